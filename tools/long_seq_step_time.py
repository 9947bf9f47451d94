"""Stage-1 step time at a long sequence: DeiT-Small at 384 px (N = 577), bf16, batch 64 by default.
python tools/long_seq_step_time.py [model_type] [img_size] [batch] [steps]
Prints img/s over `steps` timed steps after 3 warm-up steps.  Attention's share of kernel time: run under
rocprofv3 --kernel-trace --stats --output-format csv -- python tools/long_seq_step_time.py ... and sum the k_attn_* rows of the
kernel stats table."""
import sys
import time

import torch

from uvc_amd.stage1 import Stage1Trainer, default_args

model_type = sys.argv[1] if len(sys.argv) > 1 else "deit_small_patch16_224"
S = int(sys.argv[2]) if len(sys.argv) > 2 else 384
B = int(sys.argv[3]) if len(sys.argv) > 3 else 64
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 20
torch.manual_seed(0)
a = default_args(model_type=model_type, img_size=S, precision="bf16", train_batch_size=B)
tr = Stage1Trainer(a, device="cuda")
tr.begin_epoch(a.warmup_epochs + 1)
g = torch.Generator(device="cuda").manual_seed(1)
x = torch.randn(B, 3, S, S, device="cuda", generator=g)
y = torch.softmax(torch.randn(B, a.num_classes, device="cuda", generator=g), -1)
for _ in range(3):
    tr.step(x, y)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(steps):
    tr.step(x, y)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / steps
N = (S // tr.model._cfg.patch_size) ** 2 + tr.model._cfg.ntok
print(f"{model_type} img_size {S} (N = {N}) batch {B}: {dt * 1e3:.2f} ms/step, {B / dt:.0f} img/s")
