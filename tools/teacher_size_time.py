"""Stage-1 step time with a teacher of another size: a DeiT-Small student (bf16, 224 px) distilling from a DeiT-Small or a DeiT-Base
teacher built from --teacher-model's own config (weights: a seeded init handed over as teacher_state; no file is read).
python tools/teacher_size_time.py [batch] [steps] [repeats]
Prints ms/step and img/s for both teachers, alternating them `repeats` times over `steps` timed steps after 3 warm-up steps."""
import sys
import time

import torch

from uvc_amd.model_distilled import DistilledVisionTransformer
from uvc_amd.stage1 import CONFIGS, Stage1Trainer, default_args, model_kwargs

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 2
student = "deit_small_patch16_224"
g = torch.Generator(device="cuda").manual_seed(1)
x = torch.randn(B, 3, 224, 224, device="cuda", generator=g)
for rep in range(repeats):
    for teacher in (student, "deit_base_patch16_224"):
        torch.manual_seed(0)
        a = default_args(model_type=student, precision="bf16", train_batch_size=B, teacher_model=teacher)
        t = DistilledVisionTransformer(enable_dist=0, **model_kwargs(False, dict(CONFIGS[teacher]), a, "cuda"))
        state = {k: v.detach().cpu() for k, v in t.state_dict().items()}
        del t
        tr = Stage1Trainer(a, device="cuda", teacher_state=state)
        tr.begin_epoch(a.warmup_epochs + 1)
        y = torch.softmax(torch.randn(B, a.num_classes, device="cuda", generator=g), -1)
        for _ in range(3):
            tr.step(x, y)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            tr.step(x, y)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        print(f"repeat {rep}: student {student}, teacher {teacher} (D = {tr.teacher.embed_dim}), batch {B}: {dt * 1e3:.2f} ms/step, "
              f"{B / dt:.0f} img/s", flush=True)
        del tr
        torch.cuda.empty_cache()
