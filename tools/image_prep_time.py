"""Timings of the real-data input step (uvc_amd/data.py, include/uvc_data.h).
python tools/image_prep_time.py [--steps N] [--interpolation bilinear|bicubic] [--kernel_only]
  1. uvc_image_prep kernel time for a batch of 512 at 224 from ImageNet-like crops (synthetic uint8 sources, no decode): the three
     launches timed with events over N repeats, with the resampling filter of --interpolation (every leg uses it).
  2. Host pipeline images/s of DeviceLoader over a generated JPEG ImageFolder (500x375-ish photos) with 16 decode threads.
  3. DeiT-Tiny Stage-1 step time at batch 512 fed from an in-memory 32x32 dataset (DeviceLoader, S = 32 -> 224 resize as the CIFAR
     train transform) against the synthetic batches of --synthetic 1."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uvc_amd import data as D  # noqa: E402
from uvc_amd import ops  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--steps", type=int, default=20)
p.add_argument("--images", type=int, default=2048, help="JPEG files for the host pipeline leg")
p.add_argument("--skip_step", action="store_true")
p.add_argument("--kernel_only", action="store_true", help="leg 1 alone")
p.add_argument("--interpolation", choices=list(D.INTERPOLATIONS), default="bilinear")
args = p.parse_args()
torch.manual_seed(0)
rng = np.random.default_rng(0)
filt = ops.image_filter(args.interpolation)

# ---- 1. kernel time
B, S = 512, 224
hw = np.stack([rng.integers(300, 501, B), rng.integers(300, 501, B)], 1)
u = D.sample_uniforms(0, 0, np.arange(B), D.RRC_DRAWS)
i, j, ch, cw = D.rrc_params(hw[:, 0], hw[:, 1], u)
sizes = ch * cw * 3
offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
desc = np.zeros(B, ops.image_desc_dtype())
desc["src_offset"], desc["src_h"], desc["src_w"] = offs[:-1], ch, cw
desc["resize_h"] = desc["resize_w"] = S
desc["flip"] = u[:, 40] < 0.5
src = torch.randint(0, 256, (int(offs[-1]),), dtype=torch.uint8, device="cuda")
ws = torch.empty(ops.image_prep_workspace(desc, S, src.numel(), filt), dtype=torch.uint8, device="cuda")
dd = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
x = torch.empty(B, 3, S, S, device="cuda")
for _ in range(3):
    ops.image_prep(src, dd, ws, x, D.IMAGENET_MEAN, D.IMAGENET_STD, filt)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(args.steps):
    ops.image_prep(src, dd, ws, x, D.IMAGENET_MEAN, D.IMAGENET_STD, filt)
e1.record()
torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / args.steps
print(f"[kernel] {args.interpolation} batch {B} at {S}: {ms:.3f} ms per batch (3 launches), sources {src.numel() / 1e6:.1f} MB, "
      f"workspace {ws.numel() / 1e6:.1f} MB, output {x.numel() * 4 / 1e6:.1f} MB")
del src, ws, x
if args.kernel_only:
    sys.exit(0)

# ---- 2. host pipeline on JPEG files
with tempfile.TemporaryDirectory() as tmp:
    for k in range(args.images):
        d = os.path.join(tmp, f"c{k % 10}")
        os.makedirs(d, exist_ok=True)
        H, W = (375, 500) if k % 3 else (500, 375)
        a = (rng.integers(0, 64, (H, W, 3)) + np.linspace(0, 190, W)[None, :, None]).astype(np.uint8)
        Image.fromarray(a).save(os.path.join(d, f"{k}.JPEG"), quality=90)
    ds = D.ImageFolder(tmp)
    ld = D.DeviceLoader(ds, 256, 224, train=True, num_workers=16, interpolation=args.interpolation)
    n, t0 = 0, None
    for k, (xb, _) in enumerate(ld):
        if k == 0:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            continue
        n += len(xb)
    torch.cuda.synchronize()
    print(f"[host] JPEG ImageFolder, 16 threads, batch 256 at 224: {n / (time.perf_counter() - t0):.0f} img/s")

# ---- 3. Stage-1 step: in-memory 32x32 dataset vs synthetic batches
if not args.skip_step:
    from uvc_amd.cli import build_mixup, iterate_batches
    from uvc_amd.stage1 import Stage1Trainer, default_args
    a = default_args(model_type="deit_tiny_patch16_224", img_size=224, precision="bf16", train_batch_size=512)
    for k, v in dict(mixup=0.8, cutmix=1.0, cutmix_minmax=None, mixup_prob=0.8, mixup_switch_prob=0.5, mixup_mode="batch",
                     smoothing=0.1, seed=0, steps_per_epoch=args.steps + 3).items():
        setattr(a, k, v)
    tr = Stage1Trainer(a, device="cuda")
    tr.begin_epoch(a.warmup_epochs + 1)
    np.random.seed(0)
    mix = build_mixup(a)
    n_img = 512 * (args.steps + 3)
    arr = D.ArrayDataset(rng.integers(0, 256, (n_img, 32, 32, 3), dtype=np.uint8), rng.integers(0, 1000, n_img))
    ld = D.DeviceLoader(arr, 512, 224, train=True, mean=D.CIFAR_MEAN, std=D.CIFAR_STD, scale=(0.05, 1.0), flip=False, num_workers=16,
                        interpolation=args.interpolation)

    def timed(batches):
        t0 = None
        for k, ((xb, yb), nx) in enumerate(tr.lookahead(batches)):
            if k == 3:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            tr.step(xb, yb, next_x=nx)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps

    syn = timed(iterate_batches(a, torch.device("cuda"), 0, mix, 1))
    real = timed(D.soft_batches(ld, 1, mix, a.smoothing, a.num_classes))
    print(f"[step] DeiT-Tiny Stage-1 batch 512 at 224: synthetic {syn * 1e3:.2f} ms/step, in-memory 32x32 via DeviceLoader "
          f"{real * 1e3:.2f} ms/step ({(real / syn - 1) * 100:+.1f} %)")
