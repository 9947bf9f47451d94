"""Timings of the resident input path (uvc_amd/packed.py, uvc_image_prep_crops in include/uvc_data.h) against DeviceLoader.
python tools/resident_loader_time.py [--steps N] [--rounds R] [--images M] [--spare_streams K]
  1. Batches per second of ResidentLoader and DeviceLoader alone (no model): on an in-memory 32x32 dataset (batch 512, the CIFAR train
     transform to 224) and on a pack of 500x375 / 375x500 synthetic images (batch 256 at 224, the ImageNet train transform; DeviceLoader
     reads the same pack through its memmap, so neither side decodes).
  2. The three uvc_image_prep_crops launches for a batch of 512 at 224 from crop windows of a resident store, next to uvc_image_prep on
     the same crops copied out contiguously (the figure of tools/image_prep_time.py).
  3. DeiT-Tiny Stage-1 step time at batch 512 under three feeds -- synthetic batches, DeviceLoader, ResidentLoader over the in-memory
     32x32 dataset -- in one process, alternated, R rounds; every round's three numbers are printed.  --spare_streams K creates
     and uses K more streams before the trainer exists: HIP hands out hardware queues in the order of first use, so K = 0..3 moves the
     trainer's side streams over all the queues that the loaders' streams may share (DESIGN "Packed, resident datasets")."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uvc_amd import data as D  # noqa: E402
from uvc_amd import ops  # noqa: E402
from uvc_amd import packed as P  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--steps", type=int, default=20)
p.add_argument("--rounds", type=int, default=3)
p.add_argument("--images", type=int, default=2048, help="images in the 500x375 pack")
p.add_argument("--skip_step", action="store_true")
p.add_argument("--spare_streams", type=int, default=0, help="streams created and used before the trainer's: shifts which hardware queues its side streams get")
args = p.parse_args()
images = args.images
torch.manual_seed(0)
rng = np.random.default_rng(0)
CIFAR = dict(mean=D.CIFAR_MEAN, std=D.CIFAR_STD, scale=(0.05, 1.0), flip=False, num_workers=16)


def batches_per_second(loader, epoch):
    loader.set_epoch(epoch)
    n, t0 = 0, None
    for k, (xb, _) in enumerate(loader):
        if k == 0:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            continue
        n += 1
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


# ---- 1. the loaders alone
n_img = 512 * (args.steps + 3)
arr = D.ArrayDataset(rng.integers(0, 256, (n_img, 32, 32, 3), dtype=np.uint8), rng.integers(0, 1000, n_img))
dev_arr = D.DeviceLoader(arr, 512, 224, train=True, **CIFAR)
res_arr = P.ResidentLoader(arr, 512, 224, train=True, **CIFAR)
print(f"[store] in-memory 32x32 x {n_img}: {res_arr.store_bytes / 1e6:.1f} MB resident")
for r in range(args.rounds):
    d, s = batches_per_second(dev_arr, r), batches_per_second(res_arr, r)
    print(f"[loader] round {r} in-memory 32x32, batch 512 at 224: DeviceLoader {d:.1f} batches/s, ResidentLoader {s:.1f} batches/s")

with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "train" + P.EXTENSION)
    base = [(rng.integers(0, 64, (H, W, 3)) + np.linspace(0, 190, W)[None, :, None]).astype(np.uint8) for H, W in ((375, 500), (500, 375))]
    wr = P.PackWriter(path, rng.integers(0, 1000, images), source="synthetic 500x375")
    for k in range(images):
        wr.append(np.roll(base[int(k % 3 == 0)], k, axis=0))
    wr.close()
    pk = P.PackedDataset(path)
    dev_pk = D.DeviceLoader(pk, 256, 224, train=True, num_workers=16)
    t0 = time.perf_counter()
    res_pk = P.ResidentLoader(pk, 256, 224, train=True, num_workers=16)
    print(f"[store] pack of {images} 500x375 images: {res_pk.store_bytes / 1e6:.1f} MB resident, uploaded in {time.perf_counter() - t0:.2f} s")
    for r in range(args.rounds):
        d, s = batches_per_second(dev_pk, r), batches_per_second(res_pk, r)
        print(f"[loader] round {r} pack 500x375, batch 256 at 224: DeviceLoader {d:.1f} batches/s ({d * 256:.0f} img/s), "
              f"ResidentLoader {s:.1f} batches/s ({s * 256:.0f} img/s)")
    del dev_pk, res_pk, pk

# ---- 2. kernel time: crop windows of a store against the same crops copied out
B, S = 512, 224
hw = np.stack([rng.integers(300, 501, B), rng.integers(300, 501, B)], 1)
u = D.sample_uniforms(0, 0, np.arange(B), D.RRC_DRAWS)
i, j, ch, cw = D.rrc_params(hw[:, 0], hw[:, 1], u)
img_offs = np.concatenate([[0], np.cumsum(hw[:, 0] * hw[:, 1] * 3)]).astype(np.int64)
store = torch.randint(0, 256, (int(img_offs[-1]),), dtype=torch.uint8, device="cuda")
cd = np.zeros(B, ops.image_crop_desc_dtype())
cd["src_offset"], cd["img_h"], cd["img_w"] = img_offs[:-1], hw[:, 0], hw[:, 1]
cd["crop_y"], cd["crop_x"], cd["crop_h"], cd["crop_w"] = i, j, ch, cw
cd["resize_h"] = cd["resize_w"] = S
cd["flip"] = u[:, 40] < 0.5
crop_offs = np.concatenate([[0], np.cumsum(ch * cw * 3)]).astype(np.int64)
pd = np.zeros(B, ops.image_desc_dtype())
pd["src_offset"], pd["src_h"], pd["src_w"] = crop_offs[:-1], ch, cw
pd["resize_h"] = pd["resize_w"] = S
pd["flip"] = cd["flip"]
src = torch.randint(0, 256, (int(crop_offs[-1]),), dtype=torch.uint8, device="cuda")
ws = torch.empty(max(ops.image_prep_crops_workspace(cd, S, store.numel()), ops.image_prep_workspace(pd, S, src.numel())), dtype=torch.uint8,
                 device="cuda")
cdd, pdd = torch.from_numpy(cd.view(np.uint8).copy()).cuda(), torch.from_numpy(pd.view(np.uint8).copy()).cuda()
x = torch.empty(B, 3, S, S, device="cuda")


def kernel_ms(fn):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.steps


for r in range(args.rounds):
    a = kernel_ms(lambda: ops.image_prep(src, pdd, ws, x, D.IMAGENET_MEAN, D.IMAGENET_STD))
    b = kernel_ms(lambda: ops.image_prep_crops(store, cdd, ws, x, D.IMAGENET_MEAN, D.IMAGENET_STD))
    print(f"[kernel] round {r} batch {B} at {S}: uvc_image_prep {a:.3f} ms on {src.numel() / 1e6:.1f} MB of copied crops, "
          f"uvc_image_prep_crops {b:.3f} ms on windows of a {store.numel() / 1e6:.1f} MB store (3 launches each)")
del store, src, ws, x

# ---- 3. Stage-1 step under three feeds
if not args.skip_step:
    from uvc_amd.cli import build_mixup, iterate_batches
    from uvc_amd.stage1 import Stage1Trainer, default_args
    a = default_args(model_type="deit_tiny_patch16_224", img_size=224, precision="bf16", train_batch_size=512)
    for k, v in dict(mixup=0.8, cutmix=1.0, cutmix_minmax=None, mixup_prob=0.8, mixup_switch_prob=0.5, mixup_mode="batch",
                     smoothing=0.1, seed=0, steps_per_epoch=args.steps + 3).items():
        setattr(a, k, v)
    spare = [torch.cuda.Stream() for _ in range(args.spare_streams)]
    for st in spare:
        with torch.cuda.stream(st):
            torch.zeros(16, device="cuda").add_(1)
    torch.cuda.synchronize()
    tr = Stage1Trainer(a, device="cuda")
    tr.begin_epoch(a.warmup_epochs + 1)
    np.random.seed(0)
    mix = build_mixup(a)

    def timed(batches):
        t0 = None
        for k, ((xb, yb), nx) in enumerate(tr.lookahead(batches)):
            if k == 3:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            tr.step(xb, yb, next_x=nx)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    for r in range(args.rounds):
        syn = timed(iterate_batches(a, torch.device("cuda"), 0, mix, 1))
        dev = timed(D.soft_batches(dev_arr, 1 + r, mix, a.smoothing, a.num_classes))
        res = timed(D.soft_batches(res_arr, 1 + r, mix, a.smoothing, a.num_classes))
        print(f"[step] spare streams {args.spare_streams} round {r} DeiT-Tiny Stage-1 batch 512 at 224: synthetic {syn:.2f} ms/step, DeviceLoader {dev:.2f} ms/step "
              f"({(dev / syn - 1) * 100:+.1f} %), ResidentLoader {res:.2f} ms/step ({(res / syn - 1) * 100:+.1f} %)")
