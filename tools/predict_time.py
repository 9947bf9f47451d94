"""What writing the patch rows straight from the resampler is worth, on one MI355X (README "Classify images").

Kernels: a batch of 512 synthetic 500 x 375 uint8 sources through the ImageNet eval transform to 224 px, bf16 patch rows, both filters:
  a   uvc_image_prep (float32 images) + uvc_patchify            the path every other forward takes
  b   uvc_image_prep_patches                                    the rows written by the resampler's last pass
Device events, 20 warm-up + 100 timed launches, the two arms alternated three times in one process.  The yardstick is arm a in the same
process and the margin is the spread of its own three rounds.

End to end: compact.predict img/s over the same kind of sources held in memory, fused_input on and off, alternated three times.

    python tools/predict_time.py [--launches N] [--images N] [--skip_predict]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from uvc_amd import compact as CP
from uvc_amd import data as D
from uvc_amd import ops

B, S, P, H, W = 512, 224, 16, 375, 500


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / n                       # us per call


def kernels(launches):
    rng = np.random.default_rng(0)
    src = torch.from_numpy(rng.integers(0, 256, B * H * W * 3, dtype=np.uint8)).cuda()
    rh, rw = D.resize_short_side(H, W, D.eval_resize_side(S))
    wy, wx = D.center_crop_offset(rh, rw, S)
    x = torch.empty(B, 3, S, S, device="cuda")
    rows_a, rows_b = (torch.empty(B * (S // P) ** 2, 3 * P * P, dtype=torch.bfloat16, device="cuda") for _ in range(2))
    for name in D.INTERPOLATIONS:
        filt = ops.image_filter(name)
        desc = np.zeros(B, ops.image_desc_dtype())
        desc["src_offset"] = np.arange(B, dtype=np.int64) * (H * W * 3)
        desc["src_h"], desc["src_w"], desc["resize_h"], desc["resize_w"], desc["win_y"], desc["win_x"] = H, W, rh, rw, wy, wx
        ws = torch.empty(ops.image_prep_workspace(desc, S, src.numel(), filt), dtype=torch.uint8, device="cuda")
        dd = torch.from_numpy(desc.view(np.uint8).copy()).cuda()

        def arm_a():
            ops.image_prep(src, dd, ws, x, D.IMAGENET_MEAN, D.IMAGENET_STD, filt)
            ops.patchify(x, rows_a, P, ops.UVC_BF16)

        def arm_b():
            ops.image_prep_patches(src, dd, ws, rows_b, P, S, D.IMAGENET_MEAN, D.IMAGENET_STD, filt)

        prep_only = lambda: ops.image_prep(src, dd, ws, x, D.IMAGENET_MEAN, D.IMAGENET_STD, filt)
        arms = {"a_prep_patchify": arm_a, "b_prep_patches": arm_b}
        us = {k: [] for k in arms}
        for _ in range(3):
            for k, fn in arms.items():
                timed(fn, 20)
                us[k].append(timed(fn, launches))
        timed(prep_only, 20)
        prep_us = timed(prep_only, launches)
        assert torch.equal(rows_a, rows_b)
        a, b = us["a_prep_patchify"], us["b_prep_patches"]
        print(json.dumps(dict(part="kernels", filter=name, batch=B, img_size=S, source=[W, H], dtype="bf16", launches=launches,
                              rounds_us={k: [round(t, 1) for t in v] for k, v in us.items()}, image_prep_alone_us=round(prep_us, 1),
                              a_spread_us=round(max(a) - min(a), 1), a_minus_b_us=round(min(a) - min(b), 1),
                              b_faster_beyond_spread=bool(max(b) < min(a) - (max(a) - min(a))))), flush=True)


def end_to_end(n_images):
    from uvc_amd.model_distilled import DistilledVisionTransformer
    torch.manual_seed(0)
    m = DistilledVisionTransformer(enable_dist=1, embed_dim=192, num_heads=3, depth=12, precision="bf16", device="cuda")
    CP.apply_synthetic_masks(m, CP.synthetic_masks(12, 192, 768, seed=0))
    cm = CP.CompactVisionTransformer(CP.export_compact(m), precision="bf16")
    del m
    rng = np.random.default_rng(1)
    ds = D.ArrayDataset(rng.integers(0, 256, (n_images, H, W, 3), dtype=np.uint8), np.zeros(n_images, dtype=np.int64))

    def run(fused):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = sum(1 for _ in CP.predict(cm, ds, topk=5, batch_size=B, num_workers=16, fused_input=fused))
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    run(True); run(False)                                         # warm-up: pinned slots, allocator, kernels
    rate = {"fused_input_off": [], "fused_input_on": []}
    for _ in range(3):
        rate["fused_input_off"].append(run(False))
        rate["fused_input_on"].append(run(True))
    print(json.dumps(dict(part="predict", model="deit_tiny compact (synthetic masks)", images=n_images, batch=B,
                          rounds_img_per_s={k: [round(v) for v in r] for k, r in rate.items()})), flush=True)


def main(argv):
    launches = int(argv[argv.index("--launches") + 1]) if "--launches" in argv else 100
    n_images = int(argv[argv.index("--images") + 1]) if "--images" in argv else 1024
    kernels(launches)
    if "--skip_predict" not in argv:
        end_to_end(n_images)


if __name__ == "__main__":
    main(sys.argv[1:])
