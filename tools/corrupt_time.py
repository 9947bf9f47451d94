"""What the corruption kernels of ``python -m uvc_amd.compact_corrupt`` cost on one MI355X, against PyTorch.

Arms, at every shape: each kernel of uvc_amd/csrc/corrupt.hip -- ``gaussian_noise``, ``speckle_noise``, ``impulse_noise``
(``ops.corrupt_noise``), ``brightness``, ``contrast`` (``ops.corrupt_colour``), ``gaussian_blur`` at sigma 1 and 6 (``ops.blur_separable``,
9 and 49 taps), ``defocus_blur`` at r = 3 and 10 (``ops.stencil2d``, 29 and 317 taps), ``pixelate`` at k = 2 and 6 (``ops.pixelate``) -- and
the torch arms a user without them would run: ``x + c * randn_like(x)`` (``torch_noise``), a depthwise ``F.conv2d`` on a replicate-padded
input, twice with the 1-D taps (``torch_gblur_*``) or once with the disk (``torch_defocus_*``), and ``avg_pool2d`` + ``repeat_interleave``
(``torch_pixelate_*``; 224 and 384 are multiples of 2 and 6).  The torch arms clamp nothing and draw from torch's generator.
Shapes: an eval batch of 512 at 224 x 224 and of 64 at 384 x 384, three channels, float32.

Device events, 20 warm-up and 100 timed calls per arm, the arms alternated three times in one process.  The JSON line per shape carries the
ms of every round, the rounds' spread, the bytes each kernel must move (x read once, out written once; the separable blur: twice that;
contrast: x read twice) over
its best time in GB/s -- to be read against the ``copy`` rows of profiles/r1_bw_probe_hbm_ceilings.csv; the [64, 3, 384, 384] batch (113 MB)
fits the 256 MiB Infinity Cache, so only the [512, 3, 224, 224] batch (308 MB) is an HBM figure --, for the stencils the taps per output and
the fma rate, and kernel / torch per task.  Every shape runs in a child process of its own under a time limit; the first one that fails or runs
out of time ends the run.

    python tools/corrupt_time.py [b512 b64] [--iters N] [--limit SECONDS]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"b512": (512, 3, 224, 224), "b64": (64, 3, 384, 384)}
WARMUP = 20
LIMIT = 900


def timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def rounds(arms, iters, warmup):
    """{arm: [ms, ms, ms]}: warm-up of every arm, then the arms alternated three times"""
    import torch
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(3):
        for k, fn in arms.items():
            ms[k].append(timed(fn, iters))
    return ms


def one(name, iters, warmup):
    import torch
    import torch.nn.functional as F
    from uvc_amd import compact_corrupt as CC
    from uvc_amd import ops
    from uvc_amd.compact_robust import linf_bounds, preset_stats
    shape = SHAPES[name]
    B, Cc, H, W = shape
    mean, std = preset_stats("imagenet")
    _, lo, hi = linf_bounds(mean, std, 0)
    g = torch.Generator(device="cuda").manual_seed(0)
    m, s = torch.tensor(mean, device="cuda").view(1, Cc, 1, 1), torch.tensor(std, device="cuda").view(1, Cc, 1, 1)
    x = ((torch.rand(shape, device="cuda", generator=g) - m) / s).contiguous()
    out, scratch, mu = torch.empty_like(x), torch.empty_like(x), torch.empty(B, device="cuda")
    kw = dict(mean=mean, std=std, lo=lo, hi=hi)
    gtaps = {sg: CC.gaussian_taps(sg) for sg in (1, 6)}
    disks = {r: torch.from_numpy(CC.disk_taps(r)).cuda() for r in (3, 10)}
    arms, taps = {}, {}
    for kind in CC.NOISES:
        arms[kind] = lambda kind=kind: ops.corrupt_noise(x, kind, CC.SEVERITY[kind][2], index0=0, out=out, **kw)
    arms["brightness"] = lambda: ops.corrupt_colour(x, "brightness", 0.3, out=out, **kw)
    arms["contrast"] = lambda: ops.corrupt_colour(x, "contrast", 0.2, image_mean=mu, out=out, **kw)
    for sg, t in gtaps.items():
        arms[f"gaussian_blur_s{sg}"] = lambda t=t: ops.blur_separable(x, t, lo=lo, hi=hi, scratch=scratch, out=out)
        taps[f"gaussian_blur_s{sg}"] = 2 * len(t)
    for r, t in disks.items():
        arms[f"defocus_blur_r{r}"] = lambda t=t: ops.stencil2d(x, t, lo=lo, hi=hi, out=out)
        taps[f"defocus_blur_r{r}"] = int((t != 0).sum())
    for k in (2, 6):
        arms[f"pixelate_k{k}"] = lambda k=k: ops.pixelate(x, k, lo=lo, hi=hi, out=out)

    arms["torch_noise"] = lambda: x + 0.18 * torch.randn_like(x)

    def conv(inp, w4, ph, pw):
        return F.conv2d(F.pad(inp, (pw, pw, ph, ph), mode="replicate"), w4, groups=Cc)

    for sg, t in gtaps.items():
        t = torch.from_numpy(t).cuda()
        R = len(t) // 2
        wh, wv = t.view(1, 1, 1, -1).repeat(Cc, 1, 1, 1), t.view(1, 1, -1, 1).repeat(Cc, 1, 1, 1)
        arms[f"torch_gblur_s{sg}"] = lambda wh=wh, wv=wv, R=R: conv(conv(x, wh, 0, R), wv, R, 0)
    for r, t in disks.items():
        w4 = t.view(1, 1, *t.shape).repeat(Cc, 1, 1, 1)
        arms[f"torch_defocus_r{r}"] = lambda w4=w4, r=r: conv(x, w4, r, r)
    for k in (2, 6):
        arms[f"torch_pixelate_k{k}"] = lambda k=k: F.avg_pool2d(x, k).repeat_interleave(k, dim=2).repeat_interleave(k, dim=3)

    ms = rounds(arms, iters, warmup)
    torch.cuda.synchronize()
    best = {k: min(v) for k, v in ms.items()}
    nbytes = x.numel() * 4 * 2
    moved = {k: nbytes * (2 if k.startswith("gaussian_blur") else 1.5 if k == "contrast" else 1) for k in arms if not k.startswith("torch_")}
    pairs = {"gaussian_noise": "torch_noise", "speckle_noise": "torch_noise", "gaussian_blur_s1": "torch_gblur_s1", "gaussian_blur_s6": "torch_gblur_s6",
             "defocus_blur_r3": "torch_defocus_r3", "defocus_blur_r10": "torch_defocus_r10", "pixelate_k2": "torch_pixelate_k2",
             "pixelate_k6": "torch_pixelate_k6"}
    print(json.dumps(dict(shape=name, dims=list(shape), iters=iters, batch_MB=round(x.numel() * 4 / 1e6, 1),
                          ms={k: [round(t, 4) for t in v] for k, v in ms.items()},
                          spread_pct={k: round(100 * (max(v) - min(v)) / min(v), 2) for k, v in ms.items()},
                          moved_GBps={k: round(b / (best[k] * 1e-3) / 1e9, 1) for k, b in moved.items()},
                          taps_per_output=taps, fma_per_s={k: float(f"{x.numel() * n / (best[k] * 1e-3):.3e}") for k, n in taps.items()},
                          kernel_over_torch={k: round(best[k] / best[t], 4) for k, t in pairs.items()})), flush=True)


def main(argv):
    iters = int(argv[argv.index("--iters") + 1]) if "--iters" in argv else 100
    warmup = int(argv[argv.index("--warmup") + 1]) if "--warmup" in argv else WARMUP
    if "--one" in argv:
        return one(argv[argv.index("--one") + 1], iters, warmup)
    limit = int(argv[argv.index("--limit") + 1]) if "--limit" in argv else LIMIT
    for name in [a for a in argv if a in SHAPES] or list(SHAPES):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, "--iters", str(iters), "--warmup", str(warmup)],
                                timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:          # a shape that failed or hung: nothing more is started on the device
            print(json.dumps(dict(shape=name, error=f"exit status {rc}")), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
