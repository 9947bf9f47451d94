"""What the nearest-neighbour search of ``python -m uvc_amd.compact_transfer knn`` costs on one MI355X, against PyTorch.

Arms, at every shape: ``fused`` -- ``ops.knn_topk`` (uvc_knn_topk: the bank streams through the MFMA, every query's top-k stays on chip) --
and ``torch`` -- what a user of the library without it would run: ``torch.topk(q @ bank.T, k)`` over query chunks sized so that the
similarity matrix of a chunk stays under 1 GiB.  Shapes: CIFAR (10 000 test against 50 000 train features), a slice of ImageNet val
against the ImageNet train bank at D = 384 and 768, and 16 queries against that bank (the split path).  Unit-norm random features, bf16.

Device events, 20 warm-up and 100 timed calls per arm, the arms alternated three times in one process.  The JSON line per shape carries
the ms of every round, the rounds' spread, 2 nq n D over the best fused time as TFLOP/s and as a share of the 2.5 PFLOP/s dense bf16 MFMA
peak, the bank's bytes over that time (the HBM stream of one pass: the bound when few queries share it), whether both arms list the
same neighbours, and fused / torch.  Every shape runs in a child process of its own under a time limit; the first one that fails or runs
out of time ends the run.

    python tools/knn_time.py [cifar in384 in768 split] [--iters N] [--limit SECONDS]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: nq, n, D, k
SHAPES = {"cifar": (10000, 50000, 384, 20), "in384": (2048, 1281167, 384, 20), "in768": (2048, 1281167, 768, 20), "split": (16, 1281167, 384, 20)}
WARMUP = 20
LIMIT = 600
PEAK_BF16_TFLOPS = 2500.0
GIB = 1 << 30


def timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def rounds(arms, iters):
    """{arm: [ms, ms, ms]}: warm-up of every arm, then the arms alternated three times"""
    import torch
    for fn in arms.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(3):
        for k, fn in arms.items():
            ms[k].append(timed(fn, iters))
    return ms


def torch_topk(q, bank, k):
    import torch
    rows = max(1, GIB // (bank.shape[0] * q.element_size()))
    s, i = zip(*[torch.topk(q[j:j + rows] @ bank.T, k) for j in range(0, q.shape[0], rows)])
    return torch.cat(s), torch.cat(i)


def one(name, iters):
    import torch
    import torch.nn.functional as F
    from uvc_amd import ops
    nq, n, D, k = SHAPES[name]
    g = torch.Generator(device="cuda").manual_seed(0)
    with torch.no_grad():
        bank = torch.empty(n, D, device="cuda", dtype=torch.bfloat16)
        for j in range(0, n, 1 << 18):                              # normalised in float32, rounded once, in pieces
            bank[j:j + (1 << 18)] = F.normalize(torch.randn(min(1 << 18, n - j), D, device="cuda", generator=g), dim=1).bfloat16()
        q = F.normalize(torch.randn(nq, D, device="cuda", generator=g), dim=1).bfloat16()
        sims, idx = torch.empty(nq, k, device="cuda"), torch.empty(nq, k, dtype=torch.int32, device="cuda")
        ms = rounds(dict(fused=lambda: ops.knn_topk(q, bank, k, sims=sims, idx=idx), torch=lambda: torch_topk(q, bank, k)), iters)
        ts, ti = torch_topk(q, bank, k)
        same = float((ti.int() == idx).float().mean())              # (the torch arm rounds the similarities to bf16: ties may differ)
    best = min(ms["fused"])
    flops = 2.0 * nq * n * D
    tf = flops / (best * 1e-3) / 1e12
    spread = {a: round(100 * (max(v) - min(v)) / min(v), 2) for a, v in ms.items()}
    print(json.dumps(dict(shape=name, nq=nq, n=n, D=D, k=k, dtype="bf16", iters=iters, splits=ops.knn_splits(nq, n, k)[1],
                          ms={a: [round(t, 4) for t in v] for a, v in ms.items()}, spread_pct=spread, fused_TFLOPs=round(tf, 1),
                          share_of_bf16_peak=round(tf / PEAK_BF16_TFLOPS, 4), bank_GBps=round(n * D * 2 / (best * 1e-3) / 1e9, 1),
                          same_neighbours=round(same, 4), fused_over_torch=round(best / min(ms["torch"]), 4))), flush=True)


def main(argv):
    iters = int(argv[argv.index("--iters") + 1]) if "--iters" in argv else 100
    if "--one" in argv:
        return one(argv[argv.index("--one") + 1], iters)
    limit = int(argv[argv.index("--limit") + 1]) if "--limit" in argv else LIMIT
    for name in [a for a in argv if a in SHAPES] or list(SHAPES):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, "--iters", str(iters)], timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:          # a shape that failed or hung: nothing more is started on the device
            print(json.dumps(dict(shape=name, error=f"exit status {rc}")), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
