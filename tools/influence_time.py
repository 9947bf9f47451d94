"""What the proponent / opponent search of ``python -m uvc_amd.compact_influence explain`` costs on one MI355X, against PyTorch.

Arms, at every shape: ``fused`` -- ``ops.influence_topk`` (uvc_influence_topk: both products on the MFMA per tile, both lists on chip, neither
[nq, n] matrix written) -- and ``torch`` -- the chain a user of the library without it would run: over query chunks sized so that one
[chunk, n] float32 matrix stays under 1 GiB, ``fq @ fb.T`` (bf16 operands, float32 out), ``rq @ rb.T`` (float32), add, mul and two
``torch.topk``.  Shapes (nq, n, D, C): CIFAR-100 (10 000 test rows against the 50 000 train rows, 104 residual columns) and a batch of 256
queries against the ImageNet train bank (1 281 167 rows, 1000 columns), each at DeiT-Small (384) and DeiT-Base (768) width.  Unit-normal
features rounded to bf16, softmax residuals of random logits; k = 5.  ``residuals`` times ``ops.influence_residuals`` on the bank once more.

Device events, warm-up calls and then timed calls per arm, the arms alternated three times in one process.  The JSON line per shape carries
the ms of every round, the rounds' spread, fused / torch (below 1: the kernel wins), whether both arms list the same rows, and the kernel's
best time against its own estimates: the MFMA time 2 nq n D / 2.5 PFLOP/s (bf16) + 2 nq n Cr / 157.3 TFLOP/s (float32 MFMA), and the HBM time
of ONE pass per query tile row over the bank's bytes at 6.29 TB/s measured copy bandwidth -- the larger is the bound, and which it is is
said.  Every shape runs in a child process of its own under a time limit; the first one that fails or runs out of time ends the run.

    python tools/influence_time.py [cifar384 cifar768 in384 in768] [--iters N] [--limit SECONDS]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: nq, n, D, C, default timed calls
SHAPES = {"cifar384": (10000, 50000, 384, 100, 30), "cifar768": (10000, 50000, 768, 100, 30), "in384": (256, 1281167, 384, 1000, 10),
          "in768": (256, 1281167, 768, 1000, 10)}
K = 5
WARMUP = 3
LIMIT = 300
PEAK_BF16_TFLOPS, PEAK_F32_MFMA_TFLOPS, HBM_TBPS = 2500.0, 157.3, 6.29
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


def torch_chain(fq, fb, rq, rb, k, bias=1.0):
    import torch
    rows = max(1, GIB // (fb.shape[0] * 4))
    pos, neg = [], []
    for j in range(0, fq.shape[0], rows):
        v = torch.matmul(fq[j:j + rows], fb.T).float()
        v = (v + bias) * (rq[j:j + rows] @ rb.T)
        pos.append(torch.topk(v, k))
        neg.append(torch.topk(v, k, largest=False))
    cat = lambda lst, i: torch.cat([x[i] for x in lst])
    return (cat(pos, 0), cat(pos, 1)), (cat(neg, 0), cat(neg, 1))


def one(name, iters):
    import torch
    from uvc_amd import ops
    nq, n, D, C, default = SHAPES[name]
    iters = iters or default
    Cr = (C + 7) // 8 * 8
    g = torch.Generator(device="cuda").manual_seed(0)
    with torch.no_grad():
        fb = torch.empty(n, D, device="cuda", dtype=torch.bfloat16)
        zb = torch.empty(n, C, device="cuda")
        for j in range(0, n, 1 << 18):
            m = min(1 << 18, n - j)
            fb[j:j + m] = torch.randn(m, D, device="cuda", generator=g).bfloat16()
            zb[j:j + m] = 3 * torch.randn(m, C, device="cuda", generator=g)
        yb = torch.randint(0, C, (n,), device="cuda", generator=g)
        fq = torch.randn(nq, D, device="cuda", generator=g).bfloat16()
        zq = 3 * torch.randn(nq, C, device="cuda", generator=g)
        rb, _, _ = ops.influence_residuals(zb, yb, C, "label")
        rq, _, _ = ops.influence_residuals(zq, None, C, "pred")
        pos = (torch.empty(nq, K, device="cuda"), torch.empty(nq, K, dtype=torch.int32, device="cuda"))
        neg = (torch.empty(nq, K, device="cuda"), torch.empty(nq, K, dtype=torch.int32, device="cuda"))
        ms = rounds(dict(fused=lambda: ops.influence_topk(fq, fb, rq, rb, K, proponents=pos, opponents=neg),
                         torch=lambda: torch_chain(fq, fb, rq, rb, K)), iters)
        ms["residuals"] = [timed(lambda: ops.influence_residuals(zb, yb, C, "label", r=rb), 3) for _ in range(3)]
        (tp, tpi), (tn, tni) = torch_chain(fq, fb, rq, rb, K)
        same = float(((tpi.int() == pos[1]).float().mean() + (tni.int() == neg[1]).float().mean()) / 2)
    best = min(ms["fused"])
    t_mfma = (2.0 * nq * n * D / (PEAK_BF16_TFLOPS * 1e12) + 2.0 * nq * n * Cr / (PEAK_F32_MFMA_TFLOPS * 1e12)) * 1e3
    passes = (nq + 63) // 64
    splits = ops.influence_splits(nq, n, K)[1]
    t_hbm = passes * n * (D * 2 + Cr * 4) / (HBM_TBPS * 1e12) * 1e3
    spread = {a: round(100 * (max(v) - min(v)) / min(v), 2) for a, v in ms.items()}
    print(json.dumps(dict(shape=name, nq=nq, n=n, D=D, C=C, k=K, dtype="bf16", iters=iters, splits=splits,
                          ms={a: [round(t, 4) for t in v] for a, v in ms.items()}, spread_pct=spread, mfma_estimate_ms=round(t_mfma, 4),
                          hbm_estimate_ms=round(t_hbm, 4), bound="mfma" if t_mfma >= t_hbm else "hbm",
                          fused_over_bound=round(best / max(t_mfma, t_hbm), 3), same_rows=round(same, 4),
                          fused_over_torch=round(best / min(ms["torch"]), 4))), flush=True)


def main(argv):
    iters = int(argv[argv.index("--iters") + 1]) if "--iters" in argv else 0
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
