"""What the device parts of ``python -m uvc_amd.compact_ood`` cost on one MI355X, against float32 PyTorch.

Arms, one shape per process:
  scores  ``ops.ood_logit_scores`` (uvc_ood_logit_scores: four scores in one pass) against what a user without it would run:
          ``softmax().max()``, ``max()``, ``logsumexp()`` and ``(p * log_softmax).sum()``.  Shapes (n, C), row stride C rounded up to 8.
  fit     ``ops.class_gaussian_fit`` (uvc_class_moments, then uvc_center_rows + uvc_gemm_tn per chunk) against ``index_add_`` means plus
          one centred ``matmul``.  Shapes (n, D, C); read against 2 n D^2 flops and one read plus one chunked write-and-read of the bank.
  gauss   ``ops.gauss_scores`` (uvc_gemm_nt, uvc_rows_sqnorm_aug, uvc_knn_topk with k = 1) against ``z @ wmeans^T`` plus ``min``.
          Shapes (queries, D, C).

Device events, 20 warm-up and 100 timed calls per arm, the arms alternated three times in one process.  The JSON line per shape carries the
ms of every round, the rounds' spread, the largest difference between the arms' results relative to the largest result, ours / torch, and
for ``scores`` n ld 4 bytes over the kernel's best time in GB/s (to be read against the ``read`` rows of
profiles/r1_bw_probe_hbm_ceilings.csv; only a shape whose logits pass the 256 MiB Infinity Cache is an HBM figure), for ``fit`` 2 n D^2 over
its best time in TFLOP/s.  Every shape runs in a child process of its own under a time limit; the first one that fails or runs out of time
ends the run.

    python tools/ood_time.py [s_cifar s_inval s_intrain f_cifar f_in384 f_in768 g_c100 g_c1000] [--iters N] [--chunk_rows N] [--limit SECONDS]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"s_cifar": ("scores", 10000, 100), "s_inval": ("scores", 50000, 1000), "s_intrain": ("scores", 1281167, 1000),
          "f_cifar": ("fit", 50000, 384, 100), "f_in384": ("fit", 1281167, 384, 1000), "f_in768": ("fit", 1281167, 768, 1000),
          "g_c100": ("gauss", 50000, 384, 100), "g_c1000": ("gauss", 50000, 384, 1000)}
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


def randn(n, d, g, scale=1.0):
    import torch
    out = torch.empty(n, d, device="cuda")
    for j in range(0, n, 1 << 18):
        out[j:j + (1 << 18)] = scale * torch.randn(min(1 << 18, n - j), d, device="cuda", generator=g)
    return out


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def one(name, iters, chunk_rows):
    import torch
    from uvc_amd import ops
    kind, n = SHAPES[name][:2]
    g = torch.Generator(device="cuda").manual_seed(0)
    extra = {}
    if kind == "scores":
        Cc = SHAPES[name][2]
        ld = -(-Cc // 8) * 8
        Z = randn(n, ld, g, 3.0)
        Zv = Z[:, :Cc]
        outs = [torch.empty(n, device="cuda") for _ in range(4)]

        def torch_arm():
            p = torch.softmax(Zv, dim=1)
            return p.max(dim=1)[0], Zv.max(dim=1)[0], torch.logsumexp(Zv, dim=1), (p * torch.log_softmax(Zv, dim=1)).sum(dim=1)
        arms = {"ours": lambda: ops.ood_logit_scores(Z, n_valid=Cc, outs=outs), "torch": torch_arm}
        diff = lambda: max(rel(a, b) for a, b in zip(arms["ours"](), torch_arm()))
        extra = dict(C=Cc, ld=ld, logits_MB=round(n * ld * 4 / 1e6, 1))
        rate = lambda ms: dict(logits_GBps=round(n * ld * 4 / (ms * 1e-3) / 1e9, 1))
    elif kind == "fit":
        D, Cc = SHAPES[name][2:]
        X = randn(n, D, g)
        y = torch.randint(0, Cc, (n,), device="cuda", generator=g)

        def torch_arm():
            counts = torch.bincount(y, minlength=Cc)
            means = torch.zeros(Cc, D, device="cuda").index_add_(0, y, X) / counts.clamp_min(1)[:, None]
            c = X - means[y]
            return counts, means, c.T @ c
        arms = {"ours": lambda: ops.class_gaussian_fit(X, y, Cc, chunk_rows=chunk_rows), "torch": torch_arm}
        diff = lambda: max(rel(a, b) for a, b in list(zip(arms["ours"](), torch_arm()))[1:])
        extra = dict(D=D, C=Cc, bank_MB=round(n * D * 4 / 1e6, 1), chunk_rows=chunk_rows or ops.OOD_CHUNK_ROWS)
        rate = lambda ms: dict(TFLOPs=round(2.0 * n * D * D / (ms * 1e-3) / 1e12, 2))
    else:
        D, Cc = SHAPES[name][2:]
        X = randn(n, D, g)
        W = (torch.eye(D, device="cuda") + 0.05 * randn(D, D, g) * D ** -0.5).contiguous()      # a well-conditioned stand-in for L^-1
        mean0 = 0.1 * torch.randn(D, device="cuda", generator=g)
        wm = 2.0 * randn(Cc, D, g) * D ** -0.5
        counts = torch.ones(Cc, dtype=torch.int64, device="cuda")
        half = wm.square().sum(dim=1)

        def torch_arm():
            z = (X - mean0) @ W.T
            d2 = z.square().sum(dim=1, keepdim=True) - 2.0 * (z @ wm.T) + half
            return d2.min(dim=1)
        arms = {"ours": lambda: ops.gauss_scores(X, W, mean0, wm, counts), "torch": torch_arm}
        diff = lambda: rel(arms["ours"]()[0], torch_arm()[0])
        extra = dict(D=D, C=Cc)
        rate = lambda ms: {}
    ms = rounds(arms, iters)
    d = diff()
    torch.cuda.synchronize()
    best = min(ms["ours"])
    print(json.dumps(dict(shape=name, kind=kind, n=n, iters=iters, **extra, ms={k: [round(t, 4) for t in v] for k, v in ms.items()},
                          spread_pct={k: round(100 * (max(v) - min(v)) / min(v), 2) for k, v in ms.items()}, diff_rel=float(f"{d:.3e}"),
                          ours_over_torch=round(best / min(ms["torch"]), 4), **rate(best))), flush=True)


def main(argv):
    iters = int(argv[argv.index("--iters") + 1]) if "--iters" in argv else 100
    chunk = int(argv[argv.index("--chunk_rows") + 1]) if "--chunk_rows" in argv else None
    if "--one" in argv:
        return one(argv[argv.index("--one") + 1], iters, chunk)
    limit = int(argv[argv.index("--limit") + 1]) if "--limit" in argv else LIMIT
    for name in [a for a in argv if a in SHAPES] or list(SHAPES):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", name, "--iters", str(iters)] + (["--chunk_rows", str(chunk)] if chunk else [])
        try:
            rc = subprocess.run(cmd, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:          # a shape that failed or hung: nothing more is started on the device
            print(json.dumps(dict(shape=name, error=f"exit status {rc}")), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
