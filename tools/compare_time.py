"""What the device parts of ``python -m uvc_amd.compact_compare`` cost on one MI355X, against float32 PyTorch.

Arms, one shape per process:
  stats  ``ops.logits_pair_stats`` (uvc_logits_pair_stats: fourteen vectors in one read of both matrices) against what a user without it
         would run: two ``log_softmax``, ``exp``, the sums, ``argmax`` and comparisons for the ranks.  Shapes (n, C), row stride C rounded
         up to 8.
  cka    ``ops.linear_cka`` (uvc_class_moments, then uvc_center_rows + three uvc_gemm_tn per chunk) against three centred ``matmul``s.
         Shapes (n, D1, D2).

The protocol is tools/ood_time.py's: device events, 20 warm-up and 100 timed calls per arm, the arms alternated three times in one process.
The JSON line per shape carries the ms of every round, the rounds' spread, the largest difference between the arms' float results, ours /
torch, and for ``stats`` n (lda + ldb) 4 bytes over the kernel's best time in GB/s (to be read against the ``read`` rows of
profiles/r1_bw_probe_hbm_ceilings.csv; only a shape whose logits pass the 256 MiB Infinity Cache is an HBM figure).  Every shape runs in a
child process of its own under a time limit; the first one that fails or runs out of time ends the run.

    python tools/compare_time.py [p_cifar p_inval p_intrain c_inval c_intrain] [--iters N] [--chunk_rows N] [--limit SECONDS]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"p_cifar": ("stats", 10000, 100), "p_inval": ("stats", 50000, 1000), "p_intrain": ("stats", 1281167, 1000),
          "c_inval": ("cka", 50000, 384, 384), "c_intrain": ("cka", 1281167, 384, 768)}
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


def torch_pair_stats(Za, Zb, y):
    """the fourteen vectors in float32 PyTorch, the labels all inside [0, C)"""
    import torch
    la, lb = torch.log_softmax(Za, dim=1), torch.log_softmax(Zb, dim=1)
    pa, pb = la.exp(), lb.exp()
    dl = la - lb
    lm = torch.maximum(la, lb) + torch.log1p(torch.exp(-dl.abs())) - 0.6931471805599453
    ta, tb = Za.argmax(dim=1), Zb.argmax(dim=1)
    yy = y[:, None]
    cols = torch.arange(Za.shape[1], device=Za.device)[None, :]

    def rank(z, col):
        t = z.gather(1, col)
        return ((z > t) | ((z == t) & (cols < col))).sum(dim=1)
    return dict(top1_a=ta, top1_b=tb, conf_a=pa.max(dim=1)[0], conf_b=pb.max(dim=1)[0], kl_ab=(pa * dl).sum(dim=1), kl_ba=-(pb * dl).sum(dim=1),
                js=(0.5 * ((pa * (la - lm)).sum(dim=1) + (pb * (lb - lm)).sum(dim=1))).clamp_min(0.0), tv=0.5 * (pa - pb).abs().sum(dim=1),
                nll_a=-la.gather(1, yy)[:, 0], nll_b=-lb.gather(1, yy)[:, 0], rank_a=rank(Za, yy), rank_b=rank(Zb, yy),
                rank_b_top1a=rank(Zb, ta[:, None]), rank_a_top1b=rank(Za, tb[:, None]))


def one(name, iters, chunk_rows):
    import torch
    from uvc_amd import ops
    kind, n = SHAPES[name][:2]
    g = torch.Generator(device="cuda").manual_seed(0)
    if kind == "stats":
        Cc = SHAPES[name][2]
        ld = -(-Cc // 8) * 8
        Za = randn(n, ld, g, 3.0)
        Zb = Za + randn(n, ld, g, 0.5)                       # a model and a perturbed copy of it: most predictions agree
        y = torch.randint(0, Cc, (n,), device="cuda", generator=g)
        outs = {k: torch.empty(n, dtype=torch.int32 if k in ops.PAIR_STATS_INT else torch.float32, device="cuda") for k in ops.PAIR_STATS}
        # the PyTorch arm holds a handful of [n, C] temporaries: in slices of 2^17 rows it fits beside the logits of ImageNet-train
        step = 1 << 17

        def torch_arm():
            parts = [torch_pair_stats(Za[j:j + step, :Cc], Zb[j:j + step, :Cc], y[j:j + step]) for j in range(0, n, step)]
            return {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
        arms = {"ours": lambda: ops.logits_pair_stats(Za, Zb, y, n_valid=Cc, outs=outs), "torch": torch_arm}

        def diff():
            a, b = arms["ours"](), torch_arm()
            ints = all(bool((a[k].long() == b[k].long()).all()) for k in ops.PAIR_STATS_INT)
            return max(float((a[k].double() - b[k].double()).abs().max()) for k in ops.PAIR_STATS if k not in ops.PAIR_STATS_INT), ints
        extra = dict(C=Cc, ld=ld, logits_MB=round(2 * n * ld * 4 / 1e6, 1))
        rate = lambda ms: dict(logits_GBps=round(2 * n * ld * 4 / (ms * 1e-3) / 1e9, 1))
    else:
        D1, D2 = SHAPES[name][2:]
        X, Y = randn(n, D1, g), randn(n, D2, g)

        def torch_arm():
            Xc, Yc = X - X.mean(dim=0, keepdim=True), Y - Y.mean(dim=0, keepdim=True)
            kxy, kxx, kyy = Xc.T @ Yc, Xc.T @ Xc, Yc.T @ Yc
            return float(kxy.double().square().sum() / (kxx.double().square().sum().sqrt() * kyy.double().square().sum().sqrt()))
        arms = {"ours": lambda: ops.linear_cka(X, Y, chunk_rows=chunk_rows), "torch": torch_arm}
        diff = lambda: (abs(arms["ours"]() - torch_arm()), True)
        extra = dict(D1=D1, D2=D2, banks_MB=round(n * (D1 + D2) * 4 / 1e6, 1), chunk_rows=chunk_rows or ops.OOD_CHUNK_ROWS)
        rate = lambda ms: dict(TFLOPs=round(2.0 * n * (D1 * D2 + D1 * D1 + D2 * D2) / (ms * 1e-3) / 1e12, 2))
    ms = rounds(arms, iters)
    d, ints = diff()
    torch.cuda.synchronize()
    best = min(ms["ours"])
    print(json.dumps(dict(shape=name, kind=kind, n=n, iters=iters, **extra, ms={k: [round(t, 4) for t in v] for k, v in ms.items()},
                          spread_pct={k: round(100 * (max(v) - min(v)) / min(v), 2) for k, v in ms.items()}, diff_abs=float(f"{d:.3e}"),
                          integers_equal=ints, ours_over_torch=round(best / min(ms["torch"]), 4), **rate(best))), flush=True)


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
