"""What the conformal scores of a calibration split and the prediction sets of a test split cost on one MI355X
(``python -m uvc_amd.compact_conformal fit`` / ``score`` run each once), against PyTorch.

Arms, at every shape: ``scores`` -- ``ops.conformal_scores`` (uvc_conformal_scores), randomized APS --, ``sets`` and ``sets_members`` --
``ops.conformal_sets`` (uvc_conformal_sets) without and with the membership words --, and ``torch_scores`` / ``torch_sets`` -- what a user of
the library without them would run: ``softmax`` -> ``sort`` -> ``cumsum`` -> ``scatter`` -> the label's entry, or the comparison with qhat and the
row sums, in float32, in chunks of 131 072 rows where the intermediates (five arrays of the logits' size, one of them int64) would not fit
beside each other comfortably.  The logits are float32 (a bank's type).  Shapes (n, C): a CIFAR-100 test split, the ImageNet validation set and
the ImageNet train set; the row stride is C rounded up to 8, a compact file's head width.

Device events, 20 warm-up and 100 timed calls per arm, the arms alternated three times in one process.  The JSON line per shape carries the
ms of every round, the rounds' spread, n ld 4 bytes over each kernel's best time in GB/s (to be read against the ``read`` rows of
profiles/r1_bw_probe_hbm_ceilings.csv; only a shape whose logits pass the 256 MiB Infinity Cache is an HBM figure), the compare-exchanges of
the sets kernel's sorting network, the share of rows whose set size differs between the arms, and kernel / torch per task.  Every shape runs
in a child process of its own under a time limit; the first one that fails or runs out of time ends the run.

    python tools/conformal_time.py [cifar inval intrain] [--iters N] [--limit SECONDS]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: n, C
SHAPES = {"cifar": (10000, 100), "inval": (50000, 1000), "intrain": (1281167, 1000)}
WARMUP = 20
LIMIT = 900
CHUNK = 131072
QHAT = 0.9


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
    from uvc_amd import ops
    n, Cc = SHAPES[name]
    ld = -(-Cc // 8) * 8
    g = torch.Generator(device="cuda").manual_seed(0)
    Z = torch.empty(n, ld, device="cuda")
    for j in range(0, n, 1 << 18):
        Z[j:j + (1 << 18)] = 3.0 * torch.randn(min(1 << 18, n - j), ld, device="cuda", generator=g)
    y = torch.randint(0, Cc, (n,), device="cuda", generator=g)
    u = torch.rand(n, device="cuda", generator=g)
    W = (Cc + 31) // 32
    scores, counts = torch.empty(n, device="cuda"), torch.empty(1, dtype=torch.int64, device="cuda")
    size, covered = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    members = torch.empty(n, W, dtype=torch.int32, device="cuda")
    t_scores, t_size = torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda")

    def torch_all(z, uu):
        p = torch.softmax(z, dim=1)
        ps, order = torch.sort(p, dim=1, descending=True, stable=True)
        s = ps.cumsum(1) - ps + uu[:, None] * ps
        return torch.empty_like(s).scatter_(1, order, s)

    def torch_scores():
        for j in range(0, n, CHUNK):
            s = torch_all(Z[j:j + CHUNK, :Cc], u[j:j + CHUNK])
            t_scores[j:j + CHUNK] = s.gather(1, y[j:j + CHUNK, None])[:, 0]

    def torch_sets():
        for j in range(0, n, CHUNK):
            s = torch_all(Z[j:j + CHUNK, :Cc], u[j:j + CHUNK])
            t_size[j:j + CHUNK] = (s <= QHAT).sum(1)

    arms = {"scores": lambda: ops.conformal_scores(Z, y, Cc, "aps", u, scores=scores, counts=counts),
            "sets": lambda: ops.conformal_sets(Z, QHAT, y, Cc, "aps", u, size=size, covered=covered),
            "sets_members": lambda: ops.conformal_sets(Z, QHAT, y, Cc, "aps", u, size=size, covered=covered, members=members),
            "torch_scores": torch_scores, "torch_sets": torch_sets}
    ms = rounds(arms, iters, warmup)
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    P = 1 << max(1, (Cc - 1).bit_length())
    lg = P.bit_length() - 1
    spread = {k: round(100 * (max(v) - min(v)) / min(v), 2) for k, v in ms.items()}
    gbps = {k: round(n * ld * 4 / (min(ms[k]) * 1e-3) / 1e9, 1) for k in ("scores", "sets", "sets_members")}
    print(json.dumps(dict(shape=name, n=n, C=Cc, ld=ld, iters=iters, logits_MB=round(n * ld * 4 / 1e6, 1),
                          ms={k: [round(t, 4) for t in v] for k, v in ms.items()}, spread_pct=spread, logits_GBps=gbps,
                          compare_exchanges_per_row=lg * (lg + 1) // 2 * (P // 2), pairs_per_row_counting=Cc * Cc,
                          scores_diff_max=float(f"{float((scores - t_scores).abs().max()):.3e}"),
                          size_differs_share=float(f"{float((size.to(torch.int64) != t_size).double().mean()):.3e}"),
                          kernel_over_torch=dict(scores=round(min(ms["scores"]) / min(ms["torch_scores"]), 4),
                                                 sets=round(min(ms["sets"]) / min(ms["torch_sets"]), 4),
                                                 sets_members=round(min(ms["sets_members"]) / min(ms["torch_sets"]), 4)))), flush=True)


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
