"""What the perturbation test of a relevance map costs (uvc_amd/compact_perturb.py), bf16, on one MI355X.

Part 1, the three kernels, each alone at B = 64, K = 10, DeiT 224 (196 patches of 768 elements, 1000 labels): ``ops.patch_rank`` on a
[B, 198] map, ``ops.perturb_rows`` and ``ops.logits_target`` on K * B rows.  The perturb kernel moves (1 + K) * B * np * width * sizeof(T)
bytes -- every source element read once, written K times: 212 MB here -- and is to be read against that byte count at the HBM ceilings of
profiles/r1_bw_probe_hbm_ceilings.csv (the JSON line carries the bytes, the GB/s and the best `write` and `copy` rows of that file).
212 MB fit the 256 MiB Infinity Cache, and the timed calls write the same buffer again and again, so the kernel is also timed at B = 256
(848 MB), where they cannot: that second figure is the one to hold against HBM.

Part 2, the evaluator: ``perturbation_curves`` for one order against the K forwards it contains (``model.forward(patches=rows)`` K times on
ready-made rows of the same batch); the difference is patchify, the rank, the perturbed rows, the read-out and the host work between them.

The mask set is compact.synthetic_masks (seeded, about half the block MACs), as in tools/attribution_time.py.  Device events, 20 warm-up and
100 timed calls per arm, the arms alternated three times in one process.  Every model runs in a child process of its own under a time limit;
the first one that fails or runs out of time ends the run.

    python tools/perturb_time.py [tiny small base] [--iters N] [--limit SECONDS]"""
import csv
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: embed_dim, heads, image size
MODELS = {"tiny": (192, 3, 224), "small": (384, 6, 224), "base": (768, 12, 224)}
B, K = 64, 10
BIG_B = 256
WARMUP = 20
LIMIT = 300


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


def ceilings():
    """the best total GB/s of the `write` and `copy` probes in profiles/r1_bw_probe_hbm_ceilings.csv"""
    best = {}
    with open(os.path.join(ROOT, "profiles", "r1_bw_probe_hbm_ceilings.csv"), newline="") as f:
        for row in csv.DictReader(f):
            if row["kernel"] in ("write", "copy"):
                best[row["kernel"]] = max(best.get(row["kernel"], 0.0), float(row["GBps_total"]))
    return best


def one(name, iters):
    import torch
    from uvc_amd import compact as CP
    from uvc_amd import compact_perturb as PT
    from uvc_amd import ops
    from uvc_amd.model_distilled import DistilledVisionTransformer
    D, H, S = MODELS[name]
    fmt = lambda ms: {k: [round(t, 4) for t in v] for k, v in ms.items()}
    spread = lambda ms: {k: round(100 * (max(v) - min(v)) / min(v), 2) for k, v in ms.items()}
    with torch.no_grad():
        torch.manual_seed(0)
        dense = DistilledVisionTransformer(enable_dist=1, embed_dim=D, num_heads=H, depth=12, img_size=S, precision="bf16", device="cuda")
        CP.apply_synthetic_masks(dense, CP.synthetic_masks(12, D, 4 * D, seed=0))
        dense.eval()
        export = CP.export_compact(dense)
        del dense
        torch.cuda.empty_cache()
        cm = CP.CompactVisionTransformer(export, precision="bf16")
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn(B, 3, S, S, device="cuda", generator=g)
        logits, maps = cm.rollout(x)
        target = logits.argmax(1).cpu()
        npatch, width, ntok = (S // 16) ** 2, 3 * 256, 2
        # part 1: the kernels alone
        rows = torch.empty(B * npatch, width, dtype=torch.bfloat16, device="cuda")
        ops.patchify(x, rows, 16, cm._cfg.dtype)
        rank = ops.patch_rank(maps, ntok)
        counts = torch.tensor(PT.step_counts(npatch, K), dtype=torch.int32, device="cuda")
        out = torch.empty(K * B * npatch, width, dtype=torch.bfloat16, device="cuda")
        many = torch.randn(K * B, 1000, device="cuda", generator=g)
        t32 = target.int().cuda()
        kernels = rounds(dict(patch_rank=lambda: ops.patch_rank(maps, ntok), perturb_rows=lambda: ops.perturb_rows(rows, rank, counts, B, npatch, out=out),
                              logits_target=lambda: ops.logits_target(many, t32, 1000)), iters)
        moved = (1 + K) * B * npatch * width * 2
        best = min(kernels["perturb_rows"])
        # the same kernel at BIG_B images: 848 MB, more than three times the 256 MiB Infinity Cache, so its output cannot stay there between calls
        big_rows = torch.randn(BIG_B * npatch, width, device="cuda", generator=g).bfloat16()
        big_rank = ops.patch_rank(torch.rand(BIG_B, npatch, device="cuda", generator=g))
        big_out = torch.empty(K * BIG_B * npatch, width, dtype=torch.bfloat16, device="cuda")
        big = rounds(dict(perturb_rows_big=lambda: ops.perturb_rows(big_rows, big_rank, counts, BIG_B, npatch, out=big_out)), iters)
        big_moved = (1 + K) * BIG_B * npatch * width * 2
        del big_rows, big_out
        kernels.update(big)
        # part 2: the evaluator against the K forwards it contains
        arms = rounds(dict(forwards=lambda: [cm.forward(patches=rows) for _ in range(K)],
                           curves=lambda: PT.perturbation_curves(cm, x, maps, target, steps=K)), iters)
        r = PT.perturbation_curves(cm, x, maps, target, steps=K)
        p0, _ = ops.logits_target(cm.forward(patches=rows)[0], t32)
        print(json.dumps(dict(model=name, batch=B, steps=K, img_size=S, tokens=CP._seq(export["cfg"]), iters=iters,
                              kernel_ms=fmt(kernels), kernel_spread_pct=spread(kernels), perturb_bytes=moved,
                              perturb_GBps=round(moved / (best * 1e-3) / 1e9, 1), perturb_big_batch=BIG_B, perturb_big_bytes=big_moved,
                              perturb_big_GBps=round(big_moved / (min(big["perturb_rows_big"]) * 1e-3) / 1e9, 1), ceilings_GBps=ceilings(),
                              ms=fmt(arms), spread_pct=spread(arms), curves_over_forwards=round(min(arms["curves"]) / min(arms["forwards"]), 4),
                              step0_is_the_forward=bool(torch.equal(r["prob"][:, 0].contiguous().view(torch.int32), p0.view(torch.int32))),
                              auc_prob=round(float(PT.auc(r["prob"].double().mean(0), K)), 6))), flush=True)


def main(argv):
    iters = int(argv[argv.index("--iters") + 1]) if "--iters" in argv else 100
    if "--one" in argv:
        return one(argv[argv.index("--one") + 1], iters)
    limit = int(argv[argv.index("--limit") + 1]) if "--limit" in argv else LIMIT
    for name in [a for a in argv if a in MODELS] or list(MODELS):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, "--iters", str(iters)], timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:          # a model that failed or hung: nothing more is started on the device
            print(json.dumps(dict(model=name, error=f"exit status {rc}")), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
