"""What a two-model cascade costs on the device (uvc_amd/compact_cascade.py), bf16, batch 256, on one MI355X.

The small model is a compact DeiT-Tiny or DeiT-Small under compact.synthetic_masks (seeded, about half the block MACs, as in
tools/compact_eval_time.py), the large one a DeiT-Base at its full widths; both read the same ready-made patch rows.  Timed per small model:

    large_all         the large model on every image                    small_all     the small model on every image
    cascade_10/30/50  ``Cascade.forward(patches=rows)`` with tau set from the batch's own score quantiles to defer 10 %, 30 % and 50 %
    torch_10/30/50    the same cascade with ``torch.nonzero`` / ``index_select`` / ``torch.where`` in place of uvc_cascade_compact,
                      uvc_cascade_gather and uvc_cascade_merge (uvc_cascade_decide stays; ``nonzero`` is the chain's host synchronisation)
    large_m10/30/50   the large model alone on the m gathered images

The arithmetic to read a cascade against is ``small_all + large_m`` plus the four kernels and one 4-byte read-back: the JSON line carries
``overhead_ms`` = cascade - (small_all + large_m) for every rate, and ``saved`` = 1 - cascade / large_all.  Device events, 20 warm-up and 100
timed calls per arm, the arms alternated three times in one process.  Every small model runs in a child process of its own under a time
limit; the first one that fails or runs out of time ends the run.

    python tools/cascade_time.py [tiny small] [--iters N] [--limit SECONDS]"""
import copy
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: embed_dim, heads
MODELS = {"tiny": (192, 3), "small": (384, 6)}
LARGE = (768, 12)
B, S = 256, 224
RATES = (10, 30, 50)
WARMUP = 20
LIMIT = 600


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


def export_of(D, H, masks):
    import torch
    from uvc_amd import compact as CP
    from uvc_amd.model_distilled import DistilledVisionTransformer
    torch.manual_seed(0)
    dense = DistilledVisionTransformer(enable_dist=1, embed_dim=D, num_heads=H, depth=12, img_size=S, precision="bf16", device="cuda")
    if masks:
        CP.apply_synthetic_masks(dense, CP.synthetic_masks(12, D, 4 * D, seed=0))
    dense.eval()
    export = CP.export_compact(dense)
    del dense
    torch.cuda.empty_cache()
    return export


def one(name, iters):
    import torch
    from uvc_amd import compact as CP
    from uvc_amd import compact_cascade as CS
    from uvc_amd import ops
    fmt = lambda ms: {k: [round(t, 4) for t in v] for k, v in ms.items()}
    with torch.no_grad():
        ex_s, ex_l = export_of(*MODELS[name], masks=True), export_of(*LARGE, masks=False)
        first = CS.Cascade(ex_s, ex_l, threshold=0.0, precision="bf16")
        small, large, npi = first.small, first.large, first.patches_per_image
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn(B, 3, S, S, device="cuda", generator=g)
        rows = first.patch_rows(x)
        C = ex_s["cfg"]["num_classes"]
        s0 = ops.cascade_decide(small(patches=rows)[0], C)[0]
        order = torch.sort(s0)[0]
        arms = dict(large_all=lambda: large(patches=rows), small_all=lambda: small(patches=rows))
        counts, same = {}, {}
        for r in RATES:
            m = B * r // 100
            tau = float(order[m])                                            # the rows below the m-th smallest score are deferred
            c = copy.copy(first)                                             # the same two modules under another threshold
            c.threshold = tau
            out, source, _ = c.forward(patches=rows)
            counts[r] = c.deferred
            sub = ops.cascade_gather(rows, c.last_idx, c.deferred, npi)

            def chain(tau=tau):
                zs = small(patches=rows)[0]
                defer = ops.cascade_decide(zs, C, 1.0, "msp", tau, top1=False)[2]
                idx = torch.nonzero(defer)[:, 0]
                if not idx.numel():
                    return zs, defer
                zl = large(patches=rows.view(B, npi, -1).index_select(0, idx).reshape(idx.numel() * npi, -1))[0]
                pos = torch.cumsum(defer, 0) - 1
                return torch.where(defer[:, None] != 0, zl[pos.clamp_min(0)], zs), defer
            same[r] = bool(torch.equal(chain()[0].view(torch.int32), out.view(torch.int32)))
            arms.update({f"cascade_{r}": lambda c=c: c.forward(patches=rows), f"torch_{r}": chain, f"large_m{r}": lambda sub=sub: large(patches=sub)})
        ms = rounds(arms, iters)
        best = {k: min(v) for k, v in ms.items()}
        print(json.dumps(dict(small=name, batch=B, img_size=S, iters=iters, macs_small=CP.compact_macs(ex_s), macs_large=CP.compact_macs(ex_l),
                              deferred=counts, torch_chain_same_bits=same, ms=fmt(ms),
                              spread_pct={k: round(100 * (max(v) - min(v)) / min(v), 2) for k, v in ms.items()},
                              overhead_ms={r: round(best[f"cascade_{r}"] - best["small_all"] - best[f"large_m{r}"], 4) for r in RATES},
                              torch_over_kernels={r: round(best[f"torch_{r}"] / best[f"cascade_{r}"], 4) for r in RATES},
                              saved={r: round(1.0 - best[f"cascade_{r}"] / best["large_all"], 4) for r in RATES})), flush=True)


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
            print(json.dumps(dict(small=name, error=f"exit status {rc}")), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
