"""What a class-specific relevance map costs next to the forward and to a rollout map: ms per call of ``CompactVisionTransformer.forward``
(uvc_vit_compact_forward), of ``.rollout`` (uvc_vit_compact_rollout) and of ``CompactAttributionViT.attribution``
(uvc_vit_compact_attribution: the training forward, a dgrad-only backward with the attention backward at a value width, and one
uvc_attention_relevance_step per attention block), bf16, on one MI355X.  The mask set is compact.synthetic_masks (seeded, about half the
block MACs), as in tools/compact_eval_time.py and tools/rollout_time.py.  Device events, 20 warm-up and 100 timed calls per arm, the three
arms alternated three times in one process.  Every model runs in a child process of its own under a time limit; the first one that fails
or runs out of time ends the run.

    python tools/attribution_time.py [tiny small base] [--iters N] [--limit SECONDS]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: embed_dim, heads, image size, batch
MODELS = {"tiny": (192, 3, 224, 512), "small": (384, 6, 224, 512), "base": (768, 12, 224, 256)}
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


def one(name, iters):
    import torch
    from uvc_amd import compact as CP
    from uvc_amd.compact_attribution import CompactAttributionViT
    from uvc_amd.model_distilled import DistilledVisionTransformer
    D, H, S, B = MODELS[name]
    with torch.no_grad():
        torch.manual_seed(0)
        dense = DistilledVisionTransformer(enable_dist=1, embed_dim=D, num_heads=H, depth=12, img_size=S, precision="bf16", device="cuda")
        CP.apply_synthetic_masks(dense, CP.synthetic_masks(12, D, 4 * D, seed=0))
        dense.eval()
        export = CP.export_compact(dense)
        del dense
        torch.cuda.empty_cache()
        cm, am = CP.CompactVisionTransformer(export, precision="bf16"), CompactAttributionViT(export, precision="bf16")
        x = torch.randn(B, 3, S, S, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        arms = dict(forward=lambda: cm(x), rollout=lambda: cm.rollout(x), attribution=lambda: am.attribution(x))
        for fn in arms.values():          # warm-up: code objects, the three workspaces
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in arms}
        for _ in range(3):
            for k, fn in arms.items():
                ms[k].append(timed(fn, iters))
        logits, _ = cm(x)
        same, rel, target = am.attribution(x)
        best = {k: min(v) for k, v in ms.items()}
        ntok = 2
        print(json.dumps(dict(model=name, batch=B, img_size=S, tokens=CP._seq(export["cfg"]), iters=iters,
                              ms={k: [round(t, 3) for t in v] for k, v in ms.items()},
                              spread_pct={k: round(100 * (max(v) - min(v)) / min(v), 2) for k, v in ms.items()},
                              rollout_over_forward=round(best["rollout"] / best["forward"], 4),
                              attribution_over_forward=round(best["attribution"] / best["forward"], 4),
                              logits_equal=bool(torch.equal(logits, same)), target_is_top1=bool(torch.equal(target, logits.argmax(1))),
                              min_entry=float(rel.min()), min_readout=float(rel[:, :ntok].min()), min_row_sum=float(rel.double().sum(1).min()),
                              attention_blocks=sum(1 for b in export["blocks"] if b["heads"]))), flush=True)


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
