"""What an attention rollout map costs next to the forward it rides on: ms per call of ``CompactVisionTransformer.forward``
(uvc_vit_compact_forward) and of ``.rollout`` (uvc_vit_compact_rollout: the same forward with qkv and lse kept per block, plus one
uvc_attention_rollout_step per attention block), bf16, on one MI355X.  The mask set is compact.synthetic_masks (seeded, about half
the block MACs), as in tools/compact_eval_time.py.  Device events, 20 warm-up and 100 timed calls per arm, the two arms alternated
three times in one process.

    python tools/rollout_time.py [tiny small base small384] [--iters N] [--method rollout|last]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from uvc_amd import compact as CP
from uvc_amd.model_distilled import DistilledVisionTransformer

# name: embed_dim, heads, image size, batch
MODELS = {"tiny": (192, 3, 224, 512), "small": (384, 6, 224, 512), "base": (768, 12, 224, 256), "small384": (384, 6, 384, 64)}
WARMUP = 20


def build(name):
    D, H, S, B = MODELS[name]
    torch.manual_seed(0)
    dense = DistilledVisionTransformer(enable_dist=1, embed_dim=D, num_heads=H, depth=12, img_size=S, precision="bf16", device="cuda")
    CP.apply_synthetic_masks(dense, CP.synthetic_masks(12, D, 4 * D, seed=0))
    dense.eval()
    export = CP.export_compact(dense)
    del dense
    torch.cuda.empty_cache()
    return B, S, export, CP.CompactVisionTransformer(export, precision="bf16")


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


@torch.no_grad()
def main(argv):
    names = [a for a in argv if a in MODELS] or list(MODELS)
    iters = int(argv[argv.index("--iters") + 1]) if "--iters" in argv else 100
    method = argv[argv.index("--method") + 1] if "--method" in argv else "rollout"
    for name in names:
        B, S, export, cm = build(name)
        x = torch.randn(B, 3, S, S, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        arms = dict(forward=lambda: cm(x), rollout=lambda: cm.rollout(x, method=method))
        for fn in arms.values():          # warm-up: code objects, both workspaces
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in arms}
        for _ in range(3):
            for k, fn in arms.items():
                ms[k].append(timed(fn, iters))
        logits, _ = cm(x)
        same, maps = cm.rollout(x, method=method)
        best = {k: min(v) for k, v in ms.items()}
        print(json.dumps(dict(model=name, batch=B, img_size=S, tokens=CP._seq(export["cfg"]), method=method, iters=iters,
                              ms={k: [round(t, 3) for t in v] for k, v in ms.items()},
                              spread_pct={k: round(100 * (max(v) - min(v)) / min(v), 2) for k, v in ms.items()},
                              rollout_over_forward=round(best["rollout"] / best["forward"], 4),
                              logits_equal=bool(torch.equal(logits, same)), map_sum_drift=float((maps.double().sum(1) - 1).abs().max()),
                              attention_blocks=sum(1 for b in export["blocks"] if b["heads"]))), flush=True)
        del cm
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main(sys.argv[1:])
