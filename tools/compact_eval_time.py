"""Eval img/s of a pruned DeiT three ways, bf16, on one MI355X:
  dense     the full dense model (no masks),
  masked    the dense masked model with head skipping and MLP compaction on, as Stage2Trainer validates,
  compact   the exported compact model (uvc_amd/compact.py).
The mask set is compact.synthetic_masks (seeded, about half the block MACs).  Three alternating rounds, device events, warm-up.

    python tools/compact_eval_time.py [tiny small base] [--iters N] [--trace]

--trace runs the compact model alone for a few iterations (for a `rocprofv3 --kernel-trace --stats` run of its own)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from uvc_amd import compact as CP
from uvc_amd.model_distilled import DistilledVisionTransformer

MODELS = {"tiny": (192, 3, 512), "small": (384, 6, 512), "base": (768, 12, 256)}


def build(name):
    D, H, B = MODELS[name]
    torch.manual_seed(0)
    dense = DistilledVisionTransformer(enable_dist=1, embed_dim=D, num_heads=H, depth=12, precision="bf16", device="cuda")
    dense.eval()
    masked = DistilledVisionTransformer(enable_dist=1, embed_dim=D, num_heads=H, depth=12, precision="bf16", device="cuda")
    masked.load_state_dict(dense.state_dict(), strict=False)
    CP.apply_synthetic_masks(masked, CP.synthetic_masks(12, D, 4 * D, seed=0))
    masked.set_mlp_compaction()
    masked.set_head_skipping()
    masked.eval()
    export = CP.export_compact(masked)
    compact = CP.CompactVisionTransformer(export, precision="bf16")
    return B, dense, masked, compact, export


def timed(model, x, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        model(x)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


@torch.no_grad()
def main(argv):
    names = [a for a in argv if a in MODELS] or ["tiny", "small", "base"]
    iters = int(argv[argv.index("--iters") + 1]) if "--iters" in argv else 20
    for name in names:
        B, dense, masked, compact, export = build(name)
        x = torch.randn(B, 3, 224, 224, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        if "--trace" in argv:
            for _ in range(5):
                compact(x)
            torch.cuda.synchronize()
            print(json.dumps(dict(model=name, trace=True, blocks=[(len(b["heads"]), b["v_dim"], b["hidden"]) for b in export["blocks"]])))
            continue
        runs = dict(dense=dense, masked=masked, compact=compact)
        for m in runs.values():          # warm-up: code objects, workspaces
            for _ in range(3):
                m(x)
        torch.cuda.synchronize()
        ms = {k: [] for k in runs}
        for _ in range(3):
            for k, m in runs.items():
                ms[k].append(timed(m, x, iters))
        want, _ = masked(x)
        got, _ = compact(x)
        err = float((got - want).abs().max() / want.abs().max())
        print(json.dumps(dict(model=name, batch=B, img_s={k: round(B / (min(v) / 1e3)) for k, v in ms.items()},
                              ms={k: [round(t, 3) for t in v] for k, v in ms.items()}, compact_vs_masked_rel_err=err,
                              macs_full=CP.full_macs(export["cfg"]), macs_compact=CP.compact_macs(export, padded=False),
                              macs_compact_padded=CP.compact_macs(export), blocks=[(len(b["heads"]), b["v_dim"], b["hidden"]) for b in export["blocks"]])),
              flush=True)
        del dense, masked, compact
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main(sys.argv[1:])
