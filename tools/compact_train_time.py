"""Step time and peak memory of fine-tuning a pruned DeiT two ways, bf16, on one MI355X:
  masked    Stage2Trainer on the dense masked model (MLP compaction and head skipping on, its defaults),
  compact   CompactTrainer on the exported compact model (uvc_amd/compact_train.py).
The mask set is compact.synthetic_masks (seeded, about half the block MACs), as tools/compact_eval_time.py.  Device events,
20 warm-up + 100 timed steps, the two trainers alternated three times in one process; the peak memory of each trainer is taken in a
phase of its own, with nothing else alive.

    python tools/compact_train_time.py [tiny small base] [--distill none soft] [--steps N] [--trace masked|compact]

--trace runs ONE trainer for a few steps (for a `rocprofv3 --kernel-trace --stats` run of its own)."""
import copy
import gc
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from uvc_amd import compact as CP
from uvc_amd.compact_train import CompactTrainer
from uvc_amd.model_distilled import DistilledVisionTransformer
from uvc_amd.post_train import Stage2Trainer, default_args

MODELS = {"tiny": ("deit_tiny_patch16_224", 192, 3, 512), "small": ("deit_small_patch16_224", 384, 6, 256), "base": ("deit_base_patch16_224", 768, 12, 128)}


def checkpoint(name):
    """A Stage-1 style checkpoint (bare state_dict with masks and gate logits) and its compact export."""
    _, D, H, _ = MODELS[name]
    torch.manual_seed(0)
    m = DistilledVisionTransformer(enable_dist=1, embed_dim=D, num_heads=H, depth=12, precision="bf16", device="cuda")
    CP.apply_synthetic_masks(m, CP.synthetic_masks(12, D, 4 * D, seed=0))
    state = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    export = CP.export_compact(m)
    del m
    return state, export


def make(kind, name, distill, state, export):
    model_type, _, _, B = MODELS[name]
    args = default_args(model_type=model_type, enable_deit=1, precision="bf16", train_batch_size=B, distillation_type=distill)
    if kind == "masked":
        return Stage2Trainer(args, checkpoint=copy.deepcopy(state))
    return CompactTrainer(args, export)


def run(tr, x, y, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        tr.step(x, y)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main(argv):
    names = [a for a in argv if a in MODELS] or ["tiny", "small", "base"]
    distills = [a for a in argv if a in ("none", "soft")] or ["none", "soft"]
    steps = int(argv[argv.index("--steps") + 1]) if "--steps" in argv else 100
    trace = argv[argv.index("--trace") + 1] if "--trace" in argv else None
    for name in names:
        B = MODELS[name][3]
        state, export = checkpoint(name)
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn(B, 3, 224, 224, device="cuda", generator=g)
        y = torch.softmax(torch.randn(B, 1000, device="cuda", generator=g), -1)
        for distill in distills:
            if trace:
                tr = make(trace, name, distill, state, export)
                tr.begin_epoch(0)
                run(tr, x, y, 8)
                print(json.dumps(dict(model=name, distill=distill, trace=trace)), flush=True)
                del tr
                continue
            peak = {}
            for kind in ("masked", "compact"):                     # memory: one trainer alive at a time
                gc.collect(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                tr = make(kind, name, distill, state, export)
                tr.begin_epoch(0)
                run(tr, x, y, 3)
                peak[kind] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20)
                del tr
            gc.collect(); torch.cuda.empty_cache()
            trs = {kind: make(kind, name, distill, state, export) for kind in ("masked", "compact")}
            ms = {k: [] for k in trs}
            for tr in trs.values():
                tr.begin_epoch(0)
            for _ in range(3):
                for k, tr in trs.items():
                    run(tr, x, y, 20)
                    ms[k].append(run(tr, x, y, steps))
            best = {k: min(v) for k, v in ms.items()}
            print(json.dumps(dict(model=name, batch=B, distill=distill, step_ms={k: round(v, 3) for k, v in best.items()},
                                  rounds_ms={k: [round(t, 3) for t in v] for k, v in ms.items()},
                                  compact_over_masked=round(best["compact"] / best["masked"], 4), peak_mib=peak,
                                  blocks=[(len(b["heads"]), b["v_dim"], b["hidden"]) for b in export["blocks"]])), flush=True)
            del trs
            gc.collect(); torch.cuda.empty_cache()


if __name__ == "__main__":
    main(sys.argv[1:])
