"""What the Taylor gate scores cost next to the forward and to the same dgrad walk without the dots: ms per call of
``CompactVisionTransformer.forward`` (uvc_vit_compact_forward), of ``CompactRobustViT.loss_grad`` (uvc_vit_compact_loss_grad: the training
forward, the cross-entropy seed and the dgrad-only walk down to the input) and of ``CompactGateViT.gate_grads`` (uvc_vit_compact_gate_grads:
the same forward and seed, the walk down to the lowest block with one uvc_gate_dots behind each attn.proj dgrad and one in place of each fc2
dgrad's epilogue), bf16, on one MI355X; then uvc_gate_dots alone at [B * 198, hidden] of the model, both forms, with the bytes it moves.
The mask set is compact.synthetic_masks (seeded, about half the block MACs), as in tools/attribution_time.py.  Device events, 20 warm-up and
100 timed calls per arm, the three arms alternated three times in one process.  Every model runs in a child process of its own under a
time limit; the first one that fails or runs out of time ends the run.

    python tools/prune_time.py [tiny small base] [--iters N] [--limit SECONDS]"""
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
    from uvc_amd import ops
    from uvc_amd.compact_prune import CompactGateViT, gate_table
    from uvc_amd.compact_robust import CompactRobustViT
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
        cm, rm, gm = CP.CompactVisionTransformer(export, precision="bf16"), CompactRobustViT(export, precision="bf16"), CompactGateViT(export, precision="bf16")
        gen = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn(B, 3, S, S, device="cuda", generator=gen)
        y = (torch.arange(B) * 3 + 1) % 1000
        arms = dict(forward=lambda: cm(x), loss_grad=lambda: rm.loss_grad(x, y), gate_grads=lambda: gm.gate_grads(x, y))
        for fn in arms.values():          # warm-up: code objects, the three workspaces
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in arms}
        for _ in range(3):
            for k, fn in arms.items():
                ms[k].append(timed(fn, iters))
        logits, _ = cm(x)
        same, loss, s = gm.gate_grads(x, y)
        best = {k: min(v) for k, v in ms.items()}
        # the kernel alone at the model's dense hidden width: the bytes of the plain form are M F (2 + 2), of the fused form M F (2 + 4 + 2 + 2)
        M, F = B * 198, 4 * D
        a = torch.randn(M, F, device="cuda", generator=gen).bfloat16()
        g16, g32, gp = (torch.randn(M, F, device="cuda", generator=gen) * 0.1).bfloat16(), torch.randn(M, F, device="cuda", generator=gen) * 0.1, torch.rand(M, F, device="cuda", generator=gen).bfloat16()
        out = torch.empty(B, F, device="cuda")
        dots = dict(plain=lambda: ops.gate_dots(a, g16, B, 1, out=out), fused=lambda: ops.gate_dots(a, g32, B, 1, aux=gp, out=out))
        for fn in dots.values():
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        dms = {k: [] for k in dots}
        for _ in range(3):
            for k, fn in dots.items():
                dms[k].append(timed(fn, iters))
        nbytes = dict(plain=M * F * 4, fused=M * F * 10)
        print(json.dumps(dict(model=name, batch=B, img_size=S, tokens=CP._seq(export["cfg"]), iters=iters, gates=len(gate_table(export)),
                              ms={k: [round(t, 3) for t in v] for k, v in ms.items()},
                              spread_pct={k: round(100 * (max(v) - min(v)) / min(v), 2) for k, v in ms.items()},
                              loss_grad_over_forward=round(best["loss_grad"] / best["forward"], 4),
                              gate_grads_over_forward=round(best["gate_grads"] / best["forward"], 4),
                              gate_grads_over_loss_grad=round(best["gate_grads"] / best["loss_grad"], 4),
                              logits_equal=bool(torch.equal(logits, same)), finite=bool(torch.isfinite(s).all() and torch.isfinite(loss).all()),
                              dots=dict(rows=M, width=F, us={k: [round(1e3 * t, 2) for t in v] for k, v in dms.items()}, bytes=nbytes,
                                        gb_per_s={k: round(nbytes[k] / (min(v) * 1e-3) / 1e9, 1) for k, v in dms.items()}))), flush=True)


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
