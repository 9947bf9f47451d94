"""What a pixel-resolution map costs next to the forward and to an attention-based relevance map: ms per batch of
``CompactVisionTransformer.forward`` (uvc_vit_compact_forward), of ``CompactAttributionViT.attribution`` (uvc_vit_compact_attribution) and of
``CompactPixelViT.input_grad`` (uvc_vit_compact_input_grad + uvc_unpatchify), and ms per batch of ``integrated_gradients`` at 32 steps
against 32 ``input_grad`` calls on the same (smaller) batch and against the ``input_grad`` calls at the chunks' own batch (32 / chunk calls at
chunk * batch images: the engine work integrated gradients contains) -- bf16, on one MI355X.  The mask set is compact.synthetic_masks (seeded, about
half the block MACs), as in tools/compact_eval_time.py and tools/attribution_time.py.  Device events, 20 warm-up and 100 timed calls per
arm, the arms alternated three times in one process.  The four small kernels around the engine call (uvc_amd/csrc/input_grad.hip) are timed
alone at the shapes integrated gradients gives them and at 16 times those (256 images: past the Infinity Cache), with the bytes they move
beside their times.  Every model runs in a child process of its own under a time limit; the first one that fails or runs out of time ends
the run.

    python tools/pixel_attr_time.py [tiny small base] [--iters N] [--limit SECONDS]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: embed_dim, heads, image size, batch of the three single-pass arms, batch of the integrated-gradients arms
MODELS = {"tiny": (192, 3, 224, 512, 16), "small": (384, 6, 224, 512, 16), "base": (768, 12, 224, 256, 16)}
WARMUP = 20
STEPS = 32
LIMIT = 420


def timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def rounds(arms, iters, warmup=WARMUP):
    import torch
    for fn in arms.values():              # warm-up: code objects, the workspaces
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(3):
        for k, fn in arms.items():
            ms[k].append(timed(fn, iters))
    return ms


def one(name, iters):
    import torch
    from uvc_amd import compact as CP
    from uvc_amd import ops
    from uvc_amd.compact_pixel import CompactPixelViT
    from uvc_amd.model_distilled import DistilledVisionTransformer
    D, H, S, B, Bi = MODELS[name]
    with torch.no_grad():
        torch.manual_seed(0)
        dense = DistilledVisionTransformer(enable_dist=1, embed_dim=D, num_heads=H, depth=12, img_size=S, precision="bf16", device="cuda")
        CP.apply_synthetic_masks(dense, CP.synthetic_masks(12, D, 4 * D, seed=0))
        dense.eval()
        export = CP.export_compact(dense)
        del dense
        torch.cuda.empty_cache()
        cm, pm = CP.CompactVisionTransformer(export, precision="bf16"), CompactPixelViT(export, precision="bf16")
        gen = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn(B, 3, S, S, device="cuda", generator=gen)
        xi = x[:Bi].contiguous()
        ms = rounds(dict(forward=lambda: cm(x), attribution=lambda: pm.attribution(x), input_grad=lambda: pm.input_grad(x)), iters)
        chunk = max(c for c in range(1, STEPS + 1) if STEPS % c == 0 and c * Bi <= 64)

        xc = x[:chunk * Bi].contiguous()

        def calls():
            for _ in range(STEPS):
                pm.input_grad(xi)

        def chunk_calls():
            for _ in range(STEPS // chunk):
                pm.input_grad(xc)
        ms_ig = rounds(dict(integrated_gradients=lambda: pm.integrated_gradients(xi, steps=STEPS), input_grad_x32=calls, input_grad_chunks=chunk_calls), iters)
        # the small kernels alone, at integrated gradients' shapes (Bi images, `chunk` steps a call) and at 256 images
        P = export["cfg"]["patch_size"]
        K0 = 3 * P * P
        kernels, fns = {}, {}
        for images in (Bi, 256):
            R = images * (S // P) ** 2
            rows = torch.randn(R, K0, device="cuda", generator=gen).bfloat16()
            inter = torch.empty(chunk * R, K0, dtype=torch.bfloat16, device="cuda")
            d_rows = torch.randn(chunk * R, K0, device="cuda", generator=gen)
            acc, img = torch.empty(R, K0, device="cuda"), torch.empty(images, 3, S, S, device="cuda")
            n = R * K0
            for k, fn, nbytes in (("ig_rows", lambda rows=rows, inter=inter: ops.ig_rows(rows, None, 0, chunk, STEPS, out=inter), (1 + chunk) * n * 2),
                                  ("ig_accumulate", lambda d_rows=d_rows, acc=acc: ops.ig_accumulate(d_rows, acc, False), (chunk + 2) * n * 4),
                                  ("unpatchify", lambda acc=acc, img=img: ops.unpatchify(acc, 3, S, P, out=img), 2 * n * 4),
                                  ("pixel_maps", lambda acc=acc, rows=rows: ops.pixel_maps(acc, 3, S, P, rows), n * 4 + n * 2 + (n // 3 + 2 * R) * 4)):
                fns[f"{k}@{images}"], kernels[f"{k}@{images}"] = fn, nbytes
        ms_k = rounds(fns, iters)
        best = {k: min(v) for k, v in {**ms, **ms_ig, **ms_k}.items()}
        logits, _ = cm(x)
        same, grad, target = pm.input_grad(x)
        ig = pm.integrated_gradients(xi, steps=STEPS)
        print(json.dumps(dict(model=name, batch=B, ig_batch=Bi, ig_steps=STEPS, ig_chunk=chunk, img_size=S, tokens=CP._seq(export["cfg"]), iters=iters,
                              ms={k: [round(t, 3) for t in v] for k, v in {**ms, **ms_ig}.items()},
                              spread_pct={k: round(100 * (max(v) - min(v)) / min(v), 2) for k, v in {**ms, **ms_ig}.items()},
                              attribution_over_forward=round(best["attribution"] / best["forward"], 4),
                              input_grad_over_forward=round(best["input_grad"] / best["forward"], 4),
                              input_grad_over_attribution=round(best["input_grad"] / best["attribution"], 4),
                              ig_over_32_input_grads=round(best["integrated_gradients"] / best["input_grad_x32"], 4),
                              ig_over_its_input_grads=round(best["integrated_gradients"] / best["input_grad_chunks"], 4),
                              kernels={k: dict(us=round(1e3 * best[k], 2), bytes=kernels[k], gb_per_s=round(kernels[k] / best[k] / 1e6, 1))
                                       for k in kernels},
                              logits_equal=bool(torch.equal(logits, same)), target_is_top1=bool(torch.equal(target, logits.argmax(1))),
                              grad_finite=bool(torch.isfinite(grad).all()),
                              ig_completeness_gap=float((ig[1].double().sum((1, 2, 3)) - (ig[3] - ig[4]).double()).abs().max()),
                              ig_logit_range=float((ig[3] - ig[4]).abs().max()),
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
