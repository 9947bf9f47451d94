"""What an attack costs next to the calls it is made of: ms per batch of ``CompactRobustViT.attack`` (PGD-10, eps 4, no random start) at 64
images against ten ``CompactPixelViT.input_grad`` calls plus one forward at the same batch (the parent entries: the engine work the attack
contains), ms per batch of ``loss_grad`` (uvc_vit_compact_loss_grad + uvc_unpatchify) beside ``input_grad`` (uvc_vit_compact_input_grad +
uvc_unpatchify) at the single-pass batch, and ``uvc_pgd_step`` alone at 16 and 256 images with the bytes it moves (three float32 reads, one
float32 and one bf16 write: 18 bytes an element) -- bf16, on one MI355X.  The mask set is compact.synthetic_masks (seeded, about half the
block MACs), as in tools/compact_eval_time.py and tools/pixel_attr_time.py.  Device events, 20 warm-up and 100 timed calls per arm, the arms
alternated three times in one process.  Every model runs in a child process of its own under a time limit; the first one that fails or runs
out of time ends the run.

    python tools/robust_time.py [tiny small base] [--iters N] [--limit SECONDS]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

# name: embed_dim, heads, image size, batch of the single-pass arms, batch of the attack arms
MODELS = {"tiny": (192, 3, 224, 512, 64), "small": (384, 6, 224, 512, 64), "base": (768, 12, 224, 256, 64)}
PGD_STEPS = 10
LIMIT = 540


def one(name, iters):
    import torch
    from pixel_attr_time import rounds
    from uvc_amd import compact as CP
    from uvc_amd import data, ops
    from uvc_amd.compact_robust import CompactRobustViT, linf_bounds
    from uvc_amd.model_distilled import DistilledVisionTransformer
    D, H, S, B, Ba = MODELS[name]
    mean, std = data.IMAGENET_MEAN, data.IMAGENET_STD
    with torch.no_grad():
        torch.manual_seed(0)
        dense = DistilledVisionTransformer(enable_dist=1, embed_dim=D, num_heads=H, depth=12, img_size=S, precision="bf16", device="cuda")
        CP.apply_synthetic_masks(dense, CP.synthetic_masks(12, D, 4 * D, seed=0))
        dense.eval()
        export = CP.export_compact(dense)
        del dense
        torch.cuda.empty_cache()
        rm = CompactRobustViT(export, precision="bf16")
        gen = torch.Generator(device="cuda").manual_seed(1)
        eps_c, lo, hi = (t.cuda().view(1, 3, 1, 1) for t in linf_bounds(mean, std, 4))
        x = lo + torch.rand(B, 3, S, S, device="cuda", generator=gen) * (hi - lo)           # images: every entry inside the pixel range
        labels = (torch.arange(B) % export["cfg"]["num_classes"])
        xa, la = x[:Ba].contiguous(), labels[:Ba]

        def contained():
            for _ in range(PGD_STEPS):
                rm.input_grad(xa)
            rm(xa)
        attack = lambda: rm.attack(xa, la, eps=4, steps=PGD_STEPS, mean=mean, std=std)
        ms_a = rounds(dict(pgd10=attack, input_grad_x10_plus_forward=contained), iters)
        ms_g = rounds(dict(loss_grad=lambda: rm.loss_grad(x, labels), input_grad=lambda: rm.input_grad(x)), iters)
        P = export["cfg"]["patch_size"]
        K0 = 3 * P * P
        fns, nbytes = {}, {}
        for images in (16, 256):
            R = images * (S // P) ** 2
            rows0 = torch.randn(R, K0, device="cuda", generator=gen)
            master, d = rows0.clone(), torch.randn(R, K0, device="cuda", generator=gen)
            rows_t = torch.empty(R, K0, dtype=torch.bfloat16, device="cuda")
            e, l, h = linf_bounds(mean, std, 4)
            fns[f"pgd_step@{images}"] = lambda master=master, rows0=rows0, d=d, rows_t=rows_t: ops.pgd_step(master, rows0, d, P, e / 4, e, l, h, out=master, out_t=rows_t)
            nbytes[f"pgd_step@{images}"] = R * K0 * 18
        ms_k = rounds(fns, iters)
        best = {k: min(v) for k, v in {**ms_a, **ms_g, **ms_k}.items()}
        x_adv, info = attack()
        print(json.dumps(dict(model=name, batch=B, attack_batch=Ba, pgd_steps=PGD_STEPS, img_size=S, tokens=CP._seq(export["cfg"]), iters=iters,
                              ms={k: [round(t, 3) for t in v] for k, v in {**ms_a, **ms_g}.items()},
                              spread_pct={k: round(100 * (max(v) - min(v)) / min(v), 2) for k, v in {**ms_a, **ms_g}.items()},
                              pgd10_over_its_calls=round(best["pgd10"] / best["input_grad_x10_plus_forward"], 4),
                              loss_grad_over_input_grad=round(best["loss_grad"] / best["input_grad"], 4),
                              kernels={k: dict(us=round(1e3 * best[k], 2), bytes=nbytes[k], gb_per_s=round(nbytes[k] / best[k] / 1e6, 1)) for k in fns},
                              inside_ball=bool(((x_adv <= xa + eps_c) & (x_adv >= xa - eps_c)).all()), inside_range=bool(((x_adv >= lo) & (x_adv <= hi)).all()),
                              mean_loss=[round(float(v), 4) for v in info["loss"].mean(1)], clean_top1=float(info["clean_hit"].float().mean()),
                              robust_top1=float(info["robust"].float().mean()))), flush=True)


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
