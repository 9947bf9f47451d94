"""Adversarial robustness of a compact model on MI355X: top-1 under an L-infinity attack of a few 1/255.

Pruning is judged on clean accuracy; the question asked next is whether it also cost robustness.  The standard figures are top-1 under

    FGSM     x' = clip(x + eps sign(dL/dx))                                              (Goodfellow, Shlens & Szegedy, ICLR 2015)
    PGD-k    x_{t+1} = clip_{x, eps}(x_t + alpha sign(dL/dx_t)), k times, optionally from a random point of the ball
                                                                                         (Madry et al., ICLR 2018)

with ``clip`` onto the eps-ball around the clean image AND the pixel range [0, 1], both stated in the normalised input the model reads
(``linf_bounds``).  ``L`` is the image's own cross-entropy, or the margin ``z_j - z_y`` to the best other label.

    python -m uvc_amd.compact_robust --compact model.compact.pt --dataset cifar10|cifar100|imagenet --data_dir D [--split test]
        [--attack fgsm|pgd] [--eps 4] [--alpha A] [--steps 10] [--random_start 0|1] [--seed 0] [--loss ce|margin] [--labels true|own]
        [--max_images N]

``CompactRobustViT.loss_grad`` goes through ``uvc_vit_compact_loss_grad`` (include/uvc_vit.h): ``uvc_vit_compact_input_grad``'s forward and
dgrad walk seeded with ``softmax(z) - onehot(y)`` (or the margin's two entries) by ``uvc_loss_seed``.  ``attack`` keeps the float32 master
rows, the clean rows and the rows in the operand type on the device: an iterate is one such call on patch rows and one ``uvc_pgd_step``
(uvc_amd/csrc/robust.hip), which makes the next forward's rows in the same pass.  ``reference_loss_grad`` and ``reference_attack`` are the
written spec in plain PyTorch autograd.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import time
from typing import Optional, Sequence

import torch

from . import compact as CP
from . import compact_tools as TL
from .compact_pixel import CompactPixelViT, _eval_logit_graph, _pick_target, check_tokens

LOSSES = ("ce", "margin")                           # ops.LOSS_KINDS: uvc_loss_seed's kind 0 / 1
ATTACKS = ("fgsm", "pgd")
LABELS = ("true", "own")


def linf_bounds(mean, std, eps255):
    """``(eps_c, lo_c, hi_c)`` float32 [C] in the normalised input ``(pixel - mean) / std``: an L-infinity radius of ``eps255 / 255`` of the
    pixel range and the range [0, 1] itself -- ``eps255 / 255 / std_c``, ``(0 - mean_c) / std_c``, ``(1 - mean_c) / std_c`` in float64, each
    rounded once to float32."""
    m, s = torch.as_tensor(mean, dtype=torch.float64).reshape(-1), torch.as_tensor(std, dtype=torch.float64).reshape(-1)
    if m.numel() != s.numel() or m.numel() == 0 or bool((s <= 0).any()):
        raise ValueError("mean and std hold one value per channel, std positive")
    return (float(eps255) / 255 / s).float(), ((0 - m) / s).float(), ((1 - m) / s).float()


def default_alpha(eps, steps):
    """The step in units of 1/255: ``eps`` for one step (FGSM), else Madry's ``2.5 eps / steps``."""
    return float(eps) if int(steps) <= 1 else 2.5 * float(eps) / int(steps)


def check_attack(eps, alpha, steps, loss, num_labels):
    """The argument refusals, before anything is read or launched: ``(eps, alpha, steps)`` with the default step filled in."""
    eps, steps = float(eps), int(steps)
    if not eps >= 0:
        raise ValueError(f"eps {eps} must be non-negative (units of 1/255)")
    if steps < 0:
        raise ValueError(f"steps {steps} must be non-negative")
    if loss not in LOSSES:
        raise ValueError(f"loss must be one of {LOSSES}, not {loss!r}")
    if loss == "margin" and num_labels is not None and int(num_labels) < 2:
        raise ValueError("the margin loss needs at least 2 labels")
    alpha = default_alpha(eps, steps) if alpha is None else float(alpha)
    if not alpha >= 0:
        raise ValueError(f"alpha {alpha} must be non-negative (units of 1/255)")
    return eps, alpha, steps


def _check_labels(labels, B, nl):
    t = torch.as_tensor(labels)
    if t.is_floating_point() or t.dtype == torch.bool:
        raise ValueError("labels hold class indices (integers)")
    t = t.detach().to(device="cpu", dtype=torch.int64).reshape(-1)
    if t.numel() != B:
        raise ValueError(f"{t.numel()} labels for a batch of {B} images")
    if int(t.min()) < 0 or int(t.max()) >= nl:
        raise ValueError(f"labels must lie in [0, {nl}) (num_labels), not {t.tolist()}")
    return t


# ---- the written spec ------------------------------------------------------------------------------------------------------------------
def _loss_of(logits, y, nl, loss):
    """the per-image loss [B] of eval logits [B, NC] (a graph) over the first nl columns"""
    z = logits[:, :nl]
    rows = torch.arange(z.shape[0], device=z.device)
    if loss == "ce":
        return torch.logsumexp(z, dim=1) - z[rows, y]
    others = z.detach().clone()
    others[rows, y] = -float("inf")
    return z[rows, others.argmax(dim=1)] - z[rows, y]          # torch's argmax: the first maximum


def reference_loss_grad(export: dict, x: torch.Tensor, labels, num_labels=None, loss="ce"):
    """``(eval logits [B, num_classes], grad [B, C, S, S], loss [B])`` in plain PyTorch autograd, in x's dtype and on x's device: ``loss`` "ce"
    ``lse(z) - z_y`` or "margin" ``z_j - z_y`` (j the first maximum over the other labels) of the eval logits z over the first ``num_labels``
    columns on ``compact._reference_walk``'s network, and ``grad = d loss_b / d x`` of every image's own loss."""
    cfg = CP.check_export(export)["cfg"]
    nl = CP.num_labels(cfg, num_labels)
    check_attack(0, None, 0, loss, nl)
    y = _check_labels(labels, x.shape[0], nl).to(x.device)
    with torch.enable_grad():
        xg = x.detach().clone().requires_grad_(True)
        logits = _eval_logit_graph(export, xg)
        L = _loss_of(logits, y, nl, loss)
        grad, = torch.autograd.grad(L.sum(), xg)
    return logits.detach(), grad, L.detach()


def _project(x, x0, d, step, eps, lo, hi):
    """uvc_pgd_step's statement on images: per-channel [1, C, 1, 1] step / eps / lo / hi in x's dtype"""
    return torch.minimum(torch.maximum(x + step * d, torch.maximum(x0 - eps, lo)), torch.minimum(x0 + eps, hi))


def reference_attack(export: dict, x: torch.Tensor, labels, num_labels=None, *, eps, alpha=None, steps=10, start=None, loss="ce", targeted=False,
                     mean, std):
    """``(x_adv, info)`` in plain PyTorch, in x's dtype: ``attack``'s iteration with ``reference_loss_grad`` for the gradient and the float32
    bounds of ``linf_bounds`` taken to x's dtype.  ``start``: None, or the random start's draw in [-1, 1) of x's shape.  ``info`` as
    ``attack``'s."""
    cfg = CP.check_export(export)["cfg"]
    nl = CP.num_labels(cfg, num_labels)
    eps, alpha, steps = check_attack(eps, alpha, steps, loss, nl)
    y = _check_labels(labels, x.shape[0], nl).to(x.device)
    view = lambda t: t.to(device=x.device, dtype=x.dtype).view(1, -1, 1, 1)
    eps_c, lo, hi = (view(t) for t in linf_bounds(mean, std, eps))
    step = view(linf_bounds(mean, std, alpha)[0]) * (-1 if targeted else 1)
    hit_of = lambda logits: _pick_target(logits, None, nl) == y
    with torch.no_grad():
        clean_logits = _eval_logit_graph(export, x)
        clean_hit, clean_loss = hit_of(clean_logits), _loss_of(clean_logits, y, nl, loss)
    cur = x.detach().clone()
    if start is not None and steps > 0:
        cur = _project(cur, x, start.to(x.dtype), eps_c, eps_c, lo, hi)
    losses, hits = [], []
    for _ in range(steps):
        logits, g, L = reference_loss_grad(export, cur, y, nl, loss)
        losses.append(L)
        hits.append(hit_of(logits))
        cur = _project(cur, x, torch.sign(g), step, eps_c, lo, hi)
    with torch.no_grad():
        logits = _eval_logit_graph(export, cur)
        losses.append(_loss_of(logits, y, nl, loss))
        hits.append(hit_of(logits))
    hit = torch.stack(hits)
    return cur, dict(loss=torch.stack(losses), hit=hit, robust=(~hit).all(0) if targeted else hit.all(0), clean_hit=clean_hit, clean_loss=clean_loss)


# ---- the module ------------------------------------------------------------------------------------------------------------------------
class CompactRobustViT(CompactPixelViT):
    """``CompactPixelViT`` plus the gradient of an attack loss at the input and the attacks built on it: ``loss_grad`` and ``attack``."""

    def _loss_grad_rows(self, x, patches, labels, num_labels, loss, d_rows=None):
        """``(logits, logits_dist or None, d_rows float32 [B * np, K0], loss float32 [B])`` of one uvc_vit_compact_loss_grad call; ``labels``:
        int32 [B] on the device."""
        from . import _lib as L
        dev = self._flat.device
        B = self._prep_patches(patches) if patches is not None else x.shape[0]
        _, _, _, npatch, K0 = self._geometry()
        self._refresh_shadows()
        io, mask = self._io(x, B, "input_grad")
        io.patches_in = L.ptr(patches)
        nc = self._export["cfg"]["num_classes"]
        logits = torch.empty(B, nc, device=dev)
        logits_dist = torch.empty(B, nc, device=dev) if self.num_tokens == 2 else None
        io.logits, io.logits_dist = L.ptr(logits), L.ptr(logits_dist)
        if d_rows is None:
            d_rows = torch.empty(B * npatch, K0, dtype=torch.float32, device=dev)
        out = torch.empty(B, dtype=torch.float32, device=dev)
        L.check(self._lib_call("uvc_vit_compact_loss_grad", C.byref(io), L.ptr(labels), num_labels, LOSSES.index(loss), L.ptr(d_rows), L.ptr(out),
                               L.cur_stream()), "uvc_vit_compact_loss_grad")
        del mask                                         # (read by the launches above: alive until they are enqueued)
        return logits, logits_dist, d_rows, out

    @torch.no_grad()
    def loss_grad(self, x=None, labels=None, num_labels=None, *, loss="ce", patches=None):
        """``(eval logits, grad, loss)``: the logits are ``forward``'s bit for bit; ``grad`` float32 [B, C, S, S] is the gradient of every
        image's own loss with respect to the normalised input and ``loss`` float32 [B] that loss (``reference_loss_grad`` is the spec).
        ``labels``: B indices in [0, num_labels), checked on the host.  ``x`` float32 [B, C, S, S], or ``patches=`` its patch rows in the
        model's dtype, as ``input_grad`` takes them: the same bits."""
        from . import ops
        if (x is None) == (patches is None):
            raise ValueError("patch rows stand in for the image batch: pass one of x / patches")
        if labels is None:
            raise ValueError("loss_grad needs labels")
        nl = CP.num_labels(self._export["cfg"], num_labels)
        check_attack(0, None, 0, loss, nl)
        if x is not None:
            x = self._prep(x)
        B = x.shape[0] if x is not None else self._prep_patches(patches)
        y = self._targets(_check_labels(labels, B, nl), B, nl)
        Cc, S, P, _, _ = self._geometry()
        with torch.cuda.device(self._flat.device):
            o, od, d_rows, out = self._loss_grad_rows(x, patches, y, nl, loss)
            grad = ops.unpatchify(d_rows, Cc, S, P)
        return (o if od is None else (o + od) / 2), grad, out

    @torch.no_grad()
    def attack(self, x, labels, *, eps, alpha=None, steps=10, random_start=False, seed=0, loss="ce", targeted=False, mean, std, num_labels=None):
        """``(x_adv float32 [B, C, S, S], info)``: FGSM (``steps=1``) or PGD-``steps`` inside the L-infinity ball of ``eps`` / 255 of the pixel
        range around ``x`` and inside the pixel range, both in the normalised input of ``mean`` / ``std`` (``linf_bounds``;
        ``reference_attack`` is the spec).  ``alpha``, the step in the same units: default ``eps`` at one step, else ``2.5 eps / steps``.
        The attack ascends ``loss`` ("ce" or "margin") of ``labels``; ``targeted=True`` descends it towards them.  ``random_start`` starts
        from ``x + eps u``, u uniform in [-1, 1) from a ``torch.Generator`` on the device seeded with ``seed``.  ``steps=0`` returns ``x``.

        ``info``: ``loss`` float32 [steps + 1, B], the loss at every iterate (iterate 0 is the -- randomly started -- input, the last one
        ``x_adv``); ``hit`` bool [steps + 1, B], whether the label is the first maximum among ``num_labels`` there (``ops.logits_target``);
        ``robust`` bool [B]: hit at every iterate (targeted: at none); ``clean_hit`` bool [B] and ``clean_loss`` float32 [B] on ``x`` itself.

        An iterate is one ``uvc_vit_compact_loss_grad`` call on patch rows and one ``uvc_pgd_step``; one plain forward scores the last."""
        from . import ops
        cfg = self._export["cfg"]
        nl = CP.num_labels(cfg, num_labels)
        eps, alpha, steps = check_attack(eps, alpha, steps, loss, nl)
        x = self._prep(x)
        B, dev = x.shape[0], self._flat.device
        y = self._targets(_check_labels(labels, B, nl), B, nl)
        Cc, S, P, npatch, K0 = self._geometry()
        eps_c, lo_c, hi_c = linf_bounds(mean, std, eps)
        step_c = linf_bounds(mean, std, alpha)[0] * (-1 if targeted else 1)
        if eps_c.numel() != Cc:
            raise ValueError(f"mean and std hold {eps_c.numel()} channels, the model reads {Cc}")

        def score(rows):
            o, od, _ = self._forward(None, patches=rows)
            hit = ops.logits_target(o if od is None else (o + od) / 2, y, nl)[1]
            return ops.loss_seed(o, y, nl, loss, logits_dist=od)[2], hit

        with torch.cuda.device(dev):
            rows0 = self._rows_of(x, ops.UVC_F32)
            rows_t = self._rows_of(x)
            if steps == 0:
                clean_loss, clean_hit = score(rows_t)
                hit = clean_hit[None].bool()
                return x, dict(loss=clean_loss[None], hit=hit, robust=~hit[0] if targeted else hit[0], clean_hit=hit[0], clean_loss=clean_loss)
            if random_start:                             # (without it iterate 0 is x itself: its loss and hit are the clean ones)
                clean_loss, clean_hit = score(rows_t)
            master = rows0.clone()
            losses = torch.empty(steps + 1, B, dtype=torch.float32, device=dev)
            hits = torch.empty(steps + 1, B, dtype=torch.int32, device=dev)
            d_rows = torch.empty(B * npatch, K0, dtype=torch.float32, device=dev)
            if random_start:
                gen = torch.Generator(device=dev).manual_seed(int(seed))
                u = torch.rand(x.shape, generator=gen, device=dev, dtype=torch.float32) * 2 - 1
                ops.pgd_step(master, rows0, self._rows_of(u, ops.UVC_F32), P, eps_c, eps_c, lo_c, hi_c, mode=1, out=master, out_t=rows_t)
            for k in range(steps):
                o, od, _, out = self._loss_grad_rows(None, rows_t, y, nl, loss, d_rows=d_rows)
                losses[k] = out
                hits[k] = ops.logits_target(o if od is None else (o + od) / 2, y, nl)[1]
                ops.pgd_step(master, rows0, d_rows, P, step_c, eps_c, lo_c, hi_c, mode=0, out=master, out_t=rows_t)
            losses[steps], hits[steps] = score(rows_t)
            if not random_start:
                clean_loss, clean_hit = losses[0], hits[0]
            x_adv = ops.unpatchify(master, Cc, S, P)
        hit = hits.bool()
        return x_adv, dict(loss=losses, hit=hit, robust=(~hit).all(0) if targeted else hit.all(0), clean_hit=clean_hit.bool(), clean_loss=clean_loss)


# ---- the command ---------------------------------------------------------------------------------------------------------------------------
def preset_stats(dataset):
    """``(mean, std)`` of the eval transform ``data.build_eval_loader`` applies to ``dataset``."""
    from . import data
    return (data.IMAGENET_MEAN, data.IMAGENET_STD) if dataset == "imagenet" else (data.CIFAR_MEAN, data.CIFAR_STD)


def attack_plan(args):
    """``(eps, alpha, steps, random_start)`` of the parsed flags, every refusal made: fgsm is one step of ``eps`` (or --alpha) from the
    image itself; pgd takes --steps, --random_start and Madry's default step."""
    if args.attack not in ATTACKS:
        raise ValueError(f"--attack must be one of {ATTACKS}, not {args.attack!r}")
    if args.labels not in LABELS:
        raise ValueError(f"--labels must be one of {LABELS}, not {args.labels!r}")
    if args.max_images is not None and int(args.max_images) < 1:
        raise ValueError(f"--max_images {args.max_images} must be positive")
    steps = 1 if args.attack == "fgsm" else args.steps
    eps, alpha, steps = check_attack(args.eps, args.alpha, steps, args.loss, None)
    return eps, alpha, steps, bool(args.random_start) and args.attack == "pgd"


def evaluate(export_or_path, args, dev=None):
    """The command's record: ``{"images", "attack", "eps", "alpha", "steps", "loss", "labels", "clean_top1", "robust_top1",
    "mean_loss_clean", "mean_loss_adv", "img_per_s"}`` plus ``compact._report``'s widths, parameters and MACs.  ``clean_top1``: the labels
    hit on the images themselves (100 with ``--labels own``); ``robust_top1``: hit at every iterate of the attack."""
    from . import ops
    eps, alpha, steps, random_start = attack_plan(args)
    export = CP.as_export(export_or_path)
    check_tokens(export)
    known = {"cifar10": 10, "cifar100": 100}.get(args.dataset)
    if known is not None:                                # the data's label set against the model's head, before any data is read
        check_attack(eps, alpha, steps, args.loss, CP.num_labels(export["cfg"], known))
    dev = TL.device(dev)
    model = CompactRobustViT(export, precision=args.precision, device=dev)
    loader, classes = TL.eval_loader(export, args, args.split)
    nl = CP.num_labels(export["cfg"], classes)
    check_attack(eps, alpha, steps, args.loss, nl)
    mean, std = preset_stats(args.dataset)
    n = clean = robust = 0
    loss_clean = loss_adv = 0.0
    with torch.cuda.device(dev):
        t0 = time.perf_counter()
        for x, y in loader:
            if args.max_images is not None and n + x.shape[0] > args.max_images:
                x, y = x[:args.max_images - n].contiguous(), y[:args.max_images - n]
            labels = y if args.labels == "true" else ops.logits_topk(model._eval_logits(x), 1, nl)[1][:, 0]
            _, info = model.attack(x, labels, eps=eps, alpha=alpha, steps=steps, random_start=random_start, seed=args.seed + n, loss=args.loss,
                                   mean=mean, std=std, num_labels=nl)
            n += int(x.shape[0])
            clean += int(info["clean_hit"].sum())
            robust += int(info["robust"].sum())
            loss_clean += float(info["clean_loss"].double().sum())
            loss_adv += float(info["loss"][-1].double().sum())
            if args.max_images is not None and n >= args.max_images:
                break
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    if n == 0:
        raise ValueError(f"the {args.split} split is empty")
    return dict(images=n, attack=args.attack, eps=eps, alpha=alpha, steps=steps, loss=args.loss, labels=args.labels, clean_top1=100.0 * clean / n,
                robust_top1=100.0 * robust / n, mean_loss_clean=loss_clean / n, mean_loss_adv=loss_adv / n, img_per_s=n / dt if dt > 0 else 0.0,
                **CP._report(export))


def build_parser():
    p = argparse.ArgumentParser(prog="python -m uvc_amd.compact_robust", description="Top-1 of a compact model under an L-infinity FGSM or PGD attack")
    p.add_argument("--compact", required=True, help="the compact file")
    TL.add_dataset_flags(p, eval_batch_size=64, split_default="test")
    p.add_argument("--attack", choices=list(ATTACKS), default="pgd", help="fgsm: one step of eps; pgd: --steps projected steps")
    p.add_argument("--eps", type=float, default=4.0, help="the L-infinity radius in units of 1/255 of the pixel range")
    p.add_argument("--alpha", type=float, default=None, help="the step in the same units; default: eps (fgsm), 2.5 eps / steps (pgd)")
    p.add_argument("--steps", type=int, default=10, help="pgd: the number of steps")
    p.add_argument("--random_start", type=int, default=0, choices=[0, 1], help="pgd: start from a uniform point of the ball")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--loss", choices=list(LOSSES), default="ce", help="ce: cross-entropy; margin: the best other logit minus the label's")
    p.add_argument("--labels", choices=list(LABELS), default="true", help="own: attack the model's own clean top-1 (unlabelled data)")
    p.add_argument("--max_images", type=int, default=None, help="stop after this many images")
    return p


def main(argv: Optional[Sequence[str]] = None):
    """One JSON line (``evaluate``'s record), which is returned.  The argument refusals -- a negative --eps or --steps, a margin loss with
    fewer than 2 labels, labels outside the model's head -- come before any image is read."""
    args = build_parser().parse_args(argv)
    attack_plan(args)
    TL.need_data(args)
    summary = evaluate(args.compact, args)
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
