"""Perturbation tests of a compact model's relevance maps: is a map FAITHFUL, are the patches it ranks high the ones the decision rests on?

The test of Chefer, Gur & Wolf (ICCV 2021, section 4, "positive / negative perturbation"): remove patches in the order a map gives them --
most relevant first ("positive") or least relevant first ("negative") -- re-run the model at 0 %, 10 %, ... 90 % removed, and report the
curve of the target class's probability and of top-1 agreement, and its area.  A faithful map has a LOW positive and a HIGH negative area;
a seeded random order ("random") is the baseline in between.  A removed patch is +0.0 in the normalised input: the dataset's mean colour.

    python -m uvc_amd.compact_perturb --compact model.compact.pt --images PATH [PATH ...] [--methods rollout last attribution random]
        [--orders positive negative] [--steps 10] [--target INT] [--seed 0] [--output curves.jsonl]

Between the two forwards everything stays on the device: ``ops.patch_rank`` (uvc_patch_rank: the removal order of every image's patches),
``ops.perturb_rows`` (uvc_patch_rows_perturb: the K perturbed copies of the batch's patch rows) and ``ops.logits_target``
(uvc_logits_target: the target's probability and whether it is still the top-1 label).  ``reference_perturbation`` is the written spec in
plain PyTorch.
"""
from __future__ import annotations

import argparse
import os
from typing import Optional, Sequence

import torch

from . import compact as CP

ORDERS = ("positive", "negative")
RANDOM = "random"                                   # the baseline: scores drawn from a seeded generator, through the same rank kernel
PERTURB_METHODS = CP.METHODS + CP.GRAD_METHODS + (RANDOM,)
MAX_PATCHES = 1024                                  # uvc_patch_rank's limit (the engine's patch limit)


def step_counts(np: int, steps: int = 10):
    """How many patches are removed at each of the ``steps`` grid points: ``np * k // steps`` for the fractions ``k / steps``, k < steps,
    in integer arithmetic.  steps = 10: 0 %, 10 %, ... 90 %, the paper's grid."""
    np, steps = int(np), int(steps)
    if np < 1 or steps < 1:
        raise ValueError(f"step_counts: np {np} and steps {steps} must be positive")
    return [np * k // steps for k in range(steps)]


def auc(y, steps: int):
    """The area under a curve on the grid of ``step_counts``, trapezoid rule: ``(1 / steps) * sum_{k < K - 1} (y_k + y_{k+1}) / 2`` over
    the last axis of ``y`` (a sequence, an array or a tensor), in float64.  A float for one curve, an array for several."""
    import numpy as np
    a = np.asarray(y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y, dtype=np.float64)
    if a.ndim < 1 or a.shape[-1] < 1 or int(steps) < 1:
        raise ValueError("auc: y holds at least one point per curve and steps is positive")
    area = ((a[..., :-1] + a[..., 1:]) / 2).sum(axis=-1) / int(steps)
    return float(area) if area.ndim == 0 else area


def _order_flag(order):
    if order not in ORDERS:
        raise ValueError(f"order must be one of {ORDERS}, not {order!r}")
    return order == "positive"


def _counts_of(npatch, steps, counts):
    if counts is None:
        return step_counts(npatch, steps)
    counts = [int(c) for c in counts]
    if not counts or min(counts) < 0 or max(counts) > npatch:
        raise ValueError(f"counts must be a non-empty list of patch counts in [0, {npatch}], not {counts}")
    return counts


def _targets(target, B, nl):
    t = torch.as_tensor(target)
    if t.is_floating_point() or t.dtype == torch.bool:
        raise ValueError("target holds class indices (integers)")
    t = t.detach().to(device="cpu", dtype=torch.int64).reshape(-1)
    if t.numel() != B or int(t.min()) < 0 or int(t.max()) >= nl:
        raise ValueError(f"target must be {B} indices in [0, {nl}) (num_labels), not {t.tolist()}")
    return t


def _patch_scores(maps, B, npatch, ntok):
    """(maps, the column of the first patch): [B, N] over the model's tokens or [B, np] over the patches alone."""
    if maps.dim() != 2 or maps.shape[0] != B or maps.shape[1] not in (npatch, npatch + ntok):
        raise ValueError(f"maps {tuple(maps.shape)} must be [{B}, {npatch + ntok}] over the tokens or [{B}, {npatch}] over the patches")
    return maps, int(maps.shape[1] - npatch)


@torch.no_grad()
def perturbation_curves(model, x, maps, target, *, order="positive", steps=10, counts=None, num_labels=None, max_images=None):
    """The perturbation curves of one batch on the device: ``dict(prob=float32 [B, K], hit=int32 [B, K], counts=[K])`` -- per image and
    grid point the probability of the image's target class and whether it is the (first) top-1 label among ``num_labels``, with
    ``counts[k]`` patches removed in the order ``maps`` gives them (``order`` "positive": most relevant first; "negative": least).

    ``model``: a compact module with an eval forward (``CompactVisionTransformer`` or ``CompactAttributionViT``); ``x`` float32
    [B, C, S, S]; ``maps`` float32 [B, N] over the model's tokens (the readout entries take no part) or [B, np]; ``target`` B class
    indices.  ``counts`` (in [0, np]) overrides ``step_counts(np, steps)``.  ops.patchify once, ops.patch_rank, ops.perturb_rows,
    ``model.forward(patches=...)``, ops.logits_target; the perturbed rows go to the forward in chunks of whole steps with at most
    ``max_images`` images each (default B: one step per forward, and the step with count 0 is ``model.forward(patches=rows)`` bit for
    bit).  ``reference_perturbation`` is the spec."""
    from . import _lib as L
    from . import ops
    descending = _order_flag(order)
    c = model._export["cfg"]
    nl = CP.num_labels(c, num_labels)
    x = model._prep(x)
    B, P = x.shape[0], c["patch_size"]
    npatch, width = (c["img_size"] // P) ** 2, c["in_chans"] * P * P
    if npatch > MAX_PATCHES:
        raise NotImplementedError(f"perturbation curves of a model with {npatch} patches: the rank kernel takes at most {MAX_PATCHES}")
    dev = x.device
    L.require_cuda(maps)
    maps, offset = _patch_scores(maps, B, npatch, model.num_tokens)
    if maps.dtype != torch.float32 or not maps.is_contiguous():
        maps = maps.float().contiguous()
    counts = _counts_of(npatch, steps, counts)
    K = len(counts)
    max_images = B if max_images is None else int(max_images)
    if max_images < B:
        raise ValueError(f"max_images {max_images} is below the batch size {B}: the chunks are whole steps")
    per = max_images // B
    t = _targets(target, B, nl).to(device=dev, dtype=torch.int32)
    counts_dev = torch.tensor(counts, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rows = torch.empty(B * npatch, width, dtype=ops.tdtype(model._cfg.dtype), device=dev)
        ops.patchify(x, rows, P, model._cfg.dtype)
        rank = ops.patch_rank(maps, offset, descending, npatch)
        prob = torch.empty(K, B, dtype=torch.float32, device=dev)
        hit = torch.empty(K, B, dtype=torch.int32, device=dev)
        for k0 in range(0, K, per):
            k1 = min(K, k0 + per)
            logits, _ = model.forward(patches=ops.perturb_rows(rows, rank, counts_dev[k0:k1], B, npatch))
            p, h = ops.logits_target(logits, t, nl)
            prob[k0:k1], hit[k0:k1] = p.view(k1 - k0, B), h.view(k1 - k0, B)
    return dict(prob=prob.t().contiguous(), hit=hit.t().contiguous(), counts=counts)


def rank_reference(scores, descending=True):
    """What ``ops.patch_rank`` computes, on the host: int32 [B, np] from ``scores`` [B, np] taken as float32.  rank[b, p] = the number of
    patches that come before p: j before p when ``s_j > s_p`` (descending; ``<`` otherwise), or ``s_j == s_p`` and j < p; -0 equals +0, a
    NaN comes after every number, NaNs among themselves by index -- ``numpy.lexsort`` over (NaN or not, the signed score, the index)."""
    import numpy as np
    s = np.array(scores.detach().cpu().numpy() if isinstance(scores, torch.Tensor) else scores, dtype=np.float32)
    if s.ndim != 2:
        raise ValueError("rank_reference: scores must be [B, np]")
    rank = np.empty(s.shape, dtype=np.int32)
    index = np.arange(s.shape[1])
    for b, row in enumerate(s):
        nan = np.isnan(row)
        key = np.where(nan, np.float32(0), -row if descending else row) + np.float32(0)           # (-0 + 0 = +0)
        rank[b, np.lexsort((index, key, nan))] = index
    return rank


@torch.no_grad()
def reference_perturbation(export, x, maps, target, *, order="positive", steps=10, counts=None, num_labels=None):
    """The written spec of ``perturbation_curves`` in plain PyTorch, in x's dtype and on x's device:
    ``dict(prob [B, K], hit int32 [B, K], counts [K], margin [B, K], scale [K])``.  The rank is ``rank_reference`` of the float32 patch
    entries of ``maps``; at every grid point the P x P pixel blocks of the removed patches (rank below the count) are set to 0 in ``x``,
    then ``compact.reference_logits`` -- the eval logits are the mean of the two heads with a distillation token -- the softmax over the first
    ``num_labels`` columns at the target, and whether the target is their first maximum.  ``margin``: the target's logit minus the best
    other logit among the labels (what a comparison of ``hit`` across arithmetics has to look at); ``scale``: the largest absolute logit of
    each grid point's batch."""
    descending = _order_flag(order)
    cfg = CP.check_export(export)["cfg"]
    nl = CP.num_labels(cfg, num_labels)
    B, P = x.shape[0], cfg["patch_size"]
    g = cfg["img_size"] // P
    npatch, ntok = g * g, 2 if cfg["enable_dist"] else 1
    maps, offset = _patch_scores(torch.as_tensor(maps), B, npatch, ntok)
    rank = torch.from_numpy(rank_reference(maps[:, offset:], descending)).to(x.device)
    counts = _counts_of(npatch, steps, counts)
    t = _targets(target, B, nl).to(x.device)
    prob, hit, margin, scale = [], [], [], []
    for count in counts:
        removed = (rank < count).reshape(B, 1, g, g).repeat_interleave(P, dim=2).repeat_interleave(P, dim=3)
        o, od = CP.reference_logits(export, torch.where(removed, torch.zeros((), dtype=x.dtype, device=x.device), x))
        logits = (o + od) / 2
        z = logits[:, :nl]
        zt = z.gather(1, t[:, None])
        prob.append(z.softmax(dim=1).gather(1, t[:, None])[:, 0])
        cols = torch.arange(nl, device=x.device).expand(B, nl)
        first = torch.where(z == z.max(dim=1, keepdim=True).values, cols, torch.full_like(cols, nl)).min(dim=1).values
        hit.append((first == t).to(torch.int32))
        others = z.masked_fill(cols == t[:, None], float("-inf")).max(dim=1).values
        margin.append(zt[:, 0] - others)
        scale.append(logits.abs().max())
    return dict(prob=torch.stack(prob, 1), hit=torch.stack(hit, 1), counts=counts, margin=torch.stack(margin, 1), scale=torch.stack(scale))


def _check_methods(methods, orders):
    methods, orders = tuple(methods), tuple(orders)
    for m in methods:
        if m not in PERTURB_METHODS:
            raise ValueError(f"method must be one of {PERTURB_METHODS}, not {m!r}")
    for o in orders:
        _order_flag(o)
    if not methods or not orders or len(set(methods)) != len(methods) or len(set(orders)) != len(orders):
        raise ValueError("methods and orders: at least one each, none twice")
    return methods, orders


def build_modules(export, methods, precision="bf16", device=None):
    """``{"forward": the module every forward of the test runs on, "attribution": a CompactAttributionViT or None}``: ``attribution``
    needs the module with a backward and keeps its refusal of more than 256 tokens (raised here, before any file is looked at);
    ``rollout``, ``last`` and ``random`` run on a ``CompactVisionTransformer`` at any length."""
    am = cm = None
    if any(m in CP.GRAD_METHODS for m in methods):
        from .compact_attribution import CompactAttributionViT
        am = CompactAttributionViT(export, precision=precision, device=device)
    if any(m in CP.METHODS for m in methods) or am is None:
        cm = CP.CompactVisionTransformer(export, precision=precision, device=device)
    return dict(forward=cm if cm is not None else am, attribution=am)


def evaluate(export_or_path, files, *, methods=("rollout",), orders=ORDERS, steps=10, target=None, seed=0, precision="bf16", preset="imagenet",
             interpolation="bilinear", crop_pct=None, num_labels=None, batch_size=64, num_workers=8, device=None, modules=None):
    """The perturbation test of image files on a compact model (an export, or the path of a compact file): a generator.

    Per readable image and (method, order): ``{"file", "method", "order", "target", "prob": [K], "hit": [K], "auc_prob"}``; per file that
    cannot be read, once: ``{"file", "error"}``; at the end one summary per (method, order): ``{"method", "order", "images", "errors",
    "fractions", "mean_prob": [K], "accuracy": [K], "auc_prob", "auc_accuracy"}`` (curves and areas None without a readable image).

    ``methods``: "rollout" / "last" (``CompactVisionTransformer.rollout``), "attribution" (``CompactAttributionViT.attribution`` for the
    target; at most 256 tokens) and "random" (scores from a ``torch.Generator`` on the device seeded with ``seed``, through the same rank
    kernel: the baseline).  The target of an image is its own top-1 label among ``num_labels`` on the intact image, or ``target``; the
    same for every method and order.  The files go through ``FileListDataset(tolerant=True)`` and the preset's eval ``DeviceLoader`` with
    image output; ``preset`` / ``interpolation`` / ``crop_pct`` / ``num_labels`` / ``batch_size`` / ``num_workers`` are ``predict``'s.
    ``modules``: ``build_modules``' answer for this export, when the caller built it already."""
    from . import data, ops
    methods, orders = _check_methods(methods, orders)
    steps = int(steps)
    if steps < 1:
        raise ValueError(f"steps {steps} must be positive")
    if preset not in CP.PRESETS:
        raise ValueError(f"preset must be one of {CP.PRESETS}, not {preset!r}")
    export = CP.load_compact(export_or_path) if isinstance(export_or_path, (str, os.PathLike)) else CP.check_export(export_or_path)
    c = export["cfg"]
    nl = CP.num_labels(c, num_labels)
    if target is not None and not 0 <= int(target) < nl:
        raise ValueError(f"target {target} must lie in [0, {nl}) (num_labels)")
    modules = modules or build_modules(export, methods, precision, device)
    fm, am = modules["forward"], modules["attribution"]
    dev = fm._flat.device
    ds = files if hasattr(files, "load") else data.FileListDataset(files, tolerant=True)
    names = ds.paths if hasattr(ds, "paths") else list(range(len(ds)))
    errors = getattr(ds, "errors", {})
    kw = dict(mean=data.IMAGENET_MEAN, std=data.IMAGENET_STD, eval="center") if preset == "imagenet" else \
        dict(mean=data.CIFAR_MEAN, std=data.CIFAR_STD, eval="square")
    loader = data.DeviceLoader(ds, int(batch_size), c["img_size"], train=False, num_workers=num_workers, device=dev, interpolation=interpolation,
                               crop_pct=crop_pct, **kw)
    npatch, ntok = (c["img_size"] // c["patch_size"]) ** 2, fm.num_tokens
    counts = step_counts(npatch, steps)
    gen = torch.Generator(device=dev).manual_seed(int(seed))
    pairs = [(m, o) for m in methods for o in orders]
    total = {p: [torch.zeros(steps, dtype=torch.float64), torch.zeros(steps, dtype=torch.float64)] for p in pairs}
    images = nerr = first = 0
    with torch.cuda.device(dev), torch.no_grad():
        for x, _ in loader:
            B = x.shape[0]
            logits, _ = fm.forward(x)
            t = ops.logits_topk(logits, 1, nl)[1][:, 0].long() if target is None else torch.full((B,), int(target), dtype=torch.int64, device=dev)
            curves = {}
            for m in methods:
                if m == RANDOM:
                    maps = torch.rand(B, npatch, generator=gen, device=dev)
                elif m in CP.GRAD_METHODS:
                    maps = am.attribution(x, t, nl)[1]
                else:
                    maps = fm.rollout(x, method=m)[1]
                for o in orders:
                    r = perturbation_curves(fm, x, maps, t, order=o, steps=steps, num_labels=nl)
                    curves[m, o] = (r["prob"].cpu(), r["hit"].cpu())
            chosen = t.cpu().tolist()
            for b in range(B):
                i = first + b
                if i in errors:
                    nerr += 1
                    yield dict(file=names[i], error=errors[i])
                    continue
                images += 1
                for p in pairs:
                    prob, hit = curves[p][0][b], curves[p][1][b]
                    total[p][0] += prob.double()
                    total[p][1] += hit.double()
                    yield dict(file=names[i], method=p[0], order=p[1], target=chosen[b], prob=prob.tolist(), hit=hit.tolist(),
                               auc_prob=auc(prob, steps))
            first += B
    for p in pairs:
        mean = (total[p][0] / images).tolist() if images else None
        acc = (total[p][1] / images).tolist() if images else None
        yield dict(method=p[0], order=p[1], images=images, errors=nerr, fractions=[k / npatch for k in counts], mean_prob=mean, accuracy=acc,
                   auc_prob=auc(mean, steps) if images else None, auc_accuracy=auc(acc, steps) if images else None)


# ---- command line -------------------------------------------------------------------------------------------------------------
def build_parser():
    p = argparse.ArgumentParser(prog="python -m uvc_amd.compact_perturb",
                                description="Perturbation test (deletion curves and their areas) of a compact model's relevance maps")
    p.add_argument("--compact", required=True, help="the compact file")
    p.add_argument("--methods", nargs="+", choices=list(PERTURB_METHODS), default=["rollout"],
                   help="the maps put to the test; random: a seeded random order, the baseline")
    p.add_argument("--orders", nargs="+", choices=list(ORDERS), default=list(ORDERS),
                   help="positive: most relevant patches removed first (a faithful map: low area); negative: least relevant first (high area)")
    p.add_argument("--steps", type=CP._int_in(1, MAX_PATCHES, "--steps"), default=10, help="grid points: fractions k / steps removed, k < steps")
    p.add_argument("--target", type=CP._int_in(0, (1 << 20) - 1, "--target"), default=None,
                   help="the class whose probability is followed, in [0, num_labels); default: every image's own top-1 label on the intact image")
    p.add_argument("--seed", type=int, default=0, help="seed of the random baseline")
    CP.add_image_file_flags(p, topk=False, classes=False)
    return p


def main(argv: Optional[Sequence[str]] = None):
    """One JSON line per record of ``evaluate`` to --output (or stdout); returns the summaries.  With ``attribution`` among the methods a
    file with more than 256 tokens fails before any image is listed."""
    from . import data
    args = build_parser().parse_args(argv)
    methods, orders = _check_methods(args.methods, args.orders)
    dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    export = CP.load_compact(args.compact)
    modules = build_modules(export, methods, args.precision, dev)
    files = data.list_images(args.images)
    summaries = []

    def records():
        for rec in evaluate(export, files, methods=methods, orders=orders, steps=args.steps, target=args.target, seed=args.seed,
                            precision=args.precision, preset=args.preset, interpolation=args.interpolation, crop_pct=args.crop_pct,
                            num_labels=args.num_labels, batch_size=args.batch_size, num_workers=args.num_workers, modules=modules):
            if "images" in rec:
                summaries.append(rec)
            yield rec

    CP.write_records(records(), args.output)
    return summaries


if __name__ == "__main__":
    main()
