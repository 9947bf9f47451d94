"""Pixel-resolution explanations of a compact model on MI355X: the gradient of a class logit with respect to the input itself.

The maps of ``compact explain`` / ``attribute`` are attention maps: they stop at the patch grid and at the lowest block that still has
heads.  The model-agnostic baselines other explanation work measures itself against are built on the input gradient instead:

    saliency               |dy/dx|
    gradient x input       x * dy/dx
    integrated gradients   (x - x0) * mean_s dy/dx at x0 + alpha_s (x - x0), alpha_s = (s + 1/2) / S      (Sundararajan, Taly & Yan, ICML 2017)

with the completeness check ``sum IG = y(x) - y(x0)`` up to the error of the S-point midpoint rule.

    python -m uvc_amd.compact_pixel --compact model.compact.pt --images PATH [PATH ...] --method saliency|gradxinput|ig [--steps 32]
        [--baseline mean|black] [--target INT] [--output maps.jsonl] [--overlay_dir DIR] [--pixel_dir DIR]

``CompactPixelViT.input_grad`` goes through ``uvc_vit_compact_input_grad`` (include/uvc_vit.h): the training forward, the target pick and
the dgrad walk of ``uvc_vit_compact_attribution`` taken through every block, token assembly and the patch embedding.  Around it
``ops.unpatchify``, ``ops.ig_rows``, ``ops.ig_accumulate`` and ``ops.pixel_maps`` (uvc_amd/csrc/input_grad.hip) keep the S passes of
integrated gradients on the device.  ``reference_input_grad`` and ``reference_integrated_gradients`` are the written spec in plain PyTorch
autograd.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
from typing import Optional, Sequence

import torch

from . import compact as CP
from .compact_attribution import CompactAttributionViT

METHODS = ("saliency", "gradxinput", "ig")
BASELINES = ("mean", "black")
MAX_TOKENS = 256                                    # compact_attribution.MAX_TOKENS: the attention backward at a value width
MAX_CHUNK_IMAGES = 64                               # the default chunk of integrated_gradients holds at most this many interpolated images


def _check_steps(steps, chunk):
    steps = int(steps)
    if steps < 1:
        raise ValueError(f"steps {steps} must be positive")
    if chunk is not None and int(chunk) < 1:
        raise ValueError(f"chunk {chunk} must hold at least one step")
    return steps, None if chunk is None else min(int(chunk), steps)


def _baseline_image(baseline, x):
    """None (zeros: the dataset's mean colour in the normalised input), or the baseline as a tensor of x's shape, dtype and device from a
    ``[C]`` colour or a whole ``[B, C, S, S]`` batch."""
    if baseline is None:
        return None
    b = torch.as_tensor(baseline).to(device=x.device, dtype=x.dtype)
    if b.dim() == 1 and b.shape[0] == x.shape[1]:
        return b.view(1, -1, 1, 1).expand_as(x).contiguous()
    if b.shape == x.shape:
        return b.contiguous()
    raise ValueError(f"baseline {tuple(b.shape)} must be [{x.shape[1]}] (a colour) or {tuple(x.shape)}")


def black_baseline(preset):
    """The ``[C]`` baseline of a black image in the normalised input of ``preset``: ``(0 - mean) / std``."""
    from . import data
    mean, std = (data.IMAGENET_MEAN, data.IMAGENET_STD) if preset == "imagenet" else (data.CIFAR_MEAN, data.CIFAR_STD)
    return torch.tensor([-m / s for m, s in zip(mean, std)], dtype=torch.float32)


# ---- the written spec ------------------------------------------------------------------------------------------------------------------
def _eval_logit_graph(export, xg):
    cfg = export["cfg"]
    o, od, _ = CP._reference_walk(export, xg)
    return (o + od) / 2 if cfg["enable_dist"] else o


def _pick_target(logits, target, nl):
    B = logits.shape[0]
    if target is None:
        z = logits.detach()[:, :nl]
        cols = torch.arange(nl, device=z.device).expand(B, nl)
        return torch.where(z == z.max(dim=1, keepdim=True).values, cols, torch.full_like(cols, nl)).min(dim=1).values
    t = torch.as_tensor(target, dtype=torch.int64, device=logits.device).reshape(-1)
    t = t.expand(B) if t.numel() == 1 else t
    if t.numel() != B or int(t.min()) < 0 or int(t.max()) >= nl:
        raise ValueError(f"target must be {B} indices in [0, {nl}), not {t.tolist()}")
    return t.clone()


def reference_input_grad(export: dict, x: torch.Tensor, target=None, num_labels=None):
    """``(grad [B, C, S, S], target int64 [B], eval logits [B, num_classes])`` in plain PyTorch autograd, in x's dtype and on x's device:
    ``grad = dy/dx`` of ``y = eval logit of class target`` (``head(cls)[t]``, or the mean of the two heads with the distillation token) on
    ``compact._reference_walk``'s network.  ``target``: an int, or B indices; None: the first maximum of the eval logits over the first
    ``num_labels`` columns (default num_classes)."""
    cfg = CP.check_export(export)["cfg"]
    nl = CP.num_labels(cfg, num_labels)
    with torch.enable_grad():
        xg = x.detach().clone().requires_grad_(True)
        logits = _eval_logit_graph(export, xg)
        t = _pick_target(logits, target, nl)
        grad, = torch.autograd.grad(logits.gather(1, t[:, None]).sum(), xg)
    return grad, t, logits.detach()


def reference_integrated_gradients(export: dict, x: torch.Tensor, target=None, num_labels=None, baseline=None, steps=32):
    """``(ig [B, C, S, S], target int64 [B], y [B], y_baseline [B])`` in plain PyTorch, in x's dtype: the target is fixed by one plain pass
    on ``x`` (as ``reference_input_grad`` picks it), then ``ig = (x - x0) * (1 / steps) sum_s dy/dx(x0 + alpha_s (x - x0))`` with the
    midpoint rule ``alpha_s = (s + 1/2) / steps``, s ascending.  ``baseline``: None (zeros), a ``[C]`` colour or ``[B, C, S, S]``.
    ``y`` / ``y_baseline``: the target's eval logit at ``x`` / at the baseline; ``ig.sum((1, 2, 3))`` tends to their difference as steps grow."""
    cfg = CP.check_export(export)["cfg"]
    nl = CP.num_labels(cfg, num_labels)
    steps, _ = _check_steps(steps, None)
    x0 = _baseline_image(baseline, x)
    x0 = torch.zeros_like(x) if x0 is None else x0
    with torch.no_grad():
        logits = _eval_logit_graph(export, x)
        t = _pick_target(logits, target, nl)
        y = logits.gather(1, t[:, None])[:, 0]
        y0 = _eval_logit_graph(export, x0).gather(1, t[:, None])[:, 0]
    acc = torch.zeros_like(x)
    for s in range(steps):
        alpha = (s + 0.5) / steps
        acc = acc + reference_input_grad(export, x0 + alpha * (x - x0), t, nl)[0]
    return (x - x0) * acc / steps, t, y, y0


# ---- the module ------------------------------------------------------------------------------------------------------------------------
class CompactPixelViT(CompactAttributionViT):
    """``CompactAttributionViT`` plus the gradient of a class logit at the input: ``input_grad``, ``integrated_gradients`` and
    ``pixel_maps``.  ``model(x)`` and ``model.attribution`` are the base class's."""

    def _geometry(self):
        c = self._export["cfg"]
        P = c["patch_size"]
        return c["in_chans"], c["img_size"], P, (c["img_size"] // P) ** 2, c["in_chans"] * P * P

    def _rows_of(self, img, dtype=None):
        """ops.patchify of a float32 image batch, in the model's operand type (or float32)."""
        from . import ops
        _, _, P, npatch, K0 = self._geometry()
        code = self._cfg.dtype if dtype is None else dtype
        rows = torch.empty(img.shape[0] * npatch, K0, dtype=ops.tdtype(code), device=img.device)
        ops.patchify(img, rows, P, code)
        return rows

    def _input_grad_rows(self, x, patches, given, num_labels):
        """``(logits, logits_dist or None, d_rows float32 [B * np, K0], target int32 [B])`` of one uvc_vit_compact_input_grad call; ``given``:
        int32 device targets or None."""
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
        d_rows = torch.empty(B * npatch, K0, dtype=torch.float32, device=dev)
        chosen = torch.empty(B, dtype=torch.int32, device=dev)
        L.check(self._lib_call("uvc_vit_compact_input_grad", C.byref(io), L.ptr(given), num_labels, L.ptr(d_rows), L.ptr(chosen), L.cur_stream()),
                "uvc_vit_compact_input_grad")
        del mask                                         # (read by the launches above: alive until they are enqueued)
        return logits, logits_dist, d_rows, chosen

    @torch.no_grad()
    def input_grad(self, x=None, target=None, num_labels=None, *, patches=None):
        """``(eval logits, grad, target)``: the logits are ``forward``'s bit for bit; ``grad`` float32 [B, C, S, S] is the gradient of the
        target's eval logit with respect to the normalised input (``reference_input_grad`` is the spec); ``target`` int64 [B] is the class
        explained, given and checked as ``attribution`` takes it, or the first maximum of the eval logits over the first ``num_labels``
        columns.  ``x`` float32 [B, C, S, S], or ``patches=`` its patch rows in the model's dtype (ops.patchify's layout), as ``forward``
        takes them: the same gradient bits."""
        from . import ops
        if (x is None) == (patches is None):
            raise ValueError("patch rows stand in for the image batch: pass one of x / patches")
        nl = CP.num_labels(self._export["cfg"], num_labels)
        if x is not None:
            x = self._prep(x)
        B = x.shape[0] if x is not None else self._prep_patches(patches)
        given = None if target is None else self._targets(target, B, nl)
        Cc, S, P, _, _ = self._geometry()
        with torch.cuda.device(self._flat.device):
            o, od, d_rows, chosen = self._input_grad_rows(x, patches, given, nl)
            grad = ops.unpatchify(d_rows, Cc, S, P)
        return (o if od is None else (o + od) / 2), grad, chosen.long()

    @torch.no_grad()
    def integrated_gradients(self, x, target=None, num_labels=None, *, baseline=None, steps=32, chunk=None):
        """``(eval logits, ig, target, y, y_baseline)``: ``ig`` float32 [B, C, S, S] are the integrated gradients of the target's eval logit
        along the straight path from the baseline to ``x`` (``reference_integrated_gradients`` is the spec), ``y`` / ``y_baseline`` float32
        [B] the target's eval logit at ``x`` / at the baseline: ``ig.sum((1, 2, 3))`` tends to ``y - y_baseline``.

        One plain forward on ``x`` fixes the target (given, or the first top-1 label among ``num_labels``); then ``steps`` interpolated
        inputs of the midpoint rule are made as patch rows in chunks of ``chunk`` steps (``ops.ig_rows``), every chunk is ONE
        ``uvc_vit_compact_input_grad`` call at batch ``chunk * B``, and the gradients are summed in step order (``ops.ig_accumulate``).
        ``baseline``: None for zeros (the dataset's mean colour in the normalised input), a ``[C]`` colour or a ``[B, C, S, S]`` batch.
        ``chunk``: default the largest divisor of ``steps`` with ``chunk * B <= 64`` images (at least 1)."""
        from . import ops
        cfg = self._export["cfg"]
        nl = CP.num_labels(cfg, num_labels)
        steps, chunk = _check_steps(steps, chunk)
        x = self._prep(x)
        B, dev = x.shape[0], self._flat.device
        x0 = _baseline_image(baseline, x)
        given = None if target is None else self._targets(target, B, nl)
        if chunk is None:
            chunk = max([c for c in range(1, steps + 1) if steps % c == 0 and c * B <= max(B, MAX_CHUNK_IMAGES)])
        Cc, S, P, npatch, K0 = self._geometry()
        with torch.cuda.device(dev):
            rows = self._rows_of(x)
            rows0 = None if x0 is None else self._rows_of(x0)
            logits = self._eval_logits(patches=rows)
            t = ops.logits_topk(logits, 1, nl)[1][:, 0].contiguous() if given is None else given
            base = self._eval_logits(patches=rows0 if rows0 is not None else torch.zeros_like(rows))
            y = logits.gather(1, t.long()[:, None])[:, 0]
            y0 = base.gather(1, t.long()[:, None])[:, 0]
            acc = torch.empty(B * npatch, K0, dtype=torch.float32, device=dev)
            for s0 in range(0, steps, chunk):
                c = min(chunk, steps - s0)
                inter = ops.ig_rows(rows, rows0, s0, c, steps)
                _, _, d_rows, _ = self._input_grad_rows(None, inter, t.repeat(c), nl)
                ops.ig_accumulate(d_rows, acc, first=s0 == 0)
            sum_grad = ops.unpatchify(acc, Cc, S, P)
            ig = (x if x0 is None else x - x0) * sum_grad / steps
        return logits, ig, t.long(), y, y0

    @torch.no_grad()
    def pixel_maps(self, grad, x=None, baseline=None, scale=1.0):
        """``(pixel float32 [B, S, S], patch float32 [B, np], total float32 [B])`` of a gradient or an integrated-gradients result ``grad``
        float32 [B, C, S, S]: per element ``e = grad * scale``, or with ``x`` ``e = grad * (x - baseline) * scale`` (gradient x input; the
        difference is taken of the patch rows in the model's dtype); the pixel map is ``sum_c |e|``, the patch map the sum of ``|e|`` over
        a patch, the total the signed sum of ``e`` over the image (``ops.pixel_maps``)."""
        from . import ops
        grad = self._prep(grad)
        Cc, S, P, _, _ = self._geometry()
        if baseline is not None and x is None:
            raise ValueError("a baseline goes with x")
        with torch.cuda.device(self._flat.device):
            a = self._rows_of(grad, ops.UVC_F32)
            xr = x0r = None
            if x is not None:
                x = self._prep(x)
                if x.shape != grad.shape:
                    raise ValueError(f"x {tuple(x.shape)} and the gradient {tuple(grad.shape)} differ in shape")
                xr = self._rows_of(x)
                x0 = _baseline_image(baseline, x)
                x0r = None if x0 is None else self._rows_of(x0)
            return ops.pixel_maps(a, Cc, S, P, xr, x0r, scale)


# ---- image files -----------------------------------------------------------------------------------------------------------------------
def write_pixel_map(pixel_dir, index, name, pixel):
    """``<pixel_dir>/<index>_<basename>.png``: the S x S pixel map divided by its maximum, 8-bit greyscale.  Returns the path."""
    import numpy as np
    from PIL import Image
    m = np.asarray(pixel, dtype=np.float64)
    top = float(m.max()) if m.size else 0.0
    m = m / top if top > 0 else np.zeros_like(m)
    path = os.path.join(pixel_dir, f"{index}_{os.path.basename(str(name))}.png")
    Image.fromarray(np.round(m * 255).astype(np.uint8), "L").save(path)
    return path


def record_of(name, top, target, grid, patch_map, ig=None):
    """One record: ``attribute``'s without ``"tokens"`` -- ``"map"`` is the patch map divided by its sum (zeros stay zeros); ``ig``:
    ``(y, y_baseline, total)`` adds ``"y"``, ``"y_baseline"`` and ``"delta" = total - (y - y_baseline)``."""
    total = float(sum(patch_map))
    rec = dict(file=name, top=top, target=int(target), grid=[int(grid), int(grid)], map=[v / total if total > 0 else 0.0 for v in patch_map])
    if ig is not None:
        y, y0, s = (float(v) for v in ig)
        rec.update(y=y, y_baseline=y0, delta=s - (y - y0))
    return rec


def check_method(method, steps=32, baseline="mean"):
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, not {method!r}")
    if baseline not in BASELINES:
        raise ValueError(f"baseline must be one of {BASELINES}, not {baseline!r}")
    return method, _check_steps(steps, None)[0], baseline


def check_tokens(export):
    """The refusal of the module, before anything else is looked at: at most 256 tokens."""
    n = CP._seq(CP.check_export(export)["cfg"])
    if n > MAX_TOKENS:
        raise NotImplementedError(f"input gradients of a compact model with {n} tokens: the attention backward at a value width takes at most {MAX_TOKENS}")


def explain_pixels(model, files, *, method="saliency", steps=32, baseline="mean", target=None, overlay_dir=None, pixel_dir=None, topk=5,
                   batch_size=64, preset="imagenet", interpolation="bilinear", crop_pct=None, num_labels=None, classes=None, num_workers=8):
    """Pixel-resolution maps of image files on a ``CompactPixelViT``: a generator of one record per file, in input order --
    ``{"file", "top", "target", "grid", "map"}`` (``record_of``; for ``ig`` also ``"y"``, ``"y_baseline"``, ``"delta"``), or
    ``{"file", "error"}`` for a file that cannot be read.  ``method``: "saliency" ``|dy/dx|``, "gradxinput" ``|x dy/dx|``, "ig"
    (``steps`` points, ``baseline`` "mean": zeros in the normalised input, or "black").  ``target``: the class explained for every image,
    or None for each image's own top-1 label among ``num_labels``.  ``overlay_dir``: ``compact.write_overlay`` of the patch map;
    ``pixel_dir``: ``write_pixel_map``.  The other keywords are ``compact.predict``'s."""
    from . import data, ops
    method, steps, baseline = check_method(method, steps, baseline)
    if not isinstance(model, CompactPixelViT):
        raise TypeError(f"pixel maps need a CompactPixelViT, not {type(model).__name__}")
    if preset not in CP.PRESETS:
        raise ValueError(f"preset must be one of {CP.PRESETS}, not {preset!r}")
    c = model._export["cfg"]
    classes = None if classes is None else list(classes)
    if num_labels is None and classes is not None:
        num_labels = len(classes)
    nl, topk = CP.num_labels(c, num_labels), int(topk)
    if classes is not None and len(classes) < nl:
        raise ValueError(f"{len(classes)} class names for {nl} labels")
    if not 1 <= topk <= min(CP.MAX_TOPK, nl):
        raise ValueError(f"topk {topk} must lie in [1, {min(CP.MAX_TOPK, nl)}]")
    if target is not None and not 0 <= int(target) < nl:
        raise ValueError(f"target {target} must lie in [0, {nl}) (num_labels)")
    ds = files if hasattr(files, "load") else data.FileListDataset(files, tolerant=True)
    names = ds.paths if hasattr(ds, "paths") else list(range(len(ds)))
    errors = getattr(ds, "errors", {})
    dev = model._flat.device
    kw = dict(mean=data.IMAGENET_MEAN, std=data.IMAGENET_STD, eval="center") if preset == "imagenet" else \
        dict(mean=data.CIFAR_MEAN, std=data.CIFAR_STD, eval="square")
    loader = data.DeviceLoader(ds, int(batch_size), c["img_size"], train=False, num_workers=num_workers, device=dev, interpolation=interpolation,
                               crop_pct=crop_pct, **kw)
    g = c["img_size"] // c["patch_size"]
    base = black_baseline(preset) if baseline == "black" else None
    for d in (overlay_dir, pixel_dir):
        if d is not None:
            os.makedirs(d, exist_ok=True)
    first = 0
    with torch.cuda.device(dev):
        for x, _ in loader:
            t = None if target is None else int(target)
            extra = None
            if method == "ig":
                logits, ig, chosen, y, y0 = model.integrated_gradients(x, t, nl, baseline=base, steps=steps)
                pixel, patch, total = model.pixel_maps(ig)
                extra = (y.cpu().tolist(), y0.cpu().tolist(), total.cpu().tolist())
            else:
                logits, grad, chosen = model.input_grad(x, t, nl)
                pixel, patch, _ = model.pixel_maps(grad, x=x if method == "gradxinput" else None)
            probs, index = ops.logits_topk(logits, topk, nl)
            probs, index, chosen, patch = probs.cpu().tolist(), index.cpu().tolist(), chosen.cpu().tolist(), patch.cpu()
            pixel = pixel.cpu() if pixel_dir is not None else None
            for b in range(len(probs)):
                i = first + b
                if i in errors:
                    yield dict(file=names[i], error=errors[i])
                    continue
                top = [dict(index=j, label=None if classes is None else classes[j], prob=q) for j, q in zip(index[b], probs[b])]
                yield record_of(names[i], top, chosen[b], g, patch[b].tolist(), None if extra is None else (extra[0][b], extra[1][b], extra[2][b]))
                if overlay_dir is not None:
                    CP.write_overlay(overlay_dir, i, names[i], ds.load(i), patch[b].reshape(g, g).numpy(), c["img_size"], preset, interpolation, crop_pct)
                if pixel_dir is not None:
                    write_pixel_map(pixel_dir, i, names[i], pixel[b].numpy())
            first += len(probs)


# ---- command line ------------------------------------------------------------------------------------------------------------------------
def build_parser():
    p = argparse.ArgumentParser(prog="python -m uvc_amd.compact_pixel",
                                description="Pixel-resolution maps of a compact model: saliency, gradient x input, integrated gradients")
    p.add_argument("--compact", required=True, help="the compact file")
    p.add_argument("--method", choices=list(METHODS), required=True,
                   help="saliency: |dy/dx|; gradxinput: |x dy/dx|; ig: integrated gradients from the baseline to the image")
    p.add_argument("--steps", type=CP._int_in(1, 4096, "--steps"), default=32, help="ig: points of the midpoint rule")
    p.add_argument("--baseline", choices=list(BASELINES), default="mean",
                   help="ig: mean = the dataset's mean colour (zeros in the normalised input, what compact_perturb removes patches to); black")
    p.add_argument("--target", type=CP._int_in(0, (1 << 20) - 1, "--target"), default=None,
                   help="the class explained, in [0, num_labels); default: every image's own top-1 label among --num_labels")
    p.add_argument("--overlay_dir", default=None, help="write <index>_<basename>.png per readable image: the model's view with the patch map in red")
    p.add_argument("--pixel_dir", default=None, help="write <index>_<basename>.png per readable image: the pixel map, greyscale, divided by its maximum")
    CP.add_image_file_flags(p)
    return p


def main(argv: Optional[Sequence[str]] = None):
    """One JSON line per image to --output (or stdout), then ``predict``'s summary line ``{"images", "errors", "batches", "img_per_s"}``,
    which is returned.  A file with more than 256 tokens fails before any image is listed or read."""
    from . import data
    args = build_parser().parse_args(argv)
    export = CP.load_compact(args.compact)
    check_tokens(export)
    classes = CP.read_classes(args.classes) if args.classes else None
    dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    model = CompactPixelViT(export, precision=args.precision, device=dev)
    files = data.list_images(args.images)
    recs = explain_pixels(model, files, method=args.method, steps=args.steps, baseline=args.baseline, target=args.target,
                          overlay_dir=args.overlay_dir, pixel_dir=args.pixel_dir, topk=args.topk, batch_size=args.batch_size, preset=args.preset,
                          interpolation=args.interpolation, crop_pct=args.crop_pct, num_labels=args.num_labels, classes=classes,
                          num_workers=args.num_workers)
    return CP.write_records(recs, args.output, batch_size=args.batch_size)


if __name__ == "__main__":
    main()
