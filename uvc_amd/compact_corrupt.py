"""Common-corruption robustness of a compact model on MI355X: top-1 under noise, blur, contrast, brightness and pixelation at five severities,
in the style of ImageNet-C (Hendrycks & Dietterich, ICLR 2019), read as corruption error relative to an unpruned parent.

    python -m uvc_amd.compact_corrupt --compact m.compact.pt [--baseline parent.compact.pt] --dataset cifar10|cifar100|imagenet --data_dir D
        [--kinds K ...] [--severities 1 2 3 4 5] [--level FLOAT] [--seed 0] [--max_images N] [--output table.json]

The corruptions are made from the split the user has, AFTER the eval transform, at the model's input size, on the device: they are not
ImageNet-C's files.  ``x`` is the loader's batch, float32 [B, C, H, W] normalised with the preset's ``mean_c``, ``std_c``; the pixel is
``p = x std_c + mean_c`` and every kind takes one real level ``a``, is stated on pixels, computed on the normalised values and ends with
``clamp(., lo_c, hi_c)``, the normalised 0 and 1 of ``compact_robust.linf_bounds``:

    gaussian_noise   p + a z
    speckle_noise    p + a p z
    impulse_noise    u < a / 2 -> 0;  a / 2 <= u < a -> 1;  else p                       (per element and channel)
    brightness       p clipped to [0, 1]; V = max_c p_c, V' = min(V + a, 1); p' = p V' / V when V > 0, else V'      (the HSV value shift)
    contrast         (p - m) a + m, m the mean of p over the image's channels and pixels
    gaussian_blur    sigma = a, R = int(4 sigma + 0.5), weights exp(-k^2 / 2 sigma^2) normalised in float64 and rounded to float32;
                     a horizontal, then a vertical pass, borders clamp the index, the plane between the passes is float32
    defocus_blur     r = a (integer, 1 .. 12): taps float32(1 / count) where dx^2 + dy^2 <= r^2, summed in row-major order, borders clamp
    pixelate         k = a (integer): every pixel becomes the mean of its k x k cell; cells start at 0, a ragged last cell averages what exists

z and u are keyed draws (uvc_exp_noise's generator): with the global element index ``g = index0 C H W + e`` the pair ``j = g >> 1`` draws u1
(site 0) and u2 (site 1) from ``key(seed, stream, site)`` at counter j, ``r = sqrt(-2 ln u1)``, ``t = float32(2 pi_f32 u2)``, ``z = r cos t`` for
even g and ``r sin t`` for odd g; impulse_noise draws site 2 at counter g.  ``index0`` is the dataset index of the batch's first image, so
an image's noise does not depend on the batching; the module's stream is ``8 kind_index + severity`` (severity 0: an explicit level).

``corrupt`` runs uvc_amd/csrc/corrupt.hip; ``reference_corrupt`` is this spec in float64 and needs no device.
"""
from __future__ import annotations

import argparse
import json
import math
import time
from typing import Optional, Sequence

import numpy as np
import torch

from . import compact as CP
from . import compact_tools as TL
from .compact_robust import linf_bounds, preset_stats

CORRUPTIONS = ("gaussian_noise", "speckle_noise", "impulse_noise", "brightness", "contrast", "gaussian_blur", "defocus_blur", "pixelate")
NOISES, COLOURS = CORRUPTIONS[:3], CORRUPTIONS[3:5]
# ImageNet-C's constants where the kind is the same (gaussian / speckle / impulse noise, brightness, contrast, the blurs' first
# parameter); pixelate's cells are ours (ImageNet-C resizes by a real factor)
SEVERITY = {
    "gaussian_noise": (.08, .12, .18, .26, .38),
    "speckle_noise": (.15, .2, .35, .45, .6),
    "impulse_noise": (.03, .06, .09, .17, .27),
    "brightness": (.1, .2, .3, .4, .5),
    "contrast": (.4, .3, .2, .1, .05),
    "gaussian_blur": (1, 2, 3, 4, 6),
    "defocus_blur": (3, 4, 6, 8, 10),
    "pixelate": (2, 3, 4, 5, 6),
}
SEVERITIES = (1, 2, 3, 4, 5)
MAX_BLUR_RADIUS, MAX_DISK_RADIUS = 32, 12
TWO_PI_F32 = np.float32(6.28318530717958647692)


# ---- levels ----------------------------------------------------------------------------------------------------------------------------
def check_level(kind, level):
    """The level of ``kind`` as the kernels take it (a float; an int for defocus_blur and pixelate), every refusal made."""
    if kind not in CORRUPTIONS:
        raise ValueError(f"kind must be one of {CORRUPTIONS}, not {kind!r}")
    a = float(level)
    if not (a >= 0 and math.isfinite(a)):
        raise ValueError(f"{kind}: the level {level} must be non-negative and finite")
    if kind == "impulse_noise" and a > 1:
        raise ValueError(f"impulse_noise: the level {level} is a share, at most 1")
    if kind == "gaussian_blur" and int(4 * a + 0.5) > MAX_BLUR_RADIUS:
        raise ValueError(f"gaussian_blur: sigma {level} needs a radius beyond {MAX_BLUR_RADIUS}")
    if kind in ("defocus_blur", "pixelate"):
        if a != int(a) or a < 1 or a >= 2 ** 31:
            raise ValueError(f"{kind}: the level {level} must be an integer, at least 1")
        if kind == "defocus_blur" and a > MAX_DISK_RADIUS:
            raise ValueError(f"defocus_blur: the radius {level} must lie in [1, {MAX_DISK_RADIUS}]")
        return int(a)
    return a


def level_of(kind, severity=None, level=None):
    """``(level, stream)``: exactly one of ``severity`` (1 .. 5, the ``SEVERITY`` table) and ``level`` is given."""
    if kind not in CORRUPTIONS:
        raise ValueError(f"kind must be one of {CORRUPTIONS}, not {kind!r}")
    if (severity is None) == (level is None):
        raise ValueError("pass one of severity / level")
    if severity is not None:
        if severity not in SEVERITIES:
            raise ValueError(f"severity {severity!r} must be one of {SEVERITIES}")
        level = SEVERITY[kind][severity - 1]
    return check_level(kind, level), 8 * CORRUPTIONS.index(kind) + (severity or 0)


def gaussian_taps(sigma):
    """float32 [2 R + 1], R = int(4 sigma + 0.5): ``exp(-k^2 / 2 sigma^2)`` normalised in float64, rounded once."""
    R = int(4 * float(sigma) + 0.5)
    k = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-k * k / (2 * float(sigma) ** 2)) if R > 0 else np.ones(1)
    return (w / w.sum()).astype(np.float32)


def disk_taps(r):
    """float32 [2 r + 1, 2 r + 1]: ``float32(1 / count)`` where ``dx^2 + dy^2 <= r^2``, 0 elsewhere."""
    r = int(r)
    d = np.arange(-r, r + 1)
    inside = d[:, None] ** 2 + d[None, :] ** 2 <= r * r
    return np.where(inside, np.float32(1.0 / inside.sum()), np.float32(0)).astype(np.float32)


def _stats(mean, std, Cc):
    m, s = [float(v) for v in mean], [float(v) for v in std]
    if len(m) != Cc or len(s) != Cc:
        raise ValueError(f"mean and std hold {len(m)} / {len(s)} channels, the batch has {Cc}")
    if Cc > 4:
        raise ValueError("at most 4 channels")
    if not all(v > 0 and math.isfinite(v) for v in s) or not all(math.isfinite(v) for v in m):
        raise ValueError("std must be positive, mean and std finite")
    return m, s


# ---- the keyed generator on the host (elementwise.hip's uvc_exp_noise, restated) -------------------------------------------------------
_M64 = (1 << 64) - 1


def _splitmix64(x):
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _key(seed, stream, site):
    k = ((int(seed) & _M64) * 0xD1342543DE82EF95 + 0x2545F4914F6CDD1D) & _M64
    k ^= (((int(stream) & _M64) + 1) * 0x9E3779B97F4A7C15) & _M64
    k = ((k << 17) | (k >> 47)) & _M64
    return np.uint64(k ^ (((int(site) + 1) * 0xC2B2AE3D27D4EB4F) & _M64))


def keyed_uniforms(seed, stream, site, start, n):
    """float32 [n]: the uniforms of ``key(seed, stream, site)`` at the counters ``start .. start + n - 1`` (``(c + 1/2) 2^-24`` of the hash's top
    24 bits in float32 operations, the one value that rounds to 1 brought back to ``1 - 2^-24``)."""
    with np.errstate(over="ignore"):
        ctr = np.uint64(int(start) & _M64) + np.arange(n, dtype=np.uint64)
        c = (_splitmix64(_key(seed, stream, site) ^ _splitmix64(ctr)) >> np.uint64(40)).astype(np.uint32)
    u = (c.astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    return np.minimum(u, np.float32(1.0) - np.float32(2.0 ** -24))


def keyed_normals(seed, stream, gstart, n):
    """float64 [n]: z of the global indices ``gstart .. gstart + n - 1``, the Box-Muller pair ``g >> 1`` in float64 on the float32 uniforms."""
    g = np.uint64(int(gstart)) + np.arange(n, dtype=np.uint64)
    j0 = int(gstart) >> 1
    npairs = ((int(gstart) + n - 1) >> 1) - j0 + 1
    u1 = keyed_uniforms(seed, stream, 0, j0, npairs).astype(np.float64)
    u2 = keyed_uniforms(seed, stream, 1, j0, npairs)
    r = np.sqrt(-2.0 * np.log(u1))
    t = (TWO_PI_F32 * u2).astype(np.float32).astype(np.float64)
    pair = ((g >> np.uint64(1)) - np.uint64(j0)).astype(np.int64)
    odd = (g & np.uint64(1)).astype(bool)
    return np.where(odd, r[pair] * np.sin(t[pair]), r[pair] * np.cos(t[pair]))


# ---- the written spec ------------------------------------------------------------------------------------------------------------------
def _gather_sum(x, taps, dim, R):
    """sum_k taps[k] x[clamp(i + k - R)] along ``dim``, ascending k, in x's dtype"""
    n = x.shape[dim]
    out = torch.zeros_like(x)
    base = torch.arange(n)
    for k, w in enumerate(taps):
        out = out + float(w) * x.index_select(dim, (base + k - R).clamp(0, n - 1))
    return out


def reference_corrupt(x, kind, level, *, mean, std, seed=0, stream=0, index0=0, clamp=True):
    """The spec in float64 plain PyTorch / numpy on the host: float32 of x's shape (``clamp=False``: the float64 values before the clamp)."""
    level = check_level(kind, level)
    x = torch.as_tensor(x).detach().cpu()
    if x.dim() != 4 or x.numel() == 0:
        raise ValueError("x must be a non-empty [B, C, H, W]")
    B, Cc, H, W = x.shape
    m, s = _stats(mean, std, Cc)
    _, lo, hi = linf_bounds(m, s, 0)
    x = x.to(torch.float64)
    mv, sv = torch.tensor(m, dtype=torch.float64).view(1, -1, 1, 1), torch.tensor(s, dtype=torch.float64).view(1, -1, 1, 1)
    n, g0 = x.numel(), int(index0) * Cc * H * W
    if kind in ("gaussian_noise", "speckle_noise"):
        z = torch.from_numpy(keyed_normals(seed, stream, g0, n)).view(x.shape)
        out = x + z * (level / sv) if kind == "gaussian_noise" else x + z * (level * (x + mv / sv))
    elif kind == "impulse_noise":
        u = torch.from_numpy(keyed_uniforms(seed, stream, 2, g0, n).astype(np.float64)).view(x.shape)
        out = torch.where(u < level / 2, lo.double().view(1, -1, 1, 1).expand_as(x), torch.where(u < level, hi.double().view(1, -1, 1, 1).expand_as(x), x))
    elif kind == "brightness":
        p = (x * sv + mv).clamp(0, 1)
        V = p.amax(dim=1, keepdim=True)
        Vn = (V + level).clamp(max=1)
        pn = torch.where(V > 0, p * (Vn / torch.where(V > 0, V, torch.ones_like(V))), Vn.expand_as(p))
        out = (pn - mv) / sv
    elif kind == "contrast":
        mu = (x * sv + mv).mean(dim=(1, 2, 3), keepdim=True)
        out = level * x + (1 - level) * ((mu - mv) / sv)
    elif kind == "gaussian_blur":
        taps = gaussian_taps(level).astype(np.float64)
        R = len(taps) // 2
        out = _gather_sum(_gather_sum(x, taps, 3, R).float().double(), taps, 2, R)
    elif kind == "defocus_blur":
        taps = disk_taps(level).astype(np.float64)
        r = level
        out = torch.zeros_like(x)
        ys, xs = torch.arange(H), torch.arange(W)
        for dy in range(-r, r + 1):
            rows = x.index_select(2, (ys + dy).clamp(0, H - 1))
            for dx in range(-r, r + 1):
                if taps[dy + r, dx + r] != 0:
                    out = out + float(taps[dy + r, dx + r]) * rows.index_select(3, (xs + dx).clamp(0, W - 1))
    else:
        k = level
        ncx = (W + k - 1) // k
        cell = ((torch.arange(H) // k)[:, None] * ncx + (torch.arange(W) // k)[None, :]).reshape(-1)
        ncell = ((H + k - 1) // k) * ncx
        flat = x.reshape(B * Cc, H * W)
        sums = torch.zeros(B * Cc, ncell, dtype=torch.float64).index_add_(1, cell, flat)
        cnt = torch.zeros(ncell, dtype=torch.float64).index_add_(0, cell, torch.ones(H * W, dtype=torch.float64))
        out = (sums / cnt)[:, cell].view(x.shape)
    if not clamp:
        return out
    return torch.minimum(torch.maximum(out, lo.double().view(1, -1, 1, 1)), hi.double().view(1, -1, 1, 1)).float()


# ---- the device ------------------------------------------------------------------------------------------------------------------------
_DISKS = {}


def _disk_on(r, dev):
    if (r, dev) not in _DISKS:
        _DISKS[(r, dev)] = torch.from_numpy(disk_taps(r)).to(dev)
    return _DISKS[(r, dev)]


@torch.no_grad()
def corrupt(x, kind, *, severity=None, level=None, mean, std, seed=0, index0=0, out=None):
    """``out`` float32 [B, C, H, W] on x's device: ``x`` (the loader's normalised batch) under ``kind`` at ``severity`` 1 .. 5 of ``SEVERITY``
    or at an explicit ``level`` (``reference_corrupt`` is the spec).  ``index0``: the dataset index of the batch's first image (the noises)."""
    from . import ops
    level, stream = level_of(kind, severity, level)
    if x.dim() != 4:
        raise ValueError("x must be float32 [B, C, H, W]")
    m, s = _stats(mean, std, x.shape[1])
    _, lo, hi = linf_bounds(m, s, 0)
    with torch.cuda.device(x.device):
        if kind in NOISES:
            return ops.corrupt_noise(x, kind, level, mean=m, std=s, lo=lo, hi=hi, seed=seed, stream=stream, index0=index0, out=out)
        if kind == "brightness":
            return ops.corrupt_colour(x, kind, level, mean=m, std=s, lo=lo, hi=hi, out=out)
        if kind == "contrast":
            return ops.corrupt_colour(x, kind, level, mean=m, std=s, lo=lo, hi=hi, out=out)[0]
        if kind == "gaussian_blur":
            return ops.blur_separable(x, gaussian_taps(level), lo=lo, hi=hi, out=out)
        if kind == "defocus_blur":
            return ops.stencil2d(x, _disk_on(level, x.device), lo=lo, hi=hi, out=out)
        return ops.pixelate(x, level, lo=lo, hi=hi, out=out)


# ---- the arithmetic of the record --------------------------------------------------------------------------------------------------------
def _ratio(num, den):
    return num / den if den > 0 else None


def _mean_of(values):
    kept = [v for v in values if v is not None]
    return (sum(kept) / len(kept) if kept else None), len(kept)


def corruption_errors(table, base=None):
    """The error arithmetic on plain tables ``{"clean_top1": t, "kinds": {kind: {"levels": [...], "top1": [...]}}}``: every kind gains
    ``error`` (``100 - top1``) and ``mean_error``, the table ``mean_corruption_error`` (the mean over kinds of ``mean_error``, un-normalised).
    With ``base`` (the same kinds and levels): ``baseline`` (its own such record) and per kind ``ce = sum_s E / sum_s E_base`` and
    ``relative_ce = sum_s (E - E_clean) / sum_s (E_base - E_base,clean)``, None where the denominator is not positive; ``mCE`` and
    ``relative_mCE`` are their means over the kinds that have one, counted in ``mCE_kinds`` / ``relative_mCE_kinds``."""
    def own(t):
        kinds = {}
        for kind, row in t["kinds"].items():
            err = [100.0 - float(v) for v in row["top1"]]
            if not err or len(err) != len(row["levels"]):
                raise ValueError(f"{kind}: one top-1 per level")
            kinds[kind] = dict(levels=list(row["levels"]), top1=[float(v) for v in row["top1"]], error=err, mean_error=sum(err) / len(err))
        if not kinds:
            raise ValueError("a table needs at least one kind")
        return dict(clean_top1=float(t["clean_top1"]), kinds=kinds, mean_corruption_error=sum(k["mean_error"] for k in kinds.values()) / len(kinds))

    rec = own(table)
    if base is None:
        return rec
    b = own(base)
    if {k: v["levels"] for k, v in b["kinds"].items()} != {k: v["levels"] for k, v in rec["kinds"].items()}:
        raise ValueError("the baseline's table has other kinds or levels")
    e0, b0 = 100.0 - rec["clean_top1"], 100.0 - b["clean_top1"]
    for kind, row in rec["kinds"].items():
        be = b["kinds"][kind]["error"]
        row["ce"] = _ratio(sum(row["error"]), sum(be))
        row["relative_ce"] = _ratio(sum(e - e0 for e in row["error"]), sum(e - b0 for e in be))
    rec["baseline"] = b
    rec["mCE"], rec["mCE_kinds"] = _mean_of([r["ce"] for r in rec["kinds"].values()])
    rec["relative_mCE"], rec["relative_mCE_kinds"] = _mean_of([r["relative_ce"] for r in rec["kinds"].values()])
    return rec


# ---- the command ---------------------------------------------------------------------------------------------------------------------------
def plan(args):
    """``[(kind, severity or None, level), ...]`` of the parsed flags, every refusal made."""
    kinds = list(args.kinds) if args.kinds else list(CORRUPTIONS)
    for k in kinds:
        if k not in CORRUPTIONS:
            raise ValueError(f"--kinds: {k!r} is not one of {CORRUPTIONS}")
    if len(set(kinds)) != len(kinds):
        raise ValueError("--kinds names a kind twice")
    if args.max_images is not None and int(args.max_images) < 1:
        raise ValueError(f"--max_images {args.max_images} must be positive")
    if args.level is not None:
        if len(kinds) != 1:
            raise ValueError("--level replaces the severity table of a single kind: name it with --kinds")
        return [(kinds[0], None, level_of(kinds[0], level=args.level)[0])]
    sev = list(args.severities)
    if not sev or len(set(sev)) != len(sev) or any(s not in SEVERITIES for s in sev):
        raise ValueError(f"--severities must be distinct values of {SEVERITIES}")
    return [(k, s, level_of(k, severity=s)[0]) for k in kinds for s in sev]


def check_baseline(export, base):
    """Refuses a baseline that cannot read the same batch."""
    for key, what in (("img_size", "image size"), ("in_chans", "input channels")):
        if export["cfg"][key] != base["cfg"][key]:
            raise ValueError(f"the baseline's {what} {base['cfg'][key]} is not the model's {export['cfg'][key]}")


def evaluate(export_or_path, args, dev=None):
    """The command's record (``corruption_errors``' plus ``images``, ``img_per_s`` and ``compact._report``'s widths, parameters and MACs) from
    ONE walk over the split: per batch the clean forward, then for each (kind, severity) one ``corrupt`` and one forward -- of both models
    on the same corrupted batch with ``--baseline``."""
    from . import ops
    cells = plan(args)
    export = CP.as_export(export_or_path)
    base = CP.as_export(args.baseline) if getattr(args, "baseline", None) is not None else None
    exports = [export] + ([base] if base is not None else [])
    if base is not None:
        check_baseline(export, base)
    known = {"cifar10": 10, "cifar100": 100}.get(args.dataset)
    if known is not None:                                # the data's label set against both heads, before any data is read
        for ex in exports:
            CP.num_labels(ex["cfg"], known)
    mean, std = preset_stats(args.dataset)
    _stats(mean, std, export["cfg"]["in_chans"])
    dev = TL.device(dev)
    models = [CP.CompactVisionTransformer(ex, precision=args.precision, device=dev) for ex in exports]
    loader, classes = TL.eval_loader(export, args, args.split)
    nls = [CP.num_labels(ex["cfg"], classes) for ex in exports]
    n = 0
    with torch.cuda.device(dev):
        hits = torch.zeros(len(models), len(cells) + 1, dtype=torch.int64, device=dev)
        buf = None
        t0 = time.perf_counter()
        for x, y in loader:
            if args.max_images is not None and n + x.shape[0] > args.max_images:
                x, y = x[:args.max_images - n].contiguous(), y[:args.max_images - n]
            y = y.to(torch.int64)
            if buf is None or buf.shape != x.shape:
                buf = torch.empty_like(x)
            for i, cell in enumerate([None] + cells):
                xc = x if cell is None else corrupt(x, cell[0], severity=cell[1], level=None if cell[1] else cell[2], mean=mean, std=std,
                                                    seed=args.seed, index0=n, out=buf)
                for mi, (model, nl) in enumerate(zip(models, nls)):
                    hits[mi, i] += (ops.logits_topk(model(xc)[0], 1, nl)[1][:, 0].to(torch.int64) == y).sum()
            n += int(x.shape[0])
            if args.max_images is not None and n >= args.max_images:
                break
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    if n == 0:
        raise ValueError(f"the {args.split} split is empty")
    top1 = (100.0 * hits.double() / n).cpu().tolist()

    def table(row):
        kinds = {}
        for (kind, _, level), v in zip(cells, row[1:]):
            kinds.setdefault(kind, dict(levels=[], top1=[]))
            kinds[kind]["levels"].append(level)
            kinds[kind]["top1"].append(v)
        return dict(clean_top1=row[0], kinds=kinds)

    rec = corruption_errors(table(top1[0]), table(top1[1]) if base is not None else None)
    return dict(images=n, **rec, img_per_s=n / dt if dt > 0 else 0.0, **CP._report(export))


def build_parser():
    p = argparse.ArgumentParser(prog="python -m uvc_amd.compact_corrupt",
                                description="Top-1 of a compact model under common corruptions made on the device, in the style of ImageNet-C")
    p.add_argument("--compact", required=True, help="the compact file")
    p.add_argument("--baseline", default=None, help="the compact file of the parent: adds ce, relative_ce, mCE and relative_mCE")
    TL.add_dataset_flags(p, eval_batch_size=64, split_default="test")
    p.add_argument("--kinds", nargs="+", choices=list(CORRUPTIONS), default=list(CORRUPTIONS))
    p.add_argument("--severities", nargs="+", type=int, choices=list(SEVERITIES), default=list(SEVERITIES))
    p.add_argument("--level", type=float, default=None, help="an explicit level in place of the severity table, for a single kind")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--max_images", type=int, default=None, help="stop after this many images")
    p.add_argument("--output", default=None, help="also write the record to this JSON file")
    return p


def main(argv: Optional[Sequence[str]] = None):
    """One JSON line (``evaluate``'s record), which is returned.  The refusals -- --level with several kinds, a level outside its kind's
    range, a baseline of another image size, labels outside a head -- come before any image is read."""
    args = build_parser().parse_args(argv)
    plan(args)
    TL.need_data(args)
    summary = evaluate(args.compact, args)
    if args.output:
        with open(args.output, "w") as f:
            json.dump(summary, f)
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
