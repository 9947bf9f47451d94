"""A numpy restatement of PIL's Image.resize(size, BILINEAR | BICUBIC, box) for 8-bit RGB (Resample.c: bilinear_filter, bicubic_filter,
precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc, ImagingResampleInner) -- tests/pil_bilinear.py
with the filter as a parameter, and with the accumulators of both passes before clip8, which is what shows whether a case makes the
clamps work.  tests/test_image_bicubic_cpu.py checks it against the installed PIL; the spec of uvc_image_prep's filters
(include/uvc_data.h).  Also the image patterns and resize cases the CPU and GPU tests share."""
import math

import numpy as np

PRECISION_BITS = 22
BILINEAR, BICUBIC = "bilinear", "bicubic"
SUPPORT = {BILINEAR: 1.0, BICUBIC: 2.0}


def bilinear_filter(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def bicubic_filter(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


FILTER = {BILINEAR: bilinear_filter, BICUBIC: bicubic_filter}


def coeffs(in_size, in0, in1, out_size, filt):
    """(xmin [out], n [out], kk int64 [out, ksize]) of one axis, float64 arithmetic as the C."""
    in0, in1 = float(np.float32(in0)), float(np.float32(in1))          # the box is float32 in the C
    f = FILTER[filt]
    scale = (in1 - in0) / out_size
    fs = max(scale, 1.0)
    support = SUPPORT[filt] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    xmins, ns = np.zeros(out_size, np.int64), np.zeros(out_size, np.int64)
    kk = np.zeros((out_size, ksize), np.int64)
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        xmins[xx], ns[xx] = xmin, xmax
    return xmins, ns, kk


def clip8(v):
    return np.where(v >= (1 << PRECISION_BITS << 8), 255, np.where(v <= 0, 0, v >> PRECISION_BITS)).astype(np.uint8)


def _pass(a, xmins, kk, axis):
    """One pass along ``axis`` of int64 image a: acc[..., i, ...] = 2^21 + sum_k a[..., xmin_i + k, ...] * kk[i, k].  Returns
    (clip8(acc), acc)."""
    a = np.moveaxis(a, axis, 0)
    n_in = a.shape[0]
    idx = np.minimum(xmins[:, None] + np.arange(kk.shape[1])[None, :], n_in - 1)      # taps past n carry weight 0
    acc = np.full((len(xmins),) + a.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
    for k in range(kk.shape[1]):
        acc += a[idx[:, k]] * kk[:, k].reshape((-1,) + (1,) * (a.ndim - 1))
    return np.moveaxis(clip8(acc), 0, axis), np.moveaxis(acc, 0, axis)


def resize(a, size, filt, box=None, accs=None):
    """PIL Image.fromarray(a).resize(size=(w, h), filt, box) for uint8 [H, W, 3].  Image.resize itself splits a source taller than
    100 x its width that shrinks vertically into a vertical-only resize followed by a horizontal-only one.  ``accs``: a list that
    receives the int64 accumulators of every pass that ran, before clip8, in the order the passes ran."""
    H, W, _ = a.shape
    if H > W * 100 and size[1] < H:
        b = (0, 0, W, H) if box is None else box
        tmp = _resize_inner(a, (W, size[1]), filt, (0, b[1], W, b[3]), accs)
        return _resize_inner(tmp, size, filt, (b[0], 0, b[2], size[1]), accs)
    return _resize_inner(a, size, filt, box, accs)


def _resize_inner(a, size, filt, box=None, accs=None):
    """ImagingResample: horizontal pass first."""
    H, W, _ = a.shape
    ox, oy = size
    box = (0, 0, W, H) if box is None else box
    need_h = ox != W or box[0] or box[2] != ox
    need_v = oy != H or box[1] or box[3] != oy
    hx, hn, hk = coeffs(W, box[0], box[2], ox, filt)
    vy, vn, vk = coeffs(H, box[1], box[3], oy, filt)
    y0, y1 = int(vy[0]), int(vy[-1] + vn[-1])
    cur = a.astype(np.int64)
    if need_h:
        cur, acc = _pass(cur[y0:y1], hx, hk, 1)
        cur = cur.astype(np.int64)
        vy = vy - y0
        if accs is not None:
            accs.append(acc)
    if need_v:
        cur, acc = _pass(cur, vy, vk, 0)
        if accs is not None:
            accs.append(acc)
    return cur.astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- shared cases

def noise(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def checkerboard(h, w, cell=1):
    """0 / 255 cells of ``cell`` pixels."""
    y, x = np.mgrid[0:h, 0:w]
    v = ((((y // cell) + (x // cell)) & 1) * 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(v[:, :, None], 3, axis=2))


def step_edge(h, w):
    """A vertical step edge: 0 left of the middle column, 255 from it on."""
    a = np.zeros((h, w, 3), np.uint8)
    a[:, w // 2:] = 255
    return a


def step_edge_rows(h, w):
    """The same edge lying down: 0 above the middle row, 255 from it on (the edge the vertical pass sees)."""
    a = np.zeros((h, w, 3), np.uint8)
    a[h // 2:] = 255
    return a


PATTERNS = {"noise": noise, "checkerboard": checkerboard, "step": step_edge}

# (name, source (h, w), resize (w, h)): upscale, scale > 4 on both axes, the width unchanged, the height unchanged, 1 x 1 and 1 x 7
# sources, and a source Image.resize shrinks vertically first (h > 100 w, resize_h < h)
SHAPES = [("up", (32, 32), (224, 224)),
          ("down", (23, 37), (8, 8)),
          ("same_w", (30, 20), (20, 12)),
          ("same_h", (12, 30), (17, 12)),
          ("one", (1, 1), (8, 8)),
          ("row", (1, 7), (8, 8)),
          ("tall", (404, 3), (8, 8))]

# (name, image, resize (w, h)): 0 / 255 images whose bicubic resize overshoots.  A checkerboard makes both passes leave 0 .. 255 << 22
# on both sides; a step edge varies along one axis only, so the upright edge does it in the first (horizontal) pass and the edge
# lying down in the second (tests/test_image_bicubic_cpu.py holds each case to that).
CLAMP_CASES = [("checkerboard_up", checkerboard(32, 32), (224, 224)),
               ("step_up", step_edge(32, 32), (224, 224)),
               ("step_rows_up", step_edge_rows(32, 32), (224, 224)),
               ("checkerboard_8", checkerboard(5, 5), (8, 8)),
               ("checkerboard_down", checkerboard(23, 37, 8), (8, 8)),
               ("step_8", step_edge(5, 6), (8, 8)),
               ("step_rows_8", step_edge_rows(6, 5), (8, 8)),
               ("checkerboard_16", checkerboard(5, 6), (16, 16)),
               ("step_16", step_edge(7, 6), (16, 16)),
               ("step_rows_16", step_edge_rows(6, 7), (16, 16))]


def overshoot(acc):
    """(pixels below 0, pixels at or above 256 << 22) of one pass's accumulators: where clip8 does not simply shift.  (An accumulator
    in (255 << 22, 256 << 22) shifts to 255 by itself; one at 256 << 22 would shift to 256, which a byte stores as 0.)"""
    return int((acc < 0).sum()), int((acc >= (256 << PRECISION_BITS)).sum())
