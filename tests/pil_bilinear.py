"""A numpy restatement of PIL's Image.resize(size, BILINEAR, box) for 8-bit RGB (Resample.c: precompute_coeffs,
normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc, ImagingResampleInner) -- the spec uvc_image_prep is held to
(include/uvc_data.h).  tests/test_image_data_cpu.py checks it against the installed PIL."""
import math

import numpy as np

PRECISION_BITS = 22


def coeffs(in_size, in0, in1, out_size):
    """(xmin [out], n [out], kk int64 [out, ksize]) of one axis, float64 arithmetic as the C."""
    in0, in1 = float(np.float32(in0)), float(np.float32(in1))          # the box is float32 in the C
    scale = (in1 - in0) / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    xmins, ns = np.zeros(out_size, np.int64), np.zeros(out_size, np.int64)
    kk = np.zeros((out_size, ksize), np.int64)
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = []
        for x in range(xmax):
            t = abs((x + xmin - center + 0.5) * ss)
            w.append(1.0 - t if t < 1.0 else 0.0)
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
    """One pass along ``axis`` of int64 image a: out[..., i, ...] = clip8(2^21 + sum_k a[..., xmin_i + k, ...] * kk[i, k])."""
    a = np.moveaxis(a, axis, 0)
    n_in = a.shape[0]
    idx = np.minimum(xmins[:, None] + np.arange(kk.shape[1])[None, :], n_in - 1)      # taps past n carry weight 0
    acc = np.full((len(xmins),) + a.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
    for k in range(kk.shape[1]):
        acc += a[idx[:, k]] * kk[:, k].reshape((-1,) + (1,) * (a.ndim - 1))
    return np.moveaxis(clip8(acc), 0, axis)


def resize(a, size, box=None):
    """PIL Image.fromarray(a).resize(size=(w, h), BILINEAR, box) for uint8 [H, W, 3].  Image.resize itself splits a source taller
    than 100 x its width that shrinks vertically into a vertical-only resize followed by a horizontal-only one."""
    H, W, _ = a.shape
    if H > W * 100 and size[1] < H:
        b = (0, 0, W, H) if box is None else box
        tmp = _resize_inner(a, (W, size[1]), (0, b[1], W, b[3]))
        return _resize_inner(tmp, size, (b[0], 0, b[2], size[1]))
    return _resize_inner(a, size, box)


def _resize_inner(a, size, box=None):
    """ImagingResample: horizontal pass first."""
    H, W, _ = a.shape
    ox, oy = size
    box = (0, 0, W, H) if box is None else box
    need_h = ox != W or box[0] or box[2] != ox
    need_v = oy != H or box[1] or box[3] != oy
    hx, hn, hk = coeffs(W, box[0], box[2], ox)
    vy, vn, vk = coeffs(H, box[1], box[3], oy)
    y0, y1 = int(vy[0]), int(vy[-1] + vn[-1])
    cur = a.astype(np.int64)
    if need_h:
        cur = _pass(cur[y0:y1], hx, hk, 1).astype(np.int64)
        vy = vy - y0
    if need_v:
        cur = _pass(cur, vy, vk, 0)
    return cur.astype(np.uint8)
