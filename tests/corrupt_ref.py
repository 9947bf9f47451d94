"""The corruption spec of uvc_amd/compact_corrupt.py restated for the tests: numpy and tests/noise_refs.py only, nothing of uvc_amd.

``loops`` is the statement element by element (tiny inputs).  The vectorised functions give, next to the float64 value BEFORE the clamp, what a
float32 error bar needs: ``T``, the sum of the absolute values of the terms of the float64 formula at that element, and for the Gaussian kinds
the radius ``r`` of the Box-Muller pair.  ``check`` is the acceptance rule of every kernel test: inside ``[lo_c, hi_c]`` everywhere, within
the bar of the clamped spec, and exactly ``lo_c`` / ``hi_c`` where the spec lies beyond a bound by more than the bar.

Brightness.  p_c = clip(x_c s_c + m_c), V = max_c p_c, s = V' / V, out_c = (p_c s - m_c) / s_c.  A float32 evaluation carries the rounding of
p_c (relative to T_c = |x_c s_c| + |m_c|, not to p_c: the sum cancels for dark pixels) and, through s, that of V (relative to T_V of the
channel that attains the maximum): d(p_c s) = s dp_c + p_c V' dV / V^2, so T = ((T_c + (p_c / V) T_V) V' / V + |m_c|) / s_c.  At V = 0 the
statement jumps (every channel becomes V'), so pixels whose unclipped maximum lies within ``BRIGHT_EDGE`` of 0 are left out (``skip``).
"""
import numpy as np

import noise_refs as NR

KINDS = ("gaussian_noise", "speckle_noise", "impulse_noise", "brightness", "contrast", "gaussian_blur", "defocus_blur", "pixelate")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
TWO_PI_F32 = np.float32(6.28318530717958647692)
BRIGHT_EDGE = 2.0 ** -18
EPS32 = 2.0 ** -24


def stats(C):
    return MEAN[:C] if C <= 3 else MEAN + (0.45,), STD[:C] if C <= 3 else STD + (0.25,)


def bounds(mean, std):
    """(lo, hi) float32 [C]: the normalised 0 and 1, formed in float64 and rounded once."""
    m, s = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    return ((0 - m) / s).astype(np.float32), ((1 - m) / s).astype(np.float32)


def images(shape, seed, mean, std):
    """float32 [B, C, H, W] inside [lo_c, hi_c]: normalised uniform pixels, every eighth pixel black, white or one saturated channel."""
    rng = np.random.default_rng(seed)
    B, C, H, W = shape
    p = rng.random(shape)
    special = rng.integers(0, 24, (B, 1, H, W))
    p = np.where(special == 0, 0.0, np.where(special == 1, 1.0, p))
    p[:, 0] = np.where(special[:, 0] == 2, 1.0, p[:, 0])
    m, s = np.asarray(mean).reshape(1, C, 1, 1), np.asarray(std).reshape(1, C, 1, 1)
    x = ((p - m) / s).astype(np.float32)
    lo, hi = bounds(mean, std)
    return np.clip(x, lo.reshape(1, C, 1, 1), hi.reshape(1, C, 1, 1))


def channel_of(e, C, HW):
    return (e // HW) % C


def normals(seed, stream, gstart, n):
    """(z, r) float64 [n] of the global indices gstart .. gstart + n - 1"""
    gstart = int(gstart)
    j0, j1 = gstart >> 1, (gstart + n - 1) >> 1
    u1 = NR.uniforms(seed, stream, 0, j1 - j0 + 1, start=j0).astype(np.float64)
    u2 = NR.uniforms(seed, stream, 1, j1 - j0 + 1, start=j0)
    r = np.sqrt(-2.0 * np.log(u1))
    t = (TWO_PI_F32 * u2).astype(np.float32).astype(np.float64)
    idx = np.arange(n) + (gstart & 1)
    pair, odd = idx >> 1, (idx & 1) == 1
    return np.where(odd, r[pair] * np.sin(t[pair]), r[pair] * np.cos(t[pair])), r[pair]


def noise_flat(x_flat, e0, kind, a, mean, std, C, HW, seed, stream, gbase):
    """Elements e0 .. e0 + len - 1 of a batch whose element 0 has the global index gbase: (ref, T, zterm) float64; impulse: (ref, None, None)
    with ref already lo / hi / x.  zterm: (a / s_c) |factor| ulp32(r), what one ulp of r in z moves the output by."""
    n = len(x_flat)
    x = x_flat.astype(np.float64)
    c = channel_of(e0 + np.arange(n, dtype=np.int64), C, HW)
    m, s = np.asarray(mean, np.float64)[c], np.asarray(std, np.float64)[c]
    if kind == "impulse_noise":
        lo, hi = bounds(mean, std)
        u = NR.uniforms(seed, stream, 2, n, start=int(gbase) + int(e0)).astype(np.float64)
        return np.where(u < a / 2, lo.astype(np.float64)[c], np.where(u < a, hi.astype(np.float64)[c], x)), None, None
    z, r = normals(seed, stream, int(gbase) + int(e0), n)
    ulp_r = 2.0 ** (np.floor(np.log2(np.maximum(r, 2.0 ** -126))) - 23)
    if kind == "gaussian_noise":
        return x + z * (a / s), np.abs(x) + np.abs(z) * (a / s), (a / s) * ulp_r
    return x + z * (a * x + a * m / s), np.abs(x) + np.abs(z) * (np.abs(a * x) + np.abs(a * m / s)), (a / s) * np.abs(x * s + m) * ulp_r


def brightness(x, a, mean, std):
    """(ref, T, skip) of float32 x [B, C, H, W]"""
    C = x.shape[1]
    m, s = np.asarray(mean, np.float64).reshape(1, C, 1, 1), np.asarray(std, np.float64).reshape(1, C, 1, 1)
    x = x.astype(np.float64)
    raw = x * s + m
    p = np.clip(raw, 0, 1)
    Tp = np.abs(x * s) + np.abs(m)
    V = p.max(axis=1, keepdims=True)
    TV = np.take_along_axis(Tp, p.argmax(axis=1)[:, None], axis=1)
    Vn = np.minimum(V + a, 1.0)
    safe = np.where(V > 0, V, 1.0)
    pn = np.where(V > 0, p * Vn / safe, Vn)
    T = np.where(V > 0, ((Tp + p / safe * TV) * Vn / safe + np.abs(m)) / s, (np.abs(Vn) + np.abs(m)) / s)
    skip = np.broadcast_to(np.abs(raw.max(axis=1, keepdims=True)) < BRIGHT_EDGE, x.shape)
    return (pn - m) / s, T, skip


def image_mean(x, mean, std):
    C = x.shape[1]
    m, s = np.asarray(mean, np.float64).reshape(1, C, 1, 1), np.asarray(std, np.float64).reshape(1, C, 1, 1)
    p = x.astype(np.float64) * s + m
    return p.mean(axis=(1, 2, 3)), np.abs(p).max(axis=(1, 2, 3))


def contrast(x, a, mean, std, mu):
    """(ref, T) with the image means mu [B] as given"""
    C = x.shape[1]
    m, s = np.asarray(mean, np.float64).reshape(1, C, 1, 1), np.asarray(std, np.float64).reshape(1, C, 1, 1)
    x, mu = x.astype(np.float64), np.asarray(mu, np.float64).reshape(-1, 1, 1, 1)
    return a * x + (1 - a) * (mu - m) / s, np.abs(a * x) + np.abs((1 - a) * mu / s) + np.abs((1 - a) * m / s)


def gaussian_taps(sigma):
    R = int(4 * sigma + 0.5)
    if R == 0:
        return np.ones(1, np.float32)
    w = np.array([np.exp(-(k * k) / (2.0 * sigma * sigma)) for k in range(-R, R + 1)], np.float64)
    return (w / w.sum()).astype(np.float32)


def disk_taps(r):
    K = 2 * r + 1
    inside = np.array([[(dy - r) ** 2 + (dx - r) ** 2 <= r * r for dx in range(K)] for dy in range(K)])
    return np.where(inside, np.float32(1.0 / int(inside.sum())), np.float32(0.0)).astype(np.float32)


def filter_axis(x, taps, axis):
    """(sum_k w_k x[clamp(i + k - R)], sum_k |w_k x[..]|) along ``axis`` in float64"""
    x = x.astype(np.float64)
    n, R = x.shape[axis], len(taps) // 2
    out, mag = np.zeros_like(x), np.zeros_like(x)
    for k, w in enumerate(taps):
        v = np.take(x, np.clip(np.arange(n) + k - R, 0, n - 1), axis=axis) * float(w)
        out += v
        mag += np.abs(v)
    return out, mag


def stencil(x, taps):
    """(sum, sum of magnitudes, the number of non-zero taps) of the dense filter, borders clamped"""
    x = x.astype(np.float64)
    H, W = x.shape[2:]
    r = taps.shape[0] // 2
    out, mag = np.zeros_like(x), np.zeros_like(x)
    for dy in range(-r, r + 1):
        rows = np.take(x, np.clip(np.arange(H) + dy, 0, H - 1), axis=2)
        for dx in range(-r, r + 1):
            w = float(taps[dy + r, dx + r])
            if w != 0:
                v = np.take(rows, np.clip(np.arange(W) + dx, 0, W - 1), axis=3) * w
                out += v
                mag += np.abs(v)
    return out, mag, int((taps != 0).sum())


def pixelate(x, k):
    """(the cell means, the cell means of |x|, the cell sizes), each of x's shape"""
    x = x.astype(np.float64)
    B, C, H, W = x.shape
    out, mag, cnt = np.empty_like(x), np.empty_like(x), np.empty_like(x)
    for y0 in range(0, H, k):
        for x0 in range(0, W, k):
            cell = x[:, :, y0:y0 + k, x0:x0 + k]
            out[:, :, y0:y0 + k, x0:x0 + k] = cell.mean(axis=(2, 3), keepdims=True)
            mag[:, :, y0:y0 + k, x0:x0 + k] = np.abs(cell).mean(axis=(2, 3), keepdims=True)
            cnt[:, :, y0:y0 + k, x0:x0 + k] = cell.shape[2] * cell.shape[3]
    return out, mag, cnt


def loops(x, kind, a, mean, std, seed=0, stream=0, index0=0):
    """float64 of x's shape BEFORE the clamp: the statement element by element (tiny inputs only)."""
    B, C, H, W = x.shape
    xd = x.astype(np.float64)
    out = np.empty_like(xd)
    cl = lambda v, n: min(max(v, 0), n - 1)
    lo, hi = bounds(mean, std)
    if kind in KINDS[:3]:
        n = x.size
        g0 = index0 * C * H * W
        if kind != "impulse_noise":
            z, _ = normals(seed, stream, g0, n)
        else:
            u = NR.uniforms(seed, stream, 2, n, start=g0)
    for b in range(B):
        mu = sum(xd[b, c, y, w] * std[c] + mean[c] for c in range(C) for y in range(H) for w in range(W)) / (C * H * W)
        for c in range(C):
            for y in range(H):
                for w in range(W):
                    e = ((b * C + c) * H + y) * W + w
                    v, p = xd[b, c, y, w], xd[b, c, y, w] * std[c] + mean[c]
                    if kind == "gaussian_noise":
                        o = (p + a * z[e] - mean[c]) / std[c]
                    elif kind == "speckle_noise":
                        o = (p + a * p * z[e] - mean[c]) / std[c]
                    elif kind == "impulse_noise":
                        o = float(lo[c]) if u[e] < a / 2 else float(hi[c]) if u[e] < a else v
                    elif kind == "brightness":
                        ps = [min(max(xd[b, k, y, w] * std[k] + mean[k], 0.0), 1.0) for k in range(C)]
                        V = max(ps)
                        Vn = min(V + a, 1.0)
                        o = ((ps[c] * Vn / V if V > 0 else Vn) - mean[c]) / std[c]
                    elif kind == "contrast":
                        o = ((p - mu) * a + mu - mean[c]) / std[c]
                    elif kind == "gaussian_blur":
                        o = None
                    elif kind == "defocus_blur":
                        r, t = int(a), disk_taps(int(a))
                        o = 0.0
                        for dy in range(-r, r + 1):
                            for dx in range(-r, r + 1):
                                o += float(t[dy + r, dx + r]) * xd[b, c, cl(y + dy, H), cl(w + dx, W)]
                    else:
                        k = int(a)
                        cell = xd[b, c, y // k * k:y // k * k + k, w // k * k:w // k * k + k]
                        o = cell.sum() / cell.size
                    out[b, c, y, w] = 0.0 if o is None else o
    if kind == "gaussian_blur":
        t = gaussian_taps(a)
        R = len(t) // 2
        mid = np.empty_like(xd)
        for idx in np.ndindex(*x.shape):
            b, c, y, w = idx
            mid[idx] = sum(float(t[k]) * xd[b, c, y, cl(w + k - R, W)] for k in range(len(t)))
        mid = mid.astype(np.float32).astype(np.float64)
        for idx in np.ndindex(*x.shape):
            b, c, y, w = idx
            out[idx] = sum(float(t[k]) * mid[b, c, cl(y + k - R, H), w] for k in range(len(t)))
    return out


def clamp32(ref, mean, std):
    """float32: the spec's last step on float64 values of shape [B, C, H, W]"""
    lo, hi = bounds(mean, std)
    C = ref.shape[1]
    return np.clip(ref, lo.astype(np.float64).reshape(1, C, 1, 1), hi.astype(np.float64).reshape(1, C, 1, 1)).astype(np.float32)


def check(got, ref, bar, lo, hi, skip=None):
    """The acceptance rule on arrays of one shape (lo / hi: float32 broadcastable): returns the largest |got - clamp(ref)| / bar; asserts the
    range and the exact clamp where the spec is beyond a bound by more than the bar."""
    got64, lo64, hi64 = got.astype(np.float64), np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    keep = np.ones(ref.shape, bool) if skip is None else ~skip
    assert not np.isnan(got).any()
    assert (got64 >= lo64).all() and (got64 <= hi64).all()
    above, below = keep & (ref > hi64 + bar), keep & (ref < lo64 - bar)
    assert (got64[above] == np.broadcast_to(hi64, ref.shape)[above]).all()
    assert (got64[below] == np.broadcast_to(lo64, ref.shape)[below]).all()
    err = np.abs(got64 - np.clip(ref, lo64, hi64))
    floor = np.where(bar > 0, bar, 1.0)
    ratio = np.where(bar > 0, err / floor, np.where(err == 0, 0.0, np.inf))
    return float(ratio[keep].max()) if keep.any() else 0.0
