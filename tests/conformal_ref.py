"""The written spec of split conformal prediction sets (uvc_amd/compact_conformal.py, uvc_conformal_scores / uvc_conformal_sets) in float64
NumPy, and the helpers the conformal tests share.

A row's valid logits are z_c, c in [0, C), float32; columns [C, ld) are never read.  p = softmax(z / T) over the valid columns.  Order:
descending z, ties by ascending index, -0 = +0, taken on the float32 logits; r_c in 1 .. C the rank of class c, M_c the sum of p_j over the
classes ranked ahead of it.  u in [0, 1], one per row (None: 1).  lac: s(c) = 1 - p_c; aps: s(c) = M_c + u p_c; raps: s(c) = M_c + u p_c +
lam max(0, r_c - k_reg).  Over the m rows whose label lies in [0, C): k = ceil((m + 1)(1 - alpha)) in exact rational arithmetic on alpha's
decimal string, qhat the k-th smallest s(y_i), +inf when k > m.  Sets: {c : s(c) <= qhat}."""
import math
from fractions import Fraction

import numpy as np

METHODS = ("lac", "aps", "raps")


def quantile_index(m, alpha):
    a = Fraction(str(alpha))
    if not 0 < a < 1 or m < 1:
        raise ValueError("0 < alpha < 1 and m >= 1")
    return math.ceil((m + 1) * (1 - a))


def class_scores(logits, C, method, u=None, T=1.0, lam=0.0, k_reg=0):
    """float64 s [n, C]."""
    z32 = np.asarray(logits, dtype=np.float32)[:, :C]
    n = z32.shape[0]
    z = z32.astype(np.float64) / float(T)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    if method == "lac":
        return 1.0 - p
    order = np.argsort(-z32, axis=1, kind="stable")                  # -(+0) = -0 = +0 in a comparison: ties keep their ascending index
    ps = np.take_along_axis(p, order, axis=1)
    ahead = np.concatenate([np.zeros((n, 1)), np.cumsum(ps, axis=1)[:, :-1]], axis=1)
    uu = np.ones((n, 1)) if u is None else np.asarray(u, dtype=np.float64).reshape(n, 1)
    s = ahead + uu * ps
    if method == "raps":
        s = s + float(lam) * np.maximum(0, np.arange(1, C + 1) - int(k_reg))[None, :]
    out = np.empty_like(s)
    np.put_along_axis(out, order, s, axis=1)
    return out


def all_class_scores(logits, C, u=None, T=1.0, lam=0.0, k_reg=0):
    """{method: s [n, C]} of the three methods from one softmax and one sort (class_scores' arithmetic, statement by statement)."""
    z32 = np.asarray(logits, dtype=np.float32)[:, :C]
    n = z32.shape[0]
    z = z32.astype(np.float64) / float(T)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    order = np.argsort(-z32, axis=1, kind="stable")
    ps = np.take_along_axis(p, order, axis=1)
    ahead = np.concatenate([np.zeros((n, 1)), np.cumsum(ps, axis=1)[:, :-1]], axis=1)
    uu = np.ones((n, 1)) if u is None else np.asarray(u, dtype=np.float64).reshape(n, 1)
    s = ahead + uu * ps
    aps, raps = np.empty_like(s), np.empty_like(s)
    np.put_along_axis(aps, order, s, axis=1)
    np.put_along_axis(raps, order, s + float(lam) * np.maximum(0, np.arange(1, C + 1) - int(k_reg))[None, :], axis=1)
    return dict(lac=1.0 - p, aps=aps, raps=raps)


def label_scores(logits, labels, C, method, u=None, T=1.0, lam=0.0, k_reg=0):
    """(scores float64 [n] with NaN at the rows that do not count, m)."""
    s = class_scores(logits, C, method, u, T, lam, k_reg)
    y = np.asarray(labels).astype(np.int64)
    keep = (y >= 0) & (y < C)
    out = np.full(s.shape[0], np.nan)
    out[keep] = s[keep, y[keep]]
    return out, int(keep.sum())


def qhat_of(scores, alpha):
    """The k-th smallest of the scores that count (NaN: not counted), +inf when k > m."""
    s = np.sort(scores[~np.isnan(scores)])
    k = quantile_index(len(s), alpha)
    return math.inf if k > len(s) else float(s[k - 1])


def sets(logits, qhat, C, method, u=None, T=1.0, lam=0.0, k_reg=0):
    """bool [n, C]."""
    s = class_scores(logits, C, method, u, T, lam, k_reg)
    return np.ones_like(s, dtype=bool) if qhat == math.inf else s <= qhat


def brute_class_scores(row, method, u=1.0, T=1.0, lam=0.0, k_reg=0):
    """One row, by the definition, in loops."""
    C = len(row)
    z = [float(np.float32(v)) for v in row]
    mx = max(z)
    e = [math.exp((v - mx) / T) if v != -math.inf else 0.0 for v in z]
    S = sum(e)
    p = [v / S for v in e]
    out = []
    for c in range(C):
        ahead = [j for j in range(C) if z[j] > z[c] or (z[j] == z[c] and j < c)]
        r = len(ahead) + 1
        M = sum(p[j] for j in ahead)
        if method == "lac":
            out.append(1.0 - p[c])
        else:
            out.append(M + u * p[c] + (lam * max(0, r - k_reg) if method == "raps" else 0.0))
    return out


def synthetic_bank(n, C, seed, scale=2.0):
    """(logits float32 [n, C], labels int64 [n]): labels drawn from softmax(z) -- the model is calibrated on its own data."""
    rng = np.random.default_rng(seed)
    z = (scale * rng.standard_normal((n, C))).astype(np.float32)
    e = np.exp(z.astype(np.float64) - z.max(axis=1, keepdims=True))
    cdf = np.cumsum(e / e.sum(axis=1, keepdims=True), axis=1)
    y = (rng.random((n, 1)) > cdf).sum(axis=1).clip(0, C - 1)
    return z, y.astype(np.int64)
