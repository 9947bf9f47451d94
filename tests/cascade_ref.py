"""What the cascade tests share (tests/test_cascade_cpu.py, tests/test_cascade_gpu.py; nothing here needs a GPU): a direct float64 softmax
in plain Python, the brute-force curve -- one loop over every threshold --, logits cases, synthetic banks and the bars of the scores."""
import math

import torch

from uvc_amd import compact_cascade as CS

U = 2.0 ** -24                                       # the unit roundoff of float32
INF = float("inf")
NAN = float("nan")
_CACHE = {}


# ---- the scores, directly ---------------------------------------------------------------------------------------------------------------
def direct_scores(z, C, T, kind):
    """float64 [n] by one Python loop per row: softmax of the first C logits over T with ``math.exp``, then the score's definition."""
    out = []
    for row in torch.as_tensor(z)[:, :C].double().tolist():
        if any(math.isnan(v) for v in row) or max(row) in (INF, -INF):
            out.append(NAN)
            continue
        m = max(row)
        e = [math.exp((v - m) / T) for v in row]
        S = math.fsum(e)
        p = sorted((v / S for v in e), reverse=True)
        if kind == "msp":
            out.append(p[0])
        elif kind == "margin":
            out.append(p[0] - (p[1] if C > 1 else 0.0))
        else:
            out.append(1.0 if C == 1 else 1.0 + math.fsum(v * math.log(v) for v in p if v > 0.0) / math.log(C))
    return torch.tensor(out, dtype=torch.float64)


def logits_case(n, C, ld, seed, scale=3.0):
    """float32 [n, ld] on the host, built once per key: ``scale`` randn in the valid columns, NaN behind them; from 8 rows on, row 2 ties its
    maximum in two columns (the first one is lower), row 3 is all equal, row 5 holds -inf in a third of its columns."""
    key = (n, C, ld, seed, scale)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(seed)
        z = torch.full((n, ld), NAN)
        z[:, :C] = scale * torch.randn(n, C, generator=g)
        if n >= 8:
            if C > 1:
                a, b = sorted(torch.randperm(C, generator=g)[:2].tolist())
                z[2, a] = z[2, b] = float(z[2, :C].max()) + 1.0
            z[3, :C] = 0.25
            z[5, :C][torch.rand(C, generator=g) < 0.33] = -INF
            z[5, C // 2] = 1.0
        _CACHE[key] = z.contiguous()
    return _CACHE[key]


def score_bars(z, C, T, kind, eps):
    """``(reference float64 [n], bar float64 [n])`` of the float32 score of uvc_cascade_decide, derived from the spec's operations.  With m
    the row's maximum the kernel forms d_c = z_c - m (one float32 subtraction: relative error u = 2^-24), q_c = d_c / T (one float32 division:
    u), e_c = expf(q_c) (relative error at most ``eps``, measured), float64 sums and ONE rounding to float32.  So the argument of the
    exponential is off by |a_c| <= 2 u |q_c| and e^_c = e_c (1 + eta_c) with |eta_c| <= eps + 2 u |q_c| -- except at the maximum, where
    d = q = 0 and expf(0) = 1 exactly.  With E = sum_j p_j |eta_j|, to first order p^_c = p_c (1 + eta_c - sum_j p_j eta_j), hence
        msp      |err| <= p_1 E
        margin   |err| <= p_1 E + p_2 (|eta_2| + E)
        entropy  H' = sum_c p_c q_c - log S:  |err| <= sum_c p_c |q_c| (|eta_c| + E) + sum_c p_c |a_c| + E,  divided by log C
    each times 1.01 (the products of errors), plus u |score| (the rounding), plus 1e-30 (exponentials below the float32 normal range), plus
    the float64 evaluation of both sides: sums of C terms of one sign, a lane's C / 64 in sequence and a butterfly in the kernel, pairwise in
    the reference, then a handful of operations on values of at most 2 -- 2^-52 (C / 64 + log2 C + 16) 2, which is 1.8e-14 at C = 1000 and
    matters only where a score is 0 (the uniform row's entropy and margin)."""
    zz = torch.as_tensor(z)[:, :C].double()
    ref = CS.reference_scores(z, C, T, kind)
    q = (zz - zz.max(dim=1, keepdim=True)[0]) / T
    p = torch.softmax(q, dim=1)
    aq = torch.where(p > 0, q.abs(), torch.zeros_like(q))
    a = 2 * U * aq
    eta = torch.where(aq > 0, eps + a, torch.zeros_like(a))                    # (q = 0: the maximum and its ties, expf(0) = 1)
    E = (p * eta).sum(dim=1)
    top = torch.topk(p, min(2, C), dim=1)[0]
    if kind == "msp":
        err = top[:, 0] * E
    elif kind == "margin":
        p2 = top[:, 1] if C > 1 else torch.zeros_like(E)
        eta2 = torch.where(p > 0, eta, torch.zeros_like(eta)).max(dim=1)[0]                                    # (at least the second entry's)
        err = top[:, 0] * E + p2 * (eta2 + E)
    else:
        err = ((p * aq * (eta + E[:, None])).sum(dim=1) + (p * a).sum(dim=1) + E) / math.log(C) if C > 1 else torch.zeros_like(E)
    return ref, 1.01 * err + U * ref.abs() + 1e-30 + 2.0 ** -52 * (C / 64 + math.log2(max(C, 2)) + 16) * 2


# ---- the curve, by a loop over every threshold ------------------------------------------------------------------------------------------
def brute_curve(score, top1_small, top1_large, labels, C, macs_small, macs_large):
    """[{"threshold", "kept", "correct", "defer_rate", "accuracy", "macs"}] for tau = +inf and every distinct float32 score, descending:
    ``score >= tau`` row by row."""
    s = [float(v) for v in torch.as_tensor(score).float().tolist()]
    ts, tl, y = (torch.as_tensor(t).tolist() for t in (top1_small, top1_large, labels))
    n = len(s)
    rows = [j for j in range(n) if 0 <= y[j] < C]
    out = []
    for tau in [INF] + sorted(set(s), reverse=True):
        kept = [j for j in range(n) if s[j] >= tau]
        keep = set(kept)
        correct = sum(1 for j in rows if (ts[j] if j in keep else tl[j]) == y[j])
        rate = (n - len(kept)) / n
        out.append(dict(threshold=tau, kept=len(kept), correct=correct, defer_rate=rate, accuracy=correct / len(rows), macs=macs_small + rate * macs_large))
    return out


def brute_choose(points, large_top1, match_large=None, target_accuracy=None, max_macs=None):
    """the operating point the selectors' definitions give, by a loop: the cheapest point that is accurate enough, or the most accurate
    point that is cheap enough (the cheaper among equals); None when no point qualifies"""
    if max_macs is not None:
        ok = [p for p in points if p["macs"] <= max_macs]
        return min(ok, key=lambda p: (-p["accuracy"], p["macs"])) if ok else None
    want = large_top1 - match_large if match_large is not None else target_accuracy
    ok = [p for p in points if p["accuracy"] >= want]
    return min(ok, key=lambda p: p["macs"]) if ok else None


def synthetic_banks(n=300, C=5, wide=8, seed=0, tied=True):
    """(small bank, large bank): random logits of heads ``wide`` and ``wide + 4`` columns wide (so the strides differ), the small model right
    about 60 % of the time and the large one 80 %, a few labels outside [0, C), and with ``tied`` many rows sharing a score (their logits
    are copies of one another's)."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, C, (n,), generator=g)

    def head(width, right, sharp):
        z = torch.randn(n, width, generator=g)
        hit = torch.rand(n, generator=g) < right
        col = torch.where(hit, y, torch.randint(0, C, (n,), generator=g))
        z[torch.arange(n), col] += sharp * torch.rand(n, generator=g) * hit + 1.0
        z[:, C:] = 50.0                                                        # padding columns that would win if they took part
        return z
    zs, zl = head(wide, 0.6, 4.0), head(wide + 4, 0.8, 6.0)
    if tied:
        zs[n // 2:n // 2 + n // 4] = zs[:n // 4]                               # a quarter of the rows repeat another quarter's logits
    y[7], y[11] = -1, C
    mk = lambda z: dict(logits=z.float().contiguous(), labels=y.clone(), data_classes=C, num_classes=z.shape[1], meta=dict(img_size=64))
    return mk(zs), mk(zl)


def planted_banks(n=200, C=4, rate=0.35):
    """(small bank, large bank, the planted defer rate): the large model is right everywhere; the small model is right with a confident row
    exactly on the first ``n - rate n`` rows and wrong with a flat row on the others."""
    y = torch.arange(n) % C
    hard = torch.arange(n) >= n - int(round(rate * n))
    zl = torch.zeros(n, 8)
    zl[torch.arange(n), y] = 9.0
    zs = torch.zeros(n, 8)
    zs[torch.arange(n), torch.where(hard, (y + 1) % C, y)] = torch.where(hard, torch.tensor(0.5), 4.0 + torch.arange(n) * 0.01)
    mk = lambda z: dict(logits=z, labels=y.clone(), data_classes=C, num_classes=8, meta={})
    return mk(zs), mk(zl), int(hard.sum()) / n


# ---- batches for the micro exports ----------------------------------------------------------------------------------------------------------
def cluster_batch(seed, per=6, side=64):
    """float32 [2 per, 3, side, side] under the CIFAR preset's normalisation, two clusters interleaved: near-black images (the micro exports
    are unsure of them) and flat green / blue ones (they are surer): the scores fall in two groups with a wide gap between them."""
    import numpy as np
    import knn_ref as KR
    rng = np.random.default_rng(seed)
    dark = np.clip(10 + rng.integers(-8, 9, (per, side, side, 3)), 0, 255).astype(np.uint8)
    img, y = KR.colour_images(3 * per, seed, side=side)
    flat = img[y != 0][:per]
    both = np.stack([dark, flat], axis=1).reshape(2 * per, side, side, 3)
    return (torch.from_numpy(both).permute(0, 3, 1, 2).float() / 255 - 0.5) / 0.5


def widest_gap(scores):
    """(tau, gap): the midpoint and the width of the widest gap between consecutive sorted scores in the 20 - 80 % range of the batch"""
    s = torch.sort(torch.as_tensor(scores).double())[0]
    n = s.shape[0]
    lo, hi = int(0.2 * n), int(0.8 * n)
    gaps = s[lo + 1:hi + 1] - s[lo:hi]
    j = int(gaps.argmax())
    return float((s[lo + j] + s[lo + j + 1]) / 2), float(gaps[j])
