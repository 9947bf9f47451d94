"""Fixtures and float64 helpers of the out-of-distribution tests (tests/test_ood_cpu.py, tests/test_ood_gpu.py)."""
import numpy as np
import torch

from uvc_amd import compact_ood as OD

TIE_ID, TIE_OOD = [1, 2, 2, 3, 3, 3], [0, 2, 3, 3]          # 13 / 24 by the tie formula (and by sklearn)
# (n, C, D, n_ood) with seed 1: float64 Mahalanobis AUROC 1.0 / 0.9427 (rmd 0.9031) / 1.0
FIXTURES = [(600, 10, 64, 200), (650, 3, 8, 130), (1000, 100, 192, 300)]
GAP = 1e-4                                                   # argmin is compared where the relative top-2 gap exceeds this
GAP_ROWS = 0.01                                              # and at most this share of the rows may be left out
_CACHE = {}


def gauss_fixture(seed, n, C, D, n_ood):
    """dict(x [n, D], y [n], xt [n // 2, D], yt, xo [n_ood, D]) float32 / int64 tensors: class means 2 N(0, 1), one covariance factor
    Lm = Q Q^T + I / 2 with Q = N(0, 1) / sqrt(D), labels cycling, OOD rows 1.5 times as wide around half the mean of the class means."""
    key = (seed, n, C, D, n_ood)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        mu = 2.0 * rng.standard_normal((C, D))
        Q = rng.standard_normal((D, D)) / np.sqrt(D)
        Lm = Q @ Q.T + 0.5 * np.eye(D)
        y = np.arange(n) % C
        x = mu[y] + rng.standard_normal((n, D)) @ Lm.T
        yt = np.arange(n // 2) % C
        xt = mu[yt] + rng.standard_normal((n // 2, D)) @ Lm.T
        xo = 0.5 * mu.mean(0) + 1.5 * rng.standard_normal((n_ood, D)) @ Lm.T
        f = lambda a: torch.from_numpy(a.astype(np.float32))
        _CACHE[key] = dict(x=f(x), y=torch.from_numpy(y), xt=f(xt), yt=torch.from_numpy(yt), xo=f(xo))
    return _CACHE[key]


def bank_of(features, labels, classes, logits=None, num_classes=None):
    """A raw bank dict; without logits, zeros of ``num_classes`` (default: classes rounded up to 8) columns."""
    n = features.shape[0]
    if logits is None:
        logits = torch.zeros(n, num_classes or -(-classes // 8) * 8)
    return OD.make_ood_bank(features, logits, labels, classes, dataset="fixture", split="train")


def host_detector(features, labels, classes, shrinkage=1e-6, knn=True):
    """A detector dict made on the host alone: ``reference_fit`` rounded once to float32 (no device)."""
    g = OD.reference_fit(features, labels, classes, shrinkage)
    det = dict(version=1, embed_dim=int(features.shape[1]), data_classes=int(classes), num_classes=-(-classes // 8) * 8, meta={}, counts=g["counts"],
               means=g["means"].float(), mean0=g["mean0"].float(), scatter=g["scatter"].float(), whiten=g["whiten"].float().contiguous(),
               whiten0=g["whiten0"].float().contiguous(), wmeans=g["wmeans"].float().contiguous(), shrinkage=float(shrinkage), knn_seed=0,
               knn_fraction=1.0 if knn else 0.0)
    if knn:
        det["knn_bank"] = torch.nn.functional.normalize(features.float(), dim=1, eps=1e-12)
    return det


def moments(x, y, C):
    """(counts int64 [C], means float64 [C, D], scatter float64 [D, D]) on the host: the rows with a label in [0, C)"""
    x, y = x.double().cpu(), y.to(torch.int64).cpu()
    keep = (y >= 0) & (y < C)
    x, y = x[keep], y[keep]
    counts = torch.bincount(y, minlength=C)
    means = torch.zeros(C, x.shape[1], dtype=torch.float64).index_add_(0, y, x) / counts.clamp_min(1)[:, None].double()
    c = x - means[y]
    return counts, means, c.T @ c


def top2_gap(d2):
    """float64 [n]: (d2_2 - d2_1) / d2_2 of the two smallest distances of every row (1 with a single candidate)."""
    if d2.shape[1] < 2:
        return torch.ones(d2.shape[0], dtype=torch.float64)
    two = torch.topk(d2, 2, dim=1, largest=False)[0]
    gap = (two[:, 1] - two[:, 0]) / two[:, 1]
    return torch.where(torch.isfinite(two[:, 1]), gap, torch.ones_like(gap))


def auroc_interval(id_ref, ood_ref, bar):
    """(lo, hi): the AUROC when every (ID, OOD) pair closer than 2 bar counts once as a loss and once as a win."""
    si = np.asarray(id_ref, dtype=np.float64)
    so = np.sort(np.asarray(ood_ref, dtype=np.float64))
    sure = np.searchsorted(so, si - 2 * bar, side="left")                # s_o < s_i - 2 bar
    maybe = np.searchsorted(so, si + 2 * bar, side="right")              # s_o <= s_i + 2 bar
    pairs = float(len(si)) * float(len(so))
    return float(sure.sum()) / pairs, float(maybe.sum()) / pairs


def logits_case(rows, C, ld, kind, seed):
    """float32 [rows, ld]: ``normal`` N(0, 3), ``large`` of magnitude 3e4, ``tied`` rows of one value (and rows with two tied maxima);
    NaN in the padding columns [C, ld)."""
    g = torch.Generator().manual_seed(seed)
    z = 3.0 * torch.randn(rows, ld, generator=g)
    if kind == "large":
        z = 3e4 * torch.sign(z) + 10.0 * torch.randn(rows, ld, generator=g)
    elif kind == "tied":
        z = torch.round(z)
        z[::2] = z[::2, :1]
    z[:, C:] = float("nan")
    return z.float().contiguous()


def logit_refs(z, C, T):
    """(msp, maxlogit, energy, entropy) float64 of the valid columns, and max |z| per row (the energy's scale)."""
    bank = dict(logits=z[:, :C])
    r = OD.reference_scores(dict(data_classes=C), bank, OD.LOGIT_METHODS, temperature=T)
    return [r[m] for m in OD.LOGIT_METHODS], z[:, :C].double().abs().max(dim=1)[0]
