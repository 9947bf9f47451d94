"""Two compact models on one split: what did the second change relative to the first?

    python -m uvc_amd.compact_compare diff --bank_a A.pt --bank_b B.pt [--topk 5] [--worst_images 20] [--worst_classes 10] [--cka 1]
                                           [--chunk_rows N] [--output diff.pt]
    python -m uvc_amd.compact_compare run  --a A.compact.pt --b B.compact.pt --dataset cifar10|cifar100|imagenet --data_dir D [--split test]
                                           [--bank_a A.pt] [--bank_b B.pt] <diff's flags>

``diff`` needs no model and no dataset: it takes any two bank dicts that hold ``logits``, ``labels``, ``data_classes`` and ``num_classes``
(``compact_calibrate logits`` and ``compact_ood bank`` both write them) of the SAME split in the same order.  ``run`` loads both files,
walks the split ONCE with one ``features(normalize=False)`` call per model and batch, writes each bank as ``compact_ood bank`` would for
that file alone when asked to, and then does what ``diff`` does.  "Dense against pruned", "pruned against fine-tuned" and "student against
teacher" are all "file A against file B" (``compact export`` turns a dense checkpoint into a compact file).

Per image, from the first C = ``data_classes`` logits of both models, all in one read of the two matrices (uvc_logits_pair_stats): with m
the FIRST maximum of a row, ``l_c = z_c - m - log sum exp(z - m)`` and ``p_c = exp(l_c)``,

    top1          the first maximum's column                         conf      p at the top-1
    kl_ab         sum_c p_a,c (l_a,c - l_b,c)  (kl_ba: swapped)      tv        1/2 sum_c |p_a,c - p_b,c|
    js            1/2 KL(a | mix) + 1/2 KL(b | mix), mix = (p_a + p_b) / 2, through l_m = max(l_a, l_b) + log1p(exp(-|l_a - l_b|)) - log 2
    nll           -l_y                                               rank      #{c : z_c > z_y or (z_c = z_y and c < y)}, 0 = the top-1
    rank_b_top1a  the rank of A's top-1 column in B's row            rank_a_top1b  likewise

The divergences are sums of differences of LOG-probabilities, so they stay finite where ``log(p_a / p_b)`` is +-inf: a 200-logit gap gives
KL ~ 200, JS ~ log 2, TV ~ 1.  The record (one JSON line) holds prediction churn and the negative / positive flips (Milani Fard et al.
2016, Yan et al. 2021), the exact McNemar test on the discordant pairs, the mean divergences and agreement (Stanton et al. 2021), the
classes whose recall fell most and the images whose prediction moved most (Hooker et al. 2019), and linear CKA of the readout features
(Kornblith et al. 2019; ``ops.linear_cka``).  The integer tables are ``torch.bincount`` of int64 keys, exact.  ``reference_pair_stats``,
``reference_tables``, ``reference_mcnemar``, ``reference_cka`` and ``reference_compare`` are the written specs (plain float64 on the
host); the commands take ``stats=`` / ``cka_fn=`` and run on the CPU with them.
"""
from __future__ import annotations

import argparse
import json
import math
import time
from fractions import Fraction
from typing import Optional, Sequence

import torch

from . import _lib as L
from . import compact as CP
from . import compact_tools as TL

STATS = ("top1_a", "top1_b", "conf_a", "conf_b", "kl_ab", "kl_ba", "js", "tv", "nll_a", "nll_b", "rank_a", "rank_b", "rank_b_top1a", "rank_a_top1b")
INT_STATS = ("top1_a", "top1_b", "rank_a", "rank_b", "rank_b_top1a", "rank_a_top1b")
BANK_KEYS = ("logits", "labels", "data_classes", "num_classes")
MATRIX_KEYS = ("confusion_a", "confusion_b", "moved")
MAX_MATRIX = 1 << 26                                 # the [C, C] tables are skipped beyond this many entries


# ---- written specs ----------------------------------------------------------------------------------------------------------------
def _rank(z, col):
    """int64 [n]: #{c : z_c > z_col or (z_c = z_col and c < col)} per row of float64 ``z`` [n, C] for the int64 columns ``col`` [n]."""
    t = z.gather(1, col[:, None])
    c = torch.arange(z.shape[1])[None, :]
    return ((z > t) | ((z == t) & (c < col[:, None]))).sum(dim=1)


def reference_pair_stats(za, zb, labels, C):
    """``{name: [n]}`` over ``STATS`` in float64 / int64 on the host, from columns [0, C) of the logits as given (float32 read as float64).
    The first maximum is ``argmax`` with the lower column among equals; ``0 log 0 = 0``.  A label outside [0, C) (or ``labels=None``): NLL
    NaN, ``rank_a = rank_b = -1``.  A NaN in a valid column of either row: every float of the row NaN, every integer -1."""
    C = int(C)
    za, zb = torch.as_tensor(za)[:, :C].double().cpu(), torch.as_tensor(zb)[:, :C].double().cpu()
    n = za.shape[0]
    y = torch.full((n,), -1, dtype=torch.int64) if labels is None else torch.as_tensor(labels).to(torch.int64).cpu()
    bad = torch.isnan(za).any(dim=1) | torch.isnan(zb).any(dim=1)
    za, zb = torch.where(bad[:, None], torch.zeros_like(za), za), torch.where(bad[:, None], torch.zeros_like(zb), zb)
    cols = torch.arange(C)[None, :]
    first = lambda z: torch.where(z == z.max(dim=1, keepdim=True)[0], cols, C).min(dim=1)[0]
    ta, tb = first(za), first(zb)
    la, lb = torch.log_softmax(za, dim=1), torch.log_softmax(zb, dim=1)
    pa, pb = la.exp(), lb.exp()
    lm = torch.maximum(la, lb) + torch.log1p(torch.exp(-(la - lb).abs())) - math.log(2.0)
    term = lambda p, d: torch.where(p > 0, p * d, torch.zeros_like(p)).sum(dim=1)
    counted = (y >= 0) & (y < C)
    yc = torch.where(counted, y, torch.zeros_like(y))
    nan = torch.full((n,), float("nan"), dtype=torch.float64)
    out = dict(top1_a=ta, top1_b=tb, conf_a=pa.max(dim=1)[0], conf_b=pb.max(dim=1)[0], kl_ab=term(pa, la - lb), kl_ba=term(pb, lb - la),
               js=(0.5 * term(pa, la - lm) + 0.5 * term(pb, lb - lm)).clamp_min(0.0), tv=0.5 * (pa - pb).abs().sum(dim=1),
               nll_a=torch.where(counted, -la.gather(1, yc[:, None])[:, 0], nan), nll_b=torch.where(counted, -lb.gather(1, yc[:, None])[:, 0], nan),
               rank_a=torch.where(counted, _rank(za, yc), -1), rank_b=torch.where(counted, _rank(zb, yc), -1),
               rank_b_top1a=_rank(zb, ta), rank_a_top1b=_rank(za, tb))
    for k in STATS:
        out[k] = torch.where(bad, torch.full_like(out[k], -1) if k in INT_STATS else nan, out[k])
    return out


def reference_tables(top1_a, top1_b, rank_a, rank_b, labels, C, matrices=True):
    """``{"per_class": int64 [C, 5]}`` -- support and the flips both, a_only, b_only, neither of every class, over the rows whose label lies
    in [0, C), "right" meaning rank 0 -- and with ``matrices`` the int64 [C, C] tables ``confusion_a``, ``confusion_b`` (label x prediction,
    the same rows) and ``moved`` (A's prediction x B's prediction, ALL rows).  Counted one row at a time."""
    C = int(C)
    out = dict(per_class=torch.zeros(C, 5, dtype=torch.int64))
    if matrices:
        out.update({k: torch.zeros(C, C, dtype=torch.int64) for k in MATRIX_KEYS})
    for i, y in enumerate(torch.as_tensor(labels).tolist()):
        ta, tb = int(top1_a[i]), int(top1_b[i])
        if matrices:
            out["moved"][ta, tb] += 1
        if 0 <= y < C:
            ok_a, ok_b = int(rank_a[i]) == 0, int(rank_b[i]) == 0
            out["per_class"][y, 0] += 1
            out["per_class"][y, 1 + (0 if ok_a and ok_b else 1 if ok_a else 2 if ok_b else 3)] += 1
            if matrices:
                out["confusion_a"][y, ta] += 1
                out["confusion_b"][y, tb] += 1
    return out


def reference_mcnemar(a_only, b_only):
    """The exact two-sided binomial (McNemar) test on the discordant pairs, in exact integers: ``min(1, 2 sum_{i <= min(a_only, b_only)}
    C(N, i) / 2^N)`` with ``N = a_only + b_only``; 1.0 without a discordant pair."""
    a_only, b_only = int(a_only), int(b_only)
    N = a_only + b_only
    if N == 0:
        return 1.0
    return float(min(Fraction(1), Fraction(2 * sum(math.comb(N, i) for i in range(min(a_only, b_only) + 1)), 2 ** N)))


def mcnemar(a_only, b_only):
    """``reference_mcnemar``'s value in float64 through ``lgamma``: every term ``exp(lgamma(N + 1) - lgamma(i + 1) - lgamma(N - i + 1) -
    N log 2)``, summed with ``fsum``."""
    a_only, b_only = int(a_only), int(b_only)
    N = a_only + b_only
    if N == 0:
        return 1.0
    base = math.lgamma(N + 1) - N * math.log(2.0)
    return min(1.0, 2.0 * math.fsum(math.exp(base - math.lgamma(i + 1) - math.lgamma(N - i + 1)) for i in range(min(a_only, b_only) + 1)))


def reference_cka_matrices(X, Y):
    X, Y = torch.as_tensor(X).double().cpu(), torch.as_tensor(Y).double().cpu()
    Xc, Yc = X - X.mean(dim=0, keepdim=True), Y - Y.mean(dim=0, keepdim=True)
    return Xc.T @ Yc, Xc.T @ Xc, Yc.T @ Yc


def reference_cka(X, Y, chunk_rows=None):
    """Linear CKA in float64: ``|Xc^T Yc|_F^2 / (|Xc^T Xc|_F |Yc^T Yc|_F)`` with the columns of both centred; None when the denominator is
    zero (constant features)."""
    kxy, kxx, kyy = reference_cka_matrices(X, Y)
    den = float(kxx.square().sum().sqrt()) * float(kyy.square().sum().sqrt())
    return float(kxy.square().sum()) / den if den > 0.0 else None


# ---- the banks ------------------------------------------------------------------------------------------------------------------------
def check_pair(bank_a, bank_b, topk, what_a="bank A", what_b="bank B"):
    """Refuses, by name and before anything is computed, two dicts that are not banks of one split in one order; returns ``data_classes``."""
    for bank, what in ((bank_a, what_a), (bank_b, what_b)):
        missing = [k for k in BANK_KEYS if not isinstance(bank, dict) or k not in bank]
        if missing:
            raise ValueError(f"{what} is not a logits bank: it lacks {', '.join(missing)} (compact_calibrate logits and compact_ood bank write them)")
        z, y = bank["logits"], bank["labels"]
        if not torch.is_tensor(z) or z.dim() != 2 or z.shape[1] != bank["num_classes"] or not torch.is_tensor(y) or tuple(y.shape) != (z.shape[0],):
            raise ValueError(f"{what}: the logits must be [n, num_classes = {bank['num_classes']}] with one label per row")
    na, nb = bank_a["logits"].shape[0], bank_b["logits"].shape[0]
    if na != nb:
        raise ValueError(f"the banks differ in rows: {what_a} has {na}, {what_b} has {nb}")
    if na < 1:
        raise ValueError("the banks hold no row")
    differ = torch.nonzero(bank_a["labels"].to(torch.int64) != bank_b["labels"].to(torch.int64))
    if differ.numel():
        raise ValueError(f"the banks' labels differ ({differ.shape[0]} rows, the first at row {int(differ[0, 0])}): not the same split in the same order")
    C = int(bank_a["data_classes"])
    if C != int(bank_b["data_classes"]):
        raise ValueError(f"the banks differ in data_classes: {what_a} has {C}, {what_b} has {int(bank_b['data_classes'])}")
    for bank, what in ((bank_a, what_a), (bank_b, what_b)):
        if not 1 <= C <= int(bank["num_classes"]):
            raise ValueError(f"data_classes {C} is not within {what}'s num_classes {int(bank['num_classes'])}")
    if not 1 <= int(topk) <= C:
        raise ValueError(f"--topk must lie in [1, data_classes = {C}], not {topk}")
    return C


def cka_plan(bank_a, bank_b, want):
    """None when linear CKA can be computed from the two banks, else the reason it cannot."""
    if not want:
        return "--cka 0"
    for bank, what in ((bank_a, "bank A"), (bank_b, "bank B")):
        f = bank.get("features")
        if not torch.is_tensor(f) or f.dim() != 2 or f.shape[0] != bank["logits"].shape[0]:
            return f"{what} holds no features (compact_ood bank stores them)"
    if bank_a.get("normalized") != bank_b.get("normalized"):
        return f"bank A's normalized is {bank_a.get('normalized')} and bank B's {bank_b.get('normalized')}"
    from .ops import OOD_MAX_D                         # the widest bank uvc_class_moments / uvc_center_rows take
    for bank, what in ((bank_a, "bank A"), (bank_b, "bank B")):
        D = bank["features"].shape[1]
        if D % 8 or not 8 <= D <= OOD_MAX_D:
            return f"{what}'s feature width {D} is not a multiple of 8 in [8, {OOD_MAX_D}]"
    return None


# ---- the comparison -------------------------------------------------------------------------------------------------------------------
def device_stats(dev=None):
    """``stats(za, zb, labels, C)`` on the device: ``ops.logits_pair_stats``."""
    from . import ops
    dev = TL.device(dev)

    def stats(za, zb, labels, C):
        with torch.cuda.device(dev):
            return ops.logits_pair_stats(za.to(dev), zb.to(dev), labels.to(dev).contiguous(), n_valid=C)
    return stats


def device_cka(dev=None):
    from . import ops
    dev = TL.device(dev)

    def cka_fn(X, Y, chunk_rows=None):
        with torch.cuda.device(dev):
            return ops.linear_cka(X.to(dev).float(), Y.to(dev).float(), chunk_rows)
    return cka_fn


def tables(st, labels, C, matrices=True):
    """``reference_tables``' dict as ``torch.bincount`` of int64 keys on the device the vectors are on."""
    ta, tb = st["top1_a"].to(torch.int64), st["top1_b"].to(torch.int64)
    y = labels.to(ta.device, torch.int64)
    counted = (y >= 0) & (y < C)
    ok_a, ok_b = st["rank_a"][counted] == 0, st["rank_b"][counted] == 0
    kind = torch.where(ok_a & ok_b, 1, torch.where(ok_a, 2, torch.where(ok_b, 3, 4)))
    yc = y[counted]
    per = torch.bincount(yc * 5 + kind, minlength=C * 5).reshape(C, 5)
    per[:, 0] = torch.bincount(yc, minlength=C)
    out = dict(per_class=per)
    if matrices:
        out.update(confusion_a=torch.bincount(yc * C + ta[counted], minlength=C * C).reshape(C, C),
                   confusion_b=torch.bincount(yc * C + tb[counted], minlength=C * C).reshape(C, C),
                   moved=torch.bincount(ta * C + tb, minlength=C * C).reshape(C, C))
    return {k: v.cpu() for k, v in out.items()}


def compare_banks(bank_a, bank_b, *, topk=5, worst_images=20, worst_classes=10, cka=1, chunk_rows=None, stats=None, cka_fn=None, dev=None):
    """``(record, output)``: the JSON record of the module docstring without ``img_per_s``, and the dict ``--output`` saves -- the ``STATS``
    vectors (float32 / int32 from the device, float64 / int64 from ``reference_pair_stats``), ``per_class`` int64 [C, 5] and, while ``C * C``
    is at most 2^26, ``confusion_a``, ``confusion_b`` and ``moved`` int64 [C, C].  ``stats`` / ``cka_fn``: None runs on the device."""
    C = check_pair(bank_a, bank_b, topk)
    k = int(topk)
    reason = cka_plan(bank_a, bank_b, cka)
    if stats is None:
        stats = device_stats(dev)
    if cka_fn is None and reason is None:
        cka_fn = device_cka(dev)
    labels = bank_a["labels"].to(torch.int64)
    st = stats(bank_a["logits"].float(), bank_b["logits"].float(), labels, C)
    st = {name: st[name] for name in STATS}
    bad = torch.nonzero(st["top1_a"] < 0)
    if bad.numel():
        raise ValueError(f"row {int(bad[0, 0])} of the banks holds a NaN logit in its first {C} columns ({bad.shape[0]} such rows)")
    matrices = C * C <= MAX_MATRIX
    tb = tables(st, labels, C, matrices)
    host = {name: v.cpu() for name, v in st.items()}
    f = {name: v.double() for name, v in host.items() if name not in INT_STATS}
    i = {name: v.to(torch.int64) for name, v in host.items() if name in INT_STATS}
    n = int(labels.shape[0])
    counted = (labels >= 0) & (labels < C)
    m = int(counted.sum())
    mean = lambda v: float(v.mean()) if v.numel() else None
    side = lambda s: dict(top1=mean((i["rank_" + s][counted] == 0).double()), topk=mean((i["rank_" + s][counted] < k).double()),
                          nll=mean(f["nll_" + s][counted]), confidence=mean(f["conf_" + s]))
    per = tb["per_class"]
    both, a_only, b_only, neither = (int(per[:, j].sum()) for j in (1, 2, 3, 4))
    agreement = mean((i["top1_a"] == i["top1_b"]).double())
    rec = dict(images=n, counted=m, data_classes=C, topk=k, a=side("a"), b=side("b"), agreement=agreement, churn=1.0 - agreement,
               flips=dict(both=both, a_only=a_only, b_only=b_only, neither=neither),
               negative_flip_rate=a_only / m if m else None, positive_flip_rate=b_only / m if m else None, mcnemar_p=mcnemar(a_only, b_only),
               kl_ab=mean(f["kl_ab"]), kl_ba=mean(f["kl_ba"]), js=mean(f["js"]), tv=mean(f["tv"]), js_max=float(f["js"].max()),
               a_top1_in_b_topk=mean((i["rank_b_top1a"] < k).double()), b_top1_in_a_topk=mean((i["rank_a_top1b"] < k).double()))
    # the classes whose recall fell most: delta ascending, ties by class index (a stable sort of the classes with a row)
    seen = torch.nonzero(per[:, 0] > 0)[:, 0]
    sup = per[seen, 0].double()
    rec_a, rec_b = (per[seen, 1] + per[seen, 2]).double() / sup, (per[seen, 1] + per[seen, 3]).double() / sup
    order = torch.sort(rec_b - rec_a, stable=True)[1][:max(int(worst_classes), 0)]
    rec["classes_worst"] = [dict({"class": int(seen[j])}, support=int(per[seen[j], 0]), recall_a=float(rec_a[j]), recall_b=float(rec_b[j]),
                                 delta=float(rec_b[j] - rec_a[j])) for j in order.tolist()]
    # the images whose prediction moved most: js descending, ties by row index
    order = torch.sort(f["js"], descending=True, stable=True)[1][:max(int(worst_images), 0)]
    rec["images_worst"] = [dict(index=j, label=int(labels[j]), top1_a=int(i["top1_a"][j]), top1_b=int(i["top1_b"][j]), js=float(f["js"][j]))
                           for j in order.tolist()]
    rec["matrices"] = bool(matrices)
    value = None
    if reason is None:
        try:
            value = cka_fn(bank_a["features"], bank_b["features"], chunk_rows)
        except L.UvcHipError as e:                                 # (uvc_gemm_tn refuses this (D1, D2) in float32)
            reason = str(e)
        else:
            reason = None if value is not None else "constant features"
    rec["cka"] = value
    if value is None:
        rec["cka_reason"] = reason
    return rec, dict(host, **tb)


def reference_compare(bank_a, bank_b, *, topk=5, worst_images=20, worst_classes=10, cka=1, chunk_rows=None):
    """The record, written out on its own in plain Python from ``reference_pair_stats``' vectors: one loop over the rows for the counts and
    the sums (``fsum``), ``reference_tables`` for the classes, ``reference_mcnemar`` for the test (the ``lgamma`` form beyond 4096 discordant
    pairs) and ``reference_cka``.  It shares ``check_pair`` and ``cka_plan`` -- the refusals and the conditions -- with ``compare_banks`` and
    nothing else."""
    C = check_pair(bank_a, bank_b, topk)
    k = int(topk)
    labels = [int(v) for v in bank_a["labels"].tolist()]
    st = {name: v.tolist() for name, v in reference_pair_stats(bank_a["logits"], bank_b["logits"], bank_a["labels"], C).items()}
    n = len(labels)
    if min(st["top1_a"]) < 0:
        raise ValueError(f"row {st['top1_a'].index(-1)} of the banks holds a NaN logit in its first {C} columns")
    rows = [j for j in range(n) if 0 <= labels[j] < C]                                 # the counted rows
    m = len(rows)
    over = lambda name, which: math.fsum(st[name][j] for j in which) / len(which) if which else None
    share = lambda test, which: sum(1 for j in which if test(j)) / len(which) if which else None
    everything = list(range(n))
    side = lambda s: dict(top1=share(lambda j: st["rank_" + s][j] == 0, rows), topk=share(lambda j: st["rank_" + s][j] < k, rows),
                          nll=over("nll_" + s, rows), confidence=over("conf_" + s, everything))
    flips = dict(both=0, a_only=0, b_only=0, neither=0)
    for j in rows:
        ok_a, ok_b = st["rank_a"][j] == 0, st["rank_b"][j] == 0
        flips["both" if ok_a and ok_b else "a_only" if ok_a else "b_only" if ok_b else "neither"] += 1
    agreement = share(lambda j: st["top1_a"][j] == st["top1_b"][j], everything)
    N = flips["a_only"] + flips["b_only"]
    rec = dict(images=n, counted=m, data_classes=C, topk=k, a=side("a"), b=side("b"), agreement=agreement, churn=1.0 - agreement, flips=flips,
               negative_flip_rate=flips["a_only"] / m if m else None, positive_flip_rate=flips["b_only"] / m if m else None,
               mcnemar_p=(reference_mcnemar if N <= 4096 else mcnemar)(flips["a_only"], flips["b_only"]),
               kl_ab=over("kl_ab", everything), kl_ba=over("kl_ba", everything), js=over("js", everything), tv=over("tv", everything),
               js_max=max(st["js"]), a_top1_in_b_topk=share(lambda j: st["rank_b_top1a"][j] < k, everything),
               b_top1_in_a_topk=share(lambda j: st["rank_a_top1b"][j] < k, everything))
    matrices = C * C <= MAX_MATRIX
    per = reference_tables(st["top1_a"], st["top1_b"], st["rank_a"], st["rank_b"], labels, C, matrices=False)["per_class"].tolist()
    classes = [dict({"class": c}, support=p[0], recall_a=(p[1] + p[2]) / p[0], recall_b=(p[1] + p[3]) / p[0]) for c, p in enumerate(per) if p[0] > 0]
    for c in classes:
        c["delta"] = c["recall_b"] - c["recall_a"]
    rec["classes_worst"] = sorted(classes, key=lambda c: (c["delta"], c["class"]))[:max(int(worst_classes), 0)]
    order = sorted(everything, key=lambda j: (-st["js"][j], j))[:max(int(worst_images), 0)]
    rec["images_worst"] = [dict(index=j, label=labels[j], top1_a=st["top1_a"][j], top1_b=st["top1_b"][j], js=st["js"][j]) for j in order]
    rec["matrices"] = matrices
    reason = cka_plan(bank_a, bank_b, cka)
    rec["cka"] = reference_cka(bank_a["features"], bank_b["features"]) if reason is None else None
    if rec["cka"] is None:
        rec["cka_reason"] = reason if reason is not None else "constant features"
    return rec


# ---- the commands -------------------------------------------------------------------------------------------------------------------------
def _load(b):
    return b if isinstance(b, dict) else torch.load(b, map_location="cpu")


def _compare_flags(args):
    return dict(topk=args.topk, worst_images=args.worst_images, worst_classes=args.worst_classes, cka=args.cka, chunk_rows=args.chunk_rows)


def _finish(rec, out, args, n, dt):
    if getattr(args, "output", None):
        torch.save(out, args.output)
    rec["img_per_s"] = n / dt if dt > 0 else 0.0
    return rec


def diff_command(args, dev=None, stats=None, cka_fn=None):
    """``diff``: the record.  ``stats`` / ``cka_fn``: None runs on the device; ``reference_pair_stats`` and ``reference_cka`` run the same
    command on the CPU."""
    bank_a, bank_b = _load(args.bank_a), _load(args.bank_b)
    t0 = time.perf_counter()
    rec, out = compare_banks(bank_a, bank_b, stats=stats, cka_fn=cka_fn, dev=dev, **_compare_flags(args))
    if stats is None:
        torch.cuda.synchronize()
    return _finish(rec, out, args, rec["images"], time.perf_counter() - t0)


def run_command(args, dev=None):
    """``run``: ``(record, bank_a, bank_b)``.  ONE eval loader, ONE walk over ``args.split``, one ``features(normalize=False)`` call per
    model and batch; the banks are ``compact_ood``'s (saved to ``args.bank_a`` / ``args.bank_b`` when given)."""
    from . import compact_ood as OD
    ex_a, ex_b = CP.as_export(args.a), CP.as_export(args.b)
    sa, sb = ex_a["cfg"]["img_size"], ex_b["cfg"]["img_size"]
    if sa != sb:
        raise ValueError(f"the files differ in img_size: --a has {sa}, --b has {sb} (one walk decodes every image once, at one size)")
    dev = TL.device(dev)
    model_a = CP.CompactVisionTransformer(ex_a, precision=args.precision, device=dev)
    model_b = CP.CompactVisionTransformer(ex_b, precision=args.precision, device=dev)
    loader, classes = TL.eval_loader(ex_a, args, args.split)
    with torch.cuda.device(dev):
        t0 = time.perf_counter()
        (za, fa, zb, fb), labels = TL.walk(loader, lambda x: model_a.features(x, normalize=False) + model_b.features(x, normalize=False))
        meta = dict(img_size=sa, dataset=args.dataset, split=args.split, interpolation=args.interpolation, crop_pct=args.crop_pct, precision=args.precision)
        bank_a, bank_b = OD.make_ood_bank(fa, za, labels, classes, **meta), OD.make_ood_bank(fb, zb, labels, classes, **meta)
        for bank, path in ((bank_a, args.bank_a), (bank_b, args.bank_b)):
            if path:
                torch.save(bank, path)
        rec, out = compare_banks(bank_a, bank_b, dev=dev, **_compare_flags(args))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return _finish(rec, out, args, rec["images"], dt), bank_a, bank_b


def _add_compare_flags(p):
    p.add_argument("--topk", type=CP._int_in(1, 65536, "--topk"), default=5, help="the k of the top-k accuracies and of a_top1_in_b_topk")
    p.add_argument("--worst_images", type=CP._int_in(0, 1 << 30, "--worst_images"), default=20, help="rows listed by js, descending")
    p.add_argument("--worst_classes", type=CP._int_in(0, 65536, "--worst_classes"), default=10, help="classes listed by recall_b - recall_a, ascending")
    p.add_argument("--cka", type=int, default=1, choices=[0, 1], help="1: linear CKA of the banks' features, where both hold them")
    p.add_argument("--chunk_rows", type=CP._int_in(1, 1 << 30, "--chunk_rows"), default=None, help="rows centred and multiplied at a time by the CKA (default 65536)")
    p.add_argument("--output", default=None, help="the per-image vectors and the integer tables")


def build_parser():
    p = argparse.ArgumentParser(prog="python -m uvc_amd.compact_compare", description="Compare two compact models on one split")
    sub = p.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("diff")
    d.add_argument("--bank_a", required=True, help="a bank of model A (compact_calibrate logits or compact_ood bank)")
    d.add_argument("--bank_b", required=True, help="a bank of model B on the same split in the same order")
    _add_compare_flags(d)
    r = sub.add_parser("run")
    r.add_argument("--a", required=True, help="compact file A (the reference: the dense export, the teacher)")
    r.add_argument("--b", required=True, help="compact file B")
    TL.add_dataset_flags(r, split_default="test")
    r.add_argument("--bank_a", default=None, help="where to save A's bank (as compact_ood bank writes it)")
    r.add_argument("--bank_b", default=None, help="where to save B's bank")
    _add_compare_flags(r)
    return p


def main(argv: Optional[Sequence[str]] = None):
    args = build_parser().parse_args(argv)
    if args.cmd == "diff":
        rec = diff_command(args)
    else:
        TL.need_data(args)
        rec = run_command(args)[0]
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main()
