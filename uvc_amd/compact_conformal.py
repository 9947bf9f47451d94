"""Prediction sets with a coverage guarantee for a compact model: split conformal prediction on a logits bank.

    python -m uvc_amd.compact_conformal fit   --bank cal_logits.pt --alpha 0.1 [--method lac|aps|raps] [--randomized 1] [--seed 0]
                                              [--lam 0.01] [--k_reg 5] [--temperature 1.0] --output conformal.json
    python -m uvc_amd.compact_conformal score --bank test_logits.pt --calibration conformal.json [--sets_output sets.jsonl] [--classes FILE]

Given a held-out calibration split and a level ``alpha``, every input gets a set of labels that holds the true one with probability at least
``1 - alpha`` (Vovk et al.; LAC: Sadinle et al. 2019, APS: Romano et al. 2020, RAPS: Angelopoulos et al. 2021).  No retraining, no assumption
about the model; the size of the sets is the price, and so a measure of what pruning cost below the first place.  Banks are
``compact_calibrate logits`` banks (a calibrated file goes through ``logits`` as it is: the temperature is folded into its head).

The rule.  ``p = softmax(z / T)`` over the valid columns ``[0, C)``.  The classes of a row are ordered by descending float32 logit, ties by
ascending index (-0 = +0); ``r_c`` in 1 .. C is the rank of class c and ``M_c`` the sum of ``p_j`` over the classes ranked ahead of it.  With
one ``u`` in [0, 1] per row (None: 1, the deterministic variant): ``lac`` s(c) = 1 - p_c; ``aps`` s(c) = M_c + u p_c; ``raps`` s(c) = M_c +
u p_c + lam max(0, r_c - k_reg).  Over the m rows whose label lies in [0, C), ``qhat`` is the k-th smallest s(y_i) with
``k = ceil((m + 1)(1 - alpha))`` in exact rational arithmetic on alpha's decimal string; k > m gives qhat = +inf.  The set of a row is
``{c : s(c) <= qhat}``; empty sets (LAC makes them) are reported, not repaired.  ``u`` comes from a CPU ``torch.Generator`` -- ``seed`` for
``fit``, ``seed + 1`` for ``score`` -- so the device and the CPU see the same values.

``ops.conformal_scores`` and ``ops.conformal_sets`` (uvc_conformal_scores / uvc_conformal_sets) do the arithmetic on the device, writing
nothing of the size of the logits; ``reference_scores`` and ``reference_sets`` are the written spec in float64 PyTorch, and handed to the
commands as ``scorer`` / ``setter`` they run them on a bank without a device.
"""
from __future__ import annotations

import argparse
import json
import math
from fractions import Fraction
from typing import Optional, Sequence

import torch

from . import compact as CP
from . import compact_calibrate as CC
from . import compact_tools as TL

METHODS = ("lac", "aps", "raps")
FILE_KEYS = ("version", "method", "alpha", "qhat", "k", "rows", "randomized", "seed", "lam", "k_reg", "temperature", "data_classes",
             "num_classes", "meta")
STRATA = ((0, 1), (2, 3), (4, 6), (7, 10), (11, 100), (101, None))      # Angelopoulos et al. 2021, size-stratified coverage
SIZE_QUANTILES = (0.5, 0.9, 0.99)
DEFAULT_LAM, DEFAULT_K_REG = 0.01, 5


# ---- the rule -----------------------------------------------------------------------------------------------------------------------
def quantile_index(m, alpha) -> int:
    """``k = ceil((m + 1)(1 - alpha))`` in exact rational arithmetic on ``alpha``'s decimal string (``str(alpha)`` of a float): alpha = 0.1
    and m = 999 give 900.  ``0 < alpha < 1`` and ``m >= 1``, anything else is refused."""
    try:
        a = Fraction(str(alpha).strip())
    except (ValueError, ZeroDivisionError):
        raise ValueError(f"alpha {alpha!r} is not a decimal number") from None
    if not 0 < a < 1:
        raise ValueError(f"alpha {alpha} must lie in (0, 1)")
    m = int(m)
    if m < 1:
        raise ValueError(f"the calibration split holds {m} rows whose label is a class: at least 1 is needed")
    return math.ceil((m + 1) * (1 - a))


def _checked(method, temperature, lam, k_reg):
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, not {method!r}")
    if not (float(temperature) > 0 and math.isfinite(float(temperature))):
        raise ValueError(f"temperature {temperature} must be positive and finite")
    if not (float(lam) >= 0 and math.isfinite(float(lam))):
        raise ValueError(f"lam {lam} must be non-negative and finite")
    if int(k_reg) < 0:
        raise ValueError(f"k_reg {k_reg} must be non-negative")


def _row_u(u, n):
    if u is None:
        return torch.ones(n, 1, dtype=torch.float64)
    u = torch.as_tensor(u).detach().cpu().double().reshape(-1)
    if u.numel() != n:
        raise ValueError(f"u must hold one value per row ({n}), not {u.numel()}")
    return u[:, None]


def reference_class_scores(logits, classes, method="aps", u=None, temperature=1.0, lam=0.0, k_reg=0):
    """float64 ``s [n, C]``: the score of every class of every row, by the rule of the module's docstring."""
    _checked(method, temperature, lam, k_reg)
    C = int(classes)
    z = torch.as_tensor(logits).detach().cpu().float()[:, :C]
    n = z.shape[0]
    p = torch.softmax(z.double() / float(temperature), dim=1)
    if method == "lac":
        return 1.0 - p
    order = torch.sort(z, dim=1, descending=True, stable=True).indices          # equal logits (-0 = +0) keep their ascending index
    ps = p.gather(1, order)
    s = (ps.cumsum(1) - ps) + _row_u(u, n) * ps
    if method == "raps":
        s = s + float(lam) * (torch.arange(1, C + 1, dtype=torch.float64) - int(k_reg)).clamp_min(0)[None, :]
    return torch.empty_like(s).scatter_(1, order, s)


def reference_scores(logits, labels, classes, method="aps", u=None, temperature=1.0, lam=0.0, k_reg=0):
    """``(scores float64 [n], m)``: the score of every row's label, NaN for a row whose label lies outside [0, C); m counts the others."""
    C = int(classes)
    s = reference_class_scores(logits, C, method, u, temperature, lam, k_reg)
    y = torch.as_tensor(labels).detach().cpu().to(torch.int64)
    keep = (y >= 0) & (y < C)
    out = torch.full((s.shape[0],), float("nan"), dtype=torch.float64)
    out[keep] = s[keep].gather(1, y[keep][:, None])[:, 0]
    return out, int(keep.sum())


def pack_members(inset):
    """bool [n, C] -> int32 [n, ceil(C / 32)]: bit c % 32 of word c / 32 (the bits of the kernel's uint32 words), padding bits zero."""
    n, C = inset.shape
    W = (C + 31) // 32
    b = torch.zeros(n, W * 32, dtype=torch.int64)
    b[:, :C] = inset.to(torch.int64)
    w = (b.reshape(n, W, 32) << torch.arange(32, dtype=torch.int64)).sum(2)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def unpack_members(members, classes):
    """int32 / uint32 [n, W] -> bool [n, C]."""
    w = torch.as_tensor(members).detach().cpu().to(torch.int64) & 0xFFFFFFFF
    bits = (w[:, :, None] >> torch.arange(32, dtype=torch.int64)) & 1
    return bits.reshape(w.shape[0], -1)[:, :int(classes)].bool()


def reference_sets(logits, qhat, labels=None, classes=None, method="aps", u=None, temperature=1.0, lam=0.0, k_reg=0, members=False):
    """``(size int32 [n], covered uint8 [n] or None without labels, members int32 [n, ceil(C / 32)] or None)``: the sets
    ``{c : s(c) <= qhat}``; ``covered`` is 0 for a row whose label lies outside [0, C)."""
    C = int(torch.as_tensor(logits).shape[1] if classes is None else classes)
    qhat = float(qhat)
    if math.isnan(qhat):
        raise ValueError("qhat is NaN")
    s = reference_class_scores(logits, C, method, u, temperature, lam, k_reg)
    inset = torch.ones_like(s, dtype=torch.bool) if qhat == math.inf else s <= qhat
    covered = None
    if labels is not None:
        y = torch.as_tensor(labels).detach().cpu().to(torch.int64)
        keep = (y >= 0) & (y < C)
        covered = torch.zeros(s.shape[0], dtype=torch.uint8)
        covered[keep] = inset[keep].gather(1, y[keep][:, None])[:, 0].to(torch.uint8)
    return inset.sum(1).to(torch.int32), covered, (pack_members(inset) if members else None)


# ---- on the device ------------------------------------------------------------------------------------------------------------------
def _on_device(logits, labels, u, device):
    dev = TL.device(device)
    Z = torch.as_tensor(logits).to(dev, torch.float32).contiguous()
    y = None if labels is None else torch.as_tensor(labels).to(dev).contiguous()
    if y is not None and y.dtype not in (torch.int32, torch.int64):
        y = y.to(torch.int64)
    uu = None if u is None else torch.as_tensor(u).to(dev, torch.float32).reshape(-1).contiguous()
    return dev, Z, y, uu


def conformal_scores(logits, labels, classes, method="aps", u=None, temperature=1.0, lam=0.0, k_reg=0, device=None):
    """``(scores float32 [n] on the device, m)``: ``reference_scores``' result from ``ops.conformal_scores`` (``logits``, ``labels`` and
    ``u`` from anywhere)."""
    from . import ops
    _checked(method, temperature, lam, k_reg)
    dev, Z, y, uu = _on_device(logits, labels, u, device)
    with torch.cuda.device(dev):
        s, counts = ops.conformal_scores(Z, y, int(classes), method, uu, temperature=temperature, lam=lam, k_reg=k_reg)
        return s, int(counts[0])


def conformal_sets(logits, qhat, labels=None, classes=None, method="aps", u=None, temperature=1.0, lam=0.0, k_reg=0, members=False, device=None):
    """``reference_sets``' result from ``ops.conformal_sets``, tensors on the device (``members``: the words' bits as int32)."""
    from . import ops
    _checked(method, temperature, lam, k_reg)
    dev, Z, y, uu = _on_device(logits, labels, u, device)
    with torch.cuda.device(dev):
        return ops.conformal_sets(Z, qhat, y, None if classes is None else int(classes), method, uu, temperature=temperature, lam=lam, k_reg=k_reg,
                                  members=bool(members))


# ---- fitting and scoring ------------------------------------------------------------------------------------------------------------
def draw_u(n, seed):
    """``n`` float32 values in [0, 1) of a CPU ``torch.Generator`` seeded with ``seed``."""
    return torch.rand(int(n), generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float32)


def fit_conformal(logits, labels, classes, alpha, method="aps", *, randomized=True, seed=0, lam=DEFAULT_LAM, k_reg=DEFAULT_K_REG, temperature=1.0,
                  scorer=None):
    """The calibration of one split: ``{"method", "alpha", "qhat", "k", "rows", "randomized", "seed", "lam", "k_reg", "temperature"}``.
    ``scorer``: None runs ``conformal_scores`` on the device, ``reference_scores`` the same on the CPU.  ``lac`` draws no u."""
    _checked(method, temperature, lam, k_reg)
    classes = int(classes)
    y = torch.as_tensor(labels).detach().cpu().to(torch.int64)
    m = int(((y >= 0) & (y < classes)).sum())
    k = quantile_index(m, alpha)
    randomized = bool(randomized) and method != "lac"
    u = draw_u(y.shape[0], seed) if randomized else None
    s, counted = (conformal_scores if scorer is None else scorer)(logits, labels, classes, method, u, temperature, lam, k_reg)
    if int(counted) != m:
        raise RuntimeError(f"the scorer counted {int(counted)} rows, the labels say {m}")
    if k > m:
        qhat = math.inf
    else:
        keep = ((y >= 0) & (y < classes)).to(s.device)
        qhat = float(torch.sort(s[keep]).values[k - 1])               # m floats: not hot
        if math.isnan(qhat):
            raise ValueError("a score of the calibration split is NaN (NaN logits?)")
    return dict(method=method, alpha=float(alpha), qhat=qhat, k=k, rows=m, randomized=randomized, seed=int(seed), lam=float(lam), k_reg=int(k_reg),
                temperature=float(temperature))


def check_calibration(cal):
    if not isinstance(cal, dict) or not set(FILE_KEYS) <= set(cal) or cal["version"] != 1:
        raise ValueError(f"not a version-1 conformal calibration: need the keys {', '.join(FILE_KEYS)}")
    _checked(cal["method"], cal["temperature"], cal["lam"], cal["k_reg"])
    if math.isnan(float(cal["qhat"])):
        raise ValueError("the calibration's qhat is NaN")
    return cal


def load_calibration(path_or_dict):
    if isinstance(path_or_dict, dict):
        return check_calibration(path_or_dict)
    with open(path_or_dict, "r", encoding="utf-8") as f:
        try:
            return check_calibration(json.load(f))
        except ValueError as e:
            raise ValueError(f"{path_or_dict}: {e}") from None


def prediction_sets(logits, calibration, labels=None, u=None, members=False, setter=None):
    """``(size, covered or None, members or None)`` of ``logits`` under a calibration (``fit_conformal``'s dict with ``data_classes``).
    ``u``: one value per row for a randomized calibration (None there: the deterministic, larger sets)."""
    c = calibration
    return (conformal_sets if setter is None else setter)(logits, c["qhat"], labels, int(c["data_classes"]), c["method"], u, c["temperature"], c["lam"],
                                                          c["k_reg"], members)


def summarize(size, covered, labels, top1_hits, classes):
    """The record of ``score`` from the sets' sizes and coverage flags (CPU tensors): coverage and ``top1`` (percent) over the m rows whose
    label lies in [0, classes), sizes over all rows."""
    size = torch.as_tensor(size).detach().cpu().to(torch.int64)
    cov = torch.as_tensor(covered).detach().cpu().to(torch.int64)
    y = torch.as_tensor(labels).detach().cpu().to(torch.int64)
    keep = (y >= 0) & (y < classes)
    n, m = int(size.shape[0]), int(keep.sum())
    ssort = torch.sort(size).values
    q = lambda f: int(ssort[min(n - 1, max(0, math.ceil(f * n) - 1))])
    per_n = torch.bincount(y[keep], minlength=classes).double()
    per_c = torch.bincount(y[keep], weights=cov[keep].double(), minlength=classes)
    seen = per_n > 0
    cc = per_c[seen] / per_n[seen]
    strata = []
    for lo, hi in STRATA:
        inside = keep & (size >= lo) & (size <= (hi if hi is not None else 2 ** 62))
        rows = int(inside.sum())
        strata.append(dict(lo=lo, hi=hi, rows=rows, coverage=(float(cov[inside].sum()) / rows if rows else None)))
    return dict(images=n, rows=m, coverage=float(cov[keep].sum()) / m if m else 0.0, mean_size=float(size.double().mean()), median_size=q(0.5),
                size_quantiles={**{str(f): q(f) for f in SIZE_QUANTILES}, "max": int(ssort[-1])}, empty=int((size == 0).sum()),
                singleton_share=float((size == 1).sum()) / n, top1=100.0 * int(top1_hits) / m if m else 0.0,
                class_coverage_min=float(cc.min()) if m else 0.0, class_coverage_mean=float(cc.mean()) if m else 0.0, size_stratified=strata)


def evaluate(bank, calibration, setter=None):
    """The record of a logits bank under a calibration: ``score``'s JSON members.  u is drawn with ``seed + 1`` for a randomized
    calibration.  ``setter``: None builds the sets on the device (``conformal_sets``), ``reference_sets`` on the CPU."""
    return evaluate_sets(bank, calibration, setter)[0]


def evaluate_sets(bank, calibration, setter=None, members=False):
    """``(evaluate's record, (size, covered, members))``."""
    bank, cal = CC.check_logits_bank(bank), check_calibration(calibration)
    for key in ("data_classes", "num_classes"):
        if int(bank[key]) != int(cal[key]):
            raise ValueError(f"the bank's {key} {bank[key]} is not the calibration's {key} {cal[key]}")
    C = int(bank["data_classes"])
    z, y = bank["logits"], bank["labels"]
    u = draw_u(z.shape[0], cal["seed"] + 1) if cal["randomized"] else None
    size, covered, mem = prediction_sets(z, cal, y, u, members, setter)
    keep = (y >= 0) & (y < C)
    hits = int((z[:, :C].argmax(dim=1)[keep] == y[keep]).sum())            # the bank is on the CPU: [n] integers, torch's first maximum
    rec = summarize(size, covered, y, hits, C)
    return dict(method=cal["method"], alpha=cal["alpha"], qhat=cal["qhat"], data_classes=C, num_classes=int(bank["num_classes"]), **rec), (size, covered, mem)


# ---- the commands -------------------------------------------------------------------------------------------------------------------
def _bank_arg(b):
    return CC.load_logits_bank(b) if not isinstance(b, dict) else CC.check_logits_bank(b)


def fit_command(args, scorer=None):
    """``fit``: the calibration file's dict (written to ``args.output`` when given)."""
    bank = _bank_arg(args.bank)
    res = fit_conformal(bank["logits"], bank["labels"], bank["data_classes"], args.alpha, args.method, randomized=args.randomized, seed=args.seed,
                        lam=args.lam, k_reg=args.k_reg, temperature=args.temperature, scorer=scorer)
    cal = dict(version=1, **res, data_classes=int(bank["data_classes"]), num_classes=int(bank["num_classes"]), meta=dict(bank["meta"]))
    cal = {k: cal[k] for k in FILE_KEYS}
    if args.output:
        with open(args.output, "w", encoding="utf-8") as f:
            json.dump(cal, f)
    return cal


def score_command(args, setter=None):
    """``score``: the record; with ``args.sets_output`` one JSON line per row, the set decoded from ``members``."""
    bank, cal = _bank_arg(args.bank), load_calibration(args.calibration)
    names = CP.read_classes(args.classes) if getattr(args, "classes", None) else None
    C = int(bank["data_classes"])
    if names is not None and len(names) < C:
        raise ValueError(f"--classes holds {len(names)} names, the bank has {C} classes")
    want = bool(getattr(args, "sets_output", None))
    rec, (size, covered, mem) = evaluate_sets(bank, cal, setter, members=want)
    if want:
        inset = unpack_members(mem, C)
        size, covered = torch.as_tensor(size).cpu(), torch.as_tensor(covered).cpu()
        with open(args.sets_output, "w", encoding="utf-8") as f:
            for i in range(inset.shape[0]):
                idx = inset[i].nonzero()[:, 0].tolist()
                f.write(json.dumps(dict(row=i, label=int(bank["labels"][i]), size=int(size[i]), covered=bool(covered[i]),
                                        set=[names[c] for c in idx] if names is not None else idx)) + "\n")
    return rec


def _alpha_arg(v):
    try:
        quantile_index(1, v)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None
    return v.strip()


def _positive(v):
    f = float(v)
    if not (f > 0 and math.isfinite(f)):
        raise argparse.ArgumentTypeError(f"must be positive and finite, not {v}")
    return f


def _non_negative(v):
    f = float(v)
    if not (f >= 0 and math.isfinite(f)):
        raise argparse.ArgumentTypeError(f"must be non-negative and finite, not {v}")
    return f


def build_parser():
    p = argparse.ArgumentParser(prog="python -m uvc_amd.compact_conformal", description="Prediction sets with a coverage guarantee for a compact model")
    sub = p.add_subparsers(dest="cmd", required=True)
    f, s = sub.add_parser("fit"), sub.add_parser("score")
    f.add_argument("--bank", required=True, help="the logits bank of the calibration split (compact_calibrate logits)")
    f.add_argument("--alpha", required=True, type=_alpha_arg, help="the error rate, a decimal in (0, 1): sets hold the label with probability >= 1 - alpha")
    f.add_argument("--method", choices=list(METHODS), default="aps")
    f.add_argument("--randomized", type=int, choices=[0, 1], default=1, help="aps, raps: 1 draws one u per row (exact coverage), 0 takes u = 1")
    f.add_argument("--seed", type=int, default=0, help="of u: fit draws with seed, score with seed + 1")
    f.add_argument("--lam", type=_non_negative, default=DEFAULT_LAM, help="raps: the penalty per rank beyond --k_reg")
    f.add_argument("--k_reg", type=CP._int_in(0, 1 << 20, "--k_reg"), default=DEFAULT_K_REG, help="raps: the ranks that go unpenalised")
    f.add_argument("--temperature", type=_positive, default=1.0)
    f.add_argument("--output", required=True, help="the calibration file (JSON)")
    s.add_argument("--bank", required=True, help="the logits bank to build sets for")
    s.add_argument("--calibration", required=True, help="fit's file")
    s.add_argument("--sets_output", default=None, help="JSON-lines file: row, label, size, covered and the set of every row")
    s.add_argument("--classes", default=None, help="class names for --sets_output: one per line, or a JSON list")
    return p


def main(argv: Optional[Sequence[str]] = None):
    args = build_parser().parse_args(argv)
    summary = fit_command(args) if args.cmd == "fit" else score_command(args)
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
