"""Out-of-distribution detection for a compact model: does it know when an input is not from its label set at all?

    python -m uvc_amd.compact_ood bank  --compact F --dataset cifar10|cifar100|imagenet --data_dir D --split train|test --output B.pt
    python -m uvc_amd.compact_ood fit   --bank id_train.pt [--shrinkage 1e-6] [--knn_fraction 1.0] [--seed 0] [--chunk_rows N] --output det.pt
    python -m uvc_amd.compact_ood score --detector det.pt --id_bank id_test.pt --ood_bank ood.pt [--methods msp maxlogit energy entropy mahalanobis rmd knn]
                                        [--k 50] [--temperature 1.0] [--precision bf16|fp32] [--output scores.pt]

The OOD benchmark protocol (OpenOOD): score every image of an in-distribution (ID) split and of an OOD set with a handful of detectors and
report AUROC, AUPR and the false-positive rate at 95 % true-positive rate, ID being the positive class.  ``bank`` runs the EVAL transform over
one split in dataset order and saves the eval logits and the raw readout features of ONE ``features(normalize=False)`` call per batch; an
OOD set is just another ``--dataset / --data_dir`` (its labels are stored and never read by ``score``).  ``fit`` needs no model: from a raw
ID bank it fits the class-conditional Gaussian with a tied covariance on the device (``ops.class_gaussian_fit``: uvc_class_moments,
uvc_center_rows, uvc_gemm_tn), factors it on the host in float64 and keeps a seeded subset of the normalised rows for the k-NN detector.
``score`` needs no model either.  Every score is oriented HIGHER = MORE IN-DISTRIBUTION; with z the first ``data_classes`` logits and f the
raw feature:

    msp          max_c softmax(z)_c                                              (Hendrycks & Gimpel 2017)
    maxlogit     max_c z_c
    energy       T log sum_c exp(z_c / T)                                        (Liu et al. 2020)
    entropy      sum_c p_c log p_c, the negative entropy of softmax(z)
    mahalanobis  -min_c d2_c(f),  d2_c(f) = (f - mu_c)^T Sigma^-1 (f - mu_c)     (Lee et al. 2018)
    rmd          -(min_c d2_c(f) - d2_0(f)), d2_0 to the one Gaussian of all rows (Ren et al. 2021)
    knn          the cosine similarity of the k-th nearest row of the kept bank  (Sun et al. 2022: the negated distance, a monotone map of it)

The first four are one pass of uvc_ood_logit_scores; the Gaussian scores are uvc_gemm_nt, uvc_rows_sqnorm_aug and uvc_knn_topk with k = 1
(``ops.gauss_scores``); ``knn`` is uvc_knn_topk.  ``reference_fit``, ``reference_scores`` and ``reference_metrics`` are the written specs
(plain float64) the tests hold all of it to.
"""
from __future__ import annotations

import argparse
import json
import math
import time
from typing import Optional, Sequence

import torch

from . import compact as CP
from . import compact_tools as TL
from . import compact_transfer as CT

METHODS = ("msp", "maxlogit", "energy", "entropy", "mahalanobis", "rmd", "knn")
LOGIT_METHODS = METHODS[:4]
MAX_D = 1016                                        # uvc_knn_topk's widest row less the 8 augmentation columns (ops.gauss_scores)
DETECTOR_KEYS = ("version", "embed_dim", "data_classes", "num_classes", "meta", "counts", "means", "mean0", "scatter", "whiten", "whiten0",
                 "wmeans", "shrinkage", "knn_seed", "knn_fraction")


# ---- written specs ----------------------------------------------------------------------------------------------------------------
def _whitener(cov, what):
    """L^-1 of the Cholesky factor L L^T = cov (float64); a failure names --shrinkage."""
    L, info = torch.linalg.cholesky_ex(cov)
    if int(info) != 0 or not bool(torch.isfinite(L).all()):
        raise ValueError(f"the {what} covariance is not positive definite (Cholesky failed at pivot {int(info)}): raise --shrinkage")
    return torch.linalg.solve_triangular(L, torch.eye(cov.shape[0], dtype=cov.dtype), upper=False)


def gaussian_from_moments(counts, means, scatter, shrinkage):
    """The float64 host part of the fit, from the counts [C], class means [C, D] and the within-class scatter S [D, D] (any float type):
    ``mean0 = sum_c n_c mu_c / m``,  ``Sigma = S/m + lam (tr(S/m)/D) I``,  ``Sigma0 = S/m + (1/m) sum_c n_c (mu_c - mu_0)(mu_c - mu_0)^T +
    lam (tr(S/m)/D) I``,  ``whiten = L^-1`` with ``L L^T = Sigma`` (``whiten0`` likewise),  ``wmeans_c = whiten (mu_c - mu_0)``."""
    counts = counts.to(torch.int64).cpu()
    means, S = means.double().cpu(), scatter.double().cpu()
    m = int(counts.sum())
    if m < 1:
        raise ValueError("the bank has no row with a label in [0, data_classes)")
    D = means.shape[1]
    w = counts.double() / m
    mean0 = (w[:, None] * means).sum(dim=0)
    S = 0.5 * (S + S.T) / m
    ridge = float(shrinkage) * float(torch.trace(S)) / D * torch.eye(D, dtype=torch.float64)
    dm = (means - mean0) * (counts > 0)[:, None]
    cov = S + ridge
    cov0 = S + (w[:, None] * dm).T @ dm + ridge
    whiten, whiten0 = _whitener(cov, "tied within-class"), _whitener(cov0, "global")
    return dict(counts=counts, m=m, means=means, mean0=mean0, scatter=scatter.double().cpu(), cov=cov, cov0=cov0, whiten=whiten, whiten0=whiten0,
                wmeans=dm @ whiten.T)


def reference_fit(features, labels, data_classes, shrinkage=1e-6):
    """The class-conditional Gaussian of a bank in float64 (``gaussian_from_moments``' dict): the rows counted are those with a label in
    [0, C); ``mu_c`` is the mean of class c's rows (an empty class: zeros, count 0, never a candidate), ``S = sum_i (x_i - mu_{y_i})
    (x_i - mu_{y_i})^T``."""
    x, y = torch.as_tensor(features).double().cpu(), torch.as_tensor(labels).to(torch.int64).cpu()
    C = int(data_classes)
    keep = (y >= 0) & (y < C)
    x, y = x[keep], y[keep]
    counts = torch.bincount(y, minlength=C)
    means = torch.zeros(C, x.shape[1], dtype=torch.float64).index_add_(0, y, x) / counts.clamp_min(1)[:, None].double()
    c = x - means[y]
    return gaussian_from_moments(counts, means, c.T @ c, shrinkage)


def reference_gauss(detector, features):
    """``(d2 float64 [n, C], d2_0 float64 [n])`` from the detector's tensors as stored (float32 read as float64): the squared Mahalanobis
    distance of every row to every class (+inf for an empty class) and to the one Gaussian of all rows."""
    f = torch.as_tensor(features).double().cpu() - detector["mean0"].double()
    z = f @ detector["whiten"].double().T
    d2 = (z[:, None, :] - detector["wmeans"].double()[None]).square().sum(dim=2)
    d2[:, detector["counts"] == 0] = float("inf")
    return d2, (f @ detector["whiten0"].double().T).square().sum(dim=1)


def reference_scores(detector, bank, methods=METHODS, k=50, temperature=1.0, precision="fp32"):
    """``{method: float64 [n]}``: the scores of the module docstring in float64 on the float32 tensors of the detector and the bank.
    ``precision`` "bf16" rounds the normalised k-NN operands to bfloat16 once, as ``score_bank`` hands them to the search."""
    out = {}
    C, T = int(detector["data_classes"]), float(temperature)
    if set(methods) & set(LOGIT_METHODS):
        z = bank["logits"][:, :C].double()
        lse = torch.logsumexp(z, dim=1)
        p = torch.softmax(z, dim=1)
        out.update(msp=p.max(dim=1)[0], maxlogit=z.max(dim=1)[0], energy=T * torch.logsumexp(z / T, dim=1),
                   entropy=torch.where(p > 0, p * (z - lse[:, None]), torch.zeros_like(p)).sum(dim=1))
    if set(methods) & {"mahalanobis", "rmd"}:
        d2, d0 = reference_gauss(detector, bank["features"])
        out.update(mahalanobis=-d2.min(dim=1)[0], rmd=-(d2.min(dim=1)[0] - d0))
    if "knn" in methods:
        f = bank["features"].double()
        q = f / f.norm(dim=1, keepdim=True).clamp_min(1e-12)
        b = detector["knn_bank"]
        if precision == "bf16":
            q, b = q.float().bfloat16(), b.bfloat16()
        out["knn"] = torch.topk(q.double() @ b.double().T, int(k), dim=1)[0][:, int(k) - 1]
    return {name: out[name] for name in methods}


def reference_metrics(id_scores, ood_scores):
    """``{"auroc", "aupr", "fpr95", "id_mean", "ood_mean"}`` in float64 from two score vectors, ID the positive class:
    ``auroc = (#{s_i > s_o} + #{s_i = s_o} / 2) / (n_i n_o)`` over all (ID, OOD) pairs, by a sort and two binary searches;
    ``fpr95 = #{s_o >= tau} / n_o`` with tau the ceil(0.95 n_i)-th largest ID score;  ``aupr`` the average precision
    ``sum_t (R_t - R_{t-1}) P_t`` over the distinct scores in descending order."""
    import numpy as np
    f64 = lambda s: (s.detach().cpu().double().numpy() if torch.is_tensor(s) else np.asarray(s, dtype=np.float64)).ravel()
    si, so = f64(id_scores), f64(ood_scores)
    ni, no = len(si), len(so)
    if ni < 1 or no < 1:
        raise ValueError("metrics need at least one ID and one OOD score")
    if np.isnan(si).any() or np.isnan(so).any():
        raise ValueError("a NaN score in the " + ("ID" if np.isnan(si).any() else "OOD") + " bank")
    srt = np.sort(so)
    below, upto = np.searchsorted(srt, si, side="left"), np.searchsorted(srt, si, side="right")
    auroc = (float(below.sum()) + 0.5 * float((upto - below).sum())) / (float(ni) * float(no))
    tau = np.sort(si)[::-1][(95 * ni + 99) // 100 - 1]
    fpr95 = float(no - np.searchsorted(srt, tau, side="left")) / no
    both = np.concatenate([si, so])
    pos = np.concatenate([np.ones(ni), np.zeros(no)])
    order = np.argsort(-both, kind="stable")
    both, pos = both[order], pos[order]
    last = np.nonzero(np.append(both[1:] != both[:-1], True))[0]           # the last position of every distinct score
    tp = np.cumsum(pos)[last]
    prec, rec = tp / (last + 1.0), tp / ni
    aupr = float(np.sum(np.diff(np.concatenate([[0.0], rec])) * prec))
    return dict(auroc=auroc, aupr=aupr, fpr95=fpr95, id_mean=float(si.mean()), ood_mean=float(so.mean()))


def metrics(id_scores, ood_scores, method=None):
    """``reference_metrics`` on the float32 score vectors; a NaN score is an error naming the method and the bank."""
    try:
        return reference_metrics(id_scores, ood_scores)
    except ValueError as e:
        raise ValueError(f"{method}: {e}") if method else e


# ---- the bank and detector files ------------------------------------------------------------------------------------------------------
def make_ood_bank(features, logits, labels, data_classes, **meta):
    """``compact_transfer.make_bank``'s dict plus the eval logits float32 [n, num_classes], ``num_classes`` and ``normalized: False``."""
    return TL.make_bank(labels, data_classes, features=features, logits=logits, normalized=False, **meta)


def check_ood_bank(bank, what="the bank"):
    """Refuses, by name, a bank that is not raw (``normalized`` true or missing: ``compact_transfer embed`` writes those) or has no logits."""
    if not isinstance(bank, dict) or not {"features", "labels", "data_classes", "meta"} <= set(bank):
        raise ValueError(f"{what} is not a feature bank (python -m uvc_amd.compact_ood bank writes one)")
    if bank.get("normalized", True) is not False:
        raise ValueError(f"{what} is normalized (or does not say): the detectors need raw features (python -m uvc_amd.compact_ood bank)")
    if not torch.is_tensor(bank.get("logits")) or bank["logits"].dim() != 2 or bank["logits"].shape[0] != bank["features"].shape[0]:
        raise ValueError(f"{what} has no logits (python -m uvc_amd.compact_ood bank stores them)")
    if bank["logits"].shape[1] != bank.get("num_classes") or not 1 <= bank["data_classes"] <= bank["logits"].shape[1]:
        raise ValueError(f"{what}: num_classes {bank.get('num_classes')} / data_classes {bank['data_classes']} do not fit its logits")
    return bank


def load_ood_bank(path, what="the bank"):
    return check_ood_bank(torch.load(path, map_location="cpu"), f"{what} {path}")


def check_detector(det, what="the detector"):
    if not isinstance(det, dict) or not set(DETECTOR_KEYS) <= set(det) or det["version"] != 1:
        raise ValueError(f"{what} is not a version-1 detector file (python -m uvc_amd.compact_ood fit writes one)")
    return det


def check_against(det, bank, what, data_classes=False):
    """Refuses, by name, a bank whose ``embed_dim`` or ``num_classes`` (an ID bank: also ``data_classes``) is not the detector's."""
    names = ("embed_dim", "num_classes") + (("data_classes",) if data_classes else ())
    got = dict(embed_dim=int(bank["features"].shape[1]), num_classes=int(bank["num_classes"]), data_classes=int(bank["data_classes"]))
    for name in names:
        if got[name] != det[name]:
            raise ValueError(f"{what}'s {name} {got[name]} is not the detector's {name} {det[name]}")


def check_request(det, methods, k, temperature):
    """Refuses, by name and before anything is computed, a method whose ingredient is missing and a setting outside its range."""
    for name in methods:
        if name not in METHODS:
            raise ValueError(f"method {name!r} is not one of {METHODS}")
    if not float(temperature) > 0 or math.isinf(float(temperature)):
        raise ValueError(f"--temperature must be positive, not {temperature}")
    if "knn" in methods:
        if det.get("knn_bank") is None:
            raise ValueError("knn needs a knn_bank: the detector was fitted with --knn_fraction 0")
        if not 1 <= int(k) <= CT.MAX_K:
            raise ValueError(f"--k must lie in [1, {CT.MAX_K}], not {k}")
        if int(k) > det["knn_bank"].shape[0]:
            raise ValueError(f"--k {k} is more than the knn_bank's {det['knn_bank'].shape[0]} rows")


# ---- fit and score ----------------------------------------------------------------------------------------------------------------------
def knn_rows(n, fraction, seed):
    """int64, ascending: the first ceil(fraction n) entries of a seeded CPU permutation of the rows."""
    if not 0.0 <= float(fraction) <= 1.0:
        raise ValueError(f"--knn_fraction must lie in [0, 1], not {fraction}")
    m = min(n, int(math.ceil(float(fraction) * n)))
    return torch.sort(torch.randperm(n, generator=torch.Generator().manual_seed(int(seed)))[:m])[0]


def fit_detector(bank, shrinkage=1e-6, knn_fraction=1.0, seed=0, chunk_rows=None, dev=None):
    """The detector dict of a raw ID bank: counts, class means and the within-class scatter from the device (``ops.class_gaussian_fit``), the
    float64 host factorisation of ``gaussian_from_moments`` rounded once to float32, and the normalised k-NN rows."""
    from . import ops
    check_ood_bank(bank)
    n, D = bank["features"].shape
    C = int(bank["data_classes"])
    if D % 8 or not 8 <= D <= MAX_D:
        raise ValueError(f"embed_dim must be a multiple of 8 in [8, {MAX_D}], not {D}")
    rows = knn_rows(n, knn_fraction, seed)
    dev = TL.device(dev)
    with torch.cuda.device(dev):
        counts, means, scatter = ops.class_gaussian_fit(bank["features"].to(dev), bank["labels"].to(dev), C, chunk_rows=chunk_rows)
        counts, means, scatter = counts.cpu(), means.cpu(), scatter.cpu()
    g = gaussian_from_moments(counts, means, scatter, shrinkage)
    det = dict(version=1, embed_dim=int(D), data_classes=C, num_classes=int(bank["num_classes"]), meta=dict(bank["meta"]), counts=counts, means=means,
               mean0=g["mean0"].float(), scatter=scatter, whiten=g["whiten"].float().contiguous(), whiten0=g["whiten0"].float().contiguous(),
               wmeans=g["wmeans"].float().contiguous(), shrinkage=float(shrinkage), knn_seed=int(seed), knn_fraction=float(knn_fraction))
    if len(rows):
        det["knn_bank"] = torch.nn.functional.normalize(bank["features"][rows].float(), dim=1, eps=1e-12).contiguous()
    return det


@torch.no_grad()
def score_bank(detector, bank, methods=METHODS, k=50, temperature=1.0, precision="bf16", dev=None):
    """``{method: float32 [n]}`` on the host: the scores of every row of a raw bank, higher = more in-distribution.  ``precision`` only
    selects the operand type of the k-NN search."""
    from . import ops
    check_request(detector, methods, k, temperature)
    dev = TL.device(dev)
    out = {}
    C = int(detector["data_classes"])
    with torch.cuda.device(dev):
        if set(methods) & set(LOGIT_METHODS):
            want = [name in methods for name in LOGIT_METHODS]
            n = bank["logits"].shape[0]
            outs = [torch.empty(n, dtype=torch.float32, device=dev) if w else None for w in want]
            ops.ood_logit_scores(bank["logits"].to(dev), n_valid=C, temperature=temperature, outs=outs)
            out.update({name: o for name, o in zip(LOGIT_METHODS, outs) if o is not None})
        if set(methods) & {"mahalanobis", "rmd", "knn"}:
            f = bank["features"].to(dev).float().contiguous()
        if set(methods) & {"mahalanobis", "rmd"}:
            mean0 = detector["mean0"].to(dev)
            d2, _ = ops.gauss_scores(f, detector["whiten"].to(dev), mean0, detector["wmeans"].to(dev), detector["counts"].to(dev))
            if "mahalanobis" in methods:
                out["mahalanobis"] = -d2
            if "rmd" in methods:
                out["rmd"] = -(d2 - ops.gauss_scores(f, detector["whiten0"].to(dev), mean0))
        if "knn" in methods:
            q = CT.operand(f / f.norm(dim=1, keepdim=True).clamp_min(1e-12), precision).contiguous()
            out["knn"] = ops.knn_topk(q, CT.operand(detector["knn_bank"].to(dev), precision).contiguous(), int(k))[0][:, int(k) - 1]
        out = {name: out[name].float().cpu() for name in methods}
    return out


def evaluate(detector, id_bank, ood_bank, methods=METHODS, k=50, temperature=1.0, precision="bf16", dev=None):
    """``(the summary line of score, {method: {"id": float32 [n_i], "ood": float32 [n_o]}})``."""
    check_detector(detector)
    check_ood_bank(id_bank, "the ID bank")
    check_ood_bank(ood_bank, "the OOD bank")
    check_against(detector, id_bank, "the ID bank", data_classes=True)
    check_against(detector, ood_bank, "the OOD bank")
    check_request(detector, methods, k, temperature)
    dev = TL.device(dev)
    t0 = time.perf_counter()
    si = score_bank(detector, id_bank, methods, k, temperature, precision, dev)
    so = score_bank(detector, ood_bank, methods, k, temperature, precision, dev)
    dt = time.perf_counter() - t0
    line = dict(id_images=int(id_bank["features"].shape[0]), ood_images=int(ood_bank["features"].shape[0]), methods={}, k=int(k),
                temperature=float(temperature))
    for name in methods:
        for which, s in (("ID", si[name]), ("OOD", so[name])):
            if bool(torch.isnan(s).any()):
                raise ValueError(f"{name}: a NaN score in the {which} bank")
        line["methods"][name] = metrics(si[name], so[name], name)
    n = line["id_images"] + line["ood_images"]
    line["img_per_s"] = n / dt if dt > 0 else 0.0
    return line, {name: dict(id=si[name], ood=so[name]) for name in methods}


# ---- the commands -------------------------------------------------------------------------------------------------------------------------
def bank_command(export_or_path, args, dev=None):
    """``bank``: the bank dict of ``args.split`` -- the eval logits and raw features of ONE ``features(normalize=False)`` call per batch --
    (saved to ``args.output`` when given) and ``compact_transfer embed``'s summary plus ``"normalized": False, "logits": True``."""
    return TL.bank_command(export_or_path, args, dev, lambda model, x: model.features(x, normalize=False)[::-1], make_ood_bank,
                           lambda bank: dict(embed_dim=int(bank["features"].shape[1]), normalized=False, logits=True))


def fit_command(args, dev=None):
    bank = load_ood_bank(args.bank) if not isinstance(args.bank, dict) else check_ood_bank(args.bank)
    t0 = time.perf_counter()
    det = fit_detector(bank, shrinkage=args.shrinkage, knn_fraction=args.knn_fraction, seed=args.seed, chunk_rows=args.chunk_rows, dev=dev)
    dt = time.perf_counter() - t0
    if getattr(args, "output", None):
        torch.save(det, args.output)
    knn = det.get("knn_bank")
    return det, dict(output=getattr(args, "output", None), rows=int(bank["features"].shape[0]), counted_rows=int(det["counts"].sum()),
                     data_classes=det["data_classes"], embed_dim=det["embed_dim"], empty_classes=int((det["counts"] == 0).sum()),
                     shrinkage=det["shrinkage"], knn_rows=0 if knn is None else int(knn.shape[0]), seconds=dt)


def score_command(args, dev=None):
    det = check_detector(torch.load(args.detector, map_location="cpu") if not isinstance(args.detector, dict) else args.detector)
    id_bank = load_ood_bank(args.id_bank, "the ID bank") if not isinstance(args.id_bank, dict) else args.id_bank
    ood_bank = load_ood_bank(args.ood_bank, "the OOD bank") if not isinstance(args.ood_bank, dict) else args.ood_bank
    line, scores = evaluate(det, id_bank, ood_bank, methods=tuple(args.methods), k=args.k, temperature=args.temperature, precision=args.precision, dev=dev)
    if getattr(args, "output", None):
        torch.save(scores, args.output)
    return line


def build_parser():
    p = argparse.ArgumentParser(prog="python -m uvc_amd.compact_ood", description="Out-of-distribution detection for a compact model")
    sub = p.add_subparsers(dest="cmd", required=True)
    b = sub.add_parser("bank")
    b.add_argument("--compact", required=True, help="the compact file")
    TL.add_dataset_flags(b)
    b.add_argument("--output", required=True, help="the bank file: raw features, eval logits, labels, data_classes, num_classes, meta")
    f = sub.add_parser("fit")
    f.add_argument("--bank", required=True, help="a raw bank of the ID train split (bank --split train)")
    f.add_argument("--shrinkage", type=float, default=1e-6, help="lam: the covariances get lam * (trace / D) on their diagonal")
    f.add_argument("--knn_fraction", type=float, default=1.0, help="the share of the bank's rows kept for knn (0: none)")
    f.add_argument("--seed", type=int, default=0, help="of the permutation that picks the knn rows")
    f.add_argument("--chunk_rows", type=CP._int_in(1, 1 << 30, "--chunk_rows"), default=None, help="rows centred and multiplied at a time (default 65536)")
    f.add_argument("--output", required=True, help="the detector file")
    s = sub.add_parser("score")
    s.add_argument("--detector", required=True)
    s.add_argument("--id_bank", required=True, help="a raw bank of the ID test split")
    s.add_argument("--ood_bank", required=True, help="a raw bank of the OOD set")
    s.add_argument("--methods", nargs="+", choices=list(METHODS), default=list(METHODS))
    s.add_argument("--k", type=int, default=50, help="knn: the neighbour whose similarity is the score")
    s.add_argument("--temperature", type=float, default=1.0, help="energy: T log sum exp(z / T)")
    s.add_argument("--precision", choices=["bf16", "fp32"], default="bf16", help="the operand type of the knn search")
    s.add_argument("--output", default=None, help="the raw float32 score vectors per method")
    return p


def main(argv: Optional[Sequence[str]] = None):
    args = build_parser().parse_args(argv)
    if args.cmd == "bank":
        TL.need_data(args)
        summary = bank_command(args.compact, args)[1]
    elif args.cmd == "fit":
        summary = fit_command(args)[1]
    else:
        summary = score_command(args)
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
