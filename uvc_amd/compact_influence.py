"""Which training images stand behind a prediction of a compact model, and which training rows the model itself finds suspicious.

    python -m uvc_amd.compact_influence explain --train_bank T.pt --query_bank Q.pt [--rows 0 17 ...] [--k 5] [--target pred|label]
                                                [--precision bf16|fp32] --output infl.jsonl
    python -m uvc_amd.compact_influence explain --train_bank T.pt --compact F --images photos/ cat.jpg [--k 5] [--target_class 281]
                                                --output infl.jsonl
    python -m uvc_amd.compact_influence self    --bank T.pt [--top 100] [--per_class 1] --output suspects.jsonl

Banks are ``compact_ood bank``'s: raw readout features, eval logits and labels of one split in dataset order.  The head of a compact model
is ``z = W f + b`` under cross-entropy, so the gradient of example i with respect to ``(W, b)`` is the outer product ``r_i (x) [f_i; 1]`` with
``r_i = softmax(z_i) - e_target``, and the inner product of two examples' gradients -- the last-layer TracIn score of one checkpoint (Pruthi et
al. 2020), the representer-point form (Yeh et al. 2018) -- is

    I(i, t) = (f_i . f_t + 1) * (r_i . r_t)

A training row takes its label as the target (the gradient it was trained with), a query its predicted class (``--target pred``, the
explanation of the prediction), its label (``--target label``, the explanation of the loss) or one class for all (``--target_class``).  A
PROPONENT of a query has a large positive I (a step on that training row lowers the query's loss at the target), an OPPONENT a large negative
one; the SELF-INFLUENCE ``I(i, i) = (|f_i|^2 + 1) |r_i|^2`` is large for rows the model fits badly: mislabelled or atypical ones.  This is
last-layer influence at ONE checkpoint: not a Hessian-based influence function, nothing of the backbone's gradient, no sum over checkpoints.

``ops.influence_residuals``, ``ops.influence_topk`` and ``ops.self_influence`` (uvc_amd/csrc/influence.hip) do the arithmetic on the device,
without either [queries, rows] matrix; ``reference_residuals``, ``reference_influence`` and ``reference_self_influence`` are the written
specs in float64 PyTorch, and handed to the commands as ``lists`` / ``selfer`` they run them on banks without a device.
"""
from __future__ import annotations

import argparse
import json
import math
import time
from typing import Optional, Sequence

import torch

from . import compact as CP
from . import compact_ood as CO
from . import compact_tools as TL
from . import compact_transfer as CT

BIAS = 1.0                                          # the bias column of [f; 1]: every compact head has a bias
MAX_K = 64                                          # uvc_influence_topk's limits
MAX_D = 1024
MAX_CLASSES = 4096
TARGETS = ("pred", "label")
RECORD_KEYS = ("label", "pred", "target", "prob", "proponents", "opponents")
SELF_KEYS = ("row", "label", "pred", "prob_label", "value")


# ---- written specs ----------------------------------------------------------------------------------------------------------------
def reference_residuals(logits, labels, classes, target="label"):
    """``(r float64 [n, C], target int64 [n], rsq float64 [n])``: ``softmax(z) - e_target`` over the first C float32 logits in float64.  The
    target is the label (``target="label"``; a label outside [0, C) makes a SKIPPED row: zeros, target -1) or the row's first maximum
    (``"pred"``; ``labels`` may be None)."""
    C = int(classes)
    z = torch.as_tensor(logits).detach().cpu().float()[:, :C].double()
    n = z.shape[0]
    if target == "label":
        t = torch.as_tensor(labels).detach().cpu().to(torch.int64).clone()
        t[(t < 0) | (t >= C)] = -1
    elif target == "pred":
        t = z.argmax(dim=1)                                                     # torch's argmax: the first maximum
    else:
        raise ValueError(f"target must be one of {TARGETS}, not {target!r}")
    keep = t >= 0
    r = torch.zeros(n, C, dtype=torch.float64)
    p = torch.softmax(z[keep], dim=1)
    p[torch.arange(p.shape[0]), t[keep]] -= 1.0
    r[keep] = p
    return r, t, (r * r).sum(dim=1)


def _topk_rows(w, k):
    """(values [nq, k], rows int64 [nq, k]) of the k largest entries per row of float64 ``w``, descending, equal values by ascending
    column; -inf (and what was masked to it) never enters: those slots are (-inf, -1)."""
    nq, n = w.shape
    vals, idx = torch.sort(w, dim=1, descending=True, stable=True)
    vals, idx = vals[:, :k], idx[:, :k]
    idx = torch.where(vals == -math.inf, torch.full_like(idx, -1), idx)
    if n < k:
        vals = torch.cat([vals, torch.full((nq, k - n), -math.inf, dtype=torch.float64)], dim=1)
        idx = torch.cat([idx, torch.full((nq, k - n), -1, dtype=torch.int64)], dim=1)
    return vals, idx


def reference_values(fq, rq, fb, rb, bias=BIAS):
    """float64 [nq, n]: ``(fq . fb_i + bias) * (rq . rb_i)`` for every pair (operands read as float64)."""
    d = lambda t: torch.as_tensor(t).detach().cpu().double()
    return (d(fq) @ d(fb).T + float(bias)) * (d(rq) @ d(rb).T)


def reference_influence(fq, rq, fb, rb, k, bias=BIAS, exclude=None):
    """``((pos_vals, pos_idx), (neg_vals, neg_idx))``, float64 / int64 [nq, k]: per query the k largest ``reference_values`` (descending)
    and the k smallest (ascending), equal values by ascending bank row; a NaN enters neither list; ``exclude`` [nq]: one bank row per
    query that is skipped (-1: none).  A bank of fewer than k rows leaves (-inf, -1) / (+inf, -1)."""
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k must lie in [1, {MAX_K}], not {k}")
    v = reference_values(fq, rq, fb, rb, bias)
    out = torch.isnan(v)
    if exclude is not None:
        ex = torch.as_tensor(exclude).detach().cpu().to(torch.int64)
        hit = (ex >= 0) & (ex < v.shape[1])
        out[torch.arange(v.shape[0])[hit], ex[hit]] = True
    pos = _topk_rows(torch.where(out, torch.full_like(v, -math.inf), v), k)
    nv, ni = _topk_rows(torch.where(out, torch.full_like(v, -math.inf), -v), k)
    return pos, (-nv, ni)


def reference_self_influence(features, logits, labels, classes, bias=BIAS):
    """float64 [n]: ``(|f_i|^2 + bias) |r_i|^2`` with the label as the target -- the diagonal of ``reference_values`` of a bank against
    itself; 0 for a skipped row."""
    f = torch.as_tensor(features).detach().cpu().double()
    return ((f * f).sum(dim=1) + float(bias)) * reference_residuals(logits, labels, classes, "label")[2]


# ---- banks --------------------------------------------------------------------------------------------------------------------------
def check_bank(bank, what="the bank"):
    """``compact_ood.check_ood_bank``'s refusals (a normalized bank, a bank without logits), and the widths the kernels take."""
    CO.check_ood_bank(bank, what)
    D, C = int(bank["features"].shape[1]), int(bank["data_classes"])
    if D % 8 or not 8 <= D <= MAX_D:
        raise ValueError(f"{what}: embed_dim must be a multiple of 8 in [8, {MAX_D}], not {D}")
    if C > MAX_CLASSES:
        raise ValueError(f"{what}: data_classes {C} is more than the {MAX_CLASSES} the influence search takes")
    return bank


def check_pair(train_bank, query_bank):
    """Refuses, by name, two banks whose ``embed_dim``, ``data_classes`` or ``num_classes`` differ."""
    got = lambda b: dict(embed_dim=int(b["features"].shape[1]), data_classes=int(b["data_classes"]), num_classes=int(b["num_classes"]))
    a, b = got(train_bank), got(query_bank)
    for name in a:
        if a[name] != b[name]:
            raise ValueError(f"the query bank's {name} {b[name]} is not the train bank's {name} {a[name]}")


def _bank_arg(b, what):
    return check_bank(b, what) if isinstance(b, dict) else check_bank(torch.load(b, map_location="cpu"), f"{what} {b}")


# ---- the lists: on the device, and the spec ---------------------------------------------------------------------------------------------
def device_lists(fq, zq, yq, fb, zb, yb, classes, k, target="pred", exclude=None, precision="bf16", dev=None, splits=0):
    """``{"target" int64 [nq], "pos_vals", "pos_idx", "neg_vals", "neg_idx"}`` on the host from ``ops.influence_residuals`` (the bank by its
    labels, the queries by ``target``) and ``ops.influence_topk``; the features go in as ``precision``'s operand type, rounded once."""
    from . import ops
    dev = TL.device(dev)
    with torch.cuda.device(dev):
        f32 = lambda t: torch.as_tensor(t).to(dev, torch.float32).contiguous()
        lab = lambda y: None if y is None else torch.as_tensor(y).to(dev, torch.int64).contiguous()
        rb, _, _ = ops.influence_residuals(f32(zb), lab(yb), int(classes), "label")
        rq, tq, _ = ops.influence_residuals(f32(zq), lab(yq), int(classes), target)
        FQ, FB = CT.operand(f32(fq), precision).contiguous(), CT.operand(f32(fb), precision).contiguous()
        ex = None if exclude is None else torch.as_tensor(exclude).to(dev, torch.int32).contiguous()
        (pv, pi), (nv, ni) = ops.influence_topk(FQ, FB, rq, rb, int(k), bias=BIAS, exclude=ex, splits=splits)
        return dict(target=tq.cpu().to(torch.int64), pos_vals=pv.cpu(), pos_idx=pi.cpu().to(torch.int64), neg_vals=nv.cpu(), neg_idx=ni.cpu().to(torch.int64))


def reference_lists(fq, zq, yq, fb, zb, yb, classes, k, target="pred", exclude=None, precision="fp32", dev=None, splits=0):
    """``device_lists``' dict from the float64 specs; ``precision`` "bf16" rounds the features to bfloat16 once, as the device reads them."""
    rb = reference_residuals(zb, yb, classes, "label")[0]
    rq, tq, _ = reference_residuals(zq, yq, classes, target)
    low = (lambda t: torch.as_tensor(t).float().bfloat16()) if precision == "bf16" else (lambda t: torch.as_tensor(t).float())
    (pv, pi), (nv, ni) = reference_influence(low(fq), rq, low(fb), rb, k, BIAS, exclude)
    return dict(target=tq, pos_vals=pv, pos_idx=pi, neg_vals=nv, neg_idx=ni)


def device_self(features, logits, labels, classes, precision="fp32", dev=None):
    """float32 [n] on the host: ``reference_self_influence`` from ``ops.influence_residuals`` and ``ops.self_influence``."""
    from . import ops
    dev = TL.device(dev)
    with torch.cuda.device(dev):
        z = torch.as_tensor(logits).to(dev, torch.float32).contiguous()
        y = torch.as_tensor(labels).to(dev, torch.int64).contiguous()
        _, _, rsq = ops.influence_residuals(z, y, int(classes), "label")
        f = CT.operand(torch.as_tensor(features).to(dev, torch.float32), precision).contiguous()
        return ops.self_influence(f, rsq, bias=BIAS).cpu()


# ---- in Python ------------------------------------------------------------------------------------------------------------------------
def _check_k(k):
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"--k must lie in [1, {MAX_K}], not {k}")
    return k


def _query_stats(logits, classes, target):
    """(pred int64 [nq], prob float64 [nq]): the first maximum of the first C logits and the softmax probability of ``target`` (NaN for -1)."""
    z = torch.as_tensor(logits).float()[:, :classes].double()
    p = torch.softmax(z, dim=1)
    t = torch.as_tensor(target).to(torch.int64)
    prob = torch.where(t >= 0, p.gather(1, t.clamp_min(0)[:, None])[:, 0], torch.full((z.shape[0],), math.nan, dtype=torch.float64))
    return z.argmax(dim=1), prob


def influence(train_bank, query_bank, k=5, target="pred", rows=None, *, precision="bf16", exclude=None, lists=None, dev=None):
    """The proponents and opponents of query rows among the rows of a train bank: ``{"rows", "label", "pred", "target", "prob", "pos_vals",
    "pos_idx", "neg_vals", "neg_idx"}`` (CPU tensors, one entry per query).  ``rows``: the query bank's rows that are asked about (default:
    all); ``target`` "pred" or "label", or an int: one class for every query; ``exclude``: one train row per query that is skipped (a query
    that is itself a train row).  ``lists``: None runs ``device_lists``, ``reference_lists`` the float64 spec on the CPU."""
    check_bank(train_bank, "the train bank")
    check_bank(query_bank, "the query bank")
    check_pair(train_bank, query_bank)
    k, C = _check_k(k), int(train_bank["data_classes"])
    nq_all = query_bank["features"].shape[0]
    rows = torch.arange(nq_all) if rows is None else torch.as_tensor(list(rows), dtype=torch.int64)
    if rows.numel() == 0 or int(rows.min()) < 0 or int(rows.max()) >= nq_all:
        raise ValueError(f"--rows must name rows of the query bank, in [0, {nq_all})")
    fq, zq, yq = query_bank["features"][rows], query_bank["logits"][rows], query_bank["labels"][rows]
    return _influence(train_bank, fq, zq, yq, rows, k, C, target, precision, exclude, lists, dev)


def _influence(train_bank, fq, zq, yq, rows, k, C, target, precision, exclude, lists, dev):
    if isinstance(target, int) and not isinstance(target, bool):
        if not 0 <= target < C:
            raise ValueError(f"--target_class {target} must lie in [0, {C}) (data_classes)")
        ylab, mode = torch.full((fq.shape[0],), int(target), dtype=torch.int64), "label"
    elif target in TARGETS:
        ylab, mode = yq, target
        if mode == "label" and ylab is None:
            raise ValueError("--target label needs the queries' labels")
    else:
        raise ValueError(f"target must be one of {TARGETS} or a class, not {target!r}")
    res = (device_lists if lists is None else lists)(fq, zq, ylab, train_bank["features"], train_bank["logits"], train_bank["labels"], C, k, mode,
                                                     exclude=exclude, precision=precision, dev=dev)
    pred, prob = _query_stats(zq, C, res["target"])
    return dict(rows=rows, label=None if yq is None else torch.as_tensor(yq).to(torch.int64), pred=pred, prob=prob, **res)


def self_influence(bank, *, precision="fp32", selfer=None, dev=None):
    """float [n] on the host: every row's self-influence ``(|f|^2 + 1) |softmax(z) - e_label|^2`` (0 for a row whose label is no class).
    ``selfer``: None runs ``device_self``, ``reference_self_influence`` the float64 spec on the CPU."""
    check_bank(bank)
    C = int(bank["data_classes"])
    if selfer is None:
        return device_self(bank["features"], bank["logits"], bank["labels"], C, precision, dev)
    return selfer(bank["features"], bank["logits"], bank["labels"], C)


def rank_rows(values, labels, classes, top, per_class=False):
    """int64: the rows with the largest ``values``, descending, equal values by ascending row -- the ``top`` of the whole bank, or with
    ``per_class`` the ``top`` of every class, class ascending.  NaN values and rows whose label is no class are left out."""
    v = torch.as_tensor(values).double().clone()
    y = torch.as_tensor(labels).to(torch.int64)
    v[torch.isnan(v) | (y < 0) | (y >= classes)] = -math.inf
    order = torch.sort(v, descending=True, stable=True).indices
    order = order[v[order] > -math.inf]
    if not per_class:
        return order[:top]
    yo = y[order]
    return torch.cat([order[yo == c][:top] for c in range(classes)]) if classes else order[:0]


# ---- the commands -------------------------------------------------------------------------------------------------------------------
def _records(res, names, key, train_labels):
    """One record per query of ``influence``'s result; empty slots of a list are dropped."""
    tl = train_labels.tolist()
    entries = lambda vals, idx: [dict(row=int(i), label=int(tl[i]), value=float(v)) for v, i in zip(vals.tolist(), idx.tolist()) if i >= 0]
    for j, name in enumerate(names):
        yield {key: name, "label": None if res["label"] is None else int(res["label"][j]), "pred": int(res["pred"][j]),
               "target": int(res["target"][j]), "prob": float(res["prob"][j]),
               "proponents": entries(res["pos_vals"][j], res["pos_idx"][j]), "opponents": entries(res["neg_vals"][j], res["neg_idx"][j])}


def _shares(res, train_labels):
    """(the share of proponents whose label equals the query's target, the share of opponents whose label differs from it), over the
    filled slots of the queries that have a target; None without any."""
    t = res["target"][:, None]
    out = []
    for idx, same in ((res["pos_idx"], True), (res["neg_idx"], False)):
        ok = (idx >= 0) & (t >= 0)
        lab = train_labels[idx.clamp_min(0)]
        hit = ((lab == t) if same else (lab != t)) & ok
        out.append(float(hit.sum()) / int(ok.sum()) if int(ok.sum()) else None)
    return out


def _write(records, output):
    import sys
    out = open(output, "w", encoding="utf-8") if output else sys.stdout
    try:
        for rec in records:
            out.write(json.dumps(rec) + "\n")
    finally:
        if out is not sys.stdout:
            out.close()


def explain_command(args, lists=None, dev=None):
    """``explain``: one JSON line per query to ``args.output`` (or stdout) and the summary ``{"queries", "errors", "train_rows", "k",
    "target", "proponents_same_target", "opponents_other_label", "rows_per_s" | "img_per_s"}``."""
    train = _bank_arg(args.train_bank, "the train bank")
    k = _check_k(args.k)
    C = int(train["data_classes"])
    t0 = time.perf_counter()
    if getattr(args, "query_bank", None) is not None:
        if getattr(args, "images", None) or getattr(args, "compact", None):
            raise ValueError("--query_bank goes without --compact / --images")
        if getattr(args, "target_class", None) is not None:
            raise ValueError("--target_class goes with --images: a bank's queries take --target pred|label")
        query = _bank_arg(args.query_bank, "the query bank")
        res = influence(train, query, k, args.target, getattr(args, "rows", None), precision=args.precision, lists=lists, dev=dev)
        names, key, errors, rate = res["rows"].tolist(), "row", [], "rows_per_s"
    else:
        if not getattr(args, "images", None) or not getattr(args, "compact", None):
            raise ValueError("explain needs --query_bank, or --compact and --images")
        res, names, errors = _image_queries(train, args, k, C, lists, dev)
        key, rate = "file", "img_per_s"
    dt = time.perf_counter() - t0
    recs = list(_records(res, names, key, train["labels"])) if res is not None else []
    _write(recs + [dict(file=f, error=e) for f, e in errors], getattr(args, "output", None))
    same, other = _shares(res, train["labels"]) if res is not None else (None, None)
    n = len(recs)
    target = getattr(args, "target_class", None)
    return {"queries": n, "errors": len(errors), "train_rows": int(train["features"].shape[0]), "k": k,
            "target": args.target if target is None else int(target), "proponents_same_target": same, "opponents_other_label": other,
            rate: n / dt if dt > 0 else 0.0}


@torch.no_grad()
def _image_queries(train, args, k, C, lists, dev):
    """The queries of ``--images``: ONE ``features(normalize=False)`` call per batch of the preset's eval loader; ``(influence's result or
    None without a readable file, the files' names, [(file, error)])``."""
    from . import data
    export = CP.load_compact(args.compact) if not isinstance(args.compact, dict) else CP.check_export(args.compact)
    c = export["cfg"]
    if c["embed_dim"] != train["features"].shape[1] or c["num_classes"] != int(train["num_classes"]):
        raise ValueError(f"the train bank's embed_dim {train['features'].shape[1]} / num_classes {train['num_classes']} are not the model's "
                         f"{c['embed_dim']} / {c['num_classes']}")
    if getattr(args, "num_labels", None) is not None and int(args.num_labels) != C:
        raise ValueError(f"--num_labels {args.num_labels} is not the train bank's data_classes {C}")
    if args.preset not in CP.PRESETS:
        raise ValueError(f"preset must be one of {CP.PRESETS}, not {args.preset!r}")
    dev = TL.device(dev)
    model = CP.CompactVisionTransformer(export, precision=args.precision, device=dev)
    ds = data.FileListDataset(data.list_images(args.images), tolerant=True)
    kw = dict(mean=data.IMAGENET_MEAN, std=data.IMAGENET_STD, eval="center") if args.preset == "imagenet" else \
        dict(mean=data.CIFAR_MEAN, std=data.CIFAR_STD, eval="square")
    loader = data.DeviceLoader(ds, int(args.batch_size), c["img_size"], train=False, num_workers=args.num_workers, device=dev,
                               interpolation=args.interpolation, crop_pct=args.crop_pct, **kw)
    feats, logits = [], []
    with torch.cuda.device(dev):
        for x, _ in loader:
            z, f = model.features(x, normalize=False)
            feats.append(f.float())
            logits.append(z.float())
        f, z = torch.cat(feats).cpu(), torch.cat(logits).cpu()
    good = [i for i in range(len(ds)) if i not in ds.errors]
    errors = [(ds.paths[i], ds.errors[i]) for i in sorted(ds.errors)]
    if not good:
        return None, [], errors
    sel = torch.tensor(good, dtype=torch.int64)
    target = args.target if getattr(args, "target_class", None) is None else int(args.target_class)
    if target == "label":
        raise ValueError("--target label needs a query bank: image files carry no label")
    res = _influence(train, f[sel], z[sel], None, sel, k, C, target, args.precision, None, lists, dev)
    return res, [ds.paths[i] for i in good], errors


def self_command(args, selfer=None, dev=None):
    """``self``: the top rows by self-influence as ``{"row", "label", "pred", "prob_label", "value"}`` lines to ``args.output`` (or stdout)
    and the summary ``{"rows", "counted_rows", "written", "top", "per_class", "mean_value", "class_mean_value", "top_label_is_not_pred",
    "rows_per_s"}``."""
    bank = _bank_arg(args.bank, "the bank")
    C = int(bank["data_classes"])
    top = int(args.top)
    if top < 1:
        raise ValueError(f"--top must be positive, not {top}")
    t0 = time.perf_counter()
    v = torch.as_tensor(self_influence(bank, selfer=selfer, dev=dev)).double().cpu()
    dt = time.perf_counter() - t0
    y = bank["labels"].to(torch.int64)
    keep = (y >= 0) & (y < C) & ~torch.isnan(v)
    order = rank_rows(v, y, C, top, bool(args.per_class))
    pred, prob = _query_stats(bank["logits"][order], C, y[order])
    recs = [dict(row=int(i), label=int(y[i]), pred=int(p), prob_label=float(q), value=float(v[i])) for i, p, q in zip(order.tolist(), pred.tolist(), prob.tolist())]
    _write(recs, getattr(args, "output", None))
    cnt = torch.bincount(y[keep], minlength=C).double()
    tot = torch.bincount(y[keep], weights=v[keep], minlength=C)
    n = int(v.shape[0])
    return dict(rows=n, counted_rows=int(keep.sum()), written=len(recs), top=top, per_class=int(bool(args.per_class)),
                mean_value=float(v[keep].mean()) if int(keep.sum()) else None,
                class_mean_value=[float(t / c) if c else None for t, c in zip(tot.tolist(), cnt.tolist())],
                top_label_is_not_pred=float((pred != y[order]).sum()) / len(recs) if recs else None, rows_per_s=n / dt if dt > 0 else 0.0)


def build_parser():
    p = argparse.ArgumentParser(prog="python -m uvc_amd.compact_influence", description="Training-data influence for a compact model (last layer, one checkpoint)")
    sub = p.add_subparsers(dest="cmd", required=True)
    e = sub.add_parser("explain")
    e.add_argument("--train_bank", required=True, help="a raw bank of the train split (python -m uvc_amd.compact_ood bank --split train)")
    e.add_argument("--query_bank", default=None, help="a raw bank whose rows are explained; or --compact with --images")
    e.add_argument("--rows", type=int, nargs="+", default=None, help="the query bank's rows that are explained (default: all)")
    e.add_argument("--k", type=CP._int_in(1, MAX_K, "--k"), default=5, help="proponents and opponents per query")
    e.add_argument("--target", choices=list(TARGETS), default="pred", help="the class whose loss is explained: the predicted one, or the label")
    e.add_argument("--target_class", type=CP._int_in(0, MAX_CLASSES - 1, "--target_class"), default=None, help="--images: one class for every file")
    e.add_argument("--compact", default=None, help="the compact file the train bank was made with (--images)")
    CP.add_image_file_flags(e, topk=False, classes=False)
    for a in e._actions:                             # (--images is optional here: a query bank replaces it)
        if a.dest == "images":
            a.required = False
    s = sub.add_parser("self")
    s.add_argument("--bank", required=True, help="a raw bank (python -m uvc_amd.compact_ood bank)")
    s.add_argument("--top", type=CP._int_in(1, 1 << 30, "--top"), default=100, help="rows written")
    s.add_argument("--per_class", type=int, choices=[0, 1], default=0, help="1: the --top rows of every class, not of the whole bank")
    s.add_argument("--output", default=None, help="JSON-lines file; default: stdout")
    return p


def main(argv: Optional[Sequence[str]] = None, lists=None, selfer=None):
    args = build_parser().parse_args(argv)
    summary = explain_command(args, lists) if args.cmd == "explain" else self_command(args, selfer)
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
