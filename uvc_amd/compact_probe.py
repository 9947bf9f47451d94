"""Linear probe for a compact model: a new head fitted on its frozen features.

    python -m uvc_amd.compact_probe embed --compact F --dataset cifar10|cifar100|imagenet --data_dir D --split train|test --output raw.pt
    python -m uvc_amd.compact_probe fit   --compact F --bank raw_train.pt [--val_bank raw_test.pt | --val_fraction 0.1 --seed 0]
                                          [--l2 X ... | --l2_grid N --l2_min 1e-6 --l2_max 1e-1] [--bias 1] [--max_iter 1000] [--refit 1]
                                          [--precision bf16|fp32] [--chunk_rows N] --output G
    python -m uvc_amd.compact_probe score --compact G --bank raw_test.pt

The middle step between ``compact_transfer knn`` (no training) and ``compact finetune`` (a backward pass over the images): an
L2-regularised multinomial logistic regression on the features, solved by L-BFGS with the regulariser swept on a validation split (CLIP's
linear-probe protocol; DINO reports the number beside k-NN).  The features are embedded once; every pass after that runs over ``[n, D]``
features.  ``embed`` writes ``compact_transfer``'s bank with the UN-normalised readout features (what a compact file's head reads) and a
top-level ``"normalized": False``; ``fit`` sweeps ``l2`` from the largest value down, every fit warm-started from the one before, and
writes a version-1 compact file whose head is the fitted classifier; ``score`` runs a file's own head over a bank.

The objective and its gradient over the whole bank are ``uvc_probe_eval`` (``ops.probe_eval``): two GEMMs around one softmax / cross-entropy
row kernel per chunk of rows.  ``reference_objective`` is the written spec (plain PyTorch float64) the tests hold it to.
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

PAD_BIAS = -1e4                                     # the bias of a head's padding rows: `compact eval` takes its argmax over all num_classes logits
SCORE_ROWS = 65536                                  # rows per logits GEMM when a head is scored


# ---- written spec -----------------------------------------------------------------------------------------------------------------
def reference_objective(W, b, X, y, l2):
    """``(F, dW, db, hits)`` in float64: ``F = (1/m) sum_i (lse(z_i) - z_{i, y_i}) + (l2 / 2) |W|^2`` with ``z = X W^T + b`` over the m rows
    whose label lies in ``[0, C)`` (any other label counts for nothing; m = 0 leaves the l2 terms), the bias not regularised;
    ``dW = (1/m) G^T X + l2 W`` and ``db = (1/m) colsum G`` (None without b) with ``G = softmax(z) - onehot(y)``, zero on uncounted rows;
    ``hits`` the counted rows whose label is the FIRST maximum of the row."""
    W, X = torch.as_tensor(W).detach().double(), torch.as_tensor(X).detach().double()
    y = torch.as_tensor(y).detach().to(torch.int64)
    C = W.shape[0]
    z = X @ W.T
    if b is not None:
        z = z + torch.as_tensor(b).detach().double()
    keep = (y >= 0) & (y < C)
    m = int(keep.sum())
    reg = 0.5 * float(l2) * float((W * W).sum())
    if m == 0:
        return reg, float(l2) * W, (None if b is None else torch.zeros(C, dtype=torch.float64)), 0
    yk = y[keep]
    zk = z[keep]
    lse = torch.logsumexp(zk, dim=1)
    F = float((lse - zk.gather(1, yk[:, None])[:, 0]).sum()) / m + reg
    G = torch.zeros_like(z)
    Gk = torch.softmax(zk, dim=1)
    Gk[torch.arange(m), yk] -= 1.0
    G[keep] = Gk
    hits = int((zk.argmax(dim=1) == yk).sum())                       # torch's argmax: the first maximum
    return F, G.T @ X / m + float(l2) * W, (None if b is None else G.sum(0) / m), hits


# ---- the evaluator on the device ------------------------------------------------------------------------------------------------------
class DeviceEvaluator:
    """``evaluator(W, b, X, y, l2)`` of ``fit_probe`` on the device: ``ops.probe_eval`` on float32 masters padded to ``Cp`` rows.
    ``prepare`` moves a bank's features to the device in the precision's operand type once."""

    def __init__(self, classes, precision="bf16", chunk_rows=None, device=None):
        self.device = TL.device(device)
        self.classes, self.precision, self.chunk_rows = int(classes), precision, chunk_rows
        self.rows = -(-self.classes // CT.HEAD_MULTIPLE) * CT.HEAD_MULTIPLE
        self.dtype = torch.float32
        self._ws = None
        self.counts = None

    def prepare(self, features, labels):
        X = CT.operand(features.to(self.device), self.precision).contiguous()
        return X, labels.to(self.device).contiguous()

    def __call__(self, W, b, X, y, l2):
        from . import ops
        n, D = X.shape
        dtype = ops.UVC_F32 if X.dtype == torch.float32 else ops.UVC_BF16
        chunk = ops.probe_chunk_rows(n, self.classes, dtype) if self.chunk_rows is None else int(self.chunk_rows)
        need = ops.probe_workspace_bytes(n, D, self.classes, dtype, chunk)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=X.device)
        dW, db, F, self.counts = ops.probe_eval(X, y, W, b, self.classes, l2, chunk_rows=chunk, workspace=self._ws)
        return F, dW, db, self.counts[0]


# ---- fitting ----------------------------------------------------------------------------------------------------------------------
def fit_probe(features, labels, classes, l2, *, bias=True, max_iter=1000, history=10, tol_grad=1e-6, tol_change=None, precision="bf16", init=None,
              evaluator=None, chunk_rows=None):
    """L-BFGS (``torch.optim.LBFGS``, strong Wolfe line search) on ``reference_objective``'s problem.  ``evaluator(W, b, X, y, l2)`` returns
    ``(F, dW, db, hits)``; None builds the device one (``DeviceEvaluator``), the CPU tests inject ``reference_objective``.  An evaluator may
    carry ``prepare(features, labels)``, ``rows`` (the parameter rows, classes rounded up), ``dtype`` and ``device`` of the parameters
    (default: classes, float64, cpu).  ``init``: ``(W, b)`` to start from (rows ``[0, classes)`` are read), default zeros.
    Returns ``{"W" [classes, D], "b" [classes] or None, "F", "top1", "grad_inf", "iterations", "evaluations", "rows"}`` (tensors on the CPU
    in the parameters' dtype; top1 in percent of the counted rows)."""
    classes = int(classes)
    if classes < 1:
        raise ValueError(f"classes {classes} must be at least 1")
    if evaluator is None:
        evaluator = DeviceEvaluator(classes, precision, chunk_rows)
    rows, dtype, dev = getattr(evaluator, "rows", classes), getattr(evaluator, "dtype", torch.float64), getattr(evaluator, "device", "cpu")
    X, y = evaluator.prepare(features, labels) if hasattr(evaluator, "prepare") else (features, labels)
    D = X.shape[1]
    W = torch.zeros(rows, D, dtype=dtype, device=dev)
    b = torch.zeros(rows, dtype=dtype, device=dev) if bias else None
    if init is not None:
        W[:classes] = init[0][:classes].to(W)
        if bias and init[1] is not None:
            b[:classes] = init[1][:classes].to(b)
    params = [W.requires_grad_()] + ([b.requires_grad_()] if bias else [])

    def evaluate():
        F, dW, db, hits = evaluator(W.detach(), None if b is None else b.detach(), X, y, l2)
        W.grad = dW.to(W).reshape(W.shape)
        if bias:
            b.grad = db.to(b)
        return F, hits

    F, last, g, iterations, evaluations = TL.lbfgs(params, evaluate, max_iter=max_iter, history=history, tol_grad=tol_grad, tol_change=tol_change,
                                                   dtype=dtype)
    m = int(((y >= 0) & (y < classes)).sum())
    return dict(W=W.detach()[:classes].cpu().clone(), b=None if b is None else b.detach()[:classes].cpu().clone(), F=F,
                top1=100.0 * int(last["hits"]) / m if m else 0.0, grad_inf=g, iterations=iterations, evaluations=evaluations, rows=m)


def l2_grid(count, lo=1e-6, hi=1e-1):
    """``count`` values from ``hi`` down to ``lo``, evenly spaced in the logarithm."""
    count = int(count)
    if count < 1 or not 0 < lo <= hi:
        raise ValueError("--l2_grid needs at least one value and 0 < --l2_min <= --l2_max")
    if count == 1:
        return [float(hi)]
    return [float(math.exp(math.log(hi) + (math.log(lo) - math.log(hi)) * i / (count - 1))) for i in range(count)]


def score_head(W, b, X, y, classes):
    """Top-1 in percent of the head ``(W, b)`` on device features ``X`` (the operand type) over the rows whose label lies in
    ``[0, classes)``: ``ops.gemm_nt`` into float32 logits and ``ops.logits_topk`` at k = 1 over the first ``classes`` columns."""
    from . import ops
    dev = X.device
    rows = -(-int(classes) // CT.HEAD_MULTIPLE) * CT.HEAD_MULTIPLE
    D = X.shape[1]
    Wp = torch.zeros(rows, D, dtype=torch.float32, device=dev)
    Wp[:classes] = W[:classes].to(dev, torch.float32)
    bp = torch.zeros(rows, dtype=torch.float32, device=dev)
    if b is not None:
        bp[:classes] = b[:classes].to(dev, torch.float32)
    Wop = CT.operand(Wp, "bf16" if X.dtype == torch.bfloat16 else "fp32").contiguous()
    dtype = ops.UVC_F32 if X.dtype == torch.float32 else ops.UVC_BF16
    y = y.to(dev, torch.int64)
    hits = torch.zeros((), dtype=torch.int64, device=dev)
    logits = torch.empty(min(SCORE_ROWS, X.shape[0]), rows, dtype=torch.float32, device=dev)
    for r0 in range(0, X.shape[0], SCORE_ROWS):
        xc = X[r0:r0 + SCORE_ROWS]
        out = logits[:xc.shape[0]]
        ops.gemm_nt(xc, Wop, out, dtype=dtype, epilogue=ops.EPI_BIAS, bias=bp)
        pred = ops.logits_topk(out, 1, n_valid=int(classes))[1][:, 0].to(torch.int64)
        hits += (pred == y[r0:r0 + SCORE_ROWS]).sum()
    m = int(((y >= 0) & (y < classes)).sum())
    return 100.0 * int(hits) / m if m else 0.0


def sweep(train, val, l2_values, classes, *, scorer=None, **fit_args):
    """``(records, best)``: one ``fit_probe`` per value of ``l2_values``, from the largest down, every fit warm-started from the one before
    (never one stacked optimisation); each scored on ``val = (features, labels)`` by ``scorer(W, b, features, labels, classes)`` (None: the
    device's ``score_head`` on the evaluator's operands).  ``records[i] = {"l2", "F", "train_top1", "val_top1", "iterations",
    "evaluations"}``; ``best`` is the fit (``fit_probe``'s dict plus "l2" and "val_top1") with the best validation top-1, the larger
    ``l2`` on a tie."""
    values = sorted((float(v) for v in l2_values), reverse=True)
    if not values:
        raise ValueError("sweep needs at least one l2 value")
    evaluator = fit_args.get("evaluator")
    if evaluator is None:
        evaluator = fit_args["evaluator"] = DeviceEvaluator(classes, fit_args.get("precision", "bf16"), fit_args.get("chunk_rows"))
    if scorer is None:
        vx, vy = evaluator.prepare(*val)
        scorer = lambda W, b, f, l, c: score_head(W, b, vx, vy, c)
    records, best, init = [], None, fit_args.pop("init", None)
    for l2 in values:
        fit = fit_probe(train[0], train[1], classes, l2, init=init, **fit_args)
        init = (fit["W"], fit["b"])
        top1 = float(scorer(fit["W"], fit["b"], val[0], val[1], classes))
        records.append(dict(l2=l2, F=fit["F"], train_top1=fit["top1"], val_top1=top1, iterations=fit["iterations"], evaluations=fit["evaluations"]))
        if best is None or top1 > best["val_top1"]:                  # strictly better only: the larger l2 keeps a tie
            best = dict(fit, l2=l2, val_top1=top1)
    return records, best


# ---- banks ------------------------------------------------------------------------------------------------------------------------
def bank_is_normalized(bank) -> bool:
    """A bank without the ``"normalized"`` key is ``compact_transfer embed``'s: normalised."""
    return bool(bank.get("normalized", True))


def check_probe_bank(bank, export, bias, data_classes=None):
    """``compact_transfer.check_bank``'s refusals (``embed_dim``, ``data_classes``, by name), and a normalised bank only without a bias:
    a compact file's head reads the un-normalised features, and only a head without bias keeps its argmax under a positive row scale."""
    CT.check_bank(bank, export, data_classes)
    if bank_is_normalized(bank) and bias:
        raise ValueError("the bank holds normalized features (python -m uvc_amd.compact_probe embed writes raw ones): a head with a bias "
                         "fitted on them is not the classifier the file would run; refit with --bias 0")
    return bank


def make_raw_bank(features, labels, data_classes, **meta):
    """``compact_transfer.make_bank``'s dict of the UN-normalised features plus ``"normalized": False``."""
    return TL.make_bank(labels, data_classes, features=features, normalized=False, **meta)


def embed(export_or_path, args, dev=None):
    """``embed``: ``make_raw_bank``'s dict of ``args.split`` (saved to ``args.output`` when given), and the summary."""
    return TL.bank_command(export_or_path, args, dev, lambda model, x: (model.features(x, normalize=False)[1],), make_raw_bank,
                           lambda bank: dict(embed_dim=int(bank["features"].shape[1]), normalized=False))


# ---- the file ---------------------------------------------------------------------------------------------------------------------
def probe_head(export, W, b, classes):
    """A version-1 compact file whose head is the classifier ``(W [classes, D], b [classes] or None)``: ``compact_transfer.rehead(init="zero")``
    builds it (the width rule, one weight for ``head`` and ``head_dist``, every other tensor bit for bit), rows ``[0, classes)`` of weight
    and bias are then written; the padding rows keep zero weights and get the bias ``PAD_BIAS``, so no padding logit wins an argmax over
    all ``num_classes`` logits."""
    classes = int(classes)
    D = export["cfg"]["embed_dim"]
    W = torch.as_tensor(W)
    if tuple(W.shape) != (classes, D) or (b is not None and tuple(torch.as_tensor(b).shape) != (classes,)):
        raise ValueError(f"probe_head: W [{classes}, {D}] and b [{classes}] or None")
    stub = dict(features=torch.empty(0, D), labels=torch.empty(0, dtype=torch.int64), data_classes=classes, meta=dict(embed_dim=D))
    out, _ = CT.rehead(export, stub, init="zero")
    sd = out["state_dict"]
    for name in ("head", "head_dist"):
        if name + ".weight" in sd:
            w, bb = sd[name + ".weight"], sd[name + ".bias"]
            w[:classes] = W.to(w.dtype)
            bb[:classes] = 0 if b is None else torch.as_tensor(b).to(bb.dtype)
            bb[classes:] = PAD_BIAS
    return CP.check_export(out)


def file_head(export, classes):
    """``(W [classes, D], b [classes])`` of a file whose ``head`` and ``head_dist`` are one classifier (a ``probe_head`` / ``rehead`` file)."""
    sd = export["state_dict"]
    W, b = sd["head.weight"], sd["head.bias"]
    if "head_dist.weight" in sd and not (torch.equal(sd["head_dist.weight"], W) and torch.equal(sd["head_dist.bias"], b)):
        raise ValueError("score needs a file whose head and head_dist are one classifier (compact_probe fit and compact_transfer rehead write such files)")
    if not 1 <= classes <= W.shape[0]:
        raise ValueError(f"the bank's data_classes {classes} is not within the file's num_classes {W.shape[0]}")
    return W[:classes].float(), b[:classes].float()


# ---- the commands -----------------------------------------------------------------------------------------------------------------
split_bank = TL.split_bank


def fit_command(args, dev=None):
    export = CP.as_export(args.compact)
    bank = CT.load_bank(args.bank) if not isinstance(args.bank, dict) else args.bank
    bias = bool(args.bias)
    check_probe_bank(bank, export, bias)
    classes = int(bank["data_classes"])
    train, val = (bank["features"], bank["labels"]), None
    if args.val_bank is not None:
        vb = CT.load_bank(args.val_bank) if not isinstance(args.val_bank, dict) else args.val_bank
        check_probe_bank(vb, export, bias, classes)
        if bank_is_normalized(vb) != bank_is_normalized(bank):
            raise ValueError("--bank and --val_bank must both be normalized or both be raw")
        val = (vb["features"], vb["labels"])
    elif args.val_fraction is not None:
        train, val = split_bank(bank, args.val_fraction, args.seed)
    values = [float(v) for v in args.l2] if args.l2 else l2_grid(args.l2_grid, args.l2_min, args.l2_max) if args.l2_grid else [1e-3]
    if any(v < 0 for v in values):
        raise ValueError("--l2 must not be negative")
    if len(values) > 1 and val is None:
        raise ValueError("more than one l2 value needs --val_bank or --val_fraction to choose by")
    dev = TL.device(dev)
    with torch.cuda.device(dev):
        t0 = time.perf_counter()
        ev = DeviceEvaluator(classes, args.precision, args.chunk_rows, dev)
        kw = dict(bias=bias, max_iter=args.max_iter, evaluator=ev)
        if val is None:
            best = dict(fit_probe(train[0], train[1], classes, values[0], **kw), l2=values[0], val_top1=None)
            records = [dict(l2=values[0], F=best["F"], train_top1=best["top1"], val_top1=None, iterations=best["iterations"], evaluations=best["evaluations"])]
        else:
            records, best = sweep(train, val, values, classes, **kw)
        evaluations = sum(r["evaluations"] for r in records)
        refit = bool(args.refit) and val is not None
        if refit:                                                    # the chosen value on train + validation, from the chosen fit
            both = (torch.cat([train[0], val[0]]), torch.cat([train[1], val[1]]))
            again = fit_probe(both[0], both[1], classes, best["l2"], init=(best["W"], best["b"]), **kw)
            evaluations += again["evaluations"]
            best = dict(again, l2=best["l2"], val_top1=best["val_top1"])
        final_val = None
        if val is not None:
            vx, vy = ev.prepare(*val)
            final_val = score_head(best["W"], best["b"], vx, vy, classes)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    out = probe_head(export, best["W"], best["b"], classes)
    if args.output:
        torch.save(out, args.output)
    return dict(output=args.output, data_classes=classes, num_classes=out["cfg"]["num_classes"], bias=int(bias), precision=args.precision,
                normalized_bank=bank_is_normalized(bank), records=records, l2=best["l2"], refit=int(refit), F=best["F"], train_top1=best["top1"],
                val_top1=final_val, train_rows=best["rows"], evaluations=evaluations, seconds=dt, **CP._report(out))


def score_command(args, dev=None):
    export = CP.as_export(args.compact)
    bank = CT.load_bank(args.bank) if not isinstance(args.bank, dict) else args.bank
    CT.check_bank(bank, export)
    classes = int(bank["data_classes"])
    W, b = file_head(export, classes)
    if bank_is_normalized(bank) and bool((b != 0).any()):
        raise ValueError("the bank holds normalized features and the file's head has a non-zero bias: score it on a raw bank (python -m uvc_amd.compact_probe embed)")
    dev = TL.device(dev)
    with torch.cuda.device(dev):
        X = CT.operand(bank["features"].to(dev), args.precision).contiguous()
        top1 = score_head(W, b, X, bank["labels"].to(dev), classes)
    return dict(images=int(X.shape[0]), data_classes=classes, num_classes=int(export["cfg"]["num_classes"]), precision=args.precision,
                normalized_bank=bank_is_normalized(bank), top1=top1)


def build_parser():
    p = argparse.ArgumentParser(prog="python -m uvc_amd.compact_probe", description="A linear probe on a compact model's frozen features")
    sub = p.add_subparsers(dest="cmd", required=True)
    e, f, s = (sub.add_parser(n) for n in ("embed", "fit", "score"))
    for q in (e, f, s):
        q.add_argument("--compact", required=True, help="the compact file")
        q.add_argument("--precision", choices=["bf16", "fp32"], default="bf16")
    TL.add_dataset_flags(e, precision=False)
    e.add_argument("--output", required=True, help="the bank file: raw features, labels, data_classes, meta, normalized = False")
    f.add_argument("--bank", required=True, help="the bank to fit on (compact_probe embed --split train)")
    TL.add_val_flags(f, "a bank to choose l2 on")
    g = f.add_mutually_exclusive_group()
    g.add_argument("--l2", type=float, nargs="+", default=None, help="the regulariser value(s); default 1e-3")
    g.add_argument("--l2_grid", type=CP._int_in(1, 1000, "--l2_grid"), default=None, help="this many values, log-spaced in [--l2_min, --l2_max]")
    f.add_argument("--l2_min", type=float, default=1e-6)
    f.add_argument("--l2_max", type=float, default=1e-1)
    f.add_argument("--bias", type=int, default=1, choices=[0, 1])
    f.add_argument("--max_iter", type=CP._int_in(1, 1000000, "--max_iter"), default=1000)
    f.add_argument("--refit", type=int, default=1, choices=[0, 1], help="1: refit the chosen l2 on train + validation, warm-started")
    f.add_argument("--chunk_rows", type=CP._int_in(1, 2 ** 31 - 1, "--chunk_rows"), default=None, help="rows per pass of the evaluator (default: 64 MiB of logits + G)")
    f.add_argument("--output", required=True, help="the compact file with the fitted head")
    s.add_argument("--bank", required=True, help="the bank to score the file's head on")
    return p


def main(argv: Optional[Sequence[str]] = None):
    args = build_parser().parse_args(argv)
    if args.cmd == "embed":
        TL.need_data(args)
        summary = embed(args.compact, args)[1]
    else:
        summary = fit_command(args) if args.cmd == "fit" else score_command(args)
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
