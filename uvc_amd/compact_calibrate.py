"""Calibrate a compact model: expected calibration error, temperature scaling and vector scaling.

    python -m uvc_amd.compact_calibrate logits --compact F --dataset cifar10|cifar100|imagenet --data_dir D --split train|test --output val_logits.pt
    python -m uvc_amd.compact_calibrate fit    --compact F --bank val_logits.pt [--method temperature|vector] [--val_bank B | --val_fraction 0.1 --seed 0]
                                               [--bins 15] [--max_iter 500] [--chunk_rows N] --output G
    python -m uvc_amd.compact_calibrate score  --bank logits.pt [--bins 15]

Every compact command since ``predict`` reports probabilities; this one says whether they mean anything (the reliability diagram and
ECE) and corrects them post hoc (Guo et al., ICML 2017).  Both corrections are affine maps of the logits, ``z'_c = a_c z_c + d_c``
(temperature scaling: ``a_c = 1/T``, ``d = 0``), so a fitted calibration folds exactly into the file's head -- ``W'_c = a_c W_c``,
``b'_c = a_c b_c + d_c`` -- and the result is an ordinary version-1 compact file.  ``logits`` runs the eval transform over one split and
saves the model's eval logits; ``fit`` minimises the negative log-likelihood of the mapped logits by L-BFGS and writes the folded file;
``score`` prints the reliability record of a bank as it is (to score a calibrated file, run ``logits`` on it first).

The objective with its gradient is ``uvc_calib_eval`` (``ops.calib_eval``) and the reliability histogram ``uvc_calib_stats``
(``ops.calib_stats``): one pass over the logits each, nothing of their size written.  ``reference_objective`` and
``reference_reliability`` are the written specs (plain PyTorch float64) the tests hold them to; handed in as ``evaluator`` / ``scorer``
they also run the solver, ``fit`` and ``score`` on a bank without a device.
"""
from __future__ import annotations

import argparse
import json
import time
from typing import Optional, Sequence

import torch

from . import compact as CP
from . import compact_tools as TL

METHODS = ("temperature", "vector")
MAX_BINS = 64                                       # uvc_calib_stats' limit
BANK_KEYS = TL.LOGITS_BANK_KEYS
META_KEYS = tuple(k for k in TL.META_KEYS if k != "embed_dim")


# ---- written specs ----------------------------------------------------------------------------------------------------------------
def _mapped(logits, labels, scale, shift, classes):
    """float64 ``(z [m, C], z' [m, C], y [m])`` of the counted rows: ``z' = scale * z + shift`` over columns ``[0, classes)``."""
    C = int(classes)
    z = torch.as_tensor(logits).detach().double()[:, :C]
    y = torch.as_tensor(labels).detach().to(torch.int64)
    a = torch.as_tensor(scale).detach().double().reshape(-1)
    if a.numel() not in (1, C):
        raise ValueError(f"scale must hold 1 or {C} values, not {a.numel()}")
    keep = (y >= 0) & (y < C)
    z, y = z[keep], y[keep]
    zp = z * a
    if shift is not None:
        zp = zp + torch.as_tensor(shift).detach().double().reshape(C)
    return z, zp, y, a


def reference_objective(logits, labels, scale, shift, classes):
    """``(F, dscale, dshift, hits, m)`` in float64: over the m rows whose label lies in ``[0, C)``, with ``z'_ic = scale_c z_ic + shift_c``
    on the columns ``[0, C)``, ``p = softmax(z')`` and ``g_ic = p_ic - [c = y_i]``: ``F = (1/m) sum_i (lse(z'_i) - z'_{i, y_i})``;
    ``dscale_c = (1/m) sum_i g_ic z_ic`` (one value, the sum over c, when ``scale`` holds one); ``dshift_c = (1/m) sum_i g_ic`` (None
    without ``shift``); ``hits`` the rows whose label is the FIRST maximum of ``z'``.  m = 0 gives zeros."""
    z, zp, y, a = _mapped(logits, labels, scale, shift, classes)
    m, C = int(y.shape[0]), int(classes)
    if m == 0:
        return 0.0, torch.zeros(a.numel(), dtype=torch.float64), (None if shift is None else torch.zeros(C, dtype=torch.float64)), 0, 0
    F = float((torch.logsumexp(zp, dim=1) - zp.gather(1, y[:, None])[:, 0]).sum()) / m
    g = torch.softmax(zp, dim=1)
    g[torch.arange(m), y] -= 1.0
    gz = (g * z).sum(0) / m
    hits = int((zp.argmax(dim=1) == y).sum())                        # torch's argmax: the first maximum
    return F, (gz if a.numel() == C and C > 1 else gz.sum().reshape(1)), (None if shift is None else g.sum(0) / m), hits, m


def reference_reliability(logits, labels, scale, shift, classes, bins=15):
    """The raw sums ``reliability`` reads, in float64: per counted row ``conf = max_c p_c``, ``pred`` the first maximum,
    ``bin = clamp(ceil(conf * bins) - 1, 0, bins - 1)`` -- the intervals ``((j - 1) / bins, j / bins]``.  ``{"bin_count" int64 [bins],
    "bin_conf" float64 [bins] (sums), "bin_hit" int64 [bins], "nll_sum", "brier_sum" (sum_i (sum_c p_ic^2 - 2 p_{i, y_i} + 1)), "hits", "m",
    "conf" [m], "hit" [m]}``."""
    bins = int(bins)
    if not 1 <= bins <= MAX_BINS:
        raise ValueError(f"bins must lie in [1, {MAX_BINS}], not {bins}")
    z, zp, y, a = _mapped(logits, labels, scale, shift, classes)
    m = int(y.shape[0])
    p = torch.softmax(zp, dim=1)
    conf = p.max(dim=1).values if m else torch.zeros(0, dtype=torch.float64)
    hit = (zp.argmax(dim=1) == y) if m else torch.zeros(0, dtype=torch.bool)
    b = (torch.ceil(conf * bins).to(torch.int64) - 1).clamp(0, bins - 1)
    py = p.gather(1, y[:, None])[:, 0] if m else conf
    nll = (torch.logsumexp(zp, dim=1) - zp.gather(1, y[:, None])[:, 0]) if m else conf
    return dict(bin_count=torch.bincount(b, minlength=bins), bin_conf=torch.zeros(bins, dtype=torch.float64).index_add_(0, b, conf),
                bin_hit=torch.bincount(b, weights=hit.double(), minlength=bins).to(torch.int64), nll_sum=float(nll.sum()),
                brier_sum=float(((p * p).sum(1) - 2 * py + 1).sum()) if m else 0.0, hits=int(hit.sum()), m=m, conf=conf, hit=hit)


def reliability(bin_count, bin_conf, bin_hit, nll_sum, brier_sum, hits, m, **_):
    """The reliability record of the raw sums: ``ece = sum_j (n_j / m) |acc_j - conf_j|``, ``mce`` the largest gap of a non-empty bin,
    ``nll``, ``brier`` and ``top1`` (percent) over the m counted rows, and the three per-bin lists (count, mean confidence, accuracy;
    zeros for an empty bin)."""
    n = torch.as_tensor(bin_count).detach().cpu().double()
    m = int(m)
    full = n > 0
    conf = torch.where(full, torch.as_tensor(bin_conf).detach().cpu().double() / n.clamp_min(1), torch.zeros_like(n))
    acc = torch.where(full, torch.as_tensor(bin_hit).detach().cpu().double() / n.clamp_min(1), torch.zeros_like(n))
    gap = (acc - conf).abs()
    return dict(ece=float((n * gap).sum()) / m if m else 0.0, mce=float(gap[full].max()) if m else 0.0, nll=float(nll_sum) / m if m else 0.0,
                brier=float(brier_sum) / m if m else 0.0, top1=100.0 * int(hits) / m if m else 0.0, rows=m,
                bin_count=[int(v) for v in n.tolist()], bin_conf=conf.tolist(), bin_acc=acc.tolist())


def reference_scorer(logits, labels, scale, shift, classes, bins=15):
    """``reliability`` of ``reference_reliability``: the scorer of a bank on the CPU."""
    return reliability(**reference_reliability(logits, labels, scale, shift, classes, bins))


# ---- on the device ----------------------------------------------------------------------------------------------------------------
class DeviceEvaluator:
    """``evaluator(Z, y, scale, shift, classes)`` of ``fit_calibration`` on the device: ``ops.calib_eval`` on float32 masters.  ``prepare``
    moves a bank's logits to the device once.  ``chunk_rows``: rows per call (default: all of them in one); the chunks' results are
    weighted by their counted rows."""
    dtype = torch.float32

    def __init__(self, chunk_rows=None, device=None):
        self.device = TL.device(device)
        self.chunk_rows = None if chunk_rows is None else int(chunk_rows)
        self._ws = None

    def prepare(self, logits, labels):
        return logits.to(self.device, torch.float32).contiguous(), labels.to(self.device).contiguous()

    def _one(self, Z, y, scale, shift, classes):
        from . import ops
        n = Z.shape[0]
        need = ops.calib_workspace_bytes(n, Z.stride(0) if n > 1 else Z.shape[1], classes)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=Z.device)
        return ops.calib_eval(Z, y, scale, shift, classes, workspace=self._ws)

    def __call__(self, Z, y, scale, shift, classes):
        n = Z.shape[0]
        step = n if self.chunk_rows is None else max(1, self.chunk_rows)
        if step >= n:
            F, ds, dd, counts = self._one(Z, y, scale, shift, classes)
            return F, ds, dd, counts[0], counts[1]
        F = torch.zeros(1, dtype=torch.float64, device=Z.device)
        ds = torch.zeros(scale.numel(), dtype=torch.float64, device=Z.device)
        dd = None if shift is None else torch.zeros(classes, dtype=torch.float64, device=Z.device)
        counts = torch.zeros(2, dtype=torch.int64, device=Z.device)
        for r0 in range(0, n, step):
            f, s, d, c = self._one(Z[r0:r0 + step], y[r0:r0 + step], scale, shift, classes)
            w = c[1].double()
            F += f * w
            ds += s.double() * w
            if dd is not None:
                dd += d.double() * w
            counts += c
        inv = 1.0 / counts[1].clamp_min(1).double()
        return F * inv, (ds * inv).float(), None if dd is None else (dd * inv).float(), counts[0], counts[1]


def device_scorer(logits, labels, scale, shift, classes, bins=15, device=None):
    """``reliability`` of ``ops.calib_stats``: the scorer of a bank on the device (``logits`` and ``labels`` from anywhere)."""
    from . import ops
    dev = TL.device(device)
    with torch.cuda.device(dev):
        Z = torch.as_tensor(logits).to(dev, torch.float32).contiguous()
        y = torch.as_tensor(labels).to(dev).contiguous()
        a = torch.as_tensor(scale).to(dev, torch.float32).reshape(-1).contiguous()
        d = None if shift is None else torch.as_tensor(shift).to(dev, torch.float32).reshape(-1).contiguous()
        n, c, h, sums, counts = ops.calib_stats(Z, y, a, d, int(classes), int(bins))
        return reliability(n, c, h, float(sums[0]), float(sums[1]), int(counts[0]), int(counts[1]))


# ---- fitting ----------------------------------------------------------------------------------------------------------------------
def fit_calibration(logits, labels, classes, method="temperature", *, evaluator=None, max_iter=500, init=None, history=10, tol_grad=1e-6,
                    tol_change=None, chunk_rows=None):
    """L-BFGS (``torch.optim.LBFGS``, strong Wolfe line search, ``compact_probe.fit_probe``'s settings) on ``reference_objective``'s problem.
    ``"temperature"`` optimises ``u = log s`` (``dF/du = s dF/ds``), so ``s = 1/T > 0`` always; ``"vector"`` optimises ``(a [C], d [C])``
    from ``a = 1``, ``d = 0``, unconstrained.  ``evaluator(Z, y, scale, shift, classes)`` returns ``(F, dscale, dshift, hits, ...)``; None
    builds the device one (``DeviceEvaluator``: the float32 masters stay on the device), ``reference_objective`` is the float64 one on the
    CPU.  An evaluator may carry ``prepare(logits, labels)``, ``dtype`` and ``device`` of the parameters (default: float64, cpu).
    ``init``: ``(scale, shift)`` to start from.  Returns ``{"scale" [1] or [C], "shift" [C] or None, "temperature" (temperature mode), "F",
    "top1", "grad_inf", "iterations", "evaluations", "rows"}`` (tensors on the CPU in the parameters' dtype)."""
    classes = int(classes)
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, not {method!r}")
    if classes < 1:
        raise ValueError(f"classes {classes} must be at least 1")
    if evaluator is None:
        evaluator = DeviceEvaluator(chunk_rows)
    dtype, dev = getattr(evaluator, "dtype", torch.float64), getattr(evaluator, "device", "cpu")
    Z, y = evaluator.prepare(logits, labels) if hasattr(evaluator, "prepare") else (logits, labels)
    vector = method == "vector"
    if vector:
        a = torch.ones(classes, dtype=dtype, device=dev)
        d = torch.zeros(classes, dtype=dtype, device=dev)
        if init is not None:
            a.copy_(torch.as_tensor(init[0]).to(a).reshape(-1).expand(classes))
            if init[1] is not None:
                d.copy_(torch.as_tensor(init[1]).to(d).reshape(classes))
        params = [a.requires_grad_(), d.requires_grad_()]
    else:
        u = torch.zeros(1, dtype=dtype, device=dev)
        if init is not None:
            u.copy_(torch.as_tensor(init[0]).to(u).reshape(1).log())
        params = [u.requires_grad_()]

    def evaluate():
        if vector:
            F, ds, dd, hits = evaluator(Z, y, a.detach(), d.detach(), classes)[:4]
            a.grad, d.grad = torch.as_tensor(ds).to(a).reshape(a.shape), torch.as_tensor(dd).to(d).reshape(d.shape)
        else:
            s = u.detach().exp()
            F, ds, _, hits = evaluator(Z, y, s, None, classes)[:4]
            u.grad = (s * torch.as_tensor(ds).to(u).reshape(1))
        return F, hits

    F, last, g, iterations, evaluations = TL.lbfgs(params, evaluate, max_iter=max_iter, history=history, tol_grad=tol_grad, tol_change=tol_change,
                                                   dtype=dtype)
    m = int(((y >= 0) & (y < classes)).sum())
    out = dict(F=F, top1=100.0 * int(last["hits"]) / m if m else 0.0, grad_inf=g, iterations=iterations, evaluations=evaluations, rows=m)
    if vector:
        out.update(scale=a.detach().cpu().clone(), shift=d.detach().cpu().clone())
    else:
        s = u.detach().exp().cpu()
        out.update(scale=s, shift=None, temperature=1.0 / float(s))
    return out


# ---- banks ------------------------------------------------------------------------------------------------------------------------
def make_logits_bank(logits, labels, data_classes, **meta):
    """The logits bank's dict (``compact_tools.make_bank``): ``BANK_KEYS``, no ``embed_dim`` in ``meta``."""
    return TL.make_bank(labels, data_classes, logits=logits, **meta)


def check_logits_bank(bank, export=None, data_classes=None):
    """Refuses, by name, a dict that is not a logits bank (a feature bank cannot stand in: the eval logits of two differing heads cannot be
    rebuilt from the mean feature), or whose ``num_classes`` is not the file's, or whose ``data_classes`` is not the dataset's."""
    if not isinstance(bank, dict) or not set(BANK_KEYS) <= set(bank):
        what = "a feature bank" if isinstance(bank, dict) and "features" in bank else "not a logits bank"
        raise ValueError(f"{what}: need the keys {', '.join(BANK_KEYS)} (python -m uvc_amd.compact_calibrate logits writes them)")
    z, y = bank["logits"], bank["labels"]
    if not torch.is_tensor(z) or z.dim() != 2 or z.shape[1] != bank["num_classes"] or not torch.is_tensor(y) or tuple(y.shape) != (z.shape[0],):
        raise ValueError(f"the bank's logits must be [n, num_classes = {bank['num_classes']}] with one label per row")
    if not 1 <= bank["data_classes"] <= bank["num_classes"]:
        raise ValueError(f"the bank's data_classes {bank['data_classes']} is not within its num_classes {bank['num_classes']}")
    if export is not None and bank["num_classes"] != export["cfg"]["num_classes"]:
        raise ValueError(f"the bank's num_classes {bank['num_classes']} is not the file's num_classes {export['cfg']['num_classes']}")
    if data_classes is not None and bank["data_classes"] != data_classes:
        raise ValueError(f"the bank's data_classes {bank['data_classes']} is not the dataset's data_classes {data_classes}")
    return bank


def load_logits_bank(path) -> dict:
    bank = torch.load(path, map_location="cpu")
    try:
        return check_logits_bank(bank)
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from None


def logits_command(export_or_path, args, dev=None):
    """``logits``: the bank dict of ``args.split`` -- ``forward``'s eval logits of every batch -- (saved to ``args.output`` when given) and
    the summary."""
    export = CP.as_export(export_or_path)
    return TL.bank_command(export, args, dev, lambda model, x: (model(x)[0].float(),),
                           lambda z, labels, classes, **meta: check_logits_bank(make_logits_bank(z, labels, classes, **meta), export, classes),
                           lambda bank: dict(num_classes=bank["num_classes"]))


# ---- the file ---------------------------------------------------------------------------------------------------------------------
def calibrated_head(export, scale, shift, classes):
    """A version-1 compact file whose logits are ``scale * z + shift`` on the columns ``[0, classes)``: rows ``[0, classes)`` of ``head`` become
    ``W'_c = a_c W_c``, ``b'_c = a_c b_c + d_c``, folded in float64 and rounded once to the stored dtype; ``head_dist`` gets the same
    ``(a, d)``, so the mean of the two heads is ``a * mean + d``.  Every other tensor keeps its bits -- the padding rows too."""
    CP.check_export(export)
    classes = int(classes)
    a = torch.as_tensor(scale).detach().double().reshape(-1)
    if a.numel() not in (1, classes):
        raise ValueError(f"calibrated_head: scale must hold 1 or {classes} values, not {a.numel()}")
    a = a.expand(classes)
    d = torch.zeros(classes, dtype=torch.float64) if shift is None else torch.as_tensor(shift).detach().double().reshape(-1)
    if d.numel() != classes:
        raise ValueError(f"calibrated_head: shift must hold {classes} values, not {d.numel()}")
    if not 1 <= classes <= export["cfg"]["num_classes"]:
        raise ValueError(f"classes {classes} is not within the file's num_classes {export['cfg']['num_classes']}")
    sd = {k: v.clone() for k, v in export["state_dict"].items()}
    for name in ("head", "head_dist"):
        if name + ".weight" in sd:
            w, b = sd[name + ".weight"], sd[name + ".bias"]
            w[:classes] = (a[:, None] * w[:classes].double()).to(w.dtype)
            b[:classes] = (a * b[:classes].double() + d).to(b.dtype)
    return CP.with_state(export, sd)


# ---- the commands -----------------------------------------------------------------------------------------------------------------
def _bank_arg(b):
    return load_logits_bank(b) if not isinstance(b, dict) else check_logits_bank(b)


def fit_command(args, dev=None, evaluator=None, scorer=None):
    """``fit``.  ``evaluator`` / ``scorer``: None runs on the device (``DeviceEvaluator``, ``device_scorer``); ``reference_objective`` and
    ``reference_scorer`` run the same command on the CPU."""
    export = CP.as_export(args.compact)
    bank = check_logits_bank(_bank_arg(args.bank), export)
    classes = int(bank["data_classes"])
    fit, val = (bank["logits"], bank["labels"]), None
    if args.val_bank is not None:
        vb = check_logits_bank(_bank_arg(args.val_bank), export, classes)
        val = (vb["logits"], vb["labels"])
    elif args.val_fraction is not None:
        fit, val = TL.split_bank(dict(features=bank["logits"], labels=bank["labels"]), args.val_fraction, args.seed)
    on_device = evaluator is None or scorer is None
    if on_device:
        dev = TL.device(dev)
    if evaluator is None:
        evaluator = DeviceEvaluator(args.chunk_rows, dev)
    if scorer is None:
        scorer = lambda z, y, a, d, c, bins: device_scorer(z, y, a, d, c, bins, dev)
    one = torch.ones(1)
    record = lambda a, d: dict(fit=scorer(fit[0], fit[1], a, d, classes, args.bins), val=None if val is None else scorer(val[0], val[1], a, d, classes, args.bins))
    t0 = time.perf_counter()
    before = record(one, None)
    if on_device:
        with torch.cuda.device(dev):
            res = fit_calibration(fit[0], fit[1], classes, args.method, evaluator=evaluator, max_iter=args.max_iter)
            torch.cuda.synchronize()
    else:
        res = fit_calibration(fit[0], fit[1], classes, args.method, evaluator=evaluator, max_iter=args.max_iter)
    after = record(res["scale"], res["shift"])
    dt = time.perf_counter() - t0
    out = calibrated_head(export, res["scale"], res["shift"], classes)
    if args.output:
        torch.save(out, args.output)
    line = dict(output=args.output, method=args.method)
    if args.method == "temperature":
        line["temperature"] = res["temperature"]
    line.update(data_classes=classes, num_classes=out["cfg"]["num_classes"], rows=res["rows"], evaluations=res["evaluations"], seconds=dt,
                before=before, after=after, **CP._report(out))
    return line, res


def score_command(args, dev=None, scorer=None):
    bank = _bank_arg(args.bank)
    if scorer is None:
        dev = TL.device(dev)
        scorer = lambda z, y, a, d, c, bins: device_scorer(z, y, a, d, c, bins, dev)
    rec = scorer(bank["logits"], bank["labels"], torch.ones(1), None, int(bank["data_classes"]), args.bins)
    return dict(images=int(bank["logits"].shape[0]), data_classes=int(bank["data_classes"]), num_classes=int(bank["num_classes"]), bins=int(args.bins), **rec)


def build_parser():
    p = argparse.ArgumentParser(prog="python -m uvc_amd.compact_calibrate", description="Reliability, temperature scaling and vector scaling of a compact model")
    sub = p.add_subparsers(dest="cmd", required=True)
    l, f, s = (sub.add_parser(n) for n in ("logits", "fit", "score"))
    for q in (l, f):
        q.add_argument("--compact", required=True, help="the compact file")
    TL.add_dataset_flags(l)
    l.add_argument("--output", required=True, help="the bank file: eval logits, labels, data_classes, num_classes, meta")
    f.add_argument("--bank", required=True, help="the logits bank to fit on (a held-out split: compact_calibrate logits)")
    f.add_argument("--method", choices=list(METHODS), default="temperature")
    TL.add_val_flags(f, "a logits bank to report the held-out record on")
    f.add_argument("--max_iter", type=CP._int_in(1, 1000000, "--max_iter"), default=500)
    f.add_argument("--chunk_rows", type=CP._int_in(1, 2 ** 31 - 1, "--chunk_rows"), default=None, help="rows per call of the evaluator (default: the whole bank)")
    f.add_argument("--output", required=True, help="the compact file with the calibration folded into its head")
    s.add_argument("--bank", required=True, help="the logits bank to score as it is")
    for q in (f, s):
        q.add_argument("--bins", type=CP._int_in(1, MAX_BINS, "--bins"), default=15)
    return p


def main(argv: Optional[Sequence[str]] = None):
    args = build_parser().parse_args(argv)
    if args.cmd == "logits":
        TL.need_data(args)
        summary = logits_command(args.compact, args)[1]
    else:
        summary = fit_command(args)[0] if args.cmd == "fit" else score_command(args)
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
