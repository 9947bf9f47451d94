"""What the stand-alone compact tools share (``compact_transfer``, ``compact_probe``, ``compact_calibrate``, ``compact_ood``,
``compact_compare``, ``compact_robust``, ``compact_corrupt``): the dataset flags, written once, the eval loader of a compact file, the walk over one split that ends in a bank file,
the bank dict, the held-out split of a bank and the L-BFGS driver.  A flag of the dataset block is added here and nowhere else; what the
image-file tools share (``compact predict`` / ``explain`` / ``attribute``, ``compact_pixel``, ``compact_perturb``) is in ``compact``.
"""
from __future__ import annotations

import argparse
import math
import time

import torch

from . import compact as CP

META_KEYS = ("img_size", "dataset", "split", "interpolation", "crop_pct", "precision", "embed_dim")
FEATURE_BANK_KEYS = ("features", "labels", "data_classes", "meta", "logits", "num_classes", "normalized")      # the order the files have always had
LOGITS_BANK_KEYS = ("logits", "labels", "data_classes", "num_classes", "meta")


def device(dev):
    from . import _lib as L
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    dev = torch.device(dev)
    if dev.type != "cuda":
        raise L.UvcHipError("uvc_amd models run on MI355X only (no CPU fallback)")
    return dev


# ---- one split under the eval transform ---------------------------------------------------------------------------------------------
def add_dataset_flags(p, *, eval_batch_size=256, split_default="train", precision=True, split=True):
    """--dataset --data_dir --eval_batch_size --num_workers [--precision] --interpolation --crop_pct --packed_dir --resident [--split]: what
    ``eval_loader`` reads.  ``precision=False``: the caller has the flag already."""
    from .data import INTERPOLATIONS
    p.add_argument("--dataset", choices=["cifar10", "cifar100", "imagenet"], default="imagenet")
    p.add_argument("--data_dir", default=None)
    p.add_argument("--eval_batch_size", type=CP._int_in(1, 65535, "--eval_batch_size"), default=eval_batch_size)
    p.add_argument("--num_workers", type=int, default=8, help="decode threads (at most 16)")
    if precision:
        p.add_argument("--precision", choices=["bf16", "fp32"], default="bf16")
    p.add_argument("--interpolation", choices=list(INTERPOLATIONS), default="bilinear")
    p.add_argument("--crop_pct", type=CP._crop_pct_arg, default=None)
    p.add_argument("--packed_dir", default=None, help="DIR/train.uvcpack and DIR/val.uvcpack replace the folders or pickles under --data_dir")
    p.add_argument("--resident", type=int, default=0, choices=[0, 1], help="1: keep the split's pixels on the device")
    if split:
        p.add_argument("--split", choices=["train", "test"], default=split_default)


def need_data(args):
    if not args.data_dir and not args.packed_dir:
        raise SystemExit("need --data_dir or --packed_dir")


def eval_loader(export, args, split):
    """``(loader, data_classes)`` of ``split`` under the eval transform at the file's image size (``args.img_size`` is set from it)."""
    from . import data
    args.img_size = export["cfg"]["img_size"]
    return data.build_eval_loader(args, split)


@torch.no_grad()
def walk(loader, per_batch):
    """``(outputs, labels int64 [n])`` on the device: ``per_batch(x)``'s tuple of tensors, each concatenated over every batch ``loader``
    yields, in its order (an eval loader: dataset order, the short last batch included)."""
    outs, labels = [], []
    for x, y in loader:
        outs.append(per_batch(x))
        labels.append(y.to(torch.int64))
    if not labels:
        raise ValueError("the loader yields no batch")
    return tuple(torch.cat(t) for t in zip(*outs)), torch.cat(labels)


def bank_command(export_or_path, args, dev, per_batch, make, summary_extra):
    """The command that walks ``args.split`` and writes a bank: ``(bank, summary)``.  ``per_batch(model, x)`` is the tool's own model call on
    a ``CompactVisionTransformer``; ``make(*outputs, labels, data_classes, **meta)`` turns the walk's result into the bank dict, saved to
    ``args.output`` when given; the summary is ``{"output", "images", "img_per_s", "data_classes"}`` plus ``summary_extra(bank)``."""
    export = CP.as_export(export_or_path)
    dev = device(dev)
    model = CP.CompactVisionTransformer(export, precision=args.precision, device=dev)
    loader, classes = eval_loader(export, args, args.split)
    with torch.cuda.device(dev):
        t0 = time.perf_counter()
        outs, labels = walk(loader, lambda x: per_batch(model, x))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    bank = make(*outs, labels, classes, img_size=export["cfg"]["img_size"], dataset=args.dataset, split=args.split,
                interpolation=args.interpolation, crop_pct=args.crop_pct, precision=args.precision)
    output = getattr(args, "output", None)
    if output:
        torch.save(bank, output)
    n = int(labels.shape[0])
    return bank, dict(output=output, images=n, img_per_s=n / dt if dt > 0 else 0.0, data_classes=classes, **summary_extra(bank))


# ---- banks ----------------------------------------------------------------------------------------------------------------------------
def make_bank(labels, data_classes, *, features=None, logits=None, normalized=None, **meta):
    """A bank file's dict, tensors (float32 / int64, CPU) and plain values only: ``labels``, ``data_classes`` and ``meta`` (its
    ``META_KEYS``, anything else dropped); with ``features`` [n, D] also ``meta["embed_dim"]``, with ``logits`` [n, num_classes] also
    ``num_classes``, and ``normalized`` when it is said."""
    labels = labels.detach().to(torch.int64).cpu().contiguous()
    meta = {k: meta.get(k) for k in META_KEYS if k != "embed_dim"}
    bank = dict(labels=labels, data_classes=int(data_classes), meta=meta)
    if features is not None:
        features = features.detach().float().cpu().contiguous()
        if features.dim() != 2 or labels.shape != (features.shape[0],):
            raise ValueError("features [n, D] and one label per row")
        bank["features"], meta["embed_dim"] = features, int(features.shape[1])
    if logits is not None:
        logits = logits.detach().float().cpu().contiguous()
        if logits.dim() != 2 or labels.shape != (logits.shape[0],):
            raise ValueError("logits [n, num_classes]" + (": one row per feature row" if features is not None else " and one label per row"))
        bank.update(logits=logits, num_classes=int(logits.shape[1]))
    if normalized is not None:
        bank["normalized"] = bool(normalized)
    return {k: bank[k] for k in (FEATURE_BANK_KEYS if features is not None else LOGITS_BANK_KEYS) if k in bank}


def split_bank(bank, fraction, seed):
    """``(train, val)`` as ``(features, labels)``: the last ``floor(fraction * n)`` rows of a CPU ``torch.Generator(seed)`` permutation are held out."""
    n = bank["features"].shape[0]
    k = int(math.floor(float(fraction) * n))
    if not 0 < k < n:
        raise ValueError(f"--val_fraction {fraction} holds out {k} of {n} rows")
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(int(seed)))
    tr, va = perm[:n - k], perm[n - k:]
    return (bank["features"][tr], bank["labels"][tr]), (bank["features"][va], bank["labels"][va])


def _fraction(v):
    f = float(v)
    if not 0.0 < f < 1.0:
        raise argparse.ArgumentTypeError(f"--val_fraction must lie in (0, 1), not {v}")
    return f


def add_val_flags(p, val_bank_help):
    """--val_bank | --val_fraction, and the --seed of ``split_bank``."""
    v = p.add_mutually_exclusive_group()
    v.add_argument("--val_bank", default=None, help=val_bank_help)
    v.add_argument("--val_fraction", type=_fraction, default=None, help="hold out this fraction of --bank (a --seed permutation's last rows)")
    p.add_argument("--seed", type=int, default=0)


# ---- fitting --------------------------------------------------------------------------------------------------------------------------
def lbfgs(params, evaluate, *, max_iter, history, tol_grad, tol_change, dtype):
    """``torch.optim.LBFGS`` with the strong Wolfe line search over ``params`` (leaves of ``dtype``).  ``evaluate()`` returns ``(F, hits)``
    at the parameters' present values and places the gradient in their ``.grad``.  Returns ``(F, last, grad_inf, iterations, evaluations)``:
    the objective, ``{"F", "hits"}`` and the gradient's largest entry from one more evaluation AT the returned point, which is counted."""
    tol_change = (0.0 if dtype == torch.float64 else 1e-11) if tol_change is None else tol_change      # (the device's F is summed in float64: changes below torch's default 1e-9 still carry signal)
    opt = torch.optim.LBFGS(params, lr=1.0, max_iter=int(max_iter), max_eval=int(max_iter) * 5 // 4 + 1, history_size=int(history),
                            tolerance_grad=float(tol_grad), tolerance_change=float(tol_change), line_search_fn="strong_wolfe")
    last = {}

    def closure():
        with torch.no_grad():
            F, hits = evaluate()
        F = torch.as_tensor(F, dtype=torch.float64).reshape(())
        last.update(F=F, hits=hits)
        return F

    opt.step(closure)
    F = closure()
    st = opt.state[params[0]]
    return float(F), last, max(float(p.grad.abs().max()) for p in params), int(st.get("n_iter", 0)), int(st.get("func_evals", 0)) + 1
