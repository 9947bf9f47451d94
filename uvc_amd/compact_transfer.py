"""Transfer a compact model to a new label set: its features for a dataset, the weighted k-NN top-1 of those features, and a new head.

    python -m uvc_amd.compact_transfer embed  --compact F --dataset cifar10|cifar100|imagenet --data_dir D --split train|test --output bank.pt
    python -m uvc_amd.compact_transfer knn    --compact F --dataset ... --data_dir D [--bank bank.pt] [--k 20] [--temperature 0.07]
    python -m uvc_amd.compact_transfer rehead --compact F --bank bank.pt --output G [--init mean|zero] [--scale 10.0]

A compact file is tied to the label set it was trained on (``cfg["num_classes"]`` and the stored head).  ``embed`` runs the EVAL transform
over one split in dataset order and saves the normalised features (``CompactVisionTransformer.features``: the final-norm readout rows the
heads read, their mean with the distillation token -- ``uvc_vit_compact_features``).  ``knn`` is the standard training-free transfer
measure (Wu et al. 2018; DINO's ``knn_classifier``): every test feature's k most similar train features (``uvc_knn_topk``: the bank
streams through the MFMA against the queries and each query's running top-k stays on chip; no ``[nq, n]`` similarity matrix is written)
vote with weights ``exp((s_j - s_0) / T)`` (``uvc_knn_vote``).  ``rehead`` writes a version-1 compact file whose head(s) cover the new
classes, zero or the nearest-class-mean classifier of a bank, which ``python -m uvc_amd.compact finetune`` then trains as it is.

``reference_features``, ``reference_knn`` and ``reference_vote`` are the written specs (plain PyTorch / numpy float64) the tests hold the
kernels to.
"""
from __future__ import annotations

import argparse
import json
import time
from typing import Optional, Sequence

import torch
import torch.nn.functional as F

from . import compact as CP
from . import compact_tools as TL

MAX_K = 64                                          # uvc_knn_topk's and uvc_knn_vote's limit
HEAD_MULTIPLE = 8                                   # the engine's head widths (data.build_loaders: 10 -> 16, 100 -> 104)
INITS = ("mean", "zero")


# ---- written specs ----------------------------------------------------------------------------------------------------------------
def reference_features(export: dict, x: torch.Tensor, normalize: bool = True) -> torch.Tensor:
    """``[B, D]`` in x's dtype: the mean over the readout rows of ``compact._reference_walk``'s network after the final norm (the class
    row; ``(cls + dist) / 2`` with the distillation token), through ``F.normalize(eps=1e-12)`` with ``normalize``."""
    with torch.no_grad():
        rows = CP._reference_walk(export, x, keep_readout=True)[3]
    f = rows.mean(dim=1)
    return F.normalize(f, dim=1, eps=1e-12) if normalize else f


def reference_knn(queries, bank, k: int):
    """``(sims float64 [nq, k], idx int64 [nq, k])`` (numpy): the float64 dot products of the operands as given, the k largest of every
    query first, in the order ``numpy.lexsort((index, -sim))`` -- equal values by ascending bank row.  A NaN or -inf similarity is
    never listed; slots a short bank leaves are ``(-inf, -1)``."""
    import numpy as np
    q = np.asarray(torch.as_tensor(queries).detach().cpu().double().numpy())
    b = np.asarray(torch.as_tensor(bank).detach().cpu().double().numpy())
    with np.errstate(invalid="ignore", over="ignore"):
        s = q @ b.T
    nq, n = s.shape
    sims, idx = np.full((nq, k), -np.inf), np.full((nq, k), -1, dtype=np.int64)
    for i in range(nq):
        ok = np.nonzero(~np.isnan(s[i]) & (s[i] > -np.inf))[0]
        order = ok[np.lexsort((ok, -s[i, ok]))][:k]
        sims[i, :len(order)], idx[i, :len(order)] = s[i, order], order
    return sims, idx


def reference_vote(sims, idx, labels, num_classes: int, temperature: float = 0.07):
    """``(scores float64 [nq, C], pred int64 [nq])`` (numpy): ``w_j = exp((s_j - s_0) / T)`` with s_0 the row's first similarity and T
    rounded to float32 as the kernel takes it (``w_j = 1`` where ``s_j == s_0`` and for every j with ``T <= 0``);
    ``score[c] = sum_j w_j [label(idx_j) == c]``, j ascending.  Slots with an index outside the labels and labels outside ``[0, C)``
    count for nothing; pred is the first maximum, -1 for a row without a valid neighbour."""
    import numpy as np
    s = np.asarray(torch.as_tensor(sims).detach().cpu().double().numpy())
    ix = np.asarray(torch.as_tensor(idx).detach().cpu().numpy()).astype(np.int64)
    lab = np.asarray(torch.as_tensor(labels).detach().cpu().numpy()).astype(np.int64)
    T = float(np.float32(temperature))
    nq, k = s.shape
    scores, pred = np.zeros((nq, num_classes)), np.full(nq, -1, dtype=np.int64)
    for i in range(nq):
        valid = False
        for j in range(k):
            if not 0 <= ix[i, j] < len(lab) or not 0 <= lab[ix[i, j]] < num_classes:
                continue
            valid = True
            w = 1.0 if T <= 0 or s[i, j] == s[i, 0] else float(np.exp((s[i, j] - s[i, 0]) / T))
            scores[i, lab[ix[i, j]]] += w
        if valid:
            pred[i] = int(np.argmax(scores[i]))
    return scores, pred


# ---- features of a dataset ----------------------------------------------------------------------------------------------------------
def _features(model, x):
    """The walk's call: the normalised float32 features of one batch."""
    return (model.features(x)[1],)


def operand(features, precision):
    """The features in the precision's operand type: bfloat16 under "bf16", rounded once from the normalised float32 features."""
    return features.to(torch.bfloat16) if precision == "bf16" else features.float()


def knn_classify(queries, bank, labels, num_classes, k=20, temperature=0.07):
    """int32 [nq] on the device: the weighted k-NN prediction of every query (``ops.knn_topk`` then ``ops.knn_vote``).  ``queries`` and
    ``bank`` share a dtype (bfloat16 or float32); k is capped by the bank's rows."""
    from . import ops
    k = min(int(k), bank.shape[0])
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k must lie in [1, {MAX_K}], not {k}")
    sims, idx = ops.knn_topk(queries.contiguous(), bank, k)
    return ops.knn_vote(sims, idx, labels, num_classes, temperature, scores=False)[1]


# ---- the bank file ------------------------------------------------------------------------------------------------------------------
META_KEYS = TL.META_KEYS


def make_bank(features, labels, data_classes, **meta):
    """The bank file's dict (``compact_tools.make_bank``): ``{"features", "labels", "data_classes", "meta"}``."""
    return TL.make_bank(labels, data_classes, features=features, **meta)


def load_bank(path) -> dict:
    bank = torch.load(path, map_location="cpu")
    if not isinstance(bank, dict) or not {"features", "labels", "data_classes", "meta"} <= set(bank):
        raise ValueError(f"{path}: not a feature bank (python -m uvc_amd.compact_transfer embed writes one)")
    return bank


def check_bank(bank, export, data_classes=None):
    """Refuses, by name, a bank whose ``embed_dim`` is not the model's, or whose ``data_classes`` is not the dataset's."""
    D = export["cfg"]["embed_dim"]
    got = bank["meta"].get("embed_dim", bank["features"].shape[1])
    if got != D or bank["features"].shape[1] != D:
        raise ValueError(f"the bank's embed_dim {got} is not the model's embed_dim {D}")
    if data_classes is not None and bank["data_classes"] != data_classes:
        raise ValueError(f"the bank's data_classes {bank['data_classes']} is not the dataset's data_classes {data_classes}")
    return bank


# ---- a head for the new classes --------------------------------------------------------------------------------------------------------
def rehead(export: dict, bank: Optional[dict], init: str = "mean", scale: float = 10.0):
    """``(new export, class-mean top-1 on the bank in percent, or None)``: a version-1 compact file whose ``cfg["num_classes"]`` is the
    bank's ``data_classes`` rounded up to a multiple of 8 and whose ``head`` (and ``head_dist``) are ONE new ``[C', D]`` weight with a
    zero bias; every other tensor and value is the input's (cloned, bit for bit).  ``init="mean"``: row c = ``scale`` times the
    normalised mean of class c's bank features, the nearest-class-mean classifier; a class absent from the bank and the padding rows
    are zeros.  ``init="zero"``: all zeros (``bank`` then only names the class count)."""
    CP.check_export(export)
    if init not in INITS:
        raise ValueError(f"init must be one of {INITS}, not {init!r}")
    if bank is None:
        raise ValueError("rehead needs a bank: its data_classes is the new label set")
    check_bank(bank, export)
    classes = int(bank["data_classes"])
    if classes < 1:
        raise ValueError(f"data_classes {classes} must be at least 1")
    D = export["cfg"]["embed_dim"]
    width = -(-classes // HEAD_MULTIPLE) * HEAD_MULTIPLE
    W = torch.zeros(width, D, dtype=torch.float64)
    top1 = None
    if init == "mean":
        f, y = bank["features"].double(), bank["labels"].to(torch.int64)
        keep = (y >= 0) & (y < classes)
        W.index_add_(0, y[keep], f[keep])
        W = float(scale) * F.normalize(W, dim=1, eps=1e-12)          # (an absent class: a zero row stays zero)
        pred = (f @ W[:classes].T).argmax(dim=1)                     # torch's argmax: the first maximum
        top1 = 100.0 * float((pred == y).double().mean())
    sd = {k: v.clone() for k, v in export["state_dict"].items()}
    for name in ("head", "head_dist"):
        if name + ".weight" in sd:
            sd[name + ".weight"] = W.to(sd[name + ".weight"].dtype)
            sd[name + ".bias"] = torch.zeros(width, dtype=sd[name + ".bias"].dtype)
    return CP.with_state(export, sd, dict(export["cfg"], num_classes=width)), top1


# ---- the commands ---------------------------------------------------------------------------------------------------------------------
def embed(export_or_path, args, dev=None):
    """``embed``: the bank dict of ``args.split`` (saved to ``args.output`` when given) and the summary ``{"images", "img_per_s", ...}``."""
    return TL.bank_command(export_or_path, args, dev, _features, make_bank, lambda bank: dict(embed_dim=int(bank["features"].shape[1])))


def evaluate(export_or_path, args, dev=None):
    """``knn``: the weighted k-NN top-1 of the test split against the train split's features (or ``args.bank``): the summary
    ``{"k", "temperature", "bank_images", "query_images", "top1", "img_per_s"}`` plus ``compact._report``'s widths, parameters and MACs.
    The bank is held on the device in the precision's operand type; the test split is embedded, searched and voted on batch by batch."""
    export = CP.as_export(export_or_path)
    dev = TL.device(dev)
    if not 1 <= int(args.k) <= MAX_K:
        raise ValueError(f"--k must lie in [1, {MAX_K}], not {args.k}")
    model = CP.CompactVisionTransformer(export, precision=args.precision, device=dev)
    test_loader, classes = TL.eval_loader(export, args, "test")
    with torch.cuda.device(dev):
        if getattr(args, "bank", None):
            bank = check_bank(load_bank(args.bank) if not isinstance(args.bank, dict) else args.bank, export, classes)
            feats, labels = bank["features"].to(dev), bank["labels"].to(dev)
        else:
            (feats,), labels = TL.walk(TL.eval_loader(export, args, "train")[0], lambda x: _features(model, x))
        bank_t = operand(feats, args.precision).contiguous()
        del feats
        hits = torch.zeros((), dtype=torch.int64, device=dev)
        n = 0
        t0 = time.perf_counter()
        for x, y in test_loader:
            q = operand(model.features(x)[1], args.precision)
            pred = knn_classify(q, bank_t, labels, classes, args.k, args.temperature)
            hits += (pred.to(torch.int64) == y.to(torch.int64)).sum()
            n += int(y.shape[0])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    if n == 0:
        raise ValueError("the test split is empty")
    return dict(k=min(int(args.k), int(bank_t.shape[0])), temperature=float(args.temperature), bank_images=int(bank_t.shape[0]), query_images=n,
                top1=100.0 * int(hits) / n, img_per_s=n / dt if dt > 0 else 0.0, **CP._report(export))


def build_parser():
    p = argparse.ArgumentParser(prog="python -m uvc_amd.compact_transfer",
                                description="Features, k-NN top-1 and a new head for a compact model on another dataset")
    sub = p.add_subparsers(dest="cmd", required=True)
    for name in ("embed", "knn", "rehead"):
        s = sub.add_parser(name)
        s.add_argument("--compact", required=True, help="the compact file")
        TL.add_dataset_flags(s, split=name == "embed")                 # (rehead reads none of them and goes on accepting them)
    e, k, r = (sub.choices[n] for n in ("embed", "knn", "rehead"))
    e.add_argument("--output", required=True, help="the bank file: features, labels, data_classes, meta")
    k.add_argument("--bank", default=None, help="a bank of the train split (embed --split train); default: embed it now")
    k.add_argument("--k", type=CP._int_in(1, MAX_K, "--k"), default=20)
    k.add_argument("--temperature", type=float, default=0.07, help="weights exp((s_j - s_0) / T); T <= 0: a plain majority")
    r.add_argument("--bank", required=True, help="the bank whose data_classes is the new label set (and whose class means init the head)")
    r.add_argument("--output", required=True, help="the re-headed compact file")
    r.add_argument("--init", choices=list(INITS), default="mean")
    r.add_argument("--scale", type=float, default=10.0, help="--init mean: the norm of every class row (a logit is scale * cosine)")
    return p


def main(argv: Optional[Sequence[str]] = None):
    args = build_parser().parse_args(argv)
    if args.cmd == "rehead":                             # a host operation: no device, no dataset
        export = CP.load_compact(args.compact)
        bank = load_bank(args.bank)
        out, top1 = rehead(export, bank, init=args.init, scale=args.scale)
        torch.save(out, args.output)
        summary = dict(output=args.output, init=args.init, scale=args.scale, num_classes=out["cfg"]["num_classes"],
                       data_classes=int(bank["data_classes"]), class_mean_top1=top1)
        print(json.dumps(summary))
        return summary
    TL.need_data(args)
    summary = embed(args.compact, args)[1] if args.cmd == "embed" else evaluate(args.compact, args)
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
