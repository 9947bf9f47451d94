"""Two compact models used together: the small one answers the images it is sure of, the rest go to the large one (a model cascade:
Viola & Jones 2001; Wang et al. 2021).  "At what share of the parent's MACs do I get the parent's top-1 back?"

    python -m uvc_amd.compact_cascade curve   --bank_small S.pt --bank_large L.pt (--small s.compact.pt --large l.compact.pt | --macs_small X --macs_large Y)
                                              [--score msp|margin|entropy] [--temperature T] [--match_large EPS | --target_accuracy A | --max_macs M]
                                              [--points 101] [--policy policy.json] [--output curve.pt]
    python -m uvc_amd.compact_cascade run     --small s.compact.pt --large l.compact.pt (--policy policy.json | --threshold TAU [--score] [--temperature])
                                              --dataset cifar10|cifar100|imagenet --data_dir D [--split test] [--bank out.pt]
    python -m uvc_amd.compact_cascade predict --small s.compact.pt --large l.compact.pt (--policy policy.json | --threshold TAU ...) --images photos/

The rule.  ``z`` is the small model's logits, ``C = data_classes`` its valid columns (padding columns never take part), ``T > 0`` a temperature
(``compact_calibrate fit``'s value makes confidences comparable; it is taken as its float32 value).  A score is higher for a surer row:

    msp      max_c softmax(z / T)_c
    margin   the largest minus the second largest entry of softmax(z / T); 1 at C = 1
    entropy  1 + sum_c p_c log p_c / log C with 0 log 0 = 0; 1 at C = 1

The small model's answer stands iff ``score >= tau`` compared in float32, otherwise the row is DEFERRED to the large model; a NaN score
defers; ``tau = -inf`` never defers and ``tau = +inf`` always does.  The small model always runs, so an image costs ``macs_small + defer_rate *
macs_large``.  Two models only.

``curve`` needs no model and no dataset: two logit banks of one split in one order (``compact_calibrate logits``, ``compact_ood bank``,
``compact_compare run --bank_a/--bank_b`` write them; ``compact_compare.check_pair`` refuses what is not).  It sweeps every threshold -- one
point per distinct score value, a threshold always being the float32 score of the last row kept, so the same scores reproduce the same
split; the two ends are ``+inf`` and ``-inf`` -- by a stable sort and int64 prefix sums, and picks an operating point.  ``run`` walks a
split once through the device cascade; ``predict`` is ``compact predict`` with ``"model"`` and ``"score"`` in every record.

On the device (``Cascade.forward``; uvc_amd/csrc/cascade.hip): patch rows once, the small forward, ``ops.cascade_decide``,
``ops.cascade_compact``, ONE 4-byte read of the deferred count, ``ops.cascade_gather`` of the deferred images' patch rows into a dense
batch, the large forward on it, ``ops.cascade_merge``.  ``reference_scores``, ``reference_cascade`` and ``reference_curve`` are the written
specs in float64 PyTorch; every bank command runs without a device through them (``scorer=reference_scorer``).
"""
from __future__ import annotations

import argparse
import json
import math
import time
from typing import Optional, Sequence

import torch

from . import compact as CP
from . import compact_compare as CC
from . import compact_tools as TL

SCORES = ("msp", "margin", "entropy")
POINT_KEYS = ("defer_rate", "threshold", "accuracy", "macs")
POLICY_KEYS = ("score", "temperature", "threshold", "data_classes", "img_size", "patch_size", "macs_small", "macs_large", "expected")
INF = math.inf


# ---- the rule -------------------------------------------------------------------------------------------------------------------------
def check_rule(score="msp", temperature=1.0, threshold=None):
    """``(score, T, tau)`` checked: the score's name, ``T`` positive and finite (returned as its float32 value) and a threshold that is not
    NaN (as its float32 value; None stays None)."""
    if score not in SCORES:
        raise ValueError(f"--score must be one of {SCORES}, not {score!r}")
    T = float(temperature)
    if not (T > 0.0 and math.isfinite(T)):
        raise ValueError(f"--temperature must be positive and finite, not {temperature}")
    T = float(torch.tensor(T, dtype=torch.float32))
    if not (T > 0.0 and math.isfinite(T)):
        raise ValueError(f"--temperature must be positive and finite in float32, not {temperature}")
    if threshold is not None:
        if math.isnan(float(threshold)):
            raise ValueError("the threshold is NaN: no row could be compared with it")
        threshold = float(torch.tensor(float(threshold), dtype=torch.float32))
    return score, T, threshold


def check_files(export_small, export_large, data_classes=None):
    """Refuses two compact files that cannot share patch rows (``img_size``, ``patch_size``, ``in_chans``) and a ``data_classes`` above
    either head's width; returns ``data_classes`` (default: the narrower head)."""
    cs, cl = export_small["cfg"], export_large["cfg"]
    for key in ("img_size", "patch_size", "in_chans"):
        if cs[key] != cl[key]:
            raise ValueError(f"the files differ in {key}: --small has {cs[key]}, --large has {cl[key]} (the patch rows are shared)")
    width = min(cs["num_classes"], cl["num_classes"])
    C = width if data_classes is None else int(data_classes)
    if not 1 <= C <= width:
        raise ValueError(f"data_classes {C} is not within the heads' widths: --small has {cs['num_classes']}, --large has {cl['num_classes']}")
    return C


# ---- written specs --------------------------------------------------------------------------------------------------------------------
def reference_scores(z, C, T=1.0, kind="msp"):
    """float64 [n]: the score ``kind`` of ``softmax(z[:, :C] / T)`` per row of the logits as given (float32 read as float64).  A row with a
    NaN in a valid column (and a row whose softmax is undefined) is NaN."""
    if kind not in SCORES:
        raise ValueError(f"kind must be one of {SCORES}, not {kind!r}")
    C = int(C)
    z = torch.as_tensor(z).detach().cpu()[:, :C].double()
    n = z.shape[0]
    q = z / float(T)
    bad = torch.isnan(q).any(dim=1) | torch.isinf(q.max(dim=1)[0])
    q = torch.where(bad[:, None], torch.zeros_like(q), q)
    lp = torch.log_softmax(q, dim=1)
    p = lp.exp()
    if kind == "msp":
        s = p.max(dim=1)[0]
    elif kind == "margin":
        top = torch.topk(p, min(2, C), dim=1)[0]
        s = top[:, 0] - top[:, 1] if C > 1 else top[:, 0]
    else:
        s = 1.0 + torch.where(p > 0, p * lp, torch.zeros_like(p)).sum(dim=1) / math.log(C) if C > 1 else torch.ones(n, dtype=torch.float64)
    return torch.where(bad, torch.full_like(s, math.nan), s)


def reference_top1(z, C):
    """int64 [n]: the first maximum of columns [0, C); -1 for a row with a NaN there or without a maximum (every column -inf)."""
    z = torch.as_tensor(z).detach().cpu()[:, :int(C)].double()
    bad = torch.isnan(z).any(dim=1) | (z.max(dim=1)[0] == -INF)
    t = torch.where(bad[:, None], torch.zeros_like(z), z).argmax(dim=1)              # torch's argmax: the first maximum
    return torch.where(bad, torch.full_like(t, -1), t)


def reference_scorer(z, C, T, kind):
    """``scorer`` for the bank commands without a device: ``(reference_scores rounded to float32 once, reference_top1)``."""
    return reference_scores(z, C, T, kind).float(), reference_top1(z, C)


def device_scorer(dev=None):
    """``scorer(z, C, T, kind)`` on the device: ``ops.cascade_decide`` with ``tau = -inf`` -- the kernel ``run`` uses, hence its score bits."""
    from . import ops
    dev = TL.device(dev)

    def scorer(z, C, T, kind):
        with torch.cuda.device(dev):
            s, t, _ = ops.cascade_decide(torch.as_tensor(z).to(dev, torch.float32), int(C), T, kind, -INF, defer=False)
            return s, t.to(torch.int64)
    return scorer


@torch.no_grad()
def reference_cascade(export_small, export_large, x, *, score="msp", temperature=1.0, threshold, num_labels=None):
    """``(logits float64 [B, C], source int64 [B], score float64 [B])`` of the cascade in float64 PyTorch on the files' float32 master
    weights (``compact.reference_logits``): the large model's rows where ``!(score >= threshold)``, the small model's elsewhere."""
    score, T, tau = check_rule(score, temperature, threshold)
    C = check_files(export_small, export_large, num_labels)
    x = torch.as_tensor(x).detach().cpu().double()
    zs, zl = (CP.reference_forward(ex, x)[:, :C] for ex in (export_small, export_large))
    s = reference_scores(zs, C, T, score)
    source = (~(s.float() >= tau)).to(torch.int64)                                    # (the comparison is float32's)
    return torch.where(source[:, None] > 0, zl, zs), source, s


# ---- the sweep ------------------------------------------------------------------------------------------------------------------------
def sweep(score, top1_small, top1_large, labels, C, macs_small, macs_large):
    """The full curve from the float32 ``score`` [n] (no NaN), both models' top-1 columns and the labels, on the device ``score`` is on: a
    stable descending sort and int64 prefix sums.  Point 0 keeps nothing (``tau = +inf``); point k keeps the rows whose score is at least the
    k-th largest DISTINCT value, which is its threshold; the last point keeps everything and its threshold is written ``-inf``.  Returns
    CPU tensors ``{"kept" int64, "threshold" float32, "correct" int64, "defer_rate", "accuracy", "macs" float64}`` and the counts
    ``(n, counted, correct_small, correct_large, correct_either)``."""
    dev = score.device
    y = labels.to(dev, torch.int64)
    ts, tl = top1_small.to(dev, torch.int64), top1_large.to(dev, torch.int64)
    n = int(y.shape[0])
    counted = (y >= 0) & (y < int(C))
    ok_s, ok_l = (counted & (ts == y)).to(torch.int64), (counted & (tl == y)).to(torch.int64)
    order = torch.sort(score, descending=True, stable=True)[1]
    sv = score[order]
    last = torch.ones(n, dtype=torch.bool, device=dev)                                    # the last row of every run of equal scores
    last[:-1] = sv[:-1] != sv[1:]
    kept = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.nonzero(last)[:, 0] + 1])
    cs = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(ok_s[order], 0)])
    cl = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(ok_l[order], 0)])
    total_l = int(ok_l.sum())
    correct = cs[kept] + (total_l - cl[kept])
    thr = torch.cat([torch.full((1,), INF, dtype=torch.float32, device=dev), sv[kept[1:] - 1].float()])
    thr[-1] = -INF
    m = int(counted.sum())
    kept, thr, correct = kept.cpu(), thr.cpu(), correct.cpu()
    rate = (n - kept).double() / n
    out = dict(kept=kept, threshold=thr, correct=correct, defer_rate=rate, accuracy=correct.double() / max(m, 1),
               macs=float(macs_small) + rate * float(macs_large))
    return out, (n, m, int(ok_s.sum()), total_l, int((ok_s | ok_l).sum()))


def _point(full, j):
    return dict(defer_rate=float(full["defer_rate"][j]), threshold=float(full["threshold"][j]), accuracy=float(full["accuracy"][j]),
                macs=float(full["macs"][j]))


def choose(full, large_top1, match_large=None, target_accuracy=None, max_macs=None):
    """The index of the operating point among the full curve's points (cost falls with the index), or None without a selector:
    ``match_large`` EPS -- the cheapest with ``accuracy >= large_top1 - EPS``; ``target_accuracy`` A -- the cheapest with ``accuracy >= A``;
    ``max_macs`` M -- the most accurate with cost ``<= M``, the cheaper among equals.  A target that cannot be met is refused, naming the
    best value reachable."""
    given = [k for k, v in (("--match_large", match_large), ("--target_accuracy", target_accuracy), ("--max_macs", max_macs)) if v is not None]
    if len(given) > 1:
        raise ValueError(f"{' and '.join(given)}: one selector at a time")
    if not given:
        return None
    acc, macs = full["accuracy"], full["macs"]
    if max_macs is not None:
        ok = torch.nonzero(macs <= float(max_macs))[:, 0]
        if not ok.numel():
            raise ValueError(f"--max_macs {max_macs} cannot be met: the cheapest cost reachable is {float(macs.min())} (the small model always runs)")
        best = float(acc[ok].max())
        return int(ok[acc[ok] == best].max())                                           # (the largest index: the cheapest)
    want = float(large_top1) - float(match_large) if match_large is not None else float(target_accuracy)
    ok = torch.nonzero(acc >= want)[:, 0]
    if not ok.numel():
        raise ValueError(f"{given[0]} {match_large if match_large is not None else target_accuracy} cannot be met: the best accuracy reachable is "
                         f"{float(acc.max())}" + (f" (the target is {want})" if match_large is not None else ""))
    return int(ok.max())


def cascade_curve(bank_small, bank_large, *, macs_small, macs_large, score="msp", temperature=1.0, match_large=None, target_accuracy=None,
                  max_macs=None, points=101, scorer=None, dev=None):
    """``(record, output)``: the JSON record of ``curve`` (module docstring) and the dict ``--output`` saves -- the full curve's
    ``POINT_KEYS`` vectors and per row ``score`` float32, ``top1_small``, ``top1_large`` int64 and ``defer_at_chosen`` bool (absent without a
    selector).  ``scorer``: None scores on the device, ``reference_scorer`` on the CPU."""
    score, T, _ = check_rule(score, temperature)
    C = CC.check_pair(bank_small, bank_large, 1, "the small bank", "the large bank")
    points = int(points)
    if points < 2:
        raise ValueError(f"--points must be at least 2, not {points}")
    for name, v in (("macs_small", macs_small), ("macs_large", macs_large)):
        if not (float(v) > 0.0 and math.isfinite(float(v))):
            raise ValueError(f"{name} must be positive and finite, not {v}")
    if scorer is None:
        scorer = device_scorer(dev)
    labels = bank_small["labels"].to(torch.int64)
    s, ts = scorer(bank_small["logits"].float(), C, T, score)
    tl = scorer(bank_large["logits"].float(), C, T, score)[1]
    bad = torch.nonzero(torch.isnan(s))
    if bad.numel():
        raise ValueError(f"row {int(bad[0, 0])} of the small bank has no score: a NaN logit in its first {C} columns ({bad.shape[0]} such rows)")
    full, (n, m, right_s, right_l, right_any) = sweep(s, ts, tl, labels, C, macs_small, macs_large)
    if m == 0:
        raise ValueError(f"no row of the banks has a label in [0, {C}): there is no accuracy to sweep")
    K = full["kept"].shape[0]
    rate, acc = full["defer_rate"], full["accuracy"]
    asc = torch.arange(K - 1, -1, -1)                                                    # the points by ascending defer rate
    grid = torch.arange(points, dtype=torch.float64) / (points - 1)
    at = asc[torch.searchsorted(rate[asc].contiguous(), grid).clamp_max(K - 1)]          # the first point at or above every rate
    best_acc = float(acc.max())
    best = int(torch.nonzero(acc == best_acc)[:, 0].max())
    chosen = choose(full, right_l / m, match_large, target_accuracy, max_macs)
    rec = dict(images=n, counted=m, data_classes=C, score=score, temperature=T, thresholds=K,
               small=dict(top1=right_s / m, macs=float(macs_small)), large=dict(top1=right_l / m, macs=float(macs_large)), oracle=right_any / m,
               curve=[_point(full, int(j)) for j in at.tolist()], best=_point(full, best),
               area=float(torch.trapezoid(acc[asc], rate[asc])), chosen=None if chosen is None else _point(full, chosen))
    s_host = s.detach().float().cpu()
    out = dict({k: full[k] for k in POINT_KEYS}, score=s_host, top1_small=ts.cpu().to(torch.int64), top1_large=tl.cpu().to(torch.int64))
    if chosen is not None:
        out["defer_at_chosen"] = ~(s_host >= full["threshold"][chosen])
    return rec, out


def reference_curve(bank_small, bank_large, **kw):
    """``cascade_curve`` with the float64 scores of ``reference_scores`` (rounded to float32 once, as thresholds are float32), on the CPU."""
    return cascade_curve(bank_small, bank_large, scorer=reference_scorer, **kw)


def make_policy(rec, *, img_size=None, patch_size=None):
    """The policy dict of a ``curve`` record that has a chosen point (``POLICY_KEYS``)."""
    if rec.get("chosen") is None:
        raise ValueError("--policy needs an operating point: give --match_large, --target_accuracy or --max_macs")
    c = rec["chosen"]
    return dict(score=rec["score"], temperature=rec["temperature"], threshold=c["threshold"], data_classes=rec["data_classes"], img_size=img_size,
                patch_size=patch_size, macs_small=rec["small"]["macs"], macs_large=rec["large"]["macs"],
                expected=dict(accuracy=c["accuracy"], defer_rate=c["defer_rate"], macs=c["macs"]))


def load_policy(path_or_dict):
    pol = path_or_dict
    if not isinstance(pol, dict):
        with open(pol, "r", encoding="utf-8") as f:
            pol = json.load(f)
    missing = [k for k in POLICY_KEYS if not isinstance(pol, dict) or k not in pol]
    if missing:
        raise ValueError(f"not a cascade policy: it lacks {', '.join(missing)} (compact_cascade curve --policy writes them)")
    return pol


def rule_of(args):
    """``{"score", "temperature", "threshold", "data_classes", "policy"}`` of a parsed ``run`` / ``predict`` command line: the policy file's
    rule, or the flags' (``data_classes`` and ``policy`` None); checked by ``check_rule``."""
    policy = getattr(args, "policy", None)
    if policy is not None:
        if getattr(args, "threshold", None) is not None:
            raise ValueError("--policy and --threshold: one of the two")
        pol = load_policy(policy)
        score, T, tau = check_rule(pol["score"], pol["temperature"], pol["threshold"])
        return dict(score=score, temperature=T, threshold=tau, data_classes=int(pol["data_classes"]), policy=pol)
    if getattr(args, "threshold", None) is None:
        raise ValueError("need --policy or --threshold")
    score, T, tau = check_rule(args.score, args.temperature, args.threshold)
    return dict(score=score, temperature=T, threshold=tau, data_classes=None, policy=None)


def check_policy_files(rule, export_small, export_large):
    """A policy made for another geometry is refused by name."""
    pol = rule["policy"]
    if pol is None:
        return
    for key in ("img_size", "patch_size"):
        if pol.get(key) is not None and int(pol[key]) != export_small["cfg"][key]:
            raise ValueError(f"the policy was made at {key} {pol[key]}, the files have {export_small['cfg'][key]}")


# ---- on the device --------------------------------------------------------------------------------------------------------------------
class Cascade:
    """The device cascade of two compact files (exports or paths): ``forward`` returns ``(logits float32 [B, C], source int32 [B] -- 1 where
    the large model answered --, score float32 [B])``.  ``small`` / ``large`` are the ``CompactVisionTransformer`` modules; ``deferred`` is
    the last call's count and ``last_idx`` its deferred rows (int32, on the device)."""

    def __init__(self, small, large, *, score="msp", temperature=1.0, threshold, precision="bf16", device=None):
        ex_s, ex_l = CP.as_export(small), CP.as_export(large)
        self.score, self.temperature, self.threshold = check_rule(score, temperature, threshold)
        self.width = check_files(ex_s, ex_l)
        dev = TL.device(device)
        self.device, self.precision = dev, precision
        self.small = CP.CompactVisionTransformer(ex_s, precision=precision, device=dev)
        self.large = CP.CompactVisionTransformer(ex_l, precision=precision, device=dev)
        c = ex_s["cfg"]
        self.cfg = c
        self.patches_per_image = (c["img_size"] // c["patch_size"]) ** 2
        self.row_width = c["in_chans"] * c["patch_size"] ** 2
        self.deferred, self.last_idx = 0, None

    def macs(self, defer_rate):
        return self.small.macs(1) + float(defer_rate) * self.large.macs(1)

    def patch_rows(self, x):
        """The batch's patch rows [B * np, C * P * P] in the models' dtype (``ops.patchify``)."""
        from . import _lib as L
        from . import ops
        L.require_cuda(x)
        c = self.cfg
        if x.dim() != 4 or tuple(x.shape[1:]) != (c["in_chans"], c["img_size"], c["img_size"]):
            raise AssertionError(f"Input image size {tuple(x.shape[1:])} doesn't match the models ({c['in_chans']}, {c['img_size']}, {c['img_size']}).")
        x = x.contiguous().float()
        dtype = ops.UVC_F32 if self.precision == "fp32" else ops.UVC_BF16
        rows = torch.empty(x.shape[0] * self.patches_per_image, self.row_width, dtype=ops.tdtype(dtype), device=x.device)
        ops.patchify(x, rows, c["patch_size"], dtype)
        return rows

    @torch.no_grad()
    def forward(self, x=None, *, patches=None, num_labels=None):
        from . import ops
        if (x is None) == (patches is None):
            raise ValueError("pass one of x / patches")
        C = CP.num_labels(dict(num_classes=self.width), num_labels)
        with torch.cuda.device(self.device):
            rows = self.patch_rows(x) if patches is None else patches
            zs = self.small(patches=rows)[0]
            score, _, defer = ops.cascade_decide(zs, C, self.temperature, self.score, self.threshold, top1=False)
            idx, pos, count = ops.cascade_compact(defer)
            m = int(count.item())                                                    # the one synchronisation: 4 bytes
            zl = None
            if m:
                zl = self.large(patches=ops.cascade_gather(rows, idx, m, self.patches_per_image))[0]
            out, source = ops.cascade_merge(zs, zl, pos, C)
        self.deferred, self.last_idx = m, idx[:m]
        return out, source, score

    __call__ = forward


def evaluate(cascade, loader, data_classes=None):
    """Walks ``loader`` once through ``cascade``: yields per batch ``{"logits", "source", "score", "labels"}`` (on the device, the eval
    loader's order)."""
    for x, y in loader:
        logits, source, score = cascade.forward(x, num_labels=data_classes)
        yield dict(logits=logits, source=source, score=score, labels=y.to(torch.int64))


def predict(cascade, files, *, topk=5, batch_size=64, preset="imagenet", interpolation="bilinear", crop_pct=None, num_labels=None, classes=None,
            num_workers=8):
    """``compact.predict``'s records from the cascade, each with ``"model": "small" | "large"`` and ``"score"``: one per file in input order,
    ``{"file", "error"}`` for a file that cannot be read.  The loader writes the patch rows both models read."""
    from . import data, ops
    if preset not in CP.PRESETS:
        raise ValueError(f"preset must be one of {CP.PRESETS}, not {preset!r}")
    c = cascade.cfg
    classes = None if classes is None else list(classes)
    if num_labels is None:
        num_labels = len(classes) if classes is not None else cascade.width
    num_labels, topk = CP.num_labels(dict(num_classes=cascade.width), num_labels), int(topk)
    if classes is not None and len(classes) < num_labels:
        raise ValueError(f"{len(classes)} class names for {num_labels} labels")
    if not 1 <= topk <= min(CP.MAX_TOPK, num_labels):
        raise ValueError(f"topk {topk} must lie in [1, {min(CP.MAX_TOPK, num_labels)}]")
    ds = files if hasattr(files, "load") else data.FileListDataset(files, tolerant=True)
    names = ds.paths if hasattr(ds, "paths") else list(range(len(ds)))
    errors = getattr(ds, "errors", {})
    kw = dict(mean=data.IMAGENET_MEAN, std=data.IMAGENET_STD, eval="center") if preset == "imagenet" else \
        dict(mean=data.CIFAR_MEAN, std=data.CIFAR_STD, eval="square")
    loader = data.DeviceLoader(ds, int(batch_size), c["img_size"], train=False, num_workers=num_workers, device=cascade.device,
                               interpolation=interpolation, crop_pct=crop_pct, output="patches", patch_size=c["patch_size"],
                               dtype=torch.float32 if cascade.precision == "fp32" else torch.bfloat16, **kw)
    first = 0
    with torch.cuda.device(cascade.device):
        for x, _ in loader:
            logits, source, score = cascade.forward(patches=x, num_labels=num_labels)
            probs, index = ops.logits_topk(logits, topk, num_labels)
            rows = zip(probs.cpu().tolist(), index.cpu().tolist(), source.cpu().tolist(), score.cpu().tolist())
            for b, (pr, ix, src, sc) in enumerate(rows):
                i = first + b
                if i in errors:
                    yield dict(file=names[i], error=errors[i])
                    continue
                yield dict(file=names[i], top=[dict(index=j, label=None if classes is None else classes[j], prob=q) for j, q in zip(ix, pr)],
                           model="large" if src else "small", score=sc)
            first += len(probs)


# ---- the commands ---------------------------------------------------------------------------------------------------------------------
def _load(b):
    return b if isinstance(b, dict) else torch.load(b, map_location="cpu")


def curve_command(args, scorer=None, dev=None):
    """``curve``: the record.  ``scorer``: None scores on the device; ``reference_scorer`` runs the same command on the CPU."""
    check_rule(args.score, args.temperature)
    small, large = getattr(args, "small", None), getattr(args, "large", None)
    geometry = {}
    if small is not None or large is not None:
        if small is None or large is None:
            raise ValueError("--small and --large go together")
        if args.macs_small is not None or args.macs_large is not None:
            raise ValueError("--macs_small / --macs_large stand in for --small / --large: give the files or the numbers")
        ex_s, ex_l = CP.as_export(small), CP.as_export(large)
        check_files(ex_s, ex_l)
        macs_small, macs_large = CP.compact_macs(ex_s, 1, padded=True), CP.compact_macs(ex_l, 1, padded=True)
        geometry = dict(img_size=ex_s["cfg"]["img_size"], patch_size=ex_s["cfg"]["patch_size"])
    elif args.macs_small is None or args.macs_large is None:
        raise ValueError("need --small and --large, or --macs_small and --macs_large")
    else:
        macs_small, macs_large = args.macs_small, args.macs_large
    bank_small, bank_large = _load(args.bank_small), _load(args.bank_large)
    if geometry:
        check_files(ex_s, ex_l, CC.check_pair(bank_small, bank_large, 1, "the small bank", "the large bank"))
    elif isinstance(bank_small, dict) and isinstance(bank_small.get("meta"), dict):
        geometry = dict(img_size=bank_small["meta"].get("img_size"))
    t0 = time.perf_counter()
    rec, out = cascade_curve(bank_small, bank_large, macs_small=macs_small, macs_large=macs_large, score=args.score, temperature=args.temperature,
                             match_large=args.match_large, target_accuracy=args.target_accuracy, max_macs=args.max_macs, points=args.points,
                             scorer=scorer, dev=dev)
    if scorer is None:
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if getattr(args, "policy", None):
        pol = make_policy(rec, **geometry)
        with open(args.policy, "w", encoding="utf-8") as f:
            json.dump(pol, f)
    if getattr(args, "output", None):
        torch.save(out, args.output)
    rec["rows_per_s"] = rec["images"] / dt if dt > 0 else 0.0
    return rec


def _files_and_rule(args):
    """What ``run`` and ``predict`` check before any image is read: ``(export_small, export_large, rule, data_classes or None)``."""
    rule = rule_of(args)
    ex_s, ex_l = CP.as_export(args.small), CP.as_export(args.large)
    C = check_files(ex_s, ex_l, rule["data_classes"])
    check_policy_files(rule, ex_s, ex_l)
    return ex_s, ex_l, rule, (C if rule["data_classes"] is not None else None)


def run_command(args, dev=None):
    """``run``: ``(record, bank)``.  ONE eval loader, ONE walk over ``args.split``, the device cascade per batch; the bank (saved to
    ``args.bank`` when given) is a logits bank of the FINAL logits [n, C] with ``source`` int32 and ``score`` float32 per row."""
    ex_s, ex_l, rule, C = _files_and_rule(args)
    dev = TL.device(dev)
    cascade = Cascade(ex_s, ex_l, score=rule["score"], temperature=rule["temperature"], threshold=rule["threshold"], precision=args.precision, device=dev)
    loader, classes = TL.eval_loader(ex_s, args, args.split)
    if C is not None and C != classes:
        raise ValueError(f"the policy was made for data_classes {C}, the dataset has {classes}")
    C = check_files(ex_s, ex_l, classes)
    with torch.cuda.device(dev):
        t0 = time.perf_counter()
        outs = list(evaluate(cascade, loader, C))
        if not outs:
            raise ValueError(f"the {args.split} split of {args.dataset} is empty")
        logits, source, score, labels = (torch.cat([o[k] for o in outs]) for k in ("logits", "source", "score", "labels"))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        pred = logits[:, :C].argmax(dim=1)
    counted = (labels >= 0) & (labels < C)
    right = counted & (pred == labels)
    deferred = source != 0
    n, m = int(labels.shape[0]), int(counted.sum())
    share = lambda num, den: int(num.sum()) / int(den.sum()) if int(den.sum()) else None
    rate = int(deferred.sum()) / n
    rec = dict(images=n, counted=m, data_classes=C, score=rule["score"], temperature=rule["temperature"], threshold=rule["threshold"],
               top1=share(right, counted), deferred=int(deferred.sum()), defer_rate=rate, macs_per_image=cascade.macs(rate),
               small_top1_on_kept=share(right & ~deferred, counted & ~deferred), large_top1_on_deferred=share(right & deferred, counted & deferred),
               img_per_s=n / dt if dt > 0 else 0.0)
    if rule["policy"] is not None:
        rec["expected"] = rule["policy"]["expected"]
    bank = TL.make_bank(labels, C, logits=logits, img_size=ex_s["cfg"]["img_size"], dataset=args.dataset, split=args.split,
                        interpolation=args.interpolation, crop_pct=args.crop_pct, precision=args.precision)
    bank.update(source=source.cpu(), score=score.cpu())
    if getattr(args, "bank", None):
        torch.save(bank, args.bank)
    return rec, bank


def predict_command(args, dev=None):
    """``predict``: one JSON line per image to --output (or stdout), then ``compact predict``'s summary line with ``deferred``."""
    from . import data
    ex_s, ex_l, rule, C = _files_and_rule(args)
    classes = CP.read_classes(args.classes) if args.classes else None
    num_labels = args.num_labels if args.num_labels is not None else (C if classes is None else None)
    if num_labels is not None:
        check_files(ex_s, ex_l, num_labels)
    files = data.list_images(args.images)
    cascade = Cascade(ex_s, ex_l, score=rule["score"], temperature=rule["temperature"], threshold=rule["threshold"], precision=args.precision,
                      device=TL.device(dev))
    records = predict(cascade, files, topk=args.topk, batch_size=args.batch_size, preset=args.preset, interpolation=args.interpolation,
                      crop_pct=args.crop_pct, num_labels=num_labels, classes=classes, num_workers=args.num_workers)
    import sys
    out = open(args.output, "w", encoding="utf-8") if args.output else sys.stdout
    n = nerr = deferred = 0
    t0 = time.perf_counter()
    try:
        for rec in records:
            out.write(json.dumps(rec) + "\n")
            n += 1
            nerr += "error" in rec
            deferred += rec.get("model") == "large"
        dt = time.perf_counter() - t0
        summary = dict(images=n, errors=nerr, batches=math.ceil(n / args.batch_size), img_per_s=n / dt if dt > 0 else 0.0, deferred=deferred)
        out.write(json.dumps(summary) + "\n")
    finally:
        if out is not sys.stdout:
            out.close()
    return summary


def _float_arg(what):
    def parse(v):
        f = float(v)
        if math.isnan(f):
            raise argparse.ArgumentTypeError(f"{what} is NaN")
        return f
    return parse


def _add_rule_flags(p, threshold):
    p.add_argument("--score", choices=list(SCORES), default="msp", help="the small model's confidence: higher is surer")
    p.add_argument("--temperature", type=float, default=1.0, help="T > 0 of softmax(z / T): compact_calibrate fit's value")
    if threshold:
        p.add_argument("--policy", default=None, help="the file curve --policy wrote: score, temperature and threshold come from it")
        p.add_argument("--threshold", type=float, default=None, help="tau: the small model's answer stands iff score >= tau (the two ends: --threshold=inf and --threshold=-inf)")


def build_parser():
    p = argparse.ArgumentParser(prog="python -m uvc_amd.compact_cascade", description="A small compact model that defers to a large one")
    sub = p.add_subparsers(dest="cmd", required=True)
    c = sub.add_parser("curve")
    c.add_argument("--bank_small", required=True, help="a logits bank of the small model (compact_calibrate logits, compact_ood bank, compact_compare run)")
    c.add_argument("--bank_large", required=True, help="a bank of the large model on the same split in the same order")
    c.add_argument("--small", default=None, help="the small compact file: its MACs and geometry")
    c.add_argument("--large", default=None, help="the large compact file")
    c.add_argument("--macs_small", type=_float_arg("--macs_small"), default=None, help="MACs per image of the small model, in place of --small")
    c.add_argument("--macs_large", type=_float_arg("--macs_large"), default=None, help="MACs per image of the large model, in place of --large")
    _add_rule_flags(c, threshold=False)
    g = c.add_mutually_exclusive_group()
    g.add_argument("--match_large", type=_float_arg("--match_large"), default=None, help="EPS: the cheapest threshold with accuracy >= the large model's - EPS")
    g.add_argument("--target_accuracy", type=_float_arg("--target_accuracy"), default=None, help="A: the cheapest threshold with accuracy >= A")
    g.add_argument("--max_macs", type=_float_arg("--max_macs"), default=None, help="M: the most accurate threshold with MACs per image <= M")
    c.add_argument("--points", type=CP._int_in(2, 1 << 20, "--points"), default=101, help="evenly spaced defer rates the record's curve is read at")
    c.add_argument("--policy", default=None, help="write the chosen operating point as a JSON policy for run / predict")
    c.add_argument("--output", default=None, help="the full curve and the per-row score, top-1 columns and defer_at_chosen")
    r = sub.add_parser("run")
    r.add_argument("--small", required=True, help="the small compact file: it sees every image")
    r.add_argument("--large", required=True, help="the large compact file: it sees the deferred images")
    _add_rule_flags(r, threshold=True)
    TL.add_dataset_flags(r, split_default="test")
    r.add_argument("--bank", default=None, help="where to save the final logits, source and score of every row")
    q = sub.add_parser("predict")
    q.add_argument("--small", required=True, help="the small compact file")
    q.add_argument("--large", required=True, help="the large compact file")
    _add_rule_flags(q, threshold=True)
    CP.add_image_file_flags(q)
    return p


def main(argv: Optional[Sequence[str]] = None, scorer=None):
    args = build_parser().parse_args(argv)
    if args.cmd == "curve":
        rec = curve_command(args, scorer)
    elif args.cmd == "run":
        TL.need_data(args)
        rec = run_command(args)[0]
    else:
        return predict_command(args)
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main()
