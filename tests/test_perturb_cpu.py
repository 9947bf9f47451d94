"""CPU: the perturbation test of relevance maps (uvc_amd/compact_perturb.py) -- the parser, ``step_counts`` and ``auc`` against hand values, the
host statement of the rank rule, ``reference_perturbation`` on micro exports, and the condition the GPU test puts on its fixtures.  No GPU."""
import argparse
import math

import numpy as np
import pytest
import torch

import perturb_ref as PR
from uvc_amd import compact as CP
from uvc_amd import compact_perturb as PT


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def test_parser_flags_and_defaults():
    p = PT.build_parser()
    flags = {a.dest: a for a in p._actions if a.dest != "help"}
    assert set(flags) == {"compact", "images", "methods", "orders", "steps", "target", "seed", "output", "batch_size", "num_workers", "precision",
                          "preset", "interpolation", "crop_pct", "num_labels"}
    assert not any(isinstance(a, argparse._SubParsersAction) for a in p._actions)
    a = p.parse_args(["--compact", "m", "--images", "a.png", "d"])
    assert (a.compact, a.images, a.methods, a.orders, a.steps, a.target, a.seed, a.output) == ("m", ["a.png", "d"], ["rollout"],
                                                                                              ["positive", "negative"], 10, None, 0, None)
    assert (a.batch_size, a.num_workers, a.precision, a.preset, a.interpolation, a.crop_pct, a.num_labels) == (64, 8, "bf16", "imagenet", "bilinear",
                                                                                                           None, None)
    assert tuple(flags["methods"].choices) == ("rollout", "last", "attribution", "random") == PT.PERTURB_METHODS
    assert tuple(flags["orders"].choices) == ("positive", "negative") == PT.ORDERS
    b = p.parse_args(["--compact", "m", "--images", "a", "--methods", "last", "attribution", "random", "--orders", "negative", "--steps", "7",
                      "--target", "3", "--seed", "5", "--output", "curves.jsonl", "--preset", "cifar", "--num_labels", "10", "--crop_pct", "0.9"])
    assert (b.methods, b.orders, b.steps, b.target, b.seed, b.output) == (["last", "attribution", "random"], ["negative"], 7, 3, 5, "curves.jsonl")
    assert (b.preset, b.num_labels, b.crop_pct) == ("cifar", 10, 0.9)
    # the existing commands are as they were: nothing of this feature is a subcommand or a flag of uvc_amd.compact
    sub = [a for a in CP._parser()._actions if isinstance(a, argparse._SubParsersAction)][0]
    assert "perturb" not in sub.choices and CP.METHODS == ("rollout", "last") and CP.GRAD_METHODS == ("attribution",)


@pytest.mark.parametrize("argv", [["--compact", "m"], ["--images", "a"], ["--compact", "m", "--images"],
                                  ["--compact", "m", "--images", "a", "--methods", "gradcam"], ["--compact", "m", "--images", "a", "--methods"],
                                  ["--compact", "m", "--images", "a", "--orders", "both"], ["--compact", "m", "--images", "a", "--steps", "0"],
                                  ["--compact", "m", "--images", "a", "--steps", "1025"], ["--compact", "m", "--images", "a", "--target", "-1"],
                                  ["--compact", "m", "--images", "a", "--batch_size", "0"], ["--compact", "m", "--images", "a", "--crop_pct", "1.5"],
                                  ["--compact", "m", "--images", "a", "--topk", "3"]],
                         ids=["no_images", "no_compact", "empty_images", "method", "empty_methods", "order", "steps_0", "steps_1025", "target_-1",
                              "batch_size_0", "crop_pct_1.5", "predict_only_flag"])
def test_parser_refusals(argv, capsys):
    with pytest.raises(SystemExit) as e:
        PT.build_parser().parse_args(argv)
    assert e.value.code == 2
    capsys.readouterr()


def test_evaluate_refuses_before_any_file_is_read():
    ex, _ = PR.export_of("no_heads")
    for kw in (dict(methods=("gradcam",)), dict(methods=()), dict(methods=("rollout", "rollout")), dict(orders=("up",)), dict(steps=0),
               dict(preset="coco"), dict(num_labels=0), dict(num_labels=17), dict(target=10, num_labels=10), dict(target=-1)):
        with pytest.raises(ValueError):
            next(PT.evaluate(ex, ["/nonexistent/x.png"], **kw))
    with pytest.raises(ValueError):
        next(PT.evaluate({"format": "other"}, []))


# ---- the grid and the area -----------------------------------------------------------------------------------------------------------------
def test_step_counts_hand_values():
    assert PT.step_counts(196, 10) == [0, 19, 39, 58, 78, 98, 117, 137, 156, 176]
    assert PT.step_counts(196) == PT.step_counts(196, 10)
    assert PT.step_counts(16, 7) == [0, 2, 4, 6, 9, 11, 13]
    assert PT.step_counts(4, 10) == [0, 0, 0, 1, 1, 2, 2, 2, 3, 3]
    assert PT.step_counts(1, 1) == [0] and PT.step_counts(576, 4) == [0, 144, 288, 432]
    for np_, steps in ((196, 10), (16, 7), (1, 3), (1024, 1024)):
        c = PT.step_counts(np_, steps)
        assert len(c) == steps and c[0] == 0 and c[-1] < np_ and c == sorted(c) and all(isinstance(v, int) for v in c)
    for bad in ((0, 10), (196, 0), (-1, 3)):
        with pytest.raises(ValueError):
            PT.step_counts(*bad)


def test_auc_hand_values():
    assert PT.auc([1.0] * 10, 10) == pytest.approx(0.9, abs=1e-15)                    # nine trapezoids of width 1 / 10
    assert PT.auc([1.0, 0.0], 2) == 0.25 and PT.auc([0.0, 1.0], 2) == 0.25
    assert PT.auc([1.0, 0.5, 0.0, 0.0], 4) == pytest.approx((0.75 + 0.25 + 0.0) / 4, abs=1e-15)
    assert PT.auc([0.7], 1) == 0.0                                                    # one point spans nothing
    y = [0.9, 0.8, 0.4, 0.3, 0.3, 0.2, 0.1]
    want = sum((y[k] + y[k + 1]) / 2 for k in range(6)) / 7
    assert PT.auc(y, 7) == pytest.approx(want, abs=1e-15) and PT.auc(torch.tensor(y, dtype=torch.float64), 7) == pytest.approx(want, abs=1e-15)
    both = PT.auc(np.array([y, y[::-1]]), 7)
    assert both.shape == (2,) and both[0] == pytest.approx(want, abs=1e-15) and both[1] == pytest.approx(want, abs=1e-15)
    assert isinstance(PT.auc(y, 7), float)
    with pytest.raises(ValueError):
        PT.auc([], 3)


# ---- the rank rule -------------------------------------------------------------------------------------------------------------------------
def by_definition(row, descending):
    """rank[p] = #{j : j before p}, the rule as the header states it, one pair at a time"""
    n = len(row)
    nan = [math.isnan(v) for v in row]

    def before(j, p):
        if nan[j] or nan[p]:
            return (not nan[j] and nan[p]) or (nan[j] and nan[p] and j < p)
        if row[j] == row[p]:                                  # (-0.0 == 0.0)
            return j < p
        return row[j] > row[p] if descending else row[j] < row[p]
    return [sum(before(j, p) for j in range(n) if j != p) for p in range(n)]


def test_rank_rule_on_ties_signed_zeros_and_nan():
    inf, nan = float("inf"), float("nan")
    s = [[0.5, 0.5, 0.25, 0.5, 1.0, 0.25],
         [0.0, -0.0, 1.0, -0.0, 0.0, -1.0],
         [nan, 1.0, inf, nan, -inf, 1.0],
         [nan, nan, nan, nan, nan, nan],
         [1e-45, 0.0, -1e-45, -0.0, 3e38, -3e38]]
    for descending in (True, False):
        got = PT.rank_reference(torch.tensor(s), descending)
        assert got.dtype == np.int32
        for row, r in zip(s, got.tolist()):
            assert r == by_definition(row, descending), (row, descending)
            assert sorted(r) == list(range(len(row)))
    assert PT.rank_reference(torch.tensor(s), True)[0].tolist() == [1, 2, 4, 3, 0, 5]
    assert PT.rank_reference(torch.tensor(s), False)[0].tolist() == [2, 3, 0, 4, 5, 1]
    assert PT.rank_reference(torch.tensor(s), True)[1].tolist() == [1, 2, 0, 3, 4, 5]           # the zeros tie whatever their sign
    assert PT.rank_reference(torch.tensor(s), True)[2].tolist() == [4, 1, 0, 5, 3, 2]           # NaN after -inf
    assert PT.rank_reference(torch.tensor(s), False)[2].tolist() == [4, 1, 3, 5, 0, 2]          # and after +inf
    assert PT.rank_reference(torch.tensor(s), False)[3].tolist() == [0, 1, 2, 3, 4, 5]
    g = torch.Generator().manual_seed(0)
    for descending in (True, False):
        few = torch.randint(0, 3, (2, 65), generator=g).float()
        assert PT.rank_reference(few, descending).tolist() == [by_definition(r, descending) for r in few.tolist()]


# ---- the spec ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stage2_micro_deit", "no_heads", "hard_gating", "stage2_micro_none"])
def test_reference_perturbation_on_a_micro_export(name):
    ex, x = PR.export_of(name)
    x = x.double()
    cfg = ex["cfg"]
    nl = PR.num_labels_of(name)
    npatch = (cfg["img_size"] // cfg["patch_size"]) ** 2
    maps, target = PR.maps_of(name, "attribution")
    pos = PT.reference_perturbation(ex, x, maps, target, order="positive", num_labels=nl)
    neg = PT.reference_perturbation(ex, x, maps, target, order="negative", num_labels=nl)
    assert pos["counts"] == neg["counts"] == PT.step_counts(npatch, 10) and tuple(pos["prob"].shape) == (x.shape[0], 10)
    # nothing removed: reference_forward's probabilities exactly, in both orders; the target is the top-1 label there
    intact = CP.reference_forward(ex, x)[:, :nl].softmax(dim=1).gather(1, target[:, None])[:, 0]
    assert torch.equal(pos["prob"][:, 0], intact) and torch.equal(neg["prob"][:, 0], intact)
    assert pos["hit"][:, 0].tolist() == [1] * x.shape[0] and bool((pos["margin"][:, 0] > 0).all())
    assert pos["hit"].dtype == torch.int32 and bool(((pos["margin"] > 0) == (pos["hit"] == 1)).all())
    # everything removed: the same input whatever the order
    full_p = PT.reference_perturbation(ex, x, maps, target, order="positive", counts=[npatch], num_labels=nl)
    full_n = PT.reference_perturbation(ex, x, maps, target, order="negative", counts=[npatch], num_labels=nl)
    assert torch.equal(full_p["prob"], full_n["prob"]) and torch.equal(full_p["hit"], full_n["hit"])
    blank = CP.reference_forward(ex, torch.zeros_like(x))[:, :nl].softmax(dim=1).gather(1, target[:, None])
    assert torch.equal(full_p["prob"], blank)
    # one grid point by hand: the removed patches' pixel blocks are zero, the others untouched
    k, P, g = 3, cfg["patch_size"], cfg["img_size"] // cfg["patch_size"]
    ntok = 2 if cfg["enable_dist"] else 1
    rank = torch.from_numpy(PT.rank_reference(maps[:, ntok:], True))
    xk = x.clone()
    for b in range(x.shape[0]):
        for p in range(npatch):
            if rank[b, p] < pos["counts"][k]:
                xk[b, :, (p // g) * P:(p // g + 1) * P, (p % g) * P:(p % g + 1) * P] = 0
    by_hand = CP.reference_forward(ex, xk)[:, :nl].softmax(dim=1).gather(1, target[:, None])[:, 0]
    assert torch.equal(pos["prob"][:, k], by_hand)
    # maps over the patches alone are the same maps; the two orders remove different patches
    assert torch.equal(PT.reference_perturbation(ex, x, maps[:, ntok:], target, order="positive", num_labels=nl)["prob"], pos["prob"])
    assert not torch.equal(pos["prob"][:, 1:], neg["prob"][:, 1:])
    for bad in (dict(order="up"), dict(counts=[npatch + 1]), dict(counts=[-1]), dict(counts=[]), dict(num_labels=0)):
        with pytest.raises(ValueError):
            PT.reference_perturbation(ex, x, maps, target, **{"num_labels": nl, **bad})
    with pytest.raises(ValueError):
        PT.reference_perturbation(ex, x, maps, target + nl, num_labels=nl)
    with pytest.raises(ValueError):
        PT.reference_perturbation(ex, x, maps[:, 3:], target, num_labels=nl)


@pytest.mark.parametrize("name,kind", PR.CASES)
def test_fixtures_leave_the_hit_comparison_enough_pairs(name, kind):
    """The GPU test compares ``hit`` with the reference's only where the reference's margin exceeds twice the float32 logit bar: at least 90 %
    of the (image, step) pairs of every fixture, grid and order must be such pairs.  On the reference alone."""
    for steps in PR.GRIDS:
        for order in PT.ORDERS:
            ref = PR.reference_of(name, kind, order, steps)
            share = float(PR.qualifying(ref, "fp32").double().mean())
            print(f"{name} {kind} {order} steps={steps}: {share:.3f} of the pairs qualify, smallest |margin| / scale "
                  f"{float((ref['margin'].abs() / ref['scale'][None, :]).min()):.3e}")
            assert share >= PR.QUALIFY, (name, kind, order, steps, share)
