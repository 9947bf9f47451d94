"""CPU: the written specs of uvc_amd/compact_compare.py, its parser and refusals, and ``diff`` end to end with the references injected."""
import argparse
import itertools
import json
import math

import numpy as np
import pytest
import torch

import compare_ref as CR
from uvc_amd import _lib as L
from uvc_amd import compact_compare as CC
from uvc_amd import compact_tools as TL
from uvc_amd import ops

LN = math.log


def test_pair_stats_on_four_rows_worked_by_hand():
    """exp of the logits: row 0 a (2, 1, 1) b (1, 1, 1); row 1 both (1, 3, 1); row 2 a (1, 1, 2) b (2, 1, 1); row 3 holds a NaN."""
    za = torch.tensor([[LN(2), 0, 0, 9], [0, LN(3), 0, 9], [0, 0, LN(2), 9], [0, float("nan"), 0, 9]], dtype=torch.float64)
    zb = torch.tensor([[0, 0, 0], [0, LN(3), 0], [LN(2), 0, 0], [1, 2, 3]], dtype=torch.float64)
    y = torch.tensor([0, 2, -1, 1])
    r = CC.reference_pair_stats(za, zb, y, 3)
    assert set(r) == set(CC.STATS)
    nan = float("nan")
    js0 = 0.5 * (0.5 * LN(1.2) + 0.5 * LN(6 / 7)) + 0.5 * (LN(0.8) / 3 + 2 * LN(8 / 7) / 3)          # the mixture is (5/12, 7/24, 7/24)
    js2 = 0.25 * LN(2 / 3) + 0.5 * LN(4 / 3)                                                       # the mixture is (3/8, 1/4, 3/8), both sides alike
    want = dict(top1_a=[0, 1, 2, -1], top1_b=[0, 1, 0, -1], conf_a=[0.5, 0.6, 0.5, nan], conf_b=[1 / 3, 0.6, 0.5, nan],
                kl_ab=[0.5 * LN(1.125), 0.0, 0.25 * LN(2), nan], kl_ba=[LN(2 / 3) / 3 + 2 * LN(4 / 3) / 3, 0.0, 0.25 * LN(2), nan],
                js=[js0, 0.0, js2, nan], tv=[1 / 6, 0.0, 0.25, nan], nll_a=[LN(2), LN(5), nan, nan], nll_b=[LN(3), LN(5), nan, nan],
                rank_a=[0, 2, -1, -1], rank_b=[0, 2, -1, -1], rank_b_top1a=[0, 0, 2, -1], rank_a_top1b=[0, 0, 1, -1])
    for name in CC.STATS:
        if name in CC.INT_STATS:
            assert r[name].dtype == torch.int64 and r[name].tolist() == want[name], name
        else:
            assert r[name].dtype == torch.float64
            assert torch.allclose(r[name], torch.tensor(want[name], dtype=torch.float64), rtol=0, atol=1e-14, equal_nan=True), (name, r[name])
    none = CC.reference_pair_stats(za[:3], zb[:3], None, 3)                                        # no labels: as labels outside [0, C)
    assert bool(torch.isnan(none["nll_a"]).all()) and none["rank_b"].tolist() == [-1] * 3 and none["top1_a"].tolist() == [0, 1, 2]


@pytest.mark.parametrize("C", [2, 10, 1000])
def test_sharp_rows_stay_finite(C):
    za, zb, y, r, _ = CR.case(64, C, C + 3, C, "sharp", 3)
    assert bool(((r["js"] - LN(2)).abs() < 1e-12).all()) and bool(((r["tv"] - 1.0).abs() < 1e-12).all())
    assert bool(torch.isfinite(r["kl_ab"]).all()) and float(r["kl_ab"].min()) > 150.0 and float(r["kl_ba"].min()) > 150.0
    assert bool((r["top1_a"] != r["top1_b"]).all())


def test_tie_rules_on_integer_logits():
    za, zb, y, r, _ = CR.case(65, 10, 16, 12, "tied", 1)
    a, b = za[:, :10].tolist(), zb[:, :10].tolist()
    before = lambda row, col: sum(1 for c, v in enumerate(row) if v > row[col] or (v == row[col] and c < col))
    ties = 0
    for i in range(65):
        ta, tb = a[i].index(max(a[i])), b[i].index(max(b[i]))                                     # list.index: the first maximum
        ties += a[i].count(max(a[i])) > 1
        assert (int(r["top1_a"][i]), int(r["top1_b"][i])) == (ta, tb)
        assert (int(r["rank_b_top1a"][i]), int(r["rank_a_top1b"][i])) == (before(b[i], ta), before(a[i], tb))
        yi = int(y[i])
        want = (before(a[i], yi), before(b[i], yi)) if 0 <= yi < 10 else (-1, -1)
        assert (int(r["rank_a"][i]), int(r["rank_b"][i])) == want
        if want[0] == 0:
            assert ta == yi
    assert ties > 30                                                                               # the family does tie
    same = CC.reference_pair_stats(za, za, y, 10)
    for name in ("kl_ab", "kl_ba", "tv", "js"):
        assert float(same[name].abs().max()) == 0.0, name


def heads_histogram(N):
    """[N + 1]: how many of the 2^N outcomes of N coins show h heads, by counting the bits of every integer below 2^N"""
    x = np.arange(2 ** N, dtype=np.uint32)
    heads = np.zeros(2 ** N, dtype=np.uint8)
    for bit in range(N):
        heads += ((x >> np.uint32(bit)) & np.uint32(1)).astype(np.uint8)
    return np.bincount(heads, minlength=N + 1)


def test_mcnemar_against_enumeration():
    assert CC.reference_mcnemar(0, 0) == 1.0 and CC.mcnemar(0, 0) == 1.0
    hist = {N: heads_histogram(N) for N in range(1, 25)}
    assert all(int(h.sum()) == 2 ** N for N, h in hist.items())
    for a_only, b_only in itertools.product(range(13), repeat=2):                      # every pair up to (12, 12): N up to 24, 2^24 outcomes
        N = a_only + b_only
        if N == 0:
            continue
        lo = min(a_only, b_only)                               # the outcomes as or more extreme than the one seen, both tails
        brute = min(1.0, 2.0 * int(hist[N][:lo + 1].sum()) / 2 ** N)
        assert CC.reference_mcnemar(a_only, b_only) == pytest.approx(brute, rel=1e-15), (a_only, b_only)
        assert CC.mcnemar(a_only, b_only) == pytest.approx(brute, rel=1e-12), (a_only, b_only)
    assert CC.mcnemar(400, 600) == pytest.approx(CC.reference_mcnemar(400, 600), rel=1e-10)
    assert CC.reference_mcnemar(5, 5) == 1.0 and CC.reference_mcnemar(0, 10) == 2.0 / 1024


def test_reference_cka_invariances():
    g = torch.Generator().manual_seed(0)
    X = torch.randn(200, 16, generator=g, dtype=torch.float64)
    Q = torch.linalg.qr(torch.randn(16, 16, generator=g, dtype=torch.float64))[0]
    Y = 3.5 * (X @ Q) + torch.randn(16, generator=g, dtype=torch.float64)
    assert abs(CC.reference_cka(X, Y) - 1.0) < 1e-9
    Z = torch.randn(200, 24, generator=g, dtype=torch.float64)
    assert CC.reference_cka(X, Z) == pytest.approx(CC.reference_cka(Z, X), rel=1e-12) and 0.0 < CC.reference_cka(X, Z) < 0.5
    assert CC.reference_cka(X, torch.ones(200, 8, dtype=torch.float64)) is None
    assert CC.reference_cka(torch.full((200, 8), 2.0, dtype=torch.float64), X) is None


def test_reference_compare_on_the_hand_banks():
    """tests/compare_ref.hand_banks: rows 0 .. 9 are counted.  A is right on rows 0, 1, 4, 7, 8 and B on rows 0, 2, 4, 5, 7, 8."""
    a, b = CR.hand_banks()
    rec = CC.reference_compare(a, b, topk=2, worst_images=4, worst_classes=10)
    assert (rec["images"], rec["counted"], rec["data_classes"], rec["topk"]) == (12, 10, 3, 2)
    assert rec["flips"] == dict(both=4, a_only=1, b_only=2, neither=3)
    assert (rec["a"]["top1"], rec["b"]["top1"], rec["a"]["topk"], rec["b"]["topk"]) == (0.5, 0.6, 0.9, 0.9)
    assert rec["agreement"] == 8 / 12 and rec["churn"] == 1.0 - 8 / 12
    assert (rec["negative_flip_rate"], rec["positive_flip_rate"], rec["mcnemar_p"]) == (0.1, 0.2, 1.0)                 # 2 (C(3,0) + C(3,1)) / 8
    assert rec["a_top1_in_b_topk"] == 11 / 12 and rec["b_top1_in_a_topk"] == 11 / 12                                  # row 11: rank 2 both ways
    assert [c["class"] for c in rec["classes_worst"]] == [0, 2, 1]                                                   # deltas 0, 0, +1/3: ties by index
    assert rec["classes_worst"][2] == dict({"class": 1}, support=3, recall_a=1 / 3, recall_b=2 / 3, delta=2 / 3 - 1 / 3)
    assert rec["classes_worst"][0] == dict({"class": 0}, support=4, recall_a=0.5, recall_b=0.5, delta=0.0)
    assert [(w["index"], w["label"], w["top1_a"], w["top1_b"]) for w in rec["images_worst"]] == [(1, 0, 0, 1), (5, 1, 0, 1), (11, 3, 1, 2), (2, 0, 1, 0)]
    assert rec["images_worst"][0]["js"] == rec["images_worst"][1]["js"] == rec["js_max"]                              # the tie: the lower row first
    assert rec["cka"] is None and "features" in rec["cka_reason"] and rec["matrices"] is True
    # the float fields, from softmax written out here: exp of the logits is (e^g, 1, 1) up to a permutation, or all equal
    hot = lambda g: math.exp(g) / (math.exp(g) + 2.0)          # the probability of the one raised column
    nll = lambda g, hit: -math.log(hot(g)) if hit else -math.log((1.0 - hot(g)) / 2.0)
    half = math.exp(2.0) / (2.0 * math.exp(2.0) + 1.0)         # row 6: (2, 2, 0)
    conf_a = [hot(5), hot(5), hot(3), hot(5), hot(5), hot(5), half, hot(5), hot(5), 1 / 3, hot(5), hot(4)]
    conf_b = conf_a                                            # row by row B's logits are a permutation of A's
    nll_a = [nll(5, 1), nll(5, 1), nll(3, 0), nll(5, 0), nll(5, 1), nll(5, 0), -math.log(half), nll(5, 1), nll(5, 1), math.log(3)]
    nll_b = [nll(5, 1), nll(5, 0), nll(3, 1), nll(5, 0), nll(5, 1), nll(5, 1), -math.log(half), nll(5, 1), nll(5, 1), math.log(3)]
    assert rec["a"]["confidence"] == pytest.approx(sum(conf_a) / 12, rel=1e-13) and rec["b"]["confidence"] == pytest.approx(sum(conf_b) / 12, rel=1e-13)
    assert rec["a"]["nll"] == pytest.approx(sum(nll_a) / 10, rel=1e-13) and rec["b"]["nll"] == pytest.approx(sum(nll_b) / 10, rel=1e-13)     # the counted rows only
    assert rec["a"]["nll"] != pytest.approx(rec["b"]["nll"], rel=1e-3)

    def swapped(g):                                            # a = (g, 0, 0), b = (0, g, 0): (kl, js, tv); kl_ab = kl_ba by symmetry
        p, q = hot(g), (1.0 - hot(g)) / 2.0
        mid = (p + q) / 2.0
        return (p - q) * g, p * math.log(p / mid) + q * math.log(q / mid), p - q
    moved = [swapped(5), swapped(3), swapped(5), swapped(4)]   # rows 1, 2, 5, 11; every other row has equal logits: all zero
    assert rec["kl_ab"] == pytest.approx(sum(t[0] for t in moved) / 12, rel=1e-13) and rec["kl_ba"] == pytest.approx(rec["kl_ab"], rel=1e-13)
    assert rec["js"] == pytest.approx(sum(t[1] for t in moved) / 12, rel=1e-13) and rec["tv"] == pytest.approx(sum(t[2] for t in moved) / 12, rel=1e-13)
    assert rec["js_max"] == pytest.approx(swapped(5)[1], rel=1e-13)
    CR.same_record(CC.compare_banks(a, b, topk=2, worst_images=4, worst_classes=10, stats=CC.reference_pair_stats)[0], rec)
    assert CC.reference_compare(a, b, topk=1, worst_images=0, worst_classes=1)["classes_worst"][0]["class"] == 0
    _, out = CC.compare_banks(a, b, topk=2, stats=CC.reference_pair_stats)
    assert out["moved"].tolist() == [[4, 2, 0], [1, 1, 1], [0, 0, 3]]
    assert out["confusion_a"].tolist() == [[2, 1, 1], [2, 1, 0], [1, 0, 2]] and out["confusion_b"].tolist() == [[2, 1, 1], [1, 2, 0], [1, 0, 2]]
    assert out["per_class"].tolist() == [[4, 1, 1, 1, 1], [3, 1, 0, 1, 1], [3, 2, 0, 0, 1]]
    ref = CC.reference_tables(out["top1_a"], out["top1_b"], out["rank_a"], out["rank_b"], a["labels"], 3)
    assert all(torch.equal(ref[k], out[k]) for k in ref) and set(ref) == {"per_class"} | set(CC.MATRIX_KEYS)


def test_the_parser():
    p = CC.build_parser()
    flags = lambda sub: {a.dest for a in p._subparsers._group_actions[0].choices[sub]._actions} - {"help"}
    shared = {"topk", "worst_images", "worst_classes", "cka", "chunk_rows", "output"}
    assert set(p._subparsers._group_actions[0].choices) == {"diff", "run"}
    assert flags("diff") == {"bank_a", "bank_b"} | shared
    data = argparse.ArgumentParser()
    TL.add_dataset_flags(data)
    assert flags("run") == {"a", "b", "bank_a", "bank_b"} | shared | ({a.dest for a in data._actions} - {"help"})
    d = p.parse_args(["diff", "--bank_a", "x", "--bank_b", "y"])
    assert (d.topk, d.worst_images, d.worst_classes, d.cka, d.chunk_rows, d.output) == (5, 20, 10, 1, None, None)
    r = p.parse_args(["run", "--a", "x", "--b", "y"])
    assert (r.split, r.bank_a, r.bank_b, r.topk, r.cka, r.precision) == ("test", None, None, 5, 1, "bf16")
    for bad in (["diff", "--bank_a", "x"], ["run", "--a", "x"], ["diff", "--bank_a", "x", "--bank_b", "y", "--topk", "0"],
                ["diff", "--bank_a", "x", "--bank_b", "y", "--cka", "2"], ["diff", "--bank_a", "x", "--bank_b", "y", "--chunk_rows", "0"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    with pytest.raises(SystemExit, match="--data_dir"):
        CC.main(["run", "--a", "x", "--b", "y"])


def test_refusals_by_name():
    a, b = CR.hand_banks()
    stats = CC.reference_pair_stats
    with pytest.raises(ValueError, match="bank B is not a logits bank: it lacks num_classes"):
        CC.compare_banks(a, {k: v for k, v in b.items() if k != "num_classes"}, topk=1, stats=stats)
    with pytest.raises(ValueError, match="bank A is not a logits bank"):
        CC.compare_banks(dict(features=torch.zeros(12, 8), labels=a["labels"], data_classes=3, meta={}), b, topk=1, stats=stats)
    short = dict(b, logits=b["logits"][:11], labels=b["labels"][:11])
    with pytest.raises(ValueError, match="differ in rows: bank A has 12, bank B has 11"):
        CC.compare_banks(a, short, topk=1, stats=stats)
    moved = dict(b, labels=b["labels"].clone())
    moved["labels"][[4, 9]] = 0
    with pytest.raises(ValueError, match=r"labels differ \(2 rows, the first at row 4\): not the same split in the same order"):
        CC.compare_banks(a, moved, topk=1, stats=stats)
    with pytest.raises(ValueError, match="differ in data_classes: bank A has 3, bank B has 2"):
        CC.compare_banks(a, dict(b, data_classes=2), topk=1, stats=stats)
    with pytest.raises(ValueError, match="data_classes 5 is not within bank A's num_classes 4"):
        CC.compare_banks(dict(a, data_classes=5), dict(b, data_classes=5), topk=1, stats=stats)
    for k in (0, 4):
        with pytest.raises(ValueError, match=r"--topk must lie in \[1, data_classes = 3\]"):
            CC.compare_banks(a, b, topk=k, stats=stats)
    nan = dict(a, logits=a["logits"].clone())
    nan["logits"][6, 1] = float("nan")
    with pytest.raises(ValueError, match="row 6 of the banks holds a NaN logit"):
        CC.compare_banks(nan, b, topk=1, stats=stats)
    CC.compare_banks(dict(a, data_classes=2), dict(b, data_classes=2, num_classes=8), topk=2, stats=stats)          # num_classes may differ


def test_cka_conditions_are_named():
    a, b = CR.hand_banks()
    g = torch.Generator().manual_seed(2)
    fa, fb = torch.randn(12, 16, generator=g), torch.randn(12, 24, generator=g)
    run = lambda x, y, **kw: CC.compare_banks(x, y, topk=1, stats=CC.reference_pair_stats, cka_fn=CC.reference_cka, **kw)[0]
    rec = run(dict(a, features=fa, normalized=False), dict(b, features=fb, normalized=False))
    assert rec["cka"] == CC.reference_cka(fa, fb) and "cka_reason" not in rec
    assert run(dict(a, features=fa, normalized=False), dict(b, features=fb, normalized=False), cka=0)["cka_reason"] == "--cka 0"
    assert "bank B holds no features" in run(dict(a, features=fa, normalized=False), b)["cka_reason"]
    assert "normalized" in run(dict(a, features=fa, normalized=False), dict(b, features=fb, normalized=True))["cka_reason"]
    assert "width 12" in run(dict(a, features=fa[:, :12], normalized=False), dict(b, features=fb, normalized=False))["cka_reason"]
    assert "width 1024" in run(dict(a, features=fa, normalized=False), dict(b, features=torch.zeros(12, 1024), normalized=False))["cka_reason"]
    rec = run(dict(a, features=fa, normalized=False), dict(b, features=torch.ones(12, 8), normalized=False))
    assert rec["cka"] is None and rec["cka_reason"] == "constant features"

    def refusing(X, Y, chunk_rows=None):
        raise L.UvcHipError("uvc_gemm_tn: no float32 kernel for this shape")
    rec = CC.compare_banks(dict(a, features=fa, normalized=False), dict(b, features=fb, normalized=False), topk=1, stats=CC.reference_pair_stats,
                           cka_fn=refusing)[0]
    assert rec["cka"] is None and "uvc_gemm_tn" in rec["cka_reason"]


def test_diff_end_to_end_on_the_cpu(tmp_path, capsys):
    za, zb = CR.pair(50, 10, 16, 12, "normal", 4)
    y = CR.labels_for(50, 10, 4)
    g = torch.Generator().manual_seed(3)
    from uvc_amd import compact_calibrate as CAL
    from uvc_amd import compact_ood as OD
    za, zb = torch.nan_to_num(za, nan=0.5), torch.nan_to_num(zb, nan=-0.5)
    bank_a = OD.make_ood_bank(torch.randn(50, 16, generator=g), za, y, 10, dataset="fixture", split="test")         # a compact_ood bank ...
    bank_b = CAL.make_logits_bank(zb, y, 10, dataset="fixture", split="test")                                       # ... against a compact_calibrate bank
    torch.save(bank_a, tmp_path / "a.pt")
    torch.save(bank_b, tmp_path / "b.pt")
    args = CC.build_parser().parse_args(["diff", "--bank_a", str(tmp_path / "a.pt"), "--bank_b", str(tmp_path / "b.pt"), "--topk", "3",
                                         "--worst_images", "7", "--worst_classes", "4", "--output", str(tmp_path / "d.pt")])
    rec = CC.diff_command(args, stats=CC.reference_pair_stats, cka_fn=CC.reference_cka)
    assert rec.pop("img_per_s") > 0
    want = CC.reference_compare(bank_a, bank_b, topk=3, worst_images=7, worst_classes=4)
    CR.same_record(rec, want)
    assert json.loads(json.dumps(rec)) == rec
    assert len(rec["images_worst"]) == 7 and len(rec["classes_worst"]) == 4 and rec["counted"] == int(((y >= 0) & (y < 10)).sum())
    assert "bank B holds no features" in rec["cka_reason"]
    out = torch.load(tmp_path / "d.pt")
    assert set(out) == set(CC.STATS) | {"per_class"} | set(CC.MATRIX_KEYS)
    assert all(out[k].shape == (50,) for k in CC.STATS) and all(out[k].shape == (10, 10) and out[k].dtype == torch.int64 for k in CC.MATRIX_KEYS)
    assert out["per_class"].shape == (10, 5) and int(out["per_class"][:, 0].sum()) == rec["counted"] and int(out["moved"].sum()) == 50
    with pytest.raises(ValueError, match="differ in rows"):
        CC.diff_command(argparse.Namespace(**dict(vars(args), bank_b=dict(bank_b, logits=zb[:49], labels=y[:49]))), stats=CC.reference_pair_stats)


def test_the_matrices_are_skipped_beyond_the_limit(monkeypatch):
    a, b = CR.hand_banks()
    monkeypatch.setattr(CC, "MAX_MATRIX", 8)                   # 3 * 3 entries are too many now
    rec, out = CC.compare_banks(a, b, topk=1, stats=CC.reference_pair_stats)
    assert rec["matrices"] is False and not set(CC.MATRIX_KEYS) & set(out) and out["per_class"].shape == (3, 5)


def test_ops_refuse_cpu_tensors():
    za, zb = CR.pair(4, 10, 16, 16, "normal", 0)
    with pytest.raises(L.UvcHipError, match="CPU tensor"):
        ops.logits_pair_stats(za, zb, None, n_valid=10)
    with pytest.raises(L.UvcHipError, match="CPU tensor"):
        ops.linear_cka(torch.zeros(8, 8), torch.zeros(8, 8))
    assert ops.PAIR_STATS == CC.STATS and ops.PAIR_STATS_INT == CC.INT_STATS
