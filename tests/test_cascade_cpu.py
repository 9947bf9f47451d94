"""CPU: the written specs of uvc_amd/compact_cascade.py -- the scores against a direct float64 softmax, the sweep against a loop over every
threshold, the selectors, a planted case -- and the bank command, the policy file and every refusal through the float64 specs."""
import argparse
import copy
import json
import math

import pytest
import torch

import cascade_ref as CR
import knn_ref as KR
from uvc_amd import compact_cascade as CS

INF = float("inf")


# ---- the scores -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", CS.SCORES)
@pytest.mark.parametrize("T", [0.5, 1.0, 3.0])
@pytest.mark.parametrize("C,ld", [(1, 8), (2, 2), (10, 16), (37, 40)])
def test_reference_scores_equal_a_direct_softmax(kind, T, C, ld):
    z = CR.logits_case(65, C, ld, C + 3).clone()
    z[9, C - 1] = float("nan")                                               # one NaN: its row alone is NaN
    got, want = CS.reference_scores(z, C, T, kind), CR.direct_scores(z, C, T, kind)
    assert got.dtype == torch.float64 and torch.equal(torch.isnan(got), torch.isnan(want)) and torch.isnan(got).tolist() == [i == 9 for i in range(65)]
    ok = ~torch.isnan(want)
    assert float((got[ok] - want[ok]).abs().max()) <= 1e-13
    assert float(got[ok].min()) >= -1e-13 and float(got[ok].max()) <= 1.0 + 1e-13
    if C == 1:
        assert torch.equal(got[ok], torch.ones(64, dtype=torch.float64))
    else:
        if kind == "margin":
            assert float(got[2]) == 0.0                                      # the maximum appears twice: the two largest entries are equal
        assert abs(float(got[3]) - {"msp": 1.0 / C, "margin": 0.0, "entropy": 0.0}[kind]) <= 1e-13        # all equal: the uniform row
    top = CS.reference_top1(z, C)
    assert int(top[9]) == -1 and int(top[3]) == 0 and torch.equal(top[ok], z[:, :C][ok].double().argmax(dim=1))
    if C > 1:
        assert float(z[2, int(top[2])]) == float(z[2, :C].max()) and not bool((z[2, :int(top[2])] == z[2, :C].max()).any())


def test_temperature_orders_confidence():
    z = CR.logits_case(65, 10, 16, 1)
    rows = [i for i in range(65) if i not in (3,)]
    for kind in CS.SCORES:
        cold, warm = CS.reference_scores(z, 10, 0.5, kind)[rows], CS.reference_scores(z, 10, 3.0, kind)[rows]
        assert bool((cold >= warm - 1e-12).all()), kind                       # a lower temperature never makes a row less sure


# ---- the sweep --------------------------------------------------------------------------------------------------------------------------
def curve_of(bs, bl, **kw):
    return CS.reference_curve(bs, bl, macs_small=kw.pop("macs_small", 100.0), macs_large=kw.pop("macs_large", 1000.0), **kw)


@pytest.mark.parametrize("kind", CS.SCORES)
@pytest.mark.parametrize("tied", [True, False])
def test_reference_curve_equals_the_loop_over_every_threshold(kind, tied):
    bs, bl = CR.synthetic_banks(300, 5, 8, 3, tied)
    rec, out = curve_of(bs, bl, score=kind, temperature=1.5, points=11)
    C = 5
    brute = CR.brute_curve(out["score"], out["top1_small"], out["top1_large"], bs["labels"], C, 100.0, 1000.0)
    assert rec["thresholds"] == len(brute) == out["threshold"].shape[0] and (rec["images"], rec["counted"], rec["data_classes"]) == (300, 298, 5)
    if tied:
        assert len(brute) < 300 - 50                                         # tied scores: far fewer thresholds than rows
    for j, p in enumerate(brute):
        tau = p["threshold"] if j + 1 < len(brute) else -INF                 # (the last point keeps every row: its threshold is written -inf)
        assert float(out["threshold"][j]) == tau and float(out["defer_rate"][j]) == p["defer_rate"], j
        assert float(out["accuracy"][j]) == p["accuracy"] and float(out["macs"][j]) == p["macs"], j
    # the two ends: every row deferred gives the large model's accuracy, none the small model's
    assert float(out["threshold"][0]) == INF and float(out["accuracy"][0]) == rec["large"]["top1"] and float(out["defer_rate"][0]) == 1.0
    assert float(out["accuracy"][-1]) == rec["small"]["top1"] and float(out["defer_rate"][-1]) == 0.0 and float(out["macs"][-1]) == 100.0
    y, ts, tl = bs["labels"], out["top1_small"], out["top1_large"]
    counted = (y >= 0) & (y < C)
    assert rec["small"]["top1"] == int(((ts == y) & counted).sum()) / 298 and rec["large"]["top1"] == int(((tl == y) & counted).sum()) / 298
    assert rec["oracle"] == int((((ts == y) | (tl == y)) & counted).sum()) / 298 >= max(rec["small"]["top1"], rec["large"]["top1"])
    # cost rises with the defer rate, and both fall along the full curve
    assert bool((out["defer_rate"][:-1] > out["defer_rate"][1:]).all()) and bool((out["macs"][:-1] > out["macs"][1:]).all())
    # a threshold is the score of a row, and tied scores fall on one side of it together
    scores = set(out["score"].tolist())
    for j in range(1, len(brute) - 1):
        tau = float(out["threshold"][j])
        assert tau in scores
        deferred = ~(out["score"] >= tau)
        assert int((~deferred).sum()) == brute[j]["kept"]
        assert not bool(deferred[out["score"] == tau].any())
    # the record's curve: the first point at or above every evenly spaced rate
    assert len(rec["curve"]) == 11 and rec["curve"][0]["defer_rate"] == 0.0 and rec["curve"][-1]["defer_rate"] == 1.0
    for j, p in enumerate(rec["curve"]):
        want = min((q for q in brute if q["defer_rate"] >= j / 10), key=lambda q: q["defer_rate"])
        assert set(p) == set(CS.POINT_KEYS) and p["defer_rate"] == want["defer_rate"] and p["accuracy"] == want["accuracy"], j
    best = min(brute, key=lambda q: (-q["accuracy"], q["macs"]))
    assert rec["best"]["accuracy"] == best["accuracy"] and rec["best"]["macs"] == best["macs"]
    asc = brute[::-1]
    area = math.fsum((b["defer_rate"] - a["defer_rate"]) * (a["accuracy"] + b["accuracy"]) / 2 for a, b in zip(asc, asc[1:]))
    assert abs(rec["area"] - area) <= 1e-12 and rec["chosen"] is None and "defer_at_chosen" not in out


def test_each_selector_picks_what_the_loop_picks():
    bs, bl = CR.synthetic_banks(300, 5, 8, 4)
    _, out = curve_of(bs, bl)
    brute = CR.brute_curve(out["score"], out["top1_small"], out["top1_large"], bs["labels"], 5, 100.0, 1000.0)
    large, small = brute[0]["accuracy"], brute[-1]["accuracy"]
    assert large > small
    cases = [dict(match_large=0.0), dict(match_large=0.02), dict(match_large=1.0), dict(target_accuracy=(small + large) / 2), dict(target_accuracy=small),
             dict(max_macs=100.0), dict(max_macs=450.0), dict(max_macs=1100.0), dict(max_macs=5000.0)]
    for kw in cases:
        rec, o = curve_of(bs, bl, **kw)
        want = CR.brute_choose(brute, large, **kw)
        got = rec["chosen"]
        assert got["accuracy"] == want["accuracy"] and got["macs"] == want["macs"] and got["defer_rate"] == want["defer_rate"], kw
        tau = got["threshold"]
        assert tau == (want["threshold"] if want is not brute[-1] else -INF)
        assert torch.equal(o["defer_at_chosen"], ~(o["score"] >= tau)) and int(o["defer_at_chosen"].sum()) == 300 - want["kept"]
    assert curve_of(bs, bl, match_large=1.0)[0]["chosen"]["defer_rate"] == 0.0 == curve_of(bs, bl, max_macs=100.0)[0]["chosen"]["defer_rate"]
    # targets that cannot be met are refused, naming the best value reachable
    top = max(p["accuracy"] for p in brute)
    with pytest.raises(ValueError, match=r"--target_accuracy 0\.999 cannot be met: the best accuracy reachable is " + str(top)[:8]):
        curve_of(bs, bl, target_accuracy=0.999)
    with pytest.raises(ValueError, match="--match_large -0.5 cannot be met: the best accuracy reachable is"):
        curve_of(bs, bl, match_large=-0.5)
    with pytest.raises(ValueError, match=r"--max_macs 99\.0 cannot be met: the cheapest cost reachable is 100\.0"):
        curve_of(bs, bl, max_macs=99.0)
    with pytest.raises(ValueError, match="one selector at a time"):
        curve_of(bs, bl, max_macs=500.0, match_large=0.0)


def test_a_planted_case():
    """The small model is right exactly where its score is high and the large one everywhere: the curve reaches the large model's accuracy
    at the planted defer rate, and ``best`` names it."""
    bs, bl, rate = CR.planted_banks()
    for kind in CS.SCORES:
        rec, out = curve_of(bs, bl, score=kind, match_large=0.0, points=201)
        assert rec["large"]["top1"] == 1.0 == rec["oracle"] and rec["small"]["top1"] == 130 / 200 and rate == 70 / 200
        assert rec["best"]["accuracy"] == 1.0 and rec["best"]["defer_rate"] == rate and rec["chosen"] == rec["best"], kind
        assert all(p["accuracy"] < 1.0 for p in rec["curve"] if p["defer_rate"] < rate) and all(p["accuracy"] == 1.0 for p in rec["curve"] if p["defer_rate"] >= rate)
        assert torch.equal(out["defer_at_chosen"], torch.arange(200) >= 200 - int(round(rate * 200)))


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
def test_curve_command_and_the_policy_file(tmp_path, capsys):
    bs, bl = CR.synthetic_banks(300, 5, 8, 5)
    torch.save(bs, tmp_path / "s.pt")
    torch.save(bl, tmp_path / "l.pt")
    base = ["curve", "--bank_small", str(tmp_path / "s.pt"), "--bank_large", str(tmp_path / "l.pt")]
    macs = ["--macs_small", "100", "--macs_large", "1000"]
    rec = CS.main(base + macs + ["--score", "margin", "--temperature", "2", "--match_large", "0.01", "--points", "5", "--policy", str(tmp_path / "p.json"),
                                "--output", str(tmp_path / "c.pt")], scorer=CS.reference_scorer)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == rec
    want, out = curve_of(bs, bl, score="margin", temperature=2.0, match_large=0.01, points=5)
    assert {k: v for k, v in rec.items() if k != "rows_per_s"} == want and rec["rows_per_s"] > 0
    saved = torch.load(tmp_path / "c.pt")
    assert set(saved) == set(CS.POINT_KEYS) | {"score", "top1_small", "top1_large", "defer_at_chosen"} and all(torch.equal(saved[k], out[k]) for k in out)
    pol = json.load(open(tmp_path / "p.json"))
    assert tuple(pol) == CS.POLICY_KEYS and pol["expected"] == dict(accuracy=rec["chosen"]["accuracy"], defer_rate=rec["chosen"]["defer_rate"], macs=rec["chosen"]["macs"])
    assert (pol["score"], pol["temperature"], pol["threshold"], pol["data_classes"], pol["img_size"], pol["patch_size"]) == \
        ("margin", 2.0, rec["chosen"]["threshold"], 5, 64, None) and (pol["macs_small"], pol["macs_large"]) == (100.0, 1000.0)
    # the policy round-trips through run's and predict's parsers: the same rule, the same float32 threshold, hence the same split
    for cmd in (["run", "--dataset", "cifar10", "--data_dir", "x"], ["predict", "--images", "x"]):
        args = CS.build_parser().parse_args(cmd + ["--small", "a", "--large", "b", "--policy", str(tmp_path / "p.json")])
        rule = CS.rule_of(args)
        assert (rule["score"], rule["temperature"], rule["threshold"], rule["data_classes"]) == ("margin", 2.0, pol["threshold"], 5) and rule["policy"] == pol
        assert torch.equal(~(saved["score"] >= torch.tensor(rule["threshold"], dtype=torch.float32)), saved["defer_at_chosen"])
    run = CS.build_parser().parse_args(["run", "--small", "a", "--large", "b", "--threshold=-inf", "--dataset", "cifar10", "--data_dir", "x"])
    assert (run.split, run.score, run.temperature) == ("test", "msp", 1.0) and CS.rule_of(run)["threshold"] == -INF
    # a policy of the -inf end survives JSON
    CS.main(base + macs + ["--match_large", "1", "--policy", str(tmp_path / "q.json")], scorer=CS.reference_scorer)
    assert CS.load_policy(str(tmp_path / "q.json"))["threshold"] == -INF
    # the compact files give the MACs compact export prints, and their geometry
    ex_s, ex_l = KR.export_of("stage2_micro_skip")[0], KR.export_of("stage2_micro_deit")[0]
    torch.save(ex_s, tmp_path / "s.compact.pt")
    torch.save(ex_l, tmp_path / "l.compact.pt")
    from uvc_amd import compact as CP
    rec2 = CS.main(base + ["--small", str(tmp_path / "s.compact.pt"), "--large", str(tmp_path / "l.compact.pt"), "--max_macs", "1e12",
                          "--policy", str(tmp_path / "r.json")], scorer=CS.reference_scorer)
    assert rec2["small"]["macs"] == CP.compact_macs(ex_s, 1, padded=True) and rec2["large"]["macs"] == CP.compact_macs(ex_l, 1, padded=True)
    pol2 = CS.load_policy(str(tmp_path / "r.json"))
    assert (pol2["img_size"], pol2["patch_size"]) == (ex_s["cfg"]["img_size"], ex_s["cfg"]["patch_size"])


def test_refusals_by_name(tmp_path):
    bs, bl = CR.synthetic_banks(40, 5, 8, 6)
    paths = {}
    for name, b in (("s", bs), ("l", bl), ("short", dict(bl, logits=bl["logits"][:39], labels=bl["labels"][:39])),
                    ("moved", dict(bl, labels=bl["labels"].roll(1))), ("classes", dict(bl, data_classes=6)), ("nobank", dict(logits=bl["logits"])),
                    ("nan", dict(bs, logits=bs["logits"].clone().index_fill_(0, torch.tensor([4]), float("nan"))))):
        paths[name] = str(tmp_path / f"{name}.pt")
        torch.save(b, paths[name])
    macs = ["--macs_small", "100", "--macs_large", "1000"]
    curve = lambda s, l, *more: CS.main(["curve", "--bank_small", paths[s], "--bank_large", paths[l]] + list(more), scorer=CS.reference_scorer)
    for other, text in (("short", "differ in rows"), ("moved", "not the same split in the same order"), ("classes", "differ in data_classes"),
                        ("nobank", "is not a logits bank")):                # compact_compare.check_pair's refusals
        with pytest.raises(ValueError, match=text):
            curve("s", other, *macs)
    with pytest.raises(ValueError, match="row 4 of the small bank has no score"):
        curve("nan", "l", *macs)
    for T in ("0", "-1", "inf", "nan"):
        with pytest.raises(ValueError, match="--temperature must be positive and finite"):
            curve("s", "l", "--temperature", T, *macs)
    with pytest.raises(ValueError, match="need --small and --large, or --macs_small and --macs_large"):
        curve("s", "l", "--macs_small", "100")
    with pytest.raises(ValueError, match="--policy needs an operating point"):
        curve("s", "l", "--policy", str(tmp_path / "p.json"), *macs)
    with pytest.raises(SystemExit):
        curve("s", "l", "--match_large", "0", "--max_macs", "3", *macs)
    # two files
    ex_s, ex_l = KR.export_of("stage2_micro_skip")[0], KR.export_of("stage2_micro_deit")[0]
    px = KR.export_of("px384d")[0]
    p8 = copy.deepcopy(ex_l)
    p8["cfg"]["patch_size"] = 8
    ns = lambda cmd, **kw: argparse.Namespace(**dict(vars(CS.build_parser().parse_args(cmd)), **kw))
    run, pred = ["run", "--small", "a", "--large", "b", "--dataset", "cifar10", "--data_dir", "x"], ["predict", "--small", "a", "--large", "b", "--images", "x"]
    for cmd, call in ((run, CS.run_command), (pred, CS.predict_command)):
        rule = ["--threshold", "0.5"]
        with pytest.raises(ValueError, match="the files differ in img_size: --small has 64, --large has 384"):
            call(ns(cmd + rule, small=ex_s, large=px))
        with pytest.raises(ValueError, match="the files differ in patch_size"):
            call(ns(cmd + rule, small=ex_s, large=p8))
        with pytest.raises(ValueError, match="--temperature must be positive and finite"):
            call(ns(cmd + rule + ["--temperature", "0"], small=ex_s, large=ex_l))
        with pytest.raises(ValueError, match="the threshold is NaN"):
            call(ns(cmd + ["--threshold", "nan"], small=ex_s, large=ex_l))
        with pytest.raises(ValueError, match="need --policy or --threshold"):
            call(ns(cmd, small=ex_s, large=ex_l))
        pol = dict(score="msp", temperature=1.0, threshold=0.5, data_classes=17, img_size=64, patch_size=16, macs_small=1.0, macs_large=2.0, expected={})
        with pytest.raises(ValueError, match="data_classes 17 is not within the heads' widths: --small has 16, --large has 16"):
            call(ns(cmd, small=ex_s, large=ex_l, policy=pol))
        with pytest.raises(ValueError, match="the policy was made at img_size 32"):
            call(ns(cmd, small=ex_s, large=ex_l, policy=dict(pol, data_classes=10, img_size=32)))
        with pytest.raises(ValueError, match="not a cascade policy: it lacks threshold"):
            call(ns(cmd, small=ex_s, large=ex_l, policy={k: v for k, v in pol.items() if k != "threshold"}))
    with pytest.raises(ValueError, match="data_classes 5 is not within|the files differ in img_size"):
        CS.curve_command(ns(["curve", "--bank_small", paths["s"], "--bank_large", paths["l"]], small=ex_s, large=px), scorer=CS.reference_scorer)
    with pytest.raises(ValueError, match="--score must be one of"):
        CS.check_rule("energy")
    with pytest.raises(ValueError, match="--points must be at least 2"):
        CS.reference_curve(bs, bl, macs_small=1.0, macs_large=2.0, points=1)


def test_reference_cascade_follows_the_rule():
    ex_s, x = KR.export_of("stage2_micro_skip")
    ex_l = KR.export_of("stage2_micro_deit")[0]
    from uvc_amd import compact as CP
    zs, zl = CP.reference_forward(ex_s, x.double())[:, :10], CP.reference_forward(ex_l, x.double())[:, :10]
    s = CS.reference_scores(zs, 10, 1.0, "msp")
    for tau, want in ((-INF, [0] * len(x)), (INF, [1] * len(x)), (float(s.float().max()), None)):
        out, source, score = CS.reference_cascade(ex_s, ex_l, x, threshold=tau, num_labels=10)
        assert torch.equal(score, s) and out.dtype == torch.float64 and out.shape == (len(x), 10)
        if want is None:                                                     # tau is a row's own float32 score: compared in float32, that row alone is kept
            want = (~(s.float() >= tau)).long().tolist()
            assert sum(want) == len(x) - 1
        assert source.tolist() == want
        assert torch.equal(out, torch.where(source[:, None] > 0, zl, zs))


def test_the_bindings_take_the_arguments_the_header_declares():
    """ctypes passes an argument beyond ``argtypes`` as a C int: a binding that is one entry short hands the kernel launch half a stream
    handle.  Every uvc_cascade_* declaration of include/uvc_kernels.h against its row of ``_lib._SIGNATURES``, by count and by kind."""
    import ctypes
    import os
    import re
    from uvc_amd import _lib
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "uvc_kernels.h")
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    found = re.findall(r"int\s+(uvc_cascade_\w+)\s*\((.*?)\);", src, flags=re.S)
    assert sorted(n for n, _ in found) == ["uvc_cascade_compact", "uvc_cascade_compact_workspace_bytes", "uvc_cascade_decide", "uvc_cascade_gather",
                                          "uvc_cascade_merge"]
    kinds = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float}
    for name, params in found:
        want = []
        for p in params.split(","):
            p = p.strip()
            want.append(ctypes.c_void_p if "*" in p and "int64_t* bytes" not in p else ctypes.POINTER(ctypes.c_int64) if "*" in p else kinds[p.split()[0]])
        assert _lib._SIGNATURES[name] == want, name
