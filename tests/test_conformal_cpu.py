"""CPU: split conformal prediction sets (uvc_amd/compact_conformal.py) -- the float64 spec (tests/conformal_ref.py) against a brute-force loop
and against the module's ``reference_*``, the quantile index rule, ties, the coverage guarantee on a synthetic bank, the parser, the
calibration file, the refusals, and both commands end to end on the CPU evaluator."""
import json
import math

import numpy as np
import pytest
import torch

import conformal_ref as CR
from uvc_amd import compact_calibrate as CC
from uvc_amd import compact_conformal as CF

META = dict(img_size=32, dataset="cifar10", split="test", interpolation="bilinear", crop_pct=None, precision="fp32")


def tiny_rows():
    rng = np.random.default_rng(5)
    rows = [rng.standard_normal(c).astype(np.float32) * 3 for c in (1, 2, 3, 7, 12)]
    rows.append(np.array([1.0, 1.0, -0.0, 0.0, 2.0, 2.0, -1.0], dtype=np.float32))           # ties, and the two zeros
    rows.append(np.array([0.5, -np.inf, 3.0, -np.inf, 0.5], dtype=np.float32))              # -inf: p = 0, by index at the end
    rows.append(np.array([3e4, -3e4, 2.9e4, 0.0], dtype=np.float32))
    return rows


@pytest.mark.parametrize("method", CR.METHODS)
@pytest.mark.parametrize("u", [None, 0.0, 0.37])
def test_reference_equals_the_definition_in_loops(method, u):
    for row in tiny_rows():
        for T in (1.0, 2.5):
            C = len(row)
            want = np.array(CR.brute_class_scores(row, method, 1.0 if u is None else u, T, 0.05, 2))
            uu = None if u is None else np.array([u])
            got = CR.class_scores(row[None, :], C, method, uu, T, 0.05, 2)[0]
            mod = CF.reference_class_scores(torch.from_numpy(row[None, :]), C, method, None if u is None else torch.tensor([u], dtype=torch.float64), T, 0.05, 2)[0].numpy()
            assert np.allclose(got, want, rtol=0, atol=1e-14), (method, u, T, row, got, want)
            assert np.allclose(mod, want, rtol=0, atol=1e-14), (method, u, T, row, mod, want)


def test_columns_past_the_classes_are_not_read():
    rng = np.random.default_rng(0)
    z = rng.standard_normal((6, 8)).astype(np.float32)
    poisoned = z.copy()
    poisoned[:, 5:] = np.nan
    y = np.array([0, 4, -1, 5, 2, 7])
    for method in CR.METHODS:
        a, m = CR.label_scores(z[:, :5], y, 5, method)
        b, mb = CR.label_scores(poisoned, y, 5, method)
        c, mc = CF.reference_scores(torch.from_numpy(poisoned), torch.from_numpy(y), 5, method)
        assert m == mb == mc == 3 and np.array_equal(a, b, equal_nan=True) and np.allclose(c.numpy(), a, atol=1e-15, rtol=0, equal_nan=True)
        assert np.isnan(a[[2, 3, 5]]).all() and not np.isnan(a[[0, 1, 4]]).any()


def test_quantile_index_rule():
    assert CF.quantile_index(999, "0.1") == CR.quantile_index(999, "0.1") == 900        # (float arithmetic: (1000)(1 - 0.1) = 900.0000000000001 -> 901)
    assert CF.quantile_index(999, 0.1) == 900
    assert CF.quantile_index(1000, "0.1") == 901 and CF.quantile_index(9, "0.1") == 9 and CF.quantile_index(8, "0.1") == 9
    assert CF.quantile_index(1, "0.5") == 1 and CF.quantile_index(1, "0.4") == 2
    for bad in ("0", "1", "-0.1", "1.5", "x", "nan"):
        with pytest.raises(ValueError):
            CF.quantile_index(10, bad)
    with pytest.raises(ValueError):
        CF.quantile_index(0, "0.1")


def test_k_beyond_m_gives_every_class_and_m_equal_one():
    z, y = CR.synthetic_bank(8, 5, 1)
    cal = CF.fit_conformal(torch.from_numpy(z), torch.from_numpy(y), 5, "0.1", "aps", scorer=CF.reference_scores)
    assert cal["k"] == 9 and cal["rows"] == 8 and cal["qhat"] == math.inf
    size, covered, members = CF.reference_sets(torch.from_numpy(z), cal["qhat"], torch.from_numpy(y), 5, "aps", members=True)
    assert size.tolist() == [5] * 8 and covered.tolist() == [1] * 8 and members[:, 0].tolist() == [31] * 8
    one = CF.fit_conformal(torch.from_numpy(z[:1]), torch.from_numpy(y[:1]), 5, "0.5", "lac", scorer=CF.reference_scores)
    assert one["k"] == 1 and one["rows"] == 1 and abs(one["qhat"] - CR.label_scores(z[:1], y[:1], 5, "lac")[0][0]) <= 1e-15
    with pytest.raises(ValueError):
        CF.fit_conformal(torch.from_numpy(z), torch.full((8,), -1), 5, "0.1", scorer=CF.reference_scores)      # m = 0


@pytest.mark.parametrize("C", [1, 4, 10])
def test_ties_go_by_index_on_equal_rows(C):
    z = np.full((3, C), 1.25, dtype=np.float32)
    u = np.array([0.0, 0.25, 1.0])
    s = CR.class_scores(z, C, "aps", u)
    want = (np.arange(C)[None, :] + u[:, None]) / C
    assert np.allclose(s, want, rtol=0, atol=1e-15)
    assert np.allclose(CF.reference_class_scores(torch.from_numpy(z), C, "aps", torch.from_numpy(u)).numpy(), want, rtol=0, atol=1e-15)


def test_u_zero_always_admits_the_first_class():
    z, _ = CR.synthetic_bank(200, 10, 2)
    inset = CR.sets(z, 0.0, 10, "aps", np.zeros(200))
    top = np.argmax(z, axis=1)
    assert inset[np.arange(200), top].all() and (inset.sum(1) == 1).all()
    size, _, _ = CF.reference_sets(torch.from_numpy(z), 0.0, None, 10, "aps", torch.zeros(200))
    assert size.tolist() == [1] * 200


def test_raps_without_a_penalty_is_aps():
    z, y = CR.synthetic_bank(50, 12, 3)
    u = np.random.default_rng(0).random(50)
    assert np.array_equal(CR.class_scores(z, 12, "raps", u, 1.5, 0.0, 3), CR.class_scores(z, 12, "aps", u, 1.5))
    a = CF.reference_class_scores(torch.from_numpy(z), 12, "raps", torch.from_numpy(u), 1.5, 0.0, 3)
    assert torch.equal(a, CF.reference_class_scores(torch.from_numpy(z), 12, "aps", torch.from_numpy(u), 1.5))
    pen = CR.class_scores(z, 12, "raps", u, 1.5, 0.1, 3) - CR.class_scores(z, 12, "aps", u, 1.5)
    rank = (-z).argsort(axis=1, kind="stable").argsort(axis=1) + 1
    assert np.allclose(pen, 0.1 * np.maximum(0, rank - 3), rtol=0, atol=1e-15)


def test_pack_and_unpack_members():
    rng = np.random.default_rng(1)
    for C in (1, 31, 32, 33, 100):
        inset = torch.from_numpy(rng.random((7, C)) < 0.5)
        inset[0] = True
        w = CF.pack_members(inset)
        assert tuple(w.shape) == (7, (C + 31) // 32) and w.dtype == torch.int32
        assert torch.equal(CF.unpack_members(w, C), inset)
        assert all(bin(int(v) & 0xFFFFFFFF).count("1") for v in w[0].tolist()) and sum(bin(int(v) & 0xFFFFFFFF).count("1") for v in w[0].tolist()) == C


BANKS = {}


def bank_of(C):
    if C not in BANKS:
        z, y = CR.synthetic_bank(20000, C, 100 + C)
        BANKS[C] = (torch.from_numpy(z), torch.from_numpy(y))
    return BANKS[C]


@pytest.mark.parametrize("alpha", ["0.1", "0.05"])
@pytest.mark.parametrize("C", [10, 100])
@pytest.mark.parametrize("method, randomized", [("lac", False), ("aps", True), ("raps", True), ("aps", False)])
def test_coverage_guarantee_on_a_synthetic_bank(method, randomized, C, alpha):
    """5000 rows calibrate, 15000 test, labels drawn from softmax(z): coverage within 4 standard deviations of 1 - alpha for the three
    continuous scores -- the spread of the calibration quantile and of the test mean, a (1 - a)(1 / m_cal + 1 / m_test): 0.02 at alpha = 0.1 --;
    deterministic aps (u = 1) covers at least that."""
    z, y = bank_of(C)
    a = float(alpha)
    margin = 4 * math.sqrt(a * (1 - a) * (1 / 5000 + 1 / 15000))
    assert alpha != "0.1" or abs(margin - 0.02) < 5e-4
    cal = CF.fit_conformal(z[:5000], y[:5000], C, alpha, method, randomized=randomized, seed=7, scorer=CF.reference_scores)
    assert cal["rows"] == 5000 and cal["k"] == CR.quantile_index(5000, alpha) and cal["randomized"] == randomized
    u_cal = CF.draw_u(5000, 7).numpy() if randomized else None
    assert abs(cal["qhat"] - CR.qhat_of(CR.label_scores(z[:5000].numpy(), y[:5000].numpy(), C, method, u_cal, 1.0, cal["lam"], cal["k_reg"])[0], alpha)) <= 1e-14
    bank = CC.make_logits_bank(z[5000:], y[5000:], C, **META)
    rec = CF.evaluate(bank, dict(version=1, **cal, data_classes=C, num_classes=C, meta={}), setter=CF.reference_sets)
    u_test = CF.draw_u(15000, 8).numpy() if randomized else None
    inset = CR.sets(z[5000:].numpy(), cal["qhat"], C, method, u_test, 1.0, cal["lam"], cal["k_reg"])
    cov = inset[np.arange(15000), y[5000:].numpy()].mean()
    assert rec["rows"] == 15000 and abs(rec["coverage"] - cov) < 1e-12 and abs(rec["mean_size"] - inset.sum(1).mean()) < 1e-9
    print(method, randomized, C, alpha, "coverage", rec["coverage"], "mean size", rec["mean_size"], "margin", margin)
    if method == "aps" and not randomized:
        assert rec["coverage"] >= 1 - a - margin
    else:
        assert abs(rec["coverage"] - (1 - a)) <= margin


def test_record_members_on_a_hand_made_case():
    size = torch.tensor([0, 1, 1, 2, 5, 120, 3, 1])
    covered = torch.tensor([0, 1, 0, 1, 1, 1, 1, 1])
    labels = torch.tensor([0, 1, 1, 2, 0, 2, -1, 200])                    # the last two do not count
    rec = CF.summarize(size, covered, labels, 3, 200)
    assert rec["images"] == 8 and rec["rows"] == 6 and rec["coverage"] == 4 / 6 and rec["mean_size"] == 133 / 8 and rec["empty"] == 1
    assert rec["median_size"] == 1 and rec["size_quantiles"] == {"0.5": 1, "0.9": 120, "0.99": 120, "max": 120} and rec["singleton_share"] == 3 / 8
    assert rec["top1"] == 50.0 and rec["class_coverage_min"] == 0.5 and abs(rec["class_coverage_mean"] - (0.5 + 0.5 + 1.0) / 3) < 1e-15
    assert rec["size_stratified"] == [dict(lo=0, hi=1, rows=3, coverage=1 / 3), dict(lo=2, hi=3, rows=1, coverage=1.0), dict(lo=4, hi=6, rows=1, coverage=1.0),
                                      dict(lo=7, hi=10, rows=0, coverage=None), dict(lo=11, hi=100, rows=0, coverage=None),
                                      dict(lo=101, hi=None, rows=1, coverage=1.0)]
    json.dumps(rec)


def test_parser_surface():
    p = CF.build_parser()
    sub = next(a for a in p._actions if a.dest == "cmd")
    assert sorted(sub.choices) == ["fit", "score"]
    opts = lambda q: sorted(o for a in q._actions for o in a.option_strings if o not in ("-h", "--help"))
    assert opts(sub.choices["fit"]) == sorted(["--bank", "--alpha", "--method", "--randomized", "--seed", "--lam", "--k_reg", "--temperature", "--output"])
    assert opts(sub.choices["score"]) == sorted(["--bank", "--calibration", "--sets_output", "--classes"])
    a = p.parse_args(["fit", "--bank", "b", "--alpha", "0.1", "--output", "o"])
    assert (a.method, a.randomized, a.seed, a.lam, a.k_reg, a.temperature, a.alpha) == ("aps", 1, 0, 0.01, 5, 1.0, "0.1")
    s = p.parse_args(["score", "--bank", "b", "--calibration", "c"])
    assert s.sets_output is None and s.classes is None
    for bad in (["--alpha", "1"], ["--alpha", "0"], ["--alpha", "0.1", "--method", "top"], ["--alpha", "0.1", "--temperature", "0"],
                ["--alpha", "0.1", "--lam", "-1"], ["--alpha", "0.1", "--k_reg", "-1"], ["--alpha", "0.1", "--randomized", "2"], []):
        with pytest.raises(SystemExit):
            p.parse_args(["fit", "--bank", "b", "--output", "o"] + bad)


def test_refusals():
    z, y = (torch.from_numpy(t) for t in CR.synthetic_bank(20, 6, 4))
    for kw in (dict(method="top"), dict(temperature=0.0), dict(temperature=float("nan")), dict(lam=-0.1), dict(k_reg=-1)):
        with pytest.raises(ValueError):
            CF.reference_scores(z, y, 6, **{"method": "raps", **kw})
        with pytest.raises(ValueError):
            CF.fit_conformal(z, y, 6, "0.1", **{"scorer": CF.reference_scores, **kw})
    with pytest.raises(ValueError):
        CF.reference_sets(z, float("nan"), y, 6)
    with pytest.raises(ValueError):
        CF.reference_class_scores(z, 6, "aps", torch.zeros(19))
    cal = dict(version=1, **CF.fit_conformal(z, y, 6, "0.2", scorer=CF.reference_scores), data_classes=6, num_classes=6, meta={})
    bank = CC.make_logits_bank(z, y, 6, **META)
    CF.evaluate(bank, cal, setter=CF.reference_sets)
    for key, v in (("data_classes", 5), ("num_classes", 8), ("version", 2), ("qhat", float("nan")), ("method", "top")):
        with pytest.raises(ValueError):
            CF.evaluate(bank, {**cal, key: v}, setter=CF.reference_sets)
    with pytest.raises(ValueError):
        CF.evaluate(bank, {k: v for k, v in cal.items() if k != "k_reg"}, setter=CF.reference_sets)
    with pytest.raises(ValueError, match="feature bank"):
        CF.evaluate(dict(features=z, labels=y, data_classes=6, meta={}), cal, setter=CF.reference_sets)


@pytest.mark.parametrize("method", CF.METHODS)
def test_commands_end_to_end_on_the_cpu_evaluator(tmp_path, capsys, method):
    z, y = (torch.from_numpy(t) for t in CR.synthetic_bank(700, 10, 9))
    zp = torch.full((700, 16), float("nan"))
    zp[:, :10] = z                                                        # a head of 16 columns of which 10 are classes
    y[3], y[650] = -1, 12
    cal_bank, test_bank = str(tmp_path / "cal.pt"), str(tmp_path / "test.pt")
    torch.save(CC.make_logits_bank(zp[:400], y[:400], 10, **META), cal_bank)
    torch.save(CC.make_logits_bank(zp[400:], y[400:], 10, **META), test_bank)
    out = str(tmp_path / "conformal.json")
    p = CF.build_parser()
    cal = CF.fit_command(p.parse_args(["fit", "--bank", cal_bank, "--alpha", "0.1", "--method", method, "--seed", "3", "--output", out]), scorer=CF.reference_scores)
    assert tuple(cal) == CF.FILE_KEYS and json.load(open(out)) == cal
    assert (cal["version"], cal["method"], cal["alpha"], cal["rows"], cal["k"], cal["seed"], cal["data_classes"], cal["num_classes"]) == \
        (1, method, 0.1, 399, 360, 3, 10, 16)
    assert cal["randomized"] == (method != "lac") and cal["lam"] == 0.01 and cal["k_reg"] == 5 and cal["temperature"] == 1.0 and cal["meta"] == META
    u = CF.draw_u(400, 3).numpy() if cal["randomized"] else None
    assert abs(cal["qhat"] - CR.qhat_of(CR.label_scores(zp[:400].numpy(), y[:400].numpy(), 10, method, u, 1.0, 0.01, 5)[0], "0.1")) <= 1e-14
    names = tmp_path / "names.txt"
    names.write_text("\n".join(f"class{c}" for c in range(10)))
    sets_file = str(tmp_path / "sets.jsonl")
    rec = CF.score_command(p.parse_args(["score", "--bank", test_bank, "--calibration", out, "--sets_output", sets_file, "--classes", str(names)]),
                           setter=CF.reference_sets)
    json.dumps(rec)
    assert set(rec) >= {"coverage", "mean_size", "median_size", "size_quantiles", "empty", "singleton_share", "top1", "class_coverage_min",
                        "class_coverage_mean", "size_stratified"}
    assert rec["images"] == 300 and rec["rows"] == 299 and sorted(rec["size_quantiles"]) == ["0.5", "0.9", "0.99", "max"]
    assert [(s["lo"], s["hi"]) for s in rec["size_stratified"]] == [(0, 1), (2, 3), (4, 6), (7, 10), (11, 100), (101, None)]
    assert sum(s["rows"] for s in rec["size_stratified"]) == 299
    u = CF.draw_u(300, 4).numpy() if cal["randomized"] else None
    inset = CR.sets(zp[400:].numpy(), cal["qhat"], 10, method, u, 1.0, 0.01, 5)
    lines = [json.loads(l) for l in open(sets_file)]
    assert len(lines) == 300
    for i, l in enumerate(lines):
        lab = int(y[400 + i])
        assert l == dict(row=i, label=lab, size=int(inset[i].sum()), covered=bool(0 <= lab < 10 and inset[i, lab]),
                         set=[f"class{c}" for c in np.flatnonzero(inset[i])])
    keep = (y[400:] >= 0) & (y[400:] < 10)
    assert abs(rec["coverage"] - np.mean([l["covered"] for l, k in zip(lines, keep.tolist()) if k])) < 1e-12
    assert abs(rec["top1"] - 100.0 * float((z[400:].argmax(1)[keep] == y[400:][keep]).double().mean())) < 1e-9
    # a bank of another label set is refused by name
    other = str(tmp_path / "other.pt")
    torch.save(CC.make_logits_bank(zp[400:], y[400:].clamp(0, 8), 9, **META), other)
    with pytest.raises(ValueError, match="data_classes"):
        CF.score_command(p.parse_args(["score", "--bank", other, "--calibration", out]), setter=CF.reference_sets)
    # main prints the record as one line (fit needs a device: not here)
    assert "conformal" in (CF.__doc__ or "")
