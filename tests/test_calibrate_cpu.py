"""CPU: the written spec of calibration (uvc_amd/compact_calibrate.py) -- the objective against autograd, the fold into a file's head, the
solver on the synthetic over-confident bank, the reliability record on a bank whose bins are known, the bank rules and the command line."""
import copy
import json
import math

import pytest
import torch

import calib_ref as CR
from uvc_amd import compact as CP
from uvc_amd import compact_calibrate as CC
from uvc_amd import compact_transfer as CT


# ---- the objective --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", CR.MODES)
@pytest.mark.parametrize("n,C,ld", [(50, 3, 3), (200, 10, 16), (7, 1, 8)])
def test_reference_objective_against_autograd(n, C, ld, mode):
    z, y = CR.case_inputs(n, C, ld, "normal", seed=n)
    scale, shift = CR.case_maps(C, "normal", seed=n)[mode]
    F, ds, dd, hits, m = CC.reference_objective(z, y, scale, shift, C)
    wF, wds, wdd = CR.autograd_objective(z, y, scale, shift, C)
    assert m == int(((y >= 0) & (y < C)).sum())
    assert abs(F - wF) <= 1e-10 * max(1.0, abs(wF))
    assert ds.shape == wds.shape and float((ds - wds).abs().max()) <= 1e-10 * max(1.0, float(wds.abs().max()))
    assert (dd is None) == (shift is None)
    if dd is not None:
        assert float((dd - wdd).abs().max()) <= 1e-10
    zp, yk = CR.mapped(z, y, scale, shift, C)
    assert hits == int((zp.argmax(1) == yk).sum())


def test_uncounted_rows_and_an_empty_bank():
    z, y = CR.case_inputs(40, 5, 8, "normal", seed=1)
    scale, shift = CR.case_maps(5, "normal", seed=1)[("vector", True)]
    keep = (y >= 0) & (y < 5)
    assert int(keep.sum()) == 38
    a, b = CC.reference_objective(z, y, scale, shift, 5), CC.reference_objective(z[keep], y[keep], scale, shift, 5)
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3:] == b[3:]
    F, ds, dd, hits, m = CC.reference_objective(z[:2], torch.tensor([-1, 5]), scale, shift, 5)
    assert (F, hits, m) == (0.0, 0, 0) and not ds.any() and not dd.any() and ds.shape == (5,)
    assert CC.reference_objective(z[:2], torch.tensor([-1, 5]), scale[:1], None, 5)[1].shape == (1,)
    rec = CC.reference_scorer(z[:2], torch.tensor([-1, 5]), scale, shift, 5)
    assert rec["ece"] == rec["nll"] == rec["top1"] == 0.0 and rec["rows"] == 0
    with pytest.raises(ValueError):
        CC.reference_objective(z, y, scale[:3], None, 5)


@pytest.mark.parametrize("Cc,ld", CR.WIDTHS)
def test_the_device_tests_inputs_leave_at_most_one_percent_undecided(Cc, ld):
    """the inputs of tests/test_calibrate_gpu.py, by the reference alone: the rows whose first maximum leads by no more than 2^-20 max |z'|
    (an exact tie is decided by the first-maximum rule) and the rows whose confidence lies within 1e-6 of an interior bin edge"""
    for kind in ("normal", "huge", "ties"):
        for rows in CR.ROWS:
            z, y = CR.case_inputs(rows, Cc, ld, kind, seed=CR.case_seed(rows, Cc))
            maps = CR.case_maps(Cc, kind, seed=CR.case_seed(rows, Cc))
            for mode in CR.MODES:
                lo, hi, undecided = CR.hit_range(z, y, *maps[mode], Cc)
                assert undecided <= CR.CAP * rows and hi - lo <= undecided, (kind, rows, mode, undecided)
            if kind != "ties":
                for i, bins in enumerate((1, 10, 15, 64)):
                    undecided = CR.bin_ranges(z, y, *maps[CR.MODES[(i + rows) % 4]], Cc, bins)[4]
                    assert undecided <= CR.CAP * rows, (kind, rows, bins, undecided)


# ---- the fold ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", CC.METHODS)
@pytest.mark.parametrize("name", ["plain", "distilled", "probed"])
def test_calibrated_head_folds_the_map_into_the_file(name, method):
    ex, x, classes = CR.micro_exports()[name]
    before = copy.deepcopy(ex)
    g = torch.Generator().manual_seed(classes)
    a = 0.5 + torch.rand(classes if method == "vector" else 1, generator=g, dtype=torch.float64)
    d = torch.randn(classes, generator=g, dtype=torch.float64) if method == "vector" else None
    out = CC.calibrated_head(ex, a, d, classes)
    assert CP.check_export(out) is out and out["cfg"] == ex["cfg"] and out["blocks"] == ex["blocks"] and set(out["state_dict"]) == set(ex["state_dict"])
    bits = lambda t: t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)
    for k, v in before["state_dict"].items():
        assert torch.equal(ex["state_dict"][k], v)                                   # the input is untouched
        got = out["state_dict"][k]
        assert got.dtype == v.dtype and got.shape == v.shape
        if k.startswith("head"):
            assert torch.equal(bits(got[classes:]), bits(v[classes:]))               # the padding rows, a probed file's PAD_BIAS among them
        else:
            assert torch.equal(bits(got), bits(v))
    xd = x.double()
    want, got = CP.reference_logits(ex, xd), CP.reference_logits(out, xd)
    af, df = a.expand(classes), (torch.zeros(classes, dtype=torch.float64) if d is None else d)
    for w, o in zip(want, got):
        top = float(w[:, :classes].abs().max())
        assert float((o[:, :classes] - (af * w[:, :classes] + df)).abs().max()) <= 1e-5 * max(top, float((af * w[:, :classes] + df).abs().max()))
        assert torch.equal(o[:, classes:], w[:, classes:])
    mean = CP.reference_forward(out, xd)[:, :classes]
    assert float((mean - (af * CP.reference_forward(ex, xd)[:, :classes] + df)).abs().max()) <= 1e-5 * float(mean.abs().max())
    with pytest.raises(ValueError):
        CC.calibrated_head(ex, torch.ones(classes + 1), None, classes)
    with pytest.raises(ValueError):
        CC.calibrated_head(ex, torch.ones(1), None, ex["cfg"]["num_classes"] + 1)


# ---- the solver -------------------------------------------------------------------------------------------------------------------------
def test_temperature_recovers_the_factor_of_the_synthetic_bank():
    Z, y = CR.synthetic_bank()
    opt = CR.optimum("temperature")
    assert abs(opt["temperature"] / 2.5 - 1) <= 0.05 and opt["shift"] is None and tuple(opt["scale"].shape) == (1,)
    before = CC.reference_scorer(Z, y, torch.ones(1), None, 10)
    after = CC.reference_scorer(Z, y, opt["scale"], None, 10)
    assert after["top1"] == before["top1"] == opt["top1"] and after["ece"] < before["ece"] and after["nll"] < before["nll"]
    assert abs(after["nll"] - opt["F"]) <= 1e-12
    # the float32 arm of the device test, and a start away from s = 1
    low = CC.fit_calibration(Z, y, 10, "temperature", evaluator=CR.Float32Evaluator())
    assert low["scale"].dtype == torch.float32 and abs(low["temperature"] / opt["temperature"] - 1) <= 1e-4
    far = CC.fit_calibration(Z, y, 10, "temperature", evaluator=CC.reference_objective, init=(torch.tensor([3.0]), None), tol_grad=1e-10)
    assert abs(far["temperature"] / opt["temperature"] - 1) <= 1e-6


def test_vector_scaling_lowers_the_objective_further():
    Z, y = CR.synthetic_bank()
    t, v = CR.optimum("temperature"), CR.optimum("vector")
    assert v["F"] < t["F"] and tuple(v["scale"].shape) == tuple(v["shift"].shape) == (10,) and "temperature" not in v
    assert bool((v["scale"] > 0).all()) and float((1 / v["scale"] / 2.5 - 1).abs().max()) <= 0.2
    F, ds, dd, hits, m = CC.reference_objective(Z, y, v["scale"], v["shift"], 10)
    assert F == v["F"] and max(float(ds.abs().max()), float(dd.abs().max())) == v["grad_inf"] <= 1e-10 and m == v["rows"] == 4000
    with pytest.raises(ValueError):
        CC.fit_calibration(Z, y, 10, "histogram", evaluator=CC.reference_objective)


# ---- reliability ------------------------------------------------------------------------------------------------------------------------
def test_reliability_on_a_bank_whose_bins_are_known():
    logit = lambda p: math.log(p / (1 - p))
    # two classes: the confidence of [l, 0] is sigmoid(|l|); 1000 gives exactly 1.0, [0, 0] exactly 0.5 with class 0 its first maximum
    rows = [(logit(0.55), 0), (logit(0.62), 1), (-logit(0.95), 1), (1000.0, 0), (0.0, 1), (0.0, 0), (logit(0.57), 7)]
    z = torch.tensor([[l, 0.0] for l, _ in rows], dtype=torch.float64)
    y = torch.tensor([t for _, t in rows])
    raw = CC.reference_reliability(z, y, torch.ones(1), None, 2, bins=10)
    assert raw["m"] == 6 and raw["hits"] == 4
    assert raw["bin_count"].tolist() == [0, 0, 0, 0, 2, 1, 1, 0, 0, 2] and raw["bin_hit"].tolist() == [0, 0, 0, 0, 1, 1, 0, 0, 0, 2]
    rec = CC.reliability(**raw)
    conf = {4: 0.5, 5: 0.55, 6: 0.62, 9: (0.95 + 1.0) / 2}
    acc = {4: 0.5, 5: 1.0, 6: 0.0, 9: 1.0}
    n = {4: 2, 5: 1, 6: 1, 9: 2}
    assert abs(rec["ece"] - sum(n[j] / 6 * abs(acc[j] - conf[j]) for j in n)) <= 1e-12 and abs(rec["mce"] - 0.62) <= 1e-12
    assert rec["bin_count"] == raw["bin_count"].tolist() and abs(rec["bin_conf"][9] - conf[9]) <= 1e-12 and rec["bin_acc"][6] == 0.0 and rec["bin_conf"][0] == 0.0
    assert abs(rec["top1"] - 100 * 4 / 6) <= 1e-12 and rec["rows"] == 6
    p_y = [0.55, 0.38, 0.95, 1.0, 0.5, 0.5]
    assert abs(rec["nll"] - sum(-math.log(p) for p in p_y) / 6) <= 1e-12
    assert abs(rec["brier"] - sum(2 * (1 - p) ** 2 for p in p_y) / 6) <= 1e-12
    one = CC.reliability(**CC.reference_reliability(z, y, torch.ones(1), None, 2, bins=1))
    assert one["bin_count"] == [6] and abs(one["ece"] - abs(4 / 6 - (0.55 + 0.62 + 0.95 + 1.0 + 0.5 + 0.5) / 6)) <= 1e-12 and abs(one["mce"] - one["ece"]) <= 1e-12
    # a temperature moves the confidences, not the predictions
    cool = CC.reference_reliability(z, y, torch.tensor([0.5]), None, 2, bins=10)
    assert cool["hits"] == 4 and cool["bin_count"].tolist() != raw["bin_count"].tolist()
    for bad in (0, 65):
        with pytest.raises(ValueError):
            CC.reference_reliability(z, y, torch.ones(1), None, 2, bins=bad)


# ---- banks ------------------------------------------------------------------------------------------------------------------------------
def test_bank_rules(tmp_path):
    ex, _, _ = CR.micro_exports()["plain"]
    nc = ex["cfg"]["num_classes"]
    bank = CC.make_logits_bank(torch.randn(6, nc), torch.arange(6) % 3, 3, dataset="cifar10", split="test", precision="fp32", embed_dim=5)
    assert set(bank) == set(CC.BANK_KEYS) and bank["num_classes"] == nc and "embed_dim" not in bank["meta"]
    assert set(bank["meta"]) == set(CT.META_KEYS) - {"embed_dim"} and bank["logits"].dtype == torch.float32 and bank["labels"].dtype == torch.int64
    assert CC.check_logits_bank(bank, ex, 3) is bank
    torch.save(bank, tmp_path / "b.pt")
    assert torch.equal(CC.load_logits_bank(tmp_path / "b.pt")["logits"], bank["logits"])
    with pytest.raises(ValueError, match="data_classes"):
        CC.check_logits_bank(bank, ex, 10)
    with pytest.raises(ValueError, match="num_classes"):
        CC.check_logits_bank(CC.make_logits_bank(torch.randn(6, nc + 8), torch.arange(6) % 3, 3), ex)
    with pytest.raises(ValueError, match="data_classes"):
        CC.check_logits_bank(dict(bank, data_classes=nc + 1))
    feats = CT.make_bank(torch.randn(6, 8), torch.arange(6) % 3, 3)
    with pytest.raises(ValueError, match="a feature bank"):
        CC.check_logits_bank(feats)
    torch.save(feats, tmp_path / "f.pt")
    with pytest.raises(ValueError, match="f.pt"):
        CC.load_logits_bank(tmp_path / "f.pt")
    with pytest.raises(ValueError, match="not a logits bank"):
        CC.check_logits_bank([1, 2])
    with pytest.raises(ValueError, match="one label per row"):
        CC.check_logits_bank(dict(bank, labels=bank["labels"][:-1]))
    with pytest.raises(ValueError):
        CC.make_logits_bank(torch.randn(6, nc), torch.arange(5), 3)


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def test_parser():
    p = CC.build_parser()
    assert sorted(p._subparsers._group_actions[0].choices) == ["fit", "logits", "score"]
    l = p.parse_args(["logits", "--compact", "F", "--output", "z.pt", "--dataset", "cifar10", "--data_dir", "D"])
    assert (l.split, l.precision, l.eval_batch_size, l.num_workers, l.interpolation, l.crop_pct, l.packed_dir, l.resident) == \
        ("train", "bf16", 256, 8, "bilinear", None, None, 0)
    f = p.parse_args(["fit", "--compact", "F", "--bank", "b.pt", "--output", "G"])
    assert (f.method, f.val_bank, f.val_fraction, f.seed, f.bins, f.max_iter, f.chunk_rows) == ("temperature", None, None, 0, 15, 500, None)
    f = p.parse_args(["fit", "--compact", "F", "--bank", "b.pt", "--output", "G", "--method", "vector", "--val_fraction", "0.1", "--bins", "10"])
    assert (f.method, f.val_fraction, f.bins) == ("vector", 0.1, 10)
    s = p.parse_args(["score", "--bank", "b.pt"])
    assert s.bins == 15 and s.bank == "b.pt" and not hasattr(s, "compact")
    for bad in (["fit", "--compact", "F", "--bank", "b", "--output", "G", "--val_bank", "v", "--val_fraction", "0.1"],
                ["fit", "--compact", "F", "--bank", "b", "--output", "G", "--method", "isotonic"],
                ["fit", "--compact", "F", "--bank", "b", "--output", "G", "--bins", "65"],
                ["fit", "--compact", "F", "--bank", "b", "--output", "G", "--val_fraction", "1.0"],
                ["fit", "--compact", "F", "--bank", "b"], ["fit", "--bank", "b", "--output", "G"], ["score"], ["score", "--bank", "b", "--bins", "0"],
                ["logits", "--compact", "F"], ["embed", "--compact", "F", "--output", "o"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


@pytest.mark.parametrize("method", CC.METHODS)
def test_fit_then_score_on_banks_with_the_cpu_evaluator(tmp_path, method):
    ex, _, _ = CR.micro_exports()["probed"]
    nc = ex["cfg"]["num_classes"]
    Z, y = CR.synthetic_bank()
    wide = torch.full((Z.shape[0], nc), -50.0)
    wide[:, :10] = Z
    torch.save(ex, tmp_path / "f.pt")
    torch.save(CC.make_logits_bank(wide, y, 10, dataset="cifar10", split="test"), tmp_path / "z.pt")
    args = CC.build_parser().parse_args(["fit", "--compact", str(tmp_path / "f.pt"), "--bank", str(tmp_path / "z.pt"), "--method", method,
                                         "--val_fraction", "0.25", "--seed", "3", "--output", str(tmp_path / "g.pt")])
    line, res = CC.fit_command(args, evaluator=CC.reference_objective, scorer=CC.reference_scorer)
    json.dumps(line)
    assert set(line) >= {"output", "method", "data_classes", "num_classes", "rows", "evaluations", "seconds", "before", "after", "blocks", "params", "macs_compact"}
    assert ("temperature" in line) == (method == "temperature") and (line["data_classes"], line["num_classes"], line["rows"]) == (10, nc, 3000)
    for part in ("fit", "val"):
        assert line["after"][part]["ece"] < line["before"][part]["ece"] and line["after"][part]["nll"] < line["before"][part]["nll"]
        assert set(line["after"][part]) == {"ece", "mce", "nll", "brier", "top1", "rows", "bin_count", "bin_conf", "bin_acc"}
    assert line["before"]["val"]["rows"] == 1000 and len(line["after"]["fit"]["bin_count"]) == 15
    if method == "temperature":
        assert abs(line["temperature"] / 2.5 - 1) <= 0.05 and line["after"]["fit"]["top1"] == line["before"]["fit"]["top1"]
    # the written file is the fold of the fitted map, and a bank of ITS logits scores as "after" says
    out = CP.load_compact(tmp_path / "g.pt")
    want = CC.calibrated_head(ex, res["scale"], res["shift"], 10)
    assert all(torch.equal(out["state_dict"][k], v) for k, v in want["state_dict"].items())
    a = res["scale"].double().expand(10)
    d = torch.zeros(10, dtype=torch.float64) if res["shift"] is None else res["shift"].double()
    fit_rows = torch.randperm(4000, generator=torch.Generator().manual_seed(3))[:3000]
    mapped = wide[fit_rows].double()
    mapped[:, :10] = mapped[:, :10] * a + d
    torch.save(CC.make_logits_bank(mapped, y[fit_rows], 10), tmp_path / "after.pt")
    score = CC.score_command(CC.build_parser().parse_args(["score", "--bank", str(tmp_path / "after.pt")]), scorer=CC.reference_scorer)
    assert (score["images"], score["data_classes"], score["num_classes"], score["bins"]) == (3000, 10, nc, 15)
    for k in ("ece", "nll", "brier"):
        assert abs(score[k] - line["after"]["fit"][k]) <= 1e-5 * max(1.0, line["after"]["fit"][k])       # (the bank stores float32 logits)
    assert score["top1"] == line["after"]["fit"]["top1"]
    # a bank of another file's width is refused by name before anything is fitted
    torch.save(CC.make_logits_bank(Z, y, 10), tmp_path / "narrow.pt")
    args.bank = str(tmp_path / "narrow.pt")
    if nc != 10:
        with pytest.raises(ValueError, match="num_classes"):
            CC.fit_command(args, evaluator=CC.reference_objective, scorer=CC.reference_scorer)
