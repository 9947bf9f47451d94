"""CPU: the written spec of the linear probe (uvc_amd/compact_probe.py) -- the objective against autograd, the fit through an injected
evaluator, the sweep's order, the bank rules, the file and the command line."""
import copy

import pytest
import torch

import knn_ref as KR
import probe_ref as PR
from uvc_amd import compact as CP
from uvc_amd import compact_probe as PB
from uvc_amd import compact_transfer as CT


# ---- the objective --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("n,D,C,l2", [(50, 8, 3, 1e-2), (200, 16, 10, 0.0), (7, 4, 1, 1e-1)])
def test_reference_objective_against_autograd(n, D, C, l2, bias):
    X, y = PR.gaussian_classes(n, D, C, seed=n)
    g = torch.Generator().manual_seed(1)
    W = torch.randn(C, D, generator=g, dtype=torch.float64)
    b = torch.randn(C, generator=g, dtype=torch.float64) if bias else None
    F, dW, db, hits = PB.reference_objective(W, b, X, y, l2)
    wF, wdW, wdb = PR.autograd_objective(W, b, X, y, l2)
    assert abs(F - wF) <= 1e-12 * max(1.0, abs(wF))
    assert float((dW - wdW).abs().max()) <= 1e-12 * max(1.0, float(wdW.abs().max()))
    assert (db is None) == (not bias)
    if bias:
        assert float((db - wdb).abs().max()) <= 1e-12
    z = X @ W.T + (0 if b is None else b)
    assert hits == int((z.argmax(1) == y).sum())


def test_uncounted_labels_change_nothing_but_m():
    X, y = PR.gaussian_classes(60, 8, 4, seed=3)
    g = torch.Generator().manual_seed(2)
    W, b = torch.randn(4, 8, generator=g, dtype=torch.float64), torch.randn(4, generator=g, dtype=torch.float64)
    base = PB.reference_objective(W, b, X, y, 1e-2)
    extra_X = torch.cat([X, torch.randn(5, 8, generator=g, dtype=torch.float64)])
    extra_y = torch.cat([y, torch.tensor([-1, 4, -7, 100, 4])])
    more = PB.reference_objective(W, b, extra_X, extra_y, 1e-2)
    assert more[0] == base[0] and torch.equal(more[1], base[1]) and torch.equal(more[2], base[2]) and more[3] == base[3]
    none = PB.reference_objective(W, b, extra_X[60:], extra_y[60:], 1e-2)           # m = 0: the l2 terms alone
    assert none[0] == 0.5 * 1e-2 * float((W * W).sum()) and torch.equal(none[1], 1e-2 * W) and not none[2].any() and none[3] == 0


def test_one_class_and_tied_rows():
    X, _ = PR.gaussian_classes(9, 4, 2, seed=5)
    W, b = torch.randn(1, 4, dtype=torch.float64), torch.randn(1, dtype=torch.float64)
    F, dW, db, hits = PB.reference_objective(W, b, X, torch.zeros(9, dtype=torch.int64), 0.0)
    assert F == 0.0 and not dW.any() and not db.any() and hits == 9
    # rows of equal logits: the first maximum is class 0, so label 0 hits and label 2 does not
    W3 = torch.zeros(3, 4, dtype=torch.float64)
    y = torch.tensor([0, 2, 0, 1, 2, 0, 0, 1, 2])
    assert PB.reference_objective(W3, None, X, y, 0.0)[3] == int((y == 0).sum())
    b3 = torch.tensor([0.0, 1.0, 1.0], dtype=torch.float64)                          # classes 1 and 2 tie: 1 is the first maximum
    assert PB.reference_objective(W3, b3, X, y, 0.0)[3] == int((y == 1).sum())


# ---- the fit ---------------------------------------------------------------------------------------------------------------------------
def test_fit_probe_reaches_the_unique_optimum():
    X, y = PR.gaussian_classes(600, 32, 5, seed=0)
    tol = 1e-7
    a = PB.fit_probe(X, y, 5, 1e-3, evaluator=PB.reference_objective, tol_grad=tol)
    assert a["grad_inf"] <= tol and a["iterations"] < 1000 and a["rows"] == 600
    assert a["W"].dtype == torch.float64 and tuple(a["W"].shape) == (5, 32) and tuple(a["b"].shape) == (5,)
    F, dW, db, hits = PB.reference_objective(a["W"], a["b"], X, y, 1e-3)
    assert F == a["F"] and max(float(dW.abs().max()), float(db.abs().max())) == a["grad_inf"] and a["top1"] == 100.0 * hits / 600
    assert 30.0 < a["top1"] < 100.0                                                   # the classes overlap: nothing here is separable
    g = torch.Generator().manual_seed(9)
    start = (torch.randn(5, 32, generator=g, dtype=torch.float64), torch.randn(5, generator=g, dtype=torch.float64))
    c = PB.fit_probe(X, y, 5, 1e-3, evaluator=PB.reference_objective, tol_grad=tol, init=start)
    assert c["grad_inf"] <= tol
    assert abs(c["F"] - a["F"]) <= 1e-9 * abs(a["F"])                                 # strongly convex: one optimum
    nb = PB.fit_probe(X, y, 5, 1e-3, evaluator=PB.reference_objective, tol_grad=tol, bias=False)
    assert nb["b"] is None and nb["grad_inf"] <= tol and nb["F"] >= a["F"] - 1e-12


def test_fit_probe_counts_evaluations_and_ignores_foreign_labels():
    X, y = PR.gaussian_classes(120, 8, 3, seed=4)
    calls = []

    def ev(W, b, X_, y_, l2):
        calls.append(W.clone())
        return PB.reference_objective(W, b, X_, y_, l2)
    y2 = y.clone()
    y2[:5] = -1
    r = PB.fit_probe(X, y2, 3, 1e-2, evaluator=ev, tol_grad=1e-8)
    assert r["evaluations"] == len(calls) and r["rows"] == 115 and not calls[0].any()
    want = PB.fit_probe(X[5:], y[5:], 3, 1e-2, evaluator=PB.reference_objective, tol_grad=1e-8)
    assert abs(r["F"] - want["F"]) <= 1e-12


def test_sweep_order_warm_start_and_tie_rule():
    X, y = PR.gaussian_classes(200, 8, 3, seed=6)
    Xv, yv = PR.gaussian_classes(80, 8, 3, seed=6)
    first_calls, seen_l2 = [], []

    def ev(W, b, X_, y_, l2):
        if not seen_l2 or seen_l2[-1] != l2:
            seen_l2.append(l2)
            first_calls.append((W.clone(), b.clone()))
        return PB.reference_objective(W, b, X_, y_, l2)
    fits = []

    def scorer(W, b, f, l, c):
        fits.append((W.clone(), b.clone()))
        assert f is Xv and l is yv and c == 3
        return [50.0, 70.0, 70.0, 60.0][len(fits) - 1]
    records, best = PB.sweep((X, y), (Xv, yv), [1e-4, 1e-1, 1e-3, 1e-2], 3, evaluator=ev, scorer=scorer, tol_grad=1e-8)
    assert [r["l2"] for r in records] == [1e-1, 1e-2, 1e-3, 1e-4] == seen_l2      # one fit at a time, from the largest value down
    assert not first_calls[0][0].any() and not first_calls[0][1].any()               # the first starts from zeros
    for i in range(1, 4):                                                            # every later one where the one before ended
        assert torch.equal(first_calls[i][0], fits[i - 1][0]) and torch.equal(first_calls[i][1], fits[i - 1][1])
    assert [r["val_top1"] for r in records] == [50.0, 70.0, 70.0, 60.0]
    assert best["l2"] == 1e-2 and best["val_top1"] == 70.0 and torch.equal(best["W"], fits[1][0])      # a tie: the larger l2
    assert set(records[0]) == {"l2", "F", "train_top1", "val_top1", "iterations", "evaluations"}
    assert records[0]["F"] > records[-1]["F"]
    with pytest.raises(ValueError):
        PB.sweep((X, y), (Xv, yv), [], 3, evaluator=ev, scorer=scorer)


def test_default_chunk_rows():
    from uvc_amd import ops
    assert ops.probe_chunk_rows(1281167, 1000, ops.UVC_BF16) == 262144          # the measured default
    assert ops.probe_chunk_rows(50000, 100, ops.UVC_BF16) == 50000 and ops.probe_chunk_rows(5, 10, ops.UVC_F32) == 5
    rows = ops.probe_chunk_rows(10 ** 6, 65536, ops.UVC_F32)                    # a wide head: at most 2 GiB of logits plus G
    assert rows % 64 == 0 and rows * 65536 * 8 <= 2 << 30 < (rows + 64) * 65536 * 8


def test_l2_grid():
    assert PB.l2_grid(1, 1e-6, 1e-1) == [1e-1]
    g = PB.l2_grid(6, 1e-6, 1e-1)
    assert len(g) == 6 and all(abs(v / w - 1) < 1e-12 for v, w in zip(g, [1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6]))
    with pytest.raises(ValueError):
        PB.l2_grid(3, 0.0, 1.0)


# ---- banks ----------------------------------------------------------------------------------------------------------------------------
def test_bank_rules():
    ex, _ = KR.export_of("stage2_micro_deit")
    D = ex["cfg"]["embed_dim"]
    f = torch.randn(12, D, generator=torch.Generator().manual_seed(0))
    y = torch.arange(12) % 3
    raw = CT.make_bank(f, y, 3, dataset="cifar10", split="train", precision="fp32")
    assert "normalized" not in raw and "normalized" not in raw["meta"] and PB.bank_is_normalized(raw)
    raw["normalized"] = False
    assert PB.check_probe_bank(raw, ex, bias=True) is raw and PB.check_probe_bank(raw, ex, bias=False) is raw
    for normed in (CT.make_bank(f, y, 3), dict(raw, normalized=True)):                # without the key, or with it true
        with pytest.raises(ValueError, match="normalized"):
            PB.check_probe_bank(normed, ex, bias=True)
        assert PB.check_probe_bank(normed, ex, bias=False) is normed
    other = CT.make_bank(torch.randn(4, D + 8), torch.arange(4) % 3, 3)
    other["normalized"] = False
    with pytest.raises(ValueError, match="embed_dim"):
        PB.check_probe_bank(other, ex, bias=True)
    with pytest.raises(ValueError, match="data_classes"):
        PB.check_probe_bank(raw, ex, bias=True, data_classes=10)


def test_split_bank_holds_out_the_permutations_last_rows():
    bank = CT.make_bank(torch.arange(40.0).reshape(10, 4), torch.arange(10), 10)
    (tf, ty), (vf, vy) = PB.split_bank(bank, 0.35, seed=3)
    perm = torch.randperm(10, generator=torch.Generator().manual_seed(3))
    assert torch.equal(vy, perm[7:]) and torch.equal(ty, perm[:7]) and torch.equal(vf, bank["features"][perm[7:]]) and len(tf) == 7
    with pytest.raises(ValueError):
        PB.split_bank(bank, 0.05, seed=0)


# ---- the file -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stage2_micro_skip", "stage2_micro_deit"])
@pytest.mark.parametrize("classes,width,bias", [(10, 16, True), (3, 8, True), (8, 8, False)])
def test_probe_head_writes_the_classifier(name, classes, width, bias):
    ex, x = KR.export_of(name)
    before = copy.deepcopy(ex)
    D = ex["cfg"]["embed_dim"]
    g = torch.Generator().manual_seed(classes)
    W = torch.randn(classes, D, generator=g, dtype=torch.float64)
    b = torch.randn(classes, generator=g, dtype=torch.float64) if bias else None
    out = PB.probe_head(ex, W, b, classes)
    assert CP.check_export(out) is out and out["cfg"]["num_classes"] == width
    zero, _ = CT.rehead(ex, dict(features=torch.empty(0, D), labels=torch.empty(0, dtype=torch.int64), data_classes=classes, meta=dict(embed_dim=D)), init="zero")
    for k, v in before["state_dict"].items():
        assert torch.equal(ex["state_dict"][k], v)                                   # the input is untouched
        if not k.startswith("head"):
            assert torch.equal(out["state_dict"][k].view(torch.int32), v.view(torch.int32)) and out["state_dict"][k].dtype == v.dtype
    assert set(out["state_dict"]) == set(zero["state_dict"]) and out["blocks"] == zero["blocks"] and out["cfg"] == zero["cfg"]
    hw, hb = out["state_dict"]["head.weight"], out["state_dict"]["head.bias"]
    assert hw.dtype == zero["state_dict"]["head.weight"].dtype and tuple(hw.shape) == (width, D)
    assert torch.equal(hw[:classes], W.to(hw.dtype)) and not hw[classes:].any()
    assert torch.equal(hb[:classes], b.to(hb.dtype) if bias else torch.zeros(classes, dtype=hb.dtype))
    assert bool((hb[classes:] == PB.PAD_BIAS).all()) and PB.PAD_BIAS == -1e4
    if ex["cfg"]["enable_dist"]:
        assert torch.equal(out["state_dict"]["head_dist.weight"], hw) and torch.equal(out["state_dict"]["head_dist.bias"], hb)
    # the file's logits are X W^T + b on the model's own raw features, and no padding logit wins
    f = CT.reference_features(ex, x.double(), normalize=False)
    got = CP.reference_forward(out, x.double())
    want = f @ hw.double()[:classes].T + hb.double()[:classes]
    assert float((got[:, :classes] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert bool((got[:, classes:] == PB.PAD_BIAS).all()) and bool((got.argmax(1) < classes).all())
    fw, fb = PB.file_head(out, classes)
    assert torch.equal(fw, hw[:classes].float()) and torch.equal(fb, hb[:classes].float())
    with pytest.raises(ValueError):
        PB.probe_head(ex, W[:, :-1], b, classes)


def test_file_head_refuses_two_different_heads():
    ex, _ = KR.export_of("stage2_micro_deit")
    assert ex["cfg"]["enable_dist"] and not torch.equal(ex["state_dict"]["head.weight"], ex["state_dict"]["head_dist.weight"])
    with pytest.raises(ValueError, match="one classifier"):
        PB.file_head(ex, 3)


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def test_parser():
    p = PB.build_parser()
    assert sorted(p._subparsers._group_actions[0].choices) == ["embed", "fit", "score"]
    e = p.parse_args(["embed", "--compact", "F", "--output", "raw.pt", "--dataset", "cifar10", "--data_dir", "D"])
    assert (e.split, e.precision, e.eval_batch_size, e.num_workers, e.interpolation, e.crop_pct, e.packed_dir, e.resident) == \
        ("train", "bf16", 256, 8, "bilinear", None, None, 0)
    f = p.parse_args(["fit", "--compact", "F", "--bank", "b.pt", "--output", "G"])
    assert (f.val_bank, f.val_fraction, f.seed, f.l2, f.l2_grid, f.l2_min, f.l2_max, f.bias, f.max_iter, f.refit, f.precision, f.chunk_rows) == \
        (None, None, 0, None, None, 1e-6, 1e-1, 1, 1000, 1, "bf16", None)
    f = p.parse_args(["fit", "--compact", "F", "--bank", "b.pt", "--output", "G", "--l2", "1e-2", "1e-3", "--val_fraction", "0.1", "--bias", "0"])
    assert f.l2 == [1e-2, 1e-3] and f.val_fraction == 0.1 and f.bias == 0
    s = p.parse_args(["score", "--compact", "G", "--bank", "b.pt"])
    assert s.precision == "bf16" and s.bank == "b.pt"
    for bad in (["fit", "--compact", "F", "--bank", "b", "--output", "G", "--val_bank", "v", "--val_fraction", "0.1"],
                ["fit", "--compact", "F", "--bank", "b", "--output", "G", "--l2", "1e-3", "--l2_grid", "4"],
                ["fit", "--compact", "F", "--bank", "b", "--output", "G", "--val_fraction", "1.0"],
                ["fit", "--compact", "F", "--bank", "b"], ["score", "--compact", "G"], ["embed", "--compact", "F"], ["knn", "--compact", "F"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_fit_refuses_a_normalised_bank_before_it_needs_a_device(tmp_path):
    ex, _ = KR.export_of("stage2_micro_skip")
    D = ex["cfg"]["embed_dim"]
    torch.save(ex, tmp_path / "f.pt")
    torch.save(CT.make_bank(torch.randn(6, D), torch.arange(6) % 3, 3), tmp_path / "normed.pt")
    with pytest.raises(ValueError, match="--bias 0"):
        PB.main(["fit", "--compact", str(tmp_path / "f.pt"), "--bank", str(tmp_path / "normed.pt"), "--output", str(tmp_path / "g.pt")])
