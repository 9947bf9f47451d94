"""CPU: the written specs of python -m uvc_amd.compact_ood -- metrics, the Gaussian fit, the augmentation identity, the files, the refusals
and the parser (no device)."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import ood_ref as OR
from uvc_amd import _lib as L
from uvc_amd import compact_ood as OD
from uvc_amd import compact_transfer as CT


# ---- metrics ------------------------------------------------------------------------------------------------------------------------
def test_auroc_counts_ties_as_half():
    m = OD.reference_metrics(OR.TIE_ID, OR.TIE_OOD)
    assert m["auroc"] == pytest.approx(13 / 24, abs=1e-15)
    assert m["id_mean"] == pytest.approx(14 / 6) and m["ood_mean"] == 2.0
    pairs = sum((a > b) + 0.5 * (a == b) for a in OR.TIE_ID for b in OR.TIE_OOD)
    assert pairs == 13.0


@pytest.mark.parametrize("si,so,want", [([2.0] * 7, [2.0] * 5, 0.5), ([3, 4, 5], [0, 1, 2, 2], 1.0), ([0, 1, 2, 2], [3, 4, 5], 0.0)])
def test_auroc_of_equal_separated_and_reversed_scores(si, so, want):
    m = OD.reference_metrics(si, so)
    assert m["auroc"] == want
    assert m["fpr95"] == (0.0 if want == 1.0 else 1.0)
    if want == 1.0:
        assert m["aupr"] == 1.0
    if want == 0.5:
        assert m["aupr"] == pytest.approx(7 / 12)          # one threshold: precision n_i / (n_i + n_o) at recall 1


@pytest.mark.parametrize("ni", [1, 19, 20, 21, 100])
def test_fpr95_takes_the_ceil_095_n_th_largest_id_score(ni):
    si = np.random.default_rng(ni).permutation(ni).astype(np.float64)
    k = math.ceil(Fraction(95, 100) * ni)
    assert k == {1: 1, 19: 19, 20: 19, 21: 20, 100: 95}[ni]
    tau = ni - k                                             # the k-th largest of 0 .. ni - 1
    so = np.concatenate([np.arange(-2, ni + 2), [tau, tau - 0.5, tau + 0.5]]).astype(np.float64)
    want = float((so >= tau).sum()) / len(so)
    assert OD.reference_metrics(si, so)["fpr95"] == want
    assert OD.reference_metrics(si, [tau - 1e-9])["fpr95"] == 0.0 and OD.reference_metrics(si, [tau])["fpr95"] == 1.0      # a tie with tau counts


def test_metrics_against_sklearn():
    skm = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(0)
    cases = [(OR.TIE_ID, OR.TIE_OOD), (rng.standard_normal(300) + 1.0, rng.standard_normal(200)),
             (np.round(rng.standard_normal(500) * 3 + 1), np.round(rng.standard_normal(400) * 3))]      # the last: ties everywhere
    for si, so in cases:
        y = np.concatenate([np.ones(len(si)), np.zeros(len(so))])
        s = np.concatenate([np.asarray(si, dtype=np.float64), np.asarray(so, dtype=np.float64)])
        m = OD.reference_metrics(si, so)
        assert m["auroc"] == pytest.approx(skm.roc_auc_score(y, s), abs=1e-12)
        assert m["aupr"] == pytest.approx(skm.average_precision_score(y, s), abs=1e-12)


def test_a_nan_score_names_the_method_and_the_bank():
    with pytest.raises(ValueError, match="energy.*OOD bank"):
        OD.metrics([1.0, 2.0], [0.0, float("nan")], "energy")
    with pytest.raises(ValueError, match="ID bank"):
        OD.reference_metrics([float("nan")], [0.0])


# ---- the fit ------------------------------------------------------------------------------------------------------------------------
def test_reference_fit_whitens_the_within_class_scatter():
    fx = OR.gauss_fixture(1, 600, 10, 64, 200)
    for lam in (0.0, 1e-6, 1e-2):
        g = OD.reference_fit(fx["x"], fx["y"], 10, lam)
        W, S, m = g["whiten"], g["scatter"], g["m"]
        assert m == 600 and torch.equal(g["counts"], torch.full((10,), 60))
        ridge = lam * float(torch.trace(S / m)) / 64
        want = m * (torch.eye(64, dtype=torch.float64) - ridge * W @ W.T)      # W (S/m + ridge I) W^T = I
        assert float((W @ S @ W.T - want).abs().max()) <= 1e-8 * m
        assert float((W @ g["cov"] @ W.T - torch.eye(64, dtype=torch.float64)).abs().max()) <= 1e-10
        assert torch.allclose(g["wmeans"], (g["means"] - g["mean0"]) @ W.T, atol=1e-12)


def test_reference_fit_global_covariance_needs_no_second_pass():
    fx = OR.gauss_fixture(1, 650, 3, 8, 130)
    y = fx["y"].clone()
    y[::7] = -1                                              # uncounted rows take no part
    y[3::11] = 3
    g = OD.reference_fit(fx["x"], y, 3, 1e-6)
    x = fx["x"].double()[(y >= 0) & (y < 3)]
    assert g["m"] == len(x)
    c = x - x.mean(0)
    direct = c.T @ c / len(x) + 1e-6 * float(torch.trace(g["scatter"] / g["m"])) / 8 * torch.eye(8, dtype=torch.float64)
    assert float((g["mean0"] - x.mean(0)).abs().max()) <= 1e-12
    assert float((g["cov0"] - direct).abs().max()) <= 1e-10


def test_an_empty_class_is_never_the_argmin():
    fx = OR.gauss_fixture(1, 650, 3, 8, 130)
    y = fx["y"].clone()
    y[y == 1] = 4                                            # class 1 is empty, 4 lies outside [0, 4)
    det = OR.host_detector(fx["x"], y, 4)
    assert det["counts"].tolist()[1] == 0 and det["counts"].tolist()[3] == 0
    assert float(det["means"][1].abs().max()) == 0.0 and float(det["wmeans"][1].abs().max()) == 0.0
    d2, _ = OD.reference_gauss(det, torch.cat([fx["xt"], fx["xo"], torch.zeros(1, 8)]))
    arg = d2.argmin(dim=1)
    assert set(arg.tolist()) <= {0, 2} and bool(torch.isinf(d2[:, 1]).all())


def test_a_failed_cholesky_names_shrinkage():
    fx = OR.gauss_fixture(1, 650, 3, 8, 130)
    x = fx["x"].clone()
    x[:, 5] = 1.25                                           # a constant feature: a zero row and column of the scatter
    with pytest.raises(ValueError, match="--shrinkage"):
        OD.reference_fit(x, fx["y"], 3, 0.0)
    assert OD.reference_fit(x, fx["y"], 3, 1e-6)["whiten"].shape == (8, 8)


def test_the_small_fixture_gives_the_recorded_aurocs():
    fx = OR.gauss_fixture(1, 650, 3, 8, 130)
    det = OR.host_detector(fx["x"], fx["y"], 3)
    si = OD.reference_scores(det, OR.bank_of(fx["xt"], fx["yt"], 3), ("mahalanobis", "rmd"))
    so = OD.reference_scores(det, OR.bank_of(fx["xo"], torch.zeros(130, dtype=torch.int64), 3), ("mahalanobis", "rmd"))
    assert OD.reference_metrics(si["mahalanobis"], so["mahalanobis"])["auroc"] == pytest.approx(0.9427, abs=1e-3)
    assert OD.reference_metrics(si["rmd"], so["rmd"])["auroc"] == pytest.approx(0.9031, abs=1e-3)


@pytest.mark.parametrize("shape", OR.FIXTURES)
def test_fixture_gaps_stay_within_the_cap(shape):
    n, C, D, n_ood = shape
    fx = OR.gauss_fixture(1, *shape)
    det = OR.host_detector(fx["x"], fx["y"], C, knn=False)
    d2, _ = OD.reference_gauss(det, torch.cat([fx["xt"], fx["xo"]]))
    gap = OR.top2_gap(d2)
    assert float((gap <= OR.GAP).double().mean()) <= OR.GAP_ROWS
    if shape[2] != 8:
        si, so = -d2[:n // 2].min(dim=1)[0], -d2[n // 2:].min(dim=1)[0]
        assert OD.reference_metrics(si, so)["auroc"] == 1.0


def test_the_augmentation_identity():
    """min_c |z - m_c|^2 = |z|^2 - 2 max_c (z . m_c - |m_c|^2 / 2): what ops.gauss_scores hands to the k = 1 search."""
    fx = OR.gauss_fixture(1, 600, 10, 64, 200)
    det = OR.host_detector(fx["x"], fx["y"], 10, knn=False)
    q = torch.cat([fx["xt"], fx["xo"]]).double()
    z = (q - det["mean0"].double()) @ det["whiten"].double().T
    m = det["wmeans"].double()
    za = torch.cat([z, torch.ones(len(z), 1, dtype=torch.float64)], dim=1)
    ma = torch.cat([m, -0.5 * m.square().sum(dim=1, keepdim=True)], dim=1)
    sims = za @ ma.T
    direct, _ = OD.reference_gauss(det, q)
    got = z.square().sum(dim=1) - 2 * sims.max(dim=1)[0]
    assert float((got - direct.min(dim=1)[0]).abs().max()) <= 1e-9 * float(direct.max())
    assert torch.equal(sims.argmax(dim=1), direct.argmin(dim=1))
    # centred on mean0 the two terms are of the size of the distance itself
    assert float(z.square().sum(dim=1).max()) <= 4 * float(direct.max())


# ---- files, refusals, parser ------------------------------------------------------------------------------------------------------------
def _banks():
    fx = OR.gauss_fixture(1, 650, 3, 8, 130)
    g = torch.Generator().manual_seed(3)
    mk = lambda x, y: OR.bank_of(x, y, 3, logits=torch.randn(len(x), 8, generator=g))
    return mk(fx["x"], fx["y"]), mk(fx["xt"], fx["yt"]), mk(fx["xo"], torch.zeros(130, dtype=torch.int64))


def test_bank_and_detector_round_trip(tmp_path):
    train, test, ood = _banks()
    assert set(train) == {"features", "labels", "data_classes", "meta", "logits", "num_classes", "normalized"}
    assert train["normalized"] is False and train["num_classes"] == 8 and train["logits"].dtype == torch.float32
    assert train["meta"]["embed_dim"] == 8 and set(train["meta"]) == set(CT.META_KEYS)
    torch.save(train, tmp_path / "b.pt")
    back = OD.load_ood_bank(tmp_path / "b.pt")
    assert all(torch.equal(back[k], train[k]) for k in ("features", "labels", "logits")) and back["data_classes"] == 3
    assert CT.load_bank(tmp_path / "b.pt")["data_classes"] == 3            # still a feature bank
    det = OR.host_detector(train["features"], train["labels"], 3)
    assert set(OD.DETECTOR_KEYS) | {"knn_bank"} == set(det)
    torch.save(det, tmp_path / "d.pt")
    back = OD.check_detector(torch.load(tmp_path / "d.pt", map_location="cpu"))
    for k, v in det.items():
        assert torch.equal(back[k], v) if torch.is_tensor(v) else back[k] == v
    assert back["counts"].dtype == torch.int64 and all(back[k].dtype == torch.float32 for k in ("means", "mean0", "scatter", "whiten", "whiten0", "wmeans", "knn_bank"))
    assert torch.allclose(back["knn_bank"].norm(dim=1), torch.ones(650), atol=1e-6)
    ref = OD.reference_scores(det, test, OD.METHODS, k=5)
    assert set(ref) == set(OD.METHODS) and all(v.shape == (325,) and v.dtype == torch.float64 for v in ref.values())


def test_knn_rows_are_a_seeded_ascending_subset():
    rows = OD.knn_rows(1000, 0.25, 7)
    assert len(rows) == 250 and bool((rows[1:] > rows[:-1]).all())
    assert torch.equal(rows, torch.sort(torch.randperm(1000, generator=torch.Generator().manual_seed(7))[:250])[0])
    assert len(OD.knn_rows(1000, 0.0, 0)) == 0 and torch.equal(OD.knn_rows(9, 1.0, 0), torch.arange(9))
    assert len(OD.knn_rows(7, 0.5, 0)) == 4                  # ceil
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="--knn_fraction"):
            OD.knn_rows(10, bad, 0)


def test_refusals_by_name():
    train, test, ood = _banks()
    det = OR.host_detector(train["features"], train["labels"], 3)
    # fit: a bank that is not raw, or has no logits
    for bank, word in ((dict(train, normalized=True), "normalized"), ({k: v for k, v in train.items() if k != "normalized"}, "normalized"),
                       ({k: v for k, v in train.items() if k != "logits"}, "logits")):
        with pytest.raises(ValueError, match=word):
            OD.fit_detector(bank)
    with pytest.raises(ValueError, match="--knn_fraction"):
        OD.fit_detector(train, knn_fraction=1.5)
    with pytest.raises(ValueError, match="embed_dim"):
        OD.fit_detector(OR.bank_of(torch.zeros(4, 12), torch.zeros(4, dtype=torch.int64), 3))
    with pytest.raises(L.UvcHipError):                       # no CPU fallback
        OD.fit_detector(train, dev="cpu")
    # score: the banks against the detector
    wide = OR.bank_of(torch.zeros(4, 16), torch.zeros(4, dtype=torch.int64), 3)
    with pytest.raises(ValueError, match="ID bank's embed_dim 16"):
        OD.evaluate(det, wide, ood)
    with pytest.raises(ValueError, match="OOD bank's num_classes 16"):
        OD.evaluate(det, test, OR.bank_of(ood["features"], ood["labels"], 3, num_classes=16))
    with pytest.raises(ValueError, match="ID bank's data_classes 2"):
        OD.evaluate(det, dict(test, data_classes=2), ood)
    other = OR.bank_of(ood["features"], ood["labels"], 5)    # an OOD set's own label count is not read
    with pytest.raises(L.UvcHipError):
        OD.evaluate(det, test, other, methods=("msp",), dev="cpu")
    # methods and settings, before anything is computed
    no_knn = {k: v for k, v in det.items() if k != "knn_bank"}
    with pytest.raises(ValueError, match="knn_bank"):
        OD.evaluate(no_knn, test, ood, methods=("msp", "knn"))
    with pytest.raises(ValueError, match=r"--k must lie in \[1, 64\]"):
        OD.evaluate(det, test, ood, k=65)
    with pytest.raises(ValueError, match="--k 40 is more than the knn_bank's 30 rows"):
        OD.evaluate(dict(det, knn_bank=det["knn_bank"][:30]), test, ood, k=40)
    for T in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="--temperature"):
            OD.evaluate(det, test, ood, methods=("energy",), temperature=T)
    with pytest.raises(ValueError, match="not one of"):
        OD.evaluate(det, test, ood, methods=("vim",))
    with pytest.raises(ValueError, match="version-1 detector"):
        OD.evaluate({"version": 2}, test, ood)


def test_parser_flags():
    p = OD.build_parser()
    flags = lambda name: sorted(o for a in p._subparsers._group_actions[0].choices[name]._actions for o in a.option_strings if o.startswith("--") and o != "--help")
    embed = CT.build_parser()._subparsers._group_actions[0].choices["embed"]
    assert flags("bank") == sorted(o for a in embed._actions for o in a.option_strings if o.startswith("--") and o != "--help")
    assert flags("fit") == ["--bank", "--chunk_rows", "--knn_fraction", "--output", "--seed", "--shrinkage"]
    assert flags("score") == ["--detector", "--id_bank", "--k", "--methods", "--ood_bank", "--output", "--precision", "--temperature"]
    a = p.parse_args(["fit", "--bank", "b", "--output", "d"])
    assert (a.shrinkage, a.knn_fraction, a.seed, a.chunk_rows) == (1e-6, 1.0, 0, None)
    a = p.parse_args(["score", "--detector", "d", "--id_bank", "i", "--ood_bank", "o"])
    assert (tuple(a.methods), a.k, a.temperature, a.precision, a.output) == (OD.METHODS, 50, 1.0, "bf16", None)
    a = p.parse_args(["score", "--detector", "d", "--id_bank", "i", "--ood_bank", "o", "--methods", "msp", "rmd", "--precision", "fp32"])
    assert a.methods == ["msp", "rmd"] and a.precision == "fp32"
    with pytest.raises(SystemExit):
        p.parse_args(["score", "--detector", "d", "--id_bank", "i", "--ood_bank", "o", "--methods", "odin"])
    a = p.parse_args(["bank", "--compact", "f", "--output", "b", "--split", "test"])
    assert (a.split, a.dataset, a.precision, a.eval_batch_size) == ("test", "imagenet", "bf16", 256)
