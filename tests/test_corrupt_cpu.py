"""CPU: the common-corruption spec (uvc_amd.compact_corrupt.reference_corrupt) against the independent loops of tests/corrupt_ref.py, its level
identities and properties, the keyed Box-Muller and impulse draws, the error arithmetic on hand-made tables, the parser, and the share of
(image, kind, severity) triples the module fixture leaves undecided."""
import colorsys

import numpy as np
import pytest
import torch

import corrupt_ref as CR
import knn_ref as KR
from uvc_amd import compact as CP
from uvc_amd import compact_corrupt as CC

MEAN, STD = CR.MEAN, CR.STD
TINY = [(1, 1, 1, 1), (1, 3, 1, 3), (2, 3, 5, 7), (1, 2, 6, 4)]
LEVELS = {"gaussian_noise": [0.08, 0.38], "speckle_noise": [0.15, 0.6], "impulse_noise": [0.03, 0.27, 1.0], "brightness": [0.1, 0.5],
          "contrast": [0.4, 0.05], "gaussian_blur": [0.0, 1, 2.5], "defocus_blur": [1, 3], "pixelate": [1, 2, 3, 7]}
MODULE_MODELS = ("stage2_micro_deit", "stage2_micro_none")
# the module tests' images: six of a pool of 24, picked on the float64 reference alone (those it decides most often under both models)
MODULE_POOL, MODULE_SEED, MODULE_PICK, MODULE_BAR = 24, 3, (2, 11, 22, 15, 13, 17), 2e-2   # (the wider of the two precisions' bars)


def test_the_kinds_and_the_severity_table():
    assert CC.CORRUPTIONS == CR.KINDS and sorted(CC.SEVERITY) == sorted(CC.CORRUPTIONS)
    for kind, levels in CC.SEVERITY.items():
        assert len(levels) == 5
        d = np.diff(np.asarray(levels, np.float64))
        assert (d > 0).all() or (d < 0).all(), kind
        for s in (1, 2, 3, 4, 5):
            assert CC.level_of(kind, severity=s) == (CC.check_level(kind, levels[s - 1]), 8 * CC.CORRUPTIONS.index(kind) + s)
        assert CC.level_of(kind, level=levels[0])[1] == 8 * CC.CORRUPTIONS.index(kind)
    assert isinstance(CC.level_of("pixelate", severity=1)[0], int) and isinstance(CC.level_of("defocus_blur", severity=5)[0], int)


@pytest.mark.parametrize("kind", CC.CORRUPTIONS)
def test_reference_equals_the_loops(kind):
    for si, shape in enumerate(TINY):
        mean, std = CR.stats(shape[1])
        x = CR.images(shape, 10 + si, mean, std)
        for a in LEVELS[kind]:
            for index0 in (0, 3):
                kw = dict(mean=mean, std=std, seed=5, stream=9, index0=index0)
                want = CR.loops(x, kind, a, mean, std, seed=5, stream=9, index0=index0)
                got = CC.reference_corrupt(torch.from_numpy(x), kind, a, clamp=False, **kw).numpy()
                assert got.dtype == np.float64 and np.abs(got - want).max() <= 1e-12 * (1 + np.abs(want).max()), (shape, a)
                out = CC.reference_corrupt(torch.from_numpy(x), kind, a, **kw)
                assert out.dtype == torch.float32 and np.array_equal(out.numpy(), CR.clamp32(got, mean, std))
                lo, hi = CR.bounds(mean, std)
                assert (out.numpy() >= lo.reshape(1, -1, 1, 1)).all() and (out.numpy() <= hi.reshape(1, -1, 1, 1)).all()


@pytest.mark.parametrize("kind, level", [("gaussian_noise", 0), ("speckle_noise", 0), ("impulse_noise", 0), ("brightness", 0), ("contrast", 1), ("pixelate", 1)])
def test_level_identities_are_exact(kind, level):
    x = torch.from_numpy(CR.images((2, 3, 9, 11), 1, MEAN, STD))
    out = CC.reference_corrupt(x, kind, level, mean=MEAN, std=STD, seed=2, stream=4, index0=7)
    assert torch.equal(out.view(torch.int32), x.view(torch.int32))


def test_blur_weights_and_a_constant_image():
    for sigma in (0.0, 0.3, 1, 2, 3, 4, 6, 8.1):
        w = CC.gaussian_taps(sigma)
        assert w.dtype == np.float32 and len(w) == 2 * int(4 * sigma + 0.5) + 1 and np.array_equal(w, CR.gaussian_taps(sigma))
        assert abs(float(w.astype(np.float64).sum()) - 1) <= 2.0 ** -23 and np.array_equal(w, w[::-1])
    for r in (1, 3, 10, 12):
        t = CC.disk_taps(r)
        assert np.array_equal(t, CR.disk_taps(r)) and abs(float(t.astype(np.float64).sum()) - 1) <= len(t) ** 2 * 2.0 ** -25
    x = torch.full((1, 3, 9, 12), 0.75)
    for kind, a in (("gaussian_blur", 1), ("gaussian_blur", 6), ("defocus_blur", 3), ("defocus_blur", 12)):
        out = CC.reference_corrupt(x, kind, a, mean=MEAN, std=STD)
        assert bool((out == out[0, 0, 0, 0]).all()) and abs(float(out[0, 0, 0, 0]) - 0.75) <= 0.75 * 2.0 ** -21


def test_pixelate_is_idempotent_and_contrast_keeps_the_mean():
    x = torch.from_numpy(CR.images((2, 3, 13, 10), 4, MEAN, STD))
    for k in (2, 3, 6, 14):
        once = CC.reference_corrupt(x, "pixelate", k, mean=MEAN, std=STD)
        assert torch.equal(CC.reference_corrupt(once, "pixelate", k, mean=MEAN, std=STD), once)
    mu, _ = CR.image_mean(x.numpy(), MEAN, STD)
    for a in (0.4, 0.05):
        out = CC.reference_corrupt(x, "contrast", a, mean=MEAN, std=STD)          # a < 1 moves every pixel towards the mean: nothing clamps
        got, _ = CR.image_mean(out.numpy(), MEAN, STD)
        assert np.abs(got - mu).max() <= 1e-6


def test_brightness_is_the_hsv_value_shift():
    rng = np.random.default_rng(0)
    p = rng.random((1, 3, 40, 25))
    p[0, :, 0, :5] = 0.0
    m, s = np.asarray(MEAN).reshape(1, 3, 1, 1), np.asarray(STD).reshape(1, 3, 1, 1)
    x = ((p - m) / s).astype(np.float32)
    px = np.clip(x.astype(np.float64) * s + m, 0, 1)
    for a in (0.1, 0.5):
        got = CC.reference_corrupt(torch.from_numpy(x), "brightness", a, mean=MEAN, std=STD, clamp=False).numpy() * s + m
        for y in range(40):
            for w in range(25):
                h, sat, v = colorsys.rgb_to_hsv(*px[0, :, y, w])
                want = colorsys.hsv_to_rgb(h, sat, min(v + a, 1.0))
                assert np.abs(got[0, :, y, w] - np.asarray(want)).max() <= 1e-12


def test_box_muller_and_impulse_statistics():
    n = 1 << 20
    z = CC.keyed_normals(0, 0, 0, n)
    zr, _ = CR.normals(0, 0, 0, n)
    assert np.array_equal(z, zr)
    print("box-muller: mean", z.mean(), "std", z.std(), "max |z|", np.abs(z).max())
    assert abs(z.mean()) <= 4 / np.sqrt(n) and abs(z.var() - 1) <= 4 * np.sqrt(2 / n)
    assert abs(z[0::2].mean()) <= 4 / np.sqrt(n / 2) and abs(z[1::2].mean()) <= 4 / np.sqrt(n / 2)
    x = torch.zeros(4, 3, 128, 128)                                      # 0 lies strictly inside [lo_c, hi_c]
    lo, hi = CR.bounds(MEAN, STD)
    for a in (0.03, 0.27):
        out = CC.reference_corrupt(x, "impulse_noise", a, mean=MEAN, std=STD, seed=1, stream=2).numpy()
        low, high = out == lo.reshape(1, 3, 1, 1), out == hi.reshape(1, 3, 1, 1)
        assert ((out == 0) | low | high).all()
        for share in (low.mean(), high.mean()):
            assert abs(share - a / 2) <= 4 * np.sqrt(a / 2 * (1 - a / 2) / out.size)


@pytest.mark.parametrize("kind", CC.NOISES)
def test_an_images_noise_does_not_depend_on_the_batching(kind):
    x = torch.from_numpy(CR.images((4, 3, 5, 5), 2, MEAN, STD))            # C H W = 75: odd, the pairs straddle the images
    kw = dict(mean=MEAN, std=STD, seed=3, stream=1)
    whole = CC.reference_corrupt(x, kind, 0.2, index0=10, **kw)
    for i in range(4):
        assert torch.equal(CC.reference_corrupt(x[i:i + 1], kind, 0.2, index0=10 + i, **kw), whole[i:i + 1])
    assert not torch.equal(CC.reference_corrupt(x, kind, 0.2, index0=11, **kw), whole)


def _table(clean, **kinds):
    return dict(clean_top1=clean, kinds={k: dict(levels=[1, 2], top1=list(v)) for k, v in kinds.items()})


def test_corruption_errors_on_hand_made_tables():
    t = _table(90.0, contrast=(80.0, 60.0), pixelate=(85.0, 75.0))
    own = CC.corruption_errors(t)
    assert own["kinds"]["contrast"]["error"] == [20.0, 40.0] and own["kinds"]["contrast"]["mean_error"] == 30.0
    assert own["mean_corruption_error"] == 25.0 and "mCE" not in own and "ce" not in own["kinds"]["contrast"]
    same = CC.corruption_errors(t, t)
    assert all(r["ce"] == 1.0 and r["relative_ce"] == 1.0 for r in same["kinds"].values())
    assert (same["mCE"], same["relative_mCE"], same["mCE_kinds"], same["relative_mCE_kinds"]) == (1.0, 1.0, 2, 2)
    assert same["baseline"]["kinds"] == own["kinds"]
    base = _table(95.0, contrast=(95.0, 95.0), pixelate=(90.0, 80.0))       # contrast costs the baseline nothing
    rec = CC.corruption_errors(t, base)
    assert rec["kinds"]["contrast"]["relative_ce"] is None and rec["kinds"]["contrast"]["ce"] == 60.0 / 10.0
    assert rec["kinds"]["pixelate"]["ce"] == 40.0 / 30.0 and rec["kinds"]["pixelate"]["relative_ce"] == (5.0 + 15.0) / (5.0 + 15.0)
    assert rec["relative_mCE"] == 1.0 and rec["relative_mCE_kinds"] == 1 and rec["mCE_kinds"] == 2 and rec["mCE"] == (6.0 + 40.0 / 30.0) / 2
    perfect = _table(100.0, contrast=(100.0, 100.0), pixelate=(100.0, 100.0))
    rec = CC.corruption_errors(t, perfect)
    assert rec["mCE"] is None and rec["relative_mCE"] is None and rec["mCE_kinds"] == 0
    with pytest.raises(ValueError):
        CC.corruption_errors(t, _table(90.0, contrast=(80.0, 60.0)))


def test_the_parser_and_its_refusals(capsys):
    p = CC.build_parser()
    a = p.parse_args(["--compact", "m.pt"])
    assert a.kinds == list(CC.CORRUPTIONS) and a.severities == [1, 2, 3, 4, 5] and a.level is None and a.seed == 0 and a.max_images is None
    assert (a.split, a.eval_batch_size, a.baseline, a.output, a.precision, a.dataset) == ("test", 64, None, None, "bf16", "imagenet")
    cells = CC.plan(a)
    assert len(cells) == 40 and cells[0] == ("gaussian_noise", 1, 0.08) and cells[-1] == ("pixelate", 5, 6)
    kinds = next(x for x in p._actions if x.dest == "kinds")
    assert tuple(kinds.choices) == CC.CORRUPTIONS and next(x for x in p._actions if x.dest == "severities").choices == [1, 2, 3, 4, 5]
    one = p.parse_args(["--compact", "m.pt", "--kinds", "gaussian_noise", "--level", "0"])
    assert CC.plan(one) == [("gaussian_noise", None, 0.0)]
    for bad in (["--kinds", "jpeg"], ["--severities", "0"], ["--severities", "6"]):
        with pytest.raises(SystemExit):
            p.parse_args(["--compact", "m.pt", *bad])
    capsys.readouterr()
    for bad in (["--level", "0.1"], ["--kinds", "contrast", "pixelate", "--level", "2"], ["--kinds", "pixelate", "--level", "2.5"],
                ["--kinds", "defocus_blur", "--level", "13"], ["--kinds", "impulse_noise", "--level", "1.5"], ["--kinds", "gaussian_noise", "--level", "-1"],
                ["--kinds", "gaussian_noise", "--level", "nan"], ["--kinds", "gaussian_blur", "--level", "9"], ["--kinds", "contrast", "contrast"],
                ["--max_images", "0"], ["--severities", "1", "1"]):
        with pytest.raises(ValueError):
            CC.plan(p.parse_args(["--compact", "m.pt", *bad]))
    with pytest.raises(ValueError):
        CC.main(["--compact", "m.pt", "--level", "0.1"])                      # before the file is opened
    with pytest.raises(SystemExit):
        CC.main(["--compact", "m.pt"])                                       # no data


def test_a_baseline_of_another_image_size_is_refused():
    ex, _ = KR.export_of("stage2_micro_deit")
    other, _ = KR.export_of("px384d")
    assert ex["cfg"]["img_size"] != other["cfg"]["img_size"]
    CC.check_baseline(ex, ex)
    with pytest.raises(ValueError, match="image size"):
        CC.check_baseline(ex, other)
    args = CC.build_parser().parse_args(["--compact", "m.pt", "--baseline", "b.pt", "--dataset", "cifar10", "--data_dir", "/nonexistent"])
    args.baseline = other
    with pytest.raises(ValueError, match="image size"):                      # before the device or any data is touched
        CC.evaluate(ex, args)


def module_batch(ex):
    """The module tests' images (tests/test_corrupt_gpu.py imports this): MODULE_PICK of a pool of normalised images at the model's size."""
    cfg = ex["cfg"]
    mean, std = CR.stats(cfg["in_chans"])
    pool = CR.images((MODULE_POOL, cfg["in_chans"], cfg["img_size"], cfg["img_size"]), MODULE_SEED, mean, std)
    return np.ascontiguousarray(pool[list(MODULE_PICK)]), mean, std


def undecided_share(ex, batches, bar):
    """The share of rows of the float64 reference logits of ``batches`` whose top-2 margin is at most twice ``bar`` of the largest logit."""
    out = 0
    for xc in batches:
        ref = CP.reference_forward(ex, xc.double())
        top2 = ref.topk(2, dim=1).values
        out += int(((top2[:, 0] - top2[:, 1]) <= 2 * bar * float(ref.abs().max())).sum())
    return out / (len(batches) * batches[0].shape[0])


@pytest.mark.parametrize("name", MODULE_MODELS)
def test_the_module_fixture_leaves_few_triples_undecided(name):
    ex, _ = KR.export_of(name)
    x, mean, std = module_batch(ex)
    batches = [CC.reference_corrupt(torch.from_numpy(x), k, CC.SEVERITY[k][s - 1], mean=mean, std=std, stream=8 * CC.CORRUPTIONS.index(k) + s)
               for k in CC.CORRUPTIONS for s in CC.SEVERITIES]
    share = undecided_share(ex, batches, MODULE_BAR)
    print(name, "undecided share", share)
    assert share <= 0.10
