"""CPU: the bicubic filter and crop_pct of the image pipeline (uvc_amd/data.py, include/uvc_data.h) -- the filter-parameterised numpy
restatement of PIL's resize (tests/pil_resample.py) against the installed PIL, the cover condition that makes the clamps of both
passes live code in the shared cases, the eval size rule, the drivers' flags and the host reference pipeline."""
import argparse

import numpy as np
import pytest
import torch
from PIL import Image

import pil_resample as R
from uvc_amd import data as D

PIL_FILTER = {R.BILINEAR: Image.BILINEAR, R.BICUBIC: Image.BICUBIC}


@pytest.mark.parametrize("filt", [R.BICUBIC, R.BILINEAR])
@pytest.mark.parametrize("pattern", sorted(R.PATTERNS))
def test_restatement_equals_pil_resize(pattern, filt):
    for name, (h, w), size in R.SHAPES:
        a = R.PATTERNS[pattern](h, w)
        ref = np.asarray(Image.fromarray(a).resize(size, PIL_FILTER[filt]))
        assert np.array_equal(R.resize(a, size, filt), ref), (name, pattern, filt)


@pytest.mark.parametrize("pattern", sorted(R.PATTERNS))
def test_restatement_equals_pil_crop_then_resize(pattern):
    """crop().resize(): what a random resized crop is, and what uvc_image_prep_crops reads in place."""
    a = R.PATTERNS[pattern](41, 53)
    for (x0, y0, x1, y1), size in (((3, 5, 40, 28), (8, 8)), ((10, 2, 26, 39), (16, 16)), ((0, 0, 1, 41), (8, 8)), ((7, 7, 39, 39), (224, 224))):
        ref = np.asarray(Image.fromarray(a).crop((x0, y0, x1, y1)).resize(size, Image.BICUBIC))
        got = R.resize(np.ascontiguousarray(a[y0:y1, x0:x1]), size, R.BICUBIC)
        assert np.array_equal(got, ref), (pattern, (x0, y0, x1, y1), size)


def test_restatement_equals_pil_on_the_clamp_cases_and_the_eval_geometry():
    for name, a, size in R.CLAMP_CASES:
        assert np.array_equal(R.resize(a, size, R.BICUBIC), np.asarray(Image.fromarray(a).resize(size, Image.BICUBIC))), name
    a = R.noise(375, 500, seed=3)                                # 500 x 375 -> 341 x 256, the ImageNet eval resize
    assert D.resize_short_side(375, 500, 256) == (256, 341)
    assert np.array_equal(R.resize(a, (341, 256), R.BICUBIC), np.asarray(Image.fromarray(a).resize((341, 256), Image.BICUBIC)))


@pytest.mark.parametrize("name,a,size", R.CLAMP_CASES, ids=[c[0] for c in R.CLAMP_CASES])
def test_clamp_cases_overshoot_in_the_passes_they_are_there_for(name, a, size):
    """A cover condition, not a measurement: the accumulators of the restatement, before clip8, leave 0 .. 255 << 22 on both sides --
    for a checkerboard in the first pass and in the second, for an upright step edge in the first (horizontal) pass, for the edge
    lying down in the second (vertical) pass.  So code that shifted without clamping could not reproduce these images, and since the
    first pass's overshoot is clamped before the second pass reads it, neither could code that clamped at the end only."""
    accs = []
    out = R.resize(a, size, R.BICUBIC, accs=accs)
    assert len(accs) == 2
    first, second = R.overshoot(accs[0]), R.overshoot(accs[1])
    if name.startswith("checkerboard"):
        assert min(first) >= 1 and min(second) >= 1, (first, second)
    elif name.startswith("step_rows"):
        assert min(second) >= 1, second
    else:
        assert min(first) >= 1, first
    assert not np.array_equal(out, R.resize(a, size, R.BILINEAR))
    assert not np.array_equal(out, np.asarray(Image.fromarray(a).resize(size, Image.BILINEAR)))


def test_clamp_cases_cover_both_sides_of_both_passes():
    under = [0, 0]
    over = [0, 0]
    for name, a, size in R.CLAMP_CASES:
        accs = []
        R.resize(a, size, R.BICUBIC, accs=accs)
        for p, acc in enumerate(accs):
            u, o = R.overshoot(acc)
            under[p] += u
            over[p] += o
    assert min(under) >= 1 and min(over) >= 1, (under, over)


def test_bicubic_sums_fit_int32():
    """|partial sum| <= 255 * sum|w| + 2^21 for 8-bit pixels: below 2^31 for every coefficient row of the shared shapes and of a
    sweep of small sides (the bound of include/uvc_data.h; PIL accumulates in `int` as well)."""
    pairs = [(s, o) for _, (h, w), (ow, oh) in R.SHAPES for s, o in ((w, ow), (h, oh))]
    pairs += [(i, o) for i in range(1, 41) for o in (1, 2, 3, 5, 8, 13, 16, 31, 224)] + [(500, 341), (375, 256)]
    worst = 0
    for i, o in pairs:
        _, _, kk = R.coeffs(i, 0, i, o, R.BICUBIC)
        worst = max(worst, int(np.abs(kk).sum(1).max()))
    assert 255 * worst + (1 << 21) < (1 << 31)
    assert worst > (1 << 22)                                    # (negative weights are there: sum|w| > 1)
    assert worst < 1.3 * (1 << 22)                              # (the figure the header quotes)


def test_eval_resize_side_rule():
    assert D.eval_resize_side(224, 0.875) == 256
    assert D.eval_resize_side(224, 0.9) == 248
    assert D.eval_resize_side(224, 1.0) == 224
    for S in (16, 32, 224, 384):
        assert D.eval_resize_side(S, None) == S * 256 // 224 == D.eval_resize_side(S)
        assert D.eval_resize_side(S, 1.0) == S
    assert D.eval_resize_side(16, 0.9) == 17
    for bad in (0.0, -0.5, 1.0001, 2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            D.eval_resize_side(224, bad)


def test_unknown_interpolation_is_refused():
    ds = D.ArrayDataset(R.noise(4 * 8, 8).reshape(4, 8, 8, 3), np.arange(4))
    with pytest.raises(ValueError):
        D.host_reference_batch(ds, [0], 8, False, 0, 0, D.IMAGENET_MEAN, D.IMAGENET_STD, interpolation="lanczos")
    with pytest.raises(ValueError):
        D.host_reference_batch(ds, [0], 8, False, 0, 0, D.IMAGENET_MEAN, D.IMAGENET_STD, crop_pct=1.5)
    args = argparse.Namespace(img_size=8, dataset="cifar10", data_dir="/nonexistent", train_batch_size=2, eval_batch_size=2,
                              interpolation="bilinear", crop_pct=0.0)
    with pytest.raises(ValueError, match="crop_pct"):
        D.build_loaders(args)


# ---------------------------------------------------------------------------------------------------------------- drivers

def _parsers():
    from uvc_amd import cli, compact, post_train
    stage2 = post_train.add_stage2_flags(argparse.ArgumentParser())
    cp = compact._parser()
    return {"cli": (cli.build_parser(), []),
            "post_train": (stage2, []),
            "compact eval": (cp, ["eval"]),
            "compact finetune": (cp, ["finetune", "--compact", "c.pt", "--output", "o.pt"])}


@pytest.mark.parametrize("driver", ["cli", "post_train", "compact eval", "compact finetune"])
def test_drivers_accept_the_flags(driver):
    p, head = _parsers()[driver]
    a = p.parse_args(head)
    assert a.interpolation == "bilinear" and a.crop_pct is None
    a = p.parse_args(head + ["--interpolation", "bicubic", "--crop_pct", "0.9"])
    assert a.interpolation == "bicubic" and a.crop_pct == 0.9
    with pytest.raises(SystemExit):
        p.parse_args(head + ["--interpolation", "lanczos"])


class _FakeLoader:
    made = []

    def __init__(self, dataset, batch_size, img_size, **kw):
        self.kw = dict(kw, img_size=img_size)
        _FakeLoader.made.append(self)


def _write_cifar10(root):
    import pickle
    d = root / "cifar-10-batches-py"
    d.mkdir()
    rng = np.random.default_rng(0)
    for f in [f"data_batch_{i}" for i in range(1, 6)] + ["test_batch"]:
        with open(d / f, "wb") as fh:
            pickle.dump({"data": rng.integers(0, 256, (2, 3072), dtype=np.uint8), "labels": [0, 1]}, fh)


@pytest.mark.parametrize("driver", ["cli", "post_train", "compact eval", "compact finetune"])
def test_flags_reach_the_loaders_through_build_loaders(driver, tmp_path, monkeypatch):
    """Each driver's parsed namespace, handed to build_loaders as the driver hands it: the loaders are constructed with the filter
    (train and test) and, on the ImageNet path, the crop_pct; the defaults construct them with bilinear / None."""
    p, head = _parsers()[driver]
    _write_cifar10(tmp_path)
    monkeypatch.setattr(D, "DeviceLoader", _FakeLoader)
    for flags, want in (([], ("bilinear", None)), (["--interpolation", "bicubic", "--crop_pct", "0.9"], ("bicubic", 0.9))):
        a = p.parse_args(head + flags + ["--dataset", "cifar10", "--data_dir", str(tmp_path)])
        if not hasattr(a, "train_batch_size"):
            a.train_batch_size = a.eval_batch_size
        a.img_size = getattr(a, "img_size", 32)
        _FakeLoader.made.clear()
        train, test = D.build_loaders(a)
        assert train.kw["interpolation"] == test.kw["interpolation"] == want[0]
        assert "crop_pct" not in test.kw and test.kw["eval"] == "square"          # CIFAR's eval resize takes the filter and ignores crop_pct
        # the ImageNet path: an image folder of two classes
        from PIL import Image as I
        for split in ("train", "val"):
            for c in ("a", "b"):
                d = tmp_path / "inet" / split / c
                d.mkdir(parents=True, exist_ok=True)
                I.fromarray(R.noise(9, 11)).save(d / "x.png")
        a = p.parse_args(head + flags + ["--dataset", "imagenet", "--data_dir", str(tmp_path / "inet")])
        if not hasattr(a, "train_batch_size"):
            a.train_batch_size = a.eval_batch_size
        a.img_size, a.num_classes = 16, 8
        train, test = D.build_loaders(a)
        assert (train.kw["interpolation"], train.kw["crop_pct"]) == want == (test.kw["interpolation"], test.kw["crop_pct"])


def test_compact_eval_hands_the_flags_to_build_loaders(monkeypatch):
    """compact eval builds its loader from its own parsed namespace, at the export's image size and classes: the two flags reach
    build_loaders on it."""
    from uvc_amd import compact
    seen = {}

    def spy(args, **kw):
        seen.update(vars(args), splits=kw.get("splits"))
        raise KeyboardInterrupt                                  # the loader itself is test_flags_reach_the_loaders_through_build_loaders' matter

    monkeypatch.setattr(compact, "load_compact", lambda path: dict(cfg=dict(img_size=96, num_classes=24)))
    monkeypatch.setattr(compact, "CompactVisionTransformer", lambda *a, **k: None)
    monkeypatch.setattr(D, "build_loaders", spy)
    with pytest.raises(KeyboardInterrupt):
        compact.main(["eval", "--compact", "c.pt", "--synthetic", "0", "--interpolation", "bicubic", "--crop_pct", "0.9", "--eval_batch_size", "4"])
    assert (seen["interpolation"], seen["crop_pct"], seen["eval_batch_size"], seen["splits"]) == ("bicubic", 0.9, 4, ("test",))
    assert (seen["img_size"], seen["num_classes"]) == (96, 24)


# ---------------------------------------------------------------------------------------------------------------- host reference

def _small_dataset():
    rng = np.random.default_rng(5)
    imgs = [rng.integers(0, 256, (int(rng.integers(20, 41)), int(rng.integers(20, 41)), 3), dtype=np.uint8) for _ in range(6)]

    class DS:
        targets = np.arange(6)

        def __len__(self):
            return 6

        def load(self, i):
            return imgs[i]
    return DS(), imgs


def _to_tensor(im, mean, std):
    t = torch.from_numpy(np.array(im, dtype=np.uint8)).permute(2, 0, 1).float().div(255)
    return (t - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1)


def test_host_reference_batch_bicubic_is_the_pil_calls_written_out():
    ds, imgs = _small_dataset()
    S, mean, std = 16, D.IMAGENET_MEAN, D.IMAGENET_STD
    ids = [4, 0, 5, 2]
    # eval, crop_pct 0.9: Resize(int(16 / 0.9) = 17, BICUBIC) + CenterCrop(16)
    got = D.host_reference_batch(ds, ids, S, False, 0, 0, mean, std, interpolation="bicubic", crop_pct=0.9)
    for b, k in enumerate(ids):
        h, w = imgs[k].shape[:2]
        rh, rw = (17, int(17 * w / h)) if h <= w else (int(17 * h / w), 17)
        im = Image.fromarray(imgs[k]).resize((rw, rh), Image.BICUBIC)
        y0, x0 = int(round((rh - S) / 2.0)), int(round((rw - S) / 2.0))
        assert torch.equal(got[b], _to_tensor(im.crop((x0, y0, x0 + S, y0 + S)), mean, std)), k
    # eval without crop_pct: 16 * 256 // 224 = 18
    got = D.host_reference_batch(ds, ids, S, False, 0, 0, mean, std, interpolation="bicubic")
    for b, k in enumerate(ids):
        h, w = imgs[k].shape[:2]
        rh, rw = D.resize_short_side(h, w, 18)
        im = Image.fromarray(imgs[k]).resize((rw, rh), Image.BICUBIC)
        y0, x0 = D.center_crop_offset(rh, rw, S)
        assert torch.equal(got[b], _to_tensor(im.crop((x0, y0, x0 + S, y0 + S)), mean, std)), k
    # square eval (CIFAR): the filter applies, crop_pct does not
    got = D.host_reference_batch(ds, ids, S, False, 0, 0, mean, std, eval="square", interpolation="bicubic", crop_pct=0.9)
    for b, k in enumerate(ids):
        assert torch.equal(got[b], _to_tensor(Image.fromarray(imgs[k]).resize((S, S), Image.BICUBIC), mean, std)), k
    # train: the crop and flip draws of the bilinear pipeline, resized with BICUBIC
    seed, epoch = 3, 2
    got = D.host_reference_batch(ds, ids, S, True, seed, epoch, mean, std, interpolation="bicubic")
    u = D.sample_uniforms(seed, epoch, ids, D.RRC_DRAWS)
    flips = 0
    for b, k in enumerate(ids):
        h, w = imgs[k].shape[:2]
        i, j, ch, cw = (int(v[0]) for v in D.rrc_params([h], [w], u[b:b + 1]))
        im = Image.fromarray(imgs[k]).crop((j, i, j + cw, i + ch)).resize((S, S), Image.BICUBIC)
        if u[b, 40] < 0.5:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
            flips += 1
        assert torch.equal(got[b], _to_tensor(im, mean, std)), k
    bil = D.host_reference_batch(ds, ids, S, True, seed, epoch, mean, std)
    assert not torch.equal(got, bil)
    assert torch.equal(bil, D.host_reference_batch(ds, ids, S, True, seed, epoch, mean, std, interpolation="bilinear", crop_pct=None))
