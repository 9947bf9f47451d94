"""CPU: the host half of the real-data path (uvc_amd/data.py) -- ImageFolder indexing, the CIFAR pickle readers, the
DistributedSampler order, the counter-based crop draws, RandomResizedCrop / Resize / CenterCrop geometry -- and the numpy
restatement of PIL's bilinear resize that the GPU kernel is held to (tests/pil_bilinear.py)."""
import math
import os
import pickle

import numpy as np
import pytest
import torch
from PIL import Image

import pil_bilinear as PB
from uvc_amd import data as D


def _img(path, h=5, w=7, fmt=None):
    Image.fromarray(np.full((h, w, 3), 7, np.uint8)).save(path, format=fmt)


def test_image_folder_indexing(tmp_path):
    root = tmp_path / "train"
    for c in ("zebra", "ant", "Bee"):
        (root / c).mkdir(parents=True)
    (root / "ant" / "nested" / "deeper").mkdir(parents=True)
    _img(root / "ant" / "b.JPEG", fmt="JPEG")
    _img(root / "ant" / "a.png")
    _img(root / "ant" / "nested" / "c.jpg")
    _img(root / "ant" / "nested" / "deeper" / "d.Png", fmt="PNG")
    (root / "ant" / "notes.txt").write_text("not an image")
    (root / "ant" / "e.jpg.bak").write_text("nor this")
    _img(root / "Bee" / "x.bmp", fmt="BMP")
    _img(root / "zebra" / "z.webp", fmt="WEBP")
    (tmp_path / "train" / "loose.jpg").write_bytes(b"")          # a file at the root is not a class
    ds = D.ImageFolder(str(root))
    assert ds.classes == ["Bee", "ant", "zebra"]                 # sorted, case-sensitive like torchvision
    rel = [(os.path.relpath(p, root), t) for p, t in ds.samples]
    assert rel == [("Bee/x.bmp", 0), ("ant/a.png", 1), ("ant/b.JPEG", 1), ("ant/nested/c.jpg", 1),
                   ("ant/nested/deeper/d.Png", 1), ("zebra/z.webp", 2)]
    assert ds.targets.tolist() == [0, 1, 1, 1, 1, 2]
    a = ds.load(2)
    assert a.dtype == np.uint8 and a.shape == (5, 7, 3)


def test_image_folder_converts_to_rgb(tmp_path):
    (tmp_path / "c").mkdir()
    Image.fromarray(np.arange(12, dtype=np.uint8).reshape(3, 4), mode="L").save(tmp_path / "c" / "g.png")
    a = D.ImageFolder(str(tmp_path)).load(0)
    assert a.shape == (3, 4, 3) and np.array_equal(a[..., 0], a[..., 2])


def write_fake_cifar(root, name, n_train=12, n_test=6, seed=0):
    """Pickles in the layout torchvision's CIFAR readers expect (python 'latin1' dicts, rows of CHW bytes)."""
    rng = np.random.default_rng(seed)
    if name == "cifar10":
        d = os.path.join(root, "cifar-10-batches-py")
        files = [(f"data_batch_{i}", n_train // 5 + (1 if i <= n_train % 5 else 0)) for i in range(1, 6)] + [("test_batch", n_test)]
        key, ncls = "labels", 10
    else:
        d = os.path.join(root, "cifar-100-python")
        files, key, ncls = [("train", n_train), ("test", n_test)], "fine_labels", 100
    os.makedirs(d, exist_ok=True)
    out = {}
    for f, n in files:
        x = rng.integers(0, 256, (n, 3072), dtype=np.uint8)
        y = rng.integers(0, ncls, n).tolist()
        entry = {"data": x, key: y}
        if name == "cifar100":
            entry["coarse_labels"] = [v // 5 for v in y]
        with open(os.path.join(d, f), "wb") as fh:
            pickle.dump(entry, fh)
        out[f] = (x, y)
    return out


@pytest.mark.parametrize("name", ["cifar10", "cifar100"])
def test_cifar_readers(tmp_path, name):
    raw = write_fake_cifar(str(tmp_path), name)
    tr, te = D.read_cifar(str(tmp_path), name, True), D.read_cifar(str(tmp_path), name, False)
    keys = [f"data_batch_{i}" for i in range(1, 6)] if name == "cifar10" else ["train"]
    x = np.vstack([raw[k][0] for k in keys])
    y = sum([raw[k][1] for k in keys], [])
    assert tr.images.shape == (12, 32, 32, 3) and te.images.shape == (6, 32, 32, 3)
    assert np.array_equal(tr.images, x.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)) and tr.targets.tolist() == y
    test_key = "test_batch" if name == "cifar10" else "test"
    assert te.targets.tolist() == raw[test_key][1]
    # pixel (row 1, col 2) of image 0, channel c sits at c*1024 + 1*32 + 2 of the CHW row
    assert [int(tr.images[0, 1, 2, c]) for c in range(3)] == [int(x[0, c * 1024 + 34]) for c in range(3)]
    with pytest.raises(FileNotFoundError):
        D.read_cifar(str(tmp_path / "none"), name, True)


def test_sampler_matches_distributed_sampler_semantics():
    n, world = 23, 4
    for epoch in (0, 3):
        g = torch.Generator()
        g.manual_seed(7 + epoch)
        perm = torch.randperm(n, generator=g).tolist()
        padded = perm + perm[:math.ceil(n / world) * world - n]
        ranks = [D.epoch_indices(n, epoch, seed=7, rank=r, world=world) for r in range(world)]
        assert all(len(r) == math.ceil(n / world) for r in ranks)
        assert [padded[r::world] for r in range(world)] == ranks
        assert sorted(sum(ranks, [])) == sorted(padded) and set(sum(ranks, [])) == set(range(n))
        # disjoint apart from the head padding (one index appears twice only because of it)
        assert len(set(ranks[0]) & set(ranks[1])) == 0
    assert D.epoch_indices(n, 0, seed=7) == torch.randperm(n, generator=torch.Generator().manual_seed(7)).tolist()
    assert D.epoch_indices(n, 0, seed=7) != D.epoch_indices(n, 1, seed=7)          # reshuffled every epoch
    assert D.epoch_indices(3, 0, world=8) == [D.epoch_indices(3, 0)[0]]            # padding longer than the set wraps
    assert D.epoch_indices(5, 0, shuffle=False, rank=1, world=2) == [1, 3, 0]


def test_draws_are_keyed_by_sample_not_by_rank_or_workers():
    n = 40
    u_all = D.sample_uniforms(3, 2, np.arange(n), D.RRC_DRAWS)
    assert u_all.shape == (n, D.RRC_DRAWS) and (u_all >= 0).all() and (u_all < 1).all()
    for world in (1, 2, 3):
        for r in range(world):
            idx = D.epoch_indices(n, 2, seed=3, rank=r, world=world)
            assert np.array_equal(D.sample_uniforms(3, 2, idx, D.RRC_DRAWS), u_all[idx])
    # chunking the batch (what the worker threads see) does not change a sample's draws
    assert np.array_equal(np.vstack([D.sample_uniforms(3, 2, np.arange(a, min(a + 7, n)), D.RRC_DRAWS) for a in range(0, n, 7)]), u_all)
    assert not np.array_equal(D.sample_uniforms(3, 3, np.arange(n), D.RRC_DRAWS), u_all)
    assert not np.array_equal(D.sample_uniforms(4, 2, np.arange(n), D.RRC_DRAWS), u_all)
    assert abs(u_all.mean() - 0.5) < 0.05


def _ref_get_params(h, w, u, scale, ratio):
    """torchvision RandomResizedCrop.get_params written out scalar, with the same uniforms."""
    area = h * w
    lr = [float(v) for v in torch.log(torch.tensor(ratio))]
    for k in range(10):
        ta = area * (scale[0] + (scale[1] - scale[0]) * u[4 * k])
        ar = math.exp(lr[0] + (lr[1] - lr[0]) * u[4 * k + 1])
        cw, ch = int(round(math.sqrt(ta * ar))), int(round(math.sqrt(ta / ar)))
        if 0 < cw <= w and 0 < ch <= h:
            return int(u[4 * k + 2] * (h - ch + 1)), int(u[4 * k + 3] * (w - cw + 1)), ch, cw
    r = w / h
    if r < min(ratio):
        cw, ch = w, int(round(w / min(ratio)))
    elif r > max(ratio):
        ch, cw = h, int(round(h * max(ratio)))
    else:
        cw, ch = w, h
    return (h - ch) // 2, (w - cw) // 2, ch, cw


@pytest.mark.parametrize("scale", [(0.08, 1.0), (0.05, 1.0)])
def test_random_resized_crop_params(scale):
    rng = np.random.default_rng(0)
    B = 400
    h = rng.integers(1, 700, B)
    w = rng.integers(1, 700, B)
    h[:3], w[:3] = (10, 2000, 1), (2000, 10, 1)
    u = D.sample_uniforms(0, 0, np.arange(B), D.RRC_DRAWS)
    i, j, ch, cw = D.rrc_params(h, w, u, scale)
    for b in range(B):
        assert (i[b], j[b], ch[b], cw[b]) == _ref_get_params(int(h[b]), int(w[b]), u[b], scale, (3 / 4, 4 / 3)), b
    assert (ch >= 1).all() and (cw >= 1).all() and (i >= 0).all() and (j >= 0).all() and (i + ch <= h).all() and (j + cw <= w).all()
    fit = (ch * cw) / (h * w)
    normal = (h >= 50) & (w >= 50) & (np.maximum(h / w, w / h) < 1.3)
    assert (fit[normal] >= scale[0] * 0.8).all() and (fit <= 1.0 + 1e-9).all()
    r = cw[normal] / ch[normal]
    assert (r > 0.7).all() and (r < 1.43).all()
    # the fallback branch: a 10 x 2000 strip fits no 3/4..4/3 crop of >= 8 % of its area -> central crop at the 4/3 limit
    assert (i[0], j[0], ch[0], cw[0]) == (0, (2000 - 13) // 2, 10, 13)
    assert (i[1], j[1], ch[1], cw[1]) == ((2000 - 13) // 2, 0, 13, 10)
    assert (i[2], j[2], ch[2], cw[2]) == (0, 0, 1, 1)


def test_resize_and_center_crop_geometry():
    assert D.resize_short_side(375, 500, 256) == (256, 341)     # landscape: int(256 * 500 / 375) = 341
    assert D.resize_short_side(500, 375, 256) == (341, 256)
    assert D.resize_short_side(300, 300, 256) == (256, 256)
    assert D.resize_short_side(256, 999, 256) == (256, 999)
    # CenterCrop: int(round((h - 224) / 2.0)), half to even
    assert D.center_crop_offset(341, 256, 224) == (58, 16)       # (341 - 224) / 2 = 58.5 -> 58
    assert D.center_crop_offset(343, 256, 224) == (60, 16)       # 59.5 -> 60
    assert D.center_crop_offset(224, 225, 224) == (0, 0)         # 0.5 -> 0
    assert D.center_crop_offset(227, 224, 224) == (2, 0)         # 1.5 -> 2
    # the whole eval geometry == PIL resize + crop on a small case
    a = np.random.default_rng(2).integers(0, 256, (45, 61, 3), dtype=np.uint8)
    rh, rw = D.resize_short_side(45, 61, 36)
    y0, x0 = D.center_crop_offset(rh, rw, 32)
    ref = np.asarray(Image.fromarray(a).resize((rw, rh), Image.BILINEAR).crop((x0, y0, x0 + 32, y0 + 32)))
    assert np.array_equal(PB.resize(a, (rw, rh))[y0:y0 + 32, x0:x0 + 32], ref)


def test_numpy_bilinear_restatement_equals_pil():
    """>= 200 random cases: crops (box), downscales past 20x, upscales, shorter-side resizes, 1-pixel sides."""
    rng = np.random.default_rng(5)
    cases = 0
    for t in range(240):
        H, W = (int(v) for v in rng.integers(1, 260, 2))
        if t % 10 == 0:
            H, W = int(rng.integers(400, 900)), int(rng.integers(400, 900))
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        kind = t % 4
        if kind == 0:                                            # crop then resize, as RandomResizedCrop
            h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
            i, j = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
            S = int(rng.choice([1, 7, 32, 64]))
            ref = np.asarray(Image.fromarray(a).crop((j, i, j + w, i + h)).resize((S, S), Image.BILINEAR))
            got = PB.resize(np.ascontiguousarray(a[i:i + h, j:j + w]), (S, S))
        elif kind == 1:                                          # shorter side
            s = int(rng.integers(8, 80))
            rh, rw = D.resize_short_side(H, W, s)
            ref = np.asarray(Image.fromarray(a).resize((rw, rh), Image.BILINEAR))
            got = PB.resize(a, (rw, rh))
        elif kind == 2:                                          # independent sizes, up or down
            size = (int(rng.integers(1, 300)), int(rng.integers(1, 300)))
            ref = np.asarray(Image.fromarray(a).resize(size, Image.BILINEAR))
            got = PB.resize(a, size)
        else:                                                    # a resize with a box, the PIL-side crop
            x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
            box = (x0, y0, int(rng.integers(x0 + 1, W + 1)), int(rng.integers(y0 + 1, H + 1)))
            size = (int(rng.integers(1, 64)), int(rng.integers(1, 64)))
            ref = np.asarray(Image.fromarray(a).resize(size, Image.BILINEAR, box=box))
            got = PB.resize(a, size, box)
        assert np.array_equal(ref, got), (t, H, W)
        cases += 1
    # tall strips: Image.resize runs the vertical pass first for H > 100 W when the height shrinks
    for H, W, size in ((405, 3, (32, 32)), (568, 2, (32, 32)), (4223, 2, (224, 224)), (301, 3, (5, 300)), (300, 3, (7, 40)), (900, 2, (3, 1000))):
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        assert np.array_equal(np.asarray(Image.fromarray(a).resize(size, Image.BILINEAR)), PB.resize(a, size)), (H, W, size)
    # a 20x downscale and a 7x upscale
    a = rng.integers(0, 256, (40, 900, 3), dtype=np.uint8)
    assert np.array_equal(np.asarray(Image.fromarray(a).resize((45, 280), Image.BILINEAR)), PB.resize(a, (45, 280)))
    assert cases >= 200


def test_desc_dtype_and_workspace_query_refuse_bad_batches():
    """Host-only ABI: the descriptor layout and the workspace query's checks (no device access)."""
    from uvc_amd import _lib, ops
    assert ops.image_desc_dtype().itemsize == 64
    d = np.zeros(2, ops.image_desc_dtype())
    d["src_h"], d["src_w"], d["resize_h"], d["resize_w"] = (300, 10), (400, 2000), (224, 32), (224, 32)
    d["src_offset"] = (0, 300 * 400 * 3)
    need = 300 * 400 * 3 + 10 * 2000 * 3
    ws = ops.image_prep_workspace(d, 32, need)
    assert ws > 0 and ws % 16 == 0 and d["ws_offset"][0] == 0 and d["ws_offset"][1] > 0
    assert d["kh"].tolist() == [2 * math.ceil(400 / 224) + 1, 2 * math.ceil(2000 / 32) + 1] and d["kv"].tolist() == [5, 3]
    assert d["span0"].tolist() == [0, 0] and 0 < d["span"][0] < 300 and d["span"][1] == 10 and d["order"].tolist() == [0, 0]
    d4 = d[:1].copy()
    d4["src_h"], d4["src_w"] = 300, 2                            # taller than 100 x its width and shrinking: vertical pass first
    assert ops.image_prep_workspace(d4, 32, need) > 0 and d4["order"][0] == 1 and d4["span0"][0] == 0 and d4["span"][0] == 1  # the 32-column window reads column 0 only
    with pytest.raises(_lib.UvcHipError):
        ops.image_prep_workspace(d, 32, need - 1)                  # the second image reaches past the source
    d2 = d.copy()
    d2["win_y"][0] = 224 - 31
    with pytest.raises(_lib.UvcHipError):
        ops.image_prep_workspace(d2, 32, need)                     # window leaves the resized image
    d3 = d.copy()
    d3["resize_w"][1] = 16
    with pytest.raises(_lib.UvcHipError):
        ops.image_prep_workspace(d3, 32, need)                     # resized smaller than S


class _FakeLoader:
    """What soft_batches reads from a DeviceLoader: set_epoch and (x, target) batches (CPU tensors here)."""

    def __init__(self, sizes, classes):
        self.sizes, self.classes, self.epoch = sizes, classes, None

    def set_epoch(self, e):
        self.epoch = e

    def __iter__(self):
        for n in self.sizes:
            yield torch.zeros(n, 3, 4, 4), torch.arange(n) % self.classes


def test_soft_targets_cover_the_data_classes_and_zero_the_padded_head():
    ld = _FakeLoader([6, 5, 1], 10)
    out = list(D.soft_batches(ld, 3, None, 0.1, 10, 16))
    assert ld.epoch == 3 and [len(x) for x, _ in out] == [6, 4]          # odd batches trimmed, a batch of one skipped
    for x, y in out:
        assert y.shape == (len(x), 16) and torch.all(y[:, 10:] == 0)
        assert torch.allclose(y.sum(1), torch.ones(len(x)))
        t = torch.arange(len(x)) % 10
        assert torch.allclose(y[torch.arange(len(x)), t], torch.full((len(x),), 0.9 + 0.01))   # reference smoothing: 0.1 / 10
    y = next(iter(D.soft_batches(_FakeLoader([4], 10), 0, None, 0.1, 10)))[1]
    assert y.shape == (4, 10)


def test_train_steps_leave_out_a_last_batch_of_one():
    ds = D.ArrayDataset(np.zeros((17, 4, 4, 3), np.uint8), np.zeros(17))
    assert D.DeviceLoader(ds, 8, 4, device="cpu").train_steps() == 2                 # 8, 8, 1 -> the 1 is trimmed away
    assert len(D.DeviceLoader(ds, 8, 4, device="cpu")) == 3
    assert D.DeviceLoader(ds, 6, 4, device="cpu").train_steps() == 3                 # 6, 6, 5
    assert D.DeviceLoader(ds, 8, 4, rank=1, world=2, device="cpu").train_steps() == 1   # 9 per rank: 8, 1
    assert D.DeviceLoader(ds, 4, 4, rank=0, world=2, device="cpu").train_steps() == 2   # 9 per rank: 4, 4, 1


def test_post_train_keeps_the_reference_num_workers_default(monkeypatch):
    import uvc_amd.post_train as PT
    seen = {}

    def stop(self, argv=None, namespace=None):
        seen.update(vars(self._orig_parse(argv)))
        raise SystemExit(0)
    import argparse
    monkeypatch.setattr(argparse.ArgumentParser, "_orig_parse", argparse.ArgumentParser.parse_args, raising=False)
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", stop)
    with pytest.raises(SystemExit):
        PT.main([])
    assert seen["num_workers"] == 8 and seen["synthetic"] == 1 and seen["mixup"] == 0.8 and seen["smoothing"] == 0.1
