"""CPU: the packed dataset file (uvc_amd/packed.py): round trip against ImageFolder, max_side against PIL, the refusals of a damaged
file, the info line, offsets past 2^31 in a sparse file, and the --packed_dir / --resident flags of the four parsers."""
import json
import os
import struct

import numpy as np
import pytest
from PIL import Image

from uvc_amd import data as D
from uvc_amd import packed as P

SIZES = [(17, 31), (40, 25), (8, 8), (33, 64), (21, 90), (50, 50), (19, 23)]      # (h, w); short sides on both sides of 20


def write_folder(root, seed=0):
    """3 classes, 7 PNGs of different sizes from seeded arrays; one greyscale, one RGBA."""
    rng = np.random.default_rng(seed)
    for k, (h, w) in enumerate(SIZES):
        d = root / f"class_{k % 3}"
        d.mkdir(parents=True, exist_ok=True)
        if k == 2:
            im = Image.fromarray(rng.integers(0, 256, (h, w), dtype=np.uint8), "L")
        elif k == 4:
            im = Image.fromarray(rng.integers(0, 256, (h, w, 4), dtype=np.uint8), "RGBA")
        else:
            im = Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        im.save(d / f"im{k}.png")
    return D.ImageFolder(str(root))


@pytest.fixture(scope="module")
def folder_and_pack(tmp_path_factory):
    root = tmp_path_factory.mktemp("packed")
    ds = write_folder(root / "train")
    path = str(root / "train.uvcpack")
    P.write_pack(ds, path, num_workers=3)
    return ds, path


def test_round_trip_equals_image_folder(folder_and_pack):
    ds, path = folder_and_pack
    pk = P.PackedDataset(path)
    assert len(pk) == len(ds) == 7
    assert np.array_equal(pk.targets, ds.targets) and pk.targets.dtype == np.int64
    assert pk.classes == ds.classes == ["class_0", "class_1", "class_2"]
    for i in range(7):
        a = ds.load(i)
        assert np.array_equal(pk.load(i), a)
        assert tuple(pk.hw[i]) == a.shape[:2]
        assert np.shares_memory(pk.load(i), pk.pixels)                       # a view into the memmap, not a copy
    assert sorted(tuple(v) for v in pk.hw.tolist()) == sorted(SIZES)
    assert pk.offsets.dtype == np.int64 and pk.offsets[0] == 0 and pk.offsets[-1] == sum(h * w * 3 for h, w in SIZES)
    assert pk.header["arrays"]["pixels"]["pos"] % 4096 == 0 and pk.header["max_side"] == 0


def test_max_side_resizes_only_larger_images(folder_and_pack, tmp_path):
    ds, _ = folder_and_pack
    path = str(tmp_path / "m.uvcpack")
    P.write_pack(ds, path, max_side=20)
    pk = P.PackedDataset(path)
    assert pk.max_side == 20 and pk.header["max_side"] == 20
    changed = 0
    for i in range(len(ds)):
        a = ds.load(i)
        h, w = a.shape[:2]
        if min(h, w) > 20:
            nh, nw = D.resize_short_side(h, w, 20)
            want = np.asarray(Image.fromarray(a).resize((nw, nh), Image.BILINEAR))
            assert min(nh, nw) == 20
            changed += 1
        else:
            want = a
        assert np.array_equal(pk.load(i), want), i
    assert changed == 4                                                      # short sides 25, 33, 21, 50; 17, 8 and 19 stay


def _copy_with(path, out, edit):
    raw = bytearray(open(path, "rb").read())
    raw = edit(raw) or raw
    open(out, "wb").write(raw)
    return str(out)


def test_damaged_files_are_refused(folder_and_pack, tmp_path):
    _, path = folder_and_pack
    good = P.PackedDataset(path)
    size = os.path.getsize(path)
    with pytest.raises(ValueError, match="shorter"):                         # truncated inside the pixel blob
        P.PackedDataset(_copy_with(path, tmp_path / "t.uvcpack", lambda r: r[:size - 10]))
    with pytest.raises(ValueError, match="shorter"):                         # truncated inside the header
        P.PackedDataset(_copy_with(path, tmp_path / "t2.uvcpack", lambda r: r[:40]))
    with pytest.raises(ValueError, match="magic"):
        P.PackedDataset(_copy_with(path, tmp_path / "m.uvcpack", lambda r: r.__setitem__(slice(0, 4), b"NOPE")))
    with pytest.raises(ValueError, match="version"):
        P.PackedDataset(_copy_with(path, tmp_path / "v.uvcpack", lambda r: r.__setitem__(slice(8, 12), struct.pack("<I", 2))))
    opos = good.header["arrays"]["offsets"]["pos"]

    def swap(r):                                                             # offsets[2] < offsets[1]: decreasing
        r[opos + 8:opos + 16], r[opos + 16:opos + 24] = r[opos + 16:opos + 24], r[opos + 8:opos + 16]
    with pytest.raises(ValueError, match="offsets"):
        P.PackedDataset(_copy_with(path, tmp_path / "o.uvcpack", swap))
    hpos = good.header["arrays"]["hw"]["pos"]
    with pytest.raises(ValueError, match="offsets"):                         # non-decreasing but not what hw says
        P.PackedDataset(_copy_with(path, tmp_path / "h.uvcpack", lambda r: r.__setitem__(slice(hpos, hpos + 4), struct.pack("<i", 1))))


def test_info_line(folder_and_pack, capsys):
    _, path = folder_and_pack
    P.main(["info", path])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == dict(n=7, classes=3, pixel_bytes=sum(h * w * 3 for h, w in SIZES), max_side=0, smallest_side=8, largest_side=90)


def test_pack_cli_on_a_folder(tmp_path, capsys):
    write_folder(tmp_path / "data" / "val", seed=1)
    out = str(tmp_path / "val.uvcpack")
    P.main(["pack", "--dataset", "imagenet", "--data_dir", str(tmp_path / "data"), "--split", "val", "--output", out, "--max_side", "20",
            "--num_workers", "2"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["n"] == 7 and line["classes"] == 3 and line["max_side"] == 20 and line["smallest_side"] == 8
    assert line == P.PackedDataset(out).info()


def test_offsets_past_2_gib_survive_the_format(tmp_path):
    """Synthetic sizes, a sparse blob: only the header arithmetic is exercised, nothing of the blob is allocated."""
    path = str(tmp_path / "big.uvcpack")
    sizes = [(30000, 30000), (7, 5), (30000, 30000), (3, 3)]               # 2.7 GB each: offsets pass 2^31 and 2^32
    wr = P.PackWriter(path, [0, 1, 2, 1], classes=["a", "b", "c"], source="synthetic")
    for h, w in sizes:
        wr.skip(h, w)
    wr.close()
    pk = P.PackedDataset(path)
    want = np.concatenate([[0], np.cumsum([h * w * 3 for h, w in sizes])])
    assert np.array_equal(pk.offsets, want) and pk.offsets[2] > (1 << 31) and pk.offsets[3] > (1 << 32)
    assert pk.pixel_bytes == int(want[-1]) and os.path.getsize(path) == pk.header["arrays"]["pixels"]["pos"] + int(want[-1])
    assert pk.header["file_bytes"] == os.path.getsize(path)
    assert pk.load(3).shape == (3, 3, 3) and pk.load(2).shape == (30000, 30000, 3)
    assert int(pk.load(3).sum()) == 0 and int(pk.load(2)[29999, 29999].sum()) == 0     # holes read as zeros, at the right 64-bit places
    assert pk.info()["largest_side"] == 30000
    with open(path, "r+b") as f:                                             # one byte short at 5.4 GB is still noticed
        f.truncate(os.path.getsize(path) - 1)
    with pytest.raises(ValueError, match="shorter"):
        P.PackedDataset(path)


def test_all_four_parsers_take_the_flags():
    from uvc_amd import cli, compact, post_train
    import argparse
    s1 = cli.build_parser()
    s2 = post_train.add_stage2_flags(argparse.ArgumentParser())
    cp = compact._parser()
    parsed = [s1.parse_args([]), s2.parse_args([]), cp.parse_args(["eval"]), cp.parse_args(["finetune", "--compact", "c", "--output", "o"])]
    for a in parsed:
        assert a.packed_dir is None and a.resident == 0
    on = ["--packed_dir", "P", "--resident", "1"]
    parsed = [s1.parse_args(on), s2.parse_args(on), cp.parse_args(["eval"] + on),
              cp.parse_args(["finetune", "--compact", "c", "--output", "o"] + on)]
    for a in parsed:
        assert a.packed_dir == "P" and a.resident == 1


def test_resident_needs_a_pack_for_image_folders(tmp_path):
    import argparse
    args = argparse.Namespace(dataset="imagenet", data_dir=str(tmp_path), img_size=32, train_batch_size=4, eval_batch_size=4, num_classes=8,
                              packed_dir=None, resident=1)
    with pytest.raises(ValueError, match="pack first"):
        D.build_loaders(args)


def test_write_pack_keeps_the_order_past_its_window_and_removes_a_failed_pack(tmp_path):
    """More images than the decode window (4 x threads) come out in order; a dataset whose load() fails leaves no partial file."""
    rng = np.random.default_rng(1)
    arr = D.ArrayDataset(rng.integers(0, 256, (21, 4, 5, 3), dtype=np.uint8), np.arange(21))
    path = str(tmp_path / "many.uvcpack")
    P.write_pack(arr, path, num_workers=2)                                   # window of 8
    pk = P.PackedDataset(path)
    assert all(np.array_equal(pk.load(i), arr.images[i]) for i in range(21)) and np.array_equal(pk.targets, np.arange(21))

    class Broken:
        targets = np.arange(21)

        def load(self, i):
            if i == 13:
                raise OSError("unreadable image")
            return arr.images[i]
    bad = str(tmp_path / "bad.uvcpack")
    with pytest.raises(OSError, match="unreadable"):
        P.write_pack(Broken(), bad, num_workers=2)
    assert not os.path.exists(bad)
