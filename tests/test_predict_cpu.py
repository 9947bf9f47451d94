"""CPU: the host side of ``python -m uvc_amd.compact predict`` -- the parser, the directory walk, the class files, the patch-row index rule
uvc_image_prep_patches stores by (include/uvc_data.h) and the float64 top-k reference the kernel tests hold uvc_logits_topk to."""
import json
import os

import numpy as np
import pytest

from uvc_amd import compact as CP
from uvc_amd import data as D


def parse(*argv):
    return CP._parser().parse_args(["predict", *argv])


def test_parser_defaults():
    a = parse("--compact", "m.compact.pt", "--images", "a.png", "dir")
    assert a.cmd == "predict" and a.compact == "m.compact.pt" and a.images == ["a.png", "dir"]
    assert (a.topk, a.batch_size, a.num_workers, a.precision, a.preset) == (5, 64, 8, "bf16", "imagenet")
    assert (a.interpolation, a.crop_pct, a.classes, a.num_labels, a.output) == ("bilinear", None, None, None, None)
    assert a.fused_input == CP.FUSED_INPUT_DEFAULT and a.fused_input in (0, 1)
    a = parse("--compact", "m", "--images", "x", "--topk", "16", "--preset", "cifar", "--crop_pct", "0.9", "--interpolation", "bicubic",
              "--num_labels", "10", "--output", "p.jsonl")
    assert (a.topk, a.preset, a.crop_pct, a.interpolation, a.num_labels, a.output) == (16, "cifar", 0.9, "bicubic", 10, "p.jsonl")


@pytest.mark.parametrize("argv", [["--images", "a.png"], ["--compact", "m"], ["--compact", "m", "--images"],
                                  ["--compact", "m", "--images", "a", "--topk", "0"], ["--compact", "m", "--images", "a", "--topk", "17"],
                                  ["--compact", "m", "--images", "a", "--crop_pct", "1.5"], ["--compact", "m", "--images", "a", "--crop_pct", "0"],
                                  ["--compact", "m", "--images", "a", "--preset", "coco"],
                                  ["--compact", "m", "--images", "a", "--interpolation", "nearest"],
                                  ["--compact", "m", "--images", "a", "--checkpoint_dir", "dense.pt"]],
                         ids=["no_compact", "no_images", "empty_images", "topk_0", "topk_17", "crop_pct_1.5", "crop_pct_0", "preset", "interpolation",
                              "dense_checkpoint"])
def test_parser_refusals(argv, capsys):
    with pytest.raises(SystemExit) as e:
        parse(*argv)
    assert e.value.code == 2
    capsys.readouterr()


def test_directory_walk_order_and_extension_filter(tmp_path):
    for rel in ["b/2.png", "b/10.JPG", "a/z.jpeg", "a/sub/k.bmp", "a/sub/notes.txt", "a/A.webp", "top.png", "readme.md", "c/deep/er/x.tif"]:
        f = tmp_path / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_bytes(b"")
    lone = tmp_path / "lone.dat"                                   # a file named outright is taken whatever its extension
    lone.write_bytes(b"")
    got = D.list_images([str(tmp_path / "b"), str(lone), str(tmp_path)])
    rel = [os.path.relpath(p, tmp_path).replace(os.sep, "/") for p in got]
    assert rel == ["b/10.JPG", "b/2.png", "lone.dat",
                   "top.png", "a/A.webp", "a/z.jpeg", "a/sub/k.bmp", "b/10.JPG", "b/2.png", "c/deep/er/x.tif"]
    with pytest.raises(FileNotFoundError):
        D.list_images([str(tmp_path / "missing.png")])
    ds = D.FileListDataset(got)
    assert len(ds) == len(got) and ds.paths == got and ds.targets.tolist() == [0] * len(got)


def test_file_list_dataset_loads_rgb_and_tolerates_on_request(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(0)
    Image.fromarray(rng.integers(0, 256, (5, 7), dtype=np.uint8), "L").save(tmp_path / "g.png")
    Image.fromarray(rng.integers(0, 256, (4, 3, 4), dtype=np.uint8), "RGBA").save(tmp_path / "a.png")
    (tmp_path / "bad.png").write_bytes((tmp_path / "g.png").read_bytes()[:20])
    paths = [str(tmp_path / n) for n in ("g.png", "a.png", "bad.png")]
    ds = D.FileListDataset(paths, tolerant=True)
    for i, shape in enumerate([(5, 7, 3), (4, 3, 3), (1, 1, 3)]):
        a = ds.load(i)
        assert a.dtype == np.uint8 and a.shape == shape
        if i < 2:
            assert np.array_equal(a, np.asarray(Image.open(paths[i]).convert("RGB")))
    assert list(ds.errors) == [2] and ds.errors[2]
    with pytest.raises(Exception):
        D.FileListDataset(paths).load(2)


def test_class_files_as_text_and_as_json(tmp_path):
    t, j = tmp_path / "c.txt", tmp_path / "c.json"
    t.write_text("tench\ngreat white shark\n\n  hen \n")
    j.write_text(json.dumps(["tench", "great white shark", "hen"]))
    assert CP.read_classes(t) == CP.read_classes(j) == ["tench", "great white shark", "hen"]
    (tmp_path / "d.json").write_text("[1, 2")
    with pytest.raises(ValueError):
        CP.read_classes(tmp_path / "d.json")


@pytest.mark.parametrize("S,P", [(32, 16), (48, 8), (224, 16)])
def test_patch_row_index_rule(S, P):
    """Pixel (c, y, x) goes to row (y/P)(S/P) + x/P, column c P P + (y%P) P + x%P: the numpy restatement against a loop over pixels."""
    C, G = 3, S // P
    image = np.arange(C * S * S, dtype=np.int64).reshape(C, S, S)
    rows = image.reshape(C, G, P, G, P).transpose(1, 3, 0, 2, 4).reshape(G * G, C * P * P)
    loop = np.full((G * G, C * P * P), -1, dtype=np.int64)
    for c in range(C):
        for y in range(S):
            for x in range(S):
                loop[(y // P) * G + x // P, c * P * P + (y % P) * P + x % P] = image[c, y, x]
    assert np.array_equal(rows, loop)
    assert sorted(loop.reshape(-1).tolist()) == list(range(C * S * S))      # a bijection: every element written once


def test_topk_reference_on_hand_worked_rows():
    ln = np.log
    rows = np.array([[ln(1.0), ln(3.0), ln(2.0), ln(2.0), 50.0],            # p = 1/8, 3/8, 2/8, 2/8 over 4 valid columns; 50 is padding
                     [0.0, 0.0, 0.0, 0.0, 99.0],                           # all equal: index order
                     [ln(4.0), ln(1.0), ln(1.0), ln(4.0), -99.0]])         # two equal maxima, then two equal minima
    p, i = CP.topk_reference(rows, 3, n_valid=4)
    assert i.dtype == np.int32 and i.tolist() == [[1, 2, 3], [0, 1, 2], [0, 3, 1]]
    assert np.allclose(p, [[3 / 8, 2 / 8, 2 / 8], [1 / 4, 1 / 4, 1 / 4], [0.4, 0.4, 0.1]], rtol=1e-12, atol=0)
    p, i = CP.topk_reference(rows[0], 1)                                   # a single row, every column valid: the large one takes it all
    assert i.tolist() == [[4]] and abs(p[0, 0] - 1.0) < 1e-15
    z = np.zeros((1, 12))
    z[0, 7] = z[0, 3] = 2.0                                                # equal maxima at 7 and 3: 3 first
    assert CP.topk_reference(z, 2)[1].tolist() == [[3, 7]]
    p, _ = CP.topk_reference(np.array([[80.0, -80.0, 0.0]]), 3)            # the max is subtracted: no overflow
    assert np.isfinite(p).all() and p[0, 0] == 1.0
