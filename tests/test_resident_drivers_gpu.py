"""GPU: the drivers on a packed dataset (``--packed_dir``) and with the dataset resident on the device (``--resident 1``): Stage 1 from
the pack, resident or not, is bit for bit Stage 1 from the folders the pack was made from; Stage 2 and ``compact eval`` take the same
flags; image folders without a pack are told to pack first."""
import glob
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MICRO = '{"patch_size": 16, "embed_dim": 128, "depth": 2, "num_heads": 2}'


def make_tree(root, seed=0):
    """2 classes, 12 train and 6 val PNGs of ragged sizes."""
    rng = np.random.default_rng(seed)
    for split, per_class in (("train", 6), ("val", 3)):
        for c in range(2):
            d = os.path.join(root, split, f"n{c:08d}")
            os.makedirs(d)
            for k in range(per_class):
                a = rng.integers(0, 256, (int(rng.integers(40, 120)), int(rng.integers(40, 120)), 3), dtype=np.uint8)
                Image.fromarray(a).save(os.path.join(d, f"img_{k}.png"))


def stage1_argv(out, name, data_dir, extra=()):
    return ["--name", name, "--output_dir", str(out), "--model_type", "custom", "--model_cfg", MICRO, "--img_size", "64", "--num_classes", "16",
            "--train_batch_size", "8", "--eval_batch_size", "4", "--num_epochs", "1", "--warmup_epochs", "1", "--log_interval", "1",
            "--gating_interval", "2", "--warmup_steps", "1", "--precision", "fp32", "--seed", "11", "--synthetic", "0", "--dataset", "imagenet",
            "--data_dir", str(data_dir), "--num_workers", "4", "--zlr_schedule_list", "1"] + list(extra)


def stage1_record(out, name, text):
    """What a Stage-1 run leaves: both epochs' checkpoints (weights and masks), the s / r / gating logs, the logged losses and validations."""
    d = os.path.join(str(out), name)
    rec = {"ckpt": [torch.load(os.path.join(d, f"custom_{e}.pth.tar"), map_location="cpu") for e in (1, 2)]}
    for key in ("s", "r", "gating"):
        files = glob.glob(os.path.join(d, f"{key}_*.json"))
        assert len(files) == 1
        rec[key] = json.load(open(files[0]))
    rec["log"] = re.findall(r"\[\d+ / \d+ Steps\] \[LR: [^|]+\| Loss: [^\]]+\] resource \S+", text) + \
        re.findall(r"Valid (?:Loss|Accuracy): \S+", text)
    return rec


def same_tree(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same_tree(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same_tree(x, y) for x, y in zip(a, b))
    return a == b


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The folders, their packs (made by the command line) and the Stage-1 run from the folders, shared by the tests below."""
    tmp = tmp_path_factory.mktemp("resident_drivers")
    data, packs = tmp / "imagenet", tmp / "packs"
    make_tree(str(data))
    os.makedirs(packs)
    for split, n in (("train", 12), ("val", 6)):
        r = subprocess.run([sys.executable, "-m", "uvc_amd.packed", "pack", "--dataset", "imagenet", "--data_dir", str(data), "--split", split,
                            "--output", str(packs / f"{split}.uvcpack"), "--num_workers", "2"], cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        info = json.loads(r.stdout.strip().splitlines()[-1])
        assert info["n"] == n and info["classes"] == 2 and info["max_side"] == 0
    return dict(tmp=tmp, data=data, packs=packs)


@pytest.fixture(scope="module")
def folder_stage1(runs):
    import contextlib
    import io
    from uvc_amd import cli
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        tr = cli.main(stage1_argv(runs["tmp"] / "run", "folders", runs["data"]))
    assert tr.global_step == 4                                               # 12 images at batch 8: 8 + 4, two epochs
    return stage1_record(runs["tmp"] / "run", "folders", buf.getvalue())


@pytest.fixture
def built(monkeypatch):
    """Records the loaders that build_loaders hands the drivers: [(train, test), ...]."""
    from uvc_amd import data as D
    seen, real = [], D.build_loaders

    def spy(*args, **kw):
        seen.append(real(*args, **kw))
        return seen[-1]
    monkeypatch.setattr(D, "build_loaders", spy)
    return seen


@pytest.mark.parametrize("resident", [1, 0])
def test_stage1_from_the_pack_equals_stage1_from_the_folders(runs, folder_stage1, resident, capsys, built):
    from uvc_amd import cli
    from uvc_amd.data import DeviceLoader
    from uvc_amd.packed import PackedDataset, ResidentLoader
    name = f"packed_r{resident}"
    # --data_dir points nowhere: with --packed_dir the folders are not read
    tr = cli.main(stage1_argv(runs["tmp"] / "run", name, runs["tmp"] / "nowhere", ["--packed_dir", str(runs["packs"]), "--resident", str(resident)]))
    rec = stage1_record(runs["tmp"] / "run", name, capsys.readouterr().out)
    assert tr.global_step == 4 and len(rec["log"]) == 4 + 4
    assert rec["log"] == folder_stage1["log"]
    for key in ("s", "r", "gating"):
        assert rec[key] == folder_stage1[key], key
    assert same_tree(rec["ckpt"], folder_stage1["ckpt"])
    assert len(built) == 1
    for loader in built[0]:                                                  # the flags chose the loader and the dataset, not only the result
        assert type(loader) is (ResidentLoader if resident else DeviceLoader) and type(loader.dataset) is PackedDataset


def test_stage2_and_compact_eval_take_the_flags(runs, folder_stage1, capsys, built):
    from uvc_amd import compact, post_train
    from uvc_amd.data import DeviceLoader
    from uvc_amd.packed import ResidentLoader
    ckpt = str(runs["tmp"] / "run" / "folders" / "custom_2.pth.tar")

    def stage2(name, data_flags):
        torch.manual_seed(5)              # no --teacher-path: the teacher keeps its init, drawn from torch's global generator
        tr = post_train.main(["--model_type", "custom", "--model_cfg", MICRO, "--img_size", "64", "--num_classes", "16", "--train_batch_size", "8",
                              "--eval_batch_size", "4", "--epochs", "1", "--precision", "fp32", "--checkpoint_dir", ckpt, "--output_dir",
                              str(runs["tmp"] / "run"), "--name", name, "--learning_rate", "0.01", "--warmup_epochs", "0", "--compact_multiple", "64",
                              "--synthetic", "0", "--dataset", "imagenet", "--num_workers", "2"] + data_flags)
        res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        return tr.model._flat.detach().cpu(), res

    packed = ["--packed_dir", str(runs["packs"]), "--resident", "1", "--data_dir", str(runs["tmp"] / "nowhere")]
    flat_f, res_f = stage2("s2_folders", ["--data_dir", str(runs["data"])])
    flat_p, res_p = stage2("s2_packed", packed)
    assert res_p["steps"] == 2 and res_p == res_f
    assert torch.equal(flat_p, flat_f)
    assert [type(l) for pair in built for l in pair] == [DeviceLoader] * 2 + [ResidentLoader] * 2

    def compact_eval(data_flags):
        compact.main(["eval", "--model_type", "custom", "--model_cfg", MICRO, "--img_size", "64", "--num_classes", "16", "--precision", "fp32",
                      "--checkpoint_dir", ckpt, "--mlp_multiple", "64", "--eval_batch_size", "4", "--synthetic", "0", "--dataset", "imagenet",
                      "--num_workers", "2"] + data_flags)
        return json.loads(capsys.readouterr().out.strip().splitlines()[-1])["top1"]

    assert compact_eval(packed) == compact_eval(["--data_dir", str(runs["data"])])
    # compact eval builds the loader it iterates and no other: --resident 1 uploads no train store
    assert built[2][0] is None and type(built[2][1]) is ResidentLoader and built[3][0] is None and type(built[3][1]) is DeviceLoader


def test_resident_image_folders_without_a_pack_are_told_to_pack_first(runs):
    from uvc_amd import cli
    with pytest.raises(ValueError, match="pack first"):
        cli.main(stage1_argv(runs["tmp"] / "run", "refused", runs["data"], ["--resident", "1"]))
