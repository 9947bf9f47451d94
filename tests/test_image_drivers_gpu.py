"""GPU: both command-line drivers on real image data (``--synthetic 0``): Stage 1 on an ImageFolder tree (train/ + val/) with a
short last batch, on fake CIFAR-10 pickles, and Stage 2 with Mixup from the Stage-1 checkpoint, all in process."""
import glob
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

MICRO = '{"patch_size": 16, "embed_dim": 128, "depth": 2, "num_heads": 2}'


def make_imagenet_tree(root, n_train=(5, 4, 4), n_val=(2, 2, 1), seed=0):
    rng = np.random.default_rng(seed)
    for split, counts in (("train", n_train), ("val", n_val)):
        for c, n in enumerate(counts):
            d = os.path.join(root, split, f"n{c:08d}")
            os.makedirs(d)
            for k in range(n):
                a = rng.integers(0, 256, (int(rng.integers(40, 120)), int(rng.integers(40, 120)), 3), dtype=np.uint8)
                Image.fromarray(a).save(os.path.join(d, f"img_{k}.JPEG" if k % 2 else f"img_{k}.png"))


def stage1_argv(out, name, data_dir, dataset, extra=()):
    return ["--name", name, "--output_dir", str(out), "--model_type", "custom", "--model_cfg", MICRO, "--img_size", "64", "--num_classes", "16",
            "--train_batch_size", "8", "--eval_batch_size", "4", "--num_epochs", "1", "--warmup_epochs", "1", "--log_interval", "1",
            "--gating_interval", "2", "--warmup_steps", "1", "--precision", "fp32", "--seed", "11", "--synthetic", "0", "--dataset", dataset,
            "--data_dir", str(data_dir), "--num_workers", "4", "--zlr_schedule_list", "1"] + list(extra)


def test_stage1_imagenet_folder_then_stage2(tmp_path, capsys):
    from uvc_amd import cli, post_train
    data = tmp_path / "imagenet"
    make_imagenet_tree(str(data))
    out = tmp_path / "run"
    tr = cli.main(stage1_argv(out, "s1", data, "imagenet"))
    text = capsys.readouterr().out
    # 13 training images at batch 8: batches of 8 and 5; the 5 loses its last sample (odd trim) and still trains
    assert tr.args.steps_per_epoch == 2 and tr.t_total == 2
    assert tr.epoch == 2 and tr.global_step == 4
    assert text.count("Valid Accuracy:") == 2 and "Start [Epoch 2] at Stage UVC Train" in text
    d = out / "s1"
    assert os.path.exists(d / "custom_1.pth.tar") and os.path.exists(d / "custom_2.pth.tar")
    for key in ("s", "r", "gating"):
        files = glob.glob(str(d / f"{key}_*.json"))
        assert len(files) == 1 and sorted(json.load(open(files[0])), key=int) == ["3", "4"], key
    assert torch.isfinite(tr.model._flat).all()
    # ---- Stage 2 from that checkpoint on the same folders, Mixup / CutMix on (the reference's defaults)
    tr2 = post_train.main(["--model_type", "custom", "--model_cfg", MICRO, "--img_size", "64", "--num_classes", "16", "--train_batch_size", "8",
                           "--eval_batch_size", "4", "--epochs", "2", "--precision", "fp32", "--checkpoint_dir", str(d / "custom_2.pth.tar"),
                           "--output_dir", str(out), "--name", "s2", "--learning_rate", "0.01", "--warmup_epochs", "1", "--compact_multiple", "64",
                           "--synthetic", "0", "--dataset", "imagenet", "--data_dir", str(data), "--num_workers", "2"])
    text2 = capsys.readouterr().out
    assert "mixup active: True" in text2
    assert tr2.global_step == 4 and "[Stage 2] epoch 1" in text2
    res = json.loads(text2.strip().splitlines()[-1])
    assert res["steps"] == 4 and 0.0 < res["best_acc"] <= 100.0 + 1e-3
    assert glob.glob(str(out / "s2" / "custom_*.pth.tar")), "save-best policy wrote no checkpoint"
    assert torch.isfinite(tr2.model._flat).all()


def test_stage1_cifar10_pickles(tmp_path, capsys):
    import test_image_data_cpu as T
    from uvc_amd import cli
    T.write_fake_cifar(str(tmp_path / "cifar"), "cifar10", n_train=19, n_test=6)
    tr = cli.main(stage1_argv(tmp_path / "run", "c10", tmp_path / "cifar", "cifar10", ["--mixup", "0", "--cutmix", "0"]))
    text = capsys.readouterr().out
    assert tr.args.num_classes == 16 and tr.args.steps_per_epoch == 3          # 19 images at batch 8: 8, 8, 3 (-> 2)
    assert tr.global_step == 6 and text.count("Valid Accuracy:") == 2 and "mixup active: False" in text
    assert torch.isfinite(tr.model._flat).all()


def test_cifar_mixup_targets_cover_the_data_classes(tmp_path):
    """A padded head (16 logits for CIFAR-10): Mixup / CutMix and smoothing act over the 10 data classes, the padded columns are zero."""
    import argparse
    import test_image_data_cpu as T
    from uvc_amd import data as D
    T.write_fake_cifar(str(tmp_path), "cifar10", n_train=19, n_test=6)
    args = argparse.Namespace(dataset="cifar10", data_dir=str(tmp_path), img_size=32, train_batch_size=8, eval_batch_size=4, num_workers=2,
                              seed=0, num_classes=1000, mixup=0.8, cutmix=1.0, cutmix_minmax=None, mixup_prob=1.0, mixup_switch_prob=0.5,
                              mixup_mode="batch", smoothing=0.1)
    train, _ = D.build_loaders(args)
    assert args.num_classes == 16 and args.data_classes == 10 and train.train_steps() == 3
    np.random.seed(0)
    mix = D.real_mixup(args)
    n = 0
    for x, y in D.soft_batches(train, 0, mix, args.smoothing, args.data_classes, args.num_classes):
        assert y.shape == (len(x), 16) and bool((y[:, 10:] == 0).all())
        assert torch.allclose(y.sum(1), torch.ones(len(x), device=y.device), atol=1e-6)
        assert float(y[:, :10].min()) >= 0.1 / 10 - 1e-7                  # every data class keeps the reference's 0.1 / 10
        n += 1
    assert n == 3
