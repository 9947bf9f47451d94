"""GPU: classifying image files with a compact model (uvc_amd.compact.predict and the ``predict`` subcommand) -- the forward from patch
rows against the forward from images, predict() over PIL-written files against the loader + model + top-k it is made of and against the
float64 host pipeline, both input paths, the padding logits of a wide head, and the command's JSON lines."""
import json

import numpy as np
import pytest
import torch
from PIL import Image

from uvc_amd import compact as CP
from uvc_amd import data as D
from uvc_amd import ops

pytestmark = pytest.mark.gpu

BS = 3


@pytest.fixture(scope="module")
def export():
    """The small compact model of test_finetune_command_end_to_end: img 64, patch 16, embed 128, depth 3, 16 classes, synthetic masks."""
    from uvc_amd.model_distilled import DistilledVisionTransformer
    torch.manual_seed(0)
    m = DistilledVisionTransformer(enable_dist=0, img_size=64, patch_size=16, embed_dim=128, depth=3, num_heads=2, num_classes=16,
                                   precision="fp32", device="cuda")
    masks = CP.synthetic_masks(3, 128, 512, seed=3)
    masks["blocks.1.attn.proj.mask"][:, 64:] = 0
    CP.apply_synthetic_masks(m, masks)
    return CP.export_compact(m)


@pytest.fixture(scope="module")
def models(export):
    return {p: CP.CompactVisionTransformer(export, precision=p) for p in ("fp32", "bf16")}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Seven files: PNG and JPEG, one grayscale, one RGBA, 20 x 31 to 300 x 200."""
    d = tmp_path_factory.mktemp("images")
    rng = np.random.default_rng(7)
    spec = [("a.png", (31, 20), "RGB"), ("b.jpg", (200, 300), "RGB"), ("c.png", (64, 64), "L"), ("d.png", (45, 80), "RGBA"),
            ("e.jpeg", (120, 90), "RGB"), ("f.png", (300, 200), "RGB"), ("g.jpg", (50, 50), "L")]
    out = []
    for name, (h, w), mode in spec:
        a = rng.integers(0, 256, (h, w) if mode == "L" else (h, w, len(mode)), dtype=np.uint8)
        Image.fromarray(a, mode).save(d / name)
        out.append(str(d / name))
    return out


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_forward_from_patch_rows_equals_forward_from_the_image(models, prec):
    cm = models[prec]
    x = torch.randn(5, 3, 64, 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    td = torch.float32 if prec == "fp32" else torch.bfloat16
    rows = torch.empty(5 * 16, 3 * 256, dtype=td, device="cuda")
    ops.patchify(x, rows, 16, ops.UVC_F32 if prec == "fp32" else ops.UVC_BF16)
    with torch.no_grad():
        want, macs = cm(x)
        got, macs_p = cm(patches=rows)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and macs == macs_p
    wrong = torch.float32 if prec == "bf16" else torch.bfloat16
    for bad in (rows.to(wrong), rows[:-1], rows[:, :-1].contiguous(), rows.view(5 * 8, -1)):
        with pytest.raises(AssertionError):
            cm(patches=bad)
    with pytest.raises(ValueError):
        cm(x, patches=rows)


def loader_pipeline(cm, files, topk, num_labels, **kw):
    """predict()'s parts put together by hand: DeviceLoader(train=False) batches of the files, the model, logits_topk."""
    ds = D.FileListDataset(files)
    probs, index, logits = [], [], []
    for x, _ in D.DeviceLoader(ds, BS, 64, train=False, num_workers=2, **kw):
        with torch.no_grad():
            lg, _ = cm(x)
        p, i = ops.logits_topk(lg, topk, num_labels)
        probs.append(p.cpu()); index.append(i.cpu()); logits.append(lg.cpu())
    return torch.cat(probs), torch.cat(index), torch.cat(logits)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_predict_over_files(models, export, files, prec):
    cm = models[prec]
    recs = {f: list(CP.predict(cm, files, topk=5, batch_size=BS, num_workers=2, fused_input=f)) for f in (True, False)}
    assert recs[True] == recs[False]                              # floats compared exactly: the same records bit for bit
    got = recs[True]
    assert [r["file"] for r in got] == files and all("error" not in r and len(r["top"]) == 5 for r in got)
    assert all(e["label"] is None for r in got for e in r["top"])
    probs, index, logits = loader_pipeline(cm, files, 5, 16)
    assert len(probs) == 7
    assert [[e["index"] for e in r["top"]] for r in got] == index.tolist()
    gp = torch.tensor([[e["prob"] for e in r["top"]] for r in got], dtype=torch.float64)
    assert torch.equal(gp, probs.double())                        # a float32 survives the trip through a Python float
    if prec == "fp32":
        x = D.host_reference_batch(D.FileListDataset(files), list(range(7)), 64, False, 0, 0, D.IMAGENET_MEAN, D.IMAGENET_STD)
        ref = CP.reference_forward(export, x.double())
        err = float((logits.double() - ref).abs().max() / ref.abs().max())
        assert err <= 1e-3, err                                   # test_compact_gpu.compare's float32 tolerance
        wp, wi = CP.topk_reference(logits.numpy(), 5)
        assert np.array_equal(wi, index.numpy())


def test_presets_and_filters_follow_the_loaders(models, files):
    cm = models["fp32"]
    got = list(CP.predict(cm, files, topk=3, batch_size=BS, preset="cifar", interpolation="bicubic", num_workers=2))
    _, index, _ = loader_pipeline(cm, files, 3, 16, eval="square", mean=D.CIFAR_MEAN, std=D.CIFAR_STD, interpolation="bicubic")
    assert [[e["index"] for e in r["top"]] for r in got] == index.tolist()
    got = list(CP.predict(cm, files, topk=3, batch_size=BS, crop_pct=0.9, num_workers=2))
    probs, index, _ = loader_pipeline(cm, files, 3, 16, crop_pct=0.9)
    assert [[e["prob"] for e in r["top"]] for r in got] == probs.double().tolist()
    for bad in (dict(topk=0), dict(topk=17), dict(crop_pct=1.5), dict(preset="coco"), dict(interpolation="nearest"), dict(num_labels=17),
                dict(num_labels=3, topk=4), dict(classes=["a", "b"], num_labels=3)):
        with pytest.raises(ValueError):
            list(CP.predict(cm, files[:1], **bad))
    assert list(CP.predict(cm, [])) == []


def test_padding_logits_are_never_reported(export, files):
    """num_labels = 10 on the 16-wide head: with the padding rows of the head set large, an argmax over all logits would pick them."""
    ex = dict(export, state_dict={k: v.clone() for k, v in export["state_dict"].items()})
    ex["state_dict"]["head.bias"][10:] = 50.0
    cm = CP.CompactVisionTransformer(ex, precision="fp32")
    names = [f"class{i}" for i in range(10)]
    got = list(CP.predict(cm, files, topk=10, batch_size=BS, classes=names, num_workers=2))
    assert all(sorted(e["index"] for e in r["top"]) == list(range(10)) for r in got)
    assert all(e["label"] == names[e["index"]] for r in got for e in r["top"])
    assert all(abs(sum(e["prob"] for e in r["top"]) - 1.0) < 1e-5 for r in got)       # the padding took no part in the sum
    wide = list(CP.predict(cm, files, topk=1, batch_size=BS, num_workers=2))
    assert all(r["top"][0]["index"] >= 10 for r in wide)


def test_command(export, files, tmp_path, capsys):
    model, out, classes = tmp_path / "m.compact.pt", tmp_path / "preds.jsonl", tmp_path / "classes.txt"
    torch.save(export, model)
    classes.write_text("\n".join(f"name{i}" for i in range(10)) + "\n")
    broken = tmp_path / "pics" / "broken.png"
    broken.parent.mkdir()
    broken.write_bytes(open(files[0], "rb").read()[:40])          # a truncated PNG
    (tmp_path / "pics" / "notes.txt").write_text("not an image")
    summary = CP.main(["predict", "--compact", str(model), "--images", files[0], str(tmp_path / "pics"), *files[1:], "--output", str(out),
                       "--classes", str(classes), "--batch_size", str(BS), "--precision", "fp32", "--num_workers", "2", "--topk", "4"])
    lines = [json.loads(l) for l in out.read_text().splitlines()]
    assert len(lines) == 8 + 1 and lines[-1] == summary
    assert summary["images"] == 8 and summary["errors"] == 1 and summary["batches"] == 3 and summary["img_per_s"] > 0
    assert [r["file"] for r in lines[:-1]] == [files[0], str(broken), *files[1:]]
    assert set(lines[1]) == {"file", "error"} and lines[1]["error"]
    good = lines[:1] + lines[2:-1]
    assert all(set(r) == {"file", "top"} and len(r["top"]) == 4 for r in good)
    assert all(e["label"] == f"name{e['index']}" and 0 <= e["index"] < 10 and 0.0 < e["prob"] <= 1.0 for r in good for e in r["top"])
    # the broken file's stand-in shares a batch with files[0] and files[1] and changes nothing of theirs
    cm = CP.CompactVisionTransformer(export, precision="fp32")
    alone = list(CP.predict(cm, files, topk=4, batch_size=7, num_labels=10, num_workers=2))
    assert [[e["index"] for e in r["top"]] for r in good] == [[e["index"] for e in r["top"]] for r in alone]
    capsys.readouterr()
    CP.main(["predict", "--compact", str(model), "--images", files[2], "--precision", "fp32", "--topk", "1"])      # to stdout
    printed = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    assert len(printed) == 2 and printed[0]["file"] == files[2] and printed[1]["images"] == 1
