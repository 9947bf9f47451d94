"""GPU: the one dataset walk of the compact tools (uvc_amd/compact_tools.py: ``bank_command`` / ``walk``) makes, for every tool, the very
model call that tool made on its own, over the loader's batches in order, the short last batch included: each bank command's saved tensors
are ``torch.equal`` to the concatenation of the tool's per-batch call made here directly, in bf16 and fp32, on 5 images in batches of
2, 2 and 1.  And ``compact_transfer knn`` prints the same line with ``--bank`` as when it embeds the train split itself.  No kernel is
covered here that its own suite does not pin; this holds the walk to "same call, same order"."""
import argparse
import json

import pytest
import torch

import knn_ref as KR
from uvc_amd import compact as CP
from uvc_amd import compact_calibrate as CC
from uvc_amd import compact_ood as OD
from uvc_amd import compact_probe as PB
from uvc_amd import compact_transfer as CT
from uvc_amd import data

pytestmark = pytest.mark.gpu
NAME = "stage2_micro_deit"                           # the 64-pixel micro file of test_knn_gpu.test_command
PRECISIONS = ["bf16", "fp32"]
# tool -> (main, the command, the bank's tensors, the tool's own call on a batch giving those tensors in that order)
TOOLS = {"transfer": (CT.main, "embed", ("features",), lambda m, x: (m.features(x)[1],)),
         "probe": (PB.main, "embed", ("features",), lambda m, x: (m.features(x, normalize=False)[1],)),
         "calibrate": (CC.main, "logits", ("logits",), lambda m, x: (m(x)[0].float(),)),
         "ood": (OD.main, "bank", ("logits", "features"), lambda m, x: m.features(x, normalize=False))}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """(the compact file, the CIFAR-format root, the train pair, the test pair): 5 images in each split."""
    tmp = tmp_path_factory.mktemp("tools")
    ex, _ = KR.export_of(NAME)
    train, test = KR.colour_images(5, 1), KR.colour_images(5, 2)
    root = KR.write_cifar10(str(tmp / "data"), train, test)
    torch.save(ex, tmp / "f.pt")
    return str(tmp / "f.pt"), root, train, test


@pytest.fixture(scope="module")
def direct(files):
    """precision -> {tool: its tensors}: every tool's own call on the train split's batches as the eval loader yields them, concatenated;
    computed once per precision."""
    path, root, train, _ = files
    ex = CP.load_compact(path)
    done = {}

    def of(precision):
        if precision not in done:
            ns = argparse.Namespace(dataset="cifar10", data_dir=root, img_size=ex["cfg"]["img_size"], eval_batch_size=2, num_workers=2,
                                    interpolation="bilinear", crop_pct=None, packed_dir=None, resident=0)
            loader, classes = data.build_eval_loader(ns, "train")
            model = CP.CompactVisionTransformer(ex, precision=precision, device="cuda")
            outs, sizes = {tool: [] for tool in TOOLS}, []
            with torch.no_grad():
                for x, y in loader:
                    sizes.append(int(x.shape[0]))
                    for tool, (_, _, _, call) in TOOLS.items():
                        outs[tool].append(tuple(t.float().cpu() for t in call(model, x)))
            assert classes == 10 and sizes == [2, 2, 1]
            done[precision] = {tool: tuple(torch.cat(t) for t in zip(*o)) for tool, o in outs.items()}
        return done[precision]
    return of


def _common(files, precision):
    path, root, _, _ = files
    return ["--compact", path, "--dataset", "cifar10", "--data_dir", root, "--eval_batch_size", "2", "--num_workers", "2", "--precision", precision]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tool", list(TOOLS))
def test_bank_command_makes_the_tools_own_call_on_every_batch(files, direct, tmp_path, capsys, tool, precision):
    main, cmd, keys, _ = TOOLS[tool]
    out = tmp_path / "bank.pt"
    summary = main([cmd, "--split", "train", "--output", str(out)] + _common(files, precision))
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == summary
    assert (summary["output"], summary["images"], summary["data_classes"]) == (str(out), 5, 10) and summary["img_per_s"] > 0
    bank = torch.load(out, map_location="cpu")
    assert torch.equal(bank["labels"], torch.from_numpy(files[2][1]))                  # dataset order
    want = direct(precision)[tool]
    for key, t in zip(keys, want):
        assert bank[key].dtype == torch.float32 and bank[key].shape == t.shape and torch.equal(bank[key], t), key
    assert bank["meta"]["split"] == "train" and bank["meta"]["precision"] == precision


@pytest.mark.parametrize("precision", PRECISIONS)
def test_knn_prints_the_same_line_with_a_bank_and_without(files, tmp_path, capsys, precision):
    common = _common(files, precision)
    CT.main(["embed", "--split", "train", "--output", str(tmp_path / "bank.pt")] + common)
    capsys.readouterr()
    line = CT.main(["knn"] + common)
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    line_b = CT.main(["knn", "--bank", str(tmp_path / "bank.pt")] + common)
    printed_b = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    drop = lambda d: {k: v for k, v in d.items() if k != "img_per_s"}
    assert printed == line and printed_b == line_b
    assert (line["bank_images"], line["query_images"], line["k"]) == (5, 5, 5)
    assert drop(line_b) == drop(line)
