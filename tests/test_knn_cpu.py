"""CPU: the written specs of the transfer workflow (uvc_amd/compact_transfer.py) -- features against the network's logits, the k-NN order
and the vote on hand-made cases, re-heading, the bank file, the command line."""
import copy

import numpy as np
import pytest
import torch

import knn_ref as KR
from uvc_amd import compact as CP
from uvc_amd import compact_transfer as CT

NAMES = ["stage2_micro_skip", "stage2_micro_deit", "stage2_tiny8", "no_heads"]
INF = float("inf")


# ---- features ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_reference_features_times_the_head_are_the_logits(name):
    ex, x = KR.export_of(name)
    ex = copy.deepcopy(ex)
    sd = ex["state_dict"]
    if ex["cfg"]["enable_dist"]:                                    # the mean of the rows meets the mean of the heads when they are equal
        sd["head_dist.weight"], sd["head_dist.bias"] = sd["head.weight"].clone(), sd["head.bias"].clone()
    f = CT.reference_features(ex, x.double(), normalize=False)
    assert f.dtype == torch.float64 and tuple(f.shape) == (x.shape[0], ex["cfg"]["embed_dim"])
    want = CP.reference_forward(ex, x.double())
    got = f @ sd["head.weight"].double().T + sd["head.bias"].double()
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    fn = CT.reference_features(ex, x.double())
    assert torch.allclose(fn.norm(dim=1), torch.ones(x.shape[0], dtype=torch.float64), atol=1e-12)
    assert torch.allclose(fn, f / f.norm(dim=1, keepdim=True), atol=1e-14)
    # the walk's old return is what it was
    assert len(CP._reference_walk(ex, x[:1])) == 3


def test_reference_features_of_a_zero_row_are_zeros():
    assert torch.equal(torch.nn.functional.normalize(torch.zeros(2, 8), dim=1, eps=1e-12), torch.zeros(2, 8))


# ---- reference_knn --------------------------------------------------------------------------------------------------------------------
def test_reference_knn_ties_go_to_the_lower_index():
    bank = torch.tensor([[1.0, 0.0], [2.0, 0.0], [1.0, 5.0], [2.0, -1.0], [0.0, 0.0]])
    q = torch.tensor([[1.0, 0.0]])
    sims, idx = CT.reference_knn(q, bank, 4)
    assert idx.tolist() == [[1, 3, 0, 2]] and sims.tolist() == [[2.0, 2.0, 1.0, 1.0]]


def test_reference_knn_short_bank_and_zero_query():
    bank = torch.tensor([[3.0, 1.0], [-2.0, 4.0], [1.0, 1.0]])
    sims, idx = CT.reference_knn(torch.tensor([[0.0, 0.0], [1.0, 1.0]]), bank, 5)
    assert idx.tolist() == [[0, 1, 2, -1, -1], [0, 1, 2, -1, -1]]
    assert sims.tolist() == [[0.0, 0.0, 0.0, -INF, -INF], [4.0, 2.0, 2.0, -INF, -INF]]


def test_reference_knn_leaves_nan_and_minus_inf_out():
    bank = torch.tensor([[1.0], [float("nan")], [-INF], [INF], [0.5]])
    sims, idx = CT.reference_knn(torch.tensor([[1.0]]), bank, 5)
    assert idx.tolist() == [[3, 0, 4, -1, -1]] and sims[0, 0] == INF


# ---- reference_vote -------------------------------------------------------------------------------------------------------------------
def test_reference_vote_majority_and_first_maximum():
    labels = torch.tensor([0, 1, 1, 2, 2, 0])
    sims = torch.tensor([[0.9, 0.8, 0.7, 0.6, 0.5]])
    idx = torch.tensor([[0, 1, 2, 3, 4]], dtype=torch.int32)
    sc, pred = CT.reference_vote(sims, idx, labels, 3, 0.0)        # T <= 0: counts 1, 2, 2 -> the first maximum is class 1
    assert sc.tolist() == [[1.0, 2.0, 2.0]] and pred.tolist() == [1]
    sc, pred = CT.reference_vote(sims, idx, labels, 3, -1.0)
    assert pred.tolist() == [1]
    sc, pred = CT.reference_vote(sims, idx, labels, 3, 0.07)       # weighted: the nearest neighbour's class outweighs two far ones
    T = float(np.float32(0.07))
    d = (sims.double()[0] - sims.double()[0, 0]).numpy()
    want = [1.0, np.exp(d[1] / T) + np.exp(d[2] / T), np.exp(d[3] / T) + np.exp(d[4] / T)]
    assert np.allclose(sc[0], want, rtol=1e-12) and pred.tolist() == [0]


def test_reference_vote_ignores_empty_slots_and_foreign_labels():
    labels = torch.tensor([5, 1, -3, 1])
    sims = torch.tensor([[0.9, 0.8, 0.7, -INF], [-INF, -INF, -INF, -INF]])
    idx = torch.tensor([[0, 2, 3, -1], [-1, -1, -1, -1]], dtype=torch.int32)
    sc, pred = CT.reference_vote(sims, idx, labels, 3, 0.0)
    assert sc.tolist() == [[0.0, 1.0, 0.0], [0.0, 0.0, 0.0]] and pred.tolist() == [1, -1]


def test_vote_cases_have_the_margin():
    for C in (1, 10, 1003):
        sims, idx, labels, sc, pred = KR.vote_case(5, 300, 20, C, seed=C)
        assert (sims[:, :-1] >= sims[:, 1:]).all() and sc.shape == (5, C) and (pred >= 0).all()


# ---- rehead ---------------------------------------------------------------------------------------------------------------------------
def separable_bank(D, classes, per, seed=0):
    """Features around `classes` orthogonal directions, normalised: the class-mean classifier is right on every one."""
    g = torch.Generator().manual_seed(seed)
    y = torch.arange(classes * per) % classes
    centres = torch.eye(D) if classes <= D else torch.nn.functional.normalize(torch.randn(classes, D, generator=g), dim=1)
    f = centres[y] + 0.05 * torch.randn(len(y), D, generator=g)
    return CT.make_bank(torch.nn.functional.normalize(f, dim=1), y, classes, dataset="cifar10", split="train", precision="fp32")


@pytest.mark.parametrize("name", ["stage2_micro_skip", "stage2_micro_deit"])
@pytest.mark.parametrize("classes,width", [(10, 16), (100, 104), (3, 8)])
def test_rehead_writes_a_file_of_the_new_width(name, classes, width):
    ex, x = KR.export_of(name)
    D = ex["cfg"]["embed_dim"]
    before = copy.deepcopy(ex)
    bank = separable_bank(D, classes, 4)
    out, top1 = CT.rehead(ex, bank, init="mean", scale=10.0)
    assert CP.check_export(out) is out and out["cfg"]["num_classes"] == width and top1 == 100.0
    # the input is untouched and everything but the heads and num_classes keeps its bits
    for k, v in before["state_dict"].items():
        assert torch.equal(ex["state_dict"][k], v)
        if not k.startswith("head"):
            assert torch.equal(out["state_dict"][k].view(torch.int32), v.view(torch.int32)) and out["state_dict"][k].dtype == v.dtype
    assert set(out["state_dict"]) == set(before["state_dict"]) and out["blocks"] == before["blocks"]
    assert {k: v for k, v in out["cfg"].items() if k != "num_classes"} == {k: v for k, v in before["cfg"].items() if k != "num_classes"}
    W = out["state_dict"]["head.weight"]
    assert tuple(W.shape) == (width, D) and not out["state_dict"]["head.bias"].any() and not W[classes:].any()
    assert torch.allclose(W[:classes].norm(dim=1), torch.full((classes,), 10.0), rtol=1e-6)
    if ex["cfg"]["enable_dist"]:
        assert torch.equal(out["state_dict"]["head_dist.weight"], W) and not out["state_dict"]["head_dist.bias"].any()
    # the re-headed network's logits are the features times the new weight
    f = CT.reference_features(out, x.double(), normalize=False)
    o, od = CP.reference_logits(out, x.double())
    want = f @ W.double().T
    assert float(((o + od) / 2 - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    # and its features are the source file's
    assert torch.equal(f, CT.reference_features(ex, x.double(), normalize=False))


def test_rehead_zero_and_absent_classes():
    ex, _ = KR.export_of("stage2_micro_skip")
    D = ex["cfg"]["embed_dim"]
    bank = separable_bank(D, 10, 3)
    out, top1 = CT.rehead(ex, bank, init="zero")
    assert top1 is None and not out["state_dict"]["head.weight"].any() and out["cfg"]["num_classes"] == 16
    keep = bank["labels"] != 4                                     # class 4 has no feature: its row is zero
    part = dict(bank, features=bank["features"][keep], labels=bank["labels"][keep])
    out, top1 = CT.rehead(ex, part, init="mean", scale=2.0)
    W = out["state_dict"]["head.weight"]
    assert not W[4].any() and W[3].any() and top1 == 100.0
    with pytest.raises(ValueError):
        CT.rehead(ex, bank, init="ones")


# ---- the bank file and the parser --------------------------------------------------------------------------------------------------------
def test_bank_round_trips_and_a_foreign_embed_dim_is_refused_by_name(tmp_path):
    ex, _ = KR.export_of("stage2_micro_skip")
    D = ex["cfg"]["embed_dim"]
    bank = separable_bank(D, 10, 2)
    path = tmp_path / "bank.pt"
    torch.save(bank, path)
    back = CT.load_bank(path)
    assert torch.equal(back["features"], bank["features"]) and torch.equal(back["labels"], bank["labels"])
    assert back["features"].dtype == torch.float32 and back["labels"].dtype == torch.int64
    assert back["data_classes"] == 10 and back["meta"] == bank["meta"] and set(back["meta"]) == set(CT.META_KEYS)
    assert back["meta"]["embed_dim"] == D
    assert all(isinstance(v, (int, float, str, type(None))) for v in back["meta"].values())
    CT.check_bank(back, ex, 10)
    with pytest.raises(ValueError, match="data_classes"):
        CT.check_bank(back, ex, 100)
    other = separable_bank(D + 64, 10, 2)
    with pytest.raises(ValueError, match="embed_dim"):
        CT.check_bank(other, ex)
    with pytest.raises(ValueError, match="embed_dim"):
        CT.rehead(ex, other)
    torch.save({"weights": 1}, path)
    with pytest.raises(ValueError, match="not a feature bank"):
        CT.load_bank(path)


def test_parser_takes_the_loaders_flags():
    p = CT.build_parser()
    data = ["--dataset", "cifar100", "--data_dir", "D", "--eval_batch_size", "32", "--num_workers", "2", "--precision", "fp32",
            "--interpolation", "bicubic", "--crop_pct", "0.9", "--packed_dir", "P", "--resident", "1"]
    a = p.parse_args(["embed", "--compact", "F", "--split", "test", "--output", "bank.pt"] + data)
    assert (a.cmd, a.split, a.output, a.dataset, a.eval_batch_size, a.num_workers, a.precision) == ("embed", "test", "bank.pt", "cifar100", 32, 2, "fp32")
    assert (a.interpolation, a.crop_pct, a.packed_dir, a.resident) == ("bicubic", 0.9, "P", 1)
    a = p.parse_args(["knn", "--compact", "F"] + data)
    assert (a.k, a.temperature, a.bank) == (20, 0.07, None)
    a = p.parse_args(["knn", "--compact", "F", "--bank", "b.pt", "--k", "64", "--temperature", "0"] + data)
    assert (a.k, a.temperature, a.bank) == (64, 0.0, "b.pt")
    a = p.parse_args(["rehead", "--compact", "F", "--bank", "b.pt", "--output", "G"] + data)
    assert (a.init, a.scale, a.output) == ("mean", 10.0, "G")
    for bad in (["knn", "--compact", "F", "--k", "65"], ["knn", "--compact", "F", "--k", "0"], ["rehead", "--compact", "F", "--output", "G"],
                ["embed", "--compact", "F"], ["rehead", "--compact", "F", "--bank", "b", "--output", "G", "--init", "ones"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_rehead_command_needs_no_device(tmp_path, capsys):
    import json
    ex, _ = KR.export_of("stage2_micro_deit")
    bank = separable_bank(ex["cfg"]["embed_dim"], 10, 2)
    torch.save(ex, tmp_path / "f.pt")
    torch.save(bank, tmp_path / "bank.pt")
    s = CT.main(["rehead", "--compact", str(tmp_path / "f.pt"), "--bank", str(tmp_path / "bank.pt"), "--output", str(tmp_path / "g.pt")])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == s and s["num_classes"] == 16 and s["data_classes"] == 10 and s["class_mean_top1"] == 100.0
    g = CP.load_compact(tmp_path / "g.pt")
    assert g["cfg"]["num_classes"] == 16 and tuple(g["state_dict"]["head_dist.weight"].shape) == (16, ex["cfg"]["embed_dim"])


def test_exact_operands_cover_their_structures():
    """the generators of the GPU cases do what their names say (checked through the reference)"""
    q, b = KR.int_operands(5, 129, 24, 1, "ascend")
    s = q.double() @ b.double().T
    assert (s[:, 1:] > s[:, :-1]).all() and b.abs().max() <= 3
    _, idx = CT.reference_knn(q, b, 5)
    assert idx.tolist() == [[128, 127, 126, 125, 124]] * 5
    q, b = KR.int_operands(5, 129, 24, 1, "descend")
    assert CT.reference_knn(q, b, 5)[1].tolist() == [[0, 1, 2, 3, 4]] * 5
    q, b = KR.int_operands(4, 65, 64, 2, "zeroq")
    assert CT.reference_knn(q, b, 20)[1][0].tolist() == list(range(20))
    q, b = KR.int_operands(4, 66, 8, 3, "dup")
    assert torch.equal(b[0], b[2]) and torch.equal(b[3], b[5]) and not torch.equal(b[2], b[3])
    q, b = KR.int_operands(17, 127, 24, 4, "asym")
    s = q.double() @ b.double().T
    assert not torch.equal(s[:17, :17], s[:17, :17].T)
