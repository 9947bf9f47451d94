"""GPU: the transfer workflow's kernels -- uvc_knn_topk on exact integer data (equal to ``reference_knn``) and on real-valued data (the
float32 summation bound), its invariances, NaN / inf, a bank past 2^31 bytes and its refusals; uvc_knn_vote against ``reference_vote``;
uvc_vit_compact_features against ``reference_features``; and ``python -m uvc_amd.compact_transfer`` end to end."""
import copy
import json

import numpy as np
import pytest
import torch

import knn_ref as KR
from uvc_amd import _lib as L
from uvc_amd import compact as CP
from uvc_amd import compact_transfer as CT
from uvc_amd import ops

pytestmark = pytest.mark.gpu

DT = KR.DT
INF = float("inf")
BITS = lambda t: t.view(torch.int32)


def run_guarded(q, b, k, splits=0):
    """knn_topk into the middle of guarded buffers: (sims, idx) on the host after the guards were checked."""
    nq = q.shape[0]
    sims = torch.full((nq + 2, k), 12345.0, device="cuda")
    idx = torch.full((nq + 2, k), -77, dtype=torch.int32, device="cuda")
    s, i = ops.knn_topk(q, b, k, splits, sims=sims[1:nq + 1], idx=idx[1:nq + 1])
    assert s.data_ptr() == sims[1:].data_ptr() and i.data_ptr() == idx[1:].data_ptr()
    assert (sims[0] == 12345.0).all() and (sims[-1] == 12345.0).all() and (idx[0] == -77).all() and (idx[-1] == -77).all()
    return s.cpu(), i.cpu()


def assert_exact(q, b, k, splits=0, what=""):
    want_s, want_i = CT.reference_knn(q, b, k)
    for prec, dt in DT.items():
        got_s, got_i = run_guarded(q.to(dt).cuda(), b.to(dt).cuda(), k, splits)
        assert np.array_equal(got_i.numpy().astype(np.int64), want_i), (what, prec, "idx")
        assert np.array_equal(got_s.double().numpy(), want_s), (what, prec, "sims")


# (D, nq, n, k): every D, nq, n and k of the issue's lists at least once; tile edges of both operands, n < k, one bank row, several splits
EXACT = [(8, 1, 1, 1), (8, 15, 5, 20), (24, 16, 63, 5), (24, 17, 64, 64), (64, 63, 65, 20), (64, 65, 127, 1), (192, 16, 129, 20),
         (192, 1, 1000, 64), (384, 17, 1000, 20), (384, 65, 129, 5), (768, 15, 127, 20), (768, 63, 1000, 64), (1024, 16, 65, 20),
         (1024, 65, 1000, 5)]


@pytest.mark.parametrize("D,nq,n,k", EXACT)
def test_topk_equals_the_reference_on_exact_data(D, nq, n, k):
    q, b = KR.int_operands(nq, n, D, seed=1000 * D + n + nq)
    assert_exact(q, b, k, what="random")


STRUCTURED = [("dup", 8, 65, 129, 20), ("dup", 64, 17, 1000, 64), ("zeroq", 64, 17, 127, 20), ("zeroq", 384, 16, 1000, 20),
              ("ascend", 24, 16, 129, 5), ("ascend", 192, 17, 1000, 20), ("descend", 24, 15, 129, 20), ("descend", 192, 63, 1000, 64),
              ("asym", 24, 17, 127, 5), ("asym", 64, 65, 65, 64)]


@pytest.mark.parametrize("kind,D,nq,n,k", STRUCTURED)
def test_topk_on_structured_exact_banks(kind, D, nq, n, k):
    """duplicated rows (ties by index), an all-zero query (the first k rows), similarities that ascend with the index (every row inserts)
    or descend (none after the first k), and an asymmetric bank (a row / column swap of an operand map changes the answer)."""
    q, b = KR.int_operands(nq, n, D, seed=7 * D + n, kind=kind)
    assert_exact(q, b, k, what=kind)
    assert_exact(q, b, k, splits=1, what=kind + " unsplit")


# ---- real-valued data ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,nq,n,k", [(8, 63, 65, 1), (192, 17, 1000, 20), (384, 65, 129, 5), (768, 16, 1000, 64), (1024, 15, 127, 20)])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_topk_on_real_data_meets_the_float32_bound(D, nq, n, k, prec):
    g = torch.Generator().manual_seed(D + n)
    q, b = torch.randn(nq, D, generator=g).to(DT[prec]), torch.randn(n, D, generator=g).to(DT[prec])
    sims, idx = run_guarded(q.cuda(), b.cuda(), k)
    e_own, e_out = KR.check_real(q, b, sims, idx, k)
    print(f"knn real D {D} nq {nq} n {n} k {k} {prec}: listed |sim - dot| / beta {e_own:.3f}, left-out excess / beta {e_out:.3f}")


# ---- invariances ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_topk_bits_do_not_depend_on_splits_batch_or_run(prec):
    g = torch.Generator().manual_seed(5)
    D, n, k = 192, 1000, 20
    q = torch.randn(65, D, generator=g).to(DT[prec]).cuda()
    b = torch.randn(n, D, generator=g).to(DT[prec]).cuda()
    b[500] = b[3]                                                  # a tie across two splits
    s0, i0 = ops.knn_topk(q, b, k, 1)
    for splits in (2, 7, 0, 64):
        s, i = ops.knn_topk(q, b, k, splits)
        assert torch.equal(BITS(s), BITS(s0)) and torch.equal(i, i0), splits
    assert ops.knn_splits(65, n, k, 7)[1] > 1 and ops.knn_splits(65, n, k, 0)[1] > 1
    s, i = ops.knn_topk(q, b, k, 1)
    assert torch.equal(BITS(s), BITS(s0)) and torch.equal(i, i0)
    for j in (0, 17, 64):                                          # a query alone against itself in the batch of 65
        s, i = ops.knn_topk(q[j:j + 1].clone(), b, k, 0)
        assert torch.equal(BITS(s), BITS(s0[j:j + 1])) and torch.equal(i, i0[j:j + 1]), j
    s, i = ops.knn_topk(q, b[:999], k, 3)                           # and a value does not depend on n: drop a row that no list holds
    if not (i0 == 999).any():
        assert torch.equal(BITS(s), BITS(s0)) and torch.equal(i, i0)


def test_topk_two_level_merge_keeps_the_order():
    """More than 64 splits merge in two levels: 130 one-tile ranges (three groups) of an integer bank full of ties, against the reference
    and against one workgroup per query tile."""
    q, b = KR.int_operands(17, 64 * 129 + 5, 8, seed=21)
    assert ops.knn_splits(17, b.shape[0], 64, 130)[1] == 130 and ops.knn_splits(17, b.shape[0], 64, 512)[1] == 130
    want_s, want_i = CT.reference_knn(q, b, 64)
    for prec, dt in DT.items():
        qd, bd = q.to(dt).cuda(), b.to(dt).cuda()
        s1, i1 = ops.knn_topk(qd, bd, 64, 1)
        assert np.array_equal(i1.cpu().numpy().astype(np.int64), want_i) and np.array_equal(s1.double().cpu().numpy(), want_s)
        for splits in (65, 130, 512):
            s, i = run_guarded(qd, bd, 64, splits)
            assert torch.equal(BITS(s), BITS(s1.cpu())) and torch.equal(i, i1.cpu()), (prec, splits)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_topk_nan_and_infinities(prec):
    q, b = KR.int_operands(17, 129, 24, seed=3)
    q = q.abs() + 1.0                                              # strictly positive queries: inf * q keeps its sign, never inf * 0
    b[5, 2], b[70, 0], b[100, 1], b[128, 3] = float("nan"), -INF, INF, INF
    want_s, want_i = CT.reference_knn(q, b, 20)
    assert (want_i[:, 0] == 100).all() and (want_i[:, 1] == 128).all() and not np.isin(want_i, [5, 70]).any()
    for splits in (0, 1):
        s, i = run_guarded(q.to(DT[prec]).cuda(), b.to(DT[prec]).cuda(), 20, splits)
        assert np.array_equal(i.numpy().astype(np.int64), want_i) and np.array_equal(s.double().numpy(), want_s)


def test_topk_past_two_to_the_31_bytes():
    """bf16, D = 64: rows from 16 777 216 on lie past 2^31 bytes.  Two rows per query there are 4 x the query (entries in +-{1, 2, 3}):
    4 |q|^2 exceeds every other row's 3 sum |q_d|, so each list's head is known without a full reference."""
    D, nq, k = 64, 16, 5
    first = (1 << 31) // (2 * D)
    n = first + 1024
    g = torch.Generator().manual_seed(9)
    q = torch.randint(1, 4, (nq, D), generator=g) * (2 * torch.randint(0, 2, (nq, D), generator=g) - 1)
    bank = torch.randint(-3, 4, (n, D), device="cuda", dtype=torch.int8).to(torch.bfloat16)
    assert bank.numel() * 2 > (1 << 31)
    rows = first + 5 + 37 * torch.arange(nq)
    bank[rows] = (4 * q).to(torch.bfloat16).cuda()
    bank[rows + 1] = (4 * q).to(torch.bfloat16).cuda()
    sims, idx = ops.knn_topk(q.to(torch.bfloat16).cuda(), bank, k)
    assert ops.knn_splits(nq, n, k)[1] > 1
    assert idx[:, 0].cpu().tolist() == rows.tolist() and idx[:, 1].cpu().tolist() == (rows + 1).tolist()
    want = (4 * (q * q).sum(1)).float()
    assert torch.equal(sims[:, 0].cpu(), want) and torch.equal(sims[:, 1].cpu(), want)
    assert (sims[:, 2].cpu() < want).all() and (idx >= 0).all() and (idx < n).all()
    s1, i1 = ops.knn_topk(q.to(torch.bfloat16).cuda(), bank, k, 1)  # one workgroup walks the whole bank: the same lists
    assert torch.equal(s1, sims) and torch.equal(i1, idx)
    rest = bank[idx[:, 2:].long().flatten()].double().cpu().reshape(nq, k - 2, D)      # and the rest of a list is its own pairs' dots, in order
    assert torch.equal(torch.einsum("qd,qjd->qj", q.double(), rest), sims[:, 2:].double().cpu())
    assert (sims[:, 2:-1] >= sims[:, 3:]).all()
    del bank
    torch.cuda.empty_cache()


def test_topk_refusals_leave_the_outputs_alone():
    b32, q32 = torch.zeros(40, 1040, device="cuda"), torch.zeros(3, 1040, device="cuda")
    b16, q16 = b32.bfloat16(), q32.bfloat16()
    sims = torch.full((3, 65), 12345.0, device="cuda")
    idx = torch.full((3, 65), -77, dtype=torch.int32, device="cuda")

    def refused(q, b, k, rc, word):
        with pytest.raises(L.UvcHipError, match=rf"rc={rc}\).*{word}"):
            ops.knn_topk(q, b, k, sims=sims, idx=idx)
        torch.cuda.synchronize()
        assert (sims == 12345.0).all() and (idx == -77).all()

    for q, b in ((q32, b32), (q16, b16)):
        refused(q[:, :64], b[:, :64], 0, 1, "k must lie")
        refused(q[:, :64], b[:, :64], 65, 1, "k must lie")
        refused(q[:, :12], b[:, :12], 5, 3, "multiple of 8")
        refused(q[:, :1032], b[:, :1032], 5, 3, "multiple of 8")
    refused(q32[:, :64], b16[:, :64], 5, 3, "one dtype")
    refused(q16[:, :64], b32[:, :64], 5, 3, "one dtype")
    refused(q16[:, 4:68], b16[:, :64], 5, 1, "16-byte aligned")       # queries 8 bytes off
    refused(q32[:, :64], b32[:, 1:65], 5, 1, "16-byte aligned")       # bank 4 bytes off
    flat = torch.zeros(40 * 68, device="cuda", dtype=torch.bfloat16)
    refused(q16[:, :64], flat.view(40, 68)[:, :64], 5, 1, "16-byte aligned")      # a row stride of 136 bytes
    s, i = ops.knn_topk(q16[:, :64], b16[:, :64], 5, sims=sims[:, :5].contiguous(), idx=idx[:, :5].contiguous())     # the same operands run
    assert (s == 0).all() and i.tolist() == [[0, 1, 2, 3, 4]] * 3


# ---- the vote -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 10, 100, 1000, 1003])
def test_vote_equals_the_reference(C):
    for k, T, ldt in ((20, 0.07, torch.int64), (64, 0.5, torch.int32), (5, 0.0, torch.int64)):
        sims, idx, labels, want, want_pred = KR.vote_case(7, 300, k, C, seed=C + k, T=T)
        scores, pred = ops.knn_vote(sims.cuda(), idx.cuda(), labels.to(ldt).cuda(), C, T)
        got = scores.double().cpu().numpy()
        assert tuple(got.shape) == (7, C) and pred.dtype == torch.int32
        assert (np.abs(got - want) <= 1e-6 * np.abs(want)).all(), float(np.abs(got - want).max())
        assert pred.cpu().tolist() == want_pred.tolist()
        _, pred2 = ops.knn_vote(sims.cuda(), idx.cuda(), labels.to(ldt).cuda(), C, T, scores=False)
        assert torch.equal(pred2, pred)


def test_vote_ties_and_empty_slots_are_exact():
    labels = torch.tensor([2, 1, 1, 2, 0, 7, -1], device="cuda")
    sims = torch.tensor([[0.9, 0.8, 0.7, 0.6, 0.5], [0.9, 0.8, 0.7, -INF, -INF], [-INF] * 5, [0.9, 0.9, 0.5, 0.5, -INF], [0.9, 0.8, 0.7, 0.6, 0.5]], device="cuda")
    idx = torch.tensor([[0, 1, 2, 3, 4], [5, 6, 4, -1, -1], [-1] * 5, [1, 0, 3, 2, -1], [5, 6, 9, -1, 5]], dtype=torch.int32, device="cuda")
    for T in (0.0, -1.0):
        scores, pred = ops.knn_vote(sims, idx, labels, 3, T)
        want, want_pred = CT.reference_vote(sims, idx, labels, 3, T)
        assert np.array_equal(scores.double().cpu().numpy(), want) and pred.cpu().tolist() == want_pred.tolist() == [1, 0, -1, 1, -1]
    scores, pred = ops.knn_vote(sims, idx, labels, 3, 0.07)        # equal leaders with equal weights: the lower class
    assert pred.cpu().tolist() == [2, 0, -1, 1, -1] and scores[3, 1] == scores[3, 2] and float(scores[3, 1]) > 1.0
    for bad, kw in ((1, dict(num_classes=0)), (1, dict(num_classes=65537))):
        with pytest.raises(L.UvcHipError, match=rf"rc={bad}\)"):
            ops.knn_vote(sims, idx, labels, temperature=0.07, **kw)


# ---- features -------------------------------------------------------------------------------------------------------------------------------
MODEL_BARS = {"fp32": 1e-3, "bf16": 2e-2}      # the bars tests/test_compact_gpu.py holds eval logits to
NAMES = ["stage2_micro_skip", "stage2_micro_deit", "stage2_tiny8", "no_heads", "px224"]
_MODELS, _REFS = {}, {}


def model_of(name, prec):
    if (name, prec) not in _MODELS:
        _MODELS[(name, prec)] = CP.CompactVisionTransformer(KR.export_of(name)[0], precision=prec)
    return _MODELS[(name, prec)]


def feature_refs(name):
    """(un-normalised, normalised) float64 references on the float32 master weights, computed once"""
    if name not in _REFS:
        ex, x = KR.export_of(name)
        _REFS[name] = (CT.reference_features(ex, x.double(), normalize=False), CT.reference_features(ex, x.double()))
    return _REFS[name]


def metric(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_features_match_the_reference(name, prec):
    ex, x = KR.export_of(name)
    cm = model_of(name, prec)
    xd = x.cuda()
    want_logits, _ = cm(xd)
    c = ex["cfg"]
    rows = torch.empty(x.shape[0] * (c["img_size"] // c["patch_size"]) ** 2, c["in_chans"] * c["patch_size"] ** 2, dtype=DT[prec], device="cuda")
    ops.patchify(xd, rows, c["patch_size"], ops.UVC_F32 if prec == "fp32" else ops.UVC_BF16)
    for normalize, ref in zip((False, True), feature_refs(name)):
        logits, f = cm.features(xd, normalize=normalize)
        assert torch.equal(logits, want_logits)                                       # the eval forward's bits
        assert f.dtype == torch.float32 and tuple(f.shape) == (x.shape[0], c["embed_dim"])
        logits_p, f_p = cm.features(patches=rows, normalize=normalize)
        assert torch.equal(logits_p, want_logits) and torch.equal(BITS(f_p), BITS(f))  # patch rows handed in: the same bits
        _, f_low = cm.features(xd, normalize=normalize, dtype=torch.bfloat16)
        assert f_low.dtype == torch.bfloat16 and torch.equal(f_low.view(torch.int16), f.to(torch.bfloat16).view(torch.int16))    # rounded once
        _, f_two = cm.features(xd, normalize=normalize)                                # the same bits on a repeat
        assert torch.equal(BITS(f_two), BITS(f))
        e = metric(f, ref)
        bar = MODEL_BARS[prec]
        if prec == "bf16" and e > bar:                                                  # the attribution tests' rule: twice the reference's own bf16 error
            low = CT.reference_features(ex, x.bfloat16(), normalize=normalize)
            bar = max(bar, 2 * metric(low, ref))
        print(f"features {name} {prec} normalize={int(normalize)}: e {e:.2e} (bar {bar:.2e})")
        assert e <= bar, (name, prec, normalize, e, bar)
        if normalize:
            assert torch.allclose(f.double().norm(dim=1).cpu(), torch.ones(x.shape[0], dtype=torch.float64), atol=1e-5)
    again, _ = cm(xd)
    assert torch.equal(again, want_logits)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_features_of_a_zero_readout_row_are_zeros(prec):
    ex = copy.deepcopy(KR.export_of("stage2_micro_deit")[0])
    ex["state_dict"]["norm.weight"].zero_()
    ex["state_dict"]["norm.bias"].zero_()
    x = KR.export_of("stage2_micro_deit")[1].cuda()
    cm = CP.CompactVisionTransformer(ex, precision=prec)
    for normalize in (True, False):
        _, f = cm.features(x, normalize=normalize)
        assert torch.equal(BITS(f) & 0x7fffffff, torch.zeros_like(BITS(f)))           # zeros, not NaN


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_features_of_a_578_token_file(prec):
    ex, x = KR.export_of("px384d")
    cm = CP.CompactVisionTransformer(ex, precision=prec)
    logits, f = cm.features(x.cuda())
    assert torch.equal(logits, cm(x.cuda())[0])
    ref = CT.reference_features(ex, x.double())
    e = metric(f, ref)
    bar = MODEL_BARS[prec]
    if prec == "bf16" and e > bar:
        bar = max(bar, 2 * metric(CT.reference_features(ex, x.bfloat16()), ref))
    print(f"features px384d {prec}: e {e:.2e} (bar {bar:.2e})")
    assert e <= bar


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def test_command(tmp_path, capsys):
    """embed, knn, knn --bank and rehead on three flat-coloured classes through the CIFAR-10 reader; the references run on the very batches
    the loader yields."""
    from uvc_amd import data
    name = "stage2_micro_deit"
    ex, _ = KR.export_of(name)
    train, test = KR.colour_images(30, 1), KR.colour_images(12, 2)
    root = KR.write_cifar10(str(tmp_path / "data"), train, test)
    torch.save(ex, tmp_path / "f.pt")
    common = ["--compact", str(tmp_path / "f.pt"), "--dataset", "cifar10", "--data_dir", root, "--eval_batch_size", "8", "--num_workers", "2",
              "--precision", "fp32"]
    # the reference pipeline, on the loader's own batches: features, neighbours, vote -- and its margin
    import argparse
    ns = argparse.Namespace(dataset="cifar10", data_dir=root, img_size=ex["cfg"]["img_size"], eval_batch_size=8, num_workers=2, interpolation="bilinear",
                            crop_pct=None, packed_dir=None, resident=0)
    feats = {}
    for split in ("train", "test"):
        loader, classes = data.build_eval_loader(ns, split)
        assert classes == 10 and len(loader) == (4 if split == "train" else 2)
        xs, ys = zip(*[(x.cpu(), y.cpu()) for x, y in loader])
        assert torch.equal(torch.cat(ys), torch.from_numpy((train if split == "train" else test)[1]))      # dataset order, the short batch included
        feats[split] = CT.reference_features(ex, torch.cat(xs).double())
    sims, idx = CT.reference_knn(feats["test"], feats["train"], 20)
    scores, pred = CT.reference_vote(sims, idx, torch.from_numpy(train[1]), 10, 0.07)
    assert (scores.max(1) / scores.sum(1) > 0.9).all()
    ref_top1 = 100.0 * float((pred == test[1]).mean())
    assert ref_top1 == 100.0
    capsys.readouterr()
    # knn, embedding the bank itself
    line = CT.main(["knn"] + common)
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert printed == line and set(line) >= {"k", "temperature", "bank_images", "query_images", "top1", "img_per_s", "blocks", "params", "macs_compact"}
    assert (line["k"], line["temperature"], line["bank_images"], line["query_images"], line["top1"]) == (20, 0.07, 30, 12, ref_top1)
    # embed, then knn --bank: the same line
    s = CT.main(["embed", "--split", "train", "--output", str(tmp_path / "bank.pt")] + common)
    assert s["images"] == 30 and s["img_per_s"] > 0 and json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == s
    bank = CT.load_bank(tmp_path / "bank.pt")
    assert bank["data_classes"] == 10 and torch.equal(bank["labels"], torch.from_numpy(train[1]))
    assert bank["meta"] == dict(img_size=64, dataset="cifar10", split="train", interpolation="bilinear", crop_pct=None, precision="fp32", embed_dim=128)
    assert metric(bank["features"], feats["train"]) <= MODEL_BARS["fp32"]
    line_b = CT.main(["knn", "--bank", str(tmp_path / "bank.pt")] + common)
    drop = lambda d: {k: v for k, v in d.items() if k != "img_per_s"}
    assert drop(line_b) == drop(line)
    other = dict(bank, data_classes=100)
    torch.save(other, tmp_path / "bank100.pt")
    with pytest.raises(ValueError, match="data_classes"):
        CT.main(["knn", "--bank", str(tmp_path / "bank100.pt")] + common)
    # rehead --init mean: the file loads and its eval top-1 on the bank's data is the reported class-mean top-1
    capsys.readouterr()
    r = CT.main(["rehead", "--bank", str(tmp_path / "bank.pt"), "--output", str(tmp_path / "g.pt")] + common)
    assert r["num_classes"] == 16 and r["class_mean_top1"] == 100.0
    cm = CP.CompactVisionTransformer(CP.load_compact(tmp_path / "g.pt"), precision="fp32")
    loader, _ = data.build_eval_loader(ns, "train")
    hits = n = 0
    for x, y in loader:
        logits, _ = cm(x)
        hits += int((logits[:, :10].argmax(1) == y).sum())
        n += len(y)
    assert n == 30 and 100.0 * hits / n == r["class_mean_top1"]
