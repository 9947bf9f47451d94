"""GPU: uvc_logits_pair_stats, ops.linear_cka and the compact_compare commands against the float64 specs of uvc_amd/compact_compare.py.

Every test prints the worst figure it measured before it asserts (README "Comparing two models" records them).
"""
import argparse
import ctypes
import json

import pytest
import torch

import compare_ref as CR
import knn_ref as KR
from uvc_amd import _lib as L
from uvc_amd import compact_calibrate as CAL
from uvc_amd import compact_compare as CC
from uvc_amd import compact_ood as OD
from uvc_amd import ops

pytestmark = pytest.mark.gpu

REL = 1e-5                                                   # the bar tests/test_ood_gpu.py holds the same row organisation to
F32_BAR = 1e-3                                               # the project's float32 bar
CKA_BAR = 4e-3                                               # three matrices within F32_BAR in a ratio of a square and two norms
REG_MAX = 1024                                               # ops.logits_pair_stats_reg_max(): the register / workgroup switch
GUARD, SENT = 3, 7
FLOATS = tuple(k for k in CC.STATS if k not in CC.INT_STATS)
SHAPES = [(1, 8, 8), (2, 8, 4), (10, 16, 12), (100, 104, 100), (1000, 1000, 1008), (1003, 1008, 1003), (2048, 2048, 2048), (2049, 2052, 2049),
          (2500, 2501, 2504), (REG_MAX, REG_MAX, REG_MAX), (REG_MAX + 1, REG_MAX + 4, REG_MAX + 1)]


def bits(t):
    return t.view(torch.int32)


def guarded(n):
    """{name: a buffer of n + 2 GUARD elements filled with a sentinel} and {name: its [GUARD, GUARD + n) view}"""
    full = {k: torch.full((n + 2 * GUARD,), SENT, dtype=torch.int32 if k in CC.INT_STATS else torch.float32, device="cuda") for k in CC.STATS}
    return full, {k: f[GUARD:GUARD + n] for k, f in full.items()}


def guards_intact(full, n):
    return all(bool((f[:GUARD] == SENT).all()) and bool((f[GUARD + n:] == SENT).all()) for f in full.values())


def check(za, zb, y, C, ref, R, what):
    """runs the kernel on device views, asserts the integers exactly and the floats to their bars; returns {name: worst error / scale}"""
    n = za.shape[0]
    full, outs = guarded(n)
    got = ops.logits_pair_stats(za, zb, y, n_valid=C, outs=outs)
    assert guards_intact(full, n), what
    worst = {}
    for name in CC.STATS:
        g = got[name].cpu()
        if name in CC.INT_STATS:
            assert g.dtype == torch.int32 and torch.equal(g.long(), ref[name]), (what, name)
            continue
        nan = torch.isnan(ref[name])
        assert torch.equal(torch.isnan(g), nan), (what, name)
        err = torch.where(nan, torch.zeros_like(ref[name]), (g.double() - ref[name]).abs()) / CR.scale_of(name, ref[name], R)
        worst[name] = float(err.max())
        assert worst[name] <= REL, (what, name, worst[name])
    return worst


def test_the_switch_is_where_the_tests_think():
    assert ops.logits_pair_stats_reg_max() == REG_MAX


@pytest.mark.parametrize("C,lda,ldb", SHAPES)
def test_pair_stats_equal_float64(C, lda, ldb):
    worst = {k: 0.0 for k in FLOATS}
    for rows in (1, 63, 64, 65, 1000):
        for j, kind in enumerate(CR.FAMILIES):
            za, zb, y, ref, R = CR.case(rows, C, lda, ldb, kind, rows + C)
            yd = (y.int() if (rows + j) % 2 else y).cuda()                                         # int32 and int64 labels, -1 and C among them
            w = check(za.cuda(), zb.cuda(), yd, C, ref, R, (rows, C, lda, ldb, kind))
            worst = {k: max(worst[k], w[k]) for k in FLOATS}
    print(f"logits_pair_stats C {C} lda {lda} ldb {ldb}: " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()) + f" (bar {REL:.0e})")


def restride(z, C, ld):
    out = torch.full((z.shape[0], ld), float("nan"))
    out[:, :C] = z[:, :C]
    return out


@pytest.mark.parametrize("C,lda,ldb", [(10, 16, 12), (1000, 1000, 1008), (2500, 2501, 2504)])
def test_equal_rows_and_no_labels(C, lda, ldb):
    y = CR.labels_for(65, C, 3).cuda()
    for kind in ("same", "tied", "big"):
        za = CR.pair(65, C, lda, ldb, kind, 65 + C)[0]
        za, zb = za.cuda(), restride(za, C, ldb).cuda()
        got = ops.logits_pair_stats(za, zb, y, n_valid=C)
        for name in ("kl_ab", "kl_ba", "tv"):
            assert torch.equal(bits(got[name]), torch.zeros(65, dtype=torch.int32, device="cuda")), (kind, name)      # +0 exactly
        assert float(got["js"].max()) <= 1e-6 and float(got["js"].min()) >= 0.0
        for p, q in (("top1_a", "top1_b"), ("rank_a", "rank_b"), ("rank_b_top1a", "rank_a_top1b")):
            assert torch.equal(got[p], got[q]), (kind, p)
        assert torch.equal(bits(got["conf_a"]), bits(got["conf_b"])) and torch.equal(bits(got["nll_a"]), bits(got["nll_b"]))
        assert bool((got["rank_b_top1a"] == 0).all())
        none = ops.logits_pair_stats(za, zb, None, n_valid=C)                                        # NULL labels: the rest is computed
        assert bool(torch.isnan(none["nll_a"]).all()) and bool(torch.isnan(none["nll_b"]).all())
        assert bool((none["rank_a"] == -1).all()) and bool((none["rank_b"] == -1).all())
        for name in ("top1_a", "top1_b", "conf_a", "conf_b", "kl_ab", "kl_ba", "js", "tv", "rank_b_top1a", "rank_a_top1b"):
            assert torch.equal(bits(none[name]), bits(got[name])), (kind, name)


def test_a_single_class():
    za, zb = CR.pair(65, 1, 8, 5, "normal", 0)
    y = torch.zeros(65, dtype=torch.int64)
    y[3] = 1
    y[4] = -1
    got = {k: v.cpu() for k, v in ops.logits_pair_stats(za.cuda(), zb.cuda(), y.cuda(), n_valid=1).items()}
    counted = (y == 0)
    for name in ("conf_a", "conf_b"):
        assert torch.equal(got[name], torch.ones(65))
    for name in ("kl_ab", "kl_ba", "js", "tv"):
        assert torch.equal(got[name], torch.zeros(65)), name
    for s in "ab":
        assert torch.equal(got["nll_" + s][counted], torch.zeros(63)) and bool(torch.isnan(got["nll_" + s][~counted]).all())
        assert torch.equal(got["rank_" + s].long(), torch.where(counted, 0, -1))
    for name in ("top1_a", "top1_b", "rank_b_top1a", "rank_a_top1b"):
        assert torch.equal(got[name], torch.zeros(65, dtype=torch.int32))


@pytest.mark.parametrize("C,ld", [(10, 16), (100, 104), (1003, 1008), (2500, 2504)])
def test_unaligned_base_and_row_stride(C, ld):
    za, zb, y, ref, R = CR.case(65, C, ld, ld, "normal", 5)
    yd = y.cuda()
    want = {k: v.clone() for k, v in ops.logits_pair_stats(za.cuda(), zb.cuda(), yd, n_valid=C).items()}

    def same_bits(got, what):
        for k in CC.STATS:
            assert torch.equal(bits(got[k]), bits(want[k])), (what, k)
    flat = torch.empty(65 * ld + 1, device="cuda")
    off = flat[1:].view(65, ld)                              # one element off 16-byte alignment
    off.copy_(za)
    assert off.data_ptr() % 16 == 4
    check(off, zb.cuda(), yd, C, ref, R, ("offset a", C))
    same_bits(ops.logits_pair_stats(off, zb.cuda(), yd, n_valid=C), "offset a")
    off.copy_(zb)
    same_bits(ops.logits_pair_stats(za.cuda(), off, yd, n_valid=C), "offset b")
    for pad in (3, 4):                                       # a row stride that is not / is a multiple of 16 bytes
        wide = torch.full((65, ld + pad), float("nan"), device="cuda")
        view = wide[:, :ld]
        view.copy_(zb)
        check(za.cuda(), view, yd, C, ref, R, ("stride b", C, pad))
        same_bits(ops.logits_pair_stats(za.cuda(), view, yd, n_valid=C), ("stride b", pad))
        view.copy_(za)
        same_bits(ops.logits_pair_stats(view, zb.cuda(), yd, n_valid=C), ("stride a", pad))


@pytest.mark.parametrize("C,lda,ldb", [(10, 16, 12), (1000, 1000, 1008), (2500, 2504, 2504)])
def test_rows_nulls_repeats_and_nan(C, lda, ldb):
    za, zb, y, _, _ = CR.case(130, C, lda, ldb, "normal", 9)
    za, zb, y = za.cuda(), zb.cuda(), y.cuda()
    ref = ops.logits_pair_stats(za, zb, y, n_valid=C)
    again = ops.logits_pair_stats(za, zb, y, n_valid=C)
    for k in CC.STATS:
        assert torch.equal(bits(again[k]), bits(ref[k])), k
    for i in (0, 64, 129):                                   # a row alone gives the bits it has among 130
        alone = ops.logits_pair_stats(za[i:i + 1].clone(), zb[i:i + 1].clone(), y[i:i + 1].clone(), n_valid=C)
        for k in CC.STATS:
            assert torch.equal(bits(alone[k]), bits(ref[k][i:i + 1])), (i, k)
    keeps = [(k,) for k in CC.STATS] + [tuple(k for k in CC.STATS if k != drop) for drop in CC.STATS]
    for keep in keeps:                                       # NULL outputs: the others are written, nothing else is touched
        full, outs = guarded(130)
        got = ops.logits_pair_stats(za, zb, y, n_valid=C, outs={k: outs[k] for k in keep})
        assert guards_intact(full, 130)
        for k in CC.STATS:
            if k in keep:
                assert torch.equal(bits(got[k]), bits(ref[k])), (keep, k)
            else:
                assert got[k] is None and bool((full[k] == SENT).all()), (keep, k)
    bad = za.clone()
    bad[7, C - 1] = float("nan")
    bad[100, 0] = float("nan")
    got = ops.logits_pair_stats(bad, zb, y, n_valid=C)
    rows = torch.zeros(130, dtype=torch.bool, device="cuda")
    rows[[7, 100]] = True
    for k in CC.STATS:                                       # a NaN in za poisons its row, all of it, and no other
        assert torch.equal(bits(got[k][~rows]), bits(ref[k][~rows])), k
        assert bool((got[k][rows] == -1).all()) if k in CC.INT_STATS else bool(torch.isnan(got[k][rows]).all()), k


def test_refusals_leave_the_outputs_alone():
    za, zb = (t.cuda() for t in CR.pair(8, 10, 16, 12, "normal", 1))
    y = torch.zeros(8, dtype=torch.int64, device="cuda")
    outs = {k: torch.full((8,), -5 if k in CC.INT_STATS else float("nan"), dtype=torch.int32 if k in CC.INT_STATS else torch.float32, device="cuda")
            for k in CC.STATS}

    def raw(**kw):
        a = L.uvc_pair_stats_args()
        a.za, a.zb, a.labels = L.ptr(za), L.ptr(zb), L.ptr(y)
        for k, o in outs.items():
            setattr(a, k, L.ptr(o))
        a.n, a.lda, a.ldb, a.C, a.labels_i64 = 8, 16, 12, 10, 1
        for k, v in kw.items():
            setattr(a, k, v)
        return L.lib().uvc_logits_pair_stats(ctypes.byref(a), L.cur_stream())
    for kw in (dict(za=None), dict(zb=None), dict(n=0), dict(C=0), dict(C=13), dict(C=17, ldb=32), dict(C=12, lda=11)):
        assert raw(**kw) == 1, kw                            # UVC_ERR_ARG
    assert raw(C=65537, lda=70000, ldb=70000) == 3           # UVC_ERR_UNSUPPORTED
    assert raw(**{k: None for k in CC.STATS}) == 1           # no output
    for call in (lambda: ops.logits_pair_stats(za.cpu(), zb, y, outs=outs), lambda: ops.logits_pair_stats(za, zb.bfloat16(), y, outs=outs),
                 lambda: ops.logits_pair_stats(za, zb, y, n_valid=13, outs=outs), lambda: ops.logits_pair_stats(za.T.contiguous().T, zb, y, outs=outs),
                 lambda: ops.logits_pair_stats(za, zb[:7], y, outs=outs), lambda: ops.logits_pair_stats(za, zb, y.float(), outs=outs),
                 lambda: ops.logits_pair_stats(za, zb, y, n_valid=0, outs=outs)):
        with pytest.raises(L.UvcHipError):
            call()
    torch.cuda.synchronize()
    assert all(bool((o == -5).all()) if k in CC.INT_STATS else bool(torch.isnan(o).all()) for k, o in outs.items())
    assert raw() == 0                                        # and the same arguments, unrefused, write everything
    torch.cuda.synchronize()
    assert not any(bool((o == -5).any()) if k in CC.INT_STATS else bool(torch.isnan(o).any()) for k, o in outs.items())


# ---- linear_cka -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D1,D2", [(64, 8, 8), (1000, 192, 384), (4097, 64, 1016)])
def test_cka_matrices_are_exact_on_integer_features(n, D1, D2):
    g = torch.Generator().manual_seed(n + D1)

    def integers(D):                                         # rows A, -A (and a row of zeros at an odd n) in a seeded order, plus an integer per
        A = torch.randint(-3, 4, (n // 2, D), generator=g).float()                                   # column: the column means are those integers
        rows = torch.cat([A, -A, torch.zeros(n % 2, D)])[torch.randperm(n, generator=g)]
        return rows + torch.randint(-1, 2, (D,), generator=g).float()
    X, Y = integers(D1), integers(D2)
    got = ops.linear_cka_matrices(X.cuda(), Y.cuda(), chunk_rows=1000)
    for gm, rm in zip(got, CC.reference_cka_matrices(X, Y)):
        assert float(rm.abs().max()) < 2 ** 24 and torch.equal(gm.cpu().double(), rm)
    assert abs(ops.linear_cka(X.cuda(), Y.cuda()) - CC.reference_cka(X, Y)) <= 1e-12


@pytest.mark.parametrize("n,D1,D2", [(64, 8, 8), (1000, 192, 384), (4097, 64, 1016)])
def test_cka_on_unit_normal_features(n, D1, D2):
    g = torch.Generator().manual_seed(n + D2)
    X = torch.randn(n, D1, generator=g) + 2.0
    cases = {"independent": torch.randn(n, D2, generator=g) - 1.0}
    if D1 == D2:
        Q = torch.linalg.qr(torch.randn(D1, D1, generator=g))[0]
        cases["rotated"] = 1.5 * (X @ Q) + torch.randn(D1, generator=g)
    for name, Y in cases.items():
        ref_m, ref = CC.reference_cka_matrices(X, Y), CC.reference_cka(X, Y)
        values = {}
        for chunk in (64, 1000, n, 1000):
            ms = ops.linear_cka_matrices(X.cuda(), Y.cuda(), chunk_rows=chunk)
            e = max(float((gm.cpu().double() - rm).abs().max() / rm.abs().max()) for gm, rm in zip(ms, ref_m))
            v = ops.cka_from_matrices(*ms)
            print(f"linear_cka ({n}, {D1}, {D2}) {name} chunk {chunk}: matrices {e:.2e} (bar {F32_BAR:.0e}) cka {v:.6f} error {abs(v - ref):.2e} (bar {CKA_BAR:.0e})")
            assert e <= F32_BAR and abs(v - ref) <= CKA_BAR
            if chunk in values:                              # the same chunk_rows: the same bits
                assert all(torch.equal(bits(p), bits(q)) for p, q in zip(values[chunk], ms))
            values[chunk] = ms
        if name == "rotated":
            assert abs(ref - 1.0) < 1e-5


def test_cka_refusals_and_constant_features():
    X = torch.randn(100, 16, device="cuda")
    for D in (12, 1024):
        with pytest.raises(L.UvcHipError, match="multiple of 8"):
            ops.linear_cka(X, torch.randn(100, D, device="cuda"))
        a, b = CR.hand_banks()
        rec = CC.compare_banks(dict(a, features=torch.randn(12, 16), normalized=False), dict(b, features=torch.randn(12, D), normalized=False), topk=1)[0]
        assert rec["cka"] is None and f"width {D}" in rec["cka_reason"]
    with pytest.raises(L.UvcHipError):
        ops.linear_cka(X, torch.randn(99, 16, device="cuda"))
    assert ops.linear_cka(X, torch.full((100, 8), 3.0, device="cuda")) is None


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def close_to_reference(rec, ref, banks, what):
    """integer fields and both worst lists equal, floats within the kernel bars of the reference record"""
    C = rec["data_classes"]
    spread = lambda z: float((z[:, :C].double().max(dim=1)[0] - z[:, :C].double().min(dim=1)[0]).max())
    R = max(spread(banks[0]["logits"]), spread(banks[1]["logits"]), 1.0)
    assert abs(rec["mcnemar_p"] - ref["mcnemar_p"]) <= 1e-12
    for k in ("images", "counted", "data_classes", "topk", "flips", "agreement", "churn", "negative_flip_rate", "positive_flip_rate",
              "a_top1_in_b_topk", "b_top1_in_a_topk", "matrices"):
        assert rec[k] == ref[k], (what, k, rec[k], ref[k])
    for s in "ab":
        assert rec[s]["top1"] == ref[s]["top1"] and rec[s]["topk"] == ref[s]["topk"]
        assert abs(rec[s]["confidence"] - ref[s]["confidence"]) <= REL and abs(rec[s]["nll"] - ref[s]["nll"]) <= REL * max(R, ref[s]["nll"])
    for k in ("kl_ab", "kl_ba"):
        assert abs(rec[k] - ref[k]) <= REL * max(R, ref[k]), (what, k)
    for k in ("js", "tv", "js_max"):
        assert abs(rec[k] - ref[k]) <= REL, (what, k)
    assert rec["classes_worst"] == ref["classes_worst"], what
    strip = lambda ws: [{k: v for k, v in w.items() if k != "js"} for w in ws]
    assert strip(rec["images_worst"]) == strip(ref["images_worst"]), what
    assert all(abs(p["js"] - q["js"]) <= REL for p, q in zip(rec["images_worst"], ref["images_worst"]))
    print(f"{what}: agreement {rec['agreement']:.3f} js {rec['js']:.3e} (error {abs(rec['js'] - ref['js']):.1e}) kl_ab error "
          f"{abs(rec['kl_ab'] - ref['kl_ab']):.1e} of scale {max(R, ref['kl_ab']):.1f}, cka {rec['cka']} (reference {ref['cka']})")
    if ref["cka"] is None:
        assert rec["cka"] is None
    else:
        assert abs(rec["cka"] - ref["cka"]) <= CKA_BAR


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_command(tmp_path, capsys, prec):
    """run and diff on three flat-coloured classes through the CIFAR-10 reader: two exports, and one against its own rescaled head."""
    ex_a, ex_b = KR.export_of("stage2_micro_deit")[0], KR.export_of("stage2_micro_skip")[0]
    assert ex_a["cfg"]["img_size"] == ex_b["cfg"]["img_size"] == 64 and ex_a["cfg"]["num_classes"] == ex_b["cfg"]["num_classes"] == 16
    ex_c = CAL.calibrated_head(ex_a, 0.5, None, 10)
    test = KR.colour_images(12, 2)
    root = KR.write_cifar10(str(tmp_path / "id"), KR.colour_images(6, 1), test)
    for name, ex in (("a", ex_a), ("b", ex_b), ("c", ex_c)):
        torch.save(ex, tmp_path / f"{name}.pt")
    data = ["--dataset", "cifar10", "--data_dir", root, "--eval_batch_size", "8", "--num_workers", "2", "--precision", prec]      # 12 images: the last batch is short
    flags = ["--topk", "3", "--worst_images", "5", "--worst_classes", "3", "--chunk_rows", "8"]
    capsys.readouterr()
    rec = CC.main(["run", "--a", str(tmp_path / "a.pt"), "--b", str(tmp_path / "b.pt"), "--bank_a", str(tmp_path / "bank_a.pt"),
                   "--bank_b", str(tmp_path / "bank_b.pt"), "--output", str(tmp_path / "out.pt")] + data + flags)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == rec
    assert (rec["images"], rec["counted"], rec["data_classes"], rec["topk"]) == (12, 12, 10, 3) and rec["img_per_s"] > 0
    # the banks are compact_ood bank's, bit for bit
    banks = {}
    for name in ("a", "b"):
        OD.main(["bank", "--compact", str(tmp_path / f"{name}.pt"), "--split", "test", "--output", str(tmp_path / f"ood_{name}.pt")] + data)
        alone, banks[name] = OD.load_ood_bank(tmp_path / f"ood_{name}.pt"), OD.load_ood_bank(tmp_path / f"bank_{name}.pt")
        assert list(alone) == list(banks[name])
        for k, v in alone.items():
            if torch.is_tensor(v):
                assert v.dtype == banks[name][k].dtype and torch.equal(v.view(torch.uint8), banks[name][k].view(torch.uint8)), (name, k)
            else:
                assert v == banks[name][k], (name, k)
    capsys.readouterr()
    # diff on those banks prints the same record
    args = ["diff", "--bank_a", str(tmp_path / "bank_a.pt"), "--bank_b", str(tmp_path / "bank_b.pt"), "--output", str(tmp_path / "out2.pt")] + flags
    rec2 = CC.main(args)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == rec2
    assert {k: v for k, v in rec2.items() if k != "img_per_s"} == {k: v for k, v in rec.items() if k != "img_per_s"}
    out, out2 = torch.load(tmp_path / "out.pt"), torch.load(tmp_path / "out2.pt")
    assert set(out) == set(CC.STATS) | {"per_class"} | set(CC.MATRIX_KEYS) and all(torch.equal(out[k], out2[k]) or k in FLOATS for k in out)
    assert all(torch.equal(bits(out[k]), bits(out2[k])) for k in FLOATS)
    ref = CC.reference_compare(banks["a"], banks["b"], topk=3, worst_images=5, worst_classes=3, chunk_rows=8)
    with capsys.disabled():
        close_to_reference(rec, ref, (banks["a"], banks["b"]), f"command {prec} A against B")
    # A against its own head at half the scale: every prediction stays wherever the top-2 gap is not zero
    rec_c, _, bank_c = CC.run_command(CC.build_parser().parse_args(["run", "--a", str(tmp_path / "a.pt"), "--b", str(tmp_path / "c.pt"),
                                                                    "--output", str(tmp_path / "out_c.pt")] + data + flags))
    out_c = torch.load(tmp_path / "out_c.pt")
    top2 = torch.topk(banks["a"]["logits"][:, :10], 2, dim=1)[0]
    clear = top2[:, 0] > top2[:, 1]
    assert torch.equal(out_c["top1_a"][clear], out_c["top1_b"][clear]) and torch.equal(out_c["top1_a"], out["top1_a"])
    if bool(clear.all()):
        assert rec_c["agreement"] == 1.0 and rec_c["flips"]["a_only"] == rec_c["flips"]["b_only"] == 0
    assert rec_c["a"]["top1"] == rec["a"]["top1"] and torch.equal(bits(bank_c["features"]), bits(banks["a"]["features"]))
    # A against A
    rec_s = CC.main(["diff", "--bank_a", str(tmp_path / "bank_a.pt"), "--bank_b", str(tmp_path / "bank_a.pt")] + flags)
    assert rec_s["churn"] == 0.0 and rec_s["agreement"] == 1.0 and rec_s["mcnemar_p"] == 1.0 and abs(rec_s["cka"] - 1.0) <= CKA_BAR
    assert rec_s["kl_ab"] == 0.0 and rec_s["tv"] == 0.0 and rec_s["flips"]["a_only"] == 0 and rec_s["a"] == rec_s["b"]
    # refusals, by name
    short = dict(banks["b"], logits=banks["b"]["logits"][:11], labels=banks["b"]["labels"][:11], features=banks["b"]["features"][:11])
    torch.save(short, tmp_path / "short.pt")
    with pytest.raises(ValueError, match="differ in rows"):
        CC.main(["diff", "--bank_a", str(tmp_path / "bank_a.pt"), "--bank_b", str(tmp_path / "short.pt")])
    moved = dict(banks["b"], labels=banks["b"]["labels"].roll(1))
    torch.save(moved, tmp_path / "moved.pt")
    with pytest.raises(ValueError, match="not the same split in the same order"):
        CC.main(["diff", "--bank_a", str(tmp_path / "bank_a.pt"), "--bank_b", str(tmp_path / "moved.pt")])
    px = KR.export_of("px384d")[0]
    with pytest.raises(ValueError, match="differ in img_size"):
        CC.run_command(argparse.Namespace(**dict(vars(CC.build_parser().parse_args(["run", "--a", "x", "--b", "y"] + data)), a=ex_a, b=px)))
