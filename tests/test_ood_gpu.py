"""GPU: uvc_ood_logit_scores, uvc_class_moments, uvc_center_rows, uvc_rows_sqnorm_aug, ops.class_gaussian_fit, ops.gauss_scores and the
compact_ood commands against the float64 specs of uvc_amd/compact_ood.py.

Every test prints the worst figure it measured before it asserts (README "Out-of-distribution detection" records them).
"""
import argparse
import json

import numpy as np
import pytest
import torch

import knn_ref as KR
import ood_ref as OR
from uvc_amd import _lib as L
from uvc_amd import compact as CP
from uvc_amd import compact_ood as OD
from uvc_amd import ops

pytestmark = pytest.mark.gpu

BITS = lambda t: t.view(torch.int32)
REL = 1e-5                                                   # the bar uvc_logits_target and uvc_calib_stats are held to
F32_BAR = 1e-3                                               # the project's float32 bar
GUARD, SENT = 3, 7.25


def guarded(n, count=4):
    """``count`` float32 buffers of n + 2 GUARD elements filled with a sentinel, and their [GUARD, GUARD + n) views"""
    full = [torch.full((n + 2 * GUARD,), SENT, device="cuda") for _ in range(count)]
    return full, [f[GUARD:GUARD + n] for f in full]


def guards_intact(full, n):
    return all(bool((f[:GUARD] == SENT).all()) and bool((f[GUARD + n:] == SENT).all()) for f in full)


# ---- ood_logit_scores -------------------------------------------------------------------------------------------------------------------
def check_logit_scores(z, C, T, what):
    """runs the kernel on z (a device view), asserts bits and bars against float64, returns the worst (msp, energy, entropy) errors"""
    n = z.shape[0]
    full, outs = guarded(n)
    got = ops.ood_logit_scores(z, n_valid=C, temperature=T, outs=outs)
    assert guards_intact(full, n), what
    (msp, mxl, energy, entropy), zmax = OR.logit_refs(z.cpu(), C, T)
    g = [o.cpu() for o in got]
    assert torch.equal(BITS(g[1]), BITS(mxl.float())), what
    worst = []
    for name, gv, ref, scale in (("msp", g[0], msp, msp.abs().clamp_min(1.0)), ("energy", g[2], energy, torch.maximum(energy.abs(), zmax)),
                                 ("entropy", g[3], entropy, entropy.abs().clamp_min(1.0))):
        diff = (gv.double() - ref).abs()
        e = float(torch.where(scale > 0, diff / scale, torch.zeros_like(diff)).max())
        assert bool((diff <= REL * scale).all()), (what, name, e)                     # (a row of zeros: a scale of 0 asks for equality)
        worst.append(e)
    return worst


@pytest.mark.parametrize("C,ld", [(1, 8), (2, 8), (10, 16), (100, 104), (1000, 1000), (1003, 1008), (100, 102), (2500, 2501)])
def test_logit_scores_equal_float64(C, ld):
    worst = [0.0, 0.0, 0.0]
    for rows in (1, 63, 64, 65, 1000):
        for kind in ("normal", "large", "tied"):
            z = OR.logits_case(rows, C, ld, kind, seed=rows + C).cuda()
            for T in (1.0, 0.5, 4.0):
                worst = [max(a, b) for a, b in zip(worst, check_logit_scores(z, C, T, (rows, C, ld, kind, T)))]
    print(f"ood_logit_scores C {C} ld {ld}: msp {worst[0]:.2e} energy {worst[1]:.2e} entropy {worst[2]:.2e} (bar {REL:.0e})")


def test_logit_scores_single_class_and_ties_are_exact():
    z = OR.logits_case(65, 1, 8, "normal", 0).cuda()
    msp, mxl, energy, entropy = ops.ood_logit_scores(z, n_valid=1, temperature=0.5)
    assert torch.equal(msp, torch.ones(65, device="cuda")) and torch.equal(BITS(mxl), BITS(z[:, 0].contiguous()))
    assert torch.equal(BITS(energy), BITS(mxl)) and torch.equal(BITS(entropy), torch.zeros(65, dtype=torch.int32, device="cuda"))
    z = torch.full((4, 8), 2.5, device="cuda")
    msp, mxl, energy, entropy = ops.ood_logit_scores(z, n_valid=8)
    assert torch.equal(msp, torch.full((4,), 0.125, device="cuda")) and torch.equal(mxl, torch.full((4,), 2.5, device="cuda"))
    assert torch.allclose(entropy.double(), torch.full((4,), -np.log(8.0), device="cuda", dtype=torch.float64), rtol=1e-6)


@pytest.mark.parametrize("C,ld", [(10, 16), (100, 104), (1003, 1008), (2500, 2501)])
def test_logit_scores_unaligned_base_and_row_stride(C, ld):
    src = OR.logits_case(65, C, ld, "normal", 5)
    flat = torch.empty(65 * ld + 1, device="cuda")
    off = flat[1:].view(65, ld)                              # one element off 16-byte alignment
    off.copy_(src)
    assert off.data_ptr() % 16 == 4
    want = [o.clone() for o in ops.ood_logit_scores(src.cuda(), n_valid=C, temperature=4.0)]
    check_logit_scores(off, C, 4.0, ("offset", C, ld))
    for pad in (3, 4):                                       # a row stride that is not / is a multiple of 16 bytes
        wide = torch.full((65, ld + pad), float("nan"), device="cuda")
        view = wide[:, :ld]
        view.copy_(src)
        check_logit_scores(view, C, 4.0, ("stride", C, ld, pad))
        got = ops.ood_logit_scores(view, n_valid=C, temperature=4.0)
        for a, b in zip(got, want):                          # the same bits as the aligned, contiguous rows
            assert torch.equal(BITS(a), BITS(b))
        for a, b in zip(ops.ood_logit_scores(off, n_valid=C, temperature=4.0), want):
            assert torch.equal(BITS(a), BITS(b))


@pytest.mark.parametrize("C,ld", [(10, 16), (1000, 1000), (2500, 2504)])
def test_logit_scores_rows_nulls_repeats_and_nan(C, ld):
    z = OR.logits_case(130, C, ld, "normal", 9).cuda()
    ref = ops.ood_logit_scores(z, n_valid=C, temperature=0.5)
    again = ops.ood_logit_scores(z, n_valid=C, temperature=0.5)
    for i in (0, 64, 129):                                   # a row alone gives the bits it has among 130
        alone = ops.ood_logit_scores(z[i:i + 1].clone(), n_valid=C, temperature=0.5)
        for a, b in zip(alone, ref):
            assert torch.equal(BITS(a), BITS(b[i:i + 1]))
    for a, b in zip(again, ref):
        assert torch.equal(BITS(a), BITS(b))
    for keep in ((0,), (1, 3), (2,)):                        # NULL outputs: the others are written, nothing else is touched
        full, outs = guarded(130)
        got = ops.ood_logit_scores(z, n_valid=C, temperature=0.5, outs=[o if j in keep else None for j, o in enumerate(outs)])
        assert guards_intact(full, 130)
        for j in range(4):
            if j in keep:
                assert torch.equal(BITS(got[j]), BITS(ref[j]))
            else:
                assert got[j] is None and bool((full[j] == SENT).all())
    bad = z.clone()
    bad[7, C - 1] = float("nan")
    bad[100, 0] = float("nan")
    got = ops.ood_logit_scores(bad, n_valid=C, temperature=0.5)
    rows = torch.zeros(130, dtype=torch.bool, device="cuda")
    rows[[7, 100]] = True
    for a, b in zip(got, ref):
        assert bool(torch.isnan(a[rows]).all()) and torch.equal(BITS(a[~rows]), BITS(b[~rows]))


def test_logit_scores_refusals_leave_the_outputs_alone():
    z = OR.logits_case(8, 10, 16, "normal", 1).cuda()
    outs = [torch.full((8,), float("nan"), device="cuda") for _ in range(4)]
    calls = [dict(n_valid=0), dict(n_valid=17), dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")),
             dict(temperature=float("inf"))]
    for kw in calls:
        with pytest.raises(L.UvcHipError):
            ops.ood_logit_scores(z, outs=outs, **kw)
    with pytest.raises(L.UvcHipError):
        ops.ood_logit_scores(z, outs=[None] * 4)
    with pytest.raises(L.UvcHipError):
        ops.ood_logit_scores(z.cpu(), outs=outs)
    with pytest.raises(L.UvcHipError):
        ops.ood_logit_scores(z.bfloat16(), outs=outs)
    rc = L.lib().uvc_ood_logit_scores(L.ptr(z), 8, 16, 70000, 1.0, *[L.ptr(o) for o in outs], L.cur_stream())
    assert rc == 3                                           # UVC_ERR_UNSUPPORTED: n_valid above 65536
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs)


# ---- class_moments / class_gaussian_fit -------------------------------------------------------------------------------------------------
moments_ref = OR.moments


@pytest.mark.parametrize("n,D,C", [(1, 8, 1), (64, 8, 16), (1000, 192, 250), (4096, 64, 1024), (4096, 1016, 512)])
def test_fit_is_exact_on_integer_data(n, D, C):
    g = torch.Generator().manual_seed(n + D)
    x = torch.randint(-3, 4, (n, D), generator=g).float()
    y = (torch.arange(n) % C)[torch.randperm(n, generator=g)]            # every class has n / C rows: 1, 4 or 8
    counts, means, scatter = ops.class_gaussian_fit(x.cuda(), y.cuda(), C, chunk_rows=1000)
    rc, rm, rs = moments_ref(x, y, C)
    assert torch.equal(counts.cpu(), rc) and int(rc[0]) == n // C
    assert torch.equal(means.cpu().double(), rm)
    assert torch.equal(scatter.cpu().double(), rs)
    centred = ops.center_rows(x.cuda(), y.cuda(), means)
    assert torch.equal(centred.cpu().double(), x.double() - rm[y])


def spacing(ref):
    r = ref.float()
    return (torch.nextafter(r.abs(), torch.full_like(r, float("inf"))) - r.abs()).double()


@pytest.mark.parametrize("n,D,C,random_labels", [(65, 8, 3, False), (1000, 192, 10, False), (1000, 384, 100, False), (4097, 64, 1000, True),
                                                 (4097, 1016, 7, False)])
def test_fit_on_unit_normal_data(n, D, C, random_labels):
    g = torch.Generator().manual_seed(n + D + C)
    x = torch.randn(n, D, generator=g)
    y = torch.randint(0, C, (n,), generator=g) if random_labels else (torch.arange(n) % C)[torch.randperm(n, generator=g)]
    y[::13] = -1                                             # skipped rows on both sides of the range
    y[5::17] = C
    rc, rm, rs = moments_ref(x, y, C)
    if random_labels:
        assert int((rc == 0).sum()) > 0
    wide = torch.zeros(n, D + 8, device="cuda")
    odd = torch.zeros(n, D + 3, device="cuda")
    wide[:, :D] = x.cuda()
    odd[:, :D] = x.cuda()
    results = {}
    for name, xd, yd, chunk in (("i64", x.cuda(), y.cuda(), None), ("i32", x.cuda(), y.int().cuda(), 64), ("stride", wide[:, :D], y.cuda(), 1000),
                                ("odd stride", odd[:, :D], y.int().cuda(), n), ("i64 again", x.cuda(), y.cuda(), None)):
        counts, means, scatter = ops.class_gaussian_fit(xd, yd, C, chunk_rows=chunk)
        assert torch.equal(counts.cpu(), rc), name
        m = means.cpu()
        assert bool(((m.double() - rm).abs() <= spacing(rm)).all()), name
        empty = rc == 0
        assert torch.equal(BITS(m[empty]), torch.zeros_like(BITS(m[empty])))          # +0
        s = scatter.cpu().double()
        e, asym = float((s - rs).abs().max() / rs.abs().max()), float((s - s.T).abs().max() / rs.abs().max())
        print(f"class_gaussian_fit ({n}, {D}, {C}) {name}: scatter {e:.2e} asymmetry {asym:.2e} (bar {F32_BAR:.0e}) "
              f"means {float(((m.double() - rm).abs() / spacing(rm)).max()):.2f} spacings")
        assert e <= F32_BAR and asym <= F32_BAR, name
        results[name] = (m, scatter.cpu())
    first = results["i64"]
    for name, (m, s) in results.items():                     # the means do not depend on the label type, the stride or the chunk
        assert torch.equal(BITS(m), BITS(first[0])), name
        assert float((s.double() - first[1].double()).abs().max() / rs.abs().max()) <= F32_BAR, name
    assert torch.equal(BITS(results["i64 again"][1]), BITS(first[1]))                  # the same chunk_rows: the same bits


def test_moments_guards_and_refusals():
    g = torch.Generator().manual_seed(4)
    n, D, C = 300, 24, 9
    x, y = torch.randn(n, D, generator=g).cuda(), torch.randint(-1, C - 2, (n,), generator=g).cuda()      # the last two classes are empty
    counts = torch.full((C + 2,), -5, dtype=torch.int64, device="cuda")
    means = torch.full((C + 2, D), SENT, device="cuda")
    got_c, got_m = ops.class_moments(x, y, C, counts=counts[1:C + 1], means=means[1:C + 1])
    rc, rm, _ = moments_ref(x.cpu(), y.cpu(), C)
    assert torch.equal(got_c.cpu(), rc) and rc[-2:].tolist() == [0, 0]
    assert bool(((got_m.cpu().double() - rm).abs() <= spacing(rm)).all())
    assert counts[0] == -5 and counts[-1] == -5 and bool((means[0] == SENT).all()) and bool((means[-1] == SENT).all())
    out = torch.full((n + 2, D), SENT, device="cuda")
    ops.center_rows(x, y, got_m, out=out[1:n + 1])
    assert bool((out[0] == SENT).all()) and bool((out[-1] == SENT).all())
    skipped = (y < 0).cpu()
    assert torch.equal(BITS(out[1:n + 1].cpu()[skipped]), torch.zeros_like(BITS(out[1:n + 1].cpu()[skipped])))
    assert torch.equal(out[1:n + 1].cpu()[~skipped], x.cpu()[~skipped] - got_m.cpu()[y.cpu()[~skipped]])
    # refusals: nothing is launched, NaN-filled outputs stay as they are
    for Dr, Cr, xd in ((12, 4, None), (1024, 4, None), (24, 0, None), (24, 4, "cpu"), (24, 4, "bf16")):
        xr = torch.randn(40, Dr, generator=g)
        xr = xr if xd == "cpu" else xr.cuda().bfloat16() if xd == "bf16" else xr.cuda()
        yr = torch.zeros(40, dtype=torch.int64, device=xr.device)
        cnt = torch.full((max(Cr, 1),), -5, dtype=torch.int64, device="cuda")
        mn = torch.full((max(Cr, 1), Dr), float("nan"), device="cuda")
        with pytest.raises(L.UvcHipError):
            ops.class_moments(xr, yr, Cr, counts=cnt, means=mn)
        with pytest.raises(L.UvcHipError):
            ops.class_gaussian_fit(xr, yr, Cr)
        torch.cuda.synchronize()
        assert bool((cnt == -5).all()) and bool(torch.isnan(mn).all())
        if Cr > 0:
            o = torch.full((40, Dr), float("nan"), device="cuda")
            with pytest.raises(L.UvcHipError):
                ops.center_rows(xr, yr, torch.zeros(Cr, Dr, device="cuda"), out=o)
            assert bool(torch.isnan(o).all())


# ---- gauss_scores ---------------------------------------------------------------------------------------------------------------------------
def dev_detector(det):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in det.items()}


def check_gauss(det, q, what):
    """min_d2, d2_0 and argmin of the device against float64 on the same float32 detector tensors; returns (worst error / largest distance,
    the share of rows below the gap)"""
    d = dev_detector(det)
    d2, arg = ops.gauss_scores(q.cuda(), d["whiten"], d["mean0"], d["wmeans"], d["counts"])
    d0 = ops.gauss_scores(q.cuda(), d["whiten0"], d["mean0"])
    ref, ref0 = OD.reference_gauss(det, q)
    big = max(float(ref.min(dim=1)[0].max()), float(ref0.max()))
    e = max(float((d2.cpu().double() - ref.min(dim=1)[0]).abs().max()), float((d0.cpu().double() - ref0).abs().max())) / big
    assert e <= F32_BAR, (what, e)
    assert d2.dtype == torch.float32 and arg.dtype == torch.int32 and d0.dtype == torch.float32
    clear = OR.top2_gap(ref) > OR.GAP
    out = 1.0 - float(clear.double().mean())
    assert out <= OR.GAP_ROWS, (what, out)
    assert torch.equal(arg.cpu().long()[clear], ref.argmin(dim=1)[clear]), what
    assert bool((det["counts"][arg.cpu().long()] > 0).all()), what
    return e, out


@pytest.mark.parametrize("shape", OR.FIXTURES)
def test_gauss_scores_on_the_fixtures(shape):
    n, C, D, n_ood = shape
    fx = OR.gauss_fixture(1, *shape)
    det = OR.host_detector(fx["x"], fx["y"], C, knn=False)
    e, out = check_gauss(det, torch.cat([fx["xt"], fx["xo"]]), shape)
    print(f"gauss_scores {shape}: worst {e:.2e} of the largest distance (bar {F32_BAR:.0e}), {100 * out:.2f} % of the rows below the gap")


def test_gauss_scores_edges():
    fx = OR.gauss_fixture(1, 600, 10, 64, 200)
    det = OR.host_detector(fx["x"], fx["y"], 10, knn=False)
    d = dev_detector(det)
    q = torch.cat([fx["xt"], fx["xo"]])
    for nq in (1, 15, 16, 17, 63, 65):                       # uvc_knn_topk's tile edges through this path
        check_gauss(det, q[7:7 + nq], ("queries", nq))
    batch = ops.gauss_scores(q[:65].cuda(), d["whiten"], d["mean0"], d["wmeans"], d["counts"])
    batch0 = ops.gauss_scores(q[:65].cuda(), d["whiten0"], d["mean0"])
    for i in (0, 16, 64):                                    # a query alone gives the bits it has in a batch
        alone = ops.gauss_scores(q[i:i + 1].cuda(), d["whiten"], d["mean0"], d["wmeans"], d["counts"])
        assert torch.equal(BITS(alone[0]), BITS(batch[0][i:i + 1])) and torch.equal(alone[1], batch[1][i:i + 1])
        assert torch.equal(BITS(ops.gauss_scores(q[i:i + 1].cuda(), d["whiten0"], d["mean0"])), BITS(batch0[i:i + 1]))
    again = ops.gauss_scores(q[:65].cuda(), d["whiten"], d["mean0"], d["wmeans"], d["counts"])
    assert torch.equal(BITS(again[0]), BITS(batch[0])) and torch.equal(again[1], batch[1])
    one = OR.host_detector(fx["x"], torch.zeros(600, dtype=torch.int64), 1, knn=False)                    # C = 1
    check_gauss(one, q, "one class")
    y = fx["y"].clone()
    y[y == 4] = -1                                           # one class empty
    holed = OR.host_detector(fx["x"], y, 10, knn=False)
    assert holed["counts"][4] == 0
    check_gauss(holed, q, "an empty class")
    _, arg = ops.gauss_scores(q.cuda(), *[holed[k].cuda() for k in ("whiten", "mean0", "wmeans", "counts")])
    assert 4 not in set(arg.cpu().tolist())
    with pytest.raises(L.UvcHipError, match="empty"):
        ops.gauss_scores(q.cuda(), d["whiten"], d["mean0"], d["wmeans"], torch.zeros(10, dtype=torch.int64, device="cuda"))


@pytest.mark.parametrize("n,D,pad", [(1, 8, 0), (65, 64, 0), (130, 1016, 0), (9, 192, 5), (9, 192, 8)])
def test_rows_sqnorm_aug(n, D, pad):
    g = torch.Generator().manual_seed(n + D)
    ld = D + 8 + pad
    src = torch.randn(n + 2, ld, generator=g)
    z = src.clone().cuda()
    sqf, (sq,) = guarded(n, 1)
    ops.rows_sqnorm_aug(z[1:n + 1], D, sq=sq)
    zc = z.cpu()
    assert torch.equal(zc[0], src[0]) and torch.equal(zc[-1], src[-1]) and guards_intact(sqf, n)          # the guard rows
    assert torch.equal(zc[1:n + 1, :D], src[1:n + 1, :D]) and torch.equal(zc[1:n + 1, D + 8:], src[1:n + 1, D + 8:])
    aug = torch.zeros(n, 8)
    aug[:, 0] = 1.0
    assert torch.equal(BITS(zc[1:n + 1, D:D + 8].contiguous()), BITS(aug))
    ref = src[1:n + 1, :D].double().square().sum(dim=1)
    assert float(((sq.cpu().double() - ref).abs() / ref).max()) <= D * 2.0 ** -24
    again = torch.empty_like(sq)
    ops.rows_sqnorm_aug(z[1:n + 1], D, sq=again)
    assert torch.equal(BITS(again), BITS(sq))
    if pad == 0:
        with pytest.raises(L.UvcHipError):                   # no room for the augmentation columns
            ops.rows_sqnorm_aug(z[:, :D + 4], D)
        with pytest.raises(L.UvcHipError):
            L.check(L.lib().uvc_rows_sqnorm_aug(L.ptr(z), D + 7, n, D, L.ptr(sq), L.cur_stream()), "uvc_rows_sqnorm_aug")


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def score_bars(det, banks, refs, D, prec):
    """the bar of every method's score vector: the kernels' own bars above on the scales of these banks"""
    z = torch.cat([b["logits"][:, :det["data_classes"]] for b in banks]).double()
    allref = {m: torch.cat([r[m] for r in refs]) for m in refs[0]}
    d2big = 0.0
    for b in banks:
        d2, d0 = OD.reference_gauss(det, b["features"])
        d2big = max(d2big, float(d2.min(dim=1)[0].max()), float(d0.max()))
    return dict(msp=REL, entropy=REL * max(1.0, float(allref["entropy"].abs().max())), maxlogit=0.0,
                energy=REL * max(float(allref["energy"].abs().max()), float(z.abs().max())),
                mahalanobis=F32_BAR * d2big, rmd=2 * F32_BAR * d2big,            # a difference of two distances, each within the bar
                # a cosine of unit rows: the float32 sum of D products (D 2^-24) and the float32 normalisation; bf16: one operand rounding more
                knn={"fp32": (D + 8) * 2.0 ** -24, "bf16": 2.0 ** -8}[prec])


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_command(tmp_path, capsys, prec):
    """bank x 3, fit and score on three flat-coloured classes (ID) and uniform noise (OOD) through the CIFAR-10 reader."""
    from uvc_amd import data
    ex, _ = KR.export_of("stage2_micro_deit")
    train, test = KR.colour_images(30, 1), KR.colour_images(12, 2)
    rng = np.random.default_rng(5)
    noise = (rng.integers(0, 256, (16, 32, 32, 3), dtype=np.uint8), np.zeros(16, dtype=np.int64))
    root = KR.write_cifar10(str(tmp_path / "id"), train, test)
    root_ood = KR.write_cifar10(str(tmp_path / "ood"), noise, noise)
    torch.save(ex, tmp_path / "f.pt")
    common = ["--compact", str(tmp_path / "f.pt"), "--dataset", "cifar10", "--eval_batch_size", "8", "--num_workers", "2", "--precision", prec]
    capsys.readouterr()
    banks = {}
    for name, d, split, n in (("train", root, "train", 30), ("test", root, "test", 12), ("ood", root_ood, "test", 16)):
        line = OD.main(["bank", "--data_dir", d, "--split", split, "--output", str(tmp_path / f"{name}.pt")] + common)
        assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == line
        assert (line["images"], line["data_classes"], line["embed_dim"], line["normalized"], line["logits"]) == (n, 10, 128, False, True)
        assert line["img_per_s"] > 0 and line["output"] == str(tmp_path / f"{name}.pt")
        banks[name] = OD.load_ood_bank(tmp_path / f"{name}.pt")
        assert banks[name]["num_classes"] == 16 and banks[name]["meta"]["split"] == split and banks[name]["meta"]["precision"] == prec
    assert torch.equal(banks["train"]["labels"], torch.from_numpy(train[1]))
    # the bank holds features(normalize=False)'s bits, batch by batch
    cm = CP.CompactVisionTransformer(ex, precision=prec)
    ns = argparse.Namespace(dataset="cifar10", data_dir=root, img_size=64, eval_batch_size=8, num_workers=2, interpolation="bilinear", crop_pct=None,
                            packed_dir=None, resident=0)
    loader, _ = data.build_eval_loader(ns, "test")
    zs, fs = zip(*[cm.features(x, normalize=False) for x, _ in loader])
    assert torch.equal(BITS(torch.cat(zs).cpu()), BITS(banks["test"]["logits"])) and torch.equal(BITS(torch.cat(fs).cpu()), BITS(banks["test"]["features"]))
    # fit
    line = OD.main(["fit", "--bank", str(tmp_path / "train.pt"), "--output", str(tmp_path / "det.pt"), "--chunk_rows", "16"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == line
    assert {k: line[k] for k in ("rows", "counted_rows", "data_classes", "embed_dim", "empty_classes", "shrinkage", "knn_rows")} == \
        dict(rows=30, counted_rows=30, data_classes=10, embed_dim=128, empty_classes=7, shrinkage=1e-6, knn_rows=30)
    assert set(line) == {"output", "rows", "counted_rows", "data_classes", "embed_dim", "empty_classes", "shrinkage", "knn_rows", "seconds"}
    det = OD.check_detector(torch.load(tmp_path / "det.pt", map_location="cpu"))
    assert det["counts"].tolist() == [10, 10, 10] + [0] * 7 and det["knn_bank"].shape == (30, 128)
    ref_fit = OD.reference_fit(banks["train"]["features"], banks["train"]["labels"], 10, 1e-6)
    assert bool(((det["means"].double() - ref_fit["means"]).abs() <= spacing(ref_fit["means"])).all())
    assert float((det["scatter"].double() - ref_fit["scatter"]).abs().max() / ref_fit["scatter"].abs().max()) <= F32_BAR
    # score
    args = ["score", "--detector", str(tmp_path / "det.pt"), "--id_bank", str(tmp_path / "test.pt"), "--ood_bank", str(tmp_path / "ood.pt"),
            "--k", "5", "--temperature", "2.0", "--precision", prec, "--output", str(tmp_path / "scores.pt")]
    line = OD.main(args)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == line
    assert (line["id_images"], line["ood_images"], line["k"], line["temperature"]) == (12, 16, 5, 2.0) and line["img_per_s"] > 0
    assert tuple(line["methods"]) == OD.METHODS
    scores = torch.load(tmp_path / "scores.pt", map_location="cpu")
    refs = [OD.reference_scores(det, banks[b], OD.METHODS, k=5, temperature=2.0, precision=prec) for b in ("test", "ood")]
    bars = score_bars(det, [banks["test"], banks["ood"]], refs, 128, prec)
    for m in OD.METHODS:
        got_i, got_o = scores[m]["id"], scores[m]["ood"]
        assert got_i.dtype == torch.float32 and got_i.shape == (12,) and got_o.shape == (16,)
        e = max(float((got_i.double() - refs[0][m]).abs().max()), float((got_o.double() - refs[1][m]).abs().max()))
        with capsys.disabled():
            print(f"command {prec} {m}: score error {e:.3e} (bar {bars[m]:.3e}), auroc {line['methods'][m]['auroc']:.4f}")
        assert e <= bars[m], (m, e, bars[m])
        lo, hi = OR.auroc_interval(refs[0][m].numpy(), refs[1][m].numpy(), bars[m])
        assert lo <= line["methods"][m]["auroc"] <= hi, (m, lo, line["methods"][m]["auroc"], hi)
        assert line["methods"][m] == OD.reference_metrics(got_i, got_o)
        assert set(line["methods"][m]) == {"auroc", "aupr", "fpr95", "id_mean", "ood_mean"}
    # a detector fitted without k-NN rows refuses knn by name, and still scores the rest
    line = OD.main(["fit", "--bank", str(tmp_path / "train.pt"), "--output", str(tmp_path / "det0.pt"), "--knn_fraction", "0"])
    assert line["knn_rows"] == 0 and "knn_bank" not in torch.load(tmp_path / "det0.pt", map_location="cpu")
    with pytest.raises(ValueError, match="knn_bank"):
        OD.main(["score", "--detector", str(tmp_path / "det0.pt"), "--id_bank", str(tmp_path / "test.pt"), "--ood_bank", str(tmp_path / "ood.pt")])
    capsys.readouterr()
    line0 = OD.main(["score", "--detector", str(tmp_path / "det0.pt"), "--id_bank", str(tmp_path / "test.pt"), "--ood_bank", str(tmp_path / "ood.pt"),
                     "--methods", "mahalanobis", "msp"])
    assert tuple(line0["methods"]) == ("mahalanobis", "msp") and set(line0["methods"]["msp"]) == {"auroc", "aupr", "fpr95", "id_mean", "ood_mean"}
