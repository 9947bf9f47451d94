"""GPU: the kernels of uvc_amd/csrc/influence.hip -- uvc_influence_topk on exact integer data (equal to ``reference_influence``, values
and indices) and on real data (the float32 bound of both chains), its invariances and refusals; uvc_influence_residuals and
uvc_influence_self against float64; and ``python -m uvc_amd.compact_influence`` end to end on a micro model."""
import json
import math

import numpy as np
import pytest
import torch

import influence_ref as IR
from uvc_amd import _lib as L
from uvc_amd import compact_influence as CI
from uvc_amd import ops

pytestmark = pytest.mark.gpu

DT = IR.DT
INF = float("inf")
BITS = lambda t: t.view(torch.int32)
# expf on the device against float64 over the grid of test_expf_error_is_what_the_bars_assume: the worst relative error measured, and the bar
# the residual tests use for it, twice that
EXPF_MEASURED = 8.27e-8                              # 8.2616e-08 on an MI355X, 0.69 of 2^-23
EXPF_BAR = 2 * EXPF_MEASURED


def run_guarded(fq, rq, fb, rb, k, splits=0, pos=True, neg=True, exclude=None, bias=1.0):
    """influence_topk into the middle of guarded buffers: the lists on the host after the guards were checked"""
    nq = fq.shape[0]
    bufs, outs = [], []
    for want, fill in ((pos, 12345.0), (neg, -54321.0)):
        if not want:
            outs.append(False)
            continue
        v = torch.full((nq + 2, k), fill, device="cuda")
        i = torch.full((nq + 2, k), -77, dtype=torch.int32, device="cuda")
        bufs.append((v, i, fill))
        outs.append((v[1:nq + 1], i[1:nq + 1]))
    got = ops.influence_topk(fq, fb, rq, rb, k, bias=bias, exclude=exclude, splits=splits, proponents=outs[0], opponents=outs[1])
    torch.cuda.synchronize()
    for v, i, fill in bufs:
        assert (v[0] == fill).all() and (v[-1] == fill).all() and (i[0] == -77).all() and (i[-1] == -77).all()
    return tuple(None if g is None else (g[0].cpu(), g[1].cpu()) for g in got)


def assert_exact(case, k, splits=0, what="", **kw):
    fq, rq, fb, rb = case
    ex = kw.get("exclude")
    want = CI.reference_influence(fq, rq, fb, rb, k, exclude=ex)
    for prec, dt in DT.items():
        got = run_guarded(fq.to(dt).cuda(), rq.cuda(), fb.to(dt).cuda(), rb.cuda(), k, splits, exclude=None if ex is None else ex.to(torch.int32).cuda(),
                          **{a: b for a, b in kw.items() if a != "exclude"})
        for which, g in enumerate(got):
            if g is None:
                continue
            assert np.array_equal(g[1].numpy().astype(np.int64), want[which][1].numpy()), (what, prec, which, "idx")
            assert np.array_equal(g[0].double().numpy(), want[which][0].numpy()), (what, prec, which, "vals")
    return want


# (D, Cr, nq, n, k, splits): every D, Cr, nq, n, k and split count of the lists at least once; tile edges of both operands, n < k, one bank row
EXACT = [(8, 8, 1, 1, 1, 1), (8, 16, 63, 63, 5, 2), (24, 8, 64, 64, 64, 1), (24, 104, 65, 65, 5, 7), (192, 16, 1, 1000, 64, 0),
         (192, 1000, 65, 1000, 5, 2), (1024, 104, 63, 4097, 5, 7), (1024, 1000, 64, 63, 64, 0), (8, 1000, 65, 4097, 64, 0), (24, 16, 64, 5, 64, 1)]


@pytest.mark.parametrize("D,Cr,nq,n,k,splits", EXACT)
def test_topk_equals_the_reference_on_exact_data(D, Cr, nq, n, k, splits):
    """features in [-3, 3] and residuals in {-1, 0, 1}: |sf + 1| <= 9217 and |sr| <= Cr <= 1000, the product is exact in float32 and bf16 holds
    the inputs; the sparse residuals leave many equal values (zeros above all), so the order rule decides most slots"""
    case = IR.int_case(nq, n, D, Cr, seed=1000 * D + 10 * n + nq + Cr)
    want = assert_exact(case, k, splits, what="both lists")
    if n >= 2:
        v = CI.reference_values(*case)
        assert len(torch.unique(v)) < v.numel() / 2                       # ties are plentiful
    assert_exact(case, k, 1, what="unsplit")
    kk = min(k, n)
    assert (want[0][1][:, :kk] >= 0).all() and (want[0][1][:, kk:] == -1).all() and (want[1][0][:, kk:] == INF).all()


@pytest.mark.parametrize("D,Cr,nq,n,k,splits", [(24, 16, 65, 1000, 5, 0), (192, 104, 63, 65, 64, 2)])
def test_topk_one_list_exclusions_and_padded_strides(D, Cr, nq, n, k, splits):
    case = IR.int_case(nq, n, D, Cr, seed=D + n)
    assert_exact(case, k, splits, what="proponents only", neg=False)
    assert_exact(case, k, splits, what="opponents only", pos=False)
    ex = torch.randint(-1, n, (nq,), generator=torch.Generator().manual_seed(3))
    ex[0], ex[-1] = 0, n - 1
    want = assert_exact(case, k, splits, what="exclude", exclude=ex)
    for which in (0, 1):
        assert not (want[which][1] == ex[:, None]).any()
    # a query that IS a bank row, excluded: the same lists as without that row's candidates
    fq, rq, fb, rb = case
    own = torch.arange(nq) % n
    assert_exact((fb[own], rb[own], fb, rb), k, splits, what="self", exclude=own)
    # row strides above the widths, NaN between the rows
    want = CI.reference_influence(fq, rq, fb, rb, k)
    for prec, dt in DT.items():
        pad = lambda t, extra: IR.padded(t.cuda(), t.shape[1] + extra, float("nan"))
        got = run_guarded(pad(fq.to(dt), 8), pad(rq, 8), pad(fb.to(dt), 16), pad(rb, 24), k, splits)
        for which in (0, 1):
            assert np.array_equal(got[which][1].numpy().astype(np.int64), want[which][1].numpy()) and np.array_equal(got[which][0].double().numpy(), want[which][0].numpy())


def test_topk_two_level_merge_and_nan():
    """130 one-tile ranges (three groups of lists) of an integer bank full of ties; and NaN pairs, which enter neither list"""
    fq, rq, fb, rb = IR.int_case(17, 64 * 129 + 5, 8, 8, seed=21)
    assert ops.influence_splits(17, fb.shape[0], 64, 130)[1] == 130 and ops.influence_splits(17, fb.shape[0], 64, 512)[1] == 130
    assert_exact((fq, rq, fb, rb), 64, 130, what="two levels")
    fq, rq, fb, rb = IR.int_case(17, 129, 24, 16, seed=4)
    fb[5, 2], rb[70, 0] = float("nan"), float("nan")
    want = assert_exact((fq, rq, fb, rb), 20, 0, what="nan")
    assert not np.isin(want[0][1].numpy(), [5, 70]).any() and not np.isin(want[1][1].numpy(), [5, 70]).any()


# ---- real-valued data -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,C,nq,n,k", [(8, 10, 63, 65, 1), (192, 100, 17, 1000, 20), (384, 1000, 65, 1000, 5), (1024, 1000, 16, 129, 64)])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_topk_on_real_data_meets_the_float32_bound(D, C, nq, n, k, prec):
    """Unit-normal features, real softmax residuals.  Every listed value within ``influence_ref.value_bound`` of its own pair's float64 value,
    the j-th value within the row's largest bound of the reference's j-th value; values, not indices.  bf16 features are rounded once and
    the rule is applied to the rounded operands -- tests/test_knn_gpu.py's rounding model, the same bound."""
    fq, rq, fb, rb = IR.real_case(nq, n, D, C, seed=D + n)
    fq, fb = fq.to(DT[prec]), fb.to(DT[prec])
    ex = torch.arange(nq, dtype=torch.int32) % n if k == 5 else None
    got = run_guarded(fq.cuda(), rq.cuda(), fb.cuda(), rb.cuda(), k, exclude=None if ex is None else ex.cuda())
    e_own, e_rank = IR.check_lists(fq, rq, fb, rb, got, k, exclude=ex)
    print(f"influence real D {D} C {C} nq {nq} n {n} k {k} {prec}: listed |v - exact| / bound {e_own:.3f}, j-th value against the reference's / bound {e_rank:.3f}")


# ---- invariances ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_topk_bits_do_not_depend_on_splits_batch_or_run(prec):
    fq, rq, fb, rb = IR.real_case(65, 1000, 192, 100, seed=5)
    fb[500], rb[500] = fb[3], rb[3]                                   # a tie across two splits
    fq, fb = fq.to(DT[prec]).cuda(), fb.to(DT[prec]).cuda()
    rq, rb = rq.cuda(), rb.cuda()
    k = 20
    (p0, pi0), (n0, ni0) = ops.influence_topk(fq, fb, rq, rb, k, splits=1)
    same = lambda got: all(torch.equal(BITS(a), BITS(b)) for a, b in zip((got[0][0], got[0][1], got[1][0], got[1][1]), (p0, pi0, n0, ni0)))
    for splits in (2, 7, 0, 64, 1):
        assert same(ops.influence_topk(fq, fb, rq, rb, k, splits=splits)), splits
    assert ops.influence_splits(65, 1000, k, 7)[1] > 1 and ops.influence_splits(65, 1000, k, 0)[1] > 1
    # any partition of the queries into calls
    for cuts in ((0, 1, 65), (0, 17, 64, 65), (0, 40, 65)):
        parts = [ops.influence_topk(fq[a:b].clone(), fb, rq[a:b].clone(), rb, k, splits=0) for a, b in zip(cuts[:-1], cuts[1:])]
        cat = lambda w, j: torch.cat([p[w][j] for p in parts])
        assert same(((cat(0, 0), cat(0, 1)), (cat(1, 0), cat(1, 1)))), cuts
    # and a value does not depend on n: drop a last row that no list holds
    if not ((pi0 == 999) | (ni0 == 999)).any():
        assert same(ops.influence_topk(fq, fb[:999], rq, rb[:999], k, splits=3))
    # one list alone: the same bits as with the other
    got = ops.influence_topk(fq, fb, rq, rb, k, opponents=False)
    assert got[1] is None and torch.equal(BITS(got[0][0]), BITS(p0)) and torch.equal(got[0][1], pi0)


def test_topk_refusals_leave_the_outputs_alone():
    f32 = torch.zeros(40, 1040, device="cuda")
    f16 = f32.bfloat16()
    r = torch.zeros(40, 4112, device="cuda")
    pv, nv = torch.full((3, 65), 12345.0, device="cuda"), torch.full((3, 65), -5.0, device="cuda")
    pi, ni = torch.full((3, 65), -77, dtype=torch.int32, device="cuda"), torch.full((3, 65), -78, dtype=torch.int32, device="cuda")

    def refused(fq, fb, rq, rb, k, rc, word, **kw):
        kw.setdefault("proponents", (pv, pi))
        kw.setdefault("opponents", (nv, ni))
        with pytest.raises(L.UvcHipError, match=rf"rc={rc}\).*{word}"):
            ops.influence_topk(fq, fb, rq, rb, k, **kw)
        torch.cuda.synchronize()
        assert (pv == 12345.0).all() and (pi == -77).all() and (nv == -5.0).all() and (ni == -78).all()

    for f in (f32, f16):
        q, b = f[:3, :64], f[:, :64]
        refused(q, b, r[:3, :16], r[:, :16], 0, 1, "k must lie")
        refused(q, b, r[:3, :16], r[:, :16], 65, 1, "k must lie")
        refused(f[:3, :12], f[:, :12], r[:3, :16], r[:, :16], 5, 3, "D must be a multiple of 8")
        refused(f[:3, :1032], f[:, :1032], r[:3, :16], r[:, :16], 5, 3, "D must be a multiple of 8")
        refused(q, b, r[:3, :12], r[:, :12], 5, 3, "Cr must be a multiple of 8")
        refused(q, b, r[:3, :4104], r[:, :4104], 5, 3, "Cr must be a multiple of 8")
        refused(q, b, r[:3, :16], r[:, :16], 5, 1, "bias must be finite", bias=INF)
        refused(q, b, r[:3, :16], r[:, :16], 5, 1, "bias must be finite", bias=float("nan"))
        refused(q, b, r[:3, :16], r[:, :16], 5, 1, "at least one list", proponents=False, opponents=False)
        refused(q, b, r[:3, 2:18], r[:, :16], 5, 1, "16-byte aligned")
        refused(q, b, r[:3, :16], r[:, 1:17], 5, 1, "16-byte aligned")
    refused(f32[:3, :64], f16[:, :64], r[:3, :16], r[:, :16], 5, 3, "one dtype")
    refused(f16[:3, :64], f32[:, :64], r[:3, :16], r[:, :16], 5, 3, "one dtype")
    refused(f16[:3, 4:68], f16[:, :64], r[:3, :16], r[:, :16], 5, 1, "16-byte aligned")
    refused(f32[:3, :64], f32[:, 1:65], r[:3, :16], r[:, :16], 5, 1, "16-byte aligned")
    (s, i), (t, j) = ops.influence_topk(f16[:3, :64], f16[:, :64], r[:3, :16], r[:, :16], 5)      # the same operands run: every value is (0 + 1) * 0
    assert (s == 0).all() and (t == 0).all() and i.tolist() == [[0, 1, 2, 3, 4]] * 3 == j.tolist()


# ---- residuals ------------------------------------------------------------------------------------------------------------------------------
def expf_grid():
    """the arguments the residual tests hand to expf: d = z - max of logits of scale up to 30, so 0 down to about -250; 2^20 points on
    [-104, 0] (the float32 range of exp) and the same number of unit-normal draws times 3 and 30, negated in absolute value"""
    g = torch.Generator().manual_seed(0)
    return torch.cat([-torch.linspace(0, 104, 1 << 20), -(3 * torch.randn(1 << 20, generator=g)).abs(), -(30 * torch.randn(1 << 20, generator=g)).abs()])


def test_expf_error_is_what_the_bars_assume():
    """The device expf has no documented bound here, so it is measured: the relative error against float64 exp of the same float32
    argument over ``expf_grid`` wherever the result is a normal number (below, the absolute error is held to one denormal step).
    Measured: 8.2616e-08 (EXPF_MEASURED = 8.27e-8); the residual bars take EXPF_BAR = 1.654e-7, twice that."""
    d = expf_grid()
    e = ops.influence_expf(d.cuda()).cpu().double()
    want = torch.exp(d.double())
    normal = want >= 2.0 ** -126
    rel = float(((e - want).abs() / want)[normal].max())
    print(f"expf: worst relative error {rel:.4e} over {int(normal.sum())} arguments (bar {EXPF_BAR:.4e})")
    assert rel <= EXPF_BAR
    assert ((e - want).abs()[~normal] <= 2.0 ** -149).all()
    assert float(ops.influence_expf(torch.zeros(1, device="cuda"))[0]) == 1.0


def residual_case(n, C, seed, scale):
    g = torch.Generator().manual_seed(seed)
    ld = C + 3
    z = torch.full((n, ld), float("nan"))                                # poison behind the valid columns
    z[:, :C] = scale * torch.randn(n, C, generator=g)
    y = torch.randint(0, C, (n,), generator=g)
    if n >= 5:
        y[1], y[3] = -1, C                                               # two rows without a class
        z[4, :C][torch.rand(C, generator=g) < 0.3] = -INF                # -inf logits: p = 0
        z[4, 0] = 1.0
    return z, y


@pytest.mark.parametrize("C,n", [(1, 65), (2, 1000), (10, 1), (10, 1000), (1000, 65), (2049, 65), (65536, 1), (65536, 5)])
def test_residuals_against_float64(C, n):
    """target exact, the padding columns exactly +0, skipped rows all +0, r and rsq within ``influence_ref.residual_bars`` -- derived from the
    spec with the measured expf error (8.27e-8 measured, bar 1.654e-7 = twice that)."""
    for seed, scale, ldt in ((C + n, 3.0, torch.int64), (C + n + 1, 30.0, torch.int32)):
        z, y = residual_case(n, C, seed, scale)
        zd = z.cuda()[:, :C]
        for target in ("label", "pred"):
            ldr = (C + 7) // 8 * 8 + 8
            rbuf = torch.full((n + 2, ldr), 777.0, device="cuda")
            r, t, rsq = ops.influence_residuals(zd, y.to(ldt).cuda(), C, target, r=rbuf[1:n + 1])
            torch.cuda.synchronize()
            assert (rbuf[0] == 777.0).all() and (rbuf[-1] == 777.0).all()
            want_r, want_t, want_rsq, bar, bar_sq = IR.residual_bars(z, y, C, target, EXPF_BAR)
            assert t.dtype == torch.int32 and t.cpu().tolist() == want_t.tolist()
            r, rsq = r.cpu(), rsq.cpu()
            assert torch.equal(BITS(r[:, C:]), torch.zeros_like(BITS(r[:, C:])))           # +0, not -0
            skipped = want_t < 0
            assert torch.equal(BITS(r[skipped]), torch.zeros_like(BITS(r[skipped]))) and (rsq[skipped] == 0).all()
            err = (r[:, :C].double() - want_r).abs()
            assert (err <= bar).all(), (C, n, target, float((err / bar.clamp_min(1e-300)).max()))
            print(f"residuals C {C} n {n} scale {scale} {target}: worst |r - spec| / bar {float((err / bar.clamp_min(1e-300)).max()):.3f}")
            assert ((rsq.double() - want_rsq).abs() <= bar_sq + 2.0 ** -149).all()           # (one denormal step: a sum below the float32 range)
            stored = (r.double() ** 2).sum(1)
            assert ((rsq.double() - stored).abs() <= 2 * IR.U * stored + 2.0 ** -149).all()  # the squares of the values as stored
            r2, t2, rsq2 = ops.influence_residuals(zd, y.to(ldt).cuda(), C, target)         # the same bits on a repeat, into a fresh tensor
            assert torch.equal(BITS(r2.cpu()[:, :C]), BITS(r[:, :C])) and torch.equal(BITS(rsq2.cpu()), BITS(rsq)) and r2.shape[1] == (C + 7) // 8 * 8
    if n >= 5 and C > 1:
        assert (r[4, :C][z[4, :C] == -INF] == 0).all()


def test_residuals_nan_row_and_refusals():
    C, n = 1000, 65
    z, y = residual_case(n, C, 7, 3.0)
    clean = ops.influence_residuals(z.cuda()[:, :C], y.cuda(), C, "label")
    z[7, 500] = float("nan")
    for target in ("label", "pred"):
        r, t, rsq = ops.influence_residuals(z.cuda()[:, :C], y.cuda(), C, target)
        torch.cuda.synchronize()                                           # it finishes
        if target == "label":
            keep = torch.arange(n) != 7
            assert torch.equal(BITS(r.cpu()[keep]), BITS(clean[0].cpu()[keep])) and torch.equal(BITS(rsq.cpu()[keep]), BITS(clean[2].cpu()[keep]))
            assert torch.equal(t, clean[1])
        assert torch.isnan(r[7, :C]).all() and math.isnan(float(rsq[7])) and (r[7, C:] == 0).all()
    zd = torch.zeros(4, 24, device="cuda")
    yd = torch.zeros(4, dtype=torch.int64, device="cuda")
    rb = torch.full((4, 24), 5.0, device="cuda")
    for kw, rc in ((dict(num_classes=0), 1), (dict(num_classes=20, r=rb[:, :20].contiguous()), 1), (dict(labels=None), 1)):
        args = dict(labels=yd, num_classes=16, target="label", r=rb)
        args.update(kw)
        with pytest.raises(L.UvcHipError, match=rf"rc={rc}\)"):
            ops.influence_residuals(zd, **args)
        torch.cuda.synchronize()
        assert (rb == 5.0).all()
    wide = torch.zeros(1, 65544, device="cuda")
    with pytest.raises(L.UvcHipError, match=r"rc=3\).*65536"):
        ops.influence_residuals(wide, torch.zeros(1, dtype=torch.int64, device="cuda"), 65537)
    r, t, _ = ops.influence_residuals(zd, None, 16, "pred", r=rb)          # NULL labels go with the argmax target
    assert t.tolist() == [0] * 4 and float(r[0, 0]) == 1 / 16 - 1 and (r[:, 16:] == 0).all()


@pytest.mark.parametrize("D,n", [(8, 1), (24, 65), (192, 1000), (1024, 65)])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_self_influence_against_float64(D, n, prec):
    """fsq is a float32 fmaf chain of D / 4 .. terms per lane and a tree: within D u sum f^2 of the float64 sum; the value is one add and one
    multiply more.  Integer features: exact."""
    g = torch.Generator().manual_seed(D + n)
    f = torch.randn(n, D, generator=g).to(DT[prec])
    rsq = torch.rand(n, generator=g)
    out, fsq = ops.self_influence(IR.padded(f.cuda(), D + 8, float("nan")), rsq.cuda(), want_fsq=True)
    want_f = (f.double() ** 2).sum(1)
    assert ((fsq.cpu().double() - want_f).abs() <= D * IR.U * want_f).all()
    want = (want_f + 1.0) * rsq.double()
    assert ((out.cpu().double() - want).abs() <= 1.001 * (D + 2) * IR.U * want).all()
    assert torch.equal(out, (fsq + 1.0) * rsq.cuda())                      # one float32 add, one multiply
    fi = torch.randint(-3, 4, (n, D), generator=g).float().to(DT[prec])
    out, fsq = ops.self_influence(fi.cuda(), torch.ones(n, device="cuda"), bias=0.0, want_fsq=True)
    assert torch.equal(fsq.cpu().double(), (fi.double() ** 2).sum(1)) and torch.equal(out, fsq)
    again = ops.self_influence(fi.cuda(), torch.ones(n, device="cuda"), bias=0.0)
    assert torch.equal(BITS(again), BITS(out))
    with pytest.raises(L.UvcHipError, match=r"rc=3\).*multiple of 8"):
        ops.self_influence(torch.zeros(2, 12, device="cuda"), torch.ones(2, device="cuda"))


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------
def e2e_bound(fq, zq, yq, fb, zb, yb, C, target):
    """[nq, n] float64: what a device value may differ from the float64 reference of the same banks by: ``value_bound`` on the reference's
    residuals plus what the residuals' own bars (``residual_bars``) move the product by, A (bar_q . |r_b| + |r_q| . bar_b + bar_q . bar_b)."""
    rq, _, _, bq, _ = IR.residual_bars(zq, yq, C, target, EXPF_BAR)
    rb, _, _, bb, _ = IR.residual_bars(zb, yb, C, "label", EXPF_BAR)
    A = fq.double().abs() @ fb.double().abs().T + 1.0
    move = bq @ rb.abs().T + rq.abs() @ bb.T + bq @ bb.T
    pad = lambda r: torch.nn.functional.pad(r.float(), (0, (C + 7) // 8 * 8 - C))      # the chain runs over the padded width
    return IR.value_bound(fq, pad(rq), fb, pad(rb)) + 1.001 * A * move


def test_commands_end_to_end(tmp_path, capsys):
    """A micro compact model (embed_dim 64, depth 2, 16 classes, 32-pixel images), banks through ``compact_ood bank``; ``explain`` on banks
    and on written PNG files and ``self`` against the float64 reference run on the same banks, values within ``e2e_bound``."""
    import argparse
    from PIL import Image
    import knn_ref as KR
    from oracle import vit as OV
    from test_compact_cpu import dense_state
    from uvc_amd import compact as CP
    from uvc_amd import compact_ood as OD
    from uvc_amd import data
    ex = CP.export_compact(dense_state(OV.VitConfig(img_size=32, patch_size=8, num_classes=16, embed_dim=64, depth=2, num_heads=1, enable_dist=1)))
    train, test = KR.colour_images(90, 1), KR.colour_images(12, 2)
    root = KR.write_cifar10(str(tmp_path / "data"), train, test)
    torch.save(ex, tmp_path / "f.pt")
    common = ["--compact", str(tmp_path / "f.pt"), "--dataset", "cifar10", "--data_dir", root, "--eval_batch_size", "32", "--num_workers", "2",
              "--precision", "fp32"]
    for split in ("train", "test"):
        OD.main(["bank", "--split", split, "--output", str(tmp_path / f"{split}.pt")] + common)
    T, Q = OD.load_ood_bank(tmp_path / "train.pt"), OD.load_ood_bank(tmp_path / "test.pt")
    assert T["features"].shape == (90, 64) and Q["logits"].shape == (12, 16) and T["data_classes"] == 10
    C, D, k = 10, 64, 5
    capsys.readouterr()

    def close(res, fq, zq, yq, target, prec):
        low = (lambda t: t.bfloat16().float()) if prec == "bf16" else (lambda t: t)
        ref = CI.reference_lists(fq, zq, yq, T["features"], T["logits"], T["labels"], C, k, target, precision=prec)
        bound = e2e_bound(low(fq), zq, yq, low(T["features"]), T["logits"], T["labels"], C, target).max(dim=1, keepdim=True)[0]
        assert res["target"].tolist() == ref["target"].tolist()
        for name in ("pos_vals", "neg_vals"):
            err = (res[name].double() - ref[name]).abs()
            assert (err <= bound).all(), (name, prec, float((err / bound).max()))

    # explain on banks: the file, and the function
    for prec in ("fp32", "bf16"):
        for target in ("pred", "label"):
            line = CI.main(["explain", "--train_bank", str(tmp_path / "train.pt"), "--query_bank", str(tmp_path / "test.pt"), "--k", str(k), "--target", target,
                            "--precision", prec, "--output", str(tmp_path / "infl.jsonl")])
            assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == line and line["queries"] == 12 and line["rows_per_s"] > 0
            recs = [json.loads(s) for s in (tmp_path / "infl.jsonl").read_text().splitlines()]
            assert len(recs) == 12 and all(set(r) == {"row"} | set(CI.RECORD_KEYS) for r in recs)
            res = CI.influence(T, Q, k=k, target=target, precision=prec)
            for j, r in enumerate(recs):
                assert [e["row"] for e in r["proponents"]] == res["pos_idx"][j].tolist() and [e["value"] for e in r["opponents"]] == res["neg_vals"][j].tolist()
            close(res, Q["features"], Q["logits"], Q["labels"] if target == "label" else None, target, prec)
    # explain on files: the test split's first images written as PNG, read back through the cifar preset
    files = []
    for i in range(5):
        files.append(str(tmp_path / f"img{i}.png"))
        Image.fromarray(test[0][i]).save(files[-1])
    (tmp_path / "broken.png").write_bytes(b"not an image")
    line = CI.main(["explain", "--train_bank", str(tmp_path / "train.pt"), "--compact", str(tmp_path / "f.pt"), "--images"] + files + [str(tmp_path / "broken.png")]
                   + ["--k", str(k), "--preset", "cifar", "--precision", "fp32", "--batch_size", "4", "--num_workers", "2", "--output", str(tmp_path / "files.jsonl")])
    assert (line["queries"], line["errors"]) == (5, 1) and line["img_per_s"] > 0
    recs = [json.loads(s) for s in (tmp_path / "files.jsonl").read_text().splitlines()]
    assert [r["file"] for r in recs[:5]] == files and set(recs[0]) == {"file"} | set(CI.RECORD_KEYS) and "error" in recs[5]
    assert all(r["label"] is None and r["target"] == r["pred"] for r in recs[:5])
    # a PNG holds the pickle's pixels, so the files' features are the test bank's first rows (the same eval transform): the reference on those
    res = dict(target=torch.tensor([r["target"] for r in recs[:5]]),
               pos_vals=torch.tensor([[e["value"] for e in r["proponents"]] for r in recs[:5]]),
               neg_vals=torch.tensor([[e["value"] for e in r["opponents"]] for r in recs[:5]]))
    cm = CP.CompactVisionTransformer(ex, precision="fp32")
    ds = data.FileListDataset(files, tolerant=True)
    loader = data.DeviceLoader(ds, 4, 32, train=False, num_workers=2, device=torch.device("cuda", torch.cuda.current_device()), interpolation="bilinear",
                               crop_pct=None, mean=data.CIFAR_MEAN, std=data.CIFAR_STD, eval="square")
    zs, fs = zip(*[cm.features(x, normalize=False) for x, _ in loader])
    close(res, torch.cat(fs).float().cpu(), torch.cat(zs).float().cpu(), None, "pred", "fp32")
    capsys.readouterr()
    line = CI.main(["explain", "--train_bank", str(tmp_path / "train.pt"), "--compact", str(tmp_path / "f.pt"), "--images"] + files[:2]
                   + ["--target_class", "2", "--preset", "cifar", "--precision", "fp32"])
    printed = [json.loads(s) for s in capsys.readouterr().out.strip().splitlines()]
    assert line["target"] == 2 and [r["target"] for r in printed[:2]] == [2, 2]
    # self
    line = CI.main(["self", "--bank", str(tmp_path / "train.pt"), "--top", "90", "--output", str(tmp_path / "s.jsonl")])
    recs = [json.loads(s) for s in (tmp_path / "s.jsonl").read_text().splitlines()]
    assert line["written"] == 90 == len(recs) and all(tuple(r) == CI.SELF_KEYS for r in recs)
    want = CI.reference_self_influence(T["features"], T["logits"], T["labels"], C)
    _, _, rsq, _, bar_sq = IR.residual_bars(T["logits"], T["labels"], C, "label", EXPF_BAR)
    fsq = (T["features"].double() ** 2).sum(1)
    tol = (fsq + 1.0) * bar_sq + 1.001 * (D + 2) * IR.U * want
    got = torch.empty(90, dtype=torch.float64)
    got[torch.tensor([r["row"] for r in recs])] = torch.tensor([r["value"] for r in recs], dtype=torch.float64)
    assert ((got - want).abs() <= tol).all()
    assert all(a["value"] >= b["value"] for a, b in zip(recs[:-1], recs[1:]))
    v = CI.self_influence(T)
    assert torch.equal(v.double()[torch.tensor([r["row"] for r in recs])], torch.tensor([r["value"] for r in recs], dtype=torch.float64))
