"""GPU: the four kernels of uvc_amd/csrc/cascade.hip through the C ABI with guarded buffers, ``Cascade.forward`` against the two modules
and against ``reference_cascade``, and the commands end to end.

Every test prints the worst figure it measured before it asserts (README "Two-model cascades" records them).
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import cascade_ref as CR
import knn_ref as KR
from uvc_amd import _lib as L
from uvc_amd import compact as CP
from uvc_amd import compact_cascade as CS
from uvc_amd import compact_compare as CC
from uvc_amd import ops

pytestmark = pytest.mark.gpu

# expf on the device has no documented bound here: tests/test_influence_gpu.py measures it through uvc_influence_expf (8.2616e-08 on an
# MI355X, EXPF_MEASURED there) and takes twice that; cascade.hip calls the same device function under the same compiler flags, and
# test_expf_error_is_what_the_bars_assume below measures it again over the arguments uvc_cascade_decide hands to it (d / T down to -500).
EXPF_MEASURED = 8.27e-8
EXPF_BAR = 2 * EXPF_MEASURED
LOGIT_BAR = {"fp32": 1e-3, "bf16": 2e-2}                     # tests/test_compact_gpu.py's eval-logit bar, of the largest logit
SENT = 7
INF = float("inf")
SHAPES = [(1, 8), (2, 2), (10, 16), (1000, 1000), (1003, 1008), (2500, 2504)]
ROWS = (1, 63, 64, 65, 1000)
TEMPERATURES = (0.5, 1.0, 3.0)
SMALL, LARGE = "stage2_micro_skip", "stage2_micro_deit"


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int16) if t.dtype == torch.bfloat16 else t)


def guarded(n, dtype, guard=4):
    """(a buffer of n + 2 guard elements filled with a sentinel, its [guard, guard + n) view); guard 4 keeps a 4-byte view 16-byte aligned"""
    full = torch.full((n + 2 * guard,), SENT, dtype=dtype, device="cuda")
    return full, full[guard:guard + n]


def intact(full, n, guard=4):
    return bool((full[:guard] == SENT).all()) and bool((full[guard + n:] == SENT).all())


def decide_raw(z, n, ld, C, T, kind, tau, score, top1, defer):
    return L.lib().uvc_cascade_decide(L.ptr(z), n, ld, C, T, CS.SCORES.index(kind), tau, L.ptr(score), L.ptr(top1), L.ptr(defer), L.cur_stream())


def decide(z, C, T, kind, tau, want=(True, True, True), guard=4):
    """(score, top1, defer) through the C ABI into guarded buffers (None where not wanted); asserts the return code and the guards"""
    n, ld = z.shape[0], (z.stride(0) if z.shape[0] > 1 else z.shape[1])
    bufs = [guarded(n, dt, guard) if w else (None, None) for w, dt in zip(want, (torch.float32, torch.int32, torch.int32))]
    assert decide_raw(z, n, ld, C, T, kind, tau, *(b[1] for b in bufs)) == 0
    torch.cuda.synchronize()
    assert all(b[0] is None or intact(b[0], n, guard) for b in bufs)
    return tuple(b[1] for b in bufs)


# ---- decide -----------------------------------------------------------------------------------------------------------------------------
def test_expf_error_is_what_the_bars_assume():
    g = torch.Generator().manual_seed(0)
    d = torch.cat([-torch.linspace(0, 104, 1 << 20), -(3 * torch.randn(1 << 20, generator=g)).abs(), -(30 * torch.randn(1 << 20, generator=g)).abs() / 0.5])
    e = ops.influence_expf(d.cuda()).cpu().double()
    want = torch.exp(d.double())
    normal = want >= 2.0 ** -126
    rel = float(((e - want).abs() / want)[normal].max())
    print(f"expf: worst relative error {rel:.4e} over {int(normal.sum())} arguments (bar {EXPF_BAR:.4e})")
    assert rel <= EXPF_BAR and ((e - want).abs()[~normal] <= 2.0 ** -149).all()
    assert float(ops.influence_expf(torch.zeros(1, device="cuda"))[0]) == 1.0


@pytest.mark.parametrize("C,ld", SHAPES)
def test_decide_equals_float64(C, ld):
    """score within ``cascade_ref.score_bars`` (derived there from the spec's operations with the measured expf error), top1 exact on rows
    with one maximum and the first column on the planted ties, defer exact against the kernel's own float32 score."""
    worst = {k: 0.0 for k in CS.SCORES}
    for n in ROWS:
        zh = CR.logits_case(n, C, ld, n + C)
        z = zh.cuda()
        zz = zh[:, :C].double()
        unique = (zz == zz.max(dim=1, keepdim=True)[0]).sum(dim=1) == 1
        first = CS.reference_top1(zh, C)
        for kind in CS.SCORES:
            for T in TEMPERATURES:
                ref, bar = CR.score_bars(zh, C, T, kind, EXPF_BAR)
                score, top1, defer = decide(z, C, T, kind, -INF)
                s = score.cpu()
                err = (s.double() - ref).abs()
                frac = float((err / bar).max())
                worst[kind] = max(worst[kind], frac)
                assert frac <= 1.0, (n, C, kind, T, frac, int((err / bar).argmax()))
                assert torch.equal(top1.cpu().long()[unique], first[unique]) and torch.equal(top1.cpu().long(), first), (n, C, kind, T)
                assert not bool(defer.any())                                     # tau = -inf never defers
                if C == 1:
                    assert torch.equal(s, torch.ones(n))
        # defer against the kernel's own score: +inf, a row's own score (kept: >=), the float32 just above it
        score = decide(z, C, 1.0, "msp", -INF, (True, False, False))[0]
        mid = float(torch.sort(score)[0][n // 2])
        for tau in (INF, mid, float(np.nextafter(np.float32(mid), np.float32(2.0))), 0.0):
            s2, _, defer = decide(z, C, 1.0, "msp", tau, (True, False, True))
            assert torch.equal(bits(s2), bits(score)) and torch.equal(defer.bool(), ~(score >= tau)), (n, C, tau)
            if tau == INF:
                assert bool(defer.all())
        only = decide(z, C, 1.0, "msp", mid, (False, False, True))[2]            # NULL outputs: the others are written
        assert torch.equal(only.bool(), ~(score >= mid)) and not bool(only[score == mid].any())
    print(f"cascade_decide C {C} ld {ld}: worst error / bar " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("C,ld", [(10, 16), (1003, 1008), (2500, 2504)])
def test_decide_unaligned_nan_rows_and_repeats(C, ld):
    zh = CR.logits_case(65, C, ld, 65 + C)
    z = zh.cuda()
    for kind in CS.SCORES:
        want = decide(z, C, 3.0, kind, 0.5)
        again = decide(z, C, 3.0, kind, 0.5, guard=3)                           # the same bits on a repeat, into unaligned outputs
        assert all(torch.equal(bits(p), bits(q)) for p, q in zip(want, again)), kind
        flat = torch.empty(65 * ld + 1, device="cuda")
        off = flat[1:].view(65, ld)                                              # one element off 16-byte alignment: element by element
        off.copy_(z)
        assert off.data_ptr() % 16 == 4
        assert all(torch.equal(bits(p), bits(q)) for p, q in zip(want, decide(off, C, 3.0, kind, 0.5))), kind
        wide = torch.full((65, ld + 3), float("nan"), device="cuda")           # a row stride that is no multiple of 16 bytes
        wide[:, :ld].copy_(z)
        assert all(torch.equal(bits(p), bits(q)) for p, q in zip(want, decide(wide[:, :ld], C, 3.0, kind, 0.5))), kind
        for i in (0, 64):                                                        # a row alone gives the bits it has among 65
            alone = decide(z[i:i + 1].clone(), C, 3.0, kind, 0.5)
            assert all(torch.equal(bits(p), bits(q[i:i + 1])) for p, q in zip(alone, want)), (kind, i)
        bad = z.clone()
        bad[7, C - 1] = float("nan")
        bad[40, 0] = float("nan")
        bad[41, :C] = -INF                                                       # no maximum: treated as a NaN row
        rows = torch.zeros(65, dtype=torch.bool, device="cuda")
        rows[[7, 40, 41]] = True
        s, t, d = decide(bad, C, 3.0, kind, -INF)
        assert bool(torch.isnan(s[rows]).all()) and bool((t[rows] == -1).all()) and bool((d[rows] == 1).all())      # a NaN score defers even at -inf
        assert torch.equal(bits(s[~rows]), bits(want[0][~rows])) and torch.equal(t[~rows], want[1][~rows]) and not bool(d[~rows].any())


def test_decide_refusals_leave_the_outputs_alone():
    z = CR.logits_case(8, 10, 16, 1).cuda()
    outs = [guarded(8, dt)[1] for dt in (torch.float32, torch.int32, torch.int32)]
    call = lambda n=8, ld=16, C=10, T=1.0, kind="msp", tau=0.5, z=z, outs=outs: decide_raw(z, n, ld, C, T, kind, tau, *outs)
    for kw in (dict(z=None), dict(n=0), dict(C=0), dict(C=17), dict(T=0.0), dict(T=-1.0), dict(T=INF), dict(T=float("nan")), dict(tau=float("nan")),
               dict(outs=[None, None, None])):
        assert call(**kw) == 1, kw                                               # UVC_ERR_ARG
    assert L.lib().uvc_cascade_decide(L.ptr(z), 8, 16, 10, 1.0, 3, 0.5, L.ptr(outs[0]), 0, 0, L.cur_stream()) == 1
    assert call(C=65537, ld=70000) == 3                                          # UVC_ERR_UNSUPPORTED
    for bad in (lambda: ops.cascade_decide(z.cpu()), lambda: ops.cascade_decide(z, 17), lambda: ops.cascade_decide(z, kind="energy"),
                lambda: ops.cascade_decide(z.bfloat16()), lambda: ops.cascade_decide(z, 10, 0.0), lambda: ops.cascade_decide(z, 10, 1.0, "msp", float("nan"))):
        with pytest.raises(L.UvcHipError):
            bad()
    torch.cuda.synchronize()
    assert all(bool((o == SENT).all()) for o in outs)
    assert call() == 0
    torch.cuda.synchronize()
    assert not any(bool((o == SENT).all()) for o in outs[:2])


# ---- compact ----------------------------------------------------------------------------------------------------------------------------
def compact_raw(defer, n, idx, pos, count, ws, ws_bytes):
    return L.lib().uvc_cascade_compact(L.ptr(defer), n, L.ptr(idx), L.ptr(pos), L.ptr(count), L.ptr(ws), ws_bytes, L.cur_stream())


def patterns(n):
    g = torch.Generator().manual_seed(n)
    first, last = torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32)
    first[0], last[-1] = 1, 1
    sparse = (torch.rand(n, generator=g) < 0.01).int()
    return dict(none=torch.zeros(n, dtype=torch.int32), all=torch.ones(n, dtype=torch.int32), alternating=(torch.arange(n) % 2).int(), first=first,
                last=last, random=(torch.rand(n, generator=g) < 0.4).int() * torch.randint(1, 9, (n,), generator=g).int(), sparse=sparse)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2047, 2048, 2049, 4096, 100003])
def test_compact_equals_nonzero_and_cumsum(n):
    ws_bytes = ops.cascade_compact_workspace_bytes(n)
    assert ws_bytes == (n + 2047) // 2048 * 4
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    for name, dh in patterns(n).items():
        for guard in (4, 3):                                                     # 16-byte aligned buffers, and buffers that are not
            dfull, d = guarded(n, torch.int32, guard)
            d.copy_(dh)
            (ifull, idx), (pfull, pos), (cfull, count) = guarded(n, torch.int32, guard), guarded(n, torch.int32, guard), guarded(1, torch.int32, guard)
            assert compact_raw(d, n, idx, pos, count, ws, ws_bytes) == 0
            torch.cuda.synchronize()
            flag = dh != 0
            want = torch.nonzero(flag)[:, 0]
            m = int(want.shape[0])
            assert int(count[0]) == m and torch.equal(idx[:m].cpu().long(), want), (n, name)
            assert bool((idx[m:] == SENT).all()), (n, name)                      # the slots past m keep their bytes
            assert torch.equal(pos.cpu().long(), torch.where(flag, torch.cumsum(flag.long(), 0) - 1, -1)), (n, name)
            assert intact(ifull, n, guard) and intact(pfull, n, guard) and intact(cfull, 1, guard) and intact(dfull, n, guard)
        i2, p2, c2 = ops.cascade_compact(d)                                      # the same bits on a repeat, through the wrapper
        assert torch.equal(i2[:m], idx[:m]) and torch.equal(p2, pos) and torch.equal(c2, count)
        only = guarded(n, torch.int32)
        assert compact_raw(d, n, None, only[1], count, ws, ws_bytes) == 0 and torch.equal(only[1], pos)      # idx NULL: pos is written
        only = guarded(n, torch.int32)
        assert compact_raw(d, n, only[1], None, count, ws, ws_bytes) == 0 and torch.equal(only[1][:m], idx[:m])


def test_compact_refusals():
    d = torch.ones(300, dtype=torch.int32, device="cuda")
    outs = [guarded(300, torch.int32)[1], guarded(300, torch.int32)[1], guarded(1, torch.int32)[1]]
    ws = torch.empty(8, dtype=torch.uint8, device="cuda")
    assert compact_raw(None, 300, *outs, ws, 8) == 1 and compact_raw(d, 0, *outs, ws, 8) == 1 and compact_raw(d, 300, None, None, outs[2], ws, 8) == 1
    assert compact_raw(d, 300, outs[0], outs[1], None, ws, 8) == 1 and compact_raw(d, 300, *outs, None, 8) == 1 and compact_raw(d, 300, *outs, ws, 3) == 1
    assert compact_raw(d, 1 << 31, *outs, ws, 8) == 1
    nbytes = ctypes.c_int64(-1)
    assert L.lib().uvc_cascade_compact_workspace_bytes(0, ctypes.byref(nbytes)) == 1 and L.lib().uvc_cascade_compact_workspace_bytes(5, None) == 1
    for bad in (lambda: ops.cascade_compact(d.cpu()), lambda: ops.cascade_compact(d.long()), lambda: ops.cascade_compact(d[:0]),
                lambda: ops.cascade_compact(d, idx=torch.empty(299, dtype=torch.int32, device="cuda"))):
        with pytest.raises(L.UvcHipError):
            bad()
    torch.cuda.synchronize()
    assert all(bool((o == SENT).all()) for o in outs)


# ---- gather -----------------------------------------------------------------------------------------------------------------------------
def gather_raw(src, ld_src, n, rpi, width, idx, m, dst, ld_dst, dt=None):
    dt = (L.UVC_F32 if src.dtype == torch.float32 else L.UVC_BF16) if dt is None else dt
    return L.lib().uvc_cascade_gather(L.ptr(src), ld_src, dt, n, rpi, width, L.ptr(idx), m, L.ptr(dst), ld_dst, L.cur_stream())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("width", [3, 48, 192, 768])
def test_gather_equals_index_select(dtype, width):
    n = 7
    g = torch.Generator().manual_seed(width)
    for rpi in (1, 16, 196):
        src = torch.randn(n * rpi, width, generator=g).to(dtype).cuda()
        items = src.view(n, rpi, width)
        for sel in ([], list(range(n)), [5, 0, 3], [6, 6, -1, 2, n, 1]):         # m = 0, m = n, a few, and indices outside [0, n): items of +0
            m = len(sel)
            idx = torch.full((n,), 3, dtype=torch.int32, device="cuda")
            idx[:m] = torch.tensor(sel, dtype=torch.int32)
            ok = torch.tensor([0 <= s < n for s in sel], dtype=torch.bool, device="cuda")
            want = torch.where(ok[:, None, None], items[torch.tensor([s if 0 <= s < n else 0 for s in sel], dtype=torch.long, device="cuda")],
                               torch.zeros((), dtype=dtype, device="cuda")).reshape(m * rpi, width) if m else src[:0]
            # dense on both sides (16-byte copies where the bytes allow), through guarded memory
            full, dst = guarded(max(m, 1) * rpi * width, dtype, 8)
            assert gather_raw(src, width, n, rpi, width, idx, m, dst, width) == 0
            torch.cuda.synchronize()
            assert intact(full, max(m, 1) * rpi * width, 8)
            if m:
                assert torch.equal(bits(dst.view(m * rpi, width)), bits(want)), (rpi, sel)
            else:
                assert bool((dst == SENT).all())                                 # m = 0: nothing is launched
            got = ops.cascade_gather(src, idx, m, rpi)
            assert got.shape == (m * rpi, width) and torch.equal(bits(got), bits(want))
            if not m:
                continue
            # off alignment and padded strides: a source one element into its buffer with rows 5 elements apart from dense, a strided destination
            lds, ldd = width + 5, width + 3
            sbuf = torch.full((n * rpi * lds + 1,), float("nan"), dtype=dtype, device="cuda")
            sview = sbuf[1:].view(n * rpi, lds)[:, :width]
            sview.copy_(src)
            dbuf = torch.full((m * rpi, ldd), SENT, dtype=dtype, device="cuda")
            assert gather_raw(sview, lds, n, rpi, width, idx, m, dbuf, ldd) == 0
            torch.cuda.synchronize()
            assert torch.equal(bits(dbuf[:, :width].contiguous()), bits(want)) and bool((dbuf[:, width:] == SENT).all()), (rpi, sel)
            assert torch.equal(bits(ops.cascade_gather(sview, idx, m, rpi, out=dbuf[:, :width])[:, :width].contiguous()), bits(want))


def test_gather_refusals():
    src = torch.randn(12, 8, device="cuda")
    idx = torch.zeros(3, dtype=torch.int32, device="cuda")
    full, dst = guarded(96, torch.float32)
    base = dict(src=src, ld_src=8, n=3, rpi=4, width=8, idx=idx, m=3, dst=dst, ld_dst=8, dt=L.UVC_F32)
    for kw in (dict(src=None), dict(idx=None), dict(dst=None), dict(n=0), dict(m=4), dict(m=-1), dict(rpi=0), dict(width=0), dict(ld_src=7), dict(ld_dst=7),
               dict(dt=2)):
        assert gather_raw(**dict(base, **kw)) == 1, kw
    for bad in (lambda: ops.cascade_gather(src.cpu(), idx, 1), lambda: ops.cascade_gather(src, idx, 4, 4), lambda: ops.cascade_gather(src, idx, 1, 5),
                lambda: ops.cascade_gather(src, idx.long(), 1), lambda: ops.cascade_gather(src.half(), idx, 1)):
        with pytest.raises(L.UvcHipError):
            bad()
    torch.cuda.synchronize()
    assert bool((full == SENT).all())


# ---- merge ------------------------------------------------------------------------------------------------------------------------------
def merge_raw(zs, lds, zl, ldl, m, pos, n, C, out, ldo, source):
    return L.lib().uvc_cascade_merge(L.ptr(zs), lds, L.ptr(zl), ldl, m, L.ptr(pos), n, C, L.ptr(out), ldo, L.ptr(source), L.cur_stream())


@pytest.mark.parametrize("n,C,lds,ldl,ldo", [(1, 1, 1, 2, 3), (65, 10, 16, 12, 10), (65, 10, 13, 19, 11), (130, 1000, 1000, 1008, 1004), (9, 2500, 2504, 2500, 2501)])
def test_merge_equals_where(n, C, lds, ldl, ldo):
    g = torch.Generator().manual_seed(n + C)
    zs = torch.randn(n, lds, generator=g).cuda()
    zs[0, 0] = float("nan")                                                      # bits are copied, whatever they are
    for name, defer in (("none", torch.zeros(n, dtype=torch.bool)), ("all", torch.ones(n, dtype=torch.bool)), ("some", torch.rand(n, generator=g) < 0.4)):
        m = int(defer.sum())
        pos = torch.where(defer, torch.cumsum(defer.long(), 0) - 1, -1).int().cuda()
        zl = torch.randn(max(m, 1), ldl, generator=g).cuda()
        full, flat = guarded(n * ldo, torch.float32)
        out = flat.view(n, ldo)
        sfull, source = guarded(n, torch.int32)
        assert merge_raw(zs, lds, zl if m else None, ldl, m, pos, n, C, out, ldo, source) == 0
        torch.cuda.synchronize()
        want = torch.where(defer.cuda()[:, None], zl[pos.long().clamp_min(0), :C], zs[:, :C])
        assert torch.equal(bits(out[:, :C].contiguous()), bits(want.contiguous())), name
        assert bool((out[:, C:] == SENT).all()) and intact(full, n * ldo) and intact(sfull, n)      # the columns past C are not written
        assert torch.equal(source.cpu(), defer.int())
        o2, s2 = ops.cascade_merge(zs, zl[:m], pos, C)
        assert o2.shape == (n, C) and torch.equal(bits(o2), bits(want.contiguous())) and torch.equal(s2, source)
        assert merge_raw(zs, lds, zl if m else None, ldl, m, pos, n, C, out, ldo, None) == 0          # source NULL
    if n > 1:
        pos = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        pos[1] = 1                                                               # a place past the large model's one row: NaN, source -1
        o, s = ops.cascade_merge(zs, zl[:1], pos, C)
        assert bool(torch.isnan(o[1]).all()) and int(s[1]) == -1 and torch.equal(bits(o[2:]), bits(zs[2:, :C].contiguous()))


def test_merge_refusals():
    zs, zl = torch.randn(8, 16, device="cuda"), torch.randn(8, 12, device="cuda")
    pos = torch.full((8,), -1, dtype=torch.int32, device="cuda")
    full, flat = guarded(80, torch.float32)
    out = flat.view(8, 10)
    base = dict(zs=zs, lds=16, zl=zl, ldl=12, m=8, pos=pos, n=8, C=10, out=out, ldo=10, source=None)
    for kw in (dict(zs=None), dict(zl=None), dict(pos=None), dict(out=None), dict(n=0), dict(m=9), dict(m=-1), dict(C=0), dict(C=13), dict(lds=9), dict(ldo=9)):
        assert merge_raw(**dict(base, **kw)) == 1, kw
    for bad in (lambda: ops.cascade_merge(zs.cpu(), zl, pos), lambda: ops.cascade_merge(zs, zl, pos, 13), lambda: ops.cascade_merge(zs, zl, pos.long()),
                lambda: ops.cascade_merge(zs, zl.double(), pos), lambda: ops.cascade_merge(zs, zl, pos[:7])):
        with pytest.raises(L.UvcHipError):
            bad()
    torch.cuda.synchronize()
    assert bool((full == SENT).all())
    assert merge_raw(**dict(base, zl=None, m=0)) == 0                            # nothing deferred: z_large may be NULL


# ---- Cascade.forward --------------------------------------------------------------------------------------------------------------------
def exports():
    ex_s, ex_l = KR.export_of(SMALL)[0], KR.export_of(LARGE)[0]
    assert ex_s["cfg"]["img_size"] == ex_l["cfg"]["img_size"] == 64 and ex_s["cfg"]["num_classes"] == ex_l["cfg"]["num_classes"] == 16
    return ex_s, ex_l


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_forward_is_the_two_modules_bit_for_bit(prec):
    ex_s, ex_l = exports()
    x = CR.cluster_batch(3).cuda()
    B, C = x.shape[0], 10
    probe = CS.Cascade(ex_s, ex_l, threshold=-INF, precision=prec)
    rows = probe.patch_rows(x)
    npi = probe.patches_per_image
    zs, zl = probe.small(patches=rows)[0], probe.large(patches=rows)[0]
    out, source, score = probe.forward(x, num_labels=C)
    assert out.shape == (B, C) and out.dtype == torch.float32 and source.dtype == torch.int32 and score.dtype == torch.float32
    assert torch.equal(bits(out), bits(zs[:, :C].contiguous())) and not bool(source.any()) and probe.deferred == 0      # tau = -inf: the small forward
    always = CS.Cascade(ex_s, ex_l, threshold=INF, precision=prec)
    out, source, _ = always.forward(x, num_labels=C)
    assert torch.equal(bits(out), bits(zl[:, :C].contiguous())) and bool(source.all()) and always.deferred == B      # tau = +inf: the large forward
    for kind in CS.SCORES:
        s0 = ops.cascade_decide(zs, C, 1.0, kind)[0]
        tau = CR.widest_gap(s0.cpu())[0]
        cas = CS.Cascade(ex_s, ex_l, score=kind, threshold=tau, precision=prec)
        out, source, score = cas.forward(x, num_labels=C)
        defer = ~(s0 >= torch.tensor(tau, dtype=torch.float32, device="cuda"))
        m = int(defer.sum())
        assert 0 < m < B and cas.deferred == m and torch.equal(source.bool(), defer) and torch.equal(bits(score), bits(s0))
        idx = torch.nonzero(defer)[:, 0]
        assert torch.equal(cas.last_idx.long(), idx)
        assert torch.equal(bits(out[~defer]), bits(zs[~defer][:, :C].contiguous()))                    # kept rows: the small module's, bit for bit
        sub = rows.view(B, npi, -1).index_select(0, idx).reshape(m * npi, -1).contiguous()
        assert torch.equal(bits(out[defer]), bits(cas.large(patches=sub)[0][:, :C].contiguous()))     # deferred rows: the large module on the same m images
        o2, s2, c2 = cas.forward(patches=rows, num_labels=C)                                          # x= and patches= give the same bits
        assert torch.equal(bits(o2), bits(out)) and torch.equal(s2, source) and torch.equal(bits(c2), bits(score))
        wide = cas.forward(x)[0]                                                                       # every column of the heads
        assert wide.shape == (B, 16)
    with pytest.raises(ValueError, match="pass one of x / patches"):
        probe.forward()
    with pytest.raises(ValueError, match="num_labels 17"):
        probe.forward(x, num_labels=17)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["msp", "margin"])
def test_forward_against_reference_cascade(prec, kind):
    """The deferred set equals the float64 reference's exactly and the merged logits are within the eval-logit bar.  tau is the midpoint
    of the widest gap between consecutive sorted REFERENCE scores in the 20 - 80 % range of the batch, and that gap is asserted to exceed
    twice the score bar: the logit bar times 1/2 / T for msp and 1 / T for margin (a softmax entry moves by at most half the logit error).
    No row is left out: the batch (``cascade_ref.cluster_batch(0)``, two clusters of flat images; its seed was picked on the CPU with
    ``reference_cascade``) has such a gap for both scores at both precisions."""
    ex_s, ex_l = exports()
    x, C, T = CR.cluster_batch(0), 10, 1.0
    s_ref = CS.reference_cascade(ex_s, ex_l, x, score=kind, temperature=T, threshold=0.0, num_labels=C)[2]
    tau, gap = CR.widest_gap(s_ref)
    zs, zl = (CP.reference_forward(ex, x.double())[:, :C] for ex in (ex_s, ex_l))
    big = max(float(zs.abs().max()), float(zl.abs().max()))
    logit_bar = LOGIT_BAR[prec] * big
    score_bar = logit_bar * (0.5 if kind == "msp" else 1.0) / T
    print(f"cascade {prec} {kind}: gap {gap:.4f} at tau {tau:.4f}, twice the score bar {2 * score_bar:.4f}")
    assert gap > 2 * score_bar
    ref, src_ref, _ = CS.reference_cascade(ex_s, ex_l, x, score=kind, temperature=T, threshold=tau, num_labels=C)
    assert 0 < int(src_ref.sum()) < len(x)
    out, source, score = CS.Cascade(ex_s, ex_l, score=kind, temperature=T, threshold=tau, precision=prec).forward(x.cuda(), num_labels=C)
    err_s, err_z = float((score.cpu().double() - s_ref).abs().max()), float((out.cpu().double() - ref).abs().max())
    print(f"cascade {prec} {kind}: score error {err_s:.2e} (bar {score_bar:.2e}), logit error {err_z:.2e} (bar {logit_bar:.2e})")
    assert torch.equal(source.cpu().long(), src_ref) and err_s <= score_bar and err_z <= logit_bar


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_commands(tmp_path, capsys, prec):
    """compact_compare run writes the banks, curve picks an operating point and writes the policy, run walks the split with it, predict
    classifies the same images as files.  The micro files are untrained, so the twelve images are labelled with the LARGE file's own top-1 (read
    from a first pair of banks): the large model is then right everywhere, the small one almost nowhere, ``--match_large 0`` has to defer
    (nearly) everything and ``--max_macs`` at half the large model's cost picks an interior point."""
    from PIL import Image
    ex_s, ex_l = exports()
    images, _ = KR.colour_images(12, 2)
    torch.save(ex_s, tmp_path / "s.pt")
    torch.save(ex_l, tmp_path / "l.pt")
    files = ["--small", str(tmp_path / "s.pt"), "--large", str(tmp_path / "l.pt")]
    banks = ["--bank_small", str(tmp_path / "bank_s.pt"), "--bank_large", str(tmp_path / "bank_l.pt")]
    labels = np.zeros(12, dtype=np.int64)
    for name in ("first", "id"):                                                # the second pass: the same images under the large file's labels
        root = KR.write_cifar10(str(tmp_path / name), KR.colour_images(6, 1), (images, labels))
        data = ["--dataset", "cifar10", "--data_dir", root, "--eval_batch_size", "8", "--num_workers", "2", "--precision", prec]
        CC.main(["run", "--a", str(tmp_path / "s.pt"), "--b", str(tmp_path / "l.pt"), "--bank_a", str(tmp_path / "bank_s.pt"),
                 "--bank_b", str(tmp_path / "bank_l.pt"), "--topk", "1"] + data)
        bank_s, bank_l = torch.load(tmp_path / "bank_s.pt"), torch.load(tmp_path / "bank_l.pt")
        labels = bank_l["logits"][:, :10].argmax(dim=1).numpy()
    assert torch.equal(bank_l["labels"], torch.from_numpy(labels))
    capsys.readouterr()
    macs_s, macs_l = CP.compact_macs(ex_s), CP.compact_macs(ex_l)
    top2 = torch.topk(bank_l["logits"][:, :10].double(), 2, dim=1)[0]
    clear_large = (top2[:, 0] - top2[:, 1]) > 2 * LOGIT_BAR[prec] * float(bank_l["logits"][:, :10].abs().max())
    os.makedirs(tmp_path / "img")
    for i, im in enumerate(images):
        Image.fromarray(im).save(tmp_path / "img" / f"{i:02d}.png")
    deferred = {}
    for tag, selector in (("match", ["--match_large", "0"]), ("half", ["--max_macs", str(macs_s + 0.5 * macs_l)])):
        policy, saved = str(tmp_path / f"{tag}.json"), str(tmp_path / f"{tag}.pt")
        rec = CS.main(["curve"] + banks + files + selector + ["--policy", policy, "--output", saved, "--points", "5"])
        assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == rec
        kw = dict(match_large=0.0) if tag == "match" else dict(max_macs=macs_s + 0.5 * macs_l)
        ref = CS.reference_curve(bank_s, bank_l, macs_small=macs_s, macs_large=macs_l, points=5, **kw)[0]
        assert (rec["images"], rec["counted"], rec["data_classes"]) == (12, 12, 10) and rec["small"] == ref["small"] and rec["large"] == ref["large"]
        assert rec["large"]["top1"] == 1.0 == rec["oracle"] and rec["small"]["top1"] < 0.5
        pol, curve = CS.load_policy(policy), torch.load(saved)
        want_defer = curve["defer_at_chosen"]
        m = deferred[tag] = int(want_defer.sum())
        assert m == round(pol["expected"]["defer_rate"] * 12) and (pol["img_size"], pol["patch_size"], pol["data_classes"]) == (64, 16, 10)
        if tag == "match":
            assert rec["chosen"]["accuracy"] == 1.0 and m >= 12 - round(rec["small"]["top1"] * 12)      # every row the small file gets wrong is deferred
        else:
            assert 0 < m <= 6 and rec["chosen"]["macs"] <= macs_s + 0.5 * macs_l
        run = CS.main(["run"] + files + ["--policy", policy, "--bank", str(tmp_path / "out.pt")] + data)
        assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == run
        out = torch.load(tmp_path / "out.pt")
        assert run["images"] == 12 and run["expected"] == pol["expected"] and run["img_per_s"] > 0
        assert run["deferred"] == m and run["deferred"] / 12 == pol["expected"]["defer_rate"] == run["defer_rate"]      # the number deferred, exactly
        assert torch.equal(out["source"].bool(), want_defer) and torch.equal(bits(out["score"]), bits(curve["score"]))      # the same kernel, the same score bits
        assert out["logits"].shape == (12, 10) and torch.equal(bits(out["logits"][~want_defer]), bits(bank_s["logits"][~want_defer][:, :10].contiguous()))
        # the large model saw another batch here (the deferred images alone): its top-1 is compared where its top-2 gap exceeds twice the logit bar
        clear = clear_large | ~want_defer
        pred, want_pred = out["logits"].argmax(dim=1), torch.where(want_defer, curve["top1_large"], curve["top1_small"])
        err = float((out["logits"][want_defer].double() - bank_l["logits"][want_defer][:, :10].double()).abs().max()) if m else 0.0
        print(f"cascade commands {prec} {tag}: {m} of 12 deferred at tau {pol['threshold']}, {int(clear.sum())} of 12 rows compared, top1 {run['top1']} "
              f"(expected {pol['expected']['accuracy']}), the large model's logits moved by {err:.2e} with the batch")
        assert torch.equal(pred[clear], want_pred[clear])
        if bool(clear.all()):
            assert run["top1"] == pol["expected"]["accuracy"]
        assert run["macs_per_image"] == macs_s + run["defer_rate"] * macs_l
        # predict on the same images as files marks the same rows "large"
        summary = CS.main(["predict"] + files + ["--policy", policy, "--images", str(tmp_path / "img"), "--preset", "cifar", "--batch_size", "8",
                                                "--precision", prec, "--topk", "3", "--output", str(tmp_path / "pred.jsonl"), "--num_workers", "2"])
        lines = [json.loads(l) for l in open(tmp_path / "pred.jsonl")]
        assert lines[-1] == summary and summary["images"] == 12 and summary["errors"] == 0 and summary["deferred"] == m
        assert [l["model"] == "large" for l in lines[:-1]] == want_defer.tolist()
        assert all(set(l) == {"file", "top", "model", "score"} and len(l["top"]) == 3 for l in lines[:-1])
    assert deferred["half"] < deferred["match"]
    # the -inf end by flag: nothing is deferred and the large model never runs
    none = CS.run_command(CS.build_parser().parse_args(["run"] + files + ["--threshold=-inf"] + data))[0]
    assert none["deferred"] == 0 and none["top1"] == rec["small"]["top1"] and none["large_top1_on_deferred"] is None and "expected" not in none
