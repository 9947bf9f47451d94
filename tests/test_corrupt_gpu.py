"""GPU: the corruption kernels of uvc_amd/csrc/corrupt.hip against the float64 spec as tests/corrupt_ref.py restates it -- every bar is stated
relative to the spec: 8 * 2^-24 * T for the pointwise kinds (T: the sum of the absolute values of the terms of the float64 formula; at most six
float32 operations of half an ulp each, either fma contraction), EZ_ULPS ulps of r in z for the Gaussian kinds, n * 2^-24 * sum |w x| for the
fma chains of the blurs and pixelate (the second blur pass on the device's own intermediate), bit for bit for impulse_noise -- then the
refusals, ``compact_corrupt.corrupt`` + forward against ``compact.reference_forward`` on the same corrupted batch, and the command."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import corrupt_ref as CR
import knn_ref as KR
from test_corrupt_cpu import MODULE_BAR, MODULE_MODELS, module_batch
from uvc_amd import _lib as L
from uvc_amd import compact as CP
from uvc_amd import compact_corrupt as CC
from uvc_amd import compact_tools as TL
from uvc_amd import ops

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (1, 3, 1, 3), (3, 3, 17, 17), (2, 3, 7, 33), (2, 3, 32, 32), (1, 3, 64, 65), (1, 3, 224, 224)]
SENTINEL = 768.0
EPS32 = 2.0 ** -24
# The error budget of z in ulps of r.  The ROCm tree at hand documents no bounds for logf, sqrtf, sinf / cosf, so z was measured against
# float64 on the full 24-bit grid of u1 (u2 at its edges, at the quarter turns and drawn) and of u2 (u1 at its edges and drawn) and on 2^20
# keyed draws: the largest error is 2.50 ulps of r (numpy's float32 evaluation of the same chain on the same inputs: 2.66); the bar is twice that.
EZ_MEASURED, EZ_ULPS = 2.5, 5.0
LEVEL = {"gaussian_noise": 0.38, "speckle_noise": 0.6, "impulse_noise": 0.27}
L_ARG, L_UNSUPPORTED = 1, 3                             # UVC_ERR_ARG, UVC_ERR_UNSUPPORTED
DT = {"fp32": 1e-3, "bf16": 2e-2}                       # tests/test_compact_gpu.py's bars, of the largest logit


def guarded(t, shift):
    """``(view, base)``: a copy of the host array ``t`` inside a SENTINEL-filled device buffer with 16 elements of guard on either side; the view
    starts on a 16-byte boundary, or with ``shift`` one element behind one"""
    t = torch.as_tensor(t)
    base = torch.full((t.numel() + 32,), SENTINEL, dtype=torch.float32, device="cuda")
    start = 17 if shift else 16
    view = base[start:start + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == (4 if shift else 0)
    return view, base


def guards_intact(view, base, shift):
    start = 17 if shift else 16
    return bool((base[:start] == SENTINEL).all()) and bool((base[start + view.numel():] == SENTINEL).all())


def sentinel_out(shape, shift):
    return guarded(np.full(shape, SENTINEL, np.float32), shift)


def bits(t):
    return t.contiguous().view(torch.int32)


def per_channel(v, C):
    return np.asarray(v).reshape(1, C, 1, 1)


def index0s(shape):
    chw = shape[1] * shape[2] * shape[3]
    return [0, 5, (1 << 33) // chw + 7]                    # the last: the pair counter g >> 1 lies past 2^32


# ---- noise ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", CC.NOISES)
def test_noise_against_the_spec(kind):
    a, worst = LEVEL[kind], 0.0
    for si, shape in enumerate(SHAPES):
        B, Cc, H, W = shape
        mean, std = CR.stats(Cc)
        lo, hi = CR.bounds(mean, std)
        x = CR.images(shape, 20 + si, mean, std)
        chw = Cc * H * W
        for index0 in index0s(shape):
            ref, T, zt = CR.noise_flat(x.reshape(-1), 0, kind, a, mean, std, Cc, H * W, 4, 11, index0 * chw)
            ch = CR.channel_of(np.arange(x.size), Cc, H * W)
            first = None
            for shift in (0, 1):
                xv, xb = guarded(x, shift)
                ov, ob = sentinel_out(shape, shift)
                kw = dict(mean=mean, std=std, lo=lo, hi=hi, seed=4, stream=11)
                got = ops.corrupt_noise(xv, kind, a, index0=index0, out=ov, **kw)
                assert got is ov and guards_intact(ov, ob, shift) and guards_intact(xv, xb, shift) and torch.equal(xv.cpu(), torch.from_numpy(x))
                g = got.cpu().numpy().reshape(-1)
                if kind == "impulse_noise":
                    assert np.array_equal(g.view(np.int32), ref.astype(np.float32).view(np.int32)), (shape, index0, shift)
                    assert ((g == lo[ch]) | (g == hi[ch]) | (g == x.reshape(-1))).all()
                else:
                    worst = max(worst, CR.check(g, ref, 8 * EPS32 * T + EZ_ULPS * zt, lo[ch], hi[ch]))
                assert torch.equal(bits(ops.corrupt_noise(xv, kind, a, index0=index0, **kw)), bits(got))          # a repeat, and a new output
                first = got.clone() if first is None else first
                assert torch.equal(bits(first), bits(got))                                                      # either alignment
                if B > 1:                                                                                       # a batch split in two
                    h = B // 2
                    parts = [ops.corrupt_noise(xv[:h], kind, a, index0=index0, **kw), ops.corrupt_noise(xv[h:], kind, a, index0=index0 + h, **kw)]
                    assert torch.equal(bits(torch.cat(parts)), bits(got)), (shape, index0, shift)
    print(kind, "worst error / bar", worst)
    assert worst <= 1.0


def test_level_zero_and_in_place():
    mean, std = CR.stats(3)
    lo, hi = CR.bounds(mean, std)
    x = torch.from_numpy(CR.images((2, 3, 17, 17), 1, mean, std)).cuda()
    for kind in CC.NOISES:
        assert torch.equal(bits(ops.corrupt_noise(x, kind, 0.0, mean=mean, std=std, lo=lo, hi=hi, index0=3)), bits(x))
        want = ops.corrupt_noise(x, kind, LEVEL[kind], mean=mean, std=std, lo=lo, hi=hi)
        y = x.clone()
        assert ops.corrupt_noise(y, kind, LEVEL[kind], mean=mean, std=std, lo=lo, hi=hi, out=y) is y and torch.equal(bits(y), bits(want))


def test_box_muller_on_edges_and_draws():
    """z of the device against float64 at the ends of the 24-bit grid, at the quarter turns and on 2^16 keyed draws: within EZ_ULPS ulps of r."""
    grid = lambda c: ((np.asarray(c, np.float64) + 0.5) * 2.0 ** -24).astype(np.float32)
    edge = np.array([0, 1, 2, 2 ** 22 - 1, 2 ** 22, 2 ** 23 - 1, 2 ** 23, 3 * 2 ** 22 - 1, 3 * 2 ** 22, 2 ** 24 - 3, 2 ** 24 - 2])
    u1 = np.concatenate([np.repeat(grid(edge), len(edge)), CR.NR.uniforms(1, 2, 0, 1 << 16)])
    u2 = np.concatenate([np.tile(grid(edge), len(edge)), CR.NR.uniforms(1, 2, 1, 1 << 16)])
    z0, z1 = ops.box_muller(torch.from_numpy(u1).cuda(), torch.from_numpy(u2).cuda())
    r = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    t = (CR.TWO_PI_F32 * u2).astype(np.float32).astype(np.float64)
    ulp = 2.0 ** (np.floor(np.log2(r)) - 23)
    worst = max(float((np.abs(z0.cpu().numpy() - r * np.cos(t)) / ulp).max()), float((np.abs(z1.cpu().numpy() - r * np.sin(t)) / ulp).max()))
    print("box-muller worst error in ulps of r", worst)
    assert worst <= EZ_ULPS


def test_noise_past_2_31_bytes():
    """One speckle_noise call whose output passes 2^31 bytes: the first and last 4096 elements and 4096 around the 2^31-byte boundary."""
    shape = (3567, 3, 224, 224)
    n, a = int(np.prod(shape)), 0.6
    assert n * 4 > 1 << 31
    mean, std = CR.stats(3)
    lo, hi = CR.bounds(mean, std)
    x = torch.rand(n, device="cuda").mul_(3.5).sub_(1.75).view(shape)
    out = ops.corrupt_noise(x, "speckle_noise", a, mean=mean, std=std, lo=lo, hi=hi, seed=9, stream=2, index0=1)
    for e0 in (0, (1 << 29) - 2048, n - 4096):
        xs, g = x.view(-1)[e0:e0 + 4096].cpu().numpy(), out.view(-1)[e0:e0 + 4096].cpu().numpy()
        ref, T, zt = CR.noise_flat(xs, e0, "speckle_noise", a, mean, std, 3, 224 * 224, 9, 2, 3 * 224 * 224)
        ch = CR.channel_of(e0 + np.arange(4096), 3, 224 * 224)
        assert CR.check(g, ref, 8 * EPS32 * T + EZ_ULPS * zt, lo[ch], hi[ch]) <= 1.0, e0
    del x, out
    torch.cuda.empty_cache()


# ---- colour -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, levels", [("brightness", (0.1, 0.5)), ("contrast", (0.4, 0.05, 1.0))])
def test_colour_against_the_spec(kind, levels):
    worst = worst_mean = 0.0
    for si, shape in enumerate(SHAPES):
        B, Cc, H, W = shape
        mean, std = CR.stats(Cc)
        lo, hi = CR.bounds(mean, std)
        x = CR.images(shape, 40 + si, mean, std)
        for a in levels:
            first = None
            for shift in (0, 1):
                xv, xb = guarded(x, shift)
                ov, ob = sentinel_out(shape, shift)
                kw = dict(mean=mean, std=std, lo=lo, hi=hi)
                if kind == "contrast":
                    got, mu = ops.corrupt_colour(xv, kind, a, out=ov, **kw)
                    want_mu, pmax = CR.image_mean(x, mean, std)
                    worst_mean = max(worst_mean, float((np.abs(mu.cpu().numpy() - want_mu) / (2 * EPS32 * pmax)).max()))
                    ref, T = CR.contrast(x, a, mean, std, mu.cpu().numpy())              # the pointwise step, on the device's own mean
                    skip = None
                else:
                    got = ops.corrupt_colour(xv, kind, a, out=ov, **kw)
                    ref, T, skip = CR.brightness(x, a, mean, std)
                assert got is ov and guards_intact(ov, ob, shift) and guards_intact(xv, xb, shift)
                worst = max(worst, CR.check(got.cpu().numpy(), ref, 8 * EPS32 * T, per_channel(lo, Cc), per_channel(hi, Cc), skip))
                again = ops.corrupt_colour(xv, kind, a, **kw)
                assert torch.equal(bits(again[0] if kind == "contrast" else again), bits(got))
                first = got.clone() if first is None else first
                assert torch.equal(bits(first), bits(got))
                if B > 1:
                    parts = [ops.corrupt_colour(xv[:1], kind, a, **kw), ops.corrupt_colour(xv[1:], kind, a, **kw)]
                    parts = [p[0] if kind == "contrast" else p for p in parts]
                    assert torch.equal(bits(torch.cat(parts)), bits(got))
                if kind == "contrast" and a == 1.0:
                    assert torch.equal(got.cpu(), torch.from_numpy(x))
    print(kind, "worst error / bar", worst, "mean / bar", worst_mean)
    assert worst <= 1.0 and worst_mean <= 1.0


# ---- the blurs and pixelate -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma, R", [(0.25, 1), (1.0, 4), (6.0, 24), (8.0, 32)])
def test_gaussian_blur_against_the_spec(sigma, R):
    taps = CR.gaussian_taps(sigma)
    assert len(taps) == 2 * R + 1 and np.array_equal(taps, CC.gaussian_taps(sigma))
    n, worst1, worst2 = len(taps), 0.0, 0.0
    for si, shape in enumerate(SHAPES):
        Cc = shape[1]
        mean, std = CR.stats(Cc)
        lo, hi = CR.bounds(mean, std)
        x = CR.images(shape, 60 + si, mean, std)
        ref1, mag1 = CR.filter_axis(x, taps, 3)
        first = None
        for shift in (0, 1):
            xv, xb = guarded(x, shift)
            ov, ob = sentinel_out(shape, shift)
            sv, sb = sentinel_out(shape, shift)
            got = ops.blur_separable(xv, taps, lo=lo, hi=hi, scratch=sv, out=ov)
            assert got is ov and guards_intact(ov, ob, shift) and guards_intact(sv, sb, shift) and guards_intact(xv, xb, shift)
            mid = sv.cpu().numpy()
            bar1 = n * EPS32 * mag1
            assert (np.abs(mid - ref1) <= bar1).all(), (shape, shift)
            worst1 = max(worst1, float((np.abs(mid - ref1) / np.where(bar1 > 0, bar1, 1)).max()))
            ref2, mag2 = CR.filter_axis(mid, taps, 2)                                   # the second pass on the device's own intermediate
            worst2 = max(worst2, CR.check(got.cpu().numpy(), ref2, n * EPS32 * mag2, per_channel(lo, Cc), per_channel(hi, Cc)))
            assert torch.equal(bits(ops.blur_separable(xv, taps, lo=lo, hi=hi)), bits(got))
            first = got.clone() if first is None else first
            assert torch.equal(bits(first), bits(got))
            if shape[0] > 1:
                parts = [ops.blur_separable(xv[:1], taps, lo=lo, hi=hi), ops.blur_separable(xv[1:], taps, lo=lo, hi=hi)]
                assert torch.equal(bits(torch.cat(parts)), bits(got))
    print("gaussian_blur R", R, "worst error / bar: pass 1", worst1, "pass 2", worst2)
    assert worst2 <= 1.0


@pytest.mark.parametrize("r", [1, 3, 10, 12])
def test_defocus_blur_against_the_spec(r):
    taps, worst = CR.disk_taps(r), 0.0
    taps_dev = torch.from_numpy(taps).cuda()
    for si, shape in enumerate(SHAPES):
        Cc = shape[1]
        mean, std = CR.stats(Cc)
        lo, hi = CR.bounds(mean, std)
        x = CR.images(shape, 80 + si, mean, std)
        ref, mag, n = CR.stencil(x, taps)
        first = None
        for shift in (0, 1):
            xv, xb = guarded(x, shift)
            ov, ob = sentinel_out(shape, shift)
            got = ops.stencil2d(xv, taps_dev, lo=lo, hi=hi, out=ov)
            assert got is ov and guards_intact(ov, ob, shift) and guards_intact(xv, xb, shift)
            worst = max(worst, CR.check(got.cpu().numpy(), ref, n * EPS32 * mag, per_channel(lo, Cc), per_channel(hi, Cc)))
            assert torch.equal(bits(ops.stencil2d(xv, taps_dev, lo=lo, hi=hi)), bits(got))
            first = got.clone() if first is None else first
            assert torch.equal(bits(first), bits(got))
            if shape[0] > 1:
                parts = [ops.stencil2d(xv[:1], taps_dev, lo=lo, hi=hi), ops.stencil2d(xv[1:], taps_dev, lo=lo, hi=hi)]
                assert torch.equal(bits(torch.cat(parts)), bits(got))
        if si == 2:                                                                     # the module's path gives the same bits
            xd = torch.from_numpy(x).cuda()
            assert torch.equal(bits(CC.corrupt(xd, "defocus_blur", level=r, mean=mean, std=std)), bits(ops.stencil2d(xd, taps_dev, lo=lo, hi=hi)))
    print("defocus_blur r", r, "worst error / bar", worst)
    assert worst <= 1.0


def test_pixelate_against_the_spec():
    worst = 0.0
    for si, shape in enumerate(SHAPES):
        Cc, H = shape[1], shape[2]
        mean, std = CR.stats(Cc)
        lo, hi = CR.bounds(mean, std)
        x = CR.images(shape, 90 + si, mean, std)
        for k in sorted({1, 2, 3, 6, 7, 16, 17, H + 1}):                                # 16 / 17: the last cell one thread sums, the first a workgroup does
            ref, mag, cnt = CR.pixelate(x, k)
            first = None
            for shift in (0, 1):
                xv, xb = guarded(x, shift)
                ov, ob = sentinel_out(shape, shift)
                got = ops.pixelate(xv, k, lo=lo, hi=hi, out=ov)
                assert got is ov and guards_intact(ov, ob, shift) and guards_intact(xv, xb, shift)
                worst = max(worst, CR.check(got.cpu().numpy(), ref, cnt * EPS32 * mag, per_channel(lo, Cc), per_channel(hi, Cc)))
                if k == 1:
                    assert torch.equal(bits(got), bits(xv))
                assert torch.equal(bits(ops.pixelate(xv, k, lo=lo, hi=hi)), bits(got))
                first = got.clone() if first is None else first
                assert torch.equal(bits(first), bits(got))
                if shape[0] > 1:
                    assert torch.equal(bits(torch.cat([ops.pixelate(xv[:1], k, lo=lo, hi=hi), ops.pixelate(xv[1:], k, lo=lo, hi=hi)])), bits(got))
    print("pixelate worst error / bar", worst)
    assert worst <= 1.0


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    """Every refusal returns its code and leaves sentinel-filled outputs alone (the C entry points themselves: ops refuses the same on the host)."""
    lib = L.lib()
    shape = (2, 3, 8, 8)
    mean, std = CR.stats(3)
    lo, hi = CR.bounds(mean, std)
    x = torch.from_numpy(CR.images(shape, 0, mean, std)).cuda()
    out, scratch, mu = torch.full(shape, SENTINEL, device="cuda"), torch.full(shape, SENTINEL, device="cuda"), torch.full((2,), SENTINEL, device="cuda")
    taps_dev = torch.from_numpy(CR.disk_taps(1)).cuda()
    st = L.cur_stream()
    F4, D4 = C.c_float * 4, C.c_double * 4

    def args(kind, level=0.1, **over):
        a = L.uvc_corrupt_args()
        a.x, a.out, a.image_mean, a.level, a.kind = L.ptr(x), L.ptr(out), L.ptr(mu), level, kind
        a.B, a.C, a.H, a.W = shape
        a.mean, a.std, a.lo, a.hi = D4(*mean, 0), D4(*std, 1), F4(*lo, 0), F4(*hi, 0)
        for k, v in over.items():
            setattr(a, k, v)
        return a

    nan = float("nan")
    cases = []
    for fn, kind in ((lib.uvc_corrupt_noise, 0), (lib.uvc_corrupt_noise, 2), (lib.uvc_corrupt_colour, 3), (lib.uvc_corrupt_colour, 4)):
        for over in (dict(x=0), dict(out=0), dict(B=0), dict(H=0), dict(C=5), dict(level=nan), dict(level=-0.5), dict(std=D4(0.2, 0.0, 0.2, 1)),
                     dict(std=D4(0.2, -1.0, 0.2, 1)), dict(std=D4(0.2, 1e-60, 0.2, 1))):
            cases.append((fn, args(kind, **over), L_ARG))
        cases.append((fn, args(7), L_ARG))
        cases.append((fn, args(kind, C=1, H=65536, W=65536), L_UNSUPPORTED))
    cases.append((lib.uvc_corrupt_noise, args(2, 1.5), L_ARG))
    cases.append((lib.uvc_corrupt_noise, args(0, 0.1, index0=-1), L_ARG))
    cases.append((lib.uvc_corrupt_colour, args(4, 0.4, image_mean=0), L_ARG))
    for fn, a, code in cases:
        assert fn(C.byref(a), st) == code, (a.kind, a.B, a.C, a.H, a.level)
    f3 = lambda v: (C.c_float * 3)(*[float(u) for u in v])
    taps = (C.c_float * 67)(*([1.0 / 67] * 67))
    plane = (6, 3, 8, 8)
    assert lib.uvc_blur_separable(L.ptr(x), L.ptr(scratch), L.ptr(out), taps, 33, *plane, f3(lo), f3(hi), st) == L_ARG
    assert lib.uvc_blur_separable(L.ptr(x), L.ptr(scratch), L.ptr(out), taps, -1, *plane, f3(lo), f3(hi), st) == L_ARG
    assert lib.uvc_blur_separable(L.ptr(x), 0, L.ptr(out), taps, 1, *plane, f3(lo), f3(hi), st) == L_ARG
    assert lib.uvc_blur_separable(L.ptr(x), L.ptr(out), L.ptr(out), taps, 1, *plane, f3(lo), f3(hi), st) == L_ARG
    assert lib.uvc_blur_separable(L.ptr(x), L.ptr(scratch), L.ptr(out), taps, 1, 6, 5, 8, 8, None, None, st) == L_ARG
    assert lib.uvc_blur_separable(L.ptr(x), L.ptr(scratch), L.ptr(out), taps, 1, 0, 3, 8, 8, None, None, st) == L_ARG
    for K in (1, 2, 4, 27):                                                             # r < 1, an even width, r > 12
        assert lib.uvc_stencil2d(L.ptr(x), L.ptr(out), L.ptr(taps_dev), K, *plane, f3(lo), f3(hi), st) == L_ARG
    assert lib.uvc_stencil2d(L.ptr(x), L.ptr(out), 0, 3, *plane, f3(lo), f3(hi), st) == L_ARG
    assert lib.uvc_stencil2d(0, L.ptr(out), L.ptr(taps_dev), 3, *plane, f3(lo), f3(hi), st) == L_ARG
    assert lib.uvc_stencil2d(L.ptr(x), L.ptr(out), L.ptr(taps_dev), 3, 6, 3, 8, 0, None, None, st) == L_ARG
    for k in (0, -3):
        assert lib.uvc_pixelate(L.ptr(x), L.ptr(out), k, *plane, f3(lo), f3(hi), st) == L_ARG
    assert lib.uvc_pixelate(L.ptr(x), 0, 2, *plane, f3(lo), f3(hi), st) == L_ARG
    assert lib.uvc_pixelate(L.ptr(x), L.ptr(out), 2, 6, 3, 8, 8, f3(lo), None, st) == L_ARG
    assert lib.uvc_box_muller(L.ptr(x), L.ptr(x), L.ptr(out), L.ptr(scratch), 0, st) == L_ARG
    torch.cuda.synchronize()
    for t in (out, scratch, mu):
        assert bool((t == SENTINEL).all())
    for bad in (lambda: ops.corrupt_noise(x, "impulse_noise", 1.5, mean=mean, std=std, lo=lo, hi=hi),
                lambda: ops.corrupt_noise(x, "contrast", 0.1, mean=mean, std=std, lo=lo, hi=hi),
                lambda: ops.corrupt_noise(x, "gaussian_noise", nan, mean=mean, std=std, lo=lo, hi=hi),
                lambda: ops.corrupt_colour(x, "brightness", -1, mean=mean, std=std, lo=lo, hi=hi),
                lambda: ops.corrupt_colour(x, "brightness", 0.1, mean=mean, std=(0.2, 0.0, 0.2), lo=lo, hi=hi),
                lambda: ops.corrupt_colour(x.cpu(), "brightness", 0.1, mean=mean, std=std, lo=lo, hi=hi),
                lambda: ops.blur_separable(x, [1.0 / 67] * 67), lambda: ops.blur_separable(x, [0.5, 0.5]),
                lambda: ops.stencil2d(x, torch.ones(27, 27, device="cuda")), lambda: ops.stencil2d(x, torch.ones(1, 1, device="cuda")),
                lambda: ops.pixelate(x, 0), lambda: ops.pixelate(x, 2, out=x)):
        with pytest.raises(L.UvcHipError):
            bad()
    for bad in (lambda: CC.corrupt(x, "defocus_blur", level=13, mean=mean, std=std), lambda: CC.corrupt(x, "defocus_blur", level=0, mean=mean, std=std),
                lambda: CC.corrupt(x, "gaussian_blur", level=8.2, mean=mean, std=std), lambda: CC.corrupt(x, "pixelate", severity=6, mean=mean, std=std),
                lambda: CC.corrupt(x, "pixelate", mean=mean, std=std), lambda: CC.corrupt(x, "jpeg", severity=1, mean=mean, std=std)):
        with pytest.raises(ValueError):
            bad()


# ---- the module -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", MODULE_MODELS)
def test_module_against_the_reference_forward_on_the_same_corrupted_batch(name, prec):
    ex, _ = KR.export_of(name)
    x, mean, std = module_batch(ex)
    xd = torch.from_numpy(x).cuda()
    model = CP.CompactVisionTransformer(ex, precision=prec, device=xd.device)
    nl, tol = ex["cfg"]["num_classes"], DT[prec]
    triples = undecided = wide = 0
    worst = 0.0
    for kind in CC.CORRUPTIONS:
        for sev in CC.SEVERITIES:
            xc = CC.corrupt(xd, kind, severity=sev, mean=mean, std=std)
            assert xc.shape == xd.shape and xc.dtype == torch.float32 and not torch.equal(xc, xd)
            logits = model(xc)[0]
            hit = ops.logits_topk(logits, 1, nl)[1][:, 0].cpu().long()
            ref = CP.reference_forward(ex, xc.cpu().double())
            scale = float(ref.abs().max())
            worst = max(worst, float((logits.double().cpu() - ref).abs().max()) / scale)
            top2 = ref.topk(2, dim=1)
            sure = (top2.values[:, 0] - top2.values[:, 1]) > 2 * tol * scale
            assert torch.equal(hit[sure], top2.indices[sure, 0]), (kind, sev)
            triples += len(sure)
            undecided += int((~sure).sum())
            wide += int(((top2.values[:, 0] - top2.values[:, 1]) <= 2 * MODULE_BAR * scale).sum())
    print(name, prec, "worst logit error / largest logit", worst, "undecided", undecided / triples, "at the bf16 bar", wide / triples)
    assert worst <= tol
    assert undecided / triples <= 0.10 and wide / triples <= 0.10


# ---- the command ------------------------------------------------------------------------------------------------------------------------
KEYS = {"images", "clean_top1", "kinds", "mean_corruption_error", "img_per_s", "blocks", "params", "macs_full", "macs_compact", "macs_compact_padded"}


def test_command(tmp_path, capsys):
    """tests/test_robust_gpu.py's pattern: three flat-coloured classes through the CIFAR-10 reader, 12 test images, batches of 8."""
    ex, _ = KR.export_of("stage2_micro_deit")
    train, test = KR.colour_images(30, 1), KR.colour_images(12, 2)
    root = KR.write_cifar10(str(tmp_path / "data"), train, test)
    torch.save(ex, tmp_path / "f.pt")
    common = ["--compact", str(tmp_path / "f.pt"), "--dataset", "cifar10", "--data_dir", root, "--eval_batch_size", "8", "--num_workers", "2",
              "--precision", "fp32"]
    capsys.readouterr()
    kinds = ["gaussian_noise", "contrast", "pixelate"]
    line = CC.main([*common, "--kinds", *kinds, "--severities", "1", "5", "--output", str(tmp_path / "t.json")])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == line and set(line) >= KEYS
    assert json.load(open(tmp_path / "t.json")) == line
    assert line["images"] == 12 and list(line["kinds"]) == kinds and line["img_per_s"] > 0 and "mCE" not in line
    for kind in kinds:
        row = line["kinds"][kind]
        assert set(row) == {"levels", "top1", "error", "mean_error"} and row["levels"] == [CC.SEVERITY[kind][0], CC.SEVERITY[kind][4]]
        assert row["error"] == [100.0 - t for t in row["top1"]] and row["mean_error"] == sum(row["error"]) / 2
    assert line["mean_corruption_error"] == sum(line["kinds"][k]["mean_error"] for k in kinds) / 3
    # the per-cell counts: a hand loop over the same loader at the same batch size
    args = CC.build_parser().parse_args(common)
    mean, std = CC.preset_stats("cifar10")
    model = CP.CompactVisionTransformer(ex, precision="fp32", device=torch.device("cuda", torch.cuda.current_device()))
    loader, classes = TL.eval_loader(ex, args, "test")
    nl = CP.num_labels(ex["cfg"], classes)
    counts, clean, n = {(k, s): 0 for k in kinds for s in (1, 5)}, 0, 0
    for xb, yb in loader:
        top = lambda t: ops.logits_topk(model(t)[0], 1, nl)[1][:, 0].long()
        clean += int((top(xb) == yb.long()).sum())
        for k, s in counts:
            counts[(k, s)] += int((top(CC.corrupt(xb, k, severity=s, mean=mean, std=std, seed=0, index0=n)) == yb.long()).sum())
        n += xb.shape[0]
    assert n == 12 and line["clean_top1"] == 100.0 * clean / 12
    for k in kinds:
        assert line["kinds"][k]["top1"] == [100.0 * counts[(k, 1)] / 12, 100.0 * counts[(k, 5)] / 12], k
    zero = CC.main([*common, "--kinds", "gaussian_noise", "--level", "0"])
    assert zero["kinds"]["gaussian_noise"]["top1"] == [zero["clean_top1"]] and zero["clean_top1"] == line["clean_top1"]
    assert zero["kinds"]["gaussian_noise"]["levels"] == [0.0]
    both = CC.main([*common, "--baseline", str(tmp_path / "f.pt"), "--kinds", *kinds, "--severities", "1", "5", "--max_images", "10"])
    assert both["images"] == 10 and both["baseline"]["kinds"] == {k: {f: v for f, v in r.items() if f not in ("ce", "relative_ce")} for k, r in both["kinds"].items()}
    for k in kinds:
        assert both["kinds"][k]["ce"] in (1.0, None) and both["kinds"][k]["relative_ce"] in (1.0, None)
    assert both["mCE"] in (1.0, None) and both["relative_mCE"] in (1.0, None)
    assert (both["mCE"] is None) == (both["mCE_kinds"] == 0) and (both["relative_mCE"] is None) == (both["relative_mCE_kinds"] == 0)
    capsys.readouterr()
