"""GPU: the layout kernels of uvc_amd/csrc/elementwise.hip that move or blend values without a reduction -- uvc_patchify, uvc_cast_transpose,
uvc_cast_transpose_multi, uvc_mixup_batch, uvc_mixup_target -- through their C entries.  Every comparison is exact (torch.equal): a copy, one
rounding to bf16, or three separately rounded float32 operations that torch on the host performs in the same order.  Every output lies inside a
sentinel-filled parent that is compared as a whole, so a stray write shows as well as a missing one.

  uvc_patchify             16-byte loads, P / 4 vectors per patch row: P = 4 (one vector), 8, 12 (P / 4 odd), 16, 32; C = 1, 3, 4; one patch per image
                           and 196; 33 x 2 x 256 x 256 has 1081344 vectors, past grid_for's 4096 * 256, and runs the grid-stride loop
  uvc_cast_transpose       32 x 32 tiles of 8 x 32 threads: R, C on both sides of one and of two tiles, one row, one column
  uvc_cast_transpose_multi 64 x 64 tiles; the vector path (R, C and all three offsets multiples of 4) and the scalar path on the same matrices
                           must agree bit for bit; a full table of 64 entries for the ballot lookup
  uvc_mixup_batch / _target  lam = 0, 1, 0.3 and the float32 below 1; CutMix boxes empty, one pixel in each corner, the full frame"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
SENT = -7.0
GUARD = 64                                          # elements of sentinel on either side of an output; a multiple of 4 keeps 16-byte alignment


def dev():
    return torch.device("cuda")


def tt(dtype):
    return torch.float32 if dtype == F32 else torch.bfloat16


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def parent(n, dtype, lead=GUARD):
    """(parent, view of n elements at ``lead``) on the device, the parent full of the sentinel."""
    p = torch.full((lead + n + GUARD,), SENT, device=dev(), dtype=tt(dtype))
    return p, p[lead:lead + n]


def expect(n, dtype, values, lead=GUARD):
    """The parent a correct kernel leaves: the sentinel around ``values`` (host)."""
    p = torch.full((lead + n + GUARD,), SENT, dtype=tt(dtype))
    p[lead:lead + n] = values.reshape(-1).to(tt(dtype))
    return p


def refused(rc, what):
    from uvc_amd import _lib as L
    assert rc == 1 and L.lib().uvc_last_error(), f"{what}: rc = {rc}"


# ============================================================================= uvc_patchify
PATCHIFY = [(1, 1, 4, 4), (1, 3, 8, 4), (2, 3, 32, 8), (3, 4, 64, 16), (1, 3, 64, 32), (2, 3, 48, 12), (1, 3, 224, 16), (33, 2, 256, 16)]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("B,Cc,S,P", PATCHIFY)
def test_patchify_equals_unfold(B, Cc, S, P, dtype):
    from uvc_amd import ops
    x = rnd(B, Cc, S, S, seed=B + 10 * Cc + 100 * S + P)
    n = B * Cc * S * S
    if (B, S) == (33, 256):
        assert n // 4 > 4096 * 256                   # more vectors than grid_for's cap has threads
    want = F.unfold(x, P, stride=P).transpose(1, 2).reshape(B * (S // P) ** 2, Cc * P * P)
    par, out = parent(n, dtype)
    ops.patchify(x.to(dev()), out.view(want.shape), P, dtype)
    assert torch.equal(par.cpu(), expect(n, dtype, want))


def test_patchify_refusals_write_nothing():
    from uvc_amd import _lib as L
    x = rnd(2, 3, 12, 12, seed=1).to(dev())
    par, out = parent(x.numel(), F32)
    p, s = L.ptr, L.cur_stream()
    call = lambda xs, o, B, Cc, S, P: L.lib().uvc_patchify(xs, o, B, Cc, S, P, F32, s)
    refused(call(p(x), p(out), 2, 3, 12, 6), "P % 4 != 0")
    refused(call(p(x), p(out), 2, 3, 10, 4), "S % P != 0")
    refused(call(p(x), p(out), 0, 3, 12, 4), "B = 0")
    refused(call(p(x), p(out), 2, 0, 12, 4), "C = 0")
    refused(call(p(x), p(out), 2, 3, 12, 0), "P = 0")
    refused(call(0, p(out), 2, 3, 12, 4), "null x")
    refused(call(p(x), 0, 2, 3, 12, 4), "null out")
    torch.cuda.synchronize()
    assert bool((par == SENT).all())


# ============================================================================= uvc_cast_transpose
CT_EDGES = [1, 31, 32, 33, 64, 65]
CT_SHAPES = [(R, Cc) for R in CT_EDGES for Cc in CT_EDGES] + [(192, 576)]


@pytest.mark.parametrize("which", ["w", "wt", "both"])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_cast_transpose_every_tile_edge(dtype, which):
    """Odd leads (3 and 5 elements): the kernel stores element by element and may not assume more than the element's own alignment."""
    from uvc_amd import ops
    for R, Cc in CT_SHAPES:
        W = rnd(R, Cc, seed=1000 * R + Cc)
        n = R * Cc
        pw, w = parent(n, dtype, lead=3)
        pt, wt = parent(n, dtype, lead=5)
        ops.cast_transpose(W.to(dev()), R, Cc, w if which != "wt" else None, wt if which != "w" else None, dtype)
        want_w = expect(n, dtype, W, lead=3) if which != "wt" else torch.full_like(pw, SENT).cpu()
        want_t = expect(n, dtype, W.t().contiguous(), lead=5) if which != "w" else torch.full_like(pt, SENT).cpu()
        assert torch.equal(pw.cpu(), want_w), (R, Cc, "w")
        assert torch.equal(pt.cpu(), want_t), (R, Cc, "wt")


def test_cast_transpose_refusals_write_nothing():
    from uvc_amd import _lib as L
    W = rnd(8, 8, seed=2).to(dev())
    par, out = parent(64, F32)
    p, s = L.ptr, L.cur_stream()
    refused(L.lib().uvc_cast_transpose(p(W), 0, 8, p(out), 0, F32, s), "R = 0")
    refused(L.lib().uvc_cast_transpose(p(W), 8, 0, p(out), 0, F32, s), "C = 0")
    refused(L.lib().uvc_cast_transpose(0, 8, 8, p(out), 0, F32, s), "null W")
    refused(L.lib().uvc_cast_transpose(p(W), 8, 8, 0, 0, F32, s), "no output")
    torch.cuda.synchronize()
    assert bool((par == SENT).all())


# ============================================================================= uvc_cast_transpose_multi
class Table:
    """A table of matrices for uvc_cast_transpose_multi.  add() places a matrix at the next source offset congruent to ``src_mod`` mod 4 and its two
    shadows at the next shadow offsets congruent to ``w_mod`` / ``wt_mod`` mod 4 (None: -1, no such shadow), with sentinel gaps between them."""

    def __init__(self):
        self.mats, self.srcs, self.ws, self.wts, self.n_src, self.n_sh = [], [], [], [], 4, 4

    @staticmethod
    def _place(at, mod):
        return at + (mod - at) % 4

    def add(self, W, src_mod=0, w_mod=0, wt_mod=0):
        n = W.numel()
        s = self._place(self.n_src, src_mod)
        self.n_src = s + n + 4
        self.mats.append(W); self.srcs.append(s)
        for mod, offs in ((w_mod, self.ws), (wt_mod, self.wts)):
            if mod is None:
                offs.append(-1)
            else:
                o = self._place(self.n_sh, mod)
                offs.append(o)
                self.n_sh = o + n + 4
        return len(self.mats) - 1

    def vector_path(self, i):
        R, Cc = self.mats[i].shape
        return R % 4 == 0 and Cc % 4 == 0 and (self.srcs[i] | max(self.ws[i], 0) | max(self.wts[i], 0)) % 4 == 0

    def call(self, dtype, n=None):
        from uvc_amd import _lib as L
        n = len(self.mats) if n is None else n
        params = torch.full((self.n_src + 4,), float("nan"))
        for W, s in zip(self.mats, self.srcs):
            params[s:s + W.numel()] = W.reshape(-1)
        shadow = torch.full((self.n_sh + 4,), SENT, device=dev(), dtype=tt(dtype))
        m = max(len(self.mats), 1)
        a64 = lambda v: (C.c_int64 * m)(*v)
        a32 = lambda v: (C.c_int32 * m)(*v)
        pd = params.to(dev())
        rc = L.lib().uvc_cast_transpose_multi(L.ptr(pd), L.ptr(shadow), n, a64(self.srcs), a32([W.shape[0] for W in self.mats]),
                                              a32([W.shape[1] for W in self.mats]), a64(self.ws), a64(self.wts), dtype, L.cur_stream())
        torch.cuda.synchronize()
        return rc, shadow.cpu()

    def expected(self, dtype):
        sh = torch.full((self.n_sh + 4,), SENT, dtype=tt(dtype))
        for W, w, wt in zip(self.mats, self.ws, self.wts):
            if w >= 0:
                sh[w:w + W.numel()] = W.reshape(-1).to(tt(dtype))
            if wt >= 0:
                sh[wt:wt + W.numel()] = W.t().contiguous().reshape(-1).to(tt(dtype))
        return sh

    def shadows(self, sh, i):
        n = self.mats[i].numel()
        return [None if o < 0 else sh[o:o + n] for o in (self.ws[i], self.wts[i])]


VEC_EDGES = [4, 60, 64, 68, 128]
VEC_SHAPES = [(R, Cc) for R in VEC_EDGES for Cc in VEC_EDGES]
RAGGED = [(1, 1), (1, 64), (64, 1), (1, 128), (37, 37), (37, 64), (64, 37), (63, 65), (65, 63), (63, 63), (65, 65), (4, 65), (65, 4), (63, 4), (128, 37)]


def matrix(i, R, Cc):
    return rnd(R, Cc, seed=7000 + 131 * i + R * 7 + Cc)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_cast_transpose_multi_vector_and_scalar_paths_agree(dtype):
    """The same 25 matrices four times: everything aligned (the vector path), the source one element off, the plain shadow one element off, the
    transposed shadow three elements off (the scalar path each time).  Every table equals torch, so the two paths give the same bits."""
    tables = {}
    for name, mods in (("vector", (0, 0, 0)), ("odd source", (1, 0, 0)), ("odd w", (0, 1, 0)), ("odd wt", (0, 0, 3))):
        t = Table()
        for i, (R, Cc) in enumerate(VEC_SHAPES):
            t.add(matrix(i, R, Cc), *mods)
        assert all(t.vector_path(i) == (name == "vector") for i in range(len(VEC_SHAPES))), name
        rc, sh = t.call(dtype)
        assert rc == 0
        assert torch.equal(sh, t.expected(dtype)), name
        tables[name] = (t, sh)
    tv, shv = tables["vector"]
    for name in ("odd source", "odd w", "odd wt"):
        ts, shs = tables[name]
        for i in range(len(VEC_SHAPES)):
            for a, b in zip(tv.shadows(shv, i), ts.shadows(shs, i)):
                assert torch.equal(a.view(torch.int16 if dtype == BF16 else torch.int32), b.view(torch.int16 if dtype == BF16 else torch.int32)), (name, i)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_cast_transpose_multi_ragged_shapes_and_skipped_shadows(dtype):
    """R or C of 1, 37, 63, 65 (the scalar path whatever the offsets), mixed in one table with vector-path matrices, and entries with w = -1 or
    wt = -1 on both paths."""
    t = Table()
    for i, (R, Cc) in enumerate(RAGGED):
        t.add(matrix(i, R, Cc), 0, None if i % 5 == 1 else 0, None if i % 5 == 3 else 0)
    for i, (R, Cc) in enumerate([(64, 64), (68, 60), (4, 4), (128, 64)]):
        t.add(matrix(50 + i, R, Cc), 0, None if i % 2 else 0, 0 if i % 2 else None)
    assert sum(t.vector_path(i) for i in range(len(t.mats))) == 4 and t.ws.count(-1) >= 4 and t.wts.count(-1) >= 4
    rc, sh = t.call(dtype)
    assert rc == 0
    assert torch.equal(sh, t.expected(dtype))


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_cast_transpose_multi_one_entry_and_a_full_table(dtype):
    """n = 1 (one tile; nine tiles), and n = 64: the ballot lookup compares against all 64 tile offsets.  The full table mixes one-tile matrices
    with two- and four-tile ones, so the tile offsets are not the entry numbers, and both paths."""
    for R, Cc in ((64, 64), (5, 3), (132, 140)):
        t = Table()
        t.add(matrix(90, R, Cc))
        rc, sh = t.call(dtype)
        assert rc == 0 and torch.equal(sh, t.expected(dtype)), (R, Cc)
    shapes = [(4, 4), (8, 4), (5, 3), (64, 68), (1, 7), (12, 16), (65, 65), (16, 4)]
    t = Table()
    for i in range(64):
        R, Cc = shapes[i % len(shapes)]
        t.add(matrix(100 + i, R, Cc), 0 if i % 3 else 1, None if i % 7 == 2 else 0, None if i % 7 == 5 else 0)
    assert len(t.mats) == 64 and 0 < sum(t.vector_path(i) for i in range(64)) < 64
    rc, sh = t.call(dtype)
    assert rc == 0
    assert torch.equal(sh, t.expected(dtype))
    last = Table()                                   # the 64th entry alone gives the same bits as inside the table
    last.add(t.mats[63])
    rc, sh1 = last.call(dtype)
    assert rc == 0
    for a, b in zip(t.shadows(sh, 63), last.shadows(sh1, 0)):
        assert a is None or torch.equal(a, b)


def test_cast_transpose_multi_refusals_write_nothing():
    t = Table()
    for i in range(65):
        t.add(matrix(200 + i, 4, 4))
    for n in (0, 65, -1):
        rc, sh = t.call(F32, n=n)
        refused(rc, f"n = {n}")
        assert bool((sh == SENT).all()), n


# ============================================================================= uvc_mixup_batch
def f32(v):
    return float(np.float32(v))


BELOW_ONE = float(np.nextafter(np.float32(1), np.float32(0)))
LAMS = [0.0, 1.0, f32(0.3), BELOW_ONE]


def mixup_call(x, lam, oml, cutmix=0, box=(0, 0, 0, 0)):
    from uvc_amd import _lib as L
    B, Cc, H, W = x.shape
    yl, yh, xl, xh = box
    rc = L.lib().uvc_mixup_batch(L.ptr(x), B, Cc, H, W, lam, oml, cutmix, yl, yh, xl, xh, L.cur_stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("B", [2, 6])
def test_mixup_batch_is_three_separately_rounded_operations(B, lam):
    """x * lam + x.flip(0) * (1 - lam) in float32 on the host, product by product: the kernel may not contract either product into the sum.
    One vector per image (1 x 2 x 2), and 3 x 32 x 32 (several workgroups)."""
    oml = f32(1.0 - lam)
    for Cc, H, W in ((1, 2, 2), (3, 8, 8), (3, 32, 32)):
        x = rnd(B, Cc, H, W, seed=300 + B + H)
        x[0, 0, 0, 0], x[B - 1, 0, 0, 0] = 1e30, -3e-39          # a huge value and a subnormal in one pair
        want = x * torch.tensor(lam, dtype=torch.float32) + x.flip(0) * torch.tensor(oml, dtype=torch.float32)
        par, xd = parent(x.numel(), F32)
        xd.copy_(x.reshape(-1))
        assert mixup_call(xd.view(x.shape), lam, oml) == 0
        assert torch.equal(par.cpu().view(torch.int32), expect(x.numel(), F32, want).view(torch.int32)), (Cc, H, W)
        if lam == 1.0:
            assert torch.equal(want.view(torch.int32)[x != 0], x.view(torch.int32)[x != 0])


@pytest.mark.parametrize("B", [2, 6])
def test_cutmix_boxes(B):
    """The box is swapped inside each pair and nothing else moves: an empty box (both ways), one pixel in each corner, a row, a column, the full frame."""
    Cc, H, W = 3, 10, 12
    boxes = [(0, 0, 0, 0), (3, 3, 2, 9), (2, 7, 5, 5), (H, H, W, W), (0, 1, 0, 1), (0, 1, W - 1, W), (H - 1, H, 0, 1), (H - 1, H, W - 1, W),
             (4, 5, 0, W), (0, H, 7, 8), (2, 9, 1, 11), (0, H, 0, W)]
    x = rnd(B, Cc, H, W, seed=400 + B)
    for yl, yh, xl, xh in boxes:
        want = x.clone()
        want[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
        par, xd = parent(x.numel(), F32, lead=3)                  # the box path stores single floats: no alignment to keep
        xd.copy_(x.reshape(-1))
        assert mixup_call(xd.view(x.shape), 1.0, 0.0, 1, (yl, yh, xl, xh)) == 0
        assert torch.equal(par.cpu(), expect(x.numel(), F32, want, lead=3)), (yl, yh, xl, xh)
        if (yh - yl) * (xh - xl) == 0:
            assert torch.equal(want, x)
    assert torch.equal(want, x.flip(0))                           # the full frame


def test_mixup_batch_refusals_write_nothing():
    x = rnd(4, 3, 6, 6, seed=5)
    par, xd = parent(x.numel(), F32)
    xd.copy_(x.reshape(-1))
    v = xd.view(x.shape)
    refused(mixup_call(v[:3], 0.3, 0.7), "odd B")
    refused(mixup_call(v[:3], 1.0, 0.0, 1, (0, 2, 0, 2)), "odd B, CutMix")
    refused(mixup_call(xd[:4 * 3 * 3 * 5].view(4, 3, 3, 5), 0.3, 0.7), "CHW % 4 != 0")
    refused(mixup_call(par[GUARD + 1:GUARD + 1 + 2 * 3 * 4 * 4].view(2, 3, 4, 4), 0.3, 0.7), "not 16-byte aligned")
    for box in ((0, 7, 0, 2), (0, 2, 0, 7), (-1, 2, 0, 2), (0, 2, -1, 2), (3, 2, 0, 2), (0, 2, 3, 2)):
        refused(mixup_call(v, 1.0, 0.0, 1, box), f"box {box}")
    from uvc_amd import _lib as L
    refused(L.lib().uvc_mixup_batch(0, 4, 3, 6, 6, 0.3, 0.7, 0, 0, 0, 0, 0, L.cur_stream()), "null x")
    refused(L.lib().uvc_mixup_batch(L.ptr(xd), 0, 3, 6, 6, 0.3, 0.7, 0, 0, 0, 0, 0, L.cur_stream()), "B = 0")
    torch.cuda.synchronize()
    assert torch.equal(par.cpu(), expect(x.numel(), F32, x))
    assert mixup_call(xd[:4 * 3 * 3 * 5].view(4, 3, 3, 5), 1.0, 0.0, 1, (0, 3, 0, 5)) == 0     # CutMix has no size condition


# ============================================================================= uvc_mixup_target
@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("Cn", [1, 10, 1000])
def test_mixup_target(Cn, lam):
    """y = onehot_smooth(t) * lam + onehot_smooth(t.flip(0)) * (1 - lam), products rounded separately; equal and unequal label pairs, odd B (the
    middle image pairs with itself), B * C on both sides of a workgroup."""
    from uvc_amd import _lib as L
    oml = f32(1.0 - lam)
    off = f32(0.1 / Cn)
    on = f32(1.0 - 0.1 + 0.1 / Cn)
    for B in (1, 2, 3, 5, 6):
        gen = torch.Generator().manual_seed(500 + B + Cn)
        t = torch.randint(0, Cn, (B,), generator=gen)
        if B >= 2:
            t[B - 1] = t[0]                                       # an equal pair
        if B >= 5 and Cn > 1:
            t[1], t[B - 2] = 0, Cn - 1                            # an unequal pair on the first and the last class
        oh = lambda lab: torch.full((B, Cn), off).scatter_(1, lab.view(-1, 1), on)
        want = oh(t) * torch.tensor(lam, dtype=torch.float32) + oh(t.flip(0)) * torch.tensor(oml, dtype=torch.float32)
        par, y = parent(B * Cn, F32, lead=1)
        td = t.to(dev())
        rc = L.lib().uvc_mixup_target(L.ptr(td), L.ptr(y), B, Cn, lam, oml, on, off, L.cur_stream())
        torch.cuda.synchronize()
        assert rc == 0
        assert torch.equal(par.cpu().view(torch.int32), expect(B * Cn, F32, want, lead=1).view(torch.int32)), B


def test_mixup_target_refusals_write_nothing():
    from uvc_amd import _lib as L
    t = torch.zeros(4, dtype=torch.int64, device=dev())
    par, y = parent(40, F32)
    s = L.cur_stream()
    refused(L.lib().uvc_mixup_target(L.ptr(t), L.ptr(y), 0, 10, 0.3, 0.7, 0.9, 0.01, s), "B = 0")
    refused(L.lib().uvc_mixup_target(L.ptr(t), L.ptr(y), 4, 0, 0.3, 0.7, 0.9, 0.01, s), "C = 0")
    refused(L.lib().uvc_mixup_target(0, L.ptr(y), 4, 10, 0.3, 0.7, 0.9, 0.01, s), "null labels")
    refused(L.lib().uvc_mixup_target(L.ptr(t), 0, 4, 10, 0.3, 0.7, 0.9, 0.01, s), "null y")
    torch.cuda.synchronize()
    assert bool((par == SENT).all())
