"""CPU: which kernel uvc_gemm_nt / uvc_gemm_tn select, on both sides of every bound of the rules (no GPU call).

uvc_gemm_nt_route / uvc_gemm_tn_route are the functions the entry points themselves call before they launch (nt_route in gemm.hip, tn_route in gemm_tn.hip).  They never
dereference a pointer, so the operands here are fake addresses: non-null, distinct, 16-byte aligned.  Every expectation below is read from the rule
as DESIGN.md ("GEMM routing") and include/uvc_kernels.h state it, not from a run of the code; tests/golden/gemm_route_pins.json is what the commit
before the route functions launched on an MI355X (tools/gemm_route_pins.py under rocprofv3 --kernel-trace)."""
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = 0, 1
NONE, BIAS, BIAS_GELU, BIAS_RESID, BIAS_RESID_GATE, DGELU, BIAS_GELU_OUT, BIAS_GELU_GRAD, MUL_AUX, GELU_GRAD_Q8, MUL_AUX_Q8 = range(11)
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 3          # uvc_amd/csrc/common.h
NT_PTRS = ("A", "B", "C", "C2", "bias", "R", "R2", "aux", "gate")
LN_PTRS = ("ln_gamma", "ln_beta", "ln_out", "ln_mean", "ln_rstd")
PTR = 0x7F0000000000


@pytest.fixture(scope="module")
def ops():
    from uvc_amd import build, ops
    build.build()
    return ops


def nt_fields(M, N, K, epi=BIAS, fg=0, a_f32=0, c_f32=0, dtype=BF16, ln=0, **kw):
    f = dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N, dtype=dtype, a_is_f32=a_f32, c_is_f32=c_f32, epilogue=epi, force_generic=fg, alpha=1.0,
             r_is_f32=int(bool(c_f32 or dtype == F32)))
    for i, n in enumerate(NT_PTRS + (LN_PTRS if ln else ())):
        f[n] = PTR + 0x10000000 * i
    f.update(kw)
    return f


def tn_fields(M, N1, N2, variant=0, a_f32=0, dtype=BF16, **kw):
    f = dict(M=M, N1=N1, N2=N2, lda=N1, ldb=N2, ldc=N2, dtype=dtype, a_is_f32=a_f32, variant=variant, A=PTR, B=PTR + 0x10000000, C=PTR + 0x20000000,
             workspace=PTR + 0x30000000, workspace_bytes=2**62, alpha=1.0)
    f.update(kw)
    return f


@pytest.fixture(scope="module")
def nt(ops):
    def route(*a, rc=OK, **kw):
        got, r = ops.gemm_nt_route(**nt_fields(*a, **kw))
        assert got == rc, (a, kw, got, r)
        return r
    return route


@pytest.fixture(scope="module")
def tn(ops):
    def route(*a, rc=OK, **kw):
        got, r = ops.gemm_tn_route(**tn_fields(*a, **kw))
        assert got == rc, (a, kw, got, r)
        return r
    return route


def has(r, family, **args):
    assert r["family"] == family, r
    for k, v in args.items():
        assert r[k] == v, (k, v, r)
    return True


# ---------------------------------------------------------------------------------------------------- NT, bf16
def test_streaming_families_start_at_4096_rows(nt):
    """K = 192 / 128 with N % 64 == 0, K = 384 with N % 192 == 0, N = 192 with K in {768, 576, 512, 256}: M >= 4096.  One row fewer is the generic
    kernel (none of these shapes is wide enough for the 256-column kernels: K < 256, N < 256, or too few tiles with N % 256 != 0)."""
    assert has(nt(4096, 768, 192), "WS", kt=6, nw=4, nj=4, a_f32=0, c_f32=0, epilogue=BIAS)       # N % 256 == 0: four waves
    assert has(nt(4096, 320, 192), "WS", kt=6, nw=3, nj=4)                                         # N % 64 == 0 only: three
    assert has(nt(4096, 256, 128, c_f32=1), "WS", kt=4, nw=4, c_f32=1)
    assert has(nt(4096, 328, 192), "NT")                                                           # N % 64 != 0
    for N, K in ((768, 192), (320, 192), (256, 128)):
        assert has(nt(4095, N, K), "NT")
    assert has(nt(4096, 384, 384), "WS384", kt=12, nw=6, nj=2)
    assert has(nt(4095, 384, 384), "NT")
    assert has(nt(4096, 320, 384), "NT")                                                           # N % 192 != 0
    for K in (768, 576, 512, 256):
        assert has(nt(4096, 192, K), "WSN", kt=K // 32)
        assert has(nt(4095, 192, K), "NT")
    assert has(nt(4096, 192, 640), "NT")                                                           # a K the column-sliced kernel is not built for
    # the backward's multiplying epilogues at K = 192, N % 256 == 0, bf16 A and C: eight waves x 32 columns
    for e in (DGELU, MUL_AUX, MUL_AUX_Q8):
        assert has(nt(4096, 768, 192, epi=e), "WS", kt=6, nw=8, nj=2)
    assert has(nt(4096, 768, 192, epi=MUL_AUX, c_f32=1), "WS", nw=4, nj=4)
    assert has(nt(4096, 320, 192, epi=MUL_AUX), "WS", nw=3, nj=4)
    assert has(nt(4096, 768, 192, epi=GELU_GRAD_Q8), "WS", kt=6, nw=4, nj=4)


def test_row_panels_up_to_1024_rows_and_k_1024(nt, ops):
    """uvc_gemm_nt_rows_supported: M <= 1024, K <= 1024.  Below those bounds the row panels take the shapes of every streaming family (whose own row
    bound, 4096, lies above) and of the wide kernels; force_generic != 0 skips them."""
    shapes = ((768, 192), (384, 384), (192, 768), (192, 192), (768, 768), (2560, 256))
    for N, K in shapes:
        assert has(nt(1024, N, K), "NT_ROWS", a_f32=0, c_f32=0, epilogue=BIAS)
        assert nt(1025, N, K)["family"] != "NT_ROWS"
        assert ops.gemm_nt_rows_supported(1024, N, K, BF16, BIAS) and not ops.gemm_nt_rows_supported(1025, N, K, BF16, BIAS)
    assert has(nt(1025, 768, 192), "NT") and has(nt(1025, 384, 384), "NT") and has(nt(1025, 192, 768), "NT") and has(nt(1025, 768, 768), "NT")
    assert has(nt(512, 192, 1024), "NT_ROWS")
    assert has(nt(512, 192, 1032), "NT")
    assert has(nt(512, 192, 192, a_f32=1, c_f32=1), "NT_ROWS", a_f32=1, c_f32=1)
    for fg in (1, 2, 3, 4, 5):
        assert has(nt(512, 192, 192, fg=fg), "NT")
    assert has(nt(512, 192, 192, epi=BIAS_GELU), "NT")                                              # an epilogue the row panels do not take
    assert has(nt(512, 192, 192, dtype=F32, a_f32=1, c_f32=1), "NT", t_f32=1)
    assert has(nt(512, 192, 192, epi=BIAS_RESID, ldr=196), "NT")                                    # ldr % 8 != 0


def test_k192_n192_residual_ring(nt):
    """attn.proj + residual (K = N = 192, BIAS_RESID, M >= 4096, M % 16 == 0) runs the seven-stage LDS-DMA ring; M % 16 != 0 falls through to the
    K = 192 streaming kernel (N = 192 is not a multiple of 256: three waves)."""
    for c_f32 in (0, 1):
        assert has(nt(4096, 192, 192, epi=BIAS_RESID, c_f32=c_f32), "WSN16_DMA", kt=6, ln=0, nst=7, c_f32=c_f32, epilogue=BIAS_RESID)
        assert has(nt(4112 - 8, 192, 192, epi=BIAS_RESID, c_f32=c_f32), "WS", kt=6, nw=3, nj=4)
    assert has(nt(4080, 192, 192, epi=BIAS_RESID), "NT")                                            # M % 16 == 0 below 4096: neither
    assert has(nt(4096, 192, 192, epi=BIAS), "WS")                                                  # another epilogue
    assert has(nt(4096, 192, 192, epi=BIAS_RESID, a_f32=1), "WS", a_f32=1)
    assert has(nt(4096, 192, 192, epi=BIAS_RESID, alpha=0.5), "WS")
    assert has(nt(4096, 192, 192, epi=BIAS_RESID, A=PTR + 8), "WS")                                 # the ring's operands are 16-byte aligned
    for fg in (2, 3, 4, 5):
        assert has(nt(4096, 192, 192, epi=BIAS_RESID, fg=fg), "WS")
    assert has(nt(4096, 192, 192, epi=BIAS_RESID, fg=1), "NT")


def test_k384_six_or_eight_waves(nt):
    """K = 384: eight waves x 32 columns where C is bf16 and N is a multiple of 128 from 512 up, six waves x 32 otherwise; force_generic = 5 keeps six.
    With N % 192 == 0 the first N past 384 that qualifies is 768.  N = 512 itself is no multiple of 192: not this family at all, but few wide tiles
    (N % 256 == 0, M >= 2048) of the 8-phase kernel -- at 4096 x 512 the four heights cost 1 round x (ri + 8): ri = 4."""
    assert has(nt(4096, 384, 384), "WS384", nw=6)
    assert has(nt(4096, 576, 384), "WS384", nw=6)                                                   # >= 512, not a multiple of 128
    assert has(nt(4096, 768, 384), "WS384", nw=8, kt=12, nj=2)
    assert has(nt(4096, 768, 384, fg=5), "WS384", nw=6)
    assert has(nt(4096, 384, 384, fg=5), "WS384", nw=6)
    assert has(nt(4096, 768, 384, c_f32=1), "WS384", nw=6, c_f32=1)
    assert has(nt(4096, 512, 384), "NT8P", ri=4)
    assert has(nt(4096, 384, 384, epi=NONE), "NT")                                                  # the plain epilogue: eight-wave form only
    assert has(nt(4096, 768, 384, epi=NONE), "WS384", nw=8)
    assert has(nt(4096, 384, 384, epi=DGELU), "NT")


def test_n192_16_or_32_rows_and_dma_or_registers(nt):
    """N = 192: 32-row tiles (k_gemm_wsn) for bf16 C without residual, 16-row tiles for float32 C and the residual epilogues; those on the LDS-DMA ring
    at K = 768 (K = 512 / 256 with ln_out only, K = 576 never) unless force_generic = 2, A / R / R2 are not 16-byte aligned or M % 16 != 0."""
    for e in (NONE, BIAS):
        assert has(nt(4096, 192, 768, epi=e), "WSN", kt=24, c_f32=0)
        assert has(nt(4096, 192, 768, epi=e, c_f32=1), "WSN16", kt=24, c_f32=1)
    for e in (BIAS_RESID, BIAS_RESID_GATE):
        for c_f32 in (0, 1):
            assert has(nt(4096, 192, 768, epi=e, c_f32=c_f32), "WSN16_DMA", kt=24, ln=0, nst=3, c_f32=c_f32, epilogue=e)
            assert has(nt(4096, 192, 768, epi=e, c_f32=c_f32, fg=2), "WSN16", kt=24)
            assert has(nt(4096, 192, 768, epi=e, c_f32=c_f32, A=PTR + 8), "WSN16", kt=24)
            assert has(nt(4096, 192, 768, epi=e, c_f32=c_f32, R=PTR + 0x50000008), "WSN16", kt=24)
            assert has(nt(4104, 192, 768, epi=e, c_f32=c_f32), "WSN16", kt=24)
            for K in (576, 512, 256):
                assert has(nt(4096, 192, K, epi=e, c_f32=c_f32), "WSN16", kt=K // 32)
    # ln_out: always the ring (force_generic = 2 included), every row count from 16 up
    for K, nst in ((768, 3), (512, 3), (256, 4)):
        for fg in (0, 2):
            assert has(nt(4096, 192, K, epi=BIAS_RESID_GATE, ln=1, fg=fg), "WSN16_DMA", kt=K // 32, ln=1, nst=nst)
        assert has(nt(24, 192, K, epi=BIAS_RESID, ln=1, c_f32=1), "WSN16_DMA", kt=K // 32, ln=1, nst=nst, c_f32=1)
    assert has(nt(4096, 192, 192, epi=BIAS_RESID, ln=1), "WSN16_DMA", kt=6, ln=1, nst=7)
    assert has(nt(4096, 384, 384, epi=BIAS_RESID, ln=1), "ROW384")
    nt(4095, 384, 384, epi=BIAS_RESID, ln=1, rc=ERR_UNSUPPORTED)
    nt(4096, 192, 576, epi=BIAS_RESID, ln=1, rc=ERR_UNSUPPORTED)
    nt(15, 192, 768, epi=BIAS_RESID, ln=1, rc=ERR_UNSUPPORTED)
    nt(4096, 192, 768, epi=BIAS_RESID, ln=1, A=PTR + 8, rc=ERR_UNSUPPORTED)
    nt(4096, 192, 768, epi=BIAS, ln=1, rc=ERR_UNSUPPORTED)
    nt(4104, 192, 768, epi=BIAS_RESID, ln=1, R=PTR + 0x20000000, rc=ERR_ARG)                        # M % 16 != 0 and C aliases R
    nt(4096, 192, 768, epi=BIAS_RESID, ln=1, ln_gamma=0, rc=ERR_ARG)


def test_wide_kernels_256x256_8phase_or_generic(nt):
    """K >= 256 (K % 64 == 0) against N >= 256.  >= 640 tiles of 256 x 256 and M >= 2048: k_gemm_nt256.  Otherwise bf16 C with N % 256 == 0 and
    M >= 2048: k_gemm_nt8p.  Otherwise generic.  force_generic = 3 / 4 drop the size bounds (3 keeps N < 1792 with N % 256 == 0 on the 8-phase kernel)."""
    # the 640-tile rule: N = 2560 is 10 tile columns; 63 / 64 tile rows = 630 / 640 tiles
    assert has(nt(63 * 256, 2560, 256), "NT8P")
    assert has(nt(63 * 256 + 1, 2560, 256), "NT256", c_f32=0)
    assert has(nt(63 * 256 + 1, 2560, 256, c_f32=1), "NT256", c_f32=1)
    # N = 1000 is 4 tile columns and no multiple of 256: 159 / 160 tile rows = 636 / 640 tiles
    assert has(nt(159 * 256, 1000, 256), "NT")
    assert has(nt(159 * 256 + 1, 1000, 256), "NT256")
    # M = 2047 / 2048 at 640 tiles (8 x 80) and at few wide tiles
    assert has(nt(2048, 80 * 256, 256), "NT256")
    assert has(nt(2047, 80 * 256, 256), "NT")
    assert has(nt(2048, 768, 768), "NT8P")
    assert has(nt(2047, 768, 768), "NT")
    assert has(nt(2048, 768, 768, c_f32=1), "NT")                                                   # the 8-phase kernel by shape: bf16 C only
    assert has(nt(2048, 768, 768, a_f32=1), "NT", a_f32=1)
    assert has(nt(2048, 768, 320 - 64), "NT8P") and has(nt(2048, 768, 320 - 72), "NT")              # K = 256 | K = 248 (K % 64 != 0)
    # force_generic = 3: N = 1536 / 1792
    assert has(nt(1100, 1536, 768, fg=3), "NT8P")
    assert has(nt(1100, 1792, 768, fg=3), "NT256")
    assert has(nt(1100, 1536, 768, fg=3, c_f32=1), "NT256", c_f32=1)
    assert has(nt(1100, 1000, 768, fg=3), "NT256")
    assert has(nt(1100, 1536, 768, fg=4), "NT256")
    assert has(nt(1100, 1536, 768, fg=0), "NT") and has(nt(1100, 1536, 768, fg=5), "NT")
    for fg in (1, 2):
        assert has(nt(63 * 256 + 1, 2560, 256, fg=fg), "NT") and has(nt(2048, 768, 768, fg=fg), "NT")
    # tile heights: 0x100 | ri; 0 (and by shape) the height with the fewest rounds x (ri + 8): 25 216 x 768 is 2 / 2 / 2 / 3 rounds for ri 8 / 6 / 5 / 4
    for ri in (8, 6, 5, 4):
        assert has(nt(97, 512, 320, fg=0x100 | ri), "NT8P", ri=ri)
        assert has(nt(97, 512, 320, fg=0x100 | ri, c_f32=1), "NT8P", ri=8, c_f32=1)
    assert has(nt(25216, 768, 768), "NT8P", ri=5)
    assert has(nt(25216, 768, 768, fg=0x100), "NT8P", ri=5)
    assert has(nt(97, 512, 320, fg=0x107), "NT8P", ri=4)                                           # a height not built: the 128-row tile
    # the streaming families come before the forced 8-phase kernel
    assert has(nt(4096, 768, 384, fg=0x108), "WS384")


def test_force_generic_on_shapes_it_cannot_take(nt):
    """Status of every force_generic value where its kernel does not exist: 1 with ln_out or a one-byte epilogue and 0x100 | ri off the 8-phase
    kernel's shapes are UVC_ERR_UNSUPPORTED; 2, 3, 4, 5 fall back to the generic kernel."""
    nt(4096, 192, 768, epi=BIAS_RESID, ln=1, fg=1, rc=ERR_UNSUPPORTED)
    nt(4096, 384, 384, epi=BIAS_RESID, ln=1, fg=1, rc=ERR_UNSUPPORTED)
    nt(4096, 768, 192, epi=GELU_GRAD_Q8, fg=1, rc=ERR_UNSUPPORTED)
    nt(4096, 768, 192, epi=MUL_AUX_Q8, fg=1, rc=ERR_UNSUPPORTED)
    for fg in (0x100, 0x104, 0x108):
        nt(4096, 768, 192, fg=fg, rc=ERR_UNSUPPORTED)                                               # K < 256
        nt(512, 192, 1024, fg=fg, rc=ERR_UNSUPPORTED)                                               # N < 256
        nt(512, 512, 264, fg=fg, rc=ERR_UNSUPPORTED)                                                # K % 64 != 0
        nt(512, 512, 256, fg=fg, a_f32=1, rc=ERR_UNSUPPORTED)
        nt(512, 512, 256, fg=fg, A=PTR + 8, rc=ERR_UNSUPPORTED)
        nt(4096, 768, 192, epi=GELU_GRAD_Q8, fg=fg, rc=ERR_UNSUPPORTED)
    for fg in (2, 3, 4, 5):
        assert has(nt(1100, 200, 72, fg=fg), "NT")
        assert has(nt(512, 512, 256, fg=fg, a_f32=1), "NT", a_f32=1)
    assert has(nt(1100, 200, 72, fg=1), "NT")
    # the one-byte epilogues exist in the K = 192 streaming kernel only
    nt(4095, 768, 192, epi=GELU_GRAD_Q8, rc=ERR_UNSUPPORTED)
    nt(4096, 768, 192, epi=GELU_GRAD_Q8, c_f32=1, rc=ERR_UNSUPPORTED)
    nt(4096, 768, 192, epi=MUL_AUX_Q8, ldr=196, rc=ERR_UNSUPPORTED)
    # argument checks keep their status
    nt(4096, 768, 192, A=0, rc=ERR_ARG)
    nt(0, 768, 192, rc=ERR_ARG)
    nt(4096, 768, 196, rc=ERR_ARG)
    nt(4096, 768, 192, bias=0, rc=ERR_ARG)
    nt(4096, 768, 192, epi=BIAS_RESID, r_is_f32=1, rc=ERR_ARG)
    nt(4096, 768, 192, dtype=2, rc=ERR_ARG)
    nt(4096, 768, 192, dtype=F32, rc=ERR_ARG)
    for e in (-1, 11):
        for shape in ((4096, 768, 192), (4096, 768, 384), (1100, 200, 72), (63 * 256 + 1, 2560, 256), (2048, 768, 768)):
            nt(*shape, epi=e, rc=ERR_ARG)


# ---------------------------------------------------------------------------------------------------- TN
def tn_cfg_rule(N1, N2):
    """uvc_gemm_tn's tile configuration for bf16 operands, as DESIGN.md states it."""
    if N1 % 256 == 0 and N2 % 256 == 0 and (N1 // 256) * (N2 // 256) >= 9:
        return 5
    if N1 % 192 == 0 and N2 % 256 == 0:
        return 1
    if N1 % 256 == 0 and N2 % 192 == 0:
        return 2
    if N1 % 192 == 0 and N2 % 192 == 0 and (N1 // 192) * (N2 // 192) >= 2:
        return 3
    return 4 if (N1, N2) == (192, 192) else 0


TILES = {0: (128, 64), 1: (192, 256), 2: (256, 192), 3: (192, 192), 4: (96, 192), 5: (256, 256), 6: (128, 256)}


def tn_splits_rule(M, N1, N2, cfg):
    """The split rule: cfg 0 aims at 768 workgroups (rounded up), the big tiles at 256 (128 for at most four tiles; rounded down: one workgroup per
    CU), never more splits than 64-row blocks, and for the big tiles at least 1024 rows a split (2048 for 192 x 192 tiles below 32 768 rows) once
    M holds two such splits."""
    b1, b2 = TILES[cfg]
    if cfg == 0:
        splits = -(-768 // (-(-N1 // b1) * -(-N2 // b2)))
    else:
        tiles = (N1 // b1) * (N2 // b2)
        splits = (128 if tiles <= 4 else 256) // tiles
    splits = min(splits, -(-M // 64))
    rmin = 2048 if (cfg == 3 and M < 32768) else 1024
    if cfg != 0 and M >= 2 * rmin:
        splits = min(splits, M // rmin)
    return max(splits, 1)


def test_tn_cfg_by_shape(tn):
    for (N1, N2), cfg, fam in (((128, 64), 0, "TN"), ((200, 200), 0, "TN"), ((512, 512), 0, "TN"), ((192, 256), 1, "TN8P"), ((768, 512), 1, "TN8P"),
                               ((256, 192), 2, "TN8P"), ((768, 192), 2, "TN8P"), ((384, 192), 3, "TN8P"), ((192, 384), 3, "TN8P"), ((576, 192), 3, "TN8P"),
                               ((192, 192), 4, "TN_DMA"), ((768, 768), 5, "TN8P"), ((1024, 2304), 5, "TN8P")):
        assert tn_cfg_rule(N1, N2) == cfg
        assert has(tn(4096, N1, N2), fam, cfg=cfg, b1=TILES[cfg][0], b2=TILES[cfg][1])
    # the 9-tile threshold of the 256 x 256 tiles: 2 x 4 = 8 tiles stay generic (no 192-wide tile divides them), 3 x 3 = 9 take them
    assert has(tn(4096, 512, 1024), "TN", cfg=0)
    assert has(tn(4096, 768, 768), "TN8P", cfg=5)
    # float32 compute and leading dimensions that are no multiple of 8 bf16 elements... (bf16: chunks of 8 are an argument check)
    assert has(tn(4096, 192, 256, dtype=F32, a_f32=1), "TN", cfg=0, t_f32=1, a_f32=1)
    tn(4096, 192, 256, dtype=F32, rc=ERR_ARG)
    tn(4096, 192, 256, dtype=2, rc=ERR_ARG)
    tn(4096, 192, 256, lda=196, rc=ERR_ARG)
    tn(4096, 192, 256, workspace=0, rc=ERR_ARG)
    tn(0, 192, 256, rc=ERR_ARG)


def test_tn_float32_a_demotions(tn):
    """float32 A (converted on load) exists on the register-staged 192- / 256-wide tiles and the generic kernel: cfg 4 becomes 0, cfg 5 becomes 1 or 2
    where 192 divides one side, else 0."""
    assert has(tn(4096, 192, 192, a_f32=1), "TN", cfg=0, a_f32=1, t_f32=0)
    assert has(tn(4096, 768, 768, a_f32=1), "TN_BIG", cfg=1, b1=192, b2=256)
    assert has(tn(4096, 1024, 768, a_f32=1), "TN_BIG", cfg=2, b1=256, b2=192)
    assert has(tn(4096, 1024, 1024, a_f32=1), "TN", cfg=0)
    for (N1, N2), cfg in (((192, 256), 1), ((256, 192), 2), ((384, 192), 3)):
        assert has(tn(4096, N1, N2, a_f32=1), "TN_BIG", cfg=cfg)
        assert has(tn(4096, N1, N2, a_f32=1, variant=2), "TN_BIG", cfg=cfg)


def test_tn_variants(tn):
    """variant 0 == 1: by shape.  2: the ring kernel for cfgs 1, 2, 3 (cfg 4 has no other; cfg 5 has no ring form).  3: 128 x 256 tiles where the shape
    takes 256 x 256, nothing else changes."""
    for (N1, N2), cfg in (((192, 256), 1), ((256, 192), 2), ((384, 192), 3), ((192, 192), 4), ((768, 768), 5), ((128, 64), 0)):
        r0 = tn(4096, N1, N2, variant=0)
        assert tn(4096, N1, N2, variant=1) == r0
        r2, r3 = tn(4096, N1, N2, variant=2), tn(4096, N1, N2, variant=3)
        assert r2 == (dict(r0, family="TN_DMA", kernel="k_gemm_tn_dma") if cfg in (1, 2, 3) else r0)
        if cfg == 5:
            assert has(r3, "TN8P", cfg=6, b1=128, b2=256)
        else:
            assert r3 == r0
    # twice the tiles, half the splits: 9 tiles of 256 x 256 at 100 864 rows take 256 // 9 = 28 splits, 18 tiles of 128 x 256 take 14
    assert has(tn(100864, 768, 768), "TN8P", cfg=5, splits=28) and has(tn(100864, 768, 768, variant=3), "TN8P", cfg=6, splits=14)


def test_tn_two_gigabyte_bound(tn):
    """k_gemm_tn8p's 32-bit offsets: (M + 256) * max(lda, ldb) * 2 < 2^31.  With leading dimensions in whole 16-byte chunks that product is a multiple
    of 16, so the last value below the bound is 2^31 - 16 = 262 657 * 4088 * 2 (2^27 - 1 = 7 * 73 * 262 657), and 2^31 = 262 144 * 4096 * 2 -- reached
    with a long row, not many rows, so the splits stay what the small problem has.  Past the bound cfgs 1, 2, 3 keep their tiles on the ring kernel
    (64-bit offsets) and the 256 x 256 tiles go to the generic kernel."""
    below, at = dict(M=262657 - 256, ld=4088), dict(M=262144 - 256, ld=4096)
    assert (below["M"] + 256) * below["ld"] * 2 == 2**31 - 16 and (at["M"] + 256) * at["ld"] * 2 == 2**31
    for (N1, N2), cfg in (((192, 256), 1), ((256, 192), 2), ((384, 192), 3), ((768, 768), 5)):
        for side in ("lda", "ldb"):
            assert has(tn(below["M"], N1, N2, **{side: below["ld"]}), "TN8P", cfg=cfg)
            r = tn(at["M"], N1, N2, **{side: at["ld"]})
            assert has(r, "TN", cfg=0) if cfg == 5 else has(r, "TN_DMA", cfg=cfg)
            assert r["splits"] <= 256
    assert has(tn(at["M"], 192, 192, lda=at["ld"]), "TN_DMA", cfg=4)                                # never on the 32-bit-offset kernel
    assert has(tn(at["M"], 768, 768, lda=at["ld"], variant=3), "TN", cfg=0)


DEIT_TINY_WGRADS = {           # (N1, N2) at M = 100 864 rows (512 images x 197 tokens) -> cfg, splits, rows per split, worked out from the rule:
    # 3 tiles of 192 x 192 <= 4: 128 // 3 = 42 splits (<= 1576 blocks of 64 rows; 100 864 // 1024 = 98 allows them); ceil(100 864 / 42) = 2402 rows,
    # rounded up to 64-row blocks 2432; ceil(100 864 / 2432) = 42
    (576, 192): (3, 42, 2432),        # dW_qkv
    (768, 192): (2, 42, 2432),        # dW_fc1: 3 tiles of 256 x 192, the same arithmetic
    (192, 768): (1, 42, 2432),        # dW_fc2: 3 tiles of 192 x 256
    # 2 tiles of 96 x 192: 128 // 2 = 64 splits (<= 98); 100 864 / 64 = 1576 rows -> 1600; ceil(100 864 / 1600) = 64
    (192, 192): (4, 64, 1600),        # dW_proj
}


def test_tn_splits_of_deit_tiny(tn):
    for (N1, N2), (cfg, splits, rps) in DEIT_TINY_WGRADS.items():
        assert has(tn(100864, N1, N2), "TN_DMA" if cfg == 4 else "TN8P", cfg=cfg, splits=splits, rows_per_split=rps)
        assert tn_splits_rule(100864, N1, N2, cfg) == splits
    # T2T-ViT-14's 192 x 192 tiles below 32 768 rows: >= 2048 rows a split (25 216 rows: 12 splits of 2112 rows, not 256 // 4 = 64)
    assert has(tn(25216, 384, 384), "TN8P", cfg=3, splits=12, rows_per_split=2112)
    assert has(tn(32768, 384, 384), "TN8P", cfg=3, splits=32, rows_per_split=1024)
    assert has(tn(100, 192, 256), "TN8P", cfg=1, splits=2, rows_per_split=64)                       # not more splits than 64-row blocks


def test_tn_workspace_is_the_larger_of_generic_and_shape_cfg(tn, ops):
    """uvc_gemm_tn_workspace_bytes holds the generic kernel's splits or the shape's configuration's, whichever are more (a float32 A or a long row
    sends a call to the generic kernel): splits * (N1 * N2 + N1) floats."""
    problems = [(100864, n1, n2) for n1, n2 in DEIT_TINY_WGRADS] + [(4096, n1, n2) for n1, n2 in ((128, 64), (192, 256), (256, 192), (384, 192), (192, 192),
                                                                                                   (768, 768), (512, 1024), (200, 200))]
    problems += [(25216, 384, 384), (100, 192, 256), (262144 - 256, 192, 256)]
    for M, N1, N2 in problems:
        s = max(tn_splits_rule(M, N1, N2, 0), tn_splits_rule(M, N1, N2, tn_cfg_rule(N1, N2)))
        assert ops.gemm_tn_workspace_bytes(M, N1, N2) == s * (N1 * N2 + N1) * 4, (M, N1, N2)
        for kw in ({}, dict(a_f32=1), dict(variant=2), dict(variant=3), dict(lda=8192 * 64)):
            r = tn(M, N1, N2, **kw)
            assert r["splits"] <= s and r["splits"] <= tn_splits_rule(M, N1, N2, r["cfg"])
            assert r["rows_per_split"] % 64 == 0 and (r["splits"] - 1) * r["rows_per_split"] < M <= r["splits"] * r["rows_per_split"]
        # the workspace check of the call is the same size
        tn(M, N1, N2, workspace_bytes=s * (N1 * N2 + N1) * 4)
        tn(M, N1, N2, workspace_bytes=s * (N1 * N2 + N1) * 4 - 1, rc=ERR_ARG)
    assert ops.gemm_tn_workspace_bytes(100864, 576, 192) == 52 * (576 * 192 + 576) * 4              # cfg 0: 5 x 3 tiles, ceil(768 / 15) = 52 > 42


# ---------------------------------------------------------------------------------------------------- every route
def test_route_kernel_names_are_kernel_templates_of_one_gemm_family_file(ops):
    """Every kernel template is defined in exactly one gemm*.hip (a kernel must not end up in two objects), in the file of its family; gemm.hip,
    the routing, defines no kernel at all."""
    import glob
    from uvc_amd import _lib as L
    defined = {}                                              # kernel template name -> the files that define it
    files = sorted(glob.glob(os.path.join(ROOT, "uvc_amd", "csrc", "gemm*.hip")))
    for path in files:
        text = open(path).read()
        if os.path.basename(path) == "gemm.hip":
            assert not re.search(r"__global__\s", text), "gemm.hip defines no __global__ function"
        for k in re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", text):
            defined.setdefault(k, []).append(os.path.basename(path))
    assert "gemm.hip" in [os.path.basename(p) for p in files] and len(files) > 1
    assert defined["k_gemm_nt"] == defined["k_gemm_nt_rows"] == ["gemm_nt_tiled.hip"] and defined["k_gemm_ws"] == ["gemm_nt_ws.hip"]
    assert not {k: fs for k, fs in defined.items() if len(fs) != 1}, "a kernel template is defined in exactly one file"
    assert {k: fs[0] for k, fs in defined.items()} == {
        "k_gemm_nt": "gemm_nt_tiled.hip", "k_gemm_nt_rows": "gemm_nt_tiled.hip",
        "k_gemm_ws": "gemm_nt_ws.hip",
        "k_gemm_wsn": "gemm_nt_wsn.hip", "k_gemm_wsn16": "gemm_nt_wsn.hip", "k_gemm_wsn16_dma": "gemm_nt_wsn.hip",
        "k_gemm_wsn_lnbwd": "gemm_nt_lnbwd.hip", "k_gemm_wsn_lnbwd_dma": "gemm_nt_lnbwd.hip",
        "k_gemm_nt256": "gemm_nt_wide.hip", "k_gemm_row384_lnbwd": "gemm_nt_wide.hip", "k_gemm_nt8p": "gemm_nt_wide.hip",
        "k_gemm_tn": "gemm_tn.hip", "k_gemm_tn_big": "gemm_tn.hip", "k_gemm_tn_dma": "gemm_tn.hip", "k_gemm_tn8p": "gemm_tn.hip", "k_tn_reduce": "gemm_tn.hip",
    }, "the whole kernel -> file map (the table at the top of gemm_common.h)"
    kernels = set(defined)
    assert len(L.ROUTE_FAMILIES) == 14
    for fam in range(len(L.ROUTE_FAMILIES)):
        name = L.lib().uvc_gemm_route_kernel(fam)
        assert name is not None and name.decode() in kernels, (fam, name)
    assert L.lib().uvc_gemm_route_kernel(-1) is None and L.lib().uvc_gemm_route_kernel(len(L.ROUTE_FAMILIES)) is None


def template_args(r):
    """The route as the template arguments of its kernel, spelled as a demangled kernel name spells them (bf16 is unsigned short)."""
    t = lambda f32: "float" if f32 else "unsigned short"
    b = lambda v: "true" if v else "false"
    fam, e = r["family"], r["epilogue"]
    return {
        "NT": lambda: [t(r["a_f32"]), t(r["t_f32"]), t(r["c_f32"]), e],
        "NT_ROWS": lambda: [t(r["a_f32"]), t(r["c_f32"]), e],
        "WS": lambda: [t(r["a_f32"]), t(r["c_f32"]), e, r["kt"], r["nw"], r["nj"]],
        "WS384": lambda: [t(0), t(r["c_f32"]), e, 12, r["nw"], 2],
        "WSN": lambda: [t(r["c_f32"]), e, r["kt"]],
        "WSN16": lambda: [t(r["c_f32"]), e, r["kt"]],
        "WSN16_DMA": lambda: [e, r["kt"], b(r["ln"]), r["nst"], b(not r["c_f32"])],
        "ROW384": lambda: ["true", 1],
        "NT256": lambda: [t(r["c_f32"]), e],
        "NT8P": lambda: [t(r["c_f32"]), e, r["ri"]],
        "TN": lambda: [t(r["a_f32"]), t(r["t_f32"])],
        "TN_BIG": lambda: ["float", r["b1"], r["b2"]] + ([4, 2] if r["cfg"] == 2 else [2, 4]),
        "TN_DMA": lambda: [r["b1"], r["b2"]] + ([4, 2] if r["cfg"] == 2 else [2, 4]),
        "TN8P": lambda: [r["b1"] // 32, r["b2"] // 64],
    }[fam]()


def test_routes_equal_what_the_parent_commit_launched(ops):
    """tests/golden/gemm_route_pins.json: the kernels an MI355X ran for tools/gemm_route_pins.py's problems at the commit before nt_route / tn_route
    existed (rocprofv3 --kernel-trace).  The route queries must name the same kernel with the same template arguments."""
    pins = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_route_pins.json")))
    assert len(pins) >= 60
    families = set()
    for p in pins:
        m = re.match(r"(\w+)<(.*)>$", p["kernel"])
        name, args = m.group(1), [a.strip() for a in m.group(2).split(",")]
        if p["call"] == "nt":
            rc, r = ops.gemm_nt_route(**nt_fields(p["M"], p["N"], p["K"], epi=p["epilogue"], fg=p["force_generic"], a_f32=p["a_is_f32"],
                                                  c_f32=p["c_is_f32"], dtype=p["dtype"], ln=p["ln_out"]))
        else:
            rc, r = ops.gemm_tn_route(**tn_fields(p["M"], p["N1"], p["N2"], variant=p["variant"], a_f32=p["a_is_f32"], dtype=p["dtype"]))
        assert rc == OK, p
        assert r["kernel"] == name, (p, r)
        want = [str(a) for a in template_args(r)]
        # (the epilogue prints as its enum value, with or without a cast, depending on the demangler)
        got = [re.sub(r"^\(\w+\)", "", a) for a in args]
        assert got == want, (p, r, got, want)
        families.add(r["family"])
    assert len(families) == 14
