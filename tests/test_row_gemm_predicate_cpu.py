"""CPU: uvc_gemm_nt_rows_supported on both sides of each of its bounds (no GPU call).

uvc_gemm_nt asks this predicate which problems go to the row-panel kernel (k_gemm_nt_rows): bf16 compute, 1 <= M <= 1024, 8 <= K <= 1024 in whole
16-byte chunks, N a multiple of 8, leading dimensions that cover the problem in multiples of 8, and one of six epilogues.  The kernel requests a
wave's fragments of 512 elements of K at once, in at most two halves: K above 1024 must stay with the tiled kernels; so must float32 compute."""
import pytest

F32, BF16 = 0, 1
NONE, BIAS, BIAS_GELU, BIAS_RESID, BIAS_RESID_GATE, DGELU, BIAS_GELU_OUT, BIAS_GELU_GRAD, MUL_AUX, GELU_GRAD_Q8, MUL_AUX_Q8 = range(11)
TAKEN = (NONE, BIAS, BIAS_RESID, BIAS_RESID_GATE, BIAS_GELU_GRAD, MUL_AUX)


@pytest.fixture(scope="module")
def sup():
    from uvc_amd import _lib as L
    from uvc_amd import build
    build.build()
    assert (L.EPI_NONE, L.EPI_BIAS, L.EPI_BIAS_RESID, L.EPI_BIAS_RESID_GATE, L.EPI_BIAS_GELU_GRAD, L.EPI_MUL_AUX) == TAKEN
    fn = L.lib().uvc_gemm_nt_rows_supported
    return lambda M, N, K, lda=None, ldb=None, ldc=None, dtype=BF16, epi=BIAS: fn(M, N, K, K if lda is None else lda, K if ldb is None else ldb,
                                                                                  N if ldc is None else ldc, dtype, epi)


def test_row_bounds(sup):
    assert sup(0, 192, 192) == 0
    assert sup(1, 192, 192) == 1
    assert sup(1024, 192, 192) == 1
    assert sup(1025, 192, 192) == 0
    assert sup(2**31 - 1, 192, 192) == 0


def test_k_bounds(sup):
    assert sup(512, 192, 0) == 0
    assert sup(512, 192, 8) == 1
    assert sup(512, 192, 1000) == 1
    assert sup(512, 192, 1024) == 1
    assert sup(512, 192, 1032) == 0
    assert sup(512, 192, 196) == 0            # not whole 16-byte chunks
    assert sup(512, 192, 3072) == 0


def test_n_is_a_multiple_of_eight(sup):
    assert sup(512, 0, 192) == 0
    assert sup(512, 8, 192) == 1
    assert sup(512, 1000, 192) == 1
    assert sup(512, 1004, 192) == 0
    assert sup(512, 3072, 192) == 1           # no upper bound on N: more workgroups


def test_leading_dimensions(sup):
    assert sup(512, 192, 192, lda=384, ldc=384) == 1        # the heads' rows: two token rows per image
    assert sup(512, 192, 192, lda=196) == 0
    assert sup(512, 192, 192, ldb=196) == 0
    assert sup(512, 192, 192, ldc=196) == 0
    assert sup(512, 192, 192, lda=184) == 0                 # shorter than the problem's rows
    assert sup(512, 192, 192, ldb=184) == 0
    assert sup(512, 192, 192, ldc=184) == 0


def test_compute_type_and_epilogues(sup):
    assert sup(512, 192, 768, dtype=F32) == 0
    assert sup(512, 192, 768, dtype=2) == 0
    for e in range(-1, 12):
        assert sup(512, 192, 768, epi=e) == (1 if e in TAKEN else 0), e
