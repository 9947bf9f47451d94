"""CPU: the exported shape predicates on both sides of their operand-size bounds (no GPU call).

The fused LayerNorm forms run kernels that address A through 32-bit buffer offsets ("32-bit buffer offsets").  A
predicate must never promise more than its call accepts: the engine asks the predicate, and a "yes" above the bound made the call
fail with UVC_ERR_UNSUPPORTED (uvc_gemm_nt with ln_out at N = 384).  These values are pinned here."""
import pytest

F32, BF16 = 0, 1
EPI_BIAS_RESID, EPI_BIAS_RESID_GATE = 3, 4


@pytest.fixture(scope="module")
def lib():
    from uvc_amd import _lib as L
    from uvc_amd import build
    build.build()
    assert (L.EPI_BIAS_RESID, L.EPI_BIAS_RESID_GATE) == (EPI_BIAS_RESID, EPI_BIAS_RESID_GATE)
    return L.lib()


@pytest.mark.parametrize("K", [384, 1152, 1536])
@pytest.mark.parametrize("epi", [EPI_BIAS_RESID, EPI_BIAS_RESID_GATE])
def test_gemm_nt_ln_supported_n384_row_bound(lib, K, epi):
    # k_gemm_row384_lnbwd<.., 1> requests the ragged tile's rows up to M + 128: (M + 128) * K * 2 < 2^31
    top = (1 << 31) // (2 * K) - 128                      # the first M with (M + 128) * K * 2 >= 2^31 ...
    if (top + 128) * K * 2 < (1 << 31):
        top += 1
    assert (top + 127) * K * 2 < (1 << 31) <= (top + 128) * K * 2
    assert lib.uvc_gemm_nt_ln_supported(top - 1, 384, K, BF16, epi) == 1
    assert lib.uvc_gemm_nt_ln_supported(top, 384, K, BF16, epi) == 0
    assert lib.uvc_gemm_nt_ln_supported(2**31 - 1, 384, K, BF16, epi) == 0
    assert lib.uvc_gemm_nt_ln_supported(4096, 384, K, BF16, epi) == 1
    assert lib.uvc_gemm_nt_ln_supported(4095, 384, K, BF16, epi) == 0


def test_gemm_nt_ln_supported_small_fc2_values(lib):
    # DeiT-Small fc2 + residual (+ gate) -> norm1: the issue's row counts, 698 922 / 698 923 at K = 1536
    assert lib.uvc_gemm_nt_ln_supported(698922, 384, 1536, BF16, EPI_BIAS_RESID_GATE) == 1
    assert lib.uvc_gemm_nt_ln_supported(698923, 384, 1536, BF16, EPI_BIAS_RESID_GATE) == 0
    assert lib.uvc_gemm_nt_ln_supported(698923, 384, 1536, F32, EPI_BIAS_RESID_GATE) == 0


def test_gemm_nt_ln_supported_n192_has_no_row_bound(lib):
    # N = 192: the streaming kernels address with 64-bit offsets -- any row count from 16 up (whether norm is fused must not depend on the batch)
    for M in (16, 4096, 1398102, 2796250, 2**31 - 1):
        assert lib.uvc_gemm_nt_ln_supported(M, 192, 768, BF16, EPI_BIAS_RESID_GATE) == 1
        assert lib.uvc_gemm_nt_ln_supported(M, 192, 192, BF16, EPI_BIAS_RESID) == 1
    assert lib.uvc_gemm_nt_ln_supported(15, 192, 768, BF16, EPI_BIAS_RESID) == 0


@pytest.mark.parametrize("K", [384, 1152, 1536])
def test_gemm_lnbwd_supported_d384_bound(lib, K):
    # k_gemm_row384_lnbwd (backward): M * K < 2^30, i.e. A below 2^31 bytes
    top = ((1 << 30) - 1) // K                            # the largest M with M * K < 2^30
    assert top * K < (1 << 30) <= (top + 1) * K
    assert lib.uvc_gemm_lnbwd_supported(top, 384, K, BF16) == 1
    assert lib.uvc_gemm_lnbwd_supported(top + 1, 384, K, BF16) == 0
    assert lib.uvc_gemm_lnbwd_supported(4096, 384, K, BF16) == 1
    assert lib.uvc_gemm_lnbwd_supported(4095, 384, K, BF16) == 0


def test_gemm_lnbwd_supported_d192_has_no_row_bound(lib):
    for M in (4096, 1398102, 2796250, 2**31 - 1):
        assert lib.uvc_gemm_lnbwd_supported(M, 192, 768, BF16) == 1
        assert lib.uvc_gemm_lnbwd_supported(M, 192, 576, BF16) == 1
    assert lib.uvc_gemm_lnbwd_supported(4096, 192, 512, BF16) == 0
    assert lib.uvc_gemm_lnbwd_supported(4096, 192, 768, F32) == 0
