"""GPU: the row-panel NT GEMM (k_gemm_nt_rows: M <= 1024 rows, 16 rows x 64 columns per workgroup, a wave's fragments of 512 elements of K requested
at once) against the generic 128 x 128 kernel on the same operands.

The specification is equality of bits: the same k-ordered MFMA chain (2 * ceil(K / 64) steps, zero-padded past K) and the same staged epilogue.  Checked
for every row count around the 16-row panel (1, 15, 16, 17) and at 512 / 1024, the widths of the step's turnaround (192 / 768 / 1000 on either side),
every epilogue the route takes, A and C in bf16 and float32, a device alpha and the gate pair, row strides of two rows, and a repeated launch; M = 1025
and float32 compute stay on the old route (asked of the predicate).  One case per epilogue is also held against float64 at the tolerance
tests/test_kernels_gpu.py uses for uvc_gemm_nt in bf16 (2^-9 relative rounding per operand, float32 accumulation: rtol = atol = 2e-2)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
MS = (1, 15, 16, 17, 512, 1024)
SHAPES = [(192, 192), (768, 192), (192, 768), (1000, 192), (192, 1000)]            # (N, K)
EPIS = ["none", "bias", "bias_resid", "bias_resid_gate", "bias_gelu_grad", "mul_aux"]
MAXM = 1024


def _epi(name):
    from uvc_amd import ops
    from uvc_amd import _lib as L
    return dict(none=ops.EPI_NONE, bias=ops.EPI_BIAS, bias_resid=ops.EPI_BIAS_RESID, bias_resid_gate=ops.EPI_BIAS_RESID_GATE,
                bias_gelu_grad=L.EPI_BIAS_GELU_GRAD, mul_aux=L.EPI_MUL_AUX)[name]


@functools.lru_cache(maxsize=None)
def _operands(N, K, ld_mul=1):
    """One set of operands per width (MAXM rows; a case takes the first M), never modified.  ld_mul = 2: rows twice as long as the problem's."""
    g = torch.Generator().manual_seed(1000 * N + K + ld_mul)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).cuda()
    o = dict(A=r(MAXM, K * ld_mul), W=r(N, K, scale=0.05).to(torch.bfloat16), bias=r(N), R=r(MAXM, N * ld_mul), R2=r(MAXM, N * ld_mul),
             aux=r(MAXM, N * ld_mul).to(torch.bfloat16), gate=torch.tensor([0.3, 0.7]).cuda(), alpha=torch.tensor([0.6]).cuda())
    o["A16"] = o["A"].to(torch.bfloat16)
    o["R16"], o["R216"] = o["R"].to(torch.bfloat16), o["R2"].to(torch.bfloat16)
    return o


def _run(o, name, M, N, K, a_f32, c_f32, with_alpha, generic, ld_mul=1):
    from uvc_amd import ops
    cdt = torch.float32 if c_f32 else torch.bfloat16
    C1 = torch.full((M, N * ld_mul), -7.0, device="cuda", dtype=cdt)
    C2 = torch.full((M, N * ld_mul), -7.0, device="cuda", dtype=cdt) if name == "bias_gelu_grad" else None
    kw = dict(dtype=BF16, epilogue=_epi(name), M=M, N=N, K=K, lda=K * ld_mul, ldc=N * ld_mul, force_generic=generic)
    if name != "none" and name != "mul_aux":
        kw["bias"] = o["bias"]
    if name in ("bias_resid", "bias_resid_gate"):
        kw["R"] = (o["R"] if c_f32 else o["R16"])[:M]
    if name == "bias_resid_gate":
        kw["R2"] = (o["R2"] if c_f32 else o["R216"])[:M]
        kw["gate"] = o["gate"]
    if name == "mul_aux":
        kw["aux"] = o["aux"][:M]
    if name == "bias_gelu_grad":
        kw["C2"] = C2
    if with_alpha:
        kw["alpha_ptr"] = o["alpha"]
    ops.gemm_nt((o["A"] if a_f32 else o["A16"])[:M], o["W"], C1, **kw)
    return C1, C2


def _supported(M, N, K, dtype, name, lda=None, ldc=None):
    from uvc_amd import _lib as L
    return L.lib().uvc_gemm_nt_rows_supported(M, N, K, lda or K, K, ldc or N, dtype, _epi(name))


@pytest.mark.parametrize("name", EPIS)
@pytest.mark.parametrize("N,K", SHAPES)
def test_row_panel_kernel_equals_the_generic_kernel_bit_for_bit(N, K, name):
    o = _operands(N, K)
    for M in MS:
        assert _supported(M, N, K, BF16, name) == 1
        for a_f32 in (False, True):
            for c_f32 in (False, True):
                for with_alpha in (False, True):
                    new = _run(o, name, M, N, K, a_f32, c_f32, with_alpha, False)
                    old = _run(o, name, M, N, K, a_f32, c_f32, with_alpha, True)
                    for x, y in zip(new, old):
                        if x is not None:
                            assert torch.isfinite(x.float()).all() and float(x.float().abs().max()) > 0
                            assert torch.equal(x, y), (M, N, K, name, a_f32, c_f32, with_alpha)


@pytest.mark.parametrize("name", EPIS)
def test_row_strides_of_two_rows_alpha_and_the_gate_pair(name):
    """The head's calls pass lda = ntok * D (two token rows per image): A, C and the epilogue's operands on rows twice as long as the problem's; the other half of
    every C row stays as it was."""
    for N, K in ((192, 192), (1000, 192), (192, 1000)):
        o = _operands(N, K, 2)
        for M in (17, 512):
            assert _supported(M, N, K, BF16, name, lda=2 * K, ldc=2 * N) == 1
            for a_f32, c_f32 in ((False, False), (True, False), (False, True), (True, True)):
                new = _run(o, name, M, N, K, a_f32, c_f32, True, False, ld_mul=2)
                old = _run(o, name, M, N, K, a_f32, c_f32, True, True, ld_mul=2)
                for x, y in zip(new, old):
                    if x is not None:
                        assert torch.equal(x, y), (M, N, K, name, a_f32, c_f32)
                        assert bool((x[:, N:] == -7.0).all()) and bool((x[:, :N] != -7.0).any())


def test_a_repeated_launch_is_bit_identical_and_other_problems_keep_their_route():
    N, K = 768, 192
    o = _operands(N, K)
    a = _run(o, "bias_gelu_grad", 512, N, K, False, False, False, False)
    b = _run(o, "bias_gelu_grad", 512, N, K, False, False, False, False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # asked of the predicate: more than 1024 rows and float32 compute are not taken
    assert _supported(1024, N, K, BF16, "bias") == 1
    assert _supported(1025, N, K, BF16, "bias") == 0
    assert _supported(512, N, K, F32, "bias") == 0


@pytest.mark.parametrize("name", EPIS)
def test_row_panel_kernel_against_float64(name):
    M, N, K = 512, 192, 768
    o = _operands(N, K)
    t = dict(rtol=2e-2, atol=2e-2)
    Cc, C2 = _run(o, name, M, N, K, False, True, True, False)
    assert _supported(M, N, K, BF16, name) == 1
    A, W = o["A16"][:M].double(), o["W"].double()
    acc = 0.6 * (A @ W.t())
    lin = acc + o["bias"].double()
    if name == "none":
        ref = acc
    elif name == "bias":
        ref = lin
    elif name == "bias_resid":
        ref = lin + o["R"][:M].double()
    elif name == "bias_resid_gate":
        ref = 0.7 * (lin + o["R"][:M].double()) + 0.3 * o["R2"][:M].double()
    elif name == "mul_aux":
        ref = acc * o["aux"][:M].double()
    else:
        xl = lin.clone().requires_grad_(True)
        F.gelu(xl).sum().backward()
        ref = xl.grad
        torch.testing.assert_close(C2.double(), F.gelu(lin), **t)
    torch.testing.assert_close(Cc.double(), ref, **t)
