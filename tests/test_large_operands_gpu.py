"""GPU: the kernels on operands just past 2^31 bytes (and 2^32 where stated), in the production layouts.

Four kernels address their operands through 32-bit buffer offsets and rely on host-side size guards ("32-bit buffer
offsets"): k_gemm_tn8p, k_gemm_nt256, k_gemm_nt8p and k_gemm_row384_lnbwd.  Each case here sizes one operand just below or just
past such a bound and checks the result against float64 computed from the same rounded operands:
  * row-independent outputs (NT GEMMs, attention, row kernels): the first rows, every row window whose bytes straddle a multiple of
    2^31 in any operand, the ragged last rows and 256 random rows, at the tolerance of the kernel's existing test;
  * weight gradients (a reduction over M): the whole [N1, N2] against float64 accumulated in row chunks on the device, at a bound that
    a reference missing ONE 64-row k-step fails (asserted in every case), and bit equality with the ring kernel (variant 2).
Operands are made on the device and freed before the next case (each case stays under ~12 GB)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
G31 = 1 << 31


def dev():
    return torch.device("cuda")


@pytest.fixture(autouse=True)
def _free_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def randn(*shape, seed, dtype=torch.bfloat16, scale=1.0):
    g = torch.Generator(device=dev()).manual_seed(seed)
    t = torch.empty(*shape, device=dev(), dtype=dtype)
    if scale == 1.0:
        return t.normal_(generator=g)
    return t.normal_(0.0, scale, generator=g)


def check_rows(M, row_bytes, seed=0, window=256):
    """Row indices to check: the first rows, a window around every row whose bytes cross a multiple of 2^31 in an operand with
    row_bytes bytes per row, the ragged last rows, and 256 random rows."""
    rows = set(range(min(M, window)))
    for rb in row_bytes:
        j = 1
        while j * G31 // rb < M:
            r = j * G31 // rb
            rows.update(range(max(0, r - window), min(M, r + window)))
            j += 1
    rows.update(range(max(0, M - window), M))
    g = torch.Generator().manual_seed(seed)
    rows.update(torch.randint(0, M, (256,), generator=g).tolist())
    return torch.tensor(sorted(rows), device=dev(), dtype=torch.long)


def crosses(M, row_bytes):
    return any(M * rb > G31 for rb in row_bytes)


# ------------------------------------------------------------------------------------------------------------------------------
#   TN (weight gradients): C[N1, N2] = A[M, N1]^T . B[M, N2], the column sums of A beside it
# ------------------------------------------------------------------------------------------------------------------------------
def tn_reference(A, B, chunk=1 << 17):
    """float64 A^T B and colsum(A), accumulated over row chunks on the device; also the contribution of the 64-row k-step that
    holds the row just past 2^31 bytes of the wider operand (or the middle one), for the sensitivity check."""
    M = A.shape[0]
    ref = torch.zeros(A.shape[1], B.shape[1], device=dev(), dtype=torch.float64)
    cs = torch.zeros(A.shape[1], device=dev(), dtype=torch.float64)
    for m0 in range(0, M, chunk):
        a = A[m0:m0 + chunk].double()
        ref += a.t() @ B[m0:m0 + chunk].double()
        cs += a.sum(0)
    wide = max(A.shape[1] * A.element_size(), B.shape[1] * B.element_size())
    r = G31 // wide if G31 // wide < M else M // 2
    k0 = r // 64 * 64
    step = A[k0:k0 + 64].double().t() @ B[k0:k0 + 64].double()
    return ref, cs, step


def tn_bound(M):
    # float32 accumulation of M products of unit-variance operands: split partials are random walks of ~M / splits float32 roundings
    # of numbers of size sqrt(rows), summed in a fixed order -- measured errors are below 1e-2 at M = 5.6 M.  2e-7 * M (0.28 at 1.4 M
    # rows, 1.1 at 5.6 M) is far above that and far below what one missing 64-row k-step changes (a sum of 64 unit products: sd 8).
    return 2e-7 * M


def run_tn(A, B, variant=0, dtype=BF16):
    from uvc_amd import ops
    M, N1, N2 = A.shape[0], A.shape[1], B.shape[1]
    ws = torch.empty(ops.gemm_tn_workspace_bytes(M, N1, N2) // 4, device=dev())
    C = torch.full((N1, N2), float("nan"), device=dev())
    cs = torch.full((N1,), float("nan"), device=dev())
    ops.gemm_tn(A, B, C, ws, dtype=dtype, colsum_out=cs, variant=variant)
    del ws
    return C, cs


def assert_tn_close(C, cs, ref, cs_ref, step, M, what):
    bound = tn_bound(M)
    err = float((C.double() - ref).abs().max())
    assert err <= bound, (what, "C", err, bound)
    cerr = float((cs.double() - cs_ref).abs().max())
    assert cerr <= bound, (what, "colsum", cerr, bound)
    # the bound is tight enough: the reference without one 64-row k-step fails it
    miss = float((C.double() - (ref - step)).abs().max())
    assert miss > bound, (what, "a reference missing one k-step passes the bound", miss, bound)


# Tiny (D = 192, hidden 768): rows just past 2^31 bytes of the wider operand; cfg 2 also just past 2^32 bytes
TN_CASES = [
    ("cfg1_dW2", 192, 768, G31 // (768 * 2) + 43),           # 1 398 144 rows: B = [M, 768] at 2^31 + 65 KB
    ("cfg2_dW1", 768, 192, G31 // (768 * 2) + 43),
    ("cfg2_dW1_4GB", 768, 192, 2 * G31 // (768 * 2) + 47),    # A past 2^32 bytes (4.3 GB)
    ("cfg3_dWqkv", 576, 192, G31 // (576 * 2) + 37),
    ("cfg4_dWproj", 192, 192, G31 // (192 * 2) + 29),
]


@pytest.mark.parametrize("name,N1,N2,M", TN_CASES, ids=[c[0] for c in TN_CASES])
def test_gemm_tn_past_2gb_matches_float64_and_the_ring_kernel(name, N1, N2, M):
    A = randn(M, N1, seed=11)
    B = randn(M, N2, seed=12)
    assert crosses(M, (N1 * 2, N2 * 2))
    ref, cs_ref, step = tn_reference(A, B)
    C0, cs0 = run_tn(A, B, variant=0)
    assert_tn_close(C0, cs0, ref, cs_ref, step, M, (name, "variant 0"))
    C2, cs2 = run_tn(A, B, variant=2)
    assert torch.equal(C0, C2) and torch.equal(cs0, cs2), (name, "default and ring kernel differ")


def test_gemm_tn_largest_rows_below_the_bound_take_the_two_group_kernel():
    """The largest M that still takes k_gemm_tn8p at dW2 of DeiT-Tiny: (M + 256) * 768 * 2 < 2^31 -- its largest offsets; correct and
    bit-identical to the ring kernel."""
    M = G31 // (768 * 2) - 256
    assert (M + 256) * 768 * 2 < G31 <= (M + 257) * 768 * 2
    A = randn(M, 192, seed=21)
    B = randn(M, 768, seed=22)
    ref, cs_ref, step = tn_reference(A, B)
    C0, cs0 = run_tn(A, B, variant=0)
    assert_tn_close(C0, cs0, ref, cs_ref, step, M, "below")
    C2, cs2 = run_tn(A, B, variant=2)
    assert torch.equal(C0, C2) and torch.equal(cs0, cs2)


@pytest.mark.parametrize("mode", ["bf16_v0", "bf16_v3", "f32A_bf16", "fp32"])
def test_gemm_tn_base_dw1_past_2gb(mode):
    """DeiT-Base dW1 (3072 x 768: the 256 x 256 tiles, cfg 5; variant 3: 128 x 256, cfg 6) with A = [M, 3072] just past 2^31 bytes:
    the generic kernel above the bound; float32 A in bf16 mode (the register-staged 192 x 256 kernel); float32 mode."""
    M = G31 // (3072 * 2) + 45                      # 349 570 rows
    if mode == "fp32":
        A, B = randn(M, 3072, seed=31, dtype=torch.float32), randn(M, 768, seed=32, dtype=torch.float32)
        dtype = F32
    elif mode == "f32A_bf16":
        A, B = randn(M, 3072, seed=31, dtype=torch.float32), randn(M, 768, seed=32)
        dtype = BF16
    else:
        A, B = randn(M, 3072, seed=31), randn(M, 768, seed=32)
        dtype = BF16
    Aeff = A.bfloat16() if mode == "f32A_bf16" else A
    ref, cs_ref, step = tn_reference(Aeff, B)
    if mode == "f32A_bf16":
        del Aeff
    C, cs = run_tn(A, B, variant=3 if mode == "bf16_v3" else 0, dtype=dtype)
    bound = tn_bound(M)
    err = float((C.double() - ref).abs().max())
    if mode == "fp32":
        # float32 operands: the float32 MFMA chain carries 2^-24 relative rounding per product against bf16's exact products
        bound = 4 * bound
    assert err <= bound, (mode, err, bound)
    assert float((cs.double() - cs_ref).abs().max()) <= bound           # (float32 A in bf16 mode: the sums of the bf16-rounded values)
    assert float((C.double() - (ref - step)).abs().max()) > bound, (mode, "tolerance too loose to see one k-step")


# ------------------------------------------------------------------------------------------------------------------------------
#   NT
# ------------------------------------------------------------------------------------------------------------------------------
def nt_rows_close(C, A, W, rows, bias=None, tol=2e-2):
    ref = A[rows].double() @ W.double().t()
    if bias is not None:
        ref = ref + bias.double()
    torch.testing.assert_close(C[rows].double(), ref, rtol=tol, atol=tol)
    return ref


@pytest.mark.parametrize("fg,M", [(4, G31 // (768 * 2)), (4, G31 // (768 * 2) + 1), (3, G31 // (768 * 2) - 256), (3, G31 // (768 * 2) - 255)],
                         ids=["nt256_below", "nt256_above", "nt8p_below", "nt8p_above"])
def test_gemm_nt_wide_kernels_at_their_bound(fg, M):
    """k_gemm_nt256 (force_generic = 4: at any size) takes M * 768 * 2 < 2^31; k_gemm_nt8p (force_generic = 3 with N = 768) takes
    (M + 256) * 768 * 2 < 2^31.  Just below, the kernel runs with its largest offsets; just above, the dispatcher falls back.  Either
    way the output is bit-identical to the generic kernel and within the bf16 tolerance of float64 on the checked rows."""
    from uvc_amd import _lib as L
    from uvc_amd import ops
    N = K = 768
    A = randn(M, K, seed=41, scale=0.5)
    W = randn(N, K, seed=42, scale=0.04)
    bias = randn(N, seed=43, dtype=torch.float32, scale=0.1)
    C = torch.full((M, N), float("nan"), device=dev(), dtype=torch.bfloat16)
    ops.gemm_nt(A, W, C, dtype=BF16, epilogue=ops.EPI_BIAS, bias=bias, force_generic=fg)
    rows = check_rows(M, (K * 2, N * 2))
    nt_rows_close(C, A, W, rows, bias)
    C1 = torch.full((M, N), float("nan"), device=dev(), dtype=torch.bfloat16)
    ops.gemm_nt(A, W, C1, dtype=BF16, epilogue=ops.EPI_BIAS, bias=bias, force_generic=1)
    assert torch.equal(C, C1)
    if fg == 3:
        # the tuning code 0x100 | ri asks for the 8-phase kernel itself: served below the bound, refused above it
        above = (M + 256) * K * 2 >= G31
        C.fill_(float("nan"))
        if above:
            with pytest.raises(L.UvcHipError):
                ops.gemm_nt(A, W, C, dtype=BF16, epilogue=ops.EPI_BIAS, bias=bias, force_generic=0x100 | 5)
        else:
            ops.gemm_nt(A, W, C, dtype=BF16, epilogue=ops.EPI_BIAS, bias=bias, force_generic=0x100 | 5)
            assert torch.equal(C, C1)


def test_gemm_nt_fc1_gelu_grad_outputs_past_2gb():
    """fc1 of DeiT-Tiny (K = 192 -> N = 768) in the training form with C = GELU'(a) and C2 = GELU(a) past 2^31 bytes; the one-byte
    code form (C2 bit-identical, code within a step of the float64 GELU'); then the backward partners MUL_AUX / MUL_AUX_Q8 with aux past
    2^31 bytes."""
    from uvc_amd import ops
    K, N = 192, 768
    M = G31 // (N * 2) + 43
    A = randn(M, K, seed=51)
    W = randn(N, K, seed=52, scale=0.09)
    bias = randn(N, seed=53, dtype=torch.float32, scale=0.3)
    g16 = torch.empty(M, N, device=dev(), dtype=torch.bfloat16)
    u16 = torch.empty(M, N, device=dev(), dtype=torch.bfloat16)
    ops.gemm_nt(A, W, g16, dtype=BF16, epilogue=ops.EPI_BIAS_GELU_GRAD, bias=bias, C2=u16)
    rows = check_rows(M, (N * 2,))
    a64 = A[rows].double() @ W.double().t() + bias.double()
    xl = a64.clone().requires_grad_(True)
    F.gelu(xl).sum().backward()
    torch.testing.assert_close(g16[rows].double(), xl.grad, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(u16[rows].double(), F.gelu(a64), rtol=2e-2, atol=2e-2)
    assert ops.gemm_nt_q8_supported(M, N, K, BF16)
    q = torch.full((M, N), 77, device=dev(), dtype=torch.uint8)
    u8 = torch.empty(M, N, device=dev(), dtype=torch.bfloat16)
    ops.gemm_nt(A, W, q, dtype=BF16, epilogue=ops.EPI_BIAS_GELU_GRAD_Q8, bias=bias, C2=u8)
    assert torch.equal(u8, u16)
    del u8, u16
    dec = q[rows].double() * ops.Q8_STEP + ops.Q8_LO
    assert float((dec - xl.grad).abs().max()) <= ops.Q8_STEP / 2 + 2e-4
    # backward partner: dA = (alpha * G . W2t^T) * GELU'(a), G = [M, 192], aux = g16 / q
    G = randn(M, K, seed=54)
    W2t = randn(N, K, seed=55, scale=0.05)
    alpha = torch.tensor([0.6], device=dev())
    dA = torch.empty(M, N, device=dev(), dtype=torch.bfloat16)
    ops.gemm_nt(G, W2t, dA, dtype=BF16, epilogue=ops.EPI_MUL_AUX, aux=g16, alpha_ptr=alpha)
    acc = 0.6 * (G[rows].double() @ W2t.double().t())
    torch.testing.assert_close(dA[rows].double(), acc * g16[rows].double(), rtol=2e-2, atol=2e-2)
    ops.gemm_nt(G, W2t, dA, dtype=BF16, epilogue=ops.EPI_MUL_AUX_Q8, aux=q, alpha_ptr=alpha)
    torch.testing.assert_close(dA[rows].double(), acc * dec, rtol=2 ** -8, atol=1e-6)


@pytest.mark.parametrize("ln", [False, True])
def test_gemm_nt_fc2_residual_gate_past_2gb(ln):
    """fc2 of DeiT-Tiny (K = 768 -> N = 192) with residual and gate: A = [M, 768] just past 2^31 bytes, M % 16 == 0 (the LDS-DMA ring);
    with ln_out the next block's norm1 from the same launch, bit-identical to the unfused pair."""
    from uvc_amd import _lib as L
    from uvc_amd import ops
    K, N = 768, 192
    M = (G31 // (K * 2) + 16) // 16 * 16
    A = randn(M, K, seed=61, scale=0.5)
    W = randn(N, K, seed=62, scale=0.03)
    bias = randn(N, seed=63, dtype=torch.float32, scale=0.1)
    R, R2 = randn(M, N, seed=64), randn(M, N, seed=65)
    gate = torch.tensor([0.25, 0.75], device=dev())
    kw = dict(dtype=BF16, epilogue=ops.EPI_BIAS_RESID_GATE, bias=bias, R=R, R2=R2, gate=gate)
    C = torch.full((M, N), float("nan"), device=dev(), dtype=torch.bfloat16)
    gm = 1 + 0.1 * randn(N, seed=66, dtype=torch.float32)
    bt = 0.1 * randn(N, seed=67, dtype=torch.float32)
    if ln:
        assert L.lib().uvc_gemm_nt_ln_supported(M, N, K, BF16, ops.EPI_BIAS_RESID_GATE) == 1
        h = torch.full((M, N), float("nan"), device=dev(), dtype=torch.bfloat16)
        mu, rs = torch.empty(M, device=dev()), torch.empty(M, device=dev())
        ops.gemm_nt(A, W, C, ln_gamma=gm, ln_beta=bt, ln_out=h, ln_mean=mu, ln_rstd=rs, **kw)
    else:
        ops.gemm_nt(A, W, C, **kw)
    rows = check_rows(M, (K * 2,))
    ref = 0.75 * (A[rows].double() @ W.double().t() + bias.double() + R[rows].double()) + 0.25 * R2[rows].double()
    torch.testing.assert_close(C[rows].double(), ref, rtol=2e-2, atol=2e-2)
    C0 = torch.empty_like(C)
    ops.gemm_nt(A, W, C0, force_generic=1, **kw)
    torch.testing.assert_close(C.float(), C0.float(), rtol=1e-2, atol=1e-2)
    if ln:
        # the contract of test_fc2_residual_epilogue_writes_the_next_blocks_norm1: LayerNorm of the rounded C rows against float64, and
        # against uvc_layernorm_fwd on C (statistics to float32 rounding, rows within one bf16 step in < 2 % of the elements)
        ref_h = F.layer_norm(C[rows].double(), (N,), gm.double(), bt.double(), 1e-6)
        torch.testing.assert_close(h[rows].double(), ref_h, rtol=8e-3, atol=8e-3)
        h0 = torch.empty_like(C)
        m0, r0 = torch.empty(M, device=dev()), torch.empty(M, device=dev())
        ops.layernorm_fwd(C, gm, bt, h0, m0, r0, M, N, BF16)
        torch.testing.assert_close(mu, m0, rtol=2e-6, atol=1e-6)
        torch.testing.assert_close(rs, r0, rtol=2e-6, atol=0)
        diff = (h.float() - h0.float()).abs()
        assert float(diff.max()) <= 2.0 ** -7 * float(h0.float().abs().max()) + 1e-6
        assert float((diff > 0).float().mean()) < 0.02


@pytest.mark.parametrize("side", ["below", "above"])
def test_gemm_nt_row384_ln_out_at_its_bound(side):
    """fc2 of DeiT-Small (K = 1536 -> N = 384) with ln_out: k_gemm_row384_lnbwd<.., 1> takes (M + 128) * K * 2 < 2^31.  Where
    uvc_gemm_nt_ln_supported says yes the call succeeds and equals the unfused pair bit for bit; above the bound the predicate says no
    and the call refuses (the engine runs the unfused pair)."""
    from uvc_amd import _lib as L
    from uvc_amd import ops
    K, N = 1536, 384
    M = G31 // (K * 2) - 128 + (0 if side == "below" else 1)        # 698 922 / 698 923
    assert ((M + 128) * K * 2 < G31) == (side == "below")
    A = randn(M, K, seed=71, scale=0.5)
    W = randn(N, K, seed=72, scale=0.04)
    bias = randn(N, seed=73, dtype=torch.float32, scale=0.1)
    R = randn(M, N, seed=74)
    gm = 1 + 0.1 * randn(N, seed=75, dtype=torch.float32)
    bt = 0.1 * randn(N, seed=76, dtype=torch.float32)
    kw = dict(dtype=BF16, epilogue=ops.EPI_BIAS_RESID, bias=bias, R=R)
    C0 = torch.empty(M, N, device=dev(), dtype=torch.bfloat16)
    ops.gemm_nt(A, W, C0, force_generic=1, **kw)
    rows = check_rows(M, (K * 2,))
    torch.testing.assert_close(C0[rows].double(), A[rows].double() @ W.double().t() + bias.double() + R[rows].double(), rtol=2e-2, atol=2e-2)
    h0 = torch.empty_like(C0)
    m0, r0 = torch.empty(M, device=dev()), torch.empty(M, device=dev())
    ops.layernorm_fwd(C0, gm, bt, h0, m0, r0, M, N, BF16)
    supported = L.lib().uvc_gemm_nt_ln_supported(M, N, K, BF16, ops.EPI_BIAS_RESID)
    assert supported == (1 if side == "below" else 0)
    C1 = torch.full((M, N), float("nan"), device=dev(), dtype=torch.bfloat16)
    h1 = torch.full((M, N), float("nan"), device=dev(), dtype=torch.bfloat16)
    m1, r1 = torch.empty(M, device=dev()), torch.empty(M, device=dev())
    if supported:
        ops.gemm_nt(A, W, C1, ln_gamma=gm, ln_beta=bt, ln_out=h1, ln_mean=m1, ln_rstd=r1, **kw)
        assert torch.equal(C1, C0) and torch.equal(h1, h0) and torch.equal(m1, m0) and torch.equal(r1, r0)
    else:
        with pytest.raises(L.UvcHipError):
            ops.gemm_nt(A, W, C1, ln_gamma=gm, ln_beta=bt, ln_out=h1, ln_mean=m1, ln_rstd=r1, **kw)


# ------------------------------------------------------------------------------------------------------------------------------
#   dgrad + LayerNorm backward
# ------------------------------------------------------------------------------------------------------------------------------
def lnbwd_case(M, D, K, seed):
    from uvc_amd import ops
    A = randn(M, K, seed=seed)
    Wt = randn(D, K, seed=seed + 1, scale=0.05)
    x = randn(M, D, seed=seed + 2, dtype=torch.float32, scale=1.5) + 0.3
    gamma = 1.0 + 0.2 * randn(D, seed=seed + 3, dtype=torch.float32)
    add1 = randn(M, D, seed=seed + 4)
    a1 = torch.tensor([0.7], device=dev())
    mean = x.mean(1)
    rstd = torch.rsqrt(x.var(1, unbiased=False) + 1e-6)
    assert ops.gemm_lnbwd_supported(M, D, K, BF16)
    nb = max(ops.layernorm_bwd_blocks(M), 256 + 16)
    dx = torch.full((M, D), float("nan"), device=dev(), dtype=torch.bfloat16)
    part = torch.empty(nb * (2 * D + 2), device=dev())
    dg, db = torch.empty(D, device=dev()), torch.empty(D, device=dev())
    ops.gemm_nt_lnbwd(A, Wt, x, mean, rstd, gamma, dx, part, dg, db, add1=add1, a1=a1)
    rows = check_rows(M, (K * 2, D * 4))
    dy = A[rows].double() @ Wt.double().t()
    xh = (x[rows].double() - mean[rows].double()[:, None]) * rstd[rows].double()[:, None]
    gy = dy * gamma.double()
    ref = rstd[rows].double()[:, None] * (gy - gy.mean(1, keepdim=True) - xh * (gy * xh).mean(1, keepdim=True)) + 0.7 * add1[rows].double()
    torch.testing.assert_close(dx[rows].double(), ref, rtol=1e-2, atol=1e-2)
    # the unfused pair (D = 384: dx bit for bit, the row-tile kernel's contract)
    dyb = torch.empty(M, D, device=dev(), dtype=torch.bfloat16)
    ops.gemm_nt(A, Wt, dyb, dtype=BF16, epilogue=ops.EPI_NONE)
    del A
    dx2 = torch.empty(M, D, device=dev(), dtype=torch.bfloat16)
    dg2, db2 = torch.empty(D, device=dev()), torch.empty(D, device=dev())
    part = torch.empty(nb * (2 * D + 2), device=dev())
    ops.layernorm_bwd(dyb, x, gamma, mean, rstd, dx2, part, dg2, db2, M, D, BF16, add1=add1, a1=a1)
    return dx, dx2, dg, dg2, db, db2


@pytest.mark.parametrize("M", [(G31 // (768 * 2) + 16) // 16 * 16, G31 // (768 * 2) + 37], ids=["ring", "register"])
def test_gemm_nt_lnbwd_d192_past_2gb(M):
    dx, dx2, dg, dg2, db, db2 = lnbwd_case(M, 192, 768, seed=81)
    # the unfused pair rounds dy to bf16 before the LayerNorm backward: each form is within 1e-2 of float64, so 2e-2 of each other
    torch.testing.assert_close(dx.float(), dx2.float(), rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(dg, dg2, rtol=1e-4, atol=1e-2 + 1e-5 * M)
    torch.testing.assert_close(db, db2, rtol=1e-4, atol=1e-2 + 1e-5 * M)


def test_gemm_nt_lnbwd_d384_at_its_bound():
    """D = 384 (k_gemm_row384_lnbwd) is supported up to M * K < 2^30 (A below 2 GB): the largest such M at K = 1536 -- bit-identical dx."""
    from uvc_amd import ops
    K = 1536
    M = ((1 << 30) - 1) // K
    assert M * K < (1 << 30) and not ops.gemm_lnbwd_supported(M + 1, 384, K, BF16)
    dx, dx2, dg, dg2, db, db2 = lnbwd_case(M, 384, K, seed=91)
    assert torch.equal(dx, dx2)
    torch.testing.assert_close(dg, dg2, rtol=1e-4, atol=1e-2 + 1e-5 * M)
    torch.testing.assert_close(db, db2, rtol=1e-4, atol=1e-2 + 1e-5 * M)


# ------------------------------------------------------------------------------------------------------------------------------
#   attention with qkv past 2^31 bytes: the first and last images against float64
# ------------------------------------------------------------------------------------------------------------------------------
def attn_ref(qkv, dout, H):
    B, N, _ = qkv.shape
    D = H * 64
    x = qkv.double().requires_grad_(True)
    q, k, v = x.reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * 64 ** -0.5
    o = (s.softmax(-1) @ v).transpose(1, 2).reshape(B, N, D)
    o.backward(dout.double())
    return o.detach(), torch.logsumexp(s, -1).detach(), x.grad


@pytest.mark.parametrize("N,B", [(197, G31 // (197 * 576 * 2) + 2), (1026, G31 // (1026 * 576 * 2) + 2)], ids=["n197", "n1026"])
def test_attention_past_2gb(N, B):
    from uvc_amd import ops
    H = 3
    D = H * 64
    assert B * N * 3 * D * 2 > G31
    qkv = randn(B, N, 3 * D, seed=101)
    dout = randn(B, N, D, seed=102)
    o = torch.full((B, N, D), float("nan"), device=dev(), dtype=torch.bfloat16)
    lse = torch.empty(B, H, N, device=dev())
    ops.attention_fwd(qkv, o, lse, B, N, H, BF16)
    dqkv = torch.full((B, N, 3 * D), float("nan"), device=dev(), dtype=torch.bfloat16)
    delta = torch.empty(B, H, N, device=dev())
    ops.attention_bwd(qkv, o, lse, dout, dqkv, delta, B, N, H, BF16)
    for b in (0, B // 2, B - 1):
        ro, rl, rg = attn_ref(qkv[b:b + 1], dout[b:b + 1], H)
        torch.testing.assert_close(o[b:b + 1].double(), ro, rtol=3e-2, atol=3e-2)
        torch.testing.assert_close(lse[b:b + 1].double(), rl, rtol=2e-2, atol=2e-2)
        torch.testing.assert_close(dqkv[b:b + 1].double(), rg, rtol=5e-2, atol=6e-2)


# ------------------------------------------------------------------------------------------------------------------------------
#   row kernels
# ------------------------------------------------------------------------------------------------------------------------------
def test_layernorm_fwd_bwd_float32_rows_past_2gb():
    from uvc_amd import ops
    D = 192
    rows = G31 // (D * 4) + 41
    x = randn(rows, D, seed=111, dtype=torch.float32)
    gamma = 1.0 + 0.2 * randn(D, seed=112, dtype=torch.float32)
    beta = 0.1 * randn(D, seed=113, dtype=torch.float32)
    y = torch.full((rows, D), float("nan"), device=dev(), dtype=torch.bfloat16)
    mean, rstd = torch.empty(rows, device=dev()), torch.empty(rows, device=dev())
    ops.layernorm_fwd(x, gamma, beta, y, mean, rstd, rows, D, BF16)
    idx = check_rows(rows, (D * 4,))
    ref = F.layer_norm(x[idx].double(), (D,), gamma.double(), beta.double(), 1e-6)
    torch.testing.assert_close(y[idx].double(), ref, rtol=1e-2, atol=1e-2)
    dy = randn(rows, D, seed=114)
    dx = torch.full((rows, D), float("nan"), device=dev())
    partial = torch.empty(ops.layernorm_bwd_blocks(rows) * (2 * D + 2), device=dev())
    dg, db = torch.empty(D, device=dev()), torch.empty(D, device=dev())
    ops.layernorm_bwd(dy, x, gamma, mean, rstd, dx, partial, dg, db, rows, D, BF16)
    xd = x[idx].double().requires_grad_(True)
    F.layer_norm(xd, (D,), gamma.double(), None, 1e-6).backward(dy[idx].double())
    torch.testing.assert_close(dx[idx].double(), xd.grad, rtol=1e-4, atol=1e-4)
    # dbeta = column sums of dy over all rows (float64 in chunks)
    ref_db = torch.zeros(D, device=dev(), dtype=torch.float64)
    for m0 in range(0, rows, 1 << 20):
        ref_db += dy[m0:m0 + (1 << 20)].double().sum(0)
    torch.testing.assert_close(db.double(), ref_db, rtol=1e-4, atol=1e-3 * math.sqrt(rows / 1576))
