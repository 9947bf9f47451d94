"""GPU: the long-sequence kernels (256 < N <= 1026) through the C-ABI.

Attention forward / backward (the streaming kernels of attention.hip) against float64 torch at the bounds tests/test_kernels_gpu.py
uses for N <= 256, a peaky-score case that moves the row maximum late in the sequence (the online-softmax rescale), head skipping,
determinism, batch independence and the N > 1026 refusal; the patch top-k for 256 < P <= 1024 against oracle/vit.py:patch_topk_mask
with bit-exact index sets and its backward against float64 autograd."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1


def dev():
    return torch.device("cuda")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev())


def to_t(x, dtype):
    return x if dtype == F32 else x.to(torch.bfloat16)


def _run(qkv, dout, B, N, H, dtype, head_keep=None):
    from uvc_amd import ops
    T = ops.tdtype(dtype)
    D = H * 64
    o = torch.full((B, N, D), float("nan"), device=dev(), dtype=T)
    lse = torch.full((B, H, N), float("nan"), device=dev())
    ops.attention_fwd(qkv, o, lse, B, N, H, dtype, head_keep=head_keep)
    dqkv = torch.full((B, N, 3 * D), float("nan"), device=dev(), dtype=T)
    delta = torch.full((B, H, N), float("nan"), device=dev())
    ops.attention_bwd(qkv, o, lse, dout, dqkv, delta, B, N, H, dtype, head_keep=head_keep)
    torch.cuda.synchronize()
    return o, lse, dqkv, delta


def _reference(qkv, dout, B, N, H):
    x = qkv.double().requires_grad_(True)
    q, k, v = x.reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * 64 ** -0.5
    ref = (s.softmax(-1) @ v).transpose(1, 2).reshape(B, N, H * 64)
    ref.backward(dout.double())
    return ref.detach(), torch.logsumexp(s, -1).detach(), x.grad


def _check(qkv, dout, B, N, H, dtype):
    o, lse, dqkv, delta = _run(qkv, dout, B, N, H, dtype)
    ref, ref_lse, ref_dqkv = _reference(qkv, dout, B, N, H)
    # the bounds of test_kernels_gpu.py::test_attention_fwd_bwd
    t = dict(rtol=1e-4, atol=1e-5) if dtype == F32 else dict(rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(o.double(), ref, **t)
    torch.testing.assert_close(lse.double(), ref_lse, rtol=1e-4 if dtype == F32 else 2e-2, atol=1e-4 if dtype == F32 else 2e-2)
    tb = dict(rtol=2e-4, atol=2e-5) if dtype == F32 else dict(rtol=5e-2, atol=6e-2)
    torch.testing.assert_close(dqkv.double(), ref_dqkv, **tb)
    torch.testing.assert_close(delta.double(), (dout.double() * o.double()).view(B, N, H, 64).sum(-1).permute(0, 2, 1), rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("B,N,H", [(2, 257, 2), (2, 577, 3), (1, 578, 12), (2, 785, 2), (1, 1026, 3)])
def test_long_attention_fwd_bwd(dtype, B, N, H):
    D = H * 64
    qkv = to_t(rnd(B, N, 3 * D, seed=N + H), dtype)
    dout = to_t(rnd(B, N, D, seed=N + H + 1), dtype)
    _check(qkv, dout, B, N, H, dtype)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_long_attention_peaky_scores_late_maximum(dtype):
    """|scaled score| up to ~30, and for every query the largest score sits on a key in the last tiles (its K row is a scaled copy of
    the query direction): the running maximum grows tile after tile, so each rescale of the accumulated O and sum is exercised."""
    B, N, H = 2, 577, 2
    D = H * 64
    qkv = rnd(B, N, 3, H, 64, seed=7)
    q = qkv[:, :, 0]
    q = q / q.norm(dim=-1, keepdim=True)
    qkv[:, :, 0] = q * 16.0
    k = qkv[:, :, 1]
    k = k / k.norm(dim=-1, keepdim=True) * 16.0
    # key norms grow with the position (random directions: scaled scores of a few units, larger the later the key) ...
    grow = (0.2 + 0.8 * torch.arange(N, device=dev(), dtype=torch.float32) / N).view(1, N, 1, 1)
    qkv[:, :, 1] = k * grow * 0.6
    # ... and keys 530 .. 559 are parallel to the same position's query: a scaled score of 16 * 15 / 8 = 30 in the 9th of 10 key tiles
    qkv[:, 530:560, 1] = qkv[:, 530:560, 0] * (15.0 / 16.0)
    qkv = to_t(qkv.reshape(B, N, 3 * D).contiguous(), dtype)
    s = (qkv.float().view(B, N, 3, H, 64)[:, :, 0] * 0.125).transpose(1, 2) @ qkv.float().view(B, N, 3, H, 64)[:, :, 1].permute(0, 2, 3, 1)
    assert float(s.abs().max()) > 20.0
    dout = to_t(rnd(B, N, D, seed=8), dtype)
    _check(qkv, dout, B, N, H, dtype)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_long_attention_head_keep(dtype):
    """Skipped heads: exactly zero o / dq / dk / dv; the kept heads bit for bit what a run without head_keep gives (dout zero on the
    skipped head's columns, as the Stage-2 masks make it)."""
    B, N, H = 2, 577, 3
    D = H * 64
    qkv = to_t(rnd(B, N, 3 * D, seed=31), dtype)
    dout = to_t(rnd(B, N, D, seed=32), dtype)
    dout.view(B, N, H, 64)[:, :, 1] = 0
    keep = torch.tensor([1, 0, 1], device=dev(), dtype=torch.int32)
    o0, _, d0, _ = _run(qkv, dout, B, N, H, dtype)
    o1, _, d1, _ = _run(qkv, dout, B, N, H, dtype, head_keep=keep)
    assert float(o1.view(B, N, H, 64)[:, :, 1].abs().max()) == 0.0
    assert float(d1.view(B, N, 3, H, 64)[:, :, :, 1].abs().max()) == 0.0
    for h in (0, 2):
        assert torch.equal(o0.view(B, N, H, 64)[:, :, h], o1.view(B, N, H, 64)[:, :, h])
        assert torch.equal(d0.view(B, N, 3, H, 64)[:, :, :, h], d1.view(B, N, 3, H, 64)[:, :, :, h])


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_long_attention_deterministic_and_batch_independent(dtype):
    B, N, H = 5, 785, 2
    D = H * 64
    qkv = to_t(rnd(B, N, 3 * D, seed=41), dtype)
    dout = to_t(rnd(B, N, D, seed=42), dtype)
    a = _run(qkv, dout, B, N, H, dtype)
    b = _run(qkv, dout, B, N, H, dtype)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for img in (0, 3):
        one = _run(qkv[img:img + 1].contiguous(), dout[img:img + 1].contiguous(), 1, N, H, dtype)
        for x, y in zip(a, one):
            assert torch.equal(x[img:img + 1], y)


def test_long_attention_refuses_n_above_1026():
    from uvc_amd import _lib as L
    from uvc_amd import ops
    B, N, H = 1, 1027, 1
    qkv = torch.zeros(B, N, 3 * 64, device=dev(), dtype=torch.bfloat16)
    o = torch.empty(B, N, 64, device=dev(), dtype=torch.bfloat16)
    lse = torch.empty(B, H, N, device=dev())
    with pytest.raises(L.UvcHipError, match="1026"):
        ops.attention_fwd(qkv, o, lse, B, N, H, BF16)
    with pytest.raises(L.UvcHipError):
        ops.attention_bwd(qkv, o, lse, o.clone(), torch.empty_like(qkv), torch.empty_like(lse), B, N, H, BF16)
    # the one-pass backward stays refused at long N
    n2 = 577
    qkv2 = torch.zeros(B, n2, 3 * 64, device=dev(), dtype=torch.bfloat16)
    o2, lse2 = torch.empty(B, n2, 64, device=dev(), dtype=torch.bfloat16), torch.empty(B, H, n2, device=dev())
    with pytest.raises(L.UvcHipError):
        ops.attention_bwd(qkv2, o2, lse2, o2.clone(), torch.empty_like(qkv2), torch.empty_like(lse2), B, n2, H, BF16, variant=2)
    torch.cuda.synchronize()


# ---- patch top-k, 256 < P <= 1024
@pytest.mark.parametrize("B,P,tau", [(8, 257, 1.0), (16, 576, 0.7), (8, 784, 2.0), (4, 1024, 0.5)])
def test_long_patch_topk_bit_exact_indices(B, P, tau):
    from oracle import vit as OV
    from uvc_amd import ops
    k = int(0.9 * P)
    g = torch.Generator().manual_seed(77 + P)
    scores = torch.randn(B, P, generator=g) * 1.5
    e = torch.empty(B, P).exponential_(generator=g)
    ref_mask, ref_index = OV.patch_topk_mask(scores.clone(), e, k, tau)
    y_ref = ((F.log_softmax(scores, -1) - e.log()) / tau).softmax(-1)
    ys_sorted = y_ref.sort(-1, descending=True)[0]
    assert bool((ys_sorted[:, k - 1] > ys_sorted[:, k]).all())
    mask, ys, ps = (torch.empty(B, P, device=dev()) for _ in range(3))
    ops.patch_topk_mask(scores.to(dev()), e.to(dev()), mask, ys, ps, B, P, k, float(tau))
    hard = torch.zeros(B, P).scatter_(1, ref_index, 1.0) > 0.5
    hard[:, 0] = True
    assert torch.equal(mask.cpu() > 0.5, hard)
    torch.testing.assert_close(mask.cpu(), ref_mask.detach(), rtol=0, atol=2e-6)
    s64 = scores.double().requires_grad_(True)
    y64 = ((F.log_softmax(s64, -1) - e.double().log()) / tau).softmax(-1)
    torch.testing.assert_close(ys.cpu().double(), y64.detach(), rtol=2e-5, atol=1e-30)
    torch.testing.assert_close(ps.cpu().double(), F.softmax(s64, -1).detach(), rtol=2e-5, atol=1e-30)
    dmask = torch.randn(B, P, generator=g)
    dm = dmask.clone().double()
    dm[:, 0] = 0
    (y64 * dm).sum().backward()
    ds = torch.empty(B, P, device=dev())
    ops.patch_topk_mask_bwd(dmask.to(dev()), ys, ps, ds, B, P, float(tau))
    torch.testing.assert_close(ds.cpu().double(), s64.grad, rtol=5e-4, atol=3e-6 / min(tau, 1.0))


def test_long_patch_topk_exact_ties_pick_the_lower_index_and_refuses_p_above_1024():
    from uvc_amd import _lib as L
    from uvc_amd import ops
    B, P, k = 2, 784, 705
    mask, ys, ps = (torch.empty(B, P, device=dev()) for _ in range(3))
    ops.patch_topk_mask(torch.zeros(B, P, device=dev()), torch.full((B, P), 0.5, device=dev()), mask, ys, ps, B, P, k, 1.0)
    hard = mask.cpu() > 0.5
    assert hard[:, :k].all() and not hard[:, k:].any()
    P = 1025
    mask, ys, ps = (torch.empty(B, P, device=dev()) for _ in range(3))
    with pytest.raises(L.UvcHipError):
        ops.patch_topk_mask(torch.zeros(B, P, device=dev()), torch.ones(B, P, device=dev()), mask, ys, ps, B, P, 10, 1.0)
