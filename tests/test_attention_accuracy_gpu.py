"""GPU: every attention kernel of attention.hip and token_tail.hip against float64 at the tile edges of its dispatch, on four input
families, with the bf16 mode held to the rounding model of tests/attention_refs.py (``accept``: per (image, head) and per row, at most
MARGIN = 3 / ROW_MARGIN = 4 times the error of a float64 computation that rounds to bf16 only where a bf16 kernel must) and the float32
mode to the bounds tests/test_kernels_gpu.py uses for it.  lse and delta are float32 arithmetic in both modes and get the float32 bounds
in both.  On the routing family o_i == v_t(i) and dv_t(i) == dout_i are asserted exactly (after rounding a float32 result to bf16, as the
float64 reference itself is only exact there).  Every output starts as NaN, so a row no kernel wrote fails ``accept``.

What the dispatch makes of N (attention.hip: dispatch, launch): NT16 = 2 / 4 / 8 / 14 / 16 key tiles up to N = 32 / 64 / 128 / 224 / 256, the
compile-time mask NFULL = 12 for 192 <= N <= 207, the streaming kernels (LQ = 128, LK = 64) above 256; the bf16 forward is persistent
(several heads per workgroup, the next head's K / V prefetched) above 512 heads; the one-pass backward takes 193 <= N <= 200.

Measured on an MI355X, bf16 mode: the worst error / model error over every case of the kernel family, per head / per row -- the two figures
``accept`` holds to MARGIN = 3 and ROW_MARGIN = 4:
    kernel family                         o          dq         dk         dv
    short forward + dq, dk/dv pair        1.01/1.07  1.02/1.14  1.03/1.08  1.07/1.17
    persistent forward (> 512 heads)      1.01/1.15
    one-pass backward (variant 2)         1.00/1.18  1.02/1.01  1.07/1.28  1.02/1.06
    v_dim 16 / 32 / 48                    1.02/1.08  1.13/1.33  1.11/1.34  1.08/1.10
    streaming (N > 256)                   0.99/1.05  1.00/1.03  1.03/1.27  1.01/1.03
    token-query, ntok 1 and 2             1.00/1.00  1.00/1.00  1.00/1.00  1.00/1.00
  Every kernel lands at the model: none has a rounding point the model lacks, and the one-pass and token kernels needed none beyond
  attention_refs.ONE_PASS / TOKEN.  The float32 floor took the model's place in dq and dk of the routing family and of the negative family at N = 1
  and nowhere else: there the exact result and the model's are 0 to ~1e-12 and the kernels leave ~1e-7 (float32's dP - delta).  Those cases are not in
  the figures above; every other head and row, the negative and deep-negative token-query dq among them, is held to the plain margins.
  float32 mode, largest |error| / (atol + rtol |ref|): o 0.30, dqkv 0.80 (streaming), lse 0.008, delta 0.002; bf16 mode lse 0.008, delta 0.001.
The deep-negative family guards the clamp of the exponent in k_attn_bwd_dq: without it a padded key's P = exp(-lse) is +inf there and every dq row
with lse < -88.72 comes out NaN, in the pair and the v_dim kernels alike.
"""
import functools

import pytest
import torch

import attention_refs as A

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
ALL4 = (A.RANDOM, A.NEGATIVE, A.ROUTING, A.DEEP_NEGATIVE)


def dev():
    return torch.device("cuda")


@functools.lru_cache(maxsize=2)
def case(family, B, N, H, v_dim=64, ntok=None, backward=True):
    """Inputs and float64 reference on the device, shared by the precisions (and launch shapes) of one case; never modified."""
    return A.make_case(family, B, N, H, v_dim, ntok, seed=B + H, device=dev(), backward=backward)


def operands(c, dtype):
    T = torch.float32 if dtype == F32 else torch.bfloat16
    return c["qkv"].to(T), c["dout"].to(T), T


def nan(shape, T=torch.float32):
    return torch.full(shape, float("nan"), device=dev(), dtype=T)


def forward(c, dtype):
    from uvc_amd import ops
    B, N, H, dv = c["B"], c["N"], c["H"], c["v_dim"]
    qkv, _, T = operands(c, dtype)
    o, lse = nan((B, N, H * dv), T), nan((B, H, N))
    ops.attention_fwd(qkv, o, lse, B, N, H, dtype, v_dim=0 if dv == 64 else dv)
    return o, lse


def backward(c, dtype, o, lse, variant=0, grid=0):
    from uvc_amd import ops
    B, N, H, dv = c["B"], c["N"], c["H"], c["v_dim"]
    qkv, dout, T = operands(c, dtype)
    dqkv, delta = nan((B, N, H * (128 + dv)), T), nan((B, H, N))
    if dv == 64:
        ops.attention_bwd(qkv, o, lse, dout, dqkv, delta, B, N, H, dtype, variant=variant, grid=grid)
    else:
        ops.attention_bwd_vdim(qkv, o, lse, dout, dqkv, delta, B, N, H, dv, dtype)
    torch.cuda.synchronize()
    return dqkv, delta


def close(what, got, ref, rtol, atol):
    """torch.testing.assert_close's rule, with the figure printed first: the largest |got - ref| / (atol + rtol |ref|)."""
    got, ref = got.double(), ref.double()
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite elements"
    r = float(((got - ref).abs() / (atol + rtol * ref.abs())).max())
    print(f"CLOSE {what} {r:.3f}")
    assert r <= 1.0, f"{what}: |got - ref| is {r:.2f} x (atol {atol} + rtol {rtol} |ref|)"


def check(kernel, c, dtype, o, lse=None, dqkv=None, delta=None, rounding=A.PAIR):
    """One kernel family's results of one case: finite, ``accept`` (bf16; float32 on the deep-negative family, where the float32 bounds
    were not made for cancelling sums of that size) or the float32 bounds, lse / delta at the float32 bounds, the routing family's exact rows."""
    ref, H, dv, fam = c["ref"], c["H"], c["v_dim"], c["family"]
    tag = f"{kernel} {A.FAMILY_NAMES[fam]} N={c['N']} {'f32' if dtype == F32 else 'bf16'}"
    for name, t in (("o", o), ("lse", lse), ("dqkv", dqkv), ("delta", delta)):
        if t is not None:
            bad = ~torch.isfinite(t.float())
            assert not bool(bad.any()), f"{tag}: {name} has {int(bad.sum())} non-finite elements, first at {tuple(bad.nonzero()[0].tolist())}"
    got = A.got_from(o, dqkv, H, dv)
    sections = A.SECTIONS if dqkv is not None else ("o",)
    if dtype == BF16 or fam == A.DEEP_NEGATIVE:
        mod = A.model(c["qkv"], c["dout"], H, dv, c["ntok"], rounding, o_given=o if rounding.delta_from_o and dqkv is not None else None,
                      backward=dqkv is not None)
        w = A.accept(got, ref, mod, sections)
        print("RATIO", tag, " ".join(f"{s}={w[s][0]:.2f}/{w[s][1]:.2f}/{w[s][2]:.2f}" for s in sections))
    else:
        close(tag + " o", A.rows(got["o"]), A.rows(ref["o"]), rtol=1e-4, atol=1e-5)
        if dqkv is not None:
            close(tag + " dqkv", dqkv, A.dqkv_of(ref), rtol=2e-4, atol=2e-5)
    if lse is not None:
        close(tag + " lse", lse, ref["lse"], rtol=1e-4, atol=1e-4)
    if delta is not None:
        close(tag + " delta", delta, (A.heads(c["dout"], H).double() * got["o"]).sum(-1), rtol=1e-3, atol=1e-3)
    if fam == A.ROUTING:
        ok_o, ok_dv = A.routing_exact(got["o"], got.get("dv"), c["qkv"], c["dout"], c["t"], H, dv)
        assert ok_o, f"{tag}: o_i != v_t(i)"
        assert ok_dv, f"{tag}: dv_t(i) != dout_i"


# ----------------------------------------------------------------------------- N <= 256: k_attn_fwd, k_attn_bwd_dq, k_attn_bwd_dkv
SHORT_N = [1, 16, 17, 33, 64, 65, 100, 128, 129, 192, 193, 207, 208, 209, 224, 225, 241, 256]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("family", [A.RANDOM, A.NEGATIVE, A.ROUTING])
@pytest.mark.parametrize("N,B,H", [(n, 2, 3) for n in SHORT_N] + [(1, 1, 1), (256, 1, 1)])
def test_short_forward_and_backward_pair(N, B, H, family, dtype):
    """Every NT16 instantiation at both ends of its range, whole tiles of padding (65, 129, 225), no padding (16, 64, 128, 192, 208, 224, 256),
    both ends of the NFULL = 12 specialisation (192, 207) and the run-time mask either side of it."""
    c = case(family, B, N, H)
    o, lse = forward(c, dtype)
    dqkv, delta = backward(c, dtype, o, lse, variant=1)
    check("pair", c, dtype, o, lse, dqkv, delta)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("N", [17, 100, 197, 241])
def test_short_pair_deep_negative_scores(N, dtype):
    """lse < -88.72 in most rows: exp(-lse), the unmasked P of a padded key in k_attn_bwd_dq, is not a float32."""
    c = case(A.DEEP_NEGATIVE, 2, N, 2)
    o, lse = forward(c, dtype)
    dqkv, delta = backward(c, dtype, o, lse, variant=1)
    check("pair", c, dtype, o, lse, dqkv, delta)


@pytest.mark.parametrize("family", [A.ROUTING, A.RANDOM])
@pytest.mark.parametrize("B,H", [(172, 3), (343, 3), (87, 6)])
@pytest.mark.parametrize("N", [17, 40, 197])
def test_persistent_forward_walks_several_heads_per_workgroup(N, B, H, family):
    """More than 512 heads on 512 workgroups: at 516 and 522 heads a few workgroups take a second head, at 1029 every one walks two or three (the
    in-loop pf_load / pf_store twice), in the NT16 = 2, 4 and 14 (NFULL = 12) instantiations each.  The next head's K / V are prefetched while this
    one is computed.  Every head is checked; on the routing family a head computed on another head's K / V fails exactly."""
    assert B * H > 512
    c = case(family, B, N, H, backward=False)
    o, lse = forward(c, BF16)
    torch.cuda.synchronize()
    check("persistent-fwd", c, BF16, o, lse)


@pytest.mark.parametrize("family", ALL4)
@pytest.mark.parametrize("N", [193, 196, 197, 199, 200])
def test_one_pass_backward(N, family):
    """variant 2 (one::k_attn_bwd_one), one head per workgroup (grid 0: 15 heads), and 2 and 4 workgroups drawing their heads from the counter."""
    c = case(family, 5, N, 3)
    o, lse = forward(c, BF16)
    for grid in (0, 2, 4):
        dqkv, delta = backward(c, BF16, o, lse, variant=2, grid=grid)
        check(f"one-pass grid={grid}", c, BF16, o, lse, dqkv, delta, rounding=A.ONE_PASS)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("family", ALL4)
@pytest.mark.parametrize("N", [17, 100, 197, 256])
@pytest.mark.parametrize("v_dim", [16, 32, 48])
def test_compact_value_width_forward_and_backward(v_dim, N, family, dtype):
    c = case(family, 2, N, 3, v_dim)
    o, lse = forward(c, dtype)
    dqkv, delta = backward(c, dtype, o, lse)
    check(f"v_dim={v_dim}", c, dtype, o, lse, dqkv, delta)


# ----------------------------------------------------------------------------- 256 < N <= 1026: the streaming kernels
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("N,family", [(n, f) for n in (257, 320, 321, 384, 577, 1024, 1025, 1026) for f in (A.RANDOM, A.NEGATIVE, A.ROUTING)]
                         + [(321, A.DEEP_NEGATIVE)])
def test_streaming_forward_and_backward(N, family, dtype):
    """Exact multiples of LK = 64 and LQ = 128 (320, 384, 1024), one key past them (257, 321, 1025), the ragged sizes of the models."""
    c = case(family, 1, N, 2)
    o, lse = forward(c, dtype)
    dqkv, delta = backward(c, dtype, o, lse)
    check("streaming", c, dtype, o, lse, dqkv, delta)


# ----------------------------------------------------------------------------- token-query kernels (token_tail.hip)
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("family", ALL4)
@pytest.mark.parametrize("N", [2, 5, 17, 197, 256])
@pytest.mark.parametrize("ntok", [1, 2])
def test_token_query_forward_and_backward(ntok, N, family, dtype):
    from uvc_amd import ops
    B, H = 2, 3
    c = case(family, B, N, H, 64, ntok)
    qkv, dout, T = operands(c, dtype)
    o, dqkv = nan((B, ntok, H * 64), T), nan((B, N, 3 * H * 64), T)
    ops.attention_tok_fwd(qkv, o, B, N, H, ntok, dtype)
    ops.attention_tok_bwd(qkv, o, dout, dqkv, B, N, H, ntok, dtype)
    torch.cuda.synchronize()
    check(f"token ntok={ntok}", c, dtype, o, None, dqkv, None, rounding=A.TOKEN)
    assert float(A.got_from(o, dqkv, H)["dq"][:, :, ntok:].abs().sum()) == 0.0
