"""GPU: the early weight-gradient flushes of the backward's lowest block change no bit.

uvc_vit_backward hands the weight gradients of the LAST block of a call (the lowest one that runs in its stage range) to the side stream as soon as their
operands exist -- dW_proj before the attention backward, dW_qkv before dqkv + LayerNorm1' -- instead of at the block's end.  Same kernels, same split-M
reductions, same order on the side stream: the flat gradient must equal the serialized backward's (two_stream_backward off: no side stream, no flush at
all) bit for bit.  DeiT-Tiny, depth 12, 16 images, both precisions; with every block running (the last block is block 0), with blocks 0 and 4
hard-skipped (the last block is block 1, and the walk hops over block 4), and with the backward cut in two calls at block 6 (the DDP path's staged
backward: each call has a last block of its own, 6 and then 0)."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

DEPTH = 12


def _model(precision, skipped):
    from uvc_amd.model_distilled import DistilledVisionTransformer
    torch.manual_seed(11)
    m = DistilledVisionTransformer(0, enable_block_gating=0, embed_dim=192, depth=DEPTH, num_heads=3, precision=precision).cuda()
    m.train()
    with torch.no_grad():
        m.block_skip_gating.data[:, 0] = 0.0
        m.block_skip_gating.data[:, 1] = 1.0
        for l in skipped:
            m.block_skip_gating.data[l] = torch.tensor([1.0, 0.0], device="cuda")
    return m


def _grads(m, x, two_stream):
    m.two_stream_backward = two_stream
    m._flat_grad.zero_()
    out = m(x, -1, 0.9)[0]
    logits = [o for o in (out if isinstance(out, (tuple, list)) else [out]) if o is not None]
    sum((o.float() ** 2).mean() for o in {id(o): o for o in logits}.values()).backward()
    torch.cuda.synchronize()
    return m._flat_grad[:m._off.n_total].clone()


@pytest.fixture(scope="module")
def images():
    return torch.randn(16, 3, 224, 224, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("skipped", [(), (0, 4)], ids=["all_blocks", "blocks_0_and_4_skipped"])
def test_two_stream_backward_equals_the_serialized_backward(images, precision, skipped):
    m = _model(precision, skipped)
    g2 = _grads(m, images, True)
    g1 = _grads(m, images, False)
    assert torch.isfinite(g2).all() and float(g2.abs().max()) > 0
    o = m._off
    for l in range(DEPTH):                                             # a skipped block gets no gradient; every other block does (norm1.weight's here)
        seg = g2[o.blk[l][0]:o.blk[l][0] + 192]
        assert (float(seg.abs().max()) == 0.0) == (l in skipped), l
    assert torch.equal(g1, g2)


@pytest.mark.parametrize("precision", ["bf16"])
def test_backward_in_two_stage_ranges_cut_at_block_6(images, precision):
    m = _model(precision, ())
    whole = _grads(m, images, True)
    serial = _grads(m, images, False)
    calls = []
    # the DDP path's cuts with the collectives stubbed out: stages [0, 7) = heads + blocks 11 .. 6, then [7, L + 3) = blocks 5 .. 0 + the embedding
    m._ddp = SimpleNamespace(world=2, stage_ends=[DEPTH - 6 + 1, DEPTH + 3], pack_dual=lambda: None, unpack_dual=lambda: None,
                             reducer=SimpleNamespace(launch=calls.append, finish=lambda: None))
    try:
        staged = _grads(m, images, True)
    finally:
        m._ddp = None
    assert calls == [0, 1]
    assert torch.equal(staged, whole) and torch.equal(staged, serial)
