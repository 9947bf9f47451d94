"""CPU: the float64 references of tests/small_kernel_refs.py against independent statements of the same operations --
torch.optim.AdamW behind clip_grad_norm_, autograd through a dense masked MLP, and the oracle package's distillation loss."""
import pytest
import torch

import small_kernel_refs as R
from oracle import step as OS


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


@pytest.mark.parametrize("gscale", [0.002, 3.0])          # total norm below / above max_norm
def test_adamw_ref_is_clip_grad_norm_then_torch_adamw(gscale):
    """Two parameter groups (weight_decay .05 and 0), one parameter without a gradient, clip_grad_norm_ in front of each of three
    steps; the flat restatement carries the same grouping in its flag bytes."""
    na, nb, nc = 37, 11, 6
    lr, betas, eps, wd, max_norm = 3e-4, (0.9, 0.999), 1e-8, 0.05, 1.0
    a, b, c = (torch.nn.Parameter(rnd(n, seed=s)) for n, s in ((na, 1), (nb, 2), (nc, 3)))
    opt = torch.optim.AdamW([dict(params=[a, c], weight_decay=wd), dict(params=[b], weight_decay=0.0)], lr=lr, betas=betas, eps=eps)
    flags = torch.cat([torch.full((na,), R.DECAY), torch.zeros(nb), torch.full((nc,), R.DECAY | R.FROZEN)]).to(torch.uint8)
    p = torch.cat([a.data, b.data, c.data]).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step in (1, 2, 3):
        ga, gb = rnd(na, seed=10 + step, scale=gscale * step), rnd(nb, seed=20 + step, scale=gscale)
        a.grad, b.grad, c.grad = ga.clone(), gb.clone(), None
        total = torch.nn.utils.clip_grad_norm_([a, b, c], max_norm)
        assert (float(total) > max_norm) == (gscale > 1)
        opt.step()
        g = torch.cat([ga, gb, rnd(nc, seed=30 + step)])          # whatever lies under a frozen element is not read
        sq = float((ga * ga).sum() + (gb * gb).sum())
        p, m, v = R.adamw_ref(p, g, m, v, sq, lr, step, betas, eps, wd, max_norm, flags)
        torch.testing.assert_close(p, torch.cat([a.data, b.data, c.data]), rtol=1e-12, atol=1e-12)
        st = opt.state
        torch.testing.assert_close(m[:na + nb], torch.cat([st[a]["exp_avg"], st[b]["exp_avg"]]), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(v[:na + nb], torch.cat([st[a]["exp_avg_sq"], st[b]["exp_avg_sq"]]), rtol=1e-12, atol=1e-12)
        assert c not in st and not m[na + nb:].any() and not v[na + nb:].any()
    assert torch.equal(p[na + nb:], c.data)
    # flags=None: one group, every element decays
    q = torch.nn.Parameter(rnd(50, seed=4))
    opt = torch.optim.AdamW([q], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    q0, gq = q.data.clone(), rnd(50, seed=5, scale=gscale)
    q.grad = gq.clone()
    torch.nn.utils.clip_grad_norm_([q], max_norm)
    opt.step()
    pn, _, _ = R.adamw_ref(q0, gq, torch.zeros(50), torch.zeros(50), float((gq * gq).sum()), lr, 1, betas, eps, wd, max_norm, None)
    torch.testing.assert_close(pn, q.data, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("D,F_,width", [(8, 24, 5), (12, 10, 10), (6, 16, 1)])
def test_mlp_scatter_ref_rank_one_rule_is_what_autograd_gives(D, F_, width):
    """Scattering the compact MLP's gradients and filling the pruned fc2 columns with GELU(b1[j]) * db2 reproduces autograd's gradients
    of the dense MLP whose pruned fc1 rows / fc2 columns are zero."""
    x, dy = rnd(37, D, seed=1), rnd(37, D, seed=2)
    W1, b1, W2, b2 = rnd(F_, D, seed=3), rnd(F_, seed=4), rnd(D, F_, seed=5), rnd(D, seed=6)
    idx = torch.randperm(F_, generator=torch.Generator().manual_seed(7))[:width]
    ref = R.mlp_scatter_ref(x, W1, b1, W2, b2, idx, dy)
    torch.testing.assert_close(ref["outc"], ref["out"], rtol=1e-12, atol=1e-12)
    dW1, db1, dW2, pruned = R.mlp_scatter_expand(ref, idx, b1)
    assert int(pruned.sum()) == F_ - width
    torch.testing.assert_close(dW1, ref["dW1"], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(db1, ref["db1"], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(dW2, ref["dW2"], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ref["db2"], dy.sum(0), rtol=1e-12, atol=1e-12)
    assert not ref["dW1"][pruned].any() and not ref["db1"][pruned].any()
    if width < F_:
        assert ref["dW2"][:, pruned].abs().max() > 0


@pytest.mark.parametrize("kind,name", [(0, "none"), (1, "soft"), (2, "hard")])
@pytest.mark.parametrize("one_head", [True, False])
def test_distill_loss_ref_equals_the_oracle_loss(kind, name, one_head):
    B, C, alpha, tau = 5, 13, 0.3, 2.5
    o, t = rnd(B, C, seed=1, scale=2), rnd(B, C, seed=3, scale=2)
    y = torch.softmax(rnd(B, C, seed=2), -1) * torch.tensor([0.7, 1.0, 1.3, 1.0, 1.0], dtype=torch.float64)[:, None]
    okd = o if one_head else rnd(B, C, seed=4)
    loss, d_o, d_k = R.distill_loss_ref(o, okd, y, t, alpha, tau, kind)
    oo = o.clone().requires_grad_(True)
    ok = oo if one_head else okd.clone().requires_grad_(True)
    want = OS.distillation_loss(oo, ok, y, t, kind=name, alpha=alpha, T=tau)
    want.backward()
    torch.testing.assert_close(loss, want.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(d_o, oo.grad, rtol=1e-12, atol=1e-12)
    if one_head or kind == 0:
        assert d_k is None
    else:
        torch.testing.assert_close(d_k, ok.grad, rtol=1e-12, atol=1e-12)


def test_elementwise_refs_on_hand_computed_values():
    pg = torch.tensor([-5.0, 0.0, -0.0, 2.0, -1e-3])
    assert R.sigmoid_gate_ref(pg, 2, True).tolist() == [[1.0, 1.0, 1.0, 1.0, 0.0]] * 2
    torch.testing.assert_close(R.sigmoid_gate_ref(pg, 1, False)[0, 3], torch.tensor(1 / (1 + 2.718281828459045 ** -2), dtype=torch.float64))
    torch.testing.assert_close(R.sigmoid_gate_bwd_ref(torch.zeros(2), torch.tensor([[1.0, 2.0], [3.0, 4.0]])), torch.tensor([1.0, 1.5], dtype=torch.float64))
    g, e = torch.tensor([[0.3, 0.3], [0.0, 1.0], [2.0, 0.0]]), torch.tensor([[0.7, 0.7], [1.0, 1.0], [1.0, 1.0]])
    assert R.gate_distrib_ref(g, e, 3, 0.1).tolist() == [[1.0, 0.0], [0.0, 1.0], [1.0, 0.0]]          # a tie goes to index 0
    torch.testing.assert_close(R.gate_distrib_ref(g, e, 1, 0.1).sum(-1), torch.ones(3, dtype=torch.float64))
    torch.testing.assert_close(R.gate_distrib_ref(g, e, 2, 0.1)[1], torch.tensor([0.1 / 1.1, 1 / 1.1], dtype=torch.float64))
    X = torch.tensor([[1.0, 2.0], [3.0, 4.0]])
    assert R.colsum_ref(X, torch.tensor([2.0, -1.0]), 0.5).tolist() == [-0.5, 0.0]
    assert R.add_outer_ref(X, torch.tensor([1.0, 2.0]), torch.tensor([10.0, 20.0])).tolist() == [[11.0, 22.0], [23.0, 44.0]]
    assert R.patch_scores_ref(X, torch.tensor([1.0, -1.0]), torch.tensor([0.5])).tolist() == [-0.5, -0.5]
