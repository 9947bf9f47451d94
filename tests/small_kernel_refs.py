"""Plain float64 references of the small kernels (uvc_amd/csrc/elementwise.hip, loss_optim.hip): elementwise ops, the
distillation loss and clip + AdamW.  Torch only, CPU-runnable, nothing from uvc_amd; tests/test_small_kernel_refs_cpu.py checks
them against torch.optim.AdamW, autograd and the oracle package, tests/test_small_kernels_gpu.py holds the kernels to them."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

DECAY, FROZEN = 1, 2          # bits of the per-element flag byte of uvc_adamw_step


def f64(t):
    return t.detach().to(device="cpu", dtype=torch.float64)


# ----------------------------------------------------------------------------- clip + AdamW
def clip_coef(sq, max_norm):
    """clip_grad_norm_'s factor from the sum of squares of all gradients."""
    return min(1.0, max_norm / (math.sqrt(sq) + 1e-6))


def adamw_ref(p, g, m, v, sq, lr, step, betas, eps, wd, max_norm, flags):
    """clip_grad_norm_(max_norm) followed by one torch.optim.AdamW step, per element, in float64.  ``sq``: sum of squares of the
    whole gradient (float); ``flags`` (uint8 per element or None = every element decays): bit 0 selects weight decay, bit 1 leaves
    p, m, v of that element untouched (a parameter whose .grad is None).  Returns the new (p, m, v)."""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    b1, b2 = betas
    fl = torch.full(p.shape, DECAY, dtype=torch.uint8) if flags is None else flags.detach().cpu()
    decay, live = (fl & DECAY) != 0, (fl & FROZEN) == 0
    gc = g * clip_coef(sq, max_norm)
    pn = torch.where(decay, p * (1.0 - lr * wd), p)
    mn = b1 * m + (1.0 - b1) * gc
    vn = b2 * v + (1.0 - b2) * gc * gc
    denom = vn.sqrt() / math.sqrt(1.0 - b2 ** step) + eps
    pn = pn - (lr / (1.0 - b1 ** step)) * (mn / denom)
    return torch.where(live, pn, p), torch.where(live, mn, m), torch.where(live, vn, v)


# ----------------------------------------------------------------------------- distillation loss
def distill_loss_ref(o, o_kd, y, t, alpha, tau, kind):
    """DistillationLoss over SoftTargetCrossEntropy in float64 with autograd gradients.  kind 0: plain soft-target cross-entropy with
    weight 1 (o_kd, t unused); 1: soft (KL at temperature tau, scaled tau^2 / numel); 2: hard (CE against the teacher's argmax).
    ``o_kd is o`` (or None): one head.  Returns (loss, d_o, d_okd); d_okd is None with one head, where d_o is the whole gradient."""
    od = f64(o).requires_grad_(True)
    one_head = kind == 0 or o_kd is None or o_kd is o
    kd_in = od if one_head else f64(o_kd).requires_grad_(True)
    base = torch.sum(-f64(y) * F.log_softmax(od, -1), -1).mean()
    if kind == 0:
        loss = base
    else:
        td = f64(t)
        if kind == 1:
            kd = F.kl_div(F.log_softmax(kd_in / tau, 1), F.log_softmax(td / tau, 1), reduction="sum", log_target=True) * (tau * tau) / td.numel()
        else:
            kd = F.cross_entropy(kd_in, td.argmax(dim=1))
        loss = base * (1 - alpha) + kd * alpha
    loss.backward()
    return loss.detach(), od.grad, None if one_head else kd_in.grad


# ----------------------------------------------------------------------------- MLP compaction
def mlp_scatter_ref(x, W1, b1, W2, b2, idx, dy):
    """Dense float64 MLP out = fc2(GELU(fc1(x))) with loss <out, dy>, where every hidden unit NOT in ``idx`` is pruned: its fc1 row
    and fc2 column are zero, its biases stay.  Returns autograd's gradients of the dense masked MLP (dW1 [F,D], db1 [F], dW2 [D,F],
    db2 [D]) and, separately, autograd's gradients of the compact MLP built from the kept units alone (dw1c [width,D], db1c [width],
    dw2c [D,width]): the two networks compute the same output, and the dense gradient of a pruned fc2 column is GELU(b1[j]) * db2."""
    x, dy, idx = f64(x), f64(dy), idx.detach().cpu().long()
    F_ = W1.shape[0]
    keep = torch.zeros(F_, dtype=torch.bool)
    keep[idx] = True
    W1d = (f64(W1) * keep[:, None]).requires_grad_(True)
    W2d = (f64(W2) * keep[None, :]).requires_grad_(True)
    b1d, b2d = f64(b1).requires_grad_(True), f64(b2).requires_grad_(True)
    out = F.linear(F.gelu(F.linear(x, W1d, b1d)), W2d, b2d)
    (out * dy).sum().backward()
    w1c, b1c, w2c = (W1d.detach()[idx].requires_grad_(True), b1d.detach()[idx].requires_grad_(True),
                     W2d.detach()[:, idx].requires_grad_(True))
    outc = F.linear(F.gelu(F.linear(x, w1c, b1c)), w2c, b2d.detach())
    (outc * dy).sum().backward()
    return dict(dW1=W1d.grad, db1=b1d.grad, dW2=W2d.grad, db2=b2d.grad, dw1c=w1c.grad, db1c=b1c.grad, dw2c=w2c.grad,
                out=out.detach(), outc=outc.detach())


def mlp_scatter_expand(ref, idx, b1):
    """The rule uvc_mlp_scatter_grads implements, in float64: compact gradients scattered to their units, zeros for the pruned fc1
    rows / biases, GELU(b1[j]) * db2 for the pruned fc2 columns."""
    idx = idx.detach().cpu().long()
    F_, D = ref["dW1"].shape
    pruned = torch.ones(F_, dtype=torch.bool)
    pruned[idx] = False
    dW1, db1 = torch.zeros(F_, D, dtype=torch.float64), torch.zeros(F_, dtype=torch.float64)
    dW1[idx], db1[idx] = ref["dw1c"], ref["db1c"]
    dW2 = F.gelu(f64(b1))[None, :] * ref["db2"][:, None]
    dW2[:, idx] = ref["dw2c"]
    return dW1, db1, dW2, pruned


# ----------------------------------------------------------------------------- elementwise one-liners
def sigmoid_gate_ref(pg, B, hard):
    """mask[b, i] = sigmoid(pg[i]), or [sigmoid >= .5] with token 0 always kept."""
    s = torch.sigmoid(f64(pg))
    if hard:
        s = (s >= 0.5).double()
        s[0] = 1.0
    return s.expand(B, -1).clone()


def sigmoid_gate_bwd_ref(pg, dmask):
    s = torch.sigmoid(f64(pg))
    return f64(dmask).sum(0) * s * (1 - s)


def patch_scores_ref(pe, w, bias):
    return f64(pe) @ f64(w) + f64(bias)


def add_outer_ref(X, rw, w):
    return f64(X) + torch.outer(f64(rw), f64(w))


def apply_masks_ref(params, mask):
    return params * mask


def colsum_ref(X, row_weight=None, alpha=1.0):
    Xd = f64(X)
    return alpha * (Xd if row_weight is None else Xd * f64(row_weight)[:, None]).sum(0)


def gate_logits_ref(g, e):
    """u = (g + Gumbel) / tau with tau = .5, Gumbel = -log(E)."""
    return (f64(g) - f64(e).log()) / 0.5


def gate_distrib_ref(g, e, mode, eps):
    """mode 0: (.5, .5); 1: softmax(u); 2: softL0 (1 - d1, d1), d1 = g1^2 / (g1^2 + eps); 3: one-hot argmax(u), ties to index 0."""
    gd = f64(g)
    if mode == 0:
        return torch.full_like(gd, 0.5)
    if mode == 2:
        d1 = gd[:, 1] ** 2 / (gd[:, 1] ** 2 + eps)
        return torch.stack([1 - d1, d1], 1)
    u = gate_logits_ref(g, e)
    return u.softmax(-1) if mode == 1 else F.one_hot(u.argmax(-1), 2).double()
