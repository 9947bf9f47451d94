"""What the linear-probe tests share (CPU and GPU; nothing here needs a GPU): overlapping Gaussian classes, the float64 objective through
autograd, float32 / bfloat16 spacing helpers, the row kernel's float64 reference and its cases."""
import math

import torch


def gaussian_classes(n, D, C, seed, spread=1.0, scale=1.0):
    """``(X float64 [n, D], y int64 [n])``: class c is a unit Gaussian around a centre of norm ~ ``spread`` -- classes that OVERLAP, so the
    regularised optimum is finite and well inside float range -- times ``scale``."""
    g = torch.Generator().manual_seed(seed)
    centres = spread * torch.randn(C, D, generator=g, dtype=torch.float64) / math.sqrt(D) * 3.0
    y = torch.arange(n) % C
    y = y[torch.randperm(n, generator=g)]
    X = centres[y] + torch.randn(n, D, generator=g, dtype=torch.float64)
    return scale * X, y


def autograd_objective(W, b, X, y, l2):
    """``(F, dW, db)`` of the issue's objective by autograd in float64, rows with a label outside [0, C) dropped beforehand."""
    W = W.detach().double().clone().requires_grad_()
    bb = None if b is None else b.detach().double().clone().requires_grad_()
    keep = (y >= 0) & (y < W.shape[0])
    z = X.double()[keep] @ W.T + (0 if bb is None else bb)
    F = torch.nn.functional.cross_entropy(z, y[keep], reduction="mean") + 0.5 * l2 * (W * W).sum()
    F.backward()
    return float(F), W.grad, None if bb is None else bb.grad


def ulp32(v):
    """the float32 spacing at |v| (float64 tensor in, float64 out; 2^-149 at 0)"""
    v = v.abs().double().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(v)) - 23)


def bf16_key(t):
    """int32 keys of bfloat16 values that rise by one from each value to the next one up (-0 and +0 share key 0): two values are
    neighbours when their keys differ by 1"""
    bits = t.contiguous().view(torch.int16).to(torch.int32)
    mag = bits & 0x7fff
    return torch.where(bits < 0, -mag, mag)


def row_reference(logits, labels, C):
    """float64 on the float32 logits as given: ``(G [rows, ld], loss [rows], hit [rows] int64, p [rows, ld])``; columns [C, ld) and rows
    whose label lies outside [0, C) are zeros."""
    z = logits.double()[:, :C]
    rows, ld = logits.shape
    y = labels.to(torch.int64)
    keep = (y >= 0) & (y < C)
    p = torch.zeros(rows, ld, dtype=torch.float64)
    p[:, :C] = torch.softmax(z, dim=1)
    G = p.clone()
    yc = y.clamp(0, C - 1)
    others = p.clone()
    others[torch.arange(rows), yc] = 0
    G[torch.arange(rows), yc] = -others.sum(1)                       # p_y - 1 without float64's own cancellation near p_y = 1
    G[~keep] = 0
    lse = torch.logsumexp(z, dim=1)
    loss = (lse - z[torch.arange(rows), yc]) * keep
    hit = ((z.argmax(dim=1) == yc) & keep).to(torch.int64)
    return G, loss, hit, p


def row_logits(rows, C, ld, kind, seed):
    """float32 [rows, ld] logits (the padding columns hold NaN: they must never be read into a result) and int64 labels with -1 and C among them.
    normal: N(0, 3); huge: magnitude 3e4; ties: rows of equal logits, and rows whose maximum appears twice."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(rows, ld, generator=g) * 3.0
    if kind == "huge":
        z = (torch.rand(rows, ld, generator=g) * 2 - 1) * 3e4
    elif kind == "ties":
        z = torch.randint(-2, 3, (rows, ld), generator=g).float()
        z[::3] = 1.5                                                 # every third row: all equal -> the first maximum is column 0
    z[:, C:] = float("nan")
    y = torch.randint(0, C, (rows,), generator=g)
    if kind == "ties":
        y[::2] = 0
    if rows >= 4:
        y[1], y[rows - 2] = -1, C
    return z, y


def blocks_of(rows, per):
    """the rows of each workgroup's partial: runs of ``per`` consecutive rows (the last one short)"""
    return [slice(r0, min(rows, r0 + per)) for r0 in range(0, rows, per)]



class LowEvaluator:
    """``fit_probe``'s evaluator on the CPU in the device's arithmetic, as far as PyTorch states it: float32 parameters, products and sums
    ("fp32"), or with X, W and G each rounded once to bfloat16 around float32 sums ("bf16")."""
    dtype, device = torch.float32, "cpu"

    def __init__(self, precision):
        self.precision = precision

    def _round(self, t):
        return t.float().bfloat16().float() if self.precision == "bf16" else t.float()

    def prepare(self, features, labels):
        return self._round(features), labels.to(torch.int64)

    def __call__(self, W, b, X, y, l2):
        C = W.shape[0]
        keep = (y >= 0) & (y < C)
        m = max(int(keep.sum()), 1)
        z = X @ self._round(W).T + (0 if b is None else b)
        p = torch.softmax(z, dim=1)
        yc = y.clamp(0, C - 1)
        rows = torch.arange(len(y))
        loss = (torch.logsumexp(z, dim=1) - z[rows, yc]) * keep
        G = p.clone()
        G[rows, yc] -= 1.0
        G = self._round(G * keep[:, None])
        F = float(loss.sum()) / m + 0.5 * l2 * float((W * W).sum())
        hits = int(((z.argmax(1) == yc) & keep).sum())
        return F, G.T @ X / m + l2 * W, (None if b is None else G.sum(0) / m), hits
