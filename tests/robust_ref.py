"""What the robustness tests share (CPU and GPU; nothing here needs a GPU): the exports and batches they run on, the float64 references
(computed once per case and left unchanged), the float64 statement of uvc_loss_seed with its cases, and the float32 PyTorch statement of
uvc_pgd_step with its operands."""
import torch

import attribution_ref as AR
import pixel_attr_ref as PR
from probe_ref import ulp32
from uvc_amd import compact_robust as RB
from uvc_amd import data

NAMES = AR.FIXTURES + AR.EXTRA                 # attribution_ref.export_of's seven: 17 - 198 tokens
BARS = PR.BARS                                 # the project's model-level parity bars: 1e-3 float32, 2e-2 bf16
PRESETS = {"imagenet": (data.IMAGENET_MEAN, data.IMAGENET_STD), "cifar": (data.CIFAR_MEAN, data.CIFAR_STD)}
WIDE = ((0.5, 0.5, 0.5), (1 / 32, 1 / 32, 1 / 32))      # a pixel range of [-16, 16] in the normalised input: no batch entry is clipped by it
_REFS, _ATTACKS = {}, {}

export_of, metric, accept = AR.export_of, PR.metric, PR.accept


def plain_labels(name):
    ex, x = export_of(name)
    return torch.arange(x.shape[0]) % ex["cfg"]["num_classes"]


def loss_grad_reference(name, loss, labels=None, num_labels=None, dtype=torch.float64):
    """``(eval logits, grad, loss)`` of ``reference_loss_grad`` on the float32 master weights; labels None: arange(B) % num_classes"""
    labels = plain_labels(name) if labels is None else torch.as_tensor(labels)
    key = (name, loss, tuple(labels.tolist()), num_labels, dtype)
    if key not in _REFS:
        ex, x = export_of(name)
        _REFS[key] = RB.reference_loss_grad(ex, x.to(dtype), labels, num_labels, loss)
    return _REFS[key]


def top_two(name):
    """``(top-1 label [B], float64 gap to the runner-up [B], the largest |logit|)`` of the float64 reference's eval logits"""
    logits = loss_grad_reference(name, "ce")[0]
    v, i = logits.topk(2, dim=1)
    return i[:, 0], v[:, 0] - v[:, 1], float(logits.abs().max())


def attack_reference(name, labels, **kw):
    key = (name, tuple(torch.as_tensor(labels).tolist()), tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _ATTACKS:
        ex, x = export_of(name)
        _ATTACKS[key] = RB.reference_attack(ex, x.double(), labels, **kw)
    return _ATTACKS[key]


# ---- uvc_loss_seed -------------------------------------------------------------------------------------------------------------------------
SEED_BATCHES = (1, 3, 65)
SEED_WIDTHS = ((1, 8), (2, 8), (10, 16), (100, 104), (1000, 1000), (1003, 1008))
SEED_KINDS = ("normal", "huge", "ties")


def seed_logits(B, n_valid, ld, kind, seed, dist):
    """``(lg, lgd or None, labels int32 [B])``: float32 [B, ld] with NaN in the padding columns.  normal: N(0, 3); huge: magnitude 3e4;
    ties: small integers, every third row all equal, and the maximum (and so the best other column) appearing more than once."""
    g = torch.Generator().manual_seed(seed)
    def draw():
        if kind == "huge":
            z = (torch.rand(B, ld, generator=g) * 2 - 1) * 3e4
        elif kind == "ties":
            z = torch.randint(-2, 3, (B, ld), generator=g).float()
            z[::3] = 1.5
        else:
            z = torch.randn(B, ld, generator=g) * 3.0
        z[:, n_valid:] = float("nan")
        return z
    lg = draw()
    lgd = draw() if dist else None
    y = torch.randint(0, n_valid, (B,), generator=g)
    if kind == "ties":
        y[::2] = 0
    return lg, lgd, y.to(torch.int32)


def seed_reference(lg, lgd, labels, n_valid, kind):
    """float64 on the float32 logits as given: ``(dz [B, ld], loss [B], p [B, ld] or None, max |z| [B])``; dz and p are zero in the padding"""
    z = lg.double()[:, :n_valid] if lgd is None else (lg.double()[:, :n_valid] + lgd.double()[:, :n_valid]) / 2
    B, ld = lg.shape
    y = labels.long()
    rows = torch.arange(B)
    dz = torch.zeros(B, ld, dtype=torch.float64)
    if kind == "ce":
        p = torch.zeros(B, ld, dtype=torch.float64)
        p[:, :n_valid] = torch.softmax(z, dim=1)
        dz[:] = p
        others = p.clone()
        others[rows, y] = 0
        dz[rows, y] = -others.sum(1)                                 # p_y - 1 without float64's own cancellation near p_y = 1
        return dz, torch.logsumexp(z, dim=1) - z[rows, y], p, z.abs().max(dim=1).values
    masked = z.clone()
    masked[rows, y] = -float("inf")
    j = masked.argmax(dim=1)                                         # torch's argmax: the first maximum
    dz[rows, j] = 1.0
    dz[rows, y] = -1.0
    return dz, z[rows, j] - z[rows, y], None, z.abs().max(dim=1).values


# ---- uvc_pgd_step --------------------------------------------------------------------------------------------------------------------------
STEP_P = (4, 8, 16)
STEP_ROWS = (1, 63, 64, 65, 1000)
SPECIALS = [0.0, -0.0, float("nan"), float("inf"), -float("inf"), 1e-40, -1e-40, 2.0 ** -149]


def step_operands(rows, P, seed, preset, eps255):
    """``(x, x0, dir, (eps, lo, hi))`` on the host: clean rows inside the preset's pixel range, an iterate around them (inside and outside the
    ball), a direction with zeros of both signs, NaN, infinities and denormals strewn in."""
    g = torch.Generator().manual_seed(seed)
    K0 = 3 * P * P
    eps, lo, hi = RB.linf_bounds(*PRESETS[preset], eps255)
    chan = torch.arange(K0) // (P * P)
    u = torch.rand(rows, K0, generator=g)
    x0 = lo[chan] + u * (hi[chan] - lo[chan])
    x = x0 + (torch.rand(rows, K0, generator=g) * 2 - 1) * 1.5 * max(float(eps.max()), 1e-3)
    d = torch.randn(rows, K0, generator=g) * 1e-3
    where = torch.randint(0, 4 * len(SPECIALS), (rows, K0), generator=g)
    for i, v in enumerate(SPECIALS):
        d[where == i] = v
    return x, x0, d, (eps, lo, hi)


def step_statement(x, x0, d, step, eps, lo, hi, P, mode):
    """the float32 PyTorch statement (include/uvc_kernels.h: uvc_pgd_step), every operation a float32 tensor operation"""
    chan = torch.arange(x.shape[1]) // (P * P)
    step, eps, lo, hi = (t.float()[chan][None] for t in (step, eps, lo, hi))
    if mode == 0:
        d = (d > 0).float() - (d < 0).float()
    return torch.minimum(torch.maximum(x + step * d, torch.maximum(x0 - eps, lo)), torch.minimum(x0 + eps, hi))


def same_or_both_nan(a, b):
    """bit equality, a NaN matching any NaN (the statement's NaN payload is not a property of the kernel)"""
    bits = torch.int32 if a.dtype == torch.float32 else torch.int16
    return a.dtype == b.dtype and bool(((a.view(bits) == b.view(bits)) | (torch.isnan(a) & torch.isnan(b))).all())

