"""What the pixel-attribution tests share (CPU and GPU; nothing here needs a GPU): the compact exports they run on, the float64 references
(computed once per case and left unchanged), the metric and the bars, and the float64 statements of the four kernels of
uvc_amd/csrc/input_grad.hip."""
import math

import torch

import attribution_ref as AR
from test_compact_cpu import dense_state
from uvc_amd import compact as CP
from uvc_amd import compact_pixel as PX

LOW_BARE = "low_bare"                          # blocks 0 and 1 keep no head, block 0 keeps no MLP unit either: the walk below the lowest attention block
NAMES = AR.FIXTURES + AR.EXTRA + [LOW_BARE]
BARS = {"fp32": 1e-3, "bf16": 2e-2}            # the project's model-level parity bars (tests/test_rollout_gpu.py: MODEL_BARS)
IG_STEPS = 8
_EXPORTS, _GRADS, _IGS = {}, {}, {}


def export_of(name):
    """attribution_ref.export_of plus "low_bare": ``(compact export, float32 batch on the host)``."""
    if name != LOW_BARE:
        return AR.export_of(name)
    if name not in _EXPORTS:
        c = AR.TINY
        masks = {"blocks.0.attn.proj.mask": torch.zeros(c.embed_dim, c.embed_dim), "blocks.0.mlp.fc2.mask": torch.zeros(c.embed_dim, c.hidden),
                 "blocks.1.attn.proj.mask": torch.zeros(c.embed_dim, c.embed_dim)}
        ex = CP.export_compact(dense_state(c, masks=masks))
        assert [(len(b["heads"]), b["hidden"]) for b in ex["blocks"]] == [(0, 0), (0, c.hidden), (c.num_heads, c.hidden)]
        _EXPORTS[name] = (ex, torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(11)))
    return _EXPORTS[name]


def metric(got, ref):
    """e = max |got - ref| / max |ref| over the batch"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max())


def _key(target):
    return None if target is None else tuple(int(v) for v in torch.as_tensor(target).reshape(-1).tolist())


def grad_reference(name, target=None):
    """``(float64 gradient on the float32 master weights, its target, its eval logits)``"""
    key = (name, _key(target))
    if key not in _GRADS:
        ex, x = export_of(name)
        _GRADS[key] = PX.reference_input_grad(ex, x.double(), target)
    return _GRADS[key]


def grad_e_ref(name, target):
    """the metric of the same reference run on the CPU with the batch and the weights cast to bfloat16 (a reference, not the code under test)"""
    ex, x = export_of(name)
    return metric(PX.reference_input_grad(ex, x.bfloat16(), target)[0], grad_reference(name, target)[0])


def ig_reference(name, target, baseline=None, dtype=torch.float64):
    key = (name, _key(target), None if baseline is None else tuple(baseline.tolist()), dtype)
    if key not in _IGS:
        ex, x = export_of(name)
        _IGS[key] = PX.reference_integrated_gradients(ex, x.to(dtype), target, None, None if baseline is None else baseline.to(dtype), IG_STEPS)
    return _IGS[key]


def accept(e, prec, e_ref_fn):
    """``(passes, the bar used, e_ref or None)``.  float32: 1e-3.  bf16: max(2e-2, 2 e_ref), tests/test_attribution_gpu.py's rule; ``e_ref_fn``
    is called only when 2e-2 alone does not decide (the rule's verdict does not depend on it then)."""
    if prec == "fp32":
        return e <= BARS["fp32"], BARS["fp32"], None
    if e <= BARS["bf16"]:
        return True, BARS["bf16"], None
    e_ref = e_ref_fn()
    bar = max(BARS["bf16"], 2 * e_ref)
    return e <= bar, bar, e_ref


# ---- the kernels, in float64 -----------------------------------------------------------------------------------------------------------------
def patchify_rule(x, P):
    """uvc_patchify's index rule on the host, any P: [B, C, S, S] -> [B * np, C * P * P], k = c P P + ky P + kx (a copy: exact)."""
    B, C, S, _ = x.shape
    g = S // P
    return x.reshape(B, C, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, C * P * P).contiguous()


def ulp(v, mantissa_bits):
    """the spacing of a format with ``mantissa_bits`` stored mantissa bits at |v| (float64 tensor); 0 at 0"""
    a = v.abs()
    e = torch.floor(torch.log2(a.clamp_min(1e-300)))
    return torch.where(a > 0, torch.exp2(e - mantissa_bits), torch.zeros_like(a))


def ig_rows_ref(x, x0, first, count, steps):
    """float64 [count * R, width] of the stored operands"""
    x = x.double()
    x0 = torch.zeros_like(x) if x0 is None else x0.double()
    return torch.cat([x0 + ((first + s + 0.5) / steps) * (x - x0) for s in range(count)])


def ig_rows_bound(x, x0, want, count, bf16):
    """2 float32 ulps of max(|x|, |x0|) per element; bf16: plus half a bf16 ulp of the result (rounded once)"""
    m = x.double().abs() if x0 is None else torch.maximum(x.double().abs(), x0.double().abs())
    b = (2 * ulp(m, 23)).repeat(count, 1)
    return b + 0.5 * ulp(want, 7) if bf16 else b


def sum_bound(n, abs_terms_sum):
    """the float32 summation bound of n terms: n 2^-24 sum |terms|"""
    return n * math.ldexp(1.0, -24) * abs_terms_sum


def pixel_terms(a, x, x0, scale):
    """the per-element terms of uvc_pixel_maps as the header states them, each in float32: a * scale, or (a * (x - x0)) * scale with the
    stored rows taken to float32 (exact)"""
    e = a.float()
    if x is not None:
        e = e * (x.float() - (0 if x0 is None else x0.float()))
    return (e * torch.tensor(scale, dtype=torch.float32)).double()


def pixel_maps_ref(e, B, C, S, P):
    """``(pixel [B, S, S], patch [B, np], total [B], sum |e| per image [B])`` in float64 from the terms [B * np, C * P * P]"""
    g = S // P
    img = e.reshape(B, g, g, C, P, P).permute(0, 3, 1, 4, 2, 5).reshape(B, C, S, S)
    pixel = img.abs().sum(1)
    patch = e.abs().sum(1).reshape(B, g * g)
    return pixel, patch, e.reshape(B, -1).sum(1), e.abs().reshape(B, -1).sum(1)
