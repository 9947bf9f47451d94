"""What the attribution tests share (CPU and GPU; nothing here needs a GPU): the compact exports they run on, the host-drawn operands of the
relevance-step cases, the float64 statement of uvc_attention_relevance_step with two subtly wrong variants, and the acceptance rule."""
import torch

import scenarios as SC
from compact_train_ref import fixture_export
from oracle import vit as OV
from test_compact_cpu import dense_state
from uvc_amd import compact as CP

FIXTURES = ["stage2_micro_skip", "stage2_micro_deit", "stage2_micro_none", "stage2_tiny8"]
EXTRA = ["no_heads", "hard_gating", "px224"]
TINY = OV.VitConfig(img_size=32, patch_size=8, num_classes=16, embed_dim=192, depth=3, num_heads=3, enable_dist=1)
PX224 = OV.VitConfig(img_size=224, patch_size=16, num_classes=16, embed_dim=192, depth=3, num_heads=3, enable_dist=1)
_EXPORTS = {}


def export_of(name):
    """(compact export, float32 batch on the host), built once per name; the names of test_rollout_gpu.export_of plus "px224" (N = 198)."""
    if name in _EXPORTS:
        return _EXPORTS[name]
    g = torch.Generator().manual_seed(11)
    if name in FIXTURES:
        r, _, ex, _ = fixture_export(name)
        x = torch.from_numpy(SC.make_inputs(r)[0][0]).float()[:2]
    elif name == "hard_gating":
        sd = dense_state(TINY, patch_gating=1, masks=CP.synthetic_masks(TINY.depth, TINY.embed_dim, TINY.hidden, seed=1))
        sd["patch_gating"] = torch.linspace(-3, 3, sd["patch_gating"].numel()).reshape(sd["patch_gating"].shape)
        ex = CP.export_compact(sd)
        ex["cfg"]["patch_hard"] = 1
        assert ex["cfg"]["patch_gating"] == 1
        x = torch.randn(3, 3, 32, 32, generator=g)
    elif name == "no_heads":                   # the middle block keeps no head
        ex = CP.export_compact(dense_state(TINY, masks={"blocks.1.attn.proj.mask": torch.zeros(TINY.embed_dim, TINY.embed_dim)}))
        assert [len(b["heads"]) for b in ex["blocks"]] == [3, 0, 3]
        x = torch.randn(3, 3, 32, 32, generator=g)
    elif name == "px224":                      # N = 198, every value width below 64
        ex = CP.export_compact(dense_state(PX224, masks=CP.synthetic_masks(PX224.depth, PX224.embed_dim, PX224.hidden, seed=1)))
        assert [(len(b["heads"]), b["v_dim"]) for b in ex["blocks"]] == [(2, 48), (2, 32), (2, 16)] and CP._seq(ex["cfg"]) == 198
        x = torch.randn(2, 3, 224, 224, generator=g)
    else:
        raise KeyError(name)
    _EXPORTS[name] = (ex, x)
    return _EXPORTS[name]


# ---- the relevance step --------------------------------------------------------------------------------------------------------------
# (B, N, H, dv): at, and one past, every tile and block edge (64, 128, 256), every value width on a ragged N, and the streaming sizes
CASES = [(2, 1, 1, 64), (2, 5, 1, 16), (2, 64, 2, 32), (2, 65, 3, 48), (2, 128, 1, 64), (2, 129, 2, 48), (2, 197, 3, 64), (2, 198, 6, 32),
         (2, 257, 2, 16), (1, 577, 3, 16), (1, 1026, 2, 64)]
RTOL = 2e-4                                    # the project's float32 attention bar (tests/test_rollout_gpu.py)
FAMILY1_FLOOR = 1e-3                           # family 1: every reference entry is at least this, so its atol of 1e-9 is idle
# The offset of dout's seed from the family's.  dout decides the sign of dP, and at N = 1 an output entry is ONE max(0, p * dp): the constant was
# picked (from the float64 reference below, on the host) so that no family-1 entry of any case is clipped to zero, i.e. FAMILY1_FLOOR holds.
DOUT_SEED = 500004


def case_seed(which, N, H):
    return 1000 * which + N + H                # test_rollout_gpu's seeds


def family(which, B, N, H, dv, dt, seed):
    """test_rollout_gpu.family's draws, left on the host: ``(qkv, r_in)``.  1: unit-normal q, k, v and a near-uniform probability vector;
    2: k = q with rows of norm 16 (a query attends almost only to itself) and r_in = e_0."""
    g = torch.Generator().manual_seed(seed)
    if which == 1:
        qkv = torch.randn(B, N, H * (128 + dv), generator=g).to(dt)
        r_in = 1.0 + torch.rand(B, N, generator=g)
        return qkv, r_in / r_in.sum(1, keepdim=True)
    qkv = torch.randn(B, N, H * (128 + dv), generator=g)
    q = qkv[..., :H * 64].reshape(B, N, H, 64)
    q = (16.0 * q / q.norm(dim=-1, keepdim=True)).reshape(B, N, H * 64)
    qkv[..., :H * 64], qkv[..., H * 64:2 * H * 64] = q, q
    r_in = torch.zeros(B, N)
    r_in[:, 0] = 1.0
    return qkv.to(dt), r_in


def dout_of(B, N, H, dv, dt, seed):
    """unit-normal dO [B, N, H * dv] in the operand type, drawn on the host"""
    return torch.randn(B, N, H * dv, generator=torch.Generator().manual_seed(seed + DOUT_SEED)).to(dt)


def split(qkv, B, N, H, dv):
    x = qkv.double()
    q = x[..., :H * 64].reshape(B, N, H, 64).transpose(1, 2)
    k = x[..., H * 64:2 * H * 64].reshape(B, N, H, 64).transpose(1, 2)
    v = x[..., 2 * H * 64:].reshape(B, N, H, dv).transpose(1, 2)
    return q, k, v


def host_lse(qkv, B, N, H, dv):
    """float32 [B, H, N]: the log-sum-exp of the stored operands' scaled scores, as a forward would leave it"""
    q, k, _ = split(qkv, B, N, H, dv)
    return torch.logsumexp((q @ k.transpose(-2, -1)) * 0.125, dim=-1).float()


def step_ref(qkv, lse, dout, r_in, B, N, H, dv, keep, mix, variant="spec"):
    """float64 of the stored operands and of the lse the kernel reads (include/uvc_kernels.h: uvc_attention_relevance_step).  ``variant``:
    "spec"; "no_relu" (the gradient-weighted sum without the clip); "relu_after_mean" (the clip behind the head mean instead of per head)."""
    q, k, v = split(qkv.cpu(), B, N, H, dv)
    do = dout.cpu().double().reshape(B, N, H, dv).transpose(1, 2)
    p = torch.exp((q @ k.transpose(-2, -1)) * 0.125 - lse.cpu().double().unsqueeze(-1))          # [B, H, i, j]
    t = p * (do @ v.transpose(-2, -1))
    m = {"spec": lambda: t.clamp_min(0).sum(1), "no_relu": lambda: t.sum(1), "relu_after_mean": lambda: t.sum(1).clamp_min(0)}[variant]() / H
    r = r_in.cpu().double()
    return keep * r + mix * torch.einsum("bi,bij->bj", r, m)


def atol_of(which, want):
    """[B, 1]: family 1 1e-9 (idle: FAMILY1_FLOOR); family 2 (sharp attention, entries from 0 to a few units) 2e-5 of the image's maximum"""
    if which == 1:
        return torch.full((want.shape[0], 1), 1e-9, dtype=torch.float64)
    return 2e-5 * want.max(dim=1, keepdim=True).values


def accepted(got, want, which):
    """the acceptance rule of the step: |got - want| <= RTOL * |want| + atol, every entry"""
    return bool(((got.double().cpu() - want).abs() <= RTOL * want.abs() + atol_of(which, want)).all())


# ---- the model-level metric -------------------------------------------------------------------------------------------------------------
def map_errors(got, ref, ntok):
    """(e over the patch entries, e over the readout entries): max |got - ref| / max ref, each over its own entries"""
    got, ref = got.double().cpu(), ref.double().cpu()
    e = lambda a, b: float((a - b).abs().max() / b.max())
    return e(got[:, ntok:], ref[:, ntok:]), e(got[:, :ntok], ref[:, :ntok])
