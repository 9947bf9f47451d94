"""What the perturbation tests share (CPU and GPU; nothing here needs a GPU): the compact exports the curves run on, the host-made float32
maps that go to BOTH ``perturbation_curves`` and ``reference_perturbation`` (so the removed sets are identical and only the forward's
arithmetic differs), the float64 references (computed once per case and never changed), the bars and the fixture condition."""
import torch

import attribution_ref as AR
from oracle import vit as OV
from test_compact_cpu import dense_state
from uvc_amd import compact as CP
from uvc_amd import compact_perturb as PT

NAMES = AR.FIXTURES + AR.EXTRA                    # 17 - 198 tokens, with and without a distillation token, with head-less blocks
BIG = "px384"                                     # 577 tokens: above the attribution limit, `rollout` and `random` only
PX384 = OV.VitConfig(img_size=384, patch_size=16, num_classes=16, embed_dim=64, depth=2, num_heads=1, enable_dist=0)
KINDS = {**{n: ("attribution",) for n in NAMES}, BIG: ("rollout", "random")}
CASES = [(n, k) for n in NAMES + [BIG] for k in KINDS[n]]
GRIDS = (10, 7)                                   # 7 divides no fixture's patch count
# The bar tests/test_compact_gpu.py holds the eval logits to against reference_forward: max |got - ref| <= LOGIT_BAR * max |ref|.
LOGIT_BAR = {"fp32": 1e-3, "bf16": 2e-2}
# A softmax entry moves by at most half the largest logit error: |dp_t / dz_j| <= 1/4 for every j, |dp_t / dz_t| = sum_{j != t} |dp_t / dz_j|,
# so |sum_j dp_t/dz_j e_j| <= 2 * (p_t (1 - p_t)) * max |e| <= max |e| / 2.
PROB_FACTOR = 0.5
QUALIFY = 0.9                                     # the share of (image, step) pairs whose reference margin must exceed twice the logit bar
_EXPORTS, _MAPS, _REFS = {}, {}, {}


def export_of(name):
    """(compact export, float32 batch on the host) of a case, built once."""
    if name != BIG:
        return AR.export_of(name)
    if name not in _EXPORTS:
        ex = CP.export_compact(dense_state(PX384))
        assert CP._seq(ex["cfg"]) == 577
        _EXPORTS[name] = (ex, torch.randn(2, 3, 384, 384, generator=torch.Generator().manual_seed(12)))
    return _EXPORTS[name]


def num_labels_of(name):
    return min(10, export_of(name)[0]["cfg"]["num_classes"])


def maps_of(name, kind):
    """(float32 maps on the host, int64 targets): the float64 reference map of ``kind`` rounded to float32 ([B, N] over the tokens), or
    seeded uniform scores [B, np] for "random"; the target is the first top-1 label of the float64 reference on the intact image."""
    if (name, kind) not in _MAPS:
        ex, x = export_of(name)
        nl = num_labels_of(name)
        target = CP.reference_forward(ex, x.double())[:, :nl].argmax(dim=1)
        if kind == "random":
            g = ex["cfg"]["img_size"] // ex["cfg"]["patch_size"]
            maps = torch.rand(x.shape[0], g * g, generator=torch.Generator().manual_seed(13))
        elif kind == "attribution":
            maps = CP.reference_attribution(ex, x.double(), target, nl)[0].float()
        else:
            maps = CP.reference_rollout(ex, x.double(), kind).float()
        _MAPS[name, kind] = (maps, target)
    return _MAPS[name, kind]


def reference_of(name, kind, order, steps=10, counts=None):
    """``reference_perturbation`` in float64 on the host, computed once per case."""
    key = (name, kind, order, steps, None if counts is None else tuple(counts))
    if key not in _REFS:
        ex, x = export_of(name)
        maps, target = maps_of(name, kind)
        _REFS[key] = PT.reference_perturbation(ex, x.double(), maps, target, order=order, steps=steps, counts=counts, num_labels=num_labels_of(name))
    return _REFS[key]


def qualifying(ref, prec):
    """bool [B, K]: the (image, step) pairs at which ``hit`` may be compared across arithmetics -- the reference's margin (target logit minus
    the best other logit among the labels) exceeds twice the logit bar of that step's batch.  The margin counts by its size, whichever side
    leads: a target that lost by more than the bar is as safely a miss as one that leads by it is a hit, and in a deletion curve the target
    loses as the patches go (with the signed margin 10 - 30 % of a positive curve's pairs could ever qualify, whatever the head weights)."""
    return ref["margin"].abs() > 2 * LOGIT_BAR[prec] * ref["scale"][None, :]


def prob_bar(ref, prec):
    """[K]: what a probability may differ by from the reference's at each step"""
    return PROB_FACTOR * LOGIT_BAR[prec] * ref["scale"]
