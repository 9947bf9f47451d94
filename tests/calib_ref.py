"""What the calibration tests share (CPU and GPU; nothing here needs a GPU): the synthetic over-confident bank, the kernels' input cases with
their scales and shifts, the float64 objective through autograd, the margin and bin-edge rules, a float32 evaluator on the CPU and the
micro exports."""
import functools

import torch

import knn_ref as KR
from uvc_amd import compact_calibrate as CC
from uvc_amd import compact_probe as PB

ROWS = (1, 63, 64, 65, 1000, 4097)
# (C, ld): 16-byte rows and not; up to 4 / 256 / 1024 / 2048 classes (lanes per row, units per lane) and beyond (one workgroup per row)
WIDTHS = [(1, 8), (2, 8), (10, 16), (100, 104), (1000, 1000), (1003, 1008), (100, 102), (2500, 2501)]
MODES = [("temperature", False), ("temperature", True), ("vector", False), ("vector", True)]      # (scale of 1 or C values, with a shift)
MARGIN = 2.0 ** -20                                 # a first maximum is decided when it leads by more than this times max |z'|
EDGE = 1e-6                                         # a confidence is binned for certain farther than this from an interior bin edge
CAP = 0.01                                          # at most this fraction of rows may be undecided


def synthetic_bank(seed=0, n=4000, C=10, factor=2.5):
    """``(logits float32 [n, C], labels int64 [n])``: labels drawn from ``softmax(z)``, the logits then multiplied by ``factor`` -- a model
    that is over-confident by exactly that temperature."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, C, generator=g, dtype=torch.float64) * 2.0
    y = torch.multinomial(torch.softmax(z, dim=1), 1, generator=g)[:, 0]
    return (z * factor).float(), y


SEED = 0                                            # moves every case's generator: chosen so that the caps below hold for the whole grid


def case_seed(rows, C):
    return SEED * 100003 + rows * 7 + C


def case_inputs(rows, C, ld, kind, seed):
    """float32 [rows, ld] logits (the padding columns hold NaN: they must never be read into a result) and int64 labels with -1 and C among
    them.  normal: N(0, 3); huge: magnitude 3e4; ties: small integers, every third row all equal."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(rows, ld, generator=g) * 3.0
    if kind == "huge":
        z = (torch.rand(rows, ld, generator=g) * 2 - 1) * 3e4
    elif kind == "ties":
        z = torch.randint(-2, 3, (rows, ld), generator=g).float()
        z[::3] = 1.5
    z[:, C:] = float("nan")
    y = torch.randint(0, C, (rows,), generator=g)
    if kind == "ties":
        y[::2] = 0
    if rows >= 4:
        y[1], y[rows - 2] = -1, C
    return z, y


def case_maps(C, kind, seed):
    """``{mode: (scale float32 [1] or [C], shift float32 [C] or None)}``.  ties: one value for every class (exact in float32, so that equal
    logits stay equal after the map); otherwise scales in [0.5, 1.5] (huge: [0.9, 1.1]) and shifts N(0, 0.5)."""
    g = torch.Generator().manual_seed(seed + 77)
    if kind == "ties":
        a, d = torch.full((C,), 0.75), torch.full((C,), 0.25)
    else:
        lo, hi = (0.9, 1.1) if kind == "huge" else (0.5, 1.5)
        a, d = lo + (hi - lo) * torch.rand(C, generator=g), 0.5 * torch.randn(C, generator=g)
    return {("temperature", False): (a[:1].clone(), None), ("temperature", True): (a[:1].clone(), d), ("vector", False): (a, None), ("vector", True): (a, d)}


def mapped(z, y, scale, shift, C):
    """float64 ``z'`` of the counted rows and their labels"""
    _, zp, yk, _ = CC._mapped(z, y, scale, shift, C)
    return zp, yk


def hit_range(z, y, scale, shift, C):
    """``(lo, hi, undecided)`` around the float64 hits: a row is undecided when its first maximum leads the runner-up by more than 0 and at most
    ``MARGIN max |z'|`` (an exact tie is decided: the first maximum wins on both sides); it can hit only if its label is one of the two."""
    zp, yk = mapped(z, y, scale, shift, C)
    if C < 2 or not len(yk):
        h = int((zp.argmax(1) == yk).sum()) if len(yk) else 0
        return h, h, 0
    top = zp.topk(2, dim=1)
    lead = top.values[:, 0] - top.values[:, 1]
    amb = (lead > 0) & (lead <= MARGIN * float(zp.abs().max()))
    sure = int((~amb & (zp.argmax(1) == yk)).sum())
    return sure, sure + int((amb & (top.indices == yk[:, None]).any(1)).sum()), int(amb.sum())


def bin_ranges(z, y, scale, shift, C, bins):
    """``(count_lo, count_hi, hit_lo, hit_hi, undecided)`` per bin in float64: a row within ``EDGE`` of an INTERIOR edge j / bins may fall on
    either side of it (0 and 1 are no edges: the bin index is clamped), and the hit of a row ``hit_range`` calls undecided may go either way."""
    zp, yk = mapped(z, y, scale, shift, C)
    conf = torch.softmax(zp, dim=1).max(dim=1).values
    x = conf * bins
    j = torch.round(x)
    near = ((x - j).abs() <= EDGE * bins) & (j >= 1) & (j <= bins - 1)
    b = (torch.ceil(x).to(torch.int64) - 1).clamp(0, bins - 1)
    amb = torch.zeros_like(near)
    if C >= 2:
        top = zp.topk(2, dim=1).values
        amb = (top[:, 0] > top[:, 1]) & (top[:, 0] - top[:, 1] <= MARGIN * float(zp.abs().max()))
    hit = zp.argmax(1) == yk
    count = lambda mask: torch.bincount(b[mask], minlength=bins)
    jn = j[near].to(torch.int64)
    maybe = (torch.bincount(jn - 1, minlength=bins + 1) + torch.bincount(jn, minlength=bins + 1))[:bins]
    lo, hlo = count(~near), count(~near & ~amb & hit)
    return lo, lo + maybe, hlo, hlo + maybe + count(~near & amb), int((near | amb).sum())


def autograd_objective(z, y, scale, shift, C):
    """``(F, dscale, dshift)`` by autograd in float64 through ``F.cross_entropy(z * a + d, y)``, uncounted rows dropped beforehand."""
    keep = (y >= 0) & (y < C)
    a = torch.as_tensor(scale).detach().double().clone().requires_grad_()
    d = None if shift is None else torch.as_tensor(shift).detach().double().clone().requires_grad_()
    zp = z.double()[keep][:, :C] * a + (0 if d is None else d)
    F = torch.nn.functional.cross_entropy(zp, y[keep], reduction="mean")
    F.backward()
    return float(F.detach()), a.grad, None if d is None else d.grad


class Float32Evaluator:
    """``fit_calibration``'s evaluator on the CPU with float32 masters: the float64 objective, its value and gradient rounded to float32."""
    dtype, device = torch.float32, "cpu"

    def __call__(self, Z, y, scale, shift, classes):
        F, ds, dd, hits, m = CC.reference_objective(Z, y, scale, shift, classes)
        return float(torch.tensor(F).float()), ds.float(), None if dd is None else dd.float(), hits, m


@functools.lru_cache(maxsize=None)
def optimum(method):
    """``F*`` of the synthetic bank: the float64 solver asked for a gradient of 1e-10.  Vector scaling is not regularised and its Hessian is
    singular along ``d += const``; there the line search stops near 6e-9, where a step changes F by less than float64 resolves, so Newton
    steps on the gradient (the float64 Hessian by autograd, pseudo-inverse) take it the rest of the way: they need no difference of F."""
    Z, y = synthetic_bank()
    r = CC.fit_calibration(Z, y, 10, method, evaluator=CC.reference_objective, tol_grad=1e-10)
    if r["grad_inf"] > 1e-10 and method == "vector":
        z = Z.double()
        f = lambda t: torch.nn.functional.cross_entropy(z * t[:10] + t[10:], y)
        t = torch.cat([r["scale"], r["shift"]]).double()
        for _ in range(10):
            g = torch.autograd.functional.jacobian(f, t)
            if float(g.abs().max()) <= 1e-12:
                break
            t = t - torch.linalg.pinv(torch.autograd.functional.hessian(f, t), rcond=1e-10, hermitian=True) @ g
        F, ds, dd, hits, m = CC.reference_objective(Z, y, t[:10], t[10:], 10)
        r = dict(r, scale=t[:10].clone(), shift=t[10:].clone(), F=F, top1=100.0 * hits / m, grad_inf=max(float(ds.abs().max()), float(dd.abs().max())))
    assert r["grad_inf"] <= 1e-10, r["grad_inf"]
    return r


def micro_exports():
    """``{name: (export, batch, classes)}``: a plain file, a distilled one whose two heads differ, and a probed file with padding rows."""
    plain, xp = KR.export_of("stage2_micro_skip")
    deit, xd = KR.export_of("stage2_micro_deit")
    assert not torch.equal(deit["state_dict"]["head.weight"], deit["state_dict"]["head_dist.weight"])
    g = torch.Generator().manual_seed(3)
    D = deit["cfg"]["embed_dim"]
    probed = PB.probe_head(deit, torch.randn(10, D, generator=g, dtype=torch.float64) * 0.1, torch.randn(10, generator=g, dtype=torch.float64), 10)
    assert probed["cfg"]["num_classes"] == 16
    return {"plain": (plain, xp, plain["cfg"]["num_classes"]), "distilled": (deit, xd, deit["cfg"]["num_classes"]), "probed": (probed, xd, 10)}
