"""GPU: pixel attributions of compact models -- the four kernels of uvc_amd/csrc/input_grad.hip against float64 at every row width, grid
side and alignment, the engine entry point (uvc_vit_compact_input_grad) against ``compact_pixel.reference_input_grad`` in float64 on every
small export, integrated gradients against ``reference_integrated_gradients``, and ``python -m uvc_amd.compact_pixel`` end to end."""
import ctypes as C
import json

import numpy as np
import pytest
import torch
from PIL import Image

import pixel_attr_ref as PR
from oracle import vit as OV
from test_compact_cpu import dense_state
from uvc_amd import _lib as L
from uvc_amd import compact as CP
from uvc_amd import compact_perturb as PT
from uvc_amd import compact_pixel as PX
from uvc_amd import ops

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
GRIDS, BATCHES, CHUNKS = (1, 2, 3, 14), (1, 3), (1, 2, 5)


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(BITS[a.dtype]), b.view(BITS[b.dtype]))


def off_by_one(t):
    """a copy of ``t`` whose base pointer sits one element behind a 16-byte boundary"""
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = base[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size()
    return view


# ---- the kernels -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [2, 4, 16])
def test_unpatchify_is_the_inverse_of_patchify(P):
    """Bit for bit in float32, into a NaN-prefilled image.  The rows are uvc_patchify's where it takes the patch size (P % 4 == 0) and its
    index rule on the host at every P (as tests/test_image_patches_gpu.py checks P = 6); aligned and one element off."""
    g = torch.Generator().manual_seed(P)
    for side in GRIDS:
        for B in BATCHES:
            S = side * P
            x = torch.randn(B, 3, S, S, generator=g)
            rows = PR.patchify_rule(x, P).cuda()
            xd = x.cuda()
            if P % 4 == 0:
                made = torch.empty_like(rows)
                ops.patchify(xd, made, P, ops.UVC_F32)
                assert same_bits(made, rows)
                rows = made
            out = ops.unpatchify(rows, 3, S, P, out=torch.full((B, 3, S, S), float("nan"), device="cuda"))
            assert same_bits(out, xd), (side, B)
            base = torch.full((x.numel() + 1,), float("nan"), device="cuda")
            out = ops.unpatchify(off_by_one(rows), 3, S, P, out=base[1:].view(B, 3, S, S))
            assert same_bits(out, xd) and bool(torch.isnan(base[:1]).all()), (side, B)
    lib, st = L.lib(), L.cur_stream()
    assert lib.uvc_unpatchify(None, L.ptr(out), 1, 3, 8, 4, st) == 1 and lib.uvc_unpatchify(L.ptr(rows), L.ptr(out), 1, 3, 9, 4, st) == 1
    assert lib.uvc_unpatchify(L.ptr(rows), L.ptr(out), 0, 3, 8, 4, st) == 1


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("P", [2, 4, 16])
def test_ig_rows_against_float64(P, prec):
    """Within 2 float32 ulps of max(|x|, |x0|), in bf16 plus half a bf16 ulp of the result (it is rounded once); every element of the
    NaN-prefilled output is written.  Widths 12, 48, 768: 12 bf16 elements are 24 bytes a row, the element path; one element off too."""
    dt = DT[prec]
    g = torch.Generator().manual_seed(100 + P)
    width, worst = 3 * P * P, 0.0
    for side in GRIDS:
        for B in BATCHES:
            R = B * side * side
            x, x0 = torch.randn(R, width, generator=g).to(dt).cuda(), (2 * torch.randn(R, width, generator=g)).to(dt).cuda()
            for c in CHUNKS:
                for base, steps, first in ((None, c, 0), (x0, 2 * c + 3, 2)):
                    for shift in (False, True):
                        xs, bs = (off_by_one(x), None if base is None else off_by_one(base)) if shift else (x, base)
                        out = ops.ig_rows(xs, bs, first, c, steps, out=torch.full((c * R, width), float("nan"), dtype=dt, device="cuda"))
                        assert not torch.isnan(out).any()
                        want = PR.ig_rows_ref(x.cpu(), None if base is None else base.cpu(), first, c, steps)
                        err = (out.double().cpu() - want).abs()
                        bound = PR.ig_rows_bound(x.cpu(), None if base is None else base.cpu(), want, c, prec == "bf16")
                        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
                        assert bool((err <= bound).all()), (side, B, c, steps, shift, float((err / bound.clamp_min(1e-300)).max()))
    print(f"ig_rows {prec} P{P}: worst error / bound {worst:.3f}")
    lib, st = L.lib(), L.cur_stream()
    call = lambda **k: lib.uvc_ig_rows(*[{**dict(x=L.ptr(x), x0=None, out=L.ptr(out), nrows=1, width=width, first=0, count=1, steps=1,
                                                 dtype=int(prec == "bf16"), st=st), **k}[n] for n in ("x", "x0", "out", "nrows", "width", "first", "count", "steps", "dtype", "st")])
    assert call() == 0 and call(x=None) == 1 and call(out=None) == 1 and call(count=0) == 1 and call(steps=0) == 1 and call(first=-1) == 1
    assert call(first=1) == 1 and call(count=2) == 1 and call(dtype=2) == 1 and call(nrows=0) == 1 and call(width=0) == 1
    torch.cuda.synchronize()


@pytest.mark.parametrize("P", [2, 4, 16])
def test_ig_accumulate_against_float64(P):
    """Within n 2^-24 sum |terms| of the float64 sum, n the number of terms (count, plus the old value when it is kept); the same bits on a
    second call; one chain per element, so two calls of 2 and 3 steps give the bits of one call of 5."""
    g = torch.Generator().manual_seed(200 + P)
    width = 3 * P * P
    for side in GRIDS:
        for B in BATCHES:
            R = B * side * side
            for c in CHUNKS:
                d = torch.randn(c * R, width, generator=g).cuda()
                old = torch.randn(R, width, generator=g).cuda()
                for first in (True, False):
                    for shift in (False, True):
                        ds = off_by_one(d) if shift else d
                        acc = off_by_one(old) if shift else old.clone()
                        ops.ig_accumulate(ds, acc, first)
                        terms = d.double().view(c, R, width)
                        want = terms.sum(0) + (0 if first else old.double())
                        mag = terms.abs().sum(0) + (0 if first else old.double().abs())
                        n = c + (0 if first else 1)
                        assert bool(((acc.double() - want).abs() <= PR.sum_bound(n, mag)).all()), (side, B, c, first, shift)
                        again = old.clone()
                        ops.ig_accumulate(d, again, first)
                        assert same_bits(acc.contiguous(), again)
    d = torch.randn(5 * R, width, generator=g).cuda()
    one, two = torch.empty(R, width, device="cuda"), torch.empty(R, width, device="cuda")
    ops.ig_accumulate(d, one, True)
    ops.ig_accumulate(d[:2 * R], two, True)
    ops.ig_accumulate(d[2 * R:], two, False)
    assert same_bits(one, two)
    lib, st = L.lib(), L.cur_stream()
    assert lib.uvc_ig_accumulate(None, L.ptr(one), 4, 1, 1, st) == 1 and lib.uvc_ig_accumulate(L.ptr(d), None, 4, 1, 1, st) == 1
    assert lib.uvc_ig_accumulate(L.ptr(d), L.ptr(one), 0, 1, 1, st) == 1 and lib.uvc_ig_accumulate(L.ptr(d), L.ptr(one), 4, 0, 1, st) == 1


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("P", [2, 4, 16])
def test_pixel_maps_against_float64(P, prec):
    """The terms are the header's, each in float32 (a * scale, or (a * (x - x0)) * scale); every sum is held to n 2^-24 sum |terms| of the
    float64 sum of those terms -- n = C for a pixel, C P P for a patch, C P P np for an image's total.  The same bits on a second call."""
    dt = DT[prec]
    g = torch.Generator().manual_seed(300 + P)
    Cc, width = 3, 3 * P * P
    for side in GRIDS:
        for B in BATCHES:
            S, npatch = side * P, side * side
            a = torch.randn(B * npatch, width, generator=g).cuda()
            x, x0 = torch.randn(B * npatch, width, generator=g).to(dt).cuda(), torch.randn(B * npatch, width, generator=g).to(dt).cuda()
            for xs, bs, scale in ((None, None, 1.0), (x, x0, 1.0 / 7), (x, None, 3.0)):
                for shift in (False, True):
                    args = [off_by_one(t) if shift and t is not None else t for t in (a, xs, bs)]
                    pixel, patch, total = ops.pixel_maps(args[0], Cc, S, P, args[1], args[2], scale)
                    e = PR.pixel_terms(a.cpu(), None if xs is None else xs.cpu(), None if bs is None else bs.cpu(), scale)
                    w_pixel, w_patch, w_total, mag = PR.pixel_maps_ref(e, B, Cc, S, P)
                    assert bool(((pixel.double().cpu() - w_pixel).abs() <= PR.sum_bound(Cc, w_pixel)).all()), (side, B, shift)
                    assert bool(((patch.double().cpu() - w_patch).abs() <= PR.sum_bound(width, w_patch)).all()), (side, B, shift)
                    assert bool(((total.double().cpu() - w_total).abs() <= PR.sum_bound(width * npatch, mag)).all()), (side, B, shift)
                    again = ops.pixel_maps(args[0], Cc, S, P, args[1], args[2], scale)      # (the same call: the element path sums a row in another order)
                    assert all(same_bits(u, v) for u, v in zip((pixel, patch, total), again)), (side, B, shift)
    lib, st = L.lib(), L.cur_stream()
    out = torch.empty(B * S * S, device="cuda")
    call = lambda **k: lib.uvc_pixel_maps(*[{**dict(a=L.ptr(a), x=None, x0=None, scale=1.0, B=B, C=Cc, S=S, P=P, dtype=0, pixel=L.ptr(out), patch=None,
                                                    total=None, partial=None, st=st), **k}[n]
                                            for n in ("a", "x", "x0", "scale", "B", "C", "S", "P", "dtype", "pixel", "patch", "total", "partial", "st")])
    assert call() == 0 and call(a=None) == 1 and call(pixel=None) == 1 and call(x0=L.ptr(a)) == 1 and call(total=L.ptr(out)) == 1
    assert call(S=S + 1) == 1 and call(B=0) == 1 and call(dtype=2) == 1
    torch.cuda.synchronize()


# ---- the engine entry point and the module ---------------------------------------------------------------------------------------------
_MODELS = {}


def model_of(name, prec):
    if (name, prec) not in _MODELS:
        _MODELS[(name, prec)] = PX.CompactPixelViT(PR.export_of(name)[0], precision=prec)
    return _MODELS[(name, prec)]


def check_grad(name, prec, got, target, what):
    ref = PR.grad_reference(name, target)[0]
    e = PR.metric(got, ref)
    ok, bar, e_ref = PR.accept(e, prec, lambda: PR.grad_e_ref(name, target))
    print(f"input gradient {what} {name} {prec}: e {e:.2e} (bar {bar:.2e}" + (")" if e_ref is None else f", e_ref {e_ref:.2e})"))
    assert not torch.isnan(got).any() and ok, (name, prec, what, e, bar)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", PR.NAMES)
def test_input_gradient_against_the_float64_reference(name, prec):
    ex, x = PR.export_of(name)
    x = x.cuda()
    c = ex["cfg"]
    cm = model_of(name, prec)
    want_logits, _ = CP.CompactVisionTransformer(ex, precision=prec)(x)
    logits, grad, t = cm.input_grad(x)
    assert torch.equal(logits, want_logits) and torch.equal(cm(x)[0], want_logits)           # the eval forward's bits
    assert grad.dtype == torch.float32 and grad.shape == x.shape and t.dtype == torch.int64
    assert torch.equal(t, logits.argmax(1))                                                  # the forward's first top-1
    if prec == "fp32":
        assert torch.equal(t.cpu(), PR.grad_reference(name)[1])
    check_grad(name, prec, grad, t.cpu(), "top-1")
    # the same bits on a second call, from a given target equal to the argmax, and from the batch's patch rows
    _, grad2, t2 = cm.input_grad(x, target=t)
    assert same_bits(grad2, grad) and torch.equal(t2, t)
    rows = torch.empty(x.shape[0] * (c["img_size"] // c["patch_size"]) ** 2, c["in_chans"] * c["patch_size"] ** 2, dtype=DT[prec], device="cuda")
    ops.patchify(x, rows, c["patch_size"], cm._cfg.dtype)
    logits_p, grad_p, t_p = cm.input_grad(patches=rows)
    assert torch.equal(logits_p, logits) and same_bits(grad_p, grad) and torch.equal(t_p, t)
    # another class: another gradient, within the bar of its own reference; an int target, and the batch does not matter
    other = (t + 1) % c["num_classes"]
    _, grad_o, t_o = cm.input_grad(x, target=other.tolist())
    assert torch.equal(t_o, other) and float((grad_o - grad).abs().max()) > 0
    check_grad(name, prec, grad_o, other.cpu(), "other class")
    _, grad_i, t_i = cm.input_grad(x[:1], target=int(other[0]))
    assert same_bits(grad_i, grad_o[:1].contiguous()) and int(t_i[0]) == int(other[0])
    nl = max(1, int(t.min()))
    assert torch.equal(cm.input_grad(x, num_labels=nl)[2], logits[:, :nl].argmax(1))
    if name == "hard_gating":                   # the pixels of a patch the hard token mask zeroes get no gradient at all
        g = c["img_size"] // c["patch_size"]
        keep = torch.sigmoid(ex["state_dict"]["patch_gating"]).reshape(-1) >= 0.5
        keep[0] = True
        assert 0 < int(keep.sum()) < g * g
        blocks = grad.reshape(x.shape[0], 3, g, c["patch_size"], g, c["patch_size"]).permute(2, 4, 0, 1, 3, 5).reshape(g * g, -1)
        assert bool((blocks[~keep.cuda()] == 0).all()) and bool((blocks[keep.cuda()] != 0).any(dim=1).all())
    # saliency, gradient x input: the maps of the module are the kernel's sums of the gradient it returned
    pixel, patch, total = cm.pixel_maps(grad)
    assert tuple(pixel.shape) == (x.shape[0], c["img_size"], c["img_size"]) and tuple(patch.shape) == (x.shape[0], rows.shape[0] // x.shape[0])
    assert torch.allclose(pixel, grad.abs().sum(1), rtol=1e-5, atol=0) and torch.allclose(total, grad.sum((1, 2, 3)), rtol=0, atol=1e-5 * float(grad.abs().sum((1, 2, 3)).max()))
    gx = cm.pixel_maps(grad, x=x)[0]
    want_gx = (grad * rows_as_image(rows, c).float()).abs().sum(1)
    assert torch.allclose(gx, want_gx, rtol=1e-5, atol=1e-30)


def rows_as_image(rows, c):
    return ops.unpatchify(rows.float().contiguous(), c["in_chans"], c["img_size"], c["patch_size"])


def test_module_and_engine_refusals():
    ex, x = PR.export_of("no_heads")
    x = x.cuda()
    B, nc = x.shape[0], ex["cfg"]["num_classes"]
    cm = model_of("no_heads", "fp32")
    assert list(cm.parameters()) == []
    with pytest.raises(ValueError, match="one of x / patches"):
        cm.input_grad()
    with pytest.raises(ValueError, match="one of x / patches"):
        cm.input_grad(x, patches=torch.empty(B * 16, 192, device="cuda"))
    for bad in (-1, nc, [0, 1], [0, 1, nc], 1.5):
        with pytest.raises(ValueError):
            cm.input_grad(x, target=bad)
    with pytest.raises(ValueError):
        cm.input_grad(x, target=4, num_labels=4)
    for bad in (0, nc + 1):
        with pytest.raises(ValueError):
            cm.input_grad(x, num_labels=bad)
    for kw in (dict(steps=0), dict(chunk=0), dict(chunk=-1), dict(baseline=torch.zeros(4)), dict(target=nc)):
        with pytest.raises(ValueError):
            cm.integrated_gradients(x, **kw)
    with pytest.raises(TypeError, match="CompactPixelViT"):
        next(PX.explain_pixels(CP.CompactVisionTransformer(ex, precision="fp32"), []))
    # the entry point: 1 = UVC_ERR_ARG, 3 = UVC_ERR_UNSUPPORTED; nothing is launched
    cm.input_grad(x)                                            # sizes the workspace for this batch
    io, _ = cm._io(x, B, "input_grad")
    logits, ld = torch.empty(B, nc, device="cuda"), torch.empty(B, nc, device="cuda")
    io.logits, io.logits_dist = L.ptr(logits), L.ptr(ld)
    d_rows = torch.full((B * 16, 192), float("nan"), device="cuda")
    tout = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    call = lambda io, d, nl=nc, target=None: cm._lib_call("uvc_vit_compact_input_grad", C.byref(io), L.ptr(target), nl, L.ptr(d), L.ptr(tout), L.cur_stream())
    assert call(io, None) == 1 and call(io, d_rows, 0) == 1 and call(io, d_rows, nc + 1) == 1
    small, _ = cm._io(x, B, "attribution")                      # the attribution workspace is too small for an input gradient
    small.logits, small.logits_dist = L.ptr(logits), L.ptr(ld)
    assert small.workspace_bytes < io.workspace_bytes and call(small, d_rows) == 1
    nox, _ = cm._io(None, B, "input_grad")                      # neither x nor patch rows
    nox.logits, nox.logits_dist = L.ptr(logits), L.ptr(ld)
    assert call(nox, d_rows) == 1
    assert cm._lib_call("uvc_vit_compact_input_grad_workspace_bytes", 0) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(d_rows).all()) and tout.tolist() == [-7] * B
    wild = torch.tensor([-5, 3, 1 << 20], dtype=torch.int32, device="cuda")[:B]          # clamped by the kernel, as in the attribution entry
    assert call(io, d_rows, 8, wild) == 0
    torch.cuda.synchronize()
    assert tout.tolist() == [0, 3, 7][:B] and not torch.isnan(d_rows).any()
    cfg = OV.VitConfig(img_size=384, patch_size=16, num_classes=16, embed_dim=64, depth=2, num_heads=1, enable_dist=0)
    ex577 = CP.export_compact(dense_state(cfg))
    with pytest.raises(NotImplementedError, match="256"):
        PX.CompactPixelViT(ex577, precision="fp32")
    big = CP.CompactVisionTransformer(ex577, precision="fp32")
    lib = CP._bind()
    assert lib.uvc_vit_compact_input_grad_workspace_bytes(C.byref(big._cfg), big._blocks, big._nb, 2) == -1
    assert lib.uvc_vit_compact_input_grad(C.byref(big._cfg), big._blocks, big._nb, C.byref(io), None, nc, L.ptr(d_rows), None, L.cur_stream()) == 3
    assert b"256" in L.lib().uvc_last_error()
    torch.cuda.synchronize()


# ---- integrated gradients ----------------------------------------------------------------------------------------------------------------
COLOUR = torch.tensor([-0.5, 0.25, 1.0])


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", PR.NAMES)
def test_integrated_gradients_against_the_float64_reference(name, prec):
    """S = 8, the zero baseline and a colour.  The metric and bars of the input gradients; y and y_baseline are the two forwards' logits;
    the device's sum of IG is within the logit bar (1e-3 / 2e-2 of the largest logit, tests/test_compact_gpu.py's) of the reference's."""
    ex, x = PR.export_of(name)
    x = x.cuda()
    cm = model_of(name, prec)
    plain = cm(x)[0]
    for baseline in (None, COLOUR):
        logits, ig, t, y, y0 = cm.integrated_gradients(x, baseline=baseline, steps=PR.IG_STEPS)
        assert torch.equal(logits, plain) and torch.equal(t, plain.argmax(1)) and ig.dtype == torch.float32 and ig.shape == x.shape
        x0 = torch.zeros_like(x) if baseline is None else baseline.cuda().view(1, 3, 1, 1).expand_as(x).contiguous()
        assert torch.equal(y, plain.gather(1, t[:, None])[:, 0]) and torch.equal(y0, cm(x0)[0].gather(1, t[:, None])[:, 0])
        ref, _, ry, ry0 = PR.ig_reference(name, t.cpu(), baseline)
        e = PR.metric(ig, ref)
        ok, bar, e_ref = PR.accept(e, prec, lambda: PR.metric(PR.ig_reference(name, t.cpu(), baseline, torch.bfloat16)[0], ref))
        top = float(PR.grad_reference(name, t.cpu())[2].abs().max())
        gap = float((ig.double().sum((1, 2, 3)).cpu() - ref.sum((1, 2, 3))).abs().max())
        print(f"integrated gradients {name} {prec} baseline {'zero' if baseline is None else 'colour'}: e {e:.2e} (bar {bar:.2e}"
              + (")" if e_ref is None else f", e_ref {e_ref:.2e})") + f"; |sum IG - reference's| {gap:.2e} of largest logit {top:.2e}; "
              f"reference completeness gap {float((ref.sum((1, 2, 3)) - (ry - ry0)).abs().max()):.2e}")
        assert not torch.isnan(ig).any() and ok, (name, prec, e, bar)
        assert gap <= PR.BARS[prec] * top, (name, prec, gap, top)
        _, _, total = cm.pixel_maps(ig)
        assert float((total.double().cpu() - ig.double().sum((1, 2, 3)).cpu()).abs().max()) <= 1e-5 * float(ig.abs().sum((1, 2, 3)).max())
    # a given target, a whole-batch baseline, and the chunks: 1, 3 (ragged) and 8 steps a call agree within the float32 bar
    other = (t + 1) % ex["cfg"]["num_classes"]
    full = cm.integrated_gradients(x, other, baseline=x0, steps=PR.IG_STEPS, chunk=8)
    assert torch.equal(full[2], other)
    assert PR.accept(PR.metric(full[1], PR.ig_reference(name, other.cpu(), COLOUR)[0]), prec,
                     lambda: PR.metric(PR.ig_reference(name, other.cpu(), COLOUR, torch.bfloat16)[0], PR.ig_reference(name, other.cpu(), COLOUR)[0]))[0]
    for chunk in (1, 3):
        part = cm.integrated_gradients(x, other, baseline=COLOUR, steps=PR.IG_STEPS, chunk=chunk)
        e = PR.metric(part[1], full[1])
        print(f"integrated gradients {name} {prec}: chunk {chunk} against chunk 8: e {e:.2e}")
        assert e <= PR.BARS["fp32"] and torch.equal(part[3], full[3]) and torch.equal(part[4], full[4])


# ---- composition ---------------------------------------------------------------------------------------------------------------------------
def make_files(tmp_path):
    rng = np.random.default_rng(5)
    files = []
    for name, (h, w), mode in [("a.png", (31, 20), "RGB"), ("b.png", (64, 64), "L"), ("c.png", (45, 80), "RGBA")]:
        a = rng.integers(0, 256, (h, w) if mode == "L" else (h, w, len(mode)), dtype=np.uint8)
        Image.fromarray(a, mode).save(tmp_path / name)
        files.append(str(tmp_path / name))
    broken = tmp_path / "broken.png"
    broken.write_bytes(open(files[0], "rb").read()[:40])
    files.insert(2, str(broken))
    return files


def test_ig_maps_go_through_the_perturbation_test():
    ex, x = PR.export_of("no_heads")
    x = x.cuda()
    cm = model_of("no_heads", "fp32")
    logits, ig, t, y, y0 = cm.integrated_gradients(x, steps=PR.IG_STEPS)
    _, patch, total = cm.pixel_maps(ig)
    recs = [PX.record_of(str(b), [], int(t[b]), 4, patch[b].tolist(), (float(y[b]), float(y0[b]), float(total[b]))) for b in range(x.shape[0])]
    maps = torch.tensor([r["map"] for r in recs], device="cuda")
    assert torch.allclose(maps.sum(1), torch.ones(x.shape[0], device="cuda"), atol=1e-5)
    for order in PT.ORDERS:
        r = PT.perturbation_curves(cm, x, maps, t, order=order, steps=4)
        prob, hit = ops.logits_target(cm(x)[0], t.int(), None)
        assert r["counts"][0] == 0 and torch.equal(r["prob"][:, 0], prob) and torch.equal(r["hit"][:, 0], hit)      # nothing removed: the plain forward
        assert tuple(r["prob"].shape) == (x.shape[0], 4)
    for rec in recs:
        assert abs(rec["delta"] - (sum(ig[int(rec["file"])].double().flatten().tolist()) - (rec["y"] - rec["y_baseline"]))) <= 1e-4


def test_compact_pixel_command(tmp_path, capsys):
    ex, _ = PR.export_of("no_heads")
    model = tmp_path / "m.compact.pt"
    torch.save(ex, model)
    files = make_files(tmp_path)
    S, g = ex["cfg"]["img_size"], ex["cfg"]["img_size"] // ex["cfg"]["patch_size"]
    common = ["--compact", str(model), "--images", *files, "--batch_size", "3", "--precision", "fp32", "--num_workers", "2", "--topk", "3", "--num_labels", "10"]
    pred_out = tmp_path / "preds.jsonl"
    CP.main(["predict", *common, "--output", str(pred_out)])
    preds = [json.loads(l) for l in pred_out.read_text().splitlines()]
    maps = {}
    for method in PX.METHODS:
        out, odir, pdir = tmp_path / f"{method}.jsonl", tmp_path / f"ov_{method}", tmp_path / f"px_{method}"
        extra = ["--steps", "4", "--baseline", "black"] if method == "ig" else []
        summary = PX.main([*common, "--method", method, "--output", str(out), "--overlay_dir", str(odir), "--pixel_dir", str(pdir), *extra])
        lines = [json.loads(l) for l in out.read_text().splitlines()]
        assert len(lines) == 4 + 1 and lines[-1] == summary and summary["images"] == 4 and summary["errors"] == 1 and summary["batches"] == 2
        assert [r["file"] for r in lines[:-1]] == files and set(lines[2]) == {"file", "error"} and lines[2]["error"]
        keys = {"file", "top", "target", "grid", "map"} | ({"y", "y_baseline", "delta"} if method == "ig" else set())
        for i, (rec, pred) in enumerate(zip(lines[:-1], preds[:-1])):
            if i == 2:
                continue
            assert set(rec) == keys and rec["top"] == pred["top"] and rec["target"] == rec["top"][0]["index"] < 10
            assert rec["grid"] == [g, g] and len(rec["map"]) == g * g and min(rec["map"]) >= 0.0 and abs(sum(rec["map"]) - 1.0) <= 1e-5
            if method == "ig":
                assert all(np.isfinite(rec[k]) for k in ("y", "y_baseline", "delta"))
        names = ["0_a.png.png", "1_b.png.png", "3_c.png.png"]
        assert sorted(p.name for p in odir.iterdir()) == names and sorted(p.name for p in pdir.iterdir()) == names
        for p in names:
            im = Image.open(pdir / p)
            assert im.size == (S, S) and im.mode == "L" and int(np.asarray(im).max()) == 255 and Image.open(odir / p).size == (S, S)
        maps[method] = lines[0]["map"]
    assert maps["saliency"] != maps["gradxinput"] != maps["ig"]
    out_t = tmp_path / "t.jsonl"
    given = (preds[0]["top"][0]["index"] + 1) % 10
    PX.main([*common, "--method", "saliency", "--output", str(out_t), "--target", str(given)])
    lines_t = [json.loads(l) for l in out_t.read_text().splitlines()]
    assert all(r["target"] == given for r in lines_t[:-1] if "target" in r) and lines_t[0]["map"] != maps["saliency"]
    with pytest.raises(ValueError, match="target"):
        PX.main([*common, "--method", "saliency", "--target", "10"])
    capsys.readouterr()
