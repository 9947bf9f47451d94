"""GPU: adversarial robustness of compact models -- uvc_loss_seed against float64 on the same float32 logits, uvc_pgd_step bit for bit against
the float32 PyTorch statement, the engine entry point (uvc_vit_compact_loss_grad) against ``compact_robust.reference_loss_grad`` in float64
on every small export, the properties of ``CompactRobustViT.attack``, and ``python -m uvc_amd.compact_robust`` end to end."""
import ctypes as C
import json

import pytest
import torch

import knn_ref as KR
import robust_ref as RR
from uvc_amd import _lib as L
from uvc_amd import compact_robust as RB
from uvc_amd import ops

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
SENTINEL = 768.0                                    # (exact in bfloat16)
NAN = float("nan")


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(BITS[a.dtype]), b.contiguous().view(BITS[b.dtype]))


def guarded(t, shift):
    """``(view, base)``: a copy of ``t`` inside a SENTINEL-filled buffer, 16 elements of guard on either side; the view starts on a 16-byte
    boundary, or with ``shift`` one element behind one"""
    base = torch.full((t.numel() + 32,), SENTINEL, dtype=t.dtype, device="cuda")
    start = 17 if shift else 16
    view = base[start:start + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == (t.element_size() if shift else 0)
    return view, base


def guards_intact(view, base, shift):
    start = 17 if shift else 16
    return bool((base[:start] == SENTINEL).all()) and bool((base[start + view.numel():] == SENTINEL).all())


# ---- uvc_loss_seed ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", [False, True], ids=["one_head", "two_heads"])
@pytest.mark.parametrize("kind", RR.SEED_KINDS)
def test_loss_seed_against_float64(kind, dist):
    """Cross-entropy: |dz - ref| <= 4 ulp32(max(p, 2^-24)), plus at the label column half a float32 spacing of the reference p - 1
    (tests/test_probe_gpu.py's bound for uvc_softmax_xent_grad); the loss within 1e-5 relative plus the float32 spacing of max |z|.  Margin: dz
    exact (j the first maximum over the other columns), the loss within the same bound.  With two heads dl = dld = dz / 2, exactly halved.
    +0 in the padding columns (which hold NaN on the way in), guard rows intact, a row alone gives its bits in the batch."""
    worst_g = worst_l = worst_o = 0.0
    for B in RR.SEED_BATCHES:
        for n_valid, ld in RR.SEED_WIDTHS:
            lg, lgd, y = RR.seed_logits(B, n_valid, ld, kind, seed=B * 13 + n_valid, dist=dist)
            lgc, lgdc, yc = lg.cuda(), None if lgd is None else lgd.cuda(), y.cuda()
            for loss in RB.LOSSES:
                if loss == "margin" and n_valid < 2:
                    continue
                bufs = [torch.full((B + 2, ld), SENTINEL, device="cuda") for _ in range(2)]
                dl, dld, got_loss = ops.loss_seed(lgc, yc, n_valid, loss, logits_dist=lgdc, dl=bufs[0][1:B + 1], dld=bufs[1][1:B + 1] if dist else None)
                ref_dz, ref_loss, p, zmax = RR.seed_reference(lg, lgd, y, n_valid, loss)
                assert not torch.isnan(dl).any() and not torch.isnan(got_loss).any(), (B, n_valid, loss)
                assert (dld is None) == (not dist) and (dld is None or same_bits(dl, dld))
                got = dl.double().cpu() * (2 if dist else 1)
                if loss == "ce":
                    lab = torch.zeros_like(p, dtype=torch.bool)
                    lab[torch.arange(B), y.long()] = True
                    tol = 4 * RR.ulp32(p.clamp_min(2.0 ** -24)) + lab * 0.5 * RR.ulp32(ref_dz)
                    ratio = float(((got - ref_dz).abs() / tol).max())
                    worst_g = max(worst_g, ratio)
                    worst_o = max(worst_o, float(((got - ref_dz).abs() / tol)[~lab].max()) if ld > 1 else 0.0)
                    assert ratio <= 1.0, (B, n_valid, ld, loss, ratio)
                else:
                    assert torch.equal(got, ref_dz), (B, n_valid, ld)
                bound = 1e-5 * ref_loss.abs() + RR.ulp32(zmax)
                err = (got_loss.double().cpu() - ref_loss).abs()
                worst_l = max(worst_l, float((err / bound).max()))
                assert bool((err <= bound).all()), (B, n_valid, ld, loss, float((err / bound).max()))
                assert not dl.view(torch.int32)[:, n_valid:].any()                                       # +0, not -0
                for buf in bufs[:2 if dist else 1]:
                    assert bool((buf[0] == SENTINEL).all()) and bool((buf[B + 1] == SENTINEL).all())
                assert bool((bufs[1] == SENTINEL).all()) or dist                                         # dld is not touched without lgd
                for r in {0, B - 1}:
                    one = ops.loss_seed(lgc[r:r + 1].contiguous(), yc[r:r + 1].contiguous(), n_valid, loss,
                                        logits_dist=None if lgdc is None else lgdc[r:r + 1].contiguous())
                    assert same_bits(one[0][0], dl[r]) and same_bits(one[2], got_loss[r:r + 1]), (B, n_valid, loss, r)
                again = ops.loss_seed(lgc, yc, n_valid, loss, logits_dist=lgdc)
                assert same_bits(again[0], dl.contiguous()) and same_bits(again[2], got_loss)
    print(f"uvc_loss_seed {kind} {'two heads' if dist else 'one head'}: worst dz error / bound {worst_g:.3f} ({worst_o:.3f} off the label column, "
          f"where half a spacing of p - 1 is most of the bound), worst loss error / bound {worst_l:.3f}")


def test_loss_seed_ties_and_clamped_labels():
    """j is the FIRST maximum over c != y: columns 2 and 5 tie for the best other logit; the label itself holds the row maximum, or ties
    with it.  A label outside [0, n_valid) is clamped by the kernel."""
    z = torch.tensor([[0.0, 1.0, 3.0, 4.0, -1.0, 3.0, 0.5, 9.0], [2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 9.0], [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 9.0]]).cuda()
    y = torch.tensor([3, 0, -4], dtype=torch.int32).cuda()
    dl, _, loss = ops.loss_seed(z, y, 7, "margin")
    want = torch.zeros(3, 8)
    want[0, 2], want[0, 3], want[1, 1], want[1, 0], want[2, 1], want[2, 0] = 1, -1, 1, -1, 1, -1
    assert torch.equal(dl.cpu(), want) and loss.tolist() == [-1.0, 0.0, -1.0]
    dl, _, _ = ops.loss_seed(z, torch.tensor([0, 50, 6], dtype=torch.int32).cuda(), 7, "margin")
    assert dl[0].tolist() == [-1, 0, 0, 1, 0, 0, 0, 0] and dl[1].tolist() == [1, 0, 0, 0, 0, 0, -1, 0] and dl[2].tolist() == [1, 0, 0, 0, 0, 0, -1, 0]


def test_loss_seed_refusals_leave_outputs_untouched():
    lg, lgd = torch.randn(4, 16, device="cuda"), torch.randn(4, 16, device="cuda")
    y = torch.zeros(4, dtype=torch.int32, device="cuda")
    dl, dld, loss = (torch.full(s, NAN, device="cuda") for s in ((4, 16), (4, 16), (4,)))
    lib, st = L.lib(), L.cur_stream()
    base = dict(lg=L.ptr(lg), lgd=L.ptr(lgd), y=L.ptr(y), B=4, ld=16, n=10, kind=0, dl=L.ptr(dl), dld=L.ptr(dld), loss=L.ptr(loss))
    call = lambda **k: lib.uvc_loss_seed(*[{**base, **k}[n] for n in ("lg", "lgd", "y", "B", "ld", "n", "kind", "dl", "dld", "loss")], st)
    for bad in (dict(lg=None), dict(y=None), dict(dl=None), dict(dld=None), dict(B=0), dict(B=-1), dict(n=0), dict(n=17), dict(kind=2), dict(kind=-1),
                dict(kind=1, n=1)):
        assert call(**bad) == 1, bad
        assert b"uvc_loss_seed" in lib.uvc_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(dl).all()) and bool(torch.isnan(dld).all()) and bool(torch.isnan(loss).all())
    assert call(loss=None) == 0 and call(lgd=None, dld=None, loss=None) == 0 and call(kind=1, n=2, loss=None) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss).all()) and not torch.isnan(dl).any()
    with pytest.raises(L.UvcHipError):
        ops.loss_seed(lg, y.long(), 10)
    with pytest.raises(L.UvcHipError):
        ops.loss_seed(lg, y, 10, "hinge")


# ---- uvc_pgd_step ----------------------------------------------------------------------------------------------------------------------
STEP_BOUNDS = (("imagenet", 4), ("cifar", 8), ("imagenet", 0))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("P", RR.STEP_P)
def test_pgd_step_is_the_float32_statement(P, prec):
    """K0 = 48, 192, 768; rows at and around a wave; every pointer on 16 bytes, and every pointer one element off; both modes; out a buffer
    of its own, and x itself; a direction holding zeros of both signs, NaN, infinities and denormals; the per-channel bounds of both presets,
    and eps = 0.  The float32 result has the bits of the PyTorch statement (a NaN -- mode 1 alone can make one -- matches a NaN), out_t is
    it rounded once to bfloat16 (float32: its bits), every number lies in [lo_c, hi_c] and within the rounded x0 +- eps_c, compared in
    float32, and nothing around the outputs is written."""
    dt = DT[prec]
    for rows in RR.STEP_ROWS:
        for preset, eps255 in STEP_BOUNDS:
            x, x0, d, (eps, lo, hi) = RR.step_operands(rows, P, rows * 3 + P + eps255, preset, eps255)
            chan = torch.arange(x.shape[1]) // (P * P)
            low, high = torch.maximum(x0 - eps[chan], lo[chan]), torch.minimum(x0 + eps[chan], hi[chan])
            for mode in (0, 1):
                step = -eps / 4 if (mode == 0 and rows % 2) else (eps / 4 if mode == 0 else eps)
                if mode == 0 and eps255 == 0:
                    step = RB.linf_bounds(*RR.PRESETS[preset], 2)[0]                # a real step against a ball of radius zero: x0 comes back
                want = RR.step_statement(x, x0, d, step, eps, lo, hi, P, mode)
                assert mode == 1 or not torch.isnan(want).any()
                for shift in (False, True):
                    for alias in (False, True):
                        (xv, xb), (x0v, _), (dv, _) = (guarded(t.cuda(), shift) for t in (x, x0, d))
                        ov, ob = (xv, xb) if alias else guarded(torch.full_like(x, NAN).cuda(), shift)
                        tv, tb = guarded(torch.full(x.shape, NAN, dtype=dt).cuda(), shift)
                        out = ops.pgd_step(xv, x0v, dv, P, step, eps, lo, hi, mode=mode, out=ov, out_t=tv)
                        case = (rows, preset, eps255, mode, shift, alias)
                        assert out.data_ptr() == ov.data_ptr() and RR.same_or_both_nan(out.cpu(), want), case
                        assert RR.same_or_both_nan(tv.cpu(), want.to(dt)), case
                        assert guards_intact(ov, ob, shift) and guards_intact(tv, tb, shift), case
                        if prec == "fp32":
                            assert RR.same_or_both_nan(tv, out), case
            got = out.cpu()
            ok = ~torch.isnan(got)
            assert bool(((got >= lo[chan]) & (got <= hi[chan]) & (got >= low) & (got <= high))[ok].all()), (rows, preset, eps255)
            if eps255 == 0:
                assert torch.equal(got[ok], x0[ok])
    torch.cuda.synchronize()


def test_pgd_step_without_out_t_and_refusals():
    x, x0, d, (eps, lo, hi) = RR.step_operands(5, 4, 1, "imagenet", 4)
    xc, x0c, dc = x.cuda(), x0.cuda(), d.cuda()
    assert torch.equal(ops.pgd_step(xc, x0c, dc, 4, eps, eps, lo, hi).cpu(), RR.step_statement(x, x0, d, eps, eps, lo, hi, 4, 0))
    out, out_t = torch.full_like(xc, NAN), torch.full_like(xc, NAN)
    lib, st = L.lib(), L.cur_stream()
    arr = lambda v: (C.c_float * len(v))(*[float(u) for u in v])
    base = dict(x=L.ptr(xc), x0=L.ptr(x0c), d=L.ptr(dc), rows=5, P=4, C=3, step=arr(eps), eps=arr(eps), lo=arr(lo), hi=arr(hi), mode=0, out=L.ptr(out),
                out_t=L.ptr(out_t), dtype=0)
    names = ("x", "x0", "d", "rows", "P", "C", "step", "eps", "lo", "hi", "mode", "out", "out_t", "dtype")
    call = lambda **k: lib.uvc_pgd_step(*[{**base, **k}[n] for n in names], st)
    for bad in (dict(x=None), dict(x0=None), dict(d=None), dict(out=None), dict(step=None), dict(eps=None), dict(lo=None), dict(hi=None), dict(rows=0),
                dict(P=0), dict(C=0), dict(C=5), dict(mode=2), dict(mode=-1), dict(dtype=2), dict(eps=arr([0.1, -0.1, 0.1])), dict(eps=arr([NAN] * 3)),
                dict(lo=arr(hi), hi=arr(lo)), dict(step=arr([NAN] * 3))):
        assert call(**bad) == 1, bad
        assert b"uvc_pgd_step" in lib.uvc_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(out_t).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert same_bits(out, out_t) and not torch.isnan(out).any()
    for kw in (dict(P=5), dict(out=torch.empty(5, 47, device="cuda")), dict(out_t=torch.empty(5, 48, dtype=torch.float16, device="cuda")), dict(step=[0.1, 0.1])):
        with pytest.raises(L.UvcHipError):
            ops.pgd_step(xc, x0c, dc, **{**dict(P=4, step=eps, eps=eps, lo=lo, hi=hi), **kw})


# ---- the engine entry point and the module ---------------------------------------------------------------------------------------------
_MODELS = {}


def model_of(name, prec):
    if (name, prec) not in _MODELS:
        _MODELS[(name, prec)] = RB.CompactRobustViT(RR.export_of(name)[0], precision=prec)
    return _MODELS[(name, prec)]


def logit_bar(prec, top):
    """twice the eval-logit bar of tests/test_compact_gpu.py (1e-3 / 2e-2 of the largest logit): lse and z_y each move by at most the logit error"""
    return 2 * RR.BARS[prec] * top


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", RR.NAMES)
def test_loss_gradient_against_the_float64_reference(name, prec):
    """Cross-entropy, labels arange(B) % num_classes: e = max |got - ref| / max |ref| over the batch within 1e-3 (float32) or
    max(2e-2, 2 e_ref) (bf16; e_ref: the reference run in bfloat16 on the CPU), tests/test_attribution_gpu.py's rule; the losses within twice
    the logit bar; the logits are forward's bits; patch rows, a repeat and an image alone give the same bits; the pixels of the patches a
    hard token mask zeroes get exactly zero; with num_labels below num_classes the padding logits have no share."""
    ex, x = RR.export_of(name)
    c = ex["cfg"]
    x = x.cuda()
    cm = model_of(name, prec)
    labels = RR.plain_labels(name)
    ref_logits, ref_grad, ref_loss = RR.loss_grad_reference(name, "ce")
    logits, grad, loss = cm.loss_grad(x, labels)
    assert torch.equal(logits, cm(x)[0]) and grad.dtype == torch.float32 and grad.shape == x.shape and loss.shape == (x.shape[0],)
    e = RR.metric(grad, ref_grad)
    ok, bar, e_ref = RR.accept(e, prec, lambda: RR.metric(RR.loss_grad_reference(name, "ce", dtype=torch.bfloat16)[1], ref_grad))
    gap, top = float((loss.double().cpu() - ref_loss).abs().max()), float(ref_logits.abs().max())
    print(f"loss gradient ce {name} {prec}: e {e:.2e} (bar {bar:.2e}" + (")" if e_ref is None else f", e_ref {e_ref:.2e})")
          + f"; |loss - ref| {gap:.2e} (bar {logit_bar(prec, top):.2e})")
    assert not torch.isnan(grad).any() and ok, (name, prec, e, bar)
    assert gap <= logit_bar(prec, top), (name, prec, gap)
    # the same bits: a repeat, the batch's patch rows, an image alone
    _, grad2, loss2 = cm.loss_grad(x, labels.tolist())
    assert same_bits(grad2, grad) and same_bits(loss2, loss)
    logits_p, grad_p, loss_p = cm.loss_grad(patches=cm._rows_of(x), labels=labels)
    assert torch.equal(logits_p, logits) and same_bits(grad_p, grad) and same_bits(loss_p, loss)
    _, grad_1, loss_1 = cm.loss_grad(x[-1:], labels[-1:])
    assert same_bits(grad_1, grad[-1:]) and same_bits(loss_1, loss[-1:])
    if name == "hard_gating":
        g = c["img_size"] // c["patch_size"]
        keep = torch.sigmoid(ex["state_dict"]["patch_gating"]).reshape(-1) >= 0.5
        keep[0] = True
        assert 0 < int(keep.sum()) < g * g
        blocks = grad.reshape(x.shape[0], 3, g, c["patch_size"], g, c["patch_size"]).permute(2, 4, 0, 1, 3, 5).reshape(g * g, -1)
        assert bool((blocks[~keep.cuda()] == 0).all()) and bool((blocks[keep.cuda()] != 0).any(dim=1).all())
    # fewer labels than the head has classes: the reference over those columns alone, and another gradient than the full head's
    nl = c["num_classes"] // 2
    _, grad_n, loss_n = cm.loss_grad(x, labels, nl)
    ref_n = RR.loss_grad_reference(name, "ce", num_labels=nl)
    e_n = RR.metric(grad_n, ref_n[1])
    assert RR.accept(e_n, prec, lambda: RR.metric(RR.loss_grad_reference(name, "ce", num_labels=nl, dtype=torch.bfloat16)[1], ref_n[1]))[0], (name, prec, e_n)
    assert float((loss_n.double().cpu() - ref_n[2]).abs().max()) <= logit_bar(prec, top) and bool((loss_n < loss).all())
    assert RR.metric(ref_n[1], ref_grad) > 2 * RR.BARS["bf16"]            # (the references: the upper half of the head carries a share of the full gradient)
    assert RR.metric(grad_n, ref_grad) > e_n                              # closer to its own reference than to the full head's


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_margin_gradient_against_the_float64_reference(prec):
    """The label is the reference's top-1, so j is the runner-up.  An image is left out when the float64 gap between the two is at most twice
    the logit bar (the device may then rank them the other way): float32 leaves out none of the images (16: the seven batches hold 2, 2, 2, 2, 3, 3
    and 2), bf16 at most 5.  The metric and the bars of the cross-entropy test, over the images kept."""
    left = total = 0
    for name in RR.NAMES:
        ex, x = RR.export_of(name)
        labels, gap, top = RR.top_two(name)
        keep = gap > logit_bar(prec, top)
        total += len(keep)
        left += int((~keep).sum())
        print(f"margin {name} {prec}: gaps {[round(float(v), 4) for v in gap]}, largest logit {top:.2f}, kept {keep.tolist()}")
        if not bool(keep.any()):
            continue
        cm = model_of(name, prec)
        logits, grad, loss = cm.loss_grad(x.cuda(), labels, loss="margin")
        assert torch.equal(logits, cm(x.cuda())[0])
        _, ref_grad, ref_loss = RR.loss_grad_reference(name, "margin", labels)
        e = RR.metric(grad[keep.cuda()], ref_grad[keep])
        ok, bar, e_ref = RR.accept(e, prec, lambda: RR.metric(RR.loss_grad_reference(name, "margin", labels, dtype=torch.bfloat16)[1][keep], ref_grad[keep]))
        err = float((loss.double().cpu() - ref_loss)[keep].abs().max())
        print(f"loss gradient margin {name} {prec}: e {e:.2e} (bar {bar:.2e}" + (")" if e_ref is None else f", e_ref {e_ref:.2e})")
              + f"; |loss - ref| {err:.2e} (bar {logit_bar(prec, top):.2e})")
        assert ok, (name, prec, e, bar)
        assert err <= logit_bar(prec, top) and bool((loss[keep.cuda()] < 0).all())
    assert total == 16 and left <= (0 if prec == "fp32" else 5), (prec, left)


@pytest.mark.parametrize("name", RR.NAMES)
def test_one_step_moves_along_the_reference_gradient_sign(name):
    """float32 only.  One step from the clean input, labels arange(B) % num_labels, in a pixel range wide enough to clip nothing:
    sign(x_adv - x) is the reference's gradient sign wherever |g_ref| > 2e-3 max |g_ref| of its image, exactly 0 where g_ref is exactly 0 (the
    gated patches, 43.75 % of hard_gating), and the entries in between are at most 5 % of the export's."""
    ex, x = RR.export_of(name)
    cm = model_of(name, "fp32")
    labels = RR.plain_labels(name)
    mean, std = RR.WIDE
    x_adv, info = cm.attack(x.cuda(), labels, eps=1, steps=1, mean=mean, std=std)
    g = RR.loss_grad_reference(name, "ce")[1]
    moved = torch.sign(x_adv.cpu().double() - x.double())
    big = g.abs() > 2e-3 * g.abs().amax(dim=(1, 2, 3), keepdim=True)
    zero = g == 0
    between = 1.0 - float((big | zero).double().mean())
    print(f"sign agreement {name}: {100 * between:.2f} % of the entries left out, {100 * float(zero.double().mean()):.2f} % exactly zero")
    assert torch.equal(moved[big], torch.sign(g)[big]) and not moved[zero].any()
    assert between <= 0.05, (name, between)
    if name == "hard_gating":
        assert float(zero.double().mean()) == 0.4375


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", RR.NAMES)
def test_attack_properties(name, prec):
    """PGD-3 at eps = 2 and FGSM at eps = 1 in the ImageNet preset, labels arange(B) % num_classes."""
    ex, x = RR.export_of(name)
    B, nc = x.shape[0], ex["cfg"]["num_classes"]
    xc = x.cuda()
    cm = model_of(name, prec)
    labels = RR.plain_labels(name)
    y32 = labels.int().cuda()
    mean, std = RR.PRESETS["imagenet"]
    kw = dict(mean=mean, std=std)
    eps_c, lo, hi = (t.cuda().view(1, 3, 1, 1) for t in RB.linf_bounds(mean, std, 2))
    alpha = RB.default_alpha(2, 3)
    x_adv, info = cm.attack(xc, labels, eps=2, steps=3, **kw)
    assert x_adv.dtype == torch.float32 and x_adv.shape == xc.shape and not torch.isnan(x_adv).any()
    assert info["loss"].shape == (4, B) and info["hit"].shape == (4, B) and info["hit"].dtype == torch.bool and info["robust"].shape == (B,)
    # inside the ball and the pixel range, in the rounded float32 bounds: the upper bounds hold everywhere; the lower ones wherever the clean
    # entry is itself a pixel value (the batches are unit-normal: 3 % of their entries lie outside the range, and further than eps)
    inside = (xc >= lo) & (xc <= hi)
    assert 0.9 < float(inside.float().mean()) < 1.0
    assert bool((x_adv <= torch.minimum(xc + eps_c, hi)).all()) and bool((x_adv >= torch.maximum(xc - eps_c, lo))[inside].all())
    assert bool((x_adv != xc)[inside].any())
    # the recorded losses and hits are loss_grad's and logits_target's bits at every iterate (the iterate k of PGD-3 is the result of PGD-k at the same step)
    for k in range(4):
        xk = cm.attack(xc, labels, eps=2, alpha=alpha, steps=k, **kw)[0]
        logits_k, _, loss_k = cm.loss_grad(xk, labels)
        assert same_bits(loss_k, info["loss"][k]), (name, prec, k)
        assert torch.equal(ops.logits_target(logits_k, y32, nc)[1].bool(), info["hit"][k]), (name, prec, k)
        if k == 0:
            assert torch.equal(xk, xc) and same_bits(loss_k, info["clean_loss"]) and torch.equal(info["hit"][0], info["clean_hit"])
        if k == 3:
            assert same_bits(xk, x_adv)
    assert torch.equal(info["robust"], info["hit"].all(0)) and bool((info["robust"] <= info["clean_hit"]).all())
    # two runs, and an image alone
    again, info2 = cm.attack(xc, labels, eps=2, steps=3, **kw)
    assert same_bits(again, x_adv) and same_bits(info2["loss"], info["loss"]) and torch.equal(info2["hit"], info["hit"])
    alone, info1 = cm.attack(xc[-1:], labels[-1:], eps=2, steps=3, **kw)
    assert same_bits(alone, x_adv[-1:]) and same_bits(info1["loss"], info["loss"][:, -1:]) and torch.equal(info1["hit"], info["hit"][:, -1:])
    # steps = 0, FGSM = PGD with one step of eps, a targeted step goes the other way wherever the pixel range clips neither
    same, info0 = cm.attack(xc, labels, eps=2, steps=0, **kw)
    assert same is not None and torch.equal(same, xc) and info0["loss"].shape == (1, B) and same_bits(info0["loss"][0], info["clean_loss"])
    fgsm, fi = cm.attack(xc, labels, eps=2, steps=1, **kw)
    pgd1, pi = cm.attack(xc, labels, eps=2, alpha=2, steps=1, **kw)
    assert same_bits(fgsm, pgd1) and same_bits(fi["loss"], pi["loss"])
    toward, ti = cm.attack(xc, labels, eps=2, steps=1, targeted=True, **kw)
    free = (xc - eps_c >= lo) & (xc + eps_c <= hi)
    assert torch.equal(torch.sign(fgsm - xc)[free], -torch.sign(toward - xc)[free]) and bool((fgsm != xc)[free].any())
    assert torch.equal(ti["robust"], ~ti["hit"].any(0))
    # the random start: the seed's draw, inside the bounds, the same bits on a repeat
    r1, ri1 = cm.attack(xc, labels, eps=2, steps=2, random_start=True, seed=5, **kw)
    r2, ri2 = cm.attack(xc, labels, eps=2, steps=2, random_start=True, seed=5, **kw)
    r3, _ = cm.attack(xc, labels, eps=2, steps=2, random_start=True, seed=6, **kw)
    assert same_bits(r1, r2) and same_bits(ri1["loss"], ri2["loss"]) and not same_bits(r1, r3) and not same_bits(ri1["loss"][0], ri1["clean_loss"])
    assert bool((r1 <= torch.minimum(xc + eps_c, hi)).all()) and bool((r1 >= torch.maximum(xc - eps_c, lo))[inside].all())
    # effectiveness: FGSM at eps = 1 raises the float64 reference's loss of the device's x_adv on every image (the reference attack itself raises
    # it by 0.23 - 2.1 on these exports, above twice the bf16 loss bar of 0.07)
    f1, _ = cm.attack(xc, labels, eps=1, steps=1, **kw)
    clean = RR.loss_grad_reference(name, "ce")[2]
    adv = RB.reference_loss_grad(ex, f1.cpu().double(), labels, None, "ce")[2]
    ref_rise = RR.attack_reference(name, labels, eps=1, steps=1, mean=mean, std=std)[1]["loss"]
    print(f"FGSM eps 1 {name} {prec}: reference loss {[round(float(v), 3) for v in clean]} -> {[round(float(v), 3) for v in adv]} "
          f"(the reference attack: {[round(float(v), 3) for v in ref_rise[1]]})")
    assert bool((adv > clean).all()), (name, prec)


def test_module_and_engine_refusals():
    ex, x = RR.export_of("no_heads")
    x = x.cuda()
    B, nc = x.shape[0], ex["cfg"]["num_classes"]
    cm = model_of("no_heads", "fp32")
    mean, std = RR.PRESETS["imagenet"]
    labels = [0, 1, 2]
    with pytest.raises(ValueError, match="one of x / patches"):
        cm.loss_grad(labels=labels)
    with pytest.raises(ValueError, match="labels"):
        cm.loss_grad(x)
    for bad in ([0, 1], [0, 1, nc], [-1, 0, 0], [0.5, 1.0, 2.0]):
        with pytest.raises(ValueError):
            cm.loss_grad(x, bad)
        with pytest.raises(ValueError):
            cm.attack(x, bad, eps=1, mean=mean, std=std)
    with pytest.raises(ValueError):
        cm.loss_grad(x, [0, 1, 4], num_labels=4)
    for kw in (dict(eps=-1), dict(eps=1, steps=-1), dict(eps=1, alpha=-1), dict(eps=1, loss="hinge"), dict(eps=1, loss="margin", num_labels=1),
               dict(eps=1, num_labels=nc + 1), dict(eps=1, mean=(0.5,), std=(0.5,))):
        with pytest.raises(ValueError):
            cm.attack(x, [0] * B, **{**dict(mean=mean, std=std), **kw})
    # the entry point: 1 = UVC_ERR_ARG; nothing is launched
    cm.loss_grad(x, labels)                                      # sizes the workspace for this batch
    io, _ = cm._io(x, B, "input_grad")
    logits, ld = torch.empty(B, nc, device="cuda"), torch.empty(B, nc, device="cuda")
    io.logits, io.logits_dist = L.ptr(logits), L.ptr(ld)
    d_rows = torch.full((B * 16, 192), NAN, device="cuda")
    loss = torch.full((B,), NAN, device="cuda")
    y = torch.tensor(labels, dtype=torch.int32, device="cuda")
    call = lambda io, d, nl=nc, kind=0, y=y: cm._lib_call("uvc_vit_compact_loss_grad", C.byref(io), L.ptr(y), nl, kind, L.ptr(d), L.ptr(loss), L.cur_stream())
    assert call(io, None) == 1 and call(io, d_rows, y=None) == 1 and call(io, d_rows, 0) == 1 and call(io, d_rows, nc + 1) == 1
    assert call(io, d_rows, kind=2) == 1 and call(io, d_rows, kind=-1) == 1 and call(io, d_rows, 1, 1) == 1
    assert b"margin" in L.lib().uvc_last_error()
    small, _ = cm._io(x, B, "attribution")                      # the attribution workspace is too small
    small.logits, small.logits_dist = L.ptr(logits), L.ptr(ld)
    assert small.workspace_bytes < io.workspace_bytes and call(small, d_rows) == 1
    nox, _ = cm._io(None, B, "input_grad")
    nox.logits, nox.logits_dist = L.ptr(logits), L.ptr(ld)
    assert call(nox, d_rows) == 1
    torch.cuda.synchronize()
    assert bool(torch.isnan(d_rows).all()) and bool(torch.isnan(loss).all())
    assert call(io, d_rows, 2, 1) == 0 and call(io, d_rows) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(d_rows).any() and not torch.isnan(loss).any()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
KEYS = {"images", "attack", "eps", "alpha", "steps", "loss", "labels", "clean_top1", "robust_top1", "mean_loss_clean", "mean_loss_adv", "img_per_s",
        "blocks", "params", "macs_compact"}


def test_command(tmp_path, capsys):
    """tests/test_knn_gpu.py's pattern: three flat-coloured classes through the CIFAR-10 reader, 12 test images."""
    ex, _ = KR.export_of("stage2_micro_deit")
    train, test = KR.colour_images(30, 1), KR.colour_images(12, 2)
    root = KR.write_cifar10(str(tmp_path / "data"), train, test)
    torch.save(ex, tmp_path / "f.pt")
    common = ["--compact", str(tmp_path / "f.pt"), "--dataset", "cifar10", "--data_dir", root, "--eval_batch_size", "8", "--num_workers", "2",
              "--precision", "fp32"]
    capsys.readouterr()
    line = RB.main([*common, "--attack", "fgsm", "--eps", "0"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == line and set(line) >= KEYS
    assert (line["images"], line["attack"], line["eps"], line["alpha"], line["steps"], line["loss"], line["labels"]) == (12, "fgsm", 0.0, 0.0, 1, "ce", "true")
    assert line["robust_top1"] == line["clean_top1"] and line["img_per_s"] > 0
    pgd = RB.main([*common, "--attack", "pgd", "--eps", "8", "--steps", "3"])
    assert (pgd["images"], pgd["attack"], pgd["eps"], pgd["steps"]) == (12, "pgd", 8.0, 3) and abs(pgd["alpha"] - 2.5 * 8 / 3) < 1e-12
    assert pgd["robust_top1"] <= pgd["clean_top1"] == line["clean_top1"] and pgd["mean_loss_adv"] >= pgd["mean_loss_clean"] == line["mean_loss_clean"]
    own = RB.main([*common, "--attack", "pgd", "--eps", "8", "--steps", "3", "--labels", "own", "--random_start", "1", "--loss", "margin", "--max_images", "10"])
    assert own["clean_top1"] == 100.0 and own["images"] == 10 and own["labels"] == "own" and own["robust_top1"] <= 100.0
    assert own["mean_loss_clean"] <= 0.0
    capsys.readouterr()
