"""GPU: the two kernels of uvc_amd/csrc/prune.hip through the C ABI with guarded buffers, ``CompactGateViT.gate_grads`` against
``reference_gate_grads`` and against the weight form of ``CompactTrainableViT``'s gradients, the paths it must leave alone, and the
commands end to end.

Every test prints the worst figure it measured before it asserts (README "Pruning a compact file further" records them).
"""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import attribution_ref as AR
import knn_ref as KR
import prune_ref as PF
from oracle import vit as OV
from test_compact_cpu import dense_state
from uvc_amd import _lib as L
from uvc_amd import compact as CP
from uvc_amd import compact_prune as PR
from uvc_amd import ops
from uvc_amd.compact_pixel import CompactPixelViT
from uvc_amd.compact_train import CompactTrainableViT

pytestmark = pytest.mark.gpu

SENT = 7.0
BN = [(1, 1), (2, 5), (3, 64), (2, 65), (2, 197), (2, 198), (1, 256)]
WG = [(16, 16), (16, 1), (64, 64), (96, 48), (144, 48), (192, 32), (80, 1), (448, 1), (3072, 1)]
DT = {"fp32": (torch.float32, ops.UVC_F32), "bf16": (torch.bfloat16, ops.UVC_BF16)}
BARS = {"fp32": 1e-3, "bf16": 2e-2}                         # the project's model-level parity bars (tests/test_compact_gpu.py)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int16) if t.dtype == torch.bfloat16 else t)


def run_dots(a, da, aux, B, N, width, group, dt, col0=2, tail=3, lddA=None):
    """one uvc_gate_dots call through the C ABI on [B * N, ld] device buffers: ``(rc, out [B, gates], dA or None, intact)``.  out sits at
    column col0 of a sentinel-filled [B + 2, col0 + gates + tail] buffer (rows 0 and B + 1 are guards), dA in a sentinel-filled buffer of
    leading dimension lddA"""
    gates = width // group
    full = torch.full((B + 2, col0 + gates + tail), SENT, device="cuda")
    out = full[1:B + 1]
    dA_full = None
    if aux is not None:
        lddA = width + 8 if lddA is None else lddA
        dA_full = torch.full((B * N + 2, lddA), SENT, dtype=a.dtype, device="cuda")
    dA = None if dA_full is None else dA_full[1:B * N + 1]
    rc = L.lib().uvc_gate_dots(L.ptr(a), a.stride(0), L.ptr(da), da.stride(0), L.ptr(aux), 0 if aux is None else aux.stride(0), L.ptr(dA),
                               0 if dA is None else dA.stride(0), B, N, width, group, L.ptr(out), full.stride(0), col0, dt, L.cur_stream())
    torch.cuda.synchronize()
    intact = bool((full[0] == SENT).all()) and bool((full[B + 1] == SENT).all()) and bool((out[:, :col0] == SENT).all()) and \
        bool((out[:, col0 + gates:] == SENT).all())
    if dA_full is not None:
        intact = intact and bool((dA_full[0] == SENT).all()) and bool((dA_full[-1] == SENT).all()) and bool((dA[:, width:] == SENT).all())
    return rc, out[:, col0:col0 + gates], (None if dA is None else dA[:, :width]), intact


# ---- uvc_gate_dots --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_gate_dots_against_float64(prec, fused):
    """Every (B, N) x (width, group) of the issue, operands in [B N, width + 24] buffers with NaN between the rows: |got - want| within
    1.01 2^-24 |want| + n 2^-52 sum |terms| of the float64 sums of the same operands; the fused form's dA is (dh * gp.float()).to(T) bit
    for bit; a repeat gives the same bits, a row alone the bits it has in the batch, and rows whose leading dimension or base pointer rules
    out 16-byte accesses give the same bits again; guards and the columns beside the gates stay as they were."""
    tdt, dt = DT[prec]
    worst = 0.0
    for B, N in BN:
        for width, group in WG:
            a, da, aux = PF.dots_case(B, N, width, width + 24, tdt, fused, seed=1000 * B + N + width + group)
            want, bar = PF.dots_ref(a, da, B, N, width, group)
            ac, dac, auxc = a.cuda(), da.cuda(), None if aux is None else aux.cuda()
            rc, out, dA, intact = run_dots(ac, dac, auxc, B, N, width, group, dt)
            assert rc == 0 and intact, (B, N, width, group)
            err = (out.double().cpu() - want).abs()
            worst = max(worst, float((err / bar).max()))
            assert bool((err <= bar).all()), (B, N, width, group, float((err / bar).max()))
            if fused:
                want_dA = (da[:, :width] * aux[:, :width].float()).to(tdt)
                assert torch.equal(bits(dA.cpu()), bits(want_dA)), (B, N, width, group)
            rc2, out2, dA2, intact2 = run_dots(ac, dac, auxc, B, N, width, group, dt, col0=0, tail=1)
            assert rc2 == 0 and intact2 and torch.equal(bits(out2), bits(out)) and (dA is None or torch.equal(bits(dA2), bits(dA)))
            # the last image alone
            r0 = (B - 1) * N
            rc3, out3, _, intact3 = run_dots(ac[r0:], dac[r0:], None if auxc is None else auxc[r0:], 1, N, width, group, dt)
            assert rc3 == 0 and intact3 and torch.equal(bits(out3), bits(out[B - 1:])), (B, N, width, group)
            if (B, N) in ((2, 5), (2, 198)):                 # element by element: a leading dimension off 16 bytes, then a base pointer off it
                odd = [None if t is None else torch.full((B * N, width + 3), float("nan"), dtype=t.dtype, device="cuda") for t in (ac, dac, auxc)]
                for o, t in zip(odd, (ac, dac, auxc)):
                    if o is not None:
                        o[:, :width] = t[:, :width]
                rc4, out4, dA4, intact4 = run_dots(odd[0], odd[1], odd[2], B, N, width, group, dt, lddA=width + 5)
                assert rc4 == 0 and intact4 and torch.equal(bits(out4), bits(out)) and (dA is None or torch.equal(bits(dA4), bits(dA)))
                flat = torch.empty(B * N * (width + 24) + 1, dtype=tdt, device="cuda")
                off = flat[1:].view(B * N, width + 24)
                off.copy_(ac)
                assert off.data_ptr() % 16 != 0
                rc5, out5, _, intact5 = run_dots(off, dac, auxc, B, N, width, group, dt)
                assert rc5 == 0 and intact5 and torch.equal(bits(out5), bits(out))
    print(f"uvc_gate_dots {prec} {'fused' if fused else 'plain'}: worst error / bar {worst:.3f} over {len(BN) * len(WG)} cases")


def test_gate_dots_refusals():
    B, N, width = 2, 5, 64
    for prec, fused in (("bf16", True), ("fp32", False)):
        tdt, dt = DT[prec]
        a, da, aux = (None if t is None else t.cuda() for t in PF.dots_case(B, N, width, width, tdt, fused, 3))
        good = dict(a=a, da=da, aux=aux, B=B, N=N, width=width, group=16, dt=dt)
        bad = [dict(group=8), dict(group=24), dict(group=48), dict(width=72), dict(width=0), dict(B=0), dict(N=0), dict(dt=2), dict(a=None), dict(da=None)]
        for kw in bad:
            args = {**good, **kw}
            full = torch.full((B + 2, 16), SENT, device="cuda")
            dA = torch.full((B * N, width), SENT, dtype=tdt, device="cuda") if fused else None
            rc = L.lib().uvc_gate_dots(L.ptr(args["a"]), width, L.ptr(args["da"]), width, L.ptr(aux), width if fused else 0, L.ptr(dA), width if fused else 0,
                                       args["B"], args["N"], args["width"], args["group"], L.ptr(full[1:]), 16, 0, args["dt"], L.cur_stream())
            torch.cuda.synchronize()
            assert rc == 1, kw
            assert bool((full == SENT).all()) and (dA is None or bool((dA == SENT).all())), kw
        out = torch.full((B, 16), SENT, device="cuda")
        call = lambda **kw: L.lib().uvc_gate_dots(L.ptr(a), kw.get("lda", width), L.ptr(da), width, L.ptr(kw.get("aux", aux)), width if fused else 0,
                                                  L.ptr(kw.get("dA")), width if fused else 0, B, N, width, 16, L.ptr(kw.get("out", out)), kw.get("ld_out", 16),
                                                  kw.get("col0", 0), dt, L.cur_stream())
        dA = torch.full((B * N, width), SENT, dtype=tdt, device="cuda") if fused else None
        assert call(dA=dA, out=None) == 1 and call(dA=dA, lda=width - 1) == 1 and call(dA=dA, ld_out=3) == 1 and call(dA=dA, col0=13) == 1 and call(dA=dA, col0=-1) == 1
        assert call(dA=None if fused else torch.empty(B * N, width, device="cuda")) == 1        # aux without dA / dA without aux
        torch.cuda.synchronize()
        assert bool((out == SENT).all()) and (dA is None or bool((dA == SENT).all()))
        assert call(dA=dA) == 0
    with pytest.raises(L.UvcHipError):
        ops.gate_dots(a, da, B, 24)
    with pytest.raises(L.UvcHipError):
        ops.gate_dots(a, da.bfloat16(), B, 16)
    got = ops.gate_dots(a, da, B, 16)
    want, bar = PF.dots_ref(a.cpu(), da.cpu(), B, N, width, 16)
    assert bool(((got.double().cpu() - want).abs() <= bar).all())
    torch.cuda.synchronize()


# ---- uvc_gate_accumulate ----------------------------------------------------------------------------------------------------------------
def test_gate_accumulate_chunks_and_float64_chain():
    B, G, ld = 24, 1003, 1008
    g = torch.Generator().manual_seed(2)
    s = torch.full((B, ld), float("nan"))
    s[:, :G] = torch.randn(B, G, generator=g) * torch.logspace(-6, 3, G)
    s[3, 5], s[7, 9] = 0.0, -0.0
    sq, ab = torch.zeros(G, dtype=torch.float64), torch.zeros(G, dtype=torch.float64)
    for b in range(B):
        v = s[b, :G].double()
        sq += v * v
        ab += v.abs()
    sc = s.cuda()
    results = []
    for chunk in (B, 1, 3, 8):
        full = torch.full((2, G + 8), SENT, dtype=torch.float64, device="cuda")
        full[:, 4:4 + G] = 0
        for b0 in range(0, B, chunk):
            rc = L.lib().uvc_gate_accumulate(L.ptr(sc[b0:]), ld, min(chunk, B - b0), G, L.ptr(full[0, 4:]), L.ptr(full[1, 4:]), L.cur_stream())
            assert rc == 0
        torch.cuda.synchronize()
        assert bool((full[:, :4] == SENT).all()) and bool((full[:, 4 + G:] == SENT).all())
        results.append(full[:, 4:4 + G].cpu())
    for r in results:
        assert torch.equal(r[0], sq) and torch.equal(r[1], ab)
    one = torch.zeros(G, dtype=torch.float64, device="cuda")
    for args in ((None, ld, B, G, one, one), (sc, ld, 0, G, one, one), (sc, ld, B, 0, one, one), (sc, G - 1, B, G, one, one), (sc, ld, B, G, None, one),
                 (sc, ld, B, G, one, None)):
        assert L.lib().uvc_gate_accumulate(L.ptr(args[0]), args[1], args[2], args[3], L.ptr(args[4]), L.ptr(args[5]), L.cur_stream()) == 1
    torch.cuda.synchronize()
    assert not bool(one.any())
    with pytest.raises(L.UvcHipError):
        ops.gate_accumulate(sc[:, :G], one.float(), one)
    a, b2 = ops.gate_accumulate(sc[:, :G], torch.zeros_like(one), torch.zeros_like(one))
    assert torch.equal(a.cpu(), sq) and torch.equal(b2.cpu(), ab)


# ---- the engine entry point and the module ---------------------------------------------------------------------------------------------
_MODELS, _REFS = {}, {}


def model_of(name, prec):
    if (name, prec) not in _MODELS:
        _MODELS[(name, prec)] = PR.CompactGateViT(AR.export_of(name)[0], precision=prec)
    return _MODELS[(name, prec)]


def reference_of(name, dtype=torch.float64):
    """``(eval logits, loss, s)`` of ``reference_gate_grads`` on the float32 master weights, computed once and left unchanged"""
    if (name, dtype) not in _REFS:
        ex, x = AR.export_of(name)
        y, nl = PF.labels_of(x.shape[0], ex["cfg"]["num_classes"])
        _REFS[(name, dtype)] = PR.reference_gate_grads(ex, x.to(dtype), y, nl)
    return _REFS[(name, dtype)]


def raw_gate_grads(module, x, y, nl):
    """uvc_vit_compact_gate_grads through the C ABI on any compact module with the training shadows: ``(rc, logits, gates [B, G] with the
    padding columns, loss, intact)``, gates and loss in sentinel-guarded buffers"""
    ex = module._export
    B, nc = x.shape[0], ex["cfg"]["num_classes"]
    G = PR._columns(ex)[0]
    module._refresh_shadows()
    io, mask = module._io(x, B, "gate_grads")
    logits, ld = torch.empty(B, nc, device="cuda"), torch.empty(B, nc, device="cuda")
    io.logits, io.logits_dist = L.ptr(logits), L.ptr(ld)
    full = torch.full((B + 2, G), SENT, device="cuda")
    loss = torch.full((B + 2,), SENT, device="cuda")
    yc = torch.tensor(y, dtype=torch.int32, device="cuda")
    rc = module._lib_call("uvc_vit_compact_gate_grads", C.byref(io), L.ptr(yc), nl, L.ptr(full[1:]), L.ptr(loss[1:]), L.cur_stream())
    torch.cuda.synchronize()
    intact = bool((full[0] == SENT).all()) and bool((full[B + 1] == SENT).all()) and float(loss[0]) == SENT and float(loss[B + 1]) == SENT
    z = logits if module.num_tokens == 1 else (logits + ld) / 2
    return rc, z, full[1:B + 1], loss[1:B + 1], intact


def split_metric(ex, got, ref):
    """(e over the head columns, e over the unit columns): max |got - ref| / max |ref|, each over its own columns (None where there are none)"""
    kind = torch.tensor([t[0] for t in PR.gate_table(ex)])
    got, ref = got.double().cpu(), ref.double().cpu()
    e = lambda m: float((got[:, m] - ref[:, m]).abs().max() / ref[:, m].abs().max()) if bool(m.any()) else None
    return e(kind == 0), e(kind == 1)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", PF.EXPORTS)
def test_gate_grads_against_the_float64_reference(name, prec):
    """e = max |got - ref| / max |ref| over the head columns and, apart, over the unit columns: 1e-3 in float32, max(2e-2, 2 e_ref) in bf16
    (e_ref: the same reference in bfloat16 on the CPU; tests/test_attribution_gpu.py's rule).  The logits are forward's bits, the loss is
    within twice the eval-logit bar (tests/test_robust_gpu.py), the padding columns are exact zeros, a repeat and an image alone give the same
    bits."""
    ex, x = AR.export_of(name)
    y, nl = PF.labels_of(x.shape[0], ex["cfg"]["num_classes"])
    x = x.cuda()
    cm = model_of(name, prec)
    ref_logits, ref_loss, ref = reference_of(name)
    logits, loss, s = cm.gate_grads(x, y, nl)
    table = PR.gate_table(ex)
    assert s.dtype == torch.float32 and tuple(s.shape) == (x.shape[0], len(table)) and tuple(loss.shape) == (x.shape[0],)
    assert torch.equal(logits, CP.CompactVisionTransformer(ex, precision=prec)(x)[0]) and torch.equal(logits, cm(x)[0])
    assert not torch.isnan(s).any()
    eh, eu = split_metric(ex, s, ref)
    low = None
    report = []
    for what, e, pick in (("heads", eh, 0), ("units", eu, 1)):
        if e is None:
            continue
        bar, e_ref = BARS[prec], None
        if prec == "bf16" and e > bar:
            low = reference_of(name, torch.bfloat16)[2] if low is None else low
            e_ref = split_metric(ex, low, ref)[pick]
            bar = max(bar, 2 * e_ref)
        report.append(f"{what} e {e:.2e} (bar {bar:.2e}" + (")" if e_ref is None else f", e_ref {e_ref:.2e})"))
        assert e <= bar, (name, prec, what, e, bar)
    top = float(ref_logits.abs().max())
    gap = float((loss.double().cpu() - ref_loss).abs().max())
    print(f"gate_grads {name} {prec}: " + "; ".join(report) + f"; |loss - ref| {gap:.2e} (bar {2 * BARS[prec] * top:.2e})")
    assert gap <= 2 * BARS[prec] * top
    # the engine's own row: padding columns exact zeros, guards intact, the module's columns are its real ones
    rc, z, full, loss_raw, intact = raw_gate_grads(cm, x, y, nl)
    G, real, pad = PR._columns(ex)
    assert rc == 0 and intact and torch.equal(z, logits) and torch.equal(bits(loss_raw), bits(loss))
    assert not bool(full[:, pad].any()) and torch.equal(bits(full[:, real].contiguous()), bits(s))
    if name == "no_heads":
        assert not [t for t in table if t[:2] == (0, 1)] and len([t for t in table if t[0] == 0]) == 6
    # the same bits on a repeat and for an image alone
    _, loss2, s2 = cm.gate_grads(x, torch.tensor(y), nl)
    assert torch.equal(bits(s2), bits(s)) and torch.equal(bits(loss2), bits(loss))
    _, loss1, s1 = cm.gate_grads(x[-1:], y[-1:], nl)
    assert torch.equal(bits(s1), bits(s[-1:])) and torch.equal(bits(loss1), bits(loss[-1:]))


@pytest.mark.parametrize("name", PF.EXPORTS)
def test_batch_sums_equal_the_weight_form_of_the_training_backward(name):
    """Two device paths, float32: sum_b s[b, .] against sum_d W[d, cols] dW[d, cols] of ``CompactTrainableViT``'s gradient buffer after a
    backward seeded with the same per-image dz.  2e-3 of the largest entry: each side is within 1e-3 of float64."""
    ex, x = AR.export_of(name)
    y, nl = PF.labels_of(x.shape[0], ex["cfg"]["num_classes"])
    x = x.cuda()
    s = model_of(name, "fp32").gate_grads(x, y, nl)[2].double().sum(0).cpu()
    tm = CompactTrainableViT(ex, precision="fp32")
    o, od = tm._train_forward(tm._prep(x))
    dl, dld, _ = ops.loss_seed(o, torch.tensor(y, dtype=torch.int32, device="cuda"), nl, "ce", logits_dist=od)
    tm._train_backward(dl, dld)
    torch.cuda.synchronize()
    want = []
    for k, b in enumerate(ex["blocks"]):
        for n, cols, group in ((f"blocks.{k}.attn.proj.weight", len(b["heads"]), b["v_dim"]), (f"blocks.{k}.mlp.fc2.weight", len(b["hidden_index"]), 1)):
            w = tm._by_name[n].detach()
            if cols == 0:
                continue
            off = tm._offset(n)
            g = tm._flat_grad[off:off + w.numel()].view(w.shape)
            want.append((w.double() * g.double()).sum(0)[:cols * group].reshape(cols, group).sum(1).cpu())
    want = torch.cat(want)
    e = float((s - want).abs().max() / want.abs().max())
    print(f"gate sums against the weight form {name}: {e:.2e} of the largest entry {float(want.abs().max()):.2e} (bar 2e-3)")
    assert e <= 2e-3


def test_the_other_walks_are_what_they_were():
    """The training backward, the attribution and the input gradient give the same bits before and after gate_grads calls on the same module
    (and on the same workspace family): the gate mode is one more argument of the walk they share."""
    name = "stage2_micro_deit"
    ex, x = AR.export_of(name)
    y, nl = PF.labels_of(x.shape[0], ex["cfg"]["num_classes"])
    x = x.cuda()
    yc = torch.tensor(y, dtype=torch.int32, device="cuda")
    for prec in ("fp32", "bf16"):
        gate, pix, tm = model_of(name, prec), CompactPixelViT(ex, precision=prec), CompactTrainableViT(ex, precision=prec)

        def train_grads():
            o, od = tm._train_forward(tm._prep(x))
            dl, dld, _ = ops.loss_seed(o, yc, nl, "ce", logits_dist=od)
            tm._flat_grad.fill_(float("nan"))
            tm._train_backward(dl, dld)
            return tm._flat_grad[:tm._off.n_main].clone()

        before = (train_grads(), gate.attribution(x, y, nl)[1], pix.input_grad(x, y, nl)[1], pix.attribution(x, y, nl)[1])
        for m in (gate, pix, tm):
            rc, _, full, _, intact = raw_gate_grads(m, x, y, nl)
            assert rc == 0 and intact
        assert torch.equal(bits(full), bits(raw_gate_grads(gate, x, y, nl)[2]))                 # every module class gives the same row
        after = (train_grads(), gate.attribution(x, y, nl)[1], pix.input_grad(x, y, nl)[1], pix.attribution(x, y, nl)[1])
        for a, b in zip(before, after):
            assert not torch.isnan(a).any() and torch.equal(bits(a), bits(b)), prec
    torch.cuda.synchronize()


def test_engine_and_module_refusals():
    ex, x = AR.export_of("no_heads")
    y, nl = PF.labels_of(x.shape[0], ex["cfg"]["num_classes"])
    x = x.cuda()
    B, nc = x.shape[0], ex["cfg"]["num_classes"]
    cm = model_of("no_heads", "fp32")
    cm.gate_grads(x, y, nl)                                     # sizes the workspace for this batch
    io, _ = cm._io(x, B, "gate_grads")
    logits, ld = torch.empty(B, nc, device="cuda"), torch.empty(B, nc, device="cuda")
    io.logits, io.logits_dist = L.ptr(logits), L.ptr(ld)
    G = PR._columns(ex)[0]
    gates, loss = torch.full((B, G), float("nan"), device="cuda"), torch.full((B,), float("nan"), device="cuda")
    yc = torch.tensor(y, dtype=torch.int32, device="cuda")
    call = lambda io, gates, nl=nl, labels=yc: cm._lib_call("uvc_vit_compact_gate_grads", C.byref(io), L.ptr(labels), nl, L.ptr(gates), L.ptr(loss), L.cur_stream())
    assert call(io, None) == 1 and call(io, gates, labels=None) == 1
    assert call(io, gates, 0) == 1 and call(io, gates, nc + 1) == 1
    small, _ = cm._io(x, B, "attribution")                      # another mode's workspace is too small
    small.logits, small.logits_dist = L.ptr(logits), L.ptr(ld)
    assert small.workspace_bytes < io.workspace_bytes and call(small, gates) == 1
    io.accumulate = 1.0
    assert call(io, gates) == 3
    io.accumulate = 0.0
    io.logits = None
    assert call(io, gates) == 1
    io.logits = L.ptr(logits)
    assert cm._lib_call("uvc_vit_compact_gate_grads_workspace_bytes", 0) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(gates).all()) and bool(torch.isnan(loss).all())        # nothing ran
    # labels outside [0, num_labels) are clamped by the kernel (the Python layer refuses them before)
    wild = torch.tensor([-5, 3, 1 << 20], dtype=torch.int32, device="cuda")[:B]
    assert call(io, gates, 8, wild) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(gates).any() and not torch.isnan(loss).any()
    for bad in ([0, nl], [-1, 0, 0], [0, 1], 1.5):
        with pytest.raises(ValueError):
            cm.gate_grads(x, bad, nl)
    with pytest.raises(ValueError):
        cm.gate_grads(x, None, nl)
    for bad in (0, nc + 1):
        with pytest.raises(ValueError):
            cm.gate_grads(x, y, bad)
    # more than 256 tokens: the refusal of the compact training entry points
    cfg = OV.VitConfig(img_size=384, patch_size=16, num_classes=16, embed_dim=64, depth=2, num_heads=1, enable_dist=0)
    ex577 = CP.export_compact(dense_state(cfg))
    with pytest.raises(NotImplementedError, match="256"):
        PR.CompactGateViT(ex577, precision="fp32")
    big = CP.CompactVisionTransformer(ex577, precision="fp32")
    lib = CP._bind()
    assert lib.uvc_vit_compact_gate_grads_workspace_bytes(C.byref(big._cfg), big._blocks, big._nb, 2) == -1
    assert lib.uvc_vit_compact_gate_grads(C.byref(big._cfg), big._blocks, big._nb, C.byref(io), L.ptr(yc), nl, L.ptr(gates), None, L.cur_stream()) == 3
    assert b"256" in L.lib().uvc_last_error()
    torch.cuda.synchronize()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def test_commands(tmp_path, capsys):
    """score on twelve colour images through the CIFAR-10 reader, apply --keep_macs 0.7, compact eval of the result; the sums of score are
    importance's on the same batches bit for bit (whatever the batch size); the shrunk file runs within the eval-logit bar of its own spec."""
    ex, _ = AR.export_of("stage2_micro_deit")
    images, labels = KR.colour_images(12, 2)
    root = KR.write_cifar10(str(tmp_path / "data"), (images, labels), KR.colour_images(6, 1))
    src, sc, dst = (str(tmp_path / n) for n in ("m.compact.pt", "scores.pt", "small.compact.pt"))
    torch.save(ex, src)
    data = ["--dataset", "cifar10", "--data_dir", root, "--num_workers", "2"]
    rec = PR.main(["score", "--compact", src, "--output", sc, "--eval_batch_size", "5", "--precision", "fp32", "--split", "train"] + data)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == rec
    assert sorted(rec) == ["gates", "images", "img_per_s", "output"] and rec["images"] == 12 and rec["gates"] == len(PR.gate_table(ex))
    scores = PR.check_scores(torch.load(sc), ex)
    assert scores["meta"]["num_labels"] == 10 and scores["meta"]["precision"] == "fp32" and scores["meta"]["loss"] == "ce"
    # importance on the same images in other batches: the same bits
    from uvc_amd import compact_tools as TL
    args = PR.build_parser().parse_args(["score", "--compact", src, "--output", sc, "--eval_batch_size", "12", "--precision", "fp32"] + data)
    loader, classes = TL.eval_loader(ex, args, "train")
    assert classes == 10
    batches = [(x, y) for x, y in loader]
    assert len(batches) == 1 and torch.equal(batches[0][1].cpu().long(), torch.from_numpy(labels))
    cm = model_of("stage2_micro_deit", "fp32")
    whole = PR.importance(cm, batches, 10)
    x, y = batches[0]
    parts = PR.importance(cm, [(x[:1], y[:1]), (x[1:8].contiguous(), y[1:8]), (x[8:].contiguous(), y[8:])], 10)
    for k in ("sum_sq", "sum_abs"):
        assert torch.equal(scores[k], whole[k]) and torch.equal(scores[k], parts[k]), k
    assert bool((scores["sum_sq"] > 0).any()) and whole["images"] == parts["images"] == 12
    s = cm.gate_grads(x, y, 10)[2].double().cpu()
    sq = torch.zeros(s.shape[1], dtype=torch.float64)
    for b in range(12):
        sq += s[b] * s[b]
    assert torch.equal(scores["sum_sq"], sq)
    rec = PR.main(["score", "--compact", src, "--output", str(tmp_path / "five.pt"), "--eval_batch_size", "4", "--precision", "fp32", "--max_images", "5"] + data)
    assert rec["images"] == 5
    # apply, and the smaller file through compact eval
    rec = PR.main(["apply", "--compact", src, "--scores", sc, "--keep_macs", "0.7", "--output", dst])
    small = CP.load_compact(dst)
    assert rec["macs_padded_after"] == CP.compact_macs(small, padded=True) <= 0.7 * CP.compact_macs(ex, padded=True)
    capsys.readouterr()
    acc = CP.main(["eval", "--compact", dst, "--synthetic", "0", "--eval_batch_size", "6", "--precision", "fp32"] + data)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["top1"] == acc and line["macs_compact_padded"] == rec["macs_padded_after"]
    xs = x[:4].contiguous()
    got = CP.CompactVisionTransformer(small, precision="fp32")(xs)[0].double().cpu()
    want = CP.reference_forward(small, xs.cpu().double())
    e = float((got - want).abs().max() / want.abs().max())
    print(f"shrunk file, float32 eval logits against reference_forward: {e:.2e} of the largest logit (bar 1e-3)")
    assert e <= 1e-3
