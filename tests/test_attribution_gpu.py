"""GPU: class-specific relevance maps of compact models -- the kernel (uvc_attention_relevance_step) against float64 of the same stored operands
and the same lse at every tile and block edge and every value width, the engine entry point (uvc_vit_compact_attribution) against the forward's
logits and against ``compact.reference_attribution`` in float64, and the ``attribute`` subcommand end to end."""
import ctypes as C
import json

import numpy as np
import pytest
import torch
from PIL import Image

import attribution_ref as AR
import test_rollout_gpu as RG
from oracle import vit as OV
from test_compact_cpu import dense_state
from uvc_amd import _lib as L
from uvc_amd import compact as CP
from uvc_amd import ops
from uvc_amd.compact_attribution import CompactAttributionViT

pytestmark = pytest.mark.gpu

DT = RG.DT


def operands(which, B, N, H, dv, prec):
    """(qkv, lse, dout, r_in) on the GPU: test_rollout_gpu.family's draws (attribution_ref.family is their host copy), a unit-normal dout
    drawn on the host, and the lse the forward kernel leaves for these operands."""
    dt, code = DT[prec]
    seed = AR.case_seed(which, N, H)
    qkv, r_in = RG.family(which, B, N, H, dv, dt, seed)
    host_qkv, host_r = AR.family(which, B, N, H, dv, dt, seed)
    assert torch.equal(qkv.cpu(), host_qkv) and torch.equal(r_in.cpu(), host_r)
    return qkv, RG.forward_lse(qkv, B, N, H, dv, code), AR.dout_of(B, N, H, dv, dt, seed).cuda(), r_in


def step(qkv, lse, dout, r_in, B, N, H, dv, code, keep, mix):
    r_out = torch.full((B, N), float("nan"), device="cuda")
    ops.attention_relevance_step(qkv, lse, dout, r_in, r_out, B, N, H, dv, code, keep=keep, mix=mix)
    return r_out


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("B,N,H,dv", AR.CASES)
def test_step_against_float64_of_the_same_operands(B, N, H, dv, prec):
    """|got - want| <= 2e-4 |want| + atol, the project's float32 attention bar, for bf16 too (nothing in this kernel is rounded to bf16).
    Family 1: atol 1e-9, idle against the smallest reference entry (>= 1e-3, asserted); family 2 (sharp attention, entries from 0 to a few
    units): atol 2e-5 of the image's largest entry.  keep = 0, mix = 1 is the term alone (keep * r_in hides nothing); keep = 1, mix = 1 is
    what the engine runs.  tests/test_attribution_cpu.py shows that this rule rejects the sum without the ReLU and the ReLU behind the head mean."""
    code = DT[prec][1]
    for which in (1, 2):
        qkv, lse, dout, r_in = operands(which, B, N, H, dv, prec)
        for keep, mix in ((0.0, 1.0), (1.0, 1.0)):
            got = step(qkv, lse, dout, r_in, B, N, H, dv, code, keep, mix)
            torch.cuda.synchronize()
            assert not torch.isnan(got).any()                   # every element < N is written
            want = AR.step_ref(qkv, lse, dout, r_in, B, N, H, dv, keep, mix)
            diff = (got.double().cpu() - want).abs()
            rel = float((diff / want.abs().clamp_min(1e-30)).max()) if which == 1 else float("nan")
            used = float((diff / (AR.RTOL * want.abs() + AR.atol_of(which, want)).clamp_min(1e-300)).max())
            print(f"relevance step {prec} B{B} N{N} H{H} dv{dv} family {which} keep {keep:.0f}: max rel {rel:.2e} max abs {float(diff.max()):.2e} "
                  f"({used:.3f} of the bar) min ref {float(want.min()):.2e} max ref {float(want.max()):.2e}")
            assert float(got.min()) >= 0.0
            if which == 1 and keep == 0.0:
                assert float(want.min()) >= AR.FAMILY1_FLOOR
            assert AR.accepted(got, want, which), (which, keep, rel, float(diff.max()))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("N", [197, 577])
def test_step_repeats_its_bits_and_ignores_the_batch(N, prec):
    dt, code = DT[prec]
    B, H, dv = 3, 3, 48
    qkv, r_in = RG.family(1, B, N, H, dv, dt, N)
    dout = AR.dout_of(B, N, H, dv, dt, N).cuda()
    lse = RG.forward_lse(qkv, B, N, H, dv, code)
    a = step(qkv, lse, dout, r_in, B, N, H, dv, code, 1.0, 1.0)
    b = step(qkv, lse, dout, r_in, B, N, H, dv, code, 1.0, 1.0)
    one = step(qkv[:1].contiguous(), lse[:1].contiguous(), dout[:1].contiguous(), r_in[:1].contiguous(), 1, N, H, dv, code, 1.0, 1.0)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(a[:1].view(torch.int32), one.view(torch.int32))


def test_step_refusals():
    """1 = UVC_ERR_ARG, 3 = UVC_ERR_UNSUPPORTED, as uvc_attention_rollout_step; nothing is launched (r_out keeps its NaNs)."""
    B, N, H, dv = 1, 1027, 1, 64
    qkv = torch.zeros(B, N, H * (128 + dv), device="cuda", dtype=torch.bfloat16)
    dout = torch.zeros(B, N, H * dv, device="cuda", dtype=torch.bfloat16)
    lse, r_in = torch.zeros(B, H, N, device="cuda"), torch.zeros(B, N, device="cuda")
    r_out = torch.full((B, N), float("nan"), device="cuda")

    def call(N=197, v_dim=64, lse=lse, dout=dout, qkv=qkv, r_in=r_in, r_out=r_out, dtype=L.UVC_BF16, head_dim=64, H=1, B=1):
        a = L.uvc_attn_relevance_args()
        a.qkv, a.lse, a.dout, a.r_in, a.r_out = L.ptr(qkv), L.ptr(lse), L.ptr(dout), L.ptr(r_in), L.ptr(r_out)
        a.B, a.N, a.H, a.head_dim, a.v_dim, a.dtype = B, N, H, head_dim, v_dim, dtype
        a.scale, a.keep, a.mix = 0.125, 1.0, 1.0
        return L.lib().uvc_attention_relevance_step(C.byref(a), L.cur_stream())

    assert call(N=1027) == 3 and b"1026" in L.lib().uvc_last_error()
    assert call(head_dim=32) == 3
    assert call(r_out=r_in) == 1
    assert call(v_dim=24) == 1 and call(v_dim=0) == 1
    assert call(lse=None) == 1 and call(dout=None) == 1 and call(qkv=None) == 1 and call(r_in=None) == 1 and call(r_out=None) == 1
    assert call(dtype=2) == 1 and call(N=0) == 1 and call(H=0) == 1 and call(B=0) == 1
    assert L.lib().uvc_attention_relevance_step(None, L.cur_stream()) == 1
    torch.cuda.synchronize()
    assert bool(torch.isnan(r_out).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not torch.isnan(r_out[:, :197]).any() and bool(torch.isnan(r_out[:, 197:]).all())        # keys >= N are not written


# ---- the engine entry point and the module ---------------------------------------------------------------------------------------
MODEL_BARS = RG.MODEL_BARS                     # the project's model-level parity bars: fp32 1e-3, bf16 2e-2
NAMES = AR.FIXTURES + AR.EXTRA
_MODELS, _REFS = {}, {}


def model_of(name, prec):
    if (name, prec) not in _MODELS:
        _MODELS[(name, prec)] = CompactAttributionViT(AR.export_of(name)[0], precision=prec)
    return _MODELS[(name, prec)]


def reference_of(name, target=None):
    """``(float64 reference on the float32 master weights, its target, e_ref)`` -- e_ref is the metric of the same reference run on the CPU with
    the batch and the weights cast to bfloat16 (a reference, not the code under test) -- computed once and left unchanged."""
    key = (name, None if target is None else tuple(target.tolist()))
    if key not in _REFS:
        ex, x = AR.export_of(name)
        ntok = 2 if ex["cfg"]["enable_dist"] else 1
        ref, t = CP.reference_attribution(ex, x.double(), target=target)
        low, _ = CP.reference_attribution(ex, x.bfloat16(), target=t)
        _REFS[key] = (ref, t, AR.map_errors(low, ref, ntok))
    return _REFS[key]


def check_map(name, prec, got, ref, e_ref, what):
    """the issue's metric over the patch entries and, apart, over the readout entries, against the bar of the precision"""
    ex, _ = AR.export_of(name)
    ntok = 2 if ex["cfg"]["enable_dist"] else 1
    e, e_tok = AR.map_errors(got, ref, ntok)
    bar, bar_tok = (MODEL_BARS["fp32"],) * 2 if prec == "fp32" else tuple(max(MODEL_BARS["bf16"], 2 * v) for v in e_ref)
    print(f"attribution {what} {name} {prec}: e {e:.2e} (e_ref {e_ref[0]:.2e}, bar {bar:.2e}); readout entries e {e_tok:.2e} (e_ref {e_ref[1]:.2e}, bar {bar_tok:.2e})")
    assert not torch.isnan(got).any() and float(got.min()) >= 0.0
    assert float(got[:, :ntok].min()) >= 1.0 / ntok - 1e-6
    assert e <= bar and e_tok <= bar_tok, (name, prec, e, e_tok)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", NAMES)
def test_attribution_against_the_float64_reference(name, prec):
    ex, x = AR.export_of(name)
    x = x.cuda()
    nc = ex["cfg"]["num_classes"]
    cm = model_of(name, prec)
    want_logits, _ = CP.CompactVisionTransformer(ex, precision=prec)(x)
    logits, rel, t = cm.attribution(x)
    assert torch.equal(logits, want_logits)                                   # the eval forward's bits
    assert rel.dtype == torch.float32 and tuple(rel.shape) == (x.shape[0], CP._seq(ex["cfg"])) and t.dtype == torch.int64
    assert torch.equal(t, logits.argmax(1))
    ref, t_ref, e_ref = reference_of(name, t.cpu())                            # the reference explains the class the engine explained
    if prec == "fp32":
        assert torch.equal(t.cpu(), reference_of(name)[1])                    # and in float32 that is the reference's own argmax
    check_map(name, prec, rel, ref, e_ref, "top-1")
    # a second call returns the same bits, and a forward after an attribution is still the forward
    logits2, rel2, t2 = cm.attribution(x)
    assert torch.equal(rel2.view(torch.int32), rel.view(torch.int32)) and torch.equal(logits2, logits) and torch.equal(t2, t)
    assert torch.equal(cm(x)[0], want_logits)
    # num_labels restricts the argmax
    nl = max(1, int(t.min()))
    _, _, t_nl = cm.attribution(x, num_labels=nl)
    assert torch.equal(t_nl, logits[:, :nl].argmax(1))
    # a given target equal to the argmax reproduces the default; another class gives another map, within the bar of its own reference
    _, same, t_same = cm.attribution(x, target=t)
    assert torch.equal(same.view(torch.int32), rel.view(torch.int32)) and torch.equal(t_same, t)
    other = (t + 1) % nc
    _, rel_o, t_o = cm.attribution(x, target=other.tolist())
    assert torch.equal(t_o, other) and float((rel_o - rel).abs().max()) > 1e-6
    ref_o, _, e_ref_o = reference_of(name, other.cpu())
    check_map(name, prec, rel_o, ref_o, e_ref_o, "other class")
    _, rel_i, t_i = cm.attribution(x[:1], target=int(other[0]))
    assert torch.equal(rel_i.view(torch.int32), rel_o[:1].view(torch.int32)) and int(t_i[0]) == int(other[0])        # an int; the batch does not matter


def test_module_refusals():
    ex, x = AR.export_of("no_heads")
    x = x.cuda()
    cm = model_of("no_heads", "fp32")
    nc = ex["cfg"]["num_classes"]
    assert list(cm.parameters()) == [] and not hasattr(cm, "_flat_grad")
    rows = torch.empty(x.shape[0] * 16, 3 * 64, device="cuda")
    with pytest.raises(ValueError, match="patch rows"):
        cm.attribution(patches=rows)
    for bad in (-1, nc, [0, 1], [0, 1, nc], 1.5):
        with pytest.raises(ValueError):
            cm.attribution(x, target=bad)
    with pytest.raises(ValueError):
        cm.attribution(x, target=4, num_labels=4)
    for bad in (0, nc + 1):
        with pytest.raises(ValueError):
            cm.attribution(x, num_labels=bad)
    with pytest.raises(NotImplementedError):
        CompactAttributionViT(ex, precision="bf16_f32resid")
    with pytest.raises(L.UvcHipError):
        CompactAttributionViT(ex, device="cpu")
    with pytest.raises(TypeError, match="CompactAttributionViT"):
        next(CP.explain(CP.CompactVisionTransformer(ex, precision="fp32"), [], method="attribution"))


def test_engine_refusals():
    ex, x = AR.export_of("no_heads")
    x = x.cuda()
    B, nc = x.shape[0], ex["cfg"]["num_classes"]
    cm = model_of("no_heads", "fp32")
    cm.attribution(x)                                           # sizes the attribution workspace for this batch
    io, _ = cm._io(x, B, "attribution")
    logits, ld = torch.empty(B, nc, device="cuda"), torch.empty(B, nc, device="cuda")
    io.logits, io.logits_dist = L.ptr(logits), L.ptr(ld)
    rel = torch.full((B, CP._seq(ex["cfg"])), float("nan"), device="cuda")
    tout = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    call = lambda io, rel, nl=nc, target=None: cm._lib_call("uvc_vit_compact_attribution", C.byref(io), L.ptr(target), nl, L.ptr(rel), L.ptr(tout), L.cur_stream())
    assert call(io, None) == 1
    assert call(io, rel, 0) == 1 and call(io, rel, nc + 1) == 1
    small, _ = cm._io(x, B, True)                               # the training workspace is too small for an attribution
    small.logits, small.logits_dist = L.ptr(logits), L.ptr(ld)
    assert small.workspace_bytes < io.workspace_bytes and call(small, rel) == 1
    assert cm._lib_call("uvc_vit_compact_attribution_workspace_bytes", 0) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(rel).all()) and tout.tolist() == [-7] * B        # nothing ran
    assert call(io, rel) == 0
    # a target outside [0, num_labels) is clamped into it by the kernel (the Python layer refuses it before): nothing is indexed out of bounds
    wild = torch.tensor([-5, 3, 1 << 20], dtype=torch.int32, device="cuda")[:B]
    assert call(io, rel, 8, wild) == 0
    torch.cuda.synchronize()
    assert tout.tolist() == [0, 3, 7][:B] and not torch.isnan(rel).any()
    # more than 256 tokens: the refusal of the compact training entry points
    cfg = OV.VitConfig(img_size=384, patch_size=16, num_classes=16, embed_dim=64, depth=2, num_heads=1, enable_dist=0)
    ex577 = CP.export_compact(dense_state(cfg))
    with pytest.raises(NotImplementedError, match="256"):
        CompactAttributionViT(ex577, precision="fp32")
    big = CP.CompactVisionTransformer(ex577, precision="fp32")                 # its cfg and blocks describe the 577-token model
    lib = CP._bind()
    assert lib.uvc_vit_compact_attribution_workspace_bytes(C.byref(big._cfg), big._blocks, big._nb, 2) == -1
    assert lib.uvc_vit_compact_attribution(C.byref(big._cfg), big._blocks, big._nb, C.byref(io), None, nc, L.ptr(rel), None, L.cur_stream()) == 3
    assert b"256" in L.lib().uvc_last_error()
    torch.cuda.synchronize()


# ---- attribute, end to end -------------------------------------------------------------------------------------------------------------
def test_attribute_command(tmp_path, capsys):
    ex, _ = AR.export_of("no_heads")
    model, out, pred_out, odir = tmp_path / "m.compact.pt", tmp_path / "maps.jsonl", tmp_path / "preds.jsonl", tmp_path / "overlays"
    torch.save(ex, model)
    rng = np.random.default_rng(5)
    files = []
    for name, (h, w), mode in [("a.png", (31, 20), "RGB"), ("b.png", (64, 64), "L"), ("c.png", (45, 80), "RGBA"), ("d.png", (90, 120), "RGB")]:
        a = rng.integers(0, 256, (h, w) if mode == "L" else (h, w, len(mode)), dtype=np.uint8)
        Image.fromarray(a, mode).save(tmp_path / name)
        files.append(str(tmp_path / name))
    broken = tmp_path / "broken.png"
    broken.write_bytes(open(files[0], "rb").read()[:40])
    files.insert(2, str(broken))
    common = ["--compact", str(model), "--images", *files, "--batch_size", "3", "--precision", "fp32", "--num_workers", "2", "--topk", "3", "--num_labels", "10"]
    summary = CP.main(["attribute", *common, "--output", str(out), "--overlay_dir", str(odir)])
    CP.main(["predict", *common, "--output", str(pred_out)])
    lines = [json.loads(l) for l in out.read_text().splitlines()]
    preds = [json.loads(l) for l in pred_out.read_text().splitlines()]
    assert len(lines) == 5 + 1 and lines[-1] == summary and summary["images"] == 5 and summary["errors"] == 1 and summary["batches"] == 2
    assert [r["file"] for r in lines[:-1]] == files
    assert set(lines[2]) == {"file", "error"} and lines[2]["error"]
    g = ex["cfg"]["img_size"] // ex["cfg"]["patch_size"]
    for i, (rec, pred) in enumerate(zip(lines[:-1], preds[:-1])):
        if i == 2:
            continue
        assert set(rec) == {"file", "top", "target", "grid", "tokens", "map"} and rec["top"] == pred["top"]
        assert rec["target"] == rec["top"][0]["index"] < 10
        assert rec["grid"] == [g, g] and len(rec["map"]) == g * g and len(rec["tokens"]) == 2
        assert min(rec["map"]) >= 0.0 and abs(sum(rec["map"]) + sum(rec["tokens"]) - 1.0) <= 1e-5
    pngs = sorted(p.name for p in odir.iterdir())
    assert pngs == ["0_a.png.png", "1_b.png.png", "3_c.png.png", "4_d.png.png"]
    for p in pngs:
        assert Image.open(odir / p).size == (ex["cfg"]["img_size"], ex["cfg"]["img_size"])
    # --target: that class for every image, other maps, the same labels
    given = (lines[0]["target"] + 1) % 10
    out_t = tmp_path / "maps_t.jsonl"
    CP.main(["attribute", *common, "--output", str(out_t), "--target", str(given)])
    lines_t = [json.loads(l) for l in out_t.read_text().splitlines()]
    assert set(lines_t[2]) == {"file", "error"}
    assert all(r["target"] == given for r in lines_t[:-1] if "target" in r)
    assert [r.get("top") for r in lines_t[:-1]] == [r.get("top") for r in lines[:-1]]
    assert lines_t[0]["map"] != lines[0]["map"] and abs(sum(lines_t[0]["map"]) + sum(lines_t[0]["tokens"]) - 1.0) <= 1e-5
    # the function: fused_input is ignored, a target outside the labels is refused before any image is read
    cm = model_of("no_heads", "fp32")
    recs = list(CP.explain(cm, files, method="attribution", topk=3, batch_size=5, num_workers=2, num_labels=10, fused_input=True))
    assert [r.get("target") for r in recs] == [r.get("target") for r in lines[:-1]]
    with pytest.raises(ValueError, match="target"):
        CP.main(["attribute", *common, "--target", "10"])
    with pytest.raises(ValueError, match="target"):
        next(CP.explain(cm, ["/nonexistent/x.png"], method="attribution", target=10, num_labels=10))
    # a file with more than 256 tokens fails before any image is listed, with the limit named
    cfg = OV.VitConfig(img_size=384, patch_size=16, num_classes=16, embed_dim=64, depth=2, num_heads=1, enable_dist=0)
    big = tmp_path / "big.compact.pt"
    torch.save(CP.export_compact(dense_state(cfg)), big)
    with pytest.raises(NotImplementedError, match="256"):
        CP.main(["attribute", "--compact", str(big), "--images", "/nonexistent/dir", "--precision", "fp32"])
    capsys.readouterr()
