"""GPU: attention rollout maps of compact models -- the kernel (uvc_attention_rollout_step) against float64 of the same stored operands and
the same lse at every tile and block edge, the engine entry point (uvc_vit_compact_rollout) against the forward's logits and against
``compact.reference_rollout`` in float64, and the ``explain`` subcommand end to end."""
import ctypes as C
import json

import numpy as np
import pytest
import torch
from PIL import Image

import scenarios as SC
from compact_train_ref import fixture_export
from oracle import vit as OV
from test_compact_cpu import dense_state
from uvc_amd import _lib as L
from uvc_amd import compact as CP
from uvc_amd import ops

pytestmark = pytest.mark.gpu

DT = {"fp32": (torch.float32, L.UVC_F32), "bf16": (torch.bfloat16, L.UVC_BF16)}
# at, and one past, every tile and block edge (64, 128, 256), plus the models' ragged sizes
CASES = [(2, 1, 1, 64), (2, 5, 1, 16), (2, 64, 2, 32), (2, 65, 3, 48), (2, 128, 1, 64), (2, 129, 2, 64), (2, 197, 3, 64), (2, 198, 6, 32),
         (2, 257, 2, 64), (1, 577, 3, 16), (1, 1026, 2, 64)]


def gen(seed):
    return torch.Generator().manual_seed(seed)      # host draws: the same operands on every machine


def forward_lse(qkv, B, N, H, dv, code):
    o = torch.empty(B, N, H * dv, device="cuda", dtype=qkv.dtype)
    lse = torch.empty(B, H, N, device="cuda")
    ops.attention_fwd(qkv, o, lse, B, N, H, code, v_dim=dv)
    return lse


def step(qkv, lse, r_in, B, N, H, dv, code, keep=0.5, mix=0.5):
    r_out = torch.full((B, N), float("nan"), device="cuda")
    ops.attention_rollout_step(qkv, lse, r_in, r_out, B, N, H, dv, code, keep=keep, mix=mix)
    return r_out


def step_ref(qkv, lse, r_in, B, N, H, keep, mix):
    """float64 of the stored operands and of the lse the kernel reads."""
    x = qkv.double()
    q = x[..., :H * 64].reshape(B, N, H, 64).transpose(1, 2)
    k = x[..., H * 64:2 * H * 64].reshape(B, N, H, 64).transpose(1, 2)
    p = torch.exp((q @ k.transpose(-2, -1)) * 0.125 - lse.double().unsqueeze(-1))          # [B, H, i, j]
    return keep * r_in.double() + (mix / H) * torch.einsum("bi,bhij->bj", r_in.double(), p)


def family(which, B, N, H, dv, dt, seed):
    g = gen(seed)
    if which == 1:                      # unit-normal q, k; r_in a random probability vector (entries within a factor 2 of each other)
        qkv = torch.randn(B, N, H * (128 + dv), generator=g).to(dt)
        r_in = 1.0 + torch.rand(B, N, generator=g)
        return qkv.cuda(), (r_in / r_in.sum(1, keepdim=True)).cuda()
    # k = q, rows of norm 16: a query's own score is 32, another's 32 cos(angle) (standard deviation 4): it attends almost only to itself
    qkv = torch.randn(B, N, H * (128 + dv), generator=g)
    q = qkv[..., :H * 64].reshape(B, N, H, 64)
    q = (16.0 * q / q.norm(dim=-1, keepdim=True)).reshape(B, N, H * 64)
    qkv[..., :H * 64], qkv[..., H * 64:2 * H * 64] = q, q
    r_in = torch.zeros(B, N)
    r_in[:, 0] = 1.0
    return qkv.to(dt).cuda(), r_in.cuda()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("B,N,H,dv", CASES)
def test_step_against_float64_of_the_same_operands(B, N, H, dv, prec):
    """rtol 2e-4: the project's float32 attention bar, for bf16 too (nothing in this kernel is rounded to bf16).  Family 1: atol 1e-9, negligible
    against the smallest reference entry (>= 7e-4); family 2 (entries in [0, 1], maximum near 1): atol 2e-5.  keep = 0, mix = 1: every image's
    r_out sums to its r_in's sum within 1e-5 relative, what an lse rounded to float32 allows."""
    dt, code = DT[prec]
    for which, atol in ((1, 1e-9), (2, 2e-5)):
        qkv, r_in = family(which, B, N, H, dv, dt, 1000 * which + N + H)
        lse = forward_lse(qkv, B, N, H, dv, code)
        got = step(qkv, lse, r_in, B, N, H, dv, code)
        torch.cuda.synchronize()
        assert not torch.isnan(got).any()
        want = step_ref(qkv, lse, r_in, B, N, H, 0.5, 0.5)
        rel = float(((got.double() - want).abs() / want.abs().clamp_min(1e-30)).max()) if which == 1 else float("nan")
        err = float((got.double() - want).abs().max())
        print(f"rollout step {prec} B{B} N{N} H{H} dv{dv} family {which}: max rel {rel:.2e} max abs {err:.2e} min ref {float(want.min()):.2e} max ref {float(want.max()):.2e}")
        assert bool(((got.double() - want).abs() <= atol + 2e-4 * want.abs()).all()), (which, rel, err)
        if which == 1:
            assert float(want.min()) >= 7e-4
        else:
            assert 0.0 <= float(want.min()) and 0.9 <= float(want.max()) <= 1.0 + 1e-5       # (above 1 by what the float32 lse is off)
        pure = step(qkv, lse, r_in, B, N, H, dv, code, keep=0.0, mix=1.0)
        assert not torch.isnan(pure).any()
        s_in, s_out = r_in.double().sum(1), pure.double().sum(1)
        drift = float(((s_out - s_in).abs() / s_in).max())
        print(f"    keep 0, mix 1: sum drift {drift:.2e}")
        assert drift <= 1e-5, (which, drift)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("N", [197, 577])
def test_step_repeats_its_bits_and_ignores_the_batch(N, prec):
    dt, code = DT[prec]
    B, H, dv = 3, 3, 64
    qkv, r_in = family(1, B, N, H, dv, dt, N)
    lse = forward_lse(qkv, B, N, H, dv, code)
    a = step(qkv, lse, r_in, B, N, H, dv, code)
    b = step(qkv, lse, r_in, B, N, H, dv, code)
    one = step(qkv[:1].contiguous(), lse[:1].contiguous(), r_in[:1].contiguous(), 1, N, H, dv, code)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(a[:1].view(torch.int32), one.view(torch.int32))


def test_step_refusals():
    """The codes of the neighbouring attention entry points: 1 = UVC_ERR_ARG, 3 = UVC_ERR_UNSUPPORTED; nothing is launched (r_out keeps its NaNs)."""
    B, N, H, dv = 1, 1027, 1, 64
    qkv = torch.zeros(B, N, H * (128 + dv), device="cuda", dtype=torch.bfloat16)
    lse, r_in = torch.zeros(B, H, N, device="cuda"), torch.zeros(B, N, device="cuda")
    r_out = torch.full((B, N), float("nan"), device="cuda")

    def call(N=197, v_dim=64, lse=lse, r_out=r_out, dtype=L.UVC_BF16, head_dim=64, H=1):
        a = L.uvc_attn_rollout_args()
        a.qkv, a.lse, a.r_in, a.r_out = L.ptr(qkv), L.ptr(lse), L.ptr(r_in), L.ptr(r_out)
        a.B, a.N, a.H, a.head_dim, a.v_dim, a.dtype = 1, N, H, head_dim, v_dim, dtype
        a.scale, a.keep, a.mix = 0.125, 0.5, 0.5
        return L.lib().uvc_attention_rollout_step(C.byref(a), L.cur_stream())

    assert call(N=1027) == 3 and b"1026" in L.lib().uvc_last_error()
    assert call(r_out=r_in) == 1
    assert call(v_dim=24) == 1
    assert call(lse=None) == 1
    assert call(dtype=2) == 1 and call(head_dim=32) == 3 and call(N=0) == 1 and call(H=0) == 1
    torch.cuda.synchronize()
    assert bool(torch.isnan(r_out).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not torch.isnan(r_out[:, :197]).any() and bool(torch.isnan(r_out[:, 197:]).all())        # keys >= N are not written


# ---- the engine entry point and the module ---------------------------------------------------------------------------------------
MODEL_BARS = {"fp32": 1e-3, "bf16": 2e-2}      # the project's model-level parity bars
TINY = OV.VitConfig(img_size=32, patch_size=8, num_classes=16, embed_dim=192, depth=3, num_heads=3, enable_dist=1)
FIXTURES = ["stage2_micro_skip", "stage2_micro_deit", "stage2_micro_none", "stage2_tiny8"]
_EXPORTS, _REFS, _MODELS = {}, {}, {}


def export_of(name):
    """(compact export, float32 batch on the GPU), built once per name."""
    if name in _EXPORTS:
        return _EXPORTS[name]
    g = torch.Generator().manual_seed(11)
    if name in FIXTURES:
        r, _, ex, _ = fixture_export(name)
        x = torch.from_numpy(SC.make_inputs(r)[0][0]).float()[:4]
    elif name == "micro384":                   # N = 577: the streaming attention forward, five key blocks in the rollout step
        cfg = OV.VitConfig(img_size=384, patch_size=16, num_classes=16, embed_dim=64, depth=2, num_heads=1, enable_dist=0)
        ex = CP.export_compact(dense_state(cfg))
        x = torch.randn(2, 3, 384, 384, generator=g)
    elif name == "hard_gating":
        sd = dense_state(TINY, patch_gating=1, masks=CP.synthetic_masks(TINY.depth, TINY.embed_dim, TINY.hidden, seed=1))
        sd["patch_gating"] = torch.linspace(-3, 3, sd["patch_gating"].numel()).reshape(sd["patch_gating"].shape)
        ex = CP.export_compact(sd)
        ex["cfg"]["patch_hard"] = 1
        assert ex["cfg"]["patch_gating"] == 1
        x = torch.randn(3, 3, 32, 32, generator=g)
    else:                                      # "no_heads": the middle block keeps no head
        ex = CP.export_compact(dense_state(TINY, masks={"blocks.1.attn.proj.mask": torch.zeros(TINY.embed_dim, TINY.embed_dim)}))
        assert [len(b["heads"]) for b in ex["blocks"]] == [3, 0, 3]
        x = torch.randn(3, 3, 32, 32, generator=g)
    _EXPORTS[name] = (ex, x.cuda())
    return _EXPORTS[name]


def model_of(name, prec):
    if (name, prec) not in _MODELS:
        _MODELS[(name, prec)] = CP.CompactVisionTransformer(export_of(name)[0], precision=prec)
    return _MODELS[(name, prec)]


def reference_of(name, method):
    """float64 on the float32 master weights, computed once and left unchanged."""
    if (name, method) not in _REFS:
        ex, x = export_of(name)
        _REFS[(name, method)] = CP.reference_rollout(ex, x.double(), method=method)
    return _REFS[(name, method)]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", FIXTURES + ["micro384"])
def test_rollout_logits_are_the_forward_s(name, prec):
    ex, x = export_of(name)
    cm = model_of(name, prec)
    c = ex["cfg"]
    rows = torch.empty(x.shape[0] * (c["img_size"] // c["patch_size"]) ** 2, c["in_chans"] * c["patch_size"] ** 2, dtype=DT[prec][0], device="cuda")
    ops.patchify(x, rows, c["patch_size"], DT[prec][1])
    want, _ = cm(x)
    want_p, _ = cm(patches=rows)
    for method in CP.METHODS:
        got, maps = cm.rollout(x, method=method)
        got_p, maps_p = cm.rollout(patches=rows, method=method)
        assert torch.equal(got, want) and torch.equal(got_p, want_p)
        assert maps.dtype == torch.float32 and tuple(maps.shape) == (x.shape[0], CP._seq(c))
        assert torch.equal(want_p, want) and torch.equal(maps_p, maps)          # patch rows handed in: the same bits
    again, _ = cm(x)                       # and a forward after a rollout is still the forward
    assert torch.equal(again, want)
    with pytest.raises(ValueError):
        cm.rollout(x, method="max")
    with pytest.raises(ValueError):
        cm.rollout(x, patches=rows)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("method", list(CP.METHODS))
@pytest.mark.parametrize("name", FIXTURES + ["micro384", "hard_gating", "no_heads"])
def test_maps_against_the_float64_reference(name, method, prec):
    ex, x = export_of(name)
    maps = model_of(name, prec).rollout(x, method=method)[1].double()
    ref = reference_of(name, method)
    err = float((maps - ref).abs().max() / ref.max())
    drift = float((maps.sum(1) - 1).abs().max())
    print(f"rollout maps {name} {method} {prec}: max|got - ref| / max ref {err:.2e}, sum drift {drift:.2e}")
    assert not torch.isnan(maps).any() and float(maps.min()) >= 0.0
    assert err <= MODEL_BARS[prec], (name, method, prec, err)
    assert drift <= 1e-4
    again = model_of(name, prec).rollout(x, method=method)[1].double()
    assert torch.equal(again, maps)


def test_rollout_refusals():
    from uvc_amd.model_distilled import uvc_vit_io
    ex, x = export_of("no_heads")
    cm = model_of("no_heads", "fp32")
    cm.rollout(x)                                           # sizes the rollout workspace for this batch
    io, _ = cm._io(x, x.shape[0], "rollout")
    logits, ld = torch.empty(x.shape[0], 16, device="cuda"), torch.empty(x.shape[0], 16, device="cuda")
    io.logits, io.logits_dist = L.ptr(logits), L.ptr(ld)
    maps = torch.empty(x.shape[0], CP._seq(ex["cfg"]), device="cuda")
    call = lambda io, maps, method: cm._lib_call("uvc_vit_compact_rollout", C.byref(io), L.ptr(maps), method, L.cur_stream())
    assert call(io, maps, 0) == 0
    assert call(io, None, 0) == 1 and call(io, maps, 2) == 1
    small, _ = cm._io(x, x.shape[0], False)                 # the eval workspace is too small for a rollout
    small.logits, small.logits_dist = L.ptr(logits), L.ptr(ld)
    assert small.workspace_bytes < io.workspace_bytes and call(small, maps, 0) == 1
    assert cm._lib_call("uvc_vit_compact_rollout_workspace_bytes", 0) == -1
    torch.cuda.synchronize()


# ---- explain, end to end ---------------------------------------------------------------------------------------------------------------
def test_explain_command(tmp_path, capsys):
    ex, _ = export_of("no_heads")
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
    common = ["--compact", str(model), "--images", *files, "--batch_size", "3", "--precision", "fp32", "--num_workers", "2", "--topk", "3"]
    summary = CP.main(["explain", *common, "--output", str(out), "--overlay_dir", str(odir)])
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
        assert set(rec) == {"file", "top", "grid", "tokens", "map"} and rec["top"] == pred["top"]
        assert rec["grid"] == [g, g] and len(rec["map"]) == g * g and len(rec["tokens"]) == 2
        assert min(rec["map"]) >= 0.0 and abs(sum(rec["map"]) + sum(rec["tokens"]) - 1.0) <= 1e-4
    pngs = sorted(p.name for p in odir.iterdir())
    assert pngs == ["0_a.png.png", "1_b.png.png", "3_c.png.png", "4_d.png.png"]
    for p in pngs:
        assert Image.open(odir / p).size == (ex["cfg"]["img_size"], ex["cfg"]["img_size"])
    # the function, the other method, no overlays: the records of the same files
    cm = model_of("no_heads", "fp32")
    last = list(CP.explain(cm, files, method="last", topk=3, batch_size=5, num_workers=2))
    assert [r.get("top") for r in last] == [r.get("top") for r in lines[:-1]]
    assert any(r["map"] != l["map"] for r, l in zip(last, lines[:-1]) if "map" in r)
    with pytest.raises(ValueError):
        list(CP.explain(cm, files, method="max"))
    capsys.readouterr()
