"""GPU: compact models (uvc_amd/compact.py) -- the attention forward with a value head dim of its own (uvc_attn_args.v_dim), the
compact forward sequencer (uvc_vit_compact_forward) against the dense masked eval model and the float64 reference, and the
export -> eval command line on a Stage-2 checkpoint."""
import ctypes as C
import json

import pytest
import torch

from uvc_amd import _lib as L
from uvc_amd import compact as CP

pytestmark = pytest.mark.gpu

DT = {"fp32": (torch.float32, L.UVC_F32, 1e-3), "bf16": (torch.bfloat16, L.UVC_BF16, 2e-2)}


def attn(qkv, B, N, H, v_dim, dtype_code, head_keep=None, bwd=False):
    dv = v_dim or 64
    o = torch.empty(B, N, H * dv, device="cuda", dtype=qkv.dtype)
    lse = torch.empty(B, H, N, device="cuda")
    a = L.uvc_attn_args()
    a.qkv, a.o, a.lse = L.ptr(qkv), L.ptr(o), L.ptr(lse)
    a.B, a.N, a.H, a.head_dim, a.dtype, a.scale, a.v_dim = B, N, H, 64, dtype_code, 0.125, v_dim
    a.head_keep = L.ptr(head_keep)
    if bwd:
        dout, dqkv, delta = torch.zeros_like(o), torch.zeros_like(qkv), torch.zeros_like(lse)
        a.dout, a.dqkv, a.delta = L.ptr(dout), L.ptr(dqkv), L.ptr(delta)
        return L.lib().uvc_attention_bwd(C.byref(a), L.cur_stream())
    rc = L.lib().uvc_attention_fwd(C.byref(a), L.cur_stream())
    return rc, o, lse


def ref_attn(qkv, B, N, H, dv):
    x = qkv.double()
    q = x[..., :H * 64].reshape(B, N, H, 64).transpose(1, 2)
    k = x[..., H * 64:2 * H * 64].reshape(B, N, H, 64).transpose(1, 2)
    v = x[..., 2 * H * 64:].reshape(B, N, H, dv).transpose(1, 2)
    s = (q @ k.transpose(-2, -1)) * 0.125
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(B, N, H * dv), torch.logsumexp(s, -1)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("N,H", [(50, 3), (197, 3), (198, 6), (256, 2), (577, 3), (785, 1)])
def test_attention_v_dim_against_float64(prec, N, H):
    dt, code, tol = DT[prec]
    g = torch.Generator(device="cuda").manual_seed(N * 7 + H)
    B = 2
    for dv in (16, 32, 48, 64):
        qkv = (torch.randn(B, N, H * (128 + dv), device="cuda", generator=g) * 1.5).to(dt)
        rc, o, lse = attn(qkv, B, N, H, dv, code)
        assert rc == 0, L.lib().uvc_last_error()
        torch.cuda.synchronize()
        want, want_lse = ref_attn(qkv, B, N, H, dv)
        err = float((o.double() - want).abs().max() / want.abs().max())
        assert err <= tol, (prec, N, H, dv, err)
        assert float((lse.double() - want_lse).abs().max()) <= 10 * tol, (prec, N, H, dv)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("N", [197, 577])
def test_attention_v_dim_64_is_the_standard_layout(prec, N):
    dt, code, _ = DT[prec]
    B, H = 2, 3
    qkv = torch.randn(B, N, 3 * H * 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(N)).to(dt)
    rc0, o0, l0 = attn(qkv, B, N, H, 0, code)
    rc1, o1, l1 = attn(qkv, B, N, H, 64, code)
    assert rc0 == 0 and rc1 == 0
    assert torch.equal(o0, o1) and torch.equal(l0, l1)


def test_attention_v_dim_refusals():
    B, N, H = 1, 197, 2
    qkv = torch.zeros(B, N, H * (128 + 32), device="cuda", dtype=torch.bfloat16)
    keep = torch.ones(H, dtype=torch.int32, device="cuda")
    assert attn(qkv, B, N, H, 32, L.UVC_BF16, head_keep=keep)[0] == 3          # UVC_ERR_UNSUPPORTED
    assert attn(qkv, B, N, H, 24, L.UVC_BF16)[0] == 1                          # UVC_ERR_ARG
    assert attn(qkv, B, N, H, 32, L.UVC_BF16, bwd=True) == 3
    qkv64 = torch.zeros(B, N, 3 * H * 64, device="cuda", dtype=torch.bfloat16)
    assert attn(qkv64, B, N, H, 64, L.UVC_BF16, bwd=True) == 3


# ---- the compact model ------------------------------------------------------------------------------------------------------------
SHAPES = {"tiny": dict(embed_dim=192, num_heads=3), "small": dict(embed_dim=384, num_heads=6)}


def dense_model(shape, prec, depth=7, masks=None, img=224, dist=1, patch_gating=1, num_classes=64, seed=0):
    from uvc_amd.model_distilled import DistilledVisionTransformer
    torch.manual_seed(seed)
    m = DistilledVisionTransformer(enable_dist=dist, enable_patch_gating=patch_gating, img_size=img, patch_size=16, depth=depth,
                                   num_classes=num_classes, precision=prec, device="cuda", **SHAPES[shape])
    with torch.no_grad():
        for p in m.parameters():                    # larger weights than the init: attention far from uniform, logits well apart
            if p.dim() >= 2:
                p.mul_(4.0)
        if patch_gating:
            m.patch_gating.copy_(torch.linspace(-3, 3, m.patch_gating.numel()).reshape(m.patch_gating.shape))
    m.mark_weights_changed()
    CP.apply_synthetic_masks(m, masks if masks is not None else CP.synthetic_masks(depth, m.embed_dim, m._cfg.hidden, seed=seed))
    m.eval()
    return m


def compare(dense, prec, B=16, seed=1, export=None):
    _, _, tol = DT[prec]
    x = torch.randn(B, 3, dense._cfg.img_size, dense._cfg.img_size, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))
    export = export or CP.export_compact(dense)
    cm = CP.CompactVisionTransformer(export, precision=prec)
    with torch.no_grad():
        want, _ = dense(x)
        got, macs = cm(x)
    torch.cuda.synchronize()
    scale = float(want.abs().max())
    err = float((got - want).abs().max()) / scale
    assert err <= tol, (prec, err)
    top2 = want.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 2 * tol * scale
    assert torch.equal(got.argmax(1)[sure], want.argmax(1)[sure])
    ref = CP.reference_forward(export, x.double())
    err_ref = float((got.double() - ref).abs().max() / ref.abs().max())
    assert err_ref <= tol, (prec, err_ref)
    assert macs == CP.compact_macs(export, B)
    return export


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", ["tiny", "small"])
def test_compact_model_matches_dense_masked_eval(shape, prec):
    ex = compare(dense_model(shape, prec), prec)
    assert {b["v_dim"] for b in ex["blocks"]} == {16, 32, 48, 64} and len(ex["blocks"]) == 5


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_zero_head_zero_unit_and_one_block(prec):
    D, Fh, depth = 192, 768, 4
    g = torch.tensor([-1.0, 1.0]).repeat(depth, 1)
    masks = {"block_skip_gating": g.clone(), "blocks.1.attn.proj.mask": torch.zeros(D, D), "blocks.2.mlp.fc2.mask": torch.zeros(D, Fh),
             "blocks.3.attn.proj.mask": torch.zeros(D, D), "blocks.3.mlp.fc2.mask": torch.zeros(D, Fh)}
    ex = compare(dense_model("tiny", prec, depth=depth, masks=masks, dist=0, patch_gating=0), prec)
    assert [(len(b["heads"]), b["hidden"]) for b in ex["blocks"]] == [(3, 768), (0, 768), (3, 0), (0, 0)]
    gs = torch.tensor([1.0, -1.0]).repeat(depth, 1)
    gs[2] = torch.tensor([-1.0, 1.0])
    ex1 = compare(dense_model("tiny", prec, depth=depth, masks={"block_skip_gating": gs}, img=96), prec)
    assert [b["source"] for b in ex1["blocks"]] == [2]


def test_export_then_eval_cli_on_a_stage2_checkpoint(tmp_path, capsys):
    from uvc_amd import post_train
    micro = '{"patch_size": 16, "embed_dim": 128, "depth": 3, "num_heads": 2}'
    from uvc_amd.model_distilled import DistilledVisionTransformer
    m = DistilledVisionTransformer(enable_dist=0, img_size=64, patch_size=16, embed_dim=128, depth=3, num_heads=2, num_classes=16,
                                   precision="fp32", device="cuda")
    masks = CP.synthetic_masks(3, 128, 512, seed=3)
    masks["blocks.1.attn.proj.mask"][:, 64:] = 0                     # one head of block 1 pruned
    CP.apply_synthetic_masks(m, masks)
    s1 = tmp_path / "s1.pth"
    torch.save(m.state_dict(), s1)
    del m
    post_train.main(["--model_type", "custom", "--model_cfg", micro, "--img_size", "64", "--num_classes", "16", "--train_batch_size", "8",
                     "--eval_batch_size", "8", "--epochs", "1", "--steps", "2", "--precision", "fp32", "--checkpoint_dir", str(s1),
                     "--output_dir", str(tmp_path), "--name", "s2", "--learning_rate", "0.01", "--warmup_epochs", "1", "--compact_multiple", "64"])
    ck = sorted((tmp_path / "s2").glob("custom_*.pth.tar"))[0]
    capsys.readouterr()
    flags = ["--model_type", "custom", "--model_cfg", micro, "--img_size", "64", "--num_classes", "16", "--checkpoint_dir", str(ck), "--precision", "fp32"]
    out = tmp_path / "m.compact.pt"
    CP.main(["export", *flags, "--output", str(out)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["macs_compact"] <= line["macs_compact_padded"] < line["macs_full"] and len(line["blocks"]) == 3
    acc = CP.main(["eval", *flags, "--compact", str(out), "--eval_batch_size", "8", "--eval_steps", "2"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["top1"] == acc and line["params"] > 0
    # the dense --eval_only path on the same checkpoint gives the same top-1 on the same synthetic batches
    post_train.main(["--model_type", "custom", "--model_cfg", micro, "--img_size", "64", "--num_classes", "16", "--eval_batch_size", "8",
                     "--eval_steps", "2", "--precision", "fp32", "--checkpoint_dir", str(ck), "--eval_only", "1"])
    dense_line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert abs(dense_line["best_acc"] - acc) <= 100.0 / 16 + 1e-6
