"""CPU: compact-model plan, export and reference forward (uvc_amd/compact.py) against the oracle's eval forward on the masked dense
weights.  No GPU."""
import pytest
import torch

from oracle import vit as OV
from uvc_amd import compact as CP


def dense_state(cfg, seed=3, patch_gating=0, masks=None):
    """An oracle state dict (float32) with mask buffers; ``masks`` overrides entries (hand-built or synthetic)."""
    sd = OV.init_params_numpy(cfg, seed, enable_patch_gating=patch_gating, weight_gain=3.0)
    for k in list(sd):
        if k.endswith(".weight") and "norm" not in k:
            sd[k[: -len("weight")] + "mask"] = torch.ones_like(sd[k])
    for k, v in (masks or {}).items():
        sd[k] = v.clone()
    return sd


def masked_params(sd, dtype=torch.float64):
    out = {}
    for k, v in sd.items():
        if k.endswith(".mask"):
            continue
        m = sd.get(k[: -len("weight")] + "mask") if k.endswith(".weight") else None
        out[k] = (v * m if m is not None else v).to(dtype)
    return out


def hand_masks(cfg):
    """Block 0: head 0 keeps dims {0..9} (v_dim 16), head 1 all 64, head 2 pruned; MLP keeps 70 units via fc2 columns while fc1 rows
    stay live.  Block 1: skipped.  Block 2: no kept head, no kept unit."""
    D, Fh = cfg.embed_dim, cfg.hidden
    m = {}
    pm = torch.zeros(D, D)
    pm[:, 0:10] = 1
    pm[:, 64:128] = 1
    m["blocks.0.attn.proj.mask"] = pm
    m2 = torch.zeros(D, Fh)
    m2[:, torch.arange(0, 140, 2)] = 1
    m["blocks.0.mlp.fc2.mask"] = m2
    m["blocks.2.attn.proj.mask"] = torch.zeros(D, D)
    m["blocks.2.mlp.fc2.mask"] = torch.zeros(D, Fh)
    g = torch.tensor([-1.0, 1.0]).repeat(cfg.depth, 1)
    g[1] = torch.tensor([0.5, 0.5])                      # g[1] <= g[0]: skipped
    m["block_skip_gating"] = g
    return m


TINY = OV.VitConfig(img_size=32, patch_size=8, num_classes=16, embed_dim=192, depth=3, num_heads=3, enable_dist=1)


def test_plan_from_hand_built_masks():
    plan = CP.compact_plan(dense_state(TINY, masks=hand_masks(TINY)), mlp_multiple=64)
    b0, b1, b2 = plan["blocks"]
    assert b0["runs"] and not b1["runs"] and b2["runs"]
    assert b0["heads"] == [0, 1] and b0["v_index"] == [list(range(10)), list(range(64))] and b0["v_dim"] == 64
    assert b0["hidden_index"] == list(range(0, 140, 2)) and b0["hidden"] == 128
    assert b1["heads"] == [0, 1, 2] and b1["v_dim"] == 64 and b1["hidden"] == TINY.hidden
    assert b2["heads"] == [] and b2["v_dim"] == 0 and b2["hidden_index"] == [] and b2["hidden"] == 0
    # v_dim rounds the widest kept head up to 16
    for n, want in ((1, 16), (16, 16), (17, 32), (33, 48), (48, 48), (49, 64)):
        m = hand_masks(TINY)
        pm = torch.zeros(TINY.embed_dim, TINY.embed_dim)
        pm[:, 64:64 + n] = 1
        m["blocks.0.attn.proj.mask"] = pm
        b = CP.compact_plan(dense_state(TINY, masks=m))["blocks"][0]
        assert b["heads"] == [1] and b["v_dim"] == want, (n, b["v_dim"])


def test_export_slices_and_zero_padding():
    sd = dense_state(TINY, masks=hand_masks(TINY))
    ex = CP.export_compact(sd, CP.compact_plan(sd))
    P, S = masked_params(sd, torch.float32), ex["state_dict"]
    D = TINY.embed_dim
    assert [b["source"] for b in ex["blocks"]] == [0, 2]
    assert not any(k.endswith(".mask") or k.startswith("gumbel.") or k == "block_skip_gating" for k in S)
    w, bq, pw = S["blocks.0.attn.qkv.weight"], S["blocks.0.attn.qkv.bias"], S["blocks.0.attn.proj.weight"]
    assert tuple(w.shape) == (2 * (128 + 64), D) and tuple(pw.shape) == (D, 2 * 64)
    Wq, Bq, Wp = P["blocks.0.attn.qkv.weight"], P["blocks.0.attn.qkv.bias"], P["blocks.0.attn.proj.weight"]
    assert torch.equal(w[0:128], Wq[0:128]) and torch.equal(w[128:256], Wq[D:D + 128]) and torch.equal(bq[0:128], Bq[0:128])
    assert torch.equal(w[256:266], Wq[2 * D:2 * D + 10]) and torch.equal(w[320:384], Wq[2 * D + 64:2 * D + 128])
    assert torch.equal(pw[:, 0:10], Wp[:, 0:10]) and torch.equal(pw[:, 64:128], Wp[:, 64:128])
    assert not w[266:320].any() and not bq[266:320].any() and not pw[:, 10:64].any()          # padding of head 0's value dims
    idx = torch.arange(0, 140, 2)
    w1, b1, w2 = S["blocks.0.mlp.fc1.weight"], S["blocks.0.mlp.fc1.bias"], S["blocks.0.mlp.fc2.weight"]
    assert tuple(w1.shape) == (128, D) and torch.equal(w1[:70], P["blocks.0.mlp.fc1.weight"][idx]) and torch.equal(b1[:70], P["blocks.0.mlp.fc1.bias"][idx])
    assert torch.equal(w2[:, :70], P["blocks.0.mlp.fc2.weight"][:, idx])
    assert not w1[70:].any() and not b1[70:].any() and not w2[:, 70:].any()
    assert S["blocks.1.attn.qkv.weight"].numel() == 0 and S["blocks.1.mlp.fc1.weight"].numel() == 0


def _check_against_oracle(cfg, masks, patch_gating=0, patch_hard=False, B=2, seed=5):
    sd = dense_state(cfg, patch_gating=patch_gating, masks=masks)
    if patch_gating:
        sd["patch_gating"] = torch.linspace(-2, 2, cfg.num_patches).reshape(1, -1, 1)
    plan = CP.compact_plan(sd)
    plan["cfg"]["patch_hard"] = int(patch_hard)
    ex = CP.export_compact(sd, plan)
    x = torch.randn(B, cfg.in_chans, cfg.img_size, cfg.img_size, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    flags = OV.GateFlags(training=False, enable_patch_gating=patch_gating, patch_hard=patch_hard)
    want, _ = OV.forward(masked_params(sd), cfg, flags, x)
    got = CP.reference_forward(ex, x)
    err = float((got - want).abs().max() / want.abs().max())
    assert err <= 1e-10, err
    return ex


@pytest.mark.parametrize("dist", [0, 1])
def test_reference_forward_equals_oracle_eval(dist):
    cfg = OV.VitConfig(img_size=32, patch_size=8, num_classes=16, embed_dim=192, depth=6, num_heads=3, enable_dist=dist)
    _check_against_oracle(cfg, CP.synthetic_masks(cfg.depth, cfg.embed_dim, cfg.hidden, seed=1))
    _check_against_oracle(cfg, hand_masks(cfg))


@pytest.mark.parametrize("hard", [False, True])
def test_reference_forward_patch_gating_mode1(hard):
    cfg = OV.VitConfig(img_size=32, patch_size=8, num_classes=16, embed_dim=128, depth=6, num_heads=2, enable_dist=1)
    _check_against_oracle(cfg, CP.synthetic_masks(cfg.depth, cfg.embed_dim, cfg.hidden, seed=2), patch_gating=1, patch_hard=hard)


def test_reference_forward_384px():
    cfg = OV.VitConfig(img_size=384, patch_size=16, num_classes=8, embed_dim=64, depth=2, num_heads=1, enable_dist=0)
    assert cfg.seq_len == 577
    _check_against_oracle(cfg, CP.synthetic_masks(cfg.depth, cfg.embed_dim, cfg.hidden, seed=4), B=1)


def test_synthetic_masks_cover_every_case():
    masks = CP.synthetic_masks(12, 192, 768, seed=0)
    sd = dense_state(OV.VitConfig(img_size=32, patch_size=8, num_classes=16, embed_dim=192, depth=12, num_heads=3), masks=masks)
    plan = CP.compact_plan(sd)
    run = [b for b in plan["blocks"] if b["runs"]]
    assert len(run) == 10
    assert {b["v_dim"] for b in run} >= {16, 32, 48}
    assert any(len(b["heads"]) < 3 for b in run) and all(0 < len(b["hidden_index"]) < 768 for b in run)
    frac = CP.compact_macs(plan, padded=False) / CP.full_macs(plan["cfg"])
    assert 0.35 <= frac <= 0.65, frac


def test_save_load_and_refusals(tmp_path):
    sd = dense_state(TINY, masks=hand_masks(TINY))
    ex = CP.export_compact(sd)
    path = tmp_path / "m.pt"
    torch.save(ex, path)
    back = CP.load_compact(path)
    assert back["blocks"] == ex["blocks"] and back["cfg"] == ex["cfg"]
    assert all(torch.equal(back["state_dict"][k], v) for k, v in ex["state_dict"].items())
    bad = dict(ex, version=2)
    with pytest.raises(ValueError):
        CP.check_export(bad)
    with pytest.raises(ValueError):
        CP.reference_forward(dict(ex, format="something-else"), torch.zeros(1, 3, 32, 32))
    from oracle import t2t as OT
    t2t_sd = {k: torch.zeros(v) for k, v in OT.param_shapes(OT.T2TConfig()).items()}
    with pytest.raises(NotImplementedError):
        CP.compact_plan(t2t_sd)


def test_macs_without_padding_equal_mac_table_at_kept_widths():
    cfg = OV.VitConfig(img_size=32, patch_size=8, num_classes=16, embed_dim=192, depth=3, num_heads=3)
    D, Fh = cfg.embed_dim, cfg.hidden
    m = {}
    pm = torch.zeros(D, D)
    pm[:, 64:192] = 1                                    # two whole heads
    m["blocks.0.attn.proj.mask"] = pm
    m2 = torch.zeros(D, Fh)
    m2[:, :256] = 1
    m["blocks.0.mlp.fc2.mask"] = m2
    g = torch.tensor([-1.0, 1.0]).repeat(3, 1)
    g[2] = torch.tensor([1.0, -1.0])
    m["block_skip_gating"] = g
    ex = CP.export_compact(dense_state(cfg, masks=m))
    embed, _ = OV.mac_table(cfg, 4)
    k0_blk = [4 * 3 * 128 * cfg.seq_len * D, cfg.seq_len * 4 * 2 * cfg.seq_len * 64, cfg.seq_len * 4 * 2 * cfg.seq_len * 64,
              4 * cfg.seq_len * D * 128, 256 * 4 * cfg.seq_len * D, D * 4 * cfg.seq_len * 256]
    want = embed + sum(k0_blk) + sum(OV.mac_table(cfg, 4)[1][1])
    assert CP.compact_macs(ex, 4, padded=False) == want == CP.compact_macs(ex, 4, padded=True)
    assert CP.full_macs(ex["cfg"], 4) == embed + sum(sum(b) for b in OV.mac_table(cfg, 4)[1])
