"""CPU: uvc_amd.pos_embed -- loading a checkpoint into a model with another patch grid (DeiT 224 -> 384 fine-tuning)."""
import torch
import torch.nn.functional as F


def _sd(ntok, g, d=192, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return {"pos_embed": torch.randn(1, ntok + g * g, d, generator=gen), "cls_token": torch.randn(1, 1, d, generator=gen)}


def test_identity_on_an_equal_grid():
    from uvc_amd.pos_embed import resize_pos_embed
    sd = _sd(1, 14)
    out = resize_pos_embed(sd, 14)
    assert torch.equal(out["pos_embed"], sd["pos_embed"])


def test_token_rows_kept_bitwise_and_grid_bicubic():
    from uvc_amd.pos_embed import resize_pos_embed
    for ntok in (1, 2):
        sd = _sd(ntok, 14, seed=ntok)
        out = resize_pos_embed(sd, (24, 24))
        pe = out["pos_embed"]
        assert pe.shape == (1, ntok + 576, 192)
        assert torch.equal(pe[:, :ntok], sd["pos_embed"][:, :ntok])
        grid = sd["pos_embed"][:, ntok:].reshape(1, 14, 14, 192).permute(0, 3, 1, 2)
        ref = F.interpolate(grid, size=(24, 24), mode="bicubic", align_corners=False).permute(0, 2, 3, 1).reshape(1, 576, 192)
        assert torch.equal(pe[:, ntok:], ref)
        assert torch.equal(out["cls_token"], sd["cls_token"])
        assert sd["pos_embed"].shape == (1, ntok + 196, 192)       # the input is not modified


def test_deit_tiny_224_state_dict_loads_into_a_384_config():
    """A DeiT-Tiny (distilled) 224-px state dict, pos_embed resized to 24 x 24, has exactly the parameter shapes of the 384-px model
    (oracle/vit.py:param_shapes, the reference model's registration; the product's model itself only builds on the GPU)."""
    import types

    from oracle import vit as OV
    from uvc_amd.pos_embed import match_pos_embed
    kw = dict(patch_size=16, embed_dim=192, depth=12, num_heads=3, mlp_ratio=4.0, num_classes=1000, enable_dist=1)
    sd = OV.init_params_numpy(OV.VitConfig(img_size=224, **kw), seed=3)
    want = OV.param_shapes(OV.VitConfig(img_size=384, **kw), 0)
    model = types.SimpleNamespace(pos_embed=torch.empty(want["pos_embed"]), num_tokens=2)
    out = match_pos_embed(sd, model)
    assert set(out) == set(want)
    for k, shp in want.items():
        assert tuple(out[k].shape) == tuple(shp), k
        if k != "pos_embed":
            assert out[k] is sd[k]
    assert tuple(out["pos_embed"].shape) == (1, 2 + 576, 192)
    assert torch.equal(out["pos_embed"][:, :2], sd["pos_embed"][:, :2])
