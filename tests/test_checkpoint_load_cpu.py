"""CPU: uvc_amd.checkpoints.load_pretrained on a stand-in module whose state_dict has the engine DeiT's key / shape table
(oracle.vit.param_shapes, the reference's registration order): the checkpoint layouts of the reference and the public DeiT /
T2T-ViT releases, the head dropped on a class-count mismatch, pos_embed resampling, and the refusals.  Also the teacher
refusals of uvc_amd.stage1.build_teacher that are decided before any model is built."""
import argparse

import pytest
import torch
import torch.nn as nn

from oracle import vit as OV
from uvc_amd.checkpoints import load_pretrained
from uvc_amd.pos_embed import resize_pos_embed

CFG = OV.VitConfig(img_size=32, patch_size=8, num_classes=16, embed_dim=32, depth=2, num_heads=2)


class TableModel(nn.Module):
    """Parameters at the dotted names of ``shapes``, zero-initialised; ``num_tokens`` as the engine's models have it."""

    def __init__(self, shapes, num_tokens=1):
        super().__init__()
        self.num_tokens = num_tokens
        for name, shp in shapes.items():
            *path, leaf = name.split(".")
            m = self
            for p in path:
                if m._modules.get(p) is None:
                    m.add_module(p, nn.Module())
                m = m._modules[p]
            m.register_parameter(leaf, nn.Parameter(torch.zeros(shp)))


def model(cfg=CFG):
    return TableModel(OV.param_shapes(cfg), cfg.num_tokens)


def weights(cfg=CFG, seed=3):
    return OV.init_params_numpy(cfg, seed)


def params(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def test_layouts_and_module_prefix_load_the_same_tensors(tmp_path, capsys):
    sd = weights()
    got = []
    for ck in ({"model": sd}, {"state_dict_ema": sd, "state_dict": {}}, {"state_dict": sd}, dict(sd),
               {"model": {"module." + k: v for k, v in sd.items()}}, {k: v for k, v in sd.items()} | {"module.x": torch.zeros(1)}):
        m = model()
        rep = load_pretrained(ck, m, num_classes=CFG.num_classes)
        got.append(params(m))
        assert not rep.missing and not rep.dropped
    for g in got:
        assert g.keys() == sd.keys() and all(torch.equal(g[k], sd[k]) for k in sd)
    # the reference's order: "model" before "state_dict_ema" before "state_dict"
    other = weights(seed=4)
    m = model()
    rep = load_pretrained({"state_dict": other, "state_dict_ema": sd}, m, num_classes=CFG.num_classes)
    assert rep.layout == "state_dict_ema" and torch.equal(m.head.weight, sd["head.weight"])
    m = model()
    assert load_pretrained({"model": sd, "state_dict_ema": other}, m, num_classes=CFG.num_classes).layout == "model"
    assert torch.equal(m.head.weight, sd["head.weight"])
    # from a file, as timm's training scripts write it (T2T-ViT's releases): the argparse Namespace rides along
    path = str(tmp_path / "t2t_style.pth.tar")
    torch.save({"epoch": 309, "args": argparse.Namespace(model="t2t_vit_14", lr=1e-3), "state_dict": other,
                "state_dict_ema": {"module." + k: v for k, v in sd.items()}}, path)
    m = model()
    rep = load_pretrained(path, m, num_classes=CFG.num_classes)
    assert rep.layout == "state_dict_ema" and rep.source == path
    assert all(torch.equal(params(m)[k], sd[k]) for k in sd)
    assert f"student: loaded {len(sd)} tensors from {path} (state_dict_ema)" in capsys.readouterr().out


def test_missing_and_unexpected_keys_are_reported(capsys):
    sd = weights()
    public = {k: v for k, v in sd.items() if k not in ("block_skip_gating", "gumbel.weight", "gumbel.bias")}
    public["head_dist.weight"] = torch.zeros(CFG.num_classes, CFG.embed_dim)
    m = model()
    before = params(m)
    rep = load_pretrained(public, m, num_classes=CFG.num_classes, what="teacher")
    assert sorted(rep.missing) == ["block_skip_gating", "gumbel.bias", "gumbel.weight"]
    assert rep.unexpected == ["head_dist.weight"]
    assert torch.equal(m.block_skip_gating, before["block_skip_gating"])        # keeps its init
    out = capsys.readouterr().out
    assert "teacher: missing keys" in out and "teacher: unexpected keys (ignored): ['head_dist.weight']" in out
    load_pretrained(public, model(), num_classes=CFG.num_classes, verbose=False)
    assert capsys.readouterr().out == ""


def test_head_of_another_class_count_is_dropped(capsys):
    imagenet = OV.VitConfig(**{**CFG.__dict__, "num_classes": 1000})
    sd = weights(imagenet)
    m = model()
    init = params(m)
    rep = load_pretrained({"model": sd}, m, num_classes=CFG.num_classes)
    assert sorted(rep.dropped) == ["head.bias", "head.weight"] and sorted(rep.missing) == ["head.bias", "head.weight"]
    got = params(m)
    assert torch.equal(got["head.weight"], init["head.weight"]) and torch.equal(got["head.bias"], init["head.bias"])
    for k in sd:
        if not k.startswith("head."):
            assert torch.equal(got[k], sd[k]), k
    out = capsys.readouterr().out
    assert out.count("1000-class head, the model 16: head.weight, head.bias not loaded (seeded init kept)") == 1


def test_pos_embed_is_resampled_to_the_model_grid(capsys):
    big = OV.VitConfig(**{**CFG.__dict__, "img_size": 64})                       # 8 x 8 patch grid into the model's 4 x 4
    sd = weights(big)
    m = model()
    load_pretrained(sd, m, num_classes=CFG.num_classes)
    want = resize_pos_embed(sd, (4, 4), 1)["pos_embed"]
    assert m.pos_embed.shape == (1, 17, CFG.embed_dim) and torch.equal(m.pos_embed.detach(), want)
    assert torch.equal(m.pos_embed.detach()[:, :1], sd["pos_embed"][:, :1])     # class-token row kept bit for bit
    assert "pos_embed: resized from (1, 65, 32) to (1, 17, 32)" in capsys.readouterr().out


def test_non_head_shape_mismatch_names_the_key():
    sd = weights()
    sd["blocks.1.mlp.fc1.weight"] = torch.zeros(CFG.hidden + 8, CFG.embed_dim)
    with pytest.raises(ValueError, match=r"blocks\.1\.mlp\.fc1\.weight: file \(136, 32\), model \(128, 32\)"):
        load_pretrained({"model": sd}, model(), num_classes=CFG.num_classes)
    wide = weights(OV.VitConfig(**{**CFG.__dict__, "embed_dim": 64}))           # another width: the head too, at the same class count
    with pytest.raises(ValueError, match=r"head\.weight: file \(16, 64\), model \(16, 32\)"):
        load_pretrained(wide, model(), num_classes=CFG.num_classes)


def test_file_without_matching_block_weights_raises(tmp_path):
    sd = weights()
    stem_only = {k: v for k, v in sd.items() if not k.startswith("blocks.")}
    with pytest.raises(ValueError, match="no blocks"):
        load_pretrained(stem_only, model(), num_classes=CFG.num_classes)
    with pytest.raises(ValueError, match="no blocks"):
        load_pretrained({"optimizer": {"state": {}}, "epoch": 3}, model(), num_classes=CFG.num_classes)
    renamed = {"encoder.layer." + k[len("blocks."):]: v for k, v in sd.items() if k.startswith("blocks.")}
    path = str(tmp_path / "vit_b16.pth")
    torch.save(renamed, path)
    with pytest.raises(ValueError, match="wrong --model_type"):
        load_pretrained(path, model(), num_classes=CFG.num_classes)


def test_url_is_refused_without_a_download():
    for url in ("https://dl.fbaipublicfiles.com/deit/deit_tiny_distilled_patch16_224-b40b3cf7.pth", "http://example.invalid/x.pth"):
        with pytest.raises(ValueError, match="does not download"):
            load_pretrained(url, model(), num_classes=CFG.num_classes)


def test_teacher_refusals_before_any_model_is_built():
    from uvc_amd.stage1 import build_teacher, default_args
    micro = {"patch_size": 16, "embed_dim": 128, "depth": 2, "num_heads": 2}
    a = default_args(model_type="custom", model_cfg=micro, img_size=64, num_classes=16)
    for tcfg, what in (({**micro, "img_size": 96}, "img_size 96"), ({**micro, "num_classes": 1000}, "1000 logits")):
        a.teacher_model, a.teacher_cfg = "custom", tcfg
        with pytest.raises(ValueError, match=what):
            build_teacher(a, "cpu")
    a.teacher_model, a.teacher_cfg = "deit_small_patch16_224", '{"embed_dim": 192}'
    with pytest.raises(ValueError, match="--teacher_cfg goes with --teacher-model custom"):
        build_teacher(a, "cpu")
    a.teacher_model, a.teacher_cfg = "custom", {**micro, "embed_dim": 192}
    with pytest.raises(ValueError, match="has no weights: pass --teacher-path"):
        build_teacher(a, "cpu")
    a.teacher_model, a.teacher_cfg = "vit_b16", None
    with pytest.raises(ValueError, match="not in this engine's configs"):
        build_teacher(a, "cpu")
