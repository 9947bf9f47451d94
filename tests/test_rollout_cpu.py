"""CPU: the written spec of the attention rollout maps (uvc_amd/compact.py: reference_rollout) against the explicit matrix product it
stands for, on the compact exports of the Stage-2 fixture states, and the ``explain`` parser.  No GPU."""
import argparse

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import scenarios as SC
from compact_train_ref import fixture_export
from uvc_amd import compact as CP

# Both sides are float64 sums of at most N = 198 products of numbers in [0, 1] per entry, through at most L = 12 blocks, in different
# association orders: N * L * 2^-53 = 2.6e-13 bounds the difference; the rows-sum-to-1 bar of 1e-12 covers it.
TOL = 1e-12
FIXTURES = ["stage2_micro_skip", "stage2_micro_deit", "stage2_micro_none", "stage2_tiny8"]
_CACHE = {}


def fixture(name):
    """(export, float64 batch of two of the fixture's images), built once."""
    if name not in _CACHE:
        r, _, ex, _ = fixture_export(name)
        x_all, _ = SC.make_inputs(r)
        _CACHE[name] = (ex, torch.from_numpy(x_all[0]).double()[:2])
    return _CACHE[name]


def attention_matrices(export, x):
    """The head-mean attention [B, N, N] of every block with heads, restated apart from compact.py's block loop: the hidden states of
    the blocks come from forward hooks on nothing -- the loop is written out again, attention only."""
    cfg, P = export["cfg"], {k: v.to(x.dtype) for k, v in export["state_dict"].items()}
    B, D, eps = x.shape[0], cfg["embed_dim"], cfg["ln_eps"]
    t = F.conv2d(x, P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], stride=cfg["patch_size"]).flatten(2).transpose(1, 2)
    if cfg["patch_gating"]:
        pg = torch.sigmoid(P["patch_gating"])
        if cfg["patch_hard"]:
            m = (pg >= 0.5).to(t.dtype).clone()
            m[:, 0] = 1
            t = t * m
        else:
            t = t * pg
    toks = [P["cls_token"].expand(B, -1, -1)] + ([P["dist_token"].expand(B, -1, -1)] if cfg["enable_dist"] else [])
    h = torch.cat(toks + [t], dim=1) + P["pos_embed"]
    N = h.shape[1]
    out = []
    for k, b in enumerate(export["blocks"]):
        p = f"blocks.{k}."
        nh, dv = len(b["heads"]), b["v_dim"]
        if nh:
            a = F.layer_norm(h, (D,), P[p + "norm1.weight"], P[p + "norm1.bias"], eps)
            qkv = F.linear(a, P[p + "attn.qkv.weight"], P[p + "attn.qkv.bias"])
            att = torch.stack([torch.softmax(qkv[..., j * 64:(j + 1) * 64] @ qkv[..., (nh + j) * 64:(nh + j + 1) * 64].transpose(1, 2) / 8.0, dim=-1)
                               for j in range(nh)], dim=1)                                     # [B, nh, N, N], one head at a time
            v = qkv[..., 2 * nh * 64:].reshape(B, N, nh, dv).transpose(1, 2)
            h = h + F.linear((att @ v).transpose(1, 2).reshape(B, N, nh * dv), P[p + "attn.proj.weight"], P[p + "attn.proj.bias"])
            out.append(att.mean(dim=1))
        else:
            h = h + P[p + "attn.proj.bias"]
        if b["hidden"]:
            m = F.layer_norm(h, (D,), P[p + "norm2.weight"], P[p + "norm2.bias"], eps)
            h = h + F.linear(F.gelu(F.linear(m, P[p + "mlp.fc1.weight"], P[p + "mlp.fc1.bias"])), P[p + "mlp.fc2.weight"], P[p + "mlp.fc2.bias"])
        else:
            h = h + P[p + "mlp.fc2.bias"]
    return out


def explicit_product(atts):
    """A~_L ... A~_1 with A~ = A / 2 + I / 2, as full [B, N, N] matrices."""
    N = atts[0].shape[-1]
    eye = torch.eye(N, dtype=torch.float64)
    prod = eye.expand(atts[0].shape[0], N, N)
    for a in atts:                       # block 1 first: each later block multiplies from the left
        prod = (0.5 * a + 0.5 * eye) @ prod
    return prod


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_rollout_is_the_readout_row_of_the_explicit_product(name):
    ex, x = fixture(name)
    ntok = 2 if ex["cfg"]["enable_dist"] else 1
    atts = attention_matrices(ex, x)
    assert len(atts) == sum(1 for b in ex["blocks"] if b["heads"]) >= 1
    got = CP.reference_rollout(ex, x)
    assert got.dtype == torch.float64 and tuple(got.shape) == (2, CP._seq(ex["cfg"]))
    assert float(got.min()) >= 0.0 and float((got.sum(1) - 1).abs().max()) <= 1e-12
    prod = explicit_product(atts)
    want = prod[:, 0] if ntok == 1 else (prod[:, 0] + prod[:, 1]) / 2
    err = float((got - want).abs().max())
    print(f"{name}: rollout against the explicit product {err:.2e}")
    assert err <= TOL
    last = CP.reference_rollout(ex, x, method="last")
    want_last = atts[-1][:, 0] if ntok == 1 else (atts[-1][:, 0] + atts[-1][:, 1]) / 2
    assert float((last - want_last).abs().max()) <= TOL and float((last.sum(1) - 1).abs().max()) <= 1e-12
    assert (name == "stage2_micro_deit") == (ntok == 2)
    with pytest.raises(ValueError):
        CP.reference_rollout(ex, x, method="max")


def test_reference_rollout_shares_the_forward_of_reference_logits():
    ex, x = fixture("stage2_micro_deit")
    o, od = CP.reference_logits(ex, x)
    o2, od2, atts = CP._reference_walk(ex, x, keep_attention=True)
    assert torch.equal(o, o2) and torch.equal(od, od2) and len(atts) == sum(1 for b in ex["blocks"] if b["heads"])
    assert CP._reference_walk(ex, x)[2] == []


def test_a_block_without_heads_is_the_identity():
    """An export whose middle block keeps no head: its map is the recursion over the other blocks' attention alone."""
    ex, x = fixture("stage2_tiny8")
    k = 1
    assert len(ex["blocks"]) >= 3 and ex["blocks"][k]["heads"]
    sd = {n: v.clone() for n, v in ex["state_dict"].items()}
    D = ex["cfg"]["embed_dim"]
    sd[f"blocks.{k}.attn.qkv.weight"], sd[f"blocks.{k}.attn.qkv.bias"] = torch.zeros(0, D), torch.zeros(0)
    sd[f"blocks.{k}.attn.proj.weight"] = torch.zeros(D, 0)
    blocks = [dict(b) for b in ex["blocks"]]
    blocks[k].update(heads=[], v_index=[], v_dim=0)
    cut = dict(ex, blocks=blocks, state_dict=sd)
    atts = attention_matrices(cut, x)
    assert len(atts) == len(attention_matrices(ex, x)) - 1
    got = CP.reference_rollout(cut, x)
    ntok = 2 if ex["cfg"]["enable_dist"] else 1
    r = torch.zeros_like(got)
    r[:, :ntok] = 1.0 / ntok
    for a in reversed(atts):
        r = 0.5 * r + 0.5 * torch.einsum("bi,bij->bj", r, a)
    assert float((got - r).abs().max()) <= TOL and float((got.sum(1) - 1).abs().max()) <= 1e-12
    assert float((got - CP.reference_rollout(ex, x)).abs().max()) > 1e-6          # and the block's attention did count before


def test_explain_parser():
    p = CP._parser()
    sub = [a for a in p._actions if isinstance(a, argparse._SubParsersAction)][0]
    assert list(sub.choices)[-2:] == ["predict", "explain"]
    # (a range-checked int is a new closure per parser: compared by the function that made it and by what it refuses below)
    flags = lambda q: {a.dest: (tuple(a.option_strings), a.default, getattr(a.type, "__qualname__", a.type), a.nargs, a.required,
                                None if a.choices is None else tuple(a.choices), a.help) for a in q._actions if a.dest != "help"}
    pred, expl = flags(sub.choices["predict"]), flags(sub.choices["explain"])
    assert set(expl) - set(pred) == {"method", "overlay_dir"} and set(pred) <= set(expl)
    assert all(expl[d] == pred[d] for d in pred)
    assert expl["method"][1] == "rollout" and expl["method"][5] == ("rollout", "last") and expl["overlay_dir"][1] is None
    a = p.parse_args(["explain", "--compact", "m", "--images", "a.png", "d", "--method", "last", "--overlay_dir", "o", "--output", "maps.jsonl"])
    assert (a.cmd, a.method, a.overlay_dir, a.output, a.images) == ("explain", "last", "o", "maps.jsonl", ["a.png", "d"])
    b = p.parse_args(["predict", "--compact", "m", "--images", "a.png"])
    assert not hasattr(b, "method") and not hasattr(b, "overlay_dir")


@pytest.mark.parametrize("argv", [["--compact", "m"], ["--compact", "m", "--images"], ["--images", "a"],
                                  ["--compact", "m", "--images", "a", "--method", "max"], ["--compact", "m", "--images", "a", "--topk", "17"],
                                  ["--compact", "m", "--images", "a", "--batch_size", "0"], ["--compact", "m", "--images", "a", "--crop_pct", "1.5"]],
                         ids=["no_images", "empty_images", "no_compact", "method", "topk_17", "batch_size_0", "crop_pct_1.5"])
def test_explain_parser_refusals(argv, capsys):
    with pytest.raises(SystemExit) as e:
        CP._parser().parse_args(["explain", *argv])
    assert e.value.code == 2
    capsys.readouterr()


def test_write_overlay(tmp_path):
    """The overlay is the model's view (resize + centre crop) with red where the map is large and the picture where it is zero."""
    from PIL import Image
    pixels = np.full((40, 60, 3), 200, dtype=np.uint8)
    m = np.zeros((2, 2))
    m[0, 0] = 0.3
    path = CP.write_overlay(str(tmp_path), 3, "dir/pic.jpg", pixels, m, 32)
    assert path.endswith("3_pic.jpg.png")
    im = np.asarray(Image.open(path))
    assert im.shape == (32, 32, 3)
    assert tuple(im[31, 31]) == (200, 200, 200)                                   # zero map: the picture
    r, g, b = (int(v) for v in im[0, 0])
    assert r > 200 and g < 200 and g == b                                         # the map's maximum: blended towards red
    CP.write_overlay(str(tmp_path), 4, "z.png", pixels, np.zeros((2, 2)), 32, preset="cifar")
    assert np.array_equal(np.asarray(Image.open(tmp_path / "4_z.png.png")), np.full((32, 32, 3), 200, dtype=np.uint8))
