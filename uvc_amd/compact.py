"""Compact models: a pruned DeiT exported at its kept widths, and an inference module that runs it on MI355X.

UVC's masks define a smaller network than the dense model that carries them (uvc_utils.py:409-471): heads removed, value dims
removed inside the kept heads, MLP units removed, blocks skipped.  Every removed term meets only exact zeros of the masked
weights, so dropping it changes nothing but the summation order:

- value dim c of a block: its ``attn.proj`` mask column c is all zero -> v-row ``2D + c`` of ``attn.qkv`` and proj column c go;
- head h: all 64 of its proj mask columns are zero -> its q, k, v rows and proj columns go (q and k of kept heads keep 64 dims);
- MLP unit j: the ``mlp.fc2`` mask column j is all zero -> fc1 row j, ``b1[j]`` and fc2 column j go;
- block i: skipped where the Stage-2 eval skips it (``block_skip_gating[i][1] <= [i][0]``, model_distilled.py:496-500).

Padding is exact too: a block's value width ``v_dim`` is the largest kept-dim count of its kept heads rounded up to 16 (heads
with fewer dims get zero v-rows and zero proj columns); the MLP width is rounded up to ``mlp_multiple`` with zero fc1 rows,
zero ``b1`` and zero fc2 columns (GELU(0) = 0 meets a zero column).

    python -m uvc_amd.compact export --model_type ... --checkpoint_dir CK --output model.compact.pt
    python -m uvc_amd.compact eval --compact model.compact.pt [--synthetic 0 --dataset ... --data_dir ...]
    python -m uvc_amd.compact finetune --compact model.compact.pt --output tuned.compact.pt [Stage 2's flags]
    python -m uvc_amd.compact predict --compact model.compact.pt --images PATH [PATH ...] [--output preds.jsonl]
    python -m uvc_amd.compact explain --compact model.compact.pt --images PATH [PATH ...] [--output maps.jsonl] [--overlay_dir DIR]
    python -m uvc_amd.compact attribute --compact model.compact.pt --images PATH [PATH ...] [--target INT] [--output maps.jsonl] [--overlay_dir DIR]

``reference_forward`` is the written spec of the format (plain PyTorch, CPU or GPU, any dtype); ``CompactVisionTransformer``
runs it through ``uvc_vit_compact_forward`` (include/uvc_vit.h).  ``predict`` classifies image files with it (file -> eval transform -> patch rows -> compact forward -> softmax + top-k, all of it
behind the decode on the device).  ``reference_logits`` is the same network with the two heads kept
apart: the function ``compact_train.CompactTrainer`` fine-tunes (a fine-tuned file is an ordinary version-1 compact file).
``explain`` adds to ``predict``'s records what the model looked at: the attention rollout of the readout token(s) over the patches
(``uvc_vit_compact_rollout``; ``reference_rollout`` is its written spec).  ``attribute`` maps the patches that speak for ONE label, the
gradient-weighted rollout (``uvc_vit_compact_attribution`` through ``compact_attribution.CompactAttributionViT``; ``reference_attribution``).
Whether such a map is faithful -- the perturbation test, deletion curves and their areas -- is ``python -m uvc_amd.compact_perturb``.
Another label set -- the model's features for a dataset (``CompactVisionTransformer.features``), their k-NN top-1 and a new head that
``finetune`` trains -- is ``python -m uvc_amd.compact_transfer``.  A file that is still too large -- Taylor scores of its kept heads and
units, and the smaller file they imply -- is ``python -m uvc_amd.compact_prune``.
"""
from __future__ import annotations

import argparse
import copy
import ctypes as C
import json
import math
from typing import Dict, List, Mapping, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

FORMAT, VERSION = "uvc-compact-vit", 1
HEAD_DIM = 64
# MLP widths are rounded up to this multiple (zero padding is exact).  64 keeps the padding small; see DESIGN.md section 8 for
# which GEMM kernel each compact width selects.
MLP_MULTIPLE = 64


def _state_of(model):
    """(state dict, patch_hard) of a dense model or of a state dict (its ``*.mask`` entries included)."""
    if isinstance(model, Mapping):
        sd, hard = dict(model), False
    else:
        if type(model).__name__ == "T2T_ViT" or hasattr(model, "tokens_to_token"):
            raise NotImplementedError("compact export of T2T-ViT models (their tokens-to-token front end) is not supported")
        sd, hard = model.state_dict(), bool(getattr(model, "patch_hard", False))
    if any(k.startswith("tokens_to_token.") for k in sd):
        raise NotImplementedError("compact export of T2T-ViT models (their tokens-to-token front end) is not supported")
    return {k: v.detach().float().cpu() for k, v in sd.items()}, hard


def _cfg_of(sd, patch_hard):
    D = sd["cls_token"].shape[-1]
    pw = sd["patch_embed.proj.weight"]
    ntok = 2 if "dist_token" in sd else 1
    npatch = sd["pos_embed"].shape[1] - ntok
    side = int(round(math.sqrt(npatch)))
    depth = sd["block_skip_gating"].shape[0]
    if D % HEAD_DIM:
        raise ValueError("compact models need head_dim 64 (embed_dim % 64 == 0)")
    return dict(img_size=side * pw.shape[-1], patch_size=pw.shape[-1], in_chans=pw.shape[1], num_classes=sd["head.weight"].shape[0],
                embed_dim=D, depth=depth, num_heads=D // HEAD_DIM, hidden=sd["blocks.0.mlp.fc1.weight"].shape[0], enable_dist=int(ntok == 2),
                patch_gating=int("patch_gating" in sd), patch_hard=int(bool(patch_hard)), ln_eps=1e-6)


def _masked(sd, name):
    """``weight * mask`` (post_train.py:343-346) of a module's weight; other tensors as they are."""
    t = sd[name]
    if name.endswith(".weight"):
        m = sd.get(name[: -len("weight")] + "mask")
        if m is not None:
            t = t * m
    return t


def _round_up(n, m):
    return -(-n // m) * m


def compact_plan(model, mlp_multiple: int = MLP_MULTIPLE) -> dict:
    """The compact model the masks of a dense model imply (after ``apply_masks()``).  ``model``: a DistilledVisionTransformer, or a
    state dict with its ``*.mask`` buffers.  Per source block: whether it runs, the kept heads, each kept head's kept value dims, the
    padded value width ``v_dim`` (16 / 32 / 48 / 64, 0 without heads), the kept MLP units and the padded hidden width."""
    sd, hard = _state_of(model)
    cfg = _cfg_of(sd, hard)
    cfg["mlp_multiple"] = int(mlp_multiple)
    D, H, Fh = cfg["embed_dim"], cfg["num_heads"], cfg["hidden"]
    blocks = []
    for i in range(cfg["depth"]):
        p = f"blocks.{i}."
        g = sd["block_skip_gating"][i]
        mp = sd.get(p + "attn.proj.mask")
        cols = torch.ones(D, dtype=torch.bool) if mp is None else (mp != 0).any(dim=0)
        heads, v_index = [], []
        for h in range(H):
            dims = torch.nonzero(cols[h * HEAD_DIM:(h + 1) * HEAD_DIM]).flatten().tolist()
            if dims:
                heads.append(h)
                v_index.append(dims)
        v_dim = _round_up(max(len(v) for v in v_index), 16) if heads else 0
        m2 = sd.get(p + "mlp.fc2.mask")
        units = torch.ones(Fh, dtype=torch.bool) if m2 is None else (m2 != 0).any(dim=0)
        hidden_index = torch.nonzero(units).flatten().tolist()
        hidden = min(Fh, _round_up(len(hidden_index), mlp_multiple)) if hidden_index else 0
        blocks.append(dict(source=i, runs=bool(g[1] > g[0]), heads=heads, v_index=v_index, v_dim=v_dim, hidden_index=hidden_index,
                           hidden=hidden))
    return dict(cfg=cfg, blocks=blocks)


def export_compact(model, plan: Optional[dict] = None) -> dict:
    """The self-describing compact file (``torch.save`` it): ``{"format", "version", "cfg", "blocks", "state_dict"}``.  state_dict
    names as the dense model's, blocks renumbered over the blocks that run, compact shapes, masks applied; no masks, gate logits or
    ``gumbel.*``; ``patch_gating`` kept when patch-gating mode 1 is on."""
    sd, _ = _state_of(model)
    plan = plan or compact_plan(model)
    cfg = dict(plan["cfg"])
    D = cfg["embed_dim"]
    out: Dict[str, torch.Tensor] = {}
    for k in ("cls_token", "dist_token", "pos_embed", "patch_gating", "patch_embed.proj.weight", "patch_embed.proj.bias", "norm.weight",
              "norm.bias", "head.weight", "head.bias", "head_dist.weight", "head_dist.bias"):
        if k in sd:
            out[k] = _masked(sd, k).clone()
    blocks = []
    for b in plan["blocks"]:
        if not b["runs"]:
            continue
        k, p = len(blocks), f"blocks.{b['source']}."
        q = f"blocks.{k}."
        for n in ("norm1.weight", "norm1.bias", "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.fc2.bias"):
            out[q + n] = _masked(sd, p + n).clone()
        wq, bq, wp = _masked(sd, p + "attn.qkv.weight"), sd[p + "attn.qkv.bias"], _masked(sd, p + "attn.proj.weight")
        hs, dv = b["heads"], b["v_dim"]
        nh = len(hs)
        qkv_w, qkv_b = torch.zeros(nh * (128 + dv), D), torch.zeros(nh * (128 + dv))
        proj_w = torch.zeros(D, nh * dv)
        for j, (h, dims) in enumerate(zip(hs, b["v_index"])):
            for s in (0, 1):                                   # q, k: all 64 dims
                qkv_w[s * nh * 64 + j * 64:s * nh * 64 + (j + 1) * 64] = wq[s * D + h * 64:s * D + (h + 1) * 64]
                qkv_b[s * nh * 64 + j * 64:s * nh * 64 + (j + 1) * 64] = bq[s * D + h * 64:s * D + (h + 1) * 64]
            src = torch.tensor([2 * D + h * 64 + c for c in dims], dtype=torch.long)
            dst = 2 * nh * 64 + j * dv + torch.arange(len(dims))
            qkv_w[dst], qkv_b[dst] = wq[src], bq[src]
            proj_w[:, j * dv + torch.arange(len(dims))] = wp[:, torch.tensor([h * 64 + c for c in dims], dtype=torch.long)]
        out[q + "attn.qkv.weight"], out[q + "attn.qkv.bias"], out[q + "attn.proj.weight"] = qkv_w, qkv_b, proj_w
        idx = torch.tensor(b["hidden_index"], dtype=torch.long)
        Fk = b["hidden"]
        w1, b1, w2 = torch.zeros(Fk, D), torch.zeros(Fk), torch.zeros(D, Fk)
        if len(idx):
            w1[:len(idx)] = _masked(sd, p + "mlp.fc1.weight")[idx]
            b1[:len(idx)] = sd[p + "mlp.fc1.bias"][idx]
            w2[:, :len(idx)] = _masked(sd, p + "mlp.fc2.weight")[:, idx]
        out[q + "mlp.fc1.weight"], out[q + "mlp.fc1.bias"], out[q + "mlp.fc2.weight"] = w1, b1, w2
        blocks.append(dict(source=b["source"], heads=list(hs), v_index=[list(v) for v in b["v_index"]], v_dim=dv,
                           hidden_index=list(b["hidden_index"]), hidden=Fk))
    return dict(format=FORMAT, version=VERSION, cfg=cfg, blocks=blocks, state_dict=out)


def check_export(export: dict) -> dict:
    if not isinstance(export, dict) or export.get("format") != FORMAT:
        raise ValueError(f"not a {FORMAT} file")
    if export.get("version") != VERSION:
        raise ValueError(f"{FORMAT} version {export.get('version')} is not supported (this build reads version {VERSION})")
    return export


def load_compact(path) -> dict:
    return check_export(torch.load(path, map_location="cpu"))


def as_export(export_or_path) -> dict:
    """The checked compact dict of what a command was handed: the dict itself, or the file at a path."""
    return check_export(export_or_path) if isinstance(export_or_path, dict) else load_compact(export_or_path)


def with_state(export: dict, state_dict: dict, cfg: Optional[dict] = None) -> dict:
    """A compact dict with the given weights (and ``cfg``; default: the source's): ``blocks`` and ``cfg`` are copies, every other value
    is the source's."""
    out = {k: v for k, v in export.items() if k not in ("cfg", "state_dict", "blocks")}
    out.update(cfg=copy.deepcopy(export["cfg"] if cfg is None else cfg), blocks=copy.deepcopy(export["blocks"]), state_dict=state_dict)
    return check_export(out)


def num_labels(cfg, num_labels=None) -> int:
    """The valid logits of a head: ``num_labels`` (default: all ``num_classes``), refused outside the head."""
    nl = cfg["num_classes"] if num_labels is None else int(num_labels)
    if not 1 <= nl <= cfg["num_classes"]:
        raise ValueError(f"num_labels {nl} must lie in [1, {cfg['num_classes']}] (the model's head)")
    return nl


def reference_forward(export: dict, x: torch.Tensor) -> torch.Tensor:
    """Eval logits of a compact model in plain PyTorch, in x's dtype and on x's device: the written spec of the format (the Stage-2 eval
    forward of model_distilled.py:429-531 at the kept widths; ``(x + x_dist) / 2`` with the distillation token)."""
    o, od = reference_logits(export, x)
    return (o + od) / 2


def reference_logits(export: dict, x: torch.Tensor):
    """``(logits, logits_dist)`` of a compact model in plain PyTorch -- the two heads kept apart, as a training loss takes them
    (``logits_dist is logits`` without the distillation token).  Differentiable: state_dict tensors that already have x's dtype and
    device enter the graph as they are, so leaves with ``requires_grad`` receive the compact model's gradients."""
    return _reference_walk(export, x)[:2]


METHODS = ("rollout", "last")
GRAD_METHODS = ("attribution",)                     # class-specific maps: they need a backward (compact_attribution.CompactAttributionViT)


def reference_rollout(export: dict, x: torch.Tensor, method: str = "rollout") -> torch.Tensor:
    """Attention rollout (Abnar & Zuidema 2020) of a compact model's readout token(s) in plain PyTorch: float64 ``[B, N]`` over the
    tokens (class, distillation, patches), every row a probability vector.  The network and its block loop are ``reference_logits``'
    (in x's dtype); per attention block A_l is the mean of the kept heads' materialised softmax, and the class-token row of
    ``(A_L + I) / 2 ... (A_1 + I) / 2`` is the row vector ``r <- r / 2 + r A_l / 2`` pushed back from the last block to the first, in
    float64.  It starts uniform over the readout tokens (token 0; tokens 0 and 1 with the distillation token, whose two heads the eval
    logits average).  A block without heads has no attention: the identity.  ``method="last"``: ``r A_L`` of the last attention
    block alone, the head-mean attention of the readout tokens."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, not {method!r}")
    with torch.no_grad():
        atts = _reference_walk(export, x, keep_attention=True)[2]
    ntok = 2 if export["cfg"]["enable_dist"] else 1
    r = torch.zeros(x.shape[0], _seq(export["cfg"]), dtype=torch.float64, device=x.device)
    r[:, :ntok] = 1.0 / ntok
    for a in reversed(atts):
        ra = torch.einsum("bi,bij->bj", r, a.double())
        if method == "last":
            return ra
        r = 0.5 * r + 0.5 * ra
    return r


def reference_attribution(export: dict, x: torch.Tensor, target=None, num_labels=None):
    """Class-specific relevance maps of a compact model in plain PyTorch -- the gradient-weighted attention rollout of Chefer, Gur & Wolf
    (ICCV 2021, "Generic Attention-Model Explainability", self-attention rule): ``(relevance float64 [B, N], target int64 [B])``.
    y is the eval logit of class t (``head(cls)[t]``, or the mean of the two heads with the distillation token), the network and its block
    loop are ``reference_logits``' (in x's dtype) with every kept head's softmax matrix A_l^h in the autograd graph.  Per block with heads
    ``Abar_l = mean_h (A_l^h * dy/dA_l^h)^+`` -- the full gradient, nothing detached; the ReLU per head and entry, before the head mean --
    and the readout row of ``R_L``, ``R_l = R_{l-1} + Abar_l R_{l-1}`` from ``R_0 = I``, is the row vector ``r <- r + r Abar_l`` pushed
    back from the last block to the first, in float64, from the uniform vector over the readout tokens (as ``reference_rollout``).  A block
    without heads is the identity.  The map is non-negative and NOT normalised: every row sums to at least 1, every readout entry is at
    least 1 / ntok.  ``target``: an int, or B indices (sequence or tensor); None: the argmax of the eval logits over the first
    ``num_labels`` columns (default num_classes), ties to the lowest index."""
    cfg = check_export(export)["cfg"]
    nl = cfg["num_classes"] if num_labels is None else int(num_labels)
    if not 1 <= nl <= cfg["num_classes"]:
        raise ValueError(f"num_labels {nl} must lie in [1, {cfg['num_classes']}] (the model's head)")
    B = x.shape[0]
    with torch.enable_grad():
        xg = x.detach().clone().requires_grad_(True)              # a leaf above every softmax matrix: they all join the graph
        o, od, atts = _reference_walk(export, xg, keep_heads=True)
        logits = (o + od) / 2 if cfg["enable_dist"] else o
        if target is None:
            z = logits.detach()[:, :nl]
            cols = torch.arange(nl, device=z.device).expand(B, nl)
            t = torch.where(z == z.max(dim=1, keepdim=True).values, cols, torch.full_like(cols, nl)).min(dim=1).values
        else:
            t = torch.as_tensor(target, dtype=torch.int64, device=x.device).reshape(-1)
            t = t.expand(B) if t.numel() == 1 else t
            if t.numel() != B or int(t.min()) < 0 or int(t.max()) >= nl:
                raise ValueError(f"target must be {B} indices in [0, {nl}), not {t.tolist()}")
        grads = torch.autograd.grad(logits.gather(1, t[:, None]).sum(), atts) if atts else ()
    ntok = 2 if cfg["enable_dist"] else 1
    r = torch.zeros(B, _seq(cfg), dtype=torch.float64, device=x.device)
    r[:, :ntok] = 1.0 / ntok
    for a, g in zip(reversed(atts), reversed(grads)):
        abar = (a.detach().double() * g.double()).clamp_min(0).mean(dim=1)
        r = r + torch.einsum("bi,bij->bj", r, abar)
    return r, t.clone()


def _reference_walk(export: dict, x: torch.Tensor, keep_attention: bool = False, keep_heads: bool = False, keep_readout: bool = False):
    """The block loop behind ``reference_logits``, ``reference_rollout`` and ``reference_attribution``: ``(logits, logits_dist, atts)``;
    with ``keep_attention`` ``atts`` lists the head-mean softmax ``[B, N, N]`` of every block that has heads, in block order, with
    ``keep_heads`` the per-head softmax ``[B, H_l, N, N]`` itself, the very tensor the block goes on with (else it is empty).
    ``keep_readout`` appends a fourth item, the final-norm readout rows ``[B, ntok, D]`` the heads read (``compact_transfer``)."""
    check_export(export)
    cfg = export["cfg"]
    P = {k: v.to(device=x.device, dtype=x.dtype) for k, v in export["state_dict"].items()}
    B, D, eps = x.shape[0], cfg["embed_dim"], cfg["ln_eps"]
    t = F.conv2d(x, P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], stride=cfg["patch_size"]).flatten(2).transpose(1, 2)
    if cfg["patch_gating"]:                                               # mode 1 (:434-444)
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
    atts = []
    for k, b in enumerate(export["blocks"]):
        p = f"blocks.{k}."
        nh, dv = len(b["heads"]), b["v_dim"]
        if nh:
            a = F.layer_norm(h, (D,), P[p + "norm1.weight"], P[p + "norm1.bias"], eps)
            qkv = F.linear(a, P[p + "attn.qkv.weight"], P[p + "attn.qkv.bias"])
            q = qkv[..., :nh * 64].reshape(B, N, nh, 64).transpose(1, 2)
            kk = qkv[..., nh * 64:2 * nh * 64].reshape(B, N, nh, 64).transpose(1, 2)
            v = qkv[..., 2 * nh * 64:].reshape(B, N, nh, dv).transpose(1, 2)
            att = ((q @ kk.transpose(-2, -1)) * HEAD_DIM ** -0.5).softmax(dim=-1)
            if keep_heads:
                atts.append(att)
            elif keep_attention:
                atts.append(att.mean(dim=1))
            o = (att @ v).transpose(1, 2).reshape(B, N, nh * dv)
            h = h + F.linear(o, P[p + "attn.proj.weight"], P[p + "attn.proj.bias"])
        else:                                                             # no kept head: the branch is proj.bias
            h = h + P[p + "attn.proj.bias"]
        if b["hidden"]:
            m = F.layer_norm(h, (D,), P[p + "norm2.weight"], P[p + "norm2.bias"], eps)
            m = F.gelu(F.linear(m, P[p + "mlp.fc1.weight"], P[p + "mlp.fc1.bias"]))
            h = h + F.linear(m, P[p + "mlp.fc2.weight"], P[p + "mlp.fc2.bias"])
        else:                                                             # no kept unit: the branch is fc2.bias
            h = h + P[p + "mlp.fc2.bias"]
    h = F.layer_norm(h, (D,), P["norm.weight"], P["norm.bias"], eps)
    o = F.linear(h[:, 0], P["head.weight"], P["head.bias"])
    od = F.linear(h[:, 1], P["head_dist.weight"], P["head_dist.bias"]) if cfg["enable_dist"] else o
    if keep_readout:
        return o, od, atts, h[:, :2 if cfg["enable_dist"] else 1]
    return o, od, atts


# ---- MAC bookkeeping (oracle/vit.py:mac_table with per-block widths) ------------------------------------------------------------
def _seq(cfg):
    return (cfg["img_size"] // cfg["patch_size"]) ** 2 + (2 if cfg["enable_dist"] else 1)


def _block_macs(cfg, B, H, v_cols, F_):
    """qkv, q k^T, p v, proj, fc1, fc2 of one block: H heads of 64 q / k dims, v_cols value columns in all, F_ units."""
    N, D = _seq(cfg), cfg["embed_dim"]
    return [B * N * D * (2 * H * 64 + v_cols), N * B * H * N * 64, N * B * N * v_cols, B * N * D * v_cols, F_ * B * N * D, D * B * N * F_]


def embed_macs(cfg, B=1):
    P = (cfg["img_size"] // cfg["patch_size"]) ** 2
    return B * P * cfg["embed_dim"] * cfg["patch_size"] ** 2 * cfg["in_chans"]


def full_macs(cfg, B=1) -> int:
    """The dense model's MACs (every block runs)."""
    D, H = cfg["embed_dim"], cfg["num_heads"]
    return embed_macs(cfg, B) + cfg["depth"] * sum(_block_macs(cfg, B, H, D, cfg["hidden"]))


def compact_macs(export_or_plan: dict, B=1, padded=True) -> int:
    """MACs of the compact model: with ``padded`` the widths it runs (H_l heads of v_dim value dims, the padded hidden width), else
    the widths the masks imply (every kept head's own kept dims, the kept units) -- comparable to Stage 1's "Real FLOPs"."""
    cfg = export_or_plan["cfg"]
    total = embed_macs(cfg, B)
    for b in export_or_plan["blocks"]:
        if not b.get("runs", True):
            continue
        H = len(b["heads"])
        v = H * b["v_dim"] if padded else sum(len(d) for d in b["v_index"])
        f = b["hidden"] if padded else len(b["hidden_index"])
        total += sum(_block_macs(cfg, B, H, v, f))
    return int(total)


# ---- seeded synthetic masks (tests and tools/compact_eval_time.py) ----------------------------------------------------------------
def synthetic_masks(depth, embed_dim, hidden, seed=0, keep=0.5):
    """A mask set that keeps about ``keep`` of a DeiT's block MACs and produces every case of the format: pruned heads, partial value
    dims (v_dim 16 / 32 / 48 across blocks), pruned MLP units (kept widths off the multiple) and two skipped blocks (depth >= 6).
    Returns {state_dict key: tensor} for ``attn.proj.mask``, ``mlp.fc1.mask``, ``mlp.fc2.mask`` and ``block_skip_gating``."""
    g = torch.Generator().manual_seed(seed)
    H, D = embed_dim // HEAD_DIM, embed_dim
    out = {}
    gate = torch.tensor([-1.0, 1.0]).repeat(depth, 1)
    skipped = {depth // 3, (2 * depth) // 3} if depth >= 6 else set()
    for i in skipped:
        gate[i] = torch.tensor([1.0, -1.0])
    out["block_skip_gating"] = gate
    dv_cycle = [48, 32, 16, 64]
    for i in range(depth):
        p = f"blocks.{i}."
        pm = torch.zeros(D, D)
        nkeep = max(1, H - max(1, H // 4)) if H > 1 else 1
        heads = sorted(torch.randperm(H, generator=g)[:nkeep].tolist())
        dv = dv_cycle[i % len(dv_cycle)]
        for j, h in enumerate(heads):
            nd = dv - (j % 2) * 5 if dv > 16 else dv - (j % 2) * 3     # kept dims below the padded width for some heads
            dims = torch.randperm(64, generator=g)[:nd]
            pm[:, h * 64 + dims] = 1.0
        out[p + "attn.proj.mask"] = pm
        nunit = max(1, int(round(hidden * keep)) - 37 * (i % 2))
        units = torch.randperm(hidden, generator=g)[:nunit]
        m2 = torch.zeros(D, hidden)
        m2[:, units] = 1.0
        out[p + "mlp.fc2.mask"] = m2
        out[p + "mlp.fc1.mask"] = torch.ones(hidden, D)                   # live fc1 rows: the unit still goes (fc2 column decides)
    return out


def apply_synthetic_masks(model, masks):
    """Load ``masks`` into a dense model's mask buffers (registering them where missing) and its gate logits, then apply them."""
    from .post_train import register_masks
    register_masks(model)
    sd = model.state_dict()
    for k, v in masks.items():
        sd[k] = v.to(sd[k].dtype)
    model.load_state_dict(sd)
    model.apply_masks()
    return model


# ---- the MI355X module ----------------------------------------------------------------------------------------------------------
_SLOTS = ["norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "norm2.weight",
          "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias"]      # uvc_vit_offsets.blk[k][0..11]


def _bind():
    """The library with the argument types of the compact entry points (include/uvc_vit.h, uvc_vit_compact_*) set."""
    from . import _lib as L
    from .model_distilled import uvc_vit_cfg, uvc_vit_io, uvc_vit_offsets, uvc_vit_shadow_offsets
    lib = L.lib()
    if not getattr(lib, "_compact_bound", False):
        head = [C.POINTER(uvc_vit_cfg), C.POINTER(L.uvc_compact_block), C.c_int32]
        run = [C.POINTER(uvc_vit_io), C.c_void_p]
        tails = {"layout": [C.POINTER(uvc_vit_offsets), C.POINTER(uvc_vit_shadow_offsets)], "workspace_bytes": [C.c_int32],
                 "update_shadows": [C.c_void_p, C.c_void_p, C.c_void_p], "forward": run, "train_forward": run, "backward": run,
                 "frozen_ranges": [C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_int32)],
                 "rollout": [C.POINTER(uvc_vit_io), C.c_void_p, C.c_int32, C.c_void_p],
                 "attribution": [C.POINTER(uvc_vit_io), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]}
        for n in ("layout", "workspace_bytes", "update_shadows"):
            tails["train_" + n] = tails[n]
        tails["input_grad"] = tails["attribution"]
        tails["loss_grad"] = [C.POINTER(uvc_vit_io), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        tails["features"] = [C.POINTER(uvc_vit_io), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        tails["gate_grads"] = [C.POINTER(uvc_vit_io), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        tails["rollout_workspace_bytes"] = tails["attribution_workspace_bytes"] = tails["input_grad_workspace_bytes"] = tails["workspace_bytes"]
        tails["gate_grads_workspace_bytes"] = tails["workspace_bytes"]
        for n, tail in tails.items():
            f = getattr(lib, "uvc_vit_compact_" + n)
            f.argtypes, f.restype = head + tail, C.c_int64 if n.endswith("workspace_bytes") else C.c_int
        lib._compact_bound = True
    return lib


class _CompactModule(nn.Module):
    """What the inference module and the trainable one share: the refusals, the C descriptors (``_cfg``, ``_blocks``), ONE flat
    float32 parameter buffer in the layout ``layout`` names (uvc_vit_compact_layout, or the training layout, which appends to it),
    the per-batch workspaces and the eval forward through ``uvc_vit_compact_forward``.  A subclass allocates ``_shadow``."""

    def __init__(self, export: dict, precision: str, device, layout: str, max_tokens=None):
        super().__init__()
        from . import _lib as L
        from . import ops
        from .model_distilled import uvc_vit_cfg, uvc_vit_offsets, uvc_vit_shadow_offsets
        check_export(export)
        if precision == "bf16_f32resid":
            raise NotImplementedError("compact models run in 'bf16' or 'fp32' (the float32 residual rows of 'bf16_f32resid' are a dense-model mode)")
        if precision not in ("bf16", "fp32"):
            raise ValueError("precision must be 'bf16' or 'fp32'")
        dev = torch.device(device if device is not None else "cuda")
        if dev.type != "cuda":
            raise L.UvcHipError("uvc_amd models run on MI355X only (no CPU fallback)")
        c = export["cfg"]
        if max_tokens is not None and _seq(c) > max_tokens:
            raise NotImplementedError(f"fine-tuning a compact model with {_seq(c)} tokens: the attention backward at a value width takes at most "
                                      f"{max_tokens} (384-px and patch-8 files can be evaluated, not trained)")
        self._export, self.precision = export, precision
        self.num_tokens = 2 if c["enable_dist"] else 1
        self._cfg = uvc_vit_cfg(c["img_size"], c["patch_size"], c["in_chans"], c["num_classes"], c["embed_dim"], c["depth"], c["num_heads"],
                                c["hidden"], self.num_tokens, ops.UVC_F32 if precision == "fp32" else ops.UVC_BF16)
        self._cfg.ln_eps = float(c["ln_eps"])
        self._nb = len(export["blocks"])
        self._blocks = (L.uvc_compact_block * max(1, self._nb))()
        for k, b in enumerate(export["blocks"]):
            self._blocks[k].heads, self._blocks[k].v_dim, self._blocks[k].hidden = len(b["heads"]), b["v_dim"], b["hidden"]
        self._off, self._soff = uvc_vit_offsets(), uvc_vit_shadow_offsets()
        L.check(self._lib_call(layout, C.byref(self._off), C.byref(self._soff)), layout)
        flat = torch.zeros(self._off.n_total, dtype=torch.float32)
        for name, t in export["state_dict"].items():
            o = self._offset(name)
            flat[o:o + t.numel()] = t.reshape(-1).float()
        self._flat = flat.to(dev)
        self._ws = {}

    def _lib_call(self, entry, *args):
        """``entry(cfg, blocks, nblocks, *args)`` of the library."""
        return getattr(_bind(), entry)(C.byref(self._cfg), self._blocks, self._nb, *args)

    def _offset(self, name):
        o = self._off
        if name.startswith("blocks."):
            _, k, rest = name.split(".", 2)
            return o.blk[int(k)][_SLOTS.index(rest)]
        return dict(cls_token=o.cls_token, dist_token=o.dist_token, pos_embed=o.pos_embed, patch_gating=o.patch_gating,
                    **{"patch_embed.proj.weight": o.patch_w, "patch_embed.proj.bias": o.patch_b, "norm.weight": o.norm_w, "norm.bias": o.norm_b,
                       "head.weight": o.head_w, "head.bias": o.head_b, "head_dist.weight": o.headd_w, "head_dist.bias": o.headd_b})[name]

    def num_params(self) -> int:
        return sum(int(t.numel()) for k, t in self._export["state_dict"].items() if k != "patch_gating")

    def macs(self, B=1) -> int:
        return compact_macs(self._export, B, padded=True)

    def _refresh_shadows(self):
        """Bring ``_shadow`` up to date with ``_flat`` before a run (the inference module's weights never change)."""

    def _prep(self, x):
        from . import _lib as L
        L.require_cuda(x)
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.contiguous().float()
        c = self._export["cfg"]
        if tuple(x.shape[1:]) != (c["in_chans"], c["img_size"], c["img_size"]):
            raise AssertionError(f"Input image size ({x.shape[2]}*{x.shape[3]}) doesn't match model ({c['img_size']}*{c['img_size']}).")
        return x

    def _prep_patches(self, patches):
        """The batch size of ready-made patch rows ([B * np, C * P * P] in the engine's dtype, ops.patchify's layout), checked."""
        from . import _lib as L
        from . import ops
        L.require_cuda(patches)
        c = self._export["cfg"]
        npatch, K = (c["img_size"] // c["patch_size"]) ** 2, c["in_chans"] * c["patch_size"] ** 2
        want = ops.tdtype(self._cfg.dtype)
        if patches.dim() != 2 or patches.shape[1] != K or patches.shape[0] % npatch or patches.shape[0] == 0 or not patches.is_contiguous():
            raise AssertionError(f"patch rows {tuple(patches.shape)} do not match the model: contiguous [B * {npatch}, {K}]")
        if patches.dtype != want:
            raise AssertionError(f"patch rows are {patches.dtype} but the model runs in {want}")
        return patches.shape[0] // npatch

    def _workspace(self, B, training):
        """One workspace per mode (eval, training, "rollout": the eval forward that keeps qkv and lse per block, or "attribution": the
        training set plus what the relevance walk adds, or "input_grad": the training set plus what the walk down to the patch rows adds, or
        "gate_grads": the training set plus the float32 fc2 dgrad of the gate walk), for the last batch size seen."""
        mode = training if isinstance(training, str) else bool(training)
        key = (B, mode)
        if key not in self._ws:
            from . import _lib as L
            entry = {False: "uvc_vit_compact_workspace_bytes", True: "uvc_vit_compact_train_workspace_bytes",
                     "rollout": "uvc_vit_compact_rollout_workspace_bytes", "attribution": "uvc_vit_compact_attribution_workspace_bytes",
                     "input_grad": "uvc_vit_compact_input_grad_workspace_bytes", "gate_grads": "uvc_vit_compact_gate_grads_workspace_bytes"}[mode]
            n = self._lib_call(entry, B)
            if n < 0:
                L.check(-1, entry)
            self._ws = {k: v for k, v in self._ws.items() if k[1] != mode}
            self._ws[key] = torch.empty(n, dtype=torch.uint8, device=self._flat.device)
        return self._ws[key]

    def _io(self, x, B, training):
        """(uvc_vit_io of a pass over the prepared batch ``x``, its patch mask or None)."""
        from . import _lib as L
        from . import ops
        from .model_distilled import uvc_vit_io
        c, dev = self._export["cfg"], self._flat.device
        ws = self._workspace(B, training)
        mask = None
        if c["patch_gating"]:
            P = (c["img_size"] // c["patch_size"]) ** 2
            mask = torch.empty(B, P, device=dev)
            o = self._off.patch_gating
            ops.patch_gate_sigmoid(self._flat[o:o + P], mask, B, P, bool(c["patch_hard"]))
        io = uvc_vit_io()
        io.params, io.shadow, io.workspace, io.workspace_bytes = L.ptr(self._flat), L.ptr(self._shadow), L.ptr(ws), ws.numel()
        io.x, io.patch_mask, io.batch, io.training = L.ptr(x), L.ptr(mask), B, int(training is True)
        return io, mask

    def _forward(self, x, training=False, patches=None, rollout=None, features=None):
        """``(logits, logits_dist or None, what a backward needs of the pass)`` through the eval or the training forward.  ``patches``
        (eval only, in place of ``x``): the batch's patch rows, which the forward then does not make itself.  ``rollout`` (eval only;
        0 = rollout, 1 = last): the pass goes through ``uvc_vit_compact_rollout`` and its maps, float32 [B, N], come back as ``"maps"``."""
        from . import _lib as L
        dev = self._flat.device
        if patches is not None:
            if x is not None or training:
                raise ValueError("patch rows stand in for the image batch of an eval forward: pass one of x / patches")
            B = self._prep_patches(patches)
        else:
            x = self._prep(x)
            B = x.shape[0]
        if rollout is not None and training:
            raise ValueError("rollout maps come from the eval forward")
        self._refresh_shadows()
        io, mask = self._io(x, B, "rollout" if rollout is not None else bool(training))
        io.patches_in = L.ptr(patches)                  # (None: the forward rearranges x itself)
        nc = self._export["cfg"]["num_classes"]
        logits = torch.empty(B, nc, device=dev)
        logits_dist = torch.empty(B, nc, device=dev) if self.num_tokens == 2 else None
        io.logits, io.logits_dist = L.ptr(logits), L.ptr(logits_dist)
        if rollout is not None:
            maps = torch.empty(B, _seq(self._export["cfg"]), device=dev)
            L.check(self._lib_call("uvc_vit_compact_rollout", C.byref(io), L.ptr(maps), int(rollout), L.cur_stream()), "uvc_vit_compact_rollout")
            return logits, logits_dist, dict(x=x, B=B, mask=mask, maps=maps)
        if features is not None:      # (eval only; (normalize, dtype)): uvc_vit_compact_features, the forward plus the readout kernel
            if training:
                raise ValueError("features come from the eval forward")
            from . import ops
            feats = torch.empty(B, self._export["cfg"]["embed_dim"], dtype=features[1], device=dev)
            L.check(self._lib_call("uvc_vit_compact_features", C.byref(io), L.ptr(feats), int(features[0]),
                                   ops.UVC_F32 if features[1] == torch.float32 else ops.UVC_BF16, L.cur_stream()), "uvc_vit_compact_features")
            return logits, logits_dist, dict(x=x, B=B, mask=mask, feats=feats)
        entry ="uvc_vit_compact_train_forward" if training else "uvc_vit_compact_forward"
        L.check(self._lib_call(entry, C.byref(io), L.cur_stream()), entry)
        return logits, logits_dist, dict(x=x, B=B, mask=mask)

    @torch.no_grad()
    def _eval_logits(self, x=None, patches=None):
        """The eval logits: ``(x + x_dist) / 2`` with the distillation token."""
        o, od, _ = self._forward(x, patches=patches)
        return o if od is None else (o + od) / 2


class CompactVisionTransformer(_CompactModule):
    """Inference-only compact DeiT over ONE flat float32 parameter buffer (uvc_vit_compact_layout).  ``forward(x)`` returns the eval
    logits (``(x + x_dist) / 2`` with the distillation token) and the compact model's MACs, as the dense model's eval forward does."""

    def __init__(self, export: dict, precision: str = "bf16", device=None):
        from . import _lib as L
        super().__init__(export, precision, device, "uvc_vit_compact_layout")
        self.export = export
        dev = self._flat.device
        self._shadow = torch.empty(max(1, self._soff.n_total) if precision == "bf16" else 1, dtype=torch.bfloat16, device=dev)
        with torch.cuda.device(dev):
            L.check(self._lib_call("uvc_vit_compact_update_shadows", L.ptr(self._flat), L.ptr(self._shadow), L.cur_stream()), "uvc_vit_compact_update_shadows")
        self.eval()

    def forward(self, x=None, *, patches=None):
        """``x`` float32 [B, C, S, S], or ``patches=`` its patch rows [B * np, C * P * P] in the model's dtype (ops.patchify's layout, as
        ``DeviceLoader(output="patches")`` yields them): they feed ``uvc_vit_io.patches_in`` and the forward skips uvc_patchify."""
        logits = self._eval_logits(x, patches)
        return logits, self.macs(logits.shape[0])

    @torch.no_grad()
    def rollout(self, x=None, *, patches=None, method="rollout"):
        """``(eval logits, maps)``: the logits are ``forward``'s bit for bit; ``maps`` float32 [B, N] is the attention rollout of the
        readout token(s) over the model's tokens (``reference_rollout`` is the spec; ``method`` "rollout" or "last"), every row sums
        to 1.  Inputs as ``forward`` takes them."""
        if method not in METHODS:
            raise ValueError(f"method must be one of {METHODS}, not {method!r}")
        o, od, kept = self._forward(x, patches=patches, rollout=METHODS.index(method))
        return (o if od is None else (o + od) / 2), kept["maps"]

    @torch.no_grad()
    def features(self, x=None, *, patches=None, normalize=True, dtype=torch.float32):
        """``(eval logits, feats [B, D])``: the logits are ``forward``'s bit for bit; ``feats`` is the float32 mean of the final-norm
        readout rows the heads read (the class row; ``(cls + dist) / 2`` with the distillation token), divided by ``max(norm, 1e-12)``
        with ``normalize`` (``F.normalize``) -- ``compact_transfer.reference_features`` is the spec.  ``dtype`` torch.float32, or
        torch.bfloat16: the float32 result rounded once.  Inputs as ``forward`` takes them."""
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"dtype must be torch.float32 or torch.bfloat16, not {dtype!r}")
        o, od, kept = self._forward(x, patches=patches, features=(bool(normalize), dtype))
        return (o if od is None else (o + od) / 2), kept["feats"]


# ---- classify image files -------------------------------------------------------------------------------------------------------
MAX_TOPK = 16                                       # uvc_logits_topk's limit
FUSED_INPUT_DEFAULT = 1                             # decided by tools/predict_time.py's rounds (README "Classify images")
PRESETS = ("imagenet", "cifar")
OVERLAY_ALPHA = 160                                 # opacity (of 255) of the red layer where the patch map has its maximum


def read_classes(path) -> List[str]:
    """Class names from a file: a JSON list, or one name per line (blank lines dropped)."""
    with open(path, "r", encoding="utf-8") as f:
        text = f.read()
    if text.lstrip().startswith("["):
        names = json.loads(text)
        if not isinstance(names, list):
            raise ValueError(f"{path}: a JSON class file holds one list of names")
        return [str(n) for n in names]
    return [line.strip() for line in text.splitlines() if line.strip()]


def topk_reference(logits, k, n_valid=None):
    """What ``ops.logits_topk`` computes, in float64 on the host: ``(probs [B, k], index [B, k])`` (numpy) of the softmax over columns
    ``[:n_valid]``, the k largest first, in the stable order ``(-p, index)``.  Tests hold the kernel to it."""
    import numpy as np
    z = np.asarray(logits, dtype=np.float64)
    z = z.reshape(-1, z.shape[-1])[:, :n_valid]
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    index = np.stack([np.lexsort((np.arange(p.shape[1]), -row))[:k] for row in p])
    return np.take_along_axis(p, index, axis=1), index.astype(np.int32)


def _classify(model, files, method, overlay_dir, topk, batch_size, preset, interpolation, crop_pct, num_labels, classes, num_workers, fused_input,
              target=None):
    """The generator behind ``predict`` (``method`` None) and ``explain``: the checked arguments, the tolerant dataset over ``files``,
    the preset's eval loader, the forward (with the rollout maps when a method is given), top-k, one record per file.  ``method``
    "attribution": image batches, ``model.attribution`` for ``target`` (None: every image's top-1 label among ``num_labels``), the
    relevance row divided by its sum (at least 1), and ``"target"`` in the record."""
    from . import data, ops
    if preset not in PRESETS:
        raise ValueError(f"preset must be one of {PRESETS}, not {preset!r}")
    c = model._export["cfg"]
    classes = None if classes is None else list(classes)
    if num_labels is None:
        num_labels = len(classes) if classes is not None else c["num_classes"]
    num_labels, topk = int(num_labels), int(topk)
    if not 1 <= num_labels <= c["num_classes"]:
        raise ValueError(f"num_labels {num_labels} must lie in [1, {c['num_classes']}] (the model's head)")
    if classes is not None and len(classes) < num_labels:
        raise ValueError(f"{len(classes)} class names for {num_labels} labels")
    if not 1 <= topk <= min(MAX_TOPK, num_labels):
        raise ValueError(f"topk {topk} must lie in [1, {min(MAX_TOPK, num_labels)}]")
    grad = method in GRAD_METHODS
    if target is not None and not 0 <= int(target) < num_labels:
        raise ValueError(f"target {target} must lie in [0, {num_labels}) (num_labels)")
    fused_input = bool(fused_input) and not grad              # the backward's forward rearranges the images itself
    ds = files if hasattr(files, "load") else data.FileListDataset(files, tolerant=True)
    names = ds.paths if hasattr(ds, "paths") else list(range(len(ds)))
    errors = getattr(ds, "errors", {})
    dev = model._flat.device
    kw = dict(mean=data.IMAGENET_MEAN, std=data.IMAGENET_STD, eval="center") if preset == "imagenet" else \
        dict(mean=data.CIFAR_MEAN, std=data.CIFAR_STD, eval="square")
    if fused_input:
        kw.update(output="patches", patch_size=c["patch_size"], dtype=ops.tdtype(model._cfg.dtype))
    loader = data.DeviceLoader(ds, int(batch_size), c["img_size"], train=False, num_workers=num_workers, device=dev, interpolation=interpolation,
                               crop_pct=crop_pct, **kw)
    g = c["img_size"] // c["patch_size"]
    ntok = 2 if c["enable_dist"] else 1
    if overlay_dir is not None:
        import os
        os.makedirs(overlay_dir, exist_ok=True)

    def records(first, probs, index, maps, chosen=None):
        for b, (pr, ix) in enumerate(zip(probs.tolist(), index.tolist())):
            i = first + b
            if i in errors:
                yield dict(file=names[i], error=errors[i])
                continue
            rec = dict(file=names[i], top=[dict(index=j, label=None if classes is None else classes[j], prob=q) for j, q in zip(ix, pr)])
            if chosen is not None:
                rec.update(target=int(chosen[b]))
            if maps is not None:
                row = maps[b].tolist()
                rec.update(grid=[g, g], tokens=row[:ntok], map=row[ntok:])
                if overlay_dir is not None:
                    write_overlay(overlay_dir, i, names[i], ds.load(i), maps[b, ntok:].reshape(g, g).numpy(), c["img_size"], preset, interpolation, crop_pct)
            yield rec

    # the records of a batch are read back after the next batch's launches, so the device does not idle behind the host
    first, pending = 0, None
    host = lambda t: None if t is None else t.cpu()
    with torch.cuda.device(dev):
        for x, _ in loader:
            inp = dict(patches=x) if fused_input else dict(x=x)
            chosen = None
            if grad:
                logits, maps, chosen = model.attribution(x, None if target is None else int(target), num_labels)
                maps = maps / maps.sum(dim=1, keepdim=True)
            else:
                logits, maps = (model._eval_logits(**inp), None) if method is None else model.rollout(method=method, **inp)
            probs, index = ops.logits_topk(logits, topk, num_labels)
            if pending is not None:
                yield from records(pending[0], pending[1].cpu(), pending[2].cpu(), host(pending[3]), host(pending[4]))
            pending = (first, probs, index, maps, chosen)
            first += len(probs)
        if pending is not None:
            yield from records(pending[0], pending[1].cpu(), pending[2].cpu(), host(pending[3]), host(pending[4]))


def write_overlay(overlay_dir, index, name, pixels, patch_map, img_size, preset="imagenet", interpolation="bilinear", crop_pct=None):
    """``<overlay_dir>/<index>_<basename>.png``, img_size x img_size: the model's own view of the image (the preset's resize and centre
    crop, or square resize, done with PIL) with the patch map -- divided by its maximum, upsampled bilinearly -- blended in in red.
    ``pixels``: uint8 [H, W, 3]; ``patch_map``: [g, g] non-negative.  Returns the path."""
    import os
    import numpy as np
    from PIL import Image
    from . import data
    S = int(img_size)
    im = Image.fromarray(np.ascontiguousarray(pixels))
    resample = data._pil_filter(interpolation)
    if preset == "cifar":
        im = im.resize((S, S), resample)
    else:
        rh, rw = data.resize_short_side(pixels.shape[0], pixels.shape[1], data.eval_resize_side(S, crop_pct))
        im = im.resize((rw, rh), resample)
        y0, x0 = data.center_crop_offset(rh, rw, S)
        im = im.crop((x0, y0, x0 + S, y0 + S))
    m = np.asarray(patch_map, dtype=np.float64)
    top = float(m.max())
    m = m / top if top > 0 else np.zeros_like(m)
    alpha = Image.fromarray(np.round(m * 255).astype(np.uint8), "L").resize((S, S), Image.BILINEAR)
    alpha = alpha.point(lambda v: v * OVERLAY_ALPHA // 255)
    out = Image.composite(Image.new("RGB", (S, S), (255, 0, 0)), im.convert("RGB"), alpha)
    path = os.path.join(overlay_dir, f"{index}_{os.path.basename(str(name))}.png")
    out.save(path)
    return path


def predict(model, files, *, topk=5, batch_size=64, preset="imagenet", interpolation="bilinear", crop_pct=None, num_labels=None, classes=None,
            num_workers=8, fused_input=bool(FUSED_INPUT_DEFAULT)):
    """Classify image files with a ``CompactVisionTransformer``: yields one record per file, in input order,
    ``{"file", "top": [{"index", "label", "prob"}, ...]}`` with the ``topk`` most probable labels first, or ``{"file", "error"}`` for a file
    that cannot be read (the run goes on).

    preset "imagenet": Resize(eval_resize_side(S, crop_pct)) + CenterCrop(S) with ImageNet's mean / std, ``build_loaders``' test transform;
    "cifar": Resize((S, S)) with 0.5 / 0.5.  ``interpolation`` / ``crop_pct`` as the loaders take them.  The softmax runs over the first
    ``num_labels`` logits (default: ``len(classes)``, else the model's num_classes), so the padding logits of a 16 / 104-wide CIFAR head
    are never reported; ``classes`` names them (``label`` is None without).  ``fused_input``: the resampler writes the patch rows the
    forward reads (uvc_image_prep_patches); False: it writes the float32 images and the forward rearranges them (uvc_image_prep +
    uvc_patchify) -- the same records bit for bit.  ``files``: paths, or a dataset with ``load(i)`` / ``targets`` (records then name indices)."""
    yield from _classify(model, files, None, None, topk, batch_size, preset, interpolation, crop_pct, num_labels, classes, num_workers, fused_input)


def explain(model, files, *, method="rollout", overlay_dir=None, topk=5, batch_size=64, preset="imagenet", interpolation="bilinear", crop_pct=None,
            num_labels=None, classes=None, num_workers=8, fused_input=bool(FUSED_INPUT_DEFAULT), target=None):
    """``predict``'s records plus what the model looked at: ``"grid": [g, g]`` (patches per side), ``"tokens"``: the map's mass on the
    readout token(s) ``[r_cls(, r_dist)]``, ``"map"``: g * g floats, row-major, the mass on every patch -- ``CompactVisionTransformer.rollout``
    with ``method`` "rollout" or "last"; tokens and map sum to 1.  A file that cannot be read stays ``{"file", "error"}``.
    ``overlay_dir``: one PNG per readable image (``write_overlay``), named ``<running index>_<basename>.png``.  The other keywords are
    ``predict``'s.

    ``method="attribution"`` (``GRAD_METHODS``): class-specific maps, which patches speak for ONE label -- ``model`` must be a
    ``compact_attribution.CompactAttributionViT`` (``TypeError`` otherwise); ``target``: the class explained for every image, or None for
    each image's own top-1 label among ``num_labels``.  The record gains ``"target"``; ``"tokens"`` and ``"map"`` are the relevance row
    (``reference_attribution``) divided by its sum, so they still sum to 1.  The loader yields image batches: ``fused_input`` is ignored."""
    if method not in METHODS + GRAD_METHODS:
        raise ValueError(f"method must be one of {METHODS + GRAD_METHODS}, not {method!r}")
    if method in GRAD_METHODS:
        from .compact_attribution import CompactAttributionViT
        if not isinstance(model, CompactAttributionViT):
            raise TypeError(f"method {method!r} needs a CompactAttributionViT, not {type(model).__name__}")
    elif target is not None:
        raise ValueError(f"target goes with method 'attribution': the {method!r} map is the same for every class")
    yield from _classify(model, files, method, overlay_dir, topk, batch_size, preset, interpolation, crop_pct, num_labels, classes, num_workers,
                         fused_input, target)


def _int_in(lo, hi, what):
    def parse(v):
        n = int(v)
        if not lo <= n <= hi:
            raise argparse.ArgumentTypeError(f"{what} must lie in [{lo}, {hi}], not {n}")
        return n
    return parse


def _crop_pct_arg(v):
    from .data import eval_resize_side
    try:
        eval_resize_side(224, float(v))
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))
    return float(v)


def predict_command(args, dev):
    """``predict``, ``explain`` and ``attribute``: one JSON line per image to --output (or stdout), then the summary line
    ``{"images", "errors", "batches", "img_per_s"}``.  ``attribute`` is ``explain`` with method "attribution" on a ``CompactAttributionViT``:
    a file with more than 256 tokens fails here, before any image is listed or read."""
    from . import data
    export = load_compact(args.compact)
    classes = read_classes(args.classes) if args.classes else None
    if args.cmd == "attribute":                     # (its refusal of a long sequence comes first)
        from .compact_attribution import CompactAttributionViT
        cm = CompactAttributionViT(export, precision=args.precision, device=dev)
    files = data.list_images(args.images)
    if args.cmd != "attribute":
        cm = CompactVisionTransformer(export, precision=args.precision, device=dev)
    kw = dict(topk=args.topk, batch_size=args.batch_size, preset=args.preset, interpolation=args.interpolation, crop_pct=args.crop_pct,
              num_labels=args.num_labels, classes=classes, num_workers=args.num_workers, fused_input=bool(args.fused_input))
    if args.cmd == "attribute":
        recs = explain(cm, files, method="attribution", target=args.target, overlay_dir=args.overlay_dir, **kw)
    else:
        recs = explain(cm, files, method=args.method, overlay_dir=args.overlay_dir, **kw) if args.cmd == "explain" else predict(cm, files, **kw)
    return write_records(recs, args.output, batch_size=args.batch_size)


def write_records(records, output, batch_size=None):
    """The JSON-lines writer of the image-file commands: one line per record of the generator ``records`` (nothing of it has run yet) to
    the file ``output`` (None: stdout), which is closed whatever happens.  With ``batch_size`` the summary line ``{"images", "errors",
    "batches", "img_per_s"}`` follows the records and is returned."""
    import sys
    import time
    out = open(output, "w", encoding="utf-8") if output else sys.stdout
    n = nerr = 0
    summary = None
    t0 = time.perf_counter()
    try:
        for rec in records:
            out.write(json.dumps(rec) + "\n")
            n += 1
            nerr += "error" in rec
        if batch_size is not None:
            dt = time.perf_counter() - t0
            summary = dict(images=n, errors=nerr, batches=math.ceil(n / batch_size), img_per_s=n / dt if dt > 0 else 0.0)
            out.write(json.dumps(summary) + "\n")
    finally:
        if out is not sys.stdout:
            out.close()
    return summary


# ---- command line -------------------------------------------------------------------------------------------------------------
def _parser():
    p = argparse.ArgumentParser(prog="python -m uvc_amd.compact", description="Export a pruned DeiT as a compact model, or evaluate one")
    sub = p.add_subparsers(dest="cmd", required=True)
    for name in ("export", "eval"):
        s = sub.add_parser(name)
        s.add_argument("--model_type", default="deit_tiny_patch16_224")
        s.add_argument("--model_cfg", default=None, help="JSON dims for a --model_type outside models/configs.py")
        s.add_argument("--enable_deit", type=int, default=0)
        s.add_argument("--enable_patch_gating", type=int, default=0, help="1: the sigmoid token mask (mode 1) is part of the model")
        s.add_argument("--patch_hard", type=int, default=0)
        s.add_argument("--img_size", type=int, default=224)
        s.add_argument("--num_classes", type=int, default=1000)
        s.add_argument("--checkpoint_dir", default=None, help="Stage-1 / Stage-2 checkpoint (bare state_dict with masks)")
        s.add_argument("--model_path", default=None, help="pretrained checkpoint, when there is no --checkpoint_dir")
        s.add_argument("--mlp_multiple", type=int, default=MLP_MULTIPLE)
        s.add_argument("--precision", default="bf16")
        s.add_argument("--seed", type=int, default=42)
    sub.choices["export"].add_argument("--output", required=True)
    e = sub.choices["eval"]
    e.add_argument("--compact", default=None, help="an exported compact file (else the dense flags are exported on the fly)")
    e.add_argument("--eval_batch_size", type=int, default=64)
    e.add_argument("--eval_steps", type=int, default=2, help="synthetic validation batches")
    e.add_argument("--synthetic", type=int, default=1, help="synthetic batches; 0 = read --dataset under --data_dir")
    from .driver import add_data_flags
    add_data_flags(e, data_dir="/ssd1/xinyu/dataset/imagenet2012", num_workers=8)
    # fine-tune a compact file at its kept widths: Stage 2's training, distillation, teacher, data and Mixup flags (post_train's names and defaults)
    from .post_train import add_stage2_flags
    f = sub.add_parser("finetune")
    f.add_argument("--compact", required=True, help="the compact file to fine-tune")
    f.add_argument("--output", required=True, help="where the best model (validation top-1) is written, a version-1 compact file")
    add_stage2_flags(f, skip=("checkpoint_dir", "eval_only"))
    # `attribute`: explain's records with class-specific relevance maps (explain(method="attribution")) -- predict's flags, --overlay_dir, --target
    t = sub.add_parser("attribute")
    _add_predict_flags(t)
    t.add_argument("--target", type=_int_in(0, (1 << 20) - 1, "--target"), default=None,
                   help="the class whose evidence is mapped, in [0, num_labels); default: every image's own top-1 label among --num_labels")
    t.add_argument("--overlay_dir", default=None, help="write <index>_<basename>.png per readable image: the model's view with the map in red")
    # classify image files with a compact file; `explain` adds the attention rollout maps to the records
    for name in ("predict", "explain"):
        _add_predict_flags(sub.add_parser(name))
    x = sub.choices["explain"]
    x.add_argument("--method", choices=list(METHODS), default="rollout",
                   help="rollout: the readout tokens' attention rolled back through every block; last: their head-mean attention in the last block")
    x.add_argument("--overlay_dir", default=None, help="write <index>_<basename>.png per readable image: the model's view with the map in red")
    return p


def _add_predict_flags(q):
    """``predict``'s flags; ``explain`` takes the same ones with the same defaults."""
    q.add_argument("--compact", required=True, help="the compact file (a dense checkpoint goes through `export` first)")
    add_image_file_flags(q)
    q.add_argument("--fused_input", type=int, default=FUSED_INPUT_DEFAULT,
                   help="1: the resampler writes the patch rows (uvc_image_prep_patches); 0: images, then uvc_patchify")


def add_image_file_flags(q, *, topk=True, classes=True):
    """--images --output [--topk] --batch_size --num_workers --precision --preset --interpolation --crop_pct [--classes] --num_labels: what
    the commands that read image files share (``predict`` / ``explain`` / ``attribute``, ``compact_pixel``, ``compact_perturb``).  A flag
    of this block is added here and nowhere else."""
    from .data import INTERPOLATIONS
    q.add_argument("--images", nargs="+", required=True, help="image files, or directories walked recursively for image files (sorted)")
    q.add_argument("--output", default=None, help="JSON-lines file; default: stdout")
    if topk:
        q.add_argument("--topk", type=_int_in(1, MAX_TOPK, "--topk"), default=5)
    q.add_argument("--batch_size", type=_int_in(1, 65535, "--batch_size"), default=64)
    q.add_argument("--num_workers", type=int, default=8, help="decode threads (at most 16)")
    q.add_argument("--precision", default="bf16")
    q.add_argument("--preset", choices=list(PRESETS), default="imagenet",
                   help="imagenet: resize, centre crop, ImageNet mean / std; cifar: square resize, mean / std 0.5")
    q.add_argument("--interpolation", choices=list(INTERPOLATIONS), default="bilinear")
    q.add_argument("--crop_pct", type=_crop_pct_arg, default=None,
                   help="imagenet preset: resize the short side to floor(img_size / crop_pct) before the centre crop; default: img_size * 256 // 224")
    if classes:
        q.add_argument("--classes", default=None, help="class names: one per line, or a JSON list")
    q.add_argument("--num_labels", type=_int_in(1, 1 << 20, "--num_labels"), default=None,
                   help="the valid logits (the rest of the head is padding); default: " + ("the length of --classes, else " if classes else "")
                   + "the file's num_classes")


def _dense_model(args, dev):
    """The Stage-2 eval model of post_train.eval_model, with patch-gating mode 1 when asked for."""
    from .checkpoints import load_pretrained
    from .joint_train import register_masks
    from .pos_embed import match_pos_embed
    from .trainer import build_model
    if "t2t" in args.model_type:
        raise NotImplementedError("compact export of T2T-ViT models (their tokens-to-token front end) is not supported")
    if not args.checkpoint_dir and not args.model_path:
        raise SystemExit("need --checkpoint_dir or --model_path")
    model = build_model(args, dev, enable_patch_gating=args.enable_patch_gating, patch_hard=bool(args.patch_hard), gumbel_hard=True)
    register_masks(model)
    if args.checkpoint_dir:
        model.load_state_dict(match_pos_embed(torch.load(args.checkpoint_dir, map_location="cpu"), model))
    else:
        load_pretrained(args.model_path, model, num_classes=args.num_classes, what="model")
    model.apply_masks()
    model.eval()
    return model


def _report(export, B=1):
    cfg = export["cfg"]
    return dict(blocks=[dict(source=b["source"], heads=len(b["heads"]), v_dim=b["v_dim"], hidden=b["hidden"]) for b in export["blocks"]],
                params=sum(int(t.numel()) for k, t in export["state_dict"].items() if k != "patch_gating"),
                macs_full=full_macs(cfg, B), macs_compact=compact_macs(export, B, padded=False), macs_compact_padded=compact_macs(export, B, padded=True))


def finetune(args, dev):
    """``finetune``: Stage 2's epoch loop (post_train.post_training) on a compact file; the model with the best validation top-1 is saved."""
    from .compact_train import CompactTrainer
    from .driver import seeded_mixup, train_loaders
    from .post_train import post_training, train_batches, valid_fn_of
    export = load_compact(args.compact)
    c = export["cfg"]
    args.img_size, args.num_classes, args.enable_deit = c["img_size"], c["num_classes"], c["enable_dist"]
    train_loader, test_loader = train_loaders(args, rank=0, world=1)
    mixup_fn = seeded_mixup(args, real=True) if train_loader is not None else None
    tr = CompactTrainer(args, export, device=dev)
    valid_fn = valid_fn_of(args, dev, test_loader)
    before = valid_fn(tr.model) if valid_fn else None
    save = lambda tr: torch.save(tr.export(), args.output)
    best = post_training(tr, train_batches(args, dev, train_loader, mixup_fn, args.seed), epochs=args.epochs, valid_fn=valid_fn,
                         save_best=save, prefix="[compact finetune]")
    if valid_fn is None:
        save(tr)
    print(json.dumps(dict(output=args.output, top1_before=before, top1_after=best if valid_fn else None, epochs=args.epochs, steps=tr.global_step,
                          **_report(export))))
    return tr


def main(argv=None):
    args = _parser().parse_args(argv)
    dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    if args.cmd == "finetune":
        return finetune(args, dev)
    if args.cmd in ("predict", "explain", "attribute"):
        return predict_command(args, dev)
    if args.cmd == "export" or not args.compact:
        model = _dense_model(args, dev)
        export = export_compact(model, compact_plan(model, args.mlp_multiple))
        del model
    else:
        export = load_compact(args.compact)
    if args.cmd == "export":
        torch.save(export, args.output)
        print(json.dumps(dict(output=args.output, **_report(export))))
        return export
    from .post_train import loader_valid_fn, synthetic_valid_fn
    cm = CompactVisionTransformer(export, precision=args.precision, device=dev)
    args.img_size, args.num_classes = export["cfg"]["img_size"], export["cfg"]["num_classes"]
    if args.synthetic:
        acc = synthetic_valid_fn(args, dev)(cm)
    else:
        from . import data
        _, test_loader = data.build_loaders(args, rank=0, world=1, splits=("test",))
        acc = loader_valid_fn(test_loader)(cm)
    print(json.dumps(dict(top1=acc, **_report(export))))
    return acc


if __name__ == "__main__":
    main()
