"""Prune a compact model further on MI355X: Taylor gate scores of its kept heads and MLP units, and the smaller file they imply.

Every other tool measures a compact file or retrains it; this one makes it smaller without going back to the dense checkpoint and
Stage 1.  The first-order Taylor importance of a structure is built on the per-image gradient of the loss with respect to a
multiplicative gate on it, taken at gate = 1:

    taylor   mean_b s[b, g]^2          (Molchanov et al., CVPR 2019)
    abs      mean_b |s[b, g]|          (Michel et al., NeurIPS 2019, "Are Sixteen Heads Really Better than One?")

with ``s[b, head] = <o, dL_b/do>`` over the head's attention output and ``s[b, unit] = <u, dL_b/du>`` over the unit's GELU output.

    python -m uvc_amd.compact_prune score --compact F --dataset cifar10|cifar100|imagenet --data_dir D [--split train] [--max_images 2048]
        [--num_labels N] [--precision bf16|fp32] --output scores.pt
    python -m uvc_amd.compact_prune apply --compact F [--scores scores.pt] (--keep_macs 0.8 | --target_macs M)
        [--criterion taylor|abs|magnitude|random] [--rank raw|per_mac] [--min_heads 1] [--min_units 64] [--seed 0] --output smaller.compact.pt

``CompactGateViT.gate_grads`` goes through ``uvc_vit_compact_gate_grads`` (include/uvc_vit.h): the training forward, every image's own
cross-entropy seed and the dgrad-only backward walk with one ``uvc_gate_dots`` (uvc_amd/csrc/prune.hip) behind each attn.proj dgrad and one
in place of each fc2 dgrad's epilogue; ``importance`` sums the squares and absolute values over a split with ``uvc_gate_accumulate``.
``reference_gate_grads`` is the written spec in plain PyTorch autograd.  ``plan_removal`` turns scores into the heads and units to drop
for a MAC target, ``shrink`` (CPU) re-packs the file without them: an ordinary version-1 compact file, which ``compact finetune`` recovers
and every other tool reads.  The result is what ``export_compact`` gives for the dense model with those structures masked, bit for bit.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import time
from typing import Optional, Sequence

import torch

from . import compact as CP
from . import compact_tools as TL
from .compact_attribution import CompactAttributionViT
from .compact_pixel import check_tokens

SCORES_FORMAT, SCORES_VERSION = "uvc-compact-gates", 1
CRITERIA = ("taylor", "abs", "magnitude", "random")
RANKS = ("raw", "per_mac")
HEAD, UNIT = 0, 1                                   # a candidate's kind


# ---- the candidates -------------------------------------------------------------------------------------------------------------------
def gate_table(export: dict):
    """The real candidates of a compact file in the column order of ``uvc_vit_compact_gate_grads``, as ``(kind, block, position)``: blocks
    ascending, a block's kept heads (kind 0, position < len(heads)) before its kept units (kind 1, position < len(hidden_index)).  The
    padding units of a block are not candidates."""
    out = []
    for k, b in enumerate(CP.check_export(export)["blocks"]):
        out += [(HEAD, k, j) for j in range(len(b["heads"]))]
        out += [(UNIT, k, i) for i in range(len(b["hidden_index"]))]
    return out


def _columns(export):
    """(all columns G, the real candidates' columns, the padding units' columns) of the engine's gate row"""
    real, pad, col = [], [], 0
    for b in export["blocks"]:
        nh, n, F = len(b["heads"]), len(b["hidden_index"]), b["hidden"]
        real += range(col, col + nh + n)
        pad += range(col + nh + n, col + nh + F)
        col += nh + F
    return col, real, pad


def _widths(export):
    return [[len(b["heads"]), int(b["v_dim"]), int(b["hidden"]), len(b["hidden_index"])] for b in export["blocks"]]


def _meta(export, num_labels, precision):
    return dict(blocks=_widths(export), img_size=int(export["cfg"]["img_size"]), num_labels=int(num_labels), precision=precision, loss="ce")


def make_scores(export, sum_sq, sum_abs, images, num_labels, precision):
    """The scores dict ``score`` writes: ``{"format", "version", "table" int32 [G, 3], "sum_sq" float64 [G], "sum_abs" float64 [G], "images",
    "meta"}``; ``meta`` holds the file's per-block widths ``[heads, v_dim, hidden, kept units]``, ``img_size``, ``num_labels``, ``precision``
    and ``loss`` ("ce")."""
    table = torch.tensor(gate_table(export), dtype=torch.int32).reshape(-1, 3)
    sum_sq, sum_abs = (t.detach().to(device="cpu", dtype=torch.float64).contiguous() for t in (sum_sq, sum_abs))
    if sum_sq.shape != (table.shape[0],) or sum_abs.shape != sum_sq.shape:
        raise ValueError(f"sum_sq and sum_abs hold one value per candidate ({table.shape[0]})")
    return dict(format=SCORES_FORMAT, version=SCORES_VERSION, table=table, sum_sq=sum_sq, sum_abs=sum_abs, images=int(images),
                meta=_meta(export, num_labels, precision))


def check_scores(scores: dict, export: Optional[dict] = None) -> dict:
    """A scores dict of this build; with ``export`` also that it was taken on a file of these widths (``meta`` and ``table``)."""
    if not isinstance(scores, dict) or scores.get("format") != SCORES_FORMAT:
        raise ValueError(f"not a {SCORES_FORMAT} file")
    if scores.get("version") != SCORES_VERSION:
        raise ValueError(f"{SCORES_FORMAT} version {scores.get('version')} is not supported (this build reads version {SCORES_VERSION})")
    if export is not None:
        meta = scores["meta"]
        if meta.get("blocks") != _widths(export) or meta.get("img_size") != export["cfg"]["img_size"]:
            raise ValueError("the scores' meta does not match the compact file: they were taken on a file of other widths "
                             f"({meta.get('blocks')} at {meta.get('img_size')} px, the file has {_widths(export)} at {export['cfg']['img_size']} px)")
        if scores["table"].tolist() != [list(t) for t in gate_table(export)]:
            raise ValueError("the scores' table does not match the compact file's candidates")
    if int(scores["images"]) < 1:
        raise ValueError("the scores hold no image")
    return scores


# ---- the written spec -----------------------------------------------------------------------------------------------------------------
def reference_gate_grads(export: dict, x: torch.Tensor, labels, num_labels=None, padded: bool = False):
    """``(eval logits [B, num_classes], loss [B], s [B, G])`` in plain PyTorch autograd, in x's dtype and on x's device.  Per image, gates of
    ones with ``requires_grad`` enter ``compact.reference_logits``' network by scaling the columns of ``attn.proj.weight`` with
    ``gamma_head.repeat_interleave(v_dim)`` and those of ``mlp.fc2.weight`` with ``gamma_unit``; the eval logits are ``(o + od) / 2``,
    ``L = logsumexp(z[:, :num_labels]) - z_y`` and ``s = dL / dgamma``.  Columns as ``gate_table``; ``padded=True`` keeps the padding units'
    columns where the engine has them (they are exact zeros: u = GELU(0) = 0)."""
    cfg = CP.check_export(export)["cfg"]
    nl = CP.num_labels(cfg, num_labels)
    B = x.shape[0]
    y = torch.as_tensor(labels).detach().to(device="cpu", dtype=torch.int64).reshape(-1)
    if y.numel() != B or int(y.min()) < 0 or int(y.max()) >= nl:
        raise ValueError(f"labels must be {B} indices in [0, {nl}) (num_labels), not {y.tolist()}")
    sd = {k: v.to(device=x.device, dtype=x.dtype) for k, v in export["state_dict"].items()}
    G, real, _ = _columns(export)
    logits, losses, rows = [], [], []
    for b in range(B):
        with torch.enable_grad():
            gates, P = [], dict(sd)
            for k, blk in enumerate(export["blocks"]):
                p = f"blocks.{k}."
                gh = torch.ones(len(blk["heads"]), dtype=x.dtype, device=x.device, requires_grad=True)
                gu = torch.ones(blk["hidden"], dtype=x.dtype, device=x.device, requires_grad=True)
                P[p + "attn.proj.weight"] = sd[p + "attn.proj.weight"] * gh.repeat_interleave(blk["v_dim"])[None, :]
                P[p + "mlp.fc2.weight"] = sd[p + "mlp.fc2.weight"] * gu[None, :]
                gates += [gh, gu]
            o, od = CP.reference_logits(dict(export, state_dict=P), x[b:b + 1])
            z = (o + od) / 2
            L = torch.logsumexp(z[:, :nl], dim=1) - z[:, int(y[b])]
            live = [g for g in gates if g.numel()]
            got = dict(zip(map(id, live), torch.autograd.grad(L.sum(), live, allow_unused=True))) if live else {}
            row = [torch.zeros_like(g) if got.get(id(g)) is None else got[id(g)] for g in gates]
        logits.append(z.detach()[0])
        losses.append(L.detach()[0])
        rows.append(torch.cat(row) if row else torch.zeros(0, dtype=x.dtype, device=x.device))
    s = torch.stack(rows).reshape(B, G)
    return torch.stack(logits), torch.stack(losses), s if padded else s[:, real]


def reference_importance(export: dict, batches, num_labels=None, precision="reference"):
    """``importance`` on ``reference_gate_grads``: the scores dict of ``(x, y)`` batches, the sums as float64 chains over the images in order
    of each row rounded to float32 (what the engine hands ``uvc_gate_accumulate``)."""
    G = len(gate_table(export))
    sum_sq, sum_abs, n = torch.zeros(G, dtype=torch.float64), torch.zeros(G, dtype=torch.float64), 0
    nl = CP.num_labels(export["cfg"], num_labels)
    for x, y in batches:
        s = reference_gate_grads(export, x, y, nl)[2].float().double().cpu()
        for b in range(s.shape[0]):
            sum_sq += s[b] * s[b]
            sum_abs += s[b].abs()
        n += int(s.shape[0])
    return make_scores(export, sum_sq, sum_abs, n, nl, precision)


# ---- the module -----------------------------------------------------------------------------------------------------------------------
class CompactGateViT(CompactAttributionViT):
    """``CompactAttributionViT`` (the training layout and shadows, no gradient buffer) plus ``gate_grads``."""

    def __init__(self, export: dict, precision: str = "bf16", device=None):
        check_tokens(export)
        super().__init__(export, precision=precision, device=device)
        G, real, pad = _columns(export)
        dev = self._flat.device
        self._gates = G
        self._real, self._pad = torch.tensor(real, dtype=torch.int64, device=dev), torch.tensor(pad, dtype=torch.int64, device=dev)

    @torch.no_grad()
    def gate_grads(self, x, labels, num_labels=None):
        """``(eval logits, loss, s)``: the logits are ``forward``'s bit for bit; ``loss`` float32 [B] is every image's own cross-entropy over
        the first ``num_labels`` columns and ``s`` float32 [B, G] its gradient with respect to a gate on every candidate of ``gate_table``
        (``reference_gate_grads`` is the spec).  ``labels``: B indices in [0, num_labels), checked on the host.  The padding units'
        columns of the engine's row are asserted to be exact zeros, then dropped."""
        from . import _lib as L
        cfg = self._export["cfg"]
        nl = CP.num_labels(cfg, num_labels)
        x = self._prep(x)
        B, dev = x.shape[0], self._flat.device
        if labels is None:
            raise ValueError("gate_grads needs labels")
        y = self._targets(labels if isinstance(labels, (list, tuple, torch.Tensor)) else [labels], B, nl)
        with torch.cuda.device(dev):
            self._refresh_shadows()
            io, mask = self._io(x, B, "gate_grads")
            logits = torch.empty(B, cfg["num_classes"], device=dev)
            logits_dist = torch.empty(B, cfg["num_classes"], device=dev) if self.num_tokens == 2 else None
            io.logits, io.logits_dist = L.ptr(logits), L.ptr(logits_dist)
            gates = torch.empty(B, max(1, self._gates), dtype=torch.float32, device=dev)
            loss = torch.empty(B, dtype=torch.float32, device=dev)
            L.check(self._lib_call("uvc_vit_compact_gate_grads", C.byref(io), L.ptr(y), nl, L.ptr(gates), L.ptr(loss), L.cur_stream()),
                    "uvc_vit_compact_gate_grads")
            del mask, y                                  # (read by the launches above: alive until they are enqueued)
            gates = gates[:, :self._gates]
            if self._pad.numel() and bool((gates[:, self._pad] != 0).any()):
                raise AssertionError("a padding unit has a non-zero gate gradient: its fc1 row or bias is not zero in this file")
            s = gates[:, self._real].contiguous()
        return (logits if logits_dist is None else (logits + logits_dist) / 2), loss, s


def importance(model: CompactGateViT, batches, num_labels=None) -> dict:
    """The scores dict of ``(x, y)`` batches on a ``CompactGateViT``: one ``gate_grads`` call and one ``uvc_gate_accumulate`` per batch, the
    sums in float64 on the device as one chain per candidate over the images in order -- they do not depend on the batch size."""
    from . import ops
    export, dev = model._export, model._flat.device
    nl = CP.num_labels(export["cfg"], num_labels)
    G = len(gate_table(export))
    sum_sq, sum_abs = torch.zeros(G, dtype=torch.float64, device=dev), torch.zeros(G, dtype=torch.float64, device=dev)
    n = 0
    with torch.cuda.device(dev):
        for x, y in batches:
            s = model.gate_grads(x, y, nl)[2]
            if G:
                ops.gate_accumulate(s, sum_sq, sum_abs)
            n += int(s.shape[0])
    if n == 0:
        raise ValueError("the loader yields no batch of images")
    return make_scores(export, sum_sq, sum_abs, n, nl, model.precision)


# ---- from scores to a smaller file ------------------------------------------------------------------------------------------------------
def _check_removal(export, removal):
    """``{block: (sorted head positions, sorted unit positions)}`` for every block, the removal's entries checked"""
    blocks = export["blocks"]
    removal = {} if removal is None else removal
    out = {}
    for k in removal:
        if not isinstance(k, int) or not 0 <= k < len(blocks):
            raise ValueError(f"removal names block {k!r}: the file has blocks 0..{len(blocks) - 1}")
    for k, b in enumerate(blocks):
        r = removal.get(k, {})
        if set(r) - {"heads", "units"}:
            raise ValueError(f"removal of block {k}: the keys are 'heads' and 'units', not {sorted(r)}")
        hs, us = [int(j) for j in r.get("heads", [])], [int(i) for i in r.get("units", [])]
        for what, got, n in (("head", hs, len(b["heads"])), ("unit", us, len(b["hidden_index"]))):
            if len(set(got)) != len(got) or any(not 0 <= p < n for p in got):
                raise ValueError(f"removal of block {k}: {what} positions must be distinct and lie in [0, {n}), not {got}")
        out[k] = (sorted(hs), sorted(us))
    return out


def _widths_after(b, mlp_multiple, kept_heads, kept_units):
    """(v_dim, hidden) of source block ``b`` with the kept head positions and the kept unit COUNT"""
    v_dim = CP._round_up(max(len(b["v_index"][j]) for j in kept_heads), 16) if kept_heads else 0
    hidden = min(b["hidden"], CP._round_up(kept_units, mlp_multiple)) if kept_units else 0
    return v_dim, hidden


def _mlp_multiple(export):
    return int(export["cfg"].get("mlp_multiple", CP.MLP_MULTIPLE))


def shrink(export: dict, removal: dict) -> dict:
    """The version-1 compact dict of ``export`` without the heads and units of ``removal`` (``{block: {"heads": [positions], "units":
    [positions]}}``, positions into the block's ``heads`` / ``hidden_index``), on the CPU.  Kept heads' q / k / v rows and proj columns are
    re-packed at the new ``v_dim = round_up(max kept dims of the remaining heads, 16)`` (0 with none left), kept units at
    ``min(hidden, round_up(kept, mlp_multiple))``; ``heads``, ``v_index`` and ``hidden_index`` keep their source ids.  A block that loses every
    head keeps ``proj.bias``, one that loses every unit keeps ``fc2.bias``.  What ``export_compact`` gives for the dense model with the same
    structures masked, bit for bit."""
    CP.check_export(export)
    rem = _check_removal(export, removal)
    D, m = export["cfg"]["embed_dim"], _mlp_multiple(export)
    src = export["state_dict"]
    sd = {k: v.detach().clone() for k, v in src.items() if not k.startswith("blocks.")}
    blocks = []
    for k, b in enumerate(export["blocks"]):
        p = f"blocks.{k}."
        for n in ("norm1.weight", "norm1.bias", "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.fc2.bias"):
            sd[p + n] = src[p + n].detach().clone()
        gone_h, gone_u = (set(r) for r in rem[k])
        js = [j for j in range(len(b["heads"])) if j not in gone_h]
        us = [i for i in range(len(b["hidden_index"])) if i not in gone_u]
        dv, Fk = _widths_after(b, m, js, len(us))
        nh0, dv0, nh = len(b["heads"]), b["v_dim"], len(js)
        wq, bq, wp = src[p + "attn.qkv.weight"], src[p + "attn.qkv.bias"], src[p + "attn.proj.weight"]
        qkv_w, qkv_b, proj_w = torch.zeros(nh * (128 + dv), D), torch.zeros(nh * (128 + dv)), torch.zeros(D, nh * dv)
        for jj, j in enumerate(js):
            for s in (0, 1):                                   # q, k: all 64 dims
                qkv_w[s * nh * 64 + jj * 64:s * nh * 64 + (jj + 1) * 64] = wq[s * nh0 * 64 + j * 64:s * nh0 * 64 + (j + 1) * 64]
                qkv_b[s * nh * 64 + jj * 64:s * nh * 64 + (jj + 1) * 64] = bq[s * nh0 * 64 + j * 64:s * nh0 * 64 + (j + 1) * 64]
            nd = len(b["v_index"][j])
            qkv_w[2 * nh * 64 + jj * dv:2 * nh * 64 + jj * dv + nd] = wq[2 * nh0 * 64 + j * dv0:2 * nh0 * 64 + j * dv0 + nd]
            qkv_b[2 * nh * 64 + jj * dv:2 * nh * 64 + jj * dv + nd] = bq[2 * nh0 * 64 + j * dv0:2 * nh0 * 64 + j * dv0 + nd]
            proj_w[:, jj * dv:jj * dv + nd] = wp[:, j * dv0:j * dv0 + nd]
        sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"], sd[p + "attn.proj.weight"] = qkv_w, qkv_b, proj_w
        idx = torch.tensor(us, dtype=torch.long)
        w1, b1, w2 = torch.zeros(Fk, D), torch.zeros(Fk), torch.zeros(D, Fk)
        if len(us):
            w1[:len(us)] = src[p + "mlp.fc1.weight"][idx]
            b1[:len(us)] = src[p + "mlp.fc1.bias"][idx]
            w2[:, :len(us)] = src[p + "mlp.fc2.weight"][:, idx]
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"], sd[p + "mlp.fc2.weight"] = w1, b1, w2
        blocks.append(dict(source=b["source"], heads=[b["heads"][j] for j in js], v_index=[list(b["v_index"][j]) for j in js], v_dim=dv,
                           hidden_index=[b["hidden_index"][i] for i in us], hidden=Fk))
    out = CP.with_state(export, {k: sd[k] for k in src})           # (the source's key order)
    out["blocks"] = blocks
    return CP.check_export(out)


def candidate_cost(export: dict, kind: int, block: int) -> int:
    """The MACs a candidate of ``block`` costs at B = 1 in ``compact._block_macs``' terms: a head ``N D (128 + 2 v_dim) + N N (64 + v_dim)``
    (its q / k / v rows, its scores, its values, its proj columns), a unit ``2 N D``."""
    cfg = export["cfg"]
    N, D, dv = CP._seq(cfg), cfg["embed_dim"], export["blocks"][block]["v_dim"]
    return N * D * (128 + 2 * dv) + N * N * (64 + dv) if kind == HEAD else 2 * N * D


def candidate_keys(export: dict, scores: Optional[dict], criterion: str = "taylor", rank: str = "raw", seed: int = 0):
    """float64 [G]: the key of every candidate of ``gate_table`` -- ``taylor`` ``sum_sq / images``, ``abs`` ``sum_abs / images``,
    ``magnitude`` the sum of squares of its proj columns or of its fc2 column (no scores needed), ``random`` its rank in the permutation
    of ``torch.Generator().manual_seed(seed)``; with ``rank="per_mac"`` divided by ``candidate_cost``.  Low keys go first."""
    if criterion not in CRITERIA:
        raise ValueError(f"criterion must be one of {CRITERIA}, not {criterion!r}")
    if rank not in RANKS:
        raise ValueError(f"rank must be one of {RANKS}, not {rank!r}")
    table = gate_table(export)
    if scores is not None:
        check_scores(scores, export)
    if criterion in ("taylor", "abs"):
        if scores is None:
            raise ValueError(f"criterion {criterion!r} needs scores (python -m uvc_amd.compact_prune score)")
        key = scores["sum_sq" if criterion == "taylor" else "sum_abs"].double() / int(scores["images"])
    elif criterion == "magnitude":
        sd = export["state_dict"]
        vals = []
        for kind, k, pos in table:
            dv = export["blocks"][k]["v_dim"]
            w = sd[f"blocks.{k}.attn.proj.weight"][:, pos * dv:(pos + 1) * dv] if kind == HEAD else sd[f"blocks.{k}.mlp.fc2.weight"][:, pos]
            vals.append(float(w.double().pow(2).sum()))
        key = torch.tensor(vals, dtype=torch.float64)
    else:
        perm = torch.randperm(len(table), generator=torch.Generator().manual_seed(int(seed)))
        key = torch.empty(len(table), dtype=torch.float64)
        key[perm] = torch.arange(len(table), dtype=torch.float64)
    if rank == "per_mac" and len(table):
        key = key / torch.tensor([candidate_cost(export, kind, k) for kind, k, _ in table], dtype=torch.float64)
    return key


def _plan(export, scores, keep_macs, target_macs, criterion, rank, min_heads, min_units, seed):
    CP.check_export(export)
    if (keep_macs is None) == (target_macs is None):
        raise ValueError("give one of keep_macs (a fraction of the file's padded MACs) / target_macs")
    if int(min_heads) < 0 or int(min_units) < 0:
        raise ValueError(f"min_heads {min_heads} and min_units {min_units} must be non-negative")
    cfg, blocks, m = export["cfg"], export["blocks"], _mlp_multiple(export)
    source_macs = CP.compact_macs(export, padded=True)
    if keep_macs is not None:
        if not 0.0 < float(keep_macs) <= 1.0:
            raise ValueError(f"keep_macs {keep_macs} must lie in (0, 1]")
        target = float(keep_macs) * source_macs
    else:
        target = float(target_macs)
    key = candidate_keys(export, scores, criterion, rank, seed).tolist()
    table = gate_table(export)
    order = sorted(range(len(table)), key=lambda c: (key[c], table[c][1], table[c][0], table[c][2]))
    heads = [list(range(len(b["heads"]))) for b in blocks]                  # the kept head positions
    units = [len(b["hidden_index"]) for b in blocks]                         # the kept unit counts
    gone = [([], []) for _ in blocks]

    def block_macs(k):
        dv, F = _widths_after(blocks[k], m, heads[k], units[k])
        return sum(CP._block_macs(cfg, 1, len(heads[k]), len(heads[k]) * dv, F))

    per_block = [block_macs(k) for k in range(len(blocks))]
    if sum(per_block) + CP.embed_macs(cfg) != source_macs:
        raise ValueError("the file's padded widths are not what its kept heads and units imply (v_dim / hidden were not made by export_compact)")
    macs = source_macs
    for c in order:
        if macs <= target:
            break
        kind, k, pos = table[c]
        if kind == HEAD:
            if len(heads[k]) - 1 < int(min_heads):
                continue
            heads[k].remove(pos)
        else:
            if units[k] - 1 < int(min_units):
                continue
            units[k] -= 1
        gone[k][kind].append(c)
        now = block_macs(k)
        macs += now - per_block[k]
        per_block[k] = now
    if macs > target:
        raise ValueError(f"target_macs {target:.0f} cannot be reached with min_heads {min_heads} and min_units {min_units}: "
                         f"the lowest reachable value is {macs} padded MACs")
    # the fill: padding slots are free, so a block's best removed units come back while the kept count is below the padded width
    filled = 0
    for k, b in enumerate(blocks):
        width = _widths_after(b, m, heads[k], units[k])[1]
        back = sorted(gone[k][UNIT], key=lambda c: (-key[c], table[c][2]))
        while units[k] < width and back:
            gone[k][UNIT].remove(back.pop(0))
            units[k] += 1
            filled += 1
    removal = {k: dict(heads=sorted(table[c][2] for c in gone[k][HEAD]), units=sorted(table[c][2] for c in gone[k][UNIT])) for k in range(len(blocks))}
    return removal, dict(filled=filled, target_macs=target, macs_padded=macs, source_macs_padded=source_macs)


def plan_removal(export: dict, scores: Optional[dict] = None, *, keep_macs=None, target_macs=None, criterion="taylor", rank="raw", min_heads=1,
                 min_units=64, seed=0) -> dict:
    """``{block: {"heads": [positions], "units": [positions]}}`` (every block, positions ascending): what to drop of ``export`` to bring
    ``compact_macs(result, padded=True)`` to ``target_macs``, or to ``keep_macs`` times the file's own padded MACs.

    Greedy pass: the candidates in ascending ``candidate_keys``, ties by (block, heads before units, position); one that would take its block
    below ``min_heads`` heads / ``min_units`` units is skipped (0 lets a branch become its bias); after each removal the padded MACs of the
    result are recomputed and the pass stops at the first value <= the target.  A target that cannot be reached is refused, naming the lowest
    value reachable.  Fill pass: per block the removed units come back in descending key (ties: ascending position) while the kept count is
    below the padded width of the result -- padding slots are free, so the padded MACs do not change.  Deterministic.  ``scores`` (needed by
    ``taylor`` and ``abs``) are refused when their ``meta`` does not match the file."""
    return _plan(export, scores, keep_macs, target_macs, criterion, rank, min_heads, min_units, seed)[0]


# ---- the commands -------------------------------------------------------------------------------------------------------------------
def score_command(args, dev=None):
    """``score``: the scores dict of up to --max_images images of --split under the eval transform, written to --output; the record
    ``{"output", "images", "gates", "img_per_s"}``."""
    export = CP.as_export(args.compact)
    check_tokens(export)
    dev = TL.device(dev)
    model = CompactGateViT(export, precision=args.precision, device=dev)
    loader, classes = TL.eval_loader(export, args, args.split)
    nl = CP.num_labels(export["cfg"], classes if args.num_labels is None else args.num_labels)

    def batches():
        n = 0
        for x, y in loader:
            if args.max_images is not None and n + x.shape[0] > args.max_images:
                x, y = x[:args.max_images - n].contiguous(), y[:args.max_images - n]
            yield x, y
            n += int(x.shape[0])
            if args.max_images is not None and n >= args.max_images:
                return

    with torch.cuda.device(dev):
        t0 = time.perf_counter()
        scores = importance(model, batches(), nl)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    scores["meta"].update(dataset=args.dataset, split=args.split)
    torch.save(scores, args.output)
    return scores, dict(output=args.output, images=scores["images"], gates=int(scores["table"].shape[0]), img_per_s=scores["images"] / dt if dt > 0 else 0.0)


def apply_command(args):
    """``apply`` (no device): plan, shrink, write --output; the record ``{"output", "criterion", "rank", "target_macs", "source", "result",
    "removed", "macs_padded_before", "macs_padded_after", "macs_before", "macs_after", "filled"}`` with ``compact._report`` of both files."""
    export = CP.load_compact(args.compact)
    scores = check_scores(torch.load(args.scores, map_location="cpu"), export) if args.scores else None
    removal, info = _plan(export, scores, args.keep_macs, args.target_macs, args.criterion, args.rank, args.min_heads, args.min_units, args.seed)
    out = shrink(export, removal)
    torch.save(out, args.output)
    src_r, out_r = CP._report(export), CP._report(out)
    return out, dict(output=args.output, criterion=args.criterion, rank=args.rank, target_macs=info["target_macs"], source=src_r, result=out_r,
                     removed=[dict(block=k, heads=len(r["heads"]), units=len(r["units"])) for k, r in sorted(removal.items())],
                     macs_padded_before=src_r["macs_compact_padded"], macs_padded_after=out_r["macs_compact_padded"],
                     macs_before=src_r["macs_compact"], macs_after=out_r["macs_compact"], filled=info["filled"])


def _fraction(v):
    f = float(v)
    if not 0.0 < f <= 1.0:
        raise argparse.ArgumentTypeError(f"--keep_macs must lie in (0, 1], not {v}")
    return f


def build_parser():
    p = argparse.ArgumentParser(prog="python -m uvc_amd.compact_prune", description="Taylor gate scores of a compact model, and the smaller file they imply")
    sub = p.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("score", help="score every kept head and MLP unit on one split")
    s.add_argument("--compact", required=True, help="the compact file")
    TL.add_dataset_flags(s, eval_batch_size=64, split_default="train")
    s.add_argument("--max_images", type=CP._int_in(1, 1 << 30, "--max_images"), default=2048, help="stop after this many images")
    s.add_argument("--num_labels", type=CP._int_in(1, 1 << 20, "--num_labels"), default=None, help="the valid logits; default: the dataset's classes")
    s.add_argument("--output", required=True, help="the scores file")
    a = sub.add_parser("apply", help="drop the lowest-scored heads and units down to a MAC target (no device needed)")
    a.add_argument("--compact", required=True, help="the compact file")
    a.add_argument("--scores", default=None, help="the scores file of `score` (criteria taylor and abs)")
    t = a.add_mutually_exclusive_group(required=True)
    t.add_argument("--keep_macs", type=_fraction, default=None, help="the target as a fraction of the file's own padded MACs")
    t.add_argument("--target_macs", type=CP._int_in(1, 1 << 62, "--target_macs"), default=None, help="the target in padded MACs at batch 1")
    a.add_argument("--criterion", choices=list(CRITERIA), default="taylor")
    a.add_argument("--rank", choices=list(RANKS), default="raw", help="per_mac: keys divided by the candidate's own MACs")
    a.add_argument("--min_heads", type=CP._int_in(0, 1 << 20, "--min_heads"), default=1, help="heads a block keeps at least (0: the branch may become its bias)")
    a.add_argument("--min_units", type=CP._int_in(0, 1 << 20, "--min_units"), default=64, help="MLP units a block keeps at least")
    a.add_argument("--seed", type=int, default=0, help="criterion random: the permutation's seed")
    a.add_argument("--output", required=True, help="the smaller compact file")
    return p


def main(argv: Optional[Sequence[str]] = None):
    """One JSON line (the command's record), which is returned.  The argument refusals come before any file or image is read."""
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.cmd == "apply":
        if args.criterion in ("taylor", "abs") and not args.scores:
            parser.error(f"--criterion {args.criterion} needs --scores (criteria magnitude and random do not)")
        summary = apply_command(args)[1]
    else:
        TL.need_data(args)
        summary = score_command(args)[1]
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
