"""Pretrained checkpoints into the engine's models (host code, run once per load on the CPU).

``load_pretrained`` reads the layouts the reference's drivers and the public DeiT / T2T-ViT releases use -- ``{"model": sd}``,
``{"state_dict_ema": sd}``, ``{"state_dict": sd}`` or a bare state_dict (this engine's own reference-format checkpoints) -- in the
reference's key order (joint_train.py:152-166, T2TViT/utils.py:50-61), strips a leading ``module.``, resamples ``pos_embed`` to the
model's grid and loads with ``strict=False`` semantics.  Two cases the reference would let through silently raise here: a file in
which no ``blocks.*`` / ``tokens_to_token.*`` weight matches the model (a wrong file or a wrong --model_type would otherwise train
from random weights), and an ``http(s)://`` path (the engine never downloads)."""
from __future__ import annotations

import argparse
from dataclasses import dataclass, field

import torch

from .pos_embed import match_pos_embed

LAYOUT_KEYS = ("model", "state_dict_ema", "state_dict")          # joint_train.py:162-166, then T2TViT/utils.py:53-56
HEAD_PREFIXES = ("head.", "head_dist.")
BODY_PREFIXES = ("blocks.", "tokens_to_token.")


@dataclass
class LoadReport:
    source: str
    layout: str                                 # one of LAYOUT_KEYS, or "bare"
    loaded: list = field(default_factory=list)
    missing: list = field(default_factory=list)       # model keys the file does not set: they keep the model's init
    unexpected: list = field(default_factory=list)    # file keys the model does not have
    dropped: list = field(default_factory=list)       # head keys left out on a class-count mismatch


def read_checkpoint(path):
    """``torch.load`` of a local file on the CPU.  timm's training checkpoints (T2T-ViT's releases) carry their argparse
    Namespace next to the weights, which is the one non-tensor class allowed in."""
    if str(path).startswith(("http://", "https://")):
        raise ValueError(f"{path}: the engine does not download checkpoints; fetch the file and pass its local path")
    with torch.serialization.safe_globals([argparse.Namespace]):
        return torch.load(path, map_location="cpu", weights_only=True)


def unwrap_state_dict(ck):
    """(layout, state_dict) of a loaded checkpoint, with a leading ``module.`` stripped from every key."""
    if not isinstance(ck, dict):
        raise TypeError(f"a checkpoint is a dict, not {type(ck).__name__}")
    layout, sd = "bare", ck
    for k in LAYOUT_KEYS:
        if isinstance(ck.get(k), dict):
            layout, sd = k, ck[k]
            break
    return layout, {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}


def load_pretrained(path_or_dict, model, *, num_classes, what="student", verbose=True) -> LoadReport:
    """Load a pretrained checkpoint (a local path or an already loaded dict) into ``model`` and return what was loaded.

    ``head.*`` / ``head_dist.*`` rows whose class count differs from ``num_classes`` are left out (one line says so) and keep the
    model's seeded init.  Any other shape mismatch raises and names the key; so does a file none of whose ``blocks.*`` /
    ``tokens_to_token.*`` tensors the model has.  Mask buffers, ``gumbel.*``, ``patch_gating`` and ``block_skip_gating`` are not in
    public checkpoints: they keep their init unless the file has them.  ``verbose``: print the report (rank 0)."""
    say = print if verbose else (lambda *_: None)
    source = path_or_dict if isinstance(path_or_dict, str) else "<state dict>"
    ck = read_checkpoint(path_or_dict) if isinstance(path_or_dict, str) else path_or_dict
    layout, sd = unwrap_state_dict(ck)
    table = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    rep = LoadReport(source=source, layout=layout)
    head_n = {tuple(sd[k].shape)[0] for k in sd if k.startswith(HEAD_PREFIXES) and k in table}
    if head_n and head_n != {num_classes}:
        rep.dropped = [k for k in sd if k.startswith(HEAD_PREFIXES)]
        sd = {k: v for k, v in sd.items() if not k.startswith(HEAD_PREFIXES)}
        say(f"{what}: {source} has a {'/'.join(map(str, sorted(head_n)))}-class head, the model {num_classes}: "
            f"{', '.join(rep.dropped)} not loaded (seeded init kept)")
    sd = match_pos_embed(sd, model)
    bad = [f"{k}: file {tuple(v.shape)}, model {table[k]}" for k, v in sd.items() if k in table and tuple(v.shape) != table[k]]
    if bad:
        raise ValueError(f"{what}: {source} does not fit the model: " + "; ".join(bad))
    if not any(k.startswith(BODY_PREFIXES) and k in table for k in sd):
        raise ValueError(f"{what}: no blocks.* / tokens_to_token.* tensor of {source} ({layout} layout, {len(sd)} keys) matches the "
                         f"model: a wrong file, or a wrong --model_type / --teacher-model?")
    res = model.load_state_dict(sd, strict=False)
    rep.loaded = [k for k in sd if k in table]
    rep.missing, rep.unexpected = list(res.missing_keys), list(res.unexpected_keys)
    say(f"{what}: loaded {len(rep.loaded)} tensors from {source} ({layout})")
    if rep.missing:
        say(f"{what}: missing keys (model init kept): {rep.missing}")
    if rep.unexpected:
        say(f"{what}: unexpected keys (ignored): {rep.unexpected}")
    return rep
