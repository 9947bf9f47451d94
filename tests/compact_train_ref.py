"""Test plumbing for compact fine-tuning: the compact exports of the Stage-2 fixture states, float64 autograd through
``compact.reference_logits``, and the CPU restatement of one ``CompactTrainer`` step (oracle pieces only: ``oracle.step``'s loss,
clip and AdamW, ``oracle.stage2``'s decay groups and cosine schedule)."""
from __future__ import annotations

import torch

import scenarios as SC
from helpers import stage2_state
from oracle import stage2 as O2
from oracle import step as OS
from oracle import vit as OV
from uvc_amd import compact as CP

# tensors whose shape a compact export keeps (the reference's golden grad_abs_sum applies to them as it stands)
GLOBAL_KEPT = ("cls_token", "dist_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias", "norm.weight", "norm.bias",
               "head.weight", "head.bias", "head_dist.weight", "head_dist.bias")
BLOCK_KEPT = ("norm1.weight", "norm1.bias", "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.fc2.bias")


def fixture_export(name):
    """(recipe, oracle cfg, compact export, teacher state) of a Stage-2 fixture: its Stage-1 checkpoint exported at its kept widths."""
    r = SC.stage2_recipe(name)
    cfg, params, masks, teacher = stage2_state(r)
    sd = {k: v.clone() for k, v in params.items()}
    for k, v in masks.items():
        sd[k[:-len("weight")] + "mask"] = v.clone()
    return r, cfg, CP.export_compact(sd, CP.compact_plan(sd)), teacher


def teacher_logits(r, cfg, teacher, x):
    if r["distillation_type"] == "none":
        return None
    with torch.no_grad():
        tl, _ = OV.forward({k: v.to(x.dtype) for k, v in teacher.items()}, cfg, OV.GateFlags(training=False), x)
    return tl


def leaves(export, dtype=torch.float64, device="cpu"):
    return {k: v.detach().to(device=device, dtype=dtype).clone().requires_grad_(True) for k, v in export["state_dict"].items()}


def loss_and_grads(export, P, x, y, tl, r):
    """Loss, the two heads' logits and autograd gradients ({name: tensor or None}) of the compact model with leaves ``P``."""
    for p in P.values():
        p.grad = None
    o, od = CP.reference_logits(dict(export, state_dict=P), x)
    loss = OS.distillation_loss(o, od, y, tl, kind=r["distillation_type"], alpha=r["distillation_alpha"], T=r["distillation_tau"])
    loss.backward()
    return loss.detach(), o.detach(), od.detach(), {k: p.grad for k, p in P.items()}


def kept_names(export, P):
    """(compact name, source name) of the tensors that keep their shape and are read by the forward."""
    out = [(n, n) for n in GLOBAL_KEPT if n in P]
    for k, b in enumerate(export["blocks"]):
        for s in BLOCK_KEPT:
            if (s.startswith("norm1") and not b["heads"]) or (s.startswith("norm2") and not b["hidden"]):
                continue
            out.append((f"blocks.{k}.{s}", f"blocks.{b['source']}.{s}"))
    return out


class CpuCompactTrainer:
    """One ``CompactTrainer`` step restated on the CPU: autograd through ``reference_logits``, the oracle's global-norm clip, AdamW with
    timm's decay groups (parameters without a gradient are skipped entirely), the per-epoch cosine schedule on lr * batch / 512."""

    def __init__(self, export, r, cfg, teacher, dtype=torch.float64):
        self.export, self.r, self.cfg, self.teacher, self.dtype = export, r, cfg, teacher, dtype
        self.P = leaves(export, dtype)
        self.lr0 = r["learning_rate"] * r["batch"] / 512.0
        self.opt = OS.AdamWState(lr0=self.lr0, wd=r["weight_decay"], eps=r["opt_eps"])
        self.wd_of = O2.weight_decay_groups(self.P, r["weight_decay"])
        self.cur_lr = self.lr0

    def begin_epoch(self, epoch):
        r = self.r
        self.cur_lr = O2.cosine_epoch_lr(epoch, self.lr0, r["epochs"], r["min_lr"], r["warmup_epochs"], r["warmup_lr"], r["decay_rate"])

    def step(self, x, y):
        x, y = x.to(self.dtype), y.to(self.dtype)
        tl = teacher_logits(self.r, self.cfg, self.teacher, x)
        for p in self.P.values():
            p.requires_grad_(True)
        if "patch_gating" in self.P:
            self.P["patch_gating"].requires_grad_(False)
        loss, o, od, grads = loss_and_grads(self.export, self.P, x, y, tl, self.r)
        with torch.no_grad():
            gnorm = OS.clip_grad_norm([g for g in grads.values() if g is not None], self.r["max_grad_norm"])
            for p in self.P.values():
                p.requires_grad_(False)
            OS.adamw_step(self.opt, self.P, grads, self.cur_lr, wd_of=self.wd_of)
        return dict(loss=float(loss), logits=o, logits_dist=od, gnorm=float(gnorm), grads=grads)
