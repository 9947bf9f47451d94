"""Fine-tuning a compact model at its kept widths on MI355X.

``CompactTrainableViT`` is the trainable twin of ``compact.CompactVisionTransformer``: the same flat float32 parameter buffer
(uvc_vit_compact_layout), parameters exposed under the compact state_dict names as views into it, a training forward and backward
through ``uvc_vit_compact_train_forward`` / ``uvc_vit_compact_backward`` (include/uvc_vit.h) and, in eval mode, the kernels and the
bits of ``CompactVisionTransformer``.  The function being trained is ``compact.reference_logits``.

``CompactTrainer`` is ``post_train.Stage2Trainer``'s step on that module: DistillationLoss against any dense teacher, global-norm
clip, AdamW with timm's decay groups, ``lr = learning_rate * batch / 512``, the per-epoch cosine schedule.  What differs from the
masked dense Stage 2 on purpose: the clip norm is the norm of the compact gradients.

Padding entries (zero v-rows / proj columns, zero fc1 rows, b1 entries and fc2 columns) receive exactly zero gradients, so AdamW
leaves them exactly zero; parameters no forward reads (norm1 of a block without heads, norm2 of one without units) are frozen, as
torch leaves a parameter whose ``.grad`` is None.  ``patch_gating``, when the file has it, is used and frozen.
"""
from __future__ import annotations

import copy
import ctypes as C
from argparse import Namespace

import torch
import torch.nn as nn

from . import _lib as L
from . import compact as CP
from .trainer import _Trainer

MAX_TOKENS = 256
_bind = CP._bind


def unread_parameters(export: dict):
    """Names of the state_dict tensors no forward reads: autograd through ``compact.reference_logits`` leaves their ``.grad`` None."""
    out = []
    for k, b in enumerate(export["blocks"]):
        if not b["heads"]:
            out += [f"blocks.{k}.{n}" for n in ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight")]
        if not b["hidden"]:
            out += [f"blocks.{k}.{n}" for n in ("norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight")]
    if "patch_gating" in export["state_dict"]:
        out.append("patch_gating")
    return out


def padding_masks(export: dict):
    """{name: bool tensor} marking the padding entries of the restructured tensors (True = padding, exactly zero in a compact file)."""
    out = {}
    D = export["cfg"]["embed_dim"]
    for k, b in enumerate(export["blocks"]):
        p = f"blocks.{k}."
        nh, dv, Fk = len(b["heads"]), b["v_dim"], b["hidden"]
        rows = torch.zeros(nh * (128 + dv), dtype=torch.bool)
        cols = torch.zeros(nh * dv, dtype=torch.bool)
        for j, dims in enumerate(b["v_index"]):
            rows[2 * nh * 64 + j * dv + len(dims):2 * nh * 64 + (j + 1) * dv] = True
            cols[j * dv + len(dims):(j + 1) * dv] = True
        out[p + "attn.qkv.weight"] = rows[:, None].expand(-1, D).clone()
        out[p + "attn.qkv.bias"] = rows
        out[p + "attn.proj.weight"] = cols[None, :].expand(D, -1).clone()
        units = torch.zeros(Fk, dtype=torch.bool)
        units[len(b["hidden_index"]):] = True
        out[p + "mlp.fc1.weight"] = units[:, None].expand(-1, D).clone()
        out[p + "mlp.fc1.bias"] = units
        out[p + "mlp.fc2.weight"] = units[None, :].expand(D, -1).clone()
    return out


def with_state(export: dict, state_dict) -> dict:
    """``compact.with_state`` with the given weights taken to float32 on the CPU, in the source file's shapes."""
    CP.check_export(export)
    return CP.with_state(export, {k: state_dict[k].detach().to(device="cpu", dtype=torch.float32).reshape(v.shape).clone()
                                  for k, v in export["state_dict"].items()})


class _CompactFunction(torch.autograd.Function):
    """One autograd node for the whole model, as model_distilled._VitFunction: the HIP backward writes every gradient into the flat
    gradient buffer (the ``.grad`` views); nothing flows back through autograd."""

    @staticmethod
    def forward(ctx, model, x, anchor):
        logits, logits_dist = model._train_forward(x)
        ctx.model = model
        ctx.two = logits_dist is not None
        return (logits, logits_dist) if ctx.two else logits

    @staticmethod
    def backward(ctx, *grads):
        ctx.model._train_backward(grads[0], grads[1] if ctx.two else None)
        return None, None, None


class CompactTrainableViT(CP._CompactModule):
    """``model(x)`` in train mode returns ``((logits, logits_dist), macs)`` (``logits_dist is logits`` without the distillation
    token), in eval mode what ``CompactVisionTransformer`` returns -- same kernels, same bits."""

    def __init__(self, export: dict, precision: str = "bf16", device=None):
        super().__init__(export, precision, device, "uvc_vit_compact_train_layout", max_tokens=MAX_TOKENS)
        dev, nb = self._flat.device, self._nb
        self._flat_grad = torch.zeros(self._off.n_total, dtype=torch.float32, device=dev)
        tsz = 4 if precision == "fp32" else 2
        self._shadow = torch.zeros(max(1, self._soff.n_total) * tsz, dtype=torch.uint8, device=dev)
        self._shadow_fresh = False
        self._names = []
        self._by_name = {}
        for name, t in export["state_dict"].items():
            o = self._offset(name)
            p = nn.Parameter(self._flat[o:o + t.numel()].view(t.shape), requires_grad=name != "patch_gating")
            self._by_name[name] = p
            self._names.append(name)
            self.register_parameter(name.replace(".", "__"), p)
        cnt = C.c_int32()
        ranges = (C.c_int64 * (4 * max(1, nb)))()
        L.check(self._lib_call("uvc_vit_compact_frozen_ranges", ranges, 2 * max(1, nb), C.byref(cnt)), "uvc_vit_compact_frozen_ranges")
        self._frozen = [(int(ranges[2 * i]), int(ranges[2 * i + 1])) for i in range(cnt.value)]
        self._unread = set(unread_parameters(export))
        self._last = None
        self.grad_accumulate = False
        self.train()

    # -- what FusedAdamW / clip_grad_norm_ read of a model -----------------------------------------------------------------------
    @property
    def n_flat(self):
        return self._off.n_total

    def _check_flat(self):
        pass

    def _extra_live_segments(self):
        return []

    def skipped_block_ranges(self):
        return []

    def _frozen_ranges(self):
        """Parameters no forward reads (uvc_vit_compact_frozen_ranges); patch_gating lies behind n_main, where no optimiser step reaches."""
        return list(self._frozen)

    def _optim_small_tensors(self):
        return []

    def _slots(self):
        return [(self._by_name[n], self._offset(n)) for n in self._names]

    def named_parameters(self, *a, **k):
        for n in self._names:
            yield n, self._by_name[n]

    def parameters(self, recurse=True):
        for n in self._names:
            yield self._by_name[n]

    def no_weight_decay(self):
        return {"pos_embed", "cls_token", "dist_token"}

    def mark_weights_changed(self):
        self._shadow_fresh = False

    def state_dict(self, *a, **k):
        return {n: self._by_name[n].detach().clone() for n in self._names}

    def load_state_dict(self, sd, strict=True):
        missing = [n for n in self._names if n not in sd]
        extra = [n for n in sd if n not in self._by_name]
        if strict and (missing or extra):
            raise RuntimeError(f"compact state_dict mismatch: missing {missing}, unexpected {extra}")
        with torch.no_grad():
            for n in self._names:
                if n in sd:
                    self._by_name[n].copy_(sd[n].to(self._flat.device).reshape(self._by_name[n].shape))
        self.mark_weights_changed()

    def grad_views(self):
        """Point ``.grad`` of every parameter a forward reads at its slice of the flat gradient buffer; the others keep None."""
        base = self._flat_grad.data_ptr()
        for n in self._names:
            p = self._by_name[n]
            if n in self._unread:
                p.grad = None
                continue
            off = self._offset(n)
            if p.grad is None or p.grad.data_ptr() != base + 4 * off:
                p.grad = self._flat_grad[off:off + p.numel()].view(p.shape)

    # -- reference-style API ---------------------------------------------------------------------------------------------------------
    def export(self) -> dict:
        """A version-1 compact dict with the current weights and the source file's ``cfg`` / ``blocks``."""
        return with_state(self._export, self.state_dict())

    def _refresh_shadows(self):
        if not self._shadow_fresh:
            L.check(self._lib_call("uvc_vit_compact_train_update_shadows", L.ptr(self._flat), L.ptr(self._shadow), L.cur_stream()),
                    "uvc_vit_compact_train_update_shadows")
            self._shadow_fresh = True

    def _io(self, x, B, training):
        io, mask = super()._io(x, B, training)
        io.grads = L.ptr(self._flat_grad)
        return io, mask

    def _train_forward(self, x):
        logits, logits_dist, self._last = self._forward(x, True)
        return logits, logits_dist

    def _train_backward(self, d_logits, d_logits_dist):
        st = self._last
        if st is None:
            raise RuntimeError("backward without a training forward")
        self.grad_views()
        io, _ = self._io(st["x"], st["B"], True)
        io.patch_mask = L.ptr(st["mask"])
        d_logits = d_logits.contiguous()
        io.d_logits = L.ptr(d_logits)
        if self.num_tokens == 2:
            d_logits_dist = d_logits_dist.contiguous()
            io.d_logits_dist = L.ptr(d_logits_dist)
        L.check(self._lib_call("uvc_vit_compact_backward", C.byref(io), L.cur_stream()), "uvc_vit_compact_backward")

    def forward(self, x):
        macs = self.macs(x.shape[0])
        if self.training and torch.is_grad_enabled():
            out = _CompactFunction.apply(self, x, self._by_name["cls_token"])
            return (out if self.num_tokens == 2 else (out, out)), macs
        if not self.training:
            return self._eval_logits(x), macs
        with torch.no_grad():
            o, od, _ = self._forward(x)
        return (o, o if od is None else od), macs


def _refuse(args, precision):
    if int(getattr(args, "gradient_accumulation_steps", 1)) > 1:
        raise NotImplementedError("compact fine-tuning runs one micro-batch per step (gradient_accumulation_steps > 1 is not supported)")
    if int(getattr(args, "local_rank", -1)) != -1:
        raise NotImplementedError("compact fine-tuning is single-GPU (data-parallel runs, --local_rank, are not supported)")
    if precision == "bf16_f32resid":
        raise NotImplementedError("compact models train in 'bf16' or 'fp32' (the float32 residual rows of 'bf16_f32resid' are a dense-model mode)")


class CompactTrainer(_Trainer):
    """``Stage2Trainer``'s surface on a compact model: ``begin_epoch``, ``step(x, y, next_x=None)`` -> loss, outputs, gnorm;
    ``state_dict`` / ``load_state_dict`` resume bit for bit."""
    STATE_FORMAT, NOT_A_STATE = "uvc_amd.compact_train.v1", "not a uvc_amd compact training state"

    def __init__(self, args: Namespace, export: dict, device="cuda", teacher_state=None):
        from .losses import DistillationLoss, SoftTargetCrossEntropy
        from .optim import create_optimizer
        from .scheduler import create_scheduler
        from .stage1 import build_teacher
        CP.check_export(export)
        _refuse(args, args.precision)
        self.args = args
        c = export["cfg"]
        self.model = CompactTrainableViT(export, precision=args.precision, device=device)
        teacher, self.teacher_source = None, None
        if args.distillation_type != "none":
            # the teacher is a dense model: by default the architecture the compact file was pruned from, at the file's image size and classes
            ta = copy.copy(args)
            ta.model_type, ta.img_size, ta.num_classes, ta.enable_deit = "custom", c["img_size"], c["num_classes"], c["enable_dist"]
            ta.model_cfg = dict(patch_size=c["patch_size"], embed_dim=c["embed_dim"], depth=c["depth"], num_heads=c["num_heads"],
                                mlp_ratio=c["hidden"] / c["embed_dim"])
            teacher, self.teacher_source = build_teacher(ta, device, teacher_state, verbose=True)
        self.teacher = teacher
        self.criterion = DistillationLoss(SoftTargetCrossEntropy(), teacher, args.distillation_type, args.distillation_alpha, args.distillation_tau)
        args.lr = args.learning_rate * args.train_batch_size / 512.0
        self.optimizer = create_optimizer(args, self.model)
        self.scheduler, self.num_epochs = create_scheduler(args, self.optimizer)
        self.model.train()
        self._start()

    def begin_epoch(self, epoch: int):
        self.epoch = epoch
        self.model.train()
        self.scheduler.step(epoch)

    def export(self) -> dict:
        return self.model.export()
