"""What the three trainers share (``stage1.Stage1Trainer``, ``post_train.Stage2Trainer``, ``compact_train.CompactTrainer``): the model
builder, the training step with its three hooks, the one-batch look-ahead and the AdamW part of a training state.
"""
from __future__ import annotations

import json

from .losses import unit_gradient
from .model_distilled import DistilledVisionTransformer
from .optim import clip_grad_norm_

# models/configs.py:112-165 -- dims of the DeiT family the reference instantiates
CONFIGS = {
    "deit_tiny_patch16_224": dict(patch_size=16, embed_dim=192, depth=12, num_heads=3),
    "deit_small_patch16_224": dict(patch_size=16, embed_dim=384, depth=12, num_heads=6),
    "deit_base_patch16_224": dict(patch_size=16, embed_dim=768, depth=12, num_heads=12),
}


# T2TViT/models/t2t_vit.py:244-249 (models/configs.py:159-165); BASELINE config 5
T2T_CONFIGS = {"t2t_vit_14": dict(embed_dim=384, depth=14, num_heads=6, mlp_ratio=3.0)}


def model_config(name, custom_cfg=None):
    """(is_t2t, dims) of a --model_type / --teacher-model: its CONFIGS / T2T_CONFIGS entry, else ``custom_cfg`` (custom, custom_t2t:
    a dict or its JSON)."""
    t2t = "t2t" in name
    table = T2T_CONFIGS if t2t else CONFIGS
    if name in table:
        return t2t, dict(table[name])
    if not custom_cfg:
        raise ValueError(f"model type {name!r} is not in this engine's configs; custom / custom_t2t take their dims as JSON")
    return t2t, dict(json.loads(custom_cfg) if isinstance(custom_cfg, str) else custom_cfg)


def model_kwargs(t2t, cfg, args, device):
    """Constructor keywords of DistilledVisionTransformer / T2T_ViT for the dims ``cfg`` at the run's img_size, classes and precision."""
    if t2t:
        return dict(embed_dim=cfg["embed_dim"], depth=cfg["depth"], num_heads=cfg["num_heads"], mlp_ratio=cfg.get("mlp_ratio", 3.0),
                    img_size=args.img_size, num_classes=args.num_classes, precision=args.precision, device=device)
    return dict(patch_size=cfg["patch_size"], embed_dim=cfg["embed_dim"], depth=cfg["depth"], num_heads=cfg["num_heads"],
                mlp_ratio=cfg.get("mlp_ratio", 4), qkv_bias=True, drop_rate=0, img_size=args.img_size,
                num_classes=args.num_classes, precision=args.precision, device=device)


def build_model(args, device, *, name=None, cfg=None, **model_flags):
    """The DistilledVisionTransformer or T2T_ViT of ``name`` (default: --model_type) with the dims of ``model_config(name, cfg)`` (``cfg``
    default: args.model_cfg) at the run's img_size, classes and precision; ``model_flags`` (gumbel_hard, enable_patch_gating, patch_hard)
    go to the constructor as they are.  A DeiT carries the distillation token when args.enable_deit says so; T2T-ViT has none, and its
    callers refuse what it cannot do in their own words.  Draws the initial weights from torch's global generator."""
    t2t, dims = model_config(name or args.model_type, cfg if cfg is not None else getattr(args, "model_cfg", None))
    kw = model_kwargs(t2t, dims, args, device)
    if t2t:
        from .t2t_vit import T2T_ViT
        return T2T_ViT(**model_flags, **kw)
    return DistilledVisionTransformer(enable_dist=args.enable_deit, **model_flags, **kw)


def adamw_state(opt):
    """The ``adamw`` entry of a training state: both moments, the step counts and the learning rate of a FusedAdamW."""
    return dict(exp_avg=opt.exp_avg.clone(), exp_avg_sq=opt.exp_avg_sq.clone(), steps=dict(opt.steps), lr=opt.param_groups[0]["lr"])


def load_adamw_state(opt, sd):
    opt.exp_avg.copy_(sd["exp_avg"]); opt.exp_avg_sq.copy_(sd["exp_avg_sq"]); opt.steps = dict(sd["steps"])
    opt.param_groups[0]["lr"] = sd["lr"]


class _Trainer:
    """A subclass's ``__init__`` builds ``args``, ``model``, ``teacher``, ``criterion`` and ``optimizer`` in its own order (model
    construction draws from torch's global generator) and ends with ``_start``.  ``step`` is the same for all three; they differ in the
    three hooks below it.  ``STATE_FORMAT`` / ``NOT_A_STATE`` name the training state that ``state_dict`` writes."""
    STATE_FORMAT = NOT_A_STATE = None

    def _start(self, accum=1):
        self.accum = accum                  # optimiser step every ``accum`` calls of step(); the backwards in between ADD into the flat gradient buffer
        self.model.grad_accumulate = accum > 1
        self._micro = 0
        self.global_step = 0
        self.epoch = 0

    # -- the three hooks
    def _before_forward(self):
        """Runs first in every call of ``step``."""

    def _forward(self, x, tau):
        return self.model(x)

    def _after_optimizer_step(self):
        """Runs between ``optimizer.step()`` (``global_step`` already counted) and ``zero_grad``; returns further keys of the result."""
        return {}

    def step(self, x, y, *, tau=None, zero_grad=True, next_x=None):
        """One loader iteration on the batch (x, y), x / y already mixed: forward, loss, backward, and on every ``accum``-th call clip,
        AdamW and the subclass's tail; the other calls return after the backward with ``stepped=False``.  ``tau`` goes to the forward hook
        (Stage 1's patch-gating temperature).  ``next_x`` (optional): the NEXT step's input batch, if the caller already holds it (a
        prefetching loader does; ``lookahead`` below wraps one): the frozen teacher's forward for it is started on the side stream as soon
        as this step's backward is enqueued, so it runs under the optimizer / UVC tail of small launches, where the chip is otherwise
        nearly idle, instead of in front of the next step's student forward (the two forwards are whole-chip kernels that alternate,
        DESIGN 5.5).  Results do not depend on it: the next step picks the forward up only for that very tensor."""
        a = self.args
        self._before_forward()
        overlap = bool(getattr(a, "overlap_teacher", 1))
        if overlap and not self.criterion.has_prefetch(x):
            self.criterion.prefetch(x)              # teacher forward on a side stream, under the student forward
        outputs, _ = self._forward(x, tau)
        loss = self.criterion(x, outputs, y)
        if self.accum > 1:
            loss = loss / self.accum                                            # joint_train.py:413-414, post_train.py:365-366
        loss.backward(unit_gradient(loss.device))       # d(loss) = 1 without a ones_like fill or a multiply by it (losses.unit_gradient)
        if overlap and next_x is not None:
            # (enqueued behind the LOSS instead, the teacher's whole-chip kernels alternate with the backward's: 11.28 against 11.14 ms, profiles/r5zz_ab_next_teacher_at.txt)
            self.criterion.prefetch(next_x)
        self._micro += 1
        if self._micro % self.accum != 0:                                       # joint_train.py:417, post_train.py:372
            return dict(loss=loss.detach() * self.accum, outputs=outputs, stepped=False)
        gnorm = clip_grad_norm_(self.model, a.max_grad_norm)
        self.optimizer.step()
        self.global_step += 1
        more = self._after_optimizer_step()
        if zero_grad:
            self.optimizer.zero_grad()
        return dict(loss=loss.detach() * self.accum if self.accum > 1 else loss.detach(), outputs=outputs, gnorm=gnorm, **more, stepped=True)

    @staticmethod
    def lookahead(batches):
        """(x, y) batches -> ((x, y), next_x or None): what ``step(..., next_x=)`` wants, one batch read ahead."""
        it = iter(batches)
        try:
            cur = next(it)
        except StopIteration:
            return
        for nxt in it:
            yield cur, nxt[0]
            cur = nxt
        yield cur, None

    # -- resumable state of Stage 2 and of compact fine-tuning (Stage 1 has more to keep and writes its own)
    def state_dict(self):
        return dict(format=self.STATE_FORMAT, model=self.model.state_dict(), adamw=adamw_state(self.optimizer),
                    progress=dict(global_step=self.global_step, epoch=self.epoch))

    def load_state_dict(self, sd):
        if sd.get("format") != self.STATE_FORMAT:
            raise ValueError(self.NOT_A_STATE)
        self.model.load_state_dict(sd["model"])
        load_adamw_state(self.optimizer, sd["adamw"])
        self.global_step, self.epoch = int(sd["progress"]["global_step"]), int(sd["progress"]["epoch"])
