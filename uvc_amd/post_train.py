"""Stage-2 masked fine-tune on the MI355X engine (mirror of ``UVC/post_train.py``: ``setup`` :135-186, the
checkpoint hand-over :676-683 and the loop body of ``post_training`` :270-403).

Stage-2 consumes the Stage-1 checkpoint (bare state_dict with ``mask`` buffers and the learned
``block_skip_gating`` logits) and fine-tunes the pruned network: every step starts with
``weight *= mask`` for every module that carries a mask, the forward hard-skips the blocks whose gate
logits say so (model_distilled.py:496-500, in training mode too), the gate logits are frozen, and the
optimiser / schedule come from timm's factories (AdamW with no decay on 1-D tensors, biases and the
tokens; cosine schedule stepped once per epoch on a learning rate scaled by batch * world / 512).

``Stage2Trainer`` is what the CLI (``python -m uvc_amd.post_train``), ``bench.py --stage 2`` and the
parity tests drive.  No CPU fallback: everything numeric is a kernel of libuvc_hip.so.
"""
from __future__ import annotations

import argparse
import json
import time
from argparse import Namespace

import torch

from .checkpoints import load_pretrained
from .ddp import DistributedDataParallel
from .driver import add_data_flags, add_mixup_flags, add_teacher_flags, init_distributed, seeded_mixup, top1_valid_fn, train_loaders
from .joint_train import count_mask, register_masks, save_model
from .losses import DistillationLoss, SoftTargetCrossEntropy
from .optim import create_optimizer
from .pos_embed import match_pos_embed
from .scheduler import create_scheduler
from .stage1 import build_teacher
from .trainer import _Trainer, build_model, model_config, model_kwargs


def default_args(**over) -> Namespace:
    """argparse defaults of post_train.py:412-600 overlaid with run_post_train.sh; keyword arguments override."""
    a = dict(model_type="deit_tiny_patch16_224", img_size=224, num_classes=1000, train_batch_size=128, learning_rate=1e-4,
             weight_decay=0.05, epochs=120, max_grad_norm=1.0, gradient_accumulation_steps=1, seed=42,
             opt="adamw", opt_eps=1e-8, opt_betas=None, momentum=0.9, sched="cosine", lr_noise=None, warmup_lr=1e-6,
             min_lr=1e-5, decay_epochs=30, warmup_epochs=5, cooldown_epochs=10, patience_epochs=10, decay_rate=0.1,
             distillation_type="soft", distillation_alpha=0.1, distillation_tau=1.0, enable_deit=0, local_rank=-1,
             precision="bf16", output_dir="output", name="post_train", steps_per_epoch=5005, compact_mlp=1, compact_multiple=256)
    a.update(over)
    return Namespace(**a)


def setup(args, device="cuda", model_cfg=None):
    """post_train.py:135-186: the student as Stage-2 builds it (default gate flags, i.e. hard block skip; ``gumbel_hard=True``) with
    mask buffers registered -> (args, model, its constructor keywords)."""
    t2t, cfg = model_config(args.model_type, model_cfg or getattr(args, "model_cfg", None))
    if t2t and args.enable_deit:                                    # post_train.py:165-167: t2t_vit_14() with the default flags
        raise NotImplementedError("T2T-ViT has no distillation token")
    model = build_model(args, device, cfg=cfg, gumbel_hard=True)
    register_masks(model)
    return args, model, model_kwargs(t2t, cfg, args, device)


class Stage2Trainer(_Trainer):
    STATE_FORMAT, NOT_A_STATE = "uvc_amd.stage2.v1", "not a uvc_amd Stage-2 training state"

    def __init__(self, args: Namespace, device="cuda", checkpoint=None, teacher_state=None, distributed=False, world_size=1):
        self.args = args
        args, model, _ = setup(args, device)
        teacher, self.teacher_source = None, None
        if args.distillation_type != "none":                                                        # :636-666
            # --teacher-model / --teacher-path (default: the model type / --model_path); with no weights at all it keeps its init
            teacher, self.teacher_source = build_teacher(args, device, teacher_state, verbose=getattr(args, "local_rank", -1) in (-1, 0))
        self.criterion = DistillationLoss(SoftTargetCrossEntropy(), teacher, args.distillation_type,
                                          args.distillation_alpha, args.distillation_tau)          # :668-671
        if checkpoint is not None:                                                                  # :676-683
            model.load_state_dict(match_pos_embed(checkpoint, model))       # `hasattr(checkpoint, 'args')` is never true for a dict: bare state_dict
        self.model, self.teacher = model, teacher
        self.total_param = count_mask(model)
        # structured sparsity: MLP hidden units whose fc1 row and fc2 column are masked out are skipped, not multiplied
        self.mlp_widths = model.set_mlp_compaction(multiple=getattr(args, "compact_multiple", 256)) if getattr(args, "compact_mlp", 1) else None
        self.head_keep = model.set_head_skipping() if getattr(args, "compact_mlp", 1) else None     # eval forwards skip pruned heads ...
        # ... and training BACKWARDS skip their dq / dk / dv: step() multiplies the weights by the masks before every forward (:343-346), so
        # dL/d(attention output) of a head whose 64 attn.proj input columns are masked is exactly zero (the forward keeps the head: the
        # reference's clip norm sees dW_proj of the masked columns, which needs its output)
        model.skip_pruned_head_grads = model._head_keep is not None
        # post_training(): DDP, scaled learning rate, timm optimiser + schedule (:289-301)
        self.ddp = DistributedDataParallel(model, message_size=250000000, gradient_predivide_factor=1.0) if distributed else None
        args.train_batch_size = args.train_batch_size // args.gradient_accumulation_steps
        args.lr = args.learning_rate * args.train_batch_size * world_size / 512.0
        self.optimizer = create_optimizer(args, model)
        self.scheduler, self.num_epochs = create_scheduler(args, self.optimizer)
        model.block_skip_gating.requires_grad = False                                               # :313
        model.train()
        self._start(accum=max(1, int(getattr(args, "gradient_accumulation_steps", 1))))            # :365-378

    def begin_epoch(self, epoch: int):
        """post_train.py:326-339."""
        self.epoch = epoch
        self._micro = 0          # `(step + 1) % k` on the epoch's loader index (:351,372): an accumulation window never straddles epochs
        self.model.train()
        self.model.block_skip_gating.requires_grad = False
        self.scheduler.step(epoch)

    def _before_forward(self):
        """post_train.py:341-377 after the odd-batch trim and mixup: mask, then _Trainer.step's forward (hard block skip), loss,
        backward, clip, AdamW."""
        self.model.apply_masks()                                                                    # :343-346

    # resumable state (the reference saves only the best model's bare state_dict, post_train.py:395-397)
    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        if getattr(self.args, "compact_mlp", 1):     # the pruned-head table and the MLP compaction of the loaded masks
            self.head_keep = self.model.set_head_skipping()
            self.mlp_widths = self.model.set_mlp_compaction(multiple=getattr(self.args, "compact_multiple", 256))
            self.model.skip_pruned_head_grads = self.model._head_keep is not None


def post_training(trainer, batches, epochs=None, valid_fn=None, log=print, save_best=None, prefix="[Stage 2]"):
    """The epoch loop of post_train.py:326-403 over an iterable factory ``batches(epoch)`` of device (x, y) pairs
    (mixup already applied); ``valid_fn(model) -> accuracy`` drives the save-best policy (:393-399) through ``save_best(trainer)``
    (default: the reference-format checkpoint, save_model).  Also the loop of ``compact finetune``, under its own ``prefix``."""
    a = trainer.args
    save_best = save_best or (lambda tr: save_model(a, tr.model, None, tr.global_step, barrier=False))
    best_acc = 0.0
    for epoch in range(epochs if epochs is not None else a.epochs):
        trainer.begin_epoch(epoch)
        t0 = time.time()
        last = None
        def trimmed():
            for x, y in batches(epoch):
                if len(x) % 2 != 0:                                                                 # :348-350
                    x, y = x[:-1], y[:-1]
                yield x, y
        # one batch read ahead (as the reference's prefetching loader holds it): the frozen teacher's forward for the NEXT batch starts behind this
        # step's backward (_Trainer.step's next_x; same results, tests/test_stage2_gpu.py)
        for (x, y), next_x in trainer.lookahead(trimmed()):
            last = trainer.step(x, y, next_x=next_x)
        lr = trainer.scheduler.get_epoch_values(epoch)[0]
        if last is not None:
            log(f"{prefix} epoch {epoch} steps {trainer.global_step} lr {lr:.6g} loss {float(last['loss']):.4f} "
                f"({time.time() - t0:.1f}s)")
        if valid_fn is not None and a.local_rank in (-1, 0):
            acc = valid_fn(trainer.model)
            if best_acc < acc:
                save_best(trainer)
                best_acc = acc
            trainer.model.train()
    return best_acc


def synthetic_batches(args, dev, g, hard=False):
    """``args.eval_steps`` (x, hard label) validation batches if ``hard``, else ``args.steps`` (x, soft target) training batches, drawn from ``g``."""
    B = args.eval_batch_size if hard else args.train_batch_size
    for _ in range(args.eval_steps if hard else args.steps):
        x = torch.randn(B, 3, args.img_size, args.img_size, device=dev, generator=g)
        if hard:
            yield x, torch.randint(0, args.num_classes, (B,), device=dev, generator=g)
        else:
            yield x, torch.softmax(torch.randn(B, args.num_classes, device=dev, generator=g), -1)


def synthetic_valid_fn(args, dev):
    """valid() on the same ``args.eval_steps`` synthetic batches at every call."""
    return top1_valid_fn(lambda: synthetic_batches(args, dev, torch.Generator(device=dev).manual_seed(args.seed + 77), hard=True))


def loader_valid_fn(test_loader):
    """valid() on the whole test set."""
    return top1_valid_fn(lambda: test_loader)


def valid_fn_of(args, dev, test_loader):
    """The drivers' choice: the test set with --synthetic 0, synthetic batches otherwise; None with --eval_steps 0."""
    if args.eval_steps <= 0:
        return None
    return loader_valid_fn(test_loader) if test_loader is not None else synthetic_valid_fn(args, dev)


def train_batches(args, dev, train_loader, mixup_fn, seed):
    """``batches(epoch)`` of a Stage-2 style run: the dataset's with ``mixup_fn`` (post_train.py:614-621), or synthetic ones from one
    generator seeded with ``seed``."""
    if train_loader is not None:
        from .data import soft_batches
        return lambda epoch: soft_batches(train_loader, epoch, mixup_fn, args.smoothing, args.data_classes, args.num_classes)
    g = torch.Generator(device=dev).manual_seed(seed)
    return lambda epoch: synthetic_batches(args, dev, g)


def eval_model(args, device, checkpoint=None, model_path=None):
    """--eval_only: the Stage-2 model from a Stage-1 checkpoint (strict load) or else a pretrained file (load_pretrained), masked as
    every Stage-2 forward is (post_train.py:343-346), in eval mode."""
    if checkpoint is None and not model_path:
        raise SystemExit("--eval_only 1 needs --checkpoint_dir or --model_path")
    _, model, _ = setup(args, device)
    if checkpoint is not None:
        model.load_state_dict(match_pos_embed(checkpoint, model))
    else:
        load_pretrained(model_path, model, num_classes=args.num_classes, what="model", verbose=args.local_rank in (-1, 0))
    model.apply_masks()
    model.eval()
    return model


def add_stage2_flags(p, skip=()):
    """Stage 2's command-line flags on the parser ``p`` (``default_args`` as ``--name`` flags, then the run, data, Mixup and teacher
    flags); ``skip``: names a caller defines itself."""
    add = lambda *names, **kw: None if names[0].lstrip("-") in skip else p.add_argument(*names, **kw)
    d = default_args()
    for k, v in vars(d).items():
        if v is None or isinstance(v, (list, tuple)):
            add("--" + k, default=v)
        else:
            add("--" + k, type=type(v), default=v)
    add("--checkpoint_dir", type=str, default=None, help="Stage-1 checkpoint (bare state_dict)")
    add("--steps", type=int, default=20, help="steps per synthetic epoch")
    add("--model_cfg", type=str, default=None, help="JSON dims for a --model_type outside models/configs.py (tests)")
    add("--eval_steps", type=int, default=2, help="synthetic validation batches per epoch (valid(), post_train.py:188-234)")
    add("--eval_batch_size", type=int, default=64)
    add("--synthetic", type=int, default=1, help="synthetic batches; 0 = read --dataset under --data_dir")
    add_data_flags(p, data_dir="/ssd1/xinyu/dataset/imagenet2012", num_workers=8, num_workers_help="decode threads (at most 16)", add=add)
    # Stage-2 Mixup / CutMix and smoothing (post_train.py:502,539-550): applied on the real-data path only
    add("--smoothing", type=float, default=0.1)
    add_mixup_flags(p, add=add)
    # pretrained weights (post_train.py:422,554-556,635-640); the reference's --model_path default is a URL, and nothing is downloaded here
    add("--model_path", type=str, default=None, help="pretrained checkpoint: the teacher's default source, and the model of --eval_only without --checkpoint_dir")
    add_teacher_flags(p, default="", described=True, add=add)
    add("--teacher_cfg", type=str, default=None, help="with --teacher-model custom / custom_t2t: the teacher's JSON dims")
    add("--eval_only", type=int, default=0, help="1: evaluate the model once (valid()) and print the JSON line, no training")
    return p


def main(argv=None):
    """Stage-2 run: loads a Stage-1 checkpoint and fine-tunes it on synthetic batches (``--synthetic 1``, the default) or on
    ``--dataset`` under ``--data_dir`` (``--synthetic 0``: uvc_amd/data.py, with the reference's Mixup / CutMix, post_train.py:614-621)."""
    p = add_stage2_flags(argparse.ArgumentParser(description="UVC Stage-2 masked fine-tune on MI355X"))
    args = p.parse_args(argv)
    if args.model_cfg:
        args.model_cfg = json.loads(args.model_cfg)
    rank, local, world = init_distributed()
    if world > 1:
        args.local_rank = local
    train_loader, test_loader = train_loaders(args, rank, world)
    ck = torch.load(args.checkpoint_dir, map_location="cpu") if args.checkpoint_dir else None
    dev = torch.device("cuda", local)
    if args.eval_only:
        tr, model = None, eval_model(args, dev, ck, args.model_path)
        acc = (loader_valid_fn(test_loader) if test_loader is not None else synthetic_valid_fn(args, dev))(model)
        result = dict(steps=0, masked_params_M=float(count_mask(model)), best_acc=acc)
    else:
        tr = Stage2Trainer(args, device=f"cuda:{local}", checkpoint=ck, distributed=world > 1, world_size=world)
        mixup_fn = None
        if train_loader is not None:                 # --synthetic 0: Mixup / CutMix as the reference builds it (:614-621)
            mixup_fn = seeded_mixup(args, real=True)
            if rank == 0:
                print(f"mixup active: {mixup_fn is not None}")
        best = post_training(tr, train_batches(args, dev, train_loader, mixup_fn, args.seed + rank), epochs=args.epochs,
                             valid_fn=valid_fn_of(args, dev, test_loader), log=print if rank == 0 else (lambda *_: None))
        result = dict(steps=tr.global_step, masked_params_M=float(tr.total_param), best_acc=best)
    if rank == 0:
        print(json.dumps(result))
    if world > 1:
        torch.distributed.destroy_process_group()
    return model if tr is None else tr


if __name__ == "__main__":
    main()
