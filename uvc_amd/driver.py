"""What the command-line drivers share (``cli`` = Stage 1, ``post_train`` = Stage 2, ``compact eval`` and ``compact finetune``): the data,
Mixup and teacher flags, written once, the process-group set-up, the real-data loaders with their Mixup, and the top-1 validation loop.
A flag of one of these blocks is added here and nowhere else; where the drivers' defaults differ, the call site says so.
The stand-alone compact tools have two blocks of their own, kept the same way: ``compact_tools.add_dataset_flags`` (one split under the eval
transform) and ``compact.add_image_file_flags`` (image files).
"""
from __future__ import annotations

import os

import torch


def add_data_flags(p, *, data_dir, num_workers, num_workers_help=None, add=None):
    """--dataset --data_dir --num_workers --packed_dir --resident --interpolation --crop_pct: what build_loaders reads.  ``add``: the
    caller's ``add_argument`` (one that leaves out the names the caller defines itself); default ``p.add_argument``."""
    from .data import add_image_args
    add = add or p.add_argument
    add("--dataset", choices=["cifar10", "cifar100", "imagenet"], default="imagenet")              # joint_train.py:686, post_train.py:411-414
    add("--data_dir", default=data_dir)
    add("--num_workers", type=int, default=num_workers, help=num_workers_help)                      # joint_train.py:691, post_train.py:417
    add("--packed_dir", default=None, help="DIR/train.uvcpack and DIR/val.uvcpack (python -m uvc_amd.packed pack) replace the folders or pickles under --data_dir")
    add("--resident", type=int, default=0, choices=[0, 1], help="1: upload the dataset to the GPU once and crop it there (CIFAR, or any dataset with --packed_dir); in data-parallel runs every rank holds the whole store, because the sampler hands any image to any rank")
    add_image_args(p)


def add_mixup_flags(p, add=None):
    """Mixup / CutMix (joint_train.py:762-776, post_train.py:539-550); --smoothing stands where each reference parser has it."""
    add = add or p.add_argument
    add("--mixup", type=float, default=0.8); add("--cutmix", type=float, default=1.0)
    add("--cutmix-minmax", type=float, nargs="+", default=None); add("--mixup-prob", type=float, default=0.8)
    add("--mixup-switch-prob", type=float, default=0.5); add("--mixup-mode", type=str, default="batch")


def add_teacher_flags(p, *, default, described=False, add=None):
    """--teacher-model / --teacher-path (joint_train.py:777-779, post_train.py:554-556).  ``default``: what an absent flag parses to, None
    in Stage 1 and "" in Stage 2 as in the reference (build_teacher takes both for "not given"); ``described``: with help texts."""
    add = add or p.add_argument
    add("--teacher-model", type=str, default=default, help="teacher architecture (default: --model_type)" if described else None)
    add("--teacher-path", type=str, default=default, help="teacher checkpoint (default: --model_path)" if described else None)


def init_distributed(local=None):
    """(rank, local rank, world size) of a torchrun process, on its own device (``local``: Stage 1's --local_rank; default: the
    environment's); with more than one process the NCCL group is up."""
    rank, env_local, world = (int(os.environ.get(k, d)) for k, d in (("RANK", 0), ("LOCAL_RANK", 0), ("WORLD_SIZE", 1)))
    local = env_local if local is None else local
    torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.distributed.init_process_group("nccl")
    return rank, local, world


def train_loaders(args, rank, world):
    """--synthetic 0: (train, test) loaders of --dataset (get_loader, joint_train.py:272), args.steps_per_epoch = len(train_loader);
    --synthetic 1: (None, None)."""
    if args.synthetic:
        return None, None
    from . import data
    train_loader, test_loader = data.build_loaders(args, rank=rank, world=world)
    args.steps_per_epoch = train_loader.train_steps()
    return train_loader, test_loader


def seeded_mixup(args, real):
    """numpy's global RNG seeded (Mixup draws from it: set_seed, joint_train.py:191-196), then the reference's Mixup / CutMix or None:
    over the dataset's classes on real data (a padded head's extra columns get zero targets), over args.num_classes otherwise."""
    import numpy as np
    from .data import real_mixup
    from .mixup import build_mixup
    np.random.seed(args.seed)
    return real_mixup(args) if real else build_mixup(args)


def top1_valid_fn(batches_fn):
    """valid() of post_train.py:188-234 as ``valid_fn(model) -> top-1 in percent`` over the (x, hard label) batches of ``batches_fn()``:
    eval-mode logits; + epsilon: the first epoch always beats best_acc = 0 and saves (:393-397)."""
    @torch.no_grad()
    def valid_fn(model):
        from .model_distilled import drop_shared_patches
        model.eval()
        hit, n = 0, 0
        for x, t in batches_fn():
            logits, _ = model(x)
            hit = hit + (logits.argmax(dim=1) == t).sum()
            n += len(t)
        drop_shared_patches()
        return 100.0 * (int(hit) + 1e-3) / max(n, 1)
    return valid_fn
