"""Real image datasets for both stages (the loaders of ``UVC/utils/data_utils.py:13-105``) with the per-pixel work on the GPU.

Decoding stays on the CPU (PIL, in threads: PIL releases the GIL while it decodes); the random resized crop is a slice of the
decoded array, so only the crop's pixels are uploaded; resampling, flip, ToTensor and Normalize run in one ragged HIP batch
(``uvc_image_prep``, include/uvc_data.h), bit for bit what torchvision's transforms give on the PIL image.  The resampling filter is
bilinear, torchvision's default and the reference's, or bicubic (``interpolation``), what the released DeiT and T2T-ViT checkpoints
were trained and evaluated with; ``crop_pct`` sets the eval resize by timm's rule (eval_resize_side).

    ImageFolder(root)            torchvision.datasets.ImageFolder indexing (sorted classes, os.walk(followlinks=True), IMG_EXTENSIONS)
    read_cifar(root, name, train) the local python-pickle CIFAR-10 / CIFAR-100 layout, nothing is downloaded -> ArrayDataset
    ArrayDataset(images, labels) uint8 [N, H, W, 3] in memory
    FileListDataset(paths)       image files in the order given, loaded as the folder dataset loads them, dummy targets (compact predict)
    DeviceLoader(...)            (x float32 [B, 3, S, S] cuda, target int64 cuda) batches, DistributedSampler order
    (uvc_amd/packed.py: PackedDataset, a dataset decoded once into one file, and ResidentLoader, the same batches from pixels that stay on the GPU)
    build_loaders(args, ...)     the reference's train / test loaders for --dataset cifar10 | cifar100 | imagenet

Deviations from the reference, on purpose (DESIGN.md "Real image data"): the training order is reshuffled every epoch (the
reference never calls ``DistributedSampler.set_epoch``), CIFAR-100 is read from ``--data_dir`` (the reference hard-codes
``./data``), and the crop / flip draws come from a counter-based stream keyed by (seed, epoch, dataset index), so a sample's crop
does not depend on the rank count, the worker count or thread timing.
"""
from __future__ import annotations

import math
import os
import pickle
import queue
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CIFAR_MEAN, CIFAR_STD = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)
MAX_THREADS = 16


# ---------------------------------------------------------------------------------------------------------------- datasets

class ImageFolder:
    """torchvision.datasets.ImageFolder's indexing: classes are the sorted subdirectories of ``root``; each class's files come
    from os.walk(followlinks=True), directories and names sorted, extensions matched case-insensitively; images load as
    ``Image.open(f).convert("RGB")``."""

    def __init__(self, root):
        self.root = root
        self.classes = sorted(e.name for e in os.scandir(root) if e.is_dir())
        if not self.classes:
            raise FileNotFoundError(f"no class folders found in {root}")
        self.class_to_idx = {c: i for i, c in enumerate(self.classes)}
        self.samples = []
        for c in self.classes:
            for dirpath, _, fnames in sorted(os.walk(os.path.join(root, c), followlinks=True)):
                for f in sorted(fnames):
                    if f.lower().endswith(IMG_EXTENSIONS):
                        self.samples.append((os.path.join(dirpath, f), self.class_to_idx[c]))
        if not self.samples:
            raise FileNotFoundError(f"no images with extensions {IMG_EXTENSIONS} found in {root}")
        self.targets = np.asarray([t for _, t in self.samples], dtype=np.int64)

    def __len__(self):
        return len(self.samples)

    def load(self, i):
        """uint8 [H, W, 3] pixels of sample i."""
        return _open_rgb(self.samples[i][0])


class ArrayDataset:
    """uint8 [N, H, W, 3] images with int64 labels, in memory (CIFAR, tests, timing)."""

    def __init__(self, images, labels):
        images = np.ascontiguousarray(images)
        if images.dtype != np.uint8 or images.ndim != 4 or images.shape[3] != 3:
            raise ValueError("ArrayDataset wants uint8 [N, H, W, 3] images")
        self.images = images
        self.targets = np.asarray(labels, dtype=np.int64)
        if len(self.targets) != len(images):
            raise ValueError("one label per image")

    def __len__(self):
        return len(self.images)

    def load(self, i):
        return self.images[i]


def _open_rgb(path):
    """uint8 [H, W, 3] pixels of an image file: ``Image.open(f).convert("RGB")``, as torchvision's folder loader."""
    from PIL import Image
    with open(path, "rb") as f:
        img = Image.open(f)
        return np.asarray(img.convert("RGB"))


class FileListDataset:
    """Image files in the order given, without labels (targets are zeros): what ``python -m uvc_amd.compact predict`` classifies.
    ``load(i)`` is ImageFolder's (RGB conversion included).  ``tolerant``: a file that cannot be read or decoded does not end the
    epoch; its message goes to ``errors[i]`` and one black pixel stands in for it, so the batches keep their order and size."""

    def __init__(self, paths, tolerant=False):
        self.paths = [os.fspath(p) for p in paths]
        self.targets = np.zeros(len(self.paths), dtype=np.int64)
        self.tolerant, self.errors = bool(tolerant), {}

    def __len__(self):
        return len(self.paths)

    def load(self, i):
        if not self.tolerant:
            return _open_rgb(self.paths[i])
        try:
            return _open_rgb(self.paths[i])
        except Exception as e:                          # noqa: BLE001 (PIL raises OSError, SyntaxError, ValueError, ... on damaged files)
            self.errors[i] = f"{type(e).__name__}: {e}"
            return np.zeros((1, 1, 3), dtype=np.uint8)


def list_images(paths):
    """The image files ``paths`` name, in order: a file as it is (whatever its extension), a directory walked recursively for
    IMG_EXTENSIONS (case-insensitive) with directories and names sorted, as ImageFolder walks a class folder."""
    out = []
    for p in paths:
        p = os.fspath(p)
        if os.path.isdir(p):
            for dirpath, _, fnames in sorted(os.walk(p, followlinks=True)):
                out.extend(os.path.join(dirpath, f) for f in sorted(fnames) if f.lower().endswith(IMG_EXTENSIONS))
        elif os.path.exists(p):
            out.append(p)
        else:
            raise FileNotFoundError(f"{p}: no such file or directory")
    return out


def read_cifar(root, name, train):
    """torchvision's CIFAR10 / CIFAR100 from the extracted python pickles under ``root`` (cifar-10-batches-py/data_batch_1..5,
    test_batch; cifar-100-python/train, test with fine_labels).  Rows are CHW bytes, returned as HWC."""
    if name == "cifar10":
        base, files, key = "cifar-10-batches-py", ([f"data_batch_{i}" for i in range(1, 6)] if train else ["test_batch"]), "labels"
    elif name == "cifar100":
        base, files, key = "cifar-100-python", (["train"] if train else ["test"]), "fine_labels"
    else:
        raise ValueError(name)
    data, labels = [], []
    for f in files:
        path = os.path.join(root, base, f)
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} not found: extract the python version of {name} under --data_dir (nothing is downloaded)")
        with open(path, "rb") as fh:
            entry = pickle.load(fh, encoding="latin1")
        data.append(np.asarray(entry["data"], dtype=np.uint8))
        labels.extend(entry[key] if key in entry else entry["labels"])
    images = np.vstack(data).reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)
    return ArrayDataset(images, np.asarray(labels, dtype=np.int64))


# ---------------------------------------------------------------------------------------------------------------- order and draws

def epoch_indices(n, epoch, seed=0, rank=0, world=1, shuffle=True):
    """torch.utils.data.DistributedSampler(drop_last=False) after set_epoch(epoch): randperm(n) of a generator seeded seed + epoch,
    padded from its head to a multiple of world, then every world-th index from rank: ceil(n / world) indices."""
    if shuffle:
        g = torch.Generator()
        g.manual_seed(seed + epoch)
        idx = torch.randperm(n, generator=g).tolist()
    else:
        idx = list(range(n))
    num_samples = math.ceil(n / world)
    total = num_samples * world
    pad = total - n
    if pad <= len(idx):
        idx += idx[:pad]
    else:
        idx += (idx * math.ceil(pad / len(idx)))[:pad]
    return idx[rank:total:world]


def _mix64(z):
    """splitmix64 finalizer on uint64 arrays (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def sample_uniforms(seed, epoch, index, n):
    """float64 [len(index), n] uniforms in [0, 1), a pure function of (seed, epoch, dataset index, slot)."""
    index = np.asarray(index, dtype=np.uint64).reshape(-1, 1)
    with np.errstate(over="ignore"):
        k = _mix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + np.uint64(0x9E3779B97F4A7C15))
        k = _mix64(k ^ (np.uint64(epoch & 0xFFFFFFFFFFFFFFFF) * np.uint64(0xD1342543DE82EF95)))
        k = _mix64(k ^ (index * np.uint64(0xC2B2AE3D27D4EB4F)))
        z = _mix64(k + np.arange(1, n + 1, dtype=np.uint64).reshape(1, -1) * np.uint64(0x9E3779B97F4A7C15))
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))


RRC_DRAWS = 41          # 10 attempts x (area, log-ratio, top, left) + the flip


def rrc_params(h, w, u, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """torchvision RandomResizedCrop.get_params, vectorised: h, w int arrays [B], u [B, >= 40] uniforms.  Up to ten attempts of
    (target area ~ U(scale) * area, aspect = exp(U(log ratio)), w = int(round(sqrt(a * r))), h = int(round(sqrt(a / r)))), the first
    that fits wins with a uniform top / left; otherwise the central fallback clamped to the ratio range.  Returns (i, j, ch, cw)."""
    h = np.asarray(h, dtype=np.int64).reshape(-1)
    w = np.asarray(w, dtype=np.int64).reshape(-1)
    area = (h * w).astype(np.float64)
    lr0, lr1 = (float(v) for v in torch.log(torch.tensor(ratio)))        # float32 log ratio, as torchvision
    i = np.zeros_like(h); j = np.zeros_like(h); ch = h.copy(); cw = w.copy()
    done = np.zeros(len(h), dtype=bool)
    for k in range(10):
        ta = area * (scale[0] + (scale[1] - scale[0]) * u[:, 4 * k])
        ar = np.exp(lr0 + (lr1 - lr0) * u[:, 4 * k + 1])
        tw = np.rint(np.sqrt(ta * ar)).astype(np.int64)                    # round half to even, like Python's round
        th = np.rint(np.sqrt(ta / ar)).astype(np.int64)
        ok = ~done & (tw > 0) & (tw <= w) & (th > 0) & (th <= h)
        ti = np.floor(u[:, 4 * k + 2] * (h - th + 1)).astype(np.int64)
        tj = np.floor(u[:, 4 * k + 3] * (w - tw + 1)).astype(np.int64)
        i = np.where(ok, ti, i); j = np.where(ok, tj, j); ch = np.where(ok, th, ch); cw = np.where(ok, tw, cw)
        done |= ok
    if not done.all():
        for b in np.nonzero(~done)[0]:
            H, W = int(h[b]), int(w[b])
            in_ratio = float(W) / float(H)
            if in_ratio < min(ratio):
                fw, fh = W, int(round(W / min(ratio)))
            elif in_ratio > max(ratio):
                fh, fw = H, int(round(H * max(ratio)))
            else:
                fw, fh = W, H
            i[b], j[b], ch[b], cw[b] = (H - fh) // 2, (W - fw) // 2, fh, fw
    return i, j, ch, cw


def resize_short_side(h, w, size):
    """torchvision Resize(int) output (new_h, new_w): the short side becomes size, the long side int(size * long / short)."""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    return (new_long, new_short) if w <= h else (new_short, new_long)


INTERPOLATIONS = ("bilinear", "bicubic")


def eval_resize_side(S, crop_pct=None):
    """Short side the eval transform resizes to before CenterCrop(S).  crop_pct None: the reference's S * 256 // 224 (256 at 224);
    otherwise timm's int(math.floor(S / crop_pct)): 0.875 -> 256, 0.9 -> 248, 1.0 -> S at 224.  crop_pct must lie in (0, 1]."""
    if crop_pct is None:
        return S * 256 // 224
    crop_pct = float(crop_pct)
    if not 0.0 < crop_pct <= 1.0:                       # (nan fails both comparisons)
        raise ValueError(f"crop_pct must lie in (0, 1], not {crop_pct}")
    return int(math.floor(S / crop_pct))


def _pil_filter(interpolation):
    from PIL import Image
    if interpolation not in INTERPOLATIONS:
        raise ValueError(f"interpolation must be one of {INTERPOLATIONS}, not {interpolation!r}")
    return Image.BICUBIC if interpolation == "bicubic" else Image.BILINEAR


def center_crop_offset(h, w, S):
    """torchvision CenterCrop(S) top-left: int(round((h - S) / 2.0)), Python's round half to even."""
    return int(round((h - S) / 2.0)), int(round((w - S) / 2.0))


# ---------------------------------------------------------------------------------------------------------------- device loader

class _Slot:
    """Pinned host staging of one batch; reused only after the kernel that read its upload has finished (``done``)."""

    def __init__(self):
        self.pixels = torch.empty(0, dtype=torch.uint8).pin_memory()
        self.desc = None
        self.labels = None
        self.done = None
        self.n = 0
        self.src_bytes = 0
        self.ws_bytes = 0


def _grow_pinned(t, nbytes):
    if t.numel() >= nbytes:
        return t
    return torch.empty(max(nbytes, 2 * t.numel(), 1 << 16), dtype=torch.uint8).pin_memory()


class DeviceLoader:
    """Batches of (x float32 [B, 3, S, S] on the GPU, target int64 on the GPU).

    output="image" (default): x as above.  output="patches": x is the batch's patch rows instead, [B * (S / patch_size)^2,
    3 * patch_size^2] in ``dtype`` (torch.bfloat16 or torch.float32) -- bit for bit ops.patchify of the image batch, written by the
    resampler's last pass (uvc_image_prep_patches) without the float32 images in between; what a ViT forward takes as ``patches=``.

    train=True : RandomResizedCrop(S, scale, ratio) [+ RandomHorizontalFlip] + Normalize, DistributedSampler order (rank, world,
                 reshuffled by set_epoch), drop_last=False: the last batch is short.
    train=False: every sample in order; eval="center": Resize(eval_resize_side(S, crop_pct)) + CenterCrop(S) (ImageNet: 256 / 224
                 by default), eval="square": Resize((S, S)) (CIFAR test; crop_pct does not apply).
    interpolation: "bilinear" (default) or "bicubic", the filter of the training crop's resize and of the eval resize alike.
    A thread pool of min(num_workers, 16) threads decodes and crops into a pinned staging slot, about ``ahead`` batches ahead of
    the consumer; the pixels and descriptors go up on a side copy stream; the current stream waits on its event and runs the
    three uvc_image_prep launches into a freshly allocated x."""

    def __init__(self, dataset, batch_size, img_size, train=True, mean=IMAGENET_MEAN, std=IMAGENET_STD, scale=(0.08, 1.0),
                 ratio=(3.0 / 4.0, 4.0 / 3.0), flip=True, eval="center", seed=0, rank=0, world=1, num_workers=4, device=None, ahead=2,
                 interpolation="bilinear", crop_pct=None, output="image", patch_size=None, dtype=None):
        from . import ops
        if eval not in ("center", "square"):
            raise ValueError(eval)
        if output not in ("image", "patches"):
            raise ValueError(f"output must be 'image' or 'patches', not {output!r}")
        self.output, self.patch_size, self.dtype = output, None, torch.float32
        if output == "patches":
            if patch_size is None or int(patch_size) <= 0 or int(img_size) % int(patch_size):
                raise ValueError(f"output='patches' needs a patch_size that divides img_size {img_size}, not {patch_size!r}")
            if dtype not in (torch.bfloat16, torch.float32):
                raise ValueError(f"output='patches' needs dtype torch.bfloat16 or torch.float32, not {dtype!r}")
            self.patch_size, self.dtype = int(patch_size), dtype
        elif patch_size is not None or dtype is not None:
            raise ValueError("patch_size and dtype belong to output='patches'")
        self.interpolation, self.crop_pct = interpolation, crop_pct
        self.filter = ops.image_filter(interpolation)
        self.eval_side = eval_resize_side(int(img_size), crop_pct)
        self.dataset, self.batch_size, self.S, self.train = dataset, int(batch_size), int(img_size), bool(train)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.scale, self.ratio, self.flip, self.eval = tuple(scale), tuple(ratio), bool(flip), eval
        self.seed, self.rank, self.world = int(seed), int(rank), int(world)
        self.threads = max(0, min(int(num_workers), MAX_THREADS))
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.ahead = max(1, int(ahead))
        self.epoch = 0
        self._pool = ThreadPoolExecutor(self.threads) if self.threads > 1 else None
        self._copy_stream = None

    def __len__(self):
        n = math.ceil(len(self.dataset) / self.world) if self.train else len(self.dataset)
        return math.ceil(n / self.batch_size)

    def train_steps(self):
        """Batches the trainers step on per epoch: a last batch of one sample is trimmed to nothing (odd-batch trim) and skipped."""
        n = math.ceil(len(self.dataset) / self.world) if self.train else len(self.dataset)
        return len(self) - (1 if n % self.batch_size == 1 else 0)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def indices(self):
        """Dataset indices this rank sees in the current epoch, in order."""
        if self.train:
            return epoch_indices(len(self.dataset), self.epoch, self.seed, self.rank, self.world, shuffle=True)
        return list(range(len(self.dataset)))

    # -- host side: one batch into a staging slot
    def _map(self, fn, n):
        """fn(lo, hi) over contiguous chunks of range(n), on the pool when there is one."""
        if self._pool is None or n < 2:
            fn(0, n)
            return
        k = min(self.threads, n)
        bounds = [(n * c // k, n * (c + 1) // k) for c in range(k)]
        for f in [self._pool.submit(fn, lo, hi) for lo, hi in bounds]:
            f.result()

    def _geometry(self, hw, u):
        """Per-sample (i, j, ch, cw, resize_h, resize_w, win_y, win_x, flip) for sources of sizes hw [B, 2]."""
        S, B = self.S, len(hw)
        g = np.zeros((B, 9), dtype=np.int64)
        if self.train:
            i, j, ch, cw = rrc_params(hw[:, 0], hw[:, 1], u, self.scale, self.ratio)
            g[:, 0], g[:, 1], g[:, 2], g[:, 3] = i, j, ch, cw
            g[:, 4] = g[:, 5] = S
            g[:, 8] = (u[:, 40] < 0.5) if self.flip else 0
        else:
            g[:, 2], g[:, 3] = hw[:, 0], hw[:, 1]
            for b in range(B):
                h, w = int(hw[b, 0]), int(hw[b, 1])
                if self.eval == "square":
                    rh, rw, wy, wx = S, S, 0, 0
                else:
                    rh, rw = resize_short_side(h, w, self.eval_side)
                    wy, wx = center_crop_offset(rh, rw, S)
                g[b, 4:8] = rh, rw, wy, wx
        return g

    def _fill(self, slot, idx):
        from . import ops
        B = len(idx)
        ds = self.dataset
        u = sample_uniforms(self.seed, self.epoch, idx, RRC_DRAWS) if self.train else None
        if isinstance(ds, ArrayDataset):
            imgs = [ds.images[k] for k in idx]
        else:
            imgs = [None] * B

            def decode(lo, hi):
                for b in range(lo, hi):
                    imgs[b] = ds.load(idx[b])
            self._map(decode, B)
        hw = np.asarray([im.shape[:2] for im in imgs], dtype=np.int64).reshape(B, 2)
        g = self._geometry(hw, u)
        sizes = g[:, 2] * g[:, 3] * 3
        offs = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(sizes, out=offs[1:])
        total = int(offs[-1])
        slot.pixels = _grow_pinned(slot.pixels, total)
        stage = slot.pixels.numpy()

        def copy(lo, hi):
            for b in range(lo, hi):
                i, j, ch, cw = (int(v) for v in g[b, :4])
                np.copyto(stage[offs[b]:offs[b + 1]].reshape(ch, cw, 3), imgs[b][i:i + ch, j:j + cw])
        self._map(copy, B)
        desc = np.zeros(B, dtype=ops.image_desc_dtype())
        desc["src_offset"] = offs[:-1]
        desc["src_h"], desc["src_w"] = g[:, 2], g[:, 3]
        desc["resize_h"], desc["resize_w"], desc["win_y"], desc["win_x"], desc["flip"] = g[:, 4], g[:, 5], g[:, 6], g[:, 7], g[:, 8]
        slot.ws_bytes = ops.image_prep_workspace(desc, self.S, total, self.filter)
        nb = desc.nbytes
        if slot.desc is None or slot.desc.numel() < nb:
            slot.desc = torch.empty(max(nb, 64 * 512), dtype=torch.uint8).pin_memory()
            slot.labels = torch.empty(max(B, 512), dtype=torch.int64).pin_memory()
        slot.desc.numpy()[:nb] = desc.view(np.uint8)
        slot.labels.numpy()[:B] = ds.targets[np.asarray(idx, dtype=np.int64)]
        slot.n, slot.src_bytes = B, total

    def _producer(self, batches, free, ready, stop):
        try:
            for idx in batches:
                slot = free.get()
                if slot is None or stop.is_set():
                    return
                if slot.done is not None:
                    slot.done.synchronize()             # the kernel that read this slot's last upload has finished
                self._fill(slot, idx)
                ready.put(slot)
            ready.put(None)
        except BaseException as e:                      # noqa: BLE001 (re-raised in the consumer)
            ready.put(e)

    # -- device side: the upload of one slot and the launches that read it (ResidentLoader in uvc_amd/packed.py replaces these four)
    def _new_slot(self):
        return _Slot()

    def _new_copy_stream(self):
        return torch.cuda.Stream(self.device)

    def _upload(self, slot):
        """With the copy stream current: allocates the slot's device buffers and starts their copies.  Returns the buffers."""
        B = slot.n
        target = torch.empty(B, dtype=torch.int64, device=self.device)
        src = torch.empty(max(slot.src_bytes, 1), dtype=torch.uint8, device=self.device)
        desc = torch.empty(B * 64, dtype=torch.uint8, device=self.device)
        src[:slot.src_bytes].copy_(slot.pixels[:slot.src_bytes], non_blocking=True)
        desc.copy_(slot.desc[:B * 64], non_blocking=True)
        target.copy_(slot.labels[:B], non_blocking=True)
        return target, src, desc

    def _launch(self, slot, up, ws, x):
        """With the consumer's stream current, after the upload: the three launches into x.  Returns the batch's target."""
        from . import ops
        target, src, desc = up
        if self.output == "patches":
            ops.image_prep_patches(src[:max(slot.src_bytes, 1)], desc, ws, x, self.patch_size, self.S, self.mean, self.std, self.filter)
        else:
            ops.image_prep(src[:max(slot.src_bytes, 1)], desc, ws, x, self.mean, self.std, self.filter)
        return target

    def _new_batch(self, B):
        """The uninitialised output of one batch of B images."""
        if self.output == "patches":
            P = self.patch_size
            return torch.empty(B * (self.S // P) ** 2, 3 * P * P, dtype=self.dtype, device=self.device)
        return torch.empty(B, 3, self.S, self.S, dtype=torch.float32, device=self.device)

    def __iter__(self):
        idx = self.indices()
        batches = [idx[o:o + self.batch_size] for o in range(0, len(idx), self.batch_size)]
        if not batches:
            return
        if self._copy_stream is None:
            self._copy_stream = self._new_copy_stream()
        main = torch.cuda.current_stream(self.device)
        free, ready, stop = queue.Queue(), queue.Queue(), threading.Event()
        for _ in range(self.ahead + 1):
            free.put(self._new_slot())
        t = threading.Thread(target=self._producer, args=(batches, free, ready, stop), daemon=True)
        t.start()
        try:
            while True:
                slot = ready.get()
                if slot is None:
                    break
                if isinstance(slot, BaseException):
                    raise slot
                B = slot.n
                # everything the copy stream writes is allocated on the copy stream and handed to `main` with record_stream: a block the
                # allocator gives out on `main` may still be in use by kernels queued there, which the copy stream does not wait for
                with torch.cuda.stream(self._copy_stream):
                    up = self._upload(slot)
                    uploaded = torch.cuda.Event()
                    uploaded.record(self._copy_stream)
                main.wait_event(uploaded)
                ws = torch.empty(max(slot.ws_bytes, 16), dtype=torch.uint8, device=self.device)
                x = self._new_batch(B)
                with torch.cuda.stream(main):
                    target = self._launch(slot, up, ws, x)
                for buf in up:
                    buf.record_stream(main)
                slot.done = torch.cuda.Event()
                slot.done.record(main)
                free.put(slot)
                yield x, target
        finally:
            stop.set()
            free.put(None)                               # wakes a producer blocked on a slot
            t.join()


def host_reference_batch(dataset, indices, S, train, seed, epoch, mean, std, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), flip=True,
                         eval="center", interpolation="bilinear", crop_pct=None):
    """The same batch the loader yields, built the reference's way on the host: PIL crop().resize(BILINEAR or BICUBIC), flip, ToTensor,
    Normalize (float32 [B, 3, S, S] on the CPU).  Tests and tools hold the device path to it."""
    from PIL import Image
    resample = _pil_filter(interpolation)
    side = eval_resize_side(S, crop_pct)
    xs = []
    u = sample_uniforms(seed, epoch, indices, RRC_DRAWS) if train else None
    for b, k in enumerate(indices):
        a = dataset.load(k)
        im = Image.fromarray(np.ascontiguousarray(a))
        h, w = a.shape[:2]
        if train:
            i, j, ch, cw = (int(v[0]) for v in rrc_params([h], [w], u[b:b + 1], scale, ratio))
            im = im.crop((j, i, j + cw, i + ch)).resize((S, S), resample)
            if flip and u[b, 40] < 0.5:
                im = im.transpose(Image.FLIP_LEFT_RIGHT)
        elif eval == "square":
            im = im.resize((S, S), resample)
        else:
            rh, rw = resize_short_side(h, w, side)
            im = im.resize((rw, rh), resample)
            y0, x0 = center_crop_offset(rh, rw, S)
            im = im.crop((x0, y0, x0 + S, y0 + S))
        t = torch.from_numpy(np.array(im, dtype=np.uint8)).permute(2, 0, 1).float().div(255)
        xs.append((t - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1))
    return torch.stack(xs)


# ---------------------------------------------------------------------------------------------------------------- drivers

def build_loaders(args, rank=0, world=1, splits=("train", "test")):
    """get_loader (data_utils.py:13-105) for --dataset cifar10 | cifar100 | imagenet under --data_dir: (train, test) DeviceLoaders.
    A loader whose split is not in ``splits`` is None (compact eval asks for "test" alone, so --resident 1 uploads no train store).
    --packed_dir DIR reads DIR/train.uvcpack and DIR/val.uvcpack (uvc_amd/packed.py) in place of the folders or pickles; --resident 1
    returns ResidentLoaders, which keep the pixels on the device (CIFAR's in-memory arrays, or a pack).
    --interpolation bilinear | bicubic is the resampling filter of every loader, train and test; --crop_pct P resizes ImageNet's eval
    images to floor(img_size / P) before the centre crop (eval_resize_side; CIFAR's square eval resize ignores it).
    Sets args.data_classes to the dataset's class count: 10 / 100 for CIFAR, as in the reference, args.num_classes for ImageNet (the folder's
    class count must fit it).  The model head is args.num_classes wide, a multiple of 8 for the engine: for CIFAR it becomes 16 / 104; the
    soft targets cover the data classes and are zero on the padded logits (soft_batches)."""
    S = args.img_size
    nw = getattr(args, "num_workers", 4)
    seed = getattr(args, "seed", 0)
    packed_dir = getattr(args, "packed_dir", None)
    resident = bool(int(getattr(args, "resident", 0) or 0))
    interpolation = getattr(args, "interpolation", None) or "bilinear"
    crop_pct = getattr(args, "crop_pct", None)
    _pil_filter(interpolation)
    eval_resize_side(S, crop_pct)                       # refuses a crop_pct outside (0, 1] before a dataset is opened
    Loader = DeviceLoader
    if packed_dir or resident:
        from .packed import EXTENSION, PackedDataset, ResidentLoader
        if resident:
            Loader = ResidentLoader
    if args.dataset not in ("cifar10", "cifar100", "imagenet"):
        raise ValueError(args.dataset)
    if packed_dir:
        train_ds, test_ds = (PackedDataset(os.path.join(packed_dir, split + EXTENSION)) for split in ("train", "val"))
    elif args.dataset == "imagenet":
        if resident:
            raise ValueError("--resident 1 keeps decoded pixels on the device and image folders are not decoded: pack first "
                             "(python -m uvc_amd.packed pack --dataset imagenet --data_dir D --split train|val --output P/train|val.uvcpack) "
                             "and pass --packed_dir P")
        train_ds, test_ds = ImageFolder(os.path.join(args.data_dir, "train")), ImageFolder(os.path.join(args.data_dir, "val"))
    else:
        train_ds, test_ds = read_cifar(args.data_dir, args.dataset, True), read_cifar(args.data_dir, args.dataset, False)
    if args.dataset in ("cifar10", "cifar100"):
        args.data_classes = 10 if args.dataset == "cifar10" else 100
        args.num_classes = 16 if args.dataset == "cifar10" else 104
        kw = dict(mean=CIFAR_MEAN, std=CIFAR_STD, num_workers=nw, interpolation=interpolation)
        train = Loader(train_ds, args.train_batch_size, S, train=True, scale=(0.05, 1.0), flip=False, seed=seed, rank=rank,
                       world=world, **kw) if "train" in splits else None
        test = Loader(test_ds, args.eval_batch_size, S, train=False, eval="square", **kw) if "test" in splits else None
    else:
        n_classes = len(train_ds.classes) if train_ds.classes is not None else train_ds.num_classes()
        if n_classes > args.num_classes:
            where = f"classes in {os.path.join(packed_dir, 'train' + EXTENSION)}" if packed_dir else f"class folders under {args.data_dir}/train"
            raise ValueError(f"{n_classes} {where} but --num_classes {args.num_classes}")
        args.data_classes = args.num_classes
        kw = dict(mean=IMAGENET_MEAN, std=IMAGENET_STD, num_workers=nw, interpolation=interpolation, crop_pct=crop_pct)
        train = Loader(train_ds, args.train_batch_size, S, train=True, seed=seed, rank=rank, world=world, **kw) if "train" in splits else None
        test = Loader(test_ds, args.eval_batch_size, S, train=False, eval="center", **kw) if "test" in splits else None
    return train, test


def build_eval_loader(args, split, dataset=None):
    """(loader, data_classes): ONE split of --dataset ("train" or "test") under the EVAL transform, every sample in dataset order and the
    short last batch included -- what feature extraction reads (python -m uvc_amd.compact_transfer); build_loaders gives the train split
    with augmentation only.  Reads build_loaders' attributes (dataset, data_dir, img_size, eval_batch_size, num_workers, packed_dir,
    resident, interpolation, crop_pct); CIFAR: the square resize with 0.5 / 0.5, ImageNet: resize + centre crop with its mean / std.
    ``dataset``: a ready dataset (``load(i)`` / ``targets``) in place of the files, labelled by args.dataset's transform."""
    if split not in ("train", "test"):
        raise ValueError(f"split must be 'train' or 'test', not {split!r}")
    if args.dataset not in ("cifar10", "cifar100", "imagenet"):
        raise ValueError(args.dataset)
    S = args.img_size
    packed_dir = getattr(args, "packed_dir", None)
    resident = bool(int(getattr(args, "resident", 0) or 0))
    interpolation = getattr(args, "interpolation", None) or "bilinear"
    crop_pct = getattr(args, "crop_pct", None)
    _pil_filter(interpolation)
    eval_resize_side(S, crop_pct)
    Loader = DeviceLoader
    if resident:
        from .packed import ResidentLoader as Loader
    cifar = args.dataset in ("cifar10", "cifar100")
    if dataset is not None:
        ds = dataset
    elif packed_dir:
        from .packed import EXTENSION, PackedDataset
        ds = PackedDataset(os.path.join(packed_dir, ("train" if split == "train" else "val") + EXTENSION))
    elif cifar:
        ds = read_cifar(args.data_dir, args.dataset, split == "train")
    else:
        if resident:
            raise ValueError("--resident 1 keeps decoded pixels on the device and image folders are not decoded: pack first and pass --packed_dir")
        ds = ImageFolder(os.path.join(args.data_dir, "train" if split == "train" else "val"))
    if cifar:
        classes = 10 if args.dataset == "cifar10" else 100
        kw = dict(mean=CIFAR_MEAN, std=CIFAR_STD, eval="square")
    else:
        names = getattr(ds, "classes", None)
        classes = len(names) if names is not None else (ds.num_classes() if hasattr(ds, "num_classes") else int(max(ds.targets)) + 1)
        kw = dict(mean=IMAGENET_MEAN, std=IMAGENET_STD, eval="center", crop_pct=crop_pct)
    loader = Loader(ds, args.eval_batch_size, S, train=False, num_workers=getattr(args, "num_workers", 4), interpolation=interpolation, **kw)
    return loader, classes


def add_image_args(p):
    """--interpolation / --crop_pct on a driver's parser (build_loaders reads them)."""
    p.add_argument("--interpolation", choices=list(INTERPOLATIONS), default="bilinear",
                   help="resampling filter of the training crops and the eval resize: bilinear is the reference's (torchvision's default); "
                        "the released DeiT and T2T-ViT checkpoints were trained and evaluated with bicubic")
    p.add_argument("--crop_pct", type=float, default=None,
                   help="ImageNet eval: resize the short side to floor(img_size / crop_pct) before the centre crop (timm's rule; 0.875 -> 256 and "
                        "0.9 -> 248 at 224, T2T-ViT uses 0.9); default: img_size * 256 // 224")


def real_mixup(args):
    """The reference's Mixup / CutMix (or None) over the dataset's classes (args.data_classes, set by build_loaders)."""
    import argparse
    from .mixup import build_mixup
    return build_mixup(argparse.Namespace(**{**vars(args), "num_classes": args.data_classes}))


def soft_batches(loader, epoch, mixup_fn, smoothing, num_classes, head_classes=None):
    """The reference's loop head (joint_train.py:399-409, post_train.py:348-362) over real batches: set_epoch, odd batches lose their
    last sample, then Mixup / CutMix, or smoothed one-hot targets without it, over the ``num_classes`` data classes (mixup_fn must be
    built for that count); columns up to ``head_classes`` (a padded head) are zero.  Yields (x, y_soft)."""
    head_classes = num_classes if head_classes is None else head_classes
    loader.set_epoch(epoch)
    for x, t in loader:
        if len(x) % 2 != 0:
            x, t = x[:-1], t[:-1]
        if len(x) == 0:
            continue
        if mixup_fn is not None:
            x, y = mixup_fn(x.contiguous(), t)
        else:
            off = smoothing / num_classes
            y = torch.full((len(x), num_classes), off, device=x.device).scatter_(1, t.view(-1, 1), 1.0 - smoothing + off)
        if head_classes > num_classes:
            y = torch.nn.functional.pad(y, (0, head_classes - num_classes))
        yield x, y
