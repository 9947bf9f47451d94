"""Packed datasets: decode once, store the pixels in one file, keep them in device memory and crop them there.

    write_pack(dataset, path, max_side=0)   stream any dataset with .load(i) / .targets into one ``.uvcpack`` file
    PackedDataset(path)                     the file as a dataset: load(i) is a zero-copy view into an np.memmap
    ResidentLoader(dataset, ...)            DeviceLoader's protocol and batches with the pixels uploaded once: per batch the host
                                            computes crop windows only and uvc_image_prep_crops (include/uvc_data.h) reads them in place

    python -m uvc_amd.packed pack --dataset imagenet|cifar10|cifar100 --data_dir D --split train|val --output F [--max_side M]
    python -m uvc_amd.packed info F

The file (all integers little-endian, all positions 64-bit):
    bytes 0..7    magic  b"UVCPACK\\0"
    bytes 8..11   version (uint32) = 1
    bytes 12..15  length of the JSON header (uint32)
    bytes 16..    JSON: n, classes (list of names or null), max_side, source, file_bytes and the byte position and size of each array
    offsets       int64[n + 1]: byte offsets into the pixel blob (offsets[i + 1] - offsets[i] = h * w * 3)
    hw            int32[n, 2]
    labels        int64[n]
    pixels        every image HWC uint8, rows of w * 3 bytes, back to back; starts on a 4096-byte boundary
Nothing in it is executable or pickled.

``max_side = m > 0`` stores an image whose short side exceeds m as ``Image.resize(resize_short_side(h, w, m), BILINEAR)``: training then
draws its crops from a downscaled image, a deviation from the reference whose effect on accuracy is unmeasured.  Pack validation
splits with ``max_side 0``: Resize(256) of a smaller stored image would upsample.  That downscale is bilinear whatever ``interpolation``
the loaders later resample with: the file records no filter.
"""
from __future__ import annotations

import collections
import json
import os
import struct
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .data import MAX_THREADS, RRC_DRAWS, ArrayDataset, DeviceLoader, resize_short_side, sample_uniforms

MAGIC = b"UVCPACK\0"
VERSION = 1
EXTENSION = ".uvcpack"
BLOB_ALIGN = 4096
_ARRAYS = ("offsets", "hw", "labels", "pixels")


def _align(v, a):
    return (v + a - 1) // a * a


# ---------------------------------------------------------------------------------------------------------------- the file

class PackWriter:
    """Writes one pack: ``append`` every image in order (or ``skip`` its bytes, which leaves a hole in a sparse file), then ``close``.
    The arrays in front of the blob are written on close, when every size is known."""

    def __init__(self, path, labels, classes=None, max_side=0, source=""):
        self.labels = np.ascontiguousarray(labels, dtype=np.int64).reshape(-1)
        n = self.n = len(self.labels)
        self.meta = dict(n=n, classes=None if classes is None else [str(c) for c in classes], max_side=int(max_side), source=str(source))
        probe = json.dumps(self._header(dict.fromkeys(_ARRAYS, (0, 0)), 0))
        self.header_bytes = _align(16 + len(probe) + 256, 64)                 # room for the digits of the real positions
        self.pos = {}
        p = self.header_bytes
        for name, size in (("offsets", 8 * (n + 1)), ("hw", 8 * n), ("labels", 8 * n)):
            self.pos[name] = (p, size)
            p = _align(p + size, 64)
        self.blob_pos = _align(p, BLOB_ALIGN)
        self.offsets = np.zeros(n + 1, dtype=np.int64)
        self.hw = np.zeros((n, 2), dtype=np.int32)
        self.k = 0
        self.f = open(path, "wb")
        self.f.seek(self.blob_pos)

    def _header(self, pos, file_bytes):
        return dict(self.meta, file_bytes=int(file_bytes), arrays={k: dict(pos=int(p), bytes=int(b)) for k, (p, b) in pos.items()})

    def _next(self, h, w):
        if self.k >= self.n:
            raise ValueError("more images than labels")
        if h < 1 or w < 1:
            raise ValueError(f"image {self.k} is empty")
        self.hw[self.k] = h, w
        self.offsets[self.k + 1] = self.offsets[self.k] + int(h) * int(w) * 3
        self.k += 1

    def append(self, a):
        a = np.ascontiguousarray(a)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("images are uint8 [H, W, 3]")
        self._next(a.shape[0], a.shape[1])
        self.f.write(memoryview(a).cast("B"))

    def skip(self, h, w):
        self._next(h, w)
        self.f.seek(self.blob_pos + int(self.offsets[self.k]))

    def abort(self):
        """Closes the file and removes it: a pack that was not finished has no header."""
        path = self.f.name
        self.f.close()
        if os.path.exists(path):
            os.remove(path)

    def close(self):
        if self.k != self.n:
            self.f.close()
            raise ValueError(f"{self.k} images written for {self.n} labels")
        f = self.f
        blob = int(self.offsets[-1])
        f.truncate(self.blob_pos + blob)
        self.pos["pixels"] = (self.blob_pos, blob)
        head = json.dumps(self._header(self.pos, self.blob_pos + blob)).encode()
        if 16 + len(head) > self.header_bytes:
            raise ValueError("pack header outgrew its reserved room")
        f.seek(0)
        f.write(MAGIC + struct.pack("<II", VERSION, len(head)) + head)
        for name, arr in (("offsets", self.offsets), ("hw", self.hw), ("labels", self.labels)):
            f.seek(self.pos[name][0])
            f.write(arr.tobytes())
        f.close()


def write_pack(dataset, path, max_side=0, num_workers=8):
    """Streams ``dataset`` (``.load(i)`` -> uint8 [H, W, 3], ``.targets``; ``.classes`` optional) into the pack ``path``.  Decodes on
    min(num_workers, 16) threads, at most 4 x threads images decoded or in flight at a time; a failure removes the partial file.
    ``max_side = m > 0``: an image whose short side exceeds m is stored as PIL's Image.resize(BILINEAR) to resize_short_side(h, w, m);
    the header records m.  Returns the header dict."""
    max_side = int(max_side)
    if max_side < 0:
        raise ValueError("max_side >= 0")
    threads = max(1, min(int(num_workers), MAX_THREADS))

    def load(i):
        a = np.asarray(dataset.load(i))
        h, w = a.shape[:2]
        if max_side > 0 and min(h, w) > max_side:
            from PIL import Image
            nh, nw = resize_short_side(h, w, max_side)
            a = np.asarray(Image.fromarray(np.ascontiguousarray(a)).resize((nw, nh), Image.BILINEAR))
        return a

    n = len(dataset.targets)
    source = getattr(dataset, "root", None) or type(dataset).__name__
    wr = PackWriter(path, dataset.targets, getattr(dataset, "classes", None), max_side, source)
    window = 4 * threads
    try:
        with ThreadPoolExecutor(threads) as pool:
            pending = collections.deque()                        # in order; a new decode starts as soon as the oldest is written
            for i in range(n):
                if len(pending) == window:
                    wr.append(pending.popleft().result())
                pending.append(pool.submit(load, i))
            while pending:
                wr.append(pending.popleft().result())
        wr.close()
    except BaseException:
        wr.abort()                                               # no partial file stays behind
        raise
    return read_header(path)[0]


def read_header(path):
    """(header dict, file size) of a pack; ValueError names what is wrong with the file."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(16)
        if len(head) < 16 or head[:8] != MAGIC:
            raise ValueError(f"{path}: not a {EXTENSION} file (wrong magic number)")
        version, hlen = struct.unpack("<II", head[8:16])
        if version != VERSION:
            raise ValueError(f"{path}: pack version {version}, this reader understands version {VERSION}")
        raw = f.read(hlen)
    if len(raw) < hlen:
        raise ValueError(f"{path}: file is shorter than its header says ({size} bytes, header of {hlen})")
    try:
        h = json.loads(raw.decode())
        n = int(h["n"])
        arrays = {k: (int(h["arrays"][k]["pos"]), int(h["arrays"][k]["bytes"])) for k in _ARRAYS}
    except (ValueError, KeyError, TypeError) as e:
        raise ValueError(f"{path}: unreadable pack header ({e})") from None
    want = dict(offsets=8 * (n + 1), hw=8 * n, labels=8 * n)
    for k, (pos, nbytes) in arrays.items():
        if n < 0 or pos < 16 + hlen or nbytes < 0 or (k in want and nbytes != want[k]):
            raise ValueError(f"{path}: header places array {k!r} inconsistently ({pos}, {nbytes} bytes for n = {n})")
        if pos + nbytes > size:
            raise ValueError(f"{path}: file is shorter than its header says ({size} bytes, array {k!r} ends at {pos + nbytes})")
    if arrays["pixels"][0] % BLOB_ALIGN:
        raise ValueError(f"{path}: the pixel blob does not start on a {BLOB_ALIGN}-byte boundary")
    return h, size


class PackedDataset:
    """A pack as a dataset: ``load(i)`` is a zero-copy [h, w, 3] view into the memory-mapped pixel blob."""

    def __init__(self, path):
        h, _ = read_header(path)
        self.path, self.header = path, h
        n = int(h["n"])
        pos = {k: int(h["arrays"][k]["pos"]) for k in _ARRAYS}
        with open(path, "rb") as f:
            def arr(name, dtype, count):
                f.seek(pos[name])
                return np.frombuffer(f.read(count * np.dtype(dtype).itemsize), dtype=dtype).copy()
            self.offsets = arr("offsets", np.int64, n + 1)
            self.hw = arr("hw", np.int32, 2 * n).reshape(n, 2)
            self.targets = arr("labels", np.int64, n)
        self.pixel_bytes = int(h["arrays"]["pixels"]["bytes"])
        sizes = self.hw[:, 0].astype(np.int64) * self.hw[:, 1].astype(np.int64) * 3
        if n and (self.hw.min() < 1 or self.offsets[0] != 0 or not np.array_equal(np.diff(self.offsets), sizes)):
            raise ValueError(f"{path}: offsets are not non-decreasing and consistent with the image sizes")
        if int(self.offsets[-1]) != self.pixel_bytes:
            raise ValueError(f"{path}: offsets end at {int(self.offsets[-1])} but the pixel blob has {self.pixel_bytes} bytes")
        self.classes = h.get("classes")
        self.max_side = int(h.get("max_side", 0))
        self.pixels = np.memmap(path, dtype=np.uint8, mode="r", offset=pos["pixels"], shape=(self.pixel_bytes,)) if self.pixel_bytes else \
            np.zeros(0, np.uint8)

    def __len__(self):
        return len(self.targets)

    def load(self, i):
        h, w = self.hw[i]
        return self.pixels[self.offsets[i]:self.offsets[i + 1]].reshape(int(h), int(w), 3)

    def num_classes(self):
        return len(self.classes) if self.classes is not None else (int(self.targets.max()) + 1 if len(self.targets) else 0)

    def info(self):
        sides = self.hw if len(self.hw) else np.zeros((1, 2), np.int32)
        return dict(n=len(self), classes=self.num_classes(), pixel_bytes=self.pixel_bytes, max_side=self.max_side,
                    smallest_side=int(sides.min()), largest_side=int(sides.max()))


# ---------------------------------------------------------------------------------------------------------------- resident loader

def _store_of(dataset):
    """(flat uint8 pixel array, int64 offsets [n], int64 hw [n, 2]) of a dataset whose pixels lie back to back in memory."""
    if isinstance(dataset, PackedDataset):
        return dataset.pixels, dataset.offsets[:-1].astype(np.int64), dataset.hw.astype(np.int64)
    if isinstance(dataset, ArrayDataset):
        n, h, w, _ = dataset.images.shape
        hw = np.empty((n, 2), dtype=np.int64)
        hw[:, 0], hw[:, 1] = h, w
        return dataset.images.reshape(-1), np.arange(n, dtype=np.int64) * (h * w * 3), hw
    raise ValueError("ResidentLoader wants a PackedDataset or an ArrayDataset: pack the dataset first (python -m uvc_amd.packed pack)")


class _GeoSlot:
    """Pinned staging of one batch's descriptors and dataset indices; reused only after the kernels that read its upload have finished (``done``)."""

    def __init__(self):
        self.buf = None
        self.done = None
        self.n = 0
        self.ws_bytes = 0


class ResidentLoader(DeviceLoader):
    """DeviceLoader's protocol and, bit for bit, its batches, with the dataset's pixels and labels uploaded to the device once.

    Per batch the producer thread computes the geometry only (the crop window, through DeviceLoader._geometry) and completes the crop
    descriptors on the host; one small upload carries the descriptors (80 B per image) and the batch's dataset indices; the labels
    are an index_select on the device and uvc_image_prep_crops reads the crop windows inside the stored images.  No pixel crosses
    the host after construction.  In data-parallel runs every rank holds the whole store."""

    STAGE_BYTES = 32 << 20

    def __init__(self, dataset, batch_size, img_size, *args, **kw):
        from . import ops
        super().__init__(dataset, batch_size, img_size, *args, **kw)
        if self.output != "image":
            raise NotImplementedError("ResidentLoader yields image batches only (output='patches' is DeviceLoader's)")
        if self._pool is not None:                               # nothing is decoded or sliced here: no worker threads
            self._pool.shutdown()
            self._pool = None
        self._dsize = ops.image_crop_desc_dtype().itemsize
        pixels, self._offsets, self._hw = _store_of(dataset)
        self.store_bytes = int(pixels.shape[0])
        need = self.store_bytes + 8 * len(dataset.targets)
        free, _ = torch.cuda.mem_get_info(self.device)
        if need > free:
            raise ValueError(f"the resident store needs {need} bytes on the device and {free} are free: "
                             f"run with --resident 0 (or pack with a smaller --max_side)")
        self._labels = torch.from_numpy(np.ascontiguousarray(dataset.targets, dtype=np.int64)).to(self.device)
        self._store = torch.empty(max(self.store_bytes, 1), dtype=torch.uint8, device=self.device)
        self._upload_store(pixels)

    def _upload_store(self, pixels):
        """The blob through two bounded pinned staging buffers, in chunks: the file is never pinned whole."""
        chunk = min(self.STAGE_BYTES, max(self.store_bytes, 1))
        stage = [torch.empty(chunk, dtype=torch.uint8).pin_memory() for _ in range(2)]
        events = [None, None]
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            for k, lo in enumerate(range(0, self.store_bytes, chunk)):
                n = min(chunk, self.store_bytes - lo)
                s = k % 2
                if events[s] is not None:
                    events[s].synchronize()                     # the copy that read this buffer last has finished
                np.copyto(stage[s].numpy()[:n], pixels[lo:lo + n])
                self._store[lo:lo + n].copy_(stage[s][:n], non_blocking=True)
                events[s] = torch.cuda.Event()
                events[s].record(stream)
            stream.synchronize()

    def _fill(self, slot, idx):
        """One batch into a pinned slot: the crop descriptors, completed by the host query, then the dataset indices."""
        from . import ops
        B = len(idx)
        ids = np.asarray(idx, dtype=np.int64)
        u = sample_uniforms(self.seed, self.epoch, ids, RRC_DRAWS) if self.train else None
        hw = self._hw[ids]
        g = self._geometry(hw, u)
        desc = np.zeros(B, dtype=ops.image_crop_desc_dtype())
        desc["src_offset"] = self._offsets[ids]
        desc["img_h"], desc["img_w"] = hw[:, 0], hw[:, 1]
        desc["crop_y"], desc["crop_x"], desc["crop_h"], desc["crop_w"] = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
        desc["resize_h"], desc["resize_w"], desc["win_y"], desc["win_x"], desc["flip"] = g[:, 4], g[:, 5], g[:, 6], g[:, 7], g[:, 8]
        slot.ws_bytes = ops.image_prep_crops_workspace(desc, self.S, self.store_bytes, self.filter)
        nd = desc.nbytes
        if slot.buf is None or slot.buf.numel() < nd + 8 * B:
            slot.buf = torch.empty(max(nd + 8 * B, 88 * 512), dtype=torch.uint8).pin_memory()
        host = slot.buf.numpy()
        host[:nd] = desc.view(np.uint8)
        host[nd:nd + 8 * B] = ids.view(np.uint8)
        slot.n = B

    # -- device side (DeviceLoader.__iter__ keeps the slots, the producer thread and the stream and allocator discipline)
    def _new_slot(self):
        return _GeoSlot()

    def _new_copy_stream(self):
        # A high-priority stream.  HIP maps the streams of one priority onto a few hardware queues in the order of their first use, so a
        # normal-priority copy stream can come to share a queue with a trainer's side stream (wgrads, teacher forward); the 45 KB upload
        # then waits behind that stream's kernels and the consumer's stream behind the upload: +0.2 to +2 ms per DeiT-Tiny step, for
        # whichever loader's stream the history of the process put there (DESIGN "Packed, resident datasets").  The queues of another
        # priority are a pool of their own, which no side stream of the trainers uses.
        return torch.cuda.Stream(self.device, priority=-1)

    def _upload(self, slot):
        nbytes = slot.n * (self._dsize + 8)
        geo = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        geo.copy_(slot.buf[:nbytes], non_blocking=True)
        return (geo,)

    def _launch(self, slot, up, ws, x):
        from . import ops
        nd = slot.n * self._dsize
        target = self._labels.index_select(0, up[0][nd:].view(torch.int64))
        ops.image_prep_crops(self._store, up[0][:nd], ws, x, self.mean, self.std, self.filter)
        return target


# ---------------------------------------------------------------------------------------------------------------- command line

def main(argv=None):
    import argparse
    p = argparse.ArgumentParser(prog="python -m uvc_amd.packed", description="Pack a dataset into one .uvcpack file, or describe one")
    sub = p.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("pack")
    k.add_argument("--dataset", choices=["imagenet", "cifar10", "cifar100"], required=True)
    k.add_argument("--data_dir", required=True)
    k.add_argument("--split", choices=["train", "val"], required=True)
    k.add_argument("--output", required=True)
    k.add_argument("--max_side", type=int, default=0, help="store images whose short side exceeds this at this short side (0: unchanged); "
                   "a deviation from the reference whose effect on accuracy is unmeasured; keep 0 for validation splits")
    k.add_argument("--num_workers", type=int, default=8, help="decode threads (at most 16)")
    sub.add_parser("info").add_argument("file")
    args = p.parse_args(argv)
    if args.cmd == "pack":
        from .data import ImageFolder, read_cifar
        if args.dataset == "imagenet":
            ds = ImageFolder(os.path.join(args.data_dir, args.split))
        else:
            ds = read_cifar(args.data_dir, args.dataset, args.split == "train")
        write_pack(ds, args.output, max_side=args.max_side, num_workers=args.num_workers)
        path = args.output
    else:
        path = args.file
    info = PackedDataset(path).info()
    print(json.dumps(info))
    return info


if __name__ == "__main__":
    main()
