"""GPU: uvc_image_prep_patches (include/uvc_data.h) -- the resampler's last pass writing the patch rows uvc_patchify would make of
uvc_image_prep's batch.  Bit for bit against that pair over patch geometries, element types, filters, flips and batch sizes on a ragged
batch that upscales, downscales and passes through; every element overwritten; the refusals; skipped descriptors; the loaders."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from uvc_amd import _lib as L
from uvc_amd import data as D
from uvc_amd import ops

pytestmark = pytest.mark.gpu

MEAN, STD = D.IMAGENET_MEAN, D.IMAGENET_STD
FILTERS = {"bilinear": L.UVC_IMAGE_FILTER_BILINEAR, "bicubic": L.UVC_IMAGE_FILTER_BICUBIC}
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
BF16_SENTINEL = -1                                               # 0xFFFF: a NaN no cast of a finite float32 produces


def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def sources(S):
    """(uint8 HWC array, (resize_h, resize_w), (win_y, win_x)): a 1 x 1 image, a small portrait upscaled, a landscape through the eval
    transform (downscaled at 224 with a centre window), a portrait resized to the square, and an image that is S x S already."""
    side = D.eval_resize_side(S)
    rs = D.resize_short_side(200, 300, side)
    return [(noise(1, 1, 1), (S, S), (0, 0)),
            (noise(53, 37, 2), (S, S), (0, 0)),
            (noise(200, 300, 3), rs, D.center_crop_offset(*rs, S)),
            (noise(300, 200, 4), (S, S), (0, 0)),
            (noise(S, S, 5), (S, S), (0, 0))]


def descriptors(items, flip):
    offs = np.concatenate([[0], np.cumsum([a.size for a, *_ in items])]).astype(np.int64)
    desc = np.zeros(len(items), ops.image_desc_dtype())
    for b, (a, (rh, rw), (wy, wx)) in enumerate(items):
        desc[b] = (offs[b], a.shape[0], a.shape[1], rh, rw, wy, wx, int(flip), 0, 0, 0, 0, 0, 0)
    return desc, torch.from_numpy(np.concatenate([a.reshape(-1) for a, *_ in items])).cuda()


def dev(desc):
    return torch.from_numpy(desc.view(np.uint8).copy()).cuda()


def sentinel_rows(B, S, P, dtype):
    out = torch.empty(B * (S // P) ** 2, 3 * P * P, dtype=dtype, device="cuda")
    if dtype == torch.float32:
        out.fill_(float("nan"))
    else:
        out.view(torch.int16).fill_(BF16_SENTINEL)
    return out


def untouched(rows):
    return torch.isnan(rows) if rows.dtype == torch.float32 else rows.view(torch.int16) == BF16_SENTINEL


@functools.lru_cache(maxsize=None)
def image_batch(S, filt, flip, B):
    """uvc_image_prep's float32 batch of the first B sources (B = 1: the upscaled portrait), computed once and left unchanged."""
    items = sources(S)[1:2] if B == 1 else sources(S)[:B]
    desc, src = descriptors(items, flip)
    ws = torch.empty(max(ops.image_prep_workspace(desc, S, src.numel(), FILTERS[filt]), 16), dtype=torch.uint8, device="cuda")
    x = torch.full((len(items), 3, S, S), float("nan"), device="cuda")
    ops.image_prep(src, dev(desc), ws, x, MEAN, STD, filter=FILTERS[filt])
    assert not torch.isnan(x).any()
    return items, x


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("filt", sorted(FILTERS))
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("S,P", [(32, 16), (64, 16), (48, 8), (224, 16)])
def test_patch_rows_equal_patchify_of_the_image_batch(S, P, dtype, filt, flip):
    td = DTYPES[dtype]
    for B in (1, 5):
        items, x = image_batch(S, filt, flip, B)
        want = torch.empty(B * (S // P) ** 2, 3 * P * P, dtype=td, device="cuda")
        ops.patchify(x, want, P, ops.UVC_F32 if td == torch.float32 else ops.UVC_BF16)
        desc, src = descriptors(items, flip)
        nbytes = ops.image_prep_patches_workspace(desc, S, src.numel(), FILTERS[filt])
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
        got = sentinel_rows(B, S, P, td)
        ops.image_prep_patches(src, dev(desc), ws, got, P, S, MEAN, STD, filter=FILTERS[filt])
        torch.cuda.synchronize()
        assert not untouched(got).any(), (B, int(untouched(got).sum()))          # every element overwritten
        assert torch.equal(got, want), B
        assert torch.equal(got.view(torch.int16 if td == torch.bfloat16 else torch.int32), want.view(torch.int16 if td == torch.bfloat16 else torch.int32))


def test_a_patch_size_off_the_vector_width_takes_the_one_column_path():
    """P = 6 (uvc_patchify wants P % 4 == 0, so the rows are checked against the index rule itself)."""
    S, P, filt = 48, 6, "bicubic"
    items, x = image_batch(S, filt, 1, 5)
    G = S // P
    want = x.reshape(5, 3, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(5 * G * G, 3 * P * P)
    desc, src = descriptors(items, 1)
    ws = torch.empty(ops.image_prep_patches_workspace(desc, S, src.numel(), FILTERS[filt]), dtype=torch.uint8, device="cuda")
    for td in (torch.float32, torch.bfloat16):
        got = sentinel_rows(5, S, P, td)
        ops.image_prep_patches(src, dev(desc), ws, got, P, S, MEAN, STD, filter=FILTERS[filt])
        assert torch.equal(got, want.to(td))


def test_refusals():
    S, P = 32, 16
    items = sources(S)
    desc, src = descriptors(items, 0)
    ws = torch.empty(ops.image_prep_workspace(desc, S, src.numel(), 0), dtype=torch.uint8, device="cuda")
    got = sentinel_rows(5, S, P, torch.float32)
    dd = dev(desc)
    for bad in (12, 0, -16, 64):                                  # S % P != 0, P = 0, P < 0, P > S
        with pytest.raises(L.UvcHipError, match=r"rc=1"):
            ops.image_prep_patches(src, dd, ws, got, bad, S, MEAN, STD)
    a = L.uvc_image_prep_args()
    a.src, a.src_bytes, a.desc, a.workspace, a.workspace_bytes, a.out = L.ptr(src), src.numel(), L.ptr(dd), L.ptr(ws), ws.numel(), L.ptr(got)
    a.mean[:], a.std[:] = MEAN, STD
    a.B, a.S = 5, S
    for dtype in (2, -1, 7):                                      # neither UVC_F32 nor UVC_BF16
        assert L.lib().uvc_image_prep_patches(C.byref(a), P, dtype, L.cur_stream()) == 1
    assert L.lib().uvc_image_prep_patches(C.byref(a), 12, ops.UVC_F32, L.cur_stream()) == 1
    assert L.lib().uvc_image_prep_patches(C.byref(a), 0, ops.UVC_BF16, L.cur_stream()) == 1
    a.filter = 2
    assert L.lib().uvc_image_prep_patches(C.byref(a), P, ops.UVC_F32, L.cur_stream()) == 1
    torch.cuda.synchronize()
    assert untouched(got).all()                                   # refused on the host: nothing was launched
    with pytest.raises(L.UvcHipError):
        ops.image_prep_patches(src, dd, ws, got.half(), P, S, MEAN, STD)
    a.filter = 0
    assert L.lib().uvc_image_prep_patches(C.byref(a), P, ops.UVC_F32, L.cur_stream()) == 0


@pytest.mark.parametrize("launched", ["bicubic", "bilinear"])
def test_descriptors_of_the_other_filter_leave_their_rows_untouched(launched):
    S, P, B = 32, 16, 5
    other = "bilinear" if launched == "bicubic" else "bicubic"
    items, x = image_batch(S, launched, 0, B)
    desc, src = descriptors(items, 0)
    foreign = desc.copy()
    nbytes = ops.image_prep_patches_workspace(desc, S, src.numel(), FILTERS[launched])
    ops.image_prep_patches_workspace(foreign, S, src.numel(), FILTERS[other])
    mixed = desc.copy()
    mixed[[1, 3]] = foreign[[1, 3]]
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    npatch = (S // P) ** 2
    for td in (torch.bfloat16, torch.float32):
        want = torch.empty(B * npatch, 3 * P * P, dtype=td, device="cuda")
        ops.patchify(x, want, P, ops.UVC_F32 if td == torch.float32 else ops.UVC_BF16)
        got = sentinel_rows(B, S, P, td)
        ops.image_prep_patches(src, dev(mixed), ws, got, P, S, MEAN, STD, filter=FILTERS[launched])
        for b in range(B):
            rows = slice(b * npatch, (b + 1) * npatch)
            if b in (1, 3):
                assert untouched(got[rows]).all(), b
            else:
                assert torch.equal(got[rows], want[rows]), b


class _Ragged:
    def __init__(self):
        rng = np.random.default_rng(21)
        self.images = [rng.integers(0, 256, (int(rng.integers(20, 61)), int(rng.integers(20, 61)), 3), dtype=np.uint8) for _ in range(7)]
        self.targets = np.arange(7, dtype=np.int64)

    def __len__(self):
        return 7

    def load(self, i):
        return self.images[i]


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_loader_outputs(train):
    """output="image" is the loader built without the keyword, bit for bit (a ragged dataset and an in-memory array); output="patches"
    is patchify of those batches."""
    S, P, bs = 32, 16, 3
    arr = D.ArrayDataset(np.random.default_rng(5).integers(0, 256, (7, 24, 40, 3), dtype=np.uint8), np.arange(7))
    for ds in (_Ragged(), arr):
        kw = dict(train=train, seed=4, num_workers=2, interpolation="bicubic")
        plain = [(x.clone(), t.clone()) for x, t in D.DeviceLoader(ds, bs, S, **kw)]
        image = [(x.clone(), t.clone()) for x, t in D.DeviceLoader(ds, bs, S, output="image", **kw)]
        assert [len(x) for x, _ in plain] == [3, 3, 1] == [len(x) for x, _ in image]
        for (xp, tp), (xi, ti) in zip(plain, image):
            assert xi.dtype == torch.float32 and torch.equal(xp.view(torch.int32), xi.view(torch.int32)) and torch.equal(tp, ti)
        for td in (torch.bfloat16, torch.float32):
            rows = list(D.DeviceLoader(ds, bs, S, output="patches", patch_size=P, dtype=td, **kw))
            assert len(rows) == 3
            for (xp, tp), (r, tr) in zip(plain, rows):
                want = torch.empty(len(xp) * (S // P) ** 2, 3 * P * P, dtype=td, device="cuda")
                ops.patchify(xp, want, P, ops.UVC_F32 if td == torch.float32 else ops.UVC_BF16)
                assert r.dtype == td and torch.equal(r, want) and torch.equal(tr, tp)
    for bad in (dict(output="rows"), dict(output="patches"), dict(output="patches", patch_size=12, dtype=torch.float32),
                dict(output="patches", patch_size=16, dtype=torch.float16), dict(patch_size=16)):
        with pytest.raises(ValueError):
            D.DeviceLoader(arr, bs, S, **bad)
