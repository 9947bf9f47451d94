"""GPU: uvc_image_prep_crops (include/uvc_data.h) reads crop windows inside the images of a resident store.  Its output must be,
bit for bit, uvc_image_prep's on the same crops copied out contiguously (and, on sampled cases, PIL's crop().resize()), for uint8 and
float32 outputs, for stores past 2^32 bytes, and a descriptor that does not fit the store it is launched with must be skipped."""
import numpy as np
import pytest
import torch
from PIL import Image

from uvc_amd import _lib
from uvc_amd import data as D
from uvc_amd import ops

pytestmark = pytest.mark.gpu

MEAN, STD = D.IMAGENET_MEAN, D.IMAGENET_STD
SIZES = [(32, 32), (37, 53), (240, 5), (8, 8), (1, 1), (64, 48)]             # stored h x w


def make_store(sizes, seed=0):
    rng = np.random.default_rng(seed)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    offs = np.concatenate([[0], np.cumsum([a.size for a in imgs])]).astype(np.int64)
    return imgs, offs, np.concatenate([a.reshape(-1) for a in imgs])


@pytest.fixture(scope="module")
def store():
    imgs, offs, flat = make_store(SIZES)
    return imgs, offs, torch.from_numpy(flat).cuda()


def crop_desc(cases, offs, sizes):
    """cases: (image, (crop_y, crop_x, crop_h, crop_w), (resize_h, resize_w), (win_y, win_x), flip)."""
    desc = np.zeros(len(cases), ops.image_crop_desc_dtype())
    for b, (k, (cy, cx, ch, cw), (rh, rw), (wy, wx), fl) in enumerate(cases):
        desc[b] = (offs[k], sizes[k][0], sizes[k][1], cy, cx, ch, cw, rh, rw, wy, wx, int(fl), 0, 0, 0, 0, 0, 0)
    return desc


def run_crops(store_dev, desc, S, u8=True, mean=MEAN, std=STD, check_bytes=None):
    B = len(desc)
    ws_bytes = ops.image_prep_crops_workspace(desc, S, store_dev.numel() if check_bytes is None else check_bytes)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device="cuda")
    out = torch.empty(B, 3, S, S, dtype=torch.uint8 if u8 else torch.float32, device="cuda")
    out.fill_(77 if u8 else float("nan"))
    ops.image_prep_crops(store_dev, torch.from_numpy(desc.view(np.uint8).copy()).cuda(), ws, out, mean, std)
    torch.cuda.synchronize()
    return out.cpu()


def run_copied(imgs, cases, S, u8=True, mean=MEAN, std=STD):
    """The same cases through uvc_image_prep on the crops copied out contiguously."""
    crops = [np.ascontiguousarray(imgs[k][cy:cy + ch, cx:cx + cw]) for k, (cy, cx, ch, cw), *_ in cases]
    offs = np.concatenate([[0], np.cumsum([a.size for a in crops])]).astype(np.int64)
    desc = np.zeros(len(cases), ops.image_desc_dtype())
    for b, (a, (_, _, rs, win, fl)) in enumerate(zip(crops, cases)):
        desc[b] = (offs[b], a.shape[0], a.shape[1], rs[0], rs[1], win[0], win[1], int(fl), 0, 0, 0, 0, 0, 0)
    src = torch.from_numpy(np.concatenate([a.reshape(-1) for a in crops])).cuda()
    ws = torch.empty(max(ops.image_prep_workspace(desc, S, src.numel()), 16), dtype=torch.uint8, device="cuda")
    out = torch.empty(len(cases), 3, S, S, dtype=torch.uint8 if u8 else torch.float32, device="cuda")
    out.fill_(55 if u8 else float("nan"))
    ops.image_prep(src, torch.from_numpy(desc.view(np.uint8).copy()).cuda(), ws, out, mean, std)
    torch.cuda.synchronize()
    return out.cpu(), desc


def bits(t):
    return t if t.dtype == torch.uint8 else t.view(torch.int32)


S16 = ((16, 16), (0, 0))
CASES = (
    [(k, (0, 0, h, w), *S16, k % 2 == 1) for k, (h, w) in enumerate(SIZES)] +             # whole images (8 x 8 and 1 x 1 upscaled to 16)
    [(1, (5, 7, 20, 30), *S16, False), (1, (5, 7, 20, 30), *S16, True),                   # interior: row stride 53 * 3, crop width 30
     (5, (40, 30, 24, 18), *S16, False), (5, (40, 30, 24, 18), *S16, True),               # flush with the store's last byte
     (0, (31, 31, 1, 1), *S16, False), (1, (10, 12, 1, 1), *S16, True),                   # 1 x 1 crops
     (2, (20, 2, 210, 2), *S16, False), (2, (20, 2, 210, 2), *S16, True),                 # 210 > 100 * 2: vertical pass first
     (2, (0, 0, 240, 3), *S16, False),                                                      # 240 <= 100 * 3: horizontal first, tall
     (3, (2, 1, 5, 6), *S16, True),                                                         # inside the 8 x 8, upscaled
     (5, (3, 4, 60, 40), (24, 16), (4, 0), False), (5, (0, 0, 64, 48), (21, 16), (3, 0), True)])   # Resize + CenterCrop geometry


@pytest.mark.parametrize("u8", [True, False], ids=["uint8", "float32"])
def test_crops_equal_image_prep_on_copied_crops(store, u8):
    imgs, offs, dev = store
    desc = crop_desc(CASES, offs, SIZES)
    got = run_crops(dev, desc, 16, u8=u8)
    ref, rdesc = run_copied(imgs, CASES, 16, u8=u8)
    for b, c in enumerate(CASES):
        assert torch.equal(bits(got[b]), bits(ref[b])), c
    # the pass order is PIL's rule on the CROP's size: vertical first for the 210 x 2 crop only, although its image is 240 x 5
    assert desc["order"].tolist() == rdesc["order"].tolist()
    assert [c[1] == (20, 2, 210, 2) for c in CASES] == [bool(o) for o in desc["order"]]
    last = CASES[8]
    assert offs[5] + ((last[1][0] + last[1][2] - 1) * 48 + last[1][1] + last[1][3]) * 3 == dev.numel()   # it ends at the store's last byte


def test_one_image_twice_and_descriptors_not_sorted_by_offset(store):
    imgs, offs, dev = store
    cases = [CASES[8], CASES[6], CASES[0], CASES[7], CASES[6], CASES[12], CASES[1]]
    got = run_crops(dev, crop_desc(cases, offs, SIZES), 16, u8=False)
    ref, _ = run_copied(imgs, cases, 16, u8=False)
    assert torch.equal(bits(got), bits(ref))
    assert torch.equal(bits(got[1]), bits(got[4]))


def test_two_crops_of_a_photo_at_224():
    sizes = [(300, 400)]
    imgs, offs, flat = make_store(sizes, seed=1)
    cases = [(0, (10, 20, 250, 300), (224, 224), (0, 0), False), (0, (100, 150, 120, 97), (224, 224), (0, 0), True)]
    for u8 in (True, False):
        got = run_crops(torch.from_numpy(flat).cuda(), crop_desc(cases, offs, sizes), 224, u8=u8)
        ref, _ = run_copied(imgs, cases, 224, u8=u8)
        assert torch.equal(bits(got), bits(ref))


def test_against_pil_itself(store):
    """Not through uvc_image_prep: PIL's own crop().resize(), and the restated coefficients of tests/pil_bilinear.py."""
    import pil_bilinear as PB
    imgs, offs, dev = store
    cases = [CASES[1], CASES[6], CASES[7], CASES[12]]                        # a whole image, an interior window (flipped too), the tall crop
    got = run_crops(dev, crop_desc(cases, offs, SIZES), 16)
    for b, (k, (cy, cx, ch, cw), (rh, rw), (wy, wx), fl) in enumerate(cases):
        im = Image.fromarray(imgs[k]).crop((cx, cy, cx + cw, cy + ch)).resize((rw, rh), Image.BILINEAR).crop((wx, wy, wx + 16, wy + 16))
        if fl:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        assert torch.equal(got[b], torch.from_numpy(np.array(im, dtype=np.uint8)).permute(2, 0, 1)), cases[b]
    # the whole 37 x 53 image, row 3, through the restated fixed-point arithmetic
    a = imgs[1]
    hx, hn, hk = PB.coeffs(53, 0, 53, 16)
    vy, vn, vk = PB.coeffs(37, 0, 37, 16)
    rows = a[vy[3]:vy[3] + vn[3]].astype(np.float64)
    inter = np.stack([PB.clip8(np.int64(1 << 21) + (rows[:, hx[c]:hx[c] + hn[c]] * hk[c, :hn[c]][None, :, None]).sum(1).astype(np.int64))
                      for c in range(16)], 1).astype(np.float64)
    v = PB.clip8(np.int64(1 << 21) + (inter * vk[3, :vn[3]][:, None, None]).sum(0).astype(np.int64))
    assert np.array_equal(got[0, :, 3, :].numpy(), v[::-1].T)                # CASES[1] is flipped


def test_store_past_4_gib(store):
    """A 4.5 GB store with one 37 x 53 image just past 2^31 and one just past 2^32 and nothing else written: 64-bit addressing."""
    imgs, offs, dev = store
    n = int(4.5 * (1 << 30))
    big = torch.empty(n, dtype=torch.uint8, device="cuda")
    at = [(1 << 31) + 5, (1 << 32) + 11]
    img = torch.from_numpy(imgs[1].reshape(-1)).cuda()
    for o in at:
        big[o:o + img.numel()] = img
    windows = [(0, 0, 37, 53), (5, 7, 20, 30), (36, 52, 1, 1)]
    small_cases = [(1, w, *S16, fl) for w in windows for fl in (False, True)]
    small = run_crops(dev, crop_desc(small_cases, offs, SIZES), 16, u8=False)
    for o in at:
        desc = crop_desc([(0, *c[1:]) for c in small_cases], [o], [SIZES[1]])
        got = run_crops(big, desc, 16, u8=False)
        assert torch.equal(bits(got), bits(small)), o
    del big
    torch.cuda.empty_cache()


def test_workspace_query_refusals():
    _, offs, flat = make_store(SIZES)
    n = flat.size
    ok = crop_desc([CASES[6], CASES[8]], offs, SIZES)
    assert ops.image_prep_crops_workspace(ok.copy(), 16, n) > 0
    for field, value in (("crop_x", 24), ("crop_y", 18), ("crop_w", 54), ("crop_h", 0), ("crop_x", -1)):     # the crop leaves its image
        d = ok.copy()
        d[field][0] = value
        with pytest.raises(_lib.UvcHipError, match="inside its image"):
            ops.image_prep_crops_workspace(d, 16, n)
    with pytest.raises(_lib.UvcHipError, match="past the store"):            # the last image leaves the store, though the crop would not
        ops.image_prep_crops_workspace(crop_desc([CASES[5]], offs, SIZES), 16, n - 1)
    d = ok.copy()
    d["src_offset"][0] = -1
    with pytest.raises(_lib.UvcHipError, match="past the store"):
        ops.image_prep_crops_workspace(d, 16, n)
    with pytest.raises(_lib.UvcHipError, match="bad argument"):              # B = 0
        ops.image_prep_crops_workspace(ok[:0].copy(), 16, n)
    big = crop_desc([(0, (0, 0, 32, 32), (4097, 4097), (0, 0), False)], offs, SIZES)
    with pytest.raises(_lib.UvcHipError, match="bad argument"):              # S above the limit of 4096
        ops.image_prep_crops_workspace(big, 4097, n)
    d = ok.copy()
    d["resize_h"][0] = 15
    with pytest.raises(_lib.UvcHipError, match="resize sides"):
        ops.image_prep_crops_workspace(d, 16, n)


def test_launch_skips_a_descriptor_that_does_not_fit_its_store(store):
    """The descriptors are completed against the whole store, the launch is handed one byte less: the last image no longer fits and
    is skipped (its output rows keep their fill), the others are computed.  Only the descriptor check acts; nothing is read out of bounds."""
    imgs, offs, dev = store
    cases = [CASES[6], CASES[5], CASES[0]]                                   # the middle one is the whole last image
    desc = crop_desc(cases, offs, SIZES)
    got = run_crops(dev[:dev.numel() - 1], desc, 16, check_bytes=dev.numel())
    ref, _ = run_copied(imgs, cases, 16)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[2], ref[2])
    assert bool((got[1] == 77).all())
