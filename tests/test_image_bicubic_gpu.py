"""GPU: the bicubic filter of uvc_image_prep / uvc_image_prep_crops (include/uvc_data.h) against PIL's Image.resize(BICUBIC) bit for bit --
the shared cases of tests/pil_resample.py (which tests/test_image_bicubic_cpu.py shows to overshoot in both passes, so the clamps work)
in ragged batches with windows and flips, the float32 normalisation, crops of a store against copied crops, filter 0 through the new
queries against the old entry points, the refusals, and both loaders against the host pipeline."""
import numpy as np
import pytest
import torch
from PIL import Image

import pil_resample as R
from uvc_amd import _lib as L
from uvc_amd import data as D
from uvc_amd import ops
from uvc_amd import packed as P

pytestmark = pytest.mark.gpu

MEAN, STD = D.IMAGENET_MEAN, D.IMAGENET_STD
BICUBIC, BILINEAR = L.UVC_IMAGE_FILTER_BICUBIC, L.UVC_IMAGE_FILTER_BILINEAR
GUARD = 4096                                                     # sentinel bytes on both sides of every workspace


def clamp_case(name):
    """A clamp-covering image of tests/pil_resample.py as a batch item resized to its own (w, h)."""
    _, a, (w, h) = next(c for c in R.CLAMP_CASES if c[0] == name)
    return a, (h, w)


# items: (uint8 HWC array, (resize_h, resize_w), (win_y, win_x), flip); one ragged batch per key, B <= 8
BATCHES = {
    # S = 8: scale > 4 on both axes, 1 x 1 and 1 x 7 sources, the source resized vertically first (404 > 100 * 3), one axis unchanged
    # with a centre window, on noise, step edge and checkerboard
    "s8_shapes": (8, [(R.noise(23, 37), (8, 8), (0, 0), False),
                      (R.noise(1, 1, 1), (8, 8), (0, 0), True),
                      (R.noise(1, 7, 2), (8, 8), (0, 0), False),
                      (R.noise(404, 3, 3), (8, 8), (0, 0), True),
                      (R.noise(30, 20, 4), (12, 20), (2, 6), False),
                      (R.noise(12, 30, 5), (12, 17), (4, 9), True),
                      (R.checkerboard(404, 3), (8, 8), (0, 0), False),
                      (R.step_edge(23, 37), (8, 8), (0, 0), True)]),
    # S = 8: the clamp-covering images, and the other shapes on the 0 / 255 patterns (the tall one with a window)
    "s8_clamps": (8, [(*clamp_case("checkerboard_8"), (0, 0), False),
                      (*clamp_case("checkerboard_down"), (0, 0), True),
                      (*clamp_case("step_8"), (0, 0), True),
                      (*clamp_case("step_rows_8"), (0, 0), False),
                      (R.checkerboard(30, 20), (12, 20), (4, 12), False),
                      (R.step_edge(12, 30), (12, 17), (0, 3), True),
                      (R.checkerboard(1, 7), (8, 8), (0, 0), False),
                      (R.checkerboard(404, 3, 40), (10, 9), (1, 1), True)]),
    "s16": (16, [(*clamp_case("checkerboard_16"), (0, 0), True),
                 (*clamp_case("step_16"), (0, 0), False),
                 (*clamp_case("step_rows_16"), (0, 0), True),
                 (R.noise(37, 23, 6), (21, 18), (3, 1), False),
                 (R.noise(404, 3, 7), (16, 16), (0, 0), True),
                 (R.noise(1, 1, 8), (16, 16), (0, 0), False),
                 (R.checkerboard(23, 37, 8), (17, 27), (1, 6), True),
                 (R.step_edge(30, 20), (30, 16), (7, 0), False)]),
    # S = 224: the 32 -> 224 upscale of every pattern, and the ImageNet eval geometry 500 x 375 -> 341 x 256 -> centre 224
    "s224": (224, [(R.noise(32, 32, 9), (224, 224), (0, 0), False),
                   (*clamp_case("checkerboard_up"), (0, 0), True),
                   (*clamp_case("step_up"), (0, 0), True),
                   (*clamp_case("step_rows_up"), (0, 0), False),
                   (R.noise(375, 500, 10), D.resize_short_side(375, 500, 256), D.center_crop_offset(256, 341, 224), False)]),
}


def guarded(nbytes):
    """(whole tensor, 16-aligned workspace view of nbytes inside it) with GUARD sentinel bytes on both sides."""
    whole = torch.full((GUARD + max(nbytes, 16) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD:GUARD + max(nbytes, 16)]


def guards_intact(whole):
    return bool((whole[:GUARD] == 0xA5).all()) and bool((whole[-GUARD:] == 0xA5).all())


def image_desc(items):
    sizes = [a.size for a, *_ in items]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    desc = np.zeros(len(items), ops.image_desc_dtype())
    for b, (a, (rh, rw), (wy, wx), fl) in enumerate(items):
        desc[b] = (offs[b], a.shape[0], a.shape[1], rh, rw, wy, wx, int(fl), 0, 0, 0, 0, 0, 0)
    return desc, torch.from_numpy(np.concatenate([a.reshape(-1) for a, *_ in items])).cuda()


def launch(entry, src, desc, ws_bytes, S, filt, u8=True, mean=MEAN, std=STD):
    """One launch of ``entry`` (ops.image_prep or ops.image_prep_crops) on completed descriptors, into a sentinel-filled output and a
    guarded workspace; the guards must come back intact."""
    whole, ws = guarded(ws_bytes)
    out = torch.empty(len(desc), 3, S, S, dtype=torch.uint8 if u8 else torch.float32, device="cuda")
    out.fill_(77 if u8 else float("nan"))
    entry(src, torch.from_numpy(desc.view(np.uint8).copy()).cuda(), ws, out, mean, std, filter=filt)
    torch.cuda.synchronize()
    assert guards_intact(whole)
    return out.cpu()


def run_batch(items, S, filt=BICUBIC, **kw):
    desc, src = image_desc(items)
    ws_bytes = ops.image_prep_workspace(desc, S, src.numel(), filt)
    return launch(ops.image_prep, src, desc, ws_bytes, S, filt, **kw)


def pil_ref(a, rsize, win, flip, S, resample=Image.BICUBIC):
    im = Image.fromarray(a).resize((rsize[1], rsize[0]), resample).crop((win[1], win[0], win[1] + S, win[0] + S))
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return torch.from_numpy(np.array(im, dtype=np.uint8)).permute(2, 0, 1)


@pytest.fixture(scope="module")
def pil_bytes():
    """PIL's bytes of every batch, computed once."""
    return {k: torch.stack([pil_ref(*item, S) for item in items]) for k, (S, items) in BATCHES.items()}


@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_uint8_output_equals_pil_bicubic_bit_for_bit(batch, pil_bytes):
    S, items = BATCHES[batch]
    assert len(items) <= 8
    got = run_batch(items, S)
    bad = [b for b in range(len(items)) if not torch.equal(got[b], pil_bytes[batch][b])]
    assert not bad, bad
    # and through the crops entry, every source a whole-image window of the packed batch
    desc, src = image_desc(items)
    cd = np.zeros(len(items), ops.image_crop_desc_dtype())
    for b, (a, (rh, rw), (wy, wx), fl) in enumerate(items):
        cd[b] = (desc["src_offset"][b], a.shape[0], a.shape[1], 0, 0, a.shape[0], a.shape[1], rh, rw, wy, wx, int(fl), 0, 0, 0, 0, 0, 0)
    got = launch(ops.image_prep_crops, src, cd, ops.image_prep_crops_workspace(cd, S, src.numel(), BICUBIC), S, BICUBIC)
    assert torch.equal(got, pil_bytes[batch])
    for f in ("kh", "kv", "span0", "span", "order"):
        assert np.array_equal(cd[f], image_desc_completed(items, S)[f]), f


def image_desc_completed(items, S, filt=BICUBIC):
    desc, src = image_desc(items)
    ops.image_prep_workspace(desc, S, src.numel(), filt)
    return desc


def test_the_batches_take_the_paths_they_name():
    d8 = image_desc_completed(BATCHES["s8_shapes"][1], 8)
    assert d8["order"].tolist() == [0, 0, 0, 1, 0, 0, 1, 0]                        # the 404 x 3 sources go vertically first
    assert d8["kh"][0] == 2 * int(np.ceil(2 * 37 / 8)) + 1 == 21 and d8["kv"][0] == 2 * int(np.ceil(2 * 23 / 8)) + 1 == 13
    assert d8["kh"][4] == 5 and d8["kh"][1] == 5                                   # unchanged axis and upscale: support 2, ksize 5
    bl = image_desc_completed(BATCHES["s8_shapes"][1], 8, BILINEAR)
    assert (bl["kh"] < d8["kh"]).all() and (bl["kv"] < d8["kv"]).all()
    e = image_desc_completed(BATCHES["s224"][1], 224)[4]                           # 500 -> 341: ksize 7 against bilinear's 5
    eb = image_desc_completed(BATCHES["s224"][1], 224, BILINEAR)[4]
    assert (e["kh"], e["kv"]) == (7, 7) and (eb["kh"], eb["kv"]) == (5, 5)
    assert BATCHES["s224"][1][4][1:3] == ((256, 341), (16, 58))


@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_float32_output_equals_torch_normalise_bitwise(batch, pil_bytes):
    S, items = BATCHES[batch]
    u8 = pil_bytes[batch]
    for mean, std in ((MEAN, STD), (D.CIFAR_MEAN, D.CIFAR_STD)):
        f = run_batch(items, S, u8=False, mean=mean, std=std)
        ref = (u8.float() / 255 - torch.tensor(mean).view(1, 3, 1, 1)) / torch.tensor(std).view(1, 3, 1, 1)
        assert torch.equal(f.view(torch.int32), ref.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- crops of a store

STORE = [R.noise(37, 53, 11), R.checkerboard(32, 32), R.noise(240, 5, 12), R.step_edge(8, 8), R.checkerboard(64, 48, 3)]
S16 = ((16, 16), (0, 0))
# (image, (crop_y, crop_x, crop_h, crop_w), (resize_h, resize_w), (win_y, win_x), flip)
CROPS = [(0, (5, 7, 20, 30), *S16, True),                         # interior window: row stride 53 * 3, crop width 30
         (1, (3, 2, 6, 5), *S16, False),                           # 6 x 5 of the checkerboard upscaled: overshoots in both passes
         (2, (20, 2, 210, 2), *S16, True),                         # 210 > 100 * 2: vertical pass first
         (2, (0, 0, 240, 3), *S16, False),                         # 240 <= 100 * 3: horizontal first
         (3, (1, 1, 7, 6), *S16, True),                            # step edge, upscaled
         (4, (40, 30, 24, 18), *S16, False),                       # flush with the store's last byte
         (4, (3, 4, 60, 40), (24, 16), (4, 0), True),              # Resize + CenterCrop geometry
         (0, (36, 52, 1, 1), *S16, False)]                         # 1 x 1 crop


@pytest.mark.parametrize("u8", [True, False], ids=["uint8", "float32"])
def test_crops_equal_copies_under_bicubic(u8):
    S = 16
    offs = np.concatenate([[0], np.cumsum([a.size for a in STORE])]).astype(np.int64)
    store = torch.from_numpy(np.concatenate([a.reshape(-1) for a in STORE])).cuda()
    cd = np.zeros(len(CROPS), ops.image_crop_desc_dtype())
    for b, (k, (cy, cx, ch, cw), (rh, rw), (wy, wx), fl) in enumerate(CROPS):
        cd[b] = (offs[k], STORE[k].shape[0], STORE[k].shape[1], cy, cx, ch, cw, rh, rw, wy, wx, int(fl), 0, 0, 0, 0, 0, 0)
    got = launch(ops.image_prep_crops, store, cd, ops.image_prep_crops_workspace(cd, S, store.numel(), BICUBIC), S, BICUBIC, u8=u8)
    copies = [(np.ascontiguousarray(STORE[k][cy:cy + ch, cx:cx + cw]), rs, win, fl) for k, (cy, cx, ch, cw), rs, win, fl in CROPS]
    want = run_batch(copies, S, u8=u8)
    assert torch.equal(got.view(torch.int32) if not u8 else got, want.view(torch.int32) if not u8 else want)
    assert cd["order"].tolist() == [0, 0, 1, 0, 0, 0, 0, 0]
    if u8:
        for b, (a, rs, win, fl) in enumerate(copies):
            assert torch.equal(got[b], pil_ref(a, rs, win, fl, S)), b
        accs = []
        R.resize(copies[1][0], (16, 16), R.BICUBIC, accs=accs)
        assert all(min(R.overshoot(acc)) >= 1 for acc in accs)     # the checkerboard crop does make both clamps work


# ---------------------------------------------------------------------------------------------------------------- filter 0, refusals

def test_filter_0_through_the_new_queries_equals_the_old_entry_points():
    S, items = BATCHES["s16"]
    d_old, src = image_desc(items)
    d_new = d_old.copy()
    b_old, b_new = ops.image_prep_workspace(d_old, S, src.numel()), ops.image_prep_workspace(d_new, S, src.numel(), BILINEAR)
    assert b_old == b_new and d_old.tobytes() == d_new.tobytes()
    ws = torch.empty(b_old, dtype=torch.uint8, device="cuda")
    dd = torch.from_numpy(d_old.view(np.uint8).copy()).cuda()
    for dtype in (torch.uint8, torch.float32):
        o_old, o_new = (torch.zeros(len(items), 3, S, S, dtype=dtype, device="cuda") for _ in range(2))
        ops.image_prep(src, dd, ws, o_old, MEAN, STD)                                          # the struct's filter field left at 0
        ops.image_prep(src, dd, ws, o_new, MEAN, STD, filter=BILINEAR)
        assert torch.equal(o_old, o_new)
    assert torch.equal(o_old.cpu().view(torch.int32),
                       run_batch(items, S, BILINEAR, u8=False).view(torch.int32))
    assert torch.equal(run_batch(items, S, BILINEAR), torch.stack([pil_ref(*it, S, Image.BILINEAR) for it in items]))
    assert ops.image_prep_workspace(d_new.copy(), S, src.numel(), BICUBIC) > b_old
    # the crops entry
    c_old = np.zeros(len(items), ops.image_crop_desc_dtype())
    for b, (a, (rh, rw), (wy, wx), fl) in enumerate(items):
        c_old[b] = (d_old["src_offset"][b], a.shape[0], a.shape[1], 0, 0, a.shape[0], a.shape[1], rh, rw, wy, wx, int(fl), 0, 0, 0, 0, 0, 0)
    c_new = c_old.copy()
    assert ops.image_prep_crops_workspace(c_old, S, src.numel()) == ops.image_prep_crops_workspace(c_new, S, src.numel(), BILINEAR) == b_old
    assert c_old.tobytes() == c_new.tobytes()
    cdev = torch.from_numpy(c_old.view(np.uint8).copy()).cuda()
    o_c = torch.zeros(len(items), 3, S, S, dtype=torch.float32, device="cuda")
    ops.image_prep_crops(src, cdev, ws, o_c, MEAN, STD, filter=BILINEAR)
    assert torch.equal(o_c, o_old)


def test_unknown_filters_are_refused():
    S, items = BATCHES["s16"]
    desc, src = image_desc(items)
    cd = np.zeros(1, ops.image_crop_desc_dtype())
    cd[0] = (0, 37, 23, 0, 0, 37, 23, 16, 16, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    for bad in (2, -1, 7):
        with pytest.raises(L.UvcHipError, match=r"rc=1"):
            ops.image_prep_workspace(desc.copy(), S, src.numel(), bad)
        with pytest.raises(L.UvcHipError, match=r"rc=1"):
            ops.image_prep_crops_workspace(cd.copy(), S, src.numel(), bad)
    ws_bytes = ops.image_prep_workspace(desc, S, src.numel(), BICUBIC)
    whole, ws = guarded(ws_bytes)
    out = torch.full((len(items), 3, S, S), 77, dtype=torch.uint8, device="cuda")
    with pytest.raises(L.UvcHipError, match=r"rc=1"):                              # refused on the host: nothing is launched
        ops.image_prep(src, torch.from_numpy(desc.view(np.uint8).copy()).cuda(), ws, out, MEAN, STD, filter=2)
    torch.cuda.synchronize()
    assert bool((out == 77).all()) and bool((whole == 0xA5).all())


@pytest.mark.parametrize("launched", [BICUBIC, BILINEAR], ids=["bilinear_desc_as_bicubic", "bicubic_desc_as_bilinear"])
def test_descriptors_of_the_other_filter_leave_their_image_untouched(launched):
    """Images 2 and 5 carry descriptors completed for the other filter (their kh, kv, span and workspace offsets are those of that
    filter's layout): the launch skips them -- sentinel intact, nothing written outside the workspace -- and the others are PIL's."""
    S, items = BATCHES["s16"]
    other = BILINEAR if launched == BICUBIC else BICUBIC
    desc, src = image_desc(items)
    foreign = desc.copy()
    ws_bytes = ops.image_prep_workspace(desc, S, src.numel(), launched)
    ops.image_prep_workspace(foreign, S, src.numel(), other)
    assert (foreign["kh"] != desc["kh"]).all() and (foreign["kv"] != desc["kv"]).all()
    mixed = desc.copy()
    mixed[[2, 5]] = foreign[[2, 5]]
    resample = Image.BICUBIC if launched == BICUBIC else Image.BILINEAR
    for u8 in (True, False):
        got = launch(ops.image_prep, src, mixed, ws_bytes, S, launched, u8=u8)
        for b, item in enumerate(items):
            if b in (2, 5):
                assert bool((got[b] == 77).all()) if u8 else bool(torch.isnan(got[b]).all()), b
            elif u8:
                assert torch.equal(got[b], pil_ref(*item, S, resample)), b
            else:
                assert not torch.isnan(got[b]).any(), b
    # a whole batch completed for the other filter, in a workspace of that filter's (smaller or larger) size: nothing runs
    got = launch(ops.image_prep, src, foreign, ops.image_prep_workspace(foreign.copy(), S, src.numel(), other), S, launched)
    assert bool((got == 77).all())


# ---------------------------------------------------------------------------------------------------------------- loaders

class _Ragged:
    """12 images of 20-40 px sides, in memory."""

    def __init__(self):
        rng = np.random.default_rng(13)
        self.images = [rng.integers(0, 256, (int(rng.integers(20, 41)), int(rng.integers(20, 41)), 3), dtype=np.uint8) for _ in range(12)]
        self.targets = np.arange(12, dtype=np.int64) % 5
        self.classes = None

    def __len__(self):
        return 12

    def load(self, i):
        return self.images[i]


@pytest.fixture(scope="module")
def pack(tmp_path_factory):
    ds = _Ragged()
    path = str(tmp_path_factory.mktemp("bicubic") / "train.uvcpack")
    P.write_pack(ds, path)
    return ds, P.PackedDataset(path)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval_crop_pct_0.9"])
def test_loaders_equal_the_host_pipeline_under_bicubic(pack, train):
    ds, pk = pack
    S, bs, seed, epoch = 16, 4, 3, 2
    kw = dict(train=train, seed=seed, interpolation="bicubic", crop_pct=None if train else 0.9)
    dev = D.DeviceLoader(ds, bs, S, num_workers=2, **kw)
    res = P.ResidentLoader(pk, bs, S, **kw)
    assert dev.filter == res.filter == BICUBIC and dev.eval_side == (18 if train else 17)
    batches = {}
    for name, ld in (("device", dev), ("resident", res)):
        ld.set_epoch(epoch)
        batches[name] = [(x.cpu(), t.cpu()) for x, t in ld]
        assert len(batches[name]) == 3
    idx = dev.indices()
    assert idx == res.indices()
    bil = 0
    for k, ((xd, td), (xr, tr)) in enumerate(zip(batches["device"], batches["resident"])):
        ids = idx[k * bs:(k + 1) * bs]
        ref = D.host_reference_batch(ds, ids, S, train, seed, epoch, MEAN, STD, interpolation="bicubic", crop_pct=kw["crop_pct"])
        assert torch.equal(xd.view(torch.int32), ref.view(torch.int32)), k
        assert torch.equal(xr.view(torch.int32), xd.view(torch.int32)), k
        assert td.tolist() == tr.tolist() == ds.targets[ids].tolist()
        bil += int(torch.equal(ref, D.host_reference_batch(ds, ids, S, train, seed, epoch, MEAN, STD)))
    assert bil == 0                                              # (the bilinear pipeline gives other batches)
