"""GPU: uvc_image_prep (include/uvc_data.h) against PIL bit for bit, the float32 normalisation against torch bitwise, ragged
batches, a batch whose packed sources pass 2^31 bytes, and the DeviceLoader against the reference's host pipeline."""
import numpy as np
import pytest
import torch
from PIL import Image

from uvc_amd import data as D
from uvc_amd import ops

pytestmark = pytest.mark.gpu

MEAN, STD = D.IMAGENET_MEAN, D.IMAGENET_STD


def run_batch(items, S, u8=True, mean=MEAN, std=STD, src=None):
    """items: list of (uint8 HWC array, (resize_h, resize_w), (win_y, win_x), flip).  Packs the sources, completes the descriptors,
    runs the three launches; returns the [B, 3, S, S] output on the CPU."""
    B = len(items)
    sizes = [a.size for a, *_ in items]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    if src is None:
        src = torch.from_numpy(np.concatenate([a.reshape(-1) for a, *_ in items])).cuda()
    desc = np.zeros(B, ops.image_desc_dtype())
    for b, (a, (rh, rw), (wy, wx), fl) in enumerate(items):
        desc[b] = (offs[b], a.shape[0], a.shape[1], rh, rw, wy, wx, int(fl), 0, 0, 0, 0, 0, 0)
    ws_bytes = ops.image_prep_workspace(desc, S, src.numel())
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device="cuda")
    out = torch.empty(B, 3, S, S, dtype=torch.uint8 if u8 else torch.float32, device="cuda")
    out.fill_(77 if u8 else float("nan"))
    ops.image_prep(src, torch.from_numpy(desc.view(np.uint8).copy()).cuda(), ws, out, mean, std)
    torch.cuda.synchronize()
    return out.cpu()


def pil_ref(a, rsize, win, flip, S):
    im = Image.fromarray(a).resize((rsize[1], rsize[0]), Image.BILINEAR).crop((win[1], win[0], win[1] + S, win[0] + S))
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return torch.from_numpy(np.array(im, dtype=np.uint8)).permute(2, 0, 1)


def random_cases(rng, n):
    """(array, resize, window, flip, S) mixes: train crops from 1 px wide to full frame, 20x downscales, 32 -> 224 upscales, eval geometry."""
    out = []
    for t in range(n):
        S = int([32, 224, 384][t % 3])
        kind = t % 5
        if kind == 0:                                            # random resized crop of a photo-sized source
            H, W = int(rng.integers(S // 2, 2 * S)), int(rng.integers(S // 2, 2 * S))
            a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
            i, j = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
            a = np.ascontiguousarray(a[i:i + h, j:j + w])
            out.append((a, (S, S), (0, 0), bool(t & 1), S))
        elif kind == 1:                                          # up to 20x downscale, thin strips
            f = float(rng.uniform(1.0, 20.0))
            H, W = max(1, int(S * f)), (int(rng.integers(1, 4)) if t % 2 else int(rng.integers(S, 4 * S)))
            a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            out.append((a, (S, S), (0, 0), bool(t & 2), S))
        elif kind == 2:                                          # upscale from 32 x 32 and smaller
            e = int(rng.integers(1, 33))
            a = rng.integers(0, 256, (e, int(rng.integers(1, 33)), 3), dtype=np.uint8)
            out.append((a, (S, S), (0, 0), bool(t & 1), S))
        else:                                                    # eval geometry: landscape, portrait, square, odd sizes
            H = int(rng.integers(S // 2, 3 * S)) | 1
            W = [int(rng.integers(H, 3 * S)), int(rng.integers(S // 2, H + 1)), H][t % 3]
            a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            rh, rw = D.resize_short_side(H, W, S * 256 // 224)
            wy, wx = D.center_crop_offset(rh, rw, S)
            out.append((a, (rh, rw), (wy, wx), kind == 4 and bool(t & 1), S))
    return out


def test_uint8_output_equals_pil_bit_for_bit():
    rng = np.random.default_rng(0)
    cases = random_cases(rng, 330)
    bad = []
    for S in (32, 224, 384):                                     # one ragged batch per output size
        sub = [c for c in cases if c[4] == S]
        got = run_batch([c[:4] for c in sub], S)
        for b, (a, rs, win, fl, _) in enumerate(sub):
            if not torch.equal(got[b], pil_ref(a, rs, win, fl, S)):
                bad.append((S, a.shape, rs, win, fl))
    assert not bad, bad[:5]
    assert len(cases) >= 300


def test_float32_output_equals_torch_normalise_bitwise():
    rng = np.random.default_rng(1)
    cases = random_cases(rng, 60)
    for S in (32, 224):
        sub = [c[:4] for c in cases if c[4] == S]
        u8 = run_batch(sub, S)
        for mean, std in ((MEAN, STD), (D.CIFAR_MEAN, D.CIFAR_STD)):
            f = run_batch(sub, S, u8=False, mean=mean, std=std)
            ref = (u8.float() / 255 - torch.tensor(mean).view(1, 3, 1, 1)) / torch.tensor(std).view(1, 3, 1, 1)
            assert torch.equal(f.view(torch.int32), ref.view(torch.int32))


def test_ragged_batch_equals_single_images_and_is_deterministic():
    rng = np.random.default_rng(2)
    S = 224
    cases = [c[:4] for c in random_cases(rng, 200) if c[4] == S][:64]
    while len(cases) < 64:
        cases.append(cases[len(cases) % 8])
    batch = run_batch(cases, S, u8=False)
    again = run_batch(cases, S, u8=False)
    assert torch.equal(batch.view(torch.int32), again.view(torch.int32))
    perm = rng.permutation(64)
    shuffled = run_batch([cases[k] for k in perm], S, u8=False)
    assert torch.equal(shuffled.view(torch.int32), batch[torch.from_numpy(perm)].view(torch.int32))
    for b in range(0, 64, 3):
        single = run_batch([cases[b]], S, u8=False)
        assert torch.equal(single[0].view(torch.int32), batch[b].view(torch.int32)), b


def test_packed_sources_past_2_gib():
    """One batch whose packed sources pass 2^31 bytes: the images behind the boundary read their own bytes (64-bit offsets);
    sampled images checked against PIL and against a float64 evaluation of the same fixed-point weights."""
    H, W, B, S = 4096, 6144, 29, 32                             # 75.5 MB each, 2.19 GB in all
    img = H * W * 3
    total = img * B
    assert total > (1 << 31)
    torch.manual_seed(0)
    src = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda")
    items = []
    for b in range(B):
        a = np.empty((H, W, 3), np.uint8)                     # shape stand-in: the pixels live in src
        items.append((a, (S, S), (0, 0), b % 2 == 1))
    got = run_batch(items, S, src=src)
    import pil_bilinear as PB
    for b in (0, B // 2, B - 1):                             # the last one straddles byte 2^31
        a = src[b * img:(b + 1) * img].cpu().numpy().reshape(H, W, 3)
        ref = pil_ref(a, (S, S), (0, 0), b % 2 == 1, S)
        assert torch.equal(got[b], ref), b
        # float64 check of one row of outputs through the restated coefficients
        hx, hn, hk = PB.coeffs(W, 0, W, S)
        vy, vn, vk = PB.coeffs(H, 0, H, S)
        r = 5
        rows = a[vy[r]:vy[r] + vn[r]].astype(np.float64)
        inter = np.stack([PB.clip8(np.int64(1 << 21) + (rows[:, hx[c]:hx[c] + hn[c]] * hk[c, :hn[c]][None, :, None]).sum(1).astype(np.int64))
                          for c in range(S)], 1).astype(np.float64)
        v = PB.clip8(np.int64(1 << 21) + (inter * vk[r, :vn[r]][:, None, None]).sum(0).astype(np.int64))
        v = v[::-1] if b % 2 == 1 else v
        assert np.array_equal(got[b, :, r, :].numpy(), v.T), b
    del src
    torch.cuda.empty_cache()


def write_image_folder(root, n_per_class=(5, 4, 4), seed=0):
    rng = np.random.default_rng(seed)
    for c, n in enumerate(n_per_class):
        d = root / f"class_{c}"
        d.mkdir(parents=True)
        for k in range(n):
            H, W = int(rng.integers(20, 140)), int(rng.integers(20, 140))
            a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            a = (a // 3 + np.linspace(0, 160, W, dtype=np.uint8)[None, :, None]).astype(np.uint8)
            if k % 2:
                Image.fromarray(a).save(d / f"im{k}.JPEG", quality=90)
            else:
                Image.fromarray(a).save(d / f"im{k}.png")


@pytest.mark.parametrize("train", [True, False])
def test_device_loader_equals_host_pipeline(tmp_path, train):
    write_image_folder(tmp_path)
    ds = D.ImageFolder(str(tmp_path))
    S, bs = 32, 5
    runs = {}
    for threads in (1, 8):
        ld = D.DeviceLoader(ds, bs, S, train=train, seed=3, num_workers=threads)
        ld.set_epoch(2)
        got = [(x.cpu(), t.cpu()) for x, t in ld]
        assert len(got) == len(ld) == 3 and [len(t) for _, t in got] == [5, 5, 3]          # the short last batch is there
        idx = ld.indices()
        for k, (x, t) in enumerate(got):
            ids = idx[k * bs:(k + 1) * bs]
            ref = D.host_reference_batch(ds, ids, S, train, 3, 2, MEAN, STD)
            assert torch.equal(x.view(torch.int32), ref.view(torch.int32)), (threads, k)
            assert t.tolist() == ds.targets[ids].tolist()
        runs[threads] = got
    for (x1, t1), (x8, t8) in zip(runs[1], runs[8]):
        assert torch.equal(x1, x8) and torch.equal(t1, t8)


def test_device_loader_ranks_and_epochs(tmp_path):
    rng = np.random.default_rng(4)
    ds = D.ArrayDataset(rng.integers(0, 256, (21, 32, 32, 3), dtype=np.uint8), np.arange(21) % 10)
    lds = [D.DeviceLoader(ds, 4, 32, train=True, mean=D.CIFAR_MEAN, std=D.CIFAR_STD, scale=(0.05, 1.0), flip=False, seed=1, rank=r,
                          world=2, num_workers=4) for r in range(2)]
    seen = []
    for ld in lds:
        ld.set_epoch(0)
        assert len(ld) == 3 and len(ld.indices()) == 11
        n = sum(len(t) for _, t in ld)
        assert n == 11
        seen.append(ld.indices())
    assert set(seen[0][:10]).isdisjoint(seen[1][:10]) and set(seen[0]) | set(seen[1]) == set(range(21))
    # a sample's crop is the same whichever rank / world size reads it
    one = D.DeviceLoader(ds, 32, 32, train=True, mean=D.CIFAR_MEAN, std=D.CIFAR_STD, scale=(0.05, 1.0), flip=False, seed=1, num_workers=2)
    x_all, _ = next(iter(one))
    pos = {k: p for p, k in enumerate(one.indices())}
    x0, _ = next(iter(lds[0]))
    for p, k in enumerate(seen[0][:4]):
        assert torch.equal(x0[p], x_all[pos[k]])
    lds[0].set_epoch(1)
    assert lds[0].indices() != seen[0]
    # an early break leaves no producer behind and the loader can start again
    for _ in lds[0]:
        break
    assert sum(len(t) for _, t in lds[0]) == 11
