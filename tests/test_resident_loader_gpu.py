"""GPU: ResidentLoader (uvc_amd/packed.py) yields, bit for bit, DeviceLoader's batches over the same dataset -- training and both
evaluation geometries, epochs, ranks, the short last batch -- and the reference's host pipeline (PIL); it survives allocator traffic on
another stream and an abandoned iterator, and refuses a store that does not fit the device before uploading anything."""
import numpy as np
import pytest
import torch
from PIL import Image

from uvc_amd import data as D
from uvc_amd import packed as P

pytestmark = pytest.mark.gpu

S, BS = 32, 8
CIFAR = dict(mean=D.CIFAR_MEAN, std=D.CIFAR_STD, scale=(0.05, 1.0), flip=False)
IMAGENET = dict(mean=D.IMAGENET_MEAN, std=D.IMAGENET_STD)


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    rng = np.random.default_rng(5)
    arr = D.ArrayDataset(rng.integers(0, 256, (37, 32, 32, 3), dtype=np.uint8), np.arange(37) % 10)
    root = tmp_path_factory.mktemp("ragged")
    for k in range(23):                                                      # ragged PNGs, sides 20..90
        d = root / "train" / f"c{k % 4}"
        d.mkdir(parents=True, exist_ok=True)
        h, w = int(rng.integers(20, 91)), int(rng.integers(20, 91))
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(d / f"{k}.png")
    path = str(root / "train.uvcpack")
    P.write_pack(D.ImageFolder(str(root / "train")), path)
    return {"array": (arr, CIFAR), "pack": (P.PackedDataset(path), IMAGENET)}


_reference = {}


def device_batches(datasets, name, **kw):
    """DeviceLoader's batches for one setting, computed once and shared (on the CPU)."""
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _reference:
        ds, cfg = datasets[name]
        epoch = kw.pop("epoch", 0)
        ld = D.DeviceLoader(ds, BS, S, num_workers=4, seed=3, **cfg, **kw)
        ld.set_epoch(epoch)
        _reference[key] = ([(x.cpu(), t.cpu()) for x, t in ld], ld.indices(), len(ld), ld.train_steps())
    return _reference[key]


def resident(datasets, name, **kw):
    ds, cfg = datasets[name]
    return P.ResidentLoader(ds, BS, S, num_workers=4, seed=3, **cfg, **kw)


def assert_same(got, want):
    assert len(got) == len(want)
    for k, ((x, t), (rx, rt)) in enumerate(zip(got, want)):
        assert x.dtype == torch.float32 and t.dtype == torch.int64 and x.is_cuda and t.is_cuda
        assert torch.equal(x.cpu().view(torch.int32), rx.view(torch.int32)), k
        assert torch.equal(t.cpu(), rt), k


@pytest.mark.parametrize("name", ["array", "pack"])
def test_training_batches_equal_device_loader(datasets, name):
    n = len(datasets[name][0])
    for rank, world in ((0, 1), (0, 2), (1, 2)):
        ld = resident(datasets, name, train=True, rank=rank, world=world)
        for epoch in (0, 1):
            want, idx, steps, tsteps = device_batches(datasets, name, train=True, rank=rank, world=world, epoch=epoch)
            ld.set_epoch(epoch)
            assert ld.indices() == idx and len(ld) == steps and ld.train_steps() == tsteps
            got = list(ld)
            assert_same(got, want)
            per_rank = -(-n // world)
            assert [len(t) for _, t in got] == [BS] * (per_rank // BS) + ([per_rank % BS] if per_rank % BS else [])
    assert resident(datasets, "array", train=True).train_steps() == 5        # 37 = 4 * 8 + 5: the short batch of five still trains
    assert resident(datasets, "array", train=True, world=2).train_steps() == 3   # 19 per rank


@pytest.mark.parametrize("name", ["array", "pack"])
@pytest.mark.parametrize("mode", ["center", "square"])
def test_evaluation_batches_equal_device_loader(datasets, name, mode):
    want, idx, steps, _ = device_batches(datasets, name, train=False, eval=mode)
    ld = resident(datasets, name, train=False, eval=mode)
    assert ld.indices() == idx == list(range(len(datasets[name][0]))) and len(ld) == steps
    assert_same(list(ld), want)


def test_batches_equal_the_host_pipeline(datasets):
    ds, cfg = datasets["pack"]
    ld = resident(datasets, "pack", train=True)
    ld.set_epoch(2)
    x, t = next(iter(ld))
    ids = ld.indices()[:BS]
    ref = D.host_reference_batch(ds, ids, S, True, 3, 2, cfg["mean"], cfg["std"])
    assert torch.equal(x.cpu().view(torch.int32), ref.view(torch.int32)) and t.tolist() == ds.targets[ids].tolist()
    ev = resident(datasets, "pack", train=False, eval="center")
    x, t = next(iter(ev))
    ref = D.host_reference_batch(ds, list(range(BS)), S, False, 3, 0, cfg["mean"], cfg["std"], eval="center")
    assert torch.equal(x.cpu().view(torch.int32), ref.view(torch.int32)) and t.tolist() == ds.targets[:BS].tolist()
    ds, cfg = datasets["array"]
    x, _ = next(iter(resident(datasets, "array", train=True)))
    ids = resident(datasets, "array", train=True).indices()[:BS]
    ref = D.host_reference_batch(ds, ids, S, True, 3, 0, cfg["mean"], cfg["std"], scale=cfg["scale"], flip=False)
    assert torch.equal(x.cpu().view(torch.int32), ref.view(torch.int32))


def test_allocator_traffic_and_an_abandoned_iterator(datasets):
    """Another stream allocates, fills and frees blocks between the batches, batches are kept alive while later ones are produced, and an
    iterator is dropped halfway: a batch that reused memory still in flight, or a staging slot refilled too early, would differ."""
    want, *_ = device_batches(datasets, "pack", train=True, epoch=0)
    ld = resident(datasets, "pack", train=True)
    side = torch.cuda.Stream()
    for sweep in range(2):
        got = []
        for x, t in ld:
            with torch.cuda.stream(side):
                for nbytes in (x.numel() * 4, 88 * BS, 1 << 20):
                    junk = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
                    junk.fill_(255)
                    del junk
            got.append((x, t))
        assert_same(got, want)
        it = iter(ld)                                                        # abandoned after one batch
        next(it)
        del it
    for _ in ld:
        break
    assert_same(list(ld), want)


def test_copy_stream_has_a_priority_of_its_own_and_no_worker_threads(datasets):
    """The copy stream is a high-priority stream (its hardware queue is none that a trainer's normal-priority side streams share, DESIGN
    "Packed, resident datasets"), and the loader, which decodes and slices nothing, keeps no thread pool."""
    ld = resident(datasets, "array", train=True)
    next(iter(ld))
    assert ld._copy_stream.priority < torch.cuda.Stream().priority and ld._pool is None


def test_capacity_refusal_comes_before_any_upload(datasets, monkeypatch):
    ds, cfg = datasets["array"]
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1 << 20, 288 << 30))
    big = D.ArrayDataset(np.zeros((400, 32, 32, 3), dtype=np.uint8), np.zeros(400))       # 1.2 MB of pixels
    uploads = []
    monkeypatch.setattr(P.ResidentLoader, "_upload_store", lambda self, pixels: uploads.append(len(pixels)))
    with pytest.raises(ValueError, match=r"--resident 0") as e:
        P.ResidentLoader(big, BS, S, **cfg)
    assert str(400 * 32 * 32 * 3 + 8 * 400) in str(e.value) and str(1 << 20) in str(e.value)     # both numbers are named
    assert not uploads
    small = P.ResidentLoader(ds, BS, S, **cfg)                               # 114 KB fits the reported megabyte
    assert uploads == [37 * 32 * 32 * 3] and small.store_bytes == 37 * 32 * 32 * 3


def test_other_datasets_are_told_to_pack():
    class Folder:
        targets = np.zeros(1, np.int64)

        def load(self, i):
            return np.zeros((8, 8, 3), np.uint8)

        def __len__(self):
            return 1
    with pytest.raises(ValueError, match="pack"):
        P.ResidentLoader(Folder(), BS, S)
