"""What the k-NN / transfer tests share (CPU and GPU; nothing here needs a GPU): exact integer operands with the structures the search
can get wrong, the real-valued acceptance rule, vote cases with an asserted margin, a flat-coloured dataset, and the exports."""
import os
import pickle

import numpy as np
import torch

from oracle import vit as OV
from test_compact_cpu import dense_state
from uvc_amd import compact as CP
from uvc_amd import compact_transfer as CT

DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
PX384D = OV.VitConfig(img_size=384, patch_size=16, num_classes=16, embed_dim=64, depth=2, num_heads=1, enable_dist=1)     # N = 578
_EXPORTS = {}


def export_of(name):
    """attribution_ref.export_of's files, and "px384d": 576 patches and two readout tokens."""
    if name == "px384d":
        if name not in _EXPORTS:
            ex = CP.export_compact(dense_state(PX384D))
            assert CP._seq(ex["cfg"]) == 578
            _EXPORTS[name] = (ex, torch.randn(2, 3, 384, 384, generator=torch.Generator().manual_seed(11)))
        return _EXPORTS[name]
    import attribution_ref as AR
    return AR.export_of(name)


# ---- exact operands: integers in [-3, 3], every dot product exact in float32 (|s| <= 9 D <= 9216) ---------------------------------------
def int_operands(nq, n, D, seed, kind="random"):
    """(queries [nq, D], bank [n, D]) float32 on the host with integer entries in [-3, 3].
    random: independent draws (many equal similarities at small D: ties by index everywhere);
    dup: every bank row appears three times in a row; zeroq: query 0 is all zero (its list is the first k rows);
    ascend / descend: constant positive queries and bank rows whose sums rise / fall strictly with the index (every row inserts / none
    after the first k); asym: bank row i is i % 7 - 3 at column i % D alone and queries are all ones on ONE column each --
    similarities that differ under a row/column swap."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(-3, 4, (nq, D), generator=g).float()
    b = torch.randint(-3, 4, (n, D), generator=g).float()
    if kind == "dup":
        b = b[torch.arange(n) // 3]
    elif kind == "zeroq":
        q[0] = 0
    elif kind in ("ascend", "descend"):
        assert n <= 6 * D + 1                                            # row sums -3 D .. 3 D: one distinct sum per row
        q = torch.randint(1, 4, (nq, 1), generator=g).float().expand(nq, D).contiguous()      # a constant c > 0 per query: s = c * row sum
        t = torch.arange(n) if kind == "ascend" else n - 1 - torch.arange(n)
        b = (-3 + (t[:, None] - 6 * torch.arange(D)[None, :]).clamp(0, 6)).float()
    elif kind == "asym":
        b.zero_()
        b[torch.arange(n), torch.arange(n) % D] = (torch.arange(n) % 7 - 3).float()
        q.zero_()
        q[torch.arange(nq), (3 * torch.arange(nq) + 1) % D] = 1.0
    return q, b


def beta(q, b):
    """[nq, n] float64: D * 2^-24 * sum_d |q_d x_d|, the float32 summation bound of a D-term dot product (operands as given)."""
    return q.shape[1] * 2.0 ** -24 * (q.double().abs() @ b.double().abs().T)


def check_real(q, b, sims, idx, k):
    """The real-valued acceptance rule; returns (max |sim - dot| / beta over the listed pairs, max excess of a row left out / beta)."""
    q, b = q.cpu(), b.cpu()
    s = q.double() @ b.double().T
    bt = beta(q, b)
    sims, idx = sims.cpu().double(), idx.cpu().long()
    n = b.shape[0]
    assert sims.shape == (q.shape[0], k) and idx.shape == sims.shape
    kk = min(k, n)
    assert (idx[:, kk:] == -1).all() and (sims[:, kk:] == float("-inf")).all()
    li, ls = idx[:, :kk], sims[:, :kk]
    assert (li >= 0).all() and (li < n).all()
    assert all(len(set(r)) == kk for r in li.tolist())                      # no row twice
    own, own_b = s.gather(1, li), bt.gather(1, li)
    e_own = ((ls - own).abs() / own_b.clamp_min(1e-300)).max()
    assert ((ls - own).abs() <= own_b).all(), float(e_own)
    assert (ls[:, :-1] >= ls[:, 1:]).all()                                  # descending
    tie = ls[:, :-1] == ls[:, 1:]
    assert (li[:, :-1][tie] < li[:, 1:][tie]).all()                         # equal values by ascending index
    out = torch.ones_like(s, dtype=torch.bool)
    out.scatter_(1, li, False)
    excess = (s - own[:, -1:] - 2 * bt) * out
    assert (excess <= 0).all(), float(excess.max())
    return float(e_own), float((((s - own[:, -1:]) / bt.clamp_min(1e-300)) * out).max())


# ---- vote cases ----------------------------------------------------------------------------------------------------------------------
def vote_case(nq, n, k, C, seed, T=0.07):
    """(sims float32 [nq, k] descending, idx int32 [nq, k], labels int64 [n]) whose reference margin between the two best classes exceeds
    1e-4 of the best (asserted here): rows are redrawn until it does."""
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, C, (n,), generator=g)
    sims = torch.empty(nq, k)
    idx = torch.empty(nq, k, dtype=torch.int32)
    for i in range(nq):
        while True:
            s = torch.sort(torch.rand(k, generator=g) * 0.5 + 0.3, descending=True).values
            ix = torch.randperm(n, generator=g)[:k].to(torch.int32) if n >= k else torch.randint(0, n, (k,), generator=g).to(torch.int32)
            sc, _ = CT.reference_vote(s[None], ix[None], labels, C, T)
            top = np.sort(sc[0])[::-1]
            if C == 1 or top[0] - top[1] > 1e-4 * top[0]:
                break
        sims[i], idx[i] = s, ix
    sc, pred = CT.reference_vote(sims, idx, labels, C, T)
    top = np.sort(sc, axis=1)[:, ::-1]
    assert C == 1 or (top[:, 0] - top[:, 1] > 1e-4 * top[:, 0]).all()
    return sims, idx, labels, sc, pred


# ---- a dataset of flat colours ---------------------------------------------------------------------------------------------------------
COLOURS = np.array([[230, 40, 40], [40, 230, 40], [40, 40, 230]], dtype=np.int64)


def colour_images(n, seed, classes=3, side=32, noise=12):
    """(uint8 [n, side, side, 3], int64 [n]): class c is COLOURS[c] plus uniform noise in [-noise, noise]; labels cycle."""
    rng = np.random.default_rng(seed)
    y = np.arange(n) % classes
    img = COLOURS[y][:, None, None, :] + rng.integers(-noise, noise + 1, (n, side, side, 3))
    return np.clip(img, 0, 255).astype(np.uint8), y.astype(np.int64)


def write_cifar10(root, train, test):
    """The python pickles of CIFAR-10 under ``root`` from (images, labels) pairs (data.read_cifar reads them back)."""
    base = os.path.join(root, "cifar-10-batches-py")
    os.makedirs(base, exist_ok=True)
    rows = lambda im: np.ascontiguousarray(im.transpose(0, 3, 1, 2)).reshape(len(im), -1)
    parts = np.array_split(np.arange(len(train[0])), 5)
    for i, p in enumerate(parts, 1):
        with open(os.path.join(base, f"data_batch_{i}"), "wb") as f:
            pickle.dump({"data": rows(train[0][p]), "labels": train[1][p].tolist()}, f)
    with open(os.path.join(base, "test_batch"), "wb") as f:
        pickle.dump({"data": rows(test[0]), "labels": test[1].tolist()}, f)
    return root
