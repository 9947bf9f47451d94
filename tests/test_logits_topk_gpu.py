"""GPU: uvc_logits_topk (include/uvc_kernels.h) -- softmax over the valid columns + top-k -- against the float64 reference
(compact.topk_reference): exact indices on separated logits, probabilities within the float32 parity bound, ties by ascending index,
padding columns that take no part, the range, repeatability, independence of the batch size, and the refusals."""
import numpy as np
import pytest
import torch

from uvc_amd import _lib as L
from uvc_amd import compact as CP
from uvc_amd import ops

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-3, 1e-7                                           # the float32 parity bound plus an absolute floor
N_VALID = [1, 5, 10, 63, 64, 65, 1000, 1025]
WORST = {}


def separated_rows(B, n_valid, ld, seed):
    """float32 [B, ld]: each row's valid columns are a random permutation of a grid spanning [-15, 15] (spacing 30 / (n - 1) >= 1e-2 for
    n <= 3001), the padding columns hold values larger than every valid one."""
    rng = np.random.default_rng(seed)
    grid = np.linspace(-15.0, 15.0, n_valid) if n_valid > 1 else np.array([0.75])
    z = np.empty((B, ld), dtype=np.float32)
    for b in range(B):
        z[b, :n_valid] = rng.permutation(grid)
        z[b, n_valid:] = 40.0 + 10.0 * rng.random(ld - n_valid)
    return z


@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("n_valid", N_VALID)
def test_topk_against_float64(n_valid, k):
    k = min(k, n_valid)
    ld = 16 if n_valid == 10 else n_valid + 7
    z = separated_rows(70, n_valid, ld, seed=1000 * n_valid + k)
    # the separation condition, on the float32 inputs, in float64, for every row
    if n_valid > 1:
        gaps = np.diff(np.sort(z[:, :n_valid].astype(np.float64), axis=1), axis=1)
        assert gaps.shape == (70, n_valid - 1) and gaps.min() >= 1e-2
    assert (z[:, n_valid:] > z[:, :n_valid].max()).all() and ld > n_valid
    want_p, want_i = CP.topk_reference(z, k, n_valid)
    zd = torch.from_numpy(z).cuda()
    results = {}
    for B in (1, 3, 70):
        p, i = ops.logits_topk(zd[:B].contiguous(), k, n_valid)
        assert p.shape == i.shape == (B, k) and p.dtype == torch.float32 and i.dtype == torch.int32
        results[B] = (p.cpu(), i.cpu())
        assert np.array_equal(results[B][1].numpy(), want_i[:B]), B
        assert int(results[B][1].max()) < n_valid
        got = results[B][0].numpy().astype(np.float64)
        err = np.abs(got - want_p[:B])
        rel = float((err / want_p[:B]).max())
        WORST[(n_valid, k)] = max(WORST.get((n_valid, k), 0.0), rel)
        print(f"uvc_logits_topk n_valid={n_valid} k={k} B={B}: worst relative error {rel:.3e}")
        assert (err <= RTOL * want_p[:B] + ATOL).all(), (B, rel)
        assert (np.diff(got, axis=1) <= 0).all()
    # a row's result does not depend on B, and a repeat gives the same bits
    for B in (1, 3):
        assert torch.equal(results[B][0].view(torch.int32), results[70][0][:B].view(torch.int32)) and torch.equal(results[B][1], results[70][1][:B])
    p, i = ops.logits_topk(zd, k, n_valid)
    assert torch.equal(p.cpu().view(torch.int32), results[70][0].view(torch.int32)) and torch.equal(i.cpu(), results[70][1])
    print(f"uvc_logits_topk worst relative error so far: {max(WORST.values()):.3e}")


def test_ties_come_out_by_ascending_index():
    for n_valid, ld, k in ((1000, 1000, 16), (10, 16, 10), (65, 80, 5), (1, 3, 1)):
        z = torch.full((2, ld), 0.375, device="cuda")
        z[:, n_valid:] = 9.0
        p, i = ops.logits_topk(z, k, n_valid)
        assert i.cpu().tolist() == [list(range(k))] * 2
        assert np.allclose(p.cpu().numpy().astype(np.float64), 1.0 / n_valid, rtol=RTOL, atol=0)
    z = torch.zeros(3, 300, device="cuda")
    z[:, 7] = z[:, 3] = 2.0                                       # two equal maxima at 7 and 3: 3 first
    z[1, 299] = z[1, 256] = z[1, 255] = 2.0                       # and across the threads' strides and the waves
    p, i = ops.logits_topk(z, 6)
    assert i.cpu().tolist() == [[3, 7, 0, 1, 2, 4], [3, 7, 255, 256, 299, 0], [3, 7, 0, 1, 2, 4]]
    wp, wi = CP.topk_reference(z.cpu().numpy(), 6)
    assert np.array_equal(wi, i.cpu().numpy()) and np.allclose(p.cpu().numpy(), wp, rtol=RTOL, atol=ATOL)


def test_large_logits_stay_finite():
    z = torch.zeros(4, 24, device="cuda")
    z[0, 5], z[0, 9] = 80.0, -80.0
    z[1] = -80.0
    z[1, 2] = 80.0
    z[2] = 80.0
    z[3] = torch.linspace(-80, 80, 24)
    p, i = ops.logits_topk(z, 16, 20)
    assert torch.isfinite(p).all() and int(i.min()) >= 0 and int(i.max()) < 20
    wp, wi = CP.topk_reference(z.cpu().numpy(), 16, 20)
    assert np.array_equal(wi, i.cpu().numpy())
    assert (np.abs(p.cpu().numpy().astype(np.float64) - wp) <= RTOL * wp + ATOL).all()
    assert i[0, 0] == 5 and abs(float(p[0, 0]) - 1.0) < 1e-6 and i[1, 0] == 2


def test_refusals():
    z = torch.zeros(3, 24, device="cuda")
    for k, n_valid in ((0, 24), (17, 24), (6, 5), (1, 25), (1, 0), (-1, 24)):
        with pytest.raises(L.UvcHipError, match=r"rc=1"):
            ops.logits_topk(z, k, n_valid)
    with pytest.raises(L.UvcHipError):
        ops.logits_topk(z.double(), 1)
    with pytest.raises(L.UvcHipError):
        ops.logits_topk(torch.zeros(3, 24), 1)
    p, i = ops.logits_topk(z, 16, 16)
    assert i.cpu().tolist() == [list(range(16))] * 3
