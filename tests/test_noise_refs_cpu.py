"""CPU: tests/noise_refs.py on its own -- the host restatement of the keyed Exp(1) generator that tests/test_gating_noise_gpu.py holds
uvc_exp_noise to.  The published SplitMix64 vectors, the key schedule, the search for the two extreme counters (asserted non-empty, so the GPU
tests that take their positions from it can never run on nothing) and the formula before the fix, which gives u = 1.0f at c = 2^24 - 1."""
import math

import numpy as np

import noise_refs as N


def test_splitmix64_published_vectors():
    """The first two outputs of a SplitMix64 stream seeded with 0: the state advances by the golden-ratio increment before each output."""
    assert N.splitmix64(0) == 0xE220A8397B1DCDAF
    assert N.splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    a = N.splitmix64(np.array([0, 0x9E3779B97F4A7C15, N.MASK], dtype=np.uint64))
    assert a.dtype == np.uint64 and [int(v) for v in a] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, N.splitmix64(N.MASK)]


def test_key_is_injective_over_a_small_grid_and_wraps():
    grid = [(s, t, u) for s in (0, 1, 2, 730, 731, N.MASK) for t in (0, 1, 2, 107, 108, (1 << 63) - 1, 1 << 63, N.MASK)
            for u in (0, 1, 2, 3, (1 << 32) - 1)]
    keys = [N.key(*g) for g in grid]
    assert len(set(keys)) == len(grid) and all(0 <= k <= N.MASK for k in keys)
    assert N.key(1 << 64, 0, 0) == N.key(0, 0, 0) and N.key(0, 1 << 64, 0) == N.key(0, 0, 0)      # seed and step are 64-bit
    assert N.key(0, N.MASK, 0) == N.key(0, -1, 0)                                                 # step + 1 wraps to 0
    assert N.key(0, 0, (1 << 32) - 1) != N.key(0, 0, 0)                                           # site + 1 does not: it is formed in 64 bits


def test_counters_are_24_bit_prefix_stable_and_offset_stable():
    c = N.counters(730, 7, 3, 1000)
    assert c.dtype == np.uint32 and int(c.max()) <= N.C_MAX
    assert np.array_equal(N.counters(730, 7, 3, 100), c[:100]) and np.array_equal(N.counters(730, 7, 3, 100, start=900), c[900:])
    assert not np.array_equal(N.counters(730, 8, 3, 1000), c) and not np.array_equal(N.counters(730, 7, 4, 1000), c)


def test_the_extreme_counters_are_found():
    top = N.find_counter(N.C_MAX, 730, 65536, 2000)
    assert (108, 45643) in top and {(788, 63722), (789, 16288), (903, 3793)} <= set(top)
    assert all(int(N.counters(730, s, 0, 1, start=i)[0]) == N.C_MAX for s, i in top)
    # a key at the end of every field has one too: the GPU comparison with the restatement meets the top counter on its own
    assert np.nonzero(N.counters(N.MASK, 0, (1 << 32) - 1, 65536) == N.C_MAX)[0].tolist() == [34993]
    zero = N.find_counter(0, 730, 65536, 2000)
    assert len(zero) >= 1
    assert all(int(N.counters(730, s, 0, 1, start=i)[0]) == 0 for s, i in zero)


def test_the_unfixed_formula_draws_zero_at_the_top_counter():
    """(float32(2^24 - 1) + 0.5f) * 2^-24 == 1.0f, with separate roundings and fused: the draw was -0.0f and its Gumbel value +inf."""
    assert (np.float32(16777215) + np.float32(0.5)) * np.float32(2.0 ** -24) == np.float32(1.0)
    assert np.float32(16777215.0 * 2.0 ** -24 + 2.0 ** -25) == np.float32(1.0)                    # fma(c, 2^-24, 2^-25): one rounding of the exact value
    u = N.u_of_counter(np.array([N.C_MAX]), clamp=False)
    assert u.dtype == np.float32 and u[0] == np.float32(1.0)
    e = -np.log(u)
    assert e[0] == 0.0 and np.signbit(e[0])
    with np.errstate(divide="ignore"):
        assert np.isinf(-np.log(e.astype(np.float64) + 0.0)[0])


def test_the_fix_moves_one_counter_only():
    edge = np.array([0, 1, 2, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, (1 << 23) + 2, N.C_MAX - 3, N.C_MAX - 2, N.C_MAX - 1, N.C_MAX])
    rs = np.random.RandomState(5)
    c = np.concatenate([edge, rs.randint(0, 1 << 24, size=200000)])
    fixed, old = N.u_of_counter(c), N.u_of_counter(c, clamp=False)
    assert np.array_equal(fixed[c != N.C_MAX], old[c != N.C_MAX]) and bool((fixed[c == N.C_MAX] == N.U_MAX).all())
    assert float(fixed.max()) < 1.0 and float(fixed.min()) == 2.0 ** -25 and N.U_MAX.view(np.uint32) == 0x3F7FFFFF
    assert N.u_of_counter(np.array([N.C_MAX - 1]))[0] == np.float32(1.0 - 2.0 ** -23)             # the next counter down was never near the clamp
    # 23-bit resolution from 2^23 up: an odd counter shares the u of the even one above it (ties to even); below, every counter has its own
    hi = np.arange((1 << 23) + 1, (1 << 23) + 2001, 2)
    assert np.array_equal(N.u_of_counter(hi), N.u_of_counter(hi + 1))
    lo = np.arange((1 << 23) - 2000, 1 << 23)
    assert len(np.unique(N.u_of_counter(lo))) == len(lo)
    # the fused form is the same single rounding for every counter
    fused = (c.astype(np.float64) * 2.0 ** -24 + 2.0 ** -25).astype(np.float32)
    assert np.array_equal(fused, old)


def test_extreme_draws():
    assert N.E_MAX == 25 * math.log(2) and abs(N.E_MAX - 17.3287) < 1e-4
    assert abs(N.E_MIN - 2.0 ** -24 * (1 + 2.0 ** -25)) < 1e-22 and np.float32(N.E_MIN) == np.float32(2.0 ** -24)
    assert abs(-math.log(N.E_MIN) - 16.6355) < 1e-4 and abs(-math.log(N.E_MAX) + 2.8523) < 1e-4   # their Gumbel values: both finite
    s, i = N.find_counter(N.C_MAX, 730, 65536, 109)[0]
    assert (s, i) == (108, 45643) and N.draws64(730, s, 0, 1, start=i)[0] == N.E_MIN
    d = N.draws64(730, 108, 0, 65536)
    assert d.dtype == np.float64 and d.min() == N.E_MIN and d[45643] == N.E_MIN and d.max() <= N.E_MAX


def test_ordinal_distance():
    a = np.array([1.0, 1.0, 2.0 ** -24, 0.0, -0.0, 17.3287], dtype=np.float32)
    b = np.array([np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(1), np.float32(0)), 2.0 ** -24, -0.0, 0.0, 17.3287],
                 dtype=np.float32)
    assert N.ordinal_distance(a, b.astype(np.float64)).tolist() == [1, 1, 0, 0, 0, 0]
    assert N.ordinal_distance(np.float32([1.0]), np.float64([1.0 + 2.0 ** -25]))[0] == 0           # the float64 reference is rounded first
