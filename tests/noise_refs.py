"""The keyed Exp(1) generator of uvc_amd/csrc/elementwise.hip (uvc_exp_noise, k_exp_noise) restated on the host, bit for bit: numpy only, nothing
of uvc_amd.  Element i of the draw (seed, step, site):

    key = rotl17((seed * K0 + K1) ^ (step + 1) * GOLDEN) ^ (site + 1) * K2          (uint64, wrapping; site + 1 formed in 64 bits)
    h   = splitmix64(key ^ splitmix64(i))
    c   = h >> 40                                                                    (the 24-bit counter)
    u   = min(float32(float32(c) + 0.5f) * 2^-24, 1 - 2^-24)                         (float32 operations, in this order)
    E   = -log(u)

float32(c) + 0.5f is exact for c < 2^23; from 2^23 up it is no float32 and rounds to the even neighbour, so an odd c gives the u of c + 1: the
upper half of (0, 1) has 23-bit resolution.  For c = 2^24 - 1 that neighbour is 2^24 and the product 1.0f -- a draw of -0.0f, whose Gumbel value
-log(E) is +inf -- which the min() brings back to 1 - 2^-24, the largest u; it is the only c the min() changes (c = 2^24 - 2 gives 1 - 2^-23).
The multiplication by 2^-24 is exact, so the fused form fma(float32(c), 2^-24, 2^-25) a compiler may pick has the same single rounding."""
import numpy as np

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
K0, K1, K2 = 0xD1342543DE82EF95, 0x2545F4914F6CDD1D, 0xC2B2AE3D27D4EB4F
C_MAX = 0xFFFFFF
U_MAX = np.float32(1.0) - np.float32(2.0 ** -24)          # 0x3F7FFFFF, the u of c = 2^24 - 1 after the clamp
U_MIN = np.float32(2.0 ** -25)                            # the u of c = 0
E_MIN = float(-np.log(np.float64(U_MAX)))                 # smallest possible draw, 5.9604646e-08 (float32: 2^-24)
E_MAX = float(-np.log(np.float64(U_MIN)))                 # largest possible draw, 25 ln 2 = 17.3287


def splitmix64(x):
    """SplitMix64's output function of the state x (Steele, Lea, Flood 2014): a Python int, or a uint64 array (wrapping)."""
    if isinstance(x, np.ndarray):
        assert x.dtype == np.uint64
        x = x + np.uint64(GOLDEN)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))
    x = (int(x) + GOLDEN) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def key(seed, step, site):
    """The 64-bit key of a draw: seed and step are taken modulo 2^64, site is a uint32."""
    assert 0 <= int(site) < 1 << 32
    k = ((int(seed) & MASK) * K0 + K1) & MASK
    k ^= (((int(step) & MASK) + 1) * GOLDEN) & MASK
    k = ((k << 17) | (k >> 47)) & MASK
    return k ^ (((int(site) + 1) * K2) & MASK)


def _index_hash(n, start=0):
    return splitmix64(np.arange(start, start + n, dtype=np.uint64))


def counters(seed, step, site, n, start=0):
    """c = h >> 40 of elements start ... start + n - 1, uint32."""
    return (splitmix64(np.uint64(key(seed, step, site)) ^ _index_hash(n, start)) >> np.uint64(40)).astype(np.uint32)


def u_of_counter(c, clamp=True):
    """float32 u of counter values c, in the kernel's operation order; ``clamp=False`` is the formula before the fix (1.0f at c = 2^24 - 1)."""
    u = (np.asarray(c).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    assert u.dtype == np.float32
    return np.minimum(u, U_MAX) if clamp else u


def uniforms(seed, step, site, n, start=0, clamp=True):
    return u_of_counter(counters(seed, step, site, n, start), clamp)


def draws64(seed, step, site, n, start=0):
    """-log(u) in float64 of the float32 u."""
    return -np.log(uniforms(seed, step, site, n, start).astype(np.float64))


def find_counter(value, seed, n, max_steps, site=0):
    """Every (step, index) with step < max_steps, index < n at which the counter of the draw (seed, step, site) is ``value``, in order."""
    hi, v, out = _index_hash(n), np.uint64(value), []
    for step in range(max_steps):
        hit = np.nonzero((splitmix64(np.uint64(key(seed, step, site)) ^ hi) >> np.uint64(40)) == v)[0]
        out.extend((step, int(i)) for i in hit)
    return out


def ordinal(x):
    """float32 -> its position among the float32 values (sign-magnitude bits made monotone), int64."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def ordinal_distance(got32, ref64):
    """Number of float32 values between ``got32`` and the float32 nearest to ``ref64``, elementwise."""
    return np.abs(ordinal(got32) - ordinal(np.asarray(ref64, dtype=np.float64).astype(np.float32)))
