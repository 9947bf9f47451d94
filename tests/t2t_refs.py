"""Plain float64 references of the tokens-to-token kernels (include/uvc_t2t.h: soft split + LayerNorm forward / backward, fold, the Performer's
linear attention forward / backward), their input families and the acceptance rules.  Torch only, CPU-runnable (every function works on the
device of its operands), nothing from uvc_amd.  tests/test_t2t_refs_cpu.py shows that the rules accept an honest float32 kernel and reject
subtly wrong ones; tests/test_t2t_accuracy_gpu.py holds every kernel of uvc_amd/csrc/t2t.hip to them.

References, written out from the header's definitions (no autograd):
    unfold_rows   row b*L + ho*Wo + wo, feature c*k*k + ki*k + kj = source element b*sb + c*sc + (ho*s - p + ki)*sh + (wo*s - p + kj)*sw, or 0
                  where the tap lies in the padding; any element strides, any H != W; Ho = (H + 2p - k) / s + 1.
    LayerNorm     layernorm_refs.fwd_reference / bwd_reference on the unfolded rows with the fused kernel's summation depth h = NV + 6 (a lane
                  sums its NV = 3 or 9 elements, then six tree levels); the backward from the float32 mean / rstd HANDED TO the kernel;
                  dgamma / dbeta inside the any-order bound 2 (n + 4) u S of that module.
    fold          dst[b, h*W + w, c] = sum over (ki, kj) with (h + p - ki) % s == 0, ho = (h + p - ki) / s in [0, Ho) (and the same in w) of
                  src[b*L + ho*Wo + wo, c*k*k + ki*k + kj]  (tap_major: column (ki*k + kj)*C + c).
    Performer     kp = exp(w k - |k|^2 / 2) / sqrt(32), qp likewise; kptv[n, m] = sum_t v[t, n] kp[t, m]; ksum[m] = sum_t kp[t, m];
                  num = qp kptv^T; den = qp . ksum + 1e-8; att = num / den.
                  Backward:  dnum = datt / den;  dden = -sum_n datt num / den^2;  dkptv[n, m] = sum_t dnum[t, n] qp[t, m];
                  dksum[m] = sum_t dden[t] qp[t, m];  dqp = dnum kptv + dden ksum;  gq = dqp qp;  dq = gq w - q sum_m gq;
                  dv = kp dkptv^T + dskip;  dkp = v dkptv + dksum;  gk = dkp kp;  dk = gk w - k sum_m gk;  dkqv = dk | dq | dv.

Families.
  RANDOM  N(0, 1) sources and gradients.
  EDGE    the rows of layernorm_refs.make_x(EDGE) (big mean, tiny variance, constants, zero, spike, 1e15, ...) written INTO THE SOURCE through the
          unfold index map.  Only for geometries with s >= k, whose windows are disjoint: every source element belongs to at most one row, so the
          unfolded rows are the EDGE rows, except that taps in the padding read 0 (with p > 0 a border row is its EDGE row with zeros in it; with
          p >= k some rows are all zero).  Elements no window covers (s > k) are N(0, 1).  Geometries with s < k run RANDOM only.
  INTEGER, bit for bit:
      plain soft split   any input: float32 output == the gather, bf16 output == one round-to-nearest-even of it, columns [dim, ldo) == 0.
      fold               sources of integers in [-8, 8] (exact in bf16): every sum exact in any order; natural == tap-major == float64.
      LayerNorm backward layernorm_refs.make_bwd(INTEGER) mapped onto the unfolded rows of an s >= k geometry: mean (an integer) and rstd = 0.5
                         handed in; columns c and c + dim/2 carry equal xh and gamma and opposite dy.  Where a tap of a pair lies in the padding
                         the dy of BOTH columns is 0, so the row sums of gy and gy xh stay exactly 0 and dxu = 0.5 gy, dgamma, dbeta are exact
                         while every accumulator stays below 2^24 quanta (integer_magnitudes of layernorm_refs, asserted per case on the CPU).
      INTSUM             any geometry (the multi-trip ones, s < k): an integer source in [-4, 4], integer mean, rstd = 0.5, integer dy in
                         [-3, 3], gamma in {1, 2}: xh is a multiple of 1/2, so dgamma and dbeta are exact in any order and compared with
                         torch.equal (dropped rows, trips and blocks); c1 / c2 are not 0, so dxu is held to the RANDOM bound.
  Performer SPIKE  RANDOM with one token whose v (forward) and datt / dskip (backward) are 1000 times larger; the token walks through
                   SPIKE_AT = 0, 15, 16, 63, 64, 447, 448, T - 1.  Dropping or double-counting it moves kptv / dkptv by ~1 / (2 (T + 4) u) bounds.
  Performer RANGE  k and q rows scaled so that the exponent w x - |x|^2 / 2 spans about [-80, +20] (rows along a row of w reach |w_m|^2 / 2, long
                   rows reach -|x|^2 / 2), every reference value and the kernels' den^2 finite in float32 (asserted on the CPU); the LAST image keeps its RANDOM q and has its k
                   scaled until its largest qp . ksum is 5e-7, so the + 1e-8 of the denominator is 2 % or more of it.  B >= 2.

Performer rules, first order in u = 2^-24 with the factor 2 of tests/gemm_refs.py in every sum.  Every quantity carries (value, E):
    exact inputs E = 0;   a b: |a| E_b + |b| E_a + u |a b|;   a + b: E_a + E_b + u |a + b|;   a / b: E_a / |b| + |a / b| E_b / |b| + 2 u |a / b|;
    sum of n products a_i b_i: sum (|a_i| E_b + |b_i| E_a) + 2 (n + 4) u sum |a_i b_i|      (any order; n = T over tokens, 32 over features, 64)
    z = w x - |x|^2 / 2:  E_z = 2 (64 + 3) u (sum_i |w_i x_i| + |x|^2 / 2)
    p = exp(z) / sqrt(32): E_p = p (E_z + (2 X + 2) u),   X = EXPF_ULP ulps of the device expf (1 ulp = 2 u), 2 u for the division.
    every product and quotient (n of them in a sum of n products) also carries 2^-126: a float32 result below the smallest normal number may be
    flushed to zero.  It matters in the RANGE family alone, where exp(-80) / sqrt(32) = 3e-36 meets small gradients.
att and the gradients combine these through the formulas above; a bf16 output is bracketed by round_T(ref -+ E) (layernorm_refs.band).
ASSUMPTION: X = 4.  No document available to this project states the error of HIP's expf on gfx950, so 4 ulp is allowed; the GPU module's last
test reports the measured worst ratios.  The constants were fixed on the CPU simulation of tests/test_t2t_refs_cpu.py and are never changed
from a GPU result."""
from __future__ import annotations

import math

import torch

import layernorm_refs as LR

U = LR.U
LN_EPS = 1e-5
RANDOM, EDGE, INTEGER, INTSUM, SPIKE, RANGE = "random", "edge", "integer", "intsum", "spike", "range"
EXPF_ULP = 4.0
TINY = 2.0 ** -126                                # a float32 product or quotient below the smallest normal number may be flushed to 0
SPIKE_AT = (0, 15, 16, 63, 64, 447, 448, -1)       # -1: T - 1
SPIKE_GAIN = 1000.0
PT, PTPS, PM, PE = 64, 7, 32, 64                   # tokens per tile, tiles per split, random features, token width
SENTINEL, GUARD_ROWS = LR.SENTINEL, LR.GUARD_ROWS
round_to, band = LR.round_to, LR.band


def _gen(*key):
    s = 7
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 61)
    return torch.Generator().manual_seed(s)


# ----------------------------------------------------------------------------- geometry
def geometry(B, C, H, W, k, s, p, token_major):
    """Everything the kernels derive from (B, C, H, W, k, s, p) and the source layout, recomputed here from the header's text."""
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dim = C * k * k
    strides = (H * W * C, 1, W * C, C) if token_major else (C * H * W, H * W, W, 1)
    g = dict(B=B, C=C, H=H, W=W, k=k, s=s, p=p, tm=bool(token_major), Ho=Ho, Wo=Wo, L=Ho * Wo, kk=k * k, dim=dim, rows=B * Ho * Wo, strides=strides)
    g["nv"] = 3 if -(-dim // 64) <= 3 else 9
    g["c_fast"] = bool(token_major and C == 64)
    g["disjoint"] = s >= k
    return g


def with_batch(g, B):
    return geometry(B, g["C"], g["H"], g["W"], g["k"], g["s"], g["p"], g["tm"])


def ldo_choices(dim):
    """The output strides uvc_unfold_args admits at their limits: dim itself (where 8 divides it), roundup(dim, 32), roundup(dim, 64)."""
    out = [dim] if dim % 8 == 0 else []
    for m in (32, 64):
        r = -(-dim // m) * m
        if r not in out:
            out.append(r)
    return out


def fwd_trips(g):
    """Grid-stride trips of k_unfold_ln: grid = min(ceil(rows / 8), 16384) workgroups of 16 (NV 3) or 8 (NV 9) rows per trip."""
    per = 16 if g["nv"] == 3 else 8
    grid = min(-(-g["rows"] // 8), 16384)
    return -(-g["rows"] // (grid * per)), grid, per


def bwd_blocks(rows):
    return min(-(-rows // 4), 1024)


def bwd_trips(g):
    per = 16 if g["nv"] == 3 else 8
    grid = bwd_blocks(g["rows"])
    return -(-g["rows"] // (grid * per)), grid, per


def performer_splits(T):
    return -(-(-(-T // PT)) // PTPS)


def unfold_index(g, rows=None, strides=None, device="cpu"):
    """(offset [n, dim] int64 into the flat source, valid [n, dim] bool) of the unfolded rows `rows` (default: all)."""
    sb, sc, sh, sw = strides or g["strides"]
    r = torch.arange(g["rows"], device=device) if rows is None else rows.to(device)
    b, l = r // g["L"], r % g["L"]
    ho, wo = l // g["Wo"], l % g["Wo"]
    e = torch.arange(g["dim"], device=device)
    c, t = e // g["kk"], e % g["kk"]
    ki, kj = t // g["k"], t % g["k"]
    hi = (ho * g["s"] - g["p"])[:, None] + ki[None, :]
    wi = (wo * g["s"] - g["p"])[:, None] + kj[None, :]
    valid = (hi >= 0) & (hi < g["H"]) & (wi >= 0) & (wi < g["W"])
    off = b[:, None] * sb + c[None, :] * sc + hi * sh + wi * sw
    return torch.where(valid, off, torch.zeros_like(off)), valid


def unfold_rows(src, g, rows=None, strides=None):
    """The [n, dim] gather of the soft split from the flat source storage `src` (its dtype is kept: the gather is exact)."""
    off, valid = unfold_index(g, rows, strides, src.device)
    flat = src.reshape(-1)
    return torch.where(valid, flat[off], torch.zeros((), dtype=flat.dtype, device=flat.device))


def source_numel(g):
    return g["B"] * g["C"] * g["H"] * g["W"]


def scatter_rows(g, rows_t, base):
    """A flat source whose unfolded rows are `rows_t` ([rows, dim]) wherever the tap is inside the image (s >= k: windows are disjoint);
    elements outside every window keep `base`."""
    assert g["disjoint"]
    off, valid = unfold_index(g)
    src = base.clone().reshape(-1)
    src[off[valid]] = rows_t[valid]
    return src


def make_unfold_fwd(g, family, seed=0):
    """(flat float32 source, gamma, beta)."""
    gen = _gen(seed, g["rows"], g["dim"], 1)
    src = torch.randn(source_numel(g), generator=gen)
    if family == EDGE:
        src = scatter_rows(g, LR.make_x(EDGE, g["rows"], g["dim"], seed), src)
    else:
        assert family == RANDOM
    gamma, beta = LR.make_params(g["dim"], seed)
    return src, gamma, beta


def make_unfold_bwd(g, family, seed=0):
    """dict(src flat float32, dy [rows, dim] (bf16-exact for INTEGER / INTSUM), gamma, dg_old, db_old, and for INTEGER / INTSUM mean / rstd)."""
    rows, dim = g["rows"], g["dim"]
    gen = _gen(seed, rows, dim, 2)
    o = dict(family=family, rows=rows, D=dim)
    if family in (RANDOM, EDGE):
        o["src"] = make_unfold_fwd(g, family, seed)[0]
        o["gamma"] = LR.make_params(dim, seed)[0]
        o["dy"] = torch.randn(rows, dim, generator=gen)
        o["dg_old"], o["db_old"] = torch.randn(dim, generator=gen), torch.randn(dim, generator=gen)
        return o
    o["dg_old"] = torch.randint(-64, 65, (dim,), generator=gen).float()
    o["db_old"] = torch.randint(-64, 65, (dim,), generator=gen).float()
    o["rstd"] = torch.full((rows,), 0.5)
    if family == INTSUM:
        o["src"] = torch.randint(-4, 5, (source_numel(g),), generator=gen).float()
        o["mean"] = torch.randint(-3, 4, (rows,), generator=gen).float()
        o["dy"] = torch.randint(-3, 4, (rows, dim), generator=gen).float()
        o["gamma"] = torch.randint(1, 3, (dim,), generator=gen).float()
        return o
    assert family == INTEGER and g["disjoint"]
    i = LR.make_bwd(LR.INTEGER, rows, dim, seed)
    _, valid = unfold_index(g)
    half = dim // 2
    both = valid.clone()
    both[:, :half] &= valid[:, half:2 * half]
    both[:, half:2 * half] &= valid[:, :half]
    o["dy"] = torch.where(both, i["dy"], torch.zeros(()))
    o["src"] = scatter_rows(g, i["x"], torch.randint(-4, 5, (source_numel(g),), generator=gen).float())
    o["mean"], o["gamma"] = i["mean"], i["gamma"]
    return o


def integer_magnitudes(g, o, beta_acc):
    """layernorm_refs.integer_magnitudes of an INTEGER case on its unfolded rows (asserts c1 = c2 = 0); `dots` does not exist here."""
    x = unfold_rows(o["src"], g)
    m = LR.integer_magnitudes(dict(o, x=x, add1=None, add2=None, a1=1.0, a2=1.0), add1=False, add2=False, scalars=False, beta_acc=beta_acc)
    m.pop("dots")
    return m


def intsum_magnitudes(g, o, beta_acc):
    """sum |terms| / quantum (1/2) of the dgamma / dbeta accumulators of an INTSUM case."""
    xh = (unfold_rows(o["src"], g).double() - o["mean"].double()[:, None]) * 0.5
    dy = o["dy"].double()
    return dict(dgamma=float(((dy * xh).abs().sum(0) + abs(beta_acc) * o["dg_old"].double().abs()).max()) / 0.5,
                dbeta=float((dy.abs().sum(0) + abs(beta_acc) * o["db_old"].double().abs()).max()) / 0.5)


def ln_fwd_reference(x_rows, gamma, beta, nv, eps=LN_EPS):
    return LR.fwd_reference(x_rows, gamma, beta, eps, h=nv + 6)


def ln_bwd_reference(x_rows, dy, gamma, mean, rstd, nv, beta_acc, dg_old, db_old):
    return LR.bwd_reference(x_rows, dy, gamma, mean, rstd, beta_acc=beta_acc, dg_old=dg_old, db_old=db_old, h=nv + 6)


def to_tap_major(t, g):
    """[n, C*kk] natural columns -> [n, kk*C] tap-major."""
    n = t.shape[0]
    return t.reshape(n, g["C"], g["kk"]).transpose(1, 2).reshape(n, g["dim"])


# ----------------------------------------------------------------------------- fold
def fold(src, g, tap_major=False):
    """float64 [B, H*W, C] from src [B*L, >= dim] (the gather form of the header)."""
    B, C, H, W, k, s, p, Ho, Wo, L, kk = (g[n] for n in ("B", "C", "H", "W", "k", "s", "p", "Ho", "Wo", "L", "kk"))
    src = src.double()
    dst = torch.zeros(B, H, W, C, dtype=torch.float64, device=src.device)
    h, w, c = torch.arange(H, device=src.device), torch.arange(W, device=src.device), torch.arange(C, device=src.device)
    for ki in range(k):
        hh = h + p - ki
        okh = (hh >= 0) & (hh % s == 0) & (hh // s < Ho)
        for kj in range(k):
            ww = w + p - kj
            okw = (ww >= 0) & (ww % s == 0) & (ww // s < Wo)
            if not (bool(okh.any()) and bool(okw.any())):
                continue
            row = (hh[okh] // s)[:, None] * Wo + (ww[okw] // s)[None, :]                          # [h', w']
            col = (ki * k + kj) * C + c if tap_major else c * kk + ki * k + kj
            for b in range(B):
                blk = src[b * L + row][:, :, col]                                                  # [h', w', C]
                hi, wi = okh.nonzero().reshape(-1), okw.nonzero().reshape(-1)
                dst[b, hi[:, None], wi[None, :]] += blk
    return dst.reshape(B, H * W, C)


# ----------------------------------------------------------------------------- Performer
class Q:
    """A float64 value with its first-order absolute error bound."""

    def __init__(self, v, e=None):
        self.v, self.e = v, (torch.zeros_like(v) if e is None else e)

    def __getitem__(self, i):
        return Q(self.v[i], self.e[i])

    def __neg__(self):
        return Q(-self.v, self.e)


def q_mul(a, b):
    v = a.v * b.v
    return Q(v, a.v.abs() * b.e + b.v.abs() * a.e + U * v.abs() + TINY)


def q_add(a, b):
    v = a.v + b.v
    return Q(v, a.e + b.e + U * v.abs())


def q_div(a, b):
    v = a.v / b.v
    return Q(v, a.e / b.v.abs() + v.abs() * b.e / b.v.abs() + 2.0 * U * v.abs() + TINY)


def q_dot(eq, a, b, n):
    v, m = torch.einsum(eq, a.v, b.v), torch.einsum(eq, a.v.abs(), b.v.abs())
    return Q(v, torch.einsum(eq, a.v.abs(), b.e) + torch.einsum(eq, a.e, b.v.abs()) + 2.0 * (n + 4) * U * m + n * TINY)


def q_sum(a, dim, n):
    return Q(a.v.sum(dim), a.e.sum(dim) + 2.0 * (n + 4) * U * a.v.abs().sum(dim))


def prm(x, w):
    """(Q of exp(w x - |x|^2 / 2) / sqrt(32) [B, T, 32], the exponent z)."""
    xx = (x * x).sum(-1, keepdim=True) / 2
    z = torch.einsum("bti,mi->btm", x, w) - xx
    Ez = 2.0 * (64 + 3) * U * (torch.einsum("bti,mi->btm", x.abs(), w.abs()) + xx)
    p = torch.exp(z) / math.sqrt(PM)
    return Q(p, p * (Ez + (2.0 * EXPF_ULP + 2.0) * U) + TINY), z


def performer_reference(kqv, w, datt=None, dskip=None):
    """kqv [B, T, 192], w [32, 64], datt / dskip [B, T, 64] as the kernel receives them (any float type).  dict of Q: kptv [B, 65, 32] (row 64 =
    ksum), att [B, T, 64], and with datt: dkptv [B, 65, 32] (row 64 = dksum), dkqv [B, T, 192]; plus z (both exponents) and every intermediate."""
    kqv, w = kqv.double(), w.double()
    B, T, _ = kqv.shape
    k, q, v = (Q(t) for t in torch.split(kqv, PE, dim=-1))
    kp, zk = prm(k.v, w)
    qp, zq = prm(q.v, w)
    kptv = q_dot("btn,btm->bnm", v, kp, T)
    ksum = q_sum(kp, 1, T)
    den = q_dot("btm,bm->bt", qp, ksum, PM)
    den = Q(den.v + 1e-8, den.e + U * (den.v + 1e-8))
    num = q_dot("btm,bnm->btn", qp, kptv, PM)
    den1 = Q(den.v[..., None], den.e[..., None])
    att = q_div(num, den1)
    out = dict(kptv=Q(torch.cat([kptv.v, ksum.v[:, None]], 1), torch.cat([kptv.e, ksum.e[:, None]], 1)), att=att, z=torch.cat([zk, zq], -1), den=den, num=num,
               kp=kp, qp=qp)
    if datt is None:
        return out
    dy = Q(datt.double())
    dnum = q_div(dy, den1)
    dot = q_dot("btn,btn->bt", dy, num, PE)
    dden = -q_div(q_div(dot, den), den)
    dkptv = q_dot("btn,btm->bnm", dnum, qp, T)
    dksum = q_dot("bt,btm->bm", dden, qp, T)
    dden1 = Q(dden.v[..., None], dden.e[..., None])
    dqp = q_add(q_dot("btn,bnm->btm", dnum, kptv, PE), q_mul(dden1, Q(ksum.v[:, None], ksum.e[:, None])))
    wq = Q(w)

    def prm_bwd(g, x):
        gs = q_sum(g, -1, PM)
        return q_add(q_dot("btm,md->btd", g, wq, PM), -q_mul(x, Q(gs.v[..., None], gs.e[..., None])))

    dq = prm_bwd(q_mul(dqp, qp), q)
    dv = q_dot("btm,bnm->btn", kp, dkptv, PM)
    if dskip is not None:
        dv = q_add(dv, Q(dskip.double()))
    dkp = q_add(q_dot("btn,bnm->btm", v, dkptv, PE), Q(dksum.v[:, None], dksum.e[:, None]))
    dk = prm_bwd(q_mul(dkp, kp), k)
    out.update(dkptv=Q(torch.cat([dkptv.v, dksum.v[:, None]], 1), torch.cat([dkptv.e, dksum.e[:, None]], 1)),
               dkqv=Q(torch.cat([dk.v, dq.v, dv.v], -1), torch.cat([dk.e, dq.e, dv.e], -1)), dnum=dnum, dden=dden, dqp=dqp, dkp=dkp)
    return out


def spike_positions(T):
    return sorted({(T - 1 if p < 0 else p) for p in SPIKE_AT if p < T})


def make_performer(family, B, T, seed=0, spike=None):
    """dict(kqv [B, T, 192], w [32, 64], datt, dskip [B, T, 64]) float32 host tensors.  SPIKE: token `spike` of image B - 1."""
    gen = _gen(seed, B, T, 3)
    kqv = torch.randn(B, T, 192, generator=gen) * 0.5
    w = torch.randn(PM, PE, generator=gen) * 0.7
    datt, dskip = torch.randn(B, T, PE, generator=gen), torch.randn(B, T, PE, generator=gen)
    if family == SPIKE:
        kqv[B - 1, spike, 128:] *= SPIKE_GAIN
        datt[B - 1, spike] *= SPIKE_GAIN
        dskip[B - 1, spike] *= SPIKE_GAIN
    elif family == RANGE:
        assert B >= 2
        w = torch.randn(PM, PE, generator=gen)
        w = w * (math.sqrt(40.0) / w.norm(dim=1, keepdim=True))             # |w_m|^2 / 2 = 20: the exponent of a row x = w_m at feature m
        t = torch.arange(T)
        for col in (0, 64):                                                # k, then q of every image but the last
            x = torch.randn(B - 1, T, PE, generator=gen) * (1.3 * (t % 17).float() / 16.0)[None, :, None]    # |x|^2 / 2 up to ~80
            along = (t % 5 == 2) if col == 0 else (t % 5 == 4)
            x[:, along] = w[(t[along] // 5) % PM][None].expand(B - 1, -1, -1)                                   # exponent |w_m|^2 / 2 at feature m
            kqv[:B - 1, :, col:col + PE] = x
        k0 = torch.randn(1, T, PE, generator=gen).double()

        def max_den(a):
            kq = kqv[B - 1:].double()
            kq[:, :, :PE] = k0 * a
            return float((performer_reference(kq, w)["den"].v - 1e-8).max()), kq
        lo, hi = 0.5, 40.0                                                 # a larger |k| shrinks every kp: bisect the scale to max qp . ksum = 5e-7
        for _ in range(50):
            mid = 0.5 * (lo + hi)
            if max_den(mid)[0] > 5e-7:
                lo = mid
            else:
                hi = mid
        kqv[B - 1, :, :PE] = max_den(hi)[1][0, :, :PE].float()
    else:
        assert family == RANDOM
    return dict(kqv=kqv, w=w, datt=datt, dskip=dskip)


def accept(name, got, ref, fails, ratios, exact=False):
    """One output against a Q (or, exact, against a float64 tensor bit for bit after one rounding to got's type)."""
    if not bool(torch.isfinite(got.double()).all()):
        fails.append(f"{name}: {int((~torch.isfinite(got.double())).sum())} elements not written or not finite")
        return
    if exact:
        want = round_to(ref, got.dtype)
        LR._report(name + " [exact]", got == want, float((got.double() - want.double()).abs().max()), got, ref, fails, ratios)
    else:
        LR._report(name, *band(got, ref.v, ref.e), got, ref.v, fails, ratios)
