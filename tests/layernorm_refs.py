"""Plain float64 references of uvc_layernorm_fwd / uvc_layernorm_bwd (include/uvc_kernels.h), three seeded row families and the acceptance
rules that hold a kernel to them.  Torch only, CPU-runnable (every function works on the device of its operands), nothing from uvc_amd;
tests/test_layernorm_refs_cpu.py shows that the rules accept an honest float32 kernel and reject subtly wrong ones,
tests/test_layernorm_accuracy_gpu.py holds every kernel of layernorm.hip (and the fused kernels that compute the same statistics) to them.

Forward reference: y, mean, var (biased), rstd = (var + eps)^-1/2 from x AS THE KERNEL RECEIVES IT (a bf16 x is exact in float64).
Backward reference: from the float32 mean / rstd HANDED TO the kernel, not recomputed, so the backward is judged on its own arithmetic:
xh = (x - mean) rstd, gy = dy gamma, c1 = mean_c(gy), c2 = mean_c(gy xh),
    dx = rstd (gy - c1 - xh c2) + a1 add1 + a2 add2,   dgamma = sum_r dy xh + beta_acc old,   dbeta = sum_r dy + beta_acc old,
    dots = (sum dx x, sum add2 x) from the UNROUNDED dx.

Row families.  RANDOM: N(0.5, 2).  EDGE: one tensor whose row i is of kind EDGE_KINDS[i % 10] -- 1e4 + N(0, 1); 3 + 1e-4 N(0, 1); constant 1000;
constant pi; all zero; one spike of 100 in a zero row; 1e15 N(0, 1); a copy of the row above; a bf16-exact row; a RANDOM row.  INTEGER (backward
only): the test supplies mean = a small integer per row and rstd = 0.5; x - mean in {+-1, +-2}, dy in {+-1, +-2, +-3}, gamma in {1, 2}; columns
c and c + floor(D / 2) carry equal xh and gamma and opposite dy (an odd width leaves its last column with dy = 0), so the row sums of gy and
gy xh are exactly 0 in any order and dx = 0.5 gy + a1 add1 + a2 add2; add1 / add2 integers in [-8, 8] with a1 = 0.5, a2 = 0.25 (or null = 1),
the old dgamma / dbeta integers, beta_acc in {0, 1, 0.5}.  Every value is a multiple of 1/4 below 64 (exact in bf16 too) and every product
and sum is exact in float32 in any order as long as every accumulator stays below 2^24 quanta: ``integer_magnitudes`` returns sum |terms| /
quantum per accumulator, the CPU test asserts < 2^24 for every GPU case that claims exactness (a case whose `dots` would exceed it holds `dots`
to the RANDOM rule instead).  The rule is torch.equal on dx (after ONE rounding to bf16 for a bf16 gradient stream), dgamma, dbeta and dots.

Acceptance rules for RANDOM and EDGE, u = 2^-24, h = D / 16 + 6.  ASSUMPTION: h is the deepest chain of float32 additions any layout of
layernorm.hip needs -- no lane sums more than D / 16 elements before the wave tree of at most 6 levels (16 lanes x D / 16 elements at the
vector widths up to 192; the generic kernel: 64 lanes x ceil(D / 64) <= 16 elements).  First order, with a factor 2 for the higher-order terms
as in tests/gemm_refs.py:
    E_mean = 2 h u mean_c|x|
    rho    = (E_mean^2 + 2 (h + 3) u var) / (2 (var + eps)) + 4 u         (4 u: the reciprocal square root and the 1 / D factor)
    |mean - ref| <= E_mean + u |ref|,      |rstd / ref - 1| <= rho
    E_y    = |gamma| (|xh| rho + rstd (E_mean + u |mean| + u |x - mean|)) + 4 u (|gamma xh| + |beta|)
    round_T(ref - E_y) <= y <= round_T(ref + E_y)        for the output type T
    E_c1 = 2 h u mean_c|gy|,   E_c2 = 2 h u mean_c|gy xh| + 2 u |c2|
    E_dx = rstd (E_c1 + |xh| E_c2) + 6 u T,   T = sum of the magnitudes of the five terms of dx;   round_T(ref -+ E_dx) brackets dx
    dgamma, dbeta, dots: the any-order bound 2 (n + 4) u S, n the number of terms (rows, or rows D for dots), S the float64 sum of their
    magnitudes plus |beta_acc old|.  Loose by design: dropped rows, blocks and columns are the INTEGER family's job.
The constants were fixed on the CPU simulation of tests/test_layernorm_refs_cpu.py (which prints the worst honest ratio per family and the
smallest ratio of every mutant) and are never changed from a GPU result."""
from __future__ import annotations

import math

import torch

U = 2.0 ** -24
EPS = 1e-6
RANDOM, EDGE, INTEGER = "random", "edge", "integer"
EDGE_KINDS = ("big_mean", "tiny_var", "const_1000", "const_pi", "zero", "spike", "huge", "neighbour", "bf16_exact", "random")
SENTINEL = -7.0
GUARD_ROWS = 8
A1, A2 = 0.5, 0.25                   # INTEGER family's scalars


def h_of(D):
    return D / 16.0 + 6.0


def round_to(t, dtype):
    """float64 -> dtype (float32, or bf16 through float32 as the kernels hold their values)."""
    return t.to(torch.float32).to(dtype)


def _gen(seed, *key):
    s = 1000003 * seed
    for k in key:
        s = s * 31 + int(k)
    return torch.Generator().manual_seed(s % (2 ** 62))


def make_x(family, rows, D, seed=0):
    """[rows, D] float32 host rows of the RANDOM or EDGE family (not yet rounded to a bf16 stream's type)."""
    g = _gen(seed, rows, D, 1 if family == EDGE else 0)
    x = torch.randn(rows, D, generator=g) * 2.0 + 0.5
    if family == RANDOM:
        return x
    assert family == EDGE
    n = torch.randn(rows, D, generator=g)
    spike_at = torch.randint(0, D, (rows,), generator=g)
    kind = torch.arange(rows) % len(EDGE_KINDS)
    k = {name: kind == i for i, name in enumerate(EDGE_KINDS)}
    x[k["big_mean"]] = 1e4 + n[k["big_mean"]]
    x[k["tiny_var"]] = 3.0 + 1e-4 * n[k["tiny_var"]]
    x[k["const_1000"]] = 1000.0
    x[k["const_pi"]] = math.pi
    x[k["zero"] | k["spike"]] = 0.0
    sp = k["spike"].nonzero().reshape(-1)
    x[sp, spike_at[sp]] = 100.0
    x[k["huge"]] = 1e15 * n[k["huge"]]
    nb = k["neighbour"].nonzero().reshape(-1)
    x[nb] = x[nb - 1]                                   # (kind 7: never row 0)
    x[k["bf16_exact"]] = x[k["bf16_exact"]].bfloat16().float()
    return x


def make_params(D, seed=0):
    """(gamma, beta) float32 [D] for RANDOM / EDGE."""
    g = _gen(seed, D, 77)
    return torch.randn(D, generator=g) * 0.2 + 1.0, torch.randn(D, generator=g) * 0.1


def make_bwd(family, rows, D, seed=0):
    """Seeded backward operands as float32 host tensors (values a bf16 stream holds exactly where the family says so): x, dy, gamma, add1, add2,
    dg_old, db_old, and for INTEGER mean / rstd (RANDOM / EDGE: the caller takes them from fwd_reference of the x it hands over)."""
    g = _gen(seed, rows, D, {RANDOM: 10, EDGE: 11, INTEGER: 12}[family])
    o = dict(family=family, rows=rows, D=D)
    if family != INTEGER:
        o["x"] = make_x(family, rows, D, seed)
        o["gamma"] = make_params(D, seed)[0]
        o["dy"] = torch.randn(rows, D, generator=g)
        o["add1"], o["add2"] = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g)
        o["dg_old"], o["db_old"] = torch.randn(D, generator=g), torch.randn(D, generator=g)
        o["a1"], o["a2"] = 0.7, 0.3
        return o
    half = D // 2

    def pm(hi, shape):
        return torch.randint(1, hi + 1, shape, generator=g).float() * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)

    mean = torch.randint(-3, 4, (rows,), generator=g).float()
    d = torch.zeros(rows, D)
    dy = torch.zeros(rows, D)
    gamma = torch.ones(D)
    dh, dyh, gh = pm(2, (rows, half)), pm(3, (rows, half)), torch.randint(1, 3, (half,), generator=g).float()
    d[:, :half], d[:, half:2 * half] = dh, dh
    dy[:, :half], dy[:, half:2 * half] = dyh, -dyh
    gamma[:half], gamma[half:2 * half] = gh, gh
    if D % 2:
        d[:, -1] = pm(2, (rows,))
        gamma[-1] = 2.0
    o["x"], o["dy"], o["gamma"] = mean[:, None] + d, dy, gamma
    o["mean"], o["rstd"] = mean, torch.full((rows,), 0.5)
    o["add1"] = torch.randint(-8, 9, (rows, D), generator=g).float()
    o["add2"] = torch.randint(-8, 9, (rows, D), generator=g).float()
    o["dg_old"] = torch.randint(-64, 65, (D,), generator=g).float()
    o["db_old"] = torch.randint(-64, 65, (D,), generator=g).float()
    o["a1"], o["a2"] = A1, A2
    return o


# ----------------------------------------------------------------------------- references and bounds
def fwd_reference(x, gamma, beta, eps=EPS, h=None):
    """float64 LayerNorm of the rows x holds (any float type; taken as they are) with the data of its acceptance rules.  h: the summation depth of a
    kernel outside layernorm.hip (tests/t2t_refs.py); None = h_of(D)."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    D = x.shape[-1]
    mean = x.mean(-1)
    d = x - mean[:, None]
    var = (d * d).mean(-1)
    rstd = (var + eps).rsqrt()
    xh = d * rstd[:, None]
    h = h_of(D) if h is None else float(h)
    E_mean = 2.0 * h * U * x.abs().mean(-1)
    rho = (E_mean * E_mean + 2.0 * (h + 3.0) * U * var) / (2.0 * (var + eps)) + 4.0 * U
    E_y = gamma.abs() * (xh.abs() * rho[:, None] + rstd[:, None] * (E_mean[:, None] + U * mean.abs()[:, None] + U * d.abs())) \
        + 4.0 * U * ((gamma * xh).abs() + beta.abs())
    return dict(y=xh * gamma + beta, mean=mean, var=var, rstd=rstd, E_mean=E_mean + U * mean.abs(), rho=rho, E_y=E_y)


def bwd_reference(x, dy, gamma, mean, rstd, *, add1=None, a1=None, add2=None, a2=None, beta_acc=0.0, dg_old=None, db_old=None, h=None):
    """float64 backward from the statistics handed over (see the module text) and its bounds.  a1 / a2 None means 1."""
    x, dy, gamma, mean, rstd = x.double(), dy.double(), gamma.double(), mean.double()[:, None], rstd.double()[:, None]
    rows, D = x.shape
    a1, a2 = (1.0 if a1 is None else float(a1)), (1.0 if a2 is None else float(a2))
    xh, gy = (x - mean) * rstd, dy * gamma
    c1, c2 = gy.mean(-1, keepdim=True), (gy * xh).mean(-1, keepdim=True)
    dx = rstd * (gy - c1 - xh * c2)
    T = rstd * (gy.abs() + c1.abs() + (xh * c2).abs())
    if add1 is not None:
        dx, T = dx + a1 * add1.double(), T + abs(a1) * add1.double().abs()
    if add2 is not None:
        dx, T = dx + a2 * add2.double(), T + abs(a2) * add2.double().abs()
    h = h_of(D) if h is None else float(h)
    E_c1 = 2.0 * h * U * gy.abs().mean(-1, keepdim=True)
    E_c2 = 2.0 * h * U * (gy * xh).abs().mean(-1, keepdim=True) + 2.0 * U * c2.abs()
    E_dx = rstd * (E_c1 + xh.abs() * E_c2) + 6.0 * U * T
    og = beta_acc * dg_old.double() if beta_acc != 0.0 else torch.zeros(D, dtype=torch.float64, device=x.device)
    ob = beta_acc * db_old.double() if beta_acc != 0.0 else torch.zeros(D, dtype=torch.float64, device=x.device)
    unit_r, unit_rd = 2.0 * (rows + 4) * U, 2.0 * (rows * D + 4) * U
    out = dict(dx=dx, E_dx=E_dx, dgamma=(dy * xh).sum(0) + og, E_dgamma=unit_r * ((dy * xh).abs().sum(0) + og.abs()),
               dbeta=dy.sum(0) + ob, E_dbeta=unit_r * (dy.abs().sum(0) + ob.abs()))
    dotB = (add2.double() * x).sum() if add2 is not None else torch.zeros((), dtype=torch.float64, device=x.device)
    SB = (add2.double() * x).abs().sum() if add2 is not None else torch.zeros((), dtype=torch.float64, device=x.device)
    out["dots"] = torch.stack([(dx * x).sum(), dotB])
    out["E_dots"] = unit_rd * torch.stack([(dx * x).abs().sum(), SB])
    return out


def integer_magnitudes(o, *, add1, add2, scalars, beta_acc):
    """sum |terms| / quantum of every accumulator of an INTEGER case (the worst partial sum of any order, in units of the accumulator's grid):
    c1 (quantum 1), c2 (1/2), dgamma (1/2), dbeta (1/2: beta_acc 0.5), dots (1/4 with the scalars, 1/2 without)."""
    x, dy, gamma = o["x"].double(), o["dy"].double(), o["gamma"].double()
    xh, gy = (x - o["mean"].double()[:, None]) * 0.5, dy * gamma
    assert float(gy.sum(-1).abs().max()) == 0.0 and float((gy * xh).sum(-1).abs().max()) == 0.0, "INTEGER rows: c1 = c2 = 0"
    a1, a2 = (o["a1"], o["a2"]) if scalars else (1.0, 1.0)
    dx = 0.5 * gy + (a1 * o["add1"].double() if add1 else 0.0) + (a2 * o["add2"].double() if add2 else 0.0)
    assert float(dx.abs().max()) < 64.0 and float((dx * 4).frac().abs().max()) == 0.0, "INTEGER dx: a multiple of 1/4 below 64"
    qd = 0.25 if scalars else 0.5
    return dict(c1=float(gy.abs().sum(-1).max()), c2=float((gy * xh).abs().sum(-1).max()) / 0.5,
                dgamma=float(((dy * xh).abs().sum(0) + abs(beta_acc) * o["dg_old"].double().abs()).max()) / 0.5,
                dbeta=float((dy.abs().sum(0) + abs(beta_acc) * o["db_old"].double().abs()).max()) / 0.5,
                dots=max(float((dx * x).abs().sum()) / qd, float((o["add2"].double() * x).abs().sum()) if add2 else 0.0))


# ----------------------------------------------------------------------------- acceptance
def half_ulp(got):
    p = 8 if got.dtype == torch.bfloat16 else 24
    _, e = torch.frexp(got.double().abs().clamp_min(2.0 ** -120))
    return torch.ldexp(torch.ones_like(got, dtype=torch.float64), e - p - 1)


def band(got, ref, E):
    """(ok [bool tensor], ratio): round_T(ref - E) <= got <= round_T(ref + E) for got's type T; ratio is the largest error over its bound, less
    half an ulp of a bf16 output (0 where E is 0 and got is the rounding of ref itself)."""
    lo, hi = round_to(ref - E, got.dtype), round_to(ref + E, got.dtype)
    ok = (got >= lo) & (got <= hi)
    err = (got.double() - ref).abs()
    if got.dtype == torch.bfloat16:
        err = (err - half_ulp(got)).clamp_min(0.0)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / E.clamp_min(1e-300))
    ratio = torch.where(ok, ratio.clamp_max(1.0), ratio)            # (inside the rounded band: never reported above 1)
    return ok, float(ratio.max()) if ratio.numel() else 0.0


def _report(name, ok, ratio, got, ref, fails, ratios):
    ratios[name] = max(ratios.get(name, 0.0), ratio)
    if not bool(ok.all()):
        i = tuple(int(v) for v in (~ok).nonzero()[0])
        fails.append(f"{name}: {int((~ok).sum())} of {ok.numel()} outside the rule, first at {i}: got {float(got[i])!r}, ref {float(ref[i])!r}, ratio {ratio:.3g}")


def fwd_accept(y, mean, rstd, ref):
    """One forward call's y [rows, D] (float32 or bf16), mean, rstd (float32 [rows]) against fwd_reference's data.  Returns (failures, ratios)."""
    fails, ratios = [], {}
    for name, t in (("y", y), ("mean", mean), ("rstd", rstd)):
        if not bool(torch.isfinite(t.double()).all()):
            fails.append(f"{name}: {int((~torch.isfinite(t.double())).sum())} elements not written or not finite")
    if fails:
        return fails, ratios
    _report("y", *band(y, ref["y"], ref["E_y"]), y, ref["y"], fails, ratios)
    err = (mean.double() - ref["mean"]).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / ref["E_mean"].clamp_min(1e-300))
    _report("mean", err <= ref["E_mean"], float(ratio.max()), mean, ref["mean"], fails, ratios)
    rel = (rstd.double() / ref["rstd"] - 1.0).abs()
    _report("rstd", rel <= ref["rho"], float((rel / ref["rho"]).max()), rstd, ref["rstd"], fails, ratios)
    return fails, ratios


def bwd_accept(dx, dgamma, dbeta, dots, ref, *, exact, dots_exact=None):
    """One backward call's outputs (dots may be None) against bwd_reference's data; exact: the INTEGER rule (dots_exact False: dots by the bound)."""
    fails, ratios = [], {}
    dots_exact = exact if dots_exact is None else dots_exact
    for name, got, ex in (("dx", dx, exact), ("dgamma", dgamma, exact), ("dbeta", dbeta, exact), ("dots", dots, dots_exact)):
        if got is None:
            continue
        if not bool(torch.isfinite(got.double()).all()):
            fails.append(f"{name}: {int((~torch.isfinite(got.double())).sum())} elements not written or not finite")
            continue
        r = ref[name]
        if ex:
            want = round_to(r, got.dtype)
            ok = got == want
            _report(name + " [exact]", ok, float((got.double() - want.double()).abs().max()), got, r, fails, ratios)
        else:
            _report(name, *band(got, r, ref["E_" + name]), got, r, fails, ratios)
    return fails, ratios
