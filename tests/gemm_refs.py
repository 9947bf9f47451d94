"""Plain float64 references of uvc_gemm_nt (every epilogue of include/uvc_kernels.h) and uvc_gemm_tn, two seeded operand families and
the acceptance rules that hold a kernel to them.  Torch only, CPU-runnable (every function works on the device of its operands), nothing
from uvc_amd; tests/test_gemm_refs_cpu.py shows that the rules accept an honest float32 accumulation and reject subtly wrong results,
tests/test_gemm_accuracy_gpu.py holds every kernel family of the gemm*.hip files to them.

Operands are flat buffers with a leading dimension, as the C ABI takes them: ``view(buf, rows, cols, ld)`` is the [rows, cols] matrix.

INTEGER family.  A and B from {+-1, +-2, +-3} (no zeros: every term counts); bias, R, R2, aux and the old C of TN integers of magnitude
<= 64; gate (0.25, 0.75); alpha in {1, 0.5}, alpha_ptr in {none, 2.0}; TN beta in {0, 1, 0.5}.  Every partial sum in any order is an
integer of magnitude <= 9 K (9 M for TN) < 2^24, every epilogue value a multiple of 1/8 below 2^21: each product, sum and epilogue step is
exact in float32 whatever the summation order, MFMA shape or split count.  The expected output is the float64 result (float32 C) or its
one round-to-nearest-even to bf16 (bf16 C), and the rule is torch.equal.

RANDOM family.  Normal operands at the scales of tests/test_kernels_gpu.py, rounded to the operand type before the reference sees them
(a float32 A handed to the bf16 mode is rounded by the kernel while staging: the reference takes its bf16 rounding).  Linear epilogues:
round_T(ref - E) <= got <= round_T(ref + E) element-wise, T the type of C, E = 2 (K + 4) 2^-24 S with S the float64 sum of the
magnitudes of every term that enters the element -- the first-order worst case of any summation order with faithfully rounding adders
(a sum of n terms in any order: at most n - 1 roundings of partial sums each below S; the epilogue adds at most four more roundings).
In bf16 mode the products of two bf16 operands are exact in float32, and the factor 2 covers the higher-order terms and a non-fused
multiply.  In float32 mode (NT and TN with dtype UVC_F32) every product of two float32 operands is rounded too unless the MFMA fuses it:
K more roundings, but each bounded by 2^-24 times its own term, so together by 2^-24 S: one more unit, (K - 1) + 1 + 4 = K + 4 at first
order, and the factor 2 still covers the higher-order terms.  (Bounding each product rounding by 2^-24 S instead would spend the factor:
(K - 1) + K + 4 <= 2 (K + 4).)  Real error is ~ sqrt(K) smaller.  TN: K becomes M + splits.

Activation epilogues: |got - f(ref_pre)| <= L E + A + output rounding with L = 1.13 (max |GELU'|) or 0.80 (max |GELU''|, for GELU'), A the
approximant bound of test_bf16_mode_gelu_approximant_error_bounds (bf16 mode: 7.6e-4 max(|GELU|, 2e-3) and 8.5e-5) or rtol = atol = 2e-5
(float32 mode), output rounding half an ulp of T at the bounded magnitude.  UVC_EPI_DGELU multiplies two factors, alpha acc (bound E, from
its own S) and GELU'(aux) of an exact operand (bound A): |got - ref| <= E |GELU'| + (|alpha acc| + E) A + 2^-24 |ref| + output rounding.
One-byte code: the byte is the code of float64 GELU'(ref_pre), +-1 where that value lies within (L E + 8.5e-5) / STEP of a code boundary."""
from __future__ import annotations

import math

import torch

U32 = 2.0 ** -24
INTEGER, RANDOM = "integer", "random"
FAMILIES = (INTEGER, RANDOM)
(NONE, BIAS, BIAS_GELU, BIAS_RESID, BIAS_RESID_GATE, DGELU, BIAS_GELU_OUT, BIAS_GELU_GRAD, MUL_AUX, BIAS_GELU_GRAD_Q8, MUL_AUX_Q8) = range(11)
EPI_NAMES = ("none", "bias", "bias_gelu", "bias_resid", "bias_resid_gate", "dgelu", "bias_gelu_out", "bias_gelu_grad", "mul_aux", "bias_gelu_grad_q8",
             "mul_aux_q8")
LINEAR = (NONE, BIAS, BIAS_RESID, BIAS_RESID_GATE, MUL_AUX, MUL_AUX_Q8)
HAS_BIAS = (BIAS, BIAS_GELU, BIAS_GELU_OUT, BIAS_RESID, BIAS_RESID_GATE, BIAS_GELU_GRAD, BIAS_GELU_GRAD_Q8)
HAS_R, HAS_AUX, HAS_C2 = (BIAS_RESID, BIAS_RESID_GATE), (DGELU, MUL_AUX, MUL_AUX_Q8), (BIAS_GELU, BIAS_GELU_GRAD, BIAS_GELU_GRAD_Q8)
# UVC_Q8_LO = -0.13f and UVC_Q8_STEP = 1.26f / 255.0f are float32 constants: their float32 values, not the decimals (next to the code whose
# decoded value is ~0, LO + STEP * 26 = -1.5e-3, the difference is 1e-6 of the product)
Q8_LO = float(torch.tensor(-0.13, dtype=torch.float32))
Q8_STEP = float(torch.tensor(1.26, dtype=torch.float32) / torch.tensor(255.0, dtype=torch.float32))
L_GELU, L_GELUP = 1.13, 0.80
GATE = (0.25, 0.75)                  # (g0, g1)
SENTINEL = -7.0                      # padding columns [N, ld) of every output
SENTINEL_U8 = 0xA5                   # the same for the one-byte code output
INT_MAG = 64


def bf(t):
    """Round to bf16 (nearest even, through float32) and return float64."""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def round_to(t, dtype):
    """float64 -> dtype (float32, or bf16 through float32 as the kernels hold their values)."""
    return t.to(torch.float32).to(dtype)


def view(buf, rows, cols, ld):
    return buf.reshape(-1).as_strided((rows, cols), (ld, 1))


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def q8_code(g):
    """uvc_kernels.h: q = min(255, trunc(max(0, (GELU' - LO) / STEP + 0.5)))."""
    return torch.clamp(torch.floor(torch.clamp((g - Q8_LO) / Q8_STEP + 0.5, min=0.0)), max=255.0)


# ----------------------------------------------------------------------------- operands
def _draw(family, g, rows, cols, ld, scale, mag, nan_pad=True):
    """[rows, ld] float32, columns past `cols` NaN (an operand's padding is never read)."""
    if family == INTEGER:
        if mag == 3:
            v = torch.randint(1, 4, (rows, cols), generator=g).float() * (torch.randint(0, 2, (rows, cols), generator=g).float() * 2 - 1)
        else:
            v = torch.randint(-mag, mag + 1, (rows, cols), generator=g).float()
    else:
        v = torch.randn(rows, cols, generator=g) * scale
    out = torch.full((rows, ld), float("nan") if nan_pad else 0.0)
    out[:, :cols] = v
    return out


def nt_operands(family, M, N, K, *, lda=None, ldb=None, ldr=None, ldaux=None, t_f32=False, seed=0):
    """Seeded NT operands as float32 host tensors: A [M, lda] (RANDOM: not yet rounded -- ``a_eff`` is what the arithmetic sees), B [N, ldb],
    bias [N], R / R2 [M, ldr] and aux [M, ldaux] on bf16 values (usable as bf16 or float32 streams), aux_q8 bytes, the gate pair."""
    lda, ldb, ldr, ldaux = lda or K, ldb or K, ldr or N, ldaux or N
    if family == INTEGER:
        # sums: integers <= 9 K; epilogue: multiples of 1/8 (alpha 0.5, gate quarters) of magnitude <= 9 K * 64 (MUL_AUX): 24 bits hold them below 2^21
        assert 9 * K < 2 ** 24 and 9 * K * INT_MAG + 3 * INT_MAG < 2 ** 21, "INTEGER family: partial sums and epilogue values stay exact in float32"
    g = torch.Generator().manual_seed(7919 * seed + 31 * N + K + (1 if family == INTEGER else 0))
    o = dict(family=family, M=M, N=N, K=K, lda=lda, ldb=ldb, ldr=ldr, ldaux=ldaux, t_f32=t_f32)
    o["A"] = _draw(family, g, M, K, lda, 1.0, 3)
    B = _draw(family, g, N, K, ldb, 0.05, 3)
    o["B"] = B if t_f32 else B.bfloat16().float()
    o["bias"] = _draw(family, g, 1, N, N, 1.0, INT_MAG).reshape(N)
    for n, ld in (("R", ldr), ("R2", ldr), ("aux", ldaux)):
        o[n] = _draw(family, g, M, N, ld, 1.0, INT_MAG).bfloat16().float()
    o["aux_q8"] = torch.randint(0, 256, (M, ldaux), generator=g).to(torch.uint8)
    o["gate"] = torch.tensor(GATE if family == INTEGER else (0.3, 0.7))
    return o


def a_eff(o, M=None):
    """The A the arithmetic sees: float32 mode as given, bf16 mode rounded (by the caller's cast or by the kernel while staging)."""
    A = view(o["A"], M or o["M"], o["K"], o["lda"])
    return A.double() if o["t_f32"] else bf(A)


def tn_operands(family, M, N1, N2, *, lda=None, ldb=None, ldc=None, t_f32=False, seed=0):
    lda, ldb, ldc = lda or N1, ldb or N2, ldc or N2
    if family == INTEGER:
        assert 9 * M < 2 ** 24, "INTEGER family: partial sums stay exact in float32"
    g = torch.Generator().manual_seed(104729 * seed + 31 * N1 + N2 + (1 if family == INTEGER else 0))
    o = dict(family=family, M=M, N1=N1, N2=N2, lda=lda, ldb=ldb, ldc=ldc, t_f32=t_f32)
    o["A"] = _draw(family, g, M, N1, lda, 1.0, 3)
    B = _draw(family, g, M, N2, ldb, 1.0, 3)
    o["B"] = B if t_f32 else B.bfloat16().float()
    o["C_old"] = _draw(family, g, N1, N2, ldc, 1.0, INT_MAG, nan_pad=False)
    o["C_old"][:, N2:] = SENTINEL
    o["cs_old"] = _draw(family, g, 1, N1, N1, 1.0, INT_MAG).reshape(N1)
    return o


# ----------------------------------------------------------------------------- references
def nt_reference(o, M, epi, *, alpha=1.0, alpha_ptr=None):
    """The float64 result of uvc_gemm_nt on the first M rows of the operands `o` and the data of its acceptance rules: a list of checks
    (output name "C" / "C2", rule, reference, bound data).  Rules: "linear" (ref, E), "gelu" / "gelup" (f(pre), L E), "dgelu" (ref, E', A weight),
    "q8" (GELU'(pre), L E)."""
    N, K = o["N"], o["K"]
    A, B = a_eff(o, M), view(o["B"], N, K, o["ldb"]).double()
    al = alpha * (alpha_ptr if alpha_ptr is not None else 1.0)
    acc, mag = A @ B.t(), A.abs() @ B.abs().t()
    pre, S = al * acc, abs(al) * mag
    if epi in HAS_BIAS:
        pre, S = pre + o["bias"].double(), S + o["bias"].double().abs()
    unit = 2.0 * (K + 4) * U32
    if epi in HAS_R:
        R = view(o["R"], M, N, o["ldr"]).double()
        pre, S = pre + R, S + R.abs()
    if epi == BIAS_RESID_GATE:
        g0, g1 = (float(x) for x in o["gate"])
        R2 = view(o["R2"], M, N, o["ldr"]).double()
        pre, S = g1 * pre + g0 * R2, abs(g1) * S + abs(g0) * R2.abs()
    if epi in (MUL_AUX, MUL_AUX_Q8):
        ax = view(o["aux"], M, N, o["ldaux"]).double() if epi == MUL_AUX else Q8_LO + Q8_STEP * view(o["aux_q8"], M, N, o["ldaux"]).double()
        pre, S = pre * ax, S * ax.abs()
    E = unit * S
    if epi in LINEAR:
        return [("C", "linear", pre, E)]
    if epi == BIAS_GELU:
        return [("C", "linear", pre, E), ("C2", "gelu", gelu(pre), L_GELU * E)]
    if epi == BIAS_GELU_OUT:
        return [("C", "gelu", gelu(pre), L_GELU * E)]
    if epi == BIAS_GELU_GRAD:
        return [("C", "gelup", gelu_grad(pre), L_GELUP * E), ("C2", "gelu", gelu(pre), L_GELU * E)]
    if epi == BIAS_GELU_GRAD_Q8:
        return [("C", "q8", gelu_grad(pre), L_GELUP * E), ("C2", "gelu", gelu(pre), L_GELU * E)]
    assert epi == DGELU
    gp = gelu_grad(view(o["aux"], M, N, o["ldaux"]).double())
    return [("C", "dgelu", pre * gp, (E, pre.abs(), gp.abs()))]


def approximant_bound(rule, f, t_f32):
    """|kernel's GELU / GELU' - exact| for an exact argument: the bounds the project already holds its approximants to."""
    if t_f32:
        return 2e-5 + 2e-5 * f.abs()
    return 7.6e-4 * f.abs().clamp_min(2e-3) if rule == "gelu" else torch.full_like(f, 8.5e-5)


def _out_rounding(bound_mag, dtype):
    return bound_mag * (2.0 ** -8 if dtype == torch.bfloat16 else U32)      # unit roundoff: 8 and 24 significant bits


def half_ulp(got):
    """Half the spacing of got's type at got (float64)."""
    p = 8 if got.dtype == torch.bfloat16 else 24
    _, e = torch.frexp(got.double().abs().clamp_min(2.0 ** -120))
    return torch.ldexp(torch.ones_like(got, dtype=torch.float64), e - p - 1)


def check(got, rule, ref, data, *, exact, t_f32):
    """One output against its rule.  Returns (ok [bool tensor], ratio): ratio is the largest error over its bound -- for the linear rule the least
    |x - ref| / E over the x that round to got (0 where got is the rounding of ref itself)."""
    if rule == "q8":
        LE = data
        tol = LE + 8.5e-5
        lo, hi, mid = q8_code(ref - tol), q8_code(ref + tol), q8_code(ref)
        g = got.double()
        ok = (g >= lo) & (g <= hi) & ((g - mid).abs() <= 1)
        return ok, float(((g - mid).abs()).max())
    g = got.double()
    if rule == "linear":
        E = data
        if exact:
            return got == round_to(ref, got.dtype), float((g - round_to(ref, got.dtype).double()).abs().max())
        lo, hi = round_to(ref - E, got.dtype), round_to(ref + E, got.dtype)
        ok = (got >= lo) & (got <= hi)
        dist = ((g - ref).abs() - half_ulp(got)).clamp_min(0.0) if got.dtype == torch.bfloat16 else (g - ref).abs()
        return ok, float((dist / E.clamp_min(1e-300)).max())
    if rule == "dgelu":
        E, P, gp = data
        A = approximant_bound("gelup", gp, t_f32)
        bound = E * gp + (P + E) * A + U32 * ref.abs()
    else:
        bound = data + approximant_bound(rule, ref, t_f32)
    bound = bound + _out_rounding(ref.abs() + bound, got.dtype)
    err = (g - ref).abs()
    return err <= bound, float((err / bound).max())


def nt_accept(outs, checks, *, exact, t_f32, N):
    """Every output of one call (outs: name -> [M, ld] tensor that started as NaN in [:, :N] and SENTINEL in [:, N:]) against its checks.
    Returns (failures [list of str], ratios {(name, rule): ratio})."""
    fails, ratios = [], {}
    for name, rule, ref, data in checks:
        full = outs[name]
        got = full[:, :N]
        if full.shape[1] > N and not bool((full[:, N:].double() == (SENTINEL_U8 if full.dtype == torch.uint8 else SENTINEL)).all()):
            fails.append(f"{name}: a padding column [N, ld) was written")
        if got.dtype != torch.uint8 and not bool(torch.isfinite(got.double()).all()):
            fails.append(f"{name}: {int((~torch.isfinite(got.double())).sum())} elements not written or not finite")
            continue
        ok, ratio = check(got, rule, ref, data, exact=exact and rule == "linear", t_f32=t_f32)
        ratios[(name, rule)] = ratio
        if not bool(ok.all()):
            bad = (~ok).nonzero()
            i, j = (int(x) for x in bad[0])
            fails.append(f"{name} [{rule}{', exact' if exact and rule == 'linear' else ''}]: {bad.shape[0]} of {ok.numel()} elements outside the rule, first at "
                         f"({i}, {j}): got {float(got[i, j])!r}, ref {float(ref[i, j])!r}, ratio {ratio:.3g}")
    return fails, ratios


def tn_reference(o, M, *, alpha=1.0, alpha_ptr=None, beta=0.0, splits=1):
    """float64 C = beta C_old + alpha A^T B and colsum = beta cs_old + alpha colsum(A) on the first M rows, with their bounds E (K -> M + splits)."""
    N1, N2 = o["N1"], o["N2"]
    A = view(o["A"], M, N1, o["lda"])
    A = A.double() if o["t_f32"] else bf(A)
    B = view(o["B"], M, N2, o["ldb"]).double()
    al = alpha * (alpha_ptr if alpha_ptr is not None else 1.0)
    old, cs_old = o["C_old"][:, :N2].double(), o["cs_old"].double()
    C = al * (A.t() @ B) + (beta * old if beta != 0.0 else 0.0)
    S = abs(al) * (A.abs().t() @ B.abs()) + (abs(beta) * old.abs() if beta != 0.0 else 0.0)
    cs = al * A.sum(0) + (beta * cs_old if beta != 0.0 else 0.0)
    Scs = abs(al) * A.abs().sum(0) + (abs(beta) * cs_old.abs() if beta != 0.0 else 0.0)
    unit = 2.0 * (M + splits + 4) * U32
    return dict(C=C, E=unit * S, cs=cs, Ecs=unit * Scs)


def tn_accept(C_full, cs, ref, *, exact, N2):
    """C_full [N1, ldc] (padding started as SENTINEL), cs [N1] or None.  Returns (failures, ratios)."""
    fails, ratios = [], {}
    if C_full.shape[1] > N2 and not bool((C_full[:, N2:] == SENTINEL).all()):
        fails.append("C: a padding column [N2, ldc) was written")
    for name, got, r, E in (("C", C_full[:, :N2], ref["C"], ref["E"]), ("colsum", cs, ref["cs"], ref["Ecs"])):
        if got is None:
            continue
        if not bool(torch.isfinite(got).all()):
            fails.append(f"{name}: not finite")
            continue
        ok, ratio = check(got, "linear", r, E, exact=exact, t_f32=True)
        ratios[(name, "linear")] = ratio
        if not bool(ok.all()):
            i = tuple(int(x) for x in (~ok).nonzero()[0])
            fails.append(f"{name}{' [exact]' if exact else ''}: {int((~ok).sum())} of {ok.numel()} outside the rule, first at {i}: got {float(got[i])!r}, "
                         f"ref {float(r[i])!r}, ratio {ratio:.3g}")
    return fails, ratios


def layernorm_reference(rows, gamma, beta, eps):
    """float64 LayerNorm of the rows C holds, its mean and rstd."""
    x = rows.double()
    mean = x.mean(-1)
    var = x.var(-1, unbiased=False)
    rstd = (var + eps).rsqrt()
    return (x - mean[:, None]) * rstd[:, None] * gamma.double() + beta.double(), mean, rstd
