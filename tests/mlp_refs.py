"""Plain float64 references of uvc_mlp_fused_fwd (include/uvc_kernels.h; uvc_amd/csrc/fused_mlp.hip), two seeded operand families and the
acceptance rules that hold a kernel to them.  Torch only, CPU-runnable (every function works on the device of its operands), nothing from uvc_amd;
tests/test_mlp_refs_cpu.py shows that the rules accept an honest simulation of the kernel's arithmetic and reject subtly wrong ones,
tests/test_mlp_accuracy_gpu.py holds k_mlp_fused_v3 (both forms, both row types) and the persistent k_mlp_fused_p to them.

    h = bf16(LayerNorm(x; gamma, beta, eps))      pre = b1 + h . W1^T      u = bf16(GELU(pre))      gp = bf16(GELU'(pre))
    out = d1 (x + b2 + u . W2^T) + d0 x_prev      (d0, d1) = gate, or (0, 1) without one; rounded once for bf16 rows
    next_h = bf16(LayerNorm(out as stored; next_gamma, next_beta, eps))
D = 192; W1 [F, 192] and W2 [192, F] bf16; b1, b2, gamma, beta float32; x, out, x_prev float32 or bf16 rows.

EXACT family: every stage is exact in float32 whatever the summation order, so the inference form -- which shows nothing but `out` -- has no tolerance
to hide in.  Rows x: a permutation of 96 zeros, 32 + 32 values +-1 and 16 + 16 values +-2, times s in {1, 2}: the row sum is 0 and sum x^2 = 192 s^2
in any order, so the kernel's mean is exactly 0 and its rstd is 1 / s within ~1e-6 relative (eps, the float32 1 / 192, the reciprocal square root).
gamma in {1, 2}, beta in {-1, 0, 1}, and gamma = 2 wherever beta != 0: gamma x / s + beta is an integer n of magnitude <= 5 that is 0 only where x = 0
and beta = 0 (no cancellation), so the float32 LayerNorm value lies within 2^-18 relative of n and its bf16 rounding IS n.  W1: six entries +-32 per
hidden unit, b1 in {-64, -32, 0, 32}: every pre-activation is a multiple of 32 of magnitude <= 1024 (positive ones exact in bf16).  The bf16-mode
GELU of csrc/common.h returns x for x >= 16 (its logistic is exactly 1 in float32), 0 at 0 and -0 for x <= -32 (2^(x q(x)) overflows to infinity, its
reciprocal is 0); GELU' is 1, 0.5 and 0.  So u = relu(pre) and gp = step(pre).  (Multiples of 16 are not enough: at x = -16 the approximant leaves
-5.8e-23, and the MFMA's accumulation is not round-to-nearest for an addend 80 binades below the sum -- measured on an MI355X with W1 = +-16: one `out`
of 57600 one float32 ulp low, 208 - 2^-16, where x + b2 was exactly 0 when such tails arrived.  With multiples of 32 no stage rounds at all.)
The rule keeps a slack far below anything an error can be:
    |got - expected| <= 2^-20             (any indexing error moves an element by at least 1/4)
expected = the float64 result (float32 rows) or ONE round-to-nearest-even of it to bf16 (bf16 rows).  W2 from {+-1, +-2, +-3} at density
min(1, 48 / F) (so that bf16 rows still resolve small changes), b2 integers in [-4, 4], x_prev integers in [-8, 8], gate (0.25, 0.5) -- it does not sum
to 1.  ``exact_reference`` asserts, on the operands it is given, that h and u are bf16-exact and that every accumulator (fc1 in units of 32, fc2 in
units of 1, the mix in units of 1/4) stays below 2^24 quanta in magnitude sum, i.e. that every partial sum in any order is exact.  Rows come from a
pool of 4096 (x, x_prev) pairs: a case of more rows draws from the pool at random, so proving the pool exact proves every row count exact.

RANDOM family: the scales of tests/test_kernels_gpu.py (x = 1.5 N + 0.2, gamma = 1 + 0.2 N, beta = 0.1 N, W1 = 0.06 N, W2 = 0.04 N, b = 0.1 N, gate
(0.3, 0.7), eps 1e-6) and a WIDE parameter set: W1 = 0.3 N (pre-activations reach both saturating tails of the GELU), gate (0.3, 0.6), eps = 1e-3 (an
ignored eps shows in h and rstd).  Rows alternate by tens between layernorm_refs.EDGE kinds and random rows.  Each stage is anchored on the KERNEL'S OWN
stored output of the stage before, u = 2^-24:
    h, mean, rstd     layernorm_refs.fwd_accept against fwd_reference(x as received, gamma, beta, eps)
    u, gp             pre = b1 + h_got . W1^T in float64, S1 = |b1| + |h_got| . |W1|^T, E1 = 2 (192 + 4) u S1 (the any-order bound of gemm_refs.py);
                      round_bf16(GELU(pre) - t) <= u <= round_bf16(GELU(pre) + t), t = L_GELU E1 + A, A = gemm_refs.approximant_bound (7.6e-4
                      max(|GELU|, 2e-3)); gp the same with L_GELUP and 8.5e-5
    out               acc = x + b2 + u_got . W2^T, S2 = |x| + |b2| + |u_got| . |W2|^T, E2 = 2 (F + 4) u S2; without a gate ref = acc, E = E2; with one
                      ref = d1 acc + d0 x_prev (d0, d1 the float32 values the kernel reads) and E = |d1| E2 + 2 u (|d1 acc| + |d0 x_prev|): the mix is
                      fma(d1, acc, fma(d0, x_prev, 0)), two roundings, each below u times the sum of the two terms' magnitudes.
                      round_T(ref - E) <= out <= round_T(ref + E) for the row type T (float32 rows: |out - ref| <= E up to the rounding of the bounds)
    next_h, next_mean, next_rstd    fwd_accept against fwd_reference(out_got, next_gamma, next_beta, eps)
The inference form and k_mlp_fused_p store no u: their `out` is held to the same rule with u_got taken from a TRAINING-form call on the same operands.
That rests on the two forms computing the same u: they are one template, and Gelu::f and Gelu::fg of csrc/common.h share their formula (x times the
same logistic); k_mlp_fused_p repeats that arithmetic operation for operation.  Should they disagree in a single bf16 ulp of one u (<= 2^-8 |u|),
`out` moves by at most 2^-8 |u| |W2| ~ 1e-4 at these scales: below E2 at the wide widths (1e-3 at F = 1024), where the rule would not notice it, and
above E2 at the narrow ones (2e-5 at F = 64), where the rule would fail and say so (the CPU simulation shows it: a u from another summation order
breaks `out` at F = 128).  The EXACT family is the strict check of those forms.  Every element of every output is checked.

Every output buffer of a call starts as NaN in its M rows with GUARD_ROWS rows of SENTINEL behind them (``alloc``); ``guard_failures`` says which
guards lost their bytes."""
from __future__ import annotations

import functools

import torch

import gemm_refs as GR
import layernorm_refs as LR

D = 192
U = 2.0 ** -24
EXACT, RANDOM = "exact", "random"
FAMILIES = (EXACT, RANDOM)
EXACT_SLACK = 2.0 ** -20
EXACT_GATE = (0.25, 0.5)             # (d0, d1)
EXACT_POOL = 4096
SENTINEL = LR.SENTINEL
GUARD_ROWS = LR.GUARD_ROWS
F32T, BF16T = torch.float32, torch.bfloat16
TRAIN_OUTPUTS = ("h", "mean", "rstd", "u", "gp")
NEXT_NONE, NEXT_H, NEXT_STATS = "none", "next_h", "next_h+stats"
NEXT_MODES = (NEXT_STATS, NEXT_H, NEXT_NONE)


def f32_value(v):
    """The float32 value of a Python float (what a kernel reads from a float32 buffer or argument)."""
    return float(torch.tensor(v, dtype=torch.float32))


def _gen(*key):
    s = 7
    for k in key:
        s = s * 1000003 + int(k)
    return torch.Generator().manual_seed(s % (2 ** 62))


def _pm(g, hi, shape):
    """Integers of magnitude 1 .. hi with a random sign."""
    return torch.randint(1, hi + 1, shape, generator=g).float() * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


# ----------------------------------------------------------------------------- operands
@functools.lru_cache(maxsize=32)
def make_weights(family, F, wide=False, seed=0):
    """Host float32 tensors gamma, beta [D], W1 [F, D], b1 [F], W2 [D, F], b2 [D] (W1 / W2 on bf16 values), next_gamma, next_beta [D], and the scalars
    gate = (d0, d1) and eps.  Treat as read-only (cached)."""
    g = _gen(seed, F, 1 if family == EXACT else 0, int(wide))
    w = dict(family=family, F=F, wide=wide)
    if family == EXACT:
        assert not wide
        beta = torch.randint(-1, 2, (D,), generator=g).float()
        gamma = torch.randint(1, 3, (D,), generator=g).float()
        gamma[beta != 0] = 2.0
        W1 = torch.zeros(F, D)
        cols = torch.rand(F, D, generator=g).topk(6, dim=1).indices
        W1.scatter_(1, cols, 32.0 * _pm(g, 1, (F, 6)))
        b1 = 32.0 * torch.randint(-2, 2, (F,), generator=g).float()
        W2 = _pm(g, 3, (D, F)) * (torch.rand(D, F, generator=g) < min(1.0, 48.0 / F)).float()
        b2 = torch.randint(-4, 5, (D,), generator=g).float()
        w.update(gamma=gamma, beta=beta, W1=W1, b1=b1, W2=W2, b2=b2, gate=EXACT_GATE, eps=1e-6)
    else:
        assert family == RANDOM
        n = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
        w.update(gamma=n(D) * 0.2 + 1.0, beta=n(D) * 0.1, W1=(n(F, D) * (0.3 if wide else 0.06)).bfloat16().float(), b1=n(F) * 0.1,
                 W2=(n(D, F) * 0.04).bfloat16().float(), b2=n(D) * 0.1, gate=(0.3, 0.6) if wide else (0.3, 0.7), eps=1e-3 if wide else 1e-6)
    w["next_gamma"], w["next_beta"] = torch.randn(D, generator=g) * 0.3 + 1.0, torch.randn(D, generator=g) * 0.2
    return w


@functools.lru_cache(maxsize=1)
def exact_pool(seed=0):
    """(x, x_prev) [EXACT_POOL, D]: the rows every EXACT case is drawn from."""
    g = _gen(seed, 4096)
    base = torch.cat([torch.zeros(96), torch.ones(32), -torch.ones(32), torch.full((16,), 2.0), torch.full((16,), -2.0)])
    perm = torch.rand(EXACT_POOL, D, generator=g).argsort(dim=1)
    scale = torch.randint(1, 3, (EXACT_POOL, 1), generator=g).float()
    return base[perm] * scale, torch.randint(-8, 9, (EXACT_POOL, D), generator=g).float()


@functools.lru_cache(maxsize=4)
def make_rows(family, M, seed=0):
    """(x, x_prev) [M, D] host float32 (EXACT: exact in bf16 too; RANDOM: the caller rounds them to a bf16 stream's type).  Read-only (cached)."""
    g = _gen(seed, M, 2 if family == EXACT else 3)
    if family == EXACT:
        px, pp = exact_pool(seed)
        idx = torch.arange(min(M, EXACT_POOL))
        if M > EXACT_POOL:
            idx = torch.cat([idx, torch.randint(0, EXACT_POOL, (M - EXACT_POOL,), generator=g)])
        return px[idx], pp[idx]
    x = LR.make_x(LR.EDGE, M, D, seed=seed + 11)
    plain = (torch.arange(M) // 10) % 2 == 1
    x[plain] = (torch.randn(M, D, generator=g) * 1.5 + 0.2)[plain]
    return x, torch.randn(M, D, generator=g)


def on(w, device):
    """The weights of make_weights as float64 tensors on `device` (scalars kept)."""
    return {k: (v.to(device=device, dtype=torch.float64) if torch.is_tensor(v) else v) for k, v in w.items()}


def gate_of(w, gated):
    return (f32_value(w["gate"][0]), f32_value(w["gate"][1])) if gated else (0.0, 1.0)


def row_chunks(M, F):
    """Row slices that keep one [rows, max(F, D)] float64 temporary near 64 MB (a large case's reference runs chunk by chunk)."""
    step = max(1, (1 << 23) // max(F, D))
    return [slice(lo, min(M, lo + step)) for lo in range(0, M, step)]


# ----------------------------------------------------------------------------- output buffers
def alloc(M, F, rows_t, train, next_mode, device="cpu"):
    """NaN-prefilled outputs of one call, each with GUARD_ROWS rows of SENTINEL behind its M rows."""
    def buf(cols, dt):
        t = torch.full((M + GUARD_ROWS,) + ((cols,) if cols else ()), float("nan"), dtype=dt, device=device)
        t[M:] = SENTINEL
        return t
    o = dict(out=buf(D, rows_t))
    if train:
        o.update(h=buf(D, BF16T), mean=buf(0, F32T), rstd=buf(0, F32T), u=buf(F, BF16T), gp=buf(F, BF16T))
    if next_mode != NEXT_NONE:
        o["next_h"] = buf(D, BF16T)
    if next_mode == NEXT_STATS:
        o.update(next_mean=buf(0, F32T), next_rstd=buf(0, F32T))
    return o


def guard_failures(outs, M):
    return [f"{k}: guard rows behind row {M} written" for k, t in outs.items() if not bool((t[M:].float() == SENTINEL).all())]


# ----------------------------------------------------------------------------- acceptance
def _note(name, ok, ratio, got, ref, fails, ratios, rule=""):
    ratios[name] = max(ratios.get(name, 0.0), ratio)
    if not bool(ok.all()):
        i = tuple(int(v) for v in (~ok).nonzero()[0])
        fails.append(f"{name}{rule}: {int((~ok).sum())} of {ok.numel()} outside the rule, first at {i}: got {float(got[i])!r}, ref {float(ref[i])!r}, "
                     f"ratio {ratio:.3g}")


def _finite(name, got, fails):
    bad = ~torch.isfinite(got.double())
    if bool(bad.any()):
        fails.append(f"{name}: {int(bad.sum())} of {bad.numel()} elements not written or not finite, first at {tuple(int(v) for v in bad.nonzero()[0])}")
        return False
    return True


def _band(name, got, ref, E, fails, ratios):
    if _finite(name, got, fails):
        _note(name, *LR.band(got, ref, E), got, ref, fails, ratios)


def exact_reference(x, x_prev, w, gated, rows_t):
    """EXACT family: float64 h, mean, u, gp and out (rounded once to rows_t) of the rows x / x_prev (any float type, any device), w = on(weights).
    Asserts the promises the exactness rests on."""
    assert w["family"] == EXACT
    xd = x.double()
    assert float(xd.sum(-1).abs().max()) == 0.0, "EXACT rows: row sum 0"
    s2 = (xd * xd).sum(-1) / D
    s = s2.sqrt()
    assert bool(((s == 1.0) | (s == 2.0)).all()), "EXACT rows: sum x^2 = 192 s^2, s in {1, 2}"
    n = xd / s[:, None] * w["gamma"] + w["beta"]
    assert float((n - n.round()).abs().max()) == 0.0 and float(n.abs().max()) <= 5.0, "EXACT h: integers of magnitude <= 5"
    assert bool(((n != 0) | ((xd == 0) & (w["beta"] == 0))).all()), "EXACT h: 0 only without cancellation"
    y = LR.fwd_reference(x, w["gamma"], w["beta"], eps=w["eps"])["y"]
    assert bool(((y - n).abs() <= 2.0 ** -18 * n.abs()).all()), "EXACT h: the LayerNorm value lies within 2^-18 relative of its integer"
    pre = w["b1"] + n @ w["W1"].t()
    S1 = w["b1"].abs() + n.abs() @ w["W1"].abs().t()
    assert float((pre / 32 - (pre / 32).round()).abs().max()) == 0.0 and float(S1.max()) / 32 < 2 ** 24, "EXACT fc1: multiples of 32, < 2^24 quanta"
    u = pre.clamp_min(0.0)
    assert torch.equal(GR.bf(u), u) and torch.equal(GR.bf(n), n), "EXACT h and u: exact in bf16"
    gp = (pre > 0).double() + 0.5 * (pre == 0).double()
    acc = xd + w["b2"] + u @ w["W2"].t()
    S2 = xd.abs() + w["b2"].abs() + u @ w["W2"].abs().t()
    assert float(S2.max()) < 2 ** 24, "EXACT fc2: every partial sum an integer below 2^24"
    out = acc
    if gated:
        d0, d1 = gate_of(w, True)
        assert (d0, d1) == EXACT_GATE
        out = d1 * acc + d0 * x_prev.double()
        assert float((d1 * S2 + d0 * x_prev.double().abs()).max()) * 4 < 2 ** 24 and float((out * 4 - (out * 4).round()).abs().max()) == 0.0, \
            "EXACT mix: multiples of 1/4 below 2^24 quanta"
    return dict(h=n, mean=torch.zeros_like(s), u=u, gp=gp, out=LR.round_to(out, rows_t).double())


def exact_accept(outs, ref, M):
    """Every output of `outs` that the EXACT rule covers (out; h, mean, u, gp of a training-form call) against exact_reference's data, rows [0, M)."""
    fails, ratios = [], {}
    for name in ("out", "h", "mean", "u", "gp"):
        if name not in outs:
            continue
        got = outs[name][:M]
        if _finite(name, got, fails):
            err = (got.double() - ref[name]).abs()
            _note(name, err <= EXACT_SLACK, float(err.max()) if err.numel() else 0.0, got, ref[name], fails, ratios, " [exact]")
    return fails, ratios


def ln_accept(prefix, rows, gamma, beta, eps, y, mean, rstd):
    """y (and mean / rstd where stored) against the float64 LayerNorm of `rows` as they are, by the rules of layernorm_refs."""
    ref = LR.fwd_reference(rows, gamma, beta, eps=eps)
    if mean is not None:
        fails, ratios = LR.fwd_accept(y, mean, rstd, ref)
        return [prefix + f for f in fails], {prefix + k: v for k, v in ratios.items()}
    fails, ratios = [], {}
    _band(prefix + "y", y, ref["y"], ref["E_y"], fails, ratios)
    return fails, ratios


def hidden_accept(h_got, w, u, gp):
    """u and gp [rows, F] bf16 against GELU / GELU' of pre = b1 + h_got . W1^T."""
    hd = h_got.double()
    pre = w["b1"] + hd @ w["W1"].t()
    E1 = 2.0 * (D + 4) * U * (w["b1"].abs() + hd.abs() @ w["W1"].abs().t())
    fails, ratios = [], {}
    f = GR.gelu(pre)
    _band("u", u, f, GR.L_GELU * E1 + GR.approximant_bound("gelu", f, False), fails, ratios)
    f = GR.gelu_grad(pre)
    _band("gp", gp, f, GR.L_GELUP * E1 + GR.approximant_bound("gelup", f, False), fails, ratios)
    return fails, ratios


def out_reference(x, x_prev, u_got, w, gated):
    """(ref, E) float64 of `out` from the rows as received and the stored u."""
    F = w["W2"].shape[1]
    xd, ud = x.double(), u_got.double()
    acc = xd + w["b2"] + ud @ w["W2"].t()
    E = 2.0 * (F + 4) * U * (xd.abs() + w["b2"].abs() + ud.abs() @ w["W2"].abs().t())
    if not gated:
        return acc, E
    d0, d1 = gate_of(w, True)
    xp = x_prev.double()
    return d1 * acc + d0 * xp, abs(d1) * E + 2.0 * U * ((d1 * acc).abs() + (d0 * xp).abs())


def random_accept(outs, x, x_prev, w, gated, M, u_got=None):
    """RANDOM family: every output of one call (outs from ``alloc``, rows [0, M)) against the rules of the module text, chunk by chunk.  x / x_prev as the
    kernel received them; u_got: the u of a training-form call on the same operands, for a call that stores none."""
    fails, ratios = [], {}

    def merge(fr):
        for f in fr[0]:
            if len(fails) < 12:
                fails.append(f)
        for k, v in fr[1].items():
            ratios[k] = max(ratios.get(k, 0.0), v)

    train = "u" in outs
    F = w["W1"].shape[0]
    for sl in row_chunks(M, F):
        if train:
            merge(ln_accept("h ", x[sl], w["gamma"], w["beta"], w["eps"], outs["h"][:M][sl], outs["mean"][:M][sl], outs["rstd"][:M][sl]))
            merge(hidden_accept(outs["h"][:M][sl], w, outs["u"][:M][sl], outs["gp"][:M][sl]))
        ug = outs["u"][:M][sl] if train else u_got[sl]
        fr = ([], {})
        if bool(torch.isfinite(ug.float()).all()):
            ref, E = out_reference(x[sl], x_prev[sl] if gated else None, ug, w, gated)
            _band("out", outs["out"][:M][sl], ref, E, *fr)
        else:
            fr[0].append("out: the u it is anchored on is not finite")
        merge(fr)
        if "next_h" in outs and bool(torch.isfinite(outs["out"][:M][sl].float()).all()):
            st = "next_mean" in outs
            merge(ln_accept("next ", outs["out"][:M][sl], w["next_gamma"], w["next_beta"], w["eps"], outs["next_h"][:M][sl],
                            outs["next_mean"][:M][sl] if st else None, outs["next_rstd"][:M][sl] if st else None))
    return fails, ratios


def exact_case_accept(outs, x, x_prev, w, gated, M):
    """EXACT family: out (and the training outputs) within 2^-20 of their exact values; rstd, next_h and its statistics -- not exact by construction -- by the
    LayerNorm rules, next_h against the kernel's own out."""
    fails, ratios = [], {}
    F = w["W1"].shape[0]
    for sl in row_chunks(M, F):
        ref = exact_reference(x[sl], x_prev[sl] if gated else None, w, gated, outs["out"].dtype)
        part = {k: v[:M][sl] for k, v in outs.items()}
        for fr in [exact_accept(part, ref, part["out"].shape[0])]:
            fails += fr[0][:12 - len(fails)] if len(fails) < 12 else []
            for k, v in fr[1].items():
                ratios[k + " [exact]"] = max(ratios.get(k + " [exact]", 0.0), v)
        more = []
        if "rstd" in outs and bool(torch.isfinite(part["rstd"]).all()):
            lref = LR.fwd_reference(x[sl], w["gamma"], w["beta"], eps=w["eps"])
            rel = (part["rstd"].double() / lref["rstd"] - 1.0).abs()
            fr = ([], {})
            _note("rstd", rel <= lref["rho"], float((rel / lref["rho"]).max()), part["rstd"], lref["rstd"], *fr)
            more.append(fr)
        elif "rstd" in outs:
            more.append((["rstd: not written or not finite"], {}))
        if "next_h" in outs and bool(torch.isfinite(part["out"].float()).all()):
            st = "next_mean" in outs
            more.append(ln_accept("next ", part["out"], w["next_gamma"], w["next_beta"], w["eps"], part["next_h"], part["next_mean"] if st else None,
                                  part["next_rstd"] if st else None))
        for fr in more:
            fails += fr[0][:12 - len(fails)] if len(fails) < 12 else []
            for k, v in fr[1].items():
                ratios[k] = max(ratios.get(k, 0.0), v)
    return fails, ratios


def accept(outs, x, x_prev, w, gated, M, u_got=None):
    """One call's outputs against its family's rules, guards included.  Returns (failures, ratios)."""
    fails = guard_failures(outs, M)
    fr = exact_case_accept(outs, x, x_prev, w, gated, M) if w["family"] == EXACT else random_accept(outs, x, x_prev, w, gated, M, u_got)
    return fails + fr[0], fr[1]
