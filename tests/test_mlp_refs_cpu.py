"""CPU: tests/mlp_refs.py accepts an honest simulation of the fused MLP kernels' arithmetic and rejects subtly wrong ones, and the EXACT cases of
tests/test_mlp_accuracy_gpu.py keep the promises their exactness rests on.

The honest kernel is simulated in torch: a float32 LayerNorm (two-pass), h rounded to bf16, fc1 and fc2 as float32 accumulations of four-term
float32 partial products in a SHUFFLED order of k (the biases, respectively x + b2, as the initial accumulator -- as the kernel has them), the
logistic-of-a-quintic GELU of csrc/common.h written out in float32 (fused multiply-adds emulated through float64), u and gp rounded to bf16, the mix as
fma(d1, acc, fma(d0, x_prev, 0)), one rounding of a bf16 row, and the next LayerNorm of the stored row.  It must be accepted by every rule of both
families and stay below HONEST_RATIO = 0.5 of every RANDOM bound at every hidden width the GPU module uses -- except that u and gp, whose bound is
mostly the approximant's own error (APPROXIMANT_BOUND below), are held to their whole bound and to half of its arithmetic share.  Each mutant is that simulation with
one defect; it must be rejected by both families unless noted (RANDOM: by the standard or the WIDE parameter set, as noted), and the EXACT family
must reject it on `out` ALONE -- all the inference form shows:

    two hidden units swapped inside one 32-unit chunk of W2        EXACT, RANDOM
    the last chunk dropped from fc2                                EXACT, RANDOM
    b1 shifted by one chunk                                        EXACT, RANDOM
    u truncated instead of rounded to nearest                      RANDOM (EXACT u is exact in bf16: blind by construction)
    d0 = 1 - d1 assumed                                            EXACT, RANDOM WIDE (the standard gate sums to 1)
    the residual taken from the previous row                       EXACT, RANDOM
    eps ignored                                                    RANDOM WIDE (h / rstd of every row; the constant EDGE rows turn NaN)
    row M - 1's result written to row M                            EXACT, RANDOM (the row left NaN and the guard row written)

Run with -s to see the worst honest ratio per output and width and what rejected each mutant."""
import pytest
import torch

import mlp_refs as R
import test_mlp_accuracy_gpu as G

HONEST_RATIO = 0.5
F32T, BF16T = torch.float32, torch.bfloat16
D = R.D
ALL_F = sorted(set(G.V3_F) | set(G.P_F) | {F for _, F in G.V3_BIG})
SIM_M = 53
# u and gp: the approximant bound A of gemm_refs.py (7.6e-4 max(|GELU|, 2e-3), 8.5e-5) lies 2 - 3 % above the approximant's own worst error (7.4e-4, 8.3e-5:
# csrc/common.h), which every honest kernel shows in full at the worst argument -- the whole rule is held to <= 1, its arithmetic share L E1 to < 0.5
APPROXIMANT_BOUND = ("u", "gp")


def f32(t):
    return t.to(F32T)


def fma(a, b, c):
    return f32(a.double() * b.double() + c.double())


def c32(v):
    return torch.tensor(v, dtype=F32T)


def shuffled_acc(acc, A, B, g, keep=None):
    """acc + A [M, K] . B [N, K]^T in float32: four k at a time (a float32 matmul of exact bf16 x bf16 products), the groups in a shuffled order;
    keep: only the first `keep` values of k count (the dropped-chunk mutant)."""
    K = A.shape[1] if keep is None else keep
    order = torch.randperm(K, generator=g)
    for i in range(0, K, 4):
        idx = order[i:i + 4]
        acc = acc + f32(A[:, idx]) @ f32(B[:, idx]).t()
    return acc


def gelu_fast(x):
    """Gelu<bf16_t>::fg of csrc/common.h in float32: (x Phi~(x), Phi~(x) + x phi(x))."""
    x2 = x * x
    xc = torch.minimum(x2, c32(47.7))
    q = fma(c32(1.12616072e-3), xc, c32(-1.07522990e-1))
    q = fma(q, xc, c32(-2.30050278))
    cdf = 1.0 / (1.0 + torch.exp2(x * q))
    e = torch.exp2(x2 * c32(-0.72134752))
    return x * cdf, fma(x * c32(0.39894228040143267794), e, cdf)


def layernorm32(x, gamma, beta, eps, mutate=None):
    mean = x.sum(-1) * c32(1.0 / D)
    d = x - mean[:, None]
    rstd = torch.rsqrt((d * d).sum(-1) * c32(1.0 / D) + c32(0.0 if mutate == "eps_ignored" else eps))
    return (x - mean[:, None]) * rstd[:, None] * gamma + beta, mean, rstd


def simulate(w, x, xp, M, rows_t, gated, train=True, next_mode=R.NEXT_STATS, mutate=None, seed=0, raw=None):
    """Outputs (as R.alloc lays them out) of a simulated uvc_mlp_fused_fwd on the first M rows; x / xp float32 host rows not yet rounded to rows_t."""
    F = w["F"]
    g = torch.Generator().manual_seed(seed)
    x, xp = f32(x[:M].to(rows_t)), f32(xp[:M].to(rows_t))
    gamma, beta, W1, b1, W2, b2 = (w[k] for k in ("gamma", "beta", "W1", "b1", "W2", "b2"))
    y, mean, rstd = layernorm32(x, gamma, beta, w["eps"], mutate)
    h = y.to(BF16T)
    if mutate == "b1_shift":
        b1 = b1.roll(-32)
    pre = shuffled_acc(b1[None, :].expand(M, F).clone(), f32(h), W1, g)
    fu, fg = gelu_fast(pre)
    if raw is not None:
        raw.update(fu=fu, fg=fg)                  # (the unrounded float32 values: arithmetic_share)
    u = (fu.view(torch.int32) & -65536).view(F32T).to(BF16T) if mutate == "u_truncated" else fu.to(BF16T)
    gp = fg.to(BF16T)
    if mutate == "w2_swap":
        W2 = W2.clone()
        j = 32 * (F // 32 - 1) + 5
        W2[:, [j, j + 9]] = W2[:, [j + 9, j]]
    res = x.roll(1, 0) if mutate == "prev_row_residual" else x
    if mutate == "prev_row_residual":
        res[0] = x[0]
    acc = shuffled_acc(res + b2, f32(u), W2, g, keep=F - 32 if mutate == "drop_last_chunk" else None)
    if gated:
        d0, d1 = c32(w["gate"][0]), c32(w["gate"][1])
        if mutate == "d0_from_d1":
            d0 = 1.0 - d1
        acc = fma(d1, acc, fma(d0, xp, c32(0.0)))
    out = acc.to(rows_t)
    ny, nmean, nrstd = layernorm32(f32(out), w["next_gamma"], w["next_beta"], w["eps"], mutate)
    vals = dict(out=out, h=h, mean=mean, rstd=rstd, u=u, gp=gp, next_h=ny.to(BF16T), next_mean=nmean, next_rstd=nrstd)
    outs = R.alloc(M, F, rows_t, train, next_mode)
    for k, t in outs.items():
        if mutate == "row_past_m":
            t[:M - 1] = vals[k][:M - 1]
            t[M] = vals[k][M - 1]
        else:
            t[:M] = vals[k]
    return outs


def verdict(family, wide, F, M, rows_t, gated, train=True, next_mode=R.NEXT_STATS, mutate=None, u_from_honest=False):
    w = R.make_weights(family, F, wide)
    x, xp = R.make_rows(family, M)
    raw = {}
    outs = simulate(w, x, xp, M, rows_t, gated, train, next_mode, mutate, raw=raw)
    u_got = None
    if not train:
        u_got = simulate(w, x, xp, M, rows_t, gated, True, R.NEXT_NONE, mutate if not u_from_honest else None)["u"][:M]
    return R.accept(outs, x[:M].to(rows_t), xp[:M].to(rows_t), R.on(w, "cpu"), gated, M, u_got=u_got) + (outs, raw)


def arithmetic_share(outs, raw, w, M):
    """Worst |float32 value - approximant(pre)| / (L E1) of u and gp before their rounding to bf16: the error of the honest ARITHMETIC (summation order,
    float32 steps of the approximant) over the share of the bound that exists for it; the approximant itself -- evaluated in float64 on the float64
    pre-activation of the stored h -- is taken out."""
    wd = R.on(w, "cpu")
    hd = outs["h"][:M].double()
    pre = wd["b1"] + hd @ wd["W1"].t()
    E1 = 2.0 * (D + 4) * R.U * (wd["b1"].abs() + hd.abs() @ wd["W1"].abs().t())
    fu, fg = gelu_fast(pre)
    return {"u arithmetic": float(((raw["fu"].double() - fu).abs() / (R.GR.L_GELU * E1)).max()),
            "gp arithmetic": float(((raw["fg"].double() - fg).abs() / (R.GR.L_GELUP * E1)).max())}


@pytest.mark.parametrize("F", ALL_F)
def test_the_honest_simulation_is_accepted_below_half_of_every_bound(F):
    worst = {}
    for family, wide in G.SETS:
        for rows_t in (F32T, BF16T):
            for gated in (False, True):
                for train, nxt in ((True, R.NEXT_STATS), (False, R.NEXT_H), (False, R.NEXT_NONE)):
                    fails, ratios, outs, raw = verdict(family, wide, F, SIM_M, rows_t, gated, train, nxt)
                    assert not fails, (family, wide, F, rows_t, gated, train, nxt, fails)
                    if family == R.RANDOM:
                        if train:
                            ratios.update(arithmetic_share(outs, raw, R.make_weights(family, F, wide), SIM_M))
                        for k, v in ratios.items():
                            worst[k] = max(worst.get(k, 0.0), v)
    print(f"RATIO honest F={F} " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert max(v for k, v in worst.items() if k not in APPROXIMANT_BOUND) < HONEST_RATIO, worst
    assert max(worst[k] for k in APPROXIMANT_BOUND) <= 1.0, worst


# mutant -> the operand sets that must reject it
MUTANTS = {"w2_swap": G.SETS, "drop_last_chunk": G.SETS, "b1_shift": G.SETS, "u_truncated": ((R.RANDOM, False), (R.RANDOM, True)),
           "d0_from_d1": ((R.EXACT, False), (R.RANDOM, True)), "prev_row_residual": G.SETS, "eps_ignored": ((R.RANDOM, True),), "row_past_m": G.SETS}


@pytest.mark.parametrize("F", (64, 320, 1024))
@pytest.mark.parametrize("mutate", sorted(MUTANTS))
def test_every_mutant_is_rejected(mutate, F):
    for family, wide in MUTANTS[mutate]:
        for rows_t in (F32T, BF16T):
            fails = verdict(family, wide, F, SIM_M, rows_t, True, mutate=mutate)[0]
            assert fails, (mutate, family, wide, F, rows_t, "accepted")
            print(f"MUTANT {mutate} F={F} {family}{' wide' if wide else ''} {str(rows_t)[6:]}: {fails[0][:110]}")
            if family == R.EXACT:
                # the inference form shows `out` alone (its u, for the RANDOM rule, comes from a training-form call with the same defect)
                fails = verdict(family, wide, F, SIM_M, rows_t, True, train=False, next_mode=R.NEXT_NONE, mutate=mutate)[0]
                assert fails, (mutate, family, F, rows_t, "accepted on `out` alone")


def test_the_standard_gate_is_blind_to_d0_from_d1_and_the_wide_one_is_not():
    """Why the WIDE set carries a gate that does not sum to 1."""
    assert not verdict(R.RANDOM, False, 128, SIM_M, F32T, True, mutate="d0_from_d1")[0]
    assert verdict(R.RANDOM, True, 128, SIM_M, F32T, True, mutate="d0_from_d1")[0]


def test_every_exact_case_of_the_gpu_module_is_exact():
    """exact_reference's assertions (h and u bf16-exact, every accumulator below 2^24 quanta) on the whole pool at every hidden width, gated and not:
    every EXACT row of every (F, M) of the GPU tables is a pool row."""
    px, pp = R.exact_pool()
    cases = {(F, M) for F in G.V3_F for M, _ in G.v3_cases(F)} | {(F, M) for M, F in G.V3_BIG} | set(G.P_CASES)
    assert {F for F, _ in cases} == set(ALL_F)
    for F in ALL_F:
        w = R.on(R.make_weights(R.EXACT, F), "cpu")
        for gated in (False, True):
            for rows_t in (F32T, BF16T):
                ref = R.exact_reference(px, pp, w, gated, rows_t)
                assert float(ref["u"].max()) > 0 and float((ref["u"] > 0).double().mean()) > 0.2, "EXACT u: a fair share of live hidden units"
    pool = {row.tobytes() for row in torch.cat([px, pp], 1).numpy()}
    for M in sorted({M for _, M in cases}):
        x, xp = R.make_rows(R.EXACT, M)
        assert x.shape == (M, D) and xp.shape == (M, D)
        assert all(row.tobytes() in pool for row in torch.cat([x, xp], 1).numpy()), (M, "a row outside the pool")


def test_the_gpu_tables_cover_every_axis_at_every_width():
    for F in G.V3_F:
        cases = G.v3_cases(F)
        assert {M for M, _ in cases} == set(G.V3_M), F
        for axis in ("train", "rows_t", "gated", "next"):
            assert {str(f[axis]) for _, f in cases} == {str(f[axis]) for f in G.FORMS}, (F, axis)
        if F in G.FULL_F:
            assert len(cases) == len(G.V3_M) * 24
    for M in list(G.V3_M) + list(G.P_M) + [m for m, _ in G.V3_BIG]:
        m = G.prefix_rows(M)
        assert (m == 0 and M == 1) or (0 < m < M and m % 16), M
