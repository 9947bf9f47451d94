"""GPU: the two kernels of uvc_amd/csrc/fused_mlp.hip -- k_mlp_fused_v3<TRAIN, RLOW> and the persistent k_mlp_fused_p -- against the float64
references and acceptance rules of tests/mlp_refs.py: EXACT operands within 2^-20 of the exact result (the strict check of the inference form, whose
only output is `out`), RANDOM operands (the scales of tests/test_kernels_gpu.py and a WIDE set: saturating pre-activations, a gate that does not sum
to 1, eps = 1e-3) stage by stage inside first-order float32 bounds.  Every element of every output is checked.

k_mlp_fused_v3.  Hidden widths 64, 128, 192, 320, 768, 1024 = 2 / 4 / 6 / 10 / 24 / 32 chunks of 32 units (1024: b1 fills its 4 KB of LDS, the dummy
DMA target starts right behind it).  Rows 1, 16, 17, 33, 127, 129, 300: a lone row, one 16-row tile of a wave, an empty second tile, a tile and one
row of the second wave, a workgroup less a row, a lone row in a second workgroup, a ragged third workgroup.  Forms: {inference, training} x {float32,
bf16 rows} x {gated, not} x {next_h with statistics, next_h alone, none} -- the full cross at F = 64, 768, 1024, each form once (rows rotating) at the
other widths -- on three operand sets (EXACT, RANDOM, RANDOM WIDE).  bf16 rows at M = 16383 (the last row count that stays on k_mlp_fused_v3 at
F >= 256) for F = 768 and 192.
k_mlp_fused_p (bf16 rows, inference form, M >= 16384, F >= 256).  F = 256, 320, 768, 1024; M = 16384 (79 workgroups, single passes of 12 - 13
tiles), 16437 (a ragged last tile of 5 rows), 53255 (256 workgroups, one of them with 14 tiles: two passes of 7, the one-tile-per-wave path), 73725
(passes of 9), 106505 (a 27-tile range: three passes); gated with next_h and statistics, plain, and next_h alone.  Its u comes from the training form
of k_mlp_fused_v3 on the same operands (checked by its own rule in the same test); the float64 reference runs on the device in row chunks.

Every call: outputs prefilled with NaN, 8 guard rows of a sentinel behind each (mean, rstd, next_mean, next_rstd too) that must keep their bytes; a
second call gives the same bytes; the first m < M rows (m % 16 != 0) equal the call on m rows.  Refusals leave every output byte untouched.

Measured on an MI355X: 66 tests in 12.5 s, the slowest 1.2 s (the first, which loads the library), every other below 0.6 s; worst error / bound per
output in test_worst_ratios_are_reported's docstring.

The tables (v3_cases, P_CASES) are walked by tests/test_mlp_refs_cpu.py without a GPU: every EXACT case is proven exact there and the honest
simulation stays below half of every RANDOM bound at every F used here (u and gp: inside their bound and below half of its arithmetic share L E1 --
the approximant's own error alone takes up to 0.98 of the share A that gemm_refs.py states for it)."""
import ctypes as C
import functools
import time

import pytest
import torch

import mlp_refs as R

pytestmark = pytest.mark.gpu

F32T, BF16T = torch.float32, torch.bfloat16
D = R.D
V3_F = (64, 128, 192, 320, 768, 1024)
V3_M = (1, 16, 17, 33, 127, 129, 300)
FULL_F = (64, 768, 1024)
V3_BIG = ((16383, 768), (16383, 192))
P_F = (256, 320, 768, 1024)
P_M = (16384, 16437, 53255, 73725, 106505)
P_VARIANTS = ((True, R.NEXT_STATS), (False, R.NEXT_NONE), (False, R.NEXT_H))           # (gated, next)
SETS = ((R.EXACT, False), (R.RANDOM, False), (R.RANDOM, True))                          # (family, wide)
FORMS = [dict(train=t, rows_t=rt, gated=g, next=n) for t in (False, True) for rt in (F32T, BF16T) for g in (False, True) for n in R.NEXT_MODES]
P_CASES = [(F, M) for M in P_M for F in P_F]
WORST = {}                                       # (family, output) -> worst error / bound seen by this module's cases
T0 = time.time()


def v3_cases(F):
    """[(M, form)]: the full cross at FULL_F; elsewhere each of the 24 forms once, its row count rotating with the form and the width."""
    if F in FULL_F:
        return [(M, f) for M in V3_M for f in FORMS]
    k = V3_F.index(F)
    return [(V3_M[(j + 3 * k) % len(V3_M)], f) for j, f in enumerate(FORMS)]


def prefix_rows(M):
    """m < M with m % 16 != 0 (0: no prefix run)."""
    m = M - 3
    if m < 1:
        return 0
    return m if m % 16 else m - 1


def dev():
    return torch.device("cuda")


def bits(t):
    return t.view(torch.int16 if t.dtype == BF16T else torch.int32)


def note(family, ratios):
    for k, v in ratios.items():
        WORST[(family, k)] = max(WORST.get((family, k), 0.0), v)


@functools.lru_cache(maxsize=8)
def device_weights(family, F, wide):
    """(what the kernel receives, the same as float64 for the rules)."""
    w = R.make_weights(family, F, wide)
    k = {n: w[n].to(dev()) for n in ("gamma", "beta", "b1", "b2", "next_gamma", "next_beta")}
    k["W1"], k["W2"] = w["W1"].to(BF16T).to(dev()), w["W2"].to(BF16T).to(dev())
    k["gate"] = torch.tensor(w["gate"], dtype=F32T, device=dev())
    return k, R.on(w, dev())


@functools.lru_cache(maxsize=4)
def device_rows(family, M, rows_t):
    x, xp = R.make_rows(family, M)
    return x.to(rows_t).to(dev()), xp.to(rows_t).to(dev())


def call(k, w, x, xp, m, form):
    """One uvc_mlp_fused_fwd call on the first m rows into fresh NaN-prefilled, guarded outputs."""
    from uvc_amd import ops
    outs = R.alloc(m, w["F"], form["rows_t"], form["train"], form["next"], dev())
    kw = {n: outs[n] for n in outs if n != "out"}
    if form["next"] != R.NEXT_NONE:
        kw.update(next_gamma=k["next_gamma"], next_beta=k["next_beta"])
    if form["gated"]:
        kw.update(x_prev=xp[:m], gate=k["gate"])
    ops.mlp_fused_fwd(x[:m], k["gamma"], k["beta"], k["W1"], k["b1"], k["W2"], k["b2"], outs["out"], w["eps"], **kw)
    return outs


def run_case(family, wide, F, M, form, u_got=None, check_prefix=True):
    """One case: the rules, the guards, determinism, the prefix run.  Returns the outputs."""
    k, w = device_weights(family, F, wide)
    x, xp = device_rows(family, M, form["rows_t"])
    what = (family, "wide" if wide else "", F, M, {n: str(v) for n, v in form.items()})
    outs = call(k, w, x, xp, M, form)
    fails, ratios = R.accept(outs, x, xp, w, form["gated"], M, u_got=u_got)
    note(family, ratios)
    assert not fails, (what, fails)
    again = call(k, w, x, xp, M, form)
    for n in outs:
        assert torch.equal(bits(outs[n]), bits(again[n])), (what, n, "not deterministic")
    m = prefix_rows(M) if check_prefix else 0
    if m:
        part = call(k, w, x, xp, m, form)
        assert not R.guard_failures(part, m), (what, "prefix run", R.guard_failures(part, m))
        for n in outs:
            assert torch.equal(bits(part[n][:m]), bits(outs[n][:m])), (what, n, f"rows depend on the row count ({m} of {M})")
    return outs


def run_group(family, wide, F, M, forms):
    """Every form of `forms` at one (operand set, F, M); the forms that store no u take it from one training-form call per row type and gate."""
    u_of = {}
    for form in forms:
        key = (form["rows_t"], form["gated"])
        if not form["train"] and family == R.RANDOM and key not in u_of:
            k, w = device_weights(family, F, wide)
            x, xp = device_rows(family, M, form["rows_t"])
            u_of[key] = call(k, w, x, xp, M, dict(form, train=True, next=R.NEXT_NONE))["u"][:M]
        run_case(family, wide, F, M, form, u_got=u_of.get(key))


# ----------------------------------------------------------------------------- k_mlp_fused_v3
@pytest.mark.parametrize("F,M", [(F, M) for F in V3_F for M in V3_M], ids=lambda v: str(v))
def test_fused_mlp_against_float64(F, M):
    forms = [f for m, f in v3_cases(F) if m == M]
    assert forms
    for family, wide in SETS:
        run_group(family, wide, F, M, forms)


@pytest.mark.parametrize("M,F", V3_BIG, ids=lambda v: str(v))
def test_fused_mlp_bf16_rows_below_the_persistent_threshold(M, F):
    """bf16 rows, inference form, one row below the switch to k_mlp_fused_p (F = 192 stays on k_mlp_fused_v3 at any row count)."""
    for family, wide in SETS:
        run_group(family, wide, F, M, [dict(train=False, rows_t=BF16T, gated=g, next=n) for g, n in P_VARIANTS])


# ----------------------------------------------------------------------------- k_mlp_fused_p
@pytest.mark.parametrize("F,M", P_CASES, ids=lambda v: str(v))
def test_persistent_fused_mlp_against_float64(F, M):
    """k_mlp_fused_p; the training-form call whose u anchors the RANDOM rule is itself held to every rule first."""
    for family, wide in SETS:
        u_of = {}
        for gated in sorted({g for g, _ in P_VARIANTS}):
            tr = run_case(family, wide, F, M, dict(train=True, rows_t=BF16T, gated=gated, next=R.NEXT_NONE), check_prefix=False)
            u_of[gated] = tr["u"][:M]
            del tr
        for gated, nxt in P_VARIANTS:
            run_case(family, wide, F, M, dict(train=False, rows_t=BF16T, gated=gated, next=nxt), u_got=u_of[gated])


# ----------------------------------------------------------------------------- refusals
def test_unsupported_calls_are_refused_with_nothing_written():
    from uvc_amd import _lib as L, ops
    lib = L.lib()
    M = 40
    for F, ok in ((0, 0), (32, 0), (96, 0), (1088, 0), (64, 1), (1024, 1)):
        assert lib.uvc_mlp_fused_supported(D, F, ops.UVC_BF16) == ok, F
    assert lib.uvc_mlp_fused_supported(384, 768, ops.UVC_BF16) == 0 and lib.uvc_mlp_fused_supported(D, 768, ops.UVC_F32) == 0

    def attempt(what, F=128, Dv=D, mutate=None, train=False, nxt=R.NEXT_NONE, gated=False):
        Fa = max(F, 64)
        g = torch.Generator().manual_seed(3)
        x = torch.randn(M + 1, D, generator=g).to(dev())
        xp = torch.randn(M, D, generator=g).to(dev())
        gamma, beta, b2, ng, nb = (torch.randn(D, generator=g).to(dev()) for _ in range(5))
        W1, W2 = torch.randn(Fa, D, generator=g).to(BF16T).to(dev()), torch.randn(D, Fa, generator=g).to(BF16T).to(dev())
        b1 = torch.randn(Fa, generator=g).to(dev())
        gate = torch.tensor([0.3, 0.7], device=dev())
        outs = R.alloc(M, Fa, F32T, train, nxt, dev())
        before = {n: t.clone() for n, t in outs.items()}
        a = L.uvc_mlp_args()
        a.x, a.gamma, a.beta, a.w1, a.b1, a.w2, a.b2, a.out = (L.ptr(t) for t in (x, gamma, beta, W1, b1, W2, b2, outs["out"]))
        a.M, a.D, a.F, a.eps, a.rows_lowp = M, Dv, F, 1e-6, 0
        for n in R.TRAIN_OUTPUTS + ("next_h", "next_mean", "next_rstd"):
            setattr(a, n, L.ptr(outs.get(n)))
        if nxt != R.NEXT_NONE:
            a.next_gamma, a.next_beta = L.ptr(ng), L.ptr(nb)
        if gated:
            a.x_prev, a.gate = L.ptr(xp), L.ptr(gate)
        if mutate:
            mutate(a, x)
        rc = lib.uvc_mlp_fused_fwd(C.byref(a), L.cur_stream())
        torch.cuda.synchronize()
        assert rc != 0, (what, "accepted")
        for n, t in outs.items():
            assert torch.equal(bits(t), bits(before[n])), (what, n, "written by a refused call")

    for F in (0, 32, 96, 1088):
        attempt(f"F = {F}", F=F)
    attempt("D = 384", Dv=384)
    attempt("misaligned x", mutate=lambda a, x: setattr(a, "x", x.data_ptr() + 4))
    attempt("gate without x_prev", gated=True, mutate=lambda a, x: setattr(a, "x_prev", None))
    attempt("x_prev without gate", gated=True, mutate=lambda a, x: setattr(a, "gate", None))
    for name in R.TRAIN_OUTPUTS:
        attempt(f"training set without {name}", train=True, mutate=lambda a, x, name=name: setattr(a, name, None))
    attempt("next_mean without next_rstd", nxt=R.NEXT_STATS, mutate=lambda a, x: setattr(a, "next_rstd", None))
    attempt("next_rstd without next_mean", nxt=R.NEXT_STATS, mutate=lambda a, x: setattr(a, "next_mean", None))
    attempt("next_h without next_gamma", nxt=R.NEXT_H, mutate=lambda a, x: setattr(a, "next_gamma", None))
    attempt("next_h without next_beta", nxt=R.NEXT_H, mutate=lambda a, x: setattr(a, "next_beta", None))
    attempt("next_mean without next_h", nxt=R.NEXT_STATS, mutate=lambda a, x: setattr(a, "next_h", None))


# ----------------------------------------------------------------------------- inference against training, reported
def test_worst_ratios_are_reported():
    """Prints the worst error / bound per output and family over the cases above (run last; -s shows it), the module's run time, and whether the
    inference and the training form's `out` are bit-identical (reported, not asserted: the rules do not rest on it).  The rules themselves assert
    <= 1 (EXACT: an error of at most 2^-20).

    Measured on an MI355X (66 tests in 12.5 s), worst error / bound over every case of this module -- beside it the honest CPU simulation of
    tests/test_mlp_refs_cpu.py (53 rows, worst width):
        RANDOM (standard and WIDE)   h: y 0.07, mean 0.07, rstd 0.35        simulation: y 0.06, mean 0.06, rstd 0.33
                                     u 0.48, gp 0.78                        simulation: u 0.45, gp 0.72 (the approximant's own error fills most of its
                                                                            bound A: 7.4e-4 of 7.6e-4 and 8.3e-5 of 8.5e-5 at its worst argument)
                                     out 0.09                               simulation: out 0.09 (F = 64) .. 0.01 (F = 1024)
                                     next_h: y 0.08, mean 0.09, rstd 0.27   simulation: y 0.08, mean 0.08, rstd 0.11
        EXACT                        out, h, mean, u, gp: error 0 in every element of every case (bound 2^-20); rstd 0.02; next_h: y 0.05, mean 0.01, rstd 0.22
    The inference and the training form's `out` were bit-identical in 18 of 18 comparisons."""
    same = total = 0
    for family, wide in SETS:
        for F, M in ((64, 33), (768, 300), (1024, 129)):
            for rows_t in (F32T, BF16T):
                k, w = device_weights(family, F, wide)
                x, xp = device_rows(family, M, rows_t)
                a = call(k, w, x, xp, M, dict(train=False, rows_t=rows_t, gated=True, next=R.NEXT_NONE))["out"]
                b = call(k, w, x, xp, M, dict(train=True, rows_t=rows_t, gated=True, next=R.NEXT_NONE))["out"]
                same, total = same + int(torch.equal(bits(a), bits(b))), total + 1
    print(f"inference and training form `out` bit-identical in {same} of {total} comparisons")
    for (family, name), v in sorted(WORST.items()):
        print(f"worst {family:6s} {name:22s} {v:.3g}")
    print(f"module run time {time.time() - T0:.1f} s")
    assert all(v <= 1.0 for v in WORST.values()), WORST
