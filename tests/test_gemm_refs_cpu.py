"""CPU: tests/gemm_refs.py accepts an honest kernel and rejects subtly wrong ones, and the cases of tests/test_gemm_accuracy_gpu.py reach the
kernel families they name.

The honest kernel is simulated: float32 accumulation in 32-element k-chunks (one MFMA step), chunks in forward or reversed order, the epilogue
in fused (one rounding per a * b + c) or unfused float32 arithmetic, an exact activation, one rounding to C's type.  Each mutant is that
simulation with one defect, on both operand families.  The route queries make no HIP call, so every GPU case's route assertion is dry-run here
with fake aligned addresses: a case that names one family and routes to another fails without a GPU."""
import pytest
import torch

import gemm_refs as R
import test_gemm_accuracy_gpu as G

HONEST_RATIO = 0.25


# ----------------------------------------------------------------------------- the simulated kernel
def f32(t):
    return t.to(torch.float32)


def sim_acc(A, B, reverse=False, K=None):
    """[M, K] x [N, K]^T in float32, 32 elements of K at a time."""
    K = K or A.shape[1]
    acc = torch.zeros(A.shape[0], B.shape[0], dtype=torch.float32)
    starts = list(range(0, K, 32))
    for k0 in (reversed(starts) if reverse else starts):
        k1 = min(K, k0 + 32)
        acc = acc + f32(A[:, k0:k1]) @ f32(B[:, k0:k1]).t()
    return acc


def fma(a, b, c):
    return f32(a.double() * b.double() + c.double())


def sim_nt(o, M, epi, *, alpha=1.0, alpha_ptr=None, c_dtype=torch.float32, reverse=False, fused=True, mutate=None):
    """Outputs {name: [M, ld] buffer} of a simulated uvc_gemm_nt; `mutate` names one defect."""
    N, K = o["N"], o["K"]
    ldc = o.get("ldc", N + 8)
    A, B = R.a_eff(o, M), R.view(o["B"], N, K, o["ldb"]).double()
    acc = sim_acc(A, B, reverse, K - 8 if mutate == "drop_k" else K)
    al = torch.tensor(alpha * (alpha_ptr or 1.0), dtype=torch.float32)
    bias = o["bias"].clone() if epi in R.HAS_BIAS else torch.zeros(N)
    if mutate == "bias_shift":
        bias = bias.roll(1)
    v = fma(acc, al, bias) if fused else f32(acc * al) + bias
    if epi in R.HAS_R:
        ldr = o["ldc_as_ldr"] if mutate == "r_stride" else o["ldr"]
        v = v + f32(R.view(torch.nan_to_num(o["R"]), M, N, ldr))
    if epi == R.BIAS_RESID_GATE:
        g0, g1 = o["gate"].flip(0) if mutate == "gate_swap" else o["gate"]
        r2 = f32(R.view(o["R2"], M, N, o["ldr"]))
        v = fma(g1, v, f32(g0 * r2)) if fused else f32(g1 * v) + f32(g0 * r2)
    if epi == R.MUL_AUX:
        v = v * f32(R.view(o["aux"], M, N, o["ldaux"]))
    if epi == R.MUL_AUX_Q8:
        v = v * fma(torch.tensor(R.Q8_STEP, dtype=torch.float32), f32(R.view(o["aux_q8"], M, N, o["ldaux"])), torch.tensor(R.Q8_LO, dtype=torch.float32))
    if epi == R.DGELU:
        v = v * f32(R.gelu_grad(R.view(o["aux"], M, N, o["ldaux"]).double()))
    if mutate == "row_swap":
        v[[1, 2]] = v[[2, 1]]
    res = {}
    if epi in (R.BIAS_GELU, R.BIAS_GELU_GRAD, R.BIAS_GELU_GRAD_Q8):
        res["C2"] = f32(R.gelu(v.double()))
    if epi == R.BIAS_GELU_OUT:
        v = f32(R.gelu(v.double()))
    if epi in (R.BIAS_GELU_GRAD, R.BIAS_GELU_GRAD_Q8):
        v = f32(R.gelu_grad(v.double()))
    res["C"] = v
    outs = {}
    for name, val in res.items():
        if name == "C" and epi == R.BIAS_GELU_GRAD_Q8:
            q = torch.clamp(torch.trunc(torch.clamp((val - f32(torch.tensor(R.Q8_LO))) / f32(torch.tensor(R.Q8_STEP)) + 0.5, min=0.0)), max=255.0)
            outs[name] = q.to(torch.uint8)
            continue
        buf = torch.full((M, ldc), R.SENTINEL, dtype=c_dtype)
        if mutate == "trunc" and c_dtype == torch.bfloat16:
            buf[:, :N] = (val.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
        else:
            buf[:, :N] = val.to(c_dtype)
        if mutate == "past_n":
            buf[:, N] = buf[:, N - 1]
        outs[name] = buf
    return outs


def nt_verdict(o, M, epi, outs, **kw):
    checks = R.nt_reference(o, M, epi, alpha=kw.get("alpha", 1.0), alpha_ptr=kw.get("alpha_ptr"))
    exact = o["family"] == R.INTEGER and epi != R.MUL_AUX_Q8
    return R.nt_accept(outs, checks, exact=exact, t_f32=o["t_f32"], N=o["N"])


SHAPES = [(33, 24, 72), (17, 65, 136), (5, 10, 8), (40, 129, 1032)]


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("epi", range(11), ids=R.EPI_NAMES)
def test_an_honest_float32_accumulation_is_accepted(family, epi):
    """Forward and reversed chunk order, fused and unfused epilogue, float32 and bf16 C, bf16 and float32 mode; the worst RANDOM ratio of the linear
    rule stays below 0.25 -- the headroom a GPU run is compared against."""
    worst = 0.0
    for i, (M, N, K) in enumerate(SHAPES):
        for t_f32 in (False, True):
            o = R.nt_operands(family, M, N, K, lda=K + 8, ldb=K + 8, ldr=N + 3, ldaux=N + 5, t_f32=t_f32, seed=i)
            for reverse, fused, c_dtype in ((False, True, torch.float32), (True, False, torch.bfloat16), (True, True, torch.bfloat16), (False, False, torch.float32)):
                if t_f32 and c_dtype == torch.bfloat16:
                    continue
                kw = dict(alpha=(1.0, 0.5)[i % 2], alpha_ptr=(None, 2.0)[(i // 2) % 2])
                outs = sim_nt(o, M, epi, c_dtype=c_dtype, reverse=reverse, fused=fused, **kw)
                fails, ratios = nt_verdict(o, M, epi, outs, **kw)
                assert not fails, (M, N, K, t_f32, reverse, fused, c_dtype, fails)
                if family == R.RANDOM:
                    worst = max([worst] + [v for (_, rule), v in ratios.items() if rule == "linear"])
    print(f"RATIO honest {R.EPI_NAMES[epi]} {family} {worst:.4f}")
    assert worst < HONEST_RATIO


GPU_KS = (4, 8, 12, 56, 64, 68, 72, 128, 136, 192, 256, 320, 384, 512, 576, 768, 1024)


@pytest.mark.parametrize("K", GPU_KS)
def test_honest_ratio_at_the_k_of_the_gpu_cases(K):
    """The simulation at the K of the GPU cases (the figure the docstring table of tests/test_gemm_accuracy_gpu.py sets each family's against): every
    linear epilogue, both chunk orders, float32 and bf16 C; K < 128 also in float32 mode, as the generic kernel's cases are."""
    worst = 0.0
    for t_f32 in ((False, True) if K < 128 else (False,)):
        if K % 8 and not t_f32:
            continue
        o = R.nt_operands(R.RANDOM, 256, 256, K, t_f32=t_f32, seed=K)
        for epi in R.LINEAR:
            for reverse, fused, c_dtype in ((False, True, torch.float32), (True, False, torch.bfloat16)):
                if t_f32 and c_dtype == torch.bfloat16:
                    continue
                outs = sim_nt(o, 256, epi, c_dtype=c_dtype, reverse=reverse, fused=fused, alpha=0.5)
                fails, ratios = nt_verdict(o, 256, epi, outs, alpha=0.5)
                assert not fails, (K, t_f32, epi, fails)
                worst = max([worst] + list(ratios.values()))
    print(f"RATIO honest K={K} {worst:.4f}")
    assert worst < HONEST_RATIO


NT_MUTANTS = [("drop_k", R.BIAS, 72), ("bias_shift", R.BIAS, 72), ("r_stride", R.BIAS_RESID, 72), ("row_swap", R.NONE, 72), ("past_n", R.BIAS, 72),
              ("trunc", R.BIAS_RESID, 1032), ("gate_swap", R.BIAS_RESID_GATE, 72)]


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("mutate,epi,K", NT_MUTANTS, ids=[m[0] for m in NT_MUTANTS])
def test_every_nt_mutant_is_rejected(family, mutate, epi, K):
    """The last 8 elements of a ragged K dropped; bias shifted by one column; R read with ldc where ldr differs; two rows swapped; one column past N
    stored; bf16 output truncated (at a K whose sums need more than bf16's eight bits); the gate pair swapped."""
    M, N = 33, 24
    c_dtype = torch.bfloat16 if mutate == "trunc" else torch.float32
    for t_f32 in ((False,) if mutate == "trunc" else (False, True)):
        o = R.nt_operands(family, M, N, K, lda=K + 8, ldb=K + 8, ldr=N + 3, ldaux=N + 5, t_f32=t_f32, seed=11)
        o["ldc"] = o["ldc_as_ldr"] = N + 1
        honest = sim_nt(o, M, epi, c_dtype=c_dtype)
        assert not nt_verdict(o, M, epi, honest)[0]
        wrong = sim_nt(o, M, epi, c_dtype=c_dtype, mutate=mutate)
        fails, _ = nt_verdict(o, M, epi, wrong)
        assert fails, (mutate, family, t_f32)


# ----------------------------------------------------------------------------- TN
def sim_tn(o, M, *, alpha, beta, rps, mutate=None):
    N1, N2 = o["N1"], o["N2"]
    A = R.view(o["A"], M, N1, o["lda"])
    A = A.double() if o["t_f32"] else R.bf(A)
    B = R.view(o["B"], M, N2, o["ldb"]).double()
    s, cs = torch.zeros(N1, N2), torch.zeros(N1)
    splits = -(-M // rps)
    for z in range(splits):
        if mutate == "omit_last_split" and z == splits - 1:
            continue
        m0, m1 = z * rps, min(M, (z + 1) * rps)
        p, pc = torch.zeros(N1, N2), torch.zeros(N1)
        for k0 in range(m0, m1, 64):
            k1 = min(m1, k0 + 64)
            p = p + f32(A[k0:k1]).t() @ f32(B[k0:k1])
            rows = A[k0:k1 - 1] if (mutate == "colsum_last_row" and k1 == M) else A[k0:k1]
            pc = pc + f32(rows).sum(0)
        for _ in range(2 if (mutate == "split_twice" and z == 1) else 1):
            s, cs = s + p, cs + pc
    old, cs_old = o["C_old"][:, :N2], o["cs_old"]
    al, be = torch.tensor(alpha, dtype=torch.float32), torch.tensor(beta, dtype=torch.float32)
    C = torch.full((N1, o["ldc"]), R.SENTINEL)
    if mutate == "beta_on_partial":
        C[:, :N2] = be * (old + al * s)
    else:
        C[:, :N2] = (be * old if beta != 0.0 else 0.0) + al * s
    return C, (be * cs_old if beta != 0.0 else 0.0) + al * cs, splits


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("mutate", [None, "omit_last_split", "split_twice", "colsum_last_row", "beta_on_partial"])
def test_tn_honest_accepted_and_every_mutant_rejected(family, mutate):
    """M = 200 in splits of 64 rows: three whole splits and a ragged one of 8 rows."""
    M, N1, N2 = 200, 24, 40
    worst = 0.0
    for t_f32 in (False, True):
        for alpha, beta in ((1.0, 0.5), (0.5, 1.0)) + (((1.0, 0.0),) if mutate != "beta_on_partial" else ()):
            o = R.tn_operands(family, M, N1, N2, lda=N1 + 8, ldb=N2 + 8, ldc=N2 + 4, t_f32=t_f32, seed=3)
            C, cs, splits = sim_tn(o, M, alpha=alpha, beta=beta, rps=64, mutate=mutate)
            ref = R.tn_reference(o, M, alpha=alpha, beta=beta, splits=splits)
            fails, ratios = R.tn_accept(C, cs, ref, exact=family == R.INTEGER, N2=N2)
            if mutate is None:
                assert not fails, (family, t_f32, alpha, beta, fails)
                worst = max([worst] + list(ratios.values()))
            elif not (mutate == "beta_on_partial" and beta == 1.0):
                assert fails, (mutate, family, t_f32, alpha, beta)
    if mutate is None and family == R.RANDOM:
        print(f"RATIO honest tn {worst:.4f}")
        assert worst < HONEST_RATIO


@pytest.mark.parametrize("M", [1, 63, 64, 65, 191, 192, 193, 2047, 2048])
def test_tn_honest_ratio_at_the_m_of_the_gpu_cases(M):
    """The TN simulation at the row counts of the GPU cases (splits of 64 rows up to 193, two splits of 1024 at 2047 / 2048), bf16 and float32 mode."""
    worst = {}
    for t_f32 in (False, True):
        o = R.tn_operands(R.RANDOM, M, 192, 200, lda=200, ldb=208, ldc=204, t_f32=t_f32, seed=M)
        w = 0.0
        for alpha, beta in ((1.0, 0.5), (0.5, 1.0), (1.0, 0.0)):
            C, cs, splits = sim_tn(o, M, alpha=alpha, beta=beta, rps=64 if M < 2000 else 1024)
            fails, ratios = R.tn_accept(C, cs, R.tn_reference(o, M, alpha=alpha, beta=beta, splits=splits), exact=False, N2=200)
            assert not fails, (M, t_f32, alpha, beta, fails)
            w = max([w] + list(ratios.values()))
        worst[t_f32] = w
    print(f"RATIO honest tn M={M} bf16 {worst[False]:.4f} float32 {worst[True]:.4f}")
    assert max(worst.values()) < HONEST_RATIO


def test_the_integer_family_is_exact_in_float32_in_any_order():
    """What the INTEGER rule rests on: forward and reversed float32 accumulation give the float64 result bit for bit."""
    o = R.nt_operands(R.INTEGER, 64, 48, 1032, seed=5)
    A, B = R.a_eff(o), R.view(o["B"], 48, 1032, 1032).double()
    ref = A @ B.t()
    assert float(ref.abs().max()) <= 9 * 1032 and not bool((A == 0).any()) and not bool((B == 0).any())
    for reverse in (False, True):
        assert torch.equal(sim_acc(A, B, reverse).double(), ref)
    with pytest.raises(AssertionError):
        R.nt_operands(R.INTEGER, 4, 8, 2 ** 21, seed=0)


def test_q8_boundary_rule_allows_one_step_only_at_a_boundary():
    g = torch.tensor([[0.4, R.Q8_LO + R.Q8_STEP * 100.5 + 1e-6, R.Q8_LO + R.Q8_STEP * 100.5 + 1e-6, 0.4]], dtype=torch.float64)
    code = R.q8_code(g)
    LE = torch.full_like(g, 1e-5)
    near = code.clone()
    near[0, 1] -= 1                                          # the value lies 1e-6 above a boundary: the lower code is allowed ...
    assert bool(R.check(near.to(torch.uint8), "q8", g, LE, exact=False, t_f32=False)[0].all())
    far = code.clone()
    far[0, 0] += 1                                           # ... away from one it is not
    assert not bool(R.check(far.to(torch.uint8), "q8", g, LE, exact=False, t_f32=False)[0].all())
    two = code.clone()
    two[0, 2] -= 2
    assert not bool(R.check(two.to(torch.uint8), "q8", g, LE, exact=False, t_f32=False)[0].all())


# ----------------------------------------------------------------------------- the GPU cases' routes, without a GPU
@pytest.fixture(scope="module")
def ops():
    from uvc_amd import build, ops
    build.build()
    return ops


def test_every_gpu_nt_case_routes_to_the_family_it_names(ops):
    families = set()
    for c in G.NT_CASES:
        r = G.assert_nt_route(ops, c, G.fake_ptr)
        families.add(r["family"])
        if c["family"] != "NT" and c["epi"] <= R.MUL_AUX:      # the cross-route comparison runs force_generic = 1, the ln_out forms without ln_out
            G.assert_nt_route(ops, dict(c, fg=1, ln=0, family="NT", expect={}), G.fake_ptr)
    assert families == {"NT", "NT_ROWS", "WS", "WS384", "WSN", "WSN16", "WSN16_DMA", "ROW384", "NT256", "NT8P"}
    ids = [G.case_id(c) for c in G.NT_CASES]
    assert len(set(ids)) == len(ids)


def test_every_gpu_tn_case_routes_to_the_family_it_names(ops):
    families, cfgs = set(), set()
    for c in G.TN_CASES:
        for M in G.tn_ms(c):
            ints, ptrs = G.tn_struct(c, M, beta=0.5, alpha=1.0, with_cs=True, with_alpha_ptr=True)
            fake = lambda p: G.PTR + 0x10000000 * ptrs.index(p)
            r = G.assert_tn_route(ops, c, M, ints, fake, ptrs, ops.gemm_tn_workspace_bytes(M, c["N1"], c["N2"]))
            families.add(r["family"])
            cfgs.add(r["cfg"])
    assert families == {"TN", "TN_BIG", "TN_DMA", "TN8P"} and cfgs == set(range(7))


def test_the_nt_cases_cover_the_edges_listed_for_each_family():
    by = {}
    for c in G.NT_CASES:
        by.setdefault(c["family"] + ("/f32" if c["dtype"] == G.F32 else ""), []).append(c)
    vals = lambda fam, k: {c[k] for c in by[fam]}
    assert vals("NT", "M") >= {1, 127, 128, 129} and vals("NT", "N") >= {8, 10, 63, 64, 65, 129, 136} and vals("NT", "K") >= {8, 56, 64, 72, 136}
    assert vals("NT", "epi") == set(range(9)) == vals("NT/f32", "epi") and vals("NT/f32", "K") >= {4, 12, 68}
    for k in ("ldc", "ldr", "ldaux"):              # odd (the element-wise path) and a multiple of the output vector, in bf16 mode (8) and float32 mode (4)
        assert {c[k] % 2 for c in by["NT"]} == {0, 1} and any(c[k] % 8 == 0 for c in by["NT"])
        assert {c[k] % 2 for c in by["NT/f32"]} == {0, 1} and any(c[k] % 4 == 0 for c in by["NT/f32"])
    assert any(c["epi"] == R.BIAS_GELU_GRAD_Q8 and c["ldc"] > c["N"] for c in by["WS"])
    assert vals("NT", "a_f32") == {0, 1} == vals("NT", "c_f32")
    assert vals("NT_ROWS", "M") >= {1, 16, 17, 1024} and vals("NT_ROWS", "K") >= {8, 504, 512, 520, 1024} and vals("NT_ROWS", "N") >= {8, 64, 72, 1000}
    assert len(vals("NT_ROWS", "epi")) == 6
    assert vals("WS", "M") >= {4096, 4097, 4096 + 37, 64 * 257 + 5} and vals("WS", "N") >= {64, 192, 256} and vals("WS", "epi") == set(range(11))
    assert {c["expect"]["nw"] for c in by["WS"]} == {3, 4, 8} and vals("WS", "K") == {192, 128}
    assert vals("WS384", "N") >= {192, 384, 768} and {c["expect"]["nw"] for c in by["WS384"]} == {6, 8} and 5 in vals("WS384", "fg")
    assert vals("WSN", "K") == {256, 512, 576, 768} == vals("WSN16", "K") and 2 in vals("WSN16", "fg")
    assert {(c["K"], c["ln"]) for c in by["WSN16_DMA"]} >= {(768, 0), (192, 0), (192, 1), (256, 1), (512, 1), (768, 1)}
    assert vals("WSN16_DMA", "M") >= {4096, 16 * 257, 4096 + 5} and vals("WSN16_DMA", "c_f32") == {0, 1}
    assert vals("ROW384", "M") == {4096, 4096 + 129} and len(vals("ROW384", "K")) == 3 and len(vals("ROW384", "epi")) == 2
    assert vals("NT256", "M") >= {1, 255, 256, 257, 513} and vals("NT256", "N") >= {256, 264, 511} and vals("NT256", "K") == {256, 320}
    assert any(c["ldc"] % 2 for c in by["NT256"]) and vals("NT256", "c_f32") == {0, 1}
    for ri in (8, 6, 5, 4):
        ms = {c["M"] for c in by["NT8P"] if c["expect"]["ri"] == ri and c["fg"] == G.NT_8PHASE | ri}
        assert ms >= {32 * ri - 1, 32 * ri, 32 * ri + 1}
        assert any(-(-c["M"] // (32 * ri)) * -(-c["N"] // 256) >= 257 for c in by["NT8P"] if c["fg"] == G.NT_8PHASE | ri)
