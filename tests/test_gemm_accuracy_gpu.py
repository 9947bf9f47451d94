"""GPU: every kernel family of the gemm*.hip files (UVC_ROUTE_*) against tests/gemm_refs.py -- exact results on the INTEGER operand family, the
float32 bound E on the RANDOM family -- at the smallest shapes that reach each tile edge.

Every case first asks uvc_gemm_nt_route / uvc_gemm_tn_route for the route of exactly the arguments it is about to pass and asserts the
family (and nw, kt, ri, nst, cfg, splits, rows_per_split where the case names them); tests/test_gemm_refs_cpu.py dry-runs the same
assertions without a GPU.  Then both operand families run: outputs start as NaN with a sentinel in the padding columns [N, ld), operand
padding [K, ld) is NaN.  On the RANDOM family every non-generic NT route is also torch.equal to force_generic = 1 on the same operands
(include/uvc_kernels.h: "every choice computes the same bits"), and the TN variants documented as the same bits are torch.equal.

The ln_out forms: C as above; ln_out against float64 LayerNorm of the rows C holds at the bf16 bound of test_layernorm_fwd_bwd
(rtol = atol = 1e-2); ln_mean within 2 (N + 4) 2^-24 mean|x| + 1e-5 |mean| and ln_rstd within rtol 1e-4 (float32 statistics of N values:
the same first-order summation bound as E; the rows' variance is of the order of their mean square, so no cancellation enters rstd).

k_gemm_row384_lnbwd<true, 1> is reachable from uvc_gemm_nt only at K >= 384 (uvc_gemm_nt_ln_supported): K in {384, 448, 768} stand for the
K in {128, 192, 384} one might list for it.

Measured on an MI355X (`pytest -s` prints a RATIO line per check; the table is their maximum per family): the largest ratio over every case
of the family.  "linear" is the least |x - ref| / E over the x that round to the stored value (the rule's own measure; RANDOM family -- on the
INTEGER family every linear output was torch.equal to the exact result on every route, so there is no figure).  "activation" is |error| over
L E + A + output rounding, both families; with a bf16 output that bound is little more than half a bf16 ulp, which a correctly rounded
value reaches, so figures near 1 are the rounding itself and not headroom used up.
GPU worst per family and K against the CPU simulation of an honest kernel at the same K (tests/test_gemm_refs_cpu.py:
  test_honest_ratio_at_the_k_of_the_gpu_cases, 256 x 256 outputs, every linear epilogue), "gpu / sim":
    NT bf16 mode      K 8: 0.065 / 0.165   56: 0.012 / 0.022   72: 0.008 / 0.015   136: 0.0045 / 0.0046        activation 0.974
    NT float32 mode   K 4: 0.136 / 0.194   12: 0.090 / 0.110   64: 0.028 / 0.020   68: 0.026 / 0.018                   activation 0.027
    NT_ROWS           K 8: 0.080 / 0.165   504 - 520: 0.0016 / 0.0010   1024: 0.0008 / 0.0005                  activation 0.831
    WS                K 128: 0.0078 / 0.0052   192: 0.0058 / 0.0032                                            activation 0.984
    WS384             K 384: 0.0026 / 0.0012                                                                   activation 0.929
    WSN               K 256: 0.0007 / 0.0023   512: 0.0006 / 0.0010   576: 0.0004 / 0.0009   768: 0.0003 / 0.0006
    WSN16             K 256: 0.0035 / 0.0023   512: 0.0018 / 0.0010   576: 0.0015 / 0.0009   768: 0.0016 / 0.0006
    WSN16_DMA         K 192: 0.0048 / 0.0032   256: 0.0032 / 0.0023   512: 0.0017 / 0.0010   768: 0.0014 / 0.0006
    ROW384            K 384, 448: 0.0006 / 0.0012   768: 0.0004 / 0.0006
    NT256             K 256: 0.0005 / 0.0023   320: 0.0033 / 0.0016                                            activation 0.946
    NT8P              K 256: 0.0013 / 0.0023   320: 0.0027 / 0.0016                                            activation 0.971
  TN, C per M against test_tn_honest_ratio_at_the_m_of_the_gpu_cases (colsum: at most 0.006 everywhere):
    bf16 mode (TN, TN_BIG, TN_DMA, TN8P alike)   M 1: 0 / 0.083   63 - 65: 0.015 / 0.015   191 - 193: 0.0032 / 0.0031   2047 - 4096: 0.0002 / 0.0001
    float32 mode (TN)                            M 1: 0.083 / 0.150   63 - 65: 0.034 / 0.032   191 - 193: 0.0045 / 0.0058
  No family exceeds 1; the largest gpu / sim quotient is 2.7 (WSN16 at K = 768, 790 000 outputs under the gate mix against the simulation's 65 000),
  below the 4 x that would make it a finding, and the ratio falls as ~ 1 / sqrt(K) as the rule's derivation predicts.  Every non-generic NT
  route was torch.equal to force_generic = 1 on the RANDOM family, every epilogue it shares with the generic kernel included and the ln_out
  forms (ROW384, the ring at K = 192 / 256 / 512 / 768) on their C: the header's "every choice computes the same bits" holds for all ten NT
  families.  UVC_TN_BY_SHAPE, _1 and UVC_TN_RING were torch.equal.  Run time of this file: 8.5 s for 275 cases, none above 1 s.

What it found: k_gemm_ws (K = 192 / 128 and K = 384 alike) with a float32 C and UVC_EPI_DGELU or UVC_EPI_MUL_AUX wrote nothing at all -- its
epilogue multiplied eight columns per lane where a float32 C gives a lane four, an out-of-bounds write to a local array that the compiler
resolved by dropping the stores (cases WS-*-dgelu-*cf, WS-*-mul_aux-*cf and WS384-*-mul_aux-*cf: every element still NaN).  No existing test ran
that combination on a streaming shape.
"""
import functools
import itertools

import pytest
import torch

import gemm_refs as R

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
PTR = 0x7F0000000000
NT_PTRS = ("A", "B", "C", "C2", "bias", "R", "R2", "aux", "gate", "alpha_ptr", "ln_gamma", "ln_beta", "ln_out", "ln_mean", "ln_rstd")
ALPHAS = ((1.0, None), (0.5, None), (1.0, 2.0), (0.5, 2.0))
NT_8PHASE = 0x100


def up8(n):
    return (n + 7) // 8 * 8


# ----------------------------------------------------------------------------- NT cases
def nt_case(family, M, N, K, epi, *, a_f32=0, c_f32=0, dtype=BF16, fg=0, lda=None, ldb=None, ldc=None, ldr=None, ldaux=None, alpha=1.0, alpha_ptr=None,
            ln=0, **expect):
    if dtype == F32:
        a_f32 = c_f32 = 1
    return dict(family=family, M=M, N=N, K=K, epi=epi, a_f32=a_f32, c_f32=c_f32, dtype=dtype, fg=fg, lda=lda or K, ldb=ldb or K, ldc=ldc or N,
                ldr=ldr or (ldc or N), ldaux=ldaux or (ldc or N), alpha=alpha, alpha_ptr=alpha_ptr, ln=ln, expect=expect)


def case_id(c):
    s = f"{c['family']}-{c['M']}x{c['N']}x{c['K']}-{R.EPI_NAMES[c['epi']]}-a{'f' if c['a_f32'] else 'b'}c{'f' if c['c_f32'] else 'b'}"
    if c["dtype"] == F32:
        s += "-f32mode"
    if c["fg"]:
        s += f"-fg{c['fg']:x}"
    if c["ln"]:
        s += "-ln"
    if (c["lda"], c["ldb"], c["ldc"], c["ldr"], c["ldaux"]) != (c["K"], c["K"], c["N"], c["N"], c["N"]):
        s += f"-ld{c['lda']}.{c['ldb']}.{c['ldc']}.{c['ldr']}.{c['ldaux']}"
    if c["alpha"] != 1.0 or c["alpha_ptr"]:
        s += f"-al{c['alpha']}p{c['alpha_ptr']}"
    return s


def _generic_cases():
    """k_gemm_nt (force_generic = 1), bf16 and float32 mode: all nine epilogues; M around the 128-row tile, N around the 64-column wave tile and the
    128-column tile, ragged K around the 64-element k tile; A and C in either type; lda, ldb = K + 8; ldc, ldr, ldaux each a multiple of the
    output vector (the 16-byte path) and odd (N + 1, N + 3, N + 5: the element-wise path)."""
    Ms, Ns, Ks = (1, 127, 128, 129), (8, 10, 63, 64, 65, 129, 136), (8, 56, 64, 72, 136)
    out = []
    for i, epi in enumerate(range(9)):
        for j, N in enumerate(Ns):
            t = i + j
            odd = (t % 4, (t // 2) % 4)                       # which of ldc / ldr / ldaux are odd: all combinations over the table
            ldc = N + 1 if odd[0] in (1, 3) else up8(N) + 8
            ldr = N + 3 if odd[1] in (1, 2) else up8(N) + 8
            ldaux = N + 5 if odd[1] in (2, 3) else up8(N) + 16
            al, ap = ALPHAS[t % 4]
            K = Ks[t % 5]
            out.append(nt_case("NT", Ms[t % 4], N, K, epi, a_f32=t % 2, c_f32=(t // 2) % 2, fg=1, lda=K + 8, ldb=K + 8, ldc=ldc, ldr=ldr, ldaux=ldaux,
                               alpha=al, alpha_ptr=ap))
    for i, epi in enumerate(range(9)):                        # float32 mode: 4-element chunks, K around the 32-element k tile of its MFMA
        for j, K in enumerate((4, 12, 68, 64)):
            t = i + j
            N = Ns[t % 7]
            al, ap = ALPHAS[(t + 1) % 4]
            out.append(nt_case("NT", Ms[(t + 1) % 4], N, K, epi, dtype=F32, fg=1, lda=K + 8, ldb=K + 8, ldc=N + 1 if t % 2 else up8(N) + 4,
                               ldr=N + 3 if t % 3 == 0 else up8(N) + 4, ldaux=N + 5 if t % 3 == 1 else up8(N) + 8, alpha=al, alpha_ptr=ap))
    return out


def _rows_cases():
    Ms, Ks, Ns = (1, 16, 17, 1024), (8, 504, 512, 520, 1024), (8, 64, 72, 1000)
    out = []
    for i, epi in enumerate((R.NONE, R.BIAS, R.BIAS_RESID, R.BIAS_RESID_GATE, R.BIAS_GELU_GRAD, R.MUL_AUX)):
        for j, K in enumerate(Ks):
            t = i + j
            N = Ns[t % 4]
            al, ap = ALPHAS[t % 4]
            out.append(nt_case("NT_ROWS", Ms[(i + 2 * j) % 4], N, K, epi, a_f32=t % 2, c_f32=(t // 2) % 2, lda=K + 8, ldb=K + 8, ldc=N + 8, ldr=N + 16,
                               ldaux=N + 24, alpha=al, alpha_ptr=ap))
    return out


def _ws_cases():
    """k_gemm_ws at K = 192 / 128: 64-row tiles walked by persistent workgroups; 64 * 257 + 5 rows are more row groups than workgroups."""
    Ms = (4096, 4097, 4096 + 37, 64 * 257 + 5)
    out = []
    for i, epi in enumerate(range(9)):
        for j, (N, nw) in enumerate(((64, 3), (192, 3), (256, 4))):
            t = i + j
            K = (192, 128)[t % 2]
            a_f32, c_f32 = t % 2, (t // 2) % 2
            al, ap = ALPHAS[t % 4]
            vn = 4 if c_f32 else 8
            if N == 256 and K == 192 and epi in (R.DGELU, R.MUL_AUX) and not a_f32 and not c_f32:
                a_f32 = 1                                     # (the eight-wave form has its own cases below)
            out.append(nt_case("WS", Ms[t % 4], N, K, epi, a_f32=a_f32, c_f32=c_f32, lda=K + 8, ldc=N + vn, ldr=N + 2 * vn, ldaux=N + 3 * vn, alpha=al, alpha_ptr=ap,
                               kt=K // 32, nw=nw, nj=4))
    for epi, M in ((R.MUL_AUX, 4096 + 37), (R.DGELU, 4097), (R.MUL_AUX_Q8, 4096 + 37)):
        out.append(nt_case("WS", M, 256, 192, epi, lda=200, alpha=0.5, alpha_ptr=2.0 if epi == R.DGELU else None, kt=6, nw=8, nj=2))
    # (the one-byte C and its bf16 C2 on rows of N + 8: the codes leave as 16-byte stores, the padding bytes keep their sentinel)
    out.append(nt_case("WS", 4096 + 37, 256, 192, R.BIAS_GELU_GRAD_Q8, lda=200, ldc=264, kt=6, nw=4, nj=4))
    out.append(nt_case("WS", 64 * 257 + 5, 256, 192, R.BIAS_GELU_GRAD_Q8, kt=6, nw=4, nj=4))
    return out


def _ws384_cases():
    out = []
    epis = (R.BIAS, R.BIAS_GELU, R.BIAS_RESID, R.BIAS_RESID_GATE, R.BIAS_GELU_OUT, R.BIAS_GELU_GRAD, R.MUL_AUX)
    shapes = ((192, 0, 0, 6), (384, 0, 0, 6), (768, 0, 0, 8), (768, 1, 0, 6), (768, 0, 5, 6))      # N, float32 C, force_generic, waves
    for i, epi in enumerate(epis):
        for j in range(2):
            N, c_f32, fg, nw = shapes[(2 * i + j) % 5]
            al, ap = ALPHAS[(i + j) % 4]
            vn = 4 if c_f32 else 8
            out.append(nt_case("WS384", (4096, 4096 + 37)[(i + j) % 2], N, 384, epi, c_f32=c_f32, fg=fg, lda=392, ldc=N + vn, ldr=N + 2 * vn, ldaux=N + 3 * vn,
                               alpha=al, alpha_ptr=ap, kt=12, nw=nw, nj=2))
    out.append(nt_case("WS384", 4096 + 37, 768, 384, R.NONE, alpha=0.5, kt=12, nw=8, nj=2))      # the plain epilogue: eight waves only
    return out


def _wsn_cases():
    out = []
    for i, K in enumerate((256, 512, 576, 768)):
        for j, M in enumerate((4096, 4096 + 21)):
            al, ap = ALPHAS[(i + j) % 4]
            kw = dict(lda=K + 8, alpha=al, alpha_ptr=ap, kt=K // 32)
            out.append(nt_case("WSN", M, 192, K, (R.NONE, R.BIAS)[(i + j) % 2], ldc=200, **kw))
            out.append(nt_case("WSN16", M, 192, K, (R.BIAS, R.NONE)[(i + j) % 2], c_f32=1, ldc=196, **kw))
            # the residual epilogues on 16-row tiles: a strided A keeps K = 768 off the ring at M % 16 == 0 too
            out.append(nt_case("WSN16", M, 192, K, (R.BIAS_RESID, R.BIAS_RESID_GATE)[(i + j) % 2], c_f32=j, ldc=196, ldr=200, **kw))
    for epi, c_f32 in ((R.BIAS_RESID, 0), (R.BIAS_RESID_GATE, 1)):                               # UVC_NT_NO_DMA on the ring's own shape
        out.append(nt_case("WSN16", 4096, 192, 768, epi, c_f32=c_f32, fg=2, kt=24))
    return out


def _ring_cases():
    out = []
    for i, (epi, c_f32) in enumerate(itertools.product((R.BIAS_RESID, R.BIAS_RESID_GATE), (0, 1))):
        out.append(nt_case("WSN16_DMA", (4096, 16 * 257)[i % 2], 192, 768, epi, c_f32=c_f32, ldc=192 if i % 2 else 196, ldr=192, kt=24, ln=0, nst=3))
    for c_f32 in (0, 1):
        out.append(nt_case("WSN16_DMA", (16 * 257, 4096)[c_f32], 192, 192, R.BIAS_RESID, c_f32=c_f32, kt=6, ln=0, nst=7))
    for i, (K, nst) in enumerate(((192, 7), (256, 4), (512, 3), (768, 3))):
        for j, M in enumerate((4096, 16 * 257, 4096 + 5)):
            epi = R.BIAS_RESID if K == 192 else (R.BIAS_RESID, R.BIAS_RESID_GATE)[(i + j) % 2]
            out.append(nt_case("WSN16_DMA", M, 192, K, epi, c_f32=(i + j) % 2, ln=1, kt=K // 32, nst=nst))
    return out


def _row384_cases():
    return [nt_case("ROW384", M, 384, K, (R.BIAS_RESID_GATE if gate else R.BIAS_RESID), ln=1)
            for (K, M), gate in zip(itertools.product((384, 448, 768), (4096, 4096 + 129)), itertools.cycle((0, 1, 1, 0)))]


def _nt256_cases():
    Ms, Ns, Ks = (1, 255, 256, 257, 513), (256, 264, 511), (256, 320)
    epis = (R.NONE, R.BIAS, R.BIAS_GELU, R.BIAS_RESID, R.BIAS_RESID_GATE, R.DGELU, R.BIAS_GELU_OUT, R.BIAS_GELU_GRAD, R.MUL_AUX)
    out = []
    for t, (M, N) in enumerate(itertools.product(Ms, Ns)):
        al, ap = ALPHAS[t % 4]
        c_f32 = t % 2
        ldc = N + 1 if t in (4, 11) else up8(N) + 8
        out.append(nt_case("NT256", M, N, Ks[t % 2], epis[t % 9], c_f32=c_f32, fg=4, lda=Ks[t % 2] + 8, ldb=Ks[t % 2] + 8, ldc=ldc, ldr=up8(N) + 16,
                           ldaux=up8(N) + 24, alpha=al, alpha_ptr=ap))
    return out


def _nt8p_cases():
    epis = (R.BIAS, R.BIAS_RESID_GATE, R.MUL_AUX, R.BIAS_GELU_GRAD, R.NONE, R.BIAS_RESID, R.DGELU, R.BIAS_GELU, R.BIAS_GELU_OUT)
    out = []
    t = 0
    for ri in (8, 6, 5, 4):
        for M, N in zip((32 * ri - 1, 32 * ri, 32 * ri + 1), (256, 264, 520)):
            al, ap = ALPHAS[t % 4]
            K = (256, 320)[t % 2]
            out.append(nt_case("NT8P", M, N, K, epis[t % 9], fg=NT_8PHASE | ri, lda=K + 8, ldb=K + 8, ldc=up8(N) + 8, ldr=up8(N) + 16, ldaux=up8(N) + 24,
                               alpha=al, alpha_ptr=ap, ri=ri))
            t += 1
        # 86 tile rows x 3 tile columns = 258 tiles: a persistent workgroup (256 of them) takes a second tile; the last tile row is ragged
        out.append(nt_case("NT8P", 86 * 32 * ri - 3, 520, 256, epis[t % 9], fg=NT_8PHASE | ri, ri=ri))
    out.append(nt_case("NT8P", 257, 264, 320, R.BIAS_RESID, c_f32=1, fg=NT_8PHASE | 4, ldc=268, ri=8))      # float32 C: the 256-row tile
    return out


NT_CASES = (_generic_cases() + _rows_cases() + _ws_cases() + _ws384_cases() + _wsn_cases() + _ring_cases() + _row384_cases() + _nt256_cases() +
            _nt8p_cases())


def nt_struct(c):
    """The integer members of uvc_gemm_nt_args for a case and the names of its pointer members (the caller supplies tensors or, for the
    CPU dry run of the routes, fake aligned addresses)."""
    e = c["epi"]
    ints = dict(M=c["M"], N=c["N"], K=c["K"], lda=c["lda"], ldb=c["ldb"], ldc=c["ldc"], ldr=c["ldr"], ldaux=c["ldaux"], dtype=c["dtype"], a_is_f32=c["a_f32"],
                c_is_f32=c["c_f32"], epilogue=e, force_generic=c["fg"], alpha=c["alpha"], r_is_f32=int(e in R.HAS_R and bool(c["c_f32"])), ln_eps=1e-6)
    ptrs = ["A", "B", "C"]
    ptrs += ["bias"] if e in R.HAS_BIAS else []
    ptrs += ["R"] if e in R.HAS_R else []
    ptrs += ["R2", "gate"] if e == R.BIAS_RESID_GATE else []
    ptrs += ["aux"] if e in R.HAS_AUX else []
    ptrs += ["C2"] if e in R.HAS_C2 else []
    ptrs += ["alpha_ptr"] if c["alpha_ptr"] is not None else []
    ptrs += ["ln_gamma", "ln_beta", "ln_out", "ln_mean", "ln_rstd"] if c["ln"] else []
    return ints, ptrs


def assert_nt_route(ops, c, ptr_of):
    ints, ptrs = nt_struct(c)
    rc, r = ops.gemm_nt_route(**ints, **{p: ptr_of(p) for p in ptrs})
    assert rc == 0, (case_id(c), rc)
    assert r["family"] == c["family"], (case_id(c), r)
    assert (r["a_f32"], r["c_f32"], r["t_f32"], r["epilogue"]) == (c["a_f32"], c["c_f32"], int(c["dtype"] == F32), c["epi"]), (case_id(c), r)
    for k, v in c["expect"].items():
        assert r[k] == v, (case_id(c), k, v, r)
    return r


def fake_ptr(name):
    return PTR + 0x10000000 * NT_PTRS.index(name)


# ----------------------------------------------------------------------------- NT runner
def _key(c):
    return (c["N"], c["K"], c["lda"], c["ldb"], c["ldr"], c["ldaux"], c["dtype"] == F32)


NT_ROWS_OF = {}
for _c in NT_CASES:
    NT_ROWS_OF[_key(_c)] = max(NT_ROWS_OF.get(_key(_c), 0), _c["M"])


@functools.lru_cache(maxsize=None)
def _nt_operands(fam, key):
    """One operand set per widths and family (the most rows any case asks for; a case takes the first M), on the device, never modified."""
    N, K, lda, ldb, ldr, ldaux, t_f32 = key
    o = R.nt_operands(fam, NT_ROWS_OF[key], N, K, lda=lda, ldb=ldb, ldr=ldr, ldaux=ldaux, t_f32=t_f32, seed=1)
    for k, v in list(o.items()):
        if torch.is_tensor(v):
            o[k] = v.cuda()
    for k in ("A", "B", "R", "R2", "aux"):
        o[k + "16"] = o[k].bfloat16()
    o["ln_gamma"] = (1 + 0.1 * torch.randn(N, generator=torch.Generator().manual_seed(5))).cuda()
    o["ln_beta"] = (0.1 * torch.randn(N, generator=torch.Generator().manual_seed(6))).cuda()
    return o


def _out(M, N, ld, dtype):
    t = torch.full((M, ld), R.SENTINEL if dtype != torch.uint8 else R.SENTINEL_U8, device="cuda", dtype=dtype)
    t[:, :N] = float("nan") if dtype != torch.uint8 else 0
    return t


def _nt_launch(ops, c, o, fg=None, check_route=True):
    """Allocates the outputs, asserts the route of exactly these arguments, launches.  Returns the outputs by name."""
    M, N, e = c["M"], c["N"], c["epi"]
    t_f32 = c["dtype"] == F32
    cdt = torch.uint8 if e == R.BIAS_GELU_GRAD_Q8 else torch.float32 if c["c_f32"] else torch.bfloat16
    c2dt = torch.float32 if c["c_f32"] else torch.bfloat16
    lowp_r = not c["c_f32"]
    t = dict(A=o["A"] if c["a_f32"] else o["A16"], B=o["B"] if t_f32 else o["B16"], C=_out(M, N, c["ldc"], cdt), bias=o["bias"],
             R=o["R16"] if lowp_r else o["R"], R2=o["R216"] if lowp_r else o["R2"], gate=o["gate"],
             aux=o["aux_q8"] if e == R.MUL_AUX_Q8 else o["aux"] if t_f32 else o["aux16"], C2=_out(M, N, c["ldc"], c2dt),
             ln_gamma=o["ln_gamma"], ln_beta=o["ln_beta"])
    if c["alpha_ptr"] is not None:
        t["alpha_ptr"] = torch.tensor([c["alpha_ptr"]], device="cuda")
    if c["ln"]:
        t["ln_out"] = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
        t["ln_mean"], t["ln_rstd"] = torch.full((M,), float("nan"), device="cuda"), torch.full((M,), float("nan"), device="cuda")
    cc = dict(c, fg=c["fg"] if fg is None else fg)
    ints, ptrs = nt_struct(cc)
    if check_route:
        assert_nt_route(ops, cc, lambda p: t[p].data_ptr())
    else:
        rc, r = ops.gemm_nt_route(**ints, **{p: t[p].data_ptr() for p in ptrs})
        assert rc == 0 and r["family"] == "NT", (case_id(cc), rc, r)
    kw = {p: t[p] for p in ptrs if p not in ("A", "B", "C")}
    ops.gemm_nt(t["A"], t["B"], t["C"], dtype=c["dtype"], epilogue=e, alpha=c["alpha"], M=M, N=N, K=c["K"], lda=c["lda"], ldb=c["ldb"], ldc=c["ldc"],
                ldr=c["ldr"], ldaux=c["ldaux"], force_generic=cc["fg"], **kw)
    return {k: t[k] for k in ("C", "C2", "ln_out", "ln_mean", "ln_rstd") if k in ptrs or k == "C"}


def _record(c, fam, ratios):
    for (name, rule), v in ratios.items():
        if rule == "q8" or (fam == R.INTEGER and rule == "linear" and c["epi"] != R.MUL_AUX_Q8):
            continue
        print(f"RATIO {case_id(c)} {fam} {name} {rule} {v:.4f}")


def _check_ln(c, outs, o):
    M, N = c["M"], c["N"]
    rows = outs["C"][:, :N]
    ref, mean, rstd = R.layernorm_reference(rows, o["ln_gamma"], o["ln_beta"], 1e-6)
    assert bool(torch.isfinite(outs["ln_out"].float()).all()), "ln_out: rows not written"
    torch.testing.assert_close(outs["ln_out"].double(), ref, rtol=1e-2, atol=1e-2)
    m_tol = 2 * (N + 4) * R.U32 * rows.double().abs().mean(-1) + 1e-5 * mean.abs()
    assert bool(((outs["ln_mean"].double() - mean).abs() <= m_tol).all()), float(((outs["ln_mean"].double() - mean).abs() / m_tol).max())
    torch.testing.assert_close(outs["ln_rstd"].double(), rstd, rtol=1e-4, atol=0.0)


@pytest.mark.parametrize("c", NT_CASES, ids=case_id)
def test_nt_family_against_the_exact_and_the_float32_bound_rules(c):
    from uvc_amd import ops
    for fam in R.FAMILIES:
        o = _nt_operands(fam, _key(c))
        outs = _nt_launch(ops, c, o)
        checks = R.nt_reference(o, c["M"], c["epi"], alpha=c["alpha"], alpha_ptr=c["alpha_ptr"])
        exact = fam == R.INTEGER and c["epi"] != R.MUL_AUX_Q8
        fails, ratios = R.nt_accept(outs, checks, exact=exact, t_f32=c["dtype"] == F32, N=c["N"])
        _record(c, fam, ratios)
        assert not fails, (case_id(c), fam, fails)
        if c["ln"]:
            _check_ln(c, outs, o)
        if fam == R.RANDOM and c["family"] != "NT" and c["epi"] <= R.MUL_AUX:
            # (the generic kernel takes every epilogue but not ln_out: the ln_out forms are compared on C, the same call without the ln_* pointers)
            ref = _nt_launch(ops, dict(c, ln=0), o, fg=1, check_route=False)
            for k in ref:
                assert torch.equal(outs[k], ref[k]), (case_id(c), k, "differs from force_generic = 1",
                                                      float((outs[k].double() - ref[k].double()).abs().max()))


# ----------------------------------------------------------------------------- TN
def tn_case(N1, N2, cfg, family, *, variant=0, a_f32=0, dtype=BF16):
    return dict(N1=N1, N2=N2, cfg=cfg, family=family, variant=variant, a_f32=int(a_f32 or dtype == F32), dtype=dtype)


def tn_id(c):
    return f"cfg{c['cfg']}-{c['family']}-{c['N1']}x{c['N2']}-v{c['variant']}-a{'f' if c['a_f32'] else 'b'}{'-f32mode' if c['dtype'] == F32 else ''}"


TN_TILES = {0: (128, 64), 1: (192, 256), 2: (256, 192), 3: (192, 192), 4: (96, 192), 5: (256, 256), 6: (128, 256)}
TN_CASES = [tn_case(8, 16, 0, "TN"), tn_case(120, 72, 0, "TN", a_f32=1), tn_case(136, 64, 0, "TN", dtype=F32), tn_case(200, 200, 0, "TN"),
            tn_case(200, 200, 0, "TN", dtype=F32),
            tn_case(192, 256, 1, "TN8P"), tn_case(192, 256, 1, "TN_DMA", variant=2), tn_case(192, 256, 1, "TN_BIG", a_f32=1),
            tn_case(256, 192, 2, "TN8P"), tn_case(256, 192, 2, "TN_DMA", variant=2), tn_case(256, 192, 2, "TN_BIG", a_f32=1),
            tn_case(384, 192, 3, "TN8P"), tn_case(384, 192, 3, "TN_DMA", variant=2), tn_case(384, 192, 3, "TN_BIG", a_f32=1),
            tn_case(192, 192, 4, "TN_DMA"), tn_case(768, 768, 5, "TN8P"), tn_case(768, 768, 6, "TN8P", variant=3)]
TN_M_SPLIT_RULE = (2047, 2048, 4095, 4096)      # either side of ">= 1024 (2048 for 192 x 192 tiles) rows a split once M holds two such splits"
TN_MAX_M = 4096


def tn_ms(c):
    """The M list whose route-dependent part (around rows_per_split * splits at >= 3 splits) is resolved by the route itself: 3 * 64 rows are three
    splits of one 64-row step wherever the shape has few tiles; M0 - 1 / + 1 make the last split ragged / add a split of one row."""
    return (1, 63, 64, 65, 191, 192, 193) + (TN_M_SPLIT_RULE if c["cfg"] else ())


def tn_struct(c, M, *, beta, alpha, with_cs, with_alpha_ptr):
    ints = dict(M=M, N1=c["N1"], N2=c["N2"], lda=c["N1"] + 8, ldb=c["N2"] + 8, ldc=c["N2"] + 4, dtype=c["dtype"], a_is_f32=c["a_f32"], variant=c["variant"],
                alpha=alpha, beta=beta)
    ptrs = ["A", "B", "C", "workspace"] + (["colsum_out"] if with_cs else []) + (["alpha_ptr"] if with_alpha_ptr else [])
    return ints, ptrs


def assert_tn_route(ops, c, M, ints, ptr_of, ptrs, ws_bytes):
    rc, r = ops.gemm_tn_route(**ints, workspace_bytes=ws_bytes, **{p: ptr_of(p) for p in ptrs})
    assert rc == 0, (tn_id(c), M, rc)
    b1, b2 = TN_TILES[c["cfg"]]
    assert (r["family"], r["cfg"], r["b1"], r["b2"]) == (c["family"], c["cfg"], b1, b2), (tn_id(c), M, r)
    s, rps = r["splits"], r["rows_per_split"]
    assert rps % 64 == 0 and (s - 1) * rps < M <= s * rps, (tn_id(c), M, r)
    if M in (191, 192, 193):
        assert s >= 3, (tn_id(c), M, r)
    if c["cfg"] and M in TN_M_SPLIT_RULE:
        rmin = 2048 if c["cfg"] == 3 else 1024
        tiles = (c["N1"] // b1) * (c["N2"] // b2)
        want = min((128 if tiles <= 4 else 256) // tiles, -(-M // 64))
        if M >= 2 * rmin:
            want = min(want, M // rmin)
        assert s <= want and rps == -(-(-(-M // want)) // 64) * 64, (tn_id(c), M, want, r)
    return r


@functools.lru_cache(maxsize=None)
def _tn_operands(fam, N1, N2, t_f32):
    o = R.tn_operands(fam, TN_MAX_M, N1, N2, lda=N1 + 8, ldb=N2 + 8, ldc=N2 + 4, t_f32=t_f32, seed=2)
    for k, v in list(o.items()):
        if torch.is_tensor(v):
            o[k] = v.cuda()
    o["A16"], o["B16"] = o["A"].bfloat16(), o["B"].bfloat16()
    return o


def _tn_launch(ops, c, o, M, *, beta, alpha, alpha_ptr, with_cs, variant=None, check_route=True):
    N1, N2 = c["N1"], c["N2"]
    t_f32 = c["dtype"] == F32
    nbytes = ops.gemm_tn_workspace_bytes(M, N1, N2)
    t = dict(A=o["A"] if c["a_f32"] else o["A16"], B=o["B"] if t_f32 else o["B16"], workspace=torch.full((nbytes // 4,), float("nan"), device="cuda"))
    if beta == 0.0:                     # k_tn_reduce does not read C then: NaN must not come through
        t["C"] = torch.full((N1, N2 + 4), float("nan"), device="cuda")
        t["C"][:, N2:] = R.SENTINEL
        cs = torch.full((N1,), float("nan"), device="cuda")
    else:
        t["C"], cs = o["C_old"].clone(), o["cs_old"].clone()
    if with_cs:
        t["colsum_out"] = cs
    if alpha_ptr is not None:
        t["alpha_ptr"] = torch.tensor([alpha_ptr], device="cuda")
    cc = dict(c, variant=c["variant"] if variant is None else variant)
    ints, ptrs = tn_struct(cc, M, beta=beta, alpha=alpha, with_cs=with_cs, with_alpha_ptr=alpha_ptr is not None)
    r = None
    if check_route:
        r = assert_tn_route(ops, cc, M, ints, lambda p: t[p].data_ptr(), ptrs, nbytes)
    ops.gemm_tn(t["A"], t["B"], t["C"], t["workspace"], dtype=c["dtype"], alpha=alpha, alpha_ptr=t.get("alpha_ptr"), beta=beta, M=M, N1=N1, N2=N2,
                lda=N1 + 8, ldb=N2 + 8, ldc=N2 + 4, colsum_out=t.get("colsum_out"), variant=cc["variant"])
    return t["C"], t.get("colsum_out"), r


@pytest.mark.parametrize("c", TN_CASES, ids=tn_id)
def test_tn_family_against_the_exact_and_the_float32_bound_rules(c):
    from uvc_amd import ops
    for i, M in enumerate(tn_ms(c)):
        beta = (0.0, 1.0, 0.5)[i % 3]
        alpha, alpha_ptr = ALPHAS[i % 4]
        with_cs = i % 4 != 3
        for fam in R.FAMILIES:
            o = _tn_operands(fam, c["N1"], c["N2"], c["dtype"] == F32)
            kw = dict(beta=beta, alpha=alpha, alpha_ptr=alpha_ptr, with_cs=with_cs)
            C, cs, r = _tn_launch(ops, c, o, M, **kw)
            ref = R.tn_reference(o, M, alpha=alpha, alpha_ptr=alpha_ptr, beta=beta, splits=r["splits"])
            fails, ratios = R.tn_accept(C, cs, ref, exact=fam == R.INTEGER, N2=c["N2"])
            if fam == R.RANDOM:
                for (name, _), v in ratios.items():
                    print(f"RATIO {tn_id(c)} M={M} {fam} {name} {v:.4f}")
            assert not fails, (tn_id(c), M, fam, r, fails)
            C2, cs2, _ = _tn_launch(ops, c, o, M, check_route=False, **kw)
            assert torch.equal(C, C2) and (cs is None or torch.equal(cs, cs2)), (tn_id(c), M, fam, "two launches differ")
            if fam == R.RANDOM and c["dtype"] == BF16 and not c["a_f32"] and c["variant"] != 3:
                for v in (0, 1, 2):     # UVC_TN_BY_SHAPE, _1, UVC_TN_RING: documented as the same bits
                    if v != c["variant"]:
                        C3, cs3, _ = _tn_launch(ops, c, o, M, variant=v, check_route=False, **kw)
                        assert torch.equal(C, C3) and (cs is None or torch.equal(cs, cs3)), (tn_id(c), M, "variant", v, "differs")
