"""GPU: the keyed Exp(1) generator (uvc_exp_noise) against its host restatement tests/noise_refs.py, its two extreme draws, what the kernels that
take -log(E) make of them, and the patch top-k (uvc_patch_topk_mask / _bwd) at the edges of its two workgroup sizes.

uvc_exp_noise.  Every size on both sides of a 256-thread block and of the 1024-block grid cap (1024 * 256 + 300 runs the grid-stride tail), keys at
the ends of every field (seed 2^64 - 1, step 0 / 2^63 - 1 / 2^63 / 2^64 - 1, site 0 / 2^32 - 1).  E is compared with -log(float64(u)) of the
restated float32 u: elementwise.hip holds logf to 1 ulp and rounding the float64 value to float32 adds 1/2, so the float32 ordinal distance is
asserted <= 2.  Measured on an MI355X over every case of this file (1.97 M elements): largest distance 2; 46 % of the elements are one or two
float32 values away from the rounded float64 value, so the device logf is a 1-ulp logf, not a correctly rounded one, and the bound has no slack.
A draw's first m elements are the m-element draw, bit for bit, and nothing past n is written.

The extreme counters.  c = 2^24 - 1 (seed 730, step 108, element 45643 of site 0) used to give u = 1.0f and a draw of -0.0f; it now gives the
smallest draw, -log(1 - 2^-24) = 5.96e-08 (float32: 2^-24).  c = 0 (step 187, element 45602) gives the largest, 25 ln 2 = 17.3287.  The two
positions come from noise_refs.find_counter, whose result tests/test_noise_refs_cpu.py asserts non-empty.  One of the comparison's own keys (seed
2^64 - 1, step 0, site 2^32 - 1) has the top counter at element 34993, so its n = 65536 and n = 1024 * 256 + 300 cases fail without the clamp too.

Consumers.  The two device draws themselves are planted among ordinary draws -- the smallest, the largest, both in one row -- and go through
uvc_patch_topk_mask (P = 196, 576), uvc_gate_distrib (modes 1, 3; Lb = 12) and uvc_dual_step (the engine-accuracy harness of
tests/test_uvc_engine_accuracy_gpu.py, DeiT-Tiny's dims): finite outputs, and the float64 references and bounds those kernels already have.
Before the fix the smallest draw is -0.0f: +inf as a Gumbel value, NaN in every softmax it enters.

Patch top-k edges.  P on both sides of a wave, of the 256-thread kernel and of the 1024-thread kernel, k in {0, 1, floor(0.9 P), P - 1, P},
tau in {0.5, 1, 2}, B in {1, 3}: index sets bit for bit against oracle/vit.py, mask atol 2e-6, y_soft and softmax(scores) rtol 2e-5, d(scores)
against float64 autograd rtol 5e-4 / atol 3e-6 / min(tau, 1) -- the production-shape tests' bounds -- with no row excluded: the inputs are
constructed (topk_inputs) so that every row's k-th and (k+1)-th reference y_soft differ and are normal float32, which is asserted on the host
before anything is launched.  Row 0 carries the production test's near tie (64 float32 ulps of u between the k-th and the (k+1)-th)."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import noise_refs as N
import small_kernel_refs as SR

pytestmark = pytest.mark.gpu

SEED, N_EXT = 730, 65536
SENT = -7.0
WORST = {"logf ordinal distance": 0}


def dev():
    return torch.device("cuda")


def exp_noise(out, n, seed, step, site):
    from uvc_amd import _lib as L
    return L.lib().uvc_exp_noise(L.ptr(out), n, seed & N.MASK, step & N.MASK, site, L.cur_stream())


def draw(n, seed, step, site, pad=64):
    """An n-element draw inside a sentinel-filled parent: (the draw as float32 numpy, the parent's tail)."""
    buf = torch.full((n + pad,), SENT, device=dev())
    assert exp_noise(buf, n, seed, step, site) == 0
    host = buf.cpu().numpy()
    return host[:n], host[n:]


KEYS = [(0, 0, 0), (730, 7, 3), (N.MASK, 0, (1 << 32) - 1), (1, (1 << 63) - 1, 0), (0x0123456789ABCDEF, 1 << 63, 1), (N.MASK, N.MASK, (1 << 32) - 1)]


# ============================================================================= uvc_exp_noise against the restatement
@pytest.mark.parametrize("n", [1, 255, 256, 257, 65536, 1024 * 256 + 300])
def test_exp_noise_equals_the_restatement(n):
    for seed, step, site in KEYS:
        what = f"n={n} seed={seed:#x} step={step:#x} site={site:#x}"
        e, tail = draw(n, seed, step, site)
        assert bool((tail == np.float32(SENT)).all()), f"{what}: written past n"                          # (c)
        assert bool(np.isfinite(e).all()) and bool((e > 0).all()), f"{what}: a draw is not finite and positive"
        ref = N.draws64(seed, step, site, n)
        d = N.ordinal_distance(e, ref)                                                                     # (a)
        worst = int(d.max())
        WORST["logf ordinal distance"] = max(WORST["logf ordinal distance"], worst)
        print(f"{what}: largest float32 ordinal distance to -log(float64(u)) = {worst}; off by one {int((d == 1).sum())}, by two {int((d == 2).sum())} of {n}")
        assert worst <= 2, f"{what}: ordinal distance {worst} at element {int(d.argmax())}: got {e[d.argmax()]!r}, reference {ref[d.argmax()]!r}"
        for m in sorted({1, min(n, 255), n // 2 + 1, max(1, n - 1)}):                                      # (b)
            em, tm = draw(m, seed, step, site)
            assert np.array_equal(em.view(np.uint32), e[:m].view(np.uint32)), f"{what}: the {m}-element draw is not a prefix"
            assert bool((tm == np.float32(SENT)).all())


def test_exp_noise_refuses_empty_draws():
    buf = torch.full((8,), SENT, device=dev())
    from uvc_amd import _lib as L
    assert exp_noise(buf, 0, 1, 1, 1) == 1 and exp_noise(buf, -1, 1, 1, 1) == 1
    assert L.lib().uvc_exp_noise(0, 8, 1, 1, 1, L.cur_stream()) == 1
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())


# ============================================================================= the two extreme counters
@functools.lru_cache(maxsize=None)
def extreme_positions():
    top, zero = N.find_counter(N.C_MAX, SEED, N_EXT, 109), N.find_counter(0, SEED, N_EXT, 188)
    assert top and zero, "no extreme counter found: the tests below would run on nothing"
    return top[0], zero[0]


@functools.lru_cache(maxsize=None)
def extreme_draws():
    """(smallest, largest) draw as the device makes them: float32 scalars (numpy)."""
    (s_top, i_top), (s_zero, i_zero) = extreme_positions()
    return draw(N_EXT, SEED, s_top, 0)[0][i_top], draw(N_EXT, SEED, s_zero, 0)[0][i_zero]


def test_extreme_counters_draw_the_smallest_and_the_largest_value():
    (s_top, i_top), (s_zero, i_zero) = extreme_positions()
    assert (s_top, i_top) == (108, 45643)
    assert int(N.counters(SEED, s_top, 0, 1, start=i_top)[0]) == N.C_MAX and int(N.counters(SEED, s_zero, 0, 1, start=i_zero)[0]) == 0
    lo, hi = extreme_draws()
    print(f"counter 2^24 - 1 at step {s_top} element {i_top}: draw {lo!r}; counter 0 at step {s_zero} element {i_zero}: draw {hi!r}")
    for name, v in (("counter 2^24 - 1", lo), ("counter 0", hi)):
        assert np.isfinite(v) and v > 0 and not np.signbit(v), f"{name}: the draw is {v!r}, not finite and strictly positive (Gumbel value {-np.log(np.float64(v))!r})"
    assert N.draws64(SEED, s_top, 0, 1, start=i_top)[0] == N.E_MIN and N.draws64(SEED, s_zero, 0, 1, start=i_zero)[0] == N.E_MAX
    # "equal" for a float32 against a float64 value is the ordinal bound of the comparison above
    assert int(N.ordinal_distance(np.float32([lo]), [N.E_MIN])[0]) <= 2, (lo, N.E_MIN)
    assert int(N.ordinal_distance(np.float32([hi]), [N.E_MAX])[0]) <= 2, (hi, N.E_MAX)
    assert abs(float(hi) - 17.3287) < 1e-4 and abs(float(lo) - 2.0 ** -24) < 1e-14
    # they are the extremes of their draws, and of the restatement
    for step, want in ((s_top, "min"), (s_zero, "max")):
        e = draw(N_EXT, SEED, step, 0)[0]
        assert (e.min() == lo) if want == "min" else (e.max() == hi)
        assert bool((e > 0).all()) and bool(np.isfinite(e).all())


# ============================================================================= consumers at the extreme draws
def planted(P, gen):
    """[5, P] ordinary Exp(1) draws with the device's extreme draws planted: row 0 the smallest (mid-row), 1 the largest, 2 both (the smallest on
    the last token, the largest on token 1), 3 the smallest on token 0 (whose mask is forced), 4 none."""
    lo, hi = (float(v) for v in extreme_draws())
    e = torch.empty(5, P).exponential_(generator=gen).clamp_(1e-3, 12.0)
    e[0, P // 2] = lo
    e[1, P // 3] = hi
    e[2, P - 1], e[2, 1] = lo, hi
    e[3, 0] = lo
    return e


def topk_reference(scores, e, k, tau):
    from oracle import vit as OV
    ref_mask, ref_index = OV.patch_topk_mask(scores.clone(), e, k, tau)
    y_ref = ((F.log_softmax(scores, -1) - e.log()) / tau).softmax(-1)          # the reference's float32 y_soft
    return ref_mask.detach(), ref_index, y_ref


def distinct_rows(y_ref, k):
    """The production-shape test's predicate (tests/test_kernels_gpu.py): the boundary pair differs and sits in the normal float32 range."""
    ys = y_ref.sort(-1, descending=True)[0]
    return (ys[:, k - 1] > ys[:, k]) & (ys[:, k] > 1e-35)


def decided(scores, e, k, tau):
    """Every row's k-th reference y_soft is at least 1e-5 (relative) above the (k+1)-th, and the whole row is normal float32."""
    ys = ((F.log_softmax(scores, -1) - e.log()) / tau).softmax(-1).sort(-1, descending=True)[0]
    return bool(((ys[:, k - 1] >= ys[:, k] * (1 + 1e-5)) & (ys[:, -1] > 1e-30)).all())


def run_topk(scores, e, k, tau, pad=32):
    """uvc_patch_topk_mask into sentinel-filled parents: (mask, y_soft, softmax(scores)) on the host, the device y_soft / p_soft for backward."""
    from uvc_amd import ops
    B, P = scores.shape
    parents = [torch.full((B * P + pad,), SENT, device=dev()) for _ in range(3)]
    mask, ys, ps = (p[:B * P].view(B, P) for p in parents)
    ops.patch_topk_mask(scores.to(dev()), e.to(dev()), mask, ys, ps, B, P, k, float(tau))
    torch.cuda.synchronize()
    for p in parents:
        assert bool((p[B * P:] == SENT).all()), "written past the last row"
    return mask.cpu(), ys.cpu(), ps.cpu(), ys, ps


def check_topk(scores, e, k, tau, what, launch_after_check=True):
    """Forward and backward of one launch against oracle/vit.py and float64, no row excluded.  The boundary condition on the inputs is asserted
    before the launch; ``launch_after_check=False`` (inputs that hold device draws) looks at the outputs' finiteness first."""
    from uvc_amd import ops
    B, P = scores.shape
    ref_mask, ref_index, y_ref = topk_reference(scores, e, k, tau)
    inner = 1 <= k <= P - 1
    if inner and launch_after_check:
        assert bool(distinct_rows(y_ref, k).all()), f"{what}: the inputs tie at the k-th boundary in the reference"
    mask, ys, ps, ys_d, ps_d = run_topk(scores, e, k, tau)
    for name, t in (("mask", mask), ("y_soft", ys), ("softmax(scores)", ps)):
        assert bool(torch.isfinite(t).all()), f"{what}: {name} is not finite in rows {torch.nonzero(~torch.isfinite(t).all(1)).flatten().tolist()}"
    if inner:
        assert bool(distinct_rows(y_ref, k).all()), f"{what}: the inputs tie at the k-th boundary in the reference"
    hard = torch.zeros(B, P).scatter_(1, ref_index, 1.0) > 0.5
    assert int(hard.sum()) == B * min(k, P)
    hard[:, 0] = True                                                           # token 0 is forced to 1 after the scatter
    sel = mask > 0.5
    bad = [int(r) for r in range(B) if not torch.equal(sel[r], hard[r])]
    assert not bad, f"{what}: index sets differ from the reference in rows {bad}"
    assert bool((mask[:, 0] == 1.0).all()), f"{what}: token 0 is not exactly 1"
    torch.testing.assert_close(mask, ref_mask, rtol=0, atol=2e-6, msg=lambda m: f"{what} mask: {m}")
    s64 = scores.double().requires_grad_(True)
    y64 = ((F.log_softmax(s64, -1) - e.double().log()) / tau).softmax(-1)
    torch.testing.assert_close(ys.double(), y64.detach(), rtol=2e-5, atol=1e-30, msg=lambda m: f"{what} y_soft: {m}")
    torch.testing.assert_close(ps.double(), F.softmax(s64, -1).detach(), rtol=2e-5, atol=1e-30, msg=lambda m: f"{what} softmax(scores): {m}")
    g = torch.Generator().manual_seed(B * 4099 + P)
    dmask = torch.randn(B, P, generator=g)
    dm = dmask.clone().double()
    dm[:, 0] = 0                                                                # token 0 has no gradient
    (y64 * dm).sum().backward()
    parent = torch.full((B * P + 32,), SENT, device=dev())
    ds = parent[:B * P].view(B, P)
    ops.patch_topk_mask_bwd(dmask.to(dev()), ys_d, ps_d, ds, B, P, float(tau))
    torch.cuda.synchronize()
    assert bool((parent[B * P:] == SENT).all())
    torch.testing.assert_close(ds.cpu().double(), s64.grad, rtol=5e-4, atol=3e-6 / min(tau, 1.0), msg=lambda m: f"{what} d(scores): {m}")
    return mask, ys, ps, ds.cpu()


@pytest.mark.parametrize("tau", [1.0, 2.0])
@pytest.mark.parametrize("P", [196, 576])
def test_patch_topk_at_the_extreme_draws(P, tau):
    """A Gumbel value of 16.64 (the smallest draw) puts its token first whatever its score; -2.85 (the largest) all but last."""
    k = int(0.9 * P)
    for attempt in range(50):                                                   # ordinary rows and tokens: a decided boundary, as in topk_inputs
        g = torch.Generator().manual_seed(900 + P + 7919 * attempt)
        scores = torch.randn(5, P, generator=g) * 1.5
        e = planted(P, g)
        if not bool(torch.isfinite(e.log()).all()) or decided(scores, e, k, tau):
            break
    mask, ys, _, _ = check_topk(scores, e, k, tau, f"P={P} tau={tau}", launch_after_check=False)
    assert bool(mask[0, P // 2] > 0.5) and bool(mask[2, P - 1] > 0.5)           # the smallest draw's token is among the kept nine tenths


def gate_inputs_with(e, seed):
    """tests/test_small_kernels_gpu.py's construction on given draws: the second logit is placed so that |u0 - u1| >= 1e-3 in every block."""
    Lb = e.shape[0]
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(Lb, 2, generator=gen)
    gap = torch.exp(torch.empty(Lb).uniform_(math.log(1.2e-3), math.log(3.0), generator=gen)) * (torch.randint(0, 2, (Lb,), generator=gen) * 2 - 1)
    free = torch.tensor([i >= 8 for i in range(Lb)])                            # rows with a planted draw keep their own logits: the draw decides
    g[free, 1] = (g[free, 0].double() + gap[free].double() / 2 + (e[free, 1].double().log() - e[free, 0].double().log())).float()
    return g


@pytest.mark.parametrize("mode", [1, 3])
def test_gate_distrib_at_the_extreme_draws(mode):
    from uvc_amd import ops
    Lb = 12
    lo, hi = (float(v) for v in extreme_draws())
    gen = torch.Generator().manual_seed(41)
    e = torch.empty(Lb, 2).exponential_(generator=gen).clamp_min(1e-3)
    for row, (a, b) in enumerate([(lo, None), (None, lo), (hi, None), (None, hi), (lo, hi), (hi, lo), (lo, lo), (hi, hi)]):
        if a is not None:
            e[row, 0] = a
        if b is not None:
            e[row, 1] = b
    g = gate_inputs_with(e, 42)
    u = SR.gate_logits_ref(g, e)
    d = torch.full((Lb + 4, 2), float("nan"), device=dev())
    ops.gate_distrib(g.to(dev()), e.to(dev()), d[:Lb], Lb, mode, 0.1)
    got = d.cpu()
    assert bool(torch.isnan(got[Lb:]).all())
    got = got[:Lb]
    assert bool(torch.isfinite(got).all()), f"mode {mode}: gates not finite in rows {torch.nonzero(~torch.isfinite(got).all(1)).flatten().tolist()}"
    assert bool(torch.isfinite(u).all()), f"the reference's logits are not finite: a draw of {lo!r}"        # mode 3 hides it: inf > x is decided
    assert bool(((u[:, 0] - u[:, 1]).abs() >= 1e-3).all())
    want = SR.gate_distrib_ref(g, e, mode, 0.1)
    if mode == 3:
        assert torch.equal(got.double(), want)
        assert [got[i].tolist() for i in (0, 1, 4, 5)] == [[1, 0], [0, 1], [1, 0], [0, 1]]      # the smallest draw wins (16.64 against <= 6.91)
    else:
        torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(got.sum(-1), torch.ones(Lb), rtol=0, atol=2e-7)


def test_dual_step_at_the_extreme_draws():
    """uvc_dual_step through the engine-accuracy harness (scores, prox, ranks and the state phase, every bound of that file) on DeiT-Tiny's
    dims with Gumbel gates, the extreme draws planted in e1 (srloss2's sample) and e2 (zloss's): alone, in both columns, and both in one row.
    The conditions that make that harness's equal-bits demands fair (tests/test_uvc_engine_refs_cpu.py) are asserted on the oracle first."""
    import test_uvc_engine_accuracy_gpu as EA
    import uvc_engine_refs as R
    lo, hi = (float(v) for v in extreme_draws())
    assert lo > 0 and math.isfinite(hi), f"the smallest draw is {lo!r}: its Gumbel value is {-np.log(np.float64(lo))!r}, which no step of the oracle survives"
    plants = {0: [(0, 0, lo), (1, 1, lo), (2, 0, hi), (3, 1, hi), (4, 0, lo), (4, 1, hi), (5, 0, hi), (5, 1, lo)],     # exp draw number -> (row, col, value)
              1: [(0, 1, lo), (1, 0, hi), (6, 0, lo), (6, 1, hi), (11, 0, lo), (11, 1, lo)]}

    class PlantedRun(R.OracleRun):
        n_exp = 0

        def draw(self, shape, kind="exp"):
            t = super().draw(shape, kind)
            if kind == "exp":
                for row, col, v in plants[self.n_exp % 2]:
                    t[row, col] = v
                self.n_exp += 1
            return t

    run = next(r for r in R.RUNS if r.case == "tiny" and r.mode == "gumbel" and (r.wfam, r.sfam, r.clip) == ("gaussian", "interior", "in"))
    L, H, hd, F_ = run.dims
    recs = list(PlantedRun(run).steps(conditions=True))
    assert min(r.clip_margin for r in recs) >= R.MARGIN and min(r.int_margin for r in recs) >= R.MARGIN
    assert min(r.round_margin for r in recs) >= R.ROUND_MARGIN and all(r.inside for r in recs)
    for r in recs:
        assert float(r.e1.min()) == lo and float(r.e1.max()) == hi and float(r.e2.min()) == lo
        for v in ("s", "r", "y", "p", "z", "gate", "gsum"):
            assert bool(torch.isfinite(r.ref[v]).all()), f"the oracle's {v} is not finite at step {r.step}: a draw of zero"
        assert math.isfinite(r.ref["cur"]) and math.isfinite(r.ref["R2"])
    orun = PlantedRun(run)
    eng = R.Engine(L, H, hd, F_, orun.weights.W1, orun.weights.W3, orun.state0, run.seed, orun.gate0)
    smax, rmax = R.box_max(L, H, hd, F_)
    for rec in orun.steps():
        what = f"{run.id} planted, step {rec.step}"
        eng.y.copy_(rec.pre.y)
        eng.p.copy_(rec.pre.p)
        rk_pre = EA.score_phase(eng, rec.W1_pre, rec.W3_pre, rec.sc_pre, what)
        EA.prox_phase(eng, rec, rk_pre, what)
        got = EA.state_phase(eng, run, rec, smax, rmax, what)
        for k_, t in got.items():
            if k_ != "gmom" or rec.ref["mom"] is not None:
                assert bool(torch.isfinite(t.double()).all()), f"{what}: {k_} is not finite"
        assert bool(torch.isfinite(eng.gate).all()), f"{what}: the gates are not finite"


# ============================================================================= patch top-k at its edges
TOPK_P = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024]


def topk_ks(P):
    return sorted({0, 1, int(0.9 * P), P - 1, P})


def topk_inputs(B, P, k, tau, seed):
    """Scores and draws whose reference y_soft separates the k-th from the (k+1)-th in every row by at least 1e-5 relative (about 80 float32 ulps:
    what a kernel whose expf / logf are good to 1 ulp can be held to bit for bit, and the size of the gap row 0 gets) with the whole row normal
    float32.  Row 0's (k+1)-th u is then moved to 64 float32 ulps (>= 2e-5) below the k-th, as in the production-shape test.  The seed walks upwards
    until every row qualifies: a property of the inputs alone, settled before any launch."""
    inner = 1 <= k <= P - 1
    for attempt in range(50):
        g = torch.Generator().manual_seed(seed + 7919 * attempt)
        scores = torch.randn(B, P, generator=g) * 1.5
        e = torch.empty(B, P).exponential_(generator=g).clamp_(1e-3, 12.0)
        if inner:
            logp = F.log_softmax(scores[0].double(), -1)
            u = (logp - e[0].double().log()) / tau
            order = torch.argsort(u, descending=True)
            a, b = int(order[k - 1]), int(order[k])
            gap = max(2e-5, 64.0 * abs(float(u[a])) * 2.0 ** -23)
            e[0, b] = torch.exp(-((u[a] - gap) * tau - logp[b])).float()
        if not inner or decided(scores, e, k, tau):
            return scores, e
    raise AssertionError(f"no inputs with a decided boundary for B={B} P={P} k={k} tau={tau}")


@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("P", TOPK_P)
def test_patch_topk_edges(P, tau):
    for B in (1, 3):
        for k in topk_ks(P):
            what = f"B={B} P={P} k={k} tau={tau}"
            scores, e = topk_inputs(B, P, k, tau, 5000 + 31 * P + 7 * k + B)
            mask, ys, ps, _ = check_topk(scores, e, k, tau, what)
            if k == 0:
                assert bool((mask[:, 1:] <= 2e-6).all()), f"{what}: k = 0 selects a token besides token 0"
            if k >= P:
                assert bool((mask > 0.5).all()), f"{what}: k = P leaves a token out"
            n_sel = (mask[:, 1:] > 0.5).sum(1)
            assert bool(((n_sel == min(k, P)) | (n_sel == min(k, P) - 1)).all()), f"{what}: not k tokens per image"


@pytest.mark.parametrize("P", TOPK_P)
def test_patch_topk_rows_do_not_depend_on_the_batch(P):
    """Each row of a B = 3 launch against the same row alone (B = 1): the same bits in all three outputs and in d(scores)."""
    from uvc_amd import ops
    k, tau = max(1, int(0.9 * P)), 1.0
    scores, e = topk_inputs(3, P, min(k, max(P - 1, 0)), tau, 8000 + P)
    g = torch.Generator().manual_seed(8100 + P)
    dmask = torch.randn(3, P, generator=g)

    def both(sc, ee, dm):
        Bn = sc.shape[0]
        mask, ys, ps, ys_d, ps_d = run_topk(sc, ee, k, tau)
        ds = torch.full((Bn, P), SENT, device=dev())
        ops.patch_topk_mask_bwd(dm.to(dev()), ys_d, ps_d, ds, Bn, P, tau)
        return mask, ys, ps, ds.cpu()

    whole = both(scores, e, dmask)
    for r in range(3):
        alone = both(scores[r:r + 1].contiguous(), e[r:r + 1].contiguous(), dmask[r:r + 1].contiguous())
        for name, a, b in zip(("mask", "y_soft", "softmax(scores)", "d(scores)"), alone, whole):
            assert torch.equal(a[0].view(torch.int32), b[r].view(torch.int32)), f"P={P} row {r}: {name} depends on the batch"


def test_patch_topk_refusals_write_nothing():
    from uvc_amd import _lib as L
    B = 2
    src = torch.full((B * 1025,), 0.5, device=dev())
    outs = [torch.full((B * 1025,), SENT, device=dev()) for _ in range(4)]
    p, s = L.ptr, L.cur_stream()
    fwd = lambda P, k, tau: L.lib().uvc_patch_topk_mask(p(src), p(src), p(outs[0]), p(outs[1]), p(outs[2]), B, P, k, tau, s)
    bwd = lambda P, tau: L.lib().uvc_patch_topk_mask_bwd(p(src), p(src), p(src), p(outs[3]), B, P, tau, s)
    for what, rc in (("P = 0", fwd(0, 0, 1.0)), ("P = 1025", fwd(1025, 10, 1.0)), ("tau = 0", fwd(196, 176, 0.0)), ("tau < 0", fwd(196, 176, -1.0)),
                     ("k < 0", fwd(196, -1, 1.0)), ("B = 0", L.lib().uvc_patch_topk_mask(p(src), p(src), p(outs[0]), p(outs[1]), p(outs[2]), 0, 196, 176, 1.0, s)),
                     ("null e", L.lib().uvc_patch_topk_mask(p(src), 0, p(outs[0]), p(outs[1]), p(outs[2]), B, 196, 176, 1.0, s)),
                     ("bwd P = 0", bwd(0, 1.0)), ("bwd P = 1025", bwd(1025, 1.0)), ("bwd tau = 0", bwd(196, 0.0))):
        assert rc == 1 and L.lib().uvc_last_error(), what
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == SENT).all())
    assert fwd(1024, 921, 1.0) == 0 and bwd(1024, 1.0) == 0                     # the largest P is taken
    torch.cuda.synchronize()
    assert bool((outs[0][:B * 1024] != SENT).all()) and bool((outs[0][B * 1024:] == SENT).all())


def test_worst_figures_are_reported():
    """A report, not a check (every figure was asserted where it was measured): the largest logf ordinal distance this process has seen."""
    for name, v in WORST.items():
        print(f"{name}: {v}")
