"""CPU: the harness of tests/uvc_engine_refs.py does what it claims, and every case of tests/test_uvc_engine_accuracy_gpu.py meets, on the oracle
alone, the conditions under which that file may ask for equal bits without skipping anything:

  clip indicator     | |R - budget| - z_grad_clip | >= 1e-3 at every step, with runs on both sides;
  integers           every updated s, r is exactly on a bound or at least 1e-3 from an integer (a step moves s or r by at most its learning rate --
                     the gradient is clipped to infinity-norm 1 -- and two correct float32 evaluations of that increment differ by about 2^-23 of it);
  hard Gumbel gap    |y1 - y0| >= 1e-3 in every layer of the hard = 1 evaluations;
  rounding           no float64 score sum, before or after prox, within 1e-12 relative of a float32 rounding boundary: the engine's float64 sums
                     differ from the oracle's by summation order only (n * 2^-53 relative), so both round to the same float32 and every rank,
                     index set and shrunk weight follows bit for bit.
"""
import numpy as np
import pytest
import torch

import uvc_engine_refs as R
from oracle import uvc as OU

def layer_scores(W, H, hd, l):
    s1, s2 = OU.scores_w1(W.W1[l], H, hd)
    return s1.reshape(-1).numpy(), s2.numpy(), OU.scores_w3(W.W3[l]).numpy()


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
@pytest.mark.parametrize("wfam", ["exact", "constant", "staircase"])
def test_exact_families_have_float32_exact_sums(case, wfam):
    """Column and head sums of squares are whole numbers of 2^-8 below 2^24: float32 sums in two orders equal the float64 sum bit for bit."""
    _, L, H, hd, F = case
    W = R.make_weights(wfam, L, H, hd, F, 1)
    for l in (0, L - 1):
        for M in (W.W1[l], W.W3[l]):
            q = (M.double() * 16) ** 2
            assert bool((q == q.round()).all())
            col64 = (M.double() ** 2).sum(0)
            assert float(col64.max()) * 256 * (hd if M is W.W1[l] else 1) < 2 ** 24
            fwd = torch.zeros(M.shape[1])
            for row in M:                                         # strictly sequential float32 accumulation, then the reverse order
                fwd = fwd + row * row
            rev = torch.zeros(M.shape[1])
            for row in M.flip(0):
                rev = rev + row * row
            assert torch.equal(fwd.double(), col64) and torch.equal(rev.double(), col64)
        s1, s2 = OU.scores_w1(W.W1[l], H, hd)
        assert torch.equal(s1.sum(1).double(), (W.W1[l].double() ** 2).sum(0).view(H, hd).sum(1)) and torch.equal(s2, s1.sum(1))


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_families_tie_where_they_claim(case):
    _, L, H, hd, F = case
    D = H * hd
    for l in (0, L - 1):
        g = layer_scores(R.make_weights("gaussian", L, H, hd, F, 1), H, hd, l)
        assert all(R.tie_count(v) <= v.size // 100 for v in g)      # float32 coincidences only (18 of 8192 at F = 8192), none below F = 1024
        W = R.make_weights("exact", L, H, hd, F, 1)
        for step in range(2):                                     # the ties survive the between-step perturbation
            s1, s2, s3 = layer_scores(W, H, hd, l)
            for h in range(H):
                assert R.tie_count(s1[h * hd:(h + 1) * hd]) >= 4, (h, step)                   # 0 == 1, 3 == 5, 9 == 10 == 0.0
                assert s1[h * hd + 9] == 0 and s1[h * hd + 10] == 0
            assert R.tie_count(s3) >= 16 + 3 + F // 8 and not s3[F // 4:F // 4 + F // 8].any() and s3[F - 1] == s3[0]
            if H >= 2:
                assert s2[H - 1] == 0 and not s1[(H - 1) * hd:].any()
            if H >= 3:
                assert R.tie_count(s2) >= 2 and s2[0] == s2[1]
            W.perturb(np.random.default_rng(5))
        c1, c2, c3 = layer_scores(R.make_weights("constant", L, H, hd, F, 1), H, hd, l)
        assert R.tie_count(c1) == D and R.tie_count(c3) == F and (H == 1 or R.tie_count(c2) == H)
        r1, rh, r3 = R.group_ranks(c1, c2, c3, H, hd)
        assert np.array_equal(r1, np.tile(np.arange(hd), H)) and np.array_equal(rh, np.arange(H)) and np.array_equal(r3, np.arange(F))
    W = R.make_weights("staircase", L, H, hd, F, 1)
    dirs = set()
    for l in range(min(L, 2)):
        s1, s2, s3 = layer_scores(W, H, hd, l)
        for v in (s1, s3) + ((s2,) if H > 1 else ()):
            d = np.diff(v)
            assert (d > 0).all() or (d < 0).all()
        dirs |= {("proj", bool(s1[1] > s1[0])), ("fc2", bool(s3[1] > s3[0]))}
    assert {d for _, d in dirs} == {True, False}                   # descending and ascending both occur in every case


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
@pytest.mark.parametrize("wfam", R.WEIGHT_FAMILIES)
def test_lexsort_rule_is_the_oracles_least_k(case, wfam):
    """rank < k is oracle.least_k's index set for every k that matters, ties included (fmax is the case whose gaussian fc2 scores tie)."""
    name, L, H, hd, F = case
    W = R.make_weights(wfam, L, H, hd, F, 2)
    W.perturb(np.random.default_rng(2))
    for l in (0, L - 1):
        s1, s2, s3 = layer_scores(W, H, hd, l)
        for v in [s1[h * hd:(h + 1) * hd] for h in range(H)] + [s2, s3]:
            rk, n = R.lexsort_rank(v), v.size
            naive = np.array([int(((v < v[i]) | ((v == v[i]) & (np.arange(n) < i))).sum()) for i in range(n)]) if n <= 512 else rk
            assert np.array_equal(rk, naive) and np.array_equal(np.sort(rk), np.arange(n))
            for k in sorted({0, 1, n // 3, n // 2, n - 1, n}):
                assert np.array_equal(OU.least_k(torch.from_numpy(v), k)[0].numpy(), rk < k), (wfam, l, k)
        assert not (name == "fmax" and wfam == "gaussian") or R.tie_count(s3) > 0


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_state_families(case):
    _, L, H, hd, F = case
    smax, rmax = (t.numpy() for t in R.box_max(L, H, hd, F))
    assert smax[0, 0] == H - 1 and smax[0, 1] == F - 1 and rmax[0, 0] == hd - 1                # k = ceil(max) = n - 1 in every group
    for fam in R.STATE_FAMILIES:
        for flip in (0, 1):
            st = R.make_state(fam, L, H, hd, F, 0, flip)
            assert (st["s"] >= 0).all() and (st["s"] <= smax).all() and (st["r"] >= 0).all() and (st["r"] <= rmax).all(), fam
            assert (st["y"] >= 0).all() and (st["p"] >= 0).all() and st["z"] >= 0
    z = R.make_state("zero", L, H, hd, F, 0)
    assert not z["s"].any() and not z["r"].any() and np.all(z["y"] == np.float32(1e-3)) and np.all(z["p"] == np.float32(1e-3))
    d = R.make_state("dual_floor", L, H, hd, F, 0)
    assert not d["y"].any() and not d["p"].any() and d["z"] > 0
    b = [R.make_state("bounds", L, H, hd, F, 0, f) for f in ((0,) if L > 1 else (0, 1))]
    for j in (0, 1):
        col = np.concatenate([x["s"][:, j] for x in b])
        assert (col == 0).any() and (col == smax[0, j]).any() and ((col == 0) | (col == smax[0, j])).all()
    rr = np.concatenate([x["r"].ravel() for x in b])
    assert (rr == 0).any() and (rr == rmax[0, 0]).any() and ((rr == 0) | (rr == rmax[0, 0])).all()
    i = [R.make_state("integers", L, H, hd, F, 0, f) for f in ((0,) if L > 1 else (0, 1))]
    for vals in ([np.concatenate([x["s"][:, 1] for x in i]), np.concatenate([x["r"].ravel() for x in i])]
                 + ([np.concatenate([x["s"][:, 0] for x in i])] if H >= 3 else [])):
        whole = vals == np.round(vals)
        above = ~whole
        assert whole.any() and above.any() and (vals[whole] >= 1).all()
        assert np.array_equal(np.nextafter(np.floor(vals[above]), np.float32(np.inf)), vals[above])      # integer + one ulp: ceil is one more
        assert np.array_equal(np.ceil(vals[above]), np.floor(vals[above]) + 1)


ALL_RUNS = R.RUNS + R.SCHEDULE_RUNS + R.OVERBOX_RUNS


@pytest.mark.parametrize("run", ALL_RUNS, ids=[r.id for r in ALL_RUNS])
def test_run_meets_the_conditions(run):
    c = R.oracle_run(run)
    assert c["clip"] >= R.MARGIN, c
    assert c["integer"] >= R.MARGIN, c
    assert c["rounding"] >= R.ROUND_MARGIN, c
    assert all(c["inside"]) if run.clip == "in" else not any(c["inside"]), c
    if run.sfam == "dual_floor":
        assert c["z"][0] == 0.0                                    # z lands on its clamp in the first step


def test_plan_covers_what_the_gpu_file_claims():
    ids = [r.id for r in ALL_RUNS]
    assert len(set(ids)) == len(ids)
    for name, L, H, hd, F in R.CASES:
        mine = [r for r in R.RUNS if r.case == name]
        assert {r.wfam for r in mine} == set(R.WEIGHT_FAMILIES) and {r.sfam for r in mine} == set(R.STATE_FAMILIES)
        assert {r.clip for r in mine} == {"in", "out"} and {r.mode for r in mine} == set(R.MODES)
        assert all(4 <= r.steps <= 7 for r in mine)
        if L == 1:
            assert {r.flip for r in mine if r.sfam == "bounds"} == {0, 1}
    assert {r.mode for r in R.RUNS if r.case in ("l17", "l32")} == set(R.MODES)
    for run in R.SCHEDULE_RUNS:                                     # accumulate-only, first and second application all occur
        cnt = R.oracle_run(run)["counters"]
        assert run.step0 == 0 and run.steps == 7
        applied = [i for i in range(7) if (i + 1) % run.interval == 0]
        assert len(applied) >= 2 and cnt[applied[0]] == (0, 1) and cnt[-1] == (7 % run.interval, 1)
        if run.interval > 1:
            assert cnt[0] == (1, 0)                                 # a step that only accumulates, before any momentum exists


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_auxiliary_inputs_meet_the_conditions(case):
    """The masks, resource and warm-up tests: score sums off the rounding boundaries, hard Gumbel samples decided by more than 1e-3."""
    name, L, H, hd, F = case
    for kind in ("masks", "resource"):
        W = R.make_weights("gaussian", L, H, hd, F, R.aux_seed(kind, name))
        assert min(R.rounding_margin(torch.cat(x).numpy()) for x in R.scores64(W.W1, W.W3, H, hd)) >= R.ROUND_MARGIN, kind
    gate, draws = R.resource_draws(name)
    assert R.gumbel_gap(gate, draws[1]) >= R.MARGIN
    states = R.mask_states(L, H, hd, F, 11)
    k = [np.ceil(s["s"][:, 1]) for s in states]
    assert (k[1] < k[0]).any() and (k[2] > k[0]).any() and k[1][0] == 0 and k[2][L - 1] == F - 1
    for s in states:
        for v in (s["s"], s["r"]):
            free = (v != 0) & (v != np.round(v))
            assert (np.abs(v - np.round(v))[free] >= 0.2).all()
    if name in R.WARMUP_CASES:
        rec = next(R.OracleRun(R.warmup_run(name)).steps(warmup=1, conditions=True))
        assert rec.round_margin >= R.ROUND_MARGIN
