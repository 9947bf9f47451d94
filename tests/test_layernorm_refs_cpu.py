"""CPU: tests/layernorm_refs.py accepts an honest float32 LayerNorm and rejects subtly wrong ones, and the cases of
tests/test_layernorm_accuracy_gpu.py keep the promises their exactness claims rest on.

The honest kernel is simulated in float32: every row sum as per-lane sequential sums followed by a pairwise lane tree, in the layouts of
layernorm.hip -- 16, 32 or 64 lanes per row with four adjacent elements per lane and step (where 4 * lanes divides D), one 64-lane wave with
elements lane + 64 i (any D) -- and as plain torch.float32 ops (the odd widths too); dgamma / dbeta as 16 sequential row slots per block of 32
rows, a slot tree, and four sequential block slices.  It must stay below HONEST_RATIO = 0.5 of every bound at every (D, family) the GPU module
uses; the INTEGER family must come out bit for bit.  Each mutant is that simulation with one defect; the families that must reject it:

    unbiased variance                      RANDOM, EDGE      (rstd, y)
    one-pass variance E[x^2] - mean^2      EDGE              (rstd of the 1e4 + N(0,1) and the 3 + 1e-4 N(0,1) rows)
    eps = 1e-5                             EDGE              (rstd of the tiny-variance and constant rows)
    eps omitted                            EDGE              (the constant / zero rows: rstd infinite)
    mean over the padded 128 columns, D=100  RANDOM, EDGE
    the last column dropped                RANDOM, EDGE
    a tail row taking its neighbour's statistics   RANDOM, EDGE
    c1 without / D                         RANDOM, EDGE      (INTEGER rows have c1 = c2 = 0: blind to it by construction)
    c2 term dropped                        RANDOM, EDGE
    a2 applied to add1                     RANDOM, EDGE, INTEGER
    dots from the rounded bf16 dx          RANDOM at rows = 1, D <= 192: with n = rows D terms the any-order bound 2 (n + 4) u S lies below one bf16
                                           rounding per term (rms ~ 2^-9 S / sqrt(n)) only while n^1.5 < 2^14 (INTEGER dx is exact in bf16: blind;
                                           EDGE: the 1e15 rows' S drowns it)
    beta_acc ignored                       RANDOM, EDGE, INTEGER
    the last row of a block missing from dgamma    INTEGER   (RANDOM / EDGE: inside the any-order bound at small row counts or not, not relied on)
    the last block missing from the reduction      INTEGER
    dbeta summing gy instead of dy         RANDOM, EDGE, INTEGER

Run with -s to see the worst honest ratio per family and the smallest ratio of every mutant."""
import pytest
import torch

import layernorm_refs as R
import test_layernorm_accuracy_gpu as G

HONEST_RATIO = 0.5
F32T, BF16T = torch.float32, torch.bfloat16
WIDTHS = sorted({D for _, D in G.PATHS})
SIM_ROWS = 173


def f32(t):
    return t.to(torch.float32)


def layouts(D):
    return [("vec", L) for L in (16, 32, 64) if D % (4 * L) == 0] + [("gen", 64), ("plain", 0)]


def lane_sum(v, layout, cols=None):
    """float32 row sums of v [rows, D] in one of the layouts; cols: number of leading columns that count (the last-column-dropped mutant)."""
    kind, L = layout
    rows, D = v.shape
    if cols is not None:
        v = v.clone()
        v[:, cols:] = 0.0
    if kind == "plain":
        return v.sum(-1)
    if kind == "vec":
        per = v.view(rows, D // (4 * L), L, 4).permute(0, 2, 1, 3).reshape(rows, L, -1)
    else:
        nv = -(-D // 64)
        pad = torch.zeros(rows, 64 * nv, dtype=torch.float32)
        pad[:, :D] = v
        per = pad.view(rows, nv, 64).permute(0, 2, 1)
    s = torch.zeros(rows, per.shape[1], dtype=torch.float32)
    for i in range(per.shape[2]):
        s = s + per[:, :, i]
    while s.shape[1] > 1:
        half = s.shape[1] // 2
        s = s[:, :half] + s[:, half:]
    return s[:, 0]


def sim_fwd(x, gamma, beta, layout, yT, mutate=None):
    """x: float32 [rows, D] as the kernel receives it.  Returns y (yT), mean, rstd (float32)."""
    rows, D = x.shape
    eps = torch.tensor({"eps_1e-5": 1e-5, "eps_0": 0.0}.get(mutate, R.EPS), dtype=torch.float32)
    cols = D - 1 if mutate == "drop_last_col" else None
    n = torch.tensor(float(128 if mutate == "padded_mean" else D), dtype=torch.float32)
    mean = lane_sum(x, layout, cols) / n
    d = x - mean[:, None]
    if mutate == "one_pass":
        var = lane_sum(x * x, layout) / n - mean * mean
    else:
        var = lane_sum(d * d, layout, cols) / (n - 1 if mutate == "unbiased" else n)
    rstd = torch.rsqrt(var + eps)
    if mutate == "tail_stats":
        mean, rstd = mean.clone(), rstd.clone()
        mean[-1], rstd[-1] = mean[-2], rstd[-2]
    y = (x - mean[:, None]) * rstd[:, None] * gamma + beta
    return y.to(yT), mean, rstd


def col_sum(t, rpb=32, mutate=None):
    """[rows, n] -> [n]: per-block partials (16 row slots in sequence, a slot tree), then four block slices in sequence."""
    rows, n = t.shape
    nb = -(-rows // rpb)
    pad = torch.zeros(nb * rpb, n, dtype=torch.float32)
    pad[:rows] = t
    if mutate == "drop_block_row":
        pad[rpb - 1::rpb] = 0.0
    p = pad.view(nb, rpb // 16, 16, n)
    s = torch.zeros(nb, 16, n, dtype=torch.float32)
    for i in range(p.shape[1]):
        s = s + p[:, i]
    while s.shape[1] > 1:
        half = s.shape[1] // 2
        s = s[:, :half] + s[:, half:]
    part = s[:, 0]
    if mutate == "drop_last_block" and nb > 1:
        part = part[:-1]
    sl = []
    for k in range(4):
        acc = torch.zeros(n, dtype=torch.float32)
        for b in range(k, part.shape[0], 4):
            acc = acc + part[b]
        sl.append(acc)
    return ((sl[0] + sl[1]) + sl[2]) + sl[3]


def sim_bwd(o, mean, rstd, layout, *, xT=F32T, dyT=F32T, gT=F32T, add1=True, add2=True, scalars=True, beta_acc=0.0, mutate=None):
    """The backward on the operands `o` of R.make_bwd (rounded to the stream types first).  Returns (inputs as received, outputs)."""
    x, dy = f32(o["x"].to(xT)), f32(o["dy"].to(dyT))
    ad1, ad2 = (f32(o["add1"].to(gT)) if add1 else None), (f32(o["add2"].to(gT)) if add2 else None)
    gamma, D = o["gamma"], o["D"]
    a1, a2 = (torch.tensor(v if scalars else 1.0, dtype=torch.float32) for v in (o["a1"], o["a2"]))
    invD = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(D), dtype=torch.float32)
    xh, gy = (x - mean[:, None]) * rstd[:, None], dy * gamma
    c1 = lane_sum(gy, layout) * (1.0 if mutate == "c1_no_invD" else invD)
    c2 = lane_sum(gy * xh, layout) * invD
    dx = rstd[:, None] * (gy - c1[:, None] - (0.0 if mutate == "c2_dropped" else xh * c2[:, None]))
    if ad1 is not None:
        dx = dx + (a2 if mutate == "a2_on_add1" else a1) * ad1
    if ad2 is not None:
        dx = dx + a2 * ad2
    dx_out = dx.to(gT)
    dsrc = f32(dx_out) if mutate == "dots_rounded" else dx
    dotA = col_sum(lane_sum(dsrc * x, layout)[:, None])[0]
    dotB = col_sum(lane_sum(ad2 * x, layout)[:, None])[0] if ad2 is not None else torch.zeros(())
    ba = 0.0 if mutate == "beta_acc_ignored" else beta_acc
    dg = col_sum(dy * xh, mutate=mutate) + (ba * o["dg_old"] if ba else 0.0)
    db = col_sum(gy if mutate == "dbeta_gy" else dy, mutate=mutate if mutate == "drop_last_block" else None) + (ba * o["db_old"] if ba else 0.0)
    return dict(x=x, dy=dy, add1=ad1, add2=ad2), dict(dx=dx_out, dgamma=dg, dbeta=db, dots=torch.stack([dotA, dotB]))


def stats_for(o, xT):
    if o["family"] == R.INTEGER:
        return o["mean"], o["rstd"]
    st = R.fwd_reference(o["x"].to(xT), o["gamma"], o["gamma"])
    return st["mean"].float(), st["rstd"].float()


def judge_bwd(o, layout, *, mutate=None, **kw):
    mean, rstd = stats_for(o, kw.get("xT", F32T))
    ins, outs = sim_bwd(o, mean, rstd, layout, mutate=mutate, **kw)
    ref = R.bwd_reference(ins["x"], ins["dy"], o["gamma"], mean, rstd, add1=ins["add1"], a1=o["a1"] if kw.get("scalars", True) else None,
                          add2=ins["add2"], a2=o["a2"] if kw.get("scalars", True) else None, beta_acc=kw.get("beta_acc", 0.0),
                          dg_old=o["dg_old"], db_old=o["db_old"])
    return R.bwd_accept(outs["dx"], outs["dgamma"], outs["dbeta"], outs["dots"], ref, exact=o["family"] == R.INTEGER)


def judge_fwd(family, D, layout, xT, yT, mutate=None, rows=SIM_ROWS):
    x = f32(R.make_x(family, rows, D).to(xT))
    gamma, beta = R.make_params(D)
    y, mean, rstd = sim_fwd(x, gamma, beta, layout, yT, mutate)              # (eps omitted: an infinite rstd is a rejection -- "not finite")
    return R.fwd_accept(y, mean, rstd, R.fwd_reference(x, gamma, beta))


# ----------------------------------------------------------------------------- honest
@pytest.mark.parametrize("D", WIDTHS)
def test_honest_forward_stays_below_half_of_every_bound(D):
    worst = {}
    for family in (R.RANDOM, R.EDGE):
        for layout in layouts(D):
            for xT, yT in ((F32T, F32T), (BF16T, BF16T), (F32T, BF16T)):
                fails, ratios = judge_fwd(family, D, layout, xT, yT)
                assert not fails, (D, family, layout, fails)
                for k, v in ratios.items():
                    worst[(family, k)] = max(worst.get((family, k), 0.0), v)
    print(f"honest forward D={D}: " + ", ".join(f"{f} {k} {v:.3f}" for (f, k), v in sorted(worst.items())))
    assert max(worst.values()) < HONEST_RATIO, worst


@pytest.mark.parametrize("D", WIDTHS)
def test_honest_backward_stays_below_half_of_every_bound_and_integer_is_exact(D):
    worst = {}
    for family in (R.RANDOM, R.EDGE, R.INTEGER):
        o = R.make_bwd(family, SIM_ROWS, D)
        for layout in layouts(D):
            for kw in (dict(), dict(xT=BF16T, dyT=BF16T, gT=BF16T, beta_acc=0.5), dict(dyT=BF16T, add1=False, scalars=False, beta_acc=1.0)):
                fails, ratios = judge_bwd(o, layout, **kw)
                assert not fails, (D, family, layout, kw, fails)
                for k, v in ratios.items():
                    worst[(family, k)] = max(worst.get((family, k), 0.0), v)
    print(f"honest backward D={D}: " + ", ".join(f"{f} {k} {v:.3f}" for (f, k), v in sorted(worst.items())))
    assert max(v for (f, _), v in worst.items() if f != R.INTEGER) < HONEST_RATIO, worst
    assert all(v == 0.0 for (f, _), v in worst.items() if f == R.INTEGER), worst


def test_honest_column_sums_over_many_blocks():
    """dgamma / dbeta / dots through 78 blocks (2469 rows) at D = 64 and 100."""
    for D in (64, 100):
        for family in (R.RANDOM, R.EDGE, R.INTEGER):
            o = R.make_bwd(family, 2469, D)
            fails, ratios = judge_bwd(o, ("gen", 64), beta_acc=0.5)
            assert not fails, (D, family, fails)
            assert max(ratios.values()) < (HONEST_RATIO if family != R.INTEGER else 1e-30), (D, family, ratios)


# ----------------------------------------------------------------------------- mutants
FWD_MUTANTS = {"unbiased": (R.RANDOM, R.EDGE), "one_pass": (R.EDGE,), "eps_1e-5": (R.EDGE,), "eps_0": (R.EDGE,), "padded_mean": (R.RANDOM, R.EDGE),
               "drop_last_col": (R.RANDOM, R.EDGE), "tail_stats": (R.RANDOM, R.EDGE)}
BWD_MUTANTS = {"c1_no_invD": (R.RANDOM, R.EDGE), "c2_dropped": (R.RANDOM, R.EDGE), "a2_on_add1": (R.RANDOM, R.EDGE, R.INTEGER),
               "dots_rounded": (R.RANDOM,), "beta_acc_ignored": (R.RANDOM, R.EDGE, R.INTEGER), "drop_block_row": (R.INTEGER,),
               "drop_last_block": (R.INTEGER,), "dbeta_gy": (R.RANDOM, R.EDGE, R.INTEGER)}


def _mutant_ratio(fails, ratios):
    return max(ratios.values()) if ratios else float("inf")


@pytest.mark.parametrize("mutate", list(FWD_MUTANTS))
def test_forward_mutants_are_rejected(mutate):
    smallest = float("inf")
    for D in ((100,) if mutate == "padded_mean" else (64, 100, 192, 320, 768, 1024)):
        for family in FWD_MUTANTS[mutate]:
            layout = ("gen", 64) if D % 64 else ("vec", 16)
            fails, ratios = judge_fwd(family, D, layout, F32T, F32T, mutate)
            assert fails, (mutate, D, family, "accepted", ratios)
            smallest = min(smallest, _mutant_ratio(fails, ratios))
    print(f"mutant {mutate}: smallest worst-element ratio over its families and widths {smallest:.3g}")
    assert smallest > 1.0


@pytest.mark.parametrize("mutate", list(BWD_MUTANTS))
def test_backward_mutants_are_rejected(mutate):
    smallest = float("inf")
    for D in ((40, 64, 100, 192) if mutate == "dots_rounded" else (64, 100, 192, 320, 768)):
        for family in BWD_MUTANTS[mutate]:
            kw = dict(beta_acc=0.5)
            layout = ("gen", 64) if D % 64 else ("vec", 16)
            if mutate == "dots_rounded":
                # the defect is a random rounding error per term: one row of D terms, five draws, rejected in most of them
                res = [judge_bwd(R.make_bwd(family, 1, D, seed=s), layout, mutate=mutate, gT=BF16T, **kw) for s in range(5)]
                assert sum(bool(f) for f, _ in res) >= 3, (mutate, D, family, [r for _, r in res])
                smallest = min(smallest, sorted(_mutant_ratio(f, r) for f, r in res)[2])
                continue
            o = R.make_bwd(family, SIM_ROWS, D)
            fails, ratios = judge_bwd(o, layout, mutate=mutate, **kw)
            assert fails, (mutate, D, family, "accepted", ratios)
            smallest = min(smallest, _mutant_ratio(fails, ratios))
    print(f"mutant {mutate}: smallest worst-element ratio (INTEGER: absolute difference) over its families and widths {smallest:.3g}")


# ----------------------------------------------------------------------------- the GPU module's cases
def test_integer_cases_stay_exact_in_float32():
    """Every INTEGER case of the GPU module: sum |terms| / quantum < 2^24 for c1, c2, dgamma and dbeta; `dots` too wherever the case claims it
    (G.dots_exact is the same predicate the GPU test applies, and must not be vacuous: some cases claim it, the largest fall back)."""
    seen, claims = set(), []
    cases = [(D, c) for path, D in G.PATHS for c in G.bwd_cases(path, D)] + [(G.DEFER_D, dict(G.defer_case(i)[0], beta_acc=0.5)) for i in range(13)]
    for D, c in cases:
        key = (D, c["rows"], c["add1"], c["add2"], c["scalars"], c["beta_acc"])
        if c["family"] != R.INTEGER or key in seen:
            continue
        seen.add(key)
        mags = R.integer_magnitudes(G._bwd_operands(R.INTEGER, c["rows"], D), add1=c["add1"], add2=c["add2"], scalars=c["scalars"], beta_acc=c["beta_acc"])
        assert all(v < 2 ** 24 for k, v in mags.items() if k != "dots"), (key, mags)
        claims.append(G.dots_exact(c, D))
        assert claims[-1] == (mags["dots"] < 2 ** 24)
    assert any(claims) and not all(claims), (sum(claims), len(claims))
    print(f"INTEGER cases: {len(claims)} distinct, dots exact in {sum(claims)}")


def test_case_tables_reach_what_they_name():
    from uvc_amd import _lib as L
    lib = L.lib()
    assert [lib.uvc_layernorm_bwd_nblocks(r) for r in (2016, 2017, 2469, 49151, 49152, 49217)] == [63, 64, 78, 1536, 768, 770]
    for nbk, rows in G.DEFER_ROWS.items():
        assert lib.uvc_layernorm_bwd_nblocks(rows) == nbk, (rows, nbk)
    assert [-(-D // 64) <= nv for D, nv in zip(G.GEN_WIDTHS, G.GEN_NV)] == [True] * 8
    for path, D in G.PATHS:
        b = G.bwd_cases(path, D)
        assert {(c["xT"], c["dyT"], c["gT"]) for c in b} == set(G.TYPE_COMBOS)
        for rows in G.BWD_ROWS + G.BWD_ROWS_BIG + (G.BWD_ROWS_RPB if (path, D) == ("vector", 64) else ()):
            fams = {c["family"] for c in b if c["rows"] == rows}
            assert R.INTEGER in fams and (R.EDGE in fams or R.RANDOM in fams), (path, D, rows, fams)
        assert {c["beta_acc"] for c in b} == {0.0, 0.5, 1.0} and {c["dots"] for c in b} == {0, 1} and {c["scalars"] for c in b} == {0, 1}
        assert {(c["add1"], c["add2"]) for c in b} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        if path != "generic_by_stride":
            assert {c["rpg"] for c in b} == {0, 1, 2}, (path, D)
        f = G.fwd_cases(path, D)
        assert {(c["xT"], c["yT"], c["rows"]) for c in f} >= {(x, y, r) for x in (F32T, BF16T) for y in (F32T, BF16T) for r in G.FWD_ROWS}
    for rows in G.FWD_ROWS + G.BWD_ROWS + G.BWD_ROWS_BIG + G.BWD_ROWS_RPB:
        m = G.prefix_rows(rows)
        assert (m == 0 and rows < 4) or (0 < m < rows and m % 4), (rows, m)
