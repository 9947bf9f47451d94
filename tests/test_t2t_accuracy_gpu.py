"""GPU: every kernel of uvc_amd/csrc/t2t.hip against the float64 references and acceptance rules of tests/t2t_refs.py -- the soft split with
LayerNorm (forward and backward), the fold, the Performer's linear attention (forward and backward) and the stage sequenced in C.

Soft split.  GEOMS names one geometry per dispatch class and layout edge: NV 3 / NV 9 x generic / channel-fast (CF: token-major, C = 64), H != W
everywhere, NCHW and token-major sources, C = 32 token-major (generic with sc = 1), dim = 192 (the NV class edge), s > k (pixels no window covers),
p >= k (rows wholly in the padding).  Every geometry runs float32, bf16 and bf16-compute with float32 out / dy; ldo = dim (where 8 divides it),
roundup(dim, 32), roundup(dim, 64); plain and with LayerNorm; beta_acc 0 / 1 / 0.5; dxu given, null and tap-major; RANDOM everywhere, EDGE and
INTEGER where s >= k, INTSUM everywhere.  TRIP_GEOMS are the 224-class shapes whose grid-stride loops run twice (backward 18816 rows at NV 3, 8624
at NV 9; 1568 rows = 392 blocks for the reduce; forward 263424 and 131712 rows, judged on SAMPLE rows: the first 64, the last 64, 2048 seeded).
Fold.  Natural and tap-major order, every source x destination type pair, lds = dim and dim + 8 (the gap holds NaN), integer sources bit for bit
against float64, and the adjoint identity <unfold(x), g> = <x, fold(g)> in float64 on the device results, inside 2 (k k + 4) u <|x|, fold|g|>.
Performer.  T in PERF_T (1 .. 3136: partial tiles of every 16-row remainder, 448 / 449 / 897 = one split, a split of one token, three splits),
B 1 and 3, the three type combinations, dskip given and null; RANDOM at every T, SPIKE at every position of t2t_refs.SPIKE_AT inside T, RANGE at
65 and 449.  kptv, ksum, att, dkptv, dksum, dk, dq, dv each against its own bound.
Every call: outputs prefilled with NaN; guard rows behind every output, behind `partial` (sized exactly by unfold_bwd_blocks) and behind `part`
(sized exactly by performer_splits) keep their bytes; a second call gives the same bytes; the first B - 1 images alone give the same bytes as
inside the batch -- out, mean, rstd, dxu, the fold, and every Performer output.  dgamma / dbeta are left out of that last comparison: they
sum over the batch.

The case tables are walked without a GPU by tests/test_t2t_refs_cpu.py (honest simulation below half of every bound, INTEGER accumulators below
2^24 quanta, RANGE finite in float32, every dispatch class reached).
Measured on an MI355X: 55 tests in 5 s, the slowest 1.2 s (the first one, which loads the library), every other below 0.25 s; worst error / bound
per output in test_worst_ratios_are_reported's docstring (the largest 0.45, dv of a SPIKE token: one rounding of dskip + dv against u |dv|)."""
import functools

import pytest
import torch

import layernorm_refs as LR
import t2t_refs as R

pytestmark = pytest.mark.gpu

F32T, BF16T = torch.float32, torch.bfloat16
GEOMS = {  # name: (B, C, H, W, k, s, p, token_major)
    "nv3_image": (2, 3, 20, 28, 7, 4, 2, False),
    "nv3_one_row": (1, 3, 7, 7, 7, 4, 2, False),
    "nv3_dim192": (3, 3, 9, 13, 8, 3, 0, False),
    "nv9_image392": (2, 8, 12, 9, 7, 2, 3, False),
    "nv9_k14": (1, 1, 20, 17, 14, 3, 0, False),
    "nv9_tokens_c32": (2, 32, 6, 10, 3, 2, 1, True),
    "nv3cf_k1": (2, 64, 5, 9, 1, 1, 0, True),
    "nv3cf_k1_s2": (2, 64, 5, 9, 1, 2, 0, True),
    "nv9cf_321": (2, 64, 9, 14, 3, 2, 1, True),
    "nv9cf_7x7": (1, 64, 7, 7, 3, 2, 1, True),
    "nv9cf_k2": (2, 64, 6, 10, 2, 2, 0, True),
    "nv9cf_s_gt_k": (2, 64, 8, 8, 3, 4, 1, True),
    "nv9cf_p_ge_k": (1, 64, 4, 6, 2, 3, 2, True),
}
CLASSES = {(3, False): ("nv3_image", "nv3_one_row", "nv3_dim192"), (9, False): ("nv9_image392", "nv9_k14", "nv9_tokens_c32"),
           (3, True): ("nv3cf_k1", "nv3cf_k1_s2"), (9, True): ("nv9cf_321", "nv9cf_7x7", "nv9cf_k2", "nv9cf_s_gt_k", "nv9cf_p_ge_k")}
TRIP_GEOMS = {
    "bwd_trips_nv3": (6, 3, 224, 224, 7, 4, 2, False),            # 18816 rows: two trips of 1024 x 16
    "bwd_trips_nv9": (11, 64, 56, 56, 3, 2, 1, True),             # 8624 rows: two trips of 1024 x 8
    "bwd_reduce_392": (2, 64, 56, 56, 3, 2, 1, True),             # 1568 rows = 392 blocks: 24.5 per sixteenth
    "fwd_trips_nv3": (84, 3, 224, 224, 7, 4, 2, False),           # 263424 rows: two trips of 16384 x 16
    "fwd_trips_nv9": (168, 64, 56, 56, 3, 2, 1, True),            # 131712 rows: two trips of 16384 x 8
}
FOLD_GEOMS = dict({n: v for n, v in GEOMS.items() if v[1] == 64}, nv9_tokens_c32=GEOMS["nv9_tokens_c32"],
                  fold_ragged=(2, 64, 5, 7, 3, 2, 1, True), fold_ragged_k2s1=(2, 64, 5, 7, 2, 1, 1, True))      # 70 pixels: a last group of 8 holds 6
TYPES = [(F32T, F32T), (BF16T, BF16T), (BF16T, F32T)]      # (compute dtype, element type of out / dy / att / the gradient streams)
FOLD_TYPES = [(F32T, F32T, F32T), (BF16T, F32T, F32T), (BF16T, BF16T, F32T), (BF16T, F32T, BF16T), (BF16T, BF16T, BF16T)]   # (dtype, src, dst)
BETAS = (0.0, 1.0, 0.5)
DXU = ("given", "null", "tap")
PERF_T = (1, 15, 16, 17, 63, 64, 65, 200, 448, 449, 897, 3136)
PERF_B = (1, 3)
RANGE_T = (65, 449)
STAGE = (2, 64, 10, 10, 3, 2, 1, True)
SAMPLE_SEEDED = 2048
WORST = {}


def geom(name):
    return R.geometry(*{**GEOMS, **TRIP_GEOMS, **FOLD_GEOMS}[name])


def fwd_cases(name):
    g = geom(name)
    fams = [R.RANDOM] + ([R.EDGE] if g["disjoint"] else [])
    return [dict(dtype=dt, outT=oT, ldo=ldo, family=f, ln=ln) for dt, oT in TYPES for ldo in R.ldo_choices(g["dim"]) for f in fams for ln in (True, False)]


def bwd_cases(name):
    g = geom(name)
    fams = [R.RANDOM, R.INTSUM] + ([R.EDGE, R.INTEGER] if g["disjoint"] else [])
    ldos, out = R.ldo_choices(g["dim"]), []
    for dt, dyT in TYPES:
        for mode in (DXU if g["c_fast"] else DXU[:2]):
            for f in fams:
                k = len(out)
                out.append(dict(dtype=dt, dyT=dyT, dxu=mode, family=f, ldo=ldos[k % len(ldos)], beta_acc=BETAS[(k // len(ldos)) % 3]))
    return out


def trip_bwd_cases(name):
    g = geom(name)
    ldo = -(-g["dim"] // 32) * 32
    return [dict(dtype=BF16T, dyT=BF16T, dxu="tap" if g["c_fast"] else "given", family=R.INTSUM, ldo=ldo, beta_acc=0.5),
            dict(dtype=F32T, dyT=F32T, dxu="given", family=R.RANDOM, ldo=ldo, beta_acc=1.0)]


def sample_rows(rows):
    """The rows of a large forward that go against float64: the first 64, the last 64 and SAMPLE_SEEDED seeded ones in between."""
    mid = torch.randint(64, rows - 64, (SAMPLE_SEEDED,), generator=torch.Generator().manual_seed(rows))
    return torch.unique(torch.cat([torch.arange(64), mid, torch.arange(rows - 64, rows)]))


def performer_cases(T):
    out = []
    for B in PERF_B:
        for dt, gT in TYPES:
            out.append(dict(B=B, dtype=dt, gT=gT, family=R.RANDOM, spike=None, dskip=len(out) % 2 == 0))
    for pos in R.spike_positions(T):
        k = len(out)
        out.append(dict(B=PERF_B[k % 2], dtype=TYPES[k % 3][0], gT=TYPES[k % 3][1], family=R.SPIKE, spike=pos, dskip=k % 2 == 0))
    if T in RANGE_T:
        for dt, gT in TYPES:
            out.append(dict(B=3, dtype=dt, gT=gT, family=R.RANGE, spike=None, dskip=len(out) % 2 == 0))
    return out


# ----------------------------------------------------------------------------- helpers
def dev():
    return torch.device("cuda")


def nan(*shape, dtype=F32T):
    return torch.full(shape, float("nan"), device=dev(), dtype=dtype)


def code(T):
    from uvc_amd import ops
    return ops.UVC_F32 if T == F32T else ops.UVC_BF16


def bits(t):
    return t.view(torch.int16 if t.dtype == BF16T else torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def note(ratios, key):
    for k, v in ratios.items():
        WORST[(k, key)] = max(WORST.get((k, key), 0.0), v)


def gargs(g):
    return tuple(g[n] for n in ("B", "C", "H", "W", "k", "s", "p"))


def show(c):
    return {k: str(v) for k, v in c.items()}


# ----------------------------------------------------------------------------- soft split forward
@functools.lru_cache(maxsize=4)
def _fwd_operands(name, family):
    return tuple(t.to(dev()) for t in R.make_unfold_fwd(geom(name), family))


def call_unfold_fwd(g, src, c, gamma, beta):
    from uvc_amd import ops
    rows, G = g["rows"], R.GUARD_ROWS
    out, mean, rstd = nan(rows + G, c["ldo"], dtype=c["outT"]), nan(rows + G), nan(rows + G)
    ln = c["ln"]
    ops.unfold_ln_fwd(src, g["strides"], *gargs(g), out, code(c["dtype"]), gamma=gamma if ln else None, beta=beta if ln else None, mean=mean if ln else None,
                      rstd=rstd if ln else None, eps=R.LN_EPS)
    return out, mean, rstd


def check_unfold_fwd(g, src, c, gamma, beta, res, what, rows_idx=None):
    out, mean, rstd = res
    rows, dim = g["rows"], g["dim"]
    assert bool(torch.isnan(out[rows:].float()).all()) and bool(torch.isnan(mean[rows:]).all()) and bool(torch.isnan(rstd[rows:]).all()), (what, "guard rows written")
    assert float(out[:rows, dim:].float().abs().max()) == 0.0 if c["ldo"] > dim else True, (what, "columns [dim, ldo) are not zero")
    sel = slice(0, rows) if rows_idx is None else rows_idx.to(dev())
    x = R.unfold_rows(src, g, rows=rows_idx)
    if not c["ln"]:
        assert torch.equal(out[sel, :dim], x.to(c["outT"])), (what, "the plain soft split is not the gather")
        assert bool(torch.isnan(mean).all()) and bool(torch.isnan(rstd).all()), (what, "statistics written without LayerNorm")
        return
    assert bool(torch.isfinite(out[:rows].float()).all()), (what, "rows not written")
    ref = R.ln_fwd_reference(x, gamma, beta, g["nv"])
    fails, ratios = LR.fwd_accept(out[sel, :dim], mean[sel], rstd[sel], ref)
    note({"unfold fwd " + k: v for k, v in ratios.items()}, c["family"])
    assert not fails, (what, fails)


@pytest.mark.parametrize("name", list(GEOMS))
def test_soft_split_forward_against_float64(name):
    g = geom(name)
    for c in fwd_cases(name):
        what = (name, show(c))
        src, gamma, beta = _fwd_operands(name, c["family"])
        res = call_unfold_fwd(g, src, c, gamma, beta)
        check_unfold_fwd(g, src, c, gamma, beta, res, what)
        again = call_unfold_fwd(g, src, c, gamma, beta)
        assert all(same(p, q) for p, q in zip(res, again)), (what, "not deterministic")
        if g["B"] > 1:
            gb = R.with_batch(g, g["B"] - 1)
            part = call_unfold_fwd(gb, src[:R.source_numel(gb)].contiguous(), c, gamma, beta)
            assert all(same(p[:gb["rows"]], q[:gb["rows"]]) for p, q in zip(part, res)), (what, "rows depend on the batch size")


@pytest.mark.parametrize("name", ["fwd_trips_nv3", "fwd_trips_nv9"])
def test_soft_split_forward_second_grid_stride_trip(name):
    """More rows than 16384 workgroups take in one trip; bf16 out; LayerNorm against float64 on the sampled rows, the plain split on all rows."""
    g = geom(name)
    assert R.fwd_trips(g)[0] == 2
    src, gamma, beta = (t.to(dev()) for t in R.make_unfold_fwd(g, R.RANDOM))
    sample = sample_rows(g["rows"])
    for ln in (True, False):
        c = dict(dtype=BF16T, outT=BF16T, ldo=-(-g["dim"] // 32) * 32, family=R.RANDOM, ln=ln)
        res = call_unfold_fwd(g, src, c, gamma, beta)
        check_unfold_fwd(g, src, c, gamma, beta, res, (name, ln), rows_idx=sample if ln else None)
        again = call_unfold_fwd(g, src, c, gamma, beta)
        assert all(same(p, q) for p, q in zip(res, again)), (name, ln, "not deterministic")
        del res, again


# ----------------------------------------------------------------------------- soft split + LayerNorm backward
@functools.lru_cache(maxsize=4)
def _bwd_operands(name, family):
    return R.make_unfold_bwd(geom(name), family)


def bwd_inputs(name, g, c):
    o = _bwd_operands(name, c["family"])
    t = dict(src=o["src"].to(dev()), gamma=o["gamma"].to(dev()), dg_old=o["dg_old"].to(dev()), db_old=o["db_old"].to(dev()))
    t["dy"] = torch.zeros(g["rows"], c["ldo"], device=dev(), dtype=c["dyT"])
    t["dy"][:, :g["dim"]] = o["dy"].to(c["dyT"]).to(dev())
    t["x"] = R.unfold_rows(t["src"], g)
    if c["family"] in (R.INTEGER, R.INTSUM):
        t["mean"], t["rstd"] = o["mean"].to(dev()), o["rstd"].to(dev())
    else:
        st = R.ln_fwd_reference(t["x"], t["gamma"], t["gamma"], g["nv"])
        t["mean"], t["rstd"] = st["mean"].float(), st["rstd"].float()
    return t


def call_unfold_bwd(g, t, c):
    from uvc_amd import ops
    rows, dim, G = g["rows"], g["dim"], R.GUARD_ROWS
    nb = ops.unfold_bwd_blocks(rows)
    assert nb == R.bwd_blocks(rows)
    partial = nan(nb * 2 * dim + G * dim)
    dg = torch.cat([t["dg_old"], torch.full((G,), R.SENTINEL, device=dev())])
    db = torch.cat([t["db_old"], torch.full((G,), R.SENTINEL, device=dev())])
    dxu = None if c["dxu"] == "null" else nan(rows + G, dim)
    ops.unfold_ln_bwd(t["src"][:R.source_numel(g)], g["strides"], *gargs(g), t["dy"][:rows], code(c["dtype"]), gamma=t["gamma"], mean=t["mean"][:rows], rstd=t["rstd"][:rows],
                      partial=partial, dgamma=dg, dbeta=db, dxu=dxu, beta_acc=c["beta_acc"], eps=R.LN_EPS, dxu_tap_major=c["dxu"] == "tap")
    return dict(partial=partial, dgamma=dg, dbeta=db, dxu=dxu, nb=nb)


def natural(dxu, g, c):
    """dxu [rows, dim] in natural column order, whichever order the call wrote."""
    if c["dxu"] != "tap":
        return dxu
    return dxu.reshape(-1, g["kk"], g["C"]).transpose(1, 2).reshape(-1, g["dim"])


def check_unfold_bwd(g, t, c, out, what):
    rows, dim = g["rows"], g["dim"]
    assert bool(torch.isnan(out["partial"][out["nb"] * 2 * dim:]).all()), (what, "scratch past unfold_bwd_blocks(rows) written")
    for n in ("dgamma", "dbeta"):
        assert bool((out[n][dim:] == R.SENTINEL).all()), (what, n, "guard written")
    ref = R.ln_bwd_reference(t["x"], t["dy"][:, :dim], t["gamma"], t["mean"], t["rstd"], g["nv"], c["beta_acc"], t["dg_old"], t["db_old"])
    fam = c["family"]
    fails, ratios = LR.bwd_accept(None, out["dgamma"][:dim], out["dbeta"][:dim], None, ref, exact=fam in (R.INTEGER, R.INTSUM))
    if out["dxu"] is not None:
        assert bool(torch.isnan(out["dxu"][rows:]).all()), (what, "dxu guard rows written")
        f2, r2 = LR.bwd_accept(natural(out["dxu"][:rows], g, c), None, None, None, ref, exact=fam == R.INTEGER)
        fails, ratios = fails + f2, dict(ratios, **r2)
    note({"unfold bwd " + k: v for k, v in ratios.items() if "exact" not in k}, fam)
    assert not fails, (what, fails)


def run_unfold_bwd(name, cases):
    g = geom(name)
    for c in cases:
        what = (name, show(c))
        t = bwd_inputs(name, g, c)
        out = call_unfold_bwd(g, t, c)
        check_unfold_bwd(g, t, c, out, what)
        again = call_unfold_bwd(g, t, c)
        for n in ("dgamma", "dbeta", "partial") + (("dxu",) if c["dxu"] != "null" else ()):
            assert same(out[n], again[n]), (what, n, "not deterministic")
        if g["B"] > 1 and c["dxu"] != "null":
            gb = R.with_batch(g, g["B"] - 1)
            part = call_unfold_bwd(gb, t, c)
            assert same(part["dxu"][:gb["rows"]], out["dxu"][:gb["rows"]]), (what, "dxu rows depend on the batch size")


@pytest.mark.parametrize("name", list(GEOMS))
def test_soft_split_backward_against_float64(name):
    run_unfold_bwd(name, bwd_cases(name))


@pytest.mark.parametrize("name", ["bwd_trips_nv3", "bwd_trips_nv9", "bwd_reduce_392"])
def test_soft_split_backward_second_grid_stride_trip(name):
    """dgamma / dbeta accumulated over two grid-stride trips (and 392 partial blocks through the sixteen-way reduce): INTSUM bit for bit."""
    g = geom(name)
    assert R.bwd_trips(g)[0] == (1 if name == "bwd_reduce_392" else 2)
    run_unfold_bwd(name, trip_bwd_cases(name))


# ----------------------------------------------------------------------------- fold
def call_fold(g, src, dstT, dtype, tap):
    from uvc_amd import ops
    n = g["B"] * g["H"] * g["W"]
    dst = nan(n + R.GUARD_ROWS, g["C"], dtype=dstT)
    ops.fold_tokens(src, dst, *gargs(g), code(dtype), lds=src.shape[1], tap_major=tap)
    assert bool(torch.isnan(dst[n:].float()).all()), "fold: guard rows written"
    return dst[:n].view(g["B"], g["H"] * g["W"], g["C"])


@pytest.mark.parametrize("name", list(FOLD_GEOMS))
def test_fold_integer_sources_bit_for_bit_and_adjoint(name):
    from uvc_amd import ops
    g = geom(name)
    rows, dim = g["rows"], g["dim"]
    vals = torch.randint(-8, 9, (rows, dim), generator=torch.Generator().manual_seed(dim + rows)).float().to(dev())
    ref = R.fold(vals, g)
    if g["s"] > g["k"]:
        assert bool((ref == 0).any())
    for dtype, srcT, dstT in FOLD_TYPES:
        got = {}
        for tap in ((False, True) if g["C"] == 64 else (False,)):
            for lds in (dim, dim + 8):
                src = nan(rows, lds, dtype=srcT)
                src[:, :dim] = (R.to_tap_major(vals, g) if tap else vals).to(srcT)
                got[(tap, lds)] = call_fold(g, src, dstT, dtype, tap)
                assert torch.equal(got[(tap, lds)].double(), ref), (name, str(srcT), str(dstT), tap, lds, "differs from float64")
                if g["B"] > 1:
                    gb = R.with_batch(g, g["B"] - 1)
                    assert same(call_fold(gb, src[:gb["rows"]].contiguous(), dstT, dtype, tap), got[(tap, lds)][:gb["B"]].contiguous()), (name, "depends on the batch")
        first = next(iter(got.values()))
        assert all(same(v, first) for v in got.values()), (name, "natural and tap-major order differ")
    # <unfold(x), gr> = <x, fold(gr)> on the device results, float64 sums; fold's float32 sums have at most k k terms each
    gen = torch.Generator().manual_seed(rows)
    x, gr = torch.randn(R.source_numel(g), generator=gen).to(dev()), torch.randn(rows, dim, generator=gen).to(dev())
    unf = nan(rows, dim)                                               # (every fold geometry has 8 | dim)
    ops.unfold_ln_fwd(x, g["strides"], *gargs(g), unf, ops.UVC_F32)
    xt = x.view(g["B"], g["H"] * g["W"], g["C"]).double()
    for tap in ((False, True) if g["C"] == 64 else (False,)):
        fd = call_fold(g, (R.to_tap_major(gr, g) if tap else gr).contiguous(), F32T, F32T, tap)
        lhs, rhs = float((unf.double() * gr.double()).sum()), float((xt * fd.double()).sum())
        E = 2.0 * (g["kk"] + 4) * R.U * float((xt.abs() * R.fold(gr.abs(), g)).sum())
        note({"fold adjoint": abs(lhs - rhs) / E}, "random")
        assert abs(lhs - rhs) <= E, (name, tap, lhs, rhs, E)


# ----------------------------------------------------------------------------- Performer
@functools.lru_cache(maxsize=4)
def _perf_operands(family, B, T, spike):
    return R.make_performer(family, B, T, spike=spike)


def call_performer(c, T, B):
    """Forward and backward on the first B images of the case's operands; every buffer with its guard."""
    from uvc_amd import ops
    o = _perf_operands(c["family"], c["B"], T, c["spike"])
    G, gT, S = R.GUARD_ROWS, c["gT"], ops.performer_splits(B, T)
    assert S == R.performer_splits(T)
    kqv, w = o["kqv"][:B].reshape(B * T, 192).contiguous().to(dev()), o["w"].to(dev())
    datt = o["datt"][:B].reshape(B * T, 64).to(gT).contiguous().to(dev())
    dskip = o["dskip"][:B].reshape(B * T, 64).to(gT).contiguous().to(dev()) if c["dskip"] else None
    r = dict(kqv=kqv, w=w, datt=datt, dskip=dskip, n_part=B * S * 65 * 32, part=nan(B * S * 65 * 32 + G * 32), part2=nan(B * S * 65 * 32 + G * 32),
             kptv=nan(B * 65 + G, 32), dkptv=nan(B * 65 + G, 32), att=nan(B * T + G, 64, dtype=gT), dkqv=nan(B * T + G, 192, dtype=gT))
    ops.performer_fwd(kqv, w, r["part"], r["kptv"], r["att"], B, T, code(c["dtype"]))
    ops.performer_bwd(kqv, w, r["part2"], r["kptv"], datt, r["dkqv"], r["dkptv"], B, T, code(c["dtype"]), dskip=dskip)
    return r


PERF_OUT = ("kptv", "att", "dkptv", "dkqv")


@pytest.mark.parametrize("T", PERF_T)
def test_performer_against_float64(T):
    for c in performer_cases(T):
        B, what = c["B"], (T, show(c))
        r = call_performer(c, T, B)
        for n in ("part", "part2"):
            assert bool(torch.isnan(r[n][r["n_part"]:]).all()), (what, n, "scratch past performer_splits written")
        for n, rows in (("kptv", B * 65), ("dkptv", B * 65), ("att", B * T), ("dkqv", B * T)):
            assert bool(torch.isnan(r[n][rows:].float()).all()), (what, n, "guard rows written")
        ref = R.performer_reference(r["kqv"].view(B, T, 192), r["w"], r["datt"].view(B, T, 64), None if r["dskip"] is None else r["dskip"].view(B, T, 64))
        fails, ratios = [], {}
        for n, rk in (("kptv", "kptv"), ("dkptv", "dkptv")):
            got = r[n][:B * 65].view(B, 65, 32)
            R.accept(n, got[:, :64], ref[rk][:, :64], fails, ratios)
            R.accept(n.replace("kptv", "ksum"), got[:, 64], ref[rk][:, 64], fails, ratios)
        R.accept("att", r["att"][:B * T].view(B, T, 64), ref["att"], fails, ratios)
        dk = r["dkqv"][:B * T].view(B, T, 192)
        for i, n in enumerate(("dk", "dq", "dv")):
            R.accept(n, dk[:, :, 64 * i:64 * i + 64], ref["dkqv"][:, :, 64 * i:64 * i + 64], fails, ratios)
        note({"performer " + k: v for k, v in ratios.items()}, c["family"])
        assert not fails, (what, fails)
        again = call_performer(c, T, B)
        assert all(same(r[n], again[n]) for n in PERF_OUT), (what, "not deterministic")
        if B > 1:
            b = B - 1
            part = call_performer(c, T, b)
            for n, rows in (("kptv", b * 65), ("dkptv", b * 65), ("att", b * T), ("dkqv", b * T)):
                assert same(part[n][:rows], r[n][:rows]), (what, n, "an image's result depends on the batch size")


# ----------------------------------------------------------------------------- the stage sequenced in C
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_stage_in_c_gives_the_bytes_of_the_separate_calls(precision):
    """uvc_t2t_stage_forward / _backward on 2 x 64 x 10 x 10, k 3, s 2, p 1 (25 tokens per image) against the same launches issued one by one
    (T2T_ViT's front_in_c = False path): every forward buffer, every gradient stream, dxu and the parameter gradients bit for bit."""
    from uvc_amd.t2t_vit import T2T_ViT
    B, C_, H, W, k, s, p, _ = STAGE
    torch.manual_seed(11)
    m = T2T_ViT(img_size=64, num_classes=16, embed_dim=128, depth=2, num_heads=2, mlp_ratio=3.0, token_dim=64, precision=precision)
    m.train()
    m._refresh_front_shadows()
    gen = torch.Generator().manual_seed(12)
    src = torch.randn(B, H * W, C_, generator=gen).to(dev())
    snaps = []
    for in_c in (True, False):
        m.front_in_c = in_c
        m._front_bufs = {}
        size, m._cfg.img_size = m._cfg.img_size, 4 * H             # sizes the second stage's buffers for a 10 x 10 token map; only that stage is run
        bufs = m._front_buffers(B, True)
        m._cfg.img_size = size
        b = bufs["attention2"]
        assert b["T"] == 25
        for v in b.values():
            if torch.is_tensor(v):
                v.fill_(float("nan"))
        b["dout"].copy_(torch.randn(B * 25, 64, generator=torch.Generator().manual_seed(13)).to(b["dout"].dtype))
        m._flat_grad.zero_()
        strides = (H * W * C_, 1, W * C_, C_)
        m._performer_forward("attention2", src, strides, B, C_, H, W, k, s, p, b, True, bufs)
        m._performer_backward("attention2", src, strides, B, C_, H, W, k, s, p, b, bufs, True)
        torch.cuda.synchronize()
        snaps.append(({n: v.clone() for n, v in b.items() if torch.is_tensor(v)}, m._flat_grad.clone()))
    (bc, gc), (bp, gp) = snaps
    assert set(bc) == set(bp)
    for n in bc:
        if n not in ("part", "ln1_partial", "ln2_partial"):
            assert bool(torch.isfinite(bc[n].float()).all()), (n, "not written")
        assert torch.equal(bits(bc[n]) if bc[n].dtype != torch.uint8 else bc[n], bits(bp[n]) if bp[n].dtype != torch.uint8 else bp[n]), (n, "stage in C differs")
    assert torch.equal(gc, gp) and float(gc.abs().sum()) > 0


def test_worst_ratios_are_reported():
    """Prints the worst error / bound per output and family over the cases above (run last; -s shows it).  The rules themselves assert <= 1.

    Measured on an MI355X, worst over all cases [RANDOM / EDGE or SPIKE / RANGE] -- beside it the honest CPU simulation of tests/test_t2t_refs_cpu.py:
        soft split forward   y 0.16 [0.16 / 0.09]   mean 0.07 [0.04 / 0.07]   rstd 0.23 [0.23 / 0.23]           simulation: y 0.16, mean 0.08, rstd 0.23
        soft split backward  dxu 0.32 [0.32 / 0.19, INTSUM 0.09]   dgamma 0.13 [0.13 / 0.12]   dbeta 0.10     simulation: dxu 0.27, dgamma 0.16, dbeta 0.10
        fold adjoint         0.001
        Performer forward    kptv 0.03   ksum 0.03   att 0.012 [0.01 / 0.01 / 0.01]                              simulation: 0.03, 0.03, 0.015
        Performer backward   dkptv 0.011   dksum 0.004   dk 0.004   dq 0.003   dv 0.45 [0.13 / 0.45 / 0.01]     simulation: 0.011, 0.002, 0.003, 0.004, 0.45
    The Performer bounds are loose by their E_z term (2 (64 + 3) u on the exponent's magnitudes), which an honest kernel uses a fiftieth of; with
    EXPF_ULP = 4 assumed for the device expf, kp's own output (ksum) reaches 0.03 of its bound on the GPU as in the simulation (torch's CPU expf), so
    nothing here suggests the device expf is worse than the assumption.  INTEGER / INTSUM: every plain soft split, fold, dxu (INTEGER), dgamma
    and dbeta bit for bit, two grid-stride trips and 392 partial blocks included."""
    for k in sorted({k for k, _ in WORST}):
        per = {f: v for (n, f), v in WORST.items() if n == k}
        print(f"worst ratio {k}: {max(per.values()):.3f}   " + " ".join(f"{f}:{per[f]:.2f}" for f in sorted(per)))
    assert all(v <= 1.0 for v in WORST.values()), WORST
