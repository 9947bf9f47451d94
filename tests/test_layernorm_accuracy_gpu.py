"""GPU: every kernel of uvc_amd/csrc/layernorm.hip against the float64 references and acceptance rules of tests/layernorm_refs.py (RANDOM and
EDGE rows inside a first-order float32 bound, INTEGER rows bit for bit), at every width class and row edge, plus the fused kernels that compute
the same statistics (uvc_mlp_fused_fwd, uvc_gemm_nt with ln_out) and one model at an engine-accepted width outside the vector table.

Widths.  Vector path: 64, 128, 192, 256, 384, 512, 768 (forward NV4 1 / 2 / 3 / 4 / 6 / 8 / 12 -- 768 is the two-sets-at-a-time PF branch;
backward <1,16> <2,16> <3,16> <2,32> <3,32> <2,64> <3,64>, all eight combinations of x / dy / gradient-stream type).  Generic path (one wave
per row): 40, 100, 130, 200, 320, 576, 1000, 1024 = NV 2, 2, 3, 6, 6, 12, 16, 16, and 64 / 192 forced there by group_stride = D + 2.
Rows.  Forward 1, 64, 197 = 3 * 64 + 5 (a partial block, wave and row set).  Backward 1, 7, 33, 173 = 5 * 32 + 13 (several blocks, a ragged last
one, partial row sets for 16, 32 and 64 lanes per row); 2016 / 2017 = 63 / 64 blocks (one- and two-stage finish); 2469 = 78 blocks (uneven
sixteenths); at D = 64 also 49151 / 49152 / 49217 (32 -> 64 rows per block, a ragged 64-row block).
Every call: outputs prefilled with NaN, 8 guard rows behind each output and a guard behind `partial` sized exactly by layernorm_bwd_blocks(rows)
must keep their bytes, the gaps of a strided stream too; a second call gives the same bytes; the first m rows (m % 4 != 0) equal the call on m rows.

The cases are tables (fwd_cases / bwd_cases) that tests/test_layernorm_refs_cpu.py walks without a GPU: the honest simulation stays below half of
every bound at every (D, family) used here, and every INTEGER case's accumulators stay below 2^24 quanta (`dots` falls back to the bound where not).

uvc_gemm_nt's 384-wide ln_out form exists from 4096 rows up (uvc_gemm_nt_ln_supported), so its 16-row case asserts the refusal with nothing written.
Measured on an MI355X: 50 tests in 15 s, the slowest 1.4 s; worst error / bound per output in test_worst_ratios_are_reported's docstring."""
import ctypes as C
import functools

import pytest
import torch

import layernorm_refs as R

pytestmark = pytest.mark.gpu

F32T, BF16T = torch.float32, torch.bfloat16
VEC_WIDTHS = (64, 128, 192, 256, 384, 512, 768)
GEN_WIDTHS = (40, 100, 130, 200, 320, 576, 1000, 1024)
GEN_NV = (2, 2, 3, 6, 6, 12, 16, 16)
STRIDE_FORCED = (64, 192)
PATHS = [("vector", D) for D in VEC_WIDTHS] + [("generic", D) for D in GEN_WIDTHS] + [("generic_by_stride", D) for D in STRIDE_FORCED]
FWD_ROWS = (1, 64, 197)
BWD_ROWS = (1, 7, 33, 173)
BWD_ROWS_BIG = (2016, 2017, 2469)
BWD_ROWS_RPB = (49151, 49152, 49217)
STREAM_N = 9                                     # strided cases read / write the first rows of each [9, D] group of a [B, 9, D] stream
TYPE_COMBOS = [(x, dy, g) for x in (F32T, BF16T) for dy in (F32T, BF16T) for g in (F32T, BF16T)]
# (add1, add2, dots, scalars a1 / a2 given, beta_acc, rows_per_group of a strided dx: 0 = dense)
VARIANTS = [dict(add1=1, add2=1, dots=1, scalars=1, beta_acc=1.0, rpg=0), dict(add1=0, add2=0, dots=0, scalars=0, beta_acc=0.0, rpg=0),
            dict(add1=1, add2=0, dots=1, scalars=0, beta_acc=0.5, rpg=1), dict(add1=0, add2=1, dots=1, scalars=1, beta_acc=0.0, rpg=2),
            dict(add1=1, add2=1, dots=0, scalars=0, beta_acc=1.0, rpg=0), dict(add1=1, add2=1, dots=1, scalars=1, beta_acc=0.5, rpg=2),
            dict(add1=0, add2=1, dots=1, scalars=0, beta_acc=1.0, rpg=1)]
WORST = {}                                       # output -> worst error / bound seen by this module's cases (reported by the last test)


def prefix_rows(rows):
    """m < rows with m % 4 != 0 (0: no prefix run)."""
    if rows < 4:
        return 0
    m = rows - 3
    return m if m % 4 else m - 1 if (m - 1) % 4 else m + 1


def fwd_cases(path, D):
    """dict(rows, xT, yT, family, rpg, gs): every type pair at every row count, both families; strided class-token reads at D = 192 and 100."""
    out = []
    for rows in FWD_ROWS:
        for k, (xT, yT) in enumerate([(F32T, F32T), (F32T, BF16T), (BF16T, F32T), (BF16T, BF16T)]):
            for family in (R.RANDOM, R.EDGE):
                c = dict(rows=rows, xT=xT, yT=yT, family=family, rpg=0, gs=D)
                if path == "generic_by_stride":
                    c.update(rpg=1, gs=D + 2)
                out.append(c)
    if (path, D) in (("vector", 192), ("generic", 100)):
        for rpg in (1, 2):
            for xT, yT in ((F32T, F32T), (BF16T, BF16T)):
                out.append(dict(rows=5 * rpg, xT=xT, yT=yT, family=R.EDGE, rpg=rpg, gs=STREAM_N * D))
    return out


def bwd_cases(path, D):
    """dict(rows, xT, dyT, gT, family, add1, add2, dots, scalars, beta_acc, rpg, gs).  The small row counts run every type combination (the generic
    widths too: the one-wave-per-row kernel takes a bf16 x and a bf16 gradient stream since the engines hand them over at every embed_dim % 64 == 0),
    both families; the large ones rotate through the combinations; the variants rotate through everything."""
    out, k0 = [], PATHS.index((path, D))
    k = k0
    big = BWD_ROWS_BIG + (BWD_ROWS_RPB if D == 64 and path == "vector" else ())
    for ci, (xT, dyT, gT) in enumerate(TYPE_COMBOS):
        rows_here = list(BWD_ROWS) + [r for bi, r in enumerate(big) if (bi + k0) % 4 == ci % 4]
        for rows in rows_here:
            for family in (R.RANDOM if rows in BWD_ROWS and ci % 3 == 0 else R.EDGE, R.INTEGER):
                v = dict(VARIANTS[k % len(VARIANTS)])
                k += 1
                c = dict(rows=rows, xT=xT, dyT=dyT, gT=gT, family=family, gs=D, **v)
                if path == "generic_by_stride":
                    c.update(rpg=1, gs=D + 2)
                elif c["rpg"] and (rows < c["rpg"] or rows > 173):
                    c["rpg"] = 0
                elif c["rpg"]:
                    c["gs"] = STREAM_N * D
                out.append(c)
    return out


def dev():
    return torch.device("cuda")


def note(ratios, D):
    for k, v in ratios.items():
        WORST[(k, D)] = max(WORST.get((k, D), 0.0), v)


def bits(t):
    return t.view(torch.int16 if t.dtype == BF16T else torch.int32)


def stream_layout(rows, D, rpg, gs):
    """(elements of the stream buffer, element index [rows, D] of every row) as uvc_ln_args addresses rows: row r starts at
    (r / rpg) * gs + (r % rpg) * D; a row count that is no multiple of rpg leaves the last group short."""
    r = torch.arange(rows)
    if not rpg:
        return rows * D, (r * D)[:, None] + torch.arange(D)
    return -(-rows // rpg) * gs, ((r // rpg) * gs + (r % rpg) * D)[:, None] + torch.arange(D)


def to_stream(vals, rows, D, rpg, gs, dtype):
    """A stream buffer holding `vals` ([rows, D] host float32) at its rows and NaN in the gaps."""
    n, idx = stream_layout(rows, D, rpg, gs)
    buf = torch.full((n,), float("nan"), dtype=dtype)
    buf[idx.reshape(-1)] = vals.reshape(-1).to(dtype)
    return buf.to(dev())


def from_stream(buf, rows, D, rpg, gs):
    if not rpg:
        return buf[:rows * D].view(rows, D)
    return buf[stream_layout(rows, D, rpg, gs)[1].to(buf.device)]


def gaps_untouched(buf, rows, D, rpg, gs):
    """Everything of a NaN-prefilled stream buffer outside its rows (the gaps between groups, the guard behind it) is still NaN."""
    gap = torch.ones(buf.numel(), dtype=torch.bool)
    gap[stream_layout(rows, D, rpg, gs)[1].reshape(-1)] = False
    return bool(torch.isnan(buf[gap.to(buf.device)]).all())


# ----------------------------------------------------------------------------- forward
@functools.lru_cache(maxsize=8)
def _fwd_operands(family, rows, D):
    return R.make_x(family, rows, D), R.make_params(D)


def run_fwd(c, D, rows=None):
    from uvc_amd import ops
    full = c["rows"]
    rows = rows or full
    x_h, (gamma, beta) = _fwd_operands(c["family"], full, D)
    x = to_stream(x_h[:rows], rows, D, c["rpg"], c["gs"], c["xT"])
    G = R.GUARD_ROWS
    y = torch.full((rows + G, D), float("nan"), device=dev(), dtype=c["yT"])
    mean, rstd = torch.full((rows + G,), float("nan"), device=dev()), torch.full((rows + G,), float("nan"), device=dev())
    ops.layernorm_fwd(x, gamma.to(dev()), beta.to(dev()), y, mean, rstd, rows, D, ops.UVC_F32 if c["yT"] == F32T else ops.UVC_BF16,
                      rows_per_group=c["rpg"] or 1, group_stride=c["gs"])
    return x, y, mean, rstd, gamma.to(dev()), beta.to(dev())


@pytest.mark.parametrize("path,D", PATHS, ids=[f"{p}-{D}" for p, D in PATHS])
def test_layernorm_forward_against_float64(path, D):
    for c in fwd_cases(path, D):
        rows, what = c["rows"], (path, D, {k: str(v) for k, v in c.items()})
        x, y, mean, rstd, gamma, beta = run_fwd(c, D)
        assert bool(torch.isnan(y[rows:].float()).all()) and bool(torch.isnan(mean[rows:]).all()) and bool(torch.isnan(rstd[rows:]).all()), (what, "guard rows written")
        ref = R.fwd_reference(from_stream(x, rows, D, c["rpg"], c["gs"]), gamma, beta)
        fails, ratios = R.fwd_accept(y[:rows], mean[:rows], rstd[:rows], ref)
        note({"fwd " + k: v for k, v in ratios.items()}, D)
        assert not fails, (what, fails)
        again = run_fwd(c, D)
        assert all(torch.equal(bits(p), bits(q)) for p, q in zip((y, mean, rstd), again[1:4])), (what, "not deterministic")
        m = prefix_rows(rows)
        if m and not c["rpg"]:
            part = run_fwd(c, D, rows=m)
            assert torch.equal(bits(part[1][:m]), bits(y[:m])) and torch.equal(part[2][:m], mean[:m]), (what, "rows depend on the row count")


# ----------------------------------------------------------------------------- backward
@functools.lru_cache(maxsize=16)
def _bwd_operands(family, rows, D):
    return R.make_bwd(family, rows, D)


def bwd_inputs(c, D, rows=None):
    """Device operands of one case (first `rows` rows), as the kernel receives them, and the float32 statistics handed over."""
    full = c["rows"]
    rows = rows or full
    o = _bwd_operands(c["family"], full, D)
    rpg, gs = c["rpg"], c["gs"]
    t = dict(rows=rows)
    t["x"] = to_stream(o["x"][:rows], rows, D, rpg, gs, c["xT"])
    t["dy"] = o["dy"][:rows].to(c["dyT"]).to(dev()).contiguous()
    t["add1"] = to_stream(o["add1"][:rows], rows, D, rpg, gs, c["gT"]) if c["add1"] else None
    t["add2"] = to_stream(o["add2"][:rows], rows, D, rpg, gs, c["gT"]) if c["add2"] else None
    t["gamma"] = o["gamma"].to(dev())
    t["a1"] = torch.tensor([o["a1"]], device=dev()) if c["scalars"] else None
    t["a2"] = torch.tensor([o["a2"]], device=dev()) if c["scalars"] else None
    t["dg_old"], t["db_old"] = o["dg_old"].to(dev()), o["db_old"].to(dev())
    if c["family"] == R.INTEGER:
        t["mean"], t["rstd"] = o["mean"][:rows].to(dev()), o["rstd"][:rows].to(dev())
    else:
        st = R.fwd_reference(from_stream(t["x"], rows, D, rpg, gs), t["gamma"], t["gamma"])
        t["mean"], t["rstd"] = st["mean"].float(), st["rstd"].float()
    return t


def call_bwd(c, D, t, *, defer=False, partial=None):
    """One uvc_layernorm_bwd call on NaN-prefilled outputs with guards.  Returns dict(dx buffer, partial, dgamma, dbeta, dots, nblocks)."""
    from uvc_amd import _lib as L, ops
    rows, rpg, gs, G = t["rows"], c["rpg"], c["gs"], R.GUARD_ROWS
    W = 2 * D + 2
    n = stream_layout(rows, D, rpg, gs)[0]
    dx = torch.full((n + G * D,), float("nan"), device=dev(), dtype=c["gT"])
    nb = ops.layernorm_bwd_blocks(rows)
    part = torch.full(((nb + G) * W,), float("nan"), device=dev()) if partial is None else partial
    dg = torch.cat([t["dg_old"], torch.full((G,), R.SENTINEL, device=dev())])
    db = torch.cat([t["db_old"], torch.full((G,), R.SENTINEL, device=dev())])
    dots = torch.full((2 + G,), R.SENTINEL, device=dev()) if c["dots"] else None
    a = ops._ln_args(t["x"], t["gamma"], None, rows, D, ops.UVC_F32 if c["dyT"] == F32T else ops.UVC_BF16, rpg or 1, gs)
    a.mean, a.rstd, a.dy, a.dx = L.ptr(t["mean"]), L.ptr(t["rstd"]), L.ptr(t["dy"]), L.ptr(dx)
    a.add1, a.a1, a.add2, a.a2 = L.ptr(t["add1"]), L.ptr(t["a1"]), L.ptr(t["add2"]), L.ptr(t["a2"])
    a.partial, a.dgamma, a.dbeta, a.dots = L.ptr(part), L.ptr(dg), L.ptr(db), L.ptr(dots)
    a.beta_acc, a.dy_is_f32, a.g_lowp, a.defer_reduce = c["beta_acc"], int(c["dyT"] == F32T), int(c["gT"] == BF16T), int(defer)
    L.check(L.lib().uvc_layernorm_bwd(C.byref(a), L.cur_stream()), "uvc_layernorm_bwd")
    return dict(dx=dx, partial=part, dgamma=dg, dbeta=db, dots=dots, nblocks=int(L.lib().uvc_layernorm_bwd_nblocks(rows)), nb=nb)


def bwd_reference(c, D, t):
    rows, rpg, gs = t["rows"], c["rpg"], c["gs"]
    view = lambda b: None if b is None else from_stream(b, rows, D, rpg, gs)      # noqa: E731
    return R.bwd_reference(view(t["x"]), t["dy"], t["gamma"], t["mean"], t["rstd"], add1=view(t["add1"]), a1=None if t["a1"] is None else float(t["a1"]),
                           add2=view(t["add2"]), a2=None if t["a2"] is None else float(t["a2"]), beta_acc=c["beta_acc"], dg_old=t["dg_old"],
                           db_old=t["db_old"])


def dots_exact(c, D):
    """Whether an INTEGER case's dots accumulators stay below 2^24 quanta (else dots is held to the bound); every other accumulator must."""
    if c["family"] != R.INTEGER:
        return False
    mags = R.integer_magnitudes(_bwd_operands(R.INTEGER, c["rows"], D), add1=c["add1"], add2=c["add2"], scalars=c["scalars"], beta_acc=c["beta_acc"])
    assert all(v < 2 ** 24 for k, v in mags.items() if k != "dots"), mags
    return mags["dots"] < 2 ** 24


def check_bwd(c, D, t, out, what, ref=None):
    rows, rpg, gs, G, W = t["rows"], c["rpg"], c["gs"], R.GUARD_ROWS, 2 * D + 2
    assert gaps_untouched(out["dx"], rows, D, rpg, gs), (what, "dx: guard rows or the rows between groups written")
    assert bool(torch.isnan(out["partial"][out["nb"] * W:]).all()), (what, "scratch past layernorm_bwd_blocks(rows) written")
    for name in ("dgamma", "dbeta"):
        assert bool((out[name][D:] == R.SENTINEL).all()), (what, name, "guard written")
    dots = None
    if c["dots"]:
        assert bool((out["dots"][2:] == R.SENTINEL).all()), (what, "dots guard written")
        dots = out["dots"][:2]
    ref = ref or bwd_reference(c, D, t)
    if dots is not None and not c["add2"]:
        assert float(dots[1]) == 0.0, (what, "dots[1] without add2")
    exact = c["family"] == R.INTEGER
    fails, ratios = R.bwd_accept(from_stream(out["dx"], rows, D, rpg, gs), out["dgamma"][:D], out["dbeta"][:D], dots, ref, exact=exact,
                                 dots_exact=exact and dots_exact(c, D))
    if not exact:
        note({"bwd " + k: v for k, v in ratios.items()}, D)
    assert not fails, (what, fails)
    return ref


@pytest.mark.parametrize("path,D", PATHS, ids=[f"{p}-{D}" for p, D in PATHS])
def test_layernorm_backward_against_float64(path, D):
    for c in bwd_cases(path, D):
        what = (path, D, {k: str(v) for k, v in c.items()})
        t = bwd_inputs(c, D)
        out = call_bwd(c, D, t)
        check_bwd(c, D, t, out, what)
        again = call_bwd(c, D, t)
        for name in ("dx", "dgamma", "dbeta") + (("dots",) if c["dots"] else ()):
            assert torch.equal(bits(out[name]), bits(again[name])), (what, name, "not deterministic")
        m = prefix_rows(c["rows"])
        if m and not c["rpg"]:
            tp = bwd_inputs(c, D, rows=m)
            tp["mean"], tp["rstd"] = t["mean"][:m].contiguous(), t["rstd"][:m].contiguous()
            part = call_bwd(c, D, tp)
            assert torch.equal(bits(part["dx"][:m * D]), bits(out["dx"][:m * D])), (what, "dx rows depend on the row count")


# ----------------------------------------------------------------------------- deferred finish
DEFER_D = 64
DEFER_NBLOCKS = (1, 15, 16, 17, 63, 64, 1536)
DEFER_ROWS = {1: 32, 15: 15 * 32 - 5, 16: 16 * 32, 17: 16 * 32 + 1, 63: 2016, 64: 2017, 1536: 49152 * 2}      # (49152 rows up: 64 rows per block)


def defer_case(i):
    nbk = DEFER_NBLOCKS[i % len(DEFER_NBLOCKS)]
    if nbk == 1536 and i >= len(DEFER_NBLOCKS):
        nbk = 17                                                  # (one item of 98304 rows is enough)
    return dict(rows=DEFER_ROWS[nbk], xT=F32T, dyT=BF16T, gT=BF16T if i % 2 else F32T, family=R.INTEGER, add1=i % 2, add2=1, dots=int(i % 3 != 1),
                scalars=1, rpg=0, gs=DEFER_D), nbk


@functools.lru_cache(maxsize=16)
def _deferred(i, beta_acc):
    """Item i run immediately (the expected outputs) and deferred (partials left for the batch)."""
    c, nbk = defer_case(i)
    c["beta_acc"] = beta_acc
    t = bwd_inputs(c, DEFER_D)
    now = call_bwd(c, DEFER_D, t)
    ref = check_bwd(c, DEFER_D, t, now, ("deferred item", i, "immediate"))
    later = call_bwd(c, DEFER_D, t, defer=True)
    assert later["nblocks"] == nbk, (c["rows"], later["nblocks"], nbk)
    assert torch.equal(later["dgamma"][:DEFER_D], t["dg_old"]) and torch.equal(later["dbeta"][:DEFER_D], t["db_old"]), "defer_reduce touched dgamma / dbeta"
    if c["dots"]:
        assert bool((later["dots"] == R.SENTINEL).all()), "defer_reduce touched dots"
    assert torch.equal(bits(later["dx"]), bits(now["dx"]))
    return c, t, now, later, ref


@pytest.mark.parametrize("n,beta_acc", [(1, 0.0), (3, 0.5), (64, 0.0), (64, 0.5)])
def test_layernorm_backward_deferred_batched_finish(n, beta_acc):
    """defer_reduce = 1 leaves dgamma / dbeta / dots bit-untouched; uvc_layernorm_bwd_reduce_batch over 1, 3 and 64 items of 1 .. 1536 blocks (some
    without dots) gives the immediate path's and the float64 reference's INTEGER results bit for bit; 65 items, a null member, nblocks = 0 refused."""
    from uvc_amd import _lib as L
    # the first item of the 1-item batch is the 1536-block one; the 3-item batch holds 63, 64 and 1536 blocks
    idx = {1: [6], 3: [4, 5, 6]}.get(n) or [(j % 13) for j in range(64)]
    runs = {i: _deferred(i, beta_acc) for i in sorted(set(idx))}
    items = (L.uvc_ln_reduce_item * 65)()
    outs = []
    for k, i in enumerate(idx):
        c, t, now, later, ref = runs[i]
        G = R.GUARD_ROWS
        dg = torch.cat([t["dg_old"], torch.full((G,), R.SENTINEL, device=dev())])
        db = torch.cat([t["db_old"], torch.full((G,), R.SENTINEL, device=dev())])
        dots = torch.full((2 + G,), R.SENTINEL, device=dev()) if c["dots"] else None
        items[k].partial, items[k].dgamma, items[k].dbeta, items[k].dots = L.ptr(later["partial"]), L.ptr(dg), L.ptr(db), L.ptr(dots)
        items[k].nblocks = later["nblocks"]
        outs.append((i, dg, db, dots))
    before = {i: runs[i][3]["partial"].clone() for i in runs}
    L.check(L.lib().uvc_layernorm_bwd_reduce_batch(items, len(idx), DEFER_D, beta_acc, L.cur_stream()), "uvc_layernorm_bwd_reduce_batch")
    for i, dg, db, dots in outs:
        c, t, now, later, ref = runs[i]
        assert torch.equal(bits(before[i]), bits(later["partial"])), (i, "the batch wrote into a partial region")
        for name, got in (("dgamma", dg), ("dbeta", db)):
            assert bool((got[DEFER_D:] == R.SENTINEL).all()), (i, name, "guard written")
            assert torch.equal(got[:DEFER_D], now[name][:DEFER_D]), (i, name, "differs from the immediate path")
            assert torch.equal(got[:DEFER_D], R.round_to(ref[name], F32T)), (i, name, "differs from float64")
        if c["dots"]:
            assert bool((dots[2:] == R.SENTINEL).all()), (i, "dots guard written")
            if dots_exact(dict(c, beta_acc=beta_acc), DEFER_D):
                assert torch.equal(dots[:2], now["dots"][:2]) and torch.equal(dots[:2], R.round_to(ref["dots"], F32T)), (i, "dots")
            else:
                ok, ratio = R.band(dots[:2], ref["dots"], ref["E_dots"])
                assert bool(ok.all()), (i, "dots", ratio)
    if n == 64:
        lib = L.lib()
        assert lib.uvc_layernorm_bwd_reduce_batch(items, 65, DEFER_D, beta_acc, L.cur_stream()) != 0
        assert lib.uvc_layernorm_bwd_reduce_batch(items, 0, DEFER_D, beta_acc, L.cur_stream()) != 0
        bad = (L.uvc_ln_reduce_item * 2)()
        for fld, val in (("partial", None), ("dgamma", None), ("dbeta", None), ("nblocks", 0)):
            for k in range(2):
                bad[k].partial, bad[k].dgamma, bad[k].dbeta, bad[k].dots, bad[k].nblocks = items[k].partial, items[k].dgamma, items[k].dbeta, items[k].dots, items[k].nblocks
            setattr(bad[1], fld, val)
            assert lib.uvc_layernorm_bwd_reduce_batch(bad, 2, DEFER_D, beta_acc, L.cur_stream()) != 0, fld
        torch.cuda.synchronize()


# ----------------------------------------------------------------------------- other kernels that compute the same statistics
def _ln_of(rows_t, gamma, beta, h, mean, rstd, what):
    ref = R.fwd_reference(rows_t, gamma, beta)
    fails, ratios = R.fwd_accept(h, mean, rstd, ref)
    note({f"{what[0]} " + k: v for k, v in ratios.items()}, rows_t.shape[1])
    assert not fails, (what, fails)


@pytest.mark.parametrize("M", [37, 515])
@pytest.mark.parametrize("rows_t", [F32T, BF16T], ids=["f32", "bf16"])
def test_fused_mlp_statistics_on_edge_rows(M, rows_t):
    """uvc_mlp_fused_fwd, training form, D = 192, F = 128: h / mean / rstd from the EDGE rows x by the forward rule; next_h / next_mean / next_rstd
    against float64 LayerNorm of the kernel's own `out`."""
    from uvc_amd import ops
    D, F_ = 192, 128
    x = R.make_x(R.EDGE, M, D, seed=3).to(rows_t).to(dev())
    (gamma, beta), (g2, b2n) = [tuple(v.to(dev()) for v in R.make_params(D, seed=s)) for s in (3, 4)]
    g = torch.Generator().manual_seed(5)
    W1, b1 = (torch.randn(F_, D, generator=g) * 0.06).bfloat16().to(dev()), (torch.randn(F_, generator=g) * 0.1).to(dev())
    W2, b2 = (torch.randn(D, F_, generator=g) * 0.04).bfloat16().to(dev()), (torch.randn(D, generator=g) * 0.1).to(dev())
    nan = lambda *s, dt=F32T: torch.full(s, float("nan"), device=dev(), dtype=dt)      # noqa: E731
    out, h, mean, rstd = nan(M, D, dt=rows_t), nan(M, D, dt=BF16T), nan(M), nan(M)
    gp, u, nh, nm, nr = nan(M, F_, dt=BF16T), nan(M, F_, dt=BF16T), nan(M, D, dt=BF16T), nan(M), nan(M)
    ops.mlp_fused_fwd(x, gamma, beta, W1, b1, W2, b2, out, h=h, mean=mean, rstd=rstd, gp=gp, u=u, next_gamma=g2, next_beta=b2n, next_h=nh,
                      next_mean=nm, next_rstd=nr)
    _ln_of(x, gamma, beta, h, mean, rstd, ("mlp_fused h", M, str(rows_t)))
    assert bool(torch.isfinite(out.float()).all())
    _ln_of(out, g2, b2n, nh, nm, nr, ("mlp_fused next_h", M, str(rows_t)))


@pytest.mark.parametrize("N,K", [(192, 192), (192, 768), (384, 384)])
@pytest.mark.parametrize("M", [16, 4096 + 21])
def test_gemm_ln_out_statistics_on_edge_rows(N, K, M):
    """uvc_gemm_nt with ln_out: A = 0 and bias = 0, so C equals the EDGE rows R exactly (asserted) and ln_out / ln_mean / ln_rstd are their LayerNorm."""
    from uvc_amd import _lib as L, ops
    cT = F32T if N == 192 else BF16T
    Rr = R.make_x(R.EDGE, M, N, seed=6).to(cT).to(dev())
    A, W = torch.zeros(M, K, device=dev(), dtype=BF16T), torch.zeros(N, K, device=dev(), dtype=BF16T)
    W[:] = (torch.randn(N, K, generator=torch.Generator().manual_seed(7)) * 0.05).bfloat16().to(dev())
    bias = torch.zeros(N, device=dev())
    gamma, beta = (v.to(dev()) for v in R.make_params(N, seed=6))
    Cc = torch.full((M, N), float("nan"), device=dev(), dtype=cT)
    h = torch.full((M, N), float("nan"), device=dev(), dtype=BF16T)
    mean, rstd = torch.full((M,), float("nan"), device=dev()), torch.full((M,), float("nan"), device=dev())
    if N == 384 and M < 4096:            # the 384-wide fused form exists from 4096 rows up: refused, and nothing written
        assert L.lib().uvc_gemm_nt_ln_supported(M, N, K, ops.UVC_BF16, ops.EPI_BIAS_RESID) == 0
        with pytest.raises(RuntimeError):
            ops.gemm_nt(A, W, Cc, dtype=ops.UVC_BF16, epilogue=ops.EPI_BIAS_RESID, bias=bias, R=Rr, ln_gamma=gamma, ln_beta=beta, ln_out=h, ln_mean=mean,
                        ln_rstd=rstd)
        assert bool(torch.isnan(h.float()).all()) and bool(torch.isnan(mean).all()) and bool(torch.isnan(Cc.float()).all())
        return
    assert L.lib().uvc_gemm_nt_ln_supported(M, N, K, ops.UVC_BF16, ops.EPI_BIAS_RESID) == 1
    ops.gemm_nt(A, W, Cc, dtype=ops.UVC_BF16, epilogue=ops.EPI_BIAS_RESID, bias=bias, R=Rr, ln_gamma=gamma, ln_beta=beta, ln_out=h, ln_mean=mean, ln_rstd=rstd)
    assert torch.equal(Cc, Rr), "C = 0 + 0 + R"
    _ln_of(Cc, gamma, beta, h, mean, rstd, ("gemm_ln", N, K, M))


# ----------------------------------------------------------------------------- an engine-accepted width outside the vector table
def test_model_at_embed_dim_320_trains_in_bf16():
    """check_cfg admits every embed_dim % 64 == 0 up to 1024, the bf16 mode hands uvc_layernorm_bwd bf16 rows and a bf16 gradient stream at every
    width, and its vector table ends at 64 / 128 / 192 / 256 / 384 / 512 / 768: at embed_dim = 320 the first backward was refused
    (UVC_ERR_UNSUPPORTED) until the one-wave-per-row kernel took those types.  Forward + backward, batch 3: the fp32 mode against oracle.vit on the
    host (3e-3 per tensor), the bf16 mode against the fp32 run of the same weights (TOL_GRAD_BF16), relative L2 as in test_wide_models_gpu.py."""
    from oracle import vit as OV
    from test_streaming_batch_gpu import TOL_GRAD_BF16, _rel
    from uvc_amd.model_distilled import DistilledVisionTransformer
    kw = dict(img_size=32, patch_size=8, num_classes=16, embed_dim=320, depth=2, num_heads=5)
    x = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(9))

    def loss_of(outs):
        return sum((o.float() ** 2).mean() for o in outs)

    grads, logits, sd = {}, {}, None
    for prec in ("fp32", "bf16"):
        torch.manual_seed(13)
        m = DistilledVisionTransformer(1, enable_block_gating=0, precision=prec, device="cuda", **kw)
        if sd is None:
            with torch.no_grad():
                for n_, p in m.named_parameters():
                    if p.dim() >= 2 and "gating" not in n_:
                        p.mul_(3.0)
                    elif "norm" in n_:
                        p.add_(0.1 * torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())).to(p.device))
            sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        m.load_state_dict(sd, strict=True)
        if hasattr(m, "mark_weights_changed"):
            m.mark_weights_changed()
        m.train()
        out = m(x.cuda(), -1, 0.9)[0]
        loss_of(out).backward()
        torch.cuda.synchronize()
        logits[prec] = [o.detach().float().cpu() for o in out]
        grads[prec] = {n_: p.grad.detach().float().cpu().clone() for n_, p in m.named_parameters() if p.grad is not None}
    P = {k: v.double().requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
    cfg = OV.VitConfig(enable_dist=1, **kw)
    (o, od), _ = OV.forward(P, cfg, OV.GateFlags(enable_block_gating=0, training=True), x.double())
    ((o ** 2).mean() + (od ** 2).mean()).backward()
    checked = 0
    for k, p in P.items():
        if p.grad is None or float(p.grad.norm()) == 0.0:
            continue
        assert k in grads["fp32"] and k in grads["bf16"], k
        assert _rel(grads["fp32"][k], p.grad) <= 3e-3, ("fp32 vs oracle", k, _rel(grads["fp32"][k], p.grad))
        assert _rel(grads["bf16"][k], grads["fp32"][k]) <= TOL_GRAD_BF16, ("bf16 vs fp32", k, _rel(grads["bf16"][k], grads["fp32"][k]))
        checked += 1
    assert checked >= 2 * 12 + 6, checked
    for a, b, ref in zip(logits["fp32"], logits["bf16"], (o, od)):
        assert _rel(a, ref.detach()) <= 1e-3 and _rel(b, a) <= 2e-2


def test_worst_ratios_are_reported():
    """Prints the worst error / bound per output and width over the cases above (run last; -s shows it).  The rules themselves assert <= 1.

    Measured on an MI355X, RANDOM and EDGE rows, worst over all widths [range over the widths] -- beside it the honest CPU simulation of
    tests/test_layernorm_refs_cpu.py (173 rows, worst layout) over the same widths:
        forward   y 0.21 [0.04 .. 0.21]   mean 0.12 [0.01 .. 0.12]   rstd 0.22 [0.03 .. 0.22]          simulation: y 0.23, mean 0.07, rstd 0.26
                  (per width the two agree: y at D = 192 / 384 / 768 is 0.14 / 0.19 / 0.21 on the GPU, 0.14 / 0.23 / 0.20 simulated)
        backward  dx 0.40 [0.25 .. 0.40]  dgamma 0.24 [0.17 .. 0.24]  dbeta 0.10  dots 0.005            simulation: dx 0.42 [0.30 .. 0.42], dgamma 0.006
                  (dgamma / dbeta: the worst ratio is the one-row cases, one term against 2 (1 + 4) u; at 173 rows they are below 0.01 as simulated)
        uvc_mlp_fused_fwd      h: y 0.08, mean 0.09, rstd 0.34     next_h: y 0.05, mean 0.07, rstd 0.22
        uvc_gemm_nt ln_out     N = 192: y 0.03, mean 0.17, rstd 0.46     N = 384: y 0.01, mean 0.02, rstd 0.19
    INTEGER rows: every dx, dgamma, dbeta and dots bit for bit, every width, row count, type combination and finish (one-stage, two-stage, batched)."""
    names = sorted({k for k, _ in WORST})
    for k in names:
        per = {D: v for (n, D), v in WORST.items() if n == k}
        print(f"worst ratio {k}: {max(per.values()):.3f}   " + " ".join(f"{D}:{per[D]:.2f}" for D in sorted(per)))
    assert all(v <= 1.0 for v in WORST.values()), WORST
