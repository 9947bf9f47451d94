"""CPU: tests/t2t_refs.py accepts honest float32 tokens-to-token kernels and rejects subtly wrong ones, its references agree with oracle/t2t.py in
float64 (autograd there, closed forms here), and the case tables of tests/test_t2t_accuracy_gpu.py keep the promises their claims rest on.

The honest kernels are simulated in float32 with the structure of uvc_amd/csrc/t2t.hip: a row sum is 64 per-lane sums of NV elements (lane + 64 j)
followed by a six-level tree; dgamma / dbeta are per-wave sums over (trip, row slot), four waves added in order, the per-workgroup partials split
sixteen ways and added in order; the Performer's token sums are per 64-token tile, seven tiles per split in order, then the splits in order.  Every
run is repeated with a permuted order (the other butterfly, rows and tokens reversed).  Every honest ratio must stay at or below HONEST_RATIO = 0.5
for every case of the GPU tables; the INTEGER / INTSUM claims must come out bit for bit.

Mutants (MUTANTS): each is the honest simulation with one defect and must exceed a bound or break an equality:
    skip_tap            the last tap of a k = 2 window reads 0                         plain split equality, LayerNorm y
    swap_ho_wo          rows decomposed with Ho in place of Wo on a 5 x 7 output map   plain split equality
    clamp_padding       a tap in the padding reads its clamped neighbour               plain split equality
    mean_over_ldo       mean and variance over the ldo = 160 columns of a 147-wide row mean, rstd, y
    eps_omitted         eps = 0: the constant EDGE rows get an infinite rstd           not finite
    no_c2               dxu without the xh c2 term                                     dxu
    drop_last_trip      the second grid-stride trip missing from dgamma / dbeta        INTSUM equality
    fold_no_modulo      fold without the (h + p - ki) % s test                         fold equality
    drop_split_token    token 447 (the last of split 0) missing from kptv / ksum       SPIKE at 447: kptv
    dead_tokens         the 63 dead tokens of T = 65's tail tile counted with exp(0)   ksum
    norm_of_q           |k|^2 / 2 taken of q                                           kptv
    no_1e-8             den without + 1e-8                                             RANGE: att of the last image
    dden_sign           dden = + dot / den^2                                           dq, dksum
    no_dskip            dskip not added to dv                                          dv
    no_dksum            dksum missing from dkp                                         dk
Run with -s to see the worst honest ratio per family and the smallest ratio of every mutant."""
import math

import pytest
import torch
import torch.nn.functional as F

import layernorm_refs as LR
import t2t_refs as R
import test_t2t_accuracy_gpu as G
from oracle import t2t as OT

HONEST_RATIO = 0.5
F32T, BF16T = torch.float32, torch.bfloat16
WORST = {}


def f32(t):
    return t.to(torch.float32)


def keep(ratios, fam, honest=True):
    for k, v in ratios.items():
        if "exact" not in k:
            WORST[(k, fam)] = max(WORST.get((k, fam), 0.0), v)
    if honest:
        bad = {k: v for k, v in ratios.items() if "exact" not in k and v > HONEST_RATIO}
        assert not bad, (fam, bad)


# ----------------------------------------------------------------------------- honest soft split (+ LayerNorm)
def gather(src, g, mutate=None, rows=None):
    """float32 unfolded rows as k_unfold_ln's gather forms them (and its three mutants)."""
    sb, sc, sh, sw = g["strides"]
    r = torch.arange(g["rows"]) if rows is None else rows
    b, l = r // g["L"], r % g["L"]
    wdiv = g["Ho"] if mutate == "swap_ho_wo" else g["Wo"]
    ho, wo = l // wdiv, l % wdiv
    e = torch.arange(g["dim"])
    c, t = e // g["kk"], e % g["kk"]
    ki, kj = t // g["k"], t % g["k"]
    hi, wi = (ho * g["s"] - g["p"])[:, None] + ki[None], (wo * g["s"] - g["p"])[:, None] + kj[None]
    valid = (hi >= 0) & (hi < g["H"]) & (wi >= 0) & (wi < g["W"])
    if mutate == "clamp_padding":
        hi, wi, valid = hi.clamp(0, g["H"] - 1), wi.clamp(0, g["W"] - 1), torch.ones_like(valid)
    if mutate == "skip_tap":
        valid = valid & ~((ki == g["k"] - 1) & (kj == g["k"] - 1))[None]
    off = b[:, None] * sb + c[None] * sc + hi * sh + wi * sw
    return torch.where(valid, src.reshape(-1)[torch.where(valid, off, torch.zeros_like(off))], torch.zeros(()))


def lane_sum(v, nv, order=0):
    rows, D = v.shape
    pad = torch.zeros(rows, nv * 64)
    pad[:, :D] = v
    per = pad.view(rows, nv, 64)
    s = per[:, 0]
    for j in range(1, nv):
        s = s + per[:, j]
    while s.shape[1] > 1:
        s = s[:, 0::2] + s[:, 1::2] if order else s[:, :s.shape[1] // 2] + s[:, s.shape[1] // 2:]
    return s[:, 0]


def sim_ln_fwd(x, gamma, beta, g, c, order=0, mutate=None):
    n = torch.tensor(float(c["ldo"] if mutate == "mean_over_ldo" else g["dim"]))
    eps = torch.tensor(0.0 if mutate == "eps_omitted" else R.LN_EPS)
    mean = lane_sum(x, g["nv"], order) / n
    d = x - mean[:, None]
    rstd = 1.0 / torch.sqrt(lane_sum(d * d, g["nv"], order) / n + eps)
    return (d * rstd[:, None] * gamma + beta).to(c["outT"]), mean, rstd


def block_col_sum(t, g, old, beta_acc, order=0, mutate=None):
    """[rows, n] -> [n] as k_unfold_ln_bwd + k_unfold_bwd_reduce sum dgamma / dbeta."""
    rows, n = t.shape
    trips, grid, per = R.bwd_trips(g)
    if order:
        t = t.flip(0)
    pad = torch.zeros(trips * grid * per, n)
    pad[:rows] = t
    x = pad.view(trips, grid, per // 4, 4, n)
    acc = torch.zeros(grid, 4, n)
    for tr in range(trips):
        if mutate == "drop_last_trip" and tr == trips - 1 and trips > 1:
            continue
        for u in range(per // 4):
            acc = acc + x[tr, :, u]
    part = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    n16 = -(-grid // 16)
    p16 = torch.zeros(n16 * 16, n)
    p16[:grid] = part
    p16 = p16.view(n16, 16, n)
    q = torch.zeros(16, n)
    for i in range(n16):
        q = q + p16[i]
    tot = torch.zeros(n)
    for i in range(16):
        tot = tot + q[i]
    return (torch.tensor(beta_acc) * old if beta_acc else 0.0) + tot


def sim_ln_bwd(x, dy, gamma, mean, rstd, g, c, dg_old, db_old, order=0, mutate=None):
    inv = torch.tensor(1.0) / torch.tensor(float(g["dim"]))
    xh, gy = (x - mean[:, None]) * rstd[:, None], dy * gamma
    s1, s2 = lane_sum(gy, g["nv"], order) * inv, lane_sum(gy * xh, g["nv"], order) * inv
    dxu = rstd[:, None] * (gy - s1[:, None] - (0.0 if mutate == "no_c2" else xh * s2[:, None]))
    return dxu, block_col_sum(dy * xh, g, dg_old, c["beta_acc"], order, mutate), block_col_sum(dy, g, db_old, c["beta_acc"], order, mutate)


def judge_unfold_fwd(name, c, order=0, mutate=None, rows=None):
    """(fails, ratios) of one forward case of the GPU tables on the simulation."""
    g = G.geom(name)
    src, gamma, beta = R.make_unfold_fwd(g, c["family"])
    x, ref_x = gather(src, g, mutate, rows), R.unfold_rows(src, g, rows)
    if not c["ln"]:
        ok = torch.equal(x.to(c["outT"]), ref_x.to(c["outT"]))
        return ([] if ok else ["the plain soft split is not the gather"]), {}
    y, mean, rstd = sim_ln_fwd(x, gamma, beta, g, c, order, mutate)
    return LR.fwd_accept(y, mean, rstd, R.ln_fwd_reference(ref_x, gamma, beta, g["nv"]))


def judge_unfold_bwd(name, c, order=0, mutate=None):
    g = G.geom(name)
    o = R.make_unfold_bwd(g, c["family"])
    x, dy = R.unfold_rows(o["src"], g), f32(o["dy"].to(c["dyT"]))
    if c["family"] in (R.INTEGER, R.INTSUM):
        mean, rstd = o["mean"], o["rstd"]
    else:
        st = R.ln_fwd_reference(x, o["gamma"], o["gamma"], g["nv"])
        mean, rstd = st["mean"].float(), st["rstd"].float()
    dxu, dg, db = sim_ln_bwd(x, dy, o["gamma"], mean, rstd, g, c, o["dg_old"], o["db_old"], order, mutate)
    ref = R.ln_bwd_reference(x, dy, o["gamma"], mean, rstd, g["nv"], c["beta_acc"], o["dg_old"], o["db_old"])
    f1, r1 = LR.bwd_accept(None, dg, db, None, ref, exact=c["family"] in (R.INTEGER, R.INTSUM))
    f2, r2 = LR.bwd_accept(dxu, None, None, None, ref, exact=c["family"] == R.INTEGER)
    return f1 + f2, dict(r1, **r2)


def distinct(cases, keys):
    seen, out = set(), []
    for c in cases:
        k = tuple(str(c[n]) for n in keys)
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out


@pytest.mark.parametrize("name", list(G.GEOMS))
def test_honest_soft_split_stays_below_half_of_every_bound(name):
    for c in distinct(G.fwd_cases(name), ("outT", "ldo", "family", "ln")):
        for order in (0, 1):
            fails, ratios = judge_unfold_fwd(name, c, order)
            assert not fails, (name, c, fails)
            keep({"unfold fwd " + k: v for k, v in ratios.items()}, c["family"])
    for c in distinct(G.bwd_cases(name), ("dyT", "family", "beta_acc")):
        for order in (0, 1):
            fails, ratios = judge_unfold_bwd(name, c, order)
            assert not fails, (name, c, fails)
            assert all(v == 0.0 for k, v in ratios.items() if "exact" in k)
            keep({"unfold bwd " + k: v for k, v in ratios.items()}, c["family"])


@pytest.mark.parametrize("name", ["bwd_trips_nv3", "bwd_trips_nv9", "bwd_reduce_392"])
def test_honest_backward_over_two_trips(name):
    for c in G.trip_bwd_cases(name):
        fails, ratios = judge_unfold_bwd(name, c, order=int(c["family"] == R.RANDOM))
        assert not fails, (name, c, fails)
        keep({"unfold bwd " + k: v for k, v in ratios.items()}, c["family"])


@pytest.mark.parametrize("name", ["fwd_trips_nv3", "fwd_trips_nv9"])
def test_forward_sample_reaches_the_second_trip_and_stays_below_half(name):
    g = G.geom(name)
    trips, grid, per = R.fwd_trips(g)
    sample = G.sample_rows(g["rows"])
    assert trips == 2 and int((sample >= grid * per).sum()) >= 64 and int((sample < grid * per).sum()) >= 64
    assert sample.numel() >= 64 + 64 + G.SAMPLE_SEEDED * 0.9 and bool((sample[:64] == torch.arange(64)).all()) and int(sample[-1]) == g["rows"] - 1
    c = dict(outT=BF16T, ldo=-(-g["dim"] // 32) * 32, family=R.RANDOM, ln=True)
    fails, ratios = judge_unfold_fwd(name, c, rows=sample[::8])
    assert not fails, fails
    keep({"unfold fwd " + k: v for k, v in ratios.items()}, R.RANDOM)


# ----------------------------------------------------------------------------- honest fold
def sim_fold(src, g, mutate=None):
    """float32 sums in the kernels' tap order; mutate fold_no_modulo: the (h + p - ki) % s test missing."""
    B, C, H, W, k, s, p, Ho, Wo, L, kk = (g[n] for n in ("B", "C", "H", "W", "k", "s", "p", "Ho", "Wo", "L", "kk"))
    dst = torch.zeros(B, H, W, C)
    for h in range(H):
        for w in range(W):
            for ki in range(k):
                hh = h + p - ki
                if hh < 0 or (hh % s and mutate != "fold_no_modulo") or hh // s >= Ho:
                    continue
                for kj in range(k):
                    ww = w + p - kj
                    if ww < 0 or (ww % s and mutate != "fold_no_modulo") or ww // s >= Wo:
                        continue
                    rows = torch.arange(B) * L + (hh // s) * Wo + ww // s
                    dst[:, h, w] = dst[:, h, w] + src[rows][:, torch.arange(C) * kk + ki * k + kj]
    return dst.reshape(B, H * W, C)


@pytest.mark.parametrize("name", list(G.FOLD_GEOMS))
def test_honest_fold_is_exact_on_integers_and_adjoint(name):
    g = G.geom(name)
    gen = torch.Generator().manual_seed(g["rows"])
    vals = torch.randint(-8, 9, (g["rows"], g["dim"]), generator=gen).float()
    ref = R.fold(vals, g)
    assert float(ref.abs().max()) <= 256 and torch.equal(sim_fold(vals, g).double(), ref) and torch.equal(R.fold(R.to_tap_major(vals, g), g, True), ref)
    assert torch.equal(sim_fold(vals, g).bfloat16().double(), ref)
    x4 = torch.randn(g["B"], g["C"], g["H"], g["W"], generator=gen)
    want = F.fold(vals.double().reshape(g["B"], g["L"], g["dim"]).transpose(1, 2), (g["H"], g["W"]), g["k"], stride=g["s"], padding=g["p"])
    assert torch.equal(ref, want.permute(0, 2, 3, 1).reshape(ref.shape)), "fold differs from torch's"
    x = x4.permute(0, 2, 3, 1).contiguous()
    gr = torch.randn(g["rows"], g["dim"], generator=gen)
    unf = R.unfold_rows(x, g)
    assert torch.equal(unf, OT.soft_split(x4, g["k"], g["s"], g["p"]).reshape(g["rows"], g["dim"])), "unfold_rows differs from the oracle's soft split"
    lhs = float((unf.double() * gr.double()).sum())
    rhs = float((x.reshape(g["B"], -1, g["C"]).double() * sim_fold(gr, g).double()).sum())
    E = 2.0 * (g["kk"] + 4) * R.U * float((x.reshape(g["B"], -1, g["C"]).double().abs() * R.fold(gr.abs(), g)).sum())
    keep({"fold adjoint": abs(lhs - rhs) / E}, R.RANDOM)


# ----------------------------------------------------------------------------- honest Performer
def token_sum(a, order=0):
    """[B, T, ...] -> [B, ...]: 64-token tiles, seven tiles per split in order, the splits in order."""
    B, T = a.shape[:2]
    nt = -(-T // R.PT)
    S = R.performer_splits(T)
    pad = torch.zeros((B, S * R.PTPS * R.PT) + a.shape[2:])
    pad[:, :T] = a
    tiles = pad.view((B, S, R.PTPS, R.PT) + a.shape[2:])
    tiles = (tiles.flip(3) if order else tiles).sum(3)
    tot = torch.zeros((B,) + a.shape[2:])
    for s in range(S):
        acc = torch.zeros_like(tot)
        for i in range(R.PTPS):
            acc = acc + tiles[:, s, i]
        tot = tot + acc
    return tot


def sim_performer(kqv, w, datt, dskip, gT, order=0, mutate=None):
    B, T, _ = kqv.shape
    k, q, v = torch.split(kqv, R.PE, dim=-1)
    rt = torch.tensor(math.sqrt(R.PM))

    def prm(x, nx):
        return torch.exp(x @ w.T - 0.5 * (nx * nx).sum(-1, keepdim=True)) / rt
    kp, qp = prm(k, q if mutate == "norm_of_q" else k), prm(q, q)
    kps = kp.clone()
    if mutate == "drop_split_token":
        kps[:, min(T, R.PT * R.PTPS) - 1] = 0.0
    kptv, ksum = token_sum(v[..., :, None] * kps[..., None, :], order), token_sum(kps, order)
    if mutate == "dead_tokens":
        ksum = ksum + (-(-T // R.PT) * R.PT - T) / rt
    den = (qp * ksum[:, None]).sum(-1, keepdim=True) + (0.0 if mutate == "no_1e-8" else 1e-8)
    num = qp @ kptv.transpose(1, 2)
    out = dict(kptv=torch.cat([kptv, ksum[:, None]], 1), att=(num / den).to(gT))
    dy = f32(datt)
    dnum = dy / den
    dden = -(dy * num).sum(-1, keepdim=True) / (den * den) * (-1.0 if mutate == "dden_sign" else 1.0)
    dkptv, dksum = token_sum(dnum[..., :, None] * qp[..., None, :], order), token_sum(dden * qp, order)
    gq = (dnum @ kptv + dden * ksum[:, None]) * qp
    dq = gq @ w - q * gq.sum(-1, keepdim=True)
    dv = kp @ dkptv.transpose(1, 2)
    if dskip is not None and mutate != "no_dskip":
        dv = dv + f32(dskip)
    gk = (v @ dkptv + (0.0 if mutate == "no_dksum" else dksum[:, None])) * kp
    dk = gk @ w - k * gk.sum(-1, keepdim=True)
    out.update(dkptv=torch.cat([dkptv, dksum[:, None]], 1), dkqv=torch.cat([dk, dq, dv], -1).to(gT))
    return out


def judge_performer(c, T, order=0, mutate=None):
    o = R.make_performer(c["family"], c["B"], T, spike=c["spike"])
    datt, dskip = o["datt"].to(c["gT"]), (o["dskip"].to(c["gT"]) if c["dskip"] else None)
    got = sim_performer(o["kqv"], o["w"], datt, dskip, c["gT"], order, mutate)
    ref = R.performer_reference(o["kqv"], o["w"], datt, dskip)
    fails, ratios = [], {}
    for n in ("kptv", "dkptv"):
        R.accept(n, got[n][:, :64], ref[n][:, :64], fails, ratios)
        R.accept(n.replace("kptv", "ksum"), got[n][:, 64], ref[n][:, 64], fails, ratios)
    R.accept("att", got["att"], ref["att"], fails, ratios)
    for i, n in enumerate(("dk", "dq", "dv")):
        R.accept(n, got["dkqv"][:, :, 64 * i:64 * i + 64], ref["dkqv"][:, :, 64 * i:64 * i + 64], fails, ratios)
    return fails, ratios, ref


@pytest.mark.parametrize("T", G.PERF_T)
def test_honest_performer_stays_below_half_of_every_bound(T):
    for c in distinct(G.performer_cases(T), ("B", "gT", "family", "spike", "dskip")):
        for order in ((0, 1) if T <= 897 else (0,)):
            fails, ratios, ref = judge_performer(c, T, order)
            assert not fails, (T, c, fails)
            keep({"performer " + k: v for k, v in ratios.items()}, c["family"])
        if c["family"] == R.RANGE:
            for n in ("kptv", "att", "dkptv", "dkqv", "dnum", "dden", "dqp", "dkp", "num", "den"):
                assert float(ref[n].v.abs().max()) < 3e38, (T, n, "not finite in float32")
            assert float((ref["den"].v ** 2).max()) < 3e38, (T, "den^2 (an intermediate of the backward kernel) not finite in float32")
            assert float(ref["z"].min()) <= -70.0 and float(ref["z"].max()) >= 15.0, (float(ref["z"].min()), float(ref["z"].max()))
            assert float((ref["den"].v[-1] - 1e-8).max()) < 1e-6, "the last RANGE image: qp . ksum below 1e-6"


# ----------------------------------------------------------------------------- mutants
def _mut_unfold_fwd(name, mutate, **c):
    return judge_unfold_fwd(name, dict(dict(outT=F32T, ldo=R.ldo_choices(G.geom(name)["dim"])[0], family=R.RANDOM, ln=True), **c), 0, mutate)


def _mut_unfold_bwd(name, mutate, family):
    return judge_unfold_bwd(name, dict(dyT=F32T, family=family, beta_acc=0.5), 0, mutate)


def _mut_fold(mutate):
    g = G.geom("nv9cf_321")
    vals = torch.randint(-8, 9, (g["rows"], g["dim"]), generator=torch.Generator().manual_seed(1)).float()
    d = float((sim_fold(vals, g, mutate).double() - R.fold(vals, g)).abs().max())
    return (["fold differs"] if d else []), {"fold [exact]": d}


def _mut_performer(mutate, T, family, spike=None, B=1):
    return judge_performer(dict(B=B, gT=F32T, family=family, spike=spike, dskip=True), T, 0, mutate)[:2]


MUTANTS = {
    "skip_tap": [lambda m: _mut_unfold_fwd("nv9cf_k2", m, ln=False), lambda m: _mut_unfold_fwd("nv9cf_k2", m)],
    "swap_ho_wo": [lambda m: _mut_unfold_fwd("nv3_image", m, ln=False), lambda m: _mut_unfold_fwd("nv3_image", m)],
    "clamp_padding": [lambda m: _mut_unfold_fwd("nv9cf_321", m, ln=False), lambda m: _mut_unfold_fwd("nv9cf_321", m)],
    "mean_over_ldo": [lambda m: _mut_unfold_fwd("nv3_image", m)],
    "eps_omitted": [lambda m: _mut_unfold_fwd("nv3cf_k1", m, family=R.EDGE)],
    "no_c2": [lambda m: _mut_unfold_bwd("nv3_image", m, R.RANDOM), lambda m: _mut_unfold_bwd("nv9cf_321", m, R.RANDOM)],
    "drop_last_trip": [lambda m: _mut_unfold_bwd("bwd_trips_nv3", m, R.INTSUM)],
    "fold_no_modulo": [_mut_fold],
    "drop_split_token": [lambda m: _mut_performer(m, 449, R.SPIKE, 447)],
    "dead_tokens": [lambda m: _mut_performer(m, 65, R.RANDOM)],
    "norm_of_q": [lambda m: _mut_performer(m, 65, R.RANDOM)],
    "no_1e-8": [lambda m: _mut_performer(m, 65, R.RANGE, B=3)],
    "dden_sign": [lambda m: _mut_performer(m, 65, R.RANDOM)],
    "no_dskip": [lambda m: _mut_performer(m, 65, R.RANDOM)],
    "no_dksum": [lambda m: _mut_performer(m, 65, R.RANDOM)],
}


@pytest.mark.parametrize("mutate", list(MUTANTS))
def test_mutants_are_rejected(mutate):
    smallest = float("inf")
    for run in MUTANTS[mutate]:
        fails, ratios = run(mutate)
        assert fails, (mutate, "accepted", ratios)
        smallest = min(smallest, max(ratios.values()) if ratios else float("inf"))
    print(f"mutant {mutate}: rejected; smallest worst-element ratio (exact families: absolute difference) {smallest:.3g}")


# ----------------------------------------------------------------------------- the references against the oracle
def test_references_agree_with_the_oracle_in_float64():
    """LayerNorm of the soft split, its backward folded onto the source, and the Performer forward / backward: closed forms here, autograd there."""
    for name in ("nv9cf_321", "nv3_image", "nv9cf_p_ge_k"):
        g = G.geom(name)
        gen = torch.Generator().manual_seed(3)
        x4 = torch.randn(g["B"], g["C"], g["H"], g["W"], generator=gen, dtype=torch.float64).requires_grad_()
        gamma, beta = (torch.randn(g["dim"], generator=gen, dtype=torch.float64).requires_grad_() for _ in range(2))
        dy = torch.randn(g["rows"], g["dim"], generator=gen, dtype=torch.float64)
        y = F.layer_norm(OT.soft_split(x4, g["k"], g["s"], g["p"]), (g["dim"],), gamma, beta, R.LN_EPS).reshape(g["rows"], g["dim"])
        (y * dy).sum().backward()
        src = (x4.detach().permute(0, 2, 3, 1) if g["tm"] else x4.detach()).contiguous()
        rows = R.unfold_rows(src, g)
        fw = R.ln_fwd_reference(rows, gamma.detach(), beta.detach(), g["nv"])
        bw = R.ln_bwd_reference(rows, dy, gamma.detach(), fw["mean"], fw["rstd"], g["nv"], 0.0, None, None)
        assert torch.allclose(fw["y"], y.detach(), rtol=1e-11, atol=1e-11) and torch.allclose(bw["dgamma"], gamma.grad, rtol=1e-10, atol=1e-10)
        assert torch.allclose(bw["dbeta"], beta.grad, rtol=1e-10, atol=1e-10)
        dsrc = R.fold(bw["dx"], g).reshape(g["B"], g["H"], g["W"], g["C"]).permute(0, 3, 1, 2)
        assert torch.allclose(dsrc, x4.grad, rtol=1e-9, atol=1e-9), name
    gen = torch.Generator().manual_seed(4)
    kqv = (torch.randn(2, 65, 192, generator=gen, dtype=torch.float64) * 0.5).requires_grad_()
    w = torch.randn(32, 64, generator=gen, dtype=torch.float64) * 0.7
    datt, dskip = torch.randn(2, 65, 64, generator=gen, dtype=torch.float64), torch.randn(2, 65, 64, generator=gen, dtype=torch.float64)
    k, q, v = torch.split(kqv, 64, dim=-1)                      # (oracle.t2t.linear_attention casts to float32 inside: its lines, kept in float64)
    kp, qp = (torch.exp(x @ w.T - (x * x).sum(-1, keepdim=True) / 2) / math.sqrt(32) for x in (k, q))
    y = torch.einsum("bti,bni->btn", qp, torch.einsum("bin,bim->bnm", v, kp)) / (torch.einsum("bti,bi->bt", qp, kp.sum(1)).unsqueeze(2) + OT.PRM_EPS)
    y32, _ = OT.linear_attention(kqv.detach().float(), w.float())
    assert torch.allclose(y32.double(), y.detach(), rtol=1e-4, atol=1e-5)
    ((y * datt).sum() + (v * dskip).sum()).backward()
    ref = R.performer_reference(kqv.detach(), w, datt, dskip)
    assert torch.allclose(ref["att"].v, y.detach(), rtol=1e-11, atol=1e-12) and torch.allclose(ref["dkqv"].v, kqv.grad, rtol=1e-9, atol=1e-11)


# ----------------------------------------------------------------------------- the GPU module's tables
def test_integer_cases_stay_exact_in_float32():
    n = 0
    for name in list(G.GEOMS) + ["bwd_trips_nv3", "bwd_trips_nv9", "bwd_reduce_392"]:
        g = G.geom(name)
        cases = G.bwd_cases(name) if name in G.GEOMS else G.trip_bwd_cases(name)
        for c in distinct([c for c in cases if c["family"] in (R.INTEGER, R.INTSUM)], ("family", "beta_acc")):
            o = R.make_unfold_bwd(g, c["family"])
            mags = R.integer_magnitudes(g, o, c["beta_acc"]) if c["family"] == R.INTEGER else R.intsum_magnitudes(g, o, c["beta_acc"])
            assert all(v < 2 ** 24 for v in mags.values()), (name, c, mags)
            n += 1
    print(f"INTEGER / INTSUM cases: {n} distinct, every accumulator below 2^24 quanta")
    assert n >= 2 * len(G.GEOMS)


def test_case_tables_reach_what_they_name():
    from uvc_amd import _lib as L
    lib = L.lib()
    for (nv, cf), names in G.CLASSES.items():
        for name in names:
            g = G.geom(name)
            assert (3 if -(-g["dim"] // 64) <= 3 else 9) == nv == g["nv"] and (g["strides"][1] == 1 and g["C"] == 64) == cf == g["c_fast"], name
            assert g["dim"] <= 576
    assert sorted(n for v in G.CLASSES.values() for n in v) == sorted(G.GEOMS)
    gs = {n: G.geom(n) for n in G.GEOMS}
    assert any(not g["tm"] and g["nv"] == 9 for g in gs.values()), "(9, generic) from an NCHW source"
    assert any(g["c_fast"] and g["k"] == 1 and g["nv"] == 3 for g in gs.values()), "(3, CF): C = 64, k = 1"
    assert any(g["tm"] and g["C"] != 64 for g in gs.values()), "token-major, C != 64"
    assert any(g["dim"] == 192 for g in gs.values()) and any(g["dim"] == 196 for g in gs.values())
    assert all(g["H"] != g["W"] or n in ("nv3_one_row", "nv9cf_7x7", "nv9cf_s_gt_k") for n, g in gs.items())
    assert any(g["Ho"] != g["Wo"] for g in gs.values()) and any(g["s"] > g["k"] for g in gs.values())
    padded = [n for n, g in gs.items() if g["p"] >= g["k"]]
    assert padded and all(bool((~R.unfold_index(gs[n])[1].any(1)).any()) for n in padded), "p >= k: a row wholly in the padding"
    uncovered = gs["nv9cf_s_gt_k"]
    assert bool((R.fold(torch.ones(uncovered["rows"], uncovered["dim"]), uncovered) == 0).any())
    for name, g in gs.items():
        f, b = G.fwd_cases(name), G.bwd_cases(name)
        ldos = set(R.ldo_choices(g["dim"]))
        assert ldos == {x for x in ({g["dim"]} if g["dim"] % 8 == 0 else set()) | {-(-g["dim"] // 32) * 32, -(-g["dim"] // 64) * 64}}
        assert all(g["dim"] <= x <= -(-g["dim"] // 64) * 64 and x % 8 == 0 for x in ldos)
        assert {c["ldo"] for c in f} == ldos == {c["ldo"] for c in b}, name
        assert {(c["dtype"], c["outT"]) for c in f} == set(G.TYPES) == {(c["dtype"], c["dyT"]) for c in b}
        assert {c["ln"] for c in f} == {True, False} and {c["beta_acc"] for c in b} == set(G.BETAS)
        assert {c["dxu"] for c in b} == set(G.DXU if g["c_fast"] else G.DXU[:2])
        fams = {c["family"] for c in b}
        assert fams == ({R.RANDOM, R.INTSUM, R.EDGE, R.INTEGER} if g["s"] >= g["k"] else {R.RANDOM, R.INTSUM}), name
        assert lib.uvc_unfold_bwd_blocks(g["rows"]) == R.bwd_blocks(g["rows"])
    assert [R.bwd_trips(G.geom(n))[0] for n in ("bwd_trips_nv3", "bwd_trips_nv9", "bwd_reduce_392")] == [2, 2, 1]
    assert [G.geom(n)["rows"] for n in G.TRIP_GEOMS] == [18816, 8624, 1568, 263424, 131712]
    assert [lib.uvc_unfold_bwd_blocks(G.geom(n)["rows"]) for n in ("bwd_trips_nv3", "bwd_trips_nv9", "bwd_reduce_392")] == [1024, 1024, 392] and 392 % 16
    assert [R.fwd_trips(G.geom(n))[0] for n in ("fwd_trips_nv3", "fwd_trips_nv9")] == [2, 2]
    # fold: every type pair, the compile-time (3, 2, 1) form and another on the tap-major path, C = 32, 70 pixels
    assert {(s, d) for _, s, d in G.FOLD_TYPES} == {(a, b) for a in (F32T, BF16T) for b in (F32T, BF16T)}
    fg = {n: G.geom(n) for n in G.FOLD_GEOMS}
    assert {n for n, v in G.GEOMS.items() if v[1] == 64} <= set(fg) and any(g["C"] == 32 for g in fg.values())
    assert any((g["k"], g["s"], g["p"]) == (3, 2, 1) and g["C"] == 64 for g in fg.values()) and any((g["k"], g["s"], g["p"]) != (3, 2, 1) and g["C"] == 64 for g in fg.values())
    assert any(g["B"] * g["H"] * g["W"] == 70 for g in fg.values())
    # Performer: tiles, splits, spikes
    assert set(G.PERF_T) >= {1, 15, 16, 17, 63, 64, 65, 448, 449, 897} and set(G.PERF_B) == {1, 3}
    for T in G.PERF_T:
        for B in G.PERF_B:
            assert lib.uvc_performer_splits(B, T) == R.performer_splits(T), T
        cs = G.performer_cases(T)
        assert {(c["dtype"], c["gT"]) for c in cs if c["family"] == R.RANDOM} == set(G.TYPES) and {c["dskip"] for c in cs} == {True, False}
        assert {c["B"] for c in cs if c["family"] == R.RANDOM} == {1, 3}
        assert sorted(c["spike"] for c in cs if c["family"] == R.SPIKE) == sorted({p for p in (0, 15, 16, 63, 64, 447, 448) if p < T} | {T - 1})
        assert (T in (65, 449)) == any(c["family"] == R.RANGE for c in cs)
    assert [R.performer_splits(T) for T in (448, 449, 897, 3136)] == [1, 2, 3, 7] and 449 - R.PT * R.PTPS == 1
    assert G.geom("nv9cf_321") and R.geometry(*G.STAGE)["rows"] == 50


def test_worst_honest_ratios_are_reported():
    """Prints the worst honest ratio per output and family (run last; -s shows it)."""
    for k in sorted({k for k, _ in WORST}):
        per = {f: v for (n, f), v in WORST.items() if n == k}
        print(f"honest worst ratio {k}: {max(per.values()):.3f}   " + " ".join(f"{f}:{per[f]:.2f}" for f in sorted(per)))
    assert all(v <= HONEST_RATIO for v in WORST.values()), WORST
