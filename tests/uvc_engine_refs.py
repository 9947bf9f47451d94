"""Model-free harness of the UVC primal-dual engine (uvc_amd/csrc/uvc_engine.hip): plain tensors in, the six C entries
(uvc_scores, uvc_rank, uvc_prox, uvc_write_masks, uvc_resource, uvc_dual_step) called directly through uvc_amd._lib, oracle/uvc.py as the
reference -- used as it stands -- at any (L, H, hd, F) that check_dims admits.  No StubModel and no MAC table from a ViT config:
``mac_table`` is a seeded positive table handed to both sides.

Everything up to ``Engine`` runs without a GPU; tests/test_uvc_engine_refs_cpu.py walks RUNS / SCHEDULE_RUNS on the oracle alone and checks the
conditions under which tests/test_uvc_engine_accuracy_gpu.py may ask for equal bits (see ``oracle_run``).

Weight families (``make_weights``)
  gaussian   0.05 * N(0, 1), as tests/test_uvc_engine_gpu.py: scores tie by float32 coincidence only (a handful of 8192).
  exact      entries are m / 16 with |m| <= 4: every column and head sum of squares is an integer number of 2^-8 below 2^24, so float32 and float64
             agree in any summation order and ties are genuine.  Columns duplicated within a head (1 <- 0, 5 <- 3) and across heads (head 1 is a copy
             of head 0 when H >= 3), zero columns (9, 10 of every head; 20, 33, 47 of fc2), the last head zero (H >= 2), fc2 columns F/4 .. F/4 + F/8
             zero as in the masked state of stage 2, fc2 columns 2i + 1 <- 2i (i < 8) and F - 1 <- 0.
  constant   every column the same exact column: all scores tie, rank == index.
  staircase  exact scores k * 2^-8 with k strictly descending (fc2 of even layers, proj of odd ones) or ascending (the others).
Between optimizer steps the weights move by a seeded 1e-3 * N(0, 1) like the AdamW step the old test emulates -- drawn per SOURCE column, so
duplicated columns stay duplicates, and never on a zero column (a masked weight has no update): the ties survive every step.

State families (``make_state``)
  zero        s = r = 0, y = p = z = 1e-3: the reference's initial state.
  interior    every s, r at an integer + [0.25, 0.75], small and large k; y, p in [0.05, 0.5]; z = 0.5.
  bounds      s[:, 0], s[:, 1] and r alternate between 0 and their maximum from layer to layer (r from head to head too): k = 0 and k = n - 1 in
              every group; ``flip`` swaps the roles (both run where L = 1).
  integers    s, r exact integers in one layer (head) and nextafter(integer, +inf) in the next: ceil differs by one between the two.
  dual_floor  y = p = 0 (the proximal divisor is exactly 1), z = 0.3 under a budget of 2.0, so that z lands on its clamp at 0 in the first step.
              The issue's clause "learning rates negative enough to be clamped" is dropped: ksum >= 0, so with the positive rates every driver
              uses y and p cannot go below 0; only z can, and it does here.
"""
from __future__ import annotations

import ctypes as C
import itertools
from dataclasses import dataclass, replace
from typing import List, Optional

import numpy as np
import torch

from oracle import uvc as OU

STATE_RTOL, STATE_ATOL = 1e-4, 1e-7             # the bounds tests/test_uvc_engine_gpu.py holds the engine to
RES_RTOL, RES_ATOL = 1e-5, 1e-6
MARGIN = 1e-3                                   # clip indicator, distance from an integer, hard Gumbel gap
ROUND_MARGIN = 1e-12                            # float64 score sums vs a float32 rounding boundary, relative
PROX_LR = 3e-3

# (name, L, H, hd, F): what each reaches is in tests/test_uvc_engine_accuracy_gpu.py's docstring
CASES = [("min", 1, 1, 64, 64), ("hd32", 2, 2, 32, 64), ("hd48", 3, 4, 48, 320), ("narrow", 2, 3, 64, 192), ("dwide", 2, 8, 64, 64),
         ("h32", 1, 32, 16, 512), ("hd192", 2, 1, 192, 256), ("fmax", 1, 2, 128, 8192), ("l16", 16, 2, 32, 64), ("l17", 17, 2, 32, 64),
         ("l32", 32, 2, 32, 64), ("tiny", 12, 3, 64, 768)]
CASE = {c[0]: c for c in CASES}
WEIGHT_FAMILIES = ("gaussian", "exact", "constant", "staircase")
STATE_FAMILIES = ("zero", "interior", "bounds", "integers", "dual_floor")
MODES = ("gumbel", "eps", "off", "nogate")      # Gumbel gates / eps gates / enable_block_gating = 0 / gate == nullptr with gating enabled


# ----------------------------------------------------------------------------- rank rule
def lexsort_rank(v: np.ndarray) -> np.ndarray:
    """rank[i] = #{j : v[j] < v[i] or (v[j] == v[i] and j < i)} of a 1-D array."""
    v = np.asarray(v)
    order = np.lexsort((np.arange(v.size), v))
    rk = np.empty(v.size, dtype=np.int64)
    rk[order] = np.arange(v.size)
    return rk


def group_ranks(sc1: np.ndarray, sc2: np.ndarray, sc3: np.ndarray, H: int, hd: int):
    """The three rank arrays of one layer's scores: columns inside their head, heads, fc2 columns."""
    r1 = np.concatenate([lexsort_rank(sc1[h * hd:(h + 1) * hd]) for h in range(H)])
    return r1, lexsort_rank(sc2), lexsort_rank(sc3)


def tie_count(v: np.ndarray) -> int:
    """Number of elements of v that share their value with another element."""
    _, inv, cnt = np.unique(np.asarray(v), return_inverse=True, return_counts=True)
    return int((cnt[inv] > 1).sum())


# ----------------------------------------------------------------------------- weights
class Weights:
    """W1[l] [D, D] and W3[l] [D, F] float32 CPU tensors + the column source maps that keep ties alive under ``perturb``."""

    def __init__(self, W1, W3, src1, src3, live1, live3):
        self.W1, self.W3, self.src1, self.src3, self.live1, self.live3 = W1, W3, src1, src3, live1, live3

    def perturb(self, rng: np.random.Generator, scale: float = 1e-3):
        for W, src, live in itertools.chain(zip(self.W1, self.src1, self.live1), zip(self.W3, self.src3, self.live3)):
            d = rng.standard_normal(tuple(W.shape), dtype=np.float32) * np.float32(scale)
            if not (live.all() and np.array_equal(src, np.arange(src.size))):
                d = d[:, src] * live[None, :].astype(np.float32)
            W += torch.from_numpy(d)


def _stair_column(T: int, D: int) -> np.ndarray:
    """D integers m in [0, 15] with sum of m^2 == T (greedy; needs T <= 225 * (D - 8))."""
    col = np.zeros(D, dtype=np.float32)
    rem = T
    for i in range(D):
        if rem == 0:
            break
        m = min(15, int(np.floor(np.sqrt(rem))))
        col[i] = m
        rem -= m * m
    assert rem == 0, (T, D)
    return col


def make_weights(family: str, L: int, H: int, hd: int, F: int, seed: int) -> Weights:
    D = H * hd
    rs = np.random.RandomState(seed)
    W1, W3, src1, src3, live1, live3 = [], [], [], [], [], []
    for l in range(L):
        s1, s3 = np.arange(D), np.arange(F)
        v1, v3 = np.ones(D, dtype=bool), np.ones(F, dtype=bool)
        if family == "gaussian":
            b1 = (rs.standard_normal((D, D)) * 0.05).astype(np.float32)
            b3 = (rs.standard_normal((D, F)) * 0.05).astype(np.float32)
        elif family == "exact":
            b1 = (rs.randint(-4, 5, size=(D, D)) / 16.0).astype(np.float32)
            b3 = (rs.randint(-4, 5, size=(D, F)) / 16.0).astype(np.float32)
            b1[0, :] = 0.25
            b3[0, :] = 0.25                                        # no column is zero by chance
            for h in range(H):
                s1[h * hd + 1] = s1[h * hd + 0]
                s1[h * hd + 5] = s1[h * hd + 3]
                v1[h * hd + 9] = v1[h * hd + 10] = False
            if H >= 3:
                s1[hd:2 * hd] = s1[0:hd]
            if H >= 2:
                v1[(H - 1) * hd:] = False
            for i in range(8):
                s3[2 * i + 1] = s3[2 * i]
            s3[F - 1] = s3[0]
            v3[[20, 33, 47]] = False
            v3[F // 4:F // 4 + F // 8] = False
        elif family == "constant":
            c1 = (rs.randint(1, 5, size=D) / 16.0).astype(np.float32)
            c3 = (rs.randint(1, 5, size=D) / 16.0).astype(np.float32)
            b1, b3 = np.repeat(c1[:, None], D, 1), np.repeat(c3[:, None], F, 1)
            s1[:], s3[:] = 0, 0
        elif family == "staircase":
            t1 = np.arange(1, D + 1) if l % 2 == 0 else np.arange(D, 0, -1)          # proj: ascending on even layers
            t3 = np.arange(F, 0, -1) if l % 2 == 0 else np.arange(1, F + 1)          # fc2: descending on even layers
            b1 = np.stack([_stair_column(int(t), D) for t in t1], 1) / np.float32(16.0)
            b3 = np.stack([_stair_column(int(t), D) for t in t3], 1) / np.float32(16.0)
        else:
            raise ValueError(family)
        b1, b3 = b1[:, s1] * v1[None, :], b3[:, s3] * v3[None, :]
        W1.append(torch.from_numpy(np.ascontiguousarray(b1, dtype=np.float32)))
        W3.append(torch.from_numpy(np.ascontiguousarray(b3, dtype=np.float32)))
        src1.append(s1); src3.append(s3); live1.append(v1); live3.append(v3)
    return Weights(W1, W3, src1, src3, live1, live3)


# ----------------------------------------------------------------------------- state
def box_max(L: int, H: int, hd: int, F: int):
    """(smax[L, 2], rmax[L, H]) exactly as uvc_update computes them (uvc_optimizer.py:38-39)."""
    s_ub = torch.zeros(L, 2)
    s_ub[:, 0], s_ub[:, 1] = H, F
    return (s_ub - 1 - 1e-8).clamp(min=0.0), (torch.full((L, H), float(hd)) - 1 - 1e-8).clamp(min=0.0)


def make_state(family: str, L: int, H: int, hd: int, F: int, seed: int, flip: int = 0):
    """dict of float32 arrays s[L,2] r[L,H] y[L,2] p[L,H] and the float z."""
    rs = np.random.RandomState(seed + 7919)
    smax, rmax = (t.numpy() for t in box_max(L, H, hd, F))
    s, r = np.zeros((L, 2), np.float32), np.zeros((L, H), np.float32)
    y = rs.uniform(0.05, 0.5, (L, 2)).astype(np.float32)
    p = rs.uniform(0.05, 0.5, (L, H)).astype(np.float32)
    z = 0.5
    frac = lambda shape: rs.uniform(0.25, 0.75, shape)
    up = lambda a: np.nextafter(np.float32(a), np.float32(np.inf))

    def interior():
        if H >= 2:
            s[:, 0] = rs.randint(0, H - 1, L) + frac(L)
        lo_hi = np.where(np.arange(L) % 2 == 0, rs.randint(0, 8, L), F - 2 - rs.randint(0, 8, L))      # small and large k
        s[:, 1] = lo_hi + frac(L)
        r[:] = rs.randint(0, hd - 1, (L, H)) + frac((L, H))

    if family == "zero":
        y[:], p[:], z = 1e-3, 1e-3, 1e-3
    elif family == "interior":
        interior()
    elif family == "dual_floor":
        interior()
        y[:], p[:], z = 0.0, 0.0, 0.3
    elif family == "overbox":                                      # not in STATE_FAMILIES: see OVERBOX_RUNS
        interior()
        s[0, 0], s[0, 1], r[0, 0] = H - 0.5, F - 0.5, hd - 0.5
    elif family == "bounds":
        for l in range(L):
            par = (l + flip) % 2
            s[l, 0] = 0.0 if par == 0 else smax[l, 0]
            s[l, 1] = smax[l, 1] if par == 0 else 0.0
            for h in range(H):
                r[l, h] = 0.0 if (l + h + flip) % 2 == 0 else rmax[l, h]
    elif family == "integers":
        y[:, 0] = rs.uniform(1.0, 3.0, L) / hd                     # comparable gradients in both columns of s: every entry leaves its integer
        y[:, 1] = rs.uniform(1.0, 3.0, L)
        p[:] = rs.uniform(1.0, 3.0, (L, H))
        for l in range(L):
            if H >= 3:
                i = rs.randint(1, H - 1)
                s[l, 0] = i if (l + flip) % 2 == 0 else up(i)
            i = rs.randint(1, F - 1)
            s[l, 1] = i if (l + 1 + flip) % 2 == 0 else up(i)
            for h in range(H):
                i = rs.randint(1, hd - 1)
                r[l, h] = i if (l + h + flip) % 2 == 0 else up(i)
    else:
        raise ValueError(family)
    return dict(s=s, r=r, y=y, p=p, z=float(np.float32(z)))


def mac_table(L: int, seed: int):
    """(embed_macs, total_macs[L][6]): seeded, positive, float32-exact."""
    rs = np.random.RandomState(seed + 104729)
    tm = rs.uniform(1e6, 5e7, (L, 6)).astype(np.float32)
    return float(np.float32(rs.uniform(1e6, 1e7))), tm.astype(np.float64).tolist()


def make_oracle_state(L, H, hd, F, seed, state) -> OU.UvcState:
    embed, macs = mac_table(L, seed)
    st = OU.UvcState.create(L, H, hd, F, embed, macs)
    st.s, st.r = torch.from_numpy(state["s"].copy()), torch.from_numpy(state["r"].copy())
    st.y, st.p, st.z = torch.from_numpy(state["y"].copy()), torch.from_numpy(state["p"].copy()), torch.tensor(float(state["z"]))
    return st


def make_gates(L: int, seed: int) -> torch.Tensor:
    rs = np.random.RandomState(seed + 31337)
    return torch.from_numpy((np.array([-1.0, 1.0]) + rs.standard_normal((L, 2)) * 0.3).astype(np.float32))


# ----------------------------------------------------------------------------- runs
@dataclass(frozen=True)
class Run:
    case: str
    wfam: str
    sfam: str
    clip: str = "in"            # "in": |R - budget| inside z_grad_clip at every step; "out": outside
    mode: str = "gumbel"
    interval: int = 2
    steps: int = 4
    step0: int = 1
    flip: int = 0
    seed: int = 0

    @property
    def id(self):
        return f"{self.case}-{self.wfam}-{self.sfam}{self.flip}-{self.clip}-{self.mode}-i{self.interval}" + ("" if self.step0 == 1 else f"-from{self.step0}")

    @property
    def dims(self):
        return CASE[self.case][1:]


def run_hyper(run: Run) -> OU.UvcHyper:
    """The rates are the drivers' but for ylr / plr (1e-2, not 1e-4: a wrong least-k sum must move y and p by more than the bound)."""
    hp = OU.UvcHyper(budget=0.5, slr=0.02, rlr=0.02, glr=0.1, ylr=1e-2, plr=1e-2, zlr=1.0, sl2wd=0.01,
                     z_grad_clip=5.0 if run.clip == "in" else 0.01, gating_interval=run.interval, gating_weight=5e-4,
                     use_gumbel=int(run.mode != "eps"), enable_block_gating=int(run.mode != "off"))
    if run.sfam == "integers":
        hp.slr = hp.rlr = 0.1
    if run.sfam == "dual_floor":
        hp.budget, hp.z_grad_clip = 2.0, 0.1
    return hp


# weight family x the state families that make sense for it x which side of the clip.  zero and bounds run outside the clip only: inside it
# an entry at 0 with a negative gradient leaves 0 by lr * z * dR/ds << 1e-3, which the distance-from-an-integer condition excludes;
# integers runs on gaussian weights only (a zero or 2^-8 backward factor would leave an entry on its integer).
PLAN = [("gaussian", "zero", "out"), ("gaussian", "interior", "in"), ("gaussian", "interior", "out"), ("gaussian", "bounds", "out"),
        ("gaussian", "integers", "in"), ("gaussian", "dual_floor", "out"), ("exact", "interior", "in"), ("exact", "bounds", "out"),
        ("exact", "dual_floor", "out"), ("constant", "interior", "in"), ("staircase", "interior", "in"), ("staircase", "bounds", "out")]

# seeds under which the oracle satisfies every condition of ``oracle_run`` (found by walking seeds upwards; 0 where not listed)
SEEDS: dict = {
    'l17-gaussian-overbox0-in-off-i2': 1,
    'dwide-staircase-interior0-in-off-i2': 1, 'fmax-exact-bounds0-out-gumbel-i2': 6, 'fmax-gaussian-bounds0-out-off-i2': 23,
    'fmax-staircase-bounds0-out-eps-i3': 4, 'fmax-staircase-bounds1-out-off-i2': 2, 'fmax-staircase-interior0-in-gumbel-i2': 2,
    'h32-exact-bounds1-out-nogate-i3': 1, 'h32-staircase-bounds0-out-nogate-i3': 1, 'hd192-exact-bounds0-out-eps-i3': 1,
    'hd32-exact-bounds0-out-gumbel-i2': 1, 'hd32-gaussian-bounds0-out-gumbel-i2': 1, 'hd32-staircase-bounds0-out-gumbel-i2': 1,
    'hd48-gaussian-integers0-in-off-i2': 1, 'hd48-gaussian-interior0-in-gumbel-i1-from0': 1, 'hd48-gaussian-interior0-in-gumbel-i2-from0': 1,
    'hd48-gaussian-interior0-in-gumbel-i3-from0': 1, 'hd48-gaussian-interior0-in-nogate-i3': 1, 'l16-gaussian-bounds0-out-nogate-i3': 1,
    'l16-gaussian-dual_floor0-out-eps-i3': 1, 'l16-gaussian-integers0-in-gumbel-i2': 1, 'l16-gaussian-zero0-out-gumbel-i2': 1,
    'l16-staircase-interior0-in-off-i2': 1, 'l17-exact-bounds0-out-gumbel-i2': 1, 'l17-gaussian-bounds0-out-gumbel-i2': 2,
    'l17-gaussian-dual_floor0-out-off-i2': 1, 'l17-gaussian-integers0-in-eps-i3': 2, 'l17-gaussian-interior0-in-gumbel-i1-from0': 1,
    'l17-gaussian-interior0-in-gumbel-i2-from0': 1, 'l17-gaussian-interior0-in-gumbel-i3-from0': 1, 'l17-gaussian-interior0-in-off-i2': 1,
    'l17-gaussian-interior0-out-nogate-i3': 1, 'l17-gaussian-zero0-out-eps-i3': 2, 'l17-staircase-bounds0-out-gumbel-i2': 1,
    'l17-staircase-interior0-in-nogate-i3': 1, 'l32-gaussian-bounds0-out-eps-i3': 2, 'l32-gaussian-dual_floor0-out-nogate-i3': 2,
    'l32-gaussian-integers0-in-off-i2': 2, 'l32-gaussian-interior0-in-nogate-i3': 2, 'l32-gaussian-interior0-out-gumbel-i2': 2,
    'l32-gaussian-zero0-out-off-i2': 2, 'l32-staircase-interior0-in-gumbel-i2': 1, 'tiny-constant-interior0-in-gumbel-i2': 1,
    'tiny-exact-interior0-in-eps-i3': 8, 'tiny-gaussian-dual_floor0-out-gumbel-i2': 1, 'tiny-gaussian-interior0-in-gumbel-i1-from0': 34,
    'tiny-gaussian-interior0-in-gumbel-i2': 34, 'tiny-gaussian-interior0-in-gumbel-i2-from0': 34, 'tiny-gaussian-interior0-in-gumbel-i3-from0': 34,
    'tiny-gaussian-interior0-out-eps-i3': 17, 'tiny-gaussian-zero0-out-nogate-i3': 1,
}


def _runs():
    out = []
    for ci, (name, L, H, hd, F) in enumerate(CASES):
        k = 0
        for wf, sf, clip in PLAN:
            for flip in ((0, 1) if (L == 1 and sf in ("bounds", "integers")) else (0,)):
                steps = 4 if L * (H * hd + F) > 4096 else 4 + (ci + k) % 4
                r = Run(name, wf, sf, clip, MODES[(ci + k) % 4], 2 + (ci + k) % 2, steps, 1, flip)
                out.append(replace(r, seed=SEEDS.get(r.id, 0)))
                k += 1
    return out


def _schedule_runs():
    """gating_interval 1, 2, 3 over 7 steps from global_step = 0: accumulate-only steps, the first application (no momentum) and the second."""
    out = []
    for name in ("min", "hd48", "l17", "tiny"):
        for interval in (1, 2, 3):
            r = Run(name, "gaussian", "interior", "in", "gumbel", interval, 7, 0, 0)
            out.append(replace(r, seed=SEEDS.get(r.id, 0)))
    return out


RUNS: List[Run] = _runs()
# One state past the box: s[0, 0], s[0, 1], r[0, 0] = n - 0.5, so k = ceil() = n.  Only a hand-edited checkpoint gets there, but it is the one place
# where group_stat's `want` (n - 1: the reference's LeastSsum returns the maximum when k + 1 > n, uvc_utils.py:75-92) is not k; inside the box
# k <= n - 1 always.  The oracle defines it like the reference, and the step puts the three entries back on smax / rmax.
OVERBOX_RUNS: List[Run] = [replace(r, seed=SEEDS.get(r.id, 0)) for r in (Run("min", "gaussian", "overbox", "in", "gumbel", 2, 4),
                                                                        Run("hd32", "gaussian", "overbox", "in", "eps", 2, 4),
                                                                        Run("l17", "gaussian", "overbox", "in", "off", 2, 4))]
# (kind, case) -> weight seed of the masks / resource tests where the default fails the rounding condition
AUX_SEEDS: dict = {("resource", "fmax"): 20, ("resource", "tiny"): 20}


def aux_seed(kind: str, case: str) -> int:
    return AUX_SEEDS.get((kind, case), dict(masks=3, resource=5)[kind])


def warmup_run(case: str) -> Run:
    """The run whose first step the warm-up test takes, with Gumbel gates."""
    return replace(next(r for r in RUNS if r.case == case and (r.wfam, r.sfam, r.clip) == ("gaussian", "interior", "in")), mode="gumbel")


WARMUP_CASES = ("min", "hd48", "l17")
SCHEDULE_RUNS: List[Run] = _schedule_runs()


# ----------------------------------------------------------------------------- the oracle, step by step
def rounding_margin(x64: np.ndarray) -> float:
    """Smallest relative distance of the non-zero float64 sums to a float32 rounding boundary (the midpoint of two neighbouring float32)."""
    x = np.asarray(x64, dtype=np.float64).ravel()
    x = x[x != 0]
    if x.size == 0:
        return np.inf
    f = x.astype(np.float32)
    hi = (f.astype(np.float64) + np.nextafter(f, np.float32(np.inf)).astype(np.float64)) / 2
    lo = (f.astype(np.float64) + np.nextafter(f, np.float32(-np.inf)).astype(np.float64)) / 2
    return float((np.minimum(np.abs(x - hi), np.abs(x - lo)) / x).min())


def scores64(W1, W3, H, hd):
    """float64 column sums of squares, head sums and fc2 column sums, as oracle.scores_w1 / scores_w3 form them before they round."""
    c1 = [(W.double() ** 2).sum(0) for W in W1]
    return c1, [c.view(H, hd).sum(1) for c in c1], [(W.double() ** 2).sum(0) for W in W3]


def oracle_scores(W1, W3, H, hd):
    """([L, D], [L, H], [L, F]) float32 from oracle.scores_w1 / scores_w3."""
    a = [OU.scores_w1(W, H, hd) for W in W1]
    return (torch.stack([x.reshape(-1) for x, _ in a]), torch.stack([b for _, b in a]), torch.stack([OU.scores_w3(W) for W in W3]))


def int_distance(new: torch.Tensor, vmax: torch.Tensor) -> float:
    """Smallest distance to an integer among the entries that are not exactly on a bound (inf if all are)."""
    v = new.double()
    free = ~((new == 0) | (new == vmax))
    if not bool(free.any()):
        return float("inf")
    return float((v - v.round()).abs()[free].min())


def primal_norms(pre: OU.UvcState, hp: OU.UvcHyper, post_sc, gate, e1):
    """(R, |grad_s|_inf, |grad_r|_inf) of uvc_update's primal step at the state ``pre`` -- out[0], out[2], out[3] of uvc_dual_step -- from the
    oracle's own resource() and least_sum_and_next(), composed as uvc_update composes them (oracle/uvc.py).
    The oracle does not return these, so this is a second copy of uvc_update's gradient, box projection and clip: it must change with uvc_update."""
    L, H = pre.L, pre.H
    s1p, s2p, s3p = post_sc
    R, gs2, gr2, _ = OU.resource(pre, list(s2p), gate, e1, hp, hard=False, want_grad=True)
    diff = R - hp.budget
    inside = float(-hp.z_grad_clip <= diff.item() <= hp.z_grad_clip)
    cs, cr = pre.s.ceil(), pre.r.ceil()
    gs1, gr1 = torch.zeros(L, 2), torch.zeros(L, H)
    for l in range(L):
        gs1[l, 0] = pre.y[l, 0] * OU.least_sum_and_next(s2p[l], int(cs[l, 0].item()))[1]
        gs1[l, 1] = pre.y[l, 1] * OU.least_sum_and_next(s3p[l], int(cs[l, 1].item()))[1]
        for h in range(H):
            gr1[l, h] = pre.p[l, h] * OU.least_sum_and_next(s1p[l].view(H, -1)[h], int(cr[l, h].item()))[1]
    norms = []
    smax, rmax = box_max(L, H, pre.hd, pre.F)
    for var, ub, g1, g2, vmax in ((pre.s, pre.s_ub, gs1, gs2, smax), (pre.r, pre.r_ub, gr1, gr2, rmax)):
        grad = g1 + hp.sl2wd * (var / ub) + pre.z * (g2 * inside)
        over, under = var >= vmax, var <= 0
        grad[over] = grad[over].clamp(min=0.0)
        grad[under] = grad[under].clamp(max=0.0)
        norms.append(float(grad.abs().max()))
    return float(diff), norms[0], norms[1]


@dataclass
class StepRecord:
    step: int                       # global_step of this update
    W1_pre: List[torch.Tensor]      # the weights the step starts from (the engine is loaded with these)
    W3_pre: List[torch.Tensor]
    sc_pre: tuple                   # oracle scores of them
    W1: List[torch.Tensor]          # after prox_w (the run's live tensors: valid until the next step)
    W3: List[torch.Tensor]
    sc_post: tuple
    pre: OU.UvcState                # s, r, y, p, z before the update
    e1: Optional[torch.Tensor]
    e2: Optional[torch.Tensor]
    gate_grad: torch.Tensor
    ref: dict                       # s r y p z gate cur R2 mx_s mx_r gsum mom counters after the update
    clip_margin: float              # | |R - budget| - z_grad_clip |
    inside: bool
    int_margin: float               # distance of the updated s, r from an integer, entries exactly on a bound aside
    round_margin: float             # rounding_margin of every float64 score sum of this step, before and after prox


def copy_state(st: OU.UvcState) -> OU.UvcState:
    c = OU.UvcState(L=st.L, H=st.H, hd=st.hd, F=st.F)
    for k in ("s", "r", "y", "p", "z", "s_ub", "r_ub", "total_macs"):
        setattr(c, k, getattr(st, k).clone())
    c.embed_macs, c.resource_ub, c.eps = st.embed_macs, st.resource_ub, st.eps
    return c


class OracleRun:
    """One run on the oracle: ``steps()`` yields a StepRecord per update; weights are perturbed between updates."""

    def __init__(self, run: Run):
        L, H, hd, F = run.dims
        self.run, self.hp = run, run_hyper(run)
        self.weights = make_weights(run.wfam, L, H, hd, F, run.seed)
        self.state0 = make_state(run.sfam, L, H, hd, F, run.seed, run.flip)
        self.st = make_oracle_state(L, H, hd, F, run.seed, self.state0)
        self.gate0 = make_gates(L, run.seed)
        self.gate = None if run.mode == "nogate" else self.gate0.clone()
        self.rs = np.random.RandomState(run.seed + 15485863)
        self.noise = np.random.default_rng(run.seed + 32452843)

    def draw(self, shape, kind="exp"):
        a = self.rs.exponential(size=shape) if kind == "exp" else self.rs.standard_normal(shape) * 0.1
        return torch.from_numpy(a.astype(np.float32))

    def steps(self, warmup: int = 0, conditions: bool = False):
        """``conditions``: also work out the rounding margin of every score sum (the CPU test's business; it doubles the cost)."""
        run, st, hp, W = self.run, self.st, self.hp, self.weights
        L, H, hd, F = run.dims
        smax, rmax = box_max(L, H, hd, F)
        for i in range(run.steps):
            step = run.step0 + i
            e1, e2, gg = self.draw((L, 2)), self.draw((L, 2)), self.draw((L, 2), "normal")
            gum = run.mode == "gumbel"
            W1_pre, W3_pre = [w.clone() for w in W.W1], [w.clone() for w in W.W3]
            sc_pre = oracle_scores(W1_pre, W3_pre, H, hd)
            margin = min(rounding_margin(torch.cat(x).numpy()) for x in scores64(W1_pre, W3_pre, H, hd)) if conditions else np.nan
            pre = copy_state(st)
            gate_pre = None if (self.gate is None or not hp.enable_block_gating) else self.gate.clone()
            cur = OU.uvc_update(st, hp, W.W1, W.W3, PROX_LR, self.gate, gg, e1 if gum else None, e2 if gum else None, warmup, step)
            sc_post = oracle_scores(W.W1, W.W3, H, hd)
            if conditions:
                margin = min([margin] + [rounding_margin(torch.cat(x).numpy()) for x in scores64(W.W1, W.W3, H, hd)])
            diff, mx_s, mx_r = primal_norms(pre, hp, sc_post, gate_pre, e1 if gum else None)
            gate_now = None if (self.gate is None or not hp.enable_block_gating) else self.gate
            R2 = float("nan") if warmup else float(OU.resource(st, list(sc_post[1]), gate_now, e2 if gum else None, hp, hard=False))
            gl = st.gating_grad_list
            ref = dict(s=st.s.clone(), r=st.r.clone(), y=st.y.clone(), p=st.p.clone(), z=st.z.clone(),
                       gate=None if self.gate is None else self.gate.clone(), cur=float(cur), R2=R2, mx_s=mx_s, mx_r=mx_r,
                       gsum=torch.cat(gl).sum(0) if gl else torch.zeros(L, 2),
                       mom=None if st.gate_momentum is None else st.gate_momentum.clone(),
                       counters=(len(gl), int(st.gate_momentum is not None)))
            yield StepRecord(step=step, W1_pre=W1_pre, W3_pre=W3_pre, sc_pre=sc_pre, W1=W.W1, W3=W.W3, sc_post=sc_post, pre=pre,
                             e1=e1, e2=e2, gate_grad=gg, ref=ref, clip_margin=abs(abs(diff) - hp.z_grad_clip),
                             inside=abs(diff) <= hp.z_grad_clip,
                             int_margin=min(int_distance(st.s, smax), int_distance(st.r, rmax)), round_margin=margin)
            W.perturb(self.noise)


def oracle_run(run: Run):
    """Walk a run on the oracle alone and return its condition figures: what tests/test_uvc_engine_refs_cpu.py asserts so that the GPU test may
    ask for equal bits with nothing skipped.  clip: the indicator is off its edge; integer: every updated s, r is on a bound or off every
    integer; rounding: no float64 score sum is within ROUND_MARGIN of a float32 rounding boundary."""
    recs = list(OracleRun(run).steps(conditions=True))
    return dict(clip=min(r.clip_margin for r in recs), integer=min(r.int_margin for r in recs), rounding=min(r.round_margin for r in recs),
                inside=[r.inside for r in recs], counters=[r.ref["counters"] for r in recs],
                z=[float(r.ref["z"]) for r in recs], y_min=min(float(r.ref["y"].min()) for r in recs))


# ----------------------------------------------------------------------------- resource evaluations
def resource_draws(case: str, n: int = 2):
    """Seeded Exp(1) draws [L, 2] of a case's uvc_resource evaluations, with the gates they are applied to."""
    _, L, H, hd, F = CASE[case]
    rs = np.random.RandomState(CASES.index(CASE[case]) + 611953 + RESOURCE_SEEDS.get(case, 0))
    return make_gates(L, 0), [torch.from_numpy(rs.exponential(size=(L, 2)).astype(np.float32)) for _ in range(n)]


RESOURCE_SEEDS: dict = {}                          # case -> offset of its draws' seed where the default fails the hard Gumbel gap


def gumbel_gap(g: torch.Tensor, e: torch.Tensor) -> float:
    """min over layers of |y1 - y0| of the Gumbel-softmax sample (oracle.gate_d1)."""
    ysoft = ((g + (-e.log())) / 0.5).softmax(1)
    return float((ysoft[:, 1] - ysoft[:, 0]).abs().min())


# ----------------------------------------------------------------------------- masks
def mask_states(L, H, hd, F, seed):
    """Three non-monotone (s, r) of uvc_write_masks calls: fc2's k goes up, down below the first, and up again."""
    out = []
    for i, fr in enumerate((0.3, 0.1, 0.5)):
        st = make_state("interior", L, H, hd, F, seed + i)
        st["s"][:, 1] = np.floor(fr * (F - 2)) + st["s"][:, 1] % 1.0
        out.append(st)
    out[1]["s"][0, 1] = 0.0                                          # k = 0 once
    out[2]["s"][L - 1, 1] = box_max(L, H, hd, F)[0][L - 1, 1]        # and k = n - 1
    return out


# ----------------------------------------------------------------------------- the engine on the GPU
def ratio(got, ref, rtol, atol) -> float:
    """Largest |got - ref| / (atol + rtol * |ref|)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max())


def bits(t: torch.Tensor) -> torch.Tensor:
    """Integer view for comparisons that must hold for NaN sentinels too."""
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])


class Engine:
    """Device buffers of one (L, H, hd, F) and the six C entries on them.  Every output starts as a sentinel (NaN, or -1 for the ranks) so that an
    element no thread wrote fails a comparison; gsum and the counters, which the kernel reads, start at 0 and the momentum at NaN."""

    def __init__(self, L, H, hd, F, W1, W3, state, seed, gate: Optional[torch.Tensor], eps: float = 0.1, device="cuda"):
        from uvc_amd import _lib as LB
        self.LB, self.lib = LB, LB.lib()
        self.L, self.H, self.hd, self.F, self.D = L, H, hd, F, H * hd
        D = self.D
        self.dims = LB.uvc_dims(L, H, hd, D, F)
        f32, i32 = dict(device=device, dtype=torch.float32), dict(device=device, dtype=torch.int32)
        self.W1 = [w.to(device).contiguous() for w in W1]
        self.W3 = [w.to(device).contiguous() for w in W3]
        self.t1 = torch.tensor([t.data_ptr() for t in self.W1], dtype=torch.int64, device=device)
        self.t3 = torch.tensor([t.data_ptr() for t in self.W3], dtype=torch.int64, device=device)
        self.s, self.r = torch.from_numpy(state["s"].copy()).to(device), torch.from_numpy(state["r"].copy()).to(device)
        self.y, self.p = torch.from_numpy(state["y"].copy()).to(device), torch.from_numpy(state["p"].copy()).to(device)
        self.z = torch.tensor([state["z"]], **f32)
        self.gate = None if gate is None else gate.to(device).contiguous()
        self.gmom = torch.full((L, 2), float("nan"), **f32)
        self.gsum = torch.zeros(L, 2, **f32)
        self.counters = torch.zeros(2, **i32)
        embed, macs = mac_table(L, seed)
        self.total_macs = torch.tensor(np.asarray(macs, dtype=np.float32), device=device)
        self.embed_macs = float(embed)
        self.resource_ub = float((embed + torch.Tensor(macs).sum()) * 2)
        self.eps = eps
        self.ws64 = torch.full((L * (D + F),), float("nan"), device=device, dtype=torch.float64)
        self.sc = [torch.full((L, n), float("nan"), **f32) for n in (D, H, F)]
        self.rk = [torch.full((L, n), -1, **i32) for n in (D, H, F)]
        self.out = torch.full((4,), float("nan"), **f32)
        self.res_out = torch.full((1,), float("nan"), **f32)
        self.masks = None
        self._keep = []

    # -- C structs
    def hyper(self, hp: OU.UvcHyper):
        h = self.LB.uvc_hyper()
        for k in ("budget", "slr", "rlr", "glr", "ylr", "plr", "zlr", "sl2wd", "z_grad_clip", "gating_weight"):
            setattr(h, k, float(getattr(hp, k)))
        h.eps = float(self.eps)
        h.gating_interval, h.use_gumbel, h.enable_block_gating = int(hp.gating_interval), int(hp.use_gumbel), int(hp.enable_block_gating)
        return h

    def state(self, gate_grad=None, **null):
        """uvc_state over this engine's buffers; ``name=None`` keywords null that member."""
        P = self.LB.ptr
        st = self.LB.uvc_state()
        st.s, st.r, st.y, st.p, st.z = P(self.s), P(self.r), P(self.y), P(self.p), P(self.z)
        st.gate, st.gate_grad = P(self.gate), P(gate_grad)
        st.gate_momentum, st.gate_gsum, st.gate_counters = P(self.gmom), P(self.gsum), P(self.counters)
        st.total_macs, st.embed_macs, st.resource_ub = P(self.total_macs), self.embed_macs, self.resource_ub
        st.scores1, st.scores2, st.scores3 = (P(t) for t in self.sc)
        st.rank1, st.rankh, st.rank3 = (P(t) for t in self.rk)
        st.out = P(self.out)
        for k, v in null.items():
            assert v is None
            setattr(st, k, None)
        return st

    # -- entries (each returns the C return code; ``ok`` raises on a non-zero one)
    def ok(self, rc, what):
        self.LB.check(rc, what)

    def scores(self, dims=None):
        P = self.LB.ptr
        return self.lib.uvc_scores(P(self.t1), P(self.t3), dims or self.dims, P(self.ws64), *(P(t) for t in self.sc), self.LB.cur_stream())

    def rank(self, dims=None):
        P = self.LB.ptr
        return self.lib.uvc_rank(*(P(t) for t in self.sc), dims or self.dims, *(P(t) for t in self.rk), self.LB.cur_stream())

    def prox(self, lr, dims=None):
        P = self.LB.ptr
        return self.lib.uvc_prox(P(self.t1), P(self.t3), dims or self.dims, *(P(t) for t in self.rk), P(self.s), P(self.r), P(self.y),
                                 P(self.p), float(lr), P(self.ws64), *(P(t) for t in self.sc), self.LB.cur_stream())

    def dual_step(self, hp, e1, e2, gate_grad, warmup, global_step, dims=None, st=None):
        dev = self.s.device
        e1, e2, gate_grad = (None if t is None else t.to(dev).contiguous() for t in (e1, e2, gate_grad))
        self._keep = [e1, e2, gate_grad]
        st = st if st is not None else self.state(gate_grad)
        return self.lib.uvc_dual_step(C.byref(st), dims or self.dims, self.hyper(hp), self.LB.ptr(e1), self.LB.ptr(e2), int(warmup),
                                      int(global_step), self.LB.cur_stream())

    def resource(self, hp, e, hard, dims=None, st=None, out=True):
        e = None if e is None else e.to(self.s.device).contiguous()
        self._keep = [e]
        st = st if st is not None else self.state()
        return self.lib.uvc_resource(C.byref(st), dims or self.dims, self.hyper(hp), self.LB.ptr(e), int(hard),
                                     self.LB.ptr(self.res_out) if out else 0, self.LB.cur_stream())

    def alloc_masks(self):
        """proj / fc2 masks start as NaN (rebuilt by every call), the fc1 mask at 1 (the kernel only ever writes its zeros)."""
        dev, D, F = self.s.device, self.D, self.F
        self.masks = ([torch.full((D, D), float("nan"), device=dev) for _ in range(self.L)],
                      [torch.full((D, F), float("nan"), device=dev) for _ in range(self.L)],
                      [torch.ones(F, D, device=dev) for _ in range(self.L)])
        self.mask_tables = [torch.tensor([t.data_ptr() for t in ms], dtype=torch.int64, device=dev) for ms in self.masks]

    def write_masks(self, dims=None):
        P = self.LB.ptr
        return self.lib.uvc_write_masks(*(P(t) for t in self.mask_tables), dims or self.dims, *(P(t) for t in self.rk), P(self.s), P(self.r),
                                        self.LB.cur_stream())

    # -- helpers
    def load_weights(self, W1, W3):
        for dst, src in zip(self.W1 + self.W3, list(W1) + list(W3)):
            dst.copy_(src)

    def load_state(self, state):
        for k in ("s", "r", "y", "p"):
            getattr(self, k).copy_(torch.from_numpy(np.asarray(state[k], dtype=np.float32)))
        self.z.fill_(float(state["z"]))

    def reset_outputs(self):
        self.ws64.fill_(float("nan"))
        for t in self.sc:
            t.fill_(float("nan"))
        for t in self.rk:
            t.fill_(-1)

    def outputs(self):
        """name -> tensor of everything any entry may write."""
        d = dict(s=self.s, r=self.r, y=self.y, p=self.p, z=self.z, gmom=self.gmom, gsum=self.gsum, counters=self.counters, ws64=self.ws64,
                 sc1=self.sc[0], sc2=self.sc[1], sc3=self.sc[2], rk1=self.rk[0], rkh=self.rk[1], rk3=self.rk[2], out=self.out,
                 res_out=self.res_out)
        if self.gate is not None:
            d["gate"] = self.gate
        for l in range(self.L):
            d[f"W1.{l}"], d[f"W3.{l}"] = self.W1[l], self.W3[l]
        if self.masks is not None:
            for n, ms in zip(("mproj", "mfc2", "mfc1"), self.masks):
                for l, m in enumerate(ms):
                    d[f"{n}.{l}"] = m
        return d

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: bits(v).clone() for k, v in self.outputs().items()}

    def last_error(self) -> str:
        return self.lib.uvc_last_error().decode()
