"""Plain float64 reference of the attention kernels (uvc_amd/csrc/attention.hip, token_tail.hip), a rounding model of their bf16 mode,
seeded input families and the acceptance rule that holds a kernel to that model.  Torch only, CPU-runnable, nothing from uvc_amd;
tests/test_attention_refs_cpu.py checks the reference against autograd and shows that the rule rejects subtly wrong results,
tests/test_attention_accuracy_gpu.py holds the kernels to it.

Layouts.  One row of ``qkv`` is [q H*64 | k H*64 | v H*v_dim] (the compact layout; v_dim = 64 is the packed [B, N, 3, H, 64]), ``o`` and
``dout`` rows are [H*v_dim].  The token-query form (``ntok``) attends with the first ntok queries only: o / dout are [B, ntok, H*v_dim],
dqkv is whole (dq rows past ntok are zero).  Inside, everything is per head: q, k [B, H, N, 64], v [B, H, N, v_dim].

The rounding model is the float64 computation with a bf16 rounding at the points a bf16 kernel must round -- its MFMA operands and its
outputs -- and nowhere else (see ``Rounding``).  ``accept`` bounds a kernel's error against float64 by MARGIN times the model's, per
(image, head) and per row.  Where the exact result is a difference that cancels (dq, dk of the routing family and of N = 1: the model's
error there is 0 to ~1e-13, a float32 kernel's ~1e-6) the model says nothing about float32 arithmetic.  There a first-order bound of what
float32 adds (``reference``'s "floor") takes the model's place -- only where the model's error is negligible against it (CANCELS: margin times
the model's error below a thousandth of the floor; ordinary bf16 rounding, ~1e-3 relative, is never that small against a float32 bound).
Everywhere else the plain margin holds and the floor plays no part."""
from __future__ import annotations

from collections import namedtuple

import torch

HD = 64
SCALE = HD ** -0.5
MARGIN, ROW_MARGIN = 3.0, 4.0
CANCELS = 1e-3                       # the floor replaces the model only where margin * (model error) < CANCELS * floor
SECTIONS = ("o", "dq", "dk", "dv")
U32 = 2.0 ** -24                     # unit roundoff of float32


def f64(t):
    return t.detach().to(torch.float64)


def bf(t):
    """Round to bf16 (nearest even, through float32 as the kernels hold their values) and return float64."""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


# ----------------------------------------------------------------------------- layouts
def split_qkv(qkv, H, v_dim=HD):
    """[B, N, H*(128 + v_dim)] (any trailing shape with that many elements per token) -> q, k [B, H, N, 64], v [B, H, N, v_dim]."""
    B, N = qkv.shape[:2]
    x = qkv.reshape(B, N, H * (2 * HD + v_dim))
    q = x[..., :H * HD].reshape(B, N, H, HD).transpose(1, 2)
    k = x[..., H * HD:2 * H * HD].reshape(B, N, H, HD).transpose(1, 2)
    v = x[..., 2 * H * HD:].reshape(B, N, H, v_dim).transpose(1, 2)
    return q, k, v


def join_qkv(q, k, v):
    """The inverse of split_qkv: [B, N, H*(128 + v_dim)]."""
    B, H, N, _ = q.shape
    return torch.cat([t.transpose(1, 2).reshape(B, N, -1) for t in (q, k, v)], -1)


def heads(o, H):
    """[B, Nq, H*d] -> [B, H, Nq, d]."""
    B, Nq = o.shape[:2]
    return o.reshape(B, Nq, H, -1).transpose(1, 2)


def rows(o):
    """[B, H, Nq, d] -> [B, Nq, H*d]."""
    B, H, Nq, _ = o.shape
    return o.transpose(1, 2).reshape(B, Nq, -1)


# ----------------------------------------------------------------------------- reference and rounding model
Rounding = namedtuple("Rounding", "p_fwd p_bwd ds delta_from_o out")

# k_attn_fwd / k_attn_bwd_dq / k_attn_bwd_dkv (and their streaming forms k_attn_*_long, the same tile bodies):
#   forward   attn_key_block: st = exp2(s c2 - max c2) is packed to bf16 (Mma::pack) as the B operand of O^T = V^T P^T, `sum` adds the unpacked
#             values, the output is ot / l_run rounded once in store_out;
#   backward  k_attn_bwd_dkv packs pp (P, for dV) and ds (dS, for dK), k_attn_bwd_dq packs ds (for dQ); dl = rowsum(dO * O) over the bf16 o and
#             dout the caller passes (frag_dot); dq, dk, dv leave through store_tile16 / store_out, rounded once.
PAIR = Rounding(p_fwd=True, p_bwd=True, ds=True, delta_from_o=True, out=True)
# one::k_attn_bwd_one (variant 2): `pf = pack4(pp), dsf = pack4(ds)` in step() feed dV, dK and -- through the exchange tile -- dQ; the helper waves take
# delta from the bf16 dO and O rows (`frag_dot<T>(x, ov[i])`); results leave as pack4(dq / dk / dv).  The same points as the pair today.  It is a
# Rounding of its own so that a point the kernel gains (say a bf16 delta, or dP packed for a further product) becomes a new field of Rounding, set here
# and read in attention() where that value is formed, without touching the pair's model.
ONE_PASS = PAIR._replace()
# token_tail.hip k_attn_tok_fwd / k_attn_tok_bwd: scalar float32 throughout (p = e / z in LDS as float, sDS float, delta = block_sum(p * dp) from its own
# softmax, not from o); only ElemIO::store / Row::store8 round, once, on the way out.
TOKEN = Rounding(p_fwd=False, p_bwd=False, ds=False, delta_from_o=False, out=True)
EXACT = Rounding(False, False, False, False, False)


def attention(qkv, dout, H, v_dim=HD, ntok=None, rounding=EXACT, o_given=None, backward=True, floor=False):
    """softmax(q k^T / 8) v and its gradients in float64 with ``rounding``'s bf16 roundings.  ``o_given`` ([B, Nq, H*v_dim]): the o the backward
    takes delta from (a kernel's own bf16 output); default: this computation's o.  Returns per-head tensors o [B, H, Nq, v_dim], lse, delta
    [B, H, Nq], dq, dk [B, H, N, 64], dv [B, H, N, v_dim], and with ``floor`` the elementwise float32 bounds described in ``reference``."""
    R = rounding
    q, k, v = (f64(t) for t in split_qkv(qkv, H, v_dim))
    N = q.shape[2]
    Nq = N if ntok is None else ntok
    qq = q[:, :, :Nq]
    s = qq @ k.transpose(-1, -2) * SCALE
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    lse = (m + l.log()).squeeze(-1)
    o = ((bf(e) if R.p_fwd else e) @ v) / l
    if R.out:
        o = bf(o)
    out = dict(o=o, lse=lse)
    P = torch.exp(s - lse[..., None])
    if floor:
        # |delta s| <= 64 u |q|.|k| / 8 (a 64-term float32 chain), lse and the exponent's own arithmetic a few u more: the relative error of P
        relP = U32 * (64.0 * (qq.abs() @ k.abs().transpose(-1, -2)) * SCALE + 4.0 * lse.abs()[..., None] + 4.0)
        acc = U32 * (N + HD)                                 # an N-term float32 accumulation (and the output's own operations)
        fl = dict(o=(P * (relP + acc)) @ v.abs())
    if backward:
        do = f64(heads(dout, H))
        dP = do @ v.transpose(-1, -2)
        o_in = f64(heads(o_given, H)) if o_given is not None else o
        delta = (do * o_in).sum(-1) if (R.delta_from_o or o_given is not None) else (P * dP).sum(-1)
        dS = P * (dP - delta[..., None]) * SCALE
        Pb, dSb = (bf(P) if R.p_bwd else P), (bf(dS) if R.ds else dS)
        dq = torch.zeros_like(q)
        dq[:, :, :Nq] = dSb @ k
        dk, dv = dSb.transpose(-1, -2) @ qq, Pb.transpose(-1, -2) @ do
        if R.out:
            dq, dk, dv = bf(dq), bf(dk), bf(dv)
        out.update(delta=delta, dq=dq, dk=dk, dv=dv)
        if floor:
            dPbar = 64.0 * U32 * (do.abs() @ v.abs().transpose(-1, -2))
            dbar = 64.0 * U32 * (do.abs() * o_in.abs()).sum(-1)
            dSbar = SCALE * (P * relP * (dP - delta[..., None]).abs() + P * (dPbar + dbar[..., None])) + 4.0 * U32 * dS.abs()
            dSa = dSbar + acc * dS.abs()
            fq = torch.zeros_like(q)
            fq[:, :, :Nq] = dSa @ k.abs()
            fl.update(dq=fq, dk=dSa.transpose(-1, -2) @ qq.abs(), dv=(P * (relP + acc)).transpose(-1, -2) @ do.abs())
    if floor:
        out["floor"] = fl
    return out


def reference(qkv, dout, H, v_dim=HD, ntok=None, backward=True):
    """The float64 result, with "floor": per element, a first-order bound of the error that float32 arithmetic on exact operands adds -- a
    64-term chain for each score, dP and delta (64 u times the sum of the absolute products), N-term chains for the outputs, the relative
    error of P = exp(s - lse) from the absolute error of its exponent -- carried through the same products with absolute values."""
    return attention(qkv, dout, H, v_dim, ntok, EXACT, None, backward, floor=True)


def model(qkv, dout, H, v_dim=HD, ntok=None, rounding=PAIR, o_given=None, backward=True):
    return attention(qkv, dout, H, v_dim, ntok, rounding, o_given, backward)


def dqkv_of(res):
    """dq, dk, dv of a result as rows of dqkv."""
    return join_qkv(res["dq"], res["dk"], res["dv"])


def got_from(o, dqkv, H, v_dim=HD):
    """A kernel's o [B, Nq, H*v_dim] and dqkv (or None) as the per-head float64 dict ``accept`` takes."""
    got = dict(o=f64(heads(o, H)))
    if dqkv is not None:
        got["dq"], got["dk"], got["dv"] = (f64(t) for t in split_qkv(dqkv, H, v_dim))
    return got


# ----------------------------------------------------------------------------- acceptance
def accept(got, ref, mod, sections=SECTIONS, together=None, margin=MARGIN, row_margin=ROW_MARGIN):
    """Holds ``got`` to the rounding model, per section and per (image, head) -- over all heads together when ``together`` (default: N < 17,
    where a head has too few elements for its own error norm to be stable):
      * ||got - ref|| <= margin * ||mod - ref||                          (the relative L2 errors against float64, times ||ref||)
      * the same per query / key row against row_margin * the largest row error of the model in that head
      * only where the model's error is negligible (margin * model error < CANCELS * floor, norms over the same head / row: the exact result
        cancels and the model says nothing about float32) an error within the float32 floor is accepted instead
      * no element is NaN -- which also says that a NaN prefill was overwritten everywhere.
    Raises AssertionError naming the first violation; returns {section: (worst head ratio, worst row ratio, worst head ratio with no floor at all)}: error /
    model error, the first two counted as 0 where the result cancels and the error lies within the floor; they are what the margins are compared with."""
    worst = {}
    all_heads = together
    for sec in sections:
        g, r, m, f = got[sec], ref[sec], mod[sec], ref["floor"][sec]
        together = r.shape[2] < 17 if all_heads is None else all_heads
        assert g.shape == r.shape, (sec, tuple(g.shape), tuple(r.shape))
        nan = torch.isnan(g)
        assert not bool(nan.any()), f"{sec}: {int(nan.sum())} NaN elements, first at (image, head, row, col) {tuple(nan.nonzero()[0].tolist())}"
        eg, em = (g - r).square().sum(-1), (m - r).square().sum(-1)                  # squared row errors [B, H, N]
        fr = f.square().sum(-1)
        hd = (0, 1, 2) if together else (2,)
        Eg, Em, Fh = eg.sum(hd, keepdim=True).sqrt(), em.sum(hd, keepdim=True).sqrt(), fr.sum(hd, keepdim=True).sqrt()
        head_ratio = _ratio(Eg, Em, Fh, margin)
        row_ratio = _ratio(eg.sqrt(), em.amax(hd, keepdim=True).sqrt().expand_as(eg), fr.sqrt(), row_margin)
        worst[sec] = (float(head_ratio.max()), float(row_ratio.max()), float(_ratio(Eg, Em, torch.zeros_like(Fh), margin).max()))
        if float(head_ratio.max()) > margin:
            i = tuple((head_ratio == head_ratio.max()).nonzero()[0].tolist())
            raise AssertionError(f"{sec}: L2 error {float(Eg[i]):.3e} is {float(head_ratio.max()):.2f} x the rounding model's {float(Em[i]):.3e} "
                                 f"(margin {margin}, float32 floor {float(Fh[i]):.3e}) at (image, head) {i[:2]}")
        if float(row_ratio.max()) > row_margin:
            i = tuple((row_ratio == row_ratio.max()).nonzero()[0].tolist())
            raise AssertionError(f"{sec}: row error {float(eg[i].sqrt()):.3e} is {float(row_ratio.max()):.2f} x the model's largest row error in that head "
                                 f"(margin {row_margin}) at (image, head, row) {i}")
    return worst


def _ratio(err, base, floor, margin):
    """err / base; 0 where the model's error is negligible against the floor (CANCELS) and err lies within the floor; inf where another error meets a
    model without error."""
    z = torch.zeros_like(err)
    return torch.where((err == 0) | ((err <= floor) & (margin * base < CANCELS * floor)), z, torch.where(base > 0, err / base.clamp_min(1e-300), torch.full_like(err, float("inf"))))


# ----------------------------------------------------------------------------- input families
RANDOM, NEGATIVE, ROUTING, DEEP_NEGATIVE = 1, 2, 3, 4
FAMILY_NAMES = {RANDOM: "random", NEGATIVE: "negative", ROUTING: "routing", DEEP_NEGATIVE: "deep-negative"}


def _bf_exact(t):
    return t.to(torch.bfloat16).to(torch.float32)


def make_inputs(family, B, N, H, v_dim=HD, ntok=None, seed=0):
    """bf16-exact float32 CPU tensors qkv [B, N, H*(128 + v_dim)], dout [B, Nq, H*v_dim], and the routing map t [B, H, N] (None elsewhere).
      1 random         unit-normal q, k, v, dout
      2 negative       q = .5 r + 16 u, k = .5 r - 16 u with a random unit vector u per head: every scaled score is about -26 .. -32, so a padded
                       key's score of 0 would take the whole row
      3 routing        keys of norm 16 in random directions, q_i = 2 k_t(i) for a bijection t with t(0) = N - 1: row i puts all its weight on key
                       t(i) (scaled score 64 against 64 cos elsewhere), so o_i = v_t(i) and dv_t(i) = dout_i exactly in bf16 (check_routing)
      4 deep negative  family 2 with 28 in place of 16: scores about -98 and lse about -91 +- 2: in most rows lse < -88.72, where
                       exp(-lse) overflows float32"""
    g = torch.Generator().manual_seed(1000003 * family + 7919 * seed + N)
    Nq = N if ntok is None else ntok
    r = lambda *shape: torch.randn(*shape, generator=g)
    q, k, v = r(B, H, N, HD), r(B, H, N, HD), r(B, H, N, v_dim)
    dout = r(B, Nq, H * v_dim)
    t = None
    if family in (NEGATIVE, DEEP_NEGATIVE):
        u = r(B, H, 1, HD)
        u = u / u.norm(dim=-1, keepdim=True) * (16.0 if family == NEGATIVE else 28.0)
        q, k = 0.5 * q + u, 0.5 * k - u
    elif family == ROUTING:
        k = _bf_exact(k / k.norm(dim=-1, keepdim=True) * 16.0)
        t = torch.stack([torch.randperm(N, generator=g) for _ in range(B * H)]).view(B, H, N)
        for tt in t.view(-1, N):                           # t(0) = N - 1, still a bijection (so some i has t(i) = 0)
            j = int((tt == N - 1).nonzero())
            tt[j], tt[0] = tt[0].clone(), N - 1
        q = 2.0 * torch.gather(k, 2, t[..., None].expand(-1, -1, -1, HD))
    elif family != RANDOM:
        raise ValueError(family)
    return _bf_exact(join_qkv(q, k, v)).contiguous(), _bf_exact(dout).contiguous(), t


def routed(x, t, inverse=False):
    """x [B, H, N, d] gathered along the routing map: row i <- x[t(i)] (rows :Nq of t when x is shorter); inverse: row t(i) <- x[i]."""
    d = x.shape[-1]
    if inverse:
        n = x.shape[2]
        out = torch.zeros(*t.shape, d, dtype=x.dtype, device=x.device)
        return out.scatter_(2, t[:, :, :n, None].expand(-1, -1, -1, d), x)
    return torch.gather(x, 2, t[..., None].expand(-1, -1, -1, d))


def routing_exact(o, dv, qkv, dout, t, H, v_dim=HD):
    """The routing family's exact statements of per-head results o [B, H, Nq, v_dim] and dv [B, H, N, v_dim] (or None), after rounding them to
    bf16: o_i == v_t(i) for every query, dv_t(i) == dout_i for every query row i.  Returns (o holds, dv holds)."""
    v = split_qkv(qkv, H, v_dim)[2].to(o.device, torch.float64)
    Nq = o.shape[2]
    t = t.to(o.device)
    ok_o = torch.equal(bf(o), routed(v, t)[:, :, :Nq])
    if dv is None:
        return ok_o, True
    do = heads(dout, H).to(o.device, torch.float64)
    tq = t[:, :, :Nq]
    return ok_o, torch.equal(torch.gather(bf(dv), 2, tq[..., None].expand(-1, -1, -1, v_dim)), do)


def make_case(family, B, N, H, v_dim=HD, ntok=None, seed=0, device="cpu", backward=True):
    """Inputs of a family on ``device`` with their float64 reference; the routing family is redrawn (at most 4 times) until its reference
    satisfies routing_exact, and raises if none does.  Returns dict(qkv, dout, t, ref, family, B, N, H, v_dim, ntok)."""
    for attempt in range(4):
        qkv, dout, t = make_inputs(family, B, N, H, v_dim, ntok, seed + 101 * attempt)
        qkv, dout = qkv.to(device), dout.to(device)
        ref = reference(qkv, dout, H, v_dim, ntok, backward)
        if family != ROUTING or all(routing_exact(ref["o"], ref.get("dv"), qkv, dout, t, H, v_dim)):
            return dict(qkv=qkv, dout=dout, t=t, ref=ref, family=family, B=B, N=N, H=H, v_dim=v_dim, ntok=ntok)
    raise RuntimeError(f"routing family: no draw with an exact float64 reference at B, N, H = {B}, {N}, {H}")
