"""GPU: the small kernels of elementwise.hip and loss_optim.hip (gates, scores, masks, column sums, token assembly, MLP compaction,
distillation loss, global-norm clip + AdamW) called directly through ``ops``, each against the float64 references of
tests/small_kernel_refs.py, at the smallest shapes that reach every path: scalar tails (n % 4), grids past their block caps, mixed
flag quads, skipped quads, ragged tiles.  Every output written as ``beta_acc * old + value`` is run with beta_acc = 0 over a buffer
of NaN (the old contents must not be read) and with beta_acc = 1 over known values (they must be added)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import small_kernel_refs as R

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1


def dev():
    return torch.device("cuda")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev())


def to_t(x, dtype):
    return x if dtype == F32 else x.to(torch.bfloat16)


def tol(dtype):
    return dict(rtol=2e-5, atol=2e-5) if dtype == F32 else dict(rtol=2e-2, atol=2e-2)


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), device=dev(), dtype=dtype)


def f32(x):
    """The float32 value nearest to x as a Python float: what a ``float`` argument of the C ABI receives."""
    return float(np.float32(x))


def close64(got, want, **kw):
    assert torch.isfinite(got).all()
    torch.testing.assert_close(got.double().cpu(), want.double().cpu(), **kw)


def both_betas(run, value, **kw):
    """run(out, beta_acc) writes ``out``; ``value``: float64 reference of the written value."""
    out = nans(*value.shape)
    run(out, 0.0)
    close64(out, value, **kw)
    old = rnd(*value.shape, seed=999)
    out = old.clone()
    run(out, 1.0)
    close64(out, old.double().cpu() + value.double().cpu(), **kw)


# ============================================================================= clip + AdamW
# The ABI carries the hyper-parameters as float: the reference is evaluated at the float32 values the kernel receives (1 - float(.999)
# differs from 1e-3 by 1.3e-5 relative, which is no rounding error of the kernel).
HP = dict(lr=f32(3e-4), beta1=f32(0.9), beta2=f32(0.999), eps=f32(1e-8), weight_decay=f32(0.05))
ADAMW_TOL = dict(rtol=2e-6, atol=1e-7)


def adamw_ref(p, g, m, v, sq, step, max_norm, flags):
    return R.adamw_ref(p, g, m, v, sq, HP["lr"], step, (HP["beta1"], HP["beta2"]), HP["eps"], HP["weight_decay"], max_norm, flags)


def adamw_state(n, seed):
    return rnd(n, seed=seed), rnd(n, seed=seed + 1, scale=0.01), rnd(n, seed=seed + 2, scale=0.01) ** 2 + 1e-6


def flag_bytes(n):
    fl = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    for q in (0, 600):                                       # in the first and in the last workgroup
        fl[4 * q:4 * q + 16] = torch.tensor([2, 3, 2, 3,     # all frozen, mixed decay bits: the quad is skipped
                                             2, 1, 0, 3,     # frozen, decay, no decay, frozen | decay
                                             1, 1, 1, 1, 0, 0, 0, 0], dtype=torch.uint8)
    fl[n - 3:] = torch.tensor([0, 1, 2], dtype=torch.uint8)  # the scalar tail
    return fl


@pytest.mark.parametrize("with_shadow", [True, False])
@pytest.mark.parametrize("with_flags", [True, False])
def test_adamw_flag_quads_and_tail(with_shadow, with_flags):
    from uvc_amd import ops
    n = 4 * 256 * 3 + 3
    p, m, v = adamw_state(n, 100)
    flags = flag_bytes(n).to(dev()) if with_flags else None
    frozen = (flags & R.FROZEN) != 0 if with_flags else torch.zeros(n, dtype=torch.bool, device=dev())
    assert not with_flags or (int(frozen.sum()) > 100 and int(((flags & R.DECAY) != 0).sum()) > 100)
    shadow = p.bfloat16() if with_shadow else None
    partial, sq, gn = torch.empty(1024, device=dev()), torch.empty(2, device=dev()), torch.empty(1, device=dev())
    for step, gscale, clipped in ((1, 0.5, True), (2, 1e-3, False), (1000, 0.1, True)):
        g = rnd(n, seed=110 + step, scale=gscale)
        ops.grad_sqnorm(g, partial, sq)
        assert (float(sq[1]) > 1.0) == clipped
        p0, m0, v0 = p.clone(), m.clone(), v.clone()
        ops.adamw_step(p, g, m, v, sq, step=step, max_norm=1.0, p_shadow=shadow, gnorm_out=gn, flags=flags, **HP)
        pr, mr, vr = adamw_ref(p0, g, m0, v0, float(sq[0]), step, 1.0, flags)
        close64(p, pr, **ADAMW_TOL)
        close64(m, mr, **ADAMW_TOL)
        close64(v, vr, **ADAMW_TOL)
        for new, old in ((p, p0), (m, m0), (v, v0)):
            assert torch.equal(new[frozen], old[frozen])
            assert int((new[~frozen] != old[~frozen]).sum()) > 0.99 * int((~frozen).sum())
        if with_shadow:
            assert torch.equal(shadow, p.bfloat16())
        assert float(gn[0]) == float(sq[1])
        close64(gn[0], torch.tensor(math.sqrt(float(sq[0]))), rtol=2e-7, atol=0)


def test_adamw_past_the_block_cap():
    from uvc_amd import ops
    n = 2048 * 256 * 4 + 4 * 256 + 3
    p, m, v = adamw_state(n, 120)
    g = rnd(n, seed=125, scale=0.01)
    shadow = p.bfloat16()
    partial, sq = torch.empty(1024, device=dev()), torch.empty(2, device=dev())
    ops.grad_sqnorm(g, partial, sq)
    p0, m0, v0 = p.clone(), m.clone(), v.clone()
    ops.adamw_step(p, g, m, v, sq, step=1, max_norm=1.0, p_shadow=shadow, **HP)
    pr, mr, vr = adamw_ref(p0, g, m0, v0, float(sq[0]), 1, 1.0, None)
    for got, want, old in ((p, pr, p0), (m, mr, m0), (v, vr, v0)):
        close64(got[-2000:], want[-2000:], **ADAMW_TOL)
        assert not (got[-2000:] == old[-2000:]).any()            # the wrapped quads and the tail were stepped, once
        close64(got, want, **ADAMW_TOL)
    assert torch.equal(shadow, p.bfloat16())


def test_adamw_without_clipping():
    """FusedAdamW without max_grad_norm: max_norm = inf over a zeroed sq.  A zero gradient under a finite max_norm only decays."""
    from uvc_amd import ops
    n = 1027
    p, m, v = adamw_state(n, 130)
    g = rnd(n, seed=135, scale=3.0)
    sq = torch.zeros(2, device=dev())
    p0 = p.clone()
    m1, v1 = m.clone(), v.clone()
    ops.adamw_step(p, g, m1, v1, sq, step=7, max_norm=float("inf"), **HP)
    pr, mr, vr = adamw_ref(p0, g, m, v, 0.0, 7, float("inf"), None)
    close64(p, pr, **ADAMW_TOL)
    close64(m1, mr, **ADAMW_TOL)
    close64(v1, vr, **ADAMW_TOL)
    p, z = p0.clone(), torch.zeros(n, device=dev())
    m, v = z.clone(), z.clone()
    ops.adamw_step(p, z, m, v, sq, step=1, max_norm=1.0, **HP)
    close64(p, p0.double() * (1.0 - HP["lr"] * HP["weight_decay"]), **ADAMW_TOL)
    assert not m.any() and not v.any()


def test_grad_sqnorm_segments_accumulate():
    from uvc_amd import ops
    segs = [rnd(k, seed=140 + i, scale=s) for i, (k, s) in enumerate(((3, 2.0), (1024 * 256 * 4 + 4 * 7 + 1, 0.01), (100003, 0.05)))]
    segs[1][1024 * 256 * 4:] = 10.0          # the quads past the block cap and the tail carry most of the norm: losing one shows
    segs[2][-3:] = 10.0
    partial, sq = torch.empty(1024, device=dev()), nans(2)
    total = 0.0
    for i, g in enumerate(segs):
        ops.grad_sqnorm(g, partial, sq, accumulate=i > 0)
        total += float((g.double() ** 2).sum())
        close64(sq[1], torch.tensor(math.sqrt(total)), rtol=1e-5, atol=0)
        close64(sq[0], sq[1].double() ** 2, rtol=2.5e-7, atol=0)          # sqrt and the square each round once
    ops.grad_sqnorm(segs[2], partial, sq, accumulate=False)                 # forgets what came before
    close64(sq[1], segs[2].double().norm(), rtol=1e-5, atol=0)
    ops.grad_sqnorm(segs[0], partial, sq, accumulate=False)                 # the tail alone
    close64(sq[1], segs[0].double().norm(), rtol=1e-5, atol=0)
    from uvc_amd._lib import UvcHipError
    with pytest.raises(UvcHipError):
        ops.grad_sqnorm(segs[2][1:], partial, sq)


@pytest.mark.parametrize("n", [1, 256 * 256 + 5])
def test_scale_by_clip(n):
    from uvc_amd import ops
    g0 = rnd(n, seed=150)
    for sumsq, max_norm in ((9.0, 1.0), (0.25, 1.0)):                         # norm 3: scaled; norm .5: untouched
        sq = torch.tensor([sumsq, math.sqrt(sumsq)], device=dev())
        g = g0.clone()
        ops.scale_by_clip(g, sq, max_norm)
        close64(g, g0.double() * R.clip_coef(sumsq, max_norm), rtol=1e-6, atol=0)


# ============================================================================= distillation loss
LOSS_SHAPES = [(1, 1), (3, 10), (2, 63), (2, 257), (300, 16), (4, 1000)]


def loss_inputs(B, C, scale):
    o, okd, t = rnd(B, C, seed=201, scale=scale), rnd(B, C, seed=202, scale=scale), rnd(B, C, seed=203, scale=scale)
    y = F.softmax(rnd(B, C, seed=204) * 2, -1) * torch.tensor([0.7, 1.3, 1.0])[torch.arange(B) % 3, None].to(dev())    # row sums
    if C > 1:
        y[0, ::2] = 0.0                                        # exact zeros in a target row
    return o, okd, y.contiguous(), t


def run_loss(o, okd, y, t, alpha, tau, kind, d_o=None, d_k=None):
    from uvc_amd import ops
    B, C = o.shape
    loss, scratch = nans(1), nans(B)
    d_o = nans(B, C) if d_o is None else d_o
    if kind == 0:
        ops.distill_loss(o, None, y, None, loss, d_o, None, scratch, alpha, tau, kind=0)
        return loss, d_o, None
    d_k = nans(B, C) if d_k is None else d_k
    ops.distill_loss(o, okd, y, t, loss, d_o, d_k, scratch, alpha, tau, kind=kind)
    return loss, d_o, d_k


def check_loss(o, okd, y, t, alpha, tau, kind, widen=1.0):
    loss, d_o, d_k = run_loss(o, okd, y, t, alpha, tau, kind)
    rl, rdo, rdk = R.distill_loss_ref(o, okd, y, t, alpha, tau, kind)
    close64(loss[0], rl, rtol=1e-5, atol=1e-6 * widen)
    close64(d_o, rdo, rtol=1e-4, atol=1e-7 * widen)
    if kind:
        close64(d_k, rdk, rtol=1e-4, atol=1e-7 * widen)
    return loss, d_o, d_k


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("B,C", LOSS_SHAPES)
def test_distill_loss_shapes_targets_and_hyperparameters(B, C, kind):
    o, okd, y, t = loss_inputs(B, C, 2.0)
    sums = y.sum(-1).tolist()
    assert (C > 1 or abs(sums[0] - 0.7) < 1e-6) and (B < 2 or abs(sums[1] - 1.3) < 1e-5) and (C == 1 or sums[0] < 0.7)
    for tau in (0.5, 1.0, 4.0):
        for alpha in (0.0, 0.1, 1.0):
            loss, d_o, d_k = check_loss(o, okd, y, t, alpha, tau, kind)
            if C == 1 and kind:
                assert not d_k.any()                           # one class: softmax is 1 whatever the logit


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("B,C", [(3, 10), (4, 1000)])
def test_distill_loss_wide_logits(B, C, kind):
    """Logits over about +-70: most classes underflow in the fast exponential.  The absolute tolerances of |o| <~ 8 scale with
    max|o| / 8 (every term of the loss is a sum of products of that magnitude); the relative ones stay."""
    o, okd, y, t = loss_inputs(B, C, 20.0)
    widen = float(max(o.abs().max(), okd.abs().max(), t.abs().max())) / 8.0
    assert widen > 4
    for tau, alpha in ((1.0, 0.1), (4.0, 1.0), (0.5, 0.1)):
        check_loss(o, okd, y, t, alpha, tau, kind, widen)


@pytest.mark.parametrize("kind", [1, 2])
def test_distill_loss_gradient_buffer_aliasing(kind):
    """The three behaviours include/uvc_kernels.h states for d_o / d_okd."""
    B, C, alpha, tau = 3, 10, 0.3, 2.0
    o, okd, y, t = loss_inputs(B, C, 2.0)
    gt = dict(rtol=1e-4, atol=1e-7)
    _, rdo, rdk = R.distill_loss_ref(o, okd, y, t, alpha, tau, kind)
    _, d_o, d_k = run_loss(o, okd, y, t, alpha, tau, kind)                  # separate inputs, separate buffers
    close64(d_o, rdo, **gt)
    close64(d_k, rdk, **gt)
    shared = nans(B, C)
    run_loss(o, okd, y, t, alpha, tau, kind, d_o=shared, d_k=shared)       # separate inputs, one buffer: the sum
    close64(shared, rdo + rdk, **gt)
    rl, rsum, none = R.distill_loss_ref(o, o, y, t, alpha, tau, kind)
    assert none is None
    shared = nans(B, C)
    loss, _, _ = run_loss(o, o, y, t, alpha, tau, kind, d_o=shared, d_k=shared)   # one head, one buffer: the sum
    close64(shared, rsum, **gt)
    close64(loss[0], rl, rtol=1e-5, atol=1e-6)


def test_distill_loss_hard_teacher_ties():
    B, C = 2, 257                                              # the last two classes belong to different passes of the class loop
    o, okd, y, t = loss_inputs(B, C, 2.0)
    t[0] = 0.25                                                # all equal: class 0
    t[1, C - 2:] = t[1].max() + 1.0                            # tie of the last two: the lower one
    assert t.cpu().argmax(dim=1).tolist() == [0, C - 2]
    _, _, d_k = check_loss(o, okd, y, t, 0.5, 1.0, 2)
    assert float(d_k[0, 0]) < 0 and float(d_k[1, C - 2]) < 0 and int((d_k < 0).sum()) == 2


# ============================================================================= patch gates, scores, outer product
@pytest.mark.parametrize("B,P", [(1, 1), (3, 196), (5, 257)])
def test_patch_gate_sigmoid(B, P):
    """Soft: rtol 4e-6 -- the fast exponential scales its argument by log2(e) in float32 (|x| 2^-24 <= 1.2e-6 relative at |x| = 20),
    the instruction adds about 1e-7, sigmoid does not amplify either; the rest is margin for the division.  Hard: bit exact."""
    from uvc_amd import ops
    pg = torch.linspace(-20.0, 20.0, P).to(dev()) if P > 1 else torch.tensor([-20.0], device=dev())
    mask = nans(B, P)
    ops.patch_gate_sigmoid(pg, mask, B, P, False)
    close64(mask, R.sigmoid_gate_ref(pg, B, False), rtol=4e-6, atol=1e-12)
    gen = torch.Generator().manual_seed(7)
    mag = torch.exp(torch.empty(P).uniform_(math.log(1.1e-3), math.log(20.0), generator=gen))
    hp = mag * (torch.randint(0, 2, (P,), generator=gen) * 2 - 1)
    special = torch.tensor([-5.0, 0.0, -0.0, 100.0, -100.0, 1e4, -1e4, 1e-3, -1e-3])
    hp[:min(P, len(special))] = special[:P]
    assert hp[0] == -5 and (P == 1 or bool(((hp.abs() >= 1e-3) | (hp == 0)).all()))
    hp = hp.to(dev())
    mask = nans(B, P)
    ops.patch_gate_sigmoid(hp, mask, B, P, True)
    want = R.sigmoid_gate_ref(hp, B, True)
    assert torch.equal(mask.cpu().double(), want)
    if P > 8:
        assert want[0, :9].tolist() == [1, 1, 1, 1, 0, 1, 0, 1, 0] and 0.3 < float(want.mean()) < 0.7


@pytest.mark.parametrize("B,P", [(1, 1), (3, 196), (5, 257), (512, 16)])
def test_patch_gate_sigmoid_bwd(B, P):
    from uvc_amd import ops
    pg = torch.linspace(-6.0, 6.0, P).to(dev()) if P > 1 else torch.tensor([0.7], device=dev())
    dmask = rnd(B, P, seed=301)
    both_betas(lambda out, beta: ops.patch_gate_sigmoid_bwd(pg, dmask, out, B, P, beta), R.sigmoid_gate_bwd_ref(pg, dmask), **tol(F32))


@pytest.mark.parametrize("rows", [1, 5, 4 * 49 + 3])
@pytest.mark.parametrize("D", [64, 100, 192, 768])
def test_patch_scores(rows, D):
    from uvc_amd import ops
    pe, w, bias = rnd(rows, D, seed=311), rnd(D, seed=312, scale=D ** -0.5), rnd(1, seed=313)
    scores = nans(rows)
    ops.patch_scores(pe, w, bias, scores, rows, D)
    close64(scores, R.patch_scores_ref(pe, w, bias), **tol(F32))


@pytest.mark.parametrize("mode", ["f32", "bf16", "f32_under_bf16"])
@pytest.mark.parametrize("rows,D", [(1, 4), (591, 192), (4097, 100), (1400, 768)])
def test_add_outer(rows, D, mode):
    from uvc_amd import ops
    X0 = rnd(rows, D, seed=321)
    if mode == "bf16":
        X0 = X0.bfloat16()
    rw, w = rnd(rows, seed=322), rnd(D, seed=323)
    X = X0.clone()
    ops.add_outer(X, rw, w, rows, D, F32 if mode == "f32" else BF16)
    ref = R.add_outer_ref(X0, rw, w)
    if mode == "bf16":                  # one rounding to nearest of the float32 sum (a tie may flip)
        assert X.dtype == torch.bfloat16 and torch.isfinite(X).all()
        err = (X.double().cpu() - ref).abs()
        bad = err > 2.0 ** -8 * ref.abs() + 1e-30
        assert not bad.any(), (int(bad.sum()), float((err / ref.abs()).max()))
    else:                               # one fused or two separate float32 roundings
        close64(X, ref, rtol=1e-6, atol=1e-6)


# ============================================================================= masks
@pytest.mark.parametrize("n", [1, 3, 4, 7, 4096 * 256 * 4 + 4 * 300 + 2])
def test_apply_masks(n):
    from uvc_amd import ops
    gen = torch.Generator().manual_seed(n)
    nq = (n + 3) // 4
    kind = torch.randint(0, 3, (nq,), generator=gen)            # per quad: all ones, all zeros, mixed
    kind[:3] = torch.tensor([0, 1, 2])[:nq]
    mq = torch.randint(0, 2, (nq, 4), generator=gen).float()
    mq[kind == 0], mq[kind == 1] = 1.0, 0.0
    mixed = torch.nonzero(kind == 2).flatten()
    mq[mixed[:5], 1] = 0.5
    mask = mq.flatten()[:n].clone()
    if n % 4:
        mask[n - (n % 4):] = torch.tensor([0.0, 1.0, 0.5])[:n % 4]          # the scalar tail
    params = rnd(n, seed=331)
    ones = torch.nonzero(kind == 0).flatten()
    ones = ones[ones < n // 4]
    if len(ones):
        params[4 * int(ones[-1]) + 2] = float("nan")          # must come out with its bits (p * 1.0 keeps them too: the skip rule itself
                                                               # is checked by the element-wise equality, which a wrongly skipped quad fails)
    mask = mask.to(dev())
    before = params.clone()
    want = R.apply_masks_ref(before, mask)
    ops.apply_masks(params, mask)
    finite = torch.isfinite(before)
    assert torch.equal(params[finite], want[finite]) and int((~finite).sum()) == (1 if len(ones) else 0)
    keep = (mask.reshape(-1)[:4 * (n // 4)].reshape(-1, 4) == 1).all(1).repeat_interleave(4)
    assert torch.equal(params[:4 * (n // 4)][keep].view(torch.int32), before[:4 * (n // 4)][keep].view(torch.int32))
    if n >= 8:
        assert int((params != before).sum()) > n // 8
        from uvc_amd._lib import UvcHipError
        with pytest.raises(UvcHipError):
            ops.apply_masks(before[1:], mask[1:])
        with pytest.raises(UvcHipError):
            ops.apply_masks(before[4:], mask[1:n - 3])


# ============================================================================= column sums
#               M     N   ldx-N  row_weight  alpha_ptr     path (4-wide needs N % 4 == 0 and ldx % 4 == 0)
COLSUM_CASES = [(1, 1, 0, False, False),                 # scalar
                (3, 10, 0, True, False),                 # scalar
                (255, 12, 0, False, True),               # 4-wide
                (256, 260, 4, True, True),               # 4-wide, second column block
                (257, 1000, 0, True, False),             # 4-wide, ragged second row block, four column blocks
                (1029, 12, 4, False, False),             # 4-wide, ragged fifth row block, padded rows
                (1029, 260, 1, True, True),              # scalar (odd ldx), ragged rows, five column blocks
                (257, 1000, 1, False, True)]             # scalar, ragged rows, sixteen column blocks


@pytest.mark.parametrize("mode", ["f32", "bf16", "f32_under_bf16"])
@pytest.mark.parametrize("M,N,pad,with_rw,with_ptr", COLSUM_CASES)
def test_colsum(M, N, pad, with_rw, with_ptr, mode):
    from uvc_amd import ops
    ldx = N + pad
    parent = rnd(M, ldx, seed=341)
    parent[:, N:] = 1e6                                     # columns past N belong to someone else
    parent = parent.bfloat16() if mode == "bf16" else parent
    rw = rnd(M, seed=342) if with_rw else None
    aptr = torch.tensor([0.75], device=dev()) if with_ptr else None
    partial = nans(ops.colsum_blocks(M) * N)
    ref = R.colsum_ref(parent[:, :N], rw, 2.0 * (0.75 if with_ptr else 1.0))
    both_betas(lambda out, beta: ops.colsum(parent, partial, out, F32 if mode == "f32" else BF16, M=M, N=N, ldx=ldx, alpha=2.0,
                                            alpha_ptr=aptr, beta=beta, row_weight=rw), ref, rtol=1e-4, atol=1e-3)


# ============================================================================= token assembly
#                 dtype  token rows      dtok            dpe
ASSEMBLE_MODES = {"f32": (F32, torch.float32, torch.float32, torch.float32),
                  "bf16": (BF16, torch.bfloat16, torch.bfloat16, torch.bfloat16),
                  "bf16_f32_dpe": (BF16, torch.float32, torch.bfloat16, torch.float32),
                  "bf16_f32_dtok": (BF16, torch.bfloat16, torch.float32, torch.bfloat16)}


@pytest.mark.parametrize("mode", list(ASSEMBLE_MODES))
@pytest.mark.parametrize("B,P,D,ntok,masked", [(2, 196, 192, 1, False), (9, 16, 128, 2, True)])
def test_assemble_tokens_and_backward(B, P, D, ntok, masked, mode):
    from uvc_amd import ops
    dtype, t_tok, t_dtok, t_dpe = ASSEMBLE_MODES[mode]
    N = P + ntok
    pe, cls, pos = rnd(B, P, D, seed=351), rnd(D, seed=352), rnd(N, D, seed=354)
    dist = rnd(D, seed=353) if ntok == 2 else None
    mask = (rnd(B, P, seed=355) > 0).float() if masked else None
    mk = mask.unsqueeze(-1) if masked else 1.0
    tok = nans(B, N, D, dtype=t_tok)
    ops.assemble_tokens(pe, cls, dist, pos, mask, tok, B, P, D, ntok)
    heads = [cls.expand(B, 1, D)] + ([dist.expand(B, 1, D)] if ntok == 2 else [])
    reft = torch.cat(heads + [pe * mk], 1) + pos
    assert torch.equal(tok, reft.to(t_tok))
    dtok = rnd(B, N, D, seed=356).to(t_dtok)
    d64 = dtok.double().cpu()
    dmask = nans(B, P)
    dpe = nans(B, P, D, dtype=t_dpe)

    def run(dpos, dcls, ddist, beta):
        ops.assemble_tokens_bwd(dtok, pe, mask, dpe, dpos, dcls, ddist, dmask, B, P, D, ntok, dtype, beta_acc=beta)

    st = dict(rtol=1e-5, atol=1e-5)
    dpos, dcls, ddist = nans(N, D), nans(D), nans(D) if ntok == 2 else None
    run(dpos, dcls, ddist, 0.0)
    assert torch.equal(dpe, (dtok[:, ntok:].float() * mk).to(t_dpe))
    close64(dpos, d64.sum(0), **st)
    close64(dcls, d64[:, 0].sum(0), **st)
    close64(dmask, (d64[:, ntok:] * pe.double().cpu()).sum(-1), rtol=1e-4, atol=1e-4)
    if ntok == 2:
        close64(ddist, d64[:, 1].sum(0), **st)
    o_pos, o_cls, o_dist = rnd(N, D, seed=357), rnd(D, seed=358), rnd(D, seed=359)
    dpos, dcls, ddist = o_pos.clone(), o_cls.clone(), o_dist.clone() if ntok == 2 else None
    run(dpos, dcls, ddist, 1.0)
    close64(dpos, o_pos.double().cpu() + d64.sum(0), **st)
    close64(dcls, o_cls.double().cpu() + d64[:, 0].sum(0), **st)
    if ntok == 2:
        close64(ddist, o_dist.double().cpu() + d64[:, 1].sum(0), **st)


# ============================================================================= block gates
def gate_inputs(Lb, seed):
    """Logits and Exp(1) draws with |u0 - u1| >= 1e-3 in every block by construction: the second logit is placed at a chosen distance."""
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(Lb, 2, generator=gen)
    e = torch.empty(Lb, 2).exponential_(generator=gen).clamp_min(1e-3)
    gap = torch.exp(torch.empty(Lb).uniform_(math.log(1.2e-3), math.log(3.0), generator=gen)) * (torch.randint(0, 2, (Lb,), generator=gen) * 2 - 1)
    gap[:2] = torch.tensor([1.2e-3, -1.2e-3])[:Lb]
    g[:, 1] = (g[:, 0].double() + gap.double() / 2 + (e[:, 1].double().log() - e[:, 0].double().log())).float()
    u = R.gate_logits_ref(g, e)
    assert bool(((u[:, 0] - u[:, 1]).abs() >= 1e-3).all())
    return g.to(dev()), e.to(dev())


@pytest.mark.parametrize("Lb", [1, 12, 64])
def test_gate_distrib_hard_gumbel(Lb):
    from uvc_amd import ops
    g, e = gate_inputs(Lb, 360 + Lb)
    d = nans(Lb, 2)
    ops.gate_distrib(g, e, d, Lb, 3, 0.1)
    want = R.gate_distrib_ref(g, e, 3, 0.1)
    assert torch.equal(d.cpu().double(), want)
    assert bool(((d == 0) | (d == 1)).all()) and bool((d.sum(-1) == 1).all())
    if Lb >= 12:
        assert 0 < int(want[:, 1].sum()) < Lb
    d = nans(Lb, 2)
    ops.gate_distrib(g, e, d, Lb, 1, 0.1)
    close64(d, R.gate_distrib_ref(g, e, 1, 0.1), rtol=1e-5, atol=1e-6)


def test_gate_distrib_ties_and_block_limit():
    from uvc_amd import ops
    from uvc_amd._lib import UvcHipError
    g = torch.tensor([[0.3, 0.3], [-1.5, -1.5], [0.0, 0.0]], device=dev())
    e = torch.tensor([[0.7, 0.7], [2.0, 2.0], [1.0, 1.0]], device=dev())
    d = nans(3, 2)
    ops.gate_distrib(g, e, d, 3, 3, 0.1)
    assert d.tolist() == [[1.0, 0.0]] * 3
    g, e, d = rnd(65, 2, seed=371), torch.ones(65, 2, device=dev()), nans(65, 2)
    for mode in (0, 3):
        with pytest.raises(UvcHipError):
            ops.gate_distrib(g, e, d, 65, mode, 0.1)
    with pytest.raises(UvcHipError):
        ops.gate_grad(g, d, torch.zeros(66, 2, device=dev()), nans(65, 2), 65, 1, 0.1)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("Lb", [1, 12, 64])
def test_gate_grad(Lb, mode):
    """out = d1 * x2 + d0 * x per block; A = <gA, out>, B = <gA, x> arrive in the layout the LayerNorm backward leaves.  The warm-up
    and the hard gate pass no gradient to the logits."""
    from uvc_amd import ops
    eps = 0.1
    g, e = gate_inputs(Lb, 380 + Lb)
    if mode == 2:           # softL0 divides <gA, out> - <gA, x> by d1: g1 stays away from 0, where that float32 difference cancels
        gen = torch.Generator().manual_seed(390 + Lb)
        g[:, 1] = (torch.empty(Lb).uniform_(0.05, 2.0, generator=gen) * (torch.randint(0, 2, (Lb,), generator=gen) * 2 - 1)).to(dev())
    gd, ed = g.double().cpu().requires_grad_(True), e.double().cpu()
    if mode == 2:
        d1 = gd[:, 1] ** 2 / (gd[:, 1] ** 2 + eps)
        dd = torch.stack([1 - d1, d1], 1)
    else:
        dd = ((gd - ed.log()) / 0.5).softmax(-1)
    gx2, gx = rnd(Lb, seed=381).double().cpu(), rnd(Lb, seed=382).double().cpu()
    out = dd[:, 1] * gx2 + dd[:, 0] * gx
    out.sum().backward()
    want = gd.grad if mode in (1, 2) else torch.zeros(Lb, 2, dtype=torch.float64)
    dots = torch.zeros(Lb + 1, 2, dtype=torch.float64)
    dots[1:, 0] = out.detach()
    dots[:Lb, 1] = gx
    dots = dots.float().to(dev())
    d = nans(Lb, 2)
    ops.gate_distrib(g, e, d, Lb, mode, eps)
    both_betas(lambda dg, beta: ops.gate_grad(g, d, dots, dg, Lb, mode, eps, beta), want, rtol=1e-3, atol=1e-5)
    if mode in (0, 3):
        dg = nans(Lb, 2)
        ops.gate_grad(g, d, dots, dg, Lb, mode, eps, 0.0)
        assert not dg.any()
        old = rnd(Lb, 2, seed=383)
        dg = old.clone()
        ops.gate_grad(g, d, dots, dg, Lb, mode, eps, 1.0)
        assert torch.equal(dg, old)


# ============================================================================= MLP compaction
MLP_SHAPES = [(64, 256, 8), (192, 768, 256), (100, 40, 40)]


def kept_units(F_, width):
    return torch.randperm(F_, generator=torch.Generator().manual_seed(F_ + width))[:width].to(torch.int32)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("D,F_,width", MLP_SHAPES)
def test_mlp_gather_shadows(D, F_, width, dtype):
    from uvc_amd import ops
    T = ops.tdtype(dtype)
    W1, b1, W2 = rnd(F_, D, seed=401), rnd(F_, seed=402), rnd(D, F_, seed=403)
    idx = kept_units(F_, width)
    w1c, w1t, w2c, w2t = nans(width, D, dtype=T), nans(D, width, dtype=T), nans(D, width, dtype=T), nans(width, D, dtype=T)
    b1c = nans(width)
    ops.mlp_gather_shadows(W1, b1, W2, idx.to(dev()), w1c, w1t, w2c, w2t, b1c, D, F_, width, dtype)
    il = idx.long().to(dev())
    assert torch.equal(w1c, W1[il].to(T)) and torch.equal(w1t, W1[il].to(T).t().contiguous())
    assert torch.equal(w2c, W2[:, il].to(T).contiguous()) and torch.equal(w2t, W2[:, il].to(T).t().contiguous())
    assert torch.equal(b1c, b1[il])


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("D,F_,width", MLP_SHAPES)
def test_mlp_scatter_grads(D, F_, width, dtype):
    """Kept units: a copy of the compact gradients.  Pruned units: zero fc1 rows and biases, and the fc2 column GELU(b1[j]) * db2 that
    autograd gives the dense masked MLP (tests/test_small_kernel_refs_cpu.py) -- float32: x/2 * erfcf(-x / sqrt 2) and one product; bf16 mode: the
    forward's approximant (7.6e-4 max(|GELU|, 2e-3), test_bf16_mode_gelu_approximant_error_bounds) and the 2^-8 of the stored bf16."""
    from uvc_amd import ops
    rows = 37
    x, dy = rnd(rows, D, seed=411), rnd(rows, D, seed=412)
    W1, W2, b2 = rnd(F_, D, seed=413, scale=D ** -0.5), rnd(D, F_, seed=414, scale=F_ ** -0.5), rnd(D, seed=416)
    b1 = rnd(F_, seed=415, scale=0.5)
    idx = kept_units(F_, width)
    inv = torch.full((F_,), -1, dtype=torch.int32)
    inv[idx.long()] = torch.arange(width, dtype=torch.int32)
    pruned = inv < 0
    # -4 and -5: where 1 + erff(x / sqrt 2) has cancelled to a few float32 ulps, and the erfc form keeps its relative accuracy
    b1[torch.nonzero(pruned).flatten()[:8]] = torch.tensor([0.0, 0.05, -0.05, 3.0, -3.0, -9.0, -4.0, -5.0], device=dev())[:int(pruned.sum())]
    ref = R.mlp_scatter_ref(x, W1, b1, W2, b2, idx, dy)
    dw1c, db1c, dw2c, db2 = (ref[k].float().contiguous().to(dev()) for k in ("dw1c", "db1c", "dw2c", "db2"))
    invd, il = inv.to(dev()), idx.long().to(dev())

    def run(dW1, dW2, db1, beta):
        ops.mlp_scatter_grads(dw1c, dw2c, db1c, invd, b1, db2, dW1, dW2, db1, D, F_, width, dtype, beta_acc=beta)

    dW1, dW2, db1 = nans(F_, D), nans(D, F_), nans(F_)
    run(dW1, dW2, db1, 0.0)
    assert torch.isfinite(dW1).all() and torch.isfinite(dW2).all() and torch.isfinite(db1).all()
    assert torch.equal(dW1[il], dw1c) and torch.equal(db1[il], db1c) and torch.equal(dW2[:, il], dw2c)
    pd = pruned.to(dev())
    assert not dW1[pd].any() and not db1[pd].any()
    gelu = F.gelu(b1.double().cpu())[pruned]
    want = gelu[None, :] * ref["db2"][:, None]
    got = dW2[:, pd].double().cpu()
    if dtype == F32:
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-7)
    else:
        bound = (7.6e-4 * gelu.abs().clamp_min(2e-3) + 2.0 ** -8 * gelu.abs())[None, :] * ref["db2"].abs()[:, None]
        assert bool(((got - want).abs() <= bound).all()), float(((got - want).abs() / bound.clamp_min(1e-300)).max())
    o1, o2, o3 = rnd(F_, D, seed=417), rnd(D, F_, seed=418), rnd(F_, seed=419)
    a1, a2, a3 = o1.clone(), o2.clone(), o3.clone()
    run(a1, a2, a3, 1.0)
    at = dict(rtol=1e-6, atol=1e-6)
    close64(a1, o1.double() + dW1.double(), **at)
    close64(a2, o2.double() + dW2.double(), **at)
    close64(a3, o3.double() + db1.double(), **at)
