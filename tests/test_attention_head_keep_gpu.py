"""GPU: uvc_attn_args.head_keep / uvc_attn_tok_args.head_keep, the [H] table of pruned heads, in every attention kernel family of attention.hip and
token_tail.hip.  Every expected value is exact, so nothing here has a tolerance: every assertion is torch.equal or == 0.

  * a kept head depends on no other head: with the table its o, lse, dq, dk, dv and delta carry the bits of the call without the table;
  * a dead head's o (forward) and dq, dk, dv (backward) are exact zeros on all N rows and all 64 columns, whatever dout holds;
  * lse (forward) and delta (backward) of a dead head are NOT WRITTEN, in any family: the caller's bytes survive (pinned per family below, stated at
    include/uvc_kernels.h: uvc_attn_args.head_keep);
  * with dout zero on the dead heads' 64 columns -- the state Stage 2 guarantees -- the complete dqkv equals the complete dqkv of the call without
    the table: what "exact" means in the header's comment;
  * the kernels test == 0, so 1, 7 and -1 all keep a head, and a table without a zero reproduces the null-pointer call bit for bit, everywhere.

Every output (o, lse, dqkv, delta) is a view into a parent filled with a finite sentinel, GUARD elements on both sides, and WHOLE PARENTS are
compared: a stray write shows as well as a missing one.  Inputs: attention_refs.make_case, random and routing families.

Which dead-head situation each family's cases reach (asserted from the bh arithmetic where the launch fixes it):
  short forward + dq, dk/dv pair   one head per workgroup: the dead-head branch is the workgroup's only head -- every position of the table, all dead, H = 1
  persistent forward (> 512 heads) 512 workgroups walk bh, bh + 512, ...: a dead first head followed by a live one (the live head's prefetched K / V are
                                   stored behind the dead head's zeros), a dead prefetched next head, a dead last head, two dead heads in a row
  one-pass backward (variant 2)    grid 1: one workgroup walks the 15 heads in order -- first head dead, runs of two dead heads, dead -> live and
                                   live -> dead hand-overs, last head dead, every head dead; grids 2 and 4: dynamic draws; grid 0: the first-head branch
                                   alone; one launch repeated: equal bits
  selection by shape (variant 0)   1026 heads, N = 197: the one-pass kernel (its bits, not the pair's) on 224 persistent workgroups, dynamic draws
  streaming (N > 256)              one (head, block of 128 rows) per workgroup: every block of a dead head, the ragged last block (257, 321, 577)
  token-query, ntok 1 and 2        one head per workgroup, forward and backward (ops.attention_tok_bwd takes the table since this module)

Measured on an MI355X: 145 cases, 10 s wall in all (the slowest, the routing case of 1029 heads, 1.5 s; the 1026-head selection cases 0.5 s each; every
other case under 0.4 s but the first one-pass case, which loads the library).  The tests can fail: with k_attn_fwd reading head_keep[(h + 1) % H] 48 cases fail
(short at H = 3, persistent), with the one-pass store_out never zeroing 16 (one-pass at H = 3 and 2, selection), with the dead-head store loop of k_attn_fwd bounded
by N * 8 all 84 short and persistent cases (the lower half of a dead head's rows keeps the sentinel).
"""
import functools

import pytest
import torch

import attention_refs as A

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
SENT = -7.0                                         # finite, exact in bf16, and no zero
GUARD = 64                                          # elements of sentinel on either side of an output (a multiple of 8: 16-byte alignment in bf16)
KEPT = (1, 7, -1)                                   # the kernels test == 0: every other value keeps the head
FAMILIES = [A.RANDOM, A.ROUTING]
T3 = [(1, 0, 1), (0, 1, 1), (1, 1, 0), (0, 0, 0)]
ALL8 = [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]


def dev():
    return torch.device("cuda")


def tt(dtype):
    return torch.float32 if dtype == F32 else torch.bfloat16


@functools.lru_cache(maxsize=2)
def case(family, B, N, H, ntok=None, backward=True, seed=None):
    """Inputs on the device (make_case also computes their float64 reference, which nothing here needs: every expected value is a kernel's own
    result without the table); shared by the precisions of a case, never modified.  ``backward=False``: the forward-only cases.
    ``seed`` (default B + H, as tests/test_attention_accuracy_gpu.py draws): make_case accepts a routing draw only if its float64 reference is exact in
    every row, which fails where an element of v (or of dout) is drawn as exactly 0.0 -- one or two of the 13 million of a 1026-head case, in each of
    the four draws make_case tries from seed 345, so it raises; the draw of seed 347 has none."""
    return A.make_case(family, B, N, H, 64, ntok, seed=B + H if seed is None else seed, device=dev(), backward=backward)


def table(bits):
    """The int32 device table of ``bits`` (0 = dead), the kept heads marked 1, 7, -1 in turn."""
    return torch.tensor([0 if not b else KEPT[i % 3] for i, b in enumerate(bits)], device=dev(), dtype=torch.int32)


def dead_of(bits):
    return [h for h, b in enumerate(bits) if not b]


def parent(shape, T):
    """(parent, view of ``shape`` at GUARD) on the device, the parent full of the sentinel."""
    n = 1
    for s in shape:
        n *= s
    p = torch.full((GUARD + n + GUARD,), SENT, device=dev(), dtype=T)
    return p, p[GUARD:GUARD + n].view(shape)


def inner(p, shape):
    return p[GUARD:p.numel() - GUARD].view(shape)


def guards_intact(p):
    return bool((p[:GUARD] == SENT).all()) and bool((p[-GUARD:] == SENT).all())


def where(got, want, shape, what):
    """The message of a failed whole-parent comparison: how many elements differ and where the first one lies."""
    bad = (got != want).flatten().nonzero().flatten()
    i = int(bad[0]) - GUARD
    n = 1
    for s in shape:
        n *= s
    if i < 0 or i >= n:
        at = f"guard element {i if i < 0 else i - n} {'before' if i < 0 else 'behind'} the output"
    else:
        idx = []
        for s in reversed(shape):
            idx.append(i % s)
            i //= s
        at = f"index {tuple(reversed(idx))} of {tuple(shape)}"
    j = int(bad[0])
    return f"{what}: {bad.numel()} elements differ, the first at {at}: got {float(got[j])}, expected {float(want[j])}"


def with_heads(p, shape, head_dim, dead, value):
    """A copy of parent ``p`` whose view of ``shape`` holds ``value`` on the heads ``dead`` of dimension ``head_dim``: the parent a correct call with
    the table leaves, made from the parent the call without it left."""
    e = p.clone()
    if dead:
        inner(e, shape).index_fill_(head_dim, torch.tensor(dead, device=e.device), value)
    return e


def zero_dead_columns(dout, H, dead):
    """dout [B, Nq, H*64] with the 64 columns of every dead head zeroed: what a masked attn.proj hands the attention backward."""
    d = dout.clone()
    if dead:
        d.view(d.shape[0], d.shape[1], H, 64)[:, :, dead] = 0
    return d


# ----------------------------------------------------------------------------- uvc_attention_fwd / uvc_attention_bwd
def forward(c, dtype, keep=None):
    """-> (o parent, lse parent), synchronised."""
    from uvc_amd import ops
    B, N, H = c["B"], c["N"], c["H"]
    po, o = parent((B, N, H * 64), tt(dtype))
    pl, lse = parent((B, H, N), torch.float32)
    ops.attention_fwd(c["qkv"].to(tt(dtype)), o, lse, B, N, H, dtype, head_keep=keep)
    torch.cuda.synchronize()
    return po, pl


def backward(c, dtype, po, pl, dout, keep=None, variant=0, grid=0):
    """-> (dqkv parent, delta parent), synchronised; o and lse are the views of the forward's parents."""
    from uvc_amd import ops
    B, N, H = c["B"], c["N"], c["H"]
    pd, dqkv = parent((B, N, 3 * H * 64), tt(dtype))
    pe, delta = parent((B, H, N), torch.float32)
    ops.attention_bwd(c["qkv"].to(tt(dtype)), inner(po, (B, N, H * 64)), inner(pl, (B, H, N)), dout, dqkv, delta, B, N, H, dtype,
                      head_keep=keep, variant=variant, grid=grid)
    torch.cuda.synchronize()
    return pd, pe


def check_forward(c, dtype, tables, tag):
    """The forward with each table against the forward without one.  Returns the parents of the run without a table."""
    B, N, H = c["B"], c["N"], c["H"]
    so, sl = (B, N, H, 64), (B, H, N)
    po, pl = forward(c, dtype)
    assert guards_intact(po) and guards_intact(pl), f"{tag}: the forward without a table wrote outside its outputs"
    assert not bool((inner(pl, sl) == SENT).any()), f"{tag}: the forward without a table left lse elements unwritten"
    for bits in tables:
        dead = dead_of(bits)
        go, gl = forward(c, dtype, table(bits))
        eo = with_heads(po, so, 2, dead, 0.0)              # kept heads: the bits without the table; dead heads: zeros
        el = with_heads(pl, sl, 1, dead, SENT)             # lse of a dead head is not written
        assert torch.equal(go, eo), where(go, eo, so, f"{tag} table {bits}: o")
        assert torch.equal(gl, el), where(gl, el, sl, f"{tag} table {bits}: lse")
        if dead:
            assert float(inner(go, so)[:, :, dead].float().abs().max()) == 0, f"{tag} table {bits}: o of a dead head"
    return po, pl


def check_backward(c, dtype, po, pl, tables, tag, variant=0, grids=(0,), base_grid=0):
    """The backward with each table against the backward without one, on a random dout and on dout zeroed on the dead heads' columns."""
    B, N, H = c["B"], c["N"], c["H"]
    sd, se = (B, N, 3, H, 64), (B, H, N)
    dout = c["dout"].to(tt(dtype))
    pd, pe = backward(c, dtype, po, pl, dout, None, variant, base_grid)
    assert guards_intact(pd) and guards_intact(pe), f"{tag}: the backward without a table wrote outside its outputs"
    assert not bool((inner(pe, se) == SENT).any()), f"{tag}: the backward without a table left delta elements unwritten"
    for bits in tables:
        dead = dead_of(bits)
        dz = zero_dead_columns(dout, H, dead)
        zd, ze = backward(c, dtype, po, pl, dz, None, variant, base_grid) if dead else (pd, pe)
        if dead:                                            # the unskipped computation of a head without dout: zeros, and a delta of zero
            assert float(inner(zd, sd)[:, :, :, dead].float().abs().max()) == 0, f"{tag} table {bits}: the unskipped dq / dk / dv of a head with dout = 0"
        for grid in grids:
            t = f"{tag} grid {grid} table {bits}"
            # random dout: zeros on the dead heads whatever dout holds, the kept heads' bits, delta of a dead head not written
            gd, ge = backward(c, dtype, po, pl, dout, table(bits), variant, grid)
            ed, ee = with_heads(pd, sd, 3, dead, 0.0), with_heads(pe, se, 1, dead, SENT)
            assert torch.equal(gd, ed), where(gd, ed, sd, f"{t}, random dout: dqkv")
            assert torch.equal(ge, ee), where(ge, ee, se, f"{t}, random dout: delta")
            if dead:
                assert float(inner(gd, sd)[:, :, :, dead].float().abs().max()) == 0, f"{t}: dq / dk / dv of a dead head"
                # Stage 2's state: the COMPLETE dqkv is the one of the call without the table
                gd, ge = backward(c, dtype, po, pl, dz, table(bits), variant, grid)
                ee = with_heads(ze, se, 1, dead, SENT)
                assert torch.equal(gd, zd), where(gd, zd, sd, f"{t}, dout zero on the dead heads: dqkv")
                assert torch.equal(ge, ee), where(ge, ee, se, f"{t}, dout zero on the dead heads: delta")
    return pd, pe


# ----------------------------------------------------------------------------- N <= 256: k_attn_fwd, k_attn_bwd_dq, k_attn_bwd_dkv
SHORT_N = [1, 17, 64, 65, 129, 197, 207, 208, 256]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("H", [3, 1])
@pytest.mark.parametrize("N", SHORT_N)
def test_short_forward_and_pair_backward(N, H, family, dtype):
    """Every NT16 instantiation (2, 4, 8, 14, 16 key tiles), both sides of the NFULL = 12 specialisation (197, 207 | 208), padding (17, 65, 129) and
    none (64, 208, 256); 6 heads, so one head per workgroup in both precisions.  H = 1: the table is [0], every workgroup is dead."""
    c = case(family, 2, N, H)
    tables = T3 + [(1, 1, 1)] if H == 3 else [(0,), (1,)]
    tag = f"short {A.FAMILY_NAMES[family]} N={N} H={H} {'f32' if dtype == F32 else 'bf16'}"
    po, pl = check_forward(c, dtype, tables, tag)
    check_backward(c, dtype, po, pl, tables, tag + " pair", variant=1)


# ----------------------------------------------------------------------------- bf16, more than 512 heads: k_attn_fwd's persistent loop
PERSISTENT_TABLES = {3: [(0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 1)], 6: [(0, 1, 0, 1, 1, 0)]}


def persistent_walks(nbh, H, bits, grid=512):
    """What the workgroups that walk more than one head meet (launch(): 512 workgroups, bh = blockIdx.x, + 512, ...; pf_load(bh + 512) is issued before
    head bh is computed or zeroed, pf_store() behind it)."""
    seen = set()
    for w in range(min(grid, nbh)):
        ks = [bits[bh % H] for bh in range(w, nbh, grid)]
        if len(ks) < 2:
            continue
        if not ks[0] and ks[1]:
            seen.add("first head dead, then a live one")
        if any(not k for k in ks[1:]):
            seen.add("prefetched next head dead")
        if not ks[-1]:
            seen.add("last head dead")
        if any(not a and not b for a, b in zip(ks, ks[1:])):
            seen.add("two dead heads in a row")
        if any(a and not b for a, b in zip(ks, ks[1:])):
            seen.add("live head, then a dead one")
    return seen


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("B,H", [(172, 3), (343, 3), (87, 6)])
@pytest.mark.parametrize("N", [17, 197])
def test_persistent_forward(N, B, H, family):
    """516, 1029 and 522 heads on 512 workgroups.  The stride 512 is 2 mod 3 and 2 mod 6, so a workgroup's successive heads have different h: a table
    indexed by anything but bh % H, or zeros / prefetched K / V rows stored for the wrong head, changes a kept head's bits or a dead head's zeros."""
    nbh = B * H
    assert nbh > 512 and 512 % H == 2
    tables = PERSISTENT_TABLES[H]
    seen = set()
    for bits in tables:
        s = persistent_walks(nbh, H, bits)
        # every table meets the three situations by itself
        assert {"first head dead, then a live one", "prefetched next head dead", "last head dead"} <= s, (bits, s)
        seen |= s
    # (516 heads: four workgroups walk two heads, h = (0, 2), (1, 0), (2, 1), (0, 2); [0, 0, 1] gives workgroup 1 two dead heads)
    assert "live head, then a dead one" in seen and "two dead heads in a row" in seen
    c = case(family, B, N, H, backward=False)
    check_forward(c, BF16, tables + [(1,) * H], f"persistent-fwd {A.FAMILY_NAMES[family]} N={N} B={B} H={H}")


# ----------------------------------------------------------------------------- bf16, 193 <= N <= 200: one::k_attn_bwd_one
def one_pass_walk(nbh, H, bits):
    """grid = 1: the single workgroup starts on head 0 and draws 1, 2, ... from the counter -- the heads in order."""
    ks = [bits[bh % H] for bh in range(nbh)]
    seen = set()
    if not ks[0]:
        seen.add("first head dead")
    if not ks[-1]:
        seen.add("last head dead")
    if not any(ks):
        seen.add("every head dead")
    for a, b in zip(ks, ks[1:]):
        seen.add({(0, 0): "two dead heads in a row", (0, 1): "dead head, then a live one", (1, 0): "live head, then a dead one", (1, 1): "two live heads"}[(int(bool(a)), int(bool(b)))])
    if any(not a and not b and c for a, b, c in zip(ks, ks[1:], ks[2:])):
        seen.add("a live head behind two dead ones")         # neither image buffer was filled in the iteration before its fill
    return seen


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("H", [3, 2, 1])
@pytest.mark.parametrize("N", [193, 197, 200])
def test_one_pass_backward(N, H, family):
    """variant 2 on 15 (10, 5) heads.  grid 1: one workgroup walks them in order; 2 and 4: dynamic draws, so which workgroup meets which run of dead and
    live heads differs from launch to launch; 0: one head per workgroup.  The call without a table runs at grid 0."""
    B = 5
    tables = {3: ALL8, 2: [(0, 1), (1, 0)], 1: [(0,), (1,)]}[H]
    if H == 3:
        seen = set()
        for bits in tables:
            seen |= one_pass_walk(B * H, H, bits)
        assert {"first head dead", "last head dead", "every head dead", "two dead heads in a row", "dead head, then a live one",
                "live head, then a dead one", "a live head behind two dead ones"} <= seen, seen
        assert "first head dead" in one_pass_walk(B * H, H, (0, 1, 1)) and "last head dead" in one_pass_walk(B * H, H, (1, 1, 0))
        assert "two dead heads in a row" in one_pass_walk(B * H, H, (0, 0, 1)) and "two dead heads in a row" in one_pass_walk(B * H, H, (0, 1, 0))
    c = case(family, B, N, H)
    tag = f"one-pass {A.FAMILY_NAMES[family]} N={N} H={H}"
    po, pl = forward(c, BF16)
    check_backward(c, BF16, po, pl, tables, tag, variant=2, grids=(1, 2, 4, 0))


@pytest.mark.parametrize("N", [193, 197, 200])
def test_one_pass_backward_repeats_bit_for_bit(N):
    """One (N, table, grid) launch five times: the draws differ, the bits may not."""
    c = case(A.RANDOM, 5, N, 3)
    po, pl = forward(c, BF16)
    dout = c["dout"].to(torch.bfloat16)
    keep = table((0, 1, 0))
    first = backward(c, BF16, po, pl, dout, keep, 2, 2)
    for rep in range(4):
        again = backward(c, BF16, po, pl, dout, keep, 2, 2)
        assert torch.equal(again[0], first[0]), where(again[0], first[0], (5, N, 3, 3, 64), f"one-pass N={N} repeat {rep + 1}: dqkv")
        assert torch.equal(again[1], first[1]), where(again[1], first[1], (5, 3, N), f"one-pass N={N} repeat {rep + 1}: delta")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("bits", [(1, 0, 1), (0, 0, 1)])
def test_selection_by_shape_runs_the_one_pass_kernel(bits, family):
    """variant 0 at bf16, N = 197, 1026 heads (>= 1024), grid 0: the persistent one-pass kernel, every workgroup drawing several heads.  Its result with the
    table is held to variant 2's without it; that the rule chose the one-pass kernel shows in the bits: they are variant 2's and not the pair's."""
    B, N, H = 342, 197, 3
    assert B * H >= 1024
    c = case(family, B, N, H, seed=347)
    sd, se = (B, N, 3, H, 64), (B, H, N)
    dead = dead_of(bits)
    tag = f"selection {A.FAMILY_NAMES[family]} table {bits}"
    dout = c["dout"].to(torch.bfloat16)
    po, pl = forward(c, BF16)
    pd, pe = backward(c, BF16, po, pl, dout, None, 2, 0)
    assert guards_intact(pd) and guards_intact(pe) and not bool((inner(pe, se) == SENT).any())
    g0 = backward(c, BF16, po, pl, dout, table(bits), 0, 0)
    g2 = backward(c, BF16, po, pl, dout, table(bits), 2, 0)
    g1 = backward(c, BF16, po, pl, dout, table(bits), 1, 0)
    ed, ee = with_heads(pd, sd, 3, dead, 0.0), with_heads(pe, se, 1, dead, SENT)
    assert torch.equal(g0[0], ed), where(g0[0], ed, sd, f"{tag}, variant 0: dqkv")
    assert torch.equal(g0[1], ee), where(g0[1], ee, se, f"{tag}, variant 0: delta")
    assert float(inner(g0[0], sd)[:, :, :, dead].float().abs().max()) == 0
    assert torch.equal(g0[0], g2[0]) and torch.equal(g0[1], g2[1]), f"{tag}: variant 0 and variant 2 differ"
    assert not torch.equal(g0[0], g1[0]), f"{tag}: variant 0 gave the pair's bits"
    # the pair at this size, for the same table: its own kept bits, zeros, and an untouched delta
    p1 = backward(c, BF16, po, pl, dout, None, 1, 0)
    e1 = with_heads(p1[0], sd, 3, dead, 0.0)
    assert torch.equal(g1[0], e1), where(g1[0], e1, sd, f"{tag}, variant 1: dqkv")
    # Stage 2's state
    dz = zero_dead_columns(dout, H, dead)
    zd, ze = backward(c, BF16, po, pl, dz, None, 2, 0)
    gd, ge = backward(c, BF16, po, pl, dz, table(bits), 0, 0)
    ee = with_heads(ze, se, 1, dead, SENT)
    assert torch.equal(gd, zd), where(gd, zd, sd, f"{tag}, dout zero on the dead heads: dqkv")
    assert torch.equal(ge, ee), where(ge, ee, se, f"{tag}, dout zero on the dead heads: delta")


# ----------------------------------------------------------------------------- 256 < N <= 1026: the streaming kernels
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("N", [257, 321, 577])
def test_streaming_forward_and_backward(N, family, dtype):
    """3, 3 and 5 blocks of LQ = 128 rows per head, the last one ragged (1, 65 and 65 rows): zero_rows64 over [r0, min(N, r0 + 128))."""
    c = case(family, 1, N, 3)
    tables = [(1, 0, 1), (0, 1, 1), (0, 0, 0), (1, 1, 1)]
    tag = f"streaming {A.FAMILY_NAMES[family]} N={N} {'f32' if dtype == F32 else 'bf16'}"
    po, pl = check_forward(c, dtype, tables, tag)
    check_backward(c, dtype, po, pl, tables, tag)


# ----------------------------------------------------------------------------- token-query kernels (token_tail.hip)
def token_run(c, dtype, dout, keep=None):
    """-> (o parent, dqkv parent) of uvc_attention_tok_fwd and uvc_attention_tok_bwd, synchronised.  The backward reads q, k, v and dout only."""
    from uvc_amd import ops
    B, N, H, ntok = c["B"], c["N"], c["H"], c["ntok"]
    po, o = parent((B, ntok, H * 64), tt(dtype))
    pd, dqkv = parent((B, N, 3 * H * 64), tt(dtype))
    qkv = c["qkv"].to(tt(dtype))
    ops.attention_tok_fwd(qkv, o, B, N, H, ntok, dtype, head_keep=keep)
    ops.attention_tok_bwd(qkv, o, dout, dqkv, B, N, H, ntok, dtype, head_keep=keep)
    torch.cuda.synchronize()
    return po, pd


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("N", [5, 197, 256])
@pytest.mark.parametrize("ntok", [1, 2])
def test_token_query_forward_and_backward(ntok, N, family, dtype):
    """k_attn_tok_fwd zeroes the ntok rows of a dead head's o, k_attn_tok_bwd all N rows of its dq, dk, dv; there is no lse or delta."""
    B, H = 2, 3
    c = case(family, B, N, H, ntok)
    so, sd = (B, ntok, H, 64), (B, N, 3, H, 64)
    dout = c["dout"].to(tt(dtype))
    tag = f"token ntok={ntok} {A.FAMILY_NAMES[family]} N={N} {'f32' if dtype == F32 else 'bf16'}"
    po, pd = token_run(c, dtype, dout)
    assert guards_intact(po) and guards_intact(pd), f"{tag}: the call without a table wrote outside its outputs"
    for bits in T3 + [(1, 1, 1)]:
        dead = dead_of(bits)
        kept = [h for h in range(H) if h not in dead]
        go, gd = token_run(c, dtype, dout, table(bits))
        eo, ed = with_heads(po, so, 2, dead, 0.0), with_heads(pd, sd, 3, dead, 0.0)
        assert torch.equal(go, eo), where(go, eo, so, f"{tag} table {bits}: o")
        assert torch.equal(gd, ed), where(gd, ed, sd, f"{tag} table {bits}, random dout: dqkv")
        if dead:
            assert float(inner(go, so)[:, :, dead].float().abs().max()) == 0
            assert float(inner(gd, sd)[:, :, :, dead].float().abs().max()) == 0
            dz = zero_dead_columns(dout, H, dead)
            _, zd = token_run(c, dtype, dz)
            _, gz = token_run(c, dtype, dz, table(bits))
            assert torch.equal(gz, zd), where(gz, zd, sd, f"{tag} table {bits}, dout zero on the dead heads: dqkv")
        if kept:                                            # dq rows past ntok are zero for kept heads too
            assert float(inner(gd, sd)[:, ntok:, 0][:, :, kept].float().abs().sum()) == 0
