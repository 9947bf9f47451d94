"""GPU: the conformal kernels (uvc_amd/csrc/conformal.hip) -- ``ops.conformal_scores`` and ``ops.conformal_sets`` against the float64 spec
(tests/conformal_ref.py) on the same float32 inputs, bit-repeatability, the refusals, and ``fit`` + ``score`` end to end against the CPU
evaluator.

Scores: |s - s_ref| <= 1e-5 max(1, |s_ref|), the bar this project holds softmax read-outs to.  Sets: membership equals the reference at every
(row, class) pair with |s_ref(c) - qhat| > 1e-5 (a decided pair); the undecided pairs must stay under 1 % of all -- a test that exceeds the cap
has a wrong input, not a loose kernel.  The cap holds for every input of N(0, 3) or large logits on its own and for every test as a whole; rows of
equal logits hit the thresholds exactly by construction (1 - 1 / C is 0.5, 0.9, 0.999 at C = 2, 10, 1000) and count in the test's share only."""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

import conformal_ref as CR
import knn_ref as KR
from uvc_amd import _lib as L
from uvc_amd import compact_calibrate as CC
from uvc_amd import compact_conformal as CF
from uvc_amd import ops

pytestmark = pytest.mark.gpu

NAN = float("nan")
BAR = 1e-5
CAP = 0.01
ROWS = (1, 63, 64, 65, 1000, 4097)
SHAPES = [(1, 8), (2, 8), (10, 16), (100, 104), (1000, 1000), (1003, 1008), (100, 102), (2048, 2048), (2500, 2501)]
QHATS = (0.5, 0.9, 0.97, 0.999, math.inf)
LAM, K_REG = 0.01, 5
WORST = {}


def make_logits(kind, n, Cc, ld, seed):
    """float32 [n, ld] on the host, NaN in the padding columns"""
    g = torch.Generator().manual_seed(seed)
    z = torch.full((n, ld), NAN)
    if kind == "normal":
        z[:, :Cc] = 3.0 * torch.randn(n, Cc, generator=g)
    elif kind == "large":
        z[:, :Cc] = 3e4 * torch.randn(n, Cc, generator=g)
        z[::2, :Cc] = 3e4 + 3.0 * torch.randn((n + 1) // 2, Cc, generator=g)          # every other row: near 3e4, a few float32 steps apart
    else:
        z[:, :Cc] = torch.randn(n, 1, generator=g).expand(n, Cc)
    return z


def make_labels(n, Cc, seed, dtype):
    g = torch.Generator().manual_seed(seed + 1)
    y = torch.randint(0, Cc, (n,), generator=g)
    if n >= 3:
        y[n // 3], y[n // 2] = -1, Cc
    return y.to(dtype)


def on_device(z, off_by_one=False):
    """the rows on the device with their stride; ``off_by_one``: the base one element past a 16-byte boundary"""
    n, ld = z.shape
    if not off_by_one:
        return z.cuda()
    flat = torch.empty(n * ld + 1, device="cuda")
    v = flat[1:].view(n, ld)
    v.copy_(z)
    assert v.data_ptr() % 16 == 4
    return v


class Ref:
    """softmax, order and the mass ahead of one input, once; the three methods' scores from them"""

    def __init__(self, z, Cc, u, T):
        self.n, self.C = z.shape[0], Cc
        self.s = CR.all_class_scores(z.numpy(), Cc, None if u is None else u.numpy(), T, LAM, K_REG)

    def label(self, method, y):
        y = y.numpy().astype(np.int64)
        keep = (y >= 0) & (y < self.C)
        out = np.full(self.n, np.nan)
        out[keep] = self.s[method][keep, y[keep]]
        return out, int(keep.sum())


def run_scores(zd, yd, Cc, method, ud, T):
    n = zd.shape[0]
    sb = torch.full((n + 2,), -7.0, device="cuda")
    cb = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    s, counts = ops.conformal_scores(zd, yd, Cc, method, ud, temperature=T, lam=LAM, k_reg=K_REG, scores=sb[1:n + 1], counts=cb[1:2])
    assert sb[[0, -1]].tolist() == [-7.0, -7.0] and cb[[0, 2]].tolist() == [-7, -7]
    return s, counts


def run_sets(zd, qhat, yd, Cc, method, ud, T, members=True):
    n, W = zd.shape[0], (Cc + 31) // 32
    zb = torch.full((n + 2,), -7, dtype=torch.int32, device="cuda")
    vb = torch.full((n + 2,), 77, dtype=torch.uint8, device="cuda")
    mb = torch.full(((n + 2) * W,), -7, dtype=torch.int32, device="cuda")
    size, covered, mem = ops.conformal_sets(zd, qhat, yd, Cc, method, ud, temperature=T, lam=LAM, k_reg=K_REG, size=zb[1:n + 1],
                                            covered=vb[1:n + 1] if yd is not None else None, members=mb[W:(n + 1) * W].view(n, W) if members else False)
    assert zb[[0, -1]].tolist() == [-7, -7] and vb[[0, -1]].tolist() == [77, 77] and mb[:W].tolist() == [-7] * W and mb[-W:].tolist() == [-7] * W
    if not members:
        assert mb.eq(-7).all()
    return size, covered, mem


def unpack_dev(mem, Cc):
    bits = (mem.to(torch.int64)[:, :, None] >> torch.arange(32, device="cuda")) & 1
    return bits.reshape(mem.shape[0], -1)


def check_scores(ref, zd, y, Cc, ud, T, tag):
    yd = y.cuda()
    for method in CR.METHODS:
        want, m = ref.label(method, y)
        s, counts = run_scores(zd, yd, Cc, method, ud, T)
        got = s.double().cpu().numpy()
        assert int(counts[0]) == m, (tag, method, int(counts[0]), m)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (tag, method)
        keep = ~np.isnan(want)
        if keep.any():
            err = float(np.max(np.abs(got[keep] - want[keep]) / np.maximum(1.0, np.abs(want[keep]))))
            WORST["scores"] = max(WORST.get("scores", 0.0), err)
            print(tag, method, "scores err", err)
            assert err <= BAR, (tag, method, err)


def check_sets(ref, zd, y, Cc, ud, T, tag, tally, cap_each=True):
    """``tally``: [undecided pairs, pairs] of the test, summed over its inputs, methods and thresholds; ``cap_each``: this input alone must
    keep to the cap as well (rows of equal logits cannot: 1 - 1 / C IS 0.5, 0.9 or 0.999 at C = 2, 10, 1000, and (c + 1) / C meets them too)"""
    yd = y.cuda()
    yl = y.to(torch.int64).cuda()
    keep = (yl >= 0) & (yl < Cc)
    W = (Cc + 31) // 32
    for method in CR.METHODS:
        sref = torch.from_numpy(ref.s[method]).cuda()
        for qhat in QHATS:
            want = torch.ones_like(sref, dtype=torch.bool) if qhat == math.inf else sref <= qhat
            decided = torch.ones_like(want) if qhat == math.inf else (sref - qhat).abs() > BAR
            undecided = int((~decided).sum())
            share = undecided / decided.numel()
            tally[0] += undecided
            tally[1] += decided.numel()
            if cap_each:
                WORST["undecided"] = max(WORST.get("undecided", 0.0), share)
                assert share <= CAP, (tag, method, qhat, share)
            size, covered, mem = run_sets(zd, qhat, yd, Cc, method, ud, T)
            bits = unpack_dev(mem, Cc)
            assert not bits[:, Cc:].any(), (tag, method, qhat, "padding bits")
            got = bits[:, :Cc].bool()
            wrong = (got != want) & decided
            assert not wrong.any(), (tag, method, qhat, wrong.nonzero()[:4].tolist())
            assert torch.equal(got.sum(1).to(torch.int32), size), (tag, method, qhat, "popcount")
            assert bool(((size.to(torch.int64) - want.sum(1)).abs() <= (~decided).sum(1)).all()), (tag, method, qhat, "size")
            if qhat == math.inf:
                assert bool((size == Cc).all())
            cov_want = torch.zeros_like(keep)
            cov_want[keep] = want[keep].gather(1, yl[keep][:, None])[:, 0]
            cov_decided = torch.ones_like(keep)
            cov_decided[keep] = decided[keep].gather(1, yl[keep][:, None])[:, 0]
            assert bool(((covered.bool() == cov_want) | ~cov_decided).all()) and not covered[~keep].any(), (tag, method, qhat, "covered")
            cov_got = torch.zeros_like(keep)
            cov_got[keep] = got[keep].gather(1, yl[keep][:, None])[:, 0]
            assert torch.equal(cov_got, covered.bool()), (tag, method, qhat, "covered is the label's bit")


def cases(Cc, ld):
    """(kind, rows, random u, T, labels' dtype, off_by_one): N(0, 3) at every row count, the two others at the small ones; u, T and the label
    type alternate so that each value meets each row count's neighbour"""
    out, i = [], 0
    for kind, rows in (("normal", ROWS), ("large", ROWS[:5]), ("equal", ROWS[:4])):
        for n in rows:
            out.append((kind, n, i % 2 == 0, (1.0, 2.5)[(i // 2) % 2], (torch.int32, torch.int64)[(i // 3) % 2], False))
            i += 1
    out.append(("normal", 65, True, 2.5, torch.int32, True))
    out.append(("large", 65, False, 1.0, torch.int64, True))
    return out


@pytest.mark.parametrize("Cc, ld", SHAPES)
def test_kernels_against_the_spec(Cc, ld):
    tally = [0, 0]
    for j, (kind, n, rand_u, T, ydt, off) in enumerate(cases(Cc, ld)):
        tag = (Cc, ld, kind, n, rand_u, T, str(ydt), off)
        z = make_logits(kind, n, Cc, ld, 1000 * Cc + j)
        y = make_labels(n, Cc, 1000 * Cc + j, ydt)
        u = torch.rand(n, generator=torch.Generator().manual_seed(j)) if rand_u else None
        ref = Ref(z, Cc, u, T)
        zd = on_device(z, off)
        ud = None if u is None else u.cuda()
        check_scores(ref, zd, y, Cc, ud, T, tag)
        if Cc <= ops.CONFORMAL_SETS_MAX_C:
            check_sets(ref, zd, y, Cc, ud, T, tag, tally, cap_each=kind != "equal")
    print("worst", WORST, "undecided pairs of the test", tally)
    assert tally[0] <= CAP * tally[1], tally


def test_equal_rows_give_the_index_rule():
    """all-equal rows: s(c) = (c + u) / C, a tie goes to the lower index"""
    for Cc, ld in ((10, 16), (100, 104), (1003, 1008)):
        z = torch.full((5, ld), -0.0)
        z[:, 1:Cc:2] = 0.0                                                  # the two zeros are one value
        u = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0])
        y = torch.tensor([0, Cc - 1, Cc // 2, 1, Cc // 3])
        s, _ = ops.conformal_scores(z.cuda(), y.cuda(), Cc, "aps", u.cuda())
        want = (y.double() + u.double()) / Cc
        assert float((s.double().cpu() - want).abs().max()) <= 1e-6
        size, _, mem = ops.conformal_sets(z.cuda(), 0.5, None, Cc, "aps", torch.zeros(5).cuda(), members=True)
        got = unpack_dev(mem, Cc)[:, :Cc].bool()
        assert got[:, :Cc // 2].all() and not got[:, Cc // 2 + 1:].any() and bool(((size == Cc // 2) | (size == Cc // 2 + 1)).all())


def test_negative_infinity_and_nan():
    z = 3.0 * torch.randn(70, 104, generator=torch.Generator().manual_seed(3))
    z[:, 5:40] = -math.inf
    y = torch.arange(70) % 100
    ref = Ref(z, 100, None, 1.0)
    check_scores(ref, z.cuda(), y, 100, None, 1.0, "neg-inf")
    check_sets(ref, z.cuda(), y, 100, None, 1.0, "neg-inf", [0, 0])
    # a NaN among the valid columns: the call returns, the outputs' guards are intact, the rows beside it are untouched by it
    zn = z.clone()
    zn[7, 3], zn[9, 99] = NAN, -NAN
    for method in CR.METHODS:
        a, _ = run_scores(zn.cuda(), y.cuda(), 100, method, None, 1.0)
        b, _ = run_scores(z.cuda(), y.cuda(), 100, method, None, 1.0)
        clean = torch.ones(70, dtype=torch.bool)
        clean[[7, 9]] = False
        assert torch.equal(a.cpu()[clean], b.cpu()[clean])
        sa = run_sets(zn.cuda(), 0.9, y.cuda(), 100, method, None, 1.0)
        sb = run_sets(z.cuda(), 0.9, y.cuda(), 100, method, None, 1.0)
        for p, q in zip(sa, sb):
            assert torch.equal(p.cpu()[clean], q.cpu()[clean])
        assert bool(((sa[0] >= 0) & (sa[0] <= 100)).all())
    torch.cuda.synchronize()


@pytest.mark.parametrize("Cc, ld", [(10, 16), (100, 102), (1003, 1008), (2048, 2048), (2500, 2501)])
def test_same_bits_on_a_repeat_and_for_a_row_alone(Cc, ld):
    z = make_logits("normal", 130, Cc, ld, 9)
    y = make_labels(130, Cc, 9, torch.int64)
    u = torch.rand(130, generator=torch.Generator().manual_seed(9))
    zd, yd, ud = z.cuda(), y.cuda(), u.cuda()
    for method in CR.METHODS:
        a, ca = ops.conformal_scores(zd, yd, Cc, method, ud, temperature=1.5, lam=LAM, k_reg=K_REG)
        b, cb = ops.conformal_scores(zd, yd, Cc, method, ud, temperature=1.5, lam=LAM, k_reg=K_REG)
        one, c1 = ops.conformal_scores(zd[77:78].contiguous(), yd[77:78].contiguous(), Cc, method, ud[77:78].contiguous(), temperature=1.5, lam=LAM, k_reg=K_REG)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ca, cb)
        assert torch.equal(one.view(torch.int32), a[77:78].view(torch.int32)) and int(c1[0]) == 1
        if Cc > ops.CONFORMAL_SETS_MAX_C:
            continue
        for qhat in (0.9, 0.999):
            p = ops.conformal_sets(zd, qhat, yd, Cc, method, ud, temperature=1.5, lam=LAM, k_reg=K_REG, members=True)
            q = ops.conformal_sets(zd, qhat, yd, Cc, method, ud, temperature=1.5, lam=LAM, k_reg=K_REG, members=True)
            r = ops.conformal_sets(zd[77:78].contiguous(), qhat, yd[77:78].contiguous(), Cc, method, ud[77:78].contiguous(), temperature=1.5, lam=LAM,
                                   k_reg=K_REG, members=True)
            for x, w, o in zip(p, q, r):
                assert torch.equal(x, w) and torch.equal(x[77:78], o)
            # without labels and without members: the same sizes
            s2, c2, m2 = ops.conformal_sets(zd, qhat, None, Cc, method, ud, temperature=1.5, lam=LAM, k_reg=K_REG)
            assert torch.equal(s2, p[0]) and c2 is None and m2 is None


def test_scores_and_sets_agree_on_the_calibration_rows():
    """a set built at qhat = the k-th smallest score of the same rows covers at least k of them (the two kernels form the same float32 score)"""
    z = make_logits("normal", 2000, 100, 104, 21)
    y = make_labels(2000, 100, 21, torch.int64)
    u = torch.rand(2000, generator=torch.Generator().manual_seed(21))
    for method in CR.METHODS:
        s, counts = ops.conformal_scores(z.cuda(), y.cuda(), 100, method, u.cuda(), lam=LAM, k_reg=K_REG)
        keep = ~torch.isnan(s)
        srt = torch.sort(s[keep]).values
        k = 1500
        _, covered, _ = ops.conformal_sets(z.cuda(), float(srt[k - 1]), y.cuda(), 100, method, u.cuda(), lam=LAM, k_reg=K_REG)
        assert abs(int(covered.sum()) - k) <= 1, (method, int(covered.sum()))


def filled_args(n=4, Cc=10, ld=16):
    z = torch.randn(n, ld, device="cuda")
    y = torch.zeros(n, dtype=torch.int64, device="cuda")
    u = torch.rand(n, device="cuda")
    outs = dict(scores=torch.full((n,), -7.0, device="cuda"), counts=torch.full((1,), -7, dtype=torch.int64, device="cuda"),
                size=torch.full((n,), -7, dtype=torch.int32, device="cuda"), covered=torch.full((n,), 77, dtype=torch.uint8, device="cuda"),
                members=torch.full((n + 1, (Cc + 31) // 32), -7, dtype=torch.int32, device="cuda"))
    a = L.uvc_conformal_args()
    a.logits, a.labels, a.u = z.data_ptr(), y.data_ptr(), u.data_ptr()
    a.scores, a.counts, a.size, a.covered, a.members = (outs[k].data_ptr() for k in ("scores", "counts", "size", "covered", "members"))
    a.n, a.ld, a.C, a.labels_i64, a.method, a.k_reg = n, ld, Cc, 1, 1, 0
    a.inv_temperature, a.lam, a.qhat = 1.0, 0.0, 0.5
    return a, outs, (z, y, u)


def untouched(outs):
    torch.cuda.synchronize()
    return bool((outs["scores"] == -7).all() and (outs["counts"] == -7).all() and (outs["size"] == -7).all() and (outs["covered"] == 77).all()
                and (outs["members"] == -7).all())


BAD = [("logits", 0), ("method", 3), ("method", -1), ("inv_temperature", 0.0), ("inv_temperature", -1.0), ("inv_temperature", NAN),
       ("inv_temperature", math.inf), ("lam", -0.5), ("lam", NAN), ("k_reg", -1), ("n", 0), ("n", 2 ** 31), ("C", 0), ("C", 17), ("ld", 9)]


@pytest.mark.parametrize("field, value", BAD)
def test_refusals_leave_the_outputs_alone(field, value):
    for fn in ("uvc_conformal_scores", "uvc_conformal_sets"):
        a, outs, hold = filled_args()
        setattr(a, field, value)
        assert getattr(L.lib(), fn)(C.byref(a), L.cur_stream()) == 1, (fn, field, value)        # UVC_ERR_ARG
        assert untouched(outs), (fn, field, value)


def test_refusals_of_one_call_each():
    lib = L.lib()
    for fn, field, value in (("uvc_conformal_scores", "labels", 0), ("uvc_conformal_scores", "scores", 0), ("uvc_conformal_scores", "counts", 0),
                             ("uvc_conformal_sets", "size", 0), ("uvc_conformal_sets", "labels", 0), ("uvc_conformal_sets", "covered", 0),
                             ("uvc_conformal_sets", "qhat", NAN)):
        a, outs, hold = filled_args()
        setattr(a, field, value)
        assert getattr(lib, fn)(C.byref(a), L.cur_stream()) == 1, (fn, field)
        assert untouched(outs), (fn, field)
    a, outs, hold = filled_args()
    a.members = outs["members"].data_ptr() + 2                                  # members not 4-byte aligned
    assert lib.uvc_conformal_sets(C.byref(a), L.cur_stream()) == 1 and b"misaligned" in lib.uvc_last_error() and untouched(outs)
    a, outs, hold = filled_args()
    a.counts = outs["counts"].data_ptr() + 4
    assert lib.uvc_conformal_scores(C.byref(a), L.cur_stream()) == 1 and untouched(outs)
    # labels and covered both NULL: sets without coverage
    a, outs, hold = filled_args()
    a.labels, a.covered = 0, 0
    assert lib.uvc_conformal_sets(C.byref(a), L.cur_stream()) == 0
    torch.cuda.synchronize()
    assert bool((outs["covered"] == 77).all() and (outs["size"] >= 0).all() and (outs["members"][-1] == -7).all())
    # beyond the supported widths
    z = torch.zeros(2, 2056, device="cuda")
    size = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    with pytest.raises(L.UvcHipError, match="rc=3"):
        ops.conformal_sets(z, 0.5, None, 2049, size=size)
    assert size.tolist() == [-7, -7]
    # through ops, by name
    zz, yy = torch.zeros(2, 8, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")
    for kw in (dict(method="top"), dict(temperature=0.0), dict(lam=-1.0), dict(k_reg=-2)):
        with pytest.raises(L.UvcHipError):
            ops.conformal_scores(zz, yy, 8, **kw)
    with pytest.raises(L.UvcHipError):
        ops.conformal_sets(zz, NAN, yy, 8)
    with pytest.raises(L.UvcHipError):
        ops.conformal_scores(zz.cpu(), yy.cpu(), 8)


def close(a, b):
    """integers (and strings, None, bools) exact, floats within 1e-5"""
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(close(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(close(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and not isinstance(a, bool):
        return isinstance(b, float) and (a == b or abs(a - b) <= 1e-5 * max(1.0, abs(a)))
    return a == b and type(a) is type(b)


@pytest.mark.parametrize("method", CF.METHODS)
def test_fit_and_score_end_to_end(tmp_path, capsys, method):
    """a bank made by ``compact_calibrate logits`` from a micro export on three flat-coloured classes (fp32): the device's calibration and
    record equal the CPU evaluator's on the same bank"""
    ex, _ = KR.export_of("stage2_micro_deit")
    train, test = KR.colour_images(30, 1), KR.colour_images(12, 2)
    root = KR.write_cifar10(str(tmp_path / "data"), train, test)
    f = str(tmp_path / "f.pt")
    torch.save(ex, f)
    bank = {s: str(tmp_path / f"z_{s}.pt") for s in ("train", "test")}
    for split in bank:
        args = CC.build_parser().parse_args(["logits", "--compact", f, "--split", split, "--output", bank[split], "--dataset", "cifar10", "--data_dir", root,
                                             "--eval_batch_size", "8", "--num_workers", "2", "--precision", "fp32"])
        CC.logits_command(args.compact, args)
    capsys.readouterr()
    out, sets_file = str(tmp_path / "conformal.json"), str(tmp_path / "sets.jsonl")
    fit_argv = ["fit", "--bank", bank["train"], "--alpha", "0.1", "--method", method, "--seed", "5", "--output", out]
    cal = CF.main(fit_argv)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == cal == json.load(open(out))
    assert tuple(cal) == CF.FILE_KEYS and (cal["rows"], cal["k"], cal["data_classes"], cal["num_classes"]) == (30, 28, 10, 16)
    cpu_cal = CF.fit_command(CF.build_parser().parse_args(fit_argv[:-1] + [str(tmp_path / "cpu.json")]), scorer=CF.reference_scores)
    assert close(cpu_cal, cal), (cpu_cal, cal)
    score_argv = ["score", "--bank", bank["test"], "--calibration", out, "--sets_output", sets_file]
    rec = CF.main(score_argv)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == rec
    lines = [json.loads(l) for l in open(sets_file)]
    cpu_rec = CF.score_command(CF.build_parser().parse_args(score_argv), setter=CF.reference_sets)
    assert close(cpu_rec, rec), (cpu_rec, rec)
    assert lines == [json.loads(l) for l in open(sets_file)] and len(lines) == 12 and rec["rows"] == 12
    assert all(l["size"] == len(l["set"]) and l["covered"] == (l["label"] in l["set"]) for l in lines)
    assert abs(rec["coverage"] - sum(l["covered"] for l in lines) / 12) < 1e-12 and abs(rec["mean_size"] - sum(l["size"] for l in lines) / 12) < 1e-12
