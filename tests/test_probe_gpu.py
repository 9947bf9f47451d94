"""GPU: the linear probe's device code (uvc_amd/csrc/probe.hip) -- the softmax / cross-entropy row kernel against float64 on the same float32
logits, the evaluator against ``reference_objective`` on the operands as the device sees them, the fit against the same solver on the CPU,
and the commands end to end."""
import ctypes as C
import functools
import json
import math

import pytest
import torch

import knn_ref as KR
import probe_ref as PR
from uvc_amd import _lib as L
from uvc_amd import compact as CP
from uvc_amd import compact_probe as PB
from uvc_amd import compact_transfer as CT
from uvc_amd import ops

pytestmark = pytest.mark.gpu

BITS = lambda t: t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16 if t.element_size() == 2 else torch.int64)
same_bits = lambda a, b: a.shape == b.shape and a.dtype == b.dtype and torch.equal(BITS(a), BITS(b))
GDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
ROWS = (1, 63, 64, 65, 1000)
# (C, ld): ld = C rounded up to 8; one ld that is no multiple of 4 (the element path); two rows wider than 2048 columns (one workgroup per row)
WIDTHS = [(1, 8), (2, 8), (10, 16), (100, 104), (1000, 1000), (1003, 1008), (100, 102), (2500, 2504), (2500, 2501)]
SENTINEL = 768.0                                    # (exact in bfloat16)


def rows_per_block(ld):
    """the rows of one loss / hit partial at this width, from the library's own block count"""
    return max(k for k in (1, 64, 128, 256) if ops.softmax_xent_grad_blocks(k, ld) == 1)


def run_rows(z, y, Cc, prec, pad_cols=0):
    """the kernel on a G buffer with a guard row on either side and ``pad_cols`` guard columns: (G, loss_part, hit_part, whole buffer)"""
    rows, ld = z.shape
    buf = torch.full((rows + 2, ld + pad_cols), SENTINEL, dtype=GDT[prec], device="cuda")
    G, lp, hp = ops.softmax_xent_grad(z, y, Cc, G=buf[1:rows + 1], rows=rows)
    return G, lp, hp, buf


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["normal", "huge", "ties"])
def test_row_kernel_against_float64(prec, kind):
    """float32 G: |G - ref| <= 4 ulp32(max(p, 2^-24)), plus at the label column -- where G = p - 1 is ROUNDED to float32 -- half a
    float32 spacing of the reference (no float32 holds p - 1 closer than that; the issue's bound reads on p).  bfloat16 G: the float64 value
    rounded once, or a bfloat16 neighbour of it.  Loss partials: k 2^-24 sum |terms| with k = rows of the partial + 12 (a term's own error
    in units of 2^-24: 4 the exponentials, 4 log1pf, 2 the two subtractions, 2 spare).  Hits, +0 padding, guards and repeats exact."""
    worst_g = worst_l = 0.0
    for Cc, ld in (WIDTHS if kind == "normal" else WIDTHS[2:6]):
        per = rows_per_block(ld)
        for rows in ROWS:
            if ld > 2048 and rows == 1000:
                continue
            z, y = PR.row_logits(rows, Cc, ld, kind, seed=rows * 7 + Cc)
            refG, ref_loss, ref_hit, p = PR.row_reference(z, y, Cc)
            zd = z.cuda()
            for yd in (y.cuda(), y.to(torch.int32).cuda()):
                G, lp, hp, buf = run_rows(zd, yd, Cc, prec, pad_cols=8 if yd.dtype == torch.int32 else 0)
                got = G[:, :ld].double().cpu()
                assert not torch.isnan(got).any() and not torch.isinf(got).any(), (Cc, ld, rows)
                if prec == "fp32":
                    tol = 4 * PR.ulp32(p.clamp_min(2.0 ** -24))
                    keep = (y >= 0) & (y < Cc)
                    lab = torch.zeros_like(p, dtype=torch.bool)
                    lab[torch.arange(rows)[keep], y[keep]] = True
                    tol = tol + lab * 0.5 * PR.ulp32(refG)
                    ratio = float(((got - refG).abs() / tol).max())
                    worst_g = max(worst_g, ratio)
                    assert ratio <= 1.0, (Cc, ld, rows, ratio)
                else:
                    near = refG.float().bfloat16()
                    step = (PR.bf16_key(G[:, :ld].cpu()) - PR.bf16_key(near)).abs()
                    exact_zero = (refG == 0)
                    assert int(step.max()) <= 1 and not G[:, :ld].cpu()[exact_zero].any(), (Cc, ld, rows, int(step.max()))
                    worst_g = max(worst_g, float(step.max()))
                # +0 (not -0) on the padding columns and on uncounted rows
                gb = BITS(G[:, :ld]).cpu()
                assert not gb[:, Cc:].any() and not gb[(y < 0) | (y >= Cc)].any(), (Cc, ld, rows)
                # guards: the rows around and the columns behind
                assert bool((buf[0] == SENTINEL).all()) and bool((buf[rows + 1] == SENTINEL).all()) and bool((buf[:, ld:] == SENTINEL).all())
                # partials
                blocks = PR.blocks_of(rows, per)
                assert lp.shape[0] == hp.shape[0] == len(blocks)
                assert torch.equal(hp.cpu().to(torch.int64), torch.stack([ref_hit[s].sum() for s in blocks])), (Cc, ld, rows)
                for i, s in enumerate(blocks):
                    bound = sum_bound(s.stop - s.start + 12, float(ref_loss[s].abs().sum()))
                    err = abs(float(lp[i]) - float(ref_loss[s].sum()))
                    worst_l = max(worst_l, err / max(bound, 1e-300))
                    assert err <= bound, (Cc, ld, rows, i, err, bound)
                G2, lp2, hp2, buf2 = run_rows(zd, yd, Cc, prec, pad_cols=8 if yd.dtype == torch.int32 else 0)
                assert same_bits(buf, buf2) and same_bits(lp, lp2) and same_bits(hp, hp2)
    print(f"row kernel {prec} {kind}: worst G error / bound {worst_g:.3f}, worst loss error / bound {worst_l:.3f}")


def sum_bound(n, abs_terms_sum):
    """tests/pixel_attr_ref.py's float32 summation bound of n terms: n 2^-24 sum |terms|"""
    import pixel_attr_ref
    return pixel_attr_ref.sum_bound(n, abs_terms_sum)


def test_row_kernel_result_does_not_depend_on_the_rows_beside_it():
    for Cc, ld in [(10, 16), (1000, 1000), (2500, 2504)]:
        z, y = PR.row_logits(130, Cc, ld, "normal", seed=5)
        zd, yd = z.cuda(), y.cuda()
        G, _, _ = ops.softmax_xent_grad(zd, yd, Cc)
        for r in (0, 64, 129):
            one, lp, hp = ops.softmax_xent_grad(zd[r:r + 1].contiguous(), yd[r:r + 1].contiguous(), Cc)
            assert same_bits(one[0], G[r])


def test_row_kernel_refusals_leave_outputs_untouched():
    z, y = torch.randn(4, 16, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    G = torch.full((4, 16), SENTINEL, device="cuda")
    lp, hp = torch.full((1,), SENTINEL, device="cuda"), torch.full((1,), 7, dtype=torch.int32, device="cuda")
    lib, st = L.lib(), L.cur_stream()
    base = dict(z=L.ptr(z), y=L.ptr(y), i64=1, rows=4, C=10, ld=16, G=L.ptr(G), ldg=16, dt=0, lp=L.ptr(lp), hp=L.ptr(hp))
    call = lambda **k: lib.uvc_softmax_xent_grad(*[{**base, **k}[n] for n in ("z", "y", "i64", "rows", "C", "ld", "G", "ldg", "dt", "lp", "hp")], st)
    for bad in (dict(z=None), dict(y=None), dict(G=None), dict(lp=None), dict(hp=None), dict(rows=0), dict(C=0), dict(C=65537), dict(C=17), dict(ldg=8),
                dict(dt=2), dict(z=L.ptr(z) + 2), dict(G=L.ptr(G) + 1), dict(y=L.ptr(y) + 4)):
        assert call(**bad) != 0, bad
    torch.cuda.synchronize()
    assert bool((G == SENTINEL).all()) and float(lp) == SENTINEL and int(hp) == 7
    assert call() == 0


# ---- the evaluator ----------------------------------------------------------------------------------------------------------------------
# every n, D and C the issue names appears; chunk_rows 64, 1000 and n cut inside a chunk, at its end and not at all
EVAL_SHAPES = [(1, 8, 1), (1, 1024, 1000), (65, 192, 10), (65, 384, 100), (65, 1024, 1), (1000, 8, 100), (1000, 384, 1000), (1000, 1024, 10),
               (4097, 8, 1), (4097, 192, 1000), (4097, 384, 10), (4097, 1024, 100)]
L2 = 1e-2


@functools.lru_cache(maxsize=None)
def eval_case(n, D, Cc, prec):
    """host operands and the float64 reference on the operands as the device sees them (computed once, shared, never written to)"""
    X, y = PR.gaussian_classes(n, D, max(Cc, 2), seed=n + D + Cc, spread=0.6)
    g = torch.Generator().manual_seed(n * 3 + D + Cc)
    y = y % Cc
    if n >= 65:
        y[3], y[n - 2] = -1, Cc                                                       # two uncounted rows
    Cp = -(-Cc // 8) * 8
    W = torch.zeros(Cp, D)
    W[:Cc] = torch.randn(Cc, D, generator=g) * (1.0 / math.sqrt(D))
    W[Cc:] = 5.0                                                                      # padding rows: they must take no part
    b = torch.zeros(Cp)
    b[:Cc] = torch.randn(Cc, generator=g) * 0.5
    b[Cc:] = 50.0
    Xo = X.float().bfloat16() if prec == "bf16" else X.float()
    Wr = W.bfloat16().float() if prec == "bf16" else W
    # the reference sees X and W as the device's GEMMs do; l2 acts on the float32 master
    F, dW, db, hits = PB.reference_objective(Wr[:Cc], b[:Cc], Xo.double(), y, 0.0)
    F += 0.5 * L2 * float((W[:Cc].double() ** 2).sum())
    dW = dW + L2 * W[:Cc].double()
    m = int(((y >= 0) & (y < Cc)).sum())
    return Xo, y, W, b, (F, dW, db, hit_range(Xo, y, Wr, b, Cc, D, hits), m)


def hit_range(Xo, y, Wr, b, Cc, D, hits):
    """``(lo, hi)`` around the reference's hits: a row is ambiguous when its label is among the two largest float64 logits and they lie
    within twice the float32 accumulation bound of the device's logits, (D + 2) 2^-24 (sum_d |x_d w_d| + |b|) -- there the float32 argmax
    is not defined by the float64 one.  Everywhere else the count is exact (and the row kernel's own hits are held exactly, on identical
    float32 logits, above)."""
    if Cc < 2:
        return hits, hits
    Wd = Wr[:Cc].double()
    z = Xo.double() @ Wd.T + b[:Cc].double()
    top = z.topk(2, dim=1)
    yc = y.clamp(0, Cc - 1)
    keep = (y >= 0) & (y < Cc)
    err = (D + 2) * 2.0 ** -24 * ((Xo.double().abs() @ Wd.abs().T).max(1).values + float(b[:Cc].abs().max()))
    amb = keep & (top.indices == yc[:, None]).any(1) & (top.values[:, 0] - top.values[:, 1] <= 2 * err)
    sure = int((keep & ~amb & (top.indices[:, 0] == yc)).sum())
    assert int(amb.sum()) <= max(1, len(y) // 100)                                   # (the data: all but a handful of rows are decided)
    return sure, sure + int(amb.sum())


def bf16_g_error(Xo, y, W, b, Cc, ref_dW):
    """e_ref: the same reference with bf16 operands and G rounded once to bf16 on the CPU, against the reference (relative to max |ref|)"""
    X = Xo.double()
    z = X @ W[:Cc].bfloat16().double().T + b[:Cc].double()
    keep = (y >= 0) & (y < Cc)
    G = torch.softmax(z, dim=1)
    G[torch.arange(len(y)), y.clamp(0, Cc - 1)] -= 1.0
    G = (G * keep[:, None]).float().bfloat16().double()
    dW = G.T @ X / max(int(keep.sum()), 1) + L2 * W[:Cc].double()
    return float((dW - ref_dW).abs().max()) / max(float(ref_dW.abs().max()), 1e-300), G


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("n,D,Cc", EVAL_SHAPES)
def test_evaluator_against_the_reference(n, D, Cc, prec):
    """float32: max |got - ref| <= 1e-3 max |ref| for dW, db and F.  bfloat16: the issue's derivation -- (2^-9 + k 2^-24) (1/m) sum_i |g_ic x_id|
    per element -- does not close: the unit roundoff of bfloat16 is 2^-8 (2^-9 only at the top of a binade), and with C classes a column of
    G is one label term near -1 among terms near 0, so a single rounding can carry the element; so the project's rule max(2e-2, 2 e_ref)
    holds dW, db and F (relative to max |ref|), e_ref being the reference with a bf16 G on the CPU, and the fraction of the derived
    bound that was used is printed beside it.  m exact, hits exact outside ``hit_range``'s ambiguous rows; chunk_rows 64, 1000 and n agree within the same bars; a repeat in bits."""
    Xo, y, W, b, (F, dW, db, (hits_lo, hits_hi), m) = eval_case(n, D, Cc, prec)
    bar, e_ref, frac_of = 1e-3, None, None
    if prec == "bf16":
        e_ref, Gr = bf16_g_error(Xo, y, W, b, Cc, dW)
        bar = max(2e-2, 2 * e_ref)
        k = n + 64
        frac_of = (2.0 ** -9 + k * 2.0 ** -24) * (Gr.abs().T @ Xo.double().abs()) / max(m, 1) + 2.0 ** -24 * (L2 * W[:Cc].double().abs() + dW.abs())
    Xd, yd, Wd, bd = Xo.cuda(), y.cuda(), W.cuda(), b.cuda()

    def rel(got, ref):
        top = float(ref.abs().max())
        if top == 0:                                                                    # (C = 1: G is zero, db must be exactly zero)
            return 0.0 if not got.any() else float("inf")
        return float((got.double().cpu() - ref).abs().max()) / top
    first = None
    for chunk in (64, 1000, n):
        gW, gb, gF, counts = ops.probe_eval(Xd, yd, Wd, bd, Cc, L2, chunk_rows=chunk)
        e = (rel(gW[:Cc], dW), rel(gb[:Cc], db), abs(float(gF) - F) / abs(F))
        used = float(((gW[:Cc].double().cpu() - dW).abs() / frac_of.clamp_min(1e-300)).max()) if frac_of is not None else float("nan")
        print(f"probe_eval {prec} n={n} D={D} C={Cc} chunk={chunk}: dW {e[0]:.2e} db {e[1]:.2e} F {e[2]:.2e} (bar {bar:.1e}, e_ref {e_ref}, of the 2^-9 bound {used:.3f})")
        assert max(e) <= bar, (chunk, e, bar)
        assert hits_lo <= int(counts[0]) <= hits_hi and int(counts[1]) == m, (chunk, counts.tolist(), hits_lo, hits_hi, m)
        assert not BITS(gW[Cc:]).any() and not BITS(gb[Cc:]).any()                      # exactly zero gradients on the padding rows
        again = ops.probe_eval(Xd, yd, Wd, bd, Cc, L2, chunk_rows=chunk)
        assert all(same_bits(u, v) for u, v in zip((gW, gb, gF, counts), again)), chunk
        if first is None:
            first = (gW, gb, gF)
        else:                                                                           # another chunk_rows: within the bars of one another too
            assert rel(gW[:Cc], first[0][:Cc].double().cpu()) <= bar and abs(float(gF) - float(first[2])) <= bar * abs(F)
    # int32 labels, no bias and a row stride: the same objective without its bias terms
    wide = torch.zeros(n, D + 8, dtype=Xd.dtype, device="cuda")
    wide[:, :D] = Xd
    gW, gb, gF, counts = ops.probe_eval(wide[:, :D], yd.to(torch.int32), Wd, None, Cc, L2, chunk_rows=64)
    rF, rW, _, rh = PB.reference_objective((W.bfloat16().float() if prec == "bf16" else W)[:Cc], None, Xo.double(), y, 0.0)
    assert gb is None and int(counts[1]) == m
    assert rel(gW[:Cc], rW + L2 * W[:Cc].double()) <= bar


def test_evaluator_refusals_leave_outputs_untouched():
    n, D, Cc = 70, 16, 10
    X = torch.randn(n, D, device="cuda").bfloat16()
    y = torch.zeros(n, dtype=torch.int64, device="cuda")
    W, b = torch.zeros(16, D, device="cuda"), torch.zeros(16, device="cuda")
    dW, db = torch.full((16, D), SENTINEL, device="cuda"), torch.full((16,), SENTINEL, device="cuda")
    F, counts = torch.full((1,), SENTINEL, dtype=torch.float64, device="cuda"), torch.full((2,), 7, dtype=torch.int64, device="cuda")
    ws = torch.empty(ops.probe_workspace_bytes(n, D, Cc, ops.UVC_BF16, 64) + 16, dtype=torch.uint8, device="cuda")
    lib, st = L.lib(), L.cur_stream()

    def call(**k):
        a = L.uvc_probe_args()
        a.X, a.labels, a.W, a.b, a.dW, a.db, a.F, a.counts = (L.ptr(t) for t in (X, y, W, b, dW, db, F, counts))
        a.workspace, a.workspace_bytes = L.ptr(ws), ws.numel() - 16
        a.n, a.ldx, a.l2, a.D, a.C, a.dtype, a.labels_i64, a.chunk_rows = n, D, 1e-3, D, Cc, ops.UVC_BF16, 1, 64
        for name, v in k.items():
            setattr(a, name, v)
        return lib.uvc_probe_eval(C.byref(a), st)
    for bad in (dict(X=None), dict(labels=None), dict(W=None), dict(dW=None), dict(F=None), dict(counts=None), dict(workspace=None), dict(b=None),
                dict(db=None), dict(X=L.ptr(X) + 2), dict(W=L.ptr(W) + 4), dict(dW=L.ptr(dW) + 4), dict(workspace=L.ptr(ws) + 8), dict(F=L.ptr(F) + 4),
                dict(D=12), dict(D=1032), dict(D=0), dict(C=0), dict(C=65537), dict(n=0), dict(workspace_bytes=ws.numel() - 16 - 256), dict(chunk_rows=0),
                dict(ldx=8), dict(ldx=D + 4), dict(l2=-1.0), dict(dtype=2)):
        assert call(**bad) != 0, bad
    assert lib.uvc_probe_eval(None, st) != 0
    nb = C.c_int64(0)
    for bad in ((0, D, Cc), (n, 12, Cc), (n, 2048, Cc), (n, D, 0), (n, D, 65537)):
        assert lib.uvc_probe_workspace_bytes(bad[0], bad[1], bad[2], ops.UVC_BF16, 64, C.byref(nb)) != 0
    torch.cuda.synchronize()
    assert bool((dW == SENTINEL).all()) and bool((db == SENTINEL).all()) and float(F) == SENTINEL and counts.tolist() == [7, 7]
    assert call() == 0
    torch.cuda.synchronize()
    assert counts.tolist()[1] == n and not bool((dW == SENTINEL).any())


# ---- the fit ------------------------------------------------------------------------------------------------------------------------------
_FIT = {}


def fit_problem():
    if not _FIT:
        X, y = PR.gaussian_classes(600, 64, 5, seed=0, spread=0.6)
        _FIT.update(X=X, y=y)
        for l2 in (1e-4, 1e-2):
            opt = PB.fit_probe(X, y, 5, l2, evaluator=PB.reference_objective, tol_grad=1e-10)
            assert 50.0 < opt["top1"] < 95.0                                            # overlapping classes: the optimum is interior
            _FIT[l2] = opt["F"]
    return _FIT


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("l2", [1e-4, 1e-2])
def test_fit_against_the_same_solver_on_the_cpu(l2, prec):
    """F64(W_dev) - F* against the same gap of the same solver on the CPU in float32 (fp32) or with bf16-rounded operands (bf16), F* the
    float64 optimum: at most twice the reference's gap.
    Measured: see the README's probe section."""
    P = fit_problem()
    X, y, Fstar = P["X"], P["y"], P[l2]
    gap = lambda r: PB.reference_objective(r["W"].double(), r["b"].double(), X, y, l2)[0] - Fstar
    ref = PB.fit_probe(X, y, 5, l2, evaluator=PR.LowEvaluator(prec))
    dev = PB.fit_probe(X.float(), y, 5, l2, precision=prec)
    g_ref, g_dev = gap(ref), gap(dev)
    print(f"fit {prec} l2={l2:g}: device gap {g_dev:.3e} ({dev['iterations']} iterations, {dev['evaluations']} evaluations), "
          f"CPU {prec} gap {g_ref:.3e} ({ref['iterations']} iterations, {ref['evaluations']} evaluations), F* {Fstar:.6f}")
    assert g_ref > 0 and g_dev > -1e-12
    assert g_dev <= 2 * g_ref, (g_dev, g_ref)
    assert dev["W"].dtype == torch.float32 and tuple(dev["W"].shape) == (5, 64) and dev["rows"] == 600
    F64, _, _, hits = PB.reference_objective(dev["W"].double(), dev["b"].double(), X, y, l2)
    assert abs(dev["F"] - F64) <= (1e-3 if prec == "fp32" else 2e-2) * F64


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def test_command(tmp_path, capsys):
    """embed, fit and score on three flat-coloured classes through the CIFAR-10 reader; the written file, run by CompactVisionTransformer on
    the test images, gives the top-1 score printed, and no padding logit wins."""
    import argparse
    from uvc_amd import data
    ex, _ = KR.export_of("stage2_micro_deit")
    train, test = KR.colour_images(30, 1), KR.colour_images(12, 2)
    root = KR.write_cifar10(str(tmp_path / "data"), train, test)
    torch.save(ex, tmp_path / "f.pt")
    f, g = str(tmp_path / "f.pt"), str(tmp_path / "g.pt")
    raw = {s: str(tmp_path / f"raw_{s}.pt") for s in ("train", "test")}
    dflags = ["--dataset", "cifar10", "--data_dir", root, "--eval_batch_size", "8", "--num_workers", "2", "--precision", "fp32"]
    capsys.readouterr()
    for split, n in (("train", 30), ("test", 12)):
        s = PB.main(["embed", "--compact", f, "--split", split, "--output", raw[split]] + dflags)
        assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == s
        assert (s["images"], s["data_classes"], s["embed_dim"], s["normalized"]) == (n, 10, 128, False)
    bank = CT.load_bank(raw["train"])
    assert bank["normalized"] is False and "normalized" not in bank["meta"] and torch.equal(bank["labels"], torch.from_numpy(train[1]))
    want = CT.reference_features(ex, torch.cat([x.cpu() for x, _ in data.build_eval_loader(argparse.Namespace(
        dataset="cifar10", data_dir=root, img_size=ex["cfg"]["img_size"], eval_batch_size=8, num_workers=2, interpolation="bilinear", crop_pct=None,
        packed_dir=None, resident=0), "train")[0]]).double(), normalize=False)
    assert float((bank["features"].double() - want).abs().max()) <= 1e-3 * float(want.abs().max())
    line = PB.main(["fit", "--compact", f, "--bank", raw["train"], "--val_bank", raw["test"], "--l2", "1e-2", "1e-1", "--max_iter", "200", "--refit", "0",
                    "--precision", "fp32", "--output", g])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == line
    assert set(line) >= {"records", "l2", "train_top1", "val_top1", "evaluations", "seconds", "blocks", "params", "macs_compact", "normalized_bank"}
    assert [r["l2"] for r in line["records"]] == [1e-1, 1e-2] and line["normalized_bank"] is False and line["num_classes"] == 16
    assert line["val_top1"] == max(r["val_top1"] for r in line["records"]) > 50.0 and line["train_top1"] > 50.0      # (chance: a third)
    assert line["l2"] == max(r["l2"] for r in line["records"] if r["val_top1"] == line["val_top1"])
    assert line["evaluations"] == sum(r["evaluations"] for r in line["records"])
    score = PB.main(["score", "--compact", g, "--bank", raw["test"], "--precision", "fp32"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == score
    assert (score["images"], score["data_classes"], score["top1"]) == (12, 10, line["val_top1"])
    # the file in the model: the same top-1 over ALL num_classes logits
    out = CP.load_compact(g)
    assert bool((out["state_dict"]["head.bias"][10:] == PB.PAD_BIAS).all())
    cm = CP.CompactVisionTransformer(out, precision="fp32")
    ns = argparse.Namespace(dataset="cifar10", data_dir=root, img_size=ex["cfg"]["img_size"], eval_batch_size=8, num_workers=2, interpolation="bilinear",
                            crop_pct=None, packed_dir=None, resident=0)
    hits = total = 0
    for x, yb in data.build_eval_loader(ns, "test")[0]:
        logits = cm(x)[0]
        assert logits.shape[1] == 16
        pred = logits.argmax(1)
        assert bool((pred < 10).all())
        hits += int((pred.cpu() == yb.cpu()).sum())
        total += int(yb.shape[0])
    assert total == 12 and 100.0 * hits / total == score["top1"]
    # a normalised bank: refused with a bias, by fit and by score
    normed = dict(bank, normalized=True)
    torch.save(normed, tmp_path / "normed.pt")
    with pytest.raises(ValueError, match="--bias 0"):
        PB.main(["fit", "--compact", f, "--bank", str(tmp_path / "normed.pt"), "--output", g])
    with pytest.raises(ValueError, match="normalized"):
        PB.main(["score", "--compact", g, "--bank", str(tmp_path / "normed.pt")])
    nb = PB.main(["fit", "--compact", f, "--bank", str(tmp_path / "normed.pt"), "--bias", "0", "--l2", "1e-2", "--max_iter", "100", "--precision", "fp32",
                  "--output", str(tmp_path / "h.pt")])
    assert nb["normalized_bank"] is True and nb["bias"] == 0 and nb["records"][0]["val_top1"] is None and nb["refit"] == 0
