"""GPU: the calibration kernels (uvc_amd/csrc/calib.hip) -- ``ops.calib_eval`` against ``reference_objective`` and ``ops.calib_stats`` against
``reference_reliability`` in float64 on the same float32 inputs, the fit against the same solver on the CPU, and the commands end to end."""
import argparse
import ctypes as C
import json

import pytest
import torch

import calib_ref as CR
import knn_ref as KR
from uvc_amd import _lib as L
from uvc_amd import compact as CP
from uvc_amd import compact_calibrate as CC
from uvc_amd import ops

pytestmark = pytest.mark.gpu

NAN = float("nan")
BITS = lambda t: t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)
same_bits = lambda a, b: a.shape == b.shape and a.dtype == b.dtype and torch.equal(BITS(a), BITS(b))
BAR = 1e-3                                          # the project's float32 rule: max |got - ref| <= 1e-3 max |ref|
WORST = {}


def rel(got, ref, noise=0.0):
    """max |got - ref| over max |ref|, less the float64 reference's own rounding ``noise``: a sum that is zero in exact arithmetic (a row of
    equal logits gives sum_c g_c z_c = 0) comes out of float64 as 1e-17, and no bar relative to THAT means anything"""
    top = float(ref.abs().max())
    if top == 0:                                                                        # (C = 1: g is zero, the gradient must be exactly zero)
        return 0.0 if not got.any() else float("inf")
    return max(float((got.double().cpu() - ref).abs().max()) - noise, 0.0) / top


def run_eval(zd, yd, scale, shift, Cc):
    """the kernel on outputs with a guard element on either side, ``dshift`` handed in even without a shift:
    ``(F, dscale, dshift buffer view, counts, the four whole buffers)``"""
    k = scale.numel()
    Fb = torch.full((3,), NAN, dtype=torch.float64, device="cuda")
    sb, db = torch.full((k + 2,), NAN, device="cuda"), torch.full((Cc + 2,), NAN, device="cuda")
    cb = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    F, ds, dd, counts = ops.calib_eval(zd, yd, scale, shift, Cc, F=Fb[1:2], dscale=sb[1:k + 1], dshift=db[1:Cc + 1], counts=cb[1:3])
    return F, ds, db[1:Cc + 1], counts, (Fb, sb, db, cb)


def check_eval(z, y, zd, yd, maps, mode, Cc, tag):
    scale, shift = maps[mode]
    rF, rs, rd, _, m = CC.reference_objective(z, y, scale, shift, Cc)
    lo, hi, undecided = CR.hit_range(z, y, scale, shift, Cc)
    assert undecided <= CR.CAP * len(y), (tag, undecided)
    sd, hd = scale.cuda(), None if shift is None else shift.cuda()
    F, ds, dd, counts, bufs = run_eval(zd, yd, sd, hd, Cc)
    noise = 1e-12 * float(z[:, :Cc].abs().max())
    e = (abs(float(F) - rF) / abs(rF) if rF else abs(float(F)), rel(ds, rs, noise), rel(dd, rd, 1e-12) if shift is not None else 0.0)
    for name, v in zip(("F", "dscale", "dshift"), e):
        WORST[name] = max(WORST.get(name, 0.0), v)
    assert max(e) <= BAR, (tag, e)
    assert int(counts[1]) == m and lo <= int(counts[0]) <= hi, (tag, counts.tolist(), lo, hi, m)
    Fb, sb, db, cb = bufs
    assert torch.isnan(Fb[[0, 2]]).all() and torch.isnan(sb[[0, -1]]).all() and torch.isnan(db[[0, -1]]).all() and cb[[0, 3]].tolist() == [-7, -7], tag
    if shift is None:
        assert torch.isnan(db).all(), tag                                               # dshift is not touched without a shift
    again = run_eval(zd, yd, sd, hd, Cc)[4]
    assert all(same_bits(u, v) for u, v in zip(bufs, again)), tag
    return F, ds, dd, counts


@pytest.mark.parametrize("kind", ["normal", "huge", "ties"])
@pytest.mark.parametrize("Cc,ld", CR.WIDTHS)
def test_calib_eval_against_the_reference(Cc, ld, kind):
    """F, dscale and dshift within 1e-3 of max |ref| (F: relative); m exact, hits exact outside ``calib_ref.hit_range``'s undecided rows (at
    most 1 % of the rows, checked on the CPU as well); guards, an untouched dshift without a shift and a repeat in bits.  Every row count,
    both modes with and without a shift; int32 and int64 labels with -1 and C among them; NaN in the padding columns; at 65 rows also a row
    stride and a base one element off 16-byte alignment."""
    for rows in CR.ROWS:
        z, y = CR.case_inputs(rows, Cc, ld, kind, seed=CR.case_seed(rows, Cc))
        maps = CR.case_maps(Cc, kind, seed=CR.case_seed(rows, Cc))
        zd = z.cuda()
        for i, mode in enumerate(CR.MODES):
            yd = y.cuda() if i % 2 == 0 else y.to(torch.int32).cuda()
            base = check_eval(z, y, zd, yd, maps, mode, Cc, (Cc, ld, kind, rows, mode))
            if rows == 65:
                wide = torch.full((rows, ld + 12), NAN, device="cuda")
                wide[:, :ld] = zd
                flat = torch.full((rows * ld + 1,), NAN, device="cuda")
                off = flat[1:].view(rows, ld)
                off.copy_(zd)
                assert off.data_ptr() % 16 == 4
                for view in (wide[:, :ld], off):
                    got = check_eval(z, y, view, yd, maps, mode, Cc, (Cc, ld, kind, rows, mode, "view"))
                    assert torch.equal(got[3], base[3])
    print(f"calib_eval {kind} C={Cc} ld={ld}: worst errors so far {WORST}")


def test_a_row_contributes_the_same_alone_and_among_130():
    """m F and m dshift with and without a row differ by what the row gives alone: F within float64 summation of float32 row losses,
    dshift within the float32 bound 2 (130 + 4) 2^-24 sum_i |g_ic| of the two sums that are subtracted."""
    for Cc, ld in [(10, 16), (1000, 1000), (2500, 2504)]:
        z, y = CR.case_inputs(130, Cc, ld, "normal", seed=5)
        scale, shift = CR.case_maps(Cc, "normal", seed=5)[("vector", True)]
        zd, sd, hd = z.cuda(), scale.cuda(), shift.cuda()
        zp, yk = CR.mapped(z, y, scale, shift, Cc)
        g = torch.softmax(zp, dim=1)
        g[torch.arange(len(yk)), yk] -= 1.0
        bound = 2 * (130 + 4) * 2.0 ** -24 * g.abs().sum(0)
        F, _, dd, counts = ops.calib_eval(zd, y.cuda(), sd, hd, Cc)
        m = int(counts[1])
        assert m == 128
        for r in (0, 64, 129):
            y2 = y.clone()
            y2[r] = -1
            F2, _, dd2, c2 = ops.calib_eval(zd, y2.cuda(), sd, hd, Cc)
            F1, _, dd1, c1 = ops.calib_eval(zd[r:r + 1].contiguous(), y[r:r + 1].cuda(), sd, hd, Cc)
            assert int(c2[1]) == m - 1 and int(c1[1]) == 1
            assert abs(m * float(F) - (m - 1) * float(F2) - float(F1)) <= 1e-10 * m * abs(float(F)), (Cc, r)
            diff = (m * dd.double() - (m - 1) * dd2.double() - dd1.double()).abs().cpu()
            assert bool((diff <= bound).all()), (Cc, r, float((diff / bound).max()))


def test_zero_counted_rows_give_zeros():
    z = torch.randn(70, 16, device="cuda")
    y = torch.full((70,), -1, dtype=torch.int64, device="cuda")
    y[::2] = 10
    for scale, shift in ((torch.ones(1, device="cuda"), None), (torch.ones(10, device="cuda"), torch.zeros(10, device="cuda"))):
        F, ds, dd, counts = ops.calib_eval(z, y, scale, shift, 10)
        assert float(F) == 0.0 and not ds.any() and counts.tolist() == [0, 0] and (dd is None or not dd.any())
    n, c, h, sums, counts = ops.calib_stats(z, y, torch.ones(1, device="cuda"), None, 10, 15)
    assert not n.any() and not c.any() and not h.any() and not sums.any() and counts.tolist() == [0, 0]


def test_blocks_depend_on_the_shape_alone():
    assert ops.calib_blocks(1, 8) == 1 and ops.calib_blocks(1281167, 1000) <= 1024 and ops.calib_blocks(50000, 1000) == ops.calib_blocks(50000, 1000)
    assert ops.calib_blocks(4097, 2501) > 1 and ops.calib_blocks(1000, 16) > 1
    assert ops.calib_workspace_bytes(1000, 16, 10) > 0 and ops.calib_workspace_bytes(1000, 16, 10, 15) > 0


def test_refusals_leave_outputs_untouched():
    n, Cc, ld = 70, 10, 16
    z, y = torch.randn(n, ld, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
    scale, shift = torch.ones(Cc, device="cuda"), torch.zeros(Cc, device="cuda")
    F, counts = torch.full((1,), NAN, dtype=torch.float64, device="cuda"), torch.full((2,), -7, dtype=torch.int64, device="cuda")
    ds, dd = torch.full((Cc,), NAN, device="cuda"), torch.full((Cc,), NAN, device="cuda")
    bn, bh = torch.full((15,), -7, dtype=torch.int64, device="cuda"), torch.full((15,), -7, dtype=torch.int64, device="cuda")
    bc, sums = torch.full((15,), NAN, dtype=torch.float64, device="cuda"), torch.full((2,), NAN, dtype=torch.float64, device="cuda")
    ws = torch.empty(max(ops.calib_workspace_bytes(n, ld, Cc), ops.calib_workspace_bytes(n, ld, Cc, 15)) + 16, dtype=torch.uint8, device="cuda")
    lib, st = L.lib(), L.cur_stream()

    def call(fn, **k):
        a = L.uvc_calib_args()
        a.logits, a.labels, a.scale, a.shift, a.F, a.dscale, a.dshift, a.counts = (L.ptr(t) for t in (z, y, scale, shift, F, ds, dd, counts))
        a.bin_count, a.bin_conf, a.bin_hit, a.sums = (L.ptr(t) for t in (bn, bc, bh, sums))
        a.workspace, a.workspace_bytes = L.ptr(ws), ws.numel() - 16
        a.n, a.ld, a.C, a.scale_len, a.labels_i64, a.bins = n, ld, Cc, Cc, 1, 15
        for name, v in k.items():
            setattr(a, name, v)
        return fn(C.byref(a), st)
    shared = (dict(logits=None), dict(labels=None), dict(scale=None), dict(counts=None), dict(workspace=None), dict(n=0), dict(n=2 ** 31), dict(C=0),
              dict(C=65537), dict(C=17), dict(ld=9), dict(scale_len=2), dict(scale_len=0), dict(logits=L.ptr(z) + 2), dict(labels=L.ptr(y) + 4),
              dict(workspace=L.ptr(ws) + 8), dict(workspace_bytes=64), dict(counts=L.ptr(counts) + 4))
    for bad in shared + (dict(F=None), dict(dscale=None), dict(dshift=None), dict(F=L.ptr(F) + 4), dict(dscale=L.ptr(ds) + 2)):
        assert call(lib.uvc_calib_eval, **bad) != 0, bad
    for bad in shared + (dict(bins=0), dict(bins=65), dict(bin_count=None), dict(bin_conf=None), dict(bin_hit=None), dict(sums=None), dict(sums=L.ptr(sums) + 4)):
        assert call(lib.uvc_calib_stats, **bad) != 0, bad
    assert call(lib.uvc_calib_eval, C=65537, ld=65540) == 3 and call(lib.uvc_calib_eval, n=0) == 1      # UVC_ERR_UNSUPPORTED, UVC_ERR_ARG
    assert lib.uvc_calib_eval(None, st) != 0 and lib.uvc_calib_stats(None, st) != 0
    nb = C.c_int64(-1)
    for bad in ((0, ld, Cc, 0), (n, 8, Cc, 0), (n, ld, 0, 0), (n, ld, 65537, 0), (n, ld, Cc, 65), (n, ld, Cc, -1)):
        assert lib.uvc_calib_workspace_bytes(*bad, C.byref(nb)) != 0 and nb.value == -1
    assert lib.uvc_calib_blocks(0, ld, C.byref(nb)) != 0 and lib.uvc_calib_blocks(n, 0, C.byref(nb)) != 0 and lib.uvc_calib_blocks(n, ld, None) != 0
    torch.cuda.synchronize()
    assert torch.isnan(F).all() and torch.isnan(ds).all() and torch.isnan(dd).all() and torch.isnan(bc).all() and torch.isnan(sums).all()
    assert counts.tolist() == [-7, -7] and bool((bn == -7).all()) and bool((bh == -7).all())
    assert call(lib.uvc_calib_eval) == 0 and call(lib.uvc_calib_eval, shift=None) == 0
    torch.cuda.synchronize()
    assert counts.tolist()[1] == n and not torch.isnan(ds).any() and not torch.isnan(dd).any() and not torch.isnan(F).any()
    assert call(lib.uvc_calib_stats) == 0
    torch.cuda.synchronize()
    assert int(bn.sum()) == n and not torch.isnan(sums).any()


# ---- reliability ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["normal", "huge"])
@pytest.mark.parametrize("Cc,ld", CR.WIDTHS)
def test_calib_stats_against_the_reference(Cc, ld, kind):
    """Bin counts and hits exact over the rows ``calib_ref.bin_ranges`` decides (a confidence farther than 1e-6 from an interior bin edge, a
    first maximum that leads by the margin; at most 1 % of the rows are undecided), the counts over all rows sum to m; sum_conf (per bin
    where every row is decided, and in total), nll and brier within 1e-5 relative.  Every row count and bin count, the modes in turn."""
    worst = 0.0
    for rows in CR.ROWS:
        z, y = CR.case_inputs(rows, Cc, ld, kind, seed=CR.case_seed(rows, Cc))
        maps = CR.case_maps(Cc, kind, seed=CR.case_seed(rows, Cc))
        zd = z.cuda()
        for i, bins in enumerate((1, 10, 15, 64)):
            mode = CR.MODES[(i + rows) % 4]
            scale, shift = maps[mode]
            yd = y.cuda() if i % 2 == 0 else y.to(torch.int32).cuda()
            ref = CC.reference_reliability(z, y, scale, shift, Cc, bins)
            lo, hi, hlo, hhi, undecided = CR.bin_ranges(z, y, scale, shift, Cc, bins)
            assert undecided <= CR.CAP * rows, (Cc, ld, rows, bins, undecided)
            n, c, h, sums, counts = (t.cpu() for t in ops.calib_stats(zd, yd, scale.cuda(), None if shift is None else shift.cuda(), Cc, bins))
            tag = (Cc, ld, kind, rows, bins, mode)
            assert bool((lo <= n).all()) and bool((n <= hi).all()) and bool((hlo <= h).all()) and bool((h <= hhi).all()), (tag, n.tolist(), lo.tolist())
            assert int(n.sum()) == ref["m"] == int(counts[1]) and int(h.sum()) == int(counts[0]), tag
            close = lambda got, want: abs(got - want) <= 1e-5 * abs(want) if want else abs(got) <= 1e-12
            if undecided == 0:
                assert all(close(float(c[j]), float(ref["bin_conf"][j])) for j in range(bins)), (tag, c.tolist(), ref["bin_conf"].tolist())
                assert torch.equal(n, ref["bin_count"]) and torch.equal(h, ref["bin_hit"]), tag
            assert close(float(c.sum()), float(ref["bin_conf"].sum())) and close(float(sums[0]), ref["nll_sum"]) and close(float(sums[1]), ref["brier_sum"]), \
                (tag, float(c.sum()), float(ref["bin_conf"].sum()), sums.tolist(), ref["nll_sum"], ref["brier_sum"])
            for got, want in ((float(c.sum()), float(ref["bin_conf"].sum())), (float(sums[0]), ref["nll_sum"]), (float(sums[1]), ref["brier_sum"])):
                if want:
                    worst = max(worst, abs(got - want) / abs(want))
            again = ops.calib_stats(zd, yd, scale.cuda(), None if shift is None else shift.cuda(), Cc, bins)
            assert all(same_bits(u.cpu(), v) for u, v in zip(again, (n, c, h, sums, counts))), tag
    print(f"calib_stats {kind} C={Cc} ld={ld}: worst relative error of sum_conf / nll / brier {worst:.2e}")


def test_device_scorer_is_the_reference_record():
    Z, y = CR.synthetic_bank()
    for scale, shift in ((torch.ones(1), None), (CR.optimum("vector")["scale"], CR.optimum("vector")["shift"])):
        got, want = CC.device_scorer(Z, y, scale, shift, 10, 15), CC.reference_scorer(Z, y, scale.float(), None if shift is None else shift.float(), 10, 15)
        assert got["bin_count"] == want["bin_count"] and got["rows"] == want["rows"] and got["top1"] == want["top1"]
        for k in ("ece", "mce", "nll", "brier"):
            assert abs(got[k] - want[k]) <= 1e-5 * max(want[k], 1e-3), (k, got[k], want[k])


# ---- the fit ------------------------------------------------------------------------------------------------------------------------------
FLOOR_MARGIN = 1.0                                  # times 2^-23 F*: the float32 resolution of the objective; the measured gaps lie far below it (README "Calibrate")


@pytest.mark.parametrize("method", CC.METHODS)
def test_fit_against_the_same_solver_on_the_cpu(method):
    """F64(theta_device) - F* against the same gap of the same solver on the CPU with float32 masters and a float64 evaluator rounded to
    float32, F* the float64 optimum (gradient below 1e-10): at most twice the CPU arm's gap, or the floor FLOOR_MARGIN 2^-23 F* at the
    float32 resolution of the objective.  Measured: see the README's calibration section."""
    Z, y = CR.synthetic_bank()
    opt = CR.optimum(method)
    gap = lambda r: CC.reference_objective(Z, y, r["scale"].double(), None if r["shift"] is None else r["shift"].double(), 10)[0] - opt["F"]
    ref = CC.fit_calibration(Z, y, 10, method, evaluator=CR.Float32Evaluator())
    dev = CC.fit_calibration(Z, y, 10, method)
    g_ref, g_dev = gap(ref), gap(dev)
    floor = FLOOR_MARGIN * 2.0 ** -23 * opt["F"]
    print(f"fit {method}: device gap {g_dev:.3e} ({dev['iterations']} iterations, {dev['evaluations']} evaluations), CPU float32 gap {g_ref:.3e} "
          f"({ref['iterations']} iterations, {ref['evaluations']} evaluations), F* {opt['F']:.6f}, floor {floor:.3e}")
    assert g_dev > -1e-12 and g_ref > -1e-12
    assert g_dev <= max(2 * g_ref, floor), (g_dev, g_ref, floor)
    assert dev["scale"].dtype == torch.float32 and dev["rows"] == 4000 and abs(dev["F"] - (g_dev + opt["F"])) <= 1e-3 * opt["F"]
    if method == "temperature":
        assert abs(dev["temperature"] / 2.5 - 1) <= 0.05 and dev["top1"] == opt["top1"]
    chunked = CC.fit_calibration(Z, y, 10, method, chunk_rows=1500)
    assert gap(chunked) <= max(2 * g_ref, floor)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_command(tmp_path, capsys, prec):
    """logits, fit (both methods) and score on three flat-coloured classes through the CIFAR-10 reader: the written file, run by
    CompactVisionTransformer on the same images, gives ``a * logits(F) + d`` within the bar test_compact_gpu.py holds eval logits to (1e-3 /
    2e-2 of the largest logit); ``logits`` on it followed by ``score`` prints the "after" record within that bar's effect; ``predict``
    takes the file as it is."""
    from PIL import Image
    from uvc_amd import data
    bar = {"fp32": 1e-3, "bf16": 2e-2}[prec]
    ex, _ = KR.export_of("stage2_micro_deit")
    train, test = KR.colour_images(30, 1), KR.colour_images(12, 2)
    root = KR.write_cifar10(str(tmp_path / "data"), train, test)
    torch.save(ex, tmp_path / "f.pt")
    f = str(tmp_path / "f.pt")
    bank = {s: str(tmp_path / f"z_{s}.pt") for s in ("train", "test")}
    dflags = ["--dataset", "cifar10", "--data_dir", root, "--eval_batch_size", "8", "--num_workers", "2", "--precision", prec]
    capsys.readouterr()
    for split, n in (("train", 30), ("test", 12)):
        s = CC.main(["logits", "--compact", f, "--split", split, "--output", bank[split]] + dflags)
        assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == s
        assert (s["images"], s["data_classes"], s["num_classes"]) == (n, 10, 16)
    b = CC.load_logits_bank(bank["train"])
    assert tuple(b["logits"].shape) == (30, 16) and torch.equal(b["labels"], torch.from_numpy(train[1])) and b["meta"]["precision"] == prec
    ns = argparse.Namespace(dataset="cifar10", data_dir=root, img_size=ex["cfg"]["img_size"], eval_batch_size=8, num_workers=2, interpolation="bilinear",
                            crop_pct=None, packed_dir=None, resident=0)
    images = torch.cat([x for x, _ in data.build_eval_loader(ns, "train")[0]])
    want = CP.reference_forward(ex, images.cpu().double())
    top = float(want.abs().max())
    assert float((b["logits"].double() - want).abs().max()) <= bar * top                    # the bank holds forward's eval logits: the two heads' mean
    for method in CC.METHODS:
        g = str(tmp_path / f"g_{method}.pt")
        args = CC.build_parser().parse_args(["fit", "--compact", f, "--bank", bank["train"], "--val_bank", bank["test"], "--method", method, "--output", g])
        line, res = CC.fit_command(args)
        json.dumps(line)
        assert (line["data_classes"], line["num_classes"], line["rows"], line["before"]["val"]["rows"]) == (10, 16, 30, 12)
        assert line["after"]["fit"]["nll"] <= line["before"]["fit"]["nll"] + 1e-9 and ("temperature" in line) == (method == "temperature")
        a = res["scale"].double().expand(10)
        d = torch.zeros(10, dtype=torch.float64) if res["shift"] is None else res["shift"].double()
        cm = CP.CompactVisionTransformer(CP.load_compact(g), precision=prec)
        got = cm(images)[0].double().cpu()
        mapped = b["logits"].double().clone()
        mapped[:, :10] = mapped[:, :10] * a + d
        scale_top = float(mapped.abs().max())
        assert float((got - mapped).abs().max()) <= bar * scale_top, (method, float((got - mapped).abs().max()), scale_top)
        # logits on G, then score: the "after" record, as far as the logits agree
        zg = str(tmp_path / f"zg_{method}.pt")
        CC.main(["logits", "--compact", g, "--split", "train", "--output", zg] + dflags)
        capsys.readouterr()
        score = CC.main(["score", "--bank", zg])
        assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == score
        tol = 2 * bar * scale_top
        after = line["after"]["fit"]
        assert abs(score["nll"] - after["nll"]) <= tol and abs(score["brier"] - after["brier"]) <= tol, (method, score["nll"], after["nll"], tol)
        assert abs(score["ece"] - after["ece"]) <= tol + 2 / 30 and score["rows"] == 30      # (an image that changes its bin moves the ECE by at most 2 / n)
    # temperature through main: the printed line
    g = str(tmp_path / "g_main.pt")
    line = CC.main(["fit", "--compact", f, "--bank", bank["train"], "--val_fraction", "0.2", "--output", g])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == line
    assert set(line) >= {"output", "method", "temperature", "data_classes", "num_classes", "rows", "evaluations", "seconds", "before", "after", "blocks",
                         "params", "macs_compact"} and line["rows"] == 24 and line["after"]["val"]["rows"] == 6 and line["temperature"] > 0
    # predict takes the calibrated file unchanged
    files = []
    for i in range(3):
        Image.fromarray(train[0][i]).save(tmp_path / f"{i}.png")
        files.append(str(tmp_path / f"{i}.png"))
    summary = CP.main(["predict", "--compact", g, "--images", *files, "--batch_size", "3", "--precision", prec, "--num_workers", "2", "--topk", "3",
                       "--output", str(tmp_path / "preds.jsonl")])
    assert summary["images"] == 3 and summary["errors"] == 0
    preds = [json.loads(l) for l in (tmp_path / "preds.jsonl").read_text().splitlines()][:3]
    assert [r["file"] for r in preds] == files and all(len(r["top"]) == 3 for r in preds)
