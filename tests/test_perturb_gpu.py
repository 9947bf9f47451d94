"""GPU: the perturbation test of relevance maps -- the three kernels of uvc_amd/csrc/perturb.hip at the smallest shapes at which each can still
go wrong (uvc_patch_rank against the lexsort statement of its rule, uvc_patch_rows_perturb bit for bit against torch.where on both of its code
paths and past 2^31 bytes, uvc_logits_target against float64), their refusals, ``perturbation_curves`` against ``reference_perturbation`` on the
same float32 maps, and ``python -m uvc_amd.compact_perturb`` end to end."""
import json

import numpy as np
import pytest
import torch
from PIL import Image

import perturb_ref as PR
from uvc_amd import _lib as L
from uvc_amd import compact as CP
from uvc_amd import compact_perturb as PT
from uvc_amd import ops
from uvc_amd.compact_attribution import CompactAttributionViT

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


# ---- uvc_patch_rank ------------------------------------------------------------------------------------------------------------------------
def score_family(which, B, n, g):
    """float32 [B, n] on the host.  0: distinct random; 1: all equal; 2: three values, many ties; 3: with +-0, +-inf and NaN"""
    if which == 0:
        return torch.randn(B, n, generator=g)
    if which == 1:
        return torch.full((B, n), 0.25)
    if which == 2:
        return torch.randint(0, 3, (B, n), generator=g).float() - 1.0
    special = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1.0, -1.0, float("nan"), 1e-45, -1e-45])
    pick = torch.randint(0, 2 * len(special), (B, n), generator=g)
    return torch.where(pick < len(special), special[pick % len(special)], torch.randn(B, n, generator=g))


@pytest.mark.parametrize("B,np_", [(1, 1), (3, 2), (2, 63), (2, 64), (2, 65), (2, 196), (1, 576), (2, 1023), (2, 1024)])
def test_rank_is_the_lexsort_rank(B, np_):
    """Exact equality with ``rank_reference`` in both directions, with the patches at column 0, 1 and 2 of a wider row, for every score family;
    every row is a permutation.  Sizes: one patch, below / at / past a wave, the DeiT grids, and the limit with one patch less."""
    g = torch.Generator().manual_seed(100 * np_ + B)
    for which in range(4):
        for offset in (0, 1, 2):
            ld = offset + np_ + (3 if offset else 0)
            s = score_family(which, B, ld, g)
            dev = s.cuda()
            for descending in (True, False):
                got = ops.patch_rank(dev, offset, descending, np_).cpu().numpy()
                want = PT.rank_reference(s[:, offset:offset + np_], descending)
                assert got.dtype == np.int32 and got.shape == (B, np_)
                assert np.array_equal(np.sort(got, axis=1), np.tile(np.arange(np_, dtype=np.int32), (B, 1))), (which, offset, descending)
                assert np.array_equal(got, want), (which, offset, descending)
                if which == 1:
                    assert np.array_equal(got[0], np.arange(np_))
    full = ops.patch_rank(torch.randn(2, np_ + 1, generator=g).cuda(), 1)            # the default np: the rest of the row
    assert tuple(full.shape) == (2, np_)


def test_rank_of_an_image_does_not_depend_on_the_batch():
    g = torch.Generator().manual_seed(7)
    for np_ in (65, 196, 1024):
        s = score_family(3, 3, np_ + 2, g).cuda()
        for descending in (True, False):
            three = ops.patch_rank(s, 2, descending)
            one = ops.patch_rank(s[:1].contiguous(), 2, descending)
            again = ops.patch_rank(s, 2, descending)
            assert torch.equal(three[:1], one) and torch.equal(three, again)


# ---- uvc_patch_rows_perturb ----------------------------------------------------------------------------------------------------------------
def counts_for(np_, nsteps, g):
    if nsteps == 1:
        return [np_ // 2]
    return [0, np_] + torch.randint(0, np_ + 1, (nsteps - 2,), generator=g).tolist()


def expected_rows(rows, rank, counts, B, np_):
    keep = rank.view(1, B, np_, 1) >= torch.as_tensor(counts, dtype=torch.int32, device=rows.device).clamp(0, np_).view(-1, 1, 1, 1)
    return torch.where(keep, rows.view(1, B, np_, -1), torch.zeros((), dtype=rows.dtype, device=rows.device)).reshape(-1, rows.shape[1])


def same_bits(a, b):
    return torch.equal(a.view(BITS[a.dtype]), b.view(BITS[b.dtype]))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("width", [3, 12, 48, 768])
def test_perturbed_rows_are_torch_where_bit_for_bit(width, prec):
    """Widths of patch sizes 1, 2, 4 and 16: 3 and 12 float32 / bf16 elements are 12, 6 and 24 bytes a row (element by element), 48 bf16 and
    everything above are whole 16-byte chunks.  Into a NaN-prefilled output: every element is written, by its one writer."""
    dt = DT[prec]
    g = torch.Generator().manual_seed(width)
    for np_ in (1, 4, 196):
        for B in (1, 3):
            rows = torch.randn(B * np_, width, generator=g).to(dt).cuda()
            rank = torch.stack([torch.randperm(np_, generator=g) for _ in range(B)]).int().cuda()
            for nsteps in (1, 10):
                counts = counts_for(np_, nsteps, g)
                out = torch.full((nsteps * B * np_, width), float("nan"), dtype=dt, device="cuda")
                got = ops.perturb_rows(rows, rank, torch.tensor(counts, dtype=torch.int32, device="cuda"), B, np_, out=out)
                assert got is out and not torch.isnan(out).any(), (np_, B, nsteps)
                assert same_bits(out, expected_rows(rows, rank, counts, B, np_)), (np_, B, nsteps)
    # a removed row is selected, not multiplied: NaN and inf under removed ranks give exact +0 (all bits zero), in every step
    np_, B = 196, 3
    rows = torch.randn(B * np_, width, generator=g).to(dt).cuda()
    rank = torch.stack([torch.randperm(np_, generator=g) for _ in range(B)]).int().cuda()
    poison = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0], dtype=dt, device="cuda")
    low = (rank.view(-1) < 40).nonzero().flatten()
    rows[low] = poison[torch.arange(len(low), device="cuda") % 4][:, None].expand(-1, width)
    counts = [40, 41, np_, 117]
    out = ops.perturb_rows(rows, rank, torch.tensor(counts, dtype=torch.int32, device="cuda"), B, np_,
                           out=torch.full((4 * B * np_, width), float("nan"), dtype=dt, device="cuda"))
    assert not torch.isnan(out).any() and not torch.isinf(out).any()
    assert int((out.view(4, B * np_, width)[:, low].view(BITS[dt]) != 0).sum()) == 0
    assert same_bits(out, expected_rows(rows, rank, counts, B, np_))
    # a count outside [0, np] is clamped on the device
    wild = ops.perturb_rows(rows, rank, torch.tensor([-5, np_ + 7, 1 << 30, -(1 << 31)], dtype=torch.int32, device="cuda"), B, np_)
    assert same_bits(wild, expected_rows(rows, rank, [0, np_, np_, 0], B, np_))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_perturbed_rows_off_alignment_take_the_element_path(prec):
    """Rows of whole 16-byte chunks behind a base pointer that is one element off: the host picks the element-wise path (a 16-byte access there
    would be misaligned), for the source, for the output, and for both."""
    dt = DT[prec]
    g = torch.Generator().manual_seed(3)
    B, np_, width, counts = 3, 4, 48, [0, 2, 4, 1]
    rank = torch.stack([torch.randperm(np_, generator=g) for _ in range(B)]).int().cuda()
    cd = torch.tensor(counts, dtype=torch.int32, device="cuda")
    src = torch.randn(B * np_ * width + 1, generator=g).to(dt).cuda()
    for off_rows, off_out in ((1, 0), (0, 1), (1, 1)):
        rows = src[off_rows:off_rows + B * np_ * width].view(B * np_, width)
        base = torch.full((4 * B * np_ * width + 1,), float("nan"), dtype=dt, device="cuda")
        out = base[off_out:off_out + 4 * B * np_ * width].view(4 * B * np_, width)
        assert rows.data_ptr() % 16 == (off_rows * src.element_size()) % 16 and out.data_ptr() % 16 == (off_out * src.element_size()) % 16
        ops.perturb_rows(rows, rank, cd, B, np_, out=out)
        assert not torch.isnan(out).any() and same_bits(out, expected_rows(rows, rank, counts, B, np_))
        if off_out:
            assert bool(torch.isnan(base[:1]).all())                      # the element before the output is not touched


def test_perturbed_rows_past_two_gib():
    """10 steps x 384 images x 196 patches x 768 float32: 2.3 GB of output, byte offsets past 2^31 from the fifth step on."""
    B, np_, width, nsteps = 384, 196, 768, 10
    g = torch.Generator(device="cuda").manual_seed(5)
    rows = torch.randn(B * np_, width, device="cuda", generator=g)
    rank = ops.patch_rank(torch.rand(B, np_, device="cuda", generator=g))
    counts = PT.step_counts(np_, nsteps)
    out = torch.full((nsteps * B * np_, width), float("nan"), device="cuda")
    assert out.numel() * 4 > 1 << 31
    ops.perturb_rows(rows, rank, torch.tensor(counts, dtype=torch.int32, device="cuda"), B, np_, out=out)
    steps = out.view(nsteps, B * np_, width)
    assert torch.equal(steps[0].view(torch.int32), rows.view(torch.int32))           # count 0: the rows themselves
    last = expected_rows(rows, rank, counts[-1:], B, np_)
    assert torch.equal(steps[-1].view(torch.int32), last.view(torch.int32))
    sample = torch.arange(0, B * np_, 97, device="cuda")
    want = expected_rows(rows[sample], rank.view(-1)[sample].view(1, -1), counts, 1, len(sample))
    assert torch.equal(steps[:, sample].reshape(-1, width).view(torch.int32), want.view(torch.int32))
    assert not torch.isnan(steps[:, B * np_ - 1]).any() and not torch.isnan(steps[nsteps // 2]).any()


# ---- uvc_logits_target ---------------------------------------------------------------------------------------------------------------------
def target_reference(logits, target, n_valid):
    z = logits.cpu().numpy().astype(np.float64)[:, :n_valid]
    t = np.clip(np.resize(target.cpu().numpy(), len(z)), 0, n_valid - 1)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    return p[np.arange(len(z)), t], (z.argmax(axis=1) == t).astype(np.int32)


@pytest.mark.parametrize("ld,n_valid", [(16, 10), (104, 100), (1000, 1000)])
@pytest.mark.parametrize("rows,period", [(1, 1), (7, 7), (7, 1), (640, 64)])
def test_target_probability_against_float64(rows, period, ld, n_valid):
    g = torch.Generator().manual_seed(rows * 1000 + ld)
    logits = 3.0 * torch.randn(rows, ld, generator=g)
    logits[:, n_valid:] = 100.0                                   # the padding columns take no part
    if rows >= 7:
        # rows 1 and 2: one logit far from the rest (+-40: every probability stays a normal float32); row 3: -80 everywhere and +80 at its
        # target; row 4: +80 everywhere (nothing overflows once the maximum is subtracted; every column is a maximum, the first one counts)
        logits[1, 0], logits[2, n_valid - 1], logits[3, :n_valid] = 40.0, -40.0, -80.0
        logits[3, n_valid // 2], logits[4, :n_valid] = 80.0, 80.0
    target = torch.randint(0, n_valid, (period,), generator=g).int()
    if rows >= 7:
        target[3 % period] = n_valid // 2
    prob, hit = ops.logits_target(logits.cuda(), target.cuda(), n_valid)
    want_p, want_h = target_reference(logits, target, n_valid)
    rel = np.abs(prob.cpu().numpy().astype(np.float64) - want_p) / want_p
    print(f"uvc_logits_target rows={rows} period={period} n_valid={n_valid}: worst relative error {rel.max():.3e}")
    assert prob.dtype == torch.float32 and hit.dtype == torch.int32 and float(rel.max()) <= 1e-5
    assert np.array_equal(hit.cpu().numpy(), want_h)
    again = ops.logits_target(logits.cuda(), target.cuda(), n_valid)
    assert torch.equal(again[0].view(torch.int32), prob.view(torch.int32)) and torch.equal(again[1], hit)
    # the probability of the top-1 label is uvc_logits_topk's, bit for bit (the same trees)
    top_p, top_i = ops.logits_topk(logits.cuda(), 1, n_valid)
    p1, h1 = ops.logits_target(logits.cuda()[:1].contiguous(), top_i[:1, 0].contiguous(), n_valid)
    assert torch.equal(p1.view(torch.int32), top_p[:1, 0].view(torch.int32)) and h1.tolist() == [1]


def test_target_hit_is_the_first_maximum_and_targets_are_clamped():
    logits = torch.zeros(6, 16)
    logits[:, 3], logits[:, 7], logits[:, 12] = 2.5, 2.5, 9.0     # two equal maxima among the 10 labels; column 12 is padding
    target = torch.tensor([3, 7, 0, -3, 1 << 20, 9], dtype=torch.int32)
    prob, hit = ops.logits_target(logits.cuda(), target.cuda(), 10)
    assert hit.tolist() == [1, 0, 0, 0, 0, 0]
    want_p, _ = target_reference(logits, target, 10)              # (the reference clamps as the kernel does: -3 -> 0, 2^20 -> 9)
    assert np.allclose(prob.cpu().numpy(), want_p, rtol=1e-5, atol=0)
    assert prob[0] == prob[1] and prob[3] == prob[2] and prob[4] == prob[5]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone():
    lib, st = L.lib(), L.cur_stream()
    scores = torch.zeros(2, 20, device="cuda")
    rank = torch.full((2, 16), -7, dtype=torch.int32, device="cuda")
    r = lambda **k: lib.uvc_patch_rank(*[{**dict(scores=L.ptr(scores), B=2, ld=20, offset=2, np=16, descending=1, rank=L.ptr(rank), stream=st), **k}[n]
                                         for n in ("scores", "B", "ld", "offset", "np", "descending", "rank", "stream")])
    assert r(scores=None) == 1 and r(rank=None) == 1 and r(B=0) == 1 and r(B=-1) == 1
    assert r(np=0) == 1 and r(np=-3) == 1 and r(offset=-1) == 1 and r(offset=5) == 1 and r(np=19) == 1
    assert r(np=1025, ld=2000) == 3 and b"1024" in lib.uvc_last_error()
    rows = torch.ones(2 * 16, 48, device="cuda")
    counts = torch.zeros(3, dtype=torch.int32, device="cuda")
    out = torch.full((3 * 2 * 16, 48), float("nan"), device="cuda")
    good = ops.patch_rank(scores, 2, True, 16)
    p = lambda **k: lib.uvc_patch_rows_perturb(*[{**dict(rows=L.ptr(rows), rank=L.ptr(good), counts=L.ptr(counts), nsteps=3, B=2, np=16, width=48,
                                                         dtype=L.UVC_F32, out=L.ptr(out), stream=st), **k}[n]
                                                 for n in ("rows", "rank", "counts", "nsteps", "B", "np", "width", "dtype", "out", "stream")])
    assert p(rows=None) == 1 and p(rank=None) == 1 and p(counts=None) == 1 and p(out=None) == 1
    assert p(nsteps=0) == 1 and p(B=0) == 1 and p(width=0) == 1 and p(width=-48) == 1 and p(np=0) == 1
    assert p(np=1025) == 3 and p(dtype=2) == 1 and p(dtype=-1) == 1
    logits = torch.zeros(6, 16, device="cuda")
    target = torch.zeros(3, dtype=torch.int32, device="cuda")
    prob, hit = torch.full((6,), float("nan"), device="cuda"), torch.full((6,), -7, dtype=torch.int32, device="cuda")
    t = lambda **k: lib.uvc_logits_target(*[{**dict(logits=L.ptr(logits), rows=6, ld=16, n_valid=10, target=L.ptr(target), period=3, prob=L.ptr(prob),
                                                    hit=L.ptr(hit), stream=st), **k}[n]
                                            for n in ("logits", "rows", "ld", "n_valid", "target", "period", "prob", "hit", "stream")])
    assert t(logits=None) == 1 and t(target=None) == 1 and t(prob=None) == 1 and t(hit=None) == 1
    assert t(rows=0) == 1 and t(period=0) == 1 and t(period=4) == 1 and t(n_valid=0) == 1 and t(n_valid=17) == 1
    assert b"uvc_logits_target" in lib.uvc_last_error()
    torch.cuda.synchronize()
    assert rank.tolist() == [[-7] * 16] * 2 and bool(torch.isnan(out).all()) and bool(torch.isnan(prob).all()) and hit.tolist() == [-7] * 6
    assert r() == 0 and p() == 0 and t() == 0                       # and the same calls with nothing wrong run
    torch.cuda.synchronize()
    assert torch.equal(rank, good) and not torch.isnan(out).any() and not torch.isnan(prob).any()
    # the Python layer: wrong types and shapes never reach the library
    for bad in (lambda: ops.patch_rank(scores.double()), lambda: ops.patch_rank(scores[0]), lambda: ops.perturb_rows(rows, good.long(), counts, 2, 16),
                lambda: ops.perturb_rows(rows, good, counts, 2, 15), lambda: ops.perturb_rows(rows.half(), good, counts, 2, 16),
                lambda: ops.perturb_rows(rows, good, counts, 2, 16, out=out[:-1]), lambda: ops.logits_target(logits, target.long()),
                lambda: ops.logits_target(logits.double(), target), lambda: ops.patch_rank(scores.cpu())):
        with pytest.raises(L.UvcHipError):
            bad()


# ---- curves --------------------------------------------------------------------------------------------------------------------------------
_MODELS, WORST = {}, {}


def model_of(name, prec):
    """A module with an eval forward: the one with a backward where the file has at most 256 tokens, the inference module above"""
    if (name, prec) not in _MODELS:
        ex, _ = PR.export_of(name)
        _MODELS[name, prec] = (CP.CompactVisionTransformer if name == PR.BIG else CompactAttributionViT)(ex, precision=prec)
    return _MODELS[name, prec]


def check_curves(got, ref, prec, what):
    """prob within half the logit bar (a softmax entry moves by at most half the largest logit error); in float32 ``hit`` equal wherever the
    reference's margin exceeds twice the logit bar -- the target's logit against the best other, whichever of the two leads."""
    diff = (got["prob"].double().cpu() - ref["prob"]).abs()
    used = float((diff / PR.prob_bar(ref, prec)[None, :]).max())
    WORST[prec] = max(WORST.get(prec, 0.0), float(diff.max()))
    print(f"perturbation curves {what} {prec}: max |prob - ref| {float(diff.max()):.3e} ({used:.3f} of its bar); worst {prec} so far {WORST[prec]:.3e}")
    assert got["counts"] == ref["counts"] and got["prob"].dtype == torch.float32 and got["hit"].dtype == torch.int32
    assert used <= 1.0, (what, prec, used)
    if prec == "fp32":
        sure = PR.qualifying(ref, prec)
        assert float(sure.double().mean()) >= PR.QUALIFY
        assert torch.equal(got["hit"].cpu()[sure], ref["hit"][sure]), what


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name,kind", PR.CASES)
def test_curves_against_the_reference_on_the_same_maps(name, kind, prec):
    ex, x = PR.export_of(name)
    maps, target = PR.maps_of(name, kind)
    cm, nl = model_of(name, prec), PR.num_labels_of(name)
    for steps in PR.GRIDS:
        for order in PT.ORDERS:
            got = PT.perturbation_curves(cm, x.cuda(), maps.cuda(), target, order=order, steps=steps, num_labels=nl)
            assert tuple(got["prob"].shape) == tuple(got["hit"].shape) == (x.shape[0], steps)
            check_curves(got, PR.reference_of(name, kind, order, steps), prec, f"{name} {kind} {order} steps={steps}")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["stage2_micro_deit", "no_heads", "px224", PR.BIG])
def test_curve_identities(name, prec):
    ex, x = PR.export_of(name)
    kind = PR.KINDS[name][0]
    maps, target = PR.maps_of(name, kind)
    cm, nl = model_of(name, prec), PR.num_labels_of(name)
    c = ex["cfg"]
    B, npatch = x.shape[0], (c["img_size"] // c["patch_size"]) ** 2
    xd, md = x.cuda(), maps.cuda()
    pos = PT.perturbation_curves(cm, xd, md, target, num_labels=nl)
    # step 0 removes nothing: model.forward(patches=rows) bit for bit
    rows = torch.empty(B * npatch, c["in_chans"] * c["patch_size"] ** 2, dtype=DT[prec], device="cuda")
    ops.patchify(xd, rows, c["patch_size"], cm._cfg.dtype)
    p0, h0 = ops.logits_target(cm.forward(patches=rows)[0], target.int().cuda(), nl)
    assert torch.equal(pos["prob"][:, 0].contiguous().view(torch.int32), p0.view(torch.int32)) and torch.equal(pos["hit"][:, 0], h0)
    assert torch.equal(cm.forward(patches=rows)[0], cm.forward(xd)[0])
    # everything removed: the order does not matter; and a repeat gives the same bits
    full = [PT.perturbation_curves(cm, xd, md, target, order=o, counts=[npatch], num_labels=nl) for o in PT.ORDERS]
    assert torch.equal(full[0]["prob"].view(torch.int32), full[1]["prob"].view(torch.int32)) and torch.equal(full[0]["hit"], full[1]["hit"])
    check_curves(full[0], PR.reference_of(name, kind, "positive", 10, counts=[npatch]), prec, f"{name} all removed")
    again = PT.perturbation_curves(cm, xd, md, target, num_labels=nl)
    assert torch.equal(again["prob"].view(torch.int32), pos["prob"].view(torch.int32)) and torch.equal(again["hit"], pos["hit"])
    # maps over the patches alone are the same maps
    bare = PT.perturbation_curves(cm, xd, md[:, cm.num_tokens:], target, num_labels=nl)
    assert torch.equal(bare["prob"].view(torch.int32), pos["prob"].view(torch.int32))
    # three steps per forward (chunks of 3, 3, 3 and 1 steps): another batch size for the GEMMs, nothing beyond the bar
    wide = PT.perturbation_curves(cm, xd, md, target, num_labels=nl, max_images=3 * B)
    check_curves(wide, PR.reference_of(name, kind, "positive", 10), prec, f"{name} max_images=3B")
    if name == "no_heads":                                      # the inference module gives the curves of the module with a backward
        other = PT.perturbation_curves(CP.CompactVisionTransformer(ex, precision=prec), xd, md, target, num_labels=nl)
        assert torch.equal(other["prob"].view(torch.int32), pos["prob"].view(torch.int32)) and torch.equal(other["hit"], pos["hit"])
        for bad in (dict(order="up"), dict(counts=[npatch + 1]), dict(counts=[-1]), dict(max_images=B - 1), dict(num_labels=0)):
            with pytest.raises(ValueError):
                PT.perturbation_curves(cm, xd, md, target, **{"num_labels": nl, **bad})
        with pytest.raises(ValueError):
            PT.perturbation_curves(cm, xd, md, target + nl, num_labels=nl)
        with pytest.raises(ValueError):
            PT.perturbation_curves(cm, xd, md[:, 3:], target, num_labels=nl)
        with pytest.raises(L.UvcHipError):
            PT.perturbation_curves(cm, xd, maps, target, num_labels=nl)


# ---- the command, end to end ---------------------------------------------------------------------------------------------------------------
def test_command(tmp_path, capsys):
    ex, _ = PR.export_of("no_heads")
    model = tmp_path / "m.compact.pt"
    torch.save(ex, model)
    rng = np.random.default_rng(5)
    files = []
    for name, (h, w), mode in [("a.png", (31, 20), "RGB"), ("b.png", (64, 64), "L"), ("c.png", (45, 80), "RGBA"), ("d.png", (90, 120), "RGB")]:
        a = rng.integers(0, 256, (h, w) if mode == "L" else (h, w, len(mode)), dtype=np.uint8)
        Image.fromarray(a, mode).save(tmp_path / name)
        files.append(str(tmp_path / name))
    broken = tmp_path / "broken.png"
    broken.write_bytes(open(files[0], "rb").read()[:40])
    files.insert(2, str(broken))
    methods, steps = ["rollout", "last", "attribution", "random"], 5
    common = ["--compact", str(model), "--images", *files, "--batch_size", "3", "--precision", "fp32", "--num_workers", "2", "--num_labels", "10",
              "--methods", *methods, "--steps", str(steps)]

    def run(out, *extra):
        summaries = PT.main([*common, "--output", str(out), *extra])
        lines = [json.loads(l) for l in out.read_text().splitlines()]
        assert lines[-len(summaries):] == summaries
        return lines[:-len(summaries)], summaries

    recs, summaries = run(tmp_path / "curves.jsonl")
    pairs = [(m, o) for m in methods for o in PT.ORDERS]
    assert [(s["method"], s["order"]) for s in summaries] == pairs
    errs = [r for r in recs if "error" in r]
    assert len(errs) == 1 and set(errs[0]) == {"file", "error"} and errs[0]["file"] == str(broken) and errs[0]["error"]
    good = [f for f in files if f != str(broken)]
    for pair in pairs:
        mine = [r for r in recs if (r.get("method"), r.get("order")) == pair]
        assert [r["file"] for r in mine] == good
        for r in mine:
            assert set(r) == {"file", "method", "order", "target", "prob", "hit", "auc_prob"}
            assert len(r["prob"]) == len(r["hit"]) == steps and 0 <= r["target"] < 10 and r["hit"][0] == 1
            assert r["auc_prob"] == pytest.approx(PT.auc(r["prob"], steps), abs=1e-12) and all(0.0 <= q <= 1.0 for q in r["prob"])
    by_file = {f: [r for r in recs if r["file"] == f] for f in good}
    for f, rs in by_file.items():                                   # one target and one intact probability per image
        assert len(rs) == len(pairs) and len({r["target"] for r in rs}) == 1 and len({r["prob"][0] for r in rs}) == 1
    assert [r["file"] for r in recs if r["file"] != str(broken)][::len(pairs)] == good          # in input order, an image's records together
    for s in summaries:
        assert set(s) == {"method", "order", "images", "errors", "fractions", "mean_prob", "accuracy", "auc_prob", "auc_accuracy"}
        assert s["images"] == 4 and s["errors"] == 1 and s["fractions"] == [c / 16 for c in PT.step_counts(16, steps)]
        mine = [r for r in recs if (r.get("method"), r.get("order")) == (s["method"], s["order"])]
        assert s["mean_prob"] == pytest.approx(np.mean([r["prob"] for r in mine], axis=0).tolist(), abs=1e-12)
        assert s["accuracy"] == pytest.approx(np.mean([r["hit"] for r in mine], axis=0).tolist(), abs=1e-12) and s["accuracy"][0] == 1.0
        assert s["auc_prob"] == pytest.approx(PT.auc(s["mean_prob"], steps), abs=1e-12)
        assert s["auc_accuracy"] == pytest.approx(PT.auc(s["accuracy"], steps), abs=1e-12)
    assert len({s["mean_prob"][0] for s in summaries}) == 1           # the intact image is the same for every method and order
    # the targets are predict's top-1 labels
    pred_out = tmp_path / "preds.jsonl"
    CP.main(["predict", "--compact", str(model), "--images", *files, "--batch_size", "3", "--precision", "fp32", "--num_workers", "2", "--num_labels", "10",
             "--topk", "1", "--output", str(pred_out)])
    preds = {r["file"]: r for r in (json.loads(l) for l in pred_out.read_text().splitlines()[:-1])}
    for f in good:
        assert by_file[f][0]["target"] == preds[f]["top"][0]["index"]
        assert by_file[f][0]["prob"][0] == pytest.approx(preds[f]["top"][0]["prob"], rel=1e-6)
    # the random baseline is reproducible under one seed, and another seed is another order
    again, _ = run(tmp_path / "again.jsonl")
    assert again == recs
    other, _ = run(tmp_path / "other.jsonl", "--seed", "1")
    rand = lambda rs: [r["prob"] for r in rs if r.get("method") == "random"]
    assert rand(other) != rand(recs) and [r for r in other if r.get("method") != "random"] == [r for r in recs if r.get("method") != "random"]
    # --target: that class for every image
    given, _ = run(tmp_path / "given.jsonl", "--target", "4", "--methods", "rollout", "--orders", "positive")
    assert all(r["target"] == 4 for r in given if "target" in r) and len(given) == 5
    with pytest.raises(ValueError, match="target"):
        PT.main([*common, "--target", "10"])
    # the function, on an export and with a module set built by the caller
    mods = PT.build_modules(ex, ["random"], "fp32")
    assert mods["attribution"] is None and isinstance(mods["forward"], CP.CompactVisionTransformer)
    out = list(PT.evaluate(ex, files, methods=("random",), orders=("negative",), steps=steps, precision="fp32", batch_size=5, num_workers=2,
                           num_labels=10, modules=mods))
    assert len(out) == 4 + 1 + 1 and out[-1]["images"] == 4 and out[-1]["errors"] == 1 and [r["file"] for r in out[:-1]] == files
    assert isinstance(PT.build_modules(ex, ["attribution"], "fp32")["forward"], CompactAttributionViT)
    # more than 256 tokens with attribution among the methods fails before any file is listed, with the limit named; without it the file runs
    big_ex, _ = PR.export_of(PR.BIG)
    big = tmp_path / "big.compact.pt"
    torch.save(big_ex, big)
    with pytest.raises(NotImplementedError, match="256"):
        PT.main(["--compact", str(big), "--images", "/nonexistent/dir", "--precision", "fp32", "--methods", "rollout", "attribution"])
    with pytest.raises(FileNotFoundError):
        PT.main(["--compact", str(big), "--images", "/nonexistent/dir", "--precision", "fp32", "--methods", "rollout", "random"])
    capsys.readouterr()
