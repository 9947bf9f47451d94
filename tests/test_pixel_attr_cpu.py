"""CPU: the written spec of the pixel attributions (``compact_pixel.reference_input_grad`` / ``reference_integrated_gradients``) against finite
differences and against completeness, and the host side of ``python -m uvc_amd.compact_pixel``: flags, refusals, the record format."""
import json

import pytest
import torch

import pixel_attr_ref as PR
from oracle import vit as OV
from test_compact_cpu import dense_state
from uvc_amd import compact as CP
from uvc_amd import compact_pixel as PX


@pytest.mark.parametrize("name", ["no_heads", PR.LOW_BARE])
def test_reference_gradient_against_central_differences(name):
    """float64, h = 1e-4 on 24 seeded input coordinates per image, for the top-1 class and another one.  The central difference is off by
    h^2 / 6 |y'''| (1.7e-9 |y'''|) and by the rounding of y, about 1e-16 |y| / h = 1e-12 |y|: the bar, 1e-5 of the largest gradient entry,
    is three orders above both for any third derivative up to 1e3 times the gradient, and four below a wrong entry."""
    ex, x = PR.export_of(name)
    x = x[:2].double()
    nc = ex["cfg"]["num_classes"]
    g = torch.Generator().manual_seed(5)
    h = 1e-4
    for shift in (0, 3):
        _, t0, _ = PX.reference_input_grad(ex, x)
        t = (t0 + shift) % nc
        grad, t_out, logits = PX.reference_input_grad(ex, x, t)
        assert torch.equal(t_out, t) and grad.shape == x.shape and grad.dtype == torch.float64
        assert torch.equal(logits, CP.reference_forward(ex, x))
        y = lambda z: CP.reference_forward(ex, z).gather(1, t[:, None])[:, 0]
        idx = torch.randint(0, x[0].numel(), (24,), generator=g)
        worst = 0.0
        for i in idx.tolist():
            d = torch.zeros_like(x).view(2, -1)
            d[:, i] = h
            d = d.view_as(x)
            fd = (y(x + d) - y(x - d)) / (2 * h)
            worst = max(worst, float((fd - grad.view(2, -1)[:, i]).abs().max()))
        print(f"{name} shift {shift}: max |fd - grad| {worst:.2e}, max |grad| {float(grad.abs().max()):.2e}")
        assert worst <= 1e-5 * float(grad.abs().max())
    if name == "no_heads":
        assert torch.equal(PX.reference_input_grad(ex, x)[1], CP.reference_forward(ex, x).argmax(1))
        assert torch.equal(PX.reference_input_grad(ex, x, None, 4)[1], CP.reference_forward(ex, x)[:, :4].argmax(1))
        for bad in (-1, nc, [0, 1, 2]):
            with pytest.raises(ValueError):
                PX.reference_input_grad(ex, x, bad)


def test_reference_ig_completeness_gap_shrinks_with_the_steps():
    """|sum IG - (y(x) - y(x0))| is the midpoint rule's error: it falls from S = 4 to 16 to 64, for the zero and for a colour baseline; at
    S = 64 it is below 2 % of the largest logit."""
    ex, x = PR.export_of("no_heads")
    x = x.double()
    for baseline in (None, torch.tensor([-0.5, 0.25, 1.0], dtype=torch.float64)):
        gaps = []
        for S in (4, 16, 64):
            ig, t, y, y0 = PX.reference_integrated_gradients(ex, x, None, None, baseline, S)
            assert ig.shape == x.shape and torch.equal(t, CP.reference_forward(ex, x).argmax(1))
            assert torch.equal(y, CP.reference_forward(ex, x).gather(1, t[:, None])[:, 0])
            x0 = torch.zeros_like(x) if baseline is None else baseline.view(1, 3, 1, 1).expand_as(x)
            assert torch.equal(y0, CP.reference_forward(ex, x0.contiguous()).gather(1, t[:, None])[:, 0])
            gaps.append(float((ig.sum((1, 2, 3)) - (y - y0)).abs().max()))
        print("completeness gaps", gaps)
        assert gaps[0] > gaps[1] > gaps[2] and gaps[2] <= 2e-2 * float(CP.reference_forward(ex, x).abs().max())
    # a whole-batch baseline equal to the colour gives the same bits; steps and baseline are checked
    a = PX.reference_integrated_gradients(ex, x, None, None, baseline, 4)[0]
    b = PX.reference_integrated_gradients(ex, x, None, None, baseline.view(1, 3, 1, 1).expand_as(x), 4)[0]
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        PX.reference_integrated_gradients(ex, x, steps=0)
    with pytest.raises(ValueError):
        PX.reference_integrated_gradients(ex, x, baseline=torch.zeros(4))


def test_parser_flags_and_refusals(capsys):
    p = PX.build_parser()
    a = p.parse_args(["--compact", "m.pt", "--images", "a", "b", "--method", "ig"])
    assert (a.method, a.steps, a.baseline, a.target, a.output, a.overlay_dir, a.pixel_dir) == ("ig", 32, "mean", None, None, None, None)
    assert (a.topk, a.batch_size, a.num_workers, a.precision, a.preset, a.interpolation, a.crop_pct, a.classes, a.num_labels) == \
        (5, 64, 8, "bf16", "imagenet", "bilinear", None, None, None)
    a = p.parse_args(["--compact", "m.pt", "--images", "a", "--method", "saliency", "--steps", "7", "--baseline", "black", "--target", "3",
                      "--output", "o.jsonl", "--overlay_dir", "ov", "--pixel_dir", "px", "--preset", "cifar", "--num_labels", "10"])
    assert (a.method, a.steps, a.baseline, a.target, a.output, a.overlay_dir, a.pixel_dir, a.preset, a.num_labels) == \
        ("saliency", 7, "black", 3, "o.jsonl", "ov", "px", "cifar", 10)
    for bad in (["--method", "rollout"], ["--method", "ig", "--steps", "0"], ["--method", "ig", "--baseline", "white"], ["--method", "ig", "--target", "-1"],
                [], ["--method", "ig", "--fused_input", "1"]):
        with pytest.raises(SystemExit):
            p.parse_args(["--compact", "m.pt", "--images", "a", *bad])
    with pytest.raises(SystemExit):
        p.parse_args(["--images", "a", "--method", "ig"])
    capsys.readouterr()
    assert PX.METHODS == ("saliency", "gradxinput", "ig") and PX.BASELINES == ("mean", "black")
    with pytest.raises(ValueError):
        PX.check_method("attribution")
    with pytest.raises(ValueError):
        PX.check_method("ig", 0)
    with pytest.raises(ValueError):
        PX.check_method("ig", 8, "grey")
    for steps, chunk in ((0, None), (8, 0), (8, -2)):
        with pytest.raises(ValueError):
            PX._check_steps(steps, chunk)
    assert PX._check_steps(8, 3) == (8, 3) and PX._check_steps(8, 50) == (8, 8) and PX._check_steps(8, None) == (8, None)
    black = PX.black_baseline("imagenet")
    assert black.shape == (3,) and abs(float(black[0]) + 0.485 / 0.229) < 1e-6 and PX.black_baseline("cifar").tolist() == [-1.0, -1.0, -1.0]


def test_record_format():
    top = [dict(index=3, label=None, prob=0.5)]
    rec = PX.record_of("a.png", top, 3, 2, [1.0, 3.0, 0.0, 4.0])
    assert rec == dict(file="a.png", top=top, target=3, grid=[2, 2], map=[0.125, 0.375, 0.0, 0.5])
    assert json.loads(json.dumps(rec)) == rec
    rec = PX.record_of("a.png", top, 3, 2, [1.0, 3.0, 0.0, 4.0], ig=(2.5, 0.5, 1.75))
    assert set(rec) == {"file", "top", "target", "grid", "map", "y", "y_baseline", "delta"}
    assert (rec["y"], rec["y_baseline"], rec["delta"]) == (2.5, 0.5, -0.25)
    assert PX.record_of("a.png", top, 0, 1, [0.0])["map"] == [0.0]          # an all-zero map stays zeros
    # the map goes into compact_perturb's score check as it is: [B, np] over the patches
    from uvc_amd import compact_perturb as PT
    maps, offset = PT._patch_scores(torch.tensor([rec["map"]]), 1, 4, 2)
    assert offset == 0


def test_more_than_256_tokens_fail_before_any_image_is_listed(tmp_path):
    cfg = OV.VitConfig(img_size=384, patch_size=16, num_classes=16, embed_dim=64, depth=2, num_heads=1, enable_dist=0)
    big = tmp_path / "big.compact.pt"
    ex = CP.export_compact(dense_state(cfg))
    torch.save(ex, big)
    with pytest.raises(NotImplementedError, match="256"):
        PX.check_tokens(ex)
    for method in PX.METHODS:
        with pytest.raises(NotImplementedError, match="256"):
            PX.main(["--compact", str(big), "--images", "/nonexistent/dir", "--method", method, "--precision", "fp32"])
    PX.check_tokens(PR.export_of("px224")[0])
