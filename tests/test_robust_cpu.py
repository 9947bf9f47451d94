"""CPU: the written spec of the robustness module -- ``reference_loss_grad`` against central finite differences in float64, ``linf_bounds``
against hand values, the invariants of ``reference_attack``, the default step, and the command's flags and refusals."""
import argparse

import pytest
import torch

import robust_ref as RR
from uvc_amd import compact_robust as RB
from uvc_amd import data

NAME = "stage2_micro_deit"


@pytest.mark.parametrize("loss", RB.LOSSES)
def test_reference_loss_grad_against_finite_differences(loss):
    """float64, h = 1e-5, 24 coordinates per image drawn once: the central difference of the image's OWN loss (its error is O(h^2) and the
    rounding of a float64 difference over 2 h, both far below the 1e-6 of the largest gradient entry asked for).  The labels are the
    reference's top-1, so the margin's j is the runner-up and stays it over +-h."""
    ex, x = RR.export_of(NAME)
    x = x.double()
    labels, gap, _ = RR.top_two(NAME)
    assert float(gap.min()) > 1e-3
    logits, grad, L = RB.reference_loss_grad(ex, x, labels, None, loss)
    assert grad.shape == x.shape and grad.dtype == torch.float64 and L.shape == (x.shape[0],) and logits.shape == (x.shape[0], ex["cfg"]["num_classes"])
    z = logits
    rows = torch.arange(x.shape[0])
    if loss == "ce":
        assert torch.allclose(L, torch.logsumexp(z, 1) - z[rows, labels], rtol=0, atol=1e-12)
    else:
        assert torch.allclose(L, z.topk(2, dim=1).values[:, 1] - z[rows, labels], rtol=0, atol=1e-12) and bool((L < 0).all())
    g = torch.Generator().manual_seed(3)
    h, worst = 1e-5, 0.0
    for b in range(x.shape[0]):
        for flat in torch.randint(0, x[b].numel(), (24,), generator=g).tolist():
            e = torch.zeros_like(x)
            e[b].view(-1)[flat] = h
            up, dn = (RB.reference_loss_grad(ex, x + s * e, labels, None, loss)[2] for s in (1, -1))
            fd = (up - dn) / (2 * h)
            assert float(fd.abs().sum() - fd[b].abs()) == 0.0                      # the other images' losses do not move at all
            worst = max(worst, abs(float(fd[b]) - float(grad[b].view(-1)[flat])))
    print(f"reference_loss_grad {loss}: worst |fd - grad| {worst:.2e} of largest entry {float(grad.abs().max()):.2e}")
    assert worst <= 1e-6 * float(grad.abs().max())


def test_reference_loss_grad_takes_num_labels_and_checks_labels():
    ex, x = RR.export_of(NAME)
    nc = ex["cfg"]["num_classes"]
    labels = torch.zeros(x.shape[0], dtype=torch.int64)
    full = RB.reference_loss_grad(ex, x.double(), labels, None, "ce")
    part = RB.reference_loss_grad(ex, x.double(), labels, 4, "ce")
    assert torch.equal(full[0], part[0]) and bool((part[2] < full[2]).all()) and not torch.equal(full[1], part[1])
    for bad in ([0], [0, nc], [-1, 0], [0.5, 1.0]):
        with pytest.raises(ValueError):
            RB.reference_loss_grad(ex, x.double(), bad, None, "ce")
    with pytest.raises(ValueError, match="margin"):
        RB.reference_loss_grad(ex, x.double(), labels, 1, "margin")
    with pytest.raises(ValueError, match="loss"):
        RB.reference_loss_grad(ex, x.double(), labels, None, "hinge")


def test_linf_bounds_against_hand_values():
    eps, lo, hi = RB.linf_bounds(data.CIFAR_MEAN, data.CIFAR_STD, 8)
    want = torch.tensor([8 / 255 / 0.5] * 3, dtype=torch.float64).float()
    assert eps.dtype == lo.dtype == hi.dtype == torch.float32 and torch.equal(eps, want)
    assert torch.equal(lo, torch.tensor([-1.0] * 3)) and torch.equal(hi, torch.tensor([1.0] * 3))
    eps, lo, hi = RB.linf_bounds(data.IMAGENET_MEAN, data.IMAGENET_STD, 4)
    m, s = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    assert tuple(data.IMAGENET_MEAN) == m and tuple(data.IMAGENET_STD) == s
    for c in range(3):                                   # float64 arithmetic, rounded once
        assert float(eps[c]) == float(torch.tensor(4 / 255 / s[c], dtype=torch.float64).float())
        assert float(lo[c]) == float(torch.tensor((0 - m[c]) / s[c], dtype=torch.float64).float())
        assert float(hi[c]) == float(torch.tensor((1 - m[c]) / s[c], dtype=torch.float64).float())
    assert abs(float(lo[0]) + 2.1179039) < 1e-6 and abs(float(hi[2]) - 2.64) < 1e-6 and abs(float(eps[1]) - 0.0700280) < 1e-6
    assert torch.equal(RB.linf_bounds(m, s, 0)[0], torch.zeros(3))
    with pytest.raises(ValueError):
        RB.linf_bounds(m, (0.1, 0.0, 0.1), 1)


def test_default_alpha_and_argument_refusals():
    assert RB.default_alpha(4, 1) == 4.0 and RB.default_alpha(4, 10) == 1.0 and RB.default_alpha(8, 20) == 1.0 and RB.default_alpha(3, 0) == 3.0
    assert RB.check_attack(4, None, 10, "ce", 10) == (4.0, 1.0, 10) and RB.check_attack(4, 0.5, 1, "margin", 2) == (4.0, 0.5, 1)
    assert RB.check_attack(0, None, 0, "ce", 1) == (0.0, 0.0, 0)
    for bad in (dict(eps=-1), dict(steps=-1), dict(loss="hinge"), dict(loss="margin", num_labels=1), dict(alpha=-0.5), dict(eps=float("nan"))):
        kw = {**dict(eps=4, alpha=None, steps=10, loss="ce", num_labels=10), **bad}
        with pytest.raises(ValueError):
            RB.check_attack(**kw)


@pytest.mark.parametrize("loss", RB.LOSSES)
def test_reference_attack_invariants(loss):
    """Inside the ball and the pixel range (the float32 bounds, compared exactly in float64, where x0 +- eps is exact), FGSM = PGD with one
    step of eps, steps = 0 returns x, a targeted step goes the other way, and the loss at iterate 0 is the clean one without a random start."""
    ex, x = RR.export_of(NAME)
    mean, std = RR.PRESETS["imagenet"]
    eps_c, lo, hi = (t.double().view(1, 3, 1, 1) for t in RB.linf_bounds(mean, std, 2))
    x = torch.minimum(torch.maximum(x.double(), lo), hi)            # an image: the fixture's batch is unit-normal, 3 % of it outside the pixel range
    labels = RB.reference_loss_grad(ex, x, [0] * x.shape[0], None, "ce")[0].argmax(1)
    kw = dict(eps=2, loss=loss, mean=mean, std=std)
    adv, info = RB.reference_attack(ex, x, labels, steps=3, **kw)
    assert bool((adv >= torch.maximum(x - eps_c, lo)).all()) and bool((adv <= torch.minimum(x + eps_c, hi)).all())
    assert info["loss"].shape == (4, x.shape[0]) and info["hit"].shape == (4, x.shape[0]) and info["hit"].dtype == torch.bool
    assert torch.equal(info["loss"][0], info["clean_loss"]) and torch.equal(info["hit"][0], info["clean_hit"]) and bool(info["clean_hit"].all())
    assert torch.equal(info["robust"], info["hit"].all(0)) and bool((info["robust"] <= info["clean_hit"]).all())
    start = torch.rand(x.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 2 - 1
    adv_r, info_r = RB.reference_attack(ex, x, labels, steps=2, start=start, **kw)
    assert bool((adv_r >= torch.maximum(x - eps_c, lo)).all()) and bool((adv_r <= torch.minimum(x + eps_c, hi)).all()) and not torch.equal(adv_r, adv)
    assert not torch.equal(info_r["loss"][0], info_r["clean_loss"])
    fgsm, fi = RB.reference_attack(ex, x, labels, steps=1, **kw)
    pgd1, pi = RB.reference_attack(ex, x, labels, steps=1, alpha=2, **kw)
    assert torch.equal(fgsm, pgd1) and torch.equal(fi["loss"], pi["loss"])
    same, si = RB.reference_attack(ex, x, labels, steps=0, **kw)
    assert torch.equal(same, x) and si["loss"].shape == (1, x.shape[0]) and torch.equal(si["loss"][0], info["clean_loss"])
    toward, ti = RB.reference_attack(ex, x, labels, steps=1, targeted=True, **kw)
    free = (x - eps_c >= lo) & (x + eps_c <= hi)                    # the pixel range clips neither step
    assert 0.9 < float(free.double().mean()) < 1 and torch.equal((fgsm - x)[free], -(toward - x)[free]) and bool(((fgsm - x)[free] != 0).any())
    assert bool((fi["loss"][1] > fi["loss"][0]).all()) and torch.equal(ti["robust"], ~ti["hit"].any(0))


def test_parser_flags_and_refusals(tmp_path):
    p = RB.build_parser()
    flags = {a.option_strings[0] for a in p._actions if a.option_strings and a.option_strings[0] != "-h"}
    assert flags == {"--compact", "--dataset", "--data_dir", "--eval_batch_size", "--num_workers", "--precision", "--interpolation", "--crop_pct",
                     "--packed_dir", "--resident", "--split", "--attack", "--eps", "--alpha", "--steps", "--random_start", "--seed", "--loss",
                     "--labels", "--max_images"}
    a = p.parse_args(["--compact", "f.pt"])
    assert (a.dataset, a.split, a.attack, a.eps, a.alpha, a.steps, a.random_start, a.seed, a.loss, a.labels, a.max_images) == \
        ("imagenet", "test", "pgd", 4.0, None, 10, 0, 0, "ce", "true", None)
    assert RB.attack_plan(a) == (4.0, 1.0, 10, False)
    assert RB.attack_plan(p.parse_args(["--compact", "f.pt", "--attack", "fgsm", "--eps", "2", "--steps", "7", "--random_start", "1"])) == (2.0, 2.0, 1, False)
    assert RB.attack_plan(p.parse_args(["--compact", "f.pt", "--eps", "8", "--steps", "20", "--random_start", "1", "--alpha", "0.5"])) == (8.0, 0.5, 20, True)
    for bad in (["--attack", "cw"], ["--loss", "hinge"], ["--labels", "none"], ["--random_start", "2"], ["--split", "val"], ["--precision", "fp16"]):
        with pytest.raises(SystemExit):
            p.parse_args(["--compact", "f.pt", *bad])
    # refused before the compact file or any data is opened: neither exists
    missing = ["--compact", str(tmp_path / "none.pt"), "--dataset", "cifar10", "--data_dir", str(tmp_path / "nowhere")]
    for bad, word in ((["--eps", "-1"], "eps"), (["--steps", "-2"], "steps"), (["--alpha", "-1"], "alpha"), (["--max_images", "0"], "max_images")):
        with pytest.raises(ValueError, match=word):
            RB.main([*missing, *bad])
    with pytest.raises(SystemExit, match="data_dir"):
        RB.main(["--compact", str(tmp_path / "none.pt")])
    # the label set of the data against the model's head, from the file alone: no data directory exists
    ex, _ = RR.export_of(NAME)
    assert ex["cfg"]["num_classes"] == 16
    torch.save(ex, tmp_path / "f.pt")
    with pytest.raises(ValueError, match="num_labels"):
        RB.main(["--compact", str(tmp_path / "f.pt"), "--dataset", "cifar100", "--data_dir", str(tmp_path / "nowhere")])
    assert isinstance(RB.build_parser(), argparse.ArgumentParser)
