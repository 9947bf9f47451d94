"""CPU: the semantics of fine-tuning a compact model (uvc_amd/compact.py: reference_logits; uvc_amd/compact_train.py) -- the compact
export of the Stage-2 fixture states against the reference's own step-0 goldens, compact gradients against the dense masked model's,
exact zeros on padding, three CPU steps, the file round trip and the ``finetune`` parser.  No GPU."""
import numpy as np
import pytest
import torch

import scenarios as SC
from compact_train_ref import CpuCompactTrainer, fixture_export, kept_names, leaves, loss_and_grads, teacher_logits
from helpers import load_golden
from oracle import vit as OV
from test_compact_cpu import dense_state, hand_masks
from uvc_amd import compact as CP
from uvc_amd import compact_train as CT


def test_reference_logits_average_is_reference_forward():
    cfg = OV.VitConfig(img_size=32, patch_size=8, num_classes=16, embed_dim=192, depth=6, num_heads=3, enable_dist=1)
    for dist in (0, 1):
        cfg.enable_dist = dist
        sd = dense_state(cfg, masks=CP.synthetic_masks(cfg.depth, cfg.embed_dim, cfg.hidden, seed=1))
        ex = CP.export_compact(sd)
        x = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(2))
        o, od = CP.reference_logits(ex, x)
        assert (od is o) == (dist == 0)
        assert torch.equal((o + od) / 2, CP.reference_forward(ex, x))


@pytest.mark.parametrize("name", ["stage2_micro_skip", "stage2_micro_deit", "stage2_micro_none", "stage2_tiny8"])
def test_compact_export_reproduces_the_reference_step0(name):
    """float64 logits, loss and clipped gradient checksums of the compact export against the reference's own golden step 0 (the
    shape-preserved tensors; the golden clip coefficient, since the dense run's norm also counts masked weights' gradients)."""
    r, cfg, ex, teacher = fixture_export(name)
    gold = load_golden(name)
    x_all, y_all = SC.make_inputs(r)
    x, y = torch.from_numpy(x_all[0]).double(), torch.from_numpy(y_all[0]).double()
    P = leaves(ex)
    loss, o, od, grads = loss_and_grads(ex, P, x, y, teacher_logits(r, cfg, teacher, x), r)
    big = float(np.abs(gold["step0.logits"]).max())
    e_o = float(np.abs(o.numpy() - gold["step0.logits"]).max()) / big
    e_od = float(np.abs(od.numpy() - gold["step0.logits_dist"]).max()) / big
    e_loss = abs(float(loss) - float(gold["step0.loss"])) / abs(float(gold["step0.loss"]))
    print(f"{name}: logits {e_o:.2e} {e_od:.2e} loss {e_loss:.2e}")
    assert e_o <= 1e-5 and e_od <= 1e-5 and e_loss <= 1e-5
    coef = min(1.0, r["max_grad_norm"] / (float(gold["step0.grad_norm"]) + 1e-6))
    ref = dict(zip([str(n) for n in gold["param_names"]], gold["step0.grad_abs_sum"]))
    pairs = kept_names(ex, P)
    assert len(pairs) >= 8 + 4 * len(ex["blocks"])
    worst = 0.0
    for n, src in pairs:
        got = float(grads[n].abs().sum()) * coef
        worst = max(worst, abs(got - ref[src]) / ref[src])
    print(f"{name}: grad_abs_sum {worst:.2e}")
    assert worst <= 1e-5


def _dense_and_compact_grads(cfg, masks):
    sd = dense_state(cfg, masks=masks)
    ex = CP.export_compact(sd, CP.compact_plan(sd))
    x = torch.randn(4, 3, 32, 32, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    y = torch.softmax(torch.randn(4, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(6)), -1)
    raw = {k: v.double().requires_grad_(True) for k, v in sd.items() if not k.endswith(".mask")}
    Pm = {k: (v * sd[k[:-len("weight")] + "mask"].double() if k.endswith(".weight") and k[:-len("weight")] + "mask" in sd else v) for k, v in raw.items()}
    out, _ = OV.forward(Pm, cfg, OV.GateFlags(training=False), x)
    (-(y * torch.log_softmax(out, -1)).sum(-1).mean()).backward()
    S = leaves(ex)
    (-(y * torch.log_softmax(CP.reference_forward(dict(ex, state_dict=S), x), -1)).sum(-1).mean()).backward()
    return ex, raw, S


@pytest.mark.parametrize("dist", [0, 1])
@pytest.mark.parametrize("which", ["synthetic", "hand"])
def test_compact_gradients_equal_the_dense_masked_models(which, dist):
    cfg = OV.VitConfig(img_size=32, patch_size=8, num_classes=16, embed_dim=192, depth=6, num_heads=3, enable_dist=dist)
    masks = CP.synthetic_masks(cfg.depth, cfg.embed_dim, cfg.hidden, seed=1) if which == "synthetic" else hand_masks(cfg)
    ex, raw, S = _dense_and_compact_grads(cfg, masks)
    D = cfg.embed_dim
    worst = 0.0

    # largest deviation over the dense tensor's largest entry (a slice alone can be analytically zero: the gradient of the k bias is,
    # softmax being invariant to a shift of all scores of a row)
    def rel(a, r, whole=None):
        return float((a - r).abs().max() / (r if whole is None else whole).abs().max())
    for k, b in enumerate(ex["blocks"]):
        p, q = f"blocks.{b['source']}.", f"blocks.{k}."
        nh, dv = len(b["heads"]), b["v_dim"]
        gq, gb, gp = S[q + "attn.qkv.weight"].grad, S[q + "attn.qkv.bias"].grad, S[q + "attn.proj.weight"].grad
        rq, rb, rp = raw[p + "attn.qkv.weight"].grad, raw[p + "attn.qkv.bias"].grad, raw[p + "attn.proj.weight"].grad
        for j, (h, dims) in enumerate(zip(b["heads"], b["v_index"])):
            for s in (0, 1):
                lo, src = s * nh * 64 + j * 64, s * D + h * 64
                worst = max(worst, rel(gq[lo:lo + 64], rq[src:src + 64], rq), rel(gb[lo:lo + 64], rb[src:src + 64], rb))
            src = torch.tensor([2 * D + h * 64 + c for c in dims])
            dst = 2 * nh * 64 + j * dv + torch.arange(len(dims))
            worst = max(worst, rel(gq[dst], rq[src], rq), rel(gb[dst], rb[src], rb),
                        rel(gp[:, j * dv + torch.arange(len(dims))], rp[:, torch.tensor([h * 64 + c for c in dims])], rp))
        idx = torch.tensor(b["hidden_index"], dtype=torch.long)
        if len(idx):
            n = len(idx)
            worst = max(worst, rel(S[q + "mlp.fc1.weight"].grad[:n], raw[p + "mlp.fc1.weight"].grad[idx], raw[p + "mlp.fc1.weight"].grad),
                        rel(S[q + "mlp.fc1.bias"].grad[:n], raw[p + "mlp.fc1.bias"].grad[idx], raw[p + "mlp.fc1.bias"].grad),
                        rel(S[q + "mlp.fc2.weight"].grad[:, :n], raw[p + "mlp.fc2.weight"].grad[:, idx], raw[p + "mlp.fc2.weight"].grad))
    for n, src in kept_names(ex, S):
        worst = max(worst, rel(S[n].grad, raw[src].grad))
    print(f"{which} dist={dist}: worst kept-position error {worst:.2e}")
    assert worst <= 1e-10
    # padding entries: exactly zero gradients
    pads = CT.padding_masks(ex)
    assert any(m.any() for m in pads.values())
    for n, m in pads.items():
        if S[n].grad is not None and m.any():
            assert float(S[n].grad[m].abs().max()) == 0.0, n
    # exactly the parameters no forward reads have no gradient
    assert sorted(n for n, v in S.items() if v.grad is None) == sorted(CT.unread_parameters(ex))
    if which == "hand":
        assert "blocks.1.norm1.weight" in CT.unread_parameters(ex) and "blocks.1.mlp.fc2.weight" in CT.unread_parameters(ex)


def test_three_cpu_steps_keep_padding_zero_and_the_file_round_trips(tmp_path):
    r, cfg, ex, teacher = fixture_export("stage2_micro_skip")
    tr = CpuCompactTrainer(ex, r, cfg, teacher, dtype=torch.float32)
    x_all, y_all = SC.make_inputs(r)
    pads = CT.padding_masks(ex)
    assert sum(int(m.sum()) for m in pads.values()) > 0
    for step in range(3):
        tr.begin_epoch(r["epoch_of_step"][step])
        out = tr.step(torch.from_numpy(x_all[step]), torch.from_numpy(y_all[step]))
        assert np.isfinite(out["loss"])
        for n, m in pads.items():
            if m.any():
                assert float(tr.P[n][m].abs().max()) == 0.0, (step, n)
    moved = sum(int(not torch.equal(tr.P[n].detach(), ex["state_dict"][n])) for n in tr.P)
    assert moved >= len(tr.P) - len(CT.unread_parameters(ex)) - 2
    tuned = CT.with_state(ex, tr.P)
    path = tmp_path / "tuned.pt"
    torch.save(tuned, path)
    back = CP.load_compact(path)
    assert back["cfg"] == ex["cfg"] and back["blocks"] == ex["blocks"] and back["version"] == 1 and back["format"] == CP.FORMAT
    assert all(torch.equal(back["state_dict"][k], tr.P[k].detach()) for k in ex["state_dict"])
    assert torch.isfinite(CP.reference_forward(back, torch.from_numpy(x_all[0]))).all()


def test_finetune_parser_takes_stage2_flags_and_the_others_parse_as_before():
    from uvc_amd.post_train import default_args
    p = CP._parser()
    a = p.parse_args(["finetune", "--compact", "in.pt", "--output", "out.pt"])
    for k, v in vars(default_args()).items():
        assert getattr(a, k) == v, k
    assert (a.steps, a.eval_steps, a.eval_batch_size, a.synthetic, a.dataset, a.mixup, a.cutmix, a.smoothing) == (20, 2, 64, 1, "imagenet", 0.8, 1.0, 0.1)
    assert a.teacher_model == "" and a.teacher_path == "" and a.model_path is None and a.mixup_mode == "batch"
    a = p.parse_args(["finetune", "--compact", "in.pt", "--output", "out.pt", "--distillation_type", "none", "--epochs", "3", "--learning_rate", "0.01",
                      "--teacher-model", "deit_small_patch16_224", "--synthetic", "0", "--dataset", "cifar10"])
    assert (a.distillation_type, a.epochs, a.learning_rate, a.teacher_model, a.synthetic, a.dataset) == ("none", 3, 0.01, "deit_small_patch16_224", 0, "cifar10")
    with pytest.raises(SystemExit):
        p.parse_args(["finetune", "--output", "out.pt"])
    e = p.parse_args(["export", "--checkpoint_dir", "ck", "--output", "m.pt"])
    assert (e.cmd, e.checkpoint_dir, e.output, e.mlp_multiple, e.precision) == ("export", "ck", "m.pt", CP.MLP_MULTIPLE, "bf16")
    v = p.parse_args(["eval", "--compact", "m.pt"])
    assert (v.cmd, v.compact, v.eval_batch_size, v.eval_steps, v.synthetic) == ("eval", "m.pt", 64, 2, 1)
    assert not hasattr(e, "epochs") and not hasattr(v, "learning_rate")


def test_refusals_without_a_gpu():
    from uvc_amd.post_train import default_args
    cfg = OV.VitConfig(img_size=384, patch_size=16, num_classes=8, embed_dim=64, depth=2, num_heads=1, enable_dist=0)
    long = CP.export_compact(dense_state(cfg, masks=CP.synthetic_masks(cfg.depth, cfg.embed_dim, cfg.hidden, seed=4)))
    _, _, ex, _ = fixture_export("stage2_micro_none")
    with pytest.raises(NotImplementedError, match="256"):
        CT.CompactTrainer(default_args(distillation_type="none"), long)
    with pytest.raises(NotImplementedError, match="gradient_accumulation_steps"):
        CT.CompactTrainer(default_args(distillation_type="none", gradient_accumulation_steps=2), ex)
    with pytest.raises(NotImplementedError, match="local_rank"):
        CT.CompactTrainer(default_args(distillation_type="none", local_rank=0), ex)
    with pytest.raises(NotImplementedError, match="bf16_f32resid"):
        CT.CompactTrainer(default_args(distillation_type="none", precision="bf16_f32resid"), ex)
