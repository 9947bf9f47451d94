"""GPU: both drivers start from pretrained checkpoints (uvc_amd/checkpoints.py).  Stage 1 loads the student from --model_path and
the teacher from --teacher-path (default --model_path), with a teacher of another width or family; an ImageNet-width checkpoint goes
into a 16-class head; Stage 2 distils from --teacher-path and --eval_only evaluates a pretrained file; --resume rebuilds the teacher
and refuses another one.  Micro custom models in float32, as tests/test_drivers_gpu.py."""
import json
from argparse import Namespace

import pytest
import torch

pytestmark = pytest.mark.gpu

MICRO = {"patch_size": 16, "embed_dim": 128, "depth": 2, "num_heads": 2}
WIDE = {"patch_size": 16, "embed_dim": 192, "depth": 2, "num_heads": 3}
T2T_MICRO = {"embed_dim": 128, "depth": 2, "num_heads": 2, "mlp_ratio": 3.0}
IMG, NCLS, B = 64, 16, 8


def build(kind, cfg, num_classes=NCLS):
    from uvc_amd.stage1 import model_kwargs
    a = Namespace(img_size=IMG, num_classes=num_classes, precision="fp32")
    t2t = kind == "custom_t2t"
    if t2t:
        from uvc_amd.t2t_vit import T2T_ViT
        return T2T_ViT(**model_kwargs(True, cfg, a, "cuda"))
    from uvc_amd.model_distilled import DistilledVisionTransformer
    return DistilledVisionTransformer(enable_dist=0, **model_kwargs(False, cfg, a, "cuda"))


def make_checkpoint(path, seed, kind="custom", cfg=MICRO, num_classes=NCLS, layout="model"):
    """A pretrained-like file: seeded init, Linear weights x3 and the head x20 so that the logits are far from uniform."""
    torch.manual_seed(seed)
    m = build(kind, cfg, num_classes)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    for k, v in sd.items():
        if k.endswith(".weight") and v.dim() == 2:
            v.mul_(20.0 if k.startswith("head.") else 3.0)
    torch.save({layout: sd} if layout else sd, str(path))
    return sd


def standalone_logits(kind, cfg, path, x):
    from uvc_amd.checkpoints import load_pretrained
    m = build(kind, cfg)
    load_pretrained(str(path), m, num_classes=NCLS, verbose=False)
    m.eval()
    with torch.no_grad():
        return m(x)[0].clone()


def soft_loss64(o, o_kd, y, t, alpha, tau=1.0):
    """utils/losses.py:51-64 with the soft-target CE base criterion, in float64."""
    o, o_kd, y, t = (v.detach().double().cpu() for v in (o, o_kd, y, t))
    base = (-y * torch.log_softmax(o, dim=1)).sum(dim=1).mean()
    ls, lt = torch.log_softmax(o_kd / tau, dim=1), torch.log_softmax(t / tau, dim=1)
    kd = (lt.exp() * (lt - ls)).sum() * tau * tau / o_kd.numel()
    return float((1 - alpha) * base + alpha * kd)


def stage1_argv(out, name, extra=()):
    return ["--name", name, "--output_dir", str(out), "--model_type", "custom", "--model_cfg", json.dumps(MICRO), "--img_size", str(IMG),
            "--num_classes", str(NCLS), "--train_batch_size", str(B), "--eval_batch_size", "8", "--num_epochs", "1", "--warmup_epochs", "1",
            "--steps_per_epoch", "2", "--log_interval", "1", "--gating_interval", "2", "--warmup_steps", "2", "--precision", "fp32",
            "--seed", "11", "--zlr_schedule_list", "1", "--save_state", "0"] + list(extra)


def recording(monkeypatch, module, cls_name):
    """Replace the driver's trainer class by a subclass that keeps the initial student / teacher weights and the first step."""
    rec = {}
    base = getattr(module, cls_name)

    class Recording(base):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            rec["trainer"] = self
            rec["student0"] = {k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()}
            rec["teacher0"] = None if self.teacher is None else self.teacher._flat.clone()

        def step(self, x, y, *a, **k):
            out = super().step(x, y, *a, **k)
            if "x" not in rec:
                o = out["outputs"]
                rec.update(x=x.clone(), y=y.clone(), loss=out["loss"].clone(), logits=o[0].clone(), logits_kd=o[1].clone())
            return out

    monkeypatch.setattr(module, cls_name, Recording)
    return rec


def test_stage1_model_path_loads_student_and_teacher(tmp_path, monkeypatch, capsys):
    from uvc_amd import cli
    from uvc_amd.stage1 import Stage1Trainer
    ck = tmp_path / "pretrained.pth"
    sd = make_checkpoint(ck, seed=5)
    rec = recording(monkeypatch, cli, "Stage1Trainer")
    cli.main(stage1_argv(tmp_path / "run", "a", ["--model_path", str(ck)]))
    assert "student: loaded" in capsys.readouterr().out
    s0 = rec["student0"]
    for k, v in sd.items():
        assert torch.equal(s0[k], v), k
    # the same first step as a trainer handed the file's weights explicitly for both models
    args = cli.build_parser().parse_args(stage1_argv(tmp_path / "run", "b"))
    args.model_cfg = dict(MICRO)
    torch.manual_seed(args.seed)
    ref = Stage1Trainer(args, device="cuda", student_state=sd, teacher_state=sd)
    assert torch.equal(ref.teacher._flat, rec["teacher0"])
    ref.begin_epoch(1)
    out = ref.step(rec["x"], rec["y"])
    assert torch.equal(out["outputs"][0], rec["logits"])
    assert float(out["loss"]) == float(rec["loss"])


@pytest.mark.parametrize("kind,cfg", [("custom", MICRO), ("custom", WIDE), ("custom_t2t", T2T_MICRO)], ids=["same", "wide", "t2t"])
def test_stage1_teacher_path_and_teacher_model(tmp_path, monkeypatch, capsys, kind, cfg):
    from uvc_amd import cli
    ck_s, ck_t = tmp_path / "student.pth", tmp_path / "teacher.pth"
    make_checkpoint(ck_s, seed=5)
    make_checkpoint(ck_t, seed=6, kind=kind, cfg=cfg, layout="state_dict_ema")
    rec = recording(monkeypatch, cli, "Stage1Trainer")
    extra = ["--model_path", str(ck_s), "--teacher-path", str(ck_t), "--distillation-type", "soft", "--distillation-alpha", "0.5"]
    if cfg is not MICRO:
        extra += ["--teacher-model", kind, "--teacher_cfg", json.dumps(cfg)]
    cli.main(stage1_argv(tmp_path / "run", "t", extra))
    assert "teacher: loaded" in capsys.readouterr().out
    tr, x = rec["trainer"], rec["x"]
    assert tr.teacher.embed_dim == cfg["embed_dim"] and (type(tr.teacher).__name__ == "T2T_ViT") == (kind == "custom_t2t")
    t = standalone_logits(kind, cfg, ck_t, x)
    with torch.no_grad():
        got = tr.teacher(x)[0]
    assert torch.equal(got, t)
    want = soft_loss64(rec["logits"], rec["logits_kd"], rec["y"], t, alpha=0.5)
    assert abs(float(rec["loss"]) - want) <= 1e-5 * abs(want), (float(rec["loss"]), want)
    # ... and not the student file's logits
    wrong = soft_loss64(rec["logits"], rec["logits_kd"], rec["y"], standalone_logits("custom", MICRO, ck_s, x), alpha=0.5)
    assert abs(wrong - want) > 1e-3 * abs(want)


def test_imagenet_width_checkpoint_into_a_16_class_head(tmp_path, monkeypatch, capsys):
    from uvc_amd import cli
    ck = tmp_path / "imagenet.pth"
    sd = make_checkpoint(ck, seed=7, num_classes=1000)
    rec = recording(monkeypatch, cli, "Stage1Trainer")
    cli.main(stage1_argv(tmp_path / "run", "plain", ["--distillation-type", "none"]))
    plain = rec["student0"]
    cli.main(stage1_argv(tmp_path / "run", "ck", ["--distillation-type", "none", "--model_path", str(ck)]))
    text = capsys.readouterr().out
    assert "1000-class head, the model 16: head.weight, head.bias not loaded (seeded init kept)" in text
    got = rec["student0"]
    blocks = [k for k in sd if k.startswith("blocks.")]
    assert len(blocks) == 2 * 14
    for k in sd:
        if not k.startswith("head."):
            assert torch.equal(got[k], sd[k]), k
    assert torch.equal(got["head.weight"], plain["head.weight"]) and torch.equal(got["head.bias"], plain["head.bias"])
    # the teacher defaults to the same file: a 1000-class teacher cannot give the 16 logits the loss needs
    with pytest.raises(ValueError, match="not 16 classes wide"):
        cli.main(stage1_argv(tmp_path / "run", "t", ["--model_path", str(ck)]))


def stage2_argv(out, extra=()):
    return ["--model_type", "custom", "--model_cfg", json.dumps(MICRO), "--img_size", str(IMG), "--num_classes", str(NCLS),
            "--train_batch_size", str(B), "--eval_batch_size", "8", "--epochs", "2", "--steps", "2", "--precision", "fp32",
            "--output_dir", str(out), "--name", "s2", "--warmup_epochs", "1", "--compact_multiple", "64"] + list(extra)


def test_stage2_teacher_path_and_eval_only(tmp_path, monkeypatch, capsys):
    from uvc_amd import post_train
    ck_s, ck_t = tmp_path / "student.pth", tmp_path / "teacher.pth"
    sd_s = make_checkpoint(ck_s, seed=5)
    make_checkpoint(ck_t, seed=6, layout=None)
    rec = recording(monkeypatch, post_train, "Stage2Trainer")
    post_train.main(stage2_argv(tmp_path / "run", ["--model_path", str(ck_s), "--teacher-path", str(ck_t), "--distillation_alpha", "0.5"]))
    capsys.readouterr()
    assert rec["trainer"].teacher_source["path"] == str(ck_t)
    t = standalone_logits("custom", MICRO, ck_t, rec["x"])
    want = soft_loss64(rec["logits"], rec["logits_kd"], rec["y"], t, alpha=0.5)
    assert abs(float(rec["loss"]) - want) <= 1e-5 * abs(want), (float(rec["loss"]), want)
    # --teacher-path defaults to --model_path
    a2 = post_train.default_args(model_type="custom", model_cfg=MICRO, img_size=IMG, num_classes=NCLS, precision="fp32", model_path=str(ck_t),
                                 teacher_model="", teacher_path="")
    first = rec["trainer"]
    tr2 = post_train.Stage2Trainer(a2)
    assert tr2.teacher_source["path"] == str(ck_t)
    assert torch.equal(tr2.teacher._flat, first.teacher._flat)
    # --eval_only 1: valid() once on the pretrained file
    post_train.main(stage2_argv(tmp_path / "run", ["--model_path", str(ck_s), "--eval_only", "1", "--eval_steps", "3"]))
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    from uvc_amd.model_distilled import DistilledVisionTransformer
    from uvc_amd.post_train import register_masks, synthetic_valid_fn
    from uvc_amd.stage1 import model_kwargs
    a = Namespace(img_size=IMG, num_classes=NCLS, precision="fp32", seed=42, eval_steps=3, eval_batch_size=8)
    m = DistilledVisionTransformer(enable_dist=0, gumbel_hard=True, **model_kwargs(False, MICRO, a, "cuda"))
    register_masks(m)
    m.load_state_dict(sd_s, strict=False)
    assert res["steps"] == 0 and res["best_acc"] == synthetic_valid_fn(a, torch.device("cuda", 0))(m)


def test_stage1_resume_rebuilds_the_teacher_and_refuses_another(tmp_path, capsys):
    from uvc_amd import cli
    ck_s, ck_t, ck_o = tmp_path / "student.pth", tmp_path / "teacher.pth", tmp_path / "other.pth"
    make_checkpoint(ck_s, seed=5)
    make_checkpoint(ck_t, seed=6)
    make_checkpoint(ck_o, seed=8)
    out = tmp_path / "run"
    flags = ["--num_epochs", "2", "--save_state", "1", "--model_path", str(ck_s), "--teacher-path", str(ck_t), "--distillation-type", "soft"]
    tr = cli.main(stage1_argv(out, "full", flags))
    state = out / "full" / "custom_state_2.pth.tar"
    assert torch.load(str(state), map_location="cpu")["teacher"]["path"] == str(ck_t)
    tr_b = cli.main(stage1_argv(out, "resumed", flags + ["--resume", str(state)]))
    capsys.readouterr()
    assert tr_b.global_step == tr.global_step == 6 and torch.equal(tr_b.model._flat, tr.model._flat)
    for k in ("s", "r", "y", "p", "z"):
        assert torch.equal(getattr(tr_b.minimax, k).data, getattr(tr.minimax, k).data), k
    other = [f if f != str(ck_t) else str(ck_o) for f in flags]
    with pytest.raises(ValueError, match="made with teacher custom from .*teacher.pth"):
        cli.main(stage1_argv(out, "other", other + ["--resume", str(state)]))
