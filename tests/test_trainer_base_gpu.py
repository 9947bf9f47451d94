"""GPU: the three trainers share one training step (uvc_amd/trainer.py): Stage1Trainer, Stage2Trainer and CompactTrainer go through
``_Trainer.step`` and differ in its hooks alone, and the ``adamw`` entry of their training states (``adamw_state`` /
``load_adamw_state``) resumes each of them bit for bit.  Micro model of the driver tests, batch 4, 32 x 32 pixels, float32 mode."""
import pytest
import torch

pytestmark = pytest.mark.gpu

MICRO = dict(patch_size=16, embed_dim=128, depth=2, num_heads=2)
B, IMG, NCLS = 4, 32, 16
COMMON = dict(model_type="custom", model_cfg=MICRO, img_size=IMG, num_classes=NCLS, train_batch_size=B, precision="fp32", distillation_type="soft")
KEYS = {"stage1": {"loss", "outputs", "gnorm", "cur", "s", "r", "g", "stepped"}, "stage2": {"loss", "outputs", "gnorm", "stepped"},
        "compact": {"loss", "outputs", "gnorm", "stepped"}}


def build(kind):
    """A fresh trainer in its first epoch; the same seed gives the same initial student and teacher every time."""
    torch.manual_seed(3)
    if kind == "stage1":
        from uvc_amd.stage1 import Stage1Trainer, default_args
        tr = Stage1Trainer(default_args(steps_per_epoch=4, num_epochs=2, warmup_steps=2, seed=3, **COMMON))
        tr.begin_epoch(1)
        return tr
    from uvc_amd.post_train import Stage2Trainer, default_args
    args = default_args(epochs=2, warmup_epochs=0, learning_rate=0.01, compact_multiple=64, **COMMON)
    if kind == "stage2":
        tr = Stage2Trainer(args)
    else:
        from uvc_amd import compact as CP
        from uvc_amd.compact_train import CompactTrainer
        from uvc_amd.trainer import build_model
        dense = build_model(args, "cuda")
        CP.apply_synthetic_masks(dense, CP.synthetic_masks(MICRO["depth"], MICRO["embed_dim"], 4 * MICRO["embed_dim"], seed=3))
        tr = CompactTrainer(args, CP.export_compact(dense))
    tr.begin_epoch(0)
    return tr


def batch(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(B, 3, IMG, IMG, device="cuda", generator=g), torch.softmax(torch.randn(B, NCLS, device="cuda", generator=g), -1)


def adamw_of(tr):
    o = tr.optimizer
    return dict(exp_avg=o.exp_avg.clone(), exp_avg_sq=o.exp_avg_sq.clone(), steps=dict(o.steps), lr=o.param_groups[0]["lr"])


@pytest.fixture(scope="module", params=["stage1", "stage2", "compact"])
def run(request):
    """Two steps on a trainer with its forward hook counted, its state loaded into a fresh twin, then a third step on both."""
    kind = request.param
    tr = build(kind)
    owner = next(c for c in type(tr).__mro__ if "_forward" in vars(c))        # the class whose forward hook this trainer runs
    hook, calls = owner._forward, []

    def counted(self, x, tau):
        calls.append(type(self).__name__)
        return hook(self, x, tau)
    owner._forward = counted
    try:
        outs = [tr.step(*batch(10 + i)) for i in range(2)]
    finally:
        owner._forward = hook
    twin = build(kind)
    twin.load_state_dict(tr.state_dict())
    before = adamw_of(tr), adamw_of(twin)
    x, y = batch(20)
    third = [{k: (v[0].clone() if k == "outputs" else v.clone()) for k, v in t.step(x, y).items() if k in ("loss", "outputs")} for t in (tr, twin)]
    return dict(kind=kind, trainer=tr, twin=twin, calls=calls, keys=[set(o) for o in outs], stepped=[o["stepped"] for o in outs], before=before,
                third=third)


def test_every_trainer_steps_through_the_base(run):
    from uvc_amd.trainer import _Trainer
    tr = run["trainer"]
    assert isinstance(tr, _Trainer) and type(tr).step is _Trainer.step and "step" not in vars(type(tr))     # no wholesale override
    assert run["calls"] == [type(tr).__name__] * 2                           # one forward-hook call per step, from the base step
    assert run["keys"] == [KEYS[run["kind"]]] * 2 and run["stepped"] == [True, True]
    assert tr.global_step == 3 and tr.accum == 1


def test_adamw_state_round_trip_resumes_bit_for_bit(run):
    a, b = run["before"]
    assert torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"])
    assert float(a["exp_avg"].abs().sum()) > 0 and float(a["exp_avg_sq"].sum()) > 0          # two steps' worth of moments, not zeros
    assert a["steps"] == b["steps"] and a["steps"]["main"] == 2 and a["lr"] == b["lr"]
    t, w = run["third"]
    assert torch.equal(t["outputs"], w["outputs"]) and torch.equal(t["loss"], w["loss"])
    assert torch.equal(run["trainer"].model._flat, run["twin"].model._flat)
