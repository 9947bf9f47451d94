"""GPU: whole-model steps at sequence lengths above 256 (tests/golden/longseq_scenarios.py).

  * micro models with 4-pixel patches at 64 / 96 / 112 px (N = 257, 577, 578 with the distillation token, 785): one Stage-1 step
    against oracle.step.stage1_step with patch gating off, mode 1 and mode 2 -- loss, logits, clip norm, every parameter's gradient
    (relative L2), s r y p z, resource, mask index sets bit-exact; float32 at 1e-3, bf16 at 2e-2 / 2.5 %;
  * the float32 step against fixtures made by the reference's own modules (longseq_*.npz, make_golden_longseq.py) at 1e-3;
  * DeiT-Tiny at 384 px (production dims, batch 2), bf16, against the oracle; DeiT-Base at 384 px, batch 8: determinism and batch
    independence;
  * Stage 2 at N = 577 against oracle.stage2, and its eval forward with head skipping / MLP compaction against the dense masked one;
  * the drivers: uvc_amd.cli at --img_size 96 with 4-pixel patches writes a checkpoint that uvc_amd.post_train trains on."""
import os

import numpy as np
import pytest
import torch

import longseq_scenarios as LS
import scenarios as SC
from helpers import build_oracle_from_recipe, load_golden, split_draws
from oracle import step as OS
from stage1_driver import Stage1Run

pytestmark = pytest.mark.gpu

TOL = {"fp32": dict(grad=1e-3, out=1e-3, state=1e-3), "bf16": dict(grad=2.5e-2, out=2e-2, state=2e-2)}


def _rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _draws(r, L, seed):
    """Exp(1) draws of one step in the order the reference consumes them (helpers.split_draws): the patch draw [B, P] (mode 2), one [2]
    per block, then the two [L, 2] of the minimax step."""
    g = torch.Generator().manual_seed(seed)
    m = r["model_cfg"]
    P = (m["img_size"] // m["patch_size"]) ** 2
    shapes = ([(r["batch"], P)] if r["enable_patch_gating"] == 2 else []) + [(2,)] * L + [(L, 2), (L, 2)]
    d = {"step0.n_draws": np.int64(len(shapes))}
    for i, s in enumerate(shapes):
        d[f"step0.draw{i}"] = torch.empty(s).exponential_(generator=g).numpy()
    return d


def _run(name, precision, gold=None):
    r = LS.recipe(name)
    _, S = build_oracle_from_recipe(r)
    L = S.cfg.depth
    gold = gold if gold is not None else _draws(r, L, r["seed"] + 3)
    x_all, y_all = SC.make_inputs(r)
    md, e1, e2 = split_draws(r, gold, 0, L)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    o = {}
    OS.stage1_step(S, torch.from_numpy(x_all[0]), torch.from_numpy(y_all[0]), md, e1, e2, o)
    run = Stage1Run(r, precision=precision)
    md, e1, e2 = split_draws(r, gold, 0, L)
    run.inject_draws(md, e1, e2)
    out = run.step(torch.from_numpy(x_all[0]).cuda(), torch.from_numpy(y_all[0]).cuda())
    torch.cuda.synchronize()
    grads = {n: (None if p.grad is None else p.grad.detach().float().cpu().clone()) for n, p in run.model.named_parameters()}
    return r, S, o, run, out, grads


def _check(r, S, o, run, out, grads, precision):
    t = TOL[precision]
    loss, ref_loss = float(out["loss"]), float(o["loss"])
    assert abs(loss - ref_loss) <= t["out"] * abs(ref_loss), (loss, ref_loss)
    assert _rel(out["outputs"][0].detach().float().cpu(), o["logits"]) <= t["out"]
    gn, ref_gn = float(out["gnorm"]), float(o["grad_norm"])
    assert abs(gn - ref_gn) <= t["grad"] * ref_gn, (gn, ref_gn)
    coef = min(1.0, r["max_grad_norm"] / (gn + 1e-6))
    worst = {}
    for n, g in grads.items():
        ref = o["grads"].get(n)
        assert (g is None) == (ref is None), n
        if g is not None:
            worst[n] = _rel(g * (1.0 if n == "block_skip_gating" else coef), ref)
    # The gates' gradients are sums that cancel: the patch scorer's bias gets sum_p d(scores) = 0 up to rounding (the softmax's
    # Jacobian), its weight and the mode-1 gate logits sums of such differences; like the block gate's (tests/test_stage1_gpu.py) they
    # take 4 x the bound, and the scorer's bias an absolute one against the size of the scorer's weight gradient.
    gates = ("block_skip_gating", "patch_gating", "gumbel.weight")
    if "gumbel.bias" in worst:
        del worst["gumbel.bias"]
        err = float((grads["gumbel.bias"].double() * coef - o["grads"]["gumbel.bias"].double()).abs().max())
        assert err <= t["grad"] * float(o["grads"]["gumbel.weight"].double().norm()), ("gumbel.bias", err)
    bad = {k: round(v, 5) for k, v in worst.items() if v > (t["grad"] if k not in gates else 4 * t["grad"])}
    assert not bad, ("per-tensor gradient error above tolerance", bad)
    mm = run.minimax
    for k, ref in (("s", S.st.s), ("r", S.st.r), ("y", S.st.y), ("p", S.st.p)):
        np.testing.assert_allclose(getattr(mm, k).data.cpu().numpy(), ref.numpy(), rtol=t["state"], atol=1e-6, err_msg=k)
    assert abs(float(mm.z.detach()) - float(S.st.z)) <= 1e-4 * abs(float(S.st.z))
    assert abs(float(out["cur"]) - float(o["cur_resource"])) <= 1e-4
    from oracle import uvc as OU
    from uvc_amd.uvc_utils import prune_w_mask
    prune_w_mask(run.minimax, run.optimizer)
    for l, (_, _, _, keep1, keep3) in enumerate(OU.prune_masks(S.st, S.w1(), S.w3())):
        assert torch.equal(run.layers["W1"][l].mask[0].cpu().bool(), keep1.bool()), f"proj index set of layer {l}"
        assert torch.equal(run.layers["W3"][l].mask[0].cpu().bool(), keep3.bool()), f"fc2 index set of layer {l}"
    return worst


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("size", [64, 96, 112])
@pytest.mark.parametrize("gating", ["pruned", "patch1", "patch2"])
def test_micro_stage1_step_matches_oracle(size, gating, precision):
    name = f"longseq_p4_{size}_{gating}"
    r, S, o, run, out, grads = _run(name, precision)
    assert run.model._cfg.img_size == size and (size // 4) ** 2 + 1 > 256
    _check(r, S, o, run, out, grads, precision)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_micro_stage1_step_with_distillation_token_n578(precision):
    r, S, o, run, out, grads = _run("longseq_p4_96_deit", precision)
    _check(r, S, o, run, out, grads, precision)


@pytest.mark.parametrize("name", ["longseq_p4_96_pruned", "longseq_p4_96_patch2", "longseq_p4_112_pruned"])
def test_fp32_step_matches_reference_golden(name):
    """The reference's own modules (tests/golden/make_golden_longseq.py) at N = 577 / 785: loss, logits, clip norm, resource and the
    primal-dual state after the step at 1e-3, mask index sets exactly."""
    gold = load_golden(name)
    r, S, o, run, out, grads = _run(name, "fp32", gold=gold)
    for what, got, ref in (("loss", float(out["loss"]), float(gold["step0.loss"])), ("grad_norm", float(out["gnorm"]), float(gold["step0.grad_norm"]))):
        assert abs(got - ref) <= 1e-3 * abs(ref), (what, got, ref)
    np.testing.assert_allclose(out["outputs"][0].detach().cpu().numpy(), gold["step0.logits"], rtol=1e-3, atol=3e-4)
    assert abs(float(out["cur"]) - float(gold["step0.cur_resource"])) <= 1e-4
    mm = run.minimax
    np.testing.assert_allclose(mm.s.data.cpu().numpy(), gold["step0.s"], rtol=1e-3, atol=1e-6)
    np.testing.assert_allclose(mm.r.data.cpu().numpy(), gold["step0.r"], rtol=1e-3, atol=1e-6)
    from uvc_amd.uvc_utils import prune_w_mask
    prune_w_mask(mm, run.optimizer)
    for l in range(run.cfg.depth):
        assert np.array_equal(np.packbits(run.layers["W1"][l].mask[0].cpu().numpy().astype(np.uint8)), gold[f"keep_proj.{l}"])
        assert np.array_equal(np.packbits(run.layers["W3"][l].mask[0].cpu().numpy().astype(np.uint8)), gold[f"keep_fc2.{l}"])


def test_deit_tiny_384_bf16_step_matches_oracle():
    r, S, o, run, out, grads = _run("longseq_tiny384", "bf16")
    assert run.model._cfg.img_size == 384
    _check(r, S, o, run, out, grads, "bf16")


def test_deit_base_384_deterministic_and_batch_independent():
    from uvc_amd.stage1 import Stage1Trainer, default_args
    torch.manual_seed(733)
    B = 8
    a = default_args(model_type="deit_base_patch16_224", img_size=384, precision="bf16", train_batch_size=B)
    tr = Stage1Trainer(a, device="cuda")
    tr.begin_epoch(a.warmup_epochs + 1)
    L = tr.model._cfg.depth
    e = torch.empty(L, 2, device="cuda").exponential_(generator=torch.Generator(device="cuda").manual_seed(9))
    tr.model.exp_source = lambda shape, e=e: e.clone()
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(B, 3, 384, 384, device="cuda", generator=g)
    y = torch.softmax(torch.randn(B, 1000, device="cuda", generator=g), -1)

    def fwd_bwd(xx, yy):
        m = tr.model
        outputs, _ = m(xx, -1, tr.args.patch_ratio)
        loss = tr.criterion(xx, outputs, yy)
        loss.backward()
        torch.cuda.synchronize()
        return outputs[0].detach().clone(), float(loss.detach()), m._flat_grad[:m._off.n_total].clone()

    tr.model.train()
    a1, a2 = fwd_bwd(x, y), fwd_bwd(x, y)
    assert torch.isfinite(a1[2]).all() and float(a1[2].abs().max()) > 0
    assert torch.equal(a1[0], a2[0]) and a1[1] == a2[1] and torch.equal(a1[2], a2[2]), "the step is not deterministic"
    tr.model.eval()
    with torch.no_grad():
        lb, _ = tr.model(x)
        ls, _ = tr.model(x[3:5].contiguous())
    assert torch.equal(lb[3:5], ls), "eval forward is not batch independent"


def _stage2(precision):
    """tests/test_stage2_gpu.py:build for the long-sequence Stage-2 scenario: the Stage-1 checkpoint as save_model writes it."""
    from helpers import stage2_state
    from uvc_amd.post_train import Stage2Trainer, default_args, setup
    r = LS.stage2_recipe("stage2_longseq_p4_96")
    cfg, params, masks, teacher = stage2_state(r)
    m = r["model_cfg"]
    args = default_args(model_type="scenario", model_cfg=dict(patch_size=m["patch_size"], embed_dim=m["embed_dim"], depth=m["depth"],
                                                              num_heads=m["num_heads"], mlp_ratio=m["mlp_ratio"]),
                        img_size=m["img_size"], num_classes=m["num_classes"], enable_deit=m["enable_dist"], precision=precision,
                        train_batch_size=r["batch"], learning_rate=r["learning_rate"], weight_decay=r["weight_decay"],
                        max_grad_norm=r["max_grad_norm"], epochs=r["epochs"], warmup_epochs=r["warmup_epochs"],
                        warmup_lr=r["warmup_lr"], min_lr=r["min_lr"], decay_rate=r["decay_rate"], opt_eps=r["opt_eps"],
                        distillation_type=r["distillation_type"], distillation_alpha=r["distillation_alpha"],
                        distillation_tau=r["distillation_tau"], compact_mlp=1, compact_multiple=64)
    _, probe, _ = setup(default_args(**vars(args)), device="cuda")
    state = {k: v.detach().cpu().clone() for k, v in probe.state_dict().items()}
    for k, v in params.items():
        state[k] = v.clone()
    for k, v in masks.items():
        state[k[:-len("weight")] + "mask"] = v.clone()
    del probe
    return r, cfg, Stage2Trainer(args, checkpoint=state, teacher_state=teacher)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_stage2_step_at_n577_matches_oracle(precision):
    from helpers import stage2_hyper, stage2_state
    from oracle import stage2 as O2
    r, cfg, tr = _stage2(precision)
    assert cfg.num_patches + 1 == 577
    _, params, masks, teacher = stage2_state(r)
    S = O2.Stage2(cfg=cfg, params=params, masks=masks, teacher=teacher if r["distillation_type"] != "none" else None, hp=stage2_hyper(r))
    x_all, y_all = SC.make_inputs(r)
    S.begin_epoch(r["epoch_of_step"][0])
    ref = {}
    O2.stage2_step(S, torch.from_numpy(x_all[0]), torch.from_numpy(y_all[0]), ref)
    tr.begin_epoch(r["epoch_of_step"][0])
    out = tr.step(torch.from_numpy(x_all[0]).cuda(), torch.from_numpy(y_all[0]).cuda(), zero_grad=False)
    t = TOL[precision]
    assert abs(float(out["loss"]) - float(ref["loss"])) <= t["out"] * abs(float(ref["loss"]))
    assert _rel(out["outputs"][0].detach().float().cpu(), ref["logits"]) <= t["out"]
    gn = float(out["gnorm"])
    assert abs(gn - float(ref["grad_norm"])) <= t["grad"] * float(ref["grad_norm"])
    coef = min(1.0, r["max_grad_norm"] / (gn + 1e-6))
    bad = {}
    for n, p in tr.model.named_parameters():
        g = ref["grads"].get(n)
        assert (p.grad is None) == (g is None), n
        if g is not None and float(g.norm()) > 0:
            e = _rel(p.grad.detach().float().cpu() * coef, g)
            if e > t["grad"]:
                bad[n] = round(e, 5)
    assert not bad, bad


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_stage2_eval_forward_skipping_heads_and_units_at_n577(precision):
    r, cfg, tr = _stage2(precision)
    m = tr.model
    assert tr.head_keep is not None and int((tr.head_keep == 0).sum()) > 0, tr.head_keep
    m.apply_masks()
    x = torch.from_numpy(SC.make_inputs(r)[0][0]).cuda()
    m.eval()
    with torch.no_grad():
        out_skip, _ = m(x)
        m.set_head_skipping(False)
        out_heads_dense, _ = m(x)
        m.set_mlp_compaction(False)
        out_dense, _ = m(x)
    assert torch.equal(out_skip, out_heads_dense)
    tol = dict(rtol=1e-5, atol=1e-5) if precision == "fp32" else dict(rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(out_skip, out_dense, **tol)


def test_drivers_train_at_img_size_96_with_patch_4(tmp_path, capsys):
    """uvc_amd.cli (Stage 1; patch gating mode 2 by default, so the top-k runs at P = 576) at --img_size 96 with 4-pixel patches
    (N = 577) for two steps writes a checkpoint; uvc_amd.post_train (Stage 2) strict-loads it and trains on it."""
    import glob

    from uvc_amd import cli, post_train
    cfg = '{"patch_size": 4, "embed_dim": 128, "depth": 2, "num_heads": 2}'
    out = tmp_path / "run"
    tr = cli.main(["--name", "s1", "--output_dir", str(out), "--model_type", "custom", "--model_cfg", cfg, "--img_size", "96", "--num_classes", "16",
                   "--train_batch_size", "4", "--eval_batch_size", "4", "--num_epochs", "1", "--warmup_epochs", "0", "--steps_per_epoch", "1",
                   "--log_interval", "1", "--gating_interval", "1", "--precision", "bf16", "--seed", "11"])
    capsys.readouterr()
    assert tr.global_step == 2 and tr.model._cfg.img_size == 96
    cks = sorted(c for c in glob.glob(str(out / "s1" / "custom_*.pth.tar")) if "state" not in c)
    assert cks, list(out.rglob("*"))
    sd = torch.load(cks[-1], map_location="cpu")
    assert tuple(sd["pos_embed"].shape) == (1, 577, 128)
    tr2 = post_train.main(["--model_type", "custom", "--model_cfg", cfg, "--img_size", "96", "--num_classes", "16", "--train_batch_size", "4",
                           "--eval_batch_size", "4", "--epochs", "1", "--steps", "2", "--precision", "bf16", "--checkpoint_dir", cks[-1],
                           "--output_dir", str(out), "--name", "s2", "--warmup_epochs", "0", "--compact_multiple", "64"])
    capsys.readouterr()
    assert torch.isfinite(tr2.model._flat).all()
    assert not torch.equal(tr2.model.blocks[1].mlp.fc2.weight.detach().cpu(), sd["blocks.1.mlp.fc2.weight"] * sd["blocks.1.mlp.fc2.mask"])
