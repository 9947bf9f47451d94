"""GPU: fine-tuning compact models at their kept widths -- the attention backward at a value width (uvc_attention_bwd_vdim: the
dq + dk/dv pair templated on the value head dim) against float64 autograd of the compact attention, against uvc_attention_bwd at
v_dim = 64, across batch sizes, and its refusals; the compact training forward + backward (uvc_vit_compact_train_forward,
uvc_vit_compact_backward) against the reference's Stage-2 goldens, float64 autograd of compact.reference_logits and the dense
engine; CompactTrainer against its CPU restatement, resuming, and the ``finetune`` command."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import scenarios as SC
from compact_train_ref import CpuCompactTrainer, fixture_export, kept_names, leaves, loss_and_grads, teacher_logits
from helpers import load_golden
from oracle import step as OS
from test_compact_gpu import attn, dense_model, ref_attn
from test_stage1_gpu import close
from uvc_amd import _lib as L
from uvc_amd import compact as CP
from uvc_amd import compact_train as CT
from uvc_amd import ops

pytestmark = pytest.mark.gpu

# the tolerances of test_kernels_gpu.py::test_attention_fwd_bwd, on its input scale (unit normal qkv and dout)
DT = {"fp32": (torch.float32, L.UVC_F32, dict(rtol=2e-4, atol=2e-5)), "bf16": (torch.bfloat16, L.UVC_BF16, dict(rtol=5e-2, atol=6e-2))}


def inputs(B, N, H, dv, dt, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    qkv = torch.randn(B, N, H * (128 + dv), device="cuda", generator=g).to(dt)
    dout = torch.randn(B, N, H * dv, device="cuda", generator=g).to(dt)
    return qkv, dout


def forward(qkv, B, N, H, dv, code):
    rc, o, lse = attn(qkv, B, N, H, dv, code)
    assert rc == 0, L.lib().uvc_last_error()
    return o, lse


def backward(qkv, o, lse, dout, B, N, H, dv, code):
    dqkv = torch.full_like(qkv, float("nan"))
    delta = torch.full((B, H, N), float("nan"), device="cuda")
    ops.attention_bwd_vdim(qkv, o, lse, dout, dqkv, delta, B, N, H, dv, code)
    return dqkv, delta


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("N,H", [(5, 1), (50, 3), (197, 3), (198, 6), (256, 2)])
@pytest.mark.parametrize("dv", [16, 32, 48, 64])
def test_attention_backward_at_a_value_width_against_float64(prec, N, H, dv):
    dt, code, tol = DT[prec]
    B = 2
    qkv, dout = inputs(B, N, H, dv, dt, seed=N * 11 + H * 3 + dv)
    o, lse = forward(qkv, B, N, H, dv, code)
    dqkv, delta = backward(qkv, o, lse, dout, B, N, H, dv, code)
    torch.cuda.synchronize()
    x = qkv.double().requires_grad_(True)
    ref, _ = ref_attn(x, B, N, H, dv)
    ref.backward(dout.double())
    err = (dqkv.double() - x.grad).abs()
    print(f"{prec} N={N} H={H} dv={dv}: max |dqkv - f64| {float(err.max()):.3e} (max |f64| {float(x.grad.abs().max()):.3e})")
    assert not torch.isnan(dqkv.float()).any()                          # every element of the pre-filled buffer was written
    torch.testing.assert_close(dqkv.double(), x.grad, **tol)
    want_delta = (dout.double() * o.double()).view(B, N, H, dv).sum(-1).permute(0, 2, 1)
    torch.testing.assert_close(delta.double(), want_delta, rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("N", [197, 256])
def test_value_width_64_launches_the_pair_of_uvc_attention_bwd(prec, N):
    dt, code, _ = DT[prec]
    B, H = 2, 3
    qkv, dout = inputs(B, N, H, 64, dt, seed=N)
    o, lse = forward(qkv, B, N, H, 64, code)
    got, got_delta = backward(qkv, o, lse, dout, B, N, H, 64, code)
    want = torch.full_like(qkv, float("nan"))
    want_delta = torch.full((B, H, N), float("nan"), device="cuda")
    ops.attention_bwd(qkv, o, lse, dout, want, want_delta, B, N, H, code, variant=1)
    assert torch.equal(got, want) and torch.equal(got_delta, want_delta)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("dv", [16, 32, 48, 64])
def test_value_width_backward_does_not_depend_on_the_batch(prec, dv):
    dt, code, _ = DT[prec]
    N, H = 197, 3
    qkv, dout = inputs(3, N, H, dv, dt, seed=dv)
    o, lse = forward(qkv, 3, N, H, dv, code)
    d3, delta3 = backward(qkv, o, lse, dout, 3, N, H, dv, code)
    q1, do1 = qkv[:1].contiguous(), dout[:1].contiguous()
    o1, lse1 = forward(q1, 1, N, H, dv, code)
    d1, delta1 = backward(q1, o1, lse1, do1, 1, N, H, dv, code)
    assert torch.equal(o1, o[:1]) and torch.equal(d1, d3[:1]) and torch.equal(delta1, delta3[:1])
    again, _ = backward(qkv, o, lse, dout, 3, N, H, dv, code)             # deterministic: same bits on a repeat
    assert torch.equal(again, d3)


def test_value_width_backward_refusals():
    def call(N, H, v_dim, head_keep=None, alloc_dv=None):
        dv = alloc_dv or v_dim or 64
        qkv = torch.zeros(1, N, H * (128 + dv), device="cuda", dtype=torch.bfloat16)
        o = torch.zeros(1, N, H * dv, device="cuda", dtype=torch.bfloat16)
        lse, delta = torch.zeros(1, H, N, device="cuda"), torch.zeros(1, H, N, device="cuda")
        dout, dqkv = torch.zeros_like(o), torch.zeros_like(qkv)
        a = L.uvc_attn_args()
        a.qkv, a.o, a.lse, a.dout, a.dqkv, a.delta = (L.ptr(t) for t in (qkv, o, lse, dout, dqkv, delta))
        a.B, a.N, a.H, a.head_dim, a.dtype, a.scale, a.v_dim = 1, N, H, 64, L.UVC_BF16, 0.125, v_dim
        a.head_keep = L.ptr(head_keep)
        return L.lib().uvc_attention_bwd_vdim(C.byref(a), L.cur_stream())

    keep = torch.ones(2, dtype=torch.int32, device="cuda")
    assert call(197, 2, 32) == 0
    assert call(197, 2, 0) == 1                                          # UVC_ERR_ARG: a value width is required
    assert call(197, 2, 24, alloc_dv=32) == 1
    assert call(197, 2, 32, head_keep=keep) == 3                         # UVC_ERR_UNSUPPORTED
    assert call(577, 2, 32) == 3 and call(577, 2, 64) == 3               # the streaming pair has no value-width form
    torch.cuda.synchronize()


# ---- the compact training forward + backward ------------------------------------------------------------------------------------------
def trainer_args(r, ex, precision, **over):
    from uvc_amd.post_train import default_args
    c = ex["cfg"]
    kw = dict(img_size=c["img_size"], num_classes=c["num_classes"], enable_deit=c["enable_dist"], precision=precision, train_batch_size=r["batch"],
              learning_rate=r["learning_rate"], weight_decay=r["weight_decay"], max_grad_norm=r["max_grad_norm"], epochs=r["epochs"],
              warmup_epochs=r["warmup_epochs"], warmup_lr=r["warmup_lr"], min_lr=r["min_lr"], decay_rate=r["decay_rate"], opt_eps=r["opt_eps"],
              distillation_type=r["distillation_type"], distillation_alpha=r["distillation_alpha"], distillation_tau=r["distillation_tau"])
    kw.update(over)
    return default_args(**kw)


def compact_trainer(name, precision, **over):
    r, cfg, ex, teacher = fixture_export(name)
    tr = CT.CompactTrainer(trainer_args(r, ex, precision, **over), ex, teacher_state=teacher)
    return r, cfg, ex, teacher, tr


GOLDEN_CASES = [("stage2_micro_skip", "fp32"), ("stage2_micro_skip", "bf16"), ("stage2_micro_deit", "fp32"), ("stage2_micro_deit", "bf16"),
                ("stage2_micro_none", "fp32"), ("stage2_micro_none", "bf16"), ("stage2_tiny8", "fp32"), ("stage2_tiny8", "bf16")]


@pytest.mark.parametrize("name,precision", GOLDEN_CASES)
def test_compact_step0_matches_the_reference_goldens(name, precision):
    """One training forward + backward on the compact export of a Stage-2 fixture state against the reference's own golden step 0, with
    tests/test_stage2_gpu.py's tolerances (what the dense engine is held to on the same fixtures); the shape-preserved tensors'
    gradient checksums times the golden clip coefficient."""
    rtol = 1e-3 if precision == "fp32" else 2e-2
    gold = load_golden(name)
    r, cfg, ex, teacher, tr = compact_trainer(name, precision)
    x_all, y_all = SC.make_inputs(r)
    tr.begin_epoch(r["epoch_of_step"][0])
    out = tr.step(torch.from_numpy(x_all[0]).cuda(), torch.from_numpy(y_all[0]).cuda(), zero_grad=False)
    close(tr.optimizer.param_groups[0]["lr"], gold["step0.lr"], 1e-12, 0, "lr")
    close(float(out["loss"]), gold["step0.loss"], rtol, 1e-6, "loss")
    la = 3e-4 if precision == "fp32" else 3e-2
    close(out["outputs"][0].detach().cpu().numpy(), gold["step0.logits"], rtol, la, "logits")
    close(out["outputs"][1].detach().cpu().numpy(), gold["step0.logits_dist"], rtol, la, "logits_dist")
    coef = min(1.0, r["max_grad_norm"] / (float(gold["step0.grad_norm"]) + 1e-6))
    ref = dict(zip([str(n) for n in gold["param_names"]], gold["step0.grad_abs_sum"]))
    pmap = dict(tr.model.named_parameters())
    pairs = kept_names(ex, pmap)
    got = np.array([float(pmap[n].grad.double().abs().sum()) * coef for n, _ in pairs])
    want = np.array([ref[src] for _, src in pairs])
    print(f"{name} {precision}: worst grad_abs_sum error {float(np.max(np.abs(got - want) / want)):.2e}")
    close(got, want, 3e-3 if precision == "fp32" else 8e-2, 1e-6, "grad_abs_sum")
    assert all(pmap[n].grad is None for n in CT.unread_parameters(ex))


def torch_loss(o, od, y, tl, r):
    return OS.distillation_loss(o, od, y, tl, kind=r["distillation_type"], alpha=r["distillation_alpha"], T=r["distillation_tau"])


def compact_gpu_grads(ex, precision, x, y, tl, r):
    m = CT.CompactTrainableViT(ex, precision=precision)
    (o, od), _ = m(x)
    torch_loss(o, od, y, tl, r).backward()
    torch.cuda.synchronize()
    return m, {n: (None if p.grad is None else p.grad.detach().double().clone()) for n, p in m.named_parameters()}


def float64_grads(ex, x, y, tl, r):
    P = leaves(ex, device="cuda")
    if "patch_gating" in P:
        P["patch_gating"].requires_grad_(False)
    _, _, _, g = loss_and_grads(ex, P, x.double(), y.double(), None if tl is None else tl.double(), r)
    return g


def dense_grads_at_kept_positions(dense, ex, plan, x, y, tl, r):
    """Gradients of the dense engine (train mode, masks applied) gathered into the compact layout (zeros on padding)."""
    dense.train()
    dense.apply_masks()
    (o, od), _ = dense(x)
    torch_loss(o, od, y, tl, r).backward()
    torch.cuda.synchronize()
    sd = {k: v for k, v in dense.state_dict().items() if k.endswith(".mask") or k == "block_skip_gating"}
    g = {n: (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()) for n, p in dense.named_parameters()}
    g = {k: v for k, v in g.items() if k != "block_skip_gating"}
    g["block_skip_gating"] = sd["block_skip_gating"]
    return CP.export_compact(g, plan)["state_dict"]


def per_tensor_errors(got, g64):
    out = {}
    for n, ref in g64.items():
        if ref is None or ref.numel() == 0:
            continue
        out[n] = float((got[n].double().to(ref.device) - ref).abs().max() / ref.abs().max())
    return out


def fixture_problem(name):
    r, cfg, ex, teacher = fixture_export(name)
    x_all, y_all = SC.make_inputs(r)
    x, y = torch.from_numpy(x_all[0]), torch.from_numpy(y_all[0])
    tl = teacher_logits(r, cfg, teacher, x.double())
    return r, ex, x.cuda(), y.cuda(), None if tl is None else tl.float().cuda()


def synthetic_problem(shape, B=4):
    """A 224-px model of test_compact_gpu.py's shapes with synthetic masks: v_dim 16 / 32 / 48 / 64, one block without heads, one without
    units, the mode-1 token mask and the distillation token."""
    from test_compact_gpu import SHAPES
    D = SHAPES[shape]["embed_dim"]
    masks = CP.synthetic_masks(7, D, 4 * D, seed=0)
    masks["blocks.1.attn.proj.mask"] = torch.zeros(D, D)
    masks["blocks.5.mlp.fc2.mask"] = torch.zeros(D, 4 * D)
    r = dict(distillation_type="soft", distillation_alpha=0.3, distillation_tau=1.0)
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(B, 3, 224, 224, device="cuda", generator=g)
    y = torch.softmax(2 * torch.randn(B, 64, device="cuda", generator=g), -1)
    tl = 3 * torch.randn(B, 64, device="cuda", generator=g)
    return r, masks, x, y, tl


@pytest.mark.parametrize("name", ["stage2_micro_skip", "stage2_micro_deit", "stage2_micro_none", "stage2_tiny8"])
def test_compact_gradients_fp32_against_float64_on_the_fixtures(name):
    """Every tensor, restructured ones included: max |g - g64| <= 1e-3 max |g64| (the project's float32 parity bound)."""
    r, ex, x, y, tl = fixture_problem(name)
    g64 = float64_grads(ex, x, y, tl, r)
    m, got = compact_gpu_grads(ex, "fp32", x, y, tl, r)
    assert sorted(n for n, g in got.items() if g is None) == sorted(n for n, g in g64.items() if g is None) == sorted(CT.unread_parameters(ex))
    errs = per_tensor_errors(got, g64)
    print(f"{name}: worst fp32 tensor error {max(errs.values()):.2e} ({max(errs, key=errs.get)})")
    assert max(errs.values()) <= 1e-3, {n: e for n, e in errs.items() if e > 1e-3}
    for n, pm in CT.padding_masks(ex).items():
        if pm.any() and got[n] is not None:
            assert float(got[n][pm.cuda()].abs().max()) == 0.0, n


@pytest.mark.parametrize("shape", ["tiny", "small"])
def test_compact_gradients_fp32_against_float64_and_the_dense_engine_on_synthetic_masks(shape):
    """224-px models with every value width, a block without heads and one without units: against float64 autograd (1e-3 per tensor) and
    against the dense engine's gradients at the kept positions (1e-3 of each tensor's largest entry); padding gradients exactly zero."""
    r, masks, x, y, tl = synthetic_problem(shape)
    dense = dense_model(shape, "fp32", masks=masks)
    plan = CP.compact_plan(dense)
    ex = CP.export_compact(dense, plan)
    assert {b["v_dim"] for b in ex["blocks"]} == {0, 16, 32, 48, 64} and any(b["hidden"] == 0 for b in ex["blocks"])
    g64 = float64_grads(ex, x, y, tl, r)
    m, got = compact_gpu_grads(ex, "fp32", x, y, tl, r)
    assert sorted(n for n, g in got.items() if g is None) == sorted(CT.unread_parameters(ex))
    errs = per_tensor_errors(got, g64)
    print(f"{shape}: worst fp32 tensor error against float64 {max(errs.values()):.2e} ({max(errs, key=errs.get)})")
    assert max(errs.values()) <= 1e-3, {n: e for n, e in errs.items() if e > 1e-3}
    gd = dense_grads_at_kept_positions(dense, ex, plan, x, y, tl, r)
    worst = 0.0
    for n, g in got.items():
        if g is None or g.numel() == 0 or n == "patch_gating":
            continue
        ref = gd[n].double().cuda()
        worst = max(worst, float((g - ref).abs().max() / ref.abs().max()))
        assert float((g - ref).abs().max()) <= 1e-3 * float(ref.abs().max()), n
    print(f"{shape}: worst fp32 tensor difference from the dense engine {worst:.2e}")
    for n, pm in CT.padding_masks(ex).items():
        if pm.any() and got[n] is not None:
            assert float(got[n][pm.cuda()].abs().max()) == 0.0, n


def bf16_case(kind):
    if kind.startswith("stage2"):
        from test_stage2_gpu import build
        r, ex, x, y, tl = fixture_problem(kind)
        _, _, tr = build(kind, "bf16")
        dense = tr.model
        plan = CP.compact_plan(dense)
        assert CP.export_compact(dense, plan)["blocks"] == ex["blocks"]
        return r, ex, plan, dense, x, y, tl
    r, masks, x, y, tl = synthetic_problem(kind)
    dense = dense_model(kind, "bf16", masks=masks)
    plan = CP.compact_plan(dense)
    return r, CP.export_compact(dense, plan), plan, dense, x, y, tl


@pytest.mark.parametrize("kind", ["stage2_micro_skip", "stage2_micro_deit", "stage2_micro_none", "stage2_tiny8", "tiny"])
def test_compact_gradients_bf16_against_float64_and_the_dense_engines_error(kind):
    """bf16: the global gradient norm within Stage 2's 3e-2 of float64.  Per tensor no number is fixed in advance: the dense engine's
    backward (masked dense model, same inputs, same precision) is measured against the same float64 gradients at the kept positions, and
    the compact tensor's error (largest deviation over the tensor's largest float64 entry) must stay within twice that -- two summation
    orders of the same bf16 products -- or within Stage 2's bf16 bound of 8e-2 on the tensor's abs-sum, whichever is looser."""
    r, ex, plan, dense, x, y, tl = bf16_case(kind)
    g64 = float64_grads(ex, x, y, tl, r)
    m, got = compact_gpu_grads(ex, "bf16", x, y, tl, r)
    n64 = float(torch.sqrt(sum((g.double() ** 2).sum() for g in g64.values() if g is not None)))
    ngot = float(torch.sqrt(sum((g ** 2).sum() for g in got.values() if g is not None)))
    print(f"{kind}: global gradient norm {ngot:.6e} against float64 {n64:.6e} ({abs(ngot - n64) / n64:.2e})")
    assert abs(ngot - n64) <= 3e-2 * n64
    gd = dense_grads_at_kept_positions(dense, ex, plan, x, y, tl, r)
    bad = {}
    for n, ref in g64.items():
        if ref is None or ref.numel() == 0:
            continue
        scale = float(ref.abs().max())
        e_c = float((got[n] - ref).abs().max()) / scale
        e_d = float((gd[n].double().cuda() - ref).abs().max()) / scale
        e_sum = abs(float(got[n].abs().sum()) - float(ref.abs().sum())) / float(ref.abs().sum())
        print(f"  {kind} {n}: compact {e_c:.3e} dense {e_d:.3e} abs-sum {e_sum:.3e}")
        if not (e_c <= 2 * e_d or e_sum <= 8e-2):
            bad[n] = (e_c, e_d, e_sum)
    assert not bad, bad
    for n, pm in CT.padding_masks(ex).items():
        if pm.any() and got[n] is not None:
            assert float(got[n][pm.cuda()].abs().max()) == 0.0, n


@pytest.mark.parametrize("name", ["stage2_micro_skip", "stage2_tiny8"])
def test_compact_against_the_dense_trainer_and_what_three_steps_leave_alone(name):
    """fp32, no clipping: kept-position gradients of Stage2Trainer's model and of the compact model agree within 1e-3 of each tensor's
    largest entry, padding gradients are exactly zero; after 3 CompactTrainer steps every padding entry and every parameter no forward
    reads is bit-identical to its start."""
    from test_stage2_gpu import build
    r, ex, x, y, tl = fixture_problem(name)
    _, _, dtr = build(name, "fp32")
    plan = CP.compact_plan(dtr.model)
    gd = dense_grads_at_kept_positions(dtr.model, ex, plan, x, y, tl, r)
    m, got = compact_gpu_grads(ex, "fp32", x, y, tl, r)
    for n, g in got.items():
        if g is None or g.numel() == 0:
            continue
        ref = gd[n].double().cuda()
        assert float((g - ref).abs().max()) <= 1e-3 * float(ref.abs().max()), n
    pads = CT.padding_masks(ex)
    for n, pm in pads.items():
        if pm.any() and got[n] is not None:
            assert float(got[n][pm.cuda()].abs().max()) == 0.0, n
    _, cfg, _, teacher, tr = compact_trainer(name, "fp32", max_grad_norm=1e9)
    start = {n: p.detach().clone() for n, p in tr.model.named_parameters()}
    x_all, y_all = SC.make_inputs(r)
    tr.begin_epoch(1)
    for step in range(3):
        tr.step(torch.from_numpy(x_all[step % len(x_all)]).cuda(), torch.from_numpy(y_all[step % len(y_all)]).cuda())
    torch.cuda.synchronize()
    now = dict(tr.model.named_parameters())
    for n, pm in pads.items():
        if pm.any():
            assert torch.equal(now[n].detach()[pm.cuda()].view(torch.int32), start[n][pm.cuda()].view(torch.int32)), n
    for n in CT.unread_parameters(ex):
        assert torch.equal(now[n].detach().view(torch.int32), start[n].view(torch.int32)), n
    assert sum(int(not torch.equal(now[n].detach(), start[n])) for n in now) >= len(now) - len(CT.unread_parameters(ex)) - 2


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["stage2_micro_deit", "stage2_micro_skip"])
def test_compact_trainer_follows_its_cpu_restatement(name, precision):
    """The recipe's steps (its batches, hyper-parameters, epoch of each step) on the compact export against the float64 CPU
    restatement, with tests/test_stage2_gpu.py's parameter bounds."""
    r, cfg, ex, teacher, tr = compact_trainer(name, precision)
    ref = CpuCompactTrainer(ex, r, cfg, teacher)
    x_all, y_all = SC.make_inputs(r)
    pmap = dict(tr.model.named_parameters())
    names = [n for n in pmap if pmap[n].numel() > 0]
    last = len(ex["blocks"]) - 1
    for step in range(r["steps"]):
        ep = r["epoch_of_step"][step]
        tr.begin_epoch(ep)
        ref.begin_epoch(ep)
        out = tr.step(torch.from_numpy(x_all[step]).cuda(), torch.from_numpy(y_all[step]).cuda())
        want = ref.step(torch.from_numpy(x_all[step]), torch.from_numpy(y_all[step]))
        pre = f"step{step}."
        close(tr.optimizer.param_groups[0]["lr"], ref.cur_lr, 1e-12, 0, pre + "lr")
        close(float(out["loss"]), want["loss"], 1e-3 if precision == "fp32" else 2e-2, 1e-6, pre + "loss")
        close(float(out["gnorm"]), want["gnorm"], 1e-3 if precision == "fp32" else 3e-2, 0, pre + "grad_norm")
        psum = np.array([float(pmap[n].data.double().abs().sum()) for n in names])
        rsum = np.array([float(ref.P[n].abs().sum()) for n in names])
        lr = ref.cur_lr
        if precision == "fp32":
            close(psum, rsum, 1e-4, 0, pre + "param_abs_sum")
        else:
            numel = np.array([pmap[n].numel() for n in names], dtype=np.float64)
            err, tol = np.abs(psum - rsum), 2e-3 * np.abs(rsum) + 0.05 * lr * numel * (step + 1)
            assert np.all(err <= tol), [(n, e, t) for n, e, t in zip(names, err, tol) if e > t]
        wt = (1e-4, 2e-6) if precision == "fp32" else (1e-3, 2.0 * tr.args.lr * (step + 1))
        close(pmap["blocks.0.attn.proj.weight"].data[0].cpu().numpy(), ref.P["blocks.0.attn.proj.weight"][0].numpy(), *wt, pre + "proj row")
        close(pmap[f"blocks.{last}.mlp.fc1.weight"].data[:, 0].cpu().numpy(), ref.P[f"blocks.{last}.mlp.fc1.weight"][:, 0].numpy(), *wt, pre + "fc1 col")
        close(pmap["pos_embed"].data[0, 0].cpu().numpy(), ref.P["pos_embed"][0, 0].numpy(), *wt, pre + "pos_embed")


def test_compact_trainer_resumes_bit_for_bit_and_evaluates_like_the_inference_module(tmp_path):
    name = "stage2_micro_skip"
    r, cfg, ex, teacher, a = compact_trainer(name, "fp32")
    x_all, y_all = SC.make_inputs(r)
    xs = [torch.from_numpy(x).cuda() for x in x_all]; ys = [torch.from_numpy(y).cuda() for y in y_all]
    a.begin_epoch(1)
    for i in range(3):
        out_a = a.step(xs[i], ys[i])
    _, _, _, _, b = compact_trainer(name, "fp32")
    b.begin_epoch(1)
    for i in range(2):
        b.step(xs[i], ys[i])
    path = str(tmp_path / "ct.pth.tar")
    torch.save(b.state_dict(), path)
    _, _, _, _, c = compact_trainer(name, "fp32")
    c.load_state_dict(torch.load(path, map_location="cuda"))
    c.begin_epoch(c.epoch)
    out_c = c.step(xs[2], ys[2])
    assert float(out_a["loss"]) == float(out_c["loss"])
    assert torch.equal(a.model._flat, c.model._flat) and torch.equal(a.optimizer.exp_avg, c.optimizer.exp_avg)
    assert torch.equal(a.optimizer.exp_avg_sq, c.optimizer.exp_avg_sq) and a.global_step == c.global_step == 3
    # eval mode: the kernels and the bits of CompactVisionTransformer on the exported weights
    for prec in ("fp32", "bf16"):
        m = a.model if prec == "fp32" else CT.CompactTrainableViT(a.export(), precision="bf16")
        m.eval()
        with torch.no_grad():
            got, macs = m(xs[0])
            want, wmacs = CP.CompactVisionTransformer(m.export(), precision=prec)(xs[0])
        assert torch.equal(got, want) and macs == wmacs
    new = a.export()
    assert new["format"] == CP.FORMAT and new["version"] == 1 and new["cfg"] == ex["cfg"] and new["blocks"] == ex["blocks"]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_training_and_eval_forward_return_the_same_bits(precision):
    """One forward body serves both modes: the training forward (a buffer set per block, GELU' kept beside fc1's output) and the eval
    forward (one shared buffer set) launch the same kernels on the same operands, so the two heads' logits are equal bit for bit."""
    r, cfg, ex, teacher = fixture_export("stage2_micro_deit")
    S = ex["cfg"]["img_size"]
    x = torch.randn(4, 3, S, S, device="cuda", generator=torch.Generator(device="cuda").manual_seed(11))
    m = CT.CompactTrainableViT(ex, precision=precision)
    (o, od), _ = m(x)                                   # uvc_vit_compact_train_forward
    with torch.no_grad():
        (eo, eod), _ = m(x)                             # training mode without autograd: uvc_vit_compact_forward, heads kept apart
        m.eval()
        avg, _ = m(x)
    assert o.requires_grad and not eo.requires_grad
    assert torch.equal(o, eo) and torch.equal(od, eod) and torch.equal((o + od) / 2, avg)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_twenty_steps_on_one_batch_lower_the_loss(precision):
    r, cfg, ex, teacher = fixture_export("stage2_micro_none")
    args = trainer_args(r, ex, precision, train_batch_size=16, learning_rate=1e-3 * 512 / 16, distillation_type="none", warmup_epochs=0)
    tr = CT.CompactTrainer(args, ex)
    assert abs(args.lr - 1e-3) < 1e-12
    g = torch.Generator(device="cuda").manual_seed(3)
    S = ex["cfg"]["img_size"]
    x = torch.randn(16, 3, S, S, device="cuda", generator=g)
    y = torch.softmax(4 * torch.randn(16, ex["cfg"]["num_classes"], device="cuda", generator=g), -1)
    tr.begin_epoch(0)
    losses = [float(tr.step(x, y)["loss"]) for _ in range(20)]
    print(f"{precision}: loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert losses[-1] < losses[0]


def test_gpu_refusals():
    r, cfg, ex, teacher = fixture_export("stage2_micro_none")
    with pytest.raises(NotImplementedError):
        CT.CompactTrainableViT(ex, precision="bf16_f32resid")
    with pytest.raises(L.UvcHipError):
        CT.CompactTrainableViT(ex, device="cpu")
    # the C entry points refuse sequences above 256 tokens themselves: the workspace query answers -1
    from uvc_amd.model_distilled import uvc_vit_cfg
    lib = CT._bind()
    cfg577 = uvc_vit_cfg(384, 16, 3, 8, 64, 2, 1, 256, 1, L.UVC_F32)
    blocks = (L.uvc_compact_block * 1)()
    blocks[0].heads, blocks[0].v_dim, blocks[0].hidden = 1, 32, 128
    assert lib.uvc_vit_compact_workspace_bytes(C.byref(cfg577), blocks, 1, 2) > 0
    assert lib.uvc_vit_compact_train_workspace_bytes(C.byref(cfg577), blocks, 1, 2) == -1
    assert lib.uvc_vit_compact_train_layout(C.byref(cfg577), blocks, 1, None, None) == 3


def test_finetune_command_end_to_end(tmp_path, capsys):
    from uvc_amd.model_distilled import DistilledVisionTransformer
    m = DistilledVisionTransformer(enable_dist=0, img_size=64, patch_size=16, embed_dim=128, depth=3, num_heads=2, num_classes=16,
                                   precision="fp32", device="cuda")
    masks = CP.synthetic_masks(3, 128, 512, seed=3)
    masks["blocks.1.attn.proj.mask"][:, 64:] = 0                     # one head of block 1 pruned
    CP.apply_synthetic_masks(m, masks)
    ex = CP.export_compact(m)
    src, out = tmp_path / "in.compact.pt", tmp_path / "out.compact.pt"
    torch.save(ex, src)
    del m
    capsys.readouterr()
    CP.main(["finetune", "--compact", str(src), "--output", str(out), "--precision", "fp32", "--train_batch_size", "8", "--eval_batch_size", "8",
             "--epochs", "2", "--steps", "3", "--warmup_epochs", "1", "--learning_rate", "0.01", "--distillation_type", "soft"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["epochs"] == 2 and line["steps"] == 6 and line["params"] > 0 and len(line["blocks"]) == 3
    assert 0.0 <= line["top1_before"] <= 100.0 and 0.0 < line["top1_after"] <= 100.0
    assert line["macs_compact"] <= line["macs_compact_padded"] < line["macs_full"]
    tuned = CP.load_compact(out)
    assert tuned["version"] == 1 and tuned["blocks"] == ex["blocks"] and tuned["cfg"] == ex["cfg"]
    assert any(not torch.equal(tuned["state_dict"][k], v) for k, v in ex["state_dict"].items())
    acc = CP.main(["eval", "--compact", str(out), "--precision", "fp32", "--eval_batch_size", "8", "--eval_steps", "2"])
    assert 0.0 <= acc <= 100.0
