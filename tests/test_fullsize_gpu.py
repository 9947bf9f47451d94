"""GPU: BASELINE.json's metric configuration (DeiT-Tiny, per-GPU batch 512, M = 100 864 token rows) is too large for the
CPU oracle, so it is tied to the oracle-validated small runs through size-independent properties:
  * batch independence of the forward: image i of the 512-batch gets bit-identical logits to image i of an 8-batch
    (the 8-batch is the BASELINE config-1 shape the oracle / reference goldens cover),
  * linearity of the backward in the batch: grad(mean loss over 512) = mean of the grads of the two 256-halves,
  * determinism: the same step twice from the same state is bit-identical (split-M wgrads reduce in a fixed order),
  * clip: the applied update uses ||g * coef|| <= max_norm,
  * UVC engine at full size: ranks are permutations that sort the scores, masks are idempotent, count_mask is the sum of
    the mask buffers, and the flat gradient buffer is exactly the concatenation of the per-parameter .grad views
    (checksum of checksums)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B_FULL = 512


def make_trainer(precision, batch, **over):
    from uvc_amd.stage1 import Stage1Trainer, default_args
    torch.manual_seed(730)
    a = default_args(precision=precision, train_batch_size=batch, **over)
    tr = Stage1Trainer(a, device="cuda")
    mm = tr.minimax
    L, H, F = mm.n_layers, mm.num_heads, mm.dims.F
    rs = np.random.RandomState(731)
    s = np.zeros((L, 2), np.float32); s[:, 0] = rs.uniform(0, 0.6 * (H - 1) + 0.3, L); s[:, 1] = rs.uniform(0, 0.5 * F, L)
    mm.s.data.copy_(torch.from_numpy(s)); mm.r.data.copy_(torch.from_numpy(rs.uniform(0, 30.0, (L, H)).astype(np.float32)))
    mm.y.data.fill_(1.0); mm.p.data.fill_(1.0); mm.z.data.fill_(2.0)
    tr.begin_epoch(a.warmup_epochs + 1)
    return tr


def inputs(n, seed=5):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, 3, 224, 224, device="cuda", generator=g)
    y = torch.softmax(torch.randn(n, 1000, device="cuda", generator=g), -1)
    return x, y


def fixed_gate_noise(tr, seed=9):
    L = tr.model._cfg.depth
    e = torch.empty(L, 2, device="cuda").exponential_(generator=torch.Generator(device="cuda").manual_seed(seed))
    tr.model.exp_source = lambda shape, e=e: e.clone()


def fwd_bwd(tr, x, y):
    """student forward + loss + backward only (no optimiser step): returns logits, loss, flat gradient."""
    m = tr.model
    outputs, _ = m(x, -1, tr.args.patch_ratio)
    loss = tr.criterion(x, outputs, y)
    loss.backward()
    torch.cuda.synchronize()
    n = m._off.n_total
    return outputs[0].detach().clone(), float(loss.detach()), m._flat_grad[:n].clone()


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_forward_is_batch_independent_at_full_size(precision):
    tr = make_trainer(precision, B_FULL)
    fixed_gate_noise(tr)
    x, y = inputs(B_FULL)
    with torch.no_grad():
        tr.model.train()
        big = tr.model._run_forward(x, -1, 0.9, training=True)[0].clone()
        small = tr.model._run_forward(x[:8].contiguous(), -1, 0.9, training=True)[0].clone()
        t_big = tr.teacher(x)[0].clone()
        t_small = tr.teacher(x[:8].contiguous())[0].clone()
    assert torch.isfinite(big).all()
    assert torch.equal(big[:8], small), float((big[:8] - small).abs().max())
    assert torch.equal(t_big[:8], t_small)


# BASELINE configs 2 / 3 / 4 at their stated per-GPU shapes.  Config 3's "batch=1024" is read as the reference reads
# --train_batch_size: per GPU (data_utils.py:88-90); config 4 is DeiT-Base WITH the distillation token (N = 198, two heads) at
# the reference's per-GPU batch 128 (log/deit-base-log.log: global 512 on 4 ranks).
FULL = {
    "tiny512": dict(batch=512, over=dict()),
    "small1024": dict(batch=1024, over=dict(model_type="deit_small_patch16_224", budget=0.58)),
    "base128_dist": dict(batch=128, over=dict(model_type="deit_base_patch16_224", enable_deit=1)),
}


@pytest.mark.parametrize("precision,cfg", [("fp32", "tiny512"), ("bf16", "tiny512"), ("bf16", "small1024"), ("bf16", "base128_dist")])
def test_backward_is_linear_in_the_batch_and_deterministic_at_full_size(precision, cfg):
    """The bf16 mode selects different kernels from the float32 one (k_gemm_tn_dma wgrads, bf16 gradient streams), so the
    properties are checked in both.  Halving the batch doubles dL/dlogits exactly (a power of two survives the bf16 rounding
    of the gradient streams), so linearity holds to float32 summation order in bf16 as well; the stated tolerance leaves room
    for the per-row bf16 roundings that see differently-rounded float32 partial sums."""
    spec = FULL[cfg]
    B = spec["batch"]
    tr = make_trainer(precision, B, **spec["over"])
    fixed_gate_noise(tr)
    x, y = inputs(B)
    o1, loss, g_full = fwd_bwd(tr, x, y)
    o2, loss2, g_again = fwd_bwd(tr, x, y)
    assert torch.isfinite(g_full).all() and float(g_full.abs().max()) > 0
    assert loss == loss2 and torch.equal(o1, o2) and torch.equal(g_full, g_again), "the step is not deterministic"
    h = B // 2
    oa, la, ga = fwd_bwd(tr, x[:h].contiguous(), y[:h].contiguous())
    ob, lb, gb = fwd_bwd(tr, x[h:].contiguous(), y[h:].contiguous())
    assert torch.equal(o1[:h], oa) and torch.equal(o1[h:], ob), "training forward is not batch independent"
    assert abs(loss - 0.5 * (la + lb)) <= 1e-5 * abs(loss)
    ref = 0.5 * (ga.double() + gb.double())
    err = (g_full.double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    # (bf16, r5: 3e-3 instead of 2e-3 -- the attention backward is the one-pass kernel from 1024 heads up and the dq + dk/dv pair below, so the full batch
    #  and its halves may run DIFFERENT kernels, which round P / dS at different points: 2.2e-3 measured at DeiT-Base batch 128 against 64 + 64)
    assert err <= (2e-5 if precision == "fp32" else 3e-3) * scale, (err, scale)
    # checksum of checksums: the flat buffer is the concatenation of the parameters' .grad views
    total = sum(float(p.grad.double().sum()) for p in tr.model.parameters() if p.grad is not None)
    live = torch.zeros_like(g_full, dtype=torch.bool)
    for p, off in tr.model._slots():
        if p.grad is not None:
            live[off:off + p.numel()] = True
    now = tr.model._flat_grad[:g_full.numel()]              # the views alias the buffer: compare against its current content
    assert abs(total - float(now[live].double().sum())) <= 1e-9 * max(1.0, abs(total))


def test_full_step_properties_bf16():
    from uvc_amd.joint_train import count_mask
    from uvc_amd.uvc_utils import prune_w_mask
    tr = make_trainer("bf16", B_FULL)
    x, y = inputs(B_FULL)
    out = tr.step(x, y, zero_grad=False)
    assert np.isfinite(float(out["loss"])) and 0.0 < float(out["cur"]) < 1.5
    # clip: what AdamW consumed has norm <= max_grad_norm
    gn = float(out["gnorm"])
    coef = min(1.0, tr.args.max_grad_norm / (gn + 1e-6))
    assert gn * coef <= tr.args.max_grad_norm * (1 + 1e-6)
    mm = tr.minimax
    mm.refresh_scores()
    hd = mm.head_size
    for i, (sc, rk) in enumerate(zip(mm._sc, mm._rk)):         # ranks: a permutation per group that sorts the scores
        sc, rk = sc.cpu(), rk.cpu().long()
        if i == 0:                                             # proj input columns are ranked inside their head
            sc, rk = sc.reshape(-1, hd), rk.reshape(-1, hd)
        for l in range(sc.shape[0]):
            assert sorted(rk[l].tolist()) == list(range(sc.shape[1]))
            order = torch.empty_like(rk[l]); order[rk[l]] = torch.arange(sc.shape[1])
            srt = sc[l][order]
            assert bool((srt[1:] >= srt[:-1]).all())
    prune_w_mask(mm, tr.optimizer)
    m1 = [m.mask.clone() for grp in ("W1", "W2", "W3") for m in tr.uvc_layers[grp]]
    c1 = float(count_mask(tr.model))
    prune_w_mask(mm, tr.optimizer)
    m2 = [m.mask for grp in ("W1", "W2", "W3") for m in tr.uvc_layers[grp]]
    assert all(torch.equal(a, b) for a, b in zip(m1, m2)) and c1 == float(count_mask(tr.model))
    total = sum(float(mod.mask.sum()) for _, mod in tr.model.named_modules() if hasattr(mod, "mask")) / 1e6
    assert abs(total - c1) < 1e-6
    for t in m1:
        assert bool(((t == 0) | (t == 1)).all())


@pytest.mark.parametrize("cfg", ["small1024", "base128_dist"])
def test_eval_and_teacher_forward_batch_independent_at_config_3_and_4_shapes(cfg):
    """Eval-mode student (soft block gates, fixed noise) and teacher forwards of BASELINE configs 3 / 4 at their full per-GPU batch in
    bf16: image i gets bit-identical logits to image i of a 2-image batch -- the shape of the reference goldens
    small2_pruned / base2_deit (the latter with the distillation token: N = 198, the two-head average of :528-531)."""
    spec = FULL[cfg]
    B = spec["batch"]
    tr = make_trainer("bf16", B, **spec["over"])
    fixed_gate_noise(tr)               # block gating draws Gumbel noise in eval mode too (model_distilled.py:480-488)
    x, _ = inputs(B)
    tr.model.eval()
    with torch.no_grad():
        lb, _ = tr.model(x)
        ls, _ = tr.model(x[:2].contiguous())
        tb, _ = tr.teacher(x)
        ts, _ = tr.teacher(x[:2].contiguous())
    assert torch.isfinite(lb).all() and torch.equal(lb[:2], ls) and torch.equal(tb[:2], ts)
    # one full UVC-train step at this shape: finite, clip bound, resource in range
    tr.model.train()
    _, y = inputs(B, seed=6)
    out = tr.step(x, y, zero_grad=False)
    gn = float(out["gnorm"])
    assert np.isfinite(float(out["loss"])) and np.isfinite(gn) and 0.0 < float(out["cur"]) < 1.5
    if tr.model.num_tokens == 2:
        assert tr.model.head_dist.weight.grad is not None and float(tr.model.head_dist.weight.grad.abs().sum()) > 0
        assert tr.model.dist_token.grad is not None and float(tr.model.dist_token.grad.abs().sum()) > 0


@pytest.mark.parametrize("model_type,big", [("deit_small_patch16_224", 32), ("deit_base_patch16_224", 24)])
def test_forward_is_batch_independent_for_the_wider_models(model_type, big):
    """BASELINE configs 3 / 4 (DeiT-Small, DeiT-Base) in the bf16 mode: image i of a batch of `big` (>= 4096 token rows: the
    streaming K = 384 GEMMs for Small, the large-M paths for Base) gets bit-identical logits to image i of a 2-image batch (the
    shape the reference goldens cover), and a second run of the same step is bit-identical."""
    from uvc_amd.stage1 import Stage1Trainer, default_args
    torch.manual_seed(730)
    a = default_args(model_type=model_type, precision="bf16", train_batch_size=big)
    tr = Stage1Trainer(a, device="cuda")
    tr.begin_epoch(a.warmup_epochs + 1)
    fixed_gate_noise(tr)
    x, y = inputs(big)
    tr.model.eval()
    with torch.no_grad():
        lb, _ = tr.model(x)
        ls, _ = tr.model(x[:2].contiguous())
    assert torch.equal(lb[:2], ls)
    tr.model.train()
    a1 = fwd_bwd(tr, x, y)
    a2 = fwd_bwd(tr, x, y)
    assert torch.equal(a1[0], a2[0]) and a1[1] == a2[1] and torch.equal(a1[2], a2[2])


def test_stage2_step_at_the_bench_shape_with_compacted_mlps():
    """bench.py --stage 2 (per-GPU batch 512, half of the MLP units pruned, two blocks skipped): the compacted widths (512 of 768)
    tile the weight gradients differently from the dense ones -- more M splits, a larger split-M workspace.  A workspace sized for
    the dense shapes only made this step fail with 'uvc_gemm_tn: workspace too small' (r2f); it must run and give finite numbers."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from uvc_amd.post_train import Stage2Trainer, default_args
    a = default_args(model_type="deit_tiny_patch16_224", precision="bf16", train_batch_size=B_FULL)
    tr = Stage2Trainer(a, device="cuda", distributed=False, world_size=1)
    bench.stage2_checkpoint_state(tr.model)
    tr.mlp_widths = tr.model.set_mlp_compaction()
    assert any(0 < w < 768 for w in tr.mlp_widths)
    tr.begin_epoch(a.warmup_epochs + 1)
    x, y = inputs(B_FULL)
    out = None
    for _ in range(2):
        out = tr.step(x, y)
    torch.cuda.synchronize()
    assert np.isfinite(float(out["loss"])) and np.isfinite(float(out["gnorm"]))


def stage2_bench_trainer(batch):
    """The Stage-2 trainer of bench.py --stage 2 at another batch: bench.stage2_checkpoint_state's masks (one pruned head in every block), and -- as
    bench.py does, since the masks arrive after the constructor derived its tables -- the MLP compaction and the pruned-head table derived again."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from uvc_amd.post_train import Stage2Trainer, default_args
    torch.manual_seed(730)
    a = default_args(model_type="deit_tiny_patch16_224", precision="bf16", train_batch_size=batch)
    tr = Stage2Trainer(a, device="cuda", distributed=False, world_size=1)
    bench.stage2_checkpoint_state(tr.model)
    tr.mlp_widths = tr.model.set_mlp_compaction()
    tr.head_keep = tr.model.set_head_skipping()
    tr.model.skip_pruned_head_grads = tr.model._head_keep is not None
    hk = tr.model._head_keep
    assert hk is not None and tuple(hk.shape) == (12, 3) and bool((hk == 0).sum(1).eq(1).all()), hk      # one dead head in every block
    assert tr.model.skip_pruned_head_grads
    return a, tr


def test_stage2_backward_skipping_pruned_heads_is_exact_where_the_one_pass_kernel_runs():
    """test_stage2_gpu.py's test_training_backward_skipping_pruned_heads_is_exact at the size Stage 2 trains and is benchmarked at: DeiT-Tiny, bf16, batch
    344 = 1032 heads of N = 197, where uvc_attention_bwd picks the one-pass persistent kernel, whose workgroups draw runs of dead and live heads from a
    device counter.  With uvc_vit_io.head_keep_bwd the dq / dk / dv of the pruned heads are written as zeros instead of being computed; the step masks the
    weights first, so their dL/d(attention output) is exactly zero: the loss, the clip norm and every parameter gradient equal those of the step that
    computes them, bit for bit."""
    batch = 344
    assert batch * 3 >= 1024
    x, y = inputs(batch)
    res = []
    for skip in (True, False):
        a, tr = stage2_bench_trainer(batch)
        tr.model.skip_pruned_head_grads = skip
        tr.begin_epoch(a.warmup_epochs + 1)
        out = tr.step(x, y, zero_grad=False)
        torch.cuda.synchronize()
        res.append((out["loss"].detach().clone(), torch.as_tensor(out["gnorm"]).detach().clone(),
                    {n: p.grad.detach().clone() for n, p in tr.model.named_parameters() if p.grad is not None}))
        del tr, out
    assert bool(torch.isfinite(res[0][0]).all()) and bool(torch.isfinite(res[0][1]).all())
    assert torch.equal(res[0][0], res[1][0]), (res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1]), (res[0][1], res[1][1])
    assert res[0][2].keys() == res[1][2].keys() and any(n.endswith("attn.qkv.weight") for n in res[0][2])
    for n in res[0][2]:
        assert torch.equal(res[0][2][n], res[1][2][n]), n


def test_stage2_eval_forward_skipping_pruned_heads_is_exact_where_the_forward_is_persistent():
    """The same model, a no-grad forward of 176 images = 528 heads: with the table the plain attention forward runs, persistent above 512 heads (a few
    of its 512 workgroups walk a second head, with another h), and the last block's token-query kernel; without it (set_head_skipping(False)) the fused
    qkv + attention kernel.  The skipped heads' outputs only meet masked attn.proj columns, so the logits are equal bit for bit."""
    batch = 176
    assert batch * 3 > 512
    _, tr = stage2_bench_trainer(batch)
    m = tr.model
    m.apply_masks()
    x, _ = inputs(batch)
    m.eval()
    with torch.no_grad():
        out_skip, _ = m(x)
        assert m._head_keep is not None
        m.set_head_skipping(False)
        assert m._head_keep is None
        out_dense, _ = m(x)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out_skip.float()).all())
    assert torch.equal(out_skip, out_dense)


def test_t2t_14_config5_stage1_properties_at_the_benched_batch():
    """BASELINE config 5 AT THE BENCHED SHAPE: T2T-ViT-14 with patch + block gating, per-GPU batch 128, bf16 -- where the attention
    backward takes the dq + dk/dv pair (768 heads < 1024) and the D = 384 row kernels their production tiling; the oracle-checked runs of this model are at
    batch 2 / 8 / 24.  Tied to them by size-independent properties: the training forward of image i (logits, kept-token set) is bit-identical in the
    128-batch and in a 2-batch with the same per-image noise; the step is deterministic; the backward is linear in the batch (full = mean of halves),
    including the patch scorer's and the gate logits' gradients."""
    B = 128
    tr = make_trainer("bf16", B, model_type="t2t_vit_14", enable_patch_gating=2)
    m = tr.model
    L = m._cfg.depth
    P = (m._cfg.img_size // m._cfg.patch_size) ** 2
    gen = torch.Generator(device="cuda").manual_seed(9)
    e_gate = torch.empty(L, 2, device="cuda").exponential_(generator=gen)
    e_patch = torch.empty(B, P, device="cuda").exponential_(generator=gen)
    state = {"rows": slice(0, B)}

    def src(shape):
        shape = tuple(shape)
        if shape == (L, 2):
            return e_gate.clone()
        assert shape[1] == P, shape
        return e_patch[state["rows"]].contiguous().clone()

    m.exp_source = src
    tau, ratio = 1.0, tr.args.patch_ratio

    def fb(rows):
        state["rows"] = rows
        x_, y_ = x[rows].contiguous(), y[rows].contiguous()
        outputs, _ = m(x_, tau, ratio)
        kept = (m.last_patch_mask > 0.5).clone()
        loss = tr.criterion(x_, outputs, y_)
        loss.backward()
        torch.cuda.synchronize()
        return outputs[0].detach().clone(), kept, float(loss.detach()), m._flat_grad[:m._off.n_total].clone()

    x, y = inputs(B)
    o1, k1, l1, g1 = fb(slice(0, B))
    o2, k2, l2, g2 = fb(slice(0, B))
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    assert l1 == l2 and torch.equal(o1, o2) and torch.equal(k1, k2) and torch.equal(g1, g2), "the config-5 step is not deterministic at batch 128"
    n_kept = k1.sum(1).cpu()
    assert bool(((n_kept == int(ratio * P)) | (n_kept == int(ratio * P) + 1)).all()), n_kept      # 176 kept (+ token 0 when the top-k did not hold it)
    gw = m.gumbel.weight.grad
    assert gw is not None and float(gw.abs().sum()) > 0 and float(m.block_skip_gating.grad.abs().sum()) > 0
    os_, ks, _, _ = fb(slice(0, 2))
    assert torch.equal(o1[:2], os_) and torch.equal(k1[:2], ks), "image i of the 128-batch differs from image i of a 2-batch"
    h = B // 2
    oa, ka, la, ga = fb(slice(0, h))
    ob, kb, lb, gb = fb(slice(h, B))
    assert torch.equal(o1[:h], oa) and torch.equal(o1[h:], ob) and torch.equal(k1[:h], ka) and torch.equal(k1[h:], kb)
    assert abs(l1 - 0.5 * (la + lb)) <= 1e-5 * abs(l1)
    ref = 0.5 * (ga.double() + gb.double())
    err, scale = (g1.double() - ref).abs().max().item(), ref.abs().max().item()
    assert err <= 3e-3 * scale, (err, scale)
