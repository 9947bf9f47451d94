"""Thin tensor-level wrappers over the C-ABI kernels (include/uvc_kernels.h).  They check
devices/dtypes/contiguity, fill the argument structs and enqueue on torch's current HIP
stream.  No arithmetic happens in Python and there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib as L
from ._lib import (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GELU_GRAD, EPI_BIAS_GELU_GRAD_Q8, EPI_BIAS_GELU_OUT, EPI_BIAS_RESID, EPI_BIAS_RESID_GATE, EPI_DGELU,
                   EPI_MUL_AUX, EPI_MUL_AUX_Q8, EPI_NONE, Q8_LO, Q8_STEP, UVC_BF16, UVC_F32)

__all__ = ["EPI_NONE", "EPI_BIAS", "EPI_BIAS_GELU", "EPI_BIAS_RESID", "EPI_BIAS_RESID_GATE", "EPI_DGELU", "UVC_F32",
           "UVC_BF16"]


def tdtype(dtype: int) -> torch.dtype:
    return torch.float32 if dtype == UVC_F32 else torch.bfloat16


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        L.require_cuda(t)
        if not t.is_contiguous():
            raise L.UvcHipError("kernel operands must be contiguous")


def _is_f32(t) -> int:
    return int(t.dtype == torch.float32)


def gemm_nt(A, B, C_, *, dtype, epilogue=EPI_NONE, bias=None, R=None, R2=None, aux=None, gate=None, C2=None, alpha=1.0,
            alpha_ptr=None, M=None, N=None, K=None, lda=None, ldb=None, ldc=None, ldr=None, ldaux=None, force_generic=False,
            ln_gamma=None, ln_beta=None, ln_out=None, ln_mean=None, ln_rstd=None, ln_eps=1e-6):
    """C[M,N] = epi(A[M,K] . B[N,K]^T).  ln_out (where uvc_gemm_nt_ln_supported): also LayerNorm(C rows; ln_gamma, ln_beta) in the
    compute dtype, with ln_mean / ln_rstd."""
    _chk(A, B, C_, bias, R, R2, aux, gate, C2, alpha_ptr, ln_gamma, ln_beta, ln_out, ln_mean, ln_rstd)
    a = L.uvc_gemm_nt_args()
    a.ln_gamma, a.ln_beta, a.ln_out, a.ln_mean, a.ln_rstd, a.ln_eps = L.ptr(ln_gamma), L.ptr(ln_beta), L.ptr(ln_out), L.ptr(ln_mean), L.ptr(ln_rstd), ln_eps
    a.A, a.B, a.C, a.C2 = L.ptr(A), L.ptr(B), L.ptr(C_), L.ptr(C2)
    a.bias, a.R, a.R2, a.aux, a.gate, a.alpha_ptr = L.ptr(bias), L.ptr(R), L.ptr(R2), L.ptr(aux), L.ptr(gate), L.ptr(alpha_ptr)
    a.alpha = alpha
    a.M = M if M is not None else A.shape[0]
    a.K = K if K is not None else A.shape[-1]
    a.N = N if N is not None else B.shape[0]
    a.lda = lda if lda is not None else a.K
    a.ldb = ldb if ldb is not None else a.K
    a.ldc = ldc if ldc is not None else a.N
    a.ldr = ldr if ldr is not None else a.ldc
    a.ldaux = ldaux if ldaux is not None else a.ldc
    a.dtype, a.a_is_f32, a.c_is_f32, a.epilogue = dtype, _is_f32(A), _is_f32(C_), epilogue
    for t in (R, R2):
        if t is not None and t.dtype != C_.dtype:
            raise L.UvcHipError("gemm_nt: the residual operands R / R2 have C's element type")
    a.force_generic = int(force_generic)
    a.r_is_f32 = _is_f32(R) if R is not None else 0
    L.check(L.lib().uvc_gemm_nt(C.byref(a), L.cur_stream()), "uvc_gemm_nt")


def gemm_tn_workspace_bytes(M, N1, N2) -> int:
    b = C.c_int64()
    s = C.c_int32()
    L.check(L.lib().uvc_gemm_tn_workspace_bytes(M, N1, N2, C.byref(b), C.byref(s)), "uvc_gemm_tn_workspace_bytes")
    return int(b.value)


def gemm_tn(A, B, C_, workspace, *, dtype, alpha=1.0, alpha_ptr=None, beta=0.0, M=None, N1=None, N2=None, lda=None,
            ldb=None, ldc=None, colsum_out=None, variant=0):
    """C[N1,N2] = beta*C + alpha * A[M,N1]^T . B[M,N2]  (+ optional colsum_out[N1] = beta*old + alpha*colsum(A)).  ldc: row stride of C (default N2)."""
    _chk(A, B, C_, workspace, alpha_ptr, colsum_out)
    a = L.uvc_gemm_tn_args()
    a.A, a.B, a.C, a.workspace = L.ptr(A), L.ptr(B), L.ptr(C_), L.ptr(workspace)
    a.workspace_bytes = workspace.numel() * workspace.element_size()
    a.alpha_ptr, a.alpha, a.beta, a.colsum_out = L.ptr(alpha_ptr), alpha, beta, L.ptr(colsum_out)
    a.M = M if M is not None else A.shape[0]
    a.N1 = N1 if N1 is not None else A.shape[1]
    a.N2 = N2 if N2 is not None else B.shape[1]
    a.lda = lda if lda is not None else a.N1
    a.ldb = ldb if ldb is not None else a.N2
    a.ldc = ldc if ldc is not None else a.N2
    a.dtype, a.a_is_f32 = dtype, _is_f32(A)
    a.variant = int(variant)
    L.check(L.lib().uvc_gemm_tn(C.byref(a), L.cur_stream()), "uvc_gemm_tn")


def _attn_args(qkv, o, lse, B, N, H, dtype, dout=None, dqkv=None, delta=None):
    _chk(qkv, o, lse, dout, dqkv, delta)
    a = L.uvc_attn_args()
    a.qkv, a.o, a.lse, a.dout, a.dqkv, a.delta = (L.ptr(t) for t in (qkv, o, lse, dout, dqkv, delta))
    a.B, a.N, a.H, a.head_dim, a.dtype = B, N, H, 64, dtype
    a.scale = 64 ** -0.5
    return a


def attention_fwd(qkv, o, lse, B, N, H, dtype, head_keep=None, v_dim=0):
    """v_dim 16 / 32 / 48: the compact layout (include/uvc_kernels.h: uvc_attn_args.v_dim), qkv rows [q H*64 | k H*64 | v H*v_dim], o [B, N, H*v_dim]."""
    a = _attn_args(qkv, o, lse, B, N, H, dtype)
    a.v_dim = int(v_dim)
    if head_keep is not None:
        _chk(head_keep)
        a.head_keep = L.ptr(head_keep)
    L.check(L.lib().uvc_attention_fwd(C.byref(a), L.cur_stream()), "uvc_attention_fwd")


def attention_bwd(qkv, o, lse, dout, dqkv, delta, B, N, H, dtype, head_keep=None, variant=0, grid=0):
    a = _attn_args(qkv, o, lse, B, N, H, dtype, dout, dqkv, delta)
    a.variant, a.grid = int(variant), int(grid)
    if head_keep is not None:
        _chk(head_keep)
        a.head_keep = L.ptr(head_keep)
    L.check(L.lib().uvc_attention_bwd(C.byref(a), L.cur_stream()), "uvc_attention_bwd")


def attention_bwd_vdim(qkv, o, lse, dout, dqkv, delta, B, N, H, v_dim, dtype):
    """The attention backward at a compact model's value width (include/uvc_kernels.h: uvc_attention_bwd_vdim): qkv / dqkv rows
    [q H*64 | k H*64 | v H*v_dim], o / dout [B, N, H*v_dim].  v_dim 16, 32, 48 or 64, N <= 256."""
    a = _attn_args(qkv, o, lse, B, N, H, dtype, dout, dqkv, delta)
    a.v_dim = int(v_dim)
    L.check(L.lib().uvc_attention_bwd_vdim(C.byref(a), L.cur_stream()), "uvc_attention_bwd_vdim")


def attention_rollout_step(qkv, lse, r_in, r_out, B, N, H, v_dim, dtype, keep=0.5, mix=0.5):
    """One attention-rollout step (include/uvc_kernels.h: uvc_attention_rollout_step): r_out = keep * r_in + (mix / H) * sum_h P_h^T r_in over
    qkv rows [q H*64 | k H*64 | v H*v_dim] and the forward's lse [B, H, N]; r_in / r_out float32 [B, N], distinct buffers."""
    _chk(qkv, lse, r_in, r_out)
    a = L.uvc_attn_rollout_args()
    a.qkv, a.lse, a.r_in, a.r_out = (L.ptr(t) for t in (qkv, lse, r_in, r_out))
    a.B, a.N, a.H, a.head_dim, a.v_dim, a.dtype = B, N, H, 64, int(v_dim), dtype
    a.scale, a.keep, a.mix = 64 ** -0.5, float(keep), float(mix)
    L.check(L.lib().uvc_attention_rollout_step(C.byref(a), L.cur_stream()), "uvc_attention_rollout_step")


def attention_relevance_step(qkv, lse, dout, r_in, r_out, B, N, H, v_dim, dtype, keep=1.0, mix=1.0):
    """One step of the gradient-weighted rollout (include/uvc_kernels.h: uvc_attention_relevance_step):
    r_out = keep * r_in + (mix / H) * sum_h ((P_h * dP_h)^+)^T r_in with dP_h = dout_h v_h^T, over qkv rows [q H*64 | k H*64 | v H*v_dim],
    the forward's lse [B, H, N] and dout [B, N, H*v_dim] in the operand type; r_in / r_out float32 [B, N], distinct buffers."""
    _chk(qkv, lse, dout, r_in, r_out)
    a = L.uvc_attn_relevance_args()
    a.qkv, a.lse, a.dout, a.r_in, a.r_out = (L.ptr(t) for t in (qkv, lse, dout, r_in, r_out))
    a.B, a.N, a.H, a.head_dim, a.v_dim, a.dtype = B, N, H, 64, int(v_dim), dtype
    a.scale, a.keep, a.mix = 64 ** -0.5, float(keep), float(mix)
    L.check(L.lib().uvc_attention_relevance_step(C.byref(a), L.cur_stream()), "uvc_attention_relevance_step")


def qkv_attention_supported(B, N, H, D, dtype):
    return bool(L.lib().uvc_qkv_attention_supported(B, N, H, D, dtype))


def qkv_attention_fwd(h, w, bias, o, lse, B, N, H, dtype, qkv=None, grid=0):
    """The qkv Linear + attention forward as one kernel (include/uvc_kernels.h: uvc_qkv_attention_fwd); qkv is written when given."""
    _chk(h, w, o)
    a = L.uvc_qkv_attn_args()
    a.h, a.w, a.bias, a.qkv, a.o, a.lse = (L.ptr(t) for t in (h, w, bias, qkv, o, lse))
    a.B, a.N, a.H, a.D, a.dtype, a.scale, a.grid = B, N, H, H * 64, dtype, 64 ** -0.5, int(grid)
    L.check(L.lib().uvc_qkv_attention_fwd(C.byref(a), L.cur_stream()), "uvc_qkv_attention_fwd")


def _attn_tok_args(qkv, o, B, N, H, ntok, dtype, dout=None, dqkv=None):
    a = L.uvc_attn_tok_args()
    for t in (qkv, o, dout, dqkv):
        if t is not None:
            _chk(t)
    a.qkv, a.o = L.ptr(qkv), L.ptr(o)
    a.dout, a.dqkv = L.ptr(dout), L.ptr(dqkv)
    a.B, a.N, a.H, a.head_dim, a.ntok, a.dtype, a.scale = B, N, H, 64, ntok, dtype, 0.125
    return a


def attention_tok_fwd(qkv, o, B, N, H, ntok, dtype, head_keep=None):
    """Attention of the first ntok queries of every (image, head): o is [B, ntok, H*64]."""
    a = _attn_tok_args(qkv, o, B, N, H, ntok, dtype)
    if head_keep is not None:
        _chk(head_keep)
        a.head_keep = L.ptr(head_keep)
    L.check(L.lib().uvc_attention_tok_fwd(C.byref(a), L.cur_stream()), "uvc_attention_tok_fwd")


def attention_tok_bwd(qkv, o, dout, dqkv, B, N, H, ntok, dtype, head_keep=None):
    a = _attn_tok_args(qkv, o, B, N, H, ntok, dtype, dout, dqkv)
    if head_keep is not None:
        _chk(head_keep)
        a.head_keep = L.ptr(head_keep)
    L.check(L.lib().uvc_attention_tok_bwd(C.byref(a), L.cur_stream()), "uvc_attention_tok_bwd")


def copy_row_groups(src, dst, groups, group_bytes, src_group_stride, dst_group_stride):
    _chk(src)
    _chk(dst)
    L.check(L.lib().uvc_copy_row_groups(L.ptr(src), L.ptr(dst), groups, group_bytes, src_group_stride, dst_group_stride, L.cur_stream()),
            "uvc_copy_row_groups")


def _ln_args(x, gamma, beta, rows, D, dtype, rows_per_group=1, group_stride=None, eps=1e-6):
    a = L.uvc_ln_args()
    a.x, a.gamma, a.beta = L.ptr(x), L.ptr(gamma), L.ptr(beta)
    a.rows, a.D, a.rows_per_group, a.dtype = rows, D, rows_per_group, dtype
    a.group_stride = group_stride if group_stride is not None else D * rows_per_group
    a.eps = eps
    a.x_lowp = int(not _is_f32(x))                   # bf16 residual stream
    return a


def layernorm_fwd(x, gamma, beta, y, mean, rstd, rows, D, dtype, rows_per_group=1, group_stride=None, eps=1e-6):
    _chk(x, gamma, beta, y, mean, rstd)
    a = _ln_args(x, gamma, beta, rows, D, dtype, rows_per_group, group_stride, eps)
    a.y, a.mean, a.rstd, a.y_is_f32 = L.ptr(y), L.ptr(mean), L.ptr(rstd), _is_f32(y)
    L.check(L.lib().uvc_layernorm_fwd(C.byref(a), L.cur_stream()), "uvc_layernorm_fwd")


def layernorm_bwd_blocks(rows) -> int:
    return int(L.lib().uvc_layernorm_bwd_blocks(rows))


def layernorm_bwd(dy, x, gamma, mean, rstd, dx, partial, dgamma, dbeta, rows, D, dtype, *, add1=None, a1=None, add2=None,
                  a2=None, dots=None, beta_acc=0.0, rows_per_group=1, group_stride=None, eps=1e-6):
    _chk(dy, x, gamma, mean, rstd, dx, partial, dgamma, dbeta, add1, a1, add2, a2, dots)
    a = _ln_args(x, gamma, None, rows, D, dtype, rows_per_group, group_stride, eps)
    a.mean, a.rstd, a.dy, a.dx = L.ptr(mean), L.ptr(rstd), L.ptr(dy), L.ptr(dx)
    a.add1, a.a1, a.add2, a.a2 = L.ptr(add1), L.ptr(a1), L.ptr(add2), L.ptr(a2)
    a.partial, a.dgamma, a.dbeta, a.dots = L.ptr(partial), L.ptr(dgamma), L.ptr(dbeta), L.ptr(dots)
    a.beta_acc, a.dy_is_f32 = beta_acc, _is_f32(dy)
    a.g_lowp = int(not _is_f32(dx))          # gradient stream (dx, add1, add2) kept in bf16
    for t in (add1, add2):
        if t is not None and t.dtype != dx.dtype:
            raise L.UvcHipError("layernorm_bwd: add1/add2 must have dx's element type")
    L.check(L.lib().uvc_layernorm_bwd(C.byref(a), L.cur_stream()), "uvc_layernorm_bwd")


def gemm_nt_q8_supported(M, hidden, embed_dim, dtype) -> bool:
    """Where the one-byte GELU'(a) epilogues exist (EPI_BIAS_GELU_GRAD_Q8 / EPI_MUL_AUX_Q8)."""
    return bool(L.lib().uvc_gemm_nt_q8_supported(M, hidden, embed_dim, dtype))


def gemm_nt_rows_supported(M, N, K, dtype, epilogue, lda=None, ldb=None, ldc=None) -> bool:
    """Where gemm_nt (force_generic off, no ln_out) runs the row-panel kernel of few rows (M <= 1024, K <= 1024, bf16 compute)."""
    return bool(L.lib().uvc_gemm_nt_rows_supported(M, N, K, K if lda is None else lda, K if ldb is None else ldb, N if ldc is None else ldc, dtype, epilogue))


def _route(fn, args, fields):
    """(status, route) of a route query: args' members from `fields`; the route as a dict with the family's name and its kernel template."""
    for k, v in fields.items():
        setattr(args, k, v)
    r = L.uvc_gemm_route()
    rc = getattr(L.lib(), fn)(C.byref(args), C.byref(r))
    out = {n: getattr(r, n) for n, _ in r._fields_}
    out["family"] = L.ROUTE_FAMILIES[r.family]
    out["kernel"] = L.lib().uvc_gemm_route_kernel(r.family).decode()
    return rc, out


def gemm_nt_route(**fields):
    """Which kernel uvc_gemm_nt would run for the uvc_gemm_nt_args members given (integers; pointer members are never dereferenced, so any non-null
    address stands for a tensor) -- no launch, no GPU.  Returns (status, route); the route means something where status is 0."""
    return _route("uvc_gemm_nt_route", L.uvc_gemm_nt_args(), fields)


def gemm_tn_route(**fields):
    """The same for uvc_gemm_tn: kernel family, tile configuration, splits and rows per split."""
    return _route("uvc_gemm_tn_route", L.uvc_gemm_tn_args(), fields)


def gemm_lnbwd_supported(M, D, K, dtype) -> bool:
    return bool(L.lib().uvc_gemm_lnbwd_supported(M, D, K, dtype))


def gemm_nt_lnbwd(A, Wt, x, mean, rstd, gamma, dx, partial, dgamma, dbeta, *, add1=None, a1=None, add2=None, a2=None, dots=None, beta_acc=0.0,
                  variant=0):
    """dx = LN'(A . Wt^T; x, mean, rstd, gamma) + a1*add1 + a2*add2 in one kernel (include/uvc_kernels.h: uvc_gemm_nt_lnbwd), then the
    batched finish of dgamma / dbeta / dots."""
    _chk(A, Wt, x, mean, rstd, gamma, dx, partial, dgamma, dbeta, add1, a1, add2, a2, dots)
    a = L.uvc_gemm_lnbwd_args()
    a.A, a.W, a.x, a.mean, a.rstd, a.gamma = (L.ptr(t) for t in (A, Wt, x, mean, rstd, gamma))
    a.add1, a.a1, a.add2, a.a2, a.dx, a.partial = (L.ptr(t) for t in (add1, a1, add2, a2, dx, partial))
    a.M, a.D, a.K, a.dtype, a.variant, a.x_lowp = A.shape[0], x.shape[1], A.shape[1], UVC_BF16, int(variant), int(not _is_f32(x))
    L.check(L.lib().uvc_gemm_nt_lnbwd(C.byref(a), L.cur_stream()), "uvc_gemm_nt_lnbwd")
    item = (L.uvc_ln_reduce_item * 1)()
    item[0].partial, item[0].dgamma, item[0].dbeta, item[0].dots = L.ptr(partial), L.ptr(dgamma), L.ptr(dbeta), L.ptr(dots)
    item[0].nblocks = int(L.lib().uvc_gemm_lnbwd_nblocks(a.M))
    L.check(L.lib().uvc_layernorm_bwd_reduce_batch(item, 1, a.D, beta_acc, L.cur_stream()), "uvc_layernorm_bwd_reduce_batch")


def mlp_fused_fwd(x, gamma, beta, w1, b1, w2, b2, out, eps=1e-6, *, x_prev=None, gate=None, h=None, mean=None, rstd=None, gp=None, u=None,
                  next_gamma=None, next_beta=None, next_h=None, next_mean=None, next_rstd=None):
    """out = d1 * (x + fc2(GELU(fc1(LayerNorm(x))))) + d0 * x_prev for [M, 192] float32 rows; w1 [F,192] / w2 [192,F] bf16.
    Training form: h / mean / rstd / gp / u receive LayerNorm(x), its statistics, GELU'(a) and GELU(a).
    next_h (bf16 [M,192], optional): LayerNorm(out; next_gamma, next_beta) -- the next block's norm1 -- with its statistics in
    next_mean / next_rstd when given."""
    _chk(x, gamma, beta, w1, b1, w2, b2, out, x_prev, gate, h, mean, rstd, gp, u, next_gamma, next_beta, next_h, next_mean, next_rstd)
    a = L.uvc_mlp_args()
    a.next_gamma, a.next_beta, a.next_h, a.next_mean, a.next_rstd = (L.ptr(t) for t in (next_gamma, next_beta, next_h, next_mean, next_rstd))
    a.x, a.gamma, a.beta, a.w1, a.b1, a.w2, a.b2, a.out = (L.ptr(t) for t in (x, gamma, beta, w1, b1, w2, b2, out))
    a.x_prev, a.gate, a.h, a.mean, a.rstd, a.gp, a.u = (L.ptr(t) for t in (x_prev, gate, h, mean, rstd, gp, u))
    a.M, a.D, a.F, a.eps = x.shape[0], x.shape[1], w1.shape[0], eps
    a.rows_lowp = int(not _is_f32(x))                # bf16 residual stream: x, out, x_prev are bf16 rows
    for t in (out, x_prev):
        if t is not None and t.dtype != x.dtype:
            raise L.UvcHipError("mlp_fused_fwd: x, out and x_prev must share one element type")
    L.check(L.lib().uvc_mlp_fused_fwd(C.byref(a), L.cur_stream()), "uvc_mlp_fused_fwd")


def distill_loss(o, o_kd, y_soft, teacher, loss, d_o, d_okd, row_scratch, alpha, tau, kind=1):
    _chk(o, o_kd, y_soft, teacher, loss, d_o, d_okd, row_scratch)
    a = L.uvc_loss_args()
    a.o, a.o_kd, a.y_soft, a.teacher = L.ptr(o), L.ptr(o_kd), L.ptr(y_soft), L.ptr(teacher)
    a.loss, a.d_o, a.d_okd, a.row_scratch = L.ptr(loss), L.ptr(d_o), L.ptr(d_okd), L.ptr(row_scratch)
    a.alpha, a.tau, a.B, a.C, a.kind = alpha, tau, o.shape[0], o.shape[1], kind
    L.check(L.lib().uvc_distill_loss(C.byref(a), L.cur_stream()), "uvc_distill_loss")


def grad_sqnorm(g, partial, sq, accumulate=False, n=None):
    """sq: float32[2] -- sq[0] = sum of squares (accumulated over calls with accumulate=True), sq[1] = its square root."""
    _chk(g, partial, sq)
    if sq.numel() < 2:
        raise L.UvcHipError("grad_sqnorm: sq must hold 2 floats (sum of squares, norm)")
    L.check(L.lib().uvc_grad_sqnorm(L.ptr(g), n if n is not None else g.numel(), L.ptr(partial), L.ptr(sq),
                                    int(accumulate), L.cur_stream()), "uvc_grad_sqnorm")


def adamw_step(p, g, m, v, sq, *, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.05, max_norm=1.0,
               p_shadow=None, gnorm_out=None, n=None, flags=None):
    _chk(p, g, m, v, sq, p_shadow, gnorm_out, flags)
    a = L.uvc_adamw_args()
    a.p, a.g, a.m, a.v, a.p_shadow, a.sq, a.gnorm_out = (L.ptr(t) for t in (p, g, m, v, p_shadow, sq, gnorm_out))
    a.n = n if n is not None else p.numel()
    a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.max_norm, a.step = lr, beta1, beta2, eps, weight_decay, max_norm, step
    a.flags = L.ptr(flags)
    L.check(L.lib().uvc_adamw_step(C.byref(a), L.cur_stream()), "uvc_adamw_step")


def scale_by_clip(g, sq, max_norm):
    _chk(g, sq)
    L.check(L.lib().uvc_scale_by_clip(L.ptr(g), g.numel(), L.ptr(sq), max_norm, L.cur_stream()), "uvc_scale_by_clip")


def patchify(x, out, P, dtype):
    _chk(x, out)
    B, Cc, S, _ = x.shape
    L.check(L.lib().uvc_patchify(L.ptr(x), L.ptr(out), B, Cc, S, P, dtype, L.cur_stream()), "uvc_patchify")


def assemble_tokens(pe, cls, dist, pos, row_mask, tok, B, P, D, ntok):
    _chk(pe, cls, dist, pos, row_mask, tok)
    L.check(L.lib().uvc_assemble_tokens(L.ptr(pe), L.ptr(cls), L.ptr(dist), L.ptr(pos), L.ptr(row_mask), L.ptr(tok), B, P,
                                        D, ntok, int(not _is_f32(tok)), L.cur_stream()), "uvc_assemble_tokens")


def assemble_tokens_bwd(dtok, pe, row_mask, dpe, dpos, dcls, ddist, dmask, B, P, D, ntok, dtype, beta_acc=0.0):
    _chk(dtok, pe, row_mask, dpe, dpos, dcls, ddist, dmask)
    L.check(L.lib().uvc_assemble_tokens_bwd(L.ptr(dtok), L.ptr(pe), L.ptr(row_mask), L.ptr(dpe), L.ptr(dpos), L.ptr(dcls),
                                            L.ptr(ddist), L.ptr(dmask), B, P, D, ntok, dtype, _is_f32(dpe), int(not _is_f32(dtok)), beta_acc,
                                            L.cur_stream()), "uvc_assemble_tokens_bwd")


def colsum_blocks(M) -> int:
    return int(L.lib().uvc_colsum_blocks(M))


def colsum(X, partial, out, dtype, *, M=None, N=None, ldx=None, alpha=1.0, alpha_ptr=None, beta=0.0, row_weight=None):
    _chk(X, partial, out, alpha_ptr, row_weight)
    M = M if M is not None else X.shape[0]
    N = N if N is not None else X.shape[1]
    L.check(L.lib().uvc_colsum(L.ptr(X), M, N, ldx if ldx is not None else N, dtype, _is_f32(X), L.ptr(partial), L.ptr(out),
                               alpha, L.ptr(alpha_ptr), beta, L.ptr(row_weight), L.cur_stream()), "uvc_colsum")


def patch_gate_sigmoid(pg, mask, B, P, hard):
    _chk(pg, mask)
    L.check(L.lib().uvc_patch_gate_sigmoid(L.ptr(pg), L.ptr(mask), B, P, int(bool(hard)), L.cur_stream()), "uvc_patch_gate_sigmoid")


def patch_gate_sigmoid_bwd(pg, dmask, dpg, B, P, beta_acc=0.0):
    _chk(pg, dmask, dpg)
    L.check(L.lib().uvc_patch_gate_sigmoid_bwd(L.ptr(pg), L.ptr(dmask), L.ptr(dpg), B, P, beta_acc, L.cur_stream()),
            "uvc_patch_gate_sigmoid_bwd")


def patch_scores(pe, w, bias, scores, rows, D):
    _chk(pe, w, bias, scores)
    L.check(L.lib().uvc_patch_scores(L.ptr(pe), L.ptr(w), L.ptr(bias), L.ptr(scores), rows, D, L.cur_stream()), "uvc_patch_scores")


def patch_topk_mask(scores, e, mask, ysoft, psoft, B, P, k, tau):
    _chk(scores, e, mask, ysoft, psoft)
    L.check(L.lib().uvc_patch_topk_mask(L.ptr(scores), L.ptr(e), L.ptr(mask), L.ptr(ysoft), L.ptr(psoft), B, P, k, tau,
                                        L.cur_stream()), "uvc_patch_topk_mask")


def patch_topk_mask_bwd(dmask, ysoft, psoft, dscores, B, P, tau):
    _chk(dmask, ysoft, psoft, dscores)
    L.check(L.lib().uvc_patch_topk_mask_bwd(L.ptr(dmask), L.ptr(ysoft), L.ptr(psoft), L.ptr(dscores), B, P, tau, L.cur_stream()),
            "uvc_patch_topk_mask_bwd")


def apply_masks(params, mask):
    _chk(params, mask)
    L.check(L.lib().uvc_apply_masks(L.ptr(params), L.ptr(mask), params.numel(), L.cur_stream()), "uvc_apply_masks")


def mlp_gather_shadows(W1, b1, W2, idx, w1c, w1t, w2c, w2t, b1c, D, F, width, dtype):
    """Compact operand copies of an MLP (include/uvc_kernels.h: uvc_mlp_gather_shadows): idx int32 [width], copies of type T, b1c float32."""
    _chk(W1, b1, W2, idx, w1c, w1t, w2c, w2t, b1c)
    L.check(L.lib().uvc_mlp_gather_shadows(L.ptr(W1), L.ptr(b1), L.ptr(W2), L.ptr(idx), D, F, width, L.ptr(w1c), L.ptr(w1t), L.ptr(w2c),
                                           L.ptr(w2t), L.ptr(b1c), dtype, L.cur_stream()), "uvc_mlp_gather_shadows")


def mlp_scatter_grads(dw1c, dw2c, db1c, inv, b1, db2, dW1, dW2, db1, D, F, width, dtype, beta_acc=0.0):
    """Compact weight gradients expanded into the full tensors (uvc_mlp_scatter_grads): inv int32 [F] (slot or -1), all else float32."""
    _chk(dw1c, dw2c, db1c, inv, b1, db2, dW1, dW2, db1)
    L.check(L.lib().uvc_mlp_scatter_grads(L.ptr(dw1c), L.ptr(dw2c), L.ptr(db1c), L.ptr(inv), L.ptr(b1), L.ptr(db2), D, F, width, L.ptr(dW1),
                                          L.ptr(dW2), L.ptr(db1), beta_acc, dtype, L.cur_stream()), "uvc_mlp_scatter_grads")


def add_outer(X, row_weight, w, rows, D, dtype):
    _chk(X, row_weight, w)
    L.check(L.lib().uvc_add_outer(L.ptr(X), L.ptr(row_weight), L.ptr(w), rows, D, dtype, _is_f32(X), L.cur_stream()), "uvc_add_outer")


def cast_transpose(W, R, Cc, w_cast, wt, dtype):
    _chk(W, w_cast, wt)
    L.check(L.lib().uvc_cast_transpose(L.ptr(W), R, Cc, L.ptr(w_cast), L.ptr(wt), dtype, L.cur_stream()), "uvc_cast_transpose")


def gate_distrib(g, e, d, Lb, mode, eps):
    _chk(g, e, d)
    L.check(L.lib().uvc_gate_distrib(L.ptr(g), L.ptr(e), L.ptr(d), Lb, mode, eps, L.cur_stream()), "uvc_gate_distrib")


def gate_grad(g, d, dots, dg, Lb, mode, eps, beta_acc=0.0):
    _chk(g, d, dots, dg)
    L.check(L.lib().uvc_gate_grad(L.ptr(g), L.ptr(d), L.ptr(dots), L.ptr(dg), Lb, mode, eps, beta_acc, L.cur_stream()),
            "uvc_gate_grad")


# ---- T2T tokens-to-token front end (include/uvc_t2t.h) --------------------------------------------
def _unfold_args(src, strides, B, Cc, H, W, k, s, p, ldo, dtype):
    a = L.uvc_unfold_args()
    a.src = L.ptr(src)
    a.sb, a.sc, a.sh, a.sw = strides
    a.B, a.C, a.H, a.W, a.k, a.s, a.p, a.ldo, a.dtype = B, Cc, H, W, k, s, p, ldo, dtype
    return a


def unfold_out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def unfold_ln_fwd(src, strides, B, Cc, H, W, k, s, p, out, dtype, *, gamma=None, beta=None, mean=None, rstd=None, eps=1e-5):
    """out[B*L, ldo] = (LayerNorm of) the soft split rows of `src` (element strides (sb, sc, sh, sw)); ldo = out.shape[1]."""
    _chk(src, out, gamma, beta, mean, rstd)
    a = _unfold_args(src, strides, B, Cc, H, W, k, s, p, out.shape[1], dtype)
    a.out, a.out_is_f32 = L.ptr(out), _is_f32(out)
    a.gamma, a.beta, a.mean, a.rstd, a.eps = L.ptr(gamma), L.ptr(beta), L.ptr(mean), L.ptr(rstd), eps
    L.check(L.lib().uvc_unfold_ln_fwd(C.byref(a), L.cur_stream()), "uvc_unfold_ln_fwd")


def unfold_bwd_blocks(rows) -> int:
    return int(L.lib().uvc_unfold_bwd_blocks(rows))


def unfold_ln_bwd(src, strides, B, Cc, H, W, k, s, p, dy, dtype, *, gamma, mean, rstd, partial, dgamma, dbeta, dxu=None, beta_acc=0.0, eps=1e-5,
                  dxu_tap_major=False):
    """dxu_tap_major (token-major sources with 64 channels): dxu leaves as [rows][k*k][C] for fold_tokens(..., tap_major=True)."""
    _chk(src, dy, gamma, mean, rstd, partial, dgamma, dbeta, dxu)
    a = _unfold_args(src, strides, B, Cc, H, W, k, s, p, dy.shape[1], dtype)
    a.gamma, a.mean, a.rstd, a.eps = L.ptr(gamma), L.ptr(mean), L.ptr(rstd), eps
    a.dy, a.dy_is_f32, a.dxu, a.partial = L.ptr(dy), _is_f32(dy), L.ptr(dxu), L.ptr(partial)
    a.dgamma, a.dbeta, a.beta_acc = L.ptr(dgamma), L.ptr(dbeta), beta_acc
    a.dxu_tap_major = int(bool(dxu_tap_major))
    L.check(L.lib().uvc_unfold_ln_bwd(C.byref(a), L.cur_stream()), "uvc_unfold_ln_bwd")


def fold_tokens(src, dst, B, Cc, H, W, k, s, p, dtype, lds=None, tap_major=False):
    """dst[B, H*W, C] (float32 or T) = adjoint of the soft split applied to src [B*L, lds] (columns c*k*k + tap, or tap*C + c with tap_major)."""
    _chk(src, dst)
    L.check(L.lib().uvc_fold_tokens(L.ptr(src), _is_f32(src), dtype, lds if lds is not None else src.shape[1], L.ptr(dst), _is_f32(dst), B, Cc, H, W,
                                    k, s, p, int(bool(tap_major)), L.cur_stream()), "uvc_fold_tokens")


def performer_splits(B, T) -> int:
    return int(L.lib().uvc_performer_splits(B, T))


def _perf_args(kqv, w, part, kptv, B, T, dtype):
    a = L.uvc_performer_args()
    a.kqv, a.w, a.part, a.kptv, a.B, a.T, a.dtype = L.ptr(kqv), L.ptr(w), L.ptr(part), L.ptr(kptv), B, T, dtype
    return a


def performer_fwd(kqv, w, part, kptv, att, B, T, dtype):
    _chk(kqv, w, part, kptv, att)
    a = _perf_args(kqv, w, part, kptv, B, T, dtype)
    a.att, a.att_is_f32 = L.ptr(att), _is_f32(att)
    L.check(L.lib().uvc_performer_fwd(C.byref(a), L.cur_stream()), "uvc_performer_fwd")


def performer_bwd(kqv, w, part, kptv, datt, dkqv, dkptv, B, T, dtype, dskip=None):
    _chk(kqv, w, part, kptv, datt, dkqv, dkptv, dskip)
    if dkqv.dtype != datt.dtype or (dskip is not None and dskip.dtype != datt.dtype):
        raise L.UvcHipError("performer_bwd: datt, dskip and dkqv must share one element type")
    a = _perf_args(kqv, w, part, kptv, B, T, dtype)
    a.datt, a.dskip, a.dkqv, a.dkptv, a.g_is_f32 = L.ptr(datt), L.ptr(dskip), L.ptr(dkqv), L.ptr(dkptv), _is_f32(datt)
    L.check(L.lib().uvc_performer_bwd(C.byref(a), L.cur_stream()), "uvc_performer_bwd")


class KeyedExpSource:
    """Drop-in for the ``exp_source`` hooks of the model and of UVC_CP_MiniMax: Exp(1) draws from the counter-based HIP generator
    (uvc_exp_noise), keyed by (seed, step, call number within the step).  Every rank that runs the same call sequence gets the same
    numbers; nothing is shared with torch's global generators, so an extra torch draw on one rank (the reference samples its
    FLOPs report on rank 0 only, joint_train.py:509) cannot desynchronise the replicas' s, r, y, p."""

    def __init__(self, seed, device):
        self.seed, self.device = int(seed) & 0xFFFFFFFFFFFFFFFF, device
        self.step, self.site = -1, 0

    def begin_step(self, step, resume_window=False):
        """First call of an accumulation window.  The default REPLAYS: the key restarts at (seed, step, 0) also when ``step`` repeats the
        current number (a retried step, an A/B replay, a determinism test get the same numbers again).  ``resume_window=True`` is for the
        one case that must continue instead: a window left unfinished at an epoch boundary is followed by a new window with the SAME
        optimiser step number (the reference restarts its window count per epoch, joint_train.py:423) -- the trainer knows when that is
        (the previous window ended without an optimiser step) and says so; the draws then continue the site numbering."""
        if resume_window and int(step) == self.step:
            return
        self.step, self.site = int(step), 0

    def __call__(self, shape):
        import torch
        out = torch.empty(shape, device=self.device, dtype=torch.float32)
        L.check(L.lib().uvc_exp_noise(L.ptr(out), out.numel(), self.seed, self.step, self.site, L.cur_stream()), "uvc_exp_noise")
        self.site += 1
        return out


# ---- image input step (include/uvc_data.h)

def image_desc_dtype():
    """numpy dtype with the layout of uvc_image_desc (a batch of descriptors is one structured array)."""
    import numpy as np
    return np.dtype(L.uvc_image_desc)


IMAGE_FILTERS = {"bilinear": L.UVC_IMAGE_FILTER_BILINEAR, "bicubic": L.UVC_IMAGE_FILTER_BICUBIC}


def image_filter(interpolation) -> int:
    """UVC_IMAGE_FILTER_* of an interpolation name ("bilinear" | "bicubic")."""
    if interpolation not in IMAGE_FILTERS:
        raise ValueError(f"interpolation must be one of {sorted(IMAGE_FILTERS)}, not {interpolation!r}")
    return IMAGE_FILTERS[interpolation]


def image_prep_workspace(desc, S: int, src_bytes: int, filter=None) -> int:
    """Completes the host descriptors ``desc`` (numpy array of image_desc_dtype(), C-contiguous) in place and returns the workspace
    bytes the batch needs (host only, no device access).  ``filter`` None: uvc_image_prep_workspace (bilinear); a UVC_IMAGE_FILTER_*
    value: uvc_image_prep_workspace_filter, for a launch with that filter."""
    if desc.dtype != image_desc_dtype() or not desc.flags.c_contiguous:
        raise L.UvcHipError("image_prep_workspace: desc must be a C-contiguous array of image_desc_dtype()")
    out = C.c_int64(0)
    if filter is None:
        L.check(L.lib().uvc_image_prep_workspace(desc.ctypes.data, len(desc), int(S), int(src_bytes), C.byref(out)), "uvc_image_prep_workspace")
    else:
        L.check(L.lib().uvc_image_prep_workspace_filter(desc.ctypes.data, len(desc), int(S), int(src_bytes), int(filter), C.byref(out)),
                "uvc_image_prep_workspace_filter")
    return int(out.value)


def _image_prep_args(name, args_type, desc_type, src, desc_dev, workspace, out, mean, std, filter):
    _chk(src, desc_dev, workspace, out)
    if src.dtype != torch.uint8 or desc_dev.dtype != torch.uint8 or workspace.dtype != torch.uint8:
        raise L.UvcHipError(f"{name}: src, desc and workspace are byte tensors")
    if out.dim() != 4 or out.shape[1] != 3 or out.shape[2] != out.shape[3] or out.dtype not in (torch.float32, torch.uint8):
        raise L.UvcHipError(f"{name}: out must be [B, 3, S, S] float32 or uint8")
    B, S = out.shape[0], out.shape[2]
    if desc_dev.numel() != B * C.sizeof(desc_type):
        raise L.UvcHipError(f"{name}: desc holds a different number of images than out")
    a = args_type()
    a.src, a.src_bytes, a.desc = L.ptr(src), src.numel(), L.ptr(desc_dev)
    a.workspace, a.workspace_bytes, a.out = L.ptr(workspace), workspace.numel(), L.ptr(out)
    a.mean[:], a.std[:] = [float(v) for v in mean], [float(v) for v in std]
    a.B, a.S = B, S
    a.out_dtype = L.UVC_IMAGE_OUT_U8 if out.dtype == torch.uint8 else L.UVC_IMAGE_OUT_F32
    a.filter = int(filter)
    return a


def image_prep(src, desc_dev, workspace, out, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), filter=0):
    """out[B, 3, S, S] (float32: (u8 / 255 - mean) / std, or uint8) = PIL resample (``filter``: UVC_IMAGE_FILTER_*, 0 = bilinear) of the B
    packed uint8 HWC images in ``src`` described by ``desc_dev`` (uint8 device tensor holding the descriptors image_prep_workspace
    completed for the same filter; an image completed for another one is left untouched) -- three launches."""
    a = _image_prep_args("image_prep", L.uvc_image_prep_args, L.uvc_image_desc, src, desc_dev, workspace, out, mean, std, filter)
    L.check(L.lib().uvc_image_prep(C.byref(a), L.cur_stream()), "uvc_image_prep")
    return out


def image_prep_patches(src, desc_dev, workspace, out, P, S, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), filter=0):
    """out[B * (S/P)^2, 3 * P * P] (float32 or bfloat16) = the patch rows ``patchify`` makes of ``image_prep``'s float32 batch, bit for
    bit, written by the resampler's last pass without the batch in between (uvc_image_prep_patches) -- three launches.  ``desc_dev`` and
    ``workspace`` are image_prep's (the descriptors completed by image_prep_workspace for the same filter)."""
    _chk(src, desc_dev, workspace, out)
    if src.dtype != torch.uint8 or desc_dev.dtype != torch.uint8 or workspace.dtype != torch.uint8:
        raise L.UvcHipError("image_prep_patches: src, desc and workspace are byte tensors")
    P, S = int(P), int(S)
    if out.dtype not in (torch.float32, torch.bfloat16):
        raise L.UvcHipError("image_prep_patches: out must be float32 or bfloat16")
    B = desc_dev.numel() // C.sizeof(L.uvc_image_desc)
    if desc_dev.numel() != B * C.sizeof(L.uvc_image_desc) or out.numel() != B * 3 * S * S:
        raise L.UvcHipError("image_prep_patches: out must hold [B * (S/P)^2, 3 * P * P] elements for the B descriptors")
    if P > 0 and S % P == 0 and tuple(out.shape) != (B * (S // P) ** 2, 3 * P * P):     # (a P that does not divide S is the library's refusal)
        raise L.UvcHipError("image_prep_patches: out must be [B * (S/P)^2, 3 * P * P]")
    a = L.uvc_image_prep_args()
    a.src, a.src_bytes, a.desc = L.ptr(src), src.numel(), L.ptr(desc_dev)
    a.workspace, a.workspace_bytes, a.out = L.ptr(workspace), workspace.numel(), L.ptr(out)
    a.mean[:], a.std[:] = [float(v) for v in mean], [float(v) for v in std]
    a.B, a.S, a.filter = B, S, int(filter)
    L.check(L.lib().uvc_image_prep_patches(C.byref(a), P, UVC_F32 if out.dtype == torch.float32 else UVC_BF16, L.cur_stream()),
            "uvc_image_prep_patches")
    return out


def image_prep_patches_workspace(desc, S: int, src_bytes: int, filter=None) -> int:
    """The workspace query of image_prep_patches: image_prep_workspace's (the patch-row store needs nothing more)."""
    return image_prep_workspace(desc, S, src_bytes, filter)


def logits_topk(logits, k, n_valid=None):
    """(probs float32 [B, k], index int32 [B, k]) of float32 ``logits`` [B, ld]: softmax over columns [0, n_valid) (default: all), the k
    largest in descending order, equal values by ascending index (uvc_logits_topk)."""
    _chk(logits)
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise L.UvcHipError("logits_topk: logits must be float32 [B, ld]")
    B, ld = logits.shape
    n_valid = ld if n_valid is None else int(n_valid)
    k = int(k)
    probs = torch.empty(B, max(k, 0), dtype=torch.float32, device=logits.device)
    index = torch.empty(B, max(k, 0), dtype=torch.int32, device=logits.device)
    L.check(L.lib().uvc_logits_topk(L.ptr(logits), B, ld, n_valid, k, L.ptr(probs), L.ptr(index), L.cur_stream()), "uvc_logits_topk")
    return probs, index


def _knn_dtype(t, what):
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise L.UvcHipError(f"knn_topk: {what} must be float32 or bfloat16, not {t.dtype}")
    return UVC_F32 if t.dtype == torch.float32 else UVC_BF16


def knn_splits(nq, n, k, splits=0):
    """(workspace bytes, split count used) of ``knn_topk`` for these shapes (uvc_knn_workspace_bytes; ``splits=0``: the host's choice)."""
    nbytes, used = C.c_int64(0), C.c_int32(0)
    L.check(L.lib().uvc_knn_workspace_bytes(int(nq), int(n), int(k), int(splits), C.byref(nbytes), C.byref(used)), "uvc_knn_workspace_bytes")
    return nbytes.value, used.value


def knn_topk(queries, bank, k, splits=0, sims=None, idx=None):
    """(sims float32 [nq, k], idx int32 [nq, k]): the k bank rows most similar to every query by the float32 dot product, descending, equal
    values by ascending bank row; (-inf, -1) in the slots a bank of fewer than k rows leaves (uvc_knn_topk).  ``queries`` [nq, D] and
    ``bank`` [n, D]: both bfloat16 or both float32, rows with unit element stride (a row stride above D is taken as the leading dimension).
    ``splits``: ranges the bank is divided into (0: chosen from the shapes); every value gives the same bits.  ``sims`` / ``idx``:
    contiguous outputs to write into."""
    L.require_cuda(queries, bank, sims, idx)
    if queries.dim() != 2 or bank.dim() != 2 or queries.shape[1] != bank.shape[1]:
        raise L.UvcHipError("knn_topk: queries [nq, D] and bank [n, D] must share D")
    for t in (queries, bank):
        if t.shape[1] > 1 and t.stride(1) != 1:
            raise L.UvcHipError("knn_topk: rows must have unit element stride")
    nq, D = queries.shape
    n, k = bank.shape[0], int(k)
    dev = queries.device
    sims = torch.empty(nq, max(k, 0), dtype=torch.float32, device=dev) if sims is None else sims
    idx = torch.empty(nq, max(k, 0), dtype=torch.int32, device=dev) if idx is None else idx
    _chk(sims, idx)
    if sims.dtype != torch.float32 or idx.dtype != torch.int32 or sims.numel() < nq * k or idx.numel() < nq * k:
        raise L.UvcHipError("knn_topk: sims float32 and idx int32 of at least nq * k elements")
    a = L.uvc_knn_args()
    a.queries, a.bank, a.sims, a.idx = L.ptr(queries), L.ptr(bank), L.ptr(sims), L.ptr(idx)
    a.ldq, a.ldb = (queries.stride(0) if nq > 1 else D), (bank.stride(0) if n > 1 else D)
    a.nq, a.n, a.D, a.k, a.splits = nq, n, D, k, int(splits)
    a.q_dtype, a.bank_dtype = _knn_dtype(queries, "queries"), _knn_dtype(bank, "bank")
    ws = None
    if 1 <= k <= 64 and nq >= 1 and n >= 1:            # (the call itself refuses the rest, by name)
        nbytes, _ = knn_splits(nq, n, k, splits)
        if nbytes:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            a.workspace, a.workspace_bytes = L.ptr(ws), nbytes
    L.check(L.lib().uvc_knn_topk(C.byref(a), L.cur_stream()), "uvc_knn_topk")
    return sims, idx


def knn_vote(sims, idx, labels, num_classes, temperature=0.07, scores=True):
    """(scores float32 [nq, num_classes] or None, pred int32 [nq]): the weighted k-NN vote over ``knn_topk``'s lists -- weights
    exp((s_j - s_0) / temperature), 1 with ``temperature <= 0``; ``labels`` int32 or int64 [n]; the first maximum wins, -1 for a row
    without a valid neighbour (uvc_knn_vote)."""
    _chk(sims, idx, labels)
    if sims.dim() != 2 or sims.shape != idx.shape or sims.dtype != torch.float32 or idx.dtype != torch.int32:
        raise L.UvcHipError("knn_vote: sims float32 [nq, k] and idx int32 [nq, k]")
    if labels.dim() != 1 or labels.dtype not in (torch.int32, torch.int64):
        raise L.UvcHipError("knn_vote: labels must be int32 or int64 [n]")
    nq, k = sims.shape
    C_ = int(num_classes)
    out = torch.empty(nq, max(C_, 0), dtype=torch.float32, device=sims.device) if scores else None
    pred = torch.empty(nq, dtype=torch.int32, device=sims.device)
    L.check(L.lib().uvc_knn_vote(L.ptr(sims), L.ptr(idx), L.ptr(labels), int(labels.dtype == torch.int64), nq, labels.shape[0], k, C_,
                                 float(temperature), L.ptr(out), L.ptr(pred), L.cur_stream()), "uvc_knn_vote")
    return out, pred


def softmax_xent_grad_blocks(rows, ld) -> int:
    """The workgroups (loss / hit partials) ``softmax_xent_grad`` uses for ``rows`` rows of ``ld`` columns."""
    nb = C.c_int64(0)
    L.check(L.lib().uvc_softmax_xent_grad_blocks(int(rows), int(ld), C.byref(nb)), "uvc_softmax_xent_grad_blocks")
    return int(nb.value)


def softmax_xent_grad(logits, labels, num_classes, G=None, g_dtype=torch.float32, rows=None):
    """(G [rows, ld] of ``g_dtype``, loss_part float32 [blocks], hit_part int32 [blocks]) of float32 ``logits`` [rows, ld] whose columns
    [0, num_classes) are valid and int32 / int64 ``labels``: G = softmax - onehot, +0 on the padding columns and on rows whose label lies
    outside [0, num_classes); the row losses and first-maximum hits summed per workgroup in a fixed order (uvc_softmax_xent_grad).
    ``G``: an output to write into, rows with unit element stride (its row stride is the leading dimension)."""
    L.require_cuda(logits, labels, G)
    if logits.dim() != 2 or logits.dtype != torch.float32 or (logits.shape[1] > 1 and logits.stride(1) != 1):
        raise L.UvcHipError("softmax_xent_grad: logits must be float32 [rows, ld] with unit element stride")
    if labels.dim() != 1 or labels.dtype not in (torch.int32, torch.int64) or not labels.is_contiguous():
        raise L.UvcHipError("softmax_xent_grad: labels must be contiguous int32 or int64 [rows]")
    rows = logits.shape[0] if rows is None else int(rows)
    ld = logits.stride(0) if logits.shape[0] > 1 else logits.shape[1]
    if labels.shape[0] < rows or logits.shape[0] < rows:
        raise L.UvcHipError("softmax_xent_grad: fewer labels or logit rows than rows")
    if G is None:
        G = torch.empty(max(rows, 0), ld, dtype=g_dtype, device=logits.device)
    if G.dim() != 2 or G.dtype not in (torch.float32, torch.bfloat16) or G.shape[0] < rows or G.shape[1] < ld or (G.shape[1] > 1 and G.stride(1) != 1):
        raise L.UvcHipError("softmax_xent_grad: G must be float32 or bfloat16 [rows, >= ld] with unit element stride")
    ldg = G.stride(0) if G.shape[0] > 1 else G.shape[1]
    nb = softmax_xent_grad_blocks(rows, ld) if rows >= 1 and ld >= 1 else 1
    loss_part = torch.empty(nb, dtype=torch.float32, device=logits.device)
    hit_part = torch.empty(nb, dtype=torch.int32, device=logits.device)
    L.check(L.lib().uvc_softmax_xent_grad(L.ptr(logits), L.ptr(labels), int(labels.dtype == torch.int64), rows, int(num_classes), ld, L.ptr(G), ldg,
                                          UVC_F32 if G.dtype == torch.float32 else UVC_BF16, L.ptr(loss_part), L.ptr(hit_part), L.cur_stream()),
            "uvc_softmax_xent_grad")
    return G, loss_part, hit_part


PROBE_CHUNK_ROWS = 262144                           # tools/probe_time.py: the fastest of 16 384 / 65 536 / 262 144 / n at both ImageNet shapes
PROBE_CHUNK_BYTES = 2 << 30                         # and, for wide heads, at most 2 GiB of float32 logits plus G


def probe_chunk_rows(n, num_classes, dtype) -> int:
    """The default ``chunk_rows`` of ``probe_eval``: 262 144 rows, fewer where the chunk's float32 logits plus G would pass 2 GiB (a multiple
    of 64, at least 64), or n when that is smaller.  Measured, not derived: a chunk sized for the 256 MiB Infinity Cache (11 136 rows at
    1000 classes) ran 2.0 x slower than this one, its 115 chunks bound by their launches (README "Linear probe")."""
    Cp = -(-int(num_classes) // 8) * 8
    rows = min(PROBE_CHUNK_ROWS, PROBE_CHUNK_BYTES // (Cp * (4 + (4 if dtype == UVC_F32 else 2))) // 64 * 64)
    return max(1, min(int(n), max(rows, 64)))


def probe_workspace_bytes(n, D, num_classes, dtype, chunk_rows) -> int:
    nb = C.c_int64(0)
    L.check(L.lib().uvc_probe_workspace_bytes(int(n), int(D), int(num_classes), int(dtype), int(chunk_rows), C.byref(nb)), "uvc_probe_workspace_bytes")
    return int(nb.value)


def probe_eval(X, labels, W, b, num_classes, l2, *, chunk_rows=None, dW=None, db=None, F=None, counts=None, workspace=None):
    """(dW float32 [Cp, D], db float32 [Cp] or None, F float64 [1], counts int64 [2] = (hits, m)), all on the device: the L2-regularised
    multinomial logistic objective of the head (W, b) on the features ``X`` [n, D] (bfloat16 or float32, unit element stride) and its
    gradient (uvc_probe_eval).  W float32 [Cp, D] and b float32 [Cp] or None, Cp = num_classes rounded up to 8.  Nothing is synchronised."""
    L.require_cuda(X, labels, W, b, dW, db, F, counts, workspace)
    if X.dim() != 2 or X.dtype not in (torch.float32, torch.bfloat16) or (X.shape[1] > 1 and X.stride(1) != 1):
        raise L.UvcHipError("probe_eval: X must be float32 or bfloat16 [n, D] with unit element stride")
    if labels.dim() != 1 or labels.dtype not in (torch.int32, torch.int64) or labels.shape[0] != X.shape[0] or not labels.is_contiguous():
        raise L.UvcHipError("probe_eval: labels must be contiguous int32 or int64 [n]")
    n, D = X.shape
    Cc = int(num_classes)
    Cp = -(-Cc // 8) * 8
    dtype = UVC_F32 if X.dtype == torch.float32 else UVC_BF16
    if W.dtype != torch.float32 or tuple(W.shape) != (Cp, D) or not W.is_contiguous():
        raise L.UvcHipError(f"probe_eval: W must be contiguous float32 [{Cp}, {D}]")
    if b is not None and (b.dtype != torch.float32 or tuple(b.shape) != (Cp,) or not b.is_contiguous()):
        raise L.UvcHipError(f"probe_eval: b must be contiguous float32 [{Cp}]")
    dev = X.device
    dW = torch.empty(Cp, D, dtype=torch.float32, device=dev) if dW is None else dW
    db = (torch.empty(Cp, dtype=torch.float32, device=dev) if db is None else db) if b is not None else None
    F = torch.empty(1, dtype=torch.float64, device=dev) if F is None else F
    counts = torch.empty(2, dtype=torch.int64, device=dev) if counts is None else counts
    _chk(dW, db, F, counts)
    if dW.dtype != torch.float32 or dW.numel() != Cp * D or (db is not None and (db.dtype != torch.float32 or db.numel() != Cp)) or \
            F.dtype != torch.float64 or F.numel() < 1 or counts.dtype != torch.int64 or counts.numel() < 2:
        raise L.UvcHipError("probe_eval: dW float32 [Cp, D], db float32 [Cp], F float64 [1], counts int64 [2]")
    chunk_rows = probe_chunk_rows(n, max(Cc, 1), dtype) if chunk_rows is None else int(chunk_rows)
    a = L.uvc_probe_args()
    a.X, a.labels, a.W, a.b, a.dW, a.db, a.F, a.counts = L.ptr(X), L.ptr(labels), L.ptr(W), L.ptr(b), L.ptr(dW), L.ptr(db), L.ptr(F), L.ptr(counts)
    a.n, a.ldx, a.l2 = n, (X.stride(0) if n > 1 else D), float(l2)
    a.D, a.C, a.dtype, a.labels_i64, a.chunk_rows = D, Cc, dtype, int(labels.dtype == torch.int64), chunk_rows
    if workspace is None and n >= 1 and 1 <= Cc <= 65536 and 8 <= D <= 1024 and D % 8 == 0 and chunk_rows >= 1:      # (the call itself refuses the rest, by name)
        workspace = torch.empty(probe_workspace_bytes(n, D, Cc, dtype, chunk_rows), dtype=torch.uint8, device=dev)
    if workspace is not None:
        a.workspace, a.workspace_bytes = L.ptr(workspace), workspace.numel() * workspace.element_size()
    L.check(L.lib().uvc_probe_eval(C.byref(a), L.cur_stream()), "uvc_probe_eval")
    return dW, db, F, counts


def calib_blocks(n, ld) -> int:
    """The workgroups (partials) ``calib_eval`` and ``calib_stats`` use for ``n`` rows of stride ``ld``: a function of the two alone."""
    nb = C.c_int64(0)
    L.check(L.lib().uvc_calib_blocks(int(n), int(ld), C.byref(nb)), "uvc_calib_blocks")
    return int(nb.value)


def calib_workspace_bytes(n, ld, num_classes, bins=0) -> int:
    """The workspace of ``calib_eval`` (``bins`` = 0) or ``calib_stats``."""
    nb = C.c_int64(0)
    L.check(L.lib().uvc_calib_workspace_bytes(int(n), int(ld), int(num_classes), int(bins), C.byref(nb)), "uvc_calib_workspace_bytes")
    return int(nb.value)


def _calib_args(what, logits, labels, scale, shift, num_classes, bins, workspace):
    L.require_cuda(logits, labels, scale, shift, workspace)
    if logits.dim() != 2 or logits.dtype != torch.float32 or (logits.shape[1] > 1 and logits.stride(1) != 1):
        raise L.UvcHipError(f"{what}: logits must be float32 [n, ld] with unit element stride")
    if labels.dim() != 1 or labels.dtype not in (torch.int32, torch.int64) or labels.shape[0] != logits.shape[0] or not labels.is_contiguous():
        raise L.UvcHipError(f"{what}: labels must be contiguous int32 or int64 [n]")
    n = logits.shape[0]
    ld = logits.stride(0) if n > 1 else logits.shape[1]
    Cc = logits.shape[1] if num_classes is None else int(num_classes)
    if Cc > logits.shape[1]:
        raise L.UvcHipError(f"{what}: num_classes {Cc} is more than the logits' {logits.shape[1]} columns")
    if scale.dtype != torch.float32 or scale.dim() != 1 or not scale.is_contiguous() or \
            (shift is not None and (shift.dtype != torch.float32 or tuple(shift.shape) != (Cc,) or not shift.is_contiguous())):
        raise L.UvcHipError(f"{what}: scale must be contiguous float32 [1] or [{Cc}] and shift float32 [{Cc}] or None")
    a = L.uvc_calib_args()
    a.logits, a.labels, a.scale, a.shift = L.ptr(logits), L.ptr(labels), L.ptr(scale), L.ptr(shift)
    a.n, a.ld, a.C, a.scale_len, a.labels_i64, a.bins = n, ld, Cc, scale.numel(), int(labels.dtype == torch.int64), int(bins)
    if workspace is None and n >= 1 and 1 <= Cc <= 65536 and (what == "calib_eval" or 1 <= bins <= 64):      # (the call itself refuses the rest, by name)
        workspace = torch.empty(calib_workspace_bytes(n, ld, Cc, bins), dtype=torch.uint8, device=logits.device)
    if workspace is not None:
        a.workspace, a.workspace_bytes = L.ptr(workspace), workspace.numel() * workspace.element_size()
    return a, Cc, workspace


def calib_eval(logits, labels, scale, shift=None, num_classes=None, *, F=None, dscale=None, dshift=None, counts=None, workspace=None):
    """(F float64 [1], dscale float32 like ``scale``, dshift float32 [C] or None, counts int64 [2] = (hits, m)), all on the device: the mean
    negative log-likelihood of ``z' = scale * z + shift`` over the rows whose label lies in [0, C), and its gradient in ``scale`` (float32 [1]:
    temperature scaling, s = 1/T; [C]: vector scaling) and ``shift`` (float32 [C] or None) -- one pass over the float32 ``logits`` [n, ld] whose
    columns [0, num_classes) are valid (default: all), nothing of their size is written (uvc_calib_eval).  Nothing is synchronised."""
    a, Cc, workspace = _calib_args("calib_eval", logits, labels, scale, shift, num_classes, 0, workspace)
    dev = logits.device
    F = torch.empty(1, dtype=torch.float64, device=dev) if F is None else F
    dscale = torch.empty_like(scale) if dscale is None else dscale
    if dshift is None and shift is not None:                         # (a dshift handed in without a shift is left untouched)
        dshift = torch.empty(Cc, dtype=torch.float32, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev) if counts is None else counts
    _chk(F, dscale, dshift, counts)
    if F.dtype != torch.float64 or F.numel() < 1 or dscale.dtype != torch.float32 or dscale.numel() != scale.numel() or counts.dtype != torch.int64 or \
            counts.numel() < 2 or (dshift is not None and (dshift.dtype != torch.float32 or dshift.numel() != Cc)):
        raise L.UvcHipError("calib_eval: F float64 [1], dscale float32 like scale, dshift float32 [C], counts int64 [2]")
    a.F, a.dscale, a.dshift, a.counts = L.ptr(F), L.ptr(dscale), L.ptr(dshift), L.ptr(counts)
    L.check(L.lib().uvc_calib_eval(C.byref(a), L.cur_stream()), "uvc_calib_eval")
    return F, dscale, dshift, counts


def calib_stats(logits, labels, scale, shift=None, num_classes=None, bins=15, *, workspace=None):
    """(bin_count int64 [bins], bin_conf float64 [bins], bin_hit int64 [bins], sums float64 [2] = (nll, Brier) sums, counts int64 [2] =
    (hits, m)), all on the device: the reliability histogram of ``softmax(scale * z + shift)`` over the rows whose label lies in [0, C) --
    confidence = the largest probability, bins ((j - 1) / bins, j / bins] (uvc_calib_stats).  Operands as ``calib_eval`` takes them."""
    a, Cc, workspace = _calib_args("calib_stats", logits, labels, scale, shift, num_classes, bins, workspace)
    dev = logits.device
    nb = max(int(bins), 1)
    bin_count, bin_hit = torch.empty(nb, dtype=torch.int64, device=dev), torch.empty(nb, dtype=torch.int64, device=dev)
    bin_conf, sums = torch.empty(nb, dtype=torch.float64, device=dev), torch.empty(2, dtype=torch.float64, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    a.bin_count, a.bin_conf, a.bin_hit, a.sums, a.counts = L.ptr(bin_count), L.ptr(bin_conf), L.ptr(bin_hit), L.ptr(sums), L.ptr(counts)
    L.check(L.lib().uvc_calib_stats(C.byref(a), L.cur_stream()), "uvc_calib_stats")
    return bin_count, bin_conf, bin_hit, sums, counts


CONFORMAL_METHODS = ("lac", "aps", "raps")          # UVC_CONFORMAL_*
CONFORMAL_SETS_MAX_C = 2048                         # uvc_conformal_sets keeps a row's pairs in LDS


def _conformal_args(what, logits, labels, u, num_classes, method, temperature, lam, k_reg):
    L.require_cuda(logits, labels, u)
    if logits.dim() != 2 or logits.dtype != torch.float32 or (logits.shape[1] > 1 and logits.stride(1) != 1):
        raise L.UvcHipError(f"{what}: logits must be float32 [n, ld] with unit element stride")
    n = logits.shape[0]
    if labels is not None and (labels.dim() != 1 or labels.dtype not in (torch.int32, torch.int64) or labels.shape[0] != n or not labels.is_contiguous()):
        raise L.UvcHipError(f"{what}: labels must be contiguous int32 or int64 [n]")
    if u is not None and (u.dtype != torch.float32 or tuple(u.shape) != (n,) or not u.is_contiguous()):
        raise L.UvcHipError(f"{what}: u must be contiguous float32 [n] or None")
    Cc = logits.shape[1] if num_classes is None else int(num_classes)
    if Cc > logits.shape[1]:
        raise L.UvcHipError(f"{what}: num_classes {Cc} is more than the logits' {logits.shape[1]} columns")
    a = L.uvc_conformal_args()
    a.logits, a.labels, a.u = L.ptr(logits), L.ptr(labels), L.ptr(u)
    a.n, a.ld, a.C, a.labels_i64 = n, (logits.stride(0) if n > 1 else logits.shape[1]), Cc, int(labels is not None and labels.dtype == torch.int64)
    a.method = CONFORMAL_METHODS.index(method) if method in CONFORMAL_METHODS else -1      # (the call itself refuses the rest, by name)
    t = float(temperature)
    a.inv_temperature, a.lam, a.k_reg = (1.0 / t if t > 0 else -1.0), float(lam), int(k_reg)
    return a, n, Cc


def conformal_scores(logits, labels, num_classes=None, method="aps", u=None, *, temperature=1.0, lam=0.0, k_reg=0, scores=None, counts=None):
    """(scores float32 [n], counts int64 [1] = m), on the device: the conformal score of every row's label under ``softmax(z / temperature)``
    -- ``"lac"``: 1 - p_y; ``"aps"``: the mass ranked ahead of the label + u p_y; ``"raps"``: that + lam max(0, rank - k_reg) --, NaN for a row
    whose label lies outside [0, num_classes); ``u`` float32 [n] or None (= 1).  One pass over the float32 ``logits`` [n, ld] whose columns
    [0, num_classes) are valid (default: all); nothing of their size is written (uvc_conformal_scores).  Nothing is synchronised."""
    a, n, Cc = _conformal_args("conformal_scores", logits, labels, u, num_classes, method, temperature, lam, k_reg)
    if labels is None:
        raise L.UvcHipError("conformal_scores: labels must be contiguous int32 or int64 [n]")
    dev = logits.device
    scores = torch.empty(n, dtype=torch.float32, device=dev) if scores is None else scores
    counts = torch.empty(1, dtype=torch.int64, device=dev) if counts is None else counts
    _chk(scores, counts)
    if scores.dtype != torch.float32 or scores.numel() != n or counts.dtype != torch.int64 or counts.numel() < 1:
        raise L.UvcHipError("conformal_scores: scores float32 [n], counts int64 [1]")
    a.scores, a.counts = L.ptr(scores), L.ptr(counts)
    L.check(L.lib().uvc_conformal_scores(C.byref(a), L.cur_stream()), "uvc_conformal_scores")
    return scores, counts


def conformal_sets(logits, qhat, labels=None, num_classes=None, method="aps", u=None, *, temperature=1.0, lam=0.0, k_reg=0, members=False,
                   size=None, covered=None):
    """(size int32 [n], covered uint8 [n] or None without ``labels``, members uint32 [n, ceil(C / 32)] or None), on the device: the prediction
    sets ``{c : s(c) <= qhat}`` of ``conformal_scores``' score; ``covered``: the label is in the set; ``members`` (True, or a tensor to
    fill): bit c % 32 of word c / 32 (uvc_conformal_sets).  At most 2048 classes.  Operands as ``conformal_scores`` takes them."""
    a, n, Cc = _conformal_args("conformal_sets", logits, labels, u, num_classes, method, temperature, lam, k_reg)
    dev = logits.device
    W = (max(Cc, 1) + 31) // 32
    size = torch.empty(n, dtype=torch.int32, device=dev) if size is None else size
    if covered is None and labels is not None:
        covered = torch.empty(n, dtype=torch.uint8, device=dev)
    if members is True:
        members = torch.empty(n, W, dtype=torch.int32, device=dev)      # (torch has no arithmetic on uint32: the words' bits, as int32)
    elif members is False:
        members = None
    _chk(size, covered, members)
    if size.dtype != torch.int32 or size.numel() != n or (covered is not None and (covered.dtype != torch.uint8 or covered.numel() != n)) or \
            (members is not None and (members.dtype not in (torch.int32, torch.uint32) or tuple(members.shape) != (n, W))):
        raise L.UvcHipError("conformal_sets: size int32 [n], covered uint8 [n], members int32 or uint32 [n, ceil(C / 32)]")
    a.size, a.covered, a.members, a.qhat = L.ptr(size), L.ptr(covered), L.ptr(members), float(qhat)
    L.check(L.lib().uvc_conformal_sets(C.byref(a), L.cur_stream()), "uvc_conformal_sets")
    return size, covered, members


CORRUPT_KINDS = ("gaussian_noise", "speckle_noise", "impulse_noise", "brightness", "contrast")      # UVC_CORRUPT_*
BLUR_MAX_R, STENCIL_MAX_K = 32, 25


def _image_batch(what, x, out):
    _chk(x, out)
    if x.dim() != 4 or x.dtype != torch.float32 or x.numel() == 0 or x.shape[1] > 4:
        raise L.UvcHipError(f"{what}: x must be a non-empty float32 [B, C, H, W] with at most 4 channels")
    if out is None:
        out = torch.empty_like(x)
    if out.dtype != torch.float32 or out.shape != x.shape or out.device != x.device:
        raise L.UvcHipError(f"{what}: out must be float32 of x's shape on x's device")
    return out


def _floats(what, v, n, name):
    v = [float(u) for u in (v.tolist() if hasattr(v, "tolist") else v)]
    if len(v) != n:
        raise L.UvcHipError(f"{what}: {name} must hold {n} values")
    return v


def _clamp_pair(what, lo, hi, Cc):
    if (lo is None) != (hi is None):
        raise L.UvcHipError(f"{what}: lo and hi go together")
    if lo is None:
        return None, None
    lo, hi = _floats(what, lo, Cc, "lo"), _floats(what, hi, Cc, "hi")
    if not all(a <= b for a, b in zip(lo, hi)):
        raise L.UvcHipError(f"{what}: lo <= hi in every channel")
    return (C.c_float * Cc)(*lo), (C.c_float * Cc)(*hi)


def _corrupt_args(what, x, out, kind, kinds, level, mean, std, lo, hi):
    import math
    out = _image_batch(what, x, out)
    if kind not in kinds:
        raise L.UvcHipError(f"{what}: kind must be one of {kinds}, not {kind!r}")
    level = float(level)
    if not (level >= 0 and math.isfinite(level)):
        raise L.UvcHipError(f"{what}: the level {level} must be non-negative and finite")
    if kind == "impulse_noise" and level > 1:
        raise L.UvcHipError(f"{what}: impulse_noise's level {level} is a share, at most 1")
    B, Cc, H, W = x.shape
    if Cc * H * W >= 1 << 31:
        raise L.UvcHipError(f"{what}: an image of 2^31 elements or more")
    a = L.uvc_corrupt_args()
    a.x, a.out = L.ptr(x), L.ptr(out)
    a.level, a.kind = level, CORRUPT_KINDS.index(kind)
    a.B, a.C, a.H, a.W = B, Cc, H, W
    for name, v in (("mean", mean), ("std", std), ("lo", lo), ("hi", hi)):
        v = _floats(what, v, Cc, name)
        if not all(math.isfinite(u) for u in v):
            raise L.UvcHipError(f"{what}: {name} must be finite")
        getattr(a, name)[:Cc] = v
    if not all(C.c_float(s).value > 0 and math.isfinite(C.c_float(s).value) for s in a.std[:Cc]):
        raise L.UvcHipError(f"{what}: std must be positive and finite (in float32)")
    if not all(l <= h for l, h in zip(a.lo[:Cc], a.hi[:Cc])):
        raise L.UvcHipError(f"{what}: lo <= hi in every channel")
    return a, out


def corrupt_noise(x, kind, level, *, mean, std, lo, hi, seed=0, stream=0, index0=0, out=None):
    """``out`` float32 [B, C, H, W]: ``gaussian_noise`` ``p + a z``, ``speckle_noise`` ``p + a p z`` or ``impulse_noise`` (a share ``a / 2`` of
    the elements to 0, another to 1) on the pixels ``p = x std_c + mean_c`` of the normalised batch ``x``, clamped to ``[lo_c, hi_c]``.  z and u
    are keyed draws of (``seed``, ``stream``) at the global element index ``index0 C H W + e`` (uvc_corrupt_noise); ``out`` may be ``x``."""
    a, out = _corrupt_args("corrupt_noise", x, out, kind, CORRUPT_KINDS[:3], level, mean, std, lo, hi)
    index0 = int(index0)
    if index0 < 0 or (index0 + x.shape[0]) * (x.numel() // x.shape[0]) >= 1 << 64:
        raise L.UvcHipError("corrupt_noise: index0 must be non-negative, the last global index below 2^64")
    a.index0, a.seed, a.stream_id = index0, int(seed) & (2 ** 64 - 1), int(stream) & (2 ** 64 - 1)
    L.check(L.lib().uvc_corrupt_noise(C.byref(a), L.cur_stream()), "uvc_corrupt_noise")
    return out


def corrupt_colour(x, kind, level, *, mean, std, lo, hi, image_mean=None, out=None):
    """``out`` float32 [B, C, H, W]: ``brightness`` (the HSV value of the clipped pixel raised by ``level``, at most 1) or ``contrast``
    (``(p - m) a + m`` around the image's mean ``m``), clamped to ``[lo_c, hi_c]`` (uvc_corrupt_colour).  ``image_mean`` (contrast): float32
    [B] that receives ``m``; default a new tensor.  Returns ``out``, or ``(out, image_mean)`` for contrast."""
    a, out = _corrupt_args("corrupt_colour", x, out, kind, CORRUPT_KINDS[3:], level, mean, std, lo, hi)
    if kind == "contrast":
        if image_mean is None:
            image_mean = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        _chk(image_mean)
        if image_mean.dtype != torch.float32 or image_mean.shape != (x.shape[0],) or image_mean.device != x.device:
            raise L.UvcHipError("corrupt_colour: image_mean must be float32 [B] on x's device")
        a.image_mean = L.ptr(image_mean)
    L.check(L.lib().uvc_corrupt_colour(C.byref(a), L.cur_stream()), "uvc_corrupt_colour")
    return (out, image_mean) if kind == "contrast" else out


def _plane_args(what, x, out, lo, hi):
    out = _image_batch(what, x, out)
    if out.data_ptr() == x.data_ptr():
        raise L.UvcHipError(f"{what}: out must not be x")
    B, Cc, H, W = x.shape
    if H * W >= 1 << 31:
        raise L.UvcHipError(f"{what}: a plane of 2^31 elements or more")
    lo, hi = _clamp_pair(what, lo, hi, Cc)
    return out, (B * Cc, Cc, H, W, lo, hi, L.cur_stream())


def blur_separable(x, taps, *, lo=None, hi=None, scratch=None, out=None):
    """``out`` float32 [B, C, H, W]: every plane filtered along x and then along y by the ``2 R + 1`` ``taps`` (host floats, R <= 32), borders
    clamp the index, each output one fma chain over ascending taps; ``scratch``: the float32 plane between the passes (default: new);
    ``lo`` / ``hi``: the per-channel clamp of the result (uvc_blur_separable)."""
    import math
    taps = [float(t) for t in (taps.tolist() if hasattr(taps, "tolist") else taps)]
    if len(taps) % 2 == 0 or len(taps) > 2 * BLUR_MAX_R + 1 or not all(math.isfinite(t) for t in taps):
        raise L.UvcHipError(f"blur_separable: an odd number of finite taps, at most {2 * BLUR_MAX_R + 1}")
    out, tail = _plane_args("blur_separable", x, out, lo, hi)
    if scratch is None:
        scratch = torch.empty_like(x)
    _chk(scratch)
    if scratch.dtype != torch.float32 or scratch.shape != x.shape or scratch.device != x.device or scratch.data_ptr() in (x.data_ptr(), out.data_ptr()):
        raise L.UvcHipError("blur_separable: scratch must be a float32 tensor of x's shape of its own")
    L.check(L.lib().uvc_blur_separable(L.ptr(x), L.ptr(scratch), L.ptr(out), (C.c_float * len(taps))(*taps), len(taps) // 2, *tail), "uvc_blur_separable")
    return out


def stencil2d(x, taps, *, lo=None, hi=None, out=None):
    """``out`` float32 [B, C, H, W]: every plane under the dense ``K x K`` filter ``taps`` (float32 [K, K] on the device, K odd in 3 .. 25), borders
    clamp the index, each output one fma chain over the taps in row-major order, zero taps skipped (uvc_stencil2d)."""
    _chk(taps)
    if taps.dim() != 2 or taps.dtype != torch.float32 or taps.shape[0] != taps.shape[1] or taps.shape[0] % 2 == 0 or not 3 <= taps.shape[0] <= STENCIL_MAX_K \
            or taps.device != x.device:
        raise L.UvcHipError(f"stencil2d: taps must be float32 [K, K] on x's device, K odd in [3, {STENCIL_MAX_K}]")
    out, tail = _plane_args("stencil2d", x, out, lo, hi)
    L.check(L.lib().uvc_stencil2d(L.ptr(x), L.ptr(out), L.ptr(taps), taps.shape[0], *tail), "uvc_stencil2d")
    return out


def pixelate(x, k, *, lo=None, hi=None, out=None):
    """``out`` float32 [B, C, H, W]: every pixel becomes the mean of its ``k x k`` cell; cells start at 0 and a ragged last cell averages what
    exists; ``k = 1`` returns x's bits (uvc_pixelate)."""
    if int(k) != k or int(k) < 1 or int(k) >= 1 << 31:
        raise L.UvcHipError(f"pixelate: the cell width {k} must be an integer, at least 1")
    out, tail = _plane_args("pixelate", x, out, lo, hi)
    L.check(L.lib().uvc_pixelate(L.ptr(x), L.ptr(out), int(k), *tail), "uvc_pixelate")
    return out


def box_muller(u1, u2):
    """``(z0, z1)`` float32: ``r cos t`` and ``r sin t`` with ``r = sqrt(-2 ln u1)``, ``t = 2 pi u2`` of float32 ``u1`` in (0, 1) and ``u2`` in
    [0, 1) -- the device function of the noise corruptions on given uniforms (uvc_box_muller)."""
    _chk(u1, u2)
    if u1.dtype != torch.float32 or u2.dtype != torch.float32 or u1.dim() != 1 or u1.shape != u2.shape or u1.numel() == 0:
        raise L.UvcHipError("box_muller: u1 and u2 must be non-empty float32 [n]")
    z0, z1 = torch.empty_like(u1), torch.empty_like(u1)
    L.check(L.lib().uvc_box_muller(L.ptr(u1), L.ptr(u2), L.ptr(z0), L.ptr(z1), u1.numel(), L.cur_stream()), "uvc_box_muller")
    return z0, z1


INFLUENCE_MAX_CR = 4096                             # uvc_influence_topk's widest residual row
INFLUENCE_TARGETS = ("label", "pred")               # uvc_influence_residuals' target_mode 0 / 1


def influence_residuals(logits, labels=None, num_classes=None, target="label", *, r=None):
    """``(r float32 [n, ceil8(C)], target int32 [n], rsq float32 [n])``: ``softmax(z) - e_target`` over columns [0, num_classes) (default: all)
    of the float32 ``logits`` [n, ld], +0 on the padding columns; the target is the label (a label outside [0, C): a skipped row of zeros,
    target -1) or, with ``target="pred"``, the row's first maximum; ``rsq`` the rows' squared norms (uvc_influence_residuals).  ``r``: a
    float32 [n, ldr] tensor to fill, ldr a multiple of 8 and every column of it is written."""
    L.require_cuda(logits, labels, r)
    if target not in INFLUENCE_TARGETS:
        raise L.UvcHipError(f"influence_residuals: target must be one of {INFLUENCE_TARGETS}, not {target!r}")
    if logits.dim() != 2 or logits.dtype != torch.float32 or (logits.shape[1] > 1 and logits.stride(1) != 1):
        raise L.UvcHipError("influence_residuals: logits must be float32 [n, ld] with unit element stride")
    n, cols = logits.shape
    ld = logits.stride(0) if n > 1 else cols
    Cc = cols if num_classes is None else int(num_classes)
    if Cc > cols:
        raise L.UvcHipError(f"influence_residuals: num_classes {Cc} is more than the logits' {cols} columns")
    i64 = 0
    if labels is not None:
        if labels.dim() != 1 or labels.dtype not in (torch.int32, torch.int64) or labels.shape[0] != n or not labels.is_contiguous():
            raise L.UvcHipError("influence_residuals: labels must be contiguous int32 or int64 [n]")
        i64 = int(labels.dtype == torch.int64)
    dev = logits.device
    if r is None:
        r = torch.empty(n, (max(Cc, 1) + 7) // 8 * 8, dtype=torch.float32, device=dev)
    if r.dim() != 2 or r.dtype != torch.float32 or r.shape[0] != n or r.stride(1) != 1:
        raise L.UvcHipError("influence_residuals: r must be float32 [n, ldr] with unit element stride")
    ldr = r.shape[1]
    if n > 1 and r.stride(0) != ldr:
        raise L.UvcHipError("influence_residuals: r's rows must be dense (every column of r is written)")
    tgt = torch.empty(n, dtype=torch.int32, device=dev)
    rsq = torch.empty(n, dtype=torch.float32, device=dev)
    L.check(L.lib().uvc_influence_residuals(L.ptr(logits), n, ld, Cc, L.ptr(labels), i64, INFLUENCE_TARGETS.index(target), L.ptr(r), ldr, L.ptr(tgt),
                                            L.ptr(rsq), L.cur_stream()), "uvc_influence_residuals")
    return r, tgt, rsq


def influence_splits(nq, n, k, splits=0):
    """(workspace bytes, split count used) of ``influence_topk`` for these shapes (uvc_influence_workspace_bytes)."""
    nbytes, used = C.c_int64(0), C.c_int32(0)
    L.check(L.lib().uvc_influence_workspace_bytes(int(nq), int(n), int(k), int(splits), C.byref(nbytes), C.byref(used)), "uvc_influence_workspace_bytes")
    return nbytes.value, used.value


def influence_topk(fq, fb, rq, rb, k, *, bias=1.0, exclude=None, splits=0, proponents=True, opponents=True):
    """``((pos_vals, pos_idx), (neg_vals, neg_idx))``, float32 / int32 [nq, k] each: per query the k largest and the k smallest of
    ``(fq . fb_i + bias) * (rq . rb_i)`` over the bank's rows -- descending / ascending, equal values by ascending bank row, (-inf, -1) /
    (+inf, -1) in the slots a bank of fewer than k rows leaves; a NaN enters neither list (uvc_influence_topk).  ``fq`` [nq, D] and ``fb``
    [n, D]: both bfloat16 or both float32; ``rq`` [nq, Cr] and ``rb`` [n, Cr]: float32, Cr a multiple of 8 (``influence_residuals``' rows);
    a row stride above the width is taken as the leading dimension.  ``exclude`` int32 [nq]: one bank row per query to skip (-1: none).
    ``proponents`` / ``opponents``: True, False (that list is None and not computed) or a ``(vals, idx)`` pair of tensors to fill.
    ``splits``: ranges the bank is divided into (0: chosen from the shapes); every value gives the same bits."""
    L.require_cuda(fq, fb, rq, rb, exclude)
    if fq.dim() != 2 or fb.dim() != 2 or fq.shape[1] != fb.shape[1]:
        raise L.UvcHipError("influence_topk: fq [nq, D] and fb [n, D] must share D")
    if rq.dim() != 2 or rb.dim() != 2 or rq.shape[1] != rb.shape[1] or rq.shape[0] != fq.shape[0] or rb.shape[0] != fb.shape[0]:
        raise L.UvcHipError("influence_topk: rq [nq, Cr] and rb [n, Cr] must share Cr and have one row per feature row")
    if rq.dtype != torch.float32 or rb.dtype != torch.float32:
        raise L.UvcHipError("influence_topk: residuals must be float32")
    for t in (fq, fb, rq, rb):
        if t.shape[1] > 1 and t.stride(1) != 1:
            raise L.UvcHipError("influence_topk: rows must have unit element stride")
    nq, D = fq.shape
    n, Cr, k = fb.shape[0], rq.shape[1], int(k)
    dev = fq.device
    if exclude is not None and (exclude.dtype != torch.int32 or exclude.dim() != 1 or exclude.shape[0] != nq or not exclude.is_contiguous()):
        raise L.UvcHipError("influence_topk: exclude must be contiguous int32 [nq]")
    outs = []
    for want in (proponents, opponents):
        if want is False or want is None:
            outs.append(None)
            continue
        v, i = ((torch.empty(nq, max(k, 0), dtype=torch.float32, device=dev), torch.empty(nq, max(k, 0), dtype=torch.int32, device=dev))
                if want is True else want)
        _chk(v, i)
        if v.dtype != torch.float32 or i.dtype != torch.int32 or v.numel() < nq * k or i.numel() < nq * k:
            raise L.UvcHipError("influence_topk: a list is (float32, int32) tensors of at least nq * k elements")
        outs.append((v, i))
    a = L.uvc_influence_args()
    a.fq, a.fb, a.rq, a.rb, a.exclude = L.ptr(fq), L.ptr(fb), L.ptr(rq), L.ptr(rb), L.ptr(exclude)
    if outs[0] is not None:
        a.pos_vals, a.pos_idx = L.ptr(outs[0][0]), L.ptr(outs[0][1])
    if outs[1] is not None:
        a.neg_vals, a.neg_idx = L.ptr(outs[1][0]), L.ptr(outs[1][1])
    a.ldfq, a.ldfb = (fq.stride(0) if nq > 1 else D), (fb.stride(0) if n > 1 else D)
    a.ldrq, a.ldrb = (rq.stride(0) if nq > 1 else Cr), (rb.stride(0) if n > 1 else Cr)
    a.bias = float(bias)
    a.nq, a.n, a.D, a.Cr, a.k, a.splits = nq, n, D, Cr, k, int(splits)
    a.q_dtype, a.bank_dtype = _knn_dtype(fq, "fq"), _knn_dtype(fb, "fb")
    ws = None
    if 1 <= k <= 64 and nq >= 1 and n >= 1:            # (the call itself refuses the rest, by name)
        nbytes, _ = influence_splits(nq, n, k, splits)
        if nbytes:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            a.workspace, a.workspace_bytes = L.ptr(ws), nbytes
    L.check(L.lib().uvc_influence_topk(C.byref(a), L.cur_stream()), "uvc_influence_topk")
    return outs[0], outs[1]


def self_influence(features, rsq, *, bias=1.0, want_fsq=False):
    """``(|f_i|^2 + bias) * rsq_i`` float32 [n] of the bfloat16 or float32 ``features`` [n, D] and ``influence_residuals``' ``rsq``
    (uvc_influence_self); with ``want_fsq`` the pair ``(values, fsq)``."""
    L.require_cuda(features, rsq)
    if features.dim() != 2 or (features.shape[1] > 1 and features.stride(1) != 1):
        raise L.UvcHipError("self_influence: features [n, D] with unit element stride")
    n, D = features.shape
    if rsq.dim() != 1 or rsq.dtype != torch.float32 or rsq.shape[0] != n or not rsq.is_contiguous():
        raise L.UvcHipError("self_influence: rsq must be contiguous float32 [n]")
    out = torch.empty(n, dtype=torch.float32, device=features.device)
    fsq = torch.empty(n, dtype=torch.float32, device=features.device) if want_fsq else None
    L.check(L.lib().uvc_influence_self(L.ptr(features), features.stride(0) if n > 1 else D, _knn_dtype(features, "features"), n, D, L.ptr(rsq),
                                       float(bias), L.ptr(fsq), L.ptr(out), L.cur_stream()), "uvc_influence_self")
    return (out, fsq) if want_fsq else out


def influence_expf(d):
    """``expf(d)`` of float32 ``d`` [n] by the device function ``influence_residuals`` calls (uvc_influence_expf)."""
    _chk(d)
    if d.dtype != torch.float32 or d.dim() != 1 or d.numel() == 0 or not d.is_contiguous():
        raise L.UvcHipError("influence_expf: d must be non-empty contiguous float32 [n]")
    e = torch.empty_like(d)
    L.check(L.lib().uvc_influence_expf(L.ptr(d), L.ptr(e), d.numel(), L.cur_stream()), "uvc_influence_expf")
    return e


CASCADE_SCORES = ("msp", "margin", "entropy")       # uvc_cascade_decide's kind 0 / 1 / 2
CASCADE_MAX_C = 65536


def _i32_vec(t, n, what):
    if t.dim() != 1 or t.dtype != torch.int32 or t.shape[0] < n or not t.is_contiguous():
        raise L.UvcHipError(f"{what} must be contiguous int32 of at least {n} elements")


def cascade_decide(logits, num_classes=None, temperature=1.0, kind="msp", threshold=float("-inf"), *, score=True, top1=True, defer=True):
    """``(score float32 [n], top1 int32 [n], defer int32 [n])`` per row of the float32 ``logits`` [n, ld] over columns [0, num_classes)
    (default: all): the confidence of ``softmax(z / temperature)`` -- ``kind`` "msp", "margin" or "entropy" (``CASCADE_SCORES``) --, the
    first maximum and ``!(score >= threshold)`` in float32 (uvc_cascade_decide; a NaN row: NaN, -1, 1).  ``score`` / ``top1`` / ``defer``:
    True, False (None comes back, nothing is computed into it) or a contiguous tensor to write into."""
    L.require_cuda(logits)
    if kind not in CASCADE_SCORES:
        raise L.UvcHipError(f"cascade_decide: kind must be one of {CASCADE_SCORES}, not {kind!r}")
    n, cols, ld = _rows_f32(logits, "cascade_decide: logits")
    Cc = cols if num_classes is None else int(num_classes)
    if Cc > cols:
        raise L.UvcHipError(f"cascade_decide: num_classes {Cc} is more than the logits' {cols} columns")
    outs = []
    for want, dt, name in ((score, torch.float32, "score"), (top1, torch.int32, "top1"), (defer, torch.int32, "defer")):
        if want is False or want is None:
            outs.append(None)
            continue
        t = torch.empty(n, dtype=dt, device=logits.device) if want is True else want
        L.require_cuda(t)
        if t.dim() != 1 or t.dtype != dt or t.shape[0] != n or not t.is_contiguous():
            raise L.UvcHipError(f"cascade_decide: {name} must be contiguous {dt} [n]")
        outs.append(t)
    L.check(L.lib().uvc_cascade_decide(L.ptr(logits), n, ld, Cc, float(temperature), CASCADE_SCORES.index(kind), float(threshold), L.ptr(outs[0]),
                                       L.ptr(outs[1]), L.ptr(outs[2]), L.cur_stream()), "uvc_cascade_decide")
    return tuple(outs)


def cascade_compact_workspace_bytes(n):
    nbytes = C.c_int64(0)
    L.check(L.lib().uvc_cascade_compact_workspace_bytes(int(n), C.byref(nbytes)), "uvc_cascade_compact_workspace_bytes")
    return nbytes.value


def cascade_compact(defer, *, idx=None, pos=None, count=None, workspace=None):
    """``(idx int32 [n], pos int32 [n], count int32 [1])`` of the int32 ``defer`` [n] (non-zero: deferred): the deferred rows in ascending
    order in ``idx[:count]`` (the slots behind them are NOT written), every row's slot in ``idx`` or -1 in ``pos``, their number in
    ``count`` -- all on the device, nothing is read back (uvc_cascade_compact).  The outputs and the workspace may be handed in."""
    _chk(defer)
    if defer.dim() != 1 or defer.dtype != torch.int32 or defer.numel() == 0:
        raise L.UvcHipError("cascade_compact: defer must be non-empty contiguous int32 [n]")
    n, dev = defer.shape[0], defer.device
    idx = torch.empty(n, dtype=torch.int32, device=dev) if idx is None else idx
    pos = torch.empty(n, dtype=torch.int32, device=dev) if pos is None else pos
    count = torch.empty(1, dtype=torch.int32, device=dev) if count is None else count
    L.require_cuda(idx, pos, count, workspace)
    _i32_vec(idx, n, "cascade_compact: idx")
    _i32_vec(pos, n, "cascade_compact: pos")
    _i32_vec(count, 1, "cascade_compact: count")
    if workspace is None:
        workspace = torch.empty(cascade_compact_workspace_bytes(n), dtype=torch.uint8, device=dev)
    L.check(L.lib().uvc_cascade_compact(L.ptr(defer), n, L.ptr(idx), L.ptr(pos), L.ptr(count), L.ptr(workspace), workspace.numel(), L.cur_stream()),
            "uvc_cascade_compact")
    return idx, pos, count


def cascade_gather(src, idx, m, rows_per_item=1, *, out=None):
    """``[m * rows_per_item, width]``: the items ``idx[:m]`` (int32, on the device) of the bfloat16 or float32 ``src`` [n * rows_per_item,
    width], an item being ``rows_per_item`` consecutive rows, copied bit for bit; an index outside [0, n) gives an item of +0
    (uvc_cascade_gather).  ``m`` is a host integer; 0 gives an empty tensor and launches nothing.  A row stride above the width is taken
    as the leading dimension, of ``src`` and of ``out``."""
    L.require_cuda(src, idx, out)
    if src.dim() != 2 or (src.shape[1] > 1 and src.stride(1) != 1) or src.shape[0] == 0:
        raise L.UvcHipError("cascade_gather: src [rows, width] with unit element stride")
    rpi, m = int(rows_per_item), int(m)
    rows, width = src.shape
    if rpi < 1 or rows % rpi:
        raise L.UvcHipError(f"cascade_gather: {rows} rows are not a multiple of rows_per_item {rpi}")
    n = rows // rpi
    if not 0 <= m <= n:
        raise L.UvcHipError(f"cascade_gather: m {m} must lie in [0, {n}]")
    _i32_vec(idx, m, "cascade_gather: idx")
    if out is None:
        out = torch.empty(m * rpi, width, dtype=src.dtype, device=src.device)
    if out.dim() != 2 or out.dtype != src.dtype or tuple(out.shape) != (m * rpi, width) or (width > 1 and out.stride(1) != 1):
        raise L.UvcHipError(f"cascade_gather: out must be {src.dtype} [{m * rpi}, {width}] with unit element stride")
    lds, ldd = (src.stride(0) if rows > 1 else width), (out.stride(0) if m * rpi > 1 else width)
    L.check(L.lib().uvc_cascade_gather(L.ptr(src), lds, _knn_dtype(src, "src"), n, rpi, width, L.ptr(idx), m, L.ptr(out) if m else 0, ldd, L.cur_stream()),
            "uvc_cascade_gather")
    return out


def cascade_merge(z_small, z_large, pos, num_classes=None, *, out=None, source=True):
    """``(out float32 [n, C], source int32 [n])``: ``out[b] = z_large[pos[b]]`` where ``pos[b] >= 0`` and ``z_small[b]`` elsewhere, over the
    columns [0, C) (default: the narrower of the two) bit for bit, and 1 / 0 beside it (uvc_cascade_merge).  ``z_large``: [m, ldl] or None
    (nothing was deferred); a row stride above the width is taken as the leading dimension of either input and of ``out``."""
    L.require_cuda(z_small, z_large, pos, out)
    n, cs, lds = _rows_f32(z_small, "cascade_merge: z_small")
    m, cl, ldl = (0, cs, cs) if z_large is None or z_large.shape[0] == 0 else _rows_f32(z_large, "cascade_merge: z_large")
    Cc = min(cs, cl) if num_classes is None else int(num_classes)
    if Cc > min(cs, cl):
        raise L.UvcHipError(f"cascade_merge: num_classes {Cc} is more than the logits' {min(cs, cl)} columns")
    _i32_vec(pos, n, "cascade_merge: pos")
    if out is None:
        out = torch.empty(n, max(Cc, 0), dtype=torch.float32, device=z_small.device)
    no, co, ldo = _rows_f32(out, "cascade_merge: out")
    if no != n or co < Cc:
        raise L.UvcHipError(f"cascade_merge: out must be float32 [{n}, >= {Cc}]")
    src = None
    if source is not False and source is not None:
        src = torch.empty(n, dtype=torch.int32, device=z_small.device) if source is True else source
        L.require_cuda(src)
        _i32_vec(src, n, "cascade_merge: source")
    L.check(L.lib().uvc_cascade_merge(L.ptr(z_small), lds, L.ptr(z_large) if m else 0, ldl, m, L.ptr(pos), n, Cc, L.ptr(out), ldo, L.ptr(src),
                                      L.cur_stream()), "uvc_cascade_merge")
    return out, src


OOD_MAX_D = 1016                                 # D + 8 augmentation columns is knn_topk's widest row
OOD_CHUNK_ROWS = 65536                              # tools/ood_time.py: within 5 % of the best of 16 384 / 65 536 / 262 144 at both ImageNet shapes


def _rows_f32(t, what):
    if t.dim() != 2 or t.dtype != torch.float32 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise L.UvcHipError(f"{what} must be float32 [n, D] with unit element stride")
    return t.shape[0], t.shape[1], (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def _labels_1d(labels, n, what):
    if labels.dim() != 1 or labels.dtype not in (torch.int32, torch.int64) or labels.shape[0] != n or not labels.is_contiguous():
        raise L.UvcHipError(f"{what}: labels must be contiguous int32 or int64 [n]")
    return int(labels.dtype == torch.int64)


def ood_logit_scores(logits, n_valid=None, temperature=1.0, outs=None):
    """(msp, maxlogit, energy, entropy), float32 [n] each: the maximum softmax probability, the maximum logit, ``T log sum exp(z / T)`` and
    the NEGATIVE entropy of ``softmax(z)`` over columns [0, n_valid) (default: all) of the float32 ``logits`` [n, ld], one pass
    (uvc_ood_logit_scores).  ``outs``: four contiguous float32 tensors to write into, None for a score that is not wanted."""
    L.require_cuda(logits)
    n, cols, ld = _rows_f32(logits, "ood_logit_scores: logits")
    n_valid = cols if n_valid is None else int(n_valid)
    if n_valid > cols:
        raise L.UvcHipError(f"ood_logit_scores: n_valid {n_valid} is more than the logits' {cols} columns")
    if outs is None:
        outs = tuple(torch.empty(n, dtype=torch.float32, device=logits.device) for _ in range(4))
    outs = tuple(outs)
    _chk(*outs)
    if len(outs) != 4 or any(o is not None and (o.dtype != torch.float32 or o.numel() < n) for o in outs):
        raise L.UvcHipError("ood_logit_scores: outs must be four float32 tensors of at least n elements (or None)")
    L.check(L.lib().uvc_ood_logit_scores(L.ptr(logits), n, ld, n_valid, float(temperature), *[L.ptr(o) for o in outs], L.cur_stream()),
            "uvc_ood_logit_scores")
    return outs


def class_moments(X, labels, num_classes, *, counts=None, means=None):
    """(counts int64 [C], means float32 [C, D]) of the float32 bank ``X`` [n, D] by the int32 / int64 ``labels``: rows with a label outside
    [0, C) are skipped, every sum is float64 in a fixed order and rounded once, an empty class gives 0 and a row of +0 (uvc_class_moments).
    The rows of a class are found through the permutation of a stable device sort of the labels."""
    L.require_cuda(X, labels, counts, means)
    n, D, ldx = _rows_f32(X, "class_moments: X")
    i64 = _labels_1d(labels, n, "class_moments")
    Cc = int(num_classes)
    dev = X.device
    counts = torch.empty(max(Cc, 0), dtype=torch.int64, device=dev) if counts is None else counts
    means = torch.empty(max(Cc, 0), D, dtype=torch.float32, device=dev) if means is None else means
    _chk(counts, means)
    if counts.dtype != torch.int64 or counts.numel() < Cc or means.dtype != torch.float32 or means.numel() < Cc * D:
        raise L.UvcHipError("class_moments: counts int64 [C] and means float32 [C, D]")
    perm = torch.sort(labels, stable=True)[1]
    ws, nbytes = None, 0
    if n >= 1 and 8 <= D <= OOD_MAX_D and D % 8 == 0:                # (the call itself refuses the rest, by name)
        b = C.c_int64(0)
        L.check(L.lib().uvc_class_moments_workspace_bytes(n, D, C.byref(b)), "uvc_class_moments_workspace_bytes")
        nbytes = int(b.value)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    L.check(L.lib().uvc_class_moments(L.ptr(X), ldx, L.ptr(labels), i64, L.ptr(perm), n, D, Cc, L.ptr(counts), L.ptr(means), L.ptr(ws), nbytes,
                                      L.cur_stream()), "uvc_class_moments")
    return counts, means


def center_rows(X, labels, means, out=None):
    """``out`` float32 [n, D] = x_i - means[y_i], one rounding; a row whose label lies outside [0, C) becomes +0 (uvc_center_rows)."""
    L.require_cuda(X, labels, means, out)
    n, D, ldx = _rows_f32(X, "center_rows: X")
    i64 = _labels_1d(labels, n, "center_rows")
    if means.dim() != 2 or means.dtype != torch.float32 or means.shape[1] != D or not means.is_contiguous():
        raise L.UvcHipError("center_rows: means must be contiguous float32 [C, D]")
    out = torch.empty(n, D, dtype=torch.float32, device=X.device) if out is None else out
    if tuple(out.shape) != (n, D):
        raise L.UvcHipError("center_rows: out must be float32 [n, D]")
    _, _, ldo = _rows_f32(out, "center_rows: out")
    L.check(L.lib().uvc_center_rows(L.ptr(X), ldx, L.ptr(labels), i64, L.ptr(means), n, D, means.shape[0], L.ptr(out), ldo, L.cur_stream()),
            "uvc_center_rows")
    return out


def class_gaussian_fit(X, labels, num_classes, chunk_rows=None):
    """(counts int64 [C], means float32 [C, D], scatter float32 [D, D]): ``class_moments``, then per chunk of ``chunk_rows`` rows (default
    65 536) ``center_rows`` and ``gemm_tn`` in float32 onto ``scatter = sum_i (x_i - mean_{y_i}) (x_i - mean_{y_i})^T`` (beta = 1 after the first
    chunk).  The same ``chunk_rows`` gives the same bits; different ones differ by float32 summation order."""
    counts, means = class_moments(X, labels, num_classes)
    n, D = X.shape
    chunk = max(1, min(n, OOD_CHUNK_ROWS if chunk_rows is None else int(chunk_rows)))
    dev = X.device
    scatter = torch.empty(D, D, dtype=torch.float32, device=dev)
    buf = torch.empty(chunk, D, dtype=torch.float32, device=dev)
    ws = torch.empty(max(gemm_tn_workspace_bytes(chunk, D, D), 16), dtype=torch.uint8, device=dev)
    for r0 in range(0, n, chunk):
        rows = min(chunk, n - r0)
        center_rows(X[r0:r0 + rows], labels[r0:r0 + rows], means, out=buf[:rows])
        gemm_tn(buf, buf, scatter, ws, dtype=UVC_F32, beta=0.0 if r0 == 0 else 1.0, M=rows, N1=D, N2=D)
    return counts, means, scatter


def rows_sqnorm_aug(Z, D, sq=None):
    """``sq`` float32 [n] = the sum of squares of columns [0, D) of every row of the float32 ``Z`` [n, >= D + 8]; columns [D, D + 8) are set
    to 1, 0 .. 0 (uvc_rows_sqnorm_aug)."""
    L.require_cuda(Z, sq)
    n, _, ldz = _rows_f32(Z, "rows_sqnorm_aug: Z")
    if Z.shape[1] < int(D) + 8:
        raise L.UvcHipError("rows_sqnorm_aug: Z must have at least D + 8 columns")
    sq = torch.empty(n, dtype=torch.float32, device=Z.device) if sq is None else sq
    _chk(sq)
    if sq.dtype != torch.float32 or sq.numel() < n:
        raise L.UvcHipError("rows_sqnorm_aug: sq must be float32 [n]")
    L.check(L.lib().uvc_rows_sqnorm_aug(L.ptr(Z), ldz, n, int(D), L.ptr(sq), L.cur_stream()), "uvc_rows_sqnorm_aug")
    return sq


def gauss_scores(X, whiten, mean0, wmeans=None, counts=None):
    """``(min_d2 float32 [n], argmin int32 [n])``: the smallest squared Mahalanobis distance ``|whiten (x - mean_c)|^2`` of every row of the
    float32 ``X`` [n, D] to a class with ``counts[c] > 0``, and that class; ``wmeans`` float32 [C, D] holds ``whiten (mean_c - mean0)``.  With
    ``wmeans=None``: just ``|whiten (x - mean0)|^2``.  z = x whiten^T - whiten mean0 is ``gemm_nt`` in float32 with its bias epilogue into rows
    of stride D + 8, ``rows_sqnorm_aug`` takes |z|^2 and appends 1, 0 .. 0, and ``knn_topk`` with k = 1 against the rows
    (m_c, -|m_c|^2 / 2, 0 .. 0) finds ``max_c (z . m_c - |m_c|^2 / 2)``: min_c |z - m_c|^2 = |z|^2 - 2 max_c (..).  The class rows (C x D, once
    per call), the final ``sq - 2 s`` and the map from kept rows back to classes are plain torch statements; everything of size n x D or
    n x C is a kernel."""
    L.require_cuda(X, whiten, mean0, wmeans, counts)
    n, D, ldx = _rows_f32(X, "gauss_scores: X")
    if D % 8 or not 8 <= D <= OOD_MAX_D:
        raise L.UvcHipError(f"gauss_scores: D must be a multiple of 8 in [8, {OOD_MAX_D}], not {D}")
    if whiten.dtype != torch.float32 or tuple(whiten.shape) != (D, D) or not whiten.is_contiguous() or mean0.dtype != torch.float32 or \
            tuple(mean0.shape) != (D,) or not mean0.is_contiguous():
        raise L.UvcHipError("gauss_scores: whiten must be contiguous float32 [D, D] and mean0 float32 [D]")
    dev = X.device
    bias = torch.empty(1, D, dtype=torch.float32, device=dev)
    gemm_nt(mean0.view(1, D), whiten, bias, dtype=UVC_F32, alpha=-1.0)
    z = torch.empty(n, D + 8, dtype=torch.float32, device=dev)
    gemm_nt(X, whiten, z, dtype=UVC_F32, epilogue=EPI_BIAS, bias=bias.view(D), M=n, N=D, K=D, lda=ldx, ldc=D + 8)
    sq = rows_sqnorm_aug(z, D)
    if wmeans is None:
        return sq
    if wmeans.dtype != torch.float32 or wmeans.dim() != 2 or wmeans.shape[1] != D or counts is None or counts.shape[0] != wmeans.shape[0]:
        raise L.UvcHipError("gauss_scores: wmeans must be float32 [C, D] with counts [C]")
    kept = torch.nonzero(counts > 0)[:, 0]
    if kept.numel() == 0:
        raise L.UvcHipError("gauss_scores: every class is empty")
    m = wmeans[kept]
    aug = torch.zeros(kept.numel(), D + 8, dtype=torch.float32, device=dev)
    aug[:, :D] = m
    aug[:, D] = (-0.5 * m.double().square().sum(dim=1)).float()      # rounded once
    sims, idx = knn_topk(z, aug, 1)
    return sq - 2.0 * sims[:, 0], kept[idx[:, 0].long()].to(torch.int32)


PAIR_STATS = ("top1_a", "top1_b", "conf_a", "conf_b", "kl_ab", "kl_ba", "js", "tv", "nll_a", "nll_b", "rank_a", "rank_b", "rank_b_top1a",
              "rank_a_top1b")
PAIR_STATS_INT = ("top1_a", "top1_b", "rank_a", "rank_b", "rank_b_top1a", "rank_a_top1b")


def logits_pair_stats_reg_max() -> int:
    """The widest row pair ``logits_pair_stats`` holds in registers; one more column and a workgroup takes the pair."""
    return int(L.lib().uvc_logits_pair_stats_reg_max())


def logits_pair_stats(za, zb, labels=None, n_valid=None, outs=None):
    """``{name: [n]}`` over ``PAIR_STATS``: per row of the float32 logits ``za`` [n, lda] and ``zb`` [n, ldb] (columns [0, n_valid) valid,
    default: the narrower of the two), the top-1 columns, confidences, KL both ways, Jensen-Shannon, total variation, the label's NLL and
    the ranks of the label and of the other model's top-1 -- one read of both (uvc_logits_pair_stats; include/uvc_kernels.h has the
    formulas, the tie rule and the NaN rule).  ``PAIR_STATS_INT`` are int32, the rest float32.  ``labels``: contiguous int32 / int64 [n],
    or None (NLL NaN, label ranks -1).  ``outs``: a dict of contiguous tensors to write into; with it, a name that is missing or None is
    not wanted and not computed into anything."""
    L.require_cuda(za, zb, labels)
    n, ca, lda = _rows_f32(za, "logits_pair_stats: za")
    nb, cb, ldb = _rows_f32(zb, "logits_pair_stats: zb")
    if nb != n:
        raise L.UvcHipError(f"logits_pair_stats: za has {n} rows and zb {nb}")
    Cc = min(ca, cb) if n_valid is None else int(n_valid)
    if Cc > min(ca, cb):
        raise L.UvcHipError(f"logits_pair_stats: n_valid {Cc} is more than the logits' {min(ca, cb)} columns")
    i64 = 0 if labels is None else _labels_1d(labels, n, "logits_pair_stats")
    dev = za.device
    if outs is None:
        outs = {k: torch.empty(n, dtype=torch.int32 if k in PAIR_STATS_INT else torch.float32, device=dev) for k in PAIR_STATS}
    if set(outs) - set(PAIR_STATS):
        raise L.UvcHipError(f"logits_pair_stats: outs names {sorted(set(outs) - set(PAIR_STATS))} are not among {PAIR_STATS}")
    outs = {k: outs.get(k) for k in PAIR_STATS}
    _chk(*outs.values())
    for k, o in outs.items():
        if o is not None and (o.dtype != (torch.int32 if k in PAIR_STATS_INT else torch.float32) or o.numel() < n):
            raise L.UvcHipError("logits_pair_stats: outs must be int32 (top1_*, rank_*) / float32 tensors of at least n elements (or None)")
    a = L.uvc_pair_stats_args()
    a.za, a.zb, a.labels = L.ptr(za), L.ptr(zb), L.ptr(labels)
    for k, o in outs.items():
        setattr(a, k, L.ptr(o))
    a.n, a.lda, a.ldb, a.C, a.labels_i64 = n, lda, ldb, Cc, i64
    L.check(L.lib().uvc_logits_pair_stats(C.byref(a), L.cur_stream()), "uvc_logits_pair_stats")
    return outs


def _cka_width(D, what):
    if D % 8 or not 8 <= D <= OOD_MAX_D:
        raise L.UvcHipError(f"linear_cka: {what} must have a multiple of 8 columns in [8, {OOD_MAX_D}], not {D}")


def linear_cka_matrices(X, Y, chunk_rows=None):
    """(Xc^T Yc [D1, D2], Xc^T Xc [D1, D1], Yc^T Yc [D2, D2]) float32 of the column-centred float32 banks ``X`` [n, D1], ``Y`` [n, D2]: the
    column means through ``class_moments`` with one class (float64 sums, one rounding), ``center_rows``, and per chunk of ``chunk_rows``
    rows (default ``OOD_CHUNK_ROWS``) three float32 ``gemm_tn`` calls, beta = 1 after the first chunk.  The same ``chunk_rows`` gives the
    same bits."""
    L.require_cuda(X, Y)
    n, D1, _ = _rows_f32(X, "linear_cka: X")
    n2, D2, _ = _rows_f32(Y, "linear_cka: Y")
    if n2 != n:
        raise L.UvcHipError(f"linear_cka: X has {n} rows and Y {n2}")
    _cka_width(D1, "X")
    _cka_width(D2, "Y")
    dev = X.device
    zeros = torch.zeros(n, dtype=torch.int32, device=dev)
    mx, my = class_moments(X, zeros, 1)[1], class_moments(Y, zeros, 1)[1]
    chunk = max(1, min(n, OOD_CHUNK_ROWS if chunk_rows is None else int(chunk_rows)))
    bx, by = torch.empty(chunk, D1, dtype=torch.float32, device=dev), torch.empty(chunk, D2, dtype=torch.float32, device=dev)
    kxy, kxx, kyy = (torch.empty(a_, b_, dtype=torch.float32, device=dev) for a_, b_ in ((D1, D2), (D1, D1), (D2, D2)))
    ws = torch.empty(max(gemm_tn_workspace_bytes(chunk, D1, D2), gemm_tn_workspace_bytes(chunk, D1, D1), gemm_tn_workspace_bytes(chunk, D2, D2), 16),
                     dtype=torch.uint8, device=dev)
    for r0 in range(0, n, chunk):
        rows = min(chunk, n - r0)
        center_rows(X[r0:r0 + rows], zeros[r0:r0 + rows], mx, out=bx[:rows])
        center_rows(Y[r0:r0 + rows], zeros[r0:r0 + rows], my, out=by[:rows])
        beta = 0.0 if r0 == 0 else 1.0
        gemm_tn(bx, by, kxy, ws, dtype=UVC_F32, beta=beta, M=rows, N1=D1, N2=D2)
        gemm_tn(bx, bx, kxx, ws, dtype=UVC_F32, beta=beta, M=rows, N1=D1, N2=D1)
        gemm_tn(by, by, kyy, ws, dtype=UVC_F32, beta=beta, M=rows, N1=D2, N2=D2)
    return kxy, kxx, kyy


def cka_from_matrices(kxy, kxx, kyy):
    """``|Xc^T Yc|_F^2 / (|Xc^T Xc|_F |Yc^T Yc|_F)`` in float64 on the host; None when the denominator is zero (constant features)."""
    num = float(kxy.double().square().sum())
    den = float(kxx.double().square().sum().sqrt()) * float(kyy.double().square().sum().sqrt())
    return num / den if den > 0.0 else None


def linear_cka(X, Y, chunk_rows=None):
    """Linear CKA (Kornblith et al. 2019) of two float32 banks with one row per image: ``cka_from_matrices(*linear_cka_matrices(X, Y))``,
    a float, or None on constant features."""
    return cka_from_matrices(*linear_cka_matrices(X, Y, chunk_rows))


def patch_rank(scores, offset=0, descending=True, np=None):
    """int32 [B, np]: the removal order of every image's patches from float32 ``scores`` [B, ld], the patches being columns
    [offset, offset + np) (default np: the rest of the row) -- rank[b, p] patches come before p; larger score first with ``descending``,
    smaller first without, ties by index, -0 = +0, NaN last (uvc_patch_rank)."""
    _chk(scores)
    if scores.dim() != 2 or scores.dtype != torch.float32:
        raise L.UvcHipError("patch_rank: scores must be float32 [B, ld]")
    B, ld = scores.shape
    offset = int(offset)
    np = ld - offset if np is None else int(np)
    rank = torch.empty(B, max(np, 0), dtype=torch.int32, device=scores.device)
    L.check(L.lib().uvc_patch_rank(L.ptr(scores), B, ld, offset, np, int(bool(descending)), L.ptr(rank), L.cur_stream()), "uvc_patch_rank")
    return rank


def perturb_rows(rows, rank, counts, B, np, out=None):
    """[nsteps * B * np, width] in ``rows``' type: per count, a copy of the patch rows [B * np, width] (float32 or bfloat16) in which the
    rows of rank below the count are +0.0 (uvc_patch_rows_perturb).  ``rank`` int32 [B, np] (patch_rank), ``counts`` int32 [nsteps] on the
    device."""
    _chk(rows, rank, counts, out)
    B, np = int(B), int(np)
    if rows.dim() != 2 or rows.dtype not in (torch.float32, torch.bfloat16) or rows.shape[0] != B * np:
        raise L.UvcHipError("perturb_rows: rows must be float32 or bfloat16 [B * np, width]")
    if rank.dtype != torch.int32 or tuple(rank.shape) != (B, np) or counts.dtype != torch.int32 or counts.dim() != 1:
        raise L.UvcHipError("perturb_rows: rank must be int32 [B, np] and counts int32 [nsteps]")
    nsteps, width = counts.numel(), rows.shape[1]
    if out is None:
        out = torch.empty(nsteps * B * np, width, dtype=rows.dtype, device=rows.device)
    elif out.dtype != rows.dtype or tuple(out.shape) != (nsteps * B * np, width):
        raise L.UvcHipError("perturb_rows: out must be [nsteps * B * np, width] in rows' type")
    L.check(L.lib().uvc_patch_rows_perturb(L.ptr(rows), L.ptr(rank), L.ptr(counts), nsteps, B, np, width,
                                           UVC_F32 if rows.dtype == torch.float32 else UVC_BF16, L.ptr(out), L.cur_stream()),
            "uvc_patch_rows_perturb")
    return out


def logits_target(logits, target, n_valid=None):
    """(prob float32 [rows], hit int32 [rows]) of float32 ``logits`` [rows, ld]: the softmax over columns [0, n_valid) (default: all) at
    ``target[r % period]`` (int32 [period] on the device, rows a multiple of period), and whether that column is the first maximum
    (uvc_logits_target)."""
    _chk(logits, target)
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise L.UvcHipError("logits_target: logits must be float32 [rows, ld]")
    if target.dim() != 1 or target.dtype != torch.int32:
        raise L.UvcHipError("logits_target: target must be int32 [period]")
    rows, ld = logits.shape
    n_valid = ld if n_valid is None else int(n_valid)
    prob = torch.empty(rows, dtype=torch.float32, device=logits.device)
    hit = torch.empty(rows, dtype=torch.int32, device=logits.device)
    L.check(L.lib().uvc_logits_target(L.ptr(logits), rows, ld, n_valid, L.ptr(target), target.numel(), L.ptr(prob), L.ptr(hit), L.cur_stream()),
            "uvc_logits_target")
    return prob, hit


def _row_dtype(t, what):
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise L.UvcHipError(f"{what}: rows must be float32 or bfloat16")
    return UVC_F32 if t.dtype == torch.float32 else UVC_BF16


def unpatchify(rows, C, S, P, out=None):
    """float32 [B, C, S, S] from float32 patch rows [B * np, C * P * P]: the exact inverse of ``patchify`` (uvc_unpatchify)."""
    _chk(rows, out)
    C, S, P = int(C), int(S), int(P)
    if P < 1 or S < 1 or S % P:
        raise L.UvcHipError("unpatchify: S must be a positive multiple of P")
    npatch = (S // P) ** 2
    if rows.dim() != 2 or rows.dtype != torch.float32 or rows.shape[1] != C * P * P or rows.shape[0] % npatch or rows.shape[0] == 0:
        raise L.UvcHipError("unpatchify: rows must be float32 [B * np, C * P * P]")
    B = rows.shape[0] // npatch
    if out is None:
        out = torch.empty(B, C, S, S, dtype=torch.float32, device=rows.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, C, S, S):
        raise L.UvcHipError("unpatchify: out must be float32 [B, C, S, S]")
    L.check(L.lib().uvc_unpatchify(L.ptr(rows), L.ptr(out), B, C, S, P, L.cur_stream()), "uvc_unpatchify")
    return out


def ig_rows(x, x0, first_step, count, steps, out=None):
    """[count * R, width] in ``x``'s type: the interpolated inputs ``x0 + alpha_s (x - x0)``, ``alpha_s = (first_step + s + 1/2) / steps``,
    s < count, of the patch rows ``x`` [R, width] (float32 or bfloat16) and the baseline rows ``x0`` (same shape and type, or None for
    zeros), float32 arithmetic rounded once (uvc_ig_rows)."""
    _chk(x, x0, out)
    dt = _row_dtype(x, "ig_rows")
    if x.dim() != 2 or (x0 is not None and (x0.dtype != x.dtype or x0.shape != x.shape)):
        raise L.UvcHipError("ig_rows: x must be [R, width] and x0 None or of x's shape and type")
    R, width = x.shape
    count = int(count)
    if out is None:
        out = torch.empty(max(count, 0) * R, width, dtype=x.dtype, device=x.device)
    elif out.dtype != x.dtype or tuple(out.shape) != (count * R, width):
        raise L.UvcHipError("ig_rows: out must be [count * R, width] in x's type")
    L.check(L.lib().uvc_ig_rows(L.ptr(x), L.ptr(x0), L.ptr(out), R, width, int(first_step), count, int(steps), dt, L.cur_stream()), "uvc_ig_rows")
    return out


def ig_accumulate(d_rows, acc, first):
    """``acc`` float32 [R, width] = (0 if ``first`` else acc) + the sum over s, ascending, of ``d_rows`` float32 [count * R, width]
    (uvc_ig_accumulate)."""
    _chk(d_rows, acc)
    if d_rows.dtype != torch.float32 or acc.dtype != torch.float32 or acc.numel() == 0 or d_rows.numel() == 0 or d_rows.numel() % acc.numel():
        raise L.UvcHipError("ig_accumulate: float32 d_rows [count * R, width] and acc [R, width]")
    L.check(L.lib().uvc_ig_accumulate(L.ptr(d_rows), L.ptr(acc), acc.numel(), d_rows.numel() // acc.numel(), int(bool(first)), L.cur_stream()),
            "uvc_ig_accumulate")
    return acc


def pixel_maps(a, C, S, P, x=None, x0=None, scale=1.0):
    """``(pixel float32 [B, S, S], patch float32 [B, np], total float32 [B])`` of float32 gradient rows ``a`` [B * np, C * P * P]: per element
    ``e = a * scale``, or ``a * (x - x0) * scale`` with the patch rows ``x`` (and ``x0``; float32 or bfloat16) given; sum_c |e| per pixel,
    the sum of |e| per patch, the signed sum of e per image (uvc_pixel_maps)."""
    _chk(a, x, x0)
    C, S, P = int(C), int(S), int(P)
    if P < 1 or S < 1 or S % P:
        raise L.UvcHipError("pixel_maps: S must be a positive multiple of P")
    npatch = (S // P) ** 2
    if a.dim() != 2 or a.dtype != torch.float32 or a.shape[1] != C * P * P or a.shape[0] % npatch or a.shape[0] == 0:
        raise L.UvcHipError("pixel_maps: a must be float32 [B * np, C * P * P]")
    dt = UVC_F32
    if x is not None:
        dt = _row_dtype(x, "pixel_maps")
        if x.shape != a.shape or (x0 is not None and (x0.shape != a.shape or x0.dtype != x.dtype)):
            raise L.UvcHipError("pixel_maps: x (and x0) must have a's shape, x0 x's type")
    elif x0 is not None:
        raise L.UvcHipError("pixel_maps: a baseline goes with x")
    B, dev = a.shape[0] // npatch, a.device
    pixel = torch.empty(B, S, S, dtype=torch.float32, device=dev)
    patch = torch.empty(B, npatch, dtype=torch.float32, device=dev)
    total = torch.empty(B, dtype=torch.float32, device=dev)
    partial = torch.empty(B * npatch, dtype=torch.float32, device=dev)
    L.check(L.lib().uvc_pixel_maps(L.ptr(a), L.ptr(x), L.ptr(x0), float(scale), B, C, S, P, dt, L.ptr(pixel), L.ptr(patch), L.ptr(total),
                                   L.ptr(partial), L.cur_stream()), "uvc_pixel_maps")
    return pixel, patch, total


LOSS_KINDS = ("ce", "margin")                       # uvc_loss_seed's kind 0 / 1


def loss_seed(logits, labels, n_valid=None, kind="ce", logits_dist=None, dl=None, dld=None, want_loss=True):
    """``(dl, dld or None, loss float32 [B] or None)`` of float32 ``logits`` [B, ld] (and ``logits_dist``: the eval logits are their mean)
    and int32 ``labels`` [B] on the device: the attack loss ``kind`` ("ce": lse(z) - z_y; "margin": z_j - z_y, j the first maximum among the
    other labels) over columns [0, n_valid) and its gradient at the head outputs -- dz, or dz / 2 on both heads (uvc_loss_seed)."""
    _chk(logits, logits_dist, labels, dl, dld)
    if logits.dim() != 2 or logits.dtype != torch.float32 or (logits_dist is not None and (logits_dist.dtype != torch.float32 or logits_dist.shape != logits.shape)):
        raise L.UvcHipError("loss_seed: logits (and logits_dist) must be float32 [B, ld]")
    B, ld = logits.shape
    if labels.dtype != torch.int32 or tuple(labels.shape) != (B,):
        raise L.UvcHipError("loss_seed: labels must be int32 [B]")
    if kind not in LOSS_KINDS:
        raise L.UvcHipError(f"loss_seed: kind must be one of {LOSS_KINDS}")
    n_valid = ld if n_valid is None else int(n_valid)
    if dl is None:
        dl = torch.empty_like(logits)
    if dld is None and logits_dist is not None:
        dld = torch.empty_like(logits)
    for t in (dl, dld):
        if t is not None and (t.dtype != torch.float32 or t.shape != logits.shape):
            raise L.UvcHipError("loss_seed: dl / dld must be float32 [B, ld]")
    loss = torch.empty(B, dtype=torch.float32, device=logits.device) if want_loss else None
    L.check(L.lib().uvc_loss_seed(L.ptr(logits), L.ptr(logits_dist), L.ptr(labels), B, ld, n_valid, LOSS_KINDS.index(kind), L.ptr(dl),
                                  L.ptr(dld if logits_dist is not None else None), L.ptr(loss), L.cur_stream()), "uvc_loss_seed")
    return dl, (dld if logits_dist is not None else None), loss


def _channel_floats(v, Cc, what):
    import ctypes as C
    v = [float(u) for u in (v.tolist() if hasattr(v, "tolist") else v)]
    if len(v) != Cc:
        raise L.UvcHipError(f"pgd_step: {what} must hold one value per channel ({Cc})")
    return (C.c_float * Cc)(*v)


def pgd_step(x, x0, direction, P, step, eps, lo, hi, mode=0, out=None, out_t=None):
    """``out`` float32 [rows, K0]: one projected step on float32 patch rows (``patchify``'s layout) --
    ``min(max(x + step_c d, max(x0 - eps_c, lo_c)), min(x0 + eps_c, hi_c))`` with ``d = sign(direction)`` (``mode`` 0; NaN and zeros give 0) or
    ``d = direction`` (``mode`` 1), every operation a float32 operation rounded once; ``step``, ``eps``, ``lo``, ``hi``: one float per channel
    on the host.  ``out`` may be ``x`` (default: a new tensor); ``out_t`` (float32 or bfloat16 [rows, K0]): the same values rounded once to its
    type, written in the same pass (uvc_pgd_step)."""
    _chk(x, x0, direction, out, out_t)
    P = int(P)
    if x.dim() != 2 or x.dtype != torch.float32 or P < 1 or x.shape[1] % (P * P) or x.shape[0] == 0:
        raise L.UvcHipError("pgd_step: x must be float32 [rows, C * P * P]")
    Cc = x.shape[1] // (P * P)
    if out is None:
        out = torch.empty_like(x)
    for t in (x0, direction, out):
        if t.dtype != torch.float32 or t.shape != x.shape:
            raise L.UvcHipError("pgd_step: x0, direction and out must be float32 of x's shape")
    dt = UVC_F32
    if out_t is not None:
        dt = _row_dtype(out_t, "pgd_step")
        if out_t.shape != x.shape:
            raise L.UvcHipError("pgd_step: out_t must have x's shape")
    args = [_channel_floats(v, Cc, n) for v, n in ((step, "step"), (eps, "eps"), (lo, "lo"), (hi, "hi"))]
    L.check(L.lib().uvc_pgd_step(L.ptr(x), L.ptr(x0), L.ptr(direction), x.shape[0], P, Cc, *args, int(mode), L.ptr(out), L.ptr(out_t), dt,
                                 L.cur_stream()), "uvc_pgd_step")
    return out


GATE_GROUPS = (1, 16, 32, 48, 64)                   # uvc_gate_dots' group widths


def gate_dots(a, da, B, group, aux=None, out=None, col0=0):
    """``out`` float32 [B, ld_out] with ``out[b, col0 + g] = sum_n sum_{c in group g} a * da`` over image b's rows of ``a`` and ``da``
    [B * N, width] (row-major views with a unit column stride), float64 arithmetic rounded once (uvc_gate_dots).  Plain form: ``da`` of
    ``a``'s type (float32 or bfloat16), returns ``out``.  Fused form (``aux`` given, of ``a``'s type and shape): ``da`` float32, returns
    ``(out, dA)`` with ``dA = (da * aux.float()).to(a.dtype)`` written in the same pass."""
    L.require_cuda(a, da, aux, out)                  # (strided row views are the point: leading dimensions go to the kernel)
    dt = _row_dtype(a, "gate_dots")
    B, group, col0 = int(B), int(group), int(col0)
    fused = aux is not None
    ok = lambda t: t.dim() == 2 and t.shape == a.shape and (t.shape[1] == 1 or t.stride(1) == 1)
    if not ok(a) or not ok(da) or (fused and not ok(aux)) or B < 1 or a.shape[0] % B or a.shape[0] == 0:
        raise L.UvcHipError("gate_dots: a, da (and aux) must be [B * N, width] views of one shape with a unit column stride")
    if da.dtype != (torch.float32 if fused else a.dtype) or (fused and aux.dtype != a.dtype):
        raise L.UvcHipError("gate_dots: da has a's type (plain form) or is float32 beside aux of a's type (fused form)")
    M, width = a.shape
    if group not in GATE_GROUPS or width % group:
        raise L.UvcHipError(f"gate_dots: group must be one of {GATE_GROUPS} and divide the width")
    if out is None:
        out = torch.empty(B, col0 + width // group, dtype=torch.float32, device=a.device)
    elif out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != B or out.stride(1) != 1:
        raise L.UvcHipError("gate_dots: out must be float32 [B, ld_out]")
    ld = lambda t: t.stride(0) if M > 1 else width
    dA = torch.empty_like(a, memory_format=torch.contiguous_format) if fused else None
    L.check(L.lib().uvc_gate_dots(L.ptr(a), ld(a), L.ptr(da), ld(da), L.ptr(aux), ld(aux) if fused else 0, L.ptr(dA), width if fused else 0, B,
                                  M // B, width, group, L.ptr(out), out.stride(0) if B > 1 else out.shape[1], col0, dt, L.cur_stream()),
            "uvc_gate_dots")
    return (out, dA) if fused else out


def gate_accumulate(s, sum_sq, sum_abs):
    """``sum_sq[g] += s[b, g]^2`` and ``sum_abs[g] += |s[b, g]|`` (float64 [G] each, in place) over the rows of ``s`` float32 [B, G], b
    ascending: one chain per gate, so the sums over a split do not depend on how it was batched (uvc_gate_accumulate)."""
    L.require_cuda(s, sum_sq, sum_abs)
    if s.dim() != 2 or s.dtype != torch.float32 or s.shape[0] == 0 or s.shape[1] == 0 or s.stride(1) != 1:
        raise L.UvcHipError("gate_accumulate: s must be float32 [B, G]")
    B, G = s.shape
    for t in (sum_sq, sum_abs):
        if t.dtype != torch.float64 or tuple(t.shape) != (G,) or not t.is_contiguous():
            raise L.UvcHipError("gate_accumulate: sum_sq and sum_abs must be contiguous float64 [G]")
    L.check(L.lib().uvc_gate_accumulate(L.ptr(s), s.stride(0) if B > 1 else G, B, G, L.ptr(sum_sq), L.ptr(sum_abs), L.cur_stream()),
            "uvc_gate_accumulate")
    return sum_sq, sum_abs


def image_crop_desc_dtype():
    """numpy dtype with the layout of uvc_image_crop_desc: a crop window inside an image of a resident store."""
    import numpy as np
    return np.dtype(L.uvc_image_crop_desc)


def image_prep_crops_workspace(desc, S: int, store_bytes: int, filter=None) -> int:
    """image_prep_workspace for crop descriptors (numpy array of image_crop_desc_dtype()): every crop must lie inside its image and
    every image inside the ``store_bytes`` of the store (host only).  ``filter`` None: uvc_image_prep_crops_workspace (bilinear); a
    UVC_IMAGE_FILTER_* value: uvc_image_prep_crops_workspace_filter."""
    if desc.dtype != image_crop_desc_dtype() or not desc.flags.c_contiguous:
        raise L.UvcHipError("image_prep_crops_workspace: desc must be a C-contiguous array of image_crop_desc_dtype()")
    out = C.c_int64(0)
    if filter is None:
        L.check(L.lib().uvc_image_prep_crops_workspace(desc.ctypes.data, len(desc), int(S), int(store_bytes), C.byref(out)),
                "uvc_image_prep_crops_workspace")
    else:
        L.check(L.lib().uvc_image_prep_crops_workspace_filter(desc.ctypes.data, len(desc), int(S), int(store_bytes), int(filter), C.byref(out)),
                "uvc_image_prep_crops_workspace_filter")
    return int(out.value)


def image_prep_crops(store, desc_dev, workspace, out, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), filter=0):
    """image_prep reading crop windows of ``store`` (uint8 device tensor: stored images back to back) in place: bit for bit image_prep
    on the crops copied out contiguously -- three launches."""
    a = _image_prep_args("image_prep_crops", L.uvc_image_prep_crops_args, L.uvc_image_crop_desc, store, desc_dev, workspace, out, mean, std,
                         filter)
    L.check(L.lib().uvc_image_prep_crops(C.byref(a), L.cur_stream()), "uvc_image_prep_crops")
    return out
