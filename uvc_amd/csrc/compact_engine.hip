// Compact-model sequencers (include/uvc_vit.h, uvc_vit_compact_*): a pruned DeiT exported at its kept widths (uvc_amd/compact.py) --
// per block LayerNorm1, qkv GEMM, attention with a value head dim of its own (uvc_attn_args.v_dim), proj GEMM (+ bias + residual),
// LayerNorm2, fc1 (+ bias, GELU), fc2 (+ bias + residual).  Host code (but for the start vector of the rollout and the target pick of the attribution); every arithmetic step is one of the kernels behind
// uvc_kernels.h, the embedding, token assembly, final norm and heads as uvc_vit_forward runs them.
// ONE forward body serves evaluation (uvc_vit_compact_forward) and fine-tuning (uvc_vit_compact_train_forward): the same kernels in the
// same order on one stream.  The modes differ in where a block's buffers live (carve: one shared set in eval, a set per block that
// the backward reads in training) and in the fc1 epilogue (training also keeps GELU').  uvc_vit_compact_backward walks the blocks in
// reverse: plain GEMMs and the attention backward at a value width.  uvc_vit_compact_rollout is the eval forward with qkv and lse kept
// per attention block, then one uvc_attention_rollout_step per such block, last block first.  uvc_vit_compact_attribution is the training forward,
// a target pick, and the same backward walk without any parameter gradient, with one uvc_attention_relevance_step per attention block.
// uvc_vit_compact_input_grad is that forward and target pick, the dgrad walk through every block, the masked row copy of token assembly's
// backward and the patch-embedding dgrad: the gradient of the class logit at the input, as patch rows.  uvc_vit_compact_loss_grad is the same
// with the seed of an attack loss (uvc_loss_seed, robust.hip) in the target pick's place.  uvc_vit_compact_gate_grads is the training forward, the
// cross-entropy seed and the dgrad walk with one uvc_gate_dots (prune.hip) behind each attn.proj dgrad and one in place of each fc2 dgrad's epilogue.
#include "engine_host.h"

namespace {

struct CDims : Dims {
  int maxQ, maxO, maxH, maxF;    // widest qkv row, attention output row, head count and hidden width over the blocks
};

// rows of a block's qkv matrix (64 q and 64 k dims per kept head, v_dim value dims) and columns of its attention output
int qkv_rows(const uvc_compact_block& b) { return b.heads * (128 + b.v_dim); }
int attn_cols(const uvc_compact_block& b) { return b.heads * b.v_dim; }
// the four matrices of a block as [out, in] -- qkv, proj, fc1, fc2: parameter slots 2, 4, 8, 10, shadow slots 0..3
struct Mats { int64_t R[4], C[4]; };
Mats mats_of(const uvc_compact_block& b, int D) { return {{qkv_rows(b), D, b.hidden, D}, {D, attn_cols(b), D, b.hidden}}; }
constexpr int MAT_SLOT[4] = {2, 4, 8, 10};

int check_blocks(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int nblocks) {
  TRY(uvc_vit_layout(cfg, nullptr, nullptr));              // the dense model's checks (dims, dtype, ntok, classes, patches)
  if (cfg->no_qkv_bias) return uvc_set_error_msg(UVC_ERR_UNSUPPORTED, "uvc_vit_compact: DeiT blocks (qkv bias)");
  if (nblocks < 0 || nblocks > cfg->depth || (nblocks > 0 && !blocks)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact: nblocks out of range");
  for (int k = 0; k < nblocks; ++k) {
    const uvc_compact_block& b = blocks[k];
    if (b.heads < 0 || b.heads > cfg->num_heads || b.hidden < 0 || b.hidden > cfg->hidden || b.hidden % 16)
      return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact: block widths out of range (heads <= num_heads, hidden <= cfg.hidden, hidden % 16 == 0)");
    if (b.heads > 0 ? (b.v_dim != 16 && b.v_dim != 32 && b.v_dim != 48 && b.v_dim != 64) : b.v_dim != 0)
      return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact: v_dim must be 16, 32, 48 or 64 (0 with no heads)");
  }
  return UVC_OK;
}

CDims cdims_of(const uvc_vit_cfg& c, const uvc_compact_block* blocks, int nblocks, int B) {
  CDims d;
  static_cast<Dims&>(d) = dims_of(c, B);
  d.maxQ = d.maxO = d.maxH = d.maxF = 0;
  for (int k = 0; k < nblocks; ++k) {
    const uvc_compact_block& b = blocks[k];
    if (qkv_rows(b) > d.maxQ) d.maxQ = qkv_rows(b);
    if (attn_cols(b) > d.maxO) d.maxO = attn_cols(b);
    if (b.heads > d.maxH) d.maxH = b.heads;
    if (b.hidden > d.maxF) d.maxF = b.hidden;
  }
  return d;
}

constexpr int TRAIN_MAX_N = 256;     // the attention backward at a value width (uvc_attention_bwd_vdim) takes N <= 256

int check_train(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int nblocks) {
  TRY(check_blocks(cfg, blocks, nblocks));
  if (cfg->dtype == UVC_BF16 && cfg->resid_f32) return uvc_set_error_msg(UVC_ERR_UNSUPPORTED, "uvc_vit_compact training: bf16 residual rows only (cfg.resid_f32 = 0)");
  const int np = (cfg->img_size / cfg->patch_size) * (cfg->img_size / cfg->patch_size);
  if (np + cfg->ntok > TRAIN_MAX_N) return uvc_set_error_msg(UVC_ERR_UNSUPPORTED, "uvc_vit_compact training: sequences of at most 256 tokens (the attention backward at a value width)");
  return UVC_OK;
}

// ---- workspace -------------------------------------------------------------------------------------------------------------------
// Block k's buffers.  Training: its own, kept for the backward; x1 / xo (residual-stream rows [M, D]) only where the branch has a GEMM
// (a bias-only branch adds in place).  Eval: every block points at one shared set sized by the widest block (h1 = h2, one mean / rstd
// pair, no gp), and x1 / xo alternate between two residual-row buffers.  Rollout (CARVE_ROLLOUT): the eval set, but every block with heads
// owns its qkv and lse (the reverse sweep reads them), and two [B, N] float vectors behind everything else.  Attribution (CARVE_ATTRIB): the
// training set, and behind it the two [B, N] vectors, the one-hot logit gradients and 2 D floats the LayerNorm backward's parameter-gradient
// pointers aim at (never reduced into: see ln_bwd).  Input gradient (CARVE_INPUT): the training set, the one-hot logit gradients and the 2 D
// floats, the [K0, D] transposed patch-embedding weight (T) and the (N + 2) D floats that take the batch sums of uvc_assemble_tokens_bwd.
// Gate gradients (CARVE_GATES): the training set, the logit gradients and the 2 D floats, and the float32 [M, widest hidden] raw fc2 dgrad.
enum { CARVE_EVAL = 0, CARVE_TRAIN = 1, CARVE_ROLLOUT = 2, CARVE_ATTRIB = 3, CARVE_INPUT = 4, CARVE_GATES = 5 };
struct BlockBufs {
  void* h1; void* qkv; void* o; float* lse; float* mean1; float* rstd1; void* x1;
  void* h2; float* mean2; float* rstd2; void* gp; void* u; void* xo;
};
struct Work {
  void* patches; float* pe; void* x0; BlockBufs blk[UVC_VIT_MAX_DEPTH];
  void* hc; float* meanf; float* rstdf; float* ones;
  // backward: the dL/dx stream ping-pongs between g[0] and g[1] (T: bf16, or float32 in the exact mode)
  void* g[2]; void* dA; void* dH; void* dO; void* dqkv; float* delta; float* ln_partial; int64_t ln_region; float* cs_partial;
  void* tn_ws; int64_t tn_ws_bytes; void* dhc; void* dpe;
  float* roll[2];      // rollout, attribution: the row vector ping-pongs between them
  float* dl[2]; float* ln_scratch;      // attribution, input gradient: d_logits (/ d_logits_dist) [B, NC], the unused dgamma | dbeta [2 D]
  void* wpt; float* asm_scratch;        // input gradient: W_patch^T [K0, D] (T), the unused dpos [N, D] | dcls [D] | ddist [D]
  float* dh;                            // gate gradients: g . W2 [M, maxF] before GELU' (uvc_gate_dots' fused form makes dA of it)
};

int64_t train_tn_ws(const CDims& d, const uvc_compact_block* blocks, int nblocks) {
  int64_t best = 0, b; int s;
  auto one = [&](int M, int N1, int N2) { if (N1 > 0 && N2 > 0) { uvc_gemm_tn_workspace_bytes(M, N1, N2, &b, &s); if (b > best) best = b; } };
  one(d.B, d.NC, d.D); one(d.B * d.np, d.D, d.K0);
  for (int k = 0; k < nblocks; ++k) {
    const int nq = qkv_rows(blocks[k]), no = attn_cols(blocks[k]), F = blocks[k].hidden;
    one(d.M, d.D, F); one(d.M, F, d.D); one(d.M, d.D, no); one(d.M, nq, d.D);
  }
  return best;
}

int64_t carve(const CDims& d, const uvc_compact_block* blocks, int nblocks, int mode, char* base, Work& w) {
  const bool training = mode == CARVE_TRAIN || mode == CARVE_ATTRIB || mode == CARVE_INPUT || mode == CARVE_GATES;
  Carver c{base, 0};
  const int64_t M = d.M, MD = M * d.D;
  memset(&w, 0, sizeof(w));
  w.patches = c.take((int64_t)d.B * d.np * d.K0 * d.tsz);
  w.pe = (float*)c.take((int64_t)d.B * d.np * d.D * 4);
  w.x0 = c.take(MD * d.rsz);
  BlockBufs shared = {};
  void* r[2] = {w.x0, nullptr};
  int cur = 0;
  if (!training) {
    r[1] = c.take(MD * d.rsz);
    shared.h1 = shared.h2 = c.take(MD * d.tsz);
    if (mode == CARVE_EVAL) shared.qkv = c.take(M * d.maxQ * d.tsz);
    shared.o = c.take(M * d.maxO * d.tsz);
    if (mode == CARVE_EVAL) shared.lse = (float*)c.take((int64_t)d.B * d.maxH * d.N * 4);
    shared.u = c.take(M * d.maxF * d.tsz);
    shared.mean1 = shared.mean2 = (float*)c.take(M * 4); shared.rstd1 = shared.rstd2 = (float*)c.take(M * 4);
  }
  for (int k = 0; k < nblocks; ++k) {
    BlockBufs& b = w.blk[k];
    const int64_t nq = qkv_rows(blocks[k]), no = attn_cols(blocks[k]), F = blocks[k].hidden;
    if (!training) {      // the rows a GEMM writes go to the buffer its residual operand is not in
      b = shared;
      if (blocks[k].heads > 0) b.x1 = r[cur ^= 1];
      if (F > 0) b.xo = r[cur ^= 1];
      if (mode == CARVE_ROLLOUT && blocks[k].heads > 0) {
        b.qkv = c.take(M * nq * d.tsz);
        b.lse = (float*)c.take((int64_t)d.B * blocks[k].heads * d.N * 4);
      }
      continue;
    }
    if (blocks[k].heads > 0) {
      b.h1 = c.take(MD * d.tsz); b.qkv = c.take(M * nq * d.tsz); b.o = c.take(M * no * d.tsz);
      b.lse = (float*)c.take((int64_t)d.B * blocks[k].heads * d.N * 4);
      b.mean1 = (float*)c.take(M * 4); b.rstd1 = (float*)c.take(M * 4);
      b.x1 = c.take(MD * d.rsz);
    }
    if (F > 0) {
      b.h2 = c.take(MD * d.tsz); b.mean2 = (float*)c.take(M * 4); b.rstd2 = (float*)c.take(M * 4);
      b.gp = c.take(M * F * d.tsz); b.u = c.take(M * F * d.tsz);
      b.xo = c.take(MD * d.rsz);
    }
  }
  w.hc = c.take((int64_t)d.B * d.ntok * d.D * d.tsz);
  w.meanf = (float*)c.take((int64_t)d.B * d.ntok * 4); w.rstdf = (float*)c.take((int64_t)d.B * d.ntok * 4);
  w.ones = (float*)c.take(M * 4);
  if (mode == CARVE_ROLLOUT) { w.roll[0] = (float*)c.take(M * 4); w.roll[1] = (float*)c.take(M * 4); }
  if (!training) return c.off;
  w.g[0] = c.take(MD * d.tsz); w.g[1] = c.take(MD * d.tsz);
  w.dA = c.take(M * (d.maxF > 0 ? d.maxF : 1) * d.tsz);
  w.dH = c.take(MD * d.tsz);
  w.dO = c.take(M * (d.maxO > 0 ? d.maxO : 1) * d.tsz);
  w.dqkv = c.take(M * (d.maxQ > 0 ? d.maxQ : 1) * d.tsz);
  w.delta = (float*)c.take((int64_t)d.B * (d.maxH > 0 ? d.maxH : 1) * d.N * 4);
  w.ln_region = (int64_t)uvc_layernorm_bwd_blocks(d.M) * (2 * d.D + 2);
  w.ln_partial = (float*)c.take(w.ln_region * 4 * (2 * nblocks + 1));
  w.cs_partial = (float*)c.take((int64_t)uvc_colsum_blocks(d.M) * d.D * 4);
  w.tn_ws_bytes = train_tn_ws(d, blocks, nblocks);
  w.tn_ws = c.take(w.tn_ws_bytes);
  w.dhc = c.take((int64_t)d.B * d.ntok * d.D * d.tsz);
  w.dpe = c.take((int64_t)d.B * d.np * d.D * d.tsz);
  if (mode == CARVE_ATTRIB) { w.roll[0] = (float*)c.take(M * 4); w.roll[1] = (float*)c.take(M * 4); }
  if (mode == CARVE_ATTRIB || mode == CARVE_INPUT || mode == CARVE_GATES) {
    w.dl[0] = (float*)c.take((int64_t)d.B * d.NC * 4); w.dl[1] = (float*)c.take((int64_t)d.B * d.NC * 4);
    w.ln_scratch = (float*)c.take((int64_t)2 * d.D * 4);
  }
  if (mode == CARVE_INPUT) {
    w.wpt = c.take((int64_t)d.K0 * d.D * d.tsz);
    w.asm_scratch = (float*)c.take((int64_t)(d.N + 2) * d.D * 4);
  }
  if (mode == CARVE_GATES) w.dh = (float*)c.take(M * (d.maxF > 0 ? d.maxF : 1) * 4);
  return c.off;
}

// the residual-stream rows of block k: its input, the rows behind the attention branch, its output (aliases where a branch is a bias)
struct Chain { void* xin[UVC_VIT_MAX_DEPTH + 1]; void* x1[UVC_VIT_MAX_DEPTH]; };
Chain chain_of(const Work& w, const uvc_compact_block* blocks, int nblocks) {
  Chain ch;
  ch.xin[0] = w.x0;
  for (int k = 0; k < nblocks; ++k) {
    ch.x1[k] = blocks[k].heads > 0 ? w.blk[k].x1 : ch.xin[k];
    ch.xin[k + 1] = blocks[k].hidden > 0 ? w.blk[k].xo : ch.x1[k];
  }
  return ch;
}

// ---- small helpers around the kernel entry points ----------------------------------------------------------------------------------
struct Ctx { CDims d; const uvc_vit_io* io; void* st; Work w; uvc_ln_reduce_item ln_items[64]; int n_ln; };

// fills the context and carves io->workspace; false when the workspace is too small for the mode
bool bind(Ctx& c, const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int nblocks, const uvc_vit_io* io, void* stream, int mode) {
  c.d = cdims_of(*cfg, blocks, nblocks, io->batch); c.io = io; c.st = stream; c.n_ln = 0;
  const int64_t need = carve(c.d, blocks, nblocks, mode, (char*)io->workspace, c.w);
  if (io->patches_in) c.w.patches = const_cast<void*>(io->patches_in);
  return io->workspace_bytes >= need;
}

// C[M,N] = epi(A[M,K] . B[N,K]^T); B: a shadow copy (bf16 mode) or the float32 master weights
int nt(const Ctx& c, const void* A, int a_f32, const void* B, void* C, int c_f32, int M, int N, int K, int epi, const float* bias = nullptr,
       const void* R = nullptr, const void* aux = nullptr, void* C2 = nullptr, int lda = 0, int ldc = 0) {
  uvc_gemm_nt_args a;
  memset(&a, 0, sizeof(a));
  a.A = A; a.B = B; a.C = C; a.C2 = C2; a.bias = bias; a.R = R; a.aux = aux;
  a.alpha = 1.0f; a.M = M; a.N = N; a.K = K; a.lda = lda ? lda : K; a.ldb = K; a.ldc = ldc ? ldc : N; a.ldr = a.ldc; a.ldaux = a.ldc;
  a.dtype = c.d.dtype; a.a_is_f32 = a_f32 || c.d.dtype == UVC_F32; a.c_is_f32 = c_f32 || c.d.dtype == UVC_F32; a.epilogue = epi;
  a.r_is_f32 = a.c_is_f32;
  return uvc_gemm_nt(&a, c.st);
}
// C[N1,N2] = A[M,N1]^T . B[M,N2] and bias_grad[N1] = column sums of A (the weight and bias gradient of a Linear, one pass)
int tn(const Ctx& c, const void* A, int a_f32, const void* B, float* C, float* bias_grad, int M, int N1, int N2, int lda = 0, int ldb = 0) {
  uvc_gemm_tn_args a;
  memset(&a, 0, sizeof(a));
  a.A = A; a.B = B; a.C = C; a.colsum_out = bias_grad; a.workspace = c.w.tn_ws; a.workspace_bytes = c.w.tn_ws_bytes;
  a.alpha = 1.0f; a.beta = 0.f; a.M = M; a.N1 = N1; a.N2 = N2; a.lda = lda ? lda : N1; a.ldb = ldb ? ldb : N2; a.ldc = N2;
  a.dtype = c.d.dtype; a.a_is_f32 = a_f32 || c.d.dtype == UVC_F32;
  return uvc_gemm_tn(&a, c.st);
}
int ln_fwd(const Ctx& c, const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int rows, int rpg, int64_t gs) {
  uvc_ln_args a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.x_lowp = c.d.rlow; a.gamma = gamma; a.beta = beta; a.y = y; a.mean = mean; a.rstd = rstd; a.eps = c.d.eps;
  a.rows = rows; a.D = c.d.D; a.rows_per_group = rpg; a.group_stride = gs; a.dtype = c.d.dtype;
  return uvc_layernorm_fwd(&a, c.st);
}
int flush_ln(Ctx& c) {
  if (c.n_ln == 0) return UVC_OK;
  const int e = uvc_layernorm_bwd_reduce_batch(c.ln_items, c.n_ln, c.d.D, 0.f, c.st);
  c.n_ln = 0;
  return e;
}
// dx = LN'(dy; x) + add1; dgamma / dbeta through the batched reduction at the end of the pass.  dgamma == nullptr (attribution): uvc_layernorm_bwd
// has no form without the per-block partial sums, so they go to the slot as ever, no reduction is queued, and the two pointers it insists on
// aim at the workspace's 2 D scratch floats, which nothing writes
int ln_bwd(Ctx& c, int slot, const void* dy, const void* x, const float* gamma, float* dgamma, float* dbeta, const float* mean, const float* rstd,
           void* dx, const void* add1, int rows, int rpg, int64_t gs) {
  if (c.n_ln == 64) TRY(flush_ln(c));
  uvc_ln_args a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.x_lowp = c.d.rlow; a.gamma = gamma; a.mean = const_cast<float*>(mean); a.rstd = const_cast<float*>(rstd); a.dy = dy; a.dx = dx; a.add1 = add1;
  a.partial = c.w.ln_partial + c.w.ln_region * slot; a.dgamma = dgamma ? dgamma : c.w.ln_scratch; a.dbeta = dgamma ? dbeta : c.w.ln_scratch + c.d.D; a.defer_reduce = 1;
  if (dgamma) {
    uvc_ln_reduce_item& it = c.ln_items[c.n_ln++];
    it.partial = a.partial; it.dgamma = dgamma; it.dbeta = dbeta; it.dots = nullptr; it.nblocks = uvc_layernorm_bwd_nblocks(rows); it.reserved = 0;
  }
  a.eps = c.d.eps; a.beta_acc = 0.f; a.rows = rows; a.D = c.d.D; a.rows_per_group = rpg; a.group_stride = gs; a.dtype = c.d.dtype;
  a.g_lowp = c.d.dtype == UVC_BF16;
  return uvc_layernorm_bwd(&a, c.st);
}
int zero_f32(const Ctx& c, float* p, int64_t n) {
  if (n <= 0) return UVC_OK;
  const hipError_t e = hipMemsetAsync(p, 0, (size_t)n * 4, (hipStream_t)c.st);
  return e == hipSuccess ? UVC_OK : uvc_set_error(e, __FILE__, __LINE__);
}

int setup_train(Ctx& c, const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int nblocks, const uvc_vit_io* io, void* stream, int mode = CARVE_TRAIN) {
  TRY(check_train(cfg, blocks, nblocks));
  if (!io || !io->params || !io->shadow || !io->workspace || io->batch <= 0) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact training: null io member (params, shadow, workspace) or batch <= 0");
  if (io->accumulate != 0.f) return uvc_set_error_msg(UVC_ERR_UNSUPPORTED, "uvc_vit_compact training: gradient accumulation (io.accumulate must be 0)");
  if (!bind(c, cfg, blocks, nblocks, io, stream, mode)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact training: workspace too small (uvc_vit_compact_train_workspace_bytes; attribution: uvc_vit_compact_attribution_workspace_bytes; input gradient: uvc_vit_compact_input_grad_workspace_bytes; gate gradients: uvc_vit_compact_gate_grads_workspace_bytes)");
  return UVC_OK;
}

// the [out, in] shadow copies of every GEMM weight and, with `transposed` (training), the [in, out] copies behind them.  float32 mode: the
// GEMMs read the master weights, so only the transposed copies are written
int update_shadows(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int nblocks, const float* params, void* shadow, void* stream, bool transposed) {
  const CDims d = cdims_of(*cfg, blocks, nblocks, 1);
  uvc_vit_offsets off; uvc_vit_shadow_offsets so;      // (the eval layout leaves every transposed slot at -1)
  TRY((transposed ? uvc_vit_compact_train_layout : uvc_vit_compact_layout)(cfg, blocks, nblocks, &off, &so));
  const bool f32 = d.dtype == UVC_F32;
  ShadowBatch sb{params, shadow, d.dtype, stream};
  auto one = [&](int64_t p, int64_t R, int64_t C, int64_t sw, int64_t swt) { return sb.add(p, R, C, f32 ? -1 : sw, swt); };
  TRY(one(off.patch_w, d.D, d.K0, so.patch_w, -1));
  for (int k = 0; k < nblocks; ++k) {
    const Mats m = mats_of(blocks[k], d.D);
    for (int j = 0; j < 4; ++j) TRY(one(off.blk[k][MAT_SLOT[j]], m.R[j], m.C[j], so.blk_w[k][j], so.blk_wt[k][j]));
  }
  TRY(one(off.head_w, d.NC, d.D, so.head_w, so.head_wt));
  if (d.ntok == 2) TRY(one(off.headd_w, d.NC, d.D, so.headd_w, so.headd_wt));
  return sb.flush();
}

// the forward of every mode; `training` keeps GELU' of fc1 beside its output (and c.w holds a buffer set per block)
int forward(Ctx& c, const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int nblocks, int training) {
  const CDims& d = c.d;
  const Work& w = c.w;
  const uvc_vit_io* io = c.io;
  void* stream = c.st;
  uvc_vit_offsets o; uvc_vit_shadow_offsets so;
  TRY(uvc_vit_compact_layout(cfg, blocks, nblocks, &o, &so));      // (the training layout appends to it: same [out, in] offsets)
  const float* P = io->params;
  auto wm = [&](int64_t poff, int64_t soff) -> const void* { return d.dtype == UVC_F32 ? (const void*)(P + poff) : (const void*)((const char*)io->shadow + soff * d.tsz); };
  const int rf = d.rlow ? 0 : 1;                           // "C is float32" of the GEMMs that write residual-stream rows
  // patch embedding (PatchEmbed.forward :145-153) and token assembly with the mode-1 token mask (:434-471)
  if (!io->patches_in) TRY(uvc_patchify(io->x, w.patches, d.B, d.C, d.S, d.P, d.dtype, stream));
  TRY(nt(c, w.patches, 0, wm(o.patch_w, so.patch_w), w.pe, 1, d.B * d.np, d.D, d.K0, UVC_EPI_BIAS, P + o.patch_b));
  TRY(uvc_assemble_tokens(w.pe, P + o.cls_token, d.ntok == 2 ? P + o.dist_token : nullptr, P + o.pos_embed, io->patch_mask, w.x0, d.B, d.np,
                          d.D, d.ntok, d.rlow, stream));
  bool ones_ready = false;
  // a bias-only branch (no kept head / unit): rows += 1 * bias, in place -- the GEMM epilogue's acc + bias + R with acc = 0
  auto add_bias = [&](void* x, const float* bias) -> int {
    if (!ones_ready) {
      const hipError_t e = hipMemsetD32Async((hipDeviceptr_t)w.ones, 0x3f800000, (size_t)d.M, (hipStream_t)stream);
      if (e != hipSuccess) return uvc_set_error(e, __FILE__, __LINE__);
      ones_ready = true;
    }
    return uvc_add_outer(x, w.ones, bias, d.M, d.D, d.dtype, rf, stream);
  };
  const Chain ch = chain_of(w, blocks, nblocks);
  for (int k = 0; k < nblocks; ++k) {
    const uvc_compact_block& bk = blocks[k];
    const BlockBufs& b = w.blk[k];
    const int64_t* q = o.blk[k];
    void* xin = ch.xin[k];
    void* x1 = ch.x1[k];
    if (bk.heads > 0) {
      TRY(ln_fwd(c, xin, P + q[0], P + q[1], b.h1, b.mean1, b.rstd1, d.M, 1, d.D));
      TRY(nt(c, b.h1, 0, wm(q[2], so.blk_w[k][0]), b.qkv, 0, d.M, qkv_rows(bk), d.D, UVC_EPI_BIAS, P + q[3]));
      uvc_attn_args a;
      memset(&a, 0, sizeof(a));
      a.qkv = b.qkv; a.o = b.o; a.lse = b.lse; a.B = d.B; a.N = d.N; a.H = bk.heads; a.head_dim = 64; a.dtype = d.dtype; a.scale = 0.125f;
      a.v_dim = bk.v_dim;
      TRY(uvc_attention_fwd(&a, stream));
      TRY(nt(c, b.o, 0, wm(q[4], so.blk_w[k][1]), x1, rf, d.M, d.D, attn_cols(bk), UVC_EPI_BIAS_RESID, P + q[5], xin));
    } else {
      TRY(add_bias(x1, P + q[5]));
    }
    if (bk.hidden > 0) {
      TRY(ln_fwd(c, x1, P + q[6], P + q[7], b.h2, b.mean2, b.rstd2, d.M, 1, d.D));
      if (training)      // gp = GELU'(pre-activation), all the backward needs of it; u = GELU
        TRY(nt(c, b.h2, 0, wm(q[8], so.blk_w[k][2]), b.gp, 0, d.M, bk.hidden, d.D, UVC_EPI_BIAS_GELU_GRAD, P + q[9], nullptr, nullptr, b.u));
      else
        TRY(nt(c, b.h2, 0, wm(q[8], so.blk_w[k][2]), b.u, 0, d.M, bk.hidden, d.D, UVC_EPI_BIAS_GELU_OUT, P + q[9]));
      TRY(nt(c, b.u, 0, wm(q[10], so.blk_w[k][3]), b.xo, rf, d.M, d.D, bk.hidden, UVC_EPI_BIAS_RESID, P + q[11], x1));
    } else {
      TRY(add_bias(x1, P + q[11]));
    }
  }
  // final norm on the class (/ distillation) token rows (:507-508), then the head(s) (:522-526)
  TRY(ln_fwd(c, ch.xin[nblocks], P + o.norm_w, P + o.norm_b, w.hc, w.meanf, w.rstdf, d.B * d.ntok, d.ntok, (int64_t)d.N * d.D));
  TRY(nt(c, w.hc, 0, wm(o.head_w, so.head_w), io->logits, 1, d.B, d.NC, d.D, UVC_EPI_BIAS, P + o.head_b, nullptr, nullptr, nullptr, d.ntok * d.D));
  if (d.ntok == 2)
    TRY(nt(c, (const char*)w.hc + (size_t)d.D * d.tsz, 0, wm(o.headd_w, so.headd_w), io->logits_dist, 1, d.B, d.NC, d.D, UVC_EPI_BIAS, P + o.headd_b,
           nullptr, nullptr, nullptr, d.ntok * d.D));
  return UVC_OK;
}

}  // namespace

// ---- layouts, workspace sizes, shadow refresh -----------------------------------------------------------------------------------------
extern "C" int uvc_vit_compact_layout(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, uvc_vit_offsets* off,
                                      uvc_vit_shadow_offsets* soff) {
  TRY(check_blocks(cfg, blocks, nblocks));
  const CDims d = cdims_of(*cfg, blocks, nblocks, 1);
  if (off) {
    memset(off, 0xff, sizeof(*off));
    Slots put{0, 4};
    layout_embed(d, off, put);
    for (int k = 0; k < nblocks; ++k) {
      const int64_t nq = qkv_rows(blocks[k]), no = attn_cols(blocks[k]), F = blocks[k].hidden;
      int64_t* b = off->blk[k];
      put(b[0], d.D); put(b[1], d.D); put(b[2], nq * d.D); put(b[3], nq); put(b[4], d.D * no); put(b[5], d.D);
      put(b[6], d.D); put(b[7], d.D); put(b[8], F * d.D); put(b[9], F); put(b[10], d.D * F); put(b[11], d.D);
    }
    layout_heads(d, off, put);
    put(off->patch_gating, d.np);
    off->n_total = put.o;
  }
  if (soff) {
    memset(soff, 0xff, sizeof(*soff));
    Slots put{0, 8};
    put(soff->patch_w, (int64_t)d.D * d.K0);
    for (int k = 0; k < nblocks; ++k) {
      const Mats m = mats_of(blocks[k], d.D);
      for (int j = 0; j < 4; ++j) put(soff->blk_w[k][j], m.R[j] * m.C[j]);
    }
    put(soff->head_w, (int64_t)d.NC * d.D);
    if (d.ntok == 2) put(soff->headd_w, (int64_t)d.NC * d.D);
    soff->n_total = put.o;
  }
  return UVC_OK;
}

extern "C" int uvc_vit_compact_train_layout(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, uvc_vit_offsets* off,
                                            uvc_vit_shadow_offsets* soff) {
  TRY(check_train(cfg, blocks, nblocks));
  TRY(uvc_vit_compact_layout(cfg, blocks, nblocks, off, soff));
  if (soff) {      // the [out, in] copies keep the eval layout's offsets; the transposed copies follow them
    const CDims d = cdims_of(*cfg, blocks, nblocks, 1);
    Slots put{soff->n_total, 8};
    for (int k = 0; k < nblocks; ++k) {
      const Mats m = mats_of(blocks[k], d.D);
      for (int j = 0; j < 4; ++j) put(soff->blk_wt[k][j], m.R[j] * m.C[j]);
    }
    put(soff->head_wt, (int64_t)d.NC * d.D);
    if (d.ntok == 2) put(soff->headd_wt, (int64_t)d.NC * d.D);
    soff->n_total = put.o;
  }
  return UVC_OK;
}

extern "C" int64_t uvc_vit_compact_workspace_bytes(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, int32_t batch) {
  if (check_blocks(cfg, blocks, nblocks) || batch <= 0) return -1;
  Work w;
  return carve(cdims_of(*cfg, blocks, nblocks, batch), blocks, nblocks, 0, nullptr, w);
}

extern "C" int64_t uvc_vit_compact_train_workspace_bytes(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, int32_t batch) {
  if (check_train(cfg, blocks, nblocks)) return -1;
  if (batch <= 0) { uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_train_workspace_bytes: batch <= 0"); return -1; }
  Work w;
  return carve(cdims_of(*cfg, blocks, nblocks, batch), blocks, nblocks, 1, nullptr, w);
}

extern "C" int uvc_vit_compact_frozen_ranges(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, int64_t* ranges, int32_t cap,
                                             int32_t* count) {
  TRY(check_blocks(cfg, blocks, nblocks));
  if (!count || (cap > 0 && !ranges)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_frozen_ranges: null pointer");
  uvc_vit_offsets off;
  TRY(uvc_vit_compact_layout(cfg, blocks, nblocks, &off, nullptr));
  int n = 0;
  auto add = [&](int64_t begin, int64_t end) { if (n < cap) { ranges[2 * n] = begin; ranges[2 * n + 1] = end - begin; } ++n; };
  for (int k = 0; k < nblocks; ++k) {
    if (blocks[k].heads == 0) add(off.blk[k][0], off.blk[k][5]);          // norm1, (empty) qkv and proj.weight; proj.bias trains
    if (blocks[k].hidden == 0) add(off.blk[k][6], off.blk[k][11]);        // norm2, (empty) fc1 and fc2.weight; fc2.bias trains
  }
  *count = n;
  return n > cap ? uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_frozen_ranges: more ranges than `cap` (count holds the number)") : UVC_OK;
}

extern "C" int uvc_vit_compact_update_shadows(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, const float* params, void* shadow,
                                              void* stream) {
  TRY(check_blocks(cfg, blocks, nblocks));
  if (cfg->dtype == UVC_F32) return UVC_OK;                 // the GEMMs read the float32 master weights
  if (!params || !shadow) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_update_shadows: null pointer");
  return update_shadows(cfg, blocks, nblocks, params, shadow, stream, false);
}

extern "C" int uvc_vit_compact_train_update_shadows(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, const float* params,
                                                    void* shadow, void* stream) {
  TRY(check_train(cfg, blocks, nblocks));
  if (!params || !shadow) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_train_update_shadows: null pointer");
  return update_shadows(cfg, blocks, nblocks, params, shadow, stream, true);
}

// ---- forward (eval, training) and backward -------------------------------------------------------------------------------------------
// r[b, i] = 1 / ntok on the readout tokens (i < ntok), 0 elsewhere: device code of this file (with k_attrib_target), too small for an entry point of its own
static __global__ void k_rollout_start(float* r, int64_t n, int N, int ntok) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) r[i] = (int)(i % N) < ntok ? 1.0f / (float)ntok : 0.f;
}

static int setup_eval(Ctx& c, const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int nblocks, const uvc_vit_io* io, void* stream, int mode) {
  TRY(check_blocks(cfg, blocks, nblocks));
  if (!io || !io->params || !io->workspace || io->batch <= 0 || (!io->x && !io->patches_in) || !io->logits ||
      (cfg->ntok == 2 && !io->logits_dist))   // x is read by uvc_patchify alone: patch rows handed in (patches_in) stand for it
    return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_forward: null io member");
  if (cfg->dtype == UVC_BF16 && !io->shadow) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_forward: bf16 mode needs the shadow buffer");
  if (!bind(c, cfg, blocks, nblocks, io, stream, mode)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_forward: workspace too small");
  return UVC_OK;
}

extern "C" int uvc_vit_compact_forward(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, const uvc_vit_io* io, void* stream) {
  Ctx c;
  TRY(setup_eval(c, cfg, blocks, nblocks, io, stream, CARVE_EVAL));
  return forward(c, cfg, blocks, nblocks, 0);
}

// feats[b, :] = the mean of row b's ntok readout rows (/ max(its 2-norm, 1e-12)): one wave per row, a lane's dims in ascending order, the wave butterfly
template <typename T, typename O>
static __global__ __launch_bounds__(256) void k_readout_features(const T* __restrict__ hc, int B, int ntok, int D, int normalize, O* __restrict__ feats) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
  if (row >= B) return;
  const T* h = hc + (size_t)row * ntok * D;
  auto mean_at = [&](int d) { return ntok == 2 ? (ElemIO<T>::load(h + d) + ElemIO<T>::load(h + D + d)) * 0.5f : ElemIO<T>::load(h + d); };
  float scale = 1.f;
  if (normalize) {
    float ss = 0.f;
    for (int d = l; d < D; d += 64) { const float m = mean_at(d); ss = fmaf(m, m, ss); }
    scale = fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
  }
  for (int d = l; d < D; d += 64) ElemIO<O>::store(feats + (size_t)row * D + d, normalize ? __fdiv_rn(mean_at(d), scale) : mean_at(d));
}

extern "C" int uvc_vit_compact_features(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, const uvc_vit_io* io, void* feats,
                                        int32_t normalize, int32_t feats_dtype, void* stream) {
  if (!feats) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_features: null feats");
  if (feats_dtype != UVC_F32 && feats_dtype != UVC_BF16) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_features: feats_dtype must be UVC_F32 or UVC_BF16");
  Ctx c;
  TRY(setup_eval(c, cfg, blocks, nblocks, io, stream, CARVE_EVAL));
  TRY(forward(c, cfg, blocks, nblocks, 0));
  const CDims& d = c.d;
  const unsigned grid = (unsigned)((d.B + 3) / 4);
  hipStream_t st = (hipStream_t)stream;
  const int nz = normalize != 0;
  if (d.dtype == UVC_F32) {
    if (feats_dtype == UVC_F32) k_readout_features<float, float><<<grid, 256, 0, st>>>((const float*)c.w.hc, d.B, d.ntok, d.D, nz, (float*)feats);
    else k_readout_features<float, bf16_t><<<grid, 256, 0, st>>>((const float*)c.w.hc, d.B, d.ntok, d.D, nz, (bf16_t*)feats);
  } else {
    if (feats_dtype == UVC_F32) k_readout_features<bf16_t, float><<<grid, 256, 0, st>>>((const bf16_t*)c.w.hc, d.B, d.ntok, d.D, nz, (float*)feats);
    else k_readout_features<bf16_t, bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)c.w.hc, d.B, d.ntok, d.D, nz, (bf16_t*)feats);
  }
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

extern "C" int64_t uvc_vit_compact_rollout_workspace_bytes(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, int32_t batch) {
  if (check_blocks(cfg, blocks, nblocks)) return -1;
  if (batch <= 0) { uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_rollout_workspace_bytes: batch <= 0"); return -1; }
  Work w;
  return carve(cdims_of(*cfg, blocks, nblocks, batch), blocks, nblocks, CARVE_ROLLOUT, nullptr, w);
}

extern "C" int uvc_vit_compact_rollout(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, const uvc_vit_io* io, float* rollout,
                                       int32_t method, void* stream) {
  if (!rollout) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_rollout: null rollout");
  if (method != 0 && method != 1) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_rollout: method must be 0 (rollout) or 1 (last)");
  Ctx c;
  TRY(setup_eval(c, cfg, blocks, nblocks, io, stream, CARVE_ROLLOUT));
  TRY(forward(c, cfg, blocks, nblocks, 0));
  const CDims& d = c.d;
  // the start vector: uniform over the readout tokens (the eval logits are (x + x_dist) / 2 with the distillation token)
  float* r = c.w.roll[0];
  float* other = c.w.roll[1];
  k_rollout_start<<<(unsigned)((d.M + 255) / 256), 256, 0, (hipStream_t)stream>>>(r, d.M, d.N, d.ntok);
  UVC_CHECK_LAUNCH();
  for (int k = nblocks - 1; k >= 0; --k) {
    if (blocks[k].heads == 0) continue;                       // the branch is a bias: the identity for the row vector
    uvc_attn_rollout_args a;
    memset(&a, 0, sizeof(a));
    a.qkv = c.w.blk[k].qkv; a.lse = c.w.blk[k].lse; a.r_in = r; a.r_out = other;
    a.B = d.B; a.N = d.N; a.H = blocks[k].heads; a.head_dim = 64; a.v_dim = blocks[k].v_dim; a.dtype = d.dtype; a.scale = 0.125f;
    a.keep = method == 0 ? 0.5f : 0.f; a.mix = method == 0 ? 0.5f : 1.0f;
    TRY(uvc_attention_rollout_step(&a, stream));
    float* t = r; r = other; other = t;
    if (method == 1) break;
  }
  const hipError_t e = hipMemcpyAsync(rollout, r, (size_t)d.M * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return e == hipSuccess ? UVC_OK : uvc_set_error(e, __FILE__, __LINE__);
}

extern "C" int uvc_vit_compact_train_forward(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, const uvc_vit_io* io, void* stream) {
  Ctx c;
  TRY(setup_train(c, cfg, blocks, nblocks, io, stream));
  if (!io->x || !io->logits || (cfg->ntok == 2 && !io->logits_dist)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_train_forward: null io member");
  return forward(c, cfg, blocks, nblocks, 1);
}

// The backward walk of uvc_vit_compact_backward and of uvc_vit_compact_attribution: dl / dld are dL/dlogits (/ dL/dlogits_dist).
// G != nullptr (training): every parameter gradient goes to G, the walk runs down to the patch embedding.  G == nullptr (attribution): the
// dgrad chain alone -- no weight-gradient GEMM, no column sum, no zeroed slot, no LayerNorm reduction -- with one uvc_attention_relevance_step
// per block with heads right behind the attn.proj dgrad (*rel: the row vector, which ping-pongs with *rel_other); the walk ends behind the
// step of the lowest block with heads.  d_rows != nullptr (input gradient; G and rel are null): the dgrad chain alone through every block down to
// block 0 -- a bias-only branch passes the stream through unchanged -- then token assembly's backward (its batch sums go to scratch) and the
// patch-embedding dgrad d_rows [B np, K0] (float32) = dpe . W_patch, which reads the workspace's transposed weight copy.  gates != nullptr
// (gate gradients; G, rel and d_rows are null): the dgrad chain alone, with gates [B, sum_k (heads_k + hidden_k)] filled on the way -- one
// plain uvc_gate_dots(o, dO) per block with heads behind its attn.proj dgrad, and per block with units the fc2 dgrad without its epilogue
// into the float32 scratch w.dh, then one fused uvc_gate_dots(u, dh, GELU' -> dA); the walk ends behind the dot of the lowest block that
// has a head or a unit, and a bias-only branch passes the stream through unchanged.
static int backward_walk(Ctx& c, const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int nblocks, const float* dl, const float* dld, float* G,
                         float** rel, float** rel_other, float* d_rows = nullptr, float* gates = nullptr) {
  const uvc_vit_io* io = c.io;
  void* stream = c.st;
  const CDims& d = c.d;
  Work& w = c.w;
  uvc_vit_offsets o; uvc_vit_shadow_offsets so;
  TRY(uvc_vit_compact_train_layout(cfg, blocks, nblocks, &o, &so));
  const float* P = io->params;
  hipStream_t hs = (hipStream_t)stream;
  auto wt = [&](int64_t soff) -> const void* { return (const char*)io->shadow + soff * d.tsz; };      // W^T copies (T; float32 in the exact mode)
  const int gf = d.dtype == UVC_F32 ? 1 : 0;
  const int rh = d.B * d.ntok;
  const Chain ch = chain_of(w, blocks, nblocks);
  auto gp = [&](int64_t off) -> float* { return G ? G + off : nullptr; };      // a gradient slot; nullptr without parameter gradients
  int low = nblocks;                                         // the lowest block with heads: where the attribution walk ends
  for (int k = nblocks - 1; k >= 0; --k) if (blocks[k].heads > 0) low = k;
  int64_t ngates = 0, gcol[UVC_VIT_MAX_DEPTH];                // gate gradients: block k's first column, and the lowest block with a column
  int glow = nblocks;
  for (int k = nblocks - 1; k >= 0; --k) if (blocks[k].heads > 0 || blocks[k].hidden > 0) glow = k;
  for (int k = 0; k < nblocks; ++k) { gcol[k] = ngates; ngates += blocks[k].heads + blocks[k].hidden; }
  if (gates ? glow == nblocks : (!G && !d_rows && low == nblocks)) return UVC_OK;        // no block has heads: the start vector is the answer (no gate: nothing to fill)
  // heads: dhc = dlogits . W, dW = dlogits^T . hc, db = colsum(dlogits)
  TRY(nt(c, dl, 1, wt(so.head_wt), w.dhc, 0, d.B, d.D, d.NC, UVC_EPI_NONE, nullptr, nullptr, nullptr, nullptr, 0, d.ntok * d.D));
  if (G) TRY(tn(c, dl, 1, w.hc, G + o.head_w, G + o.head_b, d.B, d.NC, d.D, 0, d.ntok * d.D));
  if (d.ntok == 2) {
    TRY(nt(c, dld, 1, wt(so.headd_wt), (char*)w.dhc + (size_t)d.D * d.tsz, 0, d.B, d.D, d.NC, UVC_EPI_NONE, nullptr, nullptr, nullptr, nullptr, 0,
            d.ntok * d.D));
    if (G) TRY(tn(c, dld, 1, (const char*)w.hc + (size_t)d.D * d.tsz, G + o.headd_w, G + o.headd_b, d.B, d.NC, d.D, 0, d.ntok * d.D));
  }
  // final norm on the token rows: dL/dx_L is zero on every other row
  int cur = 0, slot = 0;
  {
    const hipError_t he = hipMemsetAsync(w.g[cur], 0, (size_t)d.M * d.D * d.tsz, hs);
    if (he != hipSuccess) return uvc_set_error(he, __FILE__, __LINE__);
  }
  TRY(ln_bwd(c, slot++, w.dhc, ch.xin[nblocks], P + o.norm_w, gp(o.norm_w), gp(o.norm_b), w.meanf, w.rstdf, w.g[cur], nullptr, rh, d.ntok, (int64_t)d.N * d.D));
  for (int k = nblocks - 1; k >= 0; --k) {
    const uvc_compact_block& bk = blocks[k];
    const BlockBufs& b = w.blk[k];
    const int64_t* q = o.blk[k];
    const int nq = qkv_rows(bk), no = attn_cols(bk), F = bk.hidden;
    // MLP branch: g = dL/d(block output)
    if (F > 0) {
      void* g = w.g[cur];
      if (gates) {                                            // dh = g . W2 (float32), then the units' dots and dA = dh * GELU' in one pass over dh
        TRY(nt(c, g, gf, wt(so.blk_wt[k][3]), w.dh, 1, d.M, F, d.D, UVC_EPI_NONE));
        TRY(uvc_gate_dots(b.u, F, w.dh, F, b.gp, F, w.dA, F, d.B, d.N, F, 1, gates, ngates, (int32_t)(gcol[k] + bk.heads), d.dtype, stream));
        if (k == glow && bk.heads == 0) return UVC_OK;        // nothing below it is needed
      } else
        TRY(nt(c, g, gf, wt(so.blk_wt[k][3]), w.dA, 0, d.M, F, d.D, UVC_EPI_MUL_AUX, nullptr, nullptr, b.gp));      // dA = (g . W2) * GELU'
      if (G) TRY(tn(c, g, gf, b.u, G + q[10], G + q[11], d.M, d.D, F));
      TRY(nt(c, w.dA, 0, wt(so.blk_wt[k][2]), w.dH, 0, d.M, d.D, F, UVC_EPI_NONE));
      if (G) TRY(tn(c, w.dA, 0, b.h2, G + q[8], G + q[9], d.M, F, d.D));
      TRY(ln_bwd(c, slot++, w.dH, ch.x1[k], P + q[6], gp(q[6]), gp(q[7]), b.mean2, b.rstd2, w.g[cur ^ 1], g, d.M, 1, d.D));      // dL/dx1
      cur ^= 1;
    } else if (G) {      // the branch is fc2.bias: its gradient is the column sum of the stream, which passes through; norm2 is never read
      TRY(uvc_colsum(w.g[cur], d.M, d.D, d.D, d.dtype, gf, w.cs_partial, G + q[11], 1.0f, nullptr, 0.f, nullptr, stream));
      TRY(zero_f32(c, G + q[6], q[11] - q[6]));
    }
    // attention branch: gB = dL/dx1
    if (bk.heads > 0) {
      void* gB = w.g[cur];
      TRY(nt(c, gB, gf, wt(so.blk_wt[k][1]), w.dO, 0, d.M, no, d.D, UVC_EPI_NONE));
      if (G) TRY(tn(c, gB, gf, b.o, G + q[4], G + q[5], d.M, d.D, no));
      if (gates) {
        TRY(uvc_gate_dots(b.o, no, w.dO, no, nullptr, 0, nullptr, 0, d.B, d.N, no, bk.v_dim, gates, ngates, (int32_t)gcol[k], d.dtype, stream));
        if (k == glow) return UVC_OK;                         // nothing below it is needed
      }
      if (rel) {
        uvc_attn_relevance_args ra;
        memset(&ra, 0, sizeof(ra));
        ra.qkv = b.qkv; ra.lse = b.lse; ra.dout = w.dO; ra.r_in = *rel; ra.r_out = *rel_other;
        ra.B = d.B; ra.N = d.N; ra.H = bk.heads; ra.head_dim = 64; ra.v_dim = bk.v_dim; ra.dtype = d.dtype; ra.scale = 0.125f; ra.keep = 1.0f; ra.mix = 1.0f;
        TRY(uvc_attention_relevance_step(&ra, stream));
        float* t = *rel; *rel = *rel_other; *rel_other = t;
        if (k == low) return UVC_OK;                          // nothing below it is needed
      }
      uvc_attn_args a;
      memset(&a, 0, sizeof(a));
      a.qkv = b.qkv; a.o = b.o; a.lse = b.lse; a.dout = w.dO; a.dqkv = w.dqkv; a.delta = w.delta;
      a.B = d.B; a.N = d.N; a.H = bk.heads; a.head_dim = 64; a.dtype = d.dtype; a.scale = 0.125f; a.v_dim = bk.v_dim;
      TRY(uvc_attention_bwd_vdim(&a, stream));
      TRY(nt(c, w.dqkv, 0, wt(so.blk_wt[k][0]), w.dH, 0, d.M, d.D, nq, UVC_EPI_NONE));
      if (G) TRY(tn(c, w.dqkv, 0, b.h1, G + q[2], G + q[3], d.M, nq, d.D));
      TRY(ln_bwd(c, slot++, w.dH, ch.xin[k], P + q[0], gp(q[0]), gp(q[1]), b.mean1, b.rstd1, w.g[cur ^ 1], gB, d.M, 1, d.D));      // dL/dx_k
      cur ^= 1;
    } else if (G) {
      TRY(uvc_colsum(w.g[cur], d.M, d.D, d.D, d.dtype, gf, w.cs_partial, G + q[5], 1.0f, nullptr, 0.f, nullptr, stream));
      TRY(zero_f32(c, G + q[0], q[5] - q[0]));
    }
  }
  if (d_rows) {
    float* sc = w.asm_scratch;
    TRY(uvc_assemble_tokens_bwd(w.g[cur], w.pe, io->patch_mask, w.dpe, sc, sc + (int64_t)d.N * d.D, d.ntok == 2 ? sc + (int64_t)(d.N + 1) * d.D : nullptr,
                                nullptr, d.B, d.np, d.D, d.ntok, d.dtype, 0, d.dtype == UVC_BF16, 0.f, stream));
    return nt(c, w.dpe, 0, w.wpt, d_rows, 1, d.B * d.np, d.K0, d.D, UVC_EPI_NONE);
  }
  if (!G) return UVC_OK;
  TRY(flush_ln(c));
  // token assembly (the mode-1 token mask is a constant: no d_patch_mask) and the patch-embedding weight gradient
  TRY(uvc_assemble_tokens_bwd(w.g[cur], w.pe, io->patch_mask, w.dpe, G + o.pos_embed, G + o.cls_token, d.ntok == 2 ? G + o.dist_token : nullptr,
                              nullptr, d.B, d.np, d.D, d.ntok, d.dtype, 0, d.dtype == UVC_BF16, 0.f, stream));
  TRY(tn(c, w.dpe, 0, w.patches, G + o.patch_w, G + o.patch_b, d.B * d.np, d.D, d.K0));
  return UVC_OK;
}

extern "C" int uvc_vit_compact_backward(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, const uvc_vit_io* io, void* stream) {
  Ctx c;
  TRY(setup_train(c, cfg, blocks, nblocks, io, stream));
  if (!io->grads || !io->d_logits || (cfg->ntok == 2 && !io->d_logits_dist)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_backward: null io member");
  return backward_walk(c, cfg, blocks, nblocks, io->d_logits, io->d_logits_dist, io->grads, nullptr, nullptr);
}

// ---- class-specific relevance maps (gradient x attention) ------------------------------------------------------------------------------
// One workgroup per image: the target class -- the given one, clamped into [0, nl), or the first maximum of the eval logits (lg, or
// (lg + lgd) / 2 with the distillation token) over [0, nl) -- and the gradient of that eval logit with respect to the head outputs: onehot(t)
// on lg, or onehot(t) / 2 on lg and lgd.
static __global__ __launch_bounds__(256) void k_attrib_target(const float* lg, const float* lgd, const int32_t* target, int nl, int NC, float* dl, float* dld,
                                                              int32_t* tout) {
  __shared__ float sv[256];
  __shared__ int si[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* a = lg + (size_t)b * NC;
  const float* ad = lgd ? lgd + (size_t)b * NC : nullptr;
  int t;
  if (target) {
    t = min(max(target[b], 0), nl - 1);
  } else {
    constexpr int NONE = 0x7fffffff;
    float bv = 0.f; int bi = NONE;
    for (int i = tid; i < nl; i += 256) {                    // ascending indices: a later equal value does not replace an earlier one
      const float v = ad ? (a[i] + ad[i]) * 0.5f : a[i];
      if (bi == NONE || v > bv) { bv = v; bi = i; }
    }
    sv[tid] = bv; si[tid] = bi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) {
        const float v = sv[tid + s]; const int i = si[tid + s];
        if (i != NONE && (si[tid] == NONE || v > sv[tid] || (v == sv[tid] && i < si[tid]))) { sv[tid] = v; si[tid] = i; }
      }
      __syncthreads();
    }
    t = si[0];
  }
  const float one = ad ? 0.5f : 1.0f;
  for (int i = tid; i < NC; i += 256) {
    dl[(size_t)b * NC + i] = i == t ? one : 0.f;
    if (ad) dld[(size_t)b * NC + i] = i == t ? one : 0.f;
  }
  if (tout && tid == 0) tout[b] = t;
}

extern "C" int64_t uvc_vit_compact_attribution_workspace_bytes(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, int32_t batch) {
  if (check_train(cfg, blocks, nblocks)) return -1;
  if (batch <= 0) { uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_attribution_workspace_bytes: batch <= 0"); return -1; }
  Work w;
  return carve(cdims_of(*cfg, blocks, nblocks, batch), blocks, nblocks, CARVE_ATTRIB, nullptr, w);
}

extern "C" int uvc_vit_compact_attribution(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, const uvc_vit_io* io, const int32_t* target,
                                           int32_t num_labels, float* relevance, int32_t* target_out, void* stream) {
  if (!relevance) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_attribution: null relevance");
  Ctx c;
  TRY(setup_train(c, cfg, blocks, nblocks, io, stream, CARVE_ATTRIB));
  if (!io->x || !io->logits || (cfg->ntok == 2 && !io->logits_dist)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_attribution: null io member");
  const CDims& d = c.d;
  if (num_labels < 1 || num_labels > d.NC) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_attribution: num_labels must lie in [1, num_classes]");
  TRY(forward(c, cfg, blocks, nblocks, 1));
  hipStream_t hs = (hipStream_t)stream;
  k_attrib_target<<<(unsigned)d.B, 256, 0, hs>>>(io->logits, d.ntok == 2 ? io->logits_dist : nullptr, target, num_labels, d.NC, c.w.dl[0], c.w.dl[1], target_out);
  UVC_CHECK_LAUNCH();
  // the start vector: uniform over the readout tokens, as in uvc_vit_compact_rollout
  float* r = c.w.roll[0];
  float* other = c.w.roll[1];
  k_rollout_start<<<(unsigned)((d.M + 255) / 256), 256, 0, hs>>>(r, d.M, d.N, d.ntok);
  UVC_CHECK_LAUNCH();
  TRY(backward_walk(c, cfg, blocks, nblocks, c.w.dl[0], c.w.dl[1], nullptr, &r, &other));
  const hipError_t e = hipMemcpyAsync(relevance, r, (size_t)d.M * 4, hipMemcpyDeviceToDevice, hs);
  return e == hipSuccess ? UVC_OK : uvc_set_error(e, __FILE__, __LINE__);
}

// ---- the gradient of a class logit at the input (saliency, gradient x input, integrated gradients) ---------------------------------------
extern "C" int64_t uvc_vit_compact_input_grad_workspace_bytes(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, int32_t batch) {
  if (check_train(cfg, blocks, nblocks)) return -1;
  if (batch <= 0) { uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_input_grad_workspace_bytes: batch <= 0"); return -1; }
  Work w;
  return carve(cdims_of(*cfg, blocks, nblocks, batch), blocks, nblocks, CARVE_INPUT, nullptr, w);
}

extern "C" int uvc_vit_compact_input_grad(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, const uvc_vit_io* io, const int32_t* target,
                                          int32_t num_labels, float* d_rows, int32_t* target_out, void* stream) {
  if (!d_rows) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_input_grad: null d_rows");
  Ctx c;
  TRY(setup_train(c, cfg, blocks, nblocks, io, stream, CARVE_INPUT));
  if ((!io->x && !io->patches_in) || !io->logits || (cfg->ntok == 2 && !io->logits_dist))   // x is read by uvc_patchify alone, as in the eval forward
    return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_input_grad: null io member");
  const CDims& d = c.d;
  if (num_labels < 1 || num_labels > d.NC) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_input_grad: num_labels must lie in [1, num_classes]");
  TRY(forward(c, cfg, blocks, nblocks, 1));
  k_attrib_target<<<(unsigned)d.B, 256, 0, (hipStream_t)stream>>>(io->logits, d.ntok == 2 ? io->logits_dist : nullptr, target, num_labels, d.NC, c.w.dl[0], c.w.dl[1],
                                                                 target_out);
  UVC_CHECK_LAUNCH();
  // W_patch^T in the operand type: the pinned shadow layouts hold no such copy, so it is made per call (K0 D elements beside the pass's GEMMs)
  uvc_vit_offsets o;
  TRY(uvc_vit_compact_layout(cfg, blocks, nblocks, &o, nullptr));
  TRY(uvc_cast_transpose(io->params + o.patch_w, d.D, d.K0, nullptr, c.w.wpt, d.dtype, stream));
  return backward_walk(c, cfg, blocks, nblocks, c.w.dl[0], c.w.dl[1], nullptr, nullptr, nullptr, d_rows);
}

// ---- the gradient of an attack loss at the input (FGSM, PGD) ------------------------------------------------------------------------------
// uvc_vit_compact_input_grad with uvc_loss_seed (robust.hip) in k_attrib_target's place: the same workspace, weight copy and walk.
extern "C" int uvc_vit_compact_loss_grad(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, const uvc_vit_io* io, const int32_t* labels,
                                         int32_t num_labels, int32_t kind, float* d_rows, float* loss_out, void* stream) {
  if (!d_rows || !labels) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_loss_grad: null d_rows or labels");
  Ctx c;
  TRY(setup_train(c, cfg, blocks, nblocks, io, stream, CARVE_INPUT));
  if ((!io->x && !io->patches_in) || !io->logits || (cfg->ntok == 2 && !io->logits_dist))
    return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_loss_grad: null io member");
  const CDims& d = c.d;
  if (num_labels < 1 || num_labels > d.NC) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_loss_grad: num_labels must lie in [1, num_classes]");
  if (kind != 0 && kind != 1) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_loss_grad: kind is 0 (cross-entropy) or 1 (margin)");
  if (kind == 1 && num_labels < 2) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_loss_grad: the margin loss needs num_labels >= 2");
  TRY(forward(c, cfg, blocks, nblocks, 1));
  TRY(uvc_loss_seed(io->logits, d.ntok == 2 ? io->logits_dist : nullptr, labels, d.B, d.NC, num_labels, kind, c.w.dl[0], c.w.dl[1], loss_out, stream));
  uvc_vit_offsets o;
  TRY(uvc_vit_compact_layout(cfg, blocks, nblocks, &o, nullptr));
  TRY(uvc_cast_transpose(io->params + o.patch_w, d.D, d.K0, nullptr, c.w.wpt, d.dtype, stream));
  return backward_walk(c, cfg, blocks, nblocks, c.w.dl[0], c.w.dl[1], nullptr, nullptr, nullptr, d_rows);
}

// ---- Taylor gate scores (python -m uvc_amd.compact_prune) ---------------------------------------------------------------------------------
extern "C" int64_t uvc_vit_compact_gate_grads_workspace_bytes(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, int32_t batch) {
  if (check_train(cfg, blocks, nblocks)) return -1;
  if (batch <= 0) { uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_gate_grads_workspace_bytes: batch <= 0"); return -1; }
  Work w;
  return carve(cdims_of(*cfg, blocks, nblocks, batch), blocks, nblocks, CARVE_GATES, nullptr, w);
}

// uvc_vit_compact_loss_grad's forward and cross-entropy seed, then the dgrad walk with the gate dots on the way (backward_walk, gates)
extern "C" int uvc_vit_compact_gate_grads(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, const uvc_vit_io* io, const int32_t* labels,
                                          int32_t num_labels, float* gates, float* loss_out, void* stream) {
  if (!gates || !labels) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_gate_grads: null gates or labels");
  Ctx c;
  TRY(setup_train(c, cfg, blocks, nblocks, io, stream, CARVE_GATES));
  if (!io->x || !io->logits || (cfg->ntok == 2 && !io->logits_dist)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_gate_grads: null io member");
  const CDims& d = c.d;
  if (num_labels < 1 || num_labels > d.NC) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_gate_grads: num_labels must lie in [1, num_classes]");
  if (d.B > 65535) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_gate_grads: at most 65535 images a call (uvc_gate_dots)");
  TRY(forward(c, cfg, blocks, nblocks, 1));
  TRY(uvc_loss_seed(io->logits, d.ntok == 2 ? io->logits_dist : nullptr, labels, d.B, d.NC, num_labels, 0, c.w.dl[0], c.w.dl[1], loss_out, stream));
  return backward_walk(c, cfg, blocks, nblocks, c.w.dl[0], c.w.dl[1], nullptr, nullptr, nullptr, nullptr, gates);
}
