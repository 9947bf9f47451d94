// Compact-model forward sequencer (include/uvc_vit.h, uvc_vit_compact_*): the eval forward of a pruned DeiT exported at its kept widths
// (uvc_amd/compact.py) -- per block LayerNorm1, qkv GEMM, attention with a value head dim of its own (uvc_attn_args.v_dim), proj GEMM
// (+ bias + residual), LayerNorm2, fc1 (+ bias, GELU), fc2 (+ bias + residual).  Host code only; every arithmetic step is one of the
// kernels behind uvc_kernels.h, the embedding, token assembly, final norm and heads as uvc_vit_forward runs them.
#include "common.h"
#include "../../include/uvc_kernels.h"
#include "../../include/uvc_vit.h"
#include <string.h>

namespace {

#define TRY(x) do { if (int e_ = (x)) return e_; } while (0)

struct CDims {
  int B, S, P, C, D, NC, ntok, np, N, M, K0, dtype, rlow;
  int maxQ, maxO, maxH, maxF;    // widest qkv row, attention output row, head count and hidden width over the blocks
  float eps;
  size_t tsz, rsz;
};

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
  d.B = B; d.S = c.img_size; d.P = c.patch_size; d.C = c.in_chans; d.D = c.embed_dim; d.NC = c.num_classes; d.ntok = c.ntok;
  d.np = (c.img_size / c.patch_size) * (c.img_size / c.patch_size);
  d.N = d.np + d.ntok; d.M = B * d.N; d.K0 = c.in_chans * c.patch_size * c.patch_size; d.dtype = c.dtype;
  d.tsz = c.dtype == UVC_F32 ? 4 : 2;
  d.rlow = (c.dtype == UVC_BF16 && !c.resid_f32) ? 1 : 0;
  d.rsz = d.rlow ? 2 : 4;
  d.eps = c.ln_eps > 0.f ? c.ln_eps : 1e-6f;
  d.maxQ = d.maxO = d.maxH = d.maxF = 0;
  for (int k = 0; k < nblocks; ++k) {
    const uvc_compact_block& b = blocks[k];
    if (b.heads * (128 + b.v_dim) > d.maxQ) d.maxQ = b.heads * (128 + b.v_dim);
    if (b.heads * b.v_dim > d.maxO) d.maxO = b.heads * b.v_dim;
    if (b.heads > d.maxH) d.maxH = b.heads;
    if (b.hidden > d.maxF) d.maxF = b.hidden;
  }
  return d;
}

struct Carver {
  char* base; int64_t off;
  void* take(int64_t bytes) { void* p = base ? base + off : nullptr; off += (bytes + 255) & ~(int64_t)255; return p; }
};

struct CWork {
  void* patches; float* pe; void* r[3];      // r: residual-stream rows [M, D]; a block's input, x1 and output take whichever are free
  void* h; void* qkv; void* o; float* lse; void* u; float* mean; float* rstd; float* ones;
  void* hc; float* meanf; float* rstdf;
};

int64_t carve(const CDims& d, char* base, CWork& w) {
  Carver c{base, 0};
  const int64_t M = d.M;
  w.patches = c.take((int64_t)d.B * d.np * d.K0 * d.tsz);
  w.pe = (float*)c.take((int64_t)d.B * d.np * d.D * 4);
  for (int i = 0; i < 3; ++i) w.r[i] = c.take(M * d.D * d.rsz);
  w.h = c.take(M * d.D * d.tsz);
  w.qkv = c.take(M * d.maxQ * d.tsz);
  w.o = c.take(M * d.maxO * d.tsz);
  w.lse = (float*)c.take((int64_t)d.B * d.maxH * d.N * 4);
  w.u = c.take(M * d.maxF * d.tsz);
  w.mean = (float*)c.take(M * 4); w.rstd = (float*)c.take(M * 4);
  w.ones = (float*)c.take(M * 4);
  w.hc = c.take((int64_t)d.B * d.ntok * d.D * d.tsz);
  w.meanf = (float*)c.take((int64_t)d.B * d.ntok * 4); w.rstdf = (float*)c.take((int64_t)d.B * d.ntok * 4);
  return c.off;
}

struct CCtx { CDims d; const uvc_vit_io* io; void* st; };

// C[M,N] = epi(A[M,K] . B[N,K]^T); bf16 mode reads the shadow's [out, in] copy, float32 mode the master weights
int nt(const CCtx& c, const void* A, const void* B, void* C, int c_f32, int M, int N, int K, int epi, const float* bias, const void* R = nullptr,
       int lda = 0) {
  uvc_gemm_nt_args a;
  memset(&a, 0, sizeof(a));
  a.A = A; a.B = B; a.C = C; a.bias = bias; a.R = R;
  a.alpha = 1.0f; a.M = M; a.N = N; a.K = K; a.lda = lda ? lda : K; a.ldb = K; a.ldc = N; a.ldr = N; a.ldaux = N;
  a.dtype = c.d.dtype; a.a_is_f32 = c.d.dtype == UVC_F32; a.c_is_f32 = c_f32 || c.d.dtype == UVC_F32; a.epilogue = epi;
  a.r_is_f32 = a.c_is_f32;
  return uvc_gemm_nt(&a, c.st);
}
int ln_fwd(const CCtx& c, const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int rows, int rpg, int64_t gs) {
  uvc_ln_args a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.x_lowp = c.d.rlow; a.gamma = gamma; a.beta = beta; a.y = y; a.mean = mean; a.rstd = rstd; a.eps = c.d.eps;
  a.rows = rows; a.D = c.d.D; a.rows_per_group = rpg; a.group_stride = gs; a.dtype = c.d.dtype;
  return uvc_layernorm_fwd(&a, c.st);
}

}  // namespace

extern "C" int uvc_vit_compact_layout(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, uvc_vit_offsets* off,
                                      uvc_vit_shadow_offsets* soff) {
  TRY(check_blocks(cfg, blocks, nblocks));
  const CDims d = cdims_of(*cfg, blocks, nblocks, 1);
  if (off) {
    memset(off, 0xff, sizeof(*off));
    int64_t o = 0;
    auto put = [&](int64_t& slot, int64_t n) { slot = o; o += (n + 3) & ~(int64_t)3; };
    put(off->cls_token, d.D);
    if (d.ntok == 2) put(off->dist_token, d.D);
    put(off->pos_embed, (int64_t)d.N * d.D);
    put(off->patch_w, (int64_t)d.D * d.K0); put(off->patch_b, d.D);
    for (int k = 0; k < nblocks; ++k) {
      int64_t* b = off->blk[k];
      const int64_t nq = (int64_t)blocks[k].heads * (128 + blocks[k].v_dim), no = (int64_t)blocks[k].heads * blocks[k].v_dim, F = blocks[k].hidden;
      put(b[0], d.D); put(b[1], d.D); put(b[2], nq * d.D); put(b[3], nq); put(b[4], d.D * no); put(b[5], d.D);
      put(b[6], d.D); put(b[7], d.D); put(b[8], F * d.D); put(b[9], F); put(b[10], d.D * F); put(b[11], d.D);
    }
    put(off->norm_w, d.D); put(off->norm_b, d.D);
    put(off->head_w, (int64_t)d.NC * d.D); put(off->head_b, d.NC);
    if (d.ntok == 2) { put(off->headd_w, (int64_t)d.NC * d.D); put(off->headd_b, d.NC); }
    off->n_main = o;
    put(off->patch_gating, d.np);
    off->n_total = o;
  }
  if (soff) {
    memset(soff, 0xff, sizeof(*soff));
    int64_t o = 0;
    auto put = [&](int64_t& slot, int64_t n) { slot = o; o += (n + 7) & ~(int64_t)7; };
    put(soff->patch_w, (int64_t)d.D * d.K0);
    for (int k = 0; k < nblocks; ++k) {
      const int64_t nq = (int64_t)blocks[k].heads * (128 + blocks[k].v_dim), no = (int64_t)blocks[k].heads * blocks[k].v_dim, F = blocks[k].hidden;
      put(soff->blk_w[k][0], nq * d.D); put(soff->blk_w[k][1], d.D * no); put(soff->blk_w[k][2], F * d.D); put(soff->blk_w[k][3], d.D * F);
    }
    put(soff->head_w, (int64_t)d.NC * d.D);
    if (d.ntok == 2) put(soff->headd_w, (int64_t)d.NC * d.D);
    soff->n_total = o;
  }
  return UVC_OK;
}

extern "C" int64_t uvc_vit_compact_workspace_bytes(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, int32_t batch) {
  if (check_blocks(cfg, blocks, nblocks) || batch <= 0) return -1;
  CWork w;
  return carve(cdims_of(*cfg, blocks, nblocks, batch), nullptr, w);
}

extern "C" int uvc_vit_compact_update_shadows(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, const float* params, void* shadow,
                                              void* stream) {
  TRY(check_blocks(cfg, blocks, nblocks));
  if (cfg->dtype == UVC_F32) return UVC_OK;                 // the GEMMs read the float32 master weights
  if (!params || !shadow) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_update_shadows: null pointer");
  const CDims d = cdims_of(*cfg, blocks, nblocks, 1);
  uvc_vit_offsets off; uvc_vit_shadow_offsets so;
  TRY(uvc_vit_compact_layout(cfg, blocks, nblocks, &off, &so));
  int64_t srcs[64], ws[64], wts[64];
  int32_t Rs[64], Cs[64];
  int n = 0;
  auto flush = [&]() -> int {
    if (n == 0) return UVC_OK;
    const int e = uvc_cast_transpose_multi(params, shadow, n, srcs, Rs, Cs, ws, wts, d.dtype, stream);
    n = 0;
    return e;
  };
  auto one = [&](int64_t p, int R, int C, int64_t sw) -> int {
    if (R == 0 || C == 0) return UVC_OK;                   // (a block without heads / units has no such matrix)
    srcs[n] = p; Rs[n] = R; Cs[n] = C; ws[n] = sw; wts[n] = -1; ++n;
    return n == 64 ? flush() : UVC_OK;
  };
  TRY(one(off.patch_w, d.D, d.K0, so.patch_w));
  for (int k = 0; k < nblocks; ++k) {
    const int nq = blocks[k].heads * (128 + blocks[k].v_dim), no = blocks[k].heads * blocks[k].v_dim, F = blocks[k].hidden;
    TRY(one(off.blk[k][2], nq, d.D, so.blk_w[k][0])); TRY(one(off.blk[k][4], d.D, no, so.blk_w[k][1]));
    TRY(one(off.blk[k][8], F, d.D, so.blk_w[k][2])); TRY(one(off.blk[k][10], d.D, F, so.blk_w[k][3]));
  }
  TRY(one(off.head_w, d.NC, d.D, so.head_w));
  if (d.ntok == 2) TRY(one(off.headd_w, d.NC, d.D, so.headd_w));
  return flush();
}

extern "C" int uvc_vit_compact_forward(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, const uvc_vit_io* io, void* stream) {
  TRY(check_blocks(cfg, blocks, nblocks));
  if (!io || !io->params || !io->workspace || io->batch <= 0 || !io->x || !io->logits || (cfg->ntok == 2 && !io->logits_dist))
    return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_forward: null io member");
  if (cfg->dtype == UVC_BF16 && !io->shadow) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_forward: bf16 mode needs the shadow buffer");
  CCtx c;
  c.d = cdims_of(*cfg, blocks, nblocks, io->batch); c.io = io; c.st = stream;
  const CDims& d = c.d;
  CWork w;
  if (io->workspace_bytes < carve(d, nullptr, w)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_vit_compact_forward: workspace too small");
  carve(d, (char*)io->workspace, w);
  if (io->patches_in) w.patches = const_cast<void*>(io->patches_in);
  uvc_vit_offsets o; uvc_vit_shadow_offsets so;
  TRY(uvc_vit_compact_layout(cfg, blocks, nblocks, &o, &so));
  const float* P = io->params;
  auto wm = [&](int64_t poff, int64_t soff) -> const void* { return d.dtype == UVC_F32 ? (const void*)(P + poff) : (const void*)((const char*)io->shadow + soff * d.tsz); };
  const int rf = d.rlow ? 0 : 1;                           // "C is float32" of the GEMMs that write residual-stream rows
  // patch embedding (PatchEmbed.forward :145-153) and token assembly with the mode-1 token mask (:434-471)
  if (!io->patches_in) TRY(uvc_patchify(io->x, w.patches, d.B, d.C, d.S, d.P, d.dtype, stream));
  TRY(nt(c, w.patches, wm(o.patch_w, so.patch_w), w.pe, 1, d.B * d.np, d.D, d.K0, UVC_EPI_BIAS, P + o.patch_b));
  void* xin = w.r[0];
  TRY(uvc_assemble_tokens(w.pe, P + o.cls_token, d.ntok == 2 ? P + o.dist_token : nullptr, P + o.pos_embed, io->patch_mask, xin, d.B, d.np,
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
  auto free_buf = [&](const void* a, const void* b) -> void* {
    for (int i = 0; i < 3; ++i) if (w.r[i] != a && w.r[i] != b) return w.r[i];
    return nullptr;
  };
  for (int k = 0; k < nblocks; ++k) {
    const uvc_compact_block& bk = blocks[k];
    const int64_t* q = o.blk[k];
    const int nq = bk.heads * (128 + bk.v_dim), no = bk.heads * bk.v_dim;
    void* x1 = xin;
    if (bk.heads > 0) {
      TRY(ln_fwd(c, xin, P + q[0], P + q[1], w.h, w.mean, w.rstd, d.M, 1, d.D));
      TRY(nt(c, w.h, wm(q[2], so.blk_w[k][0]), w.qkv, 0, d.M, nq, d.D, UVC_EPI_BIAS, P + q[3]));
      uvc_attn_args a;
      memset(&a, 0, sizeof(a));
      a.qkv = w.qkv; a.o = w.o; a.lse = w.lse; a.B = d.B; a.N = d.N; a.H = bk.heads; a.head_dim = 64; a.dtype = d.dtype; a.scale = 0.125f;
      a.v_dim = bk.v_dim;
      TRY(uvc_attention_fwd(&a, stream));
      x1 = free_buf(xin, nullptr);
      TRY(nt(c, w.o, wm(q[4], so.blk_w[k][1]), x1, rf, d.M, d.D, no, UVC_EPI_BIAS_RESID, P + q[5], xin));
    } else {
      TRY(add_bias(x1, P + q[5]));
    }
    void* xout = x1;
    if (bk.hidden > 0) {
      TRY(ln_fwd(c, x1, P + q[6], P + q[7], w.h, w.mean, w.rstd, d.M, 1, d.D));
      TRY(nt(c, w.h, wm(q[8], so.blk_w[k][2]), w.u, 0, d.M, bk.hidden, d.D, UVC_EPI_BIAS_GELU_OUT, P + q[9]));
      xout = free_buf(x1, nullptr);
      TRY(nt(c, w.u, wm(q[10], so.blk_w[k][3]), xout, rf, d.M, d.D, bk.hidden, UVC_EPI_BIAS_RESID, P + q[11], x1));
    } else {
      TRY(add_bias(xout, P + q[11]));
    }
    xin = xout;
  }
  // final norm on the class (/ distillation) token rows (:507-508), then the head(s) (:522-526)
  TRY(ln_fwd(c, xin, P + o.norm_w, P + o.norm_b, w.hc, w.meanf, w.rstdf, d.B * d.ntok, d.ntok, (int64_t)d.N * d.D));
  TRY(nt(c, w.hc, wm(o.head_w, so.head_w), io->logits, 1, d.B, d.NC, d.D, UVC_EPI_BIAS, P + o.head_b, nullptr, d.ntok * d.D));
  if (d.ntok == 2)
    TRY(nt(c, (const char*)w.hc + (size_t)d.D * d.tsz, wm(o.headd_w, so.headd_w), io->logits_dist, 1, d.B, d.NC, d.D, UVC_EPI_BIAS, P + o.headd_b,
           nullptr, d.ntok * d.D));
  return UVC_OK;
}
