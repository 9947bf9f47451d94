// Host-side plumbing shared by the two sequencers (vit_engine.hip, compact_engine.hip): model dimensions, workspace carving, the head
// and tail of the flat parameter layout and the batching of shadow-weight refreshes.  Plain C++, no kernels.
#pragma once
#include "common.h"
#include "../../include/uvc_kernels.h"
#include "../../include/uvc_vit.h"
#include <string.h>

namespace {

#define TRY(x) do { if (int e_ = (x)) return e_; } while (0)

struct Dims {
  int B, S, P, C, D, L, H, F, NC, ntok, np, N, M, K0, dtype, qkv_bias;
  int rlow;              // the residual stream (x_l, x1 of every block, the final rows) is bf16: the throughput mode unless uvc_vit_cfg.resid_f32
  float eps;
  size_t tsz, rsz;       // bytes per operand element (T); per residual-stream element
};
Dims dims_of(const uvc_vit_cfg& c, int B) {
  Dims d;
  d.B = B; d.S = c.img_size; d.P = c.patch_size; d.C = c.in_chans; d.D = c.embed_dim; d.L = c.depth; d.H = c.num_heads;
  d.F = c.hidden; d.NC = c.num_classes; d.ntok = c.ntok; d.np = (c.img_size / c.patch_size) * (c.img_size / c.patch_size);
  d.N = d.np + d.ntok; d.M = B * d.N; d.K0 = c.in_chans * c.patch_size * c.patch_size; d.dtype = c.dtype;
  d.tsz = c.dtype == UVC_F32 ? 4 : 2;
  d.rlow = (c.dtype == UVC_BF16 && !c.resid_f32) ? 1 : 0;
  d.rsz = d.rlow ? 2 : 4;
  d.eps = c.ln_eps > 0.f ? c.ln_eps : 1e-6f;
  d.qkv_bias = c.no_qkv_bias ? 0 : 1;
  return d;
}

// ---- workspace carving ---------------------------------------------------------------------------
struct Carver {
  char* base; int64_t off;
  void* take(int64_t bytes) { void* p = base ? base + off : nullptr; off += (bytes + 255) & ~(int64_t)255; return p; }
};

// ---- parameter layout ----------------------------------------------------------------------------
// hands out consecutive slots of a flat buffer, each starting on a multiple of `align` elements (4: float32 parameters, 8: shadow copies)
struct Slots {
  int64_t o, align;
  void operator()(int64_t& slot, int64_t n) { slot = o; o += (n + align - 1) & ~(align - 1); }
};
// what precedes the blocks in the parameter buffer, and what follows them up to n_main
void layout_embed(const Dims& d, uvc_vit_offsets* off, Slots& put) {
  put(off->cls_token, d.D);
  if (d.ntok == 2) put(off->dist_token, d.D);
  put(off->pos_embed, (int64_t)d.N * d.D);
  put(off->patch_w, (int64_t)d.D * d.K0); put(off->patch_b, d.D);
}
void layout_heads(const Dims& d, uvc_vit_offsets* off, Slots& put) {
  put(off->norm_w, d.D); put(off->norm_b, d.D);
  put(off->head_w, (int64_t)d.NC * d.D); put(off->head_b, d.NC);
  if (d.ntok == 2) { put(off->headd_w, (int64_t)d.NC * d.D); put(off->headd_b, d.NC); }
  off->n_main = put.o;
}

// ---- shadow refresh ------------------------------------------------------------------------------
// collects (parameter offset, R, C, shadow offset of the [R, C] copy, of the transposed copy; -1: no such copy) and casts them 64 matrices
// at a launch (uvc_cast_transpose_multi).  A matrix without rows or columns, or with neither copy asked for, is skipped.
struct ShadowBatch {
  const float* params; void* shadow; int dtype; void* stream;
  int64_t srcs[64], ws[64], wts[64];
  int32_t Rs[64], Cs[64];
  int n;
  int flush() {
    if (n == 0) return UVC_OK;
    const int e = uvc_cast_transpose_multi(params, shadow, n, srcs, Rs, Cs, ws, wts, dtype, stream);
    n = 0;
    return e;
  }
  int add(int64_t src, int64_t R, int64_t C, int64_t w, int64_t wt) {
    if (R == 0 || C == 0 || (w < 0 && wt < 0)) return UVC_OK;
    srcs[n] = src; Rs[n] = (int32_t)R; Cs[n] = (int32_t)C; ws[n] = w; wts[n] = wt; ++n;
    return n == 64 ? flush() : UVC_OK;
  }
};

}  // namespace
