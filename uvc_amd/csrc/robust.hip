// Adversarial robustness of compact models (python -m uvc_amd.compact_robust) for gfx950: the attack loss with its gradient at the head
// outputs, and the projected signed step of FGSM / PGD on patch rows.  uvc_loss_seed is one workgroup per image with fixed reduction trees
// (a wave butterfly, then the four waves in order: uvc_logits_topk's); uvc_pgd_step is bandwidth-bound, every element read once, 16-byte
// accesses where the row width and every pointer allow them and element by element otherwise, offsets in size_t.  No atomics, one writer per
// output element: the same bits on a repeat and in any batch.
#include "common.h"
#include "../../include/uvc_kernels.h"

namespace {

// ---------------------------------------------------------------------------- the attack loss and its seed (uvc_loss_seed)
constexpr int NONE = 0x7fffffff;

// The eval logit of column c as an unevaluated sum hi + lo, exact: a, or (a + ad) / 2 through TwoSum (halving is exact).  What the float64
// statement of the loss sees is this pair, not the once-rounded float32 mean.
__device__ __forceinline__ void eval_logit(const float* a, const float* ad, int c, float& hi, float& lo) {
  if (!ad) { hi = a[c]; lo = 0.f; return; }
  const float x = a[c], y = ad[c];
  const float s = x + y;
  const float bb = s - x;
  const float e = (x - (s - bb)) + (y - bb);
  hi = s * 0.5f; lo = e * 0.5f;
}
// d = a - b as hi + lo exactly (TwoSum on a + (-b)), as probe.hip takes a logit's distance from the row maximum
__device__ __forceinline__ void two_diff(float a, float b, float& hi, float& lo) {
  hi = a - b;
  const float bb = hi - a;
  lo = (a - (hi - bb)) - (b + bb);
}
// exp(hi + t) from e = exp(hi) and the small remainder t, to second order: at logits of magnitude 3e4 the remainder of a two-head mean
// reaches 1e-3, and t^2 / 2 would be four float32 spacings of the result
__device__ __forceinline__ float exp_two(float e, float t) { return __builtin_fmaf(e, __builtin_fmaf(0.5f * t, t, t), e); }
// s + c += x + xc with the rounding error of the addition kept in c: the same result whichever operand comes first, so both lanes of a
// butterfly step agree
__device__ __forceinline__ void add_two(float& s, float& c, float x, float xc) {
  const float t = s + x;
  const float bb = t - s;
  c = (c + xc) + ((s - (t - bb)) + (x - bb));
  s = t;
}
// "a before b" among the columns: the larger exact value first (hi, then lo: the pairs are normalised), equal values by ascending index
__device__ __forceinline__ bool col_before(float ah, float al, int ai, float bh, float bl, int bi) {
  if (ai == NONE) return false;
  if (bi == NONE) return true;
  return ah > bh || (ah == bh && (al > bl || (al == bl && ai < bi)));
}

__device__ __forceinline__ float block_max(float v, float* sh) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

// kind 0: L = lse(z) - z_y, dz = softmax(z) - onehot(y).  kind 1: L = z_j - z_y, dz = onehot(j) - onehot(y), j the first maximum over c != y.
__global__ __launch_bounds__(256) void k_loss_seed(const float* __restrict__ lg, const float* __restrict__ lgd, const int32_t* __restrict__ labels,
                                                   int n, int ld, int kind, float* __restrict__ dl, float* __restrict__ dld,
                                                   float* __restrict__ loss) {
  __shared__ float sh[4], sc[4], sl[4];
  __shared__ int si[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* a = lg + (size_t)b * ld;
  const float* ad = lgd ? lgd + (size_t)b * ld : nullptr;
  float* o = dl + (size_t)b * ld;
  float* od = lgd ? dld + (size_t)b * ld : nullptr;
  const int y = min(max(labels[b], 0), n - 1);
  const float half = ad ? 0.5f : 1.0f;
  float yh, yl;
  eval_logit(a, ad, y, yh, yl);
  if (kind == 1) {
    float bh = 0.f, bl = 0.f; int bi = NONE;
    for (int c = tid; c < n; c += 256) {
      if (c == y) continue;
      float h, l;
      eval_logit(a, ad, c, h, l);
      if (col_before(h, l, c, bh, bl, bi)) { bh = h; bl = l; bi = c; }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
      const float oh = __shfl_xor(bh, s, 64), ol = __shfl_xor(bl, s, 64);
      const int oi = __shfl_xor(bi, s, 64);
      if (col_before(oh, ol, oi, bh, bl, bi)) { bh = oh; bl = ol; bi = oi; }
    }
    if ((tid & 63) == 0) { sh[tid >> 6] = bh; sl[tid >> 6] = bl; si[tid >> 6] = bi; }
    __syncthreads();
    bh = sh[0]; bl = sl[0]; bi = si[0];
    for (int w = 1; w < 4; ++w)
      if (col_before(sh[w], sl[w], si[w], bh, bl, bi)) { bh = sh[w]; bl = sl[w]; bi = si[w]; }
    for (int c = tid; c < ld; c += 256) {
      const float v = c == bi ? half : (c == y ? -half : 0.f);
      o[c] = v;
      if (od) od[c] = v;
    }
    if (loss && tid == 0) loss[b] = (bh - yh) + (bl - yl);
    return;
  }
  float mx = -INFINITY;
  for (int c = tid; c < n; c += 256) {
    float h, l;
    eval_logit(a, ad, c, h, l);
    mx = fmaxf(mx, h);
  }
  mx = block_max(mx, sh);
  // the sum of the exponentials, every addition compensated: it carries one rounding, not one per level of the tree
  float sum = 0.f, comp = 0.f;
  for (int c = tid; c < n; c += 256) {
    float h, l, dh, dlo;
    eval_logit(a, ad, c, h, l);
    two_diff(h, mx, dh, dlo);
    const float e = expf(dh);
    add_two(sum, comp, exp_two(e, dlo + l), 0.f);
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) add_two(sum, comp, __shfl_xor(sum, s, 64), __shfl_xor(comp, s, 64));
  __syncthreads();
  if ((tid & 63) == 0) { sh[tid >> 6] = sum; sc[tid >> 6] = comp; }
  __syncthreads();
  sum = sh[0]; comp = sc[0];
  for (int w = 1; w < 4; ++w) add_two(sum, comp, sh[w], sc[w]);
  const float se = sum + comp;
  for (int c = tid; c < ld; c += 256) {
    float v = 0.f;
    if (c < n) {
      float h, l, dh, dlo;
      eval_logit(a, ad, c, h, l);
      two_diff(h, mx, dh, dlo);
      const float e = expf(dh);
      v = __fdiv_rn(exp_two(e, dlo + l), se);
      if (c == y) v -= 1.0f;                                 // exact from one half up, rounded once below it
      v *= half;
    }
    o[c] = v;
    if (od) od[c] = v;
  }
  if (loss && tid == 0) {
    float dh, dlo;
    two_diff(yh, mx, dh, dlo);
    loss[b] = (logf(se) - dh) - (dlo + yl);
  }
}

// ---------------------------------------------------------------------------- the projected step (uvc_pgd_step)
struct StepArgs {
  const float* x; const float* x0; const float* dir; float* out; void* out_t;
  size_t items; uint32_t per_row, per_chan;                  // items of W elements in all, in a row and in a channel of a row
  int mode, C;
  float step[4], eps[4], lo[4], hi[4];
};

// torch.maximum / torch.minimum: a NaN operand is the result
__device__ __forceinline__ float t_max(float a, float b) { return a != a ? a : (b != b ? b : (a < b ? b : a)); }
__device__ __forceinline__ float t_min(float a, float b) { return a != a ? a : (b != b ? b : (b < a ? b : a)); }

template <typename T, int W> struct RowStore;
template <> struct RowStore<float, 1> { static __device__ __forceinline__ void put(float* p, const float* v) { *p = v[0]; } };
template <> struct RowStore<float, 4> {
  static __device__ __forceinline__ void put(float* p, const float* v) { *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]}; }
};
template <> struct RowStore<bf16_t, 1> { static __device__ __forceinline__ void put(bf16_t* p, const float* v) { *p = f32_to_bf16(v[0]); } };
template <> struct RowStore<bf16_t, 4> {
  static __device__ __forceinline__ void put(bf16_t* p, const float* v) {
    u32x2 q; q[0] = pack_bf16x2(v[0], v[1]); q[1] = pack_bf16x2(v[2], v[3]);
    *reinterpret_cast<u32x2*>(p) = q;
  }
};
template <> struct RowStore<bf16_t, 8> {
  static __device__ __forceinline__ void put(bf16_t* p, const float* v) {
    u32x4 q;
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = pack_bf16x2(v[2 * i], v[2 * i + 1]);
    *reinterpret_cast<u32x4*>(p) = q;
  }
};
template <int W> __device__ __forceinline__ void load_f32(const float* p, float* v) {
  if constexpr (W == 1) {
    v[0] = *p;
  } else {
#pragma unroll
    for (int q = 0; q < W / 4; ++q) {
      const f32x4 r = reinterpret_cast<const f32x4*>(p)[q];
      v[4 * q] = r[0]; v[4 * q + 1] = r[1]; v[4 * q + 2] = r[2]; v[4 * q + 3] = r[3];
    }
  }
}

// Lane i takes item i: W consecutive elements of one row and one channel.  x and out may be the same buffer (an element is read, then
// written, by one lane), so neither is __restrict__.  Every operation is one float32 operation rounded once: the file is built with
// -ffp-contract=off (uvc_amd/build.py), so x + step * d stays a product and a sum.
template <typename T, int W>
__global__ __launch_bounds__(256) void k_pgd_step(StepArgs a) {
  const bool narrow = a.items <= 0xffffffffull;              // (uniform) a 32-bit remainder where the index allows it
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < a.items; i += (size_t)gridDim.x * 256) {
    const uint32_t k = narrow ? (uint32_t)i % a.per_row : (uint32_t)(i % a.per_row);
    const int c = min((int)(k / a.per_chan), a.C - 1);
    const float st = a.step[c], ep = a.eps[c], lo = a.lo[c], hi = a.hi[c];
    float x[W], x0[W], d[W], v[W];
    load_f32<W>(a.x + i * W, x);
    load_f32<W>(a.x0 + i * W, x0);
    load_f32<W>(a.dir + i * W, d);
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const float s = a.mode == 0 ? (float)(d[e] > 0.f) - (float)(d[e] < 0.f) : d[e];
      const float moved = x[e] + st * s;
      const float low = t_max(x0[e] - ep, lo), high = t_min(x0[e] + ep, hi);
      v[e] = t_min(t_max(moved, low), high);
    }
    if constexpr (W == 8) { RowStore<float, 4>::put(a.out + i * W, v); RowStore<float, 4>::put(a.out + i * W + 4, v + 4); }
    else RowStore<float, W>::put(a.out + i * W, v);
    if (a.out_t) RowStore<T, W>::put((T*)a.out_t + i * W, v);
  }
}

inline unsigned grid_for(size_t n) { const size_t g = (n + 255) / 256; return (unsigned)(g > 8192 ? 8192 : (g < 1 ? 1 : g)); }   // a capped grid, the rest by stride

}  // namespace

extern "C" int uvc_loss_seed(const float* lg, const float* lgd, const int32_t* labels, int32_t B, int32_t ld, int32_t n_valid, int32_t kind,
                             float* dl, float* dld, float* loss, void* stream) {
  if (!lg || !labels || !dl || (lgd && !dld)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_loss_seed: null pointer");
  if (B <= 0) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_loss_seed: B <= 0");
  if (n_valid < 1 || n_valid > ld) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_loss_seed: need 1 <= n_valid <= ld");
  if (kind != 0 && kind != 1) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_loss_seed: kind is 0 (cross-entropy) or 1 (margin)");
  if (kind == 1 && n_valid < 2) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_loss_seed: the margin loss needs n_valid >= 2");
  k_loss_seed<<<(unsigned)B, 256, 0, (hipStream_t)stream>>>(lg, lgd, labels, n_valid, ld, kind, dl, dld, loss);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

extern "C" int uvc_pgd_step(const float* x, const float* x0, const float* dir, int64_t rows, int32_t P, int32_t C, const float* step,
                            const float* eps, const float* lo, const float* hi, int32_t mode, float* out, void* out_t, int32_t dtype,
                            void* stream) {
  if (!x || !x0 || !dir || !out || !step || !eps || !lo || !hi) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_pgd_step: null pointer");
  if (rows <= 0 || P < 1 || P > 1024) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_pgd_step: rows must be positive and P in [1, 1024]");
  if (C < 1 || C > 4) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_pgd_step: 1 <= C <= 4 channels");
  if (mode != 0 && mode != 1) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_pgd_step: mode is 0 (signed step) or 1 (dir as it is)");
  if (dtype != UVC_F32 && dtype != UVC_BF16) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_pgd_step: bad dtype");
  StepArgs a;
  for (int c = 0; c < 4; ++c) {
    const int s = c < C ? c : C - 1;
    if (!(eps[s] >= 0.f) || !(lo[s] <= hi[s]) || step[s] != step[s])
      return uvc_set_error_msg(UVC_ERR_ARG, "uvc_pgd_step: need eps >= 0, lo <= hi and a step that is a number, every channel");
    a.step[c] = step[s]; a.eps[c] = eps[s]; a.lo[c] = lo[s]; a.hi[c] = hi[s];
  }
  const size_t PP = (size_t)P * P, K0 = PP * C, total = (size_t)rows * K0;
  const uintptr_t f32_ptrs = (uintptr_t)x | (uintptr_t)x0 | (uintptr_t)dir | (uintptr_t)out;
  // W elements a lane: all of one channel (PP % W == 0) and, with the pointers on 16 bytes, every access on its own size
  int W = 1;
  if ((f32_ptrs & 15) == 0 && PP % 4 == 0) {
    if (dtype == UVC_F32) W = ((uintptr_t)out_t & 15) == 0 ? 4 : 1;
    else if (PP % 8 == 0 && ((uintptr_t)out_t & 15) == 0) W = 8;
    else if (((uintptr_t)out_t & 7) == 0) W = 4;
  }
  a.x = x; a.x0 = x0; a.dir = dir; a.out = out; a.out_t = out_t;
  a.items = total / W; a.per_row = (uint32_t)(K0 / W); a.per_chan = (uint32_t)(PP / W);
  a.mode = mode; a.C = C;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = grid_for(a.items);
  if (dtype == UVC_F32) {
    if (W == 4) k_pgd_step<float, 4><<<grid, 256, 0, st>>>(a);
    else k_pgd_step<float, 1><<<grid, 256, 0, st>>>(a);
  } else {
    if (W == 8) k_pgd_step<bf16_t, 8><<<grid, 256, 0, st>>>(a);
    else if (W == 4) k_pgd_step<bf16_t, 4><<<grid, 256, 0, st>>>(a);
    else k_pgd_step<bf16_t, 1><<<grid, 256, 0, st>>>(a);
  }
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}
