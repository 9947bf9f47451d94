// Linear probe on a feature bank (python -m uvc_amd.compact_probe) for gfx950: uvc_probe_eval, the L2-regularised multinomial logistic
// objective and its gradient over the whole bank, and uvc_softmax_xent_grad, its row kernel (include/uvc_kernels.h).
//
// uvc_probe_eval runs, on one stream:  k_probe_count (m = the rows whose label lies in [0, C), one workgroup, integer sums), k_probe_prep (W rounded
// to the operand type once; dW = l2 W and db = 0, padding rows exactly 0; per-workgroup partials of |W|^2), then per chunk of rows
// logits = X_c W^T + b (uvc_gemm_nt, float32 out), the row kernel, dW += (1 / m) G_c^T X_c with db += (1 / m) colsum G_c (uvc_gemm_tn, beta = 1, the
// device scalar 1 / m as alpha_ptr), and k_probe_finish (one workgroup: loss, hit and |W|^2 partials in ascending order in float64).
// No atomics, one writer per element in every launch, the same bits on a repeat with the same chunk_rows.
//
// The row kernel is bandwidth-bound: 4 bytes in and 2 or 4 out per logit.  A row of ld floats is held in registers by a group of LPR lanes
// (1 .. 64, a power of two: a wave takes 64 / LPR rows at once), 8 consecutive floats per lane and unit: two 16-byte loads, one (bf16) or two
// (float32) 16-byte stores; above 2048 columns one workgroup takes the row in three passes (the second and third from L2).  A lane sums its
// own columns in ascending order, the group then runs the xor butterfly, so a row's result is a function of the row alone -- not of the rows
// beside it, the row count or the chunk.  The sum leaves out the first maximum's own term, exactly 1, and adds it last (the loss is log1p of the
// rest: a confident row's small loss keeps its relative accuracy).  z - max is taken as an exact two-term sum (d_hi + d_lo, Knuth's TwoSum), exp(d_hi) (1 + d_lo):
// the rounding of the subtraction, up to 2^-24 |d| in the exponent, would otherwise be 88 x 2^-24 relative in the smallest probabilities.
#include <type_traits>
#include "common.h"
#include "../../include/uvc_kernels.h"

namespace {

constexpr int PROBE_MAX_D = 1024;
constexpr int PROBE_MAX_C = 65536;
constexpr int ROW_THREADS = 256;
constexpr int WAVE_ROW_MAX_LD = 2048;       // wider rows: one workgroup per row
constexpr int PREP_THREADS = 256;
constexpr int PREP_MAX_BLOCKS = 1024;
constexpr int FIN_THREADS = 1024;

struct RowArgs {
  const float* logits; const void* labels; void* G; float* loss_part; int32_t* hit_part;
  int64_t rows, ld, ldg;
  int C, labels_i64;
};

__device__ __forceinline__ long long label_at(const void* labels, int i64, int64_t r) {
  return i64 ? ((const long long*)labels)[r] : (long long)((const int32_t*)labels)[r];
}

// d = a - b as hi + lo exactly (TwoSum on a + (-b))
__device__ __forceinline__ void two_diff(float a, float b, float& hi, float& lo) {
  hi = a - b;
  const float bb = hi - a;
  lo = (a - (hi - bb)) - (b + bb);
}
__device__ __forceinline__ float exp_two(float hi, float lo) {
  const float e = expf(hi);
  return __builtin_fmaf(e, lo, e);
}

// s + c += x with the rounding error of every addition kept in c (TwoSum): the sum of a row's exponentials carries one rounding, not one per term
__device__ __forceinline__ void add_two(float& s, float& c, float x, float xc) {
  const float t = s + x;
  const float bb = t - s;
  c = (c + xc) + ((s - (t - bb)) + (x - bb));   // the error term is exact and the same whichever operand comes first: both lanes of a butterfly step agree
  s = t;
}

template <typename TG>
__device__ __forceinline__ void store8(TG* p, const float (&v)[8], bool vec, int nvalid_store) {
  if (vec) {
    if constexpr (sizeof(TG) == 2) {
      const u32x4 o = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])};
      *(u32x4*)p = o;
    } else {
      *(f32x4*)p = f32x4{v[0], v[1], v[2], v[3]};
      *(f32x4*)(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < nvalid_store) ElemIO<TG>::store(p + j, v[j]);
  }
}

// the workgroup's loss and hit partial: the groups' sums in a fixed tree over LDS (slot s + stride into slot s)
__device__ __forceinline__ void block_partials(float loss, int hit, bool owner, int slot, int nslots, float* loss_part, int32_t* hit_part) {
  __shared__ float sl[ROW_THREADS];
  __shared__ int sh[ROW_THREADS];
  const int tid = threadIdx.x;
  sl[tid] = 0.f; sh[tid] = 0;
  __syncthreads();
  if (owner) { sl[slot] = loss; sh[slot] = hit; }
  __syncthreads();
  for (int s = ROW_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s && tid + s < nslots) { sl[tid] += sl[tid + s]; sh[tid] += sh[tid + s]; }
    __syncthreads();
  }
  if (tid == 0) { loss_part[blockIdx.x] = sl[0]; hit_part[blockIdx.x] = sh[0]; }
}

// LPR lanes hold a row, NU units of 8 columns per lane: unit u of lane g covers columns (u * LPR + g) * 8 .. + 7.  ITERS rows per group.
template <int LPR, int NU, int ITERS, bool VEC, typename TG>
__global__ __launch_bounds__(ROW_THREADS) void k_xent_rows(RowArgs a) {
  constexpr int GROUPS = ROW_THREADS / LPR;
  const int tid = threadIdx.x, g = tid & (LPR - 1), grp = tid / LPR;
  const int C = a.C;
  float loss_acc = 0.f;
  int hit_acc = 0;
  for (int it = 0; it < ITERS; ++it) {
    const int64_t r = ((int64_t)blockIdx.x * ITERS + it) * GROUPS + grp;
    if (r >= a.rows) break;                              // (uniform over the group; no barrier inside the loop)
    const float* zr = a.logits + r * a.ld;
    float z[NU][8];
    float mx = -INFINITY;
    int first = 0x7fffffff;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int c0 = (u * LPR + g) * 8;
      if (VEC) {
        f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = lo;
        if (c0 < C) { lo = *(const f32x4*)(zr + c0); hi = *(const f32x4*)(zr + c0 + 4); }      // c0 < C <= ld, ld % 8 == 0: all 8 inside the row
#pragma unroll
        for (int j = 0; j < 4; ++j) { z[u][j] = lo[j]; z[u][4 + j] = hi[j]; }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) z[u][j] = c0 + j < C ? zr[c0 + j] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (c0 + j < C && z[u][j] > mx) { mx = z[u][j]; first = c0 + j; }      // ascending columns, strictly greater: the lane's first maximum
    }
#pragma unroll
    for (int s = 1; s < LPR; s <<= 1) {
      const float om = __shfl_xor(mx, s, 64);
      const int of = __shfl_xor(first, s, 64);
      if (om > mx || (om == mx && of < first)) { mx = om; first = of; }
    }
    const long long lb = label_at(a.labels, a.labels_i64, r);
    const bool counted = lb >= 0 && lb < C;
    float sum = 0.f, comp = 0.f;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int c0 = (u * LPR + g) * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float hi, lo;
        two_diff(z[u][j], mx, hi, lo);
        const float e = c0 + j < C ? exp_two(hi, lo) : 0.f;
        z[u][j] = e;
        add_two(sum, comp, c0 + j == first ? 0.f : e, 0.f);      // the first maximum's own 1 is added last: log1p of the rest keeps a small loss relative
      }
    }
#pragma unroll
    for (int s = 1; s < LPR; s <<= 1) add_two(sum, comp, __shfl_xor(sum, s, 64), __shfl_xor(comp, s, 64));
    const float rest = sum + comp;
    sum = 1.0f + rest;
    // the label's logit: read again by every lane of the group (one cached dword) -- exact, no reduction
    float rl = 0.f;
    if (counted) {
      float hi, lo;
      two_diff(zr[lb], mx, hi, lo);
      rl = (log1pf(rest) - hi) - lo;
      loss_acc += rl;
      hit_acc += first == (int)lb;
    }
    TG* gr = (TG*)a.G + r * a.ldg;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int c0 = (u * LPR + g) * 8;
      if (c0 >= a.ld) continue;
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float p = counted && c0 + j < C ? z[u][j] / sum : 0.f;
        // p - 1 at the label: as it reads below one half (the result keeps p's absolute error and rounds once); from one half up, where the subtraction
        // would cancel, minus the OTHER terms' share of the sum (the label is then the first maximum, or ties with it: the rest, or sum - 1)
        if (counted && c0 + j == (int)lb) p = p < 0.5f ? p - 1.0f : -((int)lb == first ? rest : sum - z[u][j]) / sum;
        o[j] = p;
      }
      store8<TG>(gr + c0, o, VEC, (int)(a.ld - c0 < 8 ? a.ld - c0 : 8));
    }
  }
  block_partials(loss_acc, hit_acc, g == 0, grp, GROUPS, a.loss_part, a.hit_part);
}

// one workgroup per row: three passes over the row, units of 8 columns strided over the threads
template <bool VEC, typename TG>
__global__ __launch_bounds__(ROW_THREADS) void k_xent_wide(RowArgs a) {
  __shared__ float sv[ROW_THREADS / 64], sc[ROW_THREADS / 64];
  __shared__ int si[ROW_THREADS / 64];
  const int tid = threadIdx.x, C = a.C;
  const int64_t r = blockIdx.x;
  const float* zr = a.logits + r * a.ld;
  const int nunits = (int)((a.ld + 7) / 8);
  auto load8 = [&](int c0, float (&v)[8]) {
    if (VEC && c0 < C) {
      const f32x4 lo = *(const f32x4*)(zr + c0), hi = *(const f32x4*)(zr + c0 + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) { v[j] = lo[j]; v[4 + j] = hi[j]; }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = c0 + j < C ? zr[c0 + j] : 0.f;
    }
  };
  float mx = -INFINITY;
  int first = 0x7fffffff;
  for (int u = tid; u < nunits; u += ROW_THREADS) {
    float v[8];
    load8(u * 8, v);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (u * 8 + j < C && v[j] > mx) { mx = v[j]; first = u * 8 + j; }
  }
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const float om = __shfl_xor(mx, s, 64);
    const int of = __shfl_xor(first, s, 64);
    if (om > mx || (om == mx && of < first)) { mx = om; first = of; }
  }
  if ((tid & 63) == 0) { sv[tid >> 6] = mx; si[tid >> 6] = first; }
  __syncthreads();
  mx = sv[0]; first = si[0];
#pragma unroll
  for (int w = 1; w < ROW_THREADS / 64; ++w)
    if (sv[w] > mx || (sv[w] == mx && si[w] < first)) { mx = sv[w]; first = si[w]; }
  __syncthreads();
  float sum = 0.f, comp = 0.f;
  for (int u = tid; u < nunits; u += ROW_THREADS) {
    float v[8];
    load8(u * 8, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float hi, lo;
      two_diff(v[j], mx, hi, lo);
      add_two(sum, comp, u * 8 + j < C && u * 8 + j != first ? exp_two(hi, lo) : 0.f, 0.f);
    }
  }
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) add_two(sum, comp, __shfl_xor(sum, s, 64), __shfl_xor(comp, s, 64));
  if ((tid & 63) == 0) { sv[tid >> 6] = sum; sc[tid >> 6] = comp; }
  __syncthreads();
  sum = sv[0]; comp = sc[0];
#pragma unroll
  for (int w = 1; w < ROW_THREADS / 64; ++w) add_two(sum, comp, sv[w], sc[w]);
  const float rest = sum + comp;
  sum = 1.0f + rest;
  const long long lb = label_at(a.labels, a.labels_i64, r);
  const bool counted = lb >= 0 && lb < C;
  TG* gr = (TG*)a.G + r * a.ldg;
  for (int u = tid; u < nunits; u += ROW_THREADS) {
    float v[8], o[8];
    load8(u * 8, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float hi, lo;
      two_diff(v[j], mx, hi, lo);
      const float e = exp_two(hi, lo);
      float p = counted && u * 8 + j < C ? e / sum : 0.f;
      if (counted && u * 8 + j == (int)lb) p = p < 0.5f ? p - 1.0f : -((int)lb == first ? rest : sum - e) / sum;
      o[j] = p;
    }
    store8<TG>(gr + u * 8, o, VEC, (int)(a.ld - u * 8 < 8 ? a.ld - u * 8 : 8));
  }
  if (tid == 0) {
    float rl = 0.f;
    int hit = 0;
    if (counted) {
      float hi, lo;
      two_diff(zr[lb], mx, hi, lo);
      rl = (log1pf(rest) - hi) - lo;
      hit = first == (int)lb;
    }
    a.loss_part[r] = rl;
    a.hit_part[r] = hit;
  }
}

// ---- the row kernel's shapes: lanes per row, units per lane, rows per group and workgroup
struct RowPlan { int lpr, nu, iters; int64_t rows_per_wg; };
RowPlan row_plan(int64_t ld) {
  if (ld > WAVE_ROW_MAX_LD) return {0, 0, 0, 1};
  int lpr = 1, nu = 1;
  while (lpr < 64 && (int64_t)lpr * 8 < ld) lpr <<= 1;
  while ((int64_t)lpr * nu * 8 < ld) nu <<= 1;
  const int iters = lpr <= 16 ? lpr : 16;              // 256 rows per workgroup up to 16 lanes per row, 128 at 32, 64 at 64
  return {lpr, nu, iters, (int64_t)(ROW_THREADS / lpr) * iters};
}
int64_t row_blocks(int64_t rows, int64_t ld) {
  const RowPlan p = row_plan(ld);
  return (rows + p.rows_per_wg - 1) / p.rows_per_wg;
}

template <bool VEC, typename TG>
int launch_rows_t(const RowArgs& a, const RowPlan& p, unsigned grid, hipStream_t st) {
#define UVC_XENT_CASE(L, N, I) \
  if (p.lpr == L && p.nu == N) { k_xent_rows<L, N, I, VEC, TG><<<grid, ROW_THREADS, 0, st>>>(a); UVC_CHECK_LAUNCH(); return UVC_OK; }
  if (p.lpr == 0) { k_xent_wide<VEC, TG><<<grid, ROW_THREADS, 0, st>>>(a); UVC_CHECK_LAUNCH(); return UVC_OK; }
  UVC_XENT_CASE(1, 1, 1) UVC_XENT_CASE(2, 1, 2) UVC_XENT_CASE(4, 1, 4) UVC_XENT_CASE(8, 1, 8) UVC_XENT_CASE(16, 1, 16) UVC_XENT_CASE(32, 1, 16)
  UVC_XENT_CASE(64, 1, 16) UVC_XENT_CASE(64, 2, 16) UVC_XENT_CASE(64, 4, 16)
#undef UVC_XENT_CASE
  return uvc_set_error_msg(UVC_ERR_ARG, "uvc_softmax_xent_grad: row plan");
}

int check_rows(const RowArgs& a, int g_dtype) {
  if (!a.logits || !a.labels || !a.G || !a.loss_part || !a.hit_part) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_softmax_xent_grad: null pointer");
  if (a.rows < 1 || a.rows > 0x7fffffffll) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_softmax_xent_grad: rows must lie in [1, 2^31)");
  if (a.C < 1 || a.C > PROBE_MAX_C) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_softmax_xent_grad: C must lie in [1, 65536]");
  if (a.ld < a.C || a.ldg < a.ld || a.ld > PROBE_MAX_C + 7) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_softmax_xent_grad: C <= ld <= ldg, ld <= 65543");
  if (g_dtype != UVC_F32 && g_dtype != UVC_BF16) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_softmax_xent_grad: g_dtype must be UVC_F32 or UVC_BF16");
  const uintptr_t gal = g_dtype == UVC_F32 ? 3 : 1, lal = a.labels_i64 ? 7 : 3;
  if (((uintptr_t)a.logits & 3) || ((uintptr_t)a.G & gal) || ((uintptr_t)a.labels & lal) || (((uintptr_t)a.loss_part | (uintptr_t)a.hit_part) & 3))
    return uvc_set_error_msg(UVC_ERR_ARG, "uvc_softmax_xent_grad: misaligned pointer");
  return UVC_OK;
}

// 16-byte accesses where every row of logits and G starts on 16 bytes and holds whole units of 8
bool rows_vec(const RowArgs& a, int g_dtype) {
  const int64_t gsz = g_dtype == UVC_F32 ? 4 : 2;
  return a.ld % 8 == 0 && ((uintptr_t)a.logits & 15) == 0 && ((uintptr_t)a.G & 15) == 0 && (a.ldg * gsz) % 16 == 0;
}

int launch_rows(const RowArgs& a, int g_dtype, hipStream_t st) {
  const RowPlan p = row_plan(a.ld);
  const unsigned grid = (unsigned)row_blocks(a.rows, a.ld);
  const bool vec = rows_vec(a, g_dtype);
  if (g_dtype == UVC_F32) return vec ? launch_rows_t<true, float>(a, p, grid, st) : launch_rows_t<false, float>(a, p, grid, st);
  return vec ? launch_rows_t<true, bf16_t>(a, p, grid, st) : launch_rows_t<false, bf16_t>(a, p, grid, st);
}

// ---- the evaluator's own launches
struct Scalars { float inv_m; int32_t pad; long long m; };

// m: the labels inside [0, C).  One workgroup; integer sums (any order gives the same value)
__global__ __launch_bounds__(FIN_THREADS) void k_probe_count(const void* labels, int labels_i64, int64_t n, int C, Scalars* sc) {
  __shared__ long long sm[FIN_THREADS / 64];
  long long c = 0;
  for (int64_t i = threadIdx.x; i < n; i += FIN_THREADS) {
    const long long lb = label_at(labels, labels_i64, i);
    c += lb >= 0 && lb < C;
  }
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) c += __shfl_xor(c, s, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long m = 0;
    for (int w = 0; w < FIN_THREADS / 64; ++w) m += sm[w];
    sc->m = m;
    sc->inv_m = m > 0 ? (float)(1.0 / (double)m) : 0.f;
    sc->pad = 0;
  }
}

// W [Cp, D] -> Wop (T); dW = l2 W on rows < C, +0 on the padding rows; db = 0; the workgroup's sum of W^2 over rows < C (thread-strided, fixed tree)
template <typename T>
__global__ __launch_bounds__(PREP_THREADS) void k_probe_prep(const float* __restrict__ W, T* __restrict__ Wop, float* __restrict__ dW, float* __restrict__ db,
                                                             int64_t total, int64_t valid, int Cp, float l2, double* __restrict__ wsq_part) {
  __shared__ double sd[PREP_THREADS];
  const int64_t per = (total / 4 + gridDim.x - 1) / gridDim.x;       // float4 cells per workgroup (total % 4 == 0: D % 8 == 0)
  const int64_t c0 = (int64_t)blockIdx.x * per, c1 = c0 + per < total / 4 ? c0 + per : total / 4;
  double acc = 0.0;
  for (int64_t c = c0 + threadIdx.x; c < c1; c += PREP_THREADS) {
    const f32x4 w = *(const f32x4*)(W + c * 4);
    const bool in = c * 4 < valid;                                   // (valid = C * D, a multiple of 8: a cell is inside or outside)
    if constexpr (sizeof(T) == 2) *(u32x2*)(Wop + c * 4) = u32x2{pack_bf16x2(w[0], w[1]), pack_bf16x2(w[2], w[3])};
    else *(f32x4*)(Wop + c * 4) = w;
    *(f32x4*)(dW + c * 4) = in ? f32x4{l2 * w[0], l2 * w[1], l2 * w[2], l2 * w[3]} : f32x4{0.f, 0.f, 0.f, 0.f};
    if (in) acc += ((double)w[0] * w[0] + (double)w[1] * w[1]) + ((double)w[2] * w[2] + (double)w[3] * w[3]);
  }
  if (db && blockIdx.x == 0)
    for (int c = threadIdx.x; c < Cp; c += PREP_THREADS) db[c] = 0.f;
  sd[threadIdx.x] = acc;
  __syncthreads();
  for (int s = PREP_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sd[threadIdx.x] += sd[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) wsq_part[blockIdx.x] = sd[0];
}

// F = (1 / m) sum loss + (l2 / 2) |W|^2, hits, m.  One workgroup: thread t takes partials t, t + 1024, ... in ascending order, then a fixed tree
__global__ __launch_bounds__(FIN_THREADS) void k_probe_finish(const float* __restrict__ loss_part, const int32_t* __restrict__ hit_part, int64_t nparts,
                                                              const double* __restrict__ wsq_part, int nwsq, const Scalars* __restrict__ sc, float l2,
                                                              double* __restrict__ F, long long* __restrict__ counts) {
  __shared__ double sl[FIN_THREADS], sw[FIN_THREADS];
  __shared__ long long sh[FIN_THREADS];
  const int tid = threadIdx.x;
  double l = 0.0, w = 0.0;
  long long h = 0;
  for (int64_t i = tid; i < nparts; i += FIN_THREADS) { l += (double)loss_part[i]; h += hit_part[i]; }
  for (int i = tid; i < nwsq; i += FIN_THREADS) w += wsq_part[i];
  sl[tid] = l; sw[tid] = w; sh[tid] = h;
  __syncthreads();
  for (int s = FIN_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) { sl[tid] += sl[tid + s]; sw[tid] += sw[tid + s]; sh[tid] += sh[tid + s]; }
    __syncthreads();
  }
  if (tid == 0) {
    const long long m = sc->m;
    F[0] = (m > 0 ? sl[0] / (double)m : 0.0) + 0.5 * (double)l2 * sw[0];
    counts[0] = sh[0];
    counts[1] = m;
  }
}

int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

struct ProbePlan {
  int Cp, chunk, prep_blocks;
  int64_t nchunks, nparts, tn_bytes;
  int64_t o_wop, o_logits, o_g, o_tn, o_loss, o_hit, o_wsq, o_sc, bytes;
};

int probe_shape(int64_t n, int32_t D, int32_t C, int32_t dtype, int32_t chunk_rows) {
  if (dtype != UVC_F32 && dtype != UVC_BF16) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_probe_eval: dtype must be UVC_F32 or UVC_BF16");
  if (n < 1 || n > 0x7fffffffll) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_probe_eval: n must lie in [1, 2^31)");
  if (C < 1 || C > PROBE_MAX_C) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_probe_eval: C must lie in [1, 65536]");
  if (D < 8 || D % 8) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_probe_eval: D must be a multiple of 8");
  if (D > PROBE_MAX_D) return uvc_set_error_msg(UVC_ERR_UNSUPPORTED, "uvc_probe_eval: D must be at most 1024");
  if (chunk_rows < 1) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_probe_eval: chunk_rows must be at least 1");
  return UVC_OK;
}

int probe_plan(int64_t n, int32_t D, int32_t C, int32_t dtype, int32_t chunk_rows, ProbePlan* p) {
  if (const int rc = probe_shape(n, D, C, dtype, chunk_rows)) return rc;
  const int64_t esz = dtype == UVC_F32 ? 4 : 2;
  p->Cp = (C + 7) / 8 * 8;
  p->chunk = (int)((int64_t)chunk_rows < n ? chunk_rows : n);
  p->nchunks = (n + p->chunk - 1) / p->chunk;
  const int64_t last = n - (p->nchunks - 1) * p->chunk;
  p->nparts = (p->nchunks - 1) * row_blocks(p->chunk, p->Cp) + row_blocks(last, p->Cp);
  int64_t t0 = 0, t1 = 0;
  if (uvc_gemm_tn_workspace_bytes(p->chunk, p->Cp, D, &t0, nullptr) || uvc_gemm_tn_workspace_bytes((int)last, p->Cp, D, &t1, nullptr)) return UVC_ERR_ARG;
  p->tn_bytes = t0 > t1 ? t0 : t1;
  const int64_t cells = (int64_t)p->Cp * D / 4;
  p->prep_blocks = (int)((cells + PREP_THREADS * 4 - 1) / (PREP_THREADS * 4));
  if (p->prep_blocks > PREP_MAX_BLOCKS) p->prep_blocks = PREP_MAX_BLOCKS;
  int64_t o = 0;
  p->o_wop = o; o += align256((int64_t)p->Cp * D * esz);
  p->o_logits = o; o += align256((int64_t)p->chunk * p->Cp * 4);
  p->o_g = o; o += align256((int64_t)p->chunk * p->Cp * esz);
  p->o_tn = o; o += align256(p->tn_bytes);
  p->o_loss = o; o += align256(p->nparts * 4);
  p->o_hit = o; o += align256(p->nparts * 4);
  p->o_wsq = o; o += align256((int64_t)p->prep_blocks * 8);
  p->o_sc = o; o += align256(sizeof(Scalars));
  p->bytes = o;
  return UVC_OK;
}

}  // namespace

extern "C" int uvc_softmax_xent_grad_blocks(int64_t rows, int32_t ld, int64_t* blocks) {
  if (!blocks || rows < 1 || ld < 1) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_softmax_xent_grad_blocks: rows and ld must be at least 1");
  *blocks = row_blocks(rows, ld);
  return UVC_OK;
}

extern "C" int uvc_softmax_xent_grad(const float* logits, const void* labels, int32_t labels_i64, int64_t rows, int32_t C, int32_t ld, void* G,
                                     int32_t ldg, int32_t g_dtype, float* loss_part, int32_t* hit_part, void* stream) {
  RowArgs a;
  a.logits = logits; a.labels = labels; a.G = G; a.loss_part = loss_part; a.hit_part = hit_part;
  a.rows = rows; a.ld = ld; a.ldg = ldg; a.C = C; a.labels_i64 = labels_i64 != 0;
  if (const int rc = check_rows(a, g_dtype)) return rc;
  return launch_rows(a, g_dtype, (hipStream_t)stream);
}

extern "C" int uvc_probe_workspace_bytes(int64_t n, int32_t D, int32_t C, int32_t dtype, int32_t chunk_rows, int64_t* bytes) {
  if (!bytes) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_probe_workspace_bytes: null pointer");
  ProbePlan p;
  if (const int rc = probe_plan(n, D, C, dtype, chunk_rows, &p)) return rc;
  *bytes = p.bytes;
  return UVC_OK;
}

extern "C" int uvc_probe_eval(const uvc_probe_args* a, void* stream) {
  if (!a || !a->X || !a->labels || !a->W || !a->dW || !a->F || !a->counts) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_probe_eval: null pointer");
  if ((a->b != nullptr) != (a->db != nullptr)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_probe_eval: b and db go together (both, or neither for a head without bias)");
  ProbePlan p;
  if (const int rc = probe_plan(a->n, a->D, a->C, a->dtype, a->chunk_rows, &p)) return rc;
  const int64_t esz = a->dtype == UVC_F32 ? 4 : 2;
  if (a->ldx < a->D || a->ldx > 0x7fffffffll || (a->ldx * esz) % 16) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_probe_eval: ldx must be at least D, below 2^31, rows 16-byte aligned");
  if ((((uintptr_t)a->X | (uintptr_t)a->W | (uintptr_t)a->dW | (uintptr_t)a->workspace) & 15) || (((uintptr_t)a->b | (uintptr_t)a->db) & 3) ||
      (((uintptr_t)a->F | (uintptr_t)a->counts) & 7) || ((uintptr_t)a->labels & (a->labels_i64 ? 7 : 3)))
    return uvc_set_error_msg(UVC_ERR_ARG, "uvc_probe_eval: misaligned pointer (X, W, dW, workspace: 16 bytes; F, counts: 8; b, db: 4)");
  if (a->l2 != a->l2 || a->l2 < 0.f) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_probe_eval: l2 must be a number >= 0");
  if (!a->workspace || a->workspace_bytes < p.bytes) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_probe_eval: workspace too small (uvc_probe_workspace_bytes)");

  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)a->workspace;
  void* wop = ws + p.o_wop;
  float* logits = (float*)(ws + p.o_logits);
  void* G = ws + p.o_g;
  float* loss_part = (float*)(ws + p.o_loss);
  int32_t* hit_part = (int32_t*)(ws + p.o_hit);
  double* wsq = (double*)(ws + p.o_wsq);
  Scalars* sc = (Scalars*)(ws + p.o_sc);
  const int Cp = p.Cp, D = a->D, i64 = a->labels_i64 != 0;

  k_probe_count<<<1, FIN_THREADS, 0, st>>>(a->labels, i64, a->n, a->C, sc);
  UVC_CHECK_LAUNCH();
  const int64_t total = (int64_t)Cp * D, valid = (int64_t)a->C * D;
  if (esz == 2) k_probe_prep<bf16_t><<<p.prep_blocks, PREP_THREADS, 0, st>>>(a->W, (bf16_t*)wop, a->dW, a->db, total, valid, Cp, a->l2, wsq);
  else k_probe_prep<float><<<p.prep_blocks, PREP_THREADS, 0, st>>>(a->W, (float*)wop, a->dW, a->db, total, valid, Cp, a->l2, wsq);
  UVC_CHECK_LAUNCH();

  int64_t part0 = 0;
  for (int64_t c = 0; c < p.nchunks; ++c) {
    const int64_t r0 = c * p.chunk;
    const int rows = (int)(a->n - r0 < p.chunk ? a->n - r0 : p.chunk);
    const char* xc = (const char*)a->X + r0 * a->ldx * esz;
    const char* lc = (const char*)a->labels + r0 * (i64 ? 8 : 4);

    uvc_gemm_nt_args g = {};
    g.A = xc; g.B = wop; g.C = logits; g.bias = a->b; g.alpha = 1.0f;
    g.M = rows; g.N = Cp; g.K = D; g.lda = (int32_t)a->ldx; g.ldb = D; g.ldc = Cp;
    g.dtype = a->dtype; g.a_is_f32 = esz == 4; g.c_is_f32 = 1; g.epilogue = a->b ? UVC_EPI_BIAS : UVC_EPI_NONE;
    if (const int rc = uvc_gemm_nt(&g, stream)) return rc;

    RowArgs ra;
    ra.logits = logits; ra.labels = lc; ra.G = G; ra.loss_part = loss_part + part0; ra.hit_part = hit_part + part0;
    ra.rows = rows; ra.ld = Cp; ra.ldg = Cp; ra.C = a->C; ra.labels_i64 = i64;
    if (const int rc = launch_rows(ra, a->dtype, st)) return rc;
    part0 += row_blocks(rows, Cp);

    uvc_gemm_tn_args t = {};
    t.A = G; t.B = xc; t.C = a->dW; t.workspace = ws + p.o_tn; t.workspace_bytes = p.tn_bytes;
    t.alpha_ptr = &sc->inv_m; t.colsum_out = a->db; t.alpha = 1.0f; t.beta = 1.0f;
    t.M = rows; t.N1 = Cp; t.N2 = D; t.lda = Cp; t.ldb = (int32_t)a->ldx; t.ldc = D;
    t.dtype = a->dtype; t.a_is_f32 = esz == 4;
    if (const int rc = uvc_gemm_tn(&t, stream)) return rc;
  }
  k_probe_finish<<<1, FIN_THREADS, 0, st>>>(loss_part, hit_part, p.nparts, wsq, p.prep_blocks, sc, a->l2, a->F, (long long*)a->counts);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}
