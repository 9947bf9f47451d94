// Out-of-distribution detectors on a bank (python -m uvc_amd.compact_ood) for gfx950 (include/uvc_kernels.h):
//   uvc_ood_logit_scores  msp, maxlogit, energy and negative entropy of every logits row in ONE pass;
//   uvc_class_moments     class counts and class means of a [n, D] feature bank, float64 sums in a fixed order;
//   uvc_center_rows       x_i - mean_{y_i}, the operand of the scatter GEMM (uvc_gemm_tn);
//   uvc_rows_sqnorm_aug   |z_i|^2 and the augmentation columns 1, 0 .. 0 behind every whitened row (the query side of
//                         min_c |z - m_c|^2 = |z|^2 - 2 max_c (z . m_c - |m_c|^2 / 2), searched by uvc_knn_topk with k = 1).
// No atomics, one writer per output element in every launch, the same bits on a repeat, a row's result does not depend on the rows beside
// it, 64-bit row offsets, workgroup counts functions of the shape alone.
//
// The logit scores take uvc_calib_stats' row organisation: up to 2048 valid columns a group of LPR lanes (1 .. 64, a power of two) holds a
// row in registers, NU units of 4 columns per lane -- one 16-byte load per unit --, workgroup w owns the rows [w R, (w + 1) R) and its
// 256 / LPR groups take them round robin, the next row loaded before the current one is worked on; beyond 2048 columns one workgroup takes
// a row in two passes (the second from cache).  All of a row is float32: the FIRST maximum m (a lane's columns ascending, then the xor
// butterfly: the larger value, the lower column among equals), d_c = z_c - m, rest = sum over c != first of exp(d_c) -- the first maximum's
// own term is exactly 1 -- and sum e_c d_c over the same columns (a term whose exponential underflowed is 0: 0 log 0 = 0):
//   msp = 1 / (1 + rest),  maxlogit = m,  energy = m + T log1p(sum_{c != first} exp(d_c / T)),  -H = (sum e_c d_c) / (1 + rest) - log1p(rest).
// With T = 1 the second exponential is not taken.  A NaN in a valid column makes the row's four results NaN.
//
// The moments read the bank ONCE, whatever C is: the caller hands in the permutation of a stable sort of the labels, workgroup s takes the
// 256 positions [256 s, 256 s + 256) of the sorted order, thread t the columns 4 t .. 4 t + 3 of every row, in ascending position.  A class
// that lies inside one slice is finished there (sum / count in float64, rounded once); of a class that crosses a slice border the slice
// leaves a partial sum ("head": the run from the slice's first position, "tail": the run that reaches its end), and uvc_class_moments'
// second launch -- one workgroup per class -- adds those in ascending slice order and writes the counts and the +0 rows of empty classes.
// So the order of every (class, column) sum is a function of the sorted labels alone.
#include <cstdio>
#include "common.h"
#include "../../include/uvc_kernels.h"

namespace {

constexpr int OOD_THREADS = 256;
constexpr int OOD_WAVES = OOD_THREADS / 64;
constexpr int OOD_MAX_C = 65536;
constexpr int OOD_REG_MAX_C = 2048;         // wider rows: one workgroup per row
constexpr int OOD_MAX_BLOCKS = 2048;
constexpr int OOD_MAX_D = 1016;             // D + 8 augmentation columns is uvc_knn_topk's widest row
constexpr int CM_SL = 256;                  // positions of the sorted order per workgroup

// ---------------------------------------------------------------------------------------------------------------- the logit scores
struct LsArgs {
  const float* logits; float* msp; float* mxl; float* energy; float* entropy;
  int64_t n, ld, rows_per_wg;
  int C, t_one;
  float T;
};

__device__ __forceinline__ void ls_write(const LsArgs& a, int64_t r, bool bad, float mx, float rest, float sed, float rest_t) {
  const float nan = __builtin_nanf("");
  const float sum = 1.0f + rest, lg = log1pf(rest);
  if (a.msp) a.msp[r] = bad ? nan : 1.0f / sum;
  if (a.mxl) a.mxl[r] = bad ? nan : mx;
  if (a.energy) a.energy[r] = bad ? nan : (a.t_one ? mx + lg : __builtin_fmaf(a.T, log1pf(rest_t), mx));
  if (a.entropy) a.entropy[r] = bad ? nan : sed / sum - lg;
}

template <int LPR, int NU, bool VEC>
__global__ __launch_bounds__(OOD_THREADS) void k_ood_rows(LsArgs a) {
  constexpr int GROUPS = OOD_THREADS / LPR;
  const int tid = threadIdx.x, g = tid & (LPR - 1), grp = tid / LPR;
  const int C = a.C;
  const int64_t wg0 = (int64_t)blockIdx.x * a.rows_per_wg;
  const int64_t wg1 = wg0 + a.rows_per_wg < a.n ? wg0 + a.rows_per_wg : a.n;

  auto load = [&](float (&v)[NU][4], int64_t r) {
    const float* zr = a.logits + r * a.ld;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int c0 = (u * LPR + g) * 4;
      if (VEC) {
        f32x4 q = {0.f, 0.f, 0.f, 0.f};
        if (c0 < C) q = *(const f32x4*)(zr + c0);           // c0 < C <= ld, ld % 4 == 0: all 4 inside the row
#pragma unroll
        for (int j = 0; j < 4; ++j) v[u][j] = q[j];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[u][j] = c0 + j < C ? zr[c0 + j] : 0.f;
      }
    }
  };

  float z[NU][4], zn[NU][4];
  int64_t r = wg0 + grp;
  if (r < wg1) load(z, r);
  for (; r < wg1; r += GROUPS) {                             // (a group's lanes leave together: every shuffle partner is live)
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) zn[u][j] = z[u][j];
    if (r + GROUPS < wg1) load(zn, r + GROUPS);
    float mx = -INFINITY;
    int first = 0x7fffffff, bad = 0;
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = (u * LPR + g) * 4 + j;
        const float v = z[u][j];
        if (c < C) {
          bad |= v != v;
          if (v > mx) { mx = v; first = c; }                 // ascending columns, strictly greater: the lane's first maximum
        }
      }
#pragma unroll
    for (int s = 1; s < LPR; s <<= 1) {
      const float om = __shfl_xor(mx, s, 64);
      const int of = __shfl_xor(first, s, 64);
      bad |= __shfl_xor(bad, s, 64);
      if (om > mx || (om == mx && of < first)) { mx = om; first = of; }
    }
    float rest = 0.f, sed = 0.f, rest_t = 0.f;
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = (u * LPR + g) * 4 + j;
        if (c < C && c != first) {
          const float d = z[u][j] - mx;
          const float e = expf(d);
          rest += e;
          if (e > 0.f) sed = __builtin_fmaf(e, d, sed);
          if (!a.t_one) rest_t += expf(d / a.T);
        }
      }
#pragma unroll
    for (int s = 1; s < LPR; s <<= 1) {
      rest += __shfl_xor(rest, s, 64);
      sed += __shfl_xor(sed, s, 64);
      rest_t += __shfl_xor(rest_t, s, 64);
    }
    if (g == 0) ls_write(a, r, bad != 0, mx, rest, sed, rest_t);
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) z[u][j] = zn[u][j];
  }
}

// beyond 2048 columns: workgroup = row, thread t the units t, t + 256, ... of 4 columns
__device__ __forceinline__ float ood_wg_sum(float v, float* sv) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) v += __shfl_xor(v, s, 64);
  __syncthreads();                                           // (the readers of the call before are done)
  if ((threadIdx.x & 63) == 0) sv[threadIdx.x >> 6] = v;
  __syncthreads();
  v = sv[0];
#pragma unroll
  for (int w = 1; w < OOD_WAVES; ++w) v += sv[w];
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(OOD_THREADS) void k_ood_wide(LsArgs a) {
  __shared__ float smx[OOD_WAVES], sv[OOD_WAVES];
  __shared__ int sfi[OOD_WAVES], sbad[OOD_WAVES];
  const int tid = threadIdx.x, C = a.C;
  const int nunits = (C + 3) / 4;
  const int64_t r = blockIdx.x;
  const float* zr = a.logits + r * a.ld;
  auto load4 = [&](int c0, float (&v)[4]) {
    if (VEC) {
      const f32x4 q = *(const f32x4*)(zr + c0);             // c0 < C <= ld, ld % 4 == 0
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = q[j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = c0 + j < C ? zr[c0 + j] : 0.f;
    }
  };
  float mx = -INFINITY;
  int first = 0x7fffffff, bad = 0;
  for (int u = tid; u < nunits; u += OOD_THREADS) {
    float v[4];
    load4(u * 4, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = u * 4 + j;
      if (c < C) {
        bad |= v[j] != v[j];
        if (v[j] > mx) { mx = v[j]; first = c; }
      }
    }
  }
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const float om = __shfl_xor(mx, s, 64);
    const int of = __shfl_xor(first, s, 64);
    bad |= __shfl_xor(bad, s, 64);
    if (om > mx || (om == mx && of < first)) { mx = om; first = of; }
  }
  if ((tid & 63) == 0) { smx[tid >> 6] = mx; sfi[tid >> 6] = first; sbad[tid >> 6] = bad; }
  __syncthreads();
  mx = smx[0]; first = sfi[0]; bad = sbad[0];
#pragma unroll
  for (int w = 1; w < OOD_WAVES; ++w) {
    bad |= sbad[w];
    if (smx[w] > mx || (smx[w] == mx && sfi[w] < first)) { mx = smx[w]; first = sfi[w]; }
  }
  float rest = 0.f, sed = 0.f, rest_t = 0.f;
  for (int u = tid; u < nunits; u += OOD_THREADS) {
    float v[4];
    load4(u * 4, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = u * 4 + j;
      if (c < C && c != first) {
        const float d = v[j] - mx;
        const float e = expf(d);
        rest += e;
        if (e > 0.f) sed = __builtin_fmaf(e, d, sed);
        if (!a.t_one) rest_t += expf(d / a.T);
      }
    }
  }
  rest = ood_wg_sum(rest, sv);
  sed = ood_wg_sum(sed, sv);
  if (!a.t_one) rest_t = ood_wg_sum(rest_t, sv);             // (uniform over the workgroup)
  if (tid == 0) ls_write(a, r, bad != 0, mx, rest, sed, rest_t);
}

int64_t ls_rows_per_wg(int64_t n, int64_t ld) {
  int64_t least = 16384 / ld;                                // a workgroup reads 64 KB or more
  least = least < 4 ? 4 : least > 256 ? 256 : least;
  const int64_t spread = (n + OOD_MAX_BLOCKS - 1) / OOD_MAX_BLOCKS;
  return least > spread ? least : spread;
}

template <bool VEC>
int ls_launch(LsArgs& a, hipStream_t st) {
  if (a.C > OOD_REG_MAX_C) { k_ood_wide<VEC><<<(unsigned)a.n, OOD_THREADS, 0, st>>>(a); UVC_CHECK_LAUNCH(); return UVC_OK; }
  a.rows_per_wg = ls_rows_per_wg(a.n, a.ld);
  const unsigned grid = (unsigned)((a.n + a.rows_per_wg - 1) / a.rows_per_wg);
  int lpr = 1, nu = 1;
  while (lpr < 64 && lpr * 4 < a.C) lpr <<= 1;
  while (lpr * nu * 4 < a.C) nu <<= 1;
#define UVC_OOD_CASE(L, N) \
  if (lpr == L && nu == N) { k_ood_rows<L, N, VEC><<<grid, OOD_THREADS, 0, st>>>(a); UVC_CHECK_LAUNCH(); return UVC_OK; }
  UVC_OOD_CASE(1, 1) UVC_OOD_CASE(2, 1) UVC_OOD_CASE(4, 1) UVC_OOD_CASE(8, 1) UVC_OOD_CASE(16, 1) UVC_OOD_CASE(32, 1)
  UVC_OOD_CASE(64, 1) UVC_OOD_CASE(64, 2) UVC_OOD_CASE(64, 4) UVC_OOD_CASE(64, 8)
#undef UVC_OOD_CASE
  return uvc_set_error_msg(UVC_ERR_ARG, "uvc_ood_logit_scores: row plan");
}

// ---------------------------------------------------------------------------------------------------------------- the class moments
struct CmArgs {
  const float* X; const void* labels; const long long* perm;
  double* part;          // [slices][2][D]: head, tail
  long long* counts; float* means;
  int64_t n, ldx;
  int D, C, labels_i64, vec;
};

// the label at sorted position j; a permutation entry outside [0, n) reads nothing and counts as a skipped row
__device__ __forceinline__ long long cm_key(const CmArgs& a, int64_t j) {
  const long long row = a.perm[j];
  if (row < 0 || row >= a.n) return 0x7fffffffffffffffll;
  return a.labels_i64 ? ((const long long*)a.labels)[row] : (long long)((const int32_t*)a.labels)[row];
}
__device__ __forceinline__ int cm_class(const CmArgs& a, int64_t j) {
  const long long k = cm_key(a, j);
  return k >= 0 && k < a.C ? (int)k : -1;
}

__global__ __launch_bounds__(OOD_THREADS) void k_cm_slices(CmArgs a) {
  __shared__ long long srow[CM_SL];
  __shared__ int slab[CM_SL];
  __shared__ int sedge[2];
  const int tid = threadIdx.x, D = a.D;
  const int64_t j0 = (int64_t)blockIdx.x * CM_SL;
  const int cnt = (int)(a.n - j0 < CM_SL ? a.n - j0 : CM_SL);
  for (int i = tid; i < cnt; i += blockDim.x) {
    const long long row = a.perm[j0 + i];
    const int c = cm_class(a, j0 + i);
    srow[i] = c >= 0 ? row : -1;                             // (c >= 0: the row lies in [0, n))
    slab[i] = c;
  }
  if (tid == 0) {
    sedge[0] = j0 > 0 ? cm_class(a, j0 - 1) : -1;
    sedge[1] = j0 + cnt < a.n ? cm_class(a, j0 + cnt) : -1;
  }
  __syncthreads();
  const int c0 = tid * 4;
  if (c0 >= D) return;                                       // (no barrier below)
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  int cur = -1, run0 = 0;
  auto flush = [&](int end) {                                // the run [run0, end) of class cur
    if (cur < 0) return;
    const bool open_left = run0 == 0 && sedge[0] == cur, open_right = end == cnt && sedge[1] == cur;
    if (!open_left && !open_right) {
      const double m = (double)(end - run0);
      const f32x4 q = {(float)(acc[0] / m), (float)(acc[1] / m), (float)(acc[2] / m), (float)(acc[3] / m)};
      *(f32x4*)(a.means + (int64_t)cur * D + c0) = q;        // means is 16-byte aligned, D % 8 == 0
    } else {
      double* p = a.part + ((int64_t)blockIdx.x * 2 + (run0 == 0 ? 0 : 1)) * D + c0;
#pragma unroll
      for (int k = 0; k < 4; ++k) p[k] = acc[k];
    }
  };
  for (int i = 0; i < cnt; i += 4) {
    f32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (i + u < cnt && srow[i + u] >= 0) {
        const float* x = a.X + srow[i + u] * a.ldx + c0;
        if (a.vec) v[u] = *(const f32x4*)x;
        else v[u] = f32x4{x[0], x[1], x[2], x[3]};
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (i + u < cnt) {
        const int c = slab[i + u];
        if (c != cur) {
          flush(i + u);
          cur = c; run0 = i + u;
          acc[0] = acc[1] = acc[2] = acc[3] = 0.0;
        }
        if (c >= 0) {
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] += (double)v[u][k];
        }
      }
    }
  }
  flush(cnt);
}

__device__ __forceinline__ int64_t cm_lower_bound(const CmArgs& a, long long key) {       // the first position whose label is >= key
  int64_t lo = 0, hi = a.n;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (cm_key(a, mid) < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(OOD_THREADS) void k_cm_finish(CmArgs a) {
  __shared__ int64_t sb[2];
  const int tid = threadIdx.x, D = a.D, c = blockIdx.x;
  if (tid < 2) sb[tid] = cm_lower_bound(a, (long long)c + tid);
  __syncthreads();
  const int64_t b0 = sb[0], b1 = sb[1] > sb[0] ? sb[1] : sb[0];
  if (tid == 0) a.counts[c] = b1 - b0;
  const int c0 = tid * 4;
  if (c0 >= D) return;
  float* out = a.means + (int64_t)c * D + c0;
  if (b1 == b0) { *(f32x4*)out = f32x4{0.f, 0.f, 0.f, 0.f}; return; }
  const int64_t s0 = b0 / CM_SL, s1 = (b1 - 1) / CM_SL;
  if (s0 == s1) return;                                      // finished by its slice
  double acc[4];
  const double* p = a.part + (s0 * 2 + (b0 == s0 * CM_SL ? 0 : 1)) * D + c0;
#pragma unroll
  for (int k = 0; k < 4; ++k) acc[k] = p[k];
  for (int64_t s = s0 + 1; s <= s1; ++s) {
    p = a.part + s * 2 * D + c0;
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] += p[k];
  }
  const double m = (double)(b1 - b0);
  *(f32x4*)out = f32x4{(float)(acc[0] / m), (float)(acc[1] / m), (float)(acc[2] / m), (float)(acc[3] / m)};
}

// ---------------------------------------------------------------------------------------------------------------- centred rows
template <bool VEC>
__global__ __launch_bounds__(OOD_THREADS) void k_center_rows(const float* __restrict__ X, int64_t ldx, const void* __restrict__ labels, int labels_i64,
                                                             const float* __restrict__ means, int64_t n, int D, int C, float* __restrict__ out, int64_t ldo) {
  const int qpr = D / 4;
  const int64_t q = (int64_t)blockIdx.x * OOD_THREADS + threadIdx.x;
  const int64_t r = q / qpr;
  if (r >= n) return;
  const int c0 = (int)(q - r * qpr) * 4;
  const long long lb = labels_i64 ? ((const long long*)labels)[r] : (long long)((const int32_t*)labels)[r];
  const bool counted = lb >= 0 && lb < C;
  const float* x = X + r * ldx + c0;
  const float* m = means + (counted ? lb : 0) * (int64_t)D + c0;
  float* o = out + r * ldo + c0;
  if (VEC) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (counted) v = *(const f32x4*)x - *(const f32x4*)m;
    *(f32x4*)o = v;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = counted ? x[j] - m[j] : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------------------- |z|^2 and the augmentation
// one wave per row: lane l sums the squares of columns (64 u + l) 4 .. + 3, u ascending (a fmaf chain), then the xor butterfly
template <bool VEC>
__global__ __launch_bounds__(OOD_THREADS) void k_rows_sqnorm_aug(float* __restrict__ Z, int64_t ldz, int64_t n, int D, float* __restrict__ sq) {
  const int l = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * OOD_WAVES + (threadIdx.x >> 6);
  if (r >= n) return;                                        // (wave-uniform)
  float* z = Z + r * ldz;
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int c0 = (u * 64 + l) * 4;
    if (c0 < D) {                                            // D % 4 == 0: all 4 inside [0, D)
      f32x4 v;
      if (VEC) v = *(const f32x4*)(z + c0);
      else v = f32x4{z[c0], z[c0 + 1], z[c0 + 2], z[c0 + 3]};
#pragma unroll
      for (int j = 0; j < 4; ++j) s = __builtin_fmaf(v[j], v[j], s);
    }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
  if (l == 0) sq[r] = s;
  if (l < 8) z[D + l] = l == 0 ? 1.0f : 0.f;
}

int ood_refuse(const char* who, const char* what, int code = UVC_ERR_ARG) {
  static thread_local char msg[200];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return uvc_set_error_msg(code, msg);
}

int ood_dims(const char* who, int64_t n, int32_t D) {
  if (n < 1 || n > 0x7fffffffll) return ood_refuse(who, "n must lie in [1, 2^31)");
  if (D < 8 || D % 8) return ood_refuse(who, "D must be a multiple of 8, at least 8");
  if (D > OOD_MAX_D) return ood_refuse(who, "D must be at most 1016", UVC_ERR_UNSUPPORTED);
  return UVC_OK;
}

int64_t cm_slices(int64_t n) { return (n + CM_SL - 1) / CM_SL; }

}  // namespace

extern "C" int uvc_ood_logit_scores(const float* logits, int64_t n, int64_t ld, int32_t n_valid, float temperature, float* msp, float* maxlogit,
                                    float* energy, float* entropy, void* stream) {
  const char* who = "uvc_ood_logit_scores";
  if (!logits) return ood_refuse(who, "null pointer");
  if (!msp && !maxlogit && !energy && !entropy) return ood_refuse(who, "no output");
  if (n < 1 || n > 0x7fffffffll) return ood_refuse(who, "n must lie in [1, 2^31)");
  if (n_valid < 1) return ood_refuse(who, "n_valid must be at least 1");
  if (n_valid > OOD_MAX_C) return ood_refuse(who, "n_valid must be at most 65536", UVC_ERR_UNSUPPORTED);
  if (ld < n_valid || ld > 0x7fffffffll) return ood_refuse(who, "n_valid <= ld < 2^31");
  if (!(temperature > 0.f) || temperature == INFINITY) return ood_refuse(who, "temperature must be positive and finite");
  if (((uintptr_t)logits | (uintptr_t)msp | (uintptr_t)maxlogit | (uintptr_t)energy | (uintptr_t)entropy) & 3) return ood_refuse(who, "misaligned pointer");
  LsArgs a;
  a.logits = logits; a.msp = msp; a.mxl = maxlogit; a.energy = energy; a.entropy = entropy;
  a.n = n; a.ld = ld; a.rows_per_wg = 1; a.C = n_valid; a.t_one = temperature == 1.0f; a.T = temperature;
  const bool vec = ld % 4 == 0 && ((uintptr_t)logits & 15) == 0;
  return vec ? ls_launch<true>(a, (hipStream_t)stream) : ls_launch<false>(a, (hipStream_t)stream);
}

extern "C" int uvc_class_moments_workspace_bytes(int64_t n, int32_t D, int64_t* bytes) {
  if (!bytes) return ood_refuse("uvc_class_moments_workspace_bytes", "null pointer");
  if (const int rc = ood_dims("uvc_class_moments_workspace_bytes", n, D)) return rc;
  *bytes = cm_slices(n) * 2 * D * 8;
  return UVC_OK;
}

extern "C" int uvc_class_moments(const float* X, int64_t ldx, const void* labels, int32_t labels_i64, const int64_t* perm, int64_t n, int32_t D,
                                 int32_t C, int64_t* counts, float* means, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "uvc_class_moments";
  if (!X || !labels || !perm || !counts || !means) return ood_refuse(who, "null pointer");
  if (const int rc = ood_dims(who, n, D)) return rc;
  if (C < 1) return ood_refuse(who, "C must be at least 1");
  if (C > OOD_MAX_C) return ood_refuse(who, "C must be at most 65536", UVC_ERR_UNSUPPORTED);
  if (ldx < D) return ood_refuse(who, "ldx must be at least D");
  if (((uintptr_t)X & 3) || ((uintptr_t)means & 15) || (((uintptr_t)perm | (uintptr_t)counts | (uintptr_t)workspace) & 7) ||
      ((uintptr_t)labels & (labels_i64 ? 7 : 3)))
    return ood_refuse(who, "misaligned pointer (means: 16 bytes; perm, counts, workspace and int64 labels: 8; the rest: 4)");
  if (!workspace || workspace_bytes < cm_slices(n) * 2 * D * 8) return ood_refuse(who, "workspace too small (uvc_class_moments_workspace_bytes)");
  CmArgs a;
  a.X = X; a.labels = labels; a.perm = (const long long*)perm; a.part = (double*)workspace; a.counts = (long long*)counts; a.means = means;
  a.n = n; a.ldx = ldx; a.D = D; a.C = C; a.labels_i64 = labels_i64 != 0; a.vec = ldx % 4 == 0 && ((uintptr_t)X & 15) == 0;
  const unsigned threads = (unsigned)((D / 4 + 63) / 64 * 64);
  hipStream_t st = (hipStream_t)stream;
  k_cm_slices<<<(unsigned)cm_slices(n), threads, 0, st>>>(a);
  UVC_CHECK_LAUNCH();
  k_cm_finish<<<(unsigned)C, threads, 0, st>>>(a);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

extern "C" int uvc_center_rows(const float* X, int64_t ldx, const void* labels, int32_t labels_i64, const float* means, int64_t n, int32_t D, int32_t C,
                               float* out, int64_t ldo, void* stream) {
  const char* who = "uvc_center_rows";
  if (!X || !labels || !means || !out) return ood_refuse(who, "null pointer");
  if (const int rc = ood_dims(who, n, D)) return rc;
  if (C < 1 || C > OOD_MAX_C) return ood_refuse(who, "C must lie in [1, 65536]");
  if (ldx < D || ldo < D) return ood_refuse(who, "ldx and ldo must be at least D");
  if ((((uintptr_t)X | (uintptr_t)means | (uintptr_t)out) & 3) || ((uintptr_t)labels & (labels_i64 ? 7 : 3))) return ood_refuse(who, "misaligned pointer");
  const bool vec = ldx % 4 == 0 && ldo % 4 == 0 && (((uintptr_t)X | (uintptr_t)means | (uintptr_t)out) & 15) == 0;
  const int64_t quads = n * (D / 4);
  if ((quads + OOD_THREADS - 1) / OOD_THREADS > 0x7fffffffll) return ood_refuse(who, "n * D / 4 must stay below 2^39 (chunk the rows)", UVC_ERR_UNSUPPORTED);
  const unsigned grid = (unsigned)((quads + OOD_THREADS - 1) / OOD_THREADS);
  hipStream_t st = (hipStream_t)stream;
  if (vec) k_center_rows<true><<<grid, OOD_THREADS, 0, st>>>(X, ldx, labels, labels_i64 != 0, means, n, D, C, out, ldo);
  else k_center_rows<false><<<grid, OOD_THREADS, 0, st>>>(X, ldx, labels, labels_i64 != 0, means, n, D, C, out, ldo);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

extern "C" int uvc_rows_sqnorm_aug(float* Z, int64_t ldz, int64_t n, int32_t D, float* sq, void* stream) {
  const char* who = "uvc_rows_sqnorm_aug";
  if (!Z || !sq) return ood_refuse(who, "null pointer");
  if (const int rc = ood_dims(who, n, D)) return rc;
  if (ldz < D + 8) return ood_refuse(who, "ldz must be at least D + 8");
  if (((uintptr_t)Z | (uintptr_t)sq) & 3) return ood_refuse(who, "misaligned pointer");
  const bool vec = ldz % 4 == 0 && ((uintptr_t)Z & 15) == 0;
  const unsigned grid = (unsigned)((n + OOD_WAVES - 1) / OOD_WAVES);
  hipStream_t st = (hipStream_t)stream;
  if (vec) k_rows_sqnorm_aug<true><<<grid, OOD_THREADS, 0, st>>>(Z, ldz, n, D, sq);
  else k_rows_sqnorm_aug<false><<<grid, OOD_THREADS, 0, st>>>(Z, ldz, n, D, sq);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}
