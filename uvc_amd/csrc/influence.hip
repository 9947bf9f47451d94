// Last-layer training-data influence on feature banks (python -m uvc_amd.compact_influence) for gfx950: uvc_influence_residuals, the softmax
// residuals r = softmax(z) - e_target of a logits bank; uvc_influence_topk, the k largest and the k smallest of
// v(t, i) = (f_t . f_i + bias) * (r_t . r_i) per query without either [nq, n] matrix; uvc_influence_self, the diagonal (|f_i|^2 + bias) |r_i|^2
// (include/uvc_kernels.h).
//
// uvc_influence_topk is knn.hip's tile loop with a second product and a second list.  One workgroup takes 64 queries, 4 waves of 16; the
// bank is visited in ascending tiles of 64 rows.  Per tile a wave first forms sf, the feature dot products, exactly as k_knn_topk does: its
// queries' features live in registers as the B operand (v_mfma_f32_16x16x32_bf16, or v_mfma_f32_16x16x4_f32), the bank's features stream
// through LDS as the A operand, 256 bytes of a row at a time.  Then sr, the residual dot products: the residuals are float32 and up to 4096
// wide, too wide for registers, so BOTH operands stream through LDS in chunks of 64 columns -- the tile's 64 bank rows (A) and the
// workgroup's 64 query rows (B, re-read from L2 for every tile) -- into v_mfma_f32_16x16x4_f32, a c-ascending fmaf chain.  All chunks of a
// tile, features then residuals, go through one double-buffered pipeline: the next chunk is on its way in registers while this one is
// multiplied, one barrier per chunk.  v = (sf + bias) * sr is one float32 add and one multiply; a row past the range and the query's excluded
// row become NaN, which no comparison admits.  A lane holds ONE query and 16 of the tile's rows, so both of the query's thresholds are
// registers; the lists are knn.hip's sorted lists in LDS, the whole wave inserting one candidate.  The list of the smallest values is kept as
// a list of the largest of -v (exact) and negated on the way out: one insertion routine, one merge kernel, one tie rule -- equal values by
// ascending bank row, which the ascending visit gives for free.
// A pair's v is the same two chains of MFMAs on the same operands wherever the pair sits: it does not depend on nq, n, the tile or the
// split; the lists are a function of those values under a total order -- the same bits for every split count.  With few query tiles the
// bank is split into contiguous row ranges over gridDim.y and k_influence_merge combines the partial lists (knn.hip's scheme).  No atomics;
// every output element has one writer.
//
// Footprint: LDS 4 x 17 408 bytes of staging + 1 024 k bytes of lists -- 74 752 at k = 5 (two workgroups per CU), 135 168 at
// k = 64 (one); registers 193 .. 228 (bf16, D <= 384: two waves per SIMD), 278 / 312 beyond (one); float32 208 / 243, then 291 .. 467.
#include <type_traits>
#include <cmath>
#include "common.h"
#include "../../include/uvc_kernels.h"

namespace {

constexpr int QT = 64;                      // queries per workgroup
constexpr int BT = 64;                      // bank rows per tile
constexpr int CHB = 256;                    // bytes of a row per chunk: 128 bf16, 64 float32
constexpr int RC = CHB / 4;                 // residual columns per chunk
constexpr int ROWB = CHB + 16;              // LDS row stride, 68 dwords (knn.hip)
constexpr int BUFB = BT * ROWB;
constexpr int IF_MAX_K = 64;
constexpr int IF_MAX_D = 1024;
constexpr int IF_MAX_CR = 4096;
constexpr int IF_MAX_SPLITS = 512;          // the merge takes 64 lists per wave: at most two levels
constexpr int IF_MAX_C = 65536;

struct TopkArgs {
  const void* fq; const void* fb; const float* rq; const float* rb; const int32_t* exclude;
  float* out_s[2]; int32_t* out_i[2];       // [0]: the largest v, [1]: the largest -v; NULL: not wanted
  int64_t ldfq, ldfb, ldrq, ldrb, rows_per_split;
  float bias;
  int nq, n, D, Cr, k, final;               // final: the lists go to the caller's arrays (the second one negated), not to the workspace
};

// NCH: the feature chunks the query registers are sized for (knn.hip)
template <typename T, int NCH>
__global__ __launch_bounds__(256) void k_influence_topk(TopkArgs a) {
  constexpr bool LOWP = sizeof(T) == 2;
  constexpr int EPS = 16 / (int)sizeof(T);
  constexpr int KC = CHB / (int)sizeof(T);
  constexpr int NQF = LOWP ? NCH * 4 : NCH * 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* qsm = smem + 2 * BUFB;                           // the queries' residual chunks, two buffers
  float* ls = (float*)(smem + 4 * BUFB);                 // [2][64][k] values, descending
  int32_t* li = (int32_t*)(ls + 2 * QT * a.k);           // [2][64][k] bank rows
  const int tid = threadIdx.x, l = tid & 63, wave = tid >> 6, lc = l & 15, lq = l >> 4;
  const int nq = a.nq, D = a.D, Cr = a.Cr, k = a.k;
  const T* __restrict__ fq = (const T*)a.fq;
  const T* __restrict__ fb = (const T*)a.fb;
  const float* __restrict__ rq = a.rq;
  const float* __restrict__ rb = a.rb;
  const int nchd = (D + KC - 1) / KC, nchr = (Cr + RC - 1) / RC;
  const int64_t row_begin = (int64_t)blockIdx.y * a.rows_per_split;
  const int64_t row_end = row_begin + a.rows_per_split < (int64_t)a.n ? row_begin + a.rows_per_split : (int64_t)a.n;
  const int ntiles = row_begin < row_end ? (int)((row_end - row_begin + BT - 1) / BT) : 0;
  const int64_t q0 = (int64_t)blockIdx.x * QT;
  const int64_t qrow = q0 + wave * 16 + lc;
  const bool want[2] = {a.out_s[0] != nullptr, a.out_s[1] != nullptr};

  typename std::conditional<LOWP, bf16x8, float>::type qf[NQF];
  if constexpr (LOWP) {
#pragma unroll
    for (int s = 0; s < NQF; ++s) {
      const int e = s * 32 + lq * 8;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (qrow < nq && e < D) v = *(const u32x4*)(fq + (size_t)qrow * a.ldfq + e);
      qf[s] = __builtin_bit_cast(bf16x8, v);
    }
  } else {
#pragma unroll
    for (int s = 0; s < NQF; ++s) {
      const int e = s * 4 + lq;
      qf[s] = (qrow < nq && e < D) ? fq[(size_t)qrow * a.ldfq + e] : 0.f;
    }
  }
  if (l < 16)
    for (int w = 0; w < 2; ++w)
      for (int j = 0; j < k; ++j) { ls[(w * QT + wave * 16 + lc) * k + j] = -INFINITY; li[(w * QT + wave * 16 + lc) * k + j] = -1; }
  // the value a candidate must beat, per list: a query row past nq and a list that is not wanted never have a candidate
  float thr0 = (qrow < nq && want[0]) ? -INFINITY : INFINITY;
  float thr1 = (qrow < nq && want[1]) ? -INFINITY : INFINITY;
  const int64_t ex = (a.exclude && qrow < nq) ? (int64_t)a.exclude[qrow] : -1;
  const bool live = q0 + wave * 16 < nq;                 // (wave-uniform)

  u32x4 st[4], sq[4];
  auto gload_f = [&](int tile, int c) {                  // 64 bank rows x 16 segments of features
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int seg = tid + i * 256;
      const int64_t row = row_begin + (int64_t)tile * BT + (seg >> 4);
      const int e = c * KC + (seg & 15) * EPS;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (row < row_end && e < D) v = *(const u32x4*)(fb + (size_t)row * a.ldfb + e);
      st[i] = v;
    }
  };
  auto gload_r = [&](int tile, int c) {                  // 64 bank rows and the 64 queries x 16 segments of residuals
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int seg = tid + i * 256;
      const int64_t row = row_begin + (int64_t)tile * BT + (seg >> 4);
      const int64_t qr = q0 + (seg >> 4);
      const int e = c * RC + (seg & 15) * 4;
      u32x4 v = {0u, 0u, 0u, 0u}, w = {0u, 0u, 0u, 0u};
      if (row < row_end && e < Cr) v = *(const u32x4*)(rb + (size_t)row * a.ldrb + e);
      if (qr < nq && e < Cr) w = *(const u32x4*)(rq + (size_t)qr * a.ldrq + e);
      st[i] = v;
      sq[i] = w;
    }
  };
  // the whole wave inserts candidates of one list: w[rt][r] > thr, in ascending bank row order (knn.hip)
  auto scan = [&](const f32x4 (&w)[4], float& thr, float* lsx, int32_t* lix, int64_t tile0) {
    bool cand = false;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) cand |= w[rt][r] > thr;
    if (!__any(cand)) return;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
      unsigned long long m[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) m[r] = __ballot(w[rt][r] > thr);
#pragma unroll
      for (int qq = 0; qq < 4; ++qq)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          unsigned mm = (unsigned)(m[r] >> (16 * qq)) & 0xffffu;
          while (mm) {
            const int qi = __ffs((int)mm) - 1;
            mm &= mm - 1;
            const float v = __shfl(w[rt][r], qq * 16 + qi, 64);
            const int base = (wave * 16 + qi) * k;
            const float e = l < k ? lsx[base + l] : 0.f;
            const int pos = __popcll(__ballot(l < k && e >= v));
            if (pos < k) {
              const int ei = l < k ? lix[base + l] : -1;
              const float up_s = __shfl_up(e, 1, 64);
              const int up_i = __shfl_up(ei, 1, 64);
              const float mine = l == pos ? v : (l > pos ? up_s : e);
              if (l >= pos && l < k) {
                lsx[base + l] = mine;
                lix[base + l] = l == pos ? (int32_t)(tile0 + rt * 16 + qq * 4 + r) : up_i;
              }
              const float last = __shfl(mine, k - 1, 64);
              if (lc == qi) thr = last;
            }
          }
        }
    }
  };

  int par = 0;
  if (ntiles > 0) gload_f(0, 0);
  for (int tile = 0; tile < ntiles; ++tile) {
    f32x4 accf[4], accr[4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) { accf[rt] = f32x4{0.f, 0.f, 0.f, 0.f}; accr[rt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (c < nchd) {
        char* buf = smem + par * BUFB;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int seg = tid + i * 256;
          *(u32x4*)(buf + (seg >> 4) * ROWB + (seg & 15) * 16) = st[i];
        }
        __syncthreads();      // one barrier per chunk: the buffer written next was last read before the previous barrier
        if (c + 1 < nchd) gload_f(tile, c + 1);
        else gload_r(tile, 0);
        if (!live) {
        } else if constexpr (LOWP) {
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            if (c * KC + s * 32 < D) {
#pragma unroll
              for (int rt = 0; rt < 4; ++rt) {
                const bf16x8 af = *(const bf16x8*)(buf + (rt * 16 + lc) * ROWB + s * 64 + lq * 16);
                accf[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, qf[c * 4 + s], accf[rt], 0, 0, 0);
              }
            }
          }
        } else {
#pragma unroll
          for (int s = 0; s < 16; ++s) {
            if (c * KC + s * 4 < D) {
#pragma unroll
              for (int rt = 0; rt < 4; ++rt) {
                const float af = *(const float*)(buf + (rt * 16 + lc) * ROWB + (s * 4 + lq) * 4);
                accf[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, qf[c * 16 + s], accf[rt], 0, 0, 0);
              }
            }
          }
        }
        par ^= 1;
      }
    }
    for (int c = 0; c < nchr; ++c) {
      char* buf = smem + par * BUFB;
      char* qbuf = qsm + par * BUFB;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int seg = tid + i * 256;
        *(u32x4*)(buf + (seg >> 4) * ROWB + (seg & 15) * 16) = st[i];
        *(u32x4*)(qbuf + (seg >> 4) * ROWB + (seg & 15) * 16) = sq[i];
      }
      __syncthreads();
      if (c + 1 < nchr) gload_r(tile, c + 1);
      else if (tile + 1 < ntiles) gload_f(tile + 1, 0);
      if (live) {
#pragma unroll
        for (int s = 0; s < 16; ++s) {
          if (c * RC + s * 4 < Cr) {
            const float bq = *(const float*)(qbuf + (wave * 16 + lc) * ROWB + (s * 4 + lq) * 4);          // B[k = lane >> 4][col = lane & 15]
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) {
              const float ar = *(const float*)(buf + (rt * 16 + lc) * ROWB + (s * 4 + lq) * 4);           // A[row = lane & 15][k = lane >> 4]
              accr[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar, bq, accr[rt], 0, 0, 0);
            }
          }
        }
      }
      par ^= 1;
    }
    // acc*[rt][reg]: this lane's query against bank row tile0 + rt * 16 + (lane >> 4) * 4 + reg
    const int64_t tile0 = row_begin + (int64_t)tile * BT;
    f32x4 nv[4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = tile0 + rt * 16 + lq * 4 + r;
        float v = (accf[rt][r] + a.bias) * accr[rt][r];
        if (row >= row_end || row == ex) v = __builtin_nanf("");      // masked: a NaN beats no threshold
        accf[rt][r] = v;
        nv[rt][r] = -v;
      }
    scan(accf, thr0, ls, li, tile0);
    scan(nv, thr1, ls + QT * k, li + QT * k, tile0);
  }
  __syncthreads();
  for (int w = 0; w < 2; ++w) {
    if (!want[w]) continue;
    const bool flip = w == 1 && a.final;
    for (int qi = 0; qi < 16; ++qi) {
      const int64_t qr = q0 + wave * 16 + qi;
      if (qr < nq && l < k) {
        const size_t o = ((size_t)blockIdx.y * nq + (size_t)qr) * k + l;
        const float s = ls[(w * QT + wave * 16 + qi) * k + l];
        a.out_s[w][o] = flip ? -s : s;
        a.out_i[w][o] = li[(w * QT + wave * 16 + qi) * k + l];
      }
    }
  }
}

// k_knn_merge with a sign on the way out: one wave per query and group of 64 lists, the largest head goes out, the lowest lane among equals
__global__ __launch_bounds__(64) void k_influence_merge(const float* __restrict__ ws_s, const int32_t* __restrict__ ws_i, int nq, int k, int nlists,
                                                        float sign, float* __restrict__ vals, int32_t* __restrict__ idx) {
  const int l = threadIdx.x;
  const size_t qr = blockIdx.x;
  const int list = blockIdx.y * 64 + l;
  const size_t base = ((size_t)list * nq + qr) * k;
  vals += (size_t)blockIdx.y * nq * k;
  idx += (size_t)blockIdx.y * nq * k;
  int pos = 0;
  float hs = -INFINITY;
  int hi = -1;
  if (list < nlists) { hs = ws_s[base]; hi = ws_i[base]; }
  if (hi < 0) hs = -INFINITY;
  for (int j = 0; j < k; ++j) {
    const float mx = wave_max(hs);
    const unsigned long long m = __ballot(hi >= 0 && hs == mx);
    float os = -INFINITY;
    int oi = -1;
    if (m) {
      const int w = __ffsll(m) - 1;
      os = mx;
      oi = __shfl(hi, w, 64);
      if (l == w) {
        ++pos;
        hs = -INFINITY; hi = -1;
        if (pos < k) { hs = ws_s[base + pos]; hi = ws_i[base + pos]; }
        if (hi < 0) hs = -INFINITY;
      }
    }
    if (l == 0) { vals[qr * k + j] = sign < 0.f ? -os : os; idx[qr * k + j] = oi; }
  }
}

// ---------------------------------------------------------------------------- residuals (uvc_influence_residuals)
__device__ __forceinline__ long long if_label(const void* labels, int i64, int64_t r) {
  return i64 ? ((const long long*)labels)[r] : (long long)((const int32_t*)labels)[r];
}

// one wave per row, lane l the columns l, l + 64, ...: the maximum (and its first column), the float64 sum of the float32 exponentials,
// then the outputs; the row is read three times, twice from cache
__global__ __launch_bounds__(256) void k_influence_residuals(const float* __restrict__ logits, int64_t n, int64_t ld, int C, const void* __restrict__ labels,
                                                             int labels_i64, int mode, float* __restrict__ r, int64_t ldr, int32_t* __restrict__ target,
                                                             float* __restrict__ rsq) {
  const int l = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const float* z = logits + row * ld;
  float* out = r + row * ldr;
  float mx = -INFINITY;
  int first = 0x7fffffff;
  for (int c = l; c < C; c += 64) {
    const float v = z[c];
    if (v > mx) { mx = v; first = c; }                   // a NaN is never the maximum
  }
  const float top = wave_max(mx);
  if (!(mx == top)) first = 0x7fffffff;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) first = min(first, __shfl_xor(first, s, 64));
  long long t = -1;
  if (mode == 0) {
    const long long lb = if_label(labels, labels_i64, row);
    if (lb >= 0 && lb < C) t = lb;
  } else if (first < C) {
    t = first;
  }
  if (t < 0) {                                           // (wave-uniform) a skipped row: +0 everywhere
    for (int64_t c = l; c < ldr; c += 64) out[c] = 0.f;
    if (l == 0) { target[row] = -1; rsq[row] = 0.f; }
    return;
  }
  double sum = 0.0;
  for (int c = l; c < C; c += 64) sum += (double)expf(z[c] - top);
  sum = wave_sum_f64(sum);
  double sq = 0.0;
  for (int64_t c = l; c < ldr; c += 64) {
    float o = 0.f;
    if (c < C) {
      const double p = (double)expf(z[c] - top) / sum;
      o = (float)(c == t ? p - 1.0 : p);
      sq += (double)o * (double)o;
    }
    out[c] = o;
  }
  sq = wave_sum_f64(sq);
  if (l == 0) { target[row] = (int32_t)t; rsq[row] = (float)sq; }
}

__global__ __launch_bounds__(256) void k_influence_expf(const float* __restrict__ d, float* __restrict__ e, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) e[i] = expf(d[i]);
}

// ---------------------------------------------------------------------------- the diagonal (uvc_influence_self)
// one wave per row: lane l takes columns (64 u + l) 4 .. + 3, u ascending, as one fmaf chain, then the xor butterfly (uvc_rows_sqnorm_aug's order)
template <typename T>
__global__ __launch_bounds__(256) void k_influence_self(const T* __restrict__ f, int64_t ldf, int64_t n, int D, const float* __restrict__ rsq, float bias,
                                                        float* __restrict__ fsq, float* __restrict__ out) {
  const int l = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const T* x = f + row * ldf;
  float s = 0.f;
  for (int c = l * 4; c < D; c += 256) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float v = ElemIO<T>::load(x + c + j);
      s = __builtin_fmaf(v, v, s);
    }
  }
  s = wave_sum(s);
  if (l == 0) {
    if (fsq) fsq[row] = s;
    if (out) out[row] = (s + bias) * rsq[row];
  }
}

struct Plan { int splits; int64_t rows_per_split; };

int64_t ws_cells(int splits, int nq, int k) {
  if (splits <= 1) return 0;
  const int64_t groups = splits > 64 ? (splits + 63) / 64 : 0;
  return ((int64_t)splits + groups) * nq * k;
}

// splits <= 0: from the shapes and the device's CU count (knn.hip's rule); any request is clamped to [1, min(512, bank tiles)]
Plan plan_of(int nq, int n, int splits) {
  const int64_t ntiles = ((int64_t)n + BT - 1) / BT, qtiles = ((int64_t)nq + QT - 1) / QT;
  int64_t s = splits;
  if (s <= 0) {
    int ncu = 256, dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0) ncu = 256;
    s = qtiles >= 2 * (int64_t)ncu ? 1 : (2 * (int64_t)ncu + qtiles - 1) / qtiles;
  }
  if (s > IF_MAX_SPLITS) s = IF_MAX_SPLITS;
  if (s > ntiles) s = ntiles;
  if (s < 1) s = 1;
  const int64_t rps = (ntiles + s - 1) / s * BT;
  return {(int)(((int64_t)n + rps - 1) / rps), rps};
}

int check_shape(int32_t nq, int32_t n, int32_t k) {
  if (nq < 1 || n < 1) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_influence_topk: nq and n must be at least 1");
  if (k < 1 || k > IF_MAX_K) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_influence_topk: k must lie in [1, 64]");
  return UVC_OK;
}

template <typename T, int NCH>
int launch_topk(const TopkArgs& t, const Plan& p, hipStream_t st) {
  const int lds = 4 * BUFB + QT * t.k * 16;
  UVC_MAX_LDS(4 * BUFB + QT * IF_MAX_K * 16, k_influence_topk<T, NCH>);
  const dim3 grid((unsigned)(((int64_t)t.nq + QT - 1) / QT), (unsigned)p.splits);
  k_influence_topk<T, NCH><<<grid, 256, lds, st>>>(t);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

}  // namespace

extern "C" int uvc_influence_workspace_bytes(int32_t nq, int32_t n, int32_t k, int32_t splits, int64_t* bytes, int32_t* splits_used) {
  if (int e = check_shape(nq, n, k)) return e;
  if (!bytes) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_influence_workspace_bytes: null pointer");
  const Plan p = plan_of(nq, n, splits);
  *bytes = 2 * ws_cells(p.splits, nq, k) * 8;
  if (splits_used) *splits_used = p.splits;
  return UVC_OK;
}

extern "C" int uvc_influence_topk(const uvc_influence_args* a, void* stream) {
  if (!a || !a->fq || !a->fb || !a->rq || !a->rb) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_influence_topk: null pointer");
  if ((!a->pos_vals) != (!a->pos_idx) || (!a->neg_vals) != (!a->neg_idx) || (!a->pos_vals && !a->neg_vals))
    return uvc_set_error_msg(UVC_ERR_ARG, "uvc_influence_topk: values and indices of a list go together, and at least one list is wanted");
  if (int e = check_shape(a->nq, a->n, a->k)) return e;
  if ((a->q_dtype != UVC_F32 && a->q_dtype != UVC_BF16) || (a->bank_dtype != UVC_F32 && a->bank_dtype != UVC_BF16))
    return uvc_set_error_msg(UVC_ERR_ARG, "uvc_influence_topk: bad dtype");
  if (a->q_dtype != a->bank_dtype)
    return uvc_set_error_msg(UVC_ERR_UNSUPPORTED, "uvc_influence_topk: query and bank features must have one dtype (both bf16 or both float32)");
  if (a->D < 8 || a->D > IF_MAX_D || a->D % 8) return uvc_set_error_msg(UVC_ERR_UNSUPPORTED, "uvc_influence_topk: D must be a multiple of 8 in [8, 1024]");
  if (a->Cr < 8 || a->Cr > IF_MAX_CR || a->Cr % 8) return uvc_set_error_msg(UVC_ERR_UNSUPPORTED, "uvc_influence_topk: Cr must be a multiple of 8 in [8, 4096]");
  if (!std::isfinite(a->bias)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_influence_topk: bias must be finite");
  const int64_t esz = a->q_dtype == UVC_F32 ? 4 : 2;
  if (a->ldfq < a->D || a->ldfb < a->D || a->ldrq < a->Cr || a->ldrb < a->Cr)
    return uvc_set_error_msg(UVC_ERR_ARG, "uvc_influence_topk: leading dimensions must be at least D and Cr");
  if ((((uintptr_t)a->fq | (uintptr_t)a->fb | (uintptr_t)a->rq | (uintptr_t)a->rb) & 15) || (a->ldfq * esz) % 16 || (a->ldfb * esz) % 16 || (a->ldrq * 4) % 16 ||
      (a->ldrb * 4) % 16)
    return uvc_set_error_msg(UVC_ERR_ARG, "uvc_influence_topk: features, residuals and their row strides must be 16-byte aligned");
  if (((uintptr_t)a->exclude | (uintptr_t)a->pos_vals | (uintptr_t)a->pos_idx | (uintptr_t)a->neg_vals | (uintptr_t)a->neg_idx) & 3)
    return uvc_set_error_msg(UVC_ERR_ARG, "uvc_influence_topk: exclude and the lists must be 4-byte aligned");
  const Plan p = plan_of(a->nq, a->n, a->splits);
  TopkArgs t;
  t.fq = a->fq; t.fb = a->fb; t.rq = a->rq; t.rb = a->rb; t.exclude = a->exclude;
  t.ldfq = a->ldfq; t.ldfb = a->ldfb; t.ldrq = a->ldrq; t.ldrb = a->ldrb; t.rows_per_split = p.rows_per_split;
  t.bias = a->bias;
  t.nq = a->nq; t.n = a->n; t.D = a->D; t.Cr = a->Cr; t.k = a->k; t.final = p.splits <= 1;
  float* user_s[2] = {a->pos_vals, a->neg_vals};
  int32_t* user_i[2] = {a->pos_idx, a->neg_idx};
  const int64_t cells = ws_cells(p.splits, a->nq, a->k);
  if (p.splits > 1) {
    if (!a->workspace || a->workspace_bytes < 2 * cells * 8 || ((uintptr_t)a->workspace & 3))
      return uvc_set_error_msg(UVC_ERR_ARG, "uvc_influence_topk: workspace too small (uvc_influence_workspace_bytes)");
    for (int w = 0; w < 2; ++w) {
      t.out_s[w] = user_s[w] ? (float*)a->workspace + w * cells : nullptr;
      t.out_i[w] = user_s[w] ? (int32_t*)a->workspace + 2 * cells + w * cells : nullptr;
    }
  } else {
    for (int w = 0; w < 2; ++w) { t.out_s[w] = user_s[w]; t.out_i[w] = user_i[w]; }
  }
  hipStream_t st = (hipStream_t)stream;
  const int nchd = (int)((a->D * esz + CHB - 1) / CHB);
  int rc;
  if (esz == 2) {
    if (nchd <= 1) rc = launch_topk<bf16_t, 1>(t, p, st);
    else if (nchd <= 2) rc = launch_topk<bf16_t, 2>(t, p, st);
    else if (nchd <= 3) rc = launch_topk<bf16_t, 3>(t, p, st);
    else if (nchd <= 6) rc = launch_topk<bf16_t, 6>(t, p, st);
    else rc = launch_topk<bf16_t, 8>(t, p, st);
  } else {
    if (nchd <= 1) rc = launch_topk<float, 1>(t, p, st);
    else if (nchd <= 3) rc = launch_topk<float, 3>(t, p, st);
    else if (nchd <= 6) rc = launch_topk<float, 6>(t, p, st);
    else if (nchd <= 12) rc = launch_topk<float, 12>(t, p, st);
    else rc = launch_topk<float, 16>(t, p, st);
  }
  if (rc) return rc;
  if (p.splits > 1) {
    for (int w = 0; w < 2; ++w) {
      if (!user_s[w]) continue;
      const float sign = w ? -1.f : 1.f;
      const float* in_s = t.out_s[w];
      const int32_t* in_i = t.out_i[w];
      int lists = p.splits;
      if (lists > 64) {      // level one: groups of 64 splits into the lists behind the splits' (still values of the kept sign)
        const int groups = (lists + 63) / 64;
        float* mid_s = t.out_s[w] + (int64_t)lists * a->nq * a->k;
        int32_t* mid_i = t.out_i[w] + (int64_t)lists * a->nq * a->k;
        k_influence_merge<<<dim3((unsigned)a->nq, (unsigned)groups), 64, 0, st>>>(in_s, in_i, a->nq, a->k, lists, 1.f, mid_s, mid_i);
        UVC_CHECK_LAUNCH();
        in_s = mid_s; in_i = mid_i; lists = groups;
      }
      k_influence_merge<<<dim3((unsigned)a->nq, 1), 64, 0, st>>>(in_s, in_i, a->nq, a->k, lists, sign, user_s[w], user_i[w]);
      UVC_CHECK_LAUNCH();
    }
  }
  return UVC_OK;
}

extern "C" int uvc_influence_residuals(const float* logits, int64_t n, int64_t ld, int32_t C, const void* labels, int32_t labels_i64, int32_t target_mode,
                                       float* r, int64_t ldr, int32_t* target, float* rsq, void* stream) {
  if (!logits || !r || !target || !rsq || (target_mode == 0 && !labels)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_influence_residuals: null pointer");
  if (target_mode != 0 && target_mode != 1) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_influence_residuals: target_mode must be 0 (label) or 1 (argmax)");
  if (n < 1 || n >= (1ll << 31)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_influence_residuals: n must lie in [1, 2^31)");
  if (C < 1 || ld < C || ld >= (1ll << 31)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_influence_residuals: 1 <= C <= ld < 2^31");
  if (C > IF_MAX_C) return uvc_set_error_msg(UVC_ERR_UNSUPPORTED, "uvc_influence_residuals: at most 65536 classes");
  if (ldr < C || ldr % 8 || ldr >= (1ll << 31)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_influence_residuals: ldr must be a multiple of 8, at least C");
  if (((uintptr_t)r & 15) || ((uintptr_t)logits & 3) || ((uintptr_t)target & 3) || ((uintptr_t)rsq & 3) ||
      (labels && ((uintptr_t)labels & (labels_i64 ? 7 : 3))))
    return uvc_set_error_msg(UVC_ERR_ARG, "uvc_influence_residuals: r must be 16-byte aligned, the other operands to their element size");
  k_influence_residuals<<<(unsigned)((n + 3) / 4), 256, 0, (hipStream_t)stream>>>(logits, n, ld, C, labels, labels_i64 != 0, target_mode, r, ldr, target, rsq);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

extern "C" int uvc_influence_self(const void* f, int64_t ldf, int32_t dtype, int64_t n, int32_t D, const float* rsq, float bias, float* fsq, float* out,
                                  void* stream) {
  if (!f || (!fsq && !out) || (out && !rsq)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_influence_self: null pointer");
  if (dtype != UVC_F32 && dtype != UVC_BF16) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_influence_self: bad dtype");
  if (n < 1 || n >= (1ll << 31)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_influence_self: n must lie in [1, 2^31)");
  if (D < 8 || D > IF_MAX_D || D % 8) return uvc_set_error_msg(UVC_ERR_UNSUPPORTED, "uvc_influence_self: D must be a multiple of 8 in [8, 1024]");
  if (ldf < D) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_influence_self: ldf must be at least D");
  if (!std::isfinite(bias)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_influence_self: bias must be finite");
  const int64_t esz = dtype == UVC_F32 ? 4 : 2;
  if (((uintptr_t)f & (esz - 1)) || ((uintptr_t)rsq & 3) || ((uintptr_t)fsq & 3) || ((uintptr_t)out & 3))
    return uvc_set_error_msg(UVC_ERR_ARG, "uvc_influence_self: misaligned operand");
  const unsigned grid = (unsigned)((n + 3) / 4);
  if (dtype == UVC_F32) k_influence_self<float><<<grid, 256, 0, (hipStream_t)stream>>>((const float*)f, ldf, n, D, rsq, bias, fsq, out);
  else k_influence_self<bf16_t><<<grid, 256, 0, (hipStream_t)stream>>>((const bf16_t*)f, ldf, n, D, rsq, bias, fsq, out);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

extern "C" int uvc_influence_expf(const float* d, float* e, int64_t n, void* stream) {
  if (!d || !e || n < 1 || n >= (1ll << 31)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_influence_expf: d, e and 1 <= n < 2^31");
  k_influence_expf<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(d, e, n);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}
