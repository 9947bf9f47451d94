// Split conformal prediction on a logits bank (python -m uvc_amd.compact_conformal) for gfx950: uvc_conformal_scores, the conformal score of
// every row's label, and uvc_conformal_sets, the prediction sets {c : s(c) <= qhat} (include/uvc_kernels.h).
//
// The order of a row's classes -- descending logit, ties by ascending index, -0 = +0 -- is taken on order-preserving integer keys of the
// float32 inputs (as uvc_patch_rank's), so ranks are exact.  The exponentials e_c = expf(float((z_c - z_max) inv_T)) are float32; every sum
// of them (all of a row, or those ranked ahead of a class) is a float64 sum in a fixed order, and the score is formed in float64 and
// rounded once.
//
// Scores: only the label's rank and the mass ahead of it are wanted, O(C) per row.  The rows are read the way calib.hip reads them:
// workgroup w owns the rows [w R, (w + 1) R), up to 2048 classes a group of LPR lanes (1 .. 64) holds a row in registers, NU units of 4
// columns per lane -- one 16-byte load per unit --, the groups of a workgroup split its rows into contiguous runs and the next row is loaded
// before the current one is worked on.  A lane sums its columns in ascending order, the group then runs the xor butterfly.  Beyond 2048
// classes a workgroup takes one row at a time in two passes (the second from cache).  m is counted by one more launch over the labels.
//
// Sets: rank and mass of EVERY class.  A row's P = ceil-pow2(C) pairs (~key, index) -- 64-bit, all distinct -- are sorted ascending by a
// bitonic network in LDS: log2 P (log2 P + 1) / 2 steps of P / 2 compare-exchanges against the C^2 compare-selects of counting (C = 1000: 28 160
// against 1 000 000).  TPR = min(256, P / 2) threads take a row, a workgroup 256 / TPR rows at a time.  After the sort position i holds the class
// of rank i + 1 and position 0 the maximum; thread t owns the positions [t E, (t + 1) E), E = P / TPR, sums their exponentials, and the exclusive
// prefix over the threads is taken in two levels of at most 16 (blocks of 16 threads, then the blocks), in ascending order.  A flag per
// class goes to LDS by class index; word w of the row is then built and written by one thread.
#include <cstdio>
#include <cmath>
#include "common.h"
#include "../../include/uvc_kernels.h"

namespace {

constexpr int CF_THREADS = 256;
constexpr int CF_WAVES = CF_THREADS / 64;
constexpr int CF_MAX_C = 65536;
constexpr int CF_REG_MAX_C = 2048;        // scores: wider rows take one workgroup per row
constexpr int CF_SETS_MAX_C = 2048;       // sets: a row's pairs in LDS
constexpr int CF_MAX_BLOCKS = 2048;
constexpr int CF_SCAN_BLOCK = 16;

struct CfArgs {
  const float* logits; const void* labels; const float* u;
  float* scores; long long* counts;
  int32_t* size; uint8_t* covered; uint32_t* members;
  int64_t n, ld, rows_per_wg;
  int C, labels_i64, method, k_reg;
  float inv_t, lam, qhat;
};

__device__ __forceinline__ long long cf_label(const void* labels, int i64, int64_t r) {
  return i64 ? ((const long long*)labels)[r] : (long long)((const int32_t*)labels)[r];
}
// larger logit <=> larger key; -0 and +0 share one
__device__ __forceinline__ uint32_t cf_key(float z) {
  uint32_t b = __float_as_uint(z);
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float cf_exp(float z, float mx, float inv_t) {
  return expf((float)(((double)z - (double)mx) * (double)inv_t));
}
// e: the class's exponential, ahead: the sum of those ranked ahead of it, sum: of all, rank: 1 .. C
__device__ __forceinline__ float cf_score(int method, double e, double ahead, double sum, int rank, float u, float lam, int k_reg) {
  const double inv = 1.0 / sum;
  if (method == UVC_CONFORMAL_LAC) return (float)((sum - e) * inv);
  double s = (ahead + (double)u * e) * inv;
  if (method == UVC_CONFORMAL_RAPS && rank > k_reg) s += (double)lam * (double)(rank - k_reg);
  return (float)s;
}

// ---- scores, up to 2048 classes: LPR lanes hold a row, unit u of lane g covers columns (u * LPR + g) * 4 .. + 3
template <int LPR, int NU, bool VEC>
__global__ __launch_bounds__(CF_THREADS) void k_conformal_scores_rows(CfArgs a) {
  constexpr int GROUPS = CF_THREADS / LPR;
  const int tid = threadIdx.x, g = tid & (LPR - 1), grp = tid / LPR;
  const int C = a.C;
  const int64_t wg0 = (int64_t)blockIdx.x * a.rows_per_wg;
  const int64_t wg1 = wg0 + a.rows_per_wg < a.n ? wg0 + a.rows_per_wg : a.n;
  const int64_t k = (a.rows_per_wg + GROUPS - 1) / GROUPS;
  const int64_t r0 = wg0 + grp * k;
  const int64_t r1 = r0 + k < wg1 ? r0 + k : wg1;

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
  if (r0 < r1) load(z, r0);
  for (int64_t r = r0; r < r1; ++r) {
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) zn[u][j] = z[u][j];
    if (r + 1 < r1) load(zn, r + 1);
    const long long lb = cf_label(a.labels, a.labels_i64, r);
    float out = __builtin_nanf("");
    if (lb >= 0 && lb < C) {                                 // (uniform over the group)
      float mx = -INFINITY;
#pragma unroll
      for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int c = (u * LPR + g) * 4 + j;
          if (c < C && z[u][j] > mx) mx = z[u][j];
        }
#pragma unroll
      for (int s = 1; s < LPR; s <<= 1) {
        const float om = __shfl_xor(mx, s, 64);
        if (om > mx) mx = om;
      }
      // the label's logit: read again by every lane of the group (one cached dword)
      const float zy = a.logits[r * a.ld + lb];
      const uint32_t ky = cf_key(zy);
      double sum = 0.0, ahead = 0.0;
      int before = 0;
#pragma unroll
      for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int c = (u * LPR + g) * 4 + j;
          if (c < C) {
            const float e = cf_exp(z[u][j], mx, a.inv_t);
            const uint32_t kc = cf_key(z[u][j]);
            const bool first = kc > ky || (kc == ky && c < (int)lb);
            sum += (double)e;
            ahead += first ? (double)e : 0.0;
            before += first;
          }
        }
#pragma unroll
      for (int s = 1; s < LPR; s <<= 1) {
        sum += __shfl_xor(sum, s, 64);
        ahead += __shfl_xor(ahead, s, 64);
        before += __shfl_xor(before, s, 64);
      }
      out = cf_score(a.method, (double)cf_exp(zy, mx, a.inv_t), ahead, sum, before + 1, a.u ? a.u[r] : 1.0f, a.lam, a.k_reg);
    }
    if (g == 0) a.scores[r] = out;
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) z[u][j] = zn[u][j];
  }
}

// ---- scores, beyond 2048 classes: the workgroup takes one row at a time, thread t the units t, t + 256, ... of 4 columns
template <bool VEC>
__global__ __launch_bounds__(CF_THREADS) void k_conformal_scores_wide(CfArgs a) {
  __shared__ float smx[CF_WAVES];
  __shared__ double ssum[CF_WAVES], sah[CF_WAVES];
  __shared__ int sbe[CF_WAVES];
  const int tid = threadIdx.x, C = a.C;
  const int nunits = (C + 3) / 4;
  const int64_t wg0 = (int64_t)blockIdx.x * a.rows_per_wg;
  const int64_t wg1 = wg0 + a.rows_per_wg < a.n ? wg0 + a.rows_per_wg : a.n;
  for (int64_t r = wg0; r < wg1; ++r) {
    const long long lb = cf_label(a.labels, a.labels_i64, r);
    if (lb < 0 || lb >= C) {                                 // (uniform over the workgroup)
      if (tid == 0) a.scores[r] = __builtin_nanf("");
      continue;
    }
    const float* zr = a.logits + r * a.ld;
    auto load4 = [&](int c0, float (&v)[4]) {
      if (VEC) {
        const f32x4 q = *(const f32x4*)(zr + c0);           // c0 < C <= ld, ld % 4 == 0
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = q[j];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = c0 + j < C ? zr[c0 + j] : 0.f;
      }
    };
    float mx = -INFINITY;
    for (int u = tid; u < nunits; u += CF_THREADS) {
      float v[4];
      load4(u * 4, v);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (u * 4 + j < C && v[j] > mx) mx = v[j];
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const float om = __shfl_xor(mx, s, 64);
      if (om > mx) mx = om;
    }
    __syncthreads();                                         // (the readers of the row before are done)
    if ((tid & 63) == 0) smx[tid >> 6] = mx;
    __syncthreads();
    mx = smx[0];
#pragma unroll
    for (int w = 1; w < CF_WAVES; ++w)
      if (smx[w] > mx) mx = smx[w];
    const float zy = zr[lb];
    const uint32_t ky = cf_key(zy);
    double sum = 0.0, ahead = 0.0;
    int before = 0;
    for (int u = tid; u < nunits; u += CF_THREADS) {
      float v[4];
      load4(u * 4, v);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = u * 4 + j;
        if (c < C) {
          const float e = cf_exp(v[j], mx, a.inv_t);
          const uint32_t kc = cf_key(v[j]);
          const bool first = kc > ky || (kc == ky && c < (int)lb);
          sum += (double)e;
          ahead += first ? (double)e : 0.0;
          before += first;
        }
      }
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      sum += __shfl_xor(sum, s, 64);
      ahead += __shfl_xor(ahead, s, 64);
      before += __shfl_xor(before, s, 64);
    }
    if ((tid & 63) == 0) { ssum[tid >> 6] = sum; sah[tid >> 6] = ahead; sbe[tid >> 6] = before; }
    __syncthreads();
    if (tid == 0) {
      sum = ssum[0]; ahead = sah[0]; before = sbe[0];
      for (int w = 1; w < CF_WAVES; ++w) { sum += ssum[w]; ahead += sah[w]; before += sbe[w]; }
      a.scores[r] = cf_score(a.method, (double)cf_exp(zy, mx, a.inv_t), ahead, sum, before + 1, a.u ? a.u[r] : 1.0f, a.lam, a.k_reg);
    }
  }
}

// ---- m: the labels inside [0, C), one workgroup
__global__ __launch_bounds__(1024) void k_conformal_count(CfArgs a) {
  __shared__ long long sc[1024];
  const int tid = threadIdx.x;
  long long m = 0;
  for (int64_t r = tid; r < a.n; r += 1024) {
    const long long lb = cf_label(a.labels, a.labels_i64, r);
    m += lb >= 0 && lb < a.C;
  }
  sc[tid] = m;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if (tid < s) sc[tid] += sc[tid + s];
    __syncthreads();
  }
  if (tid == 0) a.counts[0] = sc[0];
}

// ---- sets: TPR threads sort a row's P pairs in LDS; P, TPR powers of two, TPR = min(256, P / 2) (P = 2: TPR = 1)
__global__ __launch_bounds__(CF_THREADS) void k_conformal_sets(CfArgs a, int P, int TPR) {
  __shared__ unsigned long long srt[CF_SETS_MAX_C];          // rows * P <= 2048
  __shared__ float sz[CF_SETS_MAX_C];
  __shared__ uint8_t sflag[CF_SETS_MAX_C];
  __shared__ double dsum[CF_THREADS], bsum[CF_THREADS];
  __shared__ int scnt[CF_THREADS];
  const int tid = threadIdx.x, C = a.C;
  const int rows = CF_THREADS / TPR, seg = tid / TPR, t = tid & (TPR - 1);
  const int E = P / TPR, half = P / 2;
  const int W = (C + 31) / 32;
  unsigned long long* ms = srt + seg * P;
  float* mz = sz + seg * P;
  uint8_t* mf = sflag + seg * P;
  const int64_t batches = (a.n + rows - 1) / rows;
  for (int64_t b = blockIdx.x; b < batches; b += gridDim.x) { // (uniform over the workgroup: every thread meets every barrier)
    const int64_t r = b * rows + seg;
    const bool live = r < a.n;
    const float* zr = a.logits + (live ? r : 0) * a.ld;
    for (int c = t; c < P; c += TPR) {
      const bool real = live && c < C;
      const float z = real ? zr[c] : 0.f;
      mz[c] = z;
      mf[c] = 0;
      ms[c] = ((unsigned long long)(real ? ~cf_key(z) : 0xffffffffu) << 32) | (unsigned)c;
    }
    __syncthreads();
    for (int kk = 2; kk <= P; kk <<= 1)
      for (int j = kk >> 1; j > 0; j >>= 1) {
        for (int q = t; q < half; q += TPR) {
          const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1));
          const int p = i | j;                               // i < p < P
          const unsigned long long x = ms[i], y = ms[p];
          if ((x > y) == ((i & kk) == 0)) { ms[i] = y; ms[p] = x; }
        }
        __syncthreads();
      }
    // position i < C holds the class of rank i + 1; the pairs of the padding (and of a row past n) are behind them
    const float mx = mz[(unsigned)ms[0]];
    double own = 0.0;
    for (int i = t * E; i < (t + 1) * E; ++i)
      if (i < C) own += (double)cf_exp(mz[(unsigned)ms[i]], mx, a.inv_t);
    dsum[tid] = own;
    __syncthreads();
    const int B = TPR < CF_SCAN_BLOCK ? TPR : CF_SCAN_BLOCK;
    const int blk0 = tid & ~(B - 1);
    double pre = 0.0;
    for (int q = blk0; q < tid; ++q) pre += dsum[q];
    if ((tid & (B - 1)) == B - 1) bsum[tid / B] = pre + own;
    __syncthreads();
    const int gb0 = (seg * TPR) / B, gbn = TPR / B;
    double blocks_before = 0.0, sum = 0.0;
    for (int q = 0; q < gbn; ++q) {
      if (gb0 + q == tid / B) blocks_before = sum;
      sum += bsum[gb0 + q];
    }
    double ahead = blocks_before + pre;
    const float u = live && a.u ? a.u[r] : 1.0f;
    const bool all = a.qhat == INFINITY;
    for (int i = t * E; i < (t + 1) * E; ++i)
      if (i < C) {
        const unsigned c = (unsigned)ms[i];                  // c < C: a real pair
        const double e = (double)cf_exp(mz[c], mx, a.inv_t);
        const float s = cf_score(a.method, e, ahead, sum, i + 1, u, a.lam, a.k_reg);
        mf[c] = all || s <= a.qhat;
        ahead += e;
      }
    __syncthreads();
    int cnt = 0;
    for (int w = t; w < W; w += TPR) {
      uint32_t bits = 0;
      for (int k = 0; k < 32; ++k) {
        const int c = w * 32 + k;
        if (c < C) bits |= (uint32_t)mf[c] << k;
      }
      cnt += __popc(bits);
      if (live && a.members) a.members[r * W + w] = bits;
    }
    scnt[tid] = cnt;
    __syncthreads();
    if (t == 0 && live) {
      const int nw = W < TPR ? W : TPR;
      int size = 0;
      for (int q = 0; q < nw; ++q) size += scnt[seg * TPR + q];
      a.size[r] = size;
      if (a.covered) {
        const long long lb = cf_label(a.labels, a.labels_i64, r);
        a.covered[r] = lb >= 0 && lb < C ? mf[lb] : 0;
      }
    }
    __syncthreads();                                         // (the next batch overwrites the row's LDS)
  }
}

// ---- the host side
int64_t cf_rows_per_wg(int64_t n, int64_t ld) {
  int64_t least = 16384 / ld;                                // a workgroup reads 64 KB or more
  least = least < 4 ? 4 : least > 256 ? 256 : least;
  const int64_t spread = (n + CF_MAX_BLOCKS - 1) / CF_MAX_BLOCKS;
  return least > spread ? least : spread;
}

template <bool VEC>
int cf_scores_launch(const CfArgs& a, unsigned grid, hipStream_t st) {
  if (a.C > CF_REG_MAX_C) { k_conformal_scores_wide<VEC><<<grid, CF_THREADS, 0, st>>>(a); UVC_CHECK_LAUNCH(); return UVC_OK; }
  int lpr = 1, nu = 1;
  while (lpr < 64 && lpr * 4 < a.C) lpr <<= 1;
  while (lpr * nu * 4 < a.C) nu <<= 1;
#define UVC_CF_CASE(L, N) \
  if (lpr == L && nu == N) { k_conformal_scores_rows<L, N, VEC><<<grid, CF_THREADS, 0, st>>>(a); UVC_CHECK_LAUNCH(); return UVC_OK; }
  UVC_CF_CASE(1, 1) UVC_CF_CASE(2, 1) UVC_CF_CASE(4, 1) UVC_CF_CASE(8, 1) UVC_CF_CASE(16, 1) UVC_CF_CASE(32, 1)
  UVC_CF_CASE(64, 1) UVC_CF_CASE(64, 2) UVC_CF_CASE(64, 4) UVC_CF_CASE(64, 8)
#undef UVC_CF_CASE
  return uvc_set_error_msg(UVC_ERR_ARG, "uvc_conformal_scores: row plan");
}

int cf_common(const char* who, const uvc_conformal_args* a, bool sets, CfArgs* k) {
  static thread_local char msg[200];
  auto refuse = [&](const char* what, int code = UVC_ERR_ARG) { snprintf(msg, sizeof msg, "%s: %s", who, what); return uvc_set_error_msg(code, msg); };
  if (!a || !a->logits) return refuse("null pointer");
  if (sets ? (!a->size || (!a->labels) != (!a->covered)) : (!a->labels || !a->scores || !a->counts))
    return refuse(sets ? "null pointer (size; labels and covered go together)" : "null pointer");
  if (a->n < 1 || a->n > 0x7fffffffll) return refuse("n must lie in [1, 2^31)");
  if (a->C < 1) return refuse("C must be at least 1");
  if (a->ld < a->C || a->ld > 0x7fffffffll) return refuse("C <= ld < 2^31");
  if (a->method != UVC_CONFORMAL_LAC && a->method != UVC_CONFORMAL_APS && a->method != UVC_CONFORMAL_RAPS) return refuse("method must be UVC_CONFORMAL_LAC, _APS or _RAPS");
  if (!(a->inv_temperature > 0.f) || !std::isfinite(a->inv_temperature)) return refuse("the temperature must be positive and finite");
  if (!(a->lam >= 0.f) || !std::isfinite(a->lam)) return refuse("lam must be non-negative and finite");
  if (a->k_reg < 0) return refuse("k_reg must be non-negative");
  if (sets && a->qhat != a->qhat) return refuse("qhat is NaN");
  const uintptr_t four = (uintptr_t)a->logits | (uintptr_t)a->u | (sets ? (uintptr_t)a->size | (uintptr_t)a->members : (uintptr_t)a->scores);
  if ((four & 3) || (!sets && ((uintptr_t)a->counts & 7)) || ((uintptr_t)a->labels & (a->labels_i64 ? 7 : 3)))
    return refuse("misaligned pointer (counts and int64 labels: 8 bytes; logits, u, scores, size, members and int32 labels: 4)");
  if (a->C > (sets ? CF_SETS_MAX_C : CF_MAX_C)) return refuse(sets ? "C must be at most 2048" : "C must be at most 65536", UVC_ERR_UNSUPPORTED);
  k->logits = a->logits; k->labels = a->labels; k->u = a->u;
  k->scores = a->scores; k->counts = (long long*)a->counts;
  k->size = a->size; k->covered = a->covered; k->members = a->members;
  k->n = a->n; k->ld = a->ld; k->rows_per_wg = cf_rows_per_wg(a->n, a->ld);
  k->C = a->C; k->labels_i64 = a->labels_i64 != 0; k->method = a->method; k->k_reg = a->k_reg;
  k->inv_t = a->inv_temperature; k->lam = a->lam; k->qhat = a->qhat;
  return UVC_OK;
}

}  // namespace

extern "C" int uvc_conformal_scores(const uvc_conformal_args* a, void* stream) {
  CfArgs k;
  if (const int rc = cf_common("uvc_conformal_scores", a, false, &k)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)((k.n + k.rows_per_wg - 1) / k.rows_per_wg);
  const bool vec = k.ld % 4 == 0 && ((uintptr_t)k.logits & 15) == 0;
  if (const int rc = vec ? cf_scores_launch<true>(k, grid, st) : cf_scores_launch<false>(k, grid, st)) return rc;
  k_conformal_count<<<1, 1024, 0, st>>>(k);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

extern "C" int uvc_conformal_sets(const uvc_conformal_args* a, void* stream) {
  CfArgs k;
  if (const int rc = cf_common("uvc_conformal_sets", a, true, &k)) return rc;
  int P = 2;
  while (P < k.C) P <<= 1;
  const int TPR = P / 2 < CF_THREADS ? P / 2 : CF_THREADS;
  const int64_t rows = CF_THREADS / TPR;
  const int64_t batches = (k.n + rows - 1) / rows;
  const unsigned grid = (unsigned)(batches < CF_MAX_BLOCKS ? batches : CF_MAX_BLOCKS);
  k_conformal_sets<<<grid, CF_THREADS, 0, (hipStream_t)stream>>>(k, P, TPR);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}
