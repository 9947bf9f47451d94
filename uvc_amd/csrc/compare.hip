// Two models on one split (python -m uvc_amd.compact_compare) for gfx950 (include/uvc_kernels.h):
//   uvc_logits_pair_stats  top-1, confidence, KL both ways, Jensen-Shannon, total variation, the label's NLL and four ranks of every row
//                          pair of two logit matrices, in ONE read of both.
// No atomics, one writer per output element, the same bits on a repeat, a row pair's result does not depend on the rows beside it, 64-bit
// row offsets, workgroup counts functions of the shape alone, plain vector stores.
//
// The row organisation is uvc_ood_logit_scores' (ood.hip) with two rows where that has one: up to 1024 valid columns a group of LPR lanes
// (1 .. 64, a power of two) holds BOTH rows in registers, NU units of 4 columns per lane and matrix -- one 16-byte load per unit --,
// workgroup w owns the row pairs [w R, (w + 1) R) and its 256 / LPR groups take them round robin, the next pair (and its label) loaded
// before the current one is worked on; beyond 1024 columns one workgroup takes a row pair in three passes (the second and third from
// cache).  All of a row is float32, in three steps:
//   1  the FIRST maximum m of either row (a lane's columns ascending, then the xor butterfly: the larger value, the lower column among
//      equals) -- the top-1 columns, which the two cross ranks need, are known from here on;
//   2  rest = sum over c != first of exp(z_c - m): S = 1 + rest (the first maximum's own term is exactly 1), L = log1p(rest), conf = 1 / S;
//   3  per column d = z - m, l = d - L, p = exp(d) / S (as exp(d) * conf), dl = l_a - l_b and
//        kl_ab += p_a dl,  kl_ba -= p_b dl,  tv += |p_a - p_b| / 2,  js += (p_a (l_a - l_m) + p_b (l_b - l_m)) / 2
//      with l_m = max(l_a, l_b) + log((1 + exp(-|dl|)) / 2)  (= max + log1p(exp(-|dl|)) - log 2, and exactly the max when dl = 0), a term
//      whose probability underflowed being 0 (0 log 0 = 0); and the four rank counts #{c : z_c > t or (z_c = t and c < k)} for (t, k) =
//      (za_y, y), (zb_y, y), (zb_top1a, top1a), (za_top1b, top1b) -- the four targets are read from the row (it is in cache) once the
//      label and the top-1 columns are known.
// Contraction is off in this file: a-side and b-side take the same operations in the same order, so two equal rows give 0 exactly.
#include <cstdio>
#include "common.h"
#include "../../include/uvc_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int PS_THREADS = 256;
constexpr int PS_WAVES = PS_THREADS / 64;
constexpr int PS_MAX_C = 65536;
constexpr int PS_REG_MAX_C = 1024;          // wider rows: one workgroup per row pair.  NU = 4 takes 155 VGPRs (3 waves / SIMD); NU = 8 would take
                                            // 253 (2 waves / SIMD) to hide the prefetch and the exp / log chains behind
constexpr int PS_MAX_BLOCKS = 2048;

struct PsArgs {
  const float* za; const float* zb; const void* labels;
  int32_t* top1_a; int32_t* top1_b; float* conf_a; float* conf_b; float* kl_ab; float* kl_ba; float* js; float* tv; float* nll_a; float* nll_b;
  int32_t* rank_a; int32_t* rank_b; int32_t* rank_b_top1a; int32_t* rank_a_top1b;
  int64_t n, lda, ldb, rows_per_wg;
  int C, labels_i64;
};

struct PsRow {                               // what step 3 needs of one row
  float m, L, inv;                           // first maximum, log S, 1 / S
  int first;
};

struct PsSums { float kab, kba, js, tv; };

__device__ __forceinline__ long long ps_label(const PsArgs& a, int64_t r) {
  if (!a.labels) return -1;
  return a.labels_i64 ? ((const long long*)a.labels)[r] : (long long)((const int32_t*)a.labels)[r];
}

__device__ __forceinline__ void ps_max(float v, int c, float& mx, int& first, int& bad) {
  bad |= v != v;
  if (v > mx) { mx = v; first = c; }                         // ascending columns, strictly greater: the first maximum
}

__device__ __forceinline__ void ps_merge(float om, int of, float& mx, int& first) {
  if (om > mx || (om == mx && of < first)) { mx = om; first = of; }
}

// exp and log on the hardware's exp2 / log2 (v_exp_f32, v_log_f32: 1 ulp of the float32 result); the argument's product with log2(e) rounds
// once more, |d| 2^-24 relative in a term that is at most exp(d).  The kernel is bound by these, not by bytes (README), so the library's
// range-checked expf / log1pf stay with the two per-ROW values (log1p(rest)).  ps_exp(0) = 1 and ps_log(1) = 0 exactly.
__device__ __forceinline__ float ps_exp(float d) { return __builtin_amdgcn_exp2f(d * 1.44269504088896340736f); }
__device__ __forceinline__ float ps_log(float x) { return __builtin_amdgcn_logf(x) * 0.69314718055994530942f; }

// step 3 of one column
__device__ __forceinline__ void ps_column(float va, float vb, int c, const PsRow& A, const PsRow& B, PsSums& s) {
  const float da = va - A.m, db = vb - B.m;
  const float ea = c == A.first ? 1.0f : ps_exp(da), eb = c == B.first ? 1.0f : ps_exp(db);
  const float pa = ea * A.inv, pb = eb * B.inv;
  const float la = da - A.L, lb = db - B.L;
  const float dl = la - lb;
  const float t = ps_log(0.5f + 0.5f * ps_exp(-fabsf(dl)));  // log((1 + exp(-|dl|)) / 2): the argument lies in [1/2, 1]
  const float lm = fmaxf(la, lb) + t;
  if (pa > 0.f) { s.kab += pa * dl; s.js += 0.5f * (pa * (la - lm)); }
  if (pb > 0.f) { s.kba += pb * (lb - la); s.js += 0.5f * (pb * (lb - lm)); }
  s.tv += 0.5f * fabsf(pa - pb);
}

__device__ __forceinline__ int ps_before(float v, int c, float t, int k) { return (v > t || (v == t && c < k)) ? 1 : 0; }

// lane 0 of the group / thread 0 of the workgroup: every wanted output of row r
__device__ __forceinline__ void ps_write(const PsArgs& a, int64_t r, bool bad, bool has_y, const PsRow& A, const PsRow& B, const PsSums& s, float zay,
                                         float zby, int ra, int rb, int rbt, int rat) {
  const float nan = __builtin_nanf("");
  if (a.top1_a) a.top1_a[r] = bad ? -1 : A.first;
  if (a.top1_b) a.top1_b[r] = bad ? -1 : B.first;
  if (a.conf_a) a.conf_a[r] = bad ? nan : A.inv;
  if (a.conf_b) a.conf_b[r] = bad ? nan : B.inv;
  if (a.kl_ab) a.kl_ab[r] = bad ? nan : s.kab;
  if (a.kl_ba) a.kl_ba[r] = bad ? nan : s.kba;
  if (a.js) a.js[r] = bad ? nan : fmaxf(s.js, 0.f);
  if (a.tv) a.tv[r] = bad ? nan : s.tv;
  if (a.nll_a) a.nll_a[r] = bad || !has_y ? nan : A.L - (zay - A.m);
  if (a.nll_b) a.nll_b[r] = bad || !has_y ? nan : B.L - (zby - B.m);
  if (a.rank_a) a.rank_a[r] = bad || !has_y ? -1 : ra;
  if (a.rank_b) a.rank_b[r] = bad || !has_y ? -1 : rb;
  if (a.rank_b_top1a) a.rank_b_top1a[r] = bad ? -1 : rbt;
  if (a.rank_a_top1b) a.rank_a_top1b[r] = bad ? -1 : rat;
}

template <int LPR, int NU, bool VEC>
__global__ __launch_bounds__(PS_THREADS) void k_pair_rows(PsArgs a) {
  constexpr int GROUPS = PS_THREADS / LPR;
  const int tid = threadIdx.x, g = tid & (LPR - 1), grp = tid / LPR;
  const int C = a.C;
  const int64_t wg0 = (int64_t)blockIdx.x * a.rows_per_wg;
  const int64_t wg1 = wg0 + a.rows_per_wg < a.n ? wg0 + a.rows_per_wg : a.n;

  auto load = [&](float (&v)[NU][4], const float* zr) {
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

  float za[NU][4], zb[NU][4], zan[NU][4], zbn[NU][4];
  long long y = -1, yn = -1;
  int64_t r = wg0 + grp;
  if (r < wg1) { load(za, a.za + r * a.lda); load(zb, a.zb + r * a.ldb); y = ps_label(a, r); }
  for (; r < wg1; r += GROUPS) {                             // (a group's lanes leave together: every shuffle partner is live)
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) { zan[u][j] = za[u][j]; zbn[u][j] = zb[u][j]; }
    if (r + GROUPS < wg1) { load(zan, a.za + (r + GROUPS) * a.lda); load(zbn, a.zb + (r + GROUPS) * a.ldb); yn = ps_label(a, r + GROUPS); }
    const float* ra_ = a.za + r * a.lda;
    const float* rb_ = a.zb + r * a.ldb;
    const bool has_y = y >= 0 && y < C;
    const int yc = has_y ? (int)y : 0;
    const float zay = ra_[yc], zby = rb_[yc];                // (column 0 stands in for a label that is not counted; never written)
    // 1: the first maxima
    PsRow A, B;
    A.m = B.m = -INFINITY;
    A.first = B.first = 0x7fffffff;
    int bad = 0;
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = (u * LPR + g) * 4 + j;
        if (c < C) { ps_max(za[u][j], c, A.m, A.first, bad); ps_max(zb[u][j], c, B.m, B.first, bad); }
      }
#pragma unroll
    for (int s = 1; s < LPR; s <<= 1) {
      const float oma = __shfl_xor(A.m, s, 64), omb = __shfl_xor(B.m, s, 64);
      const int ofa = __shfl_xor(A.first, s, 64), ofb = __shfl_xor(B.first, s, 64);
      bad |= __shfl_xor(bad, s, 64);
      ps_merge(oma, ofa, A.m, A.first);
      ps_merge(omb, ofb, B.m, B.first);
    }
    const int fa = A.first < C ? A.first : 0, fb = B.first < C ? B.first : 0;      // (a row of NaN has no maximum: its outputs are the NaN row's)
    const float zbt = rb_[fa], zat = ra_[fb];
    // 2: the sums
    float resta = 0.f, restb = 0.f;
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = (u * LPR + g) * 4 + j;
        if (c < C) {
          if (c != A.first) resta += ps_exp(za[u][j] - A.m);
          if (c != B.first) restb += ps_exp(zb[u][j] - B.m);
        }
      }
#pragma unroll
    for (int s = 1; s < LPR; s <<= 1) {
      resta += __shfl_xor(resta, s, 64);
      restb += __shfl_xor(restb, s, 64);
    }
    A.L = log1pf(resta); A.inv = 1.0f / (1.0f + resta);
    B.L = log1pf(restb); B.inv = 1.0f / (1.0f + restb);
    // 3: the divergences and the ranks (two counts of at most 1024 per integer)
    PsSums sm = {0.f, 0.f, 0.f, 0.f};
    int cy = 0, ct = 0;
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = (u * LPR + g) * 4 + j;
        if (c < C) {
          const float va = za[u][j], vb = zb[u][j];
          ps_column(va, vb, c, A, B, sm);
          cy += ps_before(va, c, zay, yc) + (ps_before(vb, c, zby, yc) << 16);
          ct += ps_before(vb, c, zbt, fa) + (ps_before(va, c, zat, fb) << 16);
        }
      }
#pragma unroll
    for (int s = 1; s < LPR; s <<= 1) {
      sm.kab += __shfl_xor(sm.kab, s, 64);
      sm.kba += __shfl_xor(sm.kba, s, 64);
      sm.js += __shfl_xor(sm.js, s, 64);
      sm.tv += __shfl_xor(sm.tv, s, 64);
      cy += __shfl_xor(cy, s, 64);
      ct += __shfl_xor(ct, s, 64);
    }
    if (g == 0) ps_write(a, r, bad != 0, has_y, A, B, sm, zay, zby, cy & 0xffff, cy >> 16, ct & 0xffff, ct >> 16);
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) { za[u][j] = zan[u][j]; zb[u][j] = zbn[u][j]; }
    y = yn;
  }
}

// beyond 1024 columns: workgroup = row pair, thread t the units t, t + 256, ... of 4 columns
template <typename T>
__device__ __forceinline__ T ps_wg_sum(T v, T* sv) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) v += __shfl_xor(v, s, 64);
  __syncthreads();                                           // (the readers of the call before are done)
  if ((threadIdx.x & 63) == 0) sv[threadIdx.x >> 6] = v;
  __syncthreads();
  v = sv[0];
#pragma unroll
  for (int w = 1; w < PS_WAVES; ++w) v += sv[w];
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(PS_THREADS) void k_pair_wide(PsArgs a) {
  __shared__ float sma[PS_WAVES], smb[PS_WAVES], sf[PS_WAVES];
  __shared__ int sfa[PS_WAVES], sfb[PS_WAVES], sbad[PS_WAVES], si[PS_WAVES];
  const int tid = threadIdx.x, C = a.C;
  const int nunits = (C + 3) / 4;
  const int64_t r = blockIdx.x;
  const float* ra_ = a.za + r * a.lda;
  const float* rb_ = a.zb + r * a.ldb;
  auto load4 = [&](const float* zr, int c0, float (&v)[4]) {
    if (VEC) {
      const f32x4 q = *(const f32x4*)(zr + c0);             // c0 < C <= ld, ld % 4 == 0
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = q[j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = c0 + j < C ? zr[c0 + j] : 0.f;
    }
  };
  const long long y = ps_label(a, r);
  const bool has_y = y >= 0 && y < C;
  const int yc = has_y ? (int)y : 0;
  const float zay = ra_[yc], zby = rb_[yc];
  PsRow A, B;
  A.m = B.m = -INFINITY;
  A.first = B.first = 0x7fffffff;
  int bad = 0;
  for (int u = tid; u < nunits; u += PS_THREADS) {
    float va[4], vb[4];
    load4(ra_, u * 4, va);
    load4(rb_, u * 4, vb);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = u * 4 + j;
      if (c < C) { ps_max(va[j], c, A.m, A.first, bad); ps_max(vb[j], c, B.m, B.first, bad); }
    }
  }
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const float oma = __shfl_xor(A.m, s, 64), omb = __shfl_xor(B.m, s, 64);
    const int ofa = __shfl_xor(A.first, s, 64), ofb = __shfl_xor(B.first, s, 64);
    bad |= __shfl_xor(bad, s, 64);
    ps_merge(oma, ofa, A.m, A.first);
    ps_merge(omb, ofb, B.m, B.first);
  }
  if ((tid & 63) == 0) { sma[tid >> 6] = A.m; sfa[tid >> 6] = A.first; smb[tid >> 6] = B.m; sfb[tid >> 6] = B.first; sbad[tid >> 6] = bad; }
  __syncthreads();
  A.m = sma[0]; A.first = sfa[0]; B.m = smb[0]; B.first = sfb[0]; bad = sbad[0];
#pragma unroll
  for (int w = 1; w < PS_WAVES; ++w) {
    bad |= sbad[w];
    ps_merge(sma[w], sfa[w], A.m, A.first);
    ps_merge(smb[w], sfb[w], B.m, B.first);
  }
  const int fa = A.first < C ? A.first : 0, fb = B.first < C ? B.first : 0;
  const float zbt = rb_[fa], zat = ra_[fb];
  float resta = 0.f, restb = 0.f;
  for (int u = tid; u < nunits; u += PS_THREADS) {
    float va[4], vb[4];
    load4(ra_, u * 4, va);
    load4(rb_, u * 4, vb);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = u * 4 + j;
      if (c < C) {
        if (c != A.first) resta += ps_exp(va[j] - A.m);
        if (c != B.first) restb += ps_exp(vb[j] - B.m);
      }
    }
  }
  resta = ps_wg_sum(resta, sf);
  restb = ps_wg_sum(restb, sf);
  A.L = log1pf(resta); A.inv = 1.0f / (1.0f + resta);
  B.L = log1pf(restb); B.inv = 1.0f / (1.0f + restb);
  PsSums sm = {0.f, 0.f, 0.f, 0.f};
  int ra = 0, rb = 0, rbt = 0, rat = 0;
  for (int u = tid; u < nunits; u += PS_THREADS) {
    float va[4], vb[4];
    load4(ra_, u * 4, va);
    load4(rb_, u * 4, vb);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = u * 4 + j;
      if (c < C) {
        ps_column(va[j], vb[j], c, A, B, sm);
        ra += ps_before(va[j], c, zay, yc);
        rb += ps_before(vb[j], c, zby, yc);
        rbt += ps_before(vb[j], c, zbt, fa);
        rat += ps_before(va[j], c, zat, fb);
      }
    }
  }
  sm.kab = ps_wg_sum(sm.kab, sf);
  sm.kba = ps_wg_sum(sm.kba, sf);
  sm.js = ps_wg_sum(sm.js, sf);
  sm.tv = ps_wg_sum(sm.tv, sf);
  ra = ps_wg_sum(ra, si);
  rb = ps_wg_sum(rb, si);
  rbt = ps_wg_sum(rbt, si);
  rat = ps_wg_sum(rat, si);
  if (tid == 0) ps_write(a, r, bad != 0, has_y, A, B, sm, zay, zby, ra, rb, rbt, rat);
}

int64_t ps_rows_per_wg(int64_t n, int64_t ld2) {
  int64_t least = 16384 / ld2;                               // a workgroup reads 64 KB or more
  least = least < 4 ? 4 : least > 256 ? 256 : least;
  const int64_t spread = (n + PS_MAX_BLOCKS - 1) / PS_MAX_BLOCKS;
  return least > spread ? least : spread;
}

template <bool VEC>
int ps_launch(PsArgs& a, hipStream_t st) {
  if (a.C > PS_REG_MAX_C) { k_pair_wide<VEC><<<(unsigned)a.n, PS_THREADS, 0, st>>>(a); UVC_CHECK_LAUNCH(); return UVC_OK; }
  a.rows_per_wg = ps_rows_per_wg(a.n, a.lda + a.ldb);
  const unsigned grid = (unsigned)((a.n + a.rows_per_wg - 1) / a.rows_per_wg);
  int lpr = 1, nu = 1;
  while (lpr < 64 && lpr * 4 < a.C) lpr <<= 1;
  while (lpr * nu * 4 < a.C) nu <<= 1;
#define UVC_PS_CASE(L, N) \
  if (lpr == L && nu == N) { k_pair_rows<L, N, VEC><<<grid, PS_THREADS, 0, st>>>(a); UVC_CHECK_LAUNCH(); return UVC_OK; }
  UVC_PS_CASE(1, 1) UVC_PS_CASE(2, 1) UVC_PS_CASE(4, 1) UVC_PS_CASE(8, 1) UVC_PS_CASE(16, 1) UVC_PS_CASE(32, 1)
  UVC_PS_CASE(64, 1) UVC_PS_CASE(64, 2) UVC_PS_CASE(64, 4)
#undef UVC_PS_CASE
  return uvc_set_error_msg(UVC_ERR_ARG, "uvc_logits_pair_stats: row plan");
}

int ps_refuse(const char* what, int code = UVC_ERR_ARG) {
  static thread_local char msg[200];
  snprintf(msg, sizeof msg, "uvc_logits_pair_stats: %s", what);
  return uvc_set_error_msg(code, msg);
}

}  // namespace

extern "C" int uvc_logits_pair_stats(const uvc_pair_stats_args* p, void* stream) {
  if (!p) return ps_refuse("null arguments");
  if (!p->za || !p->zb) return ps_refuse("null pointer");
  if (p->n < 1 || p->n > 0x7fffffffll) return ps_refuse("n must lie in [1, 2^31)");
  if (p->C < 1) return ps_refuse("C must be at least 1");
  if (p->C > PS_MAX_C) return ps_refuse("C must be at most 65536", UVC_ERR_UNSUPPORTED);
  if (p->lda < p->C || p->ldb < p->C || p->lda > 0x7fffffffll || p->ldb > 0x7fffffffll) return ps_refuse("C <= lda, ldb < 2^31");
  const void* outs[14] = {p->top1_a, p->top1_b, p->conf_a, p->conf_b, p->kl_ab, p->kl_ba, p->js, p->tv, p->nll_a, p->nll_b,
                          p->rank_a, p->rank_b, p->rank_b_top1a, p->rank_a_top1b};
  uintptr_t bits = (uintptr_t)p->za | (uintptr_t)p->zb, any = 0;
  for (const void* o : outs) { bits |= (uintptr_t)o; any |= (uintptr_t)o; }
  if (!any) return ps_refuse("no output");
  if ((bits & 3) || ((uintptr_t)p->labels & (p->labels_i64 ? 7 : 3))) return ps_refuse("misaligned pointer");
  PsArgs a;
  a.za = p->za; a.zb = p->zb; a.labels = p->labels;
  a.top1_a = p->top1_a; a.top1_b = p->top1_b; a.conf_a = p->conf_a; a.conf_b = p->conf_b; a.kl_ab = p->kl_ab; a.kl_ba = p->kl_ba; a.js = p->js;
  a.tv = p->tv; a.nll_a = p->nll_a; a.nll_b = p->nll_b; a.rank_a = p->rank_a; a.rank_b = p->rank_b; a.rank_b_top1a = p->rank_b_top1a;
  a.rank_a_top1b = p->rank_a_top1b;
  a.n = p->n; a.lda = p->lda; a.ldb = p->ldb; a.rows_per_wg = 1; a.C = p->C; a.labels_i64 = p->labels_i64 != 0;
  const bool vec = p->lda % 4 == 0 && p->ldb % 4 == 0 && (((uintptr_t)p->za | (uintptr_t)p->zb) & 15) == 0;
  return vec ? ps_launch<true>(a, (hipStream_t)stream) : ps_launch<false>(a, (hipStream_t)stream);
}

extern "C" int uvc_logits_pair_stats_reg_max(void) { return PS_REG_MAX_C; }
