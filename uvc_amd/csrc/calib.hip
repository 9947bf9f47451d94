// Calibration of a logits bank (python -m uvc_amd.compact_calibrate) for gfx950: uvc_calib_eval, the negative log-likelihood of the affine map
// z'_c = scale_c z_c + shift_c of the logits (temperature scaling: one scale, no shift; vector scaling: one of each per class) with its gradient,
// and uvc_calib_stats, the reliability histogram of the same z' (include/uvc_kernels.h).
//
// Both are ONE pass over the logits and write nothing of size [n, C].  Workgroup w owns the rows [w R, (w + 1) R) with R a function of (n, ld)
// alone (uvc_calib_blocks).  Up to 2048 classes a group of LPR lanes (1 .. 64, a power of two) holds a row in registers, NU units of 4 columns
// per lane -- one 16-byte load per unit -- and the 256 / LPR groups of a workgroup split its rows into contiguous runs: a lane owns the same columns
// for every row of its run, so the column sums of g = softmax(z') - onehot and of g z stay in its registers, in ascending row order, and the
// groups' sums are added in ascending group order through LDS at the end: one partial [2 Cp] per workgroup.  The next row is loaded before the
// current one is worked on.  With one scale and no shift no column sum is wanted and the kernel is compiled without them (128 VGPRs, not 228).  Beyond 2048 classes a workgroup takes one row at a time in three passes (the second and third from cache) and
// keeps its column sums in its own partial in memory, every column by the thread that owns it.  A second launch adds the partials over the
// workgroups in ascending order in float64 and divides by m.  No atomics, one writer per element in every launch, the same bits on a repeat.
//
// Arithmetic: z' is formed in float64 (one fma on the float32 inputs) and z' - max is rounded to float32 once, so the exponent carries no rounding
// of z' itself -- at logits of magnitude 3e4 a float32 z' would be off by 2e-3; the maximum is the FIRST maximum of that float64 z'.  Everything
// else is float32 as in uvc_softmax_xent_grad (probe.hip): the sum leaves out the first maximum's own term, exactly 1 (the loss is log1p of the
// rest), a lane sums its columns in ascending order, the group then runs the xor butterfly, and p - 1 at the label is taken as minus the other
// columns' share from p = 1/2 up.  The temperature gradient sum_c g_c z_c of a row is sum_c p_c (z_c - z_ref) - (z_y - z_ref) with z_ref the
// logit at the first maximum: sum_c g_c = 0, and nothing of the size of the logits cancels.
#include <cstdio>
#include "common.h"
#include "../../include/uvc_kernels.h"

namespace {

constexpr int CAL_THREADS = 256;
constexpr int CAL_WAVES = CAL_THREADS / 64;
constexpr int CAL_MAX_C = 65536;
constexpr int CAL_REG_MAX_C = 2048;        // wider rows: one workgroup per row
constexpr int CAL_MAX_BLOCKS = 1024;
constexpr int CAL_MAX_BINS = 64;

struct ScPart { double loss, tsum; long long hits, m; };
struct StPart { long long count[CAL_MAX_BINS], hit[CAL_MAX_BINS]; double conf[CAL_MAX_BINS]; double nll, brier; };

struct CalArgs {
  const float* logits; const void* labels; const float* scale; const float* shift;
  float* col_part;       // [blocks][2 Cp]: sum g, then sum g z (eval)
  ScPart* sc_part;       // [blocks] (eval)
  StPart* st_part;       // [blocks] (stats)
  int64_t n, ld, rows_per_wg;
  int C, Cp, scale_vec, labels_i64, bins;
};

__device__ __forceinline__ long long cal_label(const void* labels, int i64, int64_t r) {
  return i64 ? ((const long long*)labels)[r] : (long long)((const int32_t*)labels)[r];
}
__device__ __forceinline__ double cal_map(float a, float z, float d) { return __builtin_fma((double)a, (double)z, (double)d); }
__device__ __forceinline__ int cal_bin(float conf, int bins) {
  int b = (int)ceilf(conf * (float)bins) - 1;
  return b < 0 ? 0 : b >= bins ? bins - 1 : b;
}
// g at one column: p, or at the label p - 1 (from one half up: minus the other columns' share of the sum)
__device__ __forceinline__ float cal_g(float e, float inv, float rest, float sum, bool at_label, bool label_first) {
  const float p = e * inv;
  if (!at_label) return p;
  return p < 0.5f ? p - 1.0f : -(label_first ? rest : sum - e) * inv;
}

// ---- up to 2048 classes: LPR lanes hold a row, unit u of lane g covers columns (u * LPR + g) * 4 .. + 3
// COLSUM: the column sums of g and g z are wanted (a shift, or a scale per class); without them and without STATS the map is one scalar
template <int LPR, int NU, bool VEC, bool STATS, bool COLSUM>
__global__ __launch_bounds__(CAL_THREADS) void k_calib_rows(CalArgs a) {
  constexpr int GROUPS = CAL_THREADS / LPR;
  constexpr int COLS = LPR * NU * 4;
  constexpr bool UNI = !STATS && !COLSUM;
  __shared__ float sbuf[COLSUM ? GROUPS * COLS : 1];
  __shared__ double sdl[GROUPS], sdt[GROUPS];
  __shared__ int shit[GROUPS], sm[GROUPS];
  __shared__ float sconf[STATS ? GROUPS : 1], sbrier[STATS ? GROUPS : 1];
  const int tid = threadIdx.x, g = tid & (LPR - 1), grp = tid / LPR;
  const int C = a.C;
  const int64_t wg0 = (int64_t)blockIdx.x * a.rows_per_wg;
  const int64_t wg1 = wg0 + a.rows_per_wg < a.n ? wg0 + a.rows_per_wg : a.n;
  const int64_t k = (a.rows_per_wg + GROUPS - 1) / GROUPS;
  const int64_t r0 = wg0 + grp * k;
  const int64_t r1 = r0 + k < wg1 ? r0 + k : wg1;
  const bool has_shift = a.shift != nullptr;

  const float s0 = a.scale[0];
  float sa[NU][4], sh[NU][4];
#pragma unroll
  for (int u = 0; u < NU; ++u)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = (u * LPR + g) * 4 + j;
      sa[u][j] = UNI ? s0 : c < C ? a.scale[a.scale_vec ? c : 0] : 0.f;
      sh[u][j] = !UNI && has_shift && c < C ? a.shift[c] : 0.f;
    }
  float accg[NU][4], accz[NU][4];
#pragma unroll
  for (int u = 0; u < NU; ++u)
#pragma unroll
    for (int j = 0; j < 4; ++j) accg[u][j] = accz[u][j] = 0.f;
  double loss_acc = 0.0, t_acc = 0.0;
  int hit_acc = 0, m_acc = 0;
  // stats: thread b < bins owns bin b, thread 64 the loss, thread 65 the Brier score
  long long bin_count = 0, bin_hit = 0;
  double bin_sum = 0.0;

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
  for (int64_t it = 0; it < k; ++it) {
    const int64_t r = r0 + it;
    const bool valid = r < r1;
    if (!STATS && !valid) break;                             // (no barrier inside the loop without STATS)
    bool counted = false;
    int bin = -1, hit = 0;
    float conf = 0.f, nll = 0.f, brier = 0.f;
    if (valid) {
#pragma unroll
      for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) zn[u][j] = z[u][j];
      if (r + 1 < r1) load(zn, r + 1);
      const float* zr = a.logits + r * a.ld;
      const long long lb = cal_label(a.labels, a.labels_i64, r);
      counted = lb >= 0 && lb < C;
      if (counted) {
        double mx = -INFINITY;
        int first = 0x7fffffff;
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int c = (u * LPR + g) * 4 + j;
            const double zp = cal_map(sa[u][j], z[u][j], sh[u][j]);
            if (c < C && zp > mx) { mx = zp; first = c; }  // ascending columns, strictly greater: the lane's first maximum
          }
#pragma unroll
        for (int s = 1; s < LPR; s <<= 1) {
          const double om = __shfl_xor(mx, s, 64);
          const int of = __shfl_xor(first, s, 64);
          if (om > mx || (om == mx && of < first)) { mx = om; first = of; }
        }
        if (first >= C) first = 0;                           // (a row without a number: its results are NaN, its reads stay inside the row)
        const float zref = zr[first];
        float e[NU][4];
        float rest = 0.f, sez = 0.f, se2 = 0.f;
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int c = (u * LPR + g) * 4 + j;
            const float d = (float)(cal_map(sa[u][j], z[u][j], sh[u][j]) - mx);
            const float ev = c < C ? (c == first ? 1.0f : expf(d)) : 0.f;
            e[u][j] = ev;
            if (c < C && c != first) { rest += ev; sez = __builtin_fmaf(ev, z[u][j] - zref, sez); se2 = __builtin_fmaf(ev, ev, se2); }
          }
#pragma unroll
        for (int s = 1; s < LPR; s <<= 1) {
          rest += __shfl_xor(rest, s, 64);
          sez += __shfl_xor(sez, s, 64);
          if (STATS) se2 += __shfl_xor(se2, s, 64);
        }
        const float sum = 1.0f + rest, inv = 1.0f / sum;
        // the label's logit: read again by every lane of the group (one cached dword)
        const float zy = zr[lb];
        const float dy = (float)(cal_map(a.scale[a.scale_vec ? lb : 0], zy, has_shift ? a.shift[lb] : 0.f) - mx);
        const float rl = log1pf(rest) - dy;
        hit = first == (int)lb;
        if (STATS) {
          conf = inv;                                        // the first maximum's probability: its exponential is 1
          bin = cal_bin(conf, a.bins);
          nll = rl;
          const float py = ((int)lb == first ? 1.0f : expf(dy)) * inv;
          brier = __builtin_fmaf(1.0f + se2, inv * inv, 1.0f) - 2.0f * py;
        } else {
          loss_acc += (double)rl;
          t_acc += (double)(sez * inv - (zy - zref));
          hit_acc += hit;
          m_acc += 1;
          if constexpr (COLSUM) {
#pragma unroll
            for (int u = 0; u < NU; ++u)
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const int c = (u * LPR + g) * 4 + j;
                const float gv = c < C ? cal_g(e[u][j], inv, rest, sum, c == (int)lb, (int)lb == first) : 0.f;
                accg[u][j] += gv;
                accz[u][j] = __builtin_fmaf(gv, z[u][j], accz[u][j]);
              }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) z[u][j] = zn[u][j];
    }
    if (STATS) {
      if (g == 0) { sm[grp] = counted ? bin : -1; shit[grp] = hit; sconf[grp] = conf; sdl[grp] = (double)nll; sbrier[grp] = brier; }
      __syncthreads();
      if (tid < a.bins) {
        for (int w = 0; w < GROUPS; ++w)
          if (sm[w] == tid) { bin_count += 1; bin_hit += shit[w]; bin_sum += (double)sconf[w]; }
      } else if (tid == 64) {
        for (int w = 0; w < GROUPS; ++w)
          if (sm[w] >= 0) bin_sum += sdl[w];
      } else if (tid == 65) {
        for (int w = 0; w < GROUPS; ++w)
          if (sm[w] >= 0) bin_sum += (double)sbrier[w];
      }
      __syncthreads();
    }
  }

  if (STATS) {
    StPart* sp = a.st_part + blockIdx.x;
    if (tid < CAL_MAX_BINS) { sp->count[tid] = bin_count; sp->hit[tid] = bin_hit; sp->conf[tid] = tid < a.bins ? bin_sum : 0.0; }
    else if (tid == 64) sp->nll = bin_sum;
    else if (tid == 65) sp->brier = bin_sum;
    return;
  }
  // the groups' column sums, added in ascending group order
  float* part = a.col_part + (int64_t)blockIdx.x * 2 * a.Cp;
  for (int q = 0; COLSUM && q < 2; ++q) {
    if (q == 0 ? !has_shift : !a.scale_vec) continue;        // (uniform over the workgroup)
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) sbuf[grp * COLS + (u * LPR + g) * 4 + j] = q == 0 ? accg[u][j] : accz[u][j];
    __syncthreads();
    for (int col = tid; col < COLS && col < a.Cp; col += CAL_THREADS) {
      float s = 0.f;
      for (int w = 0; w < GROUPS; ++w) s += sbuf[w * COLS + col];
      part[q * a.Cp + col] = s;
    }
    __syncthreads();
  }
  if (g == 0) { sdl[grp] = loss_acc; sdt[grp] = t_acc; shit[grp] = hit_acc; sm[grp] = m_acc; }
  __syncthreads();
  if (tid == 0) {
    ScPart p = {0.0, 0.0, 0, 0};
    for (int w = 0; w < GROUPS; ++w) { p.loss += sdl[w]; p.tsum += sdt[w]; p.hits += shit[w]; p.m += sm[w]; }
    a.sc_part[blockIdx.x] = p;
  }
}

// ---- beyond 2048 classes: the workgroup takes one row at a time, thread t the units t, t + 256, ... of 4 columns
__device__ __forceinline__ float wg_sum(float v, float* sv) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) v += __shfl_xor(v, s, 64);
  __syncthreads();                                           // (the readers of the call before are done)
  if ((threadIdx.x & 63) == 0) sv[threadIdx.x >> 6] = v;
  __syncthreads();
  v = sv[0];
#pragma unroll
  for (int w = 1; w < CAL_WAVES; ++w) v += sv[w];
  return v;
}

template <bool VEC, bool STATS>
__global__ __launch_bounds__(CAL_THREADS) void k_calib_wide(CalArgs a) {
  __shared__ double smx[CAL_WAVES];
  __shared__ int sfi[CAL_WAVES];
  __shared__ float sv[CAL_WAVES];
  __shared__ long long sbc[STATS ? CAL_MAX_BINS : 1], sbh[STATS ? CAL_MAX_BINS : 1];
  __shared__ double sbs[STATS ? CAL_MAX_BINS : 1];
  const int tid = threadIdx.x, C = a.C;
  const int nunits = (C + 3) / 4;
  const int64_t wg0 = (int64_t)blockIdx.x * a.rows_per_wg;
  const int64_t wg1 = wg0 + a.rows_per_wg < a.n ? wg0 + a.rows_per_wg : a.n;
  const bool has_shift = a.shift != nullptr;
  const bool cols = !STATS && (has_shift || a.scale_vec);
  float* part = a.col_part + (int64_t)blockIdx.x * 2 * a.Cp;
  if (cols)
    for (int u = tid; u < nunits; u += CAL_THREADS)
      for (int j = 0; j < 4; ++j) part[u * 4 + j] = part[a.Cp + u * 4 + j] = 0.f;       // (u * 4 + j < Cp; each column by its owner)
  if (STATS && tid < CAL_MAX_BINS) { sbc[tid] = 0; sbh[tid] = 0; sbs[tid] = 0.0; }
  double loss_acc = 0.0, t_acc = 0.0;
  long long hit_acc = 0, m_acc = 0;
  double brier_acc = 0.0;

  for (int64_t r = wg0; r < wg1; ++r) {
    const long long lb = cal_label(a.labels, a.labels_i64, r);
    if (lb < 0 || lb >= C) continue;                         // (uniform over the workgroup)
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
    auto zmap = [&](int c, float zv) { return cal_map(a.scale[a.scale_vec ? c : 0], zv, has_shift ? a.shift[c] : 0.f); };
    double mx = -INFINITY;
    int first = 0x7fffffff;
    for (int u = tid; u < nunits; u += CAL_THREADS) {
      float v[4];
      load4(u * 4, v);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = u * 4 + j;
        if (c < C) {
          const double zp = zmap(c, v[j]);
          if (zp > mx) { mx = zp; first = c; }
        }
      }
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const double om = __shfl_xor(mx, s, 64);
      const int of = __shfl_xor(first, s, 64);
      if (om > mx || (om == mx && of < first)) { mx = om; first = of; }
    }
    __syncthreads();
    if ((tid & 63) == 0) { smx[tid >> 6] = mx; sfi[tid >> 6] = first; }
    __syncthreads();
    mx = smx[0]; first = sfi[0];
#pragma unroll
    for (int w = 1; w < CAL_WAVES; ++w)
      if (smx[w] > mx || (smx[w] == mx && sfi[w] < first)) { mx = smx[w]; first = sfi[w]; }
    if (first >= C) first = 0;
    const float zref = zr[first];
    float rest = 0.f, sez = 0.f, se2 = 0.f;
    for (int u = tid; u < nunits; u += CAL_THREADS) {
      float v[4];
      load4(u * 4, v);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = u * 4 + j;
        if (c < C && c != first) {
          const float ev = expf((float)(zmap(c, v[j]) - mx));
          rest += ev; sez = __builtin_fmaf(ev, v[j] - zref, sez); se2 = __builtin_fmaf(ev, ev, se2);
        }
      }
    }
    rest = wg_sum(rest, sv);
    sez = wg_sum(sez, sv);
    if (STATS) se2 = wg_sum(se2, sv);
    const float sum = 1.0f + rest, inv = 1.0f / sum;
    const float zy = zr[lb];
    const float dy = (float)(zmap((int)lb, zy) - mx);
    const float rl = log1pf(rest) - dy;
    const int hit = first == (int)lb;
    if (STATS) {
      if (tid == 0) {
        const int bin = cal_bin(inv, a.bins);
        const float py = ((int)lb == first ? 1.0f : expf(dy)) * inv;
        sbc[bin] += 1; sbh[bin] += hit; sbs[bin] += (double)inv;
        loss_acc += (double)rl;
        brier_acc += (double)(__builtin_fmaf(1.0f + se2, inv * inv, 1.0f) - 2.0f * py);
      }
      continue;
    }
    loss_acc += (double)rl;
    t_acc += (double)(sez * inv - (zy - zref));
    hit_acc += hit;
    m_acc += 1;
    if (cols)
      for (int u = tid; u < nunits; u += CAL_THREADS) {
        float v[4];
        load4(u * 4, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int c = u * 4 + j;
          if (c < C) {
            const float ev = c == first ? 1.0f : expf((float)(zmap(c, v[j]) - mx));
            const float gv = cal_g(ev, inv, rest, sum, c == (int)lb, (int)lb == first);
            if (has_shift) part[c] += gv;
            if (a.scale_vec) part[a.Cp + c] = __builtin_fmaf(gv, v[j], part[a.Cp + c]);
          }
        }
      }
  }
  if (STATS) {
    __syncthreads();
    StPart* sp = a.st_part + blockIdx.x;
    if (tid < CAL_MAX_BINS) { sp->count[tid] = sbc[tid]; sp->hit[tid] = sbh[tid]; sp->conf[tid] = sbs[tid]; }
    if (tid == 0) { sp->nll = loss_acc; sp->brier = brier_acc; }
    return;
  }
  if (tid == 0) {
    const ScPart p = {loss_acc, t_acc, hit_acc, m_acc};
    a.sc_part[blockIdx.x] = p;
  }
}

// ---- the second launch: the partials over the workgroups in ascending order, in float64, over m
struct FinArgs {
  const float* col_part; const ScPart* sc_part;
  double* F; float* dscale; float* dshift; long long* counts;
  int blocks, C, Cp, scale_vec, has_shift;
};

__global__ __launch_bounds__(CAL_THREADS) void k_calib_finish(FinArgs f) {
  __shared__ long long sm[CAL_THREADS], sh[CAL_THREADS];
  __shared__ double sl[CAL_THREADS], st[CAL_THREADS];
  const int tid = threadIdx.x;
  long long m = 0, h = 0;
  double l = 0.0, t = 0.0;
  for (int b = tid; b < f.blocks; b += CAL_THREADS) { m += f.sc_part[b].m; h += f.sc_part[b].hits; l += f.sc_part[b].loss; t += f.sc_part[b].tsum; }
  sm[tid] = m; sh[tid] = h; sl[tid] = l; st[tid] = t;
  __syncthreads();
  for (int s = CAL_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) { sm[tid] += sm[tid + s]; sh[tid] += sh[tid + s]; sl[tid] += sl[tid + s]; st[tid] += st[tid + s]; }
    __syncthreads();
  }
  m = sm[0];
  const double inv = m > 0 ? 1.0 / (double)m : 0.0;
  const int col = blockIdx.x * CAL_THREADS + tid;
  if (col < 2 * f.Cp) {
    const int q = col >= f.Cp, c = q ? col - f.Cp : col;
    if (c < f.C && (q ? f.scale_vec : f.has_shift)) {
      double s = 0.0;
#pragma unroll 8
      for (int b = 0; b < f.blocks; ++b) s += (double)f.col_part[(int64_t)b * 2 * f.Cp + col];
      (q ? f.dscale : f.dshift)[c] = (float)(s * inv);
    }
  }
  if (blockIdx.x == 0 && tid == 0) {
    f.F[0] = sl[0] * inv;
    f.counts[0] = sh[0];
    f.counts[1] = m;
    if (!f.scale_vec) f.dscale[0] = (float)(st[0] * inv);
  }
}

struct StatFinArgs {
  const StPart* st_part;
  long long* bin_count; double* bin_conf; long long* bin_hit; double* sums; long long* counts;
  int blocks, bins;
};

__global__ __launch_bounds__(CAL_THREADS) void k_calib_stats_finish(StatFinArgs f) {
  __shared__ long long sc[CAL_MAX_BINS], sh[CAL_MAX_BINS];
  const int tid = threadIdx.x;
  if (tid < CAL_MAX_BINS) {
    long long c = 0, h = 0;
    double s = 0.0;
    if (tid < f.bins)
      for (int b = 0; b < f.blocks; ++b) { c += f.st_part[b].count[tid]; h += f.st_part[b].hit[tid]; s += f.st_part[b].conf[tid]; }
    sc[tid] = c; sh[tid] = h;
    if (tid < f.bins) { f.bin_count[tid] = c; f.bin_hit[tid] = h; f.bin_conf[tid] = s; }
  } else if (tid == 64 || tid == 65) {
    double s = 0.0;
    for (int b = 0; b < f.blocks; ++b) s += tid == 64 ? f.st_part[b].nll : f.st_part[b].brier;
    f.sums[tid - 64] = s;
  }
  __syncthreads();
  if (tid == 0) {
    long long c = 0, h = 0;
    for (int b = 0; b < CAL_MAX_BINS; ++b) { c += sc[b]; h += sh[b]; }
    f.counts[0] = h;
    f.counts[1] = c;
  }
}

// ---- the host side
int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

int64_t rows_per_wg(int64_t n, int64_t ld) {
  int64_t least = 16384 / ld;                                // a workgroup reads 64 KB or more
  least = least < 4 ? 4 : least > 256 ? 256 : least;
  const int64_t spread = (n + CAL_MAX_BLOCKS - 1) / CAL_MAX_BLOCKS;
  return least > spread ? least : spread;
}
int64_t cal_blocks(int64_t n, int64_t ld) {
  const int64_t R = rows_per_wg(n, ld);
  return (n + R - 1) / R;
}

int cal_shape(const char* who, int64_t n, int64_t ld, int32_t C, int32_t bins, bool stats) {
  static thread_local char msg[160];
  const char* what = nullptr;
  int code = UVC_ERR_ARG;
  if (n < 1 || n > 0x7fffffffll) what = "n must lie in [1, 2^31)";
  else if (C < 1) what = "C must be at least 1";
  else if (C > CAL_MAX_C) { what = "C must be at most 65536"; code = UVC_ERR_UNSUPPORTED; }
  else if (ld < C || ld > 0x7fffffffll) what = "C <= ld < 2^31";
  else if (stats && (bins < 1 || bins > CAL_MAX_BINS)) what = "bins must lie in [1, 64]";
  if (!what) return UVC_OK;
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return uvc_set_error_msg(code, msg);
}

struct CalPlan { int64_t blocks, R, o_col, o_sc, bytes; int Cp; };

CalPlan cal_plan(int64_t n, int64_t ld, int32_t C, bool stats) {
  CalPlan p;
  p.R = rows_per_wg(n, ld);
  p.blocks = (n + p.R - 1) / p.R;
  p.Cp = (C + 3) / 4 * 4;
  int64_t o = 0;
  p.o_col = o; o += stats ? 0 : align256(p.blocks * 2 * p.Cp * 4);
  p.o_sc = o; o += align256(p.blocks * (int64_t)(stats ? sizeof(StPart) : sizeof(ScPart)));
  p.bytes = o;
  return p;
}

template <bool VEC, bool STATS>
int cal_launch(const CalArgs& a, unsigned grid, hipStream_t st) {
  if (a.C > CAL_REG_MAX_C) { k_calib_wide<VEC, STATS><<<grid, CAL_THREADS, 0, st>>>(a); UVC_CHECK_LAUNCH(); return UVC_OK; }
  const bool cols = !STATS && (a.shift != nullptr || a.scale_vec);
  int lpr = 1, nu = 1;
  while (lpr < 64 && lpr * 4 < a.C) lpr <<= 1;
  while (lpr * nu * 4 < a.C) nu <<= 1;
#define UVC_CAL_CASE(L, N) \
  if (lpr == L && nu == N) {                                                                                                 \
    if (cols) k_calib_rows<L, N, VEC, STATS, !STATS><<<grid, CAL_THREADS, 0, st>>>(a);                                       \
    else k_calib_rows<L, N, VEC, STATS, false><<<grid, CAL_THREADS, 0, st>>>(a);                                             \
    UVC_CHECK_LAUNCH();                                                                                                      \
    return UVC_OK;                                                                                                           \
  }
  UVC_CAL_CASE(1, 1) UVC_CAL_CASE(2, 1) UVC_CAL_CASE(4, 1) UVC_CAL_CASE(8, 1) UVC_CAL_CASE(16, 1) UVC_CAL_CASE(32, 1)
  UVC_CAL_CASE(64, 1) UVC_CAL_CASE(64, 2) UVC_CAL_CASE(64, 4) UVC_CAL_CASE(64, 8)
#undef UVC_CAL_CASE
  return uvc_set_error_msg(UVC_ERR_ARG, "uvc_calib: row plan");
}

int cal_common(const char* who, const uvc_calib_args* a, bool stats, CalArgs* k, CalPlan* p) {
  static thread_local char msg[200];
  auto refuse = [&](const char* what) { snprintf(msg, sizeof msg, "%s: %s", who, what); return uvc_set_error_msg(UVC_ERR_ARG, msg); };
  if (!a || !a->logits || !a->labels || !a->scale || !a->counts) return refuse("null pointer");
  if (stats ? (!a->bin_count || !a->bin_conf || !a->bin_hit || !a->sums) : (!a->F || !a->dscale)) return refuse("null pointer");
  if (!stats && a->shift && !a->dshift) return refuse("a shift needs dshift");
  if (const int rc = cal_shape(who, a->n, a->ld, a->C, a->bins, stats)) return rc;
  if (a->scale_len != 1 && a->scale_len != a->C) return refuse("scale_len must be 1 or C");
  const uintptr_t four = (uintptr_t)a->logits | (uintptr_t)a->scale | (uintptr_t)a->shift | (stats ? 0 : (uintptr_t)a->dscale | (uintptr_t)a->dshift);
  const uintptr_t eight = (uintptr_t)a->counts | (stats ? (uintptr_t)a->bin_count | (uintptr_t)a->bin_conf | (uintptr_t)a->bin_hit | (uintptr_t)a->sums : (uintptr_t)a->F);
  if ((four & 3) || (eight & 7) || ((uintptr_t)a->labels & (a->labels_i64 ? 7 : 3)) || ((uintptr_t)a->workspace & 15))
    return refuse("misaligned pointer (workspace: 16 bytes; F, counts, the bin arrays, sums and int64 labels: 8; the rest: 4)");
  *p = cal_plan(a->n, a->ld, a->C, stats);
  if (!a->workspace || a->workspace_bytes < p->bytes) return refuse("workspace too small (uvc_calib_workspace_bytes)");
  char* ws = (char*)a->workspace;
  k->logits = a->logits; k->labels = a->labels; k->scale = a->scale; k->shift = a->shift;
  k->col_part = (float*)(ws + p->o_col);
  k->sc_part = (ScPart*)(ws + p->o_sc);
  k->st_part = (StPart*)(ws + p->o_sc);
  k->n = a->n; k->ld = a->ld; k->rows_per_wg = p->R;
  k->C = a->C; k->Cp = p->Cp; k->scale_vec = a->scale_len == a->C && a->C > 1; k->labels_i64 = a->labels_i64 != 0; k->bins = a->bins;
  return UVC_OK;
}

bool cal_vec(const CalArgs& k) { return k.ld % 4 == 0 && ((uintptr_t)k.logits & 15) == 0; }

}  // namespace

extern "C" int uvc_calib_blocks(int64_t n, int32_t ld, int64_t* blocks) {
  if (!blocks || n < 1 || n > 0x7fffffffll || ld < 1) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_calib_blocks: 1 <= n < 2^31 and ld >= 1");
  *blocks = cal_blocks(n, ld);
  return UVC_OK;
}

extern "C" int uvc_calib_workspace_bytes(int64_t n, int32_t ld, int32_t C, int32_t bins, int64_t* bytes) {
  if (!bytes) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_calib_workspace_bytes: null pointer");
  if (const int rc = cal_shape("uvc_calib_workspace_bytes", n, ld, C, bins, bins != 0)) return rc;
  *bytes = cal_plan(n, ld, C, bins != 0).bytes;
  return UVC_OK;
}

extern "C" int uvc_calib_eval(const uvc_calib_args* a, void* stream) {
  CalArgs k;
  CalPlan p;
  if (const int rc = cal_common("uvc_calib_eval", a, false, &k, &p)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)p.blocks;
  if (const int rc = cal_vec(k) ? cal_launch<true, false>(k, grid, st) : cal_launch<false, false>(k, grid, st)) return rc;
  FinArgs f;
  f.col_part = k.col_part; f.sc_part = k.sc_part; f.F = a->F; f.dscale = a->dscale; f.dshift = a->dshift; f.counts = (long long*)a->counts;
  f.blocks = (int)p.blocks; f.C = a->C; f.Cp = p.Cp; f.scale_vec = k.scale_vec; f.has_shift = a->shift != nullptr;
  const int work = f.scale_vec || f.has_shift ? 2 * p.Cp : 1;
  k_calib_finish<<<(work + CAL_THREADS - 1) / CAL_THREADS, CAL_THREADS, 0, st>>>(f);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

extern "C" int uvc_calib_stats(const uvc_calib_args* a, void* stream) {
  CalArgs k;
  CalPlan p;
  if (const int rc = cal_common("uvc_calib_stats", a, true, &k, &p)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)p.blocks;
  if (const int rc = cal_vec(k) ? cal_launch<true, true>(k, grid, st) : cal_launch<false, true>(k, grid, st)) return rc;
  StatFinArgs f;
  f.st_part = k.st_part; f.bin_count = (long long*)a->bin_count; f.bin_conf = a->bin_conf; f.bin_hit = (long long*)a->bin_hit; f.sums = a->sums;
  f.counts = (long long*)a->counts; f.blocks = (int)p.blocks; f.bins = a->bins;
  k_calib_stats_finish<<<1, CAL_THREADS, 0, st>>>(f);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}
