// Two-model cascades (python -m uvc_amd.compact_cascade) for gfx950 (include/uvc_kernels.h): the small model answers the rows it is sure
// of, the rest go to the large model.
//   uvc_cascade_decide   the confidence score of every logits row (msp, margin or 1 - normalised entropy of softmax(z / T)), its first
//                        maximum and defer = !(score >= tau);
//   uvc_cascade_compact  the deferred rows in ascending order (idx), every row's place among them (pos) and their number (count);
//   uvc_cascade_gather   the deferred images' patch rows, packed into a dense batch for the large model;
//   uvc_cascade_merge    out[b] = pos[b] >= 0 ? z_large[pos[b]] : z_small[b], and which model answered.
// No atomics, one writer per output element in every launch, the same bits on a repeat, a row's result does not depend on the rows beside
// it, 64-bit row offsets, workgroup counts functions of the shape alone, 16-byte accesses where pointer and stride allow and element by
// element otherwise -- the same values in the same order either way.
//
// decide: one wave per row, lane l the units l, l + 64, ... of 4 columns, in ascending order.  First pass: the lane's largest and second
// largest value (counted with multiplicity: a maximum that appears twice is also the second largest) and the column of its first maximum,
// then the xor butterfly: the larger value, the lower column among equals.  Second pass (from cache): d_c = z_c - m, q_c = d_c / T and
// e_c = expf(q_c) in float32, S = sum e_c and sum e_c q_c in float64 -- a lane's columns ascending, then the butterfly --; the maximum's
// own term is expf(0) = 1.  Then, in float64 and rounded to float32 once:
//   msp = 1 / S,   margin = (1 - expf((m2 - m) / T)) / S,   entropy score = 1 + ((sum e_c q_c) / S - log S) / log C  (1 at C = 1),
// a term whose exponential is 0 adding nothing (0 log 0 = 0).  A NaN in a valid column (or a row without a maximum: every column -inf)
// gives score NaN, top1 -1, defer 1.
//
// compact: workgroup w owns the rows [2048 w, 2048 w + 2048), thread t eight consecutive ones.  k_cascade_count leaves every workgroup's
// number of deferred rows, k_cascade_scan (one workgroup) turns them into exclusive offsets in place and writes the total, and
// k_cascade_write repeats the count, scans the threads' counts inside the workgroup and writes idx and pos.  The order is a function of
// defer alone.
#include <cmath>
#include "common.h"
#include "../../include/uvc_kernels.h"

namespace {

constexpr int CS_MAX_C = 65536;
constexpr int CS_PER = 8;                   // rows of defer per thread
constexpr int CS_TILE = 256 * CS_PER;       // and per workgroup
constexpr int CS_CHUNK = 256 * 16 * 4;      // bytes of a gathered row per workgroup

// ---------------------------------------------------------------------------------------------------------------- decide
__device__ __forceinline__ void cs_unit(const float* z, int c0, int C, int vec, float (&v)[4]) {
  if (vec && c0 + 4 <= C) {
    const f32x4 q = *(const f32x4*)(z + c0);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = q[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = c0 + j < C ? z[c0 + j] : 0.f;
  }
}

__global__ __launch_bounds__(256) void k_cascade_decide(const float* __restrict__ logits, int64_t n, int64_t ld, int C, float T, int kind, float tau,
                                                        int vec, float* __restrict__ score, int32_t* __restrict__ top1,
                                                        int32_t* __restrict__ defer) {
  const int l = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;                                  // (wave-uniform)
  const float* z = logits + row * ld;
  const int units = (C + 3) >> 2;
  float m1 = -INFINITY, m2 = -INFINITY;
  int first = 0x7fffffff, bad = 0;
  for (int u = l; u < units; u += 64) {
    float v[4];
    cs_unit(z, u * 4, C, vec, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = u * 4 + j;
      const float x = v[j];
      if (c < C) {
        bad |= x != x;
        if (x > m1) { m2 = m1; m1 = x; first = c; }      // ascending columns, strictly greater: the lane's first maximum
        else if (x > m2) m2 = x;
      }
    }
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const float o1 = __shfl_xor(m1, s, 64), o2 = __shfl_xor(m2, s, 64);
    const int of = __shfl_xor(first, s, 64);
    bad |= __shfl_xor(bad, s, 64);
    const float second = fmaxf(fminf(m1, o1), fmaxf(m2, o2));
    if (o1 > m1 || (o1 == m1 && of < first)) { m1 = o1; first = of; }
    m2 = second;
  }
  if (first >= C) bad = 1;                               // no maximum: every valid column is -inf
  double S = 0.0, sed = 0.0;
  if (!bad) {                                            // (wave-uniform)
    for (int u = l; u < units; u += 64) {
      float v[4];
      cs_unit(z, u * 4, C, vec, v);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (u * 4 + j < C) {
          const float q = (v[j] - m1) / T;
          const float e = expf(q);
          S += (double)e;
          if (kind == 2 && e > 0.f) sed += (double)e * (double)q;
        }
      }
    }
    S = wave_sum_f64(S);
    if (kind == 2) sed = wave_sum_f64(sed);
  }
  if (l != 0) return;
  float sc = __builtin_nanf("");
  if (!bad) {
    if (kind == 0) sc = (float)(1.0 / S);
    else if (kind == 1) sc = (float)((1.0 - (double)expf((m2 - m1) / T)) / S);
    else sc = C == 1 ? 1.0f : (float)(1.0 + (sed / S - log(S)) / log((double)C));
  }
  if (score) score[row] = sc;
  if (top1) top1[row] = bad ? -1 : first;
  if (defer) defer[row] = !(sc >= tau);
}

// ---------------------------------------------------------------------------------------------------------------- compact
__device__ __forceinline__ int cs_flags(const int32_t* __restrict__ defer, int64_t r0, int64_t n, int vec, int (&f)[CS_PER]) {
  int cnt = 0;
#pragma unroll
  for (int h = 0; h < CS_PER / 4; ++h) {
    const int64_t b = r0 + 4 * h;
    if (vec && b + 4 <= n) {
      const u32x4 q = *(const u32x4*)(defer + b);
#pragma unroll
      for (int j = 0; j < 4; ++j) f[4 * h + j] = q[j] != 0u;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) f[4 * h + j] = b + j < n ? defer[b + j] != 0 : 0;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) cnt += f[4 * h + j];
  }
  return cnt;
}

// the exclusive prefix of cnt over the workgroup's 256 threads, and their total; sm: 4 ints of LDS
__device__ __forceinline__ int cs_block_excl(int cnt, int* sm, int& total) {
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (l >= o) inc += t;
  }
  if (l == 63) sm[w] = inc;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int s = sm[i];
    if (i < w) base += s;
    total += s;
  }
  return base + inc - cnt;
}

__global__ __launch_bounds__(256) void k_cascade_count(const int32_t* __restrict__ defer, int64_t n, int vec, int32_t* __restrict__ counts) {
  __shared__ int sm[4];
  int f[CS_PER], total;
  const int cnt = cs_flags(defer, (int64_t)blockIdx.x * CS_TILE + (int64_t)threadIdx.x * CS_PER, n, vec, f);
  cs_block_excl(cnt, sm, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_cascade_scan(int32_t* __restrict__ counts, int nb, int32_t* __restrict__ count) {
  __shared__ int sm[4];
  int carry = 0;
  for (int i0 = 0; i0 < nb; i0 += 256) {
    const int i = i0 + (int)threadIdx.x;
    const int v = i < nb ? counts[i] : 0;
    int total;
    const int ex = cs_block_excl(v, sm, total);
    if (i < nb) counts[i] = carry + ex;
    carry += total;
    __syncthreads();                                     // sm is written again in the next round
  }
  if (threadIdx.x == 0) count[0] = carry;
}

__global__ __launch_bounds__(256) void k_cascade_write(const int32_t* __restrict__ defer, int64_t n, int vec, int vec_pos,
                                                       const int32_t* __restrict__ offsets, int32_t* __restrict__ idx, int32_t* __restrict__ pos) {
  __shared__ int sm[4];
  int f[CS_PER], total;
  const int64_t r0 = (int64_t)blockIdx.x * CS_TILE + (int64_t)threadIdx.x * CS_PER;
  const int cnt = cs_flags(defer, r0, n, vec, f);
  int place = offsets[blockIdx.x] + cs_block_excl(cnt, sm, total);
  int32_t p[CS_PER];
#pragma unroll
  for (int j = 0; j < CS_PER; ++j) {
    p[j] = f[j] ? place : -1;
    if (f[j]) {                                          // (f is 0 past n)
      if (idx) idx[place] = (int32_t)(r0 + j);
      ++place;
    }
  }
  if (!pos) return;
#pragma unroll
  for (int h = 0; h < CS_PER / 4; ++h) {
    const int64_t b = r0 + 4 * h;
    if (vec_pos && b + 4 <= n) {
      const u32x4 q = {(uint32_t)p[4 * h], (uint32_t)p[4 * h + 1], (uint32_t)p[4 * h + 2], (uint32_t)p[4 * h + 3]};
      *(u32x4*)(pos + b) = q;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (b + j < n) pos[b + j] = p[4 * h + j];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- gather
struct GatherArgs {
  const char* src; char* dst; const int32_t* idx;
  int64_t n, rpi, row_bytes, lds_bytes, ldd_bytes, chunks;
  int esz, vec;
};

__device__ __forceinline__ void cs_copy_elem(const char* sp, char* dp, int64_t b, int esz, bool ok) {
  if (esz == 4) *(uint32_t*)(dp + b) = ok ? *(const uint32_t*)(sp + b) : 0u;
  else *(uint16_t*)(dp + b) = ok ? *(const uint16_t*)(sp + b) : (uint16_t)0;
}

// workgroup = (destination row, chunk of 16 384 bytes of it)
__global__ __launch_bounds__(256) void k_cascade_gather(GatherArgs a) {
  const int64_t bid = blockIdx.x;
  const int64_t row = bid / a.chunks, ch = bid - row * a.chunks;
  const int64_t item = row / a.rpi, sub = row - item * a.rpi;
  const int64_t s = a.idx[item];
  const bool ok = s >= 0 && s < a.n;                     // (workgroup-uniform) an index outside [0, n): an item of +0, nothing is read
  const char* sp = a.src + (ok ? (s * a.rpi + sub) * a.lds_bytes : 0);
  char* dp = a.dst + row * a.ldd_bytes;
  const int64_t b0 = ch * CS_CHUNK;
  const int64_t b1 = b0 + CS_CHUNK < a.row_bytes ? b0 + CS_CHUNK : a.row_bytes;
  if (a.vec) {
    for (int64_t b = b0 + (int64_t)threadIdx.x * 16; b < b1; b += 256 * 16) {
      if (b + 16 <= b1) {
        u32x4 v = {0u, 0u, 0u, 0u};
        if (ok) v = *(const u32x4*)(sp + b);
        *(u32x4*)(dp + b) = v;
      } else {
        for (int64_t e = b; e < b1; e += a.esz) cs_copy_elem(sp, dp, e, a.esz, ok);
      }
    }
  } else {
    for (int64_t b = b0 + (int64_t)threadIdx.x * a.esz; b < b1; b += 256 * a.esz) cs_copy_elem(sp, dp, b, a.esz, ok);
  }
}

// ---------------------------------------------------------------------------------------------------------------- merge
// one wave per row; bits are copied
__global__ __launch_bounds__(256) void k_cascade_merge(const uint32_t* __restrict__ zs, int64_t lds, const uint32_t* __restrict__ zl, int64_t ldl, int64_t m,
                                                       const int32_t* __restrict__ pos, int64_t n, int C, int vec, uint32_t* __restrict__ out, int64_t ldo,
                                                       int32_t* __restrict__ source) {
  const int l = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const int64_t p = pos[row];
  const int src = p < 0 ? 0 : (p < m ? 1 : -1);          // (wave-uniform) -1: a place past the large model's rows, a row of NaN
  const uint32_t* z = src == 0 ? zs + row * lds : (src == 1 ? zl + p * ldl : nullptr);
  uint32_t* o = out + row * ldo;
  const uint32_t nan = 0x7fc00000u;
  const int units = (C + 3) >> 2;
  for (int u = l; u < units; u += 64) {
    const int c0 = u * 4;
    if (vec && c0 + 4 <= C) {
      u32x4 v = {nan, nan, nan, nan};
      if (z) v = *(const u32x4*)(z + c0);
      *(u32x4*)(o + c0) = v;
    } else {
      for (int c = c0; c < C && c < c0 + 4; ++c) o[c] = z ? z[c] : nan;
    }
  }
  if (l == 0 && source) source[row] = src;
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool al4(const void* p) { return ((uintptr_t)p & 3) == 0; }

}  // namespace

extern "C" int uvc_cascade_decide(const float* logits, int64_t n, int64_t ld, int32_t C, float T, int32_t kind, float tau, float* score, int32_t* top1,
                                  int32_t* defer, void* stream) {
  if (!logits || (!score && !top1 && !defer)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_cascade_decide: logits and at least one output");
  if (kind < 0 || kind > 2) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_cascade_decide: kind must be 0 (msp), 1 (margin) or 2 (entropy)");
  if (n < 1 || n >= (1ll << 31)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_cascade_decide: n must lie in [1, 2^31)");
  if (C < 1 || ld < C || ld >= (1ll << 31)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_cascade_decide: 1 <= C <= ld < 2^31");
  if (C > CS_MAX_C) return uvc_set_error_msg(UVC_ERR_UNSUPPORTED, "uvc_cascade_decide: at most 65536 classes");
  if (!(T > 0.f) || !std::isfinite(T)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_cascade_decide: the temperature must be positive and finite");
  if (tau != tau) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_cascade_decide: the threshold is NaN");
  if (!al4(logits) || !al4(score) || !al4(top1) || !al4(defer)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_cascade_decide: misaligned operand");
  const int vec = al16(logits) && ld % 4 == 0;
  k_cascade_decide<<<(unsigned)((n + 3) / 4), 256, 0, (hipStream_t)stream>>>(logits, n, ld, C, T, kind, tau, vec, score, top1, defer);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

extern "C" int uvc_cascade_compact_workspace_bytes(int64_t n, int64_t* bytes) {
  if (!bytes || n < 1 || n >= (1ll << 31)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_cascade_compact_workspace_bytes: bytes and 1 <= n < 2^31");
  *bytes = (n + CS_TILE - 1) / CS_TILE * 4;
  return UVC_OK;
}

extern "C" int uvc_cascade_compact(const int32_t* defer, int64_t n, int32_t* idx, int32_t* pos, int32_t* count, void* workspace, int64_t workspace_bytes,
                                   void* stream) {
  if (!defer || !count || !workspace || (!idx && !pos)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_cascade_compact: null pointer");
  if (n < 1 || n >= (1ll << 31)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_cascade_compact: n must lie in [1, 2^31)");
  const int64_t nb = (n + CS_TILE - 1) / CS_TILE;
  if (workspace_bytes < nb * 4) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_cascade_compact: workspace smaller than uvc_cascade_compact_workspace_bytes()");
  if (!al4(defer) || !al4(idx) || !al4(pos) || !al4(count) || !al4(workspace)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_cascade_compact: misaligned operand");
  int32_t* counts = (int32_t*)workspace;
  const int vec = al16(defer), vec_pos = al16(pos);
  k_cascade_count<<<(unsigned)nb, 256, 0, (hipStream_t)stream>>>(defer, n, vec, counts);
  UVC_CHECK_LAUNCH();
  k_cascade_scan<<<1, 256, 0, (hipStream_t)stream>>>(counts, (int)nb, count);
  UVC_CHECK_LAUNCH();
  k_cascade_write<<<(unsigned)nb, 256, 0, (hipStream_t)stream>>>(defer, n, vec, vec_pos, counts, idx, pos);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

extern "C" int uvc_cascade_gather(const void* src, int64_t ld_src, int32_t dtype, int64_t n, int64_t rows_per_item, int64_t width, const int32_t* idx,
                                  int64_t m, void* dst, int64_t ld_dst, void* stream) {
  if (dtype != UVC_F32 && dtype != UVC_BF16) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_cascade_gather: bad dtype");
  if (n < 1 || n >= (1ll << 31) || m < 0 || m > n) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_cascade_gather: 1 <= n < 2^31 and 0 <= m <= n");
  if (rows_per_item < 1 || width < 1 || ld_src < width || ld_dst < width || rows_per_item >= (1ll << 31) || ld_src >= (1ll << 31) || ld_dst >= (1ll << 31))
    return uvc_set_error_msg(UVC_ERR_ARG, "uvc_cascade_gather: rows_per_item >= 1 and 1 <= width <= ld_src, ld_dst < 2^31");
  if (m == 0) return UVC_OK;                             // nothing is deferred: nothing is launched
  if (!src || !idx || !dst) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_cascade_gather: null pointer");
  const int esz = dtype == UVC_F32 ? 4 : 2;
  if (((uintptr_t)src & (esz - 1)) || ((uintptr_t)dst & (esz - 1)) || !al4(idx)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_cascade_gather: misaligned operand");
  GatherArgs a;
  a.src = (const char*)src; a.dst = (char*)dst; a.idx = idx; a.n = n; a.esz = esz;
  if (ld_src == width && ld_dst == width) {              // dense on both sides: an item is one row
    a.rpi = 1;
    a.row_bytes = a.lds_bytes = a.ldd_bytes = rows_per_item * width * esz;
  } else {
    a.rpi = rows_per_item;
    a.row_bytes = width * esz; a.lds_bytes = ld_src * esz; a.ldd_bytes = ld_dst * esz;
  }
  a.chunks = (a.row_bytes + CS_CHUNK - 1) / CS_CHUNK;
  a.vec = al16(src) && al16(dst) && a.lds_bytes % 16 == 0 && a.ldd_bytes % 16 == 0;
  const int64_t rows = m * a.rpi;
  if (rows > ((1ll << 31) - 1) / a.chunks) return uvc_set_error_msg(UVC_ERR_UNSUPPORTED, "uvc_cascade_gather: more than 2^31 - 1 workgroups");
  k_cascade_gather<<<(unsigned)(rows * a.chunks), 256, 0, (hipStream_t)stream>>>(a);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

extern "C" int uvc_cascade_merge(const float* z_small, int64_t ld_small, const float* z_large, int64_t ld_large, int64_t m, const int32_t* pos, int64_t n,
                                 int32_t C, float* out, int64_t ld_out, int32_t* source, void* stream) {
  if (!z_small || !pos || !out || (m > 0 && !z_large)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_cascade_merge: null pointer");
  if (n < 1 || n >= (1ll << 31) || m < 0 || m > n) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_cascade_merge: 1 <= n < 2^31 and 0 <= m <= n");
  if (C < 1 || ld_small < C || ld_out < C || (m > 0 && ld_large < C) || ld_small >= (1ll << 31) || ld_large >= (1ll << 31) || ld_out >= (1ll << 31))
    return uvc_set_error_msg(UVC_ERR_ARG, "uvc_cascade_merge: 1 <= C <= ld_small, ld_large, ld_out < 2^31");
  if (!al4(z_small) || !al4(z_large) || !al4(pos) || !al4(out) || !al4(source)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_cascade_merge: misaligned operand");
  const int vec = al16(z_small) && al16(out) && ld_small % 4 == 0 && ld_out % 4 == 0 && (m == 0 || (al16(z_large) && ld_large % 4 == 0));
  k_cascade_merge<<<(unsigned)((n + 3) / 4), 256, 0, (hipStream_t)stream>>>((const uint32_t*)z_small, ld_small, (const uint32_t*)z_large, ld_large, m, pos, n, C,
                                                                           vec, (uint32_t*)out, ld_out, source);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}
