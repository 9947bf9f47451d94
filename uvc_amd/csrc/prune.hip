// Taylor gate scores of compact models (python -m uvc_amd.compact_prune) for gfx950: the per-image gradient of the loss with respect to a
// multiplicative gate on every kept head's attention output and on every MLP unit's GELU output, taken at gate = 1 -- the per-image dot
// products  sum_n sum_{c in group} a[b n, c] * da[b n, c]  behind the attn.proj and fc2 dgrads of uvc_vit_compact_gate_grads -- and their
// running sums over a split.  uvc_gate_dots is bandwidth-bound: every operand element is read once, lanes run along the columns with
// 16-byte accesses where the width, the leading dimensions and the pointers allow them (element by element otherwise, with the same
// values), the waves of a workgroup split an image's rows and meet in LDS in wave order, offsets are 64-bit.  Products and sums are
// float64 in a fixed order, rounded once to float32.  No atomics, one writer per output element: the same bits on a repeat and for any B.
#include "common.h"
#include "../../include/uvc_kernels.h"

namespace {

constexpr int WAVES = 4;

template <typename T, int W> struct Row;      // W consecutive elements of T as floats, and back
template <> struct Row<float, 1> {
  static __device__ __forceinline__ void load(const float* p, float* v) { v[0] = *p; }
  static __device__ __forceinline__ void store(float* p, const float* v) { *p = v[0]; }
};
template <> struct Row<bf16_t, 1> {
  static __device__ __forceinline__ void load(const bf16_t* p, float* v) { v[0] = bf16_to_f32(*p); }
  static __device__ __forceinline__ void store(bf16_t* p, const float* v) { *p = f32_to_bf16(v[0]); }
};
template <> struct Row<float, 4> {
  static __device__ __forceinline__ void load(const float* p, float* v) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(p);
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
  }
  static __device__ __forceinline__ void store(float* p, const float* v) { *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]}; }
};
template <> struct Row<float, 8> {
  static __device__ __forceinline__ void load(const float* p, float* v) { Row<float, 4>::load(p, v); Row<float, 4>::load(p + 4, v + 4); }
  static __device__ __forceinline__ void store(float* p, const float* v) { Row<float, 4>::store(p, v); Row<float, 4>::store(p + 4, v + 4); }
};
template <> struct Row<bf16_t, 8> {
  static __device__ __forceinline__ void load(const bf16_t* p, float* v) {
    const u32x4 r = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[2 * i] = __uint_as_float(r[i] << 16); v[2 * i + 1] = __uint_as_float(r[i] & 0xffff0000u); }
  }
  static __device__ __forceinline__ void store(bf16_t* p, const float* v) {
    u32x4 q;
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = pack_bf16x2(v[2 * i], v[2 * i + 1]);
    *reinterpret_cast<u32x4*>(p) = q;
  }
};

struct DotArgs {
  const void* a; const void* da; const void* aux; void* dA; float* out;
  int64_t lda, ldda, ldaux, lddA, ld_out;
  int N, width, group, col0, chunk;      // chunk: the columns of a workgroup, a multiple of W and of group
};

// Workgroup (x, y): image y, columns [x chunk, min(width, (x + 1) chunk)).  A wave holds 64 / LPR rows side by side, LPR = 64 lanes of W
// columns each where the chunk needs them all, fewer (a power of two) on a narrow one; lane (sub, cl) of wave w walks the rows
// w (64 / LPR) + sub + k (WAVES 64 / LPR), k ascending, with one float64 chain per column.  Then per column the partial sums meet in LDS in
// (wave, sub) order, and one thread per gate adds the group's columns in ascending order.  FUSED: a = u (T), da = dh (float32),
// aux = GELU' (T), and dA = round_T(dh * float(aux)) is written on the way.
template <typename T, typename G, int W, bool FUSED>
__global__ __launch_bounds__(WAVES * 64) void k_gate_dots(DotArgs p, int lpr_log2) {
  __shared__ double part[WAVES * 64 * W];
  __shared__ double cols[64 * W];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lpr = 1 << lpr_log2, rpw = 64 >> lpr_log2;
  const int sub = lane >> lpr_log2, cl = lane & (lpr - 1);
  const int c0 = blockIdx.x * p.chunk, cend = min(p.width, c0 + p.chunk);
  const int col = c0 + cl * W;
  const size_t row0 = (size_t)blockIdx.y * (size_t)p.N;
  double acc[W];
#pragma unroll
  for (int e = 0; e < W; ++e) acc[e] = 0.0;
  if (col < cend) {
    const T* a = (const T*)p.a;
    const G* da = (const G*)p.da;
    for (int n = wave * rpw + sub; n < p.N; n += WAVES * rpw) {
      const size_t r = row0 + (size_t)n;
      float x[W], g[W];
      Row<T, W>::load(a + r * (size_t)p.lda + col, x);
      Row<G, W>::load(da + r * (size_t)p.ldda + col, g);
#pragma unroll
      for (int e = 0; e < W; ++e) acc[e] += (double)x[e] * (double)g[e];
      if constexpr (FUSED) {
        float s[W], v[W];
        Row<T, W>::load((const T*)p.aux + r * (size_t)p.ldaux + col, s);
#pragma unroll
        for (int e = 0; e < W; ++e) v[e] = g[e] * s[e];
        Row<T, W>::store((T*)p.dA + r * (size_t)p.lddA + col, v);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < W; ++e) part[(wave * 64 + lane) * W + e] = acc[e];
  __syncthreads();
  const int ncols = cend - c0;
  for (int c = tid; c < ncols; c += WAVES * 64) {
    const int l = c / W, e = c % W;
    double s = 0.0;
    for (int w = 0; w < WAVES; ++w)
      for (int k = 0; k < rpw; ++k) s += part[(w * 64 + (k << lpr_log2) + l) * W + e];
    cols[c] = s;
  }
  __syncthreads();
  float* o = p.out + (size_t)blockIdx.y * (size_t)p.ld_out + p.col0 + c0 / p.group;
  for (int g = tid; g < ncols / p.group; g += WAVES * 64) {
    double s = 0.0;
    for (int c = 0; c < p.group; ++c) s += cols[g * p.group + c];
    o[g] = (float)s;
  }
}

template <typename T, typename G, int W, bool FUSED>
int launch_dots(DotArgs p, int B, hipStream_t st) {
  // the columns of a workgroup: up to 64 lanes of W, whole groups only (group % 16 == 0 or group == 1, and W divides 16)
  const int full = 64 * W;
  p.chunk = p.group == 1 ? full : (full / p.group) * p.group;
  if (p.chunk > p.width) p.chunk = p.width;
  const int lanes = p.chunk / W;
  int lpr_log2 = 0;
  while ((1 << lpr_log2) < lanes) ++lpr_log2;
  const dim3 grid((unsigned)((p.width + p.chunk - 1) / p.chunk), (unsigned)B);
  k_gate_dots<T, G, W, FUSED><<<grid, WAVES * 64, 0, st>>>(p, lpr_log2);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

// sum_sq[g] += s[b, g]^2 and sum_abs[g] += |s[b, g]|, b ascending: one float64 chain per gate that goes on from the stored value
__global__ __launch_bounds__(256) void k_gate_accumulate(const float* __restrict__ s, size_t ld, int B, int G, double* __restrict__ sum_sq,
                                                         double* __restrict__ sum_abs) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  double q = sum_sq[g], a = sum_abs[g];
  for (int b = 0; b < B; ++b) {
    const double v = (double)s[(size_t)b * ld + g];
    q += v * v;
    a += fabs(v);
  }
  sum_sq[g] = q; sum_abs[g] = a;
}

}  // namespace

extern "C" int uvc_gate_dots(const void* a, int64_t lda, const void* da, int64_t ldda, const void* aux, int64_t ldaux, void* dA, int64_t lddA,
                             int32_t B, int32_t N, int32_t width, int32_t group, float* out, int64_t ld_out, int32_t col0, int32_t dtype,
                             void* stream) {
  if (!a || !da || !out) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gate_dots: null pointer");
  if ((aux == nullptr) != (dA == nullptr)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gate_dots: the fused form takes both aux and dA, the plain form neither");
  if (dtype != UVC_F32 && dtype != UVC_BF16) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gate_dots: bad dtype");
  if (B <= 0 || B > 65535 || N <= 0) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gate_dots: need 1 <= B <= 65535 and N >= 1");
  if (width <= 0 || width % 16) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gate_dots: width must be a positive multiple of 16");
  if ((group != 1 && group != 16 && group != 32 && group != 48 && group != 64) || width % group)
    return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gate_dots: group must be 1, 16, 32, 48 or 64 and divide width");
  const bool fused = aux != nullptr;
  if (lda < width || ldda < width || (fused && (ldaux < width || lddA < width)))
    return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gate_dots: a leading dimension below width");
  if (col0 < 0 || ld_out < (int64_t)col0 + width / group) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gate_dots: out row too short for col0 + width / group gates");
  DotArgs p;
  p.a = a; p.da = da; p.aux = aux; p.dA = dA; p.out = out;
  p.lda = lda; p.ldda = ldda; p.ldaux = ldaux; p.lddA = lddA; p.ld_out = ld_out;
  p.N = N; p.width = width; p.group = group; p.col0 = col0; p.chunk = 0;
  hipStream_t st = (hipStream_t)stream;
  const bool f32 = dtype == UVC_F32;
  // 16-byte accesses: rows of T (and of the float32 dgrad) start on 16 bytes whatever the row
  const int64_t tper = f32 ? 4 : 8;                          // elements of T in 16 bytes
  const bool t_ok = (((uintptr_t)a | (uintptr_t)aux | (uintptr_t)dA) & 15) == 0 && lda % tper == 0 && (!fused || (ldaux % tper == 0 && lddA % tper == 0));
  const int64_t gper = (fused || f32) ? 4 : 8;               // elements of da in 16 bytes
  const bool wide = t_ok && ((uintptr_t)da & 15) == 0 && ldda % gper == 0;
  if (f32) {
    if (fused) return wide ? launch_dots<float, float, 4, true>(p, B, st) : launch_dots<float, float, 1, true>(p, B, st);
    return wide ? launch_dots<float, float, 4, false>(p, B, st) : launch_dots<float, float, 1, false>(p, B, st);
  }
  if (fused) return wide ? launch_dots<bf16_t, float, 8, true>(p, B, st) : launch_dots<bf16_t, float, 1, true>(p, B, st);
  return wide ? launch_dots<bf16_t, bf16_t, 8, false>(p, B, st) : launch_dots<bf16_t, bf16_t, 1, false>(p, B, st);
}

extern "C" int uvc_gate_accumulate(const float* s, int64_t ld, int32_t B, int32_t G, double* sum_sq, double* sum_abs, void* stream) {
  if (!s || !sum_sq || !sum_abs) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gate_accumulate: null pointer");
  if (B <= 0 || G <= 0 || ld < G) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gate_accumulate: need B >= 1, G >= 1 and ld >= G");
  k_gate_accumulate<<<(unsigned)((G + 255) / 256), 256, 0, (hipStream_t)stream>>>(s, (size_t)ld, B, G, sum_sq, sum_abs);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}
