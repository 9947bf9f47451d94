// Pixel-resolution maps from the gradient of a class logit at the input (python -m uvc_amd.compact_pixel) for gfx950: the inverse of
// uvc_patchify, the interpolated inputs of integrated gradients, the sum of their gradients, and the read-out of a gradient as a pixel map,
// a patch map and a signed total.  Small bandwidth-bound kernels around uvc_vit_compact_input_grad: every element is read once, 16-byte
// accesses where the row width and every pointer allow them (8 bytes for four bf16 beside four float32) and element by element otherwise,
// offsets in size_t, no atomics, fixed summation orders: the same bits on a repeat and in any batch.
#include "common.h"
#include "../../include/uvc_kernels.h"

namespace {

inline unsigned grid_for(size_t n) { const size_t g = (n + 255) / 256; return (unsigned)(g > 4096 ? 4096 : (g < 1 ? 1 : g)); }   // a capped grid, the rest by stride
inline bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

// W consecutive elements of T as floats, and back (W = 1, or 4: one 16-byte / 8-byte access)
template <typename T, int W> struct Vec;
template <> struct Vec<float, 1> {
  static __device__ __forceinline__ void load(const float* p, float* v) { v[0] = *p; }
  static __device__ __forceinline__ void store(float* p, const float* v) { *p = v[0]; }
};
template <> struct Vec<bf16_t, 1> {
  static __device__ __forceinline__ void load(const bf16_t* p, float* v) { v[0] = bf16_to_f32(*p); }
  static __device__ __forceinline__ void store(bf16_t* p, const float* v) { *p = f32_to_bf16(v[0]); }
};
template <> struct Vec<float, 4> {
  static __device__ __forceinline__ void load(const float* p, float* v) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(p);
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
  }
  static __device__ __forceinline__ void store(float* p, const float* v) { *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]}; }
};
template <> struct Vec<bf16_t, 4> {
  static __device__ __forceinline__ void load(const bf16_t* p, float* v) {
    const u32x2 r = *reinterpret_cast<const u32x2*>(p);
    v[0] = __uint_as_float(r[0] << 16); v[1] = __uint_as_float(r[0] & 0xffff0000u);
    v[2] = __uint_as_float(r[1] << 16); v[3] = __uint_as_float(r[1] & 0xffff0000u);
  }
  static __device__ __forceinline__ void store(bf16_t* p, const float* v) {
    u32x2 q; q[0] = pack_bf16x2(v[0], v[1]); q[1] = pack_bf16x2(v[2], v[3]);
    *reinterpret_cast<u32x2*>(p) = q;
  }
};
template <> struct Vec<bf16_t, 8> {
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

// ---------------------------------------------------------------------------- rows -> image (uvc_unpatchify)
// k_patchify's index walk with source and destination swapped: item (r, k / W) of the rows goes to pixel (b, c, py P + ky, px P + kx).
// W = 4: P % 4 == 0, so the four kx stay inside one image line and both addresses are multiples of 16 bytes.
template <int W>
__global__ __launch_bounds__(256) void k_unpatchify(const float* __restrict__ rows, float* __restrict__ out, int C, int S, int P, size_t total) {
  const int G = S / P, KW = C * P * P / W, PW = P / W;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int kw = (int)(idx % KW);
    const size_t r = idx / KW;
    const int px = (int)(r % G), py = (int)((r / G) % G);
    const size_t b = r / ((size_t)G * G);
    const int kxw = kw % PW, ky = (kw / PW) % P, c = kw / (PW * P);
    float v[W];
    Vec<float, W>::load(rows + idx * W, v);
    Vec<float, W>::store(out + ((b * C + c) * S + (py * P + ky)) * S + px * P + kxw * W, v);
  }
}

// ---------------------------------------------------------------------------- interpolated inputs (uvc_ig_rows)
// Lane i takes W elements of x (and x0) once and writes them at every step.  alpha_s as a float pair (hi + lo of the double quotient), so
// the only roundings beside the last one are those of x - x0 and of the lo term at x0's magnitude: with |x|, |x0| <= m the value is within
// ulp(m) + ulp(m) / 2 + ulp(m) / 2 of the exact one before it is rounded to T.
template <typename T, int W>
__global__ __launch_bounds__(256) void k_ig_rows(const T* __restrict__ x, const T* __restrict__ x0, T* __restrict__ out, size_t total, size_t items,
                                                 int first_step, int count, int steps) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (size_t)gridDim.x * 256) {
    float a[W], b[W], d[W];
    Vec<T, W>::load(x + i * W, a);
#pragma unroll
    for (int e = 0; e < W; ++e) b[e] = 0.f;
    if (x0) Vec<T, W>::load(x0 + i * W, b);
#pragma unroll
    for (int e = 0; e < W; ++e) d[e] = a[e] - b[e];
    for (int s = 0; s < count; ++s) {
      const double al = ((double)(first_step + s) + 0.5) / (double)steps;
      const float hi = (float)al, lo = (float)(al - (double)hi);
      float v[W];
#pragma unroll
      for (int e = 0; e < W; ++e) v[e] = __builtin_fmaf(hi, d[e], __builtin_fmaf(lo, d[e], b[e]));
      Vec<T, W>::store(out + (size_t)s * total + i * W, v);
    }
  }
}

// ---------------------------------------------------------------------------- sum of the steps' gradients (uvc_ig_accumulate)
template <int W>
__global__ __launch_bounds__(256) void k_ig_accumulate(const float* __restrict__ g, float* __restrict__ acc, size_t n, size_t items, int count, int first) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (size_t)gridDim.x * 256) {
    float s[W];
#pragma unroll
    for (int e = 0; e < W; ++e) s[e] = 0.f;
    if (!first) Vec<float, W>::load(acc + i * W, s);
    for (int k = 0; k < count; ++k) {                         // ascending: one chain per element
      float v[W];
      Vec<float, W>::load(g + (size_t)k * n + i * W, v);
#pragma unroll
      for (int e = 0; e < W; ++e) s[e] += v[e];
    }
    Vec<float, W>::store(acc + i * W, s);
  }
}

// ---------------------------------------------------------------------------- pixel map, patch map, total (uvc_pixel_maps)
// One wave per patch row, four rows per workgroup.  A lane owns the pixel positions j, j + 64, ... of the patch (W consecutive kx each)
// and walks the channels in ascending order: sum_c |e| goes to the pixel map at once; |e| and e are also summed over the lane's positions in
// that order, then over the wave by the xor butterfly.  k_image_total then sums an image's patch totals: a thread's patches ascending, the
// wave butterfly, the waves in order.
template <typename T, int W>
__global__ __launch_bounds__(256) void k_pixel_maps(const float* __restrict__ a, const T* __restrict__ x, const T* __restrict__ x0, float scale,
                                                    int C, int S, int P, size_t nrows, float* __restrict__ pixel, float* __restrict__ patch,
                                                    float* __restrict__ partial) {
  const int lane = threadIdx.x & 63;
  const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nrows) return;                                   // (wave-uniform; no barrier below)
  const int G = S / P, PP = P * P, units = PP / W, PW = P / W;
  const size_t K0 = (size_t)C * PP;
  const int px = (int)(row % G), py = (int)((row / G) % G);
  const size_t b = row / ((size_t)G * G);
  float sabs = 0.f, ssum = 0.f;
  for (int j = lane; j < units; j += 64) {
    float m[W];
#pragma unroll
    for (int e = 0; e < W; ++e) m[e] = 0.f;
    for (int c = 0; c < C; ++c) {
      const size_t off = row * K0 + (size_t)c * PP + (size_t)j * W;
      float v[W];
      Vec<float, W>::load(a + off, v);
      if (x) {
        float xv[W], bv[W];
        Vec<T, W>::load(x + off, xv);
#pragma unroll
        for (int e = 0; e < W; ++e) bv[e] = 0.f;
        if (x0) Vec<T, W>::load(x0 + off, bv);
#pragma unroll
        for (int e = 0; e < W; ++e) v[e] = v[e] * (xv[e] - bv[e]);
      }
#pragma unroll
      for (int e = 0; e < W; ++e) {
        const float t = v[e] * scale;
        m[e] += fabsf(t); sabs += fabsf(t); ssum += t;
      }
    }
    if (pixel) {
      const int ky = j / PW, kxw = j % PW;
      Vec<float, W>::store(pixel + (b * S + (size_t)(py * P + ky)) * S + (size_t)px * P + (size_t)kxw * W, m);
    }
  }
  sabs = wave_sum(sabs);
  ssum = wave_sum(ssum);
  if (lane == 0) {
    if (patch) patch[row] = sabs;
    if (partial) partial[row] = ssum;
  }
}

__global__ __launch_bounds__(256) void k_image_total(const float* __restrict__ partial, int np, float* __restrict__ total) {
  __shared__ float sh[4];
  const float* p = partial + (size_t)blockIdx.x * np;
  float s = 0.f;
  for (int i = threadIdx.x; i < np; i += 256) s += p[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) total[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

}  // namespace

extern "C" int uvc_unpatchify(const float* rows, float* out, int32_t B, int32_t C, int32_t S, int32_t P, void* stream) {
  if (!rows || !out) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_unpatchify: null pointer");
  if (B <= 0 || C <= 0 || S <= 0 || P <= 0 || S % P) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_unpatchify: B, C, S, P must be positive and S % P == 0");
  const size_t n = (size_t)B * C * S * S;
  hipStream_t st = (hipStream_t)stream;
  if (P % 4 == 0 && aligned16(rows, out)) k_unpatchify<4><<<grid_for(n / 4), 256, 0, st>>>(rows, out, C, S, P, n / 4);
  else k_unpatchify<1><<<grid_for(n), 256, 0, st>>>(rows, out, C, S, P, n);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

extern "C" int uvc_ig_rows(const void* x, const void* x0, void* out, int64_t nrows, int32_t width, int32_t first_step, int32_t count, int32_t steps,
                           int32_t dtype, void* stream) {
  if (!x || !out) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_ig_rows: null pointer");
  if (nrows <= 0 || width <= 0 || count <= 0 || steps <= 0) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_ig_rows: nrows, width, count and steps must be positive");
  if (first_step < 0 || (int64_t)first_step + count > steps) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_ig_rows: need 0 <= first_step and first_step + count <= steps");
  if (dtype != UVC_F32 && dtype != UVC_BF16) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_ig_rows: bad dtype");
  const size_t total = (size_t)nrows * width, esz = dtype == UVC_F32 ? 4 : 2;
  const bool wide = ((size_t)width * esz) % 16 == 0 && aligned16(x, x0, out);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == UVC_F32) {
    if (wide) k_ig_rows<float, 4><<<grid_for(total / 4), 256, 0, st>>>((const float*)x, (const float*)x0, (float*)out, total, total / 4, first_step, count, steps);
    else k_ig_rows<float, 1><<<grid_for(total), 256, 0, st>>>((const float*)x, (const float*)x0, (float*)out, total, total, first_step, count, steps);
  } else {
    if (wide) k_ig_rows<bf16_t, 8><<<grid_for(total / 8), 256, 0, st>>>((const bf16_t*)x, (const bf16_t*)x0, (bf16_t*)out, total, total / 8, first_step, count, steps);
    else k_ig_rows<bf16_t, 1><<<grid_for(total), 256, 0, st>>>((const bf16_t*)x, (const bf16_t*)x0, (bf16_t*)out, total, total, first_step, count, steps);
  }
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

extern "C" int uvc_ig_accumulate(const float* d_rows, float* acc, int64_t n, int32_t count, int32_t first, void* stream) {
  if (!d_rows || !acc) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_ig_accumulate: null pointer");
  if (n <= 0 || count <= 0) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_ig_accumulate: n and count must be positive");
  hipStream_t st = (hipStream_t)stream;
  if (n % 4 == 0 && aligned16(d_rows, acc)) k_ig_accumulate<4><<<grid_for((size_t)n / 4), 256, 0, st>>>(d_rows, acc, (size_t)n, (size_t)n / 4, count, first != 0);
  else k_ig_accumulate<1><<<grid_for((size_t)n), 256, 0, st>>>(d_rows, acc, (size_t)n, (size_t)n, count, first != 0);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

extern "C" int uvc_pixel_maps(const float* a, const void* x, const void* x0, float scale, int32_t B, int32_t C, int32_t S, int32_t P, int32_t dtype,
                              float* pixel, float* patch, float* total, float* partial, void* stream) {
  if (!a) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_pixel_maps: null gradient rows");
  if (B <= 0 || C <= 0 || S <= 0 || P <= 0 || S % P) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_pixel_maps: B, C, S, P must be positive and S % P == 0");
  if (dtype != UVC_F32 && dtype != UVC_BF16) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_pixel_maps: bad dtype");
  if (x0 && !x) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_pixel_maps: a baseline (x0) goes with x");
  if (total && !partial) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_pixel_maps: total needs the partial scratch [B * np]");
  if (!pixel && !patch && !total) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_pixel_maps: no output");
  const int np = (S / P) * (S / P);
  const size_t nrows = (size_t)B * np;
  if ((nrows + 3) / 4 > 0x7fffffffull) return uvc_set_error_msg(UVC_ERR_UNSUPPORTED, "uvc_pixel_maps: too many patch rows for one launch");
  const bool wide = P % 4 == 0 && aligned16(a, pixel) && (((uintptr_t)x | (uintptr_t)x0) & (dtype == UVC_F32 ? 15 : 7)) == 0;
  const unsigned grid = (unsigned)((nrows + 3) / 4);
  hipStream_t st = (hipStream_t)stream;
  float* part = total ? partial : nullptr;
  if (dtype == UVC_F32) {
    if (wide) k_pixel_maps<float, 4><<<grid, 256, 0, st>>>(a, (const float*)x, (const float*)x0, scale, C, S, P, nrows, pixel, patch, part);
    else k_pixel_maps<float, 1><<<grid, 256, 0, st>>>(a, (const float*)x, (const float*)x0, scale, C, S, P, nrows, pixel, patch, part);
  } else {
    if (wide) k_pixel_maps<bf16_t, 4><<<grid, 256, 0, st>>>(a, (const bf16_t*)x, (const bf16_t*)x0, scale, C, S, P, nrows, pixel, patch, part);
    else k_pixel_maps<bf16_t, 1><<<grid, 256, 0, st>>>(a, (const bf16_t*)x, (const bf16_t*)x0, scale, C, S, P, nrows, pixel, patch, part);
  }
  UVC_CHECK_LAUNCH();
  if (total) {
    k_image_total<<<(unsigned)B, 256, 0, st>>>(partial, np, total);
    UVC_CHECK_LAUNCH();
  }
  return UVC_OK;
}
