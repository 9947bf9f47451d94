// Common corruptions of a normalised image batch (python -m uvc_amd.compact_corrupt) for gfx950: noise, brightness, contrast, blur, pixelate
// (include/uvc_kernels.h has the statements).  float32 in and out, size_t offsets, no atomics, one writer per output element, nothing that
// depends on the grid: the same bits on a repeat and for any split of the batch.
//
// Noise: a thread takes the 4 elements of one multiple of 4 of the GLOBAL index g = index0 C H W + e, so its two Box-Muller pairs are whole
// whatever the batch's first index is: two hashes, one logf, one sqrtf and one sincosf per pair (the accurate library functions).  When
// that quad is 16-byte aligned in x and out (decided on the host, the same for every quad) it is one 16-byte load and store; the ragged
// first and last quads, and every quad otherwise, go element by element.  The generator is elementwise.hip's (uvc_exp_noise).
// Colour: brightness is a thread per pixel over its channels; contrast reads its image's mean from a launch of its own (one workgroup per
// image, float64 per-thread sums over ascending elements, a fixed LDS tree).
// Blur: a 64 x 32 output tile with its halo in LDS, 256 threads of 8 outputs each (lane = column: LDS reads of a wave are consecutive words);
// the taps run in the outer loop, so each output is one ascending fma chain.  The separable pass is called twice through the scratch plane,
// the dense K x K stencil (defocus) skips zero taps by a wave-uniform branch.
// Pixelate: a tile of up to 256 cells per workgroup (128 pixels wide), one row-major sum per cell and thread into LDS, then the tile's pixels
// are written in row order; cells wider
// than 16 take a workgroup each and a float64 sum.
#include <cstdio>
#include <cmath>
#include "common.h"
#include "../../include/uvc_kernels.h"

namespace {

constexpr int CR_THREADS = 256;
constexpr int CR_MEAN_THREADS = 1024;                        // the contrast mean: one workgroup per image
constexpr int CR_TW = 64, CR_TH = 32;                       // the blurs' output tile
constexpr int CR_MAX_R = 32, CR_MAX_K = 25;
constexpr int CR_PIX_SMALL = 16;                            // pixelate: cells up to this width are summed by one thread
constexpr unsigned CR_MAX_GRID = 0x7fffffffu;

__device__ __forceinline__ uint64_t cr_splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
// the uniform of k_exp_noise: (c + 1/2) 2^-24 of the 24-bit counter, the one value that rounds to 1 brought back
__device__ __forceinline__ float cr_uniform(uint64_t key, uint64_t hashed_counter) {
  const uint64_t h = cr_splitmix64(key ^ hashed_counter);
  const float u = ((float)(uint32_t)(h >> 40) + 0.5f) * (1.0f / 16777216.0f);
  return fminf(u, 0x1.fffffep-1f);
}
__device__ __forceinline__ void cr_box_muller(float u1, float u2, float& z0, float& z1) {
  const float r = sqrtf(-2.0f * logf(u1));
  const float t = 6.28318530717958647692f * u2;
  float s, c;
  sincosf(t, &s, &c);
  z0 = r * c;
  z1 = r * s;
}

struct NoiseArgs {
  const float* x; float* out;
  uint64_t n, gstart, key0, key1, key2;
  uint32_t hw; int C, kind;
  float ca[4], cb[4], lo[4], hi[4];
  float t_lo, t_hi;                                          // impulse: u < t_lo -> lo, u < t_hi -> hi
};

__device__ __forceinline__ float cr_noise_one(const NoiseArgs& a, float x, int c, float z, uint64_t g) {
  if (a.kind == UVC_CORRUPT_IMPULSE_NOISE) {
    const float u = cr_uniform(a.key2, cr_splitmix64(g));
    return u < a.t_lo ? a.lo[c] : u < a.t_hi ? a.hi[c] : fminf(fmaxf(x, a.lo[c]), a.hi[c]);
  }
  const float v = fmaf(z, fmaf(a.ca[c], x, a.cb[c]), x);
  return fminf(fmaxf(v, a.lo[c]), a.hi[c]);
}

template <bool VEC>
__global__ __launch_bounds__(CR_THREADS) void k_corrupt_noise(NoiseArgs a) {
  const uint64_t q = (uint64_t)blockIdx.x * CR_THREADS + threadIdx.x;
  const uint64_t gq = (a.gstart & ~3ull) + q * 4;            // the quad's first global index, a multiple of 4
  const int64_t e0 = (int64_t)(gq - a.gstart);               // -3 .. n - 1 (the grid covers no more)
  if (e0 >= (int64_t)a.n) return;
  // channel of the quad's first element inside the batch (of element 0 for the ragged first quad)
  const uint64_t ef = e0 < 0 ? 0 : (uint64_t)e0;
  uint32_t rem; int c;
  if (a.n <= 0xffffffffull) { const uint32_t pl = (uint32_t)ef / a.hw; rem = (uint32_t)ef - pl * a.hw; c = (int)(pl % (uint32_t)a.C); }
  else { const uint64_t pl = ef / a.hw; rem = (uint32_t)(ef - pl * a.hw); c = (int)(pl % (uint64_t)a.C); }
  float z[4] = {0.f, 0.f, 0.f, 0.f};
  if (a.kind != UVC_CORRUPT_IMPULSE_NOISE) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const uint64_t hj = cr_splitmix64((gq >> 1) + p);
      cr_box_muller(cr_uniform(a.key0, hj), cr_uniform(a.key1, hj), z[2 * p], z[2 * p + 1]);
    }
  }
  const bool whole = e0 >= 0 && (uint64_t)e0 + 3 < a.n;
  if (VEC && whole) {
    const f32x4 v = *(const f32x4*)(a.x + (size_t)e0);
    f32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      o[i] = cr_noise_one(a, v[i], c, z[i], gq + i);
      if (++rem == a.hw) { rem = 0; c = c + 1 == a.C ? 0 : c + 1; }
    }
    *(f32x4*)(a.out + (size_t)e0) = o;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t e = e0 + i;
      if (e >= 0 && (uint64_t)e < a.n) {
        a.out[(size_t)e] = cr_noise_one(a, a.x[(size_t)e], c, z[i], gq + i);
        if (++rem == a.hw) { rem = 0; c = c + 1 == a.C ? 0 : c + 1; }
      }
    }
  }
}

__global__ __launch_bounds__(CR_THREADS) void k_box_muller(const float* __restrict__ u1, const float* __restrict__ u2, float* __restrict__ z0,
                                                           float* __restrict__ z1, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * CR_THREADS + threadIdx.x;
  if (i < n) {
    float a, b;
    cr_box_muller(u1[i], u2[i], a, b);
    z0[i] = a;
    z1[i] = b;
  }
}

struct ColourArgs {
  const float* x; float* out; float* image_mean;
  uint32_t hw, blocks_per_image; int C;
  float a;
  double dmean[4], dstd[4];                                  // the mean launch sums p in float64
  float mean[4], std[4], istd[4], nmis[4], lo[4], hi[4];     // istd = 1 / std, nmis = -mean / std (float64 on the host, rounded once)
};

// one workgroup per image: thread t sums p of the elements t, t + 1024, ... of every channel in turn, in float64
__global__ __launch_bounds__(CR_MEAN_THREADS) void k_image_mean(ColourArgs a) {
  __shared__ double sd[CR_MEAN_THREADS];
  const int tid = threadIdx.x;
  const float* xi = a.x + (size_t)blockIdx.x * a.C * a.hw;
  double s = 0.0;
  for (int c = 0; c < a.C; ++c) {
    const double sc = a.dstd[c], mc = a.dmean[c];
    const float* xc = xi + (size_t)c * a.hw;
#pragma unroll 4
    for (uint32_t i = tid; i < a.hw; i += CR_MEAN_THREADS) s += (double)xc[i] * sc + mc;      // (the loads of an unrolled group go out together; the sum keeps its order)
  }
  sd[tid] = s;
  __syncthreads();
  for (int w = CR_MEAN_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) sd[tid] += sd[tid + w];
    __syncthreads();
  }
  if (tid == 0) a.image_mean[blockIdx.x] = (float)(sd[0] / ((double)a.C * (double)a.hw));
}

// contrast: workgroup = 1024 elements of one plane, thread t the elements t, t + 256, t + 512, t + 768
__global__ __launch_bounds__(CR_THREADS) void k_contrast(ColourArgs a) {
  const uint32_t plane = blockIdx.x / a.blocks_per_image, chunk = blockIdx.x - plane * a.blocks_per_image;
  const int c = (int)(plane % (uint32_t)a.C);
  const float m = a.image_mean[plane / (uint32_t)a.C];
  const float cb = (1.0f - a.a) * ((m - a.mean[c]) * a.istd[c]);
  const size_t base = (size_t)plane * a.hw;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t p = chunk * 1024u + i * CR_THREADS + threadIdx.x;
    if (p < a.hw) a.out[base + p] = fminf(fmaxf(fmaf(a.a, a.x[base + p], cb), a.lo[c]), a.hi[c]);
  }
}

// brightness: a thread per pixel, over its channels
__global__ __launch_bounds__(CR_THREADS) void k_brightness(ColourArgs a) {
  const uint32_t img = blockIdx.x / a.blocks_per_image, chunk = blockIdx.x - img * a.blocks_per_image;
  const uint32_t p = chunk * CR_THREADS + threadIdx.x;
  if (p >= a.hw) return;
  const size_t base = (size_t)img * a.C * a.hw + p;
  float v[4];
  float V = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (c < a.C) {
      v[c] = fminf(fmaxf(fmaf(a.x[base + (size_t)c * a.hw], a.std[c], a.mean[c]), 0.f), 1.f);
      V = fmaxf(V, v[c]);
    }
  const float Vn = fminf(V + a.a, 1.f);
  const float s = V > 0.f ? Vn / V : 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (c < a.C) {
      const float pp = V > 0.f ? v[c] * s : Vn;
      a.out[base + (size_t)c * a.hw] = fminf(fmaxf(fmaf(pp, a.istd[c], a.nmis[c]), a.lo[c]), a.hi[c]);
    }
}

struct BlurArgs {
  const float* x; float* out;
  int C, H, W, R, tiles_x, tiles_y, clamp;
  float lo[4], hi[4];
  float w[2 * CR_MAX_R + 1];
};
__device__ __forceinline__ int cr_clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// one pass of the separable filter over a 64 x 32 output tile: along x (VERT = false: LDS [32][64 + 2 R]) or along y ([32 + 2 R][64])
template <bool VERT>
__global__ __launch_bounds__(CR_THREADS) void k_blur_pass(BlurArgs a) {
  __shared__ float s[(CR_TH + 2 * CR_MAX_R) * CR_TW];        // 24 KB; the horizontal tile needs 32 * (64 + 64) words, fewer
  __shared__ float sw[2 * CR_MAX_R + 1];
  const int tid = threadIdx.x, R = a.R, taps = 2 * R + 1;
  const uint32_t per_plane = (uint32_t)a.tiles_x * a.tiles_y;
  const uint32_t plane = blockIdx.x / per_plane, t = blockIdx.x - plane * per_plane;
  const int ty0 = (int)(t / a.tiles_x) * CR_TH, tx0 = (int)(t % a.tiles_x) * CR_TW;
  const float* xp = a.x + (size_t)plane * a.H * a.W;
  const int SW = VERT ? CR_TW : CR_TW + 2 * R, SH = VERT ? CR_TH + 2 * R : CR_TH;
  if (tid < taps) sw[tid] = a.w[tid];
  for (int i = tid; i < SH * SW; i += CR_THREADS) {
    const int r = i / SW, c = i - r * SW;
    const int gy = cr_clampi(ty0 + r - (VERT ? R : 0), a.H - 1), gx = cr_clampi(tx0 + c - (VERT ? 0 : R), a.W - 1);
    s[i] = xp[(size_t)gy * a.W + gx];
  }
  __syncthreads();
  const int col = tid & 63, row0 = tid >> 6;
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  for (int k = 0; k < taps; ++k) {
    const float w = sw[k];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = row0 + 4 * i;
      acc[i] = fmaf(w, VERT ? s[(row + k) * SW + col] : s[row * SW + col + k], acc[i]);
    }
  }
  const int gx = tx0 + col, c = (int)(plane % (uint32_t)a.C);
  if (gx < a.W) {
    float* op = a.out + (size_t)plane * a.H * a.W;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int gy = ty0 + row0 + 4 * i;
      if (gy < a.H) op[(size_t)gy * a.W + gx] = a.clamp ? fminf(fmaxf(acc[i], a.lo[c]), a.hi[c]) : acc[i];
    }
  }
}

struct StencilArgs {
  const float* x; float* out; const float* taps;
  int C, H, W, K, tiles_x, tiles_y, clamp;
  float lo[4], hi[4];
};

__global__ __launch_bounds__(CR_THREADS) void k_stencil2d(StencilArgs a) {
  __shared__ float s[(CR_TH + CR_MAX_K - 1) * (CR_TW + CR_MAX_K - 1)];      // 56 x 88 words, 19.25 KB
  __shared__ float sw[CR_MAX_K * CR_MAX_K];
  const int tid = threadIdx.x, K = a.K, r = K / 2;
  const uint32_t per_plane = (uint32_t)a.tiles_x * a.tiles_y;
  const uint32_t plane = blockIdx.x / per_plane, t = blockIdx.x - plane * per_plane;
  const int ty0 = (int)(t / a.tiles_x) * CR_TH, tx0 = (int)(t % a.tiles_x) * CR_TW;
  const float* xp = a.x + (size_t)plane * a.H * a.W;
  const int SW = CR_TW + K - 1, SH = CR_TH + K - 1;
  for (int i = tid; i < K * K; i += CR_THREADS) sw[i] = a.taps[i];
  for (int i = tid; i < SH * SW; i += CR_THREADS) {
    const int rr = i / SW, c = i - rr * SW;
    const int gy = cr_clampi(ty0 + rr - r, a.H - 1), gx = cr_clampi(tx0 + c - r, a.W - 1);
    s[i] = xp[(size_t)gy * a.W + gx];
  }
  __syncthreads();
  const int col = tid & 63, row0 = tid >> 6;
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  for (int ky = 0; ky < K; ++ky)
    for (int kx = 0; kx < K; ++kx) {
      const float w = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(sw[ky * K + kx])));
      if (w == 0.f) continue;                                // (uniform over the workgroup)
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = fmaf(w, s[(row0 + 4 * i + ky) * SW + col + kx], acc[i]);
    }
  const int gx = tx0 + col, c = (int)(plane % (uint32_t)a.C);
  if (gx < a.W) {
    float* op = a.out + (size_t)plane * a.H * a.W;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int gy = ty0 + row0 + 4 * i;
      if (gy < a.H) op[(size_t)gy * a.W + gx] = a.clamp ? fminf(fmaxf(acc[i], a.lo[c]), a.hi[c]) : acc[i];
    }
  }
}

struct PixArgs {
  const float* x; float* out;
  int C, H, W, k, cw, ch, tiles_x, tiles_y, clamp;          // a workgroup: cw x ch cells (small), or one cell (tiles = cells)
  float lo[4], hi[4];
};

__global__ __launch_bounds__(CR_THREADS) void k_pixelate_small(PixArgs a) {
  __shared__ float cm[CR_THREADS];                           // cw * ch <= 256: a cell per thread
  const int tid = threadIdx.x, k = a.k;
  const uint32_t per_plane = (uint32_t)a.tiles_x * a.tiles_y;
  const uint32_t plane = blockIdx.x / per_plane, t = blockIdx.x - plane * per_plane;
  const int cy0 = (int)(t / a.tiles_x) * a.ch, cx0 = (int)(t % a.tiles_x) * a.cw;
  const float* xp = a.x + (size_t)plane * a.H * a.W;
  for (int i = tid; i < a.cw * a.ch; i += CR_THREADS) {
    const int cy = i / a.cw, cx = i - cy * a.cw;
    const int y0 = (cy0 + cy) * k, x0 = (cx0 + cx) * k;
    if (y0 < a.H && x0 < a.W) {
      const int y1 = y0 + k < a.H ? y0 + k : a.H, x1 = x0 + k < a.W ? x0 + k : a.W;
      float sum = 0.f;
      for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) sum += xp[(size_t)y * a.W + x];
      cm[i] = sum / (float)((y1 - y0) * (x1 - x0));
    }
  }
  __syncthreads();
  const int pw = a.cw * k, ph = a.ch * k, c = (int)(plane % (uint32_t)a.C);
  float* op = a.out + (size_t)plane * a.H * a.W;
  for (int i = tid; i < pw * ph; i += CR_THREADS) {
    const int py = i / pw, px = i - py * pw;
    const int gy = cy0 * k + py, gx = cx0 * k + px;
    if (gy < a.H && gx < a.W) {
      const float v = cm[(py / k) * a.cw + px / k];
      op[(size_t)gy * a.W + gx] = a.clamp ? fminf(fmaxf(v, a.lo[c]), a.hi[c]) : v;
    }
  }
}

__global__ __launch_bounds__(CR_THREADS) void k_pixelate_big(PixArgs a) {
  __shared__ double sd[CR_THREADS];
  const int tid = threadIdx.x, k = a.k;
  const uint32_t per_plane = (uint32_t)a.tiles_x * a.tiles_y;
  const uint32_t plane = blockIdx.x / per_plane, t = blockIdx.x - plane * per_plane;
  const int y0 = (int)(t / a.tiles_x) * k, x0 = (int)(t % a.tiles_x) * k;
  const int h = y0 + k < a.H ? k : a.H - y0, w = x0 + k < a.W ? k : a.W - x0;
  const float* xp = a.x + (size_t)plane * a.H * a.W;
  const int64_t cnt = (int64_t)h * w;
  double sum = 0.0;
  for (int64_t i = tid; i < cnt; i += CR_THREADS) {
    const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
    sum += (double)xp[(size_t)(y0 + y) * a.W + x0 + x];
  }
  sd[tid] = sum;
  __syncthreads();
  for (int s = CR_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) sd[tid] += sd[tid + s];
    __syncthreads();
  }
  const int c = (int)(plane % (uint32_t)a.C);
  float v = (float)(sd[0] / (double)cnt);
  if (a.clamp) v = fminf(fmaxf(v, a.lo[c]), a.hi[c]);
  float* op = a.out + (size_t)plane * a.H * a.W;
  for (int64_t i = tid; i < cnt; i += CR_THREADS) {
    const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
    op[(size_t)(y0 + y) * a.W + x0 + x] = v;
  }
}

// ---- the host side
thread_local char cr_msg[200];
int cr_refuse(const char* who, const char* what, int code = UVC_ERR_ARG) {
  snprintf(cr_msg, sizeof cr_msg, "%s: %s", who, what);
  return uvc_set_error_msg(code, cr_msg);
}
// the smallest float32 that is >= t: for a float32 u, u < t exactly when u < cr_ceil_f32(t)
float cr_ceil_f32(double t) {
  float f = (float)t;
  if ((double)f < t) f = nextafterf(f, INFINITY);
  return f;
}
uint64_t cr_key(uint64_t seed, uint64_t step, uint32_t site) {
  uint64_t key = seed * 0xD1342543DE82EF95ull + 0x2545F4914F6CDD1Dull;
  key ^= (step + 1) * 0x9E3779B97F4A7C15ull;
  return (key << 17 | key >> 47) ^ ((uint64_t)site + 1) * 0xC2B2AE3D27D4EB4Full;
}

// what every image call checks: n = B C H W on success
int cr_check_batch(const char* who, const uvc_corrupt_args* a, uint64_t* n) {
  if (!a || !a->x || !a->out) return cr_refuse(who, "null pointer");
  if (a->B < 1 || a->C < 1 || a->H < 1 || a->W < 1) return cr_refuse(who, "B, C, H, W must be positive");
  if (a->C > 4) return cr_refuse(who, "at most 4 channels");
  if (!(a->level >= 0.0) || !std::isfinite(a->level)) return cr_refuse(who, "the level must be non-negative and finite");
  for (int c = 0; c < a->C; ++c) {
    if (!((float)a->std[c] > 0.f) || !std::isfinite((float)a->std[c]) || !std::isfinite((float)a->mean[c])) return cr_refuse(who, "std must be positive, mean and std finite (in float32)");
    if (!(a->lo[c] <= a->hi[c])) return cr_refuse(who, "lo <= hi in every channel");
  }
  if (((uintptr_t)a->x | (uintptr_t)a->out) & 3) return cr_refuse(who, "x and out must be 4-byte aligned");
  const uint64_t chw = (uint64_t)a->C * (uint64_t)a->H * (uint64_t)a->W;
  if (chw >= 0x80000000ull) return cr_refuse(who, "an image of 2^31 elements or more", UVC_ERR_UNSUPPORTED);
  *n = chw * (uint64_t)a->B;
  return UVC_OK;
}

int cr_check_planes(const char* who, const float* x, const float* out, int64_t planes, int C, int H, int W, const float* lo, const float* hi,
                    uint32_t tiles_per_plane, unsigned* grid) {
  if (!x || !out) return cr_refuse(who, "null pointer");
  if (planes < 1 || C < 1 || H < 1 || W < 1) return cr_refuse(who, "planes, C, H, W must be positive");
  if (C > 4) return cr_refuse(who, "at most 4 channels");
  if ((!lo) != (!hi)) return cr_refuse(who, "lo and hi go together");
  if (lo)
    for (int c = 0; c < C; ++c)
      if (!(lo[c] <= hi[c])) return cr_refuse(who, "lo <= hi in every channel");
  if (((uintptr_t)x | (uintptr_t)out) & 3) return cr_refuse(who, "x and out must be 4-byte aligned");
  if ((uint64_t)H * (uint64_t)W >= 0x80000000ull) return cr_refuse(who, "a plane of 2^31 elements or more", UVC_ERR_UNSUPPORTED);
  const uint64_t blocks = (uint64_t)planes * tiles_per_plane;
  if (blocks > CR_MAX_GRID) return cr_refuse(who, "more than 2^31 - 1 workgroups", UVC_ERR_UNSUPPORTED);
  *grid = (unsigned)blocks;
  return UVC_OK;
}

}  // namespace

extern "C" int uvc_corrupt_noise(const uvc_corrupt_args* a, void* stream) {
  const char* who = "uvc_corrupt_noise";
  uint64_t n = 0;
  if (const int rc = cr_check_batch(who, a, &n)) return rc;
  if (a->kind != UVC_CORRUPT_GAUSSIAN_NOISE && a->kind != UVC_CORRUPT_SPECKLE_NOISE && a->kind != UVC_CORRUPT_IMPULSE_NOISE)
    return cr_refuse(who, "kind must be UVC_CORRUPT_GAUSSIAN_NOISE, _SPECKLE_NOISE or _IMPULSE_NOISE");
  if (a->kind == UVC_CORRUPT_IMPULSE_NOISE && a->level > 1.0) return cr_refuse(who, "impulse_noise: the level is a share, at most 1");
  if (a->index0 < 0) return cr_refuse(who, "index0 must be non-negative");
  const uint64_t chw = n / (uint64_t)a->B;
  if ((uint64_t)a->index0 > (0xffffffffffffffffull - n) / chw) return cr_refuse(who, "index0 C H W + B C H W passes 2^64");
  NoiseArgs k;
  k.x = a->x; k.out = a->out; k.n = n; k.gstart = (uint64_t)a->index0 * chw;
  k.key0 = cr_key(a->seed, a->stream_id, 0); k.key1 = cr_key(a->seed, a->stream_id, 1); k.key2 = cr_key(a->seed, a->stream_id, 2);
  k.hw = (uint32_t)a->H * (uint32_t)a->W; k.C = a->C; k.kind = a->kind;
  for (int c = 0; c < 4; ++c) {
    const bool on = c < a->C;
    const double s = on ? a->std[c] : 1.0, m = on ? a->mean[c] : 0.0;
    k.ca[c] = a->kind == UVC_CORRUPT_SPECKLE_NOISE ? (float)a->level : 0.f;
    k.cb[c] = a->kind == UVC_CORRUPT_SPECKLE_NOISE ? (float)(a->level * m / s) : (float)(a->level / s);
    k.lo[c] = on ? a->lo[c] : 0.f; k.hi[c] = on ? a->hi[c] : 0.f;
  }
  k.t_lo = cr_ceil_f32(a->level * 0.5); k.t_hi = cr_ceil_f32(a->level);
  const uint64_t quads = ((k.gstart & 3) + n + 3) / 4, blocks = (quads + CR_THREADS - 1) / CR_THREADS;
  if (blocks > CR_MAX_GRID) return cr_refuse(who, "more than 2^31 - 1 workgroups", UVC_ERR_UNSUPPORTED);
  // element e = 4 q - (gstart & 3) opens quad q: its address is 16-byte aligned when (address of x / 4 - gstart) is a multiple of 4
  const bool vec = ((((uintptr_t)a->x >> 2) - k.gstart) & 3) == 0 && ((((uintptr_t)a->out >> 2) - k.gstart) & 3) == 0;
  if (vec) k_corrupt_noise<true><<<(unsigned)blocks, CR_THREADS, 0, (hipStream_t)stream>>>(k);
  else k_corrupt_noise<false><<<(unsigned)blocks, CR_THREADS, 0, (hipStream_t)stream>>>(k);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

extern "C" int uvc_box_muller(const float* u1, const float* u2, float* z0, float* z1, int64_t n, void* stream) {
  if (!u1 || !u2 || !z0 || !z1 || n < 1) return cr_refuse("uvc_box_muller", "null pointer or n < 1");
  const int64_t blocks = (n + CR_THREADS - 1) / CR_THREADS;
  if (blocks > (int64_t)CR_MAX_GRID) return cr_refuse("uvc_box_muller", "more than 2^31 - 1 workgroups", UVC_ERR_UNSUPPORTED);
  k_box_muller<<<(unsigned)blocks, CR_THREADS, 0, (hipStream_t)stream>>>(u1, u2, z0, z1, n);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

extern "C" int uvc_corrupt_colour(const uvc_corrupt_args* a, void* stream) {
  const char* who = "uvc_corrupt_colour";
  uint64_t n = 0;
  if (const int rc = cr_check_batch(who, a, &n)) return rc;
  if (a->kind != UVC_CORRUPT_BRIGHTNESS && a->kind != UVC_CORRUPT_CONTRAST) return cr_refuse(who, "kind must be UVC_CORRUPT_BRIGHTNESS or _CONTRAST");
  const bool contrast = a->kind == UVC_CORRUPT_CONTRAST;
  if (contrast && (!a->image_mean || ((uintptr_t)a->image_mean & 3))) return cr_refuse(who, "contrast needs image_mean, float32 [B]");
  ColourArgs k;
  k.x = a->x; k.out = a->out; k.image_mean = a->image_mean;
  k.hw = (uint32_t)a->H * (uint32_t)a->W; k.C = a->C; k.a = (float)a->level;
  k.blocks_per_image = contrast ? (k.hw + 1023u) / 1024u : (k.hw + CR_THREADS - 1) / CR_THREADS;
  const uint64_t blocks = (uint64_t)k.blocks_per_image * (uint64_t)a->B * (contrast ? (uint64_t)a->C : 1ull);
  if (blocks > CR_MAX_GRID) return cr_refuse(who, "more than 2^31 - 1 workgroups", UVC_ERR_UNSUPPORTED);
  for (int c = 0; c < 4; ++c) {
    const bool on = c < a->C;
    k.dmean[c] = on ? a->mean[c] : 0.0; k.dstd[c] = on ? a->std[c] : 1.0;
    k.mean[c] = (float)k.dmean[c]; k.std[c] = (float)k.dstd[c];
    k.istd[c] = (float)(1.0 / k.dstd[c]); k.nmis[c] = (float)(-k.dmean[c] / k.dstd[c]);
    k.lo[c] = on ? a->lo[c] : 0.f; k.hi[c] = on ? a->hi[c] : 0.f;
  }
  hipStream_t st = (hipStream_t)stream;
  if (contrast) {
    k_image_mean<<<(unsigned)a->B, CR_MEAN_THREADS, 0, st>>>(k);
    UVC_CHECK_LAUNCH();
    k_contrast<<<(unsigned)blocks, CR_THREADS, 0, st>>>(k);
  } else {
    k_brightness<<<(unsigned)blocks, CR_THREADS, 0, st>>>(k);
  }
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

extern "C" int uvc_blur_separable(const float* x, float* scratch, float* out, const float* taps, int32_t R, int64_t planes, int32_t C, int32_t H,
                                  int32_t W, const float* lo, const float* hi, void* stream) {
  const char* who = "uvc_blur_separable";
  if (!scratch || !taps) return cr_refuse(who, "null pointer");
  if (R < 0 || R > CR_MAX_R) return cr_refuse(who, "the radius must lie in [0, 32]");
  if (scratch == x || scratch == out || ((uintptr_t)scratch & 3)) return cr_refuse(who, "scratch is a plane of its own, 4-byte aligned");
  for (int i = 0; i < 2 * R + 1; ++i)
    if (!std::isfinite(taps[i])) return cr_refuse(who, "a tap is not finite");
  BlurArgs k;
  k.tiles_x = H > 0 && W > 0 ? (W + CR_TW - 1) / CR_TW : 0; k.tiles_y = H > 0 && W > 0 ? (H + CR_TH - 1) / CR_TH : 0;
  unsigned grid = 0;
  if (const int rc = cr_check_planes(who, x, out, planes, C, H, W, lo, hi, (uint32_t)k.tiles_x * (uint32_t)k.tiles_y, &grid)) return rc;
  k.C = C; k.H = H; k.W = W; k.R = R;
  for (int c = 0; c < 4; ++c) { k.lo[c] = lo && c < C ? lo[c] : 0.f; k.hi[c] = hi && c < C ? hi[c] : 0.f; }
  for (int i = 0; i < 2 * CR_MAX_R + 1; ++i) k.w[i] = i < 2 * R + 1 ? taps[i] : 0.f;
  hipStream_t st = (hipStream_t)stream;
  k.x = x; k.out = scratch; k.clamp = 0;
  k_blur_pass<false><<<grid, CR_THREADS, 0, st>>>(k);
  UVC_CHECK_LAUNCH();
  k.x = scratch; k.out = out; k.clamp = lo != nullptr;
  k_blur_pass<true><<<grid, CR_THREADS, 0, st>>>(k);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

extern "C" int uvc_stencil2d(const float* x, float* out, const float* taps, int32_t K, int64_t planes, int32_t C, int32_t H, int32_t W, const float* lo,
                             const float* hi, void* stream) {
  const char* who = "uvc_stencil2d";
  if (!taps || ((uintptr_t)taps & 3)) return cr_refuse(who, "null or misaligned taps");
  if (K < 3 || K > CR_MAX_K || K % 2 == 0) return cr_refuse(who, "K must be odd and lie in [3, 25]");
  if (x == out) return cr_refuse(who, "out must not be x");
  StencilArgs k;
  k.tiles_x = H > 0 && W > 0 ? (W + CR_TW - 1) / CR_TW : 0; k.tiles_y = H > 0 && W > 0 ? (H + CR_TH - 1) / CR_TH : 0;
  unsigned grid = 0;
  if (const int rc = cr_check_planes(who, x, out, planes, C, H, W, lo, hi, (uint32_t)k.tiles_x * (uint32_t)k.tiles_y, &grid)) return rc;
  k.x = x; k.out = out; k.taps = taps; k.C = C; k.H = H; k.W = W; k.K = K; k.clamp = lo != nullptr;
  for (int c = 0; c < 4; ++c) { k.lo[c] = lo && c < C ? lo[c] : 0.f; k.hi[c] = hi && c < C ? hi[c] : 0.f; }
  k_stencil2d<<<grid, CR_THREADS, 0, (hipStream_t)stream>>>(k);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

extern "C" int uvc_pixelate(const float* x, float* out, int32_t kk, int64_t planes, int32_t C, int32_t H, int32_t W, const float* lo, const float* hi,
                            void* stream) {
  const char* who = "uvc_pixelate";
  if (kk < 1) return cr_refuse(who, "the cell width must be at least 1");
  if (x == out) return cr_refuse(who, "out must not be x");
  PixArgs k;
  const bool small = kk <= CR_PIX_SMALL;
  k.k = kk; k.cw = small ? 128 / kk : 1; k.ch = small ? CR_THREADS / k.cw : 1;   // 128 pixels wide, 256 cells or fewer
  const int64_t cells_x = H > 0 && W > 0 ? ((int64_t)W + kk - 1) / kk : 0, cells_y = H > 0 && W > 0 ? ((int64_t)H + kk - 1) / kk : 0;
  k.tiles_x = (int)((cells_x + k.cw - 1) / k.cw); k.tiles_y = (int)((cells_y + k.ch - 1) / k.ch);
  unsigned grid = 0;
  if (const int rc = cr_check_planes(who, x, out, planes, C, H, W, lo, hi, (uint32_t)k.tiles_x * (uint32_t)k.tiles_y, &grid)) return rc;
  k.x = x; k.out = out; k.C = C; k.H = H; k.W = W; k.clamp = lo != nullptr;
  for (int c = 0; c < 4; ++c) { k.lo[c] = lo && c < C ? lo[c] : 0.f; k.hi[c] = hi && c < C ? hi[c] : 0.f; }
  if (small) k_pixelate_small<<<grid, CR_THREADS, 0, (hipStream_t)stream>>>(k);
  else k_pixelate_big<<<grid, CR_THREADS, 0, (hipStream_t)stream>>>(k);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}
