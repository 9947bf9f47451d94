// Image input step (include/uvc_data.h): PIL's antialiased bilinear or bicubic resample of a ragged batch of uint8 HWC images, then
// ToTensor + Normalize, into a [B, 3, S, S] batch.  The sources are contiguous uploads (uvc_image_prep) or crop windows inside the
// images of a store that stays in device memory (uvc_image_prep_crops); the kernels are templates on the args struct, whose
// descriptor type says which.  Three launches per batch:
//   k_prep_coeffs   one thread per (image, output column or row): PIL's precompute_coeffs + normalize_coeffs_8bpc in float64
//   k_prep_pass1    the first pass into a uint8 intermediate: horizontal, one thread per (covered source row, output column), or, for
//                   the tall sources Image.resize shrinks vertically first, vertical, one thread per (output row, covered source column)
//   k_prep_pass2    one thread per (image, output row, output column): the other axis, flip, normalise, and the store its policy names:
//                   the NCHW batch, or (uvc_image_prep_patches) the patch rows uvc_patchify would make of it, four columns per thread
// Built with -ffp-contract=off (uvc_amd/build.py): the float64 coefficient arithmetic must round like the C it mirrors.
//
// The launch's filter (args.filter) picks the weight function and its support in k_prep_coeffs and the tap count desc_ok expects;
// the passes are the same code for both.  Bicubic weights are negative in places, so an accumulator can leave [0, 255 << 22] and
// clip8 between and after the passes does work.  int32 holds every partial sum, as PIL's `int` does: |partial sum| <= 255 * 2^22 *
// sum|w| + 2^21, which stays below 2^31 while sum|w| < 2.007, and the normalised bicubic weights of one output pixel have sum|w| = 1.25
// at phase 1/2 of an upscale (-1/16, 9/16, 9/16, -1/16) and stay below 1.3 at the other scales and at the edges that cut taps off
// (tests/test_image_bicubic_cpu.py sweeps them).
#include "common.h"
#include "uvc_data.h"
#include "uvc_kernels.h"                 // UVC_F32 / UVC_BF16, the patch rows' element types

#include <math.h>

namespace {

constexpr int kPrecisionBits = 22;     // PIL Resample.c PRECISION_BITS (8-bit images)
constexpr int kMaxSide = 1 << 16;      // source and resize sides: exact as float32 box coordinates, int32 index products stay small
constexpr int kMaxS = 4096;

// precompute_coeffs, per axis, with box (0, in): in0 = 0.0 so `in0 + v` is v exactly, and in1 - in0 = in.
struct AxisFilter {
  double scale, support, ss;
  int ksize;
};

__host__ __device__ inline bool filter_ok(int filter) { return filter == UVC_IMAGE_FILTER_BILINEAR || filter == UVC_IMAGE_FILTER_BICUBIC; }

// PIL's filter support: BILINEAR 1.0, BICUBIC 2.0
__host__ __device__ inline int filter_support(int filter) { return filter == UVC_IMAGE_FILTER_BICUBIC ? 2 : 1; }

__host__ __device__ inline AxisFilter axis_filter(int in_size, int out_size, int filter) {
  AxisFilter f;
  f.scale = (double)in_size / (double)out_size;
  const double fs = f.scale > 1.0 ? f.scale : 1.0;
  f.support = (double)filter_support(filter) * fs;
  f.ksize = (int)ceil(f.support) * 2 + 1;
  f.ss = 1.0 / fs;
  return f;
}

__host__ __device__ inline void axis_bounds(const AxisFilter& f, int in_size, int xx, double& center, int& xmin, int& n) {
  center = ((double)xx + 0.5) * f.scale;
  int lo = (int)(center - f.support + 0.5);
  if (lo < 0) lo = 0;
  int hi = (int)(center + f.support + 0.5);
  if (hi > in_size) hi = in_size;
  xmin = lo;
  n = hi - lo;
}

__device__ inline double tri(double x) {
  if (x < 0.0) x = -x;
  if (x < 1.0) return 1.0 - x;
  return 0.0;
}

// PIL Resample.c bicubic_filter (a = -0.5), in its order of operations
__device__ inline double cubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// Is k the ksize = 2 ceil(support) + 1 of this axis under this filter?  In integers: with f = the filter's support, ceil(f max(in / out,
// 1)) = max(f, ceil(f in / out)), and the float64 quotient cannot cross an integer the exact one does not (f in / out is an integer
// or at least 1 / out >= 2^-16 away from one).  The host query holds its own float64 ksize to this before it hands it out.
__host__ __device__ inline bool ksize_ok(int k, int in_size, int out_size, int filter) {
  const int64_t f = filter_support(filter), c = (k - 1) >> 1;
  if (k < 1 || !(k & 1) || c < f) return false;
  if (f * in_size > c * out_size) return false;
  return c == f || (c - 1) * out_size < f * in_size;
}

__host__ __device__ inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// per-image workspace: h bounds int32[2S] | h taps int32[S*kh] | v bounds int32[2S] | v taps int32[S*kv] | (16-aligned) uint8 span*S*3
// (order 0: [span source rows][S columns][3]; order 1: [S rows][span source columns][3])
struct WsLayout {
  int64_t hb, hk, vb, vk, inter, total;
};

__host__ __device__ inline WsLayout ws_layout(int S, int kh, int kv, int span) {
  WsLayout L;
  L.hb = 0;
  L.hk = L.hb + 8 * (int64_t)S;
  L.vb = L.hk + 4 * (int64_t)S * kh;
  L.vk = L.vb + 8 * (int64_t)S;
  L.inter = align16(L.vk + 4 * (int64_t)S * kv);
  L.total = align16(L.inter + (int64_t)span * S * 3);
  return L;
}

// Source accessors: what the passes resample is a window of src_h x src_w pixels whose first byte is src_base() into `src` and whose
// rows lie src_row_bytes() apart.  uvc_image_desc: the whole contiguous upload.  uvc_image_crop_desc: a crop window inside an image
// of a resident store, rows at the stored image's stride.  Everything else (resize, window, flip, the "out" fields) has the same
// names in both descriptors, so one set of kernels serves both.
__host__ __device__ inline int src_h(const uvc_image_desc& d) { return d.src_h; }
__host__ __device__ inline int src_w(const uvc_image_desc& d) { return d.src_w; }
__host__ __device__ inline int64_t src_base(const uvc_image_desc& d) { return d.src_offset; }
__host__ __device__ inline int64_t src_row_bytes(const uvc_image_desc& d) { return (int64_t)d.src_w * 3; }
__host__ __device__ inline bool src_sides_ok(const uvc_image_desc& d) {
  return d.src_h >= 1 && d.src_w >= 1 && d.src_h <= kMaxSide && d.src_w <= kMaxSide;
}
__host__ __device__ inline bool src_fits(const uvc_image_desc& d, int64_t src_bytes) {
  return d.src_offset >= 0 && d.src_offset <= src_bytes - (int64_t)d.src_h * d.src_w * 3;
}

__host__ __device__ inline int src_h(const uvc_image_crop_desc& d) { return d.crop_h; }
__host__ __device__ inline int src_w(const uvc_image_crop_desc& d) { return d.crop_w; }
__host__ __device__ inline int64_t src_base(const uvc_image_crop_desc& d) {
  return d.src_offset + ((int64_t)d.crop_y * d.img_w + d.crop_x) * 3;
}
__host__ __device__ inline int64_t src_row_bytes(const uvc_image_crop_desc& d) { return (int64_t)d.img_w * 3; }
__host__ __device__ inline bool src_sides_ok(const uvc_image_crop_desc& d) {   // the crop lies inside its image
  if (d.img_h < 1 || d.img_w < 1 || d.img_h > kMaxSide || d.img_w > kMaxSide) return false;
  if (d.crop_h < 1 || d.crop_w < 1 || d.crop_y < 0 || d.crop_x < 0) return false;
  return d.crop_y <= d.img_h - d.crop_h && d.crop_x <= d.img_w - d.crop_w;
}
__host__ __device__ inline bool src_fits(const uvc_image_crop_desc& d, int64_t src_bytes) {   // the image lies inside the store
  return d.src_offset >= 0 && d.src_offset <= src_bytes - (int64_t)d.img_h * d.img_w * 3;
}

// The device trusts nothing it did not check: an image whose descriptor does not fit the buffers it was given, or whose tap counts
// are not those of the launch's filter (descriptors completed for the other one), is skipped.
template <class Desc, class Args>
__device__ inline bool desc_ok(const Desc& d, const Args& a) {
  if (!src_sides_ok(d)) return false;
  if (d.resize_h < a.S || d.resize_w < a.S || d.resize_h > kMaxSide || d.resize_w > kMaxSide) return false;
  if (d.win_y < 0 || d.win_x < 0 || d.win_y > d.resize_h - a.S || d.win_x > d.resize_w - a.S) return false;
  if (!ksize_ok(d.kh, src_w(d), d.resize_w, a.filter) || !ksize_ok(d.kv, src_h(d), d.resize_h, a.filter)) return false;   // tables of another filter
  if (d.span < 1 || d.span0 < 0 || (d.order != 0 && d.order != 1)) return false;
  if (d.span0 > (d.order ? src_w(d) : src_h(d)) - d.span) return false;
  if (!src_fits(d, a.src_bytes)) return false;
  const WsLayout L = ws_layout(a.S, d.kh, d.kv, d.span);
  if (d.ws_offset < 0 || (d.ws_offset & 15) || d.ws_offset > a.workspace_bytes - L.total) return false;
  return true;
}

template <class Args>
__global__ void __launch_bounds__(256) k_prep_coeffs(Args a) {
  const int b = blockIdx.y;
  const auto d = a.desc[b];
  if (!desc_ok(d, a)) return;
  const int S = a.S;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * S) return;
  const bool horiz = t < S;
  const int i = horiz ? t : t - S;
  const int in_size = horiz ? src_w(d) : src_h(d);
  const int out_size = horiz ? d.resize_w : d.resize_h;
  const int k = horiz ? d.kh : d.kv;
  const AxisFilter f = axis_filter(in_size, out_size, a.filter);
  const bool bicubic = a.filter == UVC_IMAGE_FILTER_BICUBIC;
  double center;
  int xmin, n;
  axis_bounds(f, in_size, (horiz ? d.win_x : d.win_y) + i, center, xmin, n);
  if (n > k) n = k;                    // cannot happen (n <= 2 ceil(support) + 1); keeps the writes inside the table
  if (n < 0) n = 0;
  const WsLayout L = ws_layout(S, d.kh, d.kv, d.span);
  uint8_t* ws = (uint8_t*)a.workspace + d.ws_offset;
  int32_t* bounds = (int32_t*)(ws + (horiz ? L.hb : L.vb)) + 2 * i;
  int32_t* kk = (int32_t*)(ws + (horiz ? L.hk : L.vk)) + (int64_t)i * k;
  double ww = 0.0;
  for (int x = 0; x < n; ++x) {
    const double t = (x + xmin - center + 0.5) * f.ss;
    ww += bicubic ? cubic(t) : tri(t);
  }
  for (int x = 0; x < k; ++x) {
    int32_t q = 0;
    if (x < n) {
      const double t = (x + xmin - center + 0.5) * f.ss;
      double w = bicubic ? cubic(t) : tri(t);
      if (ww != 0.0) w /= ww;
      q = w < 0 ? (int32_t)(-0.5 + w * (1 << kPrecisionBits)) : (int32_t)(0.5 + w * (1 << kPrecisionBits));
    }
    kk[x] = q;
  }
  int32_t lo = xmin;
  if (horiz == (d.order == 1)) {       // the second pass's taps index the intermediate, whose first line is source line span0
    lo -= d.span0;
    if (lo < 0 || lo + n > d.span) {   // cannot happen (span0 / span come from the same bounds); never read outside the intermediate
      lo = 0;
      n = 0;
    }
  }
  bounds[0] = lo;
  bounds[1] = n;
}

__device__ inline uint8_t clip8(int32_t v) {
  if (v >= (1 << kPrecisionBits << 8)) return 255;
  if (v <= 0) return 0;
  return (uint8_t)(v >> kPrecisionBits);
}

__device__ inline void mac3(const uint8_t* s, int64_t stride, const int32_t* k, int n, uint8_t* u) {
  int32_t a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
  for (int x = 0; x < n; ++x) {
    const int32_t w = k[x];
    const uint8_t* q = s + (int64_t)x * stride;
    a0 += (int32_t)q[0] * w;
    a1 += (int32_t)q[1] * w;
    a2 += (int32_t)q[2] * w;
  }
  u[0] = clip8(a0);
  u[1] = clip8(a1);
  u[2] = clip8(a2);
}

template <class Args>
__global__ void __launch_bounds__(256) k_prep_pass1(Args a) {
  const int b = blockIdx.y;
  const auto d = a.desc[b];
  if (!desc_ok(d, a)) return;
  const int S = a.S;
  const WsLayout L = ws_layout(S, d.kh, d.kv, d.span);
  uint8_t* ws = (uint8_t*)a.workspace + d.ws_offset;
  uint8_t* inter = ws + L.inter;
  const uint8_t* src = a.src + src_base(d);
  const int64_t row_bytes = src_row_bytes(d);
  const int64_t total = (int64_t)d.span * S;
  if (d.order == 0) {                  // horizontal: intermediate [span rows][S][3], row r = source row span0 + r
    const int32_t* hb = (const int32_t*)(ws + L.hb);
    const int32_t* hk = (const int32_t*)(ws + L.hk);
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (int64_t)gridDim.x * blockDim.x) {
      const int r = (int)(p / S), c = (int)(p - (int64_t)r * S);
      mac3(src + (int64_t)(d.span0 + r) * row_bytes + (int64_t)hb[2 * c] * 3, 3, hk + (int64_t)c * d.kh, hb[2 * c + 1], inter + p * 3);
    }
  } else {                             // vertical: intermediate [S][span columns][3], column c = source column span0 + c
    const int32_t* vb = (const int32_t*)(ws + L.vb);
    const int32_t* vk = (const int32_t*)(ws + L.vk);
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (int64_t)gridDim.x * blockDim.x) {
      const int r = (int)(p / d.span), c = (int)(p - (int64_t)r * d.span);
      mac3(src + (int64_t)vb[2 * r] * row_bytes + (int64_t)(d.span0 + c) * 3, row_bytes, vk + (int64_t)r * d.kv, vb[2 * r + 1], inter + p * 3);
    }
  }
}

// Store policies of k_prep_pass2.  A thread owns kPixels consecutive output pixels of one output row; the policy says where their three
// channels go.  StoreImage is the [B, 3, S, S] batch (float32 or uint8, args.out_dtype).  StorePatches writes the rows uvc_patchify would
// make of that batch, [B * (S/P)^2, 3 * P * P] of T: pixel (b, ch, y, x) at row b (S/P)^2 + (y/P)(S/P) + x/P, column ch P P + (y%P) P + x%P,
// with uvc_patchify's cast.  A patch row is contiguous only along x, P elements at a time, so a thread owns V = 4 pixels of such a run
// (P % 4 == 0: one 8-byte bf16 or 16-byte float32 store per channel, uvc_patchify's own width; a 16-pixel run is four neighbouring lanes)
// or, for the other patch sizes, one pixel.
struct StoreImage {
  static constexpr int kPixels = 1;
  static constexpr bool kReadsOutDtype = true;
  template <class Args>
  __device__ __forceinline__ void operator()(const Args& a, int b, int S, int64_t p, int, int, const uint8_t (*u)[3]) const {
    const int64_t plane = (int64_t)S * S;
    const int64_t base = (int64_t)b * 3 * plane + p;
    if (a.out_dtype == UVC_IMAGE_OUT_U8) {
      uint8_t* o = (uint8_t*)a.out + base;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) o[ch * plane] = u[0][ch];
    } else {
      float* o = (float*)a.out + base;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) o[ch * plane] = __fdiv_rn(__fdiv_rn((float)u[0][ch], 255.0f) - a.mean[ch], a.std[ch]);
    }
  }
};

template <typename T, int V>
struct StorePatches {
  static_assert(V == 1 || V == 4, "pixels per thread");
  static constexpr int kPixels = V;
  static constexpr bool kReadsOutDtype = false;
  int P;                               // S % P == 0 and P % V == 0 (uvc_image_prep_patches)
  template <class Args>
  __device__ __forceinline__ void operator()(const Args& a, int b, int S, int64_t, int r, int c, const uint8_t (*u)[3]) const {
    const int G = S / P, py = r / P, px = c / P;
    const int PP = P * P;
    const int64_t row = ((int64_t)b * G + py) * G + px;
    T* o = (T*)a.out + row * (3 * (int64_t)PP) + (r - py * P) * P + (c - px * P);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float v[V];
#pragma unroll
      for (int i = 0; i < V; ++i) v[i] = __fdiv_rn(__fdiv_rn((float)u[i][ch], 255.0f) - a.mean[ch], a.std[ch]);
      T* q = o + ch * PP;
      if constexpr (V == 1) {
        ElemIO<T>::store(q, v[0]);
      } else if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<f32x4*>(q) = f32x4{v[0], v[1], v[2], v[3]};
      } else {
        u32x2 w;
        w[0] = pack_bf16x2(v[0], v[1]);
        w[1] = pack_bf16x2(v[2], v[3]);
        *reinterpret_cast<u32x2*>(q) = w;
      }
    }
  }
};

template <class Args, class Store>
__global__ void __launch_bounds__(256) k_prep_pass2(Args a, Store store) {
  constexpr int V = Store::kPixels;
  const int b = blockIdx.y;
  const auto d = a.desc[b];
  if (!desc_ok(d, a)) return;
  const int S = a.S;
  const WsLayout L = ws_layout(S, d.kh, d.kv, d.span);
  const uint8_t* ws = (const uint8_t*)a.workspace + d.ws_offset;
  const int32_t* hb = (const int32_t*)(ws + L.hb);
  const int32_t* hk = (const int32_t*)(ws + L.hk);
  const int32_t* vb = (const int32_t*)(ws + L.vb);
  const int32_t* vk = (const int32_t*)(ws + L.vk);
  const uint8_t* inter = ws + L.inter;
  const int64_t plane = (int64_t)S * S;
  for (int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * V; p < plane; p += (int64_t)gridDim.x * blockDim.x * V) {
    const int r = (int)(p / S), c = (int)(p - (int64_t)r * S);   // S % V == 0: the V pixels share the row
    uint8_t u[V][3];
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const int cc = d.flip ? S - 1 - (c + i) : c + i;
      if (d.order == 0)                // vertical down intermediate column cc
        mac3(inter + (int64_t)vb[2 * r] * S * 3 + (int64_t)cc * 3, (int64_t)S * 3, vk + (int64_t)r * d.kv, vb[2 * r + 1], u[i]);
      else                             // horizontal along intermediate row r
        mac3(inter + ((int64_t)r * d.span + hb[2 * cc]) * 3, 3, hk + (int64_t)cc * d.kh, hb[2 * cc + 1], u[i]);
    }
    store(a, b, S, p, r, c, u);             // p = r S + c
  }
}

// workgroups per image and pass: about one pixel per thread for the S x S output (the first pass strides over its span), or one
// thread per `pixels` of them
inline int pass_blocks(int S, int pixels = 1) {
  const int64_t g = ((int64_t)S * S / pixels + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 1024 ? 1024 : g));
}

// The host query of both entries: checks, the "out" fields, the workspace layout.  `msg` holds the entry's own wording of the refusals.
struct WorkspaceMsgs {
  const char *arg, *sides, *resize, *window, *fits, *span, *ksize;
};

template <class Desc>
int prep_workspace(Desc* desc, int32_t B, int32_t S, int64_t src_bytes, int32_t filter, int64_t* bytes, const WorkspaceMsgs& msg) {
  if (!desc || !bytes || B < 1 || B > 65535 || S < 1 || S > kMaxS || src_bytes < 0 || !filter_ok(filter))
    return uvc_set_error_msg(UVC_ERR_ARG, msg.arg);
  int64_t off = 0;
  for (int32_t b = 0; b < B; ++b) {
    Desc& d = desc[b];
    if (!src_sides_ok(d)) return uvc_set_error_msg(UVC_ERR_ARG, msg.sides);
    if (d.resize_h < S || d.resize_w < S || d.resize_h > kMaxSide || d.resize_w > kMaxSide) return uvc_set_error_msg(UVC_ERR_ARG, msg.resize);
    if (d.win_y < 0 || d.win_x < 0 || d.win_y > d.resize_h - S || d.win_x > d.resize_w - S) return uvc_set_error_msg(UVC_ERR_ARG, msg.window);
    if (!src_fits(d, src_bytes)) return uvc_set_error_msg(UVC_ERR_ARG, msg.fits);
    const int h = src_h(d), w = src_w(d);
    const AxisFilter fh = axis_filter(w, d.resize_w, filter), fv = axis_filter(h, d.resize_h, filter);
    if (!ksize_ok(fh.ksize, w, d.resize_w, filter) || !ksize_ok(fv.ksize, h, d.resize_h, filter))   // cannot happen (see ksize_ok)
      return uvc_set_error_msg(UVC_ERR_UNSUPPORTED, msg.ksize);
    // Image.resize: `if self.size[1] > self.size[0] * 100 and size[1] < self.size[1]` resizes vertically, then horizontally
    // (on the size of what is resized: for a crop window, the crop's, as after Image.crop)
    d.order = (h > (int64_t)w * 100 && d.resize_h < h) ? 1 : 0;
    const AxisFilter& f1 = d.order ? fh : fv;          // the first pass covers the lines the SECOND pass's window reads
    const int in1 = d.order ? w : h, w1 = d.order ? d.win_x : d.win_y;
    double c;
    int y0, n0, y1, n1;
    axis_bounds(f1, in1, w1, c, y0, n0);
    axis_bounds(f1, in1, w1 + S - 1, c, y1, n1);
    d.kh = fh.ksize;
    d.kv = fv.ksize;
    d.span0 = y0;
    d.span = y1 + n1 - y0;
    if (d.span < 1 || d.span0 + d.span > in1) return uvc_set_error_msg(UVC_ERR_ARG, msg.span);
    d.ws_offset = off;
    off += ws_layout(S, d.kh, d.kv, d.span).total;
  }
  *bytes = off;
  return UVC_OK;
}

template <class Args, class Store>
int prep_launch(const Args* a, Store store, void* stream, const char* null_msg, const char* arg_msg, const char* align_msg) {
  if (!a || !a->src || !a->desc || !a->workspace || !a->out) return uvc_set_error_msg(UVC_ERR_ARG, null_msg);
  if (a->B < 1 || a->B > 65535 || a->S < 1 || a->S > kMaxS ||
      (Store::kReadsOutDtype && a->out_dtype != UVC_IMAGE_OUT_F32 && a->out_dtype != UVC_IMAGE_OUT_U8) || !filter_ok(a->filter))
    return uvc_set_error_msg(UVC_ERR_ARG, arg_msg);
  if (((uintptr_t)a->workspace & 15) || a->workspace_bytes < 0 || a->src_bytes < 0) return uvc_set_error_msg(UVC_ERR_ARG, align_msg);
  hipStream_t st = (hipStream_t)stream;
  const Args args = *a;
  k_prep_coeffs<Args><<<dim3((2 * args.S + 255) / 256, args.B), 256, 0, st>>>(args);
  k_prep_pass1<Args><<<dim3(pass_blocks(args.S), args.B), 256, 0, st>>>(args);
  k_prep_pass2<Args, Store><<<dim3(pass_blocks(args.S, Store::kPixels), args.B), 256, 0, st>>>(args, store);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

int image_workspace(uvc_image_desc* desc, int32_t B, int32_t S, int64_t src_bytes, int32_t filter, int64_t* bytes) {
  static const WorkspaceMsgs msg = {"uvc_image_prep_workspace: bad argument (1 <= B <= 65535, 1 <= S <= 4096, filter bilinear or bicubic)",
                                    "uvc_image_prep_workspace: source sides must lie in [1, 65536]",
                                    "uvc_image_prep_workspace: resize sides must lie in [S, 65536]",
                                    "uvc_image_prep_workspace: the S x S window leaves the resized image",
                                    "uvc_image_prep_workspace: an image reaches past the source buffer",
                                    "uvc_image_prep_workspace: empty span",
                                    "uvc_image_prep_workspace: tap count disagrees with its integer form"};
  return prep_workspace(desc, B, S, src_bytes, filter, bytes, msg);
}

int crops_workspace(uvc_image_crop_desc* desc, int32_t B, int32_t S, int64_t store_bytes, int32_t filter, int64_t* bytes) {
  static const WorkspaceMsgs msg = {"uvc_image_prep_crops_workspace: bad argument (1 <= B <= 65535, 1 <= S <= 4096, filter bilinear or bicubic)",
                                    "uvc_image_prep_crops_workspace: image sides must lie in [1, 65536] and the crop inside its image",
                                    "uvc_image_prep_crops_workspace: resize sides must lie in [S, 65536]",
                                    "uvc_image_prep_crops_workspace: the S x S window leaves the resized crop",
                                    "uvc_image_prep_crops_workspace: an image reaches past the store",
                                    "uvc_image_prep_crops_workspace: empty span",
                                    "uvc_image_prep_crops_workspace: tap count disagrees with its integer form"};
  return prep_workspace(desc, B, S, store_bytes, filter, bytes, msg);
}

template <typename T>
int patches_launch(const uvc_image_prep_args* a, int32_t P, void* stream) {
  static const char *null_msg = "uvc_image_prep_patches: null pointer", *arg_msg = "uvc_image_prep_patches: bad B, S or filter",
                    *align_msg = "uvc_image_prep_patches: workspace must be 16-byte aligned";
  if (P % 4 == 0) return prep_launch(a, StorePatches<T, 4>{P}, stream, null_msg, arg_msg, align_msg);
  return prep_launch(a, StorePatches<T, 1>{P}, stream, null_msg, arg_msg, align_msg);
}

}  // namespace

extern "C" int uvc_image_prep_workspace(uvc_image_desc* desc, int32_t B, int32_t S, int64_t src_bytes, int64_t* bytes) {
  return image_workspace(desc, B, S, src_bytes, UVC_IMAGE_FILTER_BILINEAR, bytes);
}

extern "C" int uvc_image_prep_workspace_filter(uvc_image_desc* desc, int32_t B, int32_t S, int64_t src_bytes, int32_t filter, int64_t* bytes) {
  return image_workspace(desc, B, S, src_bytes, filter, bytes);
}

extern "C" int uvc_image_prep(const uvc_image_prep_args* a, void* stream) {
  return prep_launch(a, StoreImage{}, stream, "uvc_image_prep: null pointer", "uvc_image_prep: bad B, S, out_dtype or filter",
                     "uvc_image_prep: workspace must be 16-byte aligned");
}

extern "C" int uvc_image_prep_patches(const uvc_image_prep_args* a, int32_t P, int32_t dtype, void* stream) {
  if (dtype != UVC_F32 && dtype != UVC_BF16) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_image_prep_patches: dtype must be UVC_F32 or UVC_BF16");
  if (!a || P <= 0 || a->S % P) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_image_prep_patches: the patch size must be positive and divide S");
  if ((uintptr_t)a->out & 15) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_image_prep_patches: out must be 16-byte aligned");
  return dtype == UVC_F32 ? patches_launch<float>(a, P, stream) : patches_launch<bf16_t>(a, P, stream);
}

extern "C" int uvc_image_prep_crops_workspace(uvc_image_crop_desc* desc, int32_t B, int32_t S, int64_t store_bytes, int64_t* bytes) {
  return crops_workspace(desc, B, S, store_bytes, UVC_IMAGE_FILTER_BILINEAR, bytes);
}

extern "C" int uvc_image_prep_crops_workspace_filter(uvc_image_crop_desc* desc, int32_t B, int32_t S, int64_t store_bytes, int32_t filter,
                                                     int64_t* bytes) {
  return crops_workspace(desc, B, S, store_bytes, filter, bytes);
}

extern "C" int uvc_image_prep_crops(const uvc_image_prep_crops_args* a, void* stream) {
  return prep_launch(a, StoreImage{}, stream, "uvc_image_prep_crops: null pointer", "uvc_image_prep_crops: bad B, S, out_dtype or filter",
                     "uvc_image_prep_crops: workspace must be 16-byte aligned");
}
