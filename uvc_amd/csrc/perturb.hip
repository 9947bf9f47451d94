// Perturbation tests of relevance maps (python -m uvc_amd.compact_perturb) for gfx950: the per-image removal order of the patches, the K
// perturbed copies of a batch's patch rows, and the read-out of one class's probability per logit row.  Three small kernels that sit
// between two forwards; no atomics, one writer per output element, fixed reduction trees: the same bits on a repeat and in any batch.
#include "common.h"
#include "../../include/uvc_kernels.h"

namespace {

constexpr int MAX_PATCHES = 1024;          // the engine's patch limit (LONG_MAX_N of attention.hip less the readout tokens)

// ---------------------------------------------------------------------------- removal order (uvc_patch_rank)
// A float as an unsigned key whose order is the removal order: "j before p" <=> key_j < key_p, ties by index.  The usual monotone map
// (negative: all bits flipped; else the sign bit set) after -0 became +0; descending flips it once more.  Numbers land in
// [0x007fffff, 0xff800000] in both directions, so 0xffffffff is free for NaN: after every number, NaNs among themselves by index.
__device__ __forceinline__ uint32_t rank_key(float s, int descending) {
  uint32_t u = __float_as_uint(s);                           // on the bits: no float mode (denormals, fast math) has a say
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  if ((u << 1) == 0) u = 0;                                  // -0 is +0
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return descending ? ~u : u;
}

// one workgroup per image, its np keys in LDS; a thread counts the predecessors of patches tid, tid + T, ... (np^2 comparisons, every
// LDS read a broadcast).  T = np rounded up to a wave, at most 256.
__global__ __launch_bounds__(256) void k_patch_rank(const float* __restrict__ scores, int ld, int offset, int np, int descending,
                                                    int32_t* __restrict__ rank) {
  __shared__ uint32_t keys[MAX_PATCHES];
  const float* s = scores + (size_t)blockIdx.x * ld + offset;
  for (int p = threadIdx.x; p < np; p += blockDim.x) keys[p] = rank_key(s[p], descending);
  __syncthreads();
  for (int p = threadIdx.x; p < np; p += blockDim.x) {
    const uint32_t kp = keys[p];
    int before = 0;
    for (int j = 0; j < p; ++j) before += keys[j] <= kp;     // j < p: a tie goes to j
    for (int j = p + 1; j < np; ++j) before += keys[j] < kp;
    rank[(size_t)blockIdx.x * np + p] = before;
  }
}

// ---------------------------------------------------------------------------- perturbed patch rows (uvc_patch_rows_perturb)
// V: what one lane moves (u32x4 on the 16-byte path, one element otherwise); per = V's per source row.  Lane i of the flat index takes
// source item i, reads it once, and writes item i of every step: consecutive lanes write consecutive items of one output row, and
// the next row follows without a gap.  A removed row is SELECTED to zero bits (+0.0 in both types), never multiplied.  Offsets in size_t.
template <typename V>
__global__ __launch_bounds__(256) void k_perturb_rows(const V* __restrict__ rows, const int32_t* __restrict__ rank,
                                                      const int32_t* __restrict__ counts, int nsteps, int np, size_t total, uint32_t per,
                                                      V* __restrict__ out) {
  const bool narrow = total <= 0xffffffffull;                // (uniform) a 32-bit division where the index allows it
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t row = narrow ? (size_t)((uint32_t)i / per) : i / per;
    const V v = rows[i];
    const int r = rank[row];
    V zero;
    __builtin_memset(&zero, 0, sizeof(V));
    for (int k = 0; k < nsteps; ++k) {
      const int c = min(max(counts[k], 0), np);
      out[(size_t)k * total + i] = r >= c ? v : zero;
    }
  }
}

// ---------------------------------------------------------------------------- one class's probability per row (uvc_logits_target)
__device__ __forceinline__ float block_reduce(float v, float* sh, bool is_max) {   // loss_optim.hip's tree: wave butterfly, then the waves in order
  v = is_max ? wave_max(v) : wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  float r = sh[0];
  for (int i = 1; i < (int)(blockDim.x >> 6); ++i) r = is_max ? fmaxf(r, sh[i]) : r + sh[i];
  return r;
}

// one workgroup per row, k_logits_topk's max and sum (same trees, same bits); the first column that holds the maximum is a min over ints
__global__ __launch_bounds__(256) void k_logits_target(const float* __restrict__ logits, int ld, int n, const int32_t* __restrict__ target,
                                                       int period, float* __restrict__ prob, int32_t* __restrict__ hit) {
  __shared__ float sh[4];
  __shared__ int shi[4];
  const float* o = logits + (size_t)blockIdx.x * ld;
  float mx = -INFINITY;
  for (int c = threadIdx.x; c < n; c += 256) mx = fmaxf(mx, o[c]);
  mx = block_reduce(mx, sh, true);
  float se = 0.f;
  int first = 0x7fffffff;
  for (int c = threadIdx.x; c < n; c += 256) {
    const float v = o[c];
    se += expf(v - mx);
    if (v == mx) first = min(first, c);
  }
  se = block_reduce(se, sh, false);
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) first = min(first, __shfl_xor(first, s, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) shi[threadIdx.x >> 6] = first;
  __syncthreads();
  if (threadIdx.x == 0) {
    first = min(min(shi[0], shi[1]), min(shi[2], shi[3]));
    const int t = min(max(target[blockIdx.x % period], 0), n - 1);
    prob[blockIdx.x] = __fdiv_rn(expf(o[t] - mx), se);
    hit[blockIdx.x] = first == t;
  }
}

}  // namespace

extern "C" int uvc_patch_rank(const float* scores, int32_t B, int32_t ld, int32_t offset, int32_t np, int32_t descending, int32_t* rank,
                              void* stream) {
  if (!scores || !rank) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_patch_rank: null pointer");
  if (B <= 0) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_patch_rank: B <= 0");
  if (np < 1) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_patch_rank: np < 1");
  if (np > MAX_PATCHES) return uvc_set_error_msg(UVC_ERR_UNSUPPORTED, "uvc_patch_rank: more than 1024 patches not supported");
  if (offset < 0 || ld <= 0 || (int64_t)offset + np > ld) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_patch_rank: need 0 <= offset and offset + np <= ld");
  const int threads = np >= 256 ? 256 : (np + 63) / 64 * 64;
  k_patch_rank<<<B, threads, 0, (hipStream_t)stream>>>(scores, ld, offset, np, descending != 0, rank);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

extern "C" int uvc_patch_rows_perturb(const void* rows, const int32_t* rank, const int32_t* counts, int32_t nsteps, int32_t B, int32_t np,
                                      int32_t width, int32_t dtype, void* out, void* stream) {
  if (!rows || !rank || !counts || !out) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_patch_rows_perturb: null pointer");
  if (nsteps <= 0 || B <= 0 || width <= 0) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_patch_rows_perturb: nsteps, B and width must be positive");
  if (np < 1) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_patch_rows_perturb: np < 1");
  if (np > MAX_PATCHES) return uvc_set_error_msg(UVC_ERR_UNSUPPORTED, "uvc_patch_rows_perturb: more than 1024 patches not supported");
  if (dtype != UVC_F32 && dtype != UVC_BF16) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_patch_rows_perturb: bad dtype");
  const size_t esz = dtype == UVC_F32 ? 4 : 2;
  const size_t row_bytes = (size_t)width * esz;
  const size_t nrows = (size_t)B * np;
  const bool wide = row_bytes % 16 == 0 && (((uintptr_t)rows | (uintptr_t)out) & 15) == 0;
  const size_t per = wide ? row_bytes / 16 : (size_t)width;
  const size_t total = nrows * per;
  const size_t blocks = (total + 255) / 256;
  const unsigned grid = (unsigned)(blocks < 4096 ? blocks : 4096);          // memory-bound: a capped grid, the rest by stride
  hipStream_t st = (hipStream_t)stream;
  if (wide)
    k_perturb_rows<u32x4><<<grid, 256, 0, st>>>((const u32x4*)rows, rank, counts, nsteps, np, total, (uint32_t)per, (u32x4*)out);
  else if (dtype == UVC_F32)
    k_perturb_rows<uint32_t><<<grid, 256, 0, st>>>((const uint32_t*)rows, rank, counts, nsteps, np, total, (uint32_t)per, (uint32_t*)out);
  else
    k_perturb_rows<uint16_t><<<grid, 256, 0, st>>>((const uint16_t*)rows, rank, counts, nsteps, np, total, (uint32_t)per, (uint16_t*)out);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

extern "C" int uvc_logits_target(const float* logits, int32_t rows, int32_t ld, int32_t n_valid, const int32_t* target, int32_t period,
                                 float* prob, int32_t* hit, void* stream) {
  if (!logits || !target || !prob || !hit) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_logits_target: null pointer");
  if (rows <= 0 || period <= 0) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_logits_target: rows and period must be positive");
  if (rows % period) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_logits_target: rows must be a multiple of period");
  if (n_valid < 1 || n_valid > ld) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_logits_target: need 1 <= n_valid <= ld");
  k_logits_target<<<rows, 256, 0, (hipStream_t)stream>>>(logits, ld, n_valid, target, period, prob, hit);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}
