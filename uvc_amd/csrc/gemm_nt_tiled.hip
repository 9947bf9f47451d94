// NT GEMMs on output tiles without LDS-DMA: the generic kernel and the row-panel kernel for few rows.
//   k_gemm_nt<TA, T, TC, EPI>      128 x 128 tiles, bf16 or float32 compute     UVC_ROUTE_NT
//   k_gemm_nt_rows<TA, TC, EPI>    16 x 64 row panels, M <= 1024, K <= 1024     UVC_ROUTE_NT_ROWS
//
// Tiling (64-wide wavefronts): 256 threads = 4 waves as 2x2; the block tile is staged through
// LDS in 16-byte chunks with register prefetch of the next K tile; rows are padded by 16 B (NT)
// or 32 B (TN) so ds_read_b128 / ds_read_b64_tr_b16 fragment reads are bank-conflict free.
// Operands are swapped in the MFMA (a = B-fragment, b = A-fragment) so every lane ends up with 4
// CONSECUTIVE output columns of one row -> 16-byte (fp32) / 8-byte (bf16) epilogue accesses.
#include "gemm_common.h"

// ================================================================================================
//                                            NT
// ================================================================================================
constexpr int NT_BM = 128, NT_BN = 128;
// LDS row stride in bytes (8 chunks + 32 B pad).  ds_read_b128 is served in the lane groups {0-3,12-15,20-27},
// {4-11,16-19,28-31}, ...: a fragment read (row = lane & 15, chunk = lane >> 4) is conflict-free only when the stride
// in words is 8, 24, 40 or 56 mod 64; the obvious +16 B pad (36 mod 64) costs 2 LDS cycles per group.
constexpr int NT_ROWB = 128 + 32;

template <typename TA, typename T, typename TC, int EPI>
__global__ __launch_bounds__(256, 2) void k_gemm_nt(NtArgs g) {
  typedef Mma<T> MM;
  constexpr int CH = MM::CH;
  constexpr int BK = 8 * CH;                    // elements per K tile (128 B of T per row)
  __shared__ __attribute__((aligned(16))) char smem[(NT_BM + NT_BN) * NT_ROWB];
  char* sA = smem;
  char* sB = smem + NT_BM * NT_ROWB;
  const TA* __restrict__ A = reinterpret_cast<const TA*>(g.A);
  const T* __restrict__ B = reinterpret_cast<const T*>(g.B);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w >> 1, wn = w & 1;
  // XCD-aware tile order.  Workgroups are dispatched round-robin over the 8 XCDs (block b -> XCD b % 8),
  // each with a private L2.  All N tiles of one M tile get block ids that are congruent mod 8 and
  // adjacent in dispatch order, so the A panel is fetched from HBM once and re-read from that XCD's L2.
  const int ntn = (g.N + NT_BN - 1) / NT_BN;
  const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
  const int bn = q % ntn, bm = (q / ntn) * 8 + xcd;
  const int m0 = bm * NT_BM, n0 = bn * NT_BN;
  if (m0 >= g.M) return;
  const int lc = tid & 7, lr = tid >> 3;        // chunk column / first row of this thread's loads

  u32x4 ra[4], rb[4];
  auto gload = [&](int k0) {
    const int kc = k0 + lc * CH;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = lr + 32 * i;
      const int m = m0 + row, n = n0 + row;
      u32x4 z = {0u, 0u, 0u, 0u};
      ra[i] = (m < g.M && kc < g.K) ? ChunkLoad<TA, T>::ld(A + (size_t)m * g.lda + kc) : z;
      rb[i] = (n < g.N && kc < g.K) ? ChunkLoad<T, T>::ld(B + (size_t)n * g.ldb + kc) : z;
    }
  };
  auto lstore = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = lr + 32 * i;
      *reinterpret_cast<u32x4*>(sA + row * NT_ROWB + lc * 16) = ra[i];
      *reinterpret_cast<u32x4*>(sB + row * NT_ROWB + lc * 16) = rb[i];
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (g.K + BK - 1) / BK;
  gload(0);
  lstore();
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) gload((kt + 1) * BK);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      typename MM::Frag fa[4], fb[4];
      const int coff = (ks * 4 + (lane >> 4)) * 16;
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = lds_frag<T>(sA + (wm * 64 + i * 16 + (lane & 15)) * NT_ROWB + coff);
#pragma unroll
      for (int j = 0; j < 4; ++j) fb[j] = lds_frag<T>(sB + (wn * 64 + j * 16 + (lane & 15)) * NT_ROWB + coff);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = MM::mma(fb[j], fa[i], acc[i][j]);
    }
    if (kt + 1 < nk) {
      __syncthreads();
      lstore();
      __syncthreads();
    }
  }

  // ---- epilogue.  The MFMA leaves lane (l) with row m = (l&15), columns (l>>4)*4+{0..3} of each 16x16
  // tile.  Each wave transposes its 64x64 sub-tile through LDS, 32 rows at a time, so that global
  // accesses are whole 128-byte (bf16) / 256-byte (fp32) row segments: 16 bytes per lane.
  float alpha = g.alpha;
  if (g.alpha_ptr) alpha *= *g.alpha_ptr;
  float d0 = 0.f, d1 = 1.f;
  if (EPI == UVC_EPI_BIAS_RESID_GATE) { d0 = g.dptr[0]; d1 = g.dptr[1]; }
  float* stg = reinterpret_cast<float*>(smem) + w * (32 * EP_LD);
  float bias_v[OutVec<TC>::VN];
  nt_load_bias<TC, EPI>(g, lane, n0 + wn * 64, bias_v);
  __syncthreads();
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        *reinterpret_cast<f32x4*>(stg + (ii * 16 + (lane & 15)) * EP_LD + j * 16 + (lane >> 4) * 4) = acc[2 * h + ii][j];
    __syncthreads();
    nt_epilogue_rows<T, TC, EPI>(g, stg, lane, m0 + wm * 64 + h * 32, n0 + wn * 64, alpha, d0, d1, bias_v);
    __syncthreads();
  }
}

// ================================================================================================
//                          NT, row panels (bf16, M <= 1024, K <= 1024)
// ================================================================================================
// The step's turnaround (the last block's class-token rows, the head, their backward) and the teacher's tail are GEMMs on a few hundred rows:
// 128 x 128 tiles put M = 512 on 8 of the 256 CUs, and their k loop is one 64-element tile in flight between two barriers -- 12 to 16 serial
// memory round trips for 0.1 GFLOP.  Here a workgroup owns 16 rows x 64 columns (M = 512, N = 192: 96 workgroups; the head's N = 1000: 512), wave w
// the 16 columns 16w..16w+15, and a wave requests its A and W fragments of 16 k-steps (512 elements of K: 128 VGPRs) before the first MFMA: one
// memory latency per half instead of one per tile.  No LDS in the k loop (the four waves read the same 16 A rows: 24 KB at K = 768, from L2).
// The accumulator is k_gemm_nt's: one k-ordered chain of 2 * ceil(K / 64) MFMA steps, zero-padded past K, leaving through the same staged
// epilogue -- the same bits (tests/test_row_gemm_gpu.py).
constexpr int RP_BM = 16, RP_BN = 64, RP_KS = 16;      // rows, columns of a workgroup; k-steps (of 32) requested at a time
// (RP_MAX_M, RP_MAX_K: gemm_common.h)

// NS k-steps of a wave's chain from step s0: every fragment requested first (straight-line code, no branch: one batch of loads, answered in order),
// then the MFMAs.  A lane whose row is past M / N, or whose chunk is past K, reads a valid address and multiplies zeros.
template <typename TA, int NS>
__device__ __forceinline__ f32x4 rp_steps(const TA* __restrict__ Ap, const bf16_t* __restrict__ Bp, int s0, int K, int gq, bool mv, bool nv, f32x4 acc) {
  typedef Mma<bf16_t> MM;
  u32x4 fa[NS], fb[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int kc = (s0 + s) * 32 + gq * 8, kl = kc < K ? kc : K - 8;
    fa[s] = ChunkLoad<TA, bf16_t>::ld(Ap + kl);
    fb[s] = ChunkLoad<bf16_t, bf16_t>::ld(Bp + kl);
  }
  const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const bool in = (s0 + s) * 32 + gq * 8 < K;
    acc = MM::mma(__builtin_bit_cast(MM::Frag, (nv && in) ? fb[s] : z), __builtin_bit_cast(MM::Frag, (mv && in) ? fa[s] : z), acc);
  }
  return acc;
}

template <typename TA, typename TC, int EPI>
__global__ __launch_bounds__(256) void k_gemm_nt_rows(NtArgs g) {
  typedef bf16_t T;
  typedef Mma<T> MM;
  __shared__ __attribute__((aligned(16))) float stg[RP_BM * EP_LD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, li = lane & 15, gq = lane >> 4;
  const int ntn = (g.N + RP_BN - 1) / RP_BN;
  const int m0 = ((int)blockIdx.x / ntn) * RP_BM, n0 = ((int)blockIdx.x % ntn) * RP_BN;
  const int m = m0 + li, n = n0 + w * 16 + li;
  const bool mv = m < g.M, nv = n < g.N;
  // (rows past M / N: row 0's addresses, the values replaced by zeros -- every load unconditional, so that they leave as one batch)
  const TA* __restrict__ Ap = reinterpret_cast<const TA*>(g.A) + (size_t)(mv ? m : 0) * g.lda;
  const T* __restrict__ Bp = reinterpret_cast<const T*>(g.B) + (size_t)(nv ? n : 0) * g.ldb;
  float alpha = g.alpha;
  if (g.alpha_ptr) alpha *= *g.alpha_ptr;
  float d0 = 0.f, d1 = 1.f;
  if (EPI == UVC_EPI_BIAS_RESID_GATE) { d0 = g.dptr[0]; d1 = g.dptr[1]; }
  float bias_v[OutVec<TC>::VN];
  nt_load_bias<TC, EPI>(g, lane, n0, bias_v);

  // k_gemm_nt's chain is 2 * ceil(K / 64) steps of 32; the steps run here in batches of 16 or 8, and a step past the chain's end multiplies two zero
  // fragments like any step past K: it adds +0 to an accumulator that started at +0 and so is never -0 -- the same bits
  const int nsteps = 2 * ((g.K + 63) / 64);
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  int s0 = 0;
  for (; nsteps - s0 > RP_KS / 2; s0 += RP_KS) acc = rp_steps<TA, RP_KS>(Ap, Bp, s0, g.K, gq, mv, nv, acc);
  if (s0 < nsteps) acc = rp_steps<TA, RP_KS / 2>(Ap, Bp, s0, g.K, gq, mv, nv, acc);
  // lane (li, gq) holds row li, columns 4 gq .. 4 gq + 3 of the wave's 16: the 16 x 64 tile is staged once and leaves as whole row segments,
  // eight rows per wave (waves 0 and 1)
  *reinterpret_cast<f32x4*>(stg + li * EP_LD + w * 16 + gq * 4) = acc;
  __syncthreads();
  if (w < 2) nt_epilogue_rows<T, TC, EPI, 8>(g, stg + w * 8 * EP_LD, lane, m0 + w * 8, n0, alpha, d0, d1, bias_v);
}

// ---- host code: the launchers (grid, LDS bytes, launch; they decide nothing) and what gemm.hip calls
namespace {

template <typename TA, typename T, typename TC>
int launch_nt_epi(const NtArgs& a, int epi, hipStream_t st) {
  const int grid = ceil_div(ceil_div(a.M, NT_BM), 8) * 8 * ceil_div(a.N, NT_BN);   // M tiles padded to the 8 XCDs
#define NT_CASE(E) case E: k_gemm_nt<TA, T, TC, E><<<grid, 256, 0, st>>>(a); break;
  NT_LAUNCH(epi, NT_EPI9(NT_CASE))
#undef NT_CASE
}

template <typename TA, typename TC>
int launch_nt_rows_t(const NtArgs& a, int epi, hipStream_t st) {
  const int grid = ceil_div(a.M, RP_BM) * ceil_div(a.N, RP_BN);
#define RP_CASE(E) case E: k_gemm_nt_rows<TA, TC, E><<<grid, 256, 0, st>>>(a); break;
  NT_LAUNCH(epi, RP_CASE(UVC_EPI_NONE) RP_CASE(UVC_EPI_BIAS) RP_CASE(UVC_EPI_BIAS_RESID) RP_CASE(UVC_EPI_BIAS_RESID_GATE) RP_CASE(UVC_EPI_BIAS_GELU_GRAD) RP_CASE(UVC_EPI_MUL_AUX))
#undef RP_CASE
}

}  // namespace

namespace uvc_gemm {
int launch_nt(const uvc_gemm_route& r, const NtArgs& a, hipStream_t st) {
  const int e = r.epilogue;
  if (r.t_f32) return launch_nt_epi<float, float, float>(a, e, st);
  if (r.a_f32) return r.c_f32 ? launch_nt_epi<float, bf16_t, float>(a, e, st) : launch_nt_epi<float, bf16_t, bf16_t>(a, e, st);
  return r.c_f32 ? launch_nt_epi<bf16_t, bf16_t, float>(a, e, st) : launch_nt_epi<bf16_t, bf16_t, bf16_t>(a, e, st);
}
int launch_nt_rows(const uvc_gemm_route& r, const NtArgs& a, hipStream_t st) { return NT_BY_TA_TC(launch_nt_rows_t, a, r.epilogue, st); }
}  // namespace uvc_gemm
