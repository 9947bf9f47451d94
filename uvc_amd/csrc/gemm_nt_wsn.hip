// NT GEMMs at N = 192 that give every wave a 16-column slice of the whole reduction (bf16): fc2, attn.proj and the dgrads of the narrow models.
//   k_gemm_wsn<TC, EPI, KT>                        32-row tiles, plain and bias epilogues       UVC_ROUTE_WSN
//   k_gemm_wsn16<TC, EPI, KT>                      16-row tiles, float32 C / residual epilogues UVC_ROUTE_WSN16
//   k_gemm_wsn16_dma<EPI, KT, LN, NST, RLOW>       the residual epilogues on an LDS-DMA ring    UVC_ROUTE_WSN16_DMA
// The dgrad kernels of the same geometry that end in the LayerNorm backward are in gemm_nt_lnbwd.hip.
#include "gemm_common.h"

// ================================================================================================
//        NT, weights-stationary, one 16-column slice of the FULL reduction per wave (bf16, N == 192)
// ================================================================================================
// fc2 (+ residual + gate mix), dgrad of fc1, dgrad of qkv: K = 768 / 576 against N = 192.  W [192, K] does not fit one
// wave's registers as a 64-column slice, and splitting K over waves needs a cross-wave reduction with two barriers per
// sub-tile (tried: 141 us for fc2, 60 us for dgrad fc1; this kernel 136 / 45).  Here the workgroup is 12 waves, wave w owns output columns 16w..16w+15 and keeps that slice of W for the whole K in registers
// (KT fragments = 96 VGPRs at K = 768).  With W as the MFMA A operand the accumulator of lane (row, g) is four
// CONSECUTIVE output columns of one row, so the epilogue needs no LDS transpose and no barrier: residual rows are
// read and results written as 16-byte vectors (64 contiguous bytes per row per wave, the neighbouring waves fill the
// rest of the line).  A streams through a double-buffered 32-row LDS image (one barrier per tile); the two 16-row
// sub-tiles are two independent MFMA chains; next tile's residual operands are prefetched under this tile's math.
constexpr int WN_BM = 32;

template <typename TC, int EPI, int KT>
__global__ __launch_bounds__(768) void k_gemm_wsn(NtArgs g) {
  typedef bf16_t T;
  typedef Mma<T> MM;
  constexpr int K = KT * 32, NTH = 768;
  constexpr int ROWB = K * 2 + 32, CPR = K / 8;
  constexpr int NLD = (WN_BM * CPR + NTH - 1) / NTH;
  constexpr bool RES = EPI == UVC_EPI_BIAS_RESID || EPI == UVC_EPI_BIAS_RESID_GATE;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sA0 = smem;
  char* sA1 = smem + WN_BM * ROWB;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, gq = lane >> 4, li = lane & 15;
  const T* __restrict__ A = reinterpret_cast<const T*>(g.A);
  const T* __restrict__ W = reinterpret_cast<const T*>(g.B);
  TC* __restrict__ C = reinterpret_cast<TC*>(g.C);
  const int ntiles = (g.M + WN_BM - 1) / WN_BM;
  const int n = w * 16 + gq * 4;                       // this lane's four output columns

  typename MM::Frag bf[KT];
#pragma unroll
  for (int ks = 0; ks < KT; ++ks)
    bf[ks] = __builtin_bit_cast(typename MM::Frag, *reinterpret_cast<const u32x4*>(W + (size_t)(w * 16 + li) * g.ldb + (ks * 4 + gq) * 8));
  float alpha = g.alpha;
  if (g.alpha_ptr) alpha *= *g.alpha_ptr;
  float d0 = 0.f, d1 = 1.f;
  if (EPI == UVC_EPI_BIAS_RESID_GATE) { d0 = g.dptr[0]; d1 = g.dptr[1]; }
  f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
  if (EPI == UVC_EPI_BIAS || RES) bias4 = *reinterpret_cast<const f32x4*>(g.bias + n);

  u32x4 ra[NLD];
  auto gload = [&](int tile) {
    const int m0 = tile * WN_BM;
    const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int id = tid + NTH * i, row = id / CPR, c = id % CPR;
      const int m = m0 + row;
      ra[i] = (row < WN_BM && m < g.M) ? *reinterpret_cast<const u32x4*>(A + (size_t)m * g.lda + c * 8) : z;
    }
  };
  auto lstore = [&](char* buf) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int id = tid + NTH * i, row = id / CPR, c = id % CPR;
      if (row < WN_BM) *reinterpret_cast<u32x4*>(buf + row * ROWB + c * 16) = ra[i];
    }
  };
  struct Epi { f32x4 r[2]; f32x4 r2[2]; };
  auto eload = [&](Epi& E, int tile_) {
    if (!RES) return;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const int m = tile_ * WN_BM + s2 * 16 + li;
      const size_t off = (m < g.M && tile_ < ntiles) ? (size_t)m * g.ldr + n : 0;
      E.r[s2] = Resid<TC>::f4(Resid<TC>::ld4(g.R, off));
      if (EPI == UVC_EPI_BIAS_RESID_GATE) E.r2[s2] = Resid<TC>::f4(Resid<TC>::ld4(g.R2, off));
    }
  };

  int tile = blockIdx.x;
  if (tile >= ntiles) return;
  Epi E, En;
  gload(tile);
  eload(E, tile);
  lstore(sA0);
  __syncthreads();
  int par = 0;
  for (; tile < ntiles; tile += gridDim.x) {
    const int next = tile + gridDim.x;
    if (next < ntiles) gload(next);
    const char* buf = par ? sA1 : sA0;
    f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KT; ++ks) {
      const typename MM::Frag f0 = lds_frag<T>(buf + li * ROWB + (ks * 4 + gq) * 16);
      const typename MM::Frag f1 = lds_frag<T>(buf + (16 + li) * ROWB + (ks * 4 + gq) * 16);
      c0 = MM::mma(bf[ks], f0, c0);
      c1 = MM::mma(bf[ks], f1, c1);
    }
    eload(En, next);
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const int m = tile * WN_BM + s2 * 16 + li;
      f32x4 v = s2 ? c1 : c0;
      if (m < g.M) {
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = epi_scale_bias(v[e], alpha, bias4[e]);
        if (RES) {
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] += E.r[s2][e];
        }
        if (EPI == UVC_EPI_BIAS_RESID_GATE) {
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = epi_gate_mix(o[e], E.r2[s2][e], d0, d1);
        }
        if (sizeof(TC) == 4) *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(C) + (size_t)m * g.ldc + n) = f32x4{o[0], o[1], o[2], o[3]};
        else { u32x2 q; q[0] = pack_bf16x2(o[0], o[1]); q[1] = pack_bf16x2(o[2], o[3]); *reinterpret_cast<u32x2*>(reinterpret_cast<bf16_t*>(C) + (size_t)m * g.ldc + n) = q; }
      }
    }
    E = En;
    if (next < ntiles) lstore(par ? sA0 : sA1);
    __syncthreads();
    par ^= 1;
  }
}

template <typename TC, int EPI, int KT>
__global__ __launch_bounds__(768) void k_gemm_wsn16(NtArgs g) {
  typedef bf16_t T;
  typedef Mma<T> MM;
  constexpr int K = KT * 32, NTH = 768;
  constexpr int ROWB = K * 2 + 32, CPR = K / 8;
  constexpr int NLD = (16 * CPR + NTH - 1) / NTH;
  constexpr bool RES = EPI == UVC_EPI_BIAS_RESID || EPI == UVC_EPI_BIAS_RESID_GATE;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sA0 = smem;
  char* sA1 = smem + 16 * ROWB;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, gq = lane >> 4, li = lane & 15;
  const T* __restrict__ A = reinterpret_cast<const T*>(g.A);
  const T* __restrict__ W = reinterpret_cast<const T*>(g.B);
  TC* __restrict__ C = reinterpret_cast<TC*>(g.C);
  const int ntiles = (g.M + 16 - 1) / 16;
  const int n = w * 16 + gq * 4;                       // this lane's four output columns

  typename MM::Frag bf[KT];
#pragma unroll
  for (int ks = 0; ks < KT; ++ks)
    bf[ks] = __builtin_bit_cast(typename MM::Frag, *reinterpret_cast<const u32x4*>(W + (size_t)(w * 16 + li) * g.ldb + (ks * 4 + gq) * 8));
  float alpha = g.alpha;
  if (g.alpha_ptr) alpha *= *g.alpha_ptr;
  float d0 = 0.f, d1 = 1.f;
  if (EPI == UVC_EPI_BIAS_RESID_GATE) { d0 = g.dptr[0]; d1 = g.dptr[1]; }
  f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
  if (EPI == UVC_EPI_BIAS || RES) bias4 = *reinterpret_cast<const f32x4*>(g.bias + n);

  u32x4 ra[NLD];
  auto gload = [&](int tile) {
    const int m0 = tile * 16;
    const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int id = tid + NTH * i, row = id / CPR, c = id % CPR;
      const int m = m0 + row;
      ra[i] = (row < 16 && m < g.M) ? *reinterpret_cast<const u32x4*>(A + (size_t)m * g.lda + c * 8) : z;
    }
  };
  auto lstore = [&](char* buf) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int id = tid + NTH * i, row = id / CPR, c = id % CPR;
      if (row < 16) *reinterpret_cast<u32x4*>(buf + row * ROWB + c * 16) = ra[i];
    }
  };
  struct Epi { typename Resid<TC>::Raw4 r[1]; typename Resid<TC>::Raw4 r2[1]; };      // raw: the bf16 stream keeps 2 instead of 4 registers per operand in flight
  auto eload = [&](Epi& E, int tile_) {
    if (!RES) return;
#pragma unroll
    for (int s2 = 0; s2 < 1; ++s2) {
      const int m = tile_ * 16 + s2 * 16 + li;
      const size_t off = (m < g.M && tile_ < ntiles) ? (size_t)m * g.ldr + n : 0;
      E.r[s2] = Resid<TC>::ld4(g.R, off);
      if (EPI == UVC_EPI_BIAS_RESID_GATE) E.r2[s2] = Resid<TC>::ld4(g.R2, off);
    }
  };

  int tile = blockIdx.x;
  if (tile >= ntiles) return;
  Epi E, En;
  gload(tile);
  eload(E, tile);
  lstore(sA0);
  __syncthreads();
  int par = 0;
  for (; tile < ntiles; tile += gridDim.x) {
    const int next = tile + gridDim.x;
    if (next < ntiles) gload(next);
    const char* buf = par ? sA1 : sA0;
    // one accumulation chain in k order: the same summation order as every other NT kernel of the library, so a row's result
    // does not depend on which kernel the batch size selects (tests/test_fullsize_gpu.py); the 12 waves hide the chain latency
    f32x4 c0 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KT; ++ks) c0 = MM::mma(bf[ks], lds_frag<T>(buf + li * ROWB + (ks * 4 + gq) * 16), c0);
    eload(En, next);
#pragma unroll
    for (int s2 = 0; s2 < 1; ++s2) {
      const int m = tile * 16 + s2 * 16 + li;
      f32x4 v = c0;
      if (m < g.M) {
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = epi_scale_bias(v[e], alpha, bias4[e]);
        if (RES) {
          const f32x4 rv = Resid<TC>::f4(E.r[s2]);
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] += rv[e];
        }
        if (EPI == UVC_EPI_BIAS_RESID_GATE) {
          const f32x4 rv = Resid<TC>::f4(E.r2[s2]);
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = epi_gate_mix(o[e], rv[e], d0, d1);
        }
        if (sizeof(TC) == 4) *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(C) + (size_t)m * g.ldc + n) = f32x4{o[0], o[1], o[2], o[3]};
        else { u32x2 q; q[0] = pack_bf16x2(o[0], o[1]); q[1] = pack_bf16x2(o[2], o[3]); *reinterpret_cast<u32x2*>(reinterpret_cast<bf16_t*>(C) + (size_t)m * g.ldc + n) = q; }
      }
    }
    E = En;
    if (next < ntiles) lstore(par ? sA0 : sA1);
    __syncthreads();
    par ^= 1;
  }
}


// ---- fc2 (+ bias + residual [+ gate mix]) on the same LDS-DMA ring ------------------------------------------------------------
// k_gemm_wsn16<float, RESID / RESID_GATE> keeps one 16-row tile of A and of the residual rows in flight per CU (register-staged, one
// tile ahead): 87-89 us for 387 MB = 4.4 TB/s.  Same ring as k_gemm_wsn_lnbwd_dma: A [16, K] bf16 and the float32 residual rows
// (R = x1, R2 = x_l) go HBM -> LDS by global_load_lds_dwordx4 into three stages, two in flight; one barrier per tile; the epilogue
// runs from registers after it.  The accumulation is the single k-ordered chain and the epilogue the same fmaf sequence as every other
// NT kernel, so the output bits do not depend on which kernel a problem size selects (tests/test_fullsize_gpu.py).  M % 16 == 0.
// RLOW: the residual stream is bf16 -- R, R2 and C are bf16 rows (24 + 2 slots of 16 bytes in a stage instead of 48 + 2; the result is
// rounded once, at the store, and the LayerNorm that follows is taken of the ROUNDED row: what the consumers of C will read).
template <int EPI, int KT, bool LN, int NST, bool RLOW>
__global__ __launch_bounds__(768) void k_gemm_wsn16_dma(NtArgs g) {
  typedef bf16_t T;
  typedef Mma<T> MM;
  constexpr int K = KT * 32, D = 192, NWV = 12;
  constexpr int ROWB = K * 2 + 32, SA = ROWB / 16;
  constexpr int NA = (16 * SA + 63) / 64;
  constexpr int RSZ = RLOW ? 2 : 4, RSL = D * RSZ / 16;         // bytes per residual element; data slots per residual row
  constexpr int XS = RSL + 2, XB = XS * 16, NX = (16 * XS + 63) / 64;
  constexpr bool GATE = EPI == UVC_EPI_BIAS_RESID_GATE;
  constexpr int I_R = NA, I_R2 = I_R + NX, NI = I_R2 + (GATE ? NX : 0);
  constexpr int STAGE = NI * 1024;
  constexpr int NPW = (NI + NWV - 1) / NWV;                   // DMA instructions per wave and stage (surplus ones repeat the wave's first)
  // LN: behind the ring, the row-statistics table [2][16 rows][12 waves][2] and gamma / beta of the LayerNorm that follows
  constexpr int LN_BYTES = LN ? 2 * 16 * NWV * 8 + 3 * D * 4 : 0;      // + gamma, beta, bias
  static_assert(NST >= 3 && NPW <= 5 && NST * STAGE + LN_BYTES <= 160 * 1024, "ring does not fit");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, gq = lane >> 4, li = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const T* __restrict__ W = reinterpret_cast<const T*>(g.B);
  char* __restrict__ C = reinterpret_cast<char*>(g.C);
  const int ntiles = (g.M + 15) / 16;                         // M >= 16; a ragged last tile is the LAST 16 rows (it overlaps its neighbour:
                                                              // those rows are computed twice from the same operands, same bits, same stores)
  const int n = w * 16 + gq * 4;
  float* const sRed = reinterpret_cast<float*>(smem + NST * STAGE);
  float* const sGB = sRed + 2 * 16 * NWV * 2;
  if (LN) {
    if (tid < D) { sGB[tid] = g.ln_gamma[tid]; sGB[D + tid] = g.ln_beta[tid]; sGB[2 * D + tid] = g.bias[tid]; }      // before the first DMA is issued (see k_gemm_wsn_lnbwd_dma)
  }
  const unsigned gaddr = lds_addr(sGB) + (unsigned)n * 4u;
  const unsigned redr = lds_addr(sRed) + (unsigned)(li * NWV * 8);
  typename MM::Frag bf[KT];
#pragma unroll
  for (int ks = 0; ks < KT; ++ks)
    bf[ks] = __builtin_bit_cast(typename MM::Frag, *reinterpret_cast<const u32x4*>(W + (size_t)(w * 16 + li) * K + (ks * 4 + gq) * 8));
  float alpha = g.alpha;
  if (g.alpha_ptr) alpha *= *g.alpha_ptr;
  float d0 = 0.f, d1 = 1.f;
  if (GATE) { d0 = g.dptr[0]; d1 = g.dptr[1]; }
  f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
  if (!LN) bias4 = *reinterpret_cast<const f32x4*>(g.bias + n);      // LN: re-read from LDS per tile (four VGPRs less across the MFMA chain)

  const char* rb[NPW]; unsigned rstride[NPW], rdst[NPW], loff[NPW];
#pragma unroll
  for (int q = 0; q < NPW; ++q) {
    int I = q * NWV + w;
    if (I >= NI) I = w;                               // duplicate of this wave's first A instruction: uniform count per wave
    const int sl = (I - (I < I_R ? 0 : I < I_R2 ? I_R : I_R2)) * 64 + lane;
    rdst[q] = (unsigned)I * 1024u;
    if (I < I_R) {
      const int row = sl / SA, c = sl % SA;
      rb[q] = reinterpret_cast<const char*>(g.A); rstride[q] = K * 2u;
      loff[q] = row < 16 ? (unsigned)(row * K * 2 + (c < K / 8 ? c : 0) * 16) : 0u;
    } else {
      const int row = sl / XS, c = sl % XS;
      rb[q] = reinterpret_cast<const char*>(I < I_R2 ? g.R : g.R2); rstride[q] = (unsigned)(D * RSZ);
      loff[q] = row < 16 ? (unsigned)(row * D * RSZ + (c < RSL ? c : 0) * 16) : 0u;
    }
  }
  auto issue = [&](int tile, int st) {
    const int t = tile < ntiles ? tile : ntiles - 1;
    const unsigned r0 = (unsigned)min(t * 16, g.M - 16);          // first row of the tile
#pragma unroll
    for (int q = 0; q < NPW; ++q) {
      const char* src = rb[q] + ((unsigned long long)r0 * (unsigned long long)rstride[q] + (unsigned long long)loff[q]);
      char* dst = smem + st * STAGE + rdst[q];
      // (nt on these loads -- fc2's GELU(a) operand only, or every operand of the kernel: 0.3-0.6 % slower in the step, profiles/r5zz_ab_nt_wsn.txt)
      __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)src, (void __attribute__((address_space(3)))*)dst, 16, 0, 0);
    }
  };
  const unsigned s0 = lds_addr(smem);
  const unsigned fragoff = (unsigned)(li * ROWB + gq * 16), roff = (unsigned)(I_R * 1024 + li * XB + n * RSZ);

  // NST stages, NST - 1 in flight: stage t + NST - 1 is requested at the top of iteration t into the image iteration t - 1 read
  int tile = blockIdx.x;
#pragma unroll
  for (int q = 0; q < NST - 1; ++q) issue(tile + q * gridDim.x, q);
  wait_vm<(NST - 2) * NPW>();
  __builtin_amdgcn_s_barrier();
  int st = 0, par = 0;
  // LN: the normalisation of tile t is DEFERRED into iteration t + 1.  Its operands (the 12 pairs of the statistics table, gamma, beta)
  // are requested in three small batches between the first k-step groups of tile t + 1 and consumed under its MFMAs (inside one wave the
  // VALU work fills the matrix pipe's issue gaps); as a chain of LDS round trips behind the barrier it cost 20 us of 100.
  bool have_prev = false;
  float po[4] = {0.f, 0.f, 0.f, 0.f};
  int prow0 = 0;
  float lm2 = 0.f, ls1 = 0.f, ls2 = 0.f, lpv = 0.f;
  u32x4 tq0, tq1, lgr, lbr;
  auto ln_issue = [&](auto offv) {
    constexpr int OFF = decltype(offv)::value;
    const unsigned ra = redr + (unsigned)((par ^ 1) * 16 * NWV * 8);
    tq0 = ds_read128<OFF>(ra); tq1 = ds_read128<OFF + 16>(ra);
  };
  auto ln_first = [&]() {
    asm volatile("" : "+v"(tq0), "+v"(tq1));
    const f32x4 a0 = __builtin_bit_cast(f32x4, tq0), a1 = __builtin_bit_cast(f32x4, tq1);
    lpv = a0[0];
    float dd;
    lm2 = a0[1]; dd = a0[2] - lpv; ls1 = dd; ls2 = dd * dd; lm2 += a0[3];
    dd = a1[0] - lpv; ls1 += dd; ls2 += dd * dd; lm2 += a1[1]; dd = a1[2] - lpv; ls1 += dd; ls2 += dd * dd; lm2 += a1[3];
    asm volatile("" : "+v"(lm2), "+v"(ls1), "+v"(ls2), "+v"(lpv));
  };
  auto ln_acc = [&]() {
    asm volatile("" : "+v"(tq0), "+v"(tq1));
    const f32x4 a0 = __builtin_bit_cast(f32x4, tq0), a1 = __builtin_bit_cast(f32x4, tq1);
    float dd;
    dd = a0[0] - lpv; ls1 += dd; ls2 += dd * dd; lm2 += a0[1]; dd = a0[2] - lpv; ls1 += dd; ls2 += dd * dd; lm2 += a0[3];
    dd = a1[0] - lpv; ls1 += dd; ls2 += dd * dd; lm2 += a1[1]; dd = a1[2] - lpv; ls1 += dd; ls2 += dd * dd; lm2 += a1[3];
    asm volatile("" : "+v"(lm2), "+v"(ls1), "+v"(ls2));
  };
  // mean = pivot + s1/12;  sum (m_w - mean)^2 = s2 - 12 (s1/12)^2;  var = (sum M2_w + 16 * that) / D  (Chan et al.; see the epilogue)
  auto ln_finish = [&]() {
    asm volatile("" : "+v"(lgr), "+v"(lbr));
    const float dm = ls1 * (1.0f / 12.0f);
    const float mean = lpv + dm;
    const float dv = ls2 - 12.0f * dm * dm;
    const float rstd = rsqrtf((lm2 + 16.0f * dv) * (1.0f / (float)D) + g.ln_eps);
    const f32x4 gam = __builtin_bit_cast(f32x4, lgr), bet = __builtin_bit_cast(f32x4, lbr);
    float y[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = (po[e] - mean) * rstd * gam[e] + bet[e];
    u32x2 q; q[0] = pack_bf16x2(y[0], y[1]); q[1] = pack_bf16x2(y[2], y[3]);
    const size_t trow = (size_t)prow0;
    *reinterpret_cast<u32x2*>(reinterpret_cast<char*>(reinterpret_cast<T*>(g.ln_out) + trow * D) + (unsigned)((li * D + n) * 2)) = q;
    if (g.ln_mean && w == 0 && gq == 0) {
      *reinterpret_cast<float*>(reinterpret_cast<char*>(g.ln_mean + trow) + (unsigned)(li * 4)) = mean;
      *reinterpret_cast<float*>(reinterpret_cast<char*>(g.ln_rstd + trow) + (unsigned)(li * 4)) = rstd;
    }
  };
  for (; tile < ntiles; tile += gridDim.x) {
    issue(tile + (NST - 1) * gridDim.x, st == 0 ? NST - 1 : st - 1);
    const unsigned sb = s0 + (unsigned)(st * STAGE);
    f32x4 c0 = {0.f, 0.f, 0.f, 0.f};
    u32x4 fa[2], fb[2];
    const unsigned fr = sb + fragoff;
    if (LN && have_prev) ln_issue(std::integral_constant<int, 0>{});
#define RD2(dst, ks0) dst[0] = ds_read128<(ks0) * 64>(fr); dst[1] = ds_read128<(ks0) * 64 + 64>(fr);
#define GROUP(gk, cur, nxt) if ((gk) < KT / 2) { \
      if ((gk) + 1 < KT / 2) { RD2(nxt, ((gk) + 1) * 2) wait_lgkm<2>(); } else wait_lgkm<0>(); \
      asm volatile("" : "+v"(cur[0]), "+v"(cur[1])); \
      c0 = MM::mma(bf[(gk) * 2], __builtin_bit_cast(typename MM::Frag, cur[0]), c0); \
      c0 = MM::mma(bf[(gk) * 2 + 1], __builtin_bit_cast(typename MM::Frag, cur[1]), c0); }
    static_assert(KT % 2 == 0 && KT <= 24, "pairs of k-steps");
    RD2(fa, 0)
    GROUP(0, fa, fb)                       // its wait (two youngest reads may be out) covers the older table reads
    if (LN && have_prev) { ln_first(); ln_issue(std::integral_constant<int, 32>{}); }
    GROUP(1, fb, fa)
    if (LN && have_prev) { ln_acc(); ln_issue(std::integral_constant<int, 64>{}); }
    GROUP(2, fa, fb)
    if (LN && have_prev) {
      ln_acc();
      if constexpr (KT / 2 > 3) { lgr = ds_read128<0>(gaddr); lbr = ds_read128<D * 4>(gaddr); }      // gamma, beta: consumed one group on (registers)
      else { lgr = ds_read128<0>(gaddr); lbr = ds_read128<D * 4>(gaddr); wait_lgkm<0>(); ln_finish(); }
    }
    GROUP(3, fb, fa)
    if (LN && have_prev && KT / 2 > 3) ln_finish();
    GROUP(4, fa, fb) GROUP(5, fb, fa)
    GROUP(6, fa, fb) GROUP(7, fb, fa) GROUP(8, fa, fb) GROUP(9, fb, fa) GROUP(10, fa, fb) GROUP(11, fb, fa)
#undef GROUP
#undef RD2
    // the row's residual operands: four consecutive columns = 16 bytes (float32 stream) or 8 bytes (bf16 stream)
    typename Resid<typename std::conditional<RLOW, bf16_t, float>::type>::Raw4 rr, rr2;
    if constexpr (RLOW) {
      asm volatile("ds_read_b64 %0, %1" : "=v"(rr) : "v"(sb + roff));
      rr2 = rr;
      if (GATE) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(rr2) : "v"(sb + roff), "n"(NX * 1024));
    } else {
      rr = ds_read128<0>(sb + roff); rr2 = rr;
      if (GATE) rr2 = ds_read128<NX * 1024>(sb + roff);
    }
    typedef Resid<typename std::conditional<RLOW, bf16_t, float>::type> RS;
    if constexpr (!LN) {
      wait_vm<(NST - 2) * NPW>();                                 // own part of the next stage has landed
      wait_lgkm<0>();
      asm volatile("" : "+v"(rr), "+v"(rr2));
      __builtin_amdgcn_s_barrier();
      const f32x4 r = RS::f4(rr), r2 = RS::f4(rr2);
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = epi_scale_bias(c0[e], alpha, bias4[e]);
        o[e] += r[e];
        if (GATE) o[e] = epi_gate_mix(o[e], r2[e], d0, d1);
      }
      char* cp = C + ((size_t)(min(tile * 16, g.M - 16) + li) * g.ldc + n) * RSZ;
      if constexpr (RLOW) { u32x2 q; q[0] = pack_bf16x2(o[0], o[1]); q[1] = pack_bf16x2(o[2], o[3]); *reinterpret_cast<u32x2*>(cp) = q; }
      else *reinterpret_cast<f32x4*>(cp) = f32x4{o[0], o[1], o[2], o[3]};
    } else {
      // The output row is spread over the 12 waves (16 columns each).  Every wave leaves (mean, centred sum of squares) of its 16
      // columns in the table BEFORE the tile's one barrier and picks up the 12 pairs after it; they combine exactly (Chan et al.):
      // mean = sum m_w / 12, M2 = sum M2_w + 16 sum (m_w - mean)^2 -- the two-pass variance of k_ln_fwd_v without a second exchange.
      u32x4 bq = ds_read128<2 * D * 4>(gaddr);
      wait_lgkm<0>();
      asm volatile("" : "+v"(rr), "+v"(rr2), "+v"(bq));
      const f32x4 r = RS::f4(rr), r2 = RS::f4(rr2), bv = __builtin_bit_cast(f32x4, bq);
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = epi_scale_bias(c0[e], alpha, bv[e]);
        o[e] += r[e];
        if (GATE) o[e] = epi_gate_mix(o[e], r2[e], d0, d1);
      }
      u32x2 oq = {0u, 0u};
      if constexpr (RLOW) {                       // the stored (rounded) row is what the LayerNorm and every later consumer see
        oq[0] = pack_bf16x2(o[0], o[1]); oq[1] = pack_bf16x2(o[2], o[3]);
        const f32x4 t = Resid<bf16_t>::f4(oq);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = t[e];
      }
      {
        const float sm = sum_rows4((o[0] + o[1]) + (o[2] + o[3]));
        const float mw = sm * (1.0f / 16.0f);
        float qw = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float dd = o[e] - mw; qw += dd * dd; }
        qw = sum_rows4(qw);
        if (gq == 0) ds_write64_a(redr + (unsigned)(par * 16 * NWV * 8 + w * 8), f32x2{mw, qw});
      }
      // the output rows leave now; their normalisation follows inside the next iteration (or behind the loop)
      prow0 = min(tile * 16, g.M - 16);
      if constexpr (RLOW) *reinterpret_cast<u32x2*>(C + (size_t)prow0 * g.ldc * RSZ + (unsigned)((li * g.ldc + n) * RSZ)) = oq;
      else *reinterpret_cast<f32x4*>(C + (size_t)prow0 * g.ldc * RSZ + (unsigned)((li * g.ldc + n) * RSZ)) = f32x4{o[0], o[1], o[2], o[3]};
#pragma unroll
      for (int e = 0; e < 4; ++e) po[e] = o[e];
      have_prev = true;
      wait_vm<(NST - 2) * NPW>();                                 // own part of the next stage has landed
      wait_lgkm<0>();
      __builtin_amdgcn_s_barrier();
      par ^= 1;
    }
    st = st == NST - 1 ? 0 : st + 1;
  }
  if (LN && have_prev) {                                         // the last tile of this workgroup
    ln_issue(std::integral_constant<int, 0>{});
    wait_lgkm<0>(); ln_first();
    ln_issue(std::integral_constant<int, 32>{});
    wait_lgkm<0>(); ln_acc();
    ln_issue(std::integral_constant<int, 64>{}); lgr = ds_read128<0>(gaddr); lbr = ds_read128<D * 4>(gaddr);
    wait_lgkm<0>(); ln_acc(); ln_finish();
  }
  wait_vm<0>();
}

// ---- launchers
namespace {

// k_gemm_wsn (ROWS = 32: plain and bias epilogues) and k_gemm_wsn16 (ROWS = 16): one persistent workgroup per CU
template <typename TC, int KT, int ROWS>
int launch_wsn_rows(const NtArgs& a, int epi, hipStream_t st) {
  const int ntiles = ceil_div(a.M, ROWS);
  const int grid = ntiles < 256 ? ntiles : 256;
  const size_t sh = (size_t)2 * ROWS * (KT * 64 + 32);
#define WN_CASE(KERNEL, E) case E: { \
    UVC_MAX_LDS(sh, KERNEL<TC, E, KT>); \
    KERNEL<TC, E, KT><<<grid, 768, sh, st>>>(a); } break;
  if constexpr (ROWS == 16) {
    NT_LAUNCH(epi, WN_CASE(k_gemm_wsn16, UVC_EPI_NONE) WN_CASE(k_gemm_wsn16, UVC_EPI_BIAS) WN_CASE(k_gemm_wsn16, UVC_EPI_BIAS_RESID) WN_CASE(k_gemm_wsn16, UVC_EPI_BIAS_RESID_GATE))
  } else {
    static_assert(ROWS == WN_BM, "k_gemm_wsn's tile height");
    NT_LAUNCH(epi, WN_CASE(k_gemm_wsn, UVC_EPI_NONE) WN_CASE(k_gemm_wsn, UVC_EPI_BIAS))
  }
#undef WN_CASE
}
template <typename TC>
int launch_wsn_t(const uvc_gemm_route& r, const NtArgs& a, hipStream_t st) {
#define WN_KT(KT) case KT: return r.family == UVC_ROUTE_WSN16 ? launch_wsn_rows<TC, KT, 16>(a, r.epilogue, st) : launch_wsn_rows<TC, KT, WN_BM>(a, r.epilogue, st);
  switch (r.kt) {
    WN_KT(24) WN_KT(18) WN_KT(16) WN_KT(8)
    default: return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_nt: K not built for the column-sliced kernel");
  }
#undef WN_KT
}

template <int EPI, int KT, bool LN, int NST, bool RLOW>
int launch_wsn16_dma(const NtArgs& a, hipStream_t st) {
  constexpr int NX_ = RLOW ? 7 : 13;                              // KB of a stage per residual operand (16 rows x (24 | 48) + 2 slots)
  constexpr int NA_ = (16 * (KT * 4 + 2) + 63) / 64, NI_ = NA_ + NX_ + (EPI == UVC_EPI_BIAS_RESID_GATE ? NX_ : 0);
  const int sh = NST * NI_ * 1024 + (LN ? 2 * 16 * 12 * 8 + 3 * 192 * 4 : 0);
  UVC_MAX_LDS(sh, k_gemm_wsn16_dma<EPI, KT, LN, NST, RLOW>);
  const int ntiles = ceil_div(a.M, 16);
  k_gemm_wsn16_dma<EPI, KT, LN, NST, RLOW><<<ntiles < 256 ? ntiles : 256, 768, sh, st>>>(a);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}
// the instances built: K = 192 (RESID, seven stages, with and without LayerNorm), K = 768 (three stages, both), K = 512 / 256 (with LayerNorm only)
template <bool RLOW>
int launch_ring_t(const uvc_gemm_route& r, const NtArgs& a, hipStream_t st) {
  const bool gate = r.epilogue == UVC_EPI_BIAS_RESID_GATE;
#define RING(KT, LN, NST) \
  if (r.kt == KT && r.ln == LN && r.nst == NST) \
    return gate ? launch_wsn16_dma<UVC_EPI_BIAS_RESID_GATE, KT, LN, NST, RLOW>(a, st) : launch_wsn16_dma<UVC_EPI_BIAS_RESID, KT, LN, NST, RLOW>(a, st);
  if (r.kt == 6 && r.nst == 7 && !gate)
    return r.ln ? launch_wsn16_dma<UVC_EPI_BIAS_RESID, 6, true, 7, RLOW>(a, st) : launch_wsn16_dma<UVC_EPI_BIAS_RESID, 6, false, 7, RLOW>(a, st);
  RING(24, true, 3) RING(24, false, 3) RING(16, true, 3) RING(8, true, 4)
#undef RING
  return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_nt: ring kernel not built for this route");
}

}  // namespace

namespace uvc_gemm {
int launch_wsn(const uvc_gemm_route& r, const NtArgs& a, hipStream_t st) { return NT_BY_TC(launch_wsn_t, r, a, st); }
int launch_ring(const uvc_gemm_route& r, const NtArgs& a, hipStream_t st) { return r.c_f32 ? launch_ring_t<false>(r, a, st) : launch_ring_t<true>(r, a, st); }
}  // namespace uvc_gemm
