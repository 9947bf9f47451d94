// NT GEMM that keeps the weights in registers and streams the activation rows (bf16): the skinny GEMMs of the narrow models.
//   k_gemm_ws<TA, TC, EPI, KT, NW, NJ>   K = 192 / 128                                  UVC_ROUTE_WS
//                                        K = 384 as 6 or 8 waves x 32 columns           UVC_ROUTE_WS384
// A file of its own because it is 173 of the GEMMs' 405 kernel instantiations and more than a third of their compile time.
#include "gemm_common.h"

// ================================================================================================
//                     NT, weights-stationary / activation-streaming (bf16, K <= 192)
// ================================================================================================
// The DeiT GEMMs are skinny: M = B*197 rows (1e5) against K, N of a few hundred, i.e. HBM-bound
// streaming of A and C with a weight matrix that fits in registers.  Each wave keeps the MFMA B
// fragments of its 64 output columns in VGPRs for its whole life (KT*4 fragments), the workgroup
// (3 waves = 192 columns) walks M persistently in 64-row tiles, A is staged once per tile through a
// double-buffered LDS image (register prefetch of tile i+1 under the MFMAs of tile i) and shared by
// the three waves, and C leaves through a wave-private LDS transpose as whole 128/256-byte rows.
// LDS traffic per MFMA is half of the generic kernel's (no B reads) and A is read exactly once per
// 192-column group; groups of one tile sequence are placed on one XCD so they share its L2.
constexpr int WS_BM = 64;

// NJ = 16-column accumulator tiles per wave: 4 (64 columns, 96 VGPRs of W at K = 192, two waves per SIMD) or 2 (32 columns, 48 VGPRs,
// eight waves per workgroup, four per SIMD: the GELU epilogues of fc1 overlap its stores better)
// KT = 12 (K = 384: DeiT-Small / T2T-ViT widths) runs as 6 waves x 32 columns: the wave's W slice is 96 VGPRs again, the two A images
// (64 rows x 800 B) and the transpose buffers take 116 KB of dynamic LDS, one workgroup per CU.
template <typename TA, typename TC, int EPI, int KT, int WS_NW, int NJ = 4>
__global__ __launch_bounds__(64 * WS_NW, (KT > 6 && WS_NW > 6) ? 1 : (NJ == 4 || KT > 6) ? 2 : 4) void k_gemm_ws(NtArgs g, int ngroups, int nslots) {
  typedef bf16_t T;
  typedef Mma<T> MM;
  constexpr int ROWB = KT * 64 + 32;             // bytes per staged A row (KT*32 bf16 + pad; words = 8 or 40 mod 64, see NT_ROWB)
  constexpr int CPR = KT * 4;                    // 16-byte chunks per row
  constexpr int NLD = (WS_BM * CPR + 64 * WS_NW - 1) / (64 * WS_NW);
  constexpr int CW = 16 * NJ, EPW = CW + 4;         // columns per wave; floats per staged accumulator row
  constexpr int VN = OutVec<TC>::VN, LPR = CW / VN, RPI = 64 / LPR;
  constexpr bool DYN = KT > 6;
  constexpr int IMGB = WS_BM * ROWB;
  extern __shared__ __attribute__((aligned(16))) char ws_dyn[];
  __shared__ __attribute__((aligned(16))) char sA_st[DYN ? 16 : 2 * IMGB];
  __shared__ __attribute__((aligned(16))) float sStage_st[DYN ? 4 : WS_NW * 16 * EPW];
  char* const sAb = DYN ? ws_dyn : sA_st;
  float* const sStg = DYN ? reinterpret_cast<float*>(ws_dyn + 2 * IMGB) : sStage_st;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, gq = lane >> 4, li = lane & 15;
  const int L = blockIdx.x;
  const int grp = (L >> 3) % ngroups, slot = (L / (8 * ngroups)) * 8 + (L & 7);
  const int n0 = grp * CW * WS_NW + w * CW;
  const bool active = n0 < g.N;                  // N % 64 == 0: a wave is either fully inside or idle
  const TA* __restrict__ A = reinterpret_cast<const TA*>(g.A);
  const T* __restrict__ W = reinterpret_cast<const T*>(g.B);
  TC* __restrict__ C = reinterpret_cast<TC*>(g.C);
  const int ntiles = (g.M + WS_BM - 1) / WS_BM;

  typename MM::Frag bf[NJ][KT];
  if (active) {
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int ks = 0; ks < KT; ++ks)
        bf[j][ks] = __builtin_bit_cast(typename MM::Frag, *reinterpret_cast<const u32x4*>(W + (size_t)(n0 + j * 16 + li) * g.ldb + (ks * 4 + gq) * 8));
  }
  float alpha = g.alpha;
  if (g.alpha_ptr) alpha *= *g.alpha_ptr;
  float d0 = 0.f, d1 = 1.f;
  if (EPI == UVC_EPI_BIAS_RESID_GATE) { d0 = g.dptr[0]; d1 = g.dptr[1]; }
  const int cc = (lane % LPR) * VN;
  const int n = n0 + cc;
  float bias_v[VN];
#pragma unroll
  for (int e = 0; e < VN; ++e) bias_v[e] = 0.f;
  if (active && (EPI == UVC_EPI_BIAS || EPI == UVC_EPI_BIAS_GELU || EPI == UVC_EPI_BIAS_GELU_OUT || EPI == UVC_EPI_BIAS_RESID || EPI == UVC_EPI_BIAS_RESID_GATE ||
                 EPI == UVC_EPI_BIAS_GELU_GRAD || EPI == UVC_EPI_BIAS_GELU_GRAD_Q8)) {
#pragma unroll
    for (int e = 0; e < VN; ++e) bias_v[e] = g.bias[n + e];
  }

  u32x4 ra[NLD];
  auto gload = [&](int tile) {
    const int m0 = tile * WS_BM;
    const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int id = tid + 64 * WS_NW * i, row = id / CPR, c = id % CPR;
      const int m = m0 + row;
      ra[i] = (row < WS_BM && m < g.M) ? ChunkLoad<TA, T>::ld(A + (size_t)m * g.lda + c * 8) : z;
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int id = tid + 64 * WS_NW * i, row = id / CPR, c = id % CPR;
      if (row < WS_BM) *reinterpret_cast<u32x4*>(sAb + buf * IMGB + row * ROWB + c * 16) = ra[i];
    }
  };

  // epilogue operands (residual rows / GELU pre-activation) are prefetched one 16-row sub-tile ahead into
  // registers, so their HBM latency hides under the epilogue math of the previous sub-tile and the MFMAs
  // of the current one.  The accumulator transpose buffer is private to a wave: DS operations of one wave
  // execute in order, so only a compiler-level wave barrier separates its writes from its reads.
  constexpr int IT = 16 / RPI;
  struct Epi { u32x4 r[IT]; u32x4 r2[IT]; u32x4 ax[IT]; };      // r, r2: VN residual values of C's element type in 16 bytes
  auto eload = [&](Epi& E, int tile_, int sub_) {
    if (!active) return;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int m = tile_ * WS_BM + sub_ * 16 + it * RPI + lane / LPR;
      const bool ok = m < g.M && tile_ < ntiles;
      const size_t mo = (size_t)(ok ? m : 0);
      if (EPI == UVC_EPI_BIAS_RESID || EPI == UVC_EPI_BIAS_RESID_GATE) E.r[it] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const TC*>(g.R) + mo * g.ldr + n);
      if (EPI == UVC_EPI_BIAS_RESID_GATE) E.r2[it] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const TC*>(g.R2) + mo * g.ldr + n);
      if (EPI == UVC_EPI_DGELU || EPI == UVC_EPI_MUL_AUX) {    // the lane's VN columns of aux (bf16): 16 bytes beside a bf16 C, 8 beside a float32 C
        if constexpr (VN == 8) E.ax[it] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(g.aux) + mo * g.ldaux + n);
        else {
          const u32x2 q = *reinterpret_cast<const u32x2*>(reinterpret_cast<const T*>(g.aux) + mo * g.ldaux + n);
          E.ax[it][0] = q[0]; E.ax[it][1] = q[1];
        }
      }
      if (EPI == UVC_EPI_MUL_AUX_Q8) {          // 8 one-byte codes of GELU'(a) (include/uvc_kernels.h)
        const u32x2 q = *reinterpret_cast<const u32x2*>(reinterpret_cast<const unsigned char*>(g.aux) + mo * g.ldaux + n);
        E.ax[it][0] = q[0]; E.ax[it][1] = q[1];
      }
    }
  };
  auto subtile = [&](int buf_, int m0_, int sub_, const Epi& E) {
    if (!active) return;
    float* stg = sStg + w * (16 * EPW);
    {
      typename MM::Frag fa[KT];
#pragma unroll
      for (int ks = 0; ks < KT; ++ks) fa[ks] = lds_frag<T>(sAb + buf_ * IMGB + (sub_ * 16 + li) * ROWB + (ks * 4 + gq) * 16);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KT; ++ks) c = MM::mma(bf[j][ks], fa[ks], c);
        *reinterpret_cast<f32x4*>(stg + li * EPW + j * 16 + gq * 4) = c;
      }
    }
    __builtin_amdgcn_wave_barrier();
    unsigned qc[IT][2];                                     // UVC_EPI_BIAS_GELU_GRAD_Q8: the lane's 8 one-byte codes of each of its rows
#pragma unroll
    for (int it = 0; it < IT; ++it) { qc[it][0] = 0u; qc[it][1] = 0u; }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int r = it * RPI + lane / LPR;
      const int m = m0_ + sub_ * 16 + r;
      float v[VN];
      load_vec<float, VN>(stg + r * EPW + cc, v);
      if (m < g.M) {
        const size_t mo = (size_t)m;
#pragma unroll
        for (int e = 0; e < VN; ++e) v[e] = epi_scale_bias(v[e], alpha, bias_v[e]);
        if (EPI == UVC_EPI_BIAS_RESID || EPI == UVC_EPI_BIAS_RESID_GATE) {
          float rv[VN];
          Resid<TC>::get(E.r[it], rv);
#pragma unroll
          for (int e = 0; e < VN; ++e) v[e] += rv[e];
        }
        if (EPI == UVC_EPI_BIAS_RESID_GATE) {
          float rv[VN];
          Resid<TC>::get(E.r2[it], rv);
#pragma unroll
          for (int e = 0; e < VN; ++e) v[e] = epi_gate_mix(v[e], rv[e], d0, d1);
        }
        if (EPI == UVC_EPI_DGELU) {
#pragma unroll
          for (int e = 0; e < VN / 2; ++e) {
            v[2 * e] *= Gelu<T>::g(__uint_as_float(E.ax[it][e] << 16));
            v[2 * e + 1] *= Gelu<T>::g(__uint_as_float(E.ax[it][e] & 0xffff0000u));
          }
        }
        if (EPI == UVC_EPI_MUL_AUX) {
#pragma unroll
          for (int e = 0; e < VN / 2; ++e) {
            v[2 * e] *= __uint_as_float(E.ax[it][e] << 16);
            v[2 * e + 1] *= __uint_as_float(E.ax[it][e] & 0xffff0000u);
          }
        }
        if constexpr (EPI == UVC_EPI_MUL_AUX_Q8) {
          static_assert(VN == 8, "q8 epilogue: bf16 C");
#pragma unroll
          for (int e = 0; e < 8; ++e)            // (byte -> float is one v_cvt_f32_ubyteN)
            v[e] *= __builtin_fmaf((float)((E.ax[it][e >> 2] >> (8 * (e & 3))) & 0xffu), UVC_Q8_STEP, UVC_Q8_LO);
        }
        if (EPI == UVC_EPI_BIAS_GELU_OUT) {
#pragma unroll
          for (int e = 0; e < VN; ++e) v[e] = Gelu<T>::f(v[e]);
        }
        float u[VN];
        if (EPI == UVC_EPI_BIAS_GELU_GRAD || EPI == UVC_EPI_BIAS_GELU_GRAD_Q8) {
#pragma unroll
          for (int e = 0; e < VN; ++e) { float fo, go; Gelu<T>::fg(v[e], fo, go); u[e] = fo; v[e] = go; }
        }
        if constexpr (EPI == UVC_EPI_BIAS_GELU_GRAD_Q8) {
          // GELU'(a) as one byte per activation (include/uvc_kernels.h): 8 codes = 8 bytes per lane, 64-byte row pieces per wave; GELU(a) as before.  Both stream
          // past the caches (read again in the backward / by fc2)
          static_assert(VN == 8, "q8 epilogue: bf16 C2");
          unsigned qw[2] = {0u, 0u};
#pragma unroll
          for (int e = 0; e < 8; ++e)       // v_cvt_pk_u8_f32: round to nearest, saturate to [0, 255], pack into byte e & 3 -- two VALU instructions per code
            qw[e >> 2] = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_fmaf(v[e], 1.0f / UVC_Q8_STEP, -UVC_Q8_LO / UVC_Q8_STEP), e & 3, qw[e >> 2]);
          qc[it][0] = qw[0]; qc[it][1] = qw[1];            // stored behind the loop: 16 bytes per lane (below)
          OutVec<TC>::st_nt(reinterpret_cast<TC*>(g.C2) + mo * g.ldc + n, u);
        } else {
        // GELU'(a) and GELU(a) of the training forward are STREAMING outputs (310 MB per block, read again in the backward / by fc2 after the caches have
        // turned over): non-temporal stores.  Alone 90.2 -> 83.1 us; in the step 11.19 -> 10.96 ms (GELU' only: 79.8 us alone, 11.09 in the step) -- the rest of
        // the step keeps the Infinity Cache (profiles/r5zz_ab_nt_stores.txt).  K = 192 only: at K = 384 (DeiT-Small, T2T-ViT-14) the same stores are within
        // noise or 0.5 % slower (profiles/r5zz_ab_nt_wide.txt)
        if constexpr (EPI == UVC_EPI_BIAS_GELU_GRAD && sizeof(TC) == 2 && KT == 6) OutVec<TC>::st_nt(C + mo * g.ldc + n, v);
        else
        // (also tried, each within +- 0.4 % of the step: non-temporal dA stores of dfc2 x GELU', non-temporal loads of its GELU' operand, nt on the LDS-DMA loads
        //  of the weight gradients and of the attention backward -- profiles/r5zz_ab_nt_sites.txt)
        OutVec<TC>::st(C + mo * g.ldc + n, v);
        if (EPI == UVC_EPI_BIAS_GELU || EPI == UVC_EPI_BIAS_GELU_GRAD) {
          if (EPI == UVC_EPI_BIAS_GELU) {
#pragma unroll
            for (int e = 0; e < VN; ++e) u[e] = Gelu<T>::f(v[e]);
          }
          if constexpr (EPI == UVC_EPI_BIAS_GELU_GRAD && sizeof(TC) == 2 && KT == 6) OutVec<TC>::st_nt(reinterpret_cast<TC*>(g.C2) + mo * g.ldc + n, u);
          else
          OutVec<TC>::st(reinterpret_cast<TC*>(g.C2) + mo * g.ldc + n, u);
        }
        }
      }
    }
    if constexpr (EPI == UVC_EPI_BIAS_GELU_GRAD_Q8) {
      // The codes leave as 16 bytes per lane, ONE store instruction per 16-row sub-tile instead of two of 8 bytes: fc1's epilogue is bound by its store
      // instructions as much as by its bytes (8-byte stores of the codes: the step 10.93 -> 10.90 ms where the tensor not written at all gives 10.70,
      // profiles/r6d, r6b).  Lanes l, l ^ 1 hold neighbouring 8-column groups of the SAME two rows (it = 0, 1): the even lane takes both groups of row 0,
      // the odd lane both groups of row 1 (one DPP quad permute per dword).
      const bool odd = lane & 1;
      if constexpr (IT == 2) {
        static_assert(LPR == 8 && RPI == 8, "q8 epilogue: four waves x 64 columns");
        const unsigned s0 = odd ? qc[0][0] : qc[1][0], s1 = odd ? qc[0][1] : qc[1][1];      // what the partner stores: my codes of ITS row
        const unsigned r0 = (unsigned)__builtin_amdgcn_mov_dpp((int)s0, 0xB1, 0xF, 0xF, true);      // quad_perm [1, 0, 3, 2]: lane ^ 1
        const unsigned r1 = (unsigned)__builtin_amdgcn_mov_dpp((int)s1, 0xB1, 0xF, 0xF, true);
        const int m = m0_ + sub_ * 16 + (odd ? RPI : 0) + lane / LPR;
        if (m < g.M) {
          const u32x4 o = odd ? u32x4{r0, r1, qc[1][0], qc[1][1]} : u32x4{qc[0][0], qc[0][1], r0, r1};
          __builtin_nontemporal_store(o, reinterpret_cast<u32x4*>(reinterpret_cast<unsigned char*>(g.C) + (size_t)m * g.ldc + (n & ~15)));
        }
      } else {
        // eight waves x 32 columns: one row per lane and sub-tile; the even lane of a pair stores both 8-column groups of the row
        static_assert(IT == 1 && LPR == 4, "q8 epilogue: eight waves x 32 columns");
        const unsigned r0 = (unsigned)__builtin_amdgcn_mov_dpp((int)qc[0][0], 0xB1, 0xF, 0xF, true);
        const unsigned r1 = (unsigned)__builtin_amdgcn_mov_dpp((int)qc[0][1], 0xB1, 0xF, 0xF, true);
        const int m = m0_ + sub_ * 16 + lane / LPR;
        if (m < g.M && !odd)
          __builtin_nontemporal_store(u32x4{qc[0][0], qc[0][1], r0, r1}, reinterpret_cast<u32x4*>(reinterpret_cast<unsigned char*>(g.C) + (size_t)m * g.ldc + n));
      }
    }
    __builtin_amdgcn_wave_barrier();
  };

  int tile = slot;
  if (tile >= ntiles) return;
  Epi E0, E1;
  gload(tile);
  eload(E0, tile, 0);
  lstore(0);
  __syncthreads();
  int buf = 0;
  for (; tile < ntiles; tile += nslots) {
    const int next = tile + nslots;
    if (next < ntiles) gload(next);
    const int m0 = tile * WS_BM;
    eload(E1, tile, 1);
    subtile(buf, m0, 0, E0);
    eload(E0, tile, 2);
    subtile(buf, m0, 1, E1);
    eload(E1, tile, 3);
    subtile(buf, m0, 2, E0);
    eload(E0, next, 0);
    subtile(buf, m0, 3, E1);
    if (next < ntiles) lstore(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }
}

// ---- host code: the launchers (grid, LDS bytes, launch; they decide nothing) and what gemm.hip calls
namespace {

// k_gemm_ws: `wgs` workgroups in all (512 at K = 192 / 128: ~2 per CU -- 1024 / 2048 cost +0.10 / +0.15 ms in the step, profiles/r6o_ab_ws_slots_not_kept.txt;
// 256 at K = 384: one per CU), slots a multiple of the 8 XCDs
int ws_slots(const NtArgs& a, int ngroups, int wgs) {
  const int ntiles = ceil_div(a.M, WS_BM);
  int nslots = (wgs / ngroups) & ~7;
  if (nslots < 8) nslots = 8;
  if (nslots > ((ntiles + 7) & ~7)) nslots = (ntiles + 7) & ~7;
  return nslots;
}
template <typename TA, typename TC, int KT, int WS_NW>
int launch_ws_epi(const NtArgs& a, int epi, hipStream_t st) {
  const int ngroups = ceil_div(a.N, 64 * WS_NW), nslots = ws_slots(a, ngroups, 512);
  const int grid = nslots * ngroups;
  if (epi == UVC_EPI_BIAS_GELU_GRAD_Q8) {                  // (bf16 operands and outputs, K = 192, four waves x 64 columns: nt_route checked)
    if constexpr (sizeof(TA) == 2 && sizeof(TC) == 2 && KT == 6 && WS_NW == 4) {
      k_gemm_ws<TA, TC, UVC_EPI_BIAS_GELU_GRAD_Q8, KT, WS_NW><<<grid, 64 * WS_NW, 0, st>>>(a, ngroups, nslots);
      UVC_CHECK_LAUNCH();
      return UVC_OK;
    } else return uvc_set_error_msg(UVC_ERR_UNSUPPORTED, "uvc_gemm_nt: UVC_EPI_BIAS_GELU_GRAD_Q8 outside uvc_gemm_nt_q8_supported");
  }
#define WS_CASE(E) case E: k_gemm_ws<TA, TC, E, KT, WS_NW><<<grid, 64 * WS_NW, 0, st>>>(a, ngroups, nslots); break;
  NT_LAUNCH(epi, NT_EPI9(WS_CASE))
#undef WS_CASE
}
template <typename TA, typename TC, int KT>
int launch_ws_narrow(const NtArgs& a, int epi, hipStream_t st) {      // 8 waves x 32 columns
  const int ngroups = ceil_div(a.N, 256), nslots = ws_slots(a, ngroups, 512);
  const int grid = nslots * ngroups;
#define WS_CASE(E) case E: k_gemm_ws<TA, TC, E, KT, 8, 2><<<grid, 512, 0, st>>>(a, ngroups, nslots); break;
  NT_LAUNCH(epi, WS_CASE(UVC_EPI_DGELU) WS_CASE(UVC_EPI_MUL_AUX) WS_CASE(UVC_EPI_MUL_AUX_Q8) WS_CASE(UVC_EPI_BIAS_GELU_GRAD_Q8))
#undef WS_CASE
}
template <typename TA, typename TC>
int launch_ws_t(const uvc_gemm_route& r, const NtArgs& a, hipStream_t st) {
  if constexpr (sizeof(TC) == 2 && sizeof(TA) == 2) {
    if (r.nw == 8) return launch_ws_narrow<TA, TC, 6>(a, r.epilogue, st);
  }
  if (r.kt == 6) return r.nw == 4 ? launch_ws_epi<TA, TC, 6, 4>(a, r.epilogue, st) : launch_ws_epi<TA, TC, 6, 3>(a, r.epilogue, st);
  return r.nw == 4 ? launch_ws_epi<TA, TC, 4, 4>(a, r.epilogue, st) : launch_ws_epi<TA, TC, 4, 3>(a, r.epilogue, st);
}
template <typename TC, int NW = 6>
int launch_ws384_t(const NtArgs& a, int epi, hipStream_t st) {
  constexpr int KT = 12, NJ = 2;
  const int ngroups = ceil_div(a.N, 32 * NW), nslots = ws_slots(a, ngroups, 256);     // (a last group with idle waves: N = 1152 on eight waves is 4.5 groups)
  const int grid = nslots * ngroups;
  const int sh = 2 * WS_BM * (KT * 64 + 32) + NW * 16 * (16 * NJ + 4) * 4;
#define WS_CASE(E) case E: { \
    UVC_MAX_LDS(sh, k_gemm_ws<bf16_t, TC, E, KT, NW, NJ>); \
    k_gemm_ws<bf16_t, TC, E, KT, NW, NJ><<<grid, 64 * NW, sh, st>>>(a, ngroups, nslots); } break;
  NT_LAUNCH(epi, WS_CASE(UVC_EPI_NONE) WS_CASE(UVC_EPI_BIAS) WS_CASE(UVC_EPI_BIAS_GELU) WS_CASE(UVC_EPI_BIAS_RESID) WS_CASE(UVC_EPI_BIAS_RESID_GATE)
                      WS_CASE(UVC_EPI_BIAS_GELU_OUT) WS_CASE(UVC_EPI_BIAS_GELU_GRAD) WS_CASE(UVC_EPI_MUL_AUX))
#undef WS_CASE
}

}  // namespace

namespace uvc_gemm {
int launch_ws(const uvc_gemm_route& r, const NtArgs& a, hipStream_t st) { return NT_BY_TA_TC(launch_ws_t, r, a, st); }
int launch_ws384(const uvc_gemm_route& r, const NtArgs& a, hipStream_t st) {
  return r.nw == 8 ? launch_ws384_t<bf16_t, 8>(a, r.epilogue, st) : NT_BY_TC(launch_ws384_t, a, r.epilogue, st);
}
}  // namespace uvc_gemm
