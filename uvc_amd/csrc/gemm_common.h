// What the GEMM kernels share across files: MFMA and operand-load traits, the NT kernels' argument block and staged epilogue, the inline-assembly LDS
// accesses and counted waits of the LDS-DMA kernels, the LayerNorm-backward argument block, the tile sizes the routing reads, the launch macros, and
// the launchers through which uvc_gemm_nt (gemm.hip) reaches the kernel families.  No kernel is defined here: a kernel template lives in exactly one
// gemm*.hip and is instantiated there only.  One header, not one per topic: every gemm*.hip includes this one already, and what is shared is a page;
// a definition is here only when more than one file uses it.
//   gemm_nt_tiled.hip   k_gemm_nt, k_gemm_nt_rows                           UVC_ROUTE_NT, NT_ROWS
//   gemm_nt_ws.hip      k_gemm_ws                                           UVC_ROUTE_WS, WS384
//   gemm_nt_wsn.hip     k_gemm_wsn, k_gemm_wsn16, k_gemm_wsn16_dma          UVC_ROUTE_WSN, WSN16, WSN16_DMA
//   gemm_nt_lnbwd.hip   k_gemm_wsn_lnbwd, k_gemm_wsn_lnbwd_dma              uvc_gemm_nt_lnbwd at D = 192
//   gemm_nt_wide.hip    k_gemm_nt256, k_gemm_row384_lnbwd, k_gemm_nt8p      UVC_ROUTE_NT256, ROW384, NT8P; uvc_gemm_nt_lnbwd at D = 384
//   gemm_tn.hip         k_gemm_tn, _tn_big, _tn_dma, _tn8p, k_tn_reduce     uvc_gemm_tn and its routing
//   gemm.hip            no kernel: the routing of uvc_gemm_nt, its entry point, the route -> kernel name table
#pragma once
#include <type_traits>
#include "common.h"
#include "../../include/uvc_kernels.h"

// ------------------------------------------------------------------------------------------------
template <typename T> struct Mma;
template <> struct Mma<bf16_t> {
  static constexpr int CH = 8;     // elements per 16-byte chunk
  static constexpr int KSTEP = 32; // k elements per MFMA step (4 lane groups x 1 chunk)
  typedef bf16x8 Frag;
  static __device__ __forceinline__ f32x4 mma(const Frag& a, const Frag& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
};
template <> struct Mma<float> {
  static constexpr int CH = 4;
  static constexpr int KSTEP = 16;
  typedef f32x4 Frag;
  static __device__ __forceinline__ f32x4 mma(const Frag& a, const Frag& b, f32x4 c) {
#pragma unroll
    for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], c, 0, 0, 0);
    return c;
  }
};

// 16-byte chunk of compute type T loaded from a global array of type TS (convert on load)
template <typename TS, typename T> struct ChunkLoad;
template <typename T> struct ChunkLoad<T, T> {
  static __device__ __forceinline__ u32x4 ld(const T* p) { return *reinterpret_cast<const u32x4*>(p); }
};
template <> struct ChunkLoad<float, bf16_t> {   // 8 floats -> 8 bf16
  static __device__ __forceinline__ u32x4 ld(const float* p) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p);
    const f32x4 b = *reinterpret_cast<const f32x4*>(p + 4);
    u32x4 r;
    r[0] = pack_bf16x2(a[0], a[1]); r[1] = pack_bf16x2(a[2], a[3]);
    r[2] = pack_bf16x2(b[0], b[1]); r[3] = pack_bf16x2(b[2], b[3]);
    return r;
  }
};

template <typename T> __device__ __forceinline__ typename Mma<T>::Frag lds_frag(const char* p) {
  return *reinterpret_cast<const typename Mma<T>::Frag*>(p);
}

template <typename T> struct OutIO;
template <> struct OutIO<float> {
  static __device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
  static __device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
};
template <> struct OutIO<bf16_t> {
  static __device__ __forceinline__ void st4(bf16_t* p, f32x4 v) {
    u32x2 r; r[0] = pack_bf16x2(v[0], v[1]); r[1] = pack_bf16x2(v[2], v[3]);
    *reinterpret_cast<u32x2*>(p) = r;
  }
  static __device__ __forceinline__ f32x4 ld4(const bf16_t* p) {
    const u32x2 r = *reinterpret_cast<const u32x2*>(p);
    f32x4 v; v[0] = __uint_as_float(r[0] << 16); v[1] = __uint_as_float(r[0] & 0xffff0000u);
    v[2] = __uint_as_float(r[1] << 16); v[3] = __uint_as_float(r[1] & 0xffff0000u);
    return v;
  }
};

struct NtArgs {
  const void* A; const void* B; void* C; void* C2;
  const float* bias; const void* R; const void* R2; const void* aux; const float* dptr;      // R, R2: the residual rows, element type of C
  int M, N, K, lda, ldb, ldc, ldr, ldaux;
  float alpha;
  const float* alpha_ptr;   // optional device scalar multiplied into alpha
  // optional second output of the N == 192 residual epilogues: LayerNorm of the output rows (uvc_gemm_nt_args.ln_*)
  const float* ln_gamma; const float* ln_beta; void* ln_out; float* ln_mean; float* ln_rstd; float ln_eps;
  int no_dma;               // uvc_gemm_nt_args.force_generic == 2: the register-staged streaming kernels instead of the LDS-DMA rings
};

// vector of VN consecutive outputs in the coalesced epilogue layout
template <typename TC> struct OutVec;
template <> struct OutVec<float> {
  static constexpr int VN = 4;
  static __device__ __forceinline__ void st(float* p, const float* v) { *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]}; }
};
template <> struct OutVec<bf16_t> {
  static constexpr int VN = 8;
  static __device__ __forceinline__ void st(bf16_t* p, const float* v) {
    u32x4 r;
    r[0] = pack_bf16x2(v[0], v[1]); r[1] = pack_bf16x2(v[2], v[3]); r[2] = pack_bf16x2(v[4], v[5]); r[3] = pack_bf16x2(v[6], v[7]);
    *reinterpret_cast<u32x4*>(p) = r;
  }
  static __device__ __forceinline__ void st_nt(bf16_t* p, const float* v) {      // streaming output: not read again before the caches have turned over
    u32x4 r;
    r[0] = pack_bf16x2(v[0], v[1]); r[1] = pack_bf16x2(v[2], v[3]); r[2] = pack_bf16x2(v[4], v[5]); r[3] = pack_bf16x2(v[6], v[7]);
    __builtin_nontemporal_store(r, reinterpret_cast<u32x4*>(p));
  }
};
template <typename T, int VN> __device__ __forceinline__ void load_vec(const T* p, float* v);
template <> __device__ __forceinline__ void load_vec<float, 4>(const float* p, float* v) {
  const f32x4 r = *reinterpret_cast<const f32x4*>(p); v[0] = r[0]; v[1] = r[1]; v[2] = r[2]; v[3] = r[3];
}
template <> __device__ __forceinline__ void load_vec<float, 8>(const float* p, float* v) { load_vec<float, 4>(p, v); load_vec<float, 4>(p + 4, v + 4); }
template <> __device__ __forceinline__ void load_vec<bf16_t, 8>(const bf16_t* p, float* v) {
  const u32x4 r = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[2 * e] = __uint_as_float(r[e] << 16); v[2 * e + 1] = __uint_as_float(r[e] & 0xffff0000u); }
}
template <> __device__ __forceinline__ void load_vec<bf16_t, 4>(const bf16_t* p, float* v) {
  const u32x2 r = *reinterpret_cast<const u32x2*>(p);
  v[0] = __uint_as_float(r[0] << 16); v[1] = __uint_as_float(r[0] & 0xffff0000u);
  v[2] = __uint_as_float(r[1] << 16); v[3] = __uint_as_float(r[1] & 0xffff0000u);
}

// Residual operands have the element type of C (float32 stream: 4 floats per 16 bytes; bf16 stream: 8 per 16 bytes, 4 per 8 bytes)
template <typename TC> struct Resid;
template <> struct Resid<float> {
  typedef u32x4 Raw4;                            // four consecutive columns
  static __device__ __forceinline__ Raw4 ld4(const void* base, size_t elem) { return *reinterpret_cast<const u32x4*>(reinterpret_cast<const float*>(base) + elem); }
  static __device__ __forceinline__ f32x4 f4(const Raw4& r) { return __builtin_bit_cast(f32x4, r); }
  // VN = 4 consecutive columns in 16 bytes
  static __device__ __forceinline__ void get(const u32x4& r, float* v) { const f32x4 f = __builtin_bit_cast(f32x4, r); v[0] = f[0]; v[1] = f[1]; v[2] = f[2]; v[3] = f[3]; }
};
template <> struct Resid<bf16_t> {
  typedef u32x2 Raw4;
  static __device__ __forceinline__ Raw4 ld4(const void* base, size_t elem) { return *reinterpret_cast<const u32x2*>(reinterpret_cast<const bf16_t*>(base) + elem); }
  static __device__ __forceinline__ f32x4 f4(const Raw4& r) {
    return f32x4{__uint_as_float(r[0] << 16), __uint_as_float(r[0] & 0xffff0000u), __uint_as_float(r[1] << 16), __uint_as_float(r[1] & 0xffff0000u)};
  }
  // VN = 8 consecutive columns in 16 bytes
  static __device__ __forceinline__ void get(const u32x4& r, float* v) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[2 * e] = __uint_as_float(r[e] << 16); v[2 * e + 1] = __uint_as_float(r[e] & 0xffff0000u); }
  }
};

// Epilogue arithmetic with the rounding points spelled out (hipcc contracts a*b + c*d differently from kernel to kernel):
// every NT kernel computes the same bits for the same accumulator, so a row's result does not depend on which kernel the
// problem size selects (tests/test_fullsize_gpu.py compares a 512-image run with an 8-image run bit for bit).
__device__ __forceinline__ float epi_scale_bias(float acc, float alpha, float bias) { return __builtin_fmaf(acc, alpha, bias); }
__device__ __forceinline__ float epi_gate_mix(float v, float r2, float d0, float d1) { return __builtin_fmaf(d1, v, __builtin_fmaf(d0, r2, 0.0f)); }
constexpr int EP_LD = 68;   // floats per staged accumulator row (64 + 4 pad: conflict-free 16-byte LDS writes)

// Epilogue of ROWS staged accumulator rows x 64 columns of one wave (row r = output row mrow0 + r, columns ncol0 .. ncol0 + 63):
// scale / bias / residual / gate mix / activation, then 16-byte row-contiguous stores.  Shared by the NT kernels that leave through an
// LDS transpose, so that a row's bits do not depend on the kernel that produced its accumulator.
// Staging layouts: SWZ = false: [ROWS][EP_LD] floats (padded rows); SWZ = true: [ROWS][64] floats, the 16-byte column group cg of row r
// at group cg ^ (r & 7) (no padding: 4 KB per 16 rows; conflict-free for the accumulator writes and for these reads).
// bias_v: the VN bias values of this lane's columns (0 where the epilogue has no bias or the column is past N), loaded once per tile.
template <bool SWZ> __device__ __forceinline__ float* stg_at(float* stg, int r, int cg) {
  return SWZ ? stg + r * 64 + ((cg ^ (r & 7)) << 2) : stg + r * EP_LD + (cg << 2);
}
template <typename TC, int EPI> __device__ __forceinline__ void nt_load_bias(const NtArgs& g, int lane, int ncol0, float* bias_v) {
  constexpr int VN = OutVec<TC>::VN, LPR = 64 / VN;
  constexpr bool has_bias = EPI == UVC_EPI_BIAS || EPI == UVC_EPI_BIAS_GELU || EPI == UVC_EPI_BIAS_GELU_OUT || EPI == UVC_EPI_BIAS_RESID ||
                            EPI == UVC_EPI_BIAS_RESID_GATE || EPI == UVC_EPI_BIAS_GELU_GRAD;
  const int n = ncol0 + (lane % LPR) * VN;
#pragma unroll
  for (int e = 0; e < VN; ++e) bias_v[e] = (has_bias && n + e < g.N) ? g.bias[n + e] : 0.f;
}
// Operand rows of an epilogue (R, R2, aux) requested AHEAD of the rows they meet: the epilogue of a big tile is a chain of [transpose 16 rows
// through LDS | load their operands | arithmetic | store]; with the loads inside the chain every 16-row step was a memory round trip (dfc2 x GELU'
// of DeiT-Base: 24 us of epilogue per 256 x 256 tile against 16 us of k-loop).  bf16 C only (16 bytes = the lane's 8 columns); a lane whose
// columns are not a whole aligned vector (ragged N, odd leading dimensions) keeps loading in place.
template <int NIT> struct EpiPre { u32x4 r[NIT], r2[NIT], ax[NIT]; };
template <int EPI> struct EpiOperands {
  static constexpr bool R = EPI == UVC_EPI_BIAS_RESID || EPI == UVC_EPI_BIAS_RESID_GATE, R2 = EPI == UVC_EPI_BIAS_RESID_GATE,
                        AUX = EPI == UVC_EPI_DGELU || EPI == UVC_EPI_MUL_AUX;
  static constexpr int COUNT = (R ? 1 : 0) + (R2 ? 1 : 0) + (AUX ? 1 : 0);
};
template <int EPI, int ROWS>
__device__ __forceinline__ void nt_epilogue_prefetch(const NtArgs& g, int lane, int mrow0, int ncol0, EpiPre<ROWS / 8>& P) {
  const int cc = (lane & 7) * 8, n = ncol0 + cc;
  const bool nfull = (n + 8 <= g.N) && ((g.ldc % 8) == 0);
#pragma unroll
  for (int it = 0; it < ROWS / 8; ++it) {
    const int m = mrow0 + it * 8 + (lane >> 3);
    if (m < g.M && nfull) {
      const size_t mo = (size_t)m;
      if (EpiOperands<EPI>::R && (g.ldr % 8) == 0) P.r[it] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const bf16_t*>(g.R) + mo * g.ldr + n);
      if (EpiOperands<EPI>::R2 && (g.ldr % 8) == 0) P.r2[it] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const bf16_t*>(g.R2) + mo * g.ldr + n);
      if (EpiOperands<EPI>::AUX && (g.ldaux % 8) == 0) P.ax[it] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const bf16_t*>(g.aux) + mo * g.ldaux + n);
    }
  }
}
template <typename T, typename TC, int EPI, int ROWS = 32, bool SWZ = false, bool PRE = false>
__device__ __forceinline__ void nt_epilogue_rows(const NtArgs& g, float* stg, int lane, int mrow0, int ncol0, float alpha, float d0, float d1,
                                                 const float* bias_v, const EpiPre<ROWS / 8>* pre = nullptr) {
  static_assert(!PRE || (sizeof(TC) == 2 && sizeof(T) == 2), "operand prefetch: bf16 C and operands only");
  constexpr int VN = OutVec<TC>::VN;
  constexpr int LPR = 64 / VN;                  // lanes per 64-column row
  constexpr int RPI = 64 / LPR;                 // rows per wave instruction
  TC* __restrict__ C = reinterpret_cast<TC*>(g.C);
  const int cc = (lane % LPR) * VN;
  const int n = ncol0 + cc;
  const bool nfull = (n + VN <= g.N) && ((g.ldc % VN) == 0);
#pragma unroll
  for (int it = 0; it < ROWS / RPI; ++it) {
    const int r = it * RPI + lane / LPR;
    const int m = mrow0 + r;
    float v[VN];
    load_vec<float, 4>(stg_at<SWZ>(stg, r, cc >> 2), v);
    if (VN == 8) load_vec<float, 4>(stg_at<SWZ>(stg, r, (cc >> 2) + 1), v + 4);
    if (m < g.M && n < g.N) {
      const size_t mo = (size_t)m;
#pragma unroll
      for (int e = 0; e < VN; ++e) v[e] = epi_scale_bias(v[e], alpha, bias_v[e]);
      if (EPI == UVC_EPI_BIAS_GELU_OUT) {
#pragma unroll
        for (int e = 0; e < VN; ++e) v[e] = Gelu<T>::f(v[e]);
      }
      if (EPI == UVC_EPI_BIAS_RESID || EPI == UVC_EPI_BIAS_RESID_GATE) {
        const TC* rp = reinterpret_cast<const TC*>(g.R) + mo * g.ldr + n;
        float rv[VN];
        if (nfull && (g.ldr % VN) == 0) { if constexpr (PRE) Resid<TC>::get(pre->r[it], rv); else load_vec<TC, VN>(rp, rv); }
        else {
#pragma unroll
          for (int e = 0; e < VN; ++e) rv[e] = (n + e < g.N) ? ElemIO<TC>::load(rp + e) : 0.f;
        }
#pragma unroll
        for (int e = 0; e < VN; ++e) v[e] += rv[e];
      }
      if (EPI == UVC_EPI_BIAS_RESID_GATE) {
        const TC* rp = reinterpret_cast<const TC*>(g.R2) + mo * g.ldr + n;
        float rv[VN];
        if (nfull && (g.ldr % VN) == 0) { if constexpr (PRE) Resid<TC>::get(pre->r2[it], rv); else load_vec<TC, VN>(rp, rv); }
        else {
#pragma unroll
          for (int e = 0; e < VN; ++e) rv[e] = (n + e < g.N) ? ElemIO<TC>::load(rp + e) : 0.f;
        }
#pragma unroll
        for (int e = 0; e < VN; ++e) v[e] = epi_gate_mix(v[e], rv[e], d0, d1);
      }
      if (EPI == UVC_EPI_DGELU || EPI == UVC_EPI_MUL_AUX) {
        const T* ap = reinterpret_cast<const T*>(g.aux) + mo * g.ldaux + n;
        float av[VN];
        if (nfull && (g.ldaux % VN) == 0) { if constexpr (PRE) Resid<TC>::get(pre->ax[it], av); else load_vec<T, VN>(ap, av); }
        else {
#pragma unroll
          for (int e = 0; e < VN; ++e) av[e] = (n + e < g.N) ? ElemIO<T>::load(ap + e) : 0.f;
        }
#pragma unroll
        for (int e = 0; e < VN; ++e) v[e] *= (EPI == UVC_EPI_MUL_AUX) ? av[e] : Gelu<T>::g(av[e]);
      }
      float u[VN];
      if (EPI == UVC_EPI_BIAS_GELU_GRAD) {
#pragma unroll
        for (int e = 0; e < VN; ++e) { float fo, go; Gelu<T>::fg(v[e], fo, go); u[e] = fo; v[e] = go; }
      }
      TC* cp = C + mo * g.ldc + n;
      // (GELU' / GELU of the training forward: streaming outputs, non-temporal -- DeiT-Base 23.31 -> 23.06 ms, profiles/r5zz_ab_nt_wide.txt)
      if constexpr (EPI == UVC_EPI_BIAS_GELU_GRAD && sizeof(TC) == 2) { if (nfull) OutVec<TC>::st_nt(cp, v); }
      else
      if (nfull) OutVec<TC>::st(cp, v);
      if (nfull) {}
      else {
#pragma unroll
        for (int e = 0; e < VN; ++e) if (n + e < g.N) ElemIO<TC>::store(cp + e, v[e]);
      }
      if (EPI == UVC_EPI_BIAS_GELU || EPI == UVC_EPI_BIAS_GELU_GRAD) {
        TC* c2 = reinterpret_cast<TC*>(g.C2) + mo * g.ldc + n;
        if (EPI == UVC_EPI_BIAS_GELU) {
#pragma unroll
          for (int e = 0; e < VN; ++e) u[e] = Gelu<T>::f(v[e]);
        }
        if constexpr (EPI == UVC_EPI_BIAS_GELU_GRAD && sizeof(TC) == 2) { if (nfull) OutVec<TC>::st_nt(c2, u); }
        else
        if (nfull) OutVec<TC>::st(c2, u);
        if (nfull) {}
        else {
#pragma unroll
          for (int e = 0; e < VN; ++e) if (n + e < g.N) ElemIO<TC>::store(c2 + e, u[e]);
        }
      }
    }
  }
}

// ---- LDS accesses and waits of the LDS-DMA kernels (the rings of gemm_nt_wsn.hip / gemm_nt_lnbwd.hip, the wide tiles of gemm_nt_wide.hip, gemm_tn.hip).
//      Inline assembly: for an LDS read it can see, hipcc drains s_waitcnt vmcnt(0) behind an LDS-DMA, which would serialise the stages in flight; the
//      waits are spelled out by the kernels (k_gemm_wsn_lnbwd_dma's comment has the whole argument).
__device__ __forceinline__ unsigned lds_addr(const void* p) { return (unsigned)(size_t)(LDS_PTR(char))(char*)p; }
template <int OFF> __device__ __forceinline__ u32x4 ds_read128(unsigned addr) {
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}
__device__ __forceinline__ void ds_write64_a(unsigned addr, f32x2 v) { asm volatile("ds_write_b64 %0, %1" ::"v"(addr), "v"(v) : "memory"); }
template <int N> __device__ __forceinline__ void wait_lgkm() { asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory"); }
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// ---- arguments of the dgrad kernels that end in the LayerNorm backward (uvc_gemm_nt_lnbwd): k_gemm_wsn_lnbwd / _dma (gemm_nt_lnbwd.hip, D = 192) and
//      k_gemm_row384_lnbwd (gemm_nt_wide.hip, D = 384; its forward MODE reads A, W, M, K only)
struct LnbArgs {
  const void* A; const void* W; const void* x; const float* mean; const float* rstd; const float* gamma;
  const void* add1; const float* a1; const void* add2; const float* a2; void* dx; float* partial;
  int M, K, want_dots;
};

// ---- tile sizes the routing of uvc_gemm_nt (gemm.hip) reads, each with the file that owns the kernel
// the row-panel kernel's largest problem (gemm_nt_tiled.hip), read by uvc_gemm_nt_rows_supported (gemm.hip)
constexpr int RP_MAX_M = 1024, RP_MAX_K = 1024;
// k_gemm_nt256's tile (gemm_nt_wide.hip), read by nt256_ok
constexpr int G2_BM = 256, G2_BN = 256, G2_BK = 64;
// k_gemm_row384_lnbwd's tile (gemm_nt_wide.hip): R3_BN is the one width it is built for, read by row384_fwd_ok
constexpr int R3_BM = 128, R3_BN = 384, R3_BK = 64;

// ---- launchers: grid, LDS bytes, launch.  NT_LAUNCH(epi, cases): the launch of the case that is `epi` (nt_route has checked that the family takes it)
#define NT_LAUNCH(epi, ...) \
  switch (epi) { __VA_ARGS__ default: return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_nt: epilogue not built for the routed kernel"); } \
  UVC_CHECK_LAUNCH(); \
  return UVC_OK;
#define NT_EPI9(X) X(UVC_EPI_NONE) X(UVC_EPI_BIAS) X(UVC_EPI_BIAS_GELU) X(UVC_EPI_BIAS_RESID) X(UVC_EPI_BIAS_RESID_GATE) X(UVC_EPI_DGELU) X(UVC_EPI_BIAS_GELU_OUT) \
                   X(UVC_EPI_BIAS_GELU_GRAD) X(UVC_EPI_MUL_AUX)
// the launcher instance of the route's operand types (`r` is the uvc_gemm_route in scope)
#define NT_BY_TC(F, ...) (r.c_f32 ? F<float>(__VA_ARGS__) : F<bf16_t>(__VA_ARGS__))
#define NT_BY_TA_TC(F, ...) (r.a_f32 ? (r.c_f32 ? F<float, float>(__VA_ARGS__) : F<float, bf16_t>(__VA_ARGS__)) \
                                     : (r.c_f32 ? F<bf16_t, float>(__VA_ARGS__) : F<bf16_t, bf16_t>(__VA_ARGS__)))

// ---- the launchers of the kernel families, defined next to their kernels: each picks the instance of the route's operand types, computes grid and
//      LDS bytes, launches.  Internal to the library (hidden); uvc_gemm_nt (gemm.hip) is their only caller, but for launch_row384_lnbwd, which
//      uvc_gemm_nt_lnbwd (gemm_nt_lnbwd.hip) calls at D = 384.
namespace uvc_gemm __attribute__((visibility("hidden"))) {
int launch_nt(const uvc_gemm_route& r, const NtArgs& a, hipStream_t st);            // gemm_nt_tiled.hip
int launch_nt_rows(const uvc_gemm_route& r, const NtArgs& a, hipStream_t st);
int launch_ws(const uvc_gemm_route& r, const NtArgs& a, hipStream_t st);            // gemm_nt_ws.hip
int launch_ws384(const uvc_gemm_route& r, const NtArgs& a, hipStream_t st);
int launch_wsn(const uvc_gemm_route& r, const NtArgs& a, hipStream_t st);           // gemm_nt_wsn.hip
int launch_ring(const uvc_gemm_route& r, const NtArgs& a, hipStream_t st);
int launch_row384_fwd(const NtArgs& a, int epi, hipStream_t st);                    // gemm_nt_wide.hip
int launch_row384_lnbwd(const LnbArgs& a, int x_lowp, hipStream_t st);
int launch_nt256(const uvc_gemm_route& r, const NtArgs& a, hipStream_t st);
int launch_nt8p(const uvc_gemm_route& r, const NtArgs& a, hipStream_t st);
}  // namespace uvc_gemm
