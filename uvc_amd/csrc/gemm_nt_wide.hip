// The three 8-wave NT kernels on wide LDS-DMA tiles (bf16): the GEMMs of DeiT-Small / Base and T2T-ViT.
//   k_gemm_nt256<TC, EPI>                  256 x 256 tiles, waves in lock step                          UVC_ROUTE_NT256
//   k_gemm_row384_lnbwd<XLOW, MODE>        128 x 384 row tiles: MODE 0 dgrad + LayerNorm backward       uvc_gemm_nt_lnbwd at D = 384
//                                          MODE 1 fc2 / attn.proj + residual + LayerNorm forward        UVC_ROUTE_ROW384
//   k_gemm_nt8p<TC, EPI, RI>               (32 RI) x 256 tiles, two wave groups half a phase apart      UVC_ROUTE_NT8P
// One file because they share g2_tile, the G2_EPI transpose buffers, NT_EPILOGUE_TILE and the pinned 8-wave step; NT_EPILOGUE_TILE, G2Frags and
// the R8_* / P8_* macros are private to it.
#include "gemm_common.h"

// ---- used by this file only (the shared LDS accesses are in gemm_common.h): the 16-byte read whose offset is a function argument, a constant once
//      inlined (ds_read128<OFF> takes it as a template argument: two signatures, kept as two); the 8-byte read; Raw4L
__device__ __forceinline__ u32x4 ds_read128_asm(unsigned addr, int off) {
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(off));
  return v;
}
__device__ __forceinline__ u32x2 ds_read64_a(unsigned addr) { u32x2 v; asm volatile("ds_read_b64 %0, %1" : "=v"(v) : "v"(addr)); return v; }
// four elements as they sit in memory (no conversion)
template <typename T> struct Raw4L;
template <> struct Raw4L<float> {
  typedef f32x4 V;
  static __device__ __forceinline__ V ld(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
  static __device__ __forceinline__ V zero() { return f32x4{0.f, 0.f, 0.f, 0.f}; }
  static __device__ __forceinline__ f32x4 cvt(const V& r) { return r; }
};
template <> struct Raw4L<bf16_t> {
  typedef u32x2 V;
  static __device__ __forceinline__ V ld(const bf16_t* p) { return *reinterpret_cast<const u32x2*>(p); }
  static __device__ __forceinline__ V zero() { return u32x2{0u, 0u}; }
  static __device__ __forceinline__ f32x4 cvt(const V& r) {
    return f32x4{__uint_as_float(r[0] << 16), __uint_as_float(r[0] & 0xffff0000u), __uint_as_float(r[1] << 16), __uint_as_float(r[1] & 0xffff0000u)};
  }
};

// ================================================================================================
//            NT, 256 x 256 output tile, LDS-DMA double buffer (bf16; the wide models' GEMMs)
// ================================================================================================
// DeiT-Small / Base and T2T-ViT have K = 384 ... 3072 against N = 384 ... 3072: compute-bound on the matrix pipe, not streaming
// (2 M N K / (2 (M K + N K + M N)) = 300 ... 600 flop / B), and the 128 x 128 kernel above spends its time around its two barriers
// per 64-deep step (0.5-0.85 PFLOP/s).  Here a workgroup is 8 waves (2 x 4), one per CU by LDS, and owns a 256 x 256 tile: a wave
// accumulates 128 x 64 (32 MFMA tiles, 128 accumulator registers), so a 16-byte fragment read feeds four (A) or eight (B) MFMAs.
//   * Operand tiles (256 rows x 64 k = 32 KB each) go HBM / L2 -> LDS by LDS-DMA (buffer_load_dwordx4 ... lds: no staging registers,
//     rows past M / N read as zeros through the buffer descriptor's bounds check) into TWO 64-KB stages; the DMA writes a wave's 64
//     lanes as 64 consecutive 16-byte slots, so the image is linear [row][8 chunks] and the bank swizzle sits in the SOURCE address:
//     slot (row, c) holds k-chunk c ^ (row & 7), which makes the fragment reads (row = lane & 15, chunk = 4 ks + lane / 16) of every
//     ds_read_b128 lane group hit 16 different 16-byte slots of the 256-byte bank row.
//   * One barrier per 64-deep step.  Fragments of k-half 1 are requested before the MFMAs of k-half 0 and those of the NEXT stage's
//     k-half 0 before the MFMAs of k-half 1 (two fragment sets, 96 registers), and the stage after next is requested right behind the
//     barrier, a whole step before it is needed:   [read F1 | 32 MFMA F0 | wait F1, wait DMA(t+1) | barrier | DMA(t+2) | read F0' | 32 MFMA F1].
//     All LDS reads of the loop are inline assembly: behind an LDS-DMA hipcc drains vmcnt(0) in front of any LDS read it can see.
//   * The 8 DMA instructions of a stage are issued between the rows of the second MFMA block (one per four MFMAs): issued in a burst
//     behind the barrier they kept the matrix pipe idle for ~800 cycles per step (every wave of the lock-stepped workgroup at once).
//   * Epilogue through a wave-private LDS transpose, nt_epilogue_rows: the same arithmetic and stores as k_gemm_nt.
//   * One PERSISTENT workgroup per CU walks its tiles (numbered XCD-major: block b runs on XCD b % 8, so all N tiles of an M tile
//     share an L2); the first two k-steps of the next tile are requested during the last two steps of the current one, so only the
//     first tile of a workgroup pays the operand latency and the epilogue is the only gap between tiles.
// Epilogue of a wave's NH x 16 accumulator rows (acc[h][0..3], rows MROW0 + 16 h .., columns NCOL0 .. + 63) through its swizzled 4-KB transpose
// buffer `stg`, 16 rows at a time; with a bf16 C the operand rows (R / R2 / aux) of step h + PD are requested when step h is done (PD steps in
// flight; PD1 with one operand, PD2 with two: 8 registers per operand and step).  Same arithmetic and stores as every other user of nt_epilogue_rows: same bits.
#define NT_EPILOGUE_TILE(NH, MROW0, NCOL0, PD1, PD2)                                                                                 \
  {                                                                                                                           \
    constexpr bool PRE_ = sizeof(TC) == 2 && EpiOperands<EPI>::COUNT > 0;                                                     \
    constexpr int PD_ = EpiOperands<EPI>::COUNT >= 2 ? (PD2) : (PD1);                                                              \
    EpiPre<2> pre_[PD_];                                                                                                      \
    if constexpr (PRE_) {                                                                                                     \
      _Pragma("unroll") for (int h = 0; h < PD_ && h < (NH); ++h) nt_epilogue_prefetch<EPI, 16>(g, lane, (MROW0) + h * 16, (NCOL0), pre_[h]); \
    }                                                                                                                         \
    _Pragma("unroll") for (int h = 0; h < (NH); ++h) {                                                                        \
      _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                                           \
        *reinterpret_cast<f32x4*>(stg_at<true>(stg, lane & 15, j * 4 + (lane >> 4))) = acc[h][j];                            \
      __builtin_amdgcn_wave_barrier();                                                                                        \
      nt_epilogue_rows<T, TC, EPI, 16, true, PRE_>(g, stg, lane, (MROW0) + h * 16, (NCOL0), alpha, d0, d1, bias_v, &pre_[h % PD_]); \
      if constexpr (PRE_) { if (h + PD_ < (NH)) nt_epilogue_prefetch<EPI, 16>(g, lane, (MROW0) + (h + PD_) * 16, (NCOL0), pre_[h % PD_]); } \
      __builtin_amdgcn_wave_barrier();                                                                                        \
    }                                                                                                                         \
  }

constexpr int G2_OPB = 256 * 128;              // bytes of one operand tile image (256 rows x 128 B)
constexpr int G2_STAGE = 2 * G2_OPB;           // A image + B image
constexpr int G2_EPI = 8 * 16 * 64 * 4;        // epilogue transpose buffers: 8 waves x 16 rows x 64 floats (swizzled, unpadded)
constexpr int G2_LDS = 2 * G2_STAGE + G2_EPI;  // 160 KB: the whole CU

struct G2Frags { u32x4 a[8]; u32x4 b[4]; };

// tile number (XCD-major order: block b runs on XCD b % 8, so the tiles v, v + 8, ... share an L2) -> tile coordinates
__device__ __forceinline__ bool g2_tile(int v, int tiles_m, int tiles_n, int& bm, int& bn) {
  const int xcd = v & 7, q = v >> 3;
  bn = q % tiles_n; bm = (q / tiles_n) * 8 + xcd;
  return bm < tiles_m;
}

template <typename TC, int EPI>
__global__ __launch_bounds__(512, 2) void k_gemm_nt256(NtArgs g, int tiles_m, int tiles_n, int nvirt) {
  typedef bf16_t T;
  typedef Mma<T> MM;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 2, wn = w & 3;

  // ---- LDS-DMA: 32 wave-instructions per operand tile (8 rows x 128 B each), wave w issues instructions w, w + 8, w + 16, w + 24
  const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g.A), 0, (int)(((size_t)(g.M - 1) * g.lda + g.K) * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g.B), 0, (int)(((size_t)(g.N - 1) * g.ldb + g.K) * 2), 0x00020000);
  const int lrow = lane >> 3, lchunk = (lane & 7) ^ lrow;         // slot (row, c) <- k-chunk c ^ (row & 7)
  const unsigned laneA = (unsigned)(((w * 8 + lrow) * g.lda + lchunk * 8) * 2), laneB = (unsigned)(((w * 8 + lrow) * g.ldb + lchunk * 8) * 2);
  const unsigned stepA = (unsigned)(64 * g.lda * 2), stepB = (unsigned)(64 * g.ldb * 2);
  // one of the 8 DMA instructions of a stage (t = 0..3: A rows 64 t .., 4..7: B rows): tile origin (voA, voB), k-step kt, stage st
  // (voA / voB are wave-uniform byte offsets of the tile's first row: kept in SGPRs and added to the lane's offset per instruction --
  //  the bounds check of a raw buffer covers the VGPR offset only, so the whole offset goes there)
  auto issue1 = [&](int t, unsigned voA, unsigned voB, int kt, int st) {
    char* base = smem + st * G2_STAGE + w * 1024;
    const unsigned kb = (unsigned)(kt * G2_BK * 2);
    if (t < 4) __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (__attribute__((address_space(3))) void*)(base + t * 8192), 16, laneA + (voA + kb + t * stepA), 0, 0, 0);
    else __builtin_amdgcn_raw_ptr_buffer_load_lds(rB, (__attribute__((address_space(3))) void*)(base + G2_OPB + (t - 4) * 8192), 16, laneB + (voB + kb + (t - 4) * stepB), 0, 0, 0);
  };
  // ---- fragment addresses: row = lane & 15 (+ the tile's offset), k-chunk 4 ks + lane / 16, swizzled with row & 7 = lane & 7
  const unsigned s0 = lds_addr(smem);
  const unsigned sw0 = (unsigned)((((lane >> 4)) ^ (lane & 7)) * 16);
  const unsigned fa0 = s0 + (unsigned)((wm * 128 + (lane & 15)) * 128) + sw0;                    // k-half 0; k-half 1 = address ^ 64
  const unsigned fb0 = s0 + (unsigned)(G2_OPB + (wn * 64 + (lane & 15)) * 128) + sw0;
  auto rdfrags = [&](G2Frags& F, int st, int ks) {
    const unsigned a = (fa0 ^ (unsigned)(ks * 64)) + (unsigned)(st * G2_STAGE), b = (fb0 ^ (unsigned)(ks * 64)) + (unsigned)(st * G2_STAGE);
    F.b[0] = ds_read128<0 * 2048>(b); F.b[1] = ds_read128<1 * 2048>(b); F.b[2] = ds_read128<2 * 2048>(b); F.b[3] = ds_read128<3 * 2048>(b);
    F.a[0] = ds_read128<0 * 2048>(a); F.a[1] = ds_read128<1 * 2048>(a); F.a[2] = ds_read128<2 * 2048>(a); F.a[3] = ds_read128<3 * 2048>(a);
    F.a[4] = ds_read128<4 * 2048>(a); F.a[5] = ds_read128<5 * 2048>(a); F.a[6] = ds_read128<6 * 2048>(a); F.a[7] = ds_read128<7 * 2048>(a);
  };
  auto tie = [&](G2Frags& F) {
    asm volatile("" : "+v"(F.a[0]), "+v"(F.a[1]), "+v"(F.a[2]), "+v"(F.a[3]), "+v"(F.a[4]), "+v"(F.a[5]), "+v"(F.a[6]), "+v"(F.a[7]),
                      "+v"(F.b[0]), "+v"(F.b[1]), "+v"(F.b[2]), "+v"(F.b[3]));
  };
  f32x4 acc[8][4];
  auto mfma_row = [&](const G2Frags& F, int i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = MM::mma(__builtin_bit_cast(typename MM::Frag, F.b[j]), __builtin_bit_cast(typename MM::Frag, F.a[i]), acc[i][j]);
  };
  float alpha = g.alpha;
  if (g.alpha_ptr) alpha *= *g.alpha_ptr;
  float d0 = 0.f, d1 = 1.f;
  if (EPI == UVC_EPI_BIAS_RESID_GATE) { d0 = g.dptr[0]; d1 = g.dptr[1]; }
  float* const stg = reinterpret_cast<float*>(smem + 2 * G2_STAGE) + w * (16 * 64);

  // ---- persistent walk over this workgroup's tiles: the k-steps of consecutive tiles form ONE stream through the two stages -- the
  //      first two k-steps of the NEXT tile are requested in the last two iterations of the current one, so a tile's operand latency
  //      and the previous tile's epilogue overlap
  const int nk = g.K / G2_BK;                     // >= 4 (the dispatch requires K >= 256)
  int v = blockIdx.x, bm = 0, bn = 0;
  while (v < nvirt && !g2_tile(v, tiles_m, tiles_n, bm, bn)) v += gridDim.x;
  if (v >= nvirt) return;
  unsigned voA = (unsigned)(bm * G2_BM * g.lda * 2), voB = (unsigned)(bn * G2_BN * g.ldb * 2);
  int par = 0;                                    // stage of the current tile's k-step 0
#pragma unroll
  for (int t = 0; t < 8; ++t) issue1(t, voA, voB, 0, 0);
#pragma unroll
  for (int t = 0; t < 8; ++t) issue1(t, voA, voB, 1, 1);
  wait_vm<8>();                                   // own part of the first stage has landed (loads retire in order; 8 per stage and wave)
  __builtin_amdgcn_s_barrier();
  G2Frags F0, F1;
  rdfrags(F0, 0, 0);
  wait_lgkm<0>();
  tie(F0);
  for (;;) {
    // the tile after this one (its first k-steps are requested while this one finishes)
    int vn = v + gridDim.x, bmn = 0, bnn = 0;
    while (vn < nvirt && !g2_tile(vn, tiles_m, tiles_n, bmn, bnn)) vn += gridDim.x;
    const bool more = vn < nvirt;
    const unsigned voAn = more ? (unsigned)(bmn * G2_BM * g.lda * 2) : voA, voBn = more ? (unsigned)(bnn * G2_BN * g.ldb * 2) : voB;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < nk; ++kt) {
      const int st = (kt & 1) ^ par;
      // The order of the step is pinned (scheduling fences): left to itself hipcc sinks two thirds of the first MFMA block below the
      // barrier, which exposes the fragment reads' latency in front of it and leaves the matrix pipe idle around it (s_memtime trace:
      // 2950 cycles per step for 1024 cycles of MFMA issue per SIMD).  A wave never waits with nothing queued behind it: the reads of a
      // block are requested a block ahead, the barrier sits between two MFMA blocks, and the first instructions behind it are MFMAs.
      rdfrags(F1, st, 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 8; ++i) mfma_row(F0, i);
      __builtin_amdgcn_sched_barrier(0);
      wait_lgkm<0>();                             // F1 is in registers (requested 32 MFMAs ago): this wave is done with stage st
      tie(F1);
      wait_vm<0>();                               // own part of the next k-step's stage has landed (requested a step ago)
      __builtin_amdgcn_s_barrier();               // everybody's has; nobody reads stage st any more
      __builtin_amdgcn_sched_barrier(0);
      // the stage freed now receives k-step kt + 2 of this tile, or k-step kt + 2 - nk of the next one (all scalar selects;
      // behind the workgroup's last tile the same instructions re-load k-steps 0 / 1 of that tile: no branch around a DMA)
      const bool tail = kt + 2 >= nk;
      const unsigned sA = tail ? voAn : voA, sB = tail ? voBn : voB;
      const int kk = tail ? kt + 2 - nk : kt + 2;
      mfma_row(F1, 0);
      __builtin_amdgcn_sched_barrier(0);
      rdfrags(F0, st ^ 1, 0);
      __builtin_amdgcn_sched_barrier(0);
      // the 8 DMA instructions of that stage go BETWEEN the MFMA rows: their issue cost (~100 cycles each) hides under the matrix pipe
#pragma unroll
      for (int i = 1; i < 8; ++i) {
        issue1(i - 1, sA, sB, kk, st);
        if (i == 7) issue1(7, sA, sB, kk, st);
        __builtin_amdgcn_sched_barrier(0);
        mfma_row(F1, i);
        __builtin_amdgcn_sched_barrier(0);
      }
      wait_lgkm<0>();
      tie(F0);
    }
    // ---- epilogue: 16 rows x 64 columns at a time through this wave's private transpose buffer (behind the stages: the next tile's
    //      operands keep arriving meanwhile).  Measured against an epilogue straight from the accumulator layout (v_permlane16_swap
    //      pairs, 16-byte stores in 64-byte row pieces, operands read in 32-byte pieces): equal with no operands, 10-15 % of the GEMM
    //      slower with a bias / residual / multiplier to read -- whole 128-byte row segments matter more than the LDS round trips
    {
      const int m0 = bm * G2_BM, n0 = bn * G2_BN;
      float bias_v[OutVec<TC>::VN];
      nt_load_bias<TC, EPI>(g, lane, n0 + wn * 64, bias_v);
      NT_EPILOGUE_TILE(8, m0 + wm * 128, n0 + wn * 64, 2, 1)      // (256 registers: two fragment sets are live across the epilogue)
    }
    if (!more) break;
    v = vn; bm = bmn; bn = bnn; voA = voAn; voB = voBn;
    par ^= nk & 1;
  }
  wait_vm<0>();                                   // the two redundant stages behind the last tile
}

// ================================================================================================
// D = 384 (DeiT-Small, T2T-ViT-14): the dgrad of fc1 / qkv with the LayerNorm BACKWARD as its epilogue, on a ROW TILE.
//     dx = LN'(A . W^T; x, mean, rstd, gamma) + a1 * add1 + a2 * add2        (uvc_gemm_nt_lnbwd; model_distilled.py:199-204,218-247)
// The weights (384 x 1152 / 1536) do not fit the register files the D = 192 kernels keep them in, so this is k_gemm_nt256's main loop
// on a 128 x 384 tile -- whole rows of dx per workgroup: 8 waves as 2 x 4, a wave accumulates 64 x 96 (4 A- and 6 B-fragments per
// k-half, 96 accumulator registers), the same two 64-KB stages (16 KB of A, 48 KB of W per k-step: 2 + 6 DMA instructions per wave)
// and the same pinned step.  Behind the last k-step the tile is rounded to bf16 -- exactly what the unfused pair stores between the
// GEMM and the LayerNorm pass -- into the (now free) stages as 128 rows of 776 bytes, and the eight waves run k_ln_bwd_v's row
// arithmetic over it with that kernel's lane mapping (32 lanes x 12 columns, two rows at a time, three row sets of x / add1 / add2 in
// flight): dx is BIT-IDENTICAL to k_gemm_nt + k_ln_bwd_v (tests/test_kernels_gpu.py); dgamma / dbeta / dots leave as one partial row
// per workgroup for the batched LayerNorm reduce (256 rows: workgroups without a tile write zeros).
constexpr int R3_OPA = R3_BM * 128, R3_OPB = R3_BN * 128;   // operand images of a k-step: 16 KB + 48 KB
constexpr int R3_STAGE = R3_OPA + R3_OPB;
constexpr int R3_RS = R3_BN * 2 + 8;                        // row stride of the bf16 result tile: 16 rows = 16 different 8-byte bank slots
constexpr int R3_LDS = 2 * R3_STAGE + 8 * (2 * R3_BN + 2) * 4;   // stages (the result tile lives in them) + the waves' partial rows
static_assert(R3_BM * R3_RS <= 2 * R3_STAGE, "the result tile fits the stages");

struct R3Frags { u32x4 a[4]; u32x4 b[6]; };
// MODE 1 (r4): the FORWARD counterpart on the same main loop -- fc2 / attn.proj (K -> 384) + bias + residual (+ gate mix) with the LayerNorm of the
// output rows as a second output (uvc_gemm_nt with ln_out at N = 384: the next block's norm1 / this block's norm2, two stand-alone passes per block
// before).  Behind the k-loop the float32 tile goes to LDS one 64-row half at a time (rows of 1568 bytes), and the eight waves run the epilogue of
// nt_epilogue_rows and then k_ln_fwd_v<bf16, bf16, 6>'s arithmetic over whole rows with that kernel's lane map (16 lanes x 24 columns, four rows
// at a time): C, the LayerNorm rows and the statistics are BIT-IDENTICAL to k_gemm_nt + k_ln_fwd_v, so whether a batch takes the fused form does
// not show in its results (tests/test_kernels_gpu.py; the engine's batch-independence tests).
struct R3Fwd {
  const float* bias; const void* R; const void* R2; const float* dptr; void* C;
  const float* ln_gamma; const float* ln_beta; void* ln_out; float* ln_mean; float* ln_rstd; float ln_eps; int gate;
};
constexpr int R3_FS = R3_BN * 4 + 32;                        // float32 half-tile row: 392 words = 8 mod 64 (conflict-free 16-byte writes by (row, 4-column group))
static_assert(64 * R3_FS <= 2 * R3_STAGE, "a float32 half tile fits the stages");

template <bool XLOW, int MODE = 0>
__global__ __launch_bounds__(512, 2) void k_gemm_row384_lnbwd(LnbArgs g, int tiles_m, R3Fwd f) {
  typedef bf16_t T;
  typedef Mma<T> MM;
  constexpr int D = R3_BN, NV4 = 3, LPR = 32;
  typedef typename std::conditional<XLOW, bf16_t, float>::type TX;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 2, wn = w & 3;
  const int sub = lane & (LPR - 1), rg = lane / LPR;

  // ---- main loop: k_gemm_nt8p's schedule (two wave groups half a phase apart, the fragments of a phase requested inside the MFMA block of the
  //      phase before, four LDS slots per k-step read in phases 0, 0, 1, 2) on the 128 x 384 tile: a wave's 64 x 96 block is the quadrants
  //      A0 / A1 = row blocks 0-1 / 2-3, B0 / B1 = column blocks 0-2 / 3-5 (12 MFMAs a phase).  Slots of a k-step: A'0 (64 rows: the A0 rows of
  //      both M groups, 8 KB), B'0 (192 rows of W: the B0 columns of the four N groups, 24 KB), B'1, A'1 = 64 KB, two buffers (the result tile
  //      and the row pass reuse them behind the loop).  A wave issues 1 / 3 / 3 / 1 DMA instructions for them; waits counted accordingly.
  const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g.A), 0, (int)(((size_t)(g.M - 1) * g.K + g.K) * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g.W), 0, (int)((size_t)R3_BN * g.K * 2), 0x00020000);
  constexpr int SZA = 64 * 128, SZB = 192 * 128, OFF_A0 = 0, OFF_B0 = SZA, OFF_B1 = SZA + SZB, OFF_A1 = SZA + 2 * SZB;
  static_assert(2 * SZA + 2 * SZB == R3_STAGE, "a k-step's four slots fill a stage");
  const int lrow = lane >> 3, lchunk = (lane & 7) ^ lrow;         // slot (row, c) <- k-chunk c ^ (row & 7)
  unsigned laneA[2], laneB[2][3];
  {
    const int ra = w * 8 + lrow;                                  // image row of an A slot: M group ra >> 5, row ra & 31 of its 32
#pragma unroll
    for (int h = 0; h < 2; ++h) laneA[h] = (unsigned)((((ra >> 5) * 64 + h * 32 + (ra & 31)) * g.K + lchunk * 8) * 2);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int rb = (w + 8 * q) * 8 + lrow;                      // image row of a W slot: N group rb / 48, column rb % 48 of its 48
#pragma unroll
      for (int h = 0; h < 2; ++h) laneB[h][q] = (unsigned)((((rb / 48) * 96 + h * 48 + rb % 48) * g.K + lchunk * 8) * 2);
    }
  }
  // request item IT (0 = A'0, 1 = B'0, 2 = B'1, 3 = A'1) of the k-step at byte offset kb of the rows, into buffer buf
  auto issue_item = [&](int it, unsigned voA, unsigned kb, int buf) {
    char* base = smem + buf * R3_STAGE + w * 1024;
    if (it == 0) __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (__attribute__((address_space(3))) void*)(base + OFF_A0), 16, laneA[0] + (voA + kb), 0, 0, 0);
    else if (it == 3) __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (__attribute__((address_space(3))) void*)(base + OFF_A1), 16, laneA[1] + (voA + kb), 0, 0, 0);
    else {
      const int h = it - 1;
#pragma unroll
      for (int q = 0; q < 3; ++q)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rB, (__attribute__((address_space(3))) void*)(base + (h ? OFF_B1 : OFF_B0) + q * 8192), 16, laneB[h][q] + kb, 0, 0, 0);
    }
  };
  const unsigned s0 = lds_addr(smem);
  const unsigned sw0 = (unsigned)((((lane >> 4)) ^ (lane & 7)) * 16);
  const unsigned fa0 = s0 + (unsigned)((wm * 32 + (lane & 15)) * 128) + sw0;       // inside an A slot; k-half 1 = address ^ 64
  const unsigned fb0 = s0 + (unsigned)((wn * 48 + (lane & 15)) * 128) + sw0;       // inside a W slot
  u32x4 FA[2][2], FB0[3][2], FB1[3][2];
  f32x4 acc[4][6];
#define R8_RD_B(DST, OFF, BO)                                                                                         \
  _Pragma("unroll") for (int j = 0; j < 3; ++j) {                                                                      \
    DST[j][0] = ds_read128_asm(fb0 + (BO), (OFF) + j * 2048); DST[j][1] = ds_read128_asm((fb0 ^ 64u) + (BO), (OFF) + j * 2048); }
#define R8_RD_A(I, OFF, BO) { FA[I][0] = ds_read128_asm(fa0 + (BO), (OFF) + (I) * 2048); FA[I][1] = ds_read128_asm((fa0 ^ 64u) + (BO), (OFF) + (I) * 2048); }
#define R8_MMA6(I, AI, FB, JO)                                                                                        \
  _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                                     \
  _Pragma("unroll") for (int j = 0; j < 3; ++j)                                                                        \
    acc[AI][(JO) + j] = MM::mma(__builtin_bit_cast(typename MM::Frag, FB[j][ks]), __builtin_bit_cast(typename MM::Frag, FA[I][ks]), acc[AI][(JO) + j]);
#define R8_REQ(IT, KB, SBUF, NWAIT)                                                                                   \
  issue_item(IT, voA, KB, SBUF);                                                                                       \
  if ((NWAIT) >= 0) wait_vm<((NWAIT) < 0 ? 0 : (NWAIT))>();                                                            \
  __builtin_amdgcn_s_barrier();                                                                                        \
  wait_lgkm<0>();                                                                                                      \
  __builtin_amdgcn_sched_barrier(0);                                                                                   \
  __builtin_amdgcn_s_setprio(1);
#define R8_END                                                                                                        \
  __builtin_amdgcn_s_setprio(0);                                                                                       \
  __builtin_amdgcn_sched_barrier(0);                                                                                   \
  __builtin_amdgcn_s_barrier();                                                                                        \
  __builtin_amdgcn_sched_barrier(0);

  // ---- LayerNorm backward state of this lane: columns (sub + 32 i) * 4 .. + 3, i = 0..2 (k_ln_bwd_v<.., 3, 32>'s map)
  f32x4 gam[NV4], dgam[NV4], dbet[NV4];
#pragma unroll
  for (int i = 0; i < NV4; ++i) {
    gam[i] = MODE == 0 ? *reinterpret_cast<const f32x4*>(g.gamma + (sub + LPR * i) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    dgam[i] = f32x4{0.f, 0.f, 0.f, 0.f}; dbet[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float a1 = g.a1 ? *g.a1 : 1.f, a2 = g.a2 ? *g.a2 : 1.f;
  float dotA = 0.f, dotB = 0.f;
  const float invD = 1.0f / (float)D;
  const bf16_t* add1 = reinterpret_cast<const bf16_t*>(g.add1);
  const bf16_t* add2 = reinterpret_cast<const bf16_t*>(g.add2);
  struct RawRow { typename Raw4L<TX>::V xv[NV4]; u32x2 ad1[NV4], ad2[NV4]; float mean, rstd; int r; bool ok; };

  const int nk = g.K / R3_BK;
  for (int bm = blockIdx.x; bm < tiles_m; bm += gridDim.x) {
    const unsigned voA = (unsigned)(bm * R3_BM * g.K * 2);
    __syncthreads();                                              // the last tile's row pass is done with the stages
    // prologue: k-step 0 whole, A'0 and B'0 of k-step 1
#pragma unroll
    for (int it = 0; it < 4; ++it) issue_item(it, voA, 0u, 0);
    issue_item(0, voA, 128u, 1); issue_item(1, voA, 128u, 1);
    wait_vm<5>();                                                 // A'0, B'0, B'1 of k-step 0 have landed (A'1: 1, A'0 + B'0 of k-step 1: 4 in flight)
    __builtin_amdgcn_s_barrier();
    R8_RD_B(FB0, OFF_B0, 0u)
    R8_RD_A(0, OFF_A0, 0u) R8_RD_A(1, OFF_A0, 0u)
    __builtin_amdgcn_sched_barrier(0);
    if (wm == 1) __builtin_amdgcn_s_barrier();                    // group 1 runs half a phase behind through the k-loop
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < nk; ++kt) {
      const int buf = kt & 1;
      const unsigned bo = (unsigned)(buf * R3_STAGE), bon = bo ^ (unsigned)R3_STAGE;
      // k-steps kt + 1, kt + 2 (behind the last ones: k-steps 0 / 1 of the same tile again -- no branch around a DMA; nobody multiplies them)
      const unsigned kb1 = (unsigned)((kt + 1 < nk ? kt + 1 : kt + 1 - nk) * 128), kb2 = (unsigned)((kt + 2 < nk ? kt + 2 : kt + 2 - nk) * 128);
      // phase 0: (A0, B0); requests B'1 of kt + 1 (3); reads B1.  In flight behind the wait: A'0 + B'0 + B'1 of kt + 1 = 7
      R8_REQ(2, kb1, buf ^ 1, 7)
      R8_RD_B(FB1, OFF_B1, bo)
      __builtin_amdgcn_sched_barrier(0);
      R8_MMA6(0, 0, FB0, 0) R8_MMA6(1, 1, FB0, 0)
      R8_END
      // phase 1: (A0, B1); requests A'1 of kt + 1 (1); reads A1 behind the MFMAs that free A0's registers
      R8_REQ(3, kb1, buf ^ 1, -1)
      R8_MMA6(0, 0, FB1, 3)
      __builtin_amdgcn_sched_barrier(0);
      R8_RD_A(0, OFF_A1, bo)
      __builtin_amdgcn_sched_barrier(0);
      R8_MMA6(1, 1, FB1, 3)
      __builtin_amdgcn_sched_barrier(0);
      R8_RD_A(1, OFF_A1, bo)
      R8_END
      // phase 2: (A1, B1); requests A'0 of kt + 2 (1).  In flight: B'1 + A'1 of kt + 1, A'0 of kt + 2 = 5
      R8_REQ(0, kb2, buf, 5)
      R8_MMA6(0, 2, FB1, 3) R8_MMA6(1, 3, FB1, 3)
      R8_END
      // phase 3: (A1, B0); requests B'0 of kt + 2 (3); reads A0 and B0 of kt + 1.  In flight: A'1 of kt + 1, A'0 + B'0 of kt + 2 = 5
      R8_REQ(1, kb2, buf, 5)
      R8_MMA6(0, 2, FB0, 0)
      __builtin_amdgcn_sched_barrier(0);
      R8_RD_A(0, OFF_A0, bon)
      __builtin_amdgcn_sched_barrier(0);
      R8_MMA6(1, 3, FB0, 0)
      __builtin_amdgcn_sched_barrier(0);
      R8_RD_A(1, OFF_A0, bon)
      R8_RD_B(FB0, OFF_B0, bon)
      R8_END
    }
    if (wm == 0) __builtin_amdgcn_s_barrier();                    // pairs with group 1's last barrier: the groups are level again
    wait_lgkm<0>();
    wait_vm<0>();
    __syncthreads();                                              // every wave is done with the stages and nothing is in flight into them
    if constexpr (MODE == 1) {
      const int sub16 = lane & 15, rg4 = lane >> 4;
      const float invD384 = 1.0f / (float)D;
      const float d0 = f.gate ? f.dptr[0] : 0.f, d1 = f.gate ? f.dptr[1] : 1.f;
      const bf16_t* Rp = reinterpret_cast<const bf16_t*>(f.R);
      const bf16_t* R2p = reinterpret_cast<const bf16_t*>(f.R2);
      for (int half = 0; half < 2; ++half) {
        // rows w * 8 .. + 7 of the half: two sets of four rows (16 lanes a row); both sets' residual rows are requested here, in front of the
        // staging writes and the barrier, so that their HBM round trip runs beside them
        u32x2 rr[2][6], rr2[2][6];
        int rows_[2]; bool ok_[2];
#pragma unroll
        for (int it = 0; it < 2; ++it) {
          rows_[it] = bm * R3_BM + half * 64 + w * 8 + it * 4 + rg4;
          ok_[it] = rows_[it] < g.M;
          const size_t off = (size_t)(ok_[it] ? rows_[it] : 0) * D;
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            rr[it][i] = ok_[it] ? *reinterpret_cast<const u32x2*>(Rp + off + (sub16 + 16 * i) * 4) : u32x2{0u, 0u};
            rr2[it][i] = (ok_[it] && f.gate) ? *reinterpret_cast<const u32x2*>(R2p + off + (sub16 + 16 * i) * 4) : u32x2{0u, 0u};
          }
        }
        if (wm == half) {                                          // this M group's 64 rows, float32, row-major
          const unsigned base = s0 + (unsigned)((lane & 15) * R3_FS + (wn * 96 + (lane >> 4) * 4) * 4);
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j)
              asm volatile("ds_write_b128 %0, %1" ::"v"(base + (unsigned)(i * 16 * R3_FS + j * 64)), "v"(acc[i][j]) : "memory");
        }
        wait_lgkm<0>();
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 2; ++it) {
          const unsigned la = s0 + (unsigned)((w * 8 + it * 4 + rg4) * R3_FS + sub16 * 16);
          f32x4 v[6];
#pragma unroll
          for (int i = 0; i < 6; ++i) v[i] = __builtin_bit_cast(f32x4, ds_read128_asm(la, i * 256));
          wait_lgkm<0>();
          asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]));
          float sm = 0.f;
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(f.bias + (sub16 + 16 * i) * 4);
            const f32x4 rv = Raw4L<bf16_t>::cvt(rr[it][i]), r2v = Raw4L<bf16_t>::cvt(rr2[it][i]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              float t = epi_scale_bias(v[i][e], 1.0f, bv[e]);
              t += rv[e];
              if (f.gate) t = epi_gate_mix(t, r2v[e], d0, d1);
              v[i][e] = t;
            }
            u32x2 q; q[0] = pack_bf16x2(v[i][0], v[i][1]); q[1] = pack_bf16x2(v[i][2], v[i][3]);
            if (ok_[it]) *reinterpret_cast<u32x2*>(reinterpret_cast<bf16_t*>(f.C) + (size_t)rows_[it] * D + (sub16 + 16 * i) * 4) = q;
            v[i] = Raw4L<bf16_t>::cvt(q);                          // the LayerNorm is taken of the stored (rounded) row, as the stand-alone pass does
            sm += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
          }
          sm = xor_tree_sum<16>(sm);                   // (k_ln_fwd_v's sum16)
          const float mean = sm * invD384;
          float qq = 0.f;
#pragma unroll
          for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float dd = v[i][e] - mean; qq += dd * dd; }
          qq = xor_tree_sum<16>(qq);
          const float rstd = rsqrtf(qq * invD384 + f.ln_eps);
          if (ok_[it]) {
            bf16_t* y = reinterpret_cast<bf16_t*>(f.ln_out) + (size_t)rows_[it] * D;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
              const f32x4 gm = *reinterpret_cast<const f32x4*>(f.ln_gamma + (sub16 + 16 * i) * 4), bt = *reinterpret_cast<const f32x4*>(f.ln_beta + (sub16 + 16 * i) * 4);
              f32x4 o;
#pragma unroll
              for (int e = 0; e < 4; ++e) o[e] = (v[i][e] - mean) * rstd * gm[e] + bt[e];
              u32x2 q; q[0] = pack_bf16x2(o[0], o[1]); q[1] = pack_bf16x2(o[2], o[3]);
              *reinterpret_cast<u32x2*>(y + (sub16 + 16 * i) * 4) = q;
            }
            if (sub16 == 0 && f.ln_mean) { f.ln_mean[rows_[it]] = mean; f.ln_rstd[rows_[it]] = rstd; }
          }
        }
        __syncthreads();                                           // the half is consumed: the other half / the next tile's requests may overwrite it
      }
      continue;
    }
    // ---- the tile, rounded to bf16 (what k_gemm_nt stores), row-major in LDS: lane (li, gq) of acc[i][j] = row i * 16 + li, columns j * 16 + 4 gq ..
    {
      const unsigned base = s0 + (unsigned)((wm * 64 + (lane & 15)) * R3_RS + (wn * 96 + (lane >> 4) * 4) * 2);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          f32x2 q;
          q[0] = __uint_as_float(pack_bf16x2(acc[i][j][0], acc[i][j][1]));
          q[1] = __uint_as_float(pack_bf16x2(acc[i][j][2], acc[i][j][3]));
          ds_write64_a(base + (unsigned)(i * 16 * R3_RS + j * 32), q);
        }
    }
    wait_lgkm<0>();
    __syncthreads();
    // ---- row pass: wave w owns rows w * 16 .. + 15 of the tile, two at a time (k_ln_bwd_v's arithmetic on dy = the LDS row)
    {
      const int rbase = bm * R3_BM + w * 16;
      auto load_raw = [&](RawRow& R, int it) {
        R.r = rbase + it * 2 + rg;
        R.ok = it < 8 && R.r < g.M;
        const size_t off = (size_t)(R.ok ? R.r : 0) * D;
        const TX* x = reinterpret_cast<const TX*>(g.x) + off;
        R.mean = R.ok ? g.mean[R.r] : 0.f; R.rstd = R.ok ? g.rstd[R.r] : 0.f;
#pragma unroll
        for (int i = 0; i < NV4; ++i) {
          R.ad1[i] = (R.ok && add1) ? *reinterpret_cast<const u32x2*>(add1 + off + (sub + LPR * i) * 4) : u32x2{0u, 0u};
          R.ad2[i] = (R.ok && add2) ? *reinterpret_cast<const u32x2*>(add2 + off + (sub + LPR * i) * 4) : u32x2{0u, 0u};
          R.xv[i] = R.ok ? Raw4L<TX>::ld(x + (sub + LPR * i) * 4) : Raw4L<TX>::zero();
        }
      };
      auto process = [&](const RawRow& R, int it) {
        f32x4 xv[NV4], dv[NV4], ad1[NV4], ad2[NV4], gy[NV4];
        u32x2 dq[NV4];
        const unsigned la = s0 + (unsigned)((w * 16 + it * 2 + rg) * R3_RS + sub * 8);
#pragma unroll
        for (int i = 0; i < NV4; ++i) dq[i] = ds_read64_a(la + (unsigned)(i * LPR * 8));
        wait_lgkm<0>();
        asm volatile("" : "+v"(dq[0]), "+v"(dq[1]), "+v"(dq[2]));
#pragma unroll
        for (int i = 0; i < NV4; ++i) {
          xv[i] = Raw4L<TX>::cvt(R.xv[i]); dv[i] = Raw4L<bf16_t>::cvt(R.ok ? dq[i] : u32x2{0u, 0u});
          ad1[i] = Raw4L<bf16_t>::cvt(R.ad1[i]); ad2[i] = Raw4L<bf16_t>::cvt(R.ad2[i]);
        }
        float c1 = 0.f, c2 = 0.f;
#pragma unroll
        for (int i = 0; i < NV4; ++i)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float xh = (xv[i][e] - R.mean) * R.rstd;
            gy[i][e] = dv[i][e] * gam[i][e];
            dgam[i][e] += dv[i][e] * xh;
            dbet[i][e] += dv[i][e];
            c1 += gy[i][e];
            c2 += gy[i][e] * xh;
          }
        c1 = xor_tree_sum<LPR>(c1);                    // (k_ln_bwd_v's sum_lpr: the same additions)
        c2 = xor_tree_sum<LPR>(c2);
        c1 *= invD; c2 *= invD;
        if (R.ok) {
          bf16_t* dx = reinterpret_cast<bf16_t*>(g.dx) + (size_t)R.r * D;
#pragma unroll
          for (int i = 0; i < NV4; ++i) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = R.rstd * (gy[i][e] - c1 - ((xv[i][e] - R.mean) * R.rstd) * c2);
            if (add1) {
#pragma unroll
              for (int e = 0; e < 4; ++e) o[e] += a1 * ad1[i][e]; }
            if (add2) {
#pragma unroll
              for (int e = 0; e < 4; ++e) { o[e] += a2 * ad2[i][e]; dotB += ad2[i][e] * xv[i][e]; } }
#pragma unroll
            for (int e = 0; e < 4; ++e) dotA += o[e] * xv[i][e];
            u32x2 r; r[0] = pack_bf16x2(o[0], o[1]); r[1] = pack_bf16x2(o[2], o[3]);
            *reinterpret_cast<u32x2*>(dx + (sub + LPR * i) * 4) = r;
          }
        }
      };
      RawRow Ra, Rb, Rc;
      load_raw(Ra, 0); load_raw(Rb, 1); load_raw(Rc, 2);
      for (int it = 0; it < 8; it += 3) {
        process(Ra, it); load_raw(Ra, it + 3);
        if (it + 1 < 8) { process(Rb, it + 1); load_raw(Rb, it + 4); }
        if (it + 2 < 8) { process(Rc, it + 2); load_raw(Rc, it + 5); }
      }
    }
  }
#undef R8_RD_B
#undef R8_RD_A
#undef R8_MMA6
#undef R8_REQ
#undef R8_END
  if constexpr (MODE == 1) return;
  // ---- this workgroup's partial row [2 D + 2]: the two row groups of a wave, then the eight waves in a fixed order
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem + 2 * R3_STAGE);
  constexpr int PW = 2 * D + 2;
#pragma unroll
  for (int i = 0; i < NV4; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float gq = dgam[i][e], bq = dbet[i][e];
      gq += __shfl_xor(gq, 32, 64); bq += __shfl_xor(bq, 32, 64);
      if (rg == 0) { red[w * PW + (sub + LPR * i) * 4 + e] = gq; red[w * PW + D + (sub + LPR * i) * 4 + e] = bq; }
    }
  dotA = wave_sum(dotA); dotB = wave_sum(dotB);
  if (lane == 0) { red[w * PW + 2 * D] = dotA; red[w * PW + 2 * D + 1] = dotB; }
  __syncthreads();
  float* P = g.partial + (size_t)blockIdx.x * PW;
  for (int c = tid; c < PW; c += 512) {
    float t = red[c];
#pragma unroll
    for (int q = 1; q < 8; ++q) t += red[q * PW + c];
    P[c] = t;
  }
}

// ================================================================================================
//        NT on (32 RI) x 256 tiles with two wave groups half a phase apart ("8-phase" schedule)
// ================================================================================================
// k_gemm_nt256 keeps its eight waves in lock step: everybody reads fragments, everybody issues MFMAs, everybody waits at the one
// barrier of a k-step -- the matrix pipe idles ~27 % of every step (NOTEBOOK.md 5f).  Here the workgroup's two M groups (waves 0-3 /
// 4-7: one wave of each on every SIMD) run HALF A PHASE apart: a k-step of 64 is four phases, a phase is
//     [fragment reads + LDS-DMA requests] s_barrier [16 MFMAs] s_barrier
// and group 1 passes one extra barrier up front, so that while one wave of a SIMD issues its MFMA block the other one is in its
// read / request segment (cdna_hip_programming.md 5, "the 256^2 8-phase template"; re-derived here, the example source is not in the
// image).  A wave's 16 RI x 64 output is four quadrants: rows A0 = blocks 0 .. R0-1 / A1 = the rest, columns B0 = 0-31 / B1 = 32-63;
// phases: (A0,B0) (A0,B1) (A1,B1) (A1,B0), so a phase reads at most one new A sub-tile and one new B sub-tile: 12 / 4 / 8 / 0 reads, and
// the fragment registers are 32 + 16 + 16 instead of 96.
//   * LDS: two buffers of four 16-KB slots; a slot is the image of one sub-tile OF ALL EIGHT WAVES: A'0 = rows A0 of both M groups,
//     B'0 = columns B0 of the four N groups, B'1, A'1 likewise -- so that the slots of a k-step are read in DIFFERENT phases (0, 0, 1, 2)
//     and each can be re-filled as soon as its phase is two phases back: per phase ONE slot of a later k-step is requested (two
//     buffer_load ... lds per wave), four of them are in flight at every wait (vmcnt(8), never 0 inside a tile).
//     Order of requests: phase p of k-step X asks for  p=0: B'1(X+1)  p=1: A'1(X+1)  p=2: A'0(X+2)  p=3: B'0(X+2).
//     RAW: a slot is read one phase after the wait that covers it (wait before the phase's first barrier, read in the next phase: the
//     staggered group's waits are half a phase later).  WAR: a slot is re-filled two or more phases after its last read (the other
//     group's reads of phase g are complete only behind the second barrier of phase g).
//   * image of a slot: 128 rows x 128 B, lane-linear for the DMA, 16-byte slot (row, c) <- k-chunk c ^ (row & 7) (swizzle in the source
//     address, the same involution in the fragment address): conflict-free ds_read_b128 (k_gemm_nt256's).  RI < 8: the rows a group does
//     not own are requested out of bounds (zeros, no memory traffic), so every wave issues the same two instructions per slot and the
//     counted waits hold.
//   * persistent, XCD-major tile order, the k-steps of consecutive tiles form one stream; epilogue = nt_epilogue_rows through the
//     wave-private transpose buffer: the same bits as k_gemm_nt / k_gemm_nt256.  The epilogue drains the DMA queue once (vmcnt(0)),
//     and the first k-step behind it skips the waits of phases 0 / 1 (everything they cover was drained; a counted wait there would
//     wait for the epilogue's stores).
constexpr int P8_SLOT = 128 * 128;
constexpr int P8_BUF = 4 * P8_SLOT;
constexpr int P8_LDS = 2 * P8_BUF + G2_EPI;    // 160 KB

template <typename TC, int EPI, int RI>
__global__ __launch_bounds__(512, 2) void k_gemm_nt8p(NtArgs g, int tiles_m, int tiles_n, int nvirt) {
  typedef bf16_t T;
  typedef Mma<T> MM;
  constexpr int R0 = (RI + 1) / 2, R1 = RI - R0, BM = 32 * RI;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 2, wn = w & 3;

  const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g.A), 0, (int)(((size_t)(g.M - 1) * g.lda + g.K) * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g.B), 0, (int)(((size_t)(g.N - 1) * g.ldb + g.K) * 2), 0x00020000);
  // ---- LDS-DMA: a slot is 16 wave-instructions (8 rows x 128 B each); wave w issues instructions w (image rows 8w ..: M group 0 / N
  //      groups 0-1) and w + 8 (image rows 64 + 8w ..: M group 1 / N groups 2-3)
  const int lrow = lane >> 3, lchunk = (lane & 7) ^ lrow;
  constexpr unsigned OOB = 0x80000000u;            // beyond every buffer's range (< 2 GB): reads as zeros
  const int rr = w * 8 + lrow;                     // row inside a group's 64-row share of an A slot
  const unsigned laneA0 = rr < R0 * 16 ? (unsigned)((rr * g.lda + lchunk * 8) * 2) : OOB;
  const unsigned laneA1 = rr < R1 * 16 ? (unsigned)(((R0 * 16 + rr) * g.lda + lchunk * 8) * 2) : OOB;
  const unsigned grpA = (unsigned)(16 * RI * g.lda * 2);                                      // M group 1's rows
  const unsigned laneB = (unsigned)((((w >> 2) * 64 + (w & 3) * 8 + lrow) * g.ldb + lchunk * 8) * 2);
  const unsigned halfB = (unsigned)(32 * g.ldb * 2), grpB = (unsigned)(128 * g.ldb * 2);
  // request q (0..7) of a k-step: slot q >> 1 (A'0, B'0, B'1, A'1), instruction q & 1; src = byte offset of the tile's first row + k
  auto issue = [&](int q, unsigned srcA, unsigned srcB, int buf) {
    char* dst = smem + buf * P8_BUF + (q >> 1) * P8_SLOT + (q & 1) * 8192 + w * 1024;
    const int slot = q >> 1;
    if (slot == 0) __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (__attribute__((address_space(3))) void*)dst, 16, laneA0 + (srcA + (q & 1) * grpA), 0, 0, 0);
    else if (slot == 3) __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (__attribute__((address_space(3))) void*)dst, 16, laneA1 + (srcA + (q & 1) * grpA), 0, 0, 0);
    else __builtin_amdgcn_raw_ptr_buffer_load_lds(rB, (__attribute__((address_space(3))) void*)dst, 16, laneB + (srcB + (slot - 1) * halfB + (q & 1) * grpB), 0, 0, 0);
  };
  // ---- fragment addresses (buffer 0, k-half 0; k-half 1 = address ^ 64)
  const unsigned s0 = lds_addr(smem);
  const unsigned sw0 = (unsigned)((((lane >> 4)) ^ (lane & 7)) * 16);
  const unsigned fa0 = s0 + (unsigned)((wm * 64 + (lane & 15)) * 128) + sw0;
  const unsigned fb0 = s0 + (unsigned)((wn * 32 + (lane & 15)) * 128) + sw0;
  u32x4 FA[4][2], FB0[2][2], FB1[2][2];            // [row / column block][k half]
  f32x4 acc[RI][4];
  float alpha = g.alpha;
  if (g.alpha_ptr) alpha *= *g.alpha_ptr;
  float d0 = 0.f, d1 = 1.f;
  if (EPI == UVC_EPI_BIAS_RESID_GATE) { d0 = g.dptr[0]; d1 = g.dptr[1]; }
  float* const stg = reinterpret_cast<float*>(smem + 2 * P8_BUF) + w * (16 * 64);

  const int nk = g.K / 64;                         // >= 4
  int v = blockIdx.x, bm = 0, bn = 0;
  while (v < nvirt && !g2_tile(v, tiles_m, tiles_n, bm, bn)) v += gridDim.x;
  if (v >= nvirt) return;
  unsigned voA = (unsigned)(bm * BM * g.lda * 2), voB = (unsigned)(bn * 256 * g.ldb * 2);
  int par = 0;                                     // buffer of the current tile's k-step 0
  // prologue: k-step 0 whole, A'0 and B'0 of k-step 1 (what the steady state has requested when a k-step begins)
#pragma unroll
  for (int q = 0; q < 8; ++q) issue(q, voA, voB, 0);
#pragma unroll
  for (int q = 0; q < 4; ++q) issue(q, voA + 128, voB + 128, 1);
  wait_vm<6>();                                    // A'0, B'0, B'1 of k-step 0 have landed (this wave's parts)
  __builtin_amdgcn_s_barrier();                    // ... everybody's
  // The fragments of a phase are requested INSIDE the MFMA block of the phase before (behind the MFMAs that last use their registers), so a
  // wave's segment between the two barriers of a phase is [wait for fragments requested a whole request segment ago | 16 MFMAs with the next
  // phase's reads between them], and the segment in front of the first barrier is the two DMA requests and their counted wait alone: that is
  // what runs beside the other group's MFMA block (an LDS-DMA request costs its wave 100-200 cycles of issue; with the 12 reads of phase 0 in
  // the same segment it was longer than the MFMA block and set the phase time: 707 cycles per phase for 272 of MFMA issue, measured by removing
  // one ingredient at a time).  Waits: data consumed by the MFMAs of phase c is read in phase c - 1 and waited for in phase c - 2 (the other
  // group's wait of phase c - 2 is half a phase later): vmcnt(6) in phases 2, 3, 0, three slots in flight.
#define P8_RD_B(DST, SLOT, BO)                                                                                       \
  { const unsigned b0_ = fb0 + (BO), b1_ = (fb0 ^ 64u) + (BO);                                                        \
    DST[0][0] = ds_read128<(SLOT) * P8_SLOT>(b0_); DST[0][1] = ds_read128<(SLOT) * P8_SLOT>(b1_);                      \
    DST[1][0] = ds_read128<(SLOT) * P8_SLOT + 2048>(b0_); DST[1][1] = ds_read128<(SLOT) * P8_SLOT + 2048>(b1_); }
#define P8_RD_A(I, SLOT, BO)                                                                                         \
  { FA[I][0] = ds_read128_asm(fa0 + (BO), (SLOT) * P8_SLOT + (I) * 2048); FA[I][1] = ds_read128_asm((fa0 ^ 64u) + (BO), (SLOT) * P8_SLOT + (I) * 2048); }
#define P8_MMA4(I, AI, FB, JO)                                                                                       \
  _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                                    \
  _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                                       \
    acc[AI][(JO) + j] = MM::mma(__builtin_bit_cast(typename MM::Frag, FB[j][ks]), __builtin_bit_cast(typename MM::Frag, FA[I][ks]), acc[AI][(JO) + j]);
  // request segment of a phase: two DMA instructions (q0, q0 + 1) of the k-step (sA, sB, sbuf), the counted wait, the first barrier
#define P8_REQ(Q0, SA, SB, SBUF, WAIT)                                                                               \
  issue(Q0, SA, SB, SBUF); issue(Q0 + 1, SA, SB, SBUF);                                                               \
  if (WAIT) wait_vm<6>();                                                                                             \
  __builtin_amdgcn_s_barrier();                                                                                       \
  wait_lgkm<0>();                                                                                                     \
  __builtin_amdgcn_sched_barrier(0);                                                                                  \
  __builtin_amdgcn_s_setprio(1);
#define P8_END                                                                                                       \
  __builtin_amdgcn_s_setprio(0);                                                                                      \
  __builtin_amdgcn_sched_barrier(0);                                                                                  \
  __builtin_amdgcn_s_barrier();                                                                                       \
  __builtin_amdgcn_sched_barrier(0);
  P8_RD_B(FB0, 1, 0u)
#pragma unroll
  for (int i = 0; i < R0; ++i) P8_RD_A(i, 0, 0u)
  __builtin_amdgcn_sched_barrier(0);
  if (wm == 1) __builtin_amdgcn_s_barrier();       // group 1 runs half a phase behind from here on
  bool fresh = true;                               // phase 0's wait is needed (nothing drained the queue since the requests)

  for (;;) {
    int vn = v + gridDim.x, bmn = 0, bnn = 0;
    while (vn < nvirt && !g2_tile(vn, tiles_m, tiles_n, bmn, bnn)) vn += gridDim.x;
    const bool more = vn < nvirt;
    const unsigned voAn = more ? (unsigned)(bmn * BM * g.lda * 2) : voA, voBn = more ? (unsigned)(bnn * 256 * g.ldb * 2) : voB;
#pragma unroll
    for (int i = 0; i < RI; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < nk; ++kt) {
      const int buf = (kt & 1) ^ par;
      const unsigned bo = (unsigned)(buf * P8_BUF), bon = bo ^ (unsigned)P8_BUF;
      // k-steps kt + 1 and kt + 2 of the stream: of this tile, or k-steps 0 / 1 of the next one (behind the workgroup's last tile the
      // same instructions re-load this tile's: no branch around a DMA)
      const bool t1 = kt + 1 >= nk, t2 = kt + 2 >= nk;
      const unsigned sA1 = (t1 ? voAn : voA) + (unsigned)((t1 ? kt + 1 - nk : kt + 1) * 128), sB1 = (t1 ? voBn : voB) + (unsigned)((t1 ? kt + 1 - nk : kt + 1) * 128);
      const unsigned sA2 = (t2 ? voAn : voA) + (unsigned)((t2 ? kt + 2 - nk : kt + 2) * 128), sB2 = (t2 ? voBn : voB) + (unsigned)((t2 ? kt + 2 - nk : kt + 2) * 128);
      // ---- phase 0: (A0, B0); requests B'1 of k-step kt + 1; reads B1 of this k-step (its registers are free)
      P8_REQ(4, sA1, sB1, buf ^ 1, fresh)
      P8_RD_B(FB1, 2, bo)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < R0; ++i) P8_MMA4(i, i, FB0, 0)
      P8_END
      fresh = true;
      // ---- phase 1: (A0, B1); requests A'1 of kt + 1; reads A1 of this k-step, row block by row block behind the MFMAs that free A0's registers
      P8_REQ(6, sA1, sB1, buf ^ 1, false)
#pragma unroll
      for (int i = 0; i < R0; ++i) {
        P8_MMA4(i, i, FB1, 2)
        __builtin_amdgcn_sched_barrier(0);
        if (i < R1) P8_RD_A(i, 3, bo)
        __builtin_amdgcn_sched_barrier(0);
      }
      P8_END
      // ---- phase 2: (A1, B1); requests A'0 of kt + 2
      P8_REQ(0, sA2, sB2, buf, true)
#pragma unroll
      for (int i = 0; i < R1; ++i) P8_MMA4(i, R0 + i, FB1, 2)
      P8_END
      // ---- phase 3: (A1, B0); requests B'0 of kt + 2; reads A0 and B0 of k-step kt + 1 (the other buffer)
      P8_REQ(2, sA2, sB2, buf, true)
#pragma unroll
      for (int i = R1; i < R0; ++i) P8_RD_A(i, 0, bon)          // (registers phase 3 does not use)
#pragma unroll
      for (int i = 0; i < R1; ++i) {
        P8_MMA4(i, R0 + i, FB0, 0)
        __builtin_amdgcn_sched_barrier(0);
        P8_RD_A(i, 0, bon)
        __builtin_amdgcn_sched_barrier(0);
      }
      P8_RD_B(FB0, 1, bon)
      P8_END
    }
    // ---- epilogue (16 rows x 64 columns at a time through this wave's transpose buffer)
    wait_vm<0>();                                  // the requests of the next k-steps (in flight for 1-4 phases): drained once, here
    fresh = false;
    {
      const int m0 = bm * BM, n0 = bn * 256;
      float bias_v[OutVec<TC>::VN];
      nt_load_bias<TC, EPI>(g, lane, n0 + wn * 64, bias_v);
      NT_EPILOGUE_TILE(RI, m0 + wm * 16 * RI, n0 + wn * 64, 4, 2)
    }
    if (!more) break;
    v = vn; bm = bmn; bn = bnn; voA = voAn; voB = voBn;
    par ^= nk & 1;
  }
#undef P8_RD_B
#undef P8_RD_A
#undef P8_MMA4
#undef P8_REQ
#undef P8_END
  if (wm == 0) __builtin_amdgcn_s_barrier();       // pairs with group 1's last barrier
  wait_vm<0>();
}

// ---- launchers
namespace {

template <typename TC>
int launch_nt256_t(const NtArgs& a, int epi, hipStream_t st) {
  const int tm = ceil_div(a.M, G2_BM), tn = ceil_div(a.N, G2_BN);
  const int nvirt = ceil_div(tm, 8) * 8 * tn;               // tile numbers incl. the holes of the XCD-major order (M tiles padded to the 8 XCDs)
  const int grid = nvirt < 256 ? nvirt : 256;               // one persistent workgroup per CU
#define G2_CASE(E) case E: UVC_MAX_LDS(G2_LDS, k_gemm_nt256<TC, E>); k_gemm_nt256<TC, E><<<grid, 512, G2_LDS, st>>>(a, tm, tn, nvirt); break;
  NT_LAUNCH(epi, NT_EPI9(G2_CASE))
#undef G2_CASE
}

template <typename TC, int RI>
int launch_nt8p_ri(const NtArgs& a, int epi, hipStream_t st) {
  const int tm = ceil_div(a.M, 32 * RI), tn = ceil_div(a.N, 256);
  const int nvirt = ceil_div(tm, 8) * 8 * tn;
  const int grid = nvirt < 256 ? nvirt : 256;
#define P8_CASE(E) case E: UVC_MAX_LDS(P8_LDS, k_gemm_nt8p<TC, E, RI>); k_gemm_nt8p<TC, E, RI><<<grid, 512, P8_LDS, st>>>(a, tm, tn, nvirt); break;
  NT_LAUNCH(epi, NT_EPI9(P8_CASE))
#undef P8_CASE
}
template <typename TC>
int launch_nt8p_t(const uvc_gemm_route& r, const NtArgs& a, hipStream_t st) {
  if constexpr (sizeof(TC) == 4) return launch_nt8p_ri<TC, 8>(a, r.epilogue, st);
  else switch (r.ri) {
    case 8: return launch_nt8p_ri<TC, 8>(a, r.epilogue, st);
    case 6: return launch_nt8p_ri<TC, 6>(a, r.epilogue, st);
    case 5: return launch_nt8p_ri<TC, 5>(a, r.epilogue, st);
    default: return launch_nt8p_ri<TC, 4>(a, r.epilogue, st);
  }
}

}  // namespace

namespace uvc_gemm {
int launch_row384_fwd(const NtArgs& a, int epi, hipStream_t st) {
  LnbArgs b = {};
  b.A = a.A; b.W = a.B; b.M = a.M; b.K = a.K;
  R3Fwd f;
  f.bias = a.bias; f.R = a.R; f.R2 = a.R2; f.dptr = a.dptr; f.C = a.C; f.ln_gamma = a.ln_gamma; f.ln_beta = a.ln_beta; f.ln_out = a.ln_out;
  f.ln_mean = a.ln_mean; f.ln_rstd = a.ln_rstd; f.ln_eps = a.ln_eps; f.gate = epi == UVC_EPI_BIAS_RESID_GATE ? 1 : 0;
  const int tiles_m = ceil_div(a.M, R3_BM);
  // (tiles in whole rounds of the grid, and fewer workgroups than CUs: measured and not kept, profiles/r5o, profiles/r5k)
  const int grid = tiles_m < 256 ? tiles_m : 256;
  UVC_MAX_LDS(R3_LDS, k_gemm_row384_lnbwd<true, 1>);
  k_gemm_row384_lnbwd<true, 1><<<grid, 512, R3_LDS, st>>>(b, tiles_m, f);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

int launch_row384_lnbwd(const LnbArgs& a, int x_lowp, hipStream_t st) {
  const int tiles_m = ceil_div(a.M, R3_BM);
  const int grid = uvc_gemm_lnbwd_nblocks(a.M);           // 256 partial rows (M >= 4096): workgroups past the tiles write zeros
  R3Fwd f = {};
  if (x_lowp) { UVC_MAX_LDS(R3_LDS, k_gemm_row384_lnbwd<true>); k_gemm_row384_lnbwd<true><<<grid, 512, R3_LDS, st>>>(a, tiles_m, f); }
  else { UVC_MAX_LDS(R3_LDS, k_gemm_row384_lnbwd<false>); k_gemm_row384_lnbwd<false><<<grid, 512, R3_LDS, st>>>(a, tiles_m, f); }
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

int launch_nt256(const uvc_gemm_route& r, const NtArgs& a, hipStream_t st) { return NT_BY_TC(launch_nt256_t, a, r.epilogue, st); }
int launch_nt8p(const uvc_gemm_route& r, const NtArgs& a, hipStream_t st) { return NT_BY_TC(launch_nt8p_t, r, a, st); }
}  // namespace uvc_gemm
