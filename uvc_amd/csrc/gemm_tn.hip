// TN GEMMs: the weight gradients, split over M and reduced in a fixed order.  Kernels, routing and entry point: TN shares no kernel code with NT, and
// its routing reads the tile table the launchers fill (TN_TILES), so they stay together.
//   uvc_gemm_tn : C[N1,N2] = beta*C + alpha * A[M,N1]^T . B[M,N2]
//   k_gemm_tn<TA, T>                        128 x 64 tiles, bf16 or float32 compute              UVC_ROUTE_TN
//   k_gemm_tn_big<TA, B1, B2, W1, W2>       192 / 256-wide tiles, register-staged (float32 A)    UVC_ROUTE_TN_BIG
//   k_gemm_tn_dma<B1, B2, W1, W2>           the same tiles on an LDS-DMA ring                    UVC_ROUTE_TN_DMA
//   k_gemm_tn8p<RI, RJ>                     two wave groups half a phase apart                   UVC_ROUTE_TN8P
//   k_tn_reduce<VEC>                        sums the splits' partial tiles
#include "gemm_common.h"

// ================================================================================================
//                                            TN (wgrad)
// ================================================================================================
// C[n1,n2] = beta*C + alpha * sum_m A[m,n1] * B[m,n2].  Block tile 128(n1) x 64(n2), reduction tile
// 64 rows of m.  The LDS image keeps the global [m][n] orientation; MFMA fragments are gathered with
// ds_read_b64_tr_b16 (bf16) or ds_read_b32 (float32).  Each block reduces one slice of M and writes
// a float32 partial tile; k_tn_reduce sums the slices in a fixed order (deterministic).
constexpr int TN_B1 = 128, TN_B2 = 64, TN_BM = 64;

template <typename T> struct TnGeom;
template <> struct TnGeom<bf16_t> { static constexpr int LD1 = TN_B1 * 2 + 32, LD2 = TN_B2 * 2 + 32; };
template <> struct TnGeom<float>  { static constexpr int LD1 = TN_B1 * 4 + 32, LD2 = TN_B2 * 4 + 32; };

// fragment of 16 columns (c0..c0+15) x one MFMA k-step starting at tile row k0, from an [m][n] LDS tile
template <typename T> struct TrFrag;
template <> struct TrFrag<bf16_t> {
  // k-slot map: group g slots 0-3 <-> rows k0+4g+{0..3}, slots 4-7 <-> rows k0+16+4g+{0..3}
  static __device__ __forceinline__ bf16x8 ld(const char* tile, int ld, int k0, int c0, int lane) {
    const int i = lane & 15, gq = lane >> 4;
    const char* p = tile + (k0 + 4 * gq + (i >> 2)) * ld + (c0 + (i & 3) * 4) * 2;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(p));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(p + 16 * ld));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    s16x8 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] = lo[e]; v[4 + e] = hi[e]; }
    return __builtin_bit_cast(bf16x8, v);
  }
};
template <> struct TrFrag<float> {
  // k-slot map: MFMA j of the step uses row k0 + 4g + j
  static __device__ __forceinline__ f32x4 ld(const char* tile, int ld, int k0, int c0, int lane) {
    const int i = lane & 15, gq = lane >> 4;
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const float*>(tile + (k0 + 4 * gq + j) * ld + (c0 + i) * 4);
    return v;
  }
};

struct TnArgs {
  const void* A; const void* B; float* part; float* bpart;   // bpart: [splits][N1] column sums of A (bias gradient) or null
  int M, N1, N2, lda, ldb, rows_per_split, xcd_remap;
};

template <typename T> struct ChunkSum;    // add the CH elements of a staged chunk into float accumulators
template <> struct ChunkSum<bf16_t> {
  static __device__ __forceinline__ void add(const u32x4& r, float* s) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { s[2 * e] += __uint_as_float(r[e] << 16); s[2 * e + 1] += __uint_as_float(r[e] & 0xffff0000u); }
  }
};
template <> struct ChunkSum<float> {
  static __device__ __forceinline__ void add(const u32x4& r, float* s) {
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] += __uint_as_float(r[e]);
  }
};

template <typename TA, typename T>
__global__ __launch_bounds__(256, 2) void k_gemm_tn(TnArgs g) {
  typedef Mma<T> MM;
  constexpr int CH = MM::CH;
  constexpr int LD1 = TnGeom<T>::LD1, LD2 = TnGeom<T>::LD2;
  constexpr int C1 = TN_B1 / CH, C2 = TN_B2 / CH;           // chunks per tile row
  constexpr int NLA = TN_BM * C1 / 256, NLB = TN_BM * C2 / 256;
  constexpr int KSUB = TN_BM / MM::KSTEP;                   // MFMA k-steps per reduction tile
  __shared__ __attribute__((aligned(16))) char sA[TN_BM * LD1];
  __shared__ __attribute__((aligned(16))) char sB[TN_BM * LD2];
  const TA* __restrict__ A = reinterpret_cast<const TA*>(g.A);
  const T* __restrict__ B = reinterpret_cast<const T*>(g.B);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int w1 = w >> 1, w2 = w & 1;                        // wave tile: 64 (n1) x 32 (n2)
  const int n10 = blockIdx.x * TN_B1, n20 = blockIdx.y * TN_B2;
  const int mbeg = blockIdx.z * g.rows_per_split;
  const int mend = min(g.M, mbeg + g.rows_per_split);

  u32x4 ra[NLA], rb[NLB];
  auto gload = [&](int m0) {
    const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < NLA; ++i) {
      const int id = tid + 256 * i, row = id / C1, c = id % C1;
      const int m = m0 + row, n = n10 + c * CH;
      ra[i] = (m < mend && n < g.N1) ? ChunkLoad<TA, T>::ld(A + (size_t)m * g.lda + n) : z;
    }
#pragma unroll
    for (int i = 0; i < NLB; ++i) {
      const int id = tid + 256 * i, row = id / C2, c = id % C2;
      const int m = m0 + row, n = n20 + c * CH;
      rb[i] = (m < mend && n < g.N2) ? ChunkLoad<T, T>::ld(B + (size_t)m * g.ldb + n) : z;
    }
  };
  float csum[CH];
#pragma unroll
  for (int e = 0; e < CH; ++e) csum[e] = 0.f;
  const bool do_cs = g.bpart != nullptr && blockIdx.y == 0;
  auto lstore = [&]() {
#pragma unroll
    for (int i = 0; i < NLA; ++i) {
      const int id = tid + 256 * i, row = id / C1, c = id % C1;
      *reinterpret_cast<u32x4*>(sA + row * LD1 + c * 16) = ra[i];
      if (do_cs) ChunkSum<T>::add(ra[i], csum);      // this thread always owns chunk column tid % C1
    }
#pragma unroll
    for (int i = 0; i < NLB; ++i) {
      const int id = tid + 256 * i, row = id / C2, c = id % C2;
      *reinterpret_cast<u32x4*>(sB + row * LD2 + c * 16) = rb[i];
    }
  };

  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (mbeg < mend) {
    gload(mbeg);
    lstore();
    __syncthreads();
    for (int m0 = mbeg; m0 < mend; m0 += TN_BM) {
      const bool more = m0 + TN_BM < mend;
      if (more) gload(m0 + TN_BM);
#pragma unroll
      for (int ks = 0; ks < KSUB; ++ks) {
        typename MM::Frag fa[4], fb[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) fa[i] = TrFrag<T>::ld(sA, LD1, ks * MM::KSTEP, w1 * 64 + i * 16, lane);
#pragma unroll
        for (int j = 0; j < 2; ++j) fb[j] = TrFrag<T>::ld(sB, LD2, ks * MM::KSTEP, w2 * 32 + j * 16, lane);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = MM::mma(fb[j], fa[i], acc[i][j]);
      }
      if (more) {
        __syncthreads();
        lstore();
        __syncthreads();
      }
    }
  }
  if (do_cs) {     // column sums of the A slice: reduce the 256/C1 threads that share a chunk column (fixed order)
    __syncthreads();
    float* red = reinterpret_cast<float*>(sA);                 // [256/C1][TN_B1]
    const int c = tid % C1, grp = tid / C1;
#pragma unroll
    for (int e = 0; e < CH; ++e) red[grp * TN_B1 + c * CH + e] = csum[e];
    __syncthreads();
    if (tid < TN_B1 && n10 + tid < g.N1) {
      float t = 0.f;
      for (int q = 0; q < 256 / C1; ++q) t += red[q * TN_B1 + tid];
      g.bpart[(size_t)blockIdx.z * g.N1 + n10 + tid] = t;
    }
  }
  // partial[z][n1][n2]: lane owns n1 = .. + (lane&15), n2 = .. + (lane>>4)*4 + {0..3}
  float* P = g.part + (size_t)blockIdx.z * g.N1 * g.N2;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n1 = n10 + w1 * 64 + i * 16 + (lane & 15);
    if (n1 >= g.N1) continue;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n2 = n20 + w2 * 32 + j * 16 + (lane >> 4) * 4;
      if (n2 + 3 < g.N2 && (g.N2 & 3) == 0) *reinterpret_cast<f32x4*>(P + (size_t)n1 * g.N2 + n2) = acc[i][j];
      else {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (n2 + e < g.N2) P[(size_t)n1 * g.N2 + n2 + e] = acc[i][j][e];
      }
    }
  }
}

// ---- big-tile variant (bf16): one workgroup of 8 waves owns a B1 x B2 output tile (192x256, 256x192 or
// 192x192), so for the DeiT shapes A (or B) is read exactly once and the other operand <= 4 times through
// L2, instead of 12x / 2x with the 128x64 tile.  The bias gradient (column sums of A) comes from one extra
// MFMA column against an all-ones fragment in the waves of the first column of tiles.
template <typename TA, int B1, int B2, int W1, int W2>
__global__ __launch_bounds__(512, 2) void k_gemm_tn_big(TnArgs g) {
  typedef bf16_t T;
  typedef Mma<T> MM;
  constexpr int LD1 = B1 * 2 + 32, LD2 = B2 * 2 + 32;
  constexpr int C1 = B1 / 8, C2 = B2 / 8;
  constexpr int NLA = TN_BM * C1 / 512, NLB = TN_BM * C2 / 512;
  constexpr int TI = B1 / W1 / 16, TJ = B2 / W2 / 16;
  static_assert(W1 * W2 == 8 && (TN_BM * C1) % 512 == 0 && (TN_BM * C2) % 512 == 0, "tile config");
  __shared__ __attribute__((aligned(16))) char sA[TN_BM * LD1];
  __shared__ __attribute__((aligned(16))) char sB[TN_BM * LD2];
  const TA* __restrict__ A = reinterpret_cast<const TA*>(g.A);
  const T* __restrict__ B = reinterpret_cast<const T*>(g.B);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int w1 = w / W2, w2 = w % W2;
  const int n10 = blockIdx.x * B1, n20 = blockIdx.y * B2;
  const int mbeg = blockIdx.z * g.rows_per_split;
  const int mend = min(g.M, mbeg + g.rows_per_split);
  const bool do_cs = g.bpart != nullptr && blockIdx.y == 0 && w2 == 0;

  u32x4 ra[NLA], rb[NLB];
  auto gload = [&](int m0) {
    const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < NLA; ++i) {
      const int id = tid + 512 * i, row = id / C1, c = id % C1;
      const int m = m0 + row;
      ra[i] = (m < mend) ? ChunkLoad<TA, T>::ld(A + (size_t)m * g.lda + n10 + c * 8) : z;
    }
#pragma unroll
    for (int i = 0; i < NLB; ++i) {
      const int id = tid + 512 * i, row = id / C2, c = id % C2;
      const int m = m0 + row;
      rb[i] = (m < mend) ? ChunkLoad<T, T>::ld(B + (size_t)m * g.ldb + n20 + c * 8) : z;
    }
  };
  auto lstore = [&]() {
#pragma unroll
    for (int i = 0; i < NLA; ++i) { const int id = tid + 512 * i; *reinterpret_cast<u32x4*>(sA + (id / C1) * LD1 + (id % C1) * 16) = ra[i]; }
#pragma unroll
    for (int i = 0; i < NLB; ++i) { const int id = tid + 512 * i; *reinterpret_cast<u32x4*>(sB + (id / C2) * LD2 + (id % C2) * 16) = rb[i]; }
  };

  f32x4 acc[TI][TJ], cs[TI];
#pragma unroll
  for (int i = 0; i < TI; ++i) {
    cs[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < TJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const u32x4 ones_u = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};
  const typename MM::Frag ones = __builtin_bit_cast(typename MM::Frag, ones_u);

  if (mbeg < mend) {
    gload(mbeg);
    lstore();
    __syncthreads();
    for (int m0 = mbeg; m0 < mend; m0 += TN_BM) {
      const bool more = m0 + TN_BM < mend;
      if (more) gload(m0 + TN_BM);
#pragma unroll
      for (int ks = 0; ks < TN_BM / 32; ++ks) {
        typename MM::Frag fa[TI], fb[TJ];
#pragma unroll
        for (int i = 0; i < TI; ++i) fa[i] = TrFrag<T>::ld(sA, LD1, ks * 32, w1 * (B1 / W1) + i * 16, lane);
#pragma unroll
        for (int j = 0; j < TJ; ++j) fb[j] = TrFrag<T>::ld(sB, LD2, ks * 32, w2 * (B2 / W2) + j * 16, lane);
#pragma unroll
        for (int i = 0; i < TI; ++i) {
#pragma unroll
          for (int j = 0; j < TJ; ++j) acc[i][j] = MM::mma(fb[j], fa[i], acc[i][j]);
          if (do_cs) cs[i] = MM::mma(ones, fa[i], cs[i]);
        }
      }
      if (more) {
        __syncthreads();
        lstore();
        __syncthreads();
      }
    }
  }
  if (do_cs && (lane >> 4) == 0) {      // every row of cs[i] holds the column sums of n1 = .. + (lane & 15)
#pragma unroll
    for (int i = 0; i < TI; ++i) g.bpart[(size_t)blockIdx.z * g.N1 + n10 + w1 * (B1 / W1) + i * 16 + (lane & 15)] = cs[i][0];
  }
  float* P = g.part + (size_t)blockIdx.z * g.N1 * g.N2;
#pragma unroll
  for (int i = 0; i < TI; ++i) {
    const int n1 = n10 + w1 * (B1 / W1) + i * 16 + (lane & 15);
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
      const int n2 = n20 + w2 * (B2 / W2) + j * 16 + (lane >> 4) * 4;
      *reinterpret_cast<f32x4*>(P + (size_t)n1 * g.N2 + n2) = acc[i][j];
    }
  }
}

// ---- big-tile variant with LDS-DMA staging (bf16 A and B): same tiles and split-M scheme as k_gemm_tn_big, but the operand
// rows go HBM -> LDS with global_load_lds_dwordx4 (no staging registers, no ds_write phase) through a ring of four 32-row
// images, three of them in flight while the fourth is multiplied: ~90 KB outstanding per CU instead of one 57 KB tile that
// was requested a single MFMA phase before it was needed (the register-staged kernel stalls ~3 us of every 4.6 us step on
// it).  One raw s_barrier per step; the waves wait on their own DMA with a counted s_waitcnt vmcnt, so the two younger
// stages stay in flight across the barrier (hipcc would drain vmcnt(0) at a __syncthreads()).  The LDS destination of a
// DMA instruction is wave-base + lane*16, so an image is the lane-linear sequence of 16-byte slots [row][chunk] with the two
// pad slots of every row (conflict-free transpose reads) filled by lanes that re-load chunk 0.
// (r5: a ring of FIVE stages, 151 KB: dW2 on 128 workgroups 84 us against 78 -- at 19.6 GB/s per CU the kernel is not waiting for a deeper ring; profiles/r5zz)
constexpr int TD_BM = 32, TD_NST = 4;

// Transposing fragment read issued as inline assembly: for a compiler-visible LDS load hipcc inserts s_waitcnt vmcnt(0) (any
// outstanding LDS-DMA may alias it), which would drain the whole ring before every step.  Same k-slot map as TrFrag<bf16_t>.
__device__ __forceinline__ s16x4 ds_tr16_asm(const char* p) {
  s16x4 v;
  const unsigned addr = (unsigned)(size_t)(LDS_PTR(char))p;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(addr));
  return v;
}
__device__ __forceinline__ bf16x8 tr_frag_asm(const char* tile, int ld, int c0, int lane) {
  const int i = lane & 15, gq = lane >> 4;
  const char* p = tile + (4 * gq + (i >> 2)) * ld + (c0 + (i & 3) * 4) * 2;
  const s16x4 lo = ds_tr16_asm(p), hi = ds_tr16_asm(p + 16 * ld);
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  s16x8 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[e] = lo[e]; v[4 + e] = hi[e]; }
  return __builtin_bit_cast(bf16x8, v);
}

// Timing probes (tools/tn_probes.sh builds copies of the library with -DUVC_TN_PROBE=n; 0 in the product): 1 = the operand ring only (no fragment reads, no MFMAs),
// 2 = the compute only (no DMA requests: the stages' LDS images hold whatever they hold), 3 = no partial-tile store.  Wrong results on purpose.
#ifndef UVC_TN_PROBE
#define UVC_TN_PROBE 0
#endif
template <int B1, int B2, int W1, int W2>
__global__ __launch_bounds__(512, 2) void k_gemm_tn_dma(TnArgs g) {
  typedef bf16_t T;
  typedef Mma<T> MM;
  constexpr int LD1 = B1 * 2 + 32, LD2 = B2 * 2 + 32;
  constexpr int S1 = LD1 / 16, S2 = LD2 / 16;
  constexpr int NSLOT = TD_BM * (S1 + S2);
  constexpr int NWI = (NSLOT + 63) / 64;                 // DMA wave-instructions per stage
  constexpr int PER = (NWI + 7) / 8;                     // per wave (waves past NWI aim theirs at a dummy KB)
  constexpr int IMG = NWI * 1024;
  constexpr int TI = B1 / W1 / 16, TJ = B2 / W2 / 16;
  static_assert(W1 * W2 == 8 && PER <= 5, "tile config");
  extern __shared__ __attribute__((aligned(16))) char smem_td[];
  char* const dummy = smem_td + TD_NST * IMG;
  const char* __restrict__ A = reinterpret_cast<const char*>(g.A);
  const char* __restrict__ B = reinterpret_cast<const char*>(g.B);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int w1 = w / W2, w2 = w % W2;
  // Workgroup -> (output tile, M split).  The dispatcher deals workgroups to the 8 XCDs round-robin; with at most one workgroup per
  // CU (grid <= 256) the tiles of one split are renumbered onto ONE XCD, adjacent in its sequence, so the operand rows the tiles
  // share are fetched from HBM once per L2 instead of once per tile (fetch traffic 271 -> 194 MB for dW2).
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  {
    const int tiles = gridDim.x * gridDim.y, total = tiles * gridDim.z;
    if (g.xcd_remap && tiles > 1 && total <= 256) {
      const int id = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
      const int xcd = id & 7, slot = id >> 3, q = total >> 3, r = total & 7;
      const int L = xcd * q + (xcd < r ? xcd : r) + slot;       // position in the XCD-major order
      const int t = L % tiles;
      bz = L / tiles; bx = t % gridDim.x; by = t / gridDim.x;
    }
  }
  const int n10 = bx * B1, n20 = by * B2;
  const int mbeg = bz * g.rows_per_split;
  const int mend = min(g.M, mbeg + g.rows_per_split);
  const bool do_cs = g.bpart != nullptr && by == 0 && w2 == 0;

  // this lane's source of DMA instruction q of a stage: byte offset at row 0 of the stage, bytes per row, row inside the stage
  int64_t goff[PER];
  int gstr[PER], grow[PER];
  bool isA[PER];
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    int slot = (w + 8 * q) * 64 + lane;
    if (slot >= NSLOT) slot = 0;                          // dummy instruction / tail lanes: any valid source
    if (slot < TD_BM * S1) {
      const int row = slot / S1, c = slot % S1;
      isA[q] = true; grow[q] = row; gstr[q] = g.lda * 2;
      goff[q] = (int64_t)row * g.lda * 2 + (n10 + (c < B1 / 8 ? c : 0) * 8) * 2;
    } else {
      const int s2 = slot - TD_BM * S1, row = s2 / S2, c = s2 % S2;
      isA[q] = false; grow[q] = row; gstr[q] = g.ldb * 2;
      goff[q] = (int64_t)row * g.ldb * 2 + (n20 + (c < B2 / 8 ? c : 0) * 8) * 2;
    }
  }
  auto issue_one = [&](int t, int q) {                   // DMA instruction q of stage t (full stages only: every row is inside the split)
    if (UVC_TN_PROBE == 2) return;
    const int m0 = mbeg + t * TD_BM;
    char* img = smem_td + (t % TD_NST) * IMG;
    const char* src = (isA[q] ? A : B) + goff[q] + (int64_t)m0 * gstr[q];
    char* dst = (w + 8 * q < NWI) ? img + (w + 8 * q) * 1024 : dummy;
    __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)src, (void __attribute__((address_space(3)))*)dst, 16, 0, 0);
  };
  auto issue = [&](int t) {
#pragma unroll
    for (int q = 0; q < PER; ++q) issue_one(t, q);
  };

  f32x4 acc[TI][TJ], cs[TI];
#pragma unroll
  for (int i = 0; i < TI; ++i) {
    cs[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < TJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const u32x4 ones_u = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};
  const typename MM::Frag ones = __builtin_bit_cast(typename MM::Frag, ones_u);

  // tn >= 0: the DMA instructions of stage tn go BETWEEN the MFMA rows (their issue cost hides under the matrix pipe; issued as a burst
  // behind the barrier they cost every wave of the lock-stepped workgroup 100-200 cycles each with nothing else to issue)
  auto compute = [&](const char* sA, int tn) {
    if (UVC_TN_PROBE == 1) {                                 // the ring alone: the next stage's requests, nothing else
      if (tn >= 0) {
#pragma unroll
        for (int q = 0; q < PER; ++q) issue_one(tn, q);
      }
      return;
    }
    const char* sB = sA + TD_BM * LD1;
    typename MM::Frag fa[TI], fb[TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i) fa[i] = tr_frag_asm(sA, LD1, w1 * (B1 / W1) + i * 16, lane);
#pragma unroll
    for (int j = 0; j < TJ; ++j) fb[j] = tr_frag_asm(sB, LD2, w2 * (B2 / W2) + j * 16, lane);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);                       // no MFMA may move above the wait of the hand-issued reads
#pragma unroll
    for (int i = 0; i < TI; ++i) {
#pragma unroll
      for (int j = 0; j < TJ; ++j) acc[i][j] = MM::mma(fb[j], fa[i], acc[i][j]);
      if (do_cs) cs[i] = MM::mma(ones, fa[i], cs[i]);
      if (tn >= 0) {
#pragma unroll
        for (int q = 0; q < PER; ++q)
          if (q * TI / PER == i) issue_one(tn, q);
      }
    }
  };
  const int rows = mbeg < mend ? mend - mbeg : 0;
  const int nfull = rows / TD_BM;
  for (int t = 0; t < TD_NST - 1 && t < nfull; ++t) issue(t);
  for (int t = 0; t < nfull; ++t) {
    const int younger = min(TD_NST - 2, nfull - 1 - t);      // stages issued after t that may stay in flight
    if (younger >= 2) wait_vm<2 * PER>();
    else if (younger == 1) wait_vm<PER>();
    else wait_vm<0>();
    __builtin_amdgcn_s_barrier();                            // stage t complete for every wave; image (t-1) % 4 is free again
    compute(smem_td + (t % TD_NST) * IMG, t + TD_NST - 1 < nfull ? t + TD_NST - 1 : -1);
  }
  if (rows % TD_BM) {                                        // partial last stage of the split: through registers, rows past mend = 0
    __builtin_amdgcn_s_barrier();
    const int m0 = mbeg + nfull * TD_BM;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      u32x4 v = {0u, 0u, 0u, 0u};
      if (m0 + grow[q] < mend) v = *reinterpret_cast<const u32x4*>((isA[q] ? A : B) + goff[q] + (int64_t)m0 * gstr[q]);
      if (w + 8 * q < NWI) *reinterpret_cast<u32x4*>(smem_td + (w + 8 * q) * 1024 + lane * 16) = v;
    }
    __syncthreads();
    compute(smem_td, -1);
  }
  if (do_cs && (lane >> 4) == 0) {
#pragma unroll
    for (int i = 0; i < TI; ++i) g.bpart[(size_t)bz * g.N1 + n10 + w1 * (B1 / W1) + i * 16 + (lane & 15)] = cs[i][0];
  }
  float* P = g.part + (size_t)bz * g.N1 * g.N2;
  if (UVC_TN_PROBE == 3 && g.M > 0) return;
#pragma unroll
  for (int i = 0; i < TI; ++i) {
    const int n1 = n10 + w1 * (B1 / W1) + i * 16 + (lane & 15);
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
      const int n2 = n20 + w2 * (B2 / W2) + j * 16 + (lane >> 4) * 4;
      *reinterpret_cast<f32x4*>(P + (size_t)n1 * g.N2 + n2) = acc[i][j];
    }
  }
}

// ---- 256 x 256 weight-gradient tiles with two wave groups half a phase apart (k_gemm_nt8p's schedule, transposing reads).
// k_gemm_tn_dma keeps its eight waves in lock step: [wait | barrier | 24 transposing fragment reads | wait | 32 MFMAs] per 32 rows, the read
// latency in front of every MFMA block (0.82-0.86 PFLOP/s on DeiT-Base's shapes).  Here a k-step is 64 rows of the split, a wave's 128 x 64
// block of the tile is four quadrants as in k_gemm_nt8p -- (A0, B0) (A0, B1) (A1, B1) (A1, B0), 16 MFMAs each -- the M groups w1 = 0 / 1 run
// half a phase apart, the fragments of a phase are requested inside the MFMA block of the phase before, and the operand rows go HBM / L2 -> LDS
// by buffer_load ... lds into two buffers of four 16-KB slots (A'0, B'0, B'1, A'1: read in phases 0, 0, 1, 2; one slot of a later k-step
// requested per phase; vmcnt(6) in phases 2, 3, 0).  A slot is 64 rows (of M) x 128 columns: [row][16 chunks of 16 B], chunk c of row r holds
// the columns of global chunk c ^ 2 (r & 7) -- the eight rows a 32-lane group of ds_read_b64_tr_b16 touches land in eight different 32-byte
// bank groups (the padded rows of k_gemm_tn_dma, without the pad slots).  Rows past the split's end are requested past the buffer
// descriptor's range and arrive as zeros, so a split need not be a whole number of k-steps.  The bias gradient (column sums of A: an
// all-ones operand against the A fragments) is spread over the four waves of a row group, two column blocks each.  Same k order per
// accumulator as k_gemm_tn_dma: the partial tiles are bit-identical.
constexpr int T8_SLOT = 64 * 256, T8_BUF = 4 * T8_SLOT, T8_LDS = 2 * T8_BUF;       // 128 KB

template <int OFF> __device__ __forceinline__ u32x2 ds_tr16_off(unsigned addr) {
  u32x2 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}
struct T8Frag { u32x2 lo, hi; };
__device__ __forceinline__ bf16x8 t8_frag(const T8Frag& f) {
  return __builtin_bit_cast(bf16x8, u32x4{f.lo[0], f.lo[1], f.hi[0], f.hi[1]});
}

// RI / RJ: 16-column blocks of N1 / N2 per wave (2 x 4 waves): tiles 256 x 256 (8, 4), 192 x 256 (6, 4), 256 x 192 (8, 3), 192 x 192 (6, 3).  The slot
// images keep their 64 x 128 shape; the columns a narrower tile does not have are requested out of range (zeros, no traffic).
template <int RI, int RJ>
__global__ __launch_bounds__(512, 2) void k_gemm_tn8p(TnArgs g) {
  typedef Mma<bf16_t> MM;
  constexpr int R0 = (RI + 1) / 2, R1 = RI - R0, J0 = (RJ + 1) / 2, J1 = RJ - J0, B1 = 32 * RI, B2 = 64 * RJ;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int w1 = w >> 2, w2 = w & 3;
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  {                                                       // (tile, split) -> XCD-major order, as k_gemm_tn_dma
    const int tiles = gridDim.x * gridDim.y, total = tiles * gridDim.z;
    if (g.xcd_remap && tiles > 1 && total <= 256) {
      const int id = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
      const int xcd = id & 7, slot = id >> 3, q = total >> 3, r = total & 7;
      const int L = xcd * q + (xcd < r ? xcd : r) + slot;
      const int t = L % tiles;
      bz = L / tiles; bx = t % gridDim.x; by = t / gridDim.x;
    }
  }
  const int n10 = bx * B1, n20 = by * B2;
  const int mbeg = bz * g.rows_per_split;
  const int mend = min(g.M, mbeg + g.rows_per_split);
  const int nk = (mend - mbeg + 63) / 64;
  const bool do_cs = g.bpart != nullptr && by == 0;
  const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g.A), 0, (int)((size_t)mend * g.lda * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g.B), 0, (int)((size_t)mend * g.ldb * 2), 0x00020000);
  // ---- LDS-DMA: a slot is 16 wave-instructions of 4 rows x 256 B; wave w issues instructions w (rows 4w ..) and w + 8 (rows 32 + 4w ..)
  unsigned laneA0, laneA1, laneB0, laneB1;
  {
    const int r = 4 * w + (lane >> 4), cg = (lane & 15) ^ (2 * (r & 7));        // global chunk this lane fetches
    const int ca = cg & 7, cb = cg & 3;                                          // chunk inside a row group's / column group's share of the slot
    const int colA = (cg >> 3) * (16 * RI) + ca * 8, colB = (cg >> 2) * (16 * RJ) + cb * 8;
    constexpr unsigned OOB = 0x80000000u;
    laneA0 = ca < 2 * R0 ? (unsigned)((r * g.lda + n10 + colA) * 2) : OOB;
    laneA1 = ca < 2 * R1 ? (unsigned)((r * g.lda + n10 + colA + 16 * R0) * 2) : OOB;
    laneB0 = cb < 2 * J0 ? (unsigned)((r * g.ldb + n20 + colB) * 2) : OOB;
    laneB1 = cb < 2 * J1 ? (unsigned)((r * g.ldb + n20 + colB + 16 * J0) * 2) : OOB;
  }
  const unsigned hiA = (unsigned)(32 * g.lda * 2), hiB = (unsigned)(32 * g.ldb * 2);
  // request q (0..7) of the k-step whose first row is m: slot q >> 1 (A'0, B'0, B'1, A'1), instruction q & 1
  auto issue = [&](int q, int m, int buf) {
    char* dst = smem + buf * T8_BUF + (q >> 1) * T8_SLOT + (q & 1) * 8192 + w * 1024;
    const int slot = q >> 1;
    const unsigned ra = (unsigned)(m * g.lda * 2), rb = (unsigned)(m * g.ldb * 2);
    if (slot == 0) __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (__attribute__((address_space(3))) void*)dst, 16, laneA0 + (ra + (q & 1) * hiA), 0, 0, 0);
    else if (slot == 3) __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (__attribute__((address_space(3))) void*)dst, 16, laneA1 + (ra + (q & 1) * hiA), 0, 0, 0);
    else if (slot == 1) __builtin_amdgcn_raw_ptr_buffer_load_lds(rB, (__attribute__((address_space(3))) void*)dst, 16, laneB0 + (rb + (q & 1) * hiB), 0, 0, 0);
    else __builtin_amdgcn_raw_ptr_buffer_load_lds(rB, (__attribute__((address_space(3))) void*)dst, 16, laneB1 + (rb + (q & 1) * hiB), 0, 0, 0);
  };
  // ---- fragment addresses (buffer 0, rows 0-31 of the slot, first of the two reads; + 4096: rows + 16; + 8192: rows 32-63)
  const unsigned s0 = lds_addr(smem);
  unsigned fa[4], fb[2];
  {
    const int il = lane & 15, gq = lane >> 4;
    const int R = 4 * gq + (il >> 2), sw = R & 7, b = (il >> 1) & 1, half = il & 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) fa[i] = s0 + (unsigned)(R * 256 + ((((w1 * 4 + i) ^ sw) * 2 + b) * 16) + half * 8);
#pragma unroll
    for (int j = 0; j < 2; ++j) fb[j] = s0 + (unsigned)(R * 256 + ((((w2 * 2 + j) ^ sw) * 2 + b) * 16) + half * 8);
  }
  T8Frag FA[4][2], FB0[2][2], FB1[2][2];
  f32x4 acc[RI][RJ], cs[2];
#pragma unroll
  for (int i = 0; i < RI; ++i)
#pragma unroll
    for (int j = 0; j < RJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  cs[0] = f32x4{0.f, 0.f, 0.f, 0.f}; cs[1] = cs[0];
  const u32x4 ones_u = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};
  const typename MM::Frag ones = __builtin_bit_cast(typename MM::Frag, ones_u);

#define T8_RD(F, ADDR, SLOT, KS) { F.lo = ds_tr16_off<(SLOT) * T8_SLOT + (KS) * 8192>(ADDR); F.hi = ds_tr16_off<(SLOT) * T8_SLOT + (KS) * 8192 + 4096>(ADDR); }
#define T8_RD_B(DST, SLOT, BO, NJ)                                                                                    \
  _Pragma("unroll") for (int j = 0; j < (NJ); ++j) { T8_RD(DST[j][0], fb[j] + (BO), SLOT, 0) T8_RD(DST[j][1], fb[j] + (BO), SLOT, 1) }
#define T8_RD_A(I, SLOT, BO) { T8_RD(FA[I][0], fa[I] + (BO), SLOT, 0) T8_RD(FA[I][1], fa[I] + (BO), SLOT, 1) }
#define T8_MMA4(I, AI, FB, JO, NJ)                                                                                    \
  _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                                     \
  _Pragma("unroll") for (int j = 0; j < (NJ); ++j)                                                                     \
    acc[AI][(JO) + j] = MM::mma(t8_frag(FB[j][ks]), t8_frag(FA[I][ks]), acc[AI][(JO) + j]);
#define T8_CS(U, I) { cs[U] = MM::mma(ones, t8_frag(FA[I][0]), cs[U]); cs[U] = MM::mma(ones, t8_frag(FA[I][1]), cs[U]); }
  // column sums: wave w2 of a row group takes the column blocks 2 w2, 2 w2 + 1 of its RI; HALF = 0: blocks in A0 (phase 0), 1: in A1 (phase 2)
#define T8_CS_PHASE(HALF)                                                                                             \
  if (do_cs) {                                                                                                         \
    _Pragma("unroll") for (int W = 0; W < 4; ++W)                                                                      \
      if (w2 == W) {                                                                                                   \
        _Pragma("unroll") for (int u = 0; u < 2; ++u) {                                                                \
          const int gi = 2 * W + u;                                                                                    \
          if (gi < RI && (gi >= R0) == ((HALF) == 1)) { if (u == 0) T8_CS(0, gi - (HALF) * R0) else T8_CS(1, gi - (HALF) * R0) }  \
        }                                                                                                              \
      }                                                                                                                \
  }
#define T8_REQ(Q0, M, SBUF, WAIT)                                                                                     \
  issue(Q0, M, SBUF); issue(Q0 + 1, M, SBUF);                                                                          \
  if (WAIT) wait_vm<6>();                                                                                              \
  __builtin_amdgcn_s_barrier();                                                                                        \
  wait_lgkm<0>();                                                                                                      \
  __builtin_amdgcn_sched_barrier(0);                                                                                   \
  __builtin_amdgcn_s_setprio(1);
#define T8_END                                                                                                        \
  __builtin_amdgcn_s_setprio(0);                                                                                       \
  __builtin_amdgcn_sched_barrier(0);                                                                                   \
  __builtin_amdgcn_s_barrier();                                                                                        \
  __builtin_amdgcn_sched_barrier(0);

  // prologue: k-step 0 whole, A'0 and B'0 of k-step 1
#pragma unroll
  for (int q = 0; q < 8; ++q) issue(q, mbeg, 0);
#pragma unroll
  for (int q = 0; q < 4; ++q) issue(q, mbeg + 64, 1);
  wait_vm<6>();
  __builtin_amdgcn_s_barrier();
  T8_RD_B(FB0, 1, 0u, J0)
#pragma unroll
  for (int i = 0; i < R0; ++i) T8_RD_A(i, 0, 0u)
  __builtin_amdgcn_sched_barrier(0);
  if (w1 == 1) __builtin_amdgcn_s_barrier();      // group 1 runs half a phase behind from here on
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    const unsigned bo = (unsigned)(buf * T8_BUF), bon = bo ^ (unsigned)T8_BUF;
    const int m1 = mbeg + (kt + 1) * 64, m2 = m1 + 64;   // (past the split's end: out of the descriptors' range, zeros nobody multiplies)
    // ---- phase 0: (A0, B0); requests B'1 of k-step kt + 1; reads B1 of this k-step
    T8_REQ(4, m1, buf ^ 1, true)
    T8_RD_B(FB1, 2, bo, J1)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < R0; ++i) T8_MMA4(i, i, FB0, 0, J0)
    T8_CS_PHASE(0)
    T8_END
    // ---- phase 1: (A0, B1); requests A'1 of kt + 1; reads A1 behind the MFMAs that free A0's registers
    T8_REQ(6, m1, buf ^ 1, false)
#pragma unroll
    for (int i = 0; i < R0; ++i) {
      T8_MMA4(i, i, FB1, J0, J1)
      __builtin_amdgcn_sched_barrier(0);
      if (i < R1) T8_RD_A(i, 3, bo)
      __builtin_amdgcn_sched_barrier(0);
    }
    T8_END
    // ---- phase 2: (A1, B1); requests A'0 of kt + 2
    T8_REQ(0, m2, buf, true)
#pragma unroll
    for (int i = 0; i < R1; ++i) T8_MMA4(i, R0 + i, FB1, J0, J1)
    T8_CS_PHASE(1)
    T8_END
    // ---- phase 3: (A1, B0); requests B'0 of kt + 2; reads A0 and B0 of k-step kt + 1 (the other buffer)
    T8_REQ(2, m2, buf, true)
#pragma unroll
    for (int i = R1; i < R0; ++i) T8_RD_A(i, 0, bon)            // (registers phase 3 does not use)
#pragma unroll
    for (int i = 0; i < R1; ++i) {
      T8_MMA4(i, R0 + i, FB0, 0, J0)
      __builtin_amdgcn_sched_barrier(0);
      T8_RD_A(i, 0, bon)
      __builtin_amdgcn_sched_barrier(0);
    }
    T8_RD_B(FB0, 1, bon, J0)
    T8_END
  }
#undef T8_RD
#undef T8_RD_B
#undef T8_RD_A
#undef T8_MMA4
#undef T8_CS
#undef T8_CS_PHASE
#undef T8_REQ
#undef T8_END
  if (w1 == 0) __builtin_amdgcn_s_barrier();      // pairs with group 1's last barrier
  wait_vm<0>();
  wait_lgkm<0>();
  if (do_cs && (lane >> 4) == 0) {                // every row of cs[u] holds the column sums of n1 = .. + (lane & 15)
    float* bp = g.bpart + (size_t)bz * g.N1 + n10 + w1 * (16 * RI) + w2 * 32 + (lane & 15);       // column blocks 2 w2, 2 w2 + 1
    if (2 * w2 < RI) bp[0] = cs[0][0];
    if (2 * w2 + 1 < RI) bp[16] = cs[1][0];
  }
  float* P = g.part + (size_t)bz * g.N1 * g.N2;
#pragma unroll
  for (int i = 0; i < RI; ++i) {
    const int n1 = n10 + w1 * (16 * RI) + i * 16 + (lane & 15);
#pragma unroll
    for (int j = 0; j < RJ; ++j) {
      const int n2 = n20 + w2 * (16 * RJ) + j * 16 + (lane >> 4) * 4;
      *reinterpret_cast<f32x4*>(P + (size_t)n1 * g.N2 + n2) = acc[i][j];
    }
  }
}

// sum the split-M partial tiles (and partial column sums) in a fixed order.  VEC = 4: 16-byte accesses, 4 slices in flight
template <int VEC>
__global__ __launch_bounds__(256) void k_tn_reduce(const float* __restrict__ part, float* __restrict__ C, int n, int ldc,
                                                   int N2, int splits, float alpha, const float* alpha_ptr, float beta,
                                                   const float* __restrict__ bpart, float* __restrict__ bias_out, int N1) {
  const int i = (blockIdx.x * 256 + threadIdx.x) * VEC;
  if (i >= n + (bpart ? N1 : 0)) return;
  if (alpha_ptr) alpha *= *alpha_ptr;
  const bool main_part = i < n;
  const float* src = main_part ? part + i : bpart + (i - n);
  const size_t stride = main_part ? (size_t)n : (size_t)N1;
  float s[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) s[e] = 0.f;
  int z = 0;
  for (; z + 4 <= splits; z += 4) {
    float v[4][VEC];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (VEC == 4) { const f32x4 t = *reinterpret_cast<const f32x4*>(src + (size_t)(z + u) * stride); v[u][0] = t[0]; v[u][1 % VEC] = t[1]; v[u][2 % VEC] = t[2]; v[u][3 % VEC] = t[3]; }
      else v[u][0] = src[(size_t)(z + u) * stride];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int e = 0; e < VEC; ++e) s[e] += v[u][e];
  }
  for (; z < splits; ++z)
#pragma unroll
    for (int e = 0; e < VEC; ++e) s[e] += src[(size_t)z * stride + e];
  float* dst = main_part ? C + (size_t)(i / N2) * ldc + (i % N2) : bias_out + (i - n);
#pragma unroll
  for (int e = 0; e < VEC; ++e) dst[e] = (beta != 0.f ? beta * dst[e] : 0.f) + alpha * s[e];
}

// ================================================================================================
//                      TN: routing, launchers and the entry point (host code)
// ================================================================================================
namespace {

using TnLaunch = int (*)(const TnArgs&, dim3, hipStream_t);
template <int RI, int RJ>
int launch_tn8p(const TnArgs& a, dim3 grid, hipStream_t st) {
  UVC_MAX_LDS(T8_LDS, k_gemm_tn8p<RI, RJ>);
  k_gemm_tn8p<RI, RJ><<<grid, 512, T8_LDS, st>>>(a);
  return UVC_OK;
}
template <int B1, int B2, int W1, int W2>
int launch_tn_dma(const TnArgs& a, dim3 grid, hipStream_t st) {
  const int sh = TD_NST * (((TD_BM * ((B1 * 2 + 32) / 16 + (B2 * 2 + 32) / 16) + 63) / 64) * 1024) + 1024;
  UVC_MAX_LDS(sh, k_gemm_tn_dma<B1, B2, W1, W2>);
  k_gemm_tn_dma<B1, B2, W1, W2><<<grid, 512, sh, st>>>(a);
  return UVC_OK;
}
template <int B1, int B2, int W1, int W2>
int launch_tn_big(const TnArgs& a, dim3 grid, hipStream_t st) {      // float32 A (converted on load): the register-staged kernel
  k_gemm_tn_big<float, B1, B2, W1, W2><<<grid, 512, 0, st>>>(a);
  return UVC_OK;
}

// cfg -> tile and the kernels built for it.  k_gemm_tn8p (two-group schedule): dW2 79.4 -> 64.6 us, dW1 77.4 -> 60.9, dW_qkv 45.9 -> 40.9 against the ring
// kernel k_gemm_tn_dma, bit-identical partial tiles (profiles/r6h_tn_probes.txt); k_gemm_tn_big takes float32 A.  cfg 0 is the generic 128 x 64 kernel.
struct TnTile { int b1, b2; TnLaunch tn8p, dma, big; };
const TnTile TN_TILES[7] = {
    {TN_B1, TN_B2, nullptr, nullptr, nullptr},
    {192, 256, launch_tn8p<6, 4>, launch_tn_dma<192, 256, 2, 4>, launch_tn_big<192, 256, 2, 4>},
    {256, 192, launch_tn8p<8, 3>, launch_tn_dma<256, 192, 4, 2>, launch_tn_big<256, 192, 4, 2>},
    {192, 192, launch_tn8p<6, 3>, launch_tn_dma<192, 192, 2, 4>, launch_tn_big<192, 192, 2, 4>},
    {96, 192, nullptr, launch_tn_dma<96, 192, 2, 4>, nullptr},        // dW_proj of DeiT-Tiny: two tiles x 128 splits (the generic kernel ran it at 1.75 TB/s)
    {256, 256, launch_tn8p<8, 4>, nullptr, nullptr},                  // DeiT-Base: 131 flop per operand byte through LDS against 108 for 192 x 256
    {128, 256, launch_tn8p<4, 4>, nullptr, nullptr},                  // UVC_TN_128X256 only: not the default (profiles/r6n_tn_variants_base.txt)
};

// the tile configuration a shape takes with bf16 operands
int tn_shape_cfg(int N1, int N2) {
  if (N1 % 256 == 0 && N2 % 256 == 0 && (N1 / 256) * (N2 / 256) >= 9) return 5;     // 9 tiles = DeiT-Base's dW_proj; narrower shapes divide into 192-wide tiles
  if (N1 % 192 == 0 && N2 % 256 == 0) return 1;
  if (N1 % 256 == 0 && N2 % 192 == 0) return 2;
  if (N1 % 192 == 0 && N2 % 192 == 0 && (N1 / 192) * (N2 / 192) >= 2) return 3;     // a single 192 x 192 tile would need 256 splits
  if (N1 == 192 && N2 == 192) return 4;
  return 0;
}
int tn_splits(int M, int N1, int N2, int cfg) {
  int tiles, target;
  if (cfg == 0) { tiles = ceil_div(N1, TN_B1) * ceil_div(N2, TN_B2); target = 768; }
  else {
    tiles = (N1 / TN_TILES[cfg].b1) * (N2 / TN_TILES[cfg].b2);
    // one workgroup per CU; on HALF the CUs where the output is a handful of tiles (DeiT-Tiny's 192-wide weights): half the float32 partial bytes, and the dgrad
    // chain on the other stream gets the CUs.  128 / 160 / 192 / 256 workgroups: 11.14 / 11.18 / 11.23 / 11.44 ms per step (profiles/r5z_ab_wgrad_targets.txt,
    // profiles/r6i_ab_wgrad_targets.txt)
    target = tiles <= 4 ? 128 : 256;
  }
  int splits = cfg == 0 ? ceil_div(target, tiles) : target / tiles;       // big tiles: at most 256 workgroups -- one more is a second round
  const int max_splits = ceil_div(M, TN_BM);
  if (splits > max_splits) splits = max_splits;
  // not more splits than rows justify (a split writes and the reduce re-reads a float32 tile): >= 1024 rows per split, DeiT-Tiny 12.19 -> 12.06 ms; the
  // 192 x 192 tiles at M < 32 k (T2T-ViT-14) >= 2048 rows, 13.22 -> 12.88 ms
  const int rmin = (cfg == 3 && M < 32768) ? 2048 : 1024;
  if (cfg != 0 && M >= 2 * rmin && splits > M / rmin) splits = M / rmin;
  return splits < 1 ? 1 : splits;
}
int tn_workspace_splits(int M, int N1, int N2) {             // large enough for the generic kernel and for the shape's own configuration
  const int s0 = tn_splits(M, N1, N2, 0), s1 = tn_splits(M, N1, N2, tn_shape_cfg(N1, N2));
  return s0 > s1 ? s0 : s1;
}
int64_t tn_workspace_bytes(int splits, int N1, int N2) { return (int64_t)splits * ((int64_t)N1 * N2 + N1) * 4; }   // partial tiles + partial column sums

// Every check of uvc_gemm_tn, then configuration, kernel family, splits and rows per split.  No HIP call; pointers are read as integers only.
int tn_route(const uvc_gemm_tn_args& p, uvc_gemm_route* r) {
  *r = uvc_gemm_route{};
  if (!p.A || !p.B || !p.C || !p.workspace) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_tn: null pointer");
  if (p.M <= 0 || p.N1 <= 0 || p.N2 <= 0) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_tn: empty problem");
  const int ch = (p.dtype == UVC_F32) ? 4 : 8;
  if (p.N1 % ch || p.N2 % ch || p.lda % ch || p.ldb % ch)
    return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_tn: N1, N2, lda, ldb must be multiples of a 16-byte chunk");
  if (p.workspace_bytes < tn_workspace_bytes(tn_workspace_splits(p.M, p.N1, p.N2), p.N1, p.N2))
    return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_tn: workspace too small");
  if (p.dtype == UVC_F32 && !p.a_is_f32) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_tn: float32 mode needs float32 A");
  if (p.dtype != UVC_F32 && p.dtype != UVC_BF16) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_tn: dtype must be UVC_F32 or UVC_BF16");
  const bool a_f32 = p.a_is_f32 != 0;
  int cfg = (p.dtype == UVC_BF16 && p.lda % 8 == 0 && p.ldb % 8 == 0) ? tn_shape_cfg(p.N1, p.N2) : 0;
  // float32 A: k_gemm_tn_big's tiles (cfgs 1, 2, 3) or the generic kernel
  if (cfg == 4 && a_f32) cfg = 0;
  if (cfg == 5 && a_f32) cfg = (p.N1 % 192 == 0 && p.N2 % 256 == 0) ? 1 : (p.N1 % 256 == 0 && p.N2 % 192 == 0) ? 2 : 0;
  // k_gemm_tn8p addresses its operands with 32-bit buffer offsets, the requests up to 256 rows past a split's end included: every offset below 2 GB.  Beyond,
  // cfgs 1, 2, 3 take the ring kernel (64-bit offsets; same tiles, splits and k order: the same bits) and the 256 x 256 tiles the generic kernel -- checked
  // on the configuration that will RUN
  const bool tn8p_fits = (int64_t)(p.M + 256) * (p.lda > p.ldb ? p.lda : p.ldb) * 2 < (1ll << 31);
  if (cfg == 5 && !tn8p_fits) cfg = 0;
  if (cfg == 5 && p.variant == UVC_TN_128X256) cfg = 6;
  const TnTile& t = TN_TILES[cfg];
  r->cfg = cfg; r->b1 = t.b1; r->b2 = t.b2; r->a_f32 = a_f32; r->t_f32 = p.dtype == UVC_F32;
  r->family = cfg == 0 ? UVC_ROUTE_TN : a_f32 ? UVC_ROUTE_TN_BIG : (t.tn8p && (!t.dma || (tn8p_fits && p.variant != UVC_TN_RING))) ? UVC_ROUTE_TN8P : UVC_ROUTE_TN_DMA;
  const int rps = ceil_div(ceil_div(p.M, tn_splits(p.M, p.N1, p.N2, cfg)), TN_BM) * TN_BM;
  r->rows_per_split = rps; r->splits = ceil_div(p.M, rps);
  return UVC_OK;
}

}  // namespace

extern "C" int uvc_gemm_tn_workspace_bytes(int M, int N1, int N2, int64_t* bytes, int* splits_out) {
  if (!bytes) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_tn_workspace_bytes: null");
  const int splits = tn_workspace_splits(M, N1, N2);
  *bytes = tn_workspace_bytes(splits, N1, N2);
  if (splits_out) *splits_out = splits;
  return UVC_OK;
}

extern "C" int uvc_gemm_tn_route(const uvc_gemm_tn_args* p, uvc_gemm_route* r) {
  if (!p || !r) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_tn: null pointer");
  return tn_route(*p, r);
}

extern "C" int uvc_gemm_tn(const uvc_gemm_tn_args* p, void* stream) {
  uvc_gemm_route r;
  if (const int rc = uvc_gemm_tn_route(p, &r)) return rc;
  TnArgs a;
  a.A = p->A; a.B = p->B; a.part = (float*)p->workspace; a.M = p->M; a.N1 = p->N1; a.N2 = p->N2; a.lda = p->lda; a.ldb = p->ldb;
  a.rows_per_split = r.rows_per_split;
  a.xcd_remap = 1;
  a.bpart = p->colsum_out ? a.part + (size_t)r.splits * p->N1 * p->N2 : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const TnTile& t = TN_TILES[r.cfg];
  const dim3 grid(ceil_div(p->N1, t.b1), ceil_div(p->N2, t.b2), r.splits);      // (the big tiles divide their shapes)
  switch (r.family) {
    case UVC_ROUTE_TN:
      if (r.t_f32) k_gemm_tn<float, float><<<grid, 256, 0, st>>>(a);
      else if (r.a_f32) k_gemm_tn<float, bf16_t><<<grid, 256, 0, st>>>(a);
      else k_gemm_tn<bf16_t, bf16_t><<<grid, 256, 0, st>>>(a);
      break;
    case UVC_ROUTE_TN_BIG: if (const int rc = t.big(a, grid, st)) return rc; break;
    case UVC_ROUTE_TN_DMA: if (const int rc = t.dma(a, grid, st)) return rc; break;
    case UVC_ROUTE_TN8P: if (const int rc = t.tn8p(a, grid, st)) return rc; break;
    default: return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_tn: route");
  }
  UVC_CHECK_LAUNCH();
  const int n = p->N1 * p->N2;
  const int tot = n + (a.bpart ? p->N1 : 0);
  if (n % 4 == 0 && p->N2 % 4 == 0 && p->ldc % 4 == 0 && p->N1 % 4 == 0)
    k_tn_reduce<4><<<ceil_div(tot / 4, 256), 256, 0, st>>>(a.part, p->C, n, p->ldc, p->N2, r.splits, p->alpha, p->alpha_ptr, p->beta, a.bpart, p->colsum_out, p->N1);
  else
    k_tn_reduce<1><<<ceil_div(tot, 256), 256, 0, st>>>(a.part, p->C, n, p->ldc, p->N2, r.splits, p->alpha, p->alpha_ptr, p->beta, a.bpart, p->colsum_out, p->N1);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}
