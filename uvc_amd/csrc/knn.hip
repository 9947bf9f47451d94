// Nearest neighbours in a feature bank (python -m uvc_amd.compact_transfer) for gfx950: uvc_knn_topk, the k most similar bank rows of
// every query without the [nq, n] similarity matrix, and uvc_knn_vote, the weighted k-NN vote over their labels (include/uvc_kernels.h).
//
// uvc_knn_topk.  One workgroup takes 64 queries, 4 waves of 16 each; a wave keeps its queries in registers as the B operand of the MFMA
// (v_mfma_f32_16x16x32_bf16, or v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain), the bank streams through LDS as the A operand in tiles of
// 64 rows, 256 bytes of a row at a time (two buffers, the next chunk on its way in registers while this one is multiplied).  So a lane holds
// ONE query (column lane & 15 of C/D) and four bank rows per 16-row MFMA tile (rows (lane >> 4) * 4 + reg): the query's threshold, the
// similarity of its k-th neighbour so far, is one register, and the common case -- nothing in the tile beats any threshold -- is sixteen
// compares and one wave vote.  Otherwise the wave walks the tile's rows in ascending order and, per row, the queries that have a candidate
// there; the whole wave inserts one candidate into that query's sorted list in LDS, lane j holding entry j (one read, a vote for the
// position, a shift by one lane, one write): strictly greater than the last entry only, behind every entry that is not smaller -- the
// bank is visited in ascending index order, so equal values stay in index order.
// A (query, bank row) similarity is the same chain of MFMAs on the same operands wherever the pair sits: it does not depend on nq, n,
// the tile or the split, and the lists are a function of those values under a total order -- the same bits for every split count.
// With few query tiles the bank is split into contiguous row ranges over gridDim.y; k_knn_merge combines the partial lists (one wave per
// query and 64 splits, one lane per split, the lowest split wins a tie: its indices are the lowest; above 64 splits, two levels).  No atomics;
// every output element has one writer.
#include <type_traits>
#include "common.h"
#include "../../include/uvc_kernels.h"

namespace {

constexpr int QT = 64;                      // queries per workgroup
constexpr int BT = 64;                      // bank rows per tile
constexpr int CHB = 256;                    // bytes of a bank row per chunk: 128 bf16 (4 MFMA k-steps), 64 float32 (16 k-steps)
constexpr int ROWB = CHB + 16;              // LDS row stride, 68 dwords: the 16 rows of an MFMA tile start 4 banks apart
constexpr int BUFB = BT * ROWB;
constexpr int KNN_MAX_K = 64;
constexpr int KNN_MAX_D = 1024;
constexpr int KNN_MAX_SPLITS = 512;         // the merge takes 64 lists per wave: at most two levels

// NCH: the chunks the query registers are sized for (the smallest instantiation that holds D); chunks and k-steps at or beyond D are skipped
// by wave-uniform branches of the unrolled loops, a k-step that D fills in part meets zeros on both sides.
template <typename T, int NCH>
__global__ __launch_bounds__(256) void k_knn_topk(const T* __restrict__ queries, int64_t ldq, const T* __restrict__ bank, int64_t ldb, int nq, int n, int D,
                                                  int k, int64_t rows_per_split, float* __restrict__ out_s, int32_t* __restrict__ out_i) {
  constexpr bool LOWP = sizeof(T) == 2;
  constexpr int EPS = 16 / (int)sizeof(T);              // elements per 16-byte segment
  constexpr int KC = CHB / (int)sizeof(T);              // elements per chunk
  constexpr int NQF = LOWP ? NCH * 4 : NCH * 16;        // query fragments per lane: bf16x8 per 32 dims, or one float per 4 dims
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* ls = (float*)(smem + 2 * BUFB);                // [64][k] similarities, descending
  int32_t* li = (int32_t*)(ls + QT * k);                // [64][k] bank rows
  const int tid = threadIdx.x, l = tid & 63, wave = tid >> 6, lc = l & 15, lq = l >> 4;
  const int nchd = (D + KC - 1) / KC;
  const int64_t row_begin = (int64_t)blockIdx.y * rows_per_split;
  const int64_t row_end = row_begin + rows_per_split < (int64_t)n ? row_begin + rows_per_split : (int64_t)n;
  const int ntiles = row_begin < row_end ? (int)((row_end - row_begin + BT - 1) / BT) : 0;
  const int64_t qrow = (int64_t)blockIdx.x * QT + wave * 16 + lc;
  const int lbase = (wave * 16 + lc) * k;

  // the wave's 16 queries as B fragments: B[k][col = lane & 15]
  typename std::conditional<LOWP, bf16x8, float>::type qf[NQF];
  if constexpr (LOWP) {
#pragma unroll
    for (int s = 0; s < NQF; ++s) {
      const int e = s * 32 + lq * 8;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (qrow < nq && e < D) v = *(const u32x4*)(queries + (size_t)qrow * ldq + e);
      qf[s] = __builtin_bit_cast(bf16x8, v);
    }
  } else {
#pragma unroll
    for (int s = 0; s < NQF; ++s) {
      const int e = s * 4 + lq;
      qf[s] = (qrow < nq && e < D) ? queries[(size_t)qrow * ldq + e] : 0.f;
    }
  }
  if (l < 16)
    for (int j = 0; j < k; ++j) { ls[lbase + j] = -INFINITY; li[lbase + j] = -1; }
  float thr = qrow < nq ? -INFINITY : INFINITY;         // a query row past nq never has a candidate
  const bool live = (int64_t)blockIdx.x * QT + wave * 16 < nq;      // (wave-uniform) the wave holds at least one query

  u32x4 st[4];
  auto gload = [&](int tile, int c) {                   // 64 rows x 16 segments: 4 per thread; rows past the range and columns past D are zeros
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int seg = tid + i * 256;
      const int64_t row = row_begin + (int64_t)tile * BT + (seg >> 4);
      const int e = c * KC + (seg & 15) * EPS;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (row < row_end && e < D) v = *(const u32x4*)(bank + (size_t)row * ldb + e);
      st[i] = v;
    }
  };
  int par = 0;
  if (ntiles > 0) gload(0, 0);
  for (int tile = 0; tile < ntiles; ++tile) {
    f32x4 acc[4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (c < nchd) {
        char* buf = smem + par * BUFB;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int seg = tid + i * 256;
          *(u32x4*)(buf + (seg >> 4) * ROWB + (seg & 15) * 16) = st[i];
        }
        __syncthreads();      // one barrier per chunk: the buffer written next was last read before the previous barrier
        if (c + 1 < nchd) gload(tile, c + 1);
        else if (tile + 1 < ntiles) gload(tile + 1, 0);
        if (!live) {
          // (a wave without a query stages the bank with the others and multiplies nothing)
        } else if constexpr (LOWP) {
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            if (c * KC + s * 32 < D) {
#pragma unroll
              for (int rt = 0; rt < 4; ++rt) {
                const bf16x8 a = *(const bf16x8*)(buf + (rt * 16 + lc) * ROWB + s * 64 + lq * 16);      // A[row = lane & 15][k = 8 (lane >> 4) + j]
                acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, qf[c * 4 + s], acc[rt], 0, 0, 0);
              }
            }
          }
        } else {
#pragma unroll
          for (int s = 0; s < 16; ++s) {
            if (c * KC + s * 4 < D) {
#pragma unroll
              for (int rt = 0; rt < 4; ++rt) {
                const float a = *(const float*)(buf + (rt * 16 + lc) * ROWB + (s * 4 + lq) * 4);         // A[row = lane & 15][k = lane >> 4]
                acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, qf[c * 16 + s], acc[rt], 0, 0, 0);
              }
            }
          }
        }
        par ^= 1;
      }
    }
    // acc[rt][reg]: this lane's query against bank row tile0 + rt * 16 + (lane >> 4) * 4 + reg
    const int64_t tile0 = row_begin + (int64_t)tile * BT;
    bool cand = false;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (tile0 + rt * 16 + lq * 4 + r >= row_end) acc[rt][r] = -INFINITY;      // a row past the range: masked before any comparison
        cand |= acc[rt][r] > thr;
      }
    if (__any(cand)) {
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) {
        unsigned long long m[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) m[r] = __ballot(acc[rt][r] > thr);            // against thresholds that can only have risen since: never misses
#pragma unroll
        for (int qq = 0; qq < 4; ++qq)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            // the queries with a candidate in this bank row, one at a time (wave-uniform loop); the whole wave inserts: lane j holds entry j
            unsigned mm = (unsigned)(m[r] >> (16 * qq)) & 0xffffu;
            while (mm) {
              const int qi = __ffs((int)mm) - 1;
              mm &= mm - 1;
              const float v = __shfl(acc[rt][r], qq * 16 + qi, 64);               // neither NaN nor -inf: it beat a threshold
              const int base = (wave * 16 + qi) * k;
              const float e = l < k ? ls[base + l] : 0.f;
              const int pos = __popcll(__ballot(l < k && e >= v));                // the entries that are not smaller stay in front: a prefix
              if (pos < k) {                                                      // (k: the threshold rose since the vote, a tie with the last entry included)
                const int ei = l < k ? li[base + l] : -1;
                const float up_s = __shfl_up(e, 1, 64);
                const int up_i = __shfl_up(ei, 1, 64);
                const float mine = l == pos ? v : (l > pos ? up_s : e);
                if (l >= pos && l < k) {
                  ls[base + l] = mine;
                  li[base + l] = l == pos ? (int32_t)(tile0 + rt * 16 + qq * 4 + r) : up_i;
                }
                const float last = __shfl(mine, k - 1, 64);
                if (lc == qi) thr = last;                                         // in the four lanes that hold this query
              }
            }
          }
      }
    }
  }
  __syncthreads();
  for (int qi = 0; qi < 16; ++qi) {
    const int64_t qr = (int64_t)blockIdx.x * QT + wave * 16 + qi;
    if (qr < nq && l < k) {
      const size_t o = ((size_t)blockIdx.y * nq + (size_t)qr) * k + l;
      out_s[o] = ls[(wave * 16 + qi) * k + l];
      out_i[o] = li[(wave * 16 + qi) * k + l];
    }
  }
}

// one wave per query and group of 64 lists, lane s at the head of list 64 g + s; the largest head goes out, the lowest lane among equals.
// Lists [nlists][nq][k] in, [gridDim.y][nq][k] out: more than 64 splits merge in two levels, and a group's lists cover one contiguous,
// ascending range of bank rows, so the lowest list of the lowest group still holds the lowest rows.
__global__ __launch_bounds__(64) void k_knn_merge(const float* __restrict__ ws_s, const int32_t* __restrict__ ws_i, int nq, int k, int nlists,
                                                  float* __restrict__ sims, int32_t* __restrict__ idx) {
  const int l = threadIdx.x;
  const size_t qr = blockIdx.x;
  const int list = blockIdx.y * 64 + l;
  const size_t base = ((size_t)list * nq + qr) * k;
  sims += (size_t)blockIdx.y * nq * k;
  idx += (size_t)blockIdx.y * nq * k;
  int pos = 0;
  float hs = -INFINITY;
  int hi = -1;
  if (list < nlists) { hs = ws_s[base]; hi = ws_i[base]; }
  if (hi < 0) hs = -INFINITY;
  for (int j = 0; j < k; ++j) {
    const float mx = wave_max(hs);
    const unsigned long long m = __ballot(hi >= 0 && hs == mx);
    float os = -INFINITY;
    int oi = -1;
    if (m) {
      const int w = __ffsll(m) - 1;
      os = mx;
      oi = __shfl(hi, w, 64);
      if (l == w) {
        ++pos;
        hs = -INFINITY; hi = -1;
        if (pos < k) { hs = ws_s[base + pos]; hi = ws_i[base + pos]; }
        if (hi < 0) hs = -INFINITY;
      }
    }
    if (l == 0) { sims[qr * k + j] = os; idx[qr * k + j] = oi; }
  }
}

// ---------------------------------------------------------------------------- the vote (uvc_knn_vote)
// one workgroup per query: the k weights (float64: one exp each) and labels in LDS, a thread sums class c's weights in ascending j and
// rounds once; the first maximum by the block tree of k_logits_target (max of the values, then min of the columns that hold it)
__global__ __launch_bounds__(256) void k_knn_vote(const float* __restrict__ sims, const int32_t* __restrict__ idx, const void* __restrict__ labels,
                                                  int labels_i64, int n, int k, int C, float T, float* __restrict__ scores, int32_t* __restrict__ pred) {
  __shared__ double w[KNN_MAX_K];
  __shared__ int lab[KNN_MAX_K];
  __shared__ float shv[4];
  __shared__ int shi[4];
  const size_t q = blockIdx.x;
  const int tid = threadIdx.x;
  if (tid < k) {
    const int i = idx[q * k + tid];
    int c = -1;
    double ww = 0.0;
    if (i >= 0 && i < n) {
      const long long lb = labels_i64 ? ((const long long*)labels)[i] : (long long)((const int32_t*)labels)[i];
      if (lb >= 0 && lb < C) {
        c = (int)lb;
        const float s = sims[q * k + tid], s0 = sims[q * k];
        ww = (T > 0.f && s != s0) ? exp(((double)s - (double)s0) / (double)T) : 1.0;
      }
    }
    w[tid] = ww;
    lab[tid] = c;
  }
  __syncthreads();
  bool valid = false;
  for (int j = 0; j < k; ++j) valid |= lab[j] >= 0;
  float best = -1.f;
  int first = 0x7fffffff;
  for (int c = tid; c < C; c += 256) {
    double s = 0.0;
    for (int j = 0; j < k; ++j)
      if (lab[j] == c) s += w[j];
    const float f = (float)s;
    if (scores) scores[q * C + c] = f;
    if (f > best) { best = f; first = c; }
  }
  const float mx = wave_max(best);
  if ((tid & 63) == 0) shv[tid >> 6] = mx;
  __syncthreads();
  const float top = fmaxf(fmaxf(shv[0], shv[1]), fmaxf(shv[2], shv[3]));
  if (best != top) first = 0x7fffffff;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) first = min(first, __shfl_xor(first, s, 64));
  if ((tid & 63) == 0) shi[tid >> 6] = first;
  __syncthreads();
  if (tid == 0) pred[q] = valid ? min(min(shi[0], shi[1]), min(shi[2], shi[3])) : -1;
}

struct Plan { int splits; int64_t rows_per_split; };

// (similarity, row) cells of the workspace: the splits' lists, and behind them one list per group of 64 splits when there are more than 64
int64_t ws_cells(int splits, int nq, int k) {
  if (splits <= 1) return 0;
  const int64_t groups = splits > 64 ? (splits + 63) / 64 : 0;
  return ((int64_t)splits + groups) * nq * k;
}

// splits <= 0: from the shapes and the device's CU count; any request is clamped to [1, min(512, bank tiles)] and empty ranges are dropped
Plan plan_of(int nq, int n, int splits) {
  const int64_t ntiles = ((int64_t)n + BT - 1) / BT, qtiles = ((int64_t)nq + QT - 1) / QT;
  int64_t s = splits;
  if (s <= 0) {
    int ncu = 256, dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0) ncu = 256;
    // fewer query tiles than twice the CUs: split, to two workgroups per CU (every split fills its lists anew: with four per CU the two
    // large-bank shapes of tools/knn_time.py ran 1.25 x slower)
    s = qtiles >= 2 * (int64_t)ncu ? 1 : (2 * (int64_t)ncu + qtiles - 1) / qtiles;
  }
  if (s > KNN_MAX_SPLITS) s = KNN_MAX_SPLITS;
  if (s > ntiles) s = ntiles;
  if (s < 1) s = 1;
  const int64_t rps = (ntiles + s - 1) / s * BT;
  return {(int)(((int64_t)n + rps - 1) / rps), rps};
}

int check_shape(int32_t nq, int32_t n, int32_t k) {
  if (nq < 1 || n < 1) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_knn_topk: nq and n must be at least 1");
  if (k < 1 || k > KNN_MAX_K) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_knn_topk: k must lie in [1, 64]");
  return UVC_OK;
}

template <typename T, int NCH>
int launch_topk(const uvc_knn_args* a, const Plan& p, float* out_s, int32_t* out_i, hipStream_t st) {
  const int lds = 2 * BUFB + QT * a->k * 8;
  UVC_MAX_LDS(2 * BUFB + QT * KNN_MAX_K * 8, k_knn_topk<T, NCH>);
  const dim3 grid((unsigned)(((int64_t)a->nq + QT - 1) / QT), (unsigned)p.splits);
  k_knn_topk<T, NCH><<<grid, 256, lds, st>>>((const T*)a->queries, a->ldq, (const T*)a->bank, a->ldb, a->nq, a->n, a->D, a->k, p.rows_per_split, out_s, out_i);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}

}  // namespace

extern "C" int uvc_knn_workspace_bytes(int32_t nq, int32_t n, int32_t k, int32_t splits, int64_t* bytes, int32_t* splits_used) {
  if (int e = check_shape(nq, n, k)) return e;
  if (!bytes) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_knn_workspace_bytes: null pointer");
  const Plan p = plan_of(nq, n, splits);
  *bytes = ws_cells(p.splits, nq, k) * 8;
  if (splits_used) *splits_used = p.splits;
  return UVC_OK;
}

extern "C" int uvc_knn_topk(const uvc_knn_args* a, void* stream) {
  if (!a || !a->queries || !a->bank || !a->sims || !a->idx) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_knn_topk: null pointer");
  if (int e = check_shape(a->nq, a->n, a->k)) return e;
  if ((a->q_dtype != UVC_F32 && a->q_dtype != UVC_BF16) || (a->bank_dtype != UVC_F32 && a->bank_dtype != UVC_BF16))
    return uvc_set_error_msg(UVC_ERR_ARG, "uvc_knn_topk: bad dtype");
  if (a->q_dtype != a->bank_dtype) return uvc_set_error_msg(UVC_ERR_UNSUPPORTED, "uvc_knn_topk: queries and bank must have one dtype (both bf16 or both float32)");
  if (a->D < 8 || a->D > KNN_MAX_D || a->D % 8) return uvc_set_error_msg(UVC_ERR_UNSUPPORTED, "uvc_knn_topk: D must be a multiple of 8 in [8, 1024]");
  const int64_t esz = a->q_dtype == UVC_F32 ? 4 : 2;
  if (a->ldq < a->D || a->ldb < a->D) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_knn_topk: leading dimensions must be at least D");
  if ((((uintptr_t)a->queries | (uintptr_t)a->bank) & 15) || (a->ldq * esz) % 16 || (a->ldb * esz) % 16)
    return uvc_set_error_msg(UVC_ERR_ARG, "uvc_knn_topk: queries, bank and their row strides must be 16-byte aligned");
  const Plan p = plan_of(a->nq, a->n, a->splits);
  float* out_s = a->sims;
  int32_t* out_i = a->idx;
  if (p.splits > 1) {
    const int64_t cells = ws_cells(p.splits, a->nq, a->k);
    if (!a->workspace || a->workspace_bytes < cells * 8 || ((uintptr_t)a->workspace & 3))
      return uvc_set_error_msg(UVC_ERR_ARG, "uvc_knn_topk: workspace too small (uvc_knn_workspace_bytes)");
    out_s = (float*)a->workspace;
    out_i = (int32_t*)a->workspace + cells;
  }
  hipStream_t st = (hipStream_t)stream;
  const int nchd = (int)((a->D * esz + CHB - 1) / CHB);
  int rc;
  if (esz == 2) {
    if (nchd <= 1) rc = launch_topk<bf16_t, 1>(a, p, out_s, out_i, st);
    else if (nchd <= 2) rc = launch_topk<bf16_t, 2>(a, p, out_s, out_i, st);
    else if (nchd <= 3) rc = launch_topk<bf16_t, 3>(a, p, out_s, out_i, st);
    else if (nchd <= 6) rc = launch_topk<bf16_t, 6>(a, p, out_s, out_i, st);
    else rc = launch_topk<bf16_t, 8>(a, p, out_s, out_i, st);
  } else {
    if (nchd <= 1) rc = launch_topk<float, 1>(a, p, out_s, out_i, st);
    else if (nchd <= 3) rc = launch_topk<float, 3>(a, p, out_s, out_i, st);
    else if (nchd <= 6) rc = launch_topk<float, 6>(a, p, out_s, out_i, st);
    else if (nchd <= 12) rc = launch_topk<float, 12>(a, p, out_s, out_i, st);
    else rc = launch_topk<float, 16>(a, p, out_s, out_i, st);
  }
  if (rc) return rc;
  if (p.splits > 1) {
    const float* in_s = out_s;
    const int32_t* in_i = out_i;
    int lists = p.splits;
    if (lists > 64) {      // level one: groups of 64 splits into the lists behind the splits'
      const int groups = (lists + 63) / 64;
      float* mid_s = out_s + (int64_t)lists * a->nq * a->k;
      int32_t* mid_i = out_i + (int64_t)lists * a->nq * a->k;
      k_knn_merge<<<dim3((unsigned)a->nq, (unsigned)groups), 64, 0, st>>>(in_s, in_i, a->nq, a->k, lists, mid_s, mid_i);
      UVC_CHECK_LAUNCH();
      in_s = mid_s; in_i = mid_i; lists = groups;
    }
    k_knn_merge<<<dim3((unsigned)a->nq, 1), 64, 0, st>>>(in_s, in_i, a->nq, a->k, lists, a->sims, a->idx);
    UVC_CHECK_LAUNCH();
  }
  return UVC_OK;
}

extern "C" int uvc_knn_vote(const float* sims, const int32_t* idx, const void* labels, int32_t labels_i64, int32_t nq, int32_t n, int32_t k,
                            int32_t num_classes, float temperature, float* scores, int32_t* pred, void* stream) {
  if (!sims || !idx || !labels || !pred) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_knn_vote: null pointer");
  if (nq < 1 || n < 1) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_knn_vote: nq and n must be at least 1");
  if (k < 1 || k > KNN_MAX_K) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_knn_vote: k must lie in [1, 64]");
  if (num_classes < 1 || num_classes > 65536) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_knn_vote: num_classes must lie in [1, 65536]");
  if (temperature != temperature) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_knn_vote: temperature is NaN");
  k_knn_vote<<<(unsigned)nq, 256, 0, (hipStream_t)stream>>>(sims, idx, labels, labels_i64 != 0, n, k, num_classes, temperature, scores, pred);
  UVC_CHECK_LAUNCH();
  return UVC_OK;
}
