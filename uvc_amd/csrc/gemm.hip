// MFMA GEMMs for the DeiT step on gfx950: which kernel runs a problem.
//   uvc_gemm_nt : C[M,N] = epi( A[M,K] . B[N,K]^T )       forward Linear / dgrad (with W^T copies)
//   uvc_gemm_tn : C[N1,N2] = beta*C + alpha * A[M,N1]^T . B[M,N2]   wgrad, split over M, deterministic       (gemm_tn.hip, routing included)
// Compute type T = bf16 (v_mfma_f32_16x16x32_bf16, fp32 accumulate) or float
// (v_mfma_f32_16x16x4_f32, bit-exact fmaf chain) -- the latter is the 1e-3 parity mode.
//
// No kernel is defined here.  Every kernel family has a file of its own with its launchers (the table at the top of gemm_common.h, which also holds
// what the kernels share); this file is the routing of uvc_gemm_nt -- the predicates of every family, nt_route, the *_supported queries -- the entry
// point, which reaches the kernels through uvc_gemm::launch_*, and the route -> kernel name table.
#include "gemm_common.h"

// ================================================================================================
//                      NT: routing and the entry point (host code)
// ================================================================================================
// nt_route() decides which kernel runs a problem and with which template arguments; uvc_gemm_nt() is nt_route() and one switch
// over the family.  The launchers (uvc_gemm::launch_*, next to their kernels) compute grid and LDS bytes and decide nothing.  DESIGN.md ("GEMM routing") has the table
// family -> kernel -> rule -> where measured; NOTEBOOK.md ("gemm.hip dispatcher comments") the history of each rule.
namespace {

NtArgs nt_args(const uvc_gemm_nt_args& p) {
  NtArgs a;
  a.A = p.A; a.B = p.B; a.C = p.C; a.C2 = p.C2; a.bias = p.bias; a.R = p.R; a.R2 = p.R2; a.aux = p.aux;
  a.dptr = p.gate; a.M = p.M; a.N = p.N; a.K = p.K; a.lda = p.lda; a.ldb = p.ldb; a.ldc = p.ldc;
  a.ldr = p.ldr ? p.ldr : p.ldc; a.ldaux = p.ldaux ? p.ldaux : p.ldc; a.alpha = p.alpha; a.alpha_ptr = p.alpha_ptr;
  a.ln_gamma = p.ln_gamma; a.ln_beta = p.ln_beta; a.ln_out = p.ln_out; a.ln_mean = p.ln_mean; a.ln_rstd = p.ln_rstd; a.ln_eps = p.ln_eps;
  a.no_dma = p.force_generic == UVC_NT_NO_DMA;
  return a;
}

// ---- what each family takes
bool epi_resid(int e) { return e == UVC_EPI_BIAS_RESID || e == UVC_EPI_BIAS_RESID_GATE; }
// k_gemm_ws at K = 192 / 128: N a multiple of 64, vector-aligned leading dimensions
bool ws_ok(const NtArgs& a, int vn) {
  return (a.K == 192 || a.K == 128) && a.N % 64 == 0 && a.ldb == a.K && a.lda % 8 == 0 && a.ldc % vn == 0 && a.ldr % vn == 0 &&
         a.ldaux % vn == 0 && a.M >= 4096;
}
// k_gemm_ws at K = 384, N a multiple of 192 (DeiT-Small / T2T-ViT).  The plain epilogue in the eight-wave form only, and the recomputing dGELU never: both
// were slower than the generic kernel (26 -> 28 us, 149 -> 162 us at M = 50 k)
bool ws384_ok(const NtArgs& a, int epi, int vn, bool a_f32) {
  if (epi == UVC_EPI_DGELU) return false;
  if (epi == UVC_EPI_NONE && !(vn == 8 && a.N % 128 == 0 && a.N >= 512)) return false;
  return !a_f32 && a.K == 384 && a.N % 192 == 0 && a.ldb == a.K && a.lda % 8 == 0 && a.ldc % vn == 0 && a.ldr % vn == 0 && a.ldaux % vn == 0 && a.M >= 4096;
}
// k_gemm_wsn / k_gemm_wsn16: N = 192 against K = 768 / 576 (DeiT-Tiny) or 512 / 256 (compacted Stage-2 widths)
bool wsn_ok(const NtArgs& a, int epi, bool a_f32) {
  return !a_f32 && a.N == 192 && (a.K == 768 || a.K == 576 || a.K == 512 || a.K == 256) && a.ldb == a.K && a.lda % 8 == 0 && a.ldc % 4 == 0 && a.ldr % 4 == 0 && a.M >= 4096 &&
         (epi == UVC_EPI_NONE || epi == UVC_EPI_BIAS || epi == UVC_EPI_BIAS_RESID || epi == UVC_EPI_BIAS_RESID_GATE);
}
// k_gemm_wsn16_dma: contiguous A and residual rows, 16-byte aligned
bool wsn16_dma_ok(const NtArgs& a) {
  return a.M >= 16 && a.lda == a.K && a.ldr == 192 && a.ldc % 4 == 0 && (((uintptr_t)a.R | (uintptr_t)a.R2 | (uintptr_t)a.A) & 15) == 0;
}
bool nt_rows_epilogue(int epi) {
  return epi == UVC_EPI_NONE || epi == UVC_EPI_BIAS || epi == UVC_EPI_BIAS_RESID || epi == UVC_EPI_BIAS_RESID_GATE || epi == UVC_EPI_BIAS_GELU_GRAD ||
         epi == UVC_EPI_MUL_AUX;
}
// k_gemm_row384_lnbwd<.., 1> addresses A with 32-bit buffer offsets, the ragged last tile's 128 rows past M included: below 2 GB.  Shared by
// uvc_gemm_nt_ln_supported and row384_fwd_ok, so the predicate never promises a problem the call refuses
bool row384_fwd_fits(int64_t M, int64_t K) { return (M + 128) * K * 2 < (1ll << 31); }
// uvc_gemm_nt with ln_out at N = 384 (bf16 operands, residual rows and outputs; K a multiple of 64, >= 128)
bool row384_fwd_ok(const NtArgs& a, int epi) {
  return a.N == R3_BN && a.K % 64 == 0 && a.K >= 128 && a.lda == a.K && a.ldb == a.K && a.ldc == R3_BN && a.ldr == R3_BN &&
         epi_resid(epi) && (((uintptr_t)a.A | (uintptr_t)a.B | (uintptr_t)a.C | (uintptr_t)a.R | (uintptr_t)a.ln_out) & 15) == 0 &&
         row384_fwd_fits(a.M, a.K);
}
// the two wide-tile LDS-DMA kernels: bf16 operands, 64-deep k tiles, 16-byte aligned rows, operands below 2 GB (32-bit buffer offsets; k_gemm_nt8p
// requests up to 256 rows past the edge)
bool wide_ok(const NtArgs& a, bool a_f32, int past) {
  return !a_f32 && a.K % 64 == 0 && a.K >= 256 && a.N >= 256 && a.lda % 8 == 0 && a.ldb % 8 == 0 && (((uintptr_t)a.A | (uintptr_t)a.B) & 15) == 0 &&
         (size_t)(a.M + past) * a.lda * 2 < (1ull << 31) && (size_t)(a.N + past) * a.ldb * 2 < (1ull << 31);
}
// k_gemm_nt256 by shape: at least 640 tiles (under ~3 rounds of the 256 persistent workgroups the partly filled last round costs more than the kernel gains)
bool nt256_ok(const NtArgs& a, bool a_f32, bool any_size) {
  const int tiles = ceil_div(a.M, G2_BM) * ceil_div(a.N, G2_BN);
  return (any_size || (tiles >= 640 && a.M >= 2048)) && wide_ok(a, a_f32, 0);
}
bool nt8p_ok(const NtArgs& a, bool a_f32) { return wide_ok(a, a_f32, 256); }
// k_gemm_nt8p's rows per tile / 32: the height (of 256 / 192 / 160 / 128) with the least work in the longest-running workgroup.  Tile time ~ a + b * rows with
// a / b = 8 row blocks (M = 25 216, N = 768: 189 / 150 / 137 / 169 us for ri 8 / 6 / 5 / 4)
int nt8p_pick_ri(int M, int N) {
  const int tn = ceil_div(N, 256);
  int best = 8; long best_cost = -1;
  const int cand[4] = {8, 6, 5, 4};
  for (int ri : cand) {
    const long tiles = (long)ceil_div(M, 32 * ri) * tn;
    const long cost = (tiles + 255) / 256 * (ri + 8);
    if (best_cost < 0 || cost < best_cost) { best = ri; best_cost = cost; }
  }
  return best;
}

const char* const NT_NO_LN = "uvc_gemm_nt: ln_out is not available for this problem (uvc_gemm_nt_ln_supported)";

int nt_route_ring(uvc_gemm_route* r, int kt, bool ln, int nst) {
  r->family = UVC_ROUTE_WSN16_DMA; r->kt = kt; r->ln = ln; r->nst = nst;
  return UVC_OK;
}
// N = 192 column-sliced.  16 rows per tile for float32 C and the residual epilogues (with 32 the two sub-tiles' residual prefetch spilled 24-45 VGPRs:
// 129 -> 88 us), 32 rows otherwise; the residual epilogues on the LDS-DMA ring at K = 768, and with ln_out at K = 512 / 256 too (UVC_NT_NO_DMA: never)
int nt_route_wsn(const NtArgs& a, int e, bool c_f32, uvc_gemm_route* r) {
  const int kt = a.K / 32;
  const bool rows16 = c_f32 || epi_resid(e);
  const bool dma = rows16 && kt != 18 && epi_resid(e) && (a.ln_out || kt == 24) && (!a.no_dma || a.ln_out) && wsn16_dma_ok(a) && (a.ln_out || a.M % 16 == 0);
  if (dma) return nt_route_ring(r, kt, a.ln_out != nullptr, kt == 8 ? 4 : 3);
  if (a.ln_out) return uvc_set_error_msg(UVC_ERR_UNSUPPORTED, NT_NO_LN);
  r->family = rows16 ? UVC_ROUTE_WSN16 : UVC_ROUTE_WSN; r->kt = kt;
  return UVC_OK;
}

// Every check of uvc_gemm_nt, then the family and template arguments of the kernel that runs the problem.  No HIP call; pointers are read as integers only.
// Precedence in bf16 mode: ln_out forms; K = N = 192 ring; row panels; K = 384 streaming; N = 192 column-sliced; forced 8-phase; 256 x 256; 8-phase for
// few wide tiles; K = 192 / 128 streaming; generic.
int nt_route(const uvc_gemm_nt_args& p, uvc_gemm_route* r) {
  *r = uvc_gemm_route{};
  if (!p.A || !p.B || !p.C) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_nt: null pointer");
  if (p.M <= 0 || p.N <= 0 || p.K <= 0) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_nt: empty problem");
  const int ch = (p.dtype == UVC_F32) ? 4 : 8;
  if (p.K % ch || p.lda % ch || p.ldb % ch) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_nt: K, lda, ldb must be multiples of a 16-byte chunk");
  const int e = p.epilogue, fg = p.force_generic;
  if ((e == UVC_EPI_BIAS || e == UVC_EPI_BIAS_GELU || e == UVC_EPI_BIAS_GELU_OUT || e == UVC_EPI_BIAS_RESID || e == UVC_EPI_BIAS_RESID_GATE ||
       e == UVC_EPI_BIAS_GELU_GRAD) && !p.bias)
    return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_nt: epilogue needs bias");
  if (epi_resid(e) && !p.R) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_nt: residual epilogue needs R");
  if (epi_resid(e) && (p.r_is_f32 != 0) != (p.c_is_f32 != 0 || p.dtype == UVC_F32))
    return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_nt: R / R2 have C's element type (r_is_f32 must equal c_is_f32)");
  if (e == UVC_EPI_BIAS_RESID_GATE && (!p.R2 || !p.gate)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_nt: gate epilogue needs R2 and gate");
  if ((e == UVC_EPI_BIAS_GELU || e == UVC_EPI_BIAS_GELU_GRAD) && !p.C2) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_nt: GELU epilogue needs C2");
  if ((e == UVC_EPI_DGELU || e == UVC_EPI_MUL_AUX || e == UVC_EPI_MUL_AUX_Q8) && !p.aux) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_nt: dGELU epilogue needs aux");
  const bool q8 = e == UVC_EPI_BIAS_GELU_GRAD_Q8 || e == UVC_EPI_MUL_AUX_Q8;
  if (e == UVC_EPI_BIAS_GELU_GRAD_Q8 && (!p.bias || !p.C2)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_nt: UVC_EPI_BIAS_GELU_GRAD_Q8 needs bias and C2");
  // the one-byte GELU' code exists in the streaming kernel of DeiT-Tiny's width only (uvc_gemm_nt_q8_supported): N here is the hidden width, K the embed_dim
  if (q8 && (fg == UVC_NT_GENERIC || p.a_is_f32 || p.c_is_f32 || p.ln_out || !uvc_gemm_nt_q8_supported(p.M, p.N, p.K, p.dtype) ||
             (p.ldaux ? p.ldaux : p.ldc) % 8 || p.ldc % 8 || p.ldb != p.K))
    return uvc_set_error_msg(UVC_ERR_UNSUPPORTED, "uvc_gemm_nt: the one-byte GELU' epilogues need bf16 A / C, K = 192, N % 256 == 0, M >= 4096 (uvc_gemm_nt_q8_supported)");
  const NtArgs a = nt_args(p);
  const bool generic = fg == UVC_NT_GENERIC, a_f32 = p.a_is_f32 != 0, c_f32 = p.c_is_f32 != 0;
  r->a_f32 = a_f32; r->c_f32 = c_f32; r->t_f32 = p.dtype == UVC_F32; r->epilogue = e;
  if (p.ln_out) {
    if (!p.ln_gamma || !p.ln_beta || (p.ln_mean != nullptr) != (p.ln_rstd != nullptr))
      return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_nt: ln_out needs ln_gamma, ln_beta (and ln_mean, ln_rstd together)");
    const bool ln_ok = uvc_gemm_nt_ln_supported(p.M, p.N, p.K, p.dtype, e) && !generic && !a_f32 && p.alpha == 1.0f && !p.alpha_ptr;
    if (p.N == 384) {
      if (!ln_ok || c_f32 || !row384_fwd_ok(a, e))
        return uvc_set_error_msg(UVC_ERR_UNSUPPORTED, "uvc_gemm_nt: ln_out is not available for this problem (uvc_gemm_nt_ln_supported; N = 384: bf16 C and R only)");
      r->family = UVC_ROUTE_ROW384;
      return UVC_OK;
    }
    if (!ln_ok || a.ldb != a.K || !wsn16_dma_ok(a) || ((uintptr_t)p.ln_out & 7) != 0) return uvc_set_error_msg(UVC_ERR_UNSUPPORTED, NT_NO_LN);
    if (p.M % 16 != 0 && (p.C == (const void*)p.R || p.C == (const void*)p.R2))
      return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_nt: with ln_out and M % 16 != 0 the last row tile is computed twice: C must not alias R / R2");
    if (p.K == 192) return nt_route_ring(r, 6, true, 7);       // attn.proj + residual -> norm2: 20-KB stages, seven of them
    return nt_route_wsn(a, e, c_f32, r);
  }
  if (p.dtype == UVC_F32) {
    if (!a_f32 || !c_f32) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_nt: float32 mode needs float32 A and C");
  } else if (p.dtype != UVC_BF16) {
    return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_nt: dtype must be UVC_F32 or UVC_BF16");
  } else if (!fg && !a_f32 && e == UVC_EPI_BIAS_RESID && p.K == 192 && p.N == 192 && a.ldb == 192 && p.M >= 4096 && p.M % 16 == 0 && p.alpha == 1.0f &&
             !p.alpha_ptr && wsn16_dma_ok(a)) {
    return nt_route_ring(r, 6, false, 7);                      // attn.proj + residual without ln_out: the same seven-stage ring
  } else if (!fg && a.ldr % 8 == 0 && a.ldaux % 8 == 0 && uvc_gemm_nt_rows_supported(a.M, a.N, a.K, a.lda, a.ldb, a.ldc, p.dtype, e)) {
    r->family = UVC_ROUTE_NT_ROWS;                             // few rows, whatever the widths (profiles/r7a_ab_parent_new.txt)
    return UVC_OK;
  } else {
    const int vn = c_f32 ? 4 : 8;
    const bool ws = !generic && ws_ok(a, vn);
    if (q8 && !ws) return uvc_set_error_msg(UVC_ERR_UNSUPPORTED, "uvc_gemm_nt: the one-byte GELU' epilogues exist in the K = 192 streaming kernel only");
    // eight waves x 32 columns where N is a multiple of 128 from 512 up: two waves on every SIMD, 6-15 % faster than six (UVC_NT_WS384_SIX_WAVES: the A/B)
    if (!generic && ws384_ok(a, e, vn, a_f32)) {
      r->family = UVC_ROUTE_WS384; r->kt = 12; r->nj = 2;
      r->nw = (!c_f32 && a.N % 128 == 0 && a.N >= 512 && fg != UVC_NT_WS384_SIX_WAVES) ? 8 : 6;
    } else if (!generic && wsn_ok(a, e, a_f32)) {
      return nt_route_wsn(a, e, c_f32, r);
    } else if ((fg >> 8) == 1) {                               // UVC_NT_8PHASE | ri
      if (!nt8p_ok(a, a_f32)) return uvc_set_error_msg(UVC_ERR_UNSUPPORTED, "uvc_gemm_nt: shape not taken by the 8-phase kernel");
      r->family = UVC_ROUTE_NT8P; r->ri = fg & 255;
    } else {
      // Wide GEMMs.  >= 640 tiles of 256 x 256 (qkv, fc1, dfc2 of DeiT-Base): k_gemm_nt256, 88 against 98 us for qkv.  Fewer tiles with N % 256 == 0 (N = 768:
      // 297 tiles are two rounds at 58 %): k_gemm_nt8p at the height that fills its rounds -- fc2 153 -> 137 us, dfc1 129 -> 95, dqkv 98 -> 74 against 128 x 128.
      // UVC_NT_WIDE_ANY_SIZE keeps that split at any row count: N < 1792 is what stays below 640 tiles at DeiT-Base's 25 216 rows
      const bool dma = !generic && !a.no_dma;
      const bool few_tiles_wide = !c_f32 && a.N % 256 == 0 && nt8p_ok(a, a_f32);
      if (dma && !(fg == UVC_NT_WIDE_ANY_SIZE && few_tiles_wide && a.N < 1792) && nt256_ok(a, a_f32, fg == UVC_NT_WIDE_ANY_SIZE || fg == UVC_NT_256_ANY_SIZE)) {
        r->family = UVC_ROUTE_NT256;
      } else if (dma && few_tiles_wide && (a.M >= 2048 || fg == UVC_NT_WIDE_ANY_SIZE)) {
        r->family = UVC_ROUTE_NT8P;
      } else {
        if (a_f32 && p.lda % 8 != 0) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_nt: lda");
        if (ws) {
          // bf16 A and C, N % 256 == 0, K = 192, the backward's multiplying epilogues: eight waves x 32 columns (95 -> 83 us, 118 -> 105); else four waves x 64
          // columns where N divides (more waves per CU to overlap the GELU epilogues), three otherwise
          const bool narrow = !a_f32 && !c_f32 && a.N % 256 == 0 && a.K == 192 && (e == UVC_EPI_DGELU || e == UVC_EPI_MUL_AUX || e == UVC_EPI_MUL_AUX_Q8);
          r->family = UVC_ROUTE_WS; r->kt = a.K == 192 ? 6 : 4; r->nw = narrow ? 8 : a.N % 256 == 0 ? 4 : 3; r->nj = narrow ? 2 : 4;
        }
      }
    }
  }
  if (r->family == UVC_ROUTE_NT8P) {                           // float32 C: the 256-row tile only
    if (r->ri <= 0) r->ri = nt8p_pick_ri(a.M, a.N);
    r->ri = c_f32 ? 8 : (r->ri == 8 || r->ri == 6 || r->ri == 5) ? r->ri : 4;
  }
  // (the row-panel, column-sliced and ring families have checked their epilogues above)
  if (e < UVC_EPI_NONE || (e > UVC_EPI_MUL_AUX && !q8)) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_nt: unknown epilogue");
  return UVC_OK;
}

}  // namespace

extern "C" int uvc_gemm_nt_ln_supported(int32_t M, int32_t N, int32_t K, int32_t dtype, int32_t epilogue) {
  // N = 384: k_gemm_row384_lnbwd<.., 1>, bf16 C / R only; its rows are bit-identical to the unfused pair, so the row threshold does not show in results
  if (dtype == UVC_BF16 && N == 384) return M >= 4096 && K % 64 == 0 && K >= 384 && epi_resid(epilogue) && row384_fwd_fits(M, K);
  if (dtype != UVC_BF16 || N != 192 || M < 16) return 0;      // any row count from 16 up: whether norm is fused must not depend on the batch
  return ((K == 768 || K == 512 || K == 256) && epi_resid(epilogue)) || (K == 192 && epilogue == UVC_EPI_BIAS_RESID);
}

extern "C" int uvc_gemm_nt_q8_supported(int32_t M, int32_t hidden, int32_t embed_dim, int32_t dtype) {
  return dtype == UVC_BF16 && embed_dim == 192 && hidden > 0 && hidden % 256 == 0 && M >= 4096;
}

extern "C" int uvc_gemm_nt_rows_supported(int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldb, int32_t ldc, int32_t dtype, int32_t epilogue) {
  return dtype == UVC_BF16 && M >= 1 && M <= RP_MAX_M && K >= 8 && K <= RP_MAX_K && K % 8 == 0 && N >= 8 && N % 8 == 0 && lda >= K && ldb >= K && ldc >= N &&
         lda % 8 == 0 && ldb % 8 == 0 && ldc % 8 == 0 && nt_rows_epilogue(epilogue);
}

extern "C" int uvc_gemm_nt_route(const uvc_gemm_nt_args* p, uvc_gemm_route* r) {
  if (!p || !r) return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_nt: null pointer");
  return nt_route(*p, r);
}

extern "C" int uvc_gemm_nt(const uvc_gemm_nt_args* p, void* stream) {
  uvc_gemm_route r;
  if (const int rc = uvc_gemm_nt_route(p, &r)) return rc;
  const NtArgs a = nt_args(*p);
  hipStream_t st = (hipStream_t)stream;
  switch (r.family) {
    case UVC_ROUTE_NT: return uvc_gemm::launch_nt(r, a, st);
    case UVC_ROUTE_NT_ROWS: return uvc_gemm::launch_nt_rows(r, a, st);
    case UVC_ROUTE_WS: return uvc_gemm::launch_ws(r, a, st);
    case UVC_ROUTE_WS384: return uvc_gemm::launch_ws384(r, a, st);
    case UVC_ROUTE_WSN:
    case UVC_ROUTE_WSN16: return uvc_gemm::launch_wsn(r, a, st);
    case UVC_ROUTE_WSN16_DMA: return uvc_gemm::launch_ring(r, a, st);
    case UVC_ROUTE_ROW384: return uvc_gemm::launch_row384_fwd(a, r.epilogue, st);
    case UVC_ROUTE_NT256: return uvc_gemm::launch_nt256(r, a, st);
    case UVC_ROUTE_NT8P: return uvc_gemm::launch_nt8p(r, a, st);
    default: return uvc_set_error_msg(UVC_ERR_ARG, "uvc_gemm_nt: route");
  }
}

static const char* const UVC_ROUTE_KERNELS[UVC_ROUTE_COUNT] = {
    "k_gemm_nt", "k_gemm_nt_rows", "k_gemm_ws", "k_gemm_ws", "k_gemm_wsn", "k_gemm_wsn16", "k_gemm_wsn16_dma", "k_gemm_row384_lnbwd", "k_gemm_nt256", "k_gemm_nt8p",
    "k_gemm_tn", "k_gemm_tn_big", "k_gemm_tn_dma", "k_gemm_tn8p"};
extern "C" const char* uvc_gemm_route_kernel(int32_t family) { return family >= 0 && family < UVC_ROUTE_COUNT ? UVC_ROUTE_KERNELS[family] : nullptr; }
