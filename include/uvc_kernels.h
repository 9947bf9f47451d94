/* C-ABI of the DeiT Stage-1 compute kernels on MI355X (libuvc_hip.so): MFMA GEMMs with fused
 * epilogues, LayerNorm, fused attention, distillation loss, fused clip+AdamW, token/gate helpers.
 *
 * The reference reaches these through ATen/cuBLAS/cuDNN from UVC/models/model_distilled.py,
 * UVC/utils/losses.py and torch.optim; it has no operator/FFI layer of
 * its own, so each entry point cites the reference lines whose arithmetic it performs.
 *
 * Conventions as in uvc_engine.h: device pointers owned by the caller, no allocation, no host
 * sync, `stream` is a hipStream_t, int status return (0 = ok; uvc_last_error()).
 * dtype selects the arithmetic: UVC_F32 = float32 storage + v_mfma_f32_16x16x4_f32 (exact fmaf
 * chain; the 1e-3 parity mode), UVC_BF16 = bfloat16 operands + v_mfma_f32_16x16x32_bf16 with
 * float32 accumulation (the throughput mode).  "T" below means float or bfloat16 accordingly.
 */
#ifndef UVC_KERNELS_H
#define UVC_KERNELS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { UVC_F32 = 0, UVC_BF16 = 1 };

enum {
  UVC_EPI_NONE = 0,            /* C = alpha*acc                                                        */
  UVC_EPI_BIAS = 1,            /* C = alpha*acc + bias[n]                       (nn.Linear)            */
  UVC_EPI_BIAS_GELU = 2,       /* C = a = acc + bias ; C2 = GELU_erf(a)         (Mlp fc1+act, :116-118) */
  UVC_EPI_BIAS_RESID = 3,      /* C = acc + bias + R[m,n]                       (x + proj(...), :240)   */
  UVC_EPI_BIAS_RESID_GATE = 4, /* C = g1*(acc + bias + R[m,n]) + g0*R2[m,n]     (:244 then :493)        */
  UVC_EPI_DGELU = 5,           /* C = alpha*acc * GELU'(aux[m,n])               (backward of :118)      */
  UVC_EPI_BIAS_GELU_OUT = 6,   /* C = GELU_erf(acc + bias)   (inference: pre-activation not kept)        */
  UVC_EPI_BIAS_GELU_GRAD = 7,  /* a = acc + bias ; C = GELU'(a) ; C2 = GELU_erf(a): training forward of fc1 -- the backward
                                  needs the pre-activation only through GELU'(a), so that is what is kept            */
  UVC_EPI_MUL_AUX = 8,         /* C = alpha*acc * aux[m,n]   (backward of the activation with aux = stored GELU'(a)) */
  /* r6: GELU'(a) in ONE byte.  The backward needs the fc1 pre-activation only through GELU'(a), a BOUNDED quantity ([-0.1290, 1.1290]), and fc1 + GELU, GELU'
   * is write-bound (profiles/r6b_bound_probes.txt: the step is 3.2 % faster with that tensor not written at all).  Uniform code over [UVC_Q8_LO, UVC_Q8_LO +
   * 255 UVC_Q8_STEP] = [-0.13, 1.13]:  q = min(255, trunc(max(0, (GELU' - LO) / STEP + 0.5))),  GELU' ~ LO + q STEP,  |error| <= STEP / 2 = 2.47e-3 everywhere --
   * finer than bf16 where GELU' >= 0.5 (bf16 spacing 3.9e-3 on [0.5, 1), 7.8e-3 on [1, 2)), coarser only where GELU' is small and weighs least; relative L2
   * error of dA / dW1 / dh against float64 2.0e-3 - 2.6e-3 against 1.6e-3 - 2.0e-3 for bf16 GELU' (tools/gelu_grad_codes.py, profiles/r6_gelu_grad_codes_cpu.txt).
   * bf16 compute, K = 192, N % 256 == 0, M >= 4096 (uvc_gemm_nt_q8_supported): the streaming kernel of DeiT-Tiny's width; UVC_ERR_UNSUPPORTED elsewhere. */
  UVC_EPI_BIAS_GELU_GRAD_Q8 = 9,  /* a = acc + bias ; C [M, N] BYTES (ldc in bytes = elements) = code(GELU'(a)) ; C2 = GELU_erf(a) (T)          */
  UVC_EPI_MUL_AUX_Q8 = 10         /* C = alpha*acc * (LO + STEP * aux[m,n]),  aux [M, N] bytes (ldaux in elements) written by _GELU_GRAD_Q8      */
};
#define UVC_Q8_LO (-0.13f)
#define UVC_Q8_STEP (1.26f / 255.0f)

/* uvc_gemm_nt_args.force_generic.  Every choice computes the same bits (one k-ordered accumulation chain, the same epilogue arithmetic).  Only
 * UVC_NT_BY_SHAPE is a product setting; the others exist for tests and tuning tools (uvc_vit_cfg.force_generic passes 1, 2 and 3 to a whole pass). */
enum {
  UVC_NT_BY_SHAPE = 0,         /* the kernel is picked by shape (uvc_gemm_nt_route tells which)                                                        */
  UVC_NT_GENERIC = 1,          /* tests: the generic LDS-tiled 128 x 128 kernel, the reference every other kernel must match bit for bit; ln_out and the
                                  one-byte GELU' epilogues are UVC_ERR_UNSUPPORTED                                                                     */
  UVC_NT_NO_DMA = 2,           /* tests: no LDS-DMA kernel -- the N = 192 residual epilogues on the register-staged k_gemm_wsn16 (ln_out still takes the
                                  ring), no 256 x 256 and no 8-phase kernel; the K = N = 192 ring and the row panels are skipped as for any value but 0  */
  UVC_NT_WIDE_ANY_SIZE = 3,    /* tests: the wide-tile kernels wherever the shape admits them, whatever the row / tile count, split as the production
                                  batch of DeiT-Small / Base splits them: 8-phase where N % 256 == 0 and N < 1792 (bf16 C), else 256 x 256              */
  UVC_NT_256_ANY_SIZE = 4,     /* tests / tools: the 256 x 256 kernel wherever the shape admits it, whatever the row / tile count                        */
  UVC_NT_WS384_SIX_WAVES = 5,  /* tools (A/B): the K = 384 streaming kernel in its six-wave form where eight waves are the default                        */
  UVC_NT_8PHASE = 0x100        /* tests / tools: UVC_NT_8PHASE | ri = the 8-phase kernel at 32 * ri rows per tile (ri of 8, 6, 5, 4; 0 = the height picked
                                  by shape; float32 C: 8), at any size; UVC_ERR_UNSUPPORTED where the shape is not taken.  The K = 384 and N = 192
                                  streaming kernels still come first                                                                                    */
};

/* C[M,N] = epilogue( A[M,K] . B[N,K]^T ); A, B row-major with K contiguous. */
typedef struct uvc_gemm_nt_args {
  const void* A;       /* [M,K]  T, or float32 when a_is_f32 (converted to T while staging) */
  const void* B;       /* [N,K]  T */
  void* C;             /* [M,N]  T, or float32 when c_is_f32 */
  void* C2;            /* second output of UVC_EPI_BIAS_GELU / _GELU_GRAD, same type/ld as C */
  const float* bias;   /* [N] */
  const void* R;       /* [M,N] residual rows, element type of C (float32 stream: c_is_f32; bf16 stream: C, R, R2 all bf16) */
  const void* R2;      /* [M,N] gate epilogue, same type */
  const void* aux;     /* [M,N] T: pre-activation for UVC_EPI_DGELU, multiplier for UVC_EPI_MUL_AUX */
  const float* gate;   /* device float[2] = (g0, g1) block-gate distribution */
  const float* alpha_ptr; /* optional device scalar multiplied into alpha */
  float alpha;
  int32_t M, N, K, lda, ldb, ldc, ldr, ldaux;
  int32_t dtype, a_is_f32, c_is_f32, epilogue;
  int32_t force_generic;  /* tests / tuning: one of the UVC_NT_* values above; 0 in the product */
  int32_t r_is_f32;       /* element type of R / R2, stated by the caller and checked: they have C's type (c_is_f32, or float32 mode), so
                             this must equal it whenever R is given.  Rounds 1-2 took float32 R beside a bf16 C; a caller still built to
                             that contract gets UVC_ERR_ARG instead of its rows read as bf16 */
  /* optional second output of the residual epilogues where uvc_gemm_nt_ln_supported(): ln_out[M,N] (T) = LayerNorm(C rows; ln_gamma,
   * ln_beta, ln_eps) -- norm1 of the next block on the rows fc2 + residual (+ gate mix) just produced (model_distilled.py:241-244) --
   * and its float32 statistics ln_mean / ln_rstd [M] (both or neither).  Needs alpha == 1, contiguous A / R (lda == K, ldr == N).
   * With a bf16 C the LayerNorm is taken of the ROUNDED rows (what C holds).  At N = 384 the fused kernel addresses A with 32-bit
   * offsets: uvc_gemm_nt_ln_supported() is 0 once (M + 128) * K * 2 >= 2^31, and callers run the GEMM and uvc_layernorm_fwd apart.
   * Above that bound the rows come from another GEMM kernel and can differ from the fused form's in the last bit. */
  float ln_eps;
  const float* ln_gamma; const float* ln_beta; void* ln_out; float* ln_mean; float* ln_rstd;
} uvc_gemm_nt_args;
int uvc_gemm_nt(const uvc_gemm_nt_args* args, void* stream);
int uvc_gemm_nt_ln_supported(int32_t M, int32_t N, int32_t K, int32_t dtype, int32_t epilogue);
/* 1 where UVC_EPI_BIAS_GELU_GRAD_Q8 (N = hidden width, K = embed_dim) AND its partner UVC_EPI_MUL_AUX_Q8 (N and K swapped roles: [M, K'] x [N', K'] with
 * K' = embed_dim) exist: bf16, embed_dim 192, hidden % 256 == 0, M >= 4096.  Callers fall back to UVC_EPI_BIAS_GELU_GRAD / UVC_EPI_MUL_AUX elsewhere. */
int uvc_gemm_nt_q8_supported(int32_t M, int32_t hidden, int32_t embed_dim, int32_t dtype);
/* 1 where uvc_gemm_nt (force_generic = 0, no ln_out) runs the row-panel kernel (16 rows x 64 columns per workgroup, the wave's fragments of 512 elements
 * of K requested at once): bf16 compute, 1 <= M <= 1024, 8 <= K <= 1024, K % 8 == 0, N % 8 == 0, lda / ldb / ldc multiples of 8 (ldr and ldaux too),
 * epilogue one of UVC_EPI_NONE, _BIAS, _BIAS_RESID, _BIAS_RESID_GATE, _BIAS_GELU_GRAD, _MUL_AUX; A and C bf16 or float32.  Same bits as every other route. */
int uvc_gemm_nt_rows_supported(int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldb, int32_t ldc, int32_t dtype, int32_t epilogue);

/* uvc_gemm_tn_args.variant.  Only UVC_TN_BY_SHAPE is a product setting. */
enum {
  UVC_TN_BY_SHAPE = 0,   /* kernel picked by shape: the two-group schedule (k_gemm_tn8p) for every 192- / 256-wide tile but the 96 x 192 one             */
  UVC_TN_BY_SHAPE_1 = 1, /* the same as 0 (once the two-group schedule's opt-in; kept because tests and tools pass it)                                   */
  UVC_TN_RING = 2,       /* tests / tools: the LDS-DMA ring kernel (k_gemm_tn_dma) for the 192 x 192, 192 x 256 and 256 x 192 tiles: the same bits        */
  UVC_TN_128X256 = 3     /* tools (A/B): 128 x 256 tiles where the shape takes 256 x 256 (half the splits: another summation order)                       */
};

/* C[N1,N2] = beta*C + alpha * A[M,N1]^T . B[M,N2]  (weight gradients; float32 C).
 * Deterministic: M is cut into slices reduced in a fixed order through `workspace`. */
typedef struct uvc_gemm_tn_args {
  const void* A;       /* [M,N1] T, or float32 when a_is_f32 */
  const void* B;       /* [M,N2] T */
  float* C;            /* [N1,N2] float32 */
  void* workspace;     /* >= uvc_gemm_tn_workspace_bytes() */
  int64_t workspace_bytes;
  const float* alpha_ptr;
  float* colsum_out;   /* optional [N1]: beta*old + alpha * column sums of A (the bias gradient, same pass) */
  float alpha, beta;
  int32_t M, N1, N2, lda, ldb, ldc;
  int32_t dtype, a_is_f32;
  int32_t variant;     /* tests / tuning: one of the UVC_TN_* values above; 0 in the product */
} uvc_gemm_tn_args;
int uvc_gemm_tn(const uvc_gemm_tn_args* args, void* stream);
int uvc_gemm_tn_workspace_bytes(int32_t M, int32_t N1, int32_t N2, int64_t* bytes, int32_t* splits);

/* Which kernel uvc_gemm_nt / uvc_gemm_tn run for a problem, without running it (for tests: no HIP call, pointer members are read as integers only --
 * null, alignment, aliasing).  uvc_gemm_nt_route / uvc_gemm_tn_route make every check of their entry point and return its status; the entry points
 * call them and launch what they return. */
enum {
  UVC_ROUTE_NT = 0,        /* k_gemm_nt<TA, T, TC, EPI>: the generic 128 x 128 kernel                                  */
  UVC_ROUTE_NT_ROWS,       /* k_gemm_nt_rows<TA, TC, EPI>: row panels, M <= 1024 (uvc_gemm_nt_rows_supported)          */
  UVC_ROUTE_WS,            /* k_gemm_ws<TA, TC, EPI, kt, nw, nj>: K = 192 / 128 streaming                              */
  UVC_ROUTE_WS384,         /* k_gemm_ws<bf16, TC, EPI, 12, nw, 2>: K = 384 streaming                                   */
  UVC_ROUTE_WSN,           /* k_gemm_wsn<TC, EPI, kt>: N = 192 column-sliced, 32-row tiles                             */
  UVC_ROUTE_WSN16,         /* k_gemm_wsn16<TC, EPI, kt>: the same on 16-row tiles, register-staged                     */
  UVC_ROUTE_WSN16_DMA,     /* k_gemm_wsn16_dma<EPI, kt, ln, nst, !c_f32>: N = 192 residual epilogues on the LDS-DMA ring */
  UVC_ROUTE_ROW384,        /* k_gemm_row384_lnbwd<true, 1>: N = 384 with ln_out                                        */
  UVC_ROUTE_NT256,         /* k_gemm_nt256<TC, EPI>: 256 x 256 tiles                                                   */
  UVC_ROUTE_NT8P,          /* k_gemm_nt8p<TC, EPI, ri>: (32 ri) x 256 tiles, 8-phase schedule                          */
  UVC_ROUTE_TN,            /* k_gemm_tn<TA, T>: 128 x 64 tiles (cfg 0)                                                 */
  UVC_ROUTE_TN_BIG,        /* k_gemm_tn_big<float, b1, b2, ..>: float32 A                                              */
  UVC_ROUTE_TN_DMA,        /* k_gemm_tn_dma<b1, b2, ..>: LDS-DMA ring                                                  */
  UVC_ROUTE_TN8P,          /* k_gemm_tn8p<b1 / 32, b2 / 64>: two-group schedule                                        */
  UVC_ROUTE_COUNT
};
typedef struct uvc_gemm_route {
  int32_t family;                /* UVC_ROUTE_* */
  int32_t a_f32, t_f32, c_f32;   /* TA, T (the compute type: dtype == UVC_F32), TC are float (1) or bf16 (0) */
  int32_t epilogue;              /* EPI (NT) */
  int32_t kt, nw, nj;            /* k_gemm_ws / wsn / wsn16 / wsn16_dma: K / 32; k_gemm_ws: waves, 16-column blocks per wave */
  int32_t ln, nst;               /* k_gemm_wsn16_dma: LayerNorm output, ring stages */
  int32_t ri;                    /* k_gemm_nt8p: rows per tile / 32 */
  int32_t cfg, b1, b2, splits, rows_per_split;   /* TN: tile configuration 0-6, tile, M slices and their length */
} uvc_gemm_route;
int uvc_gemm_nt_route(const uvc_gemm_nt_args* args, uvc_gemm_route* route);
int uvc_gemm_tn_route(const uvc_gemm_tn_args* args, uvc_gemm_route* route);
/* the kernel template's name of a UVC_ROUTE_* family, e.g. "k_gemm_wsn16_dma" (NULL outside the enum) */
const char* uvc_gemm_route_kernel(int32_t family);

/* Fused softmax(q k^T * scale) v for one DeiT sequence per (batch, head)
 * (UVC/models/model_distilled.py:175-185).  qkv is the packed Linear(dim, 3*dim) output
 * [B, N, 3, H, 64]; o is [B, N, H*64]; lse/delta are float32 [B, H, N].  N <= 1026, head_dim = 64
 * (N > 256: streaming kernels, K / V or Q / dO tiles through LDS; the one-pass backward, variant 2, is not among them). */
typedef struct uvc_attn_args {
  const void* qkv;   /* T */
  void* o;           /* T  (forward output; backward input) */
  float* lse;        /* log-sum-exp of the scaled scores (forward output; backward input) */
  const void* dout;  /* T  [B,N,H*64]      backward only */
  void* dqkv;        /* T  [B,N,3,H,64]    backward output */
  float* delta;      /* scratch [B,H,N]    backward only */
  int32_t B, N, H, head_dim, dtype;
  float scale;
  const int32_t* head_keep;  /* optional device [H].  Forward: heads with 0 are skipped and their slice of o is written as zeros.
                                For inference on a pruned model whose attn.proj input columns of that head are all zero (masked),
                                which makes the skip exact.  Not for training: the reference's clip norm includes the gradients of
                                masked proj columns, which need the head's output.
                                Backward: dq / dk / dv of heads with 0 are written as zeros without being computed -- exact when dout is
                                zero on the head's 64 columns, i.e. when attn.proj's input columns of that head are zero in the weights
                                the dgrad used (Stage-2 masked fine-tuning): the whole dqkv then carries the bits of the call without the
                                table.  Only the value 0 skips a head; any other value keeps it, and a kept head's o, lse, dq, dk, dv and
                                delta carry the bits they have without the table.
                                lse (forward) and delta (backward) of a head with 0 are NOT WRITTEN, in any kernel family (short, persistent,
                                dq + dk/dv pair, one-pass, streaming): the caller's bytes stay (tests/test_attention_head_keep_gpu.py) */
  int32_t variant;   /* backward, tuning / A-B: 0 = kernel picked by shape (bf16, 193 <= N <= 200, B * H >= 1024: the one-pass persistent kernel
                        k_attn_bwd_one, otherwise the dq + dk/dv pair); 1 = the pair; 2 = the one-pass kernel or UVC_ERR_UNSUPPORTED */
  int32_t grid;      /* backward, one-pass kernel: 0 = one persistent workgroup per CU; > 0 = that many (tests: several heads per workgroup
                        at small B * H) */
  int32_t v_dim;     /* uvc_attention_fwd (and uvc_attention_bwd_vdim below) only.  0: the layout above.  16 / 32 / 48 / 64: a compact model's value head dim -- qkv rows [B, N, H*64 (q) | H*64 (k) |
                        H*v_dim (v)], o [B, N, H*v_dim], lse as above; q / k keep 64 dims.  64 is the layout above and runs its kernels.  Other values:
                        UVC_ERR_ARG; with uvc_attention_bwd or head_keep: UVC_ERR_UNSUPPORTED */
} uvc_attn_args;
int uvc_attention_fwd(const uvc_attn_args* args, void* stream);
int uvc_attention_bwd(const uvc_attn_args* args, void* stream);
/* The backward of uvc_attention_fwd at a value width (training a compact model): v_dim must be 16, 32, 48 or 64, the layout is the forward's --
 * qkv and dqkv rows [q H*64 | k H*64 | v H*v_dim], o and dout [B, N, H*v_dim], lse / delta [B, H, N].  Always the dq + dk/dv kernel pair
 * (variant and grid are not read), deterministic, no atomics; every element of dqkv and delta is written.  At v_dim = 64 it launches the
 * kernels uvc_attention_bwd(variant = 1) launches.  head_keep set, or N > 256 (whatever v_dim): UVC_ERR_UNSUPPORTED. */
int uvc_attention_bwd_vdim(const uvc_attn_args* args, void* stream);

/* One step of attention rollout (Abnar & Zuidema 2020) seen from the readout token(s): a row vector over the tokens pushed back through one
 * attention block, r_out = keep * r_in + (mix / H) * sum_h P_h^T r_in, with P recomputed from q, k and the forward's lse -- no [N, N] matrix
 * exists anywhere.  1 <= N <= 1026 (UVC_ERR_UNSUPPORTED beyond), head_dim 64, v_dim 16 / 32 / 48 / 64 (it only sets the row stride), UVC_F32 or
 * UVC_BF16 operands; r and the sums are float32.  No atomics: every r_out element has one writer, the result is bit-identical on a repeat and
 * independent of the batch an image sits in.  Null pointers, overlapping r_in / r_out, a bad dtype or v_dim, an empty problem: UVC_ERR_ARG. */
typedef struct uvc_attn_rollout_args {
  const void* qkv;      /* T [B, N, H*(128 + v_dim)], rows [q H*64 | k H*64 | v H*v_dim] (the compact layout; v is not read) */
  const float* lse;     /* [B, H, N], as uvc_attention_fwd wrote it (natural log) */
  const float* r_in;    /* [B, N] */
  float* r_out;         /* [B, N], must not overlap r_in */
  int32_t B, N, H, head_dim, v_dim, dtype;
  float scale, keep, mix;
} uvc_attn_rollout_args;
/* r_out[b,j] = keep * r_in[b,j] + (mix / H) * sum_h sum_i r_in[b,i] * exp(scale * q[b,h,i].k[b,h,j] - lse[b,h,i]) */
int uvc_attention_rollout_step(const uvc_attn_rollout_args* a, void* stream);

/* One step of the gradient-weighted rollout (Chefer, Gur & Wolf, ICCV 2021, self-attention rule) seen from the readout token(s): the row vector
 * pushed back through (P . dP)^+ of one attention block, head mean, with dP = dO V^T the gradient of the explained logit with respect to the
 * softmax matrix.  P is recomputed from q, k and the forward's lse as in uvc_attention_rollout_step, dP per 16 x 16 tile from the streamed dO rows
 * and the keys' V rows (the second MFMA of the dK/dV kernel at a value width); the ReLU is per head and per entry, before the head mean; no
 * [N, N] matrix exists anywhere.  Limits as uvc_attention_rollout_step: 1 <= N <= 1026 (UVC_ERR_UNSUPPORTED beyond), head_dim 64 (otherwise
 * UVC_ERR_UNSUPPORTED), v_dim 16 / 32 / 48 / 64, UVC_F32 or UVC_BF16 operands; r, p, dP and the sums are float32.  No atomics: every r_out element
 * has one writer, the result is bit-identical on a repeat and independent of the batch an image sits in.  Null pointers, overlapping r_in /
 * r_out, a bad dtype or v_dim, an empty problem, qkv or dout not 16-byte aligned: UVC_ERR_ARG, and nothing is launched. */
typedef struct uvc_attn_relevance_args {
  const void* qkv;      /* T [B, N, H*(128 + v_dim)], rows [q H*64 | k H*64 | v H*v_dim] (the compact layout; v IS read) */
  const float* lse;     /* [B, H, N], as uvc_attention_fwd wrote it (natural log) */
  const void* dout;     /* T [B, N, H*v_dim]: the gradient at the attention output, before attn.proj */
  const float* r_in;    /* [B, N] */
  float* r_out;         /* [B, N], must not overlap r_in */
  int32_t B, N, H, head_dim, v_dim, dtype;
  float scale, keep, mix;
} uvc_attn_relevance_args;
/* r_out[b,j] = keep * r_in[b,j] + (mix / H) * sum_h sum_i r_in[b,i] * max(0, P_h[i,j] * (dout[b,i,h,:] . v[b,h,j,:])),
 * P_h[i,j] = exp(scale * q[b,h,i].k[b,h,j] - lse[b,h,i]) */
int uvc_attention_relevance_step(const uvc_attn_relevance_args* a, void* stream);

/* The qkv Linear and the attention forward of a block as ONE kernel (UVC/models/model_distilled.py:175-185: `self.qkv(x)` ... `attn @ v`):
 * h [B*N, D] (the LayerNorm-1 rows) and the qkv weight [3D, D] in, o [B,N,H*64] and lse out; qkv [B,N,3,H,64] is written only when the
 * pointer is given (the backward needs it; a no-grad forward does not).  Same bits as uvc_gemm_nt (UVC_EPI_BIAS) + uvc_attention_fwd.
 * Where uvc_qkv_attention_supported() (bf16, D = 64 H = 192 or 384, 193 <= N <= 208). */
typedef struct uvc_qkv_attn_args {
  const void* h;       /* T [B*N, D] */
  const void* w;       /* T [3D, D]   qkv weight, out-major (the bf16 shadow) */
  const float* bias;   /* [3D] or NULL */
  void* qkv;           /* T [B,N,3,H,64] or NULL */
  void* o;             /* T [B,N,H*64] */
  float* lse;          /* [B,H,N] or NULL */
  int32_t B, N, H, D, dtype;
  float scale;
  int32_t grid;        /* 0 = one persistent workgroup per CU (a workgroup takes (image, group of 3 heads) items); > 0 = that many (tests) */
} uvc_qkv_attn_args;
int uvc_qkv_attention_supported(int32_t B, int32_t N, int32_t H, int32_t D, int32_t dtype);
int uvc_qkv_attention_fwd(const uvc_qkv_attn_args* args, void* stream);

/* Attention of the first `ntok` query rows (class / distillation token) of every (image, head) against all N keys: what the LAST
 * block needs, whose other rows never reach the head (UVC/models/model_distilled.py:175-185 for rows 0 .. ntok-1, :507-526).
 * o / dout are the compact [B, ntok, H*64] rows; the backward recomputes the probabilities and writes the WHOLE dqkv
 * [B, N, 3, H, 64] (dq = 0 for the other rows, dk / dv dense).  ntok is 1 or 2, N <= 256, head_dim = 64. */
typedef struct uvc_attn_tok_args {
  const void* qkv;   /* T [B, N, 3, H, 64] */
  void* o;           /* T [B, ntok, H*64]  forward output */
  const void* dout;  /* T [B, ntok, H*64]  backward only */
  void* dqkv;        /* T [B, N, 3, H, 64] backward output */
  int32_t B, N, H, head_dim, ntok, dtype;
  float scale;
  const int32_t* head_keep;  /* optional device [H], forward and backward as in uvc_attn_args: the ntok rows of o, or all N rows of dq, dk, dv,
                                of a head with 0 are written as zeros.  These kernels have no lse or delta output, so a head with 0 writes
                                nothing else */
} uvc_attn_tok_args;
int uvc_attention_tok_fwd(const uvc_attn_tok_args* args, void* stream);
int uvc_attention_tok_bwd(const uvc_attn_tok_args* args, void* stream);

/* Copies `groups` blocks of `group_bytes` bytes: block g from src + g * src_group_stride to dst + g * dst_group_stride (all
 * multiples of 16 bytes).  Gathers the token rows of a [B, N, D] tensor into [B, ntok, D] (and scatters them back). */
int uvc_copy_row_groups(const void* src, void* dst, int64_t groups, int64_t group_bytes, int64_t src_group_stride, int64_t dst_group_stride,
                        void* stream);

/* nn.LayerNorm(D, eps) forward over `rows` rows (model_distilled.py:199,204,288; eps=1e-6 from
 * joint_train.py:138).  Row r of x starts at x + (r / rows_per_group) * group_stride + (r % rows_per_group) * D
 * (dense: rows_per_group = 1, group_stride = D; class/dist-token rows only: group_stride = N*D).
 * y is dense [rows, D] of type T (or float32 when y_is_f32); mean/rstd float32 [rows]. */
typedef struct uvc_ln_args {
  const void* x;        /* float32, or bf16 with x_lowp (the bf16 residual stream of the throughput mode) */
  const float* gamma; const float* beta;
  void* y; float* mean; float* rstd;
  /* backward */
  const void* dy;       /* dense [rows, D]; T, or float32 when dy_is_f32 */
  void* dx;             /* same row addressing as x; dx = LN'(dy) + a1*add1 + a2*add2; float32, or T when g_lowp */
  const void* add1; const float* a1;    /* optional dense-as-x addends (same element type as dx); a1/a2 device scalars (NULL = 1) */
  const void* add2; const float* a2;
  float* partial;       /* scratch [ln_bwd_blocks, 2*D + 2] */
  float* dgamma; float* dbeta;          /* [D], written as beta_acc*old + sum */
  float* dots;          /* optional [2]: { <dx, x>, <add2, x> } over all rows (gate-logit gradients) */
  float eps, beta_acc;
  int32_t rows, D, rows_per_group, dtype, y_is_f32, dy_is_f32;
  int64_t group_stride;
  int32_t g_lowp;       /* backward: the gradient stream (dx, add1, add2) is stored as T (bf16) instead of float32;
                           all arithmetic and the dots stay float32 */
  int32_t defer_reduce; /* backward: leave the per-block partials of dgamma / dbeta / dots in `partial` (one private region per
                           call) and skip the two small reduction launches; uvc_layernorm_bwd_reduce_batch finishes many calls at once */
  int32_t x_lowp;       /* x is stored as bf16 (statistics, normalisation and every sum stay float32) */
  int32_t reserved;
} uvc_ln_args;
/* one deferred uvc_layernorm_bwd call: its partial region and outputs (dots may be NULL) */
typedef struct uvc_ln_reduce_item { const float* partial; float* dgamma; float* dbeta; float* dots; int32_t nblocks; int32_t reserved; } uvc_ln_reduce_item;
/* finish up to 64 deferred LayerNorm backward calls (same D) in ONE launch; sums in a fixed order (deterministic);
 * outputs written as beta_acc*old + sum.  `items` is a HOST array. */
int uvc_layernorm_bwd_reduce_batch(const uvc_ln_reduce_item* items, int32_t n, int32_t D, float beta_acc, void* stream);
int uvc_layernorm_fwd(const uvc_ln_args* args, void* stream);
int uvc_layernorm_bwd(const uvc_ln_args* args, void* stream);
int uvc_layernorm_bwd_blocks(int32_t rows);
int uvc_layernorm_bwd_nblocks(int32_t rows);

/* dgrad GEMM with the LayerNorm backward as its epilogue (bf16 mode, D == 192, K in {576, 768}, M >= 4096): the backward of
 * `Linear(LayerNorm(x))` w.r.t. x, i.e. the pair uvc_gemm_nt(A, W -> dy) + uvc_layernorm_bwd(dy, x, ...) of
 * model_distilled.py:199-204,218-247's autograd without the [M, D] dy round trip through HBM:
 *     dy = A[M,K] . W[D,K]^T ;  dx = LN'(dy; x, mean, rstd, gamma) + a1*add1 + a2*add2   (dx, add1, add2: bf16 [M, D]; dx may alias add2)
 * dgamma / dbeta / { <dx,x>, <add2,x> } partials go to partial[uvc_gemm_lnbwd_nblocks(M)][2*D+2] (float32) and are finished by
 * uvc_layernorm_bwd_reduce_batch like a deferred uvc_layernorm_bwd call.  Deterministic (fixed summation orders). */
typedef struct uvc_gemm_lnbwd_args {
  const void* A; const void* W;                 /* bf16 [M,K], bf16 [D,K] (the W^T shadow of the Linear) */
  const void* x; const float* mean; const float* rstd; const float* gamma;    /* LayerNorm input [M,D] (float32, or bf16 with x_lowp) and saved statistics */
  const void* add1; const float* a1; const void* add2; const float* a2;       /* optional bf16 addends, device scalars (NULL = 1) */
  void* dx; float* partial;
  int32_t M, D, K, dtype;
  int32_t variant;      /* tests/tuning: 0 = LDS-DMA ring where the shape allows, 1 = the register-staged kernel */
  int32_t x_lowp;       /* 1: x is bf16 [M,D] (bf16 residual stream) instead of float32 */
} uvc_gemm_lnbwd_args;
int uvc_gemm_lnbwd_supported(int32_t M, int32_t D, int32_t K, int32_t dtype);
int uvc_gemm_lnbwd_nblocks(int32_t M);
int uvc_gemm_nt_lnbwd(const uvc_gemm_lnbwd_args* args, void* stream);

/* Fused MLP half of a block (model_distilled.py:107-124,199-204,241-247,493), bf16 mode, D == 192, F % 64 == 0:
 *     out = d1 * (x + fc2(GELU(fc1(LayerNorm(x))))) + d0 * x_prev           (gate = {d0, d1} device pair; NULL: out = x + mlp)
 * x, out, x_prev float32 [M, D]; w1 [F, D], w2 [D, F] are the bf16 weight shadows in their natural layouts; gamma/beta/b1/b2 float32.
 * Inference (teacher: utils/losses.py:47-49; eval): h = mean = rstd = gp = u = NULL, the [M, F] hidden activation never reaches memory.
 * Training: all five given -- the same pass stores what the backward reads: h = LayerNorm(x) (bf16 [M, D]), mean / rstd [M],
 * gp = GELU'(a) and u = GELU(a) (bf16 [M, F]); it replaces uvc_layernorm_fwd + two uvc_gemm_nt launches of the step. */
typedef struct uvc_mlp_args {
  const void* x; const float* gamma; const float* beta;
  const void* w1; const float* b1; const void* w2; const float* b2;
  void* out;
  int32_t M, D, F;
  float eps;
  const void* x_prev; const float* gate;
  void* h; float* mean; float* rstd; void* gp; void* u;
  /* optional: LayerNorm of the OUTPUT rows with the next block's norm1 parameters (model_distilled.py:241 of block l+1),
   * written as compute-dtype rows next_h [M,D] (+ float32 next_mean / next_rstd [M] for a backward) */
  const float* next_gamma; const float* next_beta; void* next_h; float* next_mean; float* next_rstd;
  int32_t rows_lowp;    /* 1: x, out and x_prev are bf16 rows (bf16 residual stream; out is rounded once, next_h is the LayerNorm of the rounded rows) */
  int32_t reserved;
} uvc_mlp_args;
int uvc_mlp_fused_supported(int32_t D, int32_t F, int32_t dtype);
int uvc_mlp_fused_fwd(const uvc_mlp_args* args, void* stream);

/* DistillationLoss over SoftTargetCrossEntropy (UVC/utils/losses.py:25-65, joint_train.py:940):
 * loss = (1-alpha) * mean_b sum_c -y log_softmax(o) + alpha * KL(softmax(t/T) || softmax(o_kd/T)) * T^2 / (B*C)   (kind 1, 'soft')
 *      = (1-alpha) * base + alpha * mean_b CE(o_kd, argmax_c teacher)                                            (kind 2, 'hard', :61-62)
 * All float32 [B,C].  Writes loss[0] and the gradients d_o, d_okd.  Aliasing of the gradient buffers:
 *  - o_kd != o and d_okd != d_o: d_o receives the base term's gradient and d_okd the distillation term's, separately;
 *  - o_kd == o with d_okd == d_o (enable_deit = 0, one head): d_o receives the sum of the two contributions;
 *  - o_kd != o with d_okd == d_o: the shared buffer receives the sum of d loss / d o and d loss / d o_kd.
 * (o_kd == o with a separate d_okd also leaves the sum in d_o, and d_okd is not written.)
 * kind 0: o_kd, teacher and d_okd are not read and may be NULL; alpha is taken as 0. */
typedef struct uvc_loss_args {
  const float* o; const float* o_kd; const float* y_soft; const float* teacher;
  float* loss; float* d_o; float* d_okd; float* row_scratch; /* [B] */
  float alpha, tau;
  int32_t B, C, kind; /* kind: 0 none, 1 soft, 2 hard */
} uvc_loss_args;
int uvc_distill_loss(const uvc_loss_args* args, void* stream);

/* Softmax + top-k of a batch of logits (python -m uvc_amd.compact predict).  logits float32 [B, ld]; the softmax runs over columns
 * [0, n_valid) only, so the padding logits of a head wider than its label set (the 16 / 104-wide CIFAR heads) take no part in the sum
 * and are never chosen.  probs float32 [B, k] receives the k largest probabilities of each row in descending order and index int32 [B, k]
 * their columns; equal values come out by ascending index.  The order is taken on the logits (the order of the exact probabilities);
 * prob = exp(logit - row max) / sum, in float32.  1 <= k <= min(n_valid, 16) and 1 <= n_valid <= ld, UVC_ERR_ARG otherwise.
 * One workgroup per row, fixed reduction trees, no atomics: the same bits on every run, and a row's result does not depend on B.
 * A NaN logit is never chosen; a row with fewer than k comparable logits reports index -1 and a NaN probability for the rest. */
int uvc_logits_topk(const float* logits, int32_t B, int32_t ld, int32_t n_valid, int32_t k, float* probs, int32_t* index, void* stream);

/* Perturbation tests of relevance maps (python -m uvc_amd.compact_perturb; Chefer, Gur & Wolf 2021, section 4): three kernels between two
 * forwards.  Each returns UVC_OK or refuses before anything is launched; no atomics, one writer per output element, the same bits on a
 * repeat and in any batch.
 *
 * uvc_patch_rank: the removal order of every image's patches.  scores float32 [B, ld]; the patches are columns [offset, offset + np), so a
 * [B, N] map over the tokens goes in as it is with offset = ntok.  rank int32 [B, np]: rank[b, p] = the number of patches of image b
 * that come before p.  descending = 1: j comes before p when s_j > s_p, or s_j == s_p and j < p; descending = 0: with <.  In both
 * directions -0 equals +0, a NaN comes after every number, and NaNs are ordered among themselves by index: every row of rank is a
 * permutation of 0 .. np - 1 whatever the input holds.  1 <= np (UVC_ERR_ARG), np <= 1024 (UVC_ERR_UNSUPPORTED), 0 <= offset and
 * offset + np <= ld (UVC_ERR_ARG).  One workgroup per image, sized by np.
 *
 * uvc_patch_rows_perturb: rows [B * np, width] of dtype (UVC_F32 / UVC_BF16, uvc_patchify's layout), counts device int32 [nsteps],
 * out [nsteps * B * np, width]: row (k, b, p) of out is row (b, p) of rows where rank[b, p] >= counts[k], else width elements of +0.0
 * (selected, not multiplied: a NaN or inf in a removed source row gives exact zeros).  A count outside [0, np] is clamped on the device.
 * Every source element is read once and written nsteps times; offsets are 64-bit.  16-byte loads and stores when width * sizeof(T) is a
 * multiple of 16 and rows and out are 16-byte aligned, element by element otherwise (any width, any element-aligned pointers).
 *
 * uvc_logits_target: logits float32 [rows, ld], target int32 [period] with rows % period == 0; row r reads target[r % period], clamped
 * into [0, n_valid).  prob[r] = exp(logit - row max) / sum over columns [0, n_valid) at the target, float32 arithmetic and reduction trees of
 * uvc_logits_topk; hit[r] = 1 when the target is the FIRST maximum of those columns, else 0.  1 <= n_valid <= ld. */
int uvc_patch_rank(const float* scores, int32_t B, int32_t ld, int32_t offset, int32_t np, int32_t descending, int32_t* rank, void* stream);
int uvc_patch_rows_perturb(const void* rows, const int32_t* rank, const int32_t* counts, int32_t nsteps, int32_t B, int32_t np, int32_t width,
                           int32_t dtype, void* out, void* stream);
int uvc_logits_target(const float* logits, int32_t rows, int32_t ld, int32_t n_valid, const int32_t* target, int32_t period, float* prob,
                      int32_t* hit, void* stream);

/* Pixel-resolution maps from the gradient of a class logit at the input (python -m uvc_amd.compact_pixel; uvc_vit_compact_input_grad of
 * uvc_vit.h hands out the gradient as patch rows): saliency, gradient x input and integrated gradients (Sundararajan, Taly & Yan, ICML 2017).
 * Bandwidth-bound kernels: every element is read once, 16-byte accesses where the row width and every pointer allow them and element by
 * element otherwise (any width, any element-aligned pointers), 64-bit offsets, no atomics -- every sum has a fixed order, the same bits
 * on a repeat.  Each returns UVC_OK or refuses before anything is launched.  "rows" are uvc_patchify's: [B * np, K0], K0 = C * P * P,
 * k = c * P * P + ky * P + kx, np = (S / P)^2.  dtype (UVC_F32 / UVC_BF16) is the element type T of x, x0 and uvc_ig_rows' out.
 *
 * uvc_unpatchify: rows float32 [B * np, K0] -> out float32 [B, C, S, S], the exact inverse of uvc_patchify (a copy: no arithmetic).  Any
 * P >= 1 with S % P == 0.
 *
 * uvc_ig_rows: the interpolated inputs of `count` steps of the midpoint rule: out[(s, b, p), :] = x0 + alpha_s * (x - x0),
 * alpha_s = (first_step + s + 0.5) / steps, s < count, as fmaf(alpha_s, x - x0, x0) in float32, rounded once to T.  x T [nrows, width];
 * x0 the same, or NULL for the zero baseline; out T [count * nrows, width].  0 <= first_step, first_step + count <= steps.
 *
 * uvc_ig_accumulate: acc float32 [n] = (first ? 0 : acc) + sum_{s < count} d_rows[s * n + i], s ascending (d_rows float32 [count, n]).
 *
 * uvc_pixel_maps: a float32 rows [B * np, K0] (a gradient, or uvc_ig_accumulate's sum); per element e = a * scale, or with x given
 * e = (a * (x - x0)) * scale, every step in float32 (x, x0 T rows; x0 NULL: zero).  pixel float32 [B, S, S] = sum_c |e|, channels ascending; patch float32 [B, np] =
 * the sum of |e| over the row and total float32 [B] = the signed sum of e over the image, both in fixed trees: one wave per row, a lane's
 * elements in ascending order, the wave butterfly; for the total a second launch sums the image's np row sums the same way, its waves in
 * order.  partial: float32 scratch [B * np].  Any of pixel / patch / total may be NULL (total needs partial).  x (and x0) are read
 * 8 bytes at a time in bf16, beside the 16 bytes of a. */
int uvc_unpatchify(const float* rows, float* out, int32_t B, int32_t C, int32_t S, int32_t P, void* stream);
int uvc_ig_rows(const void* x, const void* x0, void* out, int64_t nrows, int32_t width, int32_t first_step, int32_t count, int32_t steps,
                int32_t dtype, void* stream);
int uvc_ig_accumulate(const float* d_rows, float* acc, int64_t n, int32_t count, int32_t first, void* stream);
int uvc_pixel_maps(const float* a, const void* x, const void* x0, float scale, int32_t B, int32_t C, int32_t S, int32_t P, int32_t dtype,
                   float* pixel, float* patch, float* total, float* partial, void* stream);

/* Adversarial robustness of compact models (python -m uvc_amd.compact_robust): L-infinity FGSM and PGD (Goodfellow et al. 2015; Madry et
 * al. 2018) around uvc_vit_compact_loss_grad of uvc_vit.h.  Each call returns UVC_OK or refuses before anything is launched (outputs
 * untouched); no atomics, one writer per output element, fixed reduction trees: the same bits on a repeat and in any batch.
 *
 * uvc_loss_seed: the per-image attack loss and its gradient at the head outputs.  lg float32 [B, ld], lgd the same or NULL, labels int32
 * [B]; the eval logits are z = lg, or (lg + lgd) / 2 with lgd, over columns [0, n_valid), 1 <= n_valid <= ld.  A label is clamped into
 * [0, n_valid) on the device: callers check it on the host.  kind 0, cross-entropy: L = lse(z) - z_y, dz = softmax(z) - onehot(y), float32
 * arithmetic with the row maximum subtracted and uvc_logits_topk's reduction trees (a wave butterfly, then the waves in order); the mean of
 * the two heads and a logit's distance from the maximum are carried as exact float32 pairs (exp to second order in the small part) and the sum
 * of the exponentials is compensated,
 * so dz is within 4 float32 spacings of max(p, 2^-24) of the float64 value on the same float32 logits.  kind 1, margin: L = z_j - z_y,
 * dz = onehot(j) - onehot(y), j the FIRST maximum of the exact z over c != y; needs n_valid >= 2 (UVC_ERR_ARG).  dl = dz without lgd
 * (dld is not touched and may be NULL), dl = dld = dz / 2 with it; exact +0 in columns [n_valid, ld), which are never read.  loss float32
 * [B], or NULL.  One workgroup per image.
 *
 * uvc_pgd_step: one projected step on patch rows (uvc_patchify's layout, K0 = C * P * P, the channel of column k is k / (P * P)).
 * x (the iterate), x0 (the clean rows), dir and out float32 [rows, K0]; step, eps, lo, hi HOST float32 [C], C <= 4, eps >= 0, lo <= hi.
 * mode 0: d = (dir > 0) - (dir < 0) (a NaN or a zero of either sign gives 0); mode 1: d = dir (the random start: dir uniform in [-1, 1),
 * step = eps).  v = min(max(x + step_c * d, max(x0 - eps_c, lo_c)), min(x0 + eps_c, hi_c)), every operation a separate float32 operation
 * rounded once, min / max as torch.minimum / torch.maximum take them (a NaN operand is the result): the bits of that statement in
 * float32 PyTorch.  out = v and may be x itself; out_t T [rows, K0] (dtype UVC_F32 / UVC_BF16), or NULL: v rounded once to T, the rows the
 * next forward reads, made in the same pass.  Every element is read once; 16-byte loads and stores where P * P is a multiple of 4 (of 8
 * for the 16-byte bf16 store, else 8 bytes) and every pointer is aligned, element by element otherwise; offsets are 64-bit. */
int uvc_loss_seed(const float* lg, const float* lgd, const int32_t* labels, int32_t B, int32_t ld, int32_t n_valid, int32_t kind, float* dl,
                  float* dld, float* loss, void* stream);
int uvc_pgd_step(const float* x, const float* x0, const float* dir, int64_t rows, int32_t P, int32_t C, const float* step, const float* eps,
                 const float* lo, const float* hi, int32_t mode, float* out, void* out_t, int32_t dtype, void* stream);

/* Nearest neighbours in a feature bank and the weighted k-NN vote (python -m uvc_amd.compact_transfer; Wu et al. 2018, DINO's
 * knn_classifier).  Each call returns UVC_OK or refuses before anything is launched (outputs untouched); no atomics, every output
 * element has one writer, the same bits on a repeat.
 *
 * uvc_knn_topk: queries [nq, D] (row stride ldq) and bank [n, D] (row stride ldb), both UVC_BF16 or both UVC_F32 (q_dtype / bank_dtype;
 * a mix: UVC_ERR_UNSUPPORTED), row-major, pointers and row strides 16-byte aligned, strides >= D (UVC_ERR_ARG).  D a multiple of 8 in
 * [8, 1024] (UVC_ERR_UNSUPPORTED), 1 <= k <= 64, nq >= 1, n >= 1 (UVC_ERR_ARG); n is an int32, every byte offset is 64-bit.
 * s(q, x) = sum_d q_d x_d in float32, d ascending: exact products and float32 sums of v_mfma_f32_16x16x32_bf16 per 32 dims, or the fmaf
 * chain of v_mfma_f32_16x16x4_f32; nothing is normalised.  The value of a (query, bank row) pair does not depend on nq, n, the row's place
 * in the bank or the split count.  sims float32 [nq, k] and idx int32 [nq, k]: the k largest similarities of every query in descending
 * order, equal values by ascending bank row.  Lists start as (-inf, -1), the bank is visited in ascending row order and a similarity
 * enters a list only when it is strictly greater than the list's last entry: a NaN or -inf similarity never enters, +inf ranks first,
 * and with n < k the remaining slots stay (-inf, -1).  Bank rows past n are never read and masked to -inf; query rows past nq are never
 * stored.  One workgroup per 64 queries; splits > 1 divides the bank into that many contiguous row ranges over a second grid dimension
 * (partial lists in `workspace`, merged under the same order), splits = 0 chooses from the shapes and the device's CU count (split when
 * the query tiles are fewer than twice the CUs).  A request is clamped to [1, min(512, ceil(n / 64))]; every split count gives the same
 * bits.  uvc_knn_workspace_bytes: the bytes `workspace` needs for (nq, n, k, splits) -- 0 without a split -- and the split count used. */
typedef struct uvc_knn_args {
  const void* queries; const void* bank;
  float* sims; int32_t* idx;
  void* workspace; int64_t workspace_bytes;
  int64_t ldq, ldb;
  int32_t nq, n, D, k, q_dtype, bank_dtype, splits, reserved;
} uvc_knn_args;
int uvc_knn_workspace_bytes(int32_t nq, int32_t n, int32_t k, int32_t splits, int64_t* bytes, int32_t* splits_used);
int uvc_knn_topk(const uvc_knn_args* args, void* stream);
/* uvc_knn_vote: sims / idx [nq, k] as uvc_knn_topk leaves them, labels [n] (int32, or int64 with labels_i64), 1 <= num_classes <= 65536,
 * 1 <= k <= 64.  w_j = exp((s_j - s_0) / T) in float64 with s_0 the row's first (largest) similarity (w_j = 1 where s_j == s_0, and for every
 * j with T <= 0: a plain majority); score[c] = sum_j w_j [label(idx_j) == c], j ascending in float64 by one thread per class, rounded once
 * to float32.  Slots with an index outside [0, n) and labels outside [0, num_classes) count for nothing.  scores float32 [nq, num_classes]
 * or NULL; pred int32 [nq]: the first maximum of the row's scores (the lowest class), -1 for a row with no valid neighbour.  One workgroup
 * per query, fixed trees. */
int uvc_knn_vote(const float* sims, const int32_t* idx, const void* labels, int32_t labels_i64, int32_t nq, int32_t n, int32_t k,
                 int32_t num_classes, float temperature, float* scores, int32_t* pred, void* stream);

/* Linear probe on a feature bank (python -m uvc_amd.compact_probe): the L2-regularised multinomial logistic objective and its gradient,
 * what L-BFGS evaluates a few hundred times per fit.  Each call returns UVC_OK or refuses before anything is launched (outputs
 * untouched); no atomics, one writer per output element in every launch, the same bits on a repeat with the same chunk_rows; every
 * row offset is 64-bit.
 *
 * uvc_softmax_xent_grad: logits float32 [rows, ld] of which columns [0, C) are valid, labels [rows] (int32, or int64 with labels_i64).
 * Per row, in float32: the maximum of the valid columns, e_c = exp(z_c - max) with the difference carried as an exact two-term sum, their
 * sum in a fixed tree (a lane's columns ascending, then the xor butterfly), p_c = e_c / sum.  G [rows, ldg] of g_dtype (UVC_BF16: rounded
 * once; UVC_F32), ldg >= ld: p - 1 at the label (from p = 1/2 up taken as minus the other columns' share of the sum: no cancellation near p = 1) and p
 * elsewhere, +0 on columns [C, ld) and on every column of a row whose label lies outside [0, C) (an uncounted row: it adds nothing to
 * loss or hits either); columns [ld, ldg) are not written.  The row's loss term is log1p(sum without the first maximum's 1) - (z_y - max)
 * and its hit flag 1 when the label is the FIRST maximum of the valid columns.  loss_part float32 / hit_part int32
 * [uvc_softmax_xent_grad_blocks(rows, ld)]: the sums over the rows of each workgroup in a fixed order.  A row's results depend on that
 * row alone.  Up to 2048 columns a group of 1 .. 64 lanes holds a row in registers, beyond one workgroup takes a row; 16-byte accesses
 * when ld % 8 == 0, logits and G are 16-byte aligned and ldg rows are too, element by element otherwise.  1 <= C <= 65536,
 * C <= ld <= ldg, 1 <= rows < 2^31 (UVC_ERR_ARG).
 *
 * uvc_probe_eval: with z = X W^T + b over the m rows whose label lies in [0, C),
 *   F = (1/m) sum_i (lse(z_i) - z_{i, y_i}) + (l2 / 2) |W|^2,   dW = (1/m) G^T X + l2 W,   db = (1/m) colsum G,   hits = the rows whose label is the
 * first maximum.  X [n, D] (row stride ldx elements) of dtype (UVC_BF16 or UVC_F32), 16-byte aligned rows; W float32 [Cp, D] and b
 * float32 [Cp] with Cp = C rounded up to 8 -- the padding rows take no part and get exactly zero gradients, the bias is not regularised;
 * b and db may both be NULL (no bias).  dW float32 [Cp, D], db float32 [Cp], F float64 [1], counts int64 [2] = (hits, m); m = 0 gives the
 * l2 terms alone.  W is rounded to dtype once per call; the rows go through in chunks of chunk_rows (clamped to n): uvc_gemm_nt into a
 * float32 logits buffer, uvc_softmax_xent_grad, uvc_gemm_tn with beta = 1 and the device scalar 1 / m onto dW = l2 W and db = 0; one
 * workgroup then sums the loss, hit and |W|^2 partials in ascending order in float64.  Different chunk_rows differ by float32 summation
 * order only.  D a multiple of 8 (UVC_ERR_ARG) up to 1024 (UVC_ERR_UNSUPPORTED), 1 <= C <= 65536, 1 <= n < 2^31, chunk_rows >= 1,
 * l2 >= 0, workspace >= uvc_probe_workspace_bytes() and 16-byte aligned like X, W and dW (UVC_ERR_ARG). */
typedef struct uvc_probe_args {
  const void* X; const void* labels; const float* W; const float* b;
  float* dW; float* db; double* F; int64_t* counts;
  void* workspace; int64_t workspace_bytes;
  int64_t n, ldx;
  float l2;
  int32_t D, C, dtype, labels_i64, chunk_rows;
} uvc_probe_args;
int uvc_softmax_xent_grad_blocks(int64_t rows, int32_t ld, int64_t* blocks);
int uvc_softmax_xent_grad(const float* logits, const void* labels, int32_t labels_i64, int64_t rows, int32_t C, int32_t ld, void* G,
                          int32_t ldg, int32_t g_dtype, float* loss_part, int32_t* hit_part, void* stream);
int uvc_probe_workspace_bytes(int64_t n, int32_t D, int32_t C, int32_t dtype, int32_t chunk_rows, int64_t* bytes);
int uvc_probe_eval(const uvc_probe_args* args, void* stream);

/* Calibration of a logits bank (python -m uvc_amd.compact_calibrate): temperature and vector scaling are the affine map
 * z'_c = scale_c z_c + shift_c of the logits (scale_len = 1: one scale for every class, s = 1/T; scale_len = C: one per class; shift
 * float32 [C] or NULL).  logits float32 [n, ld] of which columns [0, C) are valid (the rest is never read into a result), labels [n]
 * (int32, or int64 with labels_i64); only the m rows whose label lies in [0, C) count.  With p = softmax(z') over the valid columns and
 * g_ic = p_ic - [c = y_i]:
 *
 * uvc_calib_eval:  F float64 [1] = (1/m) sum_i (lse(z'_i) - z'_{i, y_i});  dscale float32 [scale_len]: (1/m) sum_i g_ic z_ic (scale_len = 1:
 * its sum over c);  dshift float32 [C] = (1/m) sum_i g_ic, not touched when shift is NULL (and required with a shift);  counts int64 [2] =
 * (the rows whose label is the FIRST maximum of z', m).  m = 0 gives zeros.
 * uvc_calib_stats: per counted row conf = max_c p_c, pred = the first maximum, bin = clamp(ceil(conf bins) - 1, 0, bins - 1) (the intervals
 * ((j - 1) / bins, j / bins]); bin_count int64 / bin_conf float64 (the sum of conf) / bin_hit int64 (pred = label), each [bins];
 * sums float64 [2] = (sum_i -log p_{i, y_i}, sum_i (sum_c p_ic^2 - 2 p_{i, y_i} + 1)); counts int64 [2] = (hits, m).  1 <= bins <= 64.
 *
 * One pass over the logits, nothing of size [n, C] is written: workgroup w owns the rows [w R, (w + 1) R), R and the workgroup count
 * uvc_calib_blocks(n, ld) functions of (n, ld) alone -- not of the device --, and leaves one partial; a second launch adds the partials in
 * ascending workgroup order in float64 and divides by m.  z' is one float64 fma of the float32 inputs and z' - max is rounded to float32
 * once; the rest of a row is float32 in fixed trees (calib.hip).  A row's contribution does not depend on the rows beside it.  No atomics,
 * one writer per element in every launch, the same bits on a repeat; 64-bit row offsets; 16-byte loads when ld % 4 == 0 and logits is
 * 16-byte aligned, element by element otherwise; up to 2048 classes a row is read once, beyond it is read three times (twice from cache).
 * 1 <= n < 2^31, 1 <= C <= ld < 2^31, scale_len 1 or C, workspace >= uvc_calib_workspace_bytes(n, ld, C, bins; bins = 0: uvc_calib_eval) and
 * 16-byte aligned (UVC_ERR_ARG); C <= 65536 (UVC_ERR_UNSUPPORTED).  Every refusal happens before anything is launched. */
typedef struct uvc_calib_args {
  const float* logits; const void* labels; const float* scale; const float* shift;
  double* F; float* dscale; float* dshift; int64_t* counts;
  int64_t* bin_count; double* bin_conf; int64_t* bin_hit; double* sums;
  void* workspace; int64_t workspace_bytes;
  int64_t n, ld;
  int32_t C, scale_len, labels_i64, bins;
} uvc_calib_args;
int uvc_calib_blocks(int64_t n, int32_t ld, int64_t* blocks);
int uvc_calib_workspace_bytes(int64_t n, int32_t ld, int32_t C, int32_t bins, int64_t* bytes);
int uvc_calib_eval(const uvc_calib_args* args, void* stream);
int uvc_calib_stats(const uvc_calib_args* args, void* stream);

/* Split conformal prediction on a logits bank (python -m uvc_amd.compact_conformal; Sadinle et al. 2019, Romano et al. 2020, Angelopoulos et
 * al. 2021).  logits float32 [n, ld] of which columns [0, C) are valid (the rest is never read into a result); p = softmax(z * inv_temperature)
 * over the valid columns.  The classes of a row are ordered by descending z, ties by ascending index, -0 = +0 -- the order is taken on the
 * float32 inputs through order-preserving integer keys, so a rank is an exact integer; r_c in 1 .. C is the rank of class c and M_c the sum
 * of p_j over the classes ranked ahead of c.  u float32 [n], one value per row, or NULL (= 1 for every row).  The score of class c:
 *   UVC_CONFORMAL_LAC   s(c) = 1 - p_c
 *   UVC_CONFORMAL_APS   s(c) = M_c + u p_c
 *   UVC_CONFORMAL_RAPS  s(c) = M_c + u p_c + lam max(0, r_c - k_reg)
 * -inf logits are allowed (p = 0, ordered by index at the end).  A NaN in a valid column neither hangs nor reads or writes out of bounds;
 * that row's results are otherwise unspecified.
 *
 * uvc_conformal_scores: scores float32 [n] = s(y_i) of the rows whose label (int32, or int64 with labels_i64) lies in [0, C) and NaN for the
 * others; counts int64 [1] = m, the rows that count.  One pass, O(C) per row: only the label's rank and the mass ahead of it are taken.  Up
 * to 2048 classes a group of 1 .. 64 lanes holds a row in registers, the next row fetched before the current one is worked on -- 16-byte
 * loads when ld % 4 == 0 and logits is 16-byte aligned, element by element otherwise, the same bits either way --; beyond, up to 65536, one
 * workgroup takes a row (read twice, once from cache).  m is counted by a launch of its own over the labels.
 *
 * uvc_conformal_sets: the sets {c : s(c) <= qhat}: size int32 [n]; covered uint8 [n] = the label is in the set (0 for a row whose label lies
 * outside [0, C)), NULL together with labels when there are none; members uint32 [n, ceil(C / 32)] or NULL: bit c % 32 of word c / 32, the
 * padding bits zero.  qhat = +inf gives size = C.  A row's (key, index) pairs are sorted by a bitonic network in LDS, the exponentials
 * summed along the sorted order; ceil-pow2(C) / 2 threads (at most 256) take a row, so a workgroup holds 32 rows of 10 classes and 4 of
 * 100.  C <= 2048 (UVC_ERR_UNSUPPORTED beyond).  Nothing of size [n, C] is written by either call but members.
 *
 * Arithmetic: e_c = expf of the float32 rounding of (z_c - z_max) * inv_temperature, formed in float64; the sums of e (all of them, and
 * those ahead of a class) are float64 sums of these float32 terms in a fixed order, and s is formed in float64 and rounded to float32 once.
 * What remains is the error of the terms: with |d_c| <= ln(1 / p_c) and sum_c p_c ln(1 / p_c) <= ln C, the mass ahead, p_c and with them s
 * are within 2 * 2^-23 * (1 + ln C) + 2^-24 max(1, s) of the exact value -- 2.2e-6 at C = 2048.
 *
 * Both: no atomics, one writer per element, the same bits on a repeat, a row's result does not depend on the rows beside it, 64-bit row
 * offsets, workgroup counts functions of the shape alone (conformal.hip).  1 <= n < 2^31, 1 <= C <= ld < 2^31, method one of the three,
 * inv_temperature > 0 and finite, lam >= 0 and finite, k_reg >= 0, qhat not NaN, no NULL among logits and the call's outputs, scores / u /
 * members / size / int32 labels 4-byte and counts / int64 labels 8-byte aligned (UVC_ERR_ARG); scores: C <= 65536, sets: C <= 2048
 * (UVC_ERR_UNSUPPORTED).  Every refusal happens before anything is launched, outputs untouched. */
#define UVC_CONFORMAL_LAC 0
#define UVC_CONFORMAL_APS 1
#define UVC_CONFORMAL_RAPS 2
typedef struct uvc_conformal_args {
  const float* logits; const void* labels; const float* u;
  float* scores; int64_t* counts;                       /* uvc_conformal_scores */
  int32_t* size; uint8_t* covered; uint32_t* members;   /* uvc_conformal_sets */
  int64_t n, ld;
  int32_t C, labels_i64, method, k_reg;
  float inv_temperature, lam, qhat, reserved;
} uvc_conformal_args;
int uvc_conformal_scores(const uvc_conformal_args* args, void* stream);
int uvc_conformal_sets(const uvc_conformal_args* args, void* stream);

/* Out-of-distribution detectors on a bank (python -m uvc_amd.compact_ood; Hendrycks & Gimpel 2017, Liu et al. 2020, Lee et al. 2018, Ren et al.
 * 2021, Sun et al. 2022).  Each call returns UVC_OK or refuses before anything is launched (outputs untouched); no atomics, one writer per
 * output element in every launch, the same bits on a repeat, a row's result does not depend on the rows beside it, every row offset is
 * 64-bit, 16-byte accesses where the stride and the pointer allow and element by element otherwise, workgroup counts functions of the shape
 * alone (ood.hip).
 *
 * uvc_ood_logit_scores: logits float32 [n, ld] of which columns [0, n_valid) are valid (the rest is never read into a result); per row, in
 * float32, with m the first maximum and d_c = z_c - m:  msp = 1 / sum_c exp(d_c),  maxlogit = m,  energy = m + T log sum_c exp(d_c / T)
 * (= T log sum_c exp(z_c / T)),  entropy = sum_c p_c log p_c (the NEGATIVE entropy of softmax(z), 0 log 0 = 0) -- every score is higher for
 * an in-distribution row.  The maximum's own term is exactly 1 and the sums are taken without it (log1p of the rest); n_valid = 1 gives
 * 1, z_0, z_0, 0.  A NaN in a valid column gives NaN in that row's four results.  Each of the four outputs float32 [n] may be NULL (not all).
 * One pass: up to 2048 columns a group of 1 .. 64 lanes holds a row in registers, beyond one workgroup takes a row (read twice, once from
 * cache).  1 <= n < 2^31, 1 <= n_valid <= ld < 2^31, T > 0 and finite (UVC_ERR_ARG); n_valid <= 65536 (UVC_ERR_UNSUPPORTED).
 *
 * uvc_class_moments: X float32 [n, D] (row stride ldx), labels [n] (int32, or int64 with labels_i64); rows whose label lies outside [0, C)
 * are skipped.  perm int64 [n]: the permutation of a STABLE ascending sort of the labels (position j of the sorted order holds row perm[j];
 * an entry outside [0, n) reads nothing and counts as a skipped row).  counts int64 [C]; means float32 [C, D], 16-byte aligned: every
 * (class, column) sum is taken in float64 over the class's rows in ascending row order -- in slices of 256 positions of the sorted order,
 * the slices' partial sums added in ascending order: an order that is a function of (n, C, D) and the labels alone --, divided by the count
 * and rounded once; an empty class gives count 0 and a row of +0.  The bank is read once, whatever C is.  D a multiple of 8 (UVC_ERR_ARG)
 * up to 1016 (UVC_ERR_UNSUPPORTED), 1 <= C (UVC_ERR_ARG) <= 65536 (UVC_ERR_UNSUPPORTED), 1 <= n < 2^31, ldx >= D,
 * workspace >= uvc_class_moments_workspace_bytes(n, D) and 8-byte aligned (UVC_ERR_ARG).
 *
 * uvc_center_rows: out [n, D] (row stride ldo) = x_i - means[y_i] in float32, one rounding; a skipped row becomes a row of +0 (it adds
 * nothing to a scatter matrix).  Limits as uvc_class_moments'.
 *
 * uvc_rows_sqnorm_aug: Z float32 [n, ldz], ldz >= D + 8: sq[i] = sum_{d < D} z_id^2 in float32 -- lane l of the row's wave takes columns
 * (64 u + l) 4 .. + 3, u ascending, as one fmaf chain, then the xor butterfly -- and Z[i, D .. D + 8) = 1, 0, .. 0: the row becomes a query of
 * uvc_knn_topk against class rows (m_c, -|m_c|^2 / 2, 0 .. 0), whose best similarity s gives min_c |z - m_c|^2 = sq - 2 s.  Columns [0, D)
 * and [D + 8, ldz) are not written.  D as above. */
int uvc_ood_logit_scores(const float* logits, int64_t n, int64_t ld, int32_t n_valid, float temperature, float* msp, float* maxlogit,
                         float* energy, float* entropy, void* stream);
int uvc_class_moments_workspace_bytes(int64_t n, int32_t D, int64_t* bytes);
int uvc_class_moments(const float* X, int64_t ldx, const void* labels, int32_t labels_i64, const int64_t* perm, int64_t n, int32_t D,
                      int32_t C, int64_t* counts, float* means, void* workspace, int64_t workspace_bytes, void* stream);
int uvc_center_rows(const float* X, int64_t ldx, const void* labels, int32_t labels_i64, const float* means, int64_t n, int32_t D, int32_t C,
                    float* out, int64_t ldo, void* stream);
int uvc_rows_sqnorm_aug(float* Z, int64_t ldz, int64_t n, int32_t D, float* sq, void* stream);

/* Two models on one split (python -m uvc_amd.compact_compare; Milani Fard et al. 2016, Yan et al. 2021, Hooker et al. 2019, Stanton et al.
 * 2021): uvc_logits_pair_stats reads za float32 [n, lda] and zb float32 [n, ldb] ONCE -- of both, columns [0, C) are valid and the rest is
 * never read into a result -- and labels [n] (int32, or int64 with labels_i64; may be NULL) and writes, per row, each output [n] that is
 * not NULL (a NULL output is not wanted and not touched; not all may be NULL).  Per row and matrix, all in float32: m the FIRST maximum,
 * d_c = z_c - m, S = sum_c exp(d_c) with the maximum's own term exactly 1, l_c = d_c - log S, p_c = exp(d_c) / S, 0 log 0 = 0:
 *   top1_a, top1_b  int32   the first maximum's column
 *   conf_a, conf_b  float32 1 / S
 *   kl_ab           float32 sum_c p_a,c (l_a,c - l_b,c);  kl_ba likewise with a and b swapped
 *   js              float32 max(0, 1/2 sum p_a (l_a - l_m) + 1/2 sum p_b (l_b - l_m)),  l_m = max(l_a, l_b) + log1p(exp(-|l_a - l_b|)) - log 2
 *   tv              float32 1/2 sum_c |p_a,c - p_b,c|
 *   nll_a, nll_b    float32 -l_y
 *   rank_a, rank_b  int32   #{c < C : z_c > z_y or (z_c = z_y and c < y)}: 0 means the label is the top-1 under the first-maximum rule
 *   rank_b_top1a    int32   the same count in zb for the column top1_a;  rank_a_top1b: in za for the column top1_b
 * The differences of log-probabilities stay finite where log(p_a / p_b) would not: a 200-logit gap gives KL ~ 200, JS ~ log 2, TV ~ 1.
 * Two equal rows give kl = js = tv = 0 exactly.  A label outside [0, C), or NULL labels: nll_* = NaN and rank_a = rank_b = -1, the rest is
 * computed.  A NaN in a valid column of either row: every float output of the row NaN, every int output -1.  Logits are finite otherwise.
 * Up to uvc_logits_pair_stats_reg_max() = 1024 columns a group of 1 .. 64 lanes holds both rows in registers, the next pair fetched before
 * the current one is worked on; beyond, one workgroup takes a row pair (read three times, twice from cache).  16-byte loads when lda and
 * ldb are multiples of 4 and za and zb 16-byte aligned, element by element otherwise -- the same bits either way.  No atomics, one writer
 * per element, the same bits on a repeat and for a row alone or in a batch, 64-bit row offsets, workgroup counts functions of the shape
 * alone (compare.hip).  za, zb not NULL, 1 <= n < 2^31, 1 <= C <= lda, ldb < 2^31 (UVC_ERR_ARG); C <= 65536 (UVC_ERR_UNSUPPORTED).  Every
 * refusal happens before anything is launched. */
typedef struct uvc_pair_stats_args {
  const float* za; const float* zb; const void* labels;
  int32_t* top1_a; int32_t* top1_b; float* conf_a; float* conf_b; float* kl_ab; float* kl_ba; float* js; float* tv; float* nll_a; float* nll_b;
  int32_t* rank_a; int32_t* rank_b; int32_t* rank_b_top1a; int32_t* rank_a_top1b;
  int64_t n, lda, ldb;
  int32_t C, labels_i64;
} uvc_pair_stats_args;
int uvc_logits_pair_stats(const uvc_pair_stats_args* args, void* stream);
int uvc_logits_pair_stats_reg_max(void);

/* Common corruptions of a normalised image batch (python -m uvc_amd.compact_corrupt; corrupt.hip), in the style of Hendrycks & Dietterich
 * (ICLR 2019).  x, out: float32 [B, C, H, W], C <= 4, x = (pixel - mean_c) / std_c; every statement is on pixels p = x std_c + mean_c,
 * computed on the normalised values and ends with clamp(., lo_c, hi_c), the normalised 0 and 1 the caller passes.  No atomics, one writer
 * per output element, 64-bit offsets, the same bits on a repeat and for any split of the batch.  Each call returns UVC_OK or refuses before
 * anything is launched (outputs untouched): null pointers, B C H W == 0, C > 4, a NaN or negative level, std_c <= 0, lo_c > hi_c:
 * UVC_ERR_ARG; C H W >= 2^31 or more than 2^31 - 1 workgroups: UVC_ERR_UNSUPPORTED.
 *
 * uvc_corrupt_noise (kind 0 .. 2), a = level.  Element e of the batch has the global index g = index0 C H W + e (index0: the dataset index of
 * the batch's first image), so an image's noise does not depend on the batching.  The pair j = g >> 1 draws u1 (site 0) and u2 (site 1)
 * of uvc_exp_noise's keyed generator, key(seed, stream_id, site) at counter j; r = sqrt(-2 ln u1), t = float32(2 pi_f32 u2), z = r cos t for
 * even g and r sin t for odd g (logf, sqrtf, sincosf, once per pair).
 *   UVC_CORRUPT_GAUSSIAN_NOISE   p + a z             out = x + z (a / std_c)
 *   UVC_CORRUPT_SPECKLE_NOISE    p + a p z           out = x + z (a x + a mean_c / std_c)
 *   UVC_CORRUPT_IMPULSE_NOISE    u = the uniform of site 2 at counter g: u < a / 2 -> lo_c, a / 2 <= u < a -> hi_c, else x (a <= 1, UVC_ERR_ARG
 *                                beyond); the comparisons are exact (thresholds rounded up to float32 on the host).
 * Every element is read once, by 16-byte accesses when x + (e of a multiple of 4 in g) and out are 16-byte aligned, else element by element.
 *
 * uvc_corrupt_colour (kind 3, 4):
 *   UVC_CORRUPT_BRIGHTNESS   p clipped to [0, 1]; V = max_c p_c, V' = min(V + a, 1); p' = p V' / V when V > 0, else V' (the HSV value shift)
 *   UVC_CORRUPT_CONTRAST     m = the mean of p over the image's channels and pixels; (p - m) a + m, out = a x + (1 - a) (m - mean_c) / std_c.
 *                            m goes to image_mean float32 [B] (device, required) in a launch of its own: one workgroup per image, float64
 *                            per-thread sums in a fixed order and a fixed tree, whatever the grid of the pointwise launch.
 *
 * uvc_blur_separable: every plane (planes = B C, channel = plane % C) filtered along x, then along y, by the 2 R + 1 taps (host pointer,
 * 0 <= R <= 32, UVC_ERR_ARG beyond), borders clamp the index; each output is one fma chain over ascending taps from 0; the first pass
 * goes to scratch (float32, x's size, not x or out).  lo / hi (host [C], both or neither): the clamp of the second pass.
 * uvc_stencil2d: the dense K x K filter (taps: DEVICE float32 [K, K], K odd in 3 .. 25, UVC_ERR_ARG beyond), borders clamp the index, one fma
 * chain per output over the taps in row-major order, zero taps skipped.
 * uvc_pixelate: every pixel becomes the mean of its k x k cell (k >= 1; cells start at 0, a ragged last cell averages what exists): up
 * to k = 16 one float32 row-major sum per cell divided by the count, beyond a float64 sum in a fixed order; k = 1 returns x's bits.
 * uvc_box_muller: z0 = r cos t, z1 = r sin t of float32 u1 in (0, 1), u2 in [0, 1), n >= 1: the device function the noise kernels call. */
#define UVC_CORRUPT_GAUSSIAN_NOISE 0
#define UVC_CORRUPT_SPECKLE_NOISE 1
#define UVC_CORRUPT_IMPULSE_NOISE 2
#define UVC_CORRUPT_BRIGHTNESS 3
#define UVC_CORRUPT_CONTRAST 4
typedef struct uvc_corrupt_args {
  const float* x; float* out;
  float* image_mean;                                    /* contrast */
  int64_t index0; uint64_t seed, stream_id;             /* noise */
  double level;
  int32_t B, C, H, W, kind, reserved;
  double mean[4], std[4];                               /* the preset's statistics, as the spec takes them */
  float lo[4], hi[4];
} uvc_corrupt_args;
int uvc_corrupt_noise(const uvc_corrupt_args* args, void* stream);
int uvc_corrupt_colour(const uvc_corrupt_args* args, void* stream);
int uvc_blur_separable(const float* x, float* scratch, float* out, const float* taps, int32_t R, int64_t planes, int32_t C, int32_t H,
                       int32_t W, const float* lo, const float* hi, void* stream);
int uvc_stencil2d(const float* x, float* out, const float* taps, int32_t K, int64_t planes, int32_t C, int32_t H, int32_t W, const float* lo,
                  const float* hi, void* stream);
int uvc_pixelate(const float* x, float* out, int32_t k, int64_t planes, int32_t C, int32_t H, int32_t W, const float* lo, const float* hi,
                 void* stream);
int uvc_box_muller(const float* u1, const float* u2, float* z0, float* z1, int64_t n, void* stream);

/* Last-layer training-data influence on banks (python -m uvc_amd.compact_influence; influence.hip; Pruthi et al. 2020 "TracIn", Yeh et al.
 * 2018 "representer points").  For the head z = W f + b under cross-entropy the gradient of example i with respect to (W, b) is the outer
 * product r_i (x) [f_i; 1], r_i = softmax(z_i) - e_target, so the inner product of two examples' gradients is
 *   I(i, t) = (f_i . f_t + bias) * (r_i . r_t),   bias = 1 (the head's bias column; 0 for a head without one),
 * and the self-influence I(i, i) = (|f_i|^2 + bias) |r_i|^2.  Each call returns UVC_OK or refuses before anything is launched (outputs
 * untouched); no atomics, one writer per output element in every launch, the same bits on a repeat, every offset is 64-bit.
 *
 * uvc_influence_residuals: logits float32 [n, ld] of which columns [0, C) are valid (the rest is never read); labels [n] (int32, or int64
 * with labels_i64; may be NULL with target_mode 1).  The target of a row is its label (target_mode 0; a label outside [0, C) makes the row
 * a SKIPPED row) or the FIRST maximum of its valid columns (target_mode 1; a row without one -- all NaN or -inf -- is skipped).  r float32
 * [n, ldr], ldr >= C a multiple of 8 and r 16-byte aligned: softmax(z)_c - [c == target] on [0, C) and +0 on [C, ldr) -- rows that
 * uvc_influence_topk takes as they are; target int32 [n], -1 for a skipped row; rsq float32 [n] = sum_c r_c^2 of the float32 values as
 * stored.  A skipped row is +0 everywhere and rsq = 0.  Arithmetic (the convention of ood.hip / conformal.hip): m the maximum of the valid
 * columns, d_c = z_c - m in float32 (one rounding), e_c = expf(d_c) in float32, S the float64 sum of the e_c -- lane l of the row's wave
 * adds columns l, l + 64, ... in ascending order, then the xor butterfly over the lanes --, p_c = e_c / S and p_c - 1 in float64, rounded to
 * float32 once; rsq is the float64 sum of the squares in the same order, rounded once.  -inf logits are allowed (p = 0).  A NaN in a valid
 * column is never the maximum; it neither hangs nor reads or writes out of bounds, that row's r and rsq are NaN and the rows beside it
 * are not affected.  One wave per row, the row read three times (twice from cache).  1 <= n < 2^31, 1 <= C <= ld < 2^31, target_mode 0
 * or 1, no NULL among logits and the outputs (UVC_ERR_ARG); C <= 65536 (UVC_ERR_UNSUPPORTED).
 *
 * uvc_influence_topk: query features fq [nq, D] and bank features fb [n, D] (row strides ldfq, ldfb elements), both UVC_BF16 or both UVC_F32
 * (a mix: UVC_ERR_UNSUPPORTED), D a multiple of 8 in [8, 1024], 16-byte aligned pointers and row strides -- uvc_knn_topk's rules; query
 * residuals rq [nq, Cr] and bank residuals rb [n, Cr], float32 (row strides ldrq, ldrb), Cr a multiple of 8 in [8, 4096]
 * (UVC_ERR_UNSUPPORTED), 16-byte aligned likewise; bias finite.  Per (query t, bank row i):  sf = the feature dot product in exactly
 * uvc_knn_topk's arithmetic (the MFMA chain over ascending columns; float32: the fmaf chain from +0);  sr = the residual dot product as the
 * fmaf chain of v_mfma_f32_16x16x4_f32 from +0, c ascending;  v = (sf + bias) * sr, one float32 add and one float32 multiply.  v does not
 * depend on nq, n, the row's place in the bank or the split count.  pos_vals float32 / pos_idx int32 [nq, k]: the k largest v, descending,
 * equal values by ascending bank row; neg_vals / neg_idx [nq, k]: the k smallest v, ascending, equal values by ascending bank row.  Either
 * pair may be NULL (both of its pointers) and is then not computed; not both.  1 <= k <= 64.  Lists start as (-inf, -1) and (+inf, -1):
 * a bank of fewer than k rows leaves those slots; a NaN never enters either list, nor does -inf the first or +inf the second (they equal
 * the empty slot).  exclude int32 [nq] or NULL: one bank row per query that is skipped (-1, or any value outside [0, n): none) -- a query
 * that is itself a bank row.  One workgroup per 64 queries, the bank visited in ascending 64-row tiles; splits, workspace and the merge
 * are uvc_knn_topk's scheme: splits <= 0 lets the host choose from the shapes and the CU count, any value is clamped to
 * [1, min(512, ceil(n / 64))], splits_used > 1 needs workspace >= uvc_influence_workspace_bytes() (4-byte aligned), and every split count
 * gives the same bits.
 *
 * uvc_influence_self: f [n, D] of dtype (row stride ldf), D as above: fsq float32 [n] (or NULL) = sum_d f_d^2 in float32 -- lane l of the
 * row's wave takes columns (64 u + l) 4 .. + 3, u ascending, as one fmaf chain from +0, then the xor butterfly (uvc_rows_sqnorm_aug's order;
 * bf16 elements widened exactly) -- and out float32 [n] (or NULL; needs rsq float32 [n]) = (fsq + bias) * rsq, one float32 add and one
 * multiply.  Nothing else is written.
 *
 * uvc_influence_expf: e[i] = expf(d[i]), the device function uvc_influence_residuals calls, so that its error can be measured. */
typedef struct uvc_influence_args {
  const void* fq; const void* fb; const float* rq; const float* rb; const int32_t* exclude;
  float* pos_vals; int32_t* pos_idx; float* neg_vals; int32_t* neg_idx;
  void* workspace; int64_t workspace_bytes;
  int64_t ldfq, ldfb, ldrq, ldrb;
  float bias;
  int32_t nq, n, D, Cr, k, q_dtype, bank_dtype, splits, reserved;
} uvc_influence_args;
int uvc_influence_residuals(const float* logits, int64_t n, int64_t ld, int32_t C, const void* labels, int32_t labels_i64, int32_t target_mode,
                            float* r, int64_t ldr, int32_t* target, float* rsq, void* stream);
int uvc_influence_workspace_bytes(int32_t nq, int32_t n, int32_t k, int32_t splits, int64_t* bytes, int32_t* splits_used);
int uvc_influence_topk(const uvc_influence_args* args, void* stream);
int uvc_influence_self(const void* f, int64_t ldf, int32_t dtype, int64_t n, int32_t D, const float* rsq, float bias, float* fsq, float* out,
                       void* stream);
int uvc_influence_expf(const float* d, float* e, int64_t n, void* stream);

/* Two-model cascades (uvc_amd/compact_cascade.py, csrc/cascade.hip): the small model's answer stands where its confidence score reaches a
 * threshold, the other rows are deferred to the large model.  Every call returns UVC_OK or refuses before anything is launched; no atomics,
 * one writer per output element, the same bits on a repeat, a row's result independent of the rows beside it; 16-byte accesses where
 * pointers and strides allow, element by element otherwise, with the same values either way.
 *
 * uvc_cascade_decide: logits float32 [n, ld], columns [0, C) valid, 1 <= C <= 65536, 1 <= n < 2^31; T > 0 finite; kind 0 = msp
 * (max_c softmax(z / T)_c), 1 = margin (the largest minus the second largest entry of softmax(z / T); 1 at C = 1), 2 = entropy
 * (1 + sum_c p_c log p_c / log C with 0 log 0 = 0; 1 at C = 1).  With m the FIRST maximum: d_c = z_c - m, d_c / T and expf in float32, the
 * sums in float64 in a fixed lane order, every score rounded to float32 once.  score float32 [n], top1 int32 [n] (the first maximum),
 * defer int32 [n] = !(score >= tau) compared in float32 (tau = -inf never defers, +inf always; a NaN tau is refused); each may be NULL,
 * not all three.  A NaN in a valid column (or a row whose valid columns are all -inf): score NaN, top1 -1, defer 1.
 *
 * uvc_cascade_compact: defer int32 [n] (non-zero = deferred) -> idx int32 [n]: the deferred rows in ascending order in the first m slots,
 * the slots past m NOT written; pos int32 [n]: a deferred row's slot in idx, -1 for a kept row; count int32 [1] = m.  idx or pos may be
 * NULL.  Per-workgroup counts, their exclusive scan, then the writes; workspace >= uvc_cascade_compact_workspace_bytes(n), 4-byte aligned.
 *
 * uvc_cascade_gather: src [n * rows_per_item, width] of dtype (UVC_F32 / UVC_BF16; row stride ld_src elements) -> dst
 * [m * rows_per_item, width] (row stride ld_dst): item j of dst is item idx[j] of src, copied bit for bit; an index outside [0, n) gives
 * an item of +0.  0 <= m <= n comes from the host; m = 0 launches nothing.
 *
 * uvc_cascade_merge: out[b, :C] = pos[b] >= 0 ? z_large[pos[b], :C] : z_small[b, :C], bit for bit, for b in [0, n); source int32 [n] (or
 * NULL) = 1 / 0.  z_large has m rows (NULL at m = 0); a pos at or past m gives a row of NaN and source -1.  The three row strides are
 * independent; columns past C are not written. */
int uvc_cascade_decide(const float* logits, int64_t n, int64_t ld, int32_t C, float T, int32_t kind, float tau, float* score, int32_t* top1,
                       int32_t* defer, void* stream);
int uvc_cascade_compact_workspace_bytes(int64_t n, int64_t* bytes);
int uvc_cascade_compact(const int32_t* defer, int64_t n, int32_t* idx, int32_t* pos, int32_t* count, void* workspace, int64_t workspace_bytes,
                        void* stream);
int uvc_cascade_gather(const void* src, int64_t ld_src, int32_t dtype, int64_t n, int64_t rows_per_item, int64_t width, const int32_t* idx,
                       int64_t m, void* dst, int64_t ld_dst, void* stream);
int uvc_cascade_merge(const float* z_small, int64_t ld_small, const float* z_large, int64_t ld_large, int64_t m, const int32_t* pos, int64_t n,
                      int32_t C, float* out, int64_t ld_out, int32_t* source, void* stream);

/* Taylor gate scores of compact models (uvc_amd/compact_prune.py, csrc/prune.hip): the first-order importance of a multiplicative gate on
 * every kept head's attention output and on every MLP unit's GELU output (Molchanov et al., CVPR 2019; Michel et al., NeurIPS 2019), around
 * uvc_vit_compact_gate_grads of uvc_vit.h.  Each call returns UVC_OK or refuses with UVC_ERR_ARG before anything is launched (outputs
 * untouched); no atomics, one writer per output element, fixed summation orders: the same bits on a repeat and for any B, an image's row
 * independent of its neighbours.
 *
 * uvc_gate_dots: out[b, col0 + g] = sum_n sum_{c in group g} a[b N + n, c] * da[b N + n, c] for b < B, g < width / group; a and da are
 * [B N, width] row-major with leading dimensions lda / ldda (elements), image b owns rows [b N, (b + 1) N); group 1, 16, 32, 48 or 64 with
 * width % group == 0, group g the columns [g group, (g + 1) group); width a positive multiple of 16; out float32 [B, ld_out],
 * ld_out >= col0 + width / group.  Plain form (aux == dA == NULL; a head's attention output against its gradient): a and da of type T
 * (dtype UVC_F32 / UVC_BF16), nothing else is written.  Fused form (aux and dA given; a unit's GELU output against the raw fc2 input
 * gradient): a = u (T), da = dh FLOAT32, aux = GELU'(pre-activation) (T, ldaux), and dA[m, i] (T, lddA) = round_T(dh[m, i] * float(aux[m, i])),
 * one float32 multiply rounded once -- what UVC_EPI_MUL_AUX leaves -- so dh is read once for both.  Products and sums in float64 in a fixed
 * order (a lane's rows ascending, then the partial sums of a column in (wave, lane) order, then a group's columns ascending), ONE rounding to
 * float32: |out - exact| <= 2^-24 |exact| (1 + small) + n 2^-52 sum |terms|.  Bandwidth-bound: every operand element is read once, lanes run
 * along the columns, 16-byte accesses where the leading dimensions and every pointer are multiples of 16 bytes (element by element
 * otherwise: the same values), the four waves of a workgroup split an image's rows and meet in LDS in wave order; 64-bit offsets.
 * B <= 65535.
 *
 * uvc_gate_accumulate: s float32 [B, ld] with G <= ld columns; sum_sq[g] += s[b, g]^2 and sum_abs[g] += |s[b, g]| (float64 [G] each) as
 * one ascending chain over b per gate that goes on from the stored value: the sums over a split do not depend on how its images were
 * batched into calls (as uvc_ig_accumulate's). */
int uvc_gate_dots(const void* a, int64_t lda, const void* da, int64_t ldda, const void* aux, int64_t ldaux, void* dA, int64_t lddA, int32_t B,
                  int32_t N, int32_t width, int32_t group, float* out, int64_t ld_out, int32_t col0, int32_t dtype, void* stream);
int uvc_gate_accumulate(const float* s, int64_t ld, int32_t B, int32_t G, double* sum_sq, double* sum_abs, void* stream);

/* clip_grad_norm_(max_norm) + AdamW over flat float32 buffers (joint_train.py:428-429;
 * torch.optim.AdamW(lr, betas, eps, weight_decay) semantics, decoupled decay).
 * uvc_grad_sqnorm accumulates sum(g^2) of a segment into sq[0] (accumulate = 0 for the first segment) and leaves sqrt(sq[0]) -- the
 * total norm so far, clip_grad_norm_'s return value -- in sq[1]: sq is float[2];
 * uvc_adamw_step applies clip coefficient min(1, max_norm/(sqrt(sq[0])+1e-6)) read on the device. */
int uvc_grad_sqnorm(const float* g, int64_t n, float* partial /*[1024]*/, float* sq /*[2]*/, int32_t accumulate, void* stream);
typedef struct uvc_adamw_args {
  float* p; const float* g; float* m; float* v;
  void* p_shadow;        /* optional bf16 copy of p (GEMM operands), same layout */
  const float* sq;       /* device: total squared grad norm */
  float* gnorm_out;      /* optional device float: total norm (pre-clip) */
  int64_t n;
  float lr, beta1, beta2, eps, weight_decay, max_norm;
  int32_t step;          /* this segment's 1-based step count (bias correction) */
  const uint8_t* flags;  /* optional device [n]: bit 0 = weight decay applies to this element (timm add_weight_decay groups,
                            post_train.py:299), bit 1 = frozen: leave p/m/v untouched (parameter whose .grad is None) */
} uvc_adamw_args;
int uvc_adamw_step(const uvc_adamw_args* args, void* stream);
/* g *= clip coefficient (so later readers see what clip_grad_norm_ left in .grad; uvc_optimizer.py:90 reads it). */
int uvc_scale_by_clip(float* g, int64_t n, const float* sq, float max_norm, void* stream);

/* misc elementwise / layout kernels */
/* im2col of 16x16/stride-16 patches (PatchEmbed conv as a GEMM, model_distilled.py:142-151):
 * x [B,C,S,S] float32 -> out [B*(S/P)^2, C*P*P] T, k = c*P*P + ky*P + kx. */
int uvc_patchify(const float* x, void* out, int32_t B, int32_t C, int32_t S, int32_t P, int32_t dtype, void* stream);
/* tokens = cat(cls[, dist], patches * mask) + pos  (model_distilled.py:434-471).
 * pe [B,P,D] float32; row_mask optional [B,P] (patch gating), tok [B,N,D] float32. */
int uvc_assemble_tokens(const float* pe, const float* cls, const float* dist, const float* pos, const float* row_mask,
                        void* tok, int32_t B, int32_t P, int32_t D, int32_t ntok, int32_t tok_lowp /* 1: tok is bf16 */, void* stream);
/* backward of uvc_assemble_tokens: dpe [B,P,D] (T or f32) = dtok rows * mask; dpos/dcls/ddist = sums over batch
 * (written as beta_acc*old + sum); optional dmask[B,P] = <dtok row, pe row>.  dtok [B,N,D] is float32, or T when
 * dtok_lowp (the bf16 gradient stream of the backward). */
int uvc_assemble_tokens_bwd(const void* dtok, const float* pe, const float* row_mask, void* dpe, float* dpos, float* dcls,
                            float* ddist, float* dmask, int32_t B, int32_t P, int32_t D, int32_t ntok, int32_t dtype,
                            int32_t dpe_is_f32, int32_t dtok_lowp, float beta_acc, void* stream);
/* column sums: out[n] = beta*out[n] + alpha * sum_m X[m,n];  X is T or float32.  partial: [uvc_colsum_blocks(M), N]. */
int uvc_colsum(const void* X, int32_t M, int32_t N, int32_t ldx, int32_t dtype, int32_t x_is_f32, float* partial, float* out,
               float alpha, const float* alpha_ptr, float beta, const float* row_weight /* optional [M] */, void* stream);
/* patch gating (model_distilled.py:434-456, :36-63).
 * mode 1: mask[b,i] = sigmoid(patch_gating[i]) (or the hard >= .5 threshold with token 0 kept); backward sums over the batch.
 * mode 2: scores = Linear(D->1)(patch embedding); mask = straight-through Gumbel top-k of log_softmax(scores)
 *         with k = int(ratio*P), tau, Exp(1) draws e[B,P]; token 0 forced to 1.  ysoft/psoft [B,P] are kept for backward. */
int uvc_patch_gate_sigmoid(const float* pg, float* mask, int32_t B, int32_t P, int32_t hard, void* stream);
int uvc_patch_gate_sigmoid_bwd(const float* pg, const float* dmask, float* dpg, int32_t B, int32_t P, float beta_acc, void* stream);
int uvc_patch_scores(const float* pe, const float* w, const float* bias, float* scores, int32_t rows, int32_t D, void* stream);
int uvc_patch_topk_mask(const float* scores, const float* e, float* mask, float* ysoft, float* psoft, int32_t B, int32_t P, int32_t k,
                        float tau, void* stream);
int uvc_patch_topk_mask_bwd(const float* dmask, const float* ysoft, const float* psoft, float* dscores, int32_t B, int32_t P, float tau,
                            void* stream);
/* X[row,:] += row_weight[row] * w[:]   (X of type T, or float32 when x_is_f32) */
int uvc_add_outer(void* X, const float* row_weight, const float* w, int32_t rows, int32_t D, int32_t dtype, int32_t x_is_f32, void* stream);
int uvc_colsum_blocks(int32_t M);
/* timm.data.Mixup in "batch" mode (joint_train.py:409,924-933; post_train.py:362,618-621), in place on the device:
 * uvc_mixup_batch: x [B,C,H,W] float32, B even; mixup: x = x*lam + x.flip(0)*(1-lam) (both factors passed already rounded
 * to float32); cutmix: x[:,:,yl:yh,xl:xh] = x.flip(0)[:,:,yl:yh,xl:xh].
 * uvc_mixup_target: y [B,C] = onehot(t)*lam + onehot(t.flip(0))*(1-lam) with on/off values of label smoothing. */
int uvc_mixup_batch(float* x, int32_t B, int32_t C, int32_t H, int32_t W, float lam, float one_minus_lam, int32_t use_cutmix,
                    int32_t yl, int32_t yh, int32_t xl, int32_t xh, void* stream);
int uvc_mixup_target(const int64_t* labels, float* y, int32_t B, int32_t C, float lam, float one_minus_lam, float on_value,
                     float off_value, void* stream);
/* MLP compaction helpers (uvc_vit.h: uvc_mlp_compact).  idx [width]: hidden unit of each compact slot; inv [F]: slot or -1.
 * gather: w1c[s,:] = W1[idx[s],:], w1t = w1c^T, w2c[:,s] = W2[:,idx[s]], w2t = w2c^T (cast to T), b1c[s] = b1[idx[s]].
 * scatter: dW1[j,:] = dw1c[inv[j],:] or 0; db1[j] = db1c[inv[j]] or 0; dW2[:,j] = dw2c[:,inv[j]] or GELU(b1[j]) * db2[:]
 * (bf16 mode: GELU as the forward evaluates and stores it, approximant and bf16 rounding included; float32 mode: x/2 * erfc(-x/sqrt 2),
 * which is the forward's value to within its float32 rounding and keeps its relative accuracy for x < 0); written as beta_acc*old + value. */
int uvc_mlp_gather_shadows(const float* W1, const float* b1, const float* W2, const int32_t* idx, int32_t D, int32_t F, int32_t width,
                           void* w1c, void* w1t, void* w2c, void* w2t, float* b1c, int32_t dtype, void* stream);
int uvc_mlp_scatter_grads(const float* dw1c, const float* dw2c, const float* db1c, const int32_t* inv, const float* b1, const float* db2,
                          int32_t D, int32_t F, int32_t width, float* dW1, float* dW2, float* db1, float beta_acc, int32_t dtype, void* stream);
/* params[i] *= mask[i] over a flat parameter buffer: the Stage-2 `m.weight.data *= m.mask` for every module with a
 * mask buffer (post_train.py:343-346); mask is 1 where no module mask covers the element (biases, tokens). */
int uvc_apply_masks(float* params, const float* mask, int64_t n, void* stream);
/* float32 -> bf16 copy and transposed copy of a [R,C] matrix (weight shadows for the GEMMs). */
int uvc_cast_transpose(const float* W, int32_t R, int32_t C, void* w_bf16, void* wt, int32_t dtype, void* stream);
/* the same for up to 64 matrices in one launch: srcs[i] = element offset into params, ws[i]/wts[i] = element
 * offsets (units of T) into shadow for the cast / transposed copy, -1 = skip.  Host arrays. */
int uvc_cast_transpose_multi(const float* params, void* shadow, int32_t n, const int64_t* srcs, const int32_t* Rs, const int32_t* Cs,
                             const int64_t* ws, const int64_t* wts, int32_t dtype, void* stream);
/* Keyed Exp(1) noise for the Gumbel draws (model_distilled.py:40,485; uvc_utils.py:443-449): out[i] is a pure function of
 * (seed, step, site, i) -- counter-based, no generator state, identical on every data-parallel replica and after a resume.
 * out[i] = -logf(u), u = min(float32(c + 1/2) * 2^-24, 1 - 2^-24) for the 24-bit counter c = splitmix64(key ^ splitmix64(i)) >> 40
 * (24-bit resolution below u = 1/2, 23-bit above: c + 1/2 rounds to even from c = 2^23 up).  Every draw is finite and strictly
 * positive: the largest is 25 ln 2 = 17.3287 (c = 0), the smallest -logf(1 - 2^-24) = 2^-24 = 5.9604645e-08 (c = 2^24 - 1, the one
 * counter the min() changes: unclamped it gave u = 1 and a draw of -0, whose Gumbel value -log(E) is +inf).  Refuses n <= 0. */
int uvc_exp_noise(float* out, int64_t n, uint64_t seed, uint64_t step, uint32_t site, void* stream);

/* block-gate distributions (model_distilled.py:480-488): d[L,2] from g[L,2] and Exp(1) draws. */
int uvc_gate_distrib(const float* g, const float* e, float* d, int32_t L, int32_t mode, float eps, void* stream);
/* gradient of the gate logits from the dot products the LayerNorm-backward kernels leave behind
 * (DESIGN.md): dots [L+1,2], row l = { <dL/dx_l, x_l>, <dL/dout_l, x_l> } (row L: final norm), so
 * <dL/dout_l, out_l> = dots[l+1][0]; dg written as beta_acc*old + grad. */
int uvc_gate_grad(const float* g, const float* d, const float* dots, float* dg, int32_t L, int32_t mode, float eps,
                  float beta_acc, void* stream);

#ifdef __cplusplus
}
#endif
#endif
