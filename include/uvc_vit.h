/* C-ABI of the DeiT (DistilledVisionTransformer) forward / backward sequencer on MI355X.
 *
 * Replaces, for the Stage-1 hot path, what the reference runs through autograd over
 * UVC/models/model_distilled.py:429-531 (forward_features + heads) -- one call enqueues the
 * whole forward (or backward) as a fixed sequence of the kernels of uvc_kernels.h on `stream`.
 * Parameters live in ONE flat float32 buffer (layout from uvc_vit_layout) so the optimiser,
 * the gradient all-reduce and the UVC engine address them without per-tensor launches; the
 * Python module (uvc_amd/model_distilled.py) exposes them under the reference's state_dict
 * names as views.
 *
 * No allocation inside: the caller provides `workspace` (uvc_vit_workspace_bytes) which holds
 * the activations saved for backward and all scratch.
 */
#ifndef UVC_VIT_H
#define UVC_VIT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define UVC_VIT_MAX_DEPTH 32

typedef struct uvc_vit_cfg {
  int32_t img_size, patch_size, in_chans, num_classes, embed_dim, depth, num_heads, hidden;
  int32_t ntok;    /* 1, or 2 with the distillation token (enable_dist) */
  int32_t dtype;   /* UVC_F32 (exact float32 MFMA) or UVC_BF16 */
  float ln_eps;    /* LayerNorm epsilon; <= 0 selects DeiT's 1e-6 (model_distilled.py:402).  T2T-ViT uses nn.LayerNorm's 1e-5 (t2t_vit.py:111) */
  int32_t no_qkv_bias;  /* 1: attn.qkv has no bias (T2T blocks, transformer_block.py:49); its slot in the flat buffers is never read or written */
  int32_t resid_f32;    /* UVC_BF16 only.  0 (default): the residual stream -- the rows x_l every block reads and writes (model_distilled.py:240,244,
                           493) -- is stored as bf16 like every other activation (LayerNorm statistics, the residual additions and the gate mix
                           are float32 arithmetic on the loaded values; one rounding per stored row): the reference's own half-precision mode keeps
                           half activations (joint_train.py:283-287).  1: float32 rows as in rounds 1-2 (A/B runs).  UVC_F32 always has float32 rows */
  int32_t reserved;
} uvc_vit_cfg;

/* element offsets into the flat parameter / gradient buffers (every tensor 16-byte aligned) */
typedef struct uvc_vit_offsets {
  int64_t cls_token, dist_token, pos_embed, patch_w, patch_b;
  /* per block: norm1.w norm1.b qkv.w qkv.b proj.w proj.b norm2.w norm2.b fc1.w fc1.b fc2.w fc2.b */
  int64_t blk[UVC_VIT_MAX_DEPTH][12];
  int64_t norm_w, norm_b, head_w, head_b, headd_w, headd_b;
  int64_t n_main;        /* [0, n_main) always receives gradients in Stage-1 */
  int64_t gate;          /* block_skip_gating [L,2] (no gradient during warm-up) */
  int64_t gumbel_w, gumbel_b;   /* patch-gating scorer (gradient only in patch-gating mode 2) */
  int64_t patch_gating;  /* [P] (mode 1) */
  int64_t skip[UVC_VIT_MAX_DEPTH][2];  /* attn_skip_gating, mlp_skip_gating: never get gradients */
  int64_t n_total;
} uvc_vit_offsets;

/* element offsets (in units of T) into the shadow buffer: cast copies W and transposed copies W^T */
typedef struct uvc_vit_shadow_offsets {
  int64_t patch_w;
  int64_t blk_w[UVC_VIT_MAX_DEPTH][4];    /* qkv proj fc1 fc2   [out,in] */
  int64_t blk_wt[UVC_VIT_MAX_DEPTH][4];   /* transposed          [in,out] */
  int64_t head_w, head_wt, headd_w, headd_wt;
  int64_t n_total;
} uvc_vit_shadow_offsets;

int uvc_vit_layout(const uvc_vit_cfg* cfg, uvc_vit_offsets* off, uvc_vit_shadow_offsets* soff);
/* training: 0 = no-grad forward only; 1 = training, per-block backward streams (two-stream backward); 2 = training, one shared set of backward
 * streams (uvc_vit_io.shared_bwd_streams = 1; no side stream) */
int64_t uvc_vit_workspace_bytes(const uvc_vit_cfg* cfg, int32_t batch, int32_t training);
/* A HIP stream for uvc_vit_io.side_stream with a scheduling class: -1 = lowest priority the device offers (weight
 * gradients / teacher forward that should only fill idle CUs), 0 = default, +1 = highest.  Never destroyed by the
 * library; wrap it with the host framework's external-stream handle. */
int uvc_stream_create(int32_t priority_class, void** out);
int uvc_vit_ws_offsets(const uvc_vit_cfg* cfg, int32_t batch, int32_t training, int64_t* pe_off, int64_t* dpe_off);

/* refresh the T-typed shadows (W and W^T) from the float32 master weights */
int uvc_vit_update_shadows(const uvc_vit_cfg* cfg, const float* params, void* shadow, void* stream);

/* Stage-2 structured sparsity of one block's MLP: the hidden units whose fc1 row and fc2 column are masked
 * out are skipped instead of multiplied as zeros.  `width` (a multiple of 64; padding slots are pruned units, whose weights
 * are zero) compact units; w1 [width, D], w1t [D, width], w2 [D, width], w2t [width, D] of the model's operand type T and
 * b1 [width] float32 are gathered copies (uvc_mlp_gather_shadows); dw1 [width, D], dw2 [D, width], db1 [width] float32 are
 * scratch for the compact weight gradients, which uvc_mlp_scatter_grads expands into the full gradient tensors -- rows of
 * pruned units are exact zeros, and the fc2 gradient column of a pruned unit j is the rank-1 GELU(b1[j]) * db2 that the
 * dense computation produces (its activation is the constant GELU(b1[j])), so global-norm clipping sees the same norm. */
typedef struct uvc_mlp_compact {
  int32_t width; int32_t reserved;
  const void* w1; const void* w1t; const void* w2; const void* w2t; const float* b1;
  float* dw1; float* dw2; float* db1;
  const int32_t* inv;       /* device [F]: compact slot of hidden unit j, or -1 */
} uvc_mlp_compact;

typedef struct uvc_vit_io {
  const float* params;      /* flat float32 parameters */
  void* shadow;             /* flat T shadows */
  float* grads;             /* flat float32 gradients (backward) */
  void* workspace; int64_t workspace_bytes;
  const float* x;           /* [B, C, S, S] float32 */
  float* logits;            /* [B, num_classes] */
  float* logits_dist;       /* [B, num_classes], only with ntok == 2 */
  const float* d_logits;    /* backward inputs */
  const float* d_logits_dist;
  const float* gate_d;      /* device [L,2] block-gate distributions (model_distilled.py:480-488) or NULL */
  const int32_t* run_block; /* HOST [L] 0/1: hard block skip when gate_d is NULL (:496-500); NULL = run all */
  const float* patch_mask;  /* device [B,P] token mask (patch gating) or NULL */
  float* d_patch_mask;      /* backward: optional [B,P] gradient wrt patch_mask */
  int32_t batch;
  int32_t training;         /* forward: keep activations for backward */
  int32_t gate_mode;        /* 0 warm-up / none, 1 soft Gumbel, 2 softL0: selects d(gate logits) formula */
  float gate_eps;           /* softL0 eps */
  float accumulate;         /* backward: 0 = overwrite gradients, 1 = add (gradient accumulation) */
  /* stages [stage_begin, stage_end); 0,0 = everything.
   * backward: 0 = heads + final norm, 1..L = blocks L-1..0, L+1 = gate logits + token assembly,
   *           L+2 = patch-embedding weight gradient.  Lets the host cut the backward at gradient-bucket
   *           boundaries and start the RCCL all-reduce of a finished bucket on a second stream while the
   *           rest of the backward runs (and add the patch-scorer term to dpe before stage L+2).
   * forward:  0 = patch embedding, 1 = everything after it (the patch-gating mask is computed in between). */
  int32_t stage_begin, stage_end;
  /* backward, optional: a second hipStream_t.  The weight-gradient GEMMs (which hang off the dgrad chain) are
   * enqueued there and overlap the chain on `stream`; events order operand reads against buffer reuse, and
   * `stream` waits for the side stream before the call's last stage returns. */
  void* side_stream;
  const uvc_mlp_compact* mlp_compact;  /* HOST [L] or NULL; entries with width 0 or width == hidden run dense */
  const int32_t* head_keep;            /* device [L, H] or NULL: no-grad forwards skip the attention of heads marked 0 (their
                                          attn.proj input columns are masked to zero, so the result is unchanged); training forwards ignore it, backward
                                          uses it when head_keep_bwd is set */
  int32_t full_tail;                   /* 0 (default): the last block that runs computes everything behind its qkv projection on the class /
                                          distillation token rows only -- the only rows of it that reach the head (:507-526), so no output of the
                                          step changes (uvc_attention_tok_*); 1: all rows, as the reference executes it */
  int32_t fused_train_mlp;             /* 1: the training forward runs LayerNorm2 + fc1 (+GELU, GELU') + fc2 (+residual, gate mix) as ONE kernel
                                          (uvc_mlp_fused_fwd's training form, DeiT-Tiny width) instead of three; measured slower (218 us
                                          against 187), so 0 is the default */
  const void* patches_in;              /* optional T [B * np, C * P * P]: the patch rows of `x` already laid out by uvc_patchify (same image size and
                                          patch size).  The forward uses them instead of running uvc_patchify, the backward reads them for the
                                          patch-embedding weight gradient.  Lets student and teacher share the one rearrangement of a batch.
                                          uvc_vit_compact_forward reads nothing else of the batch: with patches_in, x may be NULL (rows written by
                                          uvc_image_prep_patches, uvc_data.h). */
  int32_t fuse_next_ln;                /* 1: a kernel that produces a block's output rows (uvc_mlp_fused_fwd; fc2 + residual + gate mix) also writes
                                          norm1 of the NEXT block that runs (model_distilled.py:241) from the rows it holds, and that block skips its
                                          stand-alone LayerNorm pass.  0: every LayerNorm is its own pass. */
  int32_t force_generic;               /* tests / A-B runs: passed to every uvc_gemm_nt of the pass; the values are described once, at the UVC_NT_*
                                          enum of uvc_kernels.h (UVC_NT_GENERIC, UVC_NT_NO_DMA, UVC_NT_WIDE_ANY_SIZE).  UVC_NT_GENERIC also runs every
                                          dgrad + LayerNorm backward as the unfused pair, UVC_NT_NO_DMA runs uvc_gemm_nt_lnbwd's register-staged
                                          variant.  0 = kernels picked by shape */
  int32_t head_keep_bwd;               /* 1: uvc_vit_backward skips dq / dk / dv of the heads head_keep marks 0 (written as zeros).  Exact when the
                                          64 attn.proj input columns of such a head are zero IN THE WEIGHTS the forward and the dgrad used (Stage-2:
                                          post_train.py:343-346 multiplies weight by mask before every step): dL/d(attention output) of the head is then
                                          exactly zero and so are its dq, dk, dv.  The forward still computes the head (dW_proj of the masked columns
                                          needs its output: the reference's clip norm sees it).  0: every head's backward runs */
  int32_t shared_bwd_streams;          /* 0 (default): the workspace (uvc_vit_workspace_bytes(.., training = 1)) holds per-block copies of the backward's
                                          streams dL/dx_l, dL/dx1, dA, dqkv, so that weight gradients on `side_stream` can read a block's streams while the
                                          main stream is blocks ahead (L x (5 M D + M F) elements more).  1: the workspace was sized with training = 2 --
                                          ONE shared set (dL/dx ping-pongs between two buffers); forward and backward of a step must agree, and the
                                          backward must run without a side stream (UVC_ERR_ARG otherwise).  Same results bit for bit. */
  int32_t gelu_grad_bf16;              /* 0 (default): where uvc_gemm_nt_q8_supported (bf16, embed_dim 192, hidden % 256 == 0, >= 4096 rows) the training forward
                                          leaves GELU'(a) of fc1 as ONE byte per activation (UVC_EPI_BIAS_GELU_GRAD_Q8: a uniform code over [-0.13, 1.13], |error|
                                          <= 2.47e-3 -- as accurate as bf16 on this bounded quantity, include/uvc_kernels.h) and the dgrad of fc2 decodes it
                                          (UVC_EPI_MUL_AUX_Q8): fc1 + GELU, GELU' is write-bound, 77 MB per block less at DeiT-Tiny batch 512.  1: bf16 GELU'(a)
                                          everywhere, as before r6 (A/B runs, tests).  Forward and backward of a step must agree. */
} uvc_vit_io;

int uvc_vit_forward(const uvc_vit_cfg* cfg, const uvc_vit_io* io, void* stream);
int uvc_vit_backward(const uvc_vit_cfg* cfg, const uvc_vit_io* io, void* stream);

/* ---- compact models (uvc_amd/compact.py): a pruned DeiT exported at its kept widths; the four entry points below are the no-grad forward,
 * uvc_vit_compact_train_* / uvc_vit_compact_backward further down train the same network ----
 * Block k of the export (one per block of the source model that runs) keeps `heads` heads with q / k of 64 dims and `v_dim` value dims each
 * (16, 32, 48 or 64; 0 when heads == 0), and `hidden` MLP units (a multiple of 16; may be 0).  The embedding, final norm and heads keep
 * the shapes of the dense model described by `cfg` (embed_dim, patch, classes, ntok, dtype, ln_eps; cfg.depth, num_heads and hidden
 * are those of the source model and bound the blocks: nblocks <= depth, heads <= num_heads, hidden <= cfg.hidden).
 * Per block: qkv.w [heads * (128 + v_dim), D] with rows [q heads*64 | k heads*64 | v heads*v_dim], qkv.b likewise; proj.w
 * [D, heads * v_dim]; fc1.w [hidden, D]; fc2.w [D, hidden]; the LayerNorms and biases of D as in the dense model.  A block with
 * heads == 0 adds proj.b to its rows, one with hidden == 0 adds fc2.b. */
typedef struct uvc_compact_block { int32_t heads, v_dim, hidden, reserved; } uvc_compact_block;
/* The flat float32 parameter layout (off: blk[k] for k < nblocks in the slot order of uvc_vit_offsets, cls / dist / pos / patch / norm /
 * heads and patch_gating as uvc_vit_layout; gate, gumbel and skip slots -1) and the bf16 shadow layout (soff: blk_w[k][0..3] = qkv, proj,
 * fc1, fc2 [out, in]; no transposed copies, blk_wt = -1).  Every tensor 16-byte aligned.  Either pointer may be NULL. */
int uvc_vit_compact_layout(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, uvc_vit_offsets* off,
                           uvc_vit_shadow_offsets* soff);
int64_t uvc_vit_compact_workspace_bytes(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, int32_t batch);
/* refresh the bf16 shadows (the [out, in] GEMM operands) from the float32 parameters; a no-op in float32 mode */
int uvc_vit_compact_update_shadows(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, const float* params, void* shadow,
                                   void* stream);
/* eval forward (model_distilled.py:429-531 in eval mode, every block of the export runs): logits and, with ntok == 2, logits_dist.
 * Reads io->params, shadow (bf16), workspace, x, logits, logits_dist, patch_mask (optional device [B, P]), patches_in (optional), batch;
 * the other members are ignored.  cfg.dtype UVC_F32 or UVC_BF16 (cfg.resid_f32 = 0). */
int uvc_vit_compact_forward(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, const uvc_vit_io* io, void* stream);
/* Attention rollout maps (Abnar & Zuidema 2020) of the readout token(s): uvc_vit_compact_forward with qkv and lse of every attention block kept
 * (workspace of uvc_vit_compact_rollout_workspace_bytes; io as for the forward, and logits / logits_dist are its bits), then a row vector pushed
 * back through the attention blocks, last block first, by uvc_attention_rollout_step (uvc_kernels.h).  rollout: device float32 [B, N] over
 * the model's tokens (class, distillation, patches), every row sums to 1.  The start vector is uniform over the readout tokens (1 on token
 * 0; 1/2 and 1/2 on tokens 0 and 1 with the distillation token, as the eval logits average the two heads).  method 0: rollout,
 * r <- r/2 + (1/2H) sum_h P_h^T r per block; method 1: "last", r <- (1/H) sum_h P_h^T r of the last attention block alone -- the head-mean
 * attention of the readout tokens.  A block without heads is the identity.  N <= 1026, UVC_F32 or UVC_BF16; deterministic. */
int64_t uvc_vit_compact_rollout_workspace_bytes(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, int32_t batch);
int uvc_vit_compact_rollout(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, const uvc_vit_io* io, float* rollout,
                            int32_t method, void* stream);
/* Features (python -m uvc_amd.compact_transfer): uvc_vit_compact_forward -- the same workspace (uvc_vit_compact_workspace_bytes) and io,
 * patches_in included, and logits / logits_dist are its bits -- then one small kernel over the final-norm readout rows [B, ntok, D] the
 * heads read: feats [B, D] = their float32 mean over the ntok rows (the class row; (cls + dist) / 2 with the distillation token, whose eval
 * logits average the two heads), divided by max(||.||_2, 1e-12) with `normalize` (F.normalize).  feats_dtype UVC_F32, or UVC_BF16: the
 * float32 result rounded once.  One wave per row, a lane's dims in ascending order and the wave butterfly: deterministic, and a row does
 * not depend on the batch.  Any N the eval forward takes. */
int uvc_vit_compact_features(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, const uvc_vit_io* io, void* feats,
                             int32_t normalize, int32_t feats_dtype, void* stream);

/* ---- fine-tuning a compact model at its kept widths (uvc_amd/compact_train.py) ----
 * One flat float32 parameter buffer serves eval and training, and a gradient buffer congruent with it: `off` is uvc_vit_compact_layout's.
 * The training shadow layout keeps that layout's [out, in] offsets (blk_w, head_w, headd_w, patch_w: uvc_vit_compact_forward runs on a
 * training shadow buffer) and appends the transposed copies the dgrads read (blk_wt[k][0..3], head_wt, headd_wt; units of T, T = float
 * in UVC_F32 mode, where only the transposed copies are written).  cfg.dtype UVC_F32 or UVC_BF16 with cfg.resid_f32 = 0; sequences of at
 * most 256 tokens (uvc_attention_bwd_vdim): every entry point below refuses longer ones with UVC_ERR_UNSUPPORTED (the workspace query
 * with -1), so nothing is half run. */
int uvc_vit_compact_train_layout(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, uvc_vit_offsets* off,
                                 uvc_vit_shadow_offsets* soff);
int64_t uvc_vit_compact_train_workspace_bytes(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, int32_t batch);
int uvc_vit_compact_train_update_shadows(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, const float* params, void* shadow,
                                         void* stream);
/* Parameters no forward reads, as (element offset, count) pairs into the flat buffers: norm1 (and the empty qkv / proj.weight) of a block
 * without heads, norm2 (and the empty fc1 / fc2.weight) of a block without units.  Autograd gives them no gradient, so an optimiser must
 * leave them alone (no update, no decay); uvc_vit_compact_backward writes zeros into their gradient slots.  ranges: [2 * cap]; *count
 * receives the number of pairs (UVC_ERR_ARG when it exceeds cap). */
int uvc_vit_compact_frozen_ranges(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, int64_t* ranges, int32_t cap,
                                  int32_t* count);
/* Training forward: uvc_vit_compact_forward's network, leaving in the workspace what the backward reads -- per block the LayerNorm
 * outputs and statistics, qkv, the attention output and lse, x1, GELU(a) and GELU'(a) (UVC_EPI_BIAS_GELU_GRAD).  io as for
 * uvc_vit_compact_forward (workspace of uvc_vit_compact_train_workspace_bytes, the training shadow); io->accumulate must be 0. */
int uvc_vit_compact_train_forward(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, const uvc_vit_io* io, void* stream);
/* Backward of the last uvc_vit_compact_train_forward on the same workspace, batch, patch_mask and patches_in: reads io->d_logits (and
 * d_logits_dist with ntok == 2), overwrites every gradient in io->grads[0, n_main) (frozen ranges: zeros).  One stream, existing kernels
 * in reverse order of the forward plus uvc_attention_bwd_vdim; deterministic.  A block without heads contributes colsum(dL/dx) to
 * proj.bias, one without units to fc2.bias.  The mode-1 token mask (io->patch_mask) is a constant: patch_gating gets no gradient. */
int uvc_vit_compact_backward(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, const uvc_vit_io* io, void* stream);

/* Class-specific relevance maps: the gradient-weighted attention rollout of Chefer, Gur & Wolf (ICCV 2021, "Generic Attention-Model
 * Explainability", self-attention rule) for the eval logit y of one class per image -- head(cls)[t], or (head(cls)[t] + head_dist(dist)[t]) / 2
 * with the distillation token.  Per block with heads A = (1/H) sum_h (P_h . dy/dP_h)^+, R <- R + A R from R = I; `relevance` (device float32
 * [B, N] over the model's tokens) is the readout row of the result (class token, or the mean of the class and distillation rows), computed as
 * that row vector pushed back from the last block to the first, r <- r + r A.  It is non-negative, NOT normalised (every row sums to >= 1, every
 * readout entry is >= 1 / ntok); a block without heads is the identity.
 * One stream: uvc_vit_compact_train_forward's walk (logits / logits_dist are the eval forward's bits), a small kernel that picks the target and
 * writes the one-hot logit gradient, then uvc_vit_compact_backward's walk without any weight-gradient GEMM, column sum or LayerNorm parameter
 * reduction, with one uvc_attention_relevance_step (uvc_kernels.h; keep = mix = 1) per block with heads right behind the attn.proj dgrad; the
 * walk ends behind the step of the lowest block with heads.  The gradient is the full one: the paths through later blocks' q and k included.
 * io: params, the TRAINING shadow (uvc_vit_compact_train_update_shadows: the dgrads read the transposed copies), workspace (of
 * uvc_vit_compact_attribution_workspace_bytes), x, logits, logits_dist, patch_mask, patches_in, batch; accumulate must be 0; grads is not read.
 * target: device [B] class indices, or NULL for the first maximum of the eval logits over [0, num_labels) (ties: the lowest index).  A given
 * index outside [0, num_labels) is clamped into it by the kernel -- callers check it on the host (uvc_amd/compact_attribution.py refuses it).
 * 1 <= num_labels <= num_classes, otherwise UVC_ERR_ARG.  target_out: optional device [B], the class explained.
 * Sequences above 256 tokens: UVC_ERR_UNSUPPORTED and -1 from the workspace query, as every compact training entry point.  Deterministic. */
int64_t uvc_vit_compact_attribution_workspace_bytes(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, int32_t batch);
int uvc_vit_compact_attribution(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, const uvc_vit_io* io, const int32_t* target,
                                int32_t num_labels, float* relevance, int32_t* target_out, void* stream);

/* The gradient of one class's eval logit with respect to the INPUT, as patch rows: what saliency, gradient x input and integrated gradients
 * (python -m uvc_amd.compact_pixel) are built on.  d_rows: device float32 [B * np, C * P * P] in uvc_patchify's layout (uvc_unpatchify of
 * uvc_kernels.h turns them into [B, C, S, S]).
 * One stream: uvc_vit_compact_train_forward's walk (logits / logits_dist are the eval forward's bits), uvc_vit_compact_attribution's target pick
 * and one-hot logit gradient, then uvc_vit_compact_backward's walk with dgrads only -- no weight-gradient GEMM, column sum, LayerNorm parameter
 * reduction or relevance step -- through EVERY block down to block 0 (a bias-only branch passes the stream through unchanged), the backward of
 * token assembly (dpe = dtok patch rows * patch_mask; the sums over the batch it also makes go to scratch) and the patch-embedding dgrad
 * d_rows = dpe [B * np, D] . W_patch [D, K0] through uvc_gemm_nt, whose [K0, D] operand is a transposed copy of the weight in the operand type
 * made per call in this entry's workspace (the shadow layouts do not hold one).  With mode-1 hard gating the rows of zeroed patches are zeros.
 * io as for uvc_vit_compact_attribution (the TRAINING shadow; workspace of uvc_vit_compact_input_grad_workspace_bytes), but patches_in is
 * accepted and x may then be NULL, as in uvc_vit_compact_forward: the interpolated inputs of integrated gradients exist only as patch rows.
 * target / num_labels / target_out as for uvc_vit_compact_attribution.  Sequences above 256 tokens: UVC_ERR_UNSUPPORTED and -1 from the
 * workspace query, as every compact training entry point.  Deterministic. */
int64_t uvc_vit_compact_input_grad_workspace_bytes(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, int32_t batch);
int uvc_vit_compact_input_grad(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, const uvc_vit_io* io, const int32_t* target,
                               int32_t num_labels, float* d_rows, int32_t* target_out, void* stream);

/* The gradient of a per-image attack LOSS with respect to the input, as patch rows: what FGSM and PGD (python -m uvc_amd.compact_robust) step
 * along.  uvc_vit_compact_input_grad with the one-hot seed replaced by uvc_loss_seed of uvc_kernels.h (the same kernel): kind 0 cross-entropy,
 * dz = softmax(z) - onehot(label); kind 1 margin, dz = onehot(j) - onehot(label), j the first maximum among the other labels (num_labels >= 2,
 * otherwise UVC_ERR_ARG).  The same workspace (uvc_vit_compact_input_grad_workspace_bytes), the same transposed copy of the patch weight, the
 * same dgrad walk.  labels: device int32 [B], clamped into [0, num_labels) by the kernel -- callers check them on the host.  d_rows float32
 * [B * np, K0] = dL_b / d rows of image b's OWN loss (not the batch mean): a batch's rows do not depend on its neighbours.  loss_out: device
 * float32 [B], or NULL.  io as for uvc_vit_compact_input_grad (x or patches_in; logits / logits_dist are the eval forward's bits).  Every
 * refusal comes before anything is launched.  One stream, deterministic. */
int uvc_vit_compact_loss_grad(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, const uvc_vit_io* io, const int32_t* labels,
                              int32_t num_labels, int32_t kind, float* d_rows, float* loss_out, void* stream);

/* Taylor gate scores: which kept heads and MLP units of a compact file can go next (python -m uvc_amd.compact_prune).  gates: device float32
 * [B, G], G = sum_k (heads_k + hidden_k), columns block-ascending, a block's heads first, then its hidden_k units (padding units included:
 * their entries are exact zeros).  gates[b, .] is the gradient of image b's OWN cross-entropy (uvc_loss_seed kind 0 on the eval logits over
 * [0, num_labels): uvc_vit_compact_loss_grad's loss, not the batch mean) with respect to a multiplicative gate on each head's attention
 * output and on each unit's GELU output, at gate = 1:
 *   head (k, j): sum_n sum_{c < v_dim} o_k[b, n, j v_dim + c] * dO_k[b, n, j v_dim + c]     (dO: the attn.proj input gradient)
 *   unit (k, i): sum_n u_k[b, n, i] * (g_k W2_k)[b, n, i]                                   (the raw fc2 input gradient, before GELU')
 * the quantity whose square (Molchanov et al., CVPR 2019) or absolute value (Michel et al., NeurIPS 2019) is averaged over a dataset.
 * One stream: uvc_vit_compact_train_forward's walk (logits / logits_dist are the eval forward's bits), the seed, then
 * uvc_vit_compact_backward's walk with dgrads only -- no weight-gradient GEMM, column sum or LayerNorm parameter reduction -- with one plain
 * uvc_gate_dots (uvc_kernels.h; group = v_dim) behind each attn.proj dgrad, and each fc2 dgrad run with UVC_EPI_NONE into a float32 scratch
 * followed by one fused uvc_gate_dots (group = 1), which also writes the dA the fc1 dgrad reads.  The walk ends behind the last dot it
 * needs: the lowest block that has a head or a unit.  A block without heads, or without units, contributes no columns and passes the stream
 * through.  io as for uvc_vit_compact_attribution (the TRAINING shadow; workspace of uvc_vit_compact_gate_grads_workspace_bytes; x, not
 * patches_in); accumulate must be 0.  labels: device int32 [B], clamped into [0, num_labels) by the kernel -- callers check them on the
 * host.  1 <= num_labels <= num_classes, otherwise UVC_ERR_ARG.  loss_out: device float32 [B], or NULL.  Sequences above 256 tokens:
 * UVC_ERR_UNSUPPORTED and -1 from the workspace query, as every compact training entry point.  Every refusal comes before anything is
 * launched.  Deterministic; an image's row does not depend on its neighbours. */
int64_t uvc_vit_compact_gate_grads_workspace_bytes(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, int32_t batch);
int uvc_vit_compact_gate_grads(const uvc_vit_cfg* cfg, const uvc_compact_block* blocks, int32_t nblocks, const uvc_vit_io* io, const int32_t* labels,
                               int32_t num_labels, float* gates, float* loss_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
