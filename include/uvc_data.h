/* C-ABI of the image input step on MI355X (libuvc_hip.so): resampling of decoded uint8 images into a normalised
 * [B, 3, S, S] batch.
 *
 * The reference feeds both stages through torchvision transforms on PIL images (UVC/utils/data_utils.py:13-105):
 * RandomResizedCrop / Resize / CenterCrop resample with PIL's Image.resize(size, BILINEAR), an antialiased triangle
 * filter in 8-bit fixed point, then ToTensor and Normalize.  uvc_image_prep reproduces that bit for bit:
 *   - per axis, PIL's precompute_coeffs in float64 (scale = in / out, support = max(scale, 1), ksize = 2 ceil(support) + 1,
 *     weights tri((x + xmin - center + 0.5) / support) divided by their sum, rounded to int32 with 22 fraction bits);
 *   - the horizontal pass first, into a uint8 intermediate of the source rows the vertical pass reads, then the vertical pass;
 *     each accumulates in int32 from 1 << 21 and clamps with (acc >> 22) into 0..255.  Image.resize runs the vertical pass first
 *     (two single-axis resizes) when src_h > 100 src_w and resize_h < src_h; so does this library;
 *   - output float32 = (u8 / 255 - mean[c]) / std[c] with correctly rounded divisions (torch's ToTensor + Normalize), or the
 *     uint8 pixels themselves.
 * A pass whose axis is unchanged has the identity weights (1, 0), which return the input exactly: PIL skipping such a pass
 * and this library running it give the same bytes.
 *
 * The filter is a property of the launch (the `filter` field of the args structs; 0 = bilinear, as above).  UVC_IMAGE_FILTER_BICUBIC
 * is Image.resize(size, BICUBIC), what the released DeiT and T2T-ViT checkpoints were trained and evaluated with: PIL's bicubic_filter
 * with a = -0.5,
 *     ((a + 2)|x| - (a + 3)) x^2 + 1   for |x| < 1,      (((|x| - 5)|x| + 8)|x| - 4) a   for |x| < 2,      0 otherwise,
 * evaluated in float64, so support = 2 max(scale, 1) and ksize = 2 ceil(support) + 1; everything else (bounds, normalisation by the
 * sum, the rounding of a negative weight as (int)(-0.5 + w 2^22), pass order, spans) is the same code.  Its weights are negative in
 * places, so a sum can leave 0 .. 255 << 22: each pass clamps to 0 or 255 exactly where PIL's clip8 does, and the second pass reads
 * the first's clamped bytes.  The sums stay in int32, as PIL's `int`: |sum| <= 255 * 2^22 * sum|w| + 2^21 < 2^31 while sum|w| <
 * 2.007, and the normalised bicubic weights of one output pixel have sum|w| = 1.25 at phase 1/2 of an upscale (-1/16, 9/16, 9/16,
 * -1/16) and stay below 1.3 at other scales and at the edges.
 * The workspace depends on the filter (kh, kv, span0, span): complete the descriptors with the _filter query of the filter the launch
 * will name.  An image whose kh / kv are not those of the launch's filter is skipped on the device like every other descriptor that
 * fails its checks: its output is left untouched and its workspace is neither read nor written.
 *
 * Each image resamples its WHOLE source (box = (0, 0, src_w, src_h)) to resize_h x resize_w and keeps the S x S window at
 * (win_y, win_x): a random resized crop is a host-side slice of the decoded array (only the crop is uploaded) resized to
 * S x S with window (0, 0); Resize(256) + CenterCrop(224) is a resize to the torchvision size with the centre window.
 * Output pixels depend only on their own coefficients, so the window equals PIL's resize followed by a crop.  flip mirrors
 * the output columns (RandomHorizontalFlip after the crop).
 *
 * Conventions as in uvc_kernels.h: device pointers owned by the caller, no allocation, no host sync, `stream` is a
 * hipStream_t, int status return (0 = ok; uvc_last_error()).
 */
#ifndef UVC_DATA_H
#define UVC_DATA_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* One image of a ragged batch.  The caller fills the "in" fields; uvc_image_prep_workspace completes the "out" fields on the
 * host copy, which is then uploaded (uvc_image_prep_args.desc). */
typedef struct uvc_image_desc {
  int64_t src_offset;            /* in: byte offset of the image's first pixel in the packed source (HWC uint8, rows of src_w*3 bytes) */
  int32_t src_h, src_w;          /* in: source size, >= 1 */
  int32_t resize_h, resize_w;    /* in: size the whole source is resampled to, >= S */
  int32_t win_y, win_x;          /* in: top-left of the S x S output window, win_y + S <= resize_h, win_x + S <= resize_w */
  int32_t flip;                  /* in: 1 = mirror the output columns */
  int32_t kh, kv;                /* out: taps per output column / row (PIL's ksize) */
  int32_t span0, span;           /* out: source rows (order 0) or columns (order 1) [span0, span0 + span) the first pass covers */
  int32_t order;                 /* out: 0 = horizontal pass first; 1 = vertical first (Image.resize does that for sources taller
                                    than 100 x their width that shrink vertically) */
  int64_t ws_offset;             /* out: byte offset of the image's coefficient tables and intermediate in the workspace */
} uvc_image_desc;

enum { UVC_IMAGE_OUT_F32 = 0, UVC_IMAGE_OUT_U8 = 1 };
enum { UVC_IMAGE_FILTER_BILINEAR = 0, UVC_IMAGE_FILTER_BICUBIC = 1 };

typedef struct uvc_image_prep_args {
  const uint8_t* src;            /* packed uint8 HWC sources of all B images */
  int64_t src_bytes;             /* bytes of src: an image reaching past it is not read (its output is left untouched) */
  const uvc_image_desc* desc;    /* [B] device copy of the descriptors completed by uvc_image_prep_workspace */
  void* workspace;               /* >= the bytes uvc_image_prep_workspace returned, 16-byte aligned */
  int64_t workspace_bytes;
  void* out;                     /* [B, 3, S, S]: float32 (UVC_IMAGE_OUT_F32) or uint8 (UVC_IMAGE_OUT_U8) */
  float mean[3], std[3];         /* float32 per channel (F32 output only) */
  int32_t B, S, out_dtype;
  int32_t filter;                /* UVC_IMAGE_FILTER_*: 0 (a zeroed struct) is bilinear; anything else unknown is UVC_ERR_ARG */
} uvc_image_prep_args;

/* Host only (no device access): checks the B descriptors against S and src_bytes, fills kh, kv, span0, span, order and ws_offset,
 * and writes the workspace size the batch needs to *bytes. */
int uvc_image_prep_workspace(uvc_image_desc* desc, int32_t B, int32_t S, int64_t src_bytes, int64_t* bytes);

/* The same query for a launch with `filter` (UVC_IMAGE_FILTER_*; 0 equals the function above, an unknown value is UVC_ERR_ARG). */
int uvc_image_prep_workspace_filter(uvc_image_desc* desc, int32_t B, int32_t S, int64_t src_bytes, int32_t filter, int64_t* bytes);

/* Three launches whatever B is: coefficient tables, first pass, second pass + flip + normalise. */
int uvc_image_prep(const uvc_image_prep_args* args, void* stream);

/* ---- patch rows straight from the resampler.
 * The same three launches and the same arithmetic as uvc_image_prep with a float32 output, but the last pass stores what uvc_patchify
 * (uvc_kernels.h) would make of that batch, without the batch itself ever being written: args->out is T [B * (S/P)^2, 3 * P * P], and
 * output pixel (b, c, y, x) goes to row b (S/P)^2 + (y/P)(S/P) + x/P, column c P P + (y%P) P + x%P, cast to bf16 (dtype UVC_BF16 = 1,
 * round to nearest even) or kept float32 (UVC_F32 = 0) -- bit for bit uvc_patchify(uvc_image_prep(...)).  These are the rows a ViT
 * forward takes as uvc_vit_io.patches_in (uvc_vit.h).  args->out_dtype is not read; flip, normalisation, the filter and the descriptor
 * checks are uvc_image_prep's (a descriptor that does not fit is skipped and its rows are left untouched), and so is the workspace:
 * complete the descriptors with uvc_image_prep_workspace(_filter).  UVC_ERR_ARG: P <= 0 or S % P != 0, a dtype other than the two,
 * args->out not 16-byte aligned.  With P % 4 == 0 a thread stores four neighbouring columns at once (8 or 16 bytes); other patch
 * sizes take one column per thread. */
int uvc_image_prep_patches(const uvc_image_prep_args* args, int32_t P, int32_t dtype, void* stream);

/* ---- crop windows of a resident store.
 * A dataset that stays in device memory (uvc_amd/packed.py: every image HWC uint8, rows of img_w*3 bytes, back to back) is resampled
 * without copying its crops out: each descriptor names a stored image and a window inside it, and the passes read the window's rows
 * at the stored image's row stride.  The output is, bit for bit, uvc_image_prep's on the same crops copied out contiguously; the
 * vertical-first rule is evaluated on the crop's size, as Image.resize does after crop().  All store addressing is 64-bit. */
typedef struct uvc_image_crop_desc {
  int64_t src_offset;            /* in: byte offset of the stored image's first pixel in the store */
  int32_t img_h, img_w;          /* in: stored size, >= 1; rows of img_w*3 bytes */
  int32_t crop_y, crop_x;        /* in: top-left of the crop window inside the stored image */
  int32_t crop_h, crop_w;        /* in: crop size, >= 1, crop_y + crop_h <= img_h, crop_x + crop_w <= img_w */
  int32_t resize_h, resize_w;    /* in: size the crop is resampled to, >= S */
  int32_t win_y, win_x;          /* in: top-left of the S x S output window in the resized crop */
  int32_t flip;                  /* in: 1 = mirror the output columns */
  int32_t kh, kv;                /* out: as in uvc_image_desc */
  int32_t span0, span;           /* out: crop rows (order 0) or crop columns (order 1) the first pass covers */
  int32_t order;                 /* out */
  int64_t ws_offset;             /* out */
} uvc_image_crop_desc;

typedef struct uvc_image_prep_crops_args {
  const uint8_t* src;            /* the store */
  int64_t src_bytes;             /* bytes of the store: a stored image reaching past it is not read (its output is left untouched) */
  const uvc_image_crop_desc* desc; /* [B] device copy of the descriptors completed by uvc_image_prep_crops_workspace */
  void* workspace;               /* >= the bytes uvc_image_prep_crops_workspace returned, 16-byte aligned */
  int64_t workspace_bytes;
  void* out;                     /* [B, 3, S, S]: float32 (UVC_IMAGE_OUT_F32) or uint8 (UVC_IMAGE_OUT_U8) */
  float mean[3], std[3];
  int32_t B, S, out_dtype;
  int32_t filter;                /* UVC_IMAGE_FILTER_* */
} uvc_image_prep_crops_args;

/* Host only: checks that every crop lies inside its image and every image inside the store (store_bytes), applies the limits of
 * uvc_image_prep_workspace on sides, S and B, fills the "out" fields and writes the workspace size to *bytes. */
int uvc_image_prep_crops_workspace(uvc_image_crop_desc* desc, int32_t B, int32_t S, int64_t store_bytes, int64_t* bytes);
int uvc_image_prep_crops_workspace_filter(uvc_image_crop_desc* desc, int32_t B, int32_t S, int64_t store_bytes, int32_t filter, int64_t* bytes);

/* The same three launches, reading crop windows of the store; no host sync, no allocation. */
int uvc_image_prep_crops(const uvc_image_prep_crops_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
