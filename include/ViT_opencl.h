/*
 * ViT_opencl.h -- the drop-in entry point and the extended C API around it.
 *
 * `ViT_opencl` keeps the exact prototype of the reference
 * (MulticoreMainProject/ViT_opencl.h:6, defined ViT_opencl.c:794, sole caller
 * Main.c:54) so that Main.c and comparator.c link unchanged; behind it sits a
 * batched HIP forward pass for gfx950 instead of 113 OpenCL launches per image.
 * The name is kept for link compatibility only -- nothing here uses OpenCL.
 *
 * Differences from the reference that callers can rely on:
 *   - synchronous: every probabilities[i] is complete on return
 *     (the reference may return with the last read-back in flight,
 *      ViT_opencl.c:775-778,978-985);
 *   - repeatable and with no image cap (the reference is single-shot and
 *     capped at 100 images, ViT_opencl.c:104-114,747);
 *   - no dependence on the current directory (the reference reads *.cl from
 *     CWD at run time, ViT_opencl.c:833-899).
 */
#ifndef VIT_HIP_VIT_OPENCL_H
#define VIT_HIP_VIT_OPENCL_H

#include "Network.h"
#include "kernelHandler.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Model shape.  The reference hard-codes ViT-B/16 as #defines duplicated in
 * ViT_seq.c:10-21 and ViT_opencl.c:13-24; here it is data. */
typedef struct vit_config
{
    int img_size;    /* 224: the input's height, and its width too unless img_width says otherwise */
    int patch_size;  /* 16  */
    int in_chans;    /* 3   */
    int num_classes; /* 1000 */
    int embed_dim;   /* 768 */
    int depth;       /* 12  */
    int num_heads;   /* 12  */
    int mlp_hidden;  /* (int)(embed_dim * mlp_ratio) = 3072 */
    double eps;      /* LayerNorm epsilon, a double literal in the reference (1e-6) */
    int img_width;   /* 0: img_size (a square input); otherwise the input is img_size rows by img_width columns */
} vit_config;

/* Fill `cfg` with a named preset: "vit_b_16" (the reference's only
 * configuration), "vit_l_16", "vit_h_14" (224 px), and the higher-resolution
 * fine-tuning shapes "vit_b_16_384" (T = 577), "vit_l_16_512" (T = 1025),
 * "vit_h_14_518" (T = 1370).  Returns 0, or -1 for an unknown name.
 *
 * Attention by token count T and head_dim (fixed when a context is created):
 *   T <= 208, head_dim 64, planes paths  resident kernel (attention_p3.hip)
 *   T <= 272, head_dim 80, reduced modes resident kernel (attention_h16.hip)
 *   otherwise up to T = 512              streaming kernel (attention_tiled.hip)
 *   T > 512, head_dim 64 or 80           flash-style kernel (attention_long.hip) on
 *                                        the planes paths: F32 (default planes),
 *                                        BF16_GEMM, FP8_GEMM
 * Above 512 tokens F32_FP16X2, the fp32-rows path ($VIT_HIP_P3=0,
 * $VIT_HIP_GEMM_FP32=native, embed_dim or mlp_hidden not multiples of 128) and
 * other head dims are refused at creation (code 2).
 *
 * The $VIT_HIP_* switches are read when a context is created and at no other
 * time: they are part of that context's plan, and two contexts of one process
 * may differ in them.  Which plans each one reaches:
 *   $VIT_HIP_P3=0              F32: fp32 activation rows, operands split inside
 *                              the GEMM loop (the fp32-rows path)
 *   $VIT_HIP_GEMM_FP32=native  F32: the fp32-rows path with the fp32 matrix
 *                              instruction in the patch embedding, the attention
 *                              and every projection without pre-split weights
 *   $VIT_HIP_ATTN=long         the planes paths with head_dim 64 or 80:
 *                              attention_long.hip at any T
 *   $VIT_HIP_ATTN=tiled        plans whose attention reads fp32 rows -- the
 *                              fp32-rows path, F32_FP16X2 and the "otherwise"
 *                              line above: attention_tiled.hip at every shape.
 *                              The resident planes kernels (the default ViT-B/16
 *                              plan among them) are not affected. */
int vit_config_preset(vit_config *cfg, const char *name);

/* Non-square inputs.  A context takes images of img_size rows by img_width columns (both multiples of patch_size, at most
 * 4096; at most 512 patches a side); its patches form a gh x gw grid, row-major, and T = gh * gw + 1.  Everything behind the
 * patch embedding depends on T alone.  A square input has ONE representation inside the library: wherever a config enters it
 * (vit_hip_create*, vit_resample_check*, the plan) img_width == img_size is stored as 0, so vit_hip_config() of a square
 * context reports img_width 0 whichever way it was asked for, and a square context computes, launches and exports exactly
 * what it did before the field existed.
 * vit_config_canonical: host only; *out = that form of *cfg, every byte written (out may be cfg); 0, or 1 with a message
 * that begins with `who` (NULL: its own name) for a NULL argument, an img_width that is not a positive multiple of
 * patch_size or is above 4096, or a non-square config with a grid side above 512.  vit_hip_create* refuse with it (code 1)
 * before anything is allocated; a pos_embedding (tensor 3) of the wrong row count stays code 3.
 * Still square only, and refused on a non-square context with code 1 and a message that says "non-square" before any upload
 * or launch: the resize and box ingest forms (vit_hip_resize_crop_u8, vit_hip_crop_boxes_u8, vit_hip_forward*_u8_resized,
 * vit_hip_forward*_u8_boxes: their crops are img x img) and vit_hip_export_planes. */
int vit_config_canonical(const vit_config *cfg, vit_config *out, const char *who);
void vit_config_grid(const vit_config *cfg, int *grid_h, int *grid_w);   /* img_size / patch, width / patch; either may be NULL */
int vit_config_sizeof(void);                       /* sizeof(vit_config), for bindings that restate the struct */

/* Derived sizes. */
int vit_config_tokens(const vit_config *cfg);      /* grid_h * grid_w + 1 */
int vit_config_num_tensors(const vit_config *cfg); /* 4 + 12*depth + 4 (152 for B/16) */
/* Element count tensor `idx` must have (torchvision state-dict order,
 * reference index map: ViT_seq.c:437-513, ViT_opencl.c:159,280-295). */
size_t vit_config_tensor_size(const vit_config *cfg, int idx);

/* The drop-in symbol.  ViT-B/16 only, like the reference.  `image` is an
 * array of image[0].n elements; `networks` the 152 host tensors;
 * probabilities[i] receives 1000 post-softmax values.  Uses device
 * $VIT_HIP_DEVICE (default 0).  On any device error: message + exit(EXIT_FAILURE),
 * mirroring CHECK_ERROR. */
void ViT_opencl(ImageData *image, Network *networks, float **probabilities);
/* Wall-clock split of the calling thread's last ViT_opencl(): context creation -- what the reference prints as
 * "setup time" (ViT_opencl.c:910) and what Main.c:51-57 times together with the images -- and the rest of the call. */
void vit_hip_last_call_seconds(double *setup_s, double *forward_s);

/* ---- extended API: resident weights, other configs, logits ---- */

typedef struct vit_hip_ctx vit_hip_ctx;

/* Upload `networks` (n_tensors host tensors, validated against cfg) to
 * `device` once and size the activation arena for up to `max_batch` images per
 * launch sequence.  What the reference redoes on every call inside its timed
 * region (ViT_opencl.c:908-924) happens here, once. */
int vit_hip_create(vit_hip_ctx **out, const vit_config *cfg, const Network *networks,
                   int n_tensors, int device, int max_batch);
void vit_hip_destroy(vit_hip_ctx *ctx);

/* Arithmetic of the dense projections.  F32 is the parity path (class logits within
 * 1e-4 of ViT_seq.c).  BF16_GEMM (BASELINE config 3) rounds the GEMM operands --
 * LayerNorm outputs, attention output, MLP hidden layer, and the QKV / out-proj / fc1 /
 * fc2 weights -- to bfloat16 and accumulates in fp32; the residual stream, attention
 * arithmetic, norms and classifier stay fp32.  Its logits differ from ViT_seq.c by
 * ~1e-2 (tests/test_gpu_parity.py states the tolerance), so it is opt-in:
 * vit_hip_create() (and so the drop-in ViT_opencl) uses F32 unless $VIT_HIP_PRECISION=bf16, or =fp16x2
 * for F32_FP16X2 below. */
enum { VIT_PRECISION_F32 = 0, VIT_PRECISION_BF16_GEMM = 1, VIT_PRECISION_FP8_GEMM = 2, VIT_PRECISION_F32_FP16X2 = 3 };
int vit_hip_create_ex(vit_hip_ctx **out, const vit_config *cfg, const Network *networks,
                      int n_tensors, int device, int max_batch, int precision);
int vit_hip_precision(const vit_hip_ctx *ctx);
/* 1 when the context folds every LayerNorm but the final one into the projection behind it (csrc/norm_fold.h): the
 * default of BF16_GEMM and FP8_GEMM ($VIT_HIP_LN_FOLD=0 at creation keeps the separate LayerNorm launches); on F32 only
 * as a lab variant on the three-part planes ($VIT_HIP_LN_FOLD=1); never for F32_FP16X2. */
int vit_hip_ln_fold(const vit_hip_ctx *ctx);

/* Repacked weights on disk (the offline half of the weight-format tooling): export writes what the context holds in HBM
 * after its repack -- every tensor in fp32 (reference order) plus the precision's GEMM-operand copy of the four big
 * matrices of every layer (three-part bf16 planes / one-part planes / fp16 pairs / MX values + scales) -- behind a
 * header that pins the model shape and precision; create_from_planes builds an identical context from that ONE file
 * (three reads into three allocations; the reference's loader opens 152 files, Network.c:134-218).  Logits of the two
 * contexts are bit-identical.
 * The header pins ONE image side, so export refuses a non-square context (code 1, "non-square", nothing written).  No weight
 * but pos_embedding depends on the input size: the way to a non-square context from a file is to load the square file and
 * call vit_hip_create_at_size on it. */
int vit_hip_export_planes(vit_hip_ctx *ctx, const char *path);
int vit_hip_create_from_planes(vit_hip_ctx **out, const char *path, int device, int max_batch);

/* ---- the same model at another resolution: a context derived on the GPU from one that exists ----
 * A context runs at the resolution its pos_embedding (tensor 3) was trained at: vit_hip_create_ex refuses any other row
 * count (code 3).  vit_hip_create_at_size makes a NEW context for the same weights at another img_height x img_width from a
 * context `src` that already exists -- created from host tensors or from a planes file, square or not -- without host
 * tensors; vit_hip_create_at_resolution(.., s, ..) is vit_hip_create_at_size(.., s, s, ..) under its own name:
 *   - tensor 3 is produced by vh_launch_resample_pos_embed (include/kernelHandler.h states the definition and its error
 *     bound; csrc/pos_resample.hip) with prefix = 1 and the gh x gw patch grids of the two contexts;
 *   - every other weight is copied device to device in the form it already has: the three slabs of GEMM operands,
 *     conv_proj planes and folded LayerNorm terms whole, the fp32 tensors one by one into the new layout.  Nothing is
 *     re-split, re-quantised or re-folded, so the derived context holds the bits a context created at img_size from the
 *     same tensors -- with that pos_embedding -- would hold, and computes the same logits bit for bit.
 * The derived context is an ordinary context: it takes every entry point, every armed output and vit_hip_export_planes;
 * nothing records that it was derived, and nothing is shared -- destroying `src` afterwards leaves it whole.
 * Inherited from src: the device, the precision, the LayerNorm fold (vit_hip_ln_fold) and the fp16-pair scales.  Read
 * afresh, as at every creation: the $VIT_HIP_* switches.  Not inherited: armed requests, vit_hip_set_last_layer_cls_only.
 * max_batch <= 0: src's.  how == NULL: bicubic, align_corners 0 (the Hugging Face ViT's and DINO's convention; {BICUBIC, 1}
 * is torchvision's interpolate_embeddings).
 * src is only read; its stream is synchronised first, the new context's before returning.  Refusals come before anything
 * is allocated, leave *out NULL and src untouched: code 1 with a message for a NULL out or src and for what
 * vit_resample_check refuses; code 2 with a message for a target shape this precision and these switches do not run (for
 * instance F32_FP16X2, or $VIT_HIP_P3=0, above 512 tokens) or whose operand slabs would differ in size from src's.  On a
 * failure behind that (out of device memory) the new context is destroyed.
 * Out of scope: weights shared between contexts, antialiased resampling (timm's default: another kernel constant),
 * vit_hip_create_multi, and examples/vit_main.c (which reads the reference's 224-pixel files). */
enum { VIT_POS_BICUBIC = 0, VIT_POS_BILINEAR = 1 };
typedef struct vit_pos_resample { int mode; int align_corners; } vit_pos_resample;   /* NULL = bicubic, align_corners 0 */
/* host only, touches no device: 0 and *out_cfg = *src with the two sides replaced, in the canonical form (out_cfg may be
 * src); 1 with a message for a null or bad argument (a side <= 0 or not a multiple of patch_size, a grid side above 512,
 * unknown mode, align_corners not 0 / 1).  vit_resample_check(src, s, ..) is vit_resample_check_hw(src, s, s, ..). */
int vit_resample_check_hw(const vit_config *src, int img_height, int img_width, const vit_pos_resample *how, vit_config *out_cfg);
int vit_resample_check(const vit_config *src, int img_size, const vit_pos_resample *how, vit_config *out_cfg);
int vit_hip_create_at_size(vit_hip_ctx **out, const vit_hip_ctx *src, int img_height, int img_width, int max_batch,
                           const vit_pos_resample *how);
int vit_hip_create_at_resolution(vit_hip_ctx **out, const vit_hip_ctx *src, int img_size, int max_batch,
                                 const vit_pos_resample *how);

/* FP8_GEMM (BASELINE config 5: "fp8 weights (CDNA4 fp8 MFMA)"): the same four matrices and their inputs as block-scaled
 * fp8 -- OCP "MX": e4m3 elements, one power-of-two scale per 32 consecutive K elements, computed where the tensor
 * is produced (weights at context creation; LayerNorm, the fc1 epilogue and the attention output at run time), so
 * there is NO calibration pass -- on v_mfma_scale_f32_16x16x128_f8f6f4 (twice the bf16 rate; csrc/gemm_mx.hip).
 * Everything else as in BF16_GEMM.  Opt-in ($VIT_HIP_PRECISION=fp8): logits differ from ViT_seq.c at the 1e-1 level
 * (3-bit significands; tests state the tolerance). */

/* F32_FP16X2: everything as in F32 except that the four big projections emulate the fp32 product
 * with two fp16 parts per operand and three matrix-core products (vh_launch_linear_h2) instead of
 * the exact three-part / six-product split.  Operands keep 22 of 24 significant bits; measured
 * class logits stay within the fp32 path's own tolerance of ViT_seq.c (1e-4; tests/test_gpu_parity.py),
 * but it is not an exact fp32 product, so: opt-in, never what `ViT_opencl` uses. */

/* Host-pointer forward: gathers the n separately allocated images into pinned
 * staging, runs them in chunks of <= max_batch, and returns when all outputs
 * are in host memory.  `logits` ([n][num_classes], contiguous) and `probs`
 * (n row pointers, as in the drop-in) may each be NULL. */
int vit_hip_forward(vit_hip_ctx *ctx, const ImageData *images, int n, float *logits,
                    float **probs);

/* Device-resident forward: d_images is [n][C][H][W] fp32 already in HBM (H = img_size, W = the config's width),
 * n <= max_batch; d_logits / d_probs ([n][num_classes] device buffers) may each
 * be NULL.  Asynchronous on `stream`.  A NULL / 0 handle means the CONTEXT'S OWN stream (vit_hip_stream(), created
 * non-blocking), not HIP's legacy null stream: work a caller has queued on the null stream, or on a framework's
 * "current stream" whose handle is 0, is NOT ordered against it -- pass a real stream handle to order against
 * other work on it (bench.py's RCCL gather does). */
int vit_hip_forward_device(vit_hip_ctx *ctx, const float *d_images, int n, float *d_logits,
                           float *d_probs, vh_stream_t stream);

/* ---- 8-bit images (what a JPEG / PNG decoder hands over), normalised on the GPU ----
 * x = (float)u * scale[c] + bias[c]; the product and the sum are each rounded to fp32 (no fused multiply-add), so the
 * logits are bit-identical to the fp32 entry points fed the same images normalised on the host with that arithmetic. */
typedef struct vit_pixel_norm { float scale[4]; float bias[4]; } vit_pixel_norm;
/* [n][H][W][C] as PIL / NumPy / OpenCV give it (RGB order), or [n][C][H][W] as torchvision.io gives it; H = img_size rows,
 * W = the config's width */
enum { VIT_PIXELS_HWC = 0, VIT_PIXELS_CHW = 1 };
/* scale = 1 / (255 std[c]), bias = -mean[c] / std[c], both computed in double and then rounded to float;
 * mean and std on the 0..1 scale, as torchvision's Normalize takes them; chans 1..4, std > 0; returns 0 or 1 */
int vit_pixel_norm_from_mean_std(vit_pixel_norm *out, const float *mean, const float *std, int chans);
/* Device-resident form: d_images contiguous [n][H][W][C] or [n][C][H][W] bytes in HBM, 16-byte aligned, geometry of
 * the context's config (in_chans <= 4), n <= max_batch; otherwise as vit_hip_forward_device.  On the planes paths the
 * patch embedding's gather reads the bytes and normalises them (no fp32 image in HBM); on the fp32-rows paths
 * ($VIT_HIP_P3=0, $VIT_HIP_GEMM_FP32=native, F32_FP16X2) a small kernel expands them first.  Code 1 (with a message, no
 * launch) for a NULL ctx / images / norm, n out of range, an unknown layout, in_chans > 4 or a misaligned pointer. */
int vit_hip_forward_device_u8(vit_hip_ctx *ctx, const unsigned char *d_images, int n, int layout,
                              const vit_pixel_norm *norm, float *d_logits, float *d_probs, vh_stream_t stream);
/* Host form: `images` contiguous in host memory, any n, in chunks of <= max_batch through vit_hip_forward's pipeline
 * (one byte per value crosses PCIe); synchronous; logits and probs as vit_hip_forward, each may be NULL. */
int vit_hip_forward_u8(vit_hip_ctx *ctx, const unsigned char *images, int n, int layout,
                       const vit_pixel_norm *norm, float *logits, float **probs);

/* ---- 8-bit images of any size: resized (shorter side) and centre-cropped on the GPU, bit-exact with Pillow ----
 * Each image: resized to (nh, nw) with the shorter side resize_short (torchvision's Resize(int) arithmetic), then the
 * img x img crop at (round_half_even((nh - img) / 2), likewise for x) (CenterCrop), the pixels those of Pillow's
 * Image.resize((nw, nh), BILINEAR | BICUBIC) on 8-bit channels; then normalised and run exactly as the u8 path.
 * One image: data (device memory in the device forms, host memory in the host form, any alignment); HWC rows of
 * row_stride >= width * in_chans bytes, or CHW planes of height rows of row_stride >= width bytes, height * row_stride
 * bytes apart.  1 <= height, width <= 16384; img <= resize_short <= 4 * img; in_chans <= 4.  The descriptor arrays are
 * host memory in every form.  Code 1 (with a message, no launch) for a NULL argument, n out of range, an unknown filter
 * or layout, an out-of-range size or a row_stride that is too small. */
typedef struct vit_image_u8 { const unsigned char *data; int height, width; long row_stride; } vit_image_u8;
enum { VIT_RESIZE_BILINEAR = 0, VIT_RESIZE_BICUBIC = 1 };
typedef struct vit_resize_crop { int resize_short; int filter; } vit_resize_crop;
/* host only: the resized size and crop offsets of one height x width image for a crop x crop crop; 0, or 1 with a message */
int vit_resize_crop_geometry(int height, int width, const vit_resize_crop *rc, int crop,
                             int *resized_h, int *resized_w, int *top, int *left);
/* The crops alone: [n][img][img][in_chans] bytes (HWC) into d_out; n <= max_batch; asynchronous on `stream` (0 = the
 * context's).  The coefficient tables go into the context's MLP buffer: calls on one context are ordered by their streams. */
int vit_hip_resize_crop_u8(vit_hip_ctx *ctx, const vit_image_u8 *d_images, int n, int layout,
                           const vit_resize_crop *rc, unsigned char *d_out, vh_stream_t stream);
/* resize + crop + vit_hip_forward_device_u8's forward; n <= max_batch; asynchronous like vit_hip_forward_device_u8.  The
 * descriptors travel through a ring of pinned slots, so calls may be queued back to back without a host sync. */
int vit_hip_forward_device_u8_resized(vit_hip_ctx *ctx, const vit_image_u8 *d_images, int n, int layout,
                                      const vit_resize_crop *rc, const vit_pixel_norm *norm,
                                      float *d_logits, float *d_probs, vh_stream_t stream);
/* Host form: any n, through vit_hip_forward's two staging slots; a chunk holds at most max_batch images whose packed bytes
 * (rows without their padding) fit one slot (max_batch x in_chans x img^2 x 4 bytes); a larger image is refused (code 1).
 * Synchronous; logits and probs as vit_hip_forward, each may be NULL. */
int vit_hip_forward_u8_resized(vit_hip_ctx *ctx, const vit_image_u8 *images, int n, int layout,
                               const vit_resize_crop *rc, const vit_pixel_norm *norm, float *logits, float **probs);

/* ---- regions of 8-bit images: boxes resized on the GPU, bit-exact with Pillow's Image.resize(size, resample, box=) ----
 * Detector boxes, the tiles of a slide or satellite frame, five-crop: n boxes of n_images source images (vit_image_u8, as
 * above), each resized to img x img -- a non-square box is squashed, as resize(box=) does -- with the pixels of Pillow's
 * Image.resize((img, img), BILINEAR | BICUBIC, box=(left, top, right, bottom)) on 8-bit channels (2 and 4 channels are
 * independent bands), then normalised and run exactly as the u8 path.  A box: the index of its source in the images array
 * and left, top, right, bottom in source pixel coordinates as C floats (Pillow converts a box to float first); every value
 * finite, 0 <= left, right <= width, 0 <= top, bottom <= height, right - left >= 1 and bottom - top >= 1 (the differences
 * taken in float).  Boxes may repeat a source and name the sources in any order.  Code 1 (with a message, no launch) for a
 * NULL argument, n out of range, n_images < 1, an unknown filter or layout, an image outside vit_image_u8's limits, a
 * row_stride that is too small, a box outside this domain or an image index outside 0 .. n_images - 1: every image and box
 * is checked before anything is queued. */
typedef struct vit_box_u8 { int image; float box[4]; } vit_box_u8;  /* index into the images array; left, top, right, bottom */
int vit_box_check(int height, int width, const float box[4]);        /* host only; 0, or 1 with a message */
/* host only: the source rows [first, first + count) that the `out` output rows of this box read -- the kernel's own bounds */
int vit_box_rows(int height, float top, float bottom, int out, int filter, int *first, int *count);
/* host only: row-major tiling, tile x tile boxes every `stride` px; the last row / column of tiles is moved flush to the
 * bottom / right edge when the stride does not land there, so the image is covered; tile <= min(height, width), 1 <= stride
 * <= tile; returns the number of boxes (written up to `capacity`), -1 with a message on a bad argument */
int vit_tile_boxes(int height, int width, int tile, int stride, int image, vit_box_u8 *out, int capacity);
/* The crops alone: [n][img][img][in_chans] bytes (HWC) into d_out; n <= max_batch boxes; asynchronous on `stream` (0 = the
 * context's); the coefficient tables go into the context's MLP buffer, as vit_hip_resize_crop_u8's. */
int vit_hip_crop_boxes_u8(vit_hip_ctx *ctx, const vit_image_u8 *d_images, int n_images, const vit_box_u8 *boxes, int n,
                          int layout, int filter, unsigned char *d_out, vh_stream_t stream);
/* crops + vit_hip_forward_device_u8's forward; n <= max_batch boxes; asynchronous, the descriptors through the pinned ring
 * like vit_hip_forward_device_u8_resized; armed feature, top-k and attention outputs are written for boxes like for any
 * other image. */
int vit_hip_forward_device_u8_boxes(vit_hip_ctx *ctx, const vit_image_u8 *d_images, int n_images, const vit_box_u8 *boxes,
                                    int n, int layout, int filter, const vit_pixel_norm *norm, float *d_logits,
                                    float *d_probs, vh_stream_t stream);
/* Host form: any n; outputs in box order.  Chunks are consecutive runs of boxes; per chunk every distinct source that its
 * boxes name is packed into the staging slot once, and of it only the rows that the chunk's boxes read (the union of their
 * vit_box_rows spans, at full width; per plane for CHW), so an overlapping tiling uploads every row about once per chunk and
 * a source larger than a slot works.  A chunk is cut at max_batch boxes or when the next box would push the packed bytes
 * past the slot (max_batch x in_chans x img^2 x 4 bytes); a box whose own rows do not fit a slot is refused up front (code
 * 1).  Synchronous; logits and probs as vit_hip_forward, each may be NULL; armed host outputs are served. */
int vit_hip_forward_u8_boxes(vit_hip_ctx *ctx, const vit_image_u8 *images, int n_images, const vit_box_u8 *boxes, int n,
                             int layout, int filter, const vit_pixel_norm *norm, float *logits, float **probs);

/* ---- several GPUs behind one call (the reference takes exactly one device, ViT_opencl.c:803) ----
 * Batch shards only: images never interact (ViT_opencl.c:926), so n images are cut into n_devices
 * contiguous shards (shard s = images [s*ceil(n/G), ...)); every device holds a full replica of the weights
 * and is driven by its own host thread, context and stream; each thread writes its shard's outputs
 * directly into the caller's `logits` / `probs`, so no collective is needed inside one process.
 * `ViT_opencl` takes this path when $VIT_HIP_DEVICES names more than one device ("all" or "0,1,...").
 * A device id may repeat (two replicas on one GPU: used by the single-GPU tests). */
typedef struct vit_hip_multi vit_hip_multi;
int vit_hip_create_multi(vit_hip_multi **out, const vit_config *cfg, const Network *networks, int n_tensors,
                         const int *devices, int n_devices, int max_batch_per_device, int precision);
int vit_hip_forward_multi(vit_hip_multi *m, const ImageData *images, int n, float *logits, float **probs);
void vit_hip_destroy_multi(vit_hip_multi *m);
int vit_hip_multi_devices(const vit_hip_multi *m);
vit_hip_ctx *vit_hip_multi_ctx(const vit_hip_multi *m, int i);
int vit_hip_device(const vit_hip_ctx *ctx);   /* the device a context lives on */
/* Device-resident form with the classifier gather over RCCL (the one exchange of the path; grouped ncclSend / ncclRecv
 * between the devices' compute streams, device 0 of `m` is the root): d_images[g] = shard g's images, [counts[g]][C][H][W]
 * fp32 resident on device g of `m` (counts[g] <= max_batch_per_device); d_logits_root and d_probs_root (may be NULL) =
 * [sum counts][classes] fp32 on device 0, shard after shard.  Synchronous on return -- on success AND on failure (every
 * device's stream is waited for before an error is returned, so the caller may free its buffers).  The shards are
 * enqueued concurrently, one host thread per device.  librccl is opened at run time on first use (an RCCL already in
 * the process, e.g. PyTorch's, is taken); devices must be distinct. */
int vit_hip_forward_device_multi(vit_hip_multi *m, const float *const *d_images, const int *counts, float *d_logits_root,
                                 float *d_probs_root);
/* Host milliseconds each device's thread spent enqueuing its shard in the last vit_hip_forward_device_multi (ms[d] for
 * device d of `m`); returns the device count, -1 if `capacity` is too small. */
int vit_hip_multi_last_enqueue_ms(const vit_hip_multi *m, double *ms, int capacity);
/* The sharding primitives on their own (host logic, no device needed): shard `shard` of [0, total) cut
 * into n_shards contiguous pieces of ceil(total / n_shards); and a runner that calls
 * fn(arg, shard, lo, hi) for every non-empty shard, each on its own host thread, and returns 0 or the
 * first failing shard's status. */
void vit_shard_range(int total, int shard, int n_shards, int *lo, int *hi);
int vit_shard_run(int total, int n_shards, int (*fn)(void *arg, int shard, int lo, int hi), void *arg);
/* ... also reporting the wall time of every shard's fn on its thread (ms_per_shard[n_shards]; may be NULL) */
int vit_shard_run_timed(int total, int n_shards, int (*fn)(void *arg, int shard, int lo, int hi), void *arg, double *ms_per_shard);

/* Introspection for tests / profiling. */
const vit_config *vit_hip_config(const vit_hip_ctx *ctx);
vh_stream_t vit_hip_stream(const vit_hip_ctx *ctx);
int vit_hip_max_batch(const vit_hip_ctx *ctx);
/* Device pointer of weight tensor idx (same index map as `networks`). */
const float *vit_hip_weight(const vit_hip_ctx *ctx, int idx);
/* The last encoder layer behind its attention.  The classifier reads the class-token row of every image only
 * (ViT_seq.c:511) and behind the last attention no operator mixes rows, so on the fp32 path on planes a forward evaluates
 * the last layer's output projection, LayerNorm and MLP for the class-token rows only, with the same kernels and the same
 * k order: logits and probabilities are those of the full evaluation bit for bit.  The other rows stay computable: the
 * forward leaves the pre-projection residual and the attention output in place, and vit_hip_read_tokens runs the full
 * layer's launches on them before it copies, so nothing a caller can read differs from the full evaluation.  An armed
 * request that needs patch rows of the last layer makes its forward run the layer on all rows.  With the resident
 * three-part attention such a forward also runs the last layer's Q projection and attention for the class-token query alone
 * (K and V on all rows; csrc/attention_p3.hip, CLSQ), unless an armed attention-map tap on the last layer or a rollout
 * reads its Q|K|V; vit_hip_read_tokens then runs the QKV projection and the attention again as well.
 * $VIT_HIP_LAST_LAYER at creation: "full" = every forward runs the last layer on all rows (the A/B of tests and benchmarks);
 * "all_queries" = the class-rows path with Q and the attention on all rows.
 * vit_hip_set_last_layer_cls_only is the older switch for the same path ($VIT_HIP_LAST_LAYER=cls sets it at creation): a
 * forward takes the class-rows path when either it or the default asks for it.  It returns the previous setting of its
 * own flag, -1 for a NULL context; fp32 path on planes only (ignored elsewhere). */
int vit_hip_set_last_layer_cls_only(vit_hip_ctx *ctx, int on);

/* ---- feature outputs: class, pooled and patch-token embeddings (the model as a backbone) ----
 * A feature request is ARMED on a context.  While armed, every forward through the context also writes the requested
 * embeddings, read from the fp32 residual stream behind the tapped encoder layers by one memory-bound kernel
 * (csrc/features.hip) in every precision mode; logits and probabilities are bit-identical to an un-armed forward, and an
 * un-armed context launches exactly what it launched before.
 *   taps          encoder layers whose OUTPUT is read: 0-based, or negative from the end (-1 = the last layer); after
 *                 resolution strictly ascending, each in [-depth, depth)
 *   final_norm    1: the model's final LayerNorm (tensors 4 + 12 depth and + 1, cfg.eps) is applied to every tapped row,
 *                 bit-identical to vh_launch_layer_norm on that row; 0: the rows of the residual stream as they are
 *   l2_normalize  1: every class and pooled vector is scaled to unit L2 norm, per tap, before the taps are concatenated
 *                 (a zero vector stays zero)
 *   dtype         VIT_FEATURE_BF16 = the fp32 result rounded to nearest even; nothing else differs
 * Layouts are image-major: cls and pooled are [n][n_taps][E] (per image the taps concatenated in ascending layer order:
 * what a linear probe consumes); tokens is [n][n_taps][T-1][E] (VIT_TOKENS_NLC) or [n][n_taps][E][gh][gw] (VIT_TOKENS_NCHW,
 * the patch grid of vit_config_grid: the memory of [E][T-1]).  The class token is never part of tokens.  pooled = mean over the T-1 patch rows of the values
 * tokens holds BEFORE any narrowing to bf16 (normalise, then pool, when final_norm is set).  Outputs depend on the image
 * only: bit-identical wherever it sits in the batch and whatever n is (fixed-order sums, no floating-point atomics).
 * Device form (vit_hip_set_features): device buffers, 16-byte aligned, for up to max_batch images; written asynchronously
 * on the forward's stream like the logits, by vit_hip_forward_device, _device_u8, _device_u8_resized and _device_u8_boxes.  Host form
 * (vit_hip_set_features_host): host buffers for ALL n images of the coming vit_hip_forward / _u8 / _u8_resized / _u8_boxes calls (each
 * call writes from image 0), complete on return; cls and pooled only -- tokens is refused (308 MB per 512-image chunk
 * through pinned staging).  The host form's staging is allocated when it is armed, not per call.
 * spec == NULL disarms.  Arming one form disarms the other; a device-form forward while the host form is armed (and the
 * reverse) is refused with code 1 and a message, no launch.  Code 1 with a message also for: NULL ctx, n_taps not in
 * 1..4, a tap outside [-depth, depth), taps not ascending and distinct, an unknown dtype or token_layout, all three
 * buffers NULL, a misaligned device buffer, T < 2 with pooled or tokens asked for.  A refused call leaves the previous
 * request armed.
 * The class-rows last layer (vit_hip_set_last_layer_cls_only above): a forward whose armed request needs patch rows of the
 * last layer (pooled or tokens with the last layer among the taps) runs the last layer on all rows; one that needs only cls
 * there uses the compacted class-token rows.  Logits are bit-identical either way.
 * vit_hip_multi: a context from vit_hip_multi_ctx may be armed for the device forms like any other;
 * vit_hip_forward_multi and vit_hip_forward_device_multi neither write features nor refuse. */
enum { VIT_FEATURE_F32 = 0, VIT_FEATURE_BF16 = 1 };
enum { VIT_TOKENS_NLC = 0, VIT_TOKENS_NCHW = 1 };
typedef struct vit_feature_spec
{
    int n_taps;        /* 1..4 */
    int taps[4];
    int final_norm;
    int l2_normalize;
    int dtype;         /* VIT_FEATURE_*: element type of every feature output */
    int token_layout;  /* VIT_TOKENS_* */
} vit_feature_spec;
typedef struct vit_feature_buffers { void *cls, *pooled, *tokens; } vit_feature_buffers;   /* each may be NULL, not all */
/* host only, no device: validates spec against cfg; ELEMENTS PER IMAGE of each output (each pointer may be NULL;
 * pooled and tokens are 0 when T < 2); 0, or 1 with a message */
int vit_feature_sizes(const vit_config *cfg, const vit_feature_spec *spec, size_t *cls_elems, size_t *pooled_elems,
                      size_t *tokens_elems);
int vit_hip_set_features(vit_hip_ctx *ctx, const vit_feature_spec *spec, const vit_feature_buffers *d_bufs);
int vit_hip_set_features_host(vit_hip_ctx *ctx, const vit_feature_spec *spec, const vit_feature_buffers *h_bufs);

/* ---- top-k predictions: the k best labels of every image with their scores, selected on the GPU ----
 * A top-k request is ARMED on a context like a feature request, and independently of it (both may be armed at once).
 * While armed, every forward through the context also writes labels[i][j] (class index of image i's j-th best logit) and,
 * unless scores is NULL, scores[i][j]: its probability (VIT_TOPK_PROBS) or its logit (VIT_TOPK_LOGITS), by one extra launch
 * behind the classifier (vh_launch_topk, csrc/topk.hip; timed under VIT_OP_SOFTMAX).  It reads the fp32 logits only, so it
 * is the same in every precision mode; logits, probabilities and features are bit-identical to an un-armed forward, and an
 * un-armed context launches exactly what it launched before.
 * Ranking (the library's one definition; Main.c:59-72's strict `>` is its k = 1 case): by logit, descending; equal logits
 * by ascending class index -- the lowest index wins; -0.0f and +0.0f are equal; NaN ranks below -inf, NaNs among themselves
 * by ascending index.  The labels of an image are distinct.  1 <= k <= 32, k <= num_classes <= 65536.
 * Scores: VIT_TOPK_LOGITS are the logits' own bits.  VIT_TOPK_PROBS with num_classes <= 2048 are the bits the
 * probabilities output holds at those positions; with more classes they are exp(x - max) / sum over the whole row in a
 * fixed summation order (relative error <= (ceil(num_classes / 256) + 32) * 2^-24).  The full probabilities output itself
 * stays limited to 2048 classes: a forward with probs / d_probs != NULL on a wider head is refused as before (a long-row
 * full softmax is not part of this interface); top-k is the way to read such a head.
 * An image's labels and scores depend on that image only: bit-identical wherever it sits in the batch.
 * Device form (vit_hip_set_topk): device buffers [max_batch][k], 16-byte aligned, written asynchronously on the forward's
 * stream by vit_hip_forward_device, _device_u8, _device_u8_resized and _device_u8_boxes, whether d_logits and d_probs are NULL or not.
 * Host form (vit_hip_set_topk_host): host buffers [n][k] for ALL n images of the coming vit_hip_forward / _u8 / _u8_resized
 * calls (each call writes from image 0), complete on return; two pinned slots of max_batch * k pairs are allocated when it
 * is armed.  With logits == NULL and probs == NULL a chunk's device-to-host traffic is its k pairs per image only.
 * spec == NULL disarms.  Arming one form disarms the other; a device-form forward while the host form is armed (and the
 * reverse) is refused with code 1 and a message, no launch.  Code 1 with a message also for a NULL ctx, a spec
 * vit_topk_check refuses, NULL buffers or labels, a misaligned device buffer.  A refused call leaves the previous request
 * armed.
 * vit_hip_multi: a context from vit_hip_multi_ctx may be armed for the device forms like any other; vit_hip_forward_multi
 * and vit_hip_forward_device_multi neither write top-k outputs nor refuse. */
typedef struct vit_topk_spec { int k; int score_kind; } vit_topk_spec;              /* score_kind: VIT_TOPK_PROBS | VIT_TOPK_LOGITS (kernelHandler.h) */
typedef struct vit_topk_buffers { int *labels; float *scores; } vit_topk_buffers;   /* scores may be NULL */
/* host only, no device: validates spec against cfg; 0, or 1 with a message */
int vit_topk_check(const vit_config *cfg, const vit_topk_spec *spec);
int vit_hip_set_topk(vit_hip_ctx *ctx, const vit_topk_spec *spec, const vit_topk_buffers *d_bufs);
int vit_hip_set_topk_host(vit_hip_ctx *ctx, const vit_topk_spec *spec, const vit_topk_buffers *h_bufs);

/* ---- class-token attention maps: which patches the class token looked at, per head, in any layer ----
 * An attention request is ARMED on a context like a feature or a top-k request, and independently of both (all three may
 * be armed at once).  While armed, every forward through the context also writes, for every tapped layer, the class
 * token's row of that layer's attention matrix, by one extra memory-bound launch (two when both outputs are asked for)
 * between the layer's QKV projection and its attention (vh_launch_cls_attention, csrc/attn_map.hip; timed under
 * VIT_OP_ATTENTION).  It reads the Q|K|V buffer the projection has just completed; no attention kernel is involved, and
 * logits, probabilities, features and top-k outputs are bit-identical to an un-armed forward.  An un-armed context
 * launches exactly what it launched before.
 * Definition.  For image i, tap k (layer l), head h and key t in [0, T), with D = embed_dim / num_heads:
 *     s[t]              = (1/sqrt(D)) * sum_d Q[i*T + 0][h*D + d] * K[i*T + t][h*D + d]
 *     heads[i][k][h][t] = exp(s[t] - max_t s) / sum_t exp(s[t] - max_t s)
 *     mean [i][k][t]    = (sum over h ascending of heads[i][k][h][t], in fp32) / (float)H
 * Q and K are THE VALUES LAYER l'S Q|K|V BUFFER HOLDS IN THIS CONTEXT'S PLAN, decoded exactly to fp32: fp32 rows on the
 * fp32-rows paths and wherever attention streams, the exact three-part split (so again the fp32 values) on the fp32 planes
 * path, values rounded to fp16 in the BF16_GEMM and FP8_GEMM modes' resident and long-sequence plans.  Arithmetic is fp32;
 * the sum over d runs in an order fixed per (D, stored form), the sums over t and h in orders fixed by (T, H) alone.  The
 * output is NOT the probability matrix an attention kernel forms internally (those differ per kernel: exp2 with a folded
 * scale, P rounded to fp16, online softmax); against the definition evaluated in double on the same Q and K a value p
 * errs by at most (4 (D + 2) S + T + 64) 2^-24 p, S = max_t sum_d |q_d k_d| / sqrt(D).
 * Key 0 is the class token itself, so every row of heads (and of mean) sums to 1; keys 1 .. T-1, viewed as [gh][gw]
 * (vit_config_grid), are the map.  taps are those of vit_feature_spec: layers, 0-based or negative from the end, strictly
 * ascending once resolved; here the layer's own attention is read, not its output.
 * Both outputs are fp32 and image-major: heads [n][n_taps][H][T], mean [n][n_taps][T]; either may be NULL, not both, and
 * mean has the same bits whether heads is asked for or not.  No floating-point atomics: an image's output is
 * bit-identical wherever it sits in the batch and whatever n is.  Any T; head_dim a multiple of 16, at most 128 -- anything
 * else is refused when the request is armed, not at the first forward.
 * Device form (vit_hip_set_attention): device buffers for up to max_batch images, 16-byte aligned, written asynchronously
 * on the forward's stream by vit_hip_forward_device, _device_u8, _device_u8_resized and _device_u8_boxes.  Host form
 * (vit_hip_set_attention_host): host buffers for ALL n images of the coming vit_hip_forward / _u8 / _u8_resized / _u8_boxes calls (each
 * call writes from image 0), complete on return; its staging (a device buffer and two pinned slots of max_batch images per
 * output) is allocated when it is armed.
 * spec == NULL disarms.  Arming one form disarms the other; a device-form forward while the host form is armed (and the
 * reverse) is refused with code 1 and a message, no launch.  Code 1 with a message also for: NULL ctx, n_taps not in
 * 1..4, a tap outside [-depth, depth), taps not ascending and distinct, both buffers NULL, a misaligned device buffer, a
 * head_dim the kernel does not take.  A refused call leaves the previous request armed.
 * vit_hip_set_last_layer_cls_only does not matter here: the last layer's Q|K|V is complete either way.
 * vit_hip_multi: a context from vit_hip_multi_ctx may be armed for the device forms like any other; vit_hip_forward_multi
 * and vit_hip_forward_device_multi neither write attention maps nor refuse. */
typedef struct vit_attn_spec { int n_taps; int taps[4]; } vit_attn_spec;        /* taps as in vit_feature_spec */
typedef struct vit_attn_buffers { float *heads, *mean; } vit_attn_buffers;      /* each may be NULL, not both */
/* host only, no device: validates spec against cfg; ELEMENTS PER IMAGE of each output (each pointer may be NULL):
 * n_taps * H * T and n_taps * T; 0, or 1 with a message */
int vit_attn_sizes(const vit_config *cfg, const vit_attn_spec *spec, size_t *heads_elems, size_t *mean_elems);
int vit_hip_set_attention(vit_hip_ctx *ctx, const vit_attn_spec *spec, const vit_attn_buffers *d_bufs);
int vit_hip_set_attention_host(vit_hip_ctx *ctx, const vit_attn_spec *spec, const vit_attn_buffers *h_bufs);

/* ---- attention rollout: the class token's relevance over the patches through all layers (Abnar & Zuidema, 2020) ----
 * A rollout request is ARMED on a context like a feature, a top-k or an attention request, and independently of them (all
 * four may be armed at once).  While armed, every forward through the context also forms, for every layer from
 * first_layer on, the head-averaged attention matrix of that layer, mixes it half and half with the identity for the
 * residual branch, multiplies it into a running T x T product per image, and writes the class token's row of the final
 * product: one or two extra launches per layer between the layer's QKV projection and its attention
 * (vh_launch_rollout_step, csrc/rollout.hip) and one behind the last layer (vh_launch_rollout_read), all timed under
 * VIT_OP_ATTENTION.  They read the Q|K|V buffer the projection has just completed; no attention kernel is involved, and
 * logits, probabilities, features, top-k and attention-map outputs are bit-identical to a forward without rollout armed.
 * A context that has never been armed, or has been disarmed, launches exactly what it launched before.
 * Definition.  For image i and layer l, with D = embed_dim / num_heads, Q and K THE VALUES LAYER l'S Q|K|V BUFFER HOLDS IN
 * THIS CONTEXT'S PLAN decoded exactly to fp32 (the three stored forms of the attention maps above), and `first` =
 * first_layer resolved to a 0-based layer index:
 *     s_h[u][t]  = (1/sqrt(D)) * sum_d Q[i*T+u][h*D+d] * K[i*T+t][h*D+d]      u, t in [0, T)
 *     P_h[u][t]  = exp(s_h[u][t] - max_t s_h[u][.]) / sum_t exp(s_h[u][t] - max_t s_h[u][.])
 *     A_l[u][t]  = (sum over h ascending of P_h[u][t], in fp32) / (float)H
 *     R_first    = 0.5 * A_first + 0.5 * I
 *     R_l        = 0.5 * (A_l . R_{l-1}) + 0.5 * R_{l-1}                        l = first+1 .. depth-1
 *     rollout[i][t] = R_{depth-1}[0][t]
 * All arithmetic is fp32 (the two products on the fp32-input matrix instruction, an exact k-ordered fma chain); every sum
 * runs in an order fixed by (T, H, D, stored form) alone.  No floating-point atomics: an image's output is bit-identical
 * wherever it sits in the batch and whatever n is.  Every R_l is row-stochastic and non-negative, so rollout[i] sums to 1.
 * Key 0 is the class token's own weight; keys 1 .. T-1, viewed as [gh][gw] (vit_config_grid), are the map.  Like the
 * attention maps this is defined on the stored Q|K|V; it is NOT the probabilities any attention kernel forms internally.
 * Against the definition evaluated in double on the same Q and K a value errs by at most
 * rollout * 2^-24 * sum over l of (4 (D + 2) S_l + 2 T + H + 70), S_l = the largest sum_d |q_d k_d| / sqrt(D) of layer l.
 * first_layer: 0-based, or negative from the end, in [-depth, depth).  0 is the standard rollout; a later start discards
 * the early layers (-1: 0.5 * the last layer's head-mean class row + 0.5 at key 0).
 * Output: rollout [n][T] fp32.  Scratch: the two running products and the workspace of a step, 3 * max_batch * T * T * 4
 * bytes of device memory (ViT-B/16 at max_batch 512: 3 x 79 MB; vit_h_14_518 at 64: 3 x 480 MB), allocated when the request
 * is armed and freed when it is disarmed or the context destroyed; if it cannot be allocated, arming is refused.
 * Device form (vit_hip_set_rollout): a device buffer [max_batch][T], 16-byte aligned, written asynchronously on the
 * forward's stream by vit_hip_forward_device, _device_u8, _device_u8_resized and _device_u8_boxes.  Host form
 * (vit_hip_set_rollout_host): a host buffer for ALL n images of the coming vit_hip_forward / _u8 / _u8_resized / _u8_boxes
 * calls (each call writes from image 0), across chunks, complete on return; its staging (a device buffer and two pinned
 * slots of max_batch images) is allocated when it is armed.
 * spec == NULL disarms.  Arming one form disarms the other; a device-form forward while the host form is armed (and the
 * reverse) is refused with code 1 and a message, no launch.  Code 1 with a message also for: NULL ctx, first_layer outside
 * [-depth, depth), a NULL buffer, a misaligned device buffer, a head_dim that is not a multiple of 16 or exceeds 128,
 * embed_dim % 32 != 0 in a plan that stores Q|K|V as planes, more tokens than the kernel takes
 * (vh_rollout_max_tokens(head_dim): 1856 at head_dim 128), scratch that cannot be allocated -- all when the request is
 * armed, not at the first forward.  A refused call leaves the previous request armed.
 * vit_hip_set_last_layer_cls_only does not matter here: the last layer's Q|K|V is complete before its attention either way.
 * vit_hip_multi: a context from vit_hip_multi_ctx may be armed for the device forms like any other; vit_hip_forward_multi
 * and vit_hip_forward_device_multi neither write rollouts nor refuse. */
typedef struct vit_rollout_spec { int first_layer; } vit_rollout_spec;
typedef struct vit_rollout_buffers { float *rollout; } vit_rollout_buffers;   /* [n][T] fp32 */
/* host only, no device: validates spec against cfg; ELEMENTS PER IMAGE of the output (T) and the BYTES PER IMAGE of
 * max_batch of the device scratch an armed request holds (3 * T * T * 4); each pointer may be NULL; 0, or 1 with a message */
int vit_rollout_sizes(const vit_config *cfg, const vit_rollout_spec *spec, size_t *rollout_elems, size_t *scratch_bytes_per_image);
int vit_hip_set_rollout(vit_hip_ctx *ctx, const vit_rollout_spec *spec, const vit_rollout_buffers *d_bufs);
int vit_hip_set_rollout_host(vit_hip_ctx *ctx, const vit_rollout_spec *spec, const vit_rollout_buffers *h_bufs);

/* ---- gallery search: the k nearest entries of a gallery of embeddings the caller holds in device memory ----
 * A gallery request is ARMED on a context like a feature, a top-k, an attention or a rollout request, and independently of
 * them (all five may be armed at once).  While armed, every forward through the context also reads one embedding per
 * image behind layer `tap` and writes, per image, the k rows of the gallery with the largest inner product with it and
 * (optionally) those inner products: retrieval and k-NN classification without the [n][E] embeddings or an n x G product
 * crossing PCIe.  Three extra launches behind the tapped layer (vh_launch_feature_readout, then vh_launch_gallery_topk's
 * two, csrc/gallery.hip), all timed under VIT_OP_HEAD; logits, probabilities, features, top-k, attention maps and rollout
 * are bit-identical to a forward without a gallery armed.  A context that has never been armed, or has been disarmed,
 * launches exactly what it launched before.
 * The query of image i is BY DEFINITION the vector vit_hip_set_features writes for {n_taps = 1, taps = {tap}, final_norm,
 * l2_normalize, VIT_FEATURE_F32} as `cls` (VIT_GALLERY_CLS) or `pooled` (VIT_GALLERY_POOLED), bit for bit; it is produced
 * by the same kernel into a [max_batch][E] fp32 buffer the context holds while armed.  The gallery rows are used as given:
 * a caller who wants cosine similarity stores unit rows (what l2_normalize = 1 features are) and sets l2_normalize.
 * score, ranking, indices and scores: as vh_launch_gallery_topk defines them (include/kernelHandler.h) -- score(i, r) =
 * sum_d query_i[d] * row_r[d] as one fp32 fma chain in an order fixed by embed_dim alone, within (E + 8) * 2^-24 * sum_d
 * |q_d g_d| of the exact product; by score descending, equal scores by ascending row index, NaN last; an image's result is
 * the same bits wherever it sits in the batch and whatever n is.
 * spec: tap is one layer, 0-based or negative from the end (-1 = the last), in [-depth, depth); k in 1..32, k <= n_rows
 * <= 2^31 - 1; dtype VH_GALLERY_F32 or VH_GALLERY_BF16 rows of embed_dim elements, row_stride elements apart (row_stride
 * >= embed_dim, row_stride * element size a multiple of 16); d_rows device memory of the context's device, 16-byte
 * aligned, the CALLER'S, valid and unchanged while armed; embed_dim % 4 == 0, <= 2048.
 * Output: indices [n][k] int32 and scores [n][k] fp32 (scores may be NULL).  Scratch: the queries and the search's
 * workspace, per image of max_batch embed_dim * 4 + min(VH_GALLERY_MAX_SPLITS, ceil(n_rows / 128)) * k * 8 bytes of device
 * memory (ViT-B/16, k = 5, a million rows: 44 KB; k = 32: 265 KB), allocated when the request is armed and freed when it is
 * disarmed or the context destroyed; if it cannot be allocated, arming is refused.
 * Device form (vit_hip_set_gallery): device buffers [max_batch][k], 16-byte aligned, written asynchronously on the
 * forward's stream by vit_hip_forward_device, _device_u8, _device_u8_resized and _device_u8_boxes.  Host form
 * (vit_hip_set_gallery_host): host buffers for ALL n images of the coming vit_hip_forward / _u8 / _u8_resized / _u8_boxes
 * calls (each call writes from image 0), across chunks, complete on return; its staging (device buffers and two pinned
 * slots of max_batch images) is allocated when it is armed.
 * spec == NULL disarms.  Arming one form disarms the other; a device-form forward while the host form is armed (and the
 * reverse) is refused with code 1 and a message, no launch.  Code 1 with a message also for: NULL ctx, a source, tap, k,
 * dtype, n_rows or row_stride outside the above, an embed_dim the search does not take, POOLED on a model without patch
 * tokens, NULL or misaligned d_rows, no indices buffer, a misaligned device buffer, scratch that cannot be allocated -- all
 * when the request is armed, not at the first forward.  A refused call leaves the previous request armed.
 * The class-rows last layer (vit_hip_set_last_layer_cls_only): cls of the last layer reads the compacted class rows; pooled of the last layer
 * makes that forward run the last layer on all rows, as a feature request for pooled does; logits are bit-identical either
 * way.
 * vit_hip_multi: a context from vit_hip_multi_ctx may be armed for the device forms like any other; vit_hip_forward_multi
 * and vit_hip_forward_device_multi neither write gallery results nor refuse.
 * Out of scope: gallery labels and voting (a one-line lookup on the indices), projection heads of another width (CLIP),
 * approximate search, galleries sharded over several GPUs. */
enum { VIT_GALLERY_CLS = 0, VIT_GALLERY_POOLED = 1 };
typedef struct vit_gallery_spec {
    int source;        /* VIT_GALLERY_CLS | VIT_GALLERY_POOLED */
    int tap;           /* one layer, as a vit_feature_spec tap; -1 = the last */
    int final_norm, l2_normalize;   /* as vit_feature_spec */
    int k;
    int dtype;         /* VH_GALLERY_* */
    long n_rows, row_stride;
    const void *d_rows;             /* device memory, the caller's, valid while armed */
} vit_gallery_spec;
typedef struct vit_gallery_buffers { int *indices; float *scores; } vit_gallery_buffers;   /* scores may be NULL */
/* host only, no device: validates spec against cfg (everything above but the pointers); the BYTES PER IMAGE of max_batch of
 * the device scratch an armed request holds; the pointer may be NULL; 0, or 1 with a message */
int vit_gallery_check(const vit_config *cfg, const vit_gallery_spec *spec, size_t *scratch_bytes_per_max_batch_image);
int vit_hip_set_gallery(vit_hip_ctx *ctx, const vit_gallery_spec *spec, const vit_gallery_buffers *d_bufs);
int vit_hip_set_gallery_host(vit_hip_ctx *ctx, const vit_gallery_spec *spec, const vit_gallery_buffers *h_bufs);

/* ---- dense head: a label per pixel from the patch tokens (semantic segmentation by a linear head) ----
 * A dense request is ARMED on a context like the other five requests, and independently of them (all six may be armed at
 * once).  While armed, every forward through the context also applies the caller's linear head W [n_labels][E], b to every
 * patch token behind layer `tap`, upsamples the n_labels logits per patch bilinearly from the gh x gw patch grid
 * (vit_config_grid) to out_h x out_w and writes, per pixel, the best label as one byte: 50 KB per 224 x 224 image instead of
 * the 600 KB of its patch tokens.  Two or three extra launches behind the tapped layer (vh_launch_feature_readout when
 * final_norm is set, vh_launch_dense_logits, vh_launch_dense_labels, csrc/dense_head.hip), all timed under VIT_OP_HEAD;
 * logits, probabilities and the other five requests' outputs are bit-identical to a forward without a dense request.  A
 * context that has never been armed, or has been disarmed, launches exactly what it launched before.
 * The token row x_p of patch p is BY DEFINITION the vector vit_hip_set_features writes as `tokens` for {n_taps = 1, taps =
 * {tap}, final_norm, VIT_FEATURE_F32, VIT_TOKENS_NLC}, bit for bit (the class token is no part of it): with final_norm the
 * same kernel writes them into the MLP buffer, idle behind fc2, when that holds max_batch * (T - 1) * E floats, and into
 * scratch of the request's own otherwise; without, the residual stream's patch rows are read in place.
 * Patch logits, upsampling, labels, scores and their error bound: as vh_launch_dense_logits and vh_launch_dense_labels
 * define them (include/kernelHandler.h), with GH = gh, GW = gw; an image's outputs are the same bits wherever it sits in the
 * batch and whatever n is.
 * spec: tap is one layer, 0-based or negative from the end (-1 = the last), in [-depth, depth); n_labels in 2..256; out_h,
 * out_w in 1..4096, 0 = the model's img_size (out_h) and width (out_w); d_weight [n_labels] rows of embed_dim fp32, weight_stride elements apart
 * (>= embed_dim, a multiple of 4), d_bias [n_labels] fp32 or NULL: device memory of the context's device, 16-byte aligned,
 * the CALLER'S, valid and unchanged while armed.  The model needs embed_dim % 4 == 0, <= 2048, T - 1 == gh * gw >= 1, gh and gw <= 64.
 * Outputs: labels u8 [n][out_h][out_w] (required); scores fp32 [n][out_h][out_w] and patch_logits fp32 [n][T - 1][n_labels]
 * (either may be NULL; asking for them changes no label).  Scratch, allocated when the request is armed and freed when it
 * is disarmed or the context destroyed (if it cannot be allocated, arming is refused): the patch logits [max_batch][T - 1]
 * [n_labels] fp32 when the caller gives no buffer for them, and the normalised tokens as said above; vit_dense_sizes gives
 * an upper bound per image of max_batch ((T - 1) * (n_labels + embed_dim) * 4 bytes).
 * Device form (vit_hip_set_dense): device buffers for max_batch images, 16-byte aligned, written asynchronously on the
 * forward's stream by vit_hip_forward_device, _device_u8, _device_u8_resized and _device_u8_boxes.  Host form
 * (vit_hip_set_dense_host): a host buffer of labels for ALL n images of the coming vit_hip_forward / _u8 / _u8_resized /
 * _u8_boxes calls (each call writes from image 0), across chunks, complete on return; it serves labels only -- scores and
 * patch_logits are refused there, as tokens are for features; its staging is allocated when it is armed.
 * spec == NULL disarms.  Arming one form disarms the other; a device-form forward while the host form is armed (and the
 * reverse) is refused with code 1 and a message, no launch.  Code 1 with a message also for: NULL ctx, a tap, n_labels,
 * out_h, out_w or weight_stride outside the above, a model the head does not take, NULL or misaligned d_weight, misaligned
 * d_bias, no labels buffer, a misaligned device buffer, scratch that cannot be allocated -- all when the request is armed,
 * not at the first forward.  A refused call leaves the previous request armed.
 * The class-rows last layer (vit_hip_set_last_layer_cls_only): a tap on the last layer makes that forward run the last layer on all rows, as a
 * feature request for pooled does; logits are bit-identical either way.
 * vit_hip_multi: vit_hip_forward_multi and vit_hip_forward_device_multi neither write labels nor refuse.
 * Out of scope: the full [C][H][W] probability tensor (the per-pixel confidence, expected value and entropy maps are
 * vit_hip_set_dense_soft, below; for whole frames vit_hip_segment_frame_soft_*), the "linear" (ReLU-normalised) bin
 * strategy of depth heads, a host form of the soft maps, multi-layer or non-linear decode heads, antialiased or bicubic
 * upsampling, more than 256 labels. */
typedef struct vit_dense_spec {
    int tap, final_norm;          /* as vit_gallery_spec */
    int n_labels, out_h, out_w;   /* out_h 0 = the model's img_size, out_w 0 = its width */
    long weight_stride;
    const float *d_weight, *d_bias;   /* device, the caller's; d_bias may be NULL */
} vit_dense_spec;
typedef struct vit_dense_buffers { unsigned char *labels; float *scores, *patch_logits; } vit_dense_buffers;
/* host only, no device: validates spec against cfg (everything above but the pointers); bytes of labels and elements of
 * scores and patch_logits PER IMAGE, and an upper bound on the device scratch per image of max_batch; any pointer may be
 * NULL; 0, or 1 with a message */
int vit_dense_sizes(const vit_config *cfg, const vit_dense_spec *spec, size_t *labels_bytes, size_t *scores_elems,
                    size_t *patch_logits_elems, size_t *scratch_bytes_per_image);
int vit_hip_set_dense(vit_hip_ctx *ctx, const vit_dense_spec *spec, const vit_dense_buffers *d_bufs);
int vit_hip_set_dense_host(vit_hip_ctx *ctx, const vit_dense_spec *spec, const vit_dense_buffers *h_bufs);

/* ---- dense head, soft maps: per-pixel confidence, expected value and entropy ----
 * vit_hip_set_dense_soft arms THE dense request (not a seventh one), in device form, with soft outputs attached: per pixel
 * prob = the softmax probability of the label the dense head writes (a confidence, to threshold or ignore uncertain pixels),
 * expect = sum_c p_c * d_values[c] (dense regression by bins: depth as a linear head over C <= 256 depth bins read out at
 * their centres, the linear depth protocol of DINOv2 and AdaBins' read-out) and entropy = -sum_c p_c ln p_c in nats, with p
 * = softmax_c(logit_scale * v[c]) over the upsampled logits v the labels are ranked from.  vh_launch_dense_soft
 * (include/kernelHandler.h) defines them to the operation and states their error bound.  fp32 [n][out_h][out_w] each.
 * While armed, every vit_hip_forward_device* launches behind layer `tap`, in this order: the feature readout when final_norm
 * is set, vh_launch_dense_logits, vh_launch_dense_labels -- only when a labels buffer was given -- and one
 * vh_launch_dense_soft; all timed under VIT_OP_HEAD.  Class logits, probabilities and the other five requests' outputs are
 * bit-identical to a forward without it; a context that is not soft-armed launches exactly what it launched before.
 * spec: as vit_hip_set_dense takes it.  soft: logit_scale finite and > 0 (1 for a plain softmax; the inverse temperature);
 * d_values [n_labels] fp32 in device memory, 16-byte aligned, the CALLER'S, valid and unchanged while armed -- given exactly
 * when expect is asked for.  d_bufs: may be NULL, or its labels NULL: then no labels are written and vh_launch_dense_labels
 * is not launched (scores then must be NULL too); patch_logits as for vit_hip_set_dense.  d_soft: device buffers for
 * max_batch images, 16-byte aligned; each may be NULL, not all three.
 * It is the dense request in every other respect: vit_hip_set_dense(ctx, NULL, NULL) and vit_hip_set_dense_soft(ctx, NULL,
 * ...) disarm it, arming either form of vit_hip_set_dense replaces it, vit_hip_segment_frame_* refuses while it is armed, a
 * host-form forward refuses, and a tap on the last layer runs all rows under vit_hip_set_last_layer_cls_only.
 * Code 1 with a message that starts with "vit_hip_set_dense_soft: ", the previously armed request untouched and nothing of
 * this call's left allocated: whatever vit_hip_set_dense refuses about spec, a NULL soft or d_soft, all three maps NULL,
 * expect without d_values or the reverse, a logit_scale that is not finite and > 0, a misaligned pointer, scores without
 * labels, scratch that cannot be allocated.
 * There is no host form: fp32 maps are 200 KB per 224 x 224 image, and the host form of the dense request refuses `scores`
 * for the same reason.  vit_dense_soft_check (host only, no device) validates spec against cfg and soft (everything above
 * but the buffers) and gives the elements of one map per image. */
typedef struct vit_dense_soft_spec { float logit_scale; const float *d_values; } vit_dense_soft_spec;
typedef struct vit_dense_soft_buffers { float *prob, *expect, *entropy; } vit_dense_soft_buffers;
int vit_dense_soft_check(const vit_config *cfg, const vit_dense_spec *spec, const vit_dense_soft_spec *soft, size_t *map_elems_per_image);
int vit_hip_set_dense_soft(vit_hip_ctx *ctx, const vit_dense_spec *spec, const vit_dense_soft_spec *soft,
                           const vit_dense_buffers *d_bufs, const vit_dense_soft_buffers *d_soft);

/* ---- whole frames: overlapping windows of one large 8-bit image, their logits blended into one label per frame pixel ----
 * The sliding-window protocol of semantic segmentation (mmseg's mode="slide") in one call: the windows (vit_box_u8 boxes of
 * ONE frame, e.g. from vit_tile_boxes; `image` must be 0) are cut and resized as vit_hip_forward_device_u8_boxes does, run
 * through the model with the dense head `spec->head`, and their patch logits are upsampled to their boxes, averaged where
 * boxes overlap and ranked per frame pixel by vh_launch_dense_stitch (include/kernelHandler.h, which states the definition
 * bit for bit and its error bound): labels u8 [H][W] (required), scores fp32 [H][W] (the winning mean logit; may be NULL),
 * cover u8 [H][W] (how many windows cover the pixel, at most 255; may be NULL); a pixel that no window covers gets
 * fill_label.  Neither the windows' tokens nor any [C][H][W] logits leave the GPU or exist.
 * A call: everything is validated before anything is queued; scratch is allocated (the patch logits of all windows
 * [n_windows][T - 1][n_labels] fp32, one chunk's patch logits, the boxes and the block index; refused with code 1 when that
 * fails); a device-form dense request of the call's own is armed with out_h = out_w = 1 (the per-window label maps that
 * nobody reads shrink to one byte each); the windows run in chunks of at most max_batch through
 * vit_hip_forward_device_u8_boxes on the context's stream, each chunk's patch logits copied device to device to their place
 * behind it (one request armed once: re-arming per chunk would allocate and free the request's scratch per chunk, and a
 * chunk's offset in the frame's buffer is not 16-byte aligned for every T - 1 and n_labels); the request is disarmed, the
 * stitch launched, the stream waited for, the scratch freed.  Both calls are complete on return, and on return -- success or
 * failure -- the context has no dense request armed and holds no allocation of the call's.
 * Requests of the other five kinds armed in device form are served per chunk, as by any forward: their buffers hold the
 * last chunk's outputs afterwards.
 * Device form: d_frame->data and the three output buffers are device memory of the context's device, the outputs 16-byte
 * aligned.  Host form: host memory; the frame is uploaded once, whole (the row packing of vit_hip_forward_u8_boxes is not
 * needed for one frame), the device form runs, and the buffers asked for are copied back.
 * Code 1 with a message, nothing launched: a NULL argument (norm as for the u8 forwards); a dense request of the caller's
 * armed in either form; any request armed in host form; a non-square context; a model or a head vit_hip_set_dense does not
 * take; head.out_h or head.out_w not 0; fill_label outside 0..255; n_windows < 1 or n_windows * (T - 1) >= 2^31 - 128; a frame
 * outside vit_image_u8's limits; a window outside the frame (vit_stitch_check) or with image != 0; an unknown layout or filter;
 * no labels buffer or a misaligned device buffer.
 * Out of scope: tapered blend weights, several frames per call, non-square contexts, vit_hip_multi.  Per-pixel confidence,
 * expected value and entropy: vit_hip_segment_frame_soft_*, below. */
typedef struct vit_frame_spec {
    vit_dense_spec head;   /* tap, final_norm, n_labels, weight_stride, d_weight, d_bias; out_h and out_w must be 0 */
    int fill_label;        /* 0..255: the label of pixels no window covers */
} vit_frame_spec;
typedef struct vit_frame_buffers { unsigned char *labels; float *scores; unsigned char *cover; } vit_frame_buffers; /* [H][W]; labels required */
/* host only, no device: validates spec (everything but the pointers), the frame size and n_windows against cfg; bytes of
 * labels (= of cover; scores are as many floats) and the device scratch of a call without the ids of its block index (4
 * bytes each, vit_stitch_index) and without one chunk's patch logits (max_batch windows'); either pointer may be NULL; 0, or
 * 1 with a message */
int vit_frame_sizes(const vit_config *cfg, const vit_frame_spec *spec, int frame_h, int frame_w, int n_windows,
                    size_t *labels_bytes, size_t *scratch_bytes);
/* host only: every one of the n boxes (l, t, r, b: 4 floats each) is a box of a frame_h x frame_w frame -- vit_box_check's
 * domain, 1 <= frame_h, frame_w <= 16384, n >= 1; 0, or 1 with a message that starts with `who` */
int vit_stitch_check(int frame_h, int frame_w, const float *boxes, int n, const char *who);
/* host only: the block index of vh_launch_dense_stitch.  Blocks of block x block pixels, row-major, blocks_x = ceil(frame_w
 * / block); offsets [blocks_y * blocks_x + 1] and the ids of block k at ids[offsets[k] .. offsets[k + 1]), strictly ascending
 * window indices.  EXACT: a window is listed for a block iff it covers at least one pixel centre of the block (its covered
 * columns and rows are ranges, found with the kernel's own fp32 comparisons).  Returns the number of ids; ids == NULL only
 * sizes (offsets, when given, are still written); more ids than `capacity`, a bad argument or a count of 2^31 or more: -1
 * with a message. */
long vit_stitch_index(int frame_h, int frame_w, int block, const float *boxes, int n, int *offsets, int *ids, long capacity);
int vit_hip_segment_frame_device_u8(vit_hip_ctx *ctx, const vit_image_u8 *d_frame, const vit_box_u8 *windows, int n_windows,
                                    int layout, int filter, const vit_pixel_norm *norm, const vit_frame_spec *spec,
                                    const vit_frame_buffers *d_out);
int vit_hip_segment_frame_u8(vit_hip_ctx *ctx, const vit_image_u8 *frame, const vit_box_u8 *windows, int n_windows,
                             int layout, int filter, const vit_pixel_norm *norm, const vit_frame_spec *spec,
                             const vit_frame_buffers *h_out);

/* ---- whole frames, soft maps: per-pixel confidence, expected value and entropy of a large frame ----
 * The same protocol followed by its softmax -- average the windows' logits, then softmax: sliding-window depth by bins, or a
 * mask of uncertain pixels, on a 4000 x 3000 frame.  vit_hip_segment_frame_soft_* run the windows exactly as
 * vit_hip_segment_frame_* do and write, per frame pixel, prob / expect / entropy as vit_hip_set_dense_soft defines them on
 * the blended mean logits (vh_launch_dense_stitch_soft, include/kernelHandler.h: the definition bit for bit and its error
 * bound); fp32 [H][W] each, each may be NULL, not all three; a pixel that no window covers is 0x7FC00000 in every map.
 * soft: logit_scale and d_values as vit_hip_set_dense_soft takes them; d_values is DEVICE memory in both forms, as the head's
 * d_weight is.  d_out (h_out) may be NULL, or its labels NULL: then vh_launch_dense_stitch is not launched; scores and cover
 * need labels.  Labels, scores and cover are vit_hip_segment_frame_*'s bits.
 * A call: everything is validated; the scratch of vit_hip_segment_frame_* is allocated, with one block index per stitch
 * launch (each launcher copies its index synchronously: one scratch per launch in flight); the windows run as there; the
 * request is disarmed; vh_launch_dense_stitch where labels are asked for, then vh_launch_dense_stitch_soft, both timed under
 * VIT_OP_HEAD; the stream is waited for and the scratch freed.  On return -- success or failure -- the context has no dense
 * request armed and holds no allocation of the call's.  The host form uploads the frame once, runs the device form and
 * copies back what was asked for.
 * Code 1 with a message that starts with the entry point's name, nothing queued: whatever vit_hip_segment_frame_* refuse
 * (but for the labels buffer), whatever vit_hip_set_dense_soft refuses about soft and the maps (a NULL soft or d_soft, all
 * three maps NULL, expect without d_values or the reverse, a logit_scale that is not finite and > 0, a misaligned d_values or
 * device map), scores or cover without labels.  vit_frame_soft_check (host only, no device) validates spec, soft, the frame
 * size and n_windows against cfg and gives the elements of one map.
 * Out of scope: the full [C][H][W] probabilities, tapered blend weights, several frames per call, vit_hip_multi. */
int vit_frame_soft_check(const vit_config *cfg, const vit_frame_spec *spec, const vit_dense_soft_spec *soft, int frame_h,
                         int frame_w, int n_windows, size_t *map_elems);
int vit_hip_segment_frame_soft_device_u8(vit_hip_ctx *ctx, const vit_image_u8 *d_frame, const vit_box_u8 *windows, int n_windows,
                                         int layout, int filter, const vit_pixel_norm *norm, const vit_frame_spec *spec,
                                         const vit_dense_soft_spec *soft, const vit_frame_buffers *d_out,
                                         const vit_dense_soft_buffers *d_soft);
int vit_hip_segment_frame_soft_u8(vit_hip_ctx *ctx, const vit_image_u8 *frame, const vit_box_u8 *windows, int n_windows,
                                  int layout, int filter, const vit_pixel_norm *norm, const vit_frame_spec *spec,
                                  const vit_dense_soft_spec *soft, const vit_frame_buffers *h_out,
                                  const vit_dense_soft_buffers *h_soft);

/* Debug hook: copy the residual stream of the last forward ([n*tokens][embed], un-normalised) to the host.  Where that
 * forward ran the last layer behind its attention on the class-token rows only, the full layer's launches run on all rows of
 * its images first, on the context's stream: the rows are those of the full evaluation, bit for bit; a second read runs
 * nothing.  As for the copy itself, a forward the caller put on a stream of its own must have completed.  The supported interface to the encoder's output is vit_hip_set_features above. */
int vit_hip_read_tokens(vit_hip_ctx *ctx, int n, float *host_out);
/* Images of the last forward whose last layer still waits to be finished on all rows (0: none; -1: NULL context) */
int vit_hip_last_layer_pending(const vit_hip_ctx *ctx);

/* Per-operator timing with HIP events recorded on the launch stream (the capability
 * behind the reference's dead profileEvents/printEventProfile, ViT_opencl.c:988-1048).
 * enable(ctx, k) sizes an event pool for k forwards (0 disables); read() waits for
 * the recorded launches, returns the summed milliseconds and launch counts per
 * operator class since the last read, and rewinds the pool. */
enum vit_op_class
{
    VIT_OP_PATCH_EMBED = 0, /* patch-embed GEMM + class-token rows */
    VIT_OP_LAYER_NORM,      /* every LayerNorm (2 per layer + final) */
    VIT_OP_QKV,             /* fused Q|K|V projection GEMM */
    VIT_OP_ATTENTION,       /* softmax(QK^T/sqrt(D))V */
    VIT_OP_OUT_PROJ,        /* attention output projection + residual */
    VIT_OP_FC1,             /* MLP fc1 + GELU */
    VIT_OP_FC2,             /* MLP fc2 + residual */
    VIT_OP_HEAD,            /* classifier GEMM */
    VIT_OP_SOFTMAX,         /* class softmax */
    /* the last layer on the class-token rows only: n-row launches, kept apart so that the means of the classes above stay
     * those of full-size launches (that layer's LayerNorm is timed with the LayerNorms, like the final one) */
    VIT_OP_OUT_PROJ_CLS,    /* two row gathers + output projection + residual */
    VIT_OP_FC1_CLS,
    VIT_OP_FC2_CLS,
    VIT_OP_COUNT
};
int vit_hip_profile_enable(vit_hip_ctx *ctx, int max_forwards);
int vit_hip_profile_read(vit_hip_ctx *ctx, double ms_sum[VIT_OP_COUNT], long launches[VIT_OP_COUNT]);
/* Record only the operator classes in `op_mask` (bit i = vit_op_class i; 0 = all).  Two event
 * packets per recorded launch sit between kernels and cost ~2 % of a step when every launch is
 * recorded; a throughput run records the one kernel its roofline is quoted on. */
int vit_hip_profile_select(vit_hip_ctx *ctx, unsigned op_mask);

/* Result file in Main.c's format (Main.c:59-72: "[%d] label: %d / prob: %.6f", arg-max restarted
 * per image) and a comparison stricter than comparator.c:74-86 (label equal and |dprob| <= 0.01):
 * largest / mean absolute difference, top-1 agreement, top-1 agreement not counting rows whose
 * reference margin between the two classes is within twice `tolerance`, mean
 * top-5 overlap, and the number of non-finite differences.  `got` / `want` are [rows][classes]. */
typedef struct {
    int rows, classes;
    double max_abs_diff, mean_abs_diff;
    int top1_equal, top1_equal_or_near_tie;
    double top5_overlap;
    int nonfinite;
} vit_compare_report;
int vit_write_result_file(const char *path, float *const *probabilities, int n, int classes);
/* The same file from top-k outputs ([n][k], k >= 1): line i holds labels[i][0] and scores[i][0].  Byte-identical to
 * vit_write_result_file on the full rows the columns were selected from (the lowest index wins a tie in both). */
int vit_write_result_file_topk(const char *path, const int *labels, const float *scores, int n, int k);
int vit_compare_rows(const float *got, const float *want, int n, int classes, double tolerance,
                     vit_compare_report *rep);

/* Deterministic synthetic data (counter-based integer PRNG -> exact fp32; no
 * libm): dst[i] = offset + scale * u_i, u_i uniform in [-1,1) on a 2^-23 grid,
 * fully determined by (seed, i).  Shared by tests, bench and the oracle
 * harness so inputs are regenerated instead of stored. */
void vit_synth_fill(float *dst, size_t count, unsigned long long seed, float scale, float offset);
/* The synthetic-weight recipe of SURVEY 8d for tensor idx of cfg
 * (seed = seed_base + idx); writes vit_config_tensor_size(cfg, idx) floats. */
void vit_synth_tensor(const vit_config *cfg, int idx, unsigned long long seed_base, float *dst);
/* Synthetic image: uniform in [-2,2), seed = 1000 + image_index. */
void vit_synth_image(const vit_config *cfg, int image_index, float *dst);

#ifdef __cplusplus
}
#endif

#endif /* VIT_HIP_VIT_OPENCL_H */
