/*
 * kernelHandler.h -- C ABI of the HIP device shim (libvit_hip.so).
 *
 * This is the replacement for the reference's OpenCL runtime glue
 * (MulticoreMainProject/kernelHandler.h:6-18, kernelHandler.c:15,35) plus the
 * clSetKernelArg/clEnqueueNDRangeKernel wrappers in ViT_opencl.c:361-779.
 * The reference loads .cl text at run time (get_source_code) and JIT-builds it
 * (build_error prints the log); here every kernel is compiled ahead of time
 * for gfx950 and reached through one `vh_launch_*` entry per kernel.
 *
 * Everything is extern "C" with plain pointers and sizes: host code stays C.
 * Device pointers are ordinary `float *` values that must not be dereferenced
 * on the host.  All launchers are asynchronous on `stream` (0 = the null
 * stream) and return 0 on success or a non-zero hipError_t value; the text of
 * the most recent failure on the calling thread is at vh_last_error().
 *
 * There is no CPU fallback anywhere behind this header: without a usable
 * gfx950 device vh_init() fails and every launcher returns an error.
 */
#ifndef VIT_HIP_KERNELHANDLER_H
#define VIT_HIP_KERNELHANDLER_H

#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *vh_stream_t; /* hipStream_t */
typedef void *vh_event_t;  /* hipEvent_t  */

/* Mirrors CHECK_ERROR (reference kernelHandler.h:6-10): print where, then
 * exit(EXIT_FAILURE).  Used by the drop-in ViT_opencl(), which has no way to
 * return a status; the extended vit_hip_* API returns the code instead. */
#define VH_CHECK(err)                                                          \
    do {                                                                       \
        int vh_check_err_ = (err);                                             \
        if (vh_check_err_ != 0) {                                              \
            printf("[%s:%d] HIP error %d: %s\n", __FILE__, __LINE__,           \
                   vh_check_err_, vh_last_error());                            \
            exit(EXIT_FAILURE);                                                \
        }                                                                      \
    } while (0)

/* ---- runtime (replaces clGetPlatformIDs..clCreateCommandQueue, ViT_opencl.c:799-861) ---- */
int vh_device_count(void);                 /* number of visible HIP devices (0 if none / no driver) */
int vh_init(int device);                   /* select `device`; fails unless it is a gfx950 part */
const char *vh_last_error(void);           /* text of the last failure on this thread ("" if none) */
int vh_set_error(int code, const char *message);   /* record `message` as this thread's last error; returns code (1 if 0) */
const char *vh_device_name(void);          /* e.g. "AMD Instinct MI355X (gfx950, 256 CUs)" */
int vh_set_device(int device);             /* make `device` current for the calling thread (after vh_init) */

int vh_stream_create(vh_stream_t *out);
int vh_stream_destroy(vh_stream_t s);
int vh_stream_sync(vh_stream_t s);         /* replaces clFinish */
int vh_device_sync(void);

int vh_event_create(vh_event_t *out);
int vh_event_destroy(vh_event_t e);
int vh_event_record(vh_event_t e, vh_stream_t s);
int vh_stream_wait_event(vh_stream_t s, vh_event_t e); /* work queued on s after this waits for e */
int vh_event_sync(vh_event_t e);
int vh_event_elapsed_ms(float *ms, vh_event_t start, vh_event_t stop);

/* ---- memory (replaces clCreateBuffer / clEnqueueWriteBuffer / clEnqueueReadBuffer,
 *      ViT_opencl.c:125-357, :371, :775) ---- */
int vh_malloc(void **out, size_t bytes);
int vh_free(void *p);
int vh_host_alloc(void **out, size_t bytes); /* pinned host memory for async copies */
int vh_host_free(void *p);
int vh_memset(void *dst, int value, size_t bytes, vh_stream_t s);
int vh_h2d(void *dst, const void *src, size_t bytes, vh_stream_t s); /* async w.r.t. host iff src is pinned */
int vh_d2h(void *dst, const void *src, size_t bytes, vh_stream_t s);
int vh_d2d(void *dst, const void *src, size_t bytes, vh_stream_t s);

/* ---- kernels: one launcher per HIP kernel ---- */

/* Patch embedding, fused with flatten/transpose, class-token prepend and
 * position-embedding add.  Replaces Conv2d + postConv2d (ViT_opencl.c:361-442;
 * kernels conv2d_kernel conv2d.cl:1 and postprocess conv2d.cl:39; CPU
 * Conv2d_seq..pos_emb_seq ViT_seq.c:25-118).
 *   images   [n_images][in_chans][img][img]  fp32, contiguous
 *   conv_w   [embed][in_chans][patch][patch], conv_b [embed]
 *   cls      [embed], pos [tokens][embed]   (tokens = (img/patch)^2 + 1)
 *   tokens   [n_images][tokens][embed]      output */
int vh_launch_patch_embed(vh_stream_t s, const float *images, const float *conv_w,
                          const float *conv_b, const float *cls_token, const float *pos_embed,
                          float *tokens, int n_images, int in_chans, int img_size,
                          int patch_size, int embed_dim);

/* The same for patch geometries whose rows cannot be gathered on load (patch % 4 != 0 or
 * in_chans*patch*patch % 32 != 0 -- ViT-H/14: 3*14*14 = 588): patches are gathered once
 * into zero-padded rows in `workspace` (vh_patch_embed_workspace() bytes, 16-byte aligned;
 * 0 for geometries vh_launch_patch_embed takes directly, which then ignores the workspace). */
size_t vh_patch_embed_workspace(int n_images, int in_chans, int img_size, int patch_size, int embed_dim);
int vh_launch_patch_embed_ws(vh_stream_t s, const float *images, const float *conv_w,
                             const float *conv_b, const float *cls_token, const float *pos_embed,
                             float *tokens, int n_images, int in_chans, int img_size,
                             int patch_size, int embed_dim, void *workspace, size_t workspace_bytes);

/* The patch embedding of the reduced-precision modes (bf16 / fp8 GEMM operands; conv2d.cl:1-80 for them): an im2row
 * producer writes the patches as one-part bf16 planes [Kp/32][1][n_images*grid^2][32] into `workspace` (Kp =
 * vh_patch_planes_k(): in_chans*patch^2 padded with zeros to the one-part K step; Kp * 2 bytes per patch row), and
 * the planes GEMM (vh_launch_linear_planes, parts = 1) runs with a token-row epilogue.  `conv_w_planes` =
 * [Kp/32][1][embed][32], written once by vh_launch_conv_weight_planes.  fp32 accumulation, bias, position
 * embedding and class-token rows as vh_launch_patch_embed; pixels and weights are rounded to bf16.  embed % 128 == 0. */
int vh_patch_planes_k(int in_chans, int patch_size);
int vh_launch_conv_weight_planes(vh_stream_t s, const float *conv_w, void *planes, int embed_dim, int in_chans, int patch_size);
/* ... with `parts` parts per value: 1 as above, 3 = the exact fp32 split [Kp/32][3][embed][32] for vh_launch_patch_embed_planes3 */
int vh_launch_conv_weight_planes_parts(vh_stream_t s, const float *conv_w, void *planes, int embed_dim, int in_chans, int patch_size,
                                       int parts);
/* The fp32 path's patch embedding on the planes kernel: the im2row producer writes the exact three-part split of the pixels
 * (workspace: n_images*grid^2 * Kp * 6 bytes), six bf16 products per block as vh_launch_linear_p3 -- no operand is split inside
 * a K loop.  Same arguments as vh_launch_patch_embed_planes. */
int vh_launch_patch_embed_planes3(vh_stream_t s, const float *images, const void *conv_w_planes3, const float *conv_b,
                                  const float *cls_token, const float *pos_embed, float *tokens, int n_images, int in_chans,
                                  int img_size, int patch_size, int embed_dim, void *workspace, size_t workspace_bytes);
int vh_launch_patch_embed_planes(vh_stream_t s, const float *images, const void *conv_w_planes, const float *conv_b,
                                 const float *cls_token, const float *pos_embed, float *tokens, int n_images,
                                 int in_chans, int img_size, int patch_size, int embed_dim, void *workspace,
                                 size_t workspace_bytes);

/* Row LayerNorm, y = (x-mean)*inv_std*w + b with var = E[x^2]-mean^2 and
 * inv_std = 1/sqrt(var+eps) (eps added in double, ViT_seq.c:21,135).
 * Replaces layer_norm (ViT_opencl.c:444-482; layerNorm layer_norm.cl:3; CPU
 * layer_norm_seq ViT_seq.c:120).  Row r is read at input + r*in_row_stride and
 * written at output + r*out_row_stride (strides in floats), so the final
 * norm can run on the class-token rows only. */
int vh_launch_layer_norm(vh_stream_t s, const float *input, const float *weight,
                         const float *bias, float *output, int rows, int embed_dim,
                         long in_row_stride, long out_row_stride, double eps);

/* output[rowA][colB] = input[rowA][colA] . weight[colB][colA]^T + bias[colB],
 * optionally followed by exact-erf GELU, optionally adding `residual`
 * (same shape as output; may alias output).  Argument order and names follow
 * the reference kernel linear_layer (ll.cl:7-16) and its host wrapper
 * (ViT_opencl.c:622-672); it also replaces QKV (multihead.cl:3, colB = 3*embed,
 * output rows are Q|K|V side by side) and encoderResidual (layer_norm.cl:55).
 * CPU: linear_layer_seq ViT_seq.c:295, gelu :283, residual loops :348,:360. */
int vh_launch_linear(vh_stream_t s, float *output, const float *weight, const float *input,
                     const float *bias, int rowA, int colA, int colB, int doGelu,
                     const float *residual);
/* ... and vh_launch_patch_embed_ws, with the arithmetic of the fp32 products named: the exact three-part bf16 split on the
 * bf16 matrix cores (what the two entries above run), or the native fp32 matrix instruction.  Ragged colB (% 128 != 0) and
 * pointers that are not 16-byte aligned run natively under either. */
enum { VH_FP32_SPLIT3 = 0, VH_FP32_NATIVE = 1 };
int vh_launch_linear_math(vh_stream_t s, float *output, const float *weight, const float *input, const float *bias,
                          int rowA, int colA, int colB, int doGelu, const float *residual, int fp32_math);
int vh_launch_patch_embed_ws_math(vh_stream_t s, const float *images, const float *conv_w, const float *conv_b,
                                  const float *cls_token, const float *pos_embed, float *tokens, int n_images, int in_chans,
                                  int img_size, int patch_size, int embed_dim, void *workspace, size_t workspace_bytes,
                                  int fp32_math);

/* The same product with the weight pre-split: `weight_planes` holds the exact three-way split
 * w = p0 + p1 + p2 as bfloat16, laid out [colA/32][3][colB][32] (K step, part, row, element: what one K
 * step of a tile reads is contiguous), written once by vh_launch_split3_planes (the fp32 GEMM forms
 * every product from such parts on the bf16 matrix cores; splitting the constant operand ahead
 * of time leaves only the activations to split in the inner loop).  Same results as
 * vh_launch_linear bit for bit.  colB % 128 == 0. */
int vh_launch_split3_planes(vh_stream_t s, const float *weight, void *planes, int rows, int cols);
int vh_launch_linear_w3(vh_stream_t s, float *output, const void *weight_planes, const float *input,
                        const float *bias, int rowA, int colA, int colB, int doGelu,
                        const float *residual);

/* ---- both operands pre-split ("P3"): the default fp32 path of the four big projections ----
 * The exact three-way split x = p0 + p1 + p2 of an fp32 matrix [rows][cols], stored as bfloat16 planes
 *     planes[cols/32][3][rows][32]      (K step, part, row, element; 6 bytes per value)
 * -- the layout vh_launch_split3_planes gives the weights.  When the PRODUCER of a GEMM input writes
 * this format (vh_launch_layer_norm_p3, vh_launch_attention_p3, vh_launch_linear_p3 with output_planes),
 * the GEMM's K loop contains no split arithmetic at all: matrix instructions, LDS reads and loads only
 * (csrc/gemm_p3.hip).  Same six partial products per block, in the same order, as vh_launch_linear /
 * vh_launch_linear_w3: results are identical bit for bit.  No reference counterpart (format plumbing
 * around ll.cl:7 / multihead.cl:3 / layer_norm.cl:3); rows < 2^26, cols % 32 == 0, 16-byte aligned. */
int vh_launch_split3_rows(vh_stream_t s, const float *input, void *planes, int rows, int cols);
int vh_launch_merge3_rows(vh_stream_t s, const void *planes, float *output, int rows, int cols); /* exact inverse */
/* The same format with `parts` parts per value: 3 as above, or 1 = values rounded to bfloat16 (the operands of
 * the bf16-operand mode, BASELINE config 3), planes[cols/32][1][rows][32]: the same GEMM kernel takes both. */
int vh_launch_split_rows(vh_stream_t s, const float *input, void *planes, int rows, int cols, int parts);
int vh_launch_merge_rows(vh_stream_t s, const void *planes, float *output, int rows, int cols, int parts);
/* vh_launch_layer_norm writing planes [embed_dim/32][parts][rows][32]: embed_dim % 32 == 0 and at most
 * vh_layer_norm_planes_max_embed(parts) -- 2048 with one part, 1696 with three: the kernel stages 16 rows of every part
 * in LDS, 32 * parts * embed_dim bytes of a CU's 160 KiB.  Wider rows are refused before any launch. */
int vh_layer_norm_planes_max_embed(int parts);   /* 0 for parts other than 1 and 3 */
int vh_launch_layer_norm_planes(vh_stream_t s, const float *input, const float *weight, const float *bias,
                                void *out_planes, int parts, int rows, int embed_dim, long in_row_stride, double eps);
int vh_launch_attention_planes_bf16(vh_stream_t s, const float *qkv, void *out_planes, int n_images, int tokens,
                                    int embed_dim, int num_heads);   /* one-part planes, arithmetic of vh_launch_attention_f16 */
/* colA % 64 == 0 (parts 3) or % 128 == 0 (parts 1); fp32 accumulation, bias, GELU, residual as vh_launch_linear.
 * output_planes: 0 = fp32 rows [rowA][colB]; 1 = planes of `parts` parts (no residual); 2 (parts 1, no GELU, no
 * residual) = one-part planes of FP16 values [colB/32][rowA][32] -- the Q|K|V input of vh_launch_attention_planes_f16 */
int vh_launch_linear_planes(vh_stream_t s, void *output, int output_planes, const void *weight_planes,
                            const void *input_planes, int parts, const float *bias, int rowA, int colA, int colB,
                            int doGelu, const float *residual);
/* vh_launch_layer_norm writing planes [embed_dim/32][3][rows][32]: vh_launch_layer_norm_planes with parts = 3, embed_dim <= 1696 */
int vh_launch_layer_norm_p3(vh_stream_t s, const float *input, const float *weight, const float *bias,
                            void *out_planes, int rows, int embed_dim, long in_row_stride, double eps);
/* vh_launch_attention writing planes [embed_dim/32][3][n_images*tokens][32] (head_dim 64, tokens <= 208) */
int vh_launch_attention_p3(vh_stream_t s, const float *qkv, void *out_planes, int n_images, int tokens,
                           int embed_dim, int num_heads);
/* The same attention on PRE-SPLIT Q, K, V: qkv_planes [3*embed_dim/32][3][n_images*tokens][32] (the QKV projection
 * written by vh_launch_linear_p3 with output_planes), out_planes as above; same results bit for bit, no split
 * arithmetic left but that of the probabilities (csrc/attention_p3.hip).  head_dim 64, tokens <= 208. */
int vh_launch_attention_planes(vh_stream_t s, const void *qkv_planes, void *out_planes, int n_images, int tokens,
                               int embed_dim, int num_heads);
/* The reduced-precision modes' attention on planes: qkv_planes_f16 [3*embed_dim/32][n_images*tokens][32] fp16 (the QKV
 * projection with output_planes = 2, or vh_launch_linear_mx_planes_f16); output = one-part bf16 planes
 * [embed_dim/32][rows][32] (output_planes != 0) or fp32 rows [rows][embed_dim].  Arithmetic of vh_launch_attention_f16
 * (same results bit for bit on the same fp16 values); head_dim 64, tokens <= 208. */
int vh_launch_attention_planes_f16(vh_stream_t s, const void *qkv_planes_f16, void *output, int output_planes,
                                   int n_images, int tokens, int embed_dim, int num_heads);
/* The same arithmetic for ViT-H/14's shape (head_dim 80, tokens <= 272) with one head's K and V resident in LDS
 * (csrc/attention_h16.hip): qkv_planes_f16 as above -> fp32 rows [n_images*tokens][embed_dim]. */
int vh_launch_attention_planes_f16_hd80(vh_stream_t s, const void *qkv_planes_f16, float *output, int n_images,
                                        int tokens, int embed_dim, int num_heads);
/* ... writing the output projection's operand directly: output_kind 1 = one-part bf16 planes [embed_dim/32][rows][32], 2 =
 * the block-scaled fp8 tensor (values + out_scales); the fp32 result followed by vh_launch_split_rows(parts = 1) /
 * vh_launch_quantize_mx_rows, byte for byte.  head_dim 80, num_heads even, tokens <= 272. */
int vh_launch_attention_planes_f16_hd80_operand(vh_stream_t s, const void *qkv_planes_f16, void *output, void *out_scales,
                                                int output_kind, int n_images, int tokens, int embed_dim, int num_heads);
/* Attention for any token count (csrc/attention_long.hip: flash-style, K and V stream through LDS in 64-key chunks, online
 * softmax; nothing grows with tokens).  qkv_planes: the QKV projection's planes, parts 3 = the exact three-part bf16 split
 * [3*embed_dim/32][3][rows][32] (the fp32 path; fp32 products of the splits), parts 1 = one-part fp16 [3*embed_dim/32][rows][32]
 * (the reduced modes; the arithmetic of vh_launch_attention_f16).  output: fp32 rows [rows][embed_dim], rows =
 * n_images*tokens.  head_dim 64 or 80, embed_dim % 32 == 0 (an even head count at head_dim 80), tokens >= 1, pointers
 * 16-byte aligned; anything else: code 1 with a message, no launch.  A row's result depends on its own image and head alone
 * (no split over keys, no atomics): the same bits alone and in a batch. */
int vh_launch_attention_long(vh_stream_t s, const void *qkv_planes, int parts, float *output, int n_images, int tokens,
                             int embed_dim, int num_heads);
/* vh_launch_linear on planes: input_planes [colA/32][3][rowA][32], weight_planes [colA/32][3][colB][32];
 * output fp32 [rowA][colB], or (output_planes != 0, no residual) planes [colB/32][3][rowA][32].
 * colA % 64 == 0, colB % 128 == 0. */
int vh_launch_linear_p3(vh_stream_t s, void *output, int output_planes, const void *weight_planes,
                        const void *input_planes, const float *bias, int rowA, int colA, int colB,
                        int doGelu, const float *residual);
/* colB consecutive output features of a projection that has w_features of them (no GELU, no residual): weight_planes points
 * at the first of them inside the whole matrix's planes [colA/32][3][w_features][32] (64 bytes per feature), bias at its
 * entry; output is these columns' own, fp32 [rowA][colB] or planes [colB/32][3][rowA][32].  The kernels and the k order of
 * vh_launch_linear_p3 on the whole matrix: the same bits in these columns.  w_features >= colB. */
int vh_launch_linear_p3_cols(vh_stream_t s, void *output, int output_planes, const void *weight_planes, int w_features,
                             const void *input_planes, const float *bias, int rowA, int colA, int colB);
/* vh_launch_attention_planes for the class-token query (row 0) of every image alone, as the last layer needs it:
 * qkv_planes as there, of which only K and V are read; q_cls_planes [embed_dim/32][3][n_images][32], the Q planes of the
 * n_images class rows; out_cls_planes [embed_dim/32][3][n_images][32].  One wave computes the query tile that holds the
 * class query, its other 31 columns loaded as zeros, with the products, the key mapping, the softmax and the P.V order of
 * the full kernel: row i of the output is row i * tokens of vh_launch_attention_planes' on the same Q|K|V, bit for bit. */
int vh_launch_attention_planes_cls(vh_stream_t s, const void *qkv_planes, const void *q_cls_planes, void *out_cls_planes,
                                   int n_images, int tokens, int embed_dim, int num_heads);

/* fp32 emulation with two fp16 parts per operand and three products (the "3 x TF32" scheme on
 * fp16: a = a0 + a1 + eps, |eps| <= 2^-22 |a|; a.w ~ a0w0 + a0w1 + a1w0, fp32 accumulation).  NOT
 * exact -- operands keep 22 of their 24 significant bits -- but its truncation error (~8e-8 of the
 * result) is an order of magnitude below the rounding noise of an fp32 accumulation, at half
 * the matrix-core work of the exact split.  `weight_planes` = [colA/32][2][colB][32] fp16 of
 * weight * weight_scale (a power of two that lifts the low part out of fp16's subnormal range;
 * vh_launch_split2h_planes); inputs must stay below 65504 in magnitude.  Opt-in (ViT_opencl.h). */
int vh_launch_split2h_planes(vh_stream_t s, const float *weight, void *planes, int rows, int cols, float scale);
int vh_launch_linear_h2(vh_stream_t s, float *output, const void *weight_planes, float weight_scale,
                        const float *input, const float *bias, int rowA, int colA, int colB,
                        int doGelu, const float *residual);
int vh_launch_attention_h2(vh_stream_t s, const float *qkv, float *output, int n_images, int tokens,
                           int embed_dim, int num_heads);   /* Q.K^T and P.V likewise */

/* Scaled-dot-product attention over the fused QKV rows produced by
 * vh_launch_linear (row = Q[embed] | K[embed] | V[embed]); per (image, head):
 * softmax(Q K^T / sqrt(head_dim)) V, heads concatenated.  Replaces
 * QKV_TO_SCOREV (multihead.cl:65-137, ViT_opencl.c:539-565); CPU
 * multihead_attn_seq ViT_seq.c:192-262.
 *   qkv    [n_images*tokens][3*embed],  output [n_images*tokens][embed] */
int vh_launch_attention(vh_stream_t s, const float *qkv, float *output, int n_images,
                        int tokens, int embed_dim, int num_heads);
/* Every attention on fp32 Q|K|V rows is this launcher with its choices named (vh_launch_attention = rows out, SPLIT3, AUTO).
 *   arith     how Q.K^T and P.V reach the matrix cores: the exact three-part bf16 split, the fp32 matrix instruction, two
 *             fp16 parts (vh_launch_attention_h2), operands rounded to fp16 (vh_launch_attention_f16)
 *   kernel    AUTO: K and V of a head resident in LDS where head_dim is 64 and tokens <= 208, else streamed through it
 *             (head_dim 64, 80 or 128, tokens <= 512: anything else is refused); STREAMING: streamed at every shape the
 *             streaming kernel takes, the resident ones included.  The streaming kernel has fp32 products on the fp32 matrix
 *             instruction (SPLIT3, NATIVE and FP16X2 give the same bits there) or fp16 operands (FP16), and writes fp32 rows
 *   out_kind  0 fp32 rows; 3 three-part planes (vh_launch_attention_p3: SPLIT3) and 4 one-part bf16 planes
 *             (vh_launch_attention_planes_bf16: FP16) are written by the resident kernel only: AUTO on its shapes */
enum { VH_ATTN_NATIVE = 0, VH_ATTN_FP16 = 1, VH_ATTN_FP16X2 = 2, VH_ATTN_SPLIT3 = 3 };
enum { VH_ATTN_AUTO = 0, VH_ATTN_STREAMING = 1 };
int vh_launch_attention_rows(vh_stream_t s, const float *qkv, void *output, int out_kind, int arith, int kernel, int n_images,
                             int tokens, int embed_dim, int num_heads);

/* Every row_stride-th row compacted: dst[p][i][:] = src[p][i * row_stride][:] over n_planes planes of src_rows rows of
 * row_bytes bytes (a row-major fp32 matrix: n_planes 1, row_bytes 4 * cols; a planes tensor: row_bytes 64).  Used to
 * pull out the class-token rows (ViT_seq.c:511 reads row 0 of every image only).  No reference counterpart. */
int vh_launch_gather_rows(vh_stream_t s, const void *src, void *dst, int n_planes, int src_rows, int dst_rows,
                          int row_bytes, int row_stride);

/* Row softmax with max subtraction: output[r][i] = exp(x-max)/sum.  Replaces
 * Softmax (ViT_opencl.c:750-779; softMax miniSoftMax.cl:1); CPU Softmax_seq
 * ViT_seq.c:372. */
int vh_launch_softmax(vh_stream_t s, const float *input, float *output, int rows, int length);

/* The k best entries of every row of `logits` ([rows][length] fp32): labels[r][j] = index of the j-th best, scores[r][j] its
 * logit (VIT_TOPK_LOGITS: the input's own bits) or its probability (VIT_TOPK_PROBS: exp(x - max) / sum over the whole row;
 * for length <= 2048 the bits vh_launch_softmax writes at that position, for longer rows -- which the softmax does not
 * take -- the same formula with each thread's strided elements summed in ascending index order).  Ranking: by logit,
 * descending; equal logits (-0.0f and +0.0f are equal) by ascending index; NaN below -inf, NaNs among themselves by
 * ascending index.  The labels of a row are distinct and lie in [0, length).  One workgroup per row, no atomics: a row's
 * output depends on that row only.  1 <= k <= 32, k <= length, 1 <= length <= 65536; `scores` may be NULL.  Anything
 * else: code 1 with a message, no launch.  (csrc/topk.hip; replaces the host arg-max of Main.c:59-72.) */
enum { VIT_TOPK_PROBS = 0, VIT_TOPK_LOGITS = 1 };
int vh_launch_topk(vh_stream_t s, const float *logits, int rows, int length, int k, int score_kind, int *labels, float *scores);

/* The class token's attention row of every (image, head), from one layer's Q|K|V (csrc/attn_map.hip; the kernel under
 * vit_hip_set_attention, include/ViT_opencl.h, which states the definition): tap `tap_index` of `n_taps` into
 *   heads [n_images][n_taps][num_heads][tokens]   softmax over the keys t of (q_cls . k_t) / sqrt(head_dim), fp32
 *   mean  [n_images][n_taps][tokens]              (sum over heads ascending of heads) / (float)num_heads, bit for bit
 * Either may be NULL, not both; `mean` has the same bits whether `heads` is asked for or not.  qkv as its producer left
 * it, rows = n_images * tokens, decoded exactly to fp32:
 *   VH_QKV_ROWS_F32    fp32 rows [rows][3E]
 *   VH_QKV_PLANES3     exact three-part bf16 planes [3E/32][3][rows][32], (p0 + p1) + p2 (vh_launch_merge3_rows)
 *   VH_QKV_PLANES_F16  one-part fp16 planes [3E/32][rows][32]
 * fp32 arithmetic; the sums over keys and over heads run in an order that depends on (tokens, num_heads) alone, the dot
 * products in one that depends on (head_dim, form); no atomics: an image's output is the same bits wherever it sits in
 * the batch.  Any tokens >= 1 (nothing is sized by it); head_dim a multiple of 16, at
 * most 128 (vh_cls_attention_head_dim_ok); embed_dim % 32 == 0 for the planes forms; pointers 16-byte aligned;
 * 0 <= tap_index < n_taps <= 4.  Anything else: code 1 with a message, no launch.  No reference counterpart
 * (multihead.cl:3 keeps its probabilities to itself). */
enum { VH_QKV_ROWS_F32 = 0, VH_QKV_PLANES3 = 1, VH_QKV_PLANES_F16 = 2 };
int vh_cls_attention_head_dim_ok(int head_dim);
int vh_launch_cls_attention(vh_stream_t s, const void *qkv, int qkv_form, int n_images, int tokens, int embed_dim,
                            int num_heads, int tap_index, int n_taps, float *heads, float *mean);

/* Attention rollout, one layer at a time (csrc/rollout.hip; the kernels under vit_hip_set_rollout, include/ViT_opencl.h,
 * which states the definition).  A step forms A, the head-mean attention matrix [tokens][tokens] of every image, from one
 * layer's Q|K|V (qkv and qkv_form as vh_launch_cls_attention takes them, every query row instead of the class row), and
 * folds it into the running product, all [n_images][tokens][tokens] fp32:
 *   r_prev == NULL   r_next = 0.5 A + 0.5 I                        (one launch)
 *   otherwise        r_next = 0.5 (A . r_prev) + 0.5 r_prev        (two launches; A goes through `workspace`)
 * workspace: vh_rollout_workspace(n_images, tokens) bytes, = one such buffer, needed by every step (the running sum over
 * heads lives there).  r_prev, r_next and workspace are three different buffers; r_prev is only read.  fp32 arithmetic on
 * the fp32-input matrix instruction (an exact k-ordered fma chain); every sum runs in an order fixed by (tokens,
 * num_heads, head_dim, form); no atomics: an image's rows are the same bits wherever it sits in the batch.  Rows of every
 * result are non-negative and sum to 1.  head_dim a multiple of 16, at most 128; embed_dim % 32 == 0 for the planes
 * forms; pointers 16-byte aligned; 1 <= tokens <= vh_rollout_max_tokens(head_dim) (the score rows of 16 queries stay in
 * LDS: 1856 at head_dim 128, 2176 at 64).  Anything else: code 1 with a message, no launch.
 * vh_launch_rollout_read: out[i][t] = r[i][0][t], the class token's row, [n_images][tokens], bit for bit. */
size_t vh_rollout_workspace(int n_images, int tokens);
int vh_rollout_max_tokens(int head_dim);
int vh_launch_rollout_step(vh_stream_t s, const void *qkv, int qkv_form, int n_images, int tokens, int embed_dim, int num_heads,
                           const float *r_prev /* NULL: identity */, float *r_next, void *workspace);
int vh_launch_rollout_read(vh_stream_t s, const float *r, int n_images, int tokens, float *out /* [n][T] = row 0 */);

/* ---- reduced-precision attention (the bf16- and fp8-operand modes, BASELINE configs 3 and 5) ----
 * fp32 in, fp32 out; Q, K, V and P rounded to fp16 for the two products (11-bit operands, fp32 accumulation and
 * softmax): far inside those modes' tolerances.  The bf16-operand mode itself runs on one-part planes:
 * vh_launch_layer_norm_planes / vh_launch_attention_planes_bf16 / vh_launch_linear_planes with parts = 1 (above). */
int vh_launch_attention_f16(vh_stream_t s, const float *qkv, float *output, int n_images,
                            int tokens, int embed_dim, int num_heads);

int vh_launch_absmax(vh_stream_t s, const float *input, size_t count, float *amax); /* atomic max |x| into *amax (fp16-pair mode: weight ranges) */

/* ---- block-scaled fp8 ("MX": OCP microscaling) operand variants -- BASELINE config 5 at the fp8 matrix rate ----
 * No reference counterpart.  An MX tensor [rows][cols] (cols % 128 == 0) is e4m3 elements with one e8m0
 * power-of-two scale per 32 consecutive elements of a row (scale = the smallest 2^E with max|block| / 2^E <= 448,
 * elements = e4m3_nearest_even(x / scale)), stored as
 *     values[cols/128][rows][128] bytes      scales[cols/128][4][rows] bytes
 * where scales[k][g][r] is the scale of block 2 (g & 1) + (g >> 1) of row r's K step k: the order in which the four
 * lane groups of v_mfma_scale_f32_16x16x128_f8f6f4 consume them (csrc/gemm_mx.hip; tests/mx_ref.py is the numpy
 * statement both are checked against byte for byte).  Scales are per block and computed where the tensor is
 * produced: no calibration pass. */
int vh_launch_quantize_mx_rows(vh_stream_t s, const float *input, void *values, void *scales, int rows, int cols);
/* An ACTIVATION tensor [rows][cols] as MX: values as above, scale bytes as [ceil(cols/512)][4][rows][4] -- K steps in
 * groups of four, lane group, row, K step within the group -- so that the GEMM's lane takes its scales of four K steps
 * with one dword load (vh_mx_act_scale_bytes(rows, cols) bytes, 4-byte aligned).  Every producer of a GEMM input writes
 * this form (vh_launch_layer_norm_mx, the fc1 / attention epilogues, the folded-LayerNorm producers); vh_launch_linear_mx*
 * take it for `input_scales`.  Weights keep [cols/128][4][rows] (vh_launch_quantize_mx_rows). */
int vh_launch_quantize_mx_act(vh_stream_t s, const float *input, void *values, void *scales, int rows, int cols);
size_t vh_mx_act_scale_bytes(int rows, int cols);
/* Which tile class a planes (vh_launch_linear_planes*, vh_launch_patch_embed_planes*) or MX (vh_launch_linear_mx*) projection
 * launch of `rows` x N runs on a device of num_cus compute units -- pure, touches no device; both launchers decide by it.
 * parts: 3 or 1 per value (MX: 1); resid_or_patch: the epilogue adds a residual or is the patch embedding's; small_only:
 * the launcher's own flag (residual with colA < 2048; the patch embedding with Kp < 2048).  With VH_TILES_256x256_TAIL
 * *rows_big (may be NULL) is the row at which the 256x256 launch hands over to the 128x128 launch, otherwise 0.
 * -1 for rows, N or num_cus <= 0.  Results never depend on the class: every tile sums the same products in the same order. */
enum { VH_GEMM_PLANES = 0, VH_GEMM_MX = 1 };
enum { VH_TILES_128x256 = 0, VH_TILES_128x128 = 1, VH_TILES_256x256 = 2, VH_TILES_256x256_TAIL = 3 };
int vh_gemm_tile_class(int family, int parts, int resid_or_patch, int small_only, int rows, int N, int num_cus, int *rows_big);
/* The same for the GEMMs on fp32 activation rows (csrc/gemm_mfma.hip): which kernel and tile a launch of `rows` x N over K
 * runs -- pure, touches no device; vh_launch_linear / _math and vh_launch_patch_embed* on fp32 rows (VH_ROWS_INLOOP: both
 * operands split inside the K loop, or the native fp32 instruction), vh_launch_linear_w3 (VH_ROWS_W3) and vh_launch_linear_h2
 * (VH_ROWS_H2) decide by it.  epilogue: what follows the sum; fp32_math: VH_FP32_SPLIT3 or VH_FP32_NATIVE (read by
 * VH_ROWS_INLOOP only); out_aligned16: the output, bias, residual and position-embedding pointers are all 16-byte aligned.
 *  - colB % 128 != 0 (the classifier): guarded tiles on the native instruction under either fp32_math, 32x64 while
 *    2 * ceil(rows / 128) * ceil(N / 128) < num_cus, 128x128 from there on;
 *  - 256x256 tiles where N % 256 == 0 and rows >= 4096, except with a residual over K < 2048; 128x128 otherwise;
 *  - VH_ROWS_INLOOP runs the split kernel under VH_FP32_SPLIT3 with aligned pointers, the native one otherwise;
 *  - the planes families hand the last, partly filled round of 256x256 tiles (at most 3/4 of the CUs) to a 128x128 launch
 *    from row *rows_big (may be NULL) on; every other class is one launch and leaves 0 there.
 * -1 for what the launchers refuse: a size <= 0, an unknown family, epilogue or fp32_math, and for the planes families
 * N % 128 != 0, the patch epilogue or a misaligned pointer.  Within one arithmetic (split and planes W3 / native / H2)
 * results never depend on the class: every tile sums the same products in the same order. */
enum { VH_ROWS_INLOOP = 0, VH_ROWS_W3 = 1, VH_ROWS_H2 = 2 };
enum { VH_EPI_NONE = 0, VH_EPI_GELU = 1, VH_EPI_RESID = 2, VH_EPI_PATCH = 3 };
enum {
    VH_ROWS_32x64_NATIVE_GUARDED = 0, VH_ROWS_128x128_NATIVE_GUARDED = 1, VH_ROWS_128x128_NATIVE = 2, VH_ROWS_256x256_NATIVE = 3,
    VH_ROWS_128x128_SPLIT = 4, VH_ROWS_256x256_SPLIT = 5, VH_ROWS_128x128_PLANES = 6, VH_ROWS_256x256_PLANES = 7,
    VH_ROWS_256x256_PLANES_TAIL = 8
};
int vh_gemm_rows_tile_class(int family, int epilogue, int fp32_math, int out_aligned16, int rows, int K, int N, int num_cus,
                            int *rows_big);
/* vh_launch_layer_norm writing its result as an MX tensor (embed_dim % 128 == 0) */
int vh_launch_layer_norm_mx(vh_stream_t s, const float *input, const float *weight, const float *bias,
                            void *out_values, void *out_scales, int rows, int embed_dim, long in_row_stride, double eps);
/* output (fp32 [rowA][colB]; or MX values + output_scales when output_scales != NULL, no residual) =
 *   input_mx . weight_mx^T + bias [+GELU | +residual]; fp32 accumulation.  colA % 256 == 0, colB % 128 == 0. */
int vh_launch_linear_mx(vh_stream_t s, void *output, void *output_scales, const void *weight_values,
                        const void *weight_scales, const void *input_values, const void *input_scales,
                        const float *bias, int rowA, int colA, int colB, int doGelu, const float *residual);
/* vh_launch_attention_planes_f16 writing an MX tensor (= vh_launch_quantize_mx_rows of its fp32 result, byte for byte) */
int vh_launch_attention_planes_f16_mx(vh_stream_t s, const void *qkv_planes_f16, void *out_values, void *out_scales,
                                      int n_images, int tokens, int embed_dim, int num_heads);
/* the same product (no GELU, no residual) written as one-part fp16 planes [colB/32][rowA][32] */
int vh_launch_linear_mx_planes_f16(vh_stream_t s, void *output_planes_f16, const void *weight_values,
                                   const void *weight_scales, const void *input_values, const void *input_scales,
                                   const float *bias, int rowA, int colA, int colB);

/* ---- LayerNorm folded into the projection behind it (the reduced-precision modes; csrc/norm_fold.h) ----
 * Replaces the `layerNorm` launches in front of the QKV projection and fc1 (layer_norm.cl:3-53; ViT_seq.c:120-142,346,358):
 *     LN(x) W^T + b = rstd (x (gamma.W)^T - mean colsum(gamma.W)) + (beta W^T + b)
 * The producers of the residual stream x -- patch embedding, output projection, fc2 -- leave x, besides the fp32 rows,
 * as the next projection's operand (one-part bf16 planes, or an MX tensor) and, per row and 128 columns, the partial sums
 * (sum x, sum x^2): row_stats[cols/128][rows][2] (no atomics: one writer per partial, fixed summation order).  The
 * consuming projection multiplies the un-normalised rows by the gamma-scaled weights and applies the row terms in its
 * epilogue; mean and 1/std are formed as layer_norm_seq forms them (eps added in double). */
/* context-creation helpers: out[n][k] = weight[n][k] gamma[k];  out[n] = bias[n] + sum_k beta[k] weight[n][k];
 * out[n] = sum_k of the operand's own (rounded / quantised) values of weight row n (scales NULL: one-part bf16 planes) */
int vh_launch_fold_gamma(vh_stream_t s, const float *weight, const float *gamma, float *out, int out_features, int in_features);
int vh_launch_fold_bias(vh_stream_t s, const float *weight, const float *beta, const float *bias, float *out, int out_features,
                        int in_features);
int vh_launch_colsum_operand(vh_stream_t s, const void *values, const void *scales, float *out, int out_features, int in_features);
/* vh_launch_patch_embed_planes that also leaves the token rows (class-token rows included) as the first projection's
 * operand -- one-part bf16 planes [embed/32][n*tokens][32], or MX values + scales when operand_scales_out != NULL -- and
 * their partial sums row_stats_out [embed/128][n*tokens][2] */
int vh_launch_patch_embed_planes_norm(vh_stream_t s, const float *images, const void *conv_w_planes, const float *conv_b,
                                      const float *cls_token, const float *pos_embed, float *tokens, int n_images, int in_chans,
                                      int img_size, int patch_size, int embed_dim, void *workspace, size_t workspace_bytes,
                                      void *operand_out, void *operand_scales_out, float *row_stats_out);
/* LN(A) W^T + b, folded: input_planes = the un-normalised rows (one-part bf16 planes), weight_planes = gamma-scaled.
 * output_planes as vh_launch_linear_planes (0 fp32 rows, 1 bf16 planes, 2 fp16 planes); doGelu needs output_planes 1. */
int vh_launch_linear_planes_norm(vh_stream_t s, void *output, int output_planes, const void *weight_planes,
                                 const void *input_planes, const float *row_stats, const float *colsum, const float *bias_folded,
                                 double eps, int rowA, int colA, int colB, int doGelu);
/* output = residual + A W^T + b (fp32 rows; in place allowed), the same rows as the next projection's operand (bf16
 * planes, or MX when operand_scales_out != NULL) and their partial sums row_stats_out [colB/128][rowA][2] */
int vh_launch_linear_planes_resid_norm(vh_stream_t s, float *output, const void *weight_planes, const void *input_planes,
                                       const float *bias, const float *residual, int rowA, int colA, int colB,
                                       void *operand_out, void *operand_scales_out, float *row_stats_out);
/* the same three on the exact THREE-part planes (the fp32 path's lab variant, $VIT_HIP_LN_FOLD=1): six-product arithmetic on the
 * un-normalised rows; output_planes 0 (fp32 rows) or 1 (three-part planes) */
int vh_launch_colsum_planes3(vh_stream_t s, const void *planes3, float *out, int out_features, int in_features);
int vh_launch_patch_embed_planes3_norm(vh_stream_t s, const float *images, const void *conv_w_planes3, const float *conv_b,
                                       const float *cls_token, const float *pos_embed, float *tokens, int n_images, int in_chans,
                                       int img_size, int patch_size, int embed_dim, void *workspace, size_t workspace_bytes,
                                       void *operand_planes3_out, float *row_stats_out);
int vh_launch_linear_p3_norm(vh_stream_t s, void *output, int output_planes, const void *weight_planes3, const void *input_planes3,
                             const float *row_stats, const float *colsum, const float *bias_folded, double eps, int rowA, int colA,
                             int colB, int doGelu);
int vh_launch_linear_p3_resid_norm(vh_stream_t s, float *output, const void *weight_planes3, const void *input_planes3, const float *bias,
                                   const float *residual, int rowA, int colA, int colB, void *operand_planes3_out, float *row_stats_out);
/* the same two on block-scaled fp8 operands.  output_kind: 0 fp32 rows, 1 MX tensor (the only kind doGelu takes), 2 one-part
 * fp16 planes */
int vh_launch_linear_mx_norm(vh_stream_t s, void *output, void *output_scales, int output_kind, const void *weight_values,
                             const void *weight_scales, const void *input_values, const void *input_scales, const float *row_stats,
                             const float *colsum, const float *bias_folded, double eps, int rowA, int colA, int colB, int doGelu);
int vh_launch_linear_mx_resid_norm(vh_stream_t s, float *output, const void *weight_values, const void *weight_scales,
                                   const void *input_values, const void *input_scales, const float *bias, const float *residual,
                                   int rowA, int colA, int colB, void *operand_values, void *operand_scales, float *row_stats_out);

/* ---- 8-bit pixels (vit_hip_forward_device_u8) ----
 * images: [n][img][img][in_chans] (layout 0, HWC) or [n][in_chans][img][img] (layout 1, CHW) bytes, 16-byte aligned,
 * in_chans 1..4; scale / bias: in_chans host floats.  Every value becomes x = (float)u * scale[c] + bias[c], the product
 * and the sum each rounded to fp32 (no fused multiply-add).
 * The planes paths' patch embedding: the im2row producer of vh_launch_patch_embed_planes reads the bytes and normalises as
 * it gathers (no fp32 image anywhere), then the same planes GEMM.  parts 1 with operand_out NULL = _planes, 3 = _planes3;
 * operand_out, operand_scales_out and row_stats_out as in _planes_norm (parts 1) and _planes3_norm (parts 3). */
int vh_launch_patch_embed_planes_u8(vh_stream_t s, const unsigned char *images, int layout, const float *scale, const float *bias,
                                    const void *conv_w_planes, const float *conv_b, const float *cls_token, const float *pos_embed,
                                    float *tokens, int n_images, int in_chans, int img_size, int patch_size, int embed_dim,
                                    void *workspace, size_t workspace_bytes, int parts, void *operand_out, void *operand_scales_out,
                                    float *row_stats_out);
/* The same arithmetic into normalised fp32 [n][in_chans][img][img] at `out` (the fp32-rows paths' input). */
int vh_launch_expand_u8(vh_stream_t s, const unsigned char *images, int layout, const float *scale, const float *bias, float *out,
                        int n_images, int in_chans, int img_size);

/* ---- images of img_h rows by img_w columns: the three general forms the square entries above forward to ----
 * An image is [in_chans][img_h][img_w] (fp32, 8-bit CHW) or [img_h][img_w][in_chans] (8-bit HWC); both sides are multiples of
 * patch_size; the patches of an image are row-major in its (img_h / patch) x (img_w / patch) grid, tokens = their count + 1,
 * and a patch row's K values and their order are those of the square forms.  Only the row pitch (img_w) and the plane size
 * (img_h * img_w) differ, and the vector-load conditions are conditions on img_w.
 * _planes_hw: every planes variant.  Exactly one of images_f32 and images_u8 is given (layout, scale and bias belong to the
 * 8-bit one and are ignored otherwise); parts, operand_out, operand_scales_out and row_stats_out select what
 * vh_launch_patch_embed_planes / _planes3 / _planes_norm / _planes3_norm do, as in vh_launch_patch_embed_planes_u8.
 * _rows_hw: vh_launch_patch_embed_ws_math, with vh_patch_embed_workspace_hw bytes of workspace (0 where patch % 4 == 0,
 * in_chans * patch^2 % 32 == 0 and img_w % 4 == 0: gathered on load).
 * _expand_u8_hw: vh_launch_expand_u8. */
int vh_launch_patch_embed_planes_hw(vh_stream_t s, const float *images_f32, const unsigned char *images_u8, int layout,
                                    const float *scale, const float *bias, const void *conv_w_planes, const float *conv_b,
                                    const float *cls_token, const float *pos_embed, float *tokens, int n_images, int in_chans,
                                    int img_h, int img_w, int patch_size, int embed_dim, void *workspace, size_t workspace_bytes,
                                    int parts, void *operand_out, void *operand_scales_out, float *row_stats_out);
size_t vh_patch_embed_workspace_hw(int n_images, int in_chans, int img_h, int img_w, int patch_size, int embed_dim);
int vh_launch_patch_embed_rows_hw(vh_stream_t s, const float *images, const float *conv_w, const float *conv_b,
                                  const float *cls_token, const float *pos_embed, float *tokens, int n_images, int in_chans,
                                  int img_h, int img_w, int patch_size, int embed_dim, void *workspace, size_t workspace_bytes,
                                  int fp32_math);
int vh_launch_expand_u8_hw(vh_stream_t s, const unsigned char *images, int layout, const float *scale, const float *bias, float *out,
                           int n_images, int in_chans, int img_h, int img_w);

/* ---- Pillow-exact resize + crop of 8-bit images (csrc/resize.hip; vit_hip_resize_crop_u8, vit_hip_crop_boxes_u8) ----
 * One output image: its source, and per axis Pillow's precompute_coeffs(in, in0, in1, out) -- the source span [in0, in1)
 * (C floats, as Pillow takes a box) resized to `out` samples, of which the crop indices first .. first + crop - 1 are
 * computed -- and where its coefficient tables lie in the scratch.  Resize + centre crop (vit_resize_crop_geometry) is
 * in0 = 0, in1 = (float)in, out = the resized size, first = the crop offset; a box (Image.resize(box=)) is in0 / in1 = the
 * box ends, out = crop, first = 0.  Tables of one image, at coef + coef_offset (16-byte aligned): x bounds int2 [crop]
 * (first tap, taps), y bounds int2 [crop], x weights int32 [kx][crop] (tap-major), y weights int32 [crop][ky]; weights in
 * 22 fractional bits. */
typedef struct vh_resize_desc
{
    const unsigned char *data;  /* device; any alignment; column 0 of source row `row0` */
    long row_stride;            /* bytes between rows */
    long plane_stride;          /* CHW: bytes between channel planes */
    int height, width;          /* of the whole source: the bounds are clamped to them */
    int row0;                   /* the first source row in memory: at most the first row any crop row reads */
    float x0, x1, y0, y1;       /* in0, in1 along x and y */
    int out_w, out_h;           /* out along x and y */
    int left, top;              /* first along x and y */
    int kx, ky;                 /* Pillow's ksize along x and y */
    long coef_offset;
} vh_resize_desc;
/* desc: n descriptors in device memory; filter 0 bilinear, 1 bicubic; layout 0 HWC, 1 CHW; chans 1..4; out: [n][crop][crop]
 * [chans] bytes (HWC).  One setup launch writes every image's tables into coef (coef_bytes long), then one launch per
 * (image, band of output rows) runs the horizontal pass into LDS and the vertical pass in int32 registers. */
#define VH_RESIZE_MAX_ROW_BYTES 3072   /* crop x chans at most: 12 crop bytes per thread and row */
int vh_launch_resize_crop_u8(vh_stream_t s, const vh_resize_desc *desc, int n, int chans, int layout, int filter, int crop,
                             void *coef, size_t coef_bytes, unsigned char *out);

/* Feature readout behind an encoder layer (csrc/features.hip; the kernel under vit_hip_set_features, include/ViT_opencl.h):
 * from the fp32 residual stream x [n_images * tokens][embed_dim], tap `tap_index` of `n_taps` into
 *   cls    [n_images][n_taps][embed_dim]            the class-token rows: row i * tokens of x, or row i of cls_rows at
 *                                                    cls_row_stride floats when cls_rows != NULL (compacted class rows)
 *   pooled [n_images][n_taps][embed_dim]            mean of the tokens - 1 patch rows, as tokens holds them before narrowing
 *   tokens [n_images][n_taps][tokens - 1][embed_dim] (token_layout 0) or [n_images][n_taps][embed_dim][tokens - 1] (1)
 * each may be NULL (not all).  final_norm: every row read goes through LayerNorm(gamma, beta, eps) first, bit-identical
 * to vh_launch_layer_norm on that row; final_norm 0 hands the rows through unchanged.  l2_normalize: cls and pooled are
 * scaled to unit L2 norm (a zero vector stays zero).  dtype 0 fp32, 1 bf16 (the fp32 result rounded to nearest even).
 * x is read once (only the n class rows when cls alone is asked for); pooled is summed in a fixed order that depends on
 * `tokens` alone (no atomics) through `scratch` (vh_feature_readout_scratch bytes).  embed_dim % 4 == 0, <= 2048;
 * every pointer 16-byte aligned. */
size_t vh_feature_readout_scratch(int n_images, int tokens, int embed_dim);
int vh_launch_feature_readout(vh_stream_t s, const float *x, const float *cls_rows, long cls_row_stride, const float *gamma,
                              const float *beta, double eps, int final_norm, int l2_normalize, int dtype, int token_layout,
                              int n_images, int tokens, int embed_dim, int tap_index, int n_taps, void *cls, void *pooled,
                              void *tokens_out, void *scratch, size_t scratch_bytes);

/* Gallery search (csrc/gallery.hip; the kernels under vit_hip_set_gallery, include/ViT_opencl.h): for every query the k
 * rows of a gallery with the largest inner product, selected while the gallery streams by -- the n_queries x n_rows score
 * matrix never exists.  queries [n_queries][embed_dim] fp32, contiguous; rows [n_rows] vectors of embed_dim elements,
 * row_stride elements apart, fp32 or bf16 (bf16 is decoded exactly to fp32 as it is loaded).
 * Definition.  score(i, r) = sum_d queries[i][d] * row_r[d], in fp32 on the fp32-input matrix instruction, as ONE fma chain
 * from +0 in this order of d, fixed by embed_dim alone: for c = 0, 32, 64, ...; for j = 0, 1; for e = 0..3; for g = 0..3:
 * d = c + 16 j + 4 g + e, where d >= embed_dim contributes fma(0, 0, x) = x.  The bits of score(i, r) depend on the two
 * vectors only: not on r, on where i sits among the queries, on n_queries, n_rows, splits or dtype.  A sum that is NaN is
 * returned as 0x7FC00000; a sum is never -0.  Against the exact dot product |error| <= (embed_dim + 8) * 2^-24 * sum_d
 * |q_d g_d| (with u = 2^-24 a chain of E fma steps errs by at most E u / (1 - E u) <= (E + 2 E^2 u) u <= (E + 0.5) u of
 * that sum at E <= 2048; the rest of the 8 is slack).
 * Ranking: vh_launch_topk's rule and 64-bit key -- by score descending, equal scores (-0 == +0) by ascending row index,
 * NaN below -inf, NaNs by ascending index.  indices[i][0..k) are distinct, in [0, n_rows), best first; scores[i][j] (may be
 * NULL, which changes no index) are the bits of score(i, indices[i][j]).  The keys of one query are distinct, so the
 * selected set does not depend on the order in which candidates arrive: integer LDS atomics only, no floating-point
 * atomics, the same output on every run and for every `splits`.
 * Two launches: one workgroup per (split of the gallery, tile of vh_gallery_query_tile(n_queries) = 16 or 128 queries)
 * streams its rows once in tiles of VH_GALLERY_ROW_TILE and leaves its k best keys per query in `workspace`
 * (vh_gallery_workspace bytes; splits = 0 there: a bound on whatever splits = 0 chooses here); one workgroup per query
 * then reduces splits * k keys to k.  splits = 0: chosen from (n_queries, n_rows, CU count) so that a small batch still
 * fills the machine (vh_gallery_splits); any other value gives the same bits.
 * Limits: 1 <= k <= 32; k <= n_rows <= 2^31 - 1; embed_dim % 4 == 0, 4 <= embed_dim <= 2048; row_stride >= embed_dim and
 * row_stride * element size a multiple of 16; every pointer 16-byte aligned; n_queries >= 1; 0 <= splits <=
 * VH_GALLERY_MAX_SPLITS.  Anything else: code 1 with a message, no launch.  No reference counterpart. */
enum { VH_GALLERY_F32 = 0, VH_GALLERY_BF16 = 1 };
#define VH_GALLERY_MAX_SPLITS 1024
#define VH_GALLERY_ROW_TILE 128
int vh_gallery_query_tile(int n_queries);
int vh_gallery_splits(int n_queries, long n_rows);   /* what splits = 0 launches on the current device */
size_t vh_gallery_workspace(int n_queries, long n_rows, int k, int splits);   /* bytes */
int vh_launch_gallery_topk(vh_stream_t s, const float *queries /* [n][E] fp32 */, int n_queries, int embed_dim,
                           const void *rows, int dtype, long n_rows, long row_stride /* elements */,
                           int k, int splits /* 0 = chosen by the launcher */, void *workspace,
                           int *indices /* [n][k] */, float *scores /* [n][k], may be NULL */);

/* Dense head (csrc/dense_head.hip; the kernels under vit_hip_set_dense, include/ViT_opencl.h): a label per pixel from the
 * patch tokens of a GH x GW grid -- a linear head over every token, bilinear upsampling of the C logits per patch to
 * out_h x out_w, the best label per pixel.  Two launchers; u = 2^-24 below.
 * Definition.
 * Patch logits (vh_launch_dense_logits).  Token row p of image i is the E fp32 values at rows + i * image_stride + p *
 * row_stride (elements); what lies between rows is never read, so `rows` may point at the first patch row of a residual
 * stream (x + E, image_stride = T * E, row_stride = E) or at contiguous tokens.  W [C][E] fp32, rows weight_stride apart
 * (padding never read); b [C] fp32 or NULL.  L[p][c] = (sum_d x_p[d] * W[c][d]) + b[c]: the sum in fp32 on the fp32-input
 * matrix instruction as ONE fma chain from +0 in vh_launch_gallery_topk's order of d (for c0 = 0, 32, ...; j = 0, 1; e =
 * 0..3; g = 0..3: d = c0 + 16 j + 4 g + e, d >= E contributing fma(0, 0, x) = x), then b[c] added as one fp32 add; with no
 * bias the sum's own bits (the same bits as the gallery search's score of the two vectors).  The bits of L[p][c] depend on
 * x_p, W[c] and b[c] only: not on p, the image, n_images, patches, C or any tiling.
 * Upsampling and labels (vh_launch_dense_labels): bilinear, half-pixel centres, no antialiasing, edges clamped -- what
 * torch.nn.functional.interpolate(mode="bilinear", align_corners=False) computes -- in these fp32 expressions, each
 * operation rounded once, fmaf fused:
 *   ry = (float)GH / (float)out_h;  sy = fmaxf(fmaf((float)y + 0.5f, ry, -0.5f), 0.0f);  r0 = min((int)sy, GH - 1);
 *   r1 = min(r0 + 1, GH - 1);  wy = sy - (float)r0;  uy = 1.0f - wy;   and rx, sx, c0, c1, wx, ux from x, GW, out_w alike;
 *   top = fmaf(wx, L[r0,c1][c], ux * L[r0,c0][c]);  bot = fmaf(wx, L[r1,c1][c], ux * L[r1,c0][c]);
 *   v[c] = fmaf(wy, bot, uy * top)                  (horizontal first, then vertical)
 * so v[c] is a function of (y, x, out_h, out_w, GH, GW) and the four corner values only.  An infinite corner under a zero
 * weight gives NaN, as it does in that framework.
 * labels[i][y][x] = the c that vh_launch_topk's rule ranks first among v[0..C): the largest, equal values (-0 == +0) to the
 * lowest c, NaN below -inf (all NaN: 0).  scores[i][y][x] (may be NULL, which changes no label) = that v[c]'s bits, a NaN
 * as 0x7FC00000.
 * Error bound, against this definition evaluated in float64 (coordinates, floors and lerps included) on the same fp32 x,
 * W, b, per (pixel, class):
 *   |v - v64| <= max over the four corners of (E + 8) u (sum_d |x_d w_d| + |b|)  +  k(GH, GW) u M,   k = 4 (GH + GW) + 16,
 * M = the largest |L64[.][c]| over patch rows r0 - 1 .. r0 + 2 and columns c0 - 1 .. c0 + 2 inside the grid (r0, c0 the
 * float64 cell: the four corners and their neighbours).  Derivation.  A corner: the chain errs by at most (E + 0.5) u of
 * sum |x w| (vh_launch_gallery_topk), the bias add by u |L| <= (1 + ..) u (sum |x w| + |b|); E + 8 covers both, and the
 * lerp weights are non-negative and sum to at most 1 + u, so the corners' errors reach v with at most their maximum.  The
 * coordinate: ry = (GH / out_h)(1 + e1), sy = (t ry - 0.5)(1 + e2) with t = y + 0.5 exact, |e| <= u, t / out_h < 1 and
 * |t ry - 0.5| < GH give |sy - sy64| < 2 GH u (the clamp at 0 is 1-Lipschitz); wy = sy - r0 is exact.  The bilinear
 * surface is continuous and piecewise linear with slope at most 2 M along either axis, also where (int)sy and the float64
 * floor differ by one -- then sy64 is within 2 GH u of the cell border, the value moves by at most |ds| times the slopes of
 * the two adjacent cells, whose corners M spans -- hence 4 GH u M + 4 GW u M.  The three lerps: ux, the product and the
 * fma each round once, <= 3 u M per lerp, the vertical one carrying the horizontal errors on: <= 7 u M.  The remaining 9
 * are slack (second-order terms, the float64 side's own rounding).
 * The labels kernel works per (image, patch row r0) on the band of output rows that share r0 and keeps patch rows r0, r1 x C
 * in LDS (2 * grid_w * (C | 1) * 4 bytes; 76 KB at grid_w = 37, C = 256).  Integer and LDS operations only: no atomics, the
 * same output on every run.
 * Limits: 2 <= n_labels <= VH_DENSE_MAX_LABELS; embed_dim % 4 == 0, 4 <= embed_dim <= 2048; 1 <= out_h, out_w <= 4096;
 * 1 <= grid_h, grid_w <= VH_DENSE_MAX_GRID (LDS at C = 256: 129 KB of the CU's 160); weight_stride >= embed_dim and a
 * multiple of 4, as row_stride; image_stride >= patches * row_stride, a multiple of 4; n_images, patches >= 1, n_images *
 * patches < 2^31 - 128; every pointer 16-byte aligned.  Anything else: code 1 with a message that starts with the
 * launcher's name, no launch, nothing written.  No reference counterpart. */
#define VH_DENSE_MAX_LABELS 256
#define VH_DENSE_MAX_GRID 64
#define VH_DENSE_TOKEN_TILE 128   /* token rows per workgroup of the logits kernel */
int vh_launch_dense_logits(vh_stream_t s, const float *rows, long image_stride, long row_stride /* elements */, int n_images,
                           int patches, int embed_dim, const float *weight /* [C][E] */, long weight_stride,
                           const float *bias /* [C], may be NULL */, int n_labels,
                           float *patch_logits /* [n][patches][n_labels] fp32 */);
int vh_launch_dense_labels(vh_stream_t s, const float *patch_logits /* [n][grid_h * grid_w][n_labels] */, int n_images,
                           int grid_h, int grid_w, int n_labels, int out_h, int out_w,
                           unsigned char *labels /* u8 [n][out_h][out_w] */, float *scores /* fp32, may be NULL */);

/* Soft maps of the dense head (csrc/dense_soft.hip; the kernel under vit_hip_set_dense_soft, include/ViT_opencl.h): per pixel
 * the softmax probability of the label vh_launch_dense_labels writes, the expected value of per-class `values` (depth by
 * bins: sum_c p_c * centre_c) and the entropy of the softmax, from the same patch logits.  u = 2^-24 below.
 * Definition.  Per pixel, v[c], c < C, are the fp32 values vh_launch_dense_labels defines above, by the same expressions:
 * the same bits.  With s = logit_scale, finite and > 0:
 *   m       = max_c v[c]                      (dense_labels' `scores` but for the sign of a zero, when no v is NaN)
 *   z[c]    = s * (v[c] - m)  <= 0
 *   S       = sum_c exp(z[c])  >= 1
 *   prob    = 1 / S                           (the softmax probability of the label dense_labels writes)
 *   expect  = (sum_c exp(z[c]) * values[c]) / S
 *   entropy = log S - (sum_c exp(z[c]) * z[c]) / S      nats; a term whose exp(z) is 0 contributes 0
 * Arithmetic, all fp32, each operation rounded once: k2 = s * fl(log2 e); t[c] = k2 * (v[c] - m); e[c] = v_exp_f32(t[c]) (the
 * hardware's exp2, 1 ulp, a denormal result flushed to 0); S, X = sum e[c] values[c] and A = sum e[c] max(t[c], -FLT_MAX) are
 * sequential sums over c = 0 .. C - 1 from +0, the two products as fmaf(e, ., sum): an order fixed by C alone.  prob =
 * 1 / S, expect = X / S (IEEE divisions), entropy = fl(ln 2) * (v_log_f32(S) - A / S) (the hardware's log2, 1 ulp).  No
 * atomics; an image's maps are the same bits wherever it sits in the batch and whatever n_images is, and a map's bits do not
 * depend on which other maps are asked for.
 * Special values: if any v[c] is NaN, or m is +-inf, all three outputs are written as 0x7FC00000.  A v[c] = -inf under a
 * finite m contributes nothing.  (values are taken as finite.)
 * Error bound, against this definition evaluated in float64 on the same fp32 v, s and values, K = 32:
 *   |prob - prob64|       <= (C + K) u * prob64
 *   |expect - expect64|   <= 2 (C + K) u * sum_c p64[c] |values[c]|
 *   |entropy - entropy64| <= 2 (C + K) u * (1 + ln C)
 * Derivation.  t is z / ln 2 with four roundings (the constant to half an ulp, k2, the difference, the product): a relative
 * error of 3.5 u on every z, which moves S by at most 3.5 u E_p|z| S <= 3.5 u ln C * S, because E_p|z| = ln S - H <= ln C:
 * 19.4 u at C = 256.  v_exp_f32 is good to 1 ulp = 2 u relative, a flushed term is below 2^-126 <= u S, the C-term sum costs at
 * most C u relative, the division u: (C + 3.5 ln C + 4) u <= (C + 24) u on S and on prob.  X carries the same errors term by
 * term and half an ulp more per fma, against sum e |values|; the quotient X / S adds S's: 2 (C + K) u sum p |values|.  A is X
 * with the values t (each 3.5 u off itself, and E_p|t| ln 2 <= ln C), v_log_f32(S) is within 2 u log2 S + (C + 24) u / ln 2 of
 * log2 S64, and the difference, the product with fl(ln 2) and that constant's own half ulp cost 2.5 u (1 + ln C) more: inside
 * 2 (C + K) u (1 + ln C) with room.  Measured: tests/test_gpu_dense_soft.py prints the worst |error| / bound per map
 * (profiles/dense_soft_errors.txt).
 * One launch of one 256-thread workgroup per (image, patch row), as the labels kernel's, with its LDS (2 * grid_w * (C | 1) *
 * 4 bytes); two passes over the classes, the first for m.
 * Limits: those of vh_launch_dense_labels (n_labels, the grid, out_h, out_w, n_images; csrc/kernel_limits.h states them
 * once); logit_scale finite and > 0; values given exactly when expect is; at least one of prob, expect, entropy; every pointer
 * 16-byte aligned.  Anything else: code 1 with a message that starts with "vh_launch_dense_soft: ", no launch, nothing
 * written.  No reference counterpart. */
int vh_launch_dense_soft(vh_stream_t s, const float *patch_logits /* [n][grid_h * grid_w][n_labels] */, int n_images,
                         int grid_h, int grid_w, int n_labels, int out_h, int out_w, float logit_scale,
                         const float *values /* [n_labels] fp32, device; NULL iff expect is NULL */,
                         float *prob, float *expect, float *entropy /* fp32 [n][out_h][out_w]; each may be NULL, not all three */);

/* Dense stitch (csrc/dense_stitch.hip; the kernel under vit_hip_segment_frame_u8, include/ViT_opencl.h): one label per pixel
 * of a frame_h x frame_w frame from the patch logits of n_windows overlapping windows of it -- the sliding-window protocol
 * (upsample every window's logits to its box, average where boxes overlap, take the best class) as a GATHER: per pixel the
 * windows that cover it are found, each window's patch logits are interpolated at that pixel and averaged; no frame-sized
 * logits buffer exists.  u = 2^-24 below.
 * Inputs.  patch_logits [n_windows][GH * GW][C] fp32 in device memory, as vh_launch_dense_logits writes them.  windows:
 * n_windows boxes (l, t, r, b), 4 floats each, in frame pixel coordinates, in HOST memory; offsets / ids: the block index of
 * vit_stitch_index(frame_h, frame_w, VH_STITCH_BLOCK, windows, n_windows, ..) (include/ViT_opencl.h), in HOST memory:
 * offsets [blocks_y * blocks_x + 1], the ids of block k at ids[offsets[k] .. offsets[k + 1]), strictly ascending window
 * indices; a block's list must hold every window that covers a pixel centre of the block and may hold more.
 * Definition, in these fp32 expressions, each operation rounded once, fmaf fused.
 * Coverage: window w covers pixel (X, Y) iff l <= cx < r and t <= cy < b, cx = (float)X + 0.5f, cy = (float)Y + 0.5f (exact
 * values, exact comparisons).
 * Coordinates of the pixel in w:
 *   bw = r - l;  rx = (float)GW / bw;  tx = cx - l;  sx = fmaxf(fmaf(tx, rx, -0.5f), 0.0f);  c0 = min((int)sx, GW - 1);
 *   c1 = min(c0 + 1, GW - 1);  wx = sx - (float)c0;  ux = 1.0f - wx;   and bh, ry, ty, sy, r0, r1, wy, uy from cy, t, b, GH alike.
 * Value of class c in w, the three lerps of vh_launch_dense_labels on w's logits L (horizontal first, then vertical):
 *   top = fmaf(wx, L[r0,c1][c], ux * L[r0,c0][c]);  bot = fmaf(wx, L[r1,c1][c], ux * L[r1,c0][c]);  v_w[c] = fmaf(wy, bot, uy * top)
 * Consequence: for a box of integer corners with r - l = out_w and b - t = out_h, v_w at (X, Y) has the bits
 * vh_launch_dense_labels gives at (X - l, Y - t) for that out_h x out_w: bw and (X + 0.5) - l are exact there, so rx, sx and
 * all that follows are that launcher's own values.
 * Blend: over the windows that cover the pixel, in ascending window index, acc = v_first, then acc = acc + v_next (fp32 adds);
 * m[c] = acc / (float)count, one correctly rounded fp32 division: the plain mean of the slide protocol.
 * labels[Y][X] = the c that vh_launch_topk's rule ranks first among m[0..C): the largest, equal values (-0 == +0) to the lowest
 * c, NaN below -inf (all NaN: 0).  scores[Y][X] (may be NULL) = that m[c]'s bits, a NaN as 0x7FC00000.  cover[Y][X] (may be
 * NULL) = min(count, 255).  Asking for scores or cover changes no label.  A pixel that no window covers: labels = fill_label,
 * scores = 0x7FC00000, cover = 0.
 * The bits of a pixel depend on that pixel, the windows that cover it with the order of their indices, and those windows'
 * logits: not on the frame size, on other windows, on what else a block's list names or on any tiling.  No atomics: the same
 * output on every run.
 * Error bound, against this definition evaluated in float64 (coverage is exact in both) on the same fp32 logits and boxes,
 * per (pixel, class), for count <= 2^22:
 *   |m - m64| <= (1 + A) max_w B_w + A max_w |v64_w|,      A = (count + 1) (1 + 2 count u) u,
 * B_w = the interpolation part of vh_launch_dense_labels' bound on window w with the coordinate constant doubled:
 *   B_w = k'(GH, GW) u M_w,   k' = 8 (GH + GW) + 16,   M_w as M there (|L| over rows r0 - 1 .. r0 + 2, columns c0 - 1 .. c0 + 2 of w);
 * where the logits themselves come from vh_launch_dense_logits, that launcher's corner term (E + 8) u (sum |x w| + |b|), its
 * maximum over the four corners, is added to B_w.  Derivation.  The coordinate: bw, rx, tx and the fmaf round once each where
 * vh_launch_dense_labels has two roundings: rx = (GW / (r - l)) (1 + e1)(1 + e2), tx = (cx - l)(1 + e3), sx = (tx rx - 0.5)(1 +
 * e4), |e| <= u, tx / (r - l) < 1 and |tx rx - 0.5| < GW give |sx - sx64| < 4 GW u (there: 2 GW u); the surface argument is
 * that launcher's, hence 8 GH u M + 8 GW u M; the three lerps and the slack are unchanged (7 + 9).  The blend: count - 1 adds
 * err by at most g sum_w |v_w|, g = (count - 1) u / (1 - (count - 1) u) <= (count - 1)(1 + 2 count u) u, which after the
 * division is g max_w |v_w|; the division adds u |m| <= u (1 + g) max |v_w|; together at most A max |v_w|, and |v_w| <=
 * |v64_w| + B_w.  The windows' own errors reach the mean with at most their maximum.
 * One workgroup of VH_STITCH_BLOCK^2 threads per block of VH_STITCH_BLOCK x VH_STITCH_BLOCK pixels, one pixel per thread;
 * classes in chunks of 16 whose running sums stay in registers; inside a chunk the block's list in ascending order; corner
 * logits are read from global memory, 16 bytes at a time (a frame's patch logits are some tens of MB: L2 and MALL traffic).
 * Staging each window's rectangle of patches in LDS was built and measured: the same bits, 10-18 % slower.
 * The boxes and the index are copied into d_scratch (vh_dense_stitch_scratch bytes, the CALLER'S device memory, 16-byte
 * aligned) with synchronous copies before the launch: the three host arrays may be freed when the launcher returns; the
 * kernel itself is asynchronous on s and reads d_scratch when it runs.  Until it has run, d_scratch must neither be freed
 * nor written, nor handed to another call of this launcher: that call's copies do not wait for s and would replace the index
 * under the queued kernel.  One scratch per launch in flight (the frame calls allocate theirs per call and wait for s).
 * Limits: 2 <= n_labels <= VH_DENSE_MAX_LABELS; 1 <= grid_h, grid_w <= VH_DENSE_MAX_GRID; 1 <= frame_h, frame_w <=
 * VH_STITCH_MAX_SIDE; n_windows >= 1, n_windows * grid_h * grid_w < 2^31 - 128; every box finite with 0 <= l, r <= frame_w,
 * 0 <= t, b <= frame_h, r - l >= 1, b - t >= 1 (vit_stitch_check); offsets[0] = 0, offsets non-decreasing, offsets[blocks] =
 * n_ids < 2^31, the ids of a block strictly ascending in [0, n_windows); 0 <= fill_label <= 255; scratch_bytes >=
 * vh_dense_stitch_scratch; every device pointer 16-byte aligned.  Anything else: code 1 with a message that starts with the
 * launcher's name, no launch, nothing written.  No cap on how many windows cover a pixel or fall into a block.  No reference
 * counterpart. */
#define VH_STITCH_BLOCK 16
#define VH_STITCH_MAX_SIDE 16384
size_t vh_dense_stitch_scratch(int n_windows, int frame_h, int frame_w, long n_ids);   /* bytes; 0 for arguments out of range */
int vh_launch_dense_stitch(vh_stream_t s, const float *patch_logits /* device [n_windows][grid_h * grid_w][n_labels] */,
                           int n_windows, int grid_h, int grid_w, int n_labels, const float *windows /* host [n_windows][4] */,
                           int frame_h, int frame_w, const int *offsets /* host [blocks + 1] */, const int *ids /* host */,
                           int fill_label, void *d_scratch, size_t scratch_bytes, unsigned char *labels /* u8 [frame_h][frame_w] */,
                           float *scores /* fp32, may be NULL */, unsigned char *cover /* u8, may be NULL */);

/* Soft stitch (csrc/dense_stitch_soft.hip; the kernel under vit_hip_segment_frame_soft_u8, include/ViT_opencl.h): the soft
 * maps of vh_launch_dense_soft per pixel of a frame, on the blended means of vh_launch_dense_stitch -- the slide protocol
 * followed by its softmax (average the windows' logits, then softmax), as a gather: no [C][H][W] buffer.  u = 2^-24 below.
 * Inputs.  patch_logits, windows, offsets, ids and d_scratch exactly as vh_launch_dense_stitch takes them (windows, offsets
 * and ids in HOST memory, the index that of vit_stitch_index(.., VH_STITCH_BLOCK, ..), d_scratch of vh_dense_stitch_scratch
 * bytes with that launcher's layout and that launcher's rule: one scratch per launch in flight); logit_scale, values (device
 * [n_labels], given exactly when expect is) and the three maps, fp32 [frame_h][frame_w] each, as vh_launch_dense_soft takes
 * them: each map may be NULL, not all three.
 * Definition.  Per frame pixel, m[c], c < C, is the blended mean vh_launch_dense_stitch defines above -- coverage,
 * coordinates, the three lerps per window, the adds in ascending window index with the first value replacing the zero, one
 * fp32 division by (float)count -- by the same expressions: the same bits.  The three maps are vh_launch_dense_soft's
 * definition with v[c] := m[c], operation for operation: M = max_c m[c], c ascending, a NaN never the maximum; k2 = s *
 * fl(log2 e); t = k2 * (m[c] - M); e = v_exp_f32(t); S, X = sum fmaf(e, values[c], .) and A = sum fmaf(e, max(t, -FLT_MAX), .)
 * sequential over c = 0 .. C - 1 from +0; prob = 1 / S, expect = X / S, entropy = fl(ln 2) * (v_log_f32(S) - A / S).
 * Special values: a pixel that no window covers, a pixel with any NaN m[c] (a NaN corner under a non-zero or zero weight of
 * a covering window, or +inf and -inf of one class in two covering windows) and a pixel whose M is +-inf get 0x7FC00000 in all
 * three maps.  A -inf under a finite M contributes nothing.
 * Consequences.  (1) For one window of integer corners with r - l = frame_w and b - t = frame_h the maps are
 * vh_launch_dense_soft's bits at out_h x out_w = frame_h x frame_w: count = 1, m = v / 1.0f = v, and v is
 * vh_launch_dense_labels' value by the consequence stated for the stitch.  (2) A pixel's bits depend on that pixel, on the
 * windows that cover it with the order of their indices, and on their logits: not on the frame size, on other windows, on
 * what else a block's list names, on which maps are asked for, nor on how the kernel keeps m between its two passes (below).
 * (3) No atomics: the same output on every run.
 * Error bound.  Against the definition evaluated in float64 on the same fp32 m: vh_launch_dense_soft's bound unchanged, (C
 * + 32) u relative on prob and its companions on expect and entropy -- it is the same arithmetic on the same kind of input.
 * Against float64 throughout (blend and softmax) on the same fp32 logits and boxes: m is within delta = max_c ((1 + A) max_w
 * B_w + A max_w |v64_w|) of m64, the stitch's bound; softmax is invariant under a shift of all m, so every ln p_c moves by at
 * most 2 s delta, and with g = expm1(2 s delta)
 *   |prob - prob64| <= g prob64 + (C + 32) u prob64,   |expect - expect64| <= g sum p64 |values| + 2 (C + 32) u sum p64 |values|,
 *   |entropy - entropy64| <= g (1 + ln C) + 2 (C + 32) u (1 + ln C)
 * -- the combination tests/dense_soft_ref.py::combined_bounds makes of the interpolation bound, with the stitch's delta for it.
 * Measured: tests/test_gpu_stitch_soft.py prints the worst |error| / bound per map (profiles/frame_soft_errors.txt).
 * One workgroup of VH_STITCH_BLOCK^2 threads per block, one pixel per thread, classes in chunks of 16, the block's list in
 * ascending order per chunk, corner logits as 16-byte global loads: the stitch's decomposition.  The softmax needs M before
 * its sums: pass 1 blends every chunk for M, pass 2 needs every m[c] again.  Two ways are kept, which give the same bits
 * because the definition fixes every operation: blend again (variant 1, any C), or keep the means of pass 1 in registers
 * (variant 2, C <= 160: ten chunks).  vh_dense_stitch_soft_variant(n_labels) says which a launch takes -- by n_labels alone,
 * from measurements (a third way, the means in LDS, was slower than either: docs/LABBOOK.md).  The tests and
 * tools/frame_soft_rates.py reach either variant through an internal entry that takes it as an argument of the call
 * (csrc/vit_kernels.h); the library keeps no switch.
 * Limits: vh_launch_dense_stitch's (n_labels, the grid, the frame, n_windows, the boxes, the index -- validated on the host
 * before any copy -- scratch_bytes, 16-byte alignment of every device pointer) and vh_launch_dense_soft's (logit_scale finite
 * and > 0; values given exactly when expect is; at least one map).  Anything else: code 1 with a message that starts with
 * "vh_launch_dense_stitch_soft: ", no launch, nothing written.  No reference counterpart. */
int vh_dense_stitch_soft_variant(int n_labels);
int vh_launch_dense_stitch_soft(vh_stream_t s, const float *patch_logits /* device [n_windows][grid_h * grid_w][n_labels] */,
                                int n_windows, int grid_h, int grid_w, int n_labels, const float *windows /* host [n_windows][4] */,
                                int frame_h, int frame_w, const int *offsets /* host [blocks + 1] */, const int *ids /* host */,
                                void *d_scratch, size_t scratch_bytes, float logit_scale,
                                const float *values /* [n_labels] fp32, device; NULL iff expect is NULL */,
                                float *prob, float *expect, float *entropy /* fp32 [frame_h][frame_w]; each may be NULL, not all three */);

/* Position embedding resampled to another patch grid (csrc/pos_resample.hip; the kernel under vit_hip_create_at_resolution,
 * include/ViT_opencl.h).  src [prefix + in_h * in_w][E] fp32 -> dst [prefix + out_h * out_w][E] fp32, both contiguous.
 * Definition.  The first `prefix` rows (the class token's) are copied bit for bit.  The remaining rows are a row-major
 * in_h x in_w grid of E-vectors, resampled channel by channel to out_h x out_w: what
 *     torch.nn.functional.interpolate(grid[None], size=(out_h, out_w), mode=mode, align_corners=align_corners,
 *                                     antialias=False)
 * computes on a float64 copy of the grid ([E][in_h][in_w]), rounded to fp32 once.  All coordinate and weight arithmetic and
 * every sum is float64.  Per axis (in, out, output index o):
 *   align_corners 0:  scale = (double)in / out;                           s = (o + 0.5) * scale - 0.5
 *   align_corners 1:  scale = out > 1 ? (double)(in - 1) / (out - 1) : 0; s = o * scale
 * VH_POS_BICUBIC (the Keys kernel, A = -0.75): i0 = floor(s), t = s - i0 (s is NOT clamped); taps i0 - 1 .. i0 + 2, each
 * index clamped to [0, in - 1]; weights c2(t + 1), c1(t), c1(1 - t), c2(2 - t) with
 *   c1(x) = ((A + 2) x - (A + 3)) x^2 + 1          c2(x) = ((A x - 5 A) x + 8 A) x - 4 A
 * VH_POS_BILINEAR: with align_corners 0, s = max(s, 0); i0 = min((int)s, in - 1), i1 = min(i0 + 1, in - 1); weights
 * 1 - (s - i0) and s - i0.
 * Value: v = sum_j wy_j * (sum_i wx_i * p[iy_j][ix_i]), i and j ascending, horizontal first, in float64; dst = (float)v.
 * Equal grids (in_h == out_h and in_w == out_w) are a plain copy, bit for bit, in either mode.
 * Which convention is whose: (bicubic, align_corners 0) is the Hugging Face ViT's interpolate_pos_encoding and DINO's;
 * (bicubic, align_corners 1) is torchvision's interpolate_embeddings.  antialias=True (timm's default) is another kernel
 * and is not built.
 * Error bound, against this definition evaluated in float64 (tests/pos_resample_ref.py): per element
 *   |got - want| <= 2^-24 |want| + 2^-40 M,     M = the largest |p| of the source grid.
 * The first term is the one final rounding.  The second covers float64 rounding and contraction differences in about 40
 * operations whose absolute weights sum to at most 1.375^2 = 1.89 (the bicubic weights of an axis sum to 1 and their
 * magnitudes to at most 1.375; a coordinate is a handful of float64 operations on values below 2^10, so a weight errs by
 * ~2^-50): (40 x 2^-53 + ..) x 1.89 M is below 2^-46 M, the rest is slack.  Where two evaluations of a coordinate fall on
 * either side of an integer the interpolant is continuous across the knot (cubic convolution and the linear interpolant
 * both are), so the bound does not change there.
 * float64 costs nothing here: the kernel is memory-bound (NT^2 = 16 or 4 float4 loads per 4 outputs against some 200 double
 * operations per thread) and runs once per derived context, not per forward.
 * A thread owns one output token and 4 consecutive channels (float4 loads and stores, consecutive lanes on consecutive
 * channels) and computes its at most 8 weights itself; no LDS, no atomics.  The bits of a channel's output depend on that
 * channel's grid values and the four sizes only -- not on embed_dim or on the other channels.
 * Limits: embed_dim % 4 == 0, embed_dim >= 4; every grid side in 1..512; prefix in 0..8; mode and align_corners as above;
 * src and dst distinct, not overlapping, 16-byte aligned.  Anything else: code 1 with a message that starts with the
 * launcher's name, no launch, nothing written. */
enum { VH_POS_BICUBIC = 0, VH_POS_BILINEAR = 1 };
int vh_launch_resample_pos_embed(vh_stream_t s, const float *src /* [prefix + in_h*in_w][E] */,
                                 float *dst /* [prefix + out_h*out_w][E] */, int prefix,
                                 int in_h, int in_w, int out_h, int out_w, int embed_dim,
                                 int mode, int align_corners);

#ifdef __cplusplus
}
#endif

#endif /* VIT_HIP_KERNELHANDLER_H */
