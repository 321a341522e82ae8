/*
 * ViT_hip.c -- host side of the ViT forward pass, in C, over the C-ABI device
 * shim (include/kernelHandler.h).  This file is the counterpart of the
 * reference's ViT_opencl.c host orchestration (Encoder :710-748, ViT_opencl
 * :794-986) and of its device-memory management (:125-357), redesigned:
 *
 *  - the whole batch moves through each operator at once (M = n*tokens rows)
 *    instead of one image at a time through 113 event-chained launches;
 *  - weights are uploaded once per context into one HBM slab, activations live
 *    in one arena sized at creation (the reference creates and destroys 14
 *    cl_mem objects per image, ViT_opencl.c:929,962);
 *  - one in-order stream, so no event graph is needed;
 *  - the residual adds are folded into the projection epilogues and the final
 *    LayerNorm runs on the class-token rows only (the reference normalises all
 *    197 rows and uses one, ViT_opencl.c:951-955 / ViT_seq.c:506-511).
 *
 * What a forward reads -- fp32 or 8-bit pixels, of the model's size or resized / cropped from boxes first, in device or in
 * host memory -- is one struct ingest_src (csrc/vit_ingest.h).  Everything about 8-bit sources that needs no device lives in
 * csrc/vit_ingest.c: the argument checks, the fill of the resize kernel's descriptors, and the planner and packer of the host
 * forms' staging slots.  The staging slots themselves, the chunk loop of the host forms over them and the descriptor ring are
 * csrc/vit_pipeline.c; this file keeps the launches.
 *
 * What a context will run -- the kernels of a forward, the layout of the weight slabs, the size of every arena buffer -- is one
 * struct vit_plan (csrc/vit_plan.h), made by plan_make before anything is allocated; this file allocates what it says and
 * branches on its fields.  What the plan, the requests and the frame sizing here know about the kernels -- the shapes each
 * takes, the bytes of scratch each needs -- is stated once in csrc/kernel_limits.h, plain C that the launchers read too; none
 * of them asks the shim for a size or a limit.
 *
 * What is left here is the context (both ways of making one end in ctx_finish), the layer functions, the forwards and the
 * drop-in ViT_opencl().  The repacked-weights file -- format, writer, reader and every refusal of a header -- is
 * csrc/vit_planes_file.c; shards and device replicas are csrc/vit_multi.c, and what the three files of the multi-GPU forms
 * share is declared once in csrc/vit_multi.h.
 *
 * Operator order per layer (ViT_seq.c:330-370):
 *   y = LN1(x); qkv = y Win^T + bin; a = attention(qkv); x = x + (a Wout^T + bout);
 *   y = LN2(x); h = gelu(y W1^T + b1); x = x + (h W2^T + b2)
 */
#include "ViT_opencl.h"
#include "kernel_limits.h"
#include "vit_ingest.h"
#include "vit_multi.h"
#include "vit_pipeline.h"
#include "vit_plan.h"
#include "vit_planes_file.h"
#include "vit_requests.h"

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#define TRY(expr)                 \
    do {                          \
        int try_rc_ = (expr);     \
        if (try_rc_ != 0) {       \
            rc = try_rc_;         \
            goto fail;            \
        }                         \
    } while (0)

struct vit_hip_ctx
{
    vit_config cfg;
    int device;
    int max_batch;
    int n_tensors;
    vh_stream_t stream;

    /* everything a forward, the weight layout or the arena branches on, and every size, fixed at creation before anything is
     * allocated (csrc/vit_plan.h) */
    struct vit_plan plan;

    void *slab[N_SLABS];   /* of plan.slab_bytes */
    float **w;         /* SLAB_F32: device pointer per tensor index, every tensor in fp32 */
    struct operand *op; /* SLAB_OPERAND and SLAB_FOLD: [depth][4] (in_proj, out_proj, fc1, fc2) */
    /* SLAB_CONV: conv_proj as planes [Kp/32][parts][E][32]: one part (bf16) for BF16_GEMM / FP8_GEMM
     * (vh_launch_patch_embed_planes), the exact three-part split for F32 (vh_launch_patch_embed_planes3) */

    /* activation arena (rows = max_batch * tokens), of the plan's sizes */
    float *x;           /* residual stream      [rows][E]   */
    float *y;           /* LayerNorm output     [rows][E]   */
    float *attn;        /* attention output     [rows][E]   */
    float *qkv;         /* fused Q|K|V          [rows][3E]  */
    float *hid;         /* MLP hidden           [rows][F]; plan.ws_bytes: it doubles as the workspace of whatever runs while the MLP is idle */
    float *stats;      /* ln_fold: partial (sum, sum of squares) of the residual rows, [E/128][rows][2] */
    float *cls;         /* normalised CLS rows  [max_batch][E] */
    float *d_logits;    /* [max_batch][classes] */
    float *d_probs;     /* [max_batch][classes] */
    /* host-pointer API: the staging slots, copy stream and events of the chunk loop, and the descriptor ring of the resize
     * launches (csrc/vit_pipeline.h).  resize + centre crop (vit_hip_resize_crop_u8, the _resized forwards): the crops land
     * in Q|K|V at plan.crop_off (behind the fp32 expansion on the fp32-rows paths), the coefficient tables in hid. */
    struct pipeline pipe;

    /* the armed outputs (csrc/vit_requests.h), and what of them the running forward serves: forward_device sets it for its
     * layer functions (attention_tap) and clears it when it returns; NULL between forwards */
    struct requests req;
    const struct serving *serving;

    /* images of the last forward whose last layer ran behind its attention for the class-token rows only
     * (plan.last_layer_lazy or plan.cls_only_last): x, attn and y still hold what the other rows need, and
     * finish_last_layer evaluates them for whoever reads those rows afterwards.  0: nothing is pending */
    int last_pending;
    int last_pending_attention;   /* ... and Q and the attention ran for the class query alone (plan.cls_query) */

    /* optional per-operator timing with HIP events on the launch stream */
    vh_event_t *prof_ev;   /* 2 events per recorded launch */
    int *prof_class;       /* operator class per recorded launch */
    int prof_cap;          /* launches the pool can hold */
    int prof_used;         /* launches recorded since enable */
    unsigned prof_mask;    /* operator classes to record (bit = vit_op_class); 0 = all */
};

static int prof_begin(vit_hip_ctx *ctx, vh_stream_t s, int op_class)
{
    if (!ctx->prof_ev || ctx->prof_used >= ctx->prof_cap)
        return -1;
    if (ctx->prof_mask && !(ctx->prof_mask & (1u << op_class)))
        return -1;
    const int slot = ctx->prof_used++;
    ctx->prof_class[slot] = op_class;
    vh_event_record(ctx->prof_ev[2 * slot], s);
    return slot;
}

static void prof_end(vit_hip_ctx *ctx, vh_stream_t s, int slot)
{
    if (slot >= 0)
        vh_event_record(ctx->prof_ev[2 * slot + 1], s);
}

/* Launch `call` bracketed by two events when profiling is enabled and the launch is `timed` (part of a forward). */
#define OP_T(timed, op_class, call)                                        \
    do {                                                                   \
        const int op_slot_ = (timed) ? prof_begin(ctx, s, op_class) : -1;  \
        TRY(call);                                                         \
        prof_end(ctx, s, op_slot_);                                        \
    } while (0)
#define OP(op_class, call) OP_T(1, op_class, call)

static void prof_release(vit_hip_ctx *ctx)
{
    if (ctx->prof_ev) {
        for (int i = 0; i < 2 * ctx->prof_cap; ++i)
            if (ctx->prof_ev[i])
                vh_event_destroy(ctx->prof_ev[i]);
        free(ctx->prof_ev);
        free(ctx->prof_class);
    }
    ctx->prof_ev = NULL;
    ctx->prof_class = NULL;
    ctx->prof_cap = ctx->prof_used = 0;
}

const vit_config *vit_hip_config(const vit_hip_ctx *ctx) { return &ctx->cfg; }
/* columns of an input image; its rows are cfg.img_size */
static int ctx_width(const vit_hip_ctx *ctx) { return ctx->cfg.img_width ? ctx->cfg.img_width : ctx->cfg.img_size; }
int vit_hip_device(const vit_hip_ctx *ctx) { return ctx->device; }
float *vit_hip_logits_buffer(vit_hip_ctx *ctx) { return ctx->d_logits; }   /* [max_batch][classes], vit_gather_rccl.c */
vh_stream_t vit_hip_stream(const vit_hip_ctx *ctx) { return ctx->stream; }
int vit_hip_max_batch(const vit_hip_ctx *ctx) { return ctx->max_batch; }
const float *vit_hip_weight(const vit_hip_ctx *ctx, int idx)
{
    return (idx >= 0 && idx < ctx->n_tensors) ? ctx->w[idx] : NULL;
}

void vit_hip_destroy(vit_hip_ctx *ctx)
{
    if (!ctx)
        return;
    if (ctx->stream) {   /* a context that never reached the device (refused header, bad arguments) leaves the device --
                          * and the caller's error text -- alone */
        vh_set_device(ctx->device);
        vh_stream_sync(ctx->stream);
    }
    prof_release(ctx);
    requests_release(&ctx->req);
    for (int i = 0; i < N_SLABS; ++i)
        if (ctx->slab[i])
            vh_free(ctx->slab[i]);
    float *dev[] = {ctx->x, ctx->y, ctx->attn, ctx->qkv, ctx->hid, ctx->stats, ctx->cls, ctx->d_logits, ctx->d_probs};
    for (size_t i = 0; i < sizeof(dev) / sizeof(dev[0]); ++i)
        if (dev[i])
            vh_free(dev[i]);
    pipeline_release(&ctx->pipe);
    if (ctx->stream)
        vh_stream_destroy(ctx->stream);
    free(ctx->w);
    free(ctx->op);
    free(ctx);
}

/* a layer's 12 fp32 tensors: ln1 w,b; in w,b; out w,b; ln2 w,b; fc1 w,b; fc2 w,b */
static float **layer_tensors(const vit_hip_ctx *ctx, int l) { return ctx->w + 4 + 12 * l; }

/* The weight slabs of the plan's sizes, and every tensor and operand pointed into them */
static int alloc_weights(vit_hip_ctx *ctx)
{
    int rc = 0;
    for (int i = 0; i < N_SLABS; ++i)
        if (ctx->plan.slab_bytes[i]) {
            TRY(vh_malloc(&ctx->slab[i], ctx->plan.slab_bytes[i]));
            /* the alignment gaps between the pieces too: what vit_hip_export_planes writes depends on the weights alone */
            TRY(vh_memset(ctx->slab[i], 0, ctx->plan.slab_bytes[i], ctx->stream));
        }
    plan_layout(&ctx->plan, &ctx->cfg, ctx->slab, ctx->w, ctx->op, NULL);
    return 0;
fail:
    return rc;
}

/* Upload the caller's tensors and repack the four big matrices of every layer into the mode's GEMM operand format. */
static int fill_weights(vit_hip_ctx *ctx, const Network *networks)
{
    int rc = 0;
    const vit_config *cfg = &ctx->cfg;
    const int p = ctx->plan.precision;
    float *d_amax = NULL, *d_scaled = NULL;
    for (int i = 0; i < ctx->n_tensors; ++i)
        TRY(vh_h2d(ctx->w[i], networks[i].data, networks[i].size * sizeof(float), ctx->stream));
    if (p == VIT_PRECISION_F32_FP16X2)
        TRY(vh_malloc((void **)&d_amax, sizeof(float)));
    if (ctx->plan.ln_fold)   /* gamma-scaled copy of one matrix at a time, before its rounding (the largest is fc1 / in_proj) */
        TRY(vh_malloc((void **)&d_scaled, (size_t)cfg->embed_dim * (size_t)(cfg->mlp_hidden > 3 * cfg->embed_dim ? cfg->mlp_hidden : 3 * cfg->embed_dim) * sizeof(float)));
    for (int m = 0; m < 4 * cfg->depth; ++m) {
        struct operand *o = &ctx->op[m];
        float **lw = layer_tensors(ctx, m / 4);
        const int idx = plan_operand_tensor(m), k = m % 4, fold = o->colsum != NULL;
        const int out_f = (int)networks[idx + 1].size, in_f = (int)(networks[idx].size / networks[idx + 1].size);
        const float *src = ctx->w[idx];
        if (fold) {
            /* the LayerNorm in front of this projection moves into it (csrc/norm_fold.h): W' = gamma . W rounded to the
             * mode's operand format, colsum of the ROUNDED values, bias' = bias + beta W^T from the fp32 weights.
             * ln1 (tensors 0, 1 of the layer) feeds in_proj, ln2 (6, 7) feeds fc1. */
            TRY(vh_launch_fold_gamma(ctx->stream, ctx->w[idx], lw[k == 0 ? 0 : 6], d_scaled, out_f, in_f));
            src = d_scaled;
        }
        switch (p) {
        case VIT_PRECISION_BF16_GEMM:
            /* one-part planes [K/32][1][N][32] (gemm_p3.hip); everything else (norms, biases, embeddings, classifier) stays fp32 */
            TRY(vh_launch_split_rows(ctx->stream, src, o->w, out_f, in_f, 1));
            break;
        case VIT_PRECISION_FP8_GEMM:
            TRY(vh_launch_quantize_mx_rows(ctx->stream, src, o->w, o->scales, out_f, in_f));
            break;
        case VIT_PRECISION_F32:
            /* the constant GEMM operand split once (exact 3-way bf16 split, 6 bytes per weight) */
            if (o->w)
                TRY(vh_launch_split3_planes(ctx->stream, src, o->w, out_f, in_f));
            break;
        case VIT_PRECISION_F32_FP16X2: {
            /* two fp16 parts of w * 2^k per weight (4 bytes), k per tensor such that max|w| * 2^k lands in
             * [8192, 16384): the low part stays clear of fp16's subnormals, nothing overflows */
            float amax = 0.0f;
            TRY(vh_memset(d_amax, 0, sizeof(float), ctx->stream));
            TRY(vh_launch_absmax(ctx->stream, src, networks[idx].size, d_amax));
            TRY(vh_d2h(&amax, d_amax, sizeof(float), ctx->stream));
            TRY(vh_stream_sync(ctx->stream));
            int e = 0;
            o->pair_scale = 1.0f;
            if (amax > 0.0f && amax < 3.0e38f) {
                (void)frexpf(amax, &e);                     /* amax = m * 2^e, m in [0.5, 1) */
                o->pair_scale = ldexpf(1.0f, 14 - e);       /* amax * scale in [8192, 16384) */
            }
            TRY(vh_launch_split2h_planes(ctx->stream, src, o->w, out_f, in_f, o->pair_scale));
            break;
        }
        }
        if (fold) {
            TRY(p == VIT_PRECISION_F32 ? vh_launch_colsum_planes3(ctx->stream, o->w, o->colsum, out_f, in_f)
                                       : vh_launch_colsum_operand(ctx->stream, o->w, o->scales, o->colsum, out_f, in_f));
            TRY(vh_launch_fold_bias(ctx->stream, ctx->w[idx], lw[k == 0 ? 1 : 7], ctx->w[idx + 1], o->bias_folded, out_f, in_f));
        }
    }
    if (d_scaled)
        TRY(vh_stream_sync(ctx->stream));   /* the scratch copy is freed below */
    if (ctx->slab[SLAB_CONV])
        TRY(vh_launch_conv_weight_planes_parts(ctx->stream, ctx->w[1], ctx->slab[SLAB_CONV], cfg->embed_dim, cfg->in_chans,
                                               cfg->patch_size, ctx->plan.conv_parts));
fail:
    if (d_amax)
        vh_free(d_amax);
    if (d_scaled)
        vh_free(d_scaled);
    return rc;
}

/* The weights of a context at another input size (vit_hip_create_at_size): everything device to device in the form
 * `from` holds it -- the operand, conv_proj and fold slabs whole (their layout does not depend on the input size; the caller has
 * checked the sizes), the fp32 tensors one by one into this context's SLAB_F32 layout -- except pos_embedding, resampled
 * from from's grid to this one's.  `from` is only read, after its stream has drained. */
static int derive_weights(vit_hip_ctx *ctx, const vit_hip_ctx *from, const vit_pos_resample *how)
{
    int rc = 0;
    static const int whole[] = {SLAB_OPERAND, SLAB_CONV, SLAB_FOLD};
    int gh_in, gw_in, gh_out, gw_out;
    vit_config_grid(&from->cfg, &gh_in, &gw_in);
    vit_config_grid(&ctx->cfg, &gh_out, &gw_out);
    TRY(vh_stream_sync(from->stream));
    for (size_t i = 0; i < sizeof(whole) / sizeof(whole[0]); ++i)
        if (ctx->plan.slab_bytes[whole[i]])
            TRY(vh_d2d(ctx->slab[whole[i]], from->slab[whole[i]], ctx->plan.slab_bytes[whole[i]], ctx->stream));
    for (int i = 0; i < ctx->n_tensors; ++i)
        if (i != 3)
            TRY(vh_d2d(ctx->w[i], from->w[i], vit_config_tensor_size(&ctx->cfg, i) * sizeof(float), ctx->stream));
    TRY(vh_launch_resample_pos_embed(ctx->stream, from->w[3], ctx->w[3], 1, gh_in, gw_in, gh_out, gw_out, ctx->cfg.embed_dim,
                                     how ? how->mode : VIT_POS_BICUBIC, how ? how->align_corners : 0));
fail:
    return rc;
}

static int alloc_arena(vit_hip_ctx *ctx);

/* A context from ctx_new to usable, for the three ways of making one: the device, the stream, the weight slabs -- filled
 * from the caller's tensors, read from an open planes file, or derived from another context's -- and the arena (which ends
 * by draining the stream).  On any failure the context is destroyed. */
static int ctx_finish(vit_hip_ctx *ctx, const Network *networks, struct planes_file *pf, const vit_hip_ctx *from,
                      const vit_pos_resample *how)
{
    int rc = 0;
    TRY(vh_init(ctx->device));
    TRY(vh_stream_create(&ctx->stream));
    TRY(alloc_weights(ctx));
    TRY(networks ? fill_weights(ctx, networks) : pf ? planes_file_read_slabs(pf, ctx->slab, ctx->stream) : derive_weights(ctx, from, how));
    TRY(alloc_arena(ctx));
    return 0;
fail:
    vit_hip_destroy(ctx);
    return rc;
}

/* $VIT_HIP_PRECISION picks the precision (plan_env_read) */
int vit_hip_create(vit_hip_ctx **out, const vit_config *cfg, const Network *networks,
                   int n_tensors, int device, int max_batch)
{
    struct plan_env env;
    plan_env_read(&env);
    return vit_hip_create_ex(out, cfg, networks, n_tensors, device, max_batch, env.precision);
}

int vit_hip_precision(const vit_hip_ctx *ctx) { return ctx->plan.precision; }
int vit_hip_ln_fold(const vit_hip_ctx *ctx) { return ctx ? ctx->plan.ln_fold : 0; }

/* Both ways of making a context: the empty context around the plan of its forward pass, which plan_make has accepted
 * (vit_hip_create_ex, where the plan decides the fold; planes_file_open, where the file's header fixed it).  Nothing is
 * allocated on the device. */
static int ctx_new(vit_hip_ctx **out, const vit_config *cfg, int n_tensors, int device, int max_batch, const struct vit_plan *plan)
{
    vit_hip_ctx *ctx = (vit_hip_ctx *)calloc(1, sizeof(*ctx));
    if (!ctx)
        return 4;
    ctx->cfg = *cfg;
    ctx->device = device;
    ctx->max_batch = max_batch;
    ctx->n_tensors = n_tensors;
    ctx->plan = *plan;
    ctx->w = (float **)calloc((size_t)n_tensors, sizeof(float *));
    ctx->op = (struct operand *)calloc((size_t)4 * cfg->depth, sizeof(struct operand));
    if (!ctx->w || !ctx->op) {
        free(ctx->w);
        free(ctx->op);
        free(ctx);
        return 4;
    }
    *out = ctx;
    return 0;
}

int vit_hip_create_ex(vit_hip_ctx **out, const vit_config *cfg_in, const Network *networks,
                      int n_tensors, int device, int max_batch, int precision)
{
    int rc = 0;
    if (!out)
        return 1;
    *out = NULL;
    if (!networks || !cfg_in)
        return 1;
    vit_config canon;   /* img_width == img_size stored as 0; another width checked here, before the tensors are looked at */
    if ((rc = vit_config_canonical(cfg_in, &canon, "vit_hip_create")) != 0)
        return rc;
    const vit_config *cfg = &canon;
    if (n_tensors != vit_config_num_tensors(cfg))
        return 2;
    /* The reference never checks its tensors (a missing file is a NULL
     * dereference, Network.c:144-148); here a wrong count is an error. */
    for (int i = 0; i < n_tensors; ++i)
        if (!networks[i].data || networks[i].size != vit_config_tensor_size(cfg, i)) {
            fprintf(stderr, "vit_hip_create: tensor %d has %zu elements, expected %zu\n", i,
                    networks[i].data ? networks[i].size : (size_t)0, vit_config_tensor_size(cfg, i));
            return 3;
        }
    struct plan_env env;
    struct vit_plan plan;
    plan_env_read(&env);
    if ((rc = plan_make(&plan, cfg, n_tensors, max_batch, precision, -1, &env)) != 0)
        return rc;
    vit_hip_ctx *ctx = NULL;
    if ((rc = ctx_new(&ctx, cfg, n_tensors, device, max_batch, &plan)) != 0)
        return rc;
    if ((rc = ctx_finish(ctx, networks, NULL, NULL, NULL)) != 0)
        return rc;
    *out = ctx;
    return 0;
}

/* The same model at another input size, from the weights `src` holds on its device (include/ViT_opencl.h).  Every refusal
 * falls before anything is allocated: the arguments (vit_resample_check_hw), the plan of the target shape under src's
 * precision and fold and this moment's switches, and the slabs that are copied whole.  square: the call came as
 * vit_hip_create_at_resolution, whose messages speak of one img_size. */
static int create_at_size(vit_hip_ctx **out, const vit_hip_ctx *src, int img_height, int img_width, int max_batch,
                          const vit_pos_resample *how, int square)
{
    int rc = 0;
    char msg[240];
    const char *const who = square ? "vit_hip_create_at_resolution" : "vit_hip_create_at_size";
    if (!out || !src) {
        if (out)
            *out = NULL;
        snprintf(msg, sizeof msg, "%s: null argument (%s)", who, out ? "src" : "out");
        return vh_set_error(1, msg);
    }
    *out = NULL;
    vit_config cfg;
    if ((rc = square ? vit_resample_check(&src->cfg, img_height, how, &cfg)
                     : vit_resample_check_hw(&src->cfg, img_height, img_width, how, &cfg)) != 0)
        return rc;
    if (max_batch <= 0)
        max_batch = src->max_batch;
    struct plan_env env;
    struct vit_plan plan;
    plan_env_read(&env);
    /* plan_make words most of its refusals itself; the others keep this text */
    snprintf(msg, sizeof msg, "%s: no plan runs the source's precision and LayerNorm fold at this img_size and max_batch", who);
    vh_set_error(2, msg);
    if ((rc = plan_make(&plan, &cfg, src->n_tensors, max_batch, src->plan.precision, src->plan.ln_fold, &env)) != 0)
        return rc;
    (void)vh_set_error(0, "");   /* accepted: that text was no failure */
    static const int whole[] = {SLAB_OPERAND, SLAB_CONV, SLAB_FOLD};
    for (size_t i = 0; i < sizeof(whole) / sizeof(whole[0]); ++i)
        if (plan.slab_bytes[whole[i]] != src->plan.slab_bytes[whole[i]]) {
            snprintf(msg, sizeof msg, "%s: weight slab %d would hold %zu bytes at img_size=%d, the source's holds %zu",
                     who, whole[i], plan.slab_bytes[whole[i]], img_height, src->plan.slab_bytes[whole[i]]);
            return vh_set_error(2, msg);
        }
    vit_hip_ctx *ctx = NULL;
    if ((rc = ctx_new(&ctx, &cfg, src->n_tensors, src->device, max_batch, &plan)) != 0) {
        snprintf(msg, sizeof msg, "%s: out of host memory", who);
        return vh_set_error(rc, msg);
    }
    for (int m = 0; m < 4 * cfg.depth; ++m)
        ctx->op[m].pair_scale = src->op[m].pair_scale;
    if ((rc = ctx_finish(ctx, NULL, NULL, src, how)) != 0)
        return rc;
    *out = ctx;
    return 0;
}

int vit_hip_create_at_size(vit_hip_ctx **out, const vit_hip_ctx *src, int img_height, int img_width, int max_batch,
                           const vit_pos_resample *how)
{
    return create_at_size(out, src, img_height, img_width, max_batch, how, 0);
}

int vit_hip_create_at_resolution(vit_hip_ctx **out, const vit_hip_ctx *src, int img_size, int max_batch,
                                 const vit_pos_resample *how)
{
    return create_at_size(out, src, img_size, img_size, max_batch, how, 1);
}

/* ---- repacked weights on disk: the format, the writer and the reader are csrc/vit_planes_file.c ---------------------- */

/* The planes file keeps one fp16-pair scale per tensor index: zero but at the big matrices of F32_FP16X2. */
static void pair_scales(const vit_hip_ctx *ctx, float scales[MAX_TENSORS])
{
    memset(scales, 0, sizeof(float) * (size_t)ctx->n_tensors);
    for (int m = 0; m < 4 * ctx->cfg.depth; ++m)
        scales[plan_operand_tensor(m)] = ctx->op[m].pair_scale;
}

int vit_hip_export_planes(vit_hip_ctx *ctx, const char *path)
{
    int rc = 0;
    if (!ctx || !path)
        return vh_set_error(1, "vit_hip_export_planes: null argument");
    if (ctx->cfg.img_width != 0)   /* the header pins one side; nothing but pos_embedding depends on the size */
        return vh_set_error(1, "vit_hip_export_planes: the context's input is non-square and the file's header holds one side: "
                               "export the square context and derive this one from it (vit_hip_create_at_size)");
    if ((rc = vh_set_device(ctx->device)) != 0)
        return rc;
    float scales[MAX_TENSORS];
    pair_scales(ctx, scales);
    return planes_file_write(path, &ctx->cfg, &ctx->plan, ctx->n_tensors, scales, ctx->slab, ctx->stream);
}

/* The header decides shape, precision and fold (planes_file_open: every refusal falls there, before a device is touched or
 * anything allocated); the context adopts its plan and the slabs are read into their allocations. */
int vit_hip_create_from_planes(vit_hip_ctx **out, const char *path, int device, int max_batch)
{
    int rc = 0;
    struct planes_file pf;
    if (!out)
        return 1;
    *out = NULL;
    if ((rc = planes_file_open(&pf, path, max_batch)) != 0)
        return rc;
    vit_hip_ctx *ctx = NULL;
    if ((rc = ctx_new(&ctx, &pf.cfg, pf.n_tensors, device, max_batch, &pf.plan)) == 0) {
        for (int m = 0; m < 4 * pf.cfg.depth; ++m)
            ctx->op[m].pair_scale = pf.scales[plan_operand_tensor(m)];
        if ((rc = ctx_finish(ctx, NULL, &pf, NULL, NULL)) == 0)
            *out = ctx;
    } else   /* out of host memory: the status with the text it has always come with */
        vh_set_error(rc, "vit_hip_create_from_planes: the header's model shape or precision is not one this library takes");
    planes_file_close(&pf);
    return rc;
}

/* The activation arena, of the plan's sizes, and the host-pointer path's pipeline, sized for max_batch images. */
static int alloc_arena(vit_hip_ctx *ctx)
{
    int rc = 0;
    const vit_config *cfg = &ctx->cfg;
    const struct vit_plan *plan = &ctx->plan;
    const int max_batch = ctx->max_batch;
    const size_t E = (size_t)cfg->embed_dim, NC = (size_t)cfg->num_classes;
    TRY(vh_malloc((void **)&ctx->x, plan->x_bytes));
    TRY(vh_malloc((void **)&ctx->y, plan->y_bytes));
    TRY(vh_malloc((void **)&ctx->attn, plan->attn_bytes));
    TRY(vh_malloc((void **)&ctx->qkv, plan->qkv_bytes));
    TRY(vh_malloc((void **)&ctx->hid, plan->ws_bytes));
    if (plan->stats_bytes)
        TRY(vh_malloc((void **)&ctx->stats, plan->stats_bytes));
    TRY(vh_malloc((void **)&ctx->cls, (size_t)max_batch * E * sizeof(float)));
    TRY(vh_malloc((void **)&ctx->d_logits, (size_t)max_batch * NC * sizeof(float)));
    TRY(vh_malloc((void **)&ctx->d_probs, (size_t)max_batch * NC * sizeof(float)));
    const struct pipeline_model pm = {.device = ctx->device, .max_batch = max_batch, .classes = cfg->num_classes, .stream = ctx->stream,
                                      .image_bytes = (size_t)cfg->in_chans * cfg->img_size * ctx_width(ctx) * sizeof(float),
                                      .d_logits = ctx->d_logits, .d_probs = ctx->d_probs};
    TRY(pipeline_make(&ctx->pipe, &pm));
    TRY(vh_stream_sync(ctx->stream));
    return 0;
fail:
    return rc;
}

/* ---- one encoder layer per arithmetic (ViT_seq.c:330-370; Encoder ViT_opencl.c:710-748) ------------------------------
 * Every function enqueues layer l for n images on stream s: y = LN1(x); qkv = y Win^T + bin; a = attention(qkv);
 * x += a Wout^T + bout; y = LN2(x); h = gelu(y W1^T + b1); x += h W2^T + b2 -- in its mode's operand formats.  With
 * ctx->plan.ln_fold the two LayerNorms are not launched: whoever wrote x also left it as the projection's operand in ctx->y
 * with the rows' partial sums in ctx->stats, and the QKV / fc1 launches apply the row terms (csrc/norm_fold.h). */

/* The plan's arithmetic for fp32 products on fp32 rows (kernelHandler.h) */
static int fp32_math(const vit_hip_ctx *ctx) { return ctx->plan.fp32_native ? VH_FP32_NATIVE : VH_FP32_SPLIT3; }

/* Attention on fp32 Q|K|V rows into fp32 rows at out, in the plan's kernel */
static int attention_rows(const vit_hip_ctx *ctx, vh_stream_t s, float *out, int arith, int n)
{
    return vh_launch_attention_rows(s, ctx->qkv, out, 0, arith, ctx->plan.attn_rows_streaming ? VH_ATTN_STREAMING : VH_ATTN_AUTO, n,
                                    ctx->plan.tokens, ctx->cfg.embed_dim, ctx->cfg.num_heads);
}

/* The class-token attention maps of layer l when the forward's armed request taps it: one pass over q_cls and the K
 * columns of the Q|K|V the projection has just completed, in the form the plan made it write (csrc/attn_map.hip), timed
 * with the attention.  Called between the QKV and the attention launch: nothing that reuses the buffer -- the attention's
 * output, the class-only last layer's scratch, the next layer's projection -- is earlier in stream order. */
static int attention_tap(vit_hip_ctx *ctx, vh_stream_t s, int n, int l)
{
    int rc = 0;
    const struct attn_req *ar = ctx->serving->ar;
    const struct rollout_req *ro = ctx->serving->ro;
    const vit_config *c = &ctx->cfg;
    for (int k = 0; ar && k < ar->spec.n_taps; ++k)
        if (ar->layer[k] == l)
            OP(VIT_OP_ATTENTION, vh_launch_cls_attention(s, ctx->qkv, ctx->plan.qkv_form, n, ctx->plan.tokens, c->embed_dim, c->num_heads, k,
                                                         ar->spec.n_taps, ar->out.heads, ar->out.mean));
    /* the armed rollout request: this layer's head-mean attention matrix folded into the running product, which
     * ping-pongs between the request's two buffers (csrc/rollout.hip); forward_device reads the class row behind the last
     * layer */
    if (ro && l >= ro->first)
        OP(VIT_OP_ATTENTION, vh_launch_rollout_step(s, ctx->qkv, ctx->plan.qkv_form, n, ctx->plan.tokens, c->embed_dim, c->num_heads,
                                                    l == ro->first ? NULL : (const float *)ro->head.scratch[(l - ro->first + 1) & 1],
                                                    (float *)ro->head.scratch[(l - ro->first) & 1], ro->head.scratch[2]));
    return 0;
fail:
    return rc;
}

/* The reduced modes' attention on fp16-rounded operands, writing the output projection's operand: one-part bf16 planes
 * (attn_scales NULL) or an MX tensor.  The resident kernels write it themselves; the streaming kernel leaves fp32 rows in
 * the idle MLP buffer, which are then rounded / quantised (one timed operator). */
static int attention_reduced(vit_hip_ctx *ctx, vh_stream_t s, int n, char *attn_scales)
{
    int rc = 0;
    const vit_config *c = &ctx->cfg;
    const int E = c->embed_dim, T = ctx->plan.tokens, H = c->num_heads, rows = n * T;
    if (ctx->plan.attn_form == ATTN_HD64)
        OP(VIT_OP_ATTENTION, attn_scales ? vh_launch_attention_planes_f16_mx(s, ctx->qkv, ctx->attn, attn_scales, n, T, E, H)
                                         : vh_launch_attention_planes_f16(s, ctx->qkv, ctx->attn, 1, n, T, E, H));
    else if (ctx->plan.attn_form == ATTN_HD80)
        OP(VIT_OP_ATTENTION, vh_launch_attention_planes_f16_hd80_operand(s, ctx->qkv, ctx->attn, attn_scales, attn_scales ? 2 : 1, n, T, E, H));
    else if (ctx->plan.attn_form == ATTN_LONG)
        OP(VIT_OP_ATTENTION, (rc = vh_launch_attention_long(s, ctx->qkv, 1, ctx->hid, n, T, E, H)) != 0 ? rc :
                             attn_scales ? vh_launch_quantize_mx_act(s, ctx->hid, ctx->attn, attn_scales, rows, E)
                                         : vh_launch_split_rows(s, ctx->hid, ctx->attn, rows, E, 1));
    else
        OP(VIT_OP_ATTENTION, (rc = attention_rows(ctx, s, ctx->hid, VH_ATTN_FP16, n)) != 0 ? rc :
                             attn_scales ? vh_launch_quantize_mx_act(s, ctx->hid, ctx->attn, attn_scales, rows, E)
                                         : vh_launch_split_rows(s, ctx->hid, ctx->attn, rows, E, 1));
    return 0;
fail:
    return rc;
}

/* FP8_GEMM: y, attn and hid hold MX tensors (values, then the scales, in the same allocations) */
static int layer_fp8(vit_hip_ctx *ctx, vh_stream_t s, int n, int l)
{
    int rc = 0;
    const vit_config *c = &ctx->cfg;
    const int E = c->embed_dim, F = c->mlp_hidden, rows = n * ctx->plan.tokens, fold = ctx->plan.ln_fold, last = l == c->depth - 1;
    float **lw = layer_tensors(ctx, l);
    const struct operand *op = ctx->op + 4 * l;
    char *ys = (char *)ctx->y + ctx->plan.e_scales_off, *as_ = (char *)ctx->attn + ctx->plan.e_scales_off;
    char *hs = (char *)ctx->hid + ctx->plan.hid_scales_off;
    const int kind = ctx->plan.qkv_form == VH_QKV_PLANES_F16 ? 2 : 0;   /* Q|K|V as one-part fp16 planes, or as fp32 rows */
    if (!fold)
        OP(VIT_OP_LAYER_NORM, vh_launch_layer_norm_mx(s, ctx->x, lw[0], lw[1], ctx->y, ys, rows, E, E, c->eps));
    OP(VIT_OP_QKV, fold ? vh_launch_linear_mx_norm(s, ctx->qkv, NULL, kind, op[0].w, op[0].scales, ctx->y, ys, ctx->stats, op[0].colsum, op[0].bias_folded, c->eps, rows, E, 3 * E, 0)
                 : kind ? vh_launch_linear_mx_planes_f16(s, ctx->qkv, op[0].w, op[0].scales, ctx->y, ys, lw[3], rows, E, 3 * E)
                        : vh_launch_linear_mx(s, ctx->qkv, NULL, op[0].w, op[0].scales, ctx->y, ys, lw[3], rows, E, 3 * E, 0, NULL));
    TRY(attention_tap(ctx, s, n, l));
    TRY(attention_reduced(ctx, s, n, as_));
    OP(VIT_OP_OUT_PROJ, fold ? vh_launch_linear_mx_resid_norm(s, ctx->x, op[1].w, op[1].scales, ctx->attn, as_, lw[5], ctx->x, rows, E, E, ctx->y, ys, ctx->stats)
                             : vh_launch_linear_mx(s, ctx->x, NULL, op[1].w, op[1].scales, ctx->attn, as_, lw[5], rows, E, E, 0, ctx->x));
    if (!fold)
        OP(VIT_OP_LAYER_NORM, vh_launch_layer_norm_mx(s, ctx->x, lw[6], lw[7], ctx->y, ys, rows, E, E, c->eps));
    OP(VIT_OP_FC1, fold ? vh_launch_linear_mx_norm(s, ctx->hid, hs, 1, op[2].w, op[2].scales, ctx->y, ys, ctx->stats, op[2].colsum, op[2].bias_folded, c->eps, rows, E, F, 1)
                        : vh_launch_linear_mx(s, ctx->hid, hs, op[2].w, op[2].scales, ctx->y, ys, lw[9], rows, E, F, 1, NULL));
    /* nothing reads the operand behind the last layer: the final LayerNorm takes the fp32 rows */
    OP(VIT_OP_FC2, fold && !last ? vh_launch_linear_mx_resid_norm(s, ctx->x, op[3].w, op[3].scales, ctx->hid, hs, lw[11], ctx->x, rows, F, E, ctx->y, ys, ctx->stats)
                                 : vh_launch_linear_mx(s, ctx->x, NULL, op[3].w, op[3].scales, ctx->hid, hs, lw[11], rows, F, E, 0, ctx->x));
    return 0;
fail:
    return rc;
}

/* BF16_GEMM: operands as one-part planes [K/32][1][rows][32] written by their producers; the fp32 path's kernel with one
 * product per block (gemm_p3.hip, NPL = 1) */
static int layer_bf16(vit_hip_ctx *ctx, vh_stream_t s, int n, int l)
{
    int rc = 0;
    const vit_config *c = &ctx->cfg;
    const int E = c->embed_dim, F = c->mlp_hidden, rows = n * ctx->plan.tokens, fold = ctx->plan.ln_fold, last = l == c->depth - 1;
    float **lw = layer_tensors(ctx, l);
    const struct operand *op = ctx->op + 4 * l;
    const int kind = ctx->plan.qkv_form == VH_QKV_PLANES_F16 ? 2 : 0;
    if (!fold)
        OP(VIT_OP_LAYER_NORM, vh_launch_layer_norm_planes(s, ctx->x, lw[0], lw[1], ctx->y, 1, rows, E, E, c->eps));
    OP(VIT_OP_QKV, fold ? vh_launch_linear_planes_norm(s, ctx->qkv, kind, op[0].w, ctx->y, ctx->stats, op[0].colsum, op[0].bias_folded, c->eps, rows, E, 3 * E, 0)
                        : vh_launch_linear_planes(s, ctx->qkv, kind, op[0].w, ctx->y, 1, lw[3], rows, E, 3 * E, 0, NULL));
    TRY(attention_tap(ctx, s, n, l));
    TRY(attention_reduced(ctx, s, n, NULL));
    OP(VIT_OP_OUT_PROJ, fold ? vh_launch_linear_planes_resid_norm(s, ctx->x, op[1].w, ctx->attn, lw[5], ctx->x, rows, E, E, ctx->y, NULL, ctx->stats)
                             : vh_launch_linear_planes(s, ctx->x, 0, op[1].w, ctx->attn, 1, lw[5], rows, E, E, 0, ctx->x));
    if (!fold)
        OP(VIT_OP_LAYER_NORM, vh_launch_layer_norm_planes(s, ctx->x, lw[6], lw[7], ctx->y, 1, rows, E, E, c->eps));
    OP(VIT_OP_FC1, fold ? vh_launch_linear_planes_norm(s, ctx->hid, 1, op[2].w, ctx->y, ctx->stats, op[2].colsum, op[2].bias_folded, c->eps, rows, E, F, 1)
                        : vh_launch_linear_planes(s, ctx->hid, 1, op[2].w, ctx->y, 1, lw[9], rows, E, F, 1, NULL));
    OP(VIT_OP_FC2, fold && !last ? vh_launch_linear_planes_resid_norm(s, ctx->x, op[3].w, ctx->hid, lw[11], ctx->x, rows, F, E, ctx->y, NULL, ctx->stats)
                                 : vh_launch_linear_planes(s, ctx->x, 0, op[3].w, ctx->hid, 1, lw[11], rows, F, E, 0, ctx->x));
    return 0;
fail:
    return rc;
}

/* F32_FP16X2: the fp32 layer with the four projections on two fp16 parts / three products */
static int layer_fp16x2(vit_hip_ctx *ctx, vh_stream_t s, int n, int l)
{
    int rc = 0;
    const vit_config *c = &ctx->cfg;
    const int E = c->embed_dim, F = c->mlp_hidden, T = ctx->plan.tokens, rows = n * T;
    float **lw = layer_tensors(ctx, l);
    const struct operand *op = ctx->op + 4 * l;
    OP(VIT_OP_LAYER_NORM, vh_launch_layer_norm(s, ctx->x, lw[0], lw[1], ctx->y, rows, E, E, E, c->eps));
    OP(VIT_OP_QKV, vh_launch_linear_h2(s, ctx->qkv, op[0].w, op[0].pair_scale, ctx->y, lw[3], rows, E, 3 * E, 0, NULL));
    TRY(attention_tap(ctx, s, n, l));
    OP(VIT_OP_ATTENTION, attention_rows(ctx, s, ctx->attn, VH_ATTN_FP16X2, n));
    OP(VIT_OP_OUT_PROJ, vh_launch_linear_h2(s, ctx->x, op[1].w, op[1].pair_scale, ctx->attn, lw[5], rows, E, E, 0, ctx->x));
    OP(VIT_OP_LAYER_NORM, vh_launch_layer_norm(s, ctx->x, lw[6], lw[7], ctx->y, rows, E, E, E, c->eps));
    OP(VIT_OP_FC1, vh_launch_linear_h2(s, ctx->hid, op[2].w, op[2].pair_scale, ctx->y, lw[9], rows, E, F, 1, NULL));
    OP(VIT_OP_FC2, vh_launch_linear_h2(s, ctx->x, op[3].w, op[3].pair_scale, ctx->hid, lw[11], rows, F, E, 0, ctx->x));
    return 0;
fail:
    return rc;
}

/* Layer l of the fp32 path on planes from LN1's output in y to the attention's in attn, on all rows: the QKV projection, the
 * armed attention taps, the attention.  ATTN_HD64, ATTN_LONG: Q, K, V too travel as planes (only the probabilities are split
 * inside the attention kernel); otherwise the streaming kernel, fp32 rows in.  Both but the resident kernel write fp32 rows
 * (into the idle MLP buffer), then split.  timed: the launches of a forward; 0 when finish_last_layer runs them afterwards,
 * outside every forward's operator times and with nothing armed to serve. */
static int layer_f32_planes_attention(vit_hip_ctx *ctx, vh_stream_t s, int n, int l, int timed)
{
    int rc = 0;
    const vit_config *c = &ctx->cfg;
    const int E = c->embed_dim, T = ctx->plan.tokens, rows = n * T, fold = ctx->plan.ln_fold;
    float **lw = layer_tensors(ctx, l);
    const struct operand *op = ctx->op + 4 * l;
    const int planes_attn = ctx->plan.qkv_form == VH_QKV_PLANES3;
    OP_T(timed, VIT_OP_QKV, fold ? vh_launch_linear_p3_norm(s, ctx->qkv, planes_attn, op[0].w, ctx->y, ctx->stats, op[0].colsum, op[0].bias_folded, c->eps, rows, E, 3 * E, 0)
                                 : vh_launch_linear_p3(s, ctx->qkv, planes_attn, op[0].w, ctx->y, lw[3], rows, E, 3 * E, 0, NULL));
    if (timed)
        TRY(attention_tap(ctx, s, n, l));
    OP_T(timed, VIT_OP_ATTENTION, ctx->plan.attn_form == ATTN_HD64 ? vh_launch_attention_planes(s, ctx->qkv, ctx->attn, n, T, E, c->num_heads)
                                  : (rc = ctx->plan.attn_form == ATTN_LONG ? vh_launch_attention_long(s, ctx->qkv, 3, ctx->hid, n, T, E, c->num_heads)
                                                                      : attention_rows(ctx, s, ctx->hid, VH_ATTN_SPLIT3, n)) != 0 ? rc
                                  : vh_launch_split3_rows(s, ctx->hid, ctx->attn, rows, E));
    return 0;
fail:
    return rc;
}

/* ... and behind its attention, on all rows: output projection, LayerNorm, MLP */
static int layer_f32_planes_tail(vit_hip_ctx *ctx, vh_stream_t s, int n, int l, int timed)
{
    int rc = 0;
    const vit_config *c = &ctx->cfg;
    const int E = c->embed_dim, F = c->mlp_hidden, rows = n * ctx->plan.tokens, fold = ctx->plan.ln_fold, last = l == c->depth - 1;
    float **lw = layer_tensors(ctx, l);
    const struct operand *op = ctx->op + 4 * l;
    OP_T(timed, VIT_OP_OUT_PROJ, fold ? vh_launch_linear_p3_resid_norm(s, ctx->x, op[1].w, ctx->attn, lw[5], ctx->x, rows, E, E, ctx->y, ctx->stats)
                                      : vh_launch_linear_p3(s, ctx->x, 0, op[1].w, ctx->attn, lw[5], rows, E, E, 0, ctx->x));
    if (!fold)
        OP_T(timed, VIT_OP_LAYER_NORM, vh_launch_layer_norm_p3(s, ctx->x, lw[6], lw[7], ctx->y, rows, E, E, c->eps));
    OP_T(timed, VIT_OP_FC1, fold ? vh_launch_linear_p3_norm(s, ctx->hid, 1, op[2].w, ctx->y, ctx->stats, op[2].colsum, op[2].bias_folded, c->eps, rows, E, F, 1)
                                 : vh_launch_linear_p3(s, ctx->hid, 1, op[2].w, ctx->y, lw[9], rows, E, F, 1, NULL));
    OP_T(timed, VIT_OP_FC2, fold && !last ? vh_launch_linear_p3_resid_norm(s, ctx->x, op[3].w, ctx->hid, lw[11], ctx->x, rows, F, E, ctx->y, ctx->stats)
                                          : vh_launch_linear_p3(s, ctx->x, 0, op[3].w, ctx->hid, lw[11], rows, F, E, 0, ctx->x));
    return 0;
fail:
    return rc;
}

/* What a forward on the class-rows path left pending: the last layer on all rows of those images, from what that forward
 * left untouched -- the pre-projection residual in x and the attention output in attn; where it ran Q and the attention for
 * the class query alone (last_pending_attention), from LN1's planes in y through the QKV projection and the attention
 * again.  The launches of the full layer on the same operands, on the context's stream: the residual stream is then the
 * full evaluation's, bit for bit (y holds LN2's output and hid the MLP's, as behind a full layer). */
static int finish_last_layer(vit_hip_ctx *ctx)
{
    int rc = 0;
    const int n = ctx->last_pending, l = ctx->cfg.depth - 1;
    if (!n)
        return 0;
    if (ctx->last_pending_attention)
        TRY(layer_f32_planes_attention(ctx, ctx->stream, n, l, 0));
    TRY(layer_f32_planes_tail(ctx, ctx->stream, n, l, 0));
    ctx->last_pending = ctx->last_pending_attention = 0;
fail:
    return rc;
}

/* An armed attention-map tap on layer l, or the rollout from a layer up to l: they read all of Q|K|V behind l's projection */
static int attention_tap_reads(const vit_hip_ctx *ctx, int l)
{
    const struct attn_req *ar = ctx->serving->ar;
    const struct rollout_req *ro = ctx->serving->ro;
    for (int k = 0; ar && k < ar->spec.n_taps; ++k)
        if (ar->layer[k] == l)
            return 1;
    return ro && l >= ro->first;
}

/* F32, the default: GEMM inputs as exact three-part planes written by LayerNorm, attention and the fc1 epilogue.  ln_fold
 * here is the LAB VARIANT ($VIT_HIP_LN_FOLD=1, docs/LABBOOK.md R4.6): ctx->y then holds the split of x itself.
 * cls_only: this forward runs the last layer behind its attention on the class-token rows only (the default where the plan
 * allows it); *cls_rows is set when it did (2: Q and the attention too ran for the class query alone): the final LayerNorm
 * then reads them compacted at the start of the Q|K|V buffer. */
static int layer_f32_planes(vit_hip_ctx *ctx, vh_stream_t s, int n, int l, int cls_only, int *cls_rows)
{
    int rc = 0;
    const vit_config *c = &ctx->cfg;
    const int E = c->embed_dim, F = c->mlp_hidden, T = ctx->plan.tokens, rows = n * T, fold = ctx->plan.ln_fold, last = l == c->depth - 1;
    float **lw = layer_tensors(ctx, l);
    const struct operand *op = ctx->op + 4 * l;
    if (!fold)
        OP(VIT_OP_LAYER_NORM, vh_launch_layer_norm_p3(s, ctx->x, lw[0], lw[1], ctx->y, rows, E, E, c->eps));
    if (last && cls_only) {
        /* The classifier reads row 0 of every image only (ViT_seq.c:511), and behind the last attention no operator
         * mixes rows: the output projection, LayerNorm and MLP of the last layer are evaluated for the n class-token
         * rows instead of n * T, in the Q|K|V buffer the attention has just released.  Same kernels, same k order:
         * identical logits, bit for bit.  x, attn and y are left as they are: the other rows stay computable
         * (finish_last_layer).  The three projections are timed under operator names of their own, so that the full-size
         * operators' means stay those of full-size launches. */
        size_t off[3], q_off;
        plan_cls_only_scratch(c, n, off);   /* cls_only_ok: it fits for max_batch rows */
        plan_cls_query_scratch(c, n, &q_off);
        char *scratch = (char *)ctx->qkv;
        float *x_cls = (float *)scratch;
        char *attn_cls = scratch + off[0], *y_cls = scratch + off[1], *hid_cls = scratch + off[2], *q_cls = scratch + q_off;
        const int cls_query = ctx->plan.cls_query && !attention_tap_reads(ctx, l);
        if (cls_query) {
            /* The rows that are skipped are all that Q and the attention output of the patch rows feed: K and V on all rows,
             * into their place in Q|K|V; Q for the gathered class rows of LN1's planes, by the same kernels column range by
             * column range; the attention for the class query alone, straight into attn_cls.  The scratch lies in the place
             * of the Q planes (plan.cls_query: it fits there at every n).  Timed with the QKV projections and the attentions. */
            char *kv = scratch + (size_t)rows * E * 6;
            OP(VIT_OP_QKV, (rc = vh_launch_linear_p3_cols(s, kv, 1, (const char *)op[0].w + (size_t)E * 64, 3 * E, ctx->y, lw[3] + E, rows, E, 2 * E)) != 0 ? rc :
                           (rc = vh_launch_gather_rows(s, ctx->y, y_cls, 3 * (E / 32), rows, n, 64, T)) != 0 ? rc :
                           vh_launch_linear_p3_cols(s, q_cls, 1, op[0].w, 3 * E, y_cls, lw[3], n, E, E));
            OP(VIT_OP_ATTENTION, vh_launch_attention_planes_cls(s, ctx->qkv, q_cls, attn_cls, n, T, E, c->num_heads));
        } else {
            TRY(layer_f32_planes_attention(ctx, s, n, l, 1));
        }
        OP(VIT_OP_OUT_PROJ_CLS, (rc = cls_query ? 0 : vh_launch_gather_rows(s, ctx->attn, attn_cls, 3 * (E / 32), rows, n, 64, T)) != 0 ? rc :
                                (rc = vh_launch_gather_rows(s, ctx->x, x_cls, 1, rows, n, 4 * E, T)) != 0 ? rc :
                                vh_launch_linear_p3(s, x_cls, 0, op[1].w, attn_cls, lw[5], n, E, E, 0, x_cls));
        OP(VIT_OP_LAYER_NORM, vh_launch_layer_norm_p3(s, x_cls, lw[6], lw[7], y_cls, n, E, E, c->eps));
        OP(VIT_OP_FC1_CLS, vh_launch_linear_p3(s, hid_cls, 1, op[2].w, y_cls, lw[9], n, E, F, 1, NULL));
        OP(VIT_OP_FC2_CLS, vh_launch_linear_p3(s, x_cls, 0, op[3].w, hid_cls, lw[11], n, F, E, 0, x_cls));
        *cls_rows = cls_query ? 2 : 1;
        return 0;
    }
    TRY(layer_f32_planes_attention(ctx, s, n, l, 1));
    return layer_f32_planes_tail(ctx, s, n, l, 1);
fail:
    return rc;
}

/* F32 with fp32 activation rows ($VIT_HIP_P3=0, $VIT_HIP_GEMM_FP32=native, or shapes the planes cannot take): round 1's
 * kernels, operands split inside the K loop (pre-split weight planes when built) or the native fp32 MFMA */
static int layer_f32_rows(vit_hip_ctx *ctx, vh_stream_t s, int n, int l)
{
    int rc = 0;
    const vit_config *c = &ctx->cfg;
    const int E = c->embed_dim, F = c->mlp_hidden, T = ctx->plan.tokens, rows = n * T;
    float **lw = layer_tensors(ctx, l);
    const struct operand *op = ctx->op + 4 * l;   /* pre-split weight planes, when built */
    const int math = fp32_math(ctx);
    OP(VIT_OP_LAYER_NORM, vh_launch_layer_norm(s, ctx->x, lw[0], lw[1], ctx->y, rows, E, E, E, c->eps));
    OP(VIT_OP_QKV, op[0].w ? vh_launch_linear_w3(s, ctx->qkv, op[0].w, ctx->y, lw[3], rows, E, 3 * E, 0, NULL)
                         : vh_launch_linear_math(s, ctx->qkv, lw[2], ctx->y, lw[3], rows, E, 3 * E, 0, NULL, math));
    TRY(attention_tap(ctx, s, n, l));
    OP(VIT_OP_ATTENTION, attention_rows(ctx, s, ctx->attn, ctx->plan.fp32_native ? VH_ATTN_NATIVE : VH_ATTN_SPLIT3, n));
    OP(VIT_OP_OUT_PROJ, op[1].w ? vh_launch_linear_w3(s, ctx->x, op[1].w, ctx->attn, lw[5], rows, E, E, 0, ctx->x)
                              : vh_launch_linear_math(s, ctx->x, lw[4], ctx->attn, lw[5], rows, E, E, 0, ctx->x, math));
    OP(VIT_OP_LAYER_NORM, vh_launch_layer_norm(s, ctx->x, lw[6], lw[7], ctx->y, rows, E, E, E, c->eps));
    OP(VIT_OP_FC1, op[2].w ? vh_launch_linear_w3(s, ctx->hid, op[2].w, ctx->y, lw[9], rows, E, F, 1, NULL)
                         : vh_launch_linear_math(s, ctx->hid, lw[8], ctx->y, lw[9], rows, E, F, 1, NULL, math));
    OP(VIT_OP_FC2, op[3].w ? vh_launch_linear_w3(s, ctx->x, op[3].w, ctx->hid, lw[11], rows, F, E, 0, ctx->x)
                          : vh_launch_linear_math(s, ctx->x, lw[10], ctx->hid, lw[11], rows, F, E, 0, ctx->x, math));
    return 0;
fail:
    return rc;
}

/* Queue the resize of the n validated crops of src (device data: its images where they lie whole, or the items of a staged
 * chunk) into out, [n][img][img][C] bytes: the descriptors go up through the next ring slot, the coefficient tables into
 * hid.  The slot's event is recorded behind the launches that read it. */
static int resize_crop_launch(vit_hip_ctx *ctx, vh_stream_t s, const struct ingest_src *src, int n, unsigned char *out)
{
    int rc_ = 0;
    const vit_config *c = &ctx->cfg;
    const int filter = ingest_filter(src);
    const int S = c->img_size, C = c->in_chans;
    vh_resize_desc *d, *d_desc;
    if ((rc_ = pipeline_desc_take(&ctx->pipe, &d, &d_desc)) != 0)
        return rc_;
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        const struct ingest_item item = src->items ? src->items[i] : ingest_whole_item(src, i);
        off += ingest_fill_desc(&d[i], &item, S, filter, off);
    }
    if (off > ctx->plan.ws_bytes)   /* the plan sized hid for max_batch tables at the steepest downscale */
        return vh_set_error(1, "resize: coefficient tables exceed the scratch");
    if ((rc_ = vh_h2d(d_desc, d, (size_t)n * sizeof(*d), s)) != 0)
        return rc_;
    rc_ = vh_launch_resize_crop_u8(s, d_desc, n, C, src->layout, filter, S, ctx->hid, ctx->plan.ws_bytes, out);
    const int rec = pipeline_desc_done(&ctx->pipe, s);   /* behind the copy even if the launch was refused */
    return rc_ ? rc_ : rec;
}

/* patch embedding + class token + position embedding (ViT_seq.c:437-443), in the form the mode's first layer reads.  8-bit
 * pixels: the planes paths' im2row producer normalises them as it gathers; the fp32-rows paths expand them first into the
 * Q|K|V buffer (idle here; the plan makes it hold max_batch fp32 images).  All of it is one VIT_OP_PATCH_EMBED. */
static int patch_embed_launches(vit_hip_ctx *ctx, vh_stream_t s, const struct ingest_src *src, int n)
{
    const vit_config *c = &ctx->cfg;
    const int E = c->embed_dim;
    float **w = ctx->w;
    void *conv = ctx->slab[SLAB_CONV];
    /* ln_fold: y receives the token rows as the first projection's operand -- planes, or MX values with their scales behind
     * them -- and stats their partial sums (class-token rows included) */
    char *const y_scales = ctx->plan.precision == VIT_PRECISION_FP8_GEMM ? (char *)ctx->y + ctx->plan.e_scales_off : NULL;
    const int img_h = c->img_size, img_w = ctx_width(ctx);
    if (ctx->plan.planes_patch_embed) {
        /* one launcher for every planes variant: the fp32 or the 8-bit pixels (normalised as they are gathered), the plan's
         * parts -- three on the fp32 path, one in the reduced modes -- and, under ln_fold, the first projection's operand */
        const int fold = ctx->plan.ln_fold;
        return vh_launch_patch_embed_planes_hw(s, src->u8 ? NULL : src->f32, src->u8, src->layout, src->u8 ? src->norm->scale : NULL,
                                               src->u8 ? src->norm->bias : NULL, conv, w[2], w[0], w[3], ctx->x, n, c->in_chans, img_h,
                                               img_w, c->patch_size, E, ctx->hid, ctx->plan.ws_bytes, ctx->plan.conv_parts,
                                               fold ? ctx->y : NULL, fold ? y_scales : NULL, fold ? ctx->stats : NULL);
    }
    const float *images = src->f32;
    if (src->u8) {
        const int rc = vh_launch_expand_u8_hw(s, src->u8, src->layout, src->norm->scale, src->norm->bias, ctx->qkv, n, c->in_chans,
                                              img_h, img_w);
        if (rc)
            return rc;
        images = ctx->qkv;
    }
    return vh_launch_patch_embed_rows_hw(s, images, w[1], w[2], w[0], w[3], ctx->x, n, c->in_chans, img_h, img_w, c->patch_size, E,
                                         ctx->hid, ctx->plan.ws_bytes, fp32_math(ctx));
}

/* The readout behind layer l for tap k of the armed request: one pass over the residual stream (the class rows alone when
 * only cls is asked for), timed with the LayerNorms.  Partial sums of pooled go through the MLP buffer, idle behind fc2.
 * cls_rows: the last layer ran class-only, its class rows lie compacted at the start of Q|K|V. */
static int feature_tap(vit_hip_ctx *ctx, vh_stream_t s, const struct feature_req *fr, int k, int n, int cls_rows)
{
    int rc = 0;
    const vit_config *c = &ctx->cfg;
    float **tw = ctx->w + 4 + 12 * c->depth;
    OP(VIT_OP_LAYER_NORM, vh_launch_feature_readout(s, ctx->x, cls_rows ? (const float *)ctx->qkv : NULL, c->embed_dim, tw[0], tw[1],
                                                    c->eps, fr->spec.final_norm, fr->spec.l2_normalize, fr->spec.dtype,
                                                    fr->spec.token_layout, n, ctx->plan.tokens, c->embed_dim, k, fr->spec.n_taps,
                                                    fr->out.cls, fr->out.pooled, fr->out.tokens, ctx->hid, ctx->plan.ws_bytes));
    return 0;
fail:
    return rc;
}

/* The armed gallery request behind its layer: the queries by the feature readout (cls_rows as feature_tap), then the search
 * against the caller's rows, timed with the classifier */
static int gallery_tap(vit_hip_ctx *ctx, vh_stream_t s, const struct gallery_req *ga, int n, int cls_rows)
{
    int rc = 0;
    const vit_config *c = &ctx->cfg;
    float **tw = ctx->w + 4 + 12 * c->depth;
    const int pooled = ga->spec.source == VIT_GALLERY_POOLED;
    OP(VIT_OP_HEAD, vh_launch_feature_readout(s, ctx->x, cls_rows ? (const float *)ctx->qkv : NULL, c->embed_dim, tw[0], tw[1], c->eps,
                                              ga->spec.final_norm, ga->spec.l2_normalize, VIT_FEATURE_F32, VIT_TOKENS_NLC, n,
                                              ctx->plan.tokens, c->embed_dim, 0, 1, pooled ? NULL : ga->head.scratch[0],
                                              pooled ? ga->head.scratch[0] : NULL, NULL, ctx->hid, ctx->plan.ws_bytes));
    OP(VIT_OP_HEAD, vh_launch_gallery_topk(s, (const float *)ga->head.scratch[0], n, c->embed_dim, ga->spec.d_rows, ga->spec.dtype,
                                           ga->spec.n_rows, ga->spec.row_stride, ga->spec.k, 0, ga->head.scratch[1], ga->out.indices,
                                           ga->out.scores));
    return 0;
fail:
    return rc;
}

/* The armed dense request behind its layer: the token rows (normalised by the feature readout into the MLP buffer, idle
 * behind fc2, or into the request's scratch; without final_norm the residual stream's patch rows in place), the patch
 * logits, the labels, and the soft maps when the request was armed with them; timed with the classifier */
static int dense_tap(vit_hip_ctx *ctx, vh_stream_t s, const struct dense_req *de, int n)
{
    int rc = 0;
    const vit_config *c = &ctx->cfg;
    float **tw = ctx->w + 4 + 12 * c->depth;
    const int E = c->embed_dim, T = ctx->plan.tokens, P = T - 1;
    const float *rows = ctx->x + E;
    long image_stride = (long)T * E;
    if (de->spec.final_norm) {
        float *tok = de->head.scratch[1] ? (float *)de->head.scratch[1] : ctx->hid;
        OP(VIT_OP_HEAD, vh_launch_feature_readout(s, ctx->x, NULL, E, tw[0], tw[1], c->eps, 1, 0, VIT_FEATURE_F32, VIT_TOKENS_NLC, n, T, E,
                                                  0, 1, NULL, NULL, tok, NULL, 0));
        rows = tok;
        image_stride = (long)P * E;
    }
    float *pl = de->out.patch_logits ? de->out.patch_logits : (float *)de->head.scratch[0];
    OP(VIT_OP_HEAD, vh_launch_dense_logits(s, rows, image_stride, E, n, P, E, de->spec.d_weight, de->spec.weight_stride, de->spec.d_bias,
                                           de->spec.n_labels, pl));
    const vit_dense_soft_buffers *so = &de->soft_out;
    const int soft = so->prob || so->expect || so->entropy;   /* vit_hip_set_dense_soft; labels then are optional */
    if (de->out.labels || !soft)
        OP(VIT_OP_HEAD, vh_launch_dense_labels(s, pl, n, de->grid_h, de->grid_w, de->spec.n_labels, de->out_h, de->out_w, de->out.labels,
                                               de->out.scores));
    if (soft)
        OP(VIT_OP_HEAD, vh_launch_dense_soft(s, pl, n, de->grid_h, de->grid_w, de->spec.n_labels, de->out_h, de->out_w, de->soft.logit_scale,
                                             de->soft.d_values, so->prob, so->expect, so->entropy));
    return 0;
fail:
    return rc;
}

/* Everything after the argument checks of the forwards.  sv: the armed requests to serve; NULL: none */
static int forward_device(vit_hip_ctx *ctx, const struct ingest_src *src, int n, float *d_logits, float *d_probs, vh_stream_t stream,
                          const struct serving *sv)
{
    static const struct serving none;
    int rc = 0;
    sv = sv ? sv : &none;
    const struct feature_req *fr = sv->fr;
    const struct topk_req *tk = sv->tk;
    const struct rollout_req *ro = sv->ro;
    const struct gallery_req *ga = sv->ga;
    const struct dense_req *de = sv->de;
    ctx->serving = sv;   /* read by the layer functions (attention_tap) */
    TRY(vh_set_device(ctx->device));   /* the current device is per host thread */
    const vit_config *c = &ctx->cfg;
    const int E = c->embed_dim, T = ctx->plan.tokens, NC = c->num_classes;
    vh_stream_t s = stream ? stream : ctx->stream;

    struct ingest_src crops;
    if (src->kind == INGEST_U8_RESIZED || src->kind == INGEST_U8_BOXES) {   /* crops into Q|K|V, then the u8 path on them; both count as the patch embedding */
        unsigned char *out = (unsigned char *)ctx->qkv + ctx->plan.crop_off;
        OP(VIT_OP_PATCH_EMBED, resize_crop_launch(ctx, s, src, n, out));
        crops = (struct ingest_src){.kind = INGEST_U8, .on_device = 1, .u8 = out, .layout = VIT_PIXELS_HWC, .norm = src->norm};
        src = &crops;
    }
    OP(VIT_OP_PATCH_EMBED, patch_embed_launches(ctx, s, src, n));
    int cls_rows = 0;   /* the last layer ran behind its attention on the class-token rows only (fp32 path on planes) */
    /* a request for patch rows of the last layer makes this forward run the last layer on all rows */
    const int cls_only = (ctx->plan.last_layer_lazy || ctx->plan.cls_only_last) && ctx->plan.cls_only_ok &&
                         !serving_needs_last_layer_rows(sv, c->depth);
    ctx->last_pending = ctx->last_pending_attention = 0;   /* this forward overwrites what a pending last layer would read */
    for (int l = 0, k = 0; l < c->depth; ++l) {
        switch (ctx->plan.precision) {
        case VIT_PRECISION_FP8_GEMM: TRY(layer_fp8(ctx, s, n, l)); break;
        case VIT_PRECISION_BF16_GEMM: TRY(layer_bf16(ctx, s, n, l)); break;
        case VIT_PRECISION_F32_FP16X2: TRY(layer_fp16x2(ctx, s, n, l)); break;
        default:
            if (ctx->plan.use_p3)
                TRY(layer_f32_planes(ctx, s, n, l, cls_only, &cls_rows));
            else
                TRY(layer_f32_rows(ctx, s, n, l));
        }
        if (fr && k < fr->spec.n_taps && fr->layer[k] == l)
            TRY(feature_tap(ctx, s, fr, k++, n, cls_rows));
        if (ga && ga->layer == l)
            TRY(gallery_tap(ctx, s, ga, n, cls_rows));
        if (de && de->layer == l)
            TRY(dense_tap(ctx, s, de, n));
    }
    if (ro)   /* the class token's row of the last product */
        OP(VIT_OP_ATTENTION, vh_launch_rollout_read(s, (const float *)ro->head.scratch[(c->depth - 1 - ro->first) & 1], n, T, ro->out.rollout));

    /* final LayerNorm on the class-token rows -- row i * stride of the residual stream, or compacted at the start of the
     * Q|K|V buffer -- classifier, softmax (ViT_seq.c:506-515) */
    float **tw = ctx->w + 4 + 12 * c->depth;
    float *logits = d_logits ? d_logits : ctx->d_logits;
    const float *final_x = cls_rows ? (const float *)ctx->qkv : ctx->x;
    const long final_stride = cls_rows ? (long)E : (long)T * E;
    OP(VIT_OP_LAYER_NORM, vh_launch_layer_norm(s, final_x, tw[0], tw[1], ctx->cls, n, E, final_stride, E, c->eps));
    /* ragged class counts (1000) run on the fp32 matrix instruction either way; a multiple of 128 follows the plan */
    OP(VIT_OP_HEAD, vh_launch_linear_math(s, logits, tw[2], ctx->cls, tw[3], n, E, NC, 0, NULL, fp32_math(ctx)));
    if (d_probs)
        OP(VIT_OP_SOFTMAX, vh_launch_softmax(s, logits, d_probs, n, NC));
    if (tk)   /* the k best of every row of the fp32 logits: one launch, whatever the precision mode */
        OP(VIT_OP_SOFTMAX, vh_launch_topk(s, logits, n, NC, tk->spec.k, tk->spec.score_kind, tk->out.labels, tk->out.scores));
    if (cls_rows) {
        ctx->last_pending = n;
        ctx->last_pending_attention = cls_rows == 2;
    }
fail:
    ctx->serving = NULL;
    return rc;
}

/* What the ingest path needs of a context; a staging slot of images holds max_batch fp32 images */
static struct ingest_model model_of(const vit_hip_ctx *ctx)
{
    const vit_config *c = &ctx->cfg;
    return (struct ingest_model){.max_batch = ctx->max_batch, .in_chans = c->in_chans, .img_size = c->img_size, .img_width = c->img_width,
                                 .slot_bytes = (size_t)ctx->max_batch * c->in_chans * c->img_size * ctx_width(ctx) * sizeof(float)};
}

/* The argument checks of an 8-bit form (ingest_check); a NULL context is refused there, not read here */
static int source_check(const char *who, const vit_hip_ctx *ctx, const struct ingest_src *src, int n)
{
    const struct ingest_model model = ctx ? model_of(ctx) : (struct ingest_model){0};
    return ingest_check(who, ctx ? &model : NULL, src, n);
}

/* A public device-form forward: the argument checks of the 8-bit kinds (fp32 callers have made their own), then the armed
 * requests */
static int forward_device_armed(vit_hip_ctx *ctx, const char *who, const struct ingest_src *src, int n, float *d_logits, float *d_probs,
                                vh_stream_t stream)
{
    struct serving sv;
    if ((src->kind != INGEST_F32 && source_check(who, ctx, src, n)) || requests_serving(&ctx->req, who, FEAT_DEVICE, &sv))
        return 1;
    return forward_device(ctx, src, n, d_logits, d_probs, stream, &sv);
}

/* vit_hip_forward_device with no feature output whatever is armed (vit_gather_rccl.c) */
int vit_hip_forward_device_plain(vit_hip_ctx *ctx, const float *d_images, int n, float *d_logits, float *d_probs, vh_stream_t stream)
{
    if (!ctx || !d_images || n <= 0 || n > ctx->max_batch)
        return 1;
    const struct ingest_src src = {.kind = INGEST_F32, .on_device = 1, .f32 = d_images};
    return forward_device(ctx, &src, n, d_logits, d_probs, stream, NULL);
}

int vit_hip_forward_device(vit_hip_ctx *ctx, const float *d_images, int n, float *d_logits,
                           float *d_probs, vh_stream_t stream)
{
    if (!ctx || !d_images || n <= 0 || n > ctx->max_batch)
        return 1;
    const struct ingest_src src = {.kind = INGEST_F32, .on_device = 1, .f32 = d_images};
    return forward_device_armed(ctx, "vit_hip_forward_device", &src, n, d_logits, d_probs, stream);
}

/* A public call for the crops alone, into src->crops */
static int crops_launch(vit_hip_ctx *ctx, const char *who, const struct ingest_src *src, int n, vh_stream_t stream)
{
    int rc = 0;
    if (source_check(who, ctx, src, n))
        return 1;
    if ((rc = vh_set_device(ctx->device)) != 0)
        return rc;
    return resize_crop_launch(ctx, stream ? stream : ctx->stream, src, n, src->crops);
}

int vit_hip_forward_device_u8(vit_hip_ctx *ctx, const unsigned char *d_images, int n, int layout,
                              const vit_pixel_norm *norm, float *d_logits, float *d_probs, vh_stream_t stream)
{
    const struct ingest_src src = {.kind = INGEST_U8, .on_device = 1, .u8 = d_images, .layout = layout, .norm = norm};
    return forward_device_armed(ctx, "vit_hip_forward_device_u8", &src, n, d_logits, d_probs, stream);
}

int vit_hip_resize_crop_u8(vit_hip_ctx *ctx, const vit_image_u8 *d_images, int n, int layout, const vit_resize_crop *rc,
                           unsigned char *d_out, vh_stream_t stream)
{
    const struct ingest_src src = {.kind = INGEST_U8_RESIZED, .on_device = 1, .images = d_images, .rc = rc, .layout = layout,
                                   .crops_only = 1, .crops = d_out};
    return crops_launch(ctx, "vit_hip_resize_crop_u8", &src, n, stream);
}

int vit_hip_forward_device_u8_resized(vit_hip_ctx *ctx, const vit_image_u8 *d_images, int n, int layout, const vit_resize_crop *rc,
                                      const vit_pixel_norm *norm, float *d_logits, float *d_probs, vh_stream_t stream)
{
    const struct ingest_src src = {.kind = INGEST_U8_RESIZED, .on_device = 1, .images = d_images, .rc = rc, .layout = layout, .norm = norm};
    return forward_device_armed(ctx, "vit_hip_forward_device_u8_resized", &src, n, d_logits, d_probs, stream);
}

/* boxes: regions of 8-bit images, each resized to img x img as Pillow's Image.resize(size, resample, box=) */
int vit_hip_crop_boxes_u8(vit_hip_ctx *ctx, const vit_image_u8 *d_images, int n_images, const vit_box_u8 *boxes, int n, int layout,
                          int filter, unsigned char *d_out, vh_stream_t stream)
{
    const struct ingest_src src = {.kind = INGEST_U8_BOXES, .on_device = 1, .images = d_images, .n_images = n_images, .boxes = boxes,
                                   .filter = filter, .layout = layout, .crops_only = 1, .crops = d_out};
    return crops_launch(ctx, "vit_hip_crop_boxes_u8", &src, n, stream);
}

int vit_hip_forward_device_u8_boxes(vit_hip_ctx *ctx, const vit_image_u8 *d_images, int n_images, const vit_box_u8 *boxes, int n,
                                    int layout, int filter, const vit_pixel_norm *norm, float *d_logits, float *d_probs,
                                    vh_stream_t stream)
{
    const struct ingest_src src = {.kind = INGEST_U8_BOXES, .on_device = 1, .images = d_images, .n_images = n_images, .boxes = boxes,
                                   .filter = filter, .layout = layout, .norm = norm};
    return forward_device_armed(ctx, "vit_hip_forward_device_u8_boxes", &src, n, d_logits, d_probs, stream);
}

/* The public setters, both forms of each: requests_set_* on the context's requests and on what arming reads of the context */
#define SETTER(name, kind, spec_t, bufs_t, host)                                                                                 \
    int name(vit_hip_ctx *ctx, const spec_t *spec, const bufs_t *bufs)                                                           \
    {                                                                                                                            \
        if (!ctx)                                                                                                                \
            return ingest_refuse(#name, "NULL context");                                                                         \
        const struct request_model m = {.device = ctx->device, .max_batch = ctx->max_batch, .stream = ctx->stream, .cfg = &ctx->cfg, \
                                        .tokens = ctx->plan.tokens, .qkv_form = ctx->plan.qkv_form, .ws_bytes = ctx->plan.ws_bytes}; \
        return requests_set_##kind(#name, &m, &ctx->req, spec, bufs, host);                                                      \
    }
SETTER(vit_hip_set_features, features, vit_feature_spec, vit_feature_buffers, 0)
SETTER(vit_hip_set_features_host, features, vit_feature_spec, vit_feature_buffers, 1)
SETTER(vit_hip_set_topk, topk, vit_topk_spec, vit_topk_buffers, 0)
SETTER(vit_hip_set_topk_host, topk, vit_topk_spec, vit_topk_buffers, 1)
SETTER(vit_hip_set_attention, attention, vit_attn_spec, vit_attn_buffers, 0)
SETTER(vit_hip_set_attention_host, attention, vit_attn_spec, vit_attn_buffers, 1)
SETTER(vit_hip_set_rollout, rollout, vit_rollout_spec, vit_rollout_buffers, 0)
SETTER(vit_hip_set_rollout_host, rollout, vit_rollout_spec, vit_rollout_buffers, 1)
SETTER(vit_hip_set_gallery, gallery, vit_gallery_spec, vit_gallery_buffers, 0)
SETTER(vit_hip_set_gallery_host, gallery, vit_gallery_spec, vit_gallery_buffers, 1)
SETTER(vit_hip_set_dense, dense, vit_dense_spec, vit_dense_buffers, 0)
SETTER(vit_hip_set_dense_host, dense, vit_dense_spec, vit_dense_buffers, 1)
#undef SETTER

/* the dense request in device form with the soft maps attached (include/ViT_opencl.h) */
int vit_hip_set_dense_soft(vit_hip_ctx *ctx, const vit_dense_spec *spec, const vit_dense_soft_spec *soft, const vit_dense_buffers *d_bufs,
                           const vit_dense_soft_buffers *d_soft)
{
    static const char who[] = "vit_hip_set_dense_soft";
    if (!ctx)
        return ingest_refuse(who, "NULL context");
    const struct request_model m = {.device = ctx->device, .max_batch = ctx->max_batch, .stream = ctx->stream, .cfg = &ctx->cfg,
                                    .tokens = ctx->plan.tokens, .qkv_form = ctx->plan.qkv_form, .ws_bytes = ctx->plan.ws_bytes};
    return requests_set_dense_soft(who, &m, &ctx->req, spec, soft, d_bufs, d_soft);
}

/* ---- whole frames (include/ViT_opencl.h): windows through the box forward with a dense request of the call's own, their
 * patch logits blended per frame pixel by vh_launch_dense_stitch.  Public pieces composed; nothing of a forward changes ---- */

/* spec's head as the call arms it: one label per window, which nobody reads */
static vit_dense_spec frame_head(const vit_frame_spec *spec)
{
    vit_dense_spec head = spec->head;
    head.out_h = head.out_w = 1;
    return head;
}

/* What needs no context: spec, frame size and window count against cfg; P and C of the patch logits */
static int frame_spec_check(const char *who, const vit_config *cfg, const vit_frame_spec *spec, int frame_h, int frame_w, int n_windows,
                            size_t *patch_elems)
{
    if (!cfg || !spec)
        return ingest_refuse(who, "NULL argument");
    if (cfg->img_width != 0 && cfg->img_width != cfg->img_size)
        return ingest_refuse(who, "the context's input is non-square: the box forms make square crops");
    if (spec->head.out_h != 0 || spec->head.out_w != 0)
        return ingest_refuse(who, "head.out_h and head.out_w must be 0: the output is the frame");
    if (spec->fill_label < 0 || spec->fill_label > 255)
        return ingest_refuse(who, "fill_label must be in 0..255");
    if (frame_h < 1 || frame_w < 1 || frame_h > VH_STITCH_MAX_SIDE || frame_w > VH_STITCH_MAX_SIDE)
        return ingest_refuse(who, "the frame's height and width must be in 1..16384");
    const vit_dense_spec head = frame_head(spec);
    if (vit_dense_sizes(cfg, &head, NULL, NULL, patch_elems, NULL))
        return 1;
    if (n_windows < 1 || (size_t)n_windows * (*patch_elems / (size_t)head.n_labels) >= 2147483647u - 128u)
        return ingest_refuse(who, "n_windows must be positive, n_windows * (T - 1) below 2^31 - 128");
    return 0;
}

int vit_frame_sizes(const vit_config *cfg, const vit_frame_spec *spec, int frame_h, int frame_w, int n_windows, size_t *labels_bytes,
                    size_t *scratch_bytes)
{
    size_t patch_elems = 0;
    if (frame_spec_check("vit_frame_sizes", cfg, spec, frame_h, frame_w, n_windows, &patch_elems))
        return 1;
    if (labels_bytes)
        *labels_bytes = (size_t)frame_h * frame_w;
    if (scratch_bytes)   /* all windows' patch logits, the boxes and the offsets; not the ids (4 bytes each) nor one chunk's patch
                          * logits, which depend on the boxes and on max_batch */
        *scratch_bytes = align_up((size_t)n_windows * patch_elems * sizeof(float), 16) + kl_dense_stitch_scratch(n_windows, frame_h, frame_w, 0);
    return 0;
}

/* the soft side of a frame call: a NULL pointer to it for the labels calls, which then need their labels buffer */
struct frame_soft {
    const vit_dense_soft_spec *soft;
    const vit_dense_soft_buffers *maps;
};

/* Everything both forms refuse, before anything is queued or allocated; *patch_elems: a window's patch logits, (T - 1) * n_labels */
static int frame_check(const char *who, vit_hip_ctx *ctx, const vit_image_u8 *frame, const vit_box_u8 *windows, int n_windows, int layout,
                       int filter, const vit_pixel_norm *norm, const vit_frame_spec *spec, const vit_frame_buffers *out,
                       const struct frame_soft *fs, int on_device, size_t *patch_elems)
{
    static const vit_frame_buffers no_out;
    if (fs && !out)
        out = &no_out;
    if (!ctx || !frame || !windows || !norm || !spec || !out || !frame->data)
        return ingest_refuse(who, "NULL argument");
    if (frame_spec_check(who, &ctx->cfg, spec, frame->height, frame->width, n_windows, patch_elems))
        return 1;
    if (ctx->req.dense.head.form != FEAT_NONE)
        return ingest_refuse(who, "a dense request is armed (vit_hip_set_dense / _host): the call arms its own; disarm it first");
    struct serving sv;
    if (requests_serving(&ctx->req, who, FEAT_DEVICE, &sv))   /* a request armed in host form: the call forwards in device form */
        return 1;
    if (!spec->head.d_weight || (((uintptr_t)spec->head.d_weight | (uintptr_t)spec->head.d_bias) & 15))
        return ingest_refuse(who, "the head's weight must be given, weight and bias 16-byte aligned");
    if (fs) {
        const char *why = requests_dense_soft_why(fs->soft, fs->maps, on_device);
        if (why)
            return ingest_refuse(who, why);
        if (!out->labels && (out->scores || out->cover))
            return ingest_refuse(who, "scores and cover need a labels buffer");
    } else if (!out->labels)
        return ingest_refuse(who, "no labels buffer");
    if (on_device && (((uintptr_t)out->labels | (uintptr_t)out->scores | (uintptr_t)out->cover) & 15))
        return ingest_refuse(who, "device output buffers must be 16-byte aligned");
    for (int i = 0; i < n_windows; ++i) {
        char why[120];
        if (windows[i].image != 0)
            return ingest_refuse(who, "every window's image must be 0: a call takes one frame");
        if (vit_box_check(frame->height, frame->width, windows[i].box)) {   /* vit_stitch_check's rule, window by window */
            snprintf(why, sizeof why, "window %d is not a box of the frame (finite, inside it, at least 1 px each way)", i);
            return ingest_refuse(who, why);
        }
    }
    /* the frame, layout, filter and channels as the box forward will check them, chunk by chunk */
    for (int first = 0; first < n_windows; first += ctx->max_batch) {
        const int m = n_windows - first < ctx->max_batch ? n_windows - first : ctx->max_batch;
        const struct ingest_src src = {.kind = INGEST_U8_BOXES, .on_device = 1, .images = frame, .n_images = 1, .boxes = windows + first,
                                       .filter = filter, .layout = layout, .norm = norm};
        if (source_check(who, ctx, &src, m))
            return 1;
    }
    return 0;
}

/* The device form behind its checks.  fs NULL: the labels calls.  Otherwise the soft calls: the label stitch only where labels
 * are asked for, then the soft stitch, each with an index of its own in device memory (the stitch launchers' rule: one scratch
 * per launch in flight -- the second launcher's synchronous copies must not run over the queued kernel's index), both timed
 * under VIT_OP_HEAD */
static int frame_run(const char *who, vit_hip_ctx *ctx, const vit_image_u8 *d_frame, const vit_box_u8 *windows, int n_windows, int layout,
                     int filter, const vit_pixel_norm *norm, const vit_frame_spec *spec, const vit_frame_buffers *d_out,
                     const struct frame_soft *fs, size_t patch_elems)
{
    int rc = 0, armed = 0;
    const vh_stream_t s = ctx->stream;
    const int want_labels = d_out && d_out->labels;
    const int H = d_frame->height, W = d_frame->width, mb = ctx->max_batch;
    const int C = spec->head.n_labels;
    int grid_h, grid_w;
    vit_config_grid(&ctx->cfg, &grid_h, &grid_w);
    float *boxes4 = malloc((size_t)n_windows * 4 * sizeof(float));
    int *offsets = NULL, *ids = NULL;
    void *d_all = NULL, *d_chunk = NULL, *d_lab = NULL, *d_index = NULL, *d_index_soft = NULL;
    if (!boxes4) {
        rc = ingest_refuse(who, "out of host memory");
        goto fail;
    }
    for (int i = 0; i < n_windows; ++i)
        memcpy(boxes4 + 4 * (size_t)i, windows[i].box, 4 * sizeof(float));
    const long blocks = (long)((H + VH_STITCH_BLOCK - 1) / VH_STITCH_BLOCK) * ((W + VH_STITCH_BLOCK - 1) / VH_STITCH_BLOCK);
    const long n_ids = vit_stitch_index(H, W, VH_STITCH_BLOCK, boxes4, n_windows, NULL, NULL, 0);
    if (n_ids < 0) {
        rc = 1;
        goto fail;
    }
    offsets = malloc((size_t)(blocks + 1) * sizeof(int));
    ids = malloc((size_t)(n_ids > 0 ? n_ids : 1) * sizeof(int));
    if (!offsets || !ids) {
        rc = ingest_refuse(who, "out of host memory");
        goto fail;
    }
    if (vit_stitch_index(H, W, VH_STITCH_BLOCK, boxes4, n_windows, offsets, ids, n_ids) != n_ids) {
        rc = 1;
        goto fail;
    }
    const size_t index_bytes = kl_dense_stitch_scratch(n_windows, H, W, n_ids);
    TRY(vh_set_device(ctx->device));
    if (vh_malloc(&d_all, align_up((size_t)n_windows * patch_elems * sizeof(float), 16)) || vh_malloc(&d_chunk, align_up((size_t)mb * patch_elems * sizeof(float), 16)) ||
        vh_malloc(&d_lab, align_up((size_t)mb, 16)) || (want_labels && vh_malloc(&d_index, index_bytes)) ||
        (fs && vh_malloc(&d_index_soft, index_bytes))) {
        rc = ingest_refuse(who, "the scratch of the call (patch logits of all windows, block index) cannot be allocated");
        goto fail;
    }
    const vit_dense_spec head = frame_head(spec);
    const vit_dense_buffers bufs = {.labels = d_lab, .scores = NULL, .patch_logits = d_chunk};
    TRY(vit_hip_set_dense(ctx, &head, &bufs));
    armed = 1;
    for (int first = 0; first < n_windows; first += mb) {
        const int m = n_windows - first < mb ? n_windows - first : mb;
        TRY(vit_hip_forward_device_u8_boxes(ctx, d_frame, 1, windows + first, m, layout, filter, norm, NULL, NULL, 0));
        TRY(vh_d2d((float *)d_all + (size_t)first * patch_elems, d_chunk, (size_t)m * patch_elems * sizeof(float), ctx->stream));
    }
    armed = 0;
    TRY(vit_hip_set_dense(ctx, NULL, NULL));
    if (want_labels)
        OP_T(fs != NULL, VIT_OP_HEAD, vh_launch_dense_stitch(s, d_all, n_windows, grid_h, grid_w, C, boxes4, H, W, offsets, ids, spec->fill_label,
                                                             d_index, index_bytes, d_out->labels, d_out->scores, d_out->cover));
    if (fs)
        OP(VIT_OP_HEAD, vh_launch_dense_stitch_soft(s, d_all, n_windows, grid_h, grid_w, C, boxes4, H, W, offsets, ids, d_index_soft, index_bytes,
                                                    fs->soft->logit_scale, fs->soft->d_values, fs->maps->prob, fs->maps->expect,
                                                    fs->maps->entropy));
    TRY(vh_stream_sync(ctx->stream));
fail:
    if (armed) {   /* keep the failure's message over the disarming's */
        char kept[512];
        snprintf(kept, sizeof kept, "%s", vh_last_error());
        vit_hip_set_dense(ctx, NULL, NULL);
        vh_set_error(rc, kept);
    }
    if (d_all || d_chunk || d_lab || d_index || d_index_soft) {
        if (rc)
            vh_stream_sync(ctx->stream);
        void *dev[] = {d_all, d_chunk, d_lab, d_index, d_index_soft};
        for (size_t i = 0; i < sizeof(dev) / sizeof(dev[0]); ++i)
            if (dev[i])
                vh_free(dev[i]);
    }
    free(boxes4);
    free(offsets);
    free(ids);
    return rc;
}

int vit_hip_segment_frame_device_u8(vit_hip_ctx *ctx, const vit_image_u8 *d_frame, const vit_box_u8 *windows, int n_windows, int layout,
                                    int filter, const vit_pixel_norm *norm, const vit_frame_spec *spec, const vit_frame_buffers *d_out)
{
    static const char who[] = "vit_hip_segment_frame_device_u8";
    size_t patch_elems = 0;
    if (frame_check(who, ctx, d_frame, windows, n_windows, layout, filter, norm, spec, d_out, NULL, 1, &patch_elems))
        return 1;
    return frame_run(who, ctx, d_frame, windows, n_windows, layout, filter, norm, spec, d_out, NULL, patch_elems);
}

int vit_hip_segment_frame_u8(vit_hip_ctx *ctx, const vit_image_u8 *frame, const vit_box_u8 *windows, int n_windows, int layout, int filter,
                             const vit_pixel_norm *norm, const vit_frame_spec *spec, const vit_frame_buffers *h_out)
{
    static const char who[] = "vit_hip_segment_frame_u8";
    int rc = 0;
    size_t patch_elems = 0;
    if (frame_check(who, ctx, frame, windows, n_windows, layout, filter, norm, spec, h_out, NULL, 0, &patch_elems))
        return 1;
    /* what the caller's image owns: rows of `row` bytes, row_stride apart -- the last row of the last plane ends with its pixels,
     * not with its stride (a column band of a larger array), so that is where the upload ends */
    const size_t planes = layout == VIT_PIXELS_HWC ? 1 : (size_t)ctx->cfg.in_chans;
    const size_t row = (size_t)frame->width * (layout == VIT_PIXELS_HWC ? (size_t)ctx->cfg.in_chans : 1);
    const size_t frame_bytes = (planes * (size_t)frame->height - 1) * (size_t)frame->row_stride + row;
    const size_t px = (size_t)frame->height * frame->width;
    void *d_data = NULL, *d_lab = NULL, *d_sc = NULL, *d_cov = NULL;
    TRY(vh_set_device(ctx->device));
    if (vh_malloc(&d_data, align_up(frame_bytes, 16)) || vh_malloc(&d_lab, align_up(px, 16)) ||
        (h_out->scores && vh_malloc(&d_sc, px * sizeof(float))) || (h_out->cover && vh_malloc(&d_cov, align_up(px, 16)))) {
        rc = ingest_refuse(who, "the frame and its outputs cannot be allocated on the device");
        goto fail;
    }
    TRY(vh_h2d(d_data, frame->data, frame_bytes, ctx->stream));
    const vit_image_u8 d_frame = {.data = d_data, .height = frame->height, .width = frame->width, .row_stride = frame->row_stride};
    const vit_frame_buffers d_out = {.labels = d_lab, .scores = d_sc, .cover = d_cov};
    TRY(frame_run(who, ctx, &d_frame, windows, n_windows, layout, filter, norm, spec, &d_out, NULL, patch_elems));
    TRY(vh_d2h(h_out->labels, d_lab, px, ctx->stream));
    if (d_sc)
        TRY(vh_d2h(h_out->scores, d_sc, px * sizeof(float), ctx->stream));
    if (d_cov)
        TRY(vh_d2h(h_out->cover, d_cov, px, ctx->stream));
fail:
    vh_stream_sync(ctx->stream);
    void *dev[] = {d_data, d_lab, d_sc, d_cov};
    for (size_t i = 0; i < sizeof(dev) / sizeof(dev[0]); ++i)
        if (dev[i])
            vh_free(dev[i]);
    return rc;
}

/* ---- whole frames, soft maps (include/ViT_opencl.h): frame_run with the soft stitch behind the windows ---- */

int vit_frame_soft_check(const vit_config *cfg, const vit_frame_spec *spec, const vit_dense_soft_spec *soft, int frame_h, int frame_w,
                         int n_windows, size_t *map_elems)
{
    static const char who[] = "vit_frame_soft_check";
    size_t patch_elems = 0;
    if (frame_spec_check(who, cfg, spec, frame_h, frame_w, n_windows, &patch_elems))
        return 1;
    float *const some = (float *)(uintptr_t)16;   /* the rules about soft alone: maps that fit it */
    const vit_dense_soft_buffers with = {.prob = some, .expect = soft && soft->d_values ? some : NULL};
    const char *why = requests_dense_soft_why(soft, &with, 0);
    if (why)
        return ingest_refuse(who, why);
    if (map_elems)
        *map_elems = (size_t)frame_h * frame_w;
    return 0;
}

int vit_hip_segment_frame_soft_device_u8(vit_hip_ctx *ctx, const vit_image_u8 *d_frame, const vit_box_u8 *windows, int n_windows, int layout,
                                         int filter, const vit_pixel_norm *norm, const vit_frame_spec *spec, const vit_dense_soft_spec *soft,
                                         const vit_frame_buffers *d_out, const vit_dense_soft_buffers *d_soft)
{
    static const char who[] = "vit_hip_segment_frame_soft_device_u8";
    const struct frame_soft fs = {.soft = soft, .maps = d_soft};
    size_t patch_elems = 0;
    if (frame_check(who, ctx, d_frame, windows, n_windows, layout, filter, norm, spec, d_out, &fs, 1, &patch_elems))
        return 1;
    return frame_run(who, ctx, d_frame, windows, n_windows, layout, filter, norm, spec, d_out, &fs, patch_elems);
}

int vit_hip_segment_frame_soft_u8(vit_hip_ctx *ctx, const vit_image_u8 *frame, const vit_box_u8 *windows, int n_windows, int layout,
                                  int filter, const vit_pixel_norm *norm, const vit_frame_spec *spec, const vit_dense_soft_spec *soft,
                                  const vit_frame_buffers *h_out, const vit_dense_soft_buffers *h_soft)
{
    static const char who[] = "vit_hip_segment_frame_soft_u8";
    static const vit_frame_buffers no_out;
    int rc = 0;
    size_t patch_elems = 0;
    const struct frame_soft h_fs = {.soft = soft, .maps = h_soft};
    if (frame_check(who, ctx, frame, windows, n_windows, layout, filter, norm, spec, h_out, &h_fs, 0, &patch_elems))
        return 1;
    if (!h_out)
        h_out = &no_out;
    /* the upload ends with the last row's pixels (vit_hip_segment_frame_u8) */
    const size_t planes = layout == VIT_PIXELS_HWC ? 1 : (size_t)ctx->cfg.in_chans;
    const size_t row = (size_t)frame->width * (layout == VIT_PIXELS_HWC ? (size_t)ctx->cfg.in_chans : 1);
    const size_t frame_bytes = (planes * (size_t)frame->height - 1) * (size_t)frame->row_stride + row;
    const size_t px = (size_t)frame->height * frame->width;
    void *d_data = NULL, *d_lab = NULL, *d_sc = NULL, *d_cov = NULL, *d_map[3] = {NULL, NULL, NULL};
    float *const h_map[3] = {h_soft->prob, h_soft->expect, h_soft->entropy};
    TRY(vh_set_device(ctx->device));
    if (vh_malloc(&d_data, align_up(frame_bytes, 16)) || (h_out->labels && vh_malloc(&d_lab, align_up(px, 16))) ||
        (h_out->scores && vh_malloc(&d_sc, px * sizeof(float))) || (h_out->cover && vh_malloc(&d_cov, align_up(px, 16))) ||
        (h_map[0] && vh_malloc(&d_map[0], px * sizeof(float))) || (h_map[1] && vh_malloc(&d_map[1], px * sizeof(float))) ||
        (h_map[2] && vh_malloc(&d_map[2], px * sizeof(float)))) {
        rc = ingest_refuse(who, "the frame and its outputs cannot be allocated on the device");
        goto fail;
    }
    TRY(vh_h2d(d_data, frame->data, frame_bytes, ctx->stream));
    const vit_image_u8 d_frame = {.data = d_data, .height = frame->height, .width = frame->width, .row_stride = frame->row_stride};
    const vit_frame_buffers d_out = {.labels = d_lab, .scores = d_sc, .cover = d_cov};
    const vit_dense_soft_buffers d_soft = {.prob = d_map[0], .expect = d_map[1], .entropy = d_map[2]};
    const struct frame_soft d_fs = {.soft = soft, .maps = &d_soft};
    TRY(frame_run(who, ctx, &d_frame, windows, n_windows, layout, filter, norm, spec, &d_out, &d_fs, patch_elems));
    if (d_lab)
        TRY(vh_d2h(h_out->labels, d_lab, px, ctx->stream));
    if (d_sc)
        TRY(vh_d2h(h_out->scores, d_sc, px * sizeof(float), ctx->stream));
    if (d_cov)
        TRY(vh_d2h(h_out->cover, d_cov, px, ctx->stream));
    for (int k = 0; k < 3; ++k)
        if (d_map[k])
            TRY(vh_d2h(h_map[k], d_map[k], px * sizeof(float), ctx->stream));
fail:
    vh_stream_sync(ctx->stream);
    void *dev[] = {d_data, d_lab, d_sc, d_cov, d_map[0], d_map[1], d_map[2]};
    for (size_t i = 0; i < sizeof(dev) / sizeof(dev[0]); ++i)
        if (dev[i])
            vh_free(dev[i]);
    return rc;
}

/* images whose last layer is pending behind the last forward (finish_last_layer); tests */
int vit_hip_last_layer_pending(const vit_hip_ctx *ctx) { return ctx ? ctx->last_pending : -1; }

int vit_hip_set_last_layer_cls_only(vit_hip_ctx *ctx, int on)
{
    if (!ctx)
        return -1;
    const int before = ctx->plan.cls_only_last;
    ctx->plan.cls_only_last = on && ctx->plan.use_p3 && !ctx->plan.ln_fold;   /* a forward takes it where plan.cls_only_ok */
    return before;
}

/* Debug/test hook: copy the residual stream ([n*tokens][E], un-normalised) to the host, behind the last layer on all rows
 * of the last forward's images (finish_last_layer; a second read runs nothing).  The supported interface to the encoder's
 * output is vit_hip_set_features. */
int vit_hip_read_tokens(vit_hip_ctx *ctx, int n, float *host_out)
{
    int rc = vh_set_device(ctx->device);
    if (rc)
        return rc;
    if ((rc = finish_last_layer(ctx)) != 0)
        return rc;
    rc = vh_d2h(host_out, ctx->x, (size_t)n * ctx->plan.tokens * ctx->cfg.embed_dim * sizeof(float),
                    ctx->stream);
    return rc ? rc : vh_stream_sync(ctx->stream);
}

int vit_hip_profile_enable(vit_hip_ctx *ctx, int max_forwards)
{
    int rc = 0;
    if (!ctx)
        return 1;
    TRY(vh_set_device(ctx->device));
    TRY(vh_stream_sync(ctx->stream));
    prof_release(ctx);
    if (max_forwards <= 0)
        return 0;
    /* + the readouts of an armed feature request + top-k + attention maps + the rollout's steps and read + the gallery's
     * readout and search + the dense head's readout, logits, labels and soft maps */
    const int per_forward = 1 + 7 * ctx->cfg.depth + 3 + 4 + 1 + 4 + ctx->cfg.depth + 1 + 2 + 4;
    ctx->prof_cap = per_forward * max_forwards;
    ctx->prof_ev = (vh_event_t *)calloc((size_t)2 * ctx->prof_cap, sizeof(vh_event_t));
    ctx->prof_class = (int *)calloc((size_t)ctx->prof_cap, sizeof(int));
    if (!ctx->prof_ev || !ctx->prof_class) {
        prof_release(ctx);
        return 4;
    }
    for (int i = 0; i < 2 * ctx->prof_cap; ++i)
        TRY(vh_event_create(&ctx->prof_ev[i]));
    return 0;
fail:
    prof_release(ctx);
    return rc;
}

/* Restrict recording to the operator classes in `op_mask` (bit i = vit_op_class i; 0 = all): every
 * recorded launch costs two event packets between kernels, which a timed run may not want. */
int vit_hip_profile_select(vit_hip_ctx *ctx, unsigned op_mask)
{
    if (!ctx)
        return 1;
    ctx->prof_mask = op_mask;
    return 0;
}

int vit_hip_profile_read(vit_hip_ctx *ctx, double ms_sum[VIT_OP_COUNT], long launches[VIT_OP_COUNT])
{
    int rc = 0;
    if (!ctx || !ms_sum || !launches)
        return 1;
    TRY(vh_set_device(ctx->device));
    for (int k = 0; k < VIT_OP_COUNT; ++k) {
        ms_sum[k] = 0.0;
        launches[k] = 0;
    }
    for (int i = 0; i < ctx->prof_used; ++i) {
        float ms = 0.0f;
        TRY(vh_event_sync(ctx->prof_ev[2 * i + 1]));
        TRY(vh_event_elapsed_ms(&ms, ctx->prof_ev[2 * i], ctx->prof_ev[2 * i + 1]));
        ms_sum[ctx->prof_class[i]] += ms;
        launches[ctx->prof_class[i]] += 1;
    }
    ctx->prof_used = 0;
    return 0;
fail:
    return rc;
}

/* The forward of a chunk, as the pipeline calls it (csrc/vit_pipeline.h) */
static int forward_chunk(void *arg, const struct ingest_src *dev, int m, float *d_logits, float *d_probs, const struct serving *sv)
{
    vit_hip_ctx *ctx = (vit_hip_ctx *)arg;
    return forward_device(ctx, dev, m, d_logits, d_probs, ctx->stream, sv);
}

/* Host-pointer forward, pipelined over chunks of max_batch images (pipeline_run).  plan: the scratch of the kinds whose
 * chunks are planned (vit_ingest.h), NULL for images of the model's size.  form: FEAT_HOST to serve the armed host requests,
 * FEAT_NONE to serve none. */
static int forward_pipelined(vit_hip_ctx *ctx, const struct ingest_src *src, struct ingest_plan *plan, int n, float *logits, float **probs,
                             int form)
{
    struct serving sv;
    if (requests_serving(&ctx->req, "forward", form, &sv))
        return 1;
    return pipeline_run(&ctx->pipe, src, plan, n, logits, probs, &sv, forward_chunk, ctx);
}

static int forward_host_images(vit_hip_ctx *ctx, const ImageData *images, int n, float *logits, float **probs, int form)
{
    if (!ctx || !images || n <= 0)
        return 1;
    const vit_config *c = &ctx->cfg;
    for (int i = 0; i < n; ++i)
        if (!images[i].data || images[i].c != c->in_chans || images[i].h != c->img_size ||
            images[i].w != ctx_width(ctx))
            return 5;
    const struct ingest_src src = {.kind = INGEST_F32, .host_f32 = images};
    return forward_pipelined(ctx, &src, NULL, n, logits, probs, form);
}

int vit_hip_forward(vit_hip_ctx *ctx, const ImageData *images, int n, float *logits, float **probs)
{
    return forward_host_images(ctx, images, n, logits, probs, FEAT_HOST);
}

/* vit_hip_forward with no armed output served, whatever is armed (vit_multi.c) */
int vit_hip_forward_plain(vit_hip_ctx *ctx, const ImageData *images, int n, float *logits, float **probs)
{
    return forward_host_images(ctx, images, n, logits, probs, FEAT_NONE);
}

/* A public host-form forward of 8-bit images: the checks, the call's one scratch allocation where chunks are planned */
static int forward_host_u8(vit_hip_ctx *ctx, const char *who, const struct ingest_src *src, int n, float *logits, float **probs)
{
    if (source_check(who, ctx, src, n))
        return 1;
    struct ingest_plan *plan = NULL;
    if (src->kind != INGEST_U8) {
        const struct ingest_model model = model_of(ctx);
        if (!(plan = ingest_plan_new(&model, src->kind)))
            return ingest_refuse(who, "out of host memory");
    }
    const int rc = forward_pipelined(ctx, src, plan, n, logits, probs, FEAT_HOST);
    ingest_plan_free(plan);
    return rc;
}

int vit_hip_forward_u8(vit_hip_ctx *ctx, const unsigned char *images, int n, int layout,
                       const vit_pixel_norm *norm, float *logits, float **probs)
{
    const struct ingest_src src = {.kind = INGEST_U8, .u8 = images, .layout = layout, .norm = norm};
    return forward_host_u8(ctx, "vit_hip_forward_u8", &src, n, logits, probs);
}

int vit_hip_forward_u8_resized(vit_hip_ctx *ctx, const vit_image_u8 *images, int n, int layout, const vit_resize_crop *rc,
                               const vit_pixel_norm *norm, float *logits, float **probs)
{
    const struct ingest_src src = {.kind = INGEST_U8_RESIZED, .images = images, .rc = rc, .layout = layout, .norm = norm};
    return forward_host_u8(ctx, "vit_hip_forward_u8_resized", &src, n, logits, probs);
}

int vit_hip_forward_u8_boxes(vit_hip_ctx *ctx, const vit_image_u8 *images, int n_images, const vit_box_u8 *boxes, int n, int layout,
                             int filter, const vit_pixel_norm *norm, float *logits, float **probs)
{
    const struct ingest_src src = {.kind = INGEST_U8_BOXES, .images = images, .n_images = n_images, .boxes = boxes, .filter = filter,
                                   .layout = layout, .norm = norm};
    return forward_host_u8(ctx, "vit_hip_forward_u8_boxes", &src, n, logits, probs);
}

/* $VIT_HIP_DEVICES: "all", or a comma-separated list of device ids; returns the count written. */
static int parse_devices(const char *env, int *out, int capacity)
{
    int n = 0;
    if (!env || !*env)
        return 0;
    if (strcmp(env, "all") == 0) {
        const int have = vh_device_count();
        for (int d = 0; d < have && n < capacity; ++d)
            out[n++] = d;
        return n;
    }
    for (const char *p = env; *p && n < capacity;) {
        char *end = NULL;
        const long v = strtol(p, &end, 10);
        if (end == p)
            break;
        out[n++] = (int)v;
        p = (*end == ',') ? end + 1 : end;
        if (*end != ',' && *end != '\0')
            break;
    }
    return n;
}

/* Wall-clock split of the calling thread's last ViT_opencl(): context creation (the reference's "setup time",
 * ViT_opencl.c:910) and everything after it up to the return (forward + teardown). */
static _Thread_local double last_setup_s, last_forward_s;
void vit_hip_last_call_seconds(double *setup_s, double *forward_s)
{
    if (setup_s)
        *setup_s = last_setup_s;
    if (forward_s)
        *forward_s = last_forward_s;
}

/* The drop-in entry point (reference ViT_opencl.c:794).  Same observable
 * behaviour: fills probabilities[i][0..999]; prints a setup-time line and a
 * throughput line where the reference prints "setup time" / "picture #i". */
void ViT_opencl(ImageData *image, Network *networks, float **probabilities)
{
    if (!image || !networks || !probabilities) {
        printf("[%s:%d] ViT_opencl: NULL argument\n", __FILE__, __LINE__);
        exit(EXIT_FAILURE);
    }
    const double t0 = wall_seconds();
    vit_config cfg;
    vit_config_preset(&cfg, "vit_b_16");
    const int n = image[0].n;
    if (n <= 0) {   /* the reference's per-image loop simply does not run (ViT_opencl.c:926); no device is touched */
        printf("setup time: 0.000000 sec (no images)\n\n");
        last_setup_s = last_forward_s = 0.0;
        return;
    }
    int device = 0;
    const char *env = getenv("VIT_HIP_DEVICE");
    if (env && *env)
        device = atoi(env);
    int devices[64];
    const int n_devices = parse_devices(getenv("VIT_HIP_DEVICES"), devices, 64);
    const int per_device = n_devices > 1 ? (n + n_devices - 1) / n_devices : n;
    int chunk = per_device < 512 ? per_device : 512;
    const char *envb = getenv("VIT_HIP_MAX_BATCH");
    if (envb && atoi(envb) > 0)
        chunk = atoi(envb) < per_device ? atoi(envb) : per_device;
    if (n_devices > 1) {
        /* $VIT_HIP_DEVICES names several GPUs: contiguous shards of the images, one replica per device */
        struct plan_env penv;
        plan_env_read(&penv);
        vit_hip_multi *m = NULL;
        int rcm = vit_hip_create_multi(&m, &cfg, networks, vit_config_num_tensors(&cfg), devices, n_devices, chunk, penv.precision);
        if (rcm != 0) {
            printf("[%s:%d] vit_hip_create_multi failed (%d): %s\n", __FILE__, __LINE__, rcm, vh_last_error());
            exit(EXIT_FAILURE);
        }
        const double t1m = wall_seconds();
        printf("setup time: %.6f sec (%d devices)\n\n", t1m - t0, n_devices);
        VH_CHECK(vit_hip_forward_multi(m, image, n, NULL, probabilities));
        const double t2m = wall_seconds();
        printf("pictures #0..#%d: %.6f sec (%.1f images/sec)\n\n", n - 1, t2m - t1m,
               (double)n / (t2m - t1m > 0 ? t2m - t1m : 1e-9));
        vit_hip_destroy_multi(m);
        last_setup_s = t1m - t0;
        last_forward_s = wall_seconds() - t1m;
        return;
    }
    if (n_devices == 1)
        device = devices[0];

    vit_hip_ctx *ctx = NULL;
    int rc = vit_hip_create(&ctx, &cfg, networks, vit_config_num_tensors(&cfg), device, chunk);
    if (rc != 0) {
        printf("[%s:%d] vit_hip_create failed (%d): %s\n", __FILE__, __LINE__, rc, vh_last_error());
        exit(EXIT_FAILURE);
    }
    const double t1 = wall_seconds();
    printf("setup time: %.6f sec (%s)\n\n", t1 - t0, vh_device_name());
    VH_CHECK(vit_hip_forward(ctx, image, n, NULL, probabilities));
    const double t2 = wall_seconds();
    printf("pictures #0..#%d: %.6f sec (%.1f images/sec)\n\n", n - 1, t2 - t1,
           (double)n / (t2 - t1 > 0 ? t2 - t1 : 1e-9));
    vit_hip_destroy(ctx);
    last_setup_s = t1 - t0;
    last_forward_s = wall_seconds() - t1;
}
