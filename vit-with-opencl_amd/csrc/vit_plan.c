/*
 * vit_plan.c -- the plan of a context (csrc/vit_plan.h): the switches of the environment, the argument checks, which
 * kernels a forward takes, where every weight lies in its slab and how large every arena buffer must be for all that
 * borrow it.  Host arithmetic only; nothing here allocates or touches a device.  What it knows about the kernels -- the
 * shapes each one takes, the bytes each one needs -- it reads from csrc/kernel_limits.h, as the launchers do.
 */
#include "vit_plan.h"
#include "vit_ingest.h"
#include "kernel_limits.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void plan_env_parse(struct plan_env *env, const char *const v[PLAN_ENV_COUNT])
{
    const char *const p = v[PLAN_ENV_PRECISION], *const fold = v[PLAN_ENV_LN_FOLD], *const attn = v[PLAN_ENV_ATTN];
    env->precision = (p && p[0] == 'b') ? VIT_PRECISION_BF16_GEMM
                   : (p && strncmp(p, "fp16x2", 6) == 0) ? VIT_PRECISION_F32_FP16X2
                   : (p && strncmp(p, "fp8", 3) == 0) ? VIT_PRECISION_FP8_GEMM : VIT_PRECISION_F32;
    env->p3_off = v[PLAN_ENV_P3] && v[PLAN_ENV_P3][0] == '0';
    env->fp32_native = v[PLAN_ENV_GEMM_FP32] && v[PLAN_ENV_GEMM_FP32][0] == 'n';
    env->ln_fold = (fold && fold[0] == '0') ? 0 : (fold && fold[0] == '1') ? 1 : -1;
    env->last_layer_cls = v[PLAN_ENV_LAST_LAYER] && strcmp(v[PLAN_ENV_LAST_LAYER], "cls") == 0;
    env->last_layer_full = v[PLAN_ENV_LAST_LAYER] && strcmp(v[PLAN_ENV_LAST_LAYER], "full") == 0;
    env->last_layer_all_queries = v[PLAN_ENV_LAST_LAYER] && strcmp(v[PLAN_ENV_LAST_LAYER], "all_queries") == 0;
    env->attn_long = attn && strcmp(attn, "long") == 0;
    env->attn_tiled = attn && attn[0] == 't';
}

void plan_env_read(struct plan_env *env)
{
    const char *const values[PLAN_ENV_COUNT] = {getenv("VIT_HIP_PRECISION"), getenv("VIT_HIP_P3"), getenv("VIT_HIP_GEMM_FP32"),
                                                getenv("VIT_HIP_LN_FOLD"), getenv("VIT_HIP_LAST_LAYER"), getenv("VIT_HIP_ATTN")};
    plan_env_parse(env, values);
}

static size_t max_of(size_t a, size_t b) { return a > b ? a : b; }

size_t plan_cls_only_scratch(const vit_config *cfg, int n, size_t off[3])
{
    const size_t rows = (size_t)n, E = (size_t)cfg->embed_dim, F = (size_t)cfg->mlp_hidden;
    size_t o[3];
    o[0] = align_up(rows * E * 4, 256);          /* attn_cls, behind x_cls: fp32 rows */
    o[1] = o[0] + align_up(rows * E * 6, 256);   /* y_cls; attn_cls, y_cls and hid_cls are three-part planes */
    o[2] = o[1] + align_up(rows * E * 6, 256);   /* hid_cls */
    if (off)
        memcpy(off, o, sizeof o);
    return o[2] + rows * F * 6;
}

size_t plan_cls_query_scratch(const vit_config *cfg, int n, size_t *q_off)
{
    const size_t at = align_up(plan_cls_only_scratch(cfg, n, NULL), 256);
    if (q_off)
        *q_off = at;
    return at + (size_t)n * (size_t)cfg->embed_dim * 6;
}

/* The next 256-byte aligned piece of a slab: its address once the slab exists, NULL while only sizing. */
static void *place(void *slab, size_t *off, size_t bytes)
{
    void *p = slab ? (char *)slab + *off : NULL;
    *off += align_up(bytes, 256);
    return p;
}

void plan_layout(const struct vit_plan *plan, const vit_config *cfg, void *const slabs[N_SLABS], float **w, struct operand *op,
                 size_t bytes[N_SLABS])
{
    void *const none[N_SLABS] = {NULL};
    void *const *slab = slabs ? slabs : none;
    struct operand unplaced_op;   /* while only sizing, the places go nowhere */
    size_t off[N_SLABS] = {0};
    for (int i = 0; i < vit_config_num_tensors(cfg); ++i) {
        float *p = (float *)place(slab[SLAB_F32], &off[SLAB_F32], vit_config_tensor_size(cfg, i) * sizeof(float));
        if (slabs)
            w[i] = p;
    }
    for (int m = 0; m < 4 * cfg->depth; ++m) {
        struct operand *o = slabs ? &op[m] : &unplaced_op;
        const size_t cnt = vit_config_tensor_size(cfg, plan_operand_tensor(m));
        o->w = place(slab[SLAB_OPERAND], &off[SLAB_OPERAND], cnt * (size_t)plan->operand_bytes);
        if (plan->operand_scales)
            o->scales = place(slab[SLAB_OPERAND], &off[SLAB_OPERAND], cnt / 32);
        if (plan->ln_fold && m % 2 == 0) {   /* in_proj and fc1: one float per output feature each */
            const size_t nb = vit_config_tensor_size(cfg, plan_operand_tensor(m) + 1) * sizeof(float);
            o->colsum = (float *)place(slab[SLAB_FOLD], &off[SLAB_FOLD], nb);
            o->bias_folded = (float *)place(slab[SLAB_FOLD], &off[SLAB_FOLD], nb);
        }
    }
    place(slab[SLAB_CONV], &off[SLAB_CONV],   /* E % 128 == 0 wherever there are parts: already 256-byte aligned */
          (size_t)kl_patch_planes_k(cfg->in_chans, cfg->patch_size) * (size_t)cfg->embed_dim * 2 * (size_t)plan->conv_parts);
    if (bytes)
        memcpy(bytes, off, sizeof(off));
}

/* The arena for max_batch images: every buffer is the largest of what lies in it, one line per borrower */
static void plan_arena(struct vit_plan *plan, const vit_config *cfg, int max_batch)
{
    const size_t E = (size_t)cfg->embed_dim, F = (size_t)cfg->mlp_hidden, act = (size_t)plan->act_bytes, n = (size_t)max_batch;
    const size_t rows = n * (size_t)plan->tokens, patches = (size_t)plan->tokens - 1;
    const int width = cfg->img_width ? cfg->img_width : cfg->img_size;
    const size_t img = (size_t)cfg->in_chans * cfg->img_size * width;
    const int fp8 = plan->precision == VIT_PRECISION_FP8_GEMM, resizes = cfg->in_chans <= 4;
    const int planes_path = plan->use_p3 || plan->precision == VIT_PRECISION_BF16_GEMM || fp8;
    size_t b;

    plan->x_bytes = rows * E * sizeof(float);   /* the residual stream, fp32 rows */

    /* y and attn, the LayerNorm's and the attention's output: GEMM inputs */
    b = rows * E * act;
    if (fp8) {   /* ... as MX tensors: a byte per value, then the scales (rows that overflow an int run no forward either) */
        plan->e_scales_off = align_up(rows * E, 256);
        b = max_of(b, plan->e_scales_off + kl_mx_act_scale_bytes((int)rows, cfg->embed_dim));
    }
    plan->y_bytes = plan->attn_bytes = b;

    /* Q|K|V.  The class-only last layer's scratch borrows it too, but does not size it: cls_only_ok says whether it fits */
    const size_t expanded = plan->planes_patch_embed ? 0 : n * img * sizeof(float);
    plan->crop_off = align_up(expanded, 256);
    b = rows * 3 * E * act;                       /* Q|K|V itself, as rows or planes */
    b = max_of(b, expanded);                      /* the fp32-rows paths expand max_batch 8-bit images to fp32 here */
    if (resizes)
        b = max_of(b, plan->crop_off + n * img);  /* max_batch resized crops of img x img x C bytes, behind that expansion */
    plan->qkv_bytes = b;

    /* hid, which doubles as the workspace of whatever runs while the MLP is idle.  The feature readout's partial sums go
     * through it as well; its launch checks them against ws_bytes */
    b = rows * F * act;                           /* the MLP's hidden activations */
    if (fp8) {                                    /* ... as an MX tensor */
        plan->hid_scales_off = align_up(rows * F, 256);
        b = max_of(b, plan->hid_scales_off + kl_mx_act_scale_bytes((int)rows, cfg->mlp_hidden));
    }
    /* the gathered patch rows of geometries such as H/14, square or not */
    b = max_of(b, kl_patch_rows_workspace(max_batch, cfg->in_chans, cfg->img_size, width, cfg->patch_size, cfg->embed_dim));
    /* the im2row producer's planes: patches x Kp x 2 bytes x parts (a small MLP can be smaller than that) */
    b = max_of(b, n * patches * (size_t)kl_patch_planes_k(cfg->in_chans, cfg->patch_size) * 2 * (size_t)plan->conv_parts);
    if (resizes)
        b = max_of(b, n * ingest_max_table_bytes(cfg->img_size));   /* the resize's coefficient tables at the steepest downscale */
    if (planes_path && (plan->attn_form == ATTN_STREAMING || plan->attn_form == ATTN_LONG))
        b = max_of(b, rows * E * sizeof(float));  /* the streaming and the long kernel's fp32 rows, before they are split or
                                                   * rounded into attn */
    plan->ws_bytes = b;

    plan->stats_bytes = plan->ln_fold ? rows * (E / KL_FOLD_GROUP) * 2 * sizeof(float) : 0;   /* partial (sum, sum of squares) per row */
}

int plan_make(struct vit_plan *plan, const vit_config *cfg, int n_tensors, int max_batch, int precision, int ln_fold,
              const struct plan_env *env)
{
    if (!cfg || max_batch <= 0)
        return 1;
    if (precision != VIT_PRECISION_F32 && precision != VIT_PRECISION_BF16_GEMM && precision != VIT_PRECISION_FP8_GEMM &&
        precision != VIT_PRECISION_F32_FP16X2)
        return 1;
    if (precision == VIT_PRECISION_F32_FP16X2 && (cfg->embed_dim % 128 != 0 || cfg->mlp_hidden % 128 != 0))
        return 2;
    if (precision == VIT_PRECISION_FP8_GEMM && (cfg->embed_dim % 256 != 0 || cfg->mlp_hidden % 256 != 0))
        return 2;
    if (precision == VIT_PRECISION_BF16_GEMM && (cfg->embed_dim % 128 != 0 || cfg->mlp_hidden % 128 != 0))
        return 2;
    if (cfg->depth <= 0 || cfg->embed_dim <= 0 || cfg->num_heads <= 0 || cfg->patch_size <= 0 || cfg->img_size <= 0 ||
        cfg->in_chans <= 0 || cfg->num_classes <= 0 || cfg->mlp_hidden <= 0)
        return 2;
    /* sane sizes: what a context may be asked to allocate is bounded whatever a caller or a file header says */
    if (cfg->depth > MAX_DEPTH || cfg->embed_dim > 16384 || cfg->mlp_hidden > 65536 || cfg->img_size > 4096 || cfg->in_chans > 64 ||
        cfg->num_classes > (1 << 20) || cfg->num_heads > 1024 || max_batch > (1 << 20))
        return 2;
    if (n_tensors != vit_config_num_tensors(cfg))
        return 2;
    if (cfg->embed_dim % cfg->num_heads != 0 || cfg->img_size % cfg->patch_size != 0)
        return 2;
    /* img_width: 0 or img_size is the square input; vit_config_canonical words the refusals of another width for the callers */
    if (cfg->img_width < 0 || cfg->img_width > 4096 || cfg->img_width % cfg->patch_size != 0)
        return 2;

    const int E = cfg->embed_dim, F = cfg->mlp_hidden, H = cfg->num_heads, T = vit_config_tokens(cfg);
    const int reduced = precision == VIT_PRECISION_BF16_GEMM || precision == VIT_PRECISION_FP8_GEMM;
    /* F32 by default writes every GEMM input as the exact three-part bf16 split (csrc/gemm_p3.hip), 6 bytes per value;
     * $VIT_HIP_P3=0 keeps fp32 activations and the in-loop split (csrc/gemm_mfma.hip), $VIT_HIP_GEMM_FP32=native the fp32
     * matrix instruction */
    const int planes_wanted = !env->p3_off && !env->fp32_native;
    const int weight_planes = precision == VIT_PRECISION_F32 && E % 128 == 0 && F % 128 == 0;
    const int use_p3 = weight_planes && planes_wanted && (size_t)max_batch * (size_t)T * 64 <= 0xffffffffull;
    /* the fold's row terms take at most KL_FOLD_MAX_GROUPS partial sums per row (row_norm_terms); on F32 it needs the planes
     * path */
    const int fold_fits = E % KL_FOLD_GROUP == 0 && E / KL_FOLD_GROUP <= KL_FOLD_MAX_GROUPS && (reduced || weight_planes);
    if (ln_fold < 0)
        /* the reduced modes fold unless $VIT_HIP_LN_FOLD=0 (the separate LayerNorm launches of rounds 1-3: the A/B of tests
         * and bench).  On F32 the fold is a LAB VARIANT, off unless $VIT_HIP_LN_FOLD=1: the same fold on the exact
         * three-part planes keeps the 1e-4 parity on the goldens, but puts it behind the x - mean cancellation for ~1 %
         * (docs/LABBOOK.md R4.6). */
        ln_fold = fold_fits && (reduced ? env->ln_fold != 0 : env->ln_fold == 1 && planes_wanted);
    if (ln_fold && (!fold_fits || (precision == VIT_PRECISION_F32 && !use_p3)))
        return vh_set_error(2, "vit_hip_create: this shape, precision and batch cannot fold the LayerNorms (the fp32 path "
                               "needs the planes path)");
    /* the planes path's LayerNorms write three parts per value through an LDS image that ends at embed_dim 1696
     * (kl_layer_norm_planes_max_embed; csrc/rowops.hip); the lab fold launches none of them */
    if (use_p3 && !ln_fold && E > kl_layer_norm_planes_max_embed(3)) {
        char msg[320];
        snprintf(msg, sizeof msg, "vit_hip_create: embed_dim=%d: the fp32 planes path's LayerNorm (three-part planes, 96 bytes of "
                 "LDS per column) takes a LayerNorm width of at most %d",
                 E, kl_layer_norm_planes_max_embed(3));
        return vh_set_error(2, msg);
    }
    /* attention: ATTN_LONG is the only kernel past KL_ATTN_STREAMING_MAX_TOKENS, and it reads the planes paths' Q|K|V with
     * head_dim 64 or 80; $VIT_HIP_ATTN=long forces it at any T (tests, A/B), $VIT_HIP_ATTN=tiled the streaming kernel wherever
     * attention reads fp32 rows (the planes paths' resident kernels are not rows kernels and stay).  Shapes no kernel runs are
     * refused here, not at every forward. */
    const int long_hd = kl_attn_long_head_dim_ok(E / H);   /* E % H == 0 here */
    const int long_wanted = T > KL_ATTN_STREAMING_MAX_TOKENS || env->attn_long;
    if (T > KL_ATTN_STREAMING_MAX_TOKENS &&
        (precision == VIT_PRECISION_F32_FP16X2 || (precision == VIT_PRECISION_F32 && !use_p3) || !long_hd)) {
        char msg[320];
        snprintf(msg, sizeof msg, "vit_hip_create: %d tokens: above %d tokens attention runs on the planes paths (F32 with "
                 "embed_dim and mlp_hidden multiples of 128 and neither $VIT_HIP_P3=0 nor $VIT_HIP_GEMM_FP32=native, BF16_GEMM, "
                 "FP8_GEMM; not F32_FP16X2) with head_dim 64 or 80 (precision %d, head_dim %d)",
                 T, KL_ATTN_STREAMING_MAX_TOKENS, precision, E / H);
        return vh_set_error(2, msg);
    }

    memset(plan, 0, sizeof(*plan));
    plan->precision = precision;
    plan->ln_fold = ln_fold ? 1 : 0;
    plan->use_p3 = use_p3;
    plan->cls_only_last = use_p3 && !ln_fold && env->last_layer_cls;
    plan->attn_form = !(use_p3 || reduced) ? ATTN_STREAMING
                    : (long_wanted && long_hd) ? ATTN_LONG
                    : (E == 64 * H && T <= KL_ATTN_HD64_MAX_TOKENS) ? ATTN_HD64
                    : (reduced && E == 80 * H && T <= KL_ATTN_HD80_MAX_TOKENS) ? ATTN_HD80 : ATTN_STREAMING;
    plan->fp32_native = env->fp32_native;
    plan->attn_rows_streaming = env->attn_tiled;
    plan->tokens = T;
    /* the resident and the long kernels read Q|K|V as the mode's planes -- one fp16 part in the reduced modes, the exact three
     * parts on F32 except into the streaming kernel -- everything else fp32 rows */
    plan->qkv_form = plan->attn_form == ATTN_STREAMING ? VH_QKV_ROWS_F32 : reduced ? VH_QKV_PLANES_F16 : VH_QKV_PLANES3;
    plan->weight_planes = weight_planes;
    plan->operand_bytes = precision == VIT_PRECISION_BF16_GEMM ? 2 : precision == VIT_PRECISION_FP8_GEMM ? 1
                        : precision == VIT_PRECISION_F32_FP16X2 ? 4 : weight_planes ? 6 : 0;
    plan->operand_scales = precision == VIT_PRECISION_FP8_GEMM;
    plan->conv_parts = reduced ? 1 : weight_planes ? 3 : 0;
    plan->planes_patch_embed = plan->ln_fold || use_p3 || reduced;
    plan->act_bytes = use_p3 ? 6 : (int)sizeof(float);
    plan_layout(plan, cfg, NULL, NULL, NULL, plan->slab_bytes);
    plan_arena(plan, cfg, max_batch);
    plan->cls_only_ok = use_p3 && !ln_fold && T >= 4 && plan_cls_only_scratch(cfg, max_batch, NULL) <= plan->qkv_bytes;
    plan->last_layer_lazy = plan->cls_only_ok && !env->last_layer_full;
    /* the class query's scratch lies where the Q planes of the forward's n images would, in front of K: n * T * E * 6 bytes.
     * Per class row it takes 22 E + 6 F bytes and at most 5 * 256 of alignment in all, so it fits at every n if it fits so
     * at n = 1 */
    plan->cls_query = plan->last_layer_lazy && !env->last_layer_all_queries && plan->attn_form == ATTN_HD64 &&
                      plan->qkv_form == VH_QKV_PLANES3 &&
                      22 * (size_t)E + 6 * (size_t)F + 5 * 256 <= (size_t)T * (size_t)E * 6;
    return 0;
}
