/*
 * vit_plan.h -- what a context will run, decided once before anything is allocated: the kernels a forward takes, the
 * layout of the weight slabs and the size of every arena buffer with the borrowers it has to hold.  Internal to the
 * library: ViT_hip.c makes one plan per context and only reads it afterwards.  vit_plan.c is plain C and needs no device:
 * its outside symbols are vh_set_error and ingest_max_table_bytes, and what it knows about the kernels' shape limits and
 * scratch sizes is the arithmetic of csrc/kernel_limits.h.
 * tests/plan_main.c runs it against tests/golden/plan_table.txt.
 */
#ifndef VIT_PLAN_H
#define VIT_PLAN_H

#include "ViT_opencl.h"

#include <stddef.h>

/* The mode's GEMM-operand copy of one of the four big matrices of a layer (in_proj, out_proj, fc1, fc2) */
struct operand
{
    void *w;             /* three-part planes (F32; NULL for shapes the planes cannot take), one-part planes (BF16_GEMM),
                          * two fp16 parts (F32_FP16X2) or MX e4m3 values (FP8_GEMM) */
    void *scales;        /* FP8_GEMM: the e8m0 block scales of w */
    float pair_scale;    /* F32_FP16X2: the power of two the fp16 parts were scaled by */
    /* ln_fold, in_proj and fc1 only (csrc/norm_fold.h): w holds the gamma-scaled matrix; colsum [N] of its rounded values
     * and the folded bias [N] */
    float *colsum, *bias_folded;
};

/* The weight slabs, one device allocation each, in the order a planes file stores them */
enum { SLAB_F32, SLAB_OPERAND, SLAB_CONV, SLAB_FOLD, N_SLABS };

/* How the planes paths (F32 on planes, BF16_GEMM, FP8_GEMM) run attention: Q|K|V as one-part fp16 planes into a resident
 * kernel -- head_dim 64, or head_dim 80 (ViT-H/14, reduced modes only) which writes the output projection's operand
 * itself -- or fp32 rows through the streaming kernel (T <= 512).  ATTN_LONG: Q|K|V as the mode's planes into the
 * flash-style kernel (csrc/attention_long.hip; any T, head_dim 64 or 80), fp32 rows out into the idle MLP buffer, then
 * rounded / split like the streaming kernel's -- every T > 512, and any T under $VIT_HIP_ATTN=long */
enum { ATTN_STREAMING, ATTN_HD64, ATTN_HD80, ATTN_LONG };

enum { MAX_DEPTH = 256, MAX_TENSORS = 4 + 12 * MAX_DEPTH + 4 };

/* the tensor index of operand m = 4 * layer + (0 in_proj, 1 out_proj, 2 fc1, 3 fc2) */
static inline int plan_operand_tensor(int m)
{
    static const int big[4] = {2, 4, 8, 10};   /* in_proj, out_proj, fc1, fc2 weights within a layer's 12 tensors */
    return 4 + 12 * (m / 4) + big[m % 4];
}

/* The six switches of the environment, parsed.  plan_env_read is the only reader of the environment; everything else
 * takes the struct, so a test passes switches as data. */
struct plan_env
{
    int precision;        /* $VIT_HIP_PRECISION: F32 unless "bf16" -> BF16_GEMM, "fp16x2" -> F32_FP16X2, "fp8" -> FP8_GEMM */
    int p3_off;           /* $VIT_HIP_P3=0 */
    int fp32_native;      /* $VIT_HIP_GEMM_FP32=native */
    int ln_fold;          /* $VIT_HIP_LN_FOLD: 0, 1, or -1 when it says neither */
    int last_layer_cls;   /* $VIT_HIP_LAST_LAYER=cls */
    int last_layer_full;  /* $VIT_HIP_LAST_LAYER=full */
    int last_layer_all_queries;   /* $VIT_HIP_LAST_LAYER=all_queries */
    int attn_long;        /* $VIT_HIP_ATTN=long */
    int attn_tiled;       /* $VIT_HIP_ATTN=tiled */
};
enum { PLAN_ENV_PRECISION, PLAN_ENV_P3, PLAN_ENV_GEMM_FP32, PLAN_ENV_LN_FOLD, PLAN_ENV_LAST_LAYER, PLAN_ENV_ATTN, PLAN_ENV_COUNT };
/* values[PLAN_ENV_*]: the switch's text, or NULL where it is unset */
void plan_env_parse(struct plan_env *env, const char *const values[PLAN_ENV_COUNT]);
void plan_env_read(struct plan_env *env);

/* Everything a forward, the weight layout or the arena branches on */
struct vit_plan
{
    int precision;      /* VIT_PRECISION_* */
    int ln_fold;        /* every LayerNorm but the final one folded into the projection behind it (csrc/norm_fold.h) */
    int use_p3;         /* F32: GEMM inputs travel as three-part bf16 planes (y, attn, hid hold 6 bytes per value) */
    int cls_only_last;  /* the last layer's output projection and MLP run on the class-token rows only, where cls_only_ok: the
                         * one field that changes after creation (vit_hip_set_last_layer_cls_only alone; a forward only reads it) */
    int attn_form;      /* ATTN_*, for the planes paths */
    int fp32_native;    /* $VIT_HIP_GEMM_FP32=native: F32 on fp32 rows, with the fp32 matrix instruction in the patch embedding, the
                         * attention and every projection without pre-split weights (VH_FP32_NATIVE, VH_ATTN_NATIVE) */
    int attn_rows_streaming;   /* $VIT_HIP_ATTN=tiled: attention that reads fp32 rows takes the streaming kernel at every shape */
    int tokens;
    int qkv_form;       /* VH_QKV_*: what the QKV projection writes, and the attention and the attention maps read */
    /* F32 keeps three-part planes of the weights wherever the shape allows: use_p3 without the environment and the batch
     * bound, because the weight slabs -- and with them a planes file -- must depend on (config, precision, ln_fold) alone.  A
     * file written under one setting loads under another, and the fp32-rows path reads the pre-split weights where they exist. */
    int weight_planes;
    int operand_bytes;  /* per weight of the operand copies: 6, 2, 4 or 1; 0 where F32 keeps none */
    int operand_scales; /* FP8_GEMM: one e8m0 scale per 32 weights behind each operand */
    int conv_parts;     /* of conv_proj's planes: 1 (bf16; BF16_GEMM, FP8_GEMM), 3 (the exact split; weight_planes) or 0 (none) */
    int planes_patch_embed;   /* the patch embedding runs on planes (an im2row producer); 0 on the fp32-rows paths */
    int act_bytes;      /* the arena holds this many bytes per GEMM-input value in y, attn, Q|K|V and hid */
    int cls_only_ok;    /* the class-only last layer may run: planes path, no fold, T >= 4, and its scratch for
                         * max_batch class rows (plan_cls_only_scratch) fits Q|K|V */
    int last_layer_lazy; /* where cls_only_ok, unless $VIT_HIP_LAST_LAYER=full: a forward evaluates the last layer behind its
                         * attention for the class-token rows only and leaves the other rows pending; whoever reads them
                         * afterwards (vit_hip_read_tokens) runs the same launches on all rows first */
    int cls_query;      /* such a forward also runs the last layer's Q projection and attention for the class-token query
                         * alone (K and V on all rows): last_layer_lazy with the resident three-part attention, where the
                         * scratch with the class rows of LN1 and Q behind it (plan_cls_query_scratch) fits the place of Q
                         * in Q|K|V at every batch, unless $VIT_HIP_LAST_LAYER=all_queries.  Otherwise Q|K|V and the attention
                         * run on all rows, never an allocation in the forward */
    size_t slab_bytes[N_SLABS];
    /* the arena (plan_make states each buffer's borrowers).  hid doubles as the workspace of the patch embedding, the resize
     * and the feature readout, which are told ws_bytes */
    size_t x_bytes, y_bytes, attn_bytes, qkv_bytes, ws_bytes, stats_bytes;
    size_t crop_off;    /* resized crops lie in Q|K|V from here on (behind the fp32 expansion on the fp32-rows paths) */
    size_t e_scales_off, hid_scales_off;   /* FP8_GEMM: where the MX scales lie behind the values in y and attn, and in hid */
};

/* The argument checks of both ways of making a context and the plan of its forward pass.  ln_fold < 0: decide the fold
 * here (env); 0 or 1: a planes file's header fixed it, and a fold this context cannot run is refused like any other bad
 * header.  Returns 0, 1 (bad argument) or 2 (a shape, precision or batch nothing runs; some with the thread's error text).
 * Allocates nothing. */
int plan_make(struct vit_plan *plan, const vit_config *cfg, int n_tensors, int max_batch, int precision, int ln_fold,
              const struct plan_env *env);

/* Every tensor's place in the four weight slabs, from (cfg, precision, ln_fold) alone, so a planes file written by one
 * context (vit_hip_export_planes) drops into another's slabs byte for byte.  slabs NULL: only sums the slabs' sizes into
 * bytes[] (plan_make does; vit_hip_create_from_planes checks a file's header against them BEFORE anything is allocated).
 * With the allocated slabs it points w [n_tensors] and op [4 * depth] into them; bytes may then be NULL. */
void plan_layout(const struct vit_plan *plan, const vit_config *cfg, void *const slabs[N_SLABS], float **w, struct operand *op,
                 size_t bytes[N_SLABS]);

/* The class-only last layer's scratch for n class rows, laid into Q|K|V: x_cls at 0, then attn_cls, y_cls and hid_cls at
 * off[0..2]; returns its bytes */
size_t plan_cls_only_scratch(const vit_config *cfg, int n, size_t off[3]);
/* ... with the class query's planes (n class rows of Q, [E/32][3][n][32]) behind it at *q_off; returns the bytes of both.
 * The class rows of LN1's planes, the Q projection's input, lie in y_cls until LN2 writes it. */
size_t plan_cls_query_scratch(const vit_config *cfg, int n, size_t *q_off);

#endif
