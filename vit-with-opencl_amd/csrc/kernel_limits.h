/*
 * kernel_limits.h -- what the host has to know about the kernels before it launches any: the shapes each one takes and the
 * bytes of scratch each one needs, stated once.  Plain C11 that is also C++17: constants and pure arithmetic, no device
 * code and no symbol of the shim, so that the units that run without a device (csrc/vit_plan.c, csrc/vit_requests.c, the
 * frame sizing of csrc/ViT_hip.c) and stand-alone test programs read the same numbers as the launchers.
 *
 *  - the exported sizing and limit entries of include/kernelHandler.h (vh_layer_norm_planes_max_embed, vh_rollout_workspace,
 *    ...) are one-line calls of the kl_ function of the same name;
 *  - every launcher refusal that compares against one of these limits reads the constant here;
 *  - a kernel either takes its constexpr from here or, where it derives the number from its own tiling, keeps it and holds it
 *    against this header with a static_assert in its .hip.
 * A new kernel adds its limits here in the same way.  tests/kernel_limits_main.c prints all of it over a sweep.
 */
#ifndef VIT_KERNEL_LIMITS_H
#define VIT_KERNEL_LIMITS_H

#include "kernelHandler.h"   /* the limits that are public already: VH_GALLERY_MAX_SPLITS, VH_STITCH_BLOCK, VH_STITCH_MAX_SIDE */

#include <stddef.h>

/* A function of this header: static inline in C.  In C++ it is constexpr, which lets a .hip file hold a kernel's own
 * constant against a function's result in a static_assert, and lets a kernel call it (the compiler takes a constexpr
 * function for host and device alike). */
#ifdef __cplusplus
#define KL_FN static constexpr
#else
#define KL_FN static inline
#endif

enum { KL_LDS_BYTES = 160 * 1024 };   /* the LDS of a CU (gfx950) */

/* ---- attention -------------------------------------------------------------------------------------------------------- */
enum {
    KL_ATTN_HD64_MAX_TOKENS = 208,        /* the resident head_dim-64 kernels (attention_f32.hip: three buffers of fp32 rows;
                                           * attention_p3.hip: two buffers of six 64-byte planes): K and V of a head in LDS */
    KL_ATTN_HD80_MAX_TOKENS = 272,        /* the resident head_dim-80 kernel (attention_h16.hip): 17 key tiles of 16 */
    KL_ATTN_STREAMING_MAX_TOKENS = 512    /* the streaming kernel (attention_tiled.hip): 32 key tiles of 16 in registers;
                                           * beyond it only the long kernel (attention_long.hip) runs */
};
/* the head dims the long kernel is built for; it takes any number of tokens */
KL_FN int kl_attn_long_head_dim_ok(int head_dim) { return head_dim == 64 || head_dim == 80; }

/* ---- LayerNorm on planes (rowops.hip) --------------------------------------------------------------------------------- */
enum { KL_LN_PLANES_ROWS = 16, KL_LN_PLANES_MAX_EMBED = 2048 };   /* rows staged in LDS; the widest row the registers hold */
/* the widest row: KL_LN_PLANES_ROWS rows of every part in LDS, 64 bytes per part and 32 columns.  2048 with one part, 1696
 * with three; 0 for any other number of parts */
KL_FN int kl_layer_norm_planes_max_embed(int parts)
{
    if (parts != 1 && parts != 3)
        return 0;
    const int by_lds = KL_LDS_BYTES / (parts * KL_LN_PLANES_ROWS * 64) * 32;
    return by_lds < KL_LN_PLANES_MAX_EMBED ? by_lds : KL_LN_PLANES_MAX_EMBED;
}

/* ---- the LayerNorm fold (norm_fold.h) --------------------------------------------------------------------------------- */
enum { KL_FOLD_GROUP = 128, KL_FOLD_MAX_GROUPS = 16 };   /* one partial (sum, sum of squares) per row and 128 columns; the
                                                          * consumer's four lanes of a row add at most four each */

/* ---- patch embedding -------------------------------------------------------------------------------------------------- */
enum {
    KL_PATCH_PLANES_K_STEP = 128,   /* the one-part K step of the planes GEMM (64 * P1_KG, gemm_p3.hip) */
    KL_PATCH_ROWS_K_STEP = 32       /* the K step of the fp32-rows GEMM (BK, gemm_common.h) */
};
/* in_chans * patch^2 padded with zeros to the planes GEMM's one-part K step */
KL_FN int kl_patch_planes_k(int in_chans, int patch_size)
{
    const int K = in_chans * patch_size * patch_size, step = KL_PATCH_PLANES_K_STEP;
    return (K + step - 1) / step * step;
}
/* fp32 rows, im2row on load: four consecutive kw are one aligned 16-byte read of an image row */
KL_FN int kl_patch_direct(int in_chans, int img_w, int patch_size)
{
    return patch_size % 4 == 0 && (in_chans * patch_size * patch_size) % KL_PATCH_ROWS_K_STEP == 0 && img_w % 4 == 0;
}
/* fp32 rows on an img_h x img_w image: bytes of the gathered, zero-padded patch rows and the padded weights; 0 where the
 * GEMM gathers on load */
KL_FN size_t kl_patch_rows_workspace(int n_images, int in_chans, int img_h, int img_w, int patch_size, int embed_dim)
{
    if (n_images <= 0 || in_chans <= 0 || img_h <= 0 || img_w <= 0 || patch_size <= 0 || embed_dim <= 0 ||
        img_h % patch_size != 0 || img_w % patch_size != 0 || kl_patch_direct(in_chans, img_w, patch_size))
        return 0;
    const size_t np = (size_t)(img_h / patch_size) * (size_t)(img_w / patch_size), K = (size_t)in_chans * patch_size * patch_size;
    const size_t Kp = (K + KL_PATCH_ROWS_K_STEP - 1) / KL_PATCH_ROWS_K_STEP * KL_PATCH_ROWS_K_STEP;
    return ((size_t)n_images * np + (size_t)embed_dim) * Kp * sizeof(float);
}

/* ---- MX activations (gemm_mx.hip) ------------------------------------------------------------------------------------- */
/* the scale bytes of an activation tensor [rows][cols]: [ceil(cols / 512)][4][rows][4] */
KL_FN size_t kl_mx_act_scale_bytes(int rows, int cols)
{
    return rows > 0 && cols > 0 ? (size_t)((cols / 128 + 3) / 4) * 16 * (size_t)rows : 0;
}

/* ---- class-token attention maps (attn_map.hip) and rollout (rollout.hip), which read Q|K|V through qkv_forms.h ---------- */
enum { KL_CLS_ATTN_MAX_HEAD_DIM = 128 };
KL_FN int kl_cls_attention_head_dim_ok(int head_dim)
{
    return head_dim > 0 && head_dim % 16 == 0 && head_dim <= KL_CLS_ATTN_MAX_HEAD_DIM;
}

enum { KL_ROLLOUT_QUERY_ROWS = 16, KL_ROLLOUT_KEY_CHUNK = 64 };   /* query rows per workgroup; keys per staged chunk */
/* a step's workspace: one T x T fp32 matrix per image */
KL_FN size_t kl_rollout_workspace(int n_images, int tokens)
{
    return n_images > 0 && tokens > 0 ? (size_t)n_images * (size_t)tokens * (size_t)tokens * sizeof(float) : 0;
}
/* row stride of the score tile in floats: whole key chunks, and the 4 row groups of a matrix result 16 banks apart */
KL_FN int kl_rollout_score_stride(int tokens)
{
    return (tokens + KL_ROLLOUT_KEY_CHUNK - 1) / KL_ROLLOUT_KEY_CHUNK * KL_ROLLOUT_KEY_CHUNK + 20;
}
/* the score rows of a workgroup's queries against every key, and the staged query and key rows of head_dim + 4 floats */
KL_FN size_t kl_rollout_lds_bytes(int tokens, int head_dim)
{
    return ((size_t)KL_ROLLOUT_QUERY_ROWS * kl_rollout_score_stride(tokens) +
            (size_t)(KL_ROLLOUT_QUERY_ROWS + KL_ROLLOUT_KEY_CHUNK) * (head_dim + 4)) * sizeof(float);
}
/* the most tokens whose score rows fit the LDS: whole key chunks */
KL_FN int kl_rollout_max_tokens(int head_dim)
{
    int T = 0;
    while (kl_rollout_lds_bytes(T + KL_ROLLOUT_KEY_CHUNK, head_dim) <= (size_t)KL_LDS_BYTES)
        T += KL_ROLLOUT_KEY_CHUNK;
    return T;
}

/* ---- gallery search (gallery.hip) ------------------------------------------------------------------------------------- */
enum { KL_GALLERY_ROW_TILE = 128, KL_GALLERY_MAX_EMBED = 2048 };   /* gallery rows per tile; the widest query */
/* (score, index) pairs of 8 bytes per query, split and rank; splits = 0: a bound on whatever the launcher chooses */
KL_FN size_t kl_gallery_workspace(int n_queries, long n_rows, int k, int splits)
{
    if (n_queries < 1 || n_rows < 1 || k < 1 || splits < 0)
        return 0;
    if (splits == 0) {
        const long tiles = (n_rows + KL_GALLERY_ROW_TILE - 1) / KL_GALLERY_ROW_TILE;
        splits = tiles < VH_GALLERY_MAX_SPLITS ? (int)tiles : VH_GALLERY_MAX_SPLITS;
    }
    return (size_t)n_queries * (size_t)splits * (size_t)k * sizeof(unsigned long long);
}

/* ---- feature readout (features.hip) ----------------------------------------------------------------------------------- */
enum { KL_READOUT_ROWS = 32 };   /* patch rows per workgroup: one partial sum of embed_dim floats each */
KL_FN size_t kl_feature_readout_scratch(int n_images, int tokens, int embed_dim)
{
    if (n_images <= 0 || tokens < 2 || embed_dim <= 0)
        return 0;
    return (size_t)n_images * ((tokens - 1 + KL_READOUT_ROWS - 1) / KL_READOUT_ROWS) * embed_dim * sizeof(float);
}

/* ---- dense head (dense_head.hip) -------------------------------------------------------------------------------------- */
enum { KL_DENSE_MAX_EMBED = 2048 };
/* ---- the per-pixel kernels of the dense head: labels (dense_head.hip) and the soft maps (dense_soft.hip) ------------- */
enum { KL_DENSE_MAX_OUT = 4096 };   /* the largest out_h and out_w */
/* patch rows r0 and r1 of one image x n_labels in LDS, label stride n_labels | 1 (odd: neighbouring patches on other banks) */
KL_FN int kl_dense_label_stride(int n_labels) { return n_labels | 1; }
KL_FN size_t kl_dense_labels_lds(int grid_w, int n_labels)
{
    return (size_t)2 * (size_t)grid_w * (size_t)kl_dense_label_stride(n_labels) * sizeof(float);
}
/* what vh_launch_dense_labels and vh_launch_dense_soft take besides their pointers: the shape of a launch */
KL_FN int kl_dense_pixel_shape_ok(int n_images, int grid_h, int grid_w, int n_labels, int out_h, int out_w)
{
    return n_labels >= 2 && n_labels <= VH_DENSE_MAX_LABELS && grid_h >= 1 && grid_w >= 1 && grid_h <= VH_DENSE_MAX_GRID &&
           grid_w <= VH_DENSE_MAX_GRID && out_h >= 1 && out_w >= 1 && out_h <= KL_DENSE_MAX_OUT && out_w <= KL_DENSE_MAX_OUT &&
           n_images >= 1 && (long)n_images * grid_h <= 2147483647L;
}

/* ---- stitch (dense_stitch.hip) ---------------------------------------------------------------------------------------- */
KL_FN size_t kl_round16(size_t v) { return (v + 15) & ~(size_t)15; }
/* the boxes, the offsets of every block of VH_STITCH_BLOCK^2 pixels and one more, the ids; 0 for arguments out of range */
KL_FN size_t kl_dense_stitch_scratch(int n_windows, int frame_h, int frame_w, long n_ids)
{
    if (n_windows < 1 || frame_h < 1 || frame_w < 1 || frame_h > VH_STITCH_MAX_SIDE || frame_w > VH_STITCH_MAX_SIDE || n_ids < 0 ||
        n_ids > 2147483647L)
        return 0;
    const size_t blocks = (size_t)((frame_h + VH_STITCH_BLOCK - 1) / VH_STITCH_BLOCK) * (size_t)((frame_w + VH_STITCH_BLOCK - 1) / VH_STITCH_BLOCK);
    return kl_round16((size_t)n_windows * 16) + kl_round16((blocks + 1) * sizeof(int)) + kl_round16((size_t)n_ids * sizeof(int)) + 16;
}

/* ---- soft stitch (dense_stitch_soft.hip): its scratch is the stitch's, kl_dense_stitch_scratch ---------------------------- */
/* How pass 2 comes by the means pass 1 formed (the same bits either way): blend again, or read them back from registers */
enum { KL_STITCH_SOFT_RECOMPUTE = 1, KL_STITCH_SOFT_REGISTERS = 2 };
enum { KL_STITCH_SOFT_CHUNK = 16, KL_STITCH_SOFT_REG_MAX_LABELS = 160 };   /* classes per chunk; ten chunks of means in registers */
/* the chunks of the register variant's instance that holds n_labels: built for 2, 4, 7 and 10; 0 beyond */
KL_FN int kl_dense_stitch_soft_reg_chunks(int n_labels)
{
    const int chunks = (n_labels + KL_STITCH_SOFT_CHUNK - 1) / KL_STITCH_SOFT_CHUNK;
    return chunks <= 2 ? 2 : chunks <= 4 ? 4 : chunks <= 7 ? 7 : chunks <= 10 ? 10 : 0;
}
KL_FN int kl_dense_stitch_soft_variant_ok(int variant, int n_labels)
{
    return variant == KL_STITCH_SOFT_RECOMPUTE || (variant == KL_STITCH_SOFT_REGISTERS && n_labels <= KL_STITCH_SOFT_REG_MAX_LABELS);
}
/* what a launch takes, by n_labels alone (measured: DESIGN.md 7, docs/LABBOOK.md) */
KL_FN int kl_dense_stitch_soft_variant(int n_labels)
{
    return n_labels <= KL_STITCH_SOFT_REG_MAX_LABELS ? KL_STITCH_SOFT_REGISTERS : KL_STITCH_SOFT_RECOMPUTE;
}

#endif
