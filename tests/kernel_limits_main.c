/*
 * kernel_limits_main.c -- csrc/kernel_limits.h on its own: every constant and every function of the header printed over a
 * sweep, one line each, "name arguments : results".  tests/test_kernel_limits_host.py builds it as C11 (-Wall -Wextra
 * -Wpedantic, no warning) under ASan + UBSan, and once more as C++17, whose output must be the same; it then holds every
 * exported sizing and limit entry of the loaded library against these lines, and the constants against the restatements the
 * Python references keep.  The sweep: head_dim 16..144 in steps of 16, tokens and rows on and either side of every
 * threshold, gallery rows on both sides of 128 x 1024 (where the cap on splits takes over), the patch geometries of B/16,
 * H/14 and a rectangle.
 */
#include "kernel_limits.h"

#include <stdio.h>

#define COUNT(a) (sizeof(a) / sizeof((a)[0]))
#define CONSTANT(name) printf("const " #name " : %ld\n", (long)(name))

int main(void)
{
    CONSTANT(KL_LDS_BYTES);
    CONSTANT(KL_ATTN_HD64_MAX_TOKENS);
    CONSTANT(KL_ATTN_HD80_MAX_TOKENS);
    CONSTANT(KL_ATTN_STREAMING_MAX_TOKENS);
    CONSTANT(KL_LN_PLANES_ROWS);
    CONSTANT(KL_LN_PLANES_MAX_EMBED);
    CONSTANT(KL_FOLD_GROUP);
    CONSTANT(KL_FOLD_MAX_GROUPS);
    CONSTANT(KL_PATCH_PLANES_K_STEP);
    CONSTANT(KL_PATCH_ROWS_K_STEP);
    CONSTANT(KL_CLS_ATTN_MAX_HEAD_DIM);
    CONSTANT(KL_ROLLOUT_QUERY_ROWS);
    CONSTANT(KL_ROLLOUT_KEY_CHUNK);
    CONSTANT(KL_GALLERY_ROW_TILE);
    CONSTANT(KL_GALLERY_MAX_EMBED);
    CONSTANT(KL_READOUT_ROWS);
    CONSTANT(KL_DENSE_MAX_EMBED);
    CONSTANT(VH_GALLERY_MAX_SPLITS);
    CONSTANT(VH_STITCH_BLOCK);
    CONSTANT(VH_STITCH_MAX_SIDE);

    /* per head_dim: the long kernel, the class-token maps, the rollout's most tokens and its LDS around that */
    static const int dims[] = {0, 16, 24, 32, 48, 64, 80, 96, 112, 128, 144};
    for (size_t i = 0; i < COUNT(dims); ++i) {
        const int D = dims[i], most = kl_rollout_max_tokens(D);
        printf("head_dim %d : %d %d %d\n", D, kl_attn_long_head_dim_ok(D), kl_cls_attention_head_dim_ok(D), most);
        for (int T = most - 64; T <= most + 1; T += T == most - 64 ? 63 : 1)
            printf("rollout_lds %d %d : %d %zu\n", T, D, kl_rollout_score_stride(T), kl_rollout_lds_bytes(T, D));
    }

    for (int parts = 0; parts <= 4; ++parts)
        printf("ln_planes %d : %d\n", parts, kl_layer_norm_planes_max_embed(parts));

    /* tokens on and either side of every attention limit, of a key chunk and of a readout workgroup's rows */
    static const int toks[] = {0, 1, 2, 17, 32, 33, 34, 64, 65, 197, 207, 208, 209, 257, 271, 272, 273, 511, 512, 513, 577, 1370};
    static const int batches[] = {0, 1, 4, 512};
    for (size_t b = 0; b < COUNT(batches); ++b)
        for (size_t i = 0; i < COUNT(toks); ++i) {
            printf("rollout_ws %d %d : %zu\n", batches[b], toks[i], kl_rollout_workspace(batches[b], toks[i]));
            for (int E = 0; E <= 1280; E += 640)
                printf("readout %d %d %d : %zu\n", batches[b], toks[i], E, kl_feature_readout_scratch(batches[b], toks[i], E));
        }

    /* MX scales: rows around nothing in particular, columns on and either side of a scale group of 512 */
    static const int rows[] = {0, 1, 197, 788, 100864}, cols[] = {0, 128, 256, 384, 512, 640, 768, 1024, 1152, 1280, 3072, 5120};
    for (size_t r = 0; r < COUNT(rows); ++r)
        for (size_t c = 0; c < COUNT(cols); ++c)
            printf("mx_scale %d %d : %zu\n", rows[r], cols[c], kl_mx_act_scale_bytes(rows[r], cols[c]));

    /* patch geometries {in_chans, img_h, img_w, patch, embed_dim}: B/16, B/16 at 384, H/14, H/14 at 518, rectangles, one
     * channel, a width that is no multiple of 4, sides that are no multiple of the patch */
    static const int geo[][5] = {{3, 224, 224, 16, 768}, {3, 384, 384, 16, 768},  {3, 224, 224, 14, 1280}, {3, 518, 518, 14, 1280},
                                 {3, 224, 384, 16, 768}, {3, 224, 336, 14, 1280}, {1, 64, 64, 4, 256},     {4, 30, 30, 6, 128},
                                 {2, 64, 36, 4, 128},    {3, 64, 18, 2, 128},     {3, 225, 224, 16, 768},  {3, 224, 225, 16, 768},
                                 {0, 224, 224, 16, 768}, {3, 224, 224, 16, 0}};
    for (size_t g = 0; g < COUNT(geo); ++g) {
        printf("patch_planes_k %d %d : %d\n", geo[g][0], geo[g][3], kl_patch_planes_k(geo[g][0], geo[g][3]));
        for (int n = 0; n <= 256; n = n ? n * 16 : 1)
            printf("patch_rows %d %d %d %d %d %d : %d %zu\n", n, geo[g][0], geo[g][1], geo[g][2], geo[g][3], geo[g][4],
                   kl_patch_direct(geo[g][0], geo[g][2], geo[g][3]),
                   kl_patch_rows_workspace(n, geo[g][0], geo[g][1], geo[g][2], geo[g][3], geo[g][4]));
    }

    /* gallery rows on and either side of a row tile and of 128 x 1024, from where the cap on splits holds */
    static const long n_rows[] = {0, 1, 127, 128, 129, 1000, 130944, 130945, 131071, 131072, 131073, 200000, 2147483647L};
    static const int splits[] = {-1, 0, 1, 7, 1024};
    for (size_t i = 0; i < COUNT(n_rows); ++i)
        for (int k = 0; k <= 32; k = k ? k * 4 : 1)
            for (size_t s = 0; s < COUNT(splits); ++s)
                for (int q = 0; q <= 3; q += 3)
                    printf("gallery %d %ld %d %d : %zu\n", q, n_rows[i], k, splits[s], kl_gallery_workspace(q, n_rows[i], k, splits[s]));

    /* frames on and either side of a block and of the largest side */
    static const int sides[] = {0, 1, 15, 16, 17, 3000, 4000, 16383, 16384, 16385};
    static const long n_ids[] = {-1, 0, 1, 3, 4, 5, 100000, 2147483647L, 2147483648L};
    for (size_t h = 0; h < COUNT(sides); ++h)
        for (size_t w = 0; w < COUNT(sides); ++w)
            for (size_t i = 0; i < COUNT(n_ids); ++i)
                for (int n = 0; n <= 432; n = n ? n * 432 : 1)
                    printf("stitch %d %d %d %ld : %zu\n", n, sides[h], sides[w], n_ids[i], kl_dense_stitch_scratch(n, sides[h], sides[w], n_ids[i]));
    return 0;
}
