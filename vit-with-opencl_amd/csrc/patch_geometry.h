/*
 * patch_geometry.h -- the host arithmetic of the fp32-rows patch embedding on an img_h x img_w image: which geometries the
 * GEMM gathers on load, and the workspace of the others.  Shared by csrc/gemm_mfma.hip (the launchers) and csrc/vit_plan.c
 * (the arena), so that the plan sizes a rectangular context without a symbol of the shim.  Plain C, no device.
 */
#ifndef VIT_PATCH_GEOMETRY_H
#define VIT_PATCH_GEOMETRY_H

#include <stddef.h>

enum { VH_PATCH_ROWS_K_STEP = 32 };   /* the K step of the fp32-rows GEMM (BK, csrc/gemm_common.h) */

/* im2row on load: four consecutive kw are one aligned 16-byte read of an image row */
static inline int vh_patch_direct_hw(int in_chans, int img_w, int patch_size)
{
    return patch_size % 4 == 0 && (in_chans * patch_size * patch_size) % VH_PATCH_ROWS_K_STEP == 0 && img_w % 4 == 0;
}

/* bytes of the gathered, zero-padded patch rows and the padded weights; 0 where the GEMM gathers on load */
static inline size_t vh_patch_rows_workspace_hw(int n_images, int in_chans, int img_h, int img_w, int patch_size, int embed_dim)
{
    if (n_images <= 0 || in_chans <= 0 || img_h <= 0 || img_w <= 0 || patch_size <= 0 || embed_dim <= 0 ||
        img_h % patch_size != 0 || img_w % patch_size != 0 || vh_patch_direct_hw(in_chans, img_w, patch_size))
        return 0;
    const size_t np = (size_t)(img_h / patch_size) * (size_t)(img_w / patch_size), K = (size_t)in_chans * patch_size * patch_size;
    const size_t Kp = (K + VH_PATCH_ROWS_K_STEP - 1) / VH_PATCH_ROWS_K_STEP * VH_PATCH_ROWS_K_STEP;
    return ((size_t)n_images * np + (size_t)embed_dim) * Kp * sizeof(float);
}

#endif
