/*
 * dense_coords.h -- the fp32 source coordinate of the dense head's upsampling (include/kernelHandler.h), its cell and the
 * band of output indices that share a cell, for the kernels that work per (image, patch row): dense_labels_kernel
 * (dense_head.hip) and dense_soft_kernel (dense_soft.hip).  Device code only; both kernels form the same bits from it.
 */
#ifndef VIT_DENSE_COORDS_H
#define VIT_DENSE_COORDS_H

/* The source coordinate of output index i (include/kernelHandler.h): ratio = fl(G / out) */
__device__ __forceinline__ float dh_src(int i, float ratio) { return fmaxf(fmaf((float)i + 0.5f, ratio, -0.5f), 0.0f); }
__device__ __forceinline__ int dh_cell(float s, int G)
{
    const int r = (int)s;
    return r < G - 1 ? r : G - 1;
}

/* the first output index whose cell is >= r (out when there is none): dh_cell(dh_src(.)) is non-decreasing */
__device__ __forceinline__ int dh_band_start(int r, float ratio, int G, int out)
{
    if (r <= 0)
        return 0;
    if (r >= G)
        return out;
    const float guess = ((float)r + 0.5f) * (float)out / (float)G - 0.5f;
    int y = guess < 0.0f ? 0 : guess > (float)out ? out : (int)guess;
    while (y > 0 && dh_cell(dh_src(y - 1, ratio), G) >= r)
        --y;
    while (y < out && dh_cell(dh_src(y, ratio), G) < r)
        ++y;
    return y;
}

#endif
