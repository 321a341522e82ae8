/*
 * stitch_common.h -- what the two stitch kernels share (dense_stitch.hip: labels; dense_stitch_soft.hip: the soft maps):
 * the block and chunk constants, the 16-byte load at a 4-byte aligned address, the source coordinate of
 * include/kernelHandler.h's definition, and the launchers' host side -- the shape limits, the check of the boxes and of
 * every id of the block index, and the synchronous upload of both into the caller's scratch (kl_dense_stitch_scratch's
 * layout).  Stated once, so that the two launchers refuse the same arguments with the same words and the two kernels form
 * the same coordinates.  Included by those two .hip files only.
 */
#ifndef VIT_STITCH_COMMON_H
#define VIT_STITCH_COMMON_H

#include "kernelHandler.h"
#include "kernel_limits.h"
#include "vit_kernels.h"
#include "ViT_opencl.h"

namespace {

constexpr int ST_B = VH_STITCH_BLOCK, ST_THREADS = ST_B * ST_B;
constexpr int ST_CH = 16;                  /* classes per chunk */
constexpr unsigned ST_NAN = 0x7FC00000u;   /* how a NaN score, or an undefined pixel of a soft map, is written */
static_assert(ST_THREADS == 256, "a workgroup is four waves");

struct __attribute__((packed, aligned(4))) f32x4_a4 { float v[4]; };   /* 16 bytes at a 4-byte aligned address */

/* The source coordinate of the centre c (cx or cy) in a window side [lo, hi) over G patches (include/kernelHandler.h) */
__device__ __forceinline__ float st_src(float c, float lo, float hi, int G)
{
    const float side = hi - lo, ratio = (float)G / side, t = c - lo;
    return fmaxf(fmaf(t, ratio, -0.5f), 0.0f);
}

/* the limits on the shape of a launch */
inline int st_check_shape(const char *who, int n_windows, int grid_h, int grid_w, int n_labels, int frame_h, int frame_w)
{
    if (n_labels < 2 || n_labels > VH_DENSE_MAX_LABELS)
        return vh_fail(1, "%s: n_labels=%d must be in 2..%d", who, n_labels, VH_DENSE_MAX_LABELS);
    if (grid_h < 1 || grid_w < 1 || grid_h > VH_DENSE_MAX_GRID || grid_w > VH_DENSE_MAX_GRID)
        return vh_fail(1, "%s: grid %d x %d must be in 1..%d each way", who, grid_h, grid_w, VH_DENSE_MAX_GRID);
    if (frame_h < 1 || frame_w < 1 || frame_h > VH_STITCH_MAX_SIDE || frame_w > VH_STITCH_MAX_SIDE)
        return vh_fail(1, "%s: frame %d x %d must be in 1..%d each way", who, frame_h, frame_w, VH_STITCH_MAX_SIDE);
    if (n_windows < 1 || (long)n_windows * grid_h * grid_w >= 2147483647L - 128)
        return vh_fail(1, "%s: n_windows=%d must be positive, n_windows * grid_h * grid_w below 2^31 - 128", who, n_windows);
    return 0;
}

/* the boxes, and the index: every id the kernel will follow is looked at here.  -> blocks_x, blocks, n_ids */
inline int st_check_index(const char *who, int n_windows, const float *windows, int frame_h, int frame_w, const int *offsets, const int *ids,
                          int *blocks_x_out, long *blocks_out, long *n_ids_out)
{
    if (vit_stitch_check(frame_h, frame_w, windows, n_windows, who))
        return 1;
    const int blocks_x = (frame_w + ST_B - 1) / ST_B, blocks_y = (frame_h + ST_B - 1) / ST_B;
    const long blocks = (long)blocks_x * blocks_y;
    if (offsets[0] != 0)
        return vh_fail(1, "%s: offsets[0]=%d must be 0", who, offsets[0]);
    for (long k = 0; k < blocks; ++k)
        if (offsets[k + 1] < offsets[k])
            return vh_fail(1, "%s: offsets must not decrease (block %ld)", who, k);
    const long n_ids = offsets[blocks];
    if (n_ids > 0 && !ids)
        return vh_fail(1, "%s: null pointer argument (ids)", who);
    for (long k = 0; k < blocks; ++k)
        for (long j = offsets[k]; j < offsets[k + 1]; ++j)
            if (ids[j] < 0 || ids[j] >= n_windows || (j > offsets[k] && ids[j] <= ids[j - 1]))
                return vh_fail(1, "%s: the ids of block %ld must be strictly ascending window indices in 0..%d", who, k, n_windows - 1);
    *blocks_x_out = blocks_x;
    *blocks_out = blocks;
    *n_ids_out = n_ids;
    return 0;
}

/* where the three arrays lie in a scratch of kl_dense_stitch_scratch bytes */
struct st_index_dev { const float4 *boxes; const int *offsets, *ids; };

/* boxes, offsets and ids into d_scratch, with synchronous copies */
inline int st_upload_index(void *d_scratch, int n_windows, const float *windows, long blocks, const int *offsets, long n_ids, const int *ids,
                           st_index_dev *at)
{
    char *const d_boxes = (char *)d_scratch;
    char *const d_offsets = d_boxes + kl_round16((size_t)n_windows * 16);
    char *const d_ids = d_offsets + kl_round16((size_t)(blocks + 1) * sizeof(int));
    VH_TRY(hipMemcpy(d_boxes, windows, (size_t)n_windows * 16, hipMemcpyHostToDevice));
    VH_TRY(hipMemcpy(d_offsets, offsets, (size_t)(blocks + 1) * sizeof(int), hipMemcpyHostToDevice));
    if (n_ids > 0)
        VH_TRY(hipMemcpy(d_ids, ids, (size_t)n_ids * sizeof(int), hipMemcpyHostToDevice));
    at->boxes = (const float4 *)d_boxes;
    at->offsets = (const int *)d_offsets;
    at->ids = (const int *)d_ids;
    return 0;
}

} // namespace

#endif
