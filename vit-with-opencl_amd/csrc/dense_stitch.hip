/*
 * dense_stitch.hip -- one label per pixel of a frame from the patch logits of overlapping windows of it (the kernel under
 * vit_hip_segment_frame_u8, include/ViT_opencl.h; the definition, bit for bit, is in include/kernelHandler.h).  The slide
 * protocol of semantic segmentation as a gather: no [C][H][W] buffer, no atomics.
 *
 * dense_stitch_kernel, one workgroup of 256 threads per block of 16 x 16 frame pixels, one pixel per thread (a wave is four
 * rows of 16).  The block's windows come from the host's index (vit_stitch_index): offsets and ids are wave-uniform, so a
 * window's box is read once per wave.  Classes go in chunks of ST_CH = 16: the chunk's running sums stay in 16 registers; per
 * chunk the list is walked in ascending window index, a thread tests its own pixel against the box, forms the window's
 * coordinates (the header's expressions; recomputed per chunk, some 30 operations against the chunk's 112) and reads the
 * four corners' 16 logits as 16-byte loads from global memory -- 4-byte aligned only, which the global path takes -- or
 * one by one in the ragged last chunk, where the other form would read past a patch's classes.  The 16 pixels of a row
 * mostly share their corners (a 224 px window over 14 patches: all 16), so a wave's loads fall into a few cache lines.
 * After the chunk: one division, and the running best (value, label) by `greater than`, which leaves equal values to the
 * lower label and never lets a NaN win; the lowest label that is a number at all is kept beside it for the pixel whose
 * classes are all -inf or NaN.
 */
#include "kernelHandler.h"
#include "kernel_limits.h"
#include "vit_kernels.h"
#include "ViT_opencl.h"

namespace {

constexpr int ST_B = VH_STITCH_BLOCK, ST_THREADS = ST_B * ST_B;
constexpr int ST_CH = 16;                  /* classes per chunk */
constexpr unsigned ST_NAN = 0x7FC00000u;   /* how a NaN score is written */
static_assert(ST_THREADS == 256, "a workgroup is four waves");

struct __attribute__((packed, aligned(4))) f32x4_a4 { float v[4]; };   /* 16 bytes at a 4-byte aligned address */

/* The source coordinate of the centre c (cx or cy) in a window side [lo, hi) over G patches (include/kernelHandler.h) */
__device__ __forceinline__ float st_src(float c, float lo, float hi, int G)
{
    const float side = hi - lo, ratio = (float)G / side, t = c - lo;
    return fmaxf(fmaf(t, ratio, -0.5f), 0.0f);
}

__global__ __launch_bounds__(ST_THREADS) void dense_stitch_kernel(const float *__restrict__ logits, const float4 *__restrict__ boxes,
                                                                 const int *__restrict__ offsets, const int *__restrict__ ids, int GH, int GW,
                                                                 int C, int frame_h, int frame_w, int blocks_x, int fill,
                                                                 unsigned char *__restrict__ labels, float *__restrict__ scores,
                                                                 unsigned char *__restrict__ cover)
{
    const int tid = threadIdx.x;
    const int bx = blockIdx.x % blocks_x, by = blockIdx.x / blocks_x;
    const int X = bx * ST_B + (tid & (ST_B - 1)), Y = by * ST_B + tid / ST_B;
    const bool live = X < frame_w && Y < frame_h;
    const float cx = (float)X + 0.5f, cy = (float)Y + 0.5f;
    const int k0 = offsets[blockIdx.x], k1 = offsets[blockIdx.x + 1];
    const size_t P = (size_t)GH * GW;

    float best = -INFINITY;
    int lab = -1, first_number = -1, count = 0;
    for (int cb = 0; cb < C; cb += ST_CH) {
        const bool whole = cb + ST_CH <= C;
        float acc[ST_CH];   /* the first window's value replaces, not joins, the zero: 0 + (-0) is not -0 */
#pragma unroll
        for (int j = 0; j < ST_CH; ++j)
            acc[j] = 0.0f;
        int cnt = 0;
        for (int k = k0; k < k1; ++k) {
            const int w = ids[k];
            const float4 box = boxes[w];   /* l, t, r, b */
            if (!(live && box.x <= cx && cx < box.z && box.y <= cy && cy < box.w))
                continue;
            const float sx = st_src(cx, box.x, box.z, GW), sy = st_src(cy, box.y, box.w, GH);
            const int c0 = min((int)sx, GW - 1), c1 = min(c0 + 1, GW - 1), r0 = min((int)sy, GH - 1), r1 = min(r0 + 1, GH - 1);
            const float wx = sx - (float)c0, ux = 1.0f - wx, wy = sy - (float)r0, uy = 1.0f - wy;
            const float *const base = logits + (size_t)w * P * C + cb;
            const float *const p00 = base + ((size_t)r0 * GW + c0) * C, *const p01 = base + ((size_t)r0 * GW + c1) * C;
            const float *const p10 = base + ((size_t)r1 * GW + c0) * C, *const p11 = base + ((size_t)r1 * GW + c1) * C;
            float a00[ST_CH], a01[ST_CH], a10[ST_CH], a11[ST_CH];
            if (whole) {
#pragma unroll
                for (int q = 0; q < ST_CH / 4; ++q) {
                    const f32x4_a4 v00 = reinterpret_cast<const f32x4_a4 *>(p00)[q], v01 = reinterpret_cast<const f32x4_a4 *>(p01)[q];
                    const f32x4_a4 v10 = reinterpret_cast<const f32x4_a4 *>(p10)[q], v11 = reinterpret_cast<const f32x4_a4 *>(p11)[q];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        a00[4 * q + e] = v00.v[e];
                        a01[4 * q + e] = v01.v[e];
                        a10[4 * q + e] = v10.v[e];
                        a11[4 * q + e] = v11.v[e];
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < ST_CH; ++j) {
                    const bool in = cb + j < C;   /* nothing is read past a patch's C classes */
                    a00[j] = in ? p00[j] : 0.0f;
                    a01[j] = in ? p01[j] : 0.0f;
                    a10[j] = in ? p10[j] : 0.0f;
                    a11[j] = in ? p11[j] : 0.0f;
                }
            }
#pragma unroll
            for (int j = 0; j < ST_CH; ++j) {
                const float top = fmaf(wx, a01[j], ux * a00[j]), bot = fmaf(wx, a11[j], ux * a10[j]);
                const float v = fmaf(wy, bot, uy * top);
                acc[j] = cnt == 0 ? v : acc[j] + v;
            }
            ++cnt;
        }
        count = cnt;   /* the same in every chunk */
        if (cnt > 0) {
            const float n = (float)cnt;
#pragma unroll
            for (int j = 0; j < ST_CH; ++j) {
                if (cb + j < C) {
                    const float m = acc[j] / n;
                    const bool up = m > best;
                    best = up ? m : best;
                    lab = up ? cb + j : lab;
                    first_number = first_number < 0 && m == m ? cb + j : first_number;
                }
            }
        }
    }
    if (!live)
        return;
    const size_t at = (size_t)Y * frame_w + X;
    if (count == 0) {
        labels[at] = (unsigned char)fill;
        best = __builtin_bit_cast(float, ST_NAN);
    } else {
        if (lab < 0) {   /* -inf and NaN alone: the first class that is a number (it is -inf); NaN throughout: label 0, score NaN */
            lab = first_number < 0 ? 0 : first_number;
            best = first_number < 0 ? __builtin_bit_cast(float, ST_NAN) : -INFINITY;
        }
        labels[at] = (unsigned char)lab;
    }
    if (scores)
        scores[at] = best;
    if (cover)
        cover[at] = (unsigned char)(count < 255 ? count : 255);
}

} // namespace

extern "C" size_t vh_dense_stitch_scratch(int n_windows, int frame_h, int frame_w, long n_ids)
{
    return kl_dense_stitch_scratch(n_windows, frame_h, frame_w, n_ids);
}

extern "C" int vh_launch_dense_stitch(vh_stream_t s, const float *patch_logits, int n_windows, int grid_h, int grid_w, int n_labels,
                                      const float *windows, int frame_h, int frame_w, const int *offsets, const int *ids, int fill_label,
                                      void *d_scratch, size_t scratch_bytes, unsigned char *labels, float *scores, unsigned char *cover)
{
    static const char who[] = "vh_launch_dense_stitch";
    if (!patch_logits || !windows || !offsets || !d_scratch || !labels)
        return vh_fail(1, "%s: null pointer argument (patch_logits, windows, offsets, d_scratch, labels)", who);
    if (n_labels < 2 || n_labels > VH_DENSE_MAX_LABELS)
        return vh_fail(1, "%s: n_labels=%d must be in 2..%d", who, n_labels, VH_DENSE_MAX_LABELS);
    if (grid_h < 1 || grid_w < 1 || grid_h > VH_DENSE_MAX_GRID || grid_w > VH_DENSE_MAX_GRID)
        return vh_fail(1, "%s: grid %d x %d must be in 1..%d each way", who, grid_h, grid_w, VH_DENSE_MAX_GRID);
    if (frame_h < 1 || frame_w < 1 || frame_h > VH_STITCH_MAX_SIDE || frame_w > VH_STITCH_MAX_SIDE)
        return vh_fail(1, "%s: frame %d x %d must be in 1..%d each way", who, frame_h, frame_w, VH_STITCH_MAX_SIDE);
    if (n_windows < 1 || (long)n_windows * grid_h * grid_w >= 2147483647L - 128)
        return vh_fail(1, "%s: n_windows=%d must be positive, n_windows * grid_h * grid_w below 2^31 - 128", who, n_windows);
    if (fill_label < 0 || fill_label > 255)
        return vh_fail(1, "%s: fill_label=%d must be in 0..255", who, fill_label);
    if (vit_stitch_check(frame_h, frame_w, windows, n_windows, who))
        return 1;
    const int blocks_x = (frame_w + ST_B - 1) / ST_B, blocks_y = (frame_h + ST_B - 1) / ST_B;
    const long blocks = (long)blocks_x * blocks_y;
    /* the index: every id the kernel will follow is looked at here */
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
    const size_t need = kl_dense_stitch_scratch(n_windows, frame_h, frame_w, n_ids);
    if (scratch_bytes < need)
        return vh_fail(1, "%s: scratch_bytes=%zu, %zu needed (vh_dense_stitch_scratch)", who, scratch_bytes, need);
    if ((((uintptr_t)patch_logits | (uintptr_t)d_scratch | (uintptr_t)labels | (uintptr_t)scores | (uintptr_t)cover) & 15) != 0)
        return vh_fail(1, "%s: device pointers must be 16-byte aligned", who);
    hipStream_t st = (hipStream_t)s;
    char *const d_boxes = (char *)d_scratch;
    char *const d_offsets = d_boxes + kl_round16((size_t)n_windows * 16);
    char *const d_ids = d_offsets + kl_round16((size_t)(blocks + 1) * sizeof(int));
    VH_TRY(hipMemcpy(d_boxes, windows, (size_t)n_windows * 16, hipMemcpyHostToDevice));
    VH_TRY(hipMemcpy(d_offsets, offsets, (size_t)(blocks + 1) * sizeof(int), hipMemcpyHostToDevice));
    if (n_ids > 0)
        VH_TRY(hipMemcpy(d_ids, ids, (size_t)n_ids * sizeof(int), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(dense_stitch_kernel, dim3((unsigned)blocks), dim3(ST_THREADS), 0, st, patch_logits, (const float4 *)d_boxes,
                       (const int *)d_offsets, (const int *)d_ids, grid_h, grid_w, n_labels, frame_h, frame_w, blocks_x, fill_label, labels,
                       scores, cover);
    VH_LAUNCH_CHECK("dense_stitch_kernel");
    return 0;
}
