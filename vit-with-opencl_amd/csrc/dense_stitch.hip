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
#include "stitch_common.h"   /* the constants, st_src and the launcher's host side, shared with dense_stitch_soft.hip */

namespace {

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
    if (st_check_shape(who, n_windows, grid_h, grid_w, n_labels, frame_h, frame_w))
        return 1;
    if (fill_label < 0 || fill_label > 255)
        return vh_fail(1, "%s: fill_label=%d must be in 0..255", who, fill_label);
    int blocks_x;
    long blocks, n_ids;
    if (st_check_index(who, n_windows, windows, frame_h, frame_w, offsets, ids, &blocks_x, &blocks, &n_ids))
        return 1;
    const size_t need = kl_dense_stitch_scratch(n_windows, frame_h, frame_w, n_ids);
    if (scratch_bytes < need)
        return vh_fail(1, "%s: scratch_bytes=%zu, %zu needed (vh_dense_stitch_scratch)", who, scratch_bytes, need);
    if ((((uintptr_t)patch_logits | (uintptr_t)d_scratch | (uintptr_t)labels | (uintptr_t)scores | (uintptr_t)cover) & 15) != 0)
        return vh_fail(1, "%s: device pointers must be 16-byte aligned", who);
    hipStream_t st = (hipStream_t)s;
    st_index_dev ix;
    const int rc = st_upload_index(d_scratch, n_windows, windows, blocks, offsets, n_ids, ids, &ix);
    if (rc)
        return rc;
    hipLaunchKernelGGL(dense_stitch_kernel, dim3((unsigned)blocks), dim3(ST_THREADS), 0, st, patch_logits, ix.boxes, ix.offsets, ix.ids, grid_h,
                       grid_w, n_labels, frame_h, frame_w, blocks_x, fill_label, labels, scores, cover);
    VH_LAUNCH_CHECK("dense_stitch_kernel");
    return 0;
}
