/*
 * pos_resample.hip -- the position embedding of one patch grid resampled to another, so that the weights of a context made
 * at one resolution serve a context at another (vit_hip_create_at_resolution, include/ViT_opencl.h; the definition, in full,
 * is in include/kernelHandler.h at vh_launch_resample_pos_embed).  What torchvision's interpolate_embeddings, the Hugging
 * Face ViT's interpolate_pos_encoding and DINO do with torch.nn.functional.interpolate on the host.  No reference
 * counterpart (the reference runs 224 px only).
 *
 * pos_resample_kernel<NT> (NT taps per axis: 4 bicubic, 2 bilinear): a thread owns one output token and 4 consecutive
 * channels, consecutive lanes consecutive channels, so every tap is one coalesced float4 load per lane and the result one
 * float4 store.  A thread computes its own 2 NT tap indices and weights from (token, the four sizes) in float64 -- a few
 * dozen double operations next to NT^2 16-byte loads -- sums horizontally first, then vertically, in float64, taps
 * ascending, and rounds to fp32 once.  A channel's result depends on that channel's grid values and the four sizes only:
 * not on embed_dim, the lane, or the grid of the launch (a grid-stride loop over token x channel quads).  The class-token
 * rows in front (`prefix`) and equal grids are copied.  No LDS, no atomics.  The kernel is memory-bound and runs once per
 * derived context: 577 x 768 outputs read 16 taps of a 154 KB source that stays in L2.
 */
#include "kernelHandler.h"
#include "vit_kernels.h"

namespace {

constexpr int PR_THREADS = 256;
constexpr int PR_MAX_GRID = 512, PR_MAX_PREFIX = 8;
constexpr long PR_MAX_BLOCKS = 1L << 16;   /* of the grid-stride launch: 16 M threads cover every ViT grid in one pass */

constexpr double PR_A = -0.75;             /* the Keys kernel's constant */
__device__ __forceinline__ double pr_c1(double x) { return ((PR_A + 2.0) * x - (PR_A + 3.0)) * x * x + 1.0; }
__device__ __forceinline__ double pr_c2(double x) { return ((PR_A * x - 5.0 * PR_A) * x + 8.0 * PR_A) * x - 4.0 * PR_A; }

/* The NT taps of output index o along an axis of `in` samples resampled to `out`: source indices (clamped into the axis)
 * and weights, as include/kernelHandler.h states them. */
template <int NT>
__device__ __forceinline__ void pr_axis(int o, int in, int out, int align_corners, int (&idx)[NT], double (&w)[NT])
{
    double s;
    if (align_corners) {
        const double scale = out > 1 ? (double)(in - 1) / (double)(out - 1) : 0.0;
        s = (double)o * scale;
    } else {
        const double scale = (double)in / (double)out;
        s = ((double)o + 0.5) * scale - 0.5;
    }
    if constexpr (NT == 4) {
        const double f = floor(s), t = s - f;   /* s is not clamped: the taps are */
        const int i0 = (int)f;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            idx[k] = min(max(i0 - 1 + k, 0), in - 1);
        w[0] = pr_c2(t + 1.0);
        w[1] = pr_c1(t);
        w[2] = pr_c1(1.0 - t);
        w[3] = pr_c2(2.0 - t);
    } else {
        if (!align_corners)
            s = fmax(s, 0.0);
        idx[0] = min((int)s, in - 1);
        idx[1] = min(idx[0] + 1, in - 1);
        const double lambda = s - (double)idx[0];
        w[0] = 1.0 - lambda;
        w[1] = lambda;
    }
}

template <int NT>
__global__ __launch_bounds__(PR_THREADS) void pos_resample_kernel(const float4 *__restrict__ src, float4 *__restrict__ dst, int prefix,
                                                                   int in_h, int in_w, int out_h, int out_w, int E4,
                                                                   int align_corners, int copy, long total)
{
    const long step = (long)gridDim.x * PR_THREADS;
    for (long g = (long)blockIdx.x * PR_THREADS + threadIdx.x; g < total; g += step) {
        const long token = g / E4;
        const int c4 = (int)(g - token * E4);
        if (copy || token < prefix) {   /* equal grids, and the class-token rows: the same place in both, bit for bit */
            dst[g] = src[g];
            continue;
        }
        const int o = (int)(token - prefix), oy = o / out_w, ox = o - oy * out_w;
        int iy[NT], ix[NT];
        double wy[NT], wx[NT];
        pr_axis<NT>(oy, in_h, out_h, align_corners, iy, wy);
        pr_axis<NT>(ox, in_w, out_w, align_corners, ix, wx);
        double v[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const float4 *const row = src + ((size_t)prefix + (size_t)iy[j] * (size_t)in_w) * (size_t)E4 + (size_t)c4;
            double h[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const float4 p = row[(size_t)ix[i] * (size_t)E4];
                h[0] += wx[i] * (double)p.x;
                h[1] += wx[i] * (double)p.y;
                h[2] += wx[i] * (double)p.z;
                h[3] += wx[i] * (double)p.w;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                v[e] += wy[j] * h[e];
        }
        dst[g] = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
    }
}

} // namespace

extern "C" int vh_launch_resample_pos_embed(vh_stream_t s, const float *src, float *dst, int prefix, int in_h, int in_w, int out_h,
                                            int out_w, int embed_dim, int mode, int align_corners)
{
    const int E = embed_dim;
    if (!src || !dst)
        return vh_fail(1, "vh_launch_resample_pos_embed: null pointer argument (src, dst)");
    if (mode != VH_POS_BICUBIC && mode != VH_POS_BILINEAR)
        return vh_fail(1, "vh_launch_resample_pos_embed: mode=%d must be VH_POS_BICUBIC (0) or VH_POS_BILINEAR (1)", mode);
    if (align_corners != 0 && align_corners != 1)
        return vh_fail(1, "vh_launch_resample_pos_embed: align_corners=%d must be 0 or 1", align_corners);
    if (E < 4 || E % 4 != 0)
        return vh_fail(1, "vh_launch_resample_pos_embed: embed_dim=%d must be a multiple of 4, at least 4", E);
    if (in_h < 1 || in_w < 1 || out_h < 1 || out_w < 1 || in_h > PR_MAX_GRID || in_w > PR_MAX_GRID || out_h > PR_MAX_GRID ||
        out_w > PR_MAX_GRID)
        return vh_fail(1, "vh_launch_resample_pos_embed: grids %d x %d -> %d x %d: every side must be in 1..%d", in_h, in_w, out_h,
                       out_w, PR_MAX_GRID);
    if (prefix < 0 || prefix > PR_MAX_PREFIX)
        return vh_fail(1, "vh_launch_resample_pos_embed: prefix=%d must be in 0..%d", prefix, PR_MAX_PREFIX);
    if ((((uintptr_t)src | (uintptr_t)dst) & 15) != 0)
        return vh_fail(1, "vh_launch_resample_pos_embed: pointers must be 16-byte aligned");
    const size_t src_bytes = (size_t)(prefix + in_h * in_w) * (size_t)E * sizeof(float);
    const size_t dst_bytes = (size_t)(prefix + out_h * out_w) * (size_t)E * sizeof(float);
    if ((uintptr_t)src < (uintptr_t)dst + dst_bytes && (uintptr_t)dst < (uintptr_t)src + src_bytes)
        return vh_fail(1, "vh_launch_resample_pos_embed: src and dst must be distinct buffers that do not overlap");
    const int E4 = E / 4, copy = in_h == out_h && in_w == out_w;
    const long total = (long)(prefix + out_h * out_w) * (long)E4;
    const long want = (total + PR_THREADS - 1) / PR_THREADS;
    const unsigned blocks = (unsigned)(want < PR_MAX_BLOCKS ? want : PR_MAX_BLOCKS);
    hipStream_t st = (hipStream_t)s;
    if (mode == VH_POS_BICUBIC)
        hipLaunchKernelGGL(pos_resample_kernel<4>, dim3(blocks), dim3(PR_THREADS), 0, st, (const float4 *)src, (float4 *)dst, prefix, in_h,
                           in_w, out_h, out_w, E4, align_corners, copy, total);
    else
        hipLaunchKernelGGL(pos_resample_kernel<2>, dim3(blocks), dim3(PR_THREADS), 0, st, (const float4 *)src, (float4 *)dst, prefix, in_h,
                           in_w, out_h, out_w, E4, align_corners, copy, total);
    VH_LAUNCH_CHECK("pos_resample_kernel");
    return 0;
}
