/*
 * dense_stitch_soft.hip -- the soft maps of a whole frame: per frame pixel the softmax probability of the winning label, the
 * expected value over per-class values and the entropy, from the patch logits of overlapping windows blended in logit space
 * (the kernel under vit_hip_segment_frame_soft_u8, include/ViT_opencl.h; the definition, bit for bit, and its error bound are
 * in include/kernelHandler.h).  mmseg's mode="slide" followed by its softmax, as a gather: no [C][H][W] buffer, no atomics.
 *
 * dense_stitch_soft_kernel<EXPECT, ENTROPY, STASH>: dense_stitch_kernel's decomposition (dense_stitch.hip) -- one workgroup
 * of 256 threads per block of 16 x 16 frame pixels, a pixel per thread, the block's list walked wave-uniformly in ascending
 * window index, classes in chunks of 16 whose running sums stay in registers, corner logits as 16-byte global loads, one by
 * one in the ragged last chunk.  ss_blend is that kernel's chunk, expression for expression, up to the division: m[c].
 * The softmax needs M = max_c m[c] before its sums, hence two passes over the chunks:
 *   pass 1   M = fmaxf(M, m[c])                    c ascending; a NaN never becomes the maximum
 *   pass 2   t = k2 (m[c] - M), e = exp2(t), S += e, X = fma(e, values[c], X), A = fma(e, max(t, -FLT_MAX), A)
 * -- dense_soft_kernel's arithmetic (dense_soft.hip) on m for v.  What pass 2 reads is the STASH parameter:
 *   STASH = 0    recompute: pass 2 walks the list again and blends every chunk a second time.  Any C.
 *   STASH = N    pass 1 keeps the means of up to N chunks in 16 N registers, fully unrolled; pass 2 reads them.  C <= 16 N;
 *                built for N = 2, 4, 7 and 10, of which a launch takes the smallest that holds C.
 * Both form every number by the same operations in the same order: the same bits (tests/test_gpu_stitch_soft.py holds
 * each against the other).  Which one a launch takes depends on C alone (kl_dense_stitch_soft_variant, from measurements:
 * DESIGN.md 7, docs/LABBOOK.md, where the third variant that was built -- the means in LDS -- is recorded with its times).
 * values[c] is one address for the whole wave: a scalar load.  A NaN m[c] or a maximum of +-inf leaves S NaN, which one
 * compare at the end finds; a pixel no window covers is found by its count.  Only the sums whose maps are asked for are
 * carried.  Stores are one fp32 per lane and map, a row of 16 pixels consecutive.
 */
#include "stitch_common.h"
#include <cfloat>

namespace {

constexpr float SS_LOG2E = 1.44269504088896340736f, SS_LN2 = 0.69314718055994530942f;
static_assert(KL_STITCH_SOFT_CHUNK == ST_CH, "csrc/kernel_limits.h counts the register variant's chunks");

struct ss_pixel {
    const float *logits;
    const float4 *boxes;
    const int *ids;
    int k0, k1, GH, GW, C;
    size_t P;
    bool live;
    float cx, cy;
};

/* m[j] = the blended mean of class cb + j at the thread's pixel, j < 16: dense_stitch_kernel's chunk.  A class past C, and
 * every class of a pixel that nothing covers, is 0.  -> how many windows cover the pixel */
__device__ __forceinline__ int ss_blend(const ss_pixel &px, int cb, float (&m)[ST_CH])
{
    const int GH = px.GH, GW = px.GW, C = px.C;
    const bool whole = cb + ST_CH <= C;
    float acc[ST_CH];   /* the first window's value replaces, not joins, the zero: 0 + (-0) is not -0 */
#pragma unroll
    for (int j = 0; j < ST_CH; ++j)
        acc[j] = 0.0f;
    int cnt = 0;
    for (int k = px.k0; k < px.k1; ++k) {
        const int w = px.ids[k];
        const float4 box = px.boxes[w];   /* l, t, r, b */
        if (!(px.live && box.x <= px.cx && px.cx < box.z && box.y <= px.cy && px.cy < box.w))
            continue;
        const float sx = st_src(px.cx, box.x, box.z, GW), sy = st_src(px.cy, box.y, box.w, GH);
        const int c0 = min((int)sx, GW - 1), c1 = min(c0 + 1, GW - 1), r0 = min((int)sy, GH - 1), r1 = min(r0 + 1, GH - 1);
        const float wx = sx - (float)c0, ux = 1.0f - wx, wy = sy - (float)r0, uy = 1.0f - wy;
        const float *const base = px.logits + (size_t)w * px.P * C + cb;
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
    const float n = (float)(cnt > 0 ? cnt : 1);
#pragma unroll
    for (int j = 0; j < ST_CH; ++j)
        m[j] = acc[j] / n;
    return cnt;
}

template <bool EXPECT, bool ENTROPY>
struct ss_sums {
    float k2, M, S = 0.0f, X = 0.0f, A = 0.0f;
    /* the chunk's terms, c ascending */
    __device__ __forceinline__ void add(const float (&m)[ST_CH], int cb, int C, const float *__restrict__ values)
    {
#pragma unroll
        for (int j = 0; j < ST_CH; ++j) {
            if (cb + j < C) {
                const float t = k2 * (m[j] - M);
                const float e = __builtin_amdgcn_exp2f(t);
                S += e;
                if (EXPECT)
                    X = fmaf(e, values[cb + j], X);
                if (ENTROPY)
                    A = fmaf(e, fmaxf(t, -FLT_MAX), A);
            }
        }
    }
};

template <bool EXPECT, bool ENTROPY, int STASH>
__global__ __launch_bounds__(ST_THREADS) void dense_stitch_soft_kernel(const float *__restrict__ logits, const float4 *__restrict__ boxes,
                                                                      const int *__restrict__ offsets, const int *__restrict__ ids, int GH,
                                                                      int GW, int C, int frame_h, int frame_w, int blocks_x, float scale,
                                                                      const float *__restrict__ values, float *__restrict__ prob,
                                                                      float *__restrict__ expect, float *__restrict__ entropy)
{
    const int tid = threadIdx.x;
    const int bx = blockIdx.x % blocks_x, by = blockIdx.x / blocks_x;
    const int X = bx * ST_B + (tid & (ST_B - 1)), Y = by * ST_B + tid / ST_B;
    ss_pixel px;
    px.logits = logits;
    px.boxes = boxes;
    px.ids = ids;
    px.k0 = offsets[blockIdx.x];
    px.k1 = offsets[blockIdx.x + 1];
    px.GH = GH;
    px.GW = GW;
    px.C = C;
    px.P = (size_t)GH * GW;
    px.live = X < frame_w && Y < frame_h;
    px.cx = (float)X + 0.5f;
    px.cy = (float)Y + 0.5f;

    float M = -INFINITY;
    int count = 0;
    float keep[STASH > 0 ? STASH * ST_CH : 1];
    (void)keep;
    if constexpr (STASH > 0) {
#pragma unroll
        for (int ch = 0; ch < STASH; ++ch) {
            if (ch * ST_CH < C) {
                float m[ST_CH];
                count = ss_blend(px, ch * ST_CH, m);   /* the same in every chunk */
#pragma unroll
                for (int j = 0; j < ST_CH; ++j) {
                    keep[ch * ST_CH + j] = m[j];
                    if (ch * ST_CH + j < C)
                        M = fmaxf(M, m[j]);   /* a NaN never becomes the maximum */
                }
            }
        }
    } else {
        for (int cb = 0; cb < C; cb += ST_CH) {
            float m[ST_CH];
            count = ss_blend(px, cb, m);
#pragma unroll
            for (int j = 0; j < ST_CH; ++j)
                if (cb + j < C)
                    M = fmaxf(M, m[j]);
        }
    }

    ss_sums<EXPECT, ENTROPY> sum;
    sum.k2 = scale * SS_LOG2E;
    sum.M = M;
    if constexpr (STASH > 0) {
#pragma unroll
        for (int ch = 0; ch < STASH; ++ch) {
            if (ch * ST_CH < C) {
                float m[ST_CH];
#pragma unroll
                for (int j = 0; j < ST_CH; ++j)
                    m[j] = keep[ch * ST_CH + j];
                sum.add(m, ch * ST_CH, C, values);
            }
        }
    } else {
        for (int cb = 0; cb < C; cb += ST_CH) {
            float m[ST_CH];
            ss_blend(px, cb, m);
            sum.add(m, cb, C, values);
        }
    }

    if (!px.live)
        return;
    const size_t at = (size_t)Y * frame_w + X;
    const float nan = __builtin_bit_cast(float, ST_NAN);
    const float S = sum.S;
    const bool ok = count > 0 && S <= FLT_MAX;   /* S: false for the NaN that a NaN m[c] or an infinite maximum leaves */
    if (prob)
        prob[at] = ok ? 1.0f / S : nan;
    if (EXPECT)
        expect[at] = ok ? sum.X / S : nan;
    if (ENTROPY)
        entropy[at] = ok ? SS_LN2 * (__builtin_amdgcn_logf(S) - sum.A / S) : nan;
}

struct ss_args {
    hipStream_t st;
    const float *patch_logits;
    st_index_dev ix;
    int grid_h, grid_w, n_labels, frame_h, frame_w, blocks_x;
    long blocks;
    float logit_scale;
    const float *values;
    float *prob, *expect, *entropy;
};

template <bool EXPECT, bool ENTROPY, int STASH>
int ss_launch(const ss_args &a)
{
    hipLaunchKernelGGL((dense_stitch_soft_kernel<EXPECT, ENTROPY, STASH>), dim3((unsigned)a.blocks), dim3(ST_THREADS), 0, a.st, a.patch_logits,
                       a.ix.boxes, a.ix.offsets, a.ix.ids, a.grid_h, a.grid_w, a.n_labels, a.frame_h, a.frame_w, a.blocks_x, a.logit_scale, a.values,
                       a.prob, a.expect, a.entropy);
    VH_LAUNCH_CHECK("dense_stitch_soft_kernel");
    return 0;
}

template <bool EXPECT, bool ENTROPY>
int ss_launch_variant(const ss_args &a, int variant)
{
    if (variant == KL_STITCH_SOFT_RECOMPUTE)
        return ss_launch<EXPECT, ENTROPY, 0>(a);
    static_assert(KL_STITCH_SOFT_REG_MAX_LABELS == 10 * ST_CH, "the register variant is built for up to 10 chunks");
    const int chunks = kl_dense_stitch_soft_reg_chunks(a.n_labels);
    return chunks == 2 ? ss_launch<EXPECT, ENTROPY, 2>(a)
           : chunks == 4 ? ss_launch<EXPECT, ENTROPY, 4>(a)
           : chunks == 7 ? ss_launch<EXPECT, ENTROPY, 7>(a)
                         : ss_launch<EXPECT, ENTROPY, 10>(a);
}

} // namespace

extern "C" int vh_dense_stitch_soft_variant(int n_labels) { return kl_dense_stitch_soft_variant(n_labels); }

extern "C" int vh_launch_dense_stitch_soft(vh_stream_t s, const float *patch_logits, int n_windows, int grid_h, int grid_w, int n_labels,
                                           const float *windows, int frame_h, int frame_w, const int *offsets, const int *ids, void *d_scratch,
                                           size_t scratch_bytes, float logit_scale, const float *values, float *prob, float *expect,
                                           float *entropy)
{
    return vh_launch_dense_stitch_soft_as(0, s, patch_logits, n_windows, grid_h, grid_w, n_labels, windows, frame_h, frame_w, offsets, ids, d_scratch,
                                          scratch_bytes, logit_scale, values, prob, expect, entropy);
}

/* the launcher with the variant as an argument of the call (csrc/vit_kernels.h): 0 = by n_labels */
extern "C" int vh_launch_dense_stitch_soft_as(int as_variant, void *s, const float *patch_logits, int n_windows, int grid_h, int grid_w,
                                              int n_labels, const float *windows, int frame_h, int frame_w, const int *offsets, const int *ids,
                                              void *d_scratch, size_t scratch_bytes, float logit_scale, const float *values, float *prob,
                                              float *expect, float *entropy)
{
    static const char who[] = "vh_launch_dense_stitch_soft";
    if (!patch_logits || !windows || !offsets || !d_scratch)
        return vh_fail(1, "%s: null pointer argument (patch_logits, windows, offsets, d_scratch)", who);
    if (!prob && !expect && !entropy)
        return vh_fail(1, "%s: no output asked for (prob, expect, entropy are all NULL)", who);
    if ((values != NULL) != (expect != NULL))
        return vh_fail(1, "%s: values must be given exactly when expect is asked for", who);
    if (!(logit_scale > 0.0f) || !(logit_scale <= FLT_MAX))
        return vh_fail(1, "%s: logit_scale=%g must be finite and > 0", who, (double)logit_scale);
    if (st_check_shape(who, n_windows, grid_h, grid_w, n_labels, frame_h, frame_w))
        return 1;
    ss_args a;
    long n_ids;
    if (st_check_index(who, n_windows, windows, frame_h, frame_w, offsets, ids, &a.blocks_x, &a.blocks, &n_ids))
        return 1;
    const size_t need = kl_dense_stitch_scratch(n_windows, frame_h, frame_w, n_ids);
    if (scratch_bytes < need)
        return vh_fail(1, "%s: scratch_bytes=%zu, %zu needed (vh_dense_stitch_scratch)", who, scratch_bytes, need);
    if ((((uintptr_t)patch_logits | (uintptr_t)d_scratch | (uintptr_t)values | (uintptr_t)prob | (uintptr_t)expect | (uintptr_t)entropy) & 15) != 0)
        return vh_fail(1, "%s: device pointers must be 16-byte aligned", who);
    const int variant = as_variant ? as_variant : kl_dense_stitch_soft_variant(n_labels);
    if (!kl_dense_stitch_soft_variant_ok(variant, n_labels))
        return vh_fail(1, "%s: variant %d does not take n_labels=%d", who, variant, n_labels);
    const int rc = st_upload_index(d_scratch, n_windows, windows, a.blocks, offsets, n_ids, ids, &a.ix);
    if (rc)
        return rc;
    a.st = (hipStream_t)s;
    a.patch_logits = patch_logits;
    a.grid_h = grid_h;
    a.grid_w = grid_w;
    a.n_labels = n_labels;
    a.frame_h = frame_h;
    a.frame_w = frame_w;
    a.logit_scale = logit_scale;
    a.values = values;
    a.prob = prob;
    a.expect = expect;
    a.entropy = entropy;
    if (expect && entropy)
        return ss_launch_variant<true, true>(a, variant);
    if (expect)
        return ss_launch_variant<true, false>(a, variant);
    if (entropy)
        return ss_launch_variant<false, true>(a, variant);
    return ss_launch_variant<false, false>(a, variant);
}
