/*
 * dense_soft.hip -- the soft maps of the dense head: per pixel the softmax probability of the winning label, the expected
 * value of a caller's per-class values (depth by bins: sum_c p_c * centre_c) and the entropy, from the patch logits
 * vh_launch_dense_logits writes (vit_hip_set_dense_soft, include/ViT_opencl.h; the definition and its error bound are in
 * include/kernelHandler.h).  The [n][C][H][W] probabilities never exist.  No reference counterpart.
 *
 * dense_soft_kernel<EXPECT, ENTROPY>, dense_labels_kernel's decomposition (dense_head.hip): one 256-thread workgroup per
 * (image, patch row r) on the band of output rows whose upper source row is r (dense_coords.h), patch rows r and min(r + 1,
 * GH - 1) x C in LDS at label stride C | 1, a thread per output column, 16 output rows at a time in registers.  Two passes
 * over the classes per 16 rows, each forming v[c] by the header's three lerps (the two horizontal ones shared by the 16
 * rows: 4 LDS reads and 4 VALU per class and pass):
 *   pass 1   m = max_c v[c]                                                     v_mul, v_fma, v_max
 *   pass 2   t = k2 (v[c] - m), e = exp2(t), S += e                             v_mul, v_fma, v_sub, v_mul, v_exp, v_add
 *            EXPECT:  X = fma(e, values[c], X)    ENTROPY:  A = fma(e, max(t, -FLT_MAX), A)
 * k2 = s * log2(e) once per thread; values[c] is the same address in every lane, a scalar load.  A NaN v[c], or a maximum
 * of +-inf, makes t NaN for some class and with it S: no pass looks for special values, one compare on S at the end does.
 * The max in the ENTROPY term turns t = -inf (e = 0) into a finite number, so that the term is 0 and not 0 * inf; it would
 * drop a NaN, which S keeps.  Sums are sequential in c from 0: the order depends on nothing.  Only the sums whose maps are
 * asked for are carried (the template; prob costs nothing beyond S).  Stores are one fp32 per lane and row, consecutive
 * lanes consecutive addresses.  No atomics.
 */
#include "kernelHandler.h"
#include "kernel_limits.h"
#include "vit_kernels.h"
#include "dense_coords.h"
#include <cfloat>

namespace {

constexpr int DS_THREADS = 256;
constexpr int DS_RB = 16;                  /* output rows a thread carries at a time */
constexpr unsigned DS_NAN = 0x7FC00000u;   /* how an undefined pixel is written */
constexpr float DS_LOG2E = 1.44269504088896340736f, DS_LN2 = 0.69314718055994530942f;

template <bool EXPECT, bool ENTROPY>
__global__ __launch_bounds__(DS_THREADS) void dense_soft_kernel(const float *__restrict__ logits, int GH, int GW, int C, int out_h, int out_w,
                                                               float scale, const float *__restrict__ values, float *__restrict__ prob,
                                                               float *__restrict__ expect, float *__restrict__ entropy)
{
    extern __shared__ __attribute__((aligned(16))) float ds_lds[];
    const int tid = threadIdx.x;
    const int img = blockIdx.x / GH, r = blockIdx.x % GH;
    const float ry = (float)GH / (float)out_h, rx = (float)GW / (float)out_w;
    const int y_lo = dh_band_start(r, ry, GH, out_h), y_hi = dh_band_start(r + 1, ry, GH, out_h);
    if (y_lo >= y_hi)
        return;
    const int CP = kl_dense_label_stride(C), r1 = r + 1 < GH ? r + 1 : GH - 1;
    float *const row0 = ds_lds, *const row1 = ds_lds + GW * CP;
    {
        const float *const g0 = logits + ((size_t)img * GH + r) * (size_t)GW * C;
        const float *const g1 = logits + ((size_t)img * GH + r1) * (size_t)GW * C;
        for (int i = tid; i < GW * C; i += DS_THREADS) {
            const int col = i / C, c = i - col * C;
            row0[col * CP + c] = g0[i];
            row1[col * CP + c] = g1[i];
        }
    }
    __syncthreads();
    const float k2 = scale * DS_LOG2E;

    for (int xb = 0; xb < out_w; xb += DS_THREADS) {
        const int x = xb + tid;
        if (x >= out_w)
            break;                               /* nothing below is shared between lanes */
        const float sx = dh_src(x, rx);
        const int c0 = dh_cell(sx, GW), c1 = c0 + 1 < GW ? c0 + 1 : GW - 1;
        const float wx = sx - (float)c0, ux = 1.0f - wx;
        const float *const p00 = row0 + c0 * CP, *const p01 = row0 + c1 * CP, *const p10 = row1 + c0 * CP, *const p11 = row1 + c1 * CP;
        /* DS_RB output rows of the column at a time.  A chunk past the band's end computes all DS_RB rows (the rows beyond
         * it from coordinates that belong to no pixel) and stores the band's: no branch per row in the loops over the classes */
        for (int y0 = y_lo; y0 < y_hi; y0 += DS_RB) {
            const int cnt = y_hi - y0;
            float wy[DS_RB], uy[DS_RB], m[DS_RB], S[DS_RB], X[EXPECT ? DS_RB : 1], A[ENTROPY ? DS_RB : 1];
#pragma unroll
            for (int k = 0; k < DS_RB; ++k) {
                wy[k] = dh_src(y0 + k, ry) - (float)r;
                uy[k] = 1.0f - wy[k];
                m[k] = -INFINITY;
                S[k] = 0.0f;
                if (EXPECT)
                    X[k] = 0.0f;
                if (ENTROPY)
                    A[k] = 0.0f;
            }
#pragma unroll 2
            for (int c = 0; c < C; ++c) {
                const float top = fmaf(wx, p01[c], ux * p00[c]), bot = fmaf(wx, p11[c], ux * p10[c]);
#pragma unroll
                for (int k = 0; k < DS_RB; ++k)
                    m[k] = fmaxf(m[k], fmaf(wy[k], bot, uy[k] * top));   /* a NaN never becomes the maximum */
            }
#pragma unroll 2
            for (int c = 0; c < C; ++c) {
                const float top = fmaf(wx, p01[c], ux * p00[c]), bot = fmaf(wx, p11[c], ux * p10[c]);
                const float val = EXPECT ? values[c] : 0.0f;
#pragma unroll
                for (int k = 0; k < DS_RB; ++k) {
                    const float t = k2 * (fmaf(wy[k], bot, uy[k] * top) - m[k]);
                    const float e = __builtin_amdgcn_exp2f(t);
                    S[k] += e;
                    if (EXPECT)
                        X[k] = fmaf(e, val, X[k]);
                    if (ENTROPY)
                        A[k] = fmaf(e, fmaxf(t, -FLT_MAX), A[k]);
                }
            }
#pragma unroll
            for (int k = 0; k < DS_RB; ++k) {
                if (k < cnt) {
                    const size_t at = ((size_t)img * out_h + (size_t)(y0 + k)) * (size_t)out_w + (size_t)x;
                    const float nan = __builtin_bit_cast(float, DS_NAN);
                    const bool ok = S[k] <= FLT_MAX;   /* false for the NaN that a NaN v[c] or an infinite maximum leaves */
                    if (prob)
                        prob[at] = ok ? 1.0f / S[k] : nan;
                    if (EXPECT)
                        expect[at] = ok ? X[k] / S[k] : nan;
                    if (ENTROPY)
                        entropy[at] = ok ? DS_LN2 * (__builtin_amdgcn_logf(S[k]) - A[k] / S[k]) : nan;
                }
            }
        }
    }
}

template <bool EXPECT, bool ENTROPY>
int launch_soft(hipStream_t st, const float *patch_logits, int n_images, int grid_h, int grid_w, int n_labels, int out_h, int out_w,
                float logit_scale, const float *values, float *prob, float *expect, float *entropy)
{
    VH_SET_LDS_ONCE((dense_soft_kernel<EXPECT, ENTROPY>), kl_dense_labels_lds(VH_DENSE_MAX_GRID, VH_DENSE_MAX_LABELS));
    hipLaunchKernelGGL((dense_soft_kernel<EXPECT, ENTROPY>), dim3((unsigned)n_images * (unsigned)grid_h), dim3(DS_THREADS),
                       kl_dense_labels_lds(grid_w, n_labels), st, patch_logits, grid_h, grid_w, n_labels, out_h, out_w, logit_scale, values, prob,
                       expect, entropy);
    VH_LAUNCH_CHECK("dense_soft_kernel");
    return 0;
}

} // namespace

extern "C" int vh_launch_dense_soft(vh_stream_t s, const float *patch_logits, int n_images, int grid_h, int grid_w, int n_labels, int out_h,
                                    int out_w, float logit_scale, const float *values, float *prob, float *expect, float *entropy)
{
    if (!patch_logits)
        return vh_fail(1, "vh_launch_dense_soft: null pointer argument (patch_logits)");
    if (!prob && !expect && !entropy)
        return vh_fail(1, "vh_launch_dense_soft: no output asked for (prob, expect, entropy are all NULL)");
    if ((values != NULL) != (expect != NULL))
        return vh_fail(1, "vh_launch_dense_soft: values must be given exactly when expect is asked for");
    if (!(logit_scale > 0.0f) || !(logit_scale <= FLT_MAX))
        return vh_fail(1, "vh_launch_dense_soft: logit_scale=%g must be finite and > 0", (double)logit_scale);
    if (!kl_dense_pixel_shape_ok(n_images, grid_h, grid_w, n_labels, out_h, out_w))
        return vh_fail(1, "vh_launch_dense_soft: n_labels=%d must be in 2..%d, the grid %d x %d in 1..%d each way, the output %d x %d in 1..%d each "
                          "way, n_images=%d positive with n_images * grid_h below 2^31",
                       n_labels, VH_DENSE_MAX_LABELS, grid_h, grid_w, VH_DENSE_MAX_GRID, out_h, out_w, KL_DENSE_MAX_OUT, n_images);
    if ((((uintptr_t)patch_logits | (uintptr_t)values | (uintptr_t)prob | (uintptr_t)expect | (uintptr_t)entropy) & 15) != 0)
        return vh_fail(1, "vh_launch_dense_soft: pointers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)s;
#define VH_DS_CASE(EX, EN) \
    return launch_soft<EX, EN>(st, patch_logits, n_images, grid_h, grid_w, n_labels, out_h, out_w, logit_scale, values, prob, expect, entropy)
    if (expect && entropy)
        VH_DS_CASE(true, true);
    if (expect)
        VH_DS_CASE(true, false);
    if (entropy)
        VH_DS_CASE(false, true);
    VH_DS_CASE(false, false);
#undef VH_DS_CASE
}
