/*
 * dense_head.hip -- a label per pixel from the patch tokens: a linear head over every patch token, the C logits per patch
 * upsampled bilinearly to out_h x out_w, and the best label of every pixel (vit_hip_set_dense, include/ViT_opencl.h; the
 * definition, bit for bit, is in include/kernelHandler.h).  The linear-probe protocol of DINO / DINOv2 and what a trained
 * 1x1-conv head does, without the [n][T-1][E] tokens or the [n][C][H][W] logits ever existing.  No reference counterpart.
 *
 * dense_logits_kernel<CS>, one 256-thread workgroup per tile of 128 token rows (32 per wave) and 16 CS labels -- all C of
 * them, except that a launch of fewer token tiles than half the CUs (a small batch) gives a workgroup 64 labels:
 *   - gallery_scan_kernel's main loop (gallery.hip): stages of 32 columns of the token tile and of all weight rows go
 *     through registers into LDS, the next stage's global loads are issued before the current stage's matrix instructions
 *     and written behind them; ragged E, label rows >= C and token rows past the end are zeros on the way in, so padding
 *     (and what lies between strided rows) is never read;
 *   - a wave holds 32 tokens x 16 CS labels in 2 x CS accumulators of v_mfma_f32_16x16x4_f32, all independent (two even
 *     at C <= 16), so the instruction's 40-cycle dependent latency is covered at its 32-cycle issue rate;
 *   - the chain of a logit is the gallery score's: columns 32 at a time, in those 16 at a time, a 16-column piece through
 *     four instructions e = 0..3 which add columns c + 16 j + 4 g + e for g = 0..3 in that order; ONE fp32 fma chain from
 *     +0 whichever lane, wave, workgroup or CS it falls to.  The bias is one fp32 add behind it.
 * Token row m = image * patches + p lies at rows + image * image_stride + p * row_stride: the residual stream's patch
 * rows are read in place (class rows skipped by the strides), staged normalised tokens contiguously.
 *
 * dense_labels_kernel, one 256-thread workgroup per (image, patch row r): the band of output rows whose upper source row
 * is r (dh_src: non-decreasing in y, so a band is a range, found from the fp32 function itself; empty when downsampling
 * skips r).  Patch rows r and min(r + 1, GH - 1) x C go to LDS, label stride C | 1 (odd: the four or five patches a wave's
 * 64 columns touch fall on different banks).  A thread owns one output column: per class two horizontal lerps from four
 * LDS reads, then one vertical lerp and one ranking step per output row of the band, 16 rows at a time with the running
 * (best value, best label) of each row in registers -- 4 LDS reads per class and 16 rows, not per pixel.  Labels leave as
 * dwords packed across four lanes where the address is 4-byte aligned and all four columns exist, as bytes at a row's
 * ragged ends.  No atomics at all.
 */
#include "kernelHandler.h"
#include "kernel_limits.h"
#include "vit_kernels.h"
#include "dense_coords.h"
#include <type_traits>

namespace {

constexpr int DH_THREADS = 256;
constexpr int DH_TT = VH_DENSE_TOKEN_TILE;   /* token rows per tile: 32 per wave */
constexpr int DH_KC = 32;                  /* columns per stage */
constexpr int DH_LS = DH_KC + 4;           /* LDS row stride in floats, as gallery.hip's */
constexpr int DH_MAX_C = VH_DENSE_MAX_LABELS, DH_MAX_E = KL_DENSE_MAX_EMBED, DH_MAX_OUT = KL_DENSE_MAX_OUT;
constexpr int DH_T_PIECES = DH_TT * (DH_KC / 4) / DH_THREADS;   /* 4-column pieces of a token stage per thread */
constexpr int DH_CS_SMALL = 4;             /* 16-label tiles per workgroup when the token tiles are few */
constexpr int DH_RB = 16;                  /* output rows a thread carries at a time */
constexpr unsigned DH_NAN = 0x7FC00000u;   /* how a NaN score is written */

inline size_t dh_logits_lds(int cs) { return (size_t)(DH_TT + 16 * cs) * DH_LS * sizeof(float); }
inline size_t dh_labels_lds(int gw, int C) { return kl_dense_labels_lds(gw, C); }

template <int CS>
__global__ __launch_bounds__(DH_THREADS, 2) void dense_logits_kernel(const float *__restrict__ rows, long image_stride, long row_stride,
                                                                      unsigned n_rows, int patches, int E,
                                                                      const float *__restrict__ weight, long weight_stride,
                                                                      const float *__restrict__ bias, int C, float *__restrict__ out)
{
    constexpr int W_PIECES = (16 * CS * (DH_KC / 4) + DH_THREADS - 1) / DH_THREADS;
    extern __shared__ __attribute__((aligned(16))) float dh_lds[];
    float *const t_s = dh_lds, *const w_s = t_s + DH_TT * DH_LS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lg = lane >> 4;
    const unsigned m0 = blockIdx.x * (unsigned)DH_TT;
    const int c_base = blockIdx.y * 16 * CS;    /* this workgroup's first label */
    const int nkc = (E + DH_KC - 1) / DH_KC;

    /* where this thread's token pieces start: the row is the same in every stage */
    const float *t_src[DH_T_PIECES];
#pragma unroll
    for (int i = 0; i < DH_T_PIECES; ++i) {
        const unsigned m = m0 + (unsigned)((tid + i * DH_THREADS) >> 3);
        t_src[i] = m < n_rows ? rows + (size_t)(m / (unsigned)patches) * (size_t)image_stride + (size_t)(m % (unsigned)patches) * (size_t)row_stride
                              : nullptr;
    }

    f32x4 tp[DH_T_PIECES], wp[W_PIECES];
    int ld_kc = 0;
    auto stage_load = [&]() {
        const int col0 = ld_kc * DH_KC;
#pragma unroll
        for (int i = 0; i < DH_T_PIECES; ++i) {
            const int col = col0 + 4 * ((tid + i * DH_THREADS) & 7);
            tp[i] = t_src[i] && col < E ? *reinterpret_cast<const f32x4 *>(t_src[i] + col) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
#pragma unroll
        for (int i = 0; i < W_PIECES; ++i) {
            const int p = tid + i * DH_THREADS, col = col0 + 4 * (p & 7), c = c_base + (p >> 3);
            wp[i] = c < C && col < E ? *reinterpret_cast<const f32x4 *>(weight + (size_t)c * (size_t)weight_stride + col)
                                     : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
        ++ld_kc;
    };
    auto stage_store = [&]() {
#pragma unroll
        for (int i = 0; i < DH_T_PIECES; ++i) {
            const int p = tid + i * DH_THREADS;
            *reinterpret_cast<f32x4 *>(t_s + (p >> 3) * DH_LS + 4 * (p & 7)) = tp[i];
        }
#pragma unroll
        for (int i = 0; i < W_PIECES; ++i) {
            const int p = tid + i * DH_THREADS;
            if (p < 16 * CS * (DH_KC / 4))
                *reinterpret_cast<f32x4 *>(w_s + (p >> 3) * DH_LS + 4 * (p & 7)) = wp[i];
        }
    };

    f32x4 acc[2][CS];
#pragma unroll
    for (int ts = 0; ts < 2; ++ts)
#pragma unroll
        for (int cs = 0; cs < CS; ++cs)
            acc[ts][cs] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    stage_load();
    for (int kc = 0; kc < nkc; ++kc) {
        __syncthreads();                       /* the previous stage has been read; this stage's loads have landed */
        stage_store();
        lds_barrier();
        if (ld_kc < nkc)
            stage_load();                      /* in flight during the matrix instructions below */
        const float *const tr = t_s + (wave * 32 + l15) * DH_LS + 4 * lg, *const wr = w_s + l15 * DH_LS + 4 * lg;
#pragma unroll
        for (int j = 0; j < DH_KC / 16; ++j) {
            const f32x4 t0 = *reinterpret_cast<const f32x4 *>(tr + 16 * j);
            const f32x4 t1 = *reinterpret_cast<const f32x4 *>(tr + 16 * DH_LS + 16 * j);
#pragma unroll
            for (int cs = 0; cs < CS; ++cs) {
                const f32x4 wf = *reinterpret_cast<const f32x4 *>(wr + cs * 16 * DH_LS + 16 * j);
#pragma unroll
                for (int e = 0; e < 4; ++e) {   /* result [token 16 ts + 4 lg + r][label 16 cs + l15] */
                    acc[0][cs] = __builtin_amdgcn_mfma_f32_16x16x4f32(t0[e], wf[e], acc[0][cs], 0, 0, 0);
                    acc[1][cs] = __builtin_amdgcn_mfma_f32_16x16x4f32(t1[e], wf[e], acc[1][cs], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int cs = 0; cs < CS; ++cs) {
        const int c = c_base + 16 * cs + l15;
        if (c >= C)
            continue;
        const float b = bias ? bias[c] : 0.0f;
#pragma unroll
        for (int ts = 0; ts < 2; ++ts)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned m = m0 + (unsigned)(wave * 32 + 16 * ts + 4 * lg + r);
                if (m < n_rows)
                    out[(size_t)m * C + c] = bias ? acc[ts][cs][r] + b : acc[ts][cs][r];
            }
    }
}

/* dh_src, dh_cell, dh_band_start: dense_coords.h, shared with dense_soft.hip */

__global__ __launch_bounds__(DH_THREADS) void dense_labels_kernel(const float *__restrict__ logits, int GH, int GW, int C, int out_h,
                                                                 int out_w, unsigned char *__restrict__ labels, float *__restrict__ scores)
{
    extern __shared__ __attribute__((aligned(16))) float dl_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int img = blockIdx.x / GH, r = blockIdx.x % GH;
    const float ry = (float)GH / (float)out_h, rx = (float)GW / (float)out_w;
    const int y_lo = dh_band_start(r, ry, GH, out_h), y_hi = dh_band_start(r + 1, ry, GH, out_h);
    if (y_lo >= y_hi)
        return;
    const int CP = C | 1, r1 = r + 1 < GH ? r + 1 : GH - 1;
    float *const row0 = dl_lds, *const row1 = dl_lds + GW * CP;
    {
        const float *const g0 = logits + ((size_t)img * GH + r) * (size_t)GW * C;
        const float *const g1 = logits + ((size_t)img * GH + r1) * (size_t)GW * C;
        for (int i = tid; i < GW * C; i += DH_THREADS) {
            const int col = i / C, c = i - col * C;
            row0[col * CP + c] = g0[i];
            row1[col * CP + c] = g1[i];
        }
    }
    __syncthreads();

    for (int xb = 0; xb < out_w; xb += DH_THREADS) {   /* uniform: every lane takes part in the shuffles below */
        const int x = xb + tid;
        const bool live = x < out_w;
        const float sx = dh_src(live ? x : out_w - 1, rx);
        const int c0 = dh_cell(sx, GW), c1 = c0 + 1 < GW ? c0 + 1 : GW - 1;
        const float wx = sx - (float)c0, ux = 1.0f - wx;
        const float *const p00 = row0 + c0 * CP, *const p01 = row0 + c1 * CP, *const p10 = row1 + c0 * CP, *const p11 = row1 + c1 * CP;
        /* DH_RB output rows of the column: FULL, all of them, without a branch per row */
        auto chunk = [&](auto full, int y0, int cnt) {
            constexpr bool FULL = decltype(full)::value;
            float wy[DH_RB], uy[DH_RB], best[DH_RB];
            int lab[DH_RB];
#pragma unroll
            for (int k = 0; k < DH_RB; ++k) {
                wy[k] = dh_src(y0 + k, ry) - (float)r;
                uy[k] = 1.0f - wy[k];
                best[k] = -INFINITY;
                lab[k] = -1;
            }
            /* One compare per value: a value wins when it is GREATER than the best so far, so equal values (-0 == +0) keep
             * the lower label and a NaN never wins.  What this leaves without a label is a pixel of -inf and NaN alone,
             * settled below. */
#pragma unroll 2
            for (int c = 0; c < C; ++c) {
                const float top = fmaf(wx, p01[c], ux * p00[c]), bot = fmaf(wx, p11[c], ux * p10[c]);
#pragma unroll
                for (int k = 0; k < DH_RB; ++k) {
                    if (FULL || k < cnt) {
                        const float v = fmaf(wy[k], bot, uy[k] * top);
                        const bool up = v > best[k];
                        best[k] = up ? v : best[k];
                        lab[k] = up ? c : lab[k];
                    }
                }
            }
            bool open = false;
#pragma unroll
            for (int k = 0; k < DH_RB; ++k)
                open = open || ((FULL || k < cnt) && lab[k] < 0);
            if (open) {   /* rare: the first class that is a number (it is -inf) wins; NaN throughout: label 0, score NaN */
                for (int c = 0; c < C; ++c) {
                    const float top = fmaf(wx, p01[c], ux * p00[c]), bot = fmaf(wx, p11[c], ux * p10[c]);
#pragma unroll
                    for (int k = 0; k < DH_RB; ++k) {
                        const float v = fmaf(wy[k], bot, uy[k] * top);
                        if ((FULL || k < cnt) && lab[k] < 0 && v == v)
                            lab[k] = c;
                    }
                }
#pragma unroll
                for (int k = 0; k < DH_RB; ++k)
                    if ((FULL || k < cnt) && lab[k] < 0) {
                        lab[k] = 0;
                        best[k] = __builtin_bit_cast(float, DH_NAN);
                    }
            }
#pragma unroll
            for (int k = 0; k < DH_RB; ++k) {
                if (FULL || k < cnt) {
                    const size_t at = ((size_t)img * out_h + (size_t)(y0 + k)) * (size_t)out_w + (size_t)(live ? x : 0);
                    /* four lanes' bytes in one dword where its address is aligned and the four columns are in this wave */
                    const int l0 = lab[k], l1 = __shfl_down(l0, 1), l2 = __shfl_down(l0, 2), l3 = __shfl_down(l0, 3);
                    const int off = (int)(at & 3), first = lane - off;   /* the lane at the start of this lane's dword */
                    const bool whole = live && first >= 0 && first + 3 < 64 && x - off >= 0 && x - off + 3 < out_w;
                    if (whole) {
                        if (off == 0)
                            *reinterpret_cast<unsigned *>(labels + at) = (unsigned)l0 | (unsigned)l1 << 8 | (unsigned)l2 << 16 | (unsigned)l3 << 24;
                    } else if (live) {
                        labels[at] = (unsigned char)l0;
                    }
                    if (scores && live)
                        scores[at] = best[k];
                }
            }
        };
        for (int y0 = y_lo; y0 < y_hi; y0 += DH_RB) {
            if (y_hi - y0 >= DH_RB)
                chunk(std::true_type{}, y0, DH_RB);
            else
                chunk(std::false_type{}, y0, y_hi - y0);
        }
    }
}

template <int CS>
int launch_logits(hipStream_t st, const float *rows, long image_stride, long row_stride, unsigned n_rows, int patches, int E,
                  const float *weight, long weight_stride, const float *bias, int C, float *out)
{
    VH_SET_LDS_ONCE((dense_logits_kernel<CS>), dh_logits_lds(CS));
    const unsigned label_groups = (unsigned)(((C + 15) / 16 + CS - 1) / CS);
    hipLaunchKernelGGL((dense_logits_kernel<CS>), dim3((n_rows + DH_TT - 1) / DH_TT, label_groups), dim3(DH_THREADS), dh_logits_lds(CS), st, rows,
                       image_stride, row_stride, n_rows, patches, E, weight, weight_stride, bias, C, out);
    VH_LAUNCH_CHECK("dense_logits_kernel");
    return 0;
}

} // namespace

extern "C" int vh_launch_dense_logits(vh_stream_t s, const float *rows, long image_stride, long row_stride, int n_images, int patches,
                                      int embed_dim, const float *weight, long weight_stride, const float *bias, int n_labels,
                                      float *patch_logits)
{
    const int E = embed_dim, C = n_labels;
    if (!rows || !weight || !patch_logits)
        return vh_fail(1, "vh_launch_dense_logits: null pointer argument (rows, weight, patch_logits)");
    if (C < 2 || C > DH_MAX_C)
        return vh_fail(1, "vh_launch_dense_logits: n_labels=%d must be in 2..%d", C, DH_MAX_C);
    if (E < 4 || E > DH_MAX_E || E % 4 != 0)
        return vh_fail(1, "vh_launch_dense_logits: embed_dim=%d must be a multiple of 4 in 4..%d", E, DH_MAX_E);
    if (n_images < 1 || patches < 1 || (long)n_images * patches > 2147483647L - DH_TT)
        return vh_fail(1, "vh_launch_dense_logits: n_images=%d and patches=%d must be positive, their product below 2^31", n_images, patches);
    if (weight_stride < E || weight_stride % 4 != 0 || weight_stride > (1L << 40))
        return vh_fail(1, "vh_launch_dense_logits: weight_stride=%ld must be >= embed_dim=%d and a multiple of 4", weight_stride, E);
    if (row_stride < E || row_stride % 4 != 0 || row_stride > (1L << 40) || image_stride % 4 != 0 || image_stride > (1L << 40) ||
        image_stride < (long)patches * row_stride)
        return vh_fail(1, "vh_launch_dense_logits: row_stride=%ld must be >= embed_dim=%d, image_stride=%ld >= patches * row_stride, both multiples of 4",
                       row_stride, E, image_stride);
    if ((((uintptr_t)rows | (uintptr_t)weight | (uintptr_t)bias | (uintptr_t)patch_logits) & 15) != 0)
        return vh_fail(1, "vh_launch_dense_logits: pointers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)s;
    const unsigned n_rows = (unsigned)n_images * (unsigned)patches;
#define VH_DH_CASE(CS)                                                                                                          \
    case CS:                                                                                                                    \
        return launch_logits<CS>(st, rows, image_stride, row_stride, n_rows, patches, E, weight, weight_stride, bias, C, patch_logits)
    /* few token tiles (a small batch): workgroups of DH_CS_SMALL x 16 labels each, so that more CUs share the work; the
     * bits do not depend on it */
    int cs = (C + 15) / 16;
    if (cs > DH_CS_SMALL && 2 * ((n_rows + DH_TT - 1) / DH_TT) <= (unsigned)vh_device_cus(vh_current_device()))
        cs = DH_CS_SMALL;
    switch (cs) {
        VH_DH_CASE(1); VH_DH_CASE(2); VH_DH_CASE(3); VH_DH_CASE(4); VH_DH_CASE(5); VH_DH_CASE(6); VH_DH_CASE(7); VH_DH_CASE(8);
        VH_DH_CASE(9); VH_DH_CASE(10); VH_DH_CASE(11); VH_DH_CASE(12); VH_DH_CASE(13); VH_DH_CASE(14); VH_DH_CASE(15);
    default:
        return launch_logits<16>(st, rows, image_stride, row_stride, n_rows, patches, E, weight, weight_stride, bias, C, patch_logits);
    }
#undef VH_DH_CASE
}

extern "C" int vh_launch_dense_labels(vh_stream_t s, const float *patch_logits, int n_images, int grid_h, int grid_w, int n_labels,
                                      int out_h, int out_w, unsigned char *labels, float *scores)
{
    if (!patch_logits || !labels)
        return vh_fail(1, "vh_launch_dense_labels: null pointer argument (patch_logits, labels)");
    if (n_labels < 2 || n_labels > DH_MAX_C)
        return vh_fail(1, "vh_launch_dense_labels: n_labels=%d must be in 2..%d", n_labels, DH_MAX_C);
    if (grid_h < 1 || grid_w < 1 || grid_h > VH_DENSE_MAX_GRID || grid_w > VH_DENSE_MAX_GRID)
        return vh_fail(1, "vh_launch_dense_labels: grid %d x %d must be in 1..%d each way", grid_h, grid_w, VH_DENSE_MAX_GRID);
    if (out_h < 1 || out_w < 1 || out_h > DH_MAX_OUT || out_w > DH_MAX_OUT)
        return vh_fail(1, "vh_launch_dense_labels: output %d x %d must be in 1..%d each way", out_h, out_w, DH_MAX_OUT);
    if (n_images < 1 || (long)n_images * grid_h > 2147483647L)
        return vh_fail(1, "vh_launch_dense_labels: n_images=%d must be positive, n_images * grid_h below 2^31", n_images);
    if ((((uintptr_t)patch_logits | (uintptr_t)labels | (uintptr_t)scores) & 15) != 0)
        return vh_fail(1, "vh_launch_dense_labels: pointers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)s;
    VH_SET_LDS_ONCE(dense_labels_kernel, dh_labels_lds(VH_DENSE_MAX_GRID, DH_MAX_C));
    hipLaunchKernelGGL(dense_labels_kernel, dim3((unsigned)n_images * (unsigned)grid_h), dim3(DH_THREADS), dh_labels_lds(grid_w, n_labels), st,
                       patch_logits, grid_h, grid_w, n_labels, out_h, out_w, labels, scores);
    VH_LAUNCH_CHECK("dense_labels_kernel");
    return 0;
}
