/*
 * features.hip -- feature readout: class, pooled and patch-token embeddings taken from the fp32 residual stream behind
 * a chosen encoder layer (vit_hip_set_features, include/ViT_opencl.h).  No reference counterpart: the reference hands
 * back class probabilities only (ViT_seq.c:506-515).
 *
 * Per tap the residual stream is read once.  A wave owns a row and holds it in registers, exactly as layernorm_kernel
 * (rowops.hip) does: lane l owns the 16-byte chunks c * 64 + l, the two sums run per lane in chunk order and meet in
 * the wave_sum butterflies, var = sq / E - mean^2, eps added in double, (x - mean) * inv_std * g + b un-fused -- the
 * normalised values are bit-identical to vh_launch_layer_norm on the same rows.
 *
 *   readout_cls_kernel    the n class-token rows (strided, or compacted when the last layer ran class-only)
 *   readout_rows_kernel   32 patch rows of one image per workgroup (16 waves x 2 rows): tokens out (NLC straight from
 *                         registers, NCHW through an LDS transposition) and the rows' sum into a partial slab
 *   readout_pool_kernel   the partial sums of an image added in slab order, / (T - 1), optional L2 norm
 *
 * pooled is reproducible: which rows a wave, a workgroup and a slab entry hold follows from T alone, and every sum runs
 * in a fixed order (row w + row w + 16 in the wave, waves 0..15, slab entries 0..chunks-1); no atomics.
 */
#include "kernelHandler.h"
#include "kernel_limits.h"
#include "vit_kernels.h"
#include "fp32_split.h"

namespace {

constexpr int RD_WAVES = 16;              /* waves per workgroup of readout_rows_kernel */
constexpr int RD_ROWS = 2 * RD_WAVES;     /* patch rows per workgroup */
static_assert(RD_ROWS == KL_READOUT_ROWS, "csrc/kernel_limits.h restates the rows per workgroup");
constexpr int RD_TILE_STRIDE = 257;       /* dwords per row of the transposition tile: 256 columns + 1 */

/* The row in x[], normalised in place: the arithmetic and summation order of layernorm_kernel (rowops.hip) */
template <int NV, bool FULL>
__device__ __forceinline__ void normalise_row(f32x4 (&x)[NV], const float *__restrict__ gamma, const float *__restrict__ beta,
                                              int E, double eps, int lane)
{
    const int nvec = E >> 2;
    float sum = 0.0f, sq = 0.0f;
#pragma unroll
    for (int c = 0; c < NV; ++c) {
        if (FULL || c * 64 + lane < nvec) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sum += x[c][e];
                sq += x[c][e] * x[c][e];
            }
        }
    }
    sum = wave_sum(sum);
    sq = wave_sum(sq);
    const float mean = sum / (float)E;
    const float var = sq / (float)E - mean * mean;
    const float inv_std = 1.0f / sqrtf((float)((double)var + eps));
    const f32x4 *g4 = reinterpret_cast<const f32x4 *>(gamma);
    const f32x4 *b4 = reinterpret_cast<const f32x4 *>(beta);
#pragma unroll
    for (int c = 0; c < NV; ++c) {
        const int idx = c * 64 + lane;
        if (FULL || idx < nvec) {
            const f32x4 g = g4[idx], bb = b4[idx];
            f32x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                y[e] = (x[c][e] - mean) * inv_std * g[e] + bb[e];
            x[c] = y;
        }
    }
}

/* two bf16 values (round to nearest even) in one dword, the first in the low half */
__device__ __forceinline__ unsigned pack_bf16x2(float a, float b)
{
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    const bf16x2 p = {(__bf16)a, (__bf16)b};
    return __builtin_bit_cast(unsigned, p);
}

/* chunk idx of a vector of E values to dst (fp32: 16 bytes per lane, bf16: 8) */
__device__ __forceinline__ void store_chunk(void *dst, int idx, const f32x4 &v, int bf16)
{
    if (bf16)
        reinterpret_cast<uint2 *>(dst)[idx] = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
    else
        reinterpret_cast<f32x4 *>(dst)[idx] = v;
}

/* a whole vector held by the wave, optionally scaled to unit L2 norm first (a zero vector stays zero) */
template <int NV, bool FULL>
__device__ __forceinline__ void store_vector(void *dst, f32x4 (&v)[NV], int E, int l2, int bf16, int lane)
{
    const int nvec = E >> 2;
    if (l2) {
        float ss = 0.0f;
#pragma unroll
        for (int c = 0; c < NV; ++c)
            if (FULL || c * 64 + lane < nvec)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    ss += v[c][e] * v[c][e];
        ss = wave_sum(ss);
        const float norm = sqrtf(ss);
#pragma unroll
        for (int c = 0; c < NV; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                v[c][e] = norm > 0.0f ? v[c][e] / norm : 0.0f;
    }
#pragma unroll
    for (int c = 0; c < NV; ++c)
        if (FULL || c * 64 + lane < nvec)
            store_chunk(dst, c * 64 + lane, v[c], bf16);
}

/* One wave per image: class-token row i at rows + i * row_stride -> cls[(i * n_taps + tap)][E] */
template <int NV>
__global__ __launch_bounds__(256) void readout_cls_kernel(const float *__restrict__ rows, long row_stride,
                                                          const float *__restrict__ gamma, const float *__restrict__ beta,
                                                          double eps, int final_norm, int l2, int bf16, int n, int E, int tap,
                                                          int n_taps, void *__restrict__ cls)
{
    const int lane = threadIdx.x & 63;
    const int img = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (img >= n)
        return;
    const int nvec = E >> 2;
    const f32x4 *src = reinterpret_cast<const f32x4 *>(rows + (size_t)img * row_stride);
    f32x4 x[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c)
        x[c] = src[min(c * 64 + lane, nvec - 1)];
    if (final_norm)
        normalise_row<NV, false>(x, gamma, beta, E, eps, lane);
    char *dst = static_cast<char *>(cls) + ((size_t)img * n_taps + tap) * E * (bf16 ? 2 : 4);
    store_vector<NV, false>(dst, x, E, l2, bf16, lane);
}

/* Workgroup (chunk, image): patch rows p = 32 chunk + wave and + wave + 16 of the image (token row p + 1).
 * tokens NLC: [(img * n_taps + tap)][T-1][E], written from the registers.
 * tokens NCHW: [(img * n_taps + tap)][E][T-1]: per slice of 256 columns the 32 rows go through an LDS tile of
 *   RD_TILE_STRIDE dwords per row.  Write side: lane l holds columns 4 l .. 4 l + 3 and writes column 4 l + (k + l / 8) % 4
 *   in step k, so the 32 lanes of a half hit 32 different banks; read side: lanes run along the rows at one column, and
 *   the odd row stride puts them on different banks too.  Stores are contiguous along T-1 (128 bytes per half wave in
 *   fp32; bf16 packs two rows per dword when T-1 is even).
 * partial (pooled): [img][chunks][E], the sum of the workgroup's rows. */
template <int NV, bool FULL>
__global__ __launch_bounds__(64 * RD_WAVES) void readout_rows_kernel(const float *__restrict__ x_rows,
                                                                    const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                    double eps, int final_norm, int bf16, int nchw, int T, int E,
                                                                    int tap, int n_taps, int chunks, void *__restrict__ tokens,
                                                                    float *__restrict__ partial)
{
    extern __shared__ __attribute__((aligned(16))) float rd_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int img = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    const int P = T - 1, nvec = E >> 2, p0 = chunk * RD_ROWS;
    const size_t esz = bf16 ? 2 : 4;

    f32x4 xr[2][NV];
    bool valid[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int p = p0 + wave + RD_WAVES * j;
        valid[j] = p < P;
        const f32x4 *src = reinterpret_cast<const f32x4 *>(x_rows + ((size_t)img * T + 1 + min(p, P - 1)) * E);
#pragma unroll
        for (int c = 0; c < NV; ++c)
            xr[j][c] = src[FULL ? c * 64 + lane : min(c * 64 + lane, nvec - 1)];
    }
    if (final_norm) {
        normalise_row<NV, FULL>(xr[0], gamma, beta, E, eps, lane);
        normalise_row<NV, FULL>(xr[1], gamma, beta, E, eps, lane);
    }

    if (tokens && !nchw) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (!valid[j])
                continue;
            char *dst = static_cast<char *>(tokens) + (((size_t)img * n_taps + tap) * P + (p0 + wave + RD_WAVES * j)) * E * esz;
#pragma unroll
            for (int c = 0; c < NV; ++c)
                if (FULL || c * 64 + lane < nvec)
                    store_chunk(dst, c * 64 + lane, xr[j][c], bf16);
        }
    }

    if (tokens && nchw) {
        char *map = static_cast<char *>(tokens) + ((size_t)img * n_taps + tap) * E * P * esz;
        const int rot = lane >> 3;
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            const int e0 = c * 256;   /* first column of the slice */
            if (e0 < E) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    float *trow = rd_lds + (wave + RD_WAVES * j) * RD_TILE_STRIDE + 4 * lane;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int kk = (k + rot) & 3;
                        const f32x4 v = xr[j][c];
                        trow[kk] = kk == 0 ? v[0] : kk == 1 ? v[1] : kk == 2 ? v[2] : v[3];
                    }
                }
            }
            __syncthreads();
            if (e0 < E) {
                const int cols = min(256, E - e0);
                if (bf16 && !(P & 1)) {   /* two rows per dword: p0 and P even, so the dword is aligned */
                    const int r = 2 * (threadIdx.x & 15);
                    if (p0 + r < P)
                        for (int col = threadIdx.x >> 4; col < cols; col += 64) {
                            const unsigned v = pack_bf16x2(rd_lds[r * RD_TILE_STRIDE + col], rd_lds[(r + 1) * RD_TILE_STRIDE + col]);
                            *reinterpret_cast<unsigned *>(map + ((size_t)(e0 + col) * P + p0 + r) * 2) = v;
                        }
                } else {
                    const int r = threadIdx.x & 31;
                    if (p0 + r < P)
                        for (int col = threadIdx.x >> 5; col < cols; col += 32) {
                            const float v = rd_lds[r * RD_TILE_STRIDE + col];
                            const size_t at = (size_t)(e0 + col) * P + p0 + r;
                            if (bf16)
                                reinterpret_cast<__bf16 *>(map)[at] = (__bf16)v;
                            else
                                reinterpret_cast<float *>(map)[at] = v;
                        }
                }
            }
            __syncthreads();
        }
    }

    if (partial) {
        /* row w + row w + 16 in the wave, then the 16 waves in order */
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            if (FULL || c * 64 + lane < nvec) {
                f32x4 a = valid[0] ? xr[0][c] : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                if (valid[1])
                    a += xr[1][c];
                reinterpret_cast<f32x4 *>(rd_lds + (size_t)wave * E)[c * 64 + lane] = a;
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < nvec) {
            f32x4 a = reinterpret_cast<const f32x4 *>(rd_lds)[threadIdx.x];
#pragma unroll
            for (int w = 1; w < RD_WAVES; ++w)
                a += reinterpret_cast<const f32x4 *>(rd_lds + (size_t)w * E)[threadIdx.x];
            reinterpret_cast<f32x4 *>(partial + ((size_t)img * chunks + chunk) * E)[threadIdx.x] = a;
        }
    }
}

/* One wave per image: pooled[(img * n_taps + tap)][E] = (partial[img][0] + ... + partial[img][chunks-1]) / (T - 1) */
template <int NV>
__global__ __launch_bounds__(256) void readout_pool_kernel(const float *__restrict__ partial, int chunks, int P, int l2, int bf16,
                                                           int n, int E, int tap, int n_taps, void *__restrict__ pooled)
{
    const int lane = threadIdx.x & 63;
    const int img = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (img >= n)
        return;
    const int nvec = E >> 2;
    const f32x4 *src = reinterpret_cast<const f32x4 *>(partial + (size_t)img * chunks * E);
    f32x4 v[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) {
        const int idx = min(c * 64 + lane, nvec - 1);
        f32x4 a = src[idx];
        for (int ch = 1; ch < chunks; ++ch)
            a += src[(size_t)ch * nvec + idx];
        v[c] = a / (float)P;
    }
    char *dst = static_cast<char *>(pooled) + ((size_t)img * n_taps + tap) * E * (bf16 ? 2 : 4);
    store_vector<NV, false>(dst, v, E, l2, bf16, lane);
}

} // namespace

extern "C" size_t vh_feature_readout_scratch(int n_images, int tokens, int embed_dim)
{
    return kl_feature_readout_scratch(n_images, tokens, embed_dim);
}

extern "C" int vh_launch_feature_readout(vh_stream_t s, const float *x, const float *cls_rows, long cls_row_stride,
                                         const float *gamma, const float *beta, double eps, int final_norm, int l2_normalize,
                                         int dtype, int token_layout, int n_images, int tokens_per_image, int embed_dim,
                                         int tap_index, int n_taps, void *cls, void *pooled, void *tokens, void *scratch,
                                         size_t scratch_bytes)
{
    const int n = n_images, T = tokens_per_image, E = embed_dim;
    if (!cls && !pooled && !tokens)
        return vh_fail(1, "vh_launch_feature_readout: no output buffer");
    if ((final_norm && (!gamma || !beta)) || ((pooled || tokens) && !x) || (cls && !x && !cls_rows))
        return vh_fail(1, "vh_launch_feature_readout: null pointer argument");
    if (n <= 0 || T <= 0 || E <= 0 || E % 4 != 0 || E > 2048)
        return vh_fail(1, "vh_launch_feature_readout: embed_dim=%d must be a multiple of 4, <= 2048 (n=%d, tokens=%d)", E, n, T);
    if ((dtype != 0 && dtype != 1) || (token_layout != 0 && token_layout != 1) || n_taps < 1 || n_taps > 4 || tap_index < 0 ||
        tap_index >= n_taps)
        return vh_fail(1, "vh_launch_feature_readout: dtype %d, token_layout %d or tap %d of %d out of range", dtype, token_layout,
                       tap_index, n_taps);
    if ((pooled || tokens) && T < 2)
        return vh_fail(1, "vh_launch_feature_readout: pooled / tokens need at least one patch token");
    if (cls_rows && (cls_row_stride % 4 != 0 || cls_row_stride < E))
        return vh_fail(1, "vh_launch_feature_readout: class-row stride must be a multiple of 4 floats and >= embed_dim");
    if ((((uintptr_t)x | (uintptr_t)cls_rows | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)cls | (uintptr_t)pooled |
          (uintptr_t)tokens | (uintptr_t)scratch) & 15))
        return vh_fail(1, "vh_launch_feature_readout: pointers must be 16-byte aligned");
    const int chunks = T >= 2 ? (T - 1 + RD_ROWS - 1) / RD_ROWS : 0;
    if ((size_t)n * (size_t)(chunks > 0 ? chunks : 1) > 0x7fffffffull)
        return vh_fail(1, "vh_launch_feature_readout: too many images");
    if (pooled && (!scratch || scratch_bytes < kl_feature_readout_scratch(n, T, E)))
        return vh_fail(1, "vh_launch_feature_readout: pooled needs %zu bytes of scratch", kl_feature_readout_scratch(n, T, E));
    hipStream_t st = (hipStream_t)s;
    const int nv = (E / 4 + 63) / 64, bf16 = dtype == 1;

    if (cls) {
        const float *rows = cls_rows ? cls_rows : x;
        const long stride = cls_rows ? cls_row_stride : (long)T * E;
        const dim3 grid((n + 3) / 4), block(256);
#define VH_RD_CLS(NV)                                                                                              \
    hipLaunchKernelGGL((readout_cls_kernel<NV>), grid, block, 0, st, rows, stride, gamma, beta, eps, final_norm,   \
                       l2_normalize, bf16, n, E, tap_index, n_taps, cls)
        if (nv <= 3) VH_RD_CLS(3);
        else if (nv <= 4) VH_RD_CLS(4);
        else if (nv <= 5) VH_RD_CLS(5);
        else VH_RD_CLS(8);
#undef VH_RD_CLS
        VH_LAUNCH_CHECK("readout_cls_kernel");
    }
    if (pooled || tokens) {
        const size_t tile = tokens && token_layout == 1 ? (size_t)RD_ROWS * RD_TILE_STRIDE * sizeof(float) : 0;
        const size_t sums = pooled ? (size_t)RD_WAVES * E * sizeof(float) : 0;
        const size_t lds = tile > sums ? tile : sums;
        const dim3 grid((unsigned)(n * chunks)), block(64 * RD_WAVES);
        float *partial = pooled ? static_cast<float *>(scratch) : nullptr;
#define VH_RD_ROWS_F(NV, FULL)                                                                                     \
    do {                                                                                                           \
        VH_SET_LDS_ONCE((readout_rows_kernel<NV, FULL>), KL_LDS_BYTES);                                            \
        hipLaunchKernelGGL((readout_rows_kernel<NV, FULL>), grid, block, lds, st, x, gamma, beta, eps, final_norm, \
                           bf16, token_layout, T, E, tap_index, n_taps, chunks, tokens, partial);                  \
    } while (0)
#define VH_RD_ROWS(NV)                                                                                             \
    do {                                                                                                           \
        if (E == 256 * (NV))                                                                                       \
            VH_RD_ROWS_F(NV, true);                                                                                \
        else                                                                                                       \
            VH_RD_ROWS_F(NV, false);                                                                               \
    } while (0)
        if (nv <= 3) VH_RD_ROWS(3);
        else if (nv <= 4) VH_RD_ROWS(4);
        else if (nv <= 5) VH_RD_ROWS(5);
        else VH_RD_ROWS(8);
#undef VH_RD_ROWS
#undef VH_RD_ROWS_F
        VH_LAUNCH_CHECK("readout_rows_kernel");
    }
    if (pooled) {
        const dim3 grid((n + 3) / 4), block(256);
#define VH_RD_POOL(NV)                                                                                             \
    hipLaunchKernelGGL((readout_pool_kernel<NV>), grid, block, 0, st, static_cast<const float *>(scratch), chunks, \
                       T - 1, l2_normalize, bf16, n, E, tap_index, n_taps, pooled)
        if (nv <= 3) VH_RD_POOL(3);
        else if (nv <= 4) VH_RD_POOL(4);
        else if (nv <= 5) VH_RD_POOL(5);
        else VH_RD_POOL(8);
#undef VH_RD_POOL
        VH_LAUNCH_CHECK("readout_pool_kernel");
    }
    return 0;
}
