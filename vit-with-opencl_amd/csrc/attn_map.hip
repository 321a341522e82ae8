/*
 * attn_map.hip -- the class token's attention row, per head, read from a layer's Q|K|V buffer.
 *
 * For image i and head h:  s[t] = (q_cls . k_t) / sqrt(D),  heads[t] = exp(s[t] - max s) / sum_t exp(s[t] - max s),
 * mean[t] = (sum over h ascending of heads[h][t]) / H.  The attention kernels are not involved: every plan leaves the
 * projection's Q|K|V complete before its attention launch, and the class row of the attention matrix needs q_cls and
 * the K columns only -- one memory-bound pass over a third of the buffer.  No reference counterpart (multihead.cl:3
 * never exposes its probabilities).
 *
 * One 256-thread workgroup per (image, head).  q_cls is decoded once into LDS and from there into the registers of the
 * lanes that use it.  K is read in pieces of 16 bytes per part, LPK adjacent lanes on one key:
 *   fp32 rows          [rows][3E]            16 lanes x float4 = 256 contiguous bytes of a row, twice for D > 64
 *   three-part planes  [3E/32][3][rows][32]  4 lanes x 16 B = one 64-byte segment per part; 16 adjacent keys per wave are
 *   one-part fp16      [3E/32][rows][32]     16 adjacent segments.  A head that starts mid-chunk (head_dim 80, odd h)
 *                                            is a matter of piece indices: piece p of the head is piece (E + hD)/8 + p
 *                                            of the row, chunk = that / 4.
 * Nothing is sized by T.  Scores are formed 256 keys at a time through an LDS tile; thread j then owns keys j, j + 256,
 * ...: it parks their scores in its own elements of `heads`, and re-reads only what it wrote itself for the exponentials
 * and for the division.  When `heads` is not asked for, one workgroup per image walks the heads in ascending order,
 * forms every tile again instead of parking it (three passes over an image's K slice, which stays in L2), and keeps the
 * running sum over heads in its own elements of `mean`.  Both ways run the same instructions on the same values in the
 * same order, so `mean` has the same bits either way.  Sums over t: per thread ascending, wave butterfly, then
 * (w0 + w1) + (w2 + w3) -- a function of T alone.  No atomics.
 */
#include "kernelHandler.h"
#include "qkv_forms.h"
#include "vit_kernels.h"

namespace {

constexpr int AM_THREADS = 256;
/* AmForm<FORM> and load_piece<FORM>, the piece loaders per stored form: qkv_forms.h */

__device__ __forceinline__ float am_wave_max(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
        v = fmaxf(v, __shfl_xor(v, m));
    return v;
}

/* The scaled scores of keys [base, base + 256) of one image into tile[]: LPK lanes per key, each over its own pieces in
 * ascending order, then a butterfly over the LPK lanes (the same sum in each of them).  Entries of keys >= T are left
 * alone. */
template <int FORM>
__device__ __forceinline__ void score_tile(const char *__restrict__ qkv, size_t rows, int row_floats, size_t row0, int T, int kcol,
                                           int pieces, float scale, const float (*q)[AmForm<FORM>::PIECE], int base, float *tile)
{
    constexpr int PIECE = AmForm<FORM>::PIECE, LPK = AmForm<FORM>::LPK, MAXP = AmForm<FORM>::MAXP, KPP = AM_THREADS / LPK;
    const int sub = threadIdx.x % LPK, slot = threadIdx.x / LPK;
#pragma unroll 4
    for (int pass = 0; pass < LPK; ++pass) {
        const int t = base + pass * KPP + slot;
        float k[MAXP][PIECE];
#pragma unroll
        for (int m = 0; m < MAXP; ++m)
            if (t < T && sub + m * LPK < pieces)
                load_piece<FORM>(qkv, rows, row_floats, row0 + (size_t)t, kcol + (sub + m * LPK) * PIECE, k[m]);
        float dot = 0.0f;
#pragma unroll
        for (int m = 0; m < MAXP; ++m)
            if (t < T && sub + m * LPK < pieces) {
#pragma unroll
                for (int e = 0; e < PIECE; ++e)
                    dot += q[m][e] * k[m][e];
            }
#pragma unroll
        for (int m = LPK / 2; m >= 1; m >>= 1)
            dot += __shfl_xor(dot, m);
        if (sub == 0 && t < T)
            tile[pass * KPP + slot] = dot * scale;
    }
}

/* Workgroup b serves image b / groups, heads [(b % groups) * hpb, + hpb).  heads != NULL: hpb = 1, the rows go to `heads`
 * (and mean == NULL: cls_attn_mean_kernel follows).  heads == NULL: hpb = H, the mean over heads goes to `mean`. */
template <int FORM>
__global__ __launch_bounds__(AM_THREADS) void cls_attn_kernel(const char *__restrict__ qkv, int n_images, int T, int E, int H, int hpb,
                                                              float scale, int tap, int n_taps, float *heads, float *mean)
{
    constexpr int PIECE = AmForm<FORM>::PIECE, LPK = AmForm<FORM>::LPK, MAXP = AmForm<FORM>::MAXP;
    __shared__ float q_s[AM_MAX_HEAD_DIM];
    __shared__ float tile[AM_THREADS];
    __shared__ float red_max[AM_THREADS / 64], red_sum[AM_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int groups = H / hpb, img = blockIdx.x / groups, h_first = (blockIdx.x % groups) * hpb;
    const int D = E / H, pieces = D / PIECE;
    const size_t rows = (size_t)n_images * (size_t)T, row0 = (size_t)img * (size_t)T;
    const size_t slot = (size_t)img * n_taps + tap;
    float *const acc = mean ? mean + slot * (size_t)T : nullptr;
    const float n_heads = (float)H;

    for (int h = h_first; h < h_first + hpb; ++h) {
        float *const dst = heads ? heads + (slot * H + h) * (size_t)T : nullptr;
        /* q_cls of this head: decoded once into LDS, then each lane's own pieces into registers */
        if (tid < pieces) {
            float v[PIECE];
            load_piece<FORM>(qkv, rows, 3 * E, row0, h * D + tid * PIECE, v);
#pragma unroll
            for (int e = 0; e < PIECE; ++e)
                q_s[tid * PIECE + e] = v[e];
        }
        __syncthreads();
        float q[MAXP][PIECE];
#pragma unroll
        for (int m = 0; m < MAXP; ++m)
#pragma unroll
            for (int e = 0; e < PIECE; ++e)
                q[m][e] = (tid % LPK) + m * LPK < pieces ? q_s[((tid % LPK) + m * LPK) * PIECE + e] : 0.0f;
        const int kcol = E + h * D;

        /* scores and their maximum */
        float mx = -INFINITY;
        for (int base = 0; base < T; base += AM_THREADS) {
            score_tile<FORM>(qkv, rows, 3 * E, row0, T, kcol, pieces, scale, q, base, tile);
            __syncthreads();
            if (base + tid < T) {
                const float sc = tile[tid];
                if (dst)
                    dst[base + tid] = sc;
                mx = fmaxf(mx, sc);
            }
            __syncthreads();
        }
        mx = am_wave_max(mx);
        if (lane == 0)
            red_max[wave] = mx;
        __syncthreads();
        mx = fmaxf(fmaxf(red_max[0], red_max[1]), fmaxf(red_max[2], red_max[3]));

        /* the row sum */
        float sum = 0.0f;
        for (int base = 0; base < T; base += AM_THREADS) {
            if (!dst) {
                score_tile<FORM>(qkv, rows, 3 * E, row0, T, kcol, pieces, scale, q, base, tile);
                __syncthreads();
            }
            if (base + tid < T)
                sum += expf((dst ? dst[base + tid] : tile[tid]) - mx);
            if (!dst)
                __syncthreads();
        }
        sum = wave_sum(sum);
        if (lane == 0)
            red_sum[wave] = sum;
        __syncthreads();
        sum = (red_sum[0] + red_sum[1]) + (red_sum[2] + red_sum[3]);

        /* the probabilities; without `heads`, the running sum over heads stays in this thread's elements of `mean` */
        for (int base = 0; base < T; base += AM_THREADS) {
            if (!dst) {
                score_tile<FORM>(qkv, rows, 3 * E, row0, T, kcol, pieces, scale, q, base, tile);
                __syncthreads();
            }
            if (base + tid < T) {
                const float p = expf((dst ? dst[base + tid] : tile[tid]) - mx) / sum;
                if (dst)
                    dst[base + tid] = p;
                if (acc) {
                    const float a = h == 0 ? p : acc[base + tid] + p;
                    acc[base + tid] = h == H - 1 ? a / n_heads : a;
                }
            }
            if (!dst)
                __syncthreads();
        }
    }
}

/* mean[t] = (heads[0][t] + heads[1][t] + ... ascending) / H for one (image, tap): what cls_attn_kernel forms without `heads` */
__global__ __launch_bounds__(AM_THREADS) void cls_attn_mean_kernel(const float *__restrict__ heads, float *__restrict__ mean, int T, int H,
                                                                   int tiles, int tap, int n_taps)
{
    const int img = blockIdx.x / tiles, t = (blockIdx.x % tiles) * AM_THREADS + threadIdx.x;
    if (t >= T)
        return;
    const size_t slot = (size_t)img * n_taps + tap;
    const float *src = heads + slot * H * (size_t)T + t;
    float a = src[0];
    for (int h = 1; h < H; ++h)
        a += src[(size_t)h * T];
    mean[slot * (size_t)T + t] = a / (float)H;
}

template <int FORM>
int launch_cls_attn(hipStream_t st, const void *qkv, int n, int T, int E, int H, int tap, int n_taps, float *heads, float *mean)
{
    const float scale = 1.0f / sqrtf((float)(E / H));
    const int hpb = heads ? 1 : H;
    hipLaunchKernelGGL(cls_attn_kernel<FORM>, dim3((unsigned)((size_t)n * (H / hpb))), dim3(AM_THREADS), 0, st,
                       static_cast<const char *>(qkv), n, T, E, H, hpb, scale, tap, n_taps, heads, heads ? nullptr : mean);
    VH_LAUNCH_CHECK("cls_attn_kernel");
    if (heads && mean) {
        const int tiles = (T + AM_THREADS - 1) / AM_THREADS;
        hipLaunchKernelGGL(cls_attn_mean_kernel, dim3((unsigned)((size_t)n * tiles)), dim3(AM_THREADS), 0, st, heads, mean, T, H, tiles,
                           tap, n_taps);
        VH_LAUNCH_CHECK("cls_attn_mean_kernel");
    }
    return 0;
}

} // namespace

extern "C" int vh_cls_attention_head_dim_ok(int head_dim) { return kl_cls_attention_head_dim_ok(head_dim); }

extern "C" int vh_launch_cls_attention(vh_stream_t s, const void *qkv, int qkv_form, int n_images, int tokens, int embed_dim,
                                       int num_heads, int tap_index, int n_taps, float *heads, float *mean)
{
    if (!qkv || (!heads && !mean))
        return vh_fail(1, "vh_launch_cls_attention: null pointer argument (qkv, or both heads and mean)");
    if (qkv_form != VH_QKV_ROWS_F32 && qkv_form != VH_QKV_PLANES3 && qkv_form != VH_QKV_PLANES_F16)
        return vh_fail(1, "vh_launch_cls_attention: qkv_form=%d must be VH_QKV_ROWS_F32, VH_QKV_PLANES3 or VH_QKV_PLANES_F16", qkv_form);
    if (n_images <= 0 || tokens < 1 || num_heads <= 0 || embed_dim <= 0 || embed_dim % num_heads != 0)
        return vh_fail(1, "vh_launch_cls_attention: bad arguments (n=%d tokens=%d embed=%d heads=%d)", n_images, tokens, embed_dim,
                       num_heads);
    if (!kl_cls_attention_head_dim_ok(embed_dim / num_heads))
        return vh_fail(1, "vh_launch_cls_attention: head_dim=%d must be a multiple of 16, at most %d", embed_dim / num_heads,
                       KL_CLS_ATTN_MAX_HEAD_DIM);
    if (qkv_form != VH_QKV_ROWS_F32 && embed_dim % 32 != 0)
        return vh_fail(1, "vh_launch_cls_attention: embed_dim=%d: the planes forms need a multiple of 32", embed_dim);
    if ((((uintptr_t)qkv | (uintptr_t)heads | (uintptr_t)mean) & 15) != 0)
        return vh_fail(1, "vh_launch_cls_attention: pointers must be 16-byte aligned");
    if (n_taps < 1 || n_taps > 4 || tap_index < 0 || tap_index >= n_taps)
        return vh_fail(1, "vh_launch_cls_attention: tap_index=%d, n_taps=%d: need 0 <= tap_index < n_taps <= 4", tap_index, n_taps);
    const size_t tiles = ((size_t)tokens + AM_THREADS - 1) / AM_THREADS;
    if (((size_t)n_images * num_heads) >> 31 || ((size_t)n_images * tiles) >> 31 || ((size_t)n_images * tokens) >> 31)
        return vh_fail(1, "vh_launch_cls_attention: n=%d x tokens=%d x heads=%d too large for one launch", n_images, tokens, num_heads);
    hipStream_t st = (hipStream_t)s;
    switch (qkv_form) {
    case VH_QKV_ROWS_F32: return launch_cls_attn<VH_QKV_ROWS_F32>(st, qkv, n_images, tokens, embed_dim, num_heads, tap_index, n_taps, heads, mean);
    case VH_QKV_PLANES3: return launch_cls_attn<VH_QKV_PLANES3>(st, qkv, n_images, tokens, embed_dim, num_heads, tap_index, n_taps, heads, mean);
    default: return launch_cls_attn<VH_QKV_PLANES_F16>(st, qkv, n_images, tokens, embed_dim, num_heads, tap_index, n_taps, heads, mean);
    }
}
