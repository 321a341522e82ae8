/*
 * rollout.hip -- attention rollout (Abnar & Zuidema, 2020): the head-mean attention matrix of a layer, read from its
 * Q|K|V buffer, folded into a running T x T product per image.  include/ViT_opencl.h states the definition:
 *
 *   s_h[u][t] = (q_u . k_t) / sqrt(D)        P_h = row softmax of s_h        A = (sum over h ascending of P_h) / H
 *   first step:  R_next = 0.5 A + 0.5 I      later steps:  R_next = 0.5 (A . R_prev) + 0.5 R_prev
 *
 * The attention kernels are not involved; like attn_map.hip this reads what the QKV projection has just completed, in the
 * form the plan made it write (qkv_forms.h).  No reference counterpart (multihead.cl:3 never exposes its probabilities).
 *
 * rollout_attn_kernel, one 256-thread workgroup per (image, 16 query rows), heads in ascending order:
 *   - the head's 16 query rows are decoded to fp32 in LDS once and held as v_mfma_f32_16x16x4_f32 A operands in registers;
 *   - K streams through LDS 64 keys at a time, 16 keys per wave; one float4 LDS read feeds four matrix instructions (k-step
 *     (j, e) sums columns 16 j + 4 g + e, g = 0..3, of both operands: every column once, in an order fixed by D), two
 *     accumulators per wave (even and odd j) so that the instruction's dependent latency is covered;
 *   - the scaled scores of the head land in the one T-sized array, [16][T] in LDS (88 KB at T = 1370); 16 lanes per row
 *     then take the row's maximum, the exponentials and their sum (lane c owns keys c, c + 16, ...; a 16-lane butterfly:
 *     orders fixed by T alone), and add exp / sum to the running sum over heads, which each lane keeps in its own elements
 *     of the output and divides by H behind the last head.
 *   On the first step the mix with the identity is applied there and the rows go straight to R_next.
 * rollout_product_kernel, one workgroup per (image, 64 x 64 tile of R_next): A and R_prev stream through LDS 16 columns /
 *   rows at a time, each wave owns 16 rows x 64 columns (four independent accumulators) on the same matrix instruction,
 *   zero-filled past T (adds +0 exactly); the mix with R_prev's own element is the epilogue.
 * The fp32 matrix instruction is an exact k-ordered fp32 fma chain, there are no atomics and no sum depends on the batch:
 * an image's rows are the same bits wherever it sits.
 */
#include "kernelHandler.h"
#include "kernel_limits.h"
#include "qkv_forms.h"
#include "vit_kernels.h"

namespace {

constexpr int RO_THREADS = 256;
constexpr int RO_QT = KL_ROLLOUT_QUERY_ROWS;   /* query rows per workgroup */
constexpr int RO_KC = KL_ROLLOUT_KEY_CHUNK;    /* keys per chunk: 16 per wave */
static_assert(RO_KC == 16 * RO_THREADS / 64, "a chunk is 16 keys per wave");
constexpr int RP_TILE = 64, RP_KC = 16;
constexpr int RP_AS = RP_KC + 4;     /* row strides in floats: the 16 rows of an A-operand read start in 16 distinct bank quads, */
constexpr int RP_RS = RP_TILE + 16;  /* the 4 rows of a B-operand read 16 banks apart */

/* Rows [first, first + count) of one image's Q|K|V, columns [col0, col0 + D), decoded to fp32 into dst[count][DS]; rows
 * >= T become zeros.  LPK lanes per row as in attn_map.hip, so a wave reads whole 256-byte / 64-byte segments. */
template <int FORM>
__device__ __forceinline__ void stage_rows(const char *__restrict__ qkv, size_t rows, int row_floats, size_t row0, int T, int first,
                                           int count, int col0, int D, int DS, float *dst)
{
    constexpr int PIECE = AmForm<FORM>::PIECE, LPK = AmForm<FORM>::LPK, PER_PASS = RO_THREADS / LPK;
    const int ppk = D / PIECE, sub = threadIdx.x % LPK;
    for (int grp = 0; grp * LPK < ppk; ++grp) {
        const int piece = grp * LPK + sub;
        for (int r = threadIdx.x / LPK; r < count; r += PER_PASS) {
            if (piece >= ppk)
                continue;
            float v[PIECE];
            if (first + r < T) {
                load_piece<FORM>(qkv, rows, row_floats, row0 + (size_t)(first + r), col0 + piece * PIECE, v);
            } else {
#pragma unroll
                for (int e = 0; e < PIECE; ++e)
                    v[e] = 0.0f;
            }
            float *d = dst + r * DS + piece * PIECE;
#pragma unroll
            for (int e = 0; e < PIECE; e += 4)
                *reinterpret_cast<f32x4 *>(d + e) = f32x4{v[e], v[e + 1], v[e + 2], v[e + 3]};
        }
    }
}

/* a_out [n][T][T]: the running sum over heads, then A.  r_first != NULL (the first step): the last head's rows go there as
 * 0.5 A + 0.5 I instead. */
template <int FORM>
__global__ __launch_bounds__(RO_THREADS) void rollout_attn_kernel(const char *__restrict__ qkv, int n_images, int T, int E, int H, int tiles,
                                                                  float scale, float *a_out, float *r_first)
{
    extern __shared__ __attribute__((aligned(16))) float ro_lds[];
    const int D = E / H, DS = D + 4, nj = D / 16, TP = kl_rollout_score_stride(T);
    float *const p_s = ro_lds, *const q_s = p_s + RO_QT * TP, *const k_s = q_s + RO_QT * DS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lg = lane >> 4;
    const int img = blockIdx.x / tiles, u0 = (blockIdx.x % tiles) * RO_QT;
    const size_t rows = (size_t)n_images * (size_t)T, row0 = (size_t)img * (size_t)T;
    const int row = tid >> 4, c = tid & 15, u = u0 + row;   /* the softmax's (query row, lane of 16) */
    float *const pr = p_s + row * TP;
    const size_t out_row = (row0 + (size_t)(u < T ? u : 0)) * (size_t)T;
    const float n_heads = (float)H;

    for (int h = 0; h < H; ++h) {
        stage_rows<FORM>(qkv, rows, 3 * E, row0, T, u0, RO_QT, h * D, D, DS, q_s);
        __syncthreads();
        f32x4 qf[AM_MAX_HEAD_DIM / 16];
#pragma unroll
        for (int j = 0; j < AM_MAX_HEAD_DIM / 16; ++j)
            if (j < nj)
                qf[j] = *reinterpret_cast<const f32x4 *>(q_s + l15 * DS + 16 * j + 4 * lg);

        /* the scaled scores of the 16 query rows against every key */
        for (int base = 0; base < T; base += RO_KC) {
            stage_rows<FORM>(qkv, rows, 3 * E, row0, T, base, RO_KC, E + h * D, D, DS, k_s);
            __syncthreads();
            const float *kp = k_s + (wave * 16 + l15) * DS + 4 * lg;
            f32x4 acc[2] = {f32x4{0.0f, 0.0f, 0.0f, 0.0f}, f32x4{0.0f, 0.0f, 0.0f, 0.0f}};
#pragma unroll
            for (int j = 0; j < AM_MAX_HEAD_DIM / 16; ++j)
                if (j < nj) {
                    const f32x4 kf = *reinterpret_cast<const f32x4 *>(kp + 16 * j);
#pragma unroll
                    for (int e = 0; e < 4; ++e)   /* result [query 4 lg + r][key l15] */
                        acc[j & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[j][e], kf[e], acc[j & 1], 0, 0, 0);
                }
            const int key = base + wave * 16 + l15;   /* < TP - 20; columns >= T are never read */
#pragma unroll
            for (int r = 0; r < 4; ++r)
                p_s[(4 * lg + r) * TP + key] = (acc[0][r] + acc[1][r]) * scale;
            __syncthreads();
        }

        /* softmax of the 16 rows, 16 lanes each, and the running sum over heads */
        float mx = -INFINITY;
        for (int t = c; t < T; t += 16)
            mx = fmaxf(mx, pr[t]);
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1)
            mx = fmaxf(mx, __shfl_xor(mx, m));
        float sum = 0.0f;
        for (int t = c; t < T; t += 16) {
            const float ex = expf(pr[t] - mx);
            pr[t] = ex;
            sum += ex;
        }
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1)
            sum += __shfl_xor(sum, m);
        if (u < T) {
            float *const ar = a_out + out_row;
            for (int t = c; t < T; t += 16) {
                const float p = pr[t] / sum;
                float a = h == 0 ? p : ar[t] + p;
                if (h == H - 1) {
                    a = a / n_heads;
                    if (r_first) {
                        r_first[out_row + t] = 0.5f * a + (t == u ? 0.5f : 0.0f);
                        continue;
                    }
                }
                ar[t] = a;
            }
        }
        __syncthreads();   /* the next head's Q tile and scores */
    }
}

/* r_next = 0.5 (a . r_prev) + 0.5 r_prev, per image; all three [n][T][T] */
__global__ __launch_bounds__(RO_THREADS) void rollout_product_kernel(const float *__restrict__ a, const float *__restrict__ r_prev,
                                                                     float *__restrict__ r_next, int T, int tiles)
{
    __shared__ __attribute__((aligned(16))) float a_s[RP_TILE * RP_AS];
    __shared__ __attribute__((aligned(16))) float r_s[RP_KC * RP_RS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lg = lane >> 4;
    const int img = blockIdx.x / (tiles * tiles), rem = blockIdx.x % (tiles * tiles);
    const int u0 = (rem / tiles) * RP_TILE, t0 = (rem % tiles) * RP_TILE;
    const size_t image = (size_t)img * (size_t)T * (size_t)T;
    const float *const ai = a + image, *const ri = r_prev + image;
    float *const oi = r_next + image;
    f32x4 acc[RP_TILE / 16];
#pragma unroll
    for (int j = 0; j < RP_TILE / 16; ++j)
        acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    for (int v0 = 0; v0 < T; v0 += RP_KC) {
#pragma unroll
        for (int i = 0; i < RP_TILE * RP_KC / RO_THREADS; ++i) {
            const int idx = tid + i * RO_THREADS;
            const int ur = idx / RP_KC, vc = idx % RP_KC;   /* A: 64 rows x 16 columns */
            a_s[ur * RP_AS + vc] = (u0 + ur < T && v0 + vc < T) ? ai[(size_t)(u0 + ur) * T + (size_t)(v0 + vc)] : 0.0f;
            const int vr = idx / RP_TILE, tc = idx % RP_TILE;   /* R_prev: 16 rows x 64 columns */
            r_s[vr * RP_RS + tc] = (v0 + vr < T && t0 + tc < T) ? ri[(size_t)(v0 + vr) * T + (size_t)(t0 + tc)] : 0.0f;
        }
        __syncthreads();
        const f32x4 af = *reinterpret_cast<const f32x4 *>(a_s + (wave * 16 + l15) * RP_AS + 4 * lg);
#pragma unroll
        for (int e = 0; e < 4; ++e)   /* k-step e sums v = v0 + 4 g + e, g = 0..3 */
#pragma unroll
            for (int j = 0; j < RP_TILE / 16; ++j)
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[e], r_s[(4 * lg + e) * RP_RS + 16 * j + l15], acc[j], 0, 0, 0);
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < RP_TILE / 16; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int u = u0 + wave * 16 + 4 * lg + r, t = t0 + 16 * j + l15;
            if (u < T && t < T) {
                const size_t at = (size_t)u * T + (size_t)t;
                oi[at] = 0.5f * acc[j][r] + 0.5f * ri[at];
            }
        }
}

/* out[i][t] = r[i][0][t] */
__global__ __launch_bounds__(RO_THREADS) void rollout_read_kernel(const float *__restrict__ r, float *__restrict__ out, int T, int tiles)
{
    const int img = blockIdx.x / tiles, t = (blockIdx.x % tiles) * RO_THREADS + threadIdx.x;
    if (t < T)
        out[(size_t)img * T + t] = r[(size_t)img * T * T + t];
}

template <int FORM>
int launch_rollout_attn(hipStream_t st, const void *qkv, int n, int T, int E, int H, float *a_out, float *r_first)
{
    const int tiles = (T + RO_QT - 1) / RO_QT;
    const size_t lds = kl_rollout_lds_bytes(T, E / H);
    VH_SET_LDS_ONCE((rollout_attn_kernel<FORM>), KL_LDS_BYTES);
    hipLaunchKernelGGL(rollout_attn_kernel<FORM>, dim3((unsigned)((size_t)n * tiles)), dim3(RO_THREADS), lds, st,
                       static_cast<const char *>(qkv), n, T, E, H, tiles, 1.0f / sqrtf((float)(E / H)), a_out, r_first);
    VH_LAUNCH_CHECK("rollout_attn_kernel");
    return 0;
}

} // namespace

extern "C" size_t vh_rollout_workspace(int n_images, int tokens)
{
    return kl_rollout_workspace(n_images, tokens);
}

extern "C" int vh_rollout_max_tokens(int head_dim) { return kl_rollout_max_tokens(head_dim); }

extern "C" int vh_launch_rollout_step(vh_stream_t s, const void *qkv, int qkv_form, int n_images, int tokens, int embed_dim, int num_heads,
                                      const float *r_prev, float *r_next, void *workspace)
{
    if (!qkv || !r_next || !workspace)
        return vh_fail(1, "vh_launch_rollout_step: null pointer argument (qkv, r_next or workspace)");
    if (qkv_form != VH_QKV_ROWS_F32 && qkv_form != VH_QKV_PLANES3 && qkv_form != VH_QKV_PLANES_F16)
        return vh_fail(1, "vh_launch_rollout_step: qkv_form=%d must be VH_QKV_ROWS_F32, VH_QKV_PLANES3 or VH_QKV_PLANES_F16", qkv_form);
    if (n_images <= 0 || tokens < 1 || num_heads <= 0 || embed_dim <= 0 || embed_dim % num_heads != 0)
        return vh_fail(1, "vh_launch_rollout_step: bad arguments (n=%d tokens=%d embed=%d heads=%d)", n_images, tokens, embed_dim, num_heads);
    const int D = embed_dim / num_heads;
    if (!kl_cls_attention_head_dim_ok(D))
        return vh_fail(1, "vh_launch_rollout_step: head_dim=%d must be a multiple of 16, at most %d", D, KL_CLS_ATTN_MAX_HEAD_DIM);
    if (qkv_form != VH_QKV_ROWS_F32 && embed_dim % 32 != 0)
        return vh_fail(1, "vh_launch_rollout_step: embed_dim=%d: the planes forms need a multiple of 32", embed_dim);
    if ((((uintptr_t)qkv | (uintptr_t)r_prev | (uintptr_t)r_next | (uintptr_t)workspace) & 15) != 0)
        return vh_fail(1, "vh_launch_rollout_step: pointers must be 16-byte aligned");
    if (r_prev == r_next || (const void *)r_prev == workspace || (void *)r_next == workspace)
        return vh_fail(1, "vh_launch_rollout_step: r_prev, r_next and workspace must be three different buffers");
    if (kl_rollout_lds_bytes(tokens, D) > (size_t)KL_LDS_BYTES)
        return vh_fail(1, "vh_launch_rollout_step: tokens=%d: at most %d at head_dim %d (the score rows of 16 queries stay in LDS)", tokens,
                       kl_rollout_max_tokens(D), D);
    const size_t q_tiles = ((size_t)tokens + RO_QT - 1) / RO_QT, p_tiles = ((size_t)tokens + RP_TILE - 1) / RP_TILE;
    if (((size_t)n_images * q_tiles) >> 31 || ((size_t)n_images * p_tiles * p_tiles) >> 31 || ((size_t)n_images * tokens) >> 31)
        return vh_fail(1, "vh_launch_rollout_step: n=%d x tokens=%d too large for one launch", n_images, tokens);
    hipStream_t st = (hipStream_t)s;
    float *const a = static_cast<float *>(workspace), *const first = r_prev ? nullptr : r_next;
    int rc;
    switch (qkv_form) {
    case VH_QKV_ROWS_F32: rc = launch_rollout_attn<VH_QKV_ROWS_F32>(st, qkv, n_images, tokens, embed_dim, num_heads, a, first); break;
    case VH_QKV_PLANES3: rc = launch_rollout_attn<VH_QKV_PLANES3>(st, qkv, n_images, tokens, embed_dim, num_heads, a, first); break;
    default: rc = launch_rollout_attn<VH_QKV_PLANES_F16>(st, qkv, n_images, tokens, embed_dim, num_heads, a, first); break;
    }
    if (rc != 0 || !r_prev)
        return rc;
    hipLaunchKernelGGL(rollout_product_kernel, dim3((unsigned)((size_t)n_images * p_tiles * p_tiles)), dim3(RO_THREADS), 0, st, a, r_prev,
                       r_next, tokens, (int)p_tiles);
    VH_LAUNCH_CHECK("rollout_product_kernel");
    return 0;
}

extern "C" int vh_launch_rollout_read(vh_stream_t s, const float *r, int n_images, int tokens, float *out)
{
    if (!r || !out)
        return vh_fail(1, "vh_launch_rollout_read: null pointer argument");
    if (n_images <= 0 || tokens < 1)
        return vh_fail(1, "vh_launch_rollout_read: bad arguments (n=%d tokens=%d)", n_images, tokens);
    if ((((uintptr_t)r | (uintptr_t)out) & 15) != 0)
        return vh_fail(1, "vh_launch_rollout_read: pointers must be 16-byte aligned");
    const size_t tiles = ((size_t)tokens + RO_THREADS - 1) / RO_THREADS;
    if (((size_t)n_images * tiles) >> 31)
        return vh_fail(1, "vh_launch_rollout_read: n=%d x tokens=%d too large for one launch", n_images, tokens);
    hipLaunchKernelGGL(rollout_read_kernel, dim3((unsigned)((size_t)n_images * tiles)), dim3(RO_THREADS), 0, (hipStream_t)s, r, out, tokens,
                       (int)tiles);
    VH_LAUNCH_CHECK("rollout_read_kernel");
    return 0;
}
