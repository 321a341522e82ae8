/*
 * attention_long.hip -- softmax(Q K^T / sqrt(D)) V per (image, head) for ANY token count: the higher-resolution ViTs
 * (B/16 at 384 px: T = 577, L/16 at 512: T = 1025, H/14 at 518: T = 1370), which neither the resident kernels
 * (attention_p3.hip, attention_h16.hip: one head's K and V in LDS, T <= 208 / 272) nor the streaming kernel
 * (attention_tiled.hip: the whole score row of a query in registers, T <= 512) take.
 *
 * Same operator as QKV_TO_SCOREV (multihead.cl:65-137), CPU statement multihead_attn_seq, ViT_seq.c:192-262, on the
 * Q|K|V planes the QKV projection already writes for the resident kernels:
 *  - NPL = 3: the exact three-part bf16 planes [3E/32][3][rows][32] (the F32 path).  Both products are fp32 products
 *    formed from the splits, six v_mfma_f32_16x16x32_bf16 per block (attention_p3.hip's terms); P is split in registers;
 *  - NPL = 1: one-part fp16 planes [3E/32][rows][32] (the reduced modes): fp16 operands, fp32 accumulation and softmax,
 *    the arithmetic of vh_launch_attention_f16.
 * Flash-style (online softmax), nothing grows with T:
 *  - a workgroup of NW waves takes 16 NW queries of one (image, head); a wave owns a 16-query tile.  S^T = K Q^T puts a
 *    query's scores in the registers of the four lanes l15 + 16 g: register r of key tile j is key 16j + 4g + r;
 *  - K and V stream through LDS in chunks of 64 keys, a ring of two (K, V) stages filled by LDS-DMA: chunk c + 1 lands
 *    while chunk c computes.  One workgroup barrier per chunk, behind an explicit vmcnt(0) that waits for chunk c only
 *    (c + 1 is issued after it);
 *  - the running max m (per query, identical in its four lanes) and a per-lane partial running sum l live in registers;
 *    the O^T = V^T P^T accumulators belong to the lane's query, so the rescale by exp(m_old - m_new) is register-local;
 *    the lane-group sums of l are added once at the end, and O is divided by l once;
 *  - P goes from the S^T accumulators into the B operand of P.V (converted / split) without leaving registers;
 *  - K fragments: ds_read_b128 from rows whose 16-byte chunks carry gemm_common.h's swz64; V fragments: two
 *    ds_read_b64_tr_b16 per MFMA from linear rows (attention_h16.hip's addressing);
 *  - head_dim 80: head h starts at column 80h = 32 p0 + 16 sh; the planes p0 .. p0 + 2 are staged and the 16-wide d group
 *    g sits in plane (g + sh) >> 1, half (g + sh) & 1 (attention_h16.hip).
 * The score is scaled after the dot product (one fma into exp2, as the scalar loop scales before expf).  Keys past T in
 * the ragged last chunk score -inf (P = 0 exactly, against clamped finite V rows).  Every query visits the chunks in
 * order with no split over keys: the result of a row does not depend on the batch around it.
 * Output: fp32 rows [rows][E], heads concatenated.
 */
#include "kernelHandler.h"
#include "kernel_limits.h"
#include "vit_kernels.h"
#include "fp32_split.h"
#include "gemm_common.h"

namespace {

typedef const __attribute__((address_space(1))) void *gptr_t;
typedef __attribute__((address_space(3))) void *lptr_t;
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

constexpr int KC = 64;        /* keys per chunk */
constexpr int NW = 8;         /* waves per workgroup: 128 queries */
constexpr int MAX_LDS = KL_LDS_BYTES;

template <int HD> constexpr int planes_staged() { return HD % 32 == 0 ? HD / 32 : (HD + 16 + 31) / 32; }
template <int HD, int NPL> constexpr size_t lds_bytes() { return (size_t)2 * 2 * planes_staged<HD>() * NPL * KC * 64; }

template <int HD, int NPL>
__global__ __launch_bounds__(64 * NW) void attention_long_kernel(const char *__restrict__ qkv, float *__restrict__ out,
                                                                int T, int E, int H, int n_qblocks, float scale_log2e)
{
    typedef typename PartT<NPL>::type part_t;        /* bf16x8 (three parts) or half8 (one fp16 part) */
    constexpr int NT = n_terms<NPL>();               /* products per block */
    constexpr int G = HD / 16;                       /* 16-wide d groups */
    constexpr int GS = (G + 1) / 2;                  /* 32-deep steps of Q.K^T (the last may be half empty) */
    constexpr int PLN = planes_staged<HD>();
    constexpr int OPB = PLN * NPL * KC * 64;         /* bytes of one operand's chunk: [plane][part][64 rows][64 B] */
    constexpr int PIECES = PLN * NPL * (KC / 16);    /* 1 KB LDS-DMA pieces per operand chunk */
    static_assert(HD % 16 == 0, "head_dim");
    extern __shared__ __attribute__((aligned(16))) char smem[];   /* stage s: K at 2 s OPB, V at (2 s + 1) OPB */

    const int item = blockIdx.x / n_qblocks, qb = blockIdx.x - item * n_qblocks;
    const int b = item / H, h = item - b * H;
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int E32 = E >> 5;
    const size_t prow = (size_t)(gridDim.x / n_qblocks / H) * T;    /* rows of the whole activation matrix */
    const size_t row0 = (size_t)b * T;
    const int c0 = HD * h, p0 = c0 >> 5, sh = (c0 >> 4) & 1;
    const int q_row = qb * 16 * NW + wave * 16 + l15;
    const bool active = qb * 16 * NW + wave * 16 < T;   /* wave-uniform */
    const int n_chunks = (T + KC - 1) / KC;

    /* LDS-DMA of chunk c of operand `which` (1 = K, 2 = V): piece p = 16 rows x 64 B of one (plane, part); the lane fills
     * physical chunk (lane & 3) of row 16 rb + (lane >> 2); K rows carry the read swizzle, V rows are linear */
    auto dma = [&](int c, int which, char *dst) {
        for (int p = wave; p < PIECES; p += NW) {
            const int pp = p / (KC / 16), rb = p - pp * (KC / 16);       /* pp = plane * NPL + part */
            const int plane = pp / NPL, part = pp - plane * NPL;
            const int r = KC * c + 16 * rb + (lane >> 2);
            int ch = lane & 3;
            if (which == 1)
                ch ^= swz64(lane >> 4);
            const int pl = min(which * E32 + p0 + plane, 3 * E32 - 1);   /* head_dim 80: the window may pass V's last plane */
            const char *src = qkv + (((size_t)pl * NPL + part) * prow + row0 + min(r, T - 1)) * 64 + 16 * ch;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(dst + p * 1024), 16, 0, 0);
        }
    };

    /* Q.K^T step s2: this lane group contracts the 16-wide d group 2 s2 + (g >> 1), its 8 values 8 (g & 1) .. +7 -- chunk
     * 2 ((d group + sh) & 1) + (g & 1) of plane (d group + sh) >> 1.  Lanes whose d group lies past the head carry Q = 0
     * and read the step's lower half of K again (finite values). */
    int kofs[GS];
    part_t qf[GS][NPL];
    {
        const size_t qr = row0 + min(q_row, T - 1);
#pragma unroll
        for (int s2 = 0; s2 < GS; ++s2) {
            const bool live = 2 * s2 + (g >> 1) < G;
            const int idx = (live ? 2 * s2 + (g >> 1) : 2 * s2) + sh, ch = 2 * (idx & 1) + (g & 1);
            kofs[s2] = (idx >> 1) * NPL * (KC * 64) + l15 * 64 + 16 * (ch ^ swz64(l15 >> 2));
#pragma unroll
            for (int pl = 0; pl < NPL; ++pl) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(qkv + (((size_t)(p0 + (idx >> 1)) * NPL + pl) * prow + qr) * 64 + 16 * ch);
                qf[s2][pl] = live ? __builtin_bit_cast(part_t, v) : part_t{};
            }
        }
    }
    const int vrow = (4 * g + (l15 >> 2)) * 64 + 8 * (l15 & 3);   /* transposed read: lane i addresses row i >> 2, columns 4 (i & 3) .. */

    f32x4 O[G];
#pragma unroll
    for (int dt = 0; dt < G; ++dt)
        O[dt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float m = -INFINITY, l = 0.0f;

    dma(0, 1, smem);
    dma(0, 2, smem + OPB);
    for (int c = 0; c < n_chunks; ++c) {
        /* chunk c has landed (every wave waits for its own DMA pieces: __syncthreads() alone waits for LDS operations only,
         * and a wave with no live query would never wait for its pieces); every wave is done with chunk c - 1 */
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (c + 1 < n_chunks) {
            char *nxt = smem + 2 * OPB * ((c + 1) & 1);
            dma(c + 1, 1, nxt);
            dma(c + 1, 2, nxt + OPB);
        }
        if (!active)
            continue;
        const char *Kb = smem + 2 * OPB * (c & 1), *Vb = Kb + OPB;
        const int live_keys = T - KC * c;                 /* > 0; < KC in the ragged last chunk only */

        /* S^T = K Q^T: rows = keys of tile j, column = this lane's query */
        f32x4 S[KC / 16];
#pragma unroll
        for (int j = 0; j < KC / 16; ++j) {
            f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
            if (16 * j < live_keys) {                     /* uniform */
#pragma unroll
                for (int s2 = 0; s2 < GS; ++s2) {
                    part_t kf[NPL];
#pragma unroll
                    for (int pl = 0; pl < NPL; ++pl)
                        kf[pl] = *reinterpret_cast<const part_t *>(Kb + kofs[s2] + pl * (KC * 64) + j * 1024);
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        acc = mfma_part(kf[term_w<NPL>(t)], qf[s2][term_a<NPL>(t)], acc);
                }
            }
            S[j] = acc;
        }

        /* online softmax: chunk max, new running max, rescale of what was summed at the old one */
        if (live_keys < KC) {
#pragma unroll
            for (int j = 0; j < KC / 16; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (16 * j + 4 * g + r >= live_keys)
                        S[j][r] = -INFINITY;
        }
        float cm = -INFINITY;
#pragma unroll
        for (int j = 0; j < KC / 16; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                cm = fmaxf(cm, S[j][r]);
        cm = fmaxf(cm, __shfl_xor(cm, 16));
        cm = fmaxf(cm, __shfl_xor(cm, 32));
        const float m_new = fmaxf(m, cm);                 /* finite: every chunk holds a live key */
        const float alpha = __builtin_amdgcn_exp2f((m - m_new) * scale_log2e);   /* 0 at the first chunk (m = -inf) */
        m = m_new;
        const float off = -m_new * scale_log2e;
        float sum = 0.0f;
#pragma unroll
        for (int j = 0; j < KC / 16; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                S[j][r] = __builtin_amdgcn_exp2f(__builtin_fmaf(S[j][r], scale_log2e, off));
                sum += S[j][r];
            }
        l = __builtin_fmaf(l, alpha, sum);
#pragma unroll
        for (int dt = 0; dt < G; ++dt)
            O[dt] *= alpha;

        /* O^T += V^T P^T: one MFMA contracts the key tiles 2t and 2t + 1 -- lane group g the keys 32t + 4g .. +3 (slots 0-3)
         * and 32t + 16 + 4g .. +3 (slots 4-7), the S^T registers it holds */
#pragma unroll
        for (int t = 0; t < KC / 32; ++t) {
            if (32 * t < live_keys) {                     /* uniform */
                part_t pp[NPL];
                if (NPL == 1) {
                    const half4 pl = to_half4(S[2 * t]), pu = to_half4(S[2 * t + 1]);
                    pp[0] = __builtin_bit_cast(part_t, half8{pl[0], pl[1], pl[2], pl[3], pu[0], pu[1], pu[2], pu[3]});
                } else {
                    split_parts(S[2 * t], S[2 * t + 1], pp);
                }
#pragma unroll
                for (int dt = 0; dt < G; ++dt) {
                    const int idx = dt + sh;
                    part_t vf[NPL];
#pragma unroll
                    for (int pl = 0; pl < NPL; ++pl) {
                        const char *vp = Vb + ((idx >> 1) * NPL + pl) * (KC * 64) + vrow + 32 * (idx & 1) + 2 * t * 1024;
                        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(vp));
                        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(vp + 1024));
                        vf[pl] = __builtin_bit_cast(part_t, s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
                    }
#pragma unroll
                    for (int tt = 0; tt < NT; ++tt)
                        O[dt] = mfma_part(vf[term_w<NPL>(tt)], pp[term_a<NPL>(tt)], O[dt]);
                }
            }
        }
    }

    /* O^T register r of d group dt: d = 16 dt + 4g + r, query = lane & 15 */
    if (active) {
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        if (q_row < T) {
            float *o = out + (row0 + q_row) * (size_t)E + (size_t)c0 + 4 * g;
#pragma unroll
            for (int dt = 0; dt < G; ++dt)
                *reinterpret_cast<f32x4 *>(o + 16 * dt) = O[dt] / l;
        }
    }
}

template <int HD, int NPL>
int launch_long(hipStream_t st, const char *qkv, float *out, int n_images, int T, int E, int H)
{
    constexpr size_t lds = lds_bytes<HD, NPL>();
    static_assert(lds <= MAX_LDS, "LDS");
    VH_SET_LDS_ONCE((attention_long_kernel<HD, NPL>), lds);
    const int n_qblocks = (T + 16 * NW - 1) / (16 * NW);
    const float c = 1.4426950408889634f / sqrtf((float)HD);
    hipLaunchKernelGGL((attention_long_kernel<HD, NPL>), dim3((unsigned)(n_images * H * n_qblocks)), dim3(64 * NW), lds, st, qkv, out,
                       T, E, H, n_qblocks, c);
    VH_LAUNCH_CHECK("attention_long_kernel");
    return 0;
}

} // namespace

/* qkv_planes: the QKV projection's planes -- parts 3: exact three-part bf16 [3E/32][3][rows][32] (vh_launch_linear_p3
 * with output_planes), parts 1: one-part fp16 [3E/32][rows][32] (vh_launch_linear_planes / _mx_planes_f16, kind 2);
 * rows = n_images * tokens.  output: fp32 rows [rows][embed_dim].  head_dim 64 or 80, embed_dim % 32 == 0 (whole planes: an
 * even head count at head_dim 80), any tokens >= 1. */
extern "C" int vh_launch_attention_long(vh_stream_t s, const void *qkv_planes, int parts, float *output, int n_images, int tokens,
                                        int embed_dim, int num_heads)
{
    if (!qkv_planes || !output)
        return vh_fail(1, "vh_launch_attention_long: null pointer argument");
    if (n_images <= 0 || tokens <= 0 || num_heads <= 0 || embed_dim % num_heads != 0 || (parts != 1 && parts != 3))
        return vh_fail(1, "vh_launch_attention_long: bad arguments (n=%d tokens=%d embed=%d heads=%d parts=%d)", n_images, tokens,
                       embed_dim, num_heads, parts);
    const int D = embed_dim / num_heads;
    if (!kl_attn_long_head_dim_ok(D) || embed_dim % 32 != 0)
        return vh_fail(1, "vh_launch_attention_long: head_dim %d (embed=%d heads=%d) not built: head_dim 64 or 80", D, embed_dim,
                       num_heads);
    const size_t rows = (size_t)n_images * (size_t)tokens;
    const size_t n_qblocks = ((size_t)tokens + 16 * NW - 1) / (16 * NW);
    /* grid and every row index in int / 32-bit where the kernel keeps them; byte offsets are size_t */
    if (((size_t)n_images * num_heads * n_qblocks) >> 31 || rows >> 31 || (rows * (size_t)embed_dim) >> 62)
        return vh_fail(1, "vh_launch_attention_long: n_images=%d x tokens=%d is too large", n_images, tokens);
    if ((((uintptr_t)qkv_planes | (uintptr_t)output) & 15) != 0)
        return vh_fail(1, "vh_launch_attention_long: pointers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)s;
    const char *in = static_cast<const char *>(qkv_planes);
    if (D == 64)
        return parts == 3 ? launch_long<64, 3>(st, in, output, n_images, tokens, embed_dim, num_heads)
                          : launch_long<64, 1>(st, in, output, n_images, tokens, embed_dim, num_heads);
    return parts == 3 ? launch_long<80, 3>(st, in, output, n_images, tokens, embed_dim, num_heads)
                      : launch_long<80, 1>(st, in, output, n_images, tokens, embed_dim, num_heads);
}
