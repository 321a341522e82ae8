/*
 * topk.hip -- the k best classes of every row of fp32 logits, with their logits or probabilities.
 *
 * What Main.c:59-72 does on the host for k = 1 (a strict `>` scan over a whole probability row fetched over PCIe), done
 * where the logits are: one 256-thread workgroup per row, k rounds of "the largest key strictly below the previous
 * winner".  An element's key is 64 bits: the order-preserving unsigned image of the float (-0 folded to +0, NaN -> 0,
 * so below -inf) above 0xFFFFFFFF - index.  Keys of a row are distinct, so a round needs no "taken" marks, equal logits
 * rank by ascending index, and the labels of a row are distinct by construction.  Rows up to 2048 entries stay in
 * registers (softmax_kernel's layout: element tid + 256 i in slot i); longer rows are re-read from L2 in 256-wide
 * strides every round.
 *
 * Probabilities: the arithmetic of softmax_kernel (rowops.hip), restated here operation for operation -- the same loads,
 * fmaxf chain, wave_max and LDS maximum, expf(v - mx), per-thread sum order, wave_sum and (red[0] + red[1]) + (red[2] +
 * red[3]), then expf(v - mx) / sum of the winners alone -- so that for rows the softmax takes (<= 2048) a score has the
 * bits vh_launch_softmax writes at that position.  softmax_kernel itself is untouched.  Longer rows use the same
 * formula with each thread summing its strided elements in ascending index order.  No atomics: a row's output depends on
 * that row only.
 */
#include "kernelHandler.h"
#include "vit_kernels.h"

namespace {

constexpr int TK_THREADS = 256;
constexpr int TK_REG = 8;      /* rows up to 2048 entries stay in registers, as in softmax_kernel */
constexpr int TK_MAX_K = 32;
constexpr int TK_MAX_LENGTH = 65536;

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
        v = fmaxf(v, __shfl_xor(v, m));
    return v;
}

template <bool REG>
__global__ __launch_bounds__(TK_THREADS) void topk_kernel(const float *__restrict__ in, int length, int k, int probs,
                                                         int *__restrict__ labels, float *__restrict__ scores)
{
    __shared__ float red[TK_THREADS / 64];
    __shared__ unsigned long long kred[2][TK_THREADS / 64];
    __shared__ int win[TK_MAX_K];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *src = in + (size_t)blockIdx.x * length;

    float v[TK_REG];
    float mx = -INFINITY, sum = 0.0f;
    if (REG) {
#pragma unroll
        for (int i = 0; i < TK_REG; ++i) {
            const int idx = tid + i * TK_THREADS;
            v[i] = idx < length ? src[idx] : -INFINITY;
            mx = fmaxf(mx, v[i]);
        }
    } else if (probs) {
        for (int idx = tid; idx < length; idx += TK_THREADS)
            mx = fmaxf(mx, src[idx]);
    }
    if (probs) {
        mx = wave_max(mx);
        if (lane == 0)
            red[wave] = mx;
        __syncthreads();
        mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        __syncthreads();
        if (REG) {
#pragma unroll
            for (int i = 0; i < TK_REG; ++i)
                sum += expf(v[i] - mx);          /* exp(-inf) = 0 for the padding */
        } else {
            for (int idx = tid; idx < length; idx += TK_THREADS)
                sum += expf(src[idx] - mx);
        }
        sum = wave_sum(sum);
        if (lane == 0)
            red[wave] = sum;
        __syncthreads();
        sum = (red[0] + red[1]) + (red[2] + red[3]);
    }

    unsigned long long key[TK_REG];
    if (REG) {
#pragma unroll
        for (int i = 0; i < TK_REG; ++i) {
            const int idx = tid + i * TK_THREADS;
            key[i] = idx < length ? rank_key(v[i], idx) : 0ull;
        }
    }
    unsigned long long below = ~0ull;            /* above every key: the image of +inf is 0xFF800000 */
    for (int j = 0; j < k; ++j) {
        unsigned long long best = 0ull;          /* k <= length: a key in (0, below) exists in every round */
        if (REG) {
#pragma unroll
            for (int i = 0; i < TK_REG; ++i)
                best = key[i] < below && key[i] > best ? key[i] : best;
        } else {
#pragma unroll 4
            for (int idx = tid; idx < length; idx += TK_THREADS) {
                const unsigned long long c = rank_key(src[idx], idx);
                best = c < below && c > best ? c : best;
            }
        }
        best = wave_max_key(best);
        if (lane == 0)
            kred[j & 1][wave] = best;            /* two slots: round j + 1 writes the other one while a late wave still reads */
        __syncthreads();
        const unsigned long long a = kred[j & 1][0], b = kred[j & 1][1], c = kred[j & 1][2], d = kred[j & 1][3];
        const unsigned long long ab = a > b ? a : b, cd = c > d ? c : d;
        below = ab > cd ? ab : cd;
        if (tid == 0)
            win[j] = (int)(0xFFFFFFFFu - (unsigned)below);
    }
    __syncthreads();
    if (tid < k) {                               /* the k pairs: one lane each, plain vector stores */
        const int label = win[tid];
        const size_t o = (size_t)blockIdx.x * k + tid;
        labels[o] = label;
        if (scores) {
            const float x = src[label];
            scores[o] = probs ? expf(x - mx) / sum : x;
        }
    }
}

} // namespace

extern "C" int vh_launch_topk(vh_stream_t s, const float *logits, int rows, int length, int k, int score_kind, int *labels,
                              float *scores)
{
    if (!logits || !labels)
        return vh_fail(1, "vh_launch_topk: null pointer argument (logits, labels)");
    if (rows <= 0 || length < 1 || length > TK_MAX_LENGTH)
        return vh_fail(1, "vh_launch_topk: rows=%d must be positive, length=%d in 1..%d", rows, length, TK_MAX_LENGTH);
    if (k < 1 || k > TK_MAX_K || k > length)
        return vh_fail(1, "vh_launch_topk: k=%d must be in 1..%d and <= length=%d", k, TK_MAX_K, length);
    if (score_kind != VIT_TOPK_PROBS && score_kind != VIT_TOPK_LOGITS)
        return vh_fail(1, "vh_launch_topk: score_kind=%d must be VIT_TOPK_PROBS or VIT_TOPK_LOGITS", score_kind);
    const int probs = scores && score_kind == VIT_TOPK_PROBS;   /* no scores asked for: no exponentials */
    if (length <= TK_THREADS * TK_REG)
        hipLaunchKernelGGL(topk_kernel<true>, dim3(rows), dim3(TK_THREADS), 0, (hipStream_t)s, logits, length, k, probs, labels,
                           scores);
    else
        hipLaunchKernelGGL(topk_kernel<false>, dim3(rows), dim3(TK_THREADS), 0, (hipStream_t)s, logits, length, k, probs, labels,
                           scores);
    VH_LAUNCH_CHECK("topk_kernel");
    return 0;
}
