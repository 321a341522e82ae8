/*
 * gallery.hip -- the k gallery rows most similar to every query: score(i, r) = sum_d queries[i][d] * row_r[d], selected on
 * the fly, so that the n x G score matrix never exists.  What vh_launch_topk does for logits, done for embeddings against
 * rows the caller holds in device memory (retrieval, k-NN classification, de-duplication).  No reference counterpart.
 *
 * The sum.  Columns are taken 32 at a time (c = 0, 32, ...), inside those 16 at a time (j = 0, 1), and a 16-column piece
 * goes through four v_mfma_f32_16x16x4_f32, e = 0..3, each of which adds columns c + 16 j + 4 g + e for g = 0, 1, 2, 3 in
 * that order: ONE fp32 fma chain from +0 per score, in an order fixed by embed_dim alone, columns >= embed_dim being zeros
 * in both operands (fma(0, 0, x) = x; the chain starts at +0 and so never holds -0).  Every score is formed by the same
 * instruction sequence whichever lane, wave, workgroup, query tile, split or storage type it falls to: its bits depend on
 * the two vectors only.  bf16 rows are shifted into the high half of an fp32 as they are loaded (exact), 16 bytes per lane.  Against the
 * exact dot product |error| <= E * 2^-24 * sum_d |q_d g_d| for this single chain; the header states (E + 8).
 *
 * gallery_scan_kernel, one 256-thread workgroup per (split of the gallery, tile of QT queries), QT = 16 for n <= 16 and
 * 128 beyond:
 *   - row tiles of 128 rows (32 per wave) x 32 columns and the query tile's same columns are staged in LDS through
 *     registers: the next stage's global loads are issued before the current stage's matrix instructions and written
 *     behind them.  (Register staging and LDS-DMA stream a table at the same rate on this GPU; registers let the bf16
 *     decode and the zero fill of ragged edges happen on the way.  At 16 queries the kernel reads 10^6 fp32 rows of 768 at
 *     5.8 TB/s, profiles/gallery_rates.txt.)
 *   - a wave holds 32 rows x QT queries of scores in 2 x QT/16 accumulators (64 registers at QT = 128), independent, so
 *     that the instruction's 40-cycle dependent latency is covered at its 32-cycle issue rate;
 *   - behind a row tile's last column every score becomes its 64-bit key (rank_key, vit_kernels.h) and is compared with
 *     the query's current k-th best, the last entry of its descending list [QT][k] in LDS.  A better key is bubbled in:
 *     at slot 0, 1, ... it leaves max(slot, carry) by a 64-bit integer LDS atomic and carries min(slot, carry) on.
 *     Whatever the interleaving of the lanes, slot j ends as the (j + 1)-th largest key that ever arrived (every key but
 *     the final holders of slots < j passes slot j), so the list is a function of the SET of candidates; the filter only
 *     drops keys below a value the k-th slot has already reached.  No floating-point atomics.
 *   - the lists go to workspace [n][splits][k].
 * gallery_merge_kernel, one workgroup per query: k rounds of "the largest key strictly below the previous winner" over the
 * splits * k keys, as topk_kernel's; the index and the score's bits are unpacked from the key (a NaN score is written as
 * 0x7FC00000).
 */
#include "kernelHandler.h"
#include "kernel_limits.h"
#include "vit_kernels.h"

namespace {

typedef unsigned long long u64;

constexpr int GA_THREADS = 256;
constexpr int GA_RT = KL_GALLERY_ROW_TILE;   /* gallery rows per tile: 32 per wave */
constexpr int GA_KC = 32;                  /* columns per stage */
constexpr int GA_LS = GA_KC + 4;           /* LDS row stride in floats: the 16 rows of an operand read start 4 banks apart */
constexpr int GA_QT_SMALL = 16, GA_QT_LARGE = 128;
constexpr int GA_MAX_K = 32, GA_MAX_E = KL_GALLERY_MAX_EMBED;
constexpr int GA_ROW_PIECES = GA_RT * (GA_KC / 4) / GA_THREADS;   /* 4-column pieces of a row stage per thread */

inline int ga_query_tile(int n_queries) { return n_queries <= GA_QT_SMALL ? GA_QT_SMALL : GA_QT_LARGE; }
inline long ga_row_tiles(long n_rows) { return (n_rows + GA_RT - 1) / GA_RT; }
inline size_t ga_lds_bytes(int qt, int k) { return (size_t)(GA_RT + qt) * GA_LS * sizeof(float) + (size_t)qt * k * sizeof(u64); }

/* splits = 0: enough workgroups to fill the machine -- two per CU of the 128-query kernel (70 KB of LDS each), four of
 * the 16-query one, which only streams -- and never more splits than row tiles or than VH_GALLERY_MAX_SPLITS */
int ga_choose_splits(int n_queries, long n_rows, int cus)
{
    const int qt = ga_query_tile(n_queries);
    const long q_tiles = ((long)n_queries + qt - 1) / qt, want = (long)(qt == GA_QT_SMALL ? 4 : 2) * cus;
    long s = (want + q_tiles - 1) / q_tiles;
    const long tiles = ga_row_tiles(n_rows);
    s = s > tiles ? tiles : s;
    s = s > VH_GALLERY_MAX_SPLITS ? VH_GALLERY_MAX_SPLITS : s;
    return s < 1 ? 1 : (int)s;
}

/* two bf16 values in a dword, exactly as fp32 */
__device__ __forceinline__ float ga_bf16_lo(unsigned b) { return __builtin_bit_cast(float, b << 16); }
__device__ __forceinline__ float ga_bf16_hi(unsigned b) { return __builtin_bit_cast(float, b & 0xFFFF0000u); }

template <int QS, bool BF16>
__global__ __launch_bounds__(GA_THREADS, 2) void gallery_scan_kernel(const float *__restrict__ queries, int n_queries, int E,
                                                                  const void *__restrict__ rows, unsigned n_rows, long row_stride, int k,
                                                                  int splits, int q_tiles, int tiles_per_split, u64 *__restrict__ ws)
{
    constexpr int QT = 16 * QS;
    constexpr int Q_PIECES = (QT * (GA_KC / 4) + GA_THREADS - 1) / GA_THREADS;
    extern __shared__ __attribute__((aligned(16))) float ga_lds[];
    float *const r_s = ga_lds, *const q_s = r_s + GA_RT * GA_LS;
    u64 *const list = reinterpret_cast<u64 *>(q_s + QT * GA_LS);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lg = lane >> 4;
    const int split = blockIdx.x / q_tiles, q0 = (blockIdx.x % q_tiles) * QT;
    const int tiles = (int)((n_rows + GA_RT - 1) / GA_RT), tile_first = split * tiles_per_split;
    const int tile_end = tile_first + tiles_per_split < tiles ? tile_first + tiles_per_split : tiles;
    const int nkc = (E + GA_KC - 1) / GA_KC;

    for (int i = tid; i < QT * k; i += GA_THREADS)
        list[i] = 0ull;                        /* below every key; the first stage's barriers order this before any use */

    /* the stage in flight: (ld_tile, ld_kc) in registers */
    f32x4 rp[GA_ROW_PIECES], qp[Q_PIECES];
    int ld_tile = tile_first, ld_kc = 0;
    auto stage_load = [&]() {
        const int col0 = ld_kc * GA_KC;
        if (BF16) {   /* 16 bytes = 8 columns per lane: piece i is rp[2 i], rp[2 i + 1]; embed_dim % 8 may be 4 */
#pragma unroll
            for (int i = 0; i < GA_ROW_PIECES / 2; ++i) {
                const int p = tid + i * GA_THREADS, col = col0 + 8 * (p & 3);
                const unsigned row = (unsigned)ld_tile * GA_RT + (unsigned)(p >> 2);
                const unsigned short *const src = static_cast<const unsigned short *>(rows) + (size_t)row * (size_t)row_stride + col;
                uint4 b = {0u, 0u, 0u, 0u};
                if (row < n_rows && col + 8 <= E) {
                    b = *reinterpret_cast<const uint4 *>(src);
                } else if (row < n_rows && col < E) {
                    const uint2 h = *reinterpret_cast<const uint2 *>(src);
                    b.x = h.x;
                    b.y = h.y;
                }
                rp[2 * i] = f32x4{ga_bf16_lo(b.x), ga_bf16_hi(b.x), ga_bf16_lo(b.y), ga_bf16_hi(b.y)};
                rp[2 * i + 1] = f32x4{ga_bf16_lo(b.z), ga_bf16_hi(b.z), ga_bf16_lo(b.w), ga_bf16_hi(b.w)};
            }
        } else {
#pragma unroll
            for (int i = 0; i < GA_ROW_PIECES; ++i) {
                const int p = tid + i * GA_THREADS, col = col0 + 4 * (p & 7);
                const unsigned row = (unsigned)ld_tile * GA_RT + (unsigned)(p >> 3);
                rp[i] = row < n_rows && col < E
                            ? *reinterpret_cast<const f32x4 *>(static_cast<const float *>(rows) + (size_t)row * (size_t)row_stride + col)
                            : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            }
        }
#pragma unroll
        for (int i = 0; i < Q_PIECES; ++i) {
            const int p = tid + i * GA_THREADS, col = col0 + 4 * (p & 7), q = q0 + (p >> 3);
            qp[i] = p < QT * (GA_KC / 4) && q < n_queries && col < E
                        ? *reinterpret_cast<const f32x4 *>(queries + (size_t)q * E + col)
                        : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
        if (++ld_kc == nkc) {
            ld_kc = 0;
            ++ld_tile;
        }
    };
    auto stage_store = [&]() {
#pragma unroll
        for (int i = 0; i < GA_ROW_PIECES; ++i) {   /* bf16: lane p of pass i / 2 holds columns 8 (p & 3) + 4 (i & 1) .. of row p >> 2 */
            const int p = tid + (BF16 ? i / 2 : i) * GA_THREADS;
            float *const dst = BF16 ? r_s + (p >> 2) * GA_LS + 8 * (p & 3) + 4 * (i & 1) : r_s + (p >> 3) * GA_LS + 4 * (p & 7);
            *reinterpret_cast<f32x4 *>(dst) = rp[i];
        }
#pragma unroll
        for (int i = 0; i < Q_PIECES; ++i) {
            const int p = tid + i * GA_THREADS;
            if (p < QT * (GA_KC / 4))
                *reinterpret_cast<f32x4 *>(q_s + (p >> 3) * GA_LS + 4 * (p & 7)) = qp[i];
        }
    };

    if (tile_first < tile_end)
        stage_load();
    for (int tile = tile_first; tile < tile_end; ++tile) {
        f32x4 acc[2][QS];
#pragma unroll
        for (int rs = 0; rs < 2; ++rs)
#pragma unroll
            for (int qs = 0; qs < QS; ++qs)
                acc[rs][qs] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int kc = 0; kc < nkc; ++kc) {
            __syncthreads();                   /* the previous stage has been read; this stage's loads have landed */
            stage_store();
            lds_barrier();
            if (ld_tile < tile_end)
                stage_load();                  /* in flight during the matrix instructions below */
            const float *const rr = r_s + (wave * 32 + l15) * GA_LS + 4 * lg, *const qr = q_s + l15 * GA_LS + 4 * lg;
#pragma unroll
            for (int j = 0; j < GA_KC / 16; ++j) {
                const f32x4 r0 = *reinterpret_cast<const f32x4 *>(rr + 16 * j);
                const f32x4 r1 = *reinterpret_cast<const f32x4 *>(rr + 16 * GA_LS + 16 * j);
#pragma unroll
                for (int qs = 0; qs < QS; ++qs) {
                    const f32x4 qf = *reinterpret_cast<const f32x4 *>(qr + qs * 16 * GA_LS + 16 * j);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {   /* result [query 16 qs + 4 lg + r][row 16 rs + l15] */
                        acc[0][qs] = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[e], r0[e], acc[0][qs], 0, 0, 0);
                        acc[1][qs] = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[e], r1[e], acc[1][qs], 0, 0, 0);
                    }
                }
            }
        }
        /* the tile's scores against the running lists */
#pragma unroll
        for (int rs = 0; rs < 2; ++rs) {
            const unsigned row = (unsigned)tile * GA_RT + (unsigned)(wave * 32 + rs * 16 + l15);
#pragma unroll
            for (int qs = 0; qs < QS; ++qs)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ql = 16 * qs + 4 * lg + r;
                    if (row >= n_rows || q0 + ql >= n_queries)
                        continue;
                    u64 *const lq = list + ql * k;
                    u64 carry = rank_key(acc[rs][qs][r], (int)row);
                    if (carry <= __hip_atomic_load(lq + (k - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
                        continue;
                    for (int j = 0; j < k && carry != 0ull; ++j) {
                        const u64 old = __hip_atomic_fetch_max(lq + j, carry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        carry = old < carry ? old : carry;
                    }
                }
        }
    }
    __syncthreads();
    for (int i = tid; i < QT * k; i += GA_THREADS) {
        const int q = q0 + i / k;
        if (q < n_queries)
            ws[((size_t)q * splits + split) * k + i % k] = list[i];
    }
}

/* ws [n][total] keys, 0 = none; at least k of a query's keys are real */
__global__ __launch_bounds__(GA_THREADS) void gallery_merge_kernel(const u64 *__restrict__ ws, int total, int k, int *__restrict__ indices,
                                                                   float *__restrict__ scores)
{
    __shared__ u64 kred[2][GA_THREADS / 64];
    __shared__ u64 win[GA_MAX_K];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 *const src = ws + (size_t)blockIdx.x * total;
    u64 below = ~0ull;
    for (int j = 0; j < k; ++j) {
        u64 best = 0ull;
#pragma unroll 4
        for (int idx = tid; idx < total; idx += GA_THREADS) {
            const u64 c = src[idx];
            best = c < below && c > best ? c : best;
        }
        best = wave_max_key(best);
        if (lane == 0)
            kred[j & 1][wave] = best;            /* two slots, as in topk_kernel */
        __syncthreads();
        const u64 a = kred[j & 1][0], b = kred[j & 1][1], c = kred[j & 1][2], d = kred[j & 1][3];
        const u64 ab = a > b ? a : b, cd = c > d ? c : d;
        below = ab > cd ? ab : cd;
        if (tid == 0)
            win[j] = below;
    }
    __syncthreads();
    if (tid < k) {
        const u64 key = win[tid];
        const unsigned hi = (unsigned)(key >> 32);
        const size_t o = (size_t)blockIdx.x * k + tid;
        indices[o] = (int)(0xFFFFFFFFu - (unsigned)key);
        if (scores)   /* rank_key undone: NaN has no image of its own, and the sum is never -0 */
            scores[o] = __builtin_bit_cast(float, hi == 0u ? 0x7FC00000u : (hi & 0x80000000u) ? hi ^ 0x80000000u : ~hi);
    }
}

template <int QS, bool BF16>
int launch_scan(hipStream_t st, const float *queries, int n, int E, const void *rows, long n_rows, long row_stride, int k, int splits,
                u64 *ws)
{
    constexpr int QT = 16 * QS;
    const int q_tiles = (n + QT - 1) / QT;
    const long tiles = ga_row_tiles(n_rows);
    VH_SET_LDS_ONCE((gallery_scan_kernel<QS, BF16>), ga_lds_bytes(QT, GA_MAX_K));
    hipLaunchKernelGGL((gallery_scan_kernel<QS, BF16>), dim3((unsigned)((size_t)splits * q_tiles)), dim3(GA_THREADS), ga_lds_bytes(QT, k), st,
                       queries, n, E, rows, (unsigned)n_rows, row_stride, k, splits, q_tiles, (int)((tiles + splits - 1) / splits), ws);
    VH_LAUNCH_CHECK("gallery_scan_kernel");
    return 0;
}

} // namespace

extern "C" int vh_gallery_query_tile(int n_queries) { return ga_query_tile(n_queries); }

extern "C" int vh_gallery_splits(int n_queries, long n_rows)
{
    return n_queries < 1 || n_rows < 1 ? 0 : ga_choose_splits(n_queries, n_rows, vh_device_cus(vh_current_device()));
}

extern "C" size_t vh_gallery_workspace(int n_queries, long n_rows, int k, int splits)
{
    static_assert(sizeof(u64) == 8, "csrc/kernel_limits.h sizes the (score, index) pairs");
    return kl_gallery_workspace(n_queries, n_rows, k, splits);   /* splits = 0: whatever ga_choose_splits chooses is at most this */
}

extern "C" int vh_launch_gallery_topk(vh_stream_t s, const float *queries, int n_queries, int embed_dim, const void *rows, int dtype,
                                      long n_rows, long row_stride, int k, int splits, void *workspace, int *indices, float *scores)
{
    if (!queries || !rows || !workspace || !indices)
        return vh_fail(1, "vh_launch_gallery_topk: null pointer argument (queries, rows, workspace, indices)");
    if (dtype != VH_GALLERY_F32 && dtype != VH_GALLERY_BF16)
        return vh_fail(1, "vh_launch_gallery_topk: dtype=%d must be VH_GALLERY_F32 or VH_GALLERY_BF16", dtype);
    if (n_queries < 1)
        return vh_fail(1, "vh_launch_gallery_topk: n_queries=%d must be positive", n_queries);
    if (k < 1 || k > GA_MAX_K || (long)k > n_rows || n_rows > 2147483647L)
        return vh_fail(1, "vh_launch_gallery_topk: k=%d must be in 1..%d and <= n_rows=%ld <= 2^31 - 1", k, GA_MAX_K, n_rows);
    if (embed_dim < 4 || embed_dim > GA_MAX_E || embed_dim % 4 != 0)
        return vh_fail(1, "vh_launch_gallery_topk: embed_dim=%d must be a multiple of 4 in 4..%d", embed_dim, GA_MAX_E);
    const long el = dtype == VH_GALLERY_BF16 ? 2 : 4;
    if (row_stride < embed_dim || row_stride > (1L << 40) || (row_stride * el) % 16 != 0)
        return vh_fail(1, "vh_launch_gallery_topk: row_stride=%ld elements must be >= embed_dim=%d and a multiple of 16 bytes", row_stride,
                       embed_dim);
    if (splits < 0 || splits > VH_GALLERY_MAX_SPLITS)
        return vh_fail(1, "vh_launch_gallery_topk: splits=%d must be in 0..%d (0: chosen here)", splits, VH_GALLERY_MAX_SPLITS);
    if ((((uintptr_t)queries | (uintptr_t)rows | (uintptr_t)workspace | (uintptr_t)indices | (uintptr_t)scores) & 15) != 0)
        return vh_fail(1, "vh_launch_gallery_topk: pointers must be 16-byte aligned");
    if (splits == 0)
        splits = ga_choose_splits(n_queries, n_rows, vh_device_cus(vh_current_device()));
    const int qt = ga_query_tile(n_queries);
    if (((size_t)splits * (size_t)((n_queries + qt - 1) / qt)) >> 31)
        return vh_fail(1, "vh_launch_gallery_topk: n_queries=%d x splits=%d too large for one launch", n_queries, splits);
    hipStream_t st = (hipStream_t)s;
    u64 *const ws = static_cast<u64 *>(workspace);
    int rc;
    if (qt == GA_QT_SMALL)
        rc = dtype == VH_GALLERY_BF16 ? launch_scan<GA_QT_SMALL / 16, true>(st, queries, n_queries, embed_dim, rows, n_rows, row_stride, k, splits, ws)
                                      : launch_scan<GA_QT_SMALL / 16, false>(st, queries, n_queries, embed_dim, rows, n_rows, row_stride, k, splits, ws);
    else
        rc = dtype == VH_GALLERY_BF16 ? launch_scan<GA_QT_LARGE / 16, true>(st, queries, n_queries, embed_dim, rows, n_rows, row_stride, k, splits, ws)
                                      : launch_scan<GA_QT_LARGE / 16, false>(st, queries, n_queries, embed_dim, rows, n_rows, row_stride, k, splits, ws);
    if (rc != 0)
        return rc;
    hipLaunchKernelGGL(gallery_merge_kernel, dim3((unsigned)n_queries), dim3(GA_THREADS), 0, st, ws, splits * k, k, indices, scores);
    VH_LAUNCH_CHECK("gallery_merge_kernel");
    return 0;
}
