/*
 * resize.hip -- Pillow-exact resize + centre crop of 8-bit images (vit_hip_resize_crop_u8 and the _resized forwards).
 *
 * The arithmetic is Pillow's Resample.c for 8-bit images: per output index, coefficients computed in double (support =
 * filter support x max(scale, 1); bounds rounded with (int)(v + 0.5); weights normalised by their sum, then converted to
 * int32 with 22 fractional bits), a horizontal pass that rounds to uint8, then a vertical pass on those bytes; each pass
 * is clamp((2^21 + sum u k) >> 22, 0, 255) in int32.  Only the crop's output rows and columns are computed: every output
 * index has its own coefficients, so cropping after resizing is the same thing.
 *
 * Two launches:
 *  - resize_coef_kernel: one thread per (image, axis, crop index) writes the bounds and int32 weights into the caller's
 *    scratch (the MLP hidden buffer inside a forward).  Double precision, in Pillow's operation order; the file is built
 *    with -ffp-contract=off, so no multiply-add is fused (one would change the bicubic weights in the last bit).
 *  - resize_crop_kernel<JN, R, LAYOUT>: one 256-thread workgroup per (image, band of R output rows).  The band's input rows
 *    [ymin of its first row, ymax of its last) are streamed in chunks (source row y lies at row y - row0 of the
 *    descriptor's data: a caller may hold only the rows that the crop reads): each chunk's horizontal pass (crop columns only)
 *    lands as uint8 rows in LDS, and the vertical pass adds the chunk's taps into int32 registers -- thread t owns crop
 *    bytes t, t + 256, ... (JN of them) of each of the R rows.  Chunks add into the same accumulators, so an extreme
 *    downscale (16384 -> 224 bicubic: 293 taps) takes as many chunks as it needs with the LDS fixed at 32 KiB.
 *    The horizontal pass reads source bytes with byte loads: adjacent lanes read adjacent bytes of the same rows, which
 *    the load unit merges into whole cache lines, at any alignment of the image, its rows or its planes.
 */
#include "kernelHandler.h"
#include "vit_kernels.h"

#include <cstdint>

namespace {

enum { LAYOUT_HWC = 0, LAYOUT_CHW = 1 };   /* VIT_PIXELS_* */
enum { THREADS = 256, HBUF_BYTES = 32768, ACC_REGS = 48, MAX_JN = 12 };
static_assert(MAX_JN * THREADS == VH_RESIZE_MAX_ROW_BYTES, "the callers' limit on crop x chans");

/* Pillow's filters (Resample.c), a = -0.5 for bicubic */
__device__ __forceinline__ double bilinear_filter(double x)
{
    if (x < 0.0)
        x = -x;
    if (x < 1.0)
        return 1.0 - x;
    return 0.0;
}

__device__ __forceinline__ double bicubic_filter(double x)
{
    const double a = -0.5;
    if (x < 0.0)
        x = -x;
    if (x < 1.0)
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0)
        return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

__device__ __forceinline__ double filter_at(int filter, double x) { return filter ? bicubic_filter(x) : bilinear_filter(x); }

__device__ __forceinline__ unsigned char clip8(int ss)
{
    const int v = ss >> 22;   /* arithmetic shift */
    return (unsigned char)(v < 0 ? 0 : v > 255 ? 255 : v);
}

struct Tables
{
    const int2 *xb, *yb;
    const int *wx, *wy;
};

__device__ __forceinline__ Tables tables(const char *coef, const vh_resize_desc &d, int crop)
{
    const char *base = coef + d.coef_offset;
    Tables t;
    t.xb = reinterpret_cast<const int2 *>(base);
    t.yb = t.xb + crop;
    t.wx = reinterpret_cast<const int *>(t.yb + crop);
    t.wy = t.wx + (size_t)d.kx * crop;
    return t;
}

/* One thread per (image, axis, crop index): Pillow's precompute_coeffs(in, in0, in1, out) + normalize_coeffs_8bpc for
 * output index left + o (x) or top + o (y).  in1 - in0 is a float subtraction, as in Pillow; a whole image (in0 = 0, in1 =
 * (float)in) gives scale = (double)(float)in / out and center = 0.0 + x = x. */
__global__ void resize_coef_kernel(const vh_resize_desc *__restrict__ desc, char *__restrict__ coef, int n, int crop, int filter)
{
    const int per_image = (2 * crop + THREADS - 1) / THREADS;
    const int img = blockIdx.x / per_image;
    const int o = (blockIdx.x - img * per_image) * THREADS + threadIdx.x;
    if (img >= n || o >= 2 * crop)
        return;
    const vh_resize_desc d = desc[img];
    const int axis = o >= crop, i = axis ? o - crop : o;
    const int in = axis ? d.height : d.width, out = axis ? d.out_h : d.out_w;
    const float in0 = axis ? d.y0 : d.x0, in1 = axis ? d.y1 : d.x1;
    const int xx = i + (axis ? d.top : d.left), ksize = axis ? d.ky : d.kx;
    char *base = coef + d.coef_offset;
    int2 *bounds = reinterpret_cast<int2 *>(base) + (axis ? crop : 0);
    int *wx = reinterpret_cast<int *>(reinterpret_cast<int2 *>(base) + 2 * crop);
    int *wy = wx + (size_t)d.kx * crop;

    const double scale = (double)(in1 - in0) / out;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = (filter ? 2.0 : 1.0) * filterscale;
    const double center = (double)in0 + (xx + 0.5) * scale;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0)
        xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in)
        xmax = in;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x)
        ww += filter_at(filter, (x + xmin - center + 0.5) * ss);
    for (int x = 0; x < ksize; ++x) {
        double w = x < xmax ? filter_at(filter, (x + xmin - center + 0.5) * ss) : 0.0;
        if (ww != 0.0)
            w /= ww;
        const int k = w < 0 ? (int)(-0.5 + w * (1 << 22)) : (int)(0.5 + w * (1 << 22));
        if (axis)
            wy[(size_t)i * ksize + x] = k;
        else
            wx[(size_t)x * crop + i] = k;
    }
    bounds[i] = make_int2(xmin, xmax);
}

/* One workgroup per (image, band of R crop rows).  JN = ceil(crop * chans / 256) crop bytes per thread and row. */
template <int JN, int R, int LAYOUT>
__global__ __launch_bounds__(THREADS) void resize_crop_kernel(const vh_resize_desc *__restrict__ desc, const char *__restrict__ coef,
                                                              int chans, int crop, unsigned char *__restrict__ out)
{
    __shared__ unsigned char hbuf[HBUF_BYTES];
    const int bands = (crop + R - 1) / R;
    const int img = blockIdx.x / bands, r0 = (blockIdx.x - img * bands) * R;
    const vh_resize_desc d = desc[img];
    const Tables t = tables(coef, d, crop);
    const int SC = crop * chans, rows = crop - r0 < R ? crop - r0 : R;
    const int tid = threadIdx.x;

    int ylo = t.yb[r0].x, yhi = 0;
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (r < rows) {
            const int2 b = t.yb[r0 + r];
            ylo = b.x < ylo ? b.x : ylo;
            yhi = b.x + b.y > yhi ? b.x + b.y : yhi;
        }

    int acc[R][JN];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int jj = 0; jj < JN; ++jj)
            acc[r][jj] = 1 << 21;

    const int chunk = HBUF_BYTES / SC;
    const size_t step = LAYOUT == LAYOUT_CHW ? 1 : (size_t)chans;
    for (int y0 = ylo; y0 < yhi; y0 += chunk) {
        const int ch = yhi - y0 < chunk ? yhi - y0 : chunk;
        __syncthreads();   /* the previous chunk's rows have been read */
        /* horizontal pass: crop columns of input rows [y0, y0 + ch) -> uint8 rows in LDS */
        for (int e = tid; e < ch * SC; e += THREADS) {
            const int rr = e / SC, j = e - rr * SC;
            const int col = j / chans, c = j - col * chans;
            const int2 b = t.xb[col];
            const unsigned char *src = LAYOUT == LAYOUT_CHW
                                           ? d.data + (size_t)c * d.plane_stride + (size_t)(y0 + rr - d.row0) * d.row_stride + b.x
                                           : d.data + (size_t)(y0 + rr - d.row0) * d.row_stride + (size_t)b.x * chans + c;
            const int *w = t.wx + col;
            int ss = 1 << 21;
            for (int k = 0; k < b.y; ++k)
                ss += (int)src[k * step] * w[(size_t)k * crop];
            hbuf[e] = clip8(ss);
        }
        __syncthreads();
        /* vertical pass: the chunk's taps of every band row into the accumulators */
        for (int rr = 0; rr < ch; ++rr) {
            const int yy = y0 + rr;
            int h[JN];
#pragma unroll
            for (int jj = 0; jj < JN; ++jj) {
                const int j = tid + THREADS * jj;
                h[jj] = j < SC ? (int)hbuf[rr * SC + j] : 0;
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int2 b = t.yb[r0 + (r < rows ? r : 0)];
                const int k = yy - b.x;
                if (r < rows && k >= 0 && k < b.y) {
                    const int w = t.wy[(size_t)(r0 + r) * d.ky + k];
#pragma unroll
                    for (int jj = 0; jj < JN; ++jj)
                        acc[r][jj] += h[jj] * w;
                }
            }
        }
    }

    unsigned char *dst = out + ((size_t)img * crop + r0) * SC;
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (r < rows)
#pragma unroll
            for (int jj = 0; jj < JN; ++jj) {
                const int j = tid + THREADS * jj;
                if (j < SC)
                    dst[(size_t)r * SC + j] = clip8(acc[r][jj]);
            }
}

template <int JN>
constexpr int band_rows() { return ACC_REGS / JN < 16 ? ACC_REGS / JN : 16; }

template <int JN>
hipError_t launch_crop(hipStream_t s, int layout, const vh_resize_desc *desc, const char *coef, int n, int chans, int crop,
                       unsigned char *out)
{
    constexpr int R = band_rows<JN>();
    const dim3 grid((unsigned)((size_t)n * ((crop + R - 1) / R)));
    if (layout == LAYOUT_CHW)
        hipLaunchKernelGGL((resize_crop_kernel<JN, R, LAYOUT_CHW>), grid, dim3(THREADS), 0, s, desc, coef, chans, crop, out);
    else
        hipLaunchKernelGGL((resize_crop_kernel<JN, R, LAYOUT_HWC>), grid, dim3(THREADS), 0, s, desc, coef, chans, crop, out);
    return hipGetLastError();
}

} // namespace

extern "C" int vh_launch_resize_crop_u8(vh_stream_t s, const vh_resize_desc *desc, int n, int chans, int layout, int filter, int crop,
                                        void *coef, size_t coef_bytes, unsigned char *out)
{
    if (!desc || !coef || !out || n <= 0 || chans < 1 || chans > 4 || crop <= 0 || (layout != LAYOUT_HWC && layout != LAYOUT_CHW) ||
        (filter != 0 && filter != 1))
        return vh_fail(1, "vh_launch_resize_crop_u8: bad argument");
    const int jn = (crop * chans + THREADS - 1) / THREADS;
    if (jn > MAX_JN)
        return vh_fail(1, "vh_launch_resize_crop_u8: crop x chans above %d bytes per row", MAX_JN * THREADS);
    (void)coef_bytes;   /* the caller sized the scratch from the descriptors' kx, ky (see vit_hip_resize_crop_u8) */
    hipStream_t st = (hipStream_t)s;
    const unsigned per_image = (unsigned)((2 * crop + THREADS - 1) / THREADS);
    hipLaunchKernelGGL(resize_coef_kernel, dim3(per_image * (unsigned)n), dim3(THREADS), 0, st, desc, static_cast<char *>(coef), n,
                       crop, filter);
    VH_LAUNCH_CHECK("resize_coef_kernel");
    const char *cf = static_cast<const char *>(coef);
    hipError_t e;
    switch (jn) {
    case 1: e = launch_crop<1>(st, layout, desc, cf, n, chans, crop, out); break;
    case 2: e = launch_crop<2>(st, layout, desc, cf, n, chans, crop, out); break;
    case 3: e = launch_crop<3>(st, layout, desc, cf, n, chans, crop, out); break;
    case 4: e = launch_crop<4>(st, layout, desc, cf, n, chans, crop, out); break;
    case 5: e = launch_crop<5>(st, layout, desc, cf, n, chans, crop, out); break;
    case 6: e = launch_crop<6>(st, layout, desc, cf, n, chans, crop, out); break;
    case 7: e = launch_crop<7>(st, layout, desc, cf, n, chans, crop, out); break;
    case 8: e = launch_crop<8>(st, layout, desc, cf, n, chans, crop, out); break;
    case 9: e = launch_crop<9>(st, layout, desc, cf, n, chans, crop, out); break;
    case 10: e = launch_crop<10>(st, layout, desc, cf, n, chans, crop, out); break;
    case 11: e = launch_crop<11>(st, layout, desc, cf, n, chans, crop, out); break;
    default: e = launch_crop<12>(st, layout, desc, cf, n, chans, crop, out); break;
    }
    if (e != hipSuccess)
        return vh_hip_status(e, "resize_crop_kernel");
    return 0;
}
