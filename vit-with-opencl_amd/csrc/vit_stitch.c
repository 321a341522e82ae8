/*
 * vit_stitch.c -- the host side of vh_launch_dense_stitch (include/kernelHandler.h) that needs no device: the windows of a
 * frame, checked (vit_stitch_check), and binned per block of frame pixels (vit_stitch_index), which tells every block which
 * windows to look at.  Both are public and declared in include/ViT_opencl.h, where the Python ABI table finds them; the
 * launcher and the frame calls use them from there.  Plain C, no device, no allocation; its outside symbols are
 * vit_box_check and ingest_refuse (vit_ingest.c).  tests/stitch_index_main.c runs it on its own under ASan + UBSan against
 * a per-pixel restatement.
 */
#include "ViT_opencl.h"
#include "vit_ingest.h"

#include <stdio.h>

enum { STITCH_MAX_SIDE = 16384 };

static int refuse(const char *who, const char *fmt, long a, long b)
{
    char why[160];
    snprintf(why, sizeof why, fmt, a, b);
    return ingest_refuse(who ? who : "vit_stitch_check", why);
}

int vit_stitch_check(int frame_h, int frame_w, const float *boxes, int n, const char *who)
{
    if (!boxes)
        return refuse(who, "NULL windows", 0, 0);
    if (frame_h < 1 || frame_w < 1 || frame_h > STITCH_MAX_SIDE || frame_w > STITCH_MAX_SIDE)
        return refuse(who, "frame %ld x %ld must be in 1..16384 each way", frame_h, frame_w);
    if (n < 1)
        return refuse(who, "n_windows=%ld must be positive", n, 0);
    for (int i = 0; i < n; ++i)
        if (vit_box_check(frame_h, frame_w, boxes + 4 * (size_t)i))   /* its message names vit_box_check: say whose window it is */
            return refuse(who, "window %ld is not a box of the frame (finite, inside it, at least 1 px each way)", i, 0);
    return 0;
}

/* the first pixel whose centre is >= v, for 0 <= v <= 16384: (int)v or the one after it */
static int first_centre_at_or_after(float v)
{
    const int x = (int)v;
    return (float)x + 0.5f >= v ? x : x + 1;
}

/* The pixels X of an axis whose centre (float)X + 0.5f lies in [lo, hi), as a range [*first, *end): the fp32 comparisons of
 * the kernel's coverage test, so the index and the kernel agree on every pixel.  0 <= lo < hi <= 16384. */
static void stitch_span(float lo, float hi, int *first, int *end)
{
    *first = first_centre_at_or_after(lo);   /* centre >= lo */
    *end = first_centre_at_or_after(hi);     /* the first centre that is not < hi */
}

long vit_stitch_index(int frame_h, int frame_w, int block, const float *boxes, int n, int *offsets, int *ids, long capacity)
{
    static const char who[] = "vit_stitch_index";
    if (block < 1 || block > STITCH_MAX_SIDE) {
        refuse(who, "block=%ld must be in 1..16384", block, 0);
        return -1;
    }
    if (vit_stitch_check(frame_h, frame_w, boxes, n, who))
        return -1;
    if (ids && (!offsets || capacity < 0)) {
        refuse(who, "ids without offsets, or a negative capacity", 0, 0);
        return -1;
    }
    const int bx_n = (frame_w + block - 1) / block, by_n = (frame_h + block - 1) / block;
    const long blocks = (long)bx_n * by_n;
    /* pass 1: how many windows per block; without offsets only their sum */
    long total = 0;
    if (offsets)
        for (long k = 0; k <= blocks; ++k)
            offsets[k] = 0;
    for (int w = 0; w < n; ++w) {
        const float *b = boxes + 4 * (size_t)w;
        int x0, x1, y0, y1;
        stitch_span(b[0], b[2], &x0, &x1);
        stitch_span(b[1], b[3], &y0, &y1);
        if (x0 >= x1 || y0 >= y1)
            continue;   /* not reached for a checked box: a side of 1 px or more holds a centre */
        const int bx0 = x0 / block, bx1 = (x1 - 1) / block, by0 = y0 / block, by1 = (y1 - 1) / block;
        total += (long)(bx1 - bx0 + 1) * (by1 - by0 + 1);
        if (total > 2147483647L) {
            refuse(who, "2^31 ids or more (%ld windows)", n, 0);
            return -1;
        }
        if (offsets)
            for (int by = by0; by <= by1; ++by)
                for (int bx = bx0; bx <= bx1; ++bx)
                    ++offsets[(long)by * bx_n + bx + 1];
    }
    if (offsets)
        for (long k = 0; k < blocks; ++k)
            offsets[k + 1] += offsets[k];
    if (!ids)
        return total;
    if (total > capacity) {
        refuse(who, "%ld ids do not fit a capacity of %ld", total, capacity);
        return -1;
    }
    /* pass 2: windows in ascending order, so every block's ids ascend; offsets[k] walks to the block's end and is moved
     * back afterwards */
    for (int w = 0; w < n; ++w) {
        const float *b = boxes + 4 * (size_t)w;
        int x0, x1, y0, y1;
        stitch_span(b[0], b[2], &x0, &x1);
        stitch_span(b[1], b[3], &y0, &y1);
        if (x0 >= x1 || y0 >= y1)
            continue;
        const int bx0 = x0 / block, bx1 = (x1 - 1) / block, by0 = y0 / block, by1 = (y1 - 1) / block;
        for (int by = by0; by <= by1; ++by)
            for (int bx = bx0; bx <= bx1; ++bx)
                ids[offsets[(long)by * bx_n + bx]++] = w;
    }
    for (long k = blocks; k > 0; --k)
        offsets[k] = offsets[k - 1];
    offsets[0] = 0;
    return total;
}
