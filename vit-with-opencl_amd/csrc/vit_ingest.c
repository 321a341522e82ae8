/*
 * vit_ingest.c -- everything about 8-bit sources that needs no device: the public helpers that are pure arithmetic
 * (pixel normalisation, resize + crop geometry, boxes and their rows, tilings), the one argument check of the u8, resized
 * and box forms, the fill of the resize kernel's descriptor, and the planner and packer of the host forms' staging slots.
 * Plain C11; the only symbol it takes from the rest of the library is vh_set_error, so a program without a device can
 * link it (tests/ingest_plan_main.c does, under the sanitizers).
 */
#include "vit_ingest.h"

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* Pillow's ksize: taps per output index of one axis, the span [in0, in1) -> out (the subtraction in float, as in Pillow) */
static int span_taps(float in0, float in1, int out, int filter)
{
    const double scale = (double)(in1 - in0) / out;
    const double support = (filter == VIT_RESIZE_BICUBIC ? 2.0 : 1.0) * (scale < 1.0 ? 1.0 : scale);
    return (int)ceil(support) * 2 + 1;
}

/* a whole axis (in -> out) */
static int resize_taps(int in, int out, int filter)
{
    return span_taps(0.0f, (float)in, out, filter);
}

/* bicubic taps at the steepest downscale a crop x crop crop can see: the short side 16384 -> resize_short >= crop, the
 * long side's truncated size makes its scale at most 16384 / (crop - 1) */
static int resize_max_taps(int crop)
{
    return resize_taps(RESIZE_MAX_SIDE, crop > 1 ? crop - 1 : 1, VIT_RESIZE_BICUBIC);
}

/* one image's coefficient tables (include/kernelHandler.h, vh_resize_desc) */
static size_t resize_table_bytes(int crop, int kx, int ky)
{
    return align_up((size_t)crop * 16 + ((size_t)kx + ky) * crop * 4, 16);
}

size_t ingest_max_table_bytes(int crop)
{
    return resize_table_bytes(crop, resize_max_taps(crop), resize_max_taps(crop));
}

int vit_pixel_norm_from_mean_std(vit_pixel_norm *out, const float *mean, const float *std, int chans)
{
    if (!out || !mean || !std || chans < 1 || chans > 4)
        return vh_set_error(1, "vit_pixel_norm_from_mean_std: NULL argument, or chans not in 1..4");
    for (int ch = 0; ch < chans; ++ch)
        if (!(std[ch] > 0.0f) || !isfinite(std[ch]) || !isfinite(mean[ch]))
            return vh_set_error(1, "vit_pixel_norm_from_mean_std: std must be positive and finite, mean finite");
    memset(out, 0, sizeof(*out));
    for (int ch = 0; ch < chans; ++ch) {
        out->scale[ch] = (float)(1.0 / (255.0 * (double)std[ch]));
        out->bias[ch] = (float)(-(double)mean[ch] / (double)std[ch]);
    }
    return 0;
}

int vit_resize_crop_geometry(int height, int width, const vit_resize_crop *rc, int crop, int *resized_h, int *resized_w, int *top,
                             int *left)
{
    char msg[200];
    const char *why = !rc || !resized_h || !resized_w || !top || !left ? "NULL argument"
                      : crop <= 0 ? "crop must be positive"
                      : height < 1 || width < 1 || height > RESIZE_MAX_SIDE || width > RESIZE_MAX_SIDE ? "height and width must be in 1..16384"
                      : rc->filter != VIT_RESIZE_BILINEAR && rc->filter != VIT_RESIZE_BICUBIC ? "filter must be VIT_RESIZE_BILINEAR or VIT_RESIZE_BICUBIC"
                      : rc->resize_short < crop || (long long)rc->resize_short > 4LL * crop ? "resize_short must be in crop..4 x crop"
                      : NULL;
    if (why) {
        snprintf(msg, sizeof msg, "vit_resize_crop_geometry: %s", why);
        return vh_set_error(1, msg);
    }
    /* torchvision's _compute_resized_output_size: the short side becomes resize_short, the long one
     * int(resize_short * long / short); CenterCrop: int(round((size - crop) / 2.0)), Python's round (half to even) */
    const long long rs = rc->resize_short;
    const int nh = height <= width ? (int)rs : (int)((double)(rs * height) / width);
    const int nw = height <= width ? (int)((double)(rs * width) / height) : (int)rs;
    *resized_h = nh;
    *resized_w = nw;
    *top = (int)nearbyint((nh - crop) / 2.0);
    *left = (int)nearbyint((nw - crop) / 2.0);
    return 0;
}

/* "who: why" as the thread's error text; returns 1 */
int ingest_refuse(const char *who, const char *why)
{
    char msg[200];
    snprintf(msg, sizeof msg, "%s: %s", who, why);
    return vh_set_error(1, msg);
}

/* ---- boxes: regions of 8-bit images, each resized to img x img as Pillow's Image.resize(size, resample, box=) ---- */

/* NULL, or why `box` is not a box of a height x width image.  Written so that a NaN fails its comparison. */
static const char *box_why(int height, int width, const float box[4])
{
    return !box ? "NULL box"
           : height < 1 || width < 1 || height > RESIZE_MAX_SIDE || width > RESIZE_MAX_SIDE ? "height and width must be in 1..16384"
           : !isfinite(box[0]) || !isfinite(box[1]) || !isfinite(box[2]) || !isfinite(box[3]) ? "box values must be finite"
           : !(box[0] >= 0.0f) || !(box[1] >= 0.0f) || !(box[2] <= (float)width) || !(box[3] <= (float)height) ? "box outside the image"
           : !(box[2] - box[0] >= 1.0f) || !(box[3] - box[1] >= 1.0f) ? "box narrower or lower than 1 px"
           : NULL;
}

int vit_box_check(int height, int width, const float box[4])
{
    const char *why = box_why(height, width, box);
    return why ? ingest_refuse("vit_box_check", why) : 0;
}

/* Pillow's bounds of output index xx of one axis: the first source index read and how many (resize_coef_kernel's own
 * arithmetic, csrc/resize.hip; this file too is built without fused multiply-adds) */
static void span_bounds(int in, float in0, float in1, int out, int filter, int xx, int *first, int *taps)
{
    const double scale = (double)(in1 - in0) / out;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = (filter == VIT_RESIZE_BICUBIC ? 2.0 : 1.0) * filterscale;
    const double center = (double)in0 + (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0)
        xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in)
        xmax = in;
    *first = xmin;
    *taps = xmax - xmin;
}

/* the rows [first, first + count) that the `out` output rows of a validated span read */
static void box_rows(int height, float top, float bottom, int out, int filter, int *first, int *count)
{
    int lo = height, hi = 0;
    for (int yy = 0; yy < out; ++yy) {
        int ymin, taps;
        span_bounds(height, top, bottom, out, filter, yy, &ymin, &taps);
        lo = ymin < lo ? ymin : lo;
        hi = ymin + taps > hi ? ymin + taps : hi;
    }
    *first = lo;
    *count = hi - lo;
}

int vit_box_rows(int height, float top, float bottom, int out, int filter, int *first, int *count)
{
    const float box[4] = {0.0f, top, 1.0f, bottom};
    const char *why = !first || !count ? "NULL argument"
                      : out < 1 ? "out must be positive"
                      : filter != VIT_RESIZE_BILINEAR && filter != VIT_RESIZE_BICUBIC ? "filter must be VIT_RESIZE_BILINEAR or VIT_RESIZE_BICUBIC"
                      : box_why(height, 1, box);
    if (why)
        return ingest_refuse("vit_box_rows", why);
    box_rows(height, top, bottom, out, filter, first, count);
    return 0;
}

int vit_tile_boxes(int height, int width, int tile, int stride, int image, vit_box_u8 *out, int capacity)
{
    const char *why = height < 1 || width < 1 || height > RESIZE_MAX_SIDE || width > RESIZE_MAX_SIDE ? "height and width must be in 1..16384"
                      : tile < 1 || tile > height || tile > width ? "tile must be in 1..min(height, width)"
                      : stride < 1 || stride > tile ? "stride must be in 1..tile"
                      : image < 0 ? "image must not be negative"
                      : capacity < 0 || (capacity > 0 && !out) ? "NULL out, or a negative capacity"
                      : NULL;
    if (why) {
        ingest_refuse("vit_tile_boxes", why);
        return -1;
    }
    /* tiles at 0, stride, ... while they fit; one more, flush to the far edge, when the last of those stops short of it */
    const int ny = (height - tile) / stride + 1 + ((height - tile) % stride != 0);
    const int nx = (width - tile) / stride + 1 + ((width - tile) % stride != 0);
    for (int ty = 0, k = 0; ty < ny; ++ty)
        for (int tx = 0; tx < nx; ++tx, ++k) {
            if (k >= capacity)
                continue;
            const int y = ty * stride + tile > height ? height - tile : ty * stride;
            const int x = tx * stride + tile > width ? width - tile : tx * stride;
            out[k].image = image;
            out[k].box[0] = (float)x, out[k].box[1] = (float)y;
            out[k].box[2] = (float)(x + tile), out[k].box[3] = (float)(y + tile);
        }
    return ny * nx;
}

/* ---- what a forward reads: the checks, the kernel's descriptor, the staging slot of the host forms ---- */

int ingest_filter(const struct ingest_src *src)
{
    return src->kind == INGEST_U8_RESIZED ? src->rc->filter : src->filter;
}

/* bytes of one row of one plane of a width-wide image */
static long row_bytes(int layout, int width, int chans)
{
    return layout == VIT_PIXELS_HWC ? (long)width * chans : (long)width;
}

int ingest_check(const char *who, const struct ingest_model *model, const struct ingest_src *src, int n)
{
    char msg[240];
    const int kind = src->kind, sized = kind != INGEST_U8, host = !src->on_device;
    const void *pixels = sized ? (const void *)src->images : (const void *)src->u8;
    const int null = !model || !pixels || (kind == INGEST_U8_RESIZED && !src->rc) || (kind == INGEST_U8_BOXES && !src->boxes) ||
                     (src->crops_only ? !src->crops : !src->norm);
    const int filter = null || !sized ? 0 : ingest_filter(src);
    /* One chain in the order every form had (a non-square model refuses the sized kinds first: their crops are square).  The u8 forms: NULL, n, max_batch (device), layout, channels, alignment (device).
     * The resized forms: NULL, n, max_batch (device), layout, filter, channels, crop row, resize_short.  The box forms: NULL,
     * n, n_images, max_batch (device), layout, filter, channels, crop row.  An arm that is not a form's own is guarded by
     * `sized` (resized and boxes) or by the kind, so it cannot fire for another form. */
    const char *why = null                                                                     ? (sized ? "NULL argument" : "NULL context, images or norm")
                      : sized && model->img_width != 0
                          ? "the context's input is non-square: the resize and box forms make square crops"
                      : n <= 0                                                                 ? "n must be positive"
                      : kind == INGEST_U8_BOXES && src->n_images <= 0                          ? "n_images must be positive"
                      : !host && n > model->max_batch                                          ? "n exceeds the context's max_batch"
                      : src->layout != VIT_PIXELS_HWC && src->layout != VIT_PIXELS_CHW         ? "layout must be VIT_PIXELS_HWC or VIT_PIXELS_CHW"
                      : sized && filter != VIT_RESIZE_BILINEAR && filter != VIT_RESIZE_BICUBIC ? "filter must be VIT_RESIZE_BILINEAR or VIT_RESIZE_BICUBIC"
                      : model->in_chans > 4                                                    ? "8-bit images take at most 4 channels"
                      : !sized && !host && ((uintptr_t)src->u8 & 15)                           ? "device images must be 16-byte aligned"
                      : sized && (long)model->img_size * model->in_chans > VH_RESIZE_MAX_ROW_BYTES
                          ? "img_size x in_chans above 3072 bytes per crop row"
                      : kind == INGEST_U8_RESIZED && (src->rc->resize_short < model->img_size || src->rc->resize_short > 4 * model->img_size)
                          ? "resize_short must be in img_size..4 x img_size"
                      : NULL;
    const char *what = NULL;
    int bad = -1;
    if (!why && sized) {
        const int C = model->in_chans, n_images = kind == INGEST_U8_BOXES ? src->n_images : n;
        what = "image";
        for (int i = 0; i < n_images && !why; ++i) {
            const vit_image_u8 *im = &src->images[i];
            why = !im->data ? "NULL image data"
                  : im->height < 1 || im->width < 1 || im->height > RESIZE_MAX_SIDE || im->width > RESIZE_MAX_SIDE ? "height and width must be in 1..16384"
                  : im->row_stride < row_bytes(src->layout, im->width, C) ? "row_stride below the row's bytes"
                  : host && kind == INGEST_U8_RESIZED && (size_t)im->height * im->width * C > model->slot_bytes ? "image larger than a staging slot"
                  : NULL;
            bad = i;
        }
        for (int i = 0; kind == INGEST_U8_BOXES && i < n && !why; ++i) {
            const vit_box_u8 *b = &src->boxes[i];
            what = "box";
            bad = i;
            if (b->image < 0 || b->image >= n_images) {
                why = "image index outside 0..n_images - 1";
                break;
            }
            const vit_image_u8 *im = &src->images[b->image];
            why = box_why(im->height, im->width, b->box);
            if (!why && host) {
                int first, count;
                box_rows(im->height, b->box[1], b->box[3], model->img_size, src->filter, &first, &count);
                if ((size_t)count * im->width * C > model->slot_bytes)
                    why = "the rows it reads are larger than a staging slot";
            }
        }
    }
    if (!why)
        return 0;
    if (bad >= 0)
        snprintf(msg, sizeof msg, "%s: %s %d: %s", who, what, bad, why);
    else
        snprintf(msg, sizeof msg, "%s: %s", who, why);
    return vh_set_error(1, msg);
}

struct ingest_item ingest_whole_item(const struct ingest_src *src, int i)
{
    const float *box = src->kind == INGEST_U8_BOXES ? src->boxes[i].box : NULL;
    const vit_image_u8 *im = &src->images[box ? src->boxes[i].image : i];
    return (struct ingest_item){.image = *im, .row0 = 0, .plane_stride = (long)im->height * im->row_stride, .box = box, .rc = src->rc};
}

size_t ingest_fill_desc(vh_resize_desc *e, const struct ingest_item *item, int img_size, int filter, size_t coef_offset)
{
    const vit_image_u8 *im = &item->image;
    e->data = im->data;
    e->row_stride = im->row_stride;
    e->plane_stride = item->plane_stride;
    e->height = im->height;
    e->width = im->width;
    e->row0 = item->row0;
    if (item->box) {   /* Image.resize((img, img), box=): every output index, from 0 */
        const float *b = item->box;
        e->x0 = b[0], e->y0 = b[1], e->x1 = b[2], e->y1 = b[3];
        e->out_w = e->out_h = img_size;
        e->left = e->top = 0;
    } else {           /* the whole image to the resized size, of which the centre crop's indices */
        vit_resize_crop_geometry(im->height, im->width, item->rc, img_size, &e->out_h, &e->out_w, &e->top, &e->left);
        e->x0 = e->y0 = 0.0f;
        e->x1 = (float)im->width, e->y1 = (float)im->height;
    }
    e->kx = span_taps(e->x0, e->x1, e->out_w, filter);
    e->ky = span_taps(e->y0, e->y1, e->out_h, filter);
    e->coef_offset = (long)coef_offset;
    return resize_table_bytes(img_size, e->kx, e->ky);
}

struct ingest_plan *ingest_plan_new(const struct ingest_model *model, enum ingest_kind kind)
{
    const size_t mb = (size_t)model->max_batch, maps = kind == INGEST_U8_BOXES ? mb * ROWMAP_BYTES : 0;
    /* one block: the plan, its sources, its items (all of 8-byte members), the boxes' row bitmaps */
    struct ingest_plan *plan = malloc(sizeof(*plan) + mb * (sizeof(*plan->src) + sizeof(*plan->items)) + maps);
    if (!plan)
        return NULL;
    *plan = (struct ingest_plan){.model = *model, .src = (struct ingest_packed *)(plan + 1)};
    plan->items = (struct ingest_item *)(plan->src + mb);
    for (size_t k = 0; k < mb; ++k)   /* a whole image never touches a row bitmap */
        plan->src[k].map = maps ? (unsigned char *)(plan->items + mb) + k * ROWMAP_BYTES : NULL;
    return plan;
}

void ingest_plan_free(struct ingest_plan *plan)
{
    free(plan);
}

static int map_bit(const unsigned char *map, int y)
{
    return map[y >> 3] >> (y & 7) & 1;
}

/* where the chunk holds caller's image `image`; n_src: not yet */
static int find_source(const struct ingest_plan *plan, int image)
{
    int k = 0;
    while (k < plan->n_src && plan->src[k].image != image)
        ++k;
    return k;
}

int ingest_plan_chunk(struct ingest_plan *plan, const struct ingest_src *src, int first, int n, const unsigned char *d_slot)
{
    const size_t C = (size_t)plan->model.in_chans;
    const int boxes = src->kind == INGEST_U8_BOXES;
    int m = 0;
    plan->n_src = 0;
    plan->bytes = 0;
    for (; m < plan->model.max_batch && first + m < n; ++m) {
        struct ingest_item *it = &plan->items[m];
        *it = ingest_whole_item(src, first + m);   /* completed below, once the sources' row counts are final */
        const int image = boxes ? src->boxes[first + m].image : first + m;
        int k = plan->n_src, count = it->image.height, fresh = count;   /* a whole image: a source of its own, every row */
        if (boxes) {
            k = find_source(plan, image);
            box_rows(it->image.height, it->box[1], it->box[3], plan->model.img_size, src->filter, &it->row0, &count);
            fresh = 0;
            for (int y = it->row0; y < it->row0 + count; ++y)
                fresh += k == plan->n_src || !map_bit(plan->src[k].map, y);
        }
        if (plan->bytes + (size_t)fresh * it->image.width * C > plan->model.slot_bytes)
            break;
        struct ingest_packed *ps = &plan->src[k];
        if (k == plan->n_src) {
            ++plan->n_src;
            ps->image = image;
            ps->rows = 0;
            if (boxes)
                memset(ps->map, 0, ROWMAP_BYTES);
        }
        for (int y = it->row0; boxes && y < it->row0 + count; ++y)
            ps->map[y >> 3] |= (unsigned char)(1 << (y & 7));
        ps->rows += fresh;
        plan->bytes += (size_t)fresh * it->image.width * C;
    }
    size_t off = 0;
    for (int k = 0; k < plan->n_src; ++k) {
        plan->src[k].off = off;
        off += (size_t)plan->src[k].rows * src->images[plan->src[k].image].width * C;
    }
    for (int i = 0; i < m; ++i) {
        struct ingest_item *it = &plan->items[i];
        const struct ingest_packed *ps = &plan->src[boxes ? find_source(plan, src->boxes[first + i].image) : i];
        const long row = row_bytes(src->layout, it->image.width, (int)C);
        int rank = 0;
        for (int y = 0; boxes && y < it->row0; ++y)   /* packed rows of the source ahead of the item's first */
            rank += map_bit(ps->map, y);
        it->image = (vit_image_u8){d_slot + ps->off + (size_t)rank * row, it->image.height, it->image.width, row};
        it->plane_stride = (long)ps->rows * row;
    }
    return m;
}

void ingest_pack(char *dst, const struct ingest_plan *plan, const struct ingest_src *src, int k)
{
    const struct ingest_packed *ps = &plan->src[k];
    const vit_image_u8 *im = &src->images[ps->image];
    const int planes = src->layout == VIT_PIXELS_HWC ? 1 : plan->model.in_chans;
    const size_t row = (size_t)row_bytes(src->layout, im->width, plan->model.in_chans);
    dst += ps->off;
    if (!ps->map && (size_t)im->row_stride == row) {   /* every row, and no padding between them */
        memcpy(dst, im->data, row * im->height * planes);
        return;
    }
    for (int p = 0; p < planes; ++p)   /* the rows packed, in order, HWC rows or plane after plane */
        for (int y = 0; y < im->height; ++y)
            if (!ps->map || map_bit(ps->map, y)) {
                memcpy(dst, im->data + ((size_t)p * im->height + y) * im->row_stride, row);
                dst += row;
            }
}
