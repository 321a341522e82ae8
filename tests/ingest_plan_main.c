/*
 * ingest_plan_main.c -- csrc/vit_ingest.c on its own, without a device: plans and packs chunks of the resized and the box
 * host forms in host memory and checks them against a naive restatement of the rules (a bool per source row), the
 * descriptor fill of the two forms against each other, and the refusals of the shared argument check that a zeroed
 * stand-in context cannot reach.  Built and run by tests/test_ingest_plan_host.py under ASan + UBSan; exit status 0 = every
 * check held.  The "device slot" is an ordinary buffer: the planner is told its address, the packer fills it, and every
 * item's descriptor is then read back through the pointers the kernel would follow.
 */
#include "vit_ingest.h"

#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static char last_error[512];
int vh_set_error(int code, const char *message)
{
    snprintf(last_error, sizeof last_error, "%s", message);
    return code ? code : 1;
}

#define CHECK(cond, ...)                                              \
    do {                                                              \
        if (!(cond)) {                                                \
            fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                             \
            fprintf(stderr, "  [%s]\n", context);                     \
            exit(1);                                                  \
        }                                                             \
    } while (0)

enum { IMG = 8, MAX_BATCH = 4, SLOT = 4096, MAX_H = 200, N_POOL = 7, N_BOXES = 23, N_RESIZED = 11 };

static char context[200];   /* the configuration under test, for a failure's message */
static int byte_cuts, count_cuts, shared_rows;   /* what the cases met, summed over every configuration */

/* height x width of the pool: the four sizes of the cases, two that fit a slot at every channel count, and one of 64-byte
 * rows (C = 1) for the box whose rows are exactly a slot */
static const int POOL_HW[N_POOL][2] = {{40, 30}, {7, 200}, {200, 7}, {64, 64}, {20, 30}, {16, 16}, {80, 64}};

struct pool
{
    vit_image_u8 im[N_POOL];
    unsigned char *mem[N_POOL];
};

static long row_bytes(int layout, int width, int chans) { return layout == VIT_PIXELS_HWC ? (long)width * chans : width; }
static int planes_of(int layout, int chans) { return layout == VIT_PIXELS_HWC ? 1 : chans; }

/* every image with bytes of its own, row padding included, so that a wrong row or copied padding shows */
static void pool_make(struct pool *p, int layout, int chans, int pad)
{
    unsigned state = 12345u + (unsigned)(layout * 7 + chans * 3 + pad);
    for (int i = 0; i < N_POOL; ++i) {
        const int h = POOL_HW[i][0], w = POOL_HW[i][1];
        const long stride = row_bytes(layout, w, chans) + pad;
        const size_t bytes = (size_t)stride * h * planes_of(layout, chans);
        p->mem[i] = malloc(bytes);
        for (size_t b = 0; b < bytes; ++b) {
            state = state * 1664525u + 1013904223u;
            p->mem[i][b] = (unsigned char)(state >> 24);
        }
        p->im[i] = (vit_image_u8){p->mem[i], h, w, stride};
    }
}

static void pool_free(struct pool *p)
{
    for (int i = 0; i < N_POOL; ++i)
        free(p->mem[i]);
}

/* the caller's image and the rows [*row0, *row0 + *count) that output image i of src reads, by the public helpers alone */
static int item_rows(const struct ingest_src *src, int i, int *row0, int *count)
{
    if (src->kind == INGEST_U8_RESIZED) {
        *row0 = 0;
        *count = src->images[i].height;
        return i;
    }
    const vit_box_u8 *b = &src->boxes[i];
    const int rc = vit_box_rows(src->images[b->image].height, b->box[1], b->box[3], IMG, src->filter, row0, count);
    CHECK(rc == 0, "vit_box_rows refused box %d: %s", i, last_error);
    return b->image;
}

/* The greedy rule: items from `first` while there are at most MAX_BATCH and the distinct rows fit the slot.  rows: which
 * rows of which caller's image the chunk holds; returns the items taken and the chunk's bytes. */
static int naive_chunk(const struct ingest_src *src, int n_images, int first, int n, int chans, bool rows[][MAX_H], size_t *bytes)
{
    int m = 0;
    *bytes = 0;
    for (int k = 0; k < n_images; ++k)
        memset(rows[k], 0, MAX_H * sizeof(bool));
    for (; m < MAX_BATCH && first + m < n; ++m) {
        int row0, count, fresh = 0;
        const int image = item_rows(src, first + m, &row0, &count);
        for (int y = row0; y < row0 + count; ++y)
            fresh += !rows[image][y];
        if (*bytes + (size_t)fresh * src->images[image].width * chans > SLOT)
            break;
        shared_rows += count - fresh;
        for (int y = row0; y < row0 + count; ++y)
            rows[image][y] = true;
        *bytes += (size_t)fresh * src->images[image].width * chans;
    }
    return m;
}

/* Plan, pack and read back every chunk of a checked host source of n output images; chunks_out: their sizes */
static int run_source(const struct ingest_model *model, const struct ingest_src *src, int n_images, int n, int chunks_out[])
{
    static bool rows[N_POOL > N_RESIZED ? N_POOL : N_RESIZED][MAX_H];
    static int owner[SLOT];
    const int chans = model->in_chans, planes = planes_of(src->layout, chans);
    unsigned char *slot = malloc(SLOT);   /* exactly a slot: a byte beyond it is the sanitizer's to report */
    struct ingest_plan *plan = ingest_plan_new(model, src->kind);
    CHECK(plan && slot, "out of memory");
    CHECK(ingest_check("case", model, src, n) == 0, "the case's own source was refused: %s", last_error);
    int n_chunks = 0;
    for (int first = 0, m; first < n; first += m) {
        size_t want_bytes;
        const int want_m = naive_chunk(src, n_images, first, n, chans, rows, &want_bytes);
        m = ingest_plan_chunk(plan, src, first, n, slot);
        CHECK(m == want_m && m > 0, "chunk at %d takes %d items, the greedy rule %d", first, m, want_m);
        CHECK(plan->bytes == want_bytes && plan->bytes <= SLOT, "chunk at %d: %zu bytes, the distinct rows have %zu", first, plan->bytes,
              want_bytes);
        byte_cuts += m < MAX_BATCH && first + m < n;
        count_cuts += m == MAX_BATCH;
        chunks_out[n_chunks++] = m;

        memset(slot, 0xA5, SLOT);
        for (int k = 0; k < plan->n_src; ++k)
            ingest_pack((char *)slot, plan, src, k);

        /* every byte an item reads is its own row's, no byte serves two different rows, and no packed byte goes unread */
        for (int b = 0; b < SLOT; ++b)
            owner[b] = -1;
        size_t owned = 0;
        for (int i = 0; i < m; ++i) {
            int row0, count;
            const int image = item_rows(src, first + i, &row0, &count);
            const vit_image_u8 *im = &src->images[image];
            const long row = row_bytes(src->layout, im->width, chans);
            vh_resize_desc d;
            ingest_fill_desc(&d, &plan->items[i], IMG, ingest_filter(src), 0);
            CHECK(d.row0 == row0 && d.height == im->height && d.width == im->width && d.row_stride == row,
                  "item %d: row0 %d height %d width %d row_stride %ld", first + i, d.row0, d.height, d.width, d.row_stride);
            for (int p = 0; p < planes; ++p)
                for (int y = row0; y < row0 + count; ++y) {
                    const unsigned char *got = d.data + (long)(y - row0) * d.row_stride + p * d.plane_stride;
                    const unsigned char *want = im->data + ((long)p * im->height + y) * im->row_stride;
                    CHECK(got >= slot && got + row <= slot + plan->bytes, "item %d plane %d row %d lies outside the chunk's bytes", first + i, p, y);
                    CHECK(memcmp(got, want, (size_t)row) == 0, "item %d plane %d row %d differs from the caller's", first + i, p, y);
                    const int id = (image * 4 + p) * MAX_H + y;
                    for (long b = got - slot; b < got - slot + row; ++b) {
                        CHECK(owner[b] == -1 || owner[b] == id, "slot byte %ld serves two rows", b);
                        owned += owner[b] == -1;
                        owner[b] = id;
                    }
                }
        }
        CHECK(owned == plan->bytes, "%zu bytes read of %zu packed: a row was packed twice or for nobody", owned, plan->bytes);
        /* the planner's own table of sources: distinct images, one behind the other */
        size_t end = 0;
        for (int k = 0; k < plan->n_src; ++k) {
            for (int j = 0; j < k; ++j)
                CHECK(plan->src[j].image != plan->src[k].image, "image %d is packed twice", plan->src[k].image);
            CHECK(plan->src[k].off == end, "source %d starts at %zu, the one before ends at %zu", k, plan->src[k].off, end);
            end += (size_t)plan->src[k].rows * src->images[plan->src[k].image].width * chans;
        }
        CHECK(end == plan->bytes, "the sources end at %zu of %zu", end, plan->bytes);
    }
    ingest_plan_free(plan);
    free(slot);
    return n_chunks;
}

/* 23 boxes of the sources 0 (40 x 30), 1 (7 x 200) and 3 (64 x 64), named out of order: boxes flush to each edge, fractional
 * ones, a tiny one, and neighbours in the list that share rows: 2 and 3 on the 7 x 200 source, whose rows are the widest and
 * whose second box reads no row of its own, so that they share a chunk at every channel count; 0 and 4, 1 and 5, 9 and 12 */
static const vit_box_u8 BOXES[N_BOXES] = {
    {3, {0, 0, 10, 8}},      {0, {0, 0, 30, 12}},      {1, {0, 0, 200, 1}},     {1, {20, 0, 180, 1}},
    {3, {5.5f, 4.25f, 20.5f, 13.75f}}, {0, {10, 5, 25, 15}}, {3, {54, 56, 64, 64}}, {1, {100, 6, 200, 7}},
    {0, {0, 28, 15, 40}},    {3, {0, 30, 64, 38}},     {0, {20, 14, 30, 26}},   {1, {0, 2, 50, 3}},
    {3, {20, 28, 40, 37}},   {0, {3, 3, 9, 9}},        {3, {1, 1, 3, 2.5f}},    {1, {13.3f, 0.5f, 77.7f, 3.5f}},
    {0, {0, 0, 30, 20}},     {3, {32, 10, 48, 20}},    {0, {12.5f, 30, 28, 40}}, {1, {150, 4, 199, 6}},
    {3, {0, 54, 10, 64}},    {0, {5, 18, 22, 31}},     {3, {40, 0, 64, 6}},
};

static void box_cases(const struct ingest_model *model, const struct pool *pool, int layout, int filter)
{
    const vit_pixel_norm norm = {{1, 1, 1, 1}, {0}};
    int chunks[N_BOXES];
    const struct ingest_src src = {.kind = INGEST_U8_BOXES, .images = pool->im, .n_images = N_POOL, .boxes = BOXES, .filter = filter,
                                   .layout = layout, .norm = &norm};
    int sources[N_POOL] = {0}, distinct = 0;
    for (int i = 0; i < N_BOXES; ++i)
        distinct += !sources[BOXES[i].image]++;
    CHECK(distinct == 3, "%d sources", distinct);
    run_source(model, &src, N_POOL, N_BOXES, chunks);

    /* On the 80 x 64 source: the tallest box whose rows fit a slot is accepted -- at 1 and 4 channels its rows are exactly
     * a slot -- and is a chunk of its own; a box that reads one row more is refused by name. */
    const vit_image_u8 *tall = &pool->im[6];
    const int fit = SLOT / (tall->width * model->in_chans);
    vit_box_u8 edge[3] = {BOXES[1], BOXES[5], {6, {0, 0, 0, 0}}};
    bool found_fit = false, found_over = false;
    for (int top = 0; top < 12; ++top)
        for (int bottom = top + 1; bottom <= tall->height; ++bottom) {
            int row0, count;
            CHECK(vit_box_rows(tall->height, (float)top, (float)bottom, IMG, filter, &row0, &count) == 0, "%s", last_error);
            if ((count != fit || found_fit) && (count != fit + 1 || found_over))
                continue;
            edge[2] = (vit_box_u8){6, {3, (float)top, 40, (float)bottom}};
            struct ingest_src one = src;
            one.boxes = edge;
            if (count == fit) {
                found_fit = true;
                if (model->in_chans != 3)
                    CHECK((size_t)count * tall->width * model->in_chans == SLOT, "%d rows are not a slot", count);
                CHECK(run_source(model, &one, N_POOL, 3, chunks) == 2 && chunks[0] == 2 && chunks[1] == 1, "chunks %d %d", chunks[0], chunks[1]);
            } else {
                found_over = true;
                CHECK(ingest_check("who", model, &one, 3) == 1, "a box of %d rows was accepted", count);
                CHECK(strcmp(last_error, "who: box 2: the rows it reads are larger than a staging slot") == 0, "%s", last_error);
                one.on_device = 1;   /* the device form has no slot to fit */
                CHECK(ingest_check("who", model, &one, 3) == 0, "%s", last_error);
            }
        }
    CHECK(found_fit && found_over, "no box of %d and of %d rows", fit, fit + 1);
}

static void resized_cases(const struct ingest_model *model, const struct pool *pool, int layout, int filter)
{
    const vit_pixel_norm norm = {{1, 1, 1, 1}, {0}};
    const vit_resize_crop rc = {IMG, filter};
    vit_image_u8 images[N_RESIZED];
    int chunks[N_RESIZED];
    struct ingest_src src = {.kind = INGEST_U8_RESIZED, .images = images, .rc = &rc, .layout = layout, .norm = &norm};

    /* 11 images that are small next to a slot: cut by count alone, into 4, 4 and 3.  They are windows of the pool's memory
     * (fewer rows and columns at the same stride), so tight rows become padded ones here. */
    for (int i = 0; i < N_RESIZED; ++i) {
        images[i] = pool->im[i % N_POOL];
        images[i].height = 5 + i % 3;
        images[i].width = 7 - i % 3;
    }
    CHECK(run_source(model, &src, N_RESIZED, N_RESIZED, chunks) == 3, "not three chunks");
    CHECK(chunks[0] == 4 && chunks[1] == 4 && chunks[2] == 3, "chunks %d %d %d", chunks[0], chunks[1], chunks[2]);

    /* 11 whole images of the pool, those that fit a slot at this channel count in turn: cut by bytes */
    int fits[N_POOL], n_fit = 0, cuts_before = byte_cuts;
    for (int i = 0; i < N_POOL; ++i)
        if ((size_t)pool->im[i].height * pool->im[i].width * model->in_chans <= SLOT)
            fits[n_fit++] = i;
    CHECK(n_fit >= 2, "%d images fit", n_fit);
    for (int i = 0; i < N_RESIZED; ++i)
        images[i] = pool->im[fits[(i * 3 + i / 4) % n_fit]];
    run_source(model, &src, N_RESIZED, N_RESIZED, chunks);
    CHECK(byte_cuts > cuts_before, "no chunk was cut by bytes");

    /* refusals of the shared check: an image larger than a slot (host form only), a row_stride below the row, resize_short */
    images[1] = pool->im[model->in_chans == 1 ? 6 : 3];
    CHECK(ingest_check("who", model, &src, 3) == 1 && strcmp(last_error, "who: image 1: image larger than a staging slot") == 0, "%s", last_error);
    src.on_device = 1;
    CHECK(ingest_check("who", model, &src, 3) == 0, "%s", last_error);
    src.on_device = 0;
    images[1] = pool->im[5];
    images[2].row_stride = row_bytes(layout, images[2].width, model->in_chans) - 1;
    CHECK(ingest_check("who", model, &src, 3) == 1 && strcmp(last_error, "who: image 2: row_stride below the row's bytes") == 0, "%s", last_error);
    struct ingest_src boxes = {.kind = INGEST_U8_BOXES, .images = images, .n_images = 3, .boxes = BOXES + 1, .filter = filter,
                               .layout = layout, .norm = &norm};
    CHECK(ingest_check("who", model, &boxes, 1) == 1 && strcmp(last_error, "who: image 2: row_stride below the row's bytes") == 0, "%s", last_error);
    for (int rs = IMG - 1; rs <= 4 * IMG + 1; rs += 3 * IMG + 2) {
        const vit_resize_crop bad = {rs, filter};
        src.rc = &bad;
        CHECK(ingest_check("who", model, &src, 2) == 1 && strcmp(last_error, "who: resize_short must be in img_size..4 x img_size") == 0, "%s", last_error);
    }
    struct ingest_model wide = *model;   /* 1024 x 4 bytes per crop row */
    wide.img_size = 1024;
    if (model->in_chans == 4) {
        const vit_resize_crop ok = {1024, filter};
        src.rc = &ok;
        CHECK(ingest_check("who", &wide, &src, 2) == 1 && strcmp(last_error, "who: img_size x in_chans above 3072 bytes per crop row") == 0, "%s", last_error);
        CHECK(ingest_check("who", &wide, &boxes, 1) == 1 && strcmp(last_error, "who: img_size x in_chans above 3072 bytes per crop row") == 0, "%s", last_error);
    }
}

/* A box that is the whole of a square image, and the resize + centre crop of that image at resize_short = img_size, are the
 * same descriptor: as the forms describe a whole image, and as their planners stage it */
static void same_descriptor(const struct ingest_model *model, const struct pool *pool, int layout, int filter)
{
    const vit_pixel_norm norm = {{1, 1, 1, 1}, {0}};
    const vit_resize_crop rc = {IMG, filter};
    for (int which = 3; which <= 5; which += 2) {   /* 64 x 64, and 16 x 16 which fits a slot at every channel count */
        const vit_image_u8 *im = &pool->im[which];
        const vit_box_u8 whole = {0, {0, 0, (float)im->width, (float)im->height}};
        const struct ingest_src as_box = {.kind = INGEST_U8_BOXES, .images = im, .n_images = 1, .boxes = &whole, .filter = filter,
                                          .layout = layout, .norm = &norm};
        const struct ingest_src as_resize = {.kind = INGEST_U8_RESIZED, .images = im, .rc = &rc, .layout = layout, .norm = &norm};
        for (int planned = 0; planned <= (which == 5); ++planned) {
            unsigned char *slot = malloc(SLOT);
            struct ingest_plan *plans[2] = {ingest_plan_new(model, INGEST_U8_BOXES), ingest_plan_new(model, INGEST_U8_RESIZED)};
            const struct ingest_src *srcs[2] = {&as_box, &as_resize};
            vh_resize_desc d[2];
            size_t tables[2];
            CHECK(slot && plans[0] && plans[1], "out of memory");
            for (int f = 0; f < 2; ++f) {
                struct ingest_item item = ingest_whole_item(srcs[f], 0);
                if (planned) {
                    CHECK(ingest_check("case", model, srcs[f], 1) == 0, "%s", last_error);
                    CHECK(ingest_plan_chunk(plans[f], srcs[f], 0, 1, slot) == 1, "the image was not taken");
                    item = plans[f]->items[0];
                }
                memset(&d[f], 0, sizeof d[f]);
                tables[f] = ingest_fill_desc(&d[f], &item, IMG, filter, 4096);
                CHECK(d[f].data == (planned ? slot : im->data), "data is not the start of the image");
                ingest_plan_free(plans[f]);
            }
            free(slot);
            CHECK(tables[0] == tables[1] && d[0].coef_offset == 4096 && d[1].coef_offset == 4096, "tables %zu %zu", tables[0], tables[1]);
            CHECK(d[0].row_stride == d[1].row_stride && d[0].plane_stride == d[1].plane_stride, "strides %ld %ld, %ld %ld", d[0].row_stride,
                  d[1].row_stride, d[0].plane_stride, d[1].plane_stride);
            CHECK(d[0].height == d[1].height && d[0].width == d[1].width && d[0].row0 == d[1].row0, "size or row0");
            CHECK(d[0].x0 == d[1].x0 && d[0].x1 == d[1].x1 && d[0].y0 == d[1].y0 && d[0].y1 == d[1].y1, "span");
            CHECK(d[0].out_w == d[1].out_w && d[0].out_h == d[1].out_h && d[0].left == d[1].left && d[0].top == d[1].top, "out or first");
            CHECK(d[0].kx == d[1].kx && d[0].ky == d[1].ky, "taps %d %d, %d %d", d[0].kx, d[0].ky, d[1].kx, d[1].ky);
        }
    }
}

int main(void)
{
    static const int CHANS[3] = {1, 3, 4};
    for (int c = 0; c < 3; ++c)
        for (int layout = VIT_PIXELS_HWC; layout <= VIT_PIXELS_CHW; ++layout)
            for (int filter = VIT_RESIZE_BILINEAR; filter <= VIT_RESIZE_BICUBIC; ++filter)
                for (int pad = 0; pad <= 5; pad += 5) {
                    const struct ingest_model model = {.max_batch = MAX_BATCH, .in_chans = CHANS[c], .img_size = IMG, .slot_bytes = SLOT};
                    struct pool pool;
                    snprintf(context, sizeof context, "chans %d layout %d filter %d pad %d", CHANS[c], layout, filter, pad);
                    pool_make(&pool, layout, CHANS[c], pad);
                    const int shared_before = shared_rows;
                    box_cases(&model, &pool, layout, filter);
                    CHECK(shared_rows > shared_before, "no two boxes of a chunk shared rows");
                    resized_cases(&model, &pool, layout, filter);
                    same_descriptor(&model, &pool, layout, filter);
                    pool_free(&pool);
                }
    snprintf(context, sizeof context, "all configurations");
    CHECK(byte_cuts > 0 && count_cuts > 0 && shared_rows > 0, "cuts by bytes %d, by count %d, shared rows %d", byte_cuts, count_cuts, shared_rows);
    printf("ingest plan: ok (%d chunks cut by bytes, %d by count, %d shared rows)\n", byte_cuts, count_cuts, shared_rows);
    return 0;
}
