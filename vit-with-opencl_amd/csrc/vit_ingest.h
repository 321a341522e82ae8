/*
 * vit_ingest.h -- what a forward reads, and how 8-bit sources of any size lie in a staging slot.  Internal to the library:
 * shared by ViT_hip.c (which owns the device) and vit_ingest.c (which needs none: plain C, its only outside symbol is
 * vh_set_error).
 */
#ifndef VIT_INGEST_H
#define VIT_INGEST_H

#include "ViT_opencl.h"

#include <stddef.h>

/* the largest source side of the resize and box forms */
enum { RESIZE_MAX_SIDE = 16384, ROWMAP_BYTES = RESIZE_MAX_SIDE / 8 };

enum ingest_kind
{
    INGEST_F32,          /* fp32 [C][H][W] images of the model's size */
    INGEST_U8,           /* 8-bit images of the model's size, contiguous, in `layout` */
    INGEST_U8_RESIZED,   /* 8-bit images of any size, each resized and centre-cropped (rc) */
    INGEST_U8_BOXES      /* boxes of 8-bit images of any size, each resized to img x img (filter) */
};

/* One crop of the resize kernel: a source image of which the rows from row0 on are in memory -- data is column 0 of row
 * row0, planes (CHW) plane_stride bytes apart -- and what to take of it: `box` resized to img x img, or with box NULL the
 * whole image resized and centre-cropped by rc. */
struct ingest_item
{
    vit_image_u8 image;
    int row0;
    long plane_stride;
    const float *box;
    const vit_resize_crop *rc;
};

/* What a forward reads.  Exactly the fields of `kind` and of where the data lies are set; the others stay zero. */
struct ingest_src
{
    enum ingest_kind kind;
    int on_device;                   /* the pixel data lies in device memory (the device forms); 0: in the caller's host memory */
    const float *f32;                /* F32, device: [n][C][H][W] */
    const ImageData *host_f32;       /* F32, host: one allocation per image (Network.c:90) */
    const unsigned char *u8;         /* U8: [n] images */
    const vit_image_u8 *images;      /* RESIZED: [n]; BOXES: [n_images] */
    int n_images;                    /* BOXES */
    const vit_resize_crop *rc;       /* RESIZED */
    const vit_box_u8 *boxes;         /* BOXES: [n] */
    int filter;                      /* BOXES: VIT_RESIZE_* (RESIZED carries its own in rc) */
    int layout;                      /* every 8-bit kind: VIT_PIXELS_* */
    const vit_pixel_norm *norm;      /* every 8-bit kind, unless crops_only */
    int crops_only;                  /* the call runs no forward: it needs no norm, and `crops` instead */
    unsigned char *crops;            /* crops_only: where the crops go */
    const struct ingest_item *items; /* RESIZED / BOXES staged by a plan: the chunk's crops, one per output image, read instead
                                      * of images and boxes.  NULL: every image lies whole at its `data` (ingest_whole_item) */
};

/* What the ingest path needs to know of a context */
struct ingest_model
{
    int max_batch, in_chans, img_size;
    int img_width;                   /* 0: square.  Otherwise img_size rows by img_width columns: the resized and the box kinds,
                                      * whose crops are img_size x img_size, are refused */
    size_t slot_bytes;               /* of one staging slot: what a chunk of a host form may pack */
};

/* The argument checks of the u8, resized and box forms that need no device, before anything is queued: 0, or 1 with
 * "who: why", "who: image i: why" or "who: box i: why" as the thread's error text.  model NULL: the call had no context.
 * The device forms take n <= max_batch and aligned u8 data; the host forms instead refuse an image (a box's rows) larger
 * than a staging slot. */
int ingest_check(const char *who, const struct ingest_model *model, const struct ingest_src *src, int n);

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

/* "who: why" as the thread's error text; returns 1 */
int ingest_refuse(const char *who, const char *why);

/* VIT_RESIZE_* of a checked RESIZED or BOXES source */
int ingest_filter(const struct ingest_src *src);

/* Output image i of a RESIZED or BOXES source whose images lie whole in memory */
struct ingest_item ingest_whole_item(const struct ingest_src *src, int i);

/* Fill the kernel's descriptor of one crop of img_size x img_size, its coefficient tables at coef_offset; returns the
 * tables' bytes */
size_t ingest_fill_desc(vh_resize_desc *desc, const struct ingest_item *item, int img_size, int filter, size_t coef_offset);

/* The tables' bytes of one crop at the steepest downscale the checks admit */
size_t ingest_max_table_bytes(int crop);

/* A chunk of a RESIZED or BOXES host form, as it lies in one staging slot.  Its distinct sources lie one behind the other,
 * each as the rows the chunk reads of it -- all of them (map NULL: a whole image of the resized form), or a bit per source
 * row (the box form) -- in row order, at full width and without row padding: HWC rows, or plane after plane for CHW.  The
 * rows one item reads are consecutive there, so every item describes its source from its own first row. */
struct ingest_packed
{
    int image;                   /* index into the caller's images */
    int rows;                    /* rows packed */
    size_t off;                  /* where it starts in the slot */
    unsigned char *map;          /* [ROWMAP_BYTES], or NULL: every row */
};

struct ingest_plan
{
    struct ingest_model model;
    int n_src;                     /* distinct sources of the chunk */
    struct ingest_packed *src;     /* [max_batch] */
    struct ingest_item *items;     /* [max_batch]: data in the device slot */
    size_t bytes;                  /* of the whole chunk */
};

/* The scratch of a call's chunks, one allocation: NULL when out of memory.  Released with ingest_plan_free. */
struct ingest_plan *ingest_plan_new(const struct ingest_model *model, enum ingest_kind kind);
void ingest_plan_free(struct ingest_plan *plan);

/* Plan the chunk that starts at output image `first` of the n of a checked host source, for a slot that will lie at d_slot
 * on the device: at most max_batch items, an item taken while the chunk's bytes with its fresh rows -- rows of its source
 * that no earlier item of the chunk reads; the whole height for a whole image -- stay within slot_bytes.  Returns the
 * items taken (0: the first does not fit, which ingest_check refuses beforehand). */
int ingest_plan_chunk(struct ingest_plan *plan, const struct ingest_src *src, int first, int n, const unsigned char *d_slot);

/* Pack source k of the planned chunk into the host slot that starts at dst */
void ingest_pack(char *dst, const struct ingest_plan *plan, const struct ingest_src *src, int k);

#endif
