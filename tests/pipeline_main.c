/*
 * pipeline_main.c -- csrc/vit_pipeline.c on its own, without a device.  The shim underneath it is a deferred-execution model
 * of in-order streams: a copy, an event record, a wait for an event and the forward of a chunk are queued and run later -- under
 * the LAZY schedule only when a host synchronisation forces them (in stream order, through the waits), under the EAGER one
 * as soon as their waits allow.  Device and pinned memory are host blocks of an allocator that counts what is live and fails
 * on demand.  The forward callback queues a closure that, when it runs, hashes what then lies in the chunk's device source
 * and writes values derived from the hash and the image's index into every output; what reaches the caller's memory is held
 * against the same values computed from the caller's inputs.  A mutant switch -- here, never in the product -- turns the k-th
 * vh_stream_wait_event or the k-th vh_event_sync of a run into a no-op, to show which waits a schedule needs.  Built and run
 * by tests/test_pipeline_host.py under ASan + UBSan; exit status 0 = every check held.
 */
#include "vit_pipeline.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(cond, ...)                                               \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                              \
            fprintf(stderr, "\n  [%s]\n", context);                    \
            exit(1);                                                   \
        }                                                              \
    } while (0)

static char context[200];   /* the case under test, for a failure's message */
static char last_error[512];
int vh_set_error(int code, const char *message)
{
    snprintf(last_error, sizeof last_error, "%s", message);
    return code ? code : 1;
}

int vh_set_device(int device) { return device == 0 ? 0 : 1; }

/* ---- the allocator: malloc, every live object on a list with its kind; allocation or create number fail_in from now fails.
 * Fresh memory is 0xa5 throughout: what reads it before its writer ran gets a wrong value, not a random one. ---------- */
enum { DEVICE_BLOCK, PINNED_BLOCK, STREAM_OBJ, EVENT_OBJ, N_KINDS, MAX_LIVE = 256 };
static struct { void *p; int kind; } live_blocks[MAX_LIVE];
static int n_live[N_KINDS], n_allocs, fail_in;

static int block_alloc(void **out, size_t bytes, int kind)
{
    if (fail_in > 0 && --fail_in == 0)
        return vh_set_error(2, "out of memory");
    CHECK(bytes > 0, "an allocation of no bytes");
    for (int i = 0; i < MAX_LIVE; ++i)
        if (!live_blocks[i].p) {
            live_blocks[i].p = *out = malloc(bytes);
            memset(*out, kind == STREAM_OBJ || kind == EVENT_OBJ ? 0 : 0xa5, bytes);
            live_blocks[i].kind = kind;
            ++n_live[kind];
            ++n_allocs;
            return 0;
        }
    CHECK(0, "more than %d live blocks", MAX_LIVE);
    return 1;
}

static int block_free(void *p, int kind)
{
    for (int i = 0; i < MAX_LIVE; ++i)
        if (p && live_blocks[i].p == p && live_blocks[i].kind == kind) {
            free(p);
            live_blocks[i].p = NULL;
            --n_live[kind];
            return 0;
        }
    CHECK(0, "%p freed, which is no live object of kind %d", p, kind);
    return 1;
}

static int all_live(void) { return n_live[DEVICE_BLOCK] + n_live[PINNED_BLOCK] + n_live[STREAM_OBJ] + n_live[EVENT_OBJ]; }

int vh_malloc(void **out, size_t bytes) { return block_alloc(out, bytes, DEVICE_BLOCK); }
int vh_free(void *p) { return block_free(p, DEVICE_BLOCK); }
int vh_host_alloc(void **out, size_t bytes) { return block_alloc(out, bytes, PINNED_BLOCK); }
int vh_host_free(void *p) { return block_free(p, PINNED_BLOCK); }

/* ---- streams and events ---------------------------------------------------------------------------------------------------
 * An event counts its records as they are queued and remembers the last that ran; a wait, like hipStreamWaitEvent and
 * hipEventSynchronize, means the last record queued before it (none: it waits for nothing). */
enum { OP_COPY, OP_RECORD, OP_WAIT, OP_CALL, MAX_OPS = 128, MAX_STREAMS = 4, MAX_CHUNK = 4 };
struct fake_event { int queued, done; };
struct op
{
    int kind;
    void *dst;                /* OP_COPY */
    const void *src;
    size_t bytes;
    struct fake_event *ev;    /* OP_RECORD, OP_WAIT: the event and which of its records */
    int ticket;
    void (*fn)(const struct op *);   /* OP_CALL: a forward's closure or a descriptor reader, over the fields below */
    int m, first;
    const unsigned char *in[MAX_CHUNK];
    size_t in_bytes[MAX_CHUNK];
    float *d_logits, *d_probs;
    const struct serving *sv;
};
struct fake_stream { struct op q[MAX_OPS]; int head, tail, syncs; };

static struct fake_stream *streams[MAX_STREAMS];
static int eager;             /* the schedule */
static int n_copy_calls, fail_copy_in;   /* copy number fail_copy_in from now is refused when it is queued */

/* the mutant: call number mutant_k of its kind does nothing; mutant_site: what that call named */
enum { MUTANT_NONE, MUTANT_WAIT, MUTANT_SYNC };
static int mutant_kind, mutant_k, n_wait_calls, n_sync_calls;
static char mutant_site[100];

static struct pipeline P;     /* the pipeline under test: the fake names a call's stream and event by it */
static struct fake_event *last_out_done;   /* the out_done event recorded last */

static const char *event_name(const struct fake_event *e)
{
    for (int i = 0; i < DESC_RING; ++i) {
        if (i < 2 && e == P.up_done[i]) return "up_done";
        if (i < 2 && e == P.comp_done[i]) return "comp_done";
        if (i < 2 && e == P.out_done[i]) return "out_done";
        if (e == P.desc_done[i]) return "desc_done";
    }
    return "another event";
}

static void run_op(const struct op *op)
{
    switch (op->kind) {
    case OP_COPY: memcpy(op->dst, op->src, op->bytes); break;
    case OP_RECORD: op->ev->done = op->ticket; break;
    case OP_WAIT: CHECK(op->ev->done >= op->ticket, "a wait ran before its record"); break;
    default: op->fn(op);
    }
}

/* eager: every stream runs on while the operation at its head can */
static void pump(void)
{
    for (int progress = 1; progress;) {
        progress = 0;
        for (int i = 0; i < MAX_STREAMS; ++i) {
            struct fake_stream *s = streams[i];
            while (s && s->head < s->tail && !(s->q[s->head].kind == OP_WAIT && s->q[s->head].ev->done < s->q[s->head].ticket)) {
                run_op(&s->q[s->head++]);
                progress = 1;
            }
        }
    }
}

static void force_record(const struct fake_event *e, int ticket, const struct fake_stream *waiter, int depth);

/* what a host synchronisation does: s runs up to and including operation `upto`; a wait first forces the record it names */
static void force(struct fake_stream *s, int upto, int depth)
{
    while (s->head <= upto) {
        const struct op *op = &s->q[s->head];
        if (op->kind == OP_WAIT && op->ev->done < op->ticket)
            force_record(op->ev, op->ticket, s, depth + 1);
        run_op(op);
        ++s->head;
    }
}

static void force_record(const struct fake_event *e, int ticket, const struct fake_stream *waiter, int depth)
{
    CHECK(depth < 8, "waits of %s form a cycle", event_name(e));
    for (int i = 0; i < MAX_STREAMS; ++i)
        for (int k = streams[i] ? streams[i]->head : 0; streams[i] && k < streams[i]->tail; ++k)
            if (streams[i]->q[k].kind == OP_RECORD && streams[i]->q[k].ev == e && streams[i]->q[k].ticket == ticket) {
                CHECK(streams[i] != waiter, "a stream waits for a record of %s queued behind the wait", event_name(e));
                force(streams[i], k, depth);
                return;
            }
    CHECK(0, "record %d of %s is queued nowhere: the wait can never be satisfied", ticket, event_name(e));
}

static struct op *enqueue(vh_stream_t stream, int kind)
{
    struct fake_stream *s = (struct fake_stream *)stream;
    if (s->head == s->tail)
        s->head = s->tail = 0;
    CHECK(s->tail < MAX_OPS, "more than %d operations pending on a stream", MAX_OPS);
    struct op *op = &s->q[s->tail++];
    memset(op, 0, sizeof *op);
    op->kind = kind;
    return op;
}

int vh_stream_create(vh_stream_t *out)
{
    const int rc = block_alloc(out, sizeof(struct fake_stream), STREAM_OBJ);
    for (int i = 0; rc == 0 && i <= MAX_STREAMS; ++i) {
        CHECK(i < MAX_STREAMS, "more than %d streams", MAX_STREAMS);
        if (!streams[i]) {
            streams[i] = (struct fake_stream *)*out;
            break;
        }
    }
    return rc;
}

int vh_stream_destroy(vh_stream_t stream)
{
    struct fake_stream *s = (struct fake_stream *)stream;
    CHECK(s->head == s->tail, "a stream is destroyed with %d operations pending", s->tail - s->head);
    for (int i = 0; i < MAX_STREAMS; ++i)
        if (streams[i] == s)
            streams[i] = NULL;
    return block_free(s, STREAM_OBJ);
}

int vh_stream_sync(vh_stream_t stream)
{
    struct fake_stream *s = (struct fake_stream *)stream;
    ++s->syncs;
    force(s, s->tail - 1, 0);
    return 0;
}

int vh_event_create(vh_event_t *out) { return block_alloc(out, sizeof(struct fake_event), EVENT_OBJ); }
int vh_event_destroy(vh_event_t e) { return block_free(e, EVENT_OBJ); }

int vh_event_record(vh_event_t event, vh_stream_t s)
{
    struct fake_event *e = (struct fake_event *)event;
    struct op *op = enqueue(s, OP_RECORD);
    op->ev = e;
    op->ticket = ++e->queued;
    if (e == P.out_done[0] || e == P.out_done[1])
        last_out_done = e;
    if (eager)
        pump();
    return 0;
}

int vh_stream_wait_event(vh_stream_t s, vh_event_t event)
{
    struct fake_event *e = (struct fake_event *)event;
    if (mutant_kind == MUTANT_WAIT && ++n_wait_calls == mutant_k) {
        snprintf(mutant_site, sizeof mutant_site, "stream_wait(%s, %s)", s == P.copy_stream ? "copy" : s == P.model.stream ? "compute" : "?", event_name(e));
        return 0;
    }
    if (e->queued == 0)
        return 0;
    struct op *op = enqueue(s, OP_WAIT);
    op->ev = e;
    op->ticket = e->queued;
    if (eager)
        pump();
    return 0;
}

int vh_event_sync(vh_event_t event)
{
    const struct fake_event *e = (const struct fake_event *)event;
    if (mutant_kind == MUTANT_SYNC && ++n_sync_calls == mutant_k) {
        const int out = e == P.out_done[0] || e == P.out_done[1];
        snprintf(mutant_site, sizeof mutant_site, "event_sync(%s)%s", event_name(e), !out ? "" : e == last_out_done ? ", the last chunk's" : ", the previous chunk's");
        return 0;
    }
    if (e->done < e->queued)
        force_record(e, e->queued, NULL, 0);
    return 0;
}

static int copy(void *dst, const void *src, size_t bytes, vh_stream_t s)
{
    ++n_copy_calls;
    if (fail_copy_in > 0 && --fail_copy_in == 0)
        return vh_set_error(77, "the copy is refused");
    struct op *op = enqueue(s, OP_COPY);
    op->dst = dst;
    op->src = src;
    op->bytes = bytes;
    if (eager)
        pump();
    return 0;
}

int vh_h2d(void *dst, const void *src, size_t bytes, vh_stream_t s) { return copy(dst, src, bytes, s); }
int vh_d2h(void *dst, const void *src, size_t bytes, vh_stream_t s) { return copy(dst, src, bytes, s); }

/* ---- the model, the served request and the forward ------------------------------------------------------------------------ */
enum { MAX_BATCH = MAX_CHUNK, CHANS = 3, IMG = 4, CLASSES = 5, K = 3, U8_BYTES = CHANS * IMG * IMG, F32_BYTES = 4 * U8_BYTES };
static vh_stream_t compute;
static float *d_logits, *d_probs;
static struct topk_req topk;      /* the hand-made request: two staged arrays of K words per image */
static struct serving serving;    /* .tk = &topk, or nothing */

/* vit_requests.c's, for the one request this program makes by hand (the list of all six: tests/requests_main.c) */
int serving_staged(const struct serving *sv, const struct staged *arrays[MAX_STAGED])
{
    int n = 0;
    for (int k = 0; sv->tk && k < 2; ++k)
        if (sv->tk->head.st[k].dev)
            arrays[n++] = &sv->tk->head.st[k];
    return n;
}

static void model_make(void)
{
    CHECK(vh_stream_create(&compute) == 0 && vh_malloc((void **)&d_logits, MAX_BATCH * CLASSES * 4) == 0 &&
          vh_malloc((void **)&d_probs, MAX_BATCH * CLASSES * 4) == 0, "%s", last_error);
    memset(&topk, 0, sizeof topk);
    for (int k = 0; k < 2; ++k) {
        struct staged *st = &topk.head.st[k];
        st->per_image = K * 4;
        CHECK(vh_malloc(&st->dev, MAX_BATCH * K * 4) == 0 && vh_host_alloc(&st->pinned[0], MAX_BATCH * K * 4) == 0 &&
              vh_host_alloc(&st->pinned[1], MAX_BATCH * K * 4) == 0, "%s", last_error);
    }
    const struct pipeline_model pm = {.device = 0, .max_batch = MAX_BATCH, .classes = CLASSES, .stream = compute, .image_bytes = F32_BYTES,
                                      .d_logits = d_logits, .d_probs = d_probs};
    CHECK(pipeline_make(&P, &pm) == 0, "%s", last_error);
}

static void model_release(void)
{
    vh_stream_sync(P.copy_stream);   /* a mutant may have left operations behind that nothing waited for */
    vh_stream_sync(compute);
    pipeline_release(&P);
    for (int k = 0; k < 2; ++k) {
        vh_free(topk.head.st[k].dev);
        vh_host_free(topk.head.st[k].pinned[0]);
        vh_host_free(topk.head.st[k].pinned[1]);
    }
    vh_free(d_logits);
    vh_free(d_probs);
    vh_stream_destroy(compute);
    CHECK(all_live() == 0, "%d objects are still live", all_live());
}

static uint32_t fnv(uint32_t h, const unsigned char *p, size_t bytes)
{
    for (size_t i = 0; i < bytes; ++i)
        h = (h ^ p[i]) * 16777619u;
    return h;
}

/* word j of output array a (0 logits, 1 probabilities, 2 and 3 the request's) of image g whose source bytes hash to h */
static uint32_t word(uint32_t h, int g, int a, size_t j) { return (h ^ (uint32_t)g * 2654435761u) + (uint32_t)a * 0x01000193u + (uint32_t)j; }

static void write_words(void *dst, uint32_t h, int g, int a, size_t words)
{
    for (size_t j = 0; j < words; ++j) {
        const uint32_t w = word(h, g, a, j);
        memcpy((char *)dst + 4 * j, &w, 4);
    }
}

/* the closure: what the "kernels" of a chunk do when the compute stream reaches them */
static void forward_runs(const struct op *op)
{
    for (int i = 0; i < op->m; ++i) {
        const uint32_t h = fnv(2166136261u, op->in[i], op->in_bytes[i]);
        write_words(op->d_logits + i * CLASSES, h, op->first + i, 0, CLASSES);
        if (op->d_probs)
            write_words(op->d_probs + i * CLASSES, h, op->first + i, 1, CLASSES);
        for (int k = 0; op->sv->tk && k < 2; ++k)
            write_words((char *)op->sv->tk->head.st[k].dev + i * K * 4, h, op->first + i, 2 + k, K);
    }
}

static int n_current, next_image, chunks_seen, cut_by_bytes, fail_forward_at;

/* The callback.  Like the library's forward it reads a planned chunk's items while it is called -- the plan is rewritten for
 * the next chunk -- and the device memory they point into only when its closure runs. */
static int forward(void *arg, const struct ingest_src *dev, int m, float *logits, float *probs, const struct serving *sv)
{
    CHECK(arg == &P && dev->on_device && m >= 1 && m <= MAX_BATCH && next_image + m <= n_current && logits == d_logits && (!probs || probs == d_probs),
          "the callback's arguments");
    if (chunks_seen++ == fail_forward_at)
        return vh_set_error(55, "the forward is refused");
    struct op *op = enqueue(compute, OP_CALL);
    op->fn = forward_runs;
    op->m = m;
    op->first = next_image;
    op->d_logits = logits;
    op->d_probs = probs;
    op->sv = sv;
    for (int i = 0; i < m; ++i) {
        if (dev->kind == INGEST_F32) {
            CHECK(!dev->host_f32, "a device source with host images");
            op->in[i] = (const unsigned char *)dev->f32 + (size_t)i * F32_BYTES;
            op->in_bytes[i] = F32_BYTES;
        } else if (dev->kind == INGEST_U8) {
            op->in[i] = dev->u8 + (size_t)i * U8_BYTES;
            op->in_bytes[i] = U8_BYTES;
        } else {   /* the rows item i reads lie one behind the other from its data on */
            const struct ingest_item *it = &dev->items[i];
            int row0 = 0, rows = it->image.height;
            if (dev->kind == INGEST_U8_BOXES)
                CHECK(vit_box_rows(it->image.height, it->box[1], it->box[3], IMG, dev->filter, &row0, &rows) == 0 && row0 == it->row0, "%s", last_error);
            op->in[i] = it->image.data;
            op->in_bytes[i] = (size_t)rows * it->image.width * CHANS;
        }
    }
    cut_by_bytes += m < MAX_BATCH && next_image + m < n_current;
    next_image += m;
    if (eager)
        pump();
    return 0;
}

/* ---- a caller: its inputs of one kind, its outputs pre-filled, and what they must hold ------------------------------------- */
enum { GUARD = 2, FILL = 0xee, MAX_N = 13, BOX_IMAGES = 3 };
struct caller
{
    int kind, n;
    struct ingest_src src;
    struct ingest_plan *plan;
    ImageData f32[MAX_N];
    unsigned char *u8;
    vit_image_u8 images[MAX_N];
    vit_box_u8 boxes[MAX_N];
    uint32_t hash[MAX_N];          /* of what image g reads of the inputs, computed from the inputs */
    float *logits, *rows[MAX_N + GUARD];
    char *st[2];
};
static const vit_resize_crop resize = {IMG, VIT_RESIZE_BILINEAR};
static const vit_pixel_norm norm = {{1, 1, 1, 1}, {0, 0, 0, 0}};
static unsigned rng = 12345;

static unsigned char *random_bytes(size_t bytes)
{
    unsigned char *p = malloc(bytes);
    for (size_t i = 0; i < bytes; ++i)
        p[i] = (unsigned char)((rng = rng * 1103515245u + 12345u) >> 16);
    return p;
}

/* HWC with five bytes of padding behind each row */
static vit_image_u8 random_image(int height, int width)
{
    return (vit_image_u8){random_bytes((size_t)height * (width * CHANS + 5)), height, width, width * CHANS + 5};
}

static uint32_t rows_hash(const vit_image_u8 *im, int row0, int rows)
{
    uint32_t h = 2166136261u;
    for (int y = row0; y < row0 + rows; ++y)
        h = fnv(h, im->data + (size_t)y * im->row_stride, (size_t)im->width * CHANS);
    return h;
}

/* A slot holds 768 bytes.  The resized kind's images are of 300, 252, 297 and 48 bytes in turn, the box kind's three sources
 * have rows of 30 bytes of which a box reads about twelve: chunks of both are cut by bytes before they are cut by count. */
static void caller_make(struct caller *c, int kind, int n)
{
    static const int sizes[4][2] = {{10, 10}, {12, 7}, {9, 11}, {4, 4}};
    const struct ingest_model model = {.max_batch = MAX_BATCH, .in_chans = CHANS, .img_size = IMG, .slot_bytes = MAX_BATCH * F32_BYTES};
    memset(c, 0, sizeof *c);
    c->kind = kind;
    c->n = n;
    c->src = (struct ingest_src){.kind = kind, .layout = VIT_PIXELS_HWC, .norm = &norm};
    switch (kind) {
    case INGEST_F32:
        for (int g = 0; g < n; ++g) {
            c->f32[g] = (ImageData){n, CHANS, IMG, IMG, (float *)random_bytes(F32_BYTES)};
            c->hash[g] = fnv(2166136261u, (const unsigned char *)c->f32[g].data, F32_BYTES);
        }
        c->src.host_f32 = c->f32;
        c->src.layout = 0;
        c->src.norm = NULL;
        break;
    case INGEST_U8:
        c->src.u8 = c->u8 = random_bytes((size_t)n * U8_BYTES);
        for (int g = 0; g < n; ++g)
            c->hash[g] = fnv(2166136261u, c->u8 + (size_t)g * U8_BYTES, U8_BYTES);
        break;
    case INGEST_U8_RESIZED:
        for (int g = 0; g < n; ++g) {
            c->images[g] = random_image(sizes[g % 4][0], sizes[g % 4][1]);
            c->hash[g] = rows_hash(&c->images[g], 0, c->images[g].height);
        }
        c->src.images = c->images;
        c->src.rc = &resize;
        break;
    default:
        for (int g = 0; g < BOX_IMAGES; ++g)
            c->images[g] = random_image(16, 10);
        for (int g = 0; g < n; ++g) {
            int row0, rows;
            const float top = (float)(g * 3 % 5), bottom = top + 8 + g % 4;
            c->boxes[g] = (vit_box_u8){g % BOX_IMAGES, {(float)(g % 3), top, (float)(6 + g % 5), bottom}};
            CHECK(vit_box_rows(16, top, bottom, IMG, VIT_RESIZE_BILINEAR, &row0, &rows) == 0, "%s", last_error);
            c->hash[g] = rows_hash(&c->images[g % BOX_IMAGES], row0, rows);
        }
        c->src.images = c->images;
        c->src.n_images = BOX_IMAGES;
        c->src.boxes = c->boxes;
        c->src.filter = VIT_RESIZE_BILINEAR;
    }
    if (kind != INGEST_F32)
        CHECK(ingest_check("caller", &model, &c->src, n) == 0, "%s", last_error);
    if (kind == INGEST_U8_RESIZED || kind == INGEST_U8_BOXES)
        CHECK((c->plan = ingest_plan_new(&model, kind)) != NULL, "no plan");
    /* outputs of exactly n images and GUARD more; the probabilities a row per image, each of its own, none past image n */
    c->logits = malloc((size_t)(n + GUARD) * CLASSES * 4);
    memset(c->logits, FILL, (size_t)(n + GUARD) * CLASSES * 4);
    for (int g = 0; g < n; ++g) {
        c->rows[g] = malloc(CLASSES * 4);
        memset(c->rows[g], FILL, CLASSES * 4);
    }
    for (int k = 0; k < 2; ++k) {
        c->st[k] = malloc((size_t)(n + GUARD) * K * 4);
        memset(c->st[k], FILL, (size_t)(n + GUARD) * K * 4);
    }
}

static void caller_free(struct caller *c)
{
    for (int g = 0; g < MAX_N; ++g) {
        free(c->f32[g].data);
        free((void *)c->images[g].data);
        free(c->rows[g]);
    }
    free(c->u8);
    free(c->logits);
    free(c->st[0]);
    free(c->st[1]);
    ingest_plan_free(c->plan);
}

/* words of `got` that differ from array a of images [0, n), and bytes behind them that are no longer FILL */
static int mismatches(const struct caller *c, const char *got, int a, size_t words)
{
    int bad = 0;
    for (int g = 0; g < c->n; ++g)
        for (size_t j = 0; j < words; ++j) {
            const uint32_t want = word(c->hash[g], g, a, j);
            bad += memcmp(got + ((size_t)g * words + j) * 4, &want, 4) != 0;
        }
    for (size_t i = (size_t)c->n * words * 4; i < (size_t)(c->n + GUARD) * words * 4; ++i)
        bad += (unsigned char)got[i] != FILL;
    return bad;
}

enum { WANT_LOGITS = 1, WANT_PROBS = 2, WANT_STAGED = 4 };

/* One pipeline_run of the caller's images under the schedule set; *wrong: how much of the caller's memory is not what it
 * must be (what was not asked for must be untouched).  Returns pipeline_run's code. */
static int run_once(struct caller *c, int want, int *wrong)
{
    memset(&serving, 0, sizeof serving);
    if (want & WANT_STAGED) {
        serving.tk = &topk;
        topk.head.st[0].host = c->st[0];
        topk.head.st[1].host = c->st[1];
    }
    n_current = c->n;
    next_image = chunks_seen = cut_by_bytes = n_copy_calls = n_wait_calls = n_sync_calls = 0;
    mutant_site[0] = 0;
    const int syncs[2] = {((struct fake_stream *)P.copy_stream)->syncs, ((struct fake_stream *)compute)->syncs};
    const int rc = pipeline_run(&P, &c->src, c->plan, c->n, want & WANT_LOGITS ? c->logits : NULL, want & WANT_PROBS ? c->rows : NULL, &serving, forward, &P);
    if (rc != 0) {
        CHECK(((struct fake_stream *)P.copy_stream)->syncs > syncs[0] && ((struct fake_stream *)compute)->syncs > syncs[1],
              "a failed run did not synchronise both streams");
        for (int i = 0; i < MAX_STREAMS; ++i)
            CHECK(!streams[i] || streams[i]->head == streams[i]->tail, "operations are pending behind a failed run");
        return rc;
    }
    CHECK(next_image == c->n, "the forwards covered %d of %d images", next_image, c->n);
    for (int i = 0; i < MAX_STREAMS && mutant_kind == MUTANT_NONE; ++i)
        CHECK(!streams[i] || streams[i]->head == streams[i]->tail, "operations are pending behind a run");
    *wrong = 0;
    for (int a = 0; a < 4; ++a) {
        const size_t words = a < 2 ? CLASSES : K;
        const int asked = a == 0 ? want & WANT_LOGITS : a == 1 ? want & WANT_PROBS : want & WANT_STAGED;
        const char *got = a == 0 ? (const char *)c->logits : a == 1 ? NULL : c->st[a - 2];
        if (a == 1)
            for (int g = 0; g < c->n; ++g)   /* row g alone, with no guard: it is an allocation of its own */
                for (size_t j = 0; j < words; ++j) {
                    const uint32_t w = word(c->hash[g], g, 1, j), fill = 0x01010101u * FILL;
                    *wrong += memcmp((char *)c->rows[g] + 4 * j, asked ? &w : &fill, 4) != 0;
                }
        else if (asked)
            *wrong += mismatches(c, got, a, words);
        else   /* all of it is still FILL */
            for (size_t i = 0; i < (size_t)(c->n + GUARD) * words * 4; ++i)
                *wrong += (unsigned char)got[i] != FILL;
    }
    return 0;
}

static const char *const kind_names[4] = {"fp32", "u8", "resized", "boxes"};
static const char *const schedule_names[2] = {"lazy", "eager"};

static void check_results(void)
{
    static const int ns[] = {1, 4, 5, 8, 9, 13};
    static const int wants[] = {WANT_LOGITS, WANT_PROBS, WANT_LOGITS | WANT_PROBS, 0, WANT_STAGED, WANT_LOGITS | WANT_PROBS | WANT_STAGED, WANT_PROBS | WANT_STAGED};
    int runs = 0;
    for (eager = 0; eager < 2; ++eager)
        for (int kind = 0; kind < 4; ++kind)
            for (size_t i = 0; i < sizeof ns / sizeof ns[0]; ++i)
                for (size_t w = 0; w < sizeof wants / sizeof wants[0]; ++w, ++runs) {
                    struct caller c;
                    int wrong = 0;
                    snprintf(context, sizeof context, "%s, n %d, outputs %d, %s", kind_names[kind], ns[i], wants[w], schedule_names[eager]);
                    model_make();
                    caller_make(&c, kind, ns[i]);
                    CHECK(run_once(&c, wants[w], &wrong) == 0, "%s", last_error);
                    CHECK(wrong == 0, "%d words or guard bytes of the caller's memory are wrong", wrong);
                    CHECK(chunks_seen >= (ns[i] + MAX_BATCH - 1) / MAX_BATCH && (kind < 2 ? chunks_seen == (ns[i] + MAX_BATCH - 1) / MAX_BATCH && !cut_by_bytes
                                                                                        : ns[i] < 5 || cut_by_bytes > 0),
                          "%d chunks, %d of them cut by bytes", chunks_seen, cut_by_bytes);
                    caller_free(&c);
                    model_release();
                }
    eager = 0;
    printf("results: %d runs right\n", runs);
}

/* ---- the descriptor ring: 3 x DESC_RING takes, each read by a copy and a deferred "launch" ------------------------------- */
enum { RING_TAKES = 3 * DESC_RING };
static int ring_seen[RING_TAKES][MAX_BATCH];

static void ring_reader(const struct op *op)
{
    const vh_resize_desc *d = (const vh_resize_desc *)op->src;
    for (int i = 0; i < MAX_BATCH; ++i)
        ring_seen[op->first][i] = d[i].height;
}

/* the readers that did not see the descriptors of their own call */
static int ring_once(void)
{
    int wrong = 0;
    n_sync_calls = 0;
    mutant_site[0] = 0;
    memset(ring_seen, 0, sizeof ring_seen);
    for (int j = 0; j < RING_TAKES; ++j) {
        vh_resize_desc *h, *d;
        CHECK(pipeline_desc_take(&P, &h, &d) == 0, "%s", last_error);
        CHECK(h == P.h_desc[j % DESC_RING] && d == P.d_desc[j % DESC_RING], "take %d did not hand out slot %d", j, j % DESC_RING);
        memset(h, j, MAX_BATCH * sizeof *h);
        for (int i = 0; i < MAX_BATCH; ++i)
            h[i].height = 100 * (j + 1) + i;
        CHECK(vh_h2d(d, h, MAX_BATCH * sizeof *h, compute) == 0, "%s", last_error);
        struct op *op = enqueue(compute, OP_CALL);
        op->fn = ring_reader;
        op->src = d;
        op->first = j;
        if (eager)
            pump();
        CHECK(pipeline_desc_done(&P, compute) == 0 && P.desc_live[j % DESC_RING], "done");
    }
    CHECK(vh_stream_sync(compute) == 0, "sync");
    for (int j = 0; j < RING_TAKES; ++j)
        for (int i = 0; i < MAX_BATCH; ++i)
            wrong += ring_seen[j][i] != 100 * (j + 1) + i;
    return wrong;
}

static void check_ring(void)
{
    for (eager = 0; eager < 2; ++eager) {
        snprintf(context, sizeof context, "the descriptor ring, %s", schedule_names[eager]);
        model_make();
        CHECK(ring_once() == 0, "a reader saw the descriptors of another call");
        CHECK(n_sync_calls == 0 && mutant_kind == MUTANT_NONE, "counters");
        model_release();
    }
    eager = 0;
    printf("ring: %d takes right under both schedules\n", RING_TAKES);
}

/* ---- every wait earns its place --------------------------------------------------------------------------------------------
 * Each vh_stream_wait_event and each vh_event_sync of a four-chunk run (13 fp32 images, everything asked for), and each
 * vh_event_sync of the ring's 24 takes, dropped in turn under both schedules.  Per call site -- the stream and event it names;
 * the host's two syncs on out_done told apart by whether a later chunk has been queued -- the calls dropped and how many of
 * them some schedule turned into a wrong result. */
enum { MAX_SITES = 8 };
static struct { char name[100]; int calls, caught, by[2]; } sites[MAX_SITES];

/* A site no schedule catches, and why it stays */
static const struct { const char *site, *why; } implied[] = {
    {"stream_wait(copy, comp_done)",
     "implied today: before the host queues the H2D of chunk k into slot s it has synchronised on out_done[s] of chunk k-2, which the compute stream "
     "records behind comp_done[s]; the wait stays, so that the device slot stays safe when the host's sync moves (a deferred scatter, a deeper pipeline)"}};

static void site_note(const char *name, const int wrong[2])
{
    int i = 0;
    while (i < MAX_SITES && sites[i].calls && strcmp(sites[i].name, name) != 0)
        ++i;
    CHECK(i < MAX_SITES && name[0], "more than %d call sites, or a mutant that was never reached", MAX_SITES);
    snprintf(sites[i].name, sizeof sites[i].name, "%s", name);
    ++sites[i].calls;
    sites[i].caught += wrong[0] || wrong[1];
    sites[i].by[0] += wrong[0] != 0;
    sites[i].by[1] += wrong[1] != 0;
}

static void check_mutants(void)
{
    const int want = WANT_LOGITS | WANT_PROBS | WANT_STAGED;
    for (int kind = MUTANT_WAIT; kind <= MUTANT_SYNC; ++kind)
        for (int ring = 0; ring < (kind == MUTANT_SYNC ? 2 : 1); ++ring) {
            /* the calls of the unmutated run: counted with a mutant that is never reached */
            int calls = 0;
            for (int k = 0; k <= calls; ++k) {
                int wrong[2] = {0, 0};
                char name[100] = "";
                for (eager = 0; eager < 2; ++eager) {
                    struct caller c;
                    snprintf(context, sizeof context, "mutant: %s %d dropped, %s, %s", kind == MUTANT_WAIT ? "stream wait" : "event sync", k,
                             ring ? "the ring" : "four chunks", schedule_names[eager]);
                    model_make();
                    mutant_kind = kind;
                    mutant_k = k;   /* 0: none */
                    if (ring)
                        wrong[eager] = ring_once();
                    else {
                        caller_make(&c, INGEST_F32, 13);
                        CHECK(run_once(&c, want, &wrong[eager]) == 0 && chunks_seen == 4, "%s", last_error);
                        caller_free(&c);
                    }
                    mutant_kind = MUTANT_NONE;
                    if (k == 0) {
                        calls = kind == MUTANT_WAIT ? n_wait_calls : n_sync_calls;
                        CHECK(wrong[eager] == 0 && calls == (ring ? RING_TAKES - DESC_RING : kind == MUTANT_WAIT ? 6 : 4), "%d calls, %d wrong", calls, wrong[eager]);
                    } else {
                        CHECK(mutant_site[0] && (!name[0] || strcmp(name, mutant_site) == 0), "call %d is '%s' under one schedule, '%s' under the other", k, name, mutant_site);
                        snprintf(name, sizeof name, "%s", mutant_site);
                    }
                    model_release();
                }
                if (k > 0)
                    site_note(name, wrong);
            }
        }
    eager = 0;
    for (int i = 0; i < MAX_SITES && sites[i].calls; ++i) {
        const char *why = NULL;
        for (size_t r = 0; r < sizeof implied / sizeof implied[0]; ++r)
            if (strcmp(implied[r].site, sites[i].name) == 0)
                why = implied[r].why;
        printf("site | %s | dropped %d | caught %d | lazy %d | eager %d | %s\n", sites[i].name, sites[i].calls, sites[i].caught, sites[i].by[0], sites[i].by[1],
               sites[i].caught == sites[i].calls ? "needed" : why ? why : "NOT CAUGHT, AND NO REASON GIVEN");
    }
}

/* ---- clean failure ---------------------------------------------------------------------------------------------------------- */
static void check_make_fails_clean(void)
{
    static const struct pipeline zero;
    const struct pipeline_model pm = {.device = 0, .max_batch = MAX_BATCH, .classes = CLASSES, .stream = &P, .image_bytes = F32_BYTES};
    struct pipeline p;
    const int before = n_allocs;
    snprintf(context, sizeof context, "pipeline_make");
    CHECK(pipeline_make(&p, &pm) == 0, "%s", last_error);
    const int N = n_allocs - before;
    /* the copy stream; per slot a device and three pinned blocks and three events; per ring slot two blocks and an event */
    CHECK(N == 1 + 2 * 7 + DESC_RING * 3 && all_live() == N, "%d allocations and creates, %d live", N, all_live());
    CHECK(n_live[STREAM_OBJ] == 1 && n_live[EVENT_OBJ] == 6 + DESC_RING && n_live[DEVICE_BLOCK] == 2 + DESC_RING && n_live[PINNED_BLOCK] == 6 + DESC_RING, "kinds");
    pipeline_release(&p);
    CHECK(all_live() == 0 && memcmp(&p, &zero, sizeof p) == 0, "release leaves %d objects", all_live());
    pipeline_release(&p);
    for (int k = 1; k <= N; ++k) {
        snprintf(context, sizeof context, "pipeline_make, allocation or create %d of %d fails", k, N);
        memset(&p, 0x5a, sizeof p);
        fail_in = k;
        const int rc = pipeline_make(&p, &pm);
        CHECK(fail_in == 0 && rc == 2, "rc %d", rc);
        CHECK(all_live() == 0 && memcmp(&p, &zero, sizeof p) == 0, "%d objects live, or the struct is not zero", all_live());
        pipeline_release(&p);
        CHECK(all_live() == 0 && memcmp(&p, &zero, sizeof p) == 0, "release of a zero struct does something");
    }
    printf("make: fails clean at each of %d allocations and creates\n", N);
}

/* The callback, then each queued copy, refused at each chunk of a three-chunk run: the code comes back, both streams have
 * been synchronised, nothing is pending, and the next run on the same pipeline is right */
static void check_run_fails_clean(void)
{
    const int want = WANT_LOGITS | WANT_PROBS | WANT_STAGED, copies = 3 * 5;
    int cases = 0;
    for (eager = 0; eager < 2; ++eager)
        for (int kind = 0; kind < 4; kind += 2)
            for (int f = 0; f < 3 + (kind == 0 ? copies : 0); ++f, ++cases) {
                struct caller c, good;
                int wrong = 0;
                snprintf(context, sizeof context, "%s, %s %d refused, %s", kind_names[kind], f < 3 ? "forward" : "copy", f < 3 ? f : f - 3, schedule_names[eager]);
                model_make();
                caller_make(&c, kind, kind == 0 ? 9 : 6);   /* three chunks: 4, 4, 1 images; 300, 252 | 297, 48, 300 | 252 bytes */
                fail_forward_at = f < 3 ? f : -1;
                fail_copy_in = f < 3 ? 0 : f - 3 + 1;
                const int rc = run_once(&c, want, &wrong);
                CHECK(rc == (f < 3 ? 55 : 77) && fail_copy_in == 0, "rc %d", rc);
                CHECK(f < 3 ? chunks_seen == f + 1 : n_copy_calls == f - 3 + 1, "the failure was not where it was meant to be");
                fail_forward_at = -1;
                caller_make(&good, kind, 13);
                CHECK(run_once(&good, want, &wrong) == 0 && wrong == 0, "the run behind the failure: %d wrong", wrong);
                caller_free(&c);
                caller_free(&good);
                model_release();
            }
    /* the refusal of the loop's own, kept with its text and code */
    struct caller c;
    int wrong;
    eager = 0;
    snprintf(context, sizeof context, "an image that fits no slot");
    model_make();
    caller_make(&c, INGEST_U8_RESIZED, 5);
    free((void *)c.images[4].data);
    c.images[4] = random_image(20, 20);   /* 1200 bytes; ingest_check would have refused it */
    CHECK(run_once(&c, want, &wrong) == 1 && strcmp(last_error, "forward: an image does not fit a staging slot") == 0, "'%s'", last_error);
    caller_free(&c);
    model_release();
    printf("run: fails clean in %d cases\n", cases);
}

/* ---- the gather: at every thread count each job lands where it belongs and nothing lands elsewhere -- sources and
 * destinations are allocations of exactly their size, under ASan.  (A job copied twice would leave the same bytes: that no
 * share overlaps another shows only as the shares' arithmetic covering [0, m) with no index out of range.) ------------------ */
static void check_gather(void)
{
    static const int ms[] = {1, 15, 16, 31, 32, 33, 127, 128, 129, 1000};
    enum { PER = 24, BASE = 3, U8_PER = 7, H = 2, W = 3, ROW = W * CHANS };
    for (size_t t = 0; t < sizeof ms / sizeof ms[0]; ++t) {
        const int m = ms[t];
        snprintf(context, sizeof context, "gather of %d jobs", m);
        /* per image: fp32 images allocated one by one, from image BASE on; destinations of exactly m jobs */
        ImageData *im = calloc((size_t)BASE + m, sizeof *im);
        for (int i = 0; i < BASE + m; ++i)
            im[i].data = (float *)random_bytes(PER);
        const struct ingest_src f32 = {.kind = INGEST_F32, .host_f32 = im};
        char *dst = malloc((size_t)m * PER);
        memset(dst, FILL, (size_t)m * PER);
        pipeline_gather(dst, &f32, NULL, BASE, m, PER);
        for (int i = 0; i < m; ++i)
            CHECK(memcmp(dst + (size_t)i * PER, im[BASE + i].data, PER) == 0, "fp32 job %d", i);
        for (int i = 0; i < BASE + m; ++i)
            free(im[i].data);
        free(im);
        free(dst);
        /* per image: contiguous 8-bit images */
        unsigned char *u8 = random_bytes((size_t)(BASE + m) * U8_PER);
        const struct ingest_src src8 = {.kind = INGEST_U8, .u8 = u8};
        dst = malloc((size_t)m * U8_PER);
        pipeline_gather(dst, &src8, NULL, BASE, m, U8_PER);
        CHECK(memcmp(dst, u8 + BASE * U8_PER, (size_t)m * U8_PER) == 0, "u8 jobs");
        free(u8);
        free(dst);
        /* per planned source: m padded images of 2 x 3 pixels, packed without the padding */
        const struct ingest_model model = {.max_batch = m, .in_chans = CHANS, .img_size = IMG, .slot_bytes = (size_t)m * H * ROW};
        vit_image_u8 *images = calloc((size_t)m, sizeof *images);
        for (int i = 0; i < m; ++i)
            images[i] = random_image(H, W);
        const struct ingest_src planned = {.kind = INGEST_U8_RESIZED, .layout = VIT_PIXELS_HWC, .images = images, .rc = &resize, .norm = &norm};
        struct ingest_plan *plan = ingest_plan_new(&model, INGEST_U8_RESIZED);
        CHECK(plan && ingest_plan_chunk(plan, &planned, 0, m, NULL) == m && plan->n_src == m && plan->bytes == (size_t)m * H * ROW, "the plan");
        dst = malloc(plan->bytes);
        memset(dst, FILL, plan->bytes);
        pipeline_gather(dst, &planned, plan, 0, plan->n_src, 0);
        for (int i = 0; i < m; ++i)
            for (int y = 0; y < H; ++y)
                CHECK(memcmp(dst + ((size_t)i * H + y) * ROW, images[i].data + (size_t)y * images[i].row_stride, ROW) == 0, "planned source %d, row %d", i, y);
        for (int i = 0; i < m; ++i)
            free((void *)images[i].data);
        free(images);
        free(dst);
        ingest_plan_free(plan);
    }
    printf("gather: %zu job counts right in both kinds\n", sizeof ms / sizeof ms[0]);
}

int main(void)
{
    fail_forward_at = -1;
    check_make_fails_clean();
    check_gather();
    check_results();
    check_ring();
    check_mutants();
    check_run_fails_clean();
    printf("pipeline: ok (%d allocations)\n", n_allocs);
    return 0;
}
