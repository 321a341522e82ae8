/*
 * vit_pipeline.c -- the host-pointer pipeline of a context (csrc/vit_pipeline.h): its slots, streams and events, the gather,
 * the chunk loop and the descriptor ring.  Plain C; nothing here launches a kernel or reads a context.
 */
#include "vit_pipeline.h"

#include <pthread.h>
#include <string.h>

#define TRY(expr)                 \
    do {                          \
        int try_rc_ = (expr);     \
        if (try_rc_ != 0) {       \
            rc = try_rc_;         \
            goto fail;            \
        }                         \
    } while (0)

int pipeline_make(struct pipeline *p, const struct pipeline_model *model)
{
    int rc = 0;
    const size_t mb = (size_t)model->max_batch, out = mb * (size_t)model->classes * sizeof(float);
    memset(p, 0, sizeof *p);
    p->model = *model;
    TRY(vh_stream_create(&p->copy_stream));
    for (int i = 0; i < 2; ++i) {
        TRY(vh_malloc((void **)&p->d_images[i], mb * model->image_bytes));
        TRY(vh_host_alloc((void **)&p->h_images[i], mb * model->image_bytes));
        TRY(vh_host_alloc((void **)&p->h_logits[i], out));
        TRY(vh_host_alloc((void **)&p->h_probs[i], out));
        TRY(vh_event_create(&p->up_done[i]));
        TRY(vh_event_create(&p->comp_done[i]));
        TRY(vh_event_create(&p->out_done[i]));
    }
    for (int i = 0; i < DESC_RING; ++i) {
        TRY(vh_malloc((void **)&p->d_desc[i], mb * sizeof(vh_resize_desc)));
        TRY(vh_host_alloc((void **)&p->h_desc[i], mb * sizeof(vh_resize_desc)));
        TRY(vh_event_create(&p->desc_done[i]));
    }
    return 0;
fail:
    pipeline_release(p);
    return rc;
}

void pipeline_release(struct pipeline *p)
{
    for (int i = 0; i < 2; ++i) {
        if (p->d_images[i]) vh_free(p->d_images[i]);
        if (p->h_images[i]) vh_host_free(p->h_images[i]);
        if (p->h_logits[i]) vh_host_free(p->h_logits[i]);
        if (p->h_probs[i]) vh_host_free(p->h_probs[i]);
        if (p->up_done[i]) vh_event_destroy(p->up_done[i]);
        if (p->comp_done[i]) vh_event_destroy(p->comp_done[i]);
        if (p->out_done[i]) vh_event_destroy(p->out_done[i]);
    }
    for (int i = 0; i < DESC_RING; ++i) {
        if (p->d_desc[i]) vh_free(p->d_desc[i]);
        if (p->h_desc[i]) vh_host_free(p->h_desc[i]);
        if (p->desc_done[i]) vh_event_destroy(p->desc_done[i]);
    }
    if (p->copy_stream)
        vh_stream_destroy(p->copy_stream);
    memset(p, 0, sizeof *p);
}

int pipeline_desc_take(struct pipeline *p, vh_resize_desc **h_desc, vh_resize_desc **d_desc)
{
    const int slot = p->desc_next;
    p->desc_next = (slot + 1) % DESC_RING;
    /* a slot is refilled only once the event behind its last reader has completed */
    const int rc = p->desc_live[slot] ? vh_event_sync(p->desc_done[slot]) : 0;
    if (rc != 0)
        return rc;
    p->desc_live[slot] = 0;
    *h_desc = p->h_desc[slot];
    *d_desc = p->d_desc[slot];
    return 0;
}

int pipeline_desc_done(struct pipeline *p, vh_stream_t s)
{
    const int slot = (p->desc_next + DESC_RING - 1) % DESC_RING;
    const int rc = vh_event_record(p->desc_done[slot], s);
    p->desc_live[slot] = rc == 0;
    return rc;
}

/* Queue the copy of a chunk of m images into its pinned slot */
static int staged_d2h(const struct staged *st, int slot, int m, vh_stream_t s)
{
    return vh_d2h(st->pinned[slot], st->dev, (size_t)m * st->per_image, s);
}

/* A chunk of m images from its pinned slot into the caller's memory, at image `first` */
static void staged_scatter(const struct staged *st, int slot, int first, int m)
{
    if (!st->rows) {
        memcpy(st->host + (size_t)first * st->per_image, st->pinned[slot], (size_t)m * st->per_image);
        return;
    }
    for (int i = 0; i < m; ++i)
        memcpy(st->rows[first + i], (const char *)st->pinned[slot] + (size_t)i * st->per_image, st->per_image);
}

/* The gather runs on several host threads: a single memcpy stream moves ~3 GB/s, which would cap the host-pointer path below
 * the device-resident rate. */
struct gather_job
{
    char *dst;
    const struct ingest_src *src;
    const struct ingest_plan *plan;   /* the jobs are the planned chunk's sources; NULL: the images from `base` on */
    int first, count;                 /* jobs [first, first + count) */
    int base;
    size_t per_image;                 /* plan NULL: bytes */
};

static void *gather_worker(void *arg)
{
    const struct gather_job *j = (const struct gather_job *)arg;
    for (int i = j->first; i < j->first + j->count; ++i) {
        if (j->plan) {
            ingest_pack(j->dst, j->plan, j->src, i);
            continue;
        }
        const void *from = j->src->kind == INGEST_F32 ? (const void *)j->src->host_f32[j->base + i].data
                                                      : (const void *)(j->src->u8 + (size_t)(j->base + i) * j->per_image);
        memcpy(j->dst + (size_t)i * j->per_image, from, j->per_image);
    }
    return NULL;
}

void pipeline_gather(void *dst, const struct ingest_src *src, const struct ingest_plan *plan, int base, int m, size_t per_image)
{
    enum { MAX_THREADS = 8 };
    int nt = m / 16;
    if (nt > MAX_THREADS)
        nt = MAX_THREADS;
    struct gather_job jobs[MAX_THREADS];
    pthread_t tid[MAX_THREADS];
    int started = 0;
    if (nt < 2) {
        struct gather_job all = {.dst = (char *)dst, .src = src, .plan = plan, .first = 0, .count = m, .base = base, .per_image = per_image};
        gather_worker(&all);
        return;
    }
    const int per = (m + nt - 1) / nt;
    for (int t = 0; t < nt; ++t) {
        const int first = t * per, count = first >= m ? 0 : (m - first < per ? m - first : per);
        jobs[t] = (struct gather_job){.dst = (char *)dst, .src = src, .plan = plan, .first = first, .count = count, .base = base, .per_image = per_image};
        if (count == 0)
            break;
        if (t == nt - 1 || pthread_create(&tid[started], NULL, gather_worker, &jobs[t]) != 0)
            gather_worker(&jobs[t]);          /* the last share (or a failed create) runs here */
        else
            ++started;
    }
    for (int t = 0; t < started; ++t)
        pthread_join(tid[t], NULL);
}

/* Software-pipelined over chunks of max_batch images:
 *   host     : gather chunk k into pinned slot k&1   | scatter outputs of chunk k-1
 *   copy strm: H2D chunk k                            (after compute of chunk k-2 released the slot)
 *   compute  : forward chunk k, D2H its outputs       (after the H2D)
 * so PCIe and the gather of the separately malloc'd images (Network.c:90) hide under the previous chunk's kernels.  A u8
 * chunk fills a quarter of a staging slot.  Who orders what: the table in csrc/vit_pipeline.h. */
int pipeline_run(struct pipeline *p, const struct ingest_src *src, struct ingest_plan *plan, int n, float *logits, float **probs,
                 const struct serving *sv, pipeline_forward forward, void *arg)
{
    int rc = 0;
    const struct pipeline_model *pm = &p->model;
    TRY(vh_set_device(pm->device));
    const size_t bytes = src->kind == INGEST_F32 ? pm->image_bytes : pm->image_bytes / sizeof(float);
    const size_t NC = (size_t)pm->classes * sizeof(float);
    /* only what the caller asked for comes back, in the order it is queued: the logits, the probabilities -- the ABI hands
     * them over as one allocation per image (Network.c:90) -- then the served requests' arrays (serving_staged); with neither
     * of the first two, an armed top-k request's pairs are the chunk's whole D2H traffic */
    const struct staged own[2] = {{.dev = pm->d_logits, .pinned = {p->h_logits[0], p->h_logits[1]}, .host = (char *)logits, .per_image = NC},
                                  {.dev = pm->d_probs, .pinned = {p->h_probs[0], p->h_probs[1]}, .rows = probs, .per_image = NC}};
    const struct staged *arrays[2 + MAX_STAGED];
    int n_arrays = 0;
    if (logits)
        arrays[n_arrays++] = &own[0];
    if (probs)
        arrays[n_arrays++] = &own[1];
    n_arrays += serving_staged(sv, arrays + n_arrays);

    int prev_first = 0, prev_m = 0, k = 0;
    for (int first = 0, m = 0; first < n; first += m, ++k) {
        const int s = k & 1;
        /* The chunk, and the device source it becomes once slot s is up.  Images of the model's size: max_batch of them, one
         * gather job per image.  The planned kinds: cut by count and by bytes, one gather job per distinct source, and the
         * device reads the plan's items. */
        struct ingest_src dev = *src;
        dev.on_device = 1;
        m = (n - first < pm->max_batch) ? n - first : pm->max_batch;
        size_t up = (size_t)m * bytes;
        int jobs = m;
        switch (src->kind) {
        case INGEST_F32:
            dev.host_f32 = NULL;
            dev.f32 = p->d_images[s];
            break;
        case INGEST_U8:
            dev.u8 = (const unsigned char *)p->d_images[s];
            break;
        default:
            m = ingest_plan_chunk(plan, src, first, n, (const unsigned char *)p->d_images[s]);
            up = plan->bytes;
            jobs = plan->n_src;
            dev.items = plan->items;
        }
        if (m <= 0) {
            rc = vh_set_error(1, "forward: an image does not fit a staging slot");
            goto fail;
        }
        /* slot s was last used by chunk k-2, whose outputs were waited for below */
        pipeline_gather(p->h_images[s], src, plan, first, jobs, bytes);
        if (k >= 2)
            TRY(vh_stream_wait_event(p->copy_stream, p->comp_done[s]));
        TRY(vh_h2d(p->d_images[s], p->h_images[s], up, p->copy_stream));
        TRY(vh_event_record(p->up_done[s], p->copy_stream));

        TRY(vh_stream_wait_event(pm->stream, p->up_done[s]));
        TRY(forward(arg, &dev, m, pm->d_logits, probs ? pm->d_probs : NULL, sv));
        TRY(vh_event_record(p->comp_done[s], pm->stream));
        for (int a = 0; a < n_arrays; ++a)
            TRY(staged_d2h(arrays[a], s, m, pm->stream));
        TRY(vh_event_record(p->out_done[s], pm->stream));

        if (k >= 1) { /* finish chunk k-1 while chunk k runs */
            TRY(vh_event_sync(p->out_done[s ^ 1]));
            for (int a = 0; a < n_arrays; ++a)
                staged_scatter(arrays[a], s ^ 1, prev_first, prev_m);
        }
        prev_first = first;
        prev_m = m;
    }
    TRY(vh_event_sync(p->out_done[(k - 1) & 1]));
    for (int a = 0; a < n_arrays; ++a)
        staged_scatter(arrays[a], (k - 1) & 1, prev_first, prev_m);
    return 0;
fail:
    vh_stream_sync(p->copy_stream);
    vh_stream_sync(pm->stream);
    return rc;
}
