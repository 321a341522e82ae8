/*
 * vit_pipeline.h -- the host-pointer pipeline of a context: the staging slots that host images go up and outputs come back
 * through, the gather into a slot, the chunk loop over the two streams, and beside them the descriptor ring of the resize
 * launches, which obeys the same rule: pinned memory is rewritten only behind its last reader.  Internal to the library:
 * ViT_hip.c holds one struct pipeline per context.  vit_pipeline.c is plain C, knows nothing of the context but a struct
 * pipeline_model and launches nothing -- the forward of a chunk is a callback.  Its outside symbols are vh_set_error and
 * vh_set_device; the allocators vh_malloc, vh_free, vh_host_alloc and vh_host_free; vh_stream_create, _destroy and _sync;
 * vh_event_create, _destroy, _record and _sync and vh_stream_wait_event; the copies vh_h2d and vh_d2h; ingest_plan_chunk
 * and ingest_pack (csrc/vit_ingest.c); and serving_staged (csrc/vit_requests.c).  tests/pipeline_main.c runs it over a
 * model of two in-order streams that defers every queued operation.
 *
 * The protocol, for chunk k in slot s = k & 1 (copy: the pipeline's own stream; compute: the model's):
 *   memory               written by                      read by                          ordered by
 *   h_images[s]          host, gather of chunk k         copy, H2D of chunk k-2           host sync on out_done[s] of chunk k-2
 *   d_images[s]          copy, H2D of chunk k            compute, forward of chunk k-2    copy waits for comp_done[s]
 *   d_images[s]          copy, H2D of chunk k            compute, forward of chunk k      compute waits for up_done[s]
 *   device outputs       compute, forward of chunk k     compute, D2H of chunk k-1        one in-order stream
 *   pinned outputs [s]   compute, D2H of chunk k         host, scatter of chunk k-2       program order: scattered before queued
 *   pinned outputs [s]   compute, D2H of chunk k         host, scatter of chunk k         host sync on out_done[s]
 *   h_desc[i], d_desc[i] host fill, H2D of take j        the H2D and launches of take j-8 host sync on desc_done[i]
 */
#ifndef VIT_PIPELINE_H
#define VIT_PIPELINE_H

#include "vit_ingest.h"
#include "vit_requests.h"

/* resize + crop: descriptor slots in flight */
enum { DESC_RING = 8 };

/* What the pipeline reads of a context */
struct pipeline_model
{
    int device, max_batch, classes;
    vh_stream_t stream;              /* compute: forwards and copies back are queued here */
    size_t image_bytes;              /* of one fp32 image; a staging slot holds max_batch of them */
    float *d_logits, *d_probs;       /* [max_batch][classes]: what a chunk's forward writes */
};

struct pipeline
{
    struct pipeline_model model;
    /* two staging slots, so that gathering + uploading chunk k+1 overlaps the compute of chunk k */
    float *d_images[2], *h_images[2];   /* [max_batch] fp32 images, device and pinned */
    float *h_logits[2], *h_probs[2];    /* [max_batch][classes], pinned */
    vh_stream_t copy_stream;
    vh_event_t up_done[2], comp_done[2], out_done[2];
    /* the per-call descriptors of the resize launches go up through a ring of pinned slots */
    vh_resize_desc *h_desc[DESC_RING], *d_desc[DESC_RING];   /* [max_batch] */
    vh_event_t desc_done[DESC_RING];
    int desc_live[DESC_RING], desc_next;
};

/* Everything above for `model`, on the current device.  On any failure what this call made is freed and *p is zero. */
int pipeline_make(struct pipeline *p, const struct pipeline_model *model);

/* Frees what *p holds -- made, half made or zero -- and leaves it zero; the caller has made sure nothing still reads it */
void pipeline_release(struct pipeline *p);

/* Gather m jobs into the slot at dst on several host threads.  plan NULL: job i is image base + i of src (fp32 images
 * allocated one by one, Network.c:90, or contiguous 8-bit images) of per_image bytes; else job i is source i of the planned
 * chunk (ingest_pack). */
void pipeline_gather(void *dst, const struct ingest_src *src, const struct ingest_plan *plan, int base, int m, size_t per_image);

/* The forward of a chunk of m images from the device source dev into d_logits and, unless NULL, d_probs, serving sv, queued
 * on the model's stream */
typedef int (*pipeline_forward)(void *arg, const struct ingest_src *dev, int m, float *d_logits, float *d_probs, const struct serving *sv);

/* The host-pointer forward of n images of the host source src, in chunks of at most max_batch.  plan: the scratch of the
 * kinds whose chunks are planned (vit_ingest.h), NULL for images of the model's size.  logits ([n][classes]) and probs (a row
 * per image) may be NULL; sv's staged arrays come back too.  On failure both streams have been synchronised. */
int pipeline_run(struct pipeline *p, const struct ingest_src *src, struct ingest_plan *plan, int n, float *logits, float **probs,
                 const struct serving *sv, pipeline_forward forward, void *arg);

/* The next ring slot, once whatever read it last has completed: its pinned and its device descriptors */
int pipeline_desc_take(struct pipeline *p, vh_resize_desc **h_desc, vh_resize_desc **d_desc);

/* The slot taken last is read by what has been queued on s so far */
int pipeline_desc_done(struct pipeline *p, vh_stream_t s);

#endif
