/*
 * vit_requests.h -- the armed outputs of a context (feature, top-k, attention-map, rollout, gallery and dense requests): what
 * is armed, the one way of arming it, and what a forward serves.  Internal to the library: ViT_hip.c holds one struct
 * requests per context and launches what it names.  vit_requests.c is plain C, knows nothing of the context but a struct
 * request_model and launches nothing: its outside symbols are vh_set_error and ingest_refuse, vh_set_device and
 * vh_stream_sync and the allocators vh_malloc, vh_free, vh_host_alloc and vh_host_free; the kernels' shape limits and
 * scratch sizes it checks against are the arithmetic of csrc/kernel_limits.h.
 * tests/requests_main.c runs it over a counting allocator that fails on demand.
 */
#ifndef VIT_REQUESTS_H
#define VIT_REQUESTS_H

#include "ViT_opencl.h"

#include <stddef.h>

enum { FEAT_NONE, FEAT_DEVICE, FEAT_HOST };

/* One array of a host-form forward: written on the device for a chunk, copied into the chunk's pinned slot, scattered into
 * the caller's memory at image `first`.  dev NULL: the array is not asked for. */
struct staged
{
    void *dev, *pinned[2];   /* for max_batch images: the device buffer, and a pinned one per slot */
    char *host;              /* the caller's memory, for all n images of a call ... */
    float **rows;            /* ... or, when set, one row per image instead (the probabilities, Network.c:90) */
    size_t per_image;        /* bytes */
};

/* What arming reads of a context */
struct request_model
{
    int device, max_batch;
    vh_stream_t stream;
    const vit_config *cfg;
    int tokens, qkv_form;    /* plan.tokens, plan.qkv_form */
    size_t ws_bytes;         /* plan.ws_bytes */
};

/* What the six requests share, the first member of each.  The request owns st[].dev, st[].pinned and scratch: request_arm
 * makes them, and frees them when another request takes this one's place or with requests_release. */
struct request
{
    int form;                /* FEAT_NONE, FEAT_DEVICE, FEAT_HOST */
    struct staged st[2];     /* FEAT_HOST: the arrays that come back; an unused one stays zero */
    void *scratch[3];        /* device memory the request's launches work in */
};

/* vit_hip_set_features / _host: the taps resolved to layer indices, and where the embeddings go */
struct feature_req
{
    struct request head;         /* st: cls, pooled */
    vit_feature_spec spec;
    int layer[4];                /* spec.taps resolved, ascending */
    vit_feature_buffers out;     /* FEAT_DEVICE: the caller's device buffers; FEAT_HOST: st[].dev */
};

/* vit_hip_set_topk / _host */
struct topk_req
{
    struct request head;         /* st: labels, scores */
    vit_topk_spec spec;
    vit_topk_buffers out;        /* as feature_req's */
};

/* vit_hip_set_attention / _host */
struct attn_req
{
    struct request head;         /* st: heads, mean */
    vit_attn_spec spec;
    int layer[4];                /* spec.taps resolved, ascending */
    vit_attn_buffers out;
};

/* vit_hip_set_rollout / _host.  The scratch depends on the context alone and is kept from one arming to the next. */
struct rollout_req
{
    struct request head;         /* st: rollout, none; scratch: the running product ping-pongs between [0] and [1], [2] is a
                                  * step's workspace */
    vit_rollout_spec spec;
    int first;                   /* spec.first_layer resolved */
    vit_rollout_buffers out;
};

/* vit_hip_set_gallery / _host.  The scratch depends on the spec (k, n_rows): every arming makes its own. */
struct gallery_req
{
    struct request head;         /* st: indices, scores; scratch: [0] the queries [max_batch][E] fp32, [1]
                                  * vh_launch_gallery_topk's workspace */
    vit_gallery_spec spec;
    int layer;                   /* spec.tap resolved */
    vit_gallery_buffers out;
};

/* vit_hip_set_dense / _host.  Every arming makes its own scratch. */
struct dense_req
{
    struct request head;         /* st: labels, none; scratch: [0] the patch logits, when the caller gives no buffer, [1] the
                                  * normalised tokens, when final_norm is set and the MLP buffer does not hold them */
    vit_dense_spec spec;
    int layer, grid_h, grid_w;   /* spec.tap resolved; the patch grid (vit_config_grid) */
    int out_h, out_w;            /* spec's, 0 resolved to img_size and to the width */
    vit_dense_buffers out;       /* FEAT_HOST: labels = st[0].dev.  Soft-armed: labels may be NULL (no label launch) */
    vit_dense_soft_spec soft;    /* vit_hip_set_dense_soft: the device form with soft maps attached ... */
    vit_dense_soft_buffers soft_out;   /* ... the caller's device buffers; all NULL: not soft-armed */
};

/* The requests of a context, each armed independently of the others, in the order every walk over them takes */
enum { N_REQUESTS = 6, MAX_STAGED = 2 * N_REQUESTS };
struct requests
{
    struct feature_req feat;
    struct topk_req topk;
    struct attn_req amap;
    struct rollout_req roll;
    struct gallery_req gal;
    struct dense_req dense;
};

/* Both forms of arming each request, for the public setter `who`; host: bufs are host memory, staged through device buffers
 * and pinned slots made here.  spec NULL disarms.  On any failure the request armed before stays armed, untouched, and
 * nothing this call allocated is left. */
int requests_set_features(const char *who, const struct request_model *m, struct requests *rq, const vit_feature_spec *spec, const vit_feature_buffers *bufs, int host);
int requests_set_topk(const char *who, const struct request_model *m, struct requests *rq, const vit_topk_spec *spec, const vit_topk_buffers *bufs, int host);
int requests_set_attention(const char *who, const struct request_model *m, struct requests *rq, const vit_attn_spec *spec, const vit_attn_buffers *bufs, int host);
int requests_set_rollout(const char *who, const struct request_model *m, struct requests *rq, const vit_rollout_spec *spec, const vit_rollout_buffers *bufs, int host);
int requests_set_gallery(const char *who, const struct request_model *m, struct requests *rq, const vit_gallery_spec *spec, const vit_gallery_buffers *bufs, int host);
int requests_set_dense(const char *who, const struct request_model *m, struct requests *rq, const vit_dense_spec *spec, const vit_dense_buffers *bufs, int host);
/* vit_hip_set_dense_soft: arms the dense request in device form with the soft maps attached; bufs may be NULL, or its labels */
int requests_set_dense_soft(const char *who, const struct request_model *m, struct requests *rq, const vit_dense_spec *spec,
                            const vit_dense_soft_spec *soft, const vit_dense_buffers *bufs, const vit_dense_soft_buffers *sbufs);

/* what vit_hip_set_dense_soft refuses about soft and the maps, for the soft frame calls to refuse in their own name: NULL, or why */
const char *requests_dense_soft_why(const vit_dense_soft_spec *soft, const vit_dense_soft_buffers *sbufs, int on_device);

/* Everything the six requests own; the caller has made sure that no forward still reads it */
void requests_release(struct requests *rq);

/* The armed requests one forward serves, or NULL */
struct serving
{
    const struct feature_req *fr;
    const struct topk_req *tk;
    const struct attn_req *ar;
    const struct rollout_req *ro;
    const struct gallery_req *ga;
    const struct dense_req *de;
};

/* What a forward of the function `who` serves.  form: what that call can serve -- FEAT_DEVICE, FEAT_HOST, or FEAT_NONE for a
 * call that serves nothing, whatever is armed.  A request armed in the other form refuses the call (1, with the thread's
 * error text), the first in the order of struct requests. */
int requests_serving(const struct requests *rq, const char *who, int form, struct serving *sv);

/* The arrays that come back from a host-form forward: those with a device buffer, request by request, st[0] then st[1] --
 * cls, pooled, labels, scores, heads, mean, rollout, indices, gallery scores, dense labels.  Returns their count. */
int serving_staged(const struct serving *sv, const struct staged *arrays[MAX_STAGED]);

/* A request reads rows of the last layer other than the class token's: that forward runs the last layer on all rows */
int serving_needs_last_layer_rows(const struct serving *sv, int depth);

#endif
