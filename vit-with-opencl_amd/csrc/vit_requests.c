/*
 * vit_requests.c -- the armed outputs of a context (csrc/vit_requests.h): the six spec checks and the public size
 * functions, request_arm -- the one owner of every allocation and every free of a request -- the six setters around it
 * (the dense request's has a second entry that attaches the soft maps), and what a forward serves.  Plain C; nothing here launches a kernel or reads a context.
 */
#include "vit_requests.h"
#include "kernel_limits.h"
#include "vit_ingest.h"

#include <stdint.h>
#include <stdio.h>
#include <string.h>

/* The six in the order every walk over them takes: how a refusal names a request, its public setter (vit_hip_set_...), and
 * where it lies in struct requests */
static const struct { const char *what, *setter; size_t at; } kinds[N_REQUESTS] = {
    {"feature", "features", offsetof(struct requests, feat)},   {"top-k", "topk", offsetof(struct requests, topk)},
    {"attention", "attention", offsetof(struct requests, amap)}, {"rollout", "rollout", offsetof(struct requests, roll)},
    {"gallery", "gallery", offsetof(struct requests, gal)},      {"dense", "dense", offsetof(struct requests, dense)}};

/* request r of the table: its head is its first member */
static struct request *request_at(const struct requests *rq, int r) { return (struct request *)((char *)rq + kinds[r].at); }

/* The device buffer for max_batch images of st->per_image bytes and the two pinned slots; what a failure leaves behind,
 * staged_release frees */
static int staged_alloc(int max_batch, struct staged *st)
{
    const size_t bytes = (size_t)max_batch * st->per_image;
    int rc = vh_malloc(&st->dev, bytes);
    for (int slot = 0; slot < 2 && rc == 0; ++slot)
        rc = vh_host_alloc(&st->pinned[slot], bytes);
    return rc;
}

static void staged_release(struct staged *st)
{
    if (st->dev) vh_free(st->dev);
    st->dev = NULL;
    for (int slot = 0; slot < 2; ++slot) {
        if (st->pinned[slot]) vh_host_free(st->pinned[slot]);
        st->pinned[slot] = NULL;
    }
}

/* A request's staging, and with `scratch` its scratch (0: another request holds those buffers now) */
static void request_release(struct request *r, int scratch)
{
    staged_release(&r->st[0]);
    staged_release(&r->st[1]);
    for (int k = 0; scratch && k < 3; ++k) {
        if (r->scratch[k])
            vh_free(r->scratch[k]);
        r->scratch[k] = NULL;
    }
}

void requests_release(struct requests *rq)
{
    for (int r = 0; r < N_REQUESTS; ++r)
        request_release(request_at(rq, r), 1);
}

/* What every setter does behind its own checks.  cand: the new request, `size` bytes with its head first -- zero to disarm;
 * the host form has named the caller's memory and the bytes per image of the arrays it wants.  scratch_bytes: of the device
 * scratch it wants (0: none), `oom` the refusal when that cannot be had.  keep: a request armed over an armed one takes over
 * its scratch and makes none (the sizes depend on the context alone); otherwise every arming makes its own.  Every
 * allocation and every free of a request happens here: on failure what this call made is freed and *armed is untouched; on
 * success the armed request's staging is released, its scratch unless cand took it over, and cand becomes *armed. */
static int request_arm(const char *who, const struct request_model *m, struct request *armed, struct request *cand, size_t size,
                       const size_t scratch_bytes[3], int keep, const char *oom)
{
    const int kept = keep && cand->form != FEAT_NONE && armed->scratch[0] != NULL;
    int rc = vh_set_device(m->device);
    /* the staging and the scratch of the armed request may still be read by its last forward */
    rc = rc ? rc : vh_stream_sync(m->stream);
    for (int k = 0; k < 2 && rc == 0; ++k)
        if (cand->st[k].host)
            rc = staged_alloc(m->max_batch, &cand->st[k]);
    for (int k = 0; k < 3 && rc == 0 && !kept; ++k)
        if (scratch_bytes[k] && vh_malloc(&cand->scratch[k], scratch_bytes[k]))
            rc = ingest_refuse(who, oom);
    if (rc != 0) {
        request_release(cand, 1);
        return rc;
    }
    if (kept)
        memcpy(cand->scratch, armed->scratch, sizeof cand->scratch);
    request_release(armed, !kept);
    memcpy(armed, cand, size);
    return 0;
}

static const size_t no_scratch[3];

/* What the spec checks of a feature and of an attention-map request share; NULL, or why not: the config and the count of taps ... */
static const char *taps_count_check(const vit_config *cfg, int n_taps)
{
    return cfg->depth <= 0 || cfg->embed_dim <= 0 || cfg->patch_size <= 0 || cfg->img_size < cfg->patch_size ? "bad model config"
           : n_taps < 1 || n_taps > 4 ? "n_taps must be in 1..4"
           : NULL;
}

/* ... and the taps themselves (1 <= n_taps <= 4), resolved to ascending layer indices */
static const char *resolve_taps(const vit_config *cfg, int n_taps, const int taps[4], int layer[4])
{
    for (int k = 0; k < n_taps; ++k) {
        const int t = taps[k];
        if (t < -cfg->depth || t >= cfg->depth)
            return "a tap lies outside [-depth, depth)";
        if (k > 0 && (t < 0 ? t + cfg->depth : t) <= layer[k - 1])
            return "taps must be strictly ascending once resolved";
        layer[k] = t < 0 ? t + cfg->depth : t;
    }
    return NULL;
}

/* spec against cfg; the taps resolved to ascending layer indices */
static int feature_spec_check(const char *who, const vit_config *cfg, const vit_feature_spec *spec, int layer[4])
{
    const char *why = !cfg || !spec ? "NULL argument" : taps_count_check(cfg, spec->n_taps);
    why = why ? why
          : spec->dtype != VIT_FEATURE_F32 && spec->dtype != VIT_FEATURE_BF16 ? "dtype must be VIT_FEATURE_F32 or VIT_FEATURE_BF16"
          : spec->token_layout != VIT_TOKENS_NLC && spec->token_layout != VIT_TOKENS_NCHW ? "token_layout must be VIT_TOKENS_NLC or VIT_TOKENS_NCHW"
          : resolve_taps(cfg, spec->n_taps, spec->taps, layer);
    return why ? ingest_refuse(who, why) : 0;
}

int vit_feature_sizes(const vit_config *cfg, const vit_feature_spec *spec, size_t *cls_elems, size_t *pooled_elems, size_t *tokens_elems)
{
    int layer[4];
    if (feature_spec_check("vit_feature_sizes", cfg, spec, layer))
        return 1;
    const size_t per = (size_t)spec->n_taps * (size_t)cfg->embed_dim, patches = (size_t)vit_config_tokens(cfg) - 1;
    if (cls_elems)
        *cls_elems = per;
    if (pooled_elems)
        *pooled_elems = patches ? per : 0;
    if (tokens_elems)
        *tokens_elems = per * patches;
    return 0;
}

int requests_set_features(const char *who, const struct request_model *m, struct requests *rq, const vit_feature_spec *spec,
                          const vit_feature_buffers *bufs, int host)
{
    struct feature_req fr;
    memset(&fr, 0, sizeof fr);
    if (spec) {
        if (feature_spec_check(who, m->cfg, spec, fr.layer))
            return 1;
        const char *why = !bufs || (!bufs->cls && !bufs->pooled && !bufs->tokens) ? "no output buffer"
                          : host && bufs->tokens ? "the host form takes cls and pooled only (tokens: use the device form)"
                          : m->tokens < 2 && (bufs->pooled || bufs->tokens) ? "pooled and tokens need at least one patch token"
                          : !host && (((uintptr_t)bufs->cls | (uintptr_t)bufs->pooled | (uintptr_t)bufs->tokens) & 15) ? "device buffers must be 16-byte aligned"
                          : NULL;
        if (why)
            return ingest_refuse(who, why);
        fr.head.form = host ? FEAT_HOST : FEAT_DEVICE;
        fr.spec = *spec;
        fr.out = *bufs;
        if (host) {
            const size_t per = (size_t)spec->n_taps * m->cfg->embed_dim * (spec->dtype == VIT_FEATURE_BF16 ? 2 : 4);
            fr.head.st[0] = (struct staged){.host = (char *)bufs->cls, .per_image = per};
            fr.head.st[1] = (struct staged){.host = (char *)bufs->pooled, .per_image = per};
        }
    }
    const int rc = request_arm(who, m, &rq->feat.head, &fr.head, sizeof fr, no_scratch, 0, NULL);
    if (rc == 0 && host && spec)
        rq->feat.out = (vit_feature_buffers){rq->feat.head.st[0].dev, rq->feat.head.st[1].dev, NULL};
    return rc;
}

static int topk_spec_check(const char *who, const vit_config *cfg, const vit_topk_spec *spec)
{
    const char *why = !cfg || !spec ? "NULL argument"
                      : cfg->num_classes < 1 || cfg->num_classes > 65536 ? "num_classes must be in 1..65536"
                      : spec->k < 1 || spec->k > 32 ? "k must be in 1..32"
                      : spec->k > cfg->num_classes ? "k exceeds num_classes"
                      : spec->score_kind != VIT_TOPK_PROBS && spec->score_kind != VIT_TOPK_LOGITS ? "score_kind must be VIT_TOPK_PROBS or VIT_TOPK_LOGITS"
                      : NULL;
    return why ? ingest_refuse(who, why) : 0;
}

int vit_topk_check(const vit_config *cfg, const vit_topk_spec *spec)
{
    return topk_spec_check("vit_topk_check", cfg, spec);
}

int requests_set_topk(const char *who, const struct request_model *m, struct requests *rq, const vit_topk_spec *spec,
                      const vit_topk_buffers *bufs, int host)
{
    struct topk_req tk;
    memset(&tk, 0, sizeof tk);
    if (spec) {
        if (topk_spec_check(who, m->cfg, spec))
            return 1;
        const char *why = !bufs || !bufs->labels ? "no labels buffer"
                          : !host && (((uintptr_t)bufs->labels | (uintptr_t)bufs->scores) & 15) ? "device buffers must be 16-byte aligned"
                          : NULL;
        if (why)
            return ingest_refuse(who, why);
        tk.head.form = host ? FEAT_HOST : FEAT_DEVICE;
        tk.spec = *spec;
        tk.out = *bufs;
        if (host) {
            tk.head.st[0] = (struct staged){.host = (char *)bufs->labels, .per_image = (size_t)spec->k * sizeof(int)};
            tk.head.st[1] = (struct staged){.host = (char *)bufs->scores, .per_image = (size_t)spec->k * sizeof(float)};
        }
    }
    const int rc = request_arm(who, m, &rq->topk.head, &tk.head, sizeof tk, no_scratch, 0, NULL);
    if (rc == 0 && host && spec)
        rq->topk.out = (vit_topk_buffers){rq->topk.head.st[0].dev, rq->topk.head.st[1].dev};
    return rc;
}

static int attn_spec_check(const char *who, const vit_config *cfg, const vit_attn_spec *spec, int layer[4])
{
    const char *why = !cfg || !spec ? "NULL argument" : taps_count_check(cfg, spec->n_taps);
    why = why ? why
          : cfg->num_heads <= 0 || cfg->embed_dim % cfg->num_heads != 0 ? "bad model config"
          : resolve_taps(cfg, spec->n_taps, spec->taps, layer);
    return why ? ingest_refuse(who, why) : 0;
}

int vit_attn_sizes(const vit_config *cfg, const vit_attn_spec *spec, size_t *heads_elems, size_t *mean_elems)
{
    int layer[4];
    if (attn_spec_check("vit_attn_sizes", cfg, spec, layer))
        return 1;
    const size_t per = (size_t)spec->n_taps * (size_t)vit_config_tokens(cfg);
    if (heads_elems)
        *heads_elems = per * (size_t)cfg->num_heads;
    if (mean_elems)
        *mean_elems = per;
    return 0;
}

int requests_set_attention(const char *who, const struct request_model *m, struct requests *rq, const vit_attn_spec *spec,
                           const vit_attn_buffers *bufs, int host)
{
    struct attn_req ar;
    memset(&ar, 0, sizeof ar);
    if (spec) {
        if (attn_spec_check(who, m->cfg, spec, ar.layer))
            return 1;
        const vit_config *c = m->cfg;
        const char *why = !bufs || (!bufs->heads && !bufs->mean) ? "no output buffer"
                          : !kl_cls_attention_head_dim_ok(c->embed_dim / c->num_heads) ? "head_dim must be a multiple of 16, at most 128"
                          : !host && (((uintptr_t)bufs->heads | (uintptr_t)bufs->mean) & 15) ? "device buffers must be 16-byte aligned"
                          : NULL;
        if (why)
            return ingest_refuse(who, why);
        ar.head.form = host ? FEAT_HOST : FEAT_DEVICE;
        ar.spec = *spec;
        ar.out = *bufs;
        if (host) {
            const size_t per = (size_t)spec->n_taps * m->tokens * sizeof(float);
            ar.head.st[0] = (struct staged){.host = (char *)bufs->heads, .per_image = per * c->num_heads};
            ar.head.st[1] = (struct staged){.host = (char *)bufs->mean, .per_image = per};
        }
    }
    const int rc = request_arm(who, m, &rq->amap.head, &ar.head, sizeof ar, no_scratch, 0, NULL);
    if (rc == 0 && host && spec)
        rq->amap.out = (vit_attn_buffers){rq->amap.head.st[0].dev, rq->amap.head.st[1].dev};
    return rc;
}

/* spec against cfg; first_layer resolved to a layer index */
static int rollout_spec_check(const char *who, const vit_config *cfg, const vit_rollout_spec *spec, int *first)
{
    const char *why = !cfg || !spec ? "NULL argument"
                      : cfg->depth <= 0 || cfg->embed_dim <= 0 || cfg->patch_size <= 0 || cfg->img_size < cfg->patch_size ||
                        cfg->num_heads <= 0 || cfg->embed_dim % cfg->num_heads != 0 ? "bad model config"
                      : spec->first_layer < -cfg->depth || spec->first_layer >= cfg->depth ? "first_layer lies outside [-depth, depth)"
                      : NULL;
    if (why)
        return ingest_refuse(who, why);
    *first = spec->first_layer < 0 ? spec->first_layer + cfg->depth : spec->first_layer;
    return 0;
}

int vit_rollout_sizes(const vit_config *cfg, const vit_rollout_spec *spec, size_t *rollout_elems, size_t *scratch_bytes_per_image)
{
    int first;
    if (rollout_spec_check("vit_rollout_sizes", cfg, spec, &first))
        return 1;
    const size_t T = (size_t)vit_config_tokens(cfg);
    if (rollout_elems)
        *rollout_elems = T;
    if (scratch_bytes_per_image)
        *scratch_bytes_per_image = 3 * T * T * sizeof(float);
    return 0;
}

/* The scratch (two running products and a step's workspace, of max_batch images each) is made with the first request and
 * kept until the context is disarmed or destroyed */
int requests_set_rollout(const char *who, const struct request_model *m, struct requests *rq, const vit_rollout_spec *spec,
                         const vit_rollout_buffers *bufs, int host)
{
    struct rollout_req ro;
    size_t scratch[3] = {0, 0, 0};
    char oom[160] = "";
    memset(&ro, 0, sizeof ro);
    if (spec) {
        if (rollout_spec_check(who, m->cfg, spec, &ro.first))
            return 1;
        const vit_config *c = m->cfg;
        const int D = c->embed_dim / c->num_heads;
        const char *why = !bufs || !bufs->rollout ? "no output buffer"
                          : !kl_cls_attention_head_dim_ok(D) ? "head_dim must be a multiple of 16, at most 128"
                          : m->qkv_form != VH_QKV_ROWS_F32 && c->embed_dim % 32 != 0 ? "embed_dim must be a multiple of 32 where Q|K|V is stored as planes"
                          : m->tokens > kl_rollout_max_tokens(D) ? "too many tokens for the rollout kernel at this head_dim (vh_rollout_max_tokens)"
                          : !host && ((uintptr_t)bufs->rollout & 15) ? "device buffers must be 16-byte aligned"
                          : NULL;
        if (why)
            return ingest_refuse(who, why);
        ro.head.form = host ? FEAT_HOST : FEAT_DEVICE;
        ro.spec = *spec;
        ro.out = *bufs;
        if (host)
            ro.head.st[0] = (struct staged){.host = (char *)bufs->rollout, .per_image = (size_t)m->tokens * sizeof(float)};
        scratch[0] = scratch[1] = scratch[2] = kl_rollout_workspace(m->max_batch, m->tokens);
        snprintf(oom, sizeof oom, "3 x %zu bytes of device scratch (max_batch x T x T x 4 each) cannot be allocated", scratch[0]);
    }
    const int rc = request_arm(who, m, &rq->roll.head, &ro.head, sizeof ro, scratch, 1, oom);
    if (rc == 0 && host && spec)
        rq->roll.out = (vit_rollout_buffers){rq->roll.head.st[0].dev};
    return rc;
}

/* spec against cfg, pointers aside; tap resolved to a layer index, the scratch per image of max_batch */
static int gallery_spec_check(const char *who, const vit_config *cfg, const vit_gallery_spec *spec, int *layer, size_t *per_image)
{
    const char *why = !cfg || !spec ? "NULL argument"
                      : cfg->depth <= 0 || cfg->embed_dim <= 0 || cfg->patch_size <= 0 || cfg->img_size < cfg->patch_size ? "bad model config"
                      : spec->source != VIT_GALLERY_CLS && spec->source != VIT_GALLERY_POOLED ? "source must be VIT_GALLERY_CLS or VIT_GALLERY_POOLED"
                      : spec->tap < -cfg->depth || spec->tap >= cfg->depth ? "tap lies outside [-depth, depth)"
                      : spec->source == VIT_GALLERY_POOLED && vit_config_tokens(cfg) < 2 ? "pooled needs at least one patch token"
                      : spec->dtype != VH_GALLERY_F32 && spec->dtype != VH_GALLERY_BF16 ? "dtype must be VH_GALLERY_F32 or VH_GALLERY_BF16"
                      : cfg->embed_dim % 4 != 0 || cfg->embed_dim > KL_GALLERY_MAX_EMBED ? "embed_dim must be a multiple of 4, at most 2048"
                      : spec->k < 1 || spec->k > 32 ? "k must be in 1..32"
                      : spec->n_rows < spec->k || spec->n_rows > 2147483647L ? "n_rows must be in k..2^31 - 1"
                      : spec->row_stride < cfg->embed_dim || spec->row_stride > (1L << 40) ||
                        (spec->row_stride * (spec->dtype == VH_GALLERY_BF16 ? 2 : 4)) % 16 != 0
                          ? "row_stride must be at least embed_dim, and a multiple of 16 bytes"
                      : NULL;
    if (why)
        return ingest_refuse(who, why);
    *layer = spec->tap < 0 ? spec->tap + cfg->depth : spec->tap;
    *per_image = (size_t)cfg->embed_dim * sizeof(float) + kl_gallery_workspace(1, spec->n_rows, spec->k, 0);
    return 0;
}

int vit_gallery_check(const vit_config *cfg, const vit_gallery_spec *spec, size_t *scratch_bytes_per_max_batch_image)
{
    int layer;
    size_t per_image;
    if (gallery_spec_check("vit_gallery_check", cfg, spec, &layer, &per_image))
        return 1;
    if (scratch_bytes_per_max_batch_image)
        *scratch_bytes_per_max_batch_image = per_image;
    return 0;
}

int requests_set_gallery(const char *who, const struct request_model *m, struct requests *rq, const vit_gallery_spec *spec,
                         const vit_gallery_buffers *bufs, int host)
{
    struct gallery_req ga;
    size_t scratch[3] = {0, 0, 0};
    char oom[160] = "";
    memset(&ga, 0, sizeof ga);
    if (spec) {
        size_t per_image;
        if (gallery_spec_check(who, m->cfg, spec, &ga.layer, &per_image))
            return 1;
        const char *why = !spec->d_rows ? "no gallery rows"
                          : (uintptr_t)spec->d_rows & 15 ? "the gallery rows must be 16-byte aligned"
                          : !bufs || !bufs->indices ? "no indices buffer"
                          : !host && (((uintptr_t)bufs->indices | (uintptr_t)bufs->scores) & 15) ? "device buffers must be 16-byte aligned"
                          : NULL;
        if (why)
            return ingest_refuse(who, why);
        ga.head.form = host ? FEAT_HOST : FEAT_DEVICE;
        ga.spec = *spec;
        ga.out = *bufs;
        if (host) {
            ga.head.st[0] = (struct staged){.host = (char *)bufs->indices, .per_image = (size_t)spec->k * sizeof(int)};
            ga.head.st[1] = (struct staged){.host = (char *)bufs->scores, .per_image = (size_t)spec->k * sizeof(float)};
        }
        scratch[0] = (size_t)m->max_batch * m->cfg->embed_dim * sizeof(float);
        scratch[1] = (size_t)m->max_batch * (per_image - (size_t)m->cfg->embed_dim * sizeof(float));
        snprintf(oom, sizeof oom, "%zu bytes of device scratch (the queries and the search's workspace) cannot be allocated",
                 scratch[0] + scratch[1]);
    }
    const int rc = request_arm(who, m, &rq->gal.head, &ga.head, sizeof ga, scratch, 0, oom);
    if (rc == 0 && host && spec)
        rq->gal.out = (vit_gallery_buffers){(int *)rq->gal.head.st[0].dev, (float *)rq->gal.head.st[1].dev};
    return rc;
}

/* spec against cfg, pointers aside; tap resolved to a layer index, the grid, the output size */
static int dense_spec_check(const char *who, const vit_config *cfg, const vit_dense_spec *spec, int *layer, int *grid_h, int *grid_w,
                            int *out_h, int *out_w)
{
    int gh = 0, gw = 0;
    if (cfg && cfg->patch_size > 0)
        vit_config_grid(cfg, &gh, &gw);
    const int width = cfg ? gw * cfg->patch_size : 0;
    const char *why = !cfg || !spec ? "NULL argument"
                      : cfg->depth <= 0 || cfg->embed_dim <= 0 || cfg->patch_size <= 0 || cfg->img_size < cfg->patch_size ? "bad model config"
                      : spec->tap < -cfg->depth || spec->tap >= cfg->depth ? "tap lies outside [-depth, depth)"
                      : vit_config_tokens(cfg) < 2 ? "the model needs a grid of at least one patch token"
                      : gh > VH_DENSE_MAX_GRID || gw > VH_DENSE_MAX_GRID ? "the patch grid must be at most 64 x 64"
                      : cfg->embed_dim % 4 != 0 || cfg->embed_dim > KL_DENSE_MAX_EMBED ? "embed_dim must be a multiple of 4, at most 2048"
                      : spec->n_labels < 2 || spec->n_labels > VH_DENSE_MAX_LABELS ? "n_labels must be in 2..256"
                      : spec->out_h < 0 || spec->out_h > 4096 || spec->out_w < 0 || spec->out_w > 4096 ||
                        (spec->out_h == 0 && cfg->img_size > 4096) || (spec->out_w == 0 && width > 4096)
                          ? "out_h and out_w must be in 1..4096 (0: the model's img_size and width)"
                      : spec->weight_stride < cfg->embed_dim || spec->weight_stride > (1L << 40) || spec->weight_stride % 4 != 0
                          ? "weight_stride must be at least embed_dim, and a multiple of 4"
                      : NULL;
    if (why)
        return ingest_refuse(who, why);
    *layer = spec->tap < 0 ? spec->tap + cfg->depth : spec->tap;
    *grid_h = gh;
    *grid_w = gw;
    *out_h = spec->out_h ? spec->out_h : cfg->img_size;
    *out_w = spec->out_w ? spec->out_w : width;
    return 0;
}

int vit_dense_sizes(const vit_config *cfg, const vit_dense_spec *spec, size_t *labels_bytes, size_t *scores_elems,
                    size_t *patch_logits_elems, size_t *scratch_bytes_per_image)
{
    int layer, grid_h, grid_w, out_h, out_w;
    if (dense_spec_check("vit_dense_sizes", cfg, spec, &layer, &grid_h, &grid_w, &out_h, &out_w))
        return 1;
    const size_t P = (size_t)grid_h * grid_w;
    if (labels_bytes)
        *labels_bytes = (size_t)out_h * out_w;
    if (scores_elems)
        *scores_elems = (size_t)out_h * out_w;
    if (patch_logits_elems)
        *patch_logits_elems = P * spec->n_labels;
    if (scratch_bytes_per_image)
        *scratch_bytes_per_image = P * ((size_t)spec->n_labels + (spec->final_norm ? (size_t)cfg->embed_dim : 0)) * sizeof(float);
    return 0;
}

/* soft against nothing but itself: NULL, or why not */
static const char *dense_soft_spec_why(const vit_dense_soft_spec *soft)
{
    return !soft ? "NULL argument (soft)"
           : !(soft->logit_scale > 0.0f) || !(soft->logit_scale <= 3.402823466e+38f) ? "logit_scale must be finite and > 0"
           : (uintptr_t)soft->d_values & 15 ? "d_values must be 16-byte aligned"
           : NULL;
}

/* soft and the maps asked for, as both vit_hip_set_dense_soft and the soft frame calls take them (on_device: the maps are
 * device buffers, 16-byte aligned): NULL, or why not */
const char *requests_dense_soft_why(const vit_dense_soft_spec *soft, const vit_dense_soft_buffers *sbufs, int on_device)
{
    const char *why = dense_soft_spec_why(soft);
    return why ? why
           : !sbufs ? "NULL argument (d_soft)"
           : !sbufs->prob && !sbufs->expect && !sbufs->entropy ? "no soft map asked for (prob, expect, entropy are all NULL)"
           : (sbufs->expect != NULL) != (soft->d_values != NULL) ? "d_values must be given exactly when expect is asked for"
           : on_device && (((uintptr_t)sbufs->prob | (uintptr_t)sbufs->expect | (uintptr_t)sbufs->entropy) & 15) ? "device buffers must be 16-byte aligned"
           : NULL;
}

int vit_dense_soft_check(const vit_config *cfg, const vit_dense_spec *spec, const vit_dense_soft_spec *soft, size_t *map_elems_per_image)
{
    static const char who[] = "vit_dense_soft_check";
    int layer, grid_h, grid_w, out_h, out_w;
    if (dense_spec_check(who, cfg, spec, &layer, &grid_h, &grid_w, &out_h, &out_w))
        return 1;
    const char *why = dense_soft_spec_why(soft);
    if (why)
        return ingest_refuse(who, why);
    if (map_elems_per_image)
        *map_elems_per_image = (size_t)out_h * out_w;
    return 0;
}

/* Both setters of the dense request.  soft NULL: vit_hip_set_dense / _host.  Otherwise vit_hip_set_dense_soft: the device
 * form with the soft maps attached; bufs may be NULL and labels need not be asked for. */
static int dense_arm(const char *who, const struct request_model *m, struct requests *rq, const vit_dense_spec *spec,
                     const vit_dense_buffers *bufs, int host, int with_soft, const vit_dense_soft_spec *soft,
                     const vit_dense_soft_buffers *sbufs)
{
    static const vit_dense_buffers no_bufs;
    struct dense_req de;
    size_t scratch[3] = {0, 0, 0};
    char oom[160] = "";
    memset(&de, 0, sizeof de);
    if (spec) {
        if (dense_spec_check(who, m->cfg, spec, &de.layer, &de.grid_h, &de.grid_w, &de.out_h, &de.out_w))
            return 1;
        if (with_soft && !bufs)
            bufs = &no_bufs;
        const char *why = !spec->d_weight ? "no head weight"
                          : ((uintptr_t)spec->d_weight | (uintptr_t)spec->d_bias) & 15 ? "the head's weight and bias must be 16-byte aligned"
                          : with_soft ? requests_dense_soft_why(soft, sbufs, 1)
                          : NULL;
        why = why ? why
              : with_soft && bufs->scores && !bufs->labels ? "scores need a labels buffer"
              : !with_soft && (!bufs || !bufs->labels) ? "no labels buffer"
              : host && (bufs->scores || bufs->patch_logits) ? "the host form takes labels only (scores, patch_logits: use the device form)"
              : !host && (((uintptr_t)bufs->labels | (uintptr_t)bufs->scores | (uintptr_t)bufs->patch_logits) & 15)
                  ? "device buffers must be 16-byte aligned"
              : NULL;
        if (why)
            return ingest_refuse(who, why);
        de.head.form = host ? FEAT_HOST : FEAT_DEVICE;
        de.spec = *spec;
        de.out = *bufs;
        if (with_soft) {
            de.soft = *soft;
            de.soft_out = *sbufs;
        }
        if (host)
            de.head.st[0] = (struct staged){.host = (char *)bufs->labels, .per_image = (size_t)de.out_h * de.out_w};
        const size_t P = (size_t)m->tokens - 1;
        scratch[0] = bufs->patch_logits ? 0 : (size_t)m->max_batch * P * spec->n_labels * sizeof(float);
        scratch[1] = spec->final_norm ? (size_t)m->max_batch * P * m->cfg->embed_dim * sizeof(float) : 0;
        if (scratch[1] <= m->ws_bytes)
            scratch[1] = 0;   /* they go through the MLP buffer */
        snprintf(oom, sizeof oom, "%zu bytes of device scratch (the patch logits and the normalised tokens) cannot be allocated",
                 scratch[0] + scratch[1]);
    }
    const int rc = request_arm(who, m, &rq->dense.head, &de.head, sizeof de, scratch, 0, oom);
    if (rc == 0 && host && spec)
        rq->dense.out = (vit_dense_buffers){(unsigned char *)rq->dense.head.st[0].dev, NULL, NULL};
    return rc;
}

int requests_set_dense(const char *who, const struct request_model *m, struct requests *rq, const vit_dense_spec *spec,
                       const vit_dense_buffers *bufs, int host)
{
    return dense_arm(who, m, rq, spec, bufs, host, 0, NULL, NULL);
}

int requests_set_dense_soft(const char *who, const struct request_model *m, struct requests *rq, const vit_dense_spec *spec,
                            const vit_dense_soft_spec *soft, const vit_dense_buffers *bufs, const vit_dense_soft_buffers *sbufs)
{
    return dense_arm(who, m, rq, spec, bufs, 0, 1, soft, sbufs);
}

int requests_serving(const struct requests *rq, const char *who, int form, struct serving *sv)
{
    memset(sv, 0, sizeof *sv);
    if (form == FEAT_NONE)
        return 0;
    for (int r = 0; r < N_REQUESTS; ++r) {
        const int armed = request_at(rq, r)->form;
        if (armed != FEAT_NONE && armed != form) {
            char msg[200];
            const char *const is = armed == FEAT_HOST ? "host" : "device";
            snprintf(msg, sizeof msg, "%s: the context is armed for %s %s buffers (vit_hip_set_%s%s); disarm it or use the %s forms", who, is,
                     kinds[r].what, kinds[r].setter, armed == FEAT_HOST ? "_host" : "", is);
            return vh_set_error(1, msg);
        }
    }
    sv->fr = rq->feat.head.form == form ? &rq->feat : NULL;
    sv->tk = rq->topk.head.form == form ? &rq->topk : NULL;
    sv->ar = rq->amap.head.form == form ? &rq->amap : NULL;
    sv->ro = rq->roll.head.form == form ? &rq->roll : NULL;
    sv->ga = rq->gal.head.form == form ? &rq->gal : NULL;
    sv->de = rq->dense.head.form == form ? &rq->dense : NULL;
    return 0;
}

int serving_staged(const struct serving *sv, const struct staged *arrays[MAX_STAGED])
{
    const struct request *const head[N_REQUESTS] = {sv->fr ? &sv->fr->head : NULL, sv->tk ? &sv->tk->head : NULL, sv->ar ? &sv->ar->head : NULL,
                                                    sv->ro ? &sv->ro->head : NULL, sv->ga ? &sv->ga->head : NULL, sv->de ? &sv->de->head : NULL};
    int n = 0;
    for (int r = 0; r < N_REQUESTS; ++r)
        for (int k = 0; head[r] && k < 2; ++k)
            if (head[r]->st[k].dev)
                arrays[n++] = &head[r]->st[k];
    return n;
}

int serving_needs_last_layer_rows(const struct serving *sv, int depth)
{
    const struct feature_req *fr = sv->fr;
    return (fr && fr->layer[fr->spec.n_taps - 1] == depth - 1 && (fr->out.pooled || fr->out.tokens)) ||
           (sv->ga && sv->ga->layer == depth - 1 && sv->ga->spec.source == VIT_GALLERY_POOLED) || (sv->de && sv->de->layer == depth - 1);
}
