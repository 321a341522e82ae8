/*
 * requests_main.c -- csrc/vit_requests.c on its own, without a device, over an allocator that counts its live blocks and
 * fails on demand: arming each of the six armed outputs in both forms with every allocation failing in turn, the scratch
 * rules, what a forward serves and how a request in the other form refuses it, the list of staged arrays, the last-layer
 * predicate and the release of everything.  Built and run by tests/test_requests_host.py under ASan + UBSan; exit status
 * 0 = every check held.
 *   requests_main          the checks
 *   requests_main limits   print what the sizing functions of csrc/kernel_limits.h, which the unit calls, return (the
 *                          library's exported entries are held against them)
 */
#include "vit_requests.h"
#include "kernel_limits.h"

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
int vh_stream_sync(vh_stream_t s) { return s ? 0 : 1; }

/* ---- the allocator: malloc, every live block on a list with its kind; allocation number fail_in from now fails -------- */
enum { DEVICE_BLOCK, PINNED_BLOCK, MAX_LIVE = 256 };
static struct { void *p; int kind; } live_blocks[MAX_LIVE];
static int n_live[2], n_allocs, fail_in;

static int block_alloc(void **out, size_t bytes, int kind)
{
    if (fail_in > 0 && --fail_in == 0)
        return vh_set_error(2, "out of memory");
    CHECK(bytes > 0, "an allocation of no bytes");
    for (int i = 0; i < MAX_LIVE; ++i)
        if (!live_blocks[i].p) {
            live_blocks[i].p = *out = malloc(bytes);
            live_blocks[i].kind = kind;
            ++n_live[kind];
            ++n_allocs;
            return 0;
        }
    CHECK(0, "more than %d live blocks", MAX_LIVE);
    return 1;
}

static int is_live(const void *p, int kind)
{
    for (int i = 0; i < MAX_LIVE; ++i)
        if (p && live_blocks[i].p == p && live_blocks[i].kind == kind)
            return 1;
    return 0;
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
    CHECK(0, "%p freed, which is no live %s block", p, kind == PINNED_BLOCK ? "pinned" : "device");
    return 1;
}

int vh_malloc(void **out, size_t bytes) { return block_alloc(out, bytes, DEVICE_BLOCK); }
int vh_free(void *p) { return block_free(p, DEVICE_BLOCK); }
int vh_host_alloc(void **out, size_t bytes) { return block_alloc(out, bytes, PINNED_BLOCK); }
int vh_host_free(void *p) { return block_free(p, PINNED_BLOCK); }

/* ---- the context the requests are armed on: all six take it ----------------------------------------------------------- */
static const vit_config cfg = {32, 8, 3, 10, 64, 2, 4, 128, 1e-6};
enum { MAX_BATCH = 4, TOKENS = 17, WS_BYTES = MAX_BATCH * TOKENS * 128 * 4 };
static struct request_model model = {.device = 0, .max_batch = MAX_BATCH, .stream = &model, .cfg = &cfg, .tokens = TOKENS,
                                     .qkv_form = VH_QKV_ROWS_F32, .ws_bytes = WS_BYTES};
static struct requests rq;
static const char *const names[N_REQUESTS] = {"features", "topk", "attention", "rollout", "gallery", "dense"};
static const int n_arrays[N_REQUESTS] = {2, 2, 2, 1, 2, 1}, n_scratch[N_REQUESTS] = {0, 0, 0, 3, 2, 1};

/* never read or written: 16-byte aligned stand-ins for the caller's buffers, [request][buffer], and for its rows / weights */
static _Alignas(16) char bufs[N_REQUESTS][3][16], rows[16];

static struct request *head_of(int r)
{
    struct request *const all[N_REQUESTS] = {&rq.feat.head, &rq.topk.head, &rq.amap.head, &rq.roll.head, &rq.gal.head, &rq.dense.head};
    return all[r];
}

/* Arm request r in the device (host 0) or the host form.  variant 0 or 1: two specs of other sizes.  second: the second
 * buffer (pooled / scores / mean; none for rollout and dense) is asked for too; with 0, attention drops heads instead. */
static int arm_with(int r, int host, int variant, int second)
{
    void *const b0 = bufs[r][0], *const b1 = second ? bufs[r][1] : NULL;
    const char *const who = host ? "setter_host" : "setter";
    switch (r) {
    case 0: {
        const vit_feature_spec spec = {.n_taps = 1 + variant, .taps = {variant ? 0 : -1, 1}, .final_norm = 1};
        const vit_feature_buffers fb = {b0, b1, NULL};
        return requests_set_features(who, &model, &rq, &spec, &fb, host);
    }
    case 1: {
        const vit_topk_spec spec = {.k = 3 + 2 * variant, .score_kind = VIT_TOPK_PROBS};
        const vit_topk_buffers tb = {b0, b1};
        return requests_set_topk(who, &model, &rq, &spec, &tb, host);
    }
    case 2: {
        const vit_attn_spec spec = {.n_taps = 1 + variant, .taps = {variant ? 0 : -1, 1}};
        const vit_attn_buffers ab = {second ? b0 : NULL, (float *)bufs[r][1]};
        return requests_set_attention(who, &model, &rq, &spec, &ab, host);
    }
    case 3: {
        const vit_rollout_spec spec = {.first_layer = variant};
        const vit_rollout_buffers rb = {b0};
        return requests_set_rollout(who, &model, &rq, &spec, &rb, host);
    }
    case 4: {
        const vit_gallery_spec spec = {.source = VIT_GALLERY_POOLED, .tap = -1, .k = 2 + 2 * variant, .dtype = VH_GALLERY_F32,
                                       .n_rows = 1000, .row_stride = 64, .d_rows = rows};
        const vit_gallery_buffers gb = {b0, b1};
        return requests_set_gallery(who, &model, &rq, &spec, &gb, host);
    }
    default: {
        const vit_dense_spec spec = {.tap = -1, .final_norm = 1, .n_labels = 3 + 2 * variant, .weight_stride = 64, .d_weight = (const float *)rows};
        const vit_dense_buffers db = {b0, NULL, NULL};
        return requests_set_dense(who, &model, &rq, &spec, &db, host);
    }
    }
}

static int arm(int r, int host, int variant) { return arm_with(r, host, variant, 1); }

static int disarm(int r)
{
    switch (r) {
    case 0: return requests_set_features("setter", &model, &rq, NULL, NULL, 0);
    case 1: return requests_set_topk("setter", &model, &rq, NULL, NULL, 0);
    case 2: return requests_set_attention("setter", &model, &rq, NULL, NULL, 0);
    case 3: return requests_set_rollout("setter", &model, &rq, NULL, NULL, 0);
    case 4: return requests_set_gallery("setter", &model, &rq, NULL, NULL, 0);
    default: return requests_set_dense("setter", &model, &rq, NULL, NULL, 0);
    }
}

/* Every pointer request r holds is a live block of its kind, and the live blocks are exactly those of a request r armed in
 * `form` (FEAT_NONE: none) with every array asked for, nothing else being armed */
static void check_holds(int r, int form)
{
    const struct request *h = head_of(r);
    const int arrays = form == FEAT_HOST ? n_arrays[r] : 0, scratch = form == FEAT_NONE ? 0 : n_scratch[r];
    int dev = 0, pinned = 0;
    CHECK(h->form == form, "form %d, expected %d", h->form, form);
    for (int k = 0; k < 2; ++k) {
        if (h->st[k].dev)
            CHECK(is_live(h->st[k].dev, DEVICE_BLOCK) && is_live(h->st[k].pinned[0], PINNED_BLOCK) && is_live(h->st[k].pinned[1], PINNED_BLOCK),
                  "staged array %d holds a block that is not live", k);
        else
            CHECK(!h->st[k].pinned[0] && !h->st[k].pinned[1], "staged array %d has pinned slots and no device buffer", k);
        dev += h->st[k].dev != NULL;
        pinned += 2 * (h->st[k].dev != NULL);
    }
    for (int k = 0; k < 3; ++k) {
        CHECK(!h->scratch[k] || is_live(h->scratch[k], DEVICE_BLOCK), "scratch %d is not live", k);
        dev += h->scratch[k] != NULL;
    }
    CHECK(dev == arrays + scratch && pinned == 2 * arrays, "the request holds %d device and %d pinned blocks, expected %d and %d", dev, pinned,
          arrays + scratch, 2 * arrays);
    CHECK(n_live[DEVICE_BLOCK] == dev && n_live[PINNED_BLOCK] == pinned, "%d device and %d pinned blocks live, the request holds %d and %d",
          n_live[DEVICE_BLOCK], n_live[PINNED_BLOCK], dev, pinned);
}

/* The start of a case: nothing armed, then request r as `start` says -- 0 unarmed, 1 armed in the form `host` with the
 * other spec, 2 armed in the other form */
static void start_from(int r, int host, int start)
{
    requests_release(&rq);
    memset(&rq, 0, sizeof rq);
    CHECK(n_live[DEVICE_BLOCK] == 0 && n_live[PINNED_BLOCK] == 0, "release leaves blocks");
    if (start)
        CHECK(arm(r, start == 1 ? host : !host, 1) == 0, "the start cannot be armed: %s", last_error);
}

/* Every request x form x start: the k-th allocation failing for every k of a successful arming, then the success, then
 * the disarm */
static void check_failure_at_every_allocation(void)
{
    for (int r = 0; r < N_REQUESTS; ++r)
        for (int host = 0; host < 2; ++host)
            for (int start = 0; start < 3; ++start) {
                snprintf(context, sizeof context, "%s, %s form, start %d", names[r], host ? "host" : "device", start);
                start_from(r, host, start);
                const int before = n_allocs;
                CHECK(arm(r, host, 0) == 0, "%s", last_error);
                const int N = n_allocs - before;
                /* rollout keeps its scratch from an armed request; everything else makes what it holds */
                const int kept = r == 3 && start ? 3 : 0;
                CHECK(N == (host ? 3 * n_arrays[r] : 0) + n_scratch[r] - kept, "%d allocations", N);
                check_holds(r, host ? FEAT_HOST : FEAT_DEVICE);
                for (int k = 1; k <= N; ++k) {
                    snprintf(context, sizeof context, "%s, %s form, start %d, allocation %d of %d fails", names[r], host ? "host" : "device", start, k, N);
                    start_from(r, host, start);
                    struct requests was;
                    memcpy(&was, &rq, sizeof rq);
                    const int dev = n_live[DEVICE_BLOCK], pinned = n_live[PINNED_BLOCK];
                    fail_in = k;
                    last_error[0] = 0;
                    const int rc = arm(r, host, 0);
                    CHECK(fail_in == 0, "the failure was never reached");
                    CHECK(rc != 0 && last_error[0], "rc %d, error text '%s'", rc, last_error);
                    CHECK(memcmp(&rq, &was, sizeof rq) == 0, "the armed requests changed");
                    CHECK(n_live[DEVICE_BLOCK] == dev && n_live[PINNED_BLOCK] == pinned, "%d device and %d pinned blocks live, %d and %d before",
                          n_live[DEVICE_BLOCK], n_live[PINNED_BLOCK], dev, pinned);
                    check_holds(r, start == 0 ? FEAT_NONE : (start == 1) == host ? FEAT_HOST : FEAT_DEVICE);
                    /* the out-of-memory texts of the scratch, numbers included; a staged array fails with the allocator's own */
                    const int at_scratch = k > (host ? 3 * n_arrays[r] : 0);
                    const char *const text = !at_scratch ? "out of memory"
                                             : r == 3 ? "setter: 3 x 4624 bytes of device scratch (max_batch x T x T x 4 each) cannot be allocated"
                                             : r == 4 ? "setter: 1536 bytes of device scratch (the queries and the search's workspace) cannot be allocated"
                                                      : "setter: 768 bytes of device scratch (the patch logits and the normalised tokens) cannot be allocated";
                    char want[200];
                    snprintf(want, sizeof want, "%s", text);
                    if (at_scratch && host)
                        snprintf(want, sizeof want, "setter_host%s", text + 6);
                    CHECK(strcmp(last_error, want) == 0, "error text '%s', expected '%s'", last_error, want);
                }
                snprintf(context, sizeof context, "%s, %s form, start %d: disarm", names[r], host ? "host" : "device", start);
                start_from(r, host, start);
                CHECK(arm(r, host, 0) == 0 && disarm(r) == 0, "%s", last_error);
                check_holds(r, FEAT_NONE);
            }
}

static void check_scratch_rules(void)
{
    void *old[3];
    int before;
    snprintf(context, sizeof context, "re-arming rollout keeps its scratch");
    start_from(3, 0, 0);
    CHECK(arm(3, 0, 0) == 0, "%s", last_error);
    memcpy(old, rq.roll.head.scratch, sizeof old);
    CHECK(old[0] && old[1] && old[2] && old[0] != old[1] && old[1] != old[2] && old[0] != old[2], "three buffers");
    before = n_allocs;
    CHECK(arm(3, 0, 1) == 0 && rq.roll.first == 1 && n_allocs == before, "%d allocations", n_allocs - before);
    CHECK(memcmp(old, rq.roll.head.scratch, sizeof old) == 0, "other scratch");
    CHECK(arm(3, 1, 0) == 0 && n_allocs == before + 3 && memcmp(old, rq.roll.head.scratch, sizeof old) == 0, "the host form over the device form");
    CHECK(rq.roll.out.rollout == rq.roll.head.st[0].dev && rq.roll.head.st[0].host == bufs[3][0], "the host form's buffers");
    check_holds(3, FEAT_HOST);
    for (int r = 4; r < N_REQUESTS; ++r) {
        snprintf(context, sizeof context, "re-arming %s makes fresh scratch", names[r]);
        start_from(r, 0, 0);
        CHECK(arm(r, 0, 0) == 0, "%s", last_error);
        memcpy(old, head_of(r)->scratch, sizeof old);
        CHECK(arm(r, 0, 1) == 0, "%s", last_error);
        for (int k = 0; k < n_scratch[r]; ++k)
            CHECK(old[k] && head_of(r)->scratch[k] && head_of(r)->scratch[k] != old[k] && !is_live(old[k], DEVICE_BLOCK), "scratch %d", k);
        check_holds(r, FEAT_DEVICE);
    }
    snprintf(context, sizeof context, "dense with the caller's patch_logits and tokens that fit the workspace");
    start_from(5, 0, 0);
    vit_dense_spec spec = {.tap = -1, .final_norm = 1, .n_labels = 3, .weight_stride = 64, .d_weight = (const float *)rows};
    const vit_dense_buffers own = {(unsigned char *)bufs[5][0], NULL, (float *)bufs[5][2]};
    before = n_allocs;
    CHECK(requests_set_dense("setter", &model, &rq, &spec, &own, 0) == 0 && n_allocs == before, "%d allocations", n_allocs - before);
    CHECK(rq.dense.head.form == FEAT_DEVICE && !rq.dense.head.scratch[0] && !rq.dense.head.scratch[1] && rq.dense.out.patch_logits == own.patch_logits,
          "scratch where none is needed");
    snprintf(context, sizeof context, "dense with tokens larger than the workspace");
    model.ws_bytes = (size_t)MAX_BATCH * (TOKENS - 1) * 64 * 4 - 1;
    CHECK(requests_set_dense("setter", &model, &rq, &spec, &own, 0) == 0 && n_allocs == before + 1, "%d allocations", n_allocs - before);
    CHECK(!rq.dense.head.scratch[0] && is_live(rq.dense.head.scratch[1], DEVICE_BLOCK), "scratch[1]");
    spec.final_norm = 0;
    CHECK(requests_set_dense("setter", &model, &rq, &spec, &own, 0) == 0 && n_allocs == before + 1 && n_live[DEVICE_BLOCK] == 0, "without final_norm");
    model.ws_bytes = WS_BYTES;
}

/* today's refusals of a forward that cannot serve what is armed: [request][the form armed: device, host] */
static const char *const refusals[N_REQUESTS][2] = {
    {"forward: the context is armed for device feature buffers (vit_hip_set_features); disarm it or use the device forms",
     "vit_hip_forward_device: the context is armed for host feature buffers (vit_hip_set_features_host); disarm it or use the host forms"},
    {"forward: the context is armed for device top-k buffers (vit_hip_set_topk); disarm it or use the device forms",
     "vit_hip_forward_device: the context is armed for host top-k buffers (vit_hip_set_topk_host); disarm it or use the host forms"},
    {"forward: the context is armed for device attention buffers (vit_hip_set_attention); disarm it or use the device forms",
     "vit_hip_forward_device: the context is armed for host attention buffers (vit_hip_set_attention_host); disarm it or use the host forms"},
    {"forward: the context is armed for device rollout buffers (vit_hip_set_rollout); disarm it or use the device forms",
     "vit_hip_forward_device: the context is armed for host rollout buffers (vit_hip_set_rollout_host); disarm it or use the host forms"},
    {"forward: the context is armed for device gallery buffers (vit_hip_set_gallery); disarm it or use the device forms",
     "vit_hip_forward_device: the context is armed for host gallery buffers (vit_hip_set_gallery_host); disarm it or use the host forms"},
    {"forward: the context is armed for device dense buffers (vit_hip_set_dense); disarm it or use the device forms",
     "vit_hip_forward_device: the context is armed for host dense buffers (vit_hip_set_dense_host); disarm it or use the host forms"}};

static int served(const struct serving *sv)
{
    return (sv->fr != NULL) + (sv->tk != NULL) + (sv->ar != NULL) + (sv->ro != NULL) + (sv->ga != NULL) + (sv->de != NULL);
}

static void check_serving(void)
{
    struct serving sv;
    for (int r = 0; r < N_REQUESTS; ++r)
        for (int host = 0; host < 2; ++host) {
            snprintf(context, sizeof context, "%s armed alone in the %s form", names[r], host ? "host" : "device");
            start_from(r, host, 0);
            CHECK(arm(r, host, 0) == 0, "%s", last_error);
            last_error[0] = 0;
            CHECK(requests_serving(&rq, host ? "vit_hip_forward_device" : "forward", host ? FEAT_DEVICE : FEAT_HOST, &sv) == 1, "the other form serves it");
            CHECK(strcmp(last_error, refusals[r][host]) == 0 && served(&sv) == 0, "refusal '%s'", last_error);
            CHECK(requests_serving(&rq, "forward", host ? FEAT_HOST : FEAT_DEVICE, &sv) == 0 && served(&sv) == 1, "its own form does not serve it");
            const void *const one[N_REQUESTS] = {sv.fr, sv.tk, sv.ar, sv.ro, sv.ga, sv.de};
            CHECK(one[r] == (const void *)head_of(r), "another request is served");
            CHECK(requests_serving(&rq, "forward", FEAT_NONE, &sv) == 0 && served(&sv) == 0, "FEAT_NONE serves something");
        }
    snprintf(context, sizeof context, "two armed in the wrong form");
    start_from(0, 0, 0);
    CHECK(arm(4, 1, 0) == 0 && arm(1, 1, 0) == 0 && arm(0, 0, 0) == 0, "%s", last_error);
    CHECK(requests_serving(&rq, "vit_hip_forward_device", FEAT_DEVICE, &sv) == 1 && strcmp(last_error, refusals[1][1]) == 0, "refusal '%s'", last_error);
    CHECK(requests_serving(&rq, "forward", FEAT_HOST, &sv) == 1 && strcmp(last_error, refusals[0][0]) == 0, "refusal '%s'", last_error);
    snprintf(context, sizeof context, "all six armed");
    for (int r = 0; r < N_REQUESTS; ++r)
        CHECK(arm(r, 1, 0) == 0, "%s", last_error);
    CHECK(requests_serving(&rq, "forward", FEAT_NONE, &sv) == 0 && served(&sv) == 0, "FEAT_NONE serves something");
    CHECK(requests_serving(&rq, "forward", FEAT_HOST, &sv) == 0 && served(&sv) == 6, "the host form serves %d", served(&sv));
}

static void check_staged_list(void)
{
    struct serving sv;
    const struct staged *arrays[MAX_STAGED];
    snprintf(context, sizeof context, "the staged arrays of all six");
    start_from(0, 0, 0);
    for (int r = 0; r < N_REQUESTS; ++r)
        CHECK(arm(r, 1, 0) == 0, "%s", last_error);
    CHECK(requests_serving(&rq, "forward", FEAT_HOST, &sv) == 0, "%s", last_error);
    /* cls, pooled, labels, scores, heads, mean, rollout, indices, gallery scores, dense labels */
    const struct staged *const all[10] = {&rq.feat.head.st[0], &rq.feat.head.st[1], &rq.topk.head.st[0], &rq.topk.head.st[1], &rq.amap.head.st[0],
                                          &rq.amap.head.st[1], &rq.roll.head.st[0], &rq.gal.head.st[0],  &rq.gal.head.st[1],  &rq.dense.head.st[0]};
    const char *const host_all[10] = {bufs[0][0], bufs[0][1], bufs[1][0], bufs[1][1], bufs[2][0], bufs[2][1], bufs[3][0], bufs[4][0], bufs[4][1], bufs[5][0]};
    /* per image: E fp32; E fp32; k ints; k floats; H x T and T fp32; T fp32; k ints; k floats; 32 x 32 bytes */
    const size_t per_image[10] = {256, 256, 12, 12, 4 * 17 * 4, 17 * 4, 17 * 4, 8, 8, 1024};
    CHECK(serving_staged(&sv, arrays) == 10, "not ten arrays");
    for (int a = 0; a < 10; ++a)
        CHECK(arrays[a] == all[a] && arrays[a]->host == host_all[a] && arrays[a]->per_image == per_image[a] && arrays[a]->dev, "array %d", a);
    CHECK(rq.feat.out.cls == all[0]->dev && rq.feat.out.pooled == all[1]->dev && !rq.feat.out.tokens && rq.topk.out.labels == all[2]->dev &&
          rq.topk.out.scores == all[3]->dev && rq.amap.out.heads == all[4]->dev && rq.amap.out.mean == all[5]->dev &&
          rq.roll.out.rollout == all[6]->dev && rq.gal.out.indices == all[7]->dev && rq.gal.out.scores == all[8]->dev &&
          rq.dense.out.labels == all[9]->dev && !rq.dense.out.scores && !rq.dense.out.patch_logits, "the launches do not write the staged buffers");
    snprintf(context, sizeof context, "the staged arrays with buffers left NULL");
    for (int r = 0; r < N_REQUESTS; ++r)
        CHECK(arm_with(r, 1, 0, 0) == 0, "%s", last_error);
    CHECK(requests_serving(&rq, "forward", FEAT_HOST, &sv) == 0, "%s", last_error);
    const struct staged *const some[6] = {all[0], all[2], all[5], all[6], all[7], all[9]};   /* cls, labels, mean, rollout, indices, dense labels */
    CHECK(serving_staged(&sv, arrays) == 6 && memcmp(arrays, some, sizeof some) == 0, "not those six");
    CHECK(n_live[DEVICE_BLOCK] == 6 + 3 + 2 + 1 && n_live[PINNED_BLOCK] == 12, "%d device and %d pinned blocks", n_live[DEVICE_BLOCK], n_live[PINNED_BLOCK]);
    snprintf(context, sizeof context, "a forward that serves nothing");
    CHECK(requests_serving(&rq, "forward", FEAT_NONE, &sv) == 0 && serving_staged(&sv, arrays) == 0, "arrays of nothing");
}

/* depth is 2: layer 1 is the last */
static void check_last_layer_predicate(void)
{
    struct serving sv = {0};
    struct feature_req fr = {.spec = {.n_taps = 2}, .layer = {0, 1}, .out = {bufs[0][0], bufs[0][1], NULL}};
    struct gallery_req ga = {.spec = {.source = VIT_GALLERY_POOLED}, .layer = 1};
    struct dense_req de = {.layer = 1};
    snprintf(context, sizeof context, "the last-layer predicate");
    CHECK(!serving_needs_last_layer_rows(&sv, 2), "nothing served");
    sv.fr = &fr;
    CHECK(serving_needs_last_layer_rows(&sv, 2), "pooled of the last layer");
    fr.out = (vit_feature_buffers){bufs[0][0], NULL, bufs[0][2]};
    CHECK(serving_needs_last_layer_rows(&sv, 2), "tokens of the last layer");
    fr.out = (vit_feature_buffers){bufs[0][0], NULL, NULL};
    CHECK(!serving_needs_last_layer_rows(&sv, 2), "cls alone");
    fr.out = (vit_feature_buffers){bufs[0][0], bufs[0][1], bufs[0][2]};
    fr.spec.n_taps = 1;
    CHECK(!serving_needs_last_layer_rows(&sv, 2) && serving_needs_last_layer_rows(&sv, 1), "pooled and tokens of layer 0");
    sv = (struct serving){.ga = &ga};
    CHECK(serving_needs_last_layer_rows(&sv, 2), "gallery from pooled of the last layer");
    ga.spec.source = VIT_GALLERY_CLS;
    CHECK(!serving_needs_last_layer_rows(&sv, 2), "gallery from cls");
    ga.spec.source = VIT_GALLERY_POOLED;
    ga.layer = 0;
    CHECK(!serving_needs_last_layer_rows(&sv, 2), "gallery from pooled of layer 0");
    sv = (struct serving){.de = &de};
    CHECK(serving_needs_last_layer_rows(&sv, 2), "dense on the last layer");
    de.layer = 0;
    CHECK(!serving_needs_last_layer_rows(&sv, 2), "dense on layer 0");
}

static void check_release_all(void)
{
    snprintf(context, sizeof context, "release of a fully armed table");
    start_from(0, 0, 0);
    for (int r = 0; r < N_REQUESTS; ++r)
        CHECK(arm(r, 1, 0) == 0, "%s", last_error);
    CHECK(n_live[DEVICE_BLOCK] == 10 + 3 + 2 + 1 && n_live[PINNED_BLOCK] == 20, "%d device and %d pinned blocks", n_live[DEVICE_BLOCK], n_live[PINNED_BLOCK]);
    requests_release(&rq);
    CHECK(n_live[DEVICE_BLOCK] == 0 && n_live[PINNED_BLOCK] == 0, "%d device and %d pinned blocks live", n_live[DEVICE_BLOCK], n_live[PINNED_BLOCK]);
    for (int r = 0; r < N_REQUESTS; ++r)
        for (int k = 0; k < 3; ++k)
            CHECK(!head_of(r)->scratch[k] && (k == 2 || (!head_of(r)->st[k].dev && !head_of(r)->st[k].pinned[0] && !head_of(r)->st[k].pinned[1])),
                  "%s keeps a pointer", names[r]);
}

int main(int argc, char **argv)
{
    if (argc > 1 && strcmp(argv[1], "limits") == 0) {
        const int dims[] = {0, 16, 24, 64, 80, 128, 144}, toks[] = {0, 1, 17, 197, 1370};
        const long n_rows[] = {0, 1, 128, 129, 1000, 200000, 2147483647L};
        for (size_t i = 0; i < sizeof dims / sizeof dims[0]; ++i)
            printf("head_dim %d : %d %d\n", dims[i], kl_cls_attention_head_dim_ok(dims[i]), kl_rollout_max_tokens(dims[i]));
        for (size_t i = 0; i < sizeof toks / sizeof toks[0]; ++i)
            printf("rollout %d %d : %zu\n", MAX_BATCH, toks[i], kl_rollout_workspace(MAX_BATCH, toks[i]));
        for (size_t i = 0; i < sizeof n_rows / sizeof n_rows[0]; ++i)
            for (int k = 1; k <= 32; k += k < 4 ? 1 : 28)
                printf("gallery %ld %d : %zu %zu\n", n_rows[i], k, kl_gallery_workspace(1, n_rows[i], k, 0), kl_gallery_workspace(3, n_rows[i], k, 7));
        return 0;
    }
    check_failure_at_every_allocation();
    check_scratch_rules();
    check_serving();
    check_staged_list();
    check_last_layer_predicate();
    check_release_all();
    printf("requests: ok (%d allocations)\n", n_allocs);
    return 0;
}
