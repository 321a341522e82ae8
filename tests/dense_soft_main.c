/*
 * dense_soft_main.c -- the soft arming of the dense request (requests_set_dense_soft, csrc/vit_requests.c) on its own,
 * without a device, over an allocator that counts its live blocks and fails on demand, in the manner of
 * tests/requests_main.c: arming soft with and without labels, re-arming plain over soft and soft over plain and over the
 * host form, every refusal with the previous request kept to the byte, an allocator failure at each allocation that leaves
 * nothing behind, disarming through either setter, what a forward serves, and the last-layer predicate.  Built and run by
 * tests/test_dense_soft_host.py under ASan + UBSan; exit status 0 = every check held.
 */
#include "vit_requests.h"
#include "kernel_limits.h"

#include <math.h>
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
enum { DEVICE_BLOCK, PINNED_BLOCK, MAX_LIVE = 64 };
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

static int block_free(void *p, int kind)
{
    for (int i = 0; i < MAX_LIVE; ++i)
        if (p && live_blocks[i].p == p && live_blocks[i].kind == kind) {
            free(p);
            live_blocks[i].p = NULL;
            --n_live[kind];
            return 0;
        }
    CHECK(0, "%p freed, which is no live block of its kind", p);
    return 1;
}

int vh_malloc(void **out, size_t bytes) { return block_alloc(out, bytes, DEVICE_BLOCK); }
int vh_free(void *p) { return block_free(p, DEVICE_BLOCK); }
int vh_host_alloc(void **out, size_t bytes) { return block_alloc(out, bytes, PINNED_BLOCK); }
int vh_host_free(void *p) { return block_free(p, PINNED_BLOCK); }

/* ---- the context: tests/requests_main.c's ----------------------------------------------------------------------------- */
static const vit_config cfg = {32, 8, 3, 10, 64, 2, 4, 128, 1e-6};
enum { MAX_BATCH = 4, TOKENS = 17, WS_BYTES = MAX_BATCH * TOKENS * 128 * 4 };
static struct request_model model = {.device = 0, .max_batch = MAX_BATCH, .stream = &model, .cfg = &cfg, .tokens = TOKENS,
                                     .qkv_form = VH_QKV_ROWS_F32, .ws_bytes = WS_BYTES};
static struct requests rq;
static const char who[] = "vit_hip_set_dense_soft";

/* never read or written: 16-byte aligned stand-ins for the caller's device memory */
static _Alignas(16) char lab[16], sc[16], pl[16], pr[16], ex[16], en[16], wt[32], vals[32];

static const vit_dense_spec head = {.tap = -1, .final_norm = 1, .n_labels = 5, .weight_stride = 64, .d_weight = (const float *)wt};
static const vit_dense_soft_spec plain_soft = {.logit_scale = 1.0f, .d_values = NULL};
static const vit_dense_soft_spec bins = {.logit_scale = 0.5f, .d_values = (const float *)vals};
static const vit_dense_buffers with_labels = {(unsigned char *)lab, NULL, NULL};
static const vit_dense_soft_buffers prob_only = {(float *)pr, NULL, NULL};
static const vit_dense_soft_buffers all_maps = {(float *)pr, (float *)ex, (float *)en};

static int soft_armed(void) { return rq.dense.soft_out.prob || rq.dense.soft_out.expect || rq.dense.soft_out.entropy; }

static void fresh(void)
{
    requests_release(&rq);
    memset(&rq, 0, sizeof rq);
    CHECK(n_live[DEVICE_BLOCK] == 0 && n_live[PINNED_BLOCK] == 0, "release leaves blocks");
}

static void check_arming(void)
{
    snprintf(context, sizeof context, "soft with labels and all maps");
    fresh();
    int before = n_allocs;
    CHECK(requests_set_dense_soft(who, &model, &rq, &head, &bins, &with_labels, &all_maps) == 0, "%s", last_error);
    CHECK(rq.dense.head.form == FEAT_DEVICE && soft_armed() && rq.dense.out.labels == (unsigned char *)lab, "not armed as asked");
    CHECK(rq.dense.soft.logit_scale == 0.5f && rq.dense.soft.d_values == (const float *)vals && rq.dense.soft_out.expect == (float *)ex &&
          rq.dense.soft_out.entropy == (float *)en, "the soft spec is not the caller's");
    CHECK(rq.dense.layer == 1 && rq.dense.grid_h == 4 && rq.dense.grid_w == 4 && rq.dense.out_h == 32 && rq.dense.out_w == 32, "the spec is not resolved");
    /* the patch logits are the request's own scratch: one block; the tokens fit the MLP buffer */
    CHECK(n_allocs == before + 1 && n_live[DEVICE_BLOCK] == 1 && n_live[PINNED_BLOCK] == 0 && rq.dense.head.scratch[0], "%d allocations", n_allocs - before);

    snprintf(context, sizeof context, "soft without d_bufs: no labels");
    CHECK(requests_set_dense_soft(who, &model, &rq, &head, &plain_soft, NULL, &prob_only) == 0, "%s", last_error);
    CHECK(soft_armed() && !rq.dense.out.labels && !rq.dense.out.scores && !rq.dense.out.patch_logits && !rq.dense.soft_out.expect, "buffers of the last arming");
    CHECK(n_live[DEVICE_BLOCK] == 1, "%d device blocks", n_live[DEVICE_BLOCK]);
    const vit_dense_buffers own_logits = {NULL, NULL, (float *)pl};
    CHECK(requests_set_dense_soft(who, &model, &rq, &head, &plain_soft, &own_logits, &prob_only) == 0 && n_live[DEVICE_BLOCK] == 0, "the caller's patch logits");

    snprintf(context, sizeof context, "plain over soft");
    CHECK(requests_set_dense(who, &model, &rq, &head, &with_labels, 0) == 0, "%s", last_error);
    CHECK(rq.dense.head.form == FEAT_DEVICE && !soft_armed() && rq.dense.soft.logit_scale == 0.0f && !rq.dense.soft.d_values, "soft outputs survive a plain arming");
    snprintf(context, sizeof context, "soft over plain, then the host form over soft");
    CHECK(requests_set_dense_soft(who, &model, &rq, &head, &bins, &with_labels, &all_maps) == 0 && soft_armed(), "%s", last_error);
    CHECK(requests_set_dense("vit_hip_set_dense_host", &model, &rq, &head, &with_labels, 1) == 0, "%s", last_error);
    CHECK(rq.dense.head.form == FEAT_HOST && !soft_armed() && n_live[PINNED_BLOCK] == 2, "the host form keeps soft outputs");
    CHECK(requests_set_dense_soft(who, &model, &rq, &head, &bins, &with_labels, &all_maps) == 0 && soft_armed() && n_live[PINNED_BLOCK] == 0 &&
          rq.dense.head.form == FEAT_DEVICE, "soft over the host form");

    snprintf(context, sizeof context, "disarming");
    CHECK(requests_set_dense(who, &model, &rq, NULL, NULL, 0) == 0 && rq.dense.head.form == FEAT_NONE && !soft_armed() && n_live[DEVICE_BLOCK] == 0,
          "vit_hip_set_dense(NULL) leaves it armed");
    CHECK(requests_set_dense_soft(who, &model, &rq, &head, &bins, &with_labels, &all_maps) == 0, "%s", last_error);
    CHECK(requests_set_dense_soft(who, &model, &rq, NULL, &bins, &with_labels, &all_maps) == 0 && rq.dense.head.form == FEAT_NONE && !soft_armed() &&
          n_live[DEVICE_BLOCK] == 0, "vit_hip_set_dense_soft(NULL, ...) leaves it armed");
    CHECK(requests_set_dense_soft(who, &model, &rq, NULL, NULL, NULL, NULL) == 0, "disarming the disarmed");
}

/* one refusal: code 1, the setter's name in front, `word` in the text, the armed request and the live blocks untouched */
static void refused(int rc, const char *word, const struct requests *was, int dev)
{
    CHECK(rc == 1, "rc %d", rc);
    CHECK(strncmp(last_error, "vit_hip_set_dense_soft: ", 24) == 0 && strstr(last_error, word), "refusal '%s' (expected '%s')", last_error, word);
    CHECK(memcmp(&rq, was, sizeof rq) == 0, "the armed request changed");
    CHECK(n_live[DEVICE_BLOCK] == dev && n_live[PINNED_BLOCK] == 0, "%d device blocks live, %d before", n_live[DEVICE_BLOCK], dev);
}

static void check_refusals(void)
{
    for (int start = 0; start < 3; ++start) {   /* over nothing, over a plain request, over a soft one */
        fresh();
        if (start == 1)
            CHECK(requests_set_dense(who, &model, &rq, &head, &with_labels, 0) == 0, "%s", last_error);
        if (start == 2)
            CHECK(requests_set_dense_soft(who, &model, &rq, &head, &bins, &with_labels, &all_maps) == 0, "%s", last_error);
        struct requests was;
        memcpy(&was, &rq, sizeof rq);
        const int dev = n_live[DEVICE_BLOCK];
        vit_dense_spec bad_spec;
        vit_dense_soft_spec bad_soft;
        vit_dense_soft_buffers bad_maps;
        vit_dense_buffers bad_bufs;
#define REFUSED(word, spec, soft, bufs, maps)                                                       \
    do {                                                                                            \
        snprintf(context, sizeof context, "start %d: %s", start, word);                             \
        last_error[0] = 0;                                                                          \
        refused(requests_set_dense_soft(who, &model, &rq, spec, soft, bufs, maps), word, &was, dev); \
    } while (0)
        /* what vit_hip_set_dense refuses about spec */
        bad_spec = head, bad_spec.n_labels = 1;
        REFUSED("n_labels", &bad_spec, &bins, &with_labels, &all_maps);
        bad_spec = head, bad_spec.n_labels = 257;
        REFUSED("n_labels", &bad_spec, &bins, &with_labels, &all_maps);
        bad_spec = head, bad_spec.tap = 2;
        REFUSED("tap", &bad_spec, &bins, &with_labels, &all_maps);
        bad_spec = head, bad_spec.out_h = 4097;
        REFUSED("out_h", &bad_spec, &bins, &with_labels, &all_maps);
        bad_spec = head, bad_spec.weight_stride = 60;
        REFUSED("weight_stride", &bad_spec, &bins, &with_labels, &all_maps);
        bad_spec = head, bad_spec.d_weight = NULL;
        REFUSED("no head weight", &bad_spec, &bins, &with_labels, &all_maps);
        bad_spec = head, bad_spec.d_weight = (const float *)(wt + 4);
        REFUSED("aligned", &bad_spec, &bins, &with_labels, &all_maps);
        bad_spec = head, bad_spec.d_bias = (const float *)(wt + 8);
        REFUSED("aligned", &bad_spec, &bins, &with_labels, &all_maps);
        /* the soft spec and the maps */
        REFUSED("NULL argument (soft)", &head, NULL, &with_labels, &all_maps);
        REFUSED("NULL argument (d_soft)", &head, &bins, &with_labels, NULL);
        bad_maps = (vit_dense_soft_buffers){NULL, NULL, NULL};
        REFUSED("no soft map", &head, &plain_soft, &with_labels, &bad_maps);
        REFUSED("no soft map", &head, &plain_soft, NULL, &bad_maps);            /* neither labels nor any map */
        REFUSED("d_values", &head, &plain_soft, &with_labels, &all_maps);       /* expect without d_values */
        REFUSED("d_values", &head, &bins, &with_labels, &prob_only);            /* d_values without expect */
        const float scales[] = {0.0f, -1.0f, INFINITY, -INFINITY, NAN};
        for (size_t k = 0; k < sizeof scales / sizeof scales[0]; ++k) {
            bad_soft = bins, bad_soft.logit_scale = scales[k];
            REFUSED("logit_scale", &head, &bad_soft, &with_labels, &all_maps);
        }
        bad_soft = bins, bad_soft.d_values = (const float *)(vals + 4);
        REFUSED("aligned", &head, &bad_soft, &with_labels, &all_maps);
        bad_maps = all_maps, bad_maps.prob = (float *)(pr + 4);
        REFUSED("aligned", &head, &bins, &with_labels, &bad_maps);
        bad_maps = all_maps, bad_maps.expect = (float *)(ex + 8);
        REFUSED("aligned", &head, &bins, &with_labels, &bad_maps);
        bad_maps = all_maps, bad_maps.entropy = (float *)(en + 4);
        REFUSED("aligned", &head, &bins, &with_labels, &bad_maps);
        bad_bufs = with_labels, bad_bufs.labels = (unsigned char *)(lab + 1);
        REFUSED("aligned", &head, &bins, &bad_bufs, &all_maps);
        bad_bufs = (vit_dense_buffers){NULL, NULL, (float *)(pl + 4)};
        REFUSED("aligned", &head, &bins, &bad_bufs, &all_maps);
        bad_bufs = (vit_dense_buffers){NULL, (float *)sc, NULL};
        REFUSED("scores need a labels buffer", &head, &bins, &bad_bufs, &all_maps);
#undef REFUSED
        /* and the request still arms */
        CHECK(requests_set_dense_soft(who, &model, &rq, &head, &bins, &with_labels, &all_maps) == 0, "%s", last_error);
    }
}

static void check_failure_at_every_allocation(void)
{
    const size_t small_ws = (size_t)MAX_BATCH * (TOKENS - 1) * 64 * 4 - 1;   /* the tokens do not fit: a second block */
    for (int start = 0; start < 3; ++start)
        for (int two = 0; two < 2; ++two) {
            model.ws_bytes = two ? small_ws : WS_BYTES;
            const int N = 1 + two;
            for (int k = 1; k <= N; ++k) {
                snprintf(context, sizeof context, "start %d, allocation %d of %d fails", start, k, N);
                fresh();
                if (start == 1)
                    CHECK(requests_set_dense(who, &model, &rq, &head, &with_labels, 0) == 0, "%s", last_error);
                if (start == 2)
                    CHECK(requests_set_dense_soft(who, &model, &rq, &head, &plain_soft, NULL, &prob_only) == 0, "%s", last_error);
                struct requests was;
                memcpy(&was, &rq, sizeof rq);
                const int dev = n_live[DEVICE_BLOCK];
                fail_in = k;
                last_error[0] = 0;
                const int rc = requests_set_dense_soft(who, &model, &rq, &head, &bins, &with_labels, &all_maps);
                CHECK(fail_in == 0, "the failure was never reached");
                CHECK(rc != 0 && strncmp(last_error, "vit_hip_set_dense_soft: ", 24) == 0 && strstr(last_error, "cannot be allocated"), "rc %d, '%s'", rc, last_error);
                CHECK(memcmp(&rq, &was, sizeof rq) == 0, "the armed request changed");
                CHECK(n_live[DEVICE_BLOCK] == dev && n_live[PINNED_BLOCK] == 0, "%d device blocks live, %d before", n_live[DEVICE_BLOCK], dev);
            }
            snprintf(context, sizeof context, "start %d, %d allocations succeed", start, N);
            fresh();
            const int before = n_allocs;
            CHECK(requests_set_dense_soft(who, &model, &rq, &head, &bins, &with_labels, &all_maps) == 0 && n_allocs == before + N &&
                  n_live[DEVICE_BLOCK] == N, "%d allocations: %s", n_allocs - before, last_error);
        }
    model.ws_bytes = WS_BYTES;
}

static void check_serving_and_last_layer(void)
{
    struct serving sv;
    snprintf(context, sizeof context, "what a forward serves");
    fresh();
    CHECK(requests_set_dense_soft(who, &model, &rq, &head, &bins, NULL, &all_maps) == 0, "%s", last_error);
    CHECK(requests_serving(&rq, "vit_hip_forward_device", FEAT_DEVICE, &sv) == 0 && sv.de == &rq.dense && !sv.fr && !sv.tk && !sv.ar && !sv.ro && !sv.ga,
          "the device form does not serve it");
    last_error[0] = 0;
    CHECK(requests_serving(&rq, "forward", FEAT_HOST, &sv) == 1 && !sv.de, "a host-form forward serves it");
    CHECK(strcmp(last_error, "forward: the context is armed for device dense buffers (vit_hip_set_dense); disarm it or use the device forms") == 0,
          "refusal '%s'", last_error);
    const struct staged *arrays[MAX_STAGED];
    CHECK(requests_serving(&rq, "vit_hip_forward_device", FEAT_DEVICE, &sv) == 0 && serving_staged(&sv, arrays) == 0, "a staged array");
    /* depth is 2: tap -1 is the last layer, which then runs on all rows */
    CHECK(serving_needs_last_layer_rows(&sv, 2), "a soft request on the last layer");
    vit_dense_spec early = head;
    early.tap = 0;
    CHECK(requests_set_dense_soft(who, &model, &rq, &early, &bins, NULL, &all_maps) == 0, "%s", last_error);
    CHECK(requests_serving(&rq, "vit_hip_forward_device", FEAT_DEVICE, &sv) == 0 && !serving_needs_last_layer_rows(&sv, 2), "a soft request on layer 0");
}

int main(void)
{
    check_arming();
    check_refusals();
    check_failure_at_every_allocation();
    check_serving_and_last_layer();
    fresh();
    printf("dense_soft: ok (%d allocations)\n", n_allocs);
    return 0;
}
