/*
 * multi_main.c -- csrc/vit_multi.c on its own, without a device: the shard ranges, the shard runner, and the replicas'
 * create / forward / destroy over counting stand-ins for vit_hip_create_ex, vit_hip_destroy, the plain host forward,
 * vit_hip_config, vh_last_error and vit_gather_release.  A stand-in context is a small heap block that remembers its device;
 * the stand-ins run on the runner's threads, so what they count sits behind a mutex.  Built and run by
 * tests/test_multi_host.py once under ASan + UBSan and once under ThreadSanitizer; exit status 0 = every check held.
 */
#include "vit_multi.h"

#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static char context[200];
#define CHECK(cond, ...)                                               \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                              \
            fprintf(stderr, "\n  [%s]\n", context);                    \
            exit(1);                                                   \
        }                                                              \
    } while (0)

/* ---- the stand-ins ---------------------------------------------------------------------------------------------------------- */
enum { CLASSES = 10, MAX_IMAGES = 130 };
struct vit_hip_ctx
{
    int device, destroyed;
};
static pthread_mutex_t lock = PTHREAD_MUTEX_INITIALIZER;
static vit_hip_ctx *made[VIT_MAX_SHARDS];
static int n_made, n_destroyed, fail_device = -1, gather_released;
static const vit_config the_cfg = {64, 16, 3, CLASSES, 256, 2, 4, 512, 1e-6};
static const Network *the_networks;
static char gather_state;

const char *vh_last_error(void) { return "a stand-in's error"; }
const vit_config *vit_hip_config(const vit_hip_ctx *ctx) { (void)ctx; return &the_cfg; }

void vit_gather_release(void *state)
{
    CHECK(state == NULL || state == &gather_state, "another gather state");
    gather_released += state != NULL;
}

int vit_hip_create_ex(vit_hip_ctx **out, const vit_config *cfg, const Network *networks, int n_tensors, int device, int max_batch,
                      int precision)
{
    CHECK(cfg == &the_cfg && networks == the_networks && n_tensors == 32 && max_batch == 7 && precision == VIT_PRECISION_BF16_GEMM,
          "creation arguments did not arrive");
    *out = NULL;
    if (device == fail_device)
        return 40 + device;
    vit_hip_ctx *ctx = (vit_hip_ctx *)calloc(1, sizeof(*ctx));
    ctx->device = device;
    pthread_mutex_lock(&lock);
    made[n_made++] = ctx;
    pthread_mutex_unlock(&lock);
    *out = ctx;
    return 0;
}

void vit_hip_destroy(vit_hip_ctx *ctx)
{
    if (!ctx)
        return;
    pthread_mutex_lock(&lock);
    CHECK(!ctx->destroyed, "a context destroyed twice");
    ctx->destroyed = 1;   /* the block is freed by the test, which first looks at the flag */
    ++n_destroyed;
    pthread_mutex_unlock(&lock);
}

/* the plain host forward: logits row r of image i = 1000 device + i's tag, probs row the same + 0.5; fails on a tagged image */
static int fail_image = -1;
int vit_hip_forward_plain(vit_hip_ctx *ctx, const ImageData *images, int n, float *logits, float **probs)
{
    for (int i = 0; i < n; ++i) {
        const int tag = images[i].n;   /* the image's index in the caller's array */
        if (tag == fail_image)
            return 90 + ctx->device;
        for (int c = 0; c < CLASSES; ++c) {
            if (logits)
                logits[(size_t)i * CLASSES + c] = (float)(1000 * ctx->device + tag);
            if (probs)
                probs[i][c] = (float)(1000 * ctx->device + tag) + 0.5f;
        }
    }
    return 0;
}

/* ---- shard ranges ----------------------------------------------------------------------------------------------------------- */
static void shard_ranges(void)
{
    for (int total = 0; total <= 130; ++total)
        for (int shards = 1; shards <= VIT_MAX_SHARDS; ++shards) {
            int at = 0, empty_seen = 0;
            snprintf(context, sizeof context, "ranges, %d images over %d shards", total, shards);
            for (int s = 0; s < shards; ++s) {
                int lo = -1, hi = -1;
                vit_shard_range(total, s, shards, &lo, &hi);
                CHECK(lo == at && hi >= lo && hi <= total, "shard %d is [%d, %d) behind %d", s, lo, hi, at);
                CHECK(!(empty_seen && hi > lo), "a non-empty shard behind an empty one");
                empty_seen |= hi == lo;
                at = hi;
            }
            CHECK(at == total, "the shards end at %d", at);
        }
    printf("ranges: contiguous, disjoint, covering, empty shards last for 0..130 images over 1..64 shards\n");
}

/* ---- the runner ------------------------------------------------------------------------------------------------------------- */
struct run_log
{
    int entered[VIT_MAX_SHARDS], fail_mask_lo, fail_mask_hi;
};

static int logged(void *arg, int shard, int lo, int hi)
{
    struct run_log *log = (struct run_log *)arg;
    CHECK(hi > lo, "an empty shard was run");
    log->entered[shard] += 1;   /* one writer per element */
    return shard >= log->fail_mask_lo && shard < log->fail_mask_hi ? 10 + shard : 0;
}

static void runner(void)
{
    struct run_log log;
    double ms[VIT_MAX_SHARDS + 1];
    snprintf(context, sizeof context, "runner, refusals");
    CHECK(vit_shard_run_timed(8, 0, logged, &log, NULL) == 1 && vit_shard_run_timed(8, 65, logged, &log, ms) == 1 &&
          vit_shard_run_timed(8, 4, NULL, &log, NULL) == 1 && vit_shard_run(-1, 4, logged, &log) == 1, "0 shards, 65 shards, no function, -1 images");
    for (int shards = 1; shards <= VIT_MAX_SHARDS; shards += shards < 8 ? 1 : 28)   /* 1..8, 36, 64 */
        for (int first_bad = 0; first_bad <= shards; ++first_bad) {   /* shards first_bad.. fail; first_bad == shards: none */
            snprintf(context, sizeof context, "runner, %d shards, failing from %d", shards, first_bad);
            memset(&log, 0, sizeof log);
            log.fail_mask_lo = first_bad;
            log.fail_mask_hi = shards;
            ms[shards] = -1.0;
            const int rc = vit_shard_run_timed(shards, shards, logged, &log, ms);
            CHECK(rc == (first_bad < shards ? 10 + first_bad : 0), "status %d is not the lowest failing shard's", rc);
            for (int s = 0; s < shards; ++s)
                CHECK(log.entered[s] == 1 && ms[s] >= 0.0, "shard %d ran %d times", s, log.entered[s]);
            CHECK(ms[shards] == -1.0, "a time written behind the last shard");
        }
    /* more shards than images: the empty ones are not entered and their time is 0 */
    snprintf(context, sizeof context, "runner, 3 images over 8 shards");
    memset(&log, 0, sizeof log);
    log.fail_mask_lo = log.fail_mask_hi = 0;
    for (int s = 0; s < 8; ++s)
        ms[s] = -1.0;
    CHECK(vit_shard_run_timed(3, 8, logged, &log, ms) == 0, "status");
    for (int s = 0; s < 8; ++s)
        CHECK(log.entered[s] == (s < 3) && (s < 3 || ms[s] == 0.0), "shard %d", s);
    printf("runner: refusals, the lowest failing shard's status with every other shard still run, empty shards skipped\n");
}

/* ---- create, forward, destroy -------------------------------------------------------------------------------------------- */
static void forget_contexts(void)
{
    for (int i = 0; i < n_made; ++i) {
        CHECK(made[i]->destroyed, "the context of device %d was never destroyed", made[i]->device);
        free(made[i]);
    }
    CHECK(n_destroyed == n_made, "%d contexts made, %d destroyed", n_made, n_destroyed);
    n_made = n_destroyed = 0;
}

static void replicas(void)
{
    static const int counts[4] = {1, 2, 3, 8};
    static Network networks[1];
    static vit_hip_multi sentinel;
    int devices[8], creations = 0;
    the_networks = networks;
    for (int d = 0; d < 8; ++d)
        devices[d] = 3 * d + 1;
    vit_hip_multi *m = &sentinel;   /* a refusal leaves NULL */
    snprintf(context, sizeof context, "create, refusals");
    CHECK(vit_hip_create_multi(NULL, &the_cfg, networks, 32, devices, 2, 7, 1) == 1 && vit_hip_create_multi(&m, NULL, networks, 32, devices, 2, 7, 1) == 1 &&
          vit_hip_create_multi(&m, &the_cfg, NULL, 32, devices, 2, 7, 1) == 1 && vit_hip_create_multi(&m, &the_cfg, networks, 32, NULL, 2, 7, 1) == 1 &&
          vit_hip_create_multi(&m, &the_cfg, networks, 32, devices, 0, 7, 1) == 1 && vit_hip_create_multi(&m, &the_cfg, networks, 32, devices, 65, 7, 1) == 1 &&
          vit_hip_create_multi(&m, &the_cfg, networks, 32, devices, 2, 0, 1) == 1 && n_made == 0, "bad arguments");
    for (int k = 0; k < 4; ++k)
        for (int bad = 0; bad < counts[k]; ++bad) {
            snprintf(context, sizeof context, "create, %d devices, device index %d fails", counts[k], bad);
            fail_device = devices[bad];
            m = &sentinel;   /* a refusal leaves NULL */
            const int rc = vit_hip_create_multi(&m, &the_cfg, networks, 32, devices, counts[k], 7, VIT_PRECISION_BF16_GEMM);
            CHECK(rc == 40 + devices[bad] && m == NULL, "status %d, *out %p", rc, (void *)m);
            CHECK(n_made == counts[k] - 1, "%d contexts made", n_made);   /* every other device was still built */
            forget_contexts();
            ++creations;
        }
    fail_device = -1;

    /* the forward's scatter: 13 images over 3 devices (5, 5, 3), either output NULL */
    snprintf(context, sizeof context, "forward");
    int dev_list[3] = {4, 9, 2};
    CHECK(vit_hip_create_multi(&m, &the_cfg, networks, 32, dev_list, 3, 7, VIT_PRECISION_BF16_GEMM) == 0 && m, "create");
    dev_list[1] = -1;   /* the list is copied */
    CHECK(vit_hip_multi_devices(m) == 3 && vit_hip_multi_devices(NULL) == 0 && vit_hip_multi_ctx(m, 3) == NULL && vit_hip_multi_ctx(m, -1) == NULL, "accessors");
    for (int d = 0; d < 3; ++d)
        CHECK(vit_hip_multi_ctx(m, d) && vit_hip_multi_ctx(m, d)->device == (d == 0 ? 4 : d == 1 ? 9 : 2), "device %d's context", d);
    enum { N = 13 };
    ImageData images[N];
    float logits[N * CLASSES], rows[N][CLASSES], *probs[N];
    memset(images, 0, sizeof images);
    for (int i = 0; i < N; ++i) {
        images[i].n = i;
        probs[i] = rows[i];
    }
    CHECK(vit_hip_forward_multi(NULL, images, N, logits, probs) == 1 && vit_hip_forward_multi(m, NULL, N, logits, probs) == 1 &&
          vit_hip_forward_multi(m, images, 0, logits, probs) == 1, "bad arguments");
    for (int form = 0; form < 4; ++form) {   /* both, logits only, probs only, neither */
        float *lg = form == 0 || form == 1 ? logits : NULL, **pr = form == 0 || form == 2 ? probs : NULL;
        memset(logits, 0, sizeof logits);
        memset(rows, 0, sizeof rows);
        CHECK(vit_hip_forward_multi(m, images, N, lg, pr) == 0, "form %d", form);
        for (int i = 0; i < N; ++i) {
            const float want = (float)(1000 * (i < 5 ? 4 : i < 10 ? 9 : 2) + i);
            for (int c = 0; c < CLASSES; ++c) {
                CHECK(logits[i * CLASSES + c] == (lg ? want : 0.0f), "form %d: logits of image %d", form, i);
                CHECK(rows[i][c] == (pr ? want + 0.5f : 0.0f), "form %d: probs of image %d", form, i);
            }
        }
    }
    fail_image = 11;   /* in the third shard */
    CHECK(vit_hip_forward_multi(m, images, N, logits, probs) == 92, "a failing shard's status");
    fail_image = -1;
    double ms[3];
    m->enqueue_ms[0] = 1.5, m->enqueue_ms[1] = 2.5, m->enqueue_ms[2] = 3.5;
    CHECK(vit_hip_multi_last_enqueue_ms(m, ms, 2) == -1 && vit_hip_multi_last_enqueue_ms(NULL, ms, 3) == -1 &&
          vit_hip_multi_last_enqueue_ms(m, ms, 3) == 3 && ms[0] == 1.5 && ms[2] == 3.5, "the enqueue times");
    m->gather = &gather_state;
    vit_hip_destroy_multi(m);
    vit_hip_destroy_multi(NULL);
    CHECK(gather_released == 1, "the gather state was released %d times", gather_released);
    forget_contexts();
    printf("replicas: creation failed clean at each device index of 1, 2, 3 and 8 devices (%d creations); the forward scatters 13 images over 3 devices in 4 forms\n",
           creations);
}

int main(void)
{
    shard_ranges();
    runner();
    replicas();
    printf("multi: ok\n");
    return 0;
}
