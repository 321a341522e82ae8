/*
 * vit_multi.c -- several GPUs behind one call: the shard runner and the device replicas (csrc/vit_multi.h).
 *
 * Images never interact (the reference processes them strictly one at a time, ViT_opencl.c:926), so the batch is cut into
 * contiguous shards, one per device; every device holds a full replica of the weights (346 MB for ViT-B/16) and is driven
 * by its own host thread, context and stream.  A thread writes its shard's outputs straight into the caller's arrays, so
 * inside one process the "gather of the class logits" is this scatter -- no collective.  (bench.py's one-process-per-GPU
 * form gathers with RCCL instead; vit_gather_rccl.c is the device-resident form of one process.)
 */
#include "vit_multi.h"

#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void vit_shard_range(int total, int shard, int n_shards, int *lo, int *hi)
{
    const int per = n_shards > 0 ? (total + n_shards - 1) / n_shards : total;
    int a = shard * per, b;
    if (a > total)
        a = total;
    b = a + per;
    if (b > total)
        b = total;
    *lo = a;
    *hi = b;
}

struct shard_job
{
    int (*fn)(void *arg, int shard, int lo, int hi);
    void *arg;
    int shard, lo, hi, rc;
    double ms;          /* wall time of fn on its thread */
    char err[256];
};

static void *shard_worker(void *p)
{
    struct shard_job *j = (struct shard_job *)p;
    const double t0 = wall_seconds();
    j->rc = j->fn(j->arg, j->shard, j->lo, j->hi);
    j->ms = 1e3 * (wall_seconds() - t0);
    if (j->rc != 0)
        snprintf(j->err, sizeof(j->err), "%s", vh_last_error());   /* the error text is per thread */
    return NULL;
}

/* Run fn(arg, s, lo_s, hi_s) for the n_shards contiguous shards of [0, total), each non-empty shard
 * on its own host thread (shard 0 on the caller's); returns 0 or the first failing shard's status. */
int vit_shard_run(int total, int n_shards, int (*fn)(void *arg, int shard, int lo, int hi), void *arg)
{
    return vit_shard_run_timed(total, n_shards, fn, arg, NULL);
}

/* The same; ms_per_shard[s] (may be NULL) receives the wall time shard s's fn took on its thread (0 for an empty shard). */
int vit_shard_run_timed(int total, int n_shards, int (*fn)(void *arg, int shard, int lo, int hi), void *arg, double *ms_per_shard)
{
    if (total < 0 || n_shards <= 0 || n_shards > VIT_MAX_SHARDS || !fn)
        return 1;
    struct shard_job jobs[VIT_MAX_SHARDS];
    pthread_t tid[VIT_MAX_SHARDS];
    int threaded[VIT_MAX_SHARDS];
    for (int s = 0; s < n_shards; ++s) {
        jobs[s] = (struct shard_job){fn, arg, s, 0, 0, 0, 0.0, ""};
        vit_shard_range(total, s, n_shards, &jobs[s].lo, &jobs[s].hi);
        threaded[s] = 0;
    }
    for (int s = 1; s < n_shards; ++s)
        if (jobs[s].hi > jobs[s].lo)
            threaded[s] = pthread_create(&tid[s], NULL, shard_worker, &jobs[s]) == 0;
    for (int s = 0; s < n_shards; ++s)
        if (!threaded[s] && jobs[s].hi > jobs[s].lo)
            shard_worker(&jobs[s]);               /* shard 0, and any shard whose thread could not start */
    for (int s = 1; s < n_shards; ++s)
        if (threaded[s])
            pthread_join(tid[s], NULL);
    if (ms_per_shard)
        for (int s = 0; s < n_shards; ++s)
            ms_per_shard[s] = jobs[s].ms;
    for (int s = 0; s < n_shards; ++s)
        if (jobs[s].rc != 0) {
            fprintf(stderr, "vit_shard_run: shard %d [%d, %d) failed with status %d: %s\n", s, jobs[s].lo, jobs[s].hi,
                    jobs[s].rc, jobs[s].err);
            return jobs[s].rc;
        }
    return 0;
}

int vit_hip_multi_last_enqueue_ms(const vit_hip_multi *m, double *ms, int capacity)
{
    if (!m || !ms || capacity < m->n_devices)
        return -1;
    for (int d = 0; d < m->n_devices; ++d)
        ms[d] = m->enqueue_ms[d];
    return m->n_devices;
}

static int multi_create_one(void *arg, int shard, int lo, int hi)
{
    vit_hip_multi *m = (vit_hip_multi *)arg;
    (void)lo;
    (void)hi;
    return vit_hip_create_ex(&m->ctx[shard], m->cfg, m->networks, m->n_tensors, m->devices[shard], m->max_batch,
                             m->precision);
}

int vit_hip_create_multi(vit_hip_multi **out, const vit_config *cfg, const Network *networks, int n_tensors,
                         const int *devices, int n_devices, int max_batch_per_device, int precision)
{
    if (!out || !cfg || !networks || !devices || n_devices <= 0 || n_devices > VIT_MAX_SHARDS || max_batch_per_device <= 0)
        return 1;
    *out = NULL;
    vit_hip_multi *m = (vit_hip_multi *)calloc(1, sizeof(*m));
    if (!m)
        return 4;
    m->ctx = (vit_hip_ctx **)calloc((size_t)n_devices, sizeof(*m->ctx));
    int *devs = (int *)malloc(sizeof(int) * (size_t)n_devices);
    if (!m->ctx || !devs) {
        free(m->ctx);
        free(devs);
        free(m);
        return 4;
    }
    memcpy(devs, devices, sizeof(int) * (size_t)n_devices);
    m->n_devices = n_devices;
    m->cfg = cfg;
    m->networks = networks;
    m->devices = devs;
    m->n_tensors = n_tensors;
    m->max_batch = max_batch_per_device;
    m->precision = precision;
    /* one "shard" per device: the replicas are built side by side (weight upload + repack each) */
    const int rc = vit_shard_run(n_devices, n_devices, multi_create_one, m);
    m->cfg = NULL;
    m->networks = NULL;
    if (rc != 0) {
        vit_hip_destroy_multi(m);
        return rc;
    }
    *out = m;
    return 0;
}

void vit_hip_destroy_multi(vit_hip_multi *m)
{
    if (!m)
        return;
    vit_gather_release(m->gather);
    for (int d = 0; d < m->n_devices; ++d)
        vit_hip_destroy(m->ctx[d]);
    free((void *)m->devices);
    free(m->ctx);
    free(m);
}

int vit_hip_multi_devices(const vit_hip_multi *m) { return m ? m->n_devices : 0; }
vit_hip_ctx *vit_hip_multi_ctx(const vit_hip_multi *m, int i) { return (m && i >= 0 && i < m->n_devices) ? m->ctx[i] : NULL; }

static int multi_forward_one(void *arg, int shard, int lo, int hi)
{
    vit_hip_multi *m = (vit_hip_multi *)arg;
    const size_t NC = (size_t)vit_hip_config(m->ctx[shard])->num_classes;
    /* no feature, top-k or attention-map output, whatever a caller armed on the shard's context */
    return vit_hip_forward_plain(m->ctx[shard], m->images + lo, hi - lo, m->logits ? m->logits + (size_t)lo * NC : NULL,
                                 m->probs ? m->probs + lo : NULL);
}

/* Not re-entrant on one vit_hip_multi (like vit_hip_forward on one context). */
int vit_hip_forward_multi(vit_hip_multi *m, const ImageData *images, int n, float *logits, float **probs)
{
    if (!m || !images || n <= 0)
        return 1;
    m->images = images;
    m->logits = logits;
    m->probs = probs;
    return vit_shard_run(n, m->n_devices, multi_forward_one, m);
}
