/*
 * vit_multi.h -- several GPUs behind one call: what ViT_hip.c (the context), vit_multi.c (shards and replicas) and
 * vit_gather_rccl.c (the device-resident form with its RCCL gather) share.  Internal to the library.  vit_multi.c is plain
 * C over the public API and the entries below; tests/multi_main.c runs it over counting stand-ins, without a device.
 */
#ifndef VIT_MULTI_H
#define VIT_MULTI_H

#include "ViT_opencl.h"

#include <time.h>

enum { VIT_MAX_SHARDS = 64 };

/* the clock of the runner's per-shard times and of ViT_opencl()'s setup / forward split */
static inline double wall_seconds(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

struct vit_hip_multi
{
    int n_devices;
    vit_hip_ctx **ctx;
    /* creation arguments, read by the per-device threads */
    const vit_config *cfg;
    const Network *networks;
    const int *devices;
    int n_tensors, max_batch, precision;
    /* forward arguments */
    const ImageData *images;
    float *logits;
    float **probs;
    void *gather;   /* RCCL communicators of vit_hip_forward_device_multi (vit_gather_rccl.c), made on first use */
    double enqueue_ms[VIT_MAX_SHARDS];   /* vit_hip_forward_device_multi: host time each device's thread spent enqueuing its shard, last call */
};

/* ViT_hip.c: a context's own logits buffer, [max_batch][classes] */
float *vit_hip_logits_buffer(vit_hip_ctx *ctx);
/* ViT_hip.c: vit_hip_forward_device and vit_hip_forward with no armed output served, whatever a caller armed on the context */
int vit_hip_forward_device_plain(vit_hip_ctx *ctx, const float *d_images, int n, float *d_logits, float *d_probs, vh_stream_t stream);
int vit_hip_forward_plain(vit_hip_ctx *ctx, const ImageData *images, int n, float *logits, float **probs);
/* vit_gather_rccl.c: the communicators of a vit_hip_multi (NULL: none were made) */
void vit_gather_release(void *state);

#endif
