/*
 * vit_planes_file.h -- the repacked-weights file (vit_hip_export_planes / vit_hip_create_from_planes): its format, its writer
 * and its reader.  Internal to the library.  The unit knows no context: it works on what a file is made of -- a vit_config,
 * the plan's precision, fold flag and slab sizes, the tensor count, one pair scale per tensor, the slab pointers and a
 * stream.  vit_planes_file.c is plain C and needs no device: its outside symbols are vh_set_error, vh_host_alloc,
 * vh_host_free, vh_h2d, vh_d2h, vh_stream_sync, plan_env_read / plan_make and stdio.  tests/planes_file_main.c runs it over
 * host copies of those six.
 *
 * The file: a 120-byte header ("VITPLN02", layout version 2; DESIGN.md 10 has the fields), n_tensors pair scales, then the
 * slabs in the order of vit_plan.h.  The header's checksum is FNV-1a over 64-bit words of the scales and the slabs; the
 * header itself is not hashed (DESIGN.md 10 lists the header bytes nothing protects).
 */
#ifndef VIT_PLANES_FILE_H
#define VIT_PLANES_FILE_H

#include "vit_plan.h"

#include <stdio.h>

/* Bumped whenever a repack kernel changes what it writes for the same (config, precision): the slab sizes alone would
 * not notice (csrc/gemm_p3.hip planes, csrc/gemm_mx.hip MX values / scale order, the fold terms of csrc/norm_fold.h).
 * tests/test_gpu_planes_golden.py holds every section of the files this version names against its recording. */
#define VIT_PLANES_LAYOUT_VERSION 2

/* A file whose header and scales have been accepted: what the context adopts, and where the slabs begin */
struct planes_file
{
    FILE *fp;                   /* behind the scales; NULL once closed */
    vit_config cfg;
    int n_tensors;
    struct vit_plan plan;       /* plan_make of the header's shape, precision and fold flag, for the caller's max_batch */
    float scales[MAX_TENSORS];  /* [n_tensors] */
    unsigned long long checksum, hash;   /* the header's, and FNV-1a of what has been read so far */
};

/* Everything that is decided before a device is touched, in this order: open (123), magic / header size / layout version
 * (124), the n_tensors bound and plan_make under the environment's switches (its status, or 2), the slab sizes and the
 * count of scales against the plan's (125), the scales (124).  Allocates nothing on host or device; on a refusal the file
 * is closed again. */
int planes_file_open(struct planes_file *pf, const char *path, int max_batch);

/* The slabs, of pf->plan.slab_bytes, into the caller's allocations through one pinned bounce buffer of at most 64 MiB,
 * one synchronisation per chunk: 121 for a file shorter than its header says, 126 where the checksum does not hold, or a
 * copy's own status. */
int planes_file_read_slabs(struct planes_file *pf, void *const slabs[N_SLABS], vh_stream_t stream);

void planes_file_close(struct planes_file *pf);

/* Written to `path`.tmp and renamed over `path` when complete: an interrupted export never leaves a truncated file under
 * the name a later run will open.  122: the file cannot be opened or moved into place; 120: a short write; or a copy's own
 * status; the temporary is removed on every failure. */
int planes_file_write(const char *path, const vit_config *cfg, const struct vit_plan *plan, int n_tensors, const float *scales,
                      void *const slabs[N_SLABS], vh_stream_t stream);

#endif
