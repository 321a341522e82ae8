/*
 * vit_planes_file.c -- the repacked-weights file: format, writer and reader (csrc/vit_planes_file.h).  The only code in the
 * library that parses bytes it did not produce (the offline half of the weight-format tooling).
 *
 * A file holds what a context has in HBM after its repack -- the fp32 slab (all tensors, the reference's order, 256-byte
 * aligned) followed by the mode's operand slab for the four big matrices of every layer (three-part bf16 planes, one-part
 * planes, two fp16 parts, or MX values + scales: csrc/gemm_p3.hip, gemm_mx.hip), the conv_proj planes and, with ln_fold,
 * the fold terms -- behind a header that pins model shape and precision.  Every slab's layout follows from (config,
 * precision, ln_fold) alone (plan_layout), so loading is one read per slab into its allocation: no fp32 -> format pass, no
 * per-tensor files (the reference's loader opens 152 of them, Network.c:134-218).
 */
#include "vit_planes_file.h"

#include <stdlib.h>
#include <string.h>

struct planes_header
{
    char magic[8];                 /* "VITPLN02" */
    unsigned header_bytes;
    int precision, n_tensors;
    int cfg_ints[8];               /* img, patch, chans, classes, embed, depth, heads, mlp_hidden */
    double eps;
    unsigned long long w_slab_bytes, planes_bytes, wconv16_bytes, scale_floats;   /* scale_floats = n_tensors (pair scales) */
    unsigned long long fold_bytes; /* colsum + folded bias of the gamma-scaled matrices (ln_fold) */
    int ln_fold, layout_version;
    unsigned long long checksum;   /* of everything behind the header, in file order (planes_hash) */
};

/* FNV-1a over 64-bit words (the payload slabs are all multiples of 8 bytes; a tail is taken byte-wise) */
static unsigned long long planes_hash(unsigned long long h, const void *data, size_t bytes)
{
    const unsigned long long *w = (const unsigned long long *)data;
    for (size_t i = 0; i < bytes / 8; ++i)
        h = (h ^ w[i]) * 0x100000001b3ull;
    const unsigned char *t = (const unsigned char *)data + (bytes & ~(size_t)7);
    for (size_t i = 0; i < (bytes & 7); ++i)
        h = (h ^ t[i]) * 0x100000001b3ull;
    return h;
}
#define PLANES_HASH_SEED 0xcbf29ce484222325ull

/* the bounce buffer's size; a multiple of 8, so the hash does not depend on it (tests/planes_file_main.c builds with a small one) */
#ifndef PLANES_CHUNK_BYTES
#define PLANES_CHUNK_BYTES (64 << 20)
#endif
enum { CHUNK = PLANES_CHUNK_BYTES };

/* The pinned bounce buffer of a file: the largest slab, or CHUNK; *out stays NULL where every slab is empty */
static int bounce_alloc(void **out, const size_t slab_bytes[N_SLABS])
{
    size_t most = 0;
    for (int i = 0; i < N_SLABS; ++i)
        most = slab_bytes[i] > most ? slab_bytes[i] : most;
    *out = NULL;
    return most ? vh_host_alloc(out, most < CHUNK ? most : (size_t)CHUNK) : 0;
}

/* One slab between the file and the device, CHUNK bytes at a time through `host`, hashed as it passes */
static int copy_file_and_device(FILE *fp, void *host, void *dev, size_t bytes, int to_file, vh_stream_t stream, unsigned long long *hash)
{
    int rc = 0;
    for (size_t off = 0; off < bytes; off += CHUNK) {
        const size_t n = bytes - off < CHUNK ? bytes - off : (size_t)CHUNK;
        if (to_file) {
            if ((rc = vh_d2h(host, (char *)dev + off, n, stream)) != 0 || (rc = vh_stream_sync(stream)) != 0)
                return rc;
            *hash = planes_hash(*hash, host, n);
            if (fwrite(host, 1, n, fp) != n)
                return vh_set_error(120, "vit_hip_export_planes: short write");
        } else {
            if (fread(host, 1, n, fp) != n)
                return vh_set_error(121, "vit_hip_create_from_planes: file is shorter than its header says");
            *hash = planes_hash(*hash, host, n);
            if ((rc = vh_h2d((char *)dev + off, host, n, stream)) != 0 || (rc = vh_stream_sync(stream)) != 0)
                return rc;
        }
    }
    return 0;
}

int planes_file_write(const char *path, const vit_config *c, const struct vit_plan *plan, int n_tensors, const float *scales,
                      void *const slabs[N_SLABS], vh_stream_t stream)
{
    int rc = 0;
    const size_t plen = strlen(path);
    char *tmp = (char *)malloc(plen + 5);
    if (!tmp)
        return vh_set_error(4, "vit_hip_export_planes: out of host memory");
    memcpy(tmp, path, plen);
    memcpy(tmp + plen, ".tmp", 5);
    FILE *fp = fopen(tmp, "wb");
    if (!fp) {
        free(tmp);
        return vh_set_error(122, "vit_hip_export_planes: cannot open the file for writing");
    }
    struct planes_header h;
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, "VITPLN02", 8);
    h.header_bytes = (unsigned)sizeof(h);
    h.precision = plan->precision;
    h.n_tensors = n_tensors;
    const int ints[8] = {c->img_size, c->patch_size, c->in_chans, c->num_classes, c->embed_dim, c->depth, c->num_heads, c->mlp_hidden};
    memcpy(h.cfg_ints, ints, sizeof(ints));
    h.eps = c->eps;
    h.w_slab_bytes = plan->slab_bytes[SLAB_F32];
    h.planes_bytes = plan->slab_bytes[SLAB_OPERAND];
    h.wconv16_bytes = plan->slab_bytes[SLAB_CONV];
    h.fold_bytes = plan->slab_bytes[SLAB_FOLD];
    h.ln_fold = plan->ln_fold;
    h.layout_version = VIT_PLANES_LAYOUT_VERSION;
    h.scale_floats = (unsigned long long)n_tensors;
    unsigned long long hash = planes_hash(PLANES_HASH_SEED, scales, sizeof(float) * (size_t)n_tensors);
    void *host = NULL;
    /* the header goes first with a zero checksum and is rewritten once the payload has been hashed */
    if (fwrite(&h, sizeof(h), 1, fp) != 1 || fwrite(scales, sizeof(float), (size_t)n_tensors, fp) != (size_t)n_tensors)
        rc = vh_set_error(120, "vit_hip_export_planes: short write");
    if (rc == 0)
        rc = bounce_alloc(&host, plan->slab_bytes);
    for (int i = 0; i < N_SLABS && rc == 0; ++i)
        rc = copy_file_and_device(fp, host, slabs[i], plan->slab_bytes[i], 1, stream, &hash);
    if (host)
        vh_host_free(host);
    if (rc == 0) {
        h.checksum = hash;
        if (fseek(fp, 0, SEEK_SET) != 0 || fwrite(&h, sizeof(h), 1, fp) != 1)
            rc = vh_set_error(120, "vit_hip_export_planes: short write");
    }
    if (fclose(fp) != 0 && rc == 0)
        rc = vh_set_error(120, "vit_hip_export_planes: short write");
    if (rc == 0 && rename(tmp, path) != 0)
        rc = vh_set_error(122, "vit_hip_export_planes: cannot move the finished file into place");
    if (rc != 0)
        remove(tmp);
    free(tmp);
    return rc;
}

int planes_file_open(struct planes_file *pf, const char *path, int max_batch)
{
    int rc = 0;
    pf->fp = NULL;
    if (!path)
        return vh_set_error(1, "vit_hip_create_from_planes: null path");
    FILE *fp = fopen(path, "rb");
    if (!fp)
        return vh_set_error(123, "vit_hip_create_from_planes: cannot open the file");
    struct planes_header h;
    struct plan_env env;
    if (fread(&h, sizeof(h), 1, fp) != 1 || memcmp(h.magic, "VITPLN02", 8) != 0 || h.header_bytes != sizeof(h) ||
        h.layout_version != VIT_PLANES_LAYOUT_VERSION) {
        rc = vh_set_error(124, "vit_hip_create_from_planes: not a planes file of this library version (magic, header size or operand-layout version)");
        goto fail;
    }
    /* the header holds one image side: a file's context is square (img_width 0), every byte of the config written */
    const vit_config from_header = {h.cfg_ints[0], h.cfg_ints[1], h.cfg_ints[2], h.cfg_ints[3], h.cfg_ints[4], h.cfg_ints[5], h.cfg_ints[6],
                                    h.cfg_ints[7], h.eps, 0};
    memset(&pf->cfg, 0, sizeof pf->cfg);
    (void)vit_config_canonical(&from_header, &pf->cfg, NULL);   /* a square config is never refused there: plan_make judges it */
    pf->n_tensors = h.n_tensors;
    /* plan_make bounds every dimension and checks the fold flag (n_tensors is tied to depth) */
    plan_env_read(&env);
    if (h.n_tensors <= 0 || h.n_tensors > MAX_TENSORS ||
        (rc = plan_make(&pf->plan, &pf->cfg, h.n_tensors, max_batch, h.precision, h.ln_fold ? 1 : 0, &env)) != 0) {
        rc = vh_set_error(rc ? rc : 2, "vit_hip_create_from_planes: the header's model shape or precision is not one this library takes");
        goto fail;
    }
    /* the slab sizes this library derives from (shape, precision, fold) against the header's, BEFORE anything is allocated */
    const size_t *sizes = pf->plan.slab_bytes;
    if (h.w_slab_bytes != sizes[SLAB_F32] || h.planes_bytes != sizes[SLAB_OPERAND] || h.wconv16_bytes != sizes[SLAB_CONV] ||
        h.fold_bytes != sizes[SLAB_FOLD] || h.scale_floats != (unsigned long long)h.n_tensors) {
        rc = vh_set_error(125, "vit_hip_create_from_planes: slab sizes in the file do not match this library's layout");
        goto fail;
    }
    if (fread(pf->scales, sizeof(float), (size_t)h.n_tensors, fp) != (size_t)h.n_tensors) {
        rc = vh_set_error(124, "vit_hip_create_from_planes: truncated header");
        goto fail;
    }
    pf->checksum = h.checksum;
    pf->hash = planes_hash(PLANES_HASH_SEED, pf->scales, sizeof(float) * (size_t)h.n_tensors);
    pf->fp = fp;
    return 0;
fail:
    fclose(fp);
    return rc;
}

int planes_file_read_slabs(struct planes_file *pf, void *const slabs[N_SLABS], vh_stream_t stream)
{
    void *host = NULL;
    int rc = bounce_alloc(&host, pf->plan.slab_bytes);
    for (int i = 0; i < N_SLABS && rc == 0; ++i)
        rc = copy_file_and_device(pf->fp, host, slabs[i], pf->plan.slab_bytes[i], 0, stream, &pf->hash);
    if (host)
        vh_host_free(host);
    if (rc == 0 && pf->hash != pf->checksum)
        rc = vh_set_error(126, "vit_hip_create_from_planes: payload checksum mismatch (corrupt file)");
    return rc;
}

void planes_file_close(struct planes_file *pf)
{
    if (pf->fp)
        fclose(pf->fp);
    pf->fp = NULL;
}
