/*
 * planes_file_main.c -- csrc/vit_planes_file.c on its own, without a device.  "Device" memory is host memory; the six vh_*
 * the unit calls are memcpy, malloc and a counter per kind that can fail the k-th call.  Built by
 * tests/test_planes_file_host.py under ASan + UBSan (LeakSanitizer on) with a 1 MiB bounce buffer, so that every slab takes
 * several chunks and a ragged last one; exit status 0 = every check held.
 *   planes_file_main DIR
 * writes DIR/case_<i>.planes for every case and prints, for the Python side, "case | ..." (what to rebuild the file from),
 * "sweep | ..." (the offsets at which some mutation of a byte still loads), "ln_fold | ..." (what a mutated fold flag ran
 * into), "heads | ..." (whether another head count the shape allows loads) and one summary line per part.  The production
 * bounce buffer of 64 MiB, one chunk per slab at these sizes, is what the GPU round-trip tests run.
 *
 * Slab j of case i holds the 64-bit words mix(seed + k), k = 1.., seed = 16 i + j + 1 (little-endian, the last word cut);
 * scale k of case i is (mix(16 i + k + 1) >> 40) / 2^20.
 */
#include "vit_planes_file.h"

#include <fcntl.h>
#include <signal.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <sys/resource.h>
#include <sys/stat.h>
#include <unistd.h>

static char context[300];   /* the case under test, for a failure's message */
#define CHECK(cond, ...)                                               \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                              \
            fprintf(stderr, "\n  [%s]\n", context);                    \
            exit(1);                                                   \
        }                                                              \
    } while (0)

static char last_error[512];
int vh_set_error(int code, const char *message)
{
    snprintf(last_error, sizeof last_error, "%s", message);
    return code ? code : 1;
}

/* ---- the six vh_* of the unit: call number fail_in[kind] from now fails with FAIL_STATUS + kind ------------------------- */
enum { HOST_ALLOC, H2D, D2H, SYNC, N_KINDS, FAIL_STATUS = 700 };
static const char *const kind_name[N_KINDS] = {"vh_host_alloc", "vh_h2d", "vh_d2h", "vh_stream_sync"};
static int calls[N_KINDS], fail_in[N_KINDS], pinned_live, unsynced;
static char stream_tag;   /* its address is the stream the unit must pass on */

static int counted(int kind)
{
    ++calls[kind];
    if (fail_in[kind] > 0 && --fail_in[kind] == 0)
        return vh_set_error(FAIL_STATUS + kind, kind_name[kind]);
    return 0;
}

int vh_host_alloc(void **out, size_t bytes)
{
    CHECK(bytes > 0 && bytes <= PLANES_CHUNK_BYTES, "a bounce buffer of %zu bytes", bytes);
    const int rc = counted(HOST_ALLOC);
    if (rc)
        return rc;
    *out = malloc(bytes);
    ++pinned_live;
    return 0;
}

int vh_host_free(void *p)
{
    CHECK(p && pinned_live > 0, "a pinned block freed that is not live");
    free(p);
    --pinned_live;
    return 0;
}

static int copy(int kind, void *dst, const void *src, size_t bytes, vh_stream_t s)
{
    CHECK(s == (vh_stream_t)&stream_tag, "a copy on another stream");
    CHECK(unsynced == 0, "a copy through the bounce buffer before the last one was synchronised");
    const int rc = counted(kind);
    if (rc)
        return rc;
    memcpy(dst, src, bytes);
    unsynced = 1;
    return 0;
}
int vh_h2d(void *dst, const void *src, size_t bytes, vh_stream_t s) { return copy(H2D, dst, src, bytes, s); }
int vh_d2h(void *dst, const void *src, size_t bytes, vh_stream_t s) { return copy(D2H, dst, src, bytes, s); }

int vh_stream_sync(vh_stream_t s)
{
    CHECK(s == (vh_stream_t)&stream_tag, "a synchronisation of another stream");
    unsynced = 0;
    return counted(SYNC);
}

static void reset_counters(void)
{
    memset(calls, 0, sizeof calls);
    memset(fail_in, 0, sizeof fail_in);
    unsynced = 0;
}

/* ---- cases ------------------------------------------------------------------------------------------------------------------ */
static uint64_t mix(uint64_t z)
{
    z *= 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static void fill(void *p, size_t bytes, uint64_t seed)
{
    for (size_t k = 0; k < (bytes + 7) / 8; ++k) {
        const uint64_t w = mix(seed + k + 1);
        memcpy((char *)p + 8 * k, &w, bytes - 8 * k < 8 ? bytes - 8 * k : 8);
    }
}

enum { MAX_BATCH = 2, HEADER_BYTES = 120, MAX_CASES = 24, N_BIG = 10 };   /* cases 0 .. N_BIG - 1: the tiny and the padded shape */
struct model
{
    int index, n_tensors;
    vit_config cfg;
    struct vit_plan plan;
    float *scales;
    void *slabs[N_SLABS];
    size_t file_bytes;
    char path[400];
};
static struct model cases[MAX_CASES];
static int n_cases;
static const char *dir;

static void alloc_slabs(void *slabs[N_SLABS], const size_t bytes[N_SLABS])
{
    for (int j = 0; j < N_SLABS; ++j) {
        slabs[j] = bytes[j] ? malloc(bytes[j]) : NULL;
        if (bytes[j])
            memset(slabs[j], 0xa5, bytes[j]);
    }
}

static void free_slabs(void *slabs[N_SLABS])
{
    for (int j = 0; j < N_SLABS; ++j)
        free(slabs[j]);
}

static void make_cases(void)
{
    /* "17 tokens, 4 heads of 64" of tests/test_gpu_configs.py, and a shape whose conv_proj planes are padded (patch 14:
     * K = 588 -> 640), one layer of it */
    /* and two shapes small enough to pay for a pass over the payload per mutated scale byte (cases 10 .. 16, the sweep's
     * "small" cases): one layer, 5 tokens, one channel; embed 128 where the precision takes it, 256 for FP8_GEMM */
    const vit_config shapes[4] = {{64, 16, 3, 10, 256, 2, 4, 512, 1e-6}, {56, 14, 3, 10, 256, 1, 4, 512, 1e-6},
                                  {32, 16, 1, 10, 128, 1, 2, 128, 1e-6}, {32, 16, 1, 10, 256, 1, 4, 256, 1e-6}};
    const int precisions[4] = {VIT_PRECISION_F32, VIT_PRECISION_BF16_GEMM, VIT_PRECISION_FP8_GEMM, VIT_PRECISION_F32_FP16X2};
    struct plan_env env;
    plan_env_read(&env);
    int refused = 0;
    for (int s = 0; s < 4; ++s)
        for (int p = 0; p < 4; ++p)
            for (int fold = 0; fold < 2; ++fold) {
                struct model *m = &cases[n_cases];
                if (s == 1 && !((p == 0 && !fold) || (p == 1 && fold) || (p == 3 && !fold)))
                    continue;   /* the padded shape: F32, BF16_GEMM folded, F32_FP16X2 */
                if ((s == 2 && p == 2) || (s == 3 && p != 2))
                    continue;   /* the small shapes: embed 256 for FP8_GEMM alone */
                m->cfg = shapes[s];
                m->n_tensors = vit_config_num_tensors(&m->cfg);
                if (plan_make(&m->plan, &m->cfg, m->n_tensors, MAX_BATCH, precisions[p], fold, &env) != 0) {
                    ++refused;   /* the plan does not allow this fold: the fp16-pair emulation never folds */
                    CHECK(precisions[p] == VIT_PRECISION_F32_FP16X2 && fold == 1, "plan_make refused shape %d precision %d fold %d", s, p, fold);
                    continue;
                }
                CHECK(m->plan.ln_fold == fold && m->plan.precision == precisions[p], "the plan changed what it was given");
                m->index = n_cases++;
                m->scales = (float *)malloc(sizeof(float) * (size_t)m->n_tensors);
                for (int k = 0; k < m->n_tensors; ++k)
                    m->scales[k] = (float)(mix(16u * (uint64_t)m->index + (uint64_t)k + 1) >> 40) / 1048576.0f;
                alloc_slabs(m->slabs, m->plan.slab_bytes);
                m->file_bytes = HEADER_BYTES + sizeof(float) * (size_t)m->n_tensors;
                for (int j = 0; j < N_SLABS; ++j) {
                    fill(m->slabs[j], m->plan.slab_bytes[j], 16u * (uint64_t)m->index + (uint64_t)j + 1);
                    m->file_bytes += m->plan.slab_bytes[j];
                }
                snprintf(m->path, sizeof m->path, "%s/case_%d.planes", dir, m->index);
            }
    CHECK(n_cases == N_BIG + 7 && refused == 2, "%d cases, %d refused", n_cases, refused);
    CHECK(cases[8].cfg.patch_size == 14 && cases[8].plan.slab_bytes[SLAB_CONV] == (size_t)640 * 256 * 2, "the patch-14 planes are not padded to K = 640");
}

static int write_case(const struct model *m, const char *path)
{
    return planes_file_write(path, &m->cfg, &m->plan, m->n_tensors, m->scales, m->slabs, (vh_stream_t)&stream_tag);
}

static int lowest_free_fd(void)
{
    const int fd = open("/dev/null", O_RDONLY);
    CHECK(fd >= 0, "cannot open /dev/null");
    close(fd);
    return fd;
}

static size_t file_size(const char *path)
{
    struct stat st;
    return stat(path, &st) == 0 ? (size_t)st.st_size : (size_t)-1;
}

static int exists(const char *path)
{
    struct stat st;
    return stat(path, &st) == 0;
}

static void *slabs[N_SLABS];   /* what load reads into */
static size_t slab_bytes[N_SLABS];

/* Load `path` as vit_hip_create_from_planes does: open, then the slabs into allocations of the plan's sizes.  Returns the
 * status; with want, a load must give back exactly that case.  Counts the calls afresh; a failure that is set stays. */
static int load(const char *path, const struct model *want)
{
    static struct planes_file pf;
    memset(calls, 0, sizeof calls);
    unsynced = 0;
    int rc = planes_file_open(&pf, path, MAX_BATCH);
    if (rc != 0) {
        CHECK(pf.fp == NULL, "a refused file is left open");
        return rc;
    }
    CHECK(calls[HOST_ALLOC] + calls[H2D] + calls[D2H] + calls[SYNC] == 0, "planes_file_open touched the device or allocated");
    /* fresh slabs where they are compared; otherwise kept while the sizes stay: fresh pages cost more than the copies */
    if (want || memcmp(slab_bytes, pf.plan.slab_bytes, sizeof slab_bytes) != 0) {
        free_slabs(slabs);
        alloc_slabs(slabs, pf.plan.slab_bytes);
        memcpy(slab_bytes, pf.plan.slab_bytes, sizeof slab_bytes);
    }
    rc = planes_file_read_slabs(&pf, slabs, (vh_stream_t)&stream_tag);
    if (rc == 0 && want) {
        CHECK(memcmp(&pf.cfg, &want->cfg, sizeof(vit_config)) == 0 && pf.n_tensors == want->n_tensors, "config read back differs");
        CHECK(pf.plan.precision == want->plan.precision && pf.plan.ln_fold == want->plan.ln_fold, "precision or fold read back differs");
        CHECK(memcmp(pf.scales, want->scales, sizeof(float) * (size_t)want->n_tensors) == 0, "scales read back differ");
        for (int j = 0; j < N_SLABS; ++j) {
            CHECK(pf.plan.slab_bytes[j] == want->plan.slab_bytes[j], "slab %d: size differs", j);
            CHECK(pf.plan.slab_bytes[j] == 0 || memcmp(slabs[j], want->slabs[j], pf.plan.slab_bytes[j]) == 0, "slab %d read back differs", j);
        }
    }
    planes_file_close(&pf);
    CHECK(pinned_live == 0, "a bounce buffer is left");
    return rc;
}

static int is_refusal(int rc) { return rc == 1 || rc == 2 || rc == 121 || rc == 124 || rc == 125 || rc == 126; }

/* ---- 1. round trip -------------------------------------------------------------------------------------------------------- */
static void round_trips(void)
{
    for (int i = 0; i < n_cases; ++i) {
        const struct model *m = &cases[i];
        const vit_config *c = &m->cfg;
        snprintf(context, sizeof context, "round trip, case %d", i);
        reset_counters();
        CHECK(write_case(m, m->path) == 0, "write failed: %s", last_error);
        size_t chunks = 0;
        for (int j = 0; j < N_SLABS; ++j)
            chunks += (m->plan.slab_bytes[j] + PLANES_CHUNK_BYTES - 1) / PLANES_CHUNK_BYTES;
        CHECK(calls[HOST_ALLOC] == 1 && (size_t)calls[D2H] == chunks && (size_t)calls[SYNC] == chunks && calls[H2D] == 0,
              "a write of %zu chunks made %d allocations, %d copies, %d synchronisations", chunks, calls[HOST_ALLOC], calls[D2H], calls[SYNC]);
        CHECK(file_size(m->path) == m->file_bytes, "the file has %zu bytes, not %zu", file_size(m->path), m->file_bytes);
        char tmp[420];
        snprintf(tmp, sizeof tmp, "%s.tmp", m->path);
        CHECK(!exists(tmp), "the temporary is left");
        reset_counters();
        CHECK(load(m->path, m) == 0, "load failed: %s", last_error);
        CHECK(calls[HOST_ALLOC] == 1 && (size_t)calls[H2D] == chunks && (size_t)calls[SYNC] == chunks && calls[D2H] == 0, "a load's calls");
        printf("case | %d | %s | %d %d %d %d %d %d %d %d | %d %d %d | %zu %zu %zu %zu\n", i, m->path, c->img_size, c->patch_size, c->in_chans,
               c->num_classes, c->embed_dim, c->depth, c->num_heads, c->mlp_hidden, m->plan.precision, m->plan.ln_fold, m->n_tensors,
               m->plan.slab_bytes[0], m->plan.slab_bytes[1], m->plan.slab_bytes[2], m->plan.slab_bytes[3]);
    }
    printf("round trip: %d cases right\n", n_cases);
}

/* ---- 2. header and scales sweep ------------------------------------------------------------------------------------------ */
static void poke(const char *path, size_t at, unsigned char value)
{
    FILE *fp = fopen(path, "r+b");
    CHECK(fp && fseek(fp, (long)at, SEEK_SET) == 0 && fputc(value, fp) == value && fclose(fp) == 0, "cannot patch byte %zu", at);
}

static unsigned char peek(const char *path, size_t at)
{
    FILE *fp = fopen(path, "rb");
    CHECK(fp && fseek(fp, (long)at, SEEK_SET) == 0, "cannot read byte %zu", at);
    const int v = fgetc(fp);
    fclose(fp);
    CHECK(v != EOF, "no byte %zu", at);
    return (unsigned char)v;
}

static void sweep(void)
{
    long mutated = 0, loaded = 0;
    /* Every case: every byte of the header, the first and last byte of every slab.  A mutated scale is refused by the
     * checksum alone, behind a pass over the whole payload: every byte of the scales in the seven small cases (every
     * precision, folded and not), their first and last byte in the files of the tiny and the padded shape. */
    for (int i = 0; i < n_cases; ++i) {
        const struct model *m = &cases[i];
        const size_t scales_end = HEADER_BYTES + sizeof(float) * (size_t)m->n_tensors;
        size_t at[HEADER_BYTES + sizeof(float) * MAX_TENSORS + 2 * N_SLABS + 1], n_at = 0, slab_at = scales_end;
        const int every_scale = i >= N_BIG;
        int fold_seen = 0;
        for (size_t o = 0; o < scales_end; ++o)
            if (o < HEADER_BYTES || every_scale || o == HEADER_BYTES || o == scales_end - 1)
                at[n_at++] = o;
        for (int j = 0; j < N_SLABS; ++j)
            if (m->plan.slab_bytes[j]) {
                at[n_at++] = slab_at;
                at[n_at++] = slab_at + m->plan.slab_bytes[j] - 1;   /* the last slab's is the file's last byte */
                slab_at += m->plan.slab_bytes[j];
            }
        CHECK(slab_at == m->file_bytes, "offsets");
        /* beside the four mutations: num_heads halved and doubled, head counts the shape allows as well (byte 44 is its lowest) */
        const int heads[2] = {m->cfg.num_heads / 2, m->cfg.num_heads * 2};
        printf("heads | %d | %d ->", i, m->cfg.num_heads);
        for (int u = 0; u < 2; ++u) {
            snprintf(context, sizeof context, "sweep, case %d, num_heads %d -> %d", i, m->cfg.num_heads, heads[u]);
            poke(m->path, 44, (unsigned char)heads[u]);
            reset_counters();
            const int rc = load(m->path, NULL);
            CHECK(rc == 0 || is_refusal(rc), "status %d is none of the library's: %s", rc, last_error);
            printf(" %d: %s", heads[u], rc == 0 ? "loads" : "refused");
        }
        poke(m->path, 44, (unsigned char)m->cfg.num_heads);
        printf("\n");
        printf("sweep | %d | precision %d fold %d | %zu bytes, %s | loads at", i, m->plan.precision, m->plan.ln_fold, n_at,
               every_scale ? "every scale byte" : "the scales' first and last byte");
        for (size_t k = 0; k < n_at; ++k) {
            const unsigned char was = peek(m->path, at[k]);
            const unsigned char muts[4] = {(unsigned char)(was ^ 0x01), (unsigned char)(was ^ 0x80), 0x00, 0xFF};
            int loads = 0;
            for (int u = 0; u < 4; ++u) {
                if (muts[u] == was)
                    continue;
                snprintf(context, sizeof context, "sweep, case %d, byte %zu: 0x%02x -> 0x%02x", i, at[k], was, muts[u]);
                poke(m->path, at[k], muts[u]);
                reset_counters();
                const int rc = load(m->path, NULL);
                CHECK(rc == 0 || is_refusal(rc), "status %d is none of the library's: %s", rc, last_error);
                ++mutated;
                loads += rc == 0;
                if (at[k] >= 104 && at[k] < 108)   /* ln_fold: what a mutated flag ran into */
                    fold_seen |= rc == 0 ? 1 : rc == 125 ? 2 : rc == 2 ? 4 : 8;
            }
            poke(m->path, at[k], was);
            if (loads)
                printf(" %zu", at[k]);
            loaded += loads;
        }
        printf("\n");
        printf("ln_fold | %d | precision %d fold %d | a mutated flag:%s%s%s%s\n", i, m->plan.precision, m->plan.ln_fold, fold_seen & 1 ? " loads" : "",
               fold_seen & 2 ? " 125" : "", fold_seen & 4 ? " 2" : "", fold_seen & 8 ? " another status" : "");
        snprintf(context, sizeof context, "sweep, case %d, restored", i);
        CHECK(load(m->path, m) == 0, "the restored file does not load");
    }
    printf("sweep: %ld mutated files, %ld loaded, every other refused with a status of the library's\n", mutated, loaded);
}

/* ---- 3. truncation ---------------------------------------------------------------------------------------------------------- */
static int descending(const void *a, const void *b)
{
    const size_t x = *(const size_t *)a, y = *(const size_t *)b;
    return x > y ? -1 : x < y;
}

static void truncation(void)
{
    long cuts = 0;
    char path[420];
    snprintf(path, sizeof path, "%s/cut.planes", dir);
    for (int i = 0; i < n_cases; ++i) {
        const struct model *m = &cases[i];
        const size_t scales_end = HEADER_BYTES + sizeof(float) * (size_t)m->n_tensors;
        size_t len[HEADER_BYTES + sizeof(float) * MAX_TENSORS + 1 + 3 * N_SLABS], n_len = 0, end = scales_end;
        for (size_t o = 0; o <= scales_end; ++o)
            len[n_len++] = o;
        for (int j = 0; j < N_SLABS; ++j) {
            end += m->plan.slab_bytes[j];
            for (size_t o = end - 1; o <= end + 1; ++o)
                if (o > scales_end && o < m->file_bytes)
                    len[n_len++] = o;
        }
        qsort(len, n_len, sizeof len[0], descending);
        reset_counters();
        CHECK(write_case(m, path) == 0, "write failed: %s", last_error);
        for (size_t k = 0; k < n_len; ++k) {
            snprintf(context, sizeof context, "truncation, case %d, %zu of %zu bytes", i, len[k], m->file_bytes);
            CHECK(truncate(path, (off_t)len[k]) == 0 && file_size(path) == len[k], "cannot cut the file");
            reset_counters();
            const int rc = load(path, NULL);
            CHECK(rc == (len[k] < scales_end ? 124 : 121), "status %d: %s", rc, last_error);
            ++cuts;
        }
    }
    remove(path);
    printf("truncation: %ld cuts refused, short header or scales with 124, short payload with 121\n", cuts);
}

/* ---- 4. failing copies ---------------------------------------------------------------------------------------------------- */
static void failing_copies(void)
{
    long failed = 0;
    char path[420], tmp[430];
    snprintf(path, sizeof path, "%s/failing.planes", dir);
    snprintf(tmp, sizeof tmp, "%s.tmp", path);
    const int fd_before = lowest_free_fd();
    static const int failed_in[3] = {0, 5, 8};   /* F32 unfolded; FP8 folded; the padded shape in bf16, folded */
    for (int q = 0; q < 3; ++q) {
        const int i = failed_in[q];
        const struct model *m = &cases[i];
        int clean[2][N_KINDS];
        reset_counters();
        CHECK(write_case(m, path) == 0, "write failed");
        memcpy(clean[0], calls, sizeof calls);
        reset_counters();
        CHECK(load(path, m) == 0, "load failed");
        memcpy(clean[1], calls, sizeof calls);
        for (int reading = 0; reading < 2; ++reading)
            for (int kind = 0; kind < N_KINDS; ++kind)
                for (int k = 1; k <= clean[reading][kind]; ++k) {
                    snprintf(context, sizeof context, "case %d, %s, call %d of %s fails", i, reading ? "read" : "write", k, kind_name[kind]);
                    reset_counters();
                    fail_in[kind] = k;
                    const int rc = reading ? load(m->path, NULL) : write_case(m, path);
                    CHECK(rc == FAIL_STATUS + kind, "status %d, not the call's own", rc);
                    CHECK(pinned_live == 0 && lowest_free_fd() == fd_before, "a bounce buffer or a descriptor is left");
                    CHECK(reading || !exists(tmp), "the temporary is left");
                    ++failed;
                }
        /* the file under the final name is the one of the last complete write */
        reset_counters();
        CHECK(load(path, m) == 0, "the file a failed write should have left alone does not load");
    }
    remove(path);
    printf("failing copies: %ld calls failed in turn, each status came back, nothing left behind\n", failed);
}

/* ---- 5. failing writes ---------------------------------------------------------------------------------------------------- */
static void failing_writes(void)
{
    const struct model *m = &cases[1], *other = &cases[0];   /* the same shape, folded and not */
    char path[420], tmp[430];
    snprintf(path, sizeof path, "%s/short.planes", dir);
    snprintf(tmp, sizeof tmp, "%s.tmp", path);
    snprintf(context, sizeof context, "failing writes");
    reset_counters();
    CHECK(write_case(other, path) == 0, "write failed");
    const int fd_before = lowest_free_fd();
    struct rlimit old, lim;
    CHECK(getrlimit(RLIMIT_FSIZE, &old) == 0, "getrlimit");
    signal(SIGXFSZ, SIG_IGN);
    const size_t limits[5] = {64, 200, m->file_bytes / 2, m->file_bytes - 8, m->file_bytes - 1};
    for (int k = 0; k < 5; ++k) {
        snprintf(context, sizeof context, "failing writes, a file size limit of %zu bytes", limits[k]);
        lim = old;
        lim.rlim_cur = (rlim_t)limits[k];
        CHECK(setrlimit(RLIMIT_FSIZE, &lim) == 0, "setrlimit");
        reset_counters();
        const int rc = write_case(m, path);
        CHECK(setrlimit(RLIMIT_FSIZE, &old) == 0, "setrlimit back");
        CHECK(rc == 120, "status %d: %s", rc, last_error);
        CHECK(!exists(tmp) && pinned_live == 0 && lowest_free_fd() == fd_before, "the temporary, a bounce buffer or a descriptor is left");
        reset_counters();
        CHECK(load(path, other) == 0, "the good file under the name is no longer what it was");
    }
    signal(SIGXFSZ, SIG_DFL);
    char nowhere[440];
    snprintf(nowhere, sizeof nowhere, "%s/no_such_directory/x.planes", dir);
    snprintf(context, sizeof context, "paths");
    reset_counters();
    CHECK(write_case(m, nowhere) == 122, "a path in a directory that does not exist");
    CHECK(calls[HOST_ALLOC] + calls[D2H] == 0, "a file that cannot be opened still cost copies");
    CHECK(write_case(m, dir) == 122 && exists(dir), "a path that is a directory: the finished file cannot be moved into place");
    snprintf(tmp, sizeof tmp, "%s.tmp", dir);
    CHECK(!exists(tmp), "the temporary of the failed move is left");
    CHECK(load(nowhere, NULL) == 123, "a missing file");
    CHECK(load(NULL, NULL) == 1, "a NULL path");
    CHECK(lowest_free_fd() == fd_before, "a descriptor is left");
    remove(path);
    printf("failing writes: 5 size limits gave 120 and left the good file alone; 122, 122, 123 for the paths\n");
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: %s DIR\n", argv[0]);
        return 2;
    }
    dir = argv[1];
    make_cases();
    round_trips();
    sweep();
    truncation();
    failing_copies();
    failing_writes();
    for (int i = 0; i < n_cases; ++i) {
        free(cases[i].scales);
        free_slabs(cases[i].slabs);
    }
    free_slabs(slabs);
    printf("planes file: ok\n");
    return 0;
}
