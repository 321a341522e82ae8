/*
 * plan_main.c -- csrc/vit_plan.c on its own, without a device, against tests/golden/plan_table.txt: one line per case, the
 * inputs (model shape, batch, precision, fold flag, the six switches as text), then what the plan was when the table was
 * recorded.  For every line plan_make must reproduce it, plan_layout must size the slabs as recorded and place every
 * tensor and operand 256-byte aligned, inside its slab and clear of the others; and every borrower of an arena buffer must
 * fit it.  Built and run by tests/test_plan_host.py under ASan + UBSan; exit status 0 = every check held.
 *   plan_main TABLE          the checks
 *   plan_main TABLE limits   print what the sizing functions of csrc/kernel_limits.h, which the plan calls, return for every
 *                            shape (the library's exported entries are held against them)
 *   plan_main TABLE record   print the table as this code plans it, the inputs kept: how a change that alters a plan cell on
 *                            purpose re-records it
 */
#include "vit_plan.h"
#include "kernel_limits.h"
#include "vit_ingest.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static char last_error[512];
int vh_set_error(int code, const char *message)
{
    snprintf(last_error, sizeof last_error, "%s", message);
    return code ? code : 1;
}

static char context[1200];   /* the line under test, for a failure's message */
#define CHECK(cond, ...)                                              \
    do {                                                              \
        if (!(cond)) {                                                \
            fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                             \
            fprintf(stderr, "\n  [%s]\n", context);                   \
            exit(1);                                                  \
        }                                                             \
    } while (0)

struct piece
{
    uintptr_t at;
    size_t bytes;
};

static int by_address(const void *a, const void *b)
{
    const struct piece *x = (const struct piece *)a, *y = (const struct piece *)b;
    return x->at < y->at ? -1 : x->at > y->at;
}

/* plan_layout with slabs at made-up addresses: every piece aligned, inside its slab, none overlapping */
static void check_layout(const struct vit_plan *plan, const vit_config *cfg)
{
    size_t bytes[N_SLABS];
    plan_layout(plan, cfg, NULL, NULL, NULL, bytes);
    CHECK(memcmp(bytes, plan->slab_bytes, sizeof bytes) == 0, "sizing twice gives other sizes");
    void *slabs[N_SLABS];
    for (int i = 0; i < N_SLABS; ++i)   /* as the context does: a slab of no bytes is not allocated */
        slabs[i] = bytes[i] ? (void *)((uintptr_t)(i + 1) << 40) : NULL;
    const int nt = vit_config_num_tensors(cfg), n_op = 4 * cfg->depth;
    float **w = calloc((size_t)nt, sizeof *w);
    struct operand *op = calloc((size_t)n_op, sizeof *op);
    struct piece *pc = calloc((size_t)(nt + 4 * n_op), sizeof *pc);
    plan_layout(plan, cfg, slabs, w, op, NULL);
    int n = 0;
    for (int i = 0; i < nt; ++i)
        pc[n++] = (struct piece){(uintptr_t)w[i], vit_config_tensor_size(cfg, i) * sizeof(float)};
    for (int m = 0; m < n_op; ++m) {
        const size_t cnt = vit_config_tensor_size(cfg, plan_operand_tensor(m)), out_f = vit_config_tensor_size(cfg, plan_operand_tensor(m) + 1);
        CHECK((op[m].w != NULL) == (plan->operand_bytes > 0), "operand %d", m);
        CHECK((op[m].scales != NULL) == plan->operand_scales, "operand %d scales", m);
        CHECK((op[m].colsum != NULL) == (plan->ln_fold && m % 2 == 0) && (op[m].bias_folded != NULL) == (op[m].colsum != NULL), "operand %d fold terms", m);
        if (op[m].w)
            pc[n++] = (struct piece){(uintptr_t)op[m].w, cnt * (size_t)plan->operand_bytes};
        if (op[m].scales)
            pc[n++] = (struct piece){(uintptr_t)op[m].scales, cnt / 32};
        if (op[m].colsum) {
            pc[n++] = (struct piece){(uintptr_t)op[m].colsum, out_f * sizeof(float)};
            pc[n++] = (struct piece){(uintptr_t)op[m].bias_folded, out_f * sizeof(float)};
        }
    }
    qsort(pc, (size_t)n, sizeof *pc, by_address);
    for (int i = 0; i < n; ++i) {
        const int s = (int)(pc[i].at >> 40) - 1;
        CHECK(s >= 0 && s < N_SLABS && slabs[s], "piece %d lies in no slab", i);
        CHECK(pc[i].at % 256 == 0, "piece %d is not 256-byte aligned", i);
        CHECK(pc[i].at + pc[i].bytes <= (uintptr_t)slabs[s] + bytes[s], "piece %d ends outside slab %d", i, s);
        CHECK(i == 0 || pc[i - 1].at + pc[i - 1].bytes <= pc[i].at, "pieces %d and %d overlap", i - 1, i);
    }
    /* conv_proj's planes are the whole of their slab */
    CHECK(bytes[SLAB_CONV] == (size_t)kl_patch_planes_k(cfg->in_chans, cfg->patch_size) * (size_t)cfg->embed_dim * 2 * (size_t)plan->conv_parts,
          "conv slab");
    free(pc);
    free(op);
    free(w);
}

/* What the recorded parent never stated: every borrower fits the buffer it borrows, and the Q|K|V form is the one the
 * attention maps derived for themselves */
static void check_invariants(const struct vit_plan *plan, const vit_config *cfg, int max_batch)
{
    const size_t n = (size_t)max_batch, E = (size_t)cfg->embed_dim, F = (size_t)cfg->mlp_hidden, rows = n * (size_t)plan->tokens;
    const size_t img = (size_t)cfg->in_chans * cfg->img_size * cfg->img_size;
    const int p = plan->precision, reduced = p == VIT_PRECISION_BF16_GEMM || p == VIT_PRECISION_FP8_GEMM;
    const int form = reduced ? (plan->attn_form == ATTN_STREAMING ? VH_QKV_ROWS_F32 : VH_QKV_PLANES_F16)
                   : p == VIT_PRECISION_F32 && plan->use_p3 && (plan->attn_form == ATTN_HD64 || plan->attn_form == ATTN_LONG)
                       ? VH_QKV_PLANES3 : VH_QKV_ROWS_F32;
    CHECK(plan->qkv_form == form, "qkv_form %d, the attention maps read form %d", plan->qkv_form, form);
    /* the planes paths' streaming and long attention write fp32 rows into hid */
    if ((plan->use_p3 || reduced) && (plan->attn_form == ATTN_STREAMING || plan->attn_form == ATTN_LONG))
        CHECK(rows * E * 4 <= plan->ws_bytes, "attention rows: %zu bytes into hid of %zu", rows * E * 4, plan->ws_bytes);
    CHECK(rows * F * (size_t)plan->act_bytes <= plan->ws_bytes && rows * E * (size_t)plan->act_bytes <= plan->y_bytes &&
          plan->attn_bytes == plan->y_bytes && rows * 3 * E * (size_t)plan->act_bytes <= plan->qkv_bytes, "activations");
    if (p == VIT_PRECISION_FP8_GEMM) {   /* MX scales behind the values */
        CHECK(plan->e_scales_off >= rows * E && plan->e_scales_off % 256 == 0 &&
              plan->e_scales_off + kl_mx_act_scale_bytes((int)rows, cfg->embed_dim) <= plan->y_bytes, "scales in y and attn");
        CHECK(plan->hid_scales_off >= rows * F && plan->hid_scales_off % 256 == 0 &&
              plan->hid_scales_off + kl_mx_act_scale_bytes((int)rows, cfg->mlp_hidden) <= plan->ws_bytes, "scales in hid");
    }
    if (plan->cls_only_ok) {   /* x_cls fp32, then attn_cls, y_cls, hid_cls as three-part planes, each 256-byte aligned */
        size_t off[3];
        const size_t scratch = plan_cls_only_scratch(cfg, max_batch, off);
        CHECK(plan->use_p3 && !plan->ln_fold && plan->tokens >= 4, "class-only last layer where it cannot run");
        CHECK(off[0] >= n * E * 4 && off[1] >= off[0] + n * E * 6 && off[2] >= off[1] + n * E * 6 && scratch == off[2] + n * F * 6 &&
              off[0] % 256 == 0 && off[1] % 256 == 0 && off[2] % 256 == 0, "class-only scratch layout");
        CHECK(scratch <= plan->qkv_bytes, "class-only scratch: %zu bytes into Q|K|V of %zu", scratch, plan->qkv_bytes);
    }
    CHECK(!plan->cls_only_last || (plan->use_p3 && !plan->ln_fold), "cls_only_last");
    /* the expansion of 8-bit images, and the crops behind it */
    if (!plan->planes_patch_embed)
        CHECK(n * img * 4 <= plan->crop_off && n * img * 4 <= plan->qkv_bytes, "expanded images");
    if (cfg->in_chans <= 4) {
        CHECK(plan->crop_off % 256 == 0 && plan->crop_off + n * img <= plan->qkv_bytes, "crops");
        CHECK(n * ingest_max_table_bytes(cfg->img_size) <= plan->ws_bytes, "resize tables");
    }
    CHECK(kl_patch_rows_workspace(max_batch, cfg->in_chans, cfg->img_size, cfg->img_size, cfg->patch_size, cfg->embed_dim) <= plan->ws_bytes,
          "patch workspace");
    CHECK((plan->stats_bytes != 0) == plan->ln_fold, "stats");
}

int main(int argc, char **argv)
{
    if (argc < 2)
        return 2;
    const int limits = argc > 2 && strcmp(argv[2], "limits") == 0, record = argc > 2 && strcmp(argv[2], "record") == 0;
    FILE *fp = fopen(argv[1], "r");
    if (!fp)
        return 2;
    int lines = 0, plans = 0, edited = 0;
    char line[1200], want[1200];
    while (fgets(line, sizeof line, fp)) {
        line[strcspn(line, "\n")] = 0;
        if (line[0] == '#' || line[0] == 0) {
            if (record)
                puts(line);
            continue;
        }
        snprintf(context, sizeof context, "%s", line);
        char *note = strstr(line, "  # ");   /* a hand-edited line says what the parent had */
        if (note) {
            *note = 0;
            ++edited;
        }
        int img, patch, chans, classes, E, depth, heads, F, nt, mb, fold;
        char prec[16], e[PLAN_ENV_COUNT][32];
        CHECK(sscanf(line, "%d %d %d %d %d %d %d %d %d %d %15s %d %31s %31s %31s %31s %31s %31s", &img, &patch, &chans, &classes, &E, &depth,
                     &heads, &F, &nt, &mb, prec, &fold, e[0], e[1], e[2], e[3], e[4], e[5]) == 18, "cannot parse");
        char *arrow = strstr(line, " => ");
        CHECK(arrow || record, "no result");   /* record: a new case is its inputs alone */
        const int in_len = arrow ? (int)(arrow - line) : (int)strlen(line);
        const char *values[PLAN_ENV_COUNT];
        for (int i = 0; i < PLAN_ENV_COUNT; ++i)
            values[i] = strcmp(e[i], "-") == 0 ? NULL : e[i];
        struct plan_env env;
        plan_env_parse(&env, values);
        const int precision = strcmp(prec, "env") == 0 ? env.precision : atoi(prec);
        const vit_config cfg = {img, patch, chans, classes, E, depth, heads, F, 1e-6};
        struct vit_plan plan;
        last_error[0] = 0;
        const int rc = plan_make(&plan, &cfg, nt, mb, precision, fold, &env);
        ++lines;
        if (rc) {
            snprintf(want, sizeof want, "%.*s => %d %s", in_len, line, rc, last_error[0] ? last_error : "-");
            if (record)
                puts(want);
            else
                CHECK(strcmp(want, line) == 0, "plan_make gives\n  %s", want);
            continue;
        }
        if (limits) {
            const int rows = mb * plan.tokens;
            printf("%d %d %d %d %d %d %d : %d %d %zu %zu %zu\n", chans, patch, img, E, F, mb, rows, kl_layer_norm_planes_max_embed(3),
                   kl_patch_planes_k(chans, patch), kl_patch_rows_workspace(mb, chans, img, img, patch, E), kl_mx_act_scale_bytes(rows, E),
                   kl_mx_act_scale_bytes(rows, F));
            continue;
        }
        snprintf(want, sizeof want, "%.*s => 0 p=%d fold=%d p3=%d cls=%d attn=%d native=%d tiled=%d T=%d form=%d wp=%d ob=%d os=%d cp=%d ppe=%d "
                 "act=%d clsok=%d slabs=%zu,%zu,%zu,%zu x=%zu y=%zu at=%zu qkv=%zu hid=%zu stats=%zu crop=%zu",
                 in_len, line, plan.precision, plan.ln_fold, plan.use_p3, plan.cls_only_last, plan.attn_form, plan.fp32_native,
                 plan.attn_rows_streaming, plan.tokens, plan.qkv_form, plan.weight_planes, plan.operand_bytes, plan.operand_scales,
                 plan.conv_parts, plan.planes_patch_embed, plan.act_bytes, plan.cls_only_ok, plan.slab_bytes[0], plan.slab_bytes[1],
                 plan.slab_bytes[2], plan.slab_bytes[3], plan.x_bytes, plan.y_bytes, plan.attn_bytes, plan.qkv_bytes, plan.ws_bytes,
                 plan.stats_bytes, plan.crop_off);
        if (record) {
            puts(want);
            continue;
        }
        CHECK(strcmp(want, line) == 0, "plan_make gives\n  %s", want);
        check_layout(&plan, &cfg);
        check_invariants(&plan, &cfg, mb);
        ++plans;
    }
    fclose(fp);
    if (!limits && !record)
        printf("plan table: ok (%d lines, %d plans, %d hand-edited)\n", lines, plans, edited);
    return 0;
}
