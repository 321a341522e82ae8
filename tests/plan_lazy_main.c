/*
 * plan_lazy_main.c -- the lazy last layer's part of csrc/vit_plan.c, without a device, over every case of
 * tests/golden/plan_table.txt (the format of tests/plan_main.c, which holds everything else about the plan):
 *   - last_layer_lazy is set exactly where cls_only_ok holds, $VIT_HIP_LAST_LAYER=full clears it and changes nothing else,
 *     $VIT_HIP_LAST_LAYER=all_queries keeps it and clears cls_query alone;
 *   - cls_only_last, cls_only_ok and the class-only scratch offsets are what they were: the first two against the table's
 *     recorded cells, the offsets against the arithmetic restated here;
 *   - cls_query only with the lazy layer on the resident three-part attention, and its scratch -- the class-only scratch with
 *     the class query's planes behind it -- ends in front of K in Q|K|V at every batch from 1 to max_batch.
 * Built and run by tests/test_plan_lazy_host.py under ASan + UBSan; exit status 0 = every check held.
 */
#include "vit_plan.h"
#include "vit_ingest.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int vh_set_error(int code, const char *message)
{
    (void)message;
    return code ? code : 1;
}

static char context[1200];
#define CHECK(cond, ...)                                              \
    do {                                                              \
        if (!(cond)) {                                                \
            fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                             \
            fprintf(stderr, "\n  [%s]\n", context);                   \
            exit(1);                                                  \
        }                                                             \
    } while (0)

static size_t up256(size_t v) { return (v + 255) / 256 * 256; }

/* the recorded value of a cell such as " cls=" */
static int cell(const char *line, const char *key)
{
    const char *at = strstr(line, key);
    CHECK(at, "no cell %s", key);
    return atoi(at + strlen(key));
}

/* equal in every field but the two this change adds */
static int same_but_lazy(struct vit_plan a, struct vit_plan b)
{
    a.last_layer_lazy = b.last_layer_lazy = 0;
    a.cls_query = b.cls_query = 0;
    return memcmp(&a, &b, sizeof a) == 0;
}

int main(int argc, char **argv)
{
    if (argc < 2)
        return 2;
    FILE *fp = fopen(argv[1], "r");
    if (!fp)
        return 2;
    int plans = 0, lazy = 0, query = 0, lazy_not_query = 0;
    char line[1200];
    while (fgets(line, sizeof line, fp)) {
        line[strcspn(line, "\n")] = 0;
        if (line[0] == '#' || line[0] == 0)
            continue;
        snprintf(context, sizeof context, "%s", line);
        int img, patch, chans, classes, E, depth, heads, F, nt, mb, fold;
        char prec[16], e[PLAN_ENV_COUNT][32];
        CHECK(sscanf(line, "%d %d %d %d %d %d %d %d %d %d %15s %d %31s %31s %31s %31s %31s %31s", &img, &patch, &chans, &classes, &E, &depth,
                     &heads, &F, &nt, &mb, prec, &fold, e[0], e[1], e[2], e[3], e[4], e[5]) == 18, "cannot parse");
        const char *arrow = strstr(line, " => ");
        CHECK(arrow, "no result");
        if (atoi(arrow + 4) != 0)   /* a refused case: no plan */
            continue;
        const char *values[PLAN_ENV_COUNT];
        for (int i = 0; i < PLAN_ENV_COUNT; ++i)
            values[i] = strcmp(e[i], "-") == 0 ? NULL : e[i];
        CHECK(!values[PLAN_ENV_LAST_LAYER] || strcmp(values[PLAN_ENV_LAST_LAYER], "full") != 0, "the table predates the value");
        const vit_config cfg = {img, patch, chans, classes, E, depth, heads, F, 1e-6};
        struct plan_env env;
        struct vit_plan plan, unset, full, allq;
        plan_env_parse(&env, values);
        const int precision = strcmp(prec, "env") == 0 ? env.precision : atoi(prec);
        CHECK(plan_make(&plan, &cfg, nt, mb, precision, fold, &env) == 0, "plan_make");
        ++plans;

        /* what was there stays */
        CHECK(plan.cls_only_last == cell(arrow, " cls=") && plan.cls_only_ok == cell(arrow, " clsok="), "cls=%d clsok=%d", plan.cls_only_last,
              plan.cls_only_ok);
        const int n_of[] = {1, 2, 3, mb};
        for (int i = 0; i < 4; ++i) {
            const size_t n = (size_t)(n_of[i] < mb ? n_of[i] : mb);
            size_t off[3], q_off = 0;
            const size_t o0 = up256(n * (size_t)E * 4), o1 = o0 + up256(n * (size_t)E * 6), o2 = o1 + up256(n * (size_t)E * 6);
            const size_t bytes = plan_cls_only_scratch(&cfg, (int)n, off);
            CHECK(off[0] == o0 && off[1] == o1 && off[2] == o2 && bytes == o2 + n * (size_t)F * 6, "class-only scratch at n=%zu", n);
            const size_t with_q = plan_cls_query_scratch(&cfg, (int)n, &q_off);
            CHECK(q_off >= bytes && q_off % 256 == 0 && q_off < bytes + 256 && with_q == q_off + n * (size_t)E * 6, "class query's planes at n=%zu", n);
            if (plan.cls_query)   /* K of these n images begins behind their Q planes */
                CHECK(with_q <= n * (size_t)plan.tokens * (size_t)E * 6, "n=%zu: scratch of %zu bytes runs into K at %zu", n, with_q,
                      n * (size_t)plan.tokens * (size_t)E * 6);
        }

        /* the new fields */
        const int all_queries = values[PLAN_ENV_LAST_LAYER] && strcmp(values[PLAN_ENV_LAST_LAYER], "all_queries") == 0;
        CHECK(plan.last_layer_lazy == plan.cls_only_ok, "lazy=%d where clsok=%d", plan.last_layer_lazy, plan.cls_only_ok);
        CHECK(!plan.cls_query || (plan.last_layer_lazy && !all_queries && plan.attn_form == ATTN_HD64 && plan.qkv_form == VH_QKV_PLANES3 &&
                                  plan.precision == VIT_PRECISION_F32 && plan.use_p3 && !plan.ln_fold),
              "cls_query where it cannot run");

        /* the switch: against the same case with $VIT_HIP_LAST_LAYER unset */
        values[PLAN_ENV_LAST_LAYER] = NULL;
        plan_env_parse(&env, values);
        CHECK(plan_make(&unset, &cfg, nt, mb, precision, fold, &env) == 0, "plan_make, unset");
        values[PLAN_ENV_LAST_LAYER] = "full";
        plan_env_parse(&env, values);
        CHECK(env.last_layer_full && !env.last_layer_cls, "full parses");
        CHECK(plan_make(&full, &cfg, nt, mb, precision, fold, &env) == 0, "plan_make, full");
        CHECK(!full.last_layer_lazy && !full.cls_query && !full.cls_only_last && same_but_lazy(full, unset), "full changes more than the lazy fields");
        values[PLAN_ENV_LAST_LAYER] = "all_queries";
        plan_env_parse(&env, values);
        CHECK(plan_make(&allq, &cfg, nt, mb, precision, fold, &env) == 0, "plan_make, all_queries");
        CHECK(allq.last_layer_lazy == unset.last_layer_lazy && !allq.cls_query && same_but_lazy(allq, unset), "all_queries");
        CHECK(unset.last_layer_lazy == unset.cls_only_ok, "unset");

        lazy += plan.last_layer_lazy;
        query += plan.cls_query;
        lazy_not_query += plan.last_layer_lazy && !plan.cls_query;
    }
    fclose(fp);
    printf("lazy last layer: ok (%d plans, %d lazy, %d with the class query, %d lazy without it)\n", plans, lazy, query, lazy_not_query);
    return 0;
}
