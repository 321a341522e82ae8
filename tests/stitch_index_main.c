/*
 * stitch_index_main.c -- csrc/vit_stitch.c on its own, without a device.  Reads cases from standard input, one after the
 * other: "frame_h frame_w block n" and n boxes of four floats (hexadecimal floats are taken, so a case is exact); for each
 * it calls vit_stitch_index three ways -- sizing only, sizing with offsets, and filling arrays of exactly the sizes it named
 * -- checks that the three agree and that one id less of capacity is refused, and prints
 *     ok <n_ids> / offsets ... / ids ...        or        refused <the message>
 * A case whose block is negative runs vit_stitch_check alone with who = "caller".  Built and run by
 * tests/test_stitch_host.py under ASan + UBSan, which compares what is printed with tests/stitch_ref.py's per-pixel statement.
 */
#include "ViT_opencl.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static char last_error[512];
int vh_set_error(int code, const char *message)
{
    snprintf(last_error, sizeof last_error, "%s", message);
    return code ? code : 1;
}

#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

int main(void)
{
    int h, w, block, n, cases = 0;
    while (scanf("%d %d %d %d", &h, &w, &block, &n) == 4) {
        const int count = n > 0 ? n : 0;
        float *boxes = malloc((size_t)(count ? count : 1) * 4 * sizeof(float));
        REQUIRE(boxes);
        for (int i = 0; i < 4 * count; ++i)
            REQUIRE(scanf("%f", &boxes[i]) == 1);
        ++cases;
        last_error[0] = 0;
        if (block < 0) {
            if (vit_stitch_check(h, w, n == -1 ? NULL : boxes, n, "caller"))
                printf("refused %s\n", last_error);
            else
                printf("ok 0\n");
            free(boxes);
            continue;
        }
        const long total = vit_stitch_index(h, w, block, boxes, n, NULL, NULL, 0);
        if (total < 0) {
            printf("refused %s\n", last_error);
            REQUIRE(strncmp(last_error, "vit_stitch_index: ", 18) == 0);
            free(boxes);
            continue;
        }
        const long blocks = (long)((h + block - 1) / block) * ((w + block - 1) / block);
        int *sized = malloc((size_t)(blocks + 1) * sizeof(int)), *offsets = malloc((size_t)(blocks + 1) * sizeof(int));
        int *ids = malloc((size_t)(total ? total : 1) * sizeof(int));
        REQUIRE(sized && offsets && ids);
        REQUIRE(vit_stitch_index(h, w, block, boxes, n, sized, NULL, 0) == total);
        REQUIRE(vit_stitch_index(h, w, block, boxes, n, offsets, ids, total) == total);
        REQUIRE(memcmp(sized, offsets, (size_t)(blocks + 1) * sizeof(int)) == 0);
        REQUIRE(offsets[0] == 0 && offsets[blocks] == total);
        if (total > 0) {   /* one id less of capacity: refused, and said so */
            REQUIRE(vit_stitch_index(h, w, block, boxes, n, sized, ids, total - 1) == -1);
            REQUIRE(strstr(last_error, "capacity"));
        }
        REQUIRE(vit_stitch_index(h, w, block, boxes, n, NULL, ids, total) == -1);   /* ids without offsets */
        REQUIRE(vit_stitch_index(h, w, block, boxes, n, offsets, ids, total) == total);
        printf("ok %ld\noffsets", total);
        for (long k = 0; k <= blocks; ++k)
            printf(" %d", offsets[k]);
        printf("\nids");
        for (long k = 0; k < total; ++k)
            printf(" %d", ids[k]);
        printf("\n");
        free(sized);
        free(offsets);
        free(ids);
        free(boxes);
    }
    printf("stitch index: %d cases\n", cases);
    return 0;
}
