/*
 * resample_check_main.c -- vit_resample_check (csrc/vit_config.c) in a stand-alone program, built with vit_config.c alone
 * under AddressSanitizer and UBSan by tests/test_pos_resample_host.py: what it accepts, every refusal with its text, and an
 * output config that is the source itself.  The shim's error text is a stand-in here.
 */
#include "ViT_opencl.h"
#include <stdio.h>
#include <string.h>

static char g_err[512];
const char *vh_last_error(void) { return g_err; }
int vh_set_error(int code, const char *message)
{
    snprintf(g_err, sizeof g_err, "%s", message ? message : "");
    return code ? code : 1;
}

static int fails;
#define EXPECT(cond) do { if (!(cond)) { printf("FAIL line %d: %s\n", __LINE__, #cond); ++fails; } } while (0)

int main(void)
{
    vit_config b, out, tiny;
    vit_pos_resample how = {VIT_POS_BICUBIC, 0};
    EXPECT(vit_config_preset(&b, "vit_b_16") == 0);
    memset(&out, 0, sizeof out);
    EXPECT(vit_resample_check(&b, 384, NULL, &out) == 0 && out.img_size == 384 && vit_config_tokens(&out) == 577 && out.embed_dim == 768);
    EXPECT(vit_resample_check(&b, 384, &how, &out) == 0);
    EXPECT(vit_resample_check(&b, 384, &how, &b) == 0 && b.img_size == 384);   /* aliasing */
    b.img_size = 224;
    const int bad[] = {0, -16, 230, 16 * 513};
    for (unsigned i = 0; i < sizeof bad / sizeof bad[0]; ++i) {
        g_err[0] = 0;
        EXPECT(vit_resample_check(&b, bad[i], &how, &out) == 1 && strncmp(g_err, "vit_resample_check: ", 20) == 0 && strlen(g_err) > 20);
    }
    tiny = b; tiny.patch_size = 4; tiny.img_size = 32;
    g_err[0] = 0;
    EXPECT(vit_resample_check(&tiny, 2052, &how, &out) == 1 && g_err[0]);
    EXPECT(vit_resample_check(&tiny, 2048, &how, &out) == 0);
    how.mode = 2; g_err[0] = 0;
    EXPECT(vit_resample_check(&b, 384, &how, &out) == 1 && g_err[0]);
    how.mode = 1; how.align_corners = 2; g_err[0] = 0;
    EXPECT(vit_resample_check(&b, 384, &how, &out) == 1 && g_err[0]);
    how.align_corners = 1;
    EXPECT(vit_resample_check(&b, 384, &how, &out) == 0);
    g_err[0] = 0;
    EXPECT(vit_resample_check(NULL, 384, &how, &out) == 1 && g_err[0]);
    g_err[0] = 0;
    EXPECT(vit_resample_check(&b, 384, &how, NULL) == 1 && g_err[0]);
    tiny.patch_size = 0; g_err[0] = 0;
    EXPECT(vit_resample_check(&tiny, 32, &how, &out) == 1 && g_err[0]);
    printf("%s (%d failures)\n", fails ? "FAILED" : "ok", fails);
    return fails != 0;
}
