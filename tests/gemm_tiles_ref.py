"""Python statement of the tile rule of the planes and MX projection launchers (launch_p3 in csrc/gemm_p3.hip, launch_mx in
csrc/gemm_mx.hip; the library's own statement is vh_gemm_tile_class, include/kernelHandler.h).  Written as the launchers
first stated it, branch by branch, for every family alike: that the families which take the 128x256 tile never reach the
256x256 branches is a CONSEQUENCE the host test draws from it (tests/test_plan_host.py), not something assumed here.
Below it, in the same manner, the rule of the launchers on fp32 activation rows (csrc/gemm_mfma.hip; the library's statement
is vh_gemm_rows_tile_class, swept against this one in tests/test_gemm_rows_host.py)."""

PLANES, MX = 0, 1                                        # VH_GEMM_PLANES, VH_GEMM_MX
T128x256, T128x128, T256x256, T256x256_TAIL = 0, 1, 2, 3   # VH_TILES_*
NAMES = {T128x256: "128x256", T128x128: "128x128", T256x256: "256x256", T256x256_TAIL: "256x256+128x128 tail"}


def tile_class(family, parts, resid_or_patch, small_only, rows, N, cus):
    """-> (class, rows_big): rows_big = the row where the 256x256 launch hands over to the 128x128 launch (0: one launch).
    `tiles` counts 256x256 tiles whatever class runs."""
    ntiles, mtiles = N // 256, (rows + 255) // 256
    tiles = mtiles * ntiles
    if (family == MX or (parts == 1 and resid_or_patch)) and N % 256 == 0 and tiles >= cus:
        return T128x256, 0
    if N % 256 != 0 or small_only or 2 * tiles < 5 * cus:
        return T128x128, 0
    full, rem = tiles // cus, tiles % cus
    rows_big = (full * cus // ntiles) * 256
    if rem == 0 or 4 * rem > 3 * cus or rows_big <= 0 or rows_big >= rows:
        return T256x256, 0
    return T256x256_TAIL, rows_big


def linear_small_only(resid, K):
    """the flag vh_launch_linear_planes / vh_launch_linear_mx pass: the N = K = E output projection"""
    return bool(resid) and K < 2048


def rows_big(family, parts, resid, M, K, N, cus):
    """hand-over row of vh_launch_linear_planes(parts) / vh_launch_linear_p3 / vh_launch_linear_mx at this shape (0: one launch)"""
    return tile_class(family, parts, resid, linear_small_only(resid, K), M, N, cus)[1]


# ---- the GEMMs on fp32 activation rows (csrc/gemm_mfma.hip; the library's statement is vh_gemm_rows_tile_class) -------------

INLOOP, W3, H2 = 0, 1, 2                                  # VH_ROWS_*: vh_launch_linear(_math) / patch embedding on rows, _w3, _h2
EPI_NONE, EPI_GELU, EPI_RESID, EPI_PATCH = 0, 1, 2, 3     # VH_EPI_*
SPLIT3, NATIVE = 0, 1                                     # VH_FP32_*
(R32x64_NATIVE_GUARDED, R128_NATIVE_GUARDED, R128_NATIVE, R256_NATIVE, R128_SPLIT, R256_SPLIT, R128_PLANES, R256_PLANES,
 R256_PLANES_TAIL) = range(9)                             # VH_ROWS_<tile>_<kernel>
ROWS_NAMES = {R32x64_NATIVE_GUARDED: "32x64 native guarded", R128_NATIVE_GUARDED: "128x128 native guarded",
              R128_NATIVE: "128x128 native", R256_NATIVE: "256x256 native", R128_SPLIT: "128x128 split",
              R256_SPLIT: "256x256 split", R128_PLANES: "128x128 planes", R256_PLANES: "256x256 planes",
              R256_PLANES_TAIL: "256x256 planes + 128x128 tail"}


def rows_tile_class(family, epi, fp32_math, aligned, rows, K, N, cus):
    """-> (class, rows_big) as the three launchers of csrc/gemm_mfma.hip first stated it, each in its own words: `launch`
    (both operands split in the K loop, or native), `launch_planes` behind `launch_planes_epi` (weights pre-split).  -1: the
    launcher refuses before it decides."""
    if min(rows, K, N, cus) <= 0 or family not in (INLOOP, W3, H2) or epi not in (EPI_NONE, EPI_GELU, EPI_RESID, EPI_PATCH):
        return -1, 0
    if family == INLOOP:
        if fp32_math not in (SPLIT3, NATIVE):
            return -1, 0
        big = N % 256 == 0 and rows >= 4096 and not (epi == EPI_RESID and K < 2048)
        if N % 128 != 0:                                  # ragged N: the guarded tiles on the native instruction
            tiles128 = ((rows + 127) // 128) * ((N + 127) // 128)
            return (R32x64_NATIVE_GUARDED if 2 * tiles128 < cus else R128_NATIVE_GUARDED), 0
        if fp32_math == SPLIT3 and aligned:
            return (R256_SPLIT if big else R128_SPLIT), 0
        return (R256_NATIVE if big else R128_NATIVE), 0
    # linear_params(planes = true): whole 128-column tiles, aligned pointers; no patch embedding on planes here
    if epi == EPI_PATCH or N % 128 != 0 or not aligned:
        return -1, 0
    prefer_small = epi == EPI_RESID and K < 2048          # the N = 768, K = 768 out-projection
    if not (N % 256 == 0 and rows >= 4096 and not prefer_small):
        return R128_PLANES, 0
    ntiles, mtiles = N // 256, (rows + 255) // 256
    tiles = mtiles * ntiles
    full, rem = tiles // cus, tiles % cus
    rows_big = (full * cus // ntiles) * 256
    if full < 1 or rem == 0 or 4 * rem > 3 * cus or rows_big <= 0 or rows_big >= rows:
        return R256_PLANES, 0
    return R256_PLANES_TAIL, rows_big
