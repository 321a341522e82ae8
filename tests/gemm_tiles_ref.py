"""Python statement of the tile rule of the planes and MX projection launchers (launch_p3 in csrc/gemm_p3.hip, launch_mx in
csrc/gemm_mx.hip; the library's own statement is vh_gemm_tile_class, include/kernelHandler.h).  Written as the launchers
first stated it, branch by branch, for every family alike: that the families which take the 128x256 tile never reach the
256x256 branches is a CONSEQUENCE the host test draws from it (tests/test_plan_host.py), not something assumed here."""

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
