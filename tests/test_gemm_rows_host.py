"""The fp32-rows GEMM family (csrc/gemm_mfma.hip), the part that needs no GPU: the library's tile rule
(vh_gemm_rows_tile_class) against its branch-by-branch restatement in tests/gemm_tiles_ref.py, and the sharper error bound of
tests/test_gpu_gemm_rows_classes.py held against a numpy emulation of the kernel's six-product sum -- the emulation must pass
it, and the same sum with any one third-order product left out must fail it (tests/gemm_rows_ref.py states the bound)."""
import ctypes

import numpy as np
import pytest

import gemm_rows_ref as rr
import gemm_tiles_ref as ref

CUS = (8, 64, 256, 304)
WIDTHS = (72, 128, 384, 512, 1000, 3072)


def _edge_rows(N, cus):
    """row counts on and either side of every threshold of the rule at this width: 4096 rows; 2 * tiles128 = cus (ragged N);
    tiles of 256x256 = full * cus + rem with rem = 0 and 4 rem around 3 cus, and the hand-over row at both its ends"""
    rows = {1, 127, 128, 129, 4095, 4096, 4097}
    nt128 = (N + 127) // 128
    for mt in {cus // (2 * nt128), -(-cus // (2 * nt128))}:
        for m in (mt - 1, mt, mt + 1):
            if m >= 1:
                rows |= {128 * m - 1, 128 * m, 128 * m + 1}
    ntiles = max(N // 256, 1)
    for full in (0, 1, 2, 3, 10):
        for rem in (0, 1, ntiles - 1, ntiles, 3 * cus // 4 - 1, 3 * cus // 4, 3 * cus // 4 + 1, cus - 1):
            t = full * cus + rem
            for m in {t // ntiles - 1, t // ntiles, t // ntiles + 1, -(-t // ntiles)}:
                if m >= 1:
                    rows |= {256 * m - 255, 256 * m - 128, 256 * m - 1, 256 * m, 256 * m + 1}
    return sorted(rows)


def test_the_tile_rule_of_the_rows_launchers_is_the_librarys(pkg):
    """no device is touched.  Every family, epilogue, arithmetic and alignment; CU counts 8 .. 304; widths with no 128-wide
    tile (72, 1000), no 256-wide one (128, 384) and both (512, 3072); K on both sides of 2048; the rows of _edge_rows."""
    L = pkg.lib()
    seen, tails = {c: 0 for c in ref.ROWS_NAMES}, set()
    refused = 0
    for cus in CUS:
        for N in WIDTHS:
            for rows in _edge_rows(N, cus):
                for K in (96, 2048):
                    for family in (ref.INLOOP, ref.W3, ref.H2):
                        for epi in (ref.EPI_NONE, ref.EPI_GELU, ref.EPI_RESID, ref.EPI_PATCH):
                            for math in (ref.SPLIT3, ref.NATIVE):
                                for aligned in (0, 1):
                                    want = ref.rows_tile_class(family, epi, math, aligned, rows, K, N, cus)
                                    rb = ctypes.c_int(-7)
                                    got = L.vh_gemm_rows_tile_class(family, epi, math, aligned, rows, K, N, cus, ctypes.byref(rb))
                                    where = f"family {family} epi {epi} math {math} aligned {aligned} rows {rows} K {K} N {N} cus {cus}"
                                    assert (got, rb.value) == want, where
                                    assert L.vh_gemm_rows_tile_class(family, epi, math, aligned, rows, K, N, cus, None) == got, where
                                    if got < 0:
                                        refused += 1
                                        continue
                                    seen[got] += 1
                                    assert (rb.value != 0) == (got == ref.R256_PLANES_TAIL), where
                                    if got == ref.R256_PLANES_TAIL:
                                        assert 0 < rb.value < rows and rb.value % 256 == 0 and rows >= 4096, where
                                        tails.add((cus, N))
                                    # what the kernels rely on
                                    if got in (ref.R32x64_NATIVE_GUARDED, ref.R128_NATIVE_GUARDED):
                                        assert N % 128 != 0 and family == ref.INLOOP, where
                                    else:
                                        assert N % 128 == 0, where               # unguarded tiles read whole 128-column tiles
                                    if got in (ref.R256_NATIVE, ref.R256_SPLIT, ref.R256_PLANES, ref.R256_PLANES_TAIL):
                                        assert N % 256 == 0 and rows >= 4096 and not (epi == ref.EPI_RESID and K < 2048), where
                                    if got in (ref.R128_SPLIT, ref.R256_SPLIT):
                                        assert aligned and math == ref.SPLIT3, where   # 16-byte epilogue accesses
    assert all(n > 200 for n in seen.values()), seen
    assert refused > 1000 and len(tails) >= 6, (refused, tails)


def test_the_rule_refuses_what_the_launchers_refuse(pkg):
    L = pkg.lib()
    ok = (ref.INLOOP, ref.EPI_NONE, ref.SPLIT3, 1, 300, 96, 512, 256)
    assert L.vh_gemm_rows_tile_class(*ok, None) == ref.R128_SPLIT
    for pos in (4, 5, 6, 7):                                   # rows, K, N, CUs
        for bad in (0, -1):
            rb = ctypes.c_int(-7)
            args = list(ok)
            args[pos] = bad
            assert L.vh_gemm_rows_tile_class(*args, ctypes.byref(rb)) == -1 and rb.value == 0, (pos, bad)
    assert L.vh_gemm_rows_tile_class(3, *ok[1:], None) == -1 and L.vh_gemm_rows_tile_class(ok[0], 4, *ok[2:], None) == -1
    assert L.vh_gemm_rows_tile_class(ref.INLOOP, ref.EPI_NONE, 2, 1, 300, 96, 512, 256, None) == -1     # unknown fp32_math
    for family in (ref.W3, ref.H2):
        assert L.vh_gemm_rows_tile_class(family, ref.EPI_NONE, 0, 1, 300, 96, 1000, 256, None) == -1    # N % 128 != 0
        assert L.vh_gemm_rows_tile_class(family, ref.EPI_NONE, 0, 0, 300, 96, 512, 256, None) == -1     # a misaligned pointer
        assert L.vh_gemm_rows_tile_class(family, ref.EPI_PATCH, 0, 1, 300, 96, 512, 256, None) == -1


A, B, C3, D4 = 0x10000, 0x20000, 0x30000, 0x40000      # 16-byte aligned stand-ins for device pointers: a refusal reads none


def test_the_launchers_refuse_before_any_device_call(pkg):
    L = pkg.lib()

    def refused(rc, *words):
        msg = L.vh_last_error().decode()
        assert rc == 1 and all(w in msg for w in words), msg

    for name, head in (("vh_launch_linear_w3", (None, A, B)), ("vh_launch_linear_h2", (None, A, B, ctypes.c_float(1024.0)))):
        fn = getattr(L, name)
        L.vh_set_error(1, b"stale")
        refused(fn(*head[:1], A + 4, *head[2:], C3, D4, 300, 96, 512, 0, None), name, "16-byte aligned")        # the output
        refused(fn(*head, C3, D4 + 4, 300, 96, 512, 0, None), name, "16-byte aligned")                           # the bias
        refused(fn(*head, C3, D4, 300, 96, 512, 0, A + 8), name, "16-byte aligned")                              # the residual
        refused(fn(*head, C3, D4, 300, 96, 1000, 0, None), name, "colB=1000", "multiple of 128")
        refused(fn(*head, C3, D4, 300, 96, 576, 0, None), name, "colB=576", "multiple of 128")
    L.vh_set_error(1, b"stale")
    refused(L.vh_launch_linear_math(None, A, B, C3, D4, 300, 96, 512, 0, None, 2), "unknown fp32_math 2")
    refused(L.vh_launch_linear_math(None, A, B, C3, D4, 300, 96, 512, 0, None, -1), "unknown fp32_math -1")


@pytest.fixture(scope="module")
def sharp(oracle):
    """case-1 inputs at K = 96 on 1536 rows, their float64 statement and the fp32 loop's error"""
    x, w, b = rr.inputs(oracle, 1536, 96)
    want = rr.want64(x, w, b, "NONE")
    e_ref = float(np.abs(rr.loop32(oracle, x, w, b, "NONE") - want).max())
    return x, w, b, want, e_ref


def test_the_six_products_in_the_kernels_order_pass_the_sharper_bound(sharp):
    x, w, b, want, e_ref = sharp
    err = float(np.abs(rr.six_products(x, w, b) - want).max())
    print(f"\nGEMM-ROWS-BOUND K=96 loop={e_ref:.3e} six-products={err:.3e} ratio={err / e_ref:.2f}")
    assert 0.0 < e_ref < 2e-6 and err <= rr.SHARP * e_ref, (err, e_ref)
    assert err <= e_ref, "the exact split is no worse than the sequential loop on these inputs"


@pytest.mark.parametrize("drop", rr.THIRD_ORDER)
def test_a_sum_that_loses_one_third_order_product_fails_the_sharper_bound(sharp, drop):
    x, w, b, want, e_ref = sharp
    err = float(np.abs(rr.six_products(x, w, b, drop=drop) - want).max())
    print(f"\nGEMM-ROWS-BOUND K=96 dropped w{drop[0]}.a{drop[1]}: err={err:.3e} ratio={err / e_ref:.2f}")
    assert err > rr.SHARP * e_ref, (drop, err, e_ref)
    assert err > 3.0 * e_ref, "not even the widest factor the GPU test may take lets the defect through"
    assert err < 2e-5, "and the project's operator bound alone does not see it"
