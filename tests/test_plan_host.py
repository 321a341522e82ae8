"""csrc/vit_plan.c without a device: tests/plan_main.c holds plan_make and plan_layout against every line of
tests/golden/plan_table.txt (recorded from the code before the plan became a unit of its own; DESIGN.md says how to
re-record it) and checks that every borrower of an arena buffer fits it.  Compiled with the unit into one stand-alone
program under AddressSanitizer and UBSan, which then runs."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "vit-with-opencl_amd" / "csrc"
TABLE = ROOT / "tests" / "golden" / "plan_table.txt"
FLAGS = ["-O1", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-ffp-contract=off", "-fsanitize=address,undefined",
         "-fno-omit-frame-pointer"]
ENV = {"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


@pytest.fixture(scope="module")
def plan_main(tmp_path_factory):
    exe = tmp_path_factory.mktemp("plan") / "plan_main"
    build = subprocess.run(["gcc", *FLAGS, "-Wall", f"-I{ROOT / 'include'}", f"-I{CSRC}", str(CSRC / "vit_plan.c"),
                            str(CSRC / "vit_ingest.c"), str(CSRC / "vit_config.c"), str(ROOT / "tests" / "plan_main.c"),
                            "-o", str(exe), "-lm"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    assert "warning" not in build.stderr, build.stderr
    return exe


def run(exe, *args):
    r = subprocess.run([str(exe), str(TABLE), *args], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    return r.stdout


def test_the_plan_reproduces_the_table_and_every_borrower_fits(plan_main):
    out = run(plan_main)
    assert "plan table: ok" in out
    lines = [ln for ln in TABLE.read_text().splitlines() if ln and not ln.startswith("#")]
    assert f"({len(lines)} lines," in out and len(lines) < 2000
    # the only cells that differ from the recording: the two sizing defects, each marked with what the parent had
    edited = [ln for ln in lines if "  # parent: " in ln]
    assert f"{len(edited)} hand-edited" in out
    assert all(ln.split()[:8] in (["64", "4", "5", "10", "256", "1", "4", "128"], ["64", "16", "3", "10", "128", "1", "2", "65536"])
               for ln in edited)


def test_the_programs_sizing_functions_are_the_librarys(plan_main, pkg):
    """plan_main.c prints what the sizing functions of csrc/kernel_limits.h, which the plan calls, return; the loaded
    library's exported entries (no device is touched) must agree at every shape of the table: each still forwards."""
    L = pkg.lib()
    seen = 0
    for ln in run(plan_main, "limits").splitlines():
        args, got = ln.split(" : ")
        chans, patch, img, E, F, mb, rows = map(int, args.split())
        want = [L.vh_layer_norm_planes_max_embed(3), L.vh_patch_planes_k(chans, patch), L.vh_patch_embed_workspace(mb, chans, img, patch, E),
                L.vh_mx_act_scale_bytes(rows, E), L.vh_mx_act_scale_bytes(rows, F)]
        assert list(map(int, got.split())) == want, ln
        seen += 1
    assert seen > 500


def _threshold_rows(N, cus):
    """row counts on and either side of every threshold of the tile rule, for ntiles = N / 256 column tiles"""
    ntiles = max(N // 256, 1)
    targets = {cus - 1, cus, cus + 1, (5 * cus + 1) // 2 - 1, (5 * cus + 1) // 2, (5 * cus + 1) // 2 + 1}
    for full in (2, 3, 4, 10):
        targets |= {full * cus + rem for rem in (0, 1, ntiles - 1, ntiles, 3 * cus // 4 - 1, 3 * cus // 4, 3 * cus // 4 + 1, cus - 1)}
    rows = {1, 127, 128, 129, 255, 256, 257}
    for t in targets:
        for m in {t // ntiles - 1, t // ntiles, t // ntiles + 1, -(-t // ntiles)}:
            if m >= 1:
                rows |= {256 * m - 255, 256 * m - 128, 256 * m - 1, 256 * m, 256 * m + 1}
    return sorted(rows)


def test_the_tile_rule_of_the_planes_and_mx_launchers_is_the_librarys(pkg):
    """vh_gemm_tile_class (no device is touched) against tests/gemm_tiles_ref.py, which states the rule branch by branch for
    every family alike: CU counts 32 .. 304, the widths the models use and 128 / 384 (no 256-wide tile), both families, one
    and three parts, residual or not, `small_only` or not, row counts on and either side of every threshold (tiles = cus - 1,
    cus, cus + 1; 2 tiles around 5 cus; rem = 0; 4 rem around 3 cus; the hand-over row at its ends).  And what the launchers
    rely on: MX and the one-part residual / patch producers never get a 256x256 class -- launch_mx and launch_p3 do not
    instantiate that tile for them."""
    import ctypes

    import gemm_tiles_ref as ref
    L = pkg.lib()
    assert (L.vh_gemm_tile_class(ref.PLANES, 1, 0, 0, 0, 512, 256, None), L.vh_gemm_tile_class(ref.MX, 1, 0, 0, 100, 512, 0, None)) == (-1, -1)
    seen, tails = {c: 0 for c in ref.NAMES}, set()
    for cus in (32, 64, 256, 304):
        for N in (128, 256, 384, 512, 768, 2304, 3072):
            for rows in _threshold_rows(N, cus):
                for family, parts in ((ref.PLANES, 1), (ref.PLANES, 3), (ref.MX, 1)):
                    for resid in (0, 1):
                        for small_only in (0, 1):
                            want = ref.tile_class(family, parts, resid, small_only, rows, N, cus)
                            rb = ctypes.c_int(-7)
                            got = L.vh_gemm_tile_class(family, parts, resid, small_only, rows, N, cus, ctypes.byref(rb))
                            where = f"family {family} parts {parts} resid {resid} small_only {small_only} rows {rows} N {N} cus {cus}"
                            assert (got, rb.value) == want, where
                            assert L.vh_gemm_tile_class(family, parts, resid, small_only, rows, N, cus, None) == got, where
                            if family == ref.MX or (parts == 1 and resid):
                                assert got in (ref.T128x256, ref.T128x128), where
                            else:
                                assert got != ref.T128x256, where
                            if got == ref.T256x256_TAIL:
                                assert 0 < rb.value < rows and rb.value % 256 == 0, where
                                tails.add((cus, N))
                            seen[got] += 1
    assert all(n > 1000 for n in seen.values()), seen
    assert len(tails) >= 12, tails                            # the split occurs at every CU count and most widths
