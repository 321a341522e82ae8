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
    """plan_main.c restates the shim's four pure sizing functions; the loaded library's (no device is touched) must agree
    at every shape of the table."""
    L = pkg.lib()
    seen = 0
    for ln in run(plan_main, "stubs").splitlines():
        args, got = ln.split(" : ")
        chans, patch, img, E, F, mb, rows = map(int, args.split())
        want = [L.vh_layer_norm_planes_max_embed(3), L.vh_patch_planes_k(chans, patch), L.vh_patch_embed_workspace(mb, chans, img, patch, E),
                L.vh_mx_act_scale_bytes(rows, E), L.vh_mx_act_scale_bytes(rows, F)]
        assert list(map(int, got.split())) == want, ln
        seen += 1
    assert seen > 500
