"""csrc/vit_ingest.c without a device: tests/ingest_plan_main.c plans and packs chunks of the resized and the box host forms
in host memory and checks them against a naive restatement of the rules.  Both are compiled into one stand-alone program
under AddressSanitizer and UBSan, which then runs: the planner's row bitmaps, ranks and offsets have no other test that
does not go through a GPU forward."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "vit-with-opencl_amd" / "csrc"
FLAGS = ["-O1", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-ffp-contract=off", "-fsanitize=address,undefined",
         "-fno-omit-frame-pointer"]


def test_chunks_are_planned_and_packed_as_the_naive_rule_says(tmp_path):
    exe = tmp_path / "ingest_plan"
    build = subprocess.run(["gcc", *FLAGS, "-Wall", f"-I{ROOT / 'include'}", f"-I{CSRC}", str(CSRC / "vit_ingest.c"),
                            str(ROOT / "tests" / "ingest_plan_main.c"), "-o", str(exe), "-lm"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    assert "warning" not in build.stderr, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                         env={"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ingest plan: ok" in run.stdout
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
