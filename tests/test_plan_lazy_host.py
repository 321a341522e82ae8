"""The lazy last layer in csrc/vit_plan.c, without a device: tests/plan_lazy_main.c runs every case of
tests/golden/plan_table.txt through plan_make with $VIT_HIP_LAST_LAYER as recorded, unset, "full" and "all_queries".  Compiled
with the unit into one stand-alone program under AddressSanitizer and UBSan, which then runs."""
import re
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
def summary(tmp_path_factory):
    exe = tmp_path_factory.mktemp("plan_lazy") / "plan_lazy_main"
    build = subprocess.run(["gcc", *FLAGS, "-Wall", f"-I{ROOT / 'include'}", f"-I{CSRC}", str(CSRC / "vit_plan.c"),
                            str(CSRC / "vit_ingest.c"), str(CSRC / "vit_config.c"), str(ROOT / "tests" / "plan_lazy_main.c"),
                            "-o", str(exe), "-lm"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    assert "warning" not in build.stderr, build.stderr
    r = subprocess.run([str(exe), str(TABLE)], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    return r.stdout


def test_lazy_by_default_where_the_class_rows_path_may_run_and_full_clears_it(summary):
    """Every check is in the program; here: it saw every plan of the table, and cases of each kind exist -- plans that are
    lazy, lazy plans that also take the class query, and lazy plans that do not (another attention form)."""
    m = re.search(r"lazy last layer: ok \((\d+) plans, (\d+) lazy, (\d+) with the class query, (\d+) lazy without it\)", summary)
    assert m, summary
    plans, lazy, query, lazy_only = map(int, m.groups())
    recorded = [ln for ln in TABLE.read_text().splitlines() if " => 0 " in ln and not ln.startswith("#")]
    assert plans == len(recorded) > 500
    assert lazy == sum(" clsok=1 " in ln for ln in recorded) > 20
    assert query > 10 and lazy_only > 0 and query + lazy_only == lazy
