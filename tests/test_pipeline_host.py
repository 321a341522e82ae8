"""csrc/vit_pipeline.c without a device: tests/pipeline_main.c runs the host-pointer pipeline over a model of in-order
streams that defers every queued copy, record, wait and forward -- lazily (only what a host synchronisation forces) and
eagerly (as soon as the waits allow) -- and holds what reaches the caller's memory against values computed from the
caller's inputs: every kind of source, one to four chunks, every choice of outputs.  It drops each stream wait and each
event synchronisation in turn to show which a schedule needs, runs the descriptor ring three times round, fails every
allocation of pipeline_make and every forward and copy of a run, and gathers on every thread count.  Compiled with the
unit into one stand-alone program under AddressSanitizer and UBSan, which then runs."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "vit-with-opencl_amd" / "csrc"
FLAGS = ["-O1", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-ffp-contract=off", "-fsanitize=address,undefined",
         "-fno-omit-frame-pointer"]
ENV = {"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}

# the waits the protocol rests on (the table in csrc/vit_pipeline.h)
NEEDED = {"stream_wait(compute, up_done)", "event_sync(out_done), the previous chunk's", "event_sync(out_done), the last chunk's",
          "event_sync(desc_done)"}


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pipeline") / "pipeline_main"
    build = subprocess.run(["gcc", *FLAGS, "-Wall", f"-I{ROOT / 'include'}", f"-I{CSRC}", str(CSRC / "vit_pipeline.c"),
                            str(CSRC / "vit_ingest.c"), str(CSRC / "vit_config.c"), str(ROOT / "tests" / "pipeline_main.c"),
                            "-o", str(exe), "-lm", "-lpthread"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    assert "warning" not in build.stderr, build.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    return r.stdout


def test_every_scenario_is_right_under_both_schedules_and_fails_clean(output):
    assert "pipeline: ok" in output
    # 2 schedules x 4 kinds x 6 counts x 7 choices of outputs; 1 + 2 x 7 + 8 x 3 allocations and creates; 10 job counts
    assert "results: 336 runs right" in output, output
    assert "ring: 24 takes right under both schedules" in output, output
    assert "make: fails clean at each of 39 allocations and creates" in output, output
    assert "run: fails clean in 42 cases" in output, output
    assert "gather: 10 job counts right in both kinds" in output, output


def test_every_wait_earns_its_place(output):
    """A site counts as caught when every one of its calls, dropped alone, gave a wrong result under some schedule."""
    sites = {}
    for ln in output.splitlines():
        if ln.startswith("site | "):
            _, name, dropped, caught, _lazy, _eager, verdict = [f.strip() for f in ln.split(" | ", 6)]
            sites[name] = (int(dropped.split()[1]), int(caught.split()[1]), verdict)
    caught = {name for name, (dropped, n, _) in sites.items() if dropped > 0 and n == dropped}
    assert NEEDED <= caught, output
    # a four-chunk run waits four times for up_done, syncs three times in the loop and once behind it; 24 takes wait 16 times
    assert [sites[s][0] for s in sorted(NEEDED)] == [16, 1, 3, 4], output
    for name in sites.keys() - caught:
        verdict = sites[name][2]
        assert "NO REASON" not in verdict and len(verdict) > 40, f"{name}: dropped without a wrong result, and no reason given"
    # the one wait no schedule needs today is still made
    assert sites["stream_wait(copy, comp_done)"][0] == 2, output
