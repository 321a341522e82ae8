"""csrc/vit_requests.c without a device: tests/requests_main.c arms each of the six armed outputs in both forms over an
allocator that counts its live blocks and fails on demand -- every allocation of every arming failing in turn, over an unarmed
and an armed context -- and checks the scratch rules, what a forward serves, the refusal of a request armed in the other
form, the list of staged arrays, the last-layer predicate and the release of everything.  Compiled with the unit into one
stand-alone program under AddressSanitizer and UBSan, which then runs."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "vit-with-opencl_amd" / "csrc"
FLAGS = ["-O1", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-ffp-contract=off", "-fsanitize=address,undefined",
         "-fno-omit-frame-pointer"]
ENV = {"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


@pytest.fixture(scope="module")
def requests_main(tmp_path_factory):
    exe = tmp_path_factory.mktemp("requests") / "requests_main"
    build = subprocess.run(["gcc", *FLAGS, "-Wall", f"-I{ROOT / 'include'}", f"-I{CSRC}", str(CSRC / "vit_requests.c"),
                            str(CSRC / "vit_ingest.c"), str(CSRC / "vit_config.c"), str(ROOT / "tests" / "requests_main.c"),
                            "-o", str(exe), "-lm"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    assert "warning" not in build.stderr, build.stderr
    return exe


def run(exe, *args):
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    return r.stdout


def test_arming_fails_clean_at_every_allocation_and_serves_what_is_armed(requests_main):
    out = run(requests_main)
    assert "requests: ok" in out
    # 6 requests x 2 forms x 3 starts, each armed at least three times and every host form allocating: the loops ran
    assert int(out.split("(")[1].split()[0]) > 6 * 3 * 3 * 3, out


def test_the_programs_sizing_functions_are_the_librarys(requests_main, pkg):
    """requests_main.c prints what the sizing functions of csrc/kernel_limits.h, which the unit calls, return; the loaded
    library's exported entries (no device is touched) must agree at the shapes the program arms at and around the
    functions' thresholds: each still forwards."""
    L = pkg.lib()
    seen = set()
    for ln in run(requests_main, "limits").splitlines():
        args, got = ln.split(" : ")
        kind, *args = args.split()
        args, got = list(map(int, args)), list(map(int, got.split()))
        if kind == "head_dim":
            want = [L.vh_cls_attention_head_dim_ok(args[0]), L.vh_rollout_max_tokens(args[0])]
        elif kind == "rollout":
            want = [L.vh_rollout_workspace(*args)]
        else:
            want = [L.vh_gallery_workspace(1, args[0], args[1], 0), L.vh_gallery_workspace(3, args[0], args[1], 7)]
        assert got == want, ln
        seen.add((kind, *args))
    # the program's own shapes: head_dim 16, max_batch 4 x 17 tokens, 1000 gallery rows at k = 2 and 4
    assert {("head_dim", 16), ("rollout", 4, 17), ("gallery", 1000, 2), ("gallery", 1000, 4)} <= seen and len(seen) > 40
