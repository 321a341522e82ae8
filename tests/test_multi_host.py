"""csrc/vit_multi.c without a device: tests/multi_main.c holds the shard ranges, the shard runner and the replicas' create /
forward / destroy over counting stand-ins for the context's entries.  Compiled with the unit into one stand-alone program,
which then runs: once under AddressSanitizer and UBSan (LeakSanitizer on), once under ThreadSanitizer.  The ctypes tests of
the shard functions in tests/test_host.py stay: they run the library's copy."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "vit-with-opencl_amd" / "csrc"
FLAGS = ["-O1", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-ffp-contract=off", "-fno-omit-frame-pointer"]
ENV = {"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1", "TSAN_OPTIONS": "halt_on_error=1"}


@pytest.mark.parametrize("sanitizer", ["address,undefined", "thread"])
def test_shards_and_replicas_hold_under(tmp_path, sanitizer):
    exe = tmp_path / "multi_main"
    build = subprocess.run(["gcc", *FLAGS, f"-fsanitize={sanitizer}", "-Wall", f"-I{ROOT / 'include'}", f"-I{CSRC}", str(CSRC / "vit_multi.c"),
                            str(ROOT / "tests" / "multi_main.c"), "-o", str(exe), "-lpthread"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    assert "warning" not in build.stderr, build.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    out = r.stdout
    assert "multi: ok" in out
    assert "ranges: contiguous, disjoint, covering, empty shards last for 0..130 images over 1..64 shards" in out, out
    assert "runner: refusals, the lowest failing shard's status with every other shard still run" in out, out
    assert "creation failed clean at each device index of 1, 2, 3 and 8 devices (14 creations)" in out, out
