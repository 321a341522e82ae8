"""csrc/vit_planes_file.c without a device: tests/planes_file_main.c writes and reads planes files over host copies of the
six vh_* the unit calls -- round trips in every precision; every header byte of every file, and every scale byte of the
seven small ones (the first and last scale byte of the others), mutated four ways; every truncation; every copy and
allocation failed in turn; writes cut short by a file size limit.  Compiled with the unit into one stand-alone
program under AddressSanitizer and UBSan (LeakSanitizer on), which then runs.  This side states the format on its own: it
rebuilds every file the program wrote from the same PRNG seeds with `struct` and its own FNV-1a, and requires byte equality."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "vit-with-opencl_amd" / "csrc"
FLAGS = ["-O1", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-ffp-contract=off", "-fsanitize=address,undefined",
         "-fno-omit-frame-pointer", "-DPLANES_CHUNK_BYTES=(1<<20)"]
ENV = {"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
HEADER = "<8sIii8i4xd4QQiiQ"
# header bytes neither the size check nor the checksum protects, from the code: num_heads, the padding, eps, and ln_fold
# where a non-zero value becomes another non-zero value
UNPROTECTED = set(range(44, 48)) | set(range(52, 56)) | set(range(56, 64)) | set(range(104, 108))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    work = tmp_path_factory.mktemp("planes_file")
    exe = work / "planes_file_main"
    build = subprocess.run(["gcc", *FLAGS, "-Wall", f"-I{ROOT / 'include'}", f"-I{CSRC}", str(CSRC / "vit_planes_file.c"),
                            str(CSRC / "vit_plan.c"), str(CSRC / "vit_ingest.c"), str(CSRC / "vit_config.c"),
                            str(ROOT / "tests" / "planes_file_main.c"), "-o", str(exe), "-lm"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    assert "warning" not in build.stderr, build.stderr
    files = work / "files"
    files.mkdir()
    r = subprocess.run([str(exe), str(files)], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    return r.stdout, files


def test_every_part_of_the_program_held(run):
    out, files = run
    assert "planes file: ok" in out
    assert "round trip: 17 cases right" in out, out
    assert "truncation: " in out and "failing copies: " in out and "failing writes: 5 size limits gave 120" in out, out
    assert sorted(p.name for p in files.iterdir()) == sorted(f"case_{i}.planes" for i in range(17))   # no temporary, no scratch file


def _mix(z):
    z = z * np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _words(seed, n):
    return _mix(np.uint64(seed) + np.arange(1, n + 1, dtype=np.uint64))


def _fnv1a_words(h, blob):
    """FNV-1a over little-endian 64-bit words, a tail byte-wise"""
    mask = (1 << 64) - 1
    for w in np.frombuffer(blob[:len(blob) // 8 * 8], dtype="<u8").tolist():
        h = ((h ^ w) * 0x100000001b3) & mask
    for b in blob[len(blob) // 8 * 8:]:
        h = ((h ^ b) * 0x100000001b3) & mask
    return h


def test_the_files_are_the_format_as_stated_here(run):
    out, _ = run
    cases = [ln.split(" | ") for ln in out.splitlines() if ln.startswith("case | ")]
    assert len(cases) == 17
    seen = set()
    for _, index, path, shape, mode, sizes in cases:
        i = int(index)
        ints = tuple(map(int, shape.split()))
        precision, fold, n_tensors = map(int, mode.split())
        slab_bytes = tuple(map(int, sizes.split()))
        scales = ((_words(16 * i, n_tensors) >> np.uint64(40)).astype(np.float32) / np.float32(1 << 20)).astype("<f4").tobytes()
        slabs = [_words(16 * i + j + 1, (n + 7) // 8).astype("<u8").tobytes()[:n] for j, n in enumerate(slab_bytes)]
        h = _fnv1a_words(0xcbf29ce484222325, scales)
        for s in slabs:
            assert len(s) % 8 == 0          # so hashing slab by slab is hashing the payload
            h = _fnv1a_words(h, s)
        header = struct.pack(HEADER, b"VITPLN02", 120, precision, n_tensors, *ints, 1e-6, slab_bytes[0], slab_bytes[1], slab_bytes[2],
                             n_tensors, slab_bytes[3], fold, 2, h)
        assert len(header) == 120
        assert Path(path).read_bytes() == header + scales + b"".join(slabs), f"case {i}"
        seen.add((ints[1], precision, fold))
    # the tiny shape in all four precisions, folded wherever the plan allows it, and the shape with padded conv_proj planes
    assert {(16, p, f) for p in (0, 1, 2) for f in (0, 1)} | {(16, 3, 0)} <= seen and any(s[0] == 14 for s in seen)


def test_a_mutated_byte_loads_only_where_nothing_protects_it(run):
    """The measured table of DESIGN.md 10: a loading offset outside UNPROTECTED is a finding; one inside it that in fact
    refuses under these four mutations is simply recorded there."""
    out, _ = run
    lines = [ln.split(" | ") for ln in out.splitlines() if ln.startswith("sweep | ")]
    assert len(lines) == 17                                   # every case; the seven small ones with every scale byte
    assert sum("every scale byte" in ln[3] for ln in lines) == 7
    for _, index, mode, _n, loads in lines:
        at = set(map(int, loads.replace("loads at", "").split()))
        assert at <= UNPROTECTED, f"case {index}: a mutation of byte(s) {sorted(at - UNPROTECTED)} loads"
        if mode.endswith("fold 0"):                           # zero -> non-zero never loads
            assert not at & set(range(104, 108))
        print(f"case {index} ({mode}): some mutation loads at {sorted(at)}; in the set but refused: {sorted(UNPROTECTED - at)}")
    # what a mutated ln_fold runs into: an unfolded file of a precision that can fold asks for other slab sizes (125); the
    # fp16-pair emulation, which never folds, is refused with its shape (2)
    flags = [ln.split(" | ") for ln in out.splitlines() if ln.startswith("ln_fold | ")]
    assert len(flags) == 17
    for _, index, mode, seen in flags:
        want = {"precision 3 fold 0": "a mutated flag: 2"}.get(mode, "a mutated flag: 125" if mode.endswith("fold 0") else "a mutated flag: loads 125")
        assert seen == want, f"case {index} ({mode}): {seen}"
    # recorded, not required: num_heads halved and doubled (head counts the shapes allow) is in UNPROTECTED either way
    print("\n".join(ln for ln in out.splitlines() if ln.startswith("heads | ")))
    assert "mutated files" in out
