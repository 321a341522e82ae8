"""Host side of the top-k feature (no GPU): the spec check, the ctypes mirrors of the header's structs, the result file
written from top-k columns, and the NumPy reference itself against a brute-force ranking."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import topk_ref as tr

ROOT = Path(__file__).resolve().parent.parent


def test_topk_check_refusals(pkg):
    b, L = pkg.binding, pkg.lib()
    cfg = pkg.preset("vit_b_16")

    def rc(k, kind=0, cfg_=cfg):
        spec = b.TopKSpecC(k, kind)
        return L.vit_topk_check(C.byref(cfg_), C.byref(spec))

    assert rc(1) == 0 and rc(5, 1) == 0 and rc(32) == 0
    small = pkg.preset("vit_b_16")
    small.num_classes = 3
    for bad in (lambda: rc(0), lambda: rc(33), lambda: rc(4, 0, small), lambda: rc(5, 2), lambda: rc(5, -1),
                lambda: L.vit_topk_check(None, C.byref(b.TopKSpecC(5, 0))), lambda: L.vit_topk_check(C.byref(cfg), None)):
        L.vh_set_error(1, b"stale")
        assert bad() == 1
        msg = L.vh_last_error().decode()
        assert msg.startswith("vit_topk_check: ") and len(msg) > len("vit_topk_check: ")
    assert rc(3, 0, small) == 0
    wide = pkg.preset("vit_b_16")
    wide.num_classes = 21843
    assert rc(32, 0, wide) == 0
    wide.num_classes = 65537          # beyond what one workgroup per row takes
    assert rc(5, 0, wide) == 1
    # arming without a context is refused on the host, before any device call
    assert L.vit_hip_set_topk(None, None, None) == 1 and L.vit_hip_set_topk_host(None, None, None) == 1
    assert "NULL context" in L.vh_last_error().decode()


def test_ctypes_structs_match_the_header(pkg, tmp_path):
    b = pkg.binding
    probe = tmp_path / "topk_layout.c"
    probe.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "ViT_opencl.h"
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %d %d\n", sizeof(vit_topk_spec), offsetof(vit_topk_spec, k), offsetof(vit_topk_spec, score_kind),
           sizeof(vit_topk_buffers), offsetof(vit_topk_buffers, labels), offsetof(vit_topk_buffers, scores),
           (int)VIT_TOPK_PROBS, (int)VIT_TOPK_LOGITS);
    return 0;
}
''')
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), "-o", str(tmp_path / "topk_layout"), str(probe)], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "topk_layout")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(b.TopKSpecC), b.TopKSpecC.k.offset, b.TopKSpecC.score_kind.offset,
                   C.sizeof(b.TopKBuffers), b.TopKBuffers.labels.offset, b.TopKBuffers.scores.offset,
                   b.TOPK_SCORES["probs"], b.TOPK_SCORES["logits"]]
    assert got[0] == 8 and got[3] == 16


def test_result_file_from_topk_columns_is_byte_equal(pkg, tmp_path):
    b, L = pkg.binding, pkg.lib()
    n, nc, k = 7, 1000, 5
    rng = np.random.default_rng(5)
    rows = tr.softmax64(rng.uniform(-4, 4, size=(n, nc)).astype(np.float32)).astype(np.float32)
    rows[2, 700] = rows[2, 31] = rows[2].max() * 2        # an exact tie for first place: the lowest index wins in both
    rows[4, 999] = rows[4, 0] = rows[4].max() * 2
    labels = tr.topk(rows, k)
    assert labels[2, 0] == 31 and labels[2, 1] == 700 and labels[4, 0] == 0
    scores = np.take_along_axis(rows, labels, axis=1)
    full, cols = tmp_path / "full.txt", tmp_path / "topk.txt"
    ptrs = (b.f32p * n)(*[b.fptr(rows[i]) for i in range(n)])
    assert L.vit_write_result_file(str(full).encode(), ptrs, n, nc) == 0
    assert L.vit_write_result_file_topk(str(cols).encode(), labels.ctypes.data_as(C.POINTER(C.c_int)), b.fptr(scores), n, k) == 0
    assert full.read_bytes() == cols.read_bytes() and full.read_text().count("\n") == n
    assert full.read_text().splitlines()[2].startswith("[2] label: 31 / prob: ")
    assert L.vit_write_result_file_topk(None, labels.ctypes.data_as(C.POINTER(C.c_int)), b.fptr(scores), n, k) == 1
    assert L.vit_write_result_file_topk(str(cols).encode(), labels.ctypes.data_as(C.POINTER(C.c_int)), None, n, k) == 1
    assert L.vit_write_result_file_topk(str(cols).encode(), labels.ctypes.data_as(C.POINTER(C.c_int)), b.fptr(scores), n, 0) == 1


def test_reference_agrees_with_brute_force():
    inf, nan = np.inf, np.nan
    crafted = [
        [1.0, 3.0, 3.0, -2.0, 3.0, 0.5],                       # a three-way tie for first place
        [0.0, -0.0, -0.0, 0.0, -1.0, 1e-45],                   # signed zeros are equal; a denormal beats them
        [-inf, nan, inf, -inf, nan, 0.0, inf],                 # NaN below -inf, by ascending index
        [nan, nan, nan],
        [-1.0, -1.0, -1.0, -1.0],
        [5.0],
    ]
    for row in crafted:
        for k in range(1, len(row) + 1):
            assert np.array_equal(tr.topk(np.array([row], np.float32), k)[0], tr.topk_brute(row, k)), (row, k)
    assert list(tr.topk(np.array([crafted[2]], np.float32), 7)[0]) == [2, 6, 5, 0, 3, 1, 4]
    assert list(tr.topk(np.array([crafted[1]], np.float32), 6)[0]) == [5, 0, 1, 2, 3, 4]
    rng = np.random.default_rng(0)
    for _ in range(5):
        row = rng.integers(-3, 4, size=40).astype(np.float32)   # many ties
        assert np.array_equal(tr.topk(row[None], 32)[0], tr.topk_brute(row, 32))
    labels = tr.topk(rng.standard_normal((3, 100)).astype(np.float32), 32)
    assert all(len(set(r)) == 32 for r in labels.tolist())


def test_long_row_summation_order_stays_within_the_stated_bound(pkg):
    """The bound tests/test_gpu_topk.py holds long rows to, (ceil(length / 256) + 32) * 2^-24 relative to the float64
    softmax, checked here on a plain fp32 NumPy emulation of the kernel's summation order for the same inputs."""
    for length in (2049, 4097, 21843, 65536):
        row = np.empty(length, np.float32)
        pkg.lib().vit_synth_fill(pkg.binding.fptr(row), length, 77 + length, 4.0, 0.0)
        got, want = tr.softmax_f32_strided(row).astype(np.float64), tr.softmax64(row)[0]
        rel = float(np.abs(got / want - 1.0).max())
        bound = (-(-length // 256) + 32) * 2.0 ** -24
        print(f"length {length}: emulated fp32 worst relative error {rel:.3e}, bound {bound:.3e}")
        assert rel <= bound
