"""The host side of the dense stitch without a device: csrc/vit_stitch.c (vit_stitch_check, vit_stitch_index) through
tests/stitch_index_main.c, one stand-alone program under AddressSanitizer and UBSan, against tests/stitch_ref.py's per-pixel
statement of the index; and that reference itself against tests/dense_ref.py (one whole-frame window is the dense head) and
against its own float64 definition (the float cases leave `check` something to judge)."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import dense_ref as dr
import stitch_ref as sr

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "vit-with-opencl_amd" / "csrc"
FLAGS = ["-O1", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-ffp-contract=off", "-fsanitize=address,undefined",
         "-fno-omit-frame-pointer"]

STACK = [(20.0, 8.0, 36.0, 24.0)] * 40                      # 40 windows on one 16 x 16 spot
# (frame_h, frame_w, block, boxes): frames that are no multiple of the block; a window inside one block; one over all blocks;
# the stack; edges exactly on a block border and on a pixel centre (31.5: pixel 31's centre, covered from the left edge on,
# not up to the right edge); fractional corners; the flush tiling of the GPU tests at both block sizes
INDEX_CASES = [
    (45, 70, 32, sr.tiles(45, 70, 32, 16)),
    (45, 70, 16, sr.tiles(45, 70, 32, 16)),
    (45, 70, 32, [(33.0, 33.0, 40.0, 44.0)]),
    (45, 70, 32, [(0.0, 0.0, 70.0, 45.0)]),
    (45, 70, 32, STACK),
    (45, 70, 16, STACK + [(0.0, 0.0, 70.0, 45.0)]),
    (45, 70, 32, [(31.5, 31.5, 64.0, 45.0), (0.0, 0.0, 31.5, 31.5), (32.0, 0.0, 64.0, 32.0), (31.25, 0.5, 32.5, 31.75)]),
    (45, 70, 16, [(31.5, 31.5, 64.0, 45.0), (0.0, 0.0, 31.5, 31.5), (15.5, 15.5, 16.5, 16.5), (15.75, 15.75, 16.75, 16.75)]),
    (40, 40, 16, sr.tiles(40, 40, 16, 8)),
    (1, 1, 16, [(0.0, 0.0, 1.0, 1.0)]),
    (33, 17, 1, [(0.25, 0.75, 16.5, 32.5), (3.0, 3.0, 4.0, 4.0)]),
    (260, 300, 16, sr.tiles(260, 300, 224, 150)),
]
GOOD = (10.0, 10.0, 20.0, 20.0)
# (frame_h, frame_w, block, n or None, boxes, a word of the message); block -1: vit_stitch_check alone
REFUSALS = [
    (0, 70, 32, None, [GOOD], "frame"), (45, 0, 32, None, [GOOD], "frame"), (16385, 70, 32, None, [GOOD], "frame"),
    (45, 16385, 32, None, [GOOD], "frame"), (45, 70, 0, None, [GOOD], "block"), (45, 70, 16385, None, [GOOD], "block"),
    (45, 70, 32, 0, [], "n_windows"),
    (45, 70, 32, None, [GOOD, (-1.0, 0.0, 10.0, 10.0)], "window 1"), (45, 70, 32, None, [(0.0, 0.0, 70.5, 10.0)], "window 0"),
    (45, 70, 32, None, [(0.0, 0.0, 10.0, 45.25)], "window 0"), (45, 70, 32, None, [(5.0, 5.0, 5.5, 10.0)], "window 0"),
    (45, 70, 32, None, [(5.0, 5.0, 10.0, 5.75)], "window 0"), (45, 70, 32, None, [GOOD, GOOD, (float("nan"), 0.0, 9.0, 9.0)], "window 2"),
    (45, 70, 32, None, [(0.0, 0.0, float("inf"), 9.0)], "window 0"),
    (45, 70, -1, None, [GOOD, (0.0, 40.0, 10.0, 46.0)], "window 1"), (45, 70, -1, 0, [], "n_windows"), (0, 70, -1, None, [GOOD], "frame"),
    (45, 70, -1, -1, [], "NULL"),
]


def case_text(h, w, block, boxes, n=None):
    words = [str(h), str(w), str(block), str(len(boxes) if n is None else n)]
    words += [float(np.float32(v)).hex() if np.isfinite(v) else str(v) for b in boxes for v in b]
    return " ".join(words) + "\n"


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("stitch") / "stitch_index"
    build = subprocess.run(["gcc", *FLAGS, "-Wall", f"-I{ROOT / 'include'}", f"-I{CSRC}", str(CSRC / "vit_stitch.c"), str(CSRC / "vit_ingest.c"),
                            str(ROOT / "tests" / "stitch_index_main.c"), "-o", str(exe), "-lm"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    assert "warning" not in build.stderr, build.stderr

    def run(text):
        r = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120,
                           env={"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})
        assert r.returncode == 0, r.stdout + r.stderr
        assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
        return r.stdout.splitlines()
    return run


def test_index_is_the_per_pixel_statement(program):
    """every case's offsets and ids are what looking at every pixel of every block gives: exact, not a superset"""
    out = program("".join(case_text(h, w, block, boxes) for h, w, block, boxes in INDEX_CASES))
    assert out[-1] == f"stitch index: {len(INDEX_CASES)} cases"
    assert len(out) == 3 * len(INDEX_CASES) + 1
    for k, (h, w, block, boxes) in enumerate(INDEX_CASES):
        offsets, ids = sr.index_ref(h, w, block, boxes)
        head, got_off, got_ids = (line.split() for line in out[3 * k:3 * k + 3])
        assert head == ["ok", str(len(ids))], (k, head)
        assert [int(v) for v in got_off[1:]] == offsets, k
        assert [int(v) for v in got_ids[1:]] == ids, k
        for a, b in zip(offsets, offsets[1:]):
            assert all(x < y for x, y in zip(ids[a:b], ids[a + 1:b])), k
    # what the cases hold: a block of the stack lists all 40; the window inside one block is in that block alone; pixel 31 belongs
    # to the window that starts at 31.5 and not to the one that ends there
    offsets, ids = sr.index_ref(45, 70, 32, STACK)
    assert max(b - a for a, b in zip(offsets, offsets[1:])) == 40
    offsets, ids = sr.index_ref(45, 70, 32, INDEX_CASES[2][3])
    assert offsets == [0, 0, 0, 0, 0, 1, 1]
    offsets, ids = sr.index_ref(45, 70, 32, INDEX_CASES[6][3])
    assert ids[offsets[0]:offsets[1]] == [0, 1, 3] and 1 not in ids[offsets[4]:offsets[5]]


def test_every_refusal(program):
    out = program("".join(case_text(h, w, block, boxes, n) for h, w, block, n, boxes, _ in REFUSALS))
    assert len(out) == len(REFUSALS) + 1
    for line, (h, w, block, n, boxes, word) in zip(out, REFUSALS):
        who = "caller: " if block == -1 else "vit_stitch_index: "
        assert line.startswith("refused " + who) and word in line, (line, word)


def test_library_entry_points_agree(pkg):
    """binding.stitch_index, through the built library, gives the same index; stitch_check raises with the caller's name"""
    for h, w, block, boxes in INDEX_CASES[:3] + INDEX_CASES[6:8]:
        offsets, ids = pkg.binding.stitch_index(h, w, boxes, block)
        want = sr.index_ref(h, w, block, boxes)
        assert offsets.dtype == np.int32 and offsets.tolist() == want[0] and ids.tolist() == want[1]
    pkg.binding.stitch_check(45, 70, [GOOD])
    with pytest.raises(pkg.binding.VitHipError, match="window 1"):
        pkg.binding.stitch_check(45, 70, [GOOD, (0.0, 0.0, 71.0, 10.0)])
    assert pkg.binding.STITCH_BLOCK == 16


def test_frame_sizes(pkg):
    b = pkg.binding
    cfg = pkg.preset("vit_b_16")
    L = pkg.lib()
    import ctypes as C

    def sizes(fh=3000, fw=4000, n=432, **kw):
        head = dict(tap=-1, final_norm=1, n_labels=150, out_h=0, out_w=0, weight_stride=768)
        fill = kw.pop("fill", 255)
        head.update(kw)
        spec = b.FrameSpecC(b.DenseSpecC(head["tap"], head["final_norm"], head["n_labels"], head["out_h"], head["out_w"],
                                         head["weight_stride"], None, None), fill)
        lab, scr = C.c_size_t(), C.c_size_t()
        rc = L.vit_frame_sizes(C.byref(cfg), C.byref(spec), fh, fw, n, C.byref(lab), C.byref(scr))
        return rc, lab.value, scr.value, L.vh_last_error().decode()

    rc, lab, scr, _ = sizes()
    blocks = (3000 // 16 + 1) * (4000 // 16)
    assert rc == 0 and lab == 12_000_000 and scr == 432 * 196 * 150 * 4 + L.vh_dense_stitch_scratch(432, 3000, 4000, 0)
    assert L.vh_dense_stitch_scratch(432, 3000, 4000, 0) >= 432 * 16 + (blocks + 1) * 4
    for kw, word in ((dict(out_h=224), "out_h"), (dict(out_w=1), "out_h"), (dict(fill=256), "fill_label"), (dict(fill=-1), "fill_label"),
                     (dict(fh=0), "frame"), (dict(fw=16385), "frame"), (dict(n=0), "n_windows"), (dict(n=2 ** 31 // 196 + 1), "n_windows"),
                     (dict(n_labels=257), "n_labels"), (dict(tap=12), "tap")):
        rc, _, _, msg = sizes(**kw)
        assert rc == 1 and word in msg, (kw, msg)
    fine = pkg.preset("vit_b_16")                                      # a 112 x 112 patch grid: a model the dense head does not take
    fine.patch_size = 2
    spec = b.FrameSpecC(b.DenseSpecC(-1, 1, 21, 0, 0, 768, None, None), 255)
    assert L.vit_frame_sizes(C.byref(fine), C.byref(spec), 300, 400, 4, None, None) == 1
    assert "64" in L.vh_last_error().decode()
    wide = pkg.preset("vit_b_16")
    wide.img_width = 320
    spec = b.FrameSpecC(b.DenseSpecC(-1, 1, 21, 0, 0, 768, None, None), 255)
    assert L.vit_frame_sizes(C.byref(wide), C.byref(spec), 300, 400, 4, None, None) == 1
    assert "non-square" in L.vh_last_error().decode()


# ---- the reference against itself and against dense_ref --------------------------------------------------------------

@pytest.mark.parametrize("grid,Cc,H,W", [((3, 5), 17, 37, 53), ((14, 14), 21, 224, 224), ((14, 14), 256, 7, 5), ((1, 1), 2, 33, 65)])
def test_one_whole_frame_window_is_the_dense_head(grid, Cc, H, W):
    rng = np.random.default_rng(H + W)
    box = [(0.0, 0.0, float(W), float(H))]
    Lr = rng.standard_normal((1, grid[0] * grid[1], Cc)).astype(np.float32)
    m, cnt = sr.stitch64(Lr, grid, box, H, W)
    assert (cnt == 1).all()
    assert np.allclose(m, dr.upsample64(Lr.astype(np.float64), grid, (H, W))[0], rtol=1e-13, atol=1e-13)
    Li = rng.integers(-8, 9, size=Lr.shape).astype(np.float32)
    Li[0, 0, 0], Li[0, -1, 1] = np.nan, -np.inf
    lab, bits, cover = sr.stitch32(Li, grid, box, H, W, 255)
    want_lab, want_bits = dr.dense32(Li, grid, (H, W))
    assert np.array_equal(lab, want_lab[0]) and np.array_equal(bits, want_bits[0]) and (cover == 1).all()


def test_integer_overlap_is_exact_in_both_references():
    """integer logits under dyadic weights: the fp32 statement and the float64 definition are the same numbers, so `check`
    holds with no error at all; counts 1, 2, 3, 4 and 6 occur"""
    H, W, grid, Cc = 45, 70, (4, 4), 5
    boxes = sr.tiles(H, W, 32, 16)
    Li = np.random.default_rng(5).integers(-8, 9, size=(len(boxes), 16, Cc)).astype(np.float32)
    lab, bits, cover = sr.stitch32(Li, grid, boxes, H, W, 255)
    assert set(np.unique(cover)) == {1, 2, 3, 4, 6}
    m, cnt = sr.stitch64(Li, grid, boxes, H, W)
    exact = np.isin(cnt, (1, 2, 4))                                   # thirds and sixths round
    assert np.array_equal(bits.view(np.float32)[exact], m.max(axis=-1).astype(np.float32)[exact])
    worst, _ = sr.check(Li, grid, boxes, H, W, 255, lab, bits.view(np.float32), cover)
    assert worst <= 1.0


@pytest.mark.parametrize("case", sr.FLOAT_CASES, ids=lambda c: f"{c[0]}x{c[1]}-t{c[2]}-C{c[5]}")
def test_float_cases_leave_the_check_something_to_judge(case):
    """under the float64 definition alone and twice the bound, at most 1 % of the pixels admit more than one label"""
    H, W, tile, stride, grid, Cc, seed = case
    boxes = sr.float_boxes(case)
    x, Wt, b = sr.float_case(len(boxes), grid, Cc, seed)
    L64 = dr.logits64(x, Wt, b)
    Lf = L64.astype(np.float32)
    corner = (sr.E_FLOAT + 8) * dr.U * dr.absdot(x, Wt, b)
    m, cnt = sr.stitch64(Lf, grid, boxes, H, W)
    on = cnt > 0
    assert on.mean() > 0.95 and (len(boxes) == 1 or cnt.max() >= 4)
    share = float((dr.admissible(m[on], 2 * sr.bound(Lf, grid, boxes, H, W, corner)[on]).sum(axis=-1) > 1).mean())
    assert share <= 0.01, share
