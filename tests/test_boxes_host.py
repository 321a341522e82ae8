"""CPU tests of the box crops' host side (include/ViT_opencl.h: vit_box_check, vit_box_rows, vit_tile_boxes and the argument
checks of vit_hip_crop_boxes_u8 / vit_hip_forward_device_u8_boxes / vit_hip_forward_u8_boxes), and of tests/box_ref.py, the
NumPy statement the GPU tests hold the kernel to: byte for byte Pillow's Image.resize(box=) where Pillow is installed, and
the committed Pillow hashes everywhere."""
import ctypes as C
import functools
import json
from pathlib import Path

import numpy as np
import pytest

import box_ref as B

GOLDEN = Path(__file__).resolve().parent / "golden" / "box_resize_pil_sha256.json"
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
F32 = np.float32


@functools.lru_cache(maxsize=None)
def _source(seed, h, w, c):
    """shared by the Pillow and the hash test; read only"""
    img = B.source_image(seed, h, w, c)
    img.setflags(write=False)
    return img


def test_the_case_list_holds_every_kind_of_box():
    cases = B.GOLDEN_CASES
    assert 35 <= len(cases) <= 48
    assert {c[6] for c in cases} == {"bilinear", "bicubic"} and {c[3] for c in cases} == {1, 2, 3, 4}
    assert {(c[3], c[5]) for c in cases} == {(3, 224), (1, 40), (2, 168), (4, 168), (3, 384), (4, 768)}
    kinds = {k: 0 for k in ("identity", "fractional", "left", "top", "right", "bottom", "whole", "1x1", "1xN", "Nx1", "over16",
                            "nonsquare", "src1x700", "src700x1")}
    for _, h, w, _, (l, t, r, b), out, _ in cases:
        bw, bh = r - l, b - t
        whole = (l, t, r, b) == (0, 0, w, h)
        kinds["identity"] += bw == out and bh == out and l > 0 and t > 0 and float(l).is_integer() and float(t).is_integer()
        kinds["fractional"] += any(not float(v).is_integer() for v in (l, t, r, b))
        kinds["left"] += l == 0 and not whole
        kinds["top"] += t == 0 and not whole
        kinds["right"] += r == w and not whole
        kinds["bottom"] += b == h and not whole
        kinds["whole"] += whole
        kinds["1x1"] += bw == 1 and bh == 1
        kinds["1xN"] += bw == 1 and bh > 1 and w > 1
        kinds["Nx1"] += bh == 1 and bw > 1 and h > 1
        kinds["over16"] += bw > 16 * out or bh > 16 * out
        kinds["nonsquare"] += bw != bh
        kinds["src1x700"] += (h, w) == (1, 700)
        kinds["src700x1"] += (h, w) == (700, 1)
    assert all(kinds.values()), kinds


def test_reference_equals_pillow_byte_for_byte():
    """the golden cases, and hashed quarter-pixel boxes of four sources in 1 to 4 channels with both filters"""
    pytest.importorskip("PIL")
    cases = list(B.GOLDEN_CASES)
    for k, (h, w, c, out) in enumerate(((90, 130, 1, 40), (211, 160, 2, 56), (300, 401, 3, 64), (57, 64, 4, 48))):
        for i, box in enumerate(B.hashed_boxes(50 + k, 10, h, w)):
            cases.append((500 + k, h, w, c, box, out, ("bilinear", "bicubic")[i % 2]))
    assert len(cases) >= 80
    for seed, h, w, c, box, out, f in cases:
        img = _source(seed, h, w, c)
        got = B.resize_box(img, box, out, B.FILTERS[f])
        want = B.pil_resize_box(img, box, out, B.FILTERS[f])
        assert got.shape == (out, out, c)
        assert np.array_equal(got, want), (seed, h, w, c, box, out, f, int((got != want).sum()))


def test_committed_pillow_hashes_equal_the_reference():
    golden = json.loads(GOLDEN.read_text())
    assert len(golden["cases"]) == len(B.GOLDEN_CASES)
    for case, (seed, h, w, c, box, out, f) in zip(golden["cases"], B.GOLDEN_CASES):
        assert (case["seed"], case["height"], case["width"], case["channels"], tuple(case["box"]), case["out"],
                case["filter"]) == (seed, h, w, c, tuple(float(v) for v in box), out, f)
        assert B.sha256(B.resize_box(_source(seed, h, w, c), box, out, B.FILTERS[f])) == case["sha256"], case


def test_a_whole_image_box_is_the_existing_resize():
    """in0 = 0, in1 = (float)in: the coefficients of resize_ref, which the committed resize hashes pin"""
    for in_size, out, f in ((500, 224, B.BILINEAR), (375, 256, B.BICUBIC), (16384, 224, B.BICUBIC), (100, 224, B.BILINEAR), (1, 40, B.BICUBIC)):
        for got, want in zip(B.coefficients(in_size, 0, in_size, out, f), B.R.coefficients(in_size, out, f, 0, out)):
            assert np.array_equal(got, want), (in_size, out, f)


def _check(L, h, w, box):
    return L.vit_box_check(h, w, (C.c_float * 4)(*box))


def test_box_check_accepts_and_refuses_exactly_the_domain(pkg):
    L = pkg.lib()
    h, w = 375, 500
    up, down = (lambda v: float(np.nextafter(F32(v), F32(np.inf)))), (lambda v: float(np.nextafter(F32(v), F32(-np.inf))))
    accepted = [(0, 0, w, h), (0, 0, 1, 1), (w - 1, h - 1, w, h), (10.25, 20.5, 300.75, 310.125), (-0.0, -0.0, 1, 1), (1, 1, 2, 2),
                (down(w - 1), 0, w, 1), (0, down(h - 1), 1, h), (0, 0, up(1), up(1)), (123, 0, 124, h), (0, 77, w, 78)]
    for box in accepted:
        assert _check(L, h, w, box) == 0, (box, L.vh_last_error())
    tiny = float(np.nextafter(F32(0), F32(1)))
    refused = {
        (-tiny, 0, 10, 10): b"outside", (0, -tiny, 10, 10): b"outside", (-1, 0, 10, 10): b"outside",
        (0, 0, up(w), 10): b"outside", (0, 0, 10, up(h)): b"outside", (0, 0, w + 1, h): b"outside",
        (1, 1, down(2), 2): b"1 px", (1, 1, 2, down(2)): b"1 px", (up(w - 1), 0, w, h): b"1 px", (0, up(h - 1), w, h): b"1 px",
        (10, 10, 10, 20): b"1 px", (20, 10, 10, 20): b"1 px", (10, 20, 20, 10): b"1 px",
    }
    for k in range(4):
        for bad in (np.nan, np.inf, -np.inf):
            box = [10.0, 10.0, 20.0, 20.0]
            box[k] = bad
            refused[tuple(box)] = b"finite"
    for box, msg in refused.items():
        assert _check(L, h, w, box) == 1, box
        assert b"vit_box_check" in L.vh_last_error() and msg in L.vh_last_error(), (box, L.vh_last_error())
    for hh, ww in ((0, 10), (10, 0), (16385, 10), (10, 16385)):
        assert _check(L, hh, ww, (0, 0, 1, 1)) == 1 and b"16384" in L.vh_last_error()
    assert _check(L, 16384, 16384, (0, 0, 16384, 16384)) == 0
    assert L.vit_box_check(h, w, None) == 1 and b"NULL" in L.vh_last_error()
    with pytest.raises(pkg.VitHipError, match="outside"):
        pkg.binding.box_check(h, w, (0, 0, w + 0.5, h))
    pkg.binding.box_check(h, w, (0, 0, w, h))


def test_box_rows_are_the_references_bounds(pkg):
    b = pkg.binding
    checked = 0
    for _, h, w, _, (_, top, _, bottom), out, f in B.GOLDEN_CASES:
        assert b.box_rows(h, top, bottom, out, f) == B.box_rows(h, top, bottom, out, B.FILTERS[f]), (h, top, bottom, out, f)
        checked += 1
    for k, (h, out) in enumerate(((3000, 224), (333, 224), (16384, 224), (57, 40), (1000, 768))):
        for i, (_, top, _, bottom) in enumerate(B.hashed_boxes(900 + k, 40, h, 64)):
            f = ("bilinear", "bicubic")[i % 2]
            first, count = b.box_rows(h, top, bottom, out, f)
            assert (first, count) == B.box_rows(h, top, bottom, out, B.FILTERS[f]), (h, top, bottom, out, f)
            assert 0 <= first and count >= 1 and first + count <= h
            checked += 1
    assert checked == len(B.GOLDEN_CASES) + 200


def test_box_rows_refusals(pkg):
    L = pkg.lib()
    first, count = C.c_int(), C.c_int()
    refs = (C.byref(first), C.byref(count))
    for args, msg in (((100, 0, 101, 10, 0), b"outside"), ((100, 5, 5.5, 10, 0), b"1 px"), ((100, 0, 50, 0, 0), b"out must"),
                      ((100, 0, 50, 10, 2), b"filter"), ((0, 0, 1, 10, 0), b"16384"), ((100, float("nan"), 50, 10, 1), b"finite")):
        assert L.vit_box_rows(*args, *refs) == 1, args
        assert b"vit_box_rows" in L.vh_last_error() and msg in L.vh_last_error(), (args, L.vh_last_error())
    assert L.vit_box_rows(100, 0, 50, 10, 0, None, refs[1]) == 1 and b"NULL" in L.vh_last_error()
    assert L.vit_box_rows(100, 0, 100, 10, 1, *refs) == 0 and (first.value, count.value) == (0, 100)


def _covered(boxes, h, w):
    hit = np.zeros((h, w), dtype=bool)
    for _, (l, t, r, b) in boxes:
        assert all(float(v).is_integer() for v in (l, t, r, b))
        assert 0 <= l < r <= w and 0 <= t < b <= h
        hit[int(t):int(b), int(l):int(r)] = True
    return bool(hit.all())


def test_tile_boxes_cover_the_image_row_major(pkg):
    b, L = pkg.binding, pkg.lib()
    for h, w, tile, stride in ((3000, 4000, 224, 224), (3000, 4000, 224, 160), (224, 224, 224, 224), (225, 224, 224, 1),
                               (100, 333, 40, 33), (57, 64, 57, 57), (448, 672, 224, 224), (449, 673, 224, 224), (50, 50, 7, 3)):
        boxes = b.tile_boxes(h, w, tile, stride, image=3)
        assert _covered(boxes, h, w), (h, w, tile, stride)
        assert all(img == 3 and r - l == tile and bt - t == tile for img, (l, t, r, bt) in boxes)
        keys = [(t, l) for _, (l, t, _, _) in boxes]
        assert keys == sorted(keys) and len(set(keys)) == len(keys), "row-major, no box twice"
        xs, ys = sorted({l for _, (l, _, _, _) in boxes}), sorted({t for _, (_, t, _, _) in boxes})
        assert len(boxes) == len(xs) * len(ys)
        assert xs[-1] == w - tile and ys[-1] == h - tile and xs[0] == 0 and ys[0] == 0
        assert all(x == i * stride for i, x in enumerate(xs[:-1])) and all(y == i * stride for i, y in enumerate(ys[:-1]))
        assert xs[-1] - xs[-2] <= stride if len(xs) > 1 else True
        # the count comes back whatever the capacity; only `capacity` boxes are written
        few = (b.Box * 2)()
        few[1].image = -7
        assert L.vit_tile_boxes(h, w, tile, stride, 3, few, 1) == len(boxes)
        assert (few[0].image, tuple(few[0].box)) == boxes[0] and few[1].image == -7
        assert L.vit_tile_boxes(h, w, tile, stride, 3, None, 0) == len(boxes)
    frame = b.tile_boxes(3000, 4000, 224, 224)
    assert len(frame) == 14 * 18
    assert frame[17][1] == (4000 - 224, 0, 4000, 224) and frame[-1][1] == (4000 - 224, 3000 - 224, 4000, 3000)
    assert frame[13 * 18][1] == (0, 3000 - 224, 224, 3000) and frame[18][1] == (0, 224, 224, 448)
    assert pkg.tile_boxes(448, 448, 224, 224) == [(0, (0, 0, 224, 224)), (0, (224, 0, 448, 224)), (0, (0, 224, 224, 448)),
                                                 (0, (224, 224, 448, 448))]


def test_tile_boxes_refusals(pkg):
    L, b = pkg.lib(), pkg.binding
    out = (b.Box * 4)()
    for args, msg in (((100, 100, 101, 50), b"tile"), ((100, 300, 101, 50), b"tile"), ((100, 100, 0, 1), b"tile"),
                      ((100, 100, 50, 0), b"stride"), ((100, 100, 50, 51), b"stride"), ((0, 100, 1, 1), b"16384"),
                      ((100, 16385, 50, 50), b"16384")):
        assert L.vit_tile_boxes(*args, 0, out, 4) == -1, args
        assert b"vit_tile_boxes" in L.vh_last_error() and msg in L.vh_last_error(), (args, L.vh_last_error())
    assert L.vit_tile_boxes(100, 100, 50, 50, -1, out, 4) == -1 and b"image" in L.vh_last_error()
    assert L.vit_tile_boxes(100, 100, 50, 50, 0, None, 4) == -1 and b"NULL" in L.vh_last_error()
    assert L.vit_tile_boxes(100, 100, 50, 50, 0, out, -1) == -1
    with pytest.raises(pkg.VitHipError, match="stride"):
        b.tile_boxes(100, 100, 50, 0)


def test_box_forms_refuse_bad_arguments_without_a_device(pkg):
    """Code 1 with a message before any device call.  The stand-in context is a zeroed host buffer, so every check that
    reads it sees max_batch 0 and img_size 0: only checks ahead of those are reachable here; the GPU file checks the rest on
    a live context."""
    L, b = pkg.lib(), pkg.binding
    norm = pkg.pixel_norm(*IMAGENET)
    img = np.zeros((100, 120, 3), dtype=np.uint8)
    descs = b.image_descs([(img.ctypes.data, 100, 120, 360)])
    boxes = b.box_array([(0, (0, 0, 50, 50))])
    stand_in = C.create_string_buffer(1 << 16)
    ctx = C.cast(stand_in, C.c_void_p)
    logits = np.empty((1, 1000), dtype=np.float32)
    for c, d, bx, nm in ((None, descs, boxes, norm), (ctx, None, boxes, norm), (ctx, descs, None, norm), (ctx, descs, boxes, None)):
        nmp = C.byref(nm) if nm is not None else None
        assert L.vit_hip_forward_device_u8_boxes(c, d, 1, bx, 1, 0, 0, nmp, None, None, None) == 1
        assert b"vit_hip_forward_device_u8_boxes: NULL" in L.vh_last_error()
        assert L.vit_hip_forward_u8_boxes(c, d, 1, bx, 1, 0, 0, nmp, b.fptr(logits), None) == 1
        assert b"vit_hip_forward_u8_boxes: NULL" in L.vh_last_error()
    assert L.vit_hip_crop_boxes_u8(ctx, descs, 1, boxes, 1, 0, 0, None, None) == 1
    assert b"vit_hip_crop_boxes_u8: NULL" in L.vh_last_error()
    for n_images, n, layout, f, msg in ((1, 0, 0, 0, b"n must be positive"), (0, 1, 0, 0, b"n_images"), (1, 1, 2, 0, b"layout"),
                                        (1, 1, 0, 5, b"filter")):
        assert L.vit_hip_forward_u8_boxes(ctx, descs, n_images, boxes, n, layout, f, C.byref(norm), None, None) == 1
        assert msg in L.vh_last_error(), msg
    assert L.vit_hip_forward_device_u8_boxes(ctx, descs, 1, boxes, 1, 0, 0, C.byref(norm), None, None, None) == 1
    assert b"max_batch" in L.vh_last_error()
    for bad, msg in (((1, (0, 0, 50, 50)), b"image index"), ((-1, (0, 0, 50, 50)), b"image index"), ((0, (0, 0, 121, 50)), b"outside"),
                     ((0, (0, 0, 50, float("nan"))), b"finite"), ((0, (10, 10, 10.5, 50)), b"1 px")):
        assert L.vit_hip_forward_u8_boxes(ctx, descs, 1, b.box_array([(0, (0, 0, 50, 50)), bad]), 2, 0, 0, C.byref(norm), None, None) == 1
        assert b"box 1" in L.vh_last_error() and msg in L.vh_last_error(), (bad, L.vh_last_error())
    wide = b.image_descs([(img.ctypes.data, 100, 16385, 16385 * 3)])
    assert L.vit_hip_forward_u8_boxes(ctx, wide, 1, boxes, 1, 0, 0, C.byref(norm), None, None) == 1
    assert b"image 0" in L.vh_last_error() and b"16384" in L.vh_last_error()
