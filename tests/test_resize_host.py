"""CPU tests of the resize + centre crop's host side (include/ViT_opencl.h: vit_resize_crop_geometry and the argument checks
of vit_hip_resize_crop_u8 / vit_hip_forward_device_u8_resized / vit_hip_forward_u8_resized), and of tests/resize_ref.py, the
NumPy statement the GPU tests hold the kernel to: byte for byte Pillow where Pillow is installed, and the committed Pillow
hashes everywhere."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

import resize_ref as R

GOLDEN = Path(__file__).resolve().parent / "golden" / "resize_crop_pil_sha256.json"
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def _torchvision_geometry(h, w, rs, crop):
    """torchvision.transforms.functional._compute_resized_output_size and center_crop, written out"""
    short, long_ = (w, h) if w <= h else (h, w)
    new_short, new_long = rs, int(rs * long_ / short)
    new_w, new_h = (new_short, new_long) if w <= h else (new_long, new_short)
    return new_h, new_w, int(round((new_h - crop) / 2.0)), int(round((new_w - crop) / 2.0))


def test_geometry_is_torchvisions_arithmetic(pkg):
    b = pkg.binding
    sizes = [1, 2, 3, 99, 100, 223, 224, 225, 255, 256, 257, 299, 333, 375, 384, 480, 500, 511, 640, 999, 1000, 1333, 3000,
             4000, 16384]
    seen_half = seen_square = seen_h_rs = 0
    for rs, crop in ((224, 224), (248, 224), (256, 224), (384, 384), (518, 518), (896, 224), (255, 224), (257, 224)):
        for h in sizes:
            for w in sizes:
                want = _torchvision_geometry(h, w, rs, crop)
                assert b.resize_crop_geometry(h, w, rs, crop) == want, (h, w, rs, crop)
                seen_half += ((want[0] - crop) % 2 == 1) or ((want[1] - crop) % 2 == 1)
                seen_square += h == w
                seen_h_rs += h == rs
    assert seen_half > 100 and seen_square and seen_h_rs
    # round half to even: 500 x 375 at rs 256 -> 256 x 341, left = round(58.5) = 58; 257 wide -> round(16.5) = 16
    assert b.resize_crop_geometry(375, 500, 256, 224) == (256, 341, 16, 58)
    assert b.resize_crop_geometry(256, 257, 256, 224)[3] == round(16.5) == 16
    assert b.resize_crop_geometry(256, 259, 256, 224)[3] == round(17.5) == 18


def test_geometry_refusals(pkg):
    L, b = pkg.lib(), pkg.binding
    out = [C.c_int() for _ in range(4)]
    refs = [C.byref(o) for o in out]
    ok = b.resize_crop(256)
    for (h, w, rc, crop, msg) in ((0, 10, ok, 224, b"16384"), (10, 16385, ok, 224, b"16384"), (10, 10, b.resize_crop(223), 224, b"resize_short"),
                                  (10, 10, b.resize_crop(897), 224, b"resize_short"), (10, 10, b.ResizeCrop(256, 2), 224, b"filter"),
                                  (10, 10, ok, 0, b"crop")):
        assert L.vit_resize_crop_geometry(h, w, C.byref(rc), crop, *refs) == 1
        assert msg in L.vh_last_error()
    assert L.vit_resize_crop_geometry(10, 10, None, 224, *refs) == 1
    assert L.vit_resize_crop_geometry(10, 10, C.byref(ok), 224, None, *refs[1:]) == 1
    assert L.vit_resize_crop_geometry(16384, 16384, C.byref(b.resize_crop(896)), 224, *refs) == 0


def test_resize_forms_refuse_bad_arguments_without_a_device(pkg):
    """Code 1 with a message before any device call.  The stand-in context is a zeroed host buffer, so every check that
    reads it sees max_batch 0 and img_size 0: only checks ahead of those are reachable here; the GPU file checks the rest on
    a live context."""
    L, b = pkg.lib(), pkg.binding
    norm = pkg.pixel_norm(*IMAGENET)
    img = np.zeros((100, 120, 3), dtype=np.uint8)
    descs = b.image_descs([(img.ctypes.data, 100, 120, 360)])
    ok = b.resize_crop(256)
    stand_in = C.create_string_buffer(1 << 16)
    ctx = C.cast(stand_in, C.c_void_p)
    logits = np.empty((1, 1000), dtype=np.float32)
    for c, d, rc, nm in ((None, descs, ok, norm), (ctx, None, ok, norm), (ctx, descs, None, norm), (ctx, descs, ok, None)):
        rcp = C.byref(rc) if rc is not None else None
        nmp = C.byref(nm) if nm is not None else None
        assert L.vit_hip_forward_device_u8_resized(c, d, 1, 0, rcp, nmp, None, None, None) == 1
        assert b"vit_hip_forward_device_u8_resized: NULL" in L.vh_last_error()
        assert L.vit_hip_forward_u8_resized(c, d, 1, 0, rcp, nmp, b.fptr(logits), None) == 1
        assert b"vit_hip_forward_u8_resized: NULL" in L.vh_last_error()
    assert L.vit_hip_resize_crop_u8(ctx, descs, 1, 0, C.byref(ok), None, None) == 1
    assert b"vit_hip_resize_crop_u8: NULL" in L.vh_last_error()
    for n, layout, rc, msg in ((0, 0, ok, b"n must be positive"), (1, 2, ok, b"layout"), (1, 0, b.ResizeCrop(256, 5), b"filter")):
        assert L.vit_hip_forward_u8_resized(ctx, descs, n, layout, C.byref(rc), C.byref(norm), None, None) == 1
        assert msg in L.vh_last_error(), msg
    assert L.vit_hip_forward_device_u8_resized(ctx, descs, 1, 0, C.byref(ok), C.byref(norm), None, None, None) == 1
    assert b"max_batch" in L.vh_last_error()


def _pil_cases():
    """at least 100 (seed, h, w, channels, rs, crop, filter): both filters; upscales, identity, 1 x N and N x 1, ordinary
    photographs' sizes and downscales beyond 16x"""
    shapes = [(100, 150), (150, 100), (224, 224), (256, 256), (257, 300), (375, 500), (500, 375), (481, 257), (256, 999),
              (1000, 1333), (1, 700), (700, 1), (2, 3), (60, 90), (224, 300), (333, 224)]
    cases, seed = [], 1000
    for (h, w) in shapes:
        for f in ("bilinear", "bicubic"):
            for rs in (224, 248, 256):
                seed += 1
                cases.append((seed, h, w, 3, rs, 224, f))
    for (h, w, rs) in ((6000, 4000, 224), (4000, 6000, 256), (4100, 300, 224)):
        for f in ("bilinear", "bicubic"):
            seed += 1
            cases.append((seed, h, w, 3, rs, 224, f))
    cases += [(seed + 1, 300, 400, 1, 256, 224, "bicubic"), (seed + 2, 384, 512, 3, 384, 384, "bilinear")]
    # 1, 2 and 4 channels (independent bands) at other crops, up- and downscaled
    for k, (h, w, c, rs, crop) in enumerate(((70, 50, 1, 44, 40), (130, 170, 2, 168, 168), (500, 640, 2, 180, 168),
                                             (90, 120, 4, 350, 350), (700, 900, 4, 224, 224), (33, 300, 4, 96, 96))):
        for f in ("bilinear", "bicubic"):
            cases.append((seed + 10 + 2 * k + (f == "bicubic"), h, w, c, rs, crop, f))
    return cases


def test_reference_equals_pillow_byte_for_byte():
    pytest.importorskip("PIL")
    cases = _pil_cases()
    assert len(cases) >= 100
    for seed, h, w, c, rs, crop, f in cases:
        img = R.source_image(seed, h, w, c)
        got = R.resize_crop(img, rs, crop, R.FILTERS[f])
        want = R.pil_resize_crop(img, rs, crop, R.FILTERS[f])
        assert got.shape == (crop, crop, c)
        assert np.array_equal(got, want), (seed, h, w, c, rs, crop, f, int((got != want).sum()))


def test_two_and_four_channels_are_independent_bands_not_alpha():
    """2 and 4 channels: every channel is resized as an image of its own, in the reference and in the Pillow statement the
    committed hashes come from.  Pillow's RGBA resize premultiplies by the fourth channel: on a source whose fourth channel
    varies it gives other colour bytes, which is not what the library computes."""
    for c in (2, 4):
        img = R.source_image(77 + c, 90, 130, c)
        got = R.resize_crop(img, 48, 40, R.BICUBIC)
        for ch in range(c):
            alone = R.resize_crop(np.ascontiguousarray(img[:, :, ch:ch + 1]), 48, 40, R.BICUBIC)
            assert np.array_equal(got[:, :, ch], alone[:, :, 0]), (c, ch)
    Image = pytest.importorskip("PIL.Image")
    img = R.source_image(81, 90, 130, 4)
    assert len(np.unique(img[:, :, 3])) > 16
    ours = R.pil_resize_crop(img, 48, 40, R.BILINEAR)
    assert np.array_equal(ours, R.resize_crop(img, 48, 40, R.BILINEAR))
    nh, nw, top, left = R.geometry(90, 130, 48, 40)
    rgba = np.asarray(Image.fromarray(img, "RGBA").resize((nw, nh), Image.Resampling.BILINEAR))[top:top + 40, left:left + 40]
    assert np.array_equal(rgba[:, :, 3], ours[:, :, 3]) and not np.array_equal(rgba[:, :, :3], ours[:, :, :3])


def test_sources_saturate_and_bicubic_clips():
    """the sources hold hard 0 / 255 edges, and bicubic overshoot clips at both ends"""
    img = R.source_image(5, 375, 500)
    assert (img == 0).mean() > 0.02 and (img == 255).mean() > 0.02
    xmin, cnt, k = R.coefficients(500, 341, R.BICUBIC, 58, 224)
    assert (k < 0).any()
    assert k.sum(axis=1).min() >= (1 << 22) - 8 and k.sum(axis=1).max() <= (1 << 22) + 8


def test_committed_pillow_hashes_equal_the_reference():
    golden = json.loads(GOLDEN.read_text())
    assert len(golden["cases"]) == len(R.GOLDEN_CASES)
    for case, (seed, h, w, c, rs, crop, f) in zip(golden["cases"], R.GOLDEN_CASES):
        assert (case["seed"], case["height"], case["width"], case["channels"], case["resize_short"], case["crop"],
                case["filter"]) == (seed, h, w, c, rs, crop, f)
        assert R.sha256(R.resize_crop(R.source_image(seed, h, w, c), rs, crop, R.FILTERS[f])) == case["sha256"], case
