"""Box crops on the GPU (vit_hip_crop_boxes_u8, vit_hip_forward_device_u8_boxes, vit_hip_forward_u8_boxes): crop bytes equal
to tests/box_ref.py (the NumPy statement of Pillow's Image.resize(box=)) and to Pillow's own committed hashes, the bytes of
the resize + centre crop path where the two coincide, logits bit-identical to vit_hip_forward_device_u8 fed those crops in
every operand path, and the host form's chunks -- every source's rows packed once -- bit-identical to the device form."""
import ctypes as C
import functools
import json
from pathlib import Path

import numpy as np
import pytest

import box_ref as B
from ingest_common import RESIZE_CASES, Staged, tiny_config, tiny_resize_context
from test_gpu_resize_input import ENV, IMAGENET, MODES

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "box_resize_pil_sha256.json"
TINY = [(1, 40), (2, 168), (4, 168), (3, 384), (4, 768)]   # the smallest crops that reach JN = 1, 2, 3, 5 and 12


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)


@pytest.fixture(scope="module")
def b16(pkg, device, weights):
    with pytest.MonkeyPatch.context() as mp:
        for var in ENV:
            mp.delenv(var, raising=False)
        m = pkg.ViTHip(pkg.preset("vit_b_16"), weights, device=0, max_batch=16)
    yield m
    m.close()


@functools.lru_cache(maxsize=None)
def _source(seed, h, w, c=3):
    """made once, shared, read only"""
    img = B.source_image(seed, h, w, c)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _want(seed, h, w, c, box, out, f):
    crop = B.resize_box(_source(seed, h, w, c), box, out, B.FILTERS[f])
    crop.setflags(write=False)
    return crop


def _crops_gpu(pkg, m, images, boxes, f, layout, staged=None):
    S, c = m.cfg.img_size, m.cfg.in_chans
    st = staged or Staged(pkg, images, layout)
    out = pkg.DeviceBuffer(len(boxes) * S * S * c, dtype=np.uint8)
    m.crop_boxes_u8(st.descs, boxes, out.ptr, filter=f, layout=layout)
    m.sync()
    return out.to_numpy((len(boxes), S, S, c))


def _device_u8(pkg, m, crops, norm):
    n, nc = crops.shape[0], m.cfg.num_classes
    d_img = pkg.DeviceBuffer.from_numpy(np.ascontiguousarray(crops), dtype=np.uint8)
    d_log, d_prob = pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)
    m.forward_device_u8(d_img.ptr, n, norm, "hwc", d_log.ptr, d_prob.ptr, None)
    m.sync()
    return d_log.to_numpy((n, nc)), d_prob.to_numpy((n, nc))


def _device_boxes(pkg, m, st, boxes, f, norm, layout="hwc"):
    n, nc = len(boxes), m.cfg.num_classes
    d_log, d_prob = pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)
    m.forward_device_u8_boxes(st.descs, boxes, norm, filter=f, layout=layout, d_logits=d_log.ptr, d_probs=d_prob.ptr)
    m.sync()
    return d_log.to_numpy((n, nc)), d_prob.to_numpy((n, nc))


# (seed, height, width) of five sources and sixteen boxes of them, the sources out of order: identity-size at an offset,
# fractional, the whole image, 1 x 1 px, the four edges, non-square, 1 x N and N x 1, a 1 x 700 and a 700 x 1 source, a
# downscale of 16.5x, and box 3 once more as box 12
SOURCES = [(41, 375, 500), (42, 300, 400), (43, 1, 700), (44, 700, 1), (45, 230, 3700)]
BOXES = [
    (1, (0, 50, 120, 250)), (0, (100, 50, 324, 274)), (4, (0, 0, 3700, 230)), (0, (10.3, 20.7, 300.2, 310.9)),
    (2, (0, 0, 700, 1)), (1, (250, 60, 400, 200)), (3, (0, 0, 1, 700)), (0, (0, 0, 500, 375)),
    (1, (30, 0, 330, 100)), (4, (40, 10, 41, 190)), (1, (100, 180, 360, 300)), (0, (0, 0, 1, 1)),
    (0, (10.3, 20.7, 300.2, 310.9)), (4, (5, 100, 3695, 101)), (2, (100.5, 0, 400.25, 1)), (1, (100, 100, 350, 150)),
]


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("f", ["bilinear", "bicubic"])
def test_crop_bytes_equal_the_reference_on_sixteen_boxes_of_five_sources(pkg, b16, f, layout):
    assert len(BOXES) == 16 == b16.max_batch and [i for i, _ in BOXES] != sorted(i for i, _ in BOXES)
    images = [_source(*s) for s in SOURCES]
    got = _crops_gpu(pkg, b16, images, BOXES, f, layout)   # Staged: odd offsets, padded rows
    for k, (i, box) in enumerate(BOXES):
        want = _want(*SOURCES[i], 3, box, 224, f)
        assert np.array_equal(got[k], want), f"{f} {layout} box {k} {box} of {SOURCES[i]}: {int((got[k] != want).sum())} bytes differ"
    assert np.array_equal(got[3], got[12])


def test_crop_bytes_equal_pillows_committed_hashes(pkg, b16):
    """every case of the box fixture, grouped by (channels, out) for the context -- ViT-B/16 and ingest_common's tiny contexts
    -- and into one call per filter; a source that several cases share is staged once"""
    cases = json.loads(GOLDEN.read_text())["cases"]
    by_context = {}
    for c in cases:
        by_context.setdefault((c["channels"], c["out"]), []).append(c)
    assert set(by_context) == {(3, 224)} | set(TINY) and all(key in RESIZE_CASES for key in TINY)
    checked = 0
    for (chans, out), group in by_context.items():
        m = b16 if (chans, out) == (3, 224) else tiny_resize_context(pkg, chans, out)
        try:
            for f in ("bilinear", "bicubic"):
                sub = [c for c in group if c["filter"] == f]
                keys = sorted({(c["seed"], c["height"], c["width"]) for c in sub})
                assert 0 < len(sub) <= m.max_batch
                images = [_source(*key, chans) for key in keys]
                boxes = [(keys.index((c["seed"], c["height"], c["width"])), tuple(c["box"])) for c in sub]
                for layout in ("hwc", "chw"):
                    got = _crops_gpu(pkg, m, images, boxes, f, layout)
                    for c, crop_bytes in zip(sub, got):
                        assert B.sha256(crop_bytes) == c["sha256"], f"{c} {layout}"
                        checked += 1
        finally:
            if m is not b16:
                m.close()
    assert checked == 2 * len(cases)


@pytest.mark.parametrize("f", ["bilinear", "bicubic"])
def test_a_whole_square_image_gives_the_bytes_of_resize_crop_u8(pkg, b16, f):
    """resize_short = img_size on a square source is the box (0, 0, side, side): one coefficient kernel serves both"""
    images = [_source(60 + i, side, side) for i, side in enumerate((224, 300, 1000, 57))]
    st = Staged(pkg, images, "hwc")
    old = pkg.DeviceBuffer(len(images) * 224 * 224 * 3, dtype=np.uint8)
    b16.resize_crop_u8(st.descs, 224, old.ptr, filter=f)
    b16.sync()
    got = _crops_gpu(pkg, b16, images, [(i, (0, 0, img.shape[1], img.shape[0])) for i, img in enumerate(images)], f, "hwc", staged=st)
    assert np.array_equal(got, old.to_numpy(got.shape))
    assert len(np.unique(got)) > 100


def _parity(pkg, m, chans):
    """logits and probabilities of the box forward, bit for bit those of the u8 forward fed box_ref's crops"""
    S = m.cfg.img_size
    norm = pkg.pixel_norm((IMAGENET[0] + (0.5,))[:chans], (IMAGENET[1] + (0.25,))[:chans])
    srcs = [(70, 300, 401), (71, 90, 60), (72, 1, 700)]
    images = [_source(*s, chans) for s in srcs]
    boxes = [(1, (0, 0, 60, 90)), (0, (10.25, 20.5, 300.75, 290.0)), (2, (100, 0, 400, 1)), (0, (177, 66, 401, 290)),
             (1, (59, 89, 60, 90)), (0, (0, 0, 401, 300))][: m.max_batch]
    for f, layout in (("bilinear", "hwc"), ("bicubic", "chw")):
        crops = np.stack([_want(*srcs[i], chans, box, S, f) for i, box in boxes])
        want_l, want_p = _device_u8(pkg, m, crops, norm)
        got_l, got_p = _device_boxes(pkg, m, Staged(pkg, images, layout), boxes, f, norm, layout)
        assert np.isfinite(want_l).all() and np.abs(want_l).max() > 0
        assert np.array_equal(got_l, want_l), f"{f} {layout}: max |dlogit| {np.abs(got_l - want_l).max():.3e}"
        assert np.array_equal(got_p, want_p), f"{f} {layout}: probabilities differ"


@pytest.mark.parametrize("mode", list(MODES))
def test_logits_bitwise_the_u8_path_on_reference_crops_tiny(pkg, device, monkeypatch, mode):
    """4 channels at 168 px, embed 256 (what the block-scaled mode needs), two layers"""
    precision, env = MODES[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = tiny_config(pkg, 4, 168, RESIZE_CASES[(4, 168)], embed=256, depth=2)
    m = pkg.ViTHip(cfg, pkg.synth_weights(cfg, 9), device=0, max_batch=6, precision=precision)
    try:
        _parity(pkg, m, 4)
    finally:
        m.close()


def test_logits_bitwise_the_u8_path_on_reference_crops_b16(pkg, b16):
    _parity(pkg, b16, 3)


def _device_form_in_calls(pkg, m, images, boxes, f, norm):
    st = Staged(pkg, images, "hwc")
    parts = [_device_boxes(pkg, m, st, boxes[a:a + m.max_batch], f, norm) for a in range(0, len(boxes), m.max_batch)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def test_host_form_equals_the_device_form_on_37_boxes_of_three_sources(pkg, b16):
    """three chunks of max_batch 16 (16, 16, 5); the sources named in the order 2, 0, 1, 1, 0, 2, ...; CHW and padded rows too"""
    srcs = [(80, 375, 500), (81, 640, 480), (82, 200, 1333)]
    images = [_source(*s) for s in srcs]
    order = [(2, 0, 1, 1, 0, 2, 0)[k % 7] for k in range(37)]
    pools = [B.hashed_boxes(90 + i, 37, s[1], s[2]) for i, s in enumerate(srcs)]
    boxes = [(i, pools[i][k]) for k, i in enumerate(order)]
    assert len(boxes) == 37 and order[:16] != sorted(order[:16])
    norm = pkg.pixel_norm(*IMAGENET)
    want_l, want_p = _device_form_in_calls(pkg, b16, images, boxes, "bicubic", norm)
    got_l, got_p = b16.forward_u8_boxes(images, boxes, "bicubic", *IMAGENET)
    assert np.isfinite(want_l).all()
    assert np.array_equal(got_l, want_l) and np.array_equal(got_p, want_p)
    chw = [np.ascontiguousarray(img.transpose(2, 0, 1)) for img in images]
    got_l, _ = b16.forward_u8_boxes(chw, boxes, "bicubic", *IMAGENET, layout="chw", probs=False)
    assert np.array_equal(got_l, want_l)
    wide = [np.zeros((img.shape[0], img.shape[1] + 7, 3), dtype=np.uint8) for img in images]
    for wd, img in zip(wide, images):
        wd[:, :img.shape[1]] = img
    got_l, _ = b16.forward_u8_boxes([wd[:, :img.shape[1]] for wd, img in zip(wide, images)], boxes, "bicubic", *IMAGENET, probs=False)
    assert np.array_equal(got_l, want_l)


def test_host_form_tiles_a_frame_larger_than_a_slot(pkg, b16):
    """a 4000 x 3000 frame (36 MB) through staging slots of 16 x 3 x 224^2 x 4 = 9.6 MB: per chunk only the rows its 16 tiles
    read go up.  Stride 224 gives 14 x 18 tiles, the last row and column moved flush to the edges."""
    frame = _source(15, 3000, 4000)
    slot = 16 * 3 * 224 * 224 * 4
    assert frame.nbytes > 3 * slot
    boxes = pkg.tile_boxes(3000, 4000, 224, 224)
    assert len(boxes) == 14 * 18
    got_l, got_p = b16.forward_u8_boxes([frame], boxes, "bilinear", *IMAGENET)
    norm = pkg.pixel_norm(*IMAGENET)
    st = Staged(pkg, [frame], "hwc")
    for part in (slice(0, 16), slice(len(boxes) - 16, len(boxes))):
        want_l, want_p = _device_boxes(pkg, b16, st, boxes[part], "bilinear", norm)
        assert np.array_equal(got_l[part], want_l) and np.array_equal(got_p[part], want_p)
    assert np.isfinite(got_l).all() and len(np.unique(got_l, axis=0)) > 1


def test_host_form_refuses_a_box_whose_rows_exceed_a_slot(pkg, b16):
    frame = _source(15, 3000, 4000)
    L = pkg.lib()
    # 805 rows x 4000 x 3 = 9.66 MB against a slot of 9.63 MB; the same box 8 rows lower in height fits
    for box, fits in (((0, 0, 4000, 804), False), ((0, 0, 4000, 796), True)):
        first, count = pkg.binding.box_rows(3000, box[1], box[3], 224, "bilinear")
        assert (count * 4000 * 3 <= 16 * 3 * 224 * 224 * 4) == fits, count
        if fits:
            got, _ = b16.forward_u8_boxes([frame], [(0, (0, 0, 224, 224)), (0, box)], "bilinear", *IMAGENET, probs=False)
            assert np.isfinite(got).all()
        else:
            with pytest.raises(pkg.VitHipError, match="box 1: the rows it reads are larger than a staging slot") as e:
                b16.forward_u8_boxes([frame], [(0, (0, 0, 224, 224)), (0, box)], "bilinear", *IMAGENET)
            assert "status 1" in str(e.value) and b"vit_hip_forward_u8_boxes" in L.vh_last_error()


def test_armed_topk_is_served_with_no_logits_asked_for(pkg, b16):
    b = pkg.binding
    images = [_source(80, 375, 500), _source(81, 640, 480)]
    boxes = [(k % 2, box) for k, box in enumerate(B.hashed_boxes(95, 19, 375, 480))]
    full, _ = b16.forward_u8_boxes(images, boxes, "bilinear", *IMAGENET, probs=False)
    labels = np.full((19, 5), -1, np.int32)
    b16.set_topk_host(b.TopKSpec(5, "logits"), labels=labels)
    try:
        none_l, none_p = b16.forward_u8_boxes(images, boxes, "bilinear", *IMAGENET, logits=False, probs=False)
    finally:
        b16.set_topk_host(None)
    assert none_l is None and none_p is None
    assert all(len(set(r)) == 5 for r in labels.tolist())
    assert np.array_equal(np.take_along_axis(full, labels, axis=1), -np.sort(-full, axis=1)[:, :5])
    assert np.array_equal(labels[:, 0], full.argmax(axis=1))


def test_refusals_on_a_live_context(pkg, b16):
    """every refusal is an argument check: code 1, its message, nothing launched, and the context serves the next call"""
    L, b = pkg.lib(), pkg.binding
    norm = pkg.pixel_norm(*IMAGENET)
    img = _source(85, 100, 120)
    st = Staged(pkg, [img], "hwc")
    ptr, h, w, stride = st.descs[0]
    nc = b16.cfg.num_classes
    d_log = pkg.DeviceBuffer(b16.max_batch * nc)
    sentinel = np.full(b16.max_batch * nc, -7.0, np.float32)
    assert L.vh_h2d(d_log.ptr, sentinel.ctypes.data_as(C.c_void_p), sentinel.nbytes, None) == 0
    one, ok = b.image_descs(st.descs), [(0, (0, 0, 50, 50))]
    up = float(np.nextafter(np.float32(w), np.float32(np.inf)))
    cases = {
        "n > max_batch": (one, 1, ok * (b16.max_batch + 1), 0, 0, b"max_batch"),
        "n_images 0": (one, 0, ok, 0, 0, b"n_images"),
        "layout 2": (one, 1, ok, 2, 0, b"layout"),
        "filter 2": (one, 1, ok, 0, 2, b"filter"),
        "row_stride": (b.image_descs([(ptr, h, w, w * 3 - 1)]), 1, ok, 0, 0, b"row_stride"),
        "width 16385": (b.image_descs([(ptr, h, 16385, 16385 * 3)]), 1, ok, 0, 0, b"16384"),
        "NULL data": (b.image_descs([(0, h, w, stride)]), 1, ok, 0, 0, b"NULL image data"),
        "image index 1": (one, 1, ok + [(1, (0, 0, 50, 50))], 0, 0, b"box 1: image index"),
        "image index -1": (one, 1, [(-1, (0, 0, 50, 50))], 0, 0, b"box 0: image index"),
        "right one ulp out": (one, 1, ok + [(0, (0, 0, up, 50))], 0, 0, b"box 1: box outside"),
        "bottom out": (one, 1, [(0, (0, 0, 50, h + 1))], 0, 0, b"outside"),
        "left < 0": (one, 1, [(0, (-0.25, 0, 50, 50))], 0, 0, b"outside"),
        "NaN": (one, 1, [(0, (0, float("nan"), 50, 50))], 0, 0, b"finite"),
        "inf": (one, 1, [(0, (0, 0, float("inf"), 50))], 0, 0, b"finite"),
        "half a pixel": (one, 1, ok * 3 + [(0, (10, 10, 10.5, 50))], 0, 0, b"box 3: box narrower"),
        "inverted": (one, 1, [(0, (50, 50, 10, 10))], 0, 0, b"1 px"),
    }
    for what, (descs, n_images, boxes, layout, f, msg) in cases.items():
        assert L.vit_hip_forward_device_u8_boxes(b16.ctx, descs, n_images, b.box_array(boxes), len(boxes), layout, f, C.byref(norm),
                                                 d_log.ptr, None, None) == 1, what
        assert b"vit_hip_forward_device_u8_boxes" in L.vh_last_error() and msg in L.vh_last_error(), (what, L.vh_last_error())
    out = pkg.DeviceBuffer(224 * 224 * 3, dtype=np.uint8)
    assert L.vit_hip_crop_boxes_u8(b16.ctx, one, 1, b.box_array(ok), 1, 0, 0, None, None) == 1 and b"NULL" in L.vh_last_error()
    assert L.vit_hip_crop_boxes_u8(b16.ctx, one, 1, b.box_array([(0, (0, 0, 121, 50))]), 1, 0, 0, out.ptr, None) == 1
    assert b"vit_hip_crop_boxes_u8: box 0: box outside" in L.vh_last_error()
    assert L.vit_hip_forward_device_u8_boxes(b16.ctx, one, 1, None, 1, 0, 0, C.byref(norm), d_log.ptr, None, None) == 1
    assert L.vit_hip_forward_device_u8_boxes(b16.ctx, one, 1, b.box_array(ok), 1, 0, 0, None, d_log.ptr, None, None) == 1
    host = b.host_image_descs([img], "hwc")[0]
    assert L.vit_hip_forward_u8_boxes(b16.ctx, host, 1, b.box_array([(0, (0, 0, 50, 50.5)), (2, (0, 0, 50, 50))]), 2, 0, 1, C.byref(norm),
                                      None, None) == 1
    assert b"vit_hip_forward_u8_boxes: box 1: image index" in L.vh_last_error()
    b16.sync()
    assert np.array_equal(d_log.to_numpy(), sentinel), "a refused call wrote logits"
    # the context still works
    want = _device_u8(pkg, b16, _want(85, 100, 120, 3, (0, 0, 50, 50), 224, "bilinear")[None], norm)[0]
    got, _ = _device_boxes(pkg, b16, st, ok, "bilinear", norm)
    assert np.array_equal(got, want)
