"""Resize + centre crop on the GPU (vit_hip_resize_crop_u8, vit_hip_forward_device_u8_resized, vit_hip_forward_u8_resized):
crop bytes equal to tests/resize_ref.py (the NumPy statement of Pillow's Resample.c) and to Pillow's own committed hashes,
and logits bit-identical to vit_hip_forward_device_u8 fed those crops, in every operand path."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

import resize_ref as R
from ingest_common import Staged

pytestmark = pytest.mark.gpu

ENV = ("VIT_HIP_P3", "VIT_HIP_GEMM_FP32", "VIT_HIP_ATTN", "VIT_HIP_LN_FOLD", "VIT_HIP_LAST_LAYER", "VIT_HIP_PRECISION")
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
GOLDEN = Path(__file__).resolve().parent / "golden" / "resize_crop_pil_sha256.json"

# (height, width): portrait, landscape, square, h == resize_short (256), upscales, 4000 x 3000, 1 x 700 and 700 x 1
RAGGED = [(500, 375), (375, 500), (256, 256), (256, 300), (100, 150), (4000, 3000), (1, 700), (700, 1), (257, 481)]


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)


def _crops_gpu(pkg, m, images, rs, f, layout):
    S, c = m.cfg.img_size, m.cfg.in_chans
    st = Staged(pkg, images, layout)
    out = pkg.DeviceBuffer(len(images) * S * S * c, dtype=np.uint8)
    m.resize_crop_u8(st.descs, rs, out.ptr, filter=f, layout=layout)
    m.sync()
    return out.to_numpy((len(images), S, S, c))


def _sources(shapes, seed, c=3):
    return [R.source_image(seed + i, h, w, c) for i, (h, w) in enumerate(shapes)]


def _device_u8(pkg, m, crops, norm):
    n, nc = crops.shape[0], m.cfg.num_classes
    d_img = pkg.DeviceBuffer.from_numpy(crops, dtype=np.uint8)
    d_log, d_prob = pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)
    m.forward_device_u8(d_img.ptr, n, norm, "hwc", d_log.ptr, d_prob.ptr, None)
    m.sync()
    return d_log.to_numpy((n, nc)), d_prob.to_numpy((n, nc))


def _device_resized(pkg, m, images, rs, f, norm, layout="hwc"):
    n, nc = len(images), m.cfg.num_classes
    st = Staged(pkg, images, layout)
    d_log, d_prob = pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)
    m.forward_device_u8_resized(st.descs, rs, norm, filter=f, layout=layout, d_logits=d_log.ptr, d_probs=d_prob.ptr)
    m.sync()
    return d_log.to_numpy((n, nc)), d_prob.to_numpy((n, nc))


@pytest.fixture(scope="module")
def b16(pkg, device, weights):
    with pytest.MonkeyPatch.context() as mp:
        for var in ENV:
            mp.delenv(var, raising=False)
        m = pkg.ViTHip(pkg.preset("vit_b_16"), weights, device=0, max_batch=16)
    yield m
    m.close()


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("f", ["bilinear", "bicubic"])
def test_crop_bytes_equal_the_reference_on_a_ragged_batch(pkg, b16, f, layout):
    images = _sources(RAGGED, 100)
    got = _crops_gpu(pkg, b16, images, 256, f, layout)
    for i, img in enumerate(images):
        want = R.resize_crop(img, 256, 224, R.FILTERS[f])
        assert np.array_equal(got[i], want), f"{f} {layout} image {i} {img.shape}: {int((got[i] != want).sum())} bytes differ"


def test_crop_bytes_equal_pillows_committed_hashes(pkg, b16):
    """every case of the Pillow fixture that a 3-channel 224 px context or one of ingest_common's tiny contexts serves,
    grouped by (channels, crop) for the context and into one call per (resize_short, filter)"""
    from ingest_common import RESIZE_CASES, tiny_resize_context
    cases = json.loads(GOLDEN.read_text())["cases"]
    by_context = {}
    for c in cases:
        by_context.setdefault((c["channels"], c["crop"]), []).append(c)
    served = [key for key in by_context if key == (3, 224) or key in RESIZE_CASES]
    assert (3, 224) in served and len(served) >= 12 and {1, 2, 3, 4} <= {ch for ch, _ in served}
    checked = {}
    for chans, crop in served:
        m = b16 if (chans, crop) == (3, 224) else tiny_resize_context(pkg, chans, crop)
        try:
            groups = {}
            for c in by_context[(chans, crop)]:
                groups.setdefault((c["resize_short"], c["filter"]), []).append(c)
            for (rs, f), group in groups.items():
                images = [R.source_image(c["seed"], c["height"], c["width"], chans) for c in group]
                for layout in ("hwc", "chw"):
                    got = _crops_gpu(pkg, m, images, rs, f, layout)
                    for c, crop_bytes in zip(group, got):
                        assert R.sha256(crop_bytes) == c["sha256"], f"{c} {layout}"
                        checked[(chans, crop)] = checked.get((chans, crop), 0) + 1
        finally:
            if m is not b16:
                m.close()
    assert checked[(3, 224)] >= 30
    assert sum(checked.values()) == 2 * sum(len(by_context[key]) for key in served)


MODES = {
    "f32": ("f32", {}),
    "bf16": ("bf16", {}),
    "fp8_fold": ("fp8", {}),
    "fp8_nofold": ("fp8", {"VIT_HIP_LN_FOLD": "0"}),
    "f32_fp16x2": ("f32_fp16x2", {}),
    "f32_p3_off": ("f32", {"VIT_HIP_P3": "0"}),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_logits_bitwise_the_u8_path_on_reference_crops(pkg, device, weights, monkeypatch, mode):
    precision, env = MODES[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = pkg.ViTHip(pkg.preset("vit_b_16"), weights, device=0, max_batch=8, precision=precision)
    try:
        norm = pkg.pixel_norm(*IMAGENET)
        shapes = [(500, 375), (375, 500), (224, 224), (90, 60), (1333, 1000), (1, 700)]
        for f, layout in (("bilinear", "hwc"), ("bicubic", "chw")):
            images = _sources(shapes, 200)
            crops = np.stack([R.resize_crop(img, 256, 224, R.FILTERS[f]) for img in images])
            want_l, want_p = _device_u8(pkg, m, crops, norm)
            got_l, got_p = _device_resized(pkg, m, images, 256, f, norm, layout)
            assert np.isfinite(want_l).all()
            assert np.array_equal(got_l, want_l), f"{mode} {f}: max |dlogit| {np.abs(got_l - want_l).max():.3e}"
            assert np.array_equal(got_p, want_p), f"{mode} {f}: probabilities differ"
    finally:
        m.close()


def test_b16_384_at_resize_short_384(pkg, device):
    cfg = pkg.preset("vit_b_16_384")
    m = pkg.ViTHip(cfg, pkg.synth_weights(cfg, 0), device=0, max_batch=2)
    try:
        norm = pkg.pixel_norm(*IMAGENET)
        images = _sources([(512, 683), (600, 384)], 300)
        crops = np.stack([R.resize_crop(img, 384, 384, R.BICUBIC) for img in images])
        want_l, want_p = _device_u8(pkg, m, crops, norm)
        got_l, got_p = _device_resized(pkg, m, images, 384, "bicubic", norm)
        assert np.array_equal(got_l, want_l) and np.array_equal(got_p, want_p)
    finally:
        m.close()


def test_host_form_equals_the_device_form_with_chunks_cut_by_bytes(pkg, device, weights):
    """max_batch 4: a staging slot holds 4 x 3 x 224^2 x 4 = 2408448 bytes, so a 700 x 1000 image (2100000 bytes) shares its
    chunk only with small ones, while small ones go four at a time"""
    m = pkg.ViTHip(pkg.preset("vit_b_16"), weights, device=0, max_batch=4)
    try:
        norm = pkg.pixel_norm(*IMAGENET)
        shapes = [(375, 500), (100, 150), (700, 1000), (60, 90), (224, 224), (1000, 700), (90, 90), (375, 500), (1, 700),
                  (256, 300), (80, 120)]
        images = _sources(shapes, 400)
        want_l = np.concatenate([_device_resized(pkg, m, images[i:i + 1], 256, "bilinear", norm)[0] for i in range(len(images))])
        want_p = np.concatenate([_device_resized(pkg, m, images[i:i + 1], 256, "bilinear", norm)[1] for i in range(len(images))])
        got_l, got_p = m.forward_u8_resized(images, 256, "bilinear", *IMAGENET)
        assert np.array_equal(got_l, want_l) and np.array_equal(got_p, want_p)
        chw = [np.ascontiguousarray(img.transpose(2, 0, 1)) for img in images]
        got_l, _ = m.forward_u8_resized(chw, 256, "bilinear", *IMAGENET, layout="chw", probs=False)
        assert np.array_equal(got_l, want_l)
        # rows with padding (a view into a wider array) go through as they are
        wide = [np.zeros((img.shape[0], img.shape[1] + 7, 3), dtype=np.uint8) for img in images]
        for wd, img in zip(wide, images):
            wd[:, :img.shape[1]] = img
        got_l, _ = m.forward_u8_resized([wd[:, :img.shape[1]] for wd, img in zip(wide, images)], 256, "bilinear", *IMAGENET,
                                        probs=False)
        assert np.array_equal(got_l, want_l)
        # an image larger than a whole slot is refused
        with pytest.raises(pkg.VitHipError, match="staging slot"):
            m.forward_u8_resized([R.source_image(1, 1000, 1000, 3)], 256, "bilinear", *IMAGENET)
    finally:
        m.close()


def test_batch_position_independence(pkg, b16):
    norm = pkg.pixel_norm(*IMAGENET)
    images = _sources([(375, 500), (500, 375), (224, 300), (1000, 1333), (256, 256), (90, 60), (700, 1)], 500)
    alone, _ = _device_resized(pkg, b16, [images[3]], 256, "bicubic", norm)
    for pos in (0, 3, 6):
        batch = [img for i, img in enumerate(images) if i != 3]
        batch.insert(pos, images[3])
        got, _ = _device_resized(pkg, b16, batch, 256, "bicubic", norm)
        assert np.array_equal(got[pos], alone[0]), pos


def test_queued_calls_keep_their_descriptors(pkg, b16):
    """twelve device-form calls (more than the descriptor ring holds) with different images and output buffers, queued on
    the context's stream with no host sync in between"""
    norm = pkg.pixel_norm(*IMAGENET)
    nc = b16.cfg.num_classes
    calls = []
    for k in range(12):
        shapes = [(300 + 17 * k, 400 - 9 * k), (500 - 11 * k, 375), (1 + k, 640)][: 1 + k % 3]
        images = _sources(shapes, 600 + 10 * k)
        crops = np.stack([R.resize_crop(img, 256, 224, R.BILINEAR) for img in images])
        calls.append((images, _device_u8(pkg, b16, crops, norm)[0]))
    staged = [Staged(pkg, images, "hwc") for images, _ in calls]   # uploads (and their syncs) first
    outs = [pkg.DeviceBuffer(len(images) * nc) for images, _ in calls]
    for st, d_log in zip(staged, outs):
        b16.forward_device_u8_resized(st.descs, 256, norm, d_logits=d_log.ptr)
    b16.sync()
    for k, ((images, want), d_log) in enumerate(zip(calls, outs)):
        assert np.array_equal(d_log.to_numpy((len(images), nc)), want), f"call {k}"


def test_refusals_on_a_live_context(pkg, b16):
    L = pkg.lib()
    b = pkg.binding
    norm = pkg.pixel_norm(*IMAGENET)
    st = Staged(pkg, _sources([(100, 120)], 700), "hwc")
    ptr, h, w, stride = st.descs[0]
    d_log = pkg.DeviceBuffer(b16.max_batch * b16.cfg.num_classes)
    ok = b.resize_crop(256)
    cases = {
        "n > max_batch": (b.image_descs([st.descs[0]] * (b16.max_batch + 1)), b16.max_batch + 1, 0, ok, b"max_batch"),
        "layout 2": (b.image_descs(st.descs), 1, 2, ok, b"layout"),
        "filter 2": (b.image_descs(st.descs), 1, 0, b.ResizeCrop(256, 2), b"filter"),
        "resize_short 223": (b.image_descs(st.descs), 1, 0, b.resize_crop(223), b"resize_short"),
        "resize_short 897": (b.image_descs(st.descs), 1, 0, b.resize_crop(897), b"resize_short"),
        "row_stride": (b.image_descs([(ptr, h, w, w * 3 - 1)]), 1, 0, ok, b"row_stride"),
        "width 16385": (b.image_descs([(ptr, h, 16385, 16385 * 3)]), 1, 0, ok, b"16384"),
        "NULL data": (b.image_descs([(0, h, w, stride)]), 1, 0, ok, b"NULL"),
    }
    for what, (descs, n, layout, rc, msg) in cases.items():
        assert L.vit_hip_forward_device_u8_resized(b16.ctx, descs, n, layout, C.byref(rc), C.byref(norm), d_log.ptr, None,
                                                   None) == 1, what
        assert msg in L.vh_last_error(), (what, L.vh_last_error())
    # the context still works
    want = _device_u8(pkg, b16, R.resize_crop(R.source_image(700, 100, 120, 3), 256, 224, R.BILINEAR)[None], norm)[0]
    got, _ = _device_resized(pkg, b16, [R.source_image(700, 100, 120, 3)], 256, "bilinear", norm)
    assert np.array_equal(got, want)
