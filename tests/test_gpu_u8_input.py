"""The 8-bit input path (vit_hip_forward_device_u8, vit_hip_forward_u8): logits and probabilities bit-identical to the fp32
entry points fed the same images normalised on the host, in every precision and operand path, in both layouts.

The reference image is always x = u.astype(float32) * scale[c] + bias[c] in NumPy float32 (a product and a sum, each rounded:
no fused multiply-add), with (scale, bias) from vit_pixel_norm_from_mean_std; it goes through the existing fp32 entry point
of the same context."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ENV = ("VIT_HIP_P3", "VIT_HIP_GEMM_FP32", "VIT_HIP_ATTN", "VIT_HIP_LN_FOLD", "VIT_HIP_LAST_LAYER", "VIT_HIP_PRECISION")
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
HALF = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)


def _u8_images(cfg, n, seed):
    """[n][H][W][C] random bytes; image 0 all 0, image 1 all 255 (the ends of the range)"""
    u = np.random.default_rng(seed).integers(0, 256, size=(n, cfg.img_size, cfg.img_size, cfg.in_chans), dtype=np.uint8)
    u[0], u[1] = 0, 255
    return u


def _normalised(u_hwc, norm):
    """the host-side fp32 normalisation, [n][C][H][W]"""
    C_ = u_hwc.shape[-1]
    scale = np.array(norm.scale[:C_], dtype=np.float32)
    bias = np.array(norm.bias[:C_], dtype=np.float32)
    x = u_hwc.astype(np.float32) * scale
    x = x + bias
    assert x.dtype == np.float32
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def _as_layout(u_hwc, layout):
    return u_hwc if layout == "hwc" else np.ascontiguousarray(u_hwc.transpose(0, 3, 1, 2))


def _device_fp32(pkg, m, x):
    n, nc = x.shape[0], m.cfg.num_classes
    d_img = pkg.DeviceBuffer.from_numpy(x)
    d_log, d_prob = pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)
    m.forward_device(d_img.ptr, n, d_log.ptr, d_prob.ptr, None)
    m.sync()
    return d_log.to_numpy((n, nc)), d_prob.to_numpy((n, nc))


def _device_u8(pkg, m, u, layout, norm):
    n, nc = u.shape[0], m.cfg.num_classes
    d_img = pkg.DeviceBuffer.from_numpy(_as_layout(u, layout), dtype=np.uint8)
    d_log, d_prob = pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)
    m.forward_device_u8(d_img.ptr, n, norm, layout, d_log.ptr, d_prob.ptr, None)
    m.sync()
    return d_log.to_numpy((n, nc)), d_prob.to_numpy((n, nc))


def _check_both_layouts(pkg, m, u, norm, what):
    want_l, want_p = _device_fp32(pkg, m, _normalised(u, norm))
    assert np.isfinite(want_l).all()
    for layout in ("hwc", "chw"):
        got_l, got_p = _device_u8(pkg, m, u, layout, norm)
        assert np.array_equal(got_l, want_l), f"{what} {layout}: max |dlogit| {np.abs(got_l - want_l).max():.3e}"
        assert np.array_equal(got_p, want_p), f"{what} {layout}: probabilities differ"


# (precision, env) -- every operand path of the patch embedding: three-part planes (F32), the fold on them, one-part planes
# with and without the fold (BF16_GEMM), MX behind the fold (FP8_GEMM), and the fp32-rows paths that expand first
MODES = {
    "f32": ("f32", {}),
    "f32_fold": ("f32", {"VIT_HIP_LN_FOLD": "1"}),
    "bf16_fold": ("bf16", {}),
    "bf16_nofold": ("bf16", {"VIT_HIP_LN_FOLD": "0"}),
    "fp8": ("fp8", {}),
    "f32_fp16x2": ("f32_fp16x2", {}),
    "f32_p3_off": ("f32", {"VIT_HIP_P3": "0"}),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_u8_is_bitwise_the_fp32_path_on_b16(pkg, device, weights, monkeypatch, mode):
    precision, env = MODES[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = pkg.preset("vit_b_16")
    m = pkg.ViTHip(cfg, weights, device=0, max_batch=16, precision=precision)
    try:
        norm = pkg.pixel_norm(*(HALF if mode == "bf16_nofold" else IMAGENET))
        _check_both_layouts(pkg, m, _u8_images(cfg, 13, 1), norm, mode)
    finally:
        m.close()


@pytest.mark.parametrize("precision,env", [("f32", {}), ("f32", {"VIT_HIP_P3": "0"}), ("bf16", {}), ("f32_fp16x2", {})],
                         ids=["f32", "f32_p3_off", "bf16", "f32_fp16x2"])
def test_u8_tiny_patch14_unaligned_images(pkg, device, monkeypatch, precision, env):
    """patch 14 at 42 px: T = 10, K = 588 padded, HWC images of 5292 bytes (every other image base off 8-byte alignment);
    on the fp32-rows paths the Q|K|V buffer is smaller than max_batch fp32 images and is grown for the expansion"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = pkg.preset("vit_b_16")
    cfg.img_size, cfg.patch_size, cfg.in_chans, cfg.num_classes = 42, 14, 3, 10
    cfg.embed_dim, cfg.depth, cfg.num_heads, cfg.mlp_hidden = 128, 2, 2, 256
    assert pkg.binding.tokens(cfg) == 10 and 42 * 42 * 3 == 5292
    m = pkg.ViTHip(cfg, pkg.synth_weights(cfg, 5), device=0, max_batch=7, precision=precision)
    try:
        _check_both_layouts(pkg, m, _u8_images(cfg, 7, 2), pkg.pixel_norm(*IMAGENET), f"tiny {precision}")
    finally:
        m.close()


def test_u8_b16_384_long_attention(pkg, device):
    cfg = pkg.preset("vit_b_16_384")
    assert pkg.binding.tokens(cfg) == 577
    m = pkg.ViTHip(cfg, pkg.synth_weights(cfg, 0), device=0, max_batch=2)
    try:
        _check_both_layouts(pkg, m, _u8_images(cfg, 2, 3), pkg.pixel_norm(*IMAGENET), "b16_384")
    finally:
        m.close()


@pytest.fixture(scope="module")
def b16(pkg, device, weights):
    with pytest.MonkeyPatch.context() as mp:   # created before the per-test environment cleanup runs
        for var in ENV:
            mp.delenv(var, raising=False)
        m = pkg.ViTHip(pkg.preset("vit_b_16"), weights, device=0, max_batch=16)
    yield m
    m.close()


def test_u8_host_form_pipelined_chunks(pkg, b16):
    """n = 2 * max_batch + 3: three chunks through both staging slots; logits and probs each NULL in turn"""
    cfg, norm = b16.cfg, pkg.pixel_norm(*IMAGENET)
    u = _u8_images(cfg, 35, 4)
    want_l, want_p = b16.forward(_normalised(u, norm))
    for layout in ("hwc", "chw"):
        got_l, got_p = b16.forward_u8(_as_layout(u, layout), *IMAGENET, layout=layout)
        assert np.array_equal(got_l, want_l) and np.array_equal(got_p, want_p), layout
    only_l, none_p = b16.forward_u8(u, *IMAGENET, probs=False)
    assert none_p is None and np.array_equal(only_l, want_l)
    none_l, only_p = b16.forward_u8(u, *IMAGENET, logits=False)
    assert none_l is None and np.array_equal(only_p, want_p)


def test_u8_batch_position_independence(pkg, b16):
    norm = pkg.pixel_norm(*IMAGENET)
    u = _u8_images(b16.cfg, 13, 5)
    u[11] = u[0] = _u8_images(b16.cfg, 3, 6)[2]
    for layout in ("hwc", "chw"):
        got, _ = _device_u8(pkg, b16, u, layout, norm)
        assert np.array_equal(got[0], got[11]), layout


def test_u8_f32_tied_to_the_port(pkg, b16, oracle, weights):
    norm = pkg.pixel_norm(*IMAGENET)
    u = _u8_images(b16.cfg, 4, 7)
    got, _ = _device_u8(pkg, b16, u, "hwc", norm)
    x = _normalised(u, norm)
    for i in range(4):
        want = oracle.forward(x[i], weights)[0]
        err = float(np.abs(got[i] - want).max())
        assert err < 1e-4, f"image {i}: max |dlogit| {err:.3e} vs the port"


def test_u8_refusals_on_a_live_context(pkg, b16):
    L = pkg.lib()
    cfg, norm = b16.cfg, pkg.pixel_norm(*IMAGENET)
    n, nc = 3, cfg.num_classes
    u = _u8_images(cfg, n, 8)
    want, _ = _device_fp32(pkg, b16, _normalised(u, norm))
    d_img = pkg.DeviceBuffer(u.nbytes + 64, dtype=np.uint8)
    assert L.vh_h2d(d_img.ptr, u.ctypes.data_as(C.c_void_p), u.nbytes, None) == 0
    d_log = pkg.DeviceBuffer(b16.max_batch * nc)
    refusals = {
        "n > max_batch": (d_img.ptr.value, b16.max_batch + 1, 0, b"max_batch"),
        "layout 2": (d_img.ptr.value, n, 2, b"layout"),
        "pointer + 1 byte": (d_img.ptr.value + 1, n, 0, b"aligned"),
    }
    for what, (ptr, count, layout, msg) in refusals.items():
        rc = L.vit_hip_forward_device_u8(b16.ctx, ptr, count, layout, C.byref(norm), d_log.ptr, None, None)
        assert rc == 1 and msg in L.vh_last_error(), what
        b16.forward_device_u8(d_img.ptr, n, norm, "hwc", d_log.ptr, None)
        b16.sync()
        assert np.array_equal(d_log.to_numpy((b16.max_batch, nc))[:n], want), f"forward after refusing {what}"
    assert L.vit_hip_forward_u8(b16.ctx, u.ctypes.data_as(C.POINTER(C.c_ubyte)), n, 2, C.byref(norm), None, None) == 1
