"""The image ingest path away from 3 channels, patch 14 / 16 and 224 / 384 px crops.

1. Resize + centre crop: every instantiation resize_crop_kernel<JN, R, LAYOUT> (csrc/resize.hip) byte for byte against
   tests/resize_ref.py, selected through tiny contexts' (in_chans, img_size); the case list's coverage of JN, of the band
   heights with a ragged last band and of multi-chunk bands is computed from the kernel's constants, not claimed.
2. Patch embedding at op level: every producer (fp32 rows direct and gathered, three-part and one-part planes, the MX
   first-operand form, 8-bit HWC / CHW, the 8-bit expansion) at 1, 2, 4 and 5 channels and patches 4, 8, 12, 14, 16
   against the port's conv loop with the same bounds.
3. Whole tiny models at those channel counts in every precision against the port, with the 8-bit and resized entry
   points bit-identical to the fp32 one."""
import ctypes as C

import numpy as np
import pytest

import mx_ref
import resize_ref as R
from ingest_common import (ACC_REGS, HBUF_BYTES, MAX_JN, RESIZE_CASES, THREADS, Staged, band_input_rows, resize_band_rows,
                           resize_chunk_rows, resize_constants_in_source, resize_jn, tiny_config, tiny_resize_context)
from test_gpu_fold import _act_buf
from test_gpu_p3 import OP_TOL, _bf16_rne, _dev, _launch, _planes1_to_f32
from test_gpu_u8_input import _as_layout, _check_both_layouts, _device_u8, _normalised

gpu = pytest.mark.gpu

ENV = ("VIT_HIP_P3", "VIT_HIP_GEMM_FP32", "VIT_HIP_ATTN", "VIT_HIP_LN_FOLD", "VIT_HIP_LAST_LAYER", "VIT_HIP_PRECISION")
# four channels that all differ in scale and in bias: a kernel that picks another channel's pair gives other values
MEAN4, STD4 = (0.485, 0.456, 0.406, 0.31), (0.229, 0.224, 0.225, 0.27)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)


# ---- 1. resize + centre crop ------------------------------------------------------------------------------------------

# the instantiations: (in_chans, img_size) in the order of JN; RESIZE_CASES also holds the Pillow fixture's other contexts
INSTANTIATIONS = [(1, 40), (2, 168), (4, 168), (4, 224), (3, 384), (4, 350), (4, 392), (4, 476), (4, 518), (4, 602), (4, 658),
                  (4, 714), (4, 768)]


def _downscale_factor(chans, crop):
    """the whole-number downscale, at least 4, at which a band's input rows exceed one LDS chunk: a band of R rows reads
    more than R x scale input rows"""
    return max(4, -(-(resize_chunk_rows(chans, crop) + 1) // resize_band_rows(resize_jn(chans, crop))))


def _instantiation_sources(chans, crop, seed):
    """an upscale, an identity-sized source, a downscale of at least 4 x on both axes and a 1 x N or N x 1 source"""
    side = _downscale_factor(chans, crop) * crop + 3
    line = (1, 3 * crop + 1) if (crop // 2) % 2 else (2 * crop + 5, 1)
    shapes = [(crop // 3 + 1, crop // 2 + 3), (crop, crop), (side, side), line]
    return [R.source_image(seed + i, h, w, chans) for i, (h, w) in enumerate(shapes)]


def test_resize_case_list_reaches_every_instantiation():
    """Coverage, from the kernel's own launch arithmetic: every JN in 1..MAX_JN; every band height with a ragged last band;
    tail lanes (crop x chans no multiple of THREADS) and the exact multiple at JN = MAX_JN; all of 1 to 4 channels; a band
    of the downscale source that takes several LDS chunks, in every instantiation."""
    assert resize_constants_in_source() == (THREADS, HBUF_BYTES, ACC_REGS, MAX_JN)
    assert set(INSTANTIATIONS) <= set(RESIZE_CASES)
    jns = {resize_jn(c, s) for c, s in INSTANTIATIONS}
    assert jns == set(range(1, MAX_JN + 1))
    all_r = {resize_band_rows(jn) for jn in range(1, MAX_JN + 1)}
    assert all_r == {16, 12, 9, 8, 6, 5, 4}
    ragged_r = {resize_band_rows(resize_jn(c, s)) for c, s in INSTANTIATIONS if s % resize_band_rows(resize_jn(c, s))}
    assert ragged_r == all_r
    assert any((c * s) % THREADS for c, s in INSTANTIATIONS)
    assert any((c * s) % THREADS == 0 and resize_jn(c, s) == MAX_JN for c, s in INSTANTIATIONS)
    assert {c for c, _ in INSTANTIATIONS} == {1, 2, 3, 4}
    assert max(c * s for c, s in INSTANTIATIONS) == MAX_JN * THREADS
    assert min(resize_chunk_rows(c, s) for c, s in INSTANTIATIONS) == HBUF_BYTES // (MAX_JN * THREADS) == 10
    for c, s in INSTANTIATIONS:
        side = _downscale_factor(c, s) * s + 3
        assert side >= 4 * s and side <= 16384
        for f in (R.BILINEAR, R.BICUBIC):
            rows = band_input_rows(side, s, s, f, resize_band_rows(resize_jn(c, s)))
            assert rows > resize_chunk_rows(c, s), (c, s, f, rows)


@gpu
@pytest.mark.parametrize("f", ["bilinear", "bicubic"])
@pytest.mark.parametrize("chans,crop", INSTANTIATIONS, ids=[f"{c}x{s}" for c, s in INSTANTIATIONS])
def test_resize_crop_of_every_instantiation_equals_the_reference(pkg, device, chans, crop, f):
    images = _instantiation_sources(chans, crop, 1000 + 10 * crop + chans)
    want = [R.resize_crop(img, crop, crop, R.FILTERS[f]) for img in images]
    m = tiny_resize_context(pkg, chans, crop)
    try:
        for layout in ("hwc", "chw"):
            st = Staged(pkg, images, layout)
            out = pkg.DeviceBuffer(len(images) * crop * crop * chans, dtype=np.uint8)
            m.resize_crop_u8(st.descs, crop, out.ptr, filter=f, layout=layout)
            m.sync()
            got = out.to_numpy((len(images), crop, crop, chans))
            for i, img in enumerate(images):
                assert np.array_equal(got[i], want[i]), \
                    f"{layout} source {img.shape[:2]}: {int((got[i] != want[i]).sum())} bytes differ, first rows " \
                    f"{np.unique(np.nonzero(got[i] != want[i])[0])[:8]}"
    finally:
        m.close()


@gpu
def test_resize_refuses_crop_rows_above_3072_bytes(pkg, device):
    """4 channels at 770 px: one step past JN = 12.  The context exists (fp32 and 8-bit crops run on it); the resize forms
    return 1 with a message and launch nothing."""
    L, b = pkg.lib(), pkg.binding
    cfg = tiny_config(pkg, 4, 770, 55)
    m = pkg.ViTHip(cfg, pkg.synth_weights(cfg, 9), device=0, max_batch=1)
    try:
        st = Staged(pkg, [R.source_image(7, 80, 90, 4)], "hwc")
        out = pkg.DeviceBuffer(770 * 770 * 4, dtype=np.uint8)
        rc, norm = b.resize_crop(770), pkg.pixel_norm(MEAN4, STD4)
        assert L.vit_hip_resize_crop_u8(m.ctx, b.image_descs(st.descs), 1, 0, C.byref(rc), out.ptr, None) == 1
        assert b"vit_hip_resize_crop_u8" in L.vh_last_error() and b"3072" in L.vh_last_error(), L.vh_last_error()
        d_log = pkg.DeviceBuffer(cfg.num_classes)
        assert L.vit_hip_forward_device_u8_resized(m.ctx, b.image_descs(st.descs), 1, 0, C.byref(rc), C.byref(norm), d_log.ptr, None,
                                                   None) == 1
        assert b"3072" in L.vh_last_error(), L.vh_last_error()
        assert L.vh_launch_resize_crop_u8(None, out.ptr, 1, 4, 0, 0, 770, out.ptr, 1 << 20, out.ptr) == 1   # refused before any use
        assert b"3072" in L.vh_last_error(), L.vh_last_error()
        m.sync()
    finally:
        m.close()


# ---- 2. patch embedding at op level -------------------------------------------------------------------------------------

# (C, img, patch, n images): the smallest geometry that reaches each branch.  n x grid^2 > 128 at 4 x 32 / 8 (144 rows: a
# second, ragged 128-row tile)
GEOMETRIES = {
    "C1 img32 p16": (1, 32, 16, 3),      # one channel, the 8-pixel fast paths; K = 256
    "C2 img28 p14": (2, 28, 14, 3),      # byte-wise / gathered paths; K = 392, padded
    "C4 img32 p8": (4, 32, 8, 9),        # hwc_row8<4>; patch 8; two row tiles
    "C2 img48 p12": (2, 48, 12, 3),      # the fp32 direct path with patch % 8 != 0; the planes producers' per-element path
    "C1 img16 p4": (1, 16, 4, 3),        # K = 16: below one K step, the operand is nearly all padding
    "C5 img32 p16": (5, 32, 16, 3),      # fp32 sources only; K = 1280
    "C1 img28 p14": (1, 28, 14, 3),      # 784-byte images
    "C2 img16 p8": (2, 16, 8, 3),        # hwc_row8<2>: the other two 2-channel geometries take the byte-wise path
}
E_OP = 128


def _port_for(chans, img, patch, embed=E_OP):
    from oracle.oracle import Oracle
    orc = Oracle("vit_b_16")
    c = orc.cfg
    c.img_size, c.patch_size, c.in_chans, c.embed_dim, c.num_heads, c.mlp_hidden = img, patch, chans, embed, embed // 64, 2 * embed
    return orc


def _op_inputs(pkg, name):
    chans, img, patch, n = GEOMETRIES[name]
    orc = _port_for(chans, img, patch)
    cfg = tiny_config(pkg, chans, img, patch)
    W = [orc.synth_fill(orc.tensor_size(i), 60 + i, 0.05, 0.0) for i in range(4)]
    assert W[1].size == E_OP * chans * patch * patch and W[3].size == ((img // patch) ** 2 + 1) * E_OP
    imgs = pkg.synth_images(cfg, 20, n)
    return orc, cfg, W, imgs


def _port_tokens(orc, image, W, rounded=False):
    if rounded:
        return orc.tokens_from_conv(orc.conv2d(_bf16_rne(image), _bf16_rne(W[1]), W[2]), W[0], W[3])
    return orc.tokens_from_conv(orc.conv2d(image, W[1], W[2]), W[0], W[3])


def _fp32_rows_tokens(pkg, d, n, chans, img, patch):
    """vh_launch_patch_embed_ws on device operands d = (images, conv_w, conv_b, cls, pos)"""
    L = pkg.lib()
    T = (img // patch) ** 2 + 1
    ws = L.vh_patch_embed_workspace(n, chans, img, patch, E_OP)
    d_ws, d_tok = pkg.DeviceBuffer(max(ws // 4, 4)), pkg.DeviceBuffer(n * T * E_OP)
    _launch(pkg, "vh_launch_patch_embed_ws", None, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, d_tok.ptr, n, chans, img, patch,
            E_OP, d_ws.ptr, ws)
    return d_tok.to_numpy((n, T, E_OP)), ws


def _planes_tokens(pkg, d, n, chans, img, patch, parts):
    """vh_launch_patch_embed_planes (parts 1) / _planes3 (parts 3) on fp32 device images"""
    L = pkg.lib()
    T, Kp = (img // patch) ** 2 + 1, L.vh_patch_planes_k(chans, patch)
    d_wp = pkg.DeviceBuffer(E_OP * Kp * 2 * parts // 4)
    _launch(pkg, "vh_launch_conv_weight_planes_parts", None, d[1].ptr, d_wp.ptr, E_OP, chans, patch, parts)
    need = n * (T - 1) * Kp * 2 * parts
    d_ws, d_tok = pkg.DeviceBuffer(need // 4), pkg.DeviceBuffer(n * T * E_OP)
    name = "vh_launch_patch_embed_planes3" if parts == 3 else "vh_launch_patch_embed_planes"
    assert getattr(L, name)(None, d[0].ptr, d_wp.ptr, d[2].ptr, d[3].ptr, d[4].ptr, d_tok.ptr, n, chans, img, patch, E_OP, d_ws.ptr,
                            need - 16) != 0          # workspace too small
    _launch(pkg, name, None, d[0].ptr, d_wp.ptr, d[2].ptr, d[3].ptr, d[4].ptr, d_tok.ptr, n, chans, img, patch, E_OP, d_ws.ptr, need)
    return d_tok.to_numpy((n, T, E_OP)), d_wp, d_ws, need


@gpu
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_patch_embed_on_fp32_rows_and_three_part_planes_vs_port(pkg, device, name):
    """vh_launch_patch_embed[_ws] (im2row on load where patch % 4 == 0, K % 32 == 0 and img % 4 == 0; gathered, zero-padded
    rows elsewhere) and vh_launch_patch_embed_planes3, each against the port's conv loop at the fp32 operator tolerance; the
    two against each other bit for bit, as at 3 channels."""
    chans, img, patch, n = GEOMETRIES[name]
    orc, cfg, W, imgs = _op_inputs(pkg, name)
    L = pkg.lib()
    K = chans * patch * patch
    d = [_dev(pkg, a) for a in (imgs, W[1], W[2], W[0], W[3])]
    got, ws = _fp32_rows_tokens(pkg, d, n, chans, img, patch)
    direct = patch % 4 == 0 and K % 32 == 0 and img % 4 == 0
    assert (ws == 0) == direct
    T = got.shape[1]
    d_tok = pkg.DeviceBuffer(n * T * E_OP)
    if direct:
        _launch(pkg, "vh_launch_patch_embed", None, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, d_tok.ptr, n, chans, img, patch, E_OP)
        assert np.array_equal(d_tok.to_numpy((n, T, E_OP)), got)
    else:      # the form without a workspace refuses what it cannot take
        assert L.vh_launch_patch_embed(None, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, d_tok.ptr, n, chans, img, patch, E_OP) != 0
        assert b"workspace" in L.vh_last_error()
    got3, _, _, _ = _planes_tokens(pkg, d, n, chans, img, patch, 3)
    for i in range(n):
        want = _port_tokens(orc, imgs[i], W)
        assert np.abs(got[i] - want).max() <= OP_TOL, f"fp32 rows, image {i}: {np.abs(got[i] - want).max():.3e}"
        assert np.abs(got3[i] - want).max() <= OP_TOL, f"three-part planes, image {i}: {np.abs(got3[i] - want).max():.3e}"
    assert np.array_equal(got3, got)


@gpu
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_patch_embed_on_one_part_planes_and_its_operand_forms_vs_port(pkg, device, name):
    """vh_launch_patch_embed_planes against the port on the same bf16-rounded pixels and weights (fp32 operator tolerance);
    the conv weight planes are the rounded weights, zero beyond K = C x patch^2; vh_launch_patch_embed_planes_norm leaves the
    same token rows bit for bit, those rows as bf16 planes or as the MX tensor of the NumPy quantiser, and their partial sums."""
    chans, img, patch, n = GEOMETRIES[name]
    orc, cfg, W, imgs = _op_inputs(pkg, name)
    L = pkg.lib()
    K, Kp = chans * patch * patch, L.vh_patch_planes_k(chans, patch)
    assert Kp >= K and Kp % 64 == 0
    d = [_dev(pkg, a) for a in (imgs, W[1], W[2], W[0], W[3])]
    plain, d_wp, d_ws, need = _planes_tokens(pkg, d, n, chans, img, patch, 1)
    wr = _planes1_to_f32(d_wp, E_OP, Kp)
    assert np.array_equal(wr[:, :K], _bf16_rne(W[1]).reshape(E_OP, K)) and not wr[:, K:].any()
    for i in range(n):
        want = _port_tokens(orc, imgs[i], W, rounded=True)
        assert np.abs(plain[i] - want).max() <= OP_TOL, f"image {i}: {np.abs(plain[i] - want).max():.3e}"
    T = plain.shape[1]
    rows = n * T
    for mx in (False, True):
        d_tok = pkg.DeviceBuffer(rows * E_OP)
        d_op = pkg.DeviceBuffer(rows * E_OP // 4 if mx else (rows * E_OP + 1) // 2)
        d_os = _act_buf(pkg, rows, E_OP) if mx else None
        d_st = pkg.DeviceBuffer((E_OP // 128) * rows * 2)
        _launch(pkg, "vh_launch_patch_embed_planes_norm", None, d[0].ptr, d_wp.ptr, d[2].ptr, d[3].ptr, d[4].ptr, d_tok.ptr, n, chans, img,
                patch, E_OP, d_ws.ptr, need, d_op.ptr, d_os.ptr if mx else None, d_st.ptr)
        x = d_tok.to_numpy((rows, E_OP))
        assert np.array_equal(x, plain.reshape(rows, E_OP))
        if mx:
            qv, qs = mx_ref.quantize(x)
            assert np.array_equal(d_op.to_numpy().view(np.uint8)[:rows * E_OP].reshape(E_OP // 128, rows, 128), qv)
            assert np.array_equal(mx_ref.from_act_layout(d_os.to_numpy().view(np.uint8), rows, E_OP), qs)
        else:
            assert np.array_equal(_planes1_to_f32(d_op, rows, E_OP), _bf16_rne(x))
        st = d_st.to_numpy((E_OP // 128, rows, 2))
        x64 = x.astype(np.float64).reshape(rows, E_OP // 128, 128)
        assert np.abs(st[:, :, 0].T - x64.sum(2)).max() <= 1e-5 * max(1.0, np.abs(x64).sum(2).max())
        assert np.abs(st[:, :, 1].T - (x64 * x64).sum(2)).max() <= 1e-5 * (x64 * x64).sum(2).max()


def _bytes_for(chans, img, n, seed):
    """[n][img][img][C] random bytes; image 0 all 0, image 1 all 255"""
    u = np.random.default_rng(seed).integers(0, 256, size=(n, img, img, chans), dtype=np.uint8)
    u[0], u[1] = 0, 255
    return u


@gpu
@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("name", [g for g in GEOMETRIES if GEOMETRIES[g][0] <= 4])
def test_patch_embed_on_bytes_is_bitwise_the_fp32_source_producer(pkg, device, name, layout):
    """vh_launch_patch_embed_planes_u8 (one-part and three-part planes) and vh_launch_expand_u8 followed by the fp32-rows
    producer, against the same producers fed (float)u * scale[c] + bias[c] computed on the host in fp32: the same bits.
    Every channel has its own scale and bias."""
    chans, img, patch, n = GEOMETRIES[name]
    orc, cfg, W, _ = _op_inputs(pkg, name)
    L = pkg.lib()
    norm = pkg.pixel_norm(MEAN4[:chans], STD4[:chans])
    assert len({norm.scale[c] for c in range(chans)}) == chans and len({norm.bias[c] for c in range(chans)}) == chans
    u = _bytes_for(chans, img, n, 30 + chans)
    x = _normalised(u, norm)
    assert (img * img * chans) % 16 == 0        # every image of the batch 16-byte aligned: what the launchers ask of the base
    d_u = pkg.DeviceBuffer.from_numpy(_as_layout(u, layout), dtype=np.uint8)
    d = [_dev(pkg, a) for a in (x, W[1], W[2], W[0], W[3])]
    lay = pkg.binding.PIXEL_LAYOUTS[layout]
    T = (img // patch) ** 2 + 1
    for parts in (1, 3):
        want, d_wp, d_ws, need = _planes_tokens(pkg, d, n, chans, img, patch, parts)
        d_tok = pkg.DeviceBuffer(n * T * E_OP)
        _launch(pkg, "vh_launch_patch_embed_planes_u8", None, d_u.ptr, lay, norm.scale, norm.bias, d_wp.ptr, d[2].ptr, d[3].ptr, d[4].ptr,
                d_tok.ptr, n, chans, img, patch, E_OP, d_ws.ptr, need, parts, None, None, None)
        got = d_tok.to_numpy((n, T, E_OP))
        assert np.isfinite(want).all()
        assert np.array_equal(got, want), f"parts {parts}: {int((got != want).sum())} values differ, max {np.abs(got - want).max():.3e}"
    d_x = pkg.DeviceBuffer(x.size)
    _launch(pkg, "vh_launch_expand_u8", None, d_u.ptr, lay, norm.scale, norm.bias, d_x.ptr, n, chans, img)
    assert np.array_equal(d_x.to_numpy(x.shape), x)
    want, _ = _fp32_rows_tokens(pkg, d, n, chans, img, patch)
    got, _ = _fp32_rows_tokens(pkg, [d_x] + d[1:], n, chans, img, patch)
    assert np.array_equal(got, want)
    # and those values are the port's, on the normalised image
    for i in range(n):
        assert np.abs(got[i] - _port_tokens(orc, x[i], W)).max() <= OP_TOL * max(1.0, float(np.abs(x[i]).max())), f"image {i}"


@gpu
def test_byte_producers_refuse_five_channels(pkg, device):
    chans, img, patch, n = GEOMETRIES["C5 img32 p16"]
    L = pkg.lib()
    scale = (C.c_float * 8)(*[0.01] * 8)
    d_u = pkg.DeviceBuffer(n * chans * img * img, dtype=np.uint8)
    d_f = pkg.DeviceBuffer(n * chans * img * img)
    assert L.vh_launch_expand_u8(None, d_u.ptr, 0, scale, scale, d_f.ptr, n, chans, img) != 0
    assert b"vh_launch_expand_u8" in L.vh_last_error() and b"1 to 4 channels" in L.vh_last_error()
    assert L.vh_launch_patch_embed_planes_u8(None, d_u.ptr, 1, scale, scale, d_f.ptr, d_f.ptr, d_f.ptr, d_f.ptr, d_f.ptr, n, chans, img,
                                             patch, E_OP, d_f.ptr, 1 << 20, 1, None, None, None) != 0
    assert b"vh_launch_patch_embed_planes_u8" in L.vh_last_error() and b"1 to 4 channels" in L.vh_last_error()


# ---- 3. whole tiny models ------------------------------------------------------------------------------------------------

MODEL_CONFIGS = {"C1 img32 p16": (1, 32, 16), "C2 img28 p14": (2, 28, 14), "C4 img32 p8": (4, 32, 8), "C5 img32 p16": (5, 32, 16)}
# (precision, environment)
MODEL_MODES = {
    "f32": ("f32", {}),
    "f32_p3_off": ("f32", {"VIT_HIP_P3": "0"}),
    "f32_fp16x2": ("f32_fp16x2", {}),
    "bf16_fold": ("bf16", {"VIT_HIP_LN_FOLD": "1"}),
    "bf16_nofold": ("bf16", {"VIT_HIP_LN_FOLD": "0"}),
    "fp8_fold": ("fp8", {"VIT_HIP_LN_FOLD": "1"}),
    "fp8_nofold": ("fp8", {"VIT_HIP_LN_FOLD": "0"}),
}
E_MODEL, N_MODEL = 256, 5
_port_cache = {}


def _model_reference(pkg, name):
    """(port, config, weights, images, port logits) of one config, computed once"""
    if name not in _port_cache:
        chans, img, patch = MODEL_CONFIGS[name]
        orc = _port_for(chans, img, patch, E_MODEL)
        orc.cfg.depth, orc.cfg.num_classes = 2, 10
        cfg = tiny_config(pkg, chans, img, patch, embed=E_MODEL, depth=2)
        weights = orc.synth_weights(31)
        imgs = np.stack([orc.synth_image(i) for i in range(N_MODEL)])
        want = np.stack([orc.forward(imgs[i], weights)[0] for i in range(N_MODEL)])
        _port_cache[name] = (cfg, weights, imgs, want)
    return _port_cache[name]


def _logit_rel_l2(got, want):
    return float(np.linalg.norm(got - want) / np.linalg.norm(want - want.mean()))


@gpu
@pytest.mark.parametrize("mode", list(MODEL_MODES))
@pytest.mark.parametrize("name", list(MODEL_CONFIGS))
def test_tiny_models_at_other_channel_counts_vs_port(pkg, device, monkeypatch, tmp_path, name, mode):
    """Embed 256, 2 layers, 4 heads of 64, 10 classes at 1, 2, 4 and 5 channels against the port with the same loop bounds:
    fp32 family within 1e-4 and the same arg-max; bf16 within 4e-2 and fp8 within 0.15 relative L2, the bounds of
    test_a_tiny_custom_config_in_every_precision_vs_port (docs/LABBOOK.md holds the measured errors at these shapes).
    Batch-position independence and the repacked-weights round trip bit for bit (the conv planes' padded K depends on C).
    Up to 4 channels: the 8-bit entry point in both layouts and the resized one are bitwise the fp32 entry point.
    5 channels: those two refuse and the context goes on serving fp32 images."""
    precision, env = MODEL_MODES[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    chans, img, patch = MODEL_CONFIGS[name]
    cfg, weights, imgs, want = _model_reference(pkg, name)
    L, b = pkg.lib(), pkg.binding
    m = pkg.ViTHip(cfg, weights, device=0, max_batch=N_MODEL, precision=precision)
    try:
        got, probs = m.forward(imgs)
        again, _ = m.forward(imgs[[3, 0]])
        path = tmp_path / "tiny.planes"
        m.export_planes(path)
        small = pkg.ViTHip.from_planes(path, device=0, max_batch=2)
        try:
            assert (small.cfg.in_chans, small.cfg.img_size, small.cfg.patch_size) == (chans, img, patch)
            chunked, _ = small.forward(imgs)
        finally:
            small.close()
        err = float(np.abs(got - want).max())
        rel = max(_logit_rel_l2(got[i], want[i]) for i in range(N_MODEL))
        print(f"\ningest shapes ({name}), {mode}: max |dlogit| {err:.3e}, relative L2 {rel:.4f}")
        assert np.isfinite(got).all() and np.abs(probs.sum(axis=1) - 1.0).max() < 1e-5
        assert np.array_equal(again, got[[3, 0]])
        assert np.array_equal(chunked, got)
        if precision in ("f32", "f32_fp16x2"):
            assert err <= 1e-4 and np.array_equal(got.argmax(1), want.argmax(1))
        elif precision == "bf16":
            assert err <= 4e-2
        else:
            assert rel <= 0.15
        norm = pkg.pixel_norm(MEAN4[:min(chans, 4)], STD4[:min(chans, 4)])
        nc = cfg.num_classes
        if chans <= 4:
            _check_both_layouts(pkg, m, _bytes_for(chans, img, N_MODEL, 40 + chans), norm, f"{name} {mode}")
            shapes = [(img // 2 + 1, img + 3), (img, img), (4 * img + 1, 5 * img), (1, 90)]
            sources = [R.source_image(50 + i, h, w, chans) for i, (h, w) in enumerate(shapes)]
            for f, layout in (("bilinear", "hwc"), ("bicubic", "chw")):
                crops = np.stack([R.resize_crop(s, img, img, R.FILTERS[f]) for s in sources])
                want_l, want_p = _device_u8(pkg, m, crops, "hwc", norm)
                st = Staged(pkg, sources, layout)
                d_log, d_prob = pkg.DeviceBuffer(len(sources) * nc), pkg.DeviceBuffer(len(sources) * nc)
                m.forward_device_u8_resized(st.descs, img, norm, filter=f, layout=layout, d_logits=d_log.ptr, d_probs=d_prob.ptr)
                m.sync()
                assert np.isfinite(want_l).all()
                assert np.array_equal(d_log.to_numpy((len(sources), nc)), want_l), f"{f} {layout}"
                assert np.array_equal(d_prob.to_numpy((len(sources), nc)), want_p), f"{f} {layout}"
        else:
            u = _bytes_for(chans, img, 2, 45)
            d_u = pkg.DeviceBuffer.from_numpy(u, dtype=np.uint8)
            d_log = pkg.DeviceBuffer(N_MODEL * nc)
            assert L.vit_hip_forward_device_u8(m.ctx, d_u.ptr, 2, 0, C.byref(norm), d_log.ptr, None, None) == 1
            assert b"at most 4 channels" in L.vh_last_error()
            rc = b.resize_crop(img)
            descs = b.image_descs([(d_u.ptr, img, img, img * chans)])
            assert L.vit_hip_forward_device_u8_resized(m.ctx, descs, 1, 0, C.byref(rc), C.byref(norm), d_log.ptr, None, None) == 1
            assert b"at most 4 channels" in L.vh_last_error()
            host = (b.ImageU8 * 1)(b.ImageU8(u.ctypes.data, img, img, img * chans))
            out = np.empty((1, nc), dtype=np.float32)
            assert L.vit_hip_forward_u8(m.ctx, u.ctypes.data_as(C.POINTER(C.c_ubyte)), 2, 0, C.byref(norm), b.fptr(out), None) == 1
            assert L.vit_hip_forward_u8_resized(m.ctx, host, 1, 0, C.byref(rc), C.byref(norm), b.fptr(out), None) == 1
            after, _ = m.forward(imgs)
            assert np.array_equal(after, got)
    finally:
        m.close()
