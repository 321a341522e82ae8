"""Non-square inputs on the GPU: contexts of img_size rows by img_width columns.

The independent check is a rearrangement: a gh x gw grid with gh * gw = s * s has the tokens of an s x s grid, so a rectangular
context fed image R and a square one fed S -- patch q of S (row-major in its grid) being patch q of R -- from the same tensors
run the same GEMM rows, position rows and tile classes, and every output must be EQUAL, bit for bit.  Derived contexts
(vit_hip_create_at_size) are held against contexts created natively at grids whose count is no square; the dense head and the
NCHW token map are held against tests/dense_ref.py on a 4 x 9 grid.

The tiny model is embed_dim 128, 2 heads of 64, depth 2, mlp_hidden 256, 10 classes.  FP8_GEMM refuses embed_dim % 256 != 0,
so that mode runs the same model at embed_dim 256 with 4 heads of 64.  n = 3 images, so the image stride C * H * W counts."""
import ctypes as C
import os
from contextlib import contextmanager

import numpy as np
import pytest

import dense_ref as dr
import pos_resample_ref as pr

pytestmark = pytest.mark.gpu

N = 3
PRECISIONS = ["f32", "bf16", "fp8", "f32_fp16x2"]
SWITCHES = {"p3off": {"VIT_HIP_P3": "0"}, "native": {"VIT_HIP_GEMM_FP32": "native"}}


def config(pkg, precision, h, w, patch, chans):
    wide = precision == "fp8"
    return pkg.binding.VitConfig(img_size=h, patch_size=patch, in_chans=chans, num_classes=10, embed_dim=256 if wide else 128, depth=2,
                                 num_heads=4 if wide else 2, mlp_hidden=256, eps=1e-6, img_width=w)


@contextmanager
def switches(env):
    """the $VIT_HIP_* switches of a context, which are read when it is created"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def to_square(R, grid, s, p):
    """R [n][C][gh p][gw p] -> S [n][C][s p][s p], patch q of S (row-major) = patch q of R"""
    n, ch = R.shape[:2]
    gh, gw = grid
    patches = R.reshape(n, ch, gh, p, gw, p).transpose(0, 2, 4, 1, 3, 5).reshape(n, s, s, ch, p, p)
    return np.ascontiguousarray(patches.transpose(0, 3, 1, 4, 2, 5).reshape(n, ch, s * p, s * p))


def device_outputs(pkg, model, images, rows):
    """forward_device of fp32 images with features (tokens, NLC), attention mean, rollout, top-k and a gallery armed"""
    b = pkg.binding
    n, nc, T, E, mb = images.shape[0], model.cfg.num_classes, model.tokens, model.cfg.embed_dim, model.max_batch
    d_img = pkg.DeviceBuffer.from_numpy(images)
    d_l, d_p = pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)
    d_tok, d_cls = pkg.DeviceBuffer(mb * (T - 1) * E), pkg.DeviceBuffer(mb * E)
    d_mean, d_roll = pkg.DeviceBuffer(mb * T), pkg.DeviceBuffer(mb * T)
    d_lab, d_idx = pkg.DeviceBuffer(mb * 3, np.int32), pkg.DeviceBuffer(mb * 3, np.int32)
    model.set_features(b.FeatureSpec((-1,), True), cls=d_cls, tokens=d_tok)
    model.set_attention(b.AttentionSpec((0,)), mean=d_mean)
    model.set_rollout(b.RolloutSpec(0), rollout=d_roll)
    model.set_topk(b.TopKSpec(3, "logits"), labels=d_lab)
    model.set_gallery(b.GallerySpec(3, "pooled"), rows, indices=d_idx)
    try:
        model.forward_device(d_img.ptr, n, d_l.ptr, d_p.ptr)
        model.sync()
    finally:
        for disarm in (model.set_features, model.set_attention, model.set_rollout, model.set_topk, model.set_gallery):
            disarm(None)
    return {"logits": d_l.to_numpy((n, nc)), "probs": d_p.to_numpy((n, nc)), "tokens": d_tok.to_numpy((mb, T - 1, E))[:n],
            "cls": d_cls.to_numpy((mb, E))[:n], "mean": d_mean.to_numpy((mb, T))[:n], "rollout": d_roll.to_numpy((mb, T))[:n],
            "topk": d_lab.to_numpy((mb, 3))[:n], "gallery": d_idx.to_numpy((mb, 3))[:n]}


def u8_logits(pkg, model, pixels, layout):
    """the logits of uint8 images [n][C][H][W] in `layout`, through _device_u8 and through _u8; they must agree"""
    n, nc = pixels.shape[0], model.cfg.num_classes
    ch = model.cfg.in_chans
    norm = pkg.pixel_norm([0.45, 0.5, 0.4][:ch], [0.25, 0.2, 0.3][:ch])
    arr = np.ascontiguousarray(pixels.transpose(0, 2, 3, 1) if layout == "hwc" else pixels)
    d_u, d_l = pkg.DeviceBuffer.from_numpy(arr, np.uint8), pkg.DeviceBuffer(n * nc)
    model.forward_device_u8(d_u.ptr, n, norm, layout, d_l.ptr, None)
    model.sync()
    dev = d_l.to_numpy((n, nc))
    host, _ = model.forward_u8(arr, norm, None, layout, probs=False)
    assert same(dev, host), f"u8 {layout}: the device and the host form differ"
    return dev


# (grid, square side, patch, channels): what each exercises is said in the issue's list
IDENTITY = [((2, 8), 4, 16, 3), ((8, 2), 4, 16, 3), ((1, 16), 4, 16, 3), ((16, 1), 4, 16, 3),     # direct gather, vector loads
            ((2, 8), 4, 4, 3), ((8, 2), 4, 4, 3), ((1, 16), 4, 4, 3), ((16, 1), 4, 4, 3),         # K = 48: workspace, scalar loads
            ((4, 9), 6, 14, 3), ((9, 4), 6, 14, 3),                                               # K = 588, padded
            ((2, 8), 4, 16, 1), ((8, 2), 4, 4, 1),                                                # one channel
            ((9, 16), 12, 8, 3),                                                                  # T = 145, resident attention
            ((12, 27), 18, 4, 3),                                                                 # T = 325, streaming
            ((16, 36), 24, 4, 3)]                                                                 # T = 577, attention_long.hip
MODES = [(p, None) for p in PRECISIONS] + [("f32", "p3off"), ("f32", "native")]
# above 512 tokens only the planes paths run (F32 on planes, BF16_GEMM, FP8_GEMM): the other modes are refused at creation
IDENTITY_CASES = [(*case, p, sw) for case in IDENTITY for p, sw in MODES
                  if case[0][0] * case[0][1] + 1 <= 512 or (p != "f32_fp16x2" and sw is None)]


@pytest.mark.parametrize("grid,s,patch,chans,precision,switch", IDENTITY_CASES,
                         ids=[f"{g[0]}x{g[1]}-p{p}-c{c}-{m}" + (f"-{sw}" if sw else "") for g, _, p, c, m, sw in IDENTITY_CASES])
def test_rearrangement_identity(pkg, device, grid, s, patch, chans, precision, switch):
    gh, gw = grid
    T = gh * gw + 1
    assert gh * gw == s * s
    rect_cfg, sq_cfg = config(pkg, precision, gh * patch, gw * patch, patch, chans), config(pkg, precision, s * patch, 0, patch, chans)
    weights = pkg.synth_weights(sq_cfg, 7)
    assert weights[3].shape[0] == (s * s + 1) * sq_cfg.embed_dim == pkg.synth_weights(rect_cfg, 7)[3].shape[0]
    with switches(SWITCHES[switch] if switch else {}):
        rect = pkg.ViTHip(rect_cfg, weights, device=0, max_batch=N + 1, precision=precision)
        square = pkg.ViTHip(sq_cfg, weights, device=0, max_batch=N + 1, precision=precision)
    try:
        assert rect.tokens == square.tokens == T and (rect.cfg.img_size, rect.cfg.width) == (gh * patch, gw * patch)
        rng = np.random.default_rng(gh * 100 + gw + patch)
        R = rng.uniform(-2, 2, rect_cfg.image_shape(N)).astype(np.float32)
        S = to_square(R, grid, s, patch)
        rows = rng.standard_normal((40, rect_cfg.embed_dim)).astype(np.float32)
        got, want = device_outputs(pkg, rect, R, rows), device_outputs(pkg, square, S, rows)
        for name in want:
            assert same(got[name], want[name]), f"{name} differs between the {gh} x {gw} and the {s} x {s} context"
        assert np.isfinite(got["logits"]).all() and np.ptp(got["logits"]) > 0
        assert not same(got["logits"][0], got["logits"][1])
        # fp32 host images through the pipeline
        host, _ = rect.forward(R)
        assert same(host, want["logits"])
        # 8-bit pixels, both layouts, device and host forms
        U = rng.integers(0, 256, rect_cfg.image_shape(N), dtype=np.uint8)
        US = to_square(U, grid, s, patch)
        for layout in ("hwc", "chw"):
            assert same(u8_logits(pkg, rect, U, layout), u8_logits(pkg, square, US, layout)), f"u8 {layout}"
    finally:
        rect.close()
        square.close()


# ---- derived equals native, at grids whose count is no square -----------------------------------------------------------

P = 16
DERIVE = [((4, 4), (3, 5)), ((4, 4), (5, 3)), ((4, 4), (1, 6)), ((4, 4), (14, 21)), ((3, 5), (4, 4))]
HOWS = [("bicubic", False), ("bicubic", True), ("bilinear", False), ("bilinear", True)]


def logits_and_features(pkg, model, images):
    b = pkg.binding
    n, nc, T, E, mb = images.shape[0], model.cfg.num_classes, model.tokens, model.cfg.embed_dim, model.max_batch
    d_img, d_l = pkg.DeviceBuffer.from_numpy(images), pkg.DeviceBuffer(n * nc)
    d_tok, d_cls, d_pool = pkg.DeviceBuffer(mb * (T - 1) * E), pkg.DeviceBuffer(mb * E), pkg.DeviceBuffer(mb * E)
    model.set_features(b.FeatureSpec((-1,), True), cls=d_cls, pooled=d_pool, tokens=d_tok)
    try:
        model.forward_device(d_img.ptr, n, d_l.ptr, None)
        model.sync()
    finally:
        model.set_features(None)
    return d_l.to_numpy((n, nc)), d_cls.to_numpy((mb, E))[:n], d_pool.to_numpy((mb, E))[:n], d_tok.to_numpy((mb, T - 1, E))[:n]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("src_grid,dst_grid", DERIVE, ids=[f"{a[0]}x{a[1]}-to-{b[0]}x{b[1]}" for a, b in DERIVE])
def test_derived_equals_native(pkg, device, src_grid, dst_grid, precision):
    src_cfg = config(pkg, precision, src_grid[0] * P, src_grid[1] * P, P, 3)
    weights = pkg.synth_weights(src_cfg, 3)
    E = src_cfg.embed_dim
    pos = weights[3].reshape(-1, E)
    src = pkg.ViTHip(src_cfg, weights, device=0, max_batch=N, precision=precision)
    try:
        for mode, ac in HOWS:
            derived = src.at_size(dst_grid[0] * P, dst_grid[1] * P, mode=mode, align_corners=ac)
            native = None
            try:
                assert derived.cfg.grid == dst_grid and derived.max_batch == N
                assert derived.cfg.img_width == (0 if dst_grid[0] == dst_grid[1] else dst_grid[1] * P)
                got = derived.weight(3).reshape(-1, E)
                want = pr.resample_pos_embed(pos, 1, src_grid, dst_grid, mode, ac)
                err = np.abs(got.astype(np.float64) - want)
                assert (err <= pr.bound(want, pos[1:])).all(), f"{mode} {ac}: pos_embedding off by {err.max():.3e}"
                assert same(got[0], pos[0])
                for i in (0, 1, 2, 4 + 12, 4 + 24 + 3):
                    assert same(derived.weight(i), weights[i])
                native_cfg = config(pkg, precision, dst_grid[0] * P, dst_grid[1] * P, P, 3)
                native_weights = list(weights)
                native_weights[3] = np.ascontiguousarray(got.ravel())
                native = pkg.ViTHip(native_cfg, native_weights, device=0, max_batch=N, precision=precision)
                images = pkg.synth_images(native_cfg, 5, N)
                for a, c in zip(logits_and_features(pkg, derived, images), logits_and_features(pkg, native, images)):
                    assert same(a, c), f"{mode} {ac}: derived and native differ"
            finally:
                derived.close()
                if native is not None:
                    native.close()
    finally:
        src.close()


def test_at_size_square_is_at_resolution(pkg, device):
    cfg = config(pkg, "f32", 48, 80, P, 3)
    src = pkg.ViTHip(cfg, pkg.synth_weights(cfg, 3), device=0, max_batch=N)
    a, c = src.at_size(96, 96), src.at_resolution(96)
    try:
        assert bytes(a.cfg) == bytes(c.cfg) and a.cfg.img_width == 0 and a.cfg.img_size == 96
        assert same(a.weight(3), c.weight(3))
        images = pkg.synth_images(a.cfg, 0, N)
        for x, y in zip(logits_and_features(pkg, a, images), logits_and_features(pkg, c, images)):
            assert same(x, y)
        with pytest.raises(pkg.VitHipError, match="vit_hip_create_at_size failed with status 1: vit_resample_check_hw: img_width=72 must be a positive multiple"):
            src.at_size(96, 72)
        with pytest.raises(pkg.VitHipError, match="vit_resample_check: img_size=72 must be a positive multiple"):
            src.at_resolution(72)
    finally:
        for m in (src, a, c):
            m.close()


# ---- the dense head and the token map on a 4 x 9 grid ------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_dense_head_and_token_map(pkg, device, precision):
    b = pkg.binding
    grid, NL = (4, 9), 5
    cfg = config(pkg, precision, 4 * P, 9 * P, P, 3)
    E, T = cfg.embed_dim, 37
    model = pkg.ViTHip(cfg, pkg.synth_weights(cfg, 11), device=0, max_batch=N, precision=precision)
    try:
        images = pkg.synth_images(cfg, 0, N)
        d_img = pkg.DeviceBuffer.from_numpy(images)
        rng = np.random.default_rng(5)
        W = (rng.standard_normal((NL, E)) / np.sqrt(E)).astype(np.float32)
        bias = (0.1 * rng.standard_normal(NL)).astype(np.float32)
        tok = {}
        for layout in ("nlc", "nchw"):
            d_tok = pkg.DeviceBuffer(N * (T - 1) * E)
            model.set_features(b.FeatureSpec((-1,), True, token_layout=layout), tokens=d_tok)
            model.forward_device(d_img.ptr, N, None, None)
            model.sync()
            model.set_features(None)
            tok[layout] = d_tok.to_numpy()
        nlc = tok["nlc"].reshape(N, T - 1, E)
        assert same(tok["nchw"].reshape(N, E, 4, 9), nlc.transpose(0, 2, 1).reshape(N, E, 4, 9))
        default_labels = None
        for out in ((0, 0), (37, 50)):
            size = (out[0] or cfg.img_size, out[1] or cfg.width)
            assert size == ((64, 144) if out == (0, 0) else out)
            d_lab, d_sc = pkg.DeviceBuffer(N * size[0] * size[1], np.uint8), pkg.DeviceBuffer(N * size[0] * size[1])
            d_pl = pkg.DeviceBuffer(N * (T - 1) * NL)
            model.set_dense(b.DenseSpec(NL, out[0], out[1], -1, True), W, bias, labels=d_lab, scores=d_sc, patch_logits=d_pl)
            try:
                model.forward_device(d_img.ptr, N, None, None)
                model.sync()
            finally:
                model.set_dense(None)
            pl, lab, sc = d_pl.to_numpy((N, T - 1, NL)), d_lab.to_numpy((N, *size)), d_sc.to_numpy((N, *size))
            err = np.abs(pl.astype(np.float64) - dr.logits64(nlc, W, bias))
            assert (err <= (E + 8) * dr.U * dr.absdot(nlc, W, bias)).all(), f"patch logits off by {err.max():.3e}"
            # the labels and scores from those patch logits: dense_ref's check with the identity as the head
            dr.check(pl, np.eye(NL, dtype=np.float32), None, grid, size, lab, sc)
            dr.check(nlc, W, bias, grid, size, lab, sc)
            if out == (0, 0):
                default_labels = lab
        # the host form at the default size: img_size rows by img_width columns
        assert same(model.segment(images, W, bias), default_labels)
    finally:
        model.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------

def test_refusals(pkg, device, tmp_path):
    b, L = pkg.binding, pkg.lib()
    cfg = config(pkg, "f32", 2 * P, 8 * P, P, 3)
    weights = pkg.synth_weights(cfg, 7)
    model = pkg.ViTHip(cfg, weights, device=0, max_batch=N)
    try:
        images = pkg.synth_images(cfg, 0, N)
        before, _ = model.forward(images)
        norm = pkg.pixel_norm([0.5] * 3, [0.25] * 3)
        big = np.zeros((64, 64, 3), np.uint8)
        d_big = pkg.DeviceBuffer.from_numpy(big, np.uint8)
        desc = [(d_big.ptr, 64, 64, 64 * 3)]
        fill = np.full(N * 10, -7.0, np.float32)
        d_l = pkg.DeviceBuffer.from_numpy(fill)
        d_out = pkg.DeviceBuffer.from_numpy(np.full(2 * P * 8 * P * 3, 0xEE, np.uint8), np.uint8)
        box = [(0, (0.0, 0.0, 32.0, 32.0))]
        calls = {"vit_hip_resize_crop_u8": lambda: model.resize_crop_u8(desc, 40, d_out.ptr),
                 "vit_hip_crop_boxes_u8": lambda: model.crop_boxes_u8(desc, box, d_out.ptr),
                 "vit_hip_forward_device_u8_resized": lambda: model.forward_device_u8_resized(desc, 40, norm, d_logits=d_l.ptr),
                 "vit_hip_forward_device_u8_boxes": lambda: model.forward_device_u8_boxes(desc, box, norm, d_logits=d_l.ptr),
                 "vit_hip_forward_u8_resized": lambda: model.forward_u8_resized([big], 40, mean=norm),
                 "vit_hip_forward_u8_boxes": lambda: model.forward_u8_boxes([big], box, mean=norm),
                 "vit_hip_export_planes": lambda: model.export_planes(tmp_path / "rect.planes")}
        for name, call in calls.items():
            with pytest.raises(b.VitHipError, match=name) as e:
                call()
            assert "non-square" in str(e.value) and "status 1" in str(e.value), str(e.value)
        model.sync()
        assert same(d_l.to_numpy(), fill) and (d_out.to_numpy() == 0xEE).all()
        assert not (tmp_path / "rect.planes").exists() and not list(tmp_path.iterdir())
        # a width that is no multiple of the patch, before the tensors are looked at: code 1
        bad = config(pkg, "f32", 2 * P, 8 * P + 8, P, 3)
        ctx = C.c_void_p()
        assert L.vit_hip_create_ex(C.byref(ctx), C.byref(bad), b.networks(weights), len(weights), 0, N, 0) == 1
        assert not ctx.value and L.vh_last_error().decode().startswith("vit_hip_create: img_width=136 must be a positive multiple")
        # pos_embedding with the square row count of img_size under a rectangular config: code 3
        sq = pkg.synth_weights(config(pkg, "f32", 2 * P, 0, P, 3), 7)
        assert L.vit_hip_create_ex(C.byref(ctx), C.byref(cfg), b.networks(sq), len(sq), 0, N, 0) == 3 and not ctx.value
        # a wrongly shaped array in the binding
        for wrong in (images.transpose(0, 1, 3, 2), images[:, :, :, :P]):
            with pytest.raises(ValueError, match="forward: images of shape"):
                model.forward(wrong)
        pixels = np.zeros(cfg.image_shape(N, "hwc"), np.uint8)
        with pytest.raises(ValueError, match="forward_u8: images of shape"):
            model.forward_u8(pixels, norm, None, "chw")
        with pytest.raises(ValueError, match="forward_u8: images of shape"):
            model.forward_u8(pixels.transpose(0, 2, 1, 3), norm, None, "hwc")
        after, _ = model.forward(images)
        assert same(before, after)
    finally:
        model.close()


# ---- square is untouched -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_square_is_untouched(pkg, device, tmp_path, precision):
    plain, named = config(pkg, precision, 4 * P, 0, P, 3), config(pkg, precision, 4 * P, 4 * P, P, 3)
    weights = pkg.synth_weights(plain, 7)
    a = pkg.ViTHip(plain, weights, device=0, max_batch=N, precision=precision)
    c = pkg.ViTHip(named, weights, device=0, max_batch=N, precision=precision)
    try:
        L = pkg.lib()
        for m in (a, c):
            held = L.vit_hip_config(m.ctx).contents
            assert held.img_width == 0 and held.img_size == 4 * P
        assert bytes(L.vit_hip_config(a.ctx).contents) == bytes(L.vit_hip_config(c.ctx).contents)
        images = pkg.synth_images(plain, 0, N)
        la, pa = a.forward(images)
        lc, pc = c.forward(images)
        assert same(la, lc) and same(pa, pc)
        a.export_planes(tmp_path / "a.planes")
        c.export_planes(tmp_path / "c.planes")
        assert (tmp_path / "a.planes").read_bytes() == (tmp_path / "c.planes").read_bytes()
        back = pkg.ViTHip.from_planes(tmp_path / "c.planes", device=0, max_batch=N)
        try:
            assert back.cfg.img_width == 0
            wide = back.at_size(3 * P, 5 * P)          # the way from a file to a non-square context
            try:
                assert wide.cfg.grid == (3, 5)
                assert np.isfinite(wide.forward(pkg.synth_images(wide.cfg, 0, N))[0]).all()
            finally:
                wide.close()
        finally:
            back.close()
    finally:
        a.close()
        c.close()
