"""Position-embedding resampling on the GPU (csrc/pos_resample.hip) and the contexts derived with it
(vit_hip_create_at_resolution): the kernel against the float64 statement of its definition (tests/pos_resample_ref.py)
within the header's bound for every element, channel independence, the launcher's refusals, and derived contexts against
contexts created natively at the target size from the same tensors -- bit for bit, since nothing but tensor 3 is recomputed.

The bound, per element: |got - want| <= 2^-24 |want| + 2^-40 M, M the largest |p| of the source grid
(include/kernelHandler.h derives it)."""
import ctypes as C

import numpy as np
import pytest

import pos_resample_ref as pr
from ingest_common import tiny_config

pytestmark = pytest.mark.gpu

ENV = ("VIT_HIP_P3", "VIT_HIP_GEMM_FP32", "VIT_HIP_ATTN", "VIT_HIP_LN_FOLD", "VIT_HIP_LAST_LAYER", "VIT_HIP_PRECISION")
GRIDS = [((1, 1), (3, 3)), ((2, 2), (3, 3)), ((3, 3), (2, 2)), ((14, 14), (24, 24)), ((24, 24), (14, 14)), ((4, 4), (1, 1)),
         ((3, 5), (4, 2)), ((7, 3), (1, 6))]
MODES = [("bicubic", False), ("bicubic", True), ("bilinear", False), ("bilinear", True)]


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)


def _pos(prefix, in_hw, E, seed):
    """rows of size 3 whose channels carry the scales 1e3, 1 and 1e-3 in turn"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-3.0, 3.0, size=(prefix + in_hw[0] * in_hw[1], E))
    return (p * np.array([1e3, 1.0, 1e-3])[np.arange(E) % 3]).astype(np.float32)


def _check(got, pos, prefix, in_hw, out_hw, mode, ac, what):
    """got against the float64 reference: the prefix rows and equal grids bit for bit, everything within the bound"""
    want = pr.resample_pos_embed(pos, prefix, in_hw, out_hw, mode, ac)
    assert got.shape == want.shape and got.dtype == np.float32, what
    assert np.array_equal(got[:prefix], pos[:prefix]), what
    if in_hw == out_hw:
        assert np.array_equal(got, pos), what
    err = np.abs(got.astype(np.float64) - want)
    lim = pr.bound(want, pos[prefix:])
    worst = float((err / lim).max()) if err.size else 0.0
    assert (err <= lim).all(), (what, worst)
    return worst


# ---- 1. the kernel against float64 -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,ac", MODES)
def test_kernel_within_the_bound_of_the_float64_definition(pkg, device, mode, ac):
    b = pkg.binding
    worst = 0.0
    for k, (in_hw, out_hw) in enumerate(GRIDS + [((5, 5), (5, 5))]):
        for E in (4, 132, 768):
            for prefix in (0, 1, 2):
                pos = _pos(prefix, in_hw, E, 1000 * k + E + prefix)
                got = b.resample_pos_embed(pos, prefix, in_hw, out_hw, mode, ac)
                worst = max(worst, _check(got, pos, prefix, in_hw, out_hw, mode, ac, (in_hw, out_hw, E, prefix)))
    pos = _pos(1, (37, 37), 1280, 5)                    # ViT-H/14 at 518 px down to 224 px
    got = b.resample_pos_embed(pos, 1, (37, 37), (16, 16), mode, ac)
    worst = max(worst, _check(got, pos, 1, (37, 37), (16, 16), mode, ac, "37 -> 16, E 1280"))
    print(f"resample {mode} align_corners={ac}: worst error / bound {worst:.3f}")


# ---- 2. a channel does not see its neighbours ----------------------------------------------------------------------------

@pytest.mark.parametrize("mode,ac", MODES)
def test_channel_bits_do_not_depend_on_embed_dim(pkg, device, mode, ac):
    b = pkg.binding
    for in_hw, out_hw in (((14, 14), (24, 24)), ((7, 3), (1, 6)), ((3, 3), (2, 2))):
        pos = _pos(1, in_hw, 132, 77)
        wide = b.resample_pos_embed(pos, 1, in_hw, out_hw, mode, ac)
        for c in (0, 64, 128):
            narrow = b.resample_pos_embed(np.ascontiguousarray(pos[:, c:c + 4]), 1, in_hw, out_hw, mode, ac)
            assert np.array_equal(narrow, wide[:, c:c + 4]), (in_hw, out_hw, c)


# ---- 3. the launcher's refusals ----------------------------------------------------------------------------------------------

def test_launcher_refuses_with_its_name_and_writes_nothing(pkg, device):
    L = pkg.lib()
    n = 1 << 14
    fill = np.full(n, 7.25, dtype=np.float32)
    d_src, d_dst = pkg.DeviceBuffer.from_numpy(_pos(1, (4, 4), 8, 1).ravel()), pkg.DeviceBuffer.from_numpy(fill)
    s, d = d_src.ptr.value, d_dst.ptr.value
    #        src dst prefix in_h in_w out_h out_w E  mode ac
    good = (s, d, 1, 4, 4, 6, 6, 8, 0, 0)
    bad = {
        "E = 6": (s, d, 1, 4, 4, 6, 6, 6, 0, 0),
        "E = 0": (s, d, 1, 4, 4, 6, 6, 0, 0, 0),
        "in_h = 0": (s, d, 1, 0, 4, 6, 6, 8, 0, 0),
        "out_w = 0": (s, d, 1, 4, 4, 6, 0, 8, 0, 0),
        "in_w = 513": (s, d, 1, 4, 513, 6, 6, 8, 0, 0),
        "out_h = 513": (s, d, 1, 4, 4, 513, 6, 8, 0, 0),
        "prefix = 9": (s, d, 9, 4, 4, 6, 6, 8, 0, 0),
        "prefix = -1": (s, d, -1, 4, 4, 6, 6, 8, 0, 0),
        "mode = 2": (s, d, 1, 4, 4, 6, 6, 8, 2, 0),
        "align_corners = 2": (s, d, 1, 4, 4, 6, 6, 8, 0, 2),
        "src == dst": (d, d, 1, 4, 4, 6, 6, 8, 0, 0),
        "overlap": (d + 64, d, 1, 4, 4, 6, 6, 8, 0, 0),
        "misaligned src": (s + 4, d, 1, 4, 4, 6, 6, 8, 0, 0),
        "misaligned dst": (s, d + 4, 1, 4, 4, 6, 6, 8, 0, 0),
        "null src": (None, d, 1, 4, 4, 6, 6, 8, 0, 0),
        "null dst": (s, None, 1, 4, 4, 6, 6, 8, 0, 0),
    }
    for what, args in bad.items():
        L.vh_set_error(1, b"")
        assert L.vh_launch_resample_pos_embed(None, *args) == 1, what
        msg = L.vh_last_error().decode()
        assert msg.startswith("vh_launch_resample_pos_embed: ") and len(msg) > 32, (what, msg)
    assert L.vh_device_sync() == 0
    assert np.array_equal(d_dst.to_numpy(), fill)
    assert L.vh_launch_resample_pos_embed(None, *good) == 0, L.vh_last_error().decode()
    out = d_dst.to_numpy()
    assert np.array_equal(out[37 * 8:], fill[37 * 8:]) and not np.array_equal(out[:37 * 8], fill[:37 * 8])
    d_src.free()
    d_dst.free()


# ---- 4.-6. derived contexts against native ones ------------------------------------------------------------------------------

def _derive_and_compare(pkg, cfg, img_to, precision, mode="bicubic", ac=False, seed=31, n=3):
    """src at cfg -> derived at img_to; a native context at img_to from src's host weights with the derived tensor 3.
    Checks tensor 3 against the reference and the two contexts' outputs bit for bit; -> (target cfg, weights with the
    derived tensor 3, images, logits)."""
    b = pkg.binding
    weights = pkg.synth_weights(cfg, seed)
    src = pkg.ViTHip(cfg, weights, device=0, max_batch=n, precision=precision)
    derived = src.at_resolution(img_to, mode=mode, align_corners=ac)
    g_in, g_out, E = cfg.img_size // cfg.patch_size, img_to // cfg.patch_size, cfg.embed_dim
    assert derived.cfg.img_size == img_to and derived.tokens == g_out * g_out + 1 and derived.max_batch == n
    assert derived.precision == precision and pkg.lib().vit_hip_ln_fold(derived.ctx) == pkg.lib().vit_hip_ln_fold(src.ctx)
    pos = derived.weight(3).reshape(derived.tokens, E)
    _check(pos, weights[3].reshape(-1, E), 1, (g_in, g_in), (g_out, g_out), mode, ac, ("tensor 3", precision, img_to))
    for i in (0, 1, 2, 4 + 2, len(weights) - 2):       # the fp32 tensors travel as they are
        assert np.array_equal(derived.weight(i), weights[i]), i
    w2 = list(weights)
    w2[3] = np.ascontiguousarray(pos.ravel())
    native = pkg.ViTHip(derived.cfg, w2, device=0, max_batch=n, precision=precision)
    images = pkg.synth_images(derived.cfg, 0, n)
    got_l, got_p = derived.forward(images)
    want_l, want_p = native.forward(images)
    for m in (src, derived, native):
        m.close()
    assert np.isfinite(got_l).all() and np.abs(got_p.sum(axis=1) - 1.0).max() < 1e-5
    assert np.array_equal(got_l, want_l) and np.array_equal(got_p, want_p), (precision, img_to)
    return derived.cfg, w2, images, got_l


@pytest.mark.parametrize("precision,img_from,img_to", [
    ("f32", 32, 48), ("f32", 64, 32), ("bf16", 32, 48), ("bf16", 64, 32), ("fp8", 32, 48), ("fp8", 64, 32), ("f32_fp16x2", 32, 48)])
def test_derived_context_is_bit_identical_to_a_native_one(pkg, device, precision, img_from, img_to):
    cfg = tiny_config(pkg, 3, img_from, 16, embed=256 if precision == "fp8" else 128, depth=1)
    _derive_and_compare(pkg, cfg, img_to, precision)


@pytest.mark.parametrize("mode,ac", MODES[1:])
def test_derived_context_in_the_other_conventions(pkg, device, mode, ac):
    _derive_and_compare(pkg, tiny_config(pkg, 3, 32, 16, depth=1), 48, "f32", mode, ac)


@pytest.mark.parametrize("fold", ["0", "1"])
def test_derived_context_keeps_the_sources_fold_whatever_the_switch_says_now(pkg, device, monkeypatch, fold):
    cfg = tiny_config(pkg, 3, 32, 16, depth=1)
    weights = pkg.synth_weights(cfg, 3)
    images = pkg.synth_images(tiny_config(pkg, 3, 48, 16, depth=1), 0, 2)
    monkeypatch.setenv("VIT_HIP_LN_FOLD", fold)
    src = pkg.ViTHip(cfg, weights, device=0, max_batch=2, precision="bf16")
    want = src.at_resolution(48).forward(images)[0]
    monkeypatch.setenv("VIT_HIP_LN_FOLD", "1" if fold == "0" else "0")
    other = src.at_resolution(48)
    assert pkg.lib().vit_hip_ln_fold(other.ctx) == int(fold)
    assert np.array_equal(other.forward(images)[0], want)


def test_same_size_gives_the_sources_bits(pkg, device):
    cfg = tiny_config(pkg, 3, 48, 16, depth=1)
    src = pkg.ViTHip(cfg, pkg.synth_weights(cfg, 5), device=0, max_batch=4)
    same = src.at_resolution(cfg.img_size, max_batch=2, mode="bilinear", align_corners=True)
    assert same.max_batch == 2 and same.tokens == src.tokens
    assert np.array_equal(same.weight(3), src.weight(3))
    images = pkg.synth_images(cfg, 0, 3)
    want = src.forward(images)
    got = same.forward(images)                                  # in chunks of 2
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_derived_context_crosses_into_the_long_sequence_plan(pkg, device, precision):
    """patch 4: 32 px (T = 65, resident attention) -> 96 px (T = 577, attention_long.hip); F32 also within the project's
    1e-4 of the CPU port run at that config with the read-back pos_embedding."""
    from oracle.oracle import Oracle
    cfg = tiny_config(pkg, 3, 32, 4, depth=1)
    cfg_t, w2, images, logits = _derive_and_compare(pkg, cfg, 96, precision)
    assert pkg.binding.tokens(cfg_t) == 577
    if precision == "f32":
        orc = Oracle("vit_b_16")
        for f, _ in cfg_t._fields_:
            setattr(orc.cfg, f, getattr(cfg_t, f))
        want = np.stack([orc.forward(images[i], w2)[0] for i in range(images.shape[0])])
        err = float(np.abs(logits - want).max())
        print(f"derived 32 -> 96 px, patch 4, f32 vs the port: max |dlogit| {err:.3e}")
        assert err <= 1e-4 and np.array_equal(logits.argmax(1), want.argmax(1))


# ---- 7. life cycle -----------------------------------------------------------------------------------------------------------

def test_derived_context_outlives_its_source_exports_and_serves_features(pkg, device, tmp_path):
    b = pkg.binding
    cfg = tiny_config(pkg, 3, 32, 16, depth=1)
    weights = pkg.synth_weights(cfg, 8)
    src = pkg.ViTHip(cfg, weights, device=0, max_batch=3, precision="bf16")
    derived = src.at_resolution(48)
    images = pkg.synth_images(derived.cfg, 0, 3)
    before = derived.forward(images)
    src.close()                                                  # nothing is shared
    after = derived.forward(images)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    derived.export_planes(tmp_path / "derived.planes")
    loaded = pkg.ViTHip.from_planes(tmp_path / "derived.planes", device=0, max_batch=3)
    assert loaded.cfg.img_size == 48 and loaded.precision == "bf16"
    assert np.array_equal(loaded.forward(images)[0], before[0])
    assert np.array_equal(loaded.weight(3), derived.weight(3))
    # an armed output like on any context: the patch tokens are the TARGET grid's T - 1 = 9 rows
    spec = b.FeatureSpec((-1,), final_norm=True)
    c_el, p_el, t_el = b.feature_sizes(derived.cfg, spec)
    assert (c_el, p_el, t_el) == (cfg.embed_dim, cfg.embed_dim, 9 * cfg.embed_dim)
    out = []
    for m in (derived, loaded):
        d_img, d_tok, d_cls = pkg.DeviceBuffer.from_numpy(images), pkg.DeviceBuffer(3 * t_el), pkg.DeviceBuffer(3 * c_el)
        m.set_features(spec, cls=d_cls, tokens=d_tok)
        m.forward_device(d_img.ptr, 3)
        m.sync()
        m.set_features(None)
        out.append((d_tok.to_numpy((3, 9, cfg.embed_dim)), d_cls.to_numpy((3, cfg.embed_dim))))
    assert np.isfinite(out[0][0]).all() and np.abs(out[0][0]).max() > 0
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    logits, cls, pooled = derived.embed(images, spec)
    assert np.array_equal(logits, before[0]) and np.array_equal(cls, out[0][1]) and pooled.shape == (3, cfg.embed_dim)
    derived.close()
    loaded.close()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------

def test_create_at_resolution_refusals_leave_the_source_as_it_was(pkg, device, monkeypatch):
    b, L = pkg.binding, pkg.lib()
    cfg = tiny_config(pkg, 3, 32, 4, depth=1)
    weights = pkg.synth_weights(cfg, 2)
    images = pkg.synth_images(cfg, 0, 2)

    def refused(src, img, code, how=None):
        ctx = C.c_void_p(0xdead)
        L.vh_set_error(1, b"")
        rc = L.vit_hip_create_at_resolution(C.byref(ctx), src.ctx if src is not None else None, img, 0,
                                            None if how is None else C.byref(b.PosResampleC(*how)))
        assert rc == code and not ctx.value, (img, rc)
        msg = L.vh_last_error().decode()
        assert len(msg) > 0
        return msg

    for precision in ("f32_fp16x2", "f32"):
        src = pkg.ViTHip(cfg, weights, device=0, max_batch=2, precision=precision)
        want = src.forward(images)[0]
        assert refused(src, 0, 1).startswith("vit_resample_check: ")
        assert refused(src, -32, 1).startswith("vit_resample_check: ")
        assert refused(src, 42, 1).startswith("vit_resample_check: ")          # not a multiple of the patch size
        assert refused(src, 2052, 1).startswith("vit_resample_check: ")        # 513 patches a side
        assert refused(src, 64, 1, (2, 0)).startswith("vit_resample_check: ")
        assert refused(src, 64, 1, (0, 2)).startswith("vit_resample_check: ")
        assert refused(None, 64, 1).startswith("vit_hip_create_at_resolution: ")
        if precision == "f32_fp16x2":
            assert "577 tokens" in refused(src, 96, 2)                           # no kernel runs fp16 pairs above 512 tokens
            with pytest.raises(b.VitHipError, match="status 2"):
                src.at_resolution(96)
        else:
            monkeypatch.setenv("VIT_HIP_P3", "0")                                # the switches are read afresh
            assert "577 tokens" in refused(src, 96, 2)
            monkeypatch.delenv("VIT_HIP_P3")
        assert L.vit_hip_create_at_resolution(None, src.ctx, 64, 0, None) == 1
        ok = src.at_resolution(64)                                               # and what is not refused still works
        assert ok.tokens == 257 and np.isfinite(ok.forward(pkg.synth_images(ok.cfg, 0, 1))[0]).all()
        ok.close()
        assert np.array_equal(src.forward(images)[0], want)
        src.close()
