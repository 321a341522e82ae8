"""Non-square inputs without a device: a config of img_size rows by img_width columns -- its grid, token count and
pos_embedding size, the one canonical form of a square config, vit_resample_check_hw with every refusal, and the sizes of the
feature and dense outputs on a 3 x 5 grid."""
import ctypes as C

import numpy as np
import pytest


def tiny(pkg, img_size, img_width=0, patch=16, chans=3):
    """embed 128, 2 heads of 64, depth 2, MLP 256, 10 classes"""
    return pkg.binding.VitConfig(img_size=img_size, patch_size=patch, in_chans=chans, num_classes=10, embed_dim=128, depth=2,
                                 num_heads=2, mlp_hidden=256, eps=1e-6, img_width=img_width)


def fields(cfg):
    return tuple(getattr(cfg, name) for name, _ in cfg._fields_)


def test_struct_size_is_the_c_size(pkg):
    b = pkg.binding
    assert C.sizeof(b.VitConfig) == pkg.lib().vit_config_sizeof()
    assert b.VitConfig._fields_[-1][0] == "img_width"
    assert pkg.preset("vit_b_16").img_width == 0 and pkg.preset("vit_h_14_518").img_width == 0


@pytest.mark.parametrize("h,w,patch,gh,gw", [(48, 80, 16, 3, 5), (80, 48, 16, 5, 3), (16, 96, 16, 1, 6), (56, 126, 14, 4, 9),
                                             (64, 0, 16, 4, 4), (64, 64, 16, 4, 4), (224, 336, 16, 14, 21)])
def test_grid_tokens_and_tensor_3(pkg, h, w, patch, gh, gw):
    L = pkg.lib()
    cfg = tiny(pkg, h, w, patch)
    assert cfg.grid == (gh, gw) and cfg.width == (w or h)
    assert L.vit_config_tokens(C.byref(cfg)) == gh * gw + 1 == pkg.binding.tokens(cfg)
    assert L.vit_config_tensor_size(C.byref(cfg), 3) == (gh * gw + 1) * 128
    assert L.vit_config_tensor_size(C.byref(cfg), 1) == 128 * 3 * patch * patch          # nothing else follows the size
    one = C.c_int(-1)
    L.vit_config_grid(C.byref(cfg), None, C.byref(one))                                 # either pointer may be NULL
    assert one.value == gw
    assert cfg.image_shape(3) == (3, 3, h, w or h) and cfg.image_shape(3, "hwc") == (3, h, w or h, 3)
    imgs = pkg.synth_images(cfg, 0, 3)
    assert imgs.shape == (3, 3, h, w or h)
    # the synthetic image is one stream of C * H * W values, whatever the two sides are
    assert np.array_equal(imgs[1].ravel(), pkg.synth_images(tiny(pkg, 1, h * (w or h), 1, 3), 1, 1).ravel())


def test_canonical_form(pkg):
    b = pkg.binding
    square = b.canonical_config(tiny(pkg, 64, 64))
    assert square.img_width == 0 and fields(square) == fields(tiny(pkg, 64, 0)) == fields(b.canonical_config(tiny(pkg, 64, 0)))
    assert bytes(square) == bytes(b.canonical_config(tiny(pkg, 64, 0)))                  # the padding too
    rect = b.canonical_config(tiny(pkg, 48, 80))
    assert (rect.img_size, rect.img_width) == (48, 80)
    cfg = tiny(pkg, 64, 64)                                                             # in place
    assert pkg.lib().vit_config_canonical(C.byref(cfg), C.byref(cfg), None) == 0 and cfg.img_width == 0
    for width, words in ((72, "multiple of patch_size"), (-16, "multiple of patch_size"), (4112, "above 4096")):
        with pytest.raises(b.VitHipError, match="vit_config_canonical") as e:
            b.canonical_config(tiny(pkg, 64, width))
        assert words in str(e.value) and "status 1" in str(e.value)
    with pytest.raises(b.VitHipError, match="patch grid is above 512"):
        b.canonical_config(tiny(pkg, 64, 2056, patch=4))                                # 514 patches across
    with pytest.raises(b.VitHipError, match="patch grid is above 512"):
        b.canonical_config(tiny(pkg, 2056, 64, patch=4))
    assert pkg.lib().vit_config_canonical(C.byref(cfg), C.byref(cfg), b"someone") == 0
    bad = tiny(pkg, 64, 72)
    assert pkg.lib().vit_config_canonical(C.byref(bad), C.byref(cfg), b"someone") == 1
    assert pkg.lib().vh_last_error().decode().startswith("someone: img_width=72")
    assert pkg.lib().vit_config_canonical(None, C.byref(cfg), None) == 1


def test_resample_check_hw_accepts(pkg):
    b = pkg.binding
    src = tiny(pkg, 64)
    out = b.resample_check(src, (48, 80))
    assert (out.img_size, out.img_width) == (48, 80)
    assert fields(out)[1:-1] == fields(src)[1:-1]
    assert b.resample_check(src, (80, 80)).img_width == 0 and b.resample_check(src, (80, 80)).img_size == 80
    for s in (16, 64, 224):                                                             # the square form is the hw form
        assert bytes(b.resample_check(src, s)) == bytes(b.resample_check(src, (s, s)))
    for mode in ("bicubic", "bilinear"):
        for ac in (False, True):
            assert b.resample_check(src, (16, 96), mode, ac).grid == (1, 6)
    assert pkg.lib().vit_resample_check_hw(C.byref(src), 48, 80, None, C.byref(out)) == 0   # how NULL: bicubic, 0
    # a non-square source, and out_cfg aliasing src
    rect = tiny(pkg, 48, 80)
    assert b.resample_check(rect, (64, 64)).img_width == 0
    alias = tiny(pkg, 48, 80)
    how = b.PosResampleC(0, 0)
    assert pkg.lib().vit_resample_check_hw(C.byref(alias), 32, 112, C.byref(how), C.byref(alias)) == 0
    assert (alias.img_size, alias.img_width, alias.embed_dim) == (32, 112, 128)
    assert pkg.lib().vit_resample_check_hw(C.byref(alias), 96, 96, C.byref(how), C.byref(alias)) == 0
    assert (alias.img_size, alias.img_width) == (96, 0)


def test_resample_check_hw_refuses(pkg):
    b, L = pkg.binding, pkg.lib()
    src = tiny(pkg, 64)
    untouched = tiny(pkg, 1)
    cases = [((0, 64), "img_height=0 must be a positive multiple of patch_size=16"),
             ((-16, 64), "img_height=-16 must be a positive multiple"),
             ((40, 64), "img_height=40 must be a positive multiple of patch_size=16"),
             ((64, 0), "img_width=0 must be a positive multiple of patch_size=16"),
             ((64, 72), "img_width=72 must be a positive multiple of patch_size=16"),
             ((16 * 513, 64), "img_height=8208 gives 513 patches a side"),
             ((64, 16 * 513), "img_width=8208 gives 513 patches a side")]
    for (h, w), words in cases:
        with pytest.raises(b.VitHipError, match="vit_resample_check_hw: ") as e:
            b.resample_check(src, (h, w))
        assert words in str(e.value) and "status 1" in str(e.value), str(e.value)
    for mode, ac, words in ((2, 0, "mode=2 must be VIT_POS_BICUBIC"), (-1, 0, "mode=-1"), (0, 2, "align_corners=2 must be 0 or 1")):
        how = b.PosResampleC(mode, ac)
        assert L.vit_resample_check_hw(C.byref(src), 48, 80, C.byref(how), C.byref(untouched)) == 1
        assert words in L.vh_last_error().decode() and L.vh_last_error().decode().startswith("vit_resample_check_hw: ")
    assert L.vit_resample_check_hw(None, 48, 80, None, C.byref(untouched)) == 1
    assert "null argument" in L.vh_last_error().decode()
    assert L.vit_resample_check_hw(C.byref(src), 48, 80, None, None) == 1
    for bad_src, words in ((tiny(pkg, 60), "the source's img_size=60"), (tiny(pkg, 64, 72), "the source's img_width=72"),
                           (tiny(pkg, 64, -16), "the source's img_width=-16")):
        assert L.vit_resample_check_hw(C.byref(bad_src), 48, 80, None, C.byref(untouched)) == 1
        assert words in L.vh_last_error().decode()
    assert fields(untouched) == fields(tiny(pkg, 1))                                    # a refusal writes nothing
    # the square entry keeps its own name and words
    with pytest.raises(b.VitHipError, match="vit_resample_check: img_size=40 must be a positive multiple of patch_size=16"):
        b.resample_check(src, 40)


def test_feature_and_dense_sizes_on_3_by_5(pkg):
    b = pkg.binding
    cfg = tiny(pkg, 48, 80)
    T, E = 16, 128
    for layout in ("nlc", "nchw"):
        assert b.feature_sizes(cfg, b.FeatureSpec((0, -1), token_layout=layout)) == (2 * E, 2 * E, 2 * (T - 1) * E)
    assert b.attention_sizes(cfg, b.AttentionSpec((-1,))) == (2 * T, T)
    assert b.rollout_sizes(cfg, b.RolloutSpec(0))[0] == T
    spec = b.DenseSpec(5, 0, 0, -1, True, E)
    assert b.dense_sizes(cfg, spec) == (48 * 80, 48 * 80, 15 * 5, 15 * (5 + E) * 4)      # 0, 0: img_size rows by width columns
    assert b.dense_sizes(cfg, b.DenseSpec(5, 37, 0, -1, False, E)) == (37 * 80, 37 * 80, 75, 15 * 5 * 4)
    assert b.dense_sizes(cfg, b.DenseSpec(5, 0, 50, -1, False, E))[0] == 48 * 50
    assert b.dense_sizes(tiny(pkg, 80, 48), spec)[0] == 80 * 48
    # the grid limit holds per side
    wide = tiny(pkg, 16, 16 * 65)
    with pytest.raises(b.VitHipError, match="at most 64 x 64"):
        b.dense_sizes(wide, spec)
    assert b.dense_sizes(tiny(pkg, 16, 16 * 64), spec)[2] == 64 * 5
