"""Feature outputs, the part that needs no device: vit_feature_sizes and its refusals, and the bf16 rounding of
tests/features_ref.py against torch."""
import ctypes as C

import numpy as np
import pytest

import features_ref as fr


@pytest.mark.parametrize("preset,patches,grid", [("vit_b_16", 196, 14), ("vit_h_14", 256, 16), ("vit_b_16_384", 576, 24)])
def test_feature_sizes(pkg, preset, patches, grid):
    cfg = pkg.preset(preset)
    assert patches == grid * grid == pkg.binding.tokens(cfg) - 1
    for taps in [(-1,), (3, 7, -1), (0, 1, 2, 3)]:
        spec = pkg.binding.FeatureSpec(taps=taps)
        cls, pooled, tokens = pkg.binding.feature_sizes(cfg, spec)
        assert cls == pooled == len(taps) * cfg.embed_dim
        assert tokens == len(taps) * patches * cfg.embed_dim


def test_negative_taps_resolve(pkg):
    """-1 is depth - 1: next to depth - 1 itself it is a duplicate, next to depth - 2 it is ascending"""
    cfg = pkg.preset("vit_b_16")
    b = pkg.binding
    assert b.feature_sizes(cfg, b.FeatureSpec(taps=(cfg.depth - 2, -1)))[0] == 2 * cfg.embed_dim
    assert b.feature_sizes(cfg, b.FeatureSpec(taps=(-cfg.depth, -1)))[0] == 2 * cfg.embed_dim
    with pytest.raises(b.VitHipError):
        b.feature_sizes(cfg, b.FeatureSpec(taps=(cfg.depth - 1, -1)))
    with pytest.raises(b.VitHipError):
        b.feature_sizes(cfg, b.FeatureSpec(taps=(-1, cfg.depth - 2)))


def _sizes_rc(pkg, cfg, cs):
    out = C.c_size_t()
    return pkg.lib().vit_feature_sizes(C.byref(cfg) if cfg is not None else None, C.byref(cs) if cs is not None else None,
                                       C.byref(out), None, None)


def test_refusals_without_a_device(pkg):
    b, L = pkg.binding, pkg.lib()
    cfg = pkg.preset("vit_b_16")
    good = b.FeatureSpec(taps=(3, -1)).c_struct()
    assert _sizes_rc(pkg, cfg, good) == 0
    assert _sizes_rc(pkg, None, good) == 1 and _sizes_rc(pkg, cfg, None) == 1
    bad = []
    for n_taps in (0, 5, -1):
        s = b.FeatureSpec(taps=(3, -1)).c_struct()
        s.n_taps = n_taps
        bad.append(s)
    for taps in [(12,), (-13,), (3, 3), (7, 3), (3, -9), (0, 1, 2, 100)]:
        bad.append(b.FeatureSpec(taps=taps).c_struct())
    for field in ("dtype", "token_layout"):
        for v in (2, -1):
            s = b.FeatureSpec().c_struct()
            setattr(s, field, v)
            bad.append(s)
    for s in bad:
        assert _sizes_rc(pkg, cfg, s) == 1
        assert L.vh_last_error().decode().startswith("vit_feature_sizes:")
    # arming with no context needs no device either
    bufs = b.FeatureBuffers(None, None, None)
    assert L.vit_hip_set_features(None, C.byref(good), C.byref(bufs)) == 1
    assert L.vit_hip_set_features_host(None, C.byref(good), C.byref(bufs)) == 1
    assert L.vit_hip_set_features(None, None, None) == 1


def test_bf16_rounding_matches_torch():
    import torch
    rng = np.random.default_rng(7)
    bits = rng.integers(0, 1 << 32, size=1_000_000, dtype=np.uint64).astype(np.uint32)
    bits[:65536] = (np.arange(65536, dtype=np.uint32) << 16) | 0x8000                # exact ties, every upper half
    bits[65536:70000] = rng.integers(0, 1 << 23, size=70000 - 65536).astype(np.uint32)   # subnormals
    bits[70000:74000] = bits[65536:69536] | 0x80000000
    x = bits.view(np.float32)
    x = x[~np.isnan(x)]
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(fr.bf16_bits(x), want)
    assert np.array_equal(fr.bf16_bits(fr.bf16_to_f32(want)), want)
