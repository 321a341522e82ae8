"""Attention-map outputs, the part that needs no GPU: vit_attn_sizes on the presets, every refusal of the spec, and the
self-checks of the NumPy reference (tests/attn_ref.py) the GPU tests compare against."""
import ctypes as C

import numpy as np
import pytest

import attn_ref as ar

PRESETS = ["vit_b_16", "vit_b_16_384", "vit_l_16", "vit_h_14", "vit_h_14_518"]


@pytest.mark.parametrize("name", PRESETS)
def test_sizes_on_the_presets(pkg, name):
    b = pkg.binding
    cfg = pkg.preset(name)
    T, H = pkg.binding.tokens(cfg), cfg.num_heads
    for taps in ((-1,), (0, 2, -1), (0, 1, 2, 3)):
        assert b.attention_sizes(cfg, b.AttentionSpec(taps)) == (len(taps) * H * T, len(taps) * T)
    # either pointer may be NULL
    L, cs, one = pkg.lib(), b.AttentionSpec((3, -2)).c_struct(), C.c_size_t()
    assert L.vit_attn_sizes(C.byref(cfg), C.byref(cs), None, C.byref(one)) == 0 and one.value == 2 * T
    assert L.vit_attn_sizes(C.byref(cfg), C.byref(cs), C.byref(one), None) == 0 and one.value == 2 * H * T


def test_every_refusal_of_the_spec(pkg):
    b, L = pkg.binding, pkg.lib()
    cfg = pkg.preset("vit_b_16")
    h, m = C.c_size_t(), C.c_size_t()

    def refused(n_taps, taps, why):
        cs = b.AttnSpecC(n_taps, (C.c_int * 4)(*(list(taps) + [0] * (4 - len(taps)))))
        L.vh_set_error(1, b"stale")
        assert L.vit_attn_sizes(C.byref(cfg), C.byref(cs), C.byref(h), C.byref(m)) == 1, (n_taps, taps)
        msg = L.vh_last_error().decode()
        assert msg.startswith("vit_attn_sizes: ") and why in msg, msg

    refused(0, (), "n_taps")
    refused(5, (0, 1, 2, 3), "n_taps")
    refused(1, (12,), "outside")
    refused(1, (-13,), "outside")
    refused(2, (3, 2), "ascending")
    refused(2, (4, 4), "ascending")
    refused(2, (11, -1), "ascending")          # duplicates once -1 resolves to 11
    refused(3, (0, -12, 5), "ascending")       # -12 resolves to 0
    ok = b.AttentionSpec((0, -1)).c_struct()
    assert L.vit_attn_sizes(None, C.byref(ok), C.byref(h), C.byref(m)) == 1 and "NULL" in L.vh_last_error().decode()
    assert L.vit_attn_sizes(C.byref(cfg), None, C.byref(h), C.byref(m)) == 1 and "NULL" in L.vh_last_error().decode()
    assert L.vit_hip_set_attention(None, C.byref(ok), None) == 1 and "NULL context" in L.vh_last_error().decode()
    assert L.vit_hip_set_attention_host(None, None, None) == 1
    with pytest.raises(b.VitHipError, match="n_taps"):
        b.attention_sizes(cfg, b.AttentionSpec(()))
    # the feature request's resolver, shared: the same words for the same mistake
    fs = b.FeatureSpec(taps=(11, -1)).c_struct()
    assert L.vit_feature_sizes(C.byref(cfg), C.byref(fs), None, None, None) == 1 and "ascending" in L.vh_last_error().decode()
    assert L.vh_cls_attention_head_dim_ok(64) and L.vh_cls_attention_head_dim_ok(80) and L.vh_cls_attention_head_dim_ok(128)
    assert not L.vh_cls_attention_head_dim_ok(24) and not L.vh_cls_attention_head_dim_ok(144) and not L.vh_cls_attention_head_dim_ok(0)


def test_reference_self_checks():
    rng = np.random.default_rng(0)
    n, T, H, D = 2, 37, 3, 16
    qkv = (3.0 * rng.standard_normal((n * T, 3 * H * D))).astype(np.float32)
    heads, mean = ar.cls_attention(qkv, n, T, H)
    assert heads.dtype == np.float64 and heads.shape == (n, H, T) and mean.shape == (n, T)
    assert np.abs(heads.sum(axis=2) - 1.0).max() < 1e-14 and np.abs(mean.sum(axis=1) - 1.0).max() < 1e-14
    assert (heads > 0).all()
    # against the definition written out for one (image, head, key)
    i, h, t = 1, 2, 5
    q, K = qkv[i * T, h * D:(h + 1) * D].astype(np.float64), qkv[i * T:(i + 1) * T, H * D + h * D:H * D + (h + 1) * D].astype(np.float64)
    s = K @ q / np.sqrt(D)
    assert abs(heads[i, h, t] - np.exp(s[t] - s.max()) / np.exp(s - s.max()).sum()) < 1e-15
    # T = 1: the class token attends to itself
    one, one_mean = ar.cls_attention(qkv[:3], 3, 1, H)
    assert np.array_equal(one, np.ones((3, H, 1))) and np.array_equal(one_mean, np.ones((3, 1)))
    assert ar.bound(qkv, n, T, H).shape == (n, H, 1) and (ar.bound(qkv, n, T, H) > (T + 64) * 2.0 ** -24).all()


def test_planes_encoders_round_trip():
    rng = np.random.default_rng(1)
    rows = (rng.standard_normal((7, 96)) * np.exp(rng.uniform(-8, 8, (7, 96)))).astype(np.float32)
    p3 = ar.encode_planes3(rows)
    assert p3.shape == (3, 3, 7, 32) and p3.dtype == np.uint16
    assert np.array_equal(ar.decode_planes3(p3), rows)                         # the three-part split is exact
    f16 = ar.encode_f16(rows)
    assert f16.shape == (3, 7, 32) and f16.dtype == np.float16
    back = ar.decode_f16(f16)
    assert np.array_equal(back, rows.astype(np.float16).astype(np.float32))
    assert np.array_equal(ar.decode_f16(ar.encode_f16(back)), back)            # fp16 values pass unchanged
    # element (row r, column c) sits at [c / 32][r][c % 32] in both layouts
    assert f16[2, 4, 5] == np.float16(rows[4, 69]) and ar._bf16_val(p3[1, 0, 6, 31]) == ar._bf16_val(ar._bf16_rne(rows[6:7, 63:64]))[0, 0]
