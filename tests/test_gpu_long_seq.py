"""Long-sequence attention (csrc/attention_long.hip, the plan's ATTN_LONG): the kernel against fp64 NumPy for any T,
tiny configs with T > 512 against the port, ViT-H/14 at 518 px and ViT-B/16 at 384 px against the port, and the new
kernel pinned to the reference's own outputs at 224 px through $VIT_HIP_ATTN=long.

"Parity unpinned" where the checker is the port (oracle/vit_seq_port.c with other loop bounds, bit-identical to the
reference's ViT_seq.c on ViT-B/16); the full-depth vectors are tests/golden/{b16_384,h14_518}_port_logits.npz
(tools/make_long_seq_goldens.py).  Tolerances are stated where they are asserted.
"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
ENV = ("VIT_HIP_P3", "VIT_HIP_GEMM_FP32", "VIT_HIP_ATTN", "VIT_HIP_LN_FOLD", "VIT_HIP_LAST_LAYER", "VIT_HIP_PRECISION")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)


def _logit_rel_l2(got, want):
    return float(np.linalg.norm(got - want) / np.linalg.norm(want - want.mean()))


def _rel_l2(got, want):
    return float(np.linalg.norm(got.astype(np.float64) - want) / np.linalg.norm(want.astype(np.float64)))


def _clear_top1(got, want, factor=4.0):
    top2 = np.sort(want)[-2:]
    return (top2[1] - top2[0]) <= factor * np.abs(got - want).max() or int(got.argmax()) == int(want.argmax())


# ---- 1. the kernel against fp64 ------------------------------------------------------------------------------------------

def _bf16_rne(x):
    """fp32 -> bf16 bits, round to nearest even (finite inputs)"""
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _bf16_val(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def _planes(rows, parts):
    """fused Q|K|V rows [R][3E] fp32 -> the QKV projection's planes: parts 3 = exact bf16 split [3E/32][3][R][32],
    parts 1 = fp16 [3E/32][R][32]"""
    R, N = rows.shape
    if parts == 1:
        return np.ascontiguousarray(rows.astype(np.float16).reshape(R, N // 32, 32).transpose(1, 0, 2))
    p0 = _bf16_rne(rows)
    r1 = (rows - _bf16_val(p0)).astype(np.float32)
    p1 = _bf16_rne(r1)
    p2 = _bf16_rne((r1 - _bf16_val(p1)).astype(np.float32))
    assert np.array_equal(_bf16_val(p0) + _bf16_val(p1) + _bf16_val(p2), rows)     # exact split
    st = np.stack([p.reshape(R, N // 32, 32) for p in (p0, p1, p2)])               # [3][R][N/32][32]
    return np.ascontiguousarray(st.transpose(2, 0, 1, 3))


def _upload(pkg, a):
    L = pkg.lib()
    d = pkg.DeviceBuffer((a.nbytes + 3) // 4)
    assert L.vh_h2d(d.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes, None) == 0
    return d


def _attention_fp64(qkv, n, T, H, D):
    E = H * D
    x = qkv.astype(np.float64).reshape(n, T, 3, H, D)
    out = np.empty((n, T, H, D))
    for b in range(n):
        for h in range(H):
            q, k, v = x[b, :, 0, h], x[b, :, 1, h], x[b, :, 2, h]
            s = q @ k.T / np.sqrt(D)
            s -= s.max(axis=1, keepdims=True)
            p = np.exp(s)
            out[b, :, h] = (p / p.sum(axis=1, keepdims=True)) @ v
    return out.reshape(n * T, E)


def _inputs(n, T, H, D, case, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, T, 3, H, D)).astype(np.float32)
    u = np.ones(D, dtype=np.float32)
    key = np.arange(T)
    if case == "last":        # the global maximum key of every query is the lone key of the last chunk (T = 64 k + 1)
        x[:, :, 0] += u
        x[:, T - 1, 1] += 2.0 * u
    elif case == "first":     # every maximum in chunk 0: no rescale after it
        x[:, :, 0] += u
        x[:, :64, 1] += 2.0 * u
    elif case == "rising":    # the maxima rise in every chunk (~2 softmax units per chunk): a rescale at every chunk
        x[:, :, 0] += u
        x[:, :, 1] += ((key // 64) * (2.0 / np.sqrt(D))).astype(np.float32)[:, None, None] * u
    elif case == "sink":      # key 3 outscores every other by >= 20 for every query; V has a channel at 40x
        x[:, :, 0] += u
        x[:, min(3, T - 1), 1] += (40.0 / np.sqrt(D)) * u
        x[:, :, 2, :, 5] *= 40.0
    return np.ascontiguousarray(x.reshape(n * T, 3 * H * D))


@pytest.mark.parametrize("parts", [3, 1])
@pytest.mark.parametrize("D", [64, 80])
@pytest.mark.parametrize("T", [1, 65, 577, 1025, 1370, 4097])
def test_long_attention_kernel_vs_fp64(pkg, device, T, D, parts):
    """vh_launch_attention_long on 2 images x 2 heads, gaussian Q/K/V and three inputs that steer the online softmax
    (global maximum in the lone key of the ragged last chunk, maxima in chunk 0 only, maxima rising in every chunk, an
    attention sink: one key 20+ softmax units above the rest for every query, with a V channel at 40x).
    parts 3 against fp64 on the fp32 values: the products are exact fp32 products of the splits, so what is left is fp32
    accumulation, the fp32 rounding of each score and exp2.  Measured 1e-6 - 4e-6 of max|O| up to T = 1370, 1e-5 at
    T = 4097 and 1.6e-5 for the rising maxima there (scores reach ~1100 before the 1/sqrt(D): one fp32 rounding of such a
    score is 7e-5, 8e-6 after the scale); bound 3e-5.  parts 1 against fp64 on the fp16-rounded Q/K/V: P is rounded to fp16
    (2^-11 relative) before P.V; measured 1.2e-4 - 1.9e-4, bound 1e-3."""
    L = pkg.lib()
    n, H = 2, 2
    E = H * D
    worst = 0.0
    for case in ("gauss", "last", "first", "rising", "sink"):
        qkv = _inputs(n, T, H, D, case, seed=T * 7 + D + parts)
        planes = _planes(qkv, parts)
        ref_in = qkv.astype(np.float16).astype(np.float32) if parts == 1 else qkv
        want = _attention_fp64(ref_in, n, T, H, D)
        d_in = _upload(pkg, planes)
        d_out = pkg.DeviceBuffer(n * T * E)
        assert L.vh_launch_attention_long(None, d_in.ptr, parts, d_out.ptr, n, T, E, H) == 0, L.vh_last_error().decode()
        got = d_out.to_numpy((n * T, E))
        d_in.free()
        d_out.free()
        assert np.isfinite(got).all(), case
        err = float(np.abs(got - want).max() / np.abs(want).max())
        worst = max(worst, err)
        assert err <= (3e-5 if parts == 3 else 1e-3), (case, err)
    print(f"attention_long T={T} D={D} parts={parts}: max|dO|/max|O| {worst:.2e}")


def test_long_attention_launcher_refuses_what_it_does_not_build(pkg, device):
    L = pkg.lib()
    d = pkg.DeviceBuffer(1 << 16)
    assert L.vh_launch_attention_long(None, d.ptr, 3, d.ptr, 1, 17, 256, 2) != 0      # head_dim 128
    assert L.vh_launch_attention_long(None, d.ptr, 2, d.ptr, 1, 17, 128, 2) != 0      # parts 2
    assert L.vh_launch_attention_long(None, d.ptr, 1, d.ptr, 0, 17, 128, 2) != 0      # no images
    assert L.vh_launch_attention_long(None, None, 1, d.ptr, 1, 17, 128, 2) != 0


# ---- 2. tiny long-T configs against the port -----------------------------------------------------------------------------

TINY_IMG = {368: 530, 384: 577, 512: 1025, 768: 2305}   # img -> T (patch 16)
_tiny_cache = {}


def _tiny(pkg, img):
    from oracle.oracle import Oracle
    if img not in _tiny_cache:
        orc = Oracle("vit_b_16")
        cfg = pkg.preset("vit_b_16")
        for c in (orc.cfg, cfg):
            c.img_size, c.patch_size, c.in_chans, c.num_classes = img, 16, 3, 10
            c.embed_dim, c.depth, c.num_heads, c.mlp_hidden = 256, 1, 4, 512
        weights = orc.synth_weights(23)
        imgs = np.stack([orc.synth_image(i) for i in range(5)])
        with ThreadPoolExecutor(5) as ex:
            want = np.stack(list(ex.map(lambda i: orc.forward(imgs[i], weights)[0], range(5))))
        _tiny_cache[img] = (cfg, weights, imgs, want)
    return _tiny_cache[img]


@pytest.mark.parametrize("img", sorted(TINY_IMG))
@pytest.mark.parametrize("fold", ["1", "0"])
def test_tiny_long_sequence_config_in_every_precision_vs_port(pkg, device, monkeypatch, tmp_path, fold, img):
    """embed 256, 4 heads of 64, MLP 512, depth 1, T = 530 / 577 / 1025 / 2305: every precision that runs above 512
    tokens, LayerNorms folded and not, against the port with the same loop bounds (live).  A context rebuilt from its
    planes file and run in ragged chunks gives the same bits; batch position does not change a bit; f32 within 1e-4 with
    equal arg-max, bf16 within 4e-2, fp8 within 0.15 relative L2 (the bounds of the tiny configs at T <= 226)."""
    cfg, weights, imgs, want = _tiny(pkg, img)
    assert pkg.binding.tokens(cfg) == TINY_IMG[img]
    monkeypatch.setenv("VIT_HIP_LN_FOLD", fold)
    with pytest.raises(pkg.VitHipError):      # refused at creation: no kernel runs this precision above 512 tokens
        pkg.ViTHip(cfg, weights, device=0, max_batch=5, precision="f32_fp16x2")
    for precision in ("f32", "bf16", "fp8"):
        m = pkg.ViTHip(cfg, weights, device=0, max_batch=5, precision=precision)
        got, probs = m.forward(imgs)
        again, _ = m.forward(imgs[[3, 0]])
        m.export_planes(tmp_path / f"long_{precision}.planes")
        m.close()
        small = pkg.ViTHip.from_planes(tmp_path / f"long_{precision}.planes", device=0, max_batch=2)
        chunked, _ = small.forward(imgs)
        small.close()
        err = float(np.abs(got - want).max())
        rel = max(_logit_rel_l2(got[i], want[i]) for i in range(5))
        print(f"tiny long config T={TINY_IMG[img]}, {precision}, fold {fold}: max |dlogit| {err:.3e}, relative L2 {rel:.4f}")
        assert np.array_equal(chunked, got)
        assert np.isfinite(got).all() and np.abs(probs.sum(axis=1) - 1.0).max() < 1e-5
        assert np.array_equal(again, got[[3, 0]])
        if precision == "f32":
            assert err <= 1e-4 and np.array_equal(got.argmax(1), want.argmax(1))
        elif precision == "bf16":
            assert err <= 4e-2
        else:
            assert rel <= 0.15


# ---- 3. ViT-H/14 at 518 px (head_dim 80, T = 1370) and ViT-B/16 at 384 px ------------------------------------------------

H14_SEED, H14_FIRST = 13, 9     # tests/golden/h14_518_port_logits.npz
B16_SEED, B16_FIRST = 11, 7     # tests/golden/b16_384_port_logits.npz


@pytest.fixture(scope="module")
def h14_518(pkg):
    cfg = pkg.preset("vit_h_14_518")
    return cfg, pkg.synth_weights(cfg, H14_SEED)


@pytest.fixture(scope="module")
def b16_384(pkg):
    cfg = pkg.preset("vit_b_16_384")
    return cfg, pkg.synth_weights(cfg, B16_SEED)


def test_vit_h14_518_two_layer_residual_stream_of_every_precision_vs_port(pkg, device, h14_518):
    """ViT-H/14 at 518 px (T = 1370, 16 heads of 80): the residual stream after two layers of two images against the
    port's (live, one thread per image), in f32, bf16 and fp8, with the bounds of the T = 257 three-layer test:
    max|d|/max|x| 2e-5 (f32), 6e-3 (bf16, also relative L2), 9e-2 (fp8, also relative L2)."""
    from oracle.oracle import Oracle
    cfg, weights = h14_518
    imgs = pkg.synth_images(cfg, H14_FIRST, 2)
    orc = Oracle("vit_h_14_518")
    with ThreadPoolExecutor(2) as ex:
        want = list(ex.map(lambda i: orc.forward(imgs[i], weights, stop_after_layers=2)[2], range(2)))
    short = pkg.preset("vit_h_14_518")
    short.depth = 2
    w2 = weights[:4 + 12 * 2] + weights[-4:]
    got = {}
    for precision in ("f32", "bf16", "fp8"):
        m = pkg.ViTHip(short, w2, device=0, max_batch=2, precision=precision)
        m.forward(imgs)
        got[precision] = m.read_tokens(2).reshape(2, 1370, cfg.embed_dim)
        m.close()
    for i in range(2):
        scale = max(float(np.abs(want[i]).max()), 1.0)
        err = {p: (float(np.abs(got[p][i] - want[i]).max()) / scale, _rel_l2(got[p][i], want[i])) for p in got}
        print(f"ViT-H/14 518 px image {H14_FIRST + i}, 2 layers, (max|d|/max|x|, relative L2) vs port:", err)
        assert err["f32"][0] <= 2e-5
        assert err["bf16"][0] <= 6e-3 and err["bf16"][1] <= 6e-3
        assert err["fp8"][0] <= 9e-2 and err["fp8"][1] <= 9e-2


@pytest.mark.parametrize("which", ["b16_384", "h14_518"])
def test_long_sequence_full_depth_logits_of_every_precision_vs_port_golden(pkg, device, which, request):
    """Full depth at T = 577 (ViT-B/16, 384 px) and T = 1370 (ViT-H/14, 518 px) against the port's committed logits:
    f32 within 1e-4 with equal arg-max and probabilities within 1e-6; bf16 within 5e-2 and 1.5 % relative L2; fp8 within
    0.12 relative L2 (the bounds of the 224 px full-depth tests)."""
    cfg, weights = request.getfixturevalue(which)
    seed, first = (B16_SEED, B16_FIRST) if which == "b16_384" else (H14_SEED, H14_FIRST)
    gold = np.load(GOLDEN / f"{which}_port_logits.npz")
    assert list(gold["images"]) == [first, first + 1] and int(gold["seed_base"]) == seed
    imgs = pkg.synth_images(cfg, first, 2)
    out = {}
    for precision in ("f32", "bf16", "fp8"):
        m = pkg.ViTHip(cfg, weights, device=0, max_batch=2, precision=precision)
        out[precision] = m.forward(imgs)
        m.close()
    for i in range(2):
        want_l, want_p = gold["logits"][i], gold["probs"][i]
        l32, p32 = out["f32"][0][i], out["f32"][1][i]
        l16, l8 = out["bf16"][0][i], out["fp8"][0][i]
        e32 = float(np.abs(l32 - want_l).max())
        e16, r16, r8 = float(np.abs(l16 - want_l).max()), _logit_rel_l2(l16, want_l), _logit_rel_l2(l8, want_l)
        print(f"{which} image {first + i} vs port: f32 max|dlogit| {e32:.3e}; bf16 {e16:.3e} relL2 {r16:.3e}; fp8 relL2 {r8:.3e}")
        assert e32 <= 1e-4 and int(l32.argmax()) == int(want_l.argmax())
        assert np.abs(p32 - want_p).max() <= 1e-6
        assert np.isfinite(l16).all() and np.isfinite(l8).all()
        assert e16 <= 5e-2 and r16 <= 1.5e-2 and _clear_top1(l16, want_l)
        assert r8 <= 0.12 and _clear_top1(l8, want_l)
        assert abs(float(out["fp8"][1][i].sum()) - 1.0) < 1e-5


# ---- 4. pinned to the reference: the new kernel at 224 px ----------------------------------------------------------------

def test_long_attention_forced_at_224_matches_the_references_own_outputs(pkg, device, weights, golden_full, monkeypatch):
    """$VIT_HIP_ATTN=long runs attention_long.hip at T = 197 in the fp32 path: logits of synthetic images 0..3 and of the
    reference's real image within 1e-4 of what the reference's own ViT_seq.c produced, with equal arg-max."""
    monkeypatch.setenv("VIT_HIP_ATTN", "long")
    cfg = pkg.preset("vit_b_16")
    real = np.load(GOLDEN / "b16_real_image.npz")
    assert int(golden_full["seed_base"]) == 0 and int(real["seed_base"]) == 0
    m = pkg.ViTHip(cfg, weights, device=0, max_batch=5)
    imgs = np.concatenate([pkg.synth_images(cfg, int(golden_full["first_image"]), 4), real["image"][None]])
    logits, probs = m.forward(imgs)
    m.close()
    want = np.concatenate([golden_full["logits"], real["logits"]])
    err = np.abs(logits - want).max(axis=1)
    print("VIT_HIP_ATTN=long at 224 px, max |dlogit| per image vs the reference:", err)
    assert err.max() <= 1e-4 and np.array_equal(logits.argmax(1), want.argmax(1))
    assert np.abs(probs[:4] - golden_full["probs"]).max() <= 1e-6


# ---- 5. at size ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "fp8"])
def test_vit_b16_384_at_64_images_is_batch_position_independent(pkg, device, b16_384, precision):
    """64 x ViT-B/16 at 384 px (36 928 rows): a permuted subset run on its own gets the rows it gets in the full batch,
    bit for bit."""
    cfg, weights = b16_384
    imgs = pkg.synth_images(cfg, 0, 64)
    big = pkg.ViTHip(cfg, weights, device=0, max_batch=64, precision=precision)
    lb, pb = big.forward(imgs)
    big.close()
    pick = [63, 0, 31, 32, 1, 62, 17]
    small = pkg.ViTHip(cfg, weights, device=0, max_batch=8, precision=precision)
    ls, ps = small.forward(imgs[pick])
    small.close()
    assert np.isfinite(lb).all() and np.abs(pb.sum(axis=1) - 1.0).max() < 1e-5
    assert np.array_equal(lb[pick], ls) and np.array_equal(pb[pick], ps)
