"""GPU parity tests (run with -m gpu on an MI355X): every HIP kernel, called through
the C ABI, against the CPU oracle on the same seeded inputs; the whole model against
the golden vectors produced by the reference's own ViT_seq.c.

Tolerances (fp32 path).  The reference rounds twice per MAC in index order
(ViT_seq.c, x86-64 without FMA); the fp32 MFMA is a single-rounding fmaf chain in a
permuted k order, and reductions are trees.  Per-op tolerance is
|gpu - cpu| <= 2e-5 absolute on O(1) values; the model-level bar is the north star's:
class logits within 1e-4 of ViT_seq.c and the same argmax.
"""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OP_TOL = 2e-5
LOGIT_TOL = 1e-4
GOLDEN = Path(__file__).resolve().parent / "golden"


def _dev(pkg, a):
    return pkg.DeviceBuffer.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _launch(pkg, name, *args):
    L = pkg.lib()
    rc = getattr(L, name)(*args)
    assert rc == 0, f"{name}: {L.vh_last_error().decode()}"
    assert L.vh_device_sync() == 0, L.vh_last_error().decode()


@pytest.mark.parametrize("rows", [1, 5, 197, 1000])
def test_layer_norm_vs_oracle(pkg, device, oracle, weights, rows):
    x = oracle.synth_fill(rows * 768, 11 + rows, 3.0, 0.5).reshape(rows, 768)
    g, b = weights[4], weights[5]
    d_x, d_g, d_b, d_y = _dev(pkg, x), _dev(pkg, g), _dev(pkg, b), pkg.DeviceBuffer(rows * 768)
    _launch(pkg, "vh_launch_layer_norm", None, d_x.ptr, d_g.ptr, d_b.ptr, d_y.ptr, rows, 768, 768, 768, 1e-6)
    got = d_y.to_numpy((rows, 768))
    # the oracle normalises `tokens` rows of width cfg.embed_dim = 768
    want = oracle.layer_norm(x, g, b)
    assert np.abs(got - want).max() <= OP_TOL


def test_layer_norm_strided_rows_picks_class_tokens(pkg, device, oracle, weights):
    """Final norm reads row b*T of the residual stream only (in_row_stride = T*E)."""
    n, T, E = 3, 197, 768
    x = oracle.synth_fill(n * T * E, 5, 1.0, 0.0).reshape(n * T, E)
    d_x, d_g, d_b, d_y = _dev(pkg, x), _dev(pkg, weights[148]), _dev(pkg, weights[149]), pkg.DeviceBuffer(n * E)
    _launch(pkg, "vh_launch_layer_norm", None, d_x.ptr, d_g.ptr, d_b.ptr, d_y.ptr, n, E, T * E, E, 1e-6)
    want = oracle.layer_norm(x[::T], weights[148], weights[149])
    assert np.abs(d_y.to_numpy((n, E)) - want).max() <= OP_TOL


@pytest.mark.parametrize("M,K,N,gelu,resid", [
    (197, 768, 768, 0, False),     # attention out-projection shape
    (197, 768, 2304, 0, False),    # fused QKV
    (197, 768, 3072, 1, False),    # fc1 + GELU
    (197, 3072, 768, 0, True),     # fc2 + residual
    (1, 768, 1000, 0, False),      # classifier head: M = 1, ragged N
    (130, 768, 1000, 0, False),    # ragged M and N
    (3, 32, 128, 1, False),        # smallest legal K
])
def test_linear_vs_oracle(pkg, device, oracle, M, K, N, gelu, resid):
    x = oracle.synth_fill(M * K, 100 + M, 1.0, 0.1).reshape(M, K)
    w = oracle.synth_fill(N * K, 200 + N, 0.04, 0.0)
    b = oracle.synth_fill(N, 300 + N, 0.1, 0.0)
    r = oracle.synth_fill(M * N, 400, 1.0, 0.0).reshape(M, N)
    want = oracle.linear(x, w, b, N)
    if gelu:
        want = oracle.gelu(want.ravel()).reshape(M, N)
    if resid:
        want = r + want
    d_x, d_w, d_b = _dev(pkg, x), _dev(pkg, w), _dev(pkg, b)
    d_out = _dev(pkg, r) if resid else pkg.DeviceBuffer(M * N)   # residual aliases the output
    _launch(pkg, "vh_launch_linear", None, d_out.ptr, d_w.ptr, d_x.ptr, d_b.ptr, M, K, N, gelu,
            d_out.ptr if resid else None)
    got = d_out.to_numpy((M, N))
    assert np.abs(got - want).max() <= OP_TOL


@pytest.mark.parametrize("M,K,N,gelu,resid", [
    (197, 768, 2304, 0, False), (197, 768, 768, 0, True), (300, 768, 3072, 1, False), (5000, 3072, 768, 0, True),
    (4300, 768, 3072, 1, False),       # the 256x256-tile path (M >= 4096)
])
def test_linear_presplit_weight_planes_matches_fp32_weights(pkg, device, oracle, M, K, N, gelu, resid):
    """vh_launch_linear_w3 (weights split into three bf16 planes ahead of time) against the oracle
    and, bit for bit, against vh_launch_linear on the fp32 weights: the same six products per
    block in the same order, only where the split happens differs."""
    x = oracle.synth_fill(M * K, 300 + M, 1.0, 0.1).reshape(M, K)
    w = oracle.synth_fill(N * K, 301 + N, 0.04, 0.0)
    b = oracle.synth_fill(N, 302, 0.1, 0.0)
    r = oracle.synth_fill(M * N, 303, 1.0, 0.0).reshape(M, N)
    d_x, d_w, d_b, d_r = _dev(pkg, x), _dev(pkg, w), _dev(pkg, b), _dev(pkg, r)
    d_w3 = pkg.DeviceBuffer((3 * N * K + 1) // 2)
    _launch(pkg, "vh_launch_split3_planes", None, d_w.ptr, d_w3.ptr, N, K)
    planes = d_w3.to_numpy().view(np.uint16)[:3 * N * K].reshape(K // 32, 3, N, 32)     # K step, part, row, element
    parts = (planes.astype(np.uint32) << 16).view(np.float32).transpose(1, 2, 0, 3).reshape(3, N * K)
    assert np.array_equal(parts[0].astype(np.float64) + parts[1] + parts[2], w.astype(np.float64))   # exact split
    d_o1, d_o2 = pkg.DeviceBuffer(M * N), pkg.DeviceBuffer(M * N)
    _launch(pkg, "vh_launch_linear_w3", None, d_o1.ptr, d_w3.ptr, d_x.ptr, d_b.ptr, M, K, N, gelu, d_r.ptr if resid else None)
    _launch(pkg, "vh_launch_linear", None, d_o2.ptr, d_w.ptr, d_x.ptr, d_b.ptr, M, K, N, gelu, d_r.ptr if resid else None)
    got, ref = d_o1.to_numpy((M, N)), d_o2.to_numpy((M, N))
    assert np.array_equal(got, ref)
    if M <= 300:
        want = oracle.linear(x, w, b, N)
        if gelu:
            want = oracle.gelu(want.ravel()).reshape(M, N)
        if resid:
            want = r + want
        assert np.abs(got - want).max() <= OP_TOL


@pytest.mark.parametrize("M,K,N,gelu,resid", [
    (197, 768, 2304, 0, False), (197, 768, 768, 0, True), (300, 768, 3072, 1, False), (300, 3072, 768, 0, True),
    (4300, 768, 3072, 1, False),       # the 256x256-tile path (M >= 4096): checked on a row sample
])
def test_linear_fp16x2_emulation_vs_oracle(pkg, device, oracle, M, K, N, gelu, resid):
    """vh_launch_linear_h2: fp32 product emulated with two fp16 parts per operand and three
    matrix-core products.  Not exact (22 of 24 significand bits), but it must meet the SAME
    operator tolerance as the exact path: its truncation error is ~8e-8 of the result."""
    x = oracle.synth_fill(M * K, 310 + M, 1.0, 0.1).reshape(M, K)
    w = oracle.synth_fill(N * K, 311 + N, 0.04, 0.0)
    b = oracle.synth_fill(N, 312, 0.1, 0.0)
    r = oracle.synth_fill(M * N, 313, 1.0, 0.0).reshape(M, N)
    scale = 2.0 ** 18                                     # 0.04 * 2^18 ~ 10486: inside [8192, 16384)
    d_x, d_w, d_b, d_r = _dev(pkg, x), _dev(pkg, w), _dev(pkg, b), _dev(pkg, r)
    d_w2 = pkg.DeviceBuffer(N * K)
    _launch(pkg, "vh_launch_split2h_planes", None, d_w.ptr, d_w2.ptr, N, K, scale)
    planes = d_w2.to_numpy().view(np.float16)[:2 * N * K].reshape(K // 32, 2, N, 32).transpose(1, 2, 0, 3).reshape(2, N * K)
    rec = (planes[0].astype(np.float64) + planes[1].astype(np.float64)) / scale
    assert np.abs(rec - w).max() <= 2.0 ** -21 * np.abs(w).max()           # two parts: 22 bits
    d_o = pkg.DeviceBuffer(M * N)
    _launch(pkg, "vh_launch_linear_h2", None, d_o.ptr, d_w2.ptr, scale, d_x.ptr, d_b.ptr, M, K, N, gelu,
            d_r.ptr if resid else None)
    got = d_o.to_numpy((M, N))
    rows = np.arange(M) if M <= 300 else np.r_[0:40, 2000:2040, M - 40:M]
    want = oracle.linear(x[rows], w, b, N)
    if gelu:
        want = oracle.gelu(want.ravel()).reshape(len(rows), N)
    if resid:
        want = r[rows] + want
    assert np.abs(got[rows] - want).max() <= OP_TOL


def test_linear_rejects_bad_arguments(pkg, device):
    L = pkg.lib()
    d = pkg.DeviceBuffer(1024)
    assert L.vh_launch_linear(None, d.ptr, d.ptr, d.ptr, d.ptr, 4, 30, 8, 0, None) != 0   # K % 32
    assert b"multiple of 32" in L.vh_last_error()
    assert L.vh_launch_linear(None, None, d.ptr, d.ptr, d.ptr, 4, 32, 8, 0, None) != 0
    assert L.vh_launch_linear(None, d.ptr, d.ptr, d.ptr, d.ptr, 4, 32, 8, 1, d.ptr) != 0  # gelu + residual


@pytest.mark.parametrize("n_images,tokens", [(1, 197), (3, 197), (2, 5), (1, 33), (2, 64), (3, 1), (1, 208), (300, 7)])
def test_attention_vs_oracle(pkg, device, oracle, n_images, tokens):
    E = 768
    qkv = oracle.synth_fill(n_images * tokens * 3 * E, 17 + tokens, 1.5, 0.0).reshape(n_images * tokens, 3 * E)
    d_qkv, d_out = _dev(pkg, qkv), pkg.DeviceBuffer(n_images * tokens * E)
    _launch(pkg, "vh_launch_attention", None, d_qkv.ptr, d_out.ptr, n_images, tokens, E, 12)
    got = d_out.to_numpy((n_images * tokens, E))
    for i in range(n_images):
        want = oracle.attention(qkv[i * tokens:(i + 1) * tokens])
        assert np.abs(got[i * tokens:(i + 1) * tokens] - want).max() <= OP_TOL, f"image {i}"


def test_attention_peaked_scores(pkg, device, oracle):
    """Large score spread (softmax close to one-hot): max subtraction must hold."""
    T, E = 197, 768
    qkv = oracle.synth_fill(T * 3 * E, 99, 6.0, 0.0).reshape(T, 3 * E)
    d_qkv, d_out = _dev(pkg, qkv), pkg.DeviceBuffer(T * E)
    _launch(pkg, "vh_launch_attention", None, d_qkv.ptr, d_out.ptr, 1, T, E, 12)
    got = d_out.to_numpy((T, E))
    want = oracle.attention(qkv)
    assert np.isfinite(got).all() and np.abs(got - want).max() <= 1e-4


@pytest.mark.parametrize("preset,n_images,tokens", [
    ("vit_h_14", 2, 257),    # BASELINE config 5 shape: head_dim 80, K + V of one head exceed the LDS
    ("vit_h_14", 1, 16), ("vit_h_14", 3, 65), ("vit_h_14", 1, 300),
    ("vit_b_16", 1, 257), ("vit_b_16", 2, 209), ("vit_b_16", 1, 512),   # head_dim 64 past the resident kernel's 208
])
def test_attention_streaming_kernel_vs_oracle(pkg, device, preset, n_images, tokens):
    """The K/V-streaming kernel (attention_tiled.hip) on the shapes the resident kernel does not
    take.  The reference has no such shape (ViT_seq.c:10-21 hard-codes B/16): the oracle is the
    port's loop with other bounds, "parity unpinned"."""
    from oracle.oracle import Oracle
    orc = Oracle(preset)
    E, H = orc.cfg.embed_dim, orc.cfg.num_heads
    qkv = orc.synth_fill(n_images * tokens * 3 * E, 31 + tokens, 1.5, 0.0).reshape(n_images * tokens, 3 * E)
    d_qkv, d_out = _dev(pkg, qkv), pkg.DeviceBuffer(n_images * tokens * E)
    _launch(pkg, "vh_launch_attention", None, d_qkv.ptr, d_out.ptr, n_images, tokens, E, H)
    got = d_out.to_numpy((n_images * tokens, E))
    for i in range(n_images):
        want = orc.attention(qkv[i * tokens:(i + 1) * tokens])
        assert np.abs(got[i * tokens:(i + 1) * tokens] - want).max() <= OP_TOL, f"image {i}"


def test_attention_streaming_kernel_peaked_scores(pkg, device):
    """Large score spread (softmax close to one-hot) through the streaming kernel."""
    from oracle.oracle import Oracle
    orc = Oracle("vit_h_14")
    T, E, H = 257, orc.cfg.embed_dim, orc.cfg.num_heads
    qkv = orc.synth_fill(T * 3 * E, 99, 5.0, 0.0).reshape(T, 3 * E)
    d_qkv, d_out = _dev(pkg, qkv), pkg.DeviceBuffer(T * E)
    _launch(pkg, "vh_launch_attention", None, d_qkv.ptr, d_out.ptr, 1, T, E, H)
    got = d_out.to_numpy((T, E))
    assert np.isfinite(got).all() and np.abs(got - orc.attention(qkv)).max() <= 1e-4


def test_attention_rejects_unsupported_shapes(pkg, device):
    L = pkg.lib()
    d = pkg.DeviceBuffer(16)
    assert L.vh_launch_attention(None, d.ptr, d.ptr, 1, 257, 1200, 16) != 0   # head_dim 75
    assert b"head_dim" in L.vh_last_error()
    assert L.vh_launch_attention(None, d.ptr, d.ptr, 1, 513, 768, 12) != 0    # score row no longer fits registers
    assert b"tokens=513" in L.vh_last_error()
    assert L.vh_launch_attention(None, d.ptr, d.ptr, 0, 197, 768, 12) != 0    # empty batch


@pytest.mark.parametrize("rows,length", [(1, 1000), (7, 1000), (3, 5), (2, 2048), (4, 1)])
def test_softmax_vs_oracle(pkg, device, oracle, rows, length):
    x = oracle.synth_fill(rows * length, 7 + length, 4.0, 1.0).reshape(rows, length)
    d_x, d_y = _dev(pkg, x), pkg.DeviceBuffer(rows * length)
    _launch(pkg, "vh_launch_softmax", None, d_x.ptr, d_y.ptr, rows, length)
    got = d_y.to_numpy((rows, length))
    for r in range(rows):
        want = oracle.softmax(x[r])
        assert np.abs(got[r] - want).max() <= 1e-7 + 2e-6 * want.max()
        assert abs(float(got[r].sum()) - 1.0) < 1e-5


def test_patch_embed_vs_oracle(pkg, device, oracle, weights):
    cfg = pkg.preset("vit_b_16")
    imgs = pkg.synth_images(cfg, 10, 3)
    W = weights
    d = [_dev(pkg, a) for a in (imgs, W[1], W[2], W[0], W[3])]
    d_tok = pkg.DeviceBuffer(3 * 197 * 768)
    _launch(pkg, "vh_launch_patch_embed", None, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, d_tok.ptr,
            3, 3, 224, 16, 768)
    got = d_tok.to_numpy((3, 197, 768))
    for i in range(3):
        want = oracle.tokens_from_conv(oracle.conv2d(imgs[i], W[1], W[2]), W[0], W[3])
        assert np.abs(got[i] - want).max() <= OP_TOL, f"image {i}"


def test_patch_embed_patch14_gathered_rows_vs_oracle(pkg, device):
    """ViT-H/14 geometry (patch 14: K = 3*14*14 = 588, neither patch % 4 nor K % 32 holds): the
    gathered, zero-padded rows path.  Oracle = the port's conv loop with other bounds
    ("parity unpinned": the reference hard-codes 16x16 patches, ViT_seq.c:10-21)."""
    from oracle.oracle import Oracle
    orc = Oracle("vit_h_14")
    cfg = pkg.preset("vit_h_14")
    E, T = cfg.embed_dim, 257
    W = [orc.synth_fill(orc.tensor_size(i), 40 + i, 0.05, 0.0) for i in range(4)]
    imgs = pkg.synth_images(cfg, 20, 2)
    L = pkg.lib()
    need = L.vh_patch_embed_workspace(2, 3, 224, 14, E)
    assert need == (2 * 256 + E) * 608 * 4
    assert L.vh_patch_embed_workspace(2, 3, 224, 16, 768) == 0
    d = [_dev(pkg, a) for a in (imgs, W[1], W[2], W[0], W[3])]
    d_tok, d_ws = pkg.DeviceBuffer(2 * T * E), pkg.DeviceBuffer(need // 4)
    assert L.vh_launch_patch_embed(None, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, d_tok.ptr,
                                   2, 3, 224, 14, E) != 0
    assert b"workspace" in L.vh_last_error()
    _launch(pkg, "vh_launch_patch_embed_ws", None, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, d_tok.ptr,
            2, 3, 224, 14, E, d_ws.ptr, need)
    got = d_tok.to_numpy((2, T, E))
    for i in range(2):
        want = orc.tokens_from_conv(orc.conv2d(imgs[i], W[1], W[2]), W[0], W[3])
        assert np.abs(got[i] - want).max() <= OP_TOL, f"image {i}"


# ---- whole model -----------------------------------------------------------------


@pytest.fixture(scope="module")
def model(pkg, device, weights):
    m = pkg.ViTHip(pkg.preset("vit_b_16"), weights, device=0, max_batch=8)
    yield m
    m.close()


def test_model_logits_vs_reference_goldens(pkg, model, golden_full):
    """Images 0..3: logits within 1e-4 of the reference's own output, same argmax,
    probabilities within 1e-6."""
    cfg = pkg.preset("vit_b_16")
    logits, probs = model.forward(pkg.synth_images(cfg, 0, 4))
    dl = np.abs(logits - golden_full["logits"]).max(axis=1)
    print("max |dlogit| per image:", dl)
    assert dl.max() <= LOGIT_TOL
    assert np.array_equal(logits.argmax(1), golden_full["logits"].argmax(1))
    assert np.abs(probs - golden_full["probs"]).max() <= 1e-6
    assert np.abs(probs.sum(1) - 1.0).max() < 1e-5


@pytest.mark.parametrize("precision", ["f32", "bf16", "fp8"])
def test_model_on_the_references_real_image(pkg, device, weights, precision):
    """The reference's one real input (Data/input-1.bin, kept as data in tests/golden/b16_real_image.npz: a normalised
    photograph -- spatially correlated, every channel's mean well above zero -- where all other goldens are iid-uniform
    pixels) against the logits the reference's own ViT_seq.c gives for it: the fp32 path within 1e-4 with the same
    arg-max, the bf16 mode within its 4e-2, the fp8 mode within its relative L2 of 0.15."""
    g = np.load(GOLDEN / "b16_real_image.npz")
    cfg = pkg.preset("vit_b_16")
    m = pkg.ViTHip(cfg, weights, device=0, max_batch=2, precision=precision)
    logits, probs = m.forward(np.stack([g["image"], pkg.synth_images(cfg, 0, 1)[0]]))     # next to a synthetic neighbour
    x = m.read_tokens(2)[:m.tokens].astype(np.float64)
    m.close()
    want = g["logits"][0]
    err = float(np.abs(logits[0] - want).max())
    rel = float(np.linalg.norm(logits[0] - want) / np.linalg.norm(want - want.mean()))
    print(f"real image, {precision}: max |dlogit| {err:.3e}, relative L2 {rel:.4f}; its residual rows after the last layer: "
          f"max |mean|/std {np.abs(x.mean(1) / x.std(1)).max():.3f}")
    assert np.isfinite(logits).all() and abs(float(probs[0].sum()) - 1.0) < 1e-5
    if precision == "f32":
        assert err <= LOGIT_TOL and int(logits[0].argmax()) == int(want.argmax())
        assert np.abs(probs[0] - g["probs"][0]).max() <= 1e-6
    elif precision == "bf16":
        assert err <= 4e-2
    else:
        assert rel <= 0.15


def test_model_on_a_second_weight_set_vs_reference_goldens(pkg, device, oracle):
    """Synthetic weights of seed_base 1 and images 100, 101 (tests/golden/b16_seed1.npz: the reference's own ViT_seq.c): the
    fp32 path within 1e-4 with the same arg-max, probabilities within 1e-6 -- the parity does not rest on one weight set."""
    g = np.load(GOLDEN / "b16_seed1.npz")
    cfg = pkg.preset("vit_b_16")
    m = pkg.ViTHip(cfg, oracle.synth_weights(int(g["seed_base"])), device=0, max_batch=2)
    logits, probs = m.forward(pkg.synth_images(cfg, int(g["first_image"]), 2))
    m.close()
    err = np.abs(logits - g["logits"]).max(axis=1)
    print("second weight set: max |dlogit| per image", err)
    assert err.max() <= LOGIT_TOL and np.array_equal(logits.argmax(1), g["logits"].argmax(1))
    assert np.abs(probs - g["probs"]).max() <= 1e-6


def test_model_residual_stream_vs_oracle(pkg, model, oracle, weights):
    """Residual stream after all 12 layers for one image vs the oracle (12 s of CPU)."""
    cfg = pkg.preset("vit_b_16")
    img = pkg.synth_images(cfg, 1, 1)
    model.forward(img)
    got = model.read_tokens(1)
    _, _, want = oracle.forward(img[0], weights)
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= 2e-5 * max(scale, 1.0)


def test_model_batch_position_independence(pkg, model):
    """An image's outputs do not depend on where in the batch it sits or on the batch
    size (bit-exact: the per-row arithmetic is identical), and chunking works."""
    cfg = pkg.preset("vit_b_16")
    imgs = pkg.synth_images(cfg, 0, 5)
    base, _ = model.forward(imgs)
    perm = np.array([3, 0, 4, 1, 2])
    shuffled, _ = model.forward(imgs[perm])
    assert np.array_equal(shuffled, base[perm])
    many = np.concatenate([imgs, imgs, imgs[:1]])          # 11 images > max_batch=8 -> two chunks
    out, probs = model.forward(many)
    assert np.array_equal(out[:5], base) and np.array_equal(out[5:10], base) and np.array_equal(out[10], base[0])
    assert np.isfinite(probs).all()


def test_nonfinite_pixel_poisons_only_its_own_image(pkg, model, golden_full):
    """The reference carried a NaN probe (findNaN, ViT_opencl.c:1050-1061, all calls commented
    out).  Here: a NaN pixel makes that image's outputs NaN -- no hang, no fault -- and leaves the
    other images of the batch bit-identical (nothing crosses images, ViT_opencl.c:926)."""
    cfg = pkg.preset("vit_b_16")
    imgs = pkg.synth_images(cfg, 0, 3)
    clean, _ = model.forward(imgs)
    imgs[1, 1, 100, 57] = np.nan
    logits, probs = model.forward(imgs)
    assert np.isnan(logits[1]).all() and np.isnan(probs[1]).all()
    assert np.array_equal(logits[0], clean[0]) and np.array_equal(logits[2], clean[2])
    rep = pkg.binding.CompareReport()
    import ctypes as C
    assert pkg.lib().vit_compare_rows(pkg.binding.fptr(np.ascontiguousarray(logits)),
                                      pkg.binding.fptr(np.ascontiguousarray(clean)), 3, 1000, 1e-4, C.byref(rep)) == 0
    assert rep.nonfinite == 1000 and rep.max_abs_diff == 0.0


def test_forward_rejects_empty_and_malformed_batches(pkg, model):
    """Edge cases at the boundary: n = 0, n beyond the arena, images of the wrong shape.
    Errors are status codes, never crashes, and the context stays usable."""
    L, b = pkg.lib(), pkg.binding
    cfg = pkg.preset("vit_b_16")
    imgs = pkg.synth_images(cfg, 0, 2)
    arr = b.image_array(imgs)
    logits = np.zeros((2, 1000), dtype=np.float32)
    assert L.vit_hip_forward(model.ctx, arr, 0, b.fptr(logits), None) == 1
    bad = b.image_array(np.zeros((1, 3, 112, 112), dtype=np.float32))
    assert L.vit_hip_forward(model.ctx, bad, 1, b.fptr(logits), None) == 5
    d = pkg.DeviceBuffer(16)
    assert L.vit_hip_forward_device(model.ctx, d.ptr, model.max_batch + 1, None, None, None) == 1
    assert L.vit_hip_forward_device(model.ctx, d.ptr, 0, None, None, None) == 1
    out, _ = model.forward(imgs[:1])                       # still works, n = 1
    assert np.isfinite(out).all()


def test_dropin_symbol_matches_extended_api(pkg, device, weights, golden_full):
    """ViT_opencl(ImageData*, Network*, float**) -- the reference's call surface
    (ViT_opencl.h:6, Main.c:54) -- fills caller-allocated rows synchronously, twice."""
    L, b = pkg.lib(), pkg.binding
    cfg = pkg.preset("vit_b_16")
    imgs = pkg.synth_images(cfg, 0, 2)
    for _ in range(2):                                       # repeatable, unlike the reference
        probs = np.full((2, 1000), -1.0, dtype=np.float32)
        rows = (b.f32p * 2)(*[b.fptr(probs[i]) for i in range(2)])
        L.ViT_opencl(b.image_array(imgs), b.networks(weights), rows)
        assert np.abs(probs - golden_full["probs"][:2]).max() <= 1e-6
        assert np.array_equal(probs.argmax(1), golden_full["probs"][:2].argmax(1))


def test_device_resident_path_and_full_size_properties(pkg, device, weights):
    """Bench-shaped call: 64 images resident in HBM, repeated images must give
    bit-identical rows; probabilities are a distribution; logits finite."""
    cfg = pkg.preset("vit_b_16")
    n = 64
    m = pkg.ViTHip(cfg, weights, device=0, max_batch=n)
    base = pkg.synth_images(cfg, 0, 8)
    imgs = np.concatenate([base] * 8)
    d_img = pkg.DeviceBuffer.from_numpy(imgs)
    d_logits, d_probs = pkg.DeviceBuffer(n * 1000), pkg.DeviceBuffer(n * 1000)
    m.forward_device(d_img.ptr, n, d_logits.ptr, d_probs.ptr)
    m.sync()
    logits, probs = d_logits.to_numpy((n, 1000)), d_probs.to_numpy((n, 1000))
    assert np.isfinite(logits).all()
    for k in range(1, 8):
        assert np.array_equal(logits[8 * k:8 * k + 8], logits[:8])
    assert np.abs(probs.sum(1) - 1.0).max() < 1e-5 and probs.min() >= 0
    host_logits, _ = m.forward(base)
    assert np.array_equal(host_logits, logits[:8])
    m.close()


def test_multi_device_entry_is_bit_identical_to_one_context(pkg, device, weights, golden_full):
    """vit_hip_create_multi / vit_hip_forward_multi (one host thread, context and stream per
    device, contiguous shards, outputs scattered straight into the caller's arrays).  This box has one
    GPU, so: (i) devices = [0] must equal the single-context path bit for bit; (ii) devices = [0, 0] --
    two replicas and two host threads on the same card -- splits 5 images 3 + 2 and must give the same
    bits again (an image's result does not depend on its shard); (iii) the drop-in ViT_opencl with
    $VIT_HIP_DEVICES=0,0 fills every probability row."""
    import os
    cfg = pkg.preset("vit_b_16")
    imgs = pkg.synth_images(cfg, 0, 5)
    one = pkg.ViTHip(cfg, weights, device=0, max_batch=3)
    base, base_p = one.forward(imgs)
    one.close()
    for devs in ([0], [0, 0], [0, 0, 0]):
        m = pkg.ViTHipMulti(cfg, weights, devs, max_batch_per_device=2)
        logits, probs = m.forward(imgs)
        m.close()
        assert np.array_equal(logits, base) and np.array_equal(probs, base_p), devs
    assert np.abs(base[:4] - golden_full["logits"]).max() <= LOGIT_TOL
    b, L = pkg.binding, pkg.lib()
    out = np.full((5, 1000), -1.0, dtype=np.float32)
    rows = (b.f32p * 5)(*[b.fptr(out[i]) for i in range(5)])
    os.environ["VIT_HIP_DEVICES"] = "0,0"
    try:
        L.ViT_opencl(b.image_array(imgs), b.networks(weights), rows)
    finally:
        del os.environ["VIT_HIP_DEVICES"]
    assert np.array_equal(out, base_p)
    with pytest.raises(pkg.VitHipError):
        pkg.ViTHipMulti(cfg, weights, [0, 99], max_batch_per_device=2)      # no such device: loud failure


def test_device_resident_multi_entry_with_the_rccl_gather_in_c(pkg, device, weights):
    """vit_hip_forward_device_multi ("RCCL over xGMI only for the final classifier gather", below Python):
    per-device image pointers in, logits gathered on device 0 by grouped ncclSend / ncclRecv on the compute streams.  This
    box has one GPU: the degenerate group devices = [0] (ncclCommInitAll of one, the root's shard written in place) must
    equal the single-context path bit for bit, twice in a row (the communicator is kept); two replicas on ONE device are
    refused loudly (RCCL needs distinct devices), as is a shard larger than max_batch.  N > 1: bench.py's
    in_library_multi_gpu leg."""
    cfg = pkg.preset("vit_b_16")
    n = 5
    imgs = pkg.synth_images(cfg, 40, n)
    one = pkg.ViTHip(cfg, weights, device=0, max_batch=n)
    base, base_p = one.forward(imgs)
    one.close()
    d_img = pkg.DeviceBuffer.from_numpy(imgs)
    d_l, d_p = pkg.DeviceBuffer(n * 1000), pkg.DeviceBuffer(n * 1000)
    m = pkg.ViTHipMulti(cfg, weights, [0], max_batch_per_device=n)
    for _ in range(2):
        m.forward_device([d_img.ptr], [n], d_l.ptr, d_p.ptr)
        assert np.array_equal(d_l.to_numpy((n, 1000)), base) and np.array_equal(d_p.to_numpy((n, 1000)), base_p)
    with pytest.raises(pkg.VitHipError, match="max_batch"):
        m.forward_device([d_img.ptr], [n + 1], d_l.ptr, None)
    m.close()
    m2 = pkg.ViTHipMulti(cfg, weights, [0, 0], max_batch_per_device=3)
    with pytest.raises(pkg.VitHipError, match="distinct"):
        m2.forward_device([d_img.ptr, d_img.ptr], [3, 2], d_l.ptr, None)
    m2.close()


def test_torch_interop_shares_one_hip_runtime(pkg, device, weights, golden_full):
    """bench.py hands torch-allocated HBM to the library (torch.distributed needs
    the logits in a torch tensor for the RCCL gather)."""
    import torch
    assert torch.cuda.is_available()
    cfg = pkg.preset("vit_b_16")
    m = pkg.ViTHip(cfg, weights, device=0, max_batch=2)
    imgs = torch.from_numpy(pkg.synth_images(cfg, 0, 2)).cuda()
    logits = torch.empty(2, 1000, device="cuda")
    torch.cuda.synchronize()
    # a torch SIDE stream: its handle is non-zero (handle 0 means "the context's own stream" to the
    # library, which torch does not order against), and torch work queued on it follows the forward
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    m.forward_device(imgs.data_ptr(), 2, logits.data_ptr(), None, side.cuda_stream)
    with torch.cuda.stream(side):
        host = logits.to("cpu", non_blocking=False).numpy()      # ordered after the kernels by the stream alone
    assert np.abs(host - golden_full["logits"][:2]).max() <= LOGIT_TOL
    m.close()


def test_rccl_gather_is_ordered_after_the_forward(tmp_path):
    """bench.py's N > 1 step on one GPU (VIT_DIST_FORCE=1: an RCCL group of world size 1): the forward
    is launched on a torch side stream and the gather of the logits is enqueued on the same stream, with
    NO host synchronisation in between and DIFFERENT images every step -- the gathered rows must equal a
    synchronised forward of the same images (a gather that overtook the kernels would return the previous
    step's logits)."""
    import os
    import subprocess
    import sys
    root = Path(__file__).resolve().parent.parent
    code = (
        "import sys, os, numpy as np; sys.path.insert(0, %r)\n"
        "import torch\n"
        "import __graft_entry__ as g\n"
        "pkg = g.load_package()\n"
        "from vit_with_opencl_amd.host.dist import Comm\n"
        "comm = Comm()\n"
        "assert comm.active and comm.backend == 'nccl'\n"
        "cfg = pkg.preset('vit_b_16'); w = pkg.synth_weights(cfg, 0)\n"
        "m = pkg.ViTHip(cfg, w, device=0, max_batch=4)\n"
        "side = torch.cuda.Stream(); assert side.cuda_stream != 0\n"
        "t_logits = torch.empty(4, 1000, device='cuda')\n"
        "for step in range(3):\n"
        "    imgs = torch.from_numpy(pkg.synth_images(cfg, 4 * step, 4)).cuda()\n"
        "    torch.cuda.synchronize()\n"
        "    m.forward_device(imgs.data_ptr(), 4, t_logits.data_ptr(), None, side.cuda_stream)\n"
        "    with torch.cuda.stream(side):\n"
        "        got = comm.gather_rows(t_logits)[0].clone()\n"
        "    side.synchronize()\n"
        "    ref = torch.empty(4, 1000, device='cuda')\n"
        "    m.forward_device(imgs.data_ptr(), 4, ref.data_ptr(), None, side.cuda_stream)\n"
        "    torch.cuda.synchronize()\n"
        "    assert torch.equal(got, ref), step\n"
        "m.close(); comm.close(); print('ok')\n"
    ) % str(root)
    env = dict(os.environ, VIT_DIST_FORCE="1", RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1",
               MASTER_PORT="29533")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-500:] + r.stderr[-1500:]


# ViT-L/16 and ViT-H/14 (BASELINE configs 4 and 5), in every precision and at their per-GPU batches: tests/test_gpu_configs.py


# torchvision state-dict key of tensor idx (reference file names: Network/Weight_<idx>_<key>.bin)
def _tensor_name(idx):
    if idx < 4:
        return ["class_token", "conv_proj_weight", "conv_proj_bias", "encoder_pos_embedding"][idx]
    if idx >= 148:
        return ["encoder_ln_weight", "encoder_ln_bias", "heads_head_weight", "heads_head_bias"][idx - 148]
    layer, k = divmod(idx - 4, 12)
    part = ["ln_1_weight", "ln_1_bias", "self_attention_in_proj_weight", "self_attention_in_proj_bias",
            "self_attention_out_proj_weight", "self_attention_out_proj_bias", "ln_2_weight", "ln_2_bias",
            "mlp_0_weight", "mlp_0_bias", "mlp_3_weight", "mlp_3_bias"][k]
    return f"encoder_layers_encoder_layer_{layer}_{part}"


def test_c_driver_over_files_matches_reference_flow(pkg, device, weights, tmp_path):
    """The whole drop-in flow from C, no Python in the process: a synthetic ./Data +
    ./Network tree in the reference's on-disk formats -> load_image_data / load_weights
    (with the 1e-6 rounding, Network.c:208-211) -> ViT_opencl -> result file in Main.c's
    format, checked against the outputs of the reference's own ViT_seq.c on equally rounded
    weights (oracle/make_golden.py, full_rounded).  The reference's own Main.c + comparator.c
    run in test_reference_main_and_comparator_drop_in_unchanged."""
    import shutil
    import subprocess
    from pathlib import Path
    L, b = pkg.lib(), pkg.binding
    root = Path(__file__).resolve().parent.parent
    exe = root / "vit-with-opencl_amd" / "vit_main"
    assert exe.exists(), "build with make -C vit-with-opencl_amd/csrc"
    (tmp_path / "Data").mkdir()
    (tmp_path / "Network").mkdir()
    cfg = pkg.preset("vit_b_16")
    imgs = pkg.synth_images(cfg, 0, 4)
    assert L.vit_write_image_file(str(tmp_path / "Data" / "input-100.bin").encode(), b.image_array(imgs), 4) == 0
    for idx, w in enumerate(weights):
        assert L.vit_write_weight_file(str(tmp_path / "Network").encode(), idx, _tensor_name(idx).encode(),
                                       b.fptr(w), w.size) == 0
    r = subprocess.run([str(exe)], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    print(r.stdout[-600:], r.stderr[-600:])
    assert r.returncode == 0, r.stdout[-400:] + r.stderr[-400:]
    # the same flow with the projections emulated on fp16 pairs ($VIT_HIP_PRECISION=fp16x2): same verdict
    import os
    r2 = subprocess.run([str(exe), "./Data/input-100.bin", "./Network", "./Data/fp16x2_result.txt"], cwd=tmp_path,
                        capture_output=True, text=True, timeout=300, env=dict(os.environ, VIT_HIP_PRECISION="fp16x2"))
    assert r2.returncode == 0, r2.stdout[-400:] + r2.stderr[-400:]
    assert (tmp_path / "Data" / "fp16x2_result.txt").read_text().splitlines()[0].split("/")[0] == \
        (tmp_path / "Data" / "opencl_result.txt").read_text().splitlines()[0].split("/")[0]
    # the offline repack from C: the first run with a planes file writes it, the second starts from it alone (the
    # Network directory is gone by then) and prints the same result lines
    r3 = subprocess.run([str(exe), "./Data/input-100.bin", "./Network", "./Data/planes_result_1.txt", "./b16.planes"], cwd=tmp_path,
                        capture_output=True, text=True, timeout=300)
    assert r3.returncode == 0 and (tmp_path / "b16.planes").stat().st_size > 800e6, r3.stdout[-400:] + r3.stderr[-400:]
    shutil.move(str(tmp_path / "Network"), str(tmp_path / "Network_gone"))
    r4 = subprocess.run([str(exe), "./Data/input-100.bin", "./Network", "./Data/planes_result_2.txt", "./b16.planes"], cwd=tmp_path,
                        capture_output=True, text=True, timeout=300)
    assert r4.returncode == 0 and "no weight files read" in r4.stdout, r4.stdout[-400:] + r4.stderr[-400:]
    first = (tmp_path / "Data" / "opencl_result.txt").read_text()
    assert (tmp_path / "Data" / "planes_result_1.txt").read_text() == first == (tmp_path / "Data" / "planes_result_2.txt").read_text()
    assert not (tmp_path / "b16.planes.tmp").exists()            # written under a temporary name, renamed when complete
    # a planes file that does not load (here: truncated) or that holds another precision than $VIT_HIP_PRECISION asks for is
    # rebuilt from the weight files and rewritten, with a message -- never silently used, never a dead end
    shutil.move(str(tmp_path / "Network_gone"), str(tmp_path / "Network"))
    size = (tmp_path / "b16.planes").stat().st_size
    with open(tmp_path / "b16.planes", "r+b") as f:
        f.truncate(size // 2)
    r5 = subprocess.run([str(exe), "./Data/input-100.bin", "./Network", "./Data/planes_result_3.txt", "./b16.planes"], cwd=tmp_path,
                        capture_output=True, text=True, timeout=300)
    assert r5.returncode == 0 and "rebuilding it from ./Network" in r5.stderr and (tmp_path / "b16.planes").stat().st_size == size, \
        r5.stdout[-400:] + r5.stderr[-400:]
    assert (tmp_path / "Data" / "planes_result_3.txt").read_text() == first
    r6 = subprocess.run([str(exe), "./Data/input-100.bin", "./Network", "./Data/planes_result_4.txt", "./b16.planes"], cwd=tmp_path,
                        capture_output=True, text=True, timeout=300, env=dict(os.environ, VIT_HIP_PRECISION="bf16"))
    assert r6.returncode == 0 and "asks for 1" in r6.stderr and (tmp_path / "b16.planes").stat().st_size < size, \
        r6.stdout[-400:] + r6.stderr[-400:]
    (tmp_path / "b16.planes").unlink()
    gold = np.load(root / "tests" / "golden" / "b16_full_rounded.npz")
    lines = (tmp_path / "Data" / "opencl_result.txt").read_text().splitlines()
    assert len(lines) == 4
    for i, line in enumerate(lines):
        label = int(line.split("label:")[1].split("/")[0])
        prob = float(line.split("prob:")[1])
        assert label == int(gold["probs"][i].argmax())
        assert abs(prob - float(gold["probs"][i].max())) <= 2e-6


def test_reference_main_and_comparator_drop_in_unchanged(pkg, device, weights, tmp_path):
    """North star: "Main.c and comparator.c drop in unchanged".  oracle/_ref/ref_main is the reference's
    OWN Main.c + comparator.c, compiled where they lie (oracle/Makefile; nothing copied, their own
    headers, MSVC CRT names from tests/compat/msvc_compat.h) and linked against libvit_hip.so.  Here it
    runs on a synthetic 100-image ./Data + 152-file ./Network tree in the reference's on-disk formats;
    ./Data/answer_result.txt holds what the reference's own ViT_seq.c + Main.c print for the same files
    (tests/golden/b16_answer_result_100_rounded.txt, oracle/make_golden.py answers100).  Pass = the
    comparator's success branch (Main.c:76-80: "good"), i.e. 100 labels equal, 100 probabilities within 0.01
    (comparator.c:74-86) -- and, stricter, every printed probability within 2e-6 of the golden line."""
    import shutil
    import subprocess
    from pathlib import Path
    L, b = pkg.lib(), pkg.binding
    root = Path(__file__).resolve().parent.parent
    exe = root / "oracle" / "_ref" / "ref_main"
    if not exe.exists():
        pytest.skip("oracle/_ref/ref_main not built (needs the reference tree in the build container)")
    (tmp_path / "Data").mkdir()
    (tmp_path / "Network").mkdir()
    cfg = pkg.preset("vit_b_16")
    imgs = pkg.synth_images(cfg, 0, 100)
    assert L.vit_write_image_file(str(tmp_path / "Data" / "input-100.bin").encode(), b.image_array(imgs), 100) == 0
    for idx, w in enumerate(weights):
        assert L.vit_write_weight_file(str(tmp_path / "Network").encode(), idx, _tensor_name(idx).encode(),
                                       b.fptr(w), w.size) == 0
    gold = root / "tests" / "golden" / "b16_answer_result_100_rounded.txt"
    shutil.copy(gold, tmp_path / "Data" / "answer_result.txt")
    r = subprocess.run([str(exe)], cwd=tmp_path, capture_output=True, timeout=600)
    out = r.stdout.decode("utf-8", "replace")
    print(out[-800:], r.stderr.decode("utf-8", "replace")[-400:])
    assert r.returncode == 0
    assert "good" in out and "bad1" not in out and "bad2" not in out        # Main.c:76-90
    got = (tmp_path / "Data" / "opencl_result.txt").read_text().splitlines()
    want = gold.read_text().splitlines()
    assert len(got) == len(want) == 100
    for g, w_ in zip(got, want):
        assert g.split("/")[0] == w_.split("/")[0], (g, w_)                   # "[i] label: L"
        assert abs(float(g.split("prob:")[1]) - float(w_.split("prob:")[1])) <= 2e-6, (g, w_)


# ---- bf16-operand GEMM mode (BASELINE config 3) -------------------------------------


def _to_bf16_bits(a):
    """fp32 -> bf16 bit patterns, round to nearest even (what v_cvt_pk_bf16_f32 does)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _bf16_bits_to_f32(r):
    return (r.astype(np.uint32) << 16).view(np.float32)


def _dev_raw(pkg, arr):
    """Upload any contiguous array as raw bytes."""
    arr = np.ascontiguousarray(arr)
    d = pkg.DeviceBuffer((arr.nbytes + 3) // 4)
    L = pkg.lib()
    assert L.vh_h2d(d.ptr, arr.ctypes.data, arr.nbytes, None) == 0 and L.vh_device_sync() == 0
    return d


def test_model_bf16_gemm_mode(pkg, device, weights, golden_full):
    """BASELINE config 3 (bf16 MFMA QKV/MLP GEMMs): stated tolerance for the class logits is
    4e-2 absolute against ViT_seq.c (operands carry 8 significant bits; measured ~1e-2),
    probabilities within 2e-4, arg-max equal wherever the reference's top-2 margin
    exceeds twice that tolerance."""
    cfg = pkg.preset("vit_b_16")
    m = pkg.ViTHip(cfg, weights, device=0, max_batch=4, precision="bf16")
    logits, probs = m.forward(pkg.synth_images(cfg, 0, 4))
    m.close()
    ref = golden_full["logits"]
    dl = np.abs(logits - ref).max(axis=1)
    print("bf16-GEMM mode: max |dlogit| per image:", dl)
    assert np.isfinite(logits).all() and dl.max() <= 4e-2
    assert np.abs(probs - golden_full["probs"]).max() <= 2e-4
    srt = np.sort(ref, axis=1)
    clear = (srt[:, -1] - srt[:, -2]) > 8e-2
    assert np.array_equal(logits.argmax(1)[clear], ref.argmax(1)[clear]) and clear.any()


def test_model_fp32_emulated_with_fp16_pairs_meets_the_fp32_tolerance(pkg, device, weights, golden_full):
    """VIT_PRECISION_F32_FP16X2 (opt-in): the projections on two fp16 parts / three products.  Same
    stated tolerance as the exact fp32 path -- class logits within 1e-4 of the reference's ViT_seq.c,
    same arg-max, probabilities within 1e-6 -- plus batch-position independence."""
    cfg = pkg.preset("vit_b_16")
    m = pkg.ViTHip(cfg, weights, device=0, max_batch=8, precision="f32_fp16x2")
    imgs = pkg.synth_images(cfg, 0, 4)
    logits, probs = m.forward(imgs)
    l2, _ = m.forward(np.concatenate([imgs[2:3], imgs[0:1]]))
    m.close()
    err = np.abs(logits - golden_full["logits"][:4]).max()
    print("fp16x2 emulation: max |dlogit| vs ViT_seq.c", err)
    assert err <= LOGIT_TOL
    assert np.array_equal(logits.argmax(1), golden_full["logits"][:4].argmax(1))
    assert np.abs(probs - golden_full["probs"][:4]).max() <= 1e-6
    assert np.array_equal(l2[0], logits[2]) and np.array_equal(l2[1], logits[0])


# ---- tuning / fallback paths behind environment switches ---------------------------------


SWITCHES = ("VIT_HIP_GEMM_FP32", "VIT_HIP_P3", "VIT_HIP_ATTN")


def _child_logits(env, out_path):
    """Two images through ViT-B/16 in a child process whose only switches are `env`: the child asserts the fp32
    parity against the reference's goldens and saves its logits to out_path."""
    import os
    import subprocess
    import sys
    root = Path(__file__).resolve().parent.parent
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g\n"
        "pkg = g.load_package(); cfg = pkg.preset('vit_b_16')\n"
        "m = pkg.ViTHip(cfg, pkg.synth_weights(cfg, 0), device=0, max_batch=2)\n"
        "logits, probs = m.forward(pkg.synth_images(cfg, 0, 2)); m.close()\n"
        "np.save(%r, logits)\n"
        "gold = np.load(%r)\n"
        "err = float(np.abs(logits - gold['logits'][:2]).max())\n"
        "print('max |dlogit|', err)\n"
        "assert err <= 1e-4 and (logits.argmax(1) == gold['logits'][:2].argmax(1)).all()\n"
    ) % (str(root), str(out_path), str(root / "tests" / "golden" / "b16_full.npz"))
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    r = subprocess.run([sys.executable, "-c", code], env=dict(base, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{env}: {r.stdout[-300:]} {r.stderr[-800:]}"
    return np.load(out_path)


@pytest.mark.parametrize("env", [
    {"VIT_HIP_GEMM_FP32": "native"},                                # fp32 matrix instruction: patch embedding and attention
    {"VIT_HIP_P3": "0"},                                            # activations split inside the GEMM loop (gemm_mfma.hip)
    {"VIT_HIP_P3": "0", "VIT_HIP_ATTN": "tiled"},                   # streaming attention kernel on the B/16 shape
])
def test_switchable_paths_meet_the_fp32_parity(env, tmp_path):
    """Each combination in a child process of its own: two images through the whole model against the reference's
    goldens at the fp32 tolerance.  VIT_HIP_ATTN=tiled goes with VIT_HIP_P3=0: the switch reaches only plans whose
    attention reads fp32 rows, and the default ViT-B/16 plan runs the planes attention (vh_launch_attention_planes),
    where `tiled` alone selects nothing."""
    _child_logits(env, tmp_path / "logits.npy")


def test_switches_are_read_at_context_creation_and_nowhere_else(pkg, device, weights, golden_full, monkeypatch, tmp_path):
    """Contexts made one after the other in ONE process under different switches: each meets the fp32 parity, and each
    gives, bit for bit, the logits of a process that has only ever seen that environment -- a switch that a launcher
    kept from its first use would make every context after the first run the first one's kernels."""
    cfg = pkg.preset("vit_b_16")
    images = pkg.synth_images(cfg, 0, 2)
    settings = [{"VIT_HIP_GEMM_FP32": "native"}, {}, {"VIT_HIP_P3": "0"}, {"VIT_HIP_P3": "0", "VIT_HIP_ATTN": "tiled"}, {}]
    got = []
    for env in settings:
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        m = pkg.ViTHip(cfg, weights, device=0, max_batch=2)
        logits, _ = m.forward(images)
        m.close()
        err = float(np.abs(logits - golden_full["logits"][:2]).max())
        print(env, "max |dlogit|", err)
        assert err <= LOGIT_TOL and np.array_equal(logits.argmax(1), golden_full["logits"][:2].argmax(1)), env
        got.append(logits)
    alone = {}
    for env, logits in zip(settings, got):
        key = tuple(sorted(env.items()))
        if key not in alone:
            alone[key] = _child_logits(env, tmp_path / f"alone{len(alone)}.npy")
        assert np.array_equal(logits, alone[key]), f"{env}: differs from a process with this environment alone"


def test_linear_with_explicit_fp32_math(pkg, device, oracle):
    """vh_launch_linear_math: one ragged M tile at the smallest N the split kernel takes, both arithmetics against the
    oracle; at a ragged N both run the guarded native tile and equal vh_launch_linear bit for bit."""
    M, K = 40, 64
    for N in (128, 72):
        x = oracle.synth_fill(M * K, 100 + M, 1.0, 0.1).reshape(M, K)
        w = oracle.synth_fill(N * K, 200 + N, 0.04, 0.0)
        b = oracle.synth_fill(N, 300 + N, 0.1, 0.0)
        want = oracle.linear(x, w, b, N)
        d_x, d_w, d_b, d_o = _dev(pkg, x), _dev(pkg, w), _dev(pkg, b), pkg.DeviceBuffer(M * N)
        got = {}
        for math, code in pkg.binding.FP32_MATH.items():
            _launch(pkg, "vh_launch_linear_math", None, d_o.ptr, d_w.ptr, d_x.ptr, d_b.ptr, M, K, N, 0, None, code)
            got[math] = d_o.to_numpy((M, N))
            assert np.abs(got[math] - want).max() <= OP_TOL, (N, math)
        if N == 72:
            _launch(pkg, "vh_launch_linear", None, d_o.ptr, d_w.ptr, d_x.ptr, d_b.ptr, M, K, N, 0, None)
            assert np.array_equal(got["split3"], got["native"]) and np.array_equal(got["split3"], d_o.to_numpy((M, N)))
    L = pkg.lib()
    assert L.vh_launch_linear_math(None, d_o.ptr, d_w.ptr, d_x.ptr, d_b.ptr, M, K, 72, 0, None, 2) != 0
    assert b"fp32_math" in L.vh_last_error()


def test_rows_attention_with_the_kernel_named(pkg, device):
    """vh_launch_attention_rows: the streaming kernel asked for at a shape the resident kernel would take (head_dim 64,
    one partial 32-key tile) against the oracle; where auto already streams (head_dim 80) both give the same bits; bad
    choices are refused."""
    from oracle.oracle import Oracle
    A, KN = pkg.binding.ATTN_ARITH, pkg.binding.ATTN_KERNEL
    orc = Oracle("vit_b_16")
    n, T, E, H = 2, 50, 128, 2
    orc.cfg.embed_dim, orc.cfg.num_heads = E, H
    qkv = orc.synth_fill(n * T * 3 * E, 31 + T, 1.5, 0.0).reshape(n * T, 3 * E)
    d_q, d_o = _dev(pkg, qkv), pkg.DeviceBuffer(n * T * E)
    _launch(pkg, "vh_launch_attention_rows", None, d_q.ptr, d_o.ptr, 0, A["split3"], KN["streaming"], n, T, E, H)
    got = d_o.to_numpy((n * T, E))
    for i in range(n):
        assert np.abs(got[i * T:(i + 1) * T] - orc.attention(qkv[i * T:(i + 1) * T])).max() <= OP_TOL, f"image {i}"

    n, T, E, H = 1, 50, 160, 2
    qkv = orc.synth_fill(n * T * 3 * E, 32 + T, 1.5, 0.0)
    d_q, d_a, d_b = _dev(pkg, qkv), pkg.DeviceBuffer(n * T * E), pkg.DeviceBuffer(n * T * E)
    _launch(pkg, "vh_launch_attention_rows", None, d_q.ptr, d_a.ptr, 0, A["split3"], KN["auto"], n, T, E, H)
    _launch(pkg, "vh_launch_attention_rows", None, d_q.ptr, d_b.ptr, 0, A["split3"], KN["streaming"], n, T, E, H)
    assert np.array_equal(d_a.to_numpy(), d_b.to_numpy()) and np.isfinite(d_a.to_numpy()).all()

    L = pkg.lib()
    assert L.vh_launch_attention_rows(None, d_q.ptr, d_a.ptr, 0, 7, KN["auto"], 1, 50, 128, 2) != 0
    assert b"arith" in L.vh_last_error()
    assert L.vh_launch_attention_rows(None, d_q.ptr, d_a.ptr, 0, A["split3"], 5, 1, 50, 128, 2) != 0
    assert b"kernel" in L.vh_last_error()
    assert L.vh_launch_attention_rows(None, d_q.ptr, d_a.ptr, 3, A["split3"], KN["streaming"], 1, 50, 128, 2) != 0
    assert b"planes" in L.vh_last_error()


@pytest.mark.parametrize("n_images,tokens,E,H", [(2, 257, 1280, 16), (1, 50, 1280, 16), (3, 300, 256, 2)])
def test_streaming_attention_with_fp16_operands_stays_within_the_reduced_modes_tolerance(pkg, device, oracle, n_images, tokens, E, H):
    """vh_launch_attention_f16 on shapes of the streaming kernel (head_dim 80 / 128, T > 208: ViT-H/14): Q, K, V and
    the probabilities rounded to fp16, one v_mfma_f32_16x16x16_f16 per four fp32 steps.  Against the fp32 streaming
    kernel (itself checked against the oracle above) the result differs by the operands' rounding only:
    |d| <= 2^-9 of the largest output magnitude (11-bit operands, sums of positive weights <= 1)."""
    rows = n_images * tokens
    qkv = oracle.synth_fill(rows * 3 * E, 911 + tokens, 1.0, 0.0)
    d_q, d_a, d_b = _dev(pkg, qkv), pkg.DeviceBuffer(rows * E), pkg.DeviceBuffer(rows * E)
    _launch(pkg, "vh_launch_attention", None, d_q.ptr, d_a.ptr, n_images, tokens, E, H)
    _launch(pkg, "vh_launch_attention_f16", None, d_q.ptr, d_b.ptr, n_images, tokens, E, H)
    a, b = d_a.to_numpy((rows, E)), d_b.to_numpy((rows, E))
    assert np.isfinite(b).all()
    err = np.abs(a - b).max()
    print("fp16-operand streaming attention: max |d| =", err, "of", np.abs(a).max())
    assert 0 < err <= 2.0 ** -9 * np.abs(a).max()


@pytest.mark.parametrize("n_images,tokens", [(2, 257), (1, 50), (40, 257), (3, 272), (1, 1)])
def test_resident_fp16_planes_attention_for_head_dim_80(pkg, device, oracle, n_images, tokens):
    """vh_launch_attention_planes_f16_hd80 (ViT-H/14's shape, K and V resident in LDS as fp16 planes) against
    vh_launch_attention_f16 on fp32 rows (the streaming kernel's fp16-operand form): the same operand rounding and
    softmax, another summation order -- |d| <= 2^-12 of the largest output magnitude -- and against the fp32
    streaming kernel within the operands' rounding (2^-9).  Several items per workgroup (40 x 16 on 256 workgroups),
    both rounds of query tiles, an odd and an even head offset in every image."""
    E, H = 1280, 16
    rows = n_images * tokens
    qkv = oracle.synth_fill(rows * 3 * E, 1011 + tokens, 1.0, 0.0).reshape(rows, 3 * E)
    d_q = _dev(pkg, qkv)
    planes = np.ascontiguousarray(qkv.astype(np.float16).reshape(rows, 3 * E // 32, 32).transpose(1, 0, 2))
    d_qh = pkg.DeviceBuffer.from_numpy(planes.ravel().view(np.float32))
    d_a, d_b, d_c = pkg.DeviceBuffer(rows * E), pkg.DeviceBuffer(rows * E), pkg.DeviceBuffer(rows * E)
    _launch(pkg, "vh_launch_attention", None, d_q.ptr, d_a.ptr, n_images, tokens, E, H)
    _launch(pkg, "vh_launch_attention_f16", None, d_q.ptr, d_b.ptr, n_images, tokens, E, H)
    _launch(pkg, "vh_launch_attention_planes_f16_hd80", None, d_qh.ptr, d_c.ptr, n_images, tokens, E, H)
    a, b, c = d_a.to_numpy((rows, E)), d_b.to_numpy((rows, E)), d_c.to_numpy((rows, E))
    assert np.isfinite(c).all()
    big = np.abs(a).max()
    print("resident fp16 attention: max |d| vs streaming fp16 form", np.abs(c - b).max(), "vs fp32", np.abs(c - a).max(), "of", big)
    assert np.abs(c - b).max() <= 2.0 ** -12 * big
    assert np.abs(c - a).max() <= 2.0 ** -9 * big
    L = pkg.lib()
    assert L.vh_launch_attention_planes_f16_hd80(None, d_qh.ptr, d_c.ptr, n_images, 273, E, H) != 0
    assert L.vh_launch_attention_planes_f16_hd80(None, d_qh.ptr, d_c.ptr, n_images, tokens, 1024, H) != 0


@pytest.mark.parametrize("n_images,tokens", [(2, 257), (1, 50), (40, 257), (1, 1)])
def test_head_dim_80_attention_writing_the_next_operand_equals_rows_then_the_repack_byte_for_byte(pkg, device, oracle, n_images, tokens):
    """vh_launch_attention_planes_f16_hd80_operand: ViT-H/14's attention writing the output projection's operand itself --
    one-part bf16 planes, or the block-scaled fp8 tensor -- although head_dim 80 does not tile the formats' 32-column
    blocks (a workgroup walks head pairs and carries the even head's last half block in registers).  Must equal the
    fp32-rows kernel followed by vh_launch_split_rows(parts = 1) / vh_launch_quantize_mx_act, byte for byte
    (e4m3 zeros up to their sign)."""
    E, H = 1280, 16
    rows = n_images * tokens
    qkv = oracle.synth_fill(rows * 3 * E, 1511 + tokens, 1.0, 0.0).reshape(rows, 3 * E)
    planes = np.ascontiguousarray(qkv.astype(np.float16).reshape(rows, 3 * E // 32, 32).transpose(1, 0, 2))
    d_qh = pkg.DeviceBuffer.from_numpy(planes.ravel().view(np.float32))
    d_rows = pkg.DeviceBuffer(rows * E)
    _launch(pkg, "vh_launch_attention_planes_f16_hd80", None, d_qh.ptr, d_rows.ptr, n_images, tokens, E, H)
    nb = rows * E
    # one-part bf16 planes
    d_want, d_got = pkg.DeviceBuffer(nb // 2 + 4), pkg.DeviceBuffer(nb // 2 + 4)
    _launch(pkg, "vh_launch_split_rows", None, d_rows.ptr, d_want.ptr, rows, E, 1)
    _launch(pkg, "vh_launch_attention_planes_f16_hd80_operand", None, d_qh.ptr, d_got.ptr, None, 1, n_images, tokens, E, H)
    assert np.array_equal(d_got.to_numpy().view(np.uint16)[:nb], d_want.to_numpy().view(np.uint16)[:nb])
    # block-scaled fp8
    import mx_ref
    sb = mx_ref.act_scale_bytes(rows, E)                         # activation tensors: scale bytes in the activation order
    d_wv, d_ws = pkg.DeviceBuffer(nb // 4 + 4), pkg.DeviceBuffer(sb // 4 + 4)
    d_gv, d_gs = pkg.DeviceBuffer(nb // 4 + 4), pkg.DeviceBuffer(sb // 4 + 4)
    _launch(pkg, "vh_launch_quantize_mx_act", None, d_rows.ptr, d_wv.ptr, d_ws.ptr, rows, E)
    _launch(pkg, "vh_launch_attention_planes_f16_hd80_operand", None, d_qh.ptr, d_gv.ptr, d_gs.ptr, 2, n_images, tokens, E, H)
    wv, gv = d_wv.to_numpy().view(np.uint8)[:nb], d_gv.to_numpy().view(np.uint8)[:nb]
    assert np.array_equal(mx_ref.from_act_layout(d_gs.to_numpy().view(np.uint8), rows, E),
                          mx_ref.from_act_layout(d_ws.to_numpy().view(np.uint8), rows, E))
    zero = (wv & 0x7f) == 0
    assert np.array_equal(gv[~zero], wv[~zero]) and np.array_equal(gv[zero] & 0x7f, wv[zero] & 0x7f)
    L = pkg.lib()
    assert L.vh_launch_attention_planes_f16_hd80_operand(None, d_qh.ptr, d_got.ptr, None, 1, n_images, tokens, 1200, 15) != 0   # odd head count
    assert L.vh_launch_attention_planes_f16_hd80_operand(None, d_qh.ptr, d_gv.ptr, None, 2, n_images, tokens, E, H) != 0        # no scales


@pytest.mark.parametrize("precision", ["f32", "bf16", "fp8", "f32_fp16x2"])
def test_repacked_weights_file_round_trip_is_bit_identical(pkg, device, weights, tmp_path, precision):
    """vit_hip_export_planes / vit_hip_create_from_planes (the offline repack; the reference's loader reads
    152 fp32 files per run, Network.c:134-218): a context built from ONE file of already repacked operands -- three-part
    planes, one-part planes, MX values + scales, fp16 pairs with their per-tensor scales -- gives the same logits and
    probabilities, bit for bit, as the context that wrote it; a truncated or foreign file is refused."""
    cfg = pkg.preset("vit_b_16")
    imgs = pkg.synth_images(cfg, 7, 3)
    a = pkg.ViTHip(cfg, weights, device=0, max_batch=3, precision=precision)
    la, pa = a.forward(imgs)
    path = tmp_path / f"b16_{precision}.planes"
    a.export_planes(path)
    a.close()
    per_weight = {"f32": 6, "bf16": 2, "fp8": 1 + 1 / 32, "f32_fp16x2": 4}[precision]
    big = sum(weights[4 + 12 * l + k].size for l in range(12) for k in (2, 4, 8, 10))
    assert path.stat().st_size >= 4 * sum(w.size for w in weights) + per_weight * big      # fp32 slab + operand slab (+ padding, header)
    b = pkg.ViTHip.from_planes(path, device=0, max_batch=3)
    assert b.precision == precision and b.cfg.embed_dim == 768 and b.cfg.depth == 12
    lb, pb = b.forward(imgs)
    b.close()
    assert np.array_equal(la, lb) and np.array_equal(pa, pb)
    raw = path.read_bytes()
    (tmp_path / "short.planes").write_bytes(raw[:len(raw) // 2])
    (tmp_path / "foreign.planes").write_bytes(b"NOTAPLAN" + raw[8:4096])
    for bad in ("short.planes", "foreign.planes", "missing.planes"):
        with pytest.raises(pkg.VitHipError):
            pkg.ViTHip.from_planes(tmp_path / bad, device=0, max_batch=3)
