"""The lazy last layer on the GPU (csrc/ViT_hip.c, layer_f32_planes / finish_last_layer): by default the fp32 path evaluates
the last layer behind its attention -- and, with the resident three-part attention, Q and the attention themselves -- for the
class-token rows only, and finishes the other rows when somebody reads them.  Everything a caller can observe must be the full
evaluation's ($VIT_HIP_LAST_LAYER=full), bit for bit: logits, probabilities, the residual stream of vit_hip_read_tokens, armed
outputs.  ViT-B/16 at n = 1, 3 and 40 (40 images span several 128-row tiles and a ragged one), both forms of the lazy path
(the default and $VIT_HIP_LAST_LAYER=all_queries), then the two new launchers on their own."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = (1, 3, 40)
MODES = ("default", "all_queries")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _launch(pkg, name, *args):
    L = pkg.lib()
    rc = getattr(L, name)(*args)
    assert rc == 0, f"{name}: {L.vh_last_error().decode()}"
    assert L.vh_device_sync() == 0, L.vh_last_error().decode()


@pytest.fixture(scope="module")
def cfg(pkg):
    return pkg.preset("vit_b_16")


@pytest.fixture(scope="module")
def images(pkg, cfg):
    return pkg.synth_images(cfg, 0, 40)


@pytest.fixture(scope="module")
def models(pkg, device, cfg, weights):
    """Three contexts on the same weights: the default, $VIT_HIP_LAST_LAYER=all_queries and =full (read at creation)"""
    made = {}
    with pytest.MonkeyPatch.context() as mp:
        for mode in (*MODES, "full"):
            if mode == "default":
                mp.delenv("VIT_HIP_LAST_LAYER", raising=False)
            else:
                mp.setenv("VIT_HIP_LAST_LAYER", mode)
            made[mode] = pkg.ViTHip(cfg, weights, device=0, max_batch=40)
    yield made
    for m in made.values():
        m.close()


@pytest.fixture(scope="module")
def full(models, images):
    """The full evaluation, once: {n: (logits, probabilities, residual stream)}; nothing is ever pending there"""
    out = {}
    for n in NS:
        logits, probs = models["full"].forward(images[:n])
        assert models["full"].last_layer_pending() == 0
        out[n] = (logits, probs, models["full"].read_tokens(n))
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", NS)
def test_outputs_and_the_residual_stream_are_the_full_evaluations(models, images, full, mode, n):
    m = models[mode]
    logits, probs = m.forward(images[:n])
    assert m.last_layer_pending() == n                      # the class-rows path ran
    assert same(logits, full[n][0]) and same(probs, full[n][1])
    tokens = m.read_tokens(n)
    assert m.last_layer_pending() == 0
    assert same(tokens, full[n][2])                         # every row, class and patch
    again = m.read_tokens(n)                                # nothing is pending: a plain copy
    assert m.last_layer_pending() == 0 and same(again, tokens)


@pytest.mark.parametrize("mode", MODES)
def test_a_later_forward_with_another_n_is_what_gets_finished(models, images, full, mode):
    m = models[mode]
    m.forward(images[:40])
    m.forward(images[:3])
    assert m.last_layer_pending() == 3
    assert same(m.read_tokens(3), full[3][2])
    m.forward(images[:3])
    m.read_tokens(3)
    logits, _ = m.forward(images[:40])                      # a forward after a finished one starts afresh
    assert m.last_layer_pending() == 40 and same(logits, full[40][0])
    assert same(m.read_tokens(40), full[40][2])


@pytest.mark.parametrize("mode", MODES)
def test_a_request_for_last_layer_patch_tokens_runs_the_full_layer(pkg, models, images, full, cfg, mode):
    b, n, E, T = pkg.binding, 3, cfg.embed_dim, 197
    spec = b.FeatureSpec(taps=(-1,), final_norm=False)
    got = {}
    for name in (mode, "full"):
        m = models[name]
        d_tok, d_cls = pkg.DeviceBuffer(40 * (T - 1) * E), pkg.DeviceBuffer(40 * E)
        d_img, d_l, d_p = pkg.DeviceBuffer.from_numpy(images[:n]), pkg.DeviceBuffer(n * 1000), pkg.DeviceBuffer(n * 1000)
        m.set_features(spec, cls=d_cls, tokens=d_tok)
        try:
            m.forward_device(d_img.ptr, n, d_l.ptr, d_p.ptr)
            m.sync()
        finally:
            m.set_features(None)
        assert m.last_layer_pending() == 0                  # all rows ran inside the forward
        got[name] = (d_l.to_numpy((n, 1000)), d_p.to_numpy((n, 1000)), d_tok.to_numpy()[: n * (T - 1) * E].reshape(n, T - 1, E),
                     d_cls.to_numpy()[: n * E].reshape(n, E), m.read_tokens(n))
    for a, w in zip(got[mode], got["full"]):
        assert same(a, w)
    assert same(got[mode][0], full[n][0]) and same(got[mode][4], full[n][2])
    # final_norm = 0 hands the rows through: the tokens are the residual stream's patch rows
    assert same(got[mode][2], full[n][2].reshape(n, T, E)[:, 1:]) and same(got[mode][3], full[n][2].reshape(n, T, E)[:, 0])
    # the class token alone does not need them: the class-rows path, the compacted rows, the same bits
    m = models[mode]
    d_cls, d_img = pkg.DeviceBuffer(40 * E), pkg.DeviceBuffer.from_numpy(images[:n])
    m.set_features(spec, cls=d_cls)
    try:
        m.forward_device(d_img.ptr, n)
        m.sync()
    finally:
        m.set_features(None)
    assert m.last_layer_pending() == n and same(d_cls.to_numpy()[: n * E].reshape(n, E), got["full"][3])


def test_attention_outputs_of_the_last_layer_read_a_complete_qkv(models, images, full):
    """An attention-map tap on the last layer and the rollout read all of its Q|K|V: such a forward keeps the class-rows path
    behind the attention but projects Q for every row."""
    n = 3
    want = models["full"].attention(images[:n], (0, -1))
    want_roll = models["full"].rollout(images[:n], -2)
    for mode in MODES:
        m = models[mode]
        got = m.attention(images[:n], (0, -1))
        assert m.last_layer_pending() == n
        for a, w in zip(got, want):
            assert same(a, w)
        assert same(m.read_tokens(n), full[n][2])
        assert same(m.rollout(images[:n], -2), want_roll)
        assert same(m.read_tokens(n), full[n][2])


@pytest.mark.parametrize("mode", MODES)
def test_one_image_alone_gets_the_bits_it_gets_in_the_batch(models, images, full, cfg, mode):
    m, i, T = models[mode], 7, 197
    logits, probs = m.forward(images[i:i + 1])
    assert same(logits[0], full[40][0][i]) and same(probs[0], full[40][1][i])
    assert same(m.read_tokens(1), full[40][2][i * T:(i + 1) * T])


# ---- the launchers of the class query -------------------------------------------------------------------------------------

E, H = 768, 12
NAN_BF16 = 0x7FC0


def _at(buf, byte_offset):
    """a device pointer byte_offset into buf"""
    return C.c_void_p(buf.ptr.value + byte_offset)


def _dev(pkg, a):
    return pkg.DeviceBuffer.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _planes(pkg, rows, cols, pad=0):
    """planes [cols/32][3][rows][32] bf16 as a uint16 buffer, `pad` more values behind them; every value a NaN until written"""
    return pkg.DeviceBuffer.from_numpy(np.full(3 * rows * cols + pad, NAN_BF16, np.uint16), np.uint16)


def _gather(pkg, d_planes, byte_offset, cols, rows, n, stride):
    """rows 0, stride, 2 stride, ... of planes [cols/32][3][rows][32] that begin byte_offset into d_planes -> uint16 [cols/32][3][n][32]"""
    d_out = _planes(pkg, n, cols)
    _launch(pkg, "vh_launch_gather_rows", None, _at(d_planes, byte_offset), d_out.ptr, 3 * (cols // 32), rows, n, 64, stride)
    return d_out


@pytest.mark.parametrize("tokens", [197, 33])
def test_class_query_attention_is_row_0_of_the_full_kernel(pkg, device, oracle, tokens):
    """n = 2 images at T = 197 and at T = 33, the smallest shape with two key tiles and a nearly empty last one: the rows of
    vh_launch_attention_planes_cls are rows 0 and T of vh_launch_attention_planes on the same Q|K|V, byte for byte.  The
    class kernel gets the Q planes of the class rows alone -- the Q columns of its Q|K|V are NaNs -- and must not write
    behind its n rows."""
    n, rows = 2, 2 * tokens
    qkv = oracle.synth_fill(rows * 3 * E, 91 + tokens, 1.0, 0.0).reshape(rows, 3 * E)
    d_rows, d_q3 = _dev(pkg, qkv), _planes(pkg, rows, 3 * E)
    _launch(pkg, "vh_launch_split3_rows", None, d_rows.ptr, d_q3.ptr, rows, 3 * E)
    d_full = _planes(pkg, rows, E)
    _launch(pkg, "vh_launch_attention_planes", None, d_q3.ptr, d_full.ptr, n, tokens, E, H)
    want = _gather(pkg, d_full, 0, E, rows, n, tokens).to_numpy()
    assert not (want == NAN_BF16).any()
    d_qc = _gather(pkg, d_q3, 0, E, rows, n, tokens)
    q_bytes = 3 * rows * E * 2                               # the Q planes come first: K steps 0 .. E/32 - 1
    poisoned = d_q3.to_numpy()
    poisoned[: q_bytes // 2] = NAN_BF16
    d_kv = pkg.DeviceBuffer.from_numpy(poisoned, np.uint16)
    pad = 256
    d_out = _planes(pkg, n, E, pad)
    _launch(pkg, "vh_launch_attention_planes_cls", None, d_kv.ptr, d_qc.ptr, d_out.ptr, n, tokens, E, H)
    got = d_out.to_numpy()
    assert np.array_equal(got[: 3 * n * E], want)
    assert (got[3 * n * E:] == NAN_BF16).all()
    L = pkg.lib()
    assert L.vh_launch_attention_planes_cls(None, d_kv.ptr, None, d_out.ptr, n, tokens, E, H) == 1
    assert L.vh_launch_attention_planes_cls(None, d_kv.ptr, _at(d_qc, 8), d_out.ptr, n, tokens, E, H) == 1
    assert L.vh_launch_attention_planes_cls(None, d_kv.ptr, d_qc.ptr, d_out.ptr, n, 209, E, H) == 1


@pytest.mark.parametrize("tokens", [197, 33])
def test_q_on_gathered_rows_and_k_v_by_column_range_equal_the_full_projection(pkg, device, oracle, tokens):
    """vh_launch_linear_p3_cols: K|V (columns E .. 3E) on all rows into their place in Q|K|V, and Q (columns 0 .. E) on the
    gathered class rows, against vh_launch_linear_p3 on the whole in_proj matrix: the same bytes."""
    n, rows, N = 2, 2 * tokens, 3 * E
    y = oracle.synth_fill(rows * E, 300 + tokens, 1.0, 0.1).reshape(rows, E)
    w = oracle.synth_fill(N * E, 301, 0.04, 0.0)
    bias = oracle.synth_fill(N, 302, 0.1, 0.0)
    d_y, d_w, d_b = _dev(pkg, y), _dev(pkg, w), _dev(pkg, bias)
    d_w3, d_y3 = _planes(pkg, N, E), _planes(pkg, rows, E)
    _launch(pkg, "vh_launch_split3_planes", None, d_w.ptr, d_w3.ptr, N, E)
    _launch(pkg, "vh_launch_split3_rows", None, d_y.ptr, d_y3.ptr, rows, E)
    d_full = _planes(pkg, rows, N)
    _launch(pkg, "vh_launch_linear_p3", None, d_full.ptr, 1, d_w3.ptr, d_y3.ptr, d_b.ptr, rows, E, N, 0, None)
    want = d_full.to_numpy()
    q_vals = 3 * rows * E                                    # values in the Q planes, in front of K
    d_part = _planes(pkg, rows, N)
    _launch(pkg, "vh_launch_linear_p3_cols", None, _at(d_part, 2 * q_vals), 1, _at(d_w3, 64 * E), N, d_y3.ptr,
            _at(d_b, 4 * E), rows, E, 2 * E)
    got = d_part.to_numpy()
    assert np.array_equal(got[q_vals:], want[q_vals:]) and (got[:q_vals] == NAN_BF16).all()
    d_yc = _gather(pkg, d_y3, 0, E, rows, n, tokens)
    d_qc = _planes(pkg, n, E)
    _launch(pkg, "vh_launch_linear_p3_cols", None, d_qc.ptr, 1, d_w3.ptr, N, d_yc.ptr, d_b.ptr, n, E, E)
    assert np.array_equal(d_qc.to_numpy(), _gather(pkg, d_full, 0, E, rows, n, tokens).to_numpy())
    assert pkg.lib().vh_launch_linear_p3_cols(None, d_qc.ptr, 1, d_w3.ptr, E // 2, d_yc.ptr, d_b.ptr, n, E, E) == 1
