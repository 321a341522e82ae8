"""Operator-level GPU tests on heavy-tailed inputs (tests/realistic_weights.py's shapes): the cases that catch a kernel
bug before it shows as a mode-level tolerance miss.  Every bound is the one the uniform-input test of the same kernel
asserts (cited at each assertion); only the inputs change.

  * LayerNorm rows at |mean|/std 5 and 30 (the E[x^2] - mean^2 cancellation) with a 50-sigma channel at index 485 (not a
    multiple of 32), gamma / beta of the heavy-tailed set (gamma 0.05x its median at that channel): layernorm_kernel
    against float64 LayerNorm within 2x the port's own fp32 error + 1e-6 max|y| (both use E[x^2] - mean^2 and cancel alike),
    and the bit-equality properties of layer_norm_p3 (3 parts), layer_norm_planes (1 part) and LN -> MX.
  * GEMMs with weights of kurtosis >= 8 and outlier input columns x8-16, activations with a dominant channel: the exact
    three-part path, the fp16-pair emulation (its per-tensor scale chosen from amax as context creation does), one-part
    bf16 planes and block-scaled fp8.
  * Attention with a sink: one key outscores every other by >= 20 for every query of every head, and V has a massive
    channel: the resident and streaming fp32 kernels against the port, the planes forms bit for bit against them, the
    fp16-operand forms against theirs, attention_long in test_gpu_long_seq.py ("sink" case)."""
import math

import numpy as np
import pytest

import mx_ref
import realistic_weights as rw
from test_gpu_p3 import _bf16_rne, _dev, _launch, _planes1_to_f32, _planes_buf, _planes_to_parts

pytestmark = pytest.mark.gpu

OP_TOL = 2e-5
DSTAR = 485


def _heavy_matrix(oracle, N, K, seed, sigma=0.023):
    """kurtosis >= 8 (sign(u) E^1.3) with four outlier input columns x8, x10, x12, x16 (uniform-shaped, as in the set)"""
    w = sigma * rw._heavy(N * K, seed, rw.P_MATRIX).reshape(N, K)
    for g, col in zip(rw.OUTLIER_GAINS, (7, K // 3 + 5, K // 2 + 17, K - 9)):
        w[:, col] = g * sigma * math.sqrt(3.0) * rw._uniform(N, seed + 0x6000 + col)
    w = w.astype(np.float32)
    assert rw.tensor_stats(w)["kurtosis"] >= 8.0
    return w


def _dominant_rows(oracle, M, K, seed, value=12.0):
    x = oracle.synth_fill(M * K, seed, 1.0, 0.1).reshape(M, K)
    x[:, DSTAR % K] = value
    return x


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------

def _ln_inputs(oracle, rows, E=768):
    """rows alternating |mean|/std 5 and 30; every other pair with a 50-sigma channel at DSTAR"""
    x = oracle.synth_fill(rows * E, 4242 + rows, math.sqrt(3.0), 0.0).reshape(rows, E).astype(np.float64)   # sigma 1
    for r in range(rows):
        x[r] += (5.0, 30.0)[r % 2] * (1.0 if r % 3 else -1.0)
        if (r // 2) % 2:
            x[r, DSTAR] = x[r].mean() + 50.0
    return x.astype(np.float32)


def _gamma_beta():
    import __graft_entry__ as graft
    cfg = graft.load_package().preset("vit_b_16")
    cfg.depth = 1
    ws = rw.realistic_weights(cfg, 0)
    assert rw.plan(cfg, 0)["dstar"] == DSTAR
    return ws[4], ws[5]


def _ln64(x, g, b, eps=1e-6):
    x = x.astype(np.float64)
    mean = x.mean(1, keepdims=True)
    var = (x * x).mean(1, keepdims=True) - mean * mean
    return (x - mean) / np.sqrt(var + eps) * g.astype(np.float64) + b.astype(np.float64)


@pytest.mark.parametrize("rows", [4, 197, 1000])
def test_layer_norm_kernels_on_heavy_rows(pkg, device, oracle, rows):
    E = 768
    x = _ln_inputs(oracle, rows, E)
    g, b = _gamma_beta()
    d_x, d_g, d_b = _dev(pkg, x), _dev(pkg, g), _dev(pkg, b)
    d_y = pkg.DeviceBuffer(rows * E)
    _launch(pkg, "vh_launch_layer_norm", None, d_x.ptr, d_g.ptr, d_b.ptr, d_y.ptr, rows, E, E, E, 1e-6)
    y = d_y.to_numpy((rows, E))
    want = _ln64(x, g, b)
    port = oracle.layer_norm(x, g, b)
    # per kind of row (|mean|/std 5 or 30, with or without the 50-sigma channel): a single row can be rounded luckily by
    # the port, so the two error levels are compared over the rows of one kind, not row by row
    kind = np.array([(r % 2, (r // 2) % 2) for r in range(rows)])
    e_gpu, e_port = np.abs(y - want).max(1), np.abs(port - want).max(1)
    for k in sorted({tuple(v) for v in kind}):
        sel = (kind == k).all(1)
        print(f"\nheavy LayerNorm rows |mean|/std {(5, 30)[k[0]]}, 50-sigma channel {bool(k[1])}: GPU error max "
              f"{e_gpu[sel].max():.2e}, port fp32 error max {e_port[sel].max():.2e}")
        assert e_gpu[sel].max() <= 2.0 * e_port[sel].max() + 1e-6 * np.abs(want).max(), k
    # layer_norm_p3: the exact three-part split of the same values (test_layer_norm_p3_equals_layer_norm_split)
    d_p, d_m = _planes_buf(pkg, rows, E), pkg.DeviceBuffer(rows * E)
    _launch(pkg, "vh_launch_layer_norm_p3", None, d_x.ptr, d_g.ptr, d_b.ptr, d_p.ptr, rows, E, E, 1e-6)
    _launch(pkg, "vh_launch_merge3_rows", None, d_p.ptr, d_m.ptr, rows, E)
    parts = _planes_to_parts(d_p, rows, E)
    assert np.array_equal(parts[0].astype(np.float64) + parts[1] + parts[2], y.astype(np.float64))
    assert np.array_equal(d_m.to_numpy((rows, E)), y + 0.0)
    # one part: bf16 of the fp32 result (test_layer_norm_and_attention_one_part_planes_are_the_rounded_fp32_results)
    d_p1 = pkg.DeviceBuffer(rows * E // 2)
    _launch(pkg, "vh_launch_layer_norm_planes", None, d_x.ptr, d_g.ptr, d_b.ptr, d_p1.ptr, 1, rows, E, E, 1e-6)
    assert np.array_equal(_planes1_to_f32(d_p1, rows, E), _bf16_rne(y))
    # LN -> MX: the numpy quantiser of the fp32 result (test_layer_norm_mx_is_layer_norm_then_the_numpy_quantiser)
    d_v, d_s = pkg.DeviceBuffer(rows * E // 4 + 4), pkg.DeviceBuffer(mx_ref.act_scale_bytes(rows, E) // 4 + 4)
    _launch(pkg, "vh_launch_layer_norm_mx", None, d_x.ptr, d_g.ptr, d_b.ptr, d_v.ptr, d_s.ptr, rows, E, E, 1e-6)
    want_v, want_s = mx_ref.quantize(y)
    got_v = d_v.to_numpy().view(np.uint8)[:rows * E].reshape(E // 128, rows, 128)
    assert np.array_equal(mx_ref.from_act_layout(d_s.to_numpy().view(np.uint8), rows, E), want_s)
    zero = (want_v & 0x7f) == 0
    assert np.array_equal(got_v[~zero], want_v[~zero]) and np.array_equal(got_v[zero] & 0x7f, want_v[zero] & 0x7f)


# ---- GEMMs ---------------------------------------------------------------------------------------------------------------

GEMM_SHAPES = [(197, 768, 2304, 0, False), (300, 768, 3072, 1, False), (300, 3072, 768, 0, True)]


def _gemm_inputs(oracle, M, K, N):
    x = _dominant_rows(oracle, M, K, 1300 + M)
    w = _heavy_matrix(oracle, N, K, 1301 + N)
    b = oracle.synth_fill(N, 1302, 0.1, 0.0)
    r = oracle.synth_fill(M * N, 1303, 1.0, 0.0).reshape(M, N)
    return x, w, b, r


def _oracle_out(oracle, x, w, b, r, N, gelu, resid):
    want = oracle.linear(x, w.ravel(), b, N)
    if gelu:
        want = oracle.gelu(want.ravel()).reshape(x.shape[0], N)
    return r + want if resid else want


@pytest.mark.parametrize("M,K,N,gelu,resid", GEMM_SHAPES)
def test_linear_p3_and_fp16_pairs_on_heavy_weights_vs_oracle(pkg, device, oracle, M, K, N, gelu, resid):
    """The exact path (three-part planes; bit for bit against its in-loop-split twin) and the fp16-pair emulation
    (scale 2^(14 - e) from the tensor's amax, as context creation picks it) against the oracle: the fp32 operator
    tolerance 2e-5 on O(1) values, taken relative to max(1, max|y|) as test_linear_mx_vs_float64_* does."""
    x, w, b, r = _gemm_inputs(oracle, M, K, N)
    want = _oracle_out(oracle, x, w, b, r, N, gelu, resid)
    tol = OP_TOL * max(1.0, float(np.abs(want).max()))
    d_x, d_w, d_b = _dev(pkg, x), _dev(pkg, w), _dev(pkg, b)
    d_w3, d_x3 = _planes_buf(pkg, N, K), _planes_buf(pkg, M, K)
    _launch(pkg, "vh_launch_split3_planes", None, d_w.ptr, d_w3.ptr, N, K)
    _launch(pkg, "vh_launch_split3_rows", None, d_x.ptr, d_x3.ptr, M, K)
    d_ref = _dev(pkg, r) if resid else pkg.DeviceBuffer(M * N)
    _launch(pkg, "vh_launch_linear_w3", None, d_ref.ptr, d_w3.ptr, d_x.ptr, d_b.ptr, M, K, N, gelu, d_ref.ptr if resid else None)
    d_o = _dev(pkg, r) if resid else pkg.DeviceBuffer(M * N)
    _launch(pkg, "vh_launch_linear_p3", None, d_o.ptr, 0, d_w3.ptr, d_x3.ptr, d_b.ptr, M, K, N, gelu, d_o.ptr if resid else None)
    got = d_o.to_numpy((M, N))
    assert np.array_equal(got, d_ref.to_numpy((M, N)) + 0.0)
    e3 = float(np.abs(got - want).max())
    _, e = math.frexp(float(np.abs(w).max()))
    scale = 2.0 ** (14 - e)
    d_w2, d_h = pkg.DeviceBuffer(N * K), _dev(pkg, r) if resid else pkg.DeviceBuffer(M * N)
    _launch(pkg, "vh_launch_split2h_planes", None, d_w.ptr, d_w2.ptr, N, K, scale)
    _launch(pkg, "vh_launch_linear_h2", None, d_h.ptr, d_w2.ptr, scale, d_x.ptr, d_b.ptr, M, K, N, gelu, d_h.ptr if resid else None)
    e2 = float(np.abs(d_h.to_numpy((M, N)) - want).max())
    print(f"\nheavy GEMM {M}x{K}x{N}: three-part {e3:.2e}, fp16 pairs {e2:.2e} (bound {tol:.2e}, max|y| {np.abs(want).max():.2f})")
    assert e3 <= tol and e2 <= tol


@pytest.mark.parametrize("M,K,N,gelu,resid", GEMM_SHAPES)
def test_linear_one_part_and_mx_on_heavy_weights(pkg, device, oracle, M, K, N, gelu, resid):
    """One-part bf16 planes against the oracle on the same rounded operands (fp32 operator tolerance, as
    test_linear_planes_one_part_vs_oracle_on_bf16_rounded_operands); block-scaled fp8 against float64 products of the
    dequantised operands: 2e-5 max(1, max|y|) (test_linear_mx_vs_float64_*), plus the matrix core's known loss on rows
    with a dominant product, 2^-11 of the row's largest |x w| (v_mfma_scale_f32_16x16x128_f8f6f4 sums in a fixed-point
    frame hung on the largest product: the bound test_gpu_fold.py's MX consumer test states for such rows)."""
    x, w, b, r = _gemm_inputs(oracle, M, K, N)
    d_b = _dev(pkg, b)
    d_x, d_w = _dev(pkg, x), _dev(pkg, w)
    d_w1, d_x1 = pkg.DeviceBuffer((N * K + 1) // 2), pkg.DeviceBuffer((M * K + 1) // 2)
    _launch(pkg, "vh_launch_split_rows", None, d_w.ptr, d_w1.ptr, N, K, 1)
    _launch(pkg, "vh_launch_split_rows", None, d_x.ptr, d_x1.ptr, M, K, 1)
    xr, wr = _planes1_to_f32(d_x1, M, K), _planes1_to_f32(d_w1, N, K)
    assert np.array_equal(xr, _bf16_rne(x)) and np.array_equal(wr, _bf16_rne(w))
    d_o = _dev(pkg, r) if resid else pkg.DeviceBuffer(M * N)
    _launch(pkg, "vh_launch_linear_planes", None, d_o.ptr, 0, d_w1.ptr, d_x1.ptr, 1, d_b.ptr, M, K, N, gelu, d_o.ptr if resid else None)
    want1 = _oracle_out(oracle, xr, wr, b, r, N, gelu, resid)
    e1 = float(np.abs(d_o.to_numpy((M, N)) - want1).max())
    tol1 = OP_TOL * max(1.0, float(np.abs(want1).max()))
    if K % 256 == 0 and N % 128 == 0:
        d_xv, d_xs = pkg.DeviceBuffer(M * K // 4 + 4), pkg.DeviceBuffer(mx_ref.act_scale_bytes(M, K) // 4 + 4)
        d_wv, d_ws = pkg.DeviceBuffer(N * K // 4 + 4), pkg.DeviceBuffer(N * K // 128 + 4)
        _launch(pkg, "vh_launch_quantize_mx_act", None, d_x.ptr, d_xv.ptr, d_xs.ptr, M, K)
        _launch(pkg, "vh_launch_quantize_mx_rows", None, d_w.ptr, d_wv.ptr, d_ws.ptr, N, K)
        xq, wq = mx_ref.dequantize(*mx_ref.quantize(x)), mx_ref.dequantize(*mx_ref.quantize(w))
        want8 = xq.astype(np.float64) @ wq.astype(np.float64).T + b
        if gelu:
            want8 = 0.5 * want8 * (1.0 + np.vectorize(math.erf)(want8 / math.sqrt(2.0)))
        if resid:
            want8 = r + want8
        d_o8 = _dev(pkg, r) if resid else pkg.DeviceBuffer(M * N)
        _launch(pkg, "vh_launch_linear_mx", None, d_o8.ptr, None, d_wv.ptr, d_ws.ptr, d_xv.ptr, d_xs.ptr, d_b.ptr, M, K, N, gelu,
                d_o8.ptr if resid else None)
        big = np.abs(xq).max(1) * np.abs(wq).max()
        err8 = np.abs(d_o8.to_numpy((M, N)) - want8).max(1)
        tol8 = OP_TOL * max(1.0, float(np.abs(want8).max())) + 2.0 ** -11 * big
        print(f"\nheavy GEMM {M}x{K}x{N}: one-part {e1:.2e} (bound {tol1:.2e}); MX worst row {err8.max():.2e} (bound {tol8.min():.2e})")
        assert (err8 <= tol8).all()
    assert e1 <= tol1


# ---- attention with a sink ---------------------------------------------------------------------------------------------

def _sink_qkv(oracle, n, T, E, H, seed, sink=3):
    """Q, K, V ~ 1; every query has a common direction u per head, key `sink` of every image is +c u with c such that its
    score exceeds every other by >= 20; channel 5 of every head's V is x40."""
    D = E // H
    x = oracle.synth_fill(n * T * 3 * E, seed, 1.0, 0.0).reshape(n, T, 3, H, D).astype(np.float64)
    x[:, :, 0] += 1.0
    x[:, sink, 1] += 40.0 / math.sqrt(D)
    x[:, :, 2, :, 5] *= 40.0
    x = x.astype(np.float32)
    s = np.einsum("btha,bsha->bhts", x[:, :, 0].astype(np.float64), x[:, :, 1].astype(np.float64)) / math.sqrt(D)
    others = np.delete(s, sink, axis=3).max(axis=3)
    assert (s[..., sink] - others >= 20.0).all()
    return np.ascontiguousarray(x.reshape(n * T, 3 * E))


@pytest.mark.parametrize("preset,n,T", [("vit_b_16", 2, 197), ("vit_b_16", 1, 208), ("vit_b_16", 2, 257), ("vit_h_14", 2, 257)])
def test_fp32_attention_kernels_with_a_sink_vs_port(pkg, device, preset, n, T):
    """vh_launch_attention (resident kernel at T <= 208 with head_dim 64, streaming kernel otherwise) against the port:
    2e-5 of max(1, max|O|) (test_attention_vs_oracle's operator tolerance on O(1) values); at head_dim 64 the p3 and
    planes forms bit for bit against it (test_attention_p3_equals_attention_split, test_attention_on_planes_*)."""
    from oracle.oracle import Oracle
    orc = Oracle(preset)
    E, H = orc.cfg.embed_dim, orc.cfg.num_heads
    qkv = _sink_qkv(orc, n, T, E, H, 5150 + T)
    rows = n * T
    d_q, d_o = _dev(pkg, qkv), pkg.DeviceBuffer(rows * E)
    _launch(pkg, "vh_launch_attention", None, d_q.ptr, d_o.ptr, n, T, E, H)
    got = d_o.to_numpy((rows, E))
    want = np.concatenate([orc.attention(qkv[i * T:(i + 1) * T]) for i in range(n)])
    err = float(np.abs(got - want).max())
    print(f"\nsink attention {preset} T={T}: max |d| {err:.2e} of max|O| {np.abs(want).max():.1f}")
    assert np.isfinite(got).all() and err <= OP_TOL * max(1.0, float(np.abs(want).max()))
    if E // H == 64 and T <= 208:
        d_p, d_m = _planes_buf(pkg, rows, E), pkg.DeviceBuffer(rows * E)
        _launch(pkg, "vh_launch_attention_p3", None, d_q.ptr, d_p.ptr, n, T, E, H)
        _launch(pkg, "vh_launch_merge3_rows", None, d_p.ptr, d_m.ptr, rows, E)
        assert np.array_equal(d_m.to_numpy((rows, E)), got + 0.0)
        d_q3, d_p2, d_m2 = _planes_buf(pkg, rows, 3 * E), _planes_buf(pkg, rows, E), pkg.DeviceBuffer(rows * E)
        _launch(pkg, "vh_launch_split3_rows", None, d_q.ptr, d_q3.ptr, rows, 3 * E)
        _launch(pkg, "vh_launch_attention_planes", None, d_q3.ptr, d_p2.ptr, n, T, E, H)
        _launch(pkg, "vh_launch_merge3_rows", None, d_p2.ptr, d_m2.ptr, rows, E)
        assert np.array_equal(d_m2.to_numpy((rows, E)), got + 0.0)


@pytest.mark.parametrize("n,T", [(2, 197), (2, 257)])
def test_fp16_operand_attention_kernels_with_a_sink(pkg, device, oracle, n, T):
    """The reduced modes' attention on sink inputs.  head_dim 64, T = 197: the fp16-planes kernel bit for bit against the
    fp16-operand kernel on rows (test_attention_on_fp16_planes_*).  head_dim 80 (ViT-H/14): the resident fp16 kernel
    within 2^-12 of max|O| of the streaming fp16 form and 2^-9 of the fp32 kernel (test_resident_fp16_planes_*)."""
    from test_gpu_p3 import _f16_planes_dev
    E, H = (768, 12) if T == 197 else (1280, 16)
    qkv = _sink_qkv(oracle, n, T, E, H, 6150 + T)
    rows = n * T
    d_q = _dev(pkg, qkv)
    d_a, d_b = pkg.DeviceBuffer(rows * E), pkg.DeviceBuffer(rows * E)
    _launch(pkg, "vh_launch_attention", None, d_q.ptr, d_a.ptr, n, T, E, H)
    _launch(pkg, "vh_launch_attention_f16", None, d_q.ptr, d_b.ptr, n, T, E, H)
    a, b = d_a.to_numpy((rows, E)), d_b.to_numpy((rows, E))
    big = float(np.abs(a).max())
    if T == 197:
        d_qh, d_c = _f16_planes_dev(pkg, qkv), pkg.DeviceBuffer(rows * E)
        _launch(pkg, "vh_launch_attention_planes_f16", None, d_qh.ptr, d_c.ptr, 0, n, T, E, H)
        assert np.array_equal(d_c.to_numpy((rows, E)), b)
    else:
        planes = np.ascontiguousarray(qkv.astype(np.float16).reshape(rows, 3 * E // 32, 32).transpose(1, 0, 2))
        d_qh, d_c = pkg.DeviceBuffer.from_numpy(planes.ravel().view(np.float32)), pkg.DeviceBuffer(rows * E)
        _launch(pkg, "vh_launch_attention_planes_f16_hd80", None, d_qh.ptr, d_c.ptr, n, T, E, H)
        c = d_c.to_numpy((rows, E))
        print(f"\nsink attention hd80 fp16: vs fp16 rows {np.abs(c - b).max():.2e}, vs fp32 {np.abs(c - a).max():.2e} of {big:.1f}")
        assert np.abs(c - b).max() <= 2.0 ** -12 * big and np.abs(c - a).max() <= 2.0 ** -9 * big
    assert np.isfinite(b).all() and np.abs(a - b).max() <= 2.0 ** -9 * big
