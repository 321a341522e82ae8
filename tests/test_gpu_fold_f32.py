"""The LayerNorm fold on exact three-part planes (csrc/norm_fold.h on the fp32 path: $VIT_HIP_LN_FOLD=1, or a planes file
written with the fold on; the only fp32 planes path for embed_dim above vh_layer_norm_planes_max_embed(3)), per operator
against float64 -- the twin of tests/test_gpu_fold.py, whose float64 statements are imported, not restated:

1. column terms: vh_launch_fold_gamma -> vh_launch_split3_rows -> vh_launch_colsum_planes3, vh_launch_fold_bias;
2. the producer vh_launch_linear_p3_resid_norm: rows bit for bit those of vh_launch_linear_p3(residual), operand planes byte
   for byte vh_launch_split3_rows of those rows, partial sums of every row, guard bands, tile independence;
3. the consumer vh_launch_linear_p3_norm at 1 .. 16 partial sums per row and in the 256x256 classes, against the folded
   formula in float64 on the same operands (sharp: indexing, staging, tiles) and against LayerNorm -> Linear in float64
   (accuracy: the x - mean cancellation, which on fp32 operands is the whole error), with the unfolded pair
   vh_launch_layer_norm_p3 -> vh_launch_linear_p3 measured beside it;
4. the patch embedding's operand forms, class-token rows included;
5. whole contexts at a width only the fold can run;
6. refusals.

Every case takes its tile class from the library at the device's CU count and asserts the class it was written for; the
large shapes are derived from the rule (20300 / 13700 / 15000 rows on 256 CUs).  The float64 emulation of the consumer's
formula runs without a GPU (test_emulated_fp32_fold_sits_under_half_the_accuracy_bound)."""
import ctypes as C

import numpy as np
import pytest

import gemm_tiles_ref as tiles
from test_gpu_fold import EPS, _consumer_rows, _folded_reference, _gelu64, _ln_rows, _residual_rows
from test_gpu_p3 import OP_TOL, _cus, _dev, _launch, _planes_buf, _planes_to_parts, _tile_class
from test_gpu_u8_input import _as_layout, _normalised

gpu = pytest.mark.gpu

PATTERN = 0xA5A5A5A5          # guard-band filler: a normal fp32 (-2.87e-16), so no copy canonicalises it
ROW_LIMIT = 25000             # no large case above this many rows
ENV = ("VIT_HIP_P3", "VIT_HIP_GEMM_FP32", "VIT_HIP_ATTN", "VIT_HIP_LN_FOLD", "VIT_HIP_LAST_LAYER", "VIT_HIP_PRECISION")
MEAN4, STD4 = (0.485, 0.456, 0.406, 0.31), (0.229, 0.224, 0.225, 0.27)

# consumer shapes (M, K, N): K / 128 = partial sums per row
CONSUMER_SMALL = [(1, 128, 128),       # 1
                  (17, 256, 384),      # 2
                  (131, 640, 256),     # 5: lane 0 adds two, the others one
                  (300, 768, 2304),    # 6
                  (257, 1280, 384),    # 10
                  (300, 2048, 256)]    # 16, the maximum
# The folded path's largest error over rows with amp <= 1.5 against the float64 LayerNorm -> Linear, as a multiple of the
# unfolded pair's (vh_launch_layer_norm_p3 -> vh_launch_linear_p3) on the same rows: measured on the MI355X per shape
# (profiles/fold_f32_operator_errors.txt: 0.77 .. 1.52, the largest at 300 x 768 x 2304), asserted with a margin of 2 x --
# the kernels are deterministic, the margin covers the summation orders of other shapes, not noise.
FOLD_VS_UNFOLDED_MAX = 2 * 1.52


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)


def _edge_rows(oracle, M, K, seed):
    """_residual_rows (row 1: |mean| / std ~ 5; row 3: one channel at 40) with three more edge rows where M allows:
    row 4 all zero, row 5 constant 2.5 (sums exact in any order: var = 0), row 6 = 6.0 + 0.05 noise (rms / std ~ 120).
    No constant row whose square is inexact in fp32: E[x^2] - mean^2 may then fall below -eps in any summation order, in
    layer_norm_seq's own formula (ViT_seq.c:132-135) as in the kernel's -- a property of the formula this project copies
    on purpose, not of the fold."""
    x = _residual_rows(oracle, M, K, seed)
    if M >= 8:
        x[4] = 0.0
        x[5] = 2.5
        noise = oracle.synth_fill(K, seed + 3, 1.0, 0.0).astype(np.float64)
        x[6] = (6.0 + 0.05 * noise / noise.std()).astype(np.float32)      # unit-variance noise: std 0.05
    return x


EDGE = (3, 4, 5, 6)


def _amp(x, eps=EPS):
    """rms(x_row) / sqrt(var_row + eps): how much larger the relative error of var = E[x^2] - mean^2 is than that of E[x^2]"""
    x = x.astype(np.float64)
    ms = (x * x).mean(1)
    var = ms - x.mean(1) ** 2
    return np.sqrt(ms) / np.sqrt(np.maximum(var, 0.0) + eps)


def _column_terms64(w, gamma, beta, b):
    """context creation in numpy: W' = fp32(gamma . W), colsum of W' and the folded bias (float64 sums, rounded once)"""
    wp = (w * gamma[None, :]).astype(np.float32)
    cs = wp.astype(np.float64).sum(1).astype(np.float32)
    bf = (b + w.astype(np.float64) @ beta.astype(np.float64)).astype(np.float32)
    return wp, cs, bf


def _stats32(x):
    """[K/128][M][2] partial (sum, sum of squares) in fp32 in the order the GEMM epilogue of the producers adds them
    (csrc/gemm_p3.hip, OPER): of a row's 128 columns lane q = 0..3 holds columns 32 s + 8 q .. + 7 for s = 0..3 and adds their
    even and odd elements apart, in ascending order, squares by fma; then even + odd, then (lane 0 + 1) + (lane 2 + 3)"""
    M, K = x.shape
    v = x.astype(np.float32).reshape(M, K // 128, 4, 4, 4, 2)          # [row][group][s][q][pair][even | odd]
    su, sq = np.zeros((M, K // 128, 4, 2), np.float32), np.zeros((M, K // 128, 4, 2), np.float32)
    for s in range(4):
        for e in range(4):
            t = v[:, :, s, :, e, :]
            su = su + t
            sq = (t.astype(np.float64) ** 2 + sq).astype(np.float32)   # fma: the square is exact in float64
    lane = np.stack([su[..., 0] + su[..., 1], sq[..., 0] + sq[..., 1]], axis=-1)      # [row][group][q][2]
    return ((lane[:, :, 0] + lane[:, :, 1]) + (lane[:, :, 2] + lane[:, :, 3])).transpose(1, 0, 2)


def _consumer_inputs(oracle, M, K, N):
    x = _edge_rows(oracle, M, K, 1810 + M)
    gamma = (1.0 + oracle.synth_fill(K, 1811, 0.3, 0.0)).astype(np.float32)
    beta = oracle.synth_fill(K, 1812, 0.2, 0.0)
    w = oracle.synth_fill(N * K, 1813 + N, 0.04, 0.0).reshape(N, K)
    b = oracle.synth_fill(N, 1814, 0.1, 0.0)
    return x, gamma, beta, w, b


def _tol_accuracy(x, ref):
    return (OP_TOL + 2.0 ** -23 * _amp(x) ** 2) * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("M,K,N", CONSUMER_SMALL)
def test_emulated_fp32_fold_sits_under_half_the_accuracy_bound(oracle, M, K, N):
    """No GPU: the consumer's formula in numpy fp32 -- fp32 partial sums per 128 columns, the row terms of
    _folded_reference (fp32, the kernel's order), an fp32-accumulating x W'^T, the result rounded to fp32 -- against
    _ln_rows(x) W^T + b in float64, per row, as a fraction of comparison (b)'s bound.  The bound is never met by the
    formula's own fp32 noise: every row stays under half of it (typical rows 0.02; the rms / std ~ 120 row 0.11 .. 0.48, the
    largest at K = 1280 -- a few units in the last place of E[x^2] = 36 against var = 0.0025; on the MI355X that row
    measures 0.11 .. 0.64: profiles/fold_f32_operator_errors.txt).
    (The epilogue's own two fma roundings, 2^-24 of the cancelling terms, are not emulated: amp times smaller.)"""
    x, gamma, beta, w, b = _consumer_inputs(oracle, M, K, N)
    wp, cs, bf = _column_terms64(w, gamma, beta, b)
    acc = x @ wp.T                                    # fp32 accumulation
    assert acc.dtype == np.float32
    # _folded_reference forms x_oper w_oper^T itself: handing it the fp32 sums and the identity leaves them as they are
    got = _folded_reference(acc, _stats32(x), np.eye(N, dtype=np.float32), cs, bf, K).astype(np.float32)
    ref = _ln_rows(x, gamma, beta) @ w.astype(np.float64).T + b
    ratio = np.abs(got - ref).max(1) / _tol_accuracy(x, ref)
    worst = int(np.argmax(ratio))
    print(f"\nfold_f32 emulation {M}x{K}x{N}: worst row {worst} amp {_amp(x)[worst]:.2f} at {ratio[worst]:.3f} of the bound, "
          f"median row {np.median(ratio):.3f}")
    assert ratio.max() < 0.5


# ---- device helpers ---------------------------------------------------------------------------------------------------------


class _Guarded:
    """`count` fp32 words on the device between two guard bands of `guard` words, everything filled with PATTERN (or the
    payload with `init`); to_numpy() checks that both bands still hold the pattern and returns the payload"""

    def __init__(self, pkg, count, guard, init=None):
        assert guard % 2 == 0
        full = np.full(count + 2 * guard, PATTERN, np.uint32).view(np.float32)
        if init is not None:
            full[guard:guard + count] = np.ascontiguousarray(init, dtype=np.float32).ravel()
        self.count, self.guard = count, guard
        self.buf = pkg.DeviceBuffer.from_numpy(full)
        self.ptr = C.c_void_p(self.buf.ptr.value + 4 * guard)

    def to_numpy(self, shape=None):
        raw = self.buf.to_numpy()
        g = self.guard
        bands = np.concatenate([raw[:g], raw[g + self.count:]]).view(np.uint32)
        assert (bands == PATTERN).all(), f"{int((bands != PATTERN).sum())} guard words overwritten"
        out = raw[g:g + self.count]
        return out.reshape(shape) if shape is not None else out


def _raw_planes(buf, rows, cols):
    """three-part planes as stored: uint16 [cols/32][3][rows][32]"""
    return buf.to_numpy().view(np.uint16)[:3 * rows * cols].reshape(cols // 32, 3, rows, 32)


def _split3(pkg, x):
    M, K = x.shape
    d_x, d_p = _dev(pkg, x), _planes_buf(pkg, M, K)
    _launch(pkg, "vh_launch_split3_rows", None, d_x.ptr, d_p.ptr, M, K)
    return d_p


def _assert_stats(st, x):
    """stats [N/128][M][2] against float64 sums of the fp32 rows x [M][N], every row: the bf16 test's two bounds"""
    M, N = x.shape
    x64 = x.astype(np.float64).reshape(M, N // 128, 128)
    e_sum = np.abs(st[:, :, 0].T - x64.sum(2)).max() / (1e-5 * max(1.0, np.abs(x64).sum(2).max()))
    e_sq = np.abs(st[:, :, 1].T - (x64 * x64).sum(2)).max() / (1e-5 * max((x64 * x64).sum(2).max(), 1e-300))
    assert e_sum <= 1.0 and e_sq <= 1.0, f"partial sums at {e_sum:.3f}, squares at {e_sq:.3f} of their bounds"
    return e_sum, e_sq


def _rows_for_class(parts, resid, small_only, N, classes, ragged):
    """the smallest row count (mtiles - 1) * 256 + ragged at which the tile rule gives one of `classes` on this device"""
    cus = _cus()
    for mt in range(1, ROW_LIMIT // 256 + 2):
        M = (mt - 1) * 256 + ragged
        if M <= ROW_LIMIT and tiles.tile_class(tiles.PLANES, parts, resid, small_only, M, N, cus)[0] in classes:
            return M
    return None


# ---- 1. column terms ----------------------------------------------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("N,K", [(128, 128), (384, 640), (2304, 768), (256, 2048)])
def test_column_terms_of_three_part_weights(pkg, device, oracle, N, K):
    """what context creation does on the fp32 path: gamma into W (fp32), the exact split, colsum of the values the planes
    hold, the folded bias from the original weights"""
    w = oracle.synth_fill(N * K, 1700 + N, 0.04, 0.0).reshape(N, K)
    gamma = (1.0 + oracle.synth_fill(K, 1701, 0.3, 0.0)).astype(np.float32)
    beta = oracle.synth_fill(K, 1702, 0.2, 0.0)
    b = oracle.synth_fill(N, 1703, 0.1, 0.0)
    d_w, d_g, d_be, d_b = (_dev(pkg, v) for v in (w, gamma, beta, b))
    d_ws, d_w3, d_cs, d_bf = pkg.DeviceBuffer(N * K), _planes_buf(pkg, N, K), pkg.DeviceBuffer(N), pkg.DeviceBuffer(N)
    _launch(pkg, "vh_launch_fold_gamma", None, d_w.ptr, d_g.ptr, d_ws.ptr, N, K)
    _launch(pkg, "vh_launch_split3_rows", None, d_ws.ptr, d_w3.ptr, N, K)
    _launch(pkg, "vh_launch_colsum_planes3", None, d_w3.ptr, d_cs.ptr, N, K)
    _launch(pkg, "vh_launch_fold_bias", None, d_w.ptr, d_be.ptr, d_b.ptr, d_bf.ptr, N, K)
    held = _planes_to_parts(d_w3, N, K).astype(np.float64).sum(0)             # the values the planes hold
    assert np.array_equal(held, (w * gamma[None, :]).astype(np.float64))      # = fp32(w gamma), exactly
    cs, bf = d_cs.to_numpy(), d_bf.to_numpy()
    e_cs = np.abs(cs - held.sum(1)).max()
    print(f"\nfold_f32 column terms {N}x{K}: colsum error {e_cs:.3e} (bound {1e-6 * np.abs(held).sum(1).max():.3e})")
    assert e_cs <= 1e-6 * np.abs(held).sum(1).max()
    assert np.abs(bf - (b + w.astype(np.float64) @ beta.astype(np.float64))).max() <= 1e-6


# ---- 2. the producer -----------------------------------------------------------------------------------------------------------


def _produce(pkg, d_a3, d_w3, d_b, r, M, K, N, in_place=True):
    """vh_launch_linear_p3_resid_norm into guarded outputs -> (guarded fp32 rows, guarded operand planes, guarded stats)"""
    g_x = _Guarded(pkg, M * N, N, init=r if in_place else None)
    d_r = g_x if in_place else _dev(pkg, r)
    g_op, g_st = _Guarded(pkg, 3 * M * N // 2, 3 * N // 2), _Guarded(pkg, (N // 128) * M * 2, 2 * (N // 128))
    _launch(pkg, "vh_launch_linear_p3_resid_norm", None, g_x.ptr, d_w3.ptr, d_a3.ptr, d_b.ptr, d_r.ptr, M, K, N, g_op.ptr, g_st.ptr)
    return g_x, g_op, g_st


PRODUCER_SMALL = [(1, 64, 128, True), (131, 128, 256, True), (257, 3072, 640, True), (300, 768, 768, False), (300, 768, 1280, True),
                  (129, 2048, 2048, True)]


@gpu
@pytest.mark.parametrize("M,K,N,in_place", PRODUCER_SMALL + [("large", 2048, 2048, True)])
def test_p3_producer_leaves_rows_exact_planes_and_partial_sums(pkg, device, oracle, M, K, N, in_place):
    """vh_launch_linear_p3_resid_norm: (a) the fp32 rows of vh_launch_linear_p3(residual), bit for bit; (b) the operand planes
    vh_launch_split3_rows makes of those rows, byte for byte in all three parts (the plane stride with them); (c) every row's
    partial sums and squares against float64; (d) nothing outside rows [0, M) of any output; (e) large case: its first and
    its last 300 rows as launches of their own give the same bits (norm_fold.h: no partial depends on the tile shape or on
    the row's position).  Large: the smallest M that leaves the 128x128 tile at K = N = 2048 (K >= 2048: small_only off;
    2.5 rounds of 256x256 tiles) -- 20300 rows on 256 CUs: 256x256 tiles, a tail launch, a ragged last tile."""
    large = M == "large"
    if large:
        M = _rows_for_class(3, True, False, N, (tiles.T256x256, tiles.T256x256_TAIL), 76)
        if M is None:
            pytest.skip(f"no M <= {ROW_LIMIT} leaves the 128x128 tile at N = {N} on {_cus()} CUs")
    cls, rb = _tile_class(pkg, tiles.PLANES, 3, True, K < 2048, M, N)
    assert (cls != tiles.T128x128) if large else (cls == tiles.T128x128)
    a = oracle.synth_fill(M * K, 1800 + M % 1000, 1.0, 0.1).reshape(M, K)
    w = oracle.synth_fill(N * K, 1801 + N, 0.04, 0.0).reshape(N, K)
    b = oracle.synth_fill(N, 1802, 0.1, 0.0)
    r = _residual_rows(oracle, M, N, 1803)
    d_a3, d_w3, d_b = _split3(pkg, a), _split3(pkg, w), _dev(pkg, b)
    g_x, g_op, g_st = _produce(pkg, d_a3, d_w3, d_b, r, M, K, N, in_place)
    x, planes, st = g_x.to_numpy((M, N)), _raw_planes(g_op, M, N), g_st.to_numpy((N // 128, M, 2))     # (d): the guard bands
    d_plain = _dev(pkg, r)
    _launch(pkg, "vh_launch_linear_p3", None, d_plain.ptr, 0, d_w3.ptr, d_a3.ptr, d_b.ptr, M, K, N, 0, d_plain.ptr)
    assert np.array_equal(x.view(np.uint32), d_plain.to_numpy((M, N)).view(np.uint32))                  # (a)
    del d_plain
    assert np.array_equal(planes, _raw_planes(_split3(pkg, x), M, N))                                  # (b)
    e_sum, e_sq = _assert_stats(st, x)                                                                 # (c)
    if not large:      # ... and in the fixed order norm_fold.h promises, which the emulation test relies on: the same bits
        assert np.array_equal(st.view(np.uint32), _stats32(x).view(np.uint32))
    print(f"\nfold_f32 producer {M}x{K}x{N} {'in place' if in_place else 'out of place'}: class {tiles.NAMES[cls]}, hand-over row {rb}; "
          f"partial sums at {e_sum:.3f}, squares at {e_sq:.3f} of their bounds")
    if large:                                                                                          # (e)
        for sel in (slice(0, 300), slice(M - 300, M)):
            assert _tile_class(pkg, tiles.PLANES, 3, True, False, 300, N)[0] == tiles.T128x128
            s_x, s_op, s_st = _produce(pkg, _split3(pkg, a[sel]), d_w3, d_b, r[sel], 300, K, N)
            assert np.array_equal(s_x.to_numpy((300, N)).view(np.uint32), x[sel].view(np.uint32))
            assert np.array_equal(_raw_planes(s_op, 300, N), planes[:, :, sel])
            assert np.array_equal(s_st.to_numpy((N // 128, 300, 2)).view(np.uint32), st[:, sel].view(np.uint32))


# ---- 3. the consumer -----------------------------------------------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("M,K,N", CONSUMER_SMALL + [("tail", 640, 3072), ("big", 640, 3072)])
def test_p3_consumer_applies_the_folded_layernorm(pkg, device, oracle, M, K, N):
    """vh_launch_linear_p3_norm on the rows, planes and partial sums a chained vh_launch_linear_p3_resid_norm leaves (edge
    rows of _edge_rows kept exact: their share of the producer's GEMM is zero), into fp32 rows and into three-part planes
    with and without GELU.  Per row (a) against _folded_reference on the same operands (parts added in float64, row terms
    in fp32 from the same partials) within 4 OP_TOL max(1, max |want_row|, rstd |mean| max |colsum|) -- the last term is
    the size of the two terms that cancel in the epilogue's fma; (b) against _ln_rows(x) W^T + b in float64 within
    (OP_TOL + 2^-23 amp^2) max(1, max |ref|).  The unfolded pair on the same rows is measured beside it (K <= 1696).
    "tail": 256x256 tiles handing over to a tail launch (13700 rows on 256 CUs), rows sampled around the hand-over row;
    "big": 256x256 tiles alone with a ragged last tile (15000 rows)."""
    L = pkg.lib()
    kind = M
    if kind in ("tail", "big"):
        M = _rows_for_class(3, False, False, N, (tiles.T256x256_TAIL,) if kind == "tail" else (tiles.T256x256,), 132 if kind == "tail" else 152)
        if M is None:
            pytest.skip(f"no M <= {ROW_LIMIT} reaches the class '{kind}' at N = {N} on {_cus()} CUs")
    cls, rb = _tile_class(pkg, tiles.PLANES, 3, False, False, M, N)
    assert cls == {"tail": tiles.T256x256_TAIL, "big": tiles.T256x256}.get(kind, tiles.T128x128)
    assert (rb > 0) == (kind == "tail")
    r, gamma, beta, w, b = _consumer_inputs(oracle, M, K, N)
    # the producer in front (K_p = 128, no bias): x = r + a W_p^T, the edge rows with a = 0
    a = oracle.synth_fill(M * 128, 1820, 1.0, 0.1).reshape(M, 128)
    a[np.array([i for i in EDGE if i < M], dtype=np.intp)] = 0.0
    d_wp3 = _split3(pkg, oracle.synth_fill(K * 128, 1821, 0.04, 0.0).reshape(K, 128))
    g_x, g_op, g_st = _produce(pkg, _split3(pkg, a), d_wp3, _dev(pkg, np.zeros(K, np.float32)), r, M, 128, K)
    x, stats = g_x.to_numpy((M, K)), g_st.to_numpy((K // 128, M, 2))
    if M >= 8:
        assert np.array_equal(x[list(EDGE)], r[list(EDGE)]) and not x[4].any() and (x[5] == 2.5).all()
    # context creation
    d_w, d_g, d_be, d_b = (_dev(pkg, v) for v in (w, gamma, beta, b))
    d_ws, d_w3, d_cs, d_bf = pkg.DeviceBuffer(N * K), _planes_buf(pkg, N, K), pkg.DeviceBuffer(N), pkg.DeviceBuffer(N)
    _launch(pkg, "vh_launch_fold_gamma", None, d_w.ptr, d_g.ptr, d_ws.ptr, N, K)
    _launch(pkg, "vh_launch_split3_rows", None, d_ws.ptr, d_w3.ptr, N, K)
    _launch(pkg, "vh_launch_colsum_planes3", None, d_w3.ptr, d_cs.ptr, N, K)
    _launch(pkg, "vh_launch_fold_bias", None, d_w.ptr, d_be.ptr, d_b.ptr, d_bf.ptr, N, K)
    cs, bf = d_cs.to_numpy(), d_bf.to_numpy()
    rows = _consumer_rows(pkg, tiles.PLANES, M, N)
    if kind == "tail":
        assert rb in rows and rb - 1 in rows
    xo = _planes_to_parts(g_op, M, K)[:, rows].astype(np.float64).sum(0)      # the operand: parts added in float64
    assert np.array_equal(xo, x[rows].astype(np.float64))
    wo = _planes_to_parts(d_w3, N, K).astype(np.float64).sum(0)
    want_lin = _folded_reference(xo, stats[:, rows], wo, cs, bf, K)
    ref_lin = _ln_rows(x[rows], gamma, beta) @ w.astype(np.float64).T + b
    x64 = x[rows].astype(np.float64)
    mean = x64.mean(1)
    rstd = 1.0 / np.sqrt(np.maximum((x64 * x64).mean(1) - mean * mean, 0.0) + EPS)
    amp = _amp(x[rows])
    report = []
    for out, gelu in ((0, 0), (1, 0), (1, 1)):
        want, ref = (_gelu64(want_lin), _gelu64(ref_lin)) if gelu else (want_lin, ref_lin)
        if out == 0:
            d_o = pkg.DeviceBuffer(M * N)
            _launch(pkg, "vh_launch_linear_p3_norm", None, d_o.ptr, 0, d_w3.ptr, g_op.ptr, g_st.ptr, d_cs.ptr, d_bf.ptr, EPS, M, K, N, 0)
        else:
            d_o3, d_o = _planes_buf(pkg, M, N), pkg.DeviceBuffer(M * N)
            _launch(pkg, "vh_launch_linear_p3_norm", None, d_o3.ptr, 1, d_w3.ptr, g_op.ptr, g_st.ptr, d_cs.ptr, d_bf.ptr, EPS, M, K, N, gelu)
            _launch(pkg, "vh_launch_merge3_rows", None, d_o3.ptr, d_o.ptr, M, N)      # exact
        got = d_o.to_numpy((M, N))[rows]
        assert np.isfinite(got).all()
        tol_a = 4 * OP_TOL * np.maximum(1.0, np.maximum(np.abs(want).max(1), rstd * np.abs(mean) * np.abs(cs).max()))
        tol_b = (OP_TOL + 2.0 ** -23 * amp ** 2) * max(1.0, np.abs(ref).max())
        err_a, err_b = np.abs(got - want).max(1), np.abs(got - ref).max(1)
        wa, wb = int(np.argmax(err_a / tol_a)), int(np.argmax(err_b / tol_b))
        line = (f"fold_f32 consumer {M}x{K}x{N} out {out} gelu {gelu}: class {tiles.NAMES[cls]}, hand-over row {rb}; "
                f"(a) worst row {rows[wa]} amp {amp[wa]:.2f} error {err_a[wa]:.3e} bound {tol_a[wa]:.3e} ratio {err_a[wa] / tol_a[wa]:.4f}; "
                f"(b) worst row {rows[wb]} amp {amp[wb]:.2f} error {err_b[wb]:.3e} bound {tol_b[wb]:.3e} ratio {err_b[wb] / tol_b[wb]:.4f}")
        factor = None
        if out == 0 and K <= L.vh_layer_norm_planes_max_embed(3):
            # the unfolded pair on the same rows: LayerNorm writing three-part planes, the plain projection on the original W
            d_y3, d_wu3, d_u = _planes_buf(pkg, M, K), _split3(pkg, w), pkg.DeviceBuffer(M * N)
            _launch(pkg, "vh_launch_layer_norm_p3", None, g_x.ptr, d_g.ptr, d_be.ptr, d_y3.ptr, M, K, K, EPS)
            _launch(pkg, "vh_launch_linear_p3", None, d_u.ptr, 0, d_wu3.ptr, d_y3.ptr, d_b.ptr, M, K, N, 0, None)
            err_u = np.abs(d_u.to_numpy((M, N))[rows] - ref).max(1)
            assert (err_u <= tol_b).all()
            calm = amp <= 1.5
            assert calm.any()
            factor = err_b[calm].max() / err_u[calm].max()
            line += (f"; rows with amp <= 1.5 ({int(calm.sum())}): folded {err_b[calm].max():.3e}, unfolded pair {err_u[calm].max():.3e}, "
                     f"factor {factor:.3f}; all rows: unfolded pair {err_u.max():.3e}")
        print("\n" + line)
        report.append((err_a <= tol_a).all() and (err_b <= tol_b).all() and (factor is None or factor <= FOLD_VS_UNFOLDED_MAX))
    assert all(report), "see the lines printed above"


# ---- 4. patch embedding --------------------------------------------------------------------------------------------------------

# (channels, height, width, patch, E, images, 8-bit layout)
PATCH_GEOMETRIES = {
    "32px p16 C3 E128 n3": (3, 32, 32, 16, 128, 3, "hwc"),
    "28px p14 C3 E640 n2": (3, 28, 28, 14, 640, 2, "chw"),       # K = 588 zero-padded to 640
    "48x32 p16 C1 E256 n17": (1, 48, 32, 16, 256, 17, "hwc"),    # cls_rows_operand_kernel: 16 images per wave -> the 17th, dead lanes, 2 column groups
}


def _patch_reference64(imgs, wc, bc, cls_tok, pos, P):
    """ViT_seq.c:25-57,65-80,90-93,114-117 in float64: [n][T][E]"""
    n, Cc, H, W = imgs.shape
    gh, gw = H // P, W // P
    pat = imgs.astype(np.float64).reshape(n, Cc, gh, P, gw, P).transpose(0, 2, 4, 1, 3, 5).reshape(n, gh * gw, Cc * P * P)
    E = bc.size
    pos = pos.astype(np.float64).reshape(gh * gw + 1, E)
    tok = np.empty((n, gh * gw + 1, E))
    tok[:, 0] = cls_tok.astype(np.float64) + pos[0]
    tok[:, 1:] = pat @ wc.astype(np.float64).reshape(E, -1).T + bc + pos[1:]
    return tok


@gpu
@pytest.mark.parametrize("source", ["f32", "u8"])
@pytest.mark.parametrize("name", list(PATCH_GEOMETRIES))
def test_patch_embedding_leaves_three_part_operand_and_sums_for_every_token_row(pkg, device, oracle, name, source):
    """vh_launch_patch_embed_planes3_norm / _planes_u8 (square) and vh_launch_patch_embed_planes_hw with parts = 3 and an
    operand (the call the forward makes): token rows bit for bit those of the form without an operand (and within the
    operator tolerance of float64), operand planes byte for byte vh_launch_split3_rows of all n x tokens rows, partial
    sums of every row -- class-token rows included in both -- and nothing written outside the outputs."""
    Cc, H, W, P, E, n, layout = PATCH_GEOMETRIES[name]
    L = pkg.lib()
    square = H == W
    np_, K, Kp = (H // P) * (W // P), Cc * P * P, L.vh_patch_planes_k(Cc, P)
    T, R = np_ + 1, n * (np_ + 1)
    assert _tile_class(pkg, tiles.PLANES, 3, True, Kp < 2048, n * np_, E)[0] == tiles.T128x128
    wc = oracle.synth_fill(E * K, 1901, 0.05, 0.0)
    bc, cls_tok, pos = oracle.synth_fill(E, 1902, 0.05, 0.0), oracle.synth_fill(E, 1903, 0.05, 0.0), oracle.synth_fill(T * E, 1904, 0.05, 0.0)
    if source == "u8":
        norm = pkg.pixel_norm(MEAN4[:Cc], STD4[:Cc])
        u = np.random.default_rng(1905).integers(0, 256, size=(n, H, W, Cc), dtype=np.uint8)
        imgs = _normalised(u, norm)
        assert (H * W * Cc) % 16 == 0
        d_img = pkg.DeviceBuffer.from_numpy(_as_layout(u, layout), dtype=np.uint8)
        lay, scale, bias = pkg.binding.PIXEL_LAYOUTS[layout], norm.scale, norm.bias
        hw_src = (None, d_img.ptr, lay, scale, bias)
    else:
        imgs = oracle.synth_fill(n * Cc * H * W, 1900, 1.0, 0.0).reshape(n, Cc, H, W)
        d_img = _dev(pkg, imgs)
        hw_src = (d_img.ptr, None, 0, None, None)
    d_wc, d_bc, d_cls, d_pos = (_dev(pkg, v) for v in (wc, bc, cls_tok, pos))
    d_wp = pkg.DeviceBuffer(E * Kp * 6 // 4)
    _launch(pkg, "vh_launch_conv_weight_planes_parts", None, d_wc.ptr, d_wp.ptr, E, Cc, P, 3)
    need = n * np_ * Kp * 6
    d_ws = pkg.DeviceBuffer(need // 4)
    common = (d_wp.ptr, d_bc.ptr, d_cls.ptr, d_pos.ptr)

    def hw(tok, op, st):
        _launch(pkg, "vh_launch_patch_embed_planes_hw", None, *hw_src, *common, tok, n, Cc, H, W, P, E, d_ws.ptr, need, 3, op, None, st)

    # the form without an operand
    d_plain = pkg.DeviceBuffer(R * E)
    if not square:
        hw(d_plain.ptr, None, None)
    elif source == "u8":
        _launch(pkg, "vh_launch_patch_embed_planes_u8", None, d_img.ptr, lay, scale, bias, *common, d_plain.ptr, n, Cc, H, P, E, d_ws.ptr,
                need, 3, None, None, None)
    else:
        _launch(pkg, "vh_launch_patch_embed_planes3", None, d_img.ptr, *common, d_plain.ptr, n, Cc, H, P, E, d_ws.ptr, need)
    plain = d_plain.to_numpy((R, E))
    want = _patch_reference64(imgs, wc, bc, cls_tok, pos, P).reshape(R, E)
    assert np.abs(plain - want).max() <= OP_TOL * max(1.0, float(np.abs(imgs).max()))
    want_planes = _raw_planes(_split3(pkg, plain), R, E)

    def square_form(tok, op, st):
        if source == "u8":
            _launch(pkg, "vh_launch_patch_embed_planes_u8", None, d_img.ptr, lay, scale, bias, *common, tok, n, Cc, H, P, E, d_ws.ptr, need,
                    3, op, None, st)
        else:
            _launch(pkg, "vh_launch_patch_embed_planes3_norm", None, d_img.ptr, *common, tok, n, Cc, H, P, E, d_ws.ptr, need, op, st)

    for form in ([square_form, hw] if square else [hw]):
        g_tok, g_op, g_st = _Guarded(pkg, R * E, E), _Guarded(pkg, 3 * R * E // 2, 3 * E // 2), _Guarded(pkg, (E // 128) * R * 2, 2 * (E // 128))
        form(g_tok.ptr, g_op.ptr, g_st.ptr)
        x = g_tok.to_numpy((R, E))
        assert np.array_equal(x.view(np.uint32), plain.view(np.uint32))
        assert np.array_equal(_raw_planes(g_op, R, E), want_planes)
        e_sum, e_sq = _assert_stats(g_st.to_numpy((E // 128, R, 2)), x)
        print(f"\nfold_f32 patch embedding {name} {source} ({form.__name__}): class 128x128, {R} rows; partial sums at {e_sum:.3f}, "
              f"squares at {e_sq:.3f} of their bounds")


# ---- 5. whole contexts ----------------------------------------------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("embed,heads", [(2048, 32), (1280, 16)])
def test_a_context_wider_than_the_layernorm_kernel_runs_folded_vs_port(pkg, device, monkeypatch, tmp_path, embed, heads):
    """Depth 1, MLP 2048, 32 px, patch 16, 10 classes, 5 images.  E = 2048 (32 heads of 64) is past
    vh_layer_norm_planes_max_embed(3): refused at creation on the default fp32 path with the LayerNorm width named, created
    with the fold on -- the only fp32 planes path at that width.  E = 1280 (16 heads of 80): both paths run, their difference
    is printed.  Folded against the port with the same loop bounds, live, within 1e-4 with the same arg-max; batch position
    changes no bit; the planes file carries the fold in its header: rebuilt with no environment variable set and run in
    chunks of 2, the same bits."""
    from oracle.oracle import Oracle
    L = pkg.lib()
    orc = Oracle("vit_b_16")
    cfg = pkg.preset("vit_b_16")
    for c in (orc.cfg, cfg):
        c.img_size, c.patch_size, c.in_chans, c.num_classes = 32, 16, 3, 10
        c.embed_dim, c.depth, c.num_heads, c.mlp_hidden = embed, 1, heads, 2048
    weights = orc.synth_weights(23)
    imgs = np.stack([orc.synth_image(i) for i in range(5)])
    want = np.stack([orc.forward(imgs[i], weights)[0] for i in range(5)])
    default = None
    if embed > L.vh_layer_norm_planes_max_embed(3):
        with pytest.raises(pkg.VitHipError, match="LayerNorm width"):
            pkg.ViTHip(cfg, weights, device=0, max_batch=5)
    else:
        m = pkg.ViTHip(cfg, weights, device=0, max_batch=5)
        assert not L.vit_hip_ln_fold(m.ctx)
        default, _ = m.forward(imgs)
        m.close()
    assert (default is None) == (embed == 2048)
    monkeypatch.setenv("VIT_HIP_LN_FOLD", "1")
    m = pkg.ViTHip(cfg, weights, device=0, max_batch=5)
    assert L.vit_hip_ln_fold(m.ctx)
    got, probs = m.forward(imgs)
    again, _ = m.forward(imgs[[3, 0]])
    path = tmp_path / f"folded_{embed}.planes"
    m.export_planes(path)
    m.close()
    monkeypatch.delenv("VIT_HIP_LN_FOLD")
    small = pkg.ViTHip.from_planes(path, device=0, max_batch=2)
    assert L.vit_hip_ln_fold(small.ctx) and small.cfg.embed_dim == embed
    chunked, _ = small.forward(imgs)
    small.close()
    err = float(np.abs(got - want).max())
    print(f"\nfold_f32 context E = {embed}, {heads} heads: folded vs port max |dlogit| {err:.3e}"
          + ("" if default is None else f"; default vs port {np.abs(default - want).max():.3e}; folded minus default {np.abs(got - default).max():.3e}"))
    assert np.isfinite(got).all() and np.abs(probs.sum(axis=1) - 1.0).max() < 1e-5
    assert err <= 1e-4 and np.array_equal(got.argmax(1), want.argmax(1))
    assert np.array_equal(again, got[[3, 0]])
    assert np.array_equal(chunked, got)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------


@gpu
def test_p3_fold_launchers_reject_bad_arguments(pkg, device):
    L = pkg.lib()
    buf = pkg.DeviceBuffer(4096)
    p = buf.ptr

    def refused(rc, needle):
        return rc != 0 and needle in L.vh_last_error()

    assert refused(L.vh_launch_linear_p3_norm(None, p, 1, p, p, None, p, p, EPS, 16, 128, 128, 0), b"null pointer")      # no row statistics
    assert refused(L.vh_launch_linear_p3_norm(None, p, 1, p, p, p, p, p, EPS, 16, 2176, 128, 0), b"at most 16")          # 17 partial sums per row
    assert refused(L.vh_launch_linear_p3_norm(None, p, 1, p, p, p, p, p, EPS, 16, 192, 128, 0), b"colA=192")             # K % 128 (a legal K step)
    assert refused(L.vh_launch_linear_p3_norm(None, p, 0, p, p, p, p, p, EPS, 16, 128, 128, 1), b"epilogue")             # GELU into fp32 rows
    assert refused(L.vh_launch_linear_p3_norm(None, p, 2, p, p, p, p, p, EPS, 16, 128, 128, 0), b"epilogue")             # fp16 planes: one part only
    assert refused(L.vh_launch_linear_p3_resid_norm(None, p, p, p, p, p, 16, 128, 128, None, p), b"resid_norm: null")    # no operand
    assert refused(L.vh_launch_linear_p3_resid_norm(None, p, p, p, p, p, 16, 128, 128, p, None), b"resid_norm: null")    # no statistics
    assert refused(L.vh_launch_colsum_planes3(None, p, p, 16, 48), b"colsum")                                            # K % 32
