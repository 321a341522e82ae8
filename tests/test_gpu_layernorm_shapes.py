"""The four LayerNorm launchers of csrc/rowops.hip (vh_launch_layer_norm, _p3, _planes(parts = 1), _mx) over their whole
documented domain: every (NV, FULL) instantiation and its tail-lane edges, ragged row counts against the 4- and 16-row
workgroups, row strides, persistent grids one to three groups deep (both exits of the double-buffered loop), exact and
isolation properties, and every refusal.

References.  The fp32-rows kernel against a float64 TWO-pass LayerNorm (mean, then the mean of squared deviations:
independent of the kernel's single-pass E[x^2] - mean^2), with the bound of test_layer_norm_kernels_on_heavy_rows:
    err_gpu <= 2 err_cpu32 + 1e-6 max|want|        per width, over all rows
where err_cpu32 is the error of a float32 numpy restatement of layer_norm_seq (ViT_seq.c:120-142; single-pass sum and sum of
squares in index order, eps added in double) with the loop bound E.  The three format-writing kernels against the fp32-rows
output y through bit relations: p3 parts = bf16(y), bf16(y - p0), bf16(y - p0 - p1); planes-1 = bf16(y); MX = the numpy
quantiser of y (tests/mx_ref.py) in the activation layout.

Every output buffer has room for 16 more rows in every plane / K step than the launch is told about and is prefilled with
0xff bytes (a NaN in fp32, bf16, e4m3 and e8m0): whatever does not belong to a valid row must still hold them afterwards.
"""
import ctypes as C

import numpy as np
import pytest

import mx_ref
from test_gpu_p3 import _bf16_rne, _dev

gpu = pytest.mark.gpu

EPS = 1e-6
PAD_ROWS = 16
LDS_LIMIT = 160 * 1024
P3_MAX = 1696                       # 32 * 3 * 1696 = 162 816 <= 163 840 < 32 * 3 * 1728

ROWS_ONLY_WIDTHS = [4, 36, 252, 260, 764, 772, 1028, 2044]      # multiples of 4 only; 772: one valid lane in chunk 3
PLANES_WIDTHS = [32, 96, 384, 768, 800, 1024, 1056, 1152, 1280, 1312, 1696]
P3_REFUSED_WIDTHS = [1728, 2048]
MX_WIDTHS = [128, 384, 768, 896, 1024, 1152, 1280, 1408, 1536, 1664, 2048]   # 1..16 K steps: last scale group 1, 2, 3, 4 of 4 full
ALL_WIDTHS = sorted(set(ROWS_ONLY_WIDTHS + PLANES_WIDTHS + P3_REFUSED_WIDTHS + MX_WIDTHS))


# ---- references ------------------------------------------------------------------------------------------------------------

def _ln64_two_pass(x, g, b):
    x = x.astype(np.float64)
    mean = x.mean(axis=1, keepdims=True)
    d = x - mean
    var = (d * d).mean(axis=1, keepdims=True)
    return d / np.sqrt(var + EPS) * g.astype(np.float64) + b.astype(np.float64)


def _ln32_restated(x, g, b):
    """layer_norm_seq in float32: running sums in index order (np.cumsum accumulates sequentially in its dtype)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    E = np.float32(x.shape[1])
    s = np.cumsum(x, axis=1, dtype=np.float32)[:, -1:]
    q = np.cumsum(x * x, axis=1, dtype=np.float32)[:, -1:]
    mean = s / E
    var = q / E - mean * mean
    inv_std = np.float32(1.0) / np.sqrt((var.astype(np.float64) + EPS).astype(np.float32))
    return (x - mean) * inv_std * g + b


def _inputs(oracle, rows, E, seed, stride=None):
    """x [rows][stride] (row i of the problem = the first E values of x[i]), gamma in 0.5..1.5, beta in -0.5..0.5"""
    stride = stride or E
    x = oracle.synth_fill(rows * stride, seed, 3.0, 0.5).reshape(rows, stride)
    return x, oracle.synth_fill(E, seed + 1, 0.5, 1.0), oracle.synth_fill(E, seed + 2, 0.5, 0.0)


def _against_float64(x, g, b, label):
    """-> the check of an fp32-rows output: err_gpu <= 2 err_cpu32 + 1e-6 max|want| over all rows, both errors printed"""
    E = g.size
    want = _ln64_two_pass(x[:, :E], g, b)
    err_cpu32 = float(np.abs(_ln32_restated(x[:, :E], g, b) - want).max())
    bound = 2.0 * err_cpu32 + 1e-6 * float(np.abs(want).max())

    def check(y):
        err_gpu = float(np.abs(y - want).max())
        print(f"\nLN-WIDTH {label} err_gpu={err_gpu:.3e} err_cpu32={err_cpu32:.3e} bound={bound:.3e} max|want|={np.abs(want).max():.3f}")
        assert np.isfinite(y).all() and err_gpu <= bound, (label, err_gpu, err_cpu32, bound)
    return check


# ---- launches into prefilled, padded buffers --------------------------------------------------------------------------------

def _prefilled(pkg, nbytes):
    L = pkg.lib()
    d = pkg.DeviceBuffer((nbytes + 3) // 4)
    assert L.vh_memset(d.ptr, 0xff, d.count * 4, None) == 0 and L.vh_device_sync() == 0, L.vh_last_error().decode()
    return d


def _untouched(d, first_byte=0):
    return bool((d.to_numpy().view(np.uint8)[first_byte:] == 0xff).all())


def _ok(pkg, rc, what):
    L = pkg.lib()
    assert rc == 0, f"{what}: {L.vh_last_error().decode()}"
    assert L.vh_device_sync() == 0, f"{what}: {L.vh_last_error().decode()}"


class _Problem:
    """Device copies of one input and the launches on it.  stride: the input's row stride in floats."""

    def __init__(self, pkg, x, g, b, E):
        self.pkg, self.L = pkg, pkg.lib()
        self.rows, self.stride, self.E = x.shape[0], x.shape[1], E
        self.d_x, self.d_g, self.d_b = _dev(pkg, x), _dev(pkg, g), _dev(pkg, b)

    def rows_out(self, out_stride=None):
        """-> y float32 [rows][E]; the gaps between rows and 16 rows behind the last one keep the prefill"""
        rows, E = self.rows, self.E
        os_ = out_stride or E
        d = _prefilled(self.pkg, (rows + PAD_ROWS) * os_ * 4)
        _ok(self.pkg, self.L.vh_launch_layer_norm(None, self.d_x.ptr, self.d_g.ptr, self.d_b.ptr, d.ptr, rows, E, self.stride, os_, EPS),
            "vh_launch_layer_norm")
        raw = d.to_numpy().view(np.uint32).reshape(rows + PAD_ROWS, os_)
        assert (raw[:rows, E:] == 0xffffffff).all(), "fp32 rows: a gap between two output rows was written"
        assert (raw[rows:] == 0xffffffff).all(), "fp32 rows: written behind the last row"
        return np.ascontiguousarray(raw[:rows, :E]).view(np.float32)

    def planes_out(self, parts):
        """-> uint16 [E/32][parts][rows][32]; the 16 rows of room per plane (behind the tensor) keep the prefill"""
        rows, E = self.rows, self.E
        n = E // 32 * parts
        d = _prefilled(self.pkg, n * (rows + PAD_ROWS) * 64)
        if parts == 3:
            rc = self.L.vh_launch_layer_norm_p3(None, self.d_x.ptr, self.d_g.ptr, self.d_b.ptr, d.ptr, rows, E, self.stride, EPS)
        else:
            rc = self.L.vh_launch_layer_norm_planes(None, self.d_x.ptr, self.d_g.ptr, self.d_b.ptr, d.ptr, parts, rows, E, self.stride, EPS)
        _ok(self.pkg, rc, f"vh_launch_layer_norm_planes(parts = {parts})")
        assert _untouched(d, n * rows * 64), f"planes, {parts} part(s): written behind the last plane's last row"
        return d.to_numpy().view(np.uint16)[:n * rows * 32].reshape(E // 32, parts, rows, 32).copy()

    def mx_out(self):
        """-> (values uint8 [E/128][rows][128], scales uint8 [K-step groups][4][rows][4] as stored)"""
        rows, E = self.rows, self.E
        ks, sg = E // 128, (E // 128 + 3) // 4
        assert self.L.vh_mx_act_scale_bytes(rows, E) == mx_ref.act_scale_bytes(rows, E) == sg * 16 * rows
        d_v, d_s = _prefilled(self.pkg, ks * (rows + PAD_ROWS) * 128), _prefilled(self.pkg, sg * 4 * (rows + PAD_ROWS) * 4)
        _ok(self.pkg, self.L.vh_launch_layer_norm_mx(None, self.d_x.ptr, self.d_g.ptr, self.d_b.ptr, d_v.ptr, d_s.ptr, rows, E, self.stride, EPS),
            "vh_launch_layer_norm_mx")
        assert _untouched(d_v, ks * rows * 128), "MX values: written behind the last K step's last row"
        assert _untouched(d_s, sg * 16 * rows), "MX scales: written behind the last lane group's last row"
        return (d_v.to_numpy().view(np.uint8)[:ks * rows * 128].reshape(ks, rows, 128).copy(),
                d_s.to_numpy().view(np.uint8)[:sg * 16 * rows].reshape(sg, 4, rows, 4).copy())

    def p3_refused(self):
        d = _prefilled(self.pkg, 4096)
        rc = self.L.vh_launch_layer_norm_p3(None, self.d_x.ptr, self.d_g.ptr, self.d_b.ptr, d.ptr, self.rows, self.E, self.stride, EPS)
        msg = self.L.vh_last_error().decode()
        assert rc != 0 and str(P3_MAX) in msg and _untouched(d), (rc, msg)


def _parts_of(planes):
    """uint16 [E/32][parts][rows][32] -> float32 [parts][rows][E]"""
    k, parts, rows, _ = planes.shape
    return (planes.astype(np.uint32) << 16).view(np.float32).transpose(1, 2, 0, 3).reshape(parts, rows, k * 32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_p3_is_the_split_of(pr, p3, y):
    parts = _parts_of(p3)
    p0 = _bf16_rne(y)
    p1 = _bf16_rne(y - p0)
    p2 = _bf16_rne(y - p0 - p1)
    for got, want, name in zip(parts, (p0, p1, p2), ("bf16(y)", "bf16(y - p0)", "bf16(y - p0 - p1)")):
        assert np.array_equal(_bits(got), _bits(want)), f"p3 part is not {name}"
    rows, E = y.shape
    d_p = pr.pkg.DeviceBuffer.from_numpy(np.ascontiguousarray(p3).ravel().view(np.float32))
    d_m = pr.pkg.DeviceBuffer(rows * E)
    _ok(pr.pkg, pr.L.vh_launch_merge3_rows(None, d_p.ptr, d_m.ptr, rows, E), "vh_launch_merge3_rows")
    assert np.array_equal(_bits(d_m.to_numpy((rows, E))), _bits(y + np.float32(0.0))), "merge of the p3 planes is not y + 0.0"


def _assert_planes1_is_bf16_of(p1, y):
    assert np.array_equal(_bits(_parts_of(p1)[0]), _bits(_bf16_rne(y))), "one-part planes are not bf16(y)"


def _assert_mx_is_the_quantiser_of(mx, y):
    values, scales = mx
    rows, E = y.shape
    want_v, want_s = mx_ref.quantize(y)
    got_s = mx_ref.from_act_layout(scales.ravel(), rows, E)       # drops the bytes of K steps beyond E / 128 (unspecified)
    assert np.array_equal(got_s, want_s), "MX scale bytes"
    zero = (want_v & 0x7f) == 0                                   # signed zeros: compare magnitudes (as test_gpu_mx.py does)
    assert np.array_equal(values[~zero], want_v[~zero]) and np.array_equal(values[zero] & 0x7f, want_v[zero] & 0x7f), "MX values"


def _check_all_launchers(pkg, x, g, b, E, y_check=None):
    """Runs every launcher that takes this width on x (row stride = x.shape[1]) and asserts the bit relations to the
    fp32-rows output, which it returns.  p3 must refuse the widths above P3_MAX."""
    pr = _Problem(pkg, x, g, b, E)
    y = pr.rows_out()
    if y_check is not None:
        y_check(y)
    if E % 32 == 0:
        _assert_planes1_is_bf16_of(pr.planes_out(1), y)
        if E <= P3_MAX:
            _assert_p3_is_the_split_of(pr, pr.planes_out(3), y)
        else:
            pr.p3_refused()
    if E % 128 == 0:
        _assert_mx_is_the_quantiser_of(pr.mx_out(), y)
    return y


# ---- a. width sweep -----------------------------------------------------------------------------------------------------------

def test_float32_restatement_is_finite_on_the_sweep_inputs(oracle):
    """CPU: the float32 restatement of layer_norm_seq that sets the fp32-rows bound gives finite values on every width's
    inputs (no row of them has var + eps <= 0 in float32), and the float64 two-pass reference is finite as well."""
    for E in ALL_WIDTHS:
        x, g, b = _inputs(oracle, 37, E, 7000 + E)
        y32 = _ln32_restated(x, g, b)
        assert y32.dtype == np.float32 and y32.shape == x.shape and np.isfinite(y32).all(), E
        assert np.isfinite(_ln64_two_pass(x, g, b)).all(), E


@gpu
@pytest.mark.parametrize("E", ALL_WIDTHS)
def test_width_sweep_all_launchers(pkg, device, oracle, E):
    """37 rows (ragged against 4 and 16) at every (NV, FULL) pair and tail-lane edge.  Measured on an MI355X, GPU error and
    error of the float32 restatement per width: docs/LABBOOK.md "LayerNorm width sweep"."""
    x, g, b = _inputs(oracle, 37, E, 7000 + E)
    _check_all_launchers(pkg, x, g, b, E, _against_float64(x, g, b, f"E={E:5d}"))


# ---- b. ragged rows -----------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("E", [1152, 1024])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 15, 16, 17, 31, 33])
def test_ragged_row_counts_write_valid_rows_only(pkg, device, oracle, rows, E):
    x, g, b = _inputs(oracle, rows, E, 7100 + E + rows)
    _check_all_launchers(pkg, x, g, b, E, _against_float64(x, g, b, f"E={E:5d} rows={rows:2d}"))


# ---- c. strides ---------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("E", [772, 1152])
def test_row_strides(pkg, device, oracle, E):
    """in_row_stride = 3 E + 4: only the first E values of every row are read -- results equal those of the compact call, bit
    for bit, in all launchers that take the width; out_row_stride = E + 12: the gaps keep their prefill (_Problem.rows_out)."""
    rows, stride = 37, 3 * E + 4
    x, g, b = _inputs(oracle, rows, E, 7200 + E, stride)
    compact = np.ascontiguousarray(x[:, :E])
    wide, tight = _Problem(pkg, x, g, b, E), _Problem(pkg, compact, g, b, E)
    y = tight.rows_out()
    assert np.array_equal(_bits(wide.rows_out()), _bits(y))
    assert np.array_equal(_bits(tight.rows_out(out_stride=E + 12)), _bits(y))
    assert np.array_equal(_bits(wide.rows_out(out_stride=E + 12)), _bits(y))
    assert np.abs(y - _ln64_two_pass(compact, g, b)).max() <= 2e-5
    if E % 32 == 0:
        for parts in (1, 3):
            assert np.array_equal(wide.planes_out(parts), tight.planes_out(parts)), parts
        _assert_p3_is_the_split_of(wide, wide.planes_out(3), y)
    if E % 128 == 0:
        (wv, ws), (tv, ts) = wide.mx_out(), tight.mx_out()
        assert np.array_equal(wv, tv) and np.array_equal(ws, ts)
        _assert_mx_is_the_quantiser_of((wv, ws), y)


# ---- d. persistent grid depth ---------------------------------------------------------------------------------------------------

def _cap(kernel, E):
    """The persistent grid's size as the launchers compute it (csrc/rowops.hip): workgroups resident per CU x CUs."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if kernel == "mx":
        return 2 * cus
    lds = 32 * {"planes1": 1, "p3": 3}[kernel] * E
    return (1 if LDS_LIMIT // lds < 2 else 2) * cus


@gpu
@pytest.mark.parametrize("kernel,E", [("planes1", 128), ("planes1", 1024), ("mx", 128), ("mx", 1024), ("p3", 384), ("p3", 768)])
@pytest.mark.parametrize("depth", ["cap+1", "2.5cap"])
def test_persistent_grid_one_to_three_groups_deep(pkg, device, oracle, kernel, E, depth):
    """ngroups = cap + 1 (workgroup 0 takes two groups, the others one: the first exit after one group, and after two) and
    ngroups = 2 cap + cap / 2 with 5 rows in the last group (three and two groups: the second exit, and the first on its
    second round), on a non-FULL and a FULL width per kernel: every row against the fp32-rows launcher's."""
    cap = _cap(kernel, E)
    assert cap >= 64 and cap % 2 == 0
    ngroups = cap + 1 if depth == "cap+1" else 2 * cap + cap // 2
    rows = 16 * ngroups if depth == "cap+1" else 16 * (ngroups - 1) + 5
    assert rows <= 21000
    x, g, b = _inputs(oracle, rows, E, 7300 + E)
    pr = _Problem(pkg, x, g, b, E)
    y = pr.rows_out()
    assert np.isfinite(y).all()
    sample = np.r_[0:40, rows - 40:rows]
    assert np.abs(y[sample] - _ln64_two_pass(x[sample], g, b)).max() <= 2e-5
    if kernel == "planes1":
        _assert_planes1_is_bf16_of(pr.planes_out(1), y)
    elif kernel == "p3":
        _assert_p3_is_the_split_of(pr, pr.planes_out(3), y)
    else:
        _assert_mx_is_the_quantiser_of(pr.mx_out(), y)


# ---- e. exact and isolation properties --------------------------------------------------------------------------------------------

@gpu
def test_exact_rows_and_isolation_of_non_finite_rows(pkg, device, oracle):
    """Width 1152, 40 rows.  An all-zero row and a row of constant 2.0 (sum and sum of squares exact in any order, var = 0)
    give exactly beta.  A NaN in row 18, an Inf in row 21 (one 16-row group) and a NaN in row 35 (the ragged last group):
    every other row of all four outputs keeps the bits of the run without them."""
    rows, E = 40, 1152
    x, g, b = _inputs(oracle, rows, E, 7400)
    x[3] = 0.0
    x[5] = 2.0
    clean = _Problem(pkg, x, g, b, E)
    y = _check_all_launchers(pkg, x, g, b, E)
    assert np.array_equal(y[3], b) and np.array_equal(y[5], b)
    bad = x.copy()
    bad[18, 700], bad[21, 5], bad[35, 1151] = np.nan, np.inf, np.nan
    dirty = _Problem(pkg, bad, g, b, E)
    keep = np.setdiff1d(np.arange(rows), [18, 21, 35])
    yd = dirty.rows_out()
    assert np.array_equal(_bits(yd[keep]), _bits(y[keep])) and not np.isfinite(yd[[18, 21, 35]]).all(axis=1).any()
    for parts in (1, 3):
        assert np.array_equal(dirty.planes_out(parts)[:, :, keep], clean.planes_out(parts)[:, :, keep]), parts
    (dv, ds), (cv, cs) = dirty.mx_out(), clean.mx_out()
    assert np.array_equal(dv[:, keep], cv[:, keep]) and np.array_equal(ds[:, :, keep], cs[:, :, keep])


# ---- f. refusals ----------------------------------------------------------------------------------------------------------------

@gpu
def test_refusals_launch_nothing(pkg, device, oracle):
    L = pkg.lib()
    x, g, b = _inputs(oracle, 8, 2176, 7500)
    d_x, d_g, d_b = _dev(pkg, x), _dev(pkg, g), _dev(pkg, b)
    out, out2 = _prefilled(pkg, 1 << 20), _prefilled(pkg, 1 << 16)

    def rows_(E, si, so):
        return L.vh_launch_layer_norm(None, d_x.ptr, d_g.ptr, d_b.ptr, out.ptr, 8, E, si, so, EPS)

    def planes(parts, E, si):
        return L.vh_launch_layer_norm_planes(None, d_x.ptr, d_g.ptr, d_b.ptr, out.ptr, parts, 8, E, si, EPS)

    def p3(E, si):
        return L.vh_launch_layer_norm_p3(None, d_x.ptr, d_g.ptr, d_b.ptr, out.ptr, 8, E, si, EPS)

    def mx(E, si):
        return L.vh_launch_layer_norm_mx(None, d_x.ptr, d_g.ptr, d_b.ptr, out.ptr, out2.ptr, 8, E, si, EPS)
    refused = {
        "rows E=2052": lambda: rows_(2052, 2052, 2052), "planes E=2052": lambda: planes(1, 2052, 2052), "p3 E=2052": lambda: p3(2052, 2052),
        "mx E=2052": lambda: mx(2052, 2052), "planes E=2080": lambda: planes(1, 2080, 2080), "mx E=2176": lambda: mx(2176, 2176),
        "rows E=30": lambda: rows_(30, 32, 32), "planes E=36": lambda: planes(1, 36, 36), "p3 E=36": lambda: p3(36, 36),
        "mx E=96": lambda: mx(96, 96),
        "rows in stride < E": lambda: rows_(768, 764, 768), "rows out stride < E": lambda: rows_(768, 768, 764),
        "planes stride < E": lambda: planes(1, 768, 736), "p3 stride < E": lambda: p3(768, 736), "mx stride < E": lambda: mx(768, 640),
        "rows in stride % 4": lambda: rows_(768, 770, 768), "rows out stride % 4": lambda: rows_(768, 768, 770),
        "planes stride % 4": lambda: planes(1, 768, 770), "p3 stride % 4": lambda: p3(768, 770), "mx stride % 4": lambda: mx(768, 770),
        "planes parts=2": lambda: planes(2, 768, 768), "planes parts=0": lambda: planes(0, 768, 768),
        "rows rows=0": lambda: L.vh_launch_layer_norm(None, d_x.ptr, d_g.ptr, d_b.ptr, out.ptr, 0, 768, 768, 768, EPS),
    }
    for name, call in refused.items():
        assert call() != 0, f"{name} was accepted"
        assert L.vh_last_error() != b"", name
    # the LDS budget of the three-part image: 32 * 3 * E bytes of 160 KiB
    assert L.vh_layer_norm_planes_max_embed(3) == P3_MAX and L.vh_layer_norm_planes_max_embed(1) == 2048
    assert L.vh_layer_norm_planes_max_embed(2) == 0
    for E in P3_REFUSED_WIDTHS:
        for call in (lambda: p3(E, E), lambda: planes(3, E, E)):
            assert call() != 0
            msg = L.vh_last_error().decode()
            assert str(P3_MAX) in msg and "LDS" in msg, msg
    assert L.vh_device_sync() == 0
    assert _untouched(out) and _untouched(out2)
    assert p3(P3_MAX, P3_MAX) == 0 and L.vh_device_sync() == 0, L.vh_last_error().decode()      # the widest accepted
    assert not _untouched(out)


def test_fp32_context_with_embed_dim_2048_is_refused_at_creation(pkg, monkeypatch):
    """The default fp32 mode runs its LayerNorms on three-part planes, whose LDS image ends at embed_dim 1696: a config
    beyond it (E = 2048, 32 heads of 64) is refused by vit_hip_create with the LayerNorm width named -- before the device
    is touched (this test runs without one), not at the first forward."""
    for var in ("VIT_HIP_P3", "VIT_HIP_GEMM_FP32", "VIT_HIP_LN_FOLD", "VIT_HIP_PRECISION"):
        monkeypatch.delenv(var, raising=False)
    L, bnd = pkg.lib(), pkg.binding
    cfg = bnd.VitConfig(img_size=32, patch_size=16, in_chans=3, num_classes=8, embed_dim=2048, depth=1, num_heads=32, mlp_hidden=128,
                        eps=1e-6)
    n = L.vit_config_num_tensors(C.byref(cfg))
    weights = [np.zeros(L.vit_config_tensor_size(C.byref(cfg), i), dtype=np.float32) for i in range(n)]
    for create in (lambda ctx: L.vit_hip_create(C.byref(ctx), C.byref(cfg), bnd.networks(weights), n, 0, 1),
                   lambda ctx: L.vit_hip_create_ex(C.byref(ctx), C.byref(cfg), bnd.networks(weights), n, 0, 1, 0)):
        ctx = C.c_void_p()
        rc = create(ctx)
        msg = L.vh_last_error().decode()
        assert rc == 2 and not ctx.value, (rc, msg)
        assert "LayerNorm width" in msg and "embed_dim=2048" in msg and str(P3_MAX) in msg, msg
