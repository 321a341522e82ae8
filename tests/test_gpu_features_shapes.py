"""The feature readout launcher (vh_launch_feature_readout, csrc/features.hip) over its whole documented domain, on synthetic
rows: every (NV, FULL) instantiation of the rows kernel and every NV of the class and pool kernels with their tail-lane and
NCHW slice edges, patch counts at, before and behind the 32-row workgroup edge, both bf16 NCHW store paths (two rows per dword
when P is even, one bf16 per store when P is odd), 1 / 4 / 5 images against the 4-image workgroups, taps, compacted class
rows, isolation of non-finite rows and the refusals.

References.  The file header's two contracts are held as bit relations: final_norm = 1 is vh_launch_layer_norm on the same
rows (and, so that this module stands alone, tokens are held to a float64 two-pass LayerNorm with the bound of
tests/test_gpu_layernorm_shapes.py); pooled is a float32 numpy restatement of the documented summation order
(features_ref.pooled_stated_order) applied to the GPU's own fp32 token rows.  NCHW is the transposition and bf16 the rounding
(bit arithmetic, features_ref.bf16_bits) of the fp32 NLC output of the same arguments.  L2 against float64 with a bound
derived from the kernel's sum (L2_BOUND_ULPS).

Every output buffer has room behind the launch's true size -- one more image's worth, and for tokens no less than one whole
256-column NCHW slice (256 P elements: the most a slip of the column guard could write) -- and is prefilled with 0xff bytes, a
NaN in fp32 and in bf16; so is the scratch slab.  Whatever the launch was not asked to write must still hold them.
"""
import ctypes as C

import numpy as np
import pytest

import features_ref as fr
from test_gpu_layernorm_shapes import _ln32_restated, _ln64_two_pass

gpu = pytest.mark.gpu

EPS = 1e-6
NAMES = ("cls", "pooled", "tokens")
U = 2.0 ** -24                      # unit roundoff of float32

# ---- the case lists ------------------------------------------------------------------------------------------------------------
# NV = 3: 4 .. 768 (FULL);  NV = 4: 772 (one valid lane in chunk 3) .. 1024 (FULL);  NV = 5: 1028 .. 1280 (FULL);
# NV = 8: 1284 .. 2048 (FULL).  252 / 256 / 260: the last NCHW slice holds 252, 256 and 4 columns.
WIDTHS = [4, 36, 252, 256, 260, 764, 768, 772, 1020, 1024, 1028, 1152, 1280, 1284, 1408, 1536, 2044, 2048]
PATCH_COUNTS = [1, 31, 32, 33, 49, 64, 66]
PATCH_WIDTHS = [260, 768, 1408, 2048]
CLASS_WIDTHS = [260, 772, 1152, 1408]       # one non-FULL width per NV class

WIDTH_CASES = [(5, P + 1, E) for E in WIDTHS for P in (33, 66)]
PATCH_CASES = [(5, P + 1, E) for E in PATCH_WIDTHS for P in PATCH_COUNTS if P not in (33, 66)]
BATCH_CASES = [(n, 34, E) for E in CLASS_WIDTHS for n in (1, 4)]
ALL_CASES = WIDTH_CASES + PATCH_CASES + BATCH_CASES


def l2_bound_ulps(E):
    """|got - want| <= l2_bound_ulps(E) 2^-24 |want| + 2^-126 per element of an L2-normalised vector.  The kernel squares (one
    rounding each), a lane adds at most E / 64 squares in sequence, six butterfly steps add the lanes: with E / 16 + 7 roundings
    allowed on the sum of squares, half of that reaches its square root, then sqrtf and the division round once each."""
    return (E / 16 + 7) / 2 + 2


def test_case_list_reaches_every_instantiation_and_branch():
    """CPU: the dispatch arithmetic of vh_launch_feature_readout restated (features_ref.readout_dispatch) over the case
    lists; trimming a list below what the kernels' branches need fails here."""
    assert [fr.readout_dispatch(1, 2, E)["NV"] for E in (4, 768, 772, 1024, 1028, 1280, 1284, 1792, 2048)] == [3, 3, 4, 4, 5, 5, 8, 8, 8]
    assert all(E % 4 == 0 and 4 <= E <= 2048 and 2 <= T <= 67 and 1 <= n <= 5 for n, T, E in ALL_CASES)
    assert len(set(ALL_CASES)) == len(ALL_CASES)
    d = [dict(fr.readout_dispatch(n, T, E), n=n, T=T, E=E) for n, T, E in ALL_CASES]
    every = {(nv, full) for nv in (3, 4, 5, 8) for full in (False, True)}
    assert {(c["NV"], c["FULL"]) for c in d} == every, "rows kernel: an (NV, FULL) instantiation is not launched"
    assert {c["NV"] for c in d} == {3, 4, 5, 8}, "class / pool kernel: an NV instantiation is not launched"
    # each instantiation with both bf16 NCHW store paths, and each path with a ragged last chunk
    assert {(c["NV"], c["FULL"], c["packed"]) for c in d if c["ragged"]} == {e + (p,) for e in every for p in (False, True)}
    assert {c["chunks"] for c in d} >= {1, 2, 3}
    assert {(c["chunks"], c["ragged"]) for c in d} >= {(1, True), (1, False), (2, True), (2, False), (3, True)}
    # the 4-image workgroups of the class and pool kernels: one ragged, one exact, two with a one-image tail -- per NV
    assert {(c["NV"], c["n"]) for c in d} >= {(nv, n) for nv in (3, 4, 5, 8) for n in (1, 4, 5)}
    # tail-lane edges: one valid lane in the last chunk held, all but one, and a last NCHW slice of 4 columns
    assert {E // 4 % 64 for _, _, E in ALL_CASES} >= {1, 63, 0} and any(E % 256 == 4 for _, _, E in ALL_CASES)
    assert {c["ragged_slice"] for c in d} == {False, True}
    for E in PATCH_WIDTHS:
        assert {T - 1 for n, T, e in ALL_CASES if e == E and n == 5} == set(PATCH_COUNTS), E
    for E in WIDTHS:
        assert {(5, 34, E), (5, 67, E)} <= set(ALL_CASES), E


def test_pooled_restatement_and_l2_bound_on_the_cpu():
    """CPU: the float32 restatement of the pooled order is a mean (against float64, within the bound of any summation order)
    and exact on small integers; the L2 bound is what its derivation says at the two ends of the domain."""
    rng = np.random.default_rng(5)
    for P in PATCH_COUNTS:
        tok = rng.standard_normal((2, P, 8)).astype(np.float32)
        got = fr.pooled_stated_order(tok)
        assert np.all(np.abs(got - tok.astype(np.float64).mean(axis=1)) <= 1.01 * U * np.abs(tok).astype(np.float64).sum(axis=1))
        ints = rng.integers(-64, 65, size=(2, P, 8)).astype(np.float32)
        assert np.array_equal(fr.pooled_stated_order(ints), (ints.sum(axis=1, dtype=np.float64).astype(np.float32) / np.float32(P)))
    assert l2_bound_ulps(4) == 5.625 and l2_bound_ulps(2048) == 69.5


# ---- launches into prefilled, padded buffers -----------------------------------------------------------------------------------

def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _dev(pkg, a):
    return pkg.DeviceBuffer.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _at(d, byte_offset):
    return C.c_void_p(d.ptr.value + byte_offset)


class _Outputs:
    """The three output buffers and the scratch slab of one launch shape, each with its guard region, prefilled."""

    def __init__(self, pkg, n, T, E, dtype, n_taps=1):
        self.pkg, self.L = pkg, pkg.lib()
        self.n, self.T, self.E, self.P, self.dtype, self.n_taps = n, T, E, T - 1, dtype, n_taps
        esz = 2 if dtype else 4
        P = T - 1
        self.valid = {"cls": n * n_taps * E * esz, "pooled": n * n_taps * E * esz, "tokens": n * n_taps * P * E * esz}
        guard = {"cls": n_taps * E * esz, "pooled": n_taps * E * esz, "tokens": n_taps * P * max(E, fr.READOUT_SLICE) * esz}
        self.scratch_bytes = self.L.vh_feature_readout_scratch(n, T, E)
        chunks = -(-P // fr.READOUT_ROWS)
        assert self.scratch_bytes == n * chunks * E * 4
        self.valid["scratch"], guard["scratch"] = self.scratch_bytes, chunks * E * 4
        self.d = {k: pkg.DeviceBuffer(self.valid[k] + guard[k], dtype=np.uint8) for k in NAMES + ("scratch",)}
        self.prefill()

    def prefill(self):
        for d in self.d.values():
            assert self.L.vh_memset(d.ptr, 0xff, d.count, None) == 0, self.L.vh_last_error().decode()
        assert self.L.vh_device_sync() == 0, self.L.vh_last_error().decode()

    def rc(self, x, g, b, final_norm, l2, layout, want, tap=0, cls_rows=None, cls_stride=0, scratch_bytes=None, shift=None, n_taps=None):
        shift = shift or {}

        def ptr(k):
            return _at(self.d[k], shift.get(k, 0)) if k in want else None
        sb = self.scratch_bytes if scratch_bytes is None else scratch_bytes
        return self.L.vh_launch_feature_readout(None, x, cls_rows, cls_stride, g, b, EPS, final_norm, l2, self.dtype, layout, self.n,
                                                self.T, self.E, tap, self.n_taps if n_taps is None else n_taps, ptr("cls"),
                                                ptr("pooled"), ptr("tokens"), _at(self.d["scratch"], shift.get("scratch", 0))
                                                if "pooled" in want else None, sb if "pooled" in want else 0)

    def untouched(self):
        return all(bool((d.to_numpy() == 0xff).all()) for d in self.d.values())

    def read(self, want, layout, taps=(0,)):
        """-> {name: array [n][n_taps][...]} (the tap axis dropped when n_taps = 1) after asserting that the guard regions, the
        slots of taps not in `taps` and the buffers not in `want` hold the prefill."""
        n, E, P, k = self.n, self.E, self.P, self.n_taps
        out = {}
        for name in NAMES + ("scratch",):
            raw = self.d[name].to_numpy()
            assert (raw[self.valid[name]:] == 0xff).all(), f"{name}: written behind its last element"
            written = name in want or (name == "scratch" and "pooled" in want)
            if not written:
                assert (raw == 0xff).all(), f"{name}: not requested, yet written"
            if name == "scratch" or not written:
                continue
            body = raw[:self.valid[name]].reshape(n, k, -1)
            for t in range(k):
                if t not in taps:
                    assert (body[:, t] == 0xff).all(), f"{name}: the slots of tap {t}, never launched, were written"
            typed = raw[:self.valid[name]].view(np.uint16 if self.dtype else np.float32)
            shape = (E,) if name != "tokens" else (E, P) if layout else (P, E)
            typed = typed.reshape((n, k) + shape)
            out[name] = np.ascontiguousarray(typed[:, 0] if k == 1 else typed)
        return out

    def run(self, x, g, b, final_norm, l2, layout=0, want=NAMES, **kw):
        self.prefill()
        rc = self.rc(x, g, b, final_norm, l2, layout, want, **kw)
        assert rc == 0, f"vh_launch_feature_readout: {self.L.vh_last_error().decode()}"
        assert self.L.vh_device_sync() == 0, self.L.vh_last_error().decode()
        return self.read(want, layout)


def _layer_norm(pkg, d_x, d_g, d_b, rows, E, in_stride):
    L = pkg.lib()
    d_y = pkg.DeviceBuffer(rows * E)
    assert L.vh_launch_layer_norm(None, d_x.ptr, d_g.ptr, d_b.ptr, d_y.ptr, rows, E, in_stride, E, EPS) == 0, L.vh_last_error().decode()
    assert L.vh_device_sync() == 0, L.vh_last_error().decode()
    return d_y.to_numpy((rows, E))


def _inputs(oracle, n, T, E, seed):
    """x [n][T][E] as the LayerNorm suite draws its rows, gamma in 0.5..1.5, beta in -0.5..0.5"""
    x = oracle.synth_fill(n * T * E, seed, 3.0, 0.5).reshape(n, T, E)
    return x, oracle.synth_fill(E, seed + 1, 0.5, 1.0), oracle.synth_fill(E, seed + 2, 0.5, 0.0)


# ---- assertions 1 - 8 on one shape ---------------------------------------------------------------------------------------------

def _check_case(pkg, oracle, n, T, E):
    P = T - 1
    x, g, b = _inputs(oracle, n, T, E, 9000 + 7 * E + T + n)
    x[n - 1, 0] = 0.0                                    # a zero class row: stays zero under l2 (final_norm = 0)
    d_x, d_g, d_b = _dev(pkg, x), _dev(pkg, g), _dev(pkg, b)
    f32, h16 = _Outputs(pkg, n, T, E, 0), _Outputs(pkg, n, T, E, 1)
    disp = fr.readout_dispatch(n, T, E)
    label = f"E={E:4d} P={P:2d} n={n} NV={disp['NV']} FULL={int(disp['FULL'])} chunks={disp['chunks']}"

    y = _layer_norm(pkg, d_x, d_g, d_b, n * T, E, E).reshape(n, T, E)
    y_cls = _layer_norm(pkg, d_x, d_g, d_b, n, E, T * E)
    assert _same(y_cls, y[:, 0]), "vh_launch_layer_norm: the class rows at stride T E differ from the same rows at stride E"
    want64 = _ln64_two_pass(x[:, 1:].reshape(n * P, E), g, b)
    err_cpu32 = float(np.abs(_ln32_restated(x[:, 1:].reshape(n * P, E), g, b) - want64).max())
    ln_bound = 2.0 * err_cpu32 + 1e-6 * float(np.abs(want64).max())
    worst = {}

    for final_norm in (0, 1):
        rows = y if final_norm else x
        a = f32.run(d_x.ptr, d_g.ptr, d_b.ptr, final_norm, 0)
        what = "vh_launch_layer_norm's rows" if final_norm else "the input rows"
        assert _same(a["tokens"], rows[:, 1:]), f"final_norm={final_norm}: tokens (NLC) are not {what}, bit for bit"
        assert _same(a["cls"], y_cls if final_norm else x[:, 0]), f"final_norm={final_norm}: cls is not {what}, bit for bit"
        if final_norm:
            err_gpu = float(np.abs(a["tokens"].reshape(n * P, E) - want64).max())
            worst["ln"] = (err_gpu, err_cpu32, ln_bound)
            assert np.isfinite(a["tokens"]).all() and err_gpu <= ln_bound, (label, err_gpu, err_cpu32, ln_bound)

        # 6. pooled: the documented order on the GPU's own token rows; and a mean in float64 within any order's bound
        assert _same(a["pooled"], fr.pooled_stated_order(a["tokens"])), f"final_norm={final_norm}: pooled is not the stated order's sum"
        tok64 = a["tokens"].astype(np.float64)
        assert np.all(np.abs(a["pooled"] - fr.features(rows.reshape(n * T, E), n, T, False)[1]) <= 1.01 * U * np.abs(tok64).sum(axis=1))

        # 4. NCHW is the transposition (with pooled sharing the LDS of the tile)
        t = f32.run(d_x.ptr, d_g.ptr, d_b.ptr, final_norm, 0, layout=1)
        assert _same(t["tokens"], fr.nlc_to_nchw(a["tokens"])), f"final_norm={final_norm}: fp32 NCHW is not the transposition of NLC"
        assert _same(t["cls"], a["cls"]) and _same(t["pooled"], a["pooled"]), "cls / pooled differ between the token layouts"

        # 5. bf16 is the rounding, in both layouts
        h = h16.run(d_x.ptr, d_g.ptr, d_b.ptr, final_norm, 0)
        for k in NAMES:
            assert _same(h[k], fr.bf16_bits(a[k])), f"final_norm={final_norm}: bf16 {k} (NLC) is not the rounding of the fp32 output"
        ht = h16.run(d_x.ptr, d_g.ptr, d_b.ptr, final_norm, 0, layout=1, want=("cls", "tokens"))
        path = "two rows per dword" if disp["packed"] else "one bf16 per store"
        assert _same(ht["tokens"], fr.bf16_bits(t["tokens"])), f"final_norm={final_norm}: bf16 NCHW ({path}) is not the rounding of fp32 NCHW"
        assert _same(ht["cls"], h["cls"])

        # 8. L2 against float64 of the same launch's l2 = 0 output
        u = f32.run(d_x.ptr, d_g.ptr, d_b.ptr, final_norm, 1, want=("cls", "pooled"))
        for k in ("cls", "pooled"):
            want = fr.l2_unit(a[k])
            err = np.abs(u[k] - want)
            ulps = float((err / np.maximum(np.abs(want), 2.0 ** -126)).max() / U)
            worst["l2"] = max(worst.get("l2", 0.0), ulps)
            assert np.all(err <= l2_bound_ulps(E) * U * np.abs(want) + 2.0 ** -126), (label, k, final_norm, ulps, l2_bound_ulps(E))
        hu = h16.run(d_x.ptr, d_g.ptr, d_b.ptr, final_norm, 1, want=("cls", "pooled"))
        for k in ("cls", "pooled"):
            assert _same(hu[k], fr.bf16_bits(u[k])), f"final_norm={final_norm}: bf16 {k} under l2 is not the rounding of the fp32 output"
        if not final_norm:
            assert not _bits(u["cls"][n - 1]).any() and not hu["cls"][n - 1].any(), "a zero class row did not stay exactly zero under l2"
            assert n == 1 or np.abs(u["cls"][:n - 1]).max() > 0

        # 7. pooled is a function of T alone: every image by itself
        if final_norm and n > 1:
            one = _Outputs(pkg, 1, T, E, 0)
            for i in range(n):
                alone = one.run(_at(d_x, i * T * E * 4), d_g.ptr, d_b.ptr, 1, 0, want=("pooled",))
                assert _same(alone["pooled"][0], a["pooled"][i]), f"pooled of image {i} differs between n = {n} and n = 1"

    print(f"\nREADOUT-WIDTH {label} l2 max err = {worst['l2']:.2f} x 2^-24 |want| (bound {l2_bound_ulps(E):.2f}); "
          f"ln err_gpu={worst['ln'][0]:.3e} err_cpu32={worst['ln'][1]:.3e} bound={worst['ln'][2]:.3e}")


@gpu
@pytest.mark.parametrize("n,T,E", WIDTH_CASES, ids=[f"E{E}-P{T - 1}" for n, T, E in WIDTH_CASES])
def test_every_width_at_an_odd_and_an_even_patch_count(pkg, device, oracle, n, T, E):
    """5 images, P = 33 (two chunks, a one-row tail, bf16 NCHW one value per store) and P = 66 (three chunks, a two-row tail,
    two rows per dword).  Measured on an MI355X: docs/LABBOOK.md "The feature readout in every width class"."""
    _check_case(pkg, oracle, n, T, E)


@gpu
@pytest.mark.parametrize("n,T,E", PATCH_CASES, ids=[f"E{E}-P{T - 1}" for n, T, E in PATCH_CASES])
def test_every_patch_count_at_four_widths(pkg, device, oracle, n, T, E):
    _check_case(pkg, oracle, n, T, E)


@gpu
@pytest.mark.parametrize("n,T,E", BATCH_CASES, ids=[f"E{E}-n{n}" for n, T, E in BATCH_CASES])
def test_one_and_four_images_per_width_class(pkg, device, oracle, n, T, E):
    _check_case(pkg, oracle, n, T, E)


# ---- 6. pooled on small integers: exact ----------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("E,P", [(260, 33), (260, 66), (2048, 33), (2048, 66)])
def test_pooled_is_exact_on_small_integers(pkg, device, E, P):
    """|x| <= 64 and P <= 66: every partial sum is an integer below 2^24, exact in float32 in any order, so pooled must be
    float32(sum) / float32(P), the correctly rounded mean."""
    n, T = 5, P + 1
    x = np.random.default_rng(E + P).integers(-64, 65, size=(n, T, E)).astype(np.float32)
    assert np.abs(x).max() <= 64 and P <= 66 and 64 * 66 < 2 ** 24 and np.array_equal(x, np.rint(x))
    d_x = _dev(pkg, x)
    got = _Outputs(pkg, n, T, E, 0).run(d_x.ptr, None, None, 0, 0, want=("pooled",))["pooled"]
    total = x[:, 1:].astype(np.float64).sum(axis=1)
    assert np.abs(total).max() < 2 ** 24
    assert _same(got, total.astype(np.float32) / np.float32(P))
    mean64 = fr.features(x.reshape(n * T, E), n, T, False)[1]
    assert np.all(np.abs(got - mean64) <= (U + 2.0 ** -50) * np.abs(mean64))


# ---- 9. taps -------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("E,P", [(260, 33), (1408, 66)])
@pytest.mark.parametrize("n_taps", [2, 4])
def test_taps_interleave(pkg, device, oracle, n_taps, E, P):
    """One launch per tap index, each on rows of its own, into the same buffers: slot (img n_taps + tap) of every output holds
    that tap's single-tap result, and until a tap is launched its slots keep the prefill."""
    n, T = 5, P + 1
    xs = [_inputs(oracle, n, T, E, 9500 + 10 * t + E)[0] for t in range(n_taps)]
    _, g, b = _inputs(oracle, n, T, E, 9500 + E)
    d_xs, d_g, d_b = [_dev(pkg, x) for x in xs], _dev(pkg, g), _dev(pkg, b)
    order = [1, 0] if n_taps == 2 else [3, 0, 1, 2]
    for dtype in (0, 1):
        single, multi = _Outputs(pkg, n, T, E, dtype), _Outputs(pkg, n, T, E, dtype, n_taps)
        for layout in (0, 1):
            want = [single.run(d_xs[t].ptr, d_g.ptr, d_b.ptr, 1, 1, layout=layout) for t in range(n_taps)]
            multi.prefill()
            for step, tap in enumerate(order):
                assert multi.rc(d_xs[tap].ptr, d_g.ptr, d_b.ptr, 1, 1, layout, NAMES, tap=tap) == 0, multi.L.vh_last_error().decode()
                assert multi.L.vh_device_sync() == 0, multi.L.vh_last_error().decode()
                if step in (0, n_taps - 2, n_taps - 1):
                    done = order[:step + 1]
                    got = multi.read(NAMES, layout, taps=done)
                    for t in done:
                        for k in NAMES:
                            assert _same(got[k][:, t], want[t][k]), f"dtype={dtype} layout={layout}: {k} of tap {t} of {n_taps}"


# ---- 10. compacted class rows --------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("E", CLASS_WIDTHS)
def test_compacted_class_rows(pkg, device, oracle, E):
    """cls from cls_rows with x = NULL at strides E, E + 4 (the gap holds NaNs: never read) and T E (the stream itself)."""
    n, T = 5, 34
    x, g, b = _inputs(oracle, n, T, E, 9600 + E)
    d_x, d_g, d_b = _dev(pkg, x), _dev(pkg, g), _dev(pkg, b)
    gapped = np.full((n, E + 4), np.nan, dtype=np.float32)
    gapped[:, :E] = x[:, 0]
    forms = [(_dev(pkg, x[:, 0]), E), (_dev(pkg, gapped), E + 4), (d_x, T * E)]
    for dtype in (0, 1):
        out = _Outputs(pkg, n, T, E, dtype)
        for final_norm in (0, 1):
            for l2 in (0, 1):
                full = out.run(d_x.ptr, d_g.ptr, d_b.ptr, final_norm, l2, want=("cls",))["cls"]
                assert np.isfinite(fr.bf16_to_f32(full) if dtype else full).all()
                for d_rows, stride in forms:
                    got = out.run(None, d_g.ptr, d_b.ptr, final_norm, l2, want=("cls",), cls_rows=d_rows.ptr, cls_stride=stride)["cls"]
                    assert _same(got, full), f"dtype={dtype} final_norm={final_norm} l2={l2}: cls from class rows at stride {stride}"


# ---- 11. isolation -------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_non_finite_value_stays_where_it_belongs(pkg, device, oracle, bad):
    """Width 1408 (NV = 8), P = 33, final_norm = 0: one NaN / +inf in patch row 32 of image 2 (the one-row last chunk) reaches
    that element of tokens, that column of image 2's pooled (l2 = 0) or all of image 2's pooled (l2 = 1: the norm is not
    finite), and nothing else; no cls value moves."""
    n, T, E, img, p, col = 5, 34, 1408, 2, 32, 1405
    x, _, _ = _inputs(oracle, n, T, E, 9700)
    dirty = x.copy()
    dirty[img, 1 + p, col] = bad
    d_clean, d_dirty = _dev(pkg, x), _dev(pkg, dirty)
    out = _Outputs(pkg, n, T, E, 0)
    others = np.setdiff1d(np.arange(n), [img])
    for layout in (0, 1):
        for l2 in (0, 1):
            c = out.run(d_clean.ptr, None, None, 0, l2, layout=layout)
            d = out.run(d_dirty.ptr, None, None, 0, l2, layout=layout)
            assert _same(d["cls"], c["cls"]), "cls moved"
            at = (img, col, p) if layout else (img, p, col)
            moved = _bits(d["tokens"]) != _bits(c["tokens"])
            assert moved[at] and moved.sum() == 1 and _bits(d["tokens"])[at] == _bits(np.float32(bad)), "tokens: not exactly that element"
            assert _same(d["pooled"][others], c["pooled"][others]), "pooled of another image moved"
            moved = _bits(d["pooled"][img]) != _bits(c["pooled"][img])
            if l2:
                # a NaN norm fails `norm > 0` and the vector is zeroed, as features_ref.l2_unit defines; x / inf = 0, inf / inf = NaN
                assert moved.all() and (np.isnan(d["pooled"][img]) | (d["pooled"][img] == 0)).all()
                with np.errstate(invalid="ignore"):
                    assert np.array_equal(np.isnan(d["pooled"][img]), np.isnan(fr.l2_unit(unscaled[img])))
            else:
                unscaled = d["pooled"]
                assert moved[col] and moved.sum() == 1 and not np.isfinite(d["pooled"][img, col])


# ---- 12. refusals --------------------------------------------------------------------------------------------------------------

@gpu
def test_refusals_launch_nothing(pkg, device, oracle):
    n, T, E = 2, 34, 772
    x, g, b = _inputs(oracle, n, T, E + 4, 9800)
    d_x, d_g, d_b = _dev(pkg, x), _dev(pkg, g), _dev(pkg, b)
    L = pkg.lib()
    for dtype in (0, 1):
        out = _Outputs(pkg, n, T, E, dtype)
        X, G, B = d_x.ptr, d_g.ptr, d_b.ptr
        refused = {
            "tap_index = n_taps": lambda: out.rc(X, G, B, 1, 0, 0, NAMES, tap=1),
            "tap_index = n_taps = 4": lambda: out.rc(X, G, B, 1, 0, 0, NAMES, tap=4, n_taps=4),
            "tap_index < 0": lambda: out.rc(X, G, B, 1, 0, 0, NAMES, tap=-1),
            "n_taps = 5": lambda: out.rc(X, G, B, 1, 0, 0, NAMES, tap=0, n_taps=5),
            "n_taps = 0": lambda: out.rc(X, G, B, 1, 0, 0, NAMES, tap=0, n_taps=0),
            "class-row stride < E": lambda: out.rc(None, G, B, 1, 0, 0, ("cls",), cls_rows=X, cls_stride=E - 4),
            "class-row stride % 4": lambda: out.rc(None, G, B, 1, 0, 0, ("cls",), cls_rows=X, cls_stride=E + 2),
            "class-row stride % 4, x given": lambda: out.rc(X, G, B, 1, 0, 0, NAMES, cls_rows=X, cls_stride=E + 6),
            "misaligned cls": lambda: out.rc(X, G, B, 1, 0, 0, NAMES, shift={"cls": 4}),
            "misaligned pooled": lambda: out.rc(X, G, B, 1, 0, 0, NAMES, shift={"pooled": 8}),
            "misaligned tokens": lambda: out.rc(X, G, B, 1, 0, 1, NAMES, shift={"tokens": 2}),
            "misaligned scratch": lambda: out.rc(X, G, B, 1, 0, 0, NAMES, shift={"scratch": 4}),
            "scratch one byte short": lambda: out.rc(X, G, B, 1, 0, 0, NAMES, scratch_bytes=out.scratch_bytes - 1),
            "scratch one byte short, pooled alone": lambda: out.rc(X, G, B, 0, 1, 0, ("pooled",), scratch_bytes=out.scratch_bytes - 1),
        }
        for name, call in refused.items():
            assert call() == 1, f"{name} was accepted"
            assert L.vh_last_error().decode().startswith("vh_launch_feature_readout"), (name, L.vh_last_error())
        assert L.vh_device_sync() == 0
        assert out.untouched(), "a refused launch wrote"
        # the same arguments with the fault taken out are accepted: the exact scratch size, the last tap of four
        assert out.rc(X, G, B, 1, 0, 0, NAMES) == 0 and L.vh_device_sync() == 0, L.vh_last_error().decode()
        assert not out.untouched()
        four = _Outputs(pkg, n, T, E, dtype, 4)
        assert four.rc(X, G, B, 1, 0, 0, NAMES, tap=3) == 0 and L.vh_device_sync() == 0, L.vh_last_error().decode()
        four.read(NAMES, 0, taps=(3,))
