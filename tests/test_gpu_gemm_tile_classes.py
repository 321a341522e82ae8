"""GPU tests of the reduced modes' projection GEMMs in every tile class their launchers can pick (csrc/gemm_p3.hip with one
part per value, csrc/gemm_mx.hip; no reference counterpart beyond linear_layer_seq ViT_seq.c:295-309, gelu :283, the
residual loops :348-351 and layer_norm_seq :120-142, which the float64 statements below restate), on WHOLE outputs:

    128x256          the class batch 512 runs: one-part residual / patch-embedding producers, every MX projection
    256x256 + tail   one-part planes projections that write planes or plain fp32 rows, 2.5 rounds of big tiles
    256x256 alone    the same with a whole number of rounds

Every shape is derived from the device's CU count and first PROVED, through the library's own vh_gemm_tile_class, to enter
the class the case is named for; were the rule to move, the case fails instead of silently testing another tile.  N = 512:
two column tiles of 256 (both values of tile % ntiles) and, in the operand producers, statistics groups 0 .. 3 -- the second
group of a 256-wide tile and the reset between the groups are code the 128-wide tile never runs.  The last row tile is ragged.

Each case asserts, over every row:
 a. bit-identity with the 128x128 class: the same launcher on consecutive row chunks of the same problem (inputs restaged
    for the chunk's own row count; each chunk proved to run 128x128 tiles) leaves the same bits in every output -- fp32 rows,
    plane bytes, MX value and scale bytes (in tests/mx_ref.py order), row statistics;
 b. a float64 statement on the same rounded operands, at the project's bounds: fp32 rows OP_TOL (MX: relative to
    max(1, max|want|), as tests/test_gpu_mx.py), + 2^-8 / 2^-10 of max|want| for bf16 / fp16 planes, MX outputs within 2^-3
    of their block maximum + 1e-6, folded consumers of either family against _folded_reference at 4 OP_TOL, statistics
    within 1e-5 relative; a producer's operand must be the rounded rows byte for byte.  The reference is evaluated in row
    chunks, each held to the bound of its own max|want| (never wider than the whole output's);
 c. nothing behind the output is written: every output buffer is followed by 16 fp32 rows / 1024 bytes of 0xff that must
    still be there; the patch embedding's class-token rows hold cls + pos[0].  The guard sits behind the END of a buffer
    only: in the plane, MX and statistics layouts [N/32 or N/128][rows][..] a write past the ragged last row tile lands in
    the next plane's first rows, not in the guard (the last plane excepted) -- there a stray write that loses the race, or is
    wrong, shows in (a) and (b), and one that is overwritten by the right value does not show at all;
 d. one GEMM-TILES report line.
"""
import numpy as np
import pytest

import gemm_tiles_ref as tiles
import mx_ref
from test_gpu_fold import EPS, _folded_reference, _residual_rows
from test_gpu_p3 import OP_TOL, _bf16_rne, _cus, _dev, _launch, _tile_class

pytestmark = pytest.mark.gpu

N = 512
REF_ROWS = 16384                       # rows per evaluation of the float64 reference


# ---- shapes and classes ---------------------------------------------------------------------------------------------------

def _rows_of(cls, cus):
    """the smallest ragged row count that enters `cls` with two column tiles of 256 (256 CUs: 32675, 81749, 98104)"""
    if cls == tiles.T128x256:
        return (cus - 1) * 128 + 35            # cus / 2 row tiles of 256 = cus tiles; the last 128-row tile holds 35 rows
    if cls == tiles.T256x256_TAIL:
        return (5 * cus // 4 - 1) * 256 + 85   # 2.5 cus tiles: two full rounds + cus / 2; hand-over at row cus * 256
    return (3 * cus // 2 - 1) * 256 + 56       # 3 cus tiles: rem == 0


def _chunk_rows(cus):
    return 32 * cus                            # cus / 4 big tiles: far below every threshold (8192 rows at 256 CUs)


# ---- buffers: every output followed by guard bytes ------------------------------------------------------------------------

class _Out:
    """an output buffer of `nbytes` + `pad` guard bytes, all 0xff before the launch"""

    def __init__(self, pkg, nbytes, pad=1024):
        self.nbytes = int(nbytes)
        self.d = pkg.DeviceBuffer(self.nbytes + pad, dtype=np.uint8)
        L = pkg.lib()
        assert L.vh_memset(self.d.ptr, 0xff, self.nbytes + pad, None) == 0 and L.vh_device_sync() == 0, L.vh_last_error().decode()

    @property
    def ptr(self):
        return self.d.ptr

    def take(self, what):
        raw = self.d.to_numpy()
        assert (raw[self.nbytes:] == 0xff).all(), f"{what}: written behind the end of the output"
        return raw[:self.nbytes]


def _f32_out(pkg, rows):
    return _Out(pkg, rows * N * 4, 16 * N * 4)


def _planes_bits(raw, rows):
    """one-part 16-bit planes [N/32][rows][32] -> their bits in matrix order, uint16 [rows][N]"""
    return np.ascontiguousarray(raw.view(np.uint16).reshape(N // 32, rows, 32).transpose(1, 0, 2)).reshape(rows, N)


def _bf16_bits(x):
    return (_bf16_rne(x).view(np.uint32) >> 16).astype(np.uint16)


def _bf16_val(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def _read(outs, rows):
    """guard-checked outputs in canonical form, every one with rows on axis 0: fp32 rows [rows][N]; plane bits [rows][N]; MX
    values [rows][N/128][128] and scales [rows][N/128][4] (mx_ref order); statistics [rows][N/128][2]"""
    got = {}
    for name, o in outs.items():
        raw = o.take(name)
        if name == "rows":
            got[name] = raw.view(np.float32).reshape(rows, N)
        elif name in ("planes", "planes_h", "oper"):
            got[name] = _planes_bits(raw, rows)
        elif name in ("mx", "oper_mx"):
            got[name] = np.ascontiguousarray(raw.reshape(N // 128, rows, 128).transpose(1, 0, 2))
        elif name in ("mx_scales", "oper_mx_scales"):
            got[name] = np.ascontiguousarray(mx_ref.from_act_layout(raw, rows, N).transpose(2, 0, 1))
        else:
            assert name == "stats"
            got[name] = np.ascontiguousarray(raw.view(np.float32).reshape(N // 128, rows, 2).transpose(1, 0, 2))
    return got


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _mx_values(got, name):
    """dequantised MX output [rows][N] from the canonical values / scales"""
    return mx_ref.dequantize(np.ascontiguousarray(got[name].transpose(1, 0, 2)), np.ascontiguousarray(got[name + "_scales"].transpose(1, 2, 0)))


# ---- float64 statements ---------------------------------------------------------------------------------------------------

def _gelu64(v):
    """erf-GELU in float64 over a whole output (torch's vectorised erf: tests/test_gpu_fold.py's statement calls math.erf per
    element, minutes for the 50 M values of a case here)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64))
    return (0.5 * t * (1.0 + torch.erf(t / np.sqrt(2.0)))).numpy()


def _stream_rows(oracle, M, E, seed):
    """_residual_rows (per-row offsets and scales, the |mean| / std ~ 5 row) without the single dominant channel:
    tests/test_gpu_fold.py documents what that channel does to the scaled MFMA; this file is about tiles"""
    x = _residual_rows(oracle, M, E, seed)
    x[3, 7] = 0.25
    return x


def _partial_sums(x):
    """fp32 partial (sum, sum of squares) per 128 columns, [K/128][M][2]: what a producer leaves for the folded LayerNorm"""
    xg = x.reshape(x.shape[0], x.shape[1] // 128, 128)
    return np.ascontiguousarray(np.stack([xg.sum(2, dtype=np.float32), (xg * xg).sum(2, dtype=np.float32)], axis=2).transpose(1, 0, 2))


class _Worst:
    """largest error / bound ratio seen over the reference chunks"""

    def __init__(self):
        self.err, self.bound, self.ratio = 0.0, 0.0, -1.0

    def add(self, err, bound, what):
        err, bound = np.asarray(err, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(err))
        assert np.isfinite(err).all(), what
        i = np.unravel_index(int(np.argmax(err / bound)), err.shape) if err.ndim else ()
        if err[i] / bound[i] > self.ratio:
            self.err, self.bound, self.ratio = float(err[i]), float(bound[i]), float(err[i] / bound[i])

    def __str__(self):
        return f"err={self.err:.3e} bound={self.bound:.3e}"


def _check_values(worst, got, want, out, base, what):
    """one reference chunk: `got` fp32 values against float64 `want`.  out == "mx": the dequantised MX output, per scale
    block; everything else -- the fp32 rows of the operand producers included -- at `base`, the fp32-rows bound, plus one
    rounding of the output format for 16-bit planes"""
    if out == "mx":
        r = want.shape[0]
        bmax = np.abs(want).reshape(r, N // 32, 32).max(axis=2, keepdims=True)
        worst.add(np.abs(got - want).reshape(r, N // 32, 32), np.broadcast_to(2.0 ** -3 * bmax + 1e-6, (r, N // 32, 32)), what)
    else:
        rnd = {"planes": 2.0 ** -8, "planes_h": 2.0 ** -10}.get(out, 0.0) * np.abs(want).max()
        worst.add(np.abs(got - want).max(), base + rnd, what)


def _check_stats(worst, stats, x, what):
    """statistics [rows][N/128][2] against float64 sums of the fp32 rows the same launch wrote"""
    x64 = x.astype(np.float64).reshape(x.shape[0], N // 128, 128)
    worst.add(np.abs(stats[:, :, 0] - x64.sum(2)).max(), 1e-5 * max(1.0, np.abs(x64).sum(2).max()), what)
    worst.add(np.abs(stats[:, :, 1] - (x64 * x64).sum(2)).max(), 1e-5 * (x64 * x64).sum(2).max(), what)


def _check_operand(got, x):
    """a producer's operand: the fp32 rows it wrote, rounded to the next projection's format, byte for byte"""
    if "oper" in got:
        assert np.array_equal(got["oper"], _bf16_bits(x)), "operand planes are not bf16(rows)"
    else:
        qv, qs = mx_ref.quantize(x)
        assert np.array_equal(got["oper_mx"], qv.transpose(1, 0, 2)), "operand values are not the numpy quantiser's"
        assert np.array_equal(got["oper_mx_scales"], qs.transpose(2, 0, 1)), "operand scales are not the numpy quantiser's"


# ---- one problem per (family, class, K): inputs, staged weights and the float64 products, shared by its cases --------------

class _Problem:
    def __init__(self, pkg, oracle, family, M, K, seed):
        self.pkg, self.family, self.M, self.K = pkg, family, M, K
        self.x = _stream_rows(oracle, M, K, seed) if family == tiles.MX else _residual_rows(oracle, M, K, seed)
        self._r = lambda: _stream_rows(oracle, M, N, seed + 10)
        self.w = oracle.synth_fill(N * K, seed + 20, 0.04, 0.0).reshape(N, K)
        self.b = oracle.synth_fill(N, seed + 21, 0.1, 0.0)
        gamma = (1.0 + oracle.synth_fill(K, seed + 22, 0.3, 0.0)).astype(np.float32)
        beta = oracle.synth_fill(K, seed + 23, 0.2, 0.0)
        self.stats = _partial_sums(self.x)
        self.d_b = _dev(pkg, self.b)
        d_w, d_be = _dev(pkg, self.w), _dev(pkg, beta)
        self.d_cs, self.d_bf = pkg.DeviceBuffer(N), pkg.DeviceBuffer(N)
        _launch(pkg, "vh_launch_fold_bias", None, d_w.ptr, d_be.ptr, self.d_b.ptr, self.d_bf.ptr, N, K)
        if family == tiles.MX:
            self.d_w, self.wq = self._mx_weights(self.w)
            self.d_wg, self.wgq = self._mx_weights((self.w * gamma[None, :]).astype(np.float32))
            _launch(pkg, "vh_launch_colsum_operand", None, self.d_wg[0].ptr, self.d_wg[1].ptr, self.d_cs.ptr, N, K)
            xv, xs = mx_ref.quantize(self.x)          # the library's quantiser is this statement byte for byte (test_gpu_mx.py)
            self.xq = mx_ref.dequantize(xv, xs)
        else:
            d_g, d_ws = _dev(pkg, gamma), pkg.DeviceBuffer(N * K)
            _launch(pkg, "vh_launch_fold_gamma", None, d_w.ptr, d_g.ptr, d_ws.ptr, N, K)
            self.d_w, self.wq = self._planes_weights(d_w)
            self.d_wg, self.wgq = self._planes_weights(d_ws)
            _launch(pkg, "vh_launch_colsum_operand", None, self.d_wg.ptr, None, self.d_cs.ptr, N, K)
            self.xq = _bf16_rne(self.x)
        self.cs, self.bf = self.d_cs.to_numpy(), self.d_bf.to_numpy()
        self._pre = {}

    def _planes_weights(self, d_rows):
        d = self.pkg.DeviceBuffer((N * self.K + 1) // 2)
        _launch(self.pkg, "vh_launch_split_rows", None, d_rows.ptr, d.ptr, N, self.K, 1)
        bits = d.to_numpy().view(np.uint16)[:N * self.K].reshape(self.K // 32, N, 32).transpose(1, 0, 2).reshape(N, self.K)
        return d, _bf16_val(np.ascontiguousarray(bits))

    def _mx_weights(self, w):
        d_v, d_s = self.pkg.DeviceBuffer(N * self.K // 4), self.pkg.DeviceBuffer(N * self.K // 128 + 4)
        _launch(self.pkg, "vh_launch_quantize_mx_rows", None, _dev(self.pkg, w).ptr, d_v.ptr, d_s.ptr, N, self.K)
        v = d_v.to_numpy().view(np.uint8)[:N * self.K].reshape(self.K // 128, N, 128)
        s = d_s.to_numpy().view(np.uint8)[:N * self.K // 32].reshape(self.K // 128, 4, N)
        return (d_v, d_s), mx_ref.dequantize(v, s)

    @property
    def r(self):
        """the residual rows, made when the first residual case asks for them"""
        if callable(self._r):
            self._r = self._r()
        return self._r

    def stage(self, epi, r0, r1):
        """device inputs of rows r0 .. r1 as a problem of their own: operand, and residual rows or partial sums where read"""
        pkg, rows, x = self.pkg, r1 - r0, np.ascontiguousarray(self.x[r0:r1])
        st = {}
        if epi == "RESID":
            st["r"] = _dev(pkg, self.r[r0:r1])
        if epi.startswith("NORM"):
            st["stats"] = _dev(pkg, self.stats[:, r0:r1])
        d_x = _dev(pkg, x)
        if self.family == tiles.MX:
            st["x"] = (pkg.DeviceBuffer(rows * self.K // 4), pkg.DeviceBuffer(mx_ref.act_scale_bytes(rows, self.K) // 4 + 4))
            _launch(pkg, "vh_launch_quantize_mx_act", None, d_x.ptr, st["x"][0].ptr, st["x"][1].ptr, rows, self.K)
        else:
            st["x"] = pkg.DeviceBuffer((rows * self.K + 1) // 2)
            _launch(pkg, "vh_launch_split_rows", None, d_x.ptr, st["x"].ptr, rows, self.K, 1)
        return st

    def pre(self, epi, r0, r1):
        """float64 statement of rows r0 .. r1 before GELU / residual, computed once per kind and chunk"""
        kind = "norm" if epi.startswith("NORM") else "plain"
        if (kind, r0) not in self._pre:
            if kind == "norm":
                v = _folded_reference(self.xq[r0:r1], self.stats[:, r0:r1], self.wgq, self.cs, self.bf, self.K)
            else:
                v = self.xq[r0:r1].astype(np.float64) @ self.wq.astype(np.float64).T + self.b.astype(np.float64)
            self._pre[(kind, r0)] = v
        return self._pre[(kind, r0)]

    def want(self, epi, r0, r1):
        v = self.pre(epi, r0, r1)
        if epi.endswith("GELU"):
            v = _gelu64(v)
        if epi == "RESID":
            v = self.r[r0:r1].astype(np.float64) + v
        return v


@pytest.fixture(scope="module")
def problems(pkg, device, oracle):
    """problem(family, class, K), shared by the cases of one (family, class, K) -- they follow each other in this file; only
    the latest is kept, and it is released with the module"""
    held = {}

    def problem(family, cls, K):
        key = (family, cls, K)
        if key not in held:
            held.clear()
            held[key] = _Problem(pkg, oracle, family, _rows_of(cls, _cus()), K, 1000 + 100 * cls + K // 128 + 50 * family)
        return held[key]
    yield problem
    held.clear()


# ---- the launchers, one call per (family, epilogue, output kind) ----------------------------------------------------------

def _outputs(pkg, out, rows):
    plane, mxs = lambda: _Out(pkg, rows * N * 2), lambda: _Out(pkg, mx_ref.act_scale_bytes(rows, N))
    if out == "f32":
        return {"rows": _f32_out(pkg, rows)}
    if out in ("planes", "planes_h"):
        return {out: plane()}
    if out == "mx":
        return {"mx": _Out(pkg, rows * N), "mx_scales": mxs()}
    o = {"rows": _f32_out(pkg, rows), "stats": _Out(pkg, (N // 128) * rows * 8)}
    if out == "oper":
        o["oper"] = plane()
    else:
        o["oper_mx"], o["oper_mx_scales"] = _Out(pkg, rows * N), mxs()
    return o


def _run(p, epi, out, r0, r1):
    """launch rows r0 .. r1 of problem p as a problem of their own -> canonical outputs"""
    pkg, rows, K = p.pkg, r1 - r0, p.K
    st, o = p.stage(epi, r0, r1), _outputs(p.pkg, out, r1 - r0)
    gelu, norm = int(epi.endswith("GELU")), epi.startswith("NORM")
    main = o.get("rows") or o.get("planes") or o.get("planes_h") or o["mx"]
    if p.family == tiles.PLANES:
        kind = {"f32": 0, "planes": 1, "planes_h": 2}.get(out)
        if out in ("oper", "oper_mx"):
            _launch(pkg, "vh_launch_linear_planes_resid_norm", None, main.ptr, p.d_w.ptr, st["x"].ptr, p.d_b.ptr, st["r"].ptr, rows, K, N,
                    o[out].ptr, o["oper_mx_scales"].ptr if out == "oper_mx" else None, o["stats"].ptr)
        elif norm:
            _launch(pkg, "vh_launch_linear_planes_norm", None, main.ptr, kind, p.d_wg.ptr, st["x"].ptr, st["stats"].ptr, p.d_cs.ptr,
                    p.d_bf.ptr, EPS, rows, K, N, gelu)
        else:
            _launch(pkg, "vh_launch_linear_planes", None, main.ptr, kind, p.d_w.ptr, st["x"].ptr, 1, p.d_b.ptr, rows, K, N, gelu,
                    st["r"].ptr if epi == "RESID" else None)
    else:
        xv, xs = st["x"]
        scales = o["mx_scales"].ptr if out == "mx" else None
        if out == "oper_mx":
            _launch(pkg, "vh_launch_linear_mx_resid_norm", None, main.ptr, p.d_w[0].ptr, p.d_w[1].ptr, xv.ptr, xs.ptr, p.d_b.ptr, st["r"].ptr,
                    rows, K, N, o["oper_mx"].ptr, o["oper_mx_scales"].ptr, o["stats"].ptr)
        elif norm:
            _launch(pkg, "vh_launch_linear_mx_norm", None, main.ptr, scales, {"f32": 0, "mx": 1, "planes_h": 2}[out], p.d_wg[0].ptr,
                    p.d_wg[1].ptr, xv.ptr, xs.ptr, st["stats"].ptr, p.d_cs.ptr, p.d_bf.ptr, EPS, rows, K, N, gelu)
        elif out == "planes_h":
            _launch(pkg, "vh_launch_linear_mx_planes_f16", None, main.ptr, p.d_w[0].ptr, p.d_w[1].ptr, xv.ptr, xs.ptr, p.d_b.ptr, rows, K, N)
        else:
            _launch(pkg, "vh_launch_linear_mx", None, main.ptr, scales, p.d_w[0].ptr, p.d_w[1].ptr, xv.ptr, xs.ptr, p.d_b.ptr, rows, K, N, gelu,
                    st["r"].ptr if epi == "RESID" else None)
    return _read(o, rows)


def _values(got, out):
    """the main output as fp32 values [rows][N]"""
    if out in ("f32", "oper", "oper_mx"):
        return got["rows"]
    if out == "planes":
        return _bf16_val(got["planes"])
    if out == "planes_h":
        return got["planes_h"].view(np.float16).astype(np.float32)
    return _mx_values(got, "mx")


def _case(pkg, problems, family, cls, K, epi, out):
    cus = _cus()
    p = problems(family, cls, K)
    M = p.M
    resid = epi == "RESID"
    small = tiles.linear_small_only(resid, K)      # the flag every residual launcher here hands the rule; the others pass 0
    got_cls, rb = _tile_class(pkg, family, 1, resid, small, M, N)
    assert got_cls == cls, f"{M} rows x {N} on {cus} CUs run {tiles.NAMES[got_cls]} tiles, not {tiles.NAMES[cls]}"
    assert (0 < rb < M) == (cls == tiles.T256x256_TAIL)
    big = _run(p, epi, out, 0, M)
    # a. the same bits as the 128x128 class, chunk by chunk
    step = _chunk_rows(cus)
    for r0 in range(0, M, step):
        r1 = min(M, r0 + step)
        assert _tile_class(pkg, family, 1, resid, small, r1 - r0, N) == (tiles.T128x128, 0)
        part = _run(p, epi, out, r0, r1)
        for name, v in part.items():
            assert _same_bits(v, big[name][r0:r1]), f"{name}: rows {r0} .. {r1} differ from the 128x128 tiles' bits"
    # b. float64 on the same rounded operands, every row
    norm = epi.startswith("NORM")
    worst, vals = _Worst(), _values(big, out)
    for r0 in range(0, M, REF_ROWS):
        r1 = min(M, r0 + REF_ROWS)
        want = p.want(epi, r0, r1)
        base = 4 * OP_TOL if norm else OP_TOL * max(1.0, np.abs(want).max()) if family == tiles.MX else OP_TOL
        _check_values(worst, vals[r0:r1], want, out, base, f"rows {r0} .. {r1}")
    stats = _Worst()
    if "stats" in big:
        _check_operand(big, big["rows"])
        _check_stats(stats, big["stats"], big["rows"], "statistics")
    fam = "mx" if family == tiles.MX else "planes1"
    print(f"\nGEMM-TILES {fam} epi={epi} out={out} class={tiles.NAMES[cls]} M={M} K={K} N={N} cus={cus} hand-over={rb} {worst}"
          + (f" statistics: {stats}" if "stats" in big else ""))
    assert worst.ratio <= 1.0 and stats.ratio <= 1.0, f"{worst} statistics: {stats}"


# 128x256: every one-part residual producer of gemm_p3 (K = 128: one loop iteration; 384: three)
@pytest.mark.parametrize("K,out", [(128, "f32"), (128, "oper"), (128, "oper_mx"), (384, "oper")])
def test_planes_residual_producers_on_128x256_tiles(pkg, problems, K, out):
    _case(pkg, problems, tiles.PLANES, tiles.T128x256, K, "RESID", out)


# 128x256: all eleven instantiations of gemm_mx (K = 256: one loop iteration; 768: three)
@pytest.mark.parametrize("K,epi,out", [
    (256, "NONE", "f32"), (256, "NONE", "mx"), (256, "NONE", "planes_h"), (256, "GELU", "f32"), (256, "GELU", "mx"), (256, "RESID", "f32"),
    (256, "NORM", "f32"), (256, "NORM", "mx"), (256, "NORM", "planes_h"), (256, "NORM_GELU", "mx"),
    (256, "RESID", "oper_mx"), (768, "RESID", "oper_mx"),
])
def test_mx_projections_on_128x256_tiles(pkg, problems, K, epi, out):
    _case(pkg, problems, tiles.MX, tiles.T128x256, K, epi, out)


# 256x256 + 128x128 tail: every non-residual one-part instantiation of gemm_p3
@pytest.mark.parametrize("epi,out", [
    ("NONE", "f32"), ("NONE", "planes"), ("NONE", "planes_h"), ("GELU", "f32"), ("GELU", "planes"),
    ("NORM", "f32"), ("NORM", "planes"), ("NORM", "planes_h"), ("NORM_GELU", "planes"),
])
def test_planes_projections_on_256x256_tiles_with_a_tail_launch(pkg, problems, epi, out):
    _case(pkg, problems, tiles.PLANES, tiles.T256x256_TAIL, 128, epi, out)


@pytest.mark.parametrize("epi,out", [("NONE", "f32"), ("NORM_GELU", "planes")])
def test_planes_projections_on_256x256_tiles_alone(pkg, problems, epi, out):
    _case(pkg, problems, tiles.PLANES, tiles.T256x256, 128, epi, out)


# ---- the patch embedding in the 128x256 class ------------------------------------------------------------------------------

E, PATCH, IMG, CHANS = N, 4, 32, 3
NP = (IMG // PATCH) ** 2
T = NP + 1


def _patch_rows(images):
    """[n][C][H][W] -> patch rows [n * NP][C * P * P], k = (c, py, px) as the conv weights' (ViT_seq.c:25-57)"""
    n, g = images.shape[0], IMG // PATCH
    return np.ascontiguousarray(images.reshape(n, CHANS, g, PATCH, g, PATCH).transpose(0, 2, 4, 1, 3, 5)).reshape(n * NP, CHANS * PATCH * PATCH)


def _run_patch(pkg, w, images, out):
    n = images.shape[0]
    R, Kp = n * T, w["Kp"]
    need = n * NP * Kp * 2
    d_img, d_ws = _dev(pkg, images), pkg.DeviceBuffer(need // 4)
    o = _outputs(pkg, out, R)
    head = (None, d_img.ptr, w["planes"].ptr, w["b"].ptr, w["cls"].ptr, w["pos"].ptr, o["rows"].ptr, n, CHANS, IMG, PATCH, E, d_ws.ptr, need)
    if out == "f32":
        _launch(pkg, "vh_launch_patch_embed_planes", *head)
    else:
        _launch(pkg, "vh_launch_patch_embed_planes_norm", *head, o[out].ptr, o["oper_mx_scales"].ptr if out == "oper_mx" else None, o["stats"].ptr)
    return _read(o, R)


@pytest.mark.parametrize("out", ["f32", "oper", "oper_mx"])
def test_patch_embedding_on_128x256_tiles(pkg, device, oracle, out):
    """embed 512, patch 4, image 32, 3 channels (K = 48 padded to 128); 4 (cus / 2) - 3 images (509 at 256 CUs: M = 32576 =
    254 * 128 + 64 patch rows).  The twin launches take up to 100 images each."""
    cus, L = _cus(), pkg.lib()
    n = 4 * (cus // 2) - 3
    M, K = n * NP, CHANS * PATCH * PATCH
    Kp = L.vh_patch_planes_k(CHANS, PATCH)
    assert Kp == 128
    cls, rb = _tile_class(pkg, tiles.PLANES, 1, True, Kp < 2048, M, N)
    assert (cls, rb) == (tiles.T128x256, 0), f"{M} patch rows x {N} on {cus} CUs run {tiles.NAMES[cls]} tiles"
    images = oracle.synth_fill(n * CHANS * IMG * IMG, 1300, 1.0, 0.0).reshape(n, CHANS, IMG, IMG)
    conv_w = oracle.synth_fill(E * K, 1301, 0.05, 0.0).reshape(E, K)
    conv_b, cls_tok, pos = oracle.synth_fill(E, 1302, 0.05, 0.0), oracle.synth_fill(E, 1303, 0.05, 0.0), oracle.synth_fill(T * E, 1304, 0.05, 0.0).reshape(T, E)
    w = {"Kp": Kp, "planes": pkg.DeviceBuffer(E * Kp // 2), "b": _dev(pkg, conv_b), "cls": _dev(pkg, cls_tok), "pos": _dev(pkg, pos)}
    _launch(pkg, "vh_launch_conv_weight_planes", None, _dev(pkg, conv_w).ptr, w["planes"].ptr, E, CHANS, PATCH)
    big = _run_patch(pkg, w, images, out)
    # a. the same bits from launches of at most 100 images, which run 128x128 tiles
    for i0 in range(0, n, 100):
        i1 = min(n, i0 + 100)
        assert _tile_class(pkg, tiles.PLANES, 1, True, Kp < 2048, (i1 - i0) * NP, N) == (tiles.T128x128, 0)
        part = _run_patch(pkg, w, images[i0:i1], out)
        for name, v in part.items():
            assert _same_bits(v, big[name][i0 * T:i1 * T]), f"{name}: images {i0} .. {i1} differ from the 128x128 tiles' bits"
    # b. float64 on the bf16-rounded pixels and weights; c. the class-token rows belong to the other kernel
    tok = big["rows"].reshape(n, T, E)
    assert np.array_equal(tok[:, 0], np.broadcast_to(cls_tok + pos[0], (n, E))), "class-token rows are not cls + pos[0]"
    wq, worst = _bf16_rne(conv_w).astype(np.float64), _Worst()
    for i0 in range(0, n, 128):
        i1 = min(n, i0 + 128)
        want = (_bf16_rne(_patch_rows(images[i0:i1])).astype(np.float64) @ wq.T + conv_b.astype(np.float64)).reshape(i1 - i0, NP, E) + pos[1:].astype(np.float64)
        worst.add(np.abs(tok[i0:i1, 1:] - want).max(), OP_TOL, f"images {i0} .. {i1}")
    stats = _Worst()
    if out != "f32":
        _check_operand(big, big["rows"])
        _check_stats(stats, big["stats"], big["rows"], "statistics")
    print(f"\nGEMM-TILES planes1 epi=PATCH out={out} class={tiles.NAMES[cls]} M={M} K={Kp} N={N} cus={cus} hand-over=0 {worst}"
          + (f" statistics: {stats}" if out != "f32" else ""))
    assert worst.ratio <= 1.0 and stats.ratio <= 1.0, f"{worst} statistics: {stats}"
