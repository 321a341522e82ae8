"""GPU tests of the GEMMs on fp32 activation rows (csrc/gemm_mfma.hip: gemm_f32_kernel and gemm_mf16_kernel in seven tile
configurations; the reference's linear_layer_seq ViT_seq.c:295-309, gelu :283, the residual loops :348-351 and
Conv2d_seq .. pos_emb_seq :25-118) in every class their launchers can pick, on WHOLE outputs:

    32x64 / 128x128 native guarded   ragged N (the classifier head): the small class below 2 * tiles128 = CUs, the big one above
    128x128 / 256x256 split          vh_launch_linear(_math) under VH_FP32_SPLIT3, both operands split in the K loop
    128x128 / 256x256 native         the same under VH_FP32_NATIVE, and under SPLIT3 once an output-side pointer is misaligned
    128x128 / 256x256 planes         vh_launch_linear_w3 and vh_launch_linear_h2 (weights pre-split)
    256x256 planes + 128x128 tail    the same with the last, partly filled round handed to a second launch
    and the patch embedding on rows in the 256x256 split / native classes, gathered on load and through the padded workspace

Every shape is derived from the device's CU count and first PROVED, through the library's own vh_gemm_rows_tile_class (held
against tests/gemm_tiles_ref.py in tests/test_gemm_rows_host.py), to enter the class the case is named for; every chunk is
proved to enter the small class.  N = 512 where N % 256 == 0 is needed: both values of tile % ntiles.  K = 96: three K steps,
the third refills stage 0 of the two-stage ring; a residual enters a 256x256 class only with K >= 2048.  The last row tile is
ragged (85 live rows).  Input and weight pointers stay 16-byte aligned everywhere.

Each case asserts, over every row of the output:
 a. bit identity with the small class: the same launcher on consecutive 3000-row chunks of the same problem (chunk edges are
    no tile edges: a row's bits may not depend on where in a tile it sits; the patch embedding is chunked by whole images;
    the ragged-N case by 1024 rows); vh_launch_linear against vh_launch_linear_w3, and a misaligned SPLIT3 launch against the
    NATIVE launch it must resolve to.  Nothing is claimed between split and native arithmetic;
 b. float64, per reference chunk: |got - want| <= OP_TOL * max(1, max|want|) -- fp16 pairs (h2) included;
 c. the sharper bound, K = 96, split and native arithmetic (not h2): the kernel's largest error is at most
    gemm_rows_ref.SHARP = 2 times that of the reference's own sequential fp32 loop on the same rows
    (tests/gemm_rows_ref.py says where the 2 comes from; tests/test_gemm_rows_host.py shows it rejects a lost product);
 d. nothing around the output is written: 0xff guards behind every output (and in front of a shifted one) and behind the
    patch embedding's workspace; class-token rows hold cls + pos[0];
 e. one GEMM-TILES report line.  profiles/rows_gemm_class_errors.txt keeps the lines of one run.
"""
import numpy as np
import pytest

import gemm_rows_ref as rr
import gemm_tiles_ref as tiles
from test_gpu_gemm_tile_classes import _Out, _same_bits, _Worst
from test_gpu_p3 import OP_TOL, _cus, _dev, _launch, _planes_buf

pytestmark = pytest.mark.gpu

N = rr.N
CHUNK = 3000
H2_SCALE = 2.0 ** 18                    # 0.04 * 2^18 ~ 10486: inside [8192, 16384), as tests/test_gpu_parity.py takes it
EPI = {"NONE": tiles.EPI_NONE, "GELU": tiles.EPI_GELU, "RESID": tiles.EPI_RESID, "PATCH": tiles.EPI_PATCH}
FAMILY = {tiles.INLOOP: "rows", tiles.W3: "w3", tiles.H2: "h2"}


def _class(pkg, family, epi, math, aligned, rows, K, n):
    """(class, hand-over row) of a launch on this device: the library's rule, which tests/gemm_tiles_ref.py restates"""
    import ctypes
    rb = ctypes.c_int(-1)
    cls = pkg.lib().vh_gemm_rows_tile_class(family, EPI[epi], math, int(aligned), rows, K, n, _cus(), ctypes.byref(rb))
    assert (cls, rb.value) == tiles.rows_tile_class(family, EPI[epi], math, int(aligned), rows, K, n, _cus())
    return cls, rb.value


# ---- buffers ----------------------------------------------------------------------------------------------------------------

class _Shifted(_Out):
    """an output that starts `shift` bytes into its allocation: the bytes in front of it are guard bytes too"""

    def __init__(self, pkg, nbytes, pad, shift=0):
        super().__init__(pkg, nbytes + shift, pad)
        self.shift = shift

    @property
    def ptr(self):
        return self.d.ptr.value + self.shift

    def put(self, pkg, a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        L = pkg.lib()
        assert L.vh_h2d(self.ptr, a.ctypes.data, a.nbytes, None) == 0 and L.vh_device_sync() == 0, L.vh_last_error().decode()

    def take(self, what):
        raw = super().take(what)
        assert (raw[:self.shift] == 0xff).all(), f"{what}: written in front of the output"
        return raw[self.shift:].copy()


def _dev_at(pkg, a, shift):
    """`a` in device memory `shift` bytes into an allocation -> (buffer, address)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    d = pkg.DeviceBuffer(a.size + 4)
    L = pkg.lib()
    assert L.vh_h2d(d.ptr.value + shift, a.ctypes.data, a.nbytes, None) == 0 and L.vh_device_sync() == 0, L.vh_last_error().decode()
    return d, d.ptr.value + shift


# ---- one problem per (M, K, N): inputs, staged weights, the float64 statement and the fp32 loop's error ----------------------

class _Problem:
    def __init__(self, pkg, oracle, M, K, n):
        self.pkg, self.oracle, self.M, self.K, self.n = pkg, oracle, M, K, n
        self.x, self.w, self.b = rr.inputs(oracle, M, K, n)
        self.d_w = _dev(pkg, self.w)
        self._bias, self._r, self._w3, self._h2, self._lin64, self._loop, self._e_ref = {}, None, None, None, {}, None, {}

    def bias(self, shift):
        if shift not in self._bias:
            self._bias[shift] = _dev_at(self.pkg, self.b, shift)
        return self._bias[shift][1]

    @property
    def r(self):
        if self._r is None:
            self._r = rr.residual(self.oracle, self.M, self.n)
        return self._r

    @property
    def w3(self):
        if self._w3 is None:
            self._w3 = _planes_buf(self.pkg, self.n, self.K)
            _launch(self.pkg, "vh_launch_split3_planes", None, self.d_w.ptr, self._w3.ptr, self.n, self.K)
        return self._w3

    @property
    def h2(self):
        if self._h2 is None:
            self._h2 = self.pkg.DeviceBuffer(self.n * self.K)
            _launch(self.pkg, "vh_launch_split2h_planes", None, self.d_w.ptr, self._h2.ptr, self.n, self.K, H2_SCALE)
        return self._h2

    def want(self, epi, r0, r1):
        """float64 statement of rows r0 .. r1; the products are computed once per chunk"""
        if r0 not in self._lin64:
            self._lin64[r0] = rr.linear64(self.x[r0:r1], self.w, self.b)
        v = self._lin64[r0]
        if epi == "GELU":
            v = rr.gelu64(v)
        if epi == "RESID":
            v = self.r[r0:r1].astype(np.float64) + v
        return v

    def e_ref(self, epi):
        """largest error of the reference's own fp32 loop over the whole output"""
        if epi not in self._e_ref:
            if self._loop is None:
                self._loop = self.oracle.linear(self.x, self.w.ravel(), self.b, self.n)
            v = self._loop
            if epi == "GELU":
                v = self.oracle.gelu(v.ravel()).reshape(v.shape)
            if epi == "RESID":
                v = self.r + v
            e = 0.0
            for r0 in range(0, self.M, rr.REF_ROWS):
                r1 = min(self.M, r0 + rr.REF_ROWS)
                e = max(e, float(np.abs(v[r0:r1] - self.want(epi, r0, r1)).max()))
            self._e_ref[epi] = e
        return self._e_ref[epi]


@pytest.fixture(scope="module")
def problems(pkg, device, oracle):
    """problem(M, K, N), shared by the cases of one shape -- they follow each other in this file; only the latest is kept"""
    held = {}

    def problem(M, K, n=N):
        if (M, K, n) not in held:
            held.clear()
            held[(M, K, n)] = _Problem(pkg, oracle, M, K, n)
        return held[(M, K, n)]
    yield problem
    held.clear()


def _run(p, cfg, epi, r0, r1, alias=True):
    """launch rows r0 .. r1 of problem p as a problem of their own -> fp32 [rows][N], guards checked.  cfg = (family,
    fp32_math, shift): output, bias and a separate residual start `shift` bytes behind a 16-byte boundary"""
    pkg, rows, n, K = p.pkg, r1 - r0, p.n, p.K
    family, math, shift = cfg
    d_x = _dev(pkg, p.x[r0:r1])
    out = _Shifted(pkg, rows * n * 4, 16 * n * 4, shift)
    b_ptr, r_ptr, d_r = p.bias(shift), None, None
    if epi == "RESID" and alias:
        out.put(pkg, p.r[r0:r1])
        r_ptr = out.ptr
    elif epi == "RESID":
        d_r, r_ptr = _dev_at(pkg, p.r[r0:r1], shift)
    gelu = int(epi == "GELU")
    if family == tiles.INLOOP:
        _launch(pkg, "vh_launch_linear_math", None, out.ptr, p.d_w.ptr, d_x.ptr, b_ptr, rows, K, n, gelu, r_ptr, math)
    elif family == tiles.W3:
        _launch(pkg, "vh_launch_linear_w3", None, out.ptr, p.w3.ptr, d_x.ptr, b_ptr, rows, K, n, gelu, r_ptr)
    else:
        _launch(pkg, "vh_launch_linear_h2", None, out.ptr, p.h2.ptr, H2_SCALE, d_x.ptr, b_ptr, rows, K, n, gelu, r_ptr)
    return out.take(f"rows {r0} .. {r1}").view(np.float32).reshape(rows, n)


def _native_loop_allowance(p, epi):
    """a native-arithmetic case at K = 2048 that misses (b) on an otherwise bit-consistent kernel is held to
    max(OP_TOL * max(1, max|want|), 2 x the error of the reference's own fp32 loop on those rows) instead: the native
    instruction IS a sequential fp32 sum.  Both numbers go to the report line."""
    return 2.0 * p.e_ref(epi)


def _case(p, cfg, epi, cls, small, name, chunk=CHUNK, alias=True, twins=()):
    """(a) - (e) for one launcher configuration on problem p.  twins: (configuration, what) whose whole-problem launch must
    leave the same bits.  -> the whole output"""
    pkg, cus, M, K, n = p.pkg, _cus(), p.M, p.K, p.n
    family, math, shift = cfg
    got_cls, rb = _class(pkg, family, epi, math, shift == 0, M, K, n)
    assert got_cls == cls, f"{M} rows x {n} (K {K}) on {cus} CUs run {tiles.ROWS_NAMES.get(got_cls)}, not {tiles.ROWS_NAMES[cls]}"
    assert (0 < rb < M) == (cls == tiles.R256_PLANES_TAIL)
    big = _run(p, cfg, epi, 0, M, alias)
    # a. the same bits as the small class, chunk by chunk, and as every twin
    assert chunk % 128 != 0 or chunk == 1024
    for r0 in range(0, M, chunk):
        r1 = min(M, r0 + chunk)
        assert _class(pkg, family, epi, math, shift == 0, r1 - r0, K, n) == (small, 0)
        assert _same_bits(_run(p, cfg, epi, r0, r1, alias), big[r0:r1]), f"rows {r0} .. {r1} differ from the {tiles.ROWS_NAMES[small]} tiles' bits"
    for twin, what in twins:
        assert _same_bits(_run(p, twin, epi, 0, M, alias), big), f"not the bits of {what}"
    # b. float64, every row, per reference chunk; c. against the reference's own loop
    worst, err = _Worst(), 0.0
    for r0 in range(0, M, rr.REF_ROWS):
        r1 = min(M, r0 + rr.REF_ROWS)
        want = p.want(epi, r0, r1)
        e = float(np.abs(big[r0:r1] - want).max())
        err = max(err, e)
        worst.add(e, OP_TOL * max(1.0, float(np.abs(want).max())), f"rows {r0} .. {r1}")
    note = ""
    native = family == tiles.INLOOP and (math == tiles.NATIVE or shift != 0)
    if worst.ratio > 1.0 and native and K >= 2048:
        allow = _native_loop_allowance(p, epi)
        note = f" fp32-loop-allowance={allow:.3e}"
        if worst.err <= allow:
            worst.ratio = worst.err / allow
    sharp = None
    if K == 96 and family != tiles.H2:
        sharp = err / p.e_ref(epi)
        note += f" loop={p.e_ref(epi):.3e} sharp={sharp:.2f}"
    print(f"\nGEMM-TILES {FAMILY[family]} {name} epi={epi} out=f32 class={tiles.ROWS_NAMES[cls]} chunks={tiles.ROWS_NAMES[small]} "
          f"M={M} K={K} N={n} cus={cus} hand-over={rb} {worst} ratio={worst.ratio:.3f}{note}")
    assert worst.ratio <= 1.0, f"{worst}{note}"
    assert sharp is None or sharp <= rr.SHARP, f"largest error {err:.3e} is {sharp:.2f} x the fp32 loop's {p.e_ref(epi):.3e}"
    return big


# ---- shapes -----------------------------------------------------------------------------------------------------------------

M_BIG = 16 * 256 + 85                    # 4181: the 256x256 classes start at 4096 rows; 17 row tiles, the last with 85 rows
M_SMALL = 300
EPI_K = [("NONE", 96), ("GELU", 96), ("RESID", 2048)]     # a residual enters a 256x256 class only with K >= 2048

SPLIT, NATIVE, SHIFTED = (tiles.INLOOP, tiles.SPLIT3, 0), (tiles.INLOOP, tiles.NATIVE, 0), (tiles.INLOOP, tiles.SPLIT3, 4)
W3, H2 = (tiles.W3, tiles.SPLIT3, 0), (tiles.H2, tiles.SPLIT3, 0)


def _tail_rows(cus):
    """the smallest row-tile count the rule calls TAIL at two column tiles, plus two tiles, the last with 85 rows (256 CUs:
    hand-over at 32768, M = 33365 -- the tail launch holds four full 128-row tiles and a ragged one)"""
    mt = next(m for m in range(16, 100000)
              if tiles.rows_tile_class(tiles.W3, tiles.EPI_NONE, 0, 1, 256 * m, 2048, N, cus)[0] == tiles.R256_PLANES_TAIL)
    return (mt + 1) * 256 + 85


# 1, 2: vh_launch_linear_math on 256x256 tiles, split and native
@pytest.mark.parametrize("epi,K", EPI_K)
def test_linear_split3_on_256x256_tiles(problems, epi, K):
    _case(problems(M_BIG, K), SPLIT, epi, tiles.R256_SPLIT, tiles.R128_SPLIT, "linear_math", twins=[(W3, "vh_launch_linear_w3")])


@pytest.mark.parametrize("epi,K", EPI_K)
def test_linear_native_on_256x256_tiles_and_a_misaligned_split3_launch_is_that_launch(problems, epi, K):
    """3: output, bias and residual 4 bytes behind a 16-byte boundary under VH_FP32_SPLIT3 must resolve to the native class
    and leave the native launch's bits"""
    p = problems(M_BIG, K)
    native = _case(p, NATIVE, epi, tiles.R256_NATIVE, tiles.R128_NATIVE, "linear_math-native")
    shifted = _case(p, SHIFTED, epi, tiles.R256_NATIVE, tiles.R128_NATIVE, "linear_math-split3-misaligned", alias=False)
    assert _same_bits(shifted, native), "a misaligned SPLIT3 launch is not the native launch"


@pytest.mark.parametrize("epi", ["NONE", "GELU", "RESID"])
def test_a_misaligned_split3_launch_is_the_native_launch_on_128x128_tiles(problems, epi):
    p = problems(M_SMALL, 96)
    assert _class(p.pkg, tiles.INLOOP, epi, tiles.NATIVE, True, M_SMALL, 96, N) == (tiles.R128_NATIVE, 0)
    native = _run(p, NATIVE, epi, 0, M_SMALL)
    shifted = _case(p, SHIFTED, epi, tiles.R128_NATIVE, tiles.R128_NATIVE, "linear_math-split3-misaligned", chunk=173, alias=False)
    assert _same_bits(shifted, native), "a misaligned SPLIT3 launch is not the native launch"


# 4: the classifier's ragged N on 128x128 guarded tiles
@pytest.mark.parametrize("epi", ["NONE", "GELU", "RESID"])
def test_ragged_n_on_128x128_guarded_tiles(problems, epi):
    """N = 1000: the last column tile holds 104 columns -- three full wave columns and 8 of the fourth.  M = 128 (cus / 16) +
    35 (2083 at 256 CUs): 2 * tiles128 >= cus.  1024-row chunks run the 32x64 guarded tiles."""
    p = problems(128 * (_cus() // 16) + 35, 96, 1000)
    _case(p, SPLIT, epi, tiles.R128_NATIVE_GUARDED, tiles.R32x64_NATIVE_GUARDED, "linear_math-ragged", chunk=1024,
          twins=[(NATIVE, "the same launch under VH_FP32_NATIVE")])


# 5: pre-split weights on 256x256 tiles alone
@pytest.mark.parametrize("cfg", [W3, H2], ids=["w3", "h2"])
@pytest.mark.parametrize("epi,K", EPI_K)
def test_planes_on_256x256_tiles_alone(problems, cfg, epi, K):
    twins = [(SPLIT, "vh_launch_linear")] if cfg == W3 else []
    _case(problems(M_BIG, K), cfg, epi, tiles.R256_PLANES, tiles.R128_PLANES, "linear_" + FAMILY[cfg[0]], twins=twins)


# 6: ... with a tail launch; each residual epilogue aliasing the output and in a buffer of its own
@pytest.mark.parametrize("cfg", [W3, H2], ids=["w3", "h2"])
@pytest.mark.parametrize("epi,K,alias", [("NONE", 96, True), ("GELU", 96, True), ("RESID", 2048, True), ("RESID", 2048, False)])
def test_planes_on_256x256_tiles_with_a_tail_launch(problems, cfg, epi, K, alias):
    twins = [(SPLIT, "vh_launch_linear")] if cfg == W3 else []
    _case(problems(_tail_rows(_cus()), K), cfg, epi, tiles.R256_PLANES_TAIL, tiles.R128_PLANES,
          "linear_" + FAMILY[cfg[0]] + ("" if alias else "-separate-residual"), alias=alias, twins=twins)


# ---- 7, 8: the patch embedding on rows in the 256x256 classes ------------------------------------------------------------------

E = N
GEOMETRIES = {   # name: (in_chans, patch, img_h, img_w, images) -- rows = images * patches >= 4096 and ragged
    "gather-on-load": (6, 4, 32, 48, 43),           # K = 96; 96 patches; 4128 rows
    "padded-workspace": (3, 6, 36, 48, 86),         # K = 108 -> Kp = 128; 48 patches; 4128 rows
    "padded-workspace-square": (3, 6, 48, 48, 65),  # 64 patches; 4160 rows; vh_launch_patch_embed_ws_math must give the same
}


def _patch_rows(images, P):
    """[n][C][H][W] -> patch rows [n * np][C * P * P], k = (c, py, px) as the conv weights' (ViT_seq.c:25-57)"""
    n, C, H, W = images.shape
    return np.ascontiguousarray(images.reshape(n, C, H // P, P, W // P, P).transpose(0, 2, 4, 1, 3, 5)).reshape(n * (H // P) * (W // P), C * P * P)


def _run_patch(pkg, w, images, P, math, square_entry=False):
    """-> tokens [n][T][E], the guards behind the output and the workspace checked"""
    L = pkg.lib()
    n, C, H, W = images.shape
    T = (H // P) * (W // P) + 1
    need = L.vh_patch_embed_workspace_hw(n, C, H, W, P, E)
    d_img = _dev(pkg, images)
    out, ws = _Out(pkg, n * T * E * 4, 16 * E * 4), _Out(pkg, need, 1024) if need else None
    head = (None, d_img.ptr, w["w"].ptr, w["b"].ptr, w["cls"].ptr, w["pos"].ptr, out.ptr, n, C)
    tail = (P, E, ws.ptr if ws else None, need, math)
    if square_entry:
        _launch(pkg, "vh_launch_patch_embed_ws_math", *head, H, *tail)
    else:
        _launch(pkg, "vh_launch_patch_embed_rows_hw", *head, H, W, *tail)
    if ws:
        ws.take("workspace")
    return out.take("tokens").view(np.float32).reshape(n, T, E)


@pytest.mark.parametrize("math", [tiles.SPLIT3, tiles.NATIVE], ids=["split3", "native"])
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_patch_embedding_on_rows_in_the_256x256_classes(pkg, device, oracle, geometry, math):
    C, P, H, W, n = GEOMETRIES[geometry]
    cus, L = _cus(), pkg.lib()
    NP, K = (H // P) * (W // P), C * P * P
    T, M, Kp = NP + 1, n * NP, -(-K // 32) * 32
    direct = geometry == "gather-on-load"
    assert (L.vh_patch_embed_workspace_hw(n, C, H, W, P, E) == 0) == direct and (K == Kp) == direct and M % 256 != 0
    cls, small = (tiles.R256_SPLIT, tiles.R128_SPLIT) if math == tiles.SPLIT3 else (tiles.R256_NATIVE, tiles.R128_NATIVE)
    assert _class(pkg, tiles.INLOOP, "PATCH", math, True, M, Kp, E) == (cls, 0), f"{M} patch rows x {E} on {cus} CUs"
    seed = 4300 + 10 * list(GEOMETRIES).index(geometry)
    images = oracle.synth_fill(n * C * H * W, seed, 1.0, 0.1).reshape(n, C, H, W)
    conv_w = oracle.synth_fill(E * K, seed + 1, 0.04, 0.0).reshape(E, K)
    conv_b, cls_tok = oracle.synth_fill(E, seed + 2, 0.1, 0.0), oracle.synth_fill(E, seed + 3, 0.05, 0.0)
    pos = oracle.synth_fill(T * E, seed + 4, 0.05, 0.0).reshape(T, E)
    w = {"w": _dev(pkg, conv_w), "b": _dev(pkg, conv_b), "cls": _dev(pkg, cls_tok), "pos": _dev(pkg, pos)}
    big = _run_patch(pkg, w, images, P, math)
    # a. the same bits from launches of whole images that stay below 4096 rows
    step = CHUNK // NP
    for i0 in range(0, n, step):
        i1 = min(n, i0 + step)
        assert _class(pkg, tiles.INLOOP, "PATCH", math, True, (i1 - i0) * NP, Kp, E) == (small, 0)
        assert _same_bits(_run_patch(pkg, w, images[i0:i1], P, math), big[i0:i1]), f"images {i0} .. {i1} differ from the 128x128 tiles' bits"
    if H == W:
        assert _same_bits(_run_patch(pkg, w, images, P, math, square_entry=True), big), "vh_launch_patch_embed_ws_math differs"
    # d. the class-token rows belong to the other kernel; b. float64 on every patch row; c. against the reference's loop
    assert np.array_equal(big[:, 0], np.broadcast_to(cls_tok + pos[0], (n, E))), "class-token rows are not cls + pos[0]"
    rows = _patch_rows(images, P)
    want = rr.linear64(rows, conv_w, conv_b).reshape(n, NP, E) + pos[1:].astype(np.float64)
    err, worst = float(np.abs(big[:, 1:] - want).max()), _Worst()
    worst.add(err, OP_TOL * max(1.0, float(np.abs(want).max())), "patch rows")
    note, sharp = "", None
    if K == 96:
        loop = oracle.linear(rows, conv_w.ravel(), conv_b, E).reshape(n, NP, E) + pos[1:]
        e_ref = float(np.abs(loop - want).max())
        sharp = err / e_ref
        note = f" loop={e_ref:.3e} sharp={sharp:.2f}"
    print(f"\nGEMM-TILES rows patch_embed_rows_hw-{geometry} epi=PATCH out=f32 class={tiles.ROWS_NAMES[cls]} chunks={tiles.ROWS_NAMES[small]} "
          f"M={M} K={Kp} N={E} cus={cus} hand-over=0 {worst} ratio={worst.ratio:.3f}{note}")
    assert worst.ratio <= 1.0, str(worst)
    assert sharp is None or sharp <= rr.SHARP, f"largest error {err:.3e} is {sharp:.2f} x the fp32 loop's"
