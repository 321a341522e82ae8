"""The resident attention kernels at every count of key tiles, against float64 (tests/attn_tiles_ref.py).

csrc/attention_p3.hip (Q|K|V as planes: the default fp32 path, the bf16 and fp8 modes) and csrc/attention_f32.hip (fp32
rows: the operator API, VIT_HIP_P3=0, the fp16-pair mode) are instantiated once per count NKT = ceil(T / 32) of 32-key
tiles, 1 to 7; csrc/attention_h16.hip (head dim 80) runs 16-key tiles in one or two rounds of query tiles.  Every case
first asserts the tile count it was written for, writes into buffers pre-filled with 0xff bytes that end in 256 guard
bytes, and compares ALL rows, per element, with the reference at the bound of its family (fp32: 2e-5 max(1, A); fp16
operands: half an fp16 ulp of every probability on top -- derived in attn_tiles_ref.py, and shown by
tests/test_attn_tiles_host.py to reject a kernel that drops, doubles or misplaces the last key).  Forms that promise the
same bits as another (planes against rows, bf16 planes and MX output against the rounded / quantised fp32 rows) are held
to that as well; the MX bytes are compared with the NumPy quantiser (tests/mx_ref.py), not only with the GPU one."""
import numpy as np
import pytest

import attn_ref as ar
import attn_tiles_ref as tr
import mx_ref

pytestmark = pytest.mark.gpu

ARITH = {"native": 0, "fp16": 1, "fp16x2": 2, "split3": 3}          # VH_ATTN_*
FAMILY = {"native": "fp32", "fp16x2": "fp32", "split3": "fp32", "fp16": "fp16"}
GUARD = 256


def _hd64_cases():
    """(k, T, E, H, n, kind): the table at E = 256, then the wide cases"""
    E, H, n = tr.HD64_SHAPE
    cases = [(k, T, E, H, n, kind) for k, T in tr.HD64_TABLE for kind in tr.KINDS if T > 1 or kind == "plain"]
    E, H, n = tr.HD64_WIDE_SHAPE
    return cases + [(k, T, E, H, n, kind) for k, T in tr.HD64_WIDE for kind in tr.KINDS]


def _id(case):
    return "k{}-T{}-E{}-{}".format(case[0], case[1], case[2], case[-1])


HD64 = [pytest.param(c, id=_id(c)) for c in _hd64_cases()]
H16 = [pytest.param((T, kind), id=f"T{T}-{kind}") for T in tr.H16_T for kind in tr.KINDS]

_INPUTS, _WANT = {}, {}


def _qkv(oracle, n, T, E, H, kind, tile=32):
    key = (n, T, E, H, kind)
    if key not in _INPUTS:
        qkv = tr.make_qkv(oracle.synth_fill, n, T, E, H, kind, 7000 + T, tile)
        qkv.setflags(write=False)
        _INPUTS[key] = qkv
    return _INPUTS[key]


def _want(oracle, n, T, E, H, kind, family, tile=32):
    """(O, bound), float64 [n*T][E]: computed once per (shape, input, rounding), shared and left unchanged"""
    key = (n, T, E, H, kind, family)
    if key not in _WANT:
        O, bnd = tr.expectation(_qkv(oracle, n, T, E, H, kind, tile), n, T, H, family)
        O.setflags(write=False)
        bnd.setflags(write=False)
        _WANT[key] = (O, bnd)
    return _WANT[key]


def _launch(pkg, name, *args):
    L = pkg.lib()
    rc = getattr(L, name)(*args)
    assert rc == 0, f"{name}: {L.vh_last_error().decode()}"
    assert L.vh_device_sync() == 0, L.vh_last_error().decode()


class _Out:
    """An output buffer of nbytes, every byte 0xff (a NaN in every format written here), followed by guard bytes"""

    def __init__(self, pkg, nbytes):
        self.nbytes = int(nbytes)
        self.buf = pkg.DeviceBuffer.from_numpy(np.full(self.nbytes + (-self.nbytes) % 16 + GUARD, 0xff, np.uint8), dtype=np.uint8)
        self.ptr = self.buf.ptr

    def bytes(self):
        raw = self.buf.to_numpy()
        assert (raw[self.nbytes:] == 0xff).all(), "bytes past the end of the output were written"
        return raw[:self.nbytes]

    def f32(self, rows, cols):
        return self.bytes().view(np.float32).reshape(rows, cols)


def _dev(pkg, a):
    return pkg.DeviceBuffer.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _hold(label, got, want):
    """every element of got within its bound of the float64 reference; -> the largest err / bound"""
    O, bnd = want
    assert got.shape == O.shape and np.isfinite(got).all(), f"{label}: non-finite or unwritten output"
    excess = np.abs(got.astype(np.float64) - O) / bnd
    worst = np.unravel_index(np.argmax(excess), excess.shape)
    print(f"\nattn-tiles {label}: err/bound {excess[worst]:.3f}")
    assert excess[worst] <= 1.0, f"{label}: row {worst[0]} column {worst[1]}: got {got[worst]}, want {O[worst]}, bound {bnd[worst]}"
    return float(excess[worst])


def _rows(pkg, d_q, arith, n, T, E, H):
    out = _Out(pkg, n * T * E * 4)
    _launch(pkg, "vh_launch_attention_rows", None, d_q.ptr, out.ptr, 0, ARITH[arith], 0, n, T, E, H)
    return out.f32(n * T, E)


def _planes3(pkg, d_q, n, T, E, H):
    """vh_launch_attention_planes on the exact split of the rows, merged back -> fp32 [rows][E]"""
    rows = n * T
    d_q3 = _Out(pkg, rows * 3 * E * 6)
    _launch(pkg, "vh_launch_split3_rows", None, d_q.ptr, d_q3.ptr, rows, 3 * E)
    d_q3.bytes()
    d_p, d_m = _Out(pkg, rows * E * 6), _Out(pkg, rows * E * 4)
    _launch(pkg, "vh_launch_attention_planes", None, d_q3.ptr, d_p.ptr, n, T, E, H)
    d_p.bytes()
    _launch(pkg, "vh_launch_merge3_rows", None, d_p.ptr, d_m.ptr, rows, E)
    return d_m.f32(rows, E)


def _f16_planes_in(pkg, qkv):
    return ar.upload(pkg, ar.encode_f16(qkv))


def _planes_f16(pkg, d_qh, output_planes, n, T, E, H):
    rows = n * T
    out = _Out(pkg, rows * E * (2 if output_planes else 4))
    _launch(pkg, "vh_launch_attention_planes_f16", None, d_qh.ptr, out.ptr, output_planes, n, T, E, H)
    return tr.bf16_planes_to_f32(out.bytes(), rows, E) if output_planes else out.f32(rows, E)


def _assert_mx_is_the_numpy_quantiser_of(rows_f32, d_v, d_s):
    rows, E = rows_f32.shape
    want_v, want_s = mx_ref.quantize(rows_f32)
    got_v = d_v.bytes().reshape(E // 128, rows, 128)
    got_s = mx_ref.from_act_layout(d_s.bytes(), rows, E)
    assert np.array_equal(got_s, want_s)
    zero = (want_v & 0x7f) == 0                                      # signed zeros: compare magnitudes
    assert np.array_equal(got_v[~zero], want_v[~zero]) and np.array_equal(got_v[zero] & 0x7f, want_v[zero] & 0x7f)


def _planes_f16_mx(pkg, d_qh, n, T, E, H):
    rows = n * T
    d_v, d_s = _Out(pkg, rows * E), _Out(pkg, mx_ref.act_scale_bytes(rows, E))
    _launch(pkg, "vh_launch_attention_planes_f16_mx", None, d_qh.ptr, d_v.ptr, d_s.ptr, n, T, E, H)
    return d_v, d_s


# ---- head dim 64 ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arith", list(ARITH))
@pytest.mark.parametrize("case", HD64)
def test_rows_kernels_at_every_tile_count_vs_float64(pkg, device, oracle, case, arith):
    """csrc/attention_f32.hip: vh_launch_attention_rows with each arithmetic, fp32 rows out"""
    k, T, E, H, n, kind = case
    assert (T + 31) // 32 == k and E == 64 * H
    d_q = _dev(pkg, _qkv(oracle, n, T, E, H, kind))
    got = _rows(pkg, d_q, arith, n, T, E, H)
    _hold(f"rows/{arith} {_id(case)}", got, _want(oracle, n, T, E, H, kind, FAMILY[arith]))


@pytest.mark.parametrize("case", HD64)
def test_three_part_planes_at_every_tile_count_vs_float64_and_the_rows_kernel_bitwise(pkg, device, oracle, case):
    """csrc/attention_p3.hip, three parts in, three parts out (the default fp32 path's attention): against float64, and -- the
    same six products per block on the same k assignment -- the bits of vh_launch_attention, as vh_launch_attention_p3's"""
    k, T, E, H, n, kind = case
    assert (T + 31) // 32 == k and E == 64 * H
    rows = n * T
    d_q = _dev(pkg, _qkv(oracle, n, T, E, H, kind))
    got = _planes3(pkg, d_q, n, T, E, H)
    _hold(f"planes3 {_id(case)}", got, _want(oracle, n, T, E, H, kind, "fp32"))
    d_o = _Out(pkg, rows * E * 4)
    _launch(pkg, "vh_launch_attention", None, d_q.ptr, d_o.ptr, n, T, E, H)
    on_rows = d_o.f32(rows, E)
    assert np.array_equal(got, on_rows + 0.0)
    d_p, d_m = _Out(pkg, rows * E * 6), _Out(pkg, rows * E * 4)
    _launch(pkg, "vh_launch_attention_p3", None, d_q.ptr, d_p.ptr, n, T, E, H)
    d_p.bytes()
    _launch(pkg, "vh_launch_merge3_rows", None, d_p.ptr, d_m.ptr, rows, E)
    assert np.array_equal(d_m.f32(rows, E), on_rows + 0.0)


@pytest.mark.parametrize("case", HD64)
def test_fp16_planes_at_every_tile_count_vs_float64_and_its_three_outputs(pkg, device, oracle, case):
    """csrc/attention_p3.hip on one-part fp16 planes (the bf16 and fp8 modes' attention): fp32 rows out against float64 on the
    fp16-rounded operands and bit for bit vh_launch_attention_f16; bf16 planes out = the nearest-even bf16 of those rows and
    the bits of vh_launch_attention_planes_bf16; MX out = the NumPy quantiser's bytes and scale bytes of those rows."""
    k, T, E, H, n, kind = case
    assert (T + 31) // 32 == k and E == 64 * H and E % 128 == 0
    rows = n * T
    qkv = _qkv(oracle, n, T, E, H, kind)
    d_q, d_qh = _dev(pkg, qkv), _f16_planes_in(pkg, qkv)
    got = _planes_f16(pkg, d_qh, 0, n, T, E, H)
    _hold(f"planes_f16 {_id(case)}", got, _want(oracle, n, T, E, H, kind, "fp16"))
    assert np.array_equal(got, _rows(pkg, d_q, "fp16", n, T, E, H))
    as_bf16 = _planes_f16(pkg, d_qh, 1, n, T, E, H)
    assert np.array_equal(as_bf16, tr.bf16_rne(got))
    d_b = _Out(pkg, rows * E * 2)
    _launch(pkg, "vh_launch_attention_planes_bf16", None, d_q.ptr, d_b.ptr, n, T, E, H)
    assert np.array_equal(tr.bf16_planes_to_f32(d_b.bytes(), rows, E), as_bf16)
    _assert_mx_is_the_numpy_quantiser_of(got, *_planes_f16_mx(pkg, d_qh, n, T, E, H))


@pytest.mark.parametrize("k", range(1, 8))
def test_persistent_grids_walk_two_or_three_items_at_every_tile_count(pkg, device, oracle, k):
    """More (image, head) items than twice the compute units, and not a multiple of them: every workgroup prefetches the
    next item's K and Q under this one's softmax, and the grid ends raggedly.  The rows kernel and the three forms the
    forward runs -- three-part planes; fp16 planes writing bf16 planes and MX, through the fp32 rows they are the rounding
    of -- every row against float64.  Plain inputs: every key carries weight, so K, Q or V of another item, or a buffer read
    before it has landed, moves every probability (on the sink inputs all queries of all items agree on the sink)."""
    from test_gpu_p3 import _cus
    E, H, _ = tr.HD64_SHAPE
    T, n = tr.hd64_loop_T(k), tr.loop_images(_cus(), H)
    assert (T + 31) // 32 == k and 2 * _cus() < n * H < 3 * _cus()
    qkv = tr.make_qkv(oracle.synth_fill, n, T, E, H, "plain", 7100 + T)
    want32, want16 = tr.expectation(qkv, n, T, H, "fp32"), tr.expectation(qkv, n, T, H, "fp16")
    d_q = _dev(pkg, qkv)
    _hold(f"loop rows/split3 k{k}", _rows(pkg, d_q, "split3", n, T, E, H), want32)
    _hold(f"loop planes3 k{k}", _planes3(pkg, d_q, n, T, E, H), want32)
    del d_q
    d_qh = _f16_planes_in(pkg, qkv)
    rows_out = _planes_f16(pkg, d_qh, 0, n, T, E, H)
    _hold(f"loop planes_f16 k{k}", rows_out, want16)
    # the two operand outputs the forward runs: the same bound through the bits they promise
    assert np.array_equal(_planes_f16(pkg, d_qh, 1, n, T, E, H), tr.bf16_rne(rows_out))
    _assert_mx_is_the_numpy_quantiser_of(rows_out, *_planes_f16_mx(pkg, d_qh, n, T, E, H))


# ---- head dim 80 ---------------------------------------------------------------------------------------------------------

def _h16_forms(pkg, label, qkv, want, n, T, E, H):
    rows = n * T
    d_qh = _f16_planes_in(pkg, qkv)
    d_o = _Out(pkg, rows * E * 4)
    _launch(pkg, "vh_launch_attention_planes_f16_hd80", None, d_qh.ptr, d_o.ptr, n, T, E, H)
    got = d_o.f32(rows, E)
    _hold(f"hd80 {label}", got, want)
    d_b = _Out(pkg, rows * E * 2)
    _launch(pkg, "vh_launch_attention_planes_f16_hd80_operand", None, d_qh.ptr, d_b.ptr, None, 1, n, T, E, H)
    assert np.array_equal(tr.bf16_planes_to_f32(d_b.bytes(), rows, E), tr.bf16_rne(got))
    d_v, d_s = _Out(pkg, rows * E), _Out(pkg, mx_ref.act_scale_bytes(rows, E))
    _launch(pkg, "vh_launch_attention_planes_f16_hd80_operand", None, d_qh.ptr, d_v.ptr, d_s.ptr, 2, n, T, E, H)
    _assert_mx_is_the_numpy_quantiser_of(got, d_v, d_s)


@pytest.mark.parametrize("case", H16)
def test_head_dim_80_at_its_tile_and_round_edges_vs_float64(pkg, device, oracle, case):
    """csrc/attention_h16.hip: fp32 rows against float64 on the fp16-rounded operands; the bf16-planes operand = the
    nearest-even bf16 of those rows; the MX operand = the NumPy quantiser's bytes of those rows."""
    T, kind = case
    E, H, n = tr.H16_SHAPE
    assert tr.h16_shape(T) == {16: (1, 1), 17: (2, 1), 144: (9, 1), 145: (10, 2), 256: (16, 2), 271: (17, 2)}[T] and E == 80 * H
    qkv = _qkv(oracle, n, T, E, H, kind, tile=16)
    _h16_forms(pkg, f"T{T}-{kind}", qkv, _want(oracle, n, T, E, H, kind, "fp16", tile=16), n, T, E, H)


def test_head_dim_80_grid_walks_more_than_two_head_pairs_per_workgroup(pkg, device, oracle):
    """More head pairs than twice the compute units, raggedly: the K / Q prefetch and the carried half block across items"""
    from test_gpu_p3 import _cus
    E, H, _ = tr.H16_SHAPE
    T, n = 145, tr.loop_images(_cus(), H // 2)
    assert tr.h16_shape(T) == (10, 2) and n * H // 2 > 2 * _cus() and (n * H // 2) % _cus() != 0
    qkv = tr.make_qkv(oracle.synth_fill, n, T, E, H, "plain", 7100 + T, tile=16)
    _h16_forms(pkg, "loop T145", qkv, tr.expectation(qkv, n, T, H, "fp16"), n, T, E, H)
