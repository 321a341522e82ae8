"""The streaming attention kernels at every class, tile and chunk edge, against float64 (tests/attn_tiles_ref.py).

csrc/attention_tiled.hip (fp32 Q|K|V rows, a query's score row in NJ = 8 / 17 / 32 register tiles for T <= 128 / 272 / 512,
K and V streamed in 64-key chunks, two-pass softmax: ViT-H/14 on the fp32 path) and csrc/attention_long.hip (Q|K|V planes,
online softmax over 64-key chunks through a ring of two stages: every model above 512 tokens).  As for the resident kernels
(tests/test_gpu_attention_tiles.py): every case first asserts the class or chunk count it was written for, writes into a
buffer pre-filled with 0xff bytes that ends in 256 guard bytes, and compares ALL rows, per element, with the reference at
the bound of its family (fp32: 2e-5 max(1, A); fp16 operands: half an fp16 ulp of every probability on top -- derived in
attn_tiles_ref.py, and shown by tests/test_attn_tiles_host.py to reject a kernel that drops, doubles or misplaces the last
key, skips a rescale or reads a ring stage one chunk stale).  Where the launcher promises a routing (AUTO = STREAMING
outside the resident shapes) or batch independence, the bits are held to that."""
import numpy as np
import pytest

import attn_ref as ar
import attn_tiles_ref as tr
from test_gpu_attention_tiles import _Out, _dev, _hold, _launch

pytestmark = pytest.mark.gpu

NATIVE, FP16 = 0, 1                    # VH_ATTN_*: arith
AUTO, STREAMING = 0, 1                 # VH_ATTN_*: kernel
TILED = [pytest.param((nj, T, shape), id=f"nj{nj}-T{T}-hd{shape[0] // shape[1]}")
         for shape in tr.TILED_SHAPES for nj, Ts in tr.TILED_TABLE.items() for T in Ts]
LONG = [pytest.param((c, T, shape), id=f"c{c}-T{T}-hd{shape[0] // shape[1]}") for shape in tr.LONG_SHAPES for c, T in tr.LONG_TABLE]
FAMILY_OF_PARTS = {3: "fp32", 1: "fp16"}

_INPUTS = {}


def _qkv(oracle, n, T, E, H, kind):
    """the input of a case, shared by the tests of both operand forms and left unchanged; the last few only (the long
    table's largest are 8 MB each)"""
    key = (n, T, E, H, kind)
    if key not in _INPUTS:
        if len(_INPUTS) >= 12:
            _INPUTS.pop(next(iter(_INPUTS)))
        qkv = tr.make_qkv(oracle.synth_fill, n, T, E, H, kind, 7000 + T, tr.KC)
        qkv.setflags(write=False)
        _INPUTS[key] = qkv
    return _INPUTS[key]


def _kinds(T, kinds):
    return [kind for kind in kinds if T > 1 or kind == "plain"]


def _tiled(pkg, d_q, arith, kernel, n, T, E, H):
    out = _Out(pkg, n * T * E * 4)
    _launch(pkg, "vh_launch_attention_rows", None, d_q.ptr, out.ptr, 0, arith, kernel, n, T, E, H)
    return out.f32(n * T, E)


def _long(pkg, qkv, parts, n, T, E, H):
    """vh_launch_attention_long on the host encoding of the rows: the exact three-part planes or the fp16 planes"""
    d_in = ar.upload(pkg, ar.encode_planes3(qkv) if parts == 3 else ar.encode_f16(qkv))
    out = _Out(pkg, n * T * E * 4)
    _launch(pkg, "vh_launch_attention_long", None, d_in.ptr, parts, out.ptr, n, T, E, H)
    return out.f32(n * T, E)


# ---- csrc/attention_tiled.hip --------------------------------------------------------------------------------------------

def _tiled_case(pkg, oracle, case, arith, family):
    nj, T, (E, H, n) = case
    D = E // H
    shape = tr.tiled_shape(T)
    assert shape.nj == nj and shape.tiles <= nj and shape.chunks <= (nj + 3) // 4 and T <= tr.TILED_LIMIT and D in (64, 80, 128)
    for kind in _kinds(T, tr.KINDS):
        qkv = _qkv(oracle, n, T, E, H, kind)
        d_q = _dev(pkg, qkv)
        got = _tiled(pkg, d_q, arith, STREAMING, n, T, E, H)
        _hold(f"tiled/{family} nj{nj} T{T} hd{D} {kind}", got, tr.expectation(qkv, n, T, H, family))
        if arith == NATIVE and (D != 64 or T > tr.HD64_LIMIT):      # no resident kernel takes the shape: AUTO streams it
            assert np.array_equal(_tiled(pkg, d_q, arith, AUTO, n, T, E, H).view(np.uint32), got.view(np.uint32))


@pytest.mark.parametrize("case", TILED)
def test_tiled_kernel_fp32_products_at_every_class_and_chunk_edge_vs_float64(pkg, device, oracle, case):
    """vh_launch_attention_rows(NATIVE, STREAMING): the fp32 matrix instruction, plain and sink inputs; AUTO gives the same
    bits wherever the shape is the streaming kernel's alone"""
    _tiled_case(pkg, oracle, case, NATIVE, "fp32")


@pytest.mark.parametrize("case", TILED)
def test_tiled_kernel_fp16_operands_at_every_class_and_chunk_edge_vs_float64(pkg, device, oracle, case):
    """vh_launch_attention_rows(FP16, STREAMING): Q, K, V and P rounded to fp16, against float64 on the rounded Q, K, V"""
    _tiled_case(pkg, oracle, case, FP16, "fp16")


# ---- csrc/attention_long.hip ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("parts", [3, 1])
@pytest.mark.parametrize("case", LONG)
def test_long_kernel_at_every_last_chunk_class_vs_float64(pkg, device, oracle, case, parts):
    """vh_launch_attention_long on the exact three-part planes (fp32 family) and on fp16 planes (fp16 family): plain, sink
    (the last chunk holds the maximum: everything before it is rescaled) and mid inputs (chunk 1 holds it)"""
    c, T, (E, H, n) = case
    lc = tr.last_chunk(T)
    assert lc.c == c == (T + 63) // 64 and lc.live == T - 64 * (c - 1) and lc.live in tr.LONG_LIVE and E // H in (64, 80)
    for kind in _kinds(T, tr.LONG_KINDS):
        qkv = _qkv(oracle, n, T, E, H, kind)
        got = _long(pkg, qkv, parts, n, T, E, H)
        _hold(f"long/parts{parts} c{lc.c}-{lc.klass} T{T} hd{E // H} {kind}", got, tr.expectation(qkv, n, T, H, FAMILY_OF_PARTS[parts]))


# ---- an image's rows do not depend on the batch around it ----------------------------------------------------------------

@pytest.mark.parametrize("arith", [NATIVE, FP16], ids=["fp32", "fp16"])
def test_tiled_kernel_gives_an_image_the_same_bits_alone_and_in_a_batch(pkg, device, oracle, arith):
    """T = 257, head dim 80 (ViT-H/14's shape): image 1 of three launched alone"""
    E, H, n = tr.TILED_SHAPES[1]
    T = 257
    assert T in tr.TILED_TABLE[17] and n > 1
    qkv = _qkv(oracle, n, T, E, H, "plain")
    d_q = _dev(pkg, qkv)
    batch = _tiled(pkg, d_q, arith, STREAMING, n, T, E, H)
    alone = _tiled(pkg, _dev(pkg, qkv[T:2 * T]), arith, STREAMING, 1, T, E, H)
    assert np.array_equal(alone.view(np.uint32), batch[T:2 * T].view(np.uint32))
    if arith == NATIVE:                # include/kernelHandler.h: the streaming kernel has ONE fp32 form, whatever split is named
        for other in (2, 3):           # VH_ATTN_FP16X2, VH_ATTN_SPLIT3
            assert np.array_equal(_tiled(pkg, d_q, other, STREAMING, n, T, E, H).view(np.uint32), batch.view(np.uint32))


@pytest.mark.parametrize("parts", [3, 1])
def test_long_kernel_gives_an_image_the_same_bits_alone_and_in_a_batch(pkg, device, oracle, parts):
    """T = 161 (three chunks, a ragged last one, two query blocks), head dim 80: image 1 of two launched alone"""
    E, H, n = tr.LONG_SHAPES[1]
    T = 161
    assert (3, T) in tr.LONG_TABLE and tr.last_chunk(T).c == 3 and n > 1
    qkv = _qkv(oracle, n, T, E, H, "plain")
    batch = _long(pkg, qkv, parts, n, T, E, H)
    alone = _long(pkg, qkv[T:2 * T], parts, 1, T, E, H)
    assert np.array_equal(alone.view(np.uint32), batch[T:2 * T].view(np.uint32))
