"""The attention kernels' sweeps over key-tile and key-chunk counts: the case tables, the inputs, a float64 reference of
softmax(Q K^T / sqrt(D)) V, per-element error bounds derived from the number formats, and float32 NumPy emulations of the
kernels' arithmetic with deliberate mistakes, which tests/test_attn_tiles_host.py uses to show that the bounds pass a right
kernel and reject a wrong one.  Nothing here touches a GPU.

    resident kernels (csrc/attention_f32.hip, attention_p3.hip, attention_h16.hip): HD64_TABLE, H16_T, emulate();
        held to it by tests/test_gpu_attention_tiles.py
    streaming kernels (csrc/attention_tiled.hip, attention_long.hip): TILED_TABLE, LONG_TABLE, emulate() / emulate_online();
        held to it by tests/test_gpu_attention_stream.py

The streaming kernels' constants the tables are derived from:

    attention_tiled.hip   KC = 64 keys per LDS chunk = TPC = 4 tiles of 16 keys; 64 queries (four waves of 16) per
                          workgroup; a query's whole score row in registers, NJ 16-key tiles of it: NJ = 8 for T <= 128,
                          17 for T <= 272, 32 for T <= 512 -- NC = ceil(NJ / 4) = 2, 5, 8 chunks, the fifth chunk of
                          NJ = 17 holding ONE tile (j < NJ); a chunk runs where 64 c < T, a tile where 16 j < T, a key
                          is masked where >= T; two-pass softmax (emulate()); head_dim 64, 80, 128
    attention_long.hip    KC = 64 keys per chunk through a ring of TWO (K, V) stages (chunk c in stage c & 1: chunk 2 is
                          the first to reuse one); 128 queries (eight waves of 16) per workgroup; online softmax
                          (emulate_online()); in the last chunk, live = T - 64 (c - 1) keys: Q.K^T tile j runs where
                          16 j < live, P.V pair t where 32 t < live, the mask only where live < 64; head_dim 64, 80; at 80
                          head h starts at column 80 h = 32 p0 + 16 sh, sh = h & 1

Bounds, per output element, with A = sum_k p_k |v_k| (the magnitude the element is summed from):

    fp32 family (exact three-part split, two fp16 parts, the fp32 matrix instruction):
        OP_TOL * max(1, A)                        the project's operator tolerance, per element instead of per output
    fp16 family (Q, K, V and P rounded to fp16; the reference is computed on the fp16-rounded Q, K, V):
        2^-11 * A + T * 2^-25 * max_k |v_k|  +  OP_TOL * max(1, A)
        The one assumption: every probability is rounded ONCE to fp16 -- half an ulp, 2^-11 relative, in the normal range,
        half a subnormal step, 2^-25 absolute, below it -- so the element moves by at most sum_k (2^-11 p_k + 2^-25) |v_k|;
        max_k runs over the keys of the element's own V column.  Everything else accumulates in fp32 (the second term).
        The online form keeps the assumption: the unnormalised e <= 1 is rounded once, and what multiplies it afterwards
        (alpha <= 1 at every later chunk, 1 / l <= 1 at the end) only shrinks that error.

Neither is fitted to a kernel."""
import math
from collections import namedtuple

import numpy as np

OP_TOL = 2e-5
HD64_LIMIT = 208                       # tokens the head-dim-64 resident kernels take
KINDS = ("plain", "sink")
MUTANTS = ("drop_last", "dup_last", "swap_v")
KC = 64                                # keys per LDS chunk of both streaming kernels
LONG_KINDS = KINDS + ("mid",)
ONLINE_MUTANTS = ("no_rescale", "stale_stage")      # what only an online softmax over a ring of stages can get wrong

# ---- head dim 64: one kernel instantiation per count k of 32-key tiles ---------------------------------------------------

LastTile = namedtuple("LastTile", "k lo live klass")


def last_tile(T, tile=32):
    """What the last key tile of a T-token head holds: k = ceil(T / tile) tiles, `live` keys in the last one, and the branch
    of the P.V loop its two 16-key halves take."""
    k = (T + tile - 1) // tile
    lo = tile * (k - 1)
    live = T - lo
    klass = ("one_key" if live == 1 else "first_partial" if live < 16 else "first_full" if live == 16
             else "second_partial" if live < 32 else "full")
    return LastTile(k, lo, live, klass)


# (k, T): for k = 1..6 one live key / first half full, second skipped (staged rows = T) / second half partial with
# T mod 8 = 5 (the native form stages 8-row groups) / full tile.  The limit 208 = 192 + 16 leaves k = 7 no second half:
# one live key, first half partial with T mod 8 = 5 and = 0, and the limit itself.
HD64_TABLE = tuple((k, 32 * (k - 1) + d) for k in range(1, 7) for d in (1, 16, 21, 32)) + ((7, 193), (7, 197), (7, 200), (7, 208))
HD64_SHAPE = (256, 4, 3)               # E, H, n of the table cases
HD64_WIDE = tuple((k, 32 * (k - 1) + 21) for k in range(3, 7))      # E = 768: the MX scale index reaches a second group
HD64_WIDE_SHAPE = (768, 12, 2)


def hd64_loop_T(k):
    """the token count of the loop case of tile count k: workgroups walk two or three (image, head) items"""
    return 197 if k == 7 else 32 * (k - 1) + 21


def loop_images(cus, units_per_image):
    """images such that a persistent grid of `cus` workgroups takes two or three units each, raggedly"""
    return -(-(2 * cus + 3) // units_per_image)


# ---- head dim 80 (csrc/attention_h16.hip): 16-key tiles, nine waves of 16 queries, two rounds ------------------------------

H16_T = (16, 17, 144, 145, 256, 271)   # both sides of a 16-key edge, of the second round's start, and the last tile
H16_SHAPE = (640, 8, 2)                # even head count, both column parities of a head's start, E % 128 == 0


def h16_shape(T):
    """(16-key tiles with a live key, rounds of query tiles that run)"""
    return (T + 15) // 16, 1 if T <= 9 * 16 else 2


# ---- csrc/attention_tiled.hip: a query's score row in NJ register tiles, K and V streamed in 64-key chunks ------------------

# NJ -> T: both class edges; both sides of a 16-key tile edge and of a 64-key chunk edge; one live key in a new chunk (and
# a second / third / ... query block of ONE query: 65, 129, 193, 257, 321, 449); NJ = 17's one-tile fifth chunk (257 .. 272)
TILED_TABLE = {8: (1, 16, 17, 64, 65, 127, 128), 17: (129, 192, 193, 256, 257, 271, 272), 32: (273, 320, 321, 449, 511, 512)}
TILED_SHAPES = ((128, 2, 3), (160, 2, 3), (256, 2, 3))              # (E, H, n): head_dim 64, 80, 128
TILED_LIMIT = 512

TiledShape = namedtuple("TiledShape", "nj chunks tiles qblocks")


def tiled_shape(T):
    """the register class NJ the launcher picks, and the 64-key chunks, 16-key tiles and 64-query blocks that run"""
    return TiledShape(8 if T <= 128 else 17 if T <= 272 else 32, (T + KC - 1) // KC, (T + 15) // 16, (T + 63) // 64)


# ---- csrc/attention_long.hip: online softmax over 64-key chunks, a ring of two stages ------------------------------------------

LastChunk = namedtuple("LastChunk", "c lo live tiles pairs klass")
LONG_LIVE = (1, 16, 17, 32, 33, 48, 49, 63, 64)


def last_chunk(T):
    """What the last 64-key chunk of a T-token head holds: c = ceil(T / 64) chunks, `live` keys in the last one, the Q.K^T
    tiles (16 j < live) and P.V pairs (32 t < live) that run in it, and its branch class: one_key, full (no mask), or
    <tiles run>_<last of them full | partial>."""
    c = (T + KC - 1) // KC
    lo = KC * (c - 1)
    live = T - lo
    tiles, pairs = (live + 15) // 16, (live + 31) // 32
    klass = "one_key" if live == 1 else "full" if live == KC else "{}_{}".format(tiles, "partial" if live % 16 else "full")
    return LastChunk(c, lo, live, tiles, pairs, klass)


# (c, T), T = 64 (c - 1) + live: one chunk and three (the first to reuse a ring stage) at every live; two chunks at one key,
# 33 and full; 256 = two full 128-query blocks, 1024 = 16 chunks with a full last one, 1087 = 17 chunks, 63 live
LONG_TABLE = (tuple((1, d) for d in LONG_LIVE) + tuple((2, 64 + d) for d in (1, 33, 64)) + tuple((3, 128 + d) for d in LONG_LIVE)
              + ((4, 256), (16, 1024), (17, 1087)))
LONG_SHAPES = ((256, 4, 2), (320, 4, 2))                             # (E, H, n): head_dim 64, 80 (both parities sh)


# ---- inputs --------------------------------------------------------------------------------------------------------------

def make_qkv(fill, n, T, E, H, kind, seed, tile=32):
    """fp32 Q|K|V rows [n*T][3E] from fill(count, seed, scale, offset) (the oracle's synth_fill), amplitude 1.
    plain: as filled.  sink: every query gets a common direction; key T - 1 in even heads and the first key of the last
    tile in odd heads lie along it, far enough to out-score every other key by >= 20; V channel 5 of every head is x40.
    mid (the online softmax): as sink, with the dominant key in tile 1 where there are three tiles or more -- key
    tile + 37 % tile in even heads, the tile's last key in odd heads: tile 0 is summed under a maximum that tile 1
    replaces, every later tile under an unchanged one; with fewer tiles, the two middle keys."""
    D = E // H
    x = fill(n * T * 3 * E, seed, 1.0, 0.0).reshape(n, T, 3, H, D)
    if kind == "plain":
        return np.ascontiguousarray(x.reshape(n * T, 3 * E))
    assert kind in ("sink", "mid") and T > 1
    x = x.astype(np.float64)
    if kind == "sink":
        sinks = (T - 1, tile * ((T + tile - 1) // tile - 1))
    elif T > 2 * tile:
        sinks = (tile + 37 % tile, 2 * tile - 1)
    else:
        sinks = ((T - 1) // 2, T // 2)
    x[:, :, 0] += 1.0
    x[:, sinks[0], 1, 0::2] += 40.0 / math.sqrt(D)
    x[:, sinks[1], 1, 1::2] += 40.0 / math.sqrt(D)
    x[:, :, 2, :, 5] *= 40.0
    x = x.astype(np.float32)
    m = min(n, 2)                                                    # the dominance, checked on the first images
    qk = np.ascontiguousarray(x[:m, :, :2].astype(np.float64).transpose(2, 0, 3, 1, 4))             # [2][m][H][T][D]
    s = qk[0] @ qk[1].transpose(0, 1, 3, 2) / math.sqrt(D)
    for par in (0, 1):
        sp = s[:, par::2]
        others = np.delete(sp, sinks[par], axis=3)
        assert others.size == 0 or (sp[..., sinks[par]] - others.max(axis=3) >= 20.0).all()
    return np.ascontiguousarray(x.reshape(n * T, 3 * E))


def round_f16(qkv):
    """the operands the fp16-operand kernels multiply, as fp32"""
    return np.asarray(qkv).astype(np.float16).astype(np.float32)


def _weights_f16(p):
    """non-negative weights rounded to fp16, as fp32: what is at most 2^-25 rounds to zero (the tie to even) and is zeroed
    first -- NumPy converts the same values, but takes a slow path for each that underflows"""
    return np.where(p > np.float32(2.0 ** -25), p, np.float32(0.0)).astype(np.float16).astype(np.float32)


# ---- the reference and the bounds ----------------------------------------------------------------------------------------

def _heads(rows, T, H, dtype):
    """one image's rows [T][3E] -> q, k, v [H][T][D]"""
    D = rows.shape[1] // 3 // H
    x = np.ascontiguousarray(rows.astype(dtype).reshape(T, 3, H, D).transpose(1, 2, 0, 3))      # contiguous: BLAS takes them
    return x[0], x[1], x[2]


def reference(qkv, n, T, H):
    """float64 softmax(Q K^T / sqrt(D)) V per (image, head) of qkv [n*T][3E] -> O [n*T][E], A [n*T][E] = sum_k p_k |v_k|"""
    qkv = np.asarray(qkv)
    E = qkv.shape[1] // 3
    D = E // H
    O, A = np.empty((n * T, E)), np.empty((n * T, E))
    for i in range(n):
        q, k, v = _heads(qkv[i * T:(i + 1) * T], T, H, np.float64)
        s = q @ k.transpose(0, 2, 1) / math.sqrt(D)
        p = np.exp(s - s.max(axis=2, keepdims=True))
        p /= p.sum(axis=2, keepdims=True)
        O[i * T:(i + 1) * T] = (p @ v).transpose(1, 0, 2).reshape(T, E)
        A[i * T:(i + 1) * T] = (p @ np.abs(v)).transpose(1, 0, 2).reshape(T, E)
    return O, A


def v_colmax(qkv, n, T):
    """[n*T][E]: max over the keys of an image of |V| in the element's column"""
    qkv = np.asarray(qkv)
    E = qkv.shape[1] // 3
    m = np.abs(qkv[:, 2 * E:].astype(np.float64)).reshape(n, T, E).max(axis=1, keepdims=True)
    return np.broadcast_to(m, (n, T, E)).reshape(n * T, E)


def bound(family, A, T, vmax=None):
    """per element; see the module's docstring"""
    fp32 = OP_TOL * np.maximum(1.0, A)
    if family == "fp32":
        return fp32
    assert family == "fp16" and vmax is not None
    return 2.0 ** -11 * A + T * 2.0 ** -25 * vmax + fp32


def expectation(qkv, n, T, H, family):
    """(O, bound) a kernel of `family` on the fp32 rows qkv is held to, both [n*T][E] float64"""
    ops = round_f16(qkv) if family == "fp16" else np.asarray(qkv)
    O, A = reference(ops, n, T, H)
    return O, bound(family, A, T, v_colmax(ops, n, T) if family == "fp16" else None)


# ---- the kernels' arithmetic in float32, and three ways to get the last key wrong -----------------------------------------

def emulate(qkv, n, T, H, family, mutate=None):
    """fp32 [n*T][E]: fp32 dot products, e = 2^(s c1 - max c1), p = e * (1 / sum e), O = P V; the fp16 family rounds Q, K, V
    and P to fp16 first.  mutate: drop_last (key T - 1 gets no weight), dup_last (key T - 1 is counted twice: what a mask
    one key too wide does, the staged rows past T being copies of row T - 1), swap_v (V rows of keys T - 1 and T - 2
    exchanged)."""
    assert family in ("fp32", "fp16") and mutate in (None,) + MUTANTS and (mutate is None or T >= 2)
    qkv = np.asarray(qkv, dtype=np.float32)
    E = qkv.shape[1] // 3
    D = E // H
    if family == "fp16":
        qkv = round_f16(qkv)
    c1 = np.float32(1.44269504088896340736) / np.sqrt(np.float32(D))
    out = np.empty((n * T, E), np.float32)
    for i in range(n):
        q, k, v = _heads(qkv[i * T:(i + 1) * T], T, H, np.float32)
        if mutate == "swap_v":
            v[:, [T - 1, T - 2]] = v[:, [T - 2, T - 1]]
        if mutate == "dup_last":
            k, v = np.concatenate([k, k[:, T - 1:]], axis=1), np.concatenate([v, v[:, T - 1:]], axis=1)
        s = q @ k.transpose(0, 2, 1)
        if mutate == "drop_last":
            s[:, :, T - 1] = -np.inf
        c2 = -s.max(axis=2, keepdims=True) * c1
        e = np.exp2(s * c1 + c2, dtype=np.float32)
        p = e * (np.float32(1.0) / e.sum(axis=2, keepdims=True, dtype=np.float32))
        if family == "fp16":
            p = _weights_f16(p)
        out[i * T:(i + 1) * T] = (p @ v).transpose(1, 0, 2).reshape(T, E)
    return out


def emulate_online(qkv, n, T, H, family, mutate=None):
    """fp32 [n*T][E]: csrc/attention_long.hip's arithmetic.  Per 64-key chunk: fp32 dot products, the chunk's maximum,
    m_new = max(m, chunk max), alpha = 2^((m - m_new) c1), e = 2^(s c1 - m_new c1), l = l alpha + sum e,
    O = O alpha + e V; O / l once at the end.  The fp16 family rounds Q, K, V first and e before e V.  mutate: the three of
    emulate(), and no_rescale (alpha = 1 at every chunk after the first: what was summed under an old maximum stays as it
    was), stale_stage (chunk c >= 1 computes on chunk c - 1's K and V: a ring stage read before the next chunk landed)."""
    assert family in ("fp32", "fp16") and mutate in (None,) + MUTANTS + ONLINE_MUTANTS and (mutate is None or T >= 2)
    assert mutate not in ONLINE_MUTANTS or T > KC
    qkv = np.asarray(qkv, dtype=np.float32)
    E = qkv.shape[1] // 3
    D = E // H
    if family == "fp16":
        qkv = round_f16(qkv)
    c1 = np.float32(1.44269504088896340736) / np.sqrt(np.float32(D))
    out = np.empty((n * T, E), np.float32)
    with np.errstate(invalid="ignore"):
        for i in range(n):
            q, k, v = _heads(qkv[i * T:(i + 1) * T], T, H, np.float32)
            if mutate == "swap_v":
                v[:, [T - 1, T - 2]] = v[:, [T - 2, T - 1]]
            m = np.full((H, T, 1), -np.inf, np.float32)
            l = np.zeros((H, T, 1), np.float32)
            O = np.zeros((H, T, D), np.float32)
            for lo in range(0, T, KC):
                hi = min(lo + KC, T)
                src = lo - KC if mutate == "stale_stage" and lo else lo
                kc, vc = k[:, src:src + hi - lo], v[:, src:src + hi - lo]
                if mutate == "dup_last" and hi == T:
                    kc, vc = np.concatenate([kc, kc[:, -1:]], axis=1), np.concatenate([vc, vc[:, -1:]], axis=1)
                s = q @ kc.transpose(0, 2, 1)
                if mutate == "drop_last" and hi == T:
                    s[:, :, T - 1 - lo] = -np.inf
                m_new = np.maximum(m, s.max(axis=2, keepdims=True))
                if lo == 0:
                    assert np.isfinite(m_new).all()
                    alpha = np.zeros_like(m)                             # 2^(-inf - m_new): nothing has been summed yet
                elif mutate == "no_rescale":
                    alpha = np.ones_like(m)
                else:
                    alpha = np.exp2((m - m_new) * c1, dtype=np.float32)
                e = np.exp2(s * c1 - m_new * c1, dtype=np.float32)
                l = l * alpha + e.sum(axis=2, keepdims=True, dtype=np.float32)
                if family == "fp16":
                    e = _weights_f16(e)
                O = O * alpha + e @ vc
                m = m_new
            out[i * T:(i + 1) * T] = (O / l).transpose(1, 0, 2).reshape(T, E)
    return out


# ---- formats -------------------------------------------------------------------------------------------------------------

def bf16_rne(x):
    """fp32 -> nearest-even bfloat16 as fp32 (finite inputs)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def bf16_planes_to_f32(raw, rows, cols):
    """bytes of one-part bf16 planes [cols/32][rows][32] -> fp32 [rows][cols]"""
    u = np.frombuffer(raw, dtype=np.uint16, count=rows * cols).reshape(cols // 32, rows, 32)
    return np.ascontiguousarray((u.astype(np.uint32) << 16).view(np.float32).transpose(1, 0, 2).reshape(rows, cols))
