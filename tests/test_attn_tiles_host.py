"""The attention sweeps, the part that needs no GPU (tests/attn_tiles_ref.py): the case tables cover what they claim,
the error bounds pass a float32 emulation of the kernels' arithmetic on every element of every table case, and reject each
of three mistakes at the last key on every table case -- and, for the online softmax of csrc/attention_long.hip, a missing
rescale and a stale ring stage.  tests/test_gpu_attention_tiles.py (the resident kernels) and
tests/test_gpu_attention_stream.py (the streaming ones) hold the kernels to the same reference and bounds."""
import numpy as np
import pytest

import attn_tiles_ref as tr

FAMILIES = ("fp32", "fp16")


def _table_cases():
    """(n, T, E, H, kind, tile) of every table case of both head dims"""
    E, H, n = tr.HD64_SHAPE
    cases = [(n, T, E, H, kind, 32) for _, T in tr.HD64_TABLE for kind in tr.KINDS if T > 1 or kind == "plain"]
    E, H, n = tr.H16_SHAPE
    return cases + [(n, T, E, H, kind, 16) for T in tr.H16_T for kind in tr.KINDS]


@pytest.fixture(scope="module")
def table(oracle):
    """every table case's input and, per family, what a kernel is held to -- computed once for the tests below"""
    out = []
    for n, T, E, H, kind, tile in _table_cases():
        qkv = tr.make_qkv(oracle.synth_fill, n, T, E, H, kind, 7000 + T, tile)
        out.append(((n, T, E, H, kind), qkv, {f: tr.expectation(qkv, n, T, H, f) for f in FAMILIES}))
    return out


def test_the_tables_hold_every_tile_count_in_each_of_its_classes():
    by_k = {}
    for k, T in tr.HD64_TABLE:
        lt = tr.last_tile(T)
        assert lt.k == k == (T + 31) // 32 and 1 <= T <= tr.HD64_LIMIT
        by_k.setdefault(k, []).append((T, lt))
    assert sorted(by_k) == [1, 2, 3, 4, 5, 6, 7]
    for k in range(1, 7):
        assert sorted(lt.klass for _, lt in by_k[k]) == ["first_full", "full", "one_key", "second_partial"]
        for T, lt in by_k[k]:
            if lt.klass == "second_partial":
                assert 17 <= T % 32 <= 31 and T % 8 == 5             # the native form's last 8-row group is partial too
            if lt.klass == "first_full":
                assert T % 16 == 0                                   # staged rows = T: nothing past the last key is staged
    # the limit, 208 = 192 + 16, leaves the seventh tile no second half
    assert [(T, lt.klass) for T, lt in by_k[7]] == [(193, "one_key"), (197, "first_partial"), (200, "first_partial"), (208, "first_full")]
    assert 197 % 8 == 5 and 200 % 8 == 0 and by_k[7][-1][0] == tr.HD64_LIMIT
    for k in range(1, 8):                                            # the loop cases and the wide cases stay in their tile count
        assert tr.last_tile(tr.hd64_loop_T(k)).k == k and tr.last_tile(tr.hd64_loop_T(k)).klass in ("second_partial", "first_partial")
    assert [tr.last_tile(T).k for _, T in tr.HD64_WIDE] == [k for k, _ in tr.HD64_WIDE] == [3, 4, 5, 6]
    assert tr.HD64_WIDE_SHAPE[0] // 128 > 4                          # a second group of four K steps of MX scales
    # a persistent grid takes two or three items per workgroup, and not the same number everywhere
    for cus in (256, 304, 64):
        items = tr.loop_images(cus, tr.HD64_SHAPE[1]) * tr.HD64_SHAPE[1]
        assert 2 * cus < items < 3 * cus
    # head dim 80: both sides of a 16-key edge and of the second round's start
    assert {16, 17} <= set(tr.H16_T) and tr.h16_shape(16) == (1, 1) and tr.h16_shape(17) == (2, 1)
    assert {144, 145} <= set(tr.H16_T) and tr.h16_shape(144) == (9, 1) and tr.h16_shape(145) == (10, 2)
    assert tr.h16_shape(256) == (16, 2) and tr.h16_shape(271) == (17, 2) and max(tr.H16_T) <= 272
    E, H, _ = tr.H16_SHAPE
    assert E == 80 * H and H % 2 == 0 and E % 128 == 0 and {(80 * h // 16) & 1 for h in range(H)} == {0, 1}


def test_the_reference_is_the_definition():
    rng = np.random.default_rng(3)
    n, T, H, D = 2, 37, 3, 16
    qkv = rng.standard_normal((n * T, 3 * H * D)).astype(np.float32)
    O, A = tr.reference(qkv, n, T, H)
    i, h, t, d = 1, 2, 30, 7
    x = qkv[i * T:(i + 1) * T].astype(np.float64)
    q, K, V = x[t, h * D:(h + 1) * D], x[:, H * D + h * D:H * D + (h + 1) * D], x[:, 2 * H * D + h * D + d]
    s = K @ q / np.sqrt(D)
    p = np.exp(s - s.max()) / np.exp(s - s.max()).sum()
    assert abs(O[i * T + t, h * D + d] - p @ V) < 1e-14 and abs(A[i * T + t, h * D + d] - p @ np.abs(V)) < 1e-14
    assert (np.abs(O) <= A + 1e-15).all()
    one, a_one = tr.reference(qkv[:3], 3, 1, H)                      # T = 1: every query returns its only V row
    assert np.array_equal(one, qkv[:3, 2 * H * D:].astype(np.float64)) and np.array_equal(a_one, np.abs(one))
    assert np.array_equal(tr.v_colmax(qkv, n, T)[T + 3], np.abs(qkv[T:, 2 * H * D:]).max(axis=0))
    b32, b16 = tr.bound("fp32", A, T), tr.bound("fp16", A, T, tr.v_colmax(qkv, n, T))
    assert (b32 >= tr.OP_TOL).all() and (b16 > b32 + 2.0 ** -11 * A).all()


def test_the_bounds_pass_the_emulated_kernels_on_every_element(table):
    worst = {(f, kind): (0.0, ()) for f in FAMILIES for kind in tr.KINDS}
    for (n, T, E, H, kind), qkv, want in table:
        for f in FAMILIES:
            O, bnd = want[f]
            got = tr.emulate(qkv, n, T, H, f)
            ratio = float((np.abs(got - O) / bnd).max())
            assert np.isfinite(got).all() and ratio <= 1.0, (f, kind, T, E, ratio)
            worst[f, kind] = max(worst[f, kind], (ratio, (T, E)))
    for (f, kind), (ratio, where) in sorted(worst.items()):
        print(f"\nemulated {f} kernel, {kind} inputs: largest err/bound {ratio:.3f} at (T, E) = {where}")


def test_the_bounds_reject_a_kernel_that_gets_the_last_key_wrong(table):
    """Each mistake exceeds the bound somewhere at every table token count T >= 2 -- a condition, not a measurement.  On the
    plain inputs every mistake must show; on the sink inputs dropping the last key and exchanging its V row must.  Counting
    the last key twice cannot show there: where it is the sink it holds all the weight once or twice over, elsewhere it
    holds e^-20 of it -- that mistake is the plain inputs' to catch, at every T."""
    weakest = {f: (np.inf, ()) for f in FAMILIES}
    seen = {}
    for (n, T, E, H, kind), qkv, want in table:
        if T < 2:
            continue
        for f in FAMILIES:
            O, bnd = want[f]
            for mutant in tr.MUTANTS:
                excess = float((np.abs(tr.emulate(qkv, n, T, H, f, mutant) - O) / bnd).max())
                if kind == "plain" or mutant != "dup_last":
                    assert excess > 1.0, (f, kind, T, E, mutant, excess)
                    weakest[f] = min(weakest[f], (excess, (mutant, kind, T, E)))
                seen[T, E, f, mutant] = max(seen.get((T, E, f, mutant), 0.0), excess)
    tables = [(T, tr.HD64_SHAPE[0]) for _, T in tr.HD64_TABLE if T >= 2] + [(T, tr.H16_SHAPE[0]) for T in tr.H16_T]
    assert all(seen[T, E, f, m] > 1.0 for T, E in tables for f in FAMILIES for m in tr.MUTANTS)
    for f, (excess, where) in weakest.items():
        print(f"\n{f} bound: the weakest mutant exceeds it {excess:.1f} times: {where}")


# ---- the streaming kernels (csrc/attention_tiled.hip, csrc/attention_long.hip) --------------------------------------------

def _stream_cases():
    """(kernel, n, T, E, H, kind) of every case of both streaming tables"""
    tiled = [("tiled", n, T, E, H, kind) for E, H, n in tr.TILED_SHAPES for Ts in tr.TILED_TABLE.values() for T in Ts
             for kind in tr.KINDS if T > 1 or kind == "plain"]
    return tiled + [("long", n, T, E, H, kind) for E, H, n in tr.LONG_SHAPES for _, T in tr.LONG_TABLE
                    for kind in tr.LONG_KINDS if T > 1 or kind == "plain"]


def _stream_emulation(kernel):
    return tr.emulate if kernel == "tiled" else tr.emulate_online


def test_the_streaming_tables_hold_every_class_edge_and_every_last_chunk_class():
    # tiled: every T in the class it is listed under and inside the kernel's range; both edges of every class
    edges = {8: (1, 128), 17: (129, 272), 32: (273, tr.TILED_LIMIT)}
    for nj, Ts in tr.TILED_TABLE.items():
        assert all(tr.tiled_shape(T).nj == nj and 1 <= T <= tr.TILED_LIMIT for T in Ts) and set(edges[nj]) <= set(Ts)
        assert tr.tiled_shape(edges[nj][1]).tiles <= nj
        assert any(T % 16 == 0 and T + 1 in Ts for T in Ts)          # both sides of a 16-key tile edge
        assert any(T % 64 == 0 and T + 1 in Ts for T in Ts)          # ... of a 64-key chunk edge: one live key in a new chunk
        assert any(T % 64 == 1 and T > 64 for T in Ts)               # a last query block of one query
    assert {T for T in tr.TILED_TABLE[17] if tr.tiled_shape(T).chunks == 5} == {257, 271, 272}      # the one-tile fifth chunk
    assert all(tr.tiled_shape(T).tiles == 17 for T in (257, 271, 272))
    assert [E // H for E, H, _ in tr.TILED_SHAPES] == [64, 80, 128] and all(H == 2 and n == 3 for _, H, n in tr.TILED_SHAPES)
    # long: T = 64 (c - 1) + live; every live-key class of the last chunk at one chunk and at three
    by_c = {}
    for c, T in tr.LONG_TABLE:
        lc = tr.last_chunk(T)
        assert lc.c == c == (T + 63) // 64 and T == 64 * (c - 1) + lc.live and 1 <= lc.live <= 64 and lc.tiles == -(-lc.live // 16) and lc.pairs == -(-lc.live // 32)
        by_c.setdefault(lc.c, []).append(lc)
    classes = {"one_key", "1_full", "2_partial", "2_full", "3_partial", "3_full", "4_partial", "full"}
    assert {tr.last_chunk(live).klass for live in range(1, 65)} == classes | {"1_partial"}
    for c in (1, 3):
        assert [lc.live for lc in by_c[c]] == list(tr.LONG_LIVE) and {lc.klass for lc in by_c[c]} == classes
    assert [lc.live for lc in by_c[2]] == [1, 33, 64]
    assert (tr.last_chunk(256).c, tr.last_chunk(256).klass) == (4, "full") and 256 % 128 == 0
    assert (tr.last_chunk(1024).c, tr.last_chunk(1024).klass) == (16, "full")
    assert (tr.last_chunk(1087).c, tr.last_chunk(1087).live) == (17, 63)
    assert any(T % 16 == 0 and T % 128 for _, T in tr.LONG_TABLE)       # a full last query wave in a partial block
    assert [E // H for E, H, _ in tr.LONG_SHAPES] == [64, 80]
    E, H, _ = tr.LONG_SHAPES[1]
    assert E % 32 == 0 and {(80 * h // 16) & 1 for h in range(H)} == {0, 1}      # both column parities of a head's start


def test_the_mid_inputs_put_the_dominant_key_in_chunk_one(oracle):
    E, H, n = tr.LONG_SHAPES[0]
    D, T = E // H, 129
    x = tr.make_qkv(oracle.synth_fill, n, T, E, H, "mid", 7000 + T, 64).astype(np.float64).reshape(n, T, 3, H, D)
    top = np.einsum("btha,bsha->bhts", x[:, :, 0], x[:, :, 1]).argmax(axis=3)
    assert (top[:, 0::2] == 64 + 37).all() and (top[:, 1::2] == 127).all()
    small = tr.make_qkv(oracle.synth_fill, n, 17, E, H, "mid", 7017, 64).astype(np.float64).reshape(n, 17, 3, H, D)
    top = np.einsum("btha,bsha->bhts", small[:, :, 0], small[:, :, 1]).argmax(axis=3)
    assert (top[:, 0::2] == 8).all() and (top[:, 1::2] == 8).all()


@pytest.fixture(scope="module")
def stream_sweep(oracle):
    """Per case of both streaming tables and per family: the largest err / bound of the emulated kernel, and of each
    mutant that applies -- every input, reference and emulation computed once, for the two tests below."""
    def one(case):
        kernel, n, T, E, H, kind = case
        qkv = tr.make_qkv(oracle.synth_fill, n, T, E, H, kind, 7000 + T, tr.KC)
        emu = _stream_emulation(kernel)
        mutants = tr.MUTANTS if T >= 2 else ()
        if kernel == "long" and T > tr.KC:
            mutants = mutants + tr.ONLINE_MUTANTS
        out = []
        for f in FAMILIES:
            O, bnd = tr.expectation(qkv, n, T, H, f)
            got = emu(qkv, n, T, H, f)
            assert np.isfinite(got).all(), (kernel, f, kind, T, E)
            ratios = {None: float((np.abs(got - O) / bnd).max())}
            for mutant in mutants:
                ratios[mutant] = float((np.abs(emu(qkv, n, T, H, f, mutant) - O) / bnd).max())
            out.append(((kernel, T, E, kind, f), ratios))
        return out

    return sum(map(one, _stream_cases()), [])


def test_the_bounds_pass_the_emulated_streaming_kernels_on_every_element(stream_sweep):
    worst = {}
    for (kernel, T, E, kind, f), ratios in stream_sweep:
        assert ratios[None] <= 1.0, (kernel, f, kind, T, E, ratios[None])
        worst[kernel, f, kind] = max(worst.get((kernel, f, kind), (0.0, ())), (ratios[None], (T, E)))
    for (kernel, f, kind), (ratio, where) in sorted(worst.items()):
        print(f"\nemulated {kernel} kernel, {f}, {kind} inputs: largest err/bound {ratio:.3f} at (T, E) = {where}")


def test_the_bounds_reject_a_streaming_kernel_that_gets_a_key_a_rescale_or_a_stage_wrong(stream_sweep):
    """Every mistake exceeds the bound somewhere at every table token count where it applies (the last-key mistakes at
    T >= 2, the online ones at two chunks or more), in both families and at every head dim -- a condition, not a
    measurement.  As for the resident tables, counting the last key twice is the plain inputs' to catch, and the sink inputs
    must show a dropped last key and an exchanged V row.  A stale stage must show on the plain inputs (every probability
    moves) and on the sink inputs (the chunk that holds the sink is never read); on the mid inputs it need not: the dominant
    key is still counted once, a chunk late.  A missing rescale shows only where a later chunk raises the maximum: it must
    on the sink inputs and, at three chunks or more, on the mid inputs; on the plain ones wherever the fill does."""
    must_show = {"plain": tr.MUTANTS + ("stale_stage",), "sink": ("drop_last", "swap_v", "stale_stage", "no_rescale"),
                 "mid": ("no_rescale",)}
    seen, weakest = {}, {}
    for (kernel, T, E, kind, f), ratios in stream_sweep:
        for mutant, excess in ratios.items():
            if mutant is None or (mutant == "dup_last" and kind != "plain"):
                continue
            must = mutant in must_show[kind] and (kind != "mid" or tr.last_chunk(T).c >= 3)
            if must:
                assert excess > 1.0, (kernel, f, kind, T, E, mutant, excess)
                weakest[kernel, f] = min(weakest.get((kernel, f), (np.inf, ())), (excess, (mutant, kind, T, E)))
            seen[kernel, T, E, f, mutant] = max(seen.get((kernel, T, E, f, mutant), 0.0), excess)
    for kernel, shapes, Ts in (("tiled", tr.TILED_SHAPES, sum(tr.TILED_TABLE.values(), ())), ("long", tr.LONG_SHAPES, tuple(T for _, T in tr.LONG_TABLE))):
        for E, _, _ in shapes:
            for T in Ts:
                mutants = (tr.MUTANTS if T >= 2 else ()) + (tr.ONLINE_MUTANTS if kernel == "long" and T > tr.KC else ())
                for f in FAMILIES:
                    assert all(seen[kernel, T, E, f, m] > 1.0 for m in mutants), (kernel, T, E, f)
    for (kernel, f), (excess, where) in sorted(weakest.items()):
        print(f"\n{kernel} kernel, {f} bound: the weakest mutant exceeds it {excess:.1f} times: {where}")
