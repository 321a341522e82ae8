"""Host side of the gallery search (no GPU): the judge itself (tests/gallery_ref.py `check` accepts the float64 scores
rounded to fp32 and ranked, and rejects a swapped pair, a duplicate, a missed best row and a score off by four bounds),
vit_gallery_check's acceptances and refusals through the library, and the ctypes mirror of the header's struct."""
import ctypes as C

import numpy as np
import pytest

import gallery_ref as gr

N, G, E, K = 5, 300, 64, 8


@pytest.fixture(scope="module")
def ranked():
    """unit gaussian queries and rows; the float64 scores rounded to fp32, ranked by the rule"""
    rng = np.random.default_rng(7)
    q = rng.standard_normal((N, E)).astype(np.float32)
    rows = rng.standard_normal((G, E)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    s32 = gr.scores64(q, rows).astype(np.float32)
    idx = gr.rank_exact(s32, K)
    return q, rows, idx, np.take_along_axis(s32, idx, axis=1)


def test_check_accepts_the_rounded_float64_ranking(ranked):
    q, rows, idx, sc = ranked
    assert gr.check(q, rows, K, idx, sc) <= 1.0 / (E + 8) + 1e-9   # one rounding against a bound of E + 8 of them
    # ... and with k == G, where nothing is left out
    few = rows[:K]
    s32 = gr.scores64(q, few).astype(np.float32)
    idx_all = gr.rank_exact(s32, K)
    gr.check(q, few, K, idx_all, np.take_along_axis(s32, idx_all, axis=1))


def test_check_rejects_what_is_wrong(ranked):
    q, rows, idx, sc = ranked
    ref, bnd = gr.scores64(q, rows), gr.bound(q, rows, E)
    # positions 0 and K - 1 of query 0 are clearly separated on this data: far more than both bounds apart
    assert ref[0, idx[0, 0]] - ref[0, idx[0, -1]] > 100 * (bnd[0, idx[0, 0]] + bnd[0, idx[0, -1]])

    swapped_i, swapped_s = idx.copy(), sc.copy()
    swapped_i[0, [0, -1]], swapped_s[0, [0, -1]] = idx[0, [-1, 0]], sc[0, [-1, 0]]
    with pytest.raises(AssertionError, match="out of order"):
        gr.check(q, rows, K, swapped_i, swapped_s)

    dup_i, dup_s = idx.copy(), sc.copy()
    dup_i[1, 3], dup_s[1, 3] = idx[1, 2], sc[1, 2]
    with pytest.raises(AssertionError, match="duplicate"):
        gr.check(q, rows, K, dup_i, dup_s)

    # the best row left out: positions 1..K of the ranking instead of 0..K-1
    s32 = ref.astype(np.float32)
    wide = gr.rank_exact(s32, K + 1)
    missed_i = np.ascontiguousarray(wide[:, 1:])
    missed_i[1:] = idx[1:]
    missed_s = np.take_along_axis(s32, missed_i, axis=1)
    with pytest.raises(AssertionError, match="beats the k-th"):
        gr.check(q, rows, K, missed_i, missed_s)

    # a score off by four bounds, in the last position so that the order still holds
    off = sc.copy()
    off[2, -1] = np.float32(ref[2, idx[2, -1]] - 4 * bnd[2, idx[2, -1]])
    with pytest.raises(AssertionError, match="beyond the bound"):
        gr.check(q, rows, K, idx, off)

    out_i = idx.copy()
    out_i[3, 0] = G
    with pytest.raises(AssertionError, match="out of range"):
        gr.check(q, rows, K, out_i, sc)


def test_rank_rule_on_special_values():
    """-0 == +0 by index, NaN below -inf, NaNs by index: the rule of vh_launch_topk"""
    s = np.array([[-np.inf, np.nan, 0.0, -0.0, np.inf, np.nan, 1.0, np.inf]], np.float32)
    assert gr.rank_exact(s, 8).tolist() == [[4, 7, 6, 2, 3, 0, 1, 5]]


def test_bf16_helpers():
    a = np.array([1.0, -2.5, 3.0, 0.1, 1e-3], np.float32)
    back = gr.bf16_decode(gr.bf16_round(a))
    assert (back[:3] == a[:3]).all() and np.abs(back - a).max() <= np.abs(a).max() * 2.0 ** -8


def spec_c(b, **kw):
    args = dict(k=5, source="cls", tap=-1, final_norm=True, l2_normalize=True, dtype="f32", n_rows=1000, row_stride=768, d_rows=None)
    args.update(kw)
    return b.GallerySpec(**args)


def test_gallery_check_accepts_and_sizes(pkg):
    b = pkg.binding
    cfg = pkg.preset("vit_b_16")
    tiles = lambda g: -(-g // b.GALLERY_ROW_TILE)
    for kw in (dict(), dict(source="pooled", tap=0), dict(tap=-12, k=1, n_rows=1), dict(tap=11, k=32, n_rows=32),
               dict(dtype="bf16", row_stride=776), dict(row_stride=772), dict(n_rows=2 ** 31 - 1), dict(final_norm=False, l2_normalize=False)):
        s = spec_c(b, **kw)
        want = 768 * 4 + min(b.GALLERY_MAX_SPLITS, tiles(s.n_rows)) * s.k * 8
        assert b.gallery_check(cfg, s) == want, kw
    # the two figures the header quotes: a million rows at k = 5 and k = 32
    assert b.gallery_check(cfg, spec_c(b, n_rows=10 ** 6)) == 3072 + 1024 * 5 * 8 == 44_032
    assert b.gallery_check(cfg, spec_c(b, n_rows=10 ** 6, k=32)) == 3072 + 1024 * 32 * 8 == 265_216
    # it is vh_gallery_workspace's bound per query plus the query; the pointer may be NULL
    L = pkg.lib()
    assert L.vh_gallery_workspace(1, 1000, 5, 0) == 8 * 5 * 8 and L.vh_gallery_workspace(3, 1000, 5, 7) == 3 * 7 * 5 * 8
    cs = spec_c(b).c_struct()
    assert L.vit_gallery_check(C.byref(cfg), C.byref(cs), None) == 0
    assert L.vh_gallery_query_tile(1) == L.vh_gallery_query_tile(16) == 16 and L.vh_gallery_query_tile(17) == 128


def test_gallery_check_refusals(pkg):
    b, L = pkg.binding, pkg.lib()
    cfg = pkg.preset("vit_b_16")
    no_depth, wide, odd = (pkg.preset("vit_b_16") for _ in range(3))
    no_depth.depth, wide.embed_dim, odd.embed_dim = 0, 2052, 770

    def rc(cfg_=cfg, **kw):
        cs = spec_c(b, **kw).c_struct()
        return L.vit_gallery_check(C.byref(cfg_), C.byref(cs), None)

    def raw(**fields):
        cs = spec_c(b).c_struct()
        for name, v in fields.items():
            setattr(cs, name, v)
        return L.vit_gallery_check(C.byref(cfg), C.byref(cs), None)

    assert rc() == 0
    bad = [lambda: raw(source=2), lambda: raw(source=-1), lambda: rc(tap=12), lambda: rc(tap=-13), lambda: raw(dtype=2),
           lambda: rc(k=0), lambda: rc(k=33), lambda: rc(k=6, n_rows=5), lambda: rc(n_rows=2 ** 31), lambda: rc(n_rows=0),
           lambda: rc(row_stride=764), lambda: rc(row_stride=770), lambda: rc(dtype="bf16", row_stride=772),
           lambda: rc(no_depth), lambda: rc(wide, row_stride=2052), lambda: rc(odd, row_stride=772),
           lambda: L.vit_gallery_check(None, C.byref(spec_c(b).c_struct()), None), lambda: L.vit_gallery_check(C.byref(cfg), None, None)]
    for i, f in enumerate(bad):
        L.vh_set_error(1, b"stale")
        assert f() == 1, i
        msg = L.vh_last_error().decode()
        assert msg.startswith("vit_gallery_check: ") and len(msg) > len("vit_gallery_check: "), (i, msg)
    with pytest.raises(b.VitHipError, match="k must be"):
        b.gallery_check(cfg, spec_c(b, k=40))
    # arming without a context is refused on the host, before any device call
    assert L.vit_hip_set_gallery(None, None, None) == 1 and L.vit_hip_set_gallery_host(None, None, None) == 1
    assert "NULL context" in L.vh_last_error().decode()
    cs, bufs = spec_c(b).c_struct(), b.GalleryBuffers(None, None)
    assert L.vit_hip_set_gallery(None, C.byref(cs), C.byref(bufs)) == 1


def test_struct_mirror_matches_the_header(pkg):
    """vit_gallery_spec: four ints, k, dtype, two longs, a pointer -- 48 bytes on LP64, the longs 8-aligned"""
    b = pkg.binding
    assert C.sizeof(b.GallerySpecC) == 48 and b.GallerySpecC.n_rows.offset == 24 and b.GallerySpecC.d_rows.offset == 40
    assert C.sizeof(b.GalleryBuffers) == 16
