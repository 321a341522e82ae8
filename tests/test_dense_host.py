"""Host side of the dense head (no GPU): the reference itself (tests/dense_ref.py: its upsampling against
torch.nn.functional.interpolate in float64, `check` on its own output and on what is wrong, the share of ambiguous pixels
of every float case), vit_dense_sizes' acceptances, sizes and refusals through the library, the NULL-context refusals of
both setters, and the ctypes mirror of the header's struct."""
import ctypes as C

import numpy as np
import pytest

import dense_ref as dr


@pytest.mark.parametrize("grid,out", [((14, 14), (224, 224)), ((3, 5), (37, 11)), ((24, 24), (10, 10)), ((1, 1), (8, 8)),
                                      ((5, 5), (7, 7)), ((7, 4), (1, 1))])
def test_upsampling_is_interpolate_bilinear(grid, out):
    import torch

    rng = np.random.default_rng(grid[0] * 100 + out[1])
    n, Cc = 2, 3
    L = rng.standard_normal((n, grid[0] * grid[1], Cc))
    got = dr.upsample64(L, grid, out)                                                     # [n][H][W][C]
    t = torch.from_numpy(L.reshape(n, grid[0], grid[1], Cc).transpose(0, 3, 1, 2).copy())  # NCHW, float64
    want = torch.nn.functional.interpolate(t, size=out, mode="bilinear", align_corners=False).numpy().transpose(0, 2, 3, 1)
    # to rounding: the header's derivation at float64's unit -- the two sides order the coordinate's operations differently
    # (2 G u each way, against slopes of at most 2 max |L|) and round three lerps each
    assert np.abs(got - want).max() <= dr.k_of(grid) * 2.0 ** -53 * np.abs(L).max()


def test_coordinates_fp32_against_float64():
    """the header's fp32 coordinate is within 2 G u of the float64 one (the bound's derivation), on every case's axes"""
    for G, out in [(16, 224), (3, 37), (5, 7), (24, 10), (14, 224), (37, 518), (64, 4096), (1, 9), (7, 1)]:
        r0, r1, w, u = dr.coords32(out, G)
        q0, q1, w64 = dr.coords64(out, G)
        assert np.abs((r0 + w.astype(np.float64)) - (q0 + w64)).max() <= 2 * G * dr.U, (G, out)
        assert (r0 >= 0).all() and (r1 <= G - 1).all() and (np.diff(r0) >= 0).all()


@pytest.fixture(scope="module")
def small():
    """a small case with its reference's own labels and scores (rounded to fp32)"""
    n, E, Cc, grid, out = 2, 32, 6, (4, 5), (19, 23)
    x, W, b = dr.float_case(n, E, Cc, grid, out, True, 11)
    ref = dr.upsample64(dr.logits64(x, W, b), grid, out)
    lab = ref.argmax(axis=-1)
    sc = np.take_along_axis(ref, lab[..., None], axis=-1)[..., 0].astype(np.float32)
    return x, W, b, grid, out, ref, lab.astype(np.uint8), sc


def test_check_accepts_the_reference(small):
    x, W, b, grid, out, ref, lab, sc = small
    worst, share = dr.check(x, W, b, grid, out, lab, sc)
    assert worst <= 1.0 / (32 + 8) + 1e-9 and share <= 0.01      # one rounding of the score against a bound of E + 8 of them
    assert dr.check(x, W, b, grid, out, lab)[0] == 0.0           # no scores: nothing to measure


def test_check_rejects_what_is_wrong(small):
    x, W, b, grid, out, ref, lab, sc = small
    bnd = dr.bound(x, W, b, grid, out)
    ok = dr.admissible(ref, bnd)
    # an unambiguous pixel: only its own label is admissible
    i, y, xx = (int(a[0]) for a in np.nonzero(ok.sum(axis=-1) == 1))
    flipped = lab.copy()
    flipped[i, y, xx] = (int(lab[i, y, xx]) + 1) % W.shape[0]
    with pytest.raises(AssertionError, match="beyond both bounds"):
        dr.check(x, W, b, grid, out, flipped, sc)
    off = sc.copy()
    off[i, y, xx] = np.float32(ref[i, y, xx, lab[i, y, xx]] + 2 * bnd[i, y, xx, lab[i, y, xx]])
    with pytest.raises(AssertionError, match="beyond the bound"):
        dr.check(x, W, b, grid, out, lab, off)
    ranged = lab.copy()
    ranged[0, 0, 0] = W.shape[0]
    with pytest.raises(AssertionError, match="out of range"):
        dr.check(x, W, b, grid, out, ranged, sc)


def test_rank_rule_on_special_values():
    v = np.array([[1.0, 2.0, 2.0], [-0.0, 0.0, -1.0], [np.nan, -np.inf, -np.inf], [np.nan, np.nan, np.nan], [np.nan, np.inf, 3.0],
                  [-np.inf, np.nan, -np.inf]], np.float32)
    assert dr.rank_first(v).tolist() == [1, 0, 1, 0, 1, 0]


def test_fp32_restatement_matches_float64_where_exact():
    """integer logits, out = 4 * grid: weights are multiples of 1/8, every operation exact"""
    rng = np.random.default_rng(5)
    L = rng.integers(-8, 9, size=(2, 15, 7)).astype(np.float32)
    lab, bits = dr.dense32(L, (3, 5), (12, 20))
    v = dr.upsample64(L.astype(np.float64), (3, 5), (12, 20))
    assert np.array_equal(lab, dr.rank_first(v))
    assert np.array_equal(bits.view(np.float32), v.max(axis=-1).astype(np.float32))


@pytest.mark.parametrize("case", dr.FLOAT_CASES, ids=lambda c: f"E{c[1]}-C{c[2]}-{c[3][0]}x{c[3][1]}-to-{c[4][0]}x{c[4][1]}")
def test_float_cases_are_not_vacuous(case):
    """Under the reference alone at most 1 % of a case's pixels admit more than one label: what keeps `check` on a
    kernel's output from being vacuous"""
    n, E, Cc, grid, out, bias, seed = case
    x, W, b = dr.float_case(*case)
    ref = dr.upsample64(dr.logits64(x, W, b), grid, out)
    share = float((dr.admissible(ref, dr.bound(x, W, b, grid, out)).sum(axis=-1) > 1).mean())
    print(f"{case[:5]}: {100 * share:.3f} % of the pixels admit more than one label")
    assert share <= 0.01


# ---- the library ----------------------------------------------------------------------------------------------------

def spec_c(b, **kw):
    args = dict(n_labels=21, out_h=0, out_w=0, tap=-1, final_norm=True, weight_stride=768, d_weight=None, d_bias=None)
    args.update(kw)
    return b.DenseSpec(**args)


def test_dense_sizes_accepts_and_sizes(pkg):
    b = pkg.binding
    cfg = pkg.preset("vit_b_16")
    P, E = 196, 768
    assert b.dense_sizes(cfg, spec_c(b)) == (224 * 224, 224 * 224, P * 21, P * (21 + E) * 4)
    assert b.dense_sizes(cfg, spec_c(b, final_norm=False, n_labels=150)) == (224 * 224, 224 * 224, P * 150, P * 150 * 4)
    assert b.dense_sizes(cfg, spec_c(b, out_h=37, out_w=1, n_labels=2, tap=-12, weight_stride=772))[:3] == (37, 37, P * 2)
    assert b.dense_sizes(cfg, spec_c(b, out_h=4096, out_w=4096, n_labels=256, tap=11))[0] == 4096 * 4096
    big = pkg.preset("vit_b_16_384")
    assert b.dense_sizes(big, spec_c(b))[:3] == (384 * 384, 384 * 384, 576 * 21)
    L = pkg.lib()
    cs = spec_c(b).c_struct()
    assert L.vit_dense_sizes(C.byref(cfg), C.byref(cs), None, None, None, None) == 0
    assert (b.DENSE_MAX_LABELS, b.DENSE_MAX_GRID, b.DENSE_TOKEN_TILE) == (256, 64, 128)


def test_dense_sizes_refusals(pkg):
    b, L = pkg.binding, pkg.lib()
    cfg = pkg.preset("vit_b_16")
    no_depth, wide, odd, fine, huge = (pkg.preset("vit_b_16") for _ in range(5))
    no_depth.depth, wide.embed_dim, odd.embed_dim = 0, 2052, 770
    fine.patch_size = 2                       # a 112 x 112 grid: beyond VH_DENSE_MAX_GRID
    huge.img_size, huge.patch_size = 8192, 512   # out_h = 0 would mean 8192 rows

    def rc(cfg_=cfg, **kw):
        cs = spec_c(b, **kw).c_struct()
        return L.vit_dense_sizes(C.byref(cfg_), C.byref(cs), None, None, None, None)

    assert rc() == 0
    bad = [(lambda: rc(tap=12), "tap"), (lambda: rc(tap=-13), "tap"), (lambda: rc(n_labels=1), "n_labels"),
           (lambda: rc(n_labels=257), "n_labels"), (lambda: rc(out_h=-1), "out_h"), (lambda: rc(out_w=4097), "out_h"),
           (lambda: rc(weight_stride=764), "weight_stride"), (lambda: rc(weight_stride=770), "weight_stride"),
           (lambda: rc(no_depth), "model config"), (lambda: rc(wide, weight_stride=2052), "embed_dim"),
           (lambda: rc(odd, weight_stride=772), "embed_dim"), (lambda: rc(fine), "grid"), (lambda: rc(huge), "out_h"),
           (lambda: L.vit_dense_sizes(None, C.byref(spec_c(b).c_struct()), None, None, None, None), "NULL"),
           (lambda: L.vit_dense_sizes(C.byref(cfg), None, None, None, None, None), "NULL")]
    for i, (f, word) in enumerate(bad):
        L.vh_set_error(1, b"stale")
        assert f() == 1, i
        msg = L.vh_last_error().decode()
        assert msg.startswith("vit_dense_sizes: ") and word in msg, (i, msg)
    with pytest.raises(b.VitHipError, match="n_labels must be"):
        b.dense_sizes(cfg, spec_c(b, n_labels=300))


def test_setters_refuse_a_null_context(pkg):
    b, L = pkg.binding, pkg.lib()
    for entry in (L.vit_hip_set_dense, L.vit_hip_set_dense_host):
        L.vh_set_error(1, b"stale")
        assert entry(None, None, None) == 1
        assert "NULL context" in L.vh_last_error().decode()
        cs, bufs = spec_c(b).c_struct(), b.DenseBuffers(None, None, None)
        assert entry(None, C.byref(cs), C.byref(bufs)) == 1


def test_struct_mirror_matches_the_header(pkg):
    """vit_dense_spec: five ints, a long, two pointers -- 48 bytes on LP64, the long 8-aligned behind 4 bytes of padding"""
    b = pkg.binding
    assert C.sizeof(b.DenseSpecC) == 48 and b.DenseSpecC.weight_stride.offset == 24 and b.DenseSpecC.d_weight.offset == 32
    assert b.DenseSpecC.d_bias.offset == 40 and C.sizeof(b.DenseBuffers) == 24
