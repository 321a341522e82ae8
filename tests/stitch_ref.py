"""Reference for the dense stitch (vh_launch_dense_stitch, csrc/dense_stitch.hip; vit_hip_segment_frame_u8): the definition of
include/kernelHandler.h evaluated in float64 (`stitch64`), the error bound stated there (`bound`) and `check`, which judges a
label map without deciding near-ties as dense_ref.check does; the header's fp32 expressions restated in NumPy (`stitch32`) for
data on which every operation is exact (integer logits, boxes of integer corners whose sides are the grid times a power of
two: the ratios and all weights are dyadic); and a per-pixel statement of the block index (`index_ref`)."""
import numpy as np

import dense_ref as dr

U = dr.U
NAN_BITS = dr.NAN_BITS
F32 = np.float32


def boxes4(boxes):
    return np.asarray(boxes, dtype=F32).reshape(-1, 4)


def span(lo, hi, size):
    """the pixels of one axis whose centre (float)X + 0.5f lies in [lo, hi), by the kernel's fp32 comparisons: (first, end)"""
    c = np.arange(size, dtype=F32) + F32(0.5)
    inside = np.nonzero((F32(lo) <= c) & (c < F32(hi)))[0]
    return (int(inside[0]), int(inside[-1]) + 1) if inside.size else (0, 0)


def cover_count(boxes, H, W):
    """[H][W] int: how many boxes cover each pixel"""
    n = np.zeros((H, W), dtype=np.int64)
    for l, t, r, b in boxes4(boxes):
        (x0, x1), (y0, y1) = span(l, r, W), span(t, b, H)
        n[y0:y1, x0:x1] += 1
    return n


def index_ref(H, W, block, boxes):
    """(offsets, ids) as plain lists: block by block, row-major, every window that covers a pixel centre of the block, found
    pixel by pixel"""
    B = boxes4(boxes)
    cx, cy = np.arange(W, dtype=F32) + F32(0.5), np.arange(H, dtype=F32) + F32(0.5)
    offsets, ids = [0], []
    for by in range(0, H, block):
        for bx in range(0, W, block):
            xs, ys = cx[bx:bx + block], cy[by:by + block]
            for w, (l, t, r, b) in enumerate(B):
                if ((l <= xs) & (xs < r)).any() and ((t <= ys) & (ys < b)).any():
                    ids.append(w)
            offsets.append(len(ids))
    return offsets, ids


# ---- float64 ----------------------------------------------------------------------------------------------------------

def axis64(centres, lo, hi, G):
    """(r0, r1, w) of the pixel centres of one axis in a window side [lo, hi) over G patches, float64"""
    s = np.maximum(0.0, (centres - float(lo)) * (G / (float(hi) - float(lo))) - 0.5)
    r0 = np.minimum(np.floor(s).astype(np.int64), G - 1)
    return r0, np.minimum(r0 + 1, G - 1), s - r0


def windows64(L, grid, boxes, H, W):
    """for every window: (y0, y1, x0, x1, v [y1 - y0][x1 - x0][C] float64, r0 [rows], c0 [columns]) on its covered pixels"""
    GH, GW = grid
    n, P, C = L.shape
    Lg = np.asarray(L, np.float64).reshape(n, GH, GW, C)
    for w, (l, t, r, b) in enumerate(boxes4(boxes)):
        (x0, x1), (y0, y1) = span(l, r, W), span(t, b, H)
        r0, r1, wy = axis64(np.arange(y0, y1) + 0.5, t, b, GH)
        c0, c1, wx = axis64(np.arange(x0, x1) + 0.5, l, r, GW)
        g = Lg[w]
        wx_, wy_ = wx[None, :, None], wy[:, None, None]
        top = (1 - wx_) * g[r0][:, c0] + wx_ * g[r0][:, c1]
        bot = (1 - wx_) * g[r1][:, c0] + wx_ * g[r1][:, c1]
        yield y0, y1, x0, x1, (1 - wy_) * top + wy_ * bot, r0, c0


def stitch64(L, grid, boxes, H, W):
    """L [n][GH * GW][C] (fp32 values), boxes [n][4] -> (m [H][W][C] float64, NaN where nothing covers; count [H][W])"""
    C = L.shape[2]
    acc, cnt = np.zeros((H, W, C)), np.zeros((H, W), dtype=np.int64)
    for y0, y1, x0, x1, v, _, _ in windows64(L, grid, boxes, H, W):
        acc[y0:y1, x0:x1] += v
        cnt[y0:y1, x0:x1] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        return acc / cnt[..., None], cnt


def k_of(grid):
    return 8 * (grid[0] + grid[1]) + 16


def blend_term(count):
    """A of the header: (count + 1)(1 + 2 count u) u"""
    count = np.asarray(count, np.float64)
    return (count + 1) * (1 + 2 * count * U) * U


def bound(L, grid, boxes, H, W, corner=None):
    """[H][W][C]: (1 + A) max_w B_w + A max_w |v64_w|, B_w = k'(GH, GW) u M_w (+ the largest of the four corners' `corner`
    [n][P][C], the logits launcher's own term, when the logits come from it)"""
    GH, GW = grid
    n, P, C = L.shape
    M = np.abs(np.asarray(L, np.float64)).reshape(n, GH, GW, C)
    wide = np.pad(M, ((0, 0), (1, 2), (1, 2), (0, 0)))
    Mw = np.maximum.reduce([wide[:, dy:dy + GH, dx:dx + GW] for dy in range(4) for dx in range(4)])
    Bmax, Vmax, cnt = np.zeros((H, W, C)), np.zeros((H, W, C)), np.zeros((H, W), dtype=np.int64)
    cg = None if corner is None else np.asarray(corner, np.float64).reshape(n, GH, GW, C)
    for w, (y0, y1, x0, x1, v, r0, c0) in enumerate(windows64(L, grid, boxes, H, W)):
        B = k_of(grid) * U * Mw[w][r0][:, c0]
        if cg is not None:
            r1, c1 = np.minimum(r0 + 1, GH - 1), np.minimum(c0 + 1, GW - 1)
            B = B + np.maximum.reduce([cg[w][a][:, b] for a in (r0, r1) for b in (c0, c1)])
        Bmax[y0:y1, x0:x1] = np.maximum(Bmax[y0:y1, x0:x1], B)
        Vmax[y0:y1, x0:x1] = np.maximum(Vmax[y0:y1, x0:x1], np.abs(v))
        cnt[y0:y1, x0:x1] += 1
    A = blend_term(cnt)[..., None]
    return (1 + A) * Bmax + A * Vmax


def check(L, grid, boxes, H, W, fill, labels, scores=None, cover=None, corner=None):
    """Asserts for EVERY covered pixel: the label l is in range; |score - m64[l]| <= bound[l]; m64[c] - bound[c] <= m64[l] +
    bound[l] for every c; for every other pixel the fill label, the NaN score and cover 0; cover = min(count, 255).  Finite
    data.  Returns (the worst |error| / bound, the share of covered pixels that admit more than one label)."""
    C = L.shape[2]
    ref, cnt = stitch64(L, grid, boxes, H, W)
    bnd = bound(L, grid, boxes, H, W, corner)
    on = cnt > 0
    lab = np.asarray(labels).astype(np.int64)
    assert lab.shape == (H, W)
    assert (lab[~on] == fill).all()
    if cover is not None:
        assert np.array_equal(np.asarray(cover), np.minimum(cnt, 255).astype(np.uint8))
    assert ((lab[on] >= 0) & (lab[on] < C)).all()
    ref, bnd, lab_on = ref[on], bnd[on], lab[on]
    ok = dr.admissible(ref, bnd)
    mine = np.take_along_axis(ok, lab_on[:, None], axis=-1)[:, 0]
    assert mine.all(), f"{int((~mine).sum())} labels are beaten beyond both bounds"
    worst = 0.0
    if scores is not None:
        sc = np.asarray(scores, F32)
        assert (np.ascontiguousarray(sc[~on]).view(np.uint32) == NAN_BITS).all()
        err = np.abs(sc[on].astype(np.float64) - np.take_along_axis(ref, lab_on[:, None], axis=-1)[:, 0])
        bl = np.take_along_axis(bnd, lab_on[:, None], axis=-1)[:, 0]
        assert (err <= bl).all(), f"score error {err.max():.3e} beyond the bound {bl.flat[err.argmax()]:.3e}"
        worst = float((err / np.maximum(bl, 1e-300)).max())
    return worst, float((ok.sum(axis=-1) > 1).mean())


# ---- the header's fp32 expressions, for data on which they are exact ----------------------------------------------------

def axis32(centres, lo, hi, G):
    """(r0, r1, w, u) as the header's fp32 expressions give them: side, ratio and t rounded once each, the fma formed in
    float64 (exact for the dyadic ratios these tests use) and rounded once"""
    lo, hi = F32(lo), F32(hi)
    ratio = F32(G) / F32(hi - lo)
    t = (np.asarray(centres, F32) - lo).astype(F32)
    s = np.maximum((t.astype(np.float64) * np.float64(ratio) - 0.5).astype(F32), F32(0.0))
    r0 = np.minimum(s.astype(np.int64), G - 1)
    w = (s - r0.astype(F32)).astype(F32)
    return r0, np.minimum(r0 + 1, G - 1), w, (F32(1.0) - w).astype(F32)


def stitch32(L, grid, boxes, H, W, fill):
    """-> (labels uint8 [H][W], score bits uint32 [H][W], cover uint8 [H][W]): the header's expressions, every fmaf formed in
    float64 and rounded to fp32, the blend's adds and its division in fp32"""
    GH, GW = grid
    n, P, C = L.shape
    Lg = np.asarray(L, F32).reshape(n, GH, GW, C)
    acc, cnt = np.zeros((H, W, C), dtype=F32), np.zeros((H, W), dtype=np.int64)
    f64 = lambda a: np.asarray(a, np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for w, (l, t, r, b) in enumerate(boxes4(boxes)):
            (x0, x1), (y0, y1) = span(l, r, W), span(t, b, H)
            r0, r1, wy, uy = axis32(np.arange(y0, y1, dtype=F32) + F32(0.5), t, b, GH)
            c0, c1, wx, ux = axis32(np.arange(x0, x1, dtype=F32) + F32(0.5), l, r, GW)
            g = Lg[w]
            wx, ux, wy, uy = wx[None, :, None], ux[None, :, None], wy[:, None, None], uy[:, None, None]
            top = (f64(wx) * f64(g[r0][:, c1]) + f64(ux * g[r0][:, c0])).astype(F32)
            bot = (f64(wx) * f64(g[r1][:, c1]) + f64(ux * g[r1][:, c0])).astype(F32)
            v = (f64(wy) * f64(bot) + f64(uy * top)).astype(F32)
            first = (cnt[y0:y1, x0:x1] == 0)[..., None]
            acc[y0:y1, x0:x1] = np.where(first, v, acc[y0:y1, x0:x1] + v)     # the first value replaces the zero: -0 stays -0
            cnt[y0:y1, x0:x1] += 1
        m = (acc / np.maximum(cnt, 1).astype(F32)[..., None]).astype(F32)
    lab = dr.rank_first(m)
    sc = np.ascontiguousarray(np.take_along_axis(m, lab[..., None], axis=-1)[..., 0])
    bits = sc.view(np.uint32).copy()
    bits[np.isnan(sc)] = NAN_BITS
    lab[cnt == 0], bits[cnt == 0] = fill, NAN_BITS
    return lab.astype(np.uint8), bits, np.minimum(cnt, 255).astype(np.uint8)


# ---- shapes the tests share ---------------------------------------------------------------------------------------------

def tiles(H, W, tile, stride):
    """vit_tile_boxes' rule: tile x tile boxes every `stride` px, the last row and column flush to the far edges"""
    def starts(size):
        s = list(range(0, size - tile + 1, stride))
        return s if s[-1] == size - tile else s + [size - tile]
    return [(float(x), float(y), float(x + tile), float(y + tile)) for y in starts(H) for x in starts(W)]


# (H, W, tile, stride, grid, C, seed): the float cases.  tests/test_stitch_host.py asserts that at most 1 % of their pixels admit
# more than one label under the float64 definition alone and twice the bound, so that `check` on a kernel's output is not
# vacuous.  The last is one window.
FLOAT_CASES = [
    (96, 80, 48, 32, (3, 3), 21, 1),
    (70, 100, 32, 20, (4, 4), 150, 2),
    (224, 300, 112, 80, (14, 14), 17, 3),
    (50, 50, 50, 50, (5, 5), 33, 4),
]


def float_boxes(case):
    """the tiling of a float case with its corners moved inwards by quarter, half, three-eighth and eighth pixels and every
    other box cut 3 px lower: fractional corners, boxes that are not square over a square grid, some edge pixels uncovered"""
    H, W, tile, stride = case[:4]
    return [(l + 0.25 * (i % 4), t + 0.5 * (i % 3), r - 0.375 * (i % 2), b - 0.125 * (i % 5) - 3.0 * (i % 2))
            for i, (l, t, r, b) in enumerate(tiles(H, W, tile, stride))]


E_FLOAT = 64


def float_case(n, grid, C, seed):
    """tokens, head and bias of n windows, as dense_ref.float_case makes them"""
    return dr.float_case(n, E_FLOAT, C, grid, (1, 1), True, seed)
