"""Reference for the dense head (vh_launch_dense_logits, vh_launch_dense_labels, csrc/dense_head.hip; vit_hip_set_dense):
the definition of include/kernelHandler.h evaluated in float64, the error bound stated there, `check`, which judges a
label map WITHOUT deciding near-ties (a pixel whose two best classes lie within their bounds of each other admits both), the
fp32 expressions of the header restated in NumPy for data on which every operation is exact, and the float cases the host
and the GPU tests share."""
import numpy as np

U = 2.0 ** -24
NAN_BITS = 0x7FC00000    # how a NaN score is written


def coords64(out, G):
    """source cell and weight of every output index along one axis, float64: (r0, r1, w)"""
    s = np.maximum(0.0, (np.arange(out, dtype=np.float64) + 0.5) * G / out - 0.5)
    r0 = np.minimum(np.floor(s).astype(np.int64), G - 1)
    return r0, np.minimum(r0 + 1, G - 1), s - r0


def logits64(x, W, b=None):
    """x [n][P][E], W [C][E], b [C] or None (fp32 values) -> L [n][P][C], exact products summed in float64"""
    L = np.asarray(x, np.float64) @ np.asarray(W, np.float64).T
    return L if b is None else L + np.asarray(b, np.float64)


def absdot(x, W, b=None):
    """sum_d |x_d w_d| + |b|, [n][P][C]"""
    A = np.abs(np.asarray(x, np.float64)) @ np.abs(np.asarray(W, np.float64)).T
    return A if b is None else A + np.abs(np.asarray(b, np.float64))


def corners(Lg, grid, out):
    """Lg [n][GH][GW][C] -> the four corner arrays [n][out_h][out_w][C] (00, 01, 10, 11) and the weights wy [out_h], wx [out_w]"""
    r0, r1, wy = coords64(out[0], grid[0])
    c0, c1, wx = coords64(out[1], grid[1])
    pick = lambda r, c: Lg[:, r][:, :, c]
    return (pick(r0, c0), pick(r0, c1), pick(r1, c0), pick(r1, c1)), wy, wx


def upsample64(L, grid, out):
    """L [n][GH * GW][C] float64 -> v [n][out_h][out_w][C]: bilinear, half-pixel centres, edges clamped, horizontal first"""
    n, P, C = L.shape
    (a00, a01, a10, a11), wy, wx = corners(np.asarray(L, np.float64).reshape(n, grid[0], grid[1], C), grid, out)
    wx, wy = wx[None, None, :, None], wy[None, :, None, None]
    return (1 - wy) * ((1 - wx) * a00 + wx * a01) + wy * ((1 - wx) * a10 + wx * a11)


def k_of(grid):
    return 4 * (grid[0] + grid[1]) + 16


def bound(x, W, b, grid, out):
    """[n][out_h][out_w][C]: max over the four corners of (E + 8) u (sum |x w| + |b|)  +  k(GH, GW) u M, M the largest
    |L64| over patch rows r0 - 1 .. r0 + 2 and columns c0 - 1 .. c0 + 2 inside the grid"""
    x = np.asarray(x)
    n, P, E = x.shape
    GH, GW = grid
    C = np.asarray(W).shape[0]
    A = ((E + 8) * U * absdot(x, W, b)).reshape(n, GH, GW, C)
    first = np.maximum.reduce(corners(A, grid, out)[0])
    M = np.abs(logits64(x, W, b)).reshape(n, GH, GW, C)
    wide = np.pad(M, ((0, 0), (1, 2), (1, 2), (0, 0)))           # zeros outside the grid: |L| >= 0
    Mw = np.maximum.reduce([wide[:, dy:dy + GH, dx:dx + GW] for dy in range(4) for dx in range(4)])
    r0 = coords64(out[0], GH)[0]
    c0 = coords64(out[1], GW)[0]
    return first + k_of(grid) * U * Mw[:, r0][:, :, c0]


def rank_first(v):
    """v [...][C] -> the label vh_launch_topk's rule ranks first: the largest, equal values (-0 == +0) to the lowest c, NaN
    below -inf (all NaN: 0)"""
    v = np.asarray(v)
    nan = np.isnan(v)
    vv = np.where(nan, -np.inf, v)
    lab = vv.argmax(axis=-1)
    low = vv.max(axis=-1) == -np.inf                              # only -inf and NaN: the first that is a number
    lab[low] = (~nan[low]).argmax(axis=-1)
    return lab


def admissible(ref, bnd):
    """[...][C] bool: the labels `check` accepts -- no class is better by more than both bounds"""
    floor = (ref - bnd).max(axis=-1, keepdims=True)
    return ref + bnd >= floor


def check(x, W, b, grid, out, labels, scores=None):
    """Asserts for EVERY pixel: the label l is in range; |score - ref64[l]| <= bound[l] (when scores are given); ref64[c] -
    bound[c] <= ref64[l] + bound[l] for every c.  Finite data.  Returns (the worst |error| / bound, the share of pixels that
    admit more than one label)."""
    x = np.asarray(x, np.float32)
    n, P, E = x.shape
    C = np.asarray(W).shape[0]
    labels = np.asarray(labels)
    assert labels.shape == (n, out[0], out[1]), labels.shape
    ref = upsample64(logits64(x, W, b), grid, out)
    bnd = bound(x, W, b, grid, out)
    lab = labels.astype(np.int64)
    assert ((lab >= 0) & (lab < C)).all(), f"label out of range: {lab.max()} of {C}"
    ok = admissible(ref, bnd)
    mine = np.take_along_axis(ok, lab[..., None], axis=-1)[..., 0]
    if not mine.all():
        i, y, xx = (int(a[0]) for a in np.nonzero(~mine))
        l, best = lab[i, y, xx], int(ref[i, y, xx].argmax())
        raise AssertionError(f"image {i} pixel ({y}, {xx}): label {l} ({ref[i, y, xx, l]:.6g} +- {bnd[i, y, xx, l]:.2g}) is beaten by "
                             f"{best} ({ref[i, y, xx, best]:.6g} +- {bnd[i, y, xx, best]:.2g}) beyond both bounds")
    worst = 0.0
    if scores is not None:
        scores = np.asarray(scores, np.float32)
        assert scores.shape == labels.shape
        err = np.abs(scores.astype(np.float64) - np.take_along_axis(ref, lab[..., None], axis=-1)[..., 0])
        bl = np.take_along_axis(bnd, lab[..., None], axis=-1)[..., 0]
        assert (err <= bl).all(), f"score error {err.max():.3e} beyond the bound {bl.flat[err.argmax()]:.3e}"
        worst = float((err / np.maximum(bl, 1e-300)).max())
    return worst, float((ok.sum(axis=-1) > 1).mean())


# ---- the header's fp32 expressions, for data on which they are exact ------------------------------------------------

def coords32(out, G):
    """(r0, r1, w, u) of every output index as the header's fp32 expressions give them, bit for bit: the fma is formed in
    float64, where the product (12 x 24 bits) and the sum are exact, and rounded once"""
    ratio = np.float32(G) / np.float32(out)
    t = (np.arange(out, dtype=np.float32) + np.float32(0.5)).astype(np.float64)
    s = np.maximum((t * np.float64(ratio) - 0.5).astype(np.float32), np.float32(0.0))
    r0 = np.minimum(s.astype(np.int64), G - 1)
    w = (s - r0.astype(np.float32)).astype(np.float32)
    return r0, np.minimum(r0 + 1, G - 1), w, (np.float32(1.0) - w).astype(np.float32)


def dense32(L, grid, out):
    """L [n][GH * GW][C] fp32 -> (labels uint8 [n][out_h][out_w], score bits uint32): the header's expressions with every
    fmaf formed in float64 and rounded to fp32 -- the kernel's bits wherever products and sums are exact (integer logits
    under dyadic weights); infinities and NaNs propagate as in fp32"""
    n, P, C = L.shape
    Lg = np.asarray(L, np.float32).reshape(n, grid[0], grid[1], C)
    r0, r1, wy, uy = coords32(out[0], grid[0])
    c0, c1, wx, ux = coords32(out[1], grid[1])
    pick = lambda r, c: Lg[:, r][:, :, c]
    wx, ux, wy, uy = wx[None, None, :, None], ux[None, None, :, None], wy[None, :, None, None], uy[None, :, None, None]
    f64 = lambda a: np.asarray(a, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        top = (f64(wx) * f64(pick(r0, c1)) + f64(ux * pick(r0, c0))).astype(np.float32)
        bot = (f64(wx) * f64(pick(r1, c1)) + f64(ux * pick(r1, c0))).astype(np.float32)
        v = (f64(wy) * f64(bot) + f64(uy * top)).astype(np.float32)
    lab = rank_first(v)
    sc = np.ascontiguousarray(np.take_along_axis(v, lab[..., None], axis=-1)[..., 0])
    bits = sc.view(np.uint32).copy()
    bits[np.isnan(sc)] = NAN_BITS
    return lab.astype(np.uint8), bits


# ---- the float cases: (n, E, C, grid, out, bias, seed).  Gaussian tokens, W ~ N(0, 1 / E), bias ~ N(0, 0.01): shapes at
# which at most 1 % of the pixels admit more than one label under the reference alone (tests/test_dense_host.py asserts
# it), so that `check` on a kernel's output is not vacuous.  Among them the non-dyadic ratios 16 -> 224 (patch 14), 3 -> 37
# and 5 -> 7, the down-sampling 24 -> 10, a non-square grid and output, and ViT-B/16's own E = 768, 14 -> 224.
FLOAT_CASES = [
    (2, 64, 21, (16, 16), (224, 224), True, 1),
    (3, 60, 17, (3, 3), (37, 37), False, 2),
    (3, 64, 5, (5, 5), (7, 7), True, 3),
    (2, 64, 150, (24, 24), (10, 10), True, 4),
    (2, 128, 33, (4, 7), (30, 45), True, 5),
    (1, 768, 21, (14, 14), (224, 224), True, 6),
]


def float_case(n, E, C, grid, out, bias, seed):
    """-> x [n][P][E], W [C][E], b [C] or None, fp32"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, grid[0] * grid[1], E)).astype(np.float32)
    W = (rng.standard_normal((C, E)) / np.sqrt(E)).astype(np.float32)
    b = (0.1 * rng.standard_normal(C)).astype(np.float32) if bias else None
    return x, W, b
