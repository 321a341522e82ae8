"""Reference for the soft stitch (vh_launch_dense_stitch_soft, csrc/dense_stitch_soft.hip; vit_hip_segment_frame_soft_u8): the
stitch's blended means in the header's fp32 expressions (`means32`, tests/stitch_ref.py::stitch32's blend restated, which
returns labels only), the soft maps of tests/dense_soft_ref.py on them in float64 under the sharp bounds (`check_sharp`: the
means are known to the bit), and on the all-float64 blend of tests/stitch_ref.py::stitch64 under the combined bounds
(`check_combined`: the means are known to within the stitch's bound).  Every pixel is judged: a pixel that no window covers,
or whose means hold a NaN or have an infinite maximum, must be the marker in every map."""
import numpy as np

import dense_soft_ref as ds
import stitch_ref as sr

F32 = np.float32
NAN_BITS = ds.NAN_BITS
NAMES = ds.NAMES


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def means32(L, grid, boxes, H, W):
    """-> (m [H][W][C] fp32, count [H][W]): the header's expressions, every fmaf formed in float64 and rounded to fp32, the
    blend's adds in ascending window index with the first value replacing the zero, its one division in fp32.  The kernel's
    bits wherever products and sums are exact (integer logits, dyadic ratios); m is 0 where nothing covers"""
    GH, GW = grid
    n, P, C = L.shape
    Lg = np.asarray(L, F32).reshape(n, GH, GW, C)
    acc, cnt = np.zeros((H, W, C), dtype=F32), np.zeros((H, W), dtype=np.int64)
    f64 = lambda a: np.asarray(a, np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for w, (l, t, r, b) in enumerate(sr.boxes4(boxes)):
            (x0, x1), (y0, y1) = sr.span(l, r, W), sr.span(t, b, H)
            r0, r1, wy, uy = sr.axis32(np.arange(y0, y1, dtype=F32) + F32(0.5), t, b, GH)
            c0, c1, wx, ux = sr.axis32(np.arange(x0, x1, dtype=F32) + F32(0.5), l, r, GW)
            g = Lg[w]
            wx, ux, wy, uy = wx[None, :, None], ux[None, :, None], wy[:, None, None], uy[:, None, None]
            top = (f64(wx) * f64(g[r0][:, c1]) + f64(ux * g[r0][:, c0])).astype(F32)
            bot = (f64(wx) * f64(g[r1][:, c1]) + f64(ux * g[r1][:, c0])).astype(F32)
            v = (f64(wy) * f64(bot) + f64(uy * top)).astype(F32)
            first = (cnt[y0:y1, x0:x1] == 0)[..., None]
            acc[y0:y1, x0:x1] = np.where(first, v, acc[y0:y1, x0:x1] + v)     # the first value replaces the zero: -0 stays -0
            cnt[y0:y1, x0:x1] += 1
        m = (acc / np.maximum(cnt, 1).astype(F32)[..., None]).astype(F32)
    return m, cnt


def footprint(box, grid, H, W, patch):
    """[H][W] bool: the pixels that window `box` covers and whose four corners in it include patch (row, column) -- whatever
    the weights: a weight of 0 on a NaN is a NaN"""
    l, t, r, b = sr.boxes4([box])[0]
    (x0, x1), (y0, y1) = sr.span(l, r, W), sr.span(t, b, H)
    r0, r1, _, _ = sr.axis32(np.arange(y0, y1, dtype=F32) + F32(0.5), t, b, grid[0])
    c0, c1, _, _ = sr.axis32(np.arange(x0, x1, dtype=F32) + F32(0.5), l, r, grid[1])
    hit = np.zeros((H, W), dtype=bool)
    hit[y0:y1, x0:x1] = (((r0 == patch[0]) | (r1 == patch[0]))[:, None]) & (((c0 == patch[1]) | (c1 == patch[1]))[None, :])
    return hit


def judge(got, refs, bounds, defined, what):
    """got: {map name: [H][W] fp32}.  Every pixel outside `defined` is the marker, every pixel inside it a number within its
    bound -> {name: worst |error| / bound}"""
    worst = {}
    for name, g in got.items():
        g = np.asarray(g, F32)
        assert g.shape == defined.shape, (what, name, g.shape)
        assert (bits(g)[~defined] == NAN_BITS).all(), f"{what}: {name} is not the marker on every undefined pixel"
        worst[name] = ds.worst_ratio(g[defined], refs[name][defined], bounds[name][defined]) if defined.any() else 0.0
        assert worst[name] <= 1.0, f"{what}: {name} is {worst[name]:.3f} of its bound"
    return worst


def check_sharp(L, grid, boxes, H, W, s, values, got, what=""):
    """Data on which means32 is exact: every pixel of the maps in `got` within vh_launch_dense_soft's bounds of the float64
    definition on the fp32 means; undefined pixels (uncovered, a NaN mean, an infinite maximum) the marker"""
    m, cnt = means32(L, grid, boxes, H, W)
    p, x, h, av = ds.soft64(m, s, values)
    defined = (cnt > 0) & ~np.isnan(p)
    bp, bx, bh = ds.sharp_bounds(L.shape[2], p, av)
    return judge(got, dict(prob=p, expect=x, entropy=h), dict(prob=bp, expect=bx, entropy=bh), defined, what)


def combined(L, grid, boxes, H, W, s, values, corner=None):
    """-> (refs, bounds, defined): the definition in float64 throughout on the logits L (finite), and the combined bounds: the
    sharp ones and exp(2 s delta) - 1 on every p_c, delta = the stitch's bound on a mean, its largest over the classes"""
    m64, cnt = sr.stitch64(L, grid, boxes, H, W)
    defined = cnt > 0
    delta = np.where(defined, sr.bound(L, grid, boxes, H, W, corner).max(axis=-1), 0.0)
    p, x, h, av = ds.soft64(np.where(defined[..., None], m64, 0.0), s, values)
    bp, bx, bh = ds.combined_bounds(L.shape[2], s, delta, p, av)
    return dict(prob=p, expect=x, entropy=h), dict(prob=bp, expect=bx, entropy=bh), defined


def check_combined(L, grid, boxes, H, W, s, values, got, corner=None, what=""):
    refs, bounds, defined = combined(L, grid, boxes, H, W, s, values, corner)
    return judge(got, refs, bounds, defined, what)


# ---- the cases the host and the GPU tests share -----------------------------------------------------------------------

# tests/test_gpu_stitch.py's table.  name -> (H, W, grid, boxes, fill): integer corners, sides = grid x 2^k, so ratios and
# weights are dyadic and means32 is the kernel's bits on integer logits
STRIP = [(0.0, 0.0, 32.0, 32.0), (16.0, 0.0, 48.0, 32.0), (32.0, 13.0, 64.0, 45.0), (8.0, 29.0, 24.0, 45.0)]
LAYOUTS = {
    "flush-70x45": (45, 70, (4, 4), sr.tiles(45, 70, 32, 16), 255),             # cover counts 1, 2, 3, 4, 6
    "40x40": (40, 40, (4, 4), sr.tiles(40, 40, 16, 8), 255),
    "strip-255": (45, 70, (4, 4), STRIP, 255),                                   # columns 64.. and more stay uncovered
    "strip-7": (45, 70, (2, 4), STRIP, 7),
    "stack-40": (45, 70, (4, 4), [(20.0, 8.0, 36.0, 24.0)] * 40, 255),           # 40 distinct-logit windows on one spot
}
OVERLAP_C = [2, 17, 33, 256]
SCALES = [0.37, 1.0, 3.0]


def integer_logits(n, grid, Cc, seed, special=True):
    """tests/test_gpu_stitch.py's recipe: integers in [-8, 8]; special: 3 % of the entries NaN, +inf, -inf or -0, one patch
    all NaN, and from C = 5 on whole columns of NaN, +inf and -inf, window 0 keeping a finite winner"""
    rng = np.random.default_rng(seed)
    P = grid[0] * grid[1]
    L = rng.integers(-8, 9, size=(n, P, Cc)).astype(F32)
    if not special:
        return L
    hit = rng.random(L.shape) < 0.03
    L[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0], F32), size=int(hit.sum()))
    L[n - 1, P // 2] = np.nan
    if Cc >= 5:
        L[:, :, 1], L[:, :, 2], L[:, :, Cc - 1] = np.nan, np.inf, -np.inf
        L[0, :, 2] = 8.0
    return L


def mild_logits(n, grid, Cc, seed):
    """integers in [-8, 8] with 1 % of the entries -inf or -0: most pixels stay defined, so the sharp bounds are exercised"""
    rng = np.random.default_rng(seed)
    L = rng.integers(-8, 9, size=(n, grid[0] * grid[1], Cc)).astype(F32)
    hit = rng.random(L.shape) < 0.01
    L[hit] = rng.choice(np.array([-np.inf, -0.0], F32), size=int(hit.sum()))
    return L
