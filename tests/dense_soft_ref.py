"""Reference for the soft maps of the dense head (vh_launch_dense_soft, csrc/dense_soft.hip; vit_hip_set_dense_soft): the
definition of include/kernelHandler.h in float64, its three error bounds (`sharp`: the per-pixel values v are known to the
bit), the combined bounds for inputs whose v is known only to within the interpolation bound of tests/dense_ref.py, the
kernel's fp32 arithmetic restated in NumPy, and the cases the host and the GPU tests share.  Every pixel is judged."""
import numpy as np

import dense_ref as dr

U = dr.U
K = 32                       # the header's constant: |prob - prob64| <= (C + K) u prob64, ...
NAN_BITS = dr.NAN_BITS       # how an undefined pixel is written
NAMES = ("prob", "expect", "entropy")


def soft64(v, s, values=None):
    """v [...][C] (the fp32 values, or their float64 definition), s, values [C] or None -> (prob, expect, entropy, Σ p |values|)
    in float64, by the header's definition.  A pixel with a NaN v or an infinite maximum is NaN in all of them; a -inf under
    a finite maximum contributes nothing."""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        bad = np.isnan(v).any(axis=-1)
        m = np.where(np.isnan(v), -np.inf, v).max(axis=-1)
        bad |= np.isinf(m)
        z = np.float64(s) * (v - np.where(bad, 0.0, m)[..., None])
        z = np.where(bad[..., None], 0.0, z)
        e = np.exp(z)
        S = e.sum(axis=-1)
        p = e / S[..., None]
        prob = 1.0 / S
        ent = np.log(S) - (e * np.where(e > 0, z, 0.0)).sum(axis=-1) / S
        if values is None:
            exp_, absval = np.zeros_like(S), np.zeros_like(S)
        else:
            val = np.asarray(values, np.float64)
            exp_, absval = (p * val).sum(axis=-1), (p * np.abs(val)).sum(axis=-1)
    for a in (prob, exp_, ent):
        a[bad] = np.nan
    return prob, exp_, ent, absval


def sharp_bounds(C, prob64, absval64):
    """the header's bounds, per pixel: (prob, expect, entropy)"""
    return (C + K) * U * prob64, 2 * (C + K) * U * absval64, np.full_like(prob64, 2 * (C + K) * U * (1 + np.log(C)))


def combined_bounds(C, s, delta, prob64, absval64):
    """v known to within delta (per pixel, the largest over the classes): every ln p_c moves by at most 2 eta, eta = s delta,
    because softmax is invariant under a shift of all v"""
    g = np.expm1(2 * np.float64(s) * delta)
    bp, be, bh = sharp_bounds(C, prob64, absval64)
    return g * prob64 + bp, g * absval64 + be, g * (1 + np.log(C)) + bh


def interp_bound(L, grid, out):
    """[n][out_h][out_w]: the interpolation term of dense_ref.bound, k(GH, GW) u M, maximised over the classes -- the whole
    bound on v where the patch logits L [n][GH * GW][C] are given exactly (uploaded, not computed)"""
    n, P, C = L.shape
    GH, GW = grid
    M = np.abs(np.asarray(L, np.float64)).reshape(n, GH, GW, C)
    wide = np.pad(M, ((0, 0), (1, 2), (1, 2), (0, 0)))
    Mw = np.maximum.reduce([wide[:, dy:dy + GH, dx:dx + GW] for dy in range(4) for dx in range(4)])
    r0, c0 = dr.coords64(out[0], GH)[0], dr.coords64(out[1], GW)[0]
    return dr.k_of(grid) * U * Mw[:, r0][:, :, c0].max(axis=-1)


def v32(L, grid, out):
    """L [n][GH * GW][C] fp32 -> v [n][out_h][out_w][C] fp32 by dense_ref.dense32's expressions (every fmaf formed in float64
    and rounded once): the kernel's bits wherever products and sums are exact -- out == grid (all weights 0: v is the logit's
    own bits, whatever the floats) and integer logits under dyadic ratios"""
    n, P, C = L.shape
    Lg = np.asarray(L, np.float32).reshape(n, grid[0], grid[1], C)
    r0, r1, wy, uy = dr.coords32(out[0], grid[0])
    c0, c1, wx, ux = dr.coords32(out[1], grid[1])
    pick = lambda r, c: Lg[:, r][:, :, c]
    wx, ux, wy, uy = wx[None, None, :, None], ux[None, None, :, None], wy[None, :, None, None], uy[None, :, None, None]
    f64 = lambda a: np.asarray(a, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        top = (f64(wx) * f64(pick(r0, c1)) + f64(ux * pick(r0, c0))).astype(np.float32)
        bot = (f64(wx) * f64(pick(r1, c1)) + f64(ux * pick(r1, c0))).astype(np.float32)
        return (f64(wy) * f64(bot) + f64(uy * top)).astype(np.float32)


def soft32(v, s, values=None):
    """The kernel's arithmetic restated in fp32 NumPy on v [...][C] fp32: k2 = s * fl(log2 e), t = k2 (v - m), e = exp2(t) with
    denormals flushed, sequential sums over c with the products as fmas (formed in float64, rounded once), IEEE divisions,
    entropy = fl(ln 2) (log2 S - A / S).  Not the hardware's exp2 and log2 (1 ulp each; NumPy's are at least as good), so it
    reproduces the kernel to a few ulp, not to the bit: it is here to show the bounds are neither vacuous nor wrong before a
    GPU sees them.  -> (prob, expect, entropy) fp32, NaN as the kernel writes it"""
    f32 = np.float32
    v = np.asarray(v, f32)
    C = v.shape[-1]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        m = np.where(np.isnan(v), f32(-np.inf), v).max(axis=-1)
        k2 = f32(s) * f32(1.44269504088896340736)
        S = np.zeros(v.shape[:-1], f32)
        X, A = S.copy(), S.copy()
        fma = lambda a, b, c: (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(f32)
        for c in range(C):
            t = (k2 * (v[..., c] - m).astype(f32)).astype(f32)
            e = np.exp2(t).astype(f32)
            e = np.where(np.abs(e) < f32(2.0 ** -126), f32(0), e)
            S = (S + e).astype(f32)
            if values is not None:
                X = fma(e, f32(values[c]), X)
            tt = np.where(np.isnan(t), f32(0), np.maximum(t, f32(-3.4028234663852886e38)))
            A = (e.astype(np.float64) * tt.astype(np.float64) + A.astype(np.float64)).astype(f32)
        ok = S <= f32(3.4028234663852886e38)
        prob = (f32(1) / S).astype(f32)
        exp_ = (X / S).astype(f32)
        ent = (f32(0.69314718055994530942) * (np.log2(S).astype(f32) - (A / S).astype(f32)).astype(f32)).astype(f32)
    nan = np.array([NAN_BITS], np.uint32).view(f32)[0]
    return tuple(np.where(ok, a, nan).astype(f32) for a in (prob, exp_, ent))


def worst_ratio(got, ref, bnd):
    """max |got - ref| / bound over every pixel (a zero bound admits a zero error only)"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    assert np.isfinite(err).all(), "a pixel that is not a number"
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bnd > 0, err / bnd, np.where(err == 0, 0.0, np.inf))
    return float(q.max())


def check_maps(got, refs, bounds, what):
    """got, refs, bounds: dicts by map name (a subset of NAMES).  Every pixel of every map within its bound -> {name: worst
    |error| / bound}"""
    worst = {}
    for name, g in got.items():
        worst[name] = worst_ratio(g, refs[name], bounds[name])
        assert worst[name] <= 1.0, f"{what}: {name} is {worst[name]:.3f} of its bound"
    return worst


def check_sharp(v, s, values, got, what=""):
    """v [...][C] fp32, exact: every pixel of the maps in `got` within the header's bounds of the float64 definition on v"""
    C = v.shape[-1]
    p, x, h, av = soft64(v, s, values)
    bp, bx, bh = sharp_bounds(C, p, av)
    return check_maps(got, dict(prob=p, expect=x, entropy=h), dict(prob=bp, expect=bx, entropy=bh), what)


def check_combined(L, grid, out, s, values, got, what=""):
    """L [n][P][C] fp32 patch logits given exactly: every pixel of the maps in `got` within the combined bounds of the float64
    definition (coordinates, lerps and softmax in float64)"""
    C = L.shape[-1]
    p, x, h, av = soft64(dr.upsample64(np.asarray(L, np.float64), grid, out), s, values)
    bp, bx, bh = combined_bounds(C, s, interp_bound(L, grid, out), p, av)
    return check_maps(got, dict(prob=p, expect=x, entropy=h), dict(prob=bp, expect=bx, entropy=bh), what)


# ---- the cases --------------------------------------------------------------------------------------------------------
SHARP_GRIDS = [(8, 8), (3, 5)]
SHARP_C = [2, 5, 21, 150, 256]
SPREADS = [0.0, 1.0, 8.0, 60.0]          # 0: all classes equal (prob = 1 / C, entropy = ln C); 60: terms that underflow at s = 3
SCALES = [0.37, 1.0, 3.0]
DYADIC = [((4, 4), (16, 16)), ((2, 3), (16, 24))]


def values_for(C, seed=0):
    """[C] fp32 of mixed sign"""
    return (10.0 * np.random.default_rng(1000 + C + seed).standard_normal(C)).astype(np.float32)


def spread_logits(n, grid, C, spread, seed):
    """[n][GH * GW][C] fp32: any floats within `spread` of one another per patch, around offsets that differ per patch"""
    rng = np.random.default_rng(seed)
    P = grid[0] * grid[1]
    base = rng.uniform(-20.0, 20.0, size=(n, P, 1))
    return (base + spread * rng.random((n, P, C))).astype(np.float32)


def integer_logits(n, grid, C, seed):
    """[n][GH * GW][C] fp32 integers in +-512"""
    return np.random.default_rng(seed).integers(-512, 513, size=(n, grid[0] * grid[1], C)).astype(np.float32)


# (grid, out): the band and column edges.  Non-dyadic ratios, downsampling with empty bands, a non-square case, a band on each
# side of the 16-row register chunk (2 -> 30, 32, 34: bands of 15 / 16 / 17 rows at the edges), out_w under one wave and over
# one 256-column pass
EDGE_CASES = [((16, 16), (224, 224), 21), ((3, 3), (37, 37), 17), ((5, 5), (7, 7), 5), ((24, 24), (10, 10), 150), ((4, 7), (30, 45), 33),
              ((2, 2), (30, 30), 6), ((2, 2), (32, 32), 6), ((2, 2), (34, 34), 6),
              ((3, 4), (5, 1), 9), ((3, 4), (5, 63), 9), ((3, 4), (5, 257), 9), ((3, 7), (9, 300), 9)]
