"""The numpy float64 statement of vh_launch_resample_pos_embed (include/kernelHandler.h): per axis a table of clamped tap
indices and a table of weights, then v = sum_j wy_j * (sum_i wx_i * p[iy_j][ix_i]) with i and j ascending, horizontal first.
What torch.nn.functional.interpolate(mode="bicubic" | "bilinear", antialias=False) computes on float64 tensors
(tests/test_pos_resample_host.py holds it to that)."""
import numpy as np

BICUBIC, BILINEAR = 0, 1
MODES = {"bicubic": BICUBIC, "bilinear": BILINEAR}
A = -0.75   # the Keys kernel's constant


def _c1(x):
    return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0


def _c2(x):
    return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A


def axis_tables(n_in, n_out, mode, align_corners):
    """-> (idx int64 [n_out][taps], w float64 [n_out][taps]): taps 4 (bicubic) or 2 (bilinear)"""
    mode = MODES.get(mode, mode)
    o = np.arange(n_out, dtype=np.float64)
    if align_corners:
        scale = np.float64(n_in - 1) / np.float64(n_out - 1) if n_out > 1 else np.float64(0.0)
        s = o * scale
    else:
        scale = np.float64(n_in) / np.float64(n_out)
        s = (o + 0.5) * scale - 0.5
    if mode == BICUBIC:
        f = np.floor(s)
        t = s - f
        i0 = f.astype(np.int64)
        idx = np.clip(i0[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1)
        w = np.stack([_c2(t + 1.0), _c1(t), _c1(1.0 - t), _c2(2.0 - t)], axis=1)
    elif mode == BILINEAR:
        if not align_corners:
            s = np.maximum(s, 0.0)
        i0 = np.minimum(s.astype(np.int64), n_in - 1)
        i1 = np.minimum(i0 + 1, n_in - 1)
        lam = s - i0.astype(np.float64)
        idx = np.stack([i0, i1], axis=1)
        w = np.stack([1.0 - lam, lam], axis=1)
    else:
        raise ValueError(f"unknown mode {mode}")
    return idx, w


def resample_grid(grid, out_hw, mode="bicubic", align_corners=False):
    """grid [in_h][in_w][E] -> float64 [out_h][out_w][E]; equal grids give the input's own values"""
    grid = np.asarray(grid)
    in_h, in_w = grid.shape[:2]
    out_h, out_w = out_hw
    g = grid.astype(np.float64)
    if (in_h, in_w) == (out_h, out_w):
        return g.copy()
    iy, wy = axis_tables(in_h, out_h, mode, align_corners)
    ix, wx = axis_tables(in_w, out_w, mode, align_corners)
    h = np.zeros((in_h, out_w, g.shape[2]))
    for i in range(ix.shape[1]):                       # horizontal first, taps ascending
        h += wx[None, :, i, None] * g[:, ix[:, i], :]
    v = np.zeros((out_h, out_w, g.shape[2]))
    for j in range(iy.shape[1]):
        v += wy[:, j, None, None] * h[iy[:, j], :, :]
    return v


def resample_pos_embed(pos, prefix, in_hw, out_hw, mode="bicubic", align_corners=False):
    """pos [prefix + in_h * in_w][E] -> float64 [prefix + out_h * out_w][E], the prefix rows unchanged"""
    pos = np.asarray(pos)
    in_h, in_w = in_hw
    assert pos.shape[0] == prefix + in_h * in_w
    grid = resample_grid(pos[prefix:].reshape(in_h, in_w, -1), out_hw, mode, align_corners)
    return np.concatenate([pos[:prefix].astype(np.float64), grid.reshape(out_hw[0] * out_hw[1], -1)])


def bound(want, source_grid):
    """the launcher's error bound per element: 2^-24 |want| + 2^-40 max|p|"""
    m = float(np.abs(np.asarray(source_grid, dtype=np.float64)).max()) if np.asarray(source_grid).size else 0.0
    return 2.0 ** -24 * np.abs(want) + 2.0 ** -40 * m
