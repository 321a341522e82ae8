"""The class-token attention maps as include/ViT_opencl.h defines them, in NumPy float64, and the host side of the two
planes layouts a Q|K|V buffer can have (include/kernelHandler.h, vh_launch_cls_attention).  Nothing here calls that kernel.

    s[t]           = (1/sqrt(D)) * sum_d Q[i*T + 0][h*D + d] * K[i*T + t][h*D + d]
    heads[i][h][t] = exp(s[t] - max_t s) / sum_t exp(s[t] - max_t s)
    mean [i][t]    = (sum over h of heads[i][h][t]) / H
"""
import ctypes as C

import numpy as np

ROWS_F32, PLANES3, PLANES_F16 = 0, 1, 2


def cls_attention(qkv, n, T, H):
    """qkv fp32 [n*T][3E] -> heads [n][H][T], mean [n][T], float64"""
    qkv = np.asarray(qkv)
    E = qkv.shape[1] // 3
    D = E // H
    x = qkv.astype(np.float64).reshape(n, T, 3, H, D)
    q, k = x[:, 0, 0], x[:, :, 1]                              # [n][H][D], [n][T][H][D]
    s = np.einsum("nhd,nthd->nht", q, k) / np.sqrt(D)
    s -= s.max(axis=2, keepdims=True)
    p = np.exp(s)
    heads = p / p.sum(axis=2, keepdims=True)
    return heads, heads.sum(axis=1) / H


def score_magnitude(qkv, n, T, H):
    """S [n][H] = max_t sum_d |q_d k_d| / sqrt(D), float64: what the error of an fp32 dot product scales with"""
    qkv = np.asarray(qkv)
    E = qkv.shape[1] // 3
    D = E // H
    x = np.abs(qkv.astype(np.float64)).reshape(n, T, 3, H, D)
    return (np.einsum("nhd,nthd->nht", x[:, 0, 0], x[:, :, 1]) / np.sqrt(D)).max(axis=2)


def bound(qkv, n, T, H):
    """[n][H][1]: |p - ref| <= bound * ref + 1e-30.  (D + 1) 2^-24 S is the worst error of an fp32 dot product in any
    order; twice that for s - max, doubled again for the exponential's argument rounding; T + 64 covers the row sum and
    the division; the floor covers flushed denormals."""
    D = np.asarray(qkv).shape[1] // 3 // H
    return ((4 * (D + 2) * score_magnitude(qkv, n, T, H) + T + 64) * 2.0 ** -24)[:, :, None]


# ---- one-part fp16 planes [cols/32][rows][32] ----------------------------------------------------------------------------

def encode_f16(rows):
    R, N = rows.shape
    return np.ascontiguousarray(rows.astype(np.float16).reshape(R, N // 32, 32).transpose(1, 0, 2))


def decode_f16(planes):
    c, R, _ = planes.shape
    return np.ascontiguousarray(planes.astype(np.float32).transpose(1, 0, 2).reshape(R, c * 32))


# ---- exact three-part bf16 planes [cols/32][3][rows][32], value = (p0 + p1) + p2 ------------------------------------------

def _bf16_rne(x):
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _bf16_val(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def encode_planes3(rows):
    """a host split (round to nearest even, three times); the library's own is read back by split3_on_device"""
    R, N = rows.shape
    p0 = _bf16_rne(rows)
    r1 = (rows - _bf16_val(p0)).astype(np.float32)
    p1 = _bf16_rne(r1)
    p2 = _bf16_rne((r1 - _bf16_val(p1)).astype(np.float32))
    st = np.stack([p.reshape(R, N // 32, 32) for p in (p0, p1, p2)])   # [3][R][N/32][32]
    return np.ascontiguousarray(st.transpose(2, 0, 1, 3))


def decode_planes3(planes):
    """uint16 [cols/32][3][rows][32] -> fp32 [rows][cols]"""
    c, _, R, _ = planes.shape
    v = _bf16_val(planes)
    return np.ascontiguousarray(((v[:, 0] + v[:, 1]) + v[:, 2]).transpose(1, 0, 2).reshape(R, c * 32))


def split3_on_device(pkg, rows):
    """-> (device buffer of the planes vh_launch_split3_rows writes for fp32 `rows`, the same planes as uint16)"""
    L = pkg.lib()
    R, N = rows.shape
    d_in = pkg.DeviceBuffer.from_numpy(rows)
    d_pl = pkg.DeviceBuffer(R * N * 3, dtype=np.uint16)
    assert L.vh_launch_split3_rows(None, d_in.ptr, d_pl.ptr, R, N) == 0, L.vh_last_error().decode()
    assert L.vh_device_sync() == 0, L.vh_last_error().decode()
    return d_pl, d_pl.to_numpy((N // 32, 3, R, 32))


def upload(pkg, a):
    """any array's bytes into a device buffer"""
    a = np.ascontiguousarray(a)
    d = pkg.DeviceBuffer((a.nbytes + 3) // 4)
    assert pkg.lib().vh_h2d(d.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes, None) == 0
    assert pkg.lib().vh_device_sync() == 0
    return d
