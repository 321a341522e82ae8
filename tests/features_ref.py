"""NumPy statement of the feature definitions (include/ViT_opencl.h, vit_feature_spec), given rows that are already
normalised (or deliberately not): the mean over the patch rows and the L2 norm in float64, bf16 as round-to-nearest-even
by bit arithmetic, NLC -> NCHW as a transposition.  Nothing here calls the library."""
import numpy as np


def bf16_bits(x: np.ndarray) -> np.ndarray:
    """float32 -> the uint16 bit patterns of bfloat16, round to nearest even (NaN stays NaN, quiet)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    rounded = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (u >> 16) | 0x40, rounded).astype(np.uint16)


def bf16_to_f32(bits: np.ndarray) -> np.ndarray:
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def l2_unit(v: np.ndarray) -> np.ndarray:
    """rows of v scaled to unit L2 norm in float64 (a zero row stays zero)"""
    v = np.asarray(v, dtype=np.float64)
    norm = np.sqrt((v * v).sum(axis=-1, keepdims=True))
    return np.where(norm > 0, v / np.where(norm > 0, norm, 1.0), 0.0)


def features(rows: np.ndarray, n: int, T: int, l2_normalize: bool):
    """rows [n*T][E] (token 0 of every image = class token) -> float64 (cls [n][E], pooled [n][E], tokens [n][T-1][E])"""
    r = np.asarray(rows, dtype=np.float64).reshape(n, T, -1)
    cls, tokens = r[:, 0], r[:, 1:]
    pooled = tokens.mean(axis=1) if T > 1 else np.zeros_like(cls)
    if l2_normalize:
        cls, pooled = l2_unit(cls), l2_unit(pooled)
    return cls, pooled, tokens


def nlc_to_nchw(tokens: np.ndarray) -> np.ndarray:
    """[..., T-1, E] -> [..., E, T-1] (the [E][g][g] map, flattened over g x g)"""
    return np.ascontiguousarray(np.swapaxes(tokens, -1, -2))


# ---- the readout launcher's dispatch and summation order, restated (csrc/features.hip) -------------------------------------

READOUT_ROWS = 32      # patch rows per workgroup of the rows kernel: 16 waves x 2 rows
READOUT_SLICE = 256    # columns per pass of the NCHW transposition


def readout_dispatch(n: int, T: int, E: int) -> dict:
    """Which instantiations and branches vh_launch_feature_readout takes for n images of T tokens of E values:
    NV (16-byte chunks per lane, the 3 / 4 / 5 / 8 ladder over ceil(E / 4 / 64)), FULL (E == 256 NV: no tail-lane guards in
    the rows kernel; the class and pool kernels have no FULL form), chunks (workgroups per image), ragged (the last one holds
    fewer than 32 rows), packed (bf16 NCHW stores two rows per dword, P even; one bf16 per store when P is odd), blocks
    (workgroups of the class and pool kernels, 4 images each), ragged_slice (the last NCHW slice holds fewer than 256 columns)."""
    P = T - 1
    nv = -(-(E // 4) // 64)
    NV = 3 if nv <= 3 else 4 if nv <= 4 else 5 if nv <= 5 else 8
    return dict(NV=NV, FULL=E == 256 * NV, chunks=-(-P // READOUT_ROWS), ragged=P % READOUT_ROWS != 0, packed=not (P & 1),
                blocks=-(-n // 4), ragged_slice=E % READOUT_SLICE != 0)


def pooled_stated_order(tokens: np.ndarray) -> np.ndarray:
    """float32 tokens [n][P][E] -> float32 [n][E]: the mean over the P rows in the order csrc/features.hip documents, every
    step a float32 operation: per workgroup of 32 rows, wave w holds row w and adds row w + 16 when there is one (a wave
    without a row holds +0), the waves are added 0..15, the workgroups' sums 0..chunks-1, then one division by float(P)."""
    tok = np.ascontiguousarray(tokens, dtype=np.float32)
    n, P, E = tok.shape
    total = None
    for p0 in range(0, P, READOUT_ROWS):
        v = min(READOUT_ROWS, P - p0)
        a = np.zeros((n, 16, E), dtype=np.float32)
        a[:, :min(v, 16)] = tok[:, p0:p0 + min(v, 16)]
        if v > 16:
            a[:, :v - 16] = a[:, :v - 16] + tok[:, p0 + 16:p0 + v]
        s = a[:, 0]
        for w in range(1, 16):
            s = s + a[:, w]
        total = s if total is None else total + s
    out = total / np.float32(P)
    assert out.dtype == np.float32
    return out
