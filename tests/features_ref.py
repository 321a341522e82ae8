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
