"""NumPy reference of the top-k contract (include/ViT_opencl.h, vh_launch_topk): rank by logit, descending; equal logits
(-0.0 and +0.0 are equal) by ascending index; NaN below -inf, NaNs among themselves by ascending index.  Plus a float64
softmax and an fp32 emulation of the long-row summation order of csrc/topk.hip."""
import numpy as np


def topk(rows: np.ndarray, k: int) -> np.ndarray:
    """[r][length] float32 -> labels [r][k] int32"""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float32))
    out = np.empty((rows.shape[0], k), dtype=np.int32)
    index = np.arange(rows.shape[1])
    for r, row in enumerate(rows):
        with np.errstate(invalid="ignore"):                 # signalling NaN patterns in the cast
            v = row.astype(np.float64) + 0.0                # -0 -> +0
        nan = np.isnan(v)
        neg = np.where(nan, 0.0, -v)
        out[r] = np.lexsort((index, neg, nan))[:k]          # last key is primary: non-NaN first, then -value, then index
    return out


def topk_brute(row, k: int):
    """the same by pairwise comparison, O(n^2): the rank of an element is the number of elements that beat it"""
    row = np.asarray(row, dtype=np.float32)

    def beats(a, i, b, j):
        an, bn = np.isnan(a), np.isnan(b)
        if an or bn:
            return (not an and bn) or (an == bn and i < j)
        return a > b or (a == b and i < j)               # -0.0 == +0.0 in IEEE comparison

    rank = [sum(beats(row[j], j, row[i], i) for j in range(len(row))) for i in range(len(row))]
    order = np.argsort(rank)
    assert sorted(rank) == list(range(len(row)))
    return order[:k].astype(np.int32)


def softmax64(rows: np.ndarray) -> np.ndarray:
    x = np.atleast_2d(np.asarray(rows, dtype=np.float32)).astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def softmax_f32_strided(row: np.ndarray, threads: int = 256) -> np.ndarray:
    """One row in plain fp32 with csrc/topk.hip's long-row order: thread t sums elements t, t + 256, ... in ascending
    order; a 64-lane xor butterfly per wave; (w0 + w1) + (w2 + w3); then exp(x - max) / sum.  (np.exp in fp32 stands in for
    expf: both are within an ulp or two of the exact value.)"""
    row = np.asarray(row, dtype=np.float32)
    mx = row.max()
    e = np.exp((row - mx).astype(np.float32)).astype(np.float32)
    pad = np.zeros(-len(row) % threads, dtype=np.float32)
    per = np.concatenate([e, pad]).reshape(-1, threads)
    acc = np.zeros(threads, dtype=np.float32)
    for chunk in per:
        acc = (acc + chunk).astype(np.float32)
    w = acc.reshape(threads // 64, 64)
    for m in (32, 16, 8, 4, 2, 1):
        w = (w + w[:, np.arange(64) ^ m]).astype(np.float32)
    total = np.float32(np.float32(w[0, 0] + w[1, 0]) + np.float32(w[2, 0] + w[3, 0]))
    return (e / total).astype(np.float32)
