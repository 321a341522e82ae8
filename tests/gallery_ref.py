"""Reference for the gallery search (vh_launch_gallery_topk, csrc/gallery.hip; vit_hip_set_gallery): scores in float64, the
error bound include/kernelHandler.h states, and `check`, which judges a returned ranking WITHOUT deciding near-ties -- at
E = 768 on unit vectors a fifth of the top-32 gaps lie inside the worst-case bound, so "equals the float64 ranking" is not a
property an fp32 search can have."""
import numpy as np


def bf16_round(a):
    """fp32 -> bf16 bits (uint16), round to nearest even; finite values only"""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_decode(bits):
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def scores64(q, rows):
    """[n][G] exact products of the fp32 values, summed in float64"""
    return np.asarray(q, np.float64) @ np.asarray(rows, np.float64).T


def bound(q, rows, E):
    """[n][G]: (E + 8) * 2^-24 * sum_d |q_d g_d|, in float64"""
    return (E + 8) * 2.0 ** -24 * (np.abs(np.asarray(q, np.float64)) @ np.abs(np.asarray(rows, np.float64)).T)


def key_order(scores, indices):
    """sort keys of the ranking rule, ascending = better first: score descending (-0 == +0), NaN last, then index ascending"""
    s = np.asarray(scores, np.float64)
    nan = np.isnan(s)
    return np.where(nan, 0.0, -s) + 0.0, nan, np.asarray(indices)


def rank_exact(scores, k):
    """the ranking rule applied to scores [n][G] as they are: indices [n][k]"""
    out = np.empty((scores.shape[0], k), np.int32)
    for i, row in enumerate(scores):
        neg, nan, idx = key_order(row, np.arange(row.size))
        out[i] = np.lexsort((idx, neg, nan))[:k]
    return out


def check(q, rows, k, indices, scores, report=None):
    """Asserts, for every query, with no case left out: (a) indices distinct and in range; (b) the returned scores
    non-increasing, equal scores by ascending index; (c) |score - scores64| <= bound; (d) completeness -- every row not
    returned has scores64 <= scores64 of the k-th returned row plus the two bounds.  Finite data.  Returns the worst
    |error| / bound (also appended to `report`, a list, when given)."""
    q, rows = np.asarray(q, np.float32), np.asarray(rows, np.float32)
    n, E = q.shape
    G = rows.shape[0]
    indices, scores = np.asarray(indices), np.asarray(scores, np.float32)
    assert indices.shape == (n, k) and scores.shape == (n, k)
    ref, bnd = scores64(q, rows), bound(q, rows, E)
    worst = 0.0
    for i in range(n):
        idx, sc = indices[i], scores[i]
        assert ((idx >= 0) & (idx < G)).all(), f"query {i}: index out of range: {idx}"
        assert len(set(idx.tolist())) == k, f"query {i}: duplicate index: {idx}"
        for j in range(k - 1):
            assert sc[j] > sc[j + 1] or (sc[j] == sc[j + 1] and idx[j] < idx[j + 1]), \
                f"query {i}: positions {j}, {j + 1} out of order: {sc[j]!r}@{idx[j]} before {sc[j + 1]!r}@{idx[j + 1]}"
        err, b = np.abs(sc.astype(np.float64) - ref[i, idx]), bnd[i, idx]
        assert (err <= b).all(), f"query {i}: score error {err.max():.3e} beyond the bound {b[err.argmax()]:.3e}"
        worst = max(worst, float((err / np.maximum(b, 1e-300)).max()))
        rest = np.ones(G, bool)
        rest[idx] = False
        if rest.any():
            kth = idx[-1]
            over = ref[i, rest] - bnd[i, rest] - (ref[i, kth] + bnd[i, kth])
            assert (over <= 0).all(), \
                f"query {i}: row {np.flatnonzero(rest)[over.argmax()]} beats the k-th returned row {kth} by {over.max():.3e} beyond both bounds"
    if report is not None:
        report.append(worst)
    return worst
