"""Attention rollout as include/ViT_opencl.h defines it, in NumPy float64, over a list of per-layer Q|K|V in fp32 (the
values a stored form decodes to: attn_ref's encoders and decoders make them), a plain fp32 NumPy emulation of the same
definition, and the derived bound.  Nothing here calls the kernels (csrc/rollout.hip).

    s_h[u][t] = (1/sqrt(D)) * sum_d Q[i*T+u][h*D+d] * K[i*T+t][h*D+d]
    P_h       = row softmax of s_h                       A_l = (sum over h of P_h) / H
    R_first   = 0.5 A_first + 0.5 I                      R_l = 0.5 (A_l . R_{l-1}) + 0.5 R_{l-1}
    rollout[i][t] = R_last[i][0][t]
"""
import numpy as np

from attn_ref import ROWS_F32, PLANES3, PLANES_F16, decode_f16, decode_planes3, encode_f16, encode_planes3  # noqa: F401


# The launcher cases (n, T, E, H) of tests/test_gpu_rollout.py, which tests/test_rollout_host.py holds the fp32 emulation
# to as well: T = 1 and 2; one below, at and above the 16-row query tile, the 32- and the 64-key chunk; several images;
# head_dim 64, 80 and 128; the token counts of the presets (197, 257, 577, 1370).
CASES = [(1, 1, 64, 1), (1, 2, 128, 2), (2, 15, 64, 4), (2, 16, 64, 4), (2, 17, 64, 4), (1, 31, 128, 2), (1, 32, 128, 2),
         (1, 33, 128, 2), (1, 64, 256, 2), (1, 65, 256, 2), (3, 50, 768, 12), (2, 197, 768, 12), (2, 257, 1280, 16),
         (1, 577, 128, 2), (1, 1370, 64, 1)]
AMPLITUDES = (1.0, 3.0)
STEPS = 3


def case_layers(n, T, E, H, amp):
    """the case's STEPS distinct Q|K|V, fp32 [n*T][3E] each: standard normal times amp"""
    base = np.random.default_rng(1000 * T + E).standard_normal((STEPS, n * T, 3 * E)).astype(np.float32)
    return [(np.float32(amp) * b).astype(np.float32) for b in base]


def stored_values(form, qkv):
    """the fp32 values the buffer of `form` made from qkv decodes to (the three-part planes are exact)"""
    return decode_f16(encode_f16(qkv)) if form == PLANES_F16 else qkv


def _qk(qkv, n, T, H, dtype):
    qkv = np.asarray(qkv)
    D = qkv.shape[1] // 3 // H
    x = qkv.astype(dtype).reshape(n, T, 3, H, D)
    return x[:, :, 0], x[:, :, 1], D                           # [n][T][H][D] each


def head_mean_attention(qkv, n, T, H, dtype=np.float64):
    """qkv fp32 [n*T][3E] -> A [n][T][T]: the mean over heads of the row softmax of Q K^T / sqrt(D), in `dtype`"""
    q, k, D = _qk(qkv, n, T, H, dtype)
    acc, scale = np.zeros((n, T, T), dtype), dtype(1.0) / np.sqrt(dtype(D))
    for h in range(H):                                          # ascending, as the definition sums
        s = (np.matmul(q[:, :, h], k[:, :, h].transpose(0, 2, 1)) * scale).astype(dtype)
        s = (s - s.max(axis=2, keepdims=True)).astype(dtype)
        p = np.exp(s).astype(dtype)
        acc = (acc + (p / p.sum(axis=2, keepdims=True, dtype=dtype)).astype(dtype)).astype(dtype)
    return (acc / dtype(H)).astype(dtype)


def rollout_steps(qkvs, n, T, H, dtype=np.float64):
    """qkvs: per layer from the first, fp32 [n*T][3E] -> [R after each layer], each [n][T][T] in `dtype`"""
    half, out, r = dtype(0.5), [], None
    for qkv in qkvs:
        a = head_mean_attention(qkv, n, T, H, dtype)
        if r is None:
            r = (half * a + half * np.eye(T, dtype=dtype)[None]).astype(dtype)
        else:
            r = (half * np.matmul(a, r).astype(dtype) + half * r).astype(dtype)
        out.append(r)
    return out


def rollout(qkvs, n, T, H):
    """-> rollout [n][T] float64: the class token's row of the last product"""
    return rollout_steps(qkvs, n, T, H)[-1][:, 0, :]


def rollout_steps_f32(qkvs, n, T, H):
    """the same definition with every operation rounded to fp32 (NumPy's own summation orders)"""
    return rollout_steps(qkvs, n, T, H, np.float32)


def score_magnitude(qkv, n, T, H):
    """S [n] = max over heads, queries and keys of sum_d |q_d k_d| / sqrt(D), float64"""
    q, k, D = _qk(qkv, n, T, H, np.float64)
    q, k = np.abs(q), np.abs(k)
    return np.array([max(float(np.matmul(q[i, :, h], k[i, :, h].T).max()) for h in range(H)) for i in range(n)]) / np.sqrt(D)


def bound(qkvs, n, T, H):
    """-> [b after each layer], each [n][1][1]: |R - ref| <= b * ref + 1e-30.  Every intermediate is non-negative, so
    relative errors add: per layer the score, exponential, row-sum and division terms of attn_ref.bound
    (4 (D + 2) S + T + 64), H + 1 for the head mean, T + 4 for the product and the mix, and 1 for the fp32 rounding of the
    result the test compares."""
    D = np.asarray(qkvs[0]).shape[1] // 3 // H
    out, acc = [], np.zeros(n)
    for qkv in qkvs:
        acc = acc + (4 * (D + 2) * score_magnitude(qkv, n, T, H) + 2 * T + H + 70) * 2.0 ** -24
        out.append(acc[:, None, None].copy())
    return out
