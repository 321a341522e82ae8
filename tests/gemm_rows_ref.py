"""What tests/test_gpu_gemm_rows_classes.py and tests/test_gemm_rows_host.py share: the inputs of the fp32-rows GEMM cases
(csrc/gemm_mfma.hip), their float64 statement, the error of the reference's own fp32 loop on the same rows (the yardstick of
the sharper bound), and a numpy emulation of the six-product sum in the kernel's order.  The GPU test and the host test
draw their inputs from `inputs` below, so a change of seed or scale reaches both.

The sharper bound, K = 96, split and native arithmetic:   max|kernel - float64| <= SHARP * max|fp32 loop - float64|.
SHARP = 2 comes from a CPU experiment on these inputs (K = 96, N = 512, 1500 rows): the six products in the kernel's order
sit at 0.41 x the loop's error, any one third-order product dropped (w0.a2, w2.a0, w1.a1) at 5.8 .. 6.9 x.  At K = 2048 the
loop's own rounding closes the gap (5.6e-6 against 7.4e-6 with a product dropped), so the bound is stated at K = 96 only."""
import numpy as np

N = 512
SHARP = 2.0
REF_ROWS = 8192                         # rows per evaluation of the float64 statement
TERMS = ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0))    # (weight part, activation part) per MFMA of a block: smallest first
THIRD_ORDER = ((0, 2), (2, 0), (1, 1))


def inputs(oracle, M, K, n=N, seed=4100):
    """x [M][K] at scale 1 offset 0.1, w [n][K] at 0.04, bias [n] at 0.1: the project's usual operator inputs"""
    x = oracle.synth_fill(M * K, seed + K, 1.0, 0.1).reshape(M, K)
    w = oracle.synth_fill(n * K, seed + 1 + K, 0.04, 0.0).reshape(n, K)
    b = oracle.synth_fill(n, seed + 2, 0.1, 0.0)
    return x, w, b


def residual(oracle, M, n=N, seed=4100):
    return oracle.synth_fill(M * n, seed + 3, 1.0, 0.0).reshape(M, n)


def gelu64(v):
    """erf-GELU in float64 (torch's vectorised erf)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64))
    return (0.5 * t * (1.0 + torch.erf(t / np.sqrt(2.0)))).numpy()


def linear64(x, w, b):
    """x . w^T + b in float64 (torch's float64 matmul)"""
    import torch
    return (torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)) @ torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).T
            + torch.from_numpy(np.ascontiguousarray(b, dtype=np.float64))).numpy()


def want64(x, w, b, epi, r=None):
    v = linear64(x, w, b)
    if epi == "GELU":
        v = gelu64(v)
    if epi == "RESID":
        v = r.astype(np.float64) + v
    return v


def loop32(oracle, x, w, b, epi, r=None):
    """the reference's own sequential fp32 loop (ViT_seq.c:295-309), its GELU (:283) and its residual add (:348-351)"""
    v = oracle.linear(x, np.ascontiguousarray(w).ravel(), b, w.shape[0])
    if epi == "GELU":
        v = oracle.gelu(v.ravel()).reshape(v.shape)
    if epi == "RESID":
        v = r + v
    return v


def bf16_rne(x):
    """float32 -> nearest-even bfloat16, as float32 (finite inputs)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32)).view(np.float32)


def split3(x):
    """the exact three-part split x = p0 + p1 + p2 of csrc/fp32_split.h"""
    p0 = bf16_rne(x)
    p1 = bf16_rne(x - p0)
    return p0, p1, bf16_rne(x - p0 - p1)


def six_products(x, w, b, drop=None):
    """gemm_mf16_kernel's sum in numpy: the accumulator starts at the bias; per K step of 32 values six products of bf16
    parts, smallest terms first (TERMS), each a 32-wide block product added to the fp32 accumulator.  The parts' products are
    exact in fp32; a block's 32 of them are summed in fp32 (numpy's order, not the matrix core's: the emulation claims the
    size of the error, not its bits).  drop: one (weight part, activation part) pair left out -- a defect."""
    xs, ws = split3(x), split3(w)
    acc = np.broadcast_to(b.astype(np.float32), (x.shape[0], w.shape[0])).copy()
    for k0 in range(0, x.shape[1], 32):
        for wp, ap in TERMS:
            if (wp, ap) != drop:
                acc = acc + xs[ap][:, k0:k0 + 32] @ ws[wp][:, k0:k0 + 32].T
    assert acc.dtype == np.float32
    return acc
