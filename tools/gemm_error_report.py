#!/usr/bin/env python3
"""Error of each fp32-product arithmetic of the GEMM against a float64 reference, measured on the
GPU's own outputs (not a numpy model of them): the exact three-part bf16 split (default), the
fp16-pair emulation (opt-in), the native fp32 MFMA, and -- for scale -- the reference's own
sequential fp32 loop (the oracle port).  Errors are relative to the RMS of the exact results."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import __graft_entry__ as graft  # noqa: E402

SHAPES = [(512, 768, 2304), (512, 768, 3072), (512, 3072, 768)]
LABELS = (("split3", "3 x bf16, 6 products (default)"), ("fp16x2", "2 x fp16, 3 products"), ("native", "fp32 MFMA"))


def gpu_products(pkg, x, w, b):
    """x w^T + b in each arithmetic, on the GPU"""
    L, check = pkg.lib(), pkg.binding.check
    (M, K), N = x.shape, w.shape[0]
    d_x, d_w, d_b = (pkg.DeviceBuffer.from_numpy(a) for a in (x, w, b))
    d_o = pkg.DeviceBuffer(M * N)
    out = {}
    for which, _ in LABELS:
        if which == "fp16x2":
            scale = 2.0 ** (14 - int(np.frexp(np.abs(w).max())[1]))
            d_p = pkg.DeviceBuffer(N * K)
            check(L.vh_launch_split2h_planes(None, d_w.ptr, d_p.ptr, N, K, scale), "split")
            check(L.vh_launch_linear_h2(None, d_o.ptr, d_p.ptr, scale, d_x.ptr, d_b.ptr, M, K, N, 0, None), "h2")
        else:
            check(L.vh_launch_linear_math(None, d_o.ptr, d_w.ptr, d_x.ptr, d_b.ptr, M, K, N, 0, None,
                                          pkg.binding.FP32_MATH[which]), "linear")
        check(L.vh_device_sync(), "sync")
        out[which] = d_o.to_numpy((M, N))
    return out


def main():
    from oracle.oracle import Oracle
    orc = Oracle("vit_b_16")
    pkg = graft.load_package()
    pkg.binding.check(pkg.lib().vh_init(0), "vh_init")
    rng = np.random.default_rng(11)
    print("relative error against float64 (max | rms), per shape M x K x N")
    for M, K, N in SHAPES:
        x = rng.standard_normal((M, K)).astype(np.float32)
        w = (rng.standard_normal((N, K)) * 0.03).astype(np.float32)
        b = (rng.standard_normal(N) * 0.1).astype(np.float32)
        res = gpu_products(pkg, x, w, b)
        exact = x.astype(np.float64) @ w.astype(np.float64).T + b
        scale = np.sqrt((exact ** 2).mean())
        seq = orc.linear(x[:64], w, b, N)
        line = f"  {M}x{K}x{N}:"
        for which, label in LABELS:
            e = (res[which] - exact) / scale
            line += f"  {label}: {np.abs(e).max():.2e} | {np.sqrt((e ** 2).mean()):.2e};"
        e = (seq - exact[:64]) / scale
        line += f"  reference's sequential fp32 loop (64 rows): {np.abs(e).max():.2e} | {np.sqrt((e ** 2).mean()):.2e}"
        print(line)


if __name__ == "__main__":
    main()
