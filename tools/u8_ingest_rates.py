#!/usr/bin/env python3
"""8-bit input against fp32 input on ViT-B/16: what the u8 path (vit_hip_forward_device_u8 / vit_hip_forward_u8) does to
throughput, device-resident and through the host-pointer pipeline, in f32, bf16 and fp8.

Per precision, one context (max_batch = chunk), 4096 images in chunks of 512, four configurations timed alternately, every
one --reps times:
  dev_f32   vit_hip_forward_device on fp32 [C][H][W] images in HBM       (bench.py's kind of number)
  dev_u8    vit_hip_forward_device_u8 on HWC bytes in HBM
  host_f32  vit_hip_forward: separately allocated fp32 host images in, host logits + probabilities out
  host_u8   vit_hip_forward_u8: contiguous HWC bytes in host memory in, the same outputs
and then the VIT_OP_PATCH_EMBED event time per chunk of the fp32 and u8 sources (profiling only that operator), alternating.
The host images are normalised on the host once, outside every timed region (its cost is not in host_f32).
Median and spread ((max - min) / median) per configuration.  Output: profiles/u8_ingest_rates.txt (or --out).
"""
from __future__ import annotations

import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as graft  # noqa: E402

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def spread(xs):
    med = statistics.median(xs)
    return med, (max(xs) - min(xs)) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4096)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precisions", default="f32,bf16,fp8")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "u8_ingest_rates.txt"))
    args = ap.parse_args()
    pkg = graft.load_package()
    L = pkg.lib()
    assert L.vh_init(0) == 0, L.vh_last_error()
    cfg = pkg.preset("vit_b_16")
    weights = pkg.synth_weights(cfg, 0)
    n, chunk, S, Ch, nc = args.images, args.chunk, cfg.img_size, cfg.in_chans, cfg.num_classes
    assert n % chunk == 0
    steps = n // chunk

    norm = pkg.pixel_norm(*IMAGENET)
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, size=(chunk, S, S, Ch), dtype=np.uint8)
    scale, bias = np.array(norm.scale[:Ch], np.float32), np.array(norm.bias[:Ch], np.float32)
    f32_chunk = np.ascontiguousarray(((base.astype(np.float32) * scale) + bias).transpose(0, 3, 1, 2))
    u8 = np.empty((n, S, S, Ch), np.uint8)        # the same chunk repeated: [n][H][W][C] bytes ...
    f32 = np.empty((n, Ch, S, S), np.float32)     # ... and [n][C][H][W] normalised
    for k in range(steps):
        u8[k * chunk:(k + 1) * chunk] = base
        f32[k * chunk:(k + 1) * chunk] = f32_chunk
    img_array = pkg.binding.image_array(f32)
    logits, probs = np.empty((n, nc), np.float32), np.empty((n, nc), np.float32)
    rows = (pkg.binding.f32p * n)(*[pkg.binding.fptr(probs[i]) for i in range(n)])
    u8_ptr = u8.ctypes.data_as(C.POINTER(C.c_ubyte))

    d_f32 = pkg.DeviceBuffer.from_numpy(f32_chunk)
    d_u8 = pkg.DeviceBuffer.from_numpy(base, dtype=np.uint8)
    d_log, d_prob = pkg.DeviceBuffer(chunk * nc), pkg.DeviceBuffer(chunk * nc)

    lines = [f"# tools/u8_ingest_rates.py: ViT-B/16, synthetic weights, {n} images in chunks of {chunk}, {args.reps} alternating "
             f"repetitions per configuration; images/s median (spread = (max - min) / median)",
             "# dev_*: device-resident inputs (fp32 [C][H][W] / u8 HWC), logits + probs left in HBM; host_*: host images in, "
             "host logits + probs out (vit_hip_forward / vit_hip_forward_u8, HWC); patch_embed: VIT_OP_PATCH_EMBED event ms per chunk"]
    for precision in args.precisions.split(","):
        m = pkg.ViTHip(cfg, weights, device=0, max_batch=chunk, precision=precision)

        def dev_f32():
            for _ in range(steps):
                m.forward_device(d_f32.ptr, chunk, d_log.ptr, d_prob.ptr, None)
            m.sync()

        def dev_u8():
            for _ in range(steps):
                m.forward_device_u8(d_u8.ptr, chunk, norm, "hwc", d_log.ptr, d_prob.ptr, None)
            m.sync()

        def host_f32():
            pkg.binding.check(L.vit_hip_forward(m.ctx, img_array, n, pkg.binding.fptr(logits), rows), "vit_hip_forward")

        def host_u8():
            pkg.binding.check(L.vit_hip_forward_u8(m.ctx, u8_ptr, n, 0, C.byref(norm), pkg.binding.fptr(logits), rows),
                              "vit_hip_forward_u8")

        runs = {"dev_f32": dev_f32, "dev_u8": dev_u8, "host_f32": host_f32, "host_u8": host_u8}
        outs = {}
        for name, fn in runs.items():   # warm-up, and the outputs of each path for the identity check below
            fn()
            outs[name] = (d_log.to_numpy((chunk, nc)) if name.startswith("dev") else logits.copy())
        assert np.array_equal(outs["dev_f32"], outs["dev_u8"]), precision
        assert np.array_equal(outs["host_f32"], outs["host_u8"]) and np.array_equal(outs["host_u8"][:chunk], outs["dev_u8"])
        rates = {k: [] for k in runs}
        for _ in range(args.reps):
            for name, fn in runs.items():
                t0 = time.perf_counter()
                fn()
                rates[name].append(n / (time.perf_counter() - t0))

        pe = {"f32": [], "u8": []}
        m.profile_enable(steps)
        m.profile_select(["patch_embed"])
        for _ in range(args.reps):
            for src, fn in (("f32", dev_f32), ("u8", dev_u8)):
                fn()
                ms, launches = m.profile_read()["patch_embed"]
                assert launches == steps
                pe[src].append(ms / steps)
        m.profile_enable(0)
        m.close()

        med = {k: spread(v) for k, v in rates.items()}
        for k, (r, sp) in med.items():
            lines.append(f"{precision:<5} {k:<9} {r:9.1f} img/s  (spread {100 * sp:4.1f} %, runs {', '.join(f'{x:.0f}' for x in rates[k])})")
        for src in ("f32", "u8"):
            t, sp = spread(pe[src])
            lines.append(f"{precision:<5} patch_embed {src:<3} {t:7.3f} ms per chunk of {chunk}  (spread {100 * sp:4.1f} %)")
        lines.append(f"{precision:<5} ratios: dev_u8/dev_f32 {med['dev_u8'][0] / med['dev_f32'][0]:.3f}  "
                     f"host_u8/host_f32 {med['host_u8'][0] / med['host_f32'][0]:.3f}  "
                     f"host_f32/dev_f32 {med['host_f32'][0] / med['dev_f32'][0]:.3f}  "
                     f"host_u8/dev_f32 {med['host_u8'][0] / med['dev_f32'][0]:.3f}  "
                     f"host_u8/dev_u8 {med['host_u8'][0] / med['dev_u8'][0]:.3f}  "
                     f"patch_embed u8/f32 {spread(pe['u8'])[0] / spread(pe['f32'])[0]:.3f}")
        print("\n".join(lines[-7:]), flush=True)
    for d in (d_f32, d_u8, d_log, d_prob):
        d.free()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
