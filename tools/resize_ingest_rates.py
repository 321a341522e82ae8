#!/usr/bin/env python3
"""Resize + centre crop on the GPU against 224 px crops given, on ViT-B/16: what vit_hip_forward_device_u8_resized and
vit_hip_forward_u8_resized cost, in f32, bf16 and fp8.

Per precision, one context (max_batch = chunk), 4096 images in chunks of 512, configurations timed alternately, every one
--reps times:
  dev_u8            vit_hip_forward_device_u8 on 224 x 224 HWC crops in HBM (the u8 path)
  dev_resized_500   vit_hip_forward_device_u8_resized on 500 x 375 / 375 x 500 sources in HBM (alternating), bilinear, rs 256
  dev_resized_1333  the same on 1333 x 1000 / 1000 x 1333 sources
  host_resized      vit_hip_forward_u8_resized: the 500 x 375 sources in host memory, host logits + probabilities out
and then the resize kernel's own time per chunk (HIP events around vit_hip_resize_crop_u8) with its source read rate.
Median and spread ((max - min) / median).  Output: profiles/resize_ingest_rates.txt (or --out).
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


def device_sources(pkg, L, chunk, shape):
    """chunk images in one device buffer, alternating shape and its transpose (distinct random content per orientation)"""
    h, w = shape
    rng = np.random.default_rng(h)
    imgs = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8), rng.integers(0, 256, size=(w, h, 3), dtype=np.uint8)]
    per = h * w * 3
    buf = pkg.DeviceBuffer(chunk * per, dtype=np.uint8)
    descs = []
    for i in range(chunk):
        a = imgs[i & 1]
        ptr = buf.ptr.value + i * per
        pkg.binding.check(L.vh_h2d(C.c_void_p(ptr), a.ctypes.data_as(C.c_void_p), per, None), "vh_h2d")
        descs.append((ptr, a.shape[0], a.shape[1], a.shape[1] * 3))
    pkg.binding.check(L.vh_device_sync(), "vh_device_sync")
    return buf, pkg.binding.image_descs(descs), imgs, chunk * per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4096)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precisions", default="f32,bf16,fp8")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "resize_ingest_rates.txt"))
    args = ap.parse_args()
    pkg = graft.load_package()
    L, b = pkg.lib(), pkg.binding
    assert L.vh_init(0) == 0, L.vh_last_error()
    cfg = pkg.preset("vit_b_16")
    weights = pkg.synth_weights(cfg, 0)
    n, chunk, S, nc = args.images, args.chunk, cfg.img_size, cfg.num_classes
    assert n % chunk == 0
    steps = n // chunk
    norm = pkg.pixel_norm(*IMAGENET)
    rc = b.resize_crop(256, "bilinear")

    crops = np.random.default_rng(0).integers(0, 256, size=(chunk, S, S, 3), dtype=np.uint8)
    d_crops = pkg.DeviceBuffer.from_numpy(crops, dtype=np.uint8)
    src = {k: device_sources(pkg, L, chunk, shape) for k, shape in (("500", (375, 500)), ("1333", (1000, 1333)))}
    host_imgs = src["500"][2]
    host_descs, keep = b.host_image_descs([host_imgs[i & 1] for i in range(n)], "hwc")
    d_log, d_prob = pkg.DeviceBuffer(chunk * nc), pkg.DeviceBuffer(chunk * nc)
    d_out = pkg.DeviceBuffer(chunk * S * S * 3, dtype=np.uint8)
    logits, probs = np.empty((n, nc), np.float32), np.empty((n, nc), np.float32)
    rows = (b.f32p * n)(*[b.fptr(probs[i]) for i in range(n)])
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        b.check(L.vh_event_create(C.byref(e)), "vh_event_create")

    lines = [f"# tools/resize_ingest_rates.py: ViT-B/16, synthetic weights, {n} images in chunks of {chunk}, {args.reps} alternating "
             f"repetitions per configuration; images/s median (spread = (max - min) / median)",
             "# dev_u8: 224 x 224 HWC crops in HBM; dev_resized_*: sources of that size in HBM (both orientations), bilinear, "
             "resize_short 256, centre crop 224; host_resized: 500 x 375 sources in host memory, host logits + probs out; "
             "resize: vit_hip_resize_crop_u8 event ms per chunk and source bytes read per second"]
    for precision in args.precisions.split(","):
        m = pkg.ViTHip(cfg, weights, device=0, max_batch=chunk, precision=precision)

        def dev_u8():
            for _ in range(steps):
                m.forward_device_u8(d_crops.ptr, chunk, norm, "hwc", d_log.ptr, d_prob.ptr, None)
            m.sync()

        def dev_resized(key):
            def run():
                descs = src[key][1]
                for _ in range(steps):
                    b.check(L.vit_hip_forward_device_u8_resized(m.ctx, descs, chunk, 0, C.byref(rc), C.byref(norm), d_log.ptr,
                                                                d_prob.ptr, None), "vit_hip_forward_device_u8_resized")
                m.sync()
            return run

        def host_resized():
            b.check(L.vit_hip_forward_u8_resized(m.ctx, host_descs, n, 0, C.byref(rc), C.byref(norm), b.fptr(logits), rows),
                    "vit_hip_forward_u8_resized")

        runs = {"dev_u8": dev_u8, "dev_resized_500": dev_resized("500"), "dev_resized_1333": dev_resized("1333"),
                "host_resized": host_resized}
        outs = {}
        for name, fn in runs.items():   # warm-up, and a consistency check of the host and device forms
            fn()
            outs[name] = d_log.to_numpy((chunk, nc)) if name.startswith("dev") else logits.copy()
        assert np.array_equal(outs["host_resized"][:chunk], outs["dev_resized_500"]), precision
        rates = {k: [] for k in runs}
        for _ in range(args.reps):
            for name, fn in runs.items():
                t0 = time.perf_counter()
                fn()
                rates[name].append(n / (time.perf_counter() - t0))

        kernel = {}
        for key, (_, descs, _, nbytes) in src.items():
            ms = []
            for _ in range(args.reps * steps):
                b.check(L.vh_event_record(ev[0], m.stream), "vh_event_record")
                b.check(L.vit_hip_resize_crop_u8(m.ctx, descs, chunk, 0, C.byref(rc), d_out.ptr, None), "vit_hip_resize_crop_u8")
                b.check(L.vh_event_record(ev[1], m.stream), "vh_event_record")
                b.check(L.vh_event_sync(ev[1]), "vh_event_sync")
                t = C.c_float()
                b.check(L.vh_event_elapsed_ms(C.byref(t), ev[0], ev[1]), "vh_event_elapsed_ms")
                ms.append(t.value)
            kernel[key] = (spread(ms), nbytes)
        m.close()

        med = {k: spread(v) for k, v in rates.items()}
        for k, (r, sp) in med.items():
            lines.append(f"{precision:<5} {k:<16} {r:9.1f} img/s  (spread {100 * sp:4.1f} %, runs {', '.join(f'{x:.0f}' for x in rates[k])})")
        for key, ((t, sp), nbytes) in kernel.items():
            lines.append(f"{precision:<5} resize {key:<4} {t:7.3f} ms per chunk of {chunk}  (spread {100 * sp:4.1f} %)  "
                         f"{nbytes / 1e6:7.1f} MB of sources, {nbytes / (t * 1e-3) / 1e12:5.2f} TB/s")
        lines.append(f"{precision:<5} ratios: dev_resized_500/dev_u8 {med['dev_resized_500'][0] / med['dev_u8'][0]:.3f}  "
                     f"dev_resized_1333/dev_u8 {med['dev_resized_1333'][0] / med['dev_u8'][0]:.3f}  "
                     f"host_resized/dev_resized_500 {med['host_resized'][0] / med['dev_resized_500'][0]:.3f}")
        print("\n".join(lines[-7:]), flush=True)
    del keep
    for e in ev:
        L.vh_event_destroy(e)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
