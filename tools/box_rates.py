#!/usr/bin/env python3
"""Box crops on the GPU against 224 px crops given, on ViT-B/16: what vit_hip_forward_device_u8_boxes and
vit_hip_forward_u8_boxes cost, in f32, bf16 and fp8 (the method of tools/resize_ingest_rates.py).

Per precision, one context (max_batch = chunk = 512), 4096 images in chunks of 512, configurations timed alternately, every
one --reps times:
  dev_u8         vit_hip_forward_device_u8 on 224 x 224 HWC crops in HBM (the u8 path: what every ratio is taken to)
  dev_whole_500  512 whole-image boxes of 512 sources of 500 x 375 / 375 x 500 in HBM (alternating), bilinear
  dev_tiles      512 boxes of one 4000 x 3000 frame in HBM: vit_tile_boxes at tile 224, stride 160 gives 19 x 25 = 475 tiles, the
                 first 37 are taken once more to fill the chunk
  dev_random     512 hashed quarter-pixel boxes (1 px .. the whole side each way) of 16 sources of 1333 x 1000 in HBM
  host_tiles     vit_hip_forward_u8_boxes: the 512 tiles, the frame in host memory, host logits + probabilities out
then the crop kernels' own time per chunk (HIP events around vit_hip_crop_boxes_u8), and the bytes the host form uploads
per box -- the chunking rule of include/ViT_opencl.h restated here over vit_box_rows -- next to the 3 x 224^2 bytes of a
ready crop.  Median and spread ((max - min) / median).  Output: profiles/box_rates.txt (or --out).
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
sys.path.insert(0, str(ROOT / "tests"))
import __graft_entry__ as graft  # noqa: E402
from box_ref import hashed_boxes  # noqa: E402

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def spread(xs):
    med = statistics.median(xs)
    return med, (max(xs) - min(xs)) / med


def upload(pkg, L, arrays):
    """HWC uint8 arrays into one device buffer, packed -> (buffer, [(ptr, h, w, row_stride)])"""
    buf = pkg.DeviceBuffer(sum(a.nbytes for a in arrays), dtype=np.uint8)
    descs, off = [], 0
    for a in arrays:
        ptr = buf.ptr.value + off
        pkg.binding.check(L.vh_h2d(C.c_void_p(ptr), a.ctypes.data_as(C.c_void_p), a.nbytes, None), "vh_h2d")
        descs.append((ptr, a.shape[0], a.shape[1], a.shape[1] * a.shape[2]))
        off += a.nbytes
    pkg.binding.check(L.vh_device_sync(), "vh_device_sync")
    return buf, pkg.binding.image_descs(descs)


def host_upload_bytes(b, shapes, boxes, max_batch, slot, out, f, chans):
    """bytes that vit_hip_forward_u8_boxes sends over PCIe for `boxes`: chunks of consecutive boxes, cut at max_batch or when
    the next box would push the packed rows past the slot; per chunk every source row that a box reads goes up once"""
    total, chunks, k = 0, 0, 0
    while k < len(boxes):
        rows, size, m = {}, 0, 0
        while m < max_batch and k + m < len(boxes):
            i, (_, top, _, bottom) = boxes[k + m]
            first, count = b.box_rows(shapes[i][0], top, bottom, out, f)
            fresh = set(range(first, first + count)) - rows.get(i, set())
            if size + len(fresh) * shapes[i][1] * chans > slot:
                break
            rows.setdefault(i, set()).update(fresh)
            size += len(fresh) * shapes[i][1] * chans
            m += 1
        total, chunks, k = total + size, chunks + 1, k + m
    return total, chunks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4096)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precisions", default="f32,bf16,fp8")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "box_rates.txt"))
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
    rng = np.random.default_rng(0)

    def image(h, w):
        return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)

    d_crops = pkg.DeviceBuffer.from_numpy(image(chunk * S, S).reshape(chunk, S, S, 3), dtype=np.uint8)
    two = [image(375, 500), image(500, 375)]
    frame = image(3000, 4000)
    tiles = pkg.tile_boxes(3000, 4000, S, 160)
    n_tiles = len(tiles)
    tiles = (tiles * (chunk // n_tiles + 1))[:chunk]
    sixteen = [image(1000, 1333) for _ in range(16)]
    work = {   # name -> (device buffer, image descriptors, number of images, boxes, bytes of the sources)
        "whole_500": upload(pkg, L, [two[i & 1] for i in range(chunk)]) +
        (chunk, [(i, (0, 0, two[i & 1].shape[1], two[i & 1].shape[0])) for i in range(chunk)], chunk * two[0].nbytes),
        "tiles": upload(pkg, L, [frame]) + (1, tiles, frame.nbytes),
        "random": upload(pkg, L, sixteen) + (16, [(k % 16, box) for k, box in enumerate(hashed_boxes(7, chunk, 1000, 1333))],
                                             16 * sixteen[0].nbytes),
    }
    box_arrays = {k: b.box_array(v[3]) for k, v in work.items()}
    host_desc, keep = b.host_image_descs([frame], "hwc")
    d_log, d_prob = pkg.DeviceBuffer(chunk * nc), pkg.DeviceBuffer(chunk * nc)
    d_out = pkg.DeviceBuffer(chunk * S * S * 3, dtype=np.uint8)
    logits, probs = np.empty((chunk, nc), np.float32), np.empty((chunk, nc), np.float32)
    rows = (b.f32p * chunk)(*[b.fptr(probs[i]) for i in range(chunk)])
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        b.check(L.vh_event_create(C.byref(e)), "vh_event_create")

    slot = chunk * 3 * S * S * 4
    up_bytes, up_chunks = host_upload_bytes(b, [frame.shape], tiles, chunk, slot, S, "bilinear", 3)
    lines = [f"# tools/box_rates.py: ViT-B/16, synthetic weights, {n} images in chunks of {chunk}, {args.reps} alternating "
             f"repetitions per configuration; images/s median (spread = (max - min) / median)",
             f"# dev_u8: 224 x 224 HWC crops in HBM; dev_whole_500: {chunk} whole-image boxes of 500 x 375 sources (both "
             f"orientations); dev_tiles: tile 224 / stride 160 boxes of one 4000 x 3000 frame ({n_tiles} tiles, the first "
             f"{chunk - n_tiles} once more); dev_random: hashed boxes of 16 sources of 1333 x 1000; all bilinear, sources in HBM; "
             f"host_tiles: the tiles through vit_hip_forward_u8_boxes, frame in host memory, host logits + probs out; "
             f"crops: vit_hip_crop_boxes_u8 event ms per chunk",
             f"host form, tiles: {up_bytes} bytes uploaded for {chunk} boxes in {up_chunks} chunk(s) = {up_bytes / chunk:.0f} bytes "
             f"per box, against {3 * S * S} bytes per box of uploading ready crops ({up_bytes / chunk / (3 * S * S):.2f} x)"]
    for precision in args.precisions.split(","):
        m = pkg.ViTHip(cfg, weights, device=0, max_batch=chunk, precision=precision)

        def dev_u8():
            for _ in range(steps):
                m.forward_device_u8(d_crops.ptr, chunk, norm, "hwc", d_log.ptr, d_prob.ptr, None)
            m.sync()

        def dev_boxes(key):
            def run():
                _, descs, n_images = work[key][:3]
                for _ in range(steps):
                    b.check(L.vit_hip_forward_device_u8_boxes(m.ctx, descs, n_images, box_arrays[key], chunk, 0, 0, C.byref(norm),
                                                              d_log.ptr, d_prob.ptr, None), "vit_hip_forward_device_u8_boxes")
                m.sync()
            return run

        def host_tiles():
            for _ in range(steps):
                b.check(L.vit_hip_forward_u8_boxes(m.ctx, host_desc, 1, box_arrays["tiles"], chunk, 0, 0, C.byref(norm),
                                                   b.fptr(logits), rows), "vit_hip_forward_u8_boxes")

        runs = {"dev_u8": dev_u8, "dev_whole_500": dev_boxes("whole_500"), "dev_tiles": dev_boxes("tiles"),
                "dev_random": dev_boxes("random"), "host_tiles": host_tiles}
        outs = {}
        for name, fn in runs.items():   # warm-up, and a consistency check of the host and device forms
            fn()
            outs[name] = d_log.to_numpy((chunk, nc)) if name.startswith("dev") else logits.copy()
        assert np.array_equal(outs["host_tiles"], outs["dev_tiles"]), precision
        rates = {k: [] for k in runs}
        for _ in range(args.reps):
            for name, fn in runs.items():
                t0 = time.perf_counter()
                fn()
                rates[name].append(n / (time.perf_counter() - t0))

        kernel = {}
        for key, (_, descs, n_images, _, nbytes) in work.items():
            ms = []
            for _ in range(args.reps * steps):
                b.check(L.vh_event_record(ev[0], m.stream), "vh_event_record")
                b.check(L.vit_hip_crop_boxes_u8(m.ctx, descs, n_images, box_arrays[key], chunk, 0, 0, d_out.ptr, None),
                        "vit_hip_crop_boxes_u8")
                b.check(L.vh_event_record(ev[1], m.stream), "vh_event_record")
                b.check(L.vh_event_sync(ev[1]), "vh_event_sync")
                t = C.c_float()
                b.check(L.vh_event_elapsed_ms(C.byref(t), ev[0], ev[1]), "vh_event_elapsed_ms")
                ms.append(t.value)
            kernel[key] = (spread(ms), nbytes)
        m.close()

        med = {k: spread(v) for k, v in rates.items()}
        for k, (r, sp) in med.items():
            lines.append(f"{precision:<5} {k:<14} {r:9.1f} img/s  (spread {100 * sp:4.1f} %, runs {', '.join(f'{x:.0f}' for x in rates[k])})")
        for key, ((t, sp), nbytes) in kernel.items():
            lines.append(f"{precision:<5} crops {key:<10} {t:7.3f} ms per chunk of {chunk}  (spread {100 * sp:4.1f} %)  "
                         f"{nbytes / 1e6:7.1f} MB of sources")
        lines.append(f"{precision:<5} ratios to dev_u8: " +
                     "  ".join(f"{k} {med[k][0] / med['dev_u8'][0]:.3f}" for k in list(runs)[1:]))
        print("\n".join(lines[-9:]), flush=True)
    del keep
    for e in ev:
        L.vh_event_destroy(e)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
