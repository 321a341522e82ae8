#!/usr/bin/env python3
"""What a context derived at another resolution (vit_hip_create_at_resolution) costs next to creating one from host tensors.

One process, synthetic weights, per (model, target size, precision):
  derived   wall time of vit_hip_create_at_resolution from a resident 224-pixel context: device-to-device copies of every
            weight in the form it has, the position grid resampled on the GPU, the arena
  native    wall time of vit_hip_create_ex at the target size from host tensors: upload, split / round / quantise / fold of
            the four big matrices of every layer, the arena
alternating, `--reps` times each (the first pair is a warm-up and is not reported), and the resample kernel's own time from
HIP events on the null stream around vh_launch_resample_pos_embed alone (median of 20 after 2 warm-ups), against its traffic
floor (source grid + output, once each, at 4 TB/s).
Output: profiles/pos_resample_rates.txt (or --out)."""
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

HBM = 4.0e12
CASES = [("vit_b_16", 384), ("vit_h_14", 518)]


def kernel_ms(pkg, grid_in, grid_out, E, mode, ac):
    L = pkg.lib()
    rng = np.random.default_rng(1)
    src = pkg.DeviceBuffer.from_numpy(rng.standard_normal((1 + grid_in * grid_in, E)).astype(np.float32))
    dst = pkg.DeviceBuffer((1 + grid_out * grid_out) * E)
    a, b = C.c_void_p(), C.c_void_p()
    assert L.vh_event_create(C.byref(a)) == 0 and L.vh_event_create(C.byref(b)) == 0
    out = []
    for _ in range(22):
        L.vh_event_record(a, None)
        assert L.vh_launch_resample_pos_embed(None, src.ptr, dst.ptr, 1, grid_in, grid_in, grid_out, grid_out, E, mode, ac) == 0, \
            L.vh_last_error()
        L.vh_event_record(b, None)
        assert L.vh_event_sync(b) == 0, L.vh_last_error()
        ms = C.c_float()
        L.vh_event_elapsed_ms(C.byref(ms), a, b)
        out.append(ms.value)
    L.vh_event_destroy(a)
    L.vh_event_destroy(b)
    src.free()
    dst.free()
    return statistics.median(out[2:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pos_resample_rates.txt"))
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--max-batch", type=int, default=8)
    ap.add_argument("--precisions", default="f32,bf16")
    args = ap.parse_args()
    pkg = graft.load_package()
    L = pkg.lib()
    assert L.vh_init(0) == 0, L.vh_last_error()
    lines = ["# tools/pos_resample_rates.py: synthetic weights, max_batch %d; wall ms of a context at the target size derived from a "
             "resident 224 px context (vit_hip_create_at_resolution) and created from host tensors (vit_hip_create_ex), alternating; "
             "the resample kernel alone from HIP events" % args.max_batch]
    for name, img in CASES:
        cfg = pkg.preset(name)
        weights = pkg.synth_weights(cfg, 0)
        target = pkg.binding.resample_check(cfg, img)
        g_in, g_out, E = cfg.img_size // cfg.patch_size, img // cfg.patch_size, cfg.embed_dim
        w_t = list(weights)
        w_t[3] = np.resize(weights[3], (g_out * g_out + 1) * E).astype(np.float32)   # any values: only the work is timed
        for precision in args.precisions.split(","):
            src = pkg.ViTHip(cfg, weights, device=0, max_batch=args.max_batch, precision=precision)
            derived, native = [], []
            for _ in range(args.reps + 1):
                t0 = time.perf_counter()
                d = src.at_resolution(img)
                t1 = time.perf_counter()
                d.close()
                t2 = time.perf_counter()
                n = pkg.ViTHip(target, w_t, device=0, max_batch=args.max_batch, precision=precision)
                t3 = time.perf_counter()
                n.close()
                derived.append((t1 - t0) * 1e3)
                native.append((t3 - t2) * 1e3)
            src.close()
            derived, native = derived[1:], native[1:]
            md, mn = statistics.median(derived), statistics.median(native)
            line = (f"{name} -> {img} px {precision:5s} derived {md:9.1f} ms (runs {', '.join(f'{v:.1f}' for v in derived)})   "
                    f"native {mn:9.1f} ms (runs {', '.join(f'{v:.1f}' for v in native)})   derived/native {md / mn:.3f}")
            print(line, flush=True)
            lines.append(line)
        for mode, mname in ((0, "bicubic"), (1, "bilinear")):
            ms = kernel_ms(pkg, g_in, g_out, E, mode, 0)
            floor = ((g_in * g_in + 1) + (g_out * g_out + 1)) * E * 4 / HBM * 1e3
            line = (f"{name} -> {img} px vh_launch_resample_pos_embed alone, {mname}, grid {g_in} -> {g_out}, E {E}: {ms:.4f} ms "
                    f"(traffic floor {floor:.5f} ms)")
            print(line, flush=True)
            lines.append(line)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
