#!/usr/bin/env python3
"""What a whole frame costs: vit_hip_segment_frame_device_u8 against what the parent commit offers, and the stitch kernel's time
against its floors.

A 3000 x 4000 x 3 synthetic 8-bit frame, device-resident, tiled 224 / stride 160 (vit_tile_boxes: 475 windows); ViT-B/16,
synthetic weights, max_batch 64, heads of 21 and of 150 labels.  One child process per precision; in each, alternating so
that both see the same clocks, the wall time of
  frame     vit_hip_segment_frame_device_u8, labels only: complete on return
  windows   the same windows through vit_hip_forward_device_u8_boxes in chunks of max_batch with a dense request armed for
            224 x 224 labels per window, then one sync: the per-window label maps the parent commit stops at
The stitch kernel alone (vh_launch_dense_stitch on gaussian patch logits of the same windows) is timed in two further child
processes under `rocprofv3 --kernel-trace --stats`, one per label count: the launcher copies its index synchronously before
it launches, which HIP events around the call would count in.  Its floors:
  VALU     pixels * C * (7 * mean cover + 14) lane-operations / (256 CUs * 128 lanes * 2.4 GHz): per covering window three
           lerps (6) and the add, per pixel the division (10) and the ranking (4); coordinates and loads not counted
  L1       pixels * mean cover * ceil(C / 16) * 16 loads of 16 bytes per lane, a CU's vector L1 taken at 64 bytes per clock (the rate
           the counters recorded in profiles/frame_rates.txt show it at); the line names the largest floor computed
  traffic  (pixels + patch logits * 4) bytes / 4 TB/s
Output: profiles/frame_rates.txt (or --out)."""
from __future__ import annotations

import argparse
import csv
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as graft  # noqa: E402

E, P, GRID = 768, 196, (14, 14)
FH, FW, TILE, STRIDE, MAX_BATCH = 3000, 4000, 224, 160, 64
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
HBM = 4.0e12
LANES = 256 * 128 * 2.4e9
L1_BYTES = 256 * 64 * 2.4e9


def make_head(pkg, c):
    rng = np.random.default_rng(c)
    return (pkg.DeviceBuffer.from_numpy((rng.standard_normal((c, E)) / np.sqrt(E)).astype(np.float32)),
            pkg.DeviceBuffer.from_numpy((0.1 * rng.standard_normal(c)).astype(np.float32)))


def child(args):
    pkg = graft.load_package()
    b, L = pkg.binding, pkg.lib()
    assert L.vh_init(0) == 0, L.vh_last_error()
    cfg = pkg.preset("vit_b_16")
    m = pkg.ViTHip(cfg, pkg.synth_weights(cfg, 0), device=0, max_batch=MAX_BATCH, precision=args.precision)
    frame = np.random.default_rng(3).integers(0, 256, size=(FH, FW, 3), dtype=np.uint8)
    d_frame = pkg.DeviceBuffer.from_numpy(frame, dtype=np.uint8)
    desc = (d_frame.ptr.value, FH, FW, FW * 3)
    windows = pkg.tile_boxes(FH, FW, TILE, STRIDE)
    norm = pkg.pixel_norm(MEAN, STD)
    d_out = pkg.DeviceBuffer(FH * FW, np.uint8)
    d_maps = pkg.DeviceBuffer(MAX_BATCH * TILE * TILE, np.uint8)
    lines = []
    for c in (int(x) for x in args.labels.split(",")):
        head = make_head(pkg, c)

        def frame_call():
            t0 = time.perf_counter()
            m.segment_frame_device(desc, windows, norm, head[0], head[1], labels=d_out, n_labels=c, weight_stride=E)
            return (time.perf_counter() - t0) * 1e3

        def window_maps():
            m.set_dense(b.DenseSpec(c, 0, 0, -1, True, E), head[0], head[1], labels=d_maps)
            try:
                t0 = time.perf_counter()
                for a in range(0, len(windows), MAX_BATCH):
                    m.forward_device_u8_boxes([desc], windows[a:a + MAX_BATCH], norm)
                m.sync()
                return (time.perf_counter() - t0) * 1e3
            finally:
                m.set_dense(None)

        frame_call(), window_maps()
        runs = {"frame": [], "windows": []}
        for _ in range(args.reps):
            runs["frame"].append(frame_call())
            runs["windows"].append(window_maps())
        med = {k: statistics.median(v) for k, v in runs.items()}
        tag = f"vit_b_16 {args.precision:<5} {len(windows)} windows C={c:<3}"
        for k, v in runs.items():
            lines.append(f"{tag} {k:<8} {med[k]:8.2f} ms  (runs {', '.join(f'{x:.2f}' for x in v)})")
        lines.append(f"{tag} frame - windows = {med['frame'] - med['windows']:+.2f} ms")
    m.close()
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


def stitch_only(args):
    """the launcher alone, args.reps + 2 times, for the kernel trace; prints the mean cover and the id count"""
    pkg = graft.load_package()
    b, L = pkg.binding, pkg.lib()
    assert L.vh_init(0) == 0, L.vh_last_error()
    import ctypes as C
    c = int(args.labels)
    boxes = np.array([w[1] for w in pkg.tile_boxes(FH, FW, TILE, STRIDE)], np.float32)
    n = len(boxes)
    offsets, ids = b.stitch_index(FH, FW, boxes)
    d_pl = pkg.DeviceBuffer.from_numpy(np.random.default_rng(2).standard_normal((n, P, c)).astype(np.float32))
    need = L.vh_dense_stitch_scratch(n, FH, FW, len(ids))
    d_scr, d_lab, d_cov = pkg.DeviceBuffer(need // 4 + 4), pkg.DeviceBuffer(FH * FW, np.uint8), pkg.DeviceBuffer(FH * FW, np.uint8)
    ip = C.POINTER(C.c_int)
    for k in range(args.reps + 2):
        b.check(L.vh_launch_dense_stitch(None, d_pl.ptr, n, GRID[0], GRID[1], c, b.fptr(boxes), FH, FW, offsets.ctypes.data_as(ip),
                                         ids.ctypes.data_as(ip), 255, d_scr.ptr, need, d_lab.ptr, None, d_cov.ptr if k == 0 else None),
                "vh_launch_dense_stitch")
        b.check(L.vh_device_sync(), "sync")
        if k == 0:
            print(f"cover {d_cov.to_numpy().astype(np.float64).mean():.4f} ids {len(ids)} windows {n}", flush=True)


def kernel_ms(args, c):
    """the trace's average over the launches, in ms, of dense_stitch_kernel for c labels; calls, best, the cover line"""
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, __file__,
                            "--stitch-only", "--labels", str(c), "--reps", str(args.reps)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
        cover = next(line for line in r.stdout.splitlines() if line.startswith("cover "))
        stats = next(Path(tmp).rglob("*kernel_stats.csv"))
        with open(stats) as f:
            rows = list(csv.DictReader(f))
    row = next(r_ for r_ in rows if "dense_stitch_kernel" in r_["Name"])
    return float(row["AverageNs"]) / 1e6, int(row["Calls"]), float(row["MinNs"]) / 1e6, cover.split()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--labels", default="21,150")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "frame_rates.txt"))
    ap.add_argument("--precision")
    ap.add_argument("--precisions", default="f32,bf16,fp8")
    ap.add_argument("--stitch-only", action="store_true")
    args = ap.parse_args()
    if args.stitch_only:
        return stitch_only(args)
    if args.precision:
        return child(args)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(f"# tools/frame_rates.py: a {FH} x {FW} x 3 device-resident frame tiled {TILE} / stride {STRIDE}, ViT-B/16, synthetic "
                              f"weights, max_batch {MAX_BATCH}; wall ms, median of alternating runs; the stitch kernel from rocprofv3 --kernel-trace --stats.  "
                              "The L1 floor takes a CU's vector L1 at 64 bytes per clock (the counters at the end of the recorded file show it at that "
                              "rate); \"of the L1 floor\" names the largest floor computed\n")
    lines = []
    for c in (int(x) for x in args.labels.split(",")):
        avg, calls, best, (_, cover, _, ids, _, n) = kernel_ms(args, c)
        cover, pixels, n = float(cover), FH * FW, int(n)
        valu = pixels * c * (7 * cover + 14) / LANES * 1e3
        l1 = pixels * cover * -(-c // 16) * 16 * 16 / L1_BYTES * 1e3
        traffic = (pixels + n * P * c * 4) / HBM * 1e3
        floors = {"VALU": valu, "L1": l1, "traffic": traffic}
        bind = max(floors, key=floors.get)
        lines.append(f"stitch kernel C={c:<3} {n} windows, mean cover {cover:.3f}, {ids} ids: {avg:.3f} ms average of {calls} launches (best {best:.3f}): "
                     f"VALU floor {valu:.3f} ms, L1 floor {l1:.3f} ms, traffic floor {traffic:.3f} ms -> {floors[bind] / avg:.3f} of the {bind} floor")
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    for precision in args.precisions.split(","):
        subprocess.run([sys.executable, __file__, "--precision", precision, "--labels", args.labels, "--reps", str(args.reps), "--out", args.out],
                       check=True, timeout=900)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
