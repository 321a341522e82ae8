#!/usr/bin/env python3
"""What the soft maps of a whole frame cost: the soft stitch kernel's variants against the labels stitch on the same logits and
against their floors, and vit_hip_segment_frame_soft_device_u8 against vit_hip_segment_frame_device_u8.

tools/frame_rates.py's frame: 3000 x 4000 x 3, 8-bit, device-resident, tiled 224 / stride 160 (475 windows); ViT-B/16,
synthetic weights, max_batch 64, heads of 21 and of 150 labels.

Kernels: one child process per label count under `rocprofv3 --kernel-trace --stats` (the launchers copy their index
synchronously before they launch, which events around the call would count in).  In it, on gaussian patch logits of the
windows, vh_launch_dense_stitch and vh_launch_dense_stitch_soft in every variant that takes the label count (through the
internal entry that takes the variant per call, csrc/vit_kernels.h: 1 recompute, 2 registers), with all three maps and with
prob alone, round-robin so that all see the same clocks.  The template arguments in the kernel's name tell the instances apart.  Floors of a soft launch of
`passes` blends per class (2 recompute, 1 stash):
  VALU   pixels * C * (passes * (7 * mean cover + 10) + 12) lane-operations / (256 CUs * 128 lanes * 2.4 GHz): per covering
         window three lerps (6) and the add, per blend the division (10), per class the maximum and the softmax's terms (sub,
         mul, exp at quarter rate, add, two fma, max: 12 with all maps); coordinates and loads not counted
  L1     pixels * mean cover * ceil(C / 16) * 16 loads of 16 bytes per lane * passes, a CU's vector L1 at 64 bytes per clock
`--kernel-only` is that child; with --variant and --maps it launches one instance only, which is what a counter run of its
own wraps: rocprofv3 --pmc <counters> -- python tools/frame_soft_rates.py --kernel-only --labels 150 --variant 1 --maps all --reps 1

Calls: one child process per precision; in each, alternating, the wall time of
  soft      vit_hip_segment_frame_soft_device_u8, labels and all three maps
  prob      the same, prob alone and no labels
  labels    vit_hip_segment_frame_device_u8, labels only
Output: profiles/frame_soft_rates.txt (or --out)."""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import re
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
LANES = 256 * 128 * 2.4e9
L1_BYTES = 256 * 64 * 2.4e9
VARIANTS = {1: "recompute", 2: "registers"}
LIMIT = {1: 256, 2: 160}
STASH = {"0": 1, "2": 2, "4": 2, "7": 2, "10": 2}     # the kernel's third template argument -> the variant


def make_head(pkg, c):
    rng = np.random.default_rng(c)
    return (pkg.DeviceBuffer.from_numpy((rng.standard_normal((c, E)) / np.sqrt(E)).astype(np.float32)),
            pkg.DeviceBuffer.from_numpy((0.1 * rng.standard_normal(c)).astype(np.float32)))


def child(args):
    pkg = graft.load_package()
    L = pkg.lib()
    assert L.vh_init(0) == 0, L.vh_last_error()
    cfg = pkg.preset("vit_b_16")
    m = pkg.ViTHip(cfg, pkg.synth_weights(cfg, 0), device=0, max_batch=MAX_BATCH, precision=args.precision)
    frame = np.random.default_rng(3).integers(0, 256, size=(FH, FW, 3), dtype=np.uint8)
    d_frame = pkg.DeviceBuffer.from_numpy(frame, dtype=np.uint8)
    desc = (d_frame.ptr.value, FH, FW, FW * 3)
    windows = pkg.tile_boxes(FH, FW, TILE, STRIDE)
    norm = pkg.pixel_norm(MEAN, STD)
    d_lab = pkg.DeviceBuffer(FH * FW, np.uint8)
    d_map = [pkg.DeviceBuffer(FH * FW) for _ in range(3)]
    lines = []
    for c in (int(x) for x in args.labels.split(",")):
        head = make_head(pkg, c)
        d_val = pkg.DeviceBuffer.from_numpy(np.linspace(0.5, 80.0, c).astype(np.float32))

        def timed(run):
            t0 = time.perf_counter()
            run()
            return (time.perf_counter() - t0) * 1e3

        calls = {
            "soft": lambda: m.segment_frame_soft_device(desc, windows, norm, head[0], head[1], values=d_val, prob=d_map[0], expect=d_map[1],
                                                        entropy=d_map[2], labels=d_lab, n_labels=c, weight_stride=E),
            "prob": lambda: m.segment_frame_soft_device(desc, windows, norm, head[0], head[1], prob=d_map[0], n_labels=c, weight_stride=E),
            "labels": lambda: m.segment_frame_device(desc, windows, norm, head[0], head[1], labels=d_lab, n_labels=c, weight_stride=E),
        }
        for run in calls.values():
            run()
        runs = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, run in calls.items():
                runs[k].append(timed(run))
        med = {k: statistics.median(v) for k, v in runs.items()}
        tag = f"vit_b_16 {args.precision:<5} {len(windows)} windows C={c:<3}"
        for k, v in runs.items():
            lines.append(f"{tag} {k:<7} {med[k]:8.2f} ms  (runs {', '.join(f'{x:.2f}' for x in v)})")
        lines.append(f"{tag} soft - labels = {med['soft'] - med['labels']:+.2f} ms, prob - labels = {med['prob'] - med['labels']:+.2f} ms")
    m.close()
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


def kernel_only(args):
    """the launchers alone, args.reps + 2 rounds, for a kernel trace or a counter run; prints the mean cover and the id count"""
    pkg = graft.load_package()
    b, L = pkg.binding, pkg.lib()
    assert L.vh_init(0) == 0, L.vh_last_error()
    c = int(args.labels)
    boxes = np.array([w[1] for w in pkg.tile_boxes(FH, FW, TILE, STRIDE)], np.float32)
    n = len(boxes)
    offsets, ids = b.stitch_index(FH, FW, boxes)
    d_pl = pkg.DeviceBuffer.from_numpy(np.random.default_rng(2).standard_normal((n, P, c)).astype(np.float32))
    d_val = pkg.DeviceBuffer.from_numpy(np.linspace(0.5, 80.0, c).astype(np.float32))
    need = L.vh_dense_stitch_scratch(n, FH, FW, len(ids))
    d_scr, d_lab, d_cov = pkg.DeviceBuffer(need // 4 + 4), pkg.DeviceBuffer(FH * FW, np.uint8), pkg.DeviceBuffer(FH * FW, np.uint8)
    d_map = [pkg.DeviceBuffer(FH * FW) for _ in range(3)]
    ip = C.POINTER(C.c_int)
    index = (b.fptr(boxes), FH, FW, offsets.ctypes.data_as(ip), ids.ctypes.data_as(ip))
    launch_as = L.vh_launch_dense_stitch_soft_as
    launch_as.restype, launch_as.argtypes = C.c_int, [C.c_int] + list(L.vh_launch_dense_stitch_soft.argtypes)
    variants = [int(args.variant)] if args.variant else [v for v in VARIANTS if c <= LIMIT[v]]
    kinds = [args.maps] if args.maps else ["all", "prob"]
    for k in range(args.reps + 2):
        if not args.variant:
            b.check(L.vh_launch_dense_stitch(None, d_pl.ptr, n, GRID[0], GRID[1], c, *index, 255, d_scr.ptr, need, d_lab.ptr, None,
                                             d_cov.ptr if k == 0 else None), "vh_launch_dense_stitch")
            b.check(L.vh_device_sync(), "sync")
            if k == 0:
                print(f"cover {d_cov.to_numpy().astype(np.float64).mean():.4f} ids {len(ids)} windows {n}", flush=True)
        for v in variants:
            for kind in kinds:
                maps = [d.ptr for d in d_map] if kind == "all" else [d_map[0].ptr, None, None]
                b.check(launch_as(v, None, d_pl.ptr, n, GRID[0], GRID[1], c, *index, d_scr.ptr, need, 1.0, d_val.ptr if kind == "all" else None,
                                  *maps), "vh_launch_dense_stitch_soft")
                b.check(L.vh_device_sync(), "sync")


def kernel_rows(args, c):
    """{(variant, maps) or "labels": (average ms, calls, best ms)} from the trace of one child, and its cover line"""
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, __file__,
                            "--kernel-only", "--labels", str(c), "--reps", str(args.reps)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
        cover = next(line for line in r.stdout.splitlines() if line.startswith("cover "))
        with open(next(Path(tmp).rglob("*kernel_stats.csv"))) as f:
            rows = list(csv.DictReader(f))
    out = {}
    for row in rows:
        t = (float(row["AverageNs"]) / 1e6, int(row["Calls"]), float(row["MinNs"]) / 1e6)
        hit = re.search(r"dense_stitch_soft_kernel<([^>]*)>", row["Name"])
        if hit:
            ex, en, stash = (a.replace("(bool)", "").replace("(int)", "").strip() for a in hit.group(1).split(","))
            out[(STASH[stash], "all" if ex in ("true", "1") and en in ("true", "1") else "prob")] = t
        elif "dense_stitch_kernel" in row["Name"]:
            out["labels"] = t
    return out, cover.split()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--labels", default="21,150")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "frame_soft_rates.txt"))
    ap.add_argument("--precision")
    ap.add_argument("--precisions", default="f32,bf16,fp8")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--variant")
    ap.add_argument("--maps", choices=["all", "prob"])
    args = ap.parse_args()
    if args.kernel_only:
        return kernel_only(args)
    if args.precision:
        return child(args)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(f"# tools/frame_soft_rates.py: a {FH} x {FW} x 3 device-resident frame tiled {TILE} / stride {STRIDE}, ViT-B/16, synthetic "
                              f"weights, max_batch {MAX_BATCH}; wall ms, median of alternating runs; the kernels from rocprofv3 --kernel-trace --stats, "
                              "all instances round-robin in one process per label count.  Floors as the tool's docstring states them\n")
    lines = []
    for c in (int(x) for x in args.labels.split(",")):
        rows, (_, cover, _, ids, _, n) = kernel_rows(args, c)
        cover, pixels = float(cover), FH * FW
        lab = rows["labels"]
        lines.append(f"labels stitch C={c:<3} {n} windows, mean cover {cover:.3f}, {ids} ids: {lab[0]:.3f} ms average of {lab[1]} launches (best {lab[2]:.3f})")
        for (v, kind), (avg, calls, best) in sorted((k, t) for k, t in rows.items() if k != "labels"):
            passes = 2 if v == 1 else 1
            valu = pixels * c * (passes * (7 * cover + 10) + (12 if kind == "all" else 7)) / LANES * 1e3
            l1 = pixels * cover * -(-c // 16) * 16 * 16 * passes / L1_BYTES * 1e3
            lines.append(f"soft stitch   C={c:<3} {VARIANTS[v]:<9} {kind:<4}: {avg:.3f} ms average of {calls} launches (best {best:.3f}) = {avg / lab[0]:.2f} x "
                         f"the labels stitch; VALU floor {valu:.3f} ms, L1 floor {l1:.3f} ms -> {max(valu, l1) / avg:.3f} of the larger")
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    for precision in filter(None, args.precisions.split(",")):
        subprocess.run([sys.executable, __file__, "--precision", precision, "--labels", args.labels, "--reps", str(args.reps), "--out", args.out],
                       check=True, timeout=900)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
