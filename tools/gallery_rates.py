#!/usr/bin/env python3
"""What an armed gallery request (vit_hip_set_gallery) costs, and the search's time against its two floors.

One child process per precision: ViT-B/16 in f32, bf16 and fp8, synthetic weights, device-resident images, at batch 512 and
at batch 8, against galleries of 10^5 and 10^6 rows of 768 stored as fp32 and as bf16 (uniform values, made once per child;
the search's work does not depend on them beyond how often a row enters a running list, which random rows fix).
Un-armed and armed steps alternate so that both see the same clocks:
  plain                 un-armed (the parent commit's launch sequence)
  <rows>/<storage>      the same forward with the device form armed: cls of the last layer, k = 5
Then the classifier operator's HIP-event time (VIT_OP_HEAD: the class GEMM, and when armed the query readout and the
search's two launches), armed minus un-armed, against
  traffic floor   gallery bytes x passes / 4 TB/s     passes = ceil(n / vh_gallery_query_tile(n))
  matrix floor    2 n E G / 157 TF                    the fp32-input matrix instruction's peak
The f32 child also times vh_launch_gallery_topk alone at k = 5 and k = 32 on gaussian queries.
Output: profiles/gallery_rates.txt (or --out)."""
from __future__ import annotations

import argparse
import ctypes as C
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as graft  # noqa: E402

E = 768
CHUNK = 100_000
HBM, MATRIX = 4.0e12, 157.0e12


def event_ms(pkg, fn, reps):
    L = pkg.lib()
    a, b = C.c_void_p(), C.c_void_p()
    assert L.vh_event_create(C.byref(a)) == 0 and L.vh_event_create(C.byref(b)) == 0
    out = []
    for _ in range(reps + 2):
        L.vh_event_record(a, None)
        fn()
        L.vh_event_record(b, None)
        assert L.vh_event_sync(b) == 0, L.vh_last_error()
        ms = C.c_float()
        L.vh_event_elapsed_ms(C.byref(ms), a, b)
        out.append(ms.value)
    L.vh_event_destroy(a)
    L.vh_event_destroy(b)
    return statistics.median(out[2:])


def make_galleries(pkg, rows_max):
    """rows_max rows of uniform [-0.5, 0.5) / sqrt(E / 12) values (unit length on average), as fp32 and as the same values
    rounded to bf16; smaller galleries are prefixes"""
    L = pkg.lib()
    d_f32, d_bf16 = pkg.DeviceBuffer(rows_max * E), pkg.DeviceBuffer(rows_max * E, np.uint16)
    rng = np.random.default_rng(1)
    for first in range(0, rows_max, CHUNK):
        m = min(CHUNK, rows_max - first)
        a = (rng.random((m, E), dtype=np.float32) - np.float32(0.5)) * np.float32((12.0 / E) ** 0.5)
        bits = a.view(np.uint32)
        h = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)
        assert L.vh_h2d(C.c_void_p(d_f32.ptr.value + 4 * first * E), a.ctypes.data_as(C.c_void_p), a.nbytes, None) == 0
        assert L.vh_h2d(C.c_void_p(d_bf16.ptr.value + 2 * first * E), h.ctypes.data_as(C.c_void_p), h.nbytes, None) == 0
        assert L.vh_device_sync() == 0
    return {"f32": d_f32, "bf16": d_bf16}


def child(args):
    pkg = graft.load_package()
    b, L = pkg.binding, pkg.lib()
    assert L.vh_init(0) == 0, L.vh_last_error()
    cfg = pkg.preset("vit_b_16")
    weights = pkg.synth_weights(cfg, 0)
    sizes = [int(g) for g in args.rows.split(",")]
    galleries = make_galleries(pkg, max(sizes))
    variants = [(g, dt) for g in sizes for dt in ("f32", "bf16")]
    lines = []
    for n in (int(x) for x in args.batches.split(",")):
        steps = args.steps if n >= 64 else args.steps * 8
        m = pkg.ViTHip(cfg, weights, device=0, max_batch=n, precision=args.precision)
        d_img = pkg.DeviceBuffer.from_numpy(pkg.synth_images(cfg, 0, n))
        d_log, d_prob = pkg.DeviceBuffer(n * cfg.num_classes), pkg.DeviceBuffer(n * cfg.num_classes)
        d_idx, d_sc = pkg.DeviceBuffer(n * 32, np.int32), pkg.DeviceBuffer(n * 32)
        qt = L.vh_gallery_query_tile(n)
        passes = -(-n // qt)

        def arm(which, k=5):
            if which == "plain":
                return m.set_gallery(None)
            g, dt = which
            m.set_gallery(b.GallerySpec(k, "cls", -1, True, True, dt, g, E), galleries[dt], indices=d_idx, scores=d_sc)

        def step(which):
            arm(which)
            t0 = time.perf_counter()
            for _ in range(steps):
                m.forward_device(d_img.ptr, n, d_log.ptr, d_prob.ptr, None)
            m.sync()
            return n * steps / (time.perf_counter() - t0)

        def head_ms(which):
            arm(which)
            m.profile_enable(args.reps + 1)
            for _ in range(args.reps + 1):
                m.forward_device(d_img.ptr, n, d_log.ptr, d_prob.ptr, None)
            m.sync()
            ms, count = m.profile_read()["head_gemm"]
            m.profile_enable(0)
            return ms / (args.reps + 1), count // (args.reps + 1)

        order = [w for v in variants for w in ("plain", v)]
        for w in order[:2]:
            step(w)
        rates = {w: [] for w in ["plain"] + variants}
        for _ in range(args.reps):
            for w in order:
                rates[w].append(step(w))
        med = {w: statistics.median(v) for w, v in rates.items()}
        tag = f"vit_b_16 {args.precision:<5} batch {n:<3}"
        name = lambda w: "plain" if w == "plain" else f"{w[0]:>7}/{w[1]:<4}"
        for w in rates:
            lines.append(f"{tag} {name(w):<13} {med[w]:9.1f} img/s  (runs {', '.join(f'{x:.0f}' for x in rates[w])})")
        lines.append(f"{tag} armed/un-armed: " + "  ".join(f"{name(v)} {med[v] / med['plain']:.4f}" for v in variants))
        base, _ = head_ms("plain")
        for g, dt in variants:
            ms, launches = head_ms((g, dt))
            took = ms - base
            traffic = g * E * (4 if dt == "f32" else 2) * passes / HBM * 1e3
            matrix = 2.0 * n * E * g / MATRIX * 1e3
            bind = "traffic" if traffic > matrix else "matrix"
            lines.append(f"{tag} {name((g, dt))} head operator {base:.3f} ms un-armed ({launches} launches armed), + {took:.3f} ms: "
                         f"splits {L.vh_gallery_splits(n, g)}, {passes} pass(es) of {qt} queries; traffic floor {traffic:.3f} ms, "
                         f"matrix floor {matrix:.3f} ms -> {max(traffic, matrix) / took:.3f} of the {bind} floor")
        if args.precision == "f32":   # the launcher alone, on gaussian queries of unit length
            d_q = pkg.DeviceBuffer.from_numpy(np.random.default_rng(2).standard_normal((n, E)).astype(np.float32) / np.float32(E ** 0.5))
            d_ws = pkg.DeviceBuffer(L.vh_gallery_workspace(n, max(sizes), 32, 0) // 4)
            for g, dt in variants:
                for k in (5, 32):
                    t = event_ms(pkg, lambda: b.check(L.vh_launch_gallery_topk(None, d_q.ptr, n, E, galleries[dt].ptr, b.GALLERY_DTYPES[dt],
                                                                               g, E, k, 0, d_ws.ptr, d_idx.ptr, d_sc.ptr), "gallery"),
                                 args.reps * 2)
                    lines.append(f"{tag} {name((g, dt))} vh_launch_gallery_topk alone, gaussian queries, k={k:<2} {t:.3f} ms")
        arm("plain")
        m.close()
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", default="512,8")
    ap.add_argument("--rows", default="100000,1000000")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gallery_rates.txt"))
    ap.add_argument("--precision")
    ap.add_argument("--precisions", default="f32,bf16,fp8")
    args = ap.parse_args()
    if args.precision:
        return child(args)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("# tools/gallery_rates.py: synthetic weights, device-resident images, images/s median of alternating un-armed / "
                              "armed runs (cls of the last layer, k = 5); search time from the head operator's HIP events, armed minus un-armed\n")
    for precision in args.precisions.split(","):
        subprocess.run([sys.executable, __file__, "--precision", precision, "--batches", args.batches, "--rows", args.rows,
                        "--steps", str(args.steps), "--reps", str(args.reps), "--out", args.out], check=True, timeout=900)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
