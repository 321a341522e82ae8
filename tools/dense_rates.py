#!/usr/bin/env python3
"""What an armed dense request (vit_hip_set_dense) costs, and its two kernels' times against their floors.

One child process per precision: ViT-B/16 in f32, bf16 and fp8, synthetic weights, device-resident images, at batch 512 and
at batch 8, heads of 21 and of 150 labels (gaussian rows, with bias), 224 x 224 labels from the last layer's normalised
tokens.  Un-armed and armed steps alternate so that both see the same clocks:
  plain       un-armed (the parent commit's launch sequence)
  C=<labels>  the same forward with the device form armed, labels only
Then the classifier operator's HIP-event time (VIT_OP_HEAD: the class GEMM, and when armed the token readout and the two
dense launches), armed minus un-armed.  The f32 child also times each launcher alone on gaussian tokens, against
  logits   matrix floor  2 M E C16 / 157 TF   (M = n * 196 token rows, C16 = C rounded up to 16: the instruction's tile)
           traffic floor (M E + M C + C E) * 4 bytes / 4 TB/s
  labels   VALU floor    pixels * C * 5.25 lane-operations / (256 CUs * 128 lanes * 2.4 GHz)   (DESIGN.md derives the 5.25)
           LDS floor     pixels * C / 16 * 4 ds_read_b32 lanes, 2 cycles per 64 of them, per CU at 2.4 GHz
           traffic floor (pixels + M C * 4) bytes / 4 TB/s
Output: profiles/dense_rates.txt (or --out)."""
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

E, P, GRID, OUT = 768, 196, 14, 224
HBM, MATRIX = 4.0e12, 157.0e12
LANES = 256 * 128 * 2.4e9       # VALU lane-operations per second: 256 CUs x 4 SIMDs x 32 lanes per cycle
CU_HZ = 256 * 2.4e9


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


def child(args):
    pkg = graft.load_package()
    b, L = pkg.binding, pkg.lib()
    assert L.vh_init(0) == 0, L.vh_last_error()
    cfg = pkg.preset("vit_b_16")
    weights = pkg.synth_weights(cfg, 0)
    labels = [int(c) for c in args.labels.split(",")]
    rng = np.random.default_rng(1)
    heads = {c: (pkg.DeviceBuffer.from_numpy((rng.standard_normal((c, E)) / np.sqrt(E)).astype(np.float32)),
                 pkg.DeviceBuffer.from_numpy((0.1 * rng.standard_normal(c)).astype(np.float32))) for c in labels}
    lines = []
    for n in (int(x) for x in args.batches.split(",")):
        steps = args.steps if n >= 64 else args.steps * 8
        m = pkg.ViTHip(cfg, weights, device=0, max_batch=n, precision=args.precision)
        d_img = pkg.DeviceBuffer.from_numpy(pkg.synth_images(cfg, 0, n))
        d_log, d_prob = pkg.DeviceBuffer(n * cfg.num_classes), pkg.DeviceBuffer(n * cfg.num_classes)
        d_lab = pkg.DeviceBuffer(n * OUT * OUT, np.uint8)

        def arm(which):
            if which == "plain":
                return m.set_dense(None)
            m.set_dense(b.DenseSpec(which, 0, 0, -1, True, E), heads[which][0], heads[which][1], labels=d_lab)

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

        order = [w for c in labels for w in ("plain", c)]
        for w in order[:2]:
            step(w)
        rates = {w: [] for w in ["plain"] + labels}
        for _ in range(args.reps):
            for w in order:
                rates[w].append(step(w))
        med = {w: statistics.median(v) for w, v in rates.items()}
        tag = f"vit_b_16 {args.precision:<5} batch {n:<3}"
        name = lambda w: "plain" if w == "plain" else f"C={w}"
        for w in rates:
            spread = (max(rates[w]) - min(rates[w])) / med[w]
            lines.append(f"{tag} {name(w):<6} {med[w]:9.1f} img/s  spread {100 * spread:.2f} %  (runs {', '.join(f'{x:.0f}' for x in rates[w])})")
        lines.append(f"{tag} armed/un-armed: " + "  ".join(f"{name(c)} {med[c] / med['plain']:.4f}" for c in labels))
        base, _ = head_ms("plain")
        for c in labels:
            ms, launches = head_ms(c)
            lines.append(f"{tag} {name(c):<6} head operator {base:.3f} ms un-armed ({launches} launches armed), + {ms - base:.3f} ms")
        if args.precision == "f32":   # the launchers alone, on gaussian tokens
            M, pixels = n * P, n * OUT * OUT
            d_tok = pkg.DeviceBuffer.from_numpy(np.random.default_rng(2).standard_normal((M, E)).astype(np.float32))
            d_sc = pkg.DeviceBuffer(pixels)
            for c in labels:
                d_pl = pkg.DeviceBuffer(M * c)
                t = event_ms(pkg, lambda: b.check(L.vh_launch_dense_logits(None, d_tok.ptr, P * E, E, n, P, E, heads[c][0].ptr, E,
                                                                           heads[c][1].ptr, c, d_pl.ptr), "logits"), args.reps * 2)
                c16 = -(-c // 16) * 16
                matrix, traffic = 2.0 * M * E * c16 / MATRIX * 1e3, (M * E + M * c + c * E) * 4 / HBM * 1e3
                bind = "traffic" if traffic > matrix else "matrix"
                lines.append(f"{tag} {name(c):<6} vh_launch_dense_logits alone {t:.3f} ms: matrix floor {matrix:.3f} ms, traffic floor "
                             f"{traffic:.3f} ms -> {max(matrix, traffic) / t:.3f} of the {bind} floor")
                for what, sc in (("labels", None), ("labels + scores", d_sc.ptr)):
                    t = event_ms(pkg, lambda: b.check(L.vh_launch_dense_labels(None, d_pl.ptr, n, GRID, GRID, c, OUT, OUT, d_lab.ptr, sc),
                                                      "labels"), args.reps * 2)
                    valu, lds = pixels * c * 5.25 / LANES * 1e3, pixels * c / 16 * 4 / 64 * 2 / CU_HZ * 1e3
                    traffic = (pixels * (5 if sc else 1) + M * c * 4) / HBM * 1e3
                    lines.append(f"{tag} {name(c):<6} vh_launch_dense_labels alone ({what}) {t:.3f} ms: VALU floor {valu:.3f} ms, LDS floor "
                                 f"{lds:.3f} ms, traffic floor {traffic:.3f} ms -> {max(valu, lds, traffic) / t:.3f} of the largest")
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
    ap.add_argument("--labels", default="21,150")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "dense_rates.txt"))
    ap.add_argument("--precision")
    ap.add_argument("--precisions", default="f32,bf16,fp8")
    args = ap.parse_args()
    if args.precision:
        return child(args)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("# tools/dense_rates.py: synthetic weights, device-resident images, images/s median of alternating un-armed / "
                              "armed runs (224 x 224 labels from the last layer's normalised tokens); dense time from the head operator's "
                              "HIP events, armed minus un-armed\n")
    for precision in args.precisions.split(","):
        subprocess.run([sys.executable, __file__, "--precision", precision, "--batches", args.batches, "--labels", args.labels,
                        "--steps", str(args.steps), "--reps", str(args.reps), "--out", args.out], check=True, timeout=900)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
