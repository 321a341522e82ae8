#!/usr/bin/env python3
"""What the soft maps of the dense head (vit_hip_set_dense_soft) cost, and the soft kernel's time against its floor.

One child process per precision: ViT-B/16 in f32, bf16 and fp8, synthetic weights, device-resident images, at batch 512 and
at batch 8, heads of 21 and of 150 labels (gaussian rows, with bias), 224 x 224 maps from the last layer's normalised
tokens.  Un-armed and armed steps alternate so that both see the same clocks:
  plain         un-armed (the parent commit's launch sequence)
  dense C=<..>  the same forward with vit_hip_set_dense armed, labels only (what the parent commit offers: it already makes the
                forward run its last layer on all rows)
  soft C=<..>   the same forward soft-armed: labels, prob, expect and entropy
Then, in the f32 child, each launcher alone on the patch logits of gaussian tokens, in one session: vh_launch_dense_labels
(labels only) and vh_launch_dense_soft per output set, against the soft kernel's own floor
  VALU + transcendental   pixels * C * ops lane-operations / (256 CUs * 128 lanes * 2.4 GHz), a v_exp_f32 counted as two
                          (its issue cost is twice a plain instruction's): pass 1 is mul, fma, max (3) and pass 2 mul, fma,
                          sub, mul, exp, add (5 + 2), each pass 4 / 16 for the horizontal lerps shared by 16 rows: 10.5 for
                          prob; expect adds one fma, entropy a max and an fma: 13.5 for all three
  LDS                     pixels * C / 16 * 8 ds_read_b32 lanes (two passes), 2 cycles per 64 of them, per CU at 2.4 GHz
  traffic                 (maps * pixels * 4 + M C * 4) bytes / 4 TB/s
Output: profiles/dense_soft_rates.txt (or --out)."""
from __future__ import annotations

import argparse
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import __graft_entry__ as graft  # noqa: E402
from dense_rates import CU_HZ, GRID, HBM, LANES, OUT, E, P, event_ms  # noqa: E402

SETS = {"prob": (1, 0, 0), "expect": (0, 1, 0), "entropy": (0, 0, 1), "prob + expect + entropy": (1, 1, 1)}
OPS = {"prob": 10.5, "expect": 11.5, "entropy": 12.5, "prob + expect + entropy": 13.5}


def child(args):
    pkg = graft.load_package()
    b, L = pkg.binding, pkg.lib()
    assert L.vh_init(0) == 0, L.vh_last_error()
    cfg = pkg.preset("vit_b_16")
    weights = pkg.synth_weights(cfg, 0)
    labels = [int(c) for c in args.labels.split(",")]
    rng = np.random.default_rng(1)
    heads = {c: (pkg.DeviceBuffer.from_numpy((rng.standard_normal((c, E)) / np.sqrt(E)).astype(np.float32)),
                 pkg.DeviceBuffer.from_numpy((0.1 * rng.standard_normal(c)).astype(np.float32)),
                 pkg.DeviceBuffer.from_numpy(np.linspace(0.5, 10.0, c).astype(np.float32))) for c in labels}
    lines = []
    for n in (int(x) for x in args.batches.split(",")):
        steps = args.steps if n >= 64 else args.steps * 8
        m = pkg.ViTHip(cfg, weights, device=0, max_batch=n, precision=args.precision)
        d_img = pkg.DeviceBuffer.from_numpy(pkg.synth_images(cfg, 0, n))
        d_log, d_prob = pkg.DeviceBuffer(n * cfg.num_classes), pkg.DeviceBuffer(n * cfg.num_classes)
        d_lab = pkg.DeviceBuffer(n * OUT * OUT, np.uint8)
        d_maps = [pkg.DeviceBuffer(n * OUT * OUT) for _ in range(3)]

        def arm(which):
            if which == "plain":
                return m.set_dense_soft(None)
            kind, c = which
            w, bias, centres = heads[c]
            if kind == "dense":
                return m.set_dense(b.DenseSpec(c, 0, 0, -1, True, E), w, bias, labels=d_lab)
            m.set_dense_soft(b.DenseSpec(c, 0, 0, -1, True, E), w, bias, 1.0, centres, labels=d_lab, prob=d_maps[0], expect=d_maps[1],
                             entropy=d_maps[2])

        def step(which):
            arm(which)
            t0 = time.perf_counter()
            for _ in range(steps):
                m.forward_device(d_img.ptr, n, d_log.ptr, d_prob.ptr, None)
            m.sync()
            return n * steps / (time.perf_counter() - t0)

        order = [w for c in labels for w in ("plain", ("dense", c), ("soft", c))]
        for w in order[:3]:
            step(w)
        rates = {w: [] for w in dict.fromkeys(order)}
        for _ in range(args.reps):
            for w in order:
                rates[w].append(step(w))
        med = {w: statistics.median(v) for w, v in rates.items()}
        tag = f"vit_b_16 {args.precision:<5} batch {n:<3}"
        name = lambda w: "plain" if w == "plain" else f"C={w}" if isinstance(w, int) else f"{w[0]} C={w[1]}"
        for w in rates:
            spread = (max(rates[w]) - min(rates[w])) / med[w]
            lines.append(f"{tag} {name(w):<11} {med[w]:9.1f} img/s  spread {100 * spread:.2f} %  (runs {', '.join(f'{x:.0f}' for x in rates[w])})")
        lines.append(f"{tag} soft-armed (labels + three maps) / un-armed: " + "  ".join(f"C={c} {med[('soft', c)] / med['plain']:.4f}" for c in labels))
        lines.append(f"{tag} soft-armed / dense-armed (labels only): " + "  ".join(f"C={c} {med[('soft', c)] / med[('dense', c)]:.4f}" for c in labels))
        if args.precision == "f32":   # the launchers alone, on the patch logits of gaussian tokens
            M, pixels = n * P, n * OUT * OUT
            d_tok = pkg.DeviceBuffer.from_numpy(np.random.default_rng(2).standard_normal((M, E)).astype(np.float32))
            for c in labels:
                d_pl = pkg.DeviceBuffer(M * c)
                b.check(L.vh_launch_dense_logits(None, d_tok.ptr, P * E, E, n, P, E, heads[c][0].ptr, E, heads[c][1].ptr, c, d_pl.ptr), "logits")
                t = event_ms(pkg, lambda: b.check(L.vh_launch_dense_labels(None, d_pl.ptr, n, GRID, GRID, c, OUT, OUT, d_lab.ptr, None), "labels"),
                             args.reps * 2)
                lines.append(f"{tag} {name(c):<6} vh_launch_dense_labels alone (labels) {t:.3f} ms")
                for what, (wp, wx, wh) in SETS.items():
                    t = event_ms(pkg, lambda: b.check(L.vh_launch_dense_soft(None, d_pl.ptr, n, GRID, GRID, c, OUT, OUT, 1.0,
                                                                             heads[c][2].ptr if wx else None, d_maps[0].ptr if wp else None,
                                                                             d_maps[1].ptr if wx else None, d_maps[2].ptr if wh else None), "soft"),
                                 args.reps * 2)
                    valu, lds = pixels * c * OPS[what] / LANES * 1e3, pixels * c / 16 * 8 / 64 * 2 / CU_HZ * 1e3
                    traffic = ((wp + wx + wh) * pixels * 4 + M * c * 4) / HBM * 1e3
                    lines.append(f"{tag} {name(c):<6} vh_launch_dense_soft alone ({what}) {t:.3f} ms: VALU + transcendental floor {valu:.3f} ms, "
                                 f"LDS floor {lds:.3f} ms, traffic floor {traffic:.3f} ms -> {max(valu, lds, traffic) / t:.3f} of the largest")
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "dense_soft_rates.txt"))
    ap.add_argument("--precision")
    ap.add_argument("--precisions", default="f32,bf16,fp8")
    args = ap.parse_args()
    if args.precision:
        return child(args)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("# tools/dense_soft_rates.py: synthetic weights, device-resident images, images/s median of alternating un-armed / "
                              "soft-armed runs (224 x 224 labels, prob, expect and entropy from the last layer's normalised tokens); the "
                              "launchers alone from HIP events, in the f32 child\n")
    for precision in args.precisions.split(","):
        subprocess.run([sys.executable, __file__, "--precision", precision, "--batches", args.batches, "--labels", args.labels,
                        "--steps", str(args.steps), "--reps", str(args.reps), "--out", args.out], check=True, timeout=900)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
