#!/usr/bin/env python3
"""What an armed feature request (vit_hip_set_features) costs, and the readout kernel's rate beside the LayerNorm's.

One child process per (preset, precision): ViT-B/16 at batch 512 in f32, bf16 and fp8, and vit_b_16_384 at batch 256 in f32.
Device-resident images; un-armed and armed steps alternate so that both see the same clocks:
  plain   un-armed (the parent commit's launch sequence)
  a       last layer, cls + pooled
  b       four taps, cls + pooled
  c       last layer, cls + pooled + bf16 NCHW tokens
Then, in the same process, HIP-event times of vh_launch_feature_readout (cls + pooled; and with bf16 NCHW tokens) and of
vh_launch_layer_norm_p3 (layernorm_p3_kernel: the same read pattern) on one residual stream [batch * T][E], as bytes read +
written per second.  The share line states what (a) may cost by the issue's rule: twice bytes / the LayerNorm's rate.
Output: profiles/feature_rates.txt (or --out)."""
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
    cfg = pkg.preset(args.preset)
    n, E, T, nc = args.batch, cfg.embed_dim, b.tokens(cfg), cfg.num_classes
    m = pkg.ViTHip(cfg, pkg.synth_weights(cfg, 0), device=0, max_batch=n, precision=args.precision)
    d_img = pkg.DeviceBuffer.from_numpy(pkg.synth_images(cfg, 0, n))
    d_log, d_prob = pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)
    specs = {"a": b.FeatureSpec(taps=(-1,)), "b": b.FeatureSpec(taps=(2, 5, 8, -1)),
             "c": b.FeatureSpec(taps=(-1,), dtype="bf16", token_layout="nchw")}
    bufs = {}
    for k, s in specs.items():
        c_el, p_el, t_el = b.feature_sizes(cfg, s)
        bufs[k] = dict(cls=pkg.DeviceBuffer(n * c_el, s.np_dtype), pooled=pkg.DeviceBuffer(n * p_el, s.np_dtype))
        if k == "c":
            bufs[k]["tokens"] = pkg.DeviceBuffer(n * t_el, s.np_dtype)

    def step(which):
        m.set_features(specs[which], **bufs[which]) if which != "plain" else m.set_features(None)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            m.forward_device(d_img.ptr, n, d_log.ptr, d_prob.ptr, None)
        m.sync()
        return n * args.steps / (time.perf_counter() - t0)

    order = ["plain", "a", "plain", "b", "plain", "c"]
    for w in order[:2]:
        step(w)
    rates = {k: [] for k in ("plain", "a", "b", "c")}
    for _ in range(args.reps):
        for w in order:
            rates[w].append(step(w))
    m.set_features(None)
    med = {k: statistics.median(v) for k, v in rates.items()}
    tag = f"{args.preset} {args.precision:<5} batch {n}"
    lines = [f"{tag} {k:<5} {med[k]:9.1f} img/s  (runs {', '.join(f'{x:.0f}' for x in rates[k])})" for k in rates]
    lines.append(f"{tag} armed/un-armed: " + "  ".join(f"{k} {med[k] / med['plain']:.4f}" for k in "abc"))

    # the kernels alone on one residual stream
    rows = n * T
    d_x = pkg.DeviceBuffer.from_numpy(np.random.default_rng(0).standard_normal((rows, E), dtype=np.float32))
    g, be = L.vit_hip_weight(m.ctx, 4 + 12 * cfg.depth), L.vit_hip_weight(m.ctx, 5 + 12 * cfg.depth)
    d_planes = pkg.DeviceBuffer(rows * E * 6 // 4 + 64)
    sb = L.vh_feature_readout_scratch(n, T, E)
    d_s = pkg.DeviceBuffer(sb // 4 + 4)
    o = bufs["c"]

    def readout(tokens):
        return lambda: b.check(L.vh_launch_feature_readout(None, d_x.ptr, None, 0, g, be, cfg.eps, 1, 0, 1 if tokens else 0,
                                                           1, n, T, E, 0, 1, o["cls"].ptr if tokens else bufs["a"]["cls"].ptr,
                                                           o["pooled"].ptr if tokens else bufs["a"]["pooled"].ptr,
                                                           o["tokens"].ptr if tokens else None, d_s.ptr, sb), "readout")

    ln = lambda: b.check(L.vh_launch_layer_norm_p3(None, d_x.ptr, g, be, d_planes.ptr, rows, E, E, cfg.eps), "layer_norm_p3")
    read = rows * E * 4
    t_ln, t_a, t_c = event_ms(pkg, ln, args.reps * 3), event_ms(pkg, readout(False), args.reps * 3), event_ms(pkg, readout(True), args.reps * 3)
    bw = lambda bytes_, ms: bytes_ / (ms * 1e-3) / 1e12
    w_a, w_c = 2 * n * E * 4 + sb, 2 * n * E * 2 + sb + n * (T - 1) * E * 2
    lines.append(f"{tag} layernorm_p3 {t_ln:.4f} ms  {bw(read + rows * E * 6, t_ln):.2f} TB/s (reads {read / 1e6:.0f} MB, writes {rows * E * 6 / 1e6:.0f} MB)")
    lines.append(f"{tag} readout cls+pooled {t_a:.4f} ms  {bw(read + w_a, t_a):.2f} TB/s (three launches; reads {read / 1e6:.0f} MB)")
    lines.append(f"{tag} readout cls+pooled+bf16 NCHW tokens {t_c:.4f} ms  {bw(read + w_c, t_c):.2f} TB/s (writes {w_c / 1e6:.0f} MB)")
    step_ms = 1e3 * n / med["plain"]
    allowed = 2 * (read + w_a) / (bw(read + rows * E * 6, t_ln) * 1e12) * 1e3 / step_ms
    lines.append(f"{tag} (a): loss {1 - med['a'] / med['plain']:.5f} of a step of {step_ms:.2f} ms; allowed (2 x bytes / LayerNorm rate) {allowed:.5f}")
    m.close()
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "feature_rates.txt"))
    ap.add_argument("--preset")
    ap.add_argument("--precision")
    ap.add_argument("--batch", type=int)
    ap.add_argument("--cases", default="vit_b_16:f32:512,vit_b_16:bf16:512,vit_b_16:fp8:512,vit_b_16_384:f32:256")
    args = ap.parse_args()
    if args.preset:
        return child(args)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("# tools/feature_rates.py: synthetic weights, device-resident images, images/s median of alternating un-armed / "
                              "armed runs; kernel times from HIP events, bytes read + written per second\n")
    for case in args.cases.split(","):
        preset, precision, batch = case.split(":")
        subprocess.run([sys.executable, __file__, "--preset", preset, "--precision", precision, "--batch", batch, "--steps", str(args.steps),
                        "--reps", str(args.reps), "--out", args.out], check=True, timeout=900)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
