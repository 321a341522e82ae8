#!/usr/bin/env python3
"""What an armed top-k request (vit_hip_set_topk) costs, and the selection kernel's time beside the class softmax's.

One child process per precision: ViT-B/16 at batch 512 in f32, bf16 and fp8, synthetic weights, device-resident images.
Un-armed and armed steps alternate so that both see the same clocks:
  plain   un-armed (the parent commit's launch sequence: logits + probabilities)
  k1, k5, k32   the same forward with the device form armed for k = 1, 5, 32 (probability scores)
Then, in the same process, HIP-event times of vh_launch_topk (k = 1, 5, 32, both score kinds) and of vh_launch_softmax on
the same [batch][1000] logits, and of vh_launch_topk on [batch][21843] rows (the rescan path; the softmax does not take
them).  The f32 child also times the host forms: vit_hip_forward with logits and probabilities against the same call with
neither and the host top-k request armed (k = 5).
Output: profiles/topk_rates.txt (or --out)."""
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

KS = (1, 5, 32)


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
    n, nc = args.batch, cfg.num_classes
    m = pkg.ViTHip(cfg, pkg.synth_weights(cfg, 0), device=0, max_batch=n, precision=args.precision)
    images = pkg.synth_images(cfg, 0, n)
    d_img = pkg.DeviceBuffer.from_numpy(images)
    d_log, d_prob = pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)
    d_lab, d_sc = pkg.DeviceBuffer(n * 32, np.int32), pkg.DeviceBuffer(n * 32)

    def step(which):
        m.set_topk(None) if which == "plain" else m.set_topk(b.TopKSpec(int(which[1:])), labels=d_lab, scores=d_sc)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            m.forward_device(d_img.ptr, n, d_log.ptr, d_prob.ptr, None)
        m.sync()
        return n * args.steps / (time.perf_counter() - t0)

    order = [w for k in KS for w in ("plain", f"k{k}")]
    for w in order[:2]:
        step(w)
    rates = {w: [] for w in ["plain"] + [f"k{k}" for k in KS]}
    for _ in range(args.reps):
        for w in order:
            rates[w].append(step(w))
    m.set_topk(None)
    med = {w: statistics.median(v) for w, v in rates.items()}
    tag = f"vit_b_16 {args.precision:<5} batch {n}"
    lines = [f"{tag} {w:<5} {med[w]:9.1f} img/s  (runs {', '.join(f'{x:.0f}' for x in rates[w])})" for w in rates]
    lines.append(f"{tag} armed/un-armed: " + "  ".join(f"k={k} {med[f'k{k}'] / med['plain']:.4f}" for k in KS))

    # the kernels alone, on the logits the last forward left
    reps = args.reps * 5
    t_sm = event_ms(pkg, lambda: b.check(L.vh_launch_softmax(None, d_log.ptr, d_prob.ptr, n, nc), "softmax"), reps)
    lines.append(f"{tag} softmax_kernel [{n}][{nc}] {1e3 * t_sm:.1f} us")
    for k in KS:
        for kind, name in ((0, "probs"), (1, "logits")):
            t = event_ms(pkg, lambda: b.check(L.vh_launch_topk(None, d_log.ptr, n, nc, k, kind, d_lab.ptr, d_sc.ptr), "topk"), reps)
            lines.append(f"{tag} topk_kernel    [{n}][{nc}] k={k:<2} {name:<6} {1e3 * t:.1f} us  = {t / t_sm:.2f} x softmax_kernel")
    if args.precision == "f32":
        wide = 21843
        row = np.empty(n * wide, np.float32)
        L.vit_synth_fill(b.fptr(row), row.size, 9, 4.0, 0.0)
        d_wide = pkg.DeviceBuffer.from_numpy(row)
        for k in KS:
            t = event_ms(pkg, lambda: b.check(L.vh_launch_topk(None, d_wide.ptr, n, wide, k, 0, d_lab.ptr, d_sc.ptr), "topk"), reps)
            lines.append(f"{tag} topk_kernel    [{n}][{wide}] k={k:<2} probs  {1e3 * t:.1f} us  ({n * wide * 4 / 1e6:.1f} MB of logits, re-read every round)")
        # host forms: everything through vit_hip_forward's pipeline, 2 x batch images = two chunks
        both = np.concatenate([images, images])
        host = {"logits+probs": [], "top-5 only": []}
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            m.forward(both)
            host["logits+probs"].append(2 * n / (time.perf_counter() - t0))
            t0 = time.perf_counter()
            m.classify(both, k=5)
            host["top-5 only"].append(2 * n / (time.perf_counter() - t0))
        for w, v in host.items():
            lines.append(f"{tag} host form, {w:<12} {statistics.median(v[1:]):9.1f} img/s  (runs {', '.join(f'{x:.0f}' for x in v[1:])})")
    m.close()
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "topk_rates.txt"))
    ap.add_argument("--precision")
    ap.add_argument("--precisions", default="f32,bf16,fp8")
    args = ap.parse_args()
    if args.precision:
        return child(args)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("# tools/topk_rates.py: synthetic weights, device-resident images, images/s median of alternating un-armed / "
                              "armed runs; kernel times from HIP events (median)\n")
    for precision in args.precisions.split(","):
        subprocess.run([sys.executable, __file__, "--precision", precision, "--batch", str(args.batch), "--steps", str(args.steps),
                        "--reps", str(args.reps), "--out", args.out], check=True, timeout=600)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
