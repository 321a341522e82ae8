#!/usr/bin/env python3
"""Rates of the higher-resolution presets (attention_long.hip, T > 512) next to the 224 px preset, and the same-process A/B
of attention_long.hip against the streaming kernel (attention_tiled.hip) at T = 485, where both run.

Synthetic weights, device-resident inputs (vit_hip_forward_device).  Per (preset, precision, batch): images/s over timed
steps after a warm-up, then one profiled pass of the same steps for attention's ms per step, its TFLOP/s (4 T^2 E per layer
and image: Q.K^T and P.V), and attention's share of the step time next to its share of the FLOPs.

    python tools/long_seq_rates.py --section b16_384     # also: h14_518, b16_224, ab
Sections are separate so that a caller can put each under its own time limit.  Output: profiles/long_seq_rates.txt.
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as graft  # noqa: E402

SECTIONS = {   # name: (preset, img_size override or None, batches)
    "b16_384": ("vit_b_16_384", None, (64, 256)),
    "h14_518": ("vit_h_14_518", None, (32, 64)),
    "b16_224": ("vit_b_16", None, (64, 256)),
    "ab": ("vit_b_16", 352, (64,)),
}


def flops_per_image(cfg, T):
    E, F, D, P, C = cfg.embed_dim, cfg.mlp_hidden, cfg.depth, cfg.patch_size, cfg.in_chans
    attn = D * 4.0 * T * T * E
    gemm = D * 2.0 * T * (4 * E * E + 2 * E * F) + 2.0 * (T - 1) * E * C * P * P + 2.0 * E * cfg.num_classes
    return attn + gemm, attn


def measure(pkg, cfg, weights, precision, batch, warmup, steps):
    T = pkg.binding.tokens(cfg)
    m = pkg.ViTHip(cfg, weights, device=0, max_batch=batch, precision=precision)
    d_img = pkg.DeviceBuffer.from_numpy(pkg.synth_images(cfg, 0, batch))
    d_log = pkg.DeviceBuffer(batch * cfg.num_classes)
    d_prob = pkg.DeviceBuffer(batch * cfg.num_classes)
    run = lambda: m.forward_device(d_img.ptr, batch, d_log.ptr, d_prob.ptr, None)   # noqa: E731
    for _ in range(warmup):
        run()
    m.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        run()
    m.sync()
    step_s = (time.perf_counter() - t0) / steps
    m.profile_enable(steps)
    m.profile_select(None)
    for _ in range(steps):
        run()
    m.sync()
    prof = m.profile_read()
    logits = d_log.to_numpy()
    m.close()
    for d in (d_img, d_log, d_prob):
        d.free()
    assert np.isfinite(logits).all()
    total_ms = sum(v[0] for v in prof.values()) / steps
    attn_ms = prof["attention"][0] / steps
    f_all, f_attn = flops_per_image(cfg, T)
    return {
        "T": T, "img_s": batch / step_s, "step_ms": step_s * 1e3, "attn_ms": attn_ms,
        "attn_tf": f_attn * batch / (attn_ms * 1e-3) / 1e12 if attn_ms > 0 else float("nan"),
        "time_share": attn_ms / total_ms, "flop_share": f_attn / f_all,
    }


def line(tag, precision, batch, r):
    ratio = r["time_share"] / r["flop_share"]
    return (f"{tag:<16} {precision:<5} B={batch:<4} T={r['T']:<5} {r['img_s']:9.1f} img/s  step {r['step_ms']:8.2f} ms  "
            f"attention {r['attn_ms']:7.3f} ms {r['attn_tf']:7.1f} TF/s  time share {100 * r['time_share']:5.1f} %  "
            f"FLOP share {100 * r['flop_share']:5.1f} %  (time/FLOP {ratio:4.2f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", choices=sorted(SECTIONS), required=True)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    pkg = graft.load_package()
    assert pkg.lib().vh_init(0) == 0
    preset, img, batches = SECTIONS[args.section]
    cfg = pkg.preset(preset)
    if img:
        cfg.img_size = img
    weights = pkg.synth_weights(cfg, 0)
    tag = preset if not img else f"{preset}@{img}"
    for precision in ("f32", "bf16", "fp8"):
        for batch in batches:
            if args.section != "ab":
                print(line(tag, precision, batch, measure(pkg, cfg, weights, precision, batch, args.warmup, args.steps)), flush=True)
                continue
            os.environ.pop("VIT_HIP_ATTN", None)
            tiled = measure(pkg, cfg, weights, precision, batch, args.warmup, args.steps)
            os.environ["VIT_HIP_ATTN"] = "long"
            long_ = measure(pkg, cfg, weights, precision, batch, args.warmup, args.steps)
            os.environ.pop("VIT_HIP_ATTN", None)
            print(line(tag + " tiled", precision, batch, tiled), flush=True)
            print(line(tag + " long", precision, batch, long_), flush=True)
            print(f"  A/B {precision}: attention long / tiled = {long_['attn_ms'] / tiled['attn_ms']:.3f}", flush=True)


if __name__ == "__main__":
    main()
