#!/usr/bin/env python3
"""What an armed rollout request (vit_hip_set_rollout) costs.

One child process per (model, precision): ViT-B/16 at batch 512 in f32, bf16 and fp8, and ViT-B/16 at 384 px (T = 577, the
long-sequence plan) at batch 256 in f32; synthetic weights, device-resident images.  Un-armed and armed steps alternate
in one process so that both see the same clocks:
  plain    un-armed (the parent commit's launch sequence: logits + probabilities)
  all      the same forward with the device form armed at first_layer 0: every layer a step, one read
  last4    first_layer -4
Then the step's own time: VIT_OP_ATTENTION from vit_hip_profile_read of an armed forward minus the same of an un-armed
one, per layer, beside the step's arithmetic (2 H T^2 D flop for the head-mean attention matrix, 2 T^3 for the product, per
image) and the fraction of the fp32 matrix rate (157 TF) that makes.
Output: profiles/rollout_rates.txt (or --out)."""
from __future__ import annotations

import argparse
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as graft  # noqa: E402

RUNS = (("vit_b_16", "f32", 512), ("vit_b_16", "bf16", 512), ("vit_b_16", "fp8", 512), ("vit_b_16_384", "f32", 256))
PEAK_TF = 157.0


def child(args):
    pkg = graft.load_package()
    b, L = pkg.binding, pkg.lib()
    assert L.vh_init(0) == 0, L.vh_last_error()
    cfg = pkg.preset(args.model)
    n, nc, H, E = args.batch, cfg.num_classes, cfg.num_heads, cfg.embed_dim
    m = pkg.ViTHip(cfg, pkg.synth_weights(cfg, 0), device=0, max_batch=n, precision=args.precision)
    T = m.tokens
    d_img = pkg.DeviceBuffer.from_numpy(pkg.synth_images(cfg, 0, n))
    d_log, d_prob = pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)
    d_roll = pkg.DeviceBuffer(n * T)
    arms = {"plain": None, "all": 0, "last4": -4}

    def arm(which):
        m.set_rollout(None if arms[which] is None else b.RolloutSpec(arms[which]), rollout=d_roll)

    def step(which):
        arm(which)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            m.forward_device(d_img.ptr, n, d_log.ptr, d_prob.ptr, None)
        m.sync()
        return n * args.steps / (time.perf_counter() - t0)

    order = [w for a in arms if a != "plain" for w in ("plain", a)]
    for w in order[:2]:
        step(w)
    rates = {w: [] for w in arms}
    for _ in range(args.reps):
        for w in order:
            rates[w].append(step(w))
    med = {w: statistics.median(v) for w, v in rates.items()}
    tag = f"{args.model} {args.precision:<5} batch {n}"
    lines = [f"{tag} {w:<5} {med[w]:9.1f} img/s  (runs {', '.join(f'{x:.0f}' for x in rates[w])})" for w in rates]
    lines.append(f"{tag} armed/un-armed: " + "  ".join(f"{w} {med[w] / med['plain']:.4f}" for w in arms if w != "plain"))

    # the step's own time: the attention operator's events, armed minus un-armed, per layer of the product
    def attention_ms(which):
        arm(which)
        out = []
        for _ in range(args.reps + 1):
            m.profile_enable(1)
            m.profile_select(["attention"])
            m.forward_device(d_img.ptr, n, d_log.ptr, d_prob.ptr, None)
            out.append(m.profile_read()["attention"][0])
            m.profile_enable(0)
        m.profile_select(None)
        return statistics.median(out[1:])

    base = attention_ms("plain")
    attn_flop, prod_flop = 2.0 * n * H * T * T * (E // H), 2.0 * n * T ** 3
    for w in (a for a in arms if a != "plain"):
        layers = cfg.depth if arms[w] == 0 else -arms[w]
        ms = (attention_ms(w) - base) / layers
        flop = attn_flop + prod_flop * (layers - 1) / layers             # the first step has no product
        lines.append(f"{tag} {w:<5} attention operator {base:.3f} ms un-armed, + {1e3 * ms:.1f} us per layer; "
                     f"{flop / 1e9:.1f} GFLOP per layer -> {flop / (ms * 1e-3) / 1e12:.1f} TF = {flop / (ms * 1e-3) / 1e12 / PEAK_TF:.3f} of {PEAK_TF:.0f} TF")
    m.set_rollout(None)
    m.close()
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rollout_rates.txt"))
    ap.add_argument("--model")
    ap.add_argument("--precision")
    ap.add_argument("--batch", type=int)
    args = ap.parse_args()
    if args.model:
        return child(args)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("# tools/rollout_rates.py: synthetic weights, device-resident images, images/s median of alternating un-armed / "
                              "armed runs; step time from the attention operator's HIP events, armed minus un-armed\n")
    for model, precision, batch in RUNS:
        subprocess.run([sys.executable, __file__, "--model", model, "--precision", precision, "--batch", str(batch), "--steps",
                        str(args.steps), "--reps", str(args.reps), "--out", args.out], check=True, timeout=600)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
