#!/usr/bin/env python3
"""What an armed attention-map request (vit_hip_set_attention) costs.

One child process per (model, precision): ViT-B/16 at batch 512 in f32, bf16 and fp8, and ViT-B/16 at 384 px (T = 577, the
long-sequence plan) at batch 256 in f32; synthetic weights, device-resident images.  Un-armed and armed steps alternate
in one process so that both see the same clocks:
  plain    un-armed (the parent commit's launch sequence: logits + probabilities)
  t1, t4   the same forward with the device form armed for heads and mean at taps (-1,) and (2, 5, 8, 11)
           (vit_b_16_384: t1 only)
  m1       mean alone at tap (-1,): one workgroup per image, every K tile formed three times
Then the kernel's own time: VIT_OP_ATTENTION from vit_hip_profile_read of an armed forward minus the same of an un-armed
one, per tap, beside the bytes of K (and q_cls) a tap reads and the rate that makes.
Output: profiles/attn_map_rates.txt (or --out)."""
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
# bytes per stored value of K in the plan's Q|K|V: fp32 rows 4, three-part planes 6, fp16 planes 2
BYTES = {"f32": 6, "bf16": 2, "fp8": 2}


def child(args):
    pkg = graft.load_package()
    b, L = pkg.binding, pkg.lib()
    assert L.vh_init(0) == 0, L.vh_last_error()
    cfg = pkg.preset(args.model)
    n, nc, H = args.batch, cfg.num_classes, cfg.num_heads
    m = pkg.ViTHip(cfg, pkg.synth_weights(cfg, 0), device=0, max_batch=n, precision=args.precision)
    T = m.tokens
    d_img = pkg.DeviceBuffer.from_numpy(pkg.synth_images(cfg, 0, n))
    d_log, d_prob = pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)
    d_heads, d_mean = pkg.DeviceBuffer(n * 4 * H * T), pkg.DeviceBuffer(n * 4 * T)
    last, four = (-1,), tuple(range(cfg.depth // 4 - 1, cfg.depth, cfg.depth // 4))
    arms = {"plain": None, "t1": (last, True), "m1": (last, False)}
    if args.model == "vit_b_16":
        arms["t4"] = (four, True)

    def arm(which):
        if arms[which] is None:
            m.set_attention(None)
        else:
            taps, heads = arms[which]
            m.set_attention(b.AttentionSpec(taps), heads=d_heads if heads else None, mean=d_mean)

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

    # the kernel's own time: the attention operator's events, armed minus un-armed, per tap
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
    k_bytes = n * T * cfg.embed_dim * BYTES[args.precision]
    for w in (a for a in arms if a != "plain"):
        taps = len(arms[w][0])
        ms = (attention_ms(w) - base) / taps
        lines.append(f"{tag} {w:<3} attention operator {base:.3f} ms un-armed, + {1e3 * ms:.1f} us per tap; K of a tap "
                     f"{k_bytes / 1e6:.1f} MB -> {k_bytes / (ms * 1e-3) / 1e12:.2f} TB/s" + (" (read three times)" if w == "m1" else ""))
    m.set_attention(None)
    m.close()
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "attn_map_rates.txt"))
    ap.add_argument("--model")
    ap.add_argument("--precision")
    ap.add_argument("--batch", type=int)
    args = ap.parse_args()
    if args.model:
        return child(args)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("# tools/attn_map_rates.py: synthetic weights, device-resident images, images/s median of alternating un-armed / "
                              "armed runs; kernel time from the attention operator's HIP events, armed minus un-armed\n")
    for model, precision, batch in RUNS:
        subprocess.run([sys.executable, __file__, "--model", model, "--precision", precision, "--batch", str(batch), "--steps",
                        str(args.steps), "--reps", str(args.reps), "--out", args.out], check=True, timeout=600)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
