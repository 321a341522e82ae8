#!/usr/bin/env python3
"""Generate tests/golden/{b16_384,h14_518}_port_logits.npz from the CPU port (oracle/vit_seq_port.c) at the
higher-resolution presets, whose attention runs attention_long.hip (T = 577 and T = 1370).

Like oracle/make_golden_port.py these are outputs of the port, not of the reference (which hard-codes ViT-B/16 at
224 px): "port, parity unpinned".  They let the GPU tests check full-depth images at T > 512 without spending minutes
of CPU per image on the test box.  Inputs are regenerated from seeds, never stored:
    b16_384_port_logits.npz   vit_b_16_384, weights seed_base 11, synthetic images 7 and 8
    h14_518_port_logits.npz   vit_h_14_518, weights seed_base 13, synthetic images 9 and 10
each with logits[2][1000], probs[2][1000], images[2] (the indices) and seed_base.

    python tools/make_long_seq_goldens.py       # both files, one process (one thread) per image
"""
from __future__ import annotations

import sys
import time
from multiprocessing import Pool
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from oracle.oracle import Oracle  # noqa: E402

GOLD = ROOT / "tests" / "golden"
CASES = {"b16_384": ("vit_b_16_384", 11, [7, 8]), "h14_518": ("vit_h_14_518", 13, [9, 10])}


def one_image(job):
    preset, seed_base, index = job
    t0 = time.time()
    orc = Oracle(preset)
    logits, probs, _ = orc.forward(orc.synth_image(index), orc.synth_weights(seed_base))
    print(f"{preset} image {index}: {time.time() - t0:.0f} s", flush=True)
    return logits, probs


def main() -> None:
    jobs = [(preset, seed, i) for preset, seed, idx in CASES.values() for i in idx]
    with Pool(len(jobs)) as pool:
        res = pool.map(one_image, jobs)
    k = 0
    for tag, (preset, seed, idx) in CASES.items():
        logits = np.stack([res[k + j][0] for j in range(len(idx))])
        probs = np.stack([res[k + j][1] for j in range(len(idx))])
        k += len(idx)
        np.savez_compressed(GOLD / f"{tag}_port_logits.npz", logits=logits, probs=probs,
                            images=np.array(idx), seed_base=np.array(seed),
                            note=np.array(f"{preset}: oracle/vit_seq_port.c (the port; parity unpinned -- the reference has "
                                          f"no {preset} code), tools/make_long_seq_goldens.py"))
        print(tag, "argmax", logits.argmax(1), "prob", probs.max(1))


if __name__ == "__main__":
    main()
