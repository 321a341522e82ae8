#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the REFERENCE ITSELF.

Runs oracle/_ref/ref_harness -- the reference's unmodified ViT_seq.c compiled in
place by oracle/Makefile -- on the deterministic synthetic inputs of
vit_synth_* (weights: seed_base 0; images: index i -> seed 1000+i) and stores
its outputs as small fixtures.  Only possible in the build container (needs
/root/reference); the fixtures are committed, the reference never travels.

Why synthetic inputs: 36 of the reference's 152 weight files and
Data/input-100.bin are absent from the snapshot (/root/reference/.MISSING_LARGE_BLOBS),
so its pretrained goldens (Data/answer_result*.txt) cannot be reproduced.

Fixtures (inputs are regenerated from seeds, never stored):
  b16_full.npz    logits[4][1000], probs[4][1000] for synthetic images 0..3
  b16_stages.npz  per-stage outputs for image 0 / layer 0: small tensors in full,
                  large ones as a stride-37 sample plus fp64 sum and abs-sum
  b16_answer_result.txt  Main.c-format result lines ("[i] label: L / prob: P")
  b16_full_rounded.npz / b16_answer_result_rounded.txt  the same with weights rounded to 1e-6
                  as the reference loader delivers them from disk (Network.c:208-211)
  b16_answer_result_100_rounded.txt  (`make_golden.py answers100`) 100 result lines -- comparator.c's
                  IMAGE_COUNT (comparator.c:9) -- for synthetic images 0..99 on rounded weights, written
                  with Main.c's own arg-max loop (Main.c:59-71: pred_idx is NOT reset per image and class 0
                  is never visited, so the line is what the reference's Main.c would print around ViT_seq)
  b16_seed1.npz   (`make_golden.py other_seed`) logits / probabilities of synthetic images 100, 101 on a SECOND weight set
                  (seed_base 1), from the reference's ViT_seq.c
  b16_real_image.npz  (`make_golden.py real_image`) the reference's ONE real input -- Data/input-1.bin, a normalised
                  224x224 photograph (spatially correlated pixels, unlike every synthetic image) -- kept as a data fixture,
                  with the logits / probabilities the reference's ViT_seq.c gives for it on the seed-0 synthetic weights
                  (its pretrained answer Data/answer_result_1.txt cannot be reproduced: 36 weight files are absent)
  b16_stages_sha256.json  (`make_golden.py stage_digests`) sha256 of every element of the reference's per-stage outputs
                  for image 0 / layer 0 (the tensors b16_stages.npz only samples), so that the element-by-element check of
                  the port's stages runs where the reference is absent
  ref_weight_stats.json  (`make_golden.py ref_weight_stats`) per tensor present in the reference's Network/ directory: its
                  name, sigma, |max|/sigma and kurtosis -- recorded statistics that tests/realistic_weights.py is checked against
  b16_realistic.npz  (`make_golden.py realistic`) the logits / probabilities the reference's ViT_seq.c gives on the heavy-
                  tailed B/16 set of tests/realistic_weights.py (seed 0, default offset and massive channel) for synthetic
                  images 0..2 and the real image of b16_real_image.npz, with the set's sha256, the exposure of the
                  residual rows at every LayerNorm input and tools/quant_sensitivity.py's predicted relative L2 logit error
                  of bf16 and fp8, LayerNorms folded and separate
  ref_abi_layout.json  (`make_golden.py abi_layout <reference dir>`) sizeof / offsetof of ImageData and Network as the reference's own
                  Network.h declares them (x86-64, gcc), the layout include/Network.h must keep
"""
from __future__ import annotations

import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from oracle import oracle as orc  # noqa: E402

GOLD = ROOT / "tests" / "golden"
STRIDE = 37
N_IMAGES = 4


def summarize(a: np.ndarray) -> dict[str, np.ndarray]:
    a = a.ravel()
    return {
        "sample": a[::STRIDE].copy(),
        "sum": np.array(a.astype(np.float64).sum()),
        "abssum": np.array(np.abs(a.astype(np.float64)).sum()),
        "count": np.array(a.size),
    }


def main_c_lines(probs: np.ndarray) -> list[str]:
    """The result lines exactly as Main.c:59-72 produces them from `probabilities`."""
    lines, pred = [], 0
    for i in range(probs.shape[0]):
        for j in range(1, probs.shape[1]):          # Main.c:62: j starts at 1; pred carries over (Main.c:59)
            if probs[i][j] > probs[i][pred]:
                pred = j
        lines.append("[%d] label: %d / prob: %.6f\n" % (i, pred, probs[i][pred]))
    return lines


def answers100(workers: int = 8) -> None:
    """100 images through the reference's ViT_seq.c on 1e-6-rounded weights, `workers` processes at a time."""
    import subprocess
    orc.build()
    if not orc.have_reference():
        sys.exit("oracle/_ref/ref_harness missing: run in the build container (needs /root/reference)")
    n = 100
    probs = np.empty((n, 1000), dtype=np.float32)
    with tempfile.TemporaryDirectory() as td:
        for lo in range(0, n, workers):
            idx = list(range(lo, min(n, lo + workers)))
            procs = [subprocess.Popen([str(orc.REF_HARNESS), "full_rounded", str(i), "1", "0", str(Path(td) / f"{i}.bin")],
                                      stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) for i in idx]
            assert all(p.wait() == 0 for p in procs)
            for i in idx:
                probs[i] = orc.read_records(Path(td) / f"{i}.bin")["probs"]
            print("images", idx[0], "..", idx[-1], "done", flush=True)
    (GOLD / "b16_answer_result_100_rounded.txt").write_text("".join(main_c_lines(probs)))
    # cross-check against the 4-image rounded fixture
    small = np.load(GOLD / "b16_full_rounded.npz")["probs"]
    assert np.array_equal(small, probs[:4]), "100-image run disagrees with b16_full_rounded.npz"
    print("wrote b16_answer_result_100_rounded.txt; labels:", sorted(set(int(l.split()[2]) for l in main_c_lines(probs))))


def real_image() -> None:
    """Data/input-1.bin through the reference's ViT_seq.c on the seed-0 synthetic weights -> b16_real_image.npz."""
    src = Path("/root/reference/MulticoreMainProject/Data/input-1.bin")
    orc.build()
    if not orc.have_reference() or not src.exists():
        sys.exit("needs the build container (oracle/_ref/ref_harness and the reference's Data/input-1.bin)")
    raw = src.read_bytes()
    n, c, h, w = np.frombuffer(raw, dtype=np.int32, count=4)
    assert (n, c, h, w) == (1, 3, 224, 224) and len(raw) == 16 + 4 * c * h * w
    image = np.frombuffer(raw, dtype=np.float32, offset=16).reshape(c, h, w).copy()
    with tempfile.TemporaryDirectory() as td:
        rec = orc.run_reference("full_file", src, 0, out_path=Path(td) / "real.bin")
    np.savez_compressed(GOLD / "b16_real_image.npz", image=image, logits=rec["logits"].reshape(1, 1000),
                        probs=rec["probs"].reshape(1, 1000), seed_base=np.array(0),
                        note=np.array("image = the reference's Data/input-1.bin (data, its only real input); logits/probs = "
                                      "the reference's own ViT_seq.c on it with vit_synth_tensor weights, seed_base 0"))
    lg = rec["logits"]
    print("real image: mean %.3f std %.3f  argmax %d  top-2 margin %.4f" % (image.mean(), image.std(), int(lg.argmax()),
                                                                           float(np.sort(lg)[-1] - np.sort(lg)[-2])))


def other_seed() -> None:
    """A second weight set (seed_base 1) and other images (100, 101) through the reference's ViT_seq.c -> b16_seed1.npz:
    the pinning does not rest on one draw of the synthetic weights."""
    orc.build()
    if not orc.have_reference():
        sys.exit("needs the build container (oracle/_ref/ref_harness)")
    with tempfile.TemporaryDirectory() as td:
        rec = orc.run_reference("full", 100, 2, 1, out_path=Path(td) / "seed1.bin")
    np.savez(GOLD / "b16_seed1.npz", logits=rec["logits"].reshape(2, 1000), probs=rec["probs"].reshape(2, 1000),
             seed_base=np.array(1), first_image=np.array(100))
    print("seed 1: argmax", rec["logits"].reshape(2, 1000).argmax(1))


STAGES = ("conv", "tokens", "ln", "mha", "mlp", "enc0")


def stage_digests() -> None:
    """The reference's ViT_seq.c stage outputs for image 0 / layer 0 -> sha256 of their float32 bytes, every element."""
    import hashlib
    import json
    orc.build()
    if not orc.have_reference():
        sys.exit("needs the build container (oracle/_ref/ref_harness)")
    with tempfile.TemporaryDirectory() as td:
        st = orc.run_reference("stages", 0, out_path=Path(td) / "stages.bin")
    rec = {"what": "sha256 of the float32 bytes of the reference's own ViT_seq.c stage outputs, synthetic image 0, weights "
                   "seed_base 0, encoder layer 0 (oracle/make_golden.py stage_digests)",
           "stages": {n: {"count": int(st[n].size), "sha256": hashlib.sha256(np.ascontiguousarray(st[n], np.float32).tobytes())
                          .hexdigest()} for n in STAGES}}
    (GOLD / "b16_stages_sha256.json").write_text(json.dumps(rec, indent=1) + "\n")
    print("wrote b16_stages_sha256.json")


REF_NETWORK = Path("/root/reference/MulticoreMainProject/Network")


def ref_weight_stats() -> None:
    """sigma, |max|/sigma and kurtosis of every tensor present under the reference's Network/ -> ref_weight_stats.json"""
    import json
    import re
    sys.path.insert(0, str(ROOT / "tests"))
    import realistic_weights as rw
    files = sorted(REF_NETWORK.glob("Weight_*.bin"), key=lambda p: int(p.name.split("_")[1]))
    if not files:
        sys.exit(f"{REF_NETWORK}: no weight files (needs the build container)")
    rows = []
    for f in files:
        m = re.fullmatch(r"Weight_(\d+)_(.*)\.bin", f.name)
        a = np.fromfile(f, dtype=np.float32)
        st = rw.tensor_stats(a)
        rows.append({"index": int(m.group(1)), "name": m.group(2), "count": int(a.size),
                     **{k: float("%.4g" % v) for k, v in st.items()}})
    rec = {"what": "statistics of the reference's real ViT-B/16 tensors present in its Network/ directory (36 of 152 are "
                   "absent), float64 over each tensor (oracle/make_golden.py ref_weight_stats)", "tensors": rows}
    body = ",\n".join(json.dumps(r) for r in rows)
    (GOLD / "ref_weight_stats.json").write_text(json.dumps(rec["what"]).join(['{"what": ', ', "tensors": [\n']) + body + "]}\n")
    print(f"wrote ref_weight_stats.json: {len(rows)} tensors")


REALISTIC_IMAGES = 3


def realistic() -> None:
    """The reference's ViT_seq.c on tests/realistic_weights.py's B/16 set -> b16_realistic.npz (see the module docstring)."""
    import subprocess
    import torch
    sys.path.insert(0, str(ROOT / "tests"))
    sys.path.insert(0, str(ROOT / "tools"))
    import quant_sensitivity as qs
    import realistic_weights as rw
    orc.build()
    if not orc.have_reference():
        sys.exit("needs the build container (oracle/_ref/ref_harness)")
    o = orc.Oracle("vit_b_16")
    cfg, seed = o.cfg, 0
    pl = rw.plan(cfg, seed)
    ws = rw.realistic_weights(cfg, seed)
    real = np.load(GOLD / "b16_real_image.npz")["image"]
    images = np.stack([o.synth_image(i) for i in range(REALISTIC_IMAGES)] + [real])
    with tempfile.TemporaryDirectory() as td:
        wpath, ipath = Path(td) / "w.bin", Path(td) / "real.bin"
        with open(wpath, "wb") as f:
            for a in ws:
                f.write(np.ascontiguousarray(a, np.float32).tobytes())
        ipath.write_bytes(np.array([1, 3, 224, 224], np.int32).tobytes() + np.ascontiguousarray(real, np.float32).tobytes())
        procs = [subprocess.Popen([str(orc.REF_HARNESS), "full_weights", str(wpath), str(i), "1", str(Path(td) / f"{i}.bin")])
                 for i in range(REALISTIC_IMAGES)]
        procs.append(subprocess.Popen([str(orc.REF_HARNESS), "full_weights_file", str(wpath), str(ipath), str(Path(td) / "r.bin")]))
        assert all(p.wait() == 0 for p in procs)
        recs = [orc.read_records(Path(td) / f"{i}.bin") for i in range(REALISTIC_IMAGES)] + [orc.read_records(Path(td) / "r.bin")]
    logits = np.stack([r["logits"] for r in recs])
    probs = np.stack([r["probs"] for r in recs])
    exp = rw.exposure(cfg, ws, images, pl["dstar"])
    # the independent error model: relative L2 of the logits, ||d|| / ||logits|| per image, against the
    # unquantised fp32 restatement
    w_t = [torch.from_numpy(np.ascontiguousarray(a)) for a in ws]
    x_t = torch.from_numpy(images)
    pred = {}
    with torch.no_grad():
        ref = qs.forward(cfg, w_t, x_t, {}, False)
        for mode, fq in (("bf16", qs.bf16), ("fp8", qs.mx)):
            out = {fold: qs.forward(cfg, w_t, x_t, {c: fq for c in qs.CLASSES}, bool(fold)) for fold in (1, 0)}
            for fold in (1, 0):
                pred[f"pred_{mode}_fold{fold}"] = ((out[fold] - ref).norm(dim=1) / ref.norm(dim=1)).numpy()
            pred[f"pred_{mode}_fold_vs_separate"] = ((out[1] - out[0]).norm(dim=1) / ref.norm(dim=1)).numpy()
    np.savez(GOLD / "b16_realistic.npz", logits=logits, probs=probs, synth_images=np.arange(REALISTIC_IMAGES),
             seed=np.array(seed), offset=np.array(5.0), massive=np.array(90.0), dstar=np.array(pl["dstar"]),
             weights_sha256=np.array(rw.weights_sha256(ws)),
             **{f"exposure_{k}": np.array(v) for k, v in exp.items()}, **pred,
             note=np.array("logits/probs: the reference's own ViT_seq.c on tests/realistic_weights.py's B/16 set (seed, offset, "
                           "massive above), synthetic images 0..2 then the real image of b16_real_image.npz; exposure_*: per "
                           "LayerNorm input (ln_1, ln_2 per layer, then the final one), float64 restatement over the four "
                           "images; pred_*: tools/quant_sensitivity.py's fake-quantised relative L2 per image (fold_vs_separate: "
                           "between its folded and separate passes)"))
    print("argmax", logits.argmax(1), "sha", rw.weights_sha256(ws)[:16])
    print("exposure mean/std max", np.round(exp["mean_std_max"], 2))
    print("massive ratio", np.round(exp["massive_ratio"], 1))
    for k, v in pred.items():
        print(k, np.round(v, 4))


LAYOUT_PROBE = r'''
#include <stdio.h>
#include <stddef.h>
#include "%s"
int main(void)
{
    printf("{\"ImageData\": {\"sizeof\": %%zu, \"offsetof\": {\"n\": %%zu, \"c\": %%zu, \"h\": %%zu, \"w\": %%zu, "
           "\"data\": %%zu}}, \"Network\": {\"sizeof\": %%zu, \"offsetof\": {\"data\": %%zu, \"size\": %%zu}}}\n",
           sizeof(ImageData), offsetof(ImageData, n), offsetof(ImageData, c), offsetof(ImageData, h),
           offsetof(ImageData, w), offsetof(ImageData, data), sizeof(Network), offsetof(Network, data),
           offsetof(Network, size));
    return 0;
}
'''


def abi_layout(ref_dir: str) -> None:
    """sizeof / offsetof of the reference's ImageData and Network, compiled from its own Network.h (in ref_dir, the
    reference's MulticoreMainProject directory) -> ref_abi_layout.json."""
    import json
    import subprocess
    header = Path(ref_dir) / "Network.h"
    if not header.is_file():
        sys.exit(f"{header}: not found (usage: make_golden.py abi_layout <the reference's MulticoreMainProject directory>)")
    with tempfile.TemporaryDirectory() as td:
        (Path(td) / "probe.c").write_text(LAYOUT_PROBE % header)
        subprocess.run(["gcc", "-fcommon", "-o", str(Path(td) / "probe"), str(Path(td) / "probe.c")], check=True)
        layout = json.loads(subprocess.run([str(Path(td) / "probe")], check=True, capture_output=True, text=True).stdout)
    rec = {"what": "sizeof / offsetof of ImageData and Network as the reference's Network.h declares them, x86-64 gcc "
                   "(oracle/make_golden.py abi_layout)", **layout}
    (GOLD / "ref_abi_layout.json").write_text(json.dumps(rec, indent=1) + "\n")
    print("wrote ref_abi_layout.json:", layout)


def main() -> None:
    if len(sys.argv) > 1 and sys.argv[1] == "stage_digests":
        stage_digests()
        return
    if len(sys.argv) > 2 and sys.argv[1] == "abi_layout":
        abi_layout(sys.argv[2])
        return
    if len(sys.argv) > 1 and sys.argv[1] == "ref_weight_stats":
        ref_weight_stats()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "realistic":
        realistic()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "other_seed":
        other_seed()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "answers100":
        answers100()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "real_image":
        real_image()
        return
    orc.build()
    if not orc.have_reference():
        sys.exit("oracle/_ref/ref_harness missing: run in the build container (needs /root/reference)")
    GOLD.mkdir(parents=True, exist_ok=True)
    with tempfile.TemporaryDirectory() as td:
        full = orc.run_reference("full", 0, N_IMAGES, 0, out_path=Path(td) / "full.bin")
        stages = orc.run_reference("stages", 0, out_path=Path(td) / "stages.bin")
        rounded = orc.run_reference("full_rounded", 0, N_IMAGES, 0, out_path=Path(td) / "rounded.bin")

    logits = full["logits"].reshape(N_IMAGES, 1000)
    probs = full["probs"].reshape(N_IMAGES, 1000)
    np.savez(GOLD / "b16_full.npz", logits=logits, probs=probs,
             seed_base=np.array(0), first_image=np.array(0),
             seconds_per_image=full["seconds_per_image"])

    out = {}
    for name in ("conv", "tokens", "ln", "mha", "mlp", "enc0"):
        for k, v in summarize(stages[name]).items():
            out[f"{name}_{k}"] = v
    for name in ("head", "softmax", "gelu"):
        out[name] = stages[name]
    out["stride"] = np.array(STRIDE)
    np.savez(GOLD / "b16_stages.npz", **out)

    # The file-based flow (Main.c: load_weights rounds every value to 1e-6, Network.c:208-211).
    rl = rounded["logits"].reshape(N_IMAGES, 1000)
    rp = rounded["probs"].reshape(N_IMAGES, 1000)
    np.savez(GOLD / "b16_full_rounded.npz", logits=rl, probs=rp)
    with open(GOLD / "b16_answer_result_rounded.txt", "w") as f:
        for i in range(N_IMAGES):
            k = int(np.argmax(rp[i]))
            f.write("[%d] label: %d / prob: %.6f\n" % (i, k, rp[i][k]))

    # Result lines exactly as Main.c:59-72 prints them, but with a per-image argmax
    # (Main.c:59 never resets pred_idx).
    with open(GOLD / "b16_answer_result.txt", "w") as f:
        for i in range(N_IMAGES):
            k = int(np.argmax(probs[i]))
            f.write("[%d] label: %d / prob: %.6f\n" % (i, k, probs[i][k]))
    print("wrote", sorted(p.name for p in GOLD.iterdir()))
    print("argmax", logits.argmax(1), "top-2 margin", np.sort(logits, 1)[:, -1] - np.sort(logits, 1)[:, -2])


if __name__ == "__main__":
    main()
