"""rect_rates.py -- ViT-B/16 on a non-square input: 224 x 336 pixels (14 x 21 patches, T = 295), batch 256, synthetic weights,
device-resident fp32 images; images/s of four runs of ten steps after three warm-up steps, in F32, BF16_GEMM and FP8_GEMM.
New ground with nothing to compare against: the square forward's own before / after comparison is made with bench.py
(profiles/rect_rates.txt states how)."""
import sys, time
from pathlib import Path
import numpy as np
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import __graft_entry__ as g
pkg = g.load_package()
cfg = pkg.preset("vit_b_16")
cfg.img_width = 336
weights = pkg.synth_weights(cfg, 0)
B, STEPS, WARM = 256, 10, 3
images = pkg.synth_images(cfg, 0, B)
for precision in ("f32", "bf16", "fp8"):
    model = pkg.ViTHip(cfg, weights, device=0, max_batch=B, precision=precision)
    d_img = pkg.DeviceBuffer.from_numpy(images)
    d_l, d_p = pkg.DeviceBuffer(B * 1000), pkg.DeviceBuffer(B * 1000)
    runs = []
    for r in range(4):
        for _ in range(WARM):
            model.forward_device(d_img.ptr, B, d_l.ptr, d_p.ptr)
        model.sync()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            model.forward_device(d_img.ptr, B, d_l.ptr, d_p.ptr)
        model.sync()
        runs.append(B * STEPS / (time.perf_counter() - t0))
    ok = bool(np.isfinite(d_l.to_numpy()).all())
    print(f"vit_b_16 224x336 {precision:5s} batch {B} T={model.tokens} {np.median(runs):9.1f} img/s  (runs {', '.join(f'{x:.0f}' for x in runs)}) finite={ok}", flush=True)
    model.close()
