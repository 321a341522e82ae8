"""Shared by the GPU tests of the image ingest path (test_gpu_resize_input.py, test_gpu_ingest_shapes.py): staging of
8-bit sources in device memory, the resize kernel's launch constants restated, and the tiny contexts whose
(in_chans, img_size) select each instantiation of resize_crop_kernel (csrc/resize.hip)."""
import re
from pathlib import Path

import numpy as np

import resize_ref as R

ROOT = Path(__file__).resolve().parent.parent
RESIZE_HIP = ROOT / "vit-with-opencl_amd" / "csrc" / "resize.hip"

# csrc/resize.hip: threads per workgroup, bytes of LDS for a chunk's horizontal pass, int32 accumulators per thread, the
# most crop bytes per thread and row.  resize_constants_in_source() reads the enum itself; a test asserts the two agree.
THREADS, HBUF_BYTES, ACC_REGS, MAX_JN = 256, 32768, 48, 12


def resize_constants_in_source():
    m = re.search(r"enum \{ THREADS = (\d+), HBUF_BYTES = (\d+), ACC_REGS = (\d+), MAX_JN = (\d+) \};", RESIZE_HIP.read_text())
    assert m, "csrc/resize.hip no longer states THREADS, HBUF_BYTES, ACC_REGS and MAX_JN in one enum"
    return tuple(int(g) for g in m.groups())


def resize_jn(chans, crop):
    """crop bytes per thread and row: the JN of resize_crop_kernel<JN, R, LAYOUT>"""
    return (crop * chans + THREADS - 1) // THREADS


def resize_band_rows(jn):
    """band_rows<JN>(): output rows per workgroup"""
    return min(ACC_REGS // jn, 16)


def resize_chunk_rows(chans, crop):
    """input rows whose horizontal pass fits the LDS at once"""
    return HBUF_BYTES // (crop * chans)


# (in_chans, img_size) -> patch_size of the tiny context: one per JN in 1..12 and per band height with a ragged last band,
# 4 x 768 = 3072 bytes per row exactly (JN = 12, no tail lanes), and the (channels, crop) of the committed Pillow cases
RESIZE_CASES = {
    (1, 40): 8, (2, 168): 12, (4, 168): 12, (4, 224): 16, (3, 384): 32, (4, 350): 25, (4, 392): 28, (4, 476): 34, (4, 518): 37,
    (4, 602): 43, (4, 658): 47, (4, 714): 51, (4, 768): 48,
    (1, 224): 16, (1, 384): 32,
}


def tiny_config(pkg, chans, img, patch, embed=128, depth=1, classes=10):
    """2 heads of 64 (embed 128) or 4 heads of 64 (embed 256: what the block-scaled mode needs)"""
    cfg = pkg.preset("vit_b_16")
    cfg.img_size, cfg.patch_size, cfg.in_chans, cfg.num_classes = img, patch, chans, classes
    cfg.embed_dim, cfg.depth, cfg.num_heads, cfg.mlp_hidden = embed, depth, embed // 64, 2 * embed
    return cfg


def tiny_resize_context(pkg, chans, crop, max_batch=4):
    cfg = tiny_config(pkg, chans, crop, RESIZE_CASES[(chans, crop)])
    return pkg.ViTHip(cfg, pkg.synth_weights(cfg, 9), device=0, max_batch=max_batch)


class Staged:
    """Images uploaded into one device buffer at odd byte offsets, with padded rows: descriptors for the device forms."""

    def __init__(self, pkg, images_hwc, layout):
        self.descs, blobs, off = [], [], 0
        for i, img in enumerate(images_hwc):
            h, w, c = img.shape
            a = img if layout == "hwc" else np.ascontiguousarray(img.transpose(2, 0, 1))
            pad = 3 + 5 * (i % 3)   # bytes of padding per row
            row = w * c if layout == "hwc" else w
            rows = h if layout == "hwc" else c * h
            buf = np.zeros((rows, row + pad), dtype=np.uint8)
            buf[:, :row] = a.reshape(rows, row)
            off += 1 + 2 * (i % 4)   # odd offsets
            blobs.append((off, buf))
            self.descs.append((off, h, w, row + pad))
            off += buf.nbytes
        host = np.zeros(off + 16, dtype=np.uint8)
        for o, buf in blobs:
            host[o:o + buf.nbytes] = buf.reshape(-1)
        self.buf = pkg.DeviceBuffer.from_numpy(host, dtype=np.uint8)
        base = self.buf.ptr.value
        self.descs = [(base + o, h, w, s) for o, h, w, s in self.descs]


def band_input_rows(h, resize_short, crop, f, band_rows):
    """the largest count of input rows [ylo, yhi) that one band of `band_rows` crop rows reads (resize_ref's bounds)"""
    nh, _, top, _ = R.geometry(h, h, resize_short, crop)
    ymin, ycnt, _ = R.coefficients(h, nh, f, top, crop)
    return max(int((ymin[r0:r0 + band_rows] + ycnt[r0:r0 + band_rows]).max() - ymin[r0:r0 + band_rows].min())
               for r0 in range(0, crop, band_rows))
