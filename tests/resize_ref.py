"""NumPy statement of the resize + centre crop that vit_hip_resize_crop_u8 computes (include/ViT_opencl.h): torchvision's
Resize(int) / CenterCrop geometry, then Pillow's Resample.c on 8-bit channels -- coefficients in float64 in Pillow's
operation order, converted to int32 with 22 fractional bits, a horizontal pass rounded to uint8, then a vertical pass.
Only the crop's rows and columns are computed; every output index has its own coefficients, so that is the same thing.

Source images come from an explicit integer hash of (seed, index), not from a NumPy Generator, so that they do not depend on
the NumPy version: noise, gradients and saturated hard edges, so that bicubic overshoot clips."""
from __future__ import annotations

import hashlib
import math

import numpy as np

BILINEAR, BICUBIC = 0, 1
FILTERS = {"bilinear": BILINEAR, "bicubic": BICUBIC}
PRECISION_BITS = 22


def geometry(h: int, w: int, resize_short: int, crop: int):
    """(resized_h, resized_w, top, left): torchvision's _compute_resized_output_size and CenterCrop"""
    short, long_ = (w, h) if w <= h else (h, w)
    new_short, new_long = resize_short, int(resize_short * long_ / short)
    nw, nh = (new_short, new_long) if w <= h else (new_long, new_short)
    return nh, nw, int(round((nh - crop) / 2.0)), int(round((nw - crop) / 2.0))


def _filter(f: int, x: np.ndarray) -> np.ndarray:
    x = np.abs(x)
    if f == BILINEAR:
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1,
                    np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def coefficients(in_size: int, out_size: int, f: int, first: int, count: int):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for output indices [first, first + count):
    (xmin[count], taps[count], int32 weights[count][ksize])"""
    scale = float(np.float32(in_size)) / out_size
    filterscale = max(scale, 1.0)
    support = (2.0 if f == BICUBIC else 1.0) * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(first, first + count, dtype=np.float64) + 0.5) * scale
    ss = 1.0 / filterscale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)
    arg = ((x[None, :] + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss
    w = np.where(x[None, :] < xmax[:, None], _filter(f, arg), 0.0)
    ww = np.zeros(count)
    for t in range(ksize):   # Pillow sums in order
        ww = ww + w[:, t]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    scaled = w * (1 << PRECISION_BITS)
    k = np.where(w < 0, (-0.5 + scaled).astype(np.int64), (0.5 + scaled).astype(np.int64))
    return xmin, xmax, k


def _clip8(ss: np.ndarray) -> np.ndarray:
    return np.clip(ss >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize_crop(img: np.ndarray, resize_short: int, crop: int, f: int) -> np.ndarray:
    """img [h][w][C] uint8 -> the crop x crop x C crop, uint8 (HWC)"""
    h, w = img.shape[:2]
    nh, nw, top, left = geometry(h, w, resize_short, crop)
    xmin, _, kx = coefficients(w, nw, f, left, crop)
    ymin, ycnt, ky = coefficients(h, nh, f, top, crop)
    y0, y1 = int(ymin.min()), int((ymin + ycnt).max())
    # int32 as in Resample.c: |sum u k| <= 255 x sum |k| < 2^31 for both filters (sum |k| stays below 1.3 x 2^22)
    src = img[y0:y1].astype(np.int32)
    kx, ky = kx.astype(np.int32), ky.astype(np.int32)
    acc = np.full((y1 - y0, crop, img.shape[2]), 1 << (PRECISION_BITS - 1), dtype=np.int32)
    for t in range(kx.shape[1]):   # taps beyond a column's count have weight 0; clamp their index into the row
        if kx[:, t].any():
            acc += src[:, np.minimum(xmin + t, w - 1), :] * kx[:, t][None, :, None]
    hrow = _clip8(acc).astype(np.int32)
    out = np.full((crop, crop, img.shape[2]), 1 << (PRECISION_BITS - 1), dtype=np.int32)
    for t in range(ky.shape[1]):
        if ky[:, t].any():
            out += hrow[np.minimum(ymin + t, y1 - 1) - y0] * ky[:, t][:, None, None]
    return _clip8(out)


def _mix32(v: np.ndarray) -> np.ndarray:
    """murmur3's 32-bit finaliser"""
    v = v ^ (v >> np.uint32(16))
    v = v * np.uint32(0x85EBCA6B)
    v = v ^ (v >> np.uint32(13))
    v = v * np.uint32(0xC2B2AE35)
    return v ^ (v >> np.uint32(16))


def source_image(seed: int, h: int, w: int, c: int = 3) -> np.ndarray:
    """[h][w][c] uint8 from a hash of (seed, index): the image is cut into a 4 x 3 grid of regions, each noise, a gradient or
    saturated 0/255 blocks with hard edges (chosen by the hash of the region)"""
    with np.errstate(over="ignore"):
        y = np.arange(h, dtype=np.uint32)[:, None, None]
        x = np.arange(w, dtype=np.uint32)[None, :, None]
        ch = np.arange(c, dtype=np.uint32)[None, None, :]
        s = np.uint32((seed * 0x9E3779B9) & 0xFFFFFFFF)
        noise = _mix32((y * np.uint32(w) + x) * np.uint32(c) + ch + s) & np.uint32(255)
        grad = (x * np.uint32(255) // np.uint32(max(w - 1, 1)) + y * np.uint32(97) // np.uint32(max(h - 1, 1)) +
                ch * np.uint32(60)) & np.uint32(255)
        bw, bh = max(w // 37, 1), max(h // 29, 1)
        blocks = np.where(((x // np.uint32(bw) + y // np.uint32(bh) + ch) & np.uint32(1)) != 0, np.uint32(255), np.uint32(0))
        region = (y * np.uint32(3) // np.uint32(h)) * np.uint32(4) + x * np.uint32(4) // np.uint32(w)
        kind = _mix32(region + s) % np.uint32(3)
        out = np.where(kind == 0, noise, np.where(kind == 1, grad, blocks))
    return np.ascontiguousarray(np.broadcast_to(out, (h, w, c)).astype(np.uint8))


def sha256(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def pil_resize_crop(img: np.ndarray, resize_short: int, crop: int, f: int) -> np.ndarray:
    """Pillow's Image.resize((nw, nh), BILINEAR | BICUBIC) then [top:top+crop, left:left+crop] (needs Pillow).

    1 channel is an "L" image and 3 channels an "RGB" image.  2 and 4 channels are INDEPENDENT BANDS: every channel is
    resized as an "L" image of its own and the results are stacked.  Channel 4 (or 2) is not treated as alpha: Pillow's own
    "RGBA" / "LA" resize premultiplies the colour bands by alpha and divides again, the library resizes every channel of a
    pixel alike ("Image ingest")."""
    from PIL import Image
    h, w, c = img.shape
    nh, nw, top, left = geometry(h, w, resize_short, crop)
    how = Image.Resampling.BICUBIC if f == BICUBIC else Image.Resampling.BILINEAR
    if c == 3:
        out = np.asarray(Image.fromarray(img, "RGB").resize((nw, nh), how))
    else:
        out = np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(img[:, :, ch]), "L").resize((nw, nh), how))
                        for ch in range(c)], axis=2)
    out = out.reshape(nh, nw, c)
    return np.ascontiguousarray(out[top:top + crop, left:left + crop])


# The cases the committed Pillow hashes (tests/golden/resize_crop_pil_sha256.json) were made from: (seed, h, w, channels,
# resize_short, crop, filter).  Portrait, landscape, square, h == resize_short, upscales, 1 x N and N x 1, 4000 x 3000 and a
# downscale beyond 16x; then 1, 2 and 4 channels at the crops whose row length crop x channels selects each instantiation
# of the resize kernel (40 to 768 px; 2 and 4 channels are independent bands, see pil_resize_crop).
GOLDEN_CASES = [
    (1, 375, 500, 3, 256, 224, "bilinear"), (2, 500, 375, 3, 256, 224, "bicubic"), (3, 256, 256, 3, 256, 224, "bilinear"),
    (4, 224, 224, 3, 224, 224, "bicubic"), (5, 100, 150, 3, 224, 224, "bilinear"), (6, 150, 100, 3, 248, 224, "bicubic"),
    (7, 1000, 1333, 3, 256, 224, "bilinear"), (8, 1333, 1000, 3, 248, 224, "bicubic"), (9, 3000, 4000, 3, 256, 224, "bilinear"),
    (10, 4000, 3000, 3, 256, 224, "bicubic"), (11, 1, 700, 3, 256, 224, "bilinear"), (12, 700, 1, 3, 256, 224, "bicubic"),
    (13, 257, 300, 3, 248, 224, "bicubic"), (14, 481, 257, 3, 256, 224, "bilinear"), (15, 6000, 4000, 3, 224, 224, "bicubic"),
    (16, 999, 256, 3, 256, 224, "bilinear"), (17, 300, 400, 1, 256, 224, "bicubic"), (18, 512, 683, 3, 384, 384, "bicubic"),
    (19, 384, 600, 3, 384, 384, "bilinear"), (20, 90, 60, 3, 224, 224, "bicubic"),
    (21, 60, 45, 1, 48, 40, "bilinear"), (22, 200, 13, 1, 40, 40, "bicubic"), (23, 300, 400, 2, 192, 168, "bicubic"),
    (24, 90, 120, 2, 168, 168, "bilinear"), (25, 168, 168, 4, 168, 168, "bicubic"), (26, 800, 700, 4, 176, 168, "bilinear"),
    (27, 250, 333, 4, 256, 224, "bicubic"), (28, 100, 80, 4, 350, 350, "bilinear"), (29, 500, 400, 4, 400, 392, "bicubic"),
    (30, 1, 300, 4, 476, 476, "bilinear"), (31, 64, 64, 4, 518, 518, "bicubic"), (32, 2500, 2500, 4, 602, 602, "bilinear"),
    (33, 120, 90, 4, 700, 658, "bicubic"), (34, 300, 1, 4, 714, 714, "bilinear"), (35, 200, 260, 4, 768, 768, "bicubic"),
    (36, 333, 500, 1, 400, 384, "bilinear"),
]
