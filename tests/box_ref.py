"""NumPy statement of the box crops that vit_hip_crop_boxes_u8 computes (include/ViT_opencl.h): Pillow's
Image.resize((out, out), BILINEAR | BICUBIC, box=(left, top, right, bottom)) on 8-bit channels.  It is resize_ref's
arithmetic with two more terms per axis -- Pillow's precompute_coeffs(inSize, in0, in1, outSize):

    scale  = (double)(in1 - in0) / out          the box ends are C floats and the subtraction is done in float
    center = (double)in0 + (xx + 0.5) * scale

The filters, the clip and the hashed source images are resize_ref's own."""
from __future__ import annotations

import math

import numpy as np

import resize_ref as R
from resize_ref import BICUBIC, BILINEAR, FILTERS, PRECISION_BITS, sha256, source_image  # noqa: F401


def coefficients(in_size: int, in0, in1, out_size: int, f: int):
    """Pillow's precompute_coeffs(in_size, in0, in1, out_size) + normalize_coeffs_8bpc for every output index:
    (xmin[out], taps[out], int32 weights[out][ksize])"""
    in0, in1 = np.float32(in0), np.float32(in1)
    scale = float(np.float32(in1 - in0)) / out_size
    filterscale = max(scale, 1.0)
    support = (2.0 if f == BICUBIC else 1.0) * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    center = float(in0) + (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    ss = 1.0 / filterscale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)
    arg = ((x[None, :] + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss
    w = np.where(x[None, :] < xmax[:, None], R._filter(f, arg), 0.0)
    ww = np.zeros(out_size)
    for t in range(ksize):   # Pillow sums in order
        ww = ww + w[:, t]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    scaled = w * (1 << PRECISION_BITS)
    k = np.where(w < 0, (-0.5 + scaled).astype(np.int64), (0.5 + scaled).astype(np.int64))
    return xmin, xmax, k


def box_rows(h: int, top, bottom, out: int, f: int):
    """(first, count): the source rows that the `out` output rows of a box from top to bottom read"""
    ymin, ycnt, _ = coefficients(h, top, bottom, out, f)
    first = int(ymin.min())
    return first, int((ymin + ycnt).max()) - first


def resize_box(img: np.ndarray, box, out: int, f: int) -> np.ndarray:
    """img [h][w][C] uint8, box (left, top, right, bottom) -> the out x out x C crop, uint8 (HWC)"""
    h, w = img.shape[:2]
    xmin, _, kx = coefficients(w, box[0], box[2], out, f)
    ymin, ycnt, ky = coefficients(h, box[1], box[3], out, f)
    y0, y1 = int(ymin.min()), int((ymin + ycnt).max())
    src = img[y0:y1].astype(np.int32)
    kx, ky = kx.astype(np.int32), ky.astype(np.int32)
    acc = np.full((y1 - y0, out, img.shape[2]), 1 << (PRECISION_BITS - 1), dtype=np.int32)
    for t in range(kx.shape[1]):   # taps beyond a column's count have weight 0; clamp their index into the row
        if kx[:, t].any():
            acc += src[:, np.minimum(xmin + t, w - 1), :] * kx[:, t][None, :, None]
    hrow = R._clip8(acc).astype(np.int32)
    res = np.full((out, out, img.shape[2]), 1 << (PRECISION_BITS - 1), dtype=np.int32)
    for t in range(ky.shape[1]):
        if ky[:, t].any():
            res += hrow[np.minimum(ymin + t, y1 - 1) - y0] * ky[:, t][:, None, None]
    return R._clip8(res)


def pil_resize_box(img: np.ndarray, box, out: int, f: int) -> np.ndarray:
    """Pillow's Image.resize((out, out), BILINEAR | BICUBIC, box=box) (needs Pillow); 1 channel is an "L" image, 3 channels
    an "RGB" image, 2 and 4 channels independent "L" bands, as resize_ref.pil_resize_crop states them"""
    from PIL import Image
    c = img.shape[2]
    how = Image.Resampling.BICUBIC if f == BICUBIC else Image.Resampling.BILINEAR
    box = tuple(float(v) for v in box)
    if c == 3:
        res = np.asarray(Image.fromarray(img, "RGB").resize((out, out), how, box=box))
    else:
        res = np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(img[:, :, ch]), "L").resize((out, out), how, box=box))
                        for ch in range(c)], axis=2)
    return np.ascontiguousarray(res.reshape(out, out, c))


def hashed_boxes(seed: int, count: int, h: int, w: int):
    """`count` boxes of an h x w image from an integer hash of (seed, index): quarter-pixel ends, at least 1 px each way"""
    with np.errstate(over="ignore"):
        v = R._mix32(np.arange(4 * count, dtype=np.uint32) + np.uint32((seed * 0x9E3779B9) & 0xFFFFFFFF)).reshape(count, 4)
    boxes = []
    for a, b, c, d in v.tolist():
        bw, bh = 4 + a % (4 * w - 3), 4 + b % (4 * h - 3)          # quarter pixels, 1 px .. the whole side
        left, top = c % (4 * w - bw + 1), d % (4 * h - bh + 1)
        boxes.append((left / 4.0, top / 4.0, (left + bw) / 4.0, (top + bh) / 4.0))
    return boxes


# The cases the committed Pillow hashes (tests/golden/box_resize_pil_sha256.json) were made from: (seed, h, w, channels, box,
# out, filter).  3 channels at 224: identity-size integer boxes at offsets, fractional boxes, each of the four edges, the
# whole image, 1 x 1 px boxes, 1 x N and N x 1 boxes, downscales above 16x, a 1327 x 983 box, a tile of a 4000 x 3000 frame,
# 1 x 700 and 700 x 1 sources, non-square boxes; then 1, 2, 3 and 4 channels at the sizes of ingest_common's tiny contexts
# (1, 40), (2, 168), (4, 168), (3, 384) and (4, 768), whose rows select JN = 1, 2, 3, 5 and 12 of the resize kernel.  The three
# boxes of the 4000 x 3000 frame share seed 15, so a test makes that source once.
GOLDEN_CASES = [
    (1, 375, 500, 3, (100, 50, 324, 274), 224, "bilinear"), (2, 500, 375, 3, (17, 133, 241, 357), 224, "bicubic"),
    (3, 375, 500, 3, (10.3, 20.7, 300.2, 310.9), 224, "bilinear"), (4, 500, 375, 3, (0.5, 0.25, 374.75, 499.5), 224, "bicubic"),
    (5, 300, 400, 3, (0, 50, 120, 250), 224, "bilinear"), (6, 300, 400, 3, (250, 60, 400, 200), 224, "bicubic"),
    (7, 300, 400, 3, (30, 0, 330, 100), 224, "bilinear"), (8, 300, 400, 3, (100, 180, 360, 300), 224, "bicubic"),
    (9, 300, 400, 3, (0, 0, 400, 300), 224, "bilinear"), (10, 256, 256, 3, (0, 0, 256, 256), 224, "bicubic"),
    (11, 100, 150, 3, (77, 33, 78, 34), 224, "bicubic"), (12, 100, 150, 3, (149, 99, 150, 100), 224, "bilinear"),
    (13, 200, 300, 3, (40, 10, 41, 190), 224, "bicubic"), (14, 200, 300, 3, (5, 100, 295, 101), 224, "bilinear"),
    (15, 3000, 4000, 3, (100, 50, 3900, 2950), 224, "bilinear"), (15, 3000, 4000, 3, (0, 0, 4000, 3000), 224, "bicubic"),
    (17, 1000, 1333, 3, (3.5, 2.5, 1330.5, 985.5), 224, "bicubic"), (15, 3000, 4000, 3, (3776, 2776, 4000, 3000), 224, "bilinear"),
    (19, 1, 700, 3, (0, 0, 700, 1), 224, "bilinear"), (20, 1, 700, 3, (100.5, 0, 400.25, 1), 224, "bicubic"),
    (21, 700, 1, 3, (0, 0, 1, 700), 224, "bicubic"), (22, 700, 1, 3, (0, 33.3, 1, 640.9), 224, "bilinear"),
    (23, 480, 640, 3, (100, 100, 500, 200), 224, "bicubic"), (24, 480, 640, 3, (600, 0, 640, 480), 224, "bilinear"),
    (25, 60, 90, 1, (10, 5, 50, 45), 40, "bilinear"), (26, 60, 700, 1, (0, 0, 700, 60), 40, "bicubic"),
    (27, 50, 50, 1, (20, 20, 21, 21), 40, "bilinear"),
    (28, 300, 400, 2, (50.5, 60.5, 300.25, 290.75), 168, "bicubic"), (29, 200, 200, 2, (0, 0, 200, 200), 168, "bilinear"),
    (30, 200, 180, 2, (12, 32, 180, 200), 168, "bicubic"),
    (31, 250, 333, 4, (100, 7, 268, 175), 168, "bilinear"), (32, 800, 700, 4, (1.5, 2.5, 690.5, 790), 168, "bicubic"),
    (33, 90, 120, 4, (119, 0, 120, 90), 168, "bilinear"),
    (34, 512, 683, 3, (100, 64, 484, 448), 384, "bicubic"), (35, 600, 800, 3, (0.25, 0.75, 799.5, 599.25), 384, "bilinear"),
    (36, 400, 300, 3, (150, 200, 151, 201), 384, "bicubic"),
    (37, 200, 260, 4, (0, 0, 260, 200), 768, "bicubic"), (38, 900, 1000, 4, (116, 66, 884, 834), 768, "bilinear"),
    (39, 1, 300, 4, (0, 0, 300, 1), 768, "bilinear"),
    (40, 375, 500, 3, (0, 0, 1, 1), 224, "bilinear"),
]
