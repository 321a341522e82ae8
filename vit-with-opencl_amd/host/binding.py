"""ctypes binding of libvit_hip.so -- test / bench plumbing over the C ABI.

The product is the C library (include/*.h); this module only loads it, wraps
its calls, and turns non-zero status codes into exceptions.  What the ABI is --
prototypes, struct mirrors, enum mirrors -- is stated in abi.py.  There is no
Python or CPU implementation of any operator here: if the library or a gfx950
device is missing, calls fail loudly.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

from .abi import (  # noqa: F401
    ATTN_ARITH, ATTN_KERNEL, DENSE_MAX_GRID, DENSE_MAX_LABELS, DENSE_TOKEN_TILE, ENUMS, EXPORTS, FEATURE_DTYPES, FP32_MATH,
    GALLERY_DTYPES, GALLERY_MAX_SPLITS, GALLERY_ROW_TILE, GALLERY_SOURCES, OP_NAMES, PIXEL_LAYOUTS, POS_MODES, PRECISIONS,
    PROTOTYPES, QKV_FORMS, RESIZE_FILTERS, SHARD_FN, STITCH_BLOCK, STITCH_MAX_SIDE, STRUCTS, TOKEN_LAYOUTS, TOPK_SCORES,
    AttnBuffers, AttnSpecC, Box, CompareReport, DenseBuffers, DenseSoftBuffers, DenseSoftSpecC, DenseSpecC, FeatureBuffers, FeatureSpecC, FrameBuffers, FrameSpecC,
    GalleryBuffers,
    GallerySpecC, ImageData, ImageU8, Network, PixelNorm, PosResampleC, ResizeCrop, RolloutBuffers, RolloutSpecC, TopKBuffers,
    TopKSpecC, VitConfig, declare, f32p, voidp,
)

PKG_DIR = Path(__file__).resolve().parent.parent
LIB_PATH = PKG_DIR / "libvit_hip.so"
CSRC = PKG_DIR / "csrc"


class FeatureSpec:
    """A feature request: taps (encoder layers whose output is read, negative from the end), the final LayerNorm, unit L2
    norm of cls / pooled, the element type ("f32" | "bf16"; bf16 arrives as uint16 bit patterns) and the token layout
    ("nlc" | "nchw")."""

    def __init__(self, taps=(-1,), final_norm: bool = True, l2_normalize: bool = False, dtype: str = "f32",
                 token_layout: str = "nlc"):
        self.taps, self.final_norm, self.l2_normalize = tuple(int(t) for t in taps), bool(final_norm), bool(l2_normalize)
        self.dtype, self.token_layout = dtype, token_layout

    @property
    def np_dtype(self):
        return np.dtype(np.float32 if self.dtype == "f32" else np.uint16)

    def c_struct(self) -> FeatureSpecC:
        taps = list(self.taps[:4]) + [0] * (4 - min(len(self.taps), 4))
        return FeatureSpecC(len(self.taps), (C.c_int * 4)(*taps), int(self.final_norm), int(self.l2_normalize),
                            FEATURE_DTYPES[self.dtype], TOKEN_LAYOUTS[self.token_layout])


class TopKSpec:
    """A top-k request: the k best classes per image (1..32) with their scores ("probs" | "logits")."""

    def __init__(self, k: int = 5, scores: str = "probs"):
        self.k, self.scores = int(k), scores

    def c_struct(self) -> TopKSpecC:
        return TopKSpecC(self.k, TOPK_SCORES[self.scores])


class AttentionSpec:
    """An attention-map request: taps (encoder layers whose class-token attention is read, negative from the end)."""

    def __init__(self, taps=(-1,)):
        self.taps = tuple(int(t) for t in taps)

    def c_struct(self) -> AttnSpecC:
        taps = list(self.taps[:4]) + [0] * (4 - min(len(self.taps), 4))
        return AttnSpecC(len(self.taps), (C.c_int * 4)(*taps))


def attention_sizes(cfg: "VitConfig", spec: AttentionSpec):
    """vit_attn_sizes -> (heads, mean) elements per image"""
    out = [C.c_size_t() for _ in range(2)]
    cs = spec.c_struct()
    check(lib().vit_attn_sizes(C.byref(cfg), C.byref(cs), *[C.byref(o) for o in out]), "vit_attn_sizes")
    return tuple(o.value for o in out)


class RolloutSpec:
    """A rollout request: the first layer of the product (0-based or negative from the end; 0 is the standard rollout)."""

    def __init__(self, first_layer: int = 0):
        self.first_layer = int(first_layer)

    def c_struct(self) -> RolloutSpecC:
        return RolloutSpecC(self.first_layer)


def rollout_sizes(cfg: "VitConfig", spec: RolloutSpec):
    """vit_rollout_sizes -> (rollout elements per image, device scratch bytes per image of max_batch)"""
    out = [C.c_size_t() for _ in range(2)]
    cs = spec.c_struct()
    check(lib().vit_rollout_sizes(C.byref(cfg), C.byref(cs), *[C.byref(o) for o in out]), "vit_rollout_sizes")
    return tuple(o.value for o in out)


class GallerySpec:
    """A gallery request: the k (1..32) rows nearest to the "cls" | "pooled" embedding behind layer `tap`, read as a
    FeatureSpec((tap,), final_norm, l2_normalize) would give it.  The rows themselves (n_rows, row_stride in elements,
    dtype "f32" | "bf16", d_rows a device pointer) are filled in by ViTHip.set_gallery from the array it is given."""

    def __init__(self, k: int = 5, source: str = "cls", tap: int = -1, final_norm: bool = True, l2_normalize: bool = True,
                 dtype: str = "f32", n_rows: int = 0, row_stride: int = 0, d_rows=None):
        self.k, self.source, self.tap = int(k), source, int(tap)
        self.final_norm, self.l2_normalize = bool(final_norm), bool(l2_normalize)
        self.dtype, self.n_rows, self.row_stride, self.d_rows = dtype, int(n_rows), int(row_stride), d_rows

    def c_struct(self) -> GallerySpecC:
        return GallerySpecC(GALLERY_SOURCES[self.source], self.tap, int(self.final_norm), int(self.l2_normalize), self.k,
                            GALLERY_DTYPES[self.dtype], self.n_rows, self.row_stride, _device_ptr(self.d_rows))


def gallery_check(cfg: "VitConfig", spec: GallerySpec) -> int:
    """vit_gallery_check -> device scratch bytes per image of max_batch; raises VitHipError with the library's message"""
    out = C.c_size_t()
    cs = spec.c_struct()
    check(lib().vit_gallery_check(C.byref(cfg), C.byref(cs), C.byref(out)), "vit_gallery_check")
    return out.value


class DenseSpec:
    """A dense request: a label per pixel of an out_h x out_w map (0: the model's img_size) from a linear head of n_labels
    (2..256) rows over the patch tokens behind layer `tap`, read as a FeatureSpec((tap,), final_norm) would give them.  The
    head (weight_stride in elements, d_weight / d_bias device pointers) is filled in by ViTHip.set_dense from the arrays
    it is given."""

    def __init__(self, n_labels: int = 0, out_h: int = 0, out_w: int = 0, tap: int = -1, final_norm: bool = True,
                 weight_stride: int = 0, d_weight=None, d_bias=None):
        self.n_labels, self.out_h, self.out_w, self.tap = int(n_labels), int(out_h), int(out_w), int(tap)
        self.final_norm, self.weight_stride, self.d_weight, self.d_bias = bool(final_norm), int(weight_stride), d_weight, d_bias

    def c_struct(self) -> DenseSpecC:
        return DenseSpecC(self.tap, int(self.final_norm), self.n_labels, self.out_h, self.out_w, self.weight_stride,
                          _device_ptr(self.d_weight), _device_ptr(self.d_bias))


def dense_sizes(cfg: "VitConfig", spec: DenseSpec):
    """vit_dense_sizes -> (labels bytes, scores elements, patch_logits elements, scratch bytes) per image; raises
    VitHipError with the library's message"""
    out = [C.c_size_t() for _ in range(4)]
    cs = spec.c_struct()
    check(lib().vit_dense_sizes(C.byref(cfg), C.byref(cs), *[C.byref(o) for o in out]), "vit_dense_sizes")
    return tuple(o.value for o in out)


def dense_soft_check(cfg: "VitConfig", spec: DenseSpec, logit_scale: float = 1.0, d_values=None) -> int:
    """vit_dense_soft_check -> elements of one soft map per image; raises VitHipError with the library's message"""
    out = C.c_size_t()
    cs, soft = spec.c_struct(), DenseSoftSpecC(float(logit_scale), _device_ptr(d_values))
    check(lib().vit_dense_soft_check(C.byref(cfg), C.byref(cs), C.byref(soft), C.byref(out)), "vit_dense_soft_check")
    return out.value


def frame_soft_check(cfg: "VitConfig", spec: DenseSpec, frame_h: int, frame_w: int, n_windows: int, logit_scale: float = 1.0,
                     d_values=None, fill_label: int = 255) -> int:
    """vit_frame_soft_check -> elements of one soft map of the frame; raises VitHipError with the library's message"""
    out = C.c_size_t()
    fs, soft = FrameSpecC(spec.c_struct(), int(fill_label)), DenseSoftSpecC(float(logit_scale), _device_ptr(d_values))
    check(lib().vit_frame_soft_check(C.byref(cfg), C.byref(fs), C.byref(soft), frame_h, frame_w, n_windows, C.byref(out)),
          "vit_frame_soft_check")
    return out.value


def _pos_mode(mode) -> int:
    """a mode by name, or its number handed through (the refusals of unknown numbers are the library's)"""
    return POS_MODES[mode] if isinstance(mode, str) else int(mode)


def resample_check(cfg: "VitConfig", img_size, mode="bicubic", align_corners=False) -> "VitConfig":
    """vit_resample_check -> cfg at img_size, or with img_size a (height, width) pair vit_resample_check_hw -> cfg at that
    size; raises VitHipError with the library's message"""
    how, out = PosResampleC(_pos_mode(mode), int(align_corners)), VitConfig()
    if isinstance(img_size, (tuple, list)):
        h, w = img_size
        check(lib().vit_resample_check_hw(C.byref(cfg), int(h), int(w), C.byref(how), C.byref(out)), "vit_resample_check_hw")
    else:
        check(lib().vit_resample_check(C.byref(cfg), int(img_size), C.byref(how), C.byref(out)), "vit_resample_check")
    return out


def canonical_config(cfg: "VitConfig") -> "VitConfig":
    """vit_config_canonical: cfg as the library stores it (img_width == img_size as 0); raises VitHipError for a bad width"""
    out = VitConfig()
    check(lib().vit_config_canonical(C.byref(cfg), C.byref(out), None), "vit_config_canonical")
    return out


def resample_pos_embed(pos: np.ndarray, prefix: int, in_hw, out_hw, mode="bicubic", align_corners=False) -> np.ndarray:
    """vh_launch_resample_pos_embed on pos [prefix + in_h * in_w][E] float32 -> [prefix + out_h * out_w][E]: uploads,
    launches on the null stream and downloads (tests)."""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    (in_h, in_w), (out_h, out_w) = in_hw, out_hw
    if pos.ndim != 2 or pos.shape[0] != prefix + in_h * in_w:
        raise ValueError(f"resample_pos_embed: pos of shape {pos.shape}, need [{prefix} + {in_h} * {in_w}][E]")
    E = pos.shape[1]
    d_src, d_dst = DeviceBuffer.from_numpy(pos), DeviceBuffer((prefix + out_h * out_w) * E)
    try:
        check(lib().vh_launch_resample_pos_embed(None, d_src.ptr, d_dst.ptr, prefix, in_h, in_w, out_h, out_w, E, _pos_mode(mode),
                                                 int(align_corners)), "vh_launch_resample_pos_embed")
        return d_dst.to_numpy((prefix + out_h * out_w, E))
    finally:
        d_src.free()
        d_dst.free()


def topk_check(cfg: "VitConfig", spec: TopKSpec) -> None:
    """vit_topk_check: raises VitHipError with the library's message when cfg does not take spec"""
    cs = spec.c_struct()
    check(lib().vit_topk_check(C.byref(cfg), C.byref(cs)), "vit_topk_check")


def feature_sizes(cfg: "VitConfig", spec: FeatureSpec):
    """vit_feature_sizes -> (cls, pooled, tokens) elements per image"""
    out = [C.c_size_t() for _ in range(3)]
    cs = spec.c_struct()
    check(lib().vit_feature_sizes(C.byref(cfg), C.byref(cs), *[C.byref(o) for o in out]), "vit_feature_sizes")
    return tuple(o.value for o in out)


def resize_crop(resize_short: int, filter: str = "bilinear") -> ResizeCrop:
    return ResizeCrop(int(resize_short), RESIZE_FILTERS[filter])


def resize_crop_geometry(height: int, width: int, resize_short: int, crop: int, filter: str = "bilinear"):
    """vit_resize_crop_geometry -> (resized_h, resized_w, top, left)"""
    out = [C.c_int() for _ in range(4)]
    rc = resize_crop(resize_short, filter)
    check(lib().vit_resize_crop_geometry(height, width, C.byref(rc), crop, *[C.byref(o) for o in out]), "vit_resize_crop_geometry")
    return tuple(o.value for o in out)


def box_array(boxes) -> C.Array:
    """An array of vit_box_u8 from (image, (left, top, right, bottom)) pairs, or from Box structures."""
    arr = (Box * len(boxes))()
    for i, b in enumerate(boxes):
        arr[i] = b if isinstance(b, Box) else Box(int(b[0]), (C.c_float * 4)(*[float(v) for v in b[1]]))
    return arr


def box_check(height: int, width: int, box) -> None:
    """vit_box_check: raises VitHipError unless (left, top, right, bottom) is a box of a height x width image"""
    check(lib().vit_box_check(height, width, (C.c_float * 4)(*[float(v) for v in box])), "vit_box_check")


def box_rows(height: int, top: float, bottom: float, out: int, filter: str = "bilinear"):
    """vit_box_rows -> (first, count): the source rows that the `out` output rows of a box from top to bottom read"""
    first, count = C.c_int(), C.c_int()
    check(lib().vit_box_rows(height, top, bottom, out, RESIZE_FILTERS[filter], C.byref(first), C.byref(count)), "vit_box_rows")
    return first.value, count.value


def tile_boxes(h: int, w: int, tile: int, stride: int, image: int = 0):
    """vit_tile_boxes -> [(image, (left, top, right, bottom)), ...]: row-major tile x tile boxes every `stride` px, the last
    row and column flush to the bottom and right edges"""
    n = lib().vit_tile_boxes(h, w, tile, stride, image, None, 0)
    if n < 0:
        check(1, "vit_tile_boxes")
    arr = (Box * n)()
    if lib().vit_tile_boxes(h, w, tile, stride, image, arr, n) != n:
        check(1, "vit_tile_boxes")
    return [(b.image, tuple(b.box)) for b in arr]


def _boxes4(boxes) -> np.ndarray:
    """[n][4] float32 (left, top, right, bottom) from an array of that shape or from (image, box) pairs"""
    if len(boxes) and isinstance(boxes[0], (tuple, list)) and len(boxes[0]) == 2 and not np.isscalar(boxes[0][1]):
        boxes = [b[1] for b in boxes]
    return np.ascontiguousarray(np.asarray(boxes, dtype=np.float32).reshape(-1, 4))


def stitch_check(frame_h: int, frame_w: int, boxes) -> None:
    """vit_stitch_check: raises VitHipError unless every box is a window of a frame_h x frame_w frame"""
    b = _boxes4(boxes)
    check(lib().vit_stitch_check(frame_h, frame_w, fptr(b), len(b), b"vit_stitch_check"), "vit_stitch_check")


def stitch_index(frame_h: int, frame_w: int, boxes, block: int = STITCH_BLOCK):
    """vit_stitch_index -> (offsets int32 [blocks_y * blocks_x + 1], ids int32): per block of block x block frame pixels,
    row-major, the strictly ascending indices of the windows (boxes: [n][4] left, top, right, bottom, or (image, box) pairs)
    that cover at least one pixel centre of the block -- what vh_launch_dense_stitch takes for block = STITCH_BLOCK"""
    b = _boxes4(boxes)
    L = lib()
    n = L.vit_stitch_index(frame_h, frame_w, block, fptr(b), len(b), None, None, 0)
    if n < 0:
        check(1, "vit_stitch_index")
    blocks = -(-frame_h // block) * -(-frame_w // block)
    offsets, ids = np.zeros(blocks + 1, dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
    ip = C.POINTER(C.c_int)
    if L.vit_stitch_index(frame_h, frame_w, block, fptr(b), len(b), offsets.ctypes.data_as(ip), ids.ctypes.data_as(ip), n) != n:
        check(1, "vit_stitch_index")
    return offsets, ids[:n]


def image_descs(images) -> C.Array:
    """An array of vit_image_u8 from (data pointer, height, width, row_stride) tuples (device forms)."""
    arr = (ImageU8 * len(images))()
    for i, (ptr, h, w, stride) in enumerate(images):
        arr[i] = ImageU8(int(ptr.value if isinstance(ptr, C.c_void_p) else ptr), h, w, stride)
    return arr


def host_image_descs(images, layout: str):
    """vit_image_u8 for uint8 host arrays, [h][w][C] (hwc) or [C][h][w] (chw); padded rows are passed as they are, other
    strides are made contiguous.  Returns (array, arrays kept alive)."""
    keep = []
    arr = (ImageU8 * len(images))()
    for i, a in enumerate(images):
        a = np.asarray(a)
        if a.dtype != np.uint8 or a.ndim != 3:
            raise ValueError(f"image {i}: need a 3-d uint8 array, got {a.dtype} {a.shape}")
        if layout == "hwc":
            h, w, ch = a.shape
            ok = a.strides[2] == 1 and a.strides[1] == ch and a.strides[0] >= w * ch
        else:
            ch, h, w = a.shape
            ok = a.strides[2] == 1 and a.strides[1] >= w and a.strides[0] == h * a.strides[1]
        if not ok:
            a = np.ascontiguousarray(a)
        keep.append(a)
        arr[i] = ImageU8(a.ctypes.data, h, w, a.strides[0] if layout == "hwc" else a.strides[1])
    return arr, keep


class VitHipError(RuntimeError):
    pass


def build_library(force: bool = False) -> Path:
    """Compile csrc/ into libvit_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    srcs = list(CSRC.glob("*.hip")) + list(CSRC.glob("*.c")) + list(CSRC.glob("*.h")) + \
        list((PKG_DIR.parent / "include").glob("*.h"))
    stale = (not LIB_PATH.exists()) or any(s.stat().st_mtime > LIB_PATH.stat().st_mtime for s in srcs)
    if force or stale:
        r = subprocess.run(["make", "-C", str(CSRC), "-j8"], capture_output=True, text=True)
        if r.returncode != 0:
            raise VitHipError("building libvit_hip.so failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    return LIB_PATH


_lib = None


def lib() -> C.CDLL:
    """Load libvit_hip.so (no silent fallback: a missing library is an error)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise VitHipError(f"{LIB_PATH} is missing: run __graft_entry__.build() (make -C {CSRC})")
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so (same
    # SONAME as /opt/rocm's).  If torch is going to live in this process it must be
    # loaded FIRST so that libvit_hip.so binds to the runtime torch uses -- otherwise
    # torch-allocated HBM and our streams would belong to two different runtimes.
    if os.environ.get("VIT_HIP_NO_TORCH", "0") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    # VIT_HIP_LIB: a differently built copy of the same library (kernel tuning experiments only)
    _lib = declare(C.CDLL(os.environ.get("VIT_HIP_LIB") or str(LIB_PATH)))
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        raise VitHipError(f"{what} failed with status {rc}: {lib().vh_last_error().decode()}")


def fptr(a: np.ndarray):
    assert a.dtype == np.float32 and a.flags.c_contiguous, "need contiguous float32"
    return a.ctypes.data_as(f32p)


def preset(name: str) -> VitConfig:
    cfg = VitConfig()
    if lib().vit_config_preset(C.byref(cfg), name.encode()) != 0:
        raise ValueError(f"unknown preset {name}")
    return cfg


def tokens(cfg: VitConfig) -> int:
    return lib().vit_config_tokens(C.byref(cfg))


def synth_weights(cfg: VitConfig, seed_base: int = 0) -> list[np.ndarray]:
    L = lib()
    out = []
    for idx in range(L.vit_config_num_tensors(C.byref(cfg))):
        a = np.empty(L.vit_config_tensor_size(C.byref(cfg), idx), dtype=np.float32)
        L.vit_synth_tensor(C.byref(cfg), idx, seed_base, fptr(a))
        out.append(a)
    return out


def synth_images(cfg: VitConfig, first: int, count: int) -> np.ndarray:
    L = lib()
    a = np.empty(cfg.image_shape(count), dtype=np.float32)
    for i in range(count):
        L.vit_synth_image(C.byref(cfg), first + i, fptr(a[i]))
    return a


def pixel_norm(mean, std) -> PixelNorm:
    """vit_pixel_norm_from_mean_std: mean and std per channel on the 0..1 scale (torchvision's Normalize)."""
    mean = np.ascontiguousarray(mean, dtype=np.float32)
    std = np.ascontiguousarray(std, dtype=np.float32)
    if mean.shape != std.shape or mean.ndim != 1:
        raise ValueError("mean and std: one value per channel each")
    out = PixelNorm()
    check(lib().vit_pixel_norm_from_mean_std(C.byref(out), fptr(mean), fptr(std), mean.size), "vit_pixel_norm_from_mean_std")
    return out


def networks(weights: list[np.ndarray]):
    arr = (Network * len(weights))()
    for i, w in enumerate(weights):
        arr[i].data = fptr(w)
        arr[i].size = w.size
    return arr


def image_array(images: np.ndarray):
    """[n][C][H][W] float32 -> ImageData[n] borrowing the numpy rows (like Network.c:86-90)."""
    n, c, h, w = images.shape
    arr = (ImageData * n)()
    for i in range(n):
        arr[i].n, arr[i].c, arr[i].h, arr[i].w = n, c, h, w
        arr[i].data = fptr(images[i])
    return arr


class DeviceBuffer:
    """A vh_malloc'd buffer of `count` float32 values (or of another dtype: np.uint8 for 8-bit images) with explicit copies
    (no hidden host mirror)."""

    def __init__(self, count: int, dtype=np.float32):
        self.count = int(count)
        self.dtype = np.dtype(dtype)
        self.ptr = voidp()
        check(lib().vh_malloc(C.byref(self.ptr), max(self.count, 1) * self.dtype.itemsize), "vh_malloc")

    @classmethod
    def from_numpy(cls, a: np.ndarray, dtype=np.float32) -> "DeviceBuffer":
        a = np.ascontiguousarray(a, dtype=dtype)
        d = cls(a.size, dtype)
        check(lib().vh_h2d(d.ptr, a.ctypes.data_as(voidp), a.nbytes, None), "vh_h2d")
        check(lib().vh_device_sync(), "vh_device_sync")
        return d

    def to_numpy(self, shape=None) -> np.ndarray:
        out = np.empty(self.count, dtype=self.dtype)
        check(lib().vh_d2h(out.ctypes.data_as(voidp), self.ptr, out.nbytes, None), "vh_d2h")
        check(lib().vh_device_sync(), "vh_device_sync")
        return out.reshape(shape) if shape is not None else out

    def free(self):
        if self.ptr:
            lib().vh_free(self.ptr)
            self.ptr = voidp()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _device_ptr(b):
    return b.ptr if isinstance(b, DeviceBuffer) else b


def _host_ptr(a):
    return a.ctypes.data


class ViTHip:
    """Resident-weights context (vit_hip_create / forward / destroy)."""

    PRECISIONS, OP_NAMES = PRECISIONS, OP_NAMES     # abi.py's, under the names callers know

    def __init__(self, cfg: VitConfig, weights: list[np.ndarray], device: int = 0, max_batch: int = 64,
                 precision: str = "f32"):
        self.cfg = cfg
        self.L = lib()
        self._weights = weights  # keep host arrays alive during create
        self.ctx = voidp()
        self.precision = precision
        rc = self.L.vit_hip_create_ex(C.byref(self.ctx), C.byref(cfg), networks(weights), len(weights),
                                      device, max_batch, self.PRECISIONS[precision])
        check(rc, "vit_hip_create_ex")
        self.max_batch = max_batch
        self.tokens = tokens(cfg)

    @classmethod
    def from_planes(cls, path, device: int = 0, max_batch: int = 64) -> "ViTHip":
        """A context from ONE repacked-weights file (vit_hip_export_planes / vit_hip_create_from_planes)."""
        self = cls.__new__(cls)
        self.L, self._weights, self.ctx = lib(), None, voidp()
        check(self.L.vit_hip_create_from_planes(C.byref(self.ctx), str(path).encode(), device, max_batch),
              "vit_hip_create_from_planes")
        self.cfg = VitConfig.from_buffer_copy(self.L.vit_hip_config(self.ctx).contents)
        self.precision = {v: k for k, v in cls.PRECISIONS.items()}[self.L.vit_hip_precision(self.ctx)]
        self.max_batch, self.tokens = max_batch, tokens(self.cfg)
        return self

    def at_resolution(self, img_size: int, max_batch=None, mode="bicubic", align_corners=False) -> "ViTHip":
        """A NEW context for the same weights at another img_size (vit_hip_create_at_resolution): the position grid
        resampled on the GPU (mode "bicubic" | "bilinear"), every other weight copied device to device.  max_batch None:
        this context's.  This context stays as it is and may be closed before or after the new one."""
        new = type(self).__new__(type(self))
        new.L, new._weights, new.ctx = self.L, None, voidp()
        how = PosResampleC(_pos_mode(mode), int(align_corners))
        check(self.L.vit_hip_create_at_resolution(C.byref(new.ctx), self.ctx, int(img_size), int(max_batch or 0), C.byref(how)),
              "vit_hip_create_at_resolution")
        return self._derived(new)

    def _derived(self, new: "ViTHip") -> "ViTHip":
        new.cfg = VitConfig.from_buffer_copy(self.L.vit_hip_config(new.ctx).contents)
        new.precision = self.precision
        new.max_batch, new.tokens = self.L.vit_hip_max_batch(new.ctx), tokens(new.cfg)
        return new

    def at_size(self, height: int, width: int, max_batch=None, mode="bicubic", align_corners=False) -> "ViTHip":
        """at_resolution for an input of height rows by width columns (vit_hip_create_at_size); this context may itself be
        non-square."""
        new = type(self).__new__(type(self))
        new.L, new._weights, new.ctx = self.L, None, voidp()
        how = PosResampleC(_pos_mode(mode), int(align_corners))
        check(self.L.vit_hip_create_at_size(C.byref(new.ctx), self.ctx, int(height), int(width), int(max_batch or 0), C.byref(how)),
              "vit_hip_create_at_size")
        return self._derived(new)

    def check_images(self, images: np.ndarray, layout: str = "chw", who: str = "forward") -> None:
        """ValueError unless images is [n][C][H][W] ("chw": fp32, or bytes) or [n][H][W][C] ("hwc": bytes) of this context's
        H = img_size rows, W = width columns and C = in_chans"""
        want = self.cfg.image_shape(images.shape[0] if images.ndim else 0, layout)
        if images.shape != want:
            raise ValueError(f"{who}: images of shape {images.shape}, the context's config takes {want} ({layout})")

    def weight(self, idx: int) -> np.ndarray:
        """Tensor idx as the context holds it in fp32 (vit_hip_weight), read back to the host."""
        ptr = self.L.vit_hip_weight(self.ctx, int(idx))
        if not ptr:
            raise IndexError(f"weight: no tensor {idx}")
        self.sync()
        out = np.empty(self.L.vit_config_tensor_size(C.byref(self.cfg), int(idx)), dtype=np.float32)
        check(self.L.vh_d2h(out.ctypes.data_as(voidp), ptr, out.nbytes, None), "vh_d2h")
        check(self.L.vh_device_sync(), "vh_device_sync")
        return out

    def export_planes(self, path) -> None:
        check(self.L.vit_hip_export_planes(self.ctx, str(path).encode()), "vit_hip_export_planes")

    @property
    def stream(self):
        return self.L.vit_hip_stream(self.ctx)

    def forward(self, images: np.ndarray):
        """Host-pointer path: [n][C][H][W] -> (logits[n][classes], probs[n][classes])."""
        images = np.ascontiguousarray(images, dtype=np.float32)
        self.check_images(images, "chw", "forward")
        n, nc = images.shape[0], self.cfg.num_classes
        logits = np.empty((n, nc), dtype=np.float32)
        probs = np.empty((n, nc), dtype=np.float32)
        rows = (f32p * n)(*[fptr(probs[i]) for i in range(n)])
        check(self.L.vit_hip_forward(self.ctx, image_array(images), n, fptr(logits), rows), "vit_hip_forward")
        return logits, probs

    def _u8_outputs(self, mean, std, n: int, logits: bool, probs: bool):
        """What the host 8-bit forwards share: the PixelNorm (`mean` may already be one), and for n images the logits and
        probabilities arrays (None where not asked for) with their ctypes arguments."""
        norm = mean if isinstance(mean, PixelNorm) else pixel_norm(mean, std)
        nc = self.cfg.num_classes
        out_l = np.empty((n, nc), dtype=np.float32) if logits else None
        out_p = np.empty((n, nc), dtype=np.float32) if probs else None
        rows = (f32p * n)(*[fptr(out_p[i]) for i in range(n)]) if probs else None
        return norm, out_l, out_p, fptr(out_l) if logits else None, rows

    def forward_u8(self, images: np.ndarray, mean, std, layout: str = "hwc", logits: bool = True, probs: bool = True):
        """Host 8-bit path: [n][H][W][C] (layout "hwc") or [n][C][H][W] ("chw") uint8, normalised on the GPU with
        pixel_norm(mean, std) -> (logits[n][classes], probs[n][classes]); logits=False / probs=False pass NULL and return
        None in that place."""
        cfg = self.cfg
        images = np.ascontiguousarray(images, dtype=np.uint8)
        self.check_images(images, layout, "forward_u8")
        n = images.shape[0]
        norm, out_l, out_p, lp, rows = self._u8_outputs(mean, std, n, logits, probs)
        check(self.L.vit_hip_forward_u8(self.ctx, images.ctypes.data_as(C.POINTER(C.c_ubyte)), n, PIXEL_LAYOUTS[layout],
                                        C.byref(norm), lp, rows), "vit_hip_forward_u8")
        return out_l, out_p

    def forward_device_u8(self, d_images, n: int, norm: PixelNorm, layout: str = "hwc", d_logits=None, d_probs=None,
                          stream=None):
        """Device-resident 8-bit path (d_images: a uint8 DeviceBuffer's .ptr, or any device pointer)."""
        check(self.L.vit_hip_forward_device_u8(self.ctx, d_images, n, PIXEL_LAYOUTS[layout], C.byref(norm), d_logits, d_probs,
                                               stream), "vit_hip_forward_device_u8")

    def forward_u8_resized(self, images, resize_short: int, filter: str = "bilinear", mean=None, std=None, layout: str = "hwc",
                           logits: bool = True, probs: bool = True):
        """Host 8-bit images of any size (a list of [h][w][C] or [C][h][w] uint8 arrays), resized (shorter side to
        resize_short) and centre-cropped on the GPU exactly as Pillow + torchvision's CenterCrop, normalised with
        pixel_norm(mean, std) (or a PixelNorm as `mean`) -> (logits, probs) as forward_u8."""
        n = len(images)
        norm, out_l, out_p, lp, rows = self._u8_outputs(mean, std, n, logits, probs)
        descs, keep = host_image_descs(images, layout)
        rc = resize_crop(resize_short, filter)
        check(self.L.vit_hip_forward_u8_resized(self.ctx, descs, n, PIXEL_LAYOUTS[layout], C.byref(rc), C.byref(norm), lp, rows),
              "vit_hip_forward_u8_resized")
        del keep
        return out_l, out_p

    def forward_device_u8_resized(self, d_images, resize_short: int, norm: PixelNorm, filter: str = "bilinear",
                                  layout: str = "hwc", d_logits=None, d_probs=None, stream=None):
        """Device-resident images of any size: d_images is a list of (device pointer, height, width, row_stride)."""
        rc = resize_crop(resize_short, filter)
        check(self.L.vit_hip_forward_device_u8_resized(self.ctx, image_descs(d_images), len(d_images), PIXEL_LAYOUTS[layout],
                                                       C.byref(rc), C.byref(norm), d_logits, d_probs, stream),
              "vit_hip_forward_device_u8_resized")

    def resize_crop_u8(self, d_images, resize_short: int, d_out, filter: str = "bilinear", layout: str = "hwc", stream=None):
        """The crops alone, [n][img][img][C] bytes into the device buffer d_out."""
        rc = resize_crop(resize_short, filter)
        check(self.L.vit_hip_resize_crop_u8(self.ctx, image_descs(d_images), len(d_images), PIXEL_LAYOUTS[layout], C.byref(rc),
                                            d_out, stream), "vit_hip_resize_crop_u8")

    def forward_u8_boxes(self, images, boxes, filter: str = "bilinear", mean=None, std=None, layout: str = "hwc",
                         logits: bool = True, probs: bool = True):
        """Regions of host 8-bit images: images as forward_u8_resized takes them, boxes a list of (image index, (left, top,
        right, bottom)); every box is resized to img x img on the GPU exactly as Pillow's Image.resize(box=), normalised
        with pixel_norm(mean, std) (or a PixelNorm as `mean`) -> (logits, probs) in box order, as forward_u8."""
        n = len(boxes)
        norm, out_l, out_p, lp, rows = self._u8_outputs(mean, std, n, logits, probs)
        descs, keep = host_image_descs(images, layout)
        check(self.L.vit_hip_forward_u8_boxes(self.ctx, descs, len(images), box_array(boxes), n, PIXEL_LAYOUTS[layout],
                                              RESIZE_FILTERS[filter], C.byref(norm), lp, rows), "vit_hip_forward_u8_boxes")
        del keep
        return out_l, out_p

    def forward_device_u8_boxes(self, d_images, boxes, norm: PixelNorm, filter: str = "bilinear", layout: str = "hwc",
                                d_logits=None, d_probs=None, stream=None):
        """Regions of device-resident images: d_images is a list of (device pointer, height, width, row_stride), boxes a
        list of (image index, (left, top, right, bottom)), at most max_batch of them."""
        check(self.L.vit_hip_forward_device_u8_boxes(self.ctx, image_descs(d_images), len(d_images), box_array(boxes), len(boxes),
                                                     PIXEL_LAYOUTS[layout], RESIZE_FILTERS[filter], C.byref(norm), d_logits,
                                                     d_probs, stream), "vit_hip_forward_device_u8_boxes")

    def crop_boxes_u8(self, d_images, boxes, d_out, filter: str = "bilinear", layout: str = "hwc", stream=None):
        """The boxes' crops alone, [n][img][img][C] bytes into the device buffer d_out."""
        check(self.L.vit_hip_crop_boxes_u8(self.ctx, image_descs(d_images), len(d_images), box_array(boxes), len(boxes),
                                           PIXEL_LAYOUTS[layout], RESIZE_FILTERS[filter], d_out, stream), "vit_hip_crop_boxes_u8")

    def forward_device(self, d_images, n: int, d_logits=None, d_probs=None, stream=None):
        """Device-resident path; pointers are ints / c_void_p / DeviceBuffer.ptr."""
        check(self.L.vit_hip_forward_device(self.ctx, d_images, n, d_logits, d_probs, stream),
              "vit_hip_forward_device")

    def sync(self):
        check(self.L.vh_stream_sync(self.stream), "vh_stream_sync")

    def _arm(self, entry, spec, buffers, arrays, ptr, keep):
        """What the six setters share: the C entry point `entry` gets spec's C struct and the `buffers` struct of
        ptr(array) per array, and the attribute `keep` holds the arrays alive; spec=None disarms."""
        if spec is None:
            cs = bufs = None
        else:
            cs, bufs = C.byref(spec.c_struct()), C.byref(buffers(*[None if a is None else ptr(a) for a in arrays]))
        check(getattr(self.L, entry)(self.ctx, cs, bufs), entry)
        setattr(self, keep, None if spec is None else tuple(arrays))

    def set_features(self, spec, cls=None, pooled=None, tokens=None):
        """Arm (spec=None: disarm) the device forms: cls / pooled / tokens are DeviceBuffers (or device pointers) for up to
        max_batch images, written by every forward_device* until disarmed."""
        self._arm("vit_hip_set_features", spec, FeatureBuffers, (cls, pooled, tokens), _device_ptr, "_feature_keep")

    def set_features_host(self, spec, cls=None, pooled=None, tokens=None):
        """Arm (spec=None: disarm) the host forms: cls / pooled are C-contiguous NumPy arrays of spec.np_dtype for all n
        images of the coming forward / forward_u8 / forward_u8_resized calls."""
        for a in (cls, pooled, tokens):
            if spec is not None and a is not None and not (isinstance(a, np.ndarray) and a.flags.c_contiguous and a.dtype == spec.np_dtype):
                raise ValueError(f"set_features_host: need C-contiguous arrays of {spec.np_dtype}")
        self._arm("vit_hip_set_features_host", spec, FeatureBuffers, (cls, pooled, tokens), _host_ptr, "_feature_keep")

    def embed(self, images: np.ndarray, spec):
        """fp32 images [n][C][H][W] -> (logits, cls, pooled): the host form armed for this one call."""
        n = np.asarray(images).shape[0]
        c_el, p_el, _ = feature_sizes(self.cfg, spec)
        cls = np.empty((n, c_el), dtype=spec.np_dtype)
        pooled = np.empty((n, p_el), dtype=spec.np_dtype)
        self.set_features_host(spec, cls=cls, pooled=pooled)
        try:
            logits, _ = self.forward(images)
        finally:
            self.set_features_host(None)
        return logits, cls, pooled

    def set_topk(self, spec, labels=None, scores=None):
        """Arm (spec=None: disarm) the device forms: labels (int32) / scores (float32, may be None) are DeviceBuffers (or
        device pointers) of [max_batch][k], written by every forward_device* until disarmed."""
        self._arm("vit_hip_set_topk", spec, TopKBuffers, (labels, scores), _device_ptr, "_topk_keep")

    def set_topk_host(self, spec, labels=None, scores=None):
        """Arm (spec=None: disarm) the host forms: labels (int32 [n][k]) / scores (float32 [n][k], may be None) are
        C-contiguous NumPy arrays for all n images of the coming forward / forward_u8 / forward_u8_resized calls."""
        for a, dt in ((labels, np.int32), (scores, np.float32)):
            if spec is not None and a is not None and not (isinstance(a, np.ndarray) and a.flags.c_contiguous and a.dtype == dt):
                raise ValueError("set_topk_host: need C-contiguous int32 labels and float32 scores")
        self._arm("vit_hip_set_topk_host", spec, TopKBuffers, (labels, scores), _host_ptr, "_topk_keep")

    def classify(self, images: np.ndarray, k: int = 5, scores: str = "probs"):
        """fp32 images [n][C][H][W] -> (labels[n][k] int32, scores[n][k] float32): the host form armed for this one call;
        neither logits nor probabilities cross PCIe."""
        images = np.ascontiguousarray(images, dtype=np.float32)
        n = images.shape[0]
        labels, out = np.empty((n, k), dtype=np.int32), np.empty((n, k), dtype=np.float32)
        self.set_topk_host(TopKSpec(k, scores), labels=labels, scores=out)
        try:
            check(self.L.vit_hip_forward(self.ctx, image_array(images), n, None, None), "vit_hip_forward")
        finally:
            self.set_topk_host(None)
        return labels, out

    def set_attention(self, spec, heads=None, mean=None):
        """Arm (spec=None: disarm) the device forms: heads [max_batch][taps][H][T] / mean [max_batch][taps][T] are float32
        DeviceBuffers (or device pointers), either may be None; written by every forward_device* until disarmed."""
        self._arm("vit_hip_set_attention", spec, AttnBuffers, (heads, mean), _device_ptr, "_attention_keep")

    def set_attention_host(self, spec, heads=None, mean=None):
        """Arm (spec=None: disarm) the host forms: heads [n][taps][H][T] / mean [n][taps][T] are C-contiguous float32 NumPy
        arrays for all n images of the coming forward / forward_u8 / forward_u8_resized calls."""
        for a in (heads, mean):
            if spec is not None and a is not None and not (isinstance(a, np.ndarray) and a.flags.c_contiguous and a.dtype == np.float32):
                raise ValueError("set_attention_host: need C-contiguous float32 arrays")
        self._arm("vit_hip_set_attention_host", spec, AttnBuffers, (heads, mean), _host_ptr, "_attention_keep")

    def attention(self, images: np.ndarray, taps=(-1,)):
        """fp32 images [n][C][H][W] -> (logits, heads [n][taps][H][T], mean [n][taps][T]): the class token's attention in
        the tapped layers, the host form armed for this one call."""
        images = np.ascontiguousarray(images, dtype=np.float32)
        n, spec = images.shape[0], AttentionSpec(taps)
        heads = np.empty((n, len(spec.taps), self.cfg.num_heads, self.tokens), dtype=np.float32)
        mean = np.empty((n, len(spec.taps), self.tokens), dtype=np.float32)
        self.set_attention_host(spec, heads=heads, mean=mean)
        try:
            logits, _ = self.forward(images)
        finally:
            self.set_attention_host(None)
        return logits, heads, mean

    def set_rollout(self, spec, rollout=None):
        """Arm (spec=None: disarm) the device form: rollout [max_batch][T] is a float32 DeviceBuffer (or device pointer),
        written by every forward_device* until disarmed."""
        self._arm("vit_hip_set_rollout", spec, RolloutBuffers, (rollout,), _device_ptr, "_rollout_keep")

    def set_rollout_host(self, spec, rollout=None):
        """Arm (spec=None: disarm) the host form: rollout [n][T] is a C-contiguous float32 NumPy array for all n images of
        the coming forward / forward_u8 / forward_u8_resized / forward_u8_boxes calls."""
        if spec is not None and rollout is not None and not (isinstance(rollout, np.ndarray) and rollout.flags.c_contiguous
                                                              and rollout.dtype == np.float32):
            raise ValueError("set_rollout_host: need a C-contiguous float32 array")
        self._arm("vit_hip_set_rollout_host", spec, RolloutBuffers, (rollout,), _host_ptr, "_rollout_keep")

    def rollout(self, images: np.ndarray, first_layer: int = 0):
        """fp32 images [n][C][H][W] -> rollout [n][T]: the class token's row of the attention rollout from first_layer on,
        the host form armed for this one call."""
        images = np.ascontiguousarray(images, dtype=np.float32)
        out = np.empty((images.shape[0], self.tokens), dtype=np.float32)
        self.set_rollout_host(RolloutSpec(first_layer), rollout=out)
        try:
            self.forward(images)
        finally:
            self.set_rollout_host(None)
        return out

    def _gallery_rows(self, spec, rows):
        """spec with the rows filled in: a [G][E] float32 array, or uint16 bf16 bits, is uploaded once into a DeviceBuffer
        this object keeps while armed; a DeviceBuffer is taken as spec describes it (dtype, n_rows, row_stride)."""
        if isinstance(rows, DeviceBuffer):
            spec.d_rows = rows
            spec.row_stride = spec.row_stride or self.cfg.embed_dim
            spec.n_rows = spec.n_rows or rows.count // spec.row_stride
            return spec
        rows = np.asarray(rows)
        if rows.ndim != 2 or rows.dtype not in (np.dtype(np.float32), np.dtype(np.uint16)):
            raise ValueError("set_gallery: rows must be a [G][E] float32 array, uint16 bf16 bits, or a DeviceBuffer")
        spec.dtype = "f32" if rows.dtype == np.float32 else "bf16"
        spec.n_rows, spec.row_stride = rows.shape
        spec.d_rows = DeviceBuffer.from_numpy(rows, dtype=rows.dtype)
        return spec

    def set_gallery(self, spec, rows=None, indices=None, scores=None):
        """Arm (spec=None: disarm) the device form: indices (int32) / scores (float32, may be None) are DeviceBuffers (or
        device pointers) of [max_batch][k], written by every forward_device* until disarmed.  rows: see _gallery_rows."""
        if spec is not None:
            spec = self._gallery_rows(spec, rows)
        self._arm("vit_hip_set_gallery", spec, GalleryBuffers, (indices, scores), _device_ptr, "_gallery_keep")
        self._gallery_rows_keep = None if spec is None else spec.d_rows

    def set_gallery_host(self, spec, rows=None, indices=None, scores=None):
        """Arm (spec=None: disarm) the host form: indices (int32 [n][k]) / scores (float32 [n][k], may be None) are
        C-contiguous NumPy arrays for all n images of the coming forward / forward_u8 / forward_u8_resized / _boxes calls."""
        for a, dt in ((indices, np.int32), (scores, np.float32)):
            if spec is not None and a is not None and not (isinstance(a, np.ndarray) and a.flags.c_contiguous and a.dtype == dt):
                raise ValueError("set_gallery_host: need C-contiguous int32 indices and float32 scores")
        if spec is not None:
            spec = self._gallery_rows(spec, rows)
        self._arm("vit_hip_set_gallery_host", spec, GalleryBuffers, (indices, scores), _host_ptr, "_gallery_keep")
        self._gallery_rows_keep = None if spec is None else spec.d_rows

    def search(self, images: np.ndarray, rows, k: int = 5, source: str = "cls", tap: int = -1, final_norm: bool = True,
               l2_normalize: bool = True):
        """fp32 images [n][C][H][W] -> (indices[n][k] int32, scores[n][k] float32): the k rows of the gallery `rows` nearest
        to every image's embedding, the host form armed for this one call; no embedding crosses PCIe."""
        images = np.ascontiguousarray(images, dtype=np.float32)
        n = images.shape[0]
        indices, out = np.empty((n, k), dtype=np.int32), np.empty((n, k), dtype=np.float32)
        self.set_gallery_host(GallerySpec(k, source, tap, final_norm, l2_normalize), rows, indices=indices, scores=out)
        try:
            check(self.L.vit_hip_forward(self.ctx, image_array(images), n, None, None), "vit_hip_forward")
        finally:
            self.set_gallery_host(None)
        return indices, out

    def _dense_head(self, spec, weight, bias):
        """spec with the head filled in: a [C][E] float32 weight and a [C] bias (or None) are uploaded once into
        DeviceBuffers this object keeps while armed; DeviceBuffers are taken as spec describes them."""
        if isinstance(weight, DeviceBuffer):
            spec.d_weight, spec.d_bias = weight, bias
            spec.weight_stride = spec.weight_stride or self.cfg.embed_dim
            spec.n_labels = spec.n_labels or weight.count // spec.weight_stride
            return spec
        weight = np.asarray(weight)
        if weight.ndim != 2 or weight.dtype != np.float32 or (bias is not None and np.asarray(bias).shape != weight.shape[:1]):
            raise ValueError("set_dense: weight must be a [C][E] float32 array (or a DeviceBuffer), bias [C] or None")
        spec.n_labels, spec.weight_stride = weight.shape
        spec.d_weight = DeviceBuffer.from_numpy(weight)
        spec.d_bias = None if bias is None else DeviceBuffer.from_numpy(np.asarray(bias, dtype=np.float32))
        return spec

    def set_dense(self, spec, weight=None, bias=None, labels=None, scores=None, patch_logits=None):
        """Arm (spec=None: disarm) the device form: labels (uint8 [max_batch][out_h][out_w]), scores (float32, the same
        shape, may be None) and patch_logits (float32 [max_batch][T-1][n_labels], may be None) are DeviceBuffers (or device
        pointers), written by every forward_device* until disarmed.  weight, bias: see _dense_head."""
        if spec is not None:
            spec = self._dense_head(spec, weight, bias)
        self._arm("vit_hip_set_dense", spec, DenseBuffers, (labels, scores, patch_logits), _device_ptr, "_dense_keep")
        self._dense_head_keep = None if spec is None else (spec.d_weight, spec.d_bias)

    def set_dense_host(self, spec, weight=None, bias=None, labels=None):
        """Arm (spec=None: disarm) the host form: labels is a C-contiguous uint8 [n][out_h][out_w] NumPy array for all n
        images of the coming forward / forward_u8 / forward_u8_resized / _boxes calls."""
        if spec is not None and not (isinstance(labels, np.ndarray) and labels.flags.c_contiguous and labels.dtype == np.uint8):
            raise ValueError("set_dense_host: need C-contiguous uint8 labels")
        if spec is not None:
            spec = self._dense_head(spec, weight, bias)
        self._arm("vit_hip_set_dense_host", spec, DenseBuffers, (labels, None, None), _host_ptr, "_dense_keep")
        self._dense_head_keep = None if spec is None else (spec.d_weight, spec.d_bias)

    def segment(self, images: np.ndarray, weight, bias=None, size=None, tap: int = -1, final_norm: bool = True):
        """fp32 images [n][C][H][W] -> labels [n][H][W] uint8: the label a linear head (weight [C][E], bias [C] or None)
        over the patch tokens gives every pixel of an output of `size` (an int or (height, width); None: the model's
        img_size), the host form armed for this one call."""
        images = np.ascontiguousarray(images, dtype=np.float32)
        n = images.shape[0]
        h, w = (size, size) if isinstance(size, int) else size if size is not None else (self.cfg.img_size, self.cfg.width)
        labels = np.empty((n, h, w), dtype=np.uint8)
        self.set_dense_host(DenseSpec(0, h, w, tap, final_norm), weight, bias, labels=labels)
        try:
            check(self.L.vit_hip_forward(self.ctx, image_array(images), n, None, None), "vit_hip_forward")
        finally:
            self.set_dense_host(None)
        return labels

    def set_dense_soft(self, spec, weight=None, bias=None, soft_scale: float = 1.0, values=None, labels=None, prob=None, expect=None,
                       entropy=None):
        """Arm (spec=None: disarm) the dense request with soft maps attached, device form: prob / expect / entropy are float32
        DeviceBuffers (or device pointers) of [max_batch][out_h][out_w], each may be None, not all; labels (uint8, the same
        shape) may be None, then no labels are written.  soft_scale multiplies the logits before the softmax; values (a
        [C] float32 array or DeviceBuffer: the bin centres) is given exactly when expect is.  weight, bias: see _dense_head."""
        if spec is None:
            check(self.L.vit_hip_set_dense_soft(self.ctx, None, None, None, None), "vit_hip_set_dense_soft")
            self._dense_keep = self._dense_head_keep = None
            return
        spec = self._dense_head(spec, weight, bias)
        if values is not None and not isinstance(values, (DeviceBuffer, int, C.c_void_p)):
            values = DeviceBuffer.from_numpy(np.ascontiguousarray(values, dtype=np.float32))
        soft = DenseSoftSpecC(float(soft_scale), _device_ptr(values))
        bufs = DenseBuffers(_device_ptr(labels), None, None)
        maps = DenseSoftBuffers(_device_ptr(prob), _device_ptr(expect), _device_ptr(entropy))
        cs = spec.c_struct()
        check(self.L.vit_hip_set_dense_soft(self.ctx, C.byref(cs), C.byref(soft), C.byref(bufs), C.byref(maps)), "vit_hip_set_dense_soft")
        self._dense_keep = (labels, prob, expect, entropy)
        self._dense_head_keep = (spec.d_weight, spec.d_bias, values)

    def segment_soft(self, images: np.ndarray, weight, bias=None, values=None, logit_scale: float = 1.0, size=None, tap: int = -1,
                     final_norm: bool = True, outputs=("labels", "prob")):
        """fp32 images [n][C][H][W] -> {name: array [n][H][W]} for the names in `outputs`: "labels" (uint8), "prob" (the
        softmax probability of that label), "expect" (sum_c p_c * values[c]; with values the bin centres of a depth head this
        is the depth map) and "entropy" (nats), float32.  The softmax is over logit_scale times the upsampled logits of the
        linear head (weight [C][E], bias [C] or None) at an output of `size` (an int or (height, width); None: the model's
        img_size).  Chunks of at most max_batch images through the device form, armed for this one call."""
        names = ("labels", "prob", "expect", "entropy")
        outputs = tuple(outputs)
        if not outputs or any(o not in names for o in outputs):
            raise ValueError(f"segment_soft: outputs must be a non-empty subset of {names}")
        images = np.ascontiguousarray(images, dtype=np.float32)
        n, mb = images.shape[0], self.max_batch
        h, w = (size, size) if isinstance(size, int) else size if size is not None else (self.cfg.img_size, self.cfg.width)
        got = {o: np.empty((n, h, w), dtype=np.uint8 if o == "labels" else np.float32) for o in outputs}
        dev = {o: DeviceBuffer(mb * h * w, np.uint8 if o == "labels" else np.float32) for o in outputs}
        d_img = DeviceBuffer(mb * int(np.prod(images.shape[1:])))
        self.set_dense_soft(DenseSpec(0, h, w, tap, final_norm), weight, bias, logit_scale, values, **dev)
        try:
            for a in range(0, n, mb):
                m = min(mb, n - a)
                chunk = images[a:a + m]
                check(self.L.vh_h2d(d_img.ptr, chunk.ctypes.data_as(C.c_void_p), chunk.nbytes, self.stream), "vh_h2d")
                self.forward_device(d_img.ptr, m)
                self.sync()
                for o in outputs:
                    got[o][a:a + m] = dev[o].to_numpy((mb, h, w))[:m]
        finally:
            self.set_dense_soft(None)
        return got

    def _frame_spec(self, weight, bias, tap, final_norm, fill_label, n_labels=0, weight_stride=0):
        """(FrameSpecC, what keeps the head's device arrays alive) for the frame calls: the head as _dense_head makes it"""
        spec = self._dense_head(DenseSpec(n_labels, 0, 0, tap, final_norm, weight_stride), weight, bias)
        return FrameSpecC(spec.c_struct(), int(fill_label)), (spec.d_weight, spec.d_bias)

    def segment_frame_device(self, d_frame, windows, norm: PixelNorm, weight, bias=None, labels=None, scores=None, cover=None,
                             filter: str = "bilinear", layout: str = "hwc", tap: int = -1, final_norm: bool = True,
                             fill_label: int = 255, n_labels: int = 0, weight_stride: int = 0):
        """vit_hip_segment_frame_device_u8: d_frame is (device pointer, height, width, row_stride), windows a list of (0,
        (left, top, right, bottom)); labels (uint8 [H][W]), scores (float32, may be None) and cover (uint8, may be None)
        are DeviceBuffers or device pointers; a head given as DeviceBuffers has n_labels rows weight_stride elements apart
        (0: embed_dim, and as many rows as the buffer holds).  Complete on return."""
        fs, keep = self._frame_spec(weight, bias, tap, final_norm, fill_label, n_labels, weight_stride)
        bufs = FrameBuffers(_device_ptr(labels), _device_ptr(scores), _device_ptr(cover))
        check(self.L.vit_hip_segment_frame_device_u8(self.ctx, image_descs([d_frame]), box_array(windows), len(windows),
                                                     PIXEL_LAYOUTS[layout], RESIZE_FILTERS[filter], C.byref(norm), C.byref(fs),
                                                     C.byref(bufs)), "vit_hip_segment_frame_device_u8")
        del keep

    def segment_frame(self, frame, weight, bias=None, tile=None, stride=None, windows=None, filter: str = "bilinear", mean=None,
                      std=None, layout: str = "hwc", tap: int = -1, final_norm: bool = True, fill_label: int = 255,
                      scores: bool = False, cover: bool = False):
        """A whole 8-bit frame ([H][W][C] uint8, or [C][H][W] with layout "chw") -> labels [H][W] uint8: the sliding-window
        protocol on the GPU.  The windows (a list of (0, (left, top, right, bottom)); None: tile_boxes(H, W, tile or the
        model's img_size, stride or 2 * tile // 3)) are resized as forward_u8_boxes resizes them, normalised with
        pixel_norm(mean, std) (or a PixelNorm as `mean`) and run through the model; a linear head (weight [C][E], bias [C]
        or None, as segment takes them) gives every patch its logits, which are upsampled to the window's box, averaged
        where windows overlap and ranked per frame pixel.  A pixel no window covers gets fill_label.  scores=True / cover=True:
        returns (labels, scores float32 [H][W] or None, cover uint8 [H][W] or None) -- the winning mean logit and the number
        of windows over the pixel."""
        descs, keep = host_image_descs([frame], layout)
        H, W = descs[0].height, descs[0].width
        if windows is None:
            tile = int(tile or self.cfg.img_size)
            windows = tile_boxes(H, W, tile, int(stride or 2 * tile // 3))
        norm = mean if isinstance(mean, PixelNorm) else pixel_norm(mean, std)
        fs, head_keep = self._frame_spec(weight, bias, tap, final_norm, fill_label)
        out_l = np.empty((H, W), dtype=np.uint8)
        out_s = np.empty((H, W), dtype=np.float32) if scores else None
        out_c = np.empty((H, W), dtype=np.uint8) if cover else None
        bufs = FrameBuffers(*[None if a is None else _host_ptr(a) for a in (out_l, out_s, out_c)])
        check(self.L.vit_hip_segment_frame_u8(self.ctx, descs, box_array(windows), len(windows), PIXEL_LAYOUTS[layout],
                                              RESIZE_FILTERS[filter], C.byref(norm), C.byref(fs), C.byref(bufs)),
              "vit_hip_segment_frame_u8")
        del keep, head_keep
        return (out_l, out_s, out_c) if scores or cover else out_l

    def segment_frame_soft_device(self, d_frame, windows, norm: PixelNorm, weight, bias=None, values=None, logit_scale: float = 1.0,
                                  prob=None, expect=None, entropy=None, labels=None, scores=None, cover=None, filter: str = "bilinear",
                                  layout: str = "hwc", tap: int = -1, final_norm: bool = True, fill_label: int = 255, n_labels: int = 0,
                                  weight_stride: int = 0):
        """vit_hip_segment_frame_soft_device_u8: segment_frame_device's arguments, plus prob / expect / entropy (float32 [H][W]
        DeviceBuffers or device pointers; each may be None, not all) and values (a [C] float32 array or DeviceBuffer, given
        exactly when expect is).  labels may be None: then no labels are written, and scores and cover must be None too.
        Complete on return."""
        fs, keep = self._frame_spec(weight, bias, tap, final_norm, fill_label, n_labels, weight_stride)
        if values is not None and not isinstance(values, (DeviceBuffer, int, C.c_void_p)):
            values = DeviceBuffer.from_numpy(np.ascontiguousarray(values, dtype=np.float32))
        soft = DenseSoftSpecC(float(logit_scale), _device_ptr(values))
        bufs = FrameBuffers(_device_ptr(labels), _device_ptr(scores), _device_ptr(cover))
        maps = DenseSoftBuffers(_device_ptr(prob), _device_ptr(expect), _device_ptr(entropy))
        check(self.L.vit_hip_segment_frame_soft_device_u8(self.ctx, image_descs([d_frame]), box_array(windows), len(windows),
                                                          PIXEL_LAYOUTS[layout], RESIZE_FILTERS[filter], C.byref(norm), C.byref(fs),
                                                          C.byref(soft), C.byref(bufs), C.byref(maps)),
              "vit_hip_segment_frame_soft_device_u8")
        del keep, values

    def segment_frame_soft(self, frame, weight, bias=None, values=None, logit_scale: float = 1.0, tile=None, stride=None, windows=None,
                           want=("prob",), labels: bool = True, scores: bool = False, cover: bool = False, filter: str = "bilinear",
                           mean=None, std=None, layout: str = "hwc", tap: int = -1, final_norm: bool = True, fill_label: int = 255):
        """A whole 8-bit frame -> {name: array [H][W]}: segment_frame's sliding-window protocol followed by its softmax.  `want`
        names the float32 maps: "prob" (the softmax probability of the pixel's label), "expect" (sum_c p_c * values[c]: with
        values the bin centres of a depth head, the depth map) and "entropy" (nats), over logit_scale times the mean of the
        covering windows' logits; a pixel no window covers is NaN in all of them.  labels / scores / cover add segment_frame's
        outputs under those names (scores and cover need labels).  frame, weight, bias, tile, stride, windows and the rest as
        segment_frame takes them."""
        names = ("prob", "expect", "entropy")
        want = tuple(want)
        if not want or any(o not in names for o in want):
            raise ValueError(f"segment_frame_soft: want must be a non-empty subset of {names}")
        if ("expect" in want) != (values is not None):
            raise ValueError("segment_frame_soft: values must be given exactly when \"expect\" is in want")
        if (scores or cover) and not labels:
            raise ValueError("segment_frame_soft: scores and cover need labels")
        descs, keep = host_image_descs([frame], layout)
        H, W = descs[0].height, descs[0].width
        if windows is None:
            tile = int(tile or self.cfg.img_size)
            windows = tile_boxes(H, W, tile, int(stride or 2 * tile // 3))
        norm = mean if isinstance(mean, PixelNorm) else pixel_norm(mean, std)
        fs, head_keep = self._frame_spec(weight, bias, tap, final_norm, fill_label)
        if values is not None and not isinstance(values, (DeviceBuffer, int, C.c_void_p)):
            values = DeviceBuffer.from_numpy(np.ascontiguousarray(values, dtype=np.float32))
        soft = DenseSoftSpecC(float(logit_scale), _device_ptr(values))
        got = {o: np.empty((H, W), dtype=np.float32) for o in want}
        for name, asked, dtype in (("labels", labels, np.uint8), ("scores", scores, np.float32), ("cover", cover, np.uint8)):
            if asked:
                got[name] = np.empty((H, W), dtype=dtype)
        bufs = FrameBuffers(*[_host_ptr(got[o]) if o in got else None for o in ("labels", "scores", "cover")])
        maps = DenseSoftBuffers(*[_host_ptr(got[o]) if o in got else None for o in names])
        check(self.L.vit_hip_segment_frame_soft_u8(self.ctx, descs, box_array(windows), len(windows), PIXEL_LAYOUTS[layout],
                                                   RESIZE_FILTERS[filter], C.byref(norm), C.byref(fs), C.byref(soft), C.byref(bufs),
                                                   C.byref(maps)), "vit_hip_segment_frame_soft_u8")
        del keep, head_keep, values
        return got

    def read_tokens(self, n: int) -> np.ndarray:
        out = np.empty((n * self.tokens, self.cfg.embed_dim), dtype=np.float32)
        check(self.L.vit_hip_read_tokens(self.ctx, n, fptr(out)), "vit_hip_read_tokens")
        return out

    def set_last_layer_cls_only(self, on: bool) -> bool:
        """The older switch for the last layer's output projection and MLP on the class-token rows only (identical logits;
        the default where the plan allows it).  Returns the previous setting of this flag."""
        return bool(self.L.vit_hip_set_last_layer_cls_only(self.ctx, 1 if on else 0))

    def last_layer_pending(self) -> int:
        """Images of the last forward whose last layer ran on the class-token rows only and waits for read_tokens to finish it."""
        return int(self.L.vit_hip_last_layer_pending(self.ctx))

    def profile_enable(self, max_forwards: int):
        check(self.L.vit_hip_profile_enable(self.ctx, max_forwards), "vit_hip_profile_enable")

    def profile_select(self, names=None):
        """Record only these operators (names from OP_NAMES); None = all."""
        mask = 0 if not names else sum(1 << self.OP_NAMES.index(n) for n in names)
        check(self.L.vit_hip_profile_select(self.ctx, mask), "vit_hip_profile_select")

    def profile_read(self) -> dict[str, tuple[float, int]]:
        """-> {operator: (summed ms, launches)} since the last read."""
        k = len(self.OP_NAMES)
        ms, cnt = (C.c_double * k)(), (C.c_long * k)()
        check(self.L.vit_hip_profile_read(self.ctx, ms, cnt), "vit_hip_profile_read")
        return {name: (ms[j], cnt[j]) for j, name in enumerate(self.OP_NAMES)}

    def close(self):
        if self.ctx:
            self.L.vit_hip_destroy(self.ctx)
            self.ctx = voidp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ViTHipMulti:
    """One replica per device behind one call (vit_hip_create_multi / forward_multi / destroy_multi)."""

    def __init__(self, cfg: VitConfig, weights: list[np.ndarray], devices: list[int], max_batch_per_device: int = 64,
                 precision: str = "f32"):
        self.cfg, self.L = cfg, lib()
        self.handle = voidp()
        devs = (C.c_int * len(devices))(*devices)
        check(self.L.vit_hip_create_multi(C.byref(self.handle), C.byref(cfg), networks(weights), len(weights), devs,
                                          len(devices), max_batch_per_device,
                                          PRECISIONS[precision]), "vit_hip_create_multi")

    def forward(self, images: np.ndarray):
        images = np.ascontiguousarray(images, dtype=np.float32)
        n, nc = images.shape[0], self.cfg.num_classes
        logits = np.empty((n, nc), dtype=np.float32)
        probs = np.empty((n, nc), dtype=np.float32)
        rows = (f32p * n)(*[fptr(probs[i]) for i in range(n)])
        check(self.L.vit_hip_forward_multi(self.handle, image_array(images), n, fptr(logits), rows), "vit_hip_forward_multi")
        return logits, probs

    def forward_device(self, d_images: list, counts: list[int], d_logits_root, d_probs_root=None):
        """Device-resident shards (d_images[g] on device g), logits gathered onto device 0 over RCCL (C side)."""
        n = len(counts)
        ptrs = (voidp * n)(*[p if isinstance(p, voidp) else voidp(p) for p in d_images])
        check(self.L.vit_hip_forward_device_multi(self.handle, ptrs, (C.c_int * n)(*counts), d_logits_root, d_probs_root),
              "vit_hip_forward_device_multi")

    def last_enqueue_ms(self) -> list[float]:
        """Host milliseconds each device's thread spent enqueuing its shard in the last forward_device."""
        ms = (C.c_double * 64)()
        n = self.L.vit_hip_multi_last_enqueue_ms(self.handle, ms, 64)
        return [round(ms[d], 4) for d in range(max(n, 0))]

    def close(self):
        if self.handle:
            self.L.vit_hip_destroy_multi(self.handle)
            self.handle = voidp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shard_range(total: int, rank: int, world: int) -> tuple[int, int]:
    """Contiguous batch shard of rank `rank`: images [lo, hi).  Images never
    interact (the reference processes them strictly one at a time,
    ViT_opencl.c:926), so the batch dimension is the only partition."""
    per = (total + world - 1) // world
    lo = min(rank * per, total)
    return lo, min(lo + per, total)
