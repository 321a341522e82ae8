"""The C ABI of libvit_hip.so, stated once: the struct mirrors, the enum mirrors and one table of every prototype that
include/kernelHandler.h, include/ViT_opencl.h and include/Network.h declare.  declare() applies the table to a loaded
library.  tests/test_abi_host.py parses the headers and compiles a probe from them, and holds every line here to what
they say; a new export is a header declaration and one table line, and that test names whichever is missing."""
from __future__ import annotations

import ctypes as C

P = C.POINTER
i, u, l, sz, ull, f, d = C.c_int, C.c_uint, C.c_long, C.c_size_t, C.c_ulonglong, C.c_float, C.c_double  # noqa: E741
p, s = C.c_void_p, C.c_char_p       # any object or device pointer, a handle (vh_stream_t, vit_hip_ctx *); const char *
voidp = p
f32p = fp = P(f)
pp, fpp, ip, lp, dp, szp, u8p = P(p), P(fp), P(i), P(l), P(d), P(sz), P(C.c_ubyte)

STRUCTS = {}    # C type -> its mirror
ENUMS = []      # (prefix of the C constants, {key: value}, {key: C constant} where it is not prefix + KEY)


def mirrors(ctype: str):
    """class decorator: registers the Structure below it as the mirror of the C type `ctype`"""
    def register(cls):
        STRUCTS[ctype] = cls
        return cls
    return register


def enum(prefix: str, mapping: dict, names: dict | None = None) -> dict:
    """registers `mapping` as the mirror of C constants under `prefix`; returns it"""
    ENUMS.append((prefix, mapping, names))
    return mapping


# ---- include/kernelHandler.h ----
FP32_MATH = enum("VH_FP32_", {"split3": 0, "native": 1})    # fp32_math of vh_launch_linear_math / _patch_embed_ws_math
ATTN_ARITH = enum("VH_ATTN_", {"native": 0, "fp16": 1, "fp16x2": 2, "split3": 3})   # arith of vh_launch_attention_rows
ATTN_KERNEL = enum("VH_ATTN_", {"auto": 0, "streaming": 1})                         # kernel of vh_launch_attention_rows
QKV_FORMS = enum("VH_QKV_", {"rows_f32": 0, "planes3": 1, "planes_f16": 2})         # qkv_form of vh_launch_cls_attention
TOPK_SCORES = enum("VIT_TOPK_", {"probs": 0, "logits": 1})
GALLERY_DTYPES = enum("VH_GALLERY_", {"f32": 0, "bf16": 1})
GALLERY_MAX_SPLITS, GALLERY_ROW_TILE = 1024, 128
enum("VH_GALLERY_", {"max_splits": GALLERY_MAX_SPLITS, "row_tile": GALLERY_ROW_TILE})
DENSE_MAX_LABELS, DENSE_MAX_GRID, DENSE_TOKEN_TILE = 256, 64, 128
enum("VH_DENSE_", {"max_labels": DENSE_MAX_LABELS, "max_grid": DENSE_MAX_GRID, "token_tile": DENSE_TOKEN_TILE})
STITCH_BLOCK, STITCH_MAX_SIDE = 16, 16384
enum("VH_STITCH_", {"block": STITCH_BLOCK, "max_side": STITCH_MAX_SIDE})
POS_MODES = enum("VH_POS_", {"bicubic": 0, "bilinear": 1})
enum("VIT_POS_", POS_MODES)

# ---- include/ViT_opencl.h ----
PRECISIONS = enum("VIT_PRECISION_", {"f32": 0, "bf16": 1, "fp8": 2, "f32_fp16x2": 3},
                  names={"bf16": "VIT_PRECISION_BF16_GEMM", "fp8": "VIT_PRECISION_FP8_GEMM"})
PIXEL_LAYOUTS = enum("VIT_PIXELS_", {"hwc": 0, "chw": 1})
RESIZE_FILTERS = enum("VIT_RESIZE_", {"bilinear": 0, "bicubic": 1})
FEATURE_DTYPES = enum("VIT_FEATURE_", {"f32": 0, "bf16": 1})
TOKEN_LAYOUTS = enum("VIT_TOKENS_", {"nlc": 0, "nchw": 1})
GALLERY_SOURCES = enum("VIT_GALLERY_", {"cls": 0, "pooled": 1})
# enum vit_op_class, in its order: the rows of vit_hip_profile_read
OP_NAMES = ["patch_embed", "layer_norm", "qkv_gemm", "attention", "out_proj_gemm", "fc1_gemm",
            "fc2_gemm", "head_gemm", "softmax", "out_proj_gemm_cls", "fc1_gemm_cls", "fc2_gemm_cls"]
enum("VIT_OP_", {**{name: k for k, name in enumerate(OP_NAMES)}, "count": len(OP_NAMES)},
     names={name: "VIT_OP_" + name.replace("_gemm", "").upper() for name in OP_NAMES if "_gemm" in name})


@mirrors("vit_config")
class VitConfig(C.Structure):
    _fields_ = [
        ("img_size", i), ("patch_size", i), ("in_chans", i), ("num_classes", i), ("embed_dim", i), ("depth", i),
        ("num_heads", i), ("mlp_hidden", i), ("eps", d),
        ("img_width", i),   # 0: img_size (square); otherwise the input is img_size rows by img_width columns
    ]

    @property
    def width(self) -> int:
        """columns of an input image (its rows are img_size)"""
        return self.img_width or self.img_size

    @property
    def grid(self) -> tuple:
        """(gh, gw): the patch grid, row-major (vit_config_grid)"""
        from .binding import lib
        gh, gw = i(), i()
        lib().vit_config_grid(C.byref(self), C.byref(gh), C.byref(gw))
        return gh.value, gw.value

    def image_shape(self, n: int, layout: str = "chw") -> tuple:
        """the shape of n input images: [n][C][H][W] (fp32, and bytes in layout "chw") or [n][H][W][C] (bytes, "hwc")"""
        h, w, ch = self.img_size, self.width, self.in_chans
        return (n, h, w, ch) if layout == "hwc" else (n, ch, h, w)


@mirrors("vit_pos_resample")
class PosResampleC(C.Structure):
    _fields_ = [("mode", i), ("align_corners", i)]


@mirrors("vit_pixel_norm")
class PixelNorm(C.Structure):
    """x = (float)u * scale[c] + bias[c], each step rounded to fp32."""
    _fields_ = [("scale", f * 4), ("bias", f * 4)]


@mirrors("vit_image_u8")
class ImageU8(C.Structure):
    """one 8-bit image of any size; data is a host or device pointer."""
    _fields_ = [("data", p), ("height", i), ("width", i), ("row_stride", l)]


@mirrors("vit_resize_crop")
class ResizeCrop(C.Structure):
    """shorter side resized to resize_short, then the centre crop."""
    _fields_ = [("resize_short", i), ("filter", i)]


@mirrors("vit_box_u8")
class Box(C.Structure):
    """a region (left, top, right, bottom) of image `image` of an images array."""
    _fields_ = [("image", i), ("box", f * 4)]


@mirrors("vit_feature_spec")
class FeatureSpecC(C.Structure):
    _fields_ = [("n_taps", i), ("taps", i * 4), ("final_norm", i), ("l2_normalize", i), ("dtype", i), ("token_layout", i)]


@mirrors("vit_feature_buffers")
class FeatureBuffers(C.Structure):
    """device or host pointers, each may be NULL."""
    _fields_ = [("cls", p), ("pooled", p), ("tokens", p)]


@mirrors("vit_topk_spec")
class TopKSpecC(C.Structure):
    _fields_ = [("k", i), ("score_kind", i)]


@mirrors("vit_topk_buffers")
class TopKBuffers(C.Structure):
    """device or host pointers; scores may be NULL."""
    _fields_ = [("labels", p), ("scores", p)]


@mirrors("vit_attn_spec")
class AttnSpecC(C.Structure):
    _fields_ = [("n_taps", i), ("taps", i * 4)]


@mirrors("vit_attn_buffers")
class AttnBuffers(C.Structure):
    """device or host pointers; each may be NULL, not both."""
    _fields_ = [("heads", p), ("mean", p)]


@mirrors("vit_rollout_spec")
class RolloutSpecC(C.Structure):
    _fields_ = [("first_layer", i)]


@mirrors("vit_rollout_buffers")
class RolloutBuffers(C.Structure):
    """a device or host pointer."""
    _fields_ = [("rollout", p)]


@mirrors("vit_gallery_spec")
class GallerySpecC(C.Structure):
    _fields_ = [("source", i), ("tap", i), ("final_norm", i), ("l2_normalize", i), ("k", i), ("dtype", i), ("n_rows", l),
                ("row_stride", l), ("d_rows", p)]


@mirrors("vit_gallery_buffers")
class GalleryBuffers(C.Structure):
    """device or host pointers; scores may be NULL."""
    _fields_ = [("indices", p), ("scores", p)]


@mirrors("vit_dense_spec")
class DenseSpecC(C.Structure):
    _fields_ = [("tap", i), ("final_norm", i), ("n_labels", i), ("out_h", i), ("out_w", i), ("weight_stride", l),
                ("d_weight", p), ("d_bias", p)]


@mirrors("vit_dense_buffers")
class DenseBuffers(C.Structure):
    """device or host pointers; scores and patch_logits may be NULL."""
    _fields_ = [("labels", p), ("scores", p), ("patch_logits", p)]


@mirrors("vit_dense_soft_spec")
class DenseSoftSpecC(C.Structure):
    """logit_scale finite and > 0; d_values [n_labels] fp32 on the device, NULL without expect."""
    _fields_ = [("logit_scale", f), ("d_values", p)]


@mirrors("vit_dense_soft_buffers")
class DenseSoftBuffers(C.Structure):
    """device pointers, fp32 [max_batch][out_h][out_w]; each may be NULL, not all three."""
    _fields_ = [("prob", p), ("expect", p), ("entropy", p)]


@mirrors("vit_frame_spec")
class FrameSpecC(C.Structure):
    """head: a vit_dense_spec whose out_h and out_w are 0; fill_label for pixels no window covers."""
    _fields_ = [("head", DenseSpecC), ("fill_label", i)]


@mirrors("vit_frame_buffers")
class FrameBuffers(C.Structure):
    """device or host pointers, [H][W]; scores and cover may be NULL."""
    _fields_ = [("labels", p), ("scores", p), ("cover", p)]


@mirrors("vit_compare_report")
class CompareReport(C.Structure):
    _fields_ = [("rows", i), ("classes", i), ("max_abs_diff", d), ("mean_abs_diff", d), ("top1_equal", i),
                ("top1_equal_or_near_tie", i), ("top5_overlap", d), ("nonfinite", i)]


# ---- include/Network.h ----
@mirrors("ImageData")
class ImageData(C.Structure):
    """reference Network.h:7-14"""
    _fields_ = [("n", i), ("c", i), ("h", i), ("w", i), ("data", fp)]


@mirrors("Network")
class Network(C.Structure):
    """reference Network.h:19-23"""
    _fields_ = [("data", fp), ("size", sz)]


# int fn(void *arg, int shard, int lo, int hi) -- the callback type of vit_shard_run
SHARD_FN = C.CFUNCTYPE(i, p, i, i, i)


def _fn(name: str, *argtypes, ret=i):
    return name, ret, list(argtypes)


# Every function of the three headers, in the headers' order: (name, return type, [argument types]).
PROTOTYPES = {
    "kernelHandler.h": [
        _fn("vh_device_count"),
        _fn("vh_init", i),
        _fn("vh_last_error", ret=s),
        _fn("vh_set_error", i, s),
        _fn("vh_device_name", ret=s),
        _fn("vh_set_device", i),
        _fn("vh_stream_create", pp),
        _fn("vh_stream_destroy", p),
        _fn("vh_stream_sync", p),
        _fn("vh_device_sync"),
        _fn("vh_event_create", pp),
        _fn("vh_event_destroy", p),
        _fn("vh_event_record", p, p),
        _fn("vh_stream_wait_event", p, p),
        _fn("vh_event_sync", p),
        _fn("vh_event_elapsed_ms", fp, p, p),
        _fn("vh_malloc", pp, sz),
        _fn("vh_free", p),
        _fn("vh_host_alloc", pp, sz),
        _fn("vh_host_free", p),
        _fn("vh_memset", p, i, sz, p),
        _fn("vh_h2d", p, p, sz, p),
        _fn("vh_d2h", p, p, sz, p),
        _fn("vh_d2d", p, p, sz, p),
        _fn("vh_launch_patch_embed", p, p, p, p, p, p, p, i, i, i, i, i),
        _fn("vh_patch_embed_workspace", i, i, i, i, i, ret=sz),
        _fn("vh_launch_patch_embed_ws", p, p, p, p, p, p, p, i, i, i, i, i, p, sz),
        _fn("vh_patch_planes_k", i, i),
        _fn("vh_launch_conv_weight_planes", p, p, p, i, i, i),
        _fn("vh_launch_conv_weight_planes_parts", p, p, p, i, i, i, i),
        _fn("vh_launch_patch_embed_planes3", p, p, p, p, p, p, p, i, i, i, i, i, p, sz),
        _fn("vh_launch_patch_embed_planes", p, p, p, p, p, p, p, i, i, i, i, i, p, sz),
        _fn("vh_launch_layer_norm", p, p, p, p, p, i, i, l, l, d),
        _fn("vh_launch_linear", p, p, p, p, p, i, i, i, i, p),
        _fn("vh_launch_linear_math", p, p, p, p, p, i, i, i, i, p, i),
        _fn("vh_launch_patch_embed_ws_math", p, p, p, p, p, p, p, i, i, i, i, i, p, sz, i),
        _fn("vh_launch_split3_planes", p, p, p, i, i),
        _fn("vh_launch_linear_w3", p, p, p, p, p, i, i, i, i, p),
        _fn("vh_launch_split3_rows", p, p, p, i, i),
        _fn("vh_launch_merge3_rows", p, p, p, i, i),
        _fn("vh_launch_split_rows", p, p, p, i, i, i),
        _fn("vh_launch_merge_rows", p, p, p, i, i, i),
        _fn("vh_layer_norm_planes_max_embed", i),
        _fn("vh_launch_layer_norm_planes", p, p, p, p, p, i, i, i, l, d),
        _fn("vh_launch_attention_planes_bf16", p, p, p, i, i, i, i),
        _fn("vh_launch_linear_planes", p, p, i, p, p, i, p, i, i, i, i, p),
        _fn("vh_launch_layer_norm_p3", p, p, p, p, p, i, i, l, d),
        _fn("vh_launch_attention_p3", p, p, p, i, i, i, i),
        _fn("vh_launch_attention_planes", p, p, p, i, i, i, i),
        _fn("vh_launch_attention_planes_f16", p, p, p, i, i, i, i, i),
        _fn("vh_launch_attention_planes_f16_hd80", p, p, p, i, i, i, i),
        _fn("vh_launch_attention_planes_f16_hd80_operand", p, p, p, p, i, i, i, i, i),
        _fn("vh_launch_attention_long", p, p, i, p, i, i, i, i),
        _fn("vh_launch_linear_p3", p, p, i, p, p, p, i, i, i, i, p),
        _fn("vh_launch_linear_p3_cols", p, p, i, p, i, p, p, i, i, i),
        _fn("vh_launch_attention_planes_cls", p, p, p, p, i, i, i, i),
        _fn("vh_launch_split2h_planes", p, p, p, i, i, f),
        _fn("vh_launch_linear_h2", p, p, p, f, p, p, i, i, i, i, p),
        _fn("vh_launch_attention_h2", p, p, p, i, i, i, i),
        _fn("vh_launch_attention", p, p, p, i, i, i, i),
        _fn("vh_launch_attention_rows", p, p, p, i, i, i, i, i, i, i),
        _fn("vh_launch_gather_rows", p, p, p, i, i, i, i, i),
        _fn("vh_launch_softmax", p, p, p, i, i),
        _fn("vh_launch_topk", p, p, i, i, i, i, p, p),
        _fn("vh_cls_attention_head_dim_ok", i),
        _fn("vh_launch_cls_attention", p, p, i, i, i, i, i, i, i, p, p),
        _fn("vh_rollout_workspace", i, i, ret=sz),
        _fn("vh_rollout_max_tokens", i),
        _fn("vh_launch_rollout_step", p, p, i, i, i, i, i, p, p, p),
        _fn("vh_launch_rollout_read", p, p, i, i, p),
        _fn("vh_launch_attention_f16", p, p, p, i, i, i, i),
        _fn("vh_launch_absmax", p, p, sz, p),
        _fn("vh_launch_quantize_mx_rows", p, p, p, p, i, i),
        _fn("vh_launch_quantize_mx_act", p, p, p, p, i, i),
        _fn("vh_mx_act_scale_bytes", i, i, ret=sz),
        _fn("vh_gemm_tile_class", i, i, i, i, i, i, i, ip),
        _fn("vh_gemm_rows_tile_class", i, i, i, i, i, i, i, i, ip),
        _fn("vh_launch_layer_norm_mx", p, p, p, p, p, p, i, i, l, d),
        _fn("vh_launch_linear_mx", p, p, p, p, p, p, p, p, i, i, i, i, p),
        _fn("vh_launch_attention_planes_f16_mx", p, p, p, p, i, i, i, i),
        _fn("vh_launch_linear_mx_planes_f16", p, p, p, p, p, p, p, i, i, i),
        _fn("vh_launch_fold_gamma", p, p, p, p, i, i),
        _fn("vh_launch_fold_bias", p, p, p, p, p, i, i),
        _fn("vh_launch_colsum_operand", p, p, p, p, i, i),
        _fn("vh_launch_patch_embed_planes_norm", p, p, p, p, p, p, p, i, i, i, i, i, p, sz, p, p, p),
        _fn("vh_launch_linear_planes_norm", p, p, i, p, p, p, p, p, d, i, i, i, i),
        _fn("vh_launch_linear_planes_resid_norm", p, p, p, p, p, p, i, i, i, p, p, p),
        _fn("vh_launch_colsum_planes3", p, p, p, i, i),
        _fn("vh_launch_patch_embed_planes3_norm", p, p, p, p, p, p, p, i, i, i, i, i, p, sz, p, p),
        _fn("vh_launch_linear_p3_norm", p, p, i, p, p, p, p, p, d, i, i, i, i),
        _fn("vh_launch_linear_p3_resid_norm", p, p, p, p, p, p, i, i, i, p, p),
        _fn("vh_launch_linear_mx_norm", p, p, p, i, p, p, p, p, p, p, p, d, i, i, i, i),
        _fn("vh_launch_linear_mx_resid_norm", p, p, p, p, p, p, p, p, i, i, i, p, p, p),
        _fn("vh_launch_patch_embed_planes_u8", p, p, i, fp, fp, p, p, p, p, p, i, i, i, i, i, p, sz, i, p, p, p),
        _fn("vh_launch_expand_u8", p, p, i, fp, fp, p, i, i, i),
        _fn("vh_launch_patch_embed_planes_hw", p, p, p, i, fp, fp, p, p, p, p, p, i, i, i, i, i, i, p, sz, i, p, p, p),
        _fn("vh_patch_embed_workspace_hw", i, i, i, i, i, i, ret=sz),
        _fn("vh_launch_patch_embed_rows_hw", p, p, p, p, p, p, p, i, i, i, i, i, i, p, sz, i),
        _fn("vh_launch_expand_u8_hw", p, p, i, fp, fp, p, i, i, i, i),
        _fn("vh_launch_resize_crop_u8", p, p, i, i, i, i, i, p, sz, p),     # desc: vh_resize_desc[n] in device memory
        _fn("vh_feature_readout_scratch", i, i, i, ret=sz),
        _fn("vh_launch_feature_readout", p, p, p, l, p, p, d, i, i, i, i, i, i, i, i, i, p, p, p, p, sz),
        _fn("vh_gallery_query_tile", i),
        _fn("vh_gallery_splits", i, l),
        _fn("vh_gallery_workspace", i, l, i, i, ret=sz),
        _fn("vh_launch_gallery_topk", p, p, i, i, p, i, l, l, i, i, p, p, p),
        _fn("vh_launch_dense_logits", p, p, l, l, i, i, i, p, l, p, i, p),
        _fn("vh_launch_dense_labels", p, p, i, i, i, i, i, i, p, p),
        _fn("vh_launch_dense_soft", p, p, i, i, i, i, i, i, f, p, p, p, p),
        _fn("vh_dense_stitch_scratch", i, i, i, l, ret=sz),
        _fn("vh_launch_dense_stitch", p, p, i, i, i, i, fp, i, i, ip, ip, i, p, sz, p, p, p),
        _fn("vh_dense_stitch_soft_variant", i),
        _fn("vh_launch_dense_stitch_soft", p, p, i, i, i, i, fp, i, i, ip, ip, p, sz, f, p, p, p, p),
        _fn("vh_launch_resample_pos_embed", p, p, p, i, i, i, i, i, i, i, i),
    ],
    "ViT_opencl.h": [
        _fn("vit_config_preset", P(VitConfig), s),
        _fn("vit_config_canonical", P(VitConfig), P(VitConfig), s),
        _fn("vit_config_grid", P(VitConfig), ip, ip, ret=None),
        _fn("vit_config_sizeof"),
        _fn("vit_config_tokens", P(VitConfig)),
        _fn("vit_config_num_tensors", P(VitConfig)),
        _fn("vit_config_tensor_size", P(VitConfig), i, ret=sz),
        _fn("ViT_opencl", P(ImageData), P(Network), fpp, ret=None),
        _fn("vit_hip_last_call_seconds", dp, dp, ret=None),
        _fn("vit_hip_create", pp, P(VitConfig), P(Network), i, i, i),
        _fn("vit_hip_destroy", p, ret=None),
        _fn("vit_hip_create_ex", pp, P(VitConfig), P(Network), i, i, i, i),
        _fn("vit_hip_precision", p),
        _fn("vit_hip_ln_fold", p),
        _fn("vit_hip_export_planes", p, s),
        _fn("vit_hip_create_from_planes", pp, s, i, i),
        _fn("vit_resample_check_hw", P(VitConfig), i, i, P(PosResampleC), P(VitConfig)),
        _fn("vit_resample_check", P(VitConfig), i, P(PosResampleC), P(VitConfig)),
        _fn("vit_hip_create_at_size", pp, p, i, i, i, P(PosResampleC)),
        _fn("vit_hip_create_at_resolution", pp, p, i, i, P(PosResampleC)),
        _fn("vit_hip_forward", p, P(ImageData), i, fp, fpp),
        _fn("vit_hip_forward_device", p, p, i, p, p, p),
        _fn("vit_pixel_norm_from_mean_std", P(PixelNorm), fp, fp, i),
        _fn("vit_hip_forward_device_u8", p, p, i, i, P(PixelNorm), p, p, p),
        _fn("vit_hip_forward_u8", p, u8p, i, i, P(PixelNorm), fp, fpp),
        _fn("vit_resize_crop_geometry", i, i, P(ResizeCrop), i, ip, ip, ip, ip),
        _fn("vit_hip_resize_crop_u8", p, P(ImageU8), i, i, P(ResizeCrop), p, p),
        _fn("vit_hip_forward_device_u8_resized", p, P(ImageU8), i, i, P(ResizeCrop), P(PixelNorm), p, p, p),
        _fn("vit_hip_forward_u8_resized", p, P(ImageU8), i, i, P(ResizeCrop), P(PixelNorm), fp, fpp),
        _fn("vit_box_check", i, i, fp),
        _fn("vit_box_rows", i, f, f, i, i, ip, ip),
        _fn("vit_tile_boxes", i, i, i, i, i, P(Box), i),
        _fn("vit_hip_crop_boxes_u8", p, P(ImageU8), i, P(Box), i, i, i, p, p),
        _fn("vit_hip_forward_device_u8_boxes", p, P(ImageU8), i, P(Box), i, i, i, P(PixelNorm), p, p, p),
        _fn("vit_hip_forward_u8_boxes", p, P(ImageU8), i, P(Box), i, i, i, P(PixelNorm), fp, fpp),
        _fn("vit_hip_create_multi", pp, P(VitConfig), P(Network), i, ip, i, i, i),
        _fn("vit_hip_forward_multi", p, P(ImageData), i, fp, fpp),
        _fn("vit_hip_destroy_multi", p, ret=None),
        _fn("vit_hip_multi_devices", p),
        _fn("vit_hip_multi_ctx", p, i, ret=p),
        _fn("vit_hip_device", p),
        _fn("vit_hip_forward_device_multi", p, pp, ip, p, p),
        _fn("vit_hip_multi_last_enqueue_ms", p, dp, i),
        _fn("vit_shard_range", i, i, i, ip, ip, ret=None),
        _fn("vit_shard_run", i, i, SHARD_FN, p),
        _fn("vit_shard_run_timed", i, i, SHARD_FN, p, dp),
        _fn("vit_hip_config", p, ret=P(VitConfig)),
        _fn("vit_hip_stream", p, ret=p),
        _fn("vit_hip_max_batch", p),
        _fn("vit_hip_weight", p, i, ret=p),
        _fn("vit_hip_set_last_layer_cls_only", p, i),
        _fn("vit_feature_sizes", P(VitConfig), P(FeatureSpecC), szp, szp, szp),
        _fn("vit_hip_set_features", p, P(FeatureSpecC), P(FeatureBuffers)),
        _fn("vit_hip_set_features_host", p, P(FeatureSpecC), P(FeatureBuffers)),
        _fn("vit_topk_check", P(VitConfig), P(TopKSpecC)),
        _fn("vit_hip_set_topk", p, P(TopKSpecC), P(TopKBuffers)),
        _fn("vit_hip_set_topk_host", p, P(TopKSpecC), P(TopKBuffers)),
        _fn("vit_attn_sizes", P(VitConfig), P(AttnSpecC), szp, szp),
        _fn("vit_hip_set_attention", p, P(AttnSpecC), P(AttnBuffers)),
        _fn("vit_hip_set_attention_host", p, P(AttnSpecC), P(AttnBuffers)),
        _fn("vit_rollout_sizes", P(VitConfig), P(RolloutSpecC), szp, szp),
        _fn("vit_hip_set_rollout", p, P(RolloutSpecC), P(RolloutBuffers)),
        _fn("vit_hip_set_rollout_host", p, P(RolloutSpecC), P(RolloutBuffers)),
        _fn("vit_gallery_check", P(VitConfig), P(GallerySpecC), szp),
        _fn("vit_hip_set_gallery", p, P(GallerySpecC), P(GalleryBuffers)),
        _fn("vit_hip_set_gallery_host", p, P(GallerySpecC), P(GalleryBuffers)),
        _fn("vit_dense_sizes", P(VitConfig), P(DenseSpecC), szp, szp, szp, szp),
        _fn("vit_hip_set_dense", p, P(DenseSpecC), P(DenseBuffers)),
        _fn("vit_hip_set_dense_host", p, P(DenseSpecC), P(DenseBuffers)),
        _fn("vit_dense_soft_check", P(VitConfig), P(DenseSpecC), P(DenseSoftSpecC), szp),
        _fn("vit_hip_set_dense_soft", p, P(DenseSpecC), P(DenseSoftSpecC), P(DenseBuffers), P(DenseSoftBuffers)),
        _fn("vit_frame_sizes", P(VitConfig), P(FrameSpecC), i, i, i, szp, szp),
        _fn("vit_stitch_check", i, i, fp, i, s),
        _fn("vit_stitch_index", i, i, i, fp, i, ip, ip, l, ret=l),
        _fn("vit_hip_segment_frame_device_u8", p, P(ImageU8), P(Box), i, i, i, P(PixelNorm), P(FrameSpecC), P(FrameBuffers)),
        _fn("vit_hip_segment_frame_u8", p, P(ImageU8), P(Box), i, i, i, P(PixelNorm), P(FrameSpecC), P(FrameBuffers)),
        _fn("vit_frame_soft_check", P(VitConfig), P(FrameSpecC), P(DenseSoftSpecC), i, i, i, szp),
        _fn("vit_hip_segment_frame_soft_device_u8", p, P(ImageU8), P(Box), i, i, i, P(PixelNorm), P(FrameSpecC), P(DenseSoftSpecC),
            P(FrameBuffers), P(DenseSoftBuffers)),
        _fn("vit_hip_segment_frame_soft_u8", p, P(ImageU8), P(Box), i, i, i, P(PixelNorm), P(FrameSpecC), P(DenseSoftSpecC), P(FrameBuffers),
            P(DenseSoftBuffers)),
        _fn("vit_hip_read_tokens", p, i, fp),
        _fn("vit_hip_last_layer_pending", p),
        _fn("vit_hip_profile_enable", p, i),
        _fn("vit_hip_profile_read", p, dp, lp),
        _fn("vit_hip_profile_select", p, u),
        _fn("vit_write_result_file", s, fpp, i, i),
        _fn("vit_write_result_file_topk", s, ip, fp, i, i),
        _fn("vit_compare_rows", fp, fp, i, i, d, P(CompareReport)),
        _fn("vit_synth_fill", fp, sz, ull, f, f, ret=None),
        _fn("vit_synth_tensor", P(VitConfig), i, ull, fp, ret=None),
        _fn("vit_synth_image", P(VitConfig), i, fp, ret=None),
    ],
    "Network.h": [
        _fn("load_image_data", s, ret=P(ImageData)),
        _fn("load_weights", s, P(Network), i, ret=None),
        _fn("vit_write_image_file", s, P(ImageData), i),
        _fn("vit_write_weight_file", s, i, s, fp, sz),
    ],
}

EXPORTS = [name for protos in PROTOTYPES.values() for name, _, _ in protos]


def declare(L):
    """Set argtypes and restype of every table entry on the loaded library L (any build of it); a table entry that L does
    not export is an error.  Returns L."""
    for protos in PROTOTYPES.values():
        for name, restype, argtypes in protos:
            try:
                fn = getattr(L, name)
            except AttributeError:
                raise AttributeError(f"the library does not export {name}, which host/abi.py declares") from None
            fn.argtypes, fn.restype = argtypes, restype
    return L
