"""CPU tests of the higher-resolution presets (T > 512) and of the shapes refused at context creation because no attention
kernel runs them.  No device: ctx_new decides the plan before vh_init."""
import ctypes as C

import numpy as np
import pytest

LONG_PRESETS = {   # name: (base preset, img_size, tokens)
    "vit_b_16_384": ("vit_b_16", 384, 577),
    "vit_l_16_512": ("vit_l_16", 512, 1025),
    "vit_h_14_518": ("vit_h_14", 518, 1370),
}


@pytest.mark.parametrize("name", sorted(LONG_PRESETS))
def test_long_sequence_presets(pkg, name):
    base_name, img, T = LONG_PRESETS[name]
    L, cfg, base = pkg.lib(), pkg.preset(name), pkg.preset(base_name)
    assert cfg.img_size == img and pkg.binding.tokens(cfg) == T
    for f in ("patch_size", "in_chans", "num_classes", "embed_dim", "depth", "num_heads", "mlp_hidden", "eps"):
        assert getattr(cfg, f) == getattr(base, f), f
    assert L.vit_config_num_tensors(C.byref(cfg)) == L.vit_config_num_tensors(C.byref(base))
    assert L.vit_config_tensor_size(C.byref(cfg), 3) == T * cfg.embed_dim          # pos_embedding [T][E]
    for idx in (0, 1, 2, 4, 6, 14):
        assert L.vit_config_tensor_size(C.byref(cfg), idx) == L.vit_config_tensor_size(C.byref(base), idx)


def test_long_sequence_preset_in_the_oracle(pkg):
    from oracle.oracle import Oracle
    orc = Oracle("vit_b_16_384")
    assert orc.cfg.img_size == 384 and orc.lib.vit_config_tokens(C.byref(orc.cfg)) == 577
    assert orc.lib.vit_config_tensor_size(C.byref(orc.cfg), 3) == 577 * 768


def _create(pkg, cfg, precision):
    """vit_hip_create_ex on every tensor at its expected size (one shared host buffer: creation is refused before any is
    read, or fails at vh_init without a device)."""
    L = pkg.lib()
    n = L.vit_config_num_tensors(C.byref(cfg))
    sizes = [L.vit_config_tensor_size(C.byref(cfg), i) for i in range(n)]
    buf = np.zeros(max(sizes), dtype=np.float32)
    nets = (pkg.binding.Network * n)()
    for i, s in enumerate(sizes):
        nets[i].data = buf.ctypes.data_as(C.POINTER(C.c_float))
        nets[i].size = s
    ctx = C.c_void_p()
    rc = L.vit_hip_create_ex(C.byref(ctx), C.byref(cfg), nets, n, 0, 2, pkg.ViTHip.PRECISIONS[precision])
    if rc == 0:
        L.vit_hip_destroy(ctx)
    return rc, L.vh_last_error().decode()


def _tiny(pkg, img, heads):
    cfg = pkg.preset("vit_b_16")
    cfg.img_size, cfg.num_classes, cfg.embed_dim, cfg.depth, cfg.num_heads, cfg.mlp_hidden = img, 10, 256, 1, heads, 512
    return cfg


@pytest.mark.parametrize("case", ["f32_fp16x2", "p3_off", "native", "head_dim_128"])
def test_long_sequence_shapes_no_kernel_runs_are_refused_at_creation(pkg, monkeypatch, case):
    """T = 577 (img 384, patch 16): attention above 512 tokens runs on the planes paths with head_dim 64 or 80 only.  The
    rest is refused with code 2 and a message that names the limit -- before any device call."""
    for var in ("VIT_HIP_P3", "VIT_HIP_GEMM_FP32", "VIT_HIP_ATTN", "VIT_HIP_LN_FOLD"):
        monkeypatch.delenv(var, raising=False)
    precision, heads = "f32", 4
    if case == "f32_fp16x2":
        precision = "f32_fp16x2"
    elif case == "p3_off":
        monkeypatch.setenv("VIT_HIP_P3", "0")
    elif case == "native":
        monkeypatch.setenv("VIT_HIP_GEMM_FP32", "native")
    else:
        heads = 2
    rc, msg = _create(pkg, _tiny(pkg, 384, heads), precision)
    assert rc == 2, (rc, msg)
    assert "577 tokens" in msg and "512" in msg and "head_dim 64 or 80" in msg


@pytest.mark.parametrize("precision", ["f32", "bf16", "fp8"])
def test_long_sequence_shapes_that_run_get_past_the_plan(pkg, monkeypatch, precision):
    """The same T = 577 shape on the planes paths with head_dim 64 is not refused by the plan: creation goes on to the
    device (0 with one, vh_init's failure code without)."""
    for var in ("VIT_HIP_P3", "VIT_HIP_GEMM_FP32", "VIT_HIP_ATTN", "VIT_HIP_LN_FOLD"):
        monkeypatch.delenv(var, raising=False)
    rc, msg = _create(pkg, _tiny(pkg, 384, 4), precision)
    assert rc != 2, msg
    # the same refusals do not reach T <= 512: head_dim 128 at T = 485 still goes to the streaming kernel
    rc, msg = _create(pkg, _tiny(pkg, 352, 2), precision)
    assert rc != 2, msg
