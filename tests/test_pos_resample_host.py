"""Host side of position-embedding resampling (no GPU): the NumPy float64 reference (tests/pos_resample_ref.py) against
torch.nn.functional.interpolate on float64 tensors, its fixed points, and vit_resample_check's refusals -- through the loaded
library, and in a stand-alone program (tests/resample_check_main.c) under AddressSanitizer and UBSan."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import pos_resample_ref as pr

# (in_h, in_w) -> (out_h, out_w): up, down, to and from a single sample, equal, and rectangular both ways
GRIDS = [((1, 1), (3, 3)), ((2, 2), (3, 3)), ((3, 3), (2, 2)), ((14, 14), (24, 24)), ((2, 2), (2, 2)), ((4, 4), (1, 1)),
         ((8, 8), (24, 24)), ((3, 5), (4, 2)), ((7, 3), (1, 6))]
E = 5


def _grid(in_hw, seed):
    """values of size 3 with channel scales 1e3, 1 and 1e-3 mixed in"""
    rng = np.random.default_rng(seed)
    g = rng.uniform(-3.0, 3.0, size=(in_hw[0], in_hw[1], E))
    return g * np.array([1e3, 1.0, 1e-3, 1.0, 1.0])


@pytest.mark.parametrize("align_corners", [False, True])
@pytest.mark.parametrize("mode", ["bicubic", "bilinear"])
@pytest.mark.parametrize("in_hw,out_hw", GRIDS)
def test_reference_is_torch_interpolate_on_float64(in_hw, out_hw, mode, align_corners):
    """per channel within 1e-12 of that channel's largest source magnitude"""
    g = _grid(in_hw, 17 * in_hw[0] + out_hw[1])
    got = pr.resample_grid(g, out_hw, mode, align_corners)
    t = torch.from_numpy(np.ascontiguousarray(g.transpose(2, 0, 1)))[None]
    want = torch.nn.functional.interpolate(t, size=out_hw, mode=mode, align_corners=align_corners, antialias=False)[0]
    want = want.numpy().transpose(1, 2, 0)
    assert got.shape == want.shape == (out_hw[0], out_hw[1], E) and got.dtype == np.float64
    m = np.abs(g).reshape(-1, E).max(axis=0)
    assert (np.abs(got - want) <= 1e-12 * m).all(), float((np.abs(got - want) / m).max())


@pytest.mark.parametrize("align_corners", [False, True])
@pytest.mark.parametrize("mode", ["bicubic", "bilinear"])
def test_equal_grids_give_the_input_and_a_constant_stays_constant(mode, align_corners):
    g = _grid((6, 4), 3).astype(np.float32)
    assert np.array_equal(pr.resample_grid(g, (6, 4), mode, align_corners), g.astype(np.float64))
    pos = np.concatenate([np.full((2, E), 9.0, dtype=np.float32), g.reshape(24, E)])
    out = pr.resample_pos_embed(pos, 2, (6, 4), (6, 4), mode, align_corners)
    assert np.array_equal(out, pos.astype(np.float64))
    for in_hw, out_hw in GRIDS:
        c = np.full((in_hw[0], in_hw[1], 2), 0.7)
        assert np.abs(pr.resample_grid(c, out_hw, mode, align_corners) - 0.7).max() <= 1e-12
    up = pr.resample_pos_embed(pos, 2, (6, 4), (9, 7), mode, align_corners)
    assert up.shape == (2 + 63, E) and np.array_equal(up[:2], pos[:2].astype(np.float64))


def test_bound_is_the_headers(pkg):
    want = np.array([[-2.0, 0.0, 1.0]])
    b = pr.bound(want, np.array([[4.0, -8.0]]))
    assert np.array_equal(b, 2.0 ** -24 * np.abs(want) + 2.0 ** -40 * 8.0)


def test_resample_check_in_a_stand_alone_program_under_asan_and_ubsan(tmp_path):
    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "resample_check_main"
    build = subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-Wall", "-D_POSIX_C_SOURCE=200809L", "-fsanitize=address,undefined",
                            "-fno-omit-frame-pointer", f"-I{root / 'include'}",
                            str(root / "vit-with-opencl_amd" / "csrc" / "vit_config.c"),
                            str(root / "tests" / "resample_check_main.c"), "-o", str(exe), "-lm"], capture_output=True, text=True)
    assert build.returncode == 0 and "warning" not in build.stderr, build.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60,
                       env={"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})
    assert r.returncode == 0 and "ok (0 failures)" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr


def test_resample_check_accepts_and_refuses(pkg):
    b, L = pkg.binding, pkg.lib()
    cfg = pkg.preset("vit_b_16")
    out = b.resample_check(cfg, 384)
    assert out.img_size == 384 and b.tokens(out) == 577 and cfg.img_size == 224
    assert (out.patch_size, out.embed_dim, out.depth, out.num_heads, out.mlp_hidden, out.num_classes, out.in_chans, out.eps) == \
        (cfg.patch_size, cfg.embed_dim, cfg.depth, cfg.num_heads, cfg.mlp_hidden, cfg.num_classes, cfg.in_chans, cfg.eps)
    assert b.resample_check(cfg, 512, "bilinear", True).img_size == 512
    # how == NULL is bicubic, align_corners 0
    got = b.VitConfig()
    assert L.vit_resample_check(C.byref(cfg), 384, None, C.byref(got)) == 0 and got.img_size == 384

    fine = pkg.preset("vit_b_16")
    fine.patch_size, fine.img_size = 4, 32
    assert b.resample_check(fine, 2048).img_size == 2048          # 512 patches a side: the limit

    def rc(cfg_, img, mode=0, ac=0):
        how, o = b.PosResampleC(mode, ac), b.VitConfig()
        return L.vit_resample_check(C.byref(cfg_), img, C.byref(how), C.byref(o))

    how = b.PosResampleC(0, 0)
    for bad in (lambda: rc(cfg, 0), lambda: rc(cfg, -224), lambda: rc(cfg, 230), lambda: rc(fine, 2052),
                lambda: rc(cfg, 384, 2, 0), lambda: rc(cfg, 384, 0, 2), lambda: rc(cfg, 384, -1, 0),
                lambda: L.vit_resample_check(None, 384, C.byref(how), C.byref(got)),
                lambda: L.vit_resample_check(C.byref(cfg), 384, C.byref(how), None)):
        L.vh_set_error(1, b"")
        assert bad() == 1
        msg = L.vh_last_error().decode()
        assert msg.startswith("vit_resample_check: ") and len(msg) > len("vit_resample_check: ")
    with pytest.raises(b.VitHipError, match="vit_resample_check"):
        b.resample_check(cfg, 230)
    # a null source context is refused on the host, before any device call
    ctx = C.c_void_p(123)
    assert L.vit_hip_create_at_resolution(C.byref(ctx), None, 384, 0, None) == 1 and not ctx.value
    assert L.vh_last_error().decode().startswith("vit_hip_create_at_resolution: ")
