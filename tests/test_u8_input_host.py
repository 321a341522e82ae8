"""CPU tests of the 8-bit input path's host side (include/ViT_opencl.h: vit_pixel_norm_from_mean_std, vit_hip_forward_u8,
vit_hip_forward_device_u8): the normalisation constants, and the argument checks that run before any device is touched.
The header / EXPORTS agreement of the new symbols is tests/test_host.py::test_headers_declare_exactly_the_exports."""
import ctypes as C

import numpy as np
import pytest

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
HALF = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))


@pytest.mark.parametrize("mean,std", [IMAGENET, HALF], ids=["imagenet", "half"])
def test_pixel_norm_is_the_float64_formula_rounded_once(pkg, mean, std):
    m32, s32 = np.float32(mean), np.float32(std)
    got = pkg.pixel_norm(m32, s32)
    m64, s64 = m32.astype(np.float64), s32.astype(np.float64)
    want_scale = (1.0 / (255.0 * s64)).astype(np.float32)
    want_bias = (-m64 / s64).astype(np.float32)
    assert np.array_equal(np.array(got.scale[:3], dtype=np.float32), want_scale)
    assert np.array_equal(np.array(got.bias[:3], dtype=np.float32), want_bias)
    # the unused fourth channel is left zero
    assert got.scale[3] == 0.0 and got.bias[3] == 0.0


def test_pixel_norm_refuses_bad_std_and_channel_counts(pkg):
    L, b = pkg.lib(), pkg.binding
    out = b.PixelNorm()
    ones = np.ones(5, dtype=np.float32)
    for std in ([0.2, 0.0, 0.2], [0.2, -0.1, 0.2], [0.2, float("nan"), 0.2]):
        s = np.array(std, dtype=np.float32)
        assert L.vit_pixel_norm_from_mean_std(C.byref(out), b.fptr(ones[:3]), b.fptr(s), 3) == 1
        assert b"std" in L.vh_last_error()
    for chans in (0, 5):
        assert L.vit_pixel_norm_from_mean_std(C.byref(out), b.fptr(ones), b.fptr(ones), chans) == 1
    assert L.vit_pixel_norm_from_mean_std(None, b.fptr(ones), b.fptr(ones), 3) == 1
    for chans in (1, 4):
        assert L.vit_pixel_norm_from_mean_std(C.byref(out), b.fptr(ones), b.fptr(ones), chans) == 0
    with pytest.raises(pkg.VitHipError):
        pkg.pixel_norm([0.5, 0.5], [0.5, 0.0])


def test_u8_forward_forms_refuse_null_context_and_norm_without_a_device(pkg):
    """Code 1 with a message, before any device call: this runs where there is no GPU at all.  The stand-in context is a
    zeroed host buffer; the NULL norm is refused before the context is looked at."""
    L, b = pkg.lib(), pkg.binding
    norm = pkg.pixel_norm(*IMAGENET)
    img = np.zeros((2, 224, 224, 3), dtype=np.uint8)
    host = img.ctypes.data_as(C.POINTER(C.c_ubyte))
    logits = np.empty((2, 1000), dtype=np.float32)
    stand_in = C.create_string_buffer(1 << 16)
    ctx = C.cast(stand_in, C.c_void_p)
    for c, nm in ((None, C.byref(norm)), (ctx, None), (None, None)):
        assert L.vit_hip_forward_u8(c, host, 2, 0, nm, b.fptr(logits), None) == 1
        assert b"vit_hip_forward_u8" in L.vh_last_error()
        assert L.vit_hip_forward_device_u8(c, img.ctypes.data, 2, 0, nm, None, None, None) == 1
        assert b"vit_hip_forward_device_u8" in L.vh_last_error()
    assert L.vit_hip_forward_u8(None, None, 2, 0, C.byref(norm), None, None) == 1
