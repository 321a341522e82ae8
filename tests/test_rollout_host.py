"""Host side of attention rollout (no GPU): vit_rollout_sizes and its refusals, the ctypes mirrors of the header's structs,
and the reference itself -- rows of the float64 rollout sum to 1, and a plain fp32 emulation of the definition stays inside
the bound tests/test_gpu_rollout.py holds the kernels to, on every launcher case."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import rollout_ref as rr

ROOT = Path(__file__).resolve().parent.parent
PRESETS = ("vit_b_16", "vit_l_16", "vit_h_14", "vit_b_16_384", "vit_l_16_512", "vit_h_14_518")


def test_rollout_sizes_on_every_preset(pkg):
    b = pkg.binding
    for name in PRESETS:
        cfg = pkg.preset(name)
        T = (cfg.img_size // cfg.patch_size) ** 2 + 1
        assert T == pkg.binding.tokens(cfg)
        for first in (0, 3, -1, -cfg.depth, cfg.depth - 1):
            assert b.rollout_sizes(cfg, b.RolloutSpec(first)) == (T, 3 * T * T * 4), (name, first)
    # the two figures the header quotes per buffer
    assert b.rollout_sizes(pkg.preset("vit_b_16"), b.RolloutSpec())[1] // 3 * 512 == 79_480_832
    assert b.rollout_sizes(pkg.preset("vit_h_14_518"), b.RolloutSpec())[1] // 3 * 64 == 480_486_400
    # each output pointer may be NULL
    L, cfg, spec = pkg.lib(), pkg.preset("vit_b_16"), b.RolloutSpecC(0)
    only = C.c_size_t()
    assert L.vit_rollout_sizes(C.byref(cfg), C.byref(spec), None, None) == 0
    assert L.vit_rollout_sizes(C.byref(cfg), C.byref(spec), C.byref(only), None) == 0 and only.value == 197
    assert L.vit_rollout_sizes(C.byref(cfg), C.byref(spec), None, C.byref(only)) == 0 and only.value == 3 * 197 * 197 * 4


def test_spec_refusals(pkg):
    b, L = pkg.binding, pkg.lib()
    cfg = pkg.preset("vit_b_16")

    def rc(first, cfg_=cfg):
        spec = b.RolloutSpecC(first)
        return L.vit_rollout_sizes(C.byref(cfg_), C.byref(spec), None, None)

    assert rc(0) == 0 and rc(11) == 0 and rc(-12) == 0 and rc(-1) == 0
    no_depth, no_heads, odd_heads = pkg.preset("vit_b_16"), pkg.preset("vit_b_16"), pkg.preset("vit_b_16")
    no_depth.depth, no_heads.num_heads, odd_heads.num_heads = 0, 0, 7
    for bad in (lambda: rc(12), lambda: rc(-13), lambda: rc(1 << 30), lambda: rc(0, no_depth), lambda: rc(0, no_heads),
                lambda: rc(0, odd_heads), lambda: L.vit_rollout_sizes(None, C.byref(b.RolloutSpecC(0)), None, None),
                lambda: L.vit_rollout_sizes(C.byref(cfg), None, None, None)):
        L.vh_set_error(1, b"stale")
        assert bad() == 1
        msg = L.vh_last_error().decode()
        assert msg.startswith("vit_rollout_sizes: ") and len(msg) > len("vit_rollout_sizes: ")
    with pytest.raises(b.VitHipError, match="first_layer"):
        b.rollout_sizes(cfg, b.RolloutSpec(12))
    # arming without a context is refused on the host, before any device call
    assert L.vit_hip_set_rollout(None, None, None) == 1 and L.vit_hip_set_rollout_host(None, None, None) == 1
    assert "NULL context" in L.vh_last_error().decode()
    spec, bufs = b.RolloutSpecC(0), b.RolloutBuffers(None)
    assert L.vit_hip_set_rollout(None, C.byref(spec), C.byref(bufs)) == 1
    # what the launcher takes per head_dim: whole 64-key chunks, the score rows of 16 queries in 160 KiB of LDS
    assert L.vh_rollout_max_tokens(128) == 1856 and L.vh_rollout_max_tokens(80) >= 1370 and L.vh_rollout_max_tokens(64) == 2176
    assert L.vh_rollout_workspace(512, 197) == 512 * 197 * 197 * 4 and L.vh_rollout_workspace(0, 197) == 0


def test_ctypes_structs_match_the_header(pkg, tmp_path):
    b = pkg.binding
    probe = tmp_path / "rollout_layout.c"
    probe.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "ViT_opencl.h"
int main(void)
{
    printf("%zu %zu %zu %zu\n", sizeof(vit_rollout_spec), offsetof(vit_rollout_spec, first_layer),
           sizeof(vit_rollout_buffers), offsetof(vit_rollout_buffers, rollout));
    return 0;
}
''')
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), "-o", str(tmp_path / "rollout_layout"), str(probe)], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "rollout_layout")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(b.RolloutSpecC), b.RolloutSpecC.first_layer.offset, C.sizeof(b.RolloutBuffers), b.RolloutBuffers.rollout.offset]
    assert got == [4, 0, 8, 0]


@pytest.mark.parametrize("n,T,E,H", rr.CASES)
def test_fp32_emulation_stays_within_the_bound(n, T, E, H):
    """Every launcher case, amplitudes 1 and 3, on the fp32 values and on those rounded to fp16 (what the one-part planes
    hold): after each of the three steps the fp32 emulation's whole R lies within rollout_ref.bound of the float64
    reference, whose rows sum to 1 and whose entries are non-negative."""
    worst = 0.0
    for amp in rr.AMPLITUDES:
        layers = rr.case_layers(n, T, E, H, amp)
        for form in (rr.ROWS_F32, rr.PLANES_F16):
            values = [rr.stored_values(form, q) for q in layers]
            ref, emu, bnd = rr.rollout_steps(values, n, T, H), rr.rollout_steps_f32(values, n, T, H), rr.bound(values, n, T, H)
            for step, (r64, r32, b) in enumerate(zip(ref, emu, bnd)):
                assert r64.shape == (n, T, T) and (r64 >= 0).all()
                assert np.abs(r64.sum(axis=2) - 1.0).max() <= 1e-12
                rel = float((np.abs(r32.astype(np.float64) - r64) / (b * r64 + 1e-30)).max())
                worst = max(worst, rel)
                assert rel <= 1.0, (amp, form, step, rel)
            assert np.array_equal(rr.rollout(values, n, T, H), ref[-1][:, 0])
    print(f"(n={n}, T={T}, E={E}, H={H}): fp32 emulation worst |R - ref| / bound = {worst:.5f}")


def test_first_step_is_the_half_mix_of_the_class_row():
    """first_layer = -1 in closed form: 0.5 * attn_ref's head mean + 0.5 at key 0"""
    import attn_ref as ar
    n, T, E, H = 2, 50, 128, 2
    qkv = rr.case_layers(n, T, E, H, 1.0)[0]
    want = 0.5 * ar.cls_attention(qkv, n, T, H)[1]
    want[:, 0] += 0.5
    assert np.abs(rr.rollout([qkv], n, T, H) - want).max() <= 1e-15
