"""Host side of the dense head's soft maps (no GPU): vit_dense_soft_check's sizes and refusals through the library, the
NULL-context refusal of the setter, the new structs of host/abi.py against the header by tests/test_abi_host.py's mechanism,
requests_set_dense_soft over a counting allocator (tests/dense_soft_main.c, under ASan + UBSan), the kernel's limits in
csrc/kernel_limits.h, and the reference itself (tests/dense_soft_ref.py): the fp32 NumPy restatement of the kernel's
arithmetic stays inside the sharp bounds on the launcher's sharp cases, so the bounds are neither vacuous nor wrong before a
GPU sees them."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import dense_ref as dr
import dense_soft_ref as sr
import test_abi_host as abi_host

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "vit-with-opencl_amd" / "csrc"
FLAGS = ["-O1", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-ffp-contract=off", "-fsanitize=address,undefined",
         "-fno-omit-frame-pointer"]
ENV = {"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


# ---- the library ------------------------------------------------------------------------------------------------------

def spec_c(b, **kw):
    args = dict(n_labels=21, out_h=0, out_w=0, tap=-1, final_norm=True, weight_stride=768, d_weight=None, d_bias=None)
    args.update(kw)
    return b.DenseSpec(**args)


def test_dense_soft_check_sizes(pkg):
    b = pkg.binding
    cfg = pkg.preset("vit_b_16")
    assert b.dense_soft_check(cfg, spec_c(b)) == 224 * 224
    assert b.dense_soft_check(cfg, spec_c(b, out_h=37, out_w=50, n_labels=256), 0.37, 0x1000) == 37 * 50
    assert b.dense_soft_check(cfg, spec_c(b, out_h=4096, out_w=1, n_labels=2, tap=0), 3.0) == 4096
    assert b.dense_soft_check(pkg.preset("vit_b_16_384"), spec_c(b)) == 384 * 384
    L = pkg.lib()
    cs, soft = spec_c(b).c_struct(), b.DenseSoftSpecC(1.0, None)
    assert L.vit_dense_soft_check(C.byref(cfg), C.byref(cs), C.byref(soft), None) == 0


def test_dense_soft_check_refusals(pkg):
    b, L = pkg.binding, pkg.lib()
    cfg = pkg.preset("vit_b_16")
    fine = pkg.preset("vit_b_16")
    fine.patch_size = 2                       # a 112 x 112 grid: beyond VH_DENSE_MAX_GRID

    def rc(cfg_=cfg, scale=1.0, values=None, **kw):
        cs, soft = spec_c(b, **kw).c_struct(), b.DenseSoftSpecC(scale, values)
        return L.vit_dense_soft_check(C.byref(cfg_), C.byref(cs), C.byref(soft), None)

    assert rc() == 0
    cs, soft = spec_c(b).c_struct(), b.DenseSoftSpecC(1.0, None)
    bad = [(lambda: rc(tap=12), "tap"), (lambda: rc(n_labels=1), "n_labels"), (lambda: rc(n_labels=257), "n_labels"),
           (lambda: rc(out_w=4097), "out_h"), (lambda: rc(weight_stride=770), "weight_stride"), (lambda: rc(fine), "grid"),
           (lambda: rc(scale=0.0), "logit_scale"), (lambda: rc(scale=-2.0), "logit_scale"), (lambda: rc(scale=float("inf")), "logit_scale"),
           (lambda: rc(scale=float("nan")), "logit_scale"), (lambda: rc(values=0x1004), "aligned"),
           (lambda: L.vit_dense_soft_check(None, C.byref(cs), C.byref(soft), None), "NULL"),
           (lambda: L.vit_dense_soft_check(C.byref(cfg), None, C.byref(soft), None), "NULL"),
           (lambda: L.vit_dense_soft_check(C.byref(cfg), C.byref(cs), None, None), "NULL")]
    for i, (f, word) in enumerate(bad):
        L.vh_set_error(1, b"stale")
        assert f() == 1, i
        msg = L.vh_last_error().decode()
        assert msg.startswith("vit_dense_soft_check: ") and word in msg, (i, msg)
    with pytest.raises(b.VitHipError, match="logit_scale must be"):
        b.dense_soft_check(cfg, spec_c(b), -1.0)


def test_setter_refuses_a_null_context(pkg):
    b, L = pkg.binding, pkg.lib()
    L.vh_set_error(1, b"stale")
    assert L.vit_hip_set_dense_soft(None, None, None, None, None) == 1
    assert L.vh_last_error().decode() == "vit_hip_set_dense_soft: NULL context"
    cs, soft = spec_c(b).c_struct(), b.DenseSoftSpecC(1.0, None)
    assert L.vit_hip_set_dense_soft(None, C.byref(cs), C.byref(soft), None, C.byref(b.DenseSoftBuffers(0x1000, None, None))) == 1


def test_launcher_refuses_before_any_device_call(pkg):
    """every argument check of vh_launch_dense_soft stands in front of its first device call: the refusals need no device"""
    L = pkg.lib()
    A, B, V = 0x10000, 0x20000, 0x30000
    good = dict(pl=A, n=2, gh=3, gw=4, C=6, oh=9, ow=10, s=1.0, values=V, prob=B, expect=B + 0x1000, entropy=B + 0x2000)
    bad = [dict(C=1), dict(C=257), dict(gh=0), dict(gw=65), dict(oh=0), dict(ow=4097), dict(n=0), dict(n=2 ** 30, gh=4), dict(pl=None),
           dict(s=0.0), dict(s=-1.0), dict(s=float("inf")), dict(s=float("nan")), dict(values=None), dict(expect=None),
           dict(prob=None, expect=None, entropy=None, values=None), dict(pl=A + 4), dict(values=V + 8), dict(prob=B + 4),
           dict(expect=B + 0x1004), dict(entropy=B + 0x2008)]
    for kw in bad:
        a = dict(good)
        a.update(kw)
        L.vh_set_error(1, b"stale")
        rc = L.vh_launch_dense_soft(None, a["pl"], a["n"], a["gh"], a["gw"], a["C"], a["oh"], a["ow"], a["s"], a["values"], a["prob"], a["expect"],
                                    a["entropy"])
        msg = L.vh_last_error().decode()
        assert rc == 1 and msg.startswith("vh_launch_dense_soft: ") and len(msg) > 40, (kw, msg)


def test_struct_mirrors_against_the_header(pkg, tmp_path):
    """the two new structs by tests/test_abi_host.py's mechanism: field names from the header's text, sizeof and offsetof
    from a C probe compiled against it; the prototypes are in the table in the header's place"""
    abi = pkg.host.abi
    bodies = abi_host._struct_bodies("ViT_opencl.h")
    mine = {"vit_dense_soft_spec": abi.DenseSoftSpecC, "vit_dense_soft_buffers": abi.DenseSoftBuffers}
    lines = []
    for ctype, mirror in mine.items():
        assert abi.STRUCTS[ctype] is mirror
        assert [f for f, _ in mirror._fields_] == bodies[ctype], ctype
        lines.append(f'    printf("sizeof {ctype} %zu\\n", sizeof({ctype}));')
        lines += [f'    printf("offsetof {ctype}.{f} %zu\\n", offsetof({ctype}, {f}));' for f, _ in mirror._fields_]
    (tmp_path / "probe.c").write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ViT_opencl.h"\nint main(void)\n{\n' + "\n".join(lines) +
                                      "\n    return 0;\n}\n")
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), "-o", str(tmp_path / "probe"), str(tmp_path / "probe.c")], check=True)
    out = subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout
    probe = {line.rsplit(" ", 1)[0]: int(line.rsplit(" ", 1)[1]) for line in out.splitlines()}
    for ctype, mirror in mine.items():
        assert C.sizeof(mirror) == probe[f"sizeof {ctype}"]
        for f, _ in mirror._fields_:
            assert getattr(mirror, f).offset == probe[f"offsetof {ctype}.{f}"], f"{ctype}.{f}"
    assert C.sizeof(abi.DenseSoftSpecC) == 16 and abi.DenseSoftSpecC.d_values.offset == 8 and C.sizeof(abi.DenseSoftBuffers) == 24
    parsed = {fn: (ret, params) for fn, ret, params in abi_host.parse_prototypes("ViT_opencl.h") + abi_host.parse_prototypes("kernelHandler.h")}
    table = {fn: (ret, args) for protos in abi.PROTOTYPES.values() for fn, ret, args in protos}
    for fn in ("vh_launch_dense_soft", "vit_dense_soft_check", "vit_hip_set_dense_soft"):
        ret, params = parsed[fn]
        t_ret, t_args = table[fn]
        assert len(params) == len(t_args), fn
        assert not [w for w in [abi_host._matches(abi, ret, t_ret, fn)] + [abi_host._matches(abi, p, t, f"{fn} {k}") for k, (p, t) in
                                                                         enumerate(zip(params, t_args))] if w], fn
        assert hasattr(pkg.lib(), fn)
    assert table["vh_launch_dense_soft"][1][8] is C.c_float


# ---- requests_set_dense_soft over the counting allocator ----------------------------------------------------------------

def test_soft_arming_over_a_counting_allocator(tmp_path):
    exe = tmp_path / "dense_soft_main"
    build = subprocess.run(["gcc", *FLAGS, "-Wall", f"-I{ROOT / 'include'}", f"-I{CSRC}", str(CSRC / "vit_requests.c"), str(CSRC / "vit_ingest.c"),
                            str(CSRC / "vit_config.c"), str(ROOT / "tests" / "dense_soft_main.c"), "-o", str(exe), "-lm"],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    assert "warning" not in build.stderr, build.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    assert "dense_soft: ok" in r.stdout and int(r.stdout.split("(")[1].split()[0]) > 20, r.stdout


def test_limits_are_stated_once(tmp_path):
    """csrc/kernel_limits.h: the per-pixel kernels' LDS (the header quotes 76 KB at 37 x 256 and 129 KB at the limit), the
    largest output and the shape check both launchers refuse by"""
    src = tmp_path / "limits.c"
    src.write_text('#include <stdio.h>\n#include "kernel_limits.h"\nint main(void)\n{\n'
                   '    printf("%d %d %zu %zu %zu\\n", KL_DENSE_MAX_OUT, kl_dense_label_stride(150), kl_dense_labels_lds(14, 150),\n'
                   '           kl_dense_labels_lds(37, 256), kl_dense_labels_lds(VH_DENSE_MAX_GRID, VH_DENSE_MAX_LABELS));\n'
                   '    printf("%d %d %d %d %d %d %d\\n", kl_dense_pixel_shape_ok(1, 1, 1, 2, 1, 1), kl_dense_pixel_shape_ok(8, 64, 64, 256, 4096, 4096),\n'
                   '           kl_dense_pixel_shape_ok(1, 65, 1, 2, 1, 1), kl_dense_pixel_shape_ok(1, 1, 1, 257, 1, 1), kl_dense_pixel_shape_ok(1, 1, 1, 2, 4097, 1),\n'
                   '           kl_dense_pixel_shape_ok(0, 1, 1, 2, 1, 1), kl_dense_pixel_shape_ok(1 << 30, 4, 1, 2, 1, 1));\n    return 0;\n}\n')
    for compiler in (["gcc", "-std=c11"], ["g++", "-x", "c++", "-std=c++17"]):
        exe = tmp_path / "limits"
        build = subprocess.run([*compiler, "-Wall", "-Wextra", "-Wpedantic", f"-I{ROOT / 'include'}", f"-I{CSRC}", str(src), "-o", str(exe)],
                               capture_output=True, text=True)
        assert build.returncode == 0 and "warning" not in build.stderr, build.stderr
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
        assert out[0].split() == ["4096", "151", str(2 * 14 * 151 * 4), str(2 * 37 * 257 * 4), str(2 * 64 * 257 * 4)]
        assert out[1].split() == ["1", "1", "0", "0", "0", "0", "0"]
    assert 2 * 64 * 257 * 4 <= 160 * 1024


# ---- the reference ----------------------------------------------------------------------------------------------------

def test_definition_on_known_values():
    v = np.array([[0.0, 0.0, 0.0, 0.0], [np.log(3.0), 0.0, -np.inf, -np.inf], [1.0, np.nan, 0.0, 0.0], [np.inf, 0.0, 0.0, 0.0],
                  [-np.inf, -np.inf, -np.inf, -np.inf], [5.0, -np.inf, -np.inf, -np.inf]])
    p, x, h, av = sr.soft64(v, 1.0, np.array([1.0, -2.0, 4.0, 8.0]))
    assert np.allclose(p[[0, 1, 5]], [0.25, 0.75, 1.0]) and np.allclose(x[[0, 1, 5]], [2.75, 0.25, 1.0]) and np.allclose(av[[0, 1]], [3.75, 1.25])
    assert np.allclose(h[[0, 1, 5]], [np.log(4.0), -(0.75 * np.log(0.75) + 0.25 * np.log(0.25)), 0.0])
    assert np.isnan(p[2:5]).all() and np.isnan(x[2:5]).all() and np.isnan(h[2:5]).all()
    # the scale is an inverse temperature
    p2, _, h2, _ = sr.soft64(np.array([[2.0, 0.0]]), 0.5)
    assert np.allclose(p2, 1 / (1 + np.exp(-1.0))) and h2[0] > sr.soft64(np.array([[2.0, 0.0]]), 1.0)[2][0]
    got = sr.soft32(v.astype(np.float32), 1.0, np.array([1.0, -2.0, 4.0, 8.0], np.float32))
    for g in got:
        assert (g[2:5].view(np.uint32) == sr.NAN_BITS).all() and np.isfinite(g[[0, 1, 5]]).all()
    assert got[0][0] == np.float32(0.25) and got[2][5] == 0.0


def test_exact_v_is_the_label_kernels_score():
    """v32 restates dense_ref.dense32's expressions: its maximum over the classes is dense32's score, bit for bit, on the
    dyadic cases; with out == grid it is the logits' own bits for any floats"""
    for grid, out in sr.DYADIC:
        L = sr.integer_logits(2, grid, 21, 3)
        v = sr.v32(L, grid, out)
        lab, bits = dr.dense32(L, grid, out)
        assert np.array_equal(v.max(axis=-1).view(np.uint32), bits) and np.array_equal(v.argmax(axis=-1), lab)
        assert np.array_equal(v.astype(np.float64), dr.upsample64(L.astype(np.float64), grid, out))      # every operation exact
    for grid in sr.SHARP_GRIDS:
        L = sr.spread_logits(2, grid, 5, 8.0, 1)
        assert np.array_equal(sr.v32(L, grid, grid).view(np.uint32), L.reshape(2, grid[0], grid[1], 5).view(np.uint32))


@pytest.mark.parametrize("C_", sr.SHARP_C)
def test_fp32_restatement_stays_inside_the_sharp_bounds(C_):
    """the launcher's sharp cases through the NumPy restatement of the kernel's arithmetic: every pixel within the header's
    bounds -- and not by orders of magnitude, or the bounds would test nothing"""
    worst = dict.fromkeys(sr.NAMES, 0.0)
    values = sr.values_for(C_)
    for grid in sr.SHARP_GRIDS:
        for spread in sr.SPREADS:
            v = sr.v32(sr.spread_logits(2, grid, C_, spread, int(10 * spread) + C_), grid, grid)
            for s in sr.SCALES:
                got = dict(zip(sr.NAMES, sr.soft32(v, s, values)))
                w = sr.check_sharp(v, s, values, got, f"C={C_} grid={grid} spread={spread} s={s}")
                worst = {k: max(worst[k], w[k]) for k in worst}
                if spread == 0.0:
                    assert np.all(got["prob"] == np.float32(1.0) / np.float32(C_))
                    assert np.abs(got["entropy"].astype(np.float64) - np.log(C_)).max() <= 4 * sr.U * np.log(C_)
    for grid, out in sr.DYADIC:
        v = sr.v32(sr.integer_logits(2, grid, C_, C_), grid, out)
        w = sr.check_sharp(v, 0.37, values, dict(zip(sr.NAMES, sr.soft32(v, 0.37, values))), f"C={C_} {grid}->{out}")
        worst = {k: max(worst[k], w[k]) for k in worst}
    print(f"restatement C={C_}: worst |error| / bound " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert all(1e-4 < w <= 1.0 for w in worst.values()), worst      # one rounding of the result alone is 0.5 / (C + K) >= 1.7e-3


def test_checks_reject_what_is_wrong():
    grid, C_, s = (3, 5), 21, 1.0
    values = sr.values_for(C_)
    v = sr.v32(sr.spread_logits(1, grid, C_, 8.0, 2), grid, grid)
    p, x, h = sr.soft32(v, s, values)
    sr.check_sharp(v, s, values, dict(prob=p, expect=x, entropy=h))
    for name, arr in (("prob", p), ("expect", x), ("entropy", h)):
        off = arr.copy()
        off[0, 1, 2] *= np.float32(1 + 2e-4)
        with pytest.raises(AssertionError, match=name):
            sr.check_sharp(v, s, values, {name: off})
    nan = p.copy()
    nan[0, 0, 0] = np.nan
    with pytest.raises(AssertionError, match="not a number"):
        sr.check_sharp(v, s, values, dict(prob=nan))


def test_combined_bounds_hold_for_the_restatement_on_an_edge_case():
    """a non-dyadic ratio: v32's expressions are then rounded, v is known to within the interpolation bound only, and the
    restatement on those v stays inside the combined bounds of the float64 definition"""
    grid, out, C_ = (3, 3), (37, 37), 17
    L = sr.spread_logits(2, grid, C_, 8.0, 4)
    values = sr.values_for(C_)
    v = sr.v32(L, grid, out)
    assert np.abs(v.astype(np.float64) - dr.upsample64(L.astype(np.float64), grid, out)).max(axis=-1).max() <= sr.interp_bound(L, grid, out).max()
    w = sr.check_combined(L, grid, out, 3.0, values, dict(zip(sr.NAMES, sr.soft32(v, 3.0, values))))
    assert all(0 < q <= 1 for q in w.values()), w
