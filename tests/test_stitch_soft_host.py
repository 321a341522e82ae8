"""Host side of the soft stitch (no GPU): vit_frame_soft_check's sizes and refusals through the library, the launcher's
refusals -- every one in front of its first device call -- the new prototypes of host/abi.py against the headers by
tests/test_abi_host.py's mechanism, the variant limits of csrc/kernel_limits.h, and the reference itself
(tests/stitch_soft_ref.py): the fp32 NumPy restatement of the soft maps on the restated blend stays inside the sharp bounds on
the integer layouts and inside the combined bounds of the all-float64 definition on the float cases, so the bounds are
neither wrong nor vacuous before a GPU sees them."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import dense_ref as dr
import dense_soft_ref as ds
import stitch_ref as sr
import stitch_soft_ref as ss
import test_abi_host as abi_host

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "vit-with-opencl_amd" / "csrc"
IP = C.POINTER(C.c_int)


# ---- the library ------------------------------------------------------------------------------------------------------

def spec_c(b, **kw):
    args = dict(n_labels=21, out_h=0, out_w=0, tap=-1, final_norm=True, weight_stride=768, d_weight=None, d_bias=None)
    args.update(kw)
    return b.DenseSpec(**args)


def test_frame_soft_check_sizes(pkg):
    b = pkg.binding
    cfg = pkg.preset("vit_b_16")
    assert b.frame_soft_check(cfg, spec_c(b), 3000, 4000, 475) == 3000 * 4000
    assert b.frame_soft_check(cfg, spec_c(b, n_labels=256), 1, 16384, 1, 0.37, 0x1000) == 16384
    assert b.frame_soft_check(pkg.preset("vit_b_16_384"), spec_c(b, n_labels=2, tap=0), 224, 300, 4, 3.0, fill_label=0) == 224 * 300
    L = pkg.lib()
    fs, soft = b.FrameSpecC(spec_c(b).c_struct(), 255), b.DenseSoftSpecC(1.0, None)
    assert L.vit_frame_soft_check(C.byref(cfg), C.byref(fs), C.byref(soft), 45, 70, 3, None) == 0


def test_frame_soft_check_refusals(pkg):
    b, L = pkg.binding, pkg.lib()
    cfg = pkg.preset("vit_b_16")
    wide = pkg.preset("vit_b_16")
    wide.img_width = 320

    def rc(cfg_=cfg, scale=1.0, values=None, H=260, W=300, n=4, fill=255, **kw):
        fs, soft = b.FrameSpecC(spec_c(b, **kw).c_struct(), fill), b.DenseSoftSpecC(scale, values)
        return L.vit_frame_soft_check(C.byref(cfg_), C.byref(fs), C.byref(soft), H, W, n, None)

    assert rc() == 0 and rc(values=0x1000) == 0
    fs, soft = b.FrameSpecC(spec_c(b).c_struct(), 255), b.DenseSoftSpecC(1.0, None)
    bad = [(lambda: rc(tap=12), "tap"), (lambda: rc(n_labels=1), "n_labels"), (lambda: rc(n_labels=257), "n_labels"),
           (lambda: rc(out_h=224), "out_h"), (lambda: rc(out_w=1), "out_h"), (lambda: rc(fill=256), "fill_label"), (lambda: rc(fill=-1), "fill_label"),
           (lambda: rc(H=0), "frame"), (lambda: rc(W=16385), "frame"), (lambda: rc(n=0), "n_windows"), (lambda: rc(n=2 ** 31 // 196), "n_windows"),
           (lambda: rc(wide), "non-square"),
           (lambda: rc(scale=0.0), "logit_scale"), (lambda: rc(scale=-2.0), "logit_scale"), (lambda: rc(scale=float("inf")), "logit_scale"),
           (lambda: rc(scale=float("nan")), "logit_scale"), (lambda: rc(values=0x1004), "aligned"),
           (lambda: L.vit_frame_soft_check(None, C.byref(fs), C.byref(soft), 45, 70, 3, None), "NULL"),
           (lambda: L.vit_frame_soft_check(C.byref(cfg), None, C.byref(soft), 45, 70, 3, None), "NULL"),
           (lambda: L.vit_frame_soft_check(C.byref(cfg), C.byref(fs), None, 45, 70, 3, None), "NULL")]
    for i, (f, word) in enumerate(bad):
        L.vh_set_error(1, b"stale")
        assert f() == 1, i
        msg = L.vh_last_error().decode()
        assert (msg.startswith("vit_frame_soft_check: ") or msg.startswith("vit_dense_sizes: ")) and word in msg, (i, msg)
    with pytest.raises(b.VitHipError, match="logit_scale must be"):
        b.frame_soft_check(cfg, spec_c(b), 45, 70, 3, -1.0)


def test_frame_calls_refuse_a_null_context(pkg):
    L = pkg.lib()
    for entry in ("vit_hip_segment_frame_soft_device_u8", "vit_hip_segment_frame_soft_u8"):
        L.vh_set_error(1, b"stale")
        assert getattr(L, entry)(None, None, None, 1, 0, 0, None, None, None, None, None) == 1
        assert L.vh_last_error().decode() == f"{entry}: NULL argument"


def test_launcher_refuses_before_any_device_call(pkg):
    """every argument check of vh_launch_dense_stitch_soft -- the soft maps' and the stitch's, the index id by id -- stands
    in front of its first device call: the refusals need no device, and the stand-in pointers are never followed"""
    L, b = pkg.lib(), pkg.binding
    H, W, grid, Cc = 45, 70, (4, 4), 6
    boxes = sr.boxes4(sr.tiles(H, W, 32, 16))
    n = len(boxes)
    offsets, ids = b.stitch_index(H, W, boxes)
    need = L.vh_dense_stitch_scratch(n, H, W, len(ids))
    A, S, V, B = 0x10000, 0x20000, 0x30000, 0x40000
    good = dict(pl=A, n=n, gh=4, gw=4, C=Cc, boxes=boxes, H=H, W=W, offsets=offsets, ids=ids, scr=S, bytes=need, s=1.0, values=V, prob=B,
                expect=B + 0x10000, entropy=B + 0x20000)

    def launch(**kw):
        a = dict(good)
        a.update(kw)
        bx = None if a["boxes"] is None else b.fptr(np.ascontiguousarray(a["boxes"], np.float32))
        of = None if a["offsets"] is None else np.ascontiguousarray(a["offsets"], np.int32)
        keep = None if a["ids"] is None else np.ascontiguousarray(a["ids"], np.int32)
        return L.vh_launch_dense_stitch_soft(None, a["pl"], a["n"], a["gh"], a["gw"], a["C"], bx, a["H"], a["W"],
                                             None if of is None else of.ctypes.data_as(IP), None if keep is None else keep.ctypes.data_as(IP),
                                             a["scr"], a["bytes"], a["s"], a["values"], a["prob"], a["expect"], a["entropy"])

    def box(i, **kw):
        out = boxes.copy()
        for k, v in kw.items():
            out[i, "ltrb".index(k)] = v
        return out

    def changed(arr, j, v):
        out = np.array(arr).copy()
        out[j] = v
        return out

    assert offsets[2] - offsets[1] >= 2
    bad = [dict(s=0.0), dict(s=-1.0), dict(s=float("inf")), dict(s=float("nan")), dict(values=None), dict(expect=None),
           dict(prob=None, expect=None, entropy=None, values=None),
           dict(C=1), dict(C=257), dict(gh=0), dict(gw=65), dict(H=0), dict(W=16385), dict(n=0), dict(n=2 ** 31 // 16),
           dict(boxes=box(1, l=-1.0)), dict(boxes=box(2, r=70.5)), dict(boxes=box(1, r=16.5)), dict(boxes=box(2, l=np.nan)), dict(W=60),
           dict(offsets=changed(offsets, 0, 1)), dict(offsets=changed(offsets, 3, int(offsets[4]) + 1)), dict(ids=changed(ids, 0, -1)),
           dict(ids=changed(ids, 1, n)), dict(ids=changed(ids, int(offsets[1]) + 1, int(ids[int(offsets[1])]))),
           dict(bytes=need - 16), dict(bytes=0), dict(pl=None), dict(boxes=None), dict(offsets=None), dict(ids=None), dict(scr=None),
           dict(pl=A + 4), dict(scr=S + 8), dict(values=V + 8), dict(prob=B + 4), dict(expect=B + 0x10004), dict(entropy=B + 0x20008)]
    for kw in bad:
        L.vh_set_error(1, b"stale")
        assert launch(**kw) == 1, list(kw)
        msg = L.vh_last_error().decode()
        assert msg.startswith("vh_launch_dense_stitch_soft: ") and len(msg) > 40, (list(kw), msg)
    # the internal entry that takes the variant as an argument (csrc/vit_kernels.h; not in the public headers, so not in the ABI
    # table): a variant that does not take n_labels is refused, not replaced, and so is an unknown one -- as early as the rest
    fn = L.vh_launch_dense_stitch_soft_as
    fn.restype, fn.argtypes = C.c_int, [C.c_int] + list(L.vh_launch_dense_stitch_soft.argtypes)
    entry, L.vh_launch_dense_stitch_soft = L.vh_launch_dense_stitch_soft, None
    try:
        for variant, kw, word in ((2, dict(C=161), "variant 2"), (3, {}, "variant 3"), (-1, {}, "variant -1"), (1, dict(s=0.0), "logit_scale"),
                                  (2, dict(ids=changed(ids, 1, n)), "ids")):
            L.vh_launch_dense_stitch_soft = lambda *a, v=variant: fn(v, *a)
            L.vh_set_error(1, b"stale")
            assert launch(**kw) == 1, (variant, list(kw))
            msg = L.vh_last_error().decode()
            assert msg.startswith("vh_launch_dense_stitch_soft: ") and word in msg, msg
    finally:
        L.vh_launch_dense_stitch_soft = entry
    assert "vh_launch_dense_stitch_soft_as" not in pkg.binding.EXPORTS


def test_prototypes_against_the_headers(pkg):
    """the new prototypes are in host/abi.py's table with the headers' parameters, and the library exports them"""
    abi = pkg.host.abi
    parsed = {fn: (ret, params) for fn, ret, params in abi_host.parse_prototypes("ViT_opencl.h") + abi_host.parse_prototypes("kernelHandler.h")}
    table = {fn: (ret, args) for protos in abi.PROTOTYPES.values() for fn, ret, args in protos}
    for fn in ("vh_launch_dense_stitch_soft", "vh_dense_stitch_soft_variant", "vit_frame_soft_check",
               "vit_hip_segment_frame_soft_device_u8", "vit_hip_segment_frame_soft_u8"):
        ret, params = parsed[fn]
        t_ret, t_args = table[fn]
        assert len(params) == len(t_args), fn
        assert not [w for w in [abi_host._matches(abi, ret, t_ret, fn)] + [abi_host._matches(abi, p, t, f"{fn} {k}") for k, (p, t) in
                                                                         enumerate(zip(params, t_args))] if w], fn
        assert hasattr(pkg.lib(), fn) and fn in pkg.binding.EXPORTS
    assert table["vh_launch_dense_stitch_soft"][1][13] is C.c_float
    assert len(table["vit_hip_segment_frame_soft_u8"][1]) == 11


def test_variant_limits_are_stated_once(pkg, tmp_path):
    """csrc/kernel_limits.h: which variant a launch takes by n_labels, what each takes, and the register variant's instance --
    the smallest of 2, 4, 7 and 10 chunks that holds n_labels; the library's entry forwards to it"""
    src = tmp_path / "limits.c"
    src.write_text('#include <stdio.h>\n#include "kernel_limits.h"\nint main(void)\n{\n'
                   '    for (int c = 2; c <= VH_DENSE_MAX_LABELS; ++c)\n'
                   '        printf("%d %d %d %d %d %d\\n", c, kl_dense_stitch_soft_variant(c), kl_dense_stitch_soft_variant_ok(1, c),\n'
                   '               kl_dense_stitch_soft_variant_ok(2, c), kl_dense_stitch_soft_variant_ok(3, c), kl_dense_stitch_soft_reg_chunks(c));\n'
                   '    return 0;\n}\n')
    outs = []
    for compiler in (["gcc", "-std=c11"], ["g++", "-x", "c++", "-std=c++17"]):
        exe = tmp_path / "limits"
        build = subprocess.run([*compiler, "-Wall", "-Wextra", "-Wpedantic", f"-I{ROOT / 'include'}", f"-I{CSRC}", str(src), "-o", str(exe)],
                               capture_output=True, text=True)
        assert build.returncode == 0 and "warning" not in build.stderr, build.stderr
        outs.append(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)
    assert outs[0] == outs[1]
    L = pkg.lib()
    for line in outs[0].splitlines():
        c, v, ok1, ok2, ok3, chunks = map(int, line.split())
        assert v == L.vh_dense_stitch_soft_variant(c) and (ok1, ok2, ok3) == (1, int(c <= 160), 0)
        assert (ok1, ok2, ok3)[v - 1] == 1                           # what a launch takes by itself, it takes
        assert chunks == (min(n for n in (2, 4, 7, 10) if 16 * n >= c) if c <= 160 else 0)


# ---- the reference ----------------------------------------------------------------------------------------------------

def test_means32_is_the_stitch_references_blend():
    """means32 restates stitch32's blend: its best class and that class's bits are stitch32's labels and scores, its count
    stitch32's cover; and on the dyadic layouts every operation is exact, so it equals the float64 blend"""
    for name, (H, W, grid, boxes, fill) in ss.LAYOUTS.items():
        n = len(boxes)
        L = ss.integer_logits(n, grid, 17, 5 + n, special=False)
        m, cnt = ss.means32(L, grid, boxes, H, W)
        lab, sbits, cov = sr.stitch32(L, grid, boxes, H, W, fill)
        on = cnt > 0
        assert np.array_equal(np.minimum(cnt, 255).astype(np.uint8), cov)
        assert np.array_equal(m.argmax(axis=-1)[on], lab[on]) and np.array_equal(ss.bits(m.max(axis=-1))[on], sbits[on])
        if name != "stack-40":                                       # sums of up to 6 multiples of 2^-6 below 2^6 are exact; the mean of 3 or 6 is not
            m64, _ = sr.stitch64(L, grid, boxes, H, W)
            pow2 = np.isin(cnt, (1, 2, 4))
            assert np.array_equal(m[pow2].astype(np.float64), m64[pow2])


@pytest.mark.parametrize("Cc", ss.OVERLAP_C)
@pytest.mark.parametrize("name", list(ss.LAYOUTS))
def test_fp32_restatement_stays_inside_the_sharp_bounds(name, Cc):
    """soft32 on means32 against soft64 on means32: inside the sharp bounds on every defined pixel, the marker elsewhere, and
    not inside by orders of magnitude"""
    H, W, grid, boxes, _ = ss.LAYOUTS[name]
    n = len(boxes)
    values = ds.values_for(Cc)
    worst = dict.fromkeys(ss.NAMES, 0.0)
    for L in (ss.integer_logits(n, grid, Cc, 31 * n + Cc, special=False), ss.mild_logits(n, grid, Cc, n + Cc), ss.integer_logits(n, grid, Cc, 31 * n + Cc)):
        m, cnt = ss.means32(L, grid, boxes, H, W)
        for s in ss.SCALES:
            got = dict(zip(ss.NAMES, ds.soft32(m, s, values)))
            for g in got.values():                                   # soft32 knows nothing of coverage: the kernel's count does
                g[cnt == 0] = np.array([ss.NAN_BITS], np.uint32).view(np.float32)[0]
            w = ss.check_sharp(L, grid, boxes, H, W, s, values, got, f"{name} C={Cc} s={s}")
            worst = {k: max(worst[k], w[k]) for k in worst}
    print(f"restatement {name} C={Cc}: worst |error| / bound " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert all(1e-4 < w <= 1.0 for w in worst.values()), worst


@pytest.mark.parametrize("case", sr.FLOAT_CASES, ids=lambda c: f"{c[0]}x{c[1]}-t{c[2]}-C{c[5]}")
def test_fp32_restatement_stays_inside_the_combined_bounds(case):
    """fractional boxes and Gaussian logits: the restated blend is then rounded, the means are known to within the stitch's
    bound only, and the restatement stays inside the combined bounds of the all-float64 definition"""
    H, W, tile, stride, grid, Cc, seed = case
    boxes = sr.float_boxes(case)
    x, Wt, b = sr.float_case(len(boxes), grid, Cc, seed)
    L = dr.logits64(x, Wt, b).astype(np.float32)
    values = ds.values_for(Cc)
    m, cnt = ss.means32(L, grid, boxes, H, W)
    m64, _ = sr.stitch64(L, grid, boxes, H, W)
    assert (np.abs(m.astype(np.float64) - m64)[cnt > 0] <= sr.bound(L, grid, boxes, H, W)[cnt > 0]).all()
    for s in (1.0, 3.0):
        got = dict(zip(ss.NAMES, ds.soft32(m, s, values)))
        for g in got.values():
            g[cnt == 0] = np.array([ss.NAN_BITS], np.uint32).view(np.float32)[0]
        w = ss.check_combined(L, grid, boxes, H, W, s, values, got, what=f"{case[:6]} s={s}")
        print(f"restatement {case[:6]} s={s}: worst |error| / combined bound " + ", ".join(f"{k} {v:.4f}" for k, v in w.items()))
        assert all(0 < q <= 1 for q in w.values()), w


def test_checks_reject_what_is_wrong():
    H, W, grid, boxes, _ = ss.LAYOUTS["strip-255"]
    Cc, s = 17, 1.0
    values = ds.values_for(Cc)
    L = ss.integer_logits(len(boxes), grid, Cc, 3, special=False)
    m, cnt = ss.means32(L, grid, boxes, H, W)
    marker = np.array([ss.NAN_BITS], np.uint32).view(np.float32)[0]
    got = dict(zip(ss.NAMES, ds.soft32(m, s, values)))
    for g in got.values():
        g[cnt == 0] = marker
    ss.check_sharp(L, grid, boxes, H, W, s, values, got)
    y, x = np.argwhere(cnt > 0)[7]
    for name in ss.NAMES:
        off = got[name].copy()
        off[y, x] *= np.float32(1 + 2e-4)
        with pytest.raises(AssertionError, match=name):
            ss.check_sharp(L, grid, boxes, H, W, s, values, {name: off})
        lost = got[name].copy()
        lost[y, x] = marker                                          # a covered pixel written as undefined
        with pytest.raises(AssertionError, match="not a number"):
            ss.check_sharp(L, grid, boxes, H, W, s, values, {name: lost})
        filled = got[name].copy()
        filled[cnt == 0] = 0.0                                       # an uncovered pixel written as a number
        with pytest.raises(AssertionError, match="marker"):
            ss.check_sharp(L, grid, boxes, H, W, s, values, {name: filled})


def test_footprint_is_where_a_nan_corner_reaches():
    H, W, grid, boxes, _ = ss.LAYOUTS["flush-70x45"]
    n = len(boxes)
    L = ss.integer_logits(n, grid, 5, 9, special=False)
    L[3, 1 * 4 + 2, 4] = np.nan
    m, cnt = ss.means32(L, grid, boxes, H, W)
    assert np.array_equal(np.isnan(m).any(axis=-1), ss.footprint(boxes[3], grid, H, W, (1, 2)))
