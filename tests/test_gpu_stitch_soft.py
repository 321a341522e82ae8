"""The soft stitch on the GPU (vh_launch_dense_stitch_soft, csrc/dense_stitch_soft.hip; vit_hip_segment_frame_soft_u8 /
_device_u8): one whole-frame window against the dense head's soft launcher, bit for bit, at every chunk count and on either
side of every switch between the kernel's variants and instances, each variant held against the other; overlapping windows on
integer logits, where tests/stitch_soft_ref.py's restated blend is the kernel's bits, within the sharp bounds; real values
within the combined bounds; which maps are asked for; special values; refusals; and the frame calls on ViT-B/16 against the
launcher applied to patch logits collected by hand, in every precision and both forms, with what a call must leave behind.
Measured worst |error| / bound on an MI355X: profiles/frame_soft_errors.txt."""
import ctypes as C

import numpy as np
import pytest

import dense_ref as dr
import dense_soft_ref as ds
import stitch_ref as sr
import stitch_soft_ref as ss
from test_gpu_stitch import FH, FW, MEAN, NL, STD, STRIDE, TILE, cfg, frame, frame_device, head, models, plain_logits, run_logits, run_stitch  # noqa: F401

pytestmark = pytest.mark.gpu

IP = C.POINTER(C.c_int)
VARIANTS = {1: "recompute", 2: "registers"}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def dev(pkg, a, dtype=np.float32):
    return pkg.DeviceBuffer.from_numpy(np.ascontiguousarray(a, dtype), dtype=dtype)


def launch_as(L, variant, *args):
    """the public launcher, or (variant 1, 2) the internal entry of csrc/vit_kernels.h that takes the variant as an argument of
    the call; its prototype is the public launcher's behind one int"""
    if variant == 0:
        return L.vh_launch_dense_stitch_soft(*args)
    fn = L.vh_launch_dense_stitch_soft_as
    fn.restype, fn.argtypes = C.c_int, [C.c_int] + list(L.vh_launch_dense_stitch_soft.argtypes)
    return fn(variant, *args)


def takes(variant, Cc):
    return variant in (0, 1) or (variant == 2 and Cc <= 160)


def run_soft_stitch(pkg, d_logits, n, grid, Cc, boxes, H, W, s, values, want=ss.NAMES, index=None, variant=0):
    """-> {name: float32 [H][W]} for the names in `want`; every map lies in a sentinel-filled buffer with 64 elements to
    spare, which must keep the sentinel, as must a map that is not asked for"""
    L = pkg.lib()
    b4 = sr.boxes4(boxes)
    offsets, ids = pkg.binding.stitch_index(H, W, b4) if index is None else index
    offsets, ids = np.ascontiguousarray(offsets, np.int32), np.ascontiguousarray(ids, np.int32)
    need = L.vh_dense_stitch_scratch(n, H, W, len(ids))
    assert need > 0
    d_scr = pkg.DeviceBuffer(need // 4 + 4)
    d_map = {o: dev(pkg, np.full(H * W + 64, -7.0, np.float32)) for o in ss.NAMES}
    d_val = dev(pkg, values) if "expect" in want else None
    rc = launch_as(L, variant, None, d_logits.ptr, n, grid[0], grid[1], Cc, pkg.binding.fptr(b4), H, W, offsets.ctypes.data_as(IP),
                   ids.ctypes.data_as(IP) if len(ids) else None, d_scr.ptr, need, s, None if d_val is None else d_val.ptr,
                   *[d_map[o].ptr if o in want else None for o in ss.NAMES])
    assert rc == 0, L.vh_last_error().decode()
    assert L.vh_device_sync() == 0, L.vh_last_error().decode()
    got = {}
    for o in ss.NAMES:
        a = d_map[o].to_numpy()
        assert (a[H * W:] == -7.0).all()
        if o in want:
            got[o] = a[:H * W].reshape(H, W)
        else:
            assert (a == -7.0).all()
    return got


def run_dense_soft(pkg, d_logits, grid, Cc, out, s, values):
    L = pkg.lib()
    d_map = [pkg.DeviceBuffer(out[0] * out[1]) for _ in ss.NAMES]
    d_val = dev(pkg, values)
    assert L.vh_launch_dense_soft(None, d_logits.ptr, 1, grid[0], grid[1], Cc, out[0], out[1], s, d_val.ptr, *[d.ptr for d in d_map]) == 0, \
        L.vh_last_error().decode()
    assert L.vh_device_sync() == 0, L.vh_last_error().decode()
    return {o: d.to_numpy(out) for o, d in zip(ss.NAMES, d_map)}


# ---- 1. one whole-frame window is the dense head's soft launcher ------------------------------------------------------

# the issue's five, then either side of every C at which the launcher changes its path: 32 | 33, 64 | 65 and 112 | 113 (the
# register variant's instances of 2, 4, 7 and 10 chunks), 160 | 161 (its limit: recompute beyond)
ONE_WINDOW = [((3, 5), 17, 37, 53), ((14, 14), 21, 224, 224), ((14, 14), 256, 7, 5), ((1, 1), 2, 33, 65), ((4, 4), 150, 45, 70),
              ((2, 3), 32, 19, 21), ((2, 3), 33, 19, 21), ((2, 3), 64, 19, 21), ((2, 3), 65, 19, 21), ((2, 3), 112, 19, 21), ((2, 3), 113, 19, 21),
              ((2, 3), 160, 19, 21), ((2, 3), 161, 19, 21)]


def test_every_switch_is_crossed(pkg):
    """what a launch takes by itself, it takes; and wherever that choice changes between C and C + 1, test 1 has both"""
    L = pkg.lib()
    by_c = {c: L.vh_dense_stitch_soft_variant(c) for c in range(2, 257)}
    assert all(v in VARIANTS and takes(v, c) for c, v in by_c.items())
    tested = {case[1] for case in ONE_WINDOW}
    for c in range(2, 256):
        if by_c[c] != by_c[c + 1]:
            assert c in tested and c + 1 in tested, c


@pytest.mark.parametrize("grid,Cc,H,W", ONE_WINDOW)
def test_one_whole_frame_window_is_the_dense_soft_launcher(pkg, device, grid, Cc, H, W):
    """the three maps of the one window (0, 0, W, H) are vh_launch_dense_soft's bits at out_h = H, out_w = W -- NaN, +-inf and
    -0 among integer logits, and Gaussian logits -- at three scales, and every variant that takes C gives those bits"""
    box = [(0.0, 0.0, float(W), float(H))]
    values = ds.values_for(Cc)
    for kind in ("integer", "gauss"):
        Lg = ss.mild_logits(1, grid, Cc, H + W + Cc) if kind == "integer" else np.random.default_rng(Cc).standard_normal((1, grid[0] * grid[1], Cc)).astype(np.float32)
        if kind == "integer":
            Lg[0, 0, 0], Lg[0, -1, Cc - 1] = np.nan, np.inf            # a corner patch each: markers around them
        d_l = dev(pkg, Lg)
        for s in ss.SCALES:
            want = run_dense_soft(pkg, d_l, grid, Cc, (H, W), s, values)
            got = run_soft_stitch(pkg, d_l, 1, grid, Cc, box, H, W, s, values)
            for o in ss.NAMES:
                assert same(got[o], want[o]), (kind, s, o, int((bits(got[o]) != bits(want[o])).sum()))
            marked = bits(got["prob"]) == ss.NAN_BITS
            assert marked.any() == (kind == "integer")                # (one patch: every pixel is around it)
        for variant in VARIANTS:
            if takes(variant, Cc):
                other = run_soft_stitch(pkg, d_l, 1, grid, Cc, box, H, W, 3.0, values, variant=variant)
                assert all(same(other[o], got[o]) for o in ss.NAMES), (kind, VARIANTS[variant])


# ---- 2. overlap, exact on integers ------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cc", ss.OVERLAP_C)
@pytest.mark.parametrize("name", list(ss.LAYOUTS))
def test_overlap_within_the_sharp_bounds_on_integers(pkg, device, name, Cc):
    """Integer logits under dyadic ratios: the restated blend is the kernel's bits, so every covered pixel is within the sharp
    bounds of the float64 soft maps on it, every uncovered or undefined pixel the marker.  The same bits from an index that
    lists every window for every block, from every variant, and at the shifted pixels of a larger frame"""
    H, W, grid, boxes, _ = ss.LAYOUTS[name]
    n = len(boxes)
    values = ds.values_for(Cc)
    worst = dict.fromkeys(ss.NAMES, 0.0)
    cnt = sr.cover_count(boxes, H, W)
    blocks = -(-H // 16) * -(-W // 16)
    everything = (np.arange(blocks + 1, dtype=np.int32) * n, np.tile(np.arange(n, dtype=np.int32), blocks))
    # plain: every covered pixel is a number.  mild: -inf and -0 among them, most pixels stay numbers.  special: from C = 5 on a
    # class of NaN throughout, so every pixel is the marker -- which is all that this data can show
    data = {"plain": ss.integer_logits(n, grid, Cc, 31 * n + Cc, special=False), "mild": ss.mild_logits(n, grid, Cc, n + Cc),
            "special": ss.integer_logits(n, grid, Cc, 31 * n + Cc)}
    for kind, Lg in data.items():
        d_l = dev(pkg, Lg)
        for s in (1.0, 3.0):
            got = run_soft_stitch(pkg, d_l, n, grid, Cc, boxes, H, W, s, values)
            w = ss.check_sharp(Lg, grid, boxes, H, W, s, values, got, f"{name} C={Cc} {kind} s={s}")
            worst = {k: max(worst[k], w[k]) for k in worst}
            numbers = bits(got["prob"]) != ss.NAN_BITS
            assert not numbers[cnt == 0].any()
            if kind == "plain":
                assert numbers[cnt > 0].all()
            if kind == "mild":
                assert numbers[cnt > 0].mean() > 0.4, (name, Cc, float(numbers[cnt > 0].mean()))
            # a block's list may name more windows than cover it: every block lists them all; and each variant against the default
            again = run_soft_stitch(pkg, d_l, n, grid, Cc, boxes, H, W, s, values, index=everything)
            assert all(same(again[o], got[o]) for o in ss.NAMES), (kind, s)
            for variant in VARIANTS:
                if takes(variant, Cc):
                    other = run_soft_stitch(pkg, d_l, n, grid, Cc, boxes, H, W, s, values, variant=variant)
                    assert all(same(other[o], got[o]) for o in ss.NAMES), (kind, s, VARIANTS[variant])
                    wide = run_soft_stitch(pkg, d_l, n, grid, Cc, boxes, H, W, s, values, variant=variant, index=everything)
                    assert all(same(wide[o], got[o]) for o in ss.NAMES), (kind, s, VARIANTS[variant], "every window in every block")
    print(f"soft stitch {name} C={Cc}: worst |error| / sharp bound " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    if name == "flush-70x45":
        assert set(np.unique(cnt)) == {1, 2, 3, 4, 6}
    if name.startswith("strip"):
        assert (cnt == 0).any()
    # the same windows 16 px to the right and 32 px down in a frame 32 px larger each way
    d_l = dev(pkg, data["mild"])
    here = run_soft_stitch(pkg, d_l, n, grid, Cc, boxes, H, W, 1.0, values)
    assert (bits(here["prob"]) != ss.NAN_BITS).any()
    moved = [(l + 16.0, t + 32.0, r + 16.0, b + 32.0) for l, t, r, b in boxes]
    there = run_soft_stitch(pkg, d_l, n, grid, Cc, moved, H + 32, W + 32, 1.0, values)
    for o in ss.NAMES:
        assert same(there[o][32:32 + H, 16:16 + W], here[o])
        rest = bits(there[o]).copy()
        rest[32:32 + H, 16:16 + W] = ss.NAN_BITS
        assert (rest == ss.NAN_BITS).all()


# ---- 3. real values ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", sr.FLOAT_CASES, ids=lambda c: f"{c[0]}x{c[1]}-t{c[2]}-C{c[5]}")
def test_real_values_within_the_combined_bounds(pkg, device, case):
    """Gaussian tokens and heads through vh_launch_dense_logits, then the soft stitch over boxes of fractional corners: every
    pixel within the combined bounds of the definition in float64 throughout, at two scales"""
    H, W, tile, stride, grid, Cc, seed = case
    boxes = sr.float_boxes(case)
    n = len(boxes)
    x, Wt, b = sr.float_case(n, grid, Cc, seed)
    d_pl = run_logits(pkg, x, Wt, b)
    corner = (sr.E_FLOAT + 8) * dr.U * dr.absdot(x, Wt, b)
    values = ds.values_for(Cc)
    L64 = dr.logits64(x, Wt, b)
    for s in (1.0, 3.0):
        got = run_soft_stitch(pkg, d_pl, n, grid, Cc, boxes, H, W, s, values)
        w = ss.check_combined(L64, grid, boxes, H, W, s, values, got, corner, f"{case[:6]} s={s}")
        print(f"soft stitch {case[:6]} s={s}: worst |error| / combined bound " + ", ".join(f"{k} {v:.4f}" for k, v in w.items()))


# ---- 4. which maps are asked for; the label stitch beside it ----------------------------------------------------------

def test_each_map_alone_each_pair_and_all_three(pkg, device):
    H, W, grid, boxes, fill = ss.LAYOUTS["flush-70x45"]
    n, Cc = len(boxes), 21
    values = ds.values_for(Cc)
    Lg = np.random.default_rng(4).standard_normal((n, 16, Cc)).astype(np.float32)
    d_l = dev(pkg, Lg)
    full = run_soft_stitch(pkg, d_l, n, grid, Cc, boxes, H, W, 1.0, values)
    for want in (("prob",), ("expect",), ("entropy",), ("prob", "expect"), ("prob", "entropy"), ("expect", "entropy")):
        for variant in (0, 1, 2):
            part = run_soft_stitch(pkg, d_l, n, grid, Cc, boxes, H, W, 1.0, values, want=want, variant=variant)
            assert set(part) == set(want) and all(same(part[o], full[o]) for o in want), (want, variant)
    # the label stitch, alone and with the soft launcher queued behind it on the same stream, each with its own scratch
    alone = run_stitch(pkg, d_l, n, grid, Cc, boxes, H, W, fill)
    L = pkg.lib()
    b4 = sr.boxes4(boxes)
    offsets, ids = [np.ascontiguousarray(a, np.int32) for a in pkg.binding.stitch_index(H, W, b4)]
    need = L.vh_dense_stitch_scratch(n, H, W, len(ids))
    scr = [pkg.DeviceBuffer(need // 4 + 4) for _ in range(2)]
    d_lab, d_cov = dev(pkg, np.full(H * W, 0xEE, np.uint8), np.uint8), dev(pkg, np.full(H * W, 0xDD, np.uint8), np.uint8)
    d_sc, d_p = dev(pkg, np.full(H * W, -7.0, np.float32)), dev(pkg, np.full(H * W, -7.0, np.float32))
    args = (n, grid[0], grid[1], Cc, pkg.binding.fptr(b4), H, W, offsets.ctypes.data_as(IP), ids.ctypes.data_as(IP))
    assert L.vh_launch_dense_stitch(None, d_l.ptr, *args, fill, scr[0].ptr, need, d_lab.ptr, d_sc.ptr, d_cov.ptr) == 0, L.vh_last_error().decode()
    assert L.vh_launch_dense_stitch_soft(None, d_l.ptr, *args, scr[1].ptr, need, 1.0, None, d_p.ptr, None, None) == 0, L.vh_last_error().decode()
    assert L.vh_device_sync() == 0, L.vh_last_error().decode()
    assert same(d_lab.to_numpy((H, W)), alone[0]) and same(d_sc.to_numpy((H, W)), alone[1]) and same(d_cov.to_numpy((H, W)), alone[2])
    assert same(d_p.to_numpy((H, W)), full["prob"])


# ---- 5. special values ------------------------------------------------------------------------------------------------

def test_special_values(pkg, device):
    H, W, grid, boxes, _ = ss.LAYOUTS["flush-70x45"]
    n, Cc = len(boxes), 19
    values = ds.values_for(Cc)
    base = ss.integer_logits(n, grid, Cc, 77, special=False)
    clean = run_soft_stitch(pkg, dev(pkg, base), n, grid, Cc, boxes, H, W, 1.0, values)
    assert not any((bits(g) == ss.NAN_BITS).any() for g in clean.values())           # every pixel of this layout is covered
    # a NaN logit in one window: the marker exactly where a corner of the pixel in that window is that patch
    Lg = base.copy()
    Lg[4, 2 * 4 + 1, 7] = np.nan
    got = run_soft_stitch(pkg, dev(pkg, Lg), n, grid, Cc, boxes, H, W, 1.0, values)
    reach = ss.footprint(boxes[4], grid, H, W, (2, 1))
    assert reach.any() and not reach.all()
    for o in ss.NAMES:
        assert np.array_equal(bits(got[o]) == ss.NAN_BITS, reach), o
        assert np.array_equal(bits(got[o])[~reach], bits(clean[o])[~reach]), o
    # a class of -inf everywhere is that class removed, for prob and entropy -- but under a weight of 0, where 0 * inf is NaN
    Lg = np.insert(base, 5, -np.inf, axis=2)
    got = run_soft_stitch(pkg, dev(pkg, Lg), n, grid, Cc + 1, boxes, H, W, 1.0, np.insert(values, 5, 0.0))
    m, _ = ss.means32(Lg, grid, boxes, H, W)
    undefined = np.isnan(m).any(axis=-1)
    assert 0 < undefined.mean() < 0.5
    for o in ("prob", "entropy"):
        assert np.array_equal(bits(got[o]) == ss.NAN_BITS, undefined), o
        assert np.array_equal(bits(got[o])[~undefined], bits(clean[o])[~undefined]), o
    # a maximum of +inf: the marker wherever that window reaches
    Lg = base.copy()
    Lg[4, :, 3] = np.inf
    got = run_soft_stitch(pkg, dev(pkg, Lg), n, grid, Cc, boxes, H, W, 1.0, values)
    inside = sr.cover_count([boxes[4]], H, W) > 0
    for o in ss.NAMES:
        assert np.array_equal(bits(got[o]) == ss.NAN_BITS, inside), o
    # two windows over the same pixels, +inf in one and -inf in the other of one class: inf - inf in the blend
    two = [(8.0, 8.0, 40.0, 40.0)] * 2
    Lg = ss.integer_logits(2, grid, Cc, 78, special=False)
    finite = run_soft_stitch(pkg, dev(pkg, Lg), 2, grid, Cc, two, H, W, 1.0, values)
    inside = sr.cover_count(two[:1], H, W) > 0
    assert np.array_equal(bits(finite["prob"]) == ss.NAN_BITS, ~inside)
    Lg[0, :, 2], Lg[1, :, 2] = np.inf, -np.inf
    got = run_soft_stitch(pkg, dev(pkg, Lg), 2, grid, Cc, two, H, W, 1.0, values)
    assert all((bits(g) == ss.NAN_BITS).all() for g in got.values())


# ---- 6. refusals leave the outputs untouched --------------------------------------------------------------------------

def test_launcher_refusals_write_nothing(pkg, device):
    L = pkg.lib()
    H, W, grid, Cc = 45, 70, (4, 4), 6
    boxes = sr.boxes4(sr.tiles(H, W, 32, 16))
    n = len(boxes)
    offsets, ids = pkg.binding.stitch_index(H, W, boxes)
    Lg = np.random.default_rng(1).integers(-8, 9, size=(n, 16, Cc)).astype(np.float32)
    values = ds.values_for(Cc)
    d_l = dev(pkg, np.concatenate([Lg.ravel(), np.zeros(64, np.float32)]))
    d_v = dev(pkg, np.concatenate([values, np.zeros(8, np.float32)]))
    need = L.vh_dense_stitch_scratch(n, H, W, len(ids))
    d_scr = dev(pkg, np.full(need // 4 + 8, -7.0, np.float32))
    d_map = [dev(pkg, np.full(H * W + 64, -7.0, np.float32)) for _ in ss.NAMES]
    off = lambda d, by: C.c_void_p(d.ptr.value + by)
    good = dict(pl=d_l.ptr, n=n, gh=4, gw=4, C=Cc, boxes=boxes, H=H, W=W, offsets=offsets, ids=ids, scr=d_scr.ptr, bytes=need, s=1.0,
                values=d_v.ptr, prob=d_map[0].ptr, expect=d_map[1].ptr, entropy=d_map[2].ptr)

    def launch(**kw):
        a = dict(good)
        a.update(kw)
        bx = None if a["boxes"] is None else pkg.binding.fptr(np.ascontiguousarray(a["boxes"], np.float32))
        of = None if a["offsets"] is None else np.ascontiguousarray(a["offsets"], np.int32)
        keep = None if a["ids"] is None else np.ascontiguousarray(a["ids"], np.int32)
        return L.vh_launch_dense_stitch_soft(None, a["pl"], a["n"], a["gh"], a["gw"], a["C"], bx, a["H"], a["W"],
                                             None if of is None else of.ctypes.data_as(IP), None if keep is None else keep.ctypes.data_as(IP),
                                             a["scr"], a["bytes"], a["s"], a["values"], a["prob"], a["expect"], a["entropy"])

    def changed(arr, j, v):
        out = np.array(arr).copy()
        out[j] = v
        return out

    wide = boxes.copy()
    wide[2, 2] = 70.5
    bad = [dict(s=0.0), dict(s=float("nan")), dict(values=None), dict(expect=None), dict(prob=None, expect=None, entropy=None, values=None),
           dict(C=1), dict(C=257), dict(gh=65), dict(H=0), dict(n=0), dict(boxes=wide), dict(W=60), dict(offsets=changed(offsets, 0, 1)),
           dict(ids=changed(ids, 1, n)), dict(ids=changed(ids, 0, -1)), dict(bytes=need - 16), dict(pl=None), dict(scr=None), dict(ids=None),
           dict(pl=off(d_l, 4)), dict(scr=off(d_scr, 8)), dict(values=off(d_v, 8)), dict(prob=off(d_map[0], 4)), dict(expect=off(d_map[1], 8)),
           dict(entropy=off(d_map[2], 4))]
    for kw in bad:
        L.vh_set_error(1, b"stale")
        assert launch(**kw) == 1, list(kw)
        msg = L.vh_last_error().decode()
        assert msg.startswith("vh_launch_dense_stitch_soft: ") and len(msg) > 40, (list(kw), msg)
    assert L.vh_device_sync() == 0
    assert all((d.to_numpy() == -7.0).all() for d in d_map) and (d_scr.to_numpy() == -7.0).all()
    assert launch() == 0 and L.vh_device_sync() == 0, L.vh_last_error().decode()
    got = {o: d.to_numpy()[:H * W].reshape(H, W) for o, d in zip(ss.NAMES, d_map)}
    ss.check_sharp(Lg, grid, boxes, H, W, 1.0, values, got)
    assert all((d.to_numpy()[H * W:] == -7.0).all() for d in d_map)


# ---- 7. the frame calls -----------------------------------------------------------------------------------------------

SCALE = 2.0


@pytest.fixture(scope="module")
def bins(pkg, device):
    v = np.linspace(0.5, 80.0, NL).astype(np.float32)
    return v, dev(pkg, v)


def collect(pkg, model, frame, head):
    """the patch logits of the frame's windows through forward_device_u8_boxes with a device-form dense request, chunk by
    chunk: tests/test_gpu_stitch.py's by_hand, up to the launcher"""
    img, d_img, windows = frame
    n, P, mb = len(windows), model.tokens - 1, model.max_batch
    norm = pkg.pixel_norm(MEAN, STD)
    d_lab, d_pl = pkg.DeviceBuffer(mb * 16, np.uint8), pkg.DeviceBuffer(mb * P * NL)
    spec = pkg.binding.DenseSpec(NL, 1, 1, -1, True, 772, head[2], head[3])
    pl = np.empty((n, P, NL), np.float32)
    model.set_dense(spec, spec.d_weight, spec.d_bias, labels=d_lab, patch_logits=d_pl)
    try:
        for a in range(0, n, mb):
            m = min(mb, n - a)
            model.forward_device_u8_boxes([(d_img.ptr.value, FH, FW, FW * 3)], windows[a:a + m], norm)
            model.sync()
            pl[a:a + m] = d_pl.to_numpy((mb, P, NL))[:m]
    finally:
        model.set_dense(None)
    return pl


def soft_device(pkg, model, frame, head, bins, labels=True, want=ss.NAMES):
    """the device form into sentinel-filled buffers -> ({map name: [FH][FW]}, (labels, scores, cover) or None)"""
    img, d_img, windows = frame
    d_map = {o: dev(pkg, np.full(FH * FW, -7.0, np.float32)) for o in want}
    d_lab = dev(pkg, np.full(FH * FW, 0xEE, np.uint8), np.uint8) if labels else None
    d_sc = dev(pkg, np.full(FH * FW, -7.0, np.float32)) if labels else None
    d_cov = dev(pkg, np.full(FH * FW, 0xDD, np.uint8), np.uint8) if labels else None
    model.segment_frame_soft_device((d_img.ptr.value, FH, FW, FW * 3), windows, pkg.pixel_norm(MEAN, STD), head[2], head[3],
                                    values=bins[1] if "expect" in want else None, logit_scale=SCALE, labels=d_lab, scores=d_sc, cover=d_cov,
                                    n_labels=NL, weight_stride=772, **d_map)
    maps = {o: d.to_numpy((FH, FW)) for o, d in d_map.items()}
    return maps, (d_lab.to_numpy((FH, FW)), d_sc.to_numpy((FH, FW)), d_cov.to_numpy((FH, FW))) if labels else None


def head_launches(model, run):
    model.profile_enable(8)
    try:
        out = run()
        return out, model.profile_read()["head_gemm"][1]
    finally:
        model.profile_enable(0)


@pytest.mark.parametrize("precision", ["f32", "bf16", "fp8"])
def test_frame_calls_are_the_launchers_on_collected_logits(pkg, models, cfg, frame, head, bins, precision):
    """The device form's maps are the soft launcher's bits on patch logits collected by hand, its labels, scores and cover
    vit_hip_segment_frame_device_u8's; without labels one launch less under VIT_OP_HEAD and the same maps; the host form and
    ViTHip.segment_frame_soft with tile / stride equal it; afterwards nothing is armed and nothing has moved"""
    img, d_img, windows = frame
    Wt, b, d_w, d_b = head
    model = models(precision, 8)
    images = pkg.synth_images(cfg, 0, 2)
    before = plain_logits(pkg, model, images)
    E = model.cfg.embed_dim
    d_cls = dev(pkg, np.zeros(8 * E, np.float32))
    model.set_features(pkg.binding.FeatureSpec(), cls=d_cls)
    try:
        assert same(plain_logits(pkg, model, images), before)
        cls_before = d_cls.to_numpy((8, E))[:2].copy()
        pl = collect(pkg, model, frame, head)
        boxes = [w[1] for w in windows]
        want = run_soft_stitch(pkg, dev(pkg, pl), len(windows), model.cfg.grid, NL, boxes, FH, FW, SCALE, bins[0])
        want_lab = frame_device(pkg, model, frame, head)
        (maps, labs), with_labels = head_launches(model, lambda: soft_device(pkg, model, frame, head, bins))
        (bare, none), without = head_launches(model, lambda: soft_device(pkg, model, frame, head, bins, labels=False))
        assert with_labels == without + 1 and none is None
        for o in ss.NAMES:
            assert same(maps[o], want[o]) and same(bare[o], want[o]), o
        for g, w in zip(labs, want_lab):
            assert same(g, w)
        assert np.isfinite(maps["prob"]).all() and len(np.unique(labs[0])) > 1 and set(np.unique(labs[2])) == {1, 2, 4}
        assert (maps["prob"] > 0).all() and (maps["prob"] <= 1).all() and (maps["entropy"] >= 0).all()
        assert (maps["expect"] >= bins[0].min()).all() and (maps["expect"] <= bins[0].max()).all()
        only, _ = soft_device(pkg, model, frame, head, bins, labels=False, want=("entropy",))
        assert same(only["entropy"], want["entropy"])
        # the host form, and the wrapper that tiles the frame itself
        host = model.segment_frame_soft(img, Wt, b, values=bins[0], logit_scale=SCALE, windows=windows, want=ss.NAMES, scores=True, cover=True,
                                        mean=MEAN, std=STD)
        tiled = model.segment_frame_soft(img, Wt, b, values=bins[0], logit_scale=SCALE, tile=TILE, stride=STRIDE, want=ss.NAMES, scores=True,
                                         cover=True, mean=MEAN, std=STD)
        for got in (host, tiled):
            assert set(got) == set(ss.NAMES) | {"labels", "scores", "cover"}
            assert all(same(got[o], want[o]) for o in ss.NAMES)
            assert all(same(got[o], w) for o, w in zip(("labels", "scores", "cover"), want_lab))
        lean = model.segment_frame_soft(img, Wt, b, tile=TILE, stride=STRIDE, logit_scale=SCALE, labels=False, mean=MEAN, std=STD)
        assert set(lean) == {"prob"} and same(lean["prob"], want["prob"])
        # no dense request is armed; the class logits and the feature request armed beside the calls are a plain forward's
        assert same(plain_logits(pkg, model, images), before) and same(d_cls.to_numpy((8, E))[:2], cls_before)
        spec = pkg.binding.DenseSpec(NL, 20, 30, -1, True, 772, d_w, d_b)
        d_mine = dev(pkg, np.zeros(8 * 600, np.uint8), np.uint8)
        model.set_dense(spec, d_w, d_b, labels=d_mine)                # arming succeeds and works: nothing of the calls' is in the way
        model.set_dense(None)
    finally:
        model.set_features(None)
    assert same(plain_logits(pkg, model, images), before)


@pytest.mark.parametrize("layout", ["hwc", "chw"])
def test_host_form_takes_a_column_band_of_a_larger_array(pkg, models, frame, head, bins, layout):
    img, _, windows = frame
    Wt, b, _, _ = head
    model = models("f32", 8)
    pad, chans = 52, 3
    if layout == "hwc":
        big = np.full((FH, FW + pad, chans), 0xA5, np.uint8)
        big[:, pad:] = img
        view = big[:, pad:]
    else:
        big = np.full((chans, FH, FW + pad), 0xA5, np.uint8)
        big[:, :, pad:] = img.transpose(2, 0, 1)
        view = big[:, :, pad:]
    assert not view.flags.c_contiguous
    kw = dict(values=bins[0], logit_scale=SCALE, tile=TILE, stride=STRIDE, want=ss.NAMES, cover=True, mean=MEAN, std=STD)
    got = model.segment_frame_soft(view, Wt, b, layout=layout, **kw)
    plain = model.segment_frame_soft(img, Wt, b, **kw)
    assert set(got) == set(plain) and all(same(got[o], plain[o]) for o in got)
    assert ((big[:, :pad] if layout == "hwc" else big[:, :, :pad]) == 0xA5).all()


def test_frame_call_refusals(pkg, device, models, cfg, frame, head, bins):
    """every refusal of the soft calls, by the entry point's name, leaves the buffers and the context as they were"""
    b, L = pkg.binding, pkg.lib()
    img, d_img, windows = frame
    Wt, bias, d_w, d_b = head
    model = models("f32", 8)
    norm = pkg.pixel_norm(MEAN, STD)
    d_lab = dev(pkg, np.full(FH * FW + 16, 0xEE, np.uint8), np.uint8)
    d_sc = dev(pkg, np.full(FH * FW + 16, -7.0, np.float32))
    d_map = [dev(pkg, np.full(FH * FW + 16, -7.0, np.float32)) for _ in ss.NAMES]
    desc = b.image_descs([(d_img.ptr.value, FH, FW, FW * 3)])
    boxes = b.box_array(windows)
    off = lambda d, by: C.c_void_p(d.ptr.value + by)
    good = dict(ctx=model.ctx, frame=desc, windows=boxes, n=len(windows), layout=0, filter=0, norm=C.byref(norm), out_h=0, out_w=0, fill=255,
                weight=d_w.ptr, labels=d_lab.ptr, scores=None, cover=None, spec=True, out=True, soft=True, maps=True, s=SCALE, values=bins[1].ptr,
                prob=d_map[0].ptr, expect=d_map[1].ptr, entropy=d_map[2].ptr)

    def call(entry=L.vit_hip_segment_frame_soft_device_u8, **kw):
        a = dict(good)
        a.update(kw)
        fs = b.FrameSpecC(b.DenseSpecC(-1, 1, NL, a["out_h"], a["out_w"], 772, a["weight"], d_b.ptr), a["fill"])
        bufs = b.FrameBuffers(a["labels"], a["scores"], a["cover"])
        soft, maps = b.DenseSoftSpecC(a["s"], a["values"]), b.DenseSoftBuffers(a["prob"], a["expect"], a["entropy"])
        L.vh_set_error(1, b"stale")
        rc = entry(a["ctx"], a["frame"], a["windows"], a["n"], a["layout"], a["filter"], a["norm"], C.byref(fs) if a["spec"] else None,
                   C.byref(soft) if a["soft"] else None, C.byref(bufs) if a["out"] else None, C.byref(maps) if a["maps"] else None)
        return rc, L.vh_last_error().decode()

    def moved(i, box=None, image=0):
        arr = b.box_array(windows)
        arr[i] = b.Box(image, (C.c_float * 4)(*(box or windows[i][1])))
        return arr

    images = pkg.synth_images(cfg, 0, 1)
    before = plain_logits(pkg, model, images)
    who = "vit_hip_segment_frame_soft_device_u8: "
    refused = [(dict(ctx=None), "NULL"), (dict(frame=None), "NULL"), (dict(windows=None), "NULL"), (dict(norm=None), "NULL"), (dict(spec=False), "NULL"),
               (dict(soft=False), "NULL"), (dict(maps=False), "NULL"), (dict(weight=None), "weight"),
               (dict(labels=off(d_lab, 4)), "aligned"), (dict(prob=off(d_map[0], 4)), "aligned"), (dict(entropy=off(d_map[2], 8)), "aligned"),
               (dict(values=off(bins[1], 4)), "aligned"), (dict(out_h=224), "out_h"), (dict(fill=256), "fill_label"), (dict(n=0), "n_windows"),
               (dict(layout=2), "layout"), (dict(filter=2), "filter"), (dict(windows=moved(1, image=1)), "image"),
               (dict(windows=moved(3, (100.0, 40.0, 301.0, 260.0))), "window 3"),
               (dict(s=0.0), "logit_scale"), (dict(s=float("nan")), "logit_scale"), (dict(s=float("inf")), "logit_scale"),
               (dict(prob=None, expect=None, entropy=None, values=None), "no soft map"), (dict(values=None), "d_values"), (dict(expect=None), "d_values"),
               (dict(labels=None, scores=d_sc.ptr), "need a labels"), (dict(labels=None, cover=d_lab.ptr), "need a labels"),
               (dict(out=False, labels=None, expect=None), "d_values")]
    for kw, word in refused:
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith(who) and word in msg, (list(kw), msg)
    rc, msg = call(entry=L.vit_hip_segment_frame_soft_u8, s=-1.0)
    assert rc == 1 and msg.startswith("vit_hip_segment_frame_soft_u8: ") and "logit_scale" in msg
    # a dense request of the caller's -- soft-armed too -- refuses the call and stays armed; the labels calls refuse alike
    d_mine = dev(pkg, np.zeros(8 * 600, np.float32))
    model.set_dense_soft(b.DenseSpec(NL, 20, 30, -1, True, 772, d_w, d_b), d_w, d_b, prob=d_mine)
    try:
        rc, msg = call()
        assert rc == 1 and msg.startswith(who) and "dense request" in msg
        plain_logits(pkg, model, images)
        assert d_mine.to_numpy((8, 20, 30))[0].all()
    finally:
        model.set_dense_soft(None)
    model.sync()
    assert (d_lab.to_numpy() == 0xEE).all() and (d_sc.to_numpy() == -7.0).all() and all((d.to_numpy() == -7.0).all() for d in d_map)
    assert same(plain_logits(pkg, model, images), before)
    # and the call itself, without d_out at all
    rc, msg = call(out=False, labels=None)
    assert rc == 0, msg
    model.sync()
    assert (d_lab.to_numpy() == 0xEE).all() and all((d.to_numpy()[:FH * FW] != -7.0).all() and (d.to_numpy()[FH * FW:] == -7.0).all() for d in d_map)
