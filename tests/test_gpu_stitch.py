"""The dense stitch on the GPU (vh_launch_dense_stitch, csrc/dense_stitch.hip; vit_hip_segment_frame_u8 / _device_u8): one
whole-frame window against the dense head's own launcher, bit for bit; overlapping windows on integer logits at the scales
where the header's fp32 expressions are exact, against tests/stitch_ref.py's restatement; real values under `check` and the
header's bound; every refusal of the launcher; and the frame calls on ViT-B/16 against the launcher applied to patch logits
collected by hand, in every precision, chunked and not, in both forms, with what a call must leave behind."""
import ctypes as C

import numpy as np
import pytest

import dense_ref as dr
import stitch_ref as sr

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
IP = C.POINTER(C.c_int)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def dev(pkg, a, dtype=np.float32):
    return pkg.DeviceBuffer.from_numpy(np.ascontiguousarray(a, dtype), dtype=dtype)


def test_constants_are_the_kernels(pkg):
    assert pkg.binding.STITCH_BLOCK == 16 and pkg.binding.STITCH_MAX_SIDE == 16384


def integer_logits(n, grid, Cc, seed):
    """tests/test_gpu_dense.py's recipe: integers in [-8, 8] (ties everywhere), 3 % of the entries NaN, +inf, -inf or -0, one
    patch all NaN, and from C = 5 on whole columns of NaN, +inf and -inf"""
    rng = np.random.default_rng(seed)
    P = grid[0] * grid[1]
    L = rng.integers(-8, 9, size=(n, P, Cc)).astype(np.float32)
    hit = rng.random(L.shape) < 0.03
    L[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0], np.float32), size=int(hit.sum()))
    L[n - 1, P // 2] = np.nan
    if Cc >= 5:
        L[:, :, 1], L[:, :, 2], L[:, :, Cc - 1] = np.nan, np.inf, -np.inf
        L[0, :, 2] = 8.0                                            # window 0 keeps a finite winner in most pixels
    return L


def run_stitch(pkg, d_logits, n, grid, Cc, boxes, H, W, fill=255, scores=True, cover=True, index=None):
    """-> (labels uint8 [H][W], scores float32, cover uint8); every output lies in a sentinel-filled buffer with 64 elements
    to spare, which must keep the sentinel, as must an output that is not asked for"""
    L = pkg.lib()
    b4 = sr.boxes4(boxes)
    offsets, ids = pkg.binding.stitch_index(H, W, b4) if index is None else index
    offsets, ids = np.ascontiguousarray(offsets, np.int32), np.ascontiguousarray(ids, np.int32)
    need = L.vh_dense_stitch_scratch(n, H, W, len(ids))
    assert need > 0
    d_scr = pkg.DeviceBuffer(need // 4 + 4)
    d_lab = dev(pkg, np.full(H * W + 64, 0xEE, np.uint8), np.uint8)
    d_sc = dev(pkg, np.full(H * W + 64, -7.0, np.float32))
    d_cov = dev(pkg, np.full(H * W + 64, 0xDD, np.uint8), np.uint8)
    rc = L.vh_launch_dense_stitch(None, d_logits.ptr, n, grid[0], grid[1], Cc, pkg.binding.fptr(b4), H, W, offsets.ctypes.data_as(IP),
                                  ids.ctypes.data_as(IP) if len(ids) else None, fill, d_scr.ptr, need, d_lab.ptr,
                                  d_sc.ptr if scores else None, d_cov.ptr if cover else None)
    assert rc == 0, L.vh_last_error().decode()
    assert L.vh_device_sync() == 0, L.vh_last_error().decode()
    lab, sc, cov = d_lab.to_numpy(), d_sc.to_numpy(), d_cov.to_numpy()
    assert (lab[H * W:] == 0xEE).all() and (sc[H * W:] == -7.0).all() and (cov[H * W:] == 0xDD).all()
    if not scores:
        assert (sc == -7.0).all()
    if not cover:
        assert (cov == 0xDD).all()
    return lab[:H * W].reshape(H, W), sc[:H * W].reshape(H, W), cov[:H * W].reshape(H, W)


def run_labels(pkg, d_logits, n, grid, Cc, out):
    L = pkg.lib()
    d_lab = dev(pkg, np.full(n * out[0] * out[1], 0xEE, np.uint8), np.uint8)
    d_sc = dev(pkg, np.full(n * out[0] * out[1], -7.0, np.float32))
    assert L.vh_launch_dense_labels(None, d_logits.ptr, n, grid[0], grid[1], Cc, out[0], out[1], d_lab.ptr, d_sc.ptr) == 0, L.vh_last_error().decode()
    assert L.vh_device_sync() == 0, L.vh_last_error().decode()
    return d_lab.to_numpy((n, out[0], out[1])), d_sc.to_numpy((n, out[0], out[1]))


# ---- 1. one whole-frame window is the dense head ----------------------------------------------------------------------

@pytest.mark.parametrize("grid,Cc,H,W", [((3, 5), 17, 37, 53), ((14, 14), 21, 224, 224), ((14, 14), 256, 7, 5), ((1, 1), 2, 33, 65)])
def test_one_whole_frame_window_is_the_dense_head(pkg, device, grid, Cc, H, W):
    """labels and score bits of the one window (0, 0, W, H) are vh_launch_dense_labels' at out_h = H, out_w = W: NaN, +-inf,
    -0 and an all-NaN patch among the logits"""
    Lg = integer_logits(1, grid, Cc, H + W + Cc)
    d_l = dev(pkg, Lg)
    lab, sc, cov = run_stitch(pkg, d_l, 1, grid, Cc, [(0.0, 0.0, float(W), float(H))], H, W)
    want_lab, want_sc = run_labels(pkg, d_l, 1, grid, Cc, (H, W))
    assert np.array_equal(lab, want_lab[0]) and same(sc, want_sc[0]) and (cov == 1).all()
    # real values too: the same expressions, whatever the data
    Lr = np.random.default_rng(Cc).standard_normal(Lg.shape).astype(np.float32)
    d_l = dev(pkg, Lr)
    lab, sc, _ = run_stitch(pkg, d_l, 1, grid, Cc, [(0.0, 0.0, float(W), float(H))], H, W)
    want_lab, want_sc = run_labels(pkg, d_l, 1, grid, Cc, (H, W))
    assert np.array_equal(lab, want_lab[0]) and same(sc, want_sc[0])


# ---- 2. exact on integers, with overlap -------------------------------------------------------------------------------

# name -> (H, W, grid, boxes, fill): integer corners, sides = grid x 2^k, so ratios and weights are dyadic
STRIP = [(0.0, 0.0, 32.0, 32.0), (16.0, 0.0, 48.0, 32.0), (32.0, 13.0, 64.0, 45.0), (8.0, 29.0, 24.0, 45.0)]
LAYOUTS = {
    "flush-70x45": (45, 70, (4, 4), sr.tiles(45, 70, 32, 16), 255),             # cover counts 1, 2, 3, 4, 6
    "40x40": (40, 40, (4, 4), sr.tiles(40, 40, 16, 8), 255),
    "strip-255": (45, 70, (4, 4), STRIP, 255),                                   # columns 64.. and more stay uncovered
    "strip-7": (45, 70, (2, 4), STRIP, 7),
    "stack-40": (45, 70, (4, 4), [(20.0, 8.0, 36.0, 24.0)] * 40, 255),           # 40 distinct-logit windows on one spot
}


@pytest.mark.parametrize("Cc", [2, 17, 33, 256])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_overlap_exact_on_integers(pkg, device, name, Cc):
    H, W, grid, boxes, fill = LAYOUTS[name]
    n = len(boxes)
    for special in (True, False):
        Lg = integer_logits(n, grid, Cc, 31 * n + Cc) if special else \
            np.random.default_rng(Cc + n).integers(-8, 9, size=(n, grid[0] * grid[1], Cc)).astype(np.float32)
        want_lab, want_bits, want_cov = sr.stitch32(Lg, grid, boxes, H, W, fill)
        d_l = dev(pkg, Lg)
        lab, sc, cov = run_stitch(pkg, d_l, n, grid, Cc, boxes, H, W, fill)
        assert np.array_equal(cov, want_cov)
        assert np.array_equal(lab, want_lab), (name, Cc, special, int((lab != want_lab).sum()))
        assert np.array_equal(bits(sc), want_bits)
        only, _, _ = run_stitch(pkg, d_l, n, grid, Cc, boxes, H, W, fill, scores=False, cover=False)
        assert np.array_equal(only, lab)
    if name == "flush-70x45":
        assert set(np.unique(cov)) == {1, 2, 3, 4, 6}
    if name.startswith("strip"):
        assert (cov == 0).any() and (lab[cov == 0] == fill).all()
    # a block's list may name more windows than cover it: every block lists them all, the bits are the same
    blocks = -(-H // 16) * -(-W // 16)
    everything = (np.arange(blocks + 1, dtype=np.int32) * n, np.tile(np.arange(n, dtype=np.int32), blocks))
    lab2, sc2, cov2 = run_stitch(pkg, d_l, n, grid, Cc, boxes, H, W, fill, index=everything)
    assert np.array_equal(lab2, lab) and same(sc2, sc) and np.array_equal(cov2, cov)


# ---- 3. real values ---------------------------------------------------------------------------------------------------

def run_logits(pkg, x, Wt, b):
    L = pkg.lib()
    n, P, E = x.shape
    Cc = Wt.shape[0]
    d_x, d_w, d_b = dev(pkg, x), dev(pkg, Wt), dev(pkg, b)
    d_o = pkg.DeviceBuffer(n * P * Cc)
    assert L.vh_launch_dense_logits(None, d_x.ptr, P * E, E, n, P, E, d_w.ptr, E, d_b.ptr, Cc, d_o.ptr) == 0, L.vh_last_error().decode()
    assert L.vh_device_sync() == 0, L.vh_last_error().decode()
    return d_o


@pytest.mark.parametrize("case", sr.FLOAT_CASES, ids=lambda c: f"{c[0]}x{c[1]}-t{c[2]}-C{c[5]}")
def test_real_values_hold_the_check(pkg, device, case):
    """Gaussian tokens and heads through vh_launch_dense_logits, then the stitch over boxes of fractional corners, some not
    square: every label is one the float64 definition admits within the header's bound, every score within it.  Measured
    worst |error| / bound on an MI355X, in the order of the cases: 0.027, 0.034, 0.092, 0.017; 0.00-0.09 % of the pixels admit
    more than one label."""
    H, W, tile, stride, grid, Cc, seed = case
    boxes = sr.float_boxes(case)
    n = len(boxes)
    x, Wt, b = sr.float_case(n, grid, Cc, seed)
    d_pl = run_logits(pkg, x, Wt, b)
    lab, sc, cov = run_stitch(pkg, d_pl, n, grid, Cc, boxes, H, W, 255)
    corner = (sr.E_FLOAT + 8) * dr.U * dr.absdot(x, Wt, b)
    worst, share = sr.check(dr.logits64(x, Wt, b), grid, boxes, H, W, 255, lab, sc, cov, corner)
    print(f"stitch {case[:6]}: worst |error| / bound = {worst:.4f}, {100 * share:.3f} % of the pixels admit more than one label")
    assert share <= 0.01


# ---- 4. refusals ------------------------------------------------------------------------------------------------------

def test_launcher_refusals(pkg, device):
    L = pkg.lib()
    H, W, grid, Cc = 45, 70, (4, 4), 6
    boxes = sr.boxes4(sr.tiles(H, W, 32, 16))
    n = len(boxes)
    offsets, ids = pkg.binding.stitch_index(H, W, boxes)
    Lg = np.random.default_rng(1).integers(-8, 9, size=(n, 16, Cc)).astype(np.float32)
    d_l = dev(pkg, np.concatenate([Lg.ravel(), np.zeros(64, np.float32)]))
    need = L.vh_dense_stitch_scratch(n, H, W, len(ids))
    d_scr = dev(pkg, np.full(need // 4 + 8, -7.0, np.float32))
    d_lab = dev(pkg, np.full(H * W + 64, 0xEE, np.uint8), np.uint8)
    d_sc = dev(pkg, np.full(H * W + 64, -7.0, np.float32))
    d_cov = dev(pkg, np.full(H * W + 64, 0xDD, np.uint8), np.uint8)
    off = lambda d, by: C.c_void_p(d.ptr.value + by)
    good = dict(pl=d_l.ptr, n=n, gh=4, gw=4, C=Cc, boxes=boxes, H=H, W=W, offsets=offsets, ids=ids, fill=255, scr=d_scr.ptr, bytes=need,
                lab=d_lab.ptr, sc=d_sc.ptr, cov=d_cov.ptr)

    def launch(**kw):
        a = dict(good)
        a.update(kw)
        bx = None if a["boxes"] is None else pkg.binding.fptr(np.ascontiguousarray(a["boxes"], np.float32))
        of = None if a["offsets"] is None else np.ascontiguousarray(a["offsets"], np.int32).ctypes.data_as(IP)
        keep = np.ascontiguousarray(a["ids"], np.int32) if a["ids"] is not None else None
        return L.vh_launch_dense_stitch(None, a["pl"], a["n"], a["gh"], a["gw"], a["C"], bx, a["H"], a["W"], of,
                                        None if keep is None else keep.ctypes.data_as(IP), a["fill"], a["scr"], a["bytes"], a["lab"],
                                        a["sc"], a["cov"])

    def box(i, **kw):
        b = boxes.copy()
        for k, v in kw.items():
            b[i, "ltrb".index(k)] = v
        return b

    def ids_with(j, v):
        out = ids.copy()
        out[j] = v
        return out

    def offsets_with(j, v):
        out = offsets.copy()
        out[j] = v
        return out

    bad = [dict(C=1), dict(C=257), dict(gh=0), dict(gw=0), dict(gh=65), dict(gw=65), dict(H=0), dict(W=0), dict(H=16385), dict(W=16385),
           dict(n=0), dict(n=-1), dict(n=2 ** 31 // 16), dict(fill=-1), dict(fill=256),
           dict(boxes=box(1, l=-1.0)), dict(boxes=box(2, r=70.5)), dict(boxes=box(0, t=-0.5)), dict(boxes=box(3, b=46.0)),
           dict(boxes=box(1, r=16.5)), dict(boxes=box(1, b=0.5)), dict(boxes=box(2, l=np.nan)), dict(boxes=box(2, r=np.inf)),
           dict(W=60),                                                   # boxes of a wider frame
           dict(offsets=offsets_with(0, 1)), dict(offsets=offsets_with(3, int(offsets[4]) + 1)), dict(ids=ids_with(0, -1)),
           dict(ids=ids_with(1, n)), dict(ids=ids_with(int(offsets[1]) + 1, int(ids[int(offsets[1])]))),   # not strictly ascending
           dict(bytes=need - 16), dict(bytes=0),
           dict(pl=None), dict(boxes=None), dict(offsets=None), dict(ids=None), dict(scr=None), dict(lab=None),
           dict(pl=off(d_l, 4)), dict(scr=off(d_scr, 8)), dict(lab=off(d_lab, 1)), dict(sc=off(d_sc, 4)), dict(cov=off(d_cov, 8))]
    assert offsets[2] - offsets[1] >= 2                                  # the case above needs two ids in block 1
    for kw in bad:
        L.vh_set_error(1, b"stale")
        assert launch(**kw) == 1, list(kw)
        msg = L.vh_last_error().decode()
        assert msg.startswith("vh_launch_dense_stitch: ") and len(msg) > 35, (list(kw), msg)
    assert L.vh_device_sync() == 0
    assert (d_lab.to_numpy() == 0xEE).all() and (d_sc.to_numpy() == -7.0).all() and (d_cov.to_numpy() == 0xDD).all()
    assert (d_scr.to_numpy() == -7.0).all()
    assert launch() == 0 and launch(sc=None, cov=None) == 0 and L.vh_device_sync() == 0, L.vh_last_error().decode()
    want_lab, want_bits, want_cov = sr.stitch32(Lg, grid, boxes, H, W, 255)
    m = H * W
    assert np.array_equal(d_lab.to_numpy()[:m].reshape(H, W), want_lab) and np.array_equal(bits(d_sc.to_numpy())[:m].reshape(H, W), want_bits)
    assert np.array_equal(d_cov.to_numpy()[:m].reshape(H, W), want_cov)
    assert (d_lab.to_numpy()[m:] == 0xEE).all() and (d_sc.to_numpy()[m:] == -7.0).all() and (d_cov.to_numpy()[m:] == 0xDD).all()


# ---- 5. the model -----------------------------------------------------------------------------------------------------

NL = 21
FH, FW, TILE, STRIDE = 260, 300, 224, 150


@pytest.fixture(scope="module")
def cfg(pkg):
    return pkg.preset("vit_b_16")


@pytest.fixture(scope="module")
def models(pkg, device, cfg, weights):
    """ViT-B/16, synthetic weights, one context per (precision, max_batch), made on first use"""
    made = {}

    def get(precision="f32", max_batch=8):
        key = (precision, max_batch)
        if key not in made:
            made[key] = pkg.ViTHip(cfg, weights, device=0, max_batch=max_batch, precision=precision)
        return made[key]

    yield get
    for m in made.values():
        m.close()


@pytest.fixture(scope="module")
def head(pkg, device):
    """a head of 21 labels over 768 columns, rows 772 apart, on the device once"""
    rng = np.random.default_rng(23)
    Wt = (rng.standard_normal((NL, 768)) / np.sqrt(768)).astype(np.float32)
    b = (0.1 * rng.standard_normal(NL)).astype(np.float32)
    padded = np.full((NL, 772), np.nan, np.float32)
    padded[:, :768] = Wt
    return Wt, b, dev(pkg, padded), dev(pkg, b)


@pytest.fixture(scope="module")
def frame(pkg, device):
    """a 260 x 300 frame of smooth structure plus noise, on the host and on the device, and its four windows"""
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:FH, 0:FW]
    base = np.stack([127 + 90 * np.sin(xx / 17.0 + c) * np.cos(yy / 23.0 - c) for c in range(3)], axis=-1)
    img = np.clip(base + rng.integers(-30, 31, size=base.shape), 0, 255).astype(np.uint8)
    windows = pkg.tile_boxes(FH, FW, TILE, STRIDE)
    assert len(windows) == 4
    return img, pkg.DeviceBuffer.from_numpy(img, dtype=np.uint8), windows


def by_hand(pkg, model, frame, head, tap=-1, final_norm=True, fill=255):
    """the patch logits of the windows collected through forward_device_u8_boxes with a device-form dense request, chunk by
    chunk, then the stitch launcher on them -> (labels, scores, cover)"""
    img, d_img, windows = frame
    n, P, mb = len(windows), model.tokens - 1, model.max_batch
    norm = pkg.pixel_norm(MEAN, STD)
    d_lab, d_pl = pkg.DeviceBuffer(mb * 16, np.uint8), pkg.DeviceBuffer(mb * P * NL)
    spec = pkg.binding.DenseSpec(NL, 1, 1, tap, final_norm, 772, head[2], head[3])
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
    return run_stitch(pkg, dev(pkg, pl), n, model.cfg.grid, NL, [w[1] for w in windows], FH, FW, fill)


def frame_device(pkg, model, frame, head, **kw):
    img, d_img, windows = frame
    d_lab = dev(pkg, np.full(FH * FW, 0xEE, np.uint8), np.uint8)
    d_sc, d_cov = dev(pkg, np.full(FH * FW, -7.0, np.float32)), dev(pkg, np.full(FH * FW, 0xDD, np.uint8), np.uint8)
    model.segment_frame_device((d_img.ptr.value, FH, FW, FW * 3), windows, pkg.pixel_norm(MEAN, STD), head[2], head[3], labels=d_lab,
                               scores=d_sc, cover=d_cov, n_labels=NL, weight_stride=772, **kw)
    return d_lab.to_numpy((FH, FW)), d_sc.to_numpy((FH, FW)), d_cov.to_numpy((FH, FW))


def plain_logits(pkg, model, images):
    n, nc = images.shape[0], model.cfg.num_classes
    d_img, d_l = pkg.DeviceBuffer.from_numpy(images), pkg.DeviceBuffer(n * nc)
    model.forward_device(d_img.ptr, n, d_l.ptr)
    model.sync()
    return d_l.to_numpy((n, nc))


def launch_counts(pkg, model, images):
    d_img = pkg.DeviceBuffer.from_numpy(images)
    model.profile_enable(1)
    model.forward_device(d_img.ptr, images.shape[0], None, None)
    got = {name: c for name, (_, c) in model.profile_read().items()}
    model.profile_enable(0)
    return got


@pytest.mark.parametrize("precision", ["f32", "bf16", "fp8"])
def test_frame_calls_are_the_launcher_on_collected_logits(pkg, models, cfg, frame, head, precision):
    """segment_frame (host form) and the device form give, bit for bit, the stitch launcher's labels, scores and cover on patch
    logits collected by hand; the same bits at max_batch 8 (one chunk) and 3 (chunks of 3 and 1); afterwards no dense request
    is armed, a plain forward gives the bits it gave before and launches what it launched before"""
    img, d_img, windows = frame
    Wt, b, d_w, d_b = head
    model, small = models(precision, 8), models(precision, 3)
    images = pkg.synth_images(cfg, 0, 2)
    before, counts = plain_logits(pkg, model, images), {m: launch_counts(pkg, m, images) for m in (model, small)}
    want = by_hand(pkg, model, frame, head)
    assert set(np.unique(want[2])) == {1, 2, 4} and len(np.unique(want[0])) > 1
    got_dev = frame_device(pkg, model, frame, head)
    got_host = model.segment_frame(img, Wt, b, tile=TILE, stride=STRIDE, mean=MEAN, std=STD, scores=True, cover=True)
    only = model.segment_frame(img, Wt, b, tile=TILE, stride=STRIDE, mean=MEAN, std=STD)
    for g, d, w in zip(got_host, got_dev, want):
        assert same(g, w) and same(d, w)
    assert only.dtype == np.uint8 and same(only, want[0])
    for other in (by_hand(pkg, small, frame, head), frame_device(pkg, small, frame, head),
                  small.segment_frame(img, Wt, b, tile=TILE, stride=STRIDE, mean=MEAN, std=STD, scores=True, cover=True)):
        for g, w in zip(other, want):
            assert same(g, w)
    # the default windows are tile_boxes(H, W, img_size, 2 * img_size // 3): stride 149 here
    dflt = model.segment_frame(img, Wt, b, mean=MEAN, std=STD)
    explicit = model.segment_frame(img, Wt, b, windows=pkg.tile_boxes(FH, FW, 224, 149), mean=MEAN, std=STD)
    assert same(dflt, explicit)
    # another tap, no final norm, another fill and a window list that leaves pixels uncovered
    part = (img, d_img, windows[:2])
    want2 = by_hand(pkg, model, part, head, tap=5, final_norm=False, fill=9)
    got2 = model.segment_frame(img, Wt, b, windows=windows[:2], mean=MEAN, std=STD, tap=5, final_norm=False, fill_label=9, scores=True, cover=True)
    for g, w in zip(got2, want2):
        assert same(g, w)
    assert (want2[2] == 0).any() and (want2[0][want2[2] == 0] == 9).all()
    # nothing is left armed (a dense request would add its launches to the classifier's) and nothing has moved
    assert same(plain_logits(pkg, model, images), before)
    for m in (model, small):
        assert launch_counts(pkg, m, images) == counts[m]


@pytest.mark.parametrize("layout", ["hwc", "chw"])
def test_host_form_takes_a_column_band_of_a_larger_array(pkg, models, frame, head, layout):
    """A frame whose rows lie row_stride apart with row_stride above the row's bytes -- the last FW columns of a wider array,
    handed over as the view it is, so that the frame's last row ends with the array: what lies between the rows is not the
    frame's, the upload ends with the last row's pixels, and labels, scores and cover are the contiguous frame's bits, in both
    layouts"""
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
    descs, keep = pkg.binding.host_image_descs([view], layout)
    assert descs[0].data == view.ctypes.data and descs[0].row_stride == (FW + pad) * (chans if layout == "hwc" else 1)
    assert view.ctypes.data + (descs[0].row_stride * (FH * (1 if layout == "hwc" else chans) - 1) + FW * (chans if layout == "hwc" else 1)) \
        == big.ctypes.data + big.nbytes                               # the last row's last pixel is the array's last byte
    kw = dict(tile=TILE, stride=STRIDE, mean=MEAN, std=STD, layout=layout, scores=True, cover=True)
    got = model.segment_frame(view, Wt, b, **kw)
    want = model.segment_frame(np.ascontiguousarray(view), Wt, b, **kw)
    plain = model.segment_frame(img, Wt, b, tile=TILE, stride=STRIDE, mean=MEAN, std=STD, scores=True, cover=True)
    for g, w, h in zip(got, want, plain):
        assert same(g, w) and same(g, h)
    assert len(np.unique(got[0])) > 1 and ((big[:, :pad] if layout == "hwc" else big[:, :, :pad]) == 0xA5).all()


def test_frame_call_refusals(pkg, device, models, cfg, frame, head):
    b, L = pkg.binding, pkg.lib()
    img, d_img, windows = frame
    Wt, bias, d_w, d_b = head
    model = models("f32", 8)
    norm = pkg.pixel_norm(MEAN, STD)
    d_lab = dev(pkg, np.full(FH * FW + 16, 0xEE, np.uint8), np.uint8)
    desc = b.image_descs([(d_img.ptr.value, FH, FW, FW * 3)])
    boxes = b.box_array(windows)
    good = dict(ctx=model.ctx, frame=desc, windows=boxes, n=len(windows), layout=0, filter=0, norm=C.byref(norm), out_h=0, out_w=0, fill=255,
                weight=d_w.ptr, labels=d_lab.ptr, spec=True, out=True)

    def call(entry=L.vit_hip_segment_frame_device_u8, **kw):
        a = dict(good)
        a.update(kw)
        fs = b.FrameSpecC(b.DenseSpecC(-1, 1, NL, a["out_h"], a["out_w"], 772, a["weight"], d_b.ptr), a["fill"])
        bufs = b.FrameBuffers(a["labels"], None, None)
        L.vh_set_error(1, b"stale")
        rc = entry(a["ctx"], a["frame"], a["windows"], a["n"], a["layout"], a["filter"], a["norm"], C.byref(fs) if a["spec"] else None,
                   C.byref(bufs) if a["out"] else None)
        return rc, L.vh_last_error().decode()

    def moved(i, box=None, image=0):
        arr = b.box_array(windows)
        arr[i] = b.Box(image, (C.c_float * 4)(*(box or windows[i][1])))
        return arr

    who = "vit_hip_segment_frame_device_u8: "
    refused = [(dict(ctx=None), "NULL"), (dict(frame=None), "NULL"), (dict(windows=None), "NULL"), (dict(norm=None), "NULL"),
               (dict(spec=False), "NULL"), (dict(out=False), "NULL"), (dict(labels=None), "labels"), (dict(weight=None), "weight"),
               (dict(labels=C.c_void_p(d_lab.ptr.value + 4)), "aligned"), (dict(out_h=224), "out_h"), (dict(out_w=1), "out_h"),
               (dict(fill=256), "fill_label"), (dict(fill=-1), "fill_label"), (dict(n=0), "n_windows"), (dict(layout=2), "layout"),
               (dict(filter=2), "filter"), (dict(windows=moved(1, image=1)), "image"), (dict(windows=moved(3, (100.0, 40.0, 301.0, 260.0))), "window 3"),
               (dict(windows=moved(0, (0.0, 0.0, 0.5, 224.0))), "window 0"), (dict(windows=moved(2, (0.0, -1.0, 224.0, 223.0))), "window 2"),
               (dict(frame=b.image_descs([(d_img.ptr.value, FH, FW, FW * 3 - 1)])), "row_stride"),
               (dict(frame=b.image_descs([(0, FH, FW, FW * 3)])), "NULL")]
    for kw, word in refused:
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith(who) and word in msg, (list(kw), msg)
    rc, msg = call(entry=L.vit_hip_segment_frame_u8, out_h=3)
    assert rc == 1 and msg.startswith("vit_hip_segment_frame_u8: ")
    model.sync()
    assert (d_lab.to_numpy() == 0xEE).all()
    # a caller's dense request, in either form, refuses the call and stays armed; so does any request armed in host form
    images = pkg.synth_images(cfg, 0, 1)
    spec = b.DenseSpec(NL, 20, 30, -1, True, 772, d_w, d_b)
    d_mine = dev(pkg, np.zeros(8 * 600, np.uint8), np.uint8)
    model.set_dense(spec, d_w, d_b, labels=d_mine)
    try:
        rc, msg = call()
        assert rc == 1 and msg.startswith(who) and "dense request" in msg
        plain_logits(pkg, model, images)
        assert d_mine.to_numpy((8, 20, 30))[0].any() and (d_lab.to_numpy() == 0xEE).all()
        host_lab = np.zeros((1, 20, 30), np.uint8)
        model.set_dense_host(b.DenseSpec(NL, 20, 30, -1, True, 772, d_w, d_b), d_w, d_b, labels=host_lab)
        rc, msg = call()
        assert rc == 1 and msg.startswith(who) and "dense request" in msg
        model.forward(images)
        assert host_lab.any()
    finally:
        model.set_dense_host(None)
        model.set_dense(None)
    h_top = np.zeros((1, 5), np.int32)
    model.set_topk_host(b.TopKSpec(5, "probs"), labels=h_top)
    try:
        rc, msg = call()
        assert rc == 1 and msg.startswith(who) and "vit_hip_set_topk_host" in msg
    finally:
        model.set_topk_host(None)
    wide = model.at_size(224, 320, max_batch=2)
    try:
        rc, msg = call(ctx=wide.ctx)
        assert rc == 1 and msg.startswith(who) and "non-square" in msg
    finally:
        wide.close()
    assert (d_lab.to_numpy() == 0xEE).all()
    # a request of another kind in device form is served per chunk, as by any forward
    d_top = dev(pkg, np.full(8 * 5, -1, np.int32), np.int32)
    model.set_topk(b.TopKSpec(5, "probs"), labels=d_top)
    try:
        rc, msg = call()
        assert rc == 0, msg
        assert (d_top.to_numpy((8, 5))[:4] >= 0).all() and (d_top.to_numpy((8, 5))[4:] == -1).all()
    finally:
        model.set_topk(None)
    assert (d_lab.to_numpy()[:FH * FW] != 0xEE).any() and (d_lab.to_numpy()[FH * FW:] == 0xEE).all()
