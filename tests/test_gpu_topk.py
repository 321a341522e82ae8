"""Top-k predictions on the GPU (vh_launch_topk, csrc/topk.hip; vit_hip_set_topk / _host): the launcher on crafted rows at
every boundary of wave, workgroup, registers per thread and the register / rescan switch, and the model-level guarantees
the header states (labels of the forward's own logits, scores the probabilities' own bits, nothing else moves, both forms,
batch-position independence, arming rules, a label space beyond the softmax's 2048 entries)."""
import ctypes as C
import math

import numpy as np
import pytest

import topk_ref as tr

pytestmark = pytest.mark.gpu

PROBS, LOGITS = 0, 1
LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 2047, 2048, 2049, 4097, 21843, 65536]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def long_row_bound(length):
    """relative to the float64 softmax of the same fp32 logits: ceil(length / 256) serial adds per thread, 8 reduction
    levels, expf, the subtraction at |v - mx| <= 8 and the division, one 2^-24 each (32 covers the last four)"""
    return (math.ceil(length / 256) + 32) * 2.0 ** -24


def craft(pkg, length):
    """five rows of uniform [-4, 4): 0 the maximum duplicated at the first and last index; 1 a run of 40 equal values
    (longer than any k) across index 2048, or at the end of a shorter row; 2 all negative with -0.0 / +0.0 at scattered
    indices, so the zeros are the best entries; 3 two +inf; 4 two -inf"""
    data = np.empty(5 * length, np.float32)
    pkg.lib().vit_synth_fill(pkg.binding.fptr(data), data.size, 1000 + length, 4.0, 0.0)
    data = data.reshape(5, length)
    data[0, 0] = data[0, -1] = 5.0
    start = min(2030, max(0, length - 40))
    data[1, start:start + 40] = 4.5
    data[2] = -np.abs(data[2]) - 1.0
    for j, idx in enumerate(sorted({i for i in (1, 3, length // 2, length - 2, 2047, 2048) if 0 <= i < length})):
        data[2, idx] = -0.0 if j % 2 == 0 else 0.0
    data[3, [length // 3, length - 1]] = np.inf
    data[4, [0, length // 2]] = -np.inf
    return data


def launch_topk(pkg, d_in_ptr, rows, length, k, kind, want_scores=True):
    L = pkg.lib()
    d_lab, d_sc = pkg.DeviceBuffer(rows * k, np.int32), pkg.DeviceBuffer(rows * k)
    rc = L.vh_launch_topk(None, d_in_ptr, rows, length, k, kind, d_lab.ptr, d_sc.ptr if want_scores else None)
    assert rc == 0, L.vh_last_error().decode()
    assert L.vh_device_sync() == 0, L.vh_last_error().decode()
    return d_lab.to_numpy((rows, k)), d_sc.to_numpy((rows, k))


# ---- 1. the launcher ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("length", LENGTHS)
def test_launcher_on_crafted_rows(pkg, device, length):
    """Labels exact in both score kinds; LOGITS scores the input's bits; PROBS scores the softmax kernel's bits up to 2048
    entries, within long_row_bound of the float64 softmax beyond.  Measured worst relative error of the long rows on an
    MI355X (bound): 2049 entries 1.01e-7 (2.44e-6), 4097 1.06e-7 (2.92e-6), 21 843 1.39e-7 (7.03e-6), 65 536 1.50e-7
    (1.72e-5); the plain fp32 emulation of the summation order on the CPU stays below 2.5e-7 at each of these lengths
    (tests/test_topk_host.py)."""
    L = pkg.lib()
    data = craft(pkg, length)
    d_in = pkg.DeviceBuffer.from_numpy(data)
    row_ptr = lambda r: C.c_void_p(d_in.ptr.value + 4 * r * length)
    if length <= 2048:
        d_sm = pkg.DeviceBuffer(5 * length)
        assert L.vh_launch_softmax(None, d_in.ptr, d_sm.ptr, 5, length) == 0, L.vh_last_error().decode()
        assert L.vh_device_sync() == 0
        soft = d_sm.to_numpy((5, length))
    else:
        with np.errstate(invalid="ignore"):
            soft64 = tr.softmax64(data)
    worst = 0.0
    for k in (k for k in (1, 5, 32) if k <= length):
        want = tr.topk(data, k)
        for first, rows in ((0, 3), (2, 3), (0, 1), (4, 1)):          # rows in {1, 3}; every crafted row in both
            sel = slice(first, first + rows)
            for kind in (PROBS, LOGITS):
                labels, scores = launch_topk(pkg, row_ptr(first), rows, length, k, kind)
                assert np.array_equal(labels, want[sel]), (length, k, first, rows, kind)
                if kind == LOGITS:
                    assert same(scores, np.take_along_axis(data[sel], want[sel], axis=1))
                elif length <= 2048:
                    assert same(scores, np.take_along_axis(soft[sel], want[sel], axis=1)), (length, k, first, rows)
                else:
                    ref = np.take_along_axis(soft64[sel], want[sel], axis=1)
                    got = scores.astype(np.float64)
                    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got == 0, ref == 0)
                    ok = ~np.isnan(ref) & (ref != 0)
                    rel = float(np.abs(got[ok] / ref[ok] - 1.0).max()) if ok.any() else 0.0
                    worst = max(worst, rel)
                    assert rel <= long_row_bound(length), (length, k, rel)
            only_labels, _ = launch_topk(pkg, row_ptr(first), rows, length, k, PROBS, want_scores=False)
            assert np.array_equal(only_labels, want[sel])
        assert all(len(set(r)) == k for r in want.tolist())
    if length > 2048:
        print(f"length {length}: worst relative error of PROBS scores {worst:.3e}, bound {long_row_bound(length):.3e}")


@pytest.mark.parametrize("length,finite", [(40, 28), (300, 20), (2100, 20)])
def test_nan_ranks_last_by_ascending_index(pkg, device, length, finite):
    """all but `finite` entries are NaN (of both signs and several payloads): the finite ones come first, the NaNs after
    them in ascending index -- in the register path and in the rescan path"""
    rng = np.random.default_rng(length)
    row = np.full(length, np.nan, np.float32)
    row.view(np.uint32)[::3] = 0xFFC00001           # negative quiet NaN with a payload
    row.view(np.uint32)[1::7] = 0x7F800001          # signalling pattern
    keep = np.sort(rng.choice(length, size=finite, replace=False))
    row[keep] = rng.uniform(-4, 4, size=finite).astype(np.float32)
    row[keep[0]] = -np.inf
    d_in = pkg.DeviceBuffer.from_numpy(row)
    for k in (1, 5, 32):
        labels, _ = launch_topk(pkg, d_in.ptr, 1, length, k, LOGITS)
        want = tr.topk(row[None], k)
        assert np.array_equal(labels, want)
        if k > finite:
            nan_idx = np.flatnonzero(np.isnan(row))
            assert labels[0, finite - 1] == keep[0] and list(labels[0, finite:]) == list(nan_idx[: k - finite])


def test_launcher_refusals_leave_the_output_alone(pkg, device):
    L = pkg.lib()
    d_in = pkg.DeviceBuffer.from_numpy(np.arange(64, dtype=np.float32))
    sentinel = np.full(64, -77, np.int32)
    d_lab = pkg.DeviceBuffer.from_numpy(sentinel, np.int32)
    d_sc = pkg.DeviceBuffer.from_numpy(sentinel.astype(np.float32))
    for length, k, kind, lab in ((4, 5, PROBS, d_lab.ptr), (64, 0, PROBS, d_lab.ptr), (64, 33, LOGITS, d_lab.ptr),
                                 (65537, 5, PROBS, d_lab.ptr), (64, 5, PROBS, None), (64, 5, 2, d_lab.ptr), (0, 1, PROBS, d_lab.ptr)):
        L.vh_set_error(1, b"stale")
        assert L.vh_launch_topk(None, d_in.ptr, 1, length, k, kind, lab, d_sc.ptr) == 1, (length, k, kind)
        assert L.vh_last_error().decode().startswith("vh_launch_topk: ")
    assert L.vh_launch_topk(None, None, 1, 64, 5, PROBS, d_lab.ptr, d_sc.ptr) == 1
    assert L.vh_device_sync() == 0
    assert np.array_equal(d_lab.to_numpy(), sentinel) and np.array_equal(d_sc.to_numpy(), sentinel.astype(np.float32))
    assert L.vh_launch_topk(None, d_in.ptr, 1, 64, 5, LOGITS, d_lab.ptr, d_sc.ptr) == 0 and L.vh_device_sync() == 0
    assert list(d_lab.to_numpy()[:6]) == [63, 62, 61, 60, 59, -77]


# ---- 2. the model -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cfg(pkg):
    return pkg.preset("vit_b_16")


@pytest.fixture(scope="module")
def models(pkg, device, cfg, weights):
    """ViT-B/16, synthetic weights, max_batch 8, one context per precision, made on first use"""
    made = {}

    def get(precision="f32"):
        if precision not in made:
            made[precision] = pkg.ViTHip(cfg, weights, device=0, max_batch=8, precision=precision)
        return made[precision]

    yield get
    for m in made.values():
        m.close()


@pytest.fixture(scope="module")
def images19(pkg, cfg):
    return pkg.synth_images(cfg, 0, 19)


def plain_device(pkg, model, images):
    n, nc = images.shape[0], model.cfg.num_classes
    d_img = pkg.DeviceBuffer.from_numpy(images)
    d_l, d_p = pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)
    model.forward_device(d_img.ptr, n, d_l.ptr, d_p.ptr)
    model.sync()
    return d_l.to_numpy((n, nc)), d_p.to_numpy((n, nc))


def armed_device(pkg, model, images, k=5, scores="probs", outputs=True):
    """forward_device with the device form armed -> labels, scores, logits, probs (None, None when outputs is False)"""
    n, nc = images.shape[0], model.cfg.num_classes
    d_img = pkg.DeviceBuffer.from_numpy(images)
    d_lab, d_sc = pkg.DeviceBuffer(model.max_batch * k, np.int32), pkg.DeviceBuffer(model.max_batch * k)
    d_l, d_p = (pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)) if outputs else (None, None)
    model.set_topk(pkg.binding.TopKSpec(k, scores), labels=d_lab, scores=d_sc)
    try:
        model.forward_device(d_img.ptr, n, d_l.ptr if outputs else None, d_p.ptr if outputs else None)
        model.sync()
    finally:
        model.set_topk(None)
    out = d_lab.to_numpy()[: n * k].reshape(n, k), d_sc.to_numpy()[: n * k].reshape(n, k)
    return out + ((d_l.to_numpy((n, nc)), d_p.to_numpy((n, nc))) if outputs else (None, None))


@pytest.mark.parametrize("precision", ["f32", "bf16", "fp8", "f32_fp16x2"])
def test_model_topk_in_every_precision(pkg, models, images19, precision):
    model = models(precision)
    imgs = images19[:5]
    l0, p0 = plain_device(pkg, model, imgs)
    labels, scores, logits, probs = armed_device(pkg, model, imgs)
    assert same(logits, l0) and same(probs, p0)
    assert np.array_equal(labels, tr.topk(logits, 5))
    assert same(scores, np.take_along_axis(probs, labels, axis=1))
    _, lscores, _, _ = armed_device(pkg, model, imgs, scores="logits")
    assert same(lscores, np.take_along_axis(logits, labels, axis=1))
    if precision == "f32":     # no outputs asked for: the context's own logits scratch
        labels2, scores2, _, _ = armed_device(pkg, model, imgs, outputs=False)
        assert np.array_equal(labels2, labels) and same(scores2, scores)


def test_host_form_equals_device_form(pkg, models, images19):
    model = models("f32")
    dev = [armed_device(pkg, model, images19[a:a + 8], outputs=False)[:2] for a in (0, 8, 16)]
    want_l, want_s = np.concatenate([d[0] for d in dev]), np.concatenate([d[1] for d in dev])
    labels, scores = model.classify(images19, k=5, scores="probs")      # three chunks of max_batch = 8, the last one ragged
    assert labels.dtype == np.int32 and np.array_equal(labels, want_l) and same(scores, want_s)
    # labels alone, and next to logits and probabilities that are asked for
    lab_only = np.full((19, 5), -1, np.int32)
    model.set_topk_host(pkg.binding.TopKSpec(5, "logits"), labels=lab_only)
    try:
        hl, hp = model.forward(images19)
    finally:
        model.set_topk_host(None)
    assert np.array_equal(lab_only, want_l) and np.array_equal(lab_only, tr.topk(hl, 5))
    assert same(np.take_along_axis(hp, lab_only, axis=1), want_s)
    hl0, hp0 = model.forward(images19)
    assert same(hl, hl0) and same(hp, hp0)


def test_position_independence(pkg, models, images19):
    model = models("f32")
    a = armed_device(pkg, model, images19[:5], outputs=False)
    perm = np.array([4, 1, 2, 3, 0])                                   # image 0 at position 4, image 4 at position 0
    p = armed_device(pkg, model, images19[:5][perm], outputs=False)
    assert np.array_equal(p[0], a[0][perm]) and same(p[1], a[1][perm])


def test_u8_entry_points_with_features_armed_too(pkg, models, cfg):
    model, b = models("f32"), pkg.binding
    n, S, E, k = 3, cfg.img_size, cfg.embed_dim, 5
    rng = np.random.default_rng(3)
    norm = pkg.pixel_norm(MEAN, STD)
    u8 = rng.integers(0, 256, size=(n, S, S, 3), dtype=np.uint8)
    sources = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in ((300, 260), (224, 224), (257, 401))]
    fspec, tspec = b.FeatureSpec(taps=(-1,)), b.TopKSpec(k, "probs")

    def device(call):
        d_lab, d_sc, d_cls = pkg.DeviceBuffer(8 * k, np.int32), pkg.DeviceBuffer(8 * k), pkg.DeviceBuffer(8 * E)
        model.set_topk(tspec, labels=d_lab, scores=d_sc)
        model.set_features(fspec, cls=d_cls)
        try:
            call()
            model.sync()
        finally:
            model.set_topk(None)
            model.set_features(None)
        return d_lab.to_numpy()[: n * k].reshape(n, k), d_sc.to_numpy()[: n * k].reshape(n, k), d_cls.to_numpy()[: n * E].reshape(n, E)

    def host(call):
        labels, scores, cls = np.empty((n, k), np.int32), np.empty((n, k), np.float32), np.empty((n, E), np.float32)
        model.set_topk_host(tspec, labels=labels, scores=scores)
        model.set_features_host(fspec, cls=cls)
        try:
            call()
        finally:
            model.set_topk_host(None)
            model.set_features_host(None)
        return labels, scores, cls

    d_u8 = pkg.DeviceBuffer.from_numpy(u8, dtype=np.uint8)
    d_src = [pkg.DeviceBuffer.from_numpy(a, dtype=np.uint8) for a in sources]
    descs = [(d.ptr.value, a.shape[0], a.shape[1], a.shape[1] * 3) for d, a in zip(d_src, sources)]
    pairs = ((device(lambda: model.forward_device_u8(d_u8.ptr, n, norm, "hwc")),
              host(lambda: model.forward_u8(u8, norm, None, logits=False, probs=False))),
             (device(lambda: model.forward_device_u8_resized(descs, 256, norm)),
              host(lambda: model.forward_u8_resized(sources, 256, "bilinear", norm, logits=False, probs=False))))
    for dev, hst in pairs:
        assert np.array_equal(dev[0], hst[0]) and same(dev[1], hst[1]) and same(dev[2], hst[2])
        assert np.abs(dev[2]).max() > 0 and (dev[1] > 0).all() and all(len(set(r)) == k for r in dev[0].tolist())


def test_every_staged_array_over_three_ragged_chunks(pkg, device):
    """Logits, probabilities, cls, pooled, labels and scores of the host forms at once, on the 17-token config of
    tests/test_gpu_configs.py with max_batch 2 and 5 images: chunks of 2, 2 and 1, the third in the first one's pinned slot.
    Every array has the bits of the device forms armed the same way on images [0:2], [2:4], [4:5]; again with bf16 features
    (2-byte elements), with labels only, and with neither logits nor probabilities; then a re-arm of the top-k request
    without a disarm (new stages), and the plain forward once both are disarmed."""
    b, L = pkg.binding, pkg.lib()
    cfg = pkg.preset("vit_b_16")
    cfg.img_size, cfg.patch_size, cfg.in_chans, cfg.num_classes = 64, 16, 3, 10
    cfg.embed_dim, cfg.depth, cfg.num_heads, cfg.mlp_hidden = 256, 2, 4, 512
    n, nc, mb = 5, 10, 2
    imgs = pkg.synth_images(cfg, 0, n)
    model = pkg.ViTHip(cfg, pkg.synth_weights(cfg, 21), device=0, max_batch=mb)

    def device_form(fspec, k):
        """-> logits, probs, cls, pooled, labels, scores of the chunks, concatenated"""
        c_el, p_el, _ = b.feature_sizes(cfg, fspec)
        d_cls, d_pool = pkg.DeviceBuffer(mb * c_el, dtype=fspec.np_dtype), pkg.DeviceBuffer(mb * p_el, dtype=fspec.np_dtype)
        d_lab, d_sc = pkg.DeviceBuffer(mb * k, np.int32), pkg.DeviceBuffer(mb * k)
        d_l, d_p = pkg.DeviceBuffer(mb * nc), pkg.DeviceBuffer(mb * nc)
        model.set_features(fspec, cls=d_cls, pooled=d_pool)
        model.set_topk(b.TopKSpec(k, "probs"), labels=d_lab, scores=d_sc)
        chunks = []
        try:
            for first in range(0, n, mb):
                m = min(mb, n - first)
                d_img = pkg.DeviceBuffer.from_numpy(imgs[first:first + m])
                model.forward_device(d_img.ptr, m, d_l.ptr, d_p.ptr)
                model.sync()
                chunks.append([d.to_numpy()[: m * per].reshape(m, per) for d, per in
                               ((d_l, nc), (d_p, nc), (d_cls, c_el), (d_pool, p_el), (d_lab, k), (d_sc, k))])
        finally:
            model.set_features(None)
            model.set_topk(None)
        return [np.concatenate(parts) for parts in zip(*chunks)]

    def host_arrays(fspec, k, scores=True):
        c_el, p_el, _ = b.feature_sizes(cfg, fspec)
        return (np.zeros((n, c_el), fspec.np_dtype), np.zeros((n, p_el), fspec.np_dtype), np.full((n, k), -1, np.int32),
                np.full((n, k), -1.0, np.float32) if scores else None)

    def host_form(fspec, k, scores=True, outputs=True):
        """-> the same six of one host forward; None for what was not asked for"""
        cls, pooled, labels, sc = host_arrays(fspec, k, scores)
        model.set_features_host(fspec, cls=cls, pooled=pooled)
        model.set_topk_host(b.TopKSpec(k, "probs"), labels=labels, scores=sc)
        try:
            if outputs:
                logits, probs = model.forward(imgs)
            else:
                b.check(L.vit_hip_forward(model.ctx, b.image_array(imgs), n, None, None), "vit_hip_forward")
                logits = probs = None
        finally:
            model.set_features_host(None)
            model.set_topk_host(None)
        return [logits, probs, cls, pooled, labels, sc]

    try:
        l0, p0 = model.forward(imgs)
        f32, bf16 = b.FeatureSpec(taps=(0, -1)), b.FeatureSpec(taps=(0, -1), dtype="bf16")
        want = device_form(f32, 3)
        assert same(want[0], l0) and same(want[1], p0) and np.abs(want[2]).max() > 0 and np.abs(want[3]).max() > 0
        assert np.array_equal(want[4], tr.topk(l0, 3)) and same(want[5], np.take_along_axis(p0, want[4], axis=1))
        got = host_form(f32, 3)
        assert all(same(g, w) for g, w in zip(got, want))
        want16 = device_form(bf16, 3)
        assert want16[2].dtype == np.uint16 and want16[2].any() and want16[3].any()
        got = host_form(bf16, 3)
        assert all(same(g, w) for g, w in zip(got, want16))
        got = host_form(f32, 3, scores=False)
        assert got[5] is None and all(same(g, w) for g, w in zip(got[:5], want[:5]))
        got = host_form(f32, 3, outputs=False)
        assert got[0] is None and got[1] is None and all(same(g, w) for g, w in zip(got[2:], want[2:]))
        # k = 5 over the armed k = 3, no disarm between: the stages are made anew
        want5 = device_form(f32, 5)
        cls, pooled, labels, sc = host_arrays(f32, 3)
        model.set_features_host(f32, cls=cls, pooled=pooled)
        model.set_topk_host(b.TopKSpec(3, "probs"), labels=labels, scores=sc)
        labels5, sc5 = host_arrays(f32, 5)[2:]
        model.set_topk_host(b.TopKSpec(5, "probs"), labels=labels5, scores=sc5)
        got = list(model.forward(imgs)) + [cls, pooled, labels5, sc5]
        assert all(same(g, w) for g, w in zip(got, want5)) and (labels == -1).all() and (sc == -1.0).all()
        model.set_features_host(None)
        model.set_topk_host(None)
        l1, p1 = model.forward(imgs)
        assert same(l1, l0) and same(p1, p0)
    finally:
        model.close()


def test_arming_rules_and_launch_counts(pkg, models, images19):
    model, b, L = models("f32"), pkg.binding, pkg.lib()
    n, nc, k = 5, 1000, 5
    imgs = images19[:n]
    d_img, d_l, d_p = pkg.DeviceBuffer.from_numpy(imgs), pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)
    d_lab, d_sc = pkg.DeviceBuffer(8 * k, np.int32), pkg.DeviceBuffer(8 * k)
    h_lab = np.empty((n, k), np.int32)
    l0, p0 = plain_device(pkg, model, imgs)

    def counts():
        model.profile_enable(1)
        model.forward_device(d_img.ptr, n, d_l.ptr, d_p.ptr)
        got = {name: c for name, (_, c) in model.profile_read().items()}
        model.profile_enable(0)
        return got

    unarmed = counts()
    model.set_topk(b.TopKSpec(k), labels=d_lab, scores=d_sc)
    armed = counts()
    assert armed["softmax"] == unarmed["softmax"] + 1 and all(armed[o] == unarmed[o] for o in armed if o != "softmax")
    want = d_lab.to_numpy()[: n * k].copy()
    assert np.array_equal(want.reshape(n, k), tr.topk(l0, k))
    # device form armed: the host forms refuse
    with pytest.raises(b.VitHipError, match="vit_hip_set_topk"):
        model.forward(imgs)
    # refused re-arms (k out of range, no labels, a misaligned buffer) keep the old request
    bad = b.TopKSpecC(33, 0)
    bufs = b.TopKBuffers(d_lab.ptr, d_sc.ptr)
    assert L.vit_hip_set_topk(model.ctx, C.byref(bad), C.byref(bufs)) == 1
    ok = b.TopKSpecC(3, 0)
    assert L.vit_hip_set_topk(model.ctx, C.byref(ok), C.byref(b.TopKBuffers(None, d_sc.ptr))) == 1
    assert L.vit_hip_set_topk(model.ctx, C.byref(ok), C.byref(b.TopKBuffers(d_lab.ptr.value + 4, None))) == 1
    assert L.vit_hip_set_topk(model.ctx, C.byref(ok), None) == 1
    assert L.vit_hip_set_topk_host(model.ctx, C.byref(bad), C.byref(b.TopKBuffers(h_lab.ctypes.data, None))) == 1
    assert L.vh_h2d(d_lab.ptr, np.full(8 * k, -1, np.int32).ctypes.data_as(C.c_void_p), 8 * k * 4, None) == 0
    model.forward_device(d_img.ptr, n, d_l.ptr, d_p.ptr)
    model.sync()
    assert np.array_equal(d_lab.to_numpy()[: n * k], want) and (d_lab.to_numpy()[n * k:] == -1).all()
    # host form armed (which disarms the device form): the device forms refuse, nothing is launched
    model.set_topk_host(b.TopKSpec(k), labels=h_lab)
    sentinel = np.full(n * nc, -7.0, np.float32)
    assert L.vh_h2d(d_l.ptr, sentinel.ctypes.data_as(C.c_void_p), sentinel.nbytes, None) == 0
    assert L.vit_hip_forward_device(model.ctx, d_img.ptr, n, d_l.ptr, None, None) == 1
    assert "vit_hip_set_topk_host" in L.vh_last_error().decode()
    model.sync()
    assert np.array_equal(d_l.to_numpy(), sentinel)
    hl, _ = model.forward(imgs)
    assert same(hl, l0) and np.array_equal(h_lab.ravel(), want)
    # disarmed: today's launches, today's outputs, nothing written into the old buffers
    model.set_topk_host(None)
    assert L.vh_h2d(d_lab.ptr, np.full(8 * k, -1, np.int32).ctypes.data_as(C.c_void_p), 8 * k * 4, None) == 0
    assert counts() == unarmed
    assert same(d_l.to_numpy((n, nc)), l0) and same(d_p.to_numpy((n, nc)), p0) and (d_lab.to_numpy() == -1).all()


def test_label_space_beyond_the_softmax_limit(pkg, device):
    """the tiny 17-token, depth-1 config of tests/test_gpu_configs.py with 2500 classes: the full probabilities output is
    refused as before, top-k reads the head"""
    b, L = pkg.binding, pkg.lib()
    cfg = pkg.preset("vit_b_16")
    cfg.img_size, cfg.patch_size, cfg.in_chans, cfg.num_classes = 64, 16, 3, 2500
    cfg.embed_dim, cfg.depth, cfg.num_heads, cfg.mlp_hidden = 256, 1, 2, 768
    n, nc, k = 5, 2500, 5
    model = pkg.ViTHip(cfg, pkg.synth_weights(cfg, 21), device=0, max_batch=n)
    try:
        imgs = pkg.synth_images(cfg, 0, n)
        d_img, d_l, d_p = pkg.DeviceBuffer.from_numpy(imgs), pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)
        d_lab, d_sc = pkg.DeviceBuffer(n * k, np.int32), pkg.DeviceBuffer(n * k)
        model.set_topk(b.TopKSpec(k, "probs"), labels=d_lab, scores=d_sc)
        model.forward_device(d_img.ptr, n, d_l.ptr, None)
        model.sync()
        logits, labels, scores = d_l.to_numpy((n, nc)), d_lab.to_numpy((n, k)), d_sc.to_numpy((n, k))
        assert np.isfinite(logits).all() and np.array_equal(labels, tr.topk(logits, k))
        ref = np.take_along_axis(tr.softmax64(logits), labels, axis=1)
        rel = float(np.abs(scores.astype(np.float64) / ref - 1.0).max())
        print(f"2500 classes: worst relative error of the top-5 probabilities {rel:.3e}, bound {long_row_bound(nc):.3e}")
        assert rel <= long_row_bound(nc)
        assert L.vit_hip_forward_device(model.ctx, d_img.ptr, n, d_l.ptr, d_p.ptr, None) == 1
        assert "vh_launch_softmax" in L.vh_last_error().decode()
        model.sync()
        hl, hs = model.classify(imgs, k=k)
        assert np.array_equal(hl, labels) and same(hs, scores)
    finally:
        model.close()
