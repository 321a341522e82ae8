"""Class-token attention maps (vh_launch_cls_attention, csrc/attn_map.hip; vit_hip_set_attention / _host): the launcher
against the float64 statement of the definition (tests/attn_ref.py) in the three stored forms of Q|K|V, the derived
output's exact bits, and the model-level guarantees the header states -- nothing else moves, every precision mode and
plan, both forms, every entry point, batch-position independence, arming rules, the long-sequence plan.

Tolerances.  The launcher's is derived (attn_ref.bound) and holds the model's maps too whenever the reference is given
the Q|K|V the context itself holds.  Against the ORACLE's Q|K|V (fp32, its own summation order through the layers in
front of the tap) nothing can be derived: MODEL_TOL is 8 x the largest |p - oracle| measured on an MI355X, the margin
that separates the parity test's 1e-4 from its measured 6.3e-6.  Measured values are beside the constants."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import attn_ref as ar
import topk_ref as tr

pytestmark = pytest.mark.gpu

ENV = ("VIT_HIP_P3", "VIT_HIP_GEMM_FP32", "VIT_HIP_ATTN", "VIT_HIP_LN_FOLD", "VIT_HIP_LAST_LAYER", "VIT_HIP_PRECISION")
FORMS = (ar.ROWS_F32, ar.PLANES3, ar.PLANES_F16)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

# Largest |p - oracle| over the taps of image 0, measured on an MI355X (the first run of these tests; per tap below), and
# the constants at 8 x that.  Synthetic weights make near-uniform maps (p ~ 1/197 = 5e-3), so these are 5e-7, 1e-3 and
# 1.5e-2 of a typical p.
#   f32   taps (0, 2, 11): 1.658e-09, 1.982e-09, 2.683e-09   (mean: 9.4e-10, 9.5e-10, 8.7e-10)
#   bf16  taps (2, 11):    4.347e-06, 5.836e-06               (mean: 1.1e-06, 1.5e-06)
#   fp8   taps (2, 11):    7.256e-05, 7.790e-05               (mean: 1.9e-05, 2.1e-05)
# The f32 plans of test_plans measured 2.2e-09 .. 3.2e-09 at tap 11 of images 0 and 1 (VIT_HIP_P3=0 3.165e-09,
# VIT_HIP_ATTN=long 2.264e-09, tiled with P3=0 2.393e-09, class-only last layer 2.700e-09).
MODEL_TOL = {"f32": 8 * 2.683e-09, "bf16": 8 * 5.836e-06, "fp8": 8 * 7.790e-05}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def within_bound(got, ref, bnd):
    return bool((np.abs(got.astype(np.float64) - ref) <= bnd * ref + 1e-30).all())


# ---- 1-3. the launcher --------------------------------------------------------------------------------------------------

CASES = [(1, 1, 64, 1), (1, 2, 128, 2), (3, 50, 768, 12), (2, 197, 768, 12), (2, 257, 1280, 16), (1, 255, 256, 2),
         (1, 256, 256, 2), (1, 257, 256, 2), (1, 577, 768, 12), (1, 1370, 1280, 16)]
FILL = np.float32(-77.0)


def stored(pkg, form, qkv):
    """-> (device buffer of qkv in `form`, the fp32 values that buffer decodes to)"""
    if form == ar.ROWS_F32:
        return pkg.DeviceBuffer.from_numpy(qkv), qkv
    if form == ar.PLANES_F16:
        planes = ar.encode_f16(qkv)
        return ar.upload(pkg, planes), ar.decode_f16(planes)
    d_pl, planes = ar.split3_on_device(pkg, qkv)
    assert np.array_equal(ar.decode_planes3(planes), qkv)          # exact: the reference gets the original fp32
    return d_pl, qkv


def launch(pkg, d_qkv, form, n, T, E, H, heads=True, mean=True, tap=0, n_taps=1):
    """-> heads [n][n_taps][H][T], mean [n][n_taps][T] (None where not asked for); untouched elements keep FILL"""
    L = pkg.lib()
    d_h = pkg.DeviceBuffer.from_numpy(np.full(n * n_taps * H * T, FILL)) if heads else None
    d_m = pkg.DeviceBuffer.from_numpy(np.full(n * n_taps * T, FILL)) if mean else None
    rc = L.vh_launch_cls_attention(None, d_qkv.ptr, form, n, T, E, H, tap, n_taps, d_h.ptr if heads else None, d_m.ptr if mean else None)
    assert rc == 0, L.vh_last_error().decode()
    assert L.vh_device_sync() == 0, L.vh_last_error().decode()
    return (d_h.to_numpy((n, n_taps, H, T)) if heads else None), (d_m.to_numpy((n, n_taps, T)) if mean else None)


def mean_of(heads):
    """the fp32 ascending-h sum of heads [..][H][T] divided by float32(H)"""
    acc = heads[..., 0, :].copy()
    for h in range(1, heads.shape[-2]):
        acc = (acc + heads[..., h, :]).astype(np.float32)
    return (acc / np.float32(heads.shape[-2])).astype(np.float32)


@pytest.mark.parametrize("n,T,E,H", CASES)
def test_launcher_vs_reference_and_derived_output(pkg, device, n, T, E, H):
    """All three forms at amplitudes 1 and 3: every p within attn_ref.bound of the float64 definition on the values the
    buffer holds, rows summing to 1; mean the exact fp32 function of heads, and the same bits when asked for alone; tap 1
    of 3 leaves the other taps' slots alone.  Measured worst |p - ref| / bound on an MI355X: 0.0014 - 0.0072 over these
    cases (the largest at T = 577, three-part planes, amplitude 3); an fp32 emulation on the CPU stays below 0.012."""
    D = E // H
    rng = np.random.default_rng(1000 * T + E)
    base = rng.standard_normal((n * T, 3 * E)).astype(np.float32)
    worst = 0.0
    for amp in (1.0, 3.0):
        qkv = (np.float32(amp) * base).astype(np.float32)
        for form in FORMS:
            d_qkv, values = stored(pkg, form, qkv)
            ref, _ = ar.cls_attention(values, n, T, H)
            bnd = ar.bound(values, n, T, H)
            heads, mean = launch(pkg, d_qkv, form, n, T, E, H)
            got = heads[:, 0].astype(np.float64)
            rel = float((np.abs(got - ref) / (bnd * ref + 1e-30)).max())
            worst = max(worst, rel)
            print(f"(n={n}, T={T}, E={E}, H={H}) form {form} amplitude {amp}: worst |p - ref| / bound = {rel:.4f}")
            assert within_bound(heads[:, 0], ref, bnd), (form, amp, rel)
            if D == 80:          # a head whose columns start mid-chunk in the planes forms
                assert within_bound(heads[:, 0, 1:2], ref[:, 1:2], bnd[:, 1:2]) and within_bound(heads[:, 0, 15:], ref[:, 15:], bnd[:, 15:])
            assert np.abs(got.sum(axis=2) - 1.0).max() <= (T + 64) * 2.0 ** -24
            assert same(mean, mean_of(heads)), (form, amp)
            none, alone = launch(pkg, d_qkv, form, n, T, E, H, heads=False)
            assert none is None and same(alone, mean), (form, amp)
            only, none = launch(pkg, d_qkv, form, n, T, E, H, mean=False)
            assert none is None and same(only, heads)
            if amp == 3.0:
                h3, m3 = launch(pkg, d_qkv, form, n, T, E, H, tap=1, n_taps=3)
                assert same(h3[:, 1], heads[:, 0]) and same(m3[:, 1], mean[:, 0])
                assert (h3[:, [0, 2]] == FILL).all() and (m3[:, [0, 2]] == FILL).all()
                _, m3 = launch(pkg, d_qkv, form, n, T, E, H, heads=False, tap=1, n_taps=3)
                assert same(m3[:, 1], mean[:, 0]) and (m3[:, [0, 2]] == FILL).all()
    assert worst <= 1.0


def test_launcher_refusals(pkg, device):
    L = pkg.lib()
    n, T, E, H = 1, 10, 128, 2
    qkv = np.random.default_rng(5).standard_normal((n * T, 3 * E)).astype(np.float32)
    d_qkv = pkg.DeviceBuffer.from_numpy(np.concatenate([qkv.ravel(), np.zeros(3 * 288 * T, np.float32)]))
    d_h, d_m = pkg.DeviceBuffer.from_numpy(np.full(H * T + 4, FILL)), pkg.DeviceBuffer.from_numpy(np.full(T + 4, FILL))
    off = lambda d: C.c_void_p(d.ptr.value + 4)
    for args in ((d_qkv.ptr, 0, n, T, 48, 2, 0, 1, d_h.ptr, d_m.ptr),         # head_dim 24
                 (d_qkv.ptr, 0, n, T, 288, 2, 0, 1, d_h.ptr, d_m.ptr),        # head_dim 144
                 (d_qkv.ptr, 0, n, T, E, H, 0, 1, None, None),                # both NULL
                 (off(d_qkv), 0, n, T, E, H, 0, 1, d_h.ptr, d_m.ptr),         # misaligned
                 (d_qkv.ptr, 0, n, T, E, H, 0, 1, off(d_h), d_m.ptr),
                 (d_qkv.ptr, 0, n, T, E, H, 0, 1, d_h.ptr, off(d_m)),
                 (d_qkv.ptr, 0, n, T, E, H, 1, 1, d_h.ptr, d_m.ptr),          # tap_index >= n_taps
                 (d_qkv.ptr, 0, n, T, E, H, 0, 5, d_h.ptr, d_m.ptr),
                 (d_qkv.ptr, 0, n, T, E, H, -1, 1, d_h.ptr, d_m.ptr),
                 (d_qkv.ptr, 3, n, T, E, H, 0, 1, d_h.ptr, d_m.ptr),          # unknown form
                 (d_qkv.ptr, 1, n, T, 80, 1, 0, 1, d_h.ptr, d_m.ptr),         # planes need embed_dim % 32 == 0
                 (d_qkv.ptr, 0, n, 0, E, H, 0, 1, d_h.ptr, d_m.ptr),          # no tokens
                 (None, 0, n, T, E, H, 0, 1, d_h.ptr, d_m.ptr)):
        L.vh_set_error(1, b"stale")
        assert L.vh_launch_cls_attention(None, *args) == 1, args[1:8]
        assert L.vh_last_error().decode().startswith("vh_launch_cls_attention: "), args[1:8]
    assert L.vh_device_sync() == 0
    assert (d_h.to_numpy() == FILL).all() and (d_m.to_numpy() == FILL).all()
    assert L.vh_launch_cls_attention(None, d_qkv.ptr, 0, n, T, E, H, 0, 1, d_h.ptr, d_m.ptr) == 0 and L.vh_device_sync() == 0
    ref, _ = ar.cls_attention(qkv, n, T, H)
    assert within_bound(d_h.to_numpy()[:H * T].reshape(n, H, T), ref, ar.bound(qkv, n, T, H))
    assert (d_h.to_numpy()[H * T:] == FILL).all() and (d_m.to_numpy()[T:] == FILL).all()


# ---- 4-9. the model ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cfg(pkg):
    return pkg.preset("vit_b_16")


@pytest.fixture(scope="module")
def models(pkg, device, cfg, weights):
    """ViT-B/16, synthetic weights, max_batch 8, one context per precision, made on first use (default plan)"""
    made = {}

    def get(precision="f32"):
        if precision not in made:
            made[precision] = pkg.ViTHip(cfg, weights, device=0, max_batch=8, precision=precision)
        return made[precision]

    yield get
    for m in made.values():
        m.close()


@pytest.fixture(scope="module")
def images11(pkg, cfg):
    return pkg.synth_images(cfg, 0, 11)


@pytest.fixture(scope="module")
def oracle_qkv(oracle, weights, images11):
    """(image index, layer) -> the oracle's Q|K|V of that layer, fp32 [T][3E]; computed once per pair"""
    made = {}

    def one(key):
        i, l = key
        lw = weights[4 + 12 * l: 4 + 12 * (l + 1)]
        x = oracle.forward(images11[i], weights, stop_after_layers=l)[2]
        return oracle.linear(oracle.layer_norm(x, lw[0], lw[1]), lw[2], lw[3], 3 * oracle.cfg.embed_dim)

    def get(*keys):
        todo = [k for k in keys if k not in made]
        with ThreadPoolExecutor(max(1, min(4, len(todo)))) as ex:
            for k, v in zip(todo, ex.map(one, todo)):
                made[k] = v
        return [made[k] for k in keys]

    return get


def plain_device(pkg, model, images):
    n, nc = images.shape[0], model.cfg.num_classes
    d_img, d_l, d_p = pkg.DeviceBuffer.from_numpy(images), pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)
    model.forward_device(d_img.ptr, n, d_l.ptr, d_p.ptr)
    model.sync()
    return d_l.to_numpy((n, nc)), d_p.to_numpy((n, nc))


def attn_buffers(pkg, model, taps):
    H, T, mb = model.cfg.num_heads, model.tokens, model.max_batch
    return pkg.DeviceBuffer(mb * len(taps) * H * T), pkg.DeviceBuffer(mb * len(taps) * T)


def read_attn(model, d_h, d_m, n, taps):
    H, T, k = model.cfg.num_heads, model.tokens, len(taps)
    return d_h.to_numpy()[: n * k * H * T].reshape(n, k, H, T), d_m.to_numpy()[: n * k * T].reshape(n, k, T)


def armed_device(pkg, model, images, taps=(-1,), call=None):
    """a device-form forward with attention armed -> heads, mean, logits, probs"""
    n, nc = images.shape[0] if call is None else call[1], model.cfg.num_classes
    d_h, d_m = attn_buffers(pkg, model, taps)
    d_l, d_p = pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)
    model.set_attention(pkg.binding.AttentionSpec(taps), heads=d_h, mean=d_m)
    try:
        if call is None:
            d_img = pkg.DeviceBuffer.from_numpy(images)
            model.forward_device(d_img.ptr, n, d_l.ptr, d_p.ptr)
        else:
            call[0](d_l, d_p)
        model.sync()
    finally:
        model.set_attention(None)
    return read_attn(model, d_h, d_m, n, taps) + (d_l.to_numpy((n, nc)), d_p.to_numpy((n, nc)))


@pytest.mark.parametrize("precision", ["f32", "bf16", "fp8", "f32_fp16x2"])
def test_nothing_else_moves(pkg, models, images11, precision):
    model, b = models(precision), pkg.binding
    imgs, n, k, E = images11[:5], 5, 5, model.cfg.embed_dim
    taps = (0, 5, -1)
    l0, p0 = plain_device(pkg, model, imgs)

    def counts():
        d_img = pkg.DeviceBuffer.from_numpy(imgs)
        model.profile_enable(1)
        model.forward_device(d_img.ptr, n, None, None)
        got = {name: c for name, (_, c) in model.profile_read().items()}
        model.profile_enable(0)
        return got

    before = counts()
    heads, mean, l1, p1 = armed_device(pkg, model, imgs, taps)
    assert same(l1, l0) and same(p1, p0)
    assert np.abs(heads.astype(np.float64).sum(axis=3) - 1.0).max() <= (model.tokens + 64) * 2.0 ** -24
    assert same(mean, mean_of(heads)) and not same(heads[:, 0], heads[:, 2])
    # the host form: logits, probabilities and maps
    hl, hh, hm = model.attention(imgs, taps)
    assert same(hl, l0) and same(hh, heads) and same(hm, mean)
    assert same(model.forward(imgs)[1], p0)
    # all three requests armed at once: every output as when armed alone
    fspec, tspec = b.FeatureSpec(taps=(3, -1)), b.TopKSpec(k, "probs")
    d_cls, d_pool = pkg.DeviceBuffer(8 * 2 * E), pkg.DeviceBuffer(8 * 2 * E)
    d_lab, d_sc = pkg.DeviceBuffer(8 * k, np.int32), pkg.DeviceBuffer(8 * k)
    d_img = pkg.DeviceBuffer.from_numpy(imgs)
    model.set_features(fspec, cls=d_cls, pooled=d_pool)
    model.forward_device(d_img.ptr, n)
    model.sync()
    model.set_features(None)
    cls, pooled = d_cls.to_numpy()[: n * 2 * E].copy(), d_pool.to_numpy()[: n * 2 * E].copy()
    model.set_topk(tspec, labels=d_lab, scores=d_sc)
    model.forward_device(d_img.ptr, n)
    model.sync()
    model.set_topk(None)
    labels, scores = d_lab.to_numpy()[: n * k].copy(), d_sc.to_numpy()[: n * k].copy()
    assert np.array_equal(labels.reshape(n, k), tr.topk(l0, k))
    for d in (d_cls, d_pool, d_sc):
        assert pkg.lib().vh_memset(d.ptr, 0, d.count * 4, None) == 0
    model.set_features(fspec, cls=d_cls, pooled=d_pool)
    model.set_topk(tspec, labels=d_lab, scores=d_sc)
    try:
        armed = counts()
        h3, m3, l3, p3 = armed_device(pkg, model, imgs, taps)
    finally:
        model.set_features(None)
        model.set_topk(None)
    assert same(h3, heads) and same(m3, mean) and same(l3, l0) and same(p3, p0)
    assert same(d_cls.to_numpy()[: n * 2 * E], cls) and same(d_pool.to_numpy()[: n * 2 * E], pooled)
    assert np.array_equal(d_lab.to_numpy()[: n * k], labels) and same(d_sc.to_numpy()[: n * k], scores)
    assert armed["layer_norm"] == before["layer_norm"] + 2 and armed["softmax"] == before["softmax"] + 1
    # armed: two launches per tap (heads, then mean), counted as one timed operator each; disarmed: today's launches
    model.set_attention(b.AttentionSpec(taps), heads=attn_buffers(pkg, model, taps)[0])
    with_attn = counts()
    model.set_attention(None)
    assert with_attn["attention"] == before["attention"] + len(taps)
    assert all(with_attn[o] == before[o] for o in before if o != "attention")
    assert counts() == before


def check_against_oracle(tag, heads, mean, qkvs, H, tol):
    """heads [n][taps][H][T] against attn_ref on the oracle's Q|K|V, qkvs[i][k]; prints the largest |p - oracle| per tap"""
    for i, per_tap in enumerate(qkvs):
        for k, qkv in enumerate(per_tap):
            T = qkv.shape[0]
            ref, ref_mean = ar.cls_attention(qkv, 1, T, H)
            diff = float(np.abs(heads[i, k].astype(np.float64) - ref[0]).max())
            dmean = float(np.abs(mean[i, k].astype(np.float64) - ref_mean[0]).max())
            print(f"{tag}: image {i} tap {k}: max |p - oracle| = {diff:.3e}, mean {dmean:.3e}")
            assert diff <= tol and dmean <= tol, (tag, i, k, diff, dmean)
            # wherever the oracle's two largest probabilities are further apart than twice the tolerance, its arg-max key
            top2 = np.sort(ref[0], axis=1)[:, -2:]
            clear = (top2[:, 1] - top2[:, 0]) > 2 * tol
            assert np.array_equal(heads[i, k].argmax(axis=1)[clear], ref[0].argmax(axis=1)[clear]), (tag, i, k)


@pytest.mark.parametrize("precision,taps", [("f32", (0, 2, 11)), ("bf16", (2, 11)), ("fp8", (2, 11))])
def test_model_maps_vs_oracle(pkg, models, images11, oracle_qkv, precision, taps):
    """One image; the reference is attn_ref on the oracle's own Q|K|V of the tapped layers (fp32 throughout), so the
    difference holds everything the mode does in front of the tap."""
    model = models(precision)
    heads, mean, _, _ = armed_device(pkg, model, images11[:1], taps)
    qkvs = [oracle_qkv(*[(0, l) for l in taps])]
    check_against_oracle(precision, heads, mean, qkvs, model.cfg.num_heads, MODEL_TOL[precision])


@pytest.mark.parametrize("plan", ["p3_off", "attn_long", "tiled_p3_off", "cls_only"])
def test_plans(pkg, device, cfg, weights, models, images11, oracle_qkv, monkeypatch, plan):
    """Two images, tap (-1,): the device-form maps of every plan a context can be created in meet the f32 constant."""
    env = {"p3_off": {"VIT_HIP_P3": "0"}, "attn_long": {"VIT_HIP_ATTN": "long"},
           "tiled_p3_off": {"VIT_HIP_ATTN": "tiled", "VIT_HIP_P3": "0"}, "cls_only": {}}[plan]
    for var, value in env.items():
        monkeypatch.setenv(var, value)
    model = pkg.ViTHip(cfg, weights, device=0, max_batch=2) if env else models("f32")
    imgs = images11[:2]
    try:
        if plan == "cls_only":
            assert model.set_last_layer_cls_only(True) is False
        l0, p0 = plain_device(pkg, model, imgs)
        heads, mean, l1, p1 = armed_device(pkg, model, imgs, (-1,))
        assert same(l1, l0) and same(p1, p0)
        if plan == "cls_only":
            model.set_last_layer_cls_only(False)
            l2, _ = plain_device(pkg, model, imgs)
            h2, m2, _, _ = armed_device(pkg, model, imgs, (-1,))
            assert same(l2, l0) and same(h2, heads) and same(m2, mean)
        qkvs = [[q] for q in oracle_qkv((0, 11), (1, 11))]
        check_against_oracle(plan, heads, mean, qkvs, cfg.num_heads, MODEL_TOL["f32"])
    finally:
        if env:
            model.close()
        else:
            model.set_last_layer_cls_only(False)


def test_batch_position_independence(pkg, models, images11):
    model = models("f32")
    order = np.array([0, 1, 2, 4, 5, 3, 6, 7])                       # image 3 at position 5 of 8
    h8, m8, _, _ = armed_device(pkg, model, images11[order], (4, -1))
    h1, m1, _, _ = armed_device(pkg, model, images11[3:4], (4, -1))
    assert same(h8[5:6], h1) and same(m8[5:6], m1)
    # and mean alone, in the reduced mode whose Q|K|V are fp16 planes laid out by the batch's row count
    model = models("bf16")
    d_m8, d_m1 = pkg.DeviceBuffer(8 * model.tokens), pkg.DeviceBuffer(8 * model.tokens)
    for d_m, imgs in ((d_m8, images11[order]), (d_m1, images11[3:4])):
        model.set_attention(pkg.binding.AttentionSpec((-1,)), mean=d_m)
        d_img = pkg.DeviceBuffer.from_numpy(imgs)
        model.forward_device(d_img.ptr, imgs.shape[0])
        model.sync()
        model.set_attention(None)
    T = model.tokens
    assert same(d_m8.to_numpy()[5 * T:6 * T], d_m1.to_numpy()[:T])
    hb, mb, _, _ = armed_device(pkg, model, images11[3:4], (-1,))
    assert same(mb.ravel(), d_m1.to_numpy()[:T])


def test_entry_points(pkg, device, cfg, weights, models, images11):
    b = pkg.binding
    taps = (1, -1)
    # host form, 11 images through max_batch 4: chunks of 4, 4 and 3
    small = pkg.ViTHip(cfg, weights, device=0, max_batch=4)
    try:
        dev = [armed_device(pkg, small, images11[a:a + 4], taps) for a in (0, 4, 8)]
        logits, heads, mean = small.attention(images11, taps)
        assert same(heads, np.concatenate([d[0] for d in dev])) and same(mean, np.concatenate([d[1] for d in dev]))
        assert same(logits, np.concatenate([d[2] for d in dev]))
        only = np.zeros((11, 2, small.tokens), np.float32)
        small.set_attention_host(b.AttentionSpec(taps), mean=only)
        small.forward(images11)
        small.set_attention_host(None)
        assert same(only, mean)
    finally:
        small.close()
    # 8-bit entry points against the fp32 one fed the same normalised crops
    model = models("f32")
    n, S = 3, cfg.img_size
    rng = np.random.default_rng(3)
    norm = pkg.pixel_norm(MEAN, STD)
    sources = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in ((300, 260), (224, 224), (257, 401))]
    d_src = [pkg.DeviceBuffer.from_numpy(a, dtype=np.uint8) for a in sources]
    descs = [(d.ptr.value, a.shape[0], a.shape[1], a.shape[1] * 3) for d, a in zip(d_src, sources)]
    d_crops = pkg.DeviceBuffer(n * S * S * 3, dtype=np.uint8)
    model.resize_crop_u8(descs, 256, d_crops.ptr)
    model.sync()
    u8 = d_crops.to_numpy((n, S, S, 3))
    scale, bias = np.array(norm.scale[:3], dtype=np.float32), np.array(norm.bias[:3], dtype=np.float32)
    f32 = np.ascontiguousarray(((u8.astype(np.float32) * scale).astype(np.float32) + bias).astype(np.float32).transpose(0, 3, 1, 2))
    want = armed_device(pkg, model, f32, taps)
    got = armed_device(pkg, model, None, taps, call=(lambda d_l, d_p: model.forward_device_u8(d_crops.ptr, n, norm, "hwc", d_l.ptr, d_p.ptr), n))
    got_r = armed_device(pkg, model, None, taps,
                         call=(lambda d_l, d_p: model.forward_device_u8_resized(descs, 256, norm, "bilinear", "hwc", d_l.ptr, d_p.ptr), n))
    for a, b_, w in zip(got, got_r, want):
        assert same(a, w) and same(b_, w)
    # their host forms
    hh, hm = np.empty_like(want[0]), np.empty_like(want[1])
    for call in (lambda: model.forward_u8(u8, norm, None), lambda: model.forward_u8_resized(sources, 256, "bilinear", norm)):
        hh.fill(0), hm.fill(0)
        model.set_attention_host(b.AttentionSpec(taps), heads=hh, mean=hm)
        try:
            hl, _ = call()
        finally:
            model.set_attention_host(None)
        assert same(hh, want[0]) and same(hm, want[1]) and same(hl, want[2])


def test_context_refusals(pkg, device, models, images11):
    model, b, L = models("f32"), pkg.binding, pkg.lib()
    n, nc, taps = 2, 1000, (-1,)
    imgs = images11[:n]
    want_h, want_m, l0, _ = armed_device(pkg, model, imgs, taps)
    d_img, d_l = pkg.DeviceBuffer.from_numpy(imgs), pkg.DeviceBuffer(n * nc)
    d_h, d_m = attn_buffers(pkg, model, taps)
    spec = b.AttentionSpec(taps)
    model.set_attention(spec, heads=d_h, mean=d_m)
    try:
        # device form armed: the host forms refuse
        with pytest.raises(b.VitHipError, match="vit_hip_set_attention"):
            model.forward(imgs)
        # refused re-arms keep the request: a misaligned buffer, no buffer, no buffers struct, a bad spec
        cs = spec.c_struct()
        assert L.vit_hip_set_attention(model.ctx, C.byref(cs), C.byref(b.AttnBuffers(d_h.ptr.value + 4, None))) == 1
        assert "aligned" in L.vh_last_error().decode()
        assert L.vit_hip_set_attention(model.ctx, C.byref(cs), C.byref(b.AttnBuffers(None, d_m.ptr.value + 8))) == 1
        assert L.vit_hip_set_attention(model.ctx, C.byref(cs), C.byref(b.AttnBuffers(None, None))) == 1
        assert L.vit_hip_set_attention(model.ctx, C.byref(cs), None) == 1
        bad = b.AttentionSpec((11, -1)).c_struct()
        assert L.vit_hip_set_attention(model.ctx, C.byref(bad), C.byref(b.AttnBuffers(d_h.ptr, d_m.ptr))) == 1
        assert L.vit_hip_set_attention_host(model.ctx, C.byref(bad), C.byref(b.AttnBuffers(d_h.ptr, d_m.ptr))) == 1
        model.forward_device(d_img.ptr, n, d_l.ptr)
        model.sync()
        got_h, got_m = read_attn(model, d_h, d_m, n, taps)
        assert same(got_h, want_h) and same(got_m, want_m) and same(d_l.to_numpy((n, nc)), l0)
        # host form armed (which disarms the device form): the device forms refuse, nothing is launched
        hh = np.zeros_like(want_h)
        model.set_attention_host(spec, heads=hh)
        sentinel = np.full(n * nc, -7.0, np.float32)
        assert L.vh_h2d(d_l.ptr, sentinel.ctypes.data_as(C.c_void_p), sentinel.nbytes, None) == 0
        assert L.vh_memset(d_h.ptr, 0, d_h.count * 4, None) == 0
        assert L.vit_hip_forward_device(model.ctx, d_img.ptr, n, d_l.ptr, None, None) == 1
        assert "vit_hip_set_attention_host" in L.vh_last_error().decode()
        model.sync()
        assert np.array_equal(d_l.to_numpy(), sentinel) and not d_h.to_numpy().any()
        hl, _ = model.forward(imgs)
        assert same(hh, want_h) and same(hl, l0)
    finally:
        model.set_attention_host(None)
        model.set_attention(None)
    # a head_dim the kernel does not take: refused when armed, not at the first forward
    odd = pkg.preset("vit_b_16")
    odd.img_size, odd.patch_size, odd.num_classes = 64, 16, 10
    odd.embed_dim, odd.depth, odd.num_heads, odd.mlp_hidden = 96, 1, 4, 192
    m = pkg.ViTHip(odd, pkg.synth_weights(odd, 21), device=0, max_batch=2)
    try:
        d_h = pkg.DeviceBuffer(2 * 4 * m.tokens)
        with pytest.raises(b.VitHipError, match="head_dim"):
            m.set_attention(spec, heads=d_h)
    finally:
        m.close()


# ---- 10. the long-sequence plan -------------------------------------------------------------------------------------------

def test_long_sequence(pkg, device):
    """vit_b_16_384 cut to two layers (T = 577, the plan's ATTN_LONG: Q|K|V as three-part planes), two images, taps
    (0, 1): against attn_ref on the oracle's Q|K|V of those layers (computed as in test_model_maps_vs_oracle) the maps
    meet the LAUNCHER's bound -- two layers in, what the layers in front of the tap add stays inside the margin the bound
    leaves over fp32 summation -- and logits are bit-identical to un-armed."""
    from oracle.oracle import Oracle
    cfg = pkg.preset("vit_b_16_384")
    full = pkg.synth_weights(cfg, 0)
    cfg.depth = 2
    weights = full[:4 + 12 * 2] + full[-4:]
    imgs = pkg.synth_images(cfg, 0, 2)
    orc = Oracle("vit_b_16_384")

    def qkv_of(key):
        i, l = key
        lw = full[4 + 12 * l: 4 + 12 * (l + 1)]
        x = orc.forward(imgs[i], full, stop_after_layers=l)[2]
        return orc.linear(orc.layer_norm(x, lw[0], lw[1]), lw[2], lw[3], 3 * cfg.embed_dim)

    keys = [(i, l) for i in range(2) for l in range(2)]
    with ThreadPoolExecutor(4) as ex:
        qkv = dict(zip(keys, ex.map(qkv_of, keys)))
    model = pkg.ViTHip(cfg, weights, device=0, max_batch=2)
    try:
        l0, p0 = plain_device(pkg, model, imgs)
        heads, mean, l1, p1 = armed_device(pkg, model, imgs, (0, 1))
        assert same(l1, l0) and same(p1, p0) and same(mean, mean_of(heads))
        T, H = model.tokens, cfg.num_heads
        assert T == 577
        ok = True
        for i, l in keys:
            ref, _ = ar.cls_attention(qkv[(i, l)], 1, T, H)
            bnd = ar.bound(qkv[(i, l)], 1, T, H)
            rel = float((np.abs(heads[i, l].astype(np.float64) - ref[0]) / (bnd[0] * ref[0] + 1e-30)).max())
            print(f"b16_384 image {i} tap {l}: worst |p - oracle| / launcher bound = {rel:.4f}, "
                  f"max |p - oracle| = {np.abs(heads[i, l] - ref[0]).max():.3e}")
            ok = ok and within_bound(heads[i, l], ref[0], bnd[0])
        assert ok
    finally:
        model.close()
