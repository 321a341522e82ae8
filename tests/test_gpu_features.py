"""Feature outputs on the GPU (vit_hip_set_features, csrc/features.hip): the readout launcher against the oracle, its
bit-identity with the existing LayerNorm, the model-level outputs against the oracle at intermediate layers, and the
guarantees the header states (logits untouched, derived outputs exact, batch-position independence, entry points,
refusals)."""
import ctypes as C

import numpy as np
import pytest

import features_ref as fr

pytestmark = pytest.mark.gpu

OP_TOL = 2e-5          # the tolerance tests/test_gpu_parity.py holds the LayerNorm to, same input scale
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _launch(pkg, name, *args):
    L = pkg.lib()
    rc = getattr(L, name)(*args)
    assert rc == 0, f"{name}: {L.vh_last_error().decode()}"
    assert L.vh_device_sync() == 0, L.vh_last_error().decode()


def _np_dtype(spec):
    return spec.np_dtype


def _alloc(pkg, cfg, spec, n, want):
    sizes = dict(zip(("cls", "pooled", "tokens"), pkg.binding.feature_sizes(cfg, spec)))
    return {k: pkg.DeviceBuffer(n * sizes[k], dtype=_np_dtype(spec)) for k in want}, sizes


def _read(bufs, sizes, n):
    return {k: b.to_numpy()[: n * sizes[k]].reshape(n, -1) for k, b in bufs.items()}


def run_device(pkg, model, images, spec, want=("cls", "pooled", "tokens")):
    """images fp32 [n][C][H][W] through forward_device with `spec` armed -> dict of outputs + logits + probs"""
    n, nc = images.shape[0], model.cfg.num_classes
    bufs, sizes = _alloc(pkg, model.cfg, spec, n, want)
    d_img = pkg.DeviceBuffer.from_numpy(images)
    d_l, d_p = pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)
    model.set_features(spec, **bufs)
    model.forward_device(d_img.ptr, n, d_l.ptr, d_p.ptr)
    model.sync()
    model.set_features(None)
    out = _read(bufs, sizes, n)
    out["logits"], out["probs"] = d_l.to_numpy((n, nc)), d_p.to_numpy((n, nc))
    return out


def plain_device(pkg, model, images):
    n, nc = images.shape[0], model.cfg.num_classes
    d_img = pkg.DeviceBuffer.from_numpy(images)
    d_l, d_p = pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)
    model.forward_device(d_img.ptr, n, d_l.ptr, d_p.ptr)
    model.sync()
    return d_l.to_numpy((n, nc)), d_p.to_numpy((n, nc))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def cfg(pkg):
    return pkg.preset("vit_b_16")


@pytest.fixture(scope="module")
def models(pkg, device, cfg, weights):
    """ViT-B/16, synthetic weights, one context per precision, made on first use"""
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
def images8(pkg, cfg):
    return pkg.synth_images(cfg, 0, 8)


# ---- 1. the launcher against the oracle ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n,T,E,preset", [(1, 2, 768, "vit_b_16"), (3, 197, 768, "vit_b_16"), (2, 577, 768, "vit_b_16"),
                                          (5, 50, 768, "vit_b_16"), (2, 197, 1024, "vit_l_16"), (2, 257, 1280, "vit_h_14")])
def test_readout_vs_oracle(pkg, device, n, T, E, preset):
    from oracle.oracle import Oracle
    orc = Oracle(preset)
    assert orc.cfg.embed_dim == E
    L = pkg.lib()
    x = orc.synth_fill(n * T * E, 11 + n * T, 3.0, 0.5).reshape(n * T, E)
    g, b = orc.synth_fill(E, 5, 0.5, 1.0), orc.synth_fill(E, 6, 0.2, 0.0)
    normed = orc.layer_norm(x, g, b)
    d_x, d_g, d_b = (pkg.DeviceBuffer.from_numpy(a) for a in (x, g, b))
    scratch_bytes = L.vh_feature_readout_scratch(n, T, E)
    d_s = pkg.DeviceBuffer(scratch_bytes // 4 + 4)
    P = T - 1
    d_cls, d_pool, d_tok = pkg.DeviceBuffer(n * E), pkg.DeviceBuffer(n * E), pkg.DeviceBuffer(n * P * E)
    worst = 0.0
    for final_norm in (0, 1):
        for l2 in (0, 1):
            for layout in (0, 1):
                _launch(pkg, "vh_launch_feature_readout", None, d_x.ptr, None, 0, d_g.ptr, d_b.ptr, 1e-6, final_norm, l2, 0, layout,
                        n, T, E, 0, 1, d_cls.ptr, d_pool.ptr, d_tok.ptr, d_s.ptr, scratch_bytes)
                rows = normed if final_norm else x
                want_cls, want_pool, want_tok = fr.features(rows, n, T, bool(l2))
                got_tok = d_tok.to_numpy((n, E, P) if layout else (n, P, E))
                if layout:
                    want_tok = fr.nlc_to_nchw(want_tok)
                errs = [np.abs(d_cls.to_numpy((n, E)) - want_cls).max(), np.abs(d_pool.to_numpy((n, E)) - want_pool).max(),
                        np.abs(got_tok - want_tok).max()]
                print(f"readout n={n} T={T} E={E} norm={final_norm} l2={l2} layout={layout}: max err cls/pooled/tokens = {errs}")
                worst = max(worst, *errs)
                assert max(errs) <= OP_TOL
                if not final_norm:
                    assert same(got_tok, want_tok.astype(np.float32)), "final_norm = 0 must hand the rows through bit for bit"
    # cls alone reads the class rows only; compacted class rows with their own stride give the same values
    d_c2 = pkg.DeviceBuffer(n * E)
    d_rows = pkg.DeviceBuffer.from_numpy(x[::T].copy())
    _launch(pkg, "vh_launch_feature_readout", None, d_x.ptr, None, 0, d_g.ptr, d_b.ptr, 1e-6, 1, 0, 0, 0, n, T, E, 0, 1, d_cls.ptr, None,
            None, None, 0)
    _launch(pkg, "vh_launch_feature_readout", None, None, d_rows.ptr, E, d_g.ptr, d_b.ptr, 1e-6, 1, 0, 0, 0, n, T, E, 0, 1, d_c2.ptr,
            None, None, None, 0)
    assert same(d_cls.to_numpy(), d_c2.to_numpy())
    assert np.abs(d_cls.to_numpy((n, E)) - normed[::T]).max() <= OP_TOL


def test_readout_launcher_refusals(pkg, device):
    L = pkg.lib()
    d, d_out = pkg.DeviceBuffer.from_numpy(np.ones(4 * 772, np.float32)), pkg.DeviceBuffer(768)
    base = dict(x=d.ptr, g=d.ptr, b=d.ptr, E=768, T=2, n=1, dtype=0, layout=0, cls=d_out.ptr, pooled=None, scratch=None, sb=0)

    def rc(**kw):
        a = dict(base, **kw)
        return L.vh_launch_feature_readout(None, a["x"], None, 0, a["g"], a["b"], 1e-6, 1, 0, a["dtype"], a["layout"], a["n"], a["T"],
                                           a["E"], 0, 1, a["cls"], a["pooled"], None, a["scratch"], a["sb"])

    assert rc(E=770) == 1 and rc(E=4096) == 1 and rc(dtype=2) == 1 and rc(layout=3) == 1 and rc(cls=None) == 1
    assert rc(g=None) == 1 and rc(pooled=d_out.ptr) == 1 and rc(pooled=d_out.ptr, T=1) == 1 and rc(n=0) == 1
    assert L.vh_last_error().decode().startswith("vh_launch_feature_readout")
    assert rc() == 0 and L.vh_device_sync() == 0


# ---- 2. bit-identity with the existing LayerNorm ------------------------------------------------------------------------

def _layer_norm_of_stream(pkg, model, n):
    cfg, T = model.cfg, model.tokens
    E = cfg.embed_dim
    stream = model.read_tokens(n)
    d_x, d_y = pkg.DeviceBuffer.from_numpy(stream), pkg.DeviceBuffer(n * T * E)
    L = pkg.lib()
    g, b = L.vit_hip_weight(model.ctx, 4 + 12 * cfg.depth), L.vit_hip_weight(model.ctx, 5 + 12 * cfg.depth)
    _launch(pkg, "vh_launch_layer_norm", None, d_x.ptr, g, b, d_y.ptr, n * T, E, E, E, cfg.eps)
    return d_y.to_numpy((n, T, E))


@pytest.mark.parametrize("precision", ["f32", "bf16", "fp8", "f32_fp16x2"])
def test_last_layer_is_the_final_layer_norm_bit_for_bit(pkg, models, images8, precision):
    model = models(precision)
    out = run_device(pkg, model, images8[:3], pkg.binding.FeatureSpec(taps=(-1,)))
    want = _layer_norm_of_stream(pkg, model, 3)
    assert same(out["tokens"].reshape(3, -1, 768), want[:, 1:])
    assert same(out["cls"], want[:, 0])


def test_last_layer_bit_for_bit_long_sequence(pkg, device):
    cfg = pkg.preset("vit_b_16_384")
    model = pkg.ViTHip(cfg, pkg.synth_weights(cfg, 0), device=0, max_batch=2)
    try:
        out = run_device(pkg, model, pkg.synth_images(cfg, 0, 2), pkg.binding.FeatureSpec(taps=(-1,)))
        want = _layer_norm_of_stream(pkg, model, 2)
        assert same(out["tokens"].reshape(2, 576, 768), want[:, 1:])
        assert same(out["cls"], want[:, 0])
        assert np.abs(out["pooled"] - want[:, 1:].astype(np.float64).mean(axis=1)).max() <= OP_TOL
    finally:
        model.close()


# ---- 3. model level against the oracle, intermediate layers included ----------------------------------------------------

def test_model_features_vs_oracle(pkg, models, oracle, weights, images8):
    """Bound: the residual stream is held to 2e-5 * max(1, max|x|) of the oracle's (test_model_residual_stream_vs_oracle);
    the LayerNorm scales a perturbation of a row by at most max|gamma| / sigma_row; plus the LayerNorm's own OP_TOL."""
    taps, n, T, E = (3, 7, -1), 2, 197, 768
    out = run_device(pkg, models("f32"), images8[:n], pkg.binding.FeatureSpec(taps=taps))
    g, b = weights[4 + 12 * 12], weights[5 + 12 * 12]
    for k, tap in enumerate(taps):
        layer = tap % 12
        for i in range(n):
            _, _, rows = oracle.forward(images8[i], weights, stop_after_layers=layer + 1)
            rows = rows.reshape(T, E)
            sigma = np.sqrt(rows.astype(np.float64).var(axis=1) + 1e-6)
            bound = 2e-5 * max(1.0, float(np.abs(rows).max())) * float(np.abs(g).max()) / float(sigma.min()) + OP_TOL
            cls, pooled, tokens = fr.features(oracle.layer_norm(rows, g, b), 1, T, False)
            errs = [np.abs(out["cls"][i].reshape(3, E)[k] - cls[0]).max(), np.abs(out["pooled"][i].reshape(3, E)[k] - pooled[0]).max(),
                    np.abs(out["tokens"][i].reshape(3, T - 1, E)[k] - tokens[0]).max()]
            print(f"layer {layer} image {i}: max err cls/pooled/tokens = {errs}, bound {bound:.3e}")
            assert max(errs) <= bound


# ---- 4. nothing else moves ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "bf16", "fp8"])
def test_logits_unchanged_and_disarm_is_clean(pkg, models, images8, precision):
    model = models(precision)
    b = pkg.binding
    imgs = images8[:5]
    l0, p0 = plain_device(pkg, model, imgs)
    hl0, hp0 = model.forward(imgs)
    spec = b.FeatureSpec(taps=(5, -1), l2_normalize=True)
    last = run_device(pkg, model, imgs, b.FeatureSpec(taps=(-1,)), want=("cls", "pooled"))
    for cls_only in (False, True):
        before = model.set_last_layer_cls_only(cls_only)
        try:
            out = run_device(pkg, model, imgs, spec)
            assert same(out["logits"], l0) and same(out["probs"], p0)
            only_cls = run_device(pkg, model, imgs, b.FeatureSpec(taps=(-1,)), want=("cls",))   # compacted class rows when on
            assert same(only_cls["logits"], l0) and same(only_cls["cls"], last["cls"])
            again = run_device(pkg, model, imgs, b.FeatureSpec(taps=(-1,)), want=("cls", "pooled"))
            assert same(again["pooled"], last["pooled"]) and same(again["cls"], last["cls"]) and same(again["logits"], l0)
            logits, cls, pooled = model.embed(imgs, spec)
            assert same(logits, hl0) and same(cls, out["cls"]) and same(pooled, out["pooled"])
        finally:
            model.set_last_layer_cls_only(before)
    # disarmed: a forward writes nothing into the old buffers
    bufs, sizes = _alloc(pkg, model.cfg, spec, 5, ("cls", "pooled", "tokens"))
    model.set_features(spec, **bufs)
    model.set_features(None)
    sentinel = {k: np.full(v.count, 0x7FC01234, dtype=np.uint32).view(np.float32) for k, v in bufs.items()}
    for k, v in bufs.items():
        assert pkg.lib().vh_h2d(v.ptr, sentinel[k].ctypes.data_as(C.c_void_p), sentinel[k].nbytes, None) == 0
    l1, p1 = plain_device(pkg, model, imgs)
    assert same(l1, l0) and same(p1, p0)
    for k, v in bufs.items():
        assert np.array_equal(v.to_numpy().view(np.uint32), sentinel[k].view(np.uint32))
    hl1, hp1 = model.forward(imgs)
    assert same(hl1, hl0) and same(hp1, hp0)


# ---- 5. derived outputs are exact functions of the fp32 NLC output ------------------------------------------------------

def test_derived_outputs_are_exact(pkg, models, images8):
    model, b = models("f32"), pkg.binding
    imgs, n, P, E = images8[:3], 3, 196, 768
    for l2 in (False, True):
        base = run_device(pkg, model, imgs, b.FeatureSpec(taps=(4, 9), l2_normalize=l2))
        tok = base["tokens"].reshape(n, 2, P, E)
        nchw = run_device(pkg, model, imgs, b.FeatureSpec(taps=(4, 9), l2_normalize=l2, token_layout="nchw"))
        assert same(nchw["tokens"].reshape(n, 2, E, P), fr.nlc_to_nchw(tok))
        assert same(nchw["cls"], base["cls"]) and same(nchw["pooled"], base["pooled"])
        for layout in ("nlc", "nchw"):
            h = run_device(pkg, model, imgs, b.FeatureSpec(taps=(4, 9), l2_normalize=l2, dtype="bf16", token_layout=layout))
            want_tok = tok if layout == "nlc" else fr.nlc_to_nchw(tok)
            assert np.array_equal(h["tokens"].reshape(want_tok.shape), fr.bf16_bits(want_tok))
            assert np.array_equal(h["cls"], fr.bf16_bits(base["cls"])) and np.array_equal(h["pooled"], fr.bf16_bits(base["pooled"]))
            assert same(h["logits"], base["logits"])
        for k, tap in enumerate((4, 9)):
            one = run_device(pkg, model, imgs, b.FeatureSpec(taps=(tap,), l2_normalize=l2))
            assert same(one["cls"], base["cls"].reshape(n, 2, E)[:, k]) and same(one["pooled"], base["pooled"].reshape(n, 2, E)[:, k])
            assert same(one["tokens"].reshape(n, P, E), tok[:, k])


# ---- 6. batch-position independence -------------------------------------------------------------------------------------

def test_batch_position_independence(pkg, models, cfg, images8):
    model, b = models("f32"), pkg.binding
    spec = b.FeatureSpec(taps=(2, -1), l2_normalize=True)
    imgs = images8[:5]
    perm = np.array([3, 0, 4, 1, 2])
    a, p = run_device(pkg, model, imgs, spec), run_device(pkg, model, imgs[perm], spec)
    for k in ("cls", "pooled", "tokens", "logits"):
        assert same(p[k], a[k][perm]), k
    full = run_device(pkg, model, images8, spec)
    one = run_device(pkg, model, images8[6:7], spec)
    for k in ("cls", "pooled", "tokens"):
        assert same(full[k][:5], a[k]) and same(full[k][6:7], one[k]), k
    # host form: 11 images through max_batch = 8 (two chunks), and a permutation of them
    eleven = pkg.synth_images(cfg, 0, 11)
    _, cls, pooled = model.embed(eleven, spec)
    assert same(cls[:8], full["cls"]) and same(pooled[:8], full["pooled"])
    perm11 = np.array([10, 3, 7, 0, 9, 1, 8, 2, 6, 4, 5])
    _, cls_p, pooled_p = model.embed(eleven[perm11], spec)
    assert same(cls_p, cls[perm11]) and same(pooled_p, pooled[perm11])


# ---- 7. entry points ----------------------------------------------------------------------------------------------------

def test_u8_entry_points_give_the_same_features(pkg, models, cfg):
    model, b = models("f32"), pkg.binding
    n, S = 3, cfg.img_size
    rng = np.random.default_rng(3)
    norm = pkg.pixel_norm(MEAN, STD)
    # sources of three sizes; their crops (vit_hip_resize_crop_u8) are the pixels every other entry point is given
    sources = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in ((300, 260), (224, 224), (257, 401))]
    d_src = [pkg.DeviceBuffer.from_numpy(a, dtype=np.uint8) for a in sources]
    descs = [(d.ptr.value, a.shape[0], a.shape[1], a.shape[1] * 3) for d, a in zip(d_src, sources)]
    d_crops = pkg.DeviceBuffer(n * S * S * 3, dtype=np.uint8)
    model.resize_crop_u8(descs, 256, d_crops.ptr)
    model.sync()
    u8 = d_crops.to_numpy((n, S, S, 3))
    scale, bias = np.array(norm.scale[:3], dtype=np.float32), np.array(norm.bias[:3], dtype=np.float32)
    f32 = np.ascontiguousarray(((u8.astype(np.float32) * scale).astype(np.float32) + bias).astype(np.float32).transpose(0, 3, 1, 2))
    spec = b.FeatureSpec(taps=(6, -1))
    want = run_device(pkg, model, f32, spec)
    nc = cfg.num_classes

    def armed(call):
        bufs, sizes = _alloc(pkg, cfg, spec, n, ("cls", "pooled", "tokens"))
        d_l = pkg.DeviceBuffer(n * nc)
        model.set_features(spec, **bufs)
        call(d_l)
        model.sync()
        model.set_features(None)
        out = _read(bufs, sizes, n)
        out["logits"] = d_l.to_numpy((n, nc))
        return out

    d_u8 = pkg.DeviceBuffer.from_numpy(u8, dtype=np.uint8)
    got = armed(lambda d_l: model.forward_device_u8(d_u8.ptr, n, norm, "hwc", d_l.ptr))
    got_r = armed(lambda d_l: model.forward_device_u8_resized(descs, 256, norm, "bilinear", "hwc", d_l.ptr))
    for k in ("cls", "pooled", "tokens", "logits"):
        assert same(got[k], want[k]), k
        assert same(got_r[k], want[k]), k
    # host forms
    c_el, p_el, _ = b.feature_sizes(cfg, spec)
    cls, pooled = np.empty((n, c_el), np.float32), np.empty((n, p_el), np.float32)
    model.set_features_host(spec, cls=cls, pooled=pooled)
    try:
        model.forward_u8(u8, norm, None)
    finally:
        model.set_features_host(None)
    _, cls_f, pooled_f = model.embed(f32, spec)
    assert same(cls, cls_f) and same(pooled, pooled_f) and same(cls, want["cls"]) and same(pooled, want["pooled"])


# ---- 8. refusals that need a context ------------------------------------------------------------------------------------

def test_context_refusals(pkg, models, cfg, images8):
    model, b, L = models("f32"), pkg.binding, pkg.lib()
    spec = b.FeatureSpec(taps=(-1,))
    cs = spec.c_struct()
    n, nc, E = 2, cfg.num_classes, cfg.embed_dim
    imgs = images8[:n]
    l0, _ = plain_device(pkg, model, imgs)
    d_cls = pkg.DeviceBuffer(n * E)
    h_cls, h_tok = np.zeros((n, E), np.float32), np.zeros((n, 196 * E), np.float32)
    d_img, d_l = pkg.DeviceBuffer.from_numpy(imgs), pkg.DeviceBuffer(n * nc)

    none = b.FeatureBuffers(None, None, None)
    assert L.vit_hip_set_features(model.ctx, C.byref(cs), C.byref(none)) == 1
    assert L.vit_hip_set_features_host(model.ctx, C.byref(cs), C.byref(none)) == 1
    assert L.vit_hip_set_features(model.ctx, C.byref(cs), None) == 1
    with pytest.raises(b.VitHipError, match="host form"):
        model.set_features_host(spec, cls=h_cls, tokens=h_tok)
    bad = b.FeatureSpec(taps=(12,)).c_struct()
    bufs = b.FeatureBuffers(d_cls.ptr, None, None)
    assert L.vit_hip_set_features(model.ctx, C.byref(bad), C.byref(bufs)) == 1
    misaligned = b.FeatureBuffers(d_cls.ptr.value + 4, None, None)
    assert L.vit_hip_set_features(model.ctx, C.byref(cs), C.byref(misaligned)) == 1

    # host form armed: the device forms refuse, nothing is launched, and the host form still works
    model.set_features_host(spec, cls=h_cls)
    sentinel = np.full(n * nc, -7.0, np.float32)
    assert L.vh_h2d(d_l.ptr, sentinel.ctypes.data_as(C.c_void_p), sentinel.nbytes, None) == 0
    assert L.vit_hip_forward_device(model.ctx, d_img.ptr, n, d_l.ptr, None, None) == 1
    assert "vit_hip_set_features_host" in L.vh_last_error().decode()
    model.sync()
    assert np.array_equal(d_l.to_numpy(), sentinel)
    hl, _ = model.forward(imgs)
    assert same(hl, l0) and np.abs(h_cls).max() > 0
    # device form armed (which disarms the host form): the host forms refuse
    model.set_features(spec, cls=d_cls)
    with pytest.raises(b.VitHipError, match="armed for device"):
        model.forward(imgs)
    model.forward_device(d_img.ptr, n, d_l.ptr)
    model.sync()
    assert same(d_l.to_numpy((n, nc)), l0) and same(d_cls.to_numpy((n, E)), h_cls)
    model.set_features(None)
    hl, _ = model.forward(imgs)
    assert same(hl, l0)


# ---- 9. full size once --------------------------------------------------------------------------------------------------

def test_full_size_batch(pkg, models, cfg):
    b = pkg.binding
    big, n, E, P = models("f32", 512), 512, 768, 196
    spec = b.FeatureSpec(taps=(2, 5, 8, -1), dtype="bf16", token_layout="nchw", l2_normalize=True)
    imgs = pkg.synth_images(cfg, 0, n)
    out = run_device(pkg, big, imgs, spec)
    assert out["cls"].shape == (n, 4 * E) and out["tokens"].shape == (n, 4 * E * P)
    for i in (0, 255, 511):
        alone = run_device(pkg, big, imgs[i:i + 1], spec)
        for k in ("cls", "pooled", "tokens", "logits"):
            assert same(alone[k][0], out[k][i]), (k, i)
    assert np.isfinite(fr.bf16_to_f32(out["pooled"])).all()
