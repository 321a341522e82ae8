"""Gallery search on the GPU (vh_launch_gallery_topk, csrc/gallery.hip; vit_hip_set_gallery / _host): the launcher on integer
data, where indices and score bits must equal the integer reference exactly, at every boundary of its row tile, query tile
and split; on real values under tests/gallery_ref.py `check`; its bit-for-bit invariances and its refusals; and the
model-level guarantees include/ViT_opencl.h states (the query is the feature output's own bits, the classifier's logits
are found again, nothing else moves, batch-position independence, both forms, every entry point, arming rules)."""
import ctypes as C

import numpy as np
import pytest

import gallery_ref as gr
import topk_ref as tr

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
RT = 128                 # VH_GALLERY_ROW_TILE: gallery rows per tile of the scan kernel
QS, QL = 16, 128         # its two query tiles: vh_gallery_query_tile(n) is QS up to QS queries and QL beyond
MAX_SPLITS = 1024        # VH_GALLERY_MAX_SPLITS
NAN_BITS = 0x7FC00000    # how a NaN score is returned
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def test_constants_are_the_kernels(pkg):
    L, b = pkg.lib(), pkg.binding
    assert (b.GALLERY_ROW_TILE, b.GALLERY_MAX_SPLITS) == (RT, MAX_SPLITS)
    assert [L.vh_gallery_query_tile(n) for n in (1, QS, QS + 1, QL, QL + 1)] == [QS, QS, QL, QL, QL]


class Gallery:
    """rows [G][E] fp32 values (for BF16: exactly representable) on the device in `dtype`, `pad` unused elements per row"""

    def __init__(self, pkg, rows, dtype=F32, pad=0):
        G, E = rows.shape
        self.G, self.E, self.dtype, self.stride = G, E, dtype, E + pad
        store = gr.bf16_round(rows) if dtype == BF16 else np.ascontiguousarray(rows, np.float32)
        if dtype == BF16:
            assert same(gr.bf16_decode(store), np.ascontiguousarray(rows, np.float32))
        padded = np.full((G, E + pad), 0x7FC1 if dtype == BF16 else np.nan, store.dtype)   # NaN in the padding: never read
        padded[:, :E] = store
        self.buf = pkg.DeviceBuffer.from_numpy(padded, dtype=store.dtype)


def search(pkg, q, gal, k, splits=0, want_scores=True, expect=0):
    """-> (indices [n][k], scores [n][k]); outputs pre-filled with a sentinel"""
    L = pkg.lib()
    n, E = q.shape
    assert E == gal.E
    d_q = pkg.DeviceBuffer.from_numpy(q)
    d_ws = pkg.DeviceBuffer(max(L.vh_gallery_workspace(n, gal.G, k, splits), 16) // 4)
    d_i = pkg.DeviceBuffer.from_numpy(np.full(n * k, -7, np.int32), dtype=np.int32)
    d_s = pkg.DeviceBuffer.from_numpy(np.full(n * k, -7.0, np.float32))
    rc = L.vh_launch_gallery_topk(None, d_q.ptr, n, E, gal.buf.ptr, gal.dtype, gal.G, gal.stride, k, splits, d_ws.ptr, d_i.ptr,
                                  d_s.ptr if want_scores else None)
    assert rc == expect, L.vh_last_error().decode()
    assert L.vh_device_sync() == 0, L.vh_last_error().decode()
    return d_i.to_numpy((n, k)), d_s.to_numpy((n, k))


# ---- 1. exact: integers in [-3, 3], every partial sum exact in fp32 (9 * 2048 < 2^24), bf16 holds the values ------------

def integer_case(n, G, E, seed):
    """Queries and rows of integers in [-3, 3].  A row is duplicated across every row-tile boundary (which every split
    boundary is), a run of 40 equal rows -- longer than any k -- crosses the first one, and where there is room rows of -0
    and +0, +inf, -inf and of two infinities of opposite sign (NaN for most queries, as 0 * inf is) are placed."""
    rng = np.random.default_rng(seed)
    q = rng.integers(-3, 4, size=(n, E)).astype(np.float32)
    rows = rng.integers(-3, 4, size=(G, E)).astype(np.float32)
    for b in range(RT, G, RT):
        rows[b] = rows[b - 1]
    if G >= RT + 20:
        rows[RT - 20:RT + 20] = rows[RT - 1]
    if G >= 16:
        rows[3], rows[5] = -0.0, 0.0
        rows[7, 0], rows[9, 0] = np.inf, -np.inf
        rows[11, 0], rows[11, E - 1] = np.inf, -np.inf
        if G > RT + 40:
            rows[G - 1], rows[G - 2] = rows[7], rows[11]
    return q, rows


def integer_reference(q, rows, k):
    """scores as fp32 (zero is +0: the kernel's chain starts at +0; NaN as NAN_BITS) and the ranking rule applied to them"""
    with np.errstate(invalid="ignore", over="ignore"):
        finite = np.isfinite(rows).all(axis=1)
        s = np.zeros((q.shape[0], rows.shape[0]))
        s[:, finite] = q.astype(np.float64) @ rows[finite].astype(np.float64).T
        for r in np.flatnonzero(~finite):
            s[:, r] = (q.astype(np.float64) * rows[r].astype(np.float64)).sum(axis=1)
    s32 = (s + 0.0).astype(np.float32)
    assert (s32[:, finite] == s[:, finite]).all()
    idx = gr.rank_exact(s32, k)
    sc = bits(np.take_along_axis(s32, idx, axis=1)).copy()
    sc[np.isnan(np.take_along_axis(s32, idx, axis=1))] = NAN_BITS
    return idx, sc


# (n_queries, n_rows, embed_dim, k, splits, dtype, pad).  Five row tiles (600 rows) under 3 splits leave a last split of one
# ragged tile, under 7 (and 1024) empty splits; 677 rows under 4 splits a ragged tile and an empty split.
EXACT = [
    (1, 1, 4, 1, 0, F32, 0),                 # one row, k == n_rows
    (1, 5, 60, 5, 1, BF16, 4),               # k == n_rows, row_stride > embed_dim
    (QS - 1, RT - 1, 64, 5, 1, F32, 0),
    (QS, RT, 64, 32, 2, BF16, 0),
    (QS + 1, RT + 1, 768, 5, 2, F32, 0),
    (QS, 32, 768, 32, 0, F32, 0),            # k == n_rows == 32
    (8, 3 * RT, 4, 5, 5, F32, 4),            # more splits than row tiles
    (QL - 1, 677, 60, 32, 4, F32, 4),
    (QL, 600, 768, 5, 3, BF16, 0),
    (QL + 1, 600, 2048, 32, 0, F32, 0),
    (1, 600, 2048, 1, 7, BF16, 8),
    (2 * QL + 2, 2 * RT + 1, 64, 5, MAX_SPLITS, BF16, 0),
]


@pytest.mark.parametrize("n,G,E,k,splits,dtype,pad", EXACT)
def test_exact_on_integers(pkg, device, n, G, E, k, splits, dtype, pad):
    q, rows = integer_case(n, G, E, 100 * n + G + E)
    want_i, want_s = integer_reference(q, rows, k)
    gal = Gallery(pkg, rows, dtype, pad)
    idx, sc = search(pkg, q, gal, k, splits)
    assert np.array_equal(idx, want_i)
    assert np.array_equal(bits(sc), want_s)
    only_i, untouched = search(pkg, q, gal, k, splits, want_scores=False)
    assert np.array_equal(only_i, want_i) and (untouched == -7.0).all()


# ---- 2. real values ------------------------------------------------------------------------------------------------------

def unit_gaussian(n, E, seed):
    a = np.random.default_rng(seed).standard_normal((n, E)).astype(np.float32)
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("n,G,E,dtype", [(5, 1000, 60, F32), (QL + 2, 1000, 768, F32), (7, 1000, 768, BF16), (QS, 700, 2048, F32),
                                        (QL + 2, 700, 2048, BF16)])
def test_real_values_hold_the_check(pkg, device, n, G, E, dtype):
    """Unit gaussian queries and rows, k = 32: indices distinct, order by the rule, every score within (E + 8) * 2^-24 *
    sum |q g| of the float64 product, nothing better left out.  Measured worst |error| / bound on an MI355X, in the order
    of the cases: 0.0556 (E = 60), 0.0051, 0.0049 (E = 768), 0.0013, 0.0019 (E = 2048); on the model's embeddings against
    the same gallery (test_against_the_feature_output) 0.0035-0.0071, and |score + bias - logit| is 0.0008 of its two
    bounds (test_against_the_classifier).  The bound is the worst case of E roundings of one sign; random ones cancel."""
    q, rows = unit_gaussian(n, E, 3 + E), unit_gaussian(G, E, 5 + E)
    if dtype == BF16:
        rows = gr.bf16_decode(gr.bf16_round(rows))
    idx, sc = search(pkg, q, Gallery(pkg, rows, dtype), 32)
    worst = gr.check(q, rows, 32, idx, sc)
    print(f"gallery n={n} G={G} E={E} dtype={dtype}: worst |error| / bound = {worst:.4f}")


# ---- 3. invariance, bit for bit ------------------------------------------------------------------------------------------

def test_invariances(pkg, device):
    E, G, k = 768, 5 * RT + 37, 32
    q, rows = unit_gaussian(QL + 3, E, 11), gr.bf16_decode(gr.bf16_round(unit_gaussian(G, E, 13)))
    rows[RT] = rows[RT - 1]
    rows[2 * RT + 5] = rows[7]
    gal = Gallery(pkg, rows, F32)
    idx, sc = search(pkg, q, gal, k, 0)
    gr.check(q, rows, k, idx, sc)
    # the same gallery under every number of splits
    for splits in (1, 2, 3, 5, 6, 7, MAX_SPLITS):
        i2, s2 = search(pkg, q, gal, k, splits)
        assert same(i2, idx) and same(s2, sc), splits
    # the same queries at other positions among another number of queries, through both query-tile kernels
    for pick in ([7], [QL + 2, 0, 5], list(range(QS)), list(range(QL + 2, -1, -1))):
        i2, s2 = search(pkg, np.ascontiguousarray(q[pick]), gal, k, 2)
        assert same(i2, idx[pick]) and same(s2, sc[pick]), pick[:3]
    # the same values stored as bf16, padded rows
    i2, s2 = search(pkg, q, Gallery(pkg, rows, BF16, 8), k, 3)
    assert same(i2, idx) and same(s2, sc)
    # no scores asked for: the same indices
    i2, untouched = search(pkg, q, gal, k, 0, want_scores=False)
    assert same(i2, idx) and (untouched == -7.0).all()
    # a row's score does not depend on where the row sits: the rows reversed give the same 32 best scores
    _, s3 = search(pkg, q, Gallery(pkg, np.ascontiguousarray(rows[::-1]), F32), k, 0)
    assert same(s3, sc)


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------

def test_launcher_refusals(pkg, device):
    L = pkg.lib()
    n, G, E, k = 3, 200, 64, 5
    q, rows = unit_gaussian(n, E, 1), unit_gaussian(G, E, 2)
    d_q, d_r = pkg.DeviceBuffer.from_numpy(q), pkg.DeviceBuffer.from_numpy(rows)
    d_ws = pkg.DeviceBuffer(L.vh_gallery_workspace(n, G, 32, 0) // 4 + 4)
    d_i = pkg.DeviceBuffer.from_numpy(np.full(n * 32, -7, np.int32), dtype=np.int32)
    d_s = pkg.DeviceBuffer.from_numpy(np.full(n * 32, -7.0, np.float32))
    off = lambda d, by: C.c_void_p(d.ptr.value + by)
    good = dict(queries=d_q.ptr, n=n, E=E, rows=d_r.ptr, dtype=F32, G=G, stride=E, k=k, splits=0, ws=d_ws.ptr, idx=d_i.ptr, sc=d_s.ptr)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return L.vh_launch_gallery_topk(None, a["queries"], a["n"], a["E"], a["rows"], a["dtype"], a["G"], a["stride"], a["k"],
                                        a["splits"], a["ws"], a["idx"], a["sc"])

    bad = [dict(k=0), dict(k=33), dict(k=6, G=5), dict(G=2 ** 31), dict(G=0), dict(E=0), dict(E=62, stride=64), dict(E=2052, stride=2052),
           dict(stride=60), dict(stride=66), dict(dtype=BF16, stride=68), dict(dtype=2), dict(n=0), dict(splits=-1),
           dict(splits=MAX_SPLITS + 1), dict(queries=None), dict(rows=None), dict(ws=None), dict(idx=None),
           dict(queries=off(d_q, 4)), dict(rows=off(d_r, 8)), dict(ws=off(d_ws, 8)), dict(idx=off(d_i, 4)), dict(sc=off(d_s, 4))]
    for kw in bad:
        L.vh_set_error(1, b"stale")
        assert call(**kw) == 1, kw
        msg = L.vh_last_error().decode()
        assert msg.startswith("vh_launch_gallery_topk: ") and len(msg) > 30, (kw, msg)
    assert L.vh_device_sync() == 0
    assert (d_i.to_numpy() == -7).all() and (d_s.to_numpy() == -7.0).all()
    assert call() == 0 and call(sc=None) == 0 and L.vh_device_sync() == 0
    gr.check(q, rows, k, d_i.to_numpy()[: n * k].reshape(n, k), d_s.to_numpy()[: n * k].reshape(n, k))


# ---- 5. the model --------------------------------------------------------------------------------------------------------

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
def images19(pkg, cfg):
    return pkg.synth_images(cfg, 0, 19)


@pytest.fixture(scope="module")
def gallery1000(pkg, device):
    """G = 1000 unit rows, bf16-representable, on the device once as fp32 and once as bf16"""
    rows = gr.bf16_decode(gr.bf16_round(unit_gaussian(1000, 768, 17)))
    return rows, pkg.DeviceBuffer.from_numpy(rows), pkg.DeviceBuffer.from_numpy(gr.bf16_round(rows), dtype=np.uint16)


def spec_for(pkg, d_rows, k=5, source="cls", tap=-1, final_norm=True, l2=True, dtype="f32", G=1000):
    return pkg.binding.GallerySpec(k, source, tap, final_norm, l2, dtype, G, 768, d_rows)


def armed_device(pkg, model, images, spec, call=None, want_scores=True):
    """forward_device with `spec` armed -> (indices, scores, logits, probs); rows beyond n keep the fill"""
    n = images.shape[0] if call is None else call[1]
    nc, k, mb = model.cfg.num_classes, spec.k, model.max_batch
    d_i = pkg.DeviceBuffer.from_numpy(np.full(mb * k, -7, np.int32), dtype=np.int32)
    d_s = pkg.DeviceBuffer.from_numpy(np.full(mb * k, -7.0, np.float32))
    d_l, d_p = pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)
    model.set_gallery(spec, spec.d_rows, indices=d_i, scores=d_s if want_scores else None)
    try:
        if call is None:
            d_img = pkg.DeviceBuffer.from_numpy(images)
            model.forward_device(d_img.ptr, n, d_l.ptr, d_p.ptr)
        else:
            call[0](d_l, d_p)
        model.sync()
    finally:
        model.set_gallery(None)
    idx, sc = d_i.to_numpy((mb, k)), d_s.to_numpy((mb, k))
    assert (idx[n:] == -7).all() and (sc[n:] == -7.0).all()
    return idx[:n], sc[:n], d_l.to_numpy((n, nc)), d_p.to_numpy((n, nc))


def plain_device(pkg, model, images):
    n, nc = images.shape[0], model.cfg.num_classes
    d_img = pkg.DeviceBuffer.from_numpy(images)
    d_l, d_p = pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)
    model.forward_device(d_img.ptr, n, d_l.ptr, d_p.ptr)
    model.sync()
    return d_l.to_numpy((n, nc)), d_p.to_numpy((n, nc))


def queries_of(pkg, model, images, source, tap, final_norm, l2):
    _, cls, pooled = model.embed(images, pkg.binding.FeatureSpec((tap,), final_norm, l2))
    return cls if source == "cls" else pooled


FEATURE_CASES = [("f32", "cls", -1, True, True), ("f32", "pooled", -1, True, True), ("f32", "cls", 5, False, False),
                 ("f32", "pooled", 5, True, False), ("f32", "cls", -1, False, True), ("f32", "pooled", 0, False, True),
                 ("bf16", "cls", -1, True, True), ("bf16", "pooled", 5, True, True), ("fp8", "cls", -1, True, True),
                 ("fp8", "pooled", -1, False, True)]


@pytest.mark.parametrize("precision,source,tap,final_norm,l2", FEATURE_CASES)
def test_against_the_feature_output(pkg, models, images19, gallery1000, precision, source, tap, final_norm, l2):
    """The query is the feature output's own bits: searching the embeddings ViTHip.embed returns, through the launcher,
    gives the armed result bit for bit, and `check` holds on them."""
    model = models(precision)
    rows, d_f32, d_bf16 = gallery1000
    imgs = images19[:8]
    q = queries_of(pkg, model, imgs, source, tap, final_norm, l2)
    k = 32
    idx, sc, logits, probs = armed_device(pkg, model, imgs, spec_for(pkg, d_f32, k, source, tap, final_norm, l2))
    print(f"{precision} {source} tap {tap}: worst |error| / bound = {gr.check(q, rows, k, idx, sc):.4f}")
    gal = Gallery(pkg, rows, F32)
    i2, s2 = search(pkg, q, gal, k, 0)
    assert same(idx, i2) and same(sc, s2)
    l0, p0 = plain_device(pkg, model, imgs)
    assert same(logits, l0) and same(probs, p0)
    # bf16 storage of the same rows: the same bits
    i3, s3, _, _ = armed_device(pkg, model, imgs, spec_for(pkg, d_bf16, k, source, tap, final_norm, l2, "bf16"))
    assert same(i3, idx) and same(s3, sc)


def test_against_the_classifier(pkg, models, cfg, weights, images19):
    """The gallery is the classifier's weight matrix: scores + bias lie within 2 bounds of the forward's own logits at
    those classes, and the best rows are the top-k classes up to what the bounds leave open."""
    model = models("f32")
    head = 4 + 12 * cfg.depth + 2
    W, bias = weights[head].reshape(cfg.num_classes, cfg.embed_dim), weights[head + 1]
    d_w = pkg.DeviceBuffer.from_numpy(W)
    imgs, k = images19[:8], 32
    idx, sc, logits, _ = armed_device(pkg, model, imgs, spec_for(pkg, d_w, k, "cls", -1, True, False))
    q = queries_of(pkg, model, imgs, "cls", -1, True, False)
    bnd = np.take_along_axis(gr.bound(q, W, cfg.embed_dim), idx, axis=1)
    diff = np.abs(sc.astype(np.float64) + bias[idx].astype(np.float64) - np.take_along_axis(logits, idx, axis=1).astype(np.float64))
    print(f"classifier: worst |score + bias - logit| / (2 bound) = {(diff / (2 * bnd)).max():.4f}")
    assert (diff <= 2 * bnd).all()
    gr.check(q, W, k, idx, sc)


@pytest.mark.parametrize("precision", ["f32", "bf16", "fp8"])
def test_nothing_else_moves(pkg, models, images19, gallery1000, precision):
    """Features, top-k, attention maps and rollout armed: all their outputs, the logits and the probabilities are the same
    bits with a gallery armed beside them, and after it is disarmed; an un-armed forward launches what it launched before."""
    model, b = models(precision), pkg.binding
    _, d_f32, _ = gallery1000
    imgs, n, k, E, T, H = images19[:5], 5, 5, model.cfg.embed_dim, model.tokens, model.cfg.num_heads

    def counts():
        d_img = pkg.DeviceBuffer.from_numpy(imgs)
        model.profile_enable(1)
        model.forward_device(d_img.ptr, n, None, None)
        got = {name: c for name, (_, c) in model.profile_read().items()}
        model.profile_enable(0)
        return got

    before = counts()
    d_cls, d_pool = pkg.DeviceBuffer(8 * 2 * E), pkg.DeviceBuffer(8 * 2 * E)
    d_lab, d_sc = pkg.DeviceBuffer(8 * k, np.int32), pkg.DeviceBuffer(8 * k)
    d_h, d_m, d_r = pkg.DeviceBuffer(8 * 2 * H * T), pkg.DeviceBuffer(8 * 2 * T), pkg.DeviceBuffer(8 * T)
    d_img, d_l, d_p = pkg.DeviceBuffer.from_numpy(imgs), pkg.DeviceBuffer(n * 1000), pkg.DeviceBuffer(n * 1000)
    outputs = (d_cls, d_pool, d_lab, d_sc, d_h, d_m, d_r, d_l, d_p)

    def others():
        for d in outputs:
            assert pkg.lib().vh_memset(d.ptr, 0, d.count * 4, None) == 0
        model.forward_device(d_img.ptr, n, d_l.ptr, d_p.ptr)
        model.sync()
        return [d.to_numpy().copy() for d in outputs]

    model.set_features(b.FeatureSpec(taps=(3, -1)), cls=d_cls, pooled=d_pool)
    model.set_topk(b.TopKSpec(k, "probs"), labels=d_lab, scores=d_sc)
    model.set_attention(b.AttentionSpec((0, -1)), heads=d_h, mean=d_m)
    model.set_rollout(b.RolloutSpec(-2), rollout=d_r)
    try:
        want = others()
        assert np.array_equal(want[2][: n * k].reshape(n, k), tr.topk(want[7].reshape(n, 1000), k)) and want[4].any() and want[6].any()
        d_gi, d_gs = pkg.DeviceBuffer(8 * k, np.int32), pkg.DeviceBuffer(8 * k)
        model.set_gallery(spec_for(pkg, d_f32, k, "pooled", -1), d_f32, indices=d_gi, scores=d_gs)
        armed = others()
        with_all = counts()
        model.set_gallery(None)
        after = others()
        for w, a, c in zip(want, armed, after):
            assert same(w, a) and same(w, c)
        # the readout and the search, timed with the classifier
        plain = counts()
        assert with_all["head_gemm"] == plain["head_gemm"] + 2
        assert all(with_all[o] == plain[o] for o in plain if o != "head_gemm")
    finally:
        for disarm in (model.set_features, model.set_topk, model.set_attention, model.set_rollout, model.set_gallery):
            disarm(None)
    assert counts() == before


def test_batch_position_independence(pkg, models, images19, gallery1000):
    _, d_f32, _ = gallery1000
    order = np.array([0, 1, 2, 4, 5, 3, 6, 7])                       # image 3 at position 5 of 8
    for precision in ("f32", "bf16"):
        model = models(precision)
        for source in ("cls", "pooled"):
            spec = spec_for(pkg, d_f32, 32, source, -1)
            i8, s8, _, _ = armed_device(pkg, model, images19[order], spec)
            i1, s1, _, _ = armed_device(pkg, model, images19[3:4], spec)
            assert same(i8[5:6], i1) and same(s8[5:6], s1) and not same(s8[4:5], s1), (precision, source)


def test_forms_and_entry_points(pkg, device, models, cfg, images19, gallery1000):
    b = pkg.binding
    rows, d_f32, d_bf16 = gallery1000
    model = models("f32")
    k = 5
    # host form, 19 images through max_batch 8 (chunks of 8, 8 and 3), against the device form; ViTHip.search
    for source, tap in (("cls", -1), ("pooled", 3)):
        spec = spec_for(pkg, d_f32, k, source, tap)
        dev = [armed_device(pkg, model, images19[a:a + 8], spec) for a in (0, 8, 16)]
        hi, hs = np.full((19, k), -7, np.int32), np.full((19, k), -7.0, np.float32)
        model.set_gallery_host(spec_for(pkg, d_f32, k, source, tap), d_f32, indices=hi, scores=hs)
        try:
            logits, _ = model.forward(images19)
        finally:
            model.set_gallery_host(None)
        assert same(hi, np.concatenate([d[0] for d in dev])) and same(hs, np.concatenate([d[1] for d in dev]))
        assert same(logits, np.concatenate([d[2] for d in dev]))
        si, ss = model.search(images19, rows, k, source, tap)
        assert same(si, hi) and same(ss, hs)
    si, ss = model.search(images19[:3], gr.bf16_round(rows), k)                 # uint16 rows: bf16 storage
    want = armed_device(pkg, model, images19[:3], spec_for(pkg, d_f32, k))
    assert same(si, want[0]) and same(ss, want[1])
    # no scores buffer in the host form
    hi = np.full((3, k), -7, np.int32)
    model.set_gallery_host(spec_for(pkg, d_f32, k), d_f32, indices=hi)
    try:
        model.forward(images19[:3])
    finally:
        model.set_gallery_host(None)
    assert same(hi, want[0])
    # 8-bit, resized and box entry points against the fp32 one fed the same normalised crops
    n, S = 3, cfg.img_size
    rng = np.random.default_rng(3)
    norm = pkg.pixel_norm(MEAN, STD)
    sources = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in ((300, 260), (224, 224), (257, 401))]
    d_src = [pkg.DeviceBuffer.from_numpy(a, dtype=np.uint8) for a in sources]
    descs = [(d.ptr.value, a.shape[0], a.shape[1], a.shape[1] * 3) for d, a in zip(d_src, sources)]
    d_crops = pkg.DeviceBuffer(n * S * S * 3, dtype=np.uint8)
    scale, bias = np.array(norm.scale[:3], dtype=np.float32), np.array(norm.bias[:3], dtype=np.float32)
    spec = spec_for(pkg, d_bf16, k, "pooled", -1, dtype="bf16")

    def normalised():
        u8 = d_crops.to_numpy((n, S, S, 3))
        return u8, np.ascontiguousarray(((u8.astype(np.float32) * scale).astype(np.float32) + bias).astype(np.float32).transpose(0, 3, 1, 2))

    def host(call):
        hi, hs = np.full((n, k), -7, np.int32), np.full((n, k), -7.0, np.float32)
        model.set_gallery_host(spec, spec.d_rows, indices=hi, scores=hs)
        try:
            hl, _ = call()
        finally:
            model.set_gallery_host(None)
        return hi, hs, hl

    model.resize_crop_u8(descs, 256, d_crops.ptr)
    model.sync()
    u8, f32 = normalised()
    want = armed_device(pkg, model, f32, spec)
    got = armed_device(pkg, model, None, spec, call=(lambda d_l, d_p: model.forward_device_u8(d_crops.ptr, n, norm, "hwc", d_l.ptr, d_p.ptr), n))
    got_r = armed_device(pkg, model, None, spec,
                         call=(lambda d_l, d_p: model.forward_device_u8_resized(descs, 256, norm, "bilinear", "hwc", d_l.ptr, d_p.ptr), n))
    for a, b_, w in zip(got, got_r, want):
        assert same(a, w) and same(b_, w)
    for call in (lambda: model.forward_u8(u8, norm, None), lambda: model.forward_u8_resized(sources, 256, "bilinear", norm)):
        for a, w in zip(host(call), want):
            assert same(a, w)
    boxes = [(0, (10.0, 20.0, 250.0, 290.0)), (2, (0.0, 0.0, 401.0, 257.0)), (2, (100.5, 30.25, 300.0, 200.0))]
    model.crop_boxes_u8(descs, boxes, d_crops.ptr, filter="bicubic")
    model.sync()
    _, f32 = normalised()
    want = armed_device(pkg, model, f32, spec)
    got = armed_device(pkg, model, None, spec,
                       call=(lambda d_l, d_p: model.forward_device_u8_boxes(descs, boxes, norm, "bicubic", "hwc", d_l.ptr, d_p.ptr), n))
    for a, w in zip(got, want):
        assert same(a, w)
    for a, w in zip(host(lambda: model.forward_u8_boxes(sources, boxes, "bicubic", norm)), want):
        assert same(a, w)


def test_cls_only_last_gives_equal_bits(pkg, models, images19, gallery1000):
    _, d_f32, _ = gallery1000
    model = models("f32")
    imgs = images19[:4]
    try:
        off = {s: armed_device(pkg, model, imgs, spec_for(pkg, d_f32, 32, s, -1)) for s in ("cls", "pooled")}
        inner = armed_device(pkg, model, imgs, spec_for(pkg, d_f32, 32, "pooled", 5))
        model.set_last_layer_cls_only(True)
        for s in ("cls", "pooled"):
            on = armed_device(pkg, model, imgs, spec_for(pkg, d_f32, 32, s, -1))
            for a, w in zip(on, off[s]):
                assert same(a, w), s
        for a, w in zip(armed_device(pkg, model, imgs, spec_for(pkg, d_f32, 32, "pooled", 5)), inner):
            assert same(a, w)
    finally:
        model.set_last_layer_cls_only(False)


def test_arming_rules(pkg, device, models, images19, gallery1000):
    model, b, L = models("f32"), pkg.binding, pkg.lib()
    _, d_f32, _ = gallery1000
    n, nc, k = 2, 1000, 5
    imgs = images19[:n]
    spec = spec_for(pkg, d_f32, k)
    want_i, want_s, l0, _ = armed_device(pkg, model, imgs, spec)
    d_img, d_l = pkg.DeviceBuffer.from_numpy(imgs), pkg.DeviceBuffer(n * nc)
    d_i, d_s = pkg.DeviceBuffer(8 * k, np.int32), pkg.DeviceBuffer(8 * k)
    model.set_gallery(spec, d_f32, indices=d_i, scores=d_s)
    try:
        # device form armed: the host forms refuse
        with pytest.raises(b.VitHipError, match="vit_hip_set_gallery"):
            model.forward(imgs)
        assert "gallery" in L.vh_last_error().decode()
        # refused re-arms keep the request
        cs = spec.c_struct()
        bufs = lambda i, s: C.byref(b.GalleryBuffers(i, s))
        assert L.vit_hip_set_gallery(model.ctx, C.byref(cs), bufs(d_i.ptr.value + 4, d_s.ptr)) == 1
        assert "aligned" in L.vh_last_error().decode()
        assert L.vit_hip_set_gallery(model.ctx, C.byref(cs), bufs(None, d_s.ptr)) == 1
        assert L.vit_hip_set_gallery(model.ctx, C.byref(cs), None) == 1
        for field, value, word in (("k", 33, "k must"), ("n_rows", 3, "n_rows"), ("tap", 12, "tap"), ("source", 2, "source"), ("dtype", 3, "dtype"),
                                   ("row_stride", 764, "row_stride"), ("d_rows", None, "rows"), ("d_rows", d_f32.ptr.value + 4, "aligned")):
            bad = spec.c_struct()
            setattr(bad, field, value)
            for entry in (L.vit_hip_set_gallery, L.vit_hip_set_gallery_host):
                assert entry(model.ctx, C.byref(bad), bufs(d_i.ptr, d_s.ptr)) == 1, field
                assert word in L.vh_last_error().decode(), (field, L.vh_last_error().decode())
        model.forward_device(d_img.ptr, n, d_l.ptr)
        model.sync()
        assert same(d_i.to_numpy((8, k))[:n], want_i) and same(d_s.to_numpy((8, k))[:n], want_s) and same(d_l.to_numpy((n, nc)), l0)
        # host form armed (which disarms the device form): the device forms refuse, nothing is launched
        hi, hs = np.zeros_like(want_i), np.zeros_like(want_s)
        model.set_gallery_host(spec_for(pkg, d_f32, k), d_f32, indices=hi, scores=hs)
        sentinel = np.full(n * nc, -7.0, np.float32)
        assert L.vh_h2d(d_l.ptr, sentinel.ctypes.data_as(C.c_void_p), sentinel.nbytes, None) == 0
        assert L.vh_memset(d_i.ptr, 0, d_i.count * 4, None) == 0
        assert L.vit_hip_forward_device(model.ctx, d_img.ptr, n, d_l.ptr, None, None) == 1
        assert "vit_hip_set_gallery_host" in L.vh_last_error().decode()
        model.sync()
        assert np.array_equal(d_l.to_numpy(), sentinel) and not d_i.to_numpy().any()
        hl, _ = model.forward(imgs)
        assert same(hi, want_i) and same(hs, want_s) and same(hl, l0)
    finally:
        model.set_gallery_host(None)
        model.set_gallery(None)
    # disarm frees: a gallery whose scratch is large (k = 32 over 1024 splits' worth of rows: 8 x 265 KB), disarmed and
    # armed again, several times over, then used
    big_rows = 1024 * RT
    d_big = pkg.DeviceBuffer(big_rows * 768 // 2, dtype=np.float32)            # bf16 rows: 2 bytes each
    assert L.vh_memset(d_big.ptr, 0, d_big.count * 4, None) == 0
    big = spec_for(pkg, d_big, 32, dtype="bf16", G=big_rows)
    assert b.gallery_check(model.cfg, big) == 768 * 4 + 1024 * 32 * 8
    d_i32, d_s32 = pkg.DeviceBuffer(8 * 32, np.int32), pkg.DeviceBuffer(8 * 32)
    for _ in range(3):
        model.set_gallery(big, d_big, indices=d_i32, scores=d_s32)
        model.set_gallery(None)
    model.set_gallery(big, d_big, indices=d_i32, scores=d_s32)
    try:
        model.forward_device(d_img.ptr, n, d_l.ptr)
        model.sync()
        got = d_i32.to_numpy((8, 32))[:n]
        assert (got == np.arange(32)).all()                                    # all scores equal: the lowest indices
    finally:
        model.set_gallery(None)
