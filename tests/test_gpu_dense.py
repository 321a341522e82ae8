"""The dense head on the GPU (vh_launch_dense_logits, vh_launch_dense_labels, csrc/dense_head.hip; vit_hip_set_dense /
_host): the logits launcher on integer data, where the bits must equal the integer reference at every class-tile, width and
token-tile boundary and under strides that skip NaN rows; the labels launcher on integer logits at the scales where the
header's fp32 expressions are exact, ties, NaNs and infinities everywhere; both under tests/dense_ref.py `check` on real
values; their refusals; and the model-level guarantees include/ViT_opencl.h states (the token rows are the feature
output's own bits, nothing else moves, batch-position independence, both forms, every entry point, arming rules)."""
import ctypes as C

import numpy as np
import pytest

import dense_ref as dr
import gallery_ref as gr

pytestmark = pytest.mark.gpu

TT = 128                 # VH_DENSE_TOKEN_TILE: token rows per workgroup of the logits kernel
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def test_constants_are_the_kernels(pkg):
    assert pkg.binding.DENSE_TOKEN_TILE == TT and pkg.binding.DENSE_MAX_LABELS == 256


def dev(pkg, a, dtype=np.float32):
    return pkg.DeviceBuffer.from_numpy(np.ascontiguousarray(a, dtype), dtype=dtype)


def run_logits(pkg, x, W, b, t_pad=0, w_pad=0, skip_rows=0):
    """x [n][P][E] -> patch logits [n][P][C].  The tokens lie as [n][skip_rows + P][E + t_pad] with NaN in the skipped rows
    and in every padding, the weight as [C][E + w_pad] with NaN padding: none of that may be read."""
    L = pkg.lib()
    n, P, E = x.shape
    Cc = W.shape[0]
    tok = np.full((n, skip_rows + P, E + t_pad), np.nan, np.float32)
    tok[:, skip_rows:, :E] = x
    wgt = np.full((Cc, E + w_pad), np.nan, np.float32)
    wgt[:, :E] = W
    d_t, d_w, d_b = dev(pkg, tok), dev(pkg, wgt), None if b is None else dev(pkg, b)
    d_o = dev(pkg, np.full(n * P * Cc, -7.0, np.float32))
    rows = C.c_void_p(d_t.ptr.value + skip_rows * (E + t_pad) * 4)
    rc = L.vh_launch_dense_logits(None, rows, (skip_rows + P) * (E + t_pad), E + t_pad, n, P, E, d_w.ptr, E + w_pad,
                                  None if b is None else d_b.ptr, Cc, d_o.ptr)
    assert rc == 0, L.vh_last_error().decode()
    assert L.vh_device_sync() == 0, L.vh_last_error().decode()
    return d_o.to_numpy((n, P, Cc))


def run_labels(pkg, logits, grid, out, want_scores=True):
    """logits [n][GH * GW][C] -> (labels uint8 [n][out_h][out_w], scores); outputs pre-filled with a sentinel"""
    L = pkg.lib()
    n, P, Cc = logits.shape
    assert P == grid[0] * grid[1]
    d_l = dev(pkg, logits)
    d_lab = dev(pkg, np.full(n * out[0] * out[1], 0xEE, np.uint8), np.uint8)
    d_sc = dev(pkg, np.full(n * out[0] * out[1], -7.0, np.float32))
    rc = L.vh_launch_dense_labels(None, d_l.ptr, n, grid[0], grid[1], Cc, out[0], out[1], d_lab.ptr, d_sc.ptr if want_scores else None)
    assert rc == 0, L.vh_last_error().decode()
    assert L.vh_device_sync() == 0, L.vh_last_error().decode()
    return d_lab.to_numpy((n, out[0], out[1])), d_sc.to_numpy((n, out[0], out[1]))


# ---- 1. logits, exact: integers in [-3, 3], every partial sum exact in fp32 (9 * 2048 + 3 < 2^24) ---------------------

# (n, patches, E, C, token padding, weight padding, skipped rows per image): every class-tile count's edge (C = 15, 16, 17,
# 255, 256), ragged E (4, 60), the widest E, one patch, n * patches on both sides of the token tile and across several tiles
# with images changing inside a tile.  With few token tiles (all cases but the last) a workgroup takes 64 labels.
LOGIT_CASES = [
    (1, 1, 4, 2, 0, 0, 0),
    (3, 1, 60, 15, 4, 4, 1),
    (1, TT - 1, 64, 16, 0, 8, 1),
    (1, TT, 64, 17, 4, 0, 0),
    (1, TT + 1, 768, 150, 0, 0, 1),
    (2, TT + 1, 60, 255, 8, 4, 2),
    (3, 100, 2048, 256, 0, 4, 1),
    (5, 9, 768, 21, 4, 0, 1),
    (130, TT, 8, 150, 0, 4, 0),           # more token tiles than half the CUs: a workgroup takes all 150 labels
]


@pytest.mark.parametrize("n,P,E,Cc,t_pad,w_pad,skip", LOGIT_CASES)
def test_logits_exact_on_integers(pkg, device, n, P, E, Cc, t_pad, w_pad, skip):
    rng = np.random.default_rng(1000 * n + P + E + Cc)
    x = rng.integers(-3, 4, size=(n, P, E)).astype(np.float32)
    W = rng.integers(-3, 4, size=(Cc, E)).astype(np.float32)
    b = rng.integers(-3, 4, size=Cc).astype(np.float32)
    x[0, 0], W[Cc - 1] = 0.0, 0.0                                   # zero sums: +0, with and without the bias
    want = x.astype(np.float64) @ W.astype(np.float64).T
    got = run_logits(pkg, x, W, b, t_pad, w_pad, skip)
    assert same(got, (want + b.astype(np.float64) + 0.0).astype(np.float32))
    plain = run_logits(pkg, x, W, None, t_pad, w_pad, skip)
    assert same(plain, (want + 0.0).astype(np.float32))
    # contiguous tokens give the same bits
    assert same(run_logits(pkg, x, W, b), got)


@pytest.mark.parametrize("n,P,E,Cc", [(2, 9, 60, 2), (1, TT + 3, 768, 17), (3, 50, 2048, 32), (1, 5, 64, 15)])
def test_logits_are_the_gallery_scores(pkg, device, n, P, E, Cc):
    """With no bias a patch logit is the gallery search's score of the same two vectors, bit for bit (k = C returns every
    score): real values, so the order of the chain matters"""
    L = pkg.lib()
    rng = np.random.default_rng(E + Cc)
    x = rng.standard_normal((n, P, E)).astype(np.float32)
    W = (rng.standard_normal((Cc, E)) / np.sqrt(E)).astype(np.float32)
    got = run_logits(pkg, x, W, None)
    M = n * P
    d_q, d_r = dev(pkg, x.reshape(M, E)), dev(pkg, W)
    d_ws = pkg.DeviceBuffer(max(L.vh_gallery_workspace(M, Cc, Cc, 0), 16) // 4)
    d_i, d_s = pkg.DeviceBuffer(M * Cc, np.int32), pkg.DeviceBuffer(M * Cc)
    assert L.vh_launch_gallery_topk(None, d_q.ptr, M, E, d_r.ptr, 0, Cc, E, Cc, 0, d_ws.ptr, d_i.ptr, d_s.ptr) == 0, L.vh_last_error().decode()
    assert L.vh_device_sync() == 0
    idx, sc = d_i.to_numpy((M, Cc)), d_s.to_numpy((M, Cc))
    scores = np.empty((M, Cc), np.float32)
    np.put_along_axis(scores, idx.astype(np.int64), sc, axis=1)
    assert same(got.reshape(M, Cc), scores)
    worst = np.abs(got.astype(np.float64) - dr.logits64(x, W)) / ((E + 8) * dr.U * dr.absdot(x, W))
    print(f"logits n={n} P={P} E={E} C={Cc}: worst |error| / bound = {worst.max():.4f}")
    assert worst.max() <= 1.0


# ---- 2. labels, exact: integer logits in [-8, 8], out = grid * s (s = 1, 2, 4, 16) or grid / 2 per axis ----------------

# (n, grid, C, out): lerp weights are multiples of 1/32, values of 1/1024: every operation of the header's expressions is
# exact.  1x1 and 1x5 grids, the 76 KB of LDS of 37 x 37 x 256, out_w = 1, 3, 15, 16, 17, 224 (odd widths move the rows'
# alignment from image to image and row to row), more than 256 columns, bands of 24 rows (two register chunks), empty and
# one-row bands
LABEL_CASES = [
    (2, (1, 1), 256, (1, 1)),
    (2, (1, 1), 5, (16, 16)),
    (3, (1, 5), 7, (4, 20)),
    (1, (1, 5), 256, (2, 10)),
    (1, (3, 5), 256, (3, 5)),
    (2, (2, 2), 256, (1, 1)),
    (2, (2, 2), 3, (32, 8)),
    (2, (2, 3), 9, (4, 3)),
    (2, (3, 5), 17, (6, 10)),
    (3, (3, 5), 2, (3, 5)),
    (2, (2, 15), 16, (2, 15)),
    (1, (4, 30), 4, (2, 15)),
    (3, (3, 17), 15, (12, 17)),
    (1, (14, 14), 21, (224, 224)),
    (1, (14, 14), 256, (28, 28)),
    (2, (14, 14), 150, (7, 7)),
    (1, (37, 37), 256, (37, 37)),
    (1, (37, 37), 256, (74, 74)),
    (1, (2, 37), 3, (4, 592)),
]


def integer_logits(n, grid, Cc, seed):
    """integers in [-8, 8] (ties everywhere), 3 % of the entries NaN, +inf, -inf or -0, one patch all NaN, and from C = 5 on
    whole columns of NaN, +inf and -inf"""
    rng = np.random.default_rng(seed)
    P = grid[0] * grid[1]
    L = rng.integers(-8, 9, size=(n, P, Cc)).astype(np.float32)
    hit = rng.random(L.shape) < 0.03
    L[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0], np.float32), size=int(hit.sum()))
    L[n - 1, P // 2] = np.nan
    if Cc >= 5:
        L[:, :, 1], L[:, :, 2], L[:, :, Cc - 1] = np.nan, np.inf, -np.inf
        L[0, :, 2] = 8.0                                            # image 0 keeps a finite winner in most pixels
    return L


@pytest.mark.parametrize("n,grid,Cc,out", LABEL_CASES)
def test_labels_exact_on_integers(pkg, device, n, grid, Cc, out):
    L = integer_logits(n, grid, Cc, 7 * n + grid[1] + Cc + out[1])
    want_lab, want_bits = dr.dense32(L, grid, out)
    lab, sc = run_labels(pkg, L, grid, out)
    assert np.array_equal(lab, want_lab)
    assert np.array_equal(bits(sc), want_bits)
    only, untouched = run_labels(pkg, L, grid, out, want_scores=False)
    assert np.array_equal(only, lab) and (untouched == -7.0).all()
    # plain integers, no special values: the float64 definition itself
    Li = np.random.default_rng(Cc).integers(-8, 9, size=L.shape).astype(np.float32)
    lab, sc = run_labels(pkg, Li, grid, out)
    v = dr.upsample64(Li.astype(np.float64), grid, out)
    assert np.array_equal(lab, dr.rank_first(v)) and same(sc, v.max(axis=-1).astype(np.float32))


# ---- 3. real values ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", dr.FLOAT_CASES, ids=lambda c: f"E{c[1]}-C{c[2]}-{c[3][0]}x{c[3][1]}-to-{c[4][0]}x{c[4][1]}")
def test_real_values_hold_the_check(pkg, device, case):
    """Both launchers on gaussian tokens and heads: every pixel's label is one the float64 definition admits within the
    header's bound, every score within it.  Measured worst |error| / bound on an MI355X, in the order of the cases: 0.145,
    0.034, 0.027, 0.171, 0.029 (E = 60 .. 128, where the coordinate term is most of the bound), 0.0036 (E = 768); on the
    model's tokens (test_against_the_feature_output) 0.004-0.006.  The bound is the worst case of E roundings of one sign."""
    n, E, Cc, grid, out, bias, seed = case
    x, W, b = dr.float_case(*case)
    pl = run_logits(pkg, x, W, b)
    lab, sc = run_labels(pkg, pl, grid, out)
    worst, share = dr.check(x, W, b, grid, out, lab, sc)
    print(f"dense {case[:5]}: worst |error| / bound = {worst:.4f}, {100 * share:.3f} % of the pixels admit more than one label")
    assert share <= 0.01


# ---- 4. refusals ------------------------------------------------------------------------------------------------------

def test_launcher_refusals(pkg, device):
    L = pkg.lib()
    n, grid, E, Cc, out = 2, (3, 4), 64, 6, (9, 10)
    P = grid[0] * grid[1]
    x, W, b = dr.float_case(n, E, Cc, grid, out, True, 1)
    d_x, d_w, d_b = dev(pkg, x), dev(pkg, W), dev(pkg, b)
    d_pl = dev(pkg, np.full(n * P * 256, -7.0, np.float32))
    d_lab = dev(pkg, np.full(n * out[0] * out[1] + 64, 0xEE, np.uint8), np.uint8)
    d_sc = dev(pkg, np.full(n * out[0] * out[1] + 64, -7.0, np.float32))
    off = lambda d, by: C.c_void_p(d.ptr.value + by)
    good = dict(rows=d_x.ptr, istride=P * E, rstride=E, n=n, P=P, E=E, w=d_w.ptr, wstride=E, b=d_b.ptr, C=Cc, pl=d_pl.ptr)

    def logits(**kw):
        a = dict(good)
        a.update(kw)
        return L.vh_launch_dense_logits(None, a["rows"], a["istride"], a["rstride"], a["n"], a["P"], a["E"], a["w"], a["wstride"], a["b"],
                                        a["C"], a["pl"])

    bad = [dict(C=1), dict(C=257), dict(E=0), dict(E=62), dict(E=2052, rstride=2052, wstride=2052, istride=P * 2052), dict(n=0), dict(P=0),
           dict(n=2 ** 20, P=2 ** 11), dict(wstride=60), dict(wstride=66), dict(rstride=60), dict(rstride=66, istride=P * 66),
           dict(istride=P * E - 4), dict(istride=P * E + 2), dict(rows=None), dict(w=None), dict(pl=None), dict(rows=off(d_x, 4)),
           dict(w=off(d_w, 8)), dict(b=off(d_b, 4)), dict(pl=off(d_pl, 4))]
    for kw in bad:
        L.vh_set_error(1, b"stale")
        assert logits(**kw) == 1, kw
        msg = L.vh_last_error().decode()
        assert msg.startswith("vh_launch_dense_logits: ") and len(msg) > 30, (kw, msg)

    good2 = dict(pl=d_pl.ptr, n=n, gh=grid[0], gw=grid[1], C=Cc, oh=out[0], ow=out[1], lab=d_lab.ptr, sc=d_sc.ptr)

    def labels(**kw):
        a = dict(good2)
        a.update(kw)
        return L.vh_launch_dense_labels(None, a["pl"], a["n"], a["gh"], a["gw"], a["C"], a["oh"], a["ow"], a["lab"], a["sc"])

    bad = [dict(C=1), dict(C=257), dict(gh=0), dict(gw=0), dict(gh=65), dict(gw=65), dict(oh=0), dict(ow=0), dict(oh=4097), dict(ow=4097),
           dict(n=0), dict(pl=None), dict(lab=None), dict(pl=off(d_pl, 4)), dict(lab=off(d_lab, 1)), dict(lab=off(d_lab, 8)),
           dict(sc=off(d_sc, 4))]
    for kw in bad:
        L.vh_set_error(1, b"stale")
        assert labels(**kw) == 1, kw
        msg = L.vh_last_error().decode()
        assert msg.startswith("vh_launch_dense_labels: ") and len(msg) > 30, (kw, msg)
    assert L.vh_device_sync() == 0
    assert (d_pl.to_numpy() == -7.0).all() and (d_lab.to_numpy() == 0xEE).all() and (d_sc.to_numpy() == -7.0).all()
    assert logits() == 0 and labels() == 0 and labels(sc=None) == 0 and L.vh_device_sync() == 0
    m = n * out[0] * out[1]
    dr.check(x, W, b, grid, out, d_lab.to_numpy()[:m].reshape(n, *out), d_sc.to_numpy()[:m].reshape(n, *out))
    assert (d_lab.to_numpy()[m:] == 0xEE).all() and (d_sc.to_numpy()[m:] == -7.0).all() and (d_pl.to_numpy()[n * P * Cc:] == -7.0).all()


# ---- 5. the model -----------------------------------------------------------------------------------------------------

NL = 21


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
def head(pkg, device):
    """a head of 21 labels over 768 columns, rows 772 apart, on the device once"""
    rng = np.random.default_rng(23)
    W = (rng.standard_normal((NL, 768)) / np.sqrt(768)).astype(np.float32)
    b = (0.1 * rng.standard_normal(NL)).astype(np.float32)
    padded = np.full((NL, 772), np.nan, np.float32)
    padded[:, :768] = W
    return W, b, dev(pkg, padded), dev(pkg, b)


def spec_for(pkg, head, out=(0, 0), tap=-1, final_norm=True, bias=True):
    return pkg.binding.DenseSpec(NL, out[0], out[1], tap, final_norm, 772, head[2], head[3] if bias else None)


def armed_device(pkg, model, images, spec, call=None, extras=True):
    """forward_device with `spec` armed -> (labels, scores, patch_logits, logits, probs); what lies beyond n keeps the fill"""
    n = images.shape[0] if call is None else call[1]
    nc, mb, P = model.cfg.num_classes, model.max_batch, model.tokens - 1
    H, Wd = spec.out_h or model.cfg.img_size, spec.out_w or model.cfg.img_size
    d_lab = dev(pkg, np.full(mb * H * Wd, 0xEE, np.uint8), np.uint8)
    d_sc, d_pl = dev(pkg, np.full(mb * H * Wd, -7.0, np.float32)), dev(pkg, np.full(mb * P * NL, -7.0, np.float32))
    d_l, d_p = pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)
    model.set_dense(spec, spec.d_weight, spec.d_bias, labels=d_lab, scores=d_sc if extras else None, patch_logits=d_pl if extras else None)
    try:
        if call is None:
            d_img = pkg.DeviceBuffer.from_numpy(images)
            model.forward_device(d_img.ptr, n, d_l.ptr, d_p.ptr)
        else:
            call[0](d_l, d_p)
        model.sync()
    finally:
        model.set_dense(None)
    lab, sc, pl = d_lab.to_numpy((mb, H, Wd)), d_sc.to_numpy((mb, H, Wd)), d_pl.to_numpy((mb, P, NL))
    assert (lab[n:] == 0xEE).all() and (sc[n:] == -7.0).all() and (pl[n:] == -7.0).all()
    if not extras:
        assert (sc == -7.0).all() and (pl == -7.0).all()
    return lab[:n], sc[:n], pl[:n], d_l.to_numpy((n, nc)), d_p.to_numpy((n, nc))


def plain_device(pkg, model, images):
    n, nc = images.shape[0], model.cfg.num_classes
    d_img = pkg.DeviceBuffer.from_numpy(images)
    d_l, d_p = pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)
    model.forward_device(d_img.ptr, n, d_l.ptr, d_p.ptr)
    model.sync()
    return d_l.to_numpy((n, nc)), d_p.to_numpy((n, nc))


def tokens_of(pkg, model, images, tap, final_norm):
    """the feature output's patch tokens [n][T - 1][E], fp32, NLC (the device form: the host form does not carry tokens)"""
    n, P, E = images.shape[0], model.tokens - 1, model.cfg.embed_dim
    d_tok, d_img = pkg.DeviceBuffer(model.max_batch * P * E), pkg.DeviceBuffer.from_numpy(images)
    model.set_features(pkg.binding.FeatureSpec((tap,), final_norm), tokens=d_tok)
    try:
        model.forward_device(d_img.ptr, n, None, None)
        model.sync()
    finally:
        model.set_features(None)
    return d_tok.to_numpy((model.max_batch, P, E))[:n].copy()


MODEL_CASES = [("f32", -1, True, (0, 0)), ("f32", 5, False, (37, 50)), ("f32", -1, False, (37, 50)), ("f32", 5, True, (0, 0)),
               ("bf16", -1, True, (0, 0)), ("bf16", 5, False, (37, 50)), ("fp8", -1, True, (37, 50)), ("fp8", 5, False, (0, 0))]


@pytest.mark.parametrize("precision,tap,final_norm,out", MODEL_CASES)
def test_against_the_feature_output(pkg, models, images19, head, precision, tap, final_norm, out):
    """The token rows are the feature output's own bits: the two launchers on the tokens a feature request writes give the
    armed labels, scores and patch logits bit for bit; `check` holds on them; logits and probabilities do not move; asking
    for labels alone gives the same labels."""
    model = models(precision)
    W, b, _, _ = head
    imgs = images19[:8]
    spec = spec_for(pkg, head, out, tap, final_norm)
    lab, sc, pl, logits, probs = armed_device(pkg, model, imgs, spec)
    tok = tokens_of(pkg, model, imgs, tap, final_norm)
    size = (out[0] or 224, out[1] or 224)
    pl2 = run_logits(pkg, tok, W, b)
    lab2, sc2 = run_labels(pkg, pl2, (14, 14), size)
    assert same(pl, pl2) and same(lab, lab2) and same(sc, sc2)
    worst, share = dr.check(tok, W, b, (14, 14), size, lab, sc)
    print(f"{precision} tap {tap} norm {final_norm}: worst |error| / bound = {worst:.4f}, {100 * share:.2f} % ambiguous")
    l0, p0 = plain_device(pkg, model, imgs)
    assert same(logits, l0) and same(probs, p0)
    only = armed_device(pkg, model, imgs, spec, extras=False)
    assert same(only[0], lab) and same(only[3], l0)
    nb = armed_device(pkg, model, imgs[:2], spec_for(pkg, head, out, tap, final_norm, bias=False))
    assert same(nb[2], run_logits(pkg, tok[:2], W, None))


@pytest.mark.parametrize("precision", ["f32", "bf16", "fp8"])
def test_nothing_else_moves(pkg, models, images19, head, precision):
    """Features, top-k, attention maps, rollout and a gallery armed: all their outputs, the logits and the probabilities
    are the same bits with a dense request armed beside them (all six in one forward), and after it is disarmed; an
    un-armed forward launches what it launched before."""
    model, b = models(precision), pkg.binding
    imgs, n, k, E, T, H = images19[:5], 5, 5, model.cfg.embed_dim, model.tokens, model.cfg.num_heads
    rows = gr.bf16_decode(gr.bf16_round(np.random.default_rng(17).standard_normal((300, E)).astype(np.float32)))
    d_rows = dev(pkg, rows)

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
    d_gi, d_gs = pkg.DeviceBuffer(8 * k, np.int32), pkg.DeviceBuffer(8 * k)
    d_img, d_l, d_p = pkg.DeviceBuffer.from_numpy(imgs), pkg.DeviceBuffer(n * 1000), pkg.DeviceBuffer(n * 1000)
    outputs = (d_cls, d_pool, d_lab, d_sc, d_h, d_m, d_r, d_gi, d_gs, d_l, d_p)

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
    model.set_gallery(b.GallerySpec(k, "pooled", -1, True, True, "f32", 300, E, d_rows), d_rows, indices=d_gi, scores=d_gs)
    try:
        want = others()
        assert want[4].any() and want[6].any() and want[8].any()
        alone = armed_device(pkg, models(precision), imgs, spec_for(pkg, head, (40, 33)))      # disarms the dense request only
        d_dl, d_ds = dev(pkg, np.zeros(8 * 40 * 33, np.uint8), np.uint8), pkg.DeviceBuffer(8 * 40 * 33)
        spec = spec_for(pkg, head, (40, 33))
        model.set_dense(spec, spec.d_weight, spec.d_bias, labels=d_dl, scores=d_ds)
        armed = others()
        assert same(d_dl.to_numpy((8, 40, 33))[:n], alone[0]) and same(d_ds.to_numpy((8, 40, 33))[:n], alone[1])
        with_all = counts()
        model.set_dense(None)
        after = others()
        for w, a, c in zip(want, armed, after):
            assert same(w, a) and same(w, c)
        # the readout, the logits and the labels, timed with the classifier; without final_norm no readout
        plain = counts()
        assert with_all["head_gemm"] == plain["head_gemm"] + 3
        assert all(with_all[o] == plain[o] for o in plain if o != "head_gemm")
        spec = spec_for(pkg, head, (40, 33), 5, False)
        model.set_dense(spec, spec.d_weight, spec.d_bias, labels=d_dl)
        assert counts()["head_gemm"] == plain["head_gemm"] + 2
        model.set_dense(None)
    finally:
        for disarm in (model.set_features, model.set_topk, model.set_attention, model.set_rollout, model.set_gallery, model.set_dense):
            disarm(None)
    assert counts() == before


def test_batch_position_independence(pkg, models, images19, head):
    order = np.array([0, 1, 2, 4, 5, 3, 6, 7])                       # image 3 at position 5 of 8
    for precision in ("f32", "bf16"):
        model = models(precision)
        for tap, final_norm in ((-1, True), (5, False)):
            spec = spec_for(pkg, head, (56, 75), tap, final_norm)
            o8 = armed_device(pkg, model, images19[order], spec)
            o1 = armed_device(pkg, model, images19[3:4], spec)
            for a8, a1 in zip(o8[:3], o1[:3]):
                assert same(a8[5:6], a1), (precision, tap)
            assert not same(o8[2][4:5], o1[2])


def test_forms_and_entry_points(pkg, device, models, cfg, images19, head):
    W, b, d_w, d_b = head
    model = models("f32")
    # host form, 19 images through max_batch 8 (chunks of 8, 8 and 3), against the device form; ViTHip.segment
    for tap, final_norm, out in ((-1, True, (0, 0)), (3, False, (30, 41))):
        spec = spec_for(pkg, head, out, tap, final_norm)
        devs = [armed_device(pkg, model, images19[a:a + 8], spec) for a in (0, 8, 16)]
        size = (out[0] or 224, out[1] or 224)
        hl = np.full((19,) + size, 0xEE, np.uint8)
        model.set_dense_host(spec_for(pkg, head, out, tap, final_norm), d_w, d_b, labels=hl)
        try:
            logits, _ = model.forward(images19)
        finally:
            model.set_dense_host(None)
        assert same(hl, np.concatenate([d[0] for d in devs])) and same(logits, np.concatenate([d[3] for d in devs]))
        seg = model.segment(images19, W, b, size=size, tap=tap, final_norm=final_norm)     # contiguous rows of 768: the same bits
        assert seg.dtype == np.uint8 and same(seg, hl)
    assert same(model.segment(images19[:3], W, b), model.segment(images19[:3], W, b, size=224))
    nb = model.segment(images19[:3], W, None, size=(30, 41))
    assert same(nb, armed_device(pkg, model, images19[:3], spec_for(pkg, head, (30, 41), bias=False))[0])
    # 8-bit, resized and box entry points against the fp32 one fed the same normalised crops
    n, S = 3, cfg.img_size
    rng = np.random.default_rng(3)
    norm = pkg.pixel_norm(MEAN, STD)
    sources = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in ((300, 260), (224, 224), (257, 401))]
    d_src = [pkg.DeviceBuffer.from_numpy(a, dtype=np.uint8) for a in sources]
    descs = [(d.ptr.value, a.shape[0], a.shape[1], a.shape[1] * 3) for d, a in zip(d_src, sources)]
    d_crops = pkg.DeviceBuffer(n * S * S * 3, dtype=np.uint8)
    scale, bias = np.array(norm.scale[:3], dtype=np.float32), np.array(norm.bias[:3], dtype=np.float32)
    spec = spec_for(pkg, head, (61, 47), -1, True)

    def normalised():
        u8 = d_crops.to_numpy((n, S, S, 3))
        return u8, np.ascontiguousarray(((u8.astype(np.float32) * scale).astype(np.float32) + bias).astype(np.float32).transpose(0, 3, 1, 2))

    def host(call):
        hl = np.full((n, 61, 47), 0xEE, np.uint8)
        model.set_dense_host(spec, d_w, d_b, labels=hl)
        try:
            logits, _ = call()
        finally:
            model.set_dense_host(None)
        return hl, logits

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
        hl, logits = host(call)
        assert same(hl, want[0]) and same(logits, want[3])
    boxes = [(0, (10.0, 20.0, 250.0, 290.0)), (2, (0.0, 0.0, 401.0, 257.0)), (2, (100.5, 30.25, 300.0, 200.0))]
    model.crop_boxes_u8(descs, boxes, d_crops.ptr, filter="bicubic")
    model.sync()
    _, f32 = normalised()
    want = armed_device(pkg, model, f32, spec)
    got = armed_device(pkg, model, None, spec,
                       call=(lambda d_l, d_p: model.forward_device_u8_boxes(descs, boxes, norm, "bicubic", "hwc", d_l.ptr, d_p.ptr), n))
    for a, w in zip(got, want):
        assert same(a, w)
    hl, logits = host(lambda: model.forward_u8_boxes(sources, boxes, "bicubic", norm))
    assert same(hl, want[0]) and same(logits, want[3])


def test_cls_only_last_gives_equal_bits(pkg, models, images19, head):
    model = models("f32")
    imgs = images19[:4]
    try:
        off = {t: armed_device(pkg, model, imgs, spec_for(pkg, head, (37, 50), t)) for t in (-1, 5)}
        model.set_last_layer_cls_only(True)
        for t in (-1, 5):
            for a, w in zip(armed_device(pkg, model, imgs, spec_for(pkg, head, (37, 50), t)), off[t]):
                assert same(a, w), t
        l0, p0 = plain_device(pkg, model, imgs)
        assert same(l0, off[-1][3]) and same(p0, off[-1][4])
    finally:
        model.set_last_layer_cls_only(False)


def test_arming_rules(pkg, device, models, images19, head):
    model, b, L = models("f32"), pkg.binding, pkg.lib()
    W, bias, d_w, d_b = head
    n, nc, out = 2, 1000, (20, 30)
    imgs = images19[:n]
    spec = spec_for(pkg, head, out)
    want_lab, want_sc, _, l0, _ = armed_device(pkg, model, imgs, spec)
    d_img, d_l = pkg.DeviceBuffer.from_numpy(imgs), pkg.DeviceBuffer(n * nc)
    d_lab, d_sc = dev(pkg, np.zeros(8 * 600, np.uint8), np.uint8), pkg.DeviceBuffer(8 * 600)
    model.set_dense(spec, d_w, d_b, labels=d_lab, scores=d_sc)
    try:
        # device form armed: the host forms refuse
        with pytest.raises(b.VitHipError, match="vit_hip_set_dense"):
            model.forward(imgs)
        assert "dense" in L.vh_last_error().decode()
        # refused re-arms keep the request
        cs = spec.c_struct()
        bufs = lambda lab, sc=None, pl=None: C.byref(b.DenseBuffers(lab, sc, pl))
        assert L.vit_hip_set_dense(model.ctx, C.byref(cs), bufs(d_lab.ptr.value + 4, d_sc.ptr)) == 1
        assert "aligned" in L.vh_last_error().decode()
        assert L.vit_hip_set_dense(model.ctx, C.byref(cs), bufs(None, d_sc.ptr)) == 1
        assert "labels" in L.vh_last_error().decode()
        assert L.vit_hip_set_dense(model.ctx, C.byref(cs), None) == 1
        host_lab = np.zeros((n,) + out, np.uint8)
        host_sc = np.zeros((n,) + out, np.float32)
        assert L.vit_hip_set_dense_host(model.ctx, C.byref(cs), bufs(host_lab.ctypes.data, host_sc.ctypes.data)) == 1
        assert "labels only" in L.vh_last_error().decode()
        assert L.vit_hip_set_dense_host(model.ctx, C.byref(cs), bufs(host_lab.ctypes.data, None, host_sc.ctypes.data)) == 1
        for field, value, word in (("n_labels", 1, "n_labels"), ("n_labels", 257, "n_labels"), ("tap", 12, "tap"), ("out_h", 4097, "out_h"),
                                   ("out_w", -1, "out_h"), ("weight_stride", 764, "weight_stride"), ("weight_stride", 770, "weight_stride"),
                                   ("d_weight", None, "weight"), ("d_weight", d_w.ptr.value + 4, "aligned"),
                                   ("d_bias", d_b.ptr.value + 4, "aligned")):
            bad = spec.c_struct()
            setattr(bad, field, value)
            for entry, lab in ((L.vit_hip_set_dense, d_lab.ptr), (L.vit_hip_set_dense_host, host_lab.ctypes.data)):
                assert entry(model.ctx, C.byref(bad), bufs(lab)) == 1, field
                msg = L.vh_last_error().decode()
                assert msg.startswith("vit_hip_set_dense") and word in msg, (field, msg)
        model.forward_device(d_img.ptr, n, d_l.ptr)
        model.sync()
        assert same(d_lab.to_numpy((8,) + out)[:n], want_lab) and same(d_sc.to_numpy((8,) + out)[:n], want_sc)
        assert same(d_l.to_numpy((n, nc)), l0)
        # host form armed (which disarms the device form): the device forms refuse, nothing is launched
        model.set_dense_host(spec_for(pkg, head, out), d_w, d_b, labels=host_lab)
        sentinel = np.full(n * nc, -7.0, np.float32)
        assert L.vh_h2d(d_l.ptr, sentinel.ctypes.data_as(C.c_void_p), sentinel.nbytes, None) == 0
        assert L.vh_memset(d_lab.ptr, 0, d_lab.count, None) == 0
        assert L.vit_hip_forward_device(model.ctx, d_img.ptr, n, d_l.ptr, None, None) == 1
        assert "vit_hip_set_dense_host" in L.vh_last_error().decode()
        model.sync()
        assert np.array_equal(d_l.to_numpy(), sentinel) and not d_lab.to_numpy().any()
        hl, _ = model.forward(imgs)
        assert same(host_lab, want_lab) and same(hl, l0)
    finally:
        model.set_dense_host(None)
        model.set_dense(None)
    # disarmed: a forward writes nothing; armed and disarmed several times over, then used (scratch is freed and made anew)
    assert L.vh_memset(d_lab.ptr, 0, d_lab.count, None) == 0
    model.forward_device(d_img.ptr, n, d_l.ptr)
    model.sync()
    assert not d_lab.to_numpy().any()
    for _ in range(3):
        model.set_dense(spec, d_w, d_b, labels=d_lab)
        model.set_dense(None)
    model.set_dense(spec, d_w, d_b, labels=d_lab)
    try:
        model.forward_device(d_img.ptr, n, d_l.ptr)
        model.sync()
        assert same(d_lab.to_numpy((8,) + out)[:n], want_lab)
    finally:
        model.set_dense(None)


def test_long_sequence_model(pkg, device, head):
    """vit_b_16_384 cut to two layers (T = 577, a 24 x 24 grid, the plan's long-sequence attention), two images, 384 x 384
    labels: the armed outputs are the launchers' on the feature output's tokens, logits bit-identical to un-armed"""
    W, b, _, _ = head
    cfg = pkg.preset("vit_b_16_384")
    full = pkg.synth_weights(cfg, 0)
    cfg.depth = 2
    weights = full[:4 + 12 * 2] + full[-4:]
    imgs = pkg.synth_images(cfg, 0, 2)
    model = pkg.ViTHip(cfg, weights, device=0, max_batch=2)
    try:
        assert model.tokens == 577
        l0, p0 = plain_device(pkg, model, imgs)
        lab, sc, pl, l1, p1 = armed_device(pkg, model, imgs, spec_for(pkg, head))
        assert lab.shape == (2, 384, 384) and same(l1, l0) and same(p1, p0)
        tok = tokens_of(pkg, model, imgs, -1, True)
        pl2 = run_logits(pkg, tok, W, b)
        lab2, sc2 = run_labels(pkg, pl2, (24, 24), (384, 384))
        assert same(pl, pl2) and same(lab, lab2) and same(sc, sc2)
        worst, share = dr.check(tok, W, b, (24, 24), (384, 384), lab, sc)
        print(f"b16_384: worst |error| / bound = {worst:.4f}, {100 * share:.2f} % ambiguous")
    finally:
        model.close()
