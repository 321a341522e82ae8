"""The soft maps of the dense head on the GPU (vh_launch_dense_soft, csrc/dense_soft.hip; vit_hip_set_dense_soft;
ViTHip.segment_soft), against tests/dense_soft_ref.py.  At the launcher, on patch logits uploaded directly: the sharp tier,
where the per-pixel values v are known to the bit (out == grid for any floats; integer logits under dyadic ratios) and the
kernel's own arithmetic is held to the header's (C + K) u; the band and column edges under the combined bound; output
subsets, special values, refusals.  Through the model: the armed maps are the launcher's on the patch logits the same
forward wrote, nothing else moves, the launch counts, chunking, the class-rows last layer.

Measured on an MI355X, worst |error| / bound over the sharp tier (every pixel of every case): prob 0.121, expect 0.060,
entropy 0.026 (profiles/dense_soft_errors.txt has them per class count); at the edges, against the combined bound, 0.027 at most."""
import ctypes as C

import numpy as np
import pytest

import dense_ref as dr
import dense_soft_ref as sr
import gallery_ref as gr
from test_gpu_dense import dev, same

pytestmark = pytest.mark.gpu

FILL = -7.0
WORST = {}           # (tier, C) -> {map: worst |error| / bound so far}: what the sharp tests print


def run_soft(pkg, L, grid, out, s, values=None, which=sr.NAMES, d_logits=None):
    """L [n][GH * GW][C] fp32 -> {name: [n][out_h][out_w] fp32} for the maps in `which`, every buffer pre-filled with FILL and
    one image longer than the launch writes; a map not asked for must keep the fill"""
    lib = pkg.lib()
    n, P, Cc = L.shape
    assert P == grid[0] * grid[1]
    d_l = d_logits if d_logits is not None else dev(pkg, L)
    m = n * out[0] * out[1]
    bufs = {name: dev(pkg, np.full(m + out[0] * out[1], FILL, np.float32)) for name in sr.NAMES}
    d_v = dev(pkg, values) if "expect" in which else None
    ptr = lambda name: bufs[name].ptr if name in which else None
    rc = lib.vh_launch_dense_soft(None, d_l.ptr, n, grid[0], grid[1], Cc, out[0], out[1], s, None if d_v is None else d_v.ptr, ptr("prob"),
                                  ptr("expect"), ptr("entropy"))
    assert rc == 0, lib.vh_last_error().decode()
    assert lib.vh_device_sync() == 0, lib.vh_last_error().decode()
    got = {}
    for name in sr.NAMES:
        a = bufs[name].to_numpy()
        assert (a[m:] == FILL).all(), f"{name}: written past the last image"
        if name in which:
            got[name] = a[:m].reshape(n, *out)
        else:
            assert (a == FILL).all(), f"{name}: written though not asked for"
    return got


def note(tier, Cc, worst):
    have = WORST.setdefault((tier, Cc), dict.fromkeys(sr.NAMES, 0.0))
    for k, v in worst.items():
        have[k] = max(have[k], v)


# ---- 1. the sharp tier: v is exact ------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cc", sr.SHARP_C)
@pytest.mark.parametrize("grid", sr.SHARP_GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_sharp_out_equals_grid(pkg, device, grid, Cc):
    """out == grid: every lerp weight is 0 and v is the logit's own bits, for any floats.  Spreads 0 (all classes equal: prob
    = 1 / C to the bit, entropy = ln C), 1, 8 and 60 (terms that underflow), three scales, values of mixed sign"""
    values = sr.values_for(Cc)
    for spread in sr.SPREADS:
        L = sr.spread_logits(2, grid, Cc, spread, int(10 * spread) + Cc)
        v = sr.v32(L, grid, grid)
        d_l = dev(pkg, L)
        for s in sr.SCALES:
            got = run_soft(pkg, L, grid, grid, s, values, d_logits=d_l)
            worst = sr.check_sharp(v, s, values, got, f"C={Cc} grid={grid} spread={spread} s={s}")
            note("out == grid", Cc, worst)
            if spread == 0.0:
                assert same(got["prob"], np.full_like(got["prob"], np.float32(1.0) / np.float32(Cc)))
    print(f"sharp, out == grid {grid}, C={Cc}: worst |error| / bound " + ", ".join(f"{k} {v:.4f}" for k, v in WORST[("out == grid", Cc)].items()))


@pytest.mark.parametrize("Cc", sr.SHARP_C)
@pytest.mark.parametrize("grid,out", sr.DYADIC, ids=lambda g: f"{g[0]}x{g[1]}")
def test_sharp_dyadic_ratios(pkg, device, grid, out, Cc):
    """integer logits in +-512 under 4 -> 16 and (2, 3) -> (16, 24): every operation of the three lerps is exact and
    dense_ref.dense32's expressions give v's bits"""
    values = sr.values_for(Cc, 1)
    L = sr.integer_logits(2, grid, Cc, 31 * Cc + out[1])
    v = sr.v32(L, grid, out)
    for s in sr.SCALES + [1.0 / 64]:            # 1 / 64: the classes stay within a few units of each other
        worst = sr.check_sharp(v, s, values, run_soft(pkg, L, grid, out, s, values), f"C={Cc} {grid}->{out} s={s}")
        note("dyadic", Cc, worst)
    print(f"sharp, dyadic {grid}->{out}, C={Cc}: worst |error| / bound " + ", ".join(f"{k} {v:.4f}" for k, v in WORST[("dyadic", Cc)].items()))


# ---- 2. band and column edges, under the combined bound ---------------------------------------------------------------

@pytest.mark.parametrize("grid,out,Cc", sr.EDGE_CASES, ids=lambda a: "x".join(map(str, a)) if isinstance(a, tuple) else f"C{a}")
def test_band_and_column_edges(pkg, device, grid, out, Cc):
    """n = 3 with image 0 again at position 2 (the same bits at both positions) and n = 1 (the same bits again)"""
    L = sr.spread_logits(3, grid, Cc, 8.0, 7 * Cc + out[1])
    L[2] = L[0]
    values = sr.values_for(Cc, 2)
    for s in (1.0, 3.0):
        got = run_soft(pkg, L, grid, out, s, values)
        worst = sr.check_combined(L, grid, out, s, values, got, f"{grid}->{out} C={Cc} s={s}")
        print(f"edges {grid}->{out} C={Cc} s={s}: worst |error| / combined bound " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
        one = run_soft(pkg, L[:1], grid, out, s, values)
        for name in sr.NAMES:
            assert same(got[name][2], got[name][0]) and same(one[name][0], got[name][0]), name
            assert not same(got[name][1], got[name][0])


# ---- 3. output subsets, special values, refusals ----------------------------------------------------------------------

def test_each_map_alone_gives_the_same_bits(pkg, device):
    for grid, out, Cc in (((3, 5), (20, 37), 21), ((2, 2), (34, 34), 150)):
        L = sr.spread_logits(2, grid, Cc, 8.0, Cc)
        values = sr.values_for(Cc)
        full = run_soft(pkg, L, grid, out, 1.0, values)
        for which in (("prob",), ("expect",), ("entropy",), ("prob", "entropy"), ("expect", "entropy"), ("prob", "expect")):
            part = run_soft(pkg, L, grid, out, 1.0, values, which=which)
            assert set(part) == set(which)
            for name in which:
                assert same(part[name], full[name]), (which, name)


def test_special_values(pkg, device):
    """integer logits, (2, 2) -> (8, 8): image 0 has a NaN class, image 1 a +inf class, image 2 nothing but -inf, image 3 one
    class of -inf beside finite ones, image 4 one NaN logit at patch (0, 0).  A pixel with a NaN v (an infinity under a zero
    weight is one, as at the clamped edges) or an infinite maximum is 0x7FC00000 in all three maps; elsewhere a -inf
    contributes nothing and the maps hold the sharp bounds"""
    grid, out, Cc = (2, 2), (8, 8), 5
    L = sr.integer_logits(5, grid, Cc, 9) / np.float32(64.0)
    L[0, :, 1] = np.nan
    L[1, :, 2] = np.inf
    L[2] = -np.inf
    L[3, :, 0] = -np.inf
    L[4, 0, 4] = np.nan
    values = sr.values_for(Cc)
    v = sr.v32(L, grid, out)
    got = run_soft(pkg, L, grid, out, 1.0, values)
    p, x, h, av = sr.soft64(v, 1.0, values)
    bad = np.isnan(p)
    # columns and rows 0 and 1 are clamped to the first patch with a zero weight on the second; patch (0, 0) is a corner of
    # the pixels whose cell is (0, 0): rows and columns 0..5
    assert bad[:3].all() and bad[3, :2].all() and bad[3, :, :2].all() and not bad[3, 2:, 2:].any()
    assert bad[4, :6, :6].all() and not bad[4, 6:].any() and not bad[4, :, 6:].any()
    bp, bx, bh = sr.sharp_bounds(Cc, p, av)
    for name, ref, bnd in (("prob", p, bp), ("expect", x, bx), ("entropy", h, bh)):
        assert (got[name].view(np.uint32)[bad] == sr.NAN_BITS).all(), name
        assert np.isfinite(got[name][~bad]).all() and (np.abs(got[name][~bad].astype(np.float64) - ref[~bad]) <= bnd[~bad]).all(), name
    # the -inf class contributes nothing: image 3 without it gives the same interior bits
    rest = run_soft(pkg, np.ascontiguousarray(L[3:4, :, 1:]), grid, out, 1.0, values[1:])
    for name in sr.NAMES:
        assert same(rest[name][0, 2:, 2:], got[name][3, 2:, 2:]), name


def test_launcher_refusals_leave_the_buffers(pkg, device):
    lib = pkg.lib()
    n, grid, Cc, out = 2, (3, 4), 6, (9, 10)
    L = sr.spread_logits(n, grid, Cc, 8.0, 1)
    values = sr.values_for(Cc)
    m = n * out[0] * out[1]
    d_l, d_v = dev(pkg, L), dev(pkg, values)
    d_p, d_x, d_h = (dev(pkg, np.full(m + 64, FILL, np.float32)) for _ in range(3))
    off = lambda d, by: C.c_void_p(d.ptr.value + by)
    good = dict(pl=d_l.ptr, n=n, gh=grid[0], gw=grid[1], C=Cc, oh=out[0], ow=out[1], s=1.0, values=d_v.ptr, prob=d_p.ptr, expect=d_x.ptr,
                entropy=d_h.ptr)

    def soft(**kw):
        a = dict(good)
        a.update(kw)
        return lib.vh_launch_dense_soft(None, a["pl"], a["n"], a["gh"], a["gw"], a["C"], a["oh"], a["ow"], a["s"], a["values"], a["prob"],
                                        a["expect"], a["entropy"])

    bad = [dict(C=1), dict(C=257), dict(gh=0), dict(gw=0), dict(gh=65), dict(gw=65), dict(oh=0), dict(ow=0), dict(oh=4097), dict(ow=4097),
           dict(n=0), dict(pl=None), dict(s=0.0), dict(s=-1.0), dict(s=float("inf")), dict(s=float("nan")), dict(values=None),
           dict(expect=None), dict(prob=None, expect=None, entropy=None, values=None), dict(pl=off(d_l, 4)), dict(values=off(d_v, 4)),
           dict(prob=off(d_p, 4)), dict(expect=off(d_x, 8)), dict(entropy=off(d_h, 4))]
    for kw in bad:
        lib.vh_set_error(1, b"stale")
        assert soft(**kw) == 1, kw
        msg = lib.vh_last_error().decode()
        assert msg.startswith("vh_launch_dense_soft: ") and len(msg) > 40, (kw, msg)
    assert lib.vh_device_sync() == 0
    for d in (d_p, d_x, d_h):
        assert (d.to_numpy() == FILL).all()
    assert soft() == 0 and lib.vh_device_sync() == 0
    got = dict(prob=d_p.to_numpy()[:m].reshape(n, *out), expect=d_x.to_numpy()[:m].reshape(n, *out), entropy=d_h.to_numpy()[:m].reshape(n, *out))
    sr.check_combined(L, grid, out, 1.0, values, got)
    for d in (d_p, d_x, d_h):
        assert (d.to_numpy()[m:] == FILL).all()


# ---- 4. through the model ---------------------------------------------------------------------------------------------

NL, MB = 21, 4


@pytest.fixture(scope="module")
def small(pkg, device, weights):
    """ViT-B/16 cut to two layers (the 14 x 14 grid, T = 197), max_batch 4, one context per precision made on first use"""
    cfg = pkg.preset("vit_b_16")
    cfg.depth = 2
    w2 = list(weights[:4 + 12 * 2]) + list(weights[-4:])
    made = {}

    def get(precision):
        if precision not in made:
            made[precision] = pkg.ViTHip(cfg, w2, device=0, max_batch=MB, precision=precision)
        return made[precision]

    yield get
    for m in made.values():
        m.close()


@pytest.fixture(scope="module")
def images9(pkg):
    return pkg.synth_images(pkg.preset("vit_b_16"), 0, 9)


@pytest.fixture(scope="module")
def head(pkg, device):
    rng = np.random.default_rng(23)
    W = (rng.standard_normal((NL, 768)) / np.sqrt(768)).astype(np.float32)
    b = (0.1 * rng.standard_normal(NL)).astype(np.float32)
    centres = np.linspace(0.5, 10.0, NL).astype(np.float32)            # depth bins
    return W, b, centres, dev(pkg, W), dev(pkg, b), dev(pkg, centres)


def soft_forward(pkg, model, images, head, out, tap=-1, final_norm=True, scale=2.0, labels=True, which=sr.NAMES):
    """one forward_device with the soft request armed -> (labels or None, {map}, patch logits, class logits, probabilities)"""
    b = pkg.binding
    W, bias, centres, d_w, d_b, d_c = head
    n, nc, P = images.shape[0], model.cfg.num_classes, model.tokens - 1
    d_lab = dev(pkg, np.full(MB * out[0] * out[1], 0xEE, np.uint8), np.uint8) if labels else None
    d_pl = dev(pkg, np.full(MB * P * NL, FILL, np.float32))
    maps = {name: dev(pkg, np.full(MB * out[0] * out[1], FILL, np.float32)) for name in which}
    d_img, d_l, d_p = pkg.DeviceBuffer.from_numpy(images), pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)
    spec = b.DenseSpec(NL, out[0], out[1], tap, final_norm, 768, d_w, d_b)
    cs = spec.c_struct()
    soft = b.DenseSoftSpecC(scale, d_c.ptr if "expect" in which else None)
    bufs = b.DenseBuffers(d_lab.ptr if labels else None, None, d_pl.ptr)
    mp = b.DenseSoftBuffers(*[maps[name].ptr if name in which else None for name in sr.NAMES])
    lib = pkg.lib()
    assert lib.vit_hip_set_dense_soft(model.ctx, C.byref(cs), C.byref(soft), C.byref(bufs), C.byref(mp)) == 0, lib.vh_last_error().decode()
    try:
        model.forward_device(d_img.ptr, n, d_l.ptr, d_p.ptr)
        model.sync()
    finally:
        model.set_dense_soft(None)
    got = {}
    for name in which:
        a = maps[name].to_numpy((MB, *out))
        assert (a[n:] == FILL).all()
        got[name] = a[:n]
    lab = d_lab.to_numpy((MB, *out))[:n] if labels else None
    return lab, got, d_pl.to_numpy((MB, P, NL))[:n], d_l.to_numpy((n, nc)), d_p.to_numpy((n, nc))


def plain_forward(pkg, model, images, head=None, out=None, tap=-1, final_norm=True):
    """un-armed (head None) or with vit_hip_set_dense armed -> (labels or None, class logits, probabilities)"""
    n, nc = images.shape[0], model.cfg.num_classes
    d_img, d_l, d_p = pkg.DeviceBuffer.from_numpy(images), pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)
    d_lab = None
    if head is not None:
        d_lab = dev(pkg, np.full(MB * out[0] * out[1], 0xEE, np.uint8), np.uint8)
        model.set_dense(pkg.binding.DenseSpec(NL, out[0], out[1], tap, final_norm, 768, head[3], head[4]), head[3], head[4], labels=d_lab)
    try:
        model.forward_device(d_img.ptr, n, d_l.ptr, d_p.ptr)
        model.sync()
    finally:
        model.set_dense(None)
    return None if d_lab is None else d_lab.to_numpy((MB, *out))[:n], d_l.to_numpy((n, nc)), d_p.to_numpy((n, nc))


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_armed_maps_are_the_launchers(pkg, small, images9, head, precision):
    """The soft-armed maps equal vh_launch_dense_soft run on the patch logits the same forward wrote, bit for bit; the labels
    equal vit_hip_set_dense's; class logits and probabilities equal an un-armed forward's; without a labels buffer the maps
    are the same bits; expect with the bin centres lies inside the bins"""
    model = small(precision)
    imgs = images9[:3]
    for tap, final_norm, out in ((-1, True, (56, 75)), (0, False, (224, 224))):
        lab, got, pl, logits, probs = soft_forward(pkg, model, imgs, head, out, tap, final_norm)
        want = run_soft(pkg, pl, (14, 14), out, 2.0, head[2])
        for name in sr.NAMES:
            assert same(got[name], want[name]), (precision, tap, name)
        lab0, l0, p0 = plain_forward(pkg, model, imgs, head, out, tap, final_norm)
        un = plain_forward(pkg, model, imgs)
        assert same(lab, lab0) and same(logits, l0) and same(probs, p0) and same(logits, un[1]) and same(probs, un[2])
        none, got2, pl2, l2, _ = soft_forward(pkg, model, imgs, head, out, tap, final_norm, labels=False, which=("expect",))
        assert none is None and same(got2["expect"], got["expect"]) and same(pl2, pl) and same(l2, l0)
        assert (got["expect"] >= 0.5).all() and (got["expect"] <= 10.0).all() and (got["prob"] > 1.0 / NL - 1e-6).all() and (got["prob"] <= 1).all()
        worst = sr.check_combined(pl, (14, 14), out, 2.0, head[2], got, f"{precision} tap {tap}")
        print(f"{precision} tap {tap} -> {out}: worst |error| / combined bound " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_nothing_else_moves_and_launch_counts(pkg, small, images9, head, precision):
    """All six requests armed at once, the dense one with soft maps: the other five's outputs, the class logits and the
    probabilities are the bits of a forward without it.  vit_hip_profile_read: with labels one VIT_OP_HEAD launch more than the
    plain dense request, without a labels buffer as many; after disarming, the un-armed counts"""
    model, b, lib = small(precision), pkg.binding, pkg.lib()
    imgs, n, k, E, T, H = images9[:3], 3, 5, model.cfg.embed_dim, model.tokens, model.cfg.num_heads
    rows = gr.bf16_decode(gr.bf16_round(np.random.default_rng(17).standard_normal((300, E)).astype(np.float32)))
    d_rows = dev(pkg, rows)
    out = (40, 33)

    def counts():
        d_img = pkg.DeviceBuffer.from_numpy(imgs)
        model.profile_enable(1)
        model.forward_device(d_img.ptr, n, None, None)
        got = {name: c for name, (_, c) in model.profile_read().items()}
        model.profile_enable(0)
        return got

    before = counts()
    d_cls, d_pool = pkg.DeviceBuffer(MB * 2 * E), pkg.DeviceBuffer(MB * 2 * E)
    d_lab, d_sc = pkg.DeviceBuffer(MB * k, np.int32), pkg.DeviceBuffer(MB * k)
    d_h, d_m, d_r = pkg.DeviceBuffer(MB * 2 * H * T), pkg.DeviceBuffer(MB * 2 * T), pkg.DeviceBuffer(MB * T)
    d_gi, d_gs = pkg.DeviceBuffer(MB * k, np.int32), pkg.DeviceBuffer(MB * k)
    d_img, d_l, d_p = pkg.DeviceBuffer.from_numpy(imgs), pkg.DeviceBuffer(n * 1000), pkg.DeviceBuffer(n * 1000)
    outputs = (d_cls, d_pool, d_lab, d_sc, d_h, d_m, d_r, d_gi, d_gs, d_l, d_p)

    def others():
        for d in outputs:
            assert lib.vh_memset(d.ptr, 0, d.count * 4, None) == 0
        model.forward_device(d_img.ptr, n, d_l.ptr, d_p.ptr)
        model.sync()
        return [d.to_numpy().copy() for d in outputs]

    d_dl = dev(pkg, np.zeros(MB * out[0] * out[1], np.uint8), np.uint8)
    d_maps = [pkg.DeviceBuffer(MB * out[0] * out[1]) for _ in range(3)]
    spec = lambda: b.DenseSpec(NL, out[0], out[1], -1, True, 768, head[3], head[4])
    model.set_features(b.FeatureSpec(taps=(0, -1)), cls=d_cls, pooled=d_pool)
    model.set_topk(b.TopKSpec(k, "probs"), labels=d_lab, scores=d_sc)
    model.set_attention(b.AttentionSpec((0, -1)), heads=d_h, mean=d_m)
    model.set_rollout(b.RolloutSpec(-2), rollout=d_r)
    model.set_gallery(b.GallerySpec(k, "pooled", -1, True, True, "f32", 300, E, d_rows), d_rows, indices=d_gi, scores=d_gs)
    try:
        want = others()
        assert want[4].any() and want[6].any() and want[8].any()
        plain = counts()
        model.set_dense(spec(), head[3], head[4], labels=d_dl)
        dense = counts()
        assert dense["head_gemm"] == plain["head_gemm"] + 3
        model.set_dense_soft(spec(), head[3], head[4], 2.0, head[5], labels=d_dl, prob=d_maps[0], expect=d_maps[1], entropy=d_maps[2])
        armed = others()
        alone = soft_forward(pkg, small(precision), imgs, head, out)            # re-arms, then disarms the dense request only
        model.set_dense_soft(spec(), head[3], head[4], 2.0, head[5], labels=d_dl, prob=d_maps[0], expect=d_maps[1], entropy=d_maps[2])
        again = others()
        assert same(d_dl.to_numpy((MB, *out))[:n], alone[0])
        for d, name in zip(d_maps, sr.NAMES):
            assert same(d.to_numpy((MB, *out))[:n], alone[1][name]), name
        with_soft = counts()
        assert with_soft["head_gemm"] == dense["head_gemm"] + 1
        assert all(with_soft[o] == plain[o] for o in plain if o != "head_gemm")
        model.set_dense_soft(spec(), head[3], head[4], 2.0, None, prob=d_maps[0], entropy=d_maps[2])      # no labels buffer
        assert counts()["head_gemm"] == dense["head_gemm"]
        model.set_dense(None)                                                  # the plain setter disarms the soft request
        after = others()
        assert counts() == plain
        for w, a, a2, c in zip(want, armed, again, after):
            assert same(w, a) and same(w, a2) and same(w, c)
    finally:
        for disarm in (model.set_features, model.set_topk, model.set_attention, model.set_rollout, model.set_gallery, model.set_dense_soft):
            disarm(None)
    assert counts() == before


def test_arming_rules_on_a_context(pkg, small, images9, head):
    """refusals at arming keep the request armed before; vit_hip_segment_frame_* and the host forms refuse a soft-armed
    context as they refuse a dense-armed one; a host-form arming takes the request over"""
    model, b, lib = small("f32"), pkg.binding, pkg.lib()
    out, imgs = (20, 30), images9[:2]
    lab, got, _, l0, _ = soft_forward(pkg, model, imgs, head, out)
    d_lab = dev(pkg, np.zeros(MB * 600, np.uint8), np.uint8)
    d_p, d_x = pkg.DeviceBuffer(MB * 600), pkg.DeviceBuffer(MB * 600)
    spec = b.DenseSpec(NL, out[0], out[1], -1, True, 768, head[3], head[4])
    model.set_dense_soft(spec, head[3], head[4], 2.0, head[5], labels=d_lab, prob=d_p, expect=d_x)
    try:
        cs, soft = spec.c_struct(), b.DenseSoftSpecC(2.0, head[5].ptr)
        maps = lambda p=d_p.ptr, x=d_x.ptr, h=None: C.byref(b.DenseSoftBuffers(p, x, h))
        bufs = C.byref(b.DenseBuffers(d_lab.ptr, None, None))
        refusals = [(lambda: lib.vit_hip_set_dense_soft(model.ctx, C.byref(cs), None, bufs, maps()), "soft"),
                    (lambda: lib.vit_hip_set_dense_soft(model.ctx, C.byref(cs), C.byref(soft), bufs, None), "d_soft"),
                    (lambda: lib.vit_hip_set_dense_soft(model.ctx, C.byref(cs), C.byref(soft), bufs, maps(None, None, None)), "no soft map"),
                    (lambda: lib.vit_hip_set_dense_soft(model.ctx, C.byref(cs), C.byref(soft), bufs, maps(x=None)), "d_values"),
                    (lambda: lib.vit_hip_set_dense_soft(model.ctx, C.byref(cs), C.byref(b.DenseSoftSpecC(2.0, None)), bufs, maps()), "d_values"),
                    (lambda: lib.vit_hip_set_dense_soft(model.ctx, C.byref(cs), C.byref(b.DenseSoftSpecC(0.0, head[5].ptr)), bufs, maps()), "logit_scale"),
                    (lambda: lib.vit_hip_set_dense_soft(model.ctx, C.byref(cs), C.byref(soft), bufs, maps(p=d_p.ptr.value + 4)), "aligned")]
        bad = spec.c_struct()
        bad.n_labels = 257
        refusals.append((lambda: lib.vit_hip_set_dense_soft(model.ctx, C.byref(bad), C.byref(soft), bufs, maps()), "n_labels"))
        for i, (f, word) in enumerate(refusals):
            lib.vh_set_error(1, b"stale")
            assert f() == 1, i
            msg = lib.vh_last_error().decode()
            assert msg.startswith("vit_hip_set_dense_soft: ") and word in msg, (i, msg)
        with pytest.raises(b.VitHipError, match="vit_hip_set_dense"):
            model.forward(imgs)
        frame = np.zeros((300, 300, 3), np.uint8)
        with pytest.raises(b.VitHipError, match="a dense request is armed"):
            model.segment_frame(frame, head[0], head[1], mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5))
        # still armed as before the refusals
        d_img, d_l = pkg.DeviceBuffer.from_numpy(imgs), pkg.DeviceBuffer(2 * 1000)
        model.forward_device(d_img.ptr, 2, d_l.ptr)
        model.sync()
        assert same(d_lab.to_numpy((MB, *out))[:2], lab) and same(d_p.to_numpy((MB, *out))[:2], got["prob"])
        assert same(d_x.to_numpy((MB, *out))[:2], got["expect"]) and same(d_l.to_numpy((2, 1000)), l0)
        # the host form takes the request over: no soft map is written any more
        host_lab = np.zeros((2, *out), np.uint8)
        assert lib.vh_memset(d_p.ptr, 0, d_p.count * 4, None) == 0
        model.set_dense_host(b.DenseSpec(NL, out[0], out[1], -1, True, 768, head[3], head[4]), head[3], head[4], labels=host_lab)
        model.forward(imgs)
        assert same(host_lab, lab) and not d_p.to_numpy().any()
    finally:
        model.set_dense_host(None)
        model.set_dense_soft(None)


def test_segment_soft_chunks(pkg, small, images9, head):
    """ViTHip.segment_soft with n = 9 > max_batch = 4 (chunks of 4, 4 and 1): per image what single-chunk runs give; the
    defaults return labels and prob; outputs=("expect",) with the bin centres is the depth call"""
    model = small("f32")
    W, bias, centres = head[:3]

    def head_launches():
        d_img = pkg.DeviceBuffer.from_numpy(images9[:1])
        model.profile_enable(1)
        model.forward_device(d_img.ptr, 1, None, None)
        count = model.profile_read()["head_gemm"][1]
        model.profile_enable(0)
        return count

    unarmed = head_launches()
    every = model.segment_soft(images9, W, bias, values=centres, logit_scale=2.0, size=(37, 50), outputs=("labels", "prob", "expect", "entropy"))
    assert {k: (v.shape, v.dtype) for k, v in every.items()} == {
        "labels": ((9, 37, 50), np.dtype(np.uint8)), "prob": ((9, 37, 50), np.dtype(np.float32)),
        "expect": ((9, 37, 50), np.dtype(np.float32)), "entropy": ((9, 37, 50), np.dtype(np.float32))}
    for a in (0, 4, 8):
        one = model.segment_soft(images9[a:a + 4], W, bias, values=centres, logit_scale=2.0, size=(37, 50),
                                 outputs=("labels", "prob", "expect", "entropy"))
        for name, arr in one.items():
            assert same(arr, every[name][a:a + 4]), (a, name)
    dflt = model.segment_soft(images9[:2], W, bias, logit_scale=2.0, size=(37, 50))
    assert set(dflt) == {"labels", "prob"} and same(dflt["prob"], every["prob"][:2]) and same(dflt["labels"], every["labels"][:2])
    assert same(dflt["labels"], model.segment(images9[:2], W, bias, size=(37, 50)))
    depth = model.segment_soft(images9[:2], W, bias, values=centres, logit_scale=2.0, size=(37, 50), outputs=("expect",))
    assert set(depth) == {"expect"} and same(depth["expect"], every["expect"][:2])
    with pytest.raises(ValueError):
        model.segment_soft(images9[:1], W, bias, outputs=("logits",))
    assert head_launches() == unarmed                                          # disarmed on return


def test_cls_only_last_layer_agrees(pkg, small, images9, head):
    """a tap on the last layer under vit_hip_set_last_layer_cls_only runs all rows: the same bits either way"""
    model = small("f32")
    imgs = images9[:3]
    try:
        off = {t: soft_forward(pkg, model, imgs, head, (37, 50), t) for t in (-1, 0)}
        model.set_last_layer_cls_only(True)
        for t in (-1, 0):
            lab, got, pl, logits, probs = soft_forward(pkg, model, imgs, head, (37, 50), t)
            assert same(lab, off[t][0]) and same(pl, off[t][2]) and same(logits, off[t][3]) and same(probs, off[t][4]), t
            for name in sr.NAMES:
                assert same(got[name], off[t][1][name]), (t, name)
    finally:
        model.set_last_layer_cls_only(False)
