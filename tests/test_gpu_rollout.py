"""Attention rollout (vh_launch_rollout_step / _read, csrc/rollout.hip; vit_hip_set_rollout / _host): the launcher against
the float64 statement of the definition (tests/rollout_ref.py) in the three stored forms of Q|K|V over chains of three
steps, and the model-level guarantees the header states -- nothing else moves, every precision mode and plan, both forms,
every entry point, batch-position independence, arming rules, the long-sequence plan.

Tolerances.  The launcher's is derived (rollout_ref.bound) and holds the model's rollout too whenever the reference is
given the Q|K|V the context itself holds.  first_layer = -1 needs no reference at all: that rollout is 0.5 * the attention
map's head mean + 0.5 at key 0, and both kernels are held to derived bounds.  Against the ORACLE's Q|K|V (fp32, its own
summation order through the layers in front) nothing can be derived: MODEL_TOL is 8 x the largest |rollout - oracle|
measured on an MI355X, the margin tests/test_gpu_attn_map.py keeps.  Measured values are beside the constants."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import attn_ref as ar
import rollout_ref as rr
import topk_ref as tr

pytestmark = pytest.mark.gpu

ENV = ("VIT_HIP_P3", "VIT_HIP_GEMM_FP32", "VIT_HIP_ATTN", "VIT_HIP_LN_FOLD", "VIT_HIP_LAST_LAYER", "VIT_HIP_PRECISION")
FORMS = (rr.ROWS_F32, rr.PLANES3, rr.PLANES_F16)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FILL = np.float32(-77.0)

# Largest |rollout - oracle| of image 0 through a ViT-B/16 cut to 3 layers, measured on an MI355X (the first run of these
# tests), and the constants at 8 x that: MODEL_TOL for first_layer = 0, LATE_TOL for first_layer = 1 (the last two layers
# alone).  Synthetic weights make near-uniform attention: rollout[0] = 0.1294 and the patch values are about 4.4e-3, so
# the constants are 3.5e-6, 4.4e-4 and 6.6e-3 of a typical patch value.
#   f32   first_layer 0: 1.943e-09   first_layer 1: 5.615e-09
#   bf16  first_layer 0: 2.415e-07   first_layer 1: 4.492e-07
#   fp8   first_layer 0: 3.644e-06   first_layer 1: 4.700e-06
MODEL_TOL = {"f32": 8 * 1.943e-09, "bf16": 8 * 2.415e-07, "fp8": 8 * 3.644e-06}
LATE_TOL = {"f32": 8 * 5.615e-09, "bf16": 8 * 4.492e-07, "fp8": 8 * 4.700e-06}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def worst_ratio(got, ref, bnd):
    """the largest |got - ref| / (bnd * ref + 1e-30): <= 1 is inside the bound"""
    return float((np.abs(got.astype(np.float64) - ref) / (bnd * ref + 1e-30)).max())


# ---- the launcher ----------------------------------------------------------------------------------------------------------

def stored(pkg, form, qkv):
    """-> (device buffer of qkv in `form`, the fp32 values that buffer decodes to)"""
    if form == rr.ROWS_F32:
        return pkg.DeviceBuffer.from_numpy(qkv), qkv
    if form == rr.PLANES_F16:
        planes = ar.encode_f16(qkv)
        return ar.upload(pkg, planes), ar.decode_f16(planes)
    d_pl, planes = ar.split3_on_device(pkg, qkv)
    assert np.array_equal(ar.decode_planes3(planes), qkv)          # exact: the reference gets the original fp32
    return d_pl, qkv


class Chain:
    """Two sentinel-filled R buffers with PAD elements behind [n][T][T], and the workspace of a step"""
    PAD = 64

    def __init__(self, pkg, n, T):
        self.pkg, self.L, self.n, self.T, self.size = pkg, pkg.lib(), n, T, n * T * T
        self.r = [pkg.DeviceBuffer.from_numpy(np.full(self.size + self.PAD, FILL)) for _ in range(2)]
        self.ws = pkg.DeviceBuffer(max(self.L.vh_rollout_workspace(n, T) // 4, 4))
        self.steps = 0

    def step(self, d_qkv, form, E, H):
        """one more step -> (R_next [n][T][T], the bytes of R_prev before and after, R_next's padding)"""
        k = self.steps
        nxt, prv = self.r[k & 1], self.r[(k + 1) & 1]
        before = prv.to_numpy()
        rc = self.L.vh_launch_rollout_step(None, d_qkv.ptr, form, self.n, self.T, E, H, None if k == 0 else prv.ptr, nxt.ptr, self.ws.ptr)
        assert rc == 0, self.L.vh_last_error().decode()
        assert self.L.vh_device_sync() == 0, self.L.vh_last_error().decode()
        self.steps += 1
        out = nxt.to_numpy()
        return out[:self.size].reshape(self.n, self.T, self.T), before, prv.to_numpy(), out[self.size:]

    def read(self):
        """vh_launch_rollout_read of the last product -> [n][T], the padding behind it"""
        d_out = self.pkg.DeviceBuffer.from_numpy(np.full(self.n * self.T + self.PAD, FILL))
        rc = self.L.vh_launch_rollout_read(None, self.r[(self.steps - 1) & 1].ptr, self.n, self.T, d_out.ptr)
        assert rc == 0 and self.L.vh_device_sync() == 0, self.L.vh_last_error().decode()
        out = d_out.to_numpy()
        return out[:self.n * self.T].reshape(self.n, self.T), out[self.n * self.T:]


@pytest.mark.parametrize("n,T,E,H", rr.CASES)
def test_launcher_chain_vs_reference(pkg, device, n, T, E, H):
    """Three chained steps with distinct Q|K|V, the first from the identity, in all three forms at amplitudes 1 and 3: the
    whole R after every step within rollout_ref.bound of the float64 definition on the values the buffers hold, rows
    summing to 1, nothing negative, nothing written outside [n][T][T] of R_next or anywhere in R_prev; the read returns row
    0 bit for bit; image 0 appended as image n of a batch of n + 1 gives the bits it gave at position 0 of n.  Measured
    worst |R - ref| / bound on an MI355X: up to 0.019 over these cases (the largest at T = 15, amplitude 3, first step); the
    fp32 emulation of tests/test_rollout_host.py reaches the same 0.019."""
    worst = 0.0
    for amp in rr.AMPLITUDES:
        layers = rr.case_layers(n, T, E, H, amp)
        refs = {}
        for form in FORMS:
            held = [stored(pkg, form, q) for q in layers]
            kind = form == rr.PLANES_F16                            # fp32 rows and three-part planes hold the same values
            if kind not in refs:
                values = [v for _, v in held]
                refs[kind] = rr.rollout_steps(values, n, T, H), rr.bound(values, n, T, H)
            chain, got = Chain(pkg, n, T), None
            for step, ((d_qkv, _), ref, bnd) in enumerate(zip(held, *refs[kind])):
                got, before, after, pad = chain.step(d_qkv, form, E, H)
                rel = worst_ratio(got, ref, bnd)
                worst = max(worst, rel)
                print(f"(n={n}, T={T}, E={E}, H={H}) form {form} amplitude {amp} step {step}: worst |R - ref| / bound = {rel:.4f}")
                assert rel <= 1.0, (form, amp, step, rel)
                assert (got >= 0).all()
                assert np.abs(got.astype(np.float64).sum(axis=2) - 1.0).max() <= (step + 1) * (2 * T + 8) * 2.0 ** -24
                assert (pad == FILL).all() and same(before, after), (form, amp, step)
            row0, pad = chain.read()
            assert same(row0, got[:, 0, :]) and (pad == FILL).all()
            if amp == rr.AMPLITUDES[-1]:
                more = [np.concatenate([q, q[:T]]) for q in layers]            # image 0 again, at position n of n + 1
                longer, again = Chain(pkg, n + 1, T), None
                for q in more:
                    again = longer.step(stored(pkg, form, q)[0], form, E, H)[0]
                assert same(again[:n], got) and same(again[n], got[0]), form
    assert worst <= 1.0


def test_launcher_refusals(pkg, device):
    L = pkg.lib()
    n, T, E, H = 1, 10, 128, 2
    qkv = rr.case_layers(n, T, E, H, 1.0)[0]
    d_qkv = pkg.DeviceBuffer.from_numpy(np.concatenate([qkv.ravel(), np.zeros(3 * 288 * T, np.float32)]))
    size = n * T * T
    d_a, d_b, d_w = (pkg.DeviceBuffer.from_numpy(np.full(size + 4, FILL)) for _ in range(3))
    d_out = pkg.DeviceBuffer.from_numpy(np.full(n * T + 4, FILL))
    off = lambda d: C.c_void_p(d.ptr.value + 4)
    for args in ((d_qkv.ptr, 3, n, T, E, H, d_a.ptr, d_b.ptr, d_w.ptr),           # unknown form
                 (d_qkv.ptr, -1, n, T, E, H, d_a.ptr, d_b.ptr, d_w.ptr),
                 (d_qkv.ptr, 0, n, T, 48, 2, d_a.ptr, d_b.ptr, d_w.ptr),          # head_dim 24
                 (d_qkv.ptr, 0, n, T, 288, 2, d_a.ptr, d_b.ptr, d_w.ptr),         # head_dim 144
                 (d_qkv.ptr, 1, n, T, 80, 1, d_a.ptr, d_b.ptr, d_w.ptr),          # planes need embed_dim % 32 == 0
                 (d_qkv.ptr, 2, n, T, 80, 1, d_a.ptr, d_b.ptr, d_w.ptr),
                 (off(d_qkv), 0, n, T, E, H, d_a.ptr, d_b.ptr, d_w.ptr),          # misaligned
                 (d_qkv.ptr, 0, n, T, E, H, off(d_a), d_b.ptr, d_w.ptr),
                 (d_qkv.ptr, 0, n, T, E, H, d_a.ptr, off(d_b), d_w.ptr),
                 (d_qkv.ptr, 0, n, T, E, H, d_a.ptr, d_b.ptr, off(d_w)),
                 (d_qkv.ptr, 0, n, T, E, H, d_a.ptr, d_a.ptr, d_w.ptr),           # r_prev == r_next
                 (d_qkv.ptr, 0, n, T, E, H, d_a.ptr, d_w.ptr, d_w.ptr),           # r_next is the workspace
                 (d_qkv.ptr, 0, 0, T, E, H, d_a.ptr, d_b.ptr, d_w.ptr),           # n <= 0
                 (d_qkv.ptr, 0, -1, T, E, H, d_a.ptr, d_b.ptr, d_w.ptr),
                 (d_qkv.ptr, 0, n, 0, E, H, d_a.ptr, d_b.ptr, d_w.ptr),           # no tokens
                 (d_qkv.ptr, 0, n, 1857, E, 1, d_a.ptr, d_b.ptr, d_w.ptr),        # more tokens than LDS holds at head_dim 128
                 (d_qkv.ptr, 0, n, T, E, 0, d_a.ptr, d_b.ptr, d_w.ptr),
                 (None, 0, n, T, E, H, d_a.ptr, d_b.ptr, d_w.ptr),
                 (d_qkv.ptr, 0, n, T, E, H, d_a.ptr, None, d_w.ptr),
                 (d_qkv.ptr, 0, n, T, E, H, d_a.ptr, d_b.ptr, None)):
        L.vh_set_error(1, b"stale")
        assert L.vh_launch_rollout_step(None, *args) == 1, args[1:6]
        assert L.vh_last_error().decode().startswith("vh_launch_rollout_step: "), args[1:6]
    for args in ((None, n, T, d_out.ptr), (d_a.ptr, n, T, None), (d_a.ptr, 0, T, d_out.ptr), (d_a.ptr, n, 0, d_out.ptr),
                 (off(d_a), n, T, d_out.ptr), (d_a.ptr, n, T, off(d_out))):
        L.vh_set_error(1, b"stale")
        assert L.vh_launch_rollout_read(None, *args) == 1
        assert L.vh_last_error().decode().startswith("vh_launch_rollout_read: ")
    assert L.vh_device_sync() == 0
    for d in (d_a, d_b, d_w, d_out):
        assert (d.to_numpy() == FILL).all()
    # and the same arguments in order are taken: identity step into b, then b -> a
    assert L.vh_launch_rollout_step(None, d_qkv.ptr, 0, n, T, E, H, None, d_b.ptr, d_w.ptr) == 0
    assert L.vh_launch_rollout_step(None, d_qkv.ptr, 0, n, T, E, H, d_b.ptr, d_a.ptr, d_w.ptr) == 0
    assert L.vh_launch_rollout_read(None, d_a.ptr, n, T, d_out.ptr) == 0 and L.vh_device_sync() == 0
    ref, bnd = rr.rollout_steps([qkv, qkv], n, T, H), rr.bound([qkv, qkv], n, T, H)
    assert worst_ratio(d_b.to_numpy()[:size].reshape(n, T, T), ref[0], bnd[0]) <= 1.0
    assert worst_ratio(d_a.to_numpy()[:size].reshape(n, T, T), ref[1], bnd[1]) <= 1.0
    assert same(d_out.to_numpy()[:T], d_a.to_numpy()[:T])
    assert (d_a.to_numpy()[size:] == FILL).all() and (d_b.to_numpy()[size:] == FILL).all() and (d_out.to_numpy()[n * T:] == FILL).all()


# ---- the model -------------------------------------------------------------------------------------------------------------

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


def armed_device(pkg, model, images, first=0, call=None):
    """a device-form forward with rollout armed -> rollout [n][T], logits, probs; rows of images beyond n keep FILL"""
    n, nc, T, mb = images.shape[0] if call is None else call[1], model.cfg.num_classes, model.tokens, model.max_batch
    d_r = pkg.DeviceBuffer.from_numpy(np.full(mb * T, FILL))
    d_l, d_p = pkg.DeviceBuffer(n * nc), pkg.DeviceBuffer(n * nc)
    model.set_rollout(pkg.binding.RolloutSpec(first), rollout=d_r)
    try:
        if call is None:
            d_img = pkg.DeviceBuffer.from_numpy(images)
            model.forward_device(d_img.ptr, n, d_l.ptr, d_p.ptr)
        else:
            call[0](d_l, d_p)
        model.sync()
    finally:
        model.set_rollout(None)
    out = d_r.to_numpy((mb, T))
    assert (out[n:] == FILL).all()
    return out[:n].copy(), d_l.to_numpy((n, nc)), d_p.to_numpy((n, nc))


def stochastic(roll, layers, T):
    """non-negative, finite, rows summing to 1 within layers * (2T + 8) * 2^-24"""
    return bool(np.isfinite(roll).all() and (roll >= 0).all()
                and np.abs(roll.astype(np.float64).sum(axis=1) - 1.0).max() <= layers * (2 * T + 8) * 2.0 ** -24)


def last_layer_identity(pkg, model, images, qkv_last, tag):
    """first_layer = -1 against the attention map of the same forward: rollout = 0.5 * mean + 0.5 e_0.  Both kernels are
    within their derived bounds of the same exact value m (b_r: rollout_ref.bound of one layer; b_m: attn_ref.bound of the
    heads plus (H + 1) 2^-24 for their fp32 mean), so
    |rollout - (0.5 mean + 0.5 e_0)| <= b_r (0.5 m + 0.5 e_0) + 0.5 b_m m <= (b_r + b_m) (1 + b_m) (0.5 mean + 0.5 e_0).
    The bounds need S, the layer's largest sum_d |q_d k_d| / sqrt(D), which enters them linearly: it is taken from the
    oracle's fp32 Q|K|V of that layer and DOUBLED.  S is a maximum of sums of D magnitudes; a precision mode's rounding in
    front of the layer moves single q and k by a few percent at most, which doubling covers with a wide margin.
    -> rollout, logits, probs"""
    n, T, H = images.shape[0], model.tokens, model.cfg.num_heads
    d_m = pkg.DeviceBuffer(model.max_batch * T)
    model.set_attention(pkg.binding.AttentionSpec((-1,)), mean=d_m)
    try:
        roll, logits, probs = armed_device(pkg, model, images, -1)
    finally:
        model.set_attention(None)
    mean = d_m.to_numpy()[: n * T].reshape(n, T).astype(np.float64)
    want = 0.5 * mean
    want[:, 0] += 0.5
    for i in range(n):
        qkv2 = (qkv_last[i] * np.float32(np.sqrt(2.0))).astype(np.float32)       # doubles every |q k|
        b_r, b_m = float(rr.bound([qkv2], 1, T, H)[0].max()), float(ar.bound(qkv2, 1, T, H).max()) + (H + 1) * 2.0 ** -24
        b = (b_r + b_m) * (1.0 + b_m)
        rel = float((np.abs(roll[i].astype(np.float64) - want[i]) / (b * want[i] + 1e-30)).max())
        print(f"{tag}: image {i}: first_layer -1, worst |rollout - (0.5 mean + 0.5 e0)| / bound = {rel:.4f}")
        assert rel <= 1.0, (tag, i, rel)
    assert stochastic(roll, 1, T)
    return roll, logits, probs


@pytest.mark.parametrize("precision", ["f32", "bf16", "fp8"])
def test_last_layer_rollout_is_half_the_attention_map(pkg, models, images11, oracle_qkv, precision):
    model = models(precision)
    imgs = images11[:2]
    l0, p0 = plain_device(pkg, model, imgs)
    _, l1, p1 = last_layer_identity(pkg, model, imgs, oracle_qkv((0, 11), (1, 11)), precision)
    assert same(l1, l0) and same(p1, p0)


@pytest.fixture(scope="module")
def cut3(pkg, cfg, weights):
    """ViT-B/16 cut to its first three layers: (config, weights)"""
    small = pkg.preset("vit_b_16")
    small.depth = 3
    return small, weights[:4 + 12 * 3] + weights[-4:]


@pytest.mark.parametrize("precision", ["f32", "bf16", "fp8"])
def test_three_layer_rollout_vs_oracle(pkg, device, cut3, images11, oracle_qkv, precision):
    """One image through the three-layer model, first_layer = 0; the reference is rollout_ref on the oracle's own Q|K|V of
    the three layers (fp32 throughout), so the difference holds everything the mode does in front of each layer."""
    small, w3 = cut3
    model = pkg.ViTHip(small, w3, device=0, max_batch=8, precision=precision)
    try:
        roll, _, _ = armed_device(pkg, model, images11[:1], 0)
        late, _, _ = armed_device(pkg, model, images11[:1], 1)
        T, H = model.tokens, small.num_heads
    finally:
        model.close()
    qkvs = oracle_qkv((0, 0), (0, 1), (0, 2))
    ref = rr.rollout(qkvs, 1, T, H)
    diff = float(np.abs(roll.astype(np.float64) - ref).max())
    dlate = float(np.abs(late.astype(np.float64) - rr.rollout(qkvs[1:], 1, T, H)).max())
    print(f"{precision}: three layers, max |rollout - oracle| = {diff:.3e} (first_layer 1: {dlate:.3e}); "
          f"rollout[0] = {roll[0, 0]:.4f}, largest patch value {roll[0, 1:].max():.3e}")
    assert stochastic(roll, 3, T) and stochastic(late, 2, T) and not same(roll, late)
    assert diff <= MODEL_TOL[precision] and dlate <= LATE_TOL[precision], (precision, diff, dlate)


@pytest.mark.parametrize("precision", ["f32", "bf16", "fp8", "f32_fp16x2"])
def test_nothing_else_moves(pkg, models, images11, precision):
    """Features, top-k and attention maps armed: all their outputs, the logits and the probabilities are the same bits
    with rollout armed beside them, and after it is disarmed; an un-armed forward launches what it launched before."""
    model, b = models(precision), pkg.binding
    imgs, n, k, E, T, H = images11[:5], 5, 5, model.cfg.embed_dim, model.tokens, model.cfg.num_heads
    taps = (0, -1)

    def counts():
        d_img = pkg.DeviceBuffer.from_numpy(imgs)
        model.profile_enable(1)
        model.forward_device(d_img.ptr, n, None, None)
        got = {name: c for name, (_, c) in model.profile_read().items()}
        model.profile_enable(0)
        return got

    before = counts()
    fspec, tspec, aspec = b.FeatureSpec(taps=(3, -1)), b.TopKSpec(k, "probs"), b.AttentionSpec(taps)
    d_cls, d_pool = pkg.DeviceBuffer(8 * 2 * E), pkg.DeviceBuffer(8 * 2 * E)
    d_lab, d_sc = pkg.DeviceBuffer(8 * k, np.int32), pkg.DeviceBuffer(8 * k)
    d_h, d_m = pkg.DeviceBuffer(8 * 2 * H * T), pkg.DeviceBuffer(8 * 2 * T)
    d_img, d_l, d_p = pkg.DeviceBuffer.from_numpy(imgs), pkg.DeviceBuffer(n * 1000), pkg.DeviceBuffer(n * 1000)
    outputs = (d_cls, d_pool, d_lab, d_sc, d_h, d_m, d_l, d_p)

    def others():
        for d in outputs:
            assert pkg.lib().vh_memset(d.ptr, 0, d.count * 4, None) == 0
        model.forward_device(d_img.ptr, n, d_l.ptr, d_p.ptr)
        model.sync()
        return [d.to_numpy().copy() for d in outputs]

    model.set_features(fspec, cls=d_cls, pooled=d_pool)
    model.set_topk(tspec, labels=d_lab, scores=d_sc)
    model.set_attention(aspec, heads=d_h, mean=d_m)
    try:
        want = others()
        assert np.array_equal(want[2][: n * k].reshape(n, k), tr.topk(want[6].reshape(n, 1000), k)) and want[4].any()
        d_r = pkg.DeviceBuffer.from_numpy(np.full(8 * T, FILL))
        model.set_rollout(b.RolloutSpec(0), rollout=d_r)
        armed = others()
        with_all = counts()
        model.set_rollout(None)
        after = others()
        for w, a, c in zip(want, armed, after):
            assert same(w, a) and same(w, c)
        roll = d_r.to_numpy((8, T))
        assert stochastic(roll[:n], model.cfg.depth, T) and (roll[n:] == FILL).all()
        # one timed operator per layer from first_layer on and the read, beside the two attention taps
        plain = counts()
        assert with_all["attention"] == plain["attention"] + model.cfg.depth + 1
        assert all(with_all[o] == plain[o] for o in plain if o != "attention")
    finally:
        model.set_features(None)
        model.set_topk(None)
        model.set_attention(None)
        model.set_rollout(None)
    assert counts() == before
    # rollout alone: logits and probabilities of an un-armed forward; a later first layer counts fewer launches
    l0, p0 = plain_device(pkg, model, imgs)
    alone, l1, p1 = armed_device(pkg, model, imgs, 0)
    assert same(l1, l0) and same(p1, p0) and same(alone, roll[:n])
    model.set_rollout(b.RolloutSpec(-2), rollout=d_r)
    late = counts()
    model.set_rollout(None)
    assert late["attention"] == before["attention"] + 3 and counts() == before


@pytest.mark.parametrize("plan", ["p3_off", "attn_long", "tiled_p3_off", "cls_only"])
def test_plans(pkg, device, cfg, weights, models, images11, oracle_qkv, monkeypatch, plan):
    """Two images in every plan a context can be created in: the last layer's rollout against the same forward's attention
    map, the full rollout row-stochastic, logits bit-identical to un-armed."""
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
        last, l1, p1 = last_layer_identity(pkg, model, imgs, oracle_qkv((0, 11), (1, 11)), plan)
        full, l2, p2 = armed_device(pkg, model, imgs, 0)
        assert same(l1, l0) and same(p1, p0) and same(l2, l0) and same(p2, p0)
        assert stochastic(full, cfg.depth, model.tokens) and not same(full, last)
        if plan == "cls_only":
            model.set_last_layer_cls_only(False)
            l3, _ = plain_device(pkg, model, imgs)
            again, _, _ = armed_device(pkg, model, imgs, 0)
            assert same(l3, l0) and same(again, full)
    finally:
        if env:
            model.close()
        else:
            model.set_last_layer_cls_only(False)


def test_batch_position_independence(pkg, models, images11):
    order = np.array([0, 1, 2, 4, 5, 3, 6, 7])                       # image 3 at position 5 of 8
    for precision in ("f32", "bf16"):                                # bf16: fp16 planes laid out by the batch's row count
        model = models(precision)
        r8, _, _ = armed_device(pkg, model, images11[order], 0)
        r1, _, _ = armed_device(pkg, model, images11[3:4], 0)
        assert same(r8[5:6], r1) and not same(r8[4:5], r1), precision


def test_entry_points(pkg, device, cfg, weights, models, images11):
    b = pkg.binding
    # host form, 11 images through max_batch 4: chunks of 4, 4 and 3
    small = pkg.ViTHip(cfg, weights, device=0, max_batch=4)
    try:
        dev = [armed_device(pkg, small, images11[a:a + 4], 0) for a in (0, 4, 8)]
        host = small.rollout(images11, 0)
        assert same(host, np.concatenate([d[0] for d in dev]))
        late = np.zeros((11, small.tokens), np.float32)
        small.set_rollout_host(b.RolloutSpec(-3), rollout=late)
        logits, _ = small.forward(images11)
        small.set_rollout_host(None)
        assert same(logits, np.concatenate([d[1] for d in dev]))
        assert same(late, np.concatenate([armed_device(pkg, small, images11[a:a + 4], 9)[0] for a in (0, 4, 8)]))
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
    scale, bias = np.array(norm.scale[:3], dtype=np.float32), np.array(norm.bias[:3], dtype=np.float32)

    def normalised():
        u8 = d_crops.to_numpy((n, S, S, 3))
        return u8, np.ascontiguousarray(((u8.astype(np.float32) * scale).astype(np.float32) + bias).astype(np.float32).transpose(0, 3, 1, 2))

    model.resize_crop_u8(descs, 256, d_crops.ptr)
    model.sync()
    u8, f32 = normalised()
    want = armed_device(pkg, model, f32, 0)
    got = armed_device(pkg, model, None, 0, call=(lambda d_l, d_p: model.forward_device_u8(d_crops.ptr, n, norm, "hwc", d_l.ptr, d_p.ptr), n))
    got_r = armed_device(pkg, model, None, 0,
                         call=(lambda d_l, d_p: model.forward_device_u8_resized(descs, 256, norm, "bilinear", "hwc", d_l.ptr, d_p.ptr), n))
    for a, b_, w in zip(got, got_r, want):
        assert same(a, w) and same(b_, w)
    # their host forms
    hr = np.empty_like(want[0])
    for call in (lambda: model.forward_u8(u8, norm, None), lambda: model.forward_u8_resized(sources, 256, "bilinear", norm)):
        hr.fill(0)
        model.set_rollout_host(b.RolloutSpec(0), rollout=hr)
        try:
            hl, _ = call()
        finally:
            model.set_rollout_host(None)
        assert same(hr, want[0]) and same(hl, want[1])
    # boxes: three regions of two of the images, device and host form
    boxes = [(0, (10.0, 20.0, 250.0, 290.0)), (2, (0.0, 0.0, 401.0, 257.0)), (2, (100.5, 30.25, 300.0, 200.0))]
    model.crop_boxes_u8(descs, boxes, d_crops.ptr, filter="bicubic")
    model.sync()
    _, f32 = normalised()
    want = armed_device(pkg, model, f32, 0)
    got = armed_device(pkg, model, None, 0,
                       call=(lambda d_l, d_p: model.forward_device_u8_boxes(descs, boxes, norm, "bicubic", "hwc", d_l.ptr, d_p.ptr), n))
    for a, w in zip(got, want):
        assert same(a, w)
    hr.fill(0)
    model.set_rollout_host(b.RolloutSpec(0), rollout=hr)
    try:
        hl, _ = model.forward_u8_boxes(sources, boxes, "bicubic", norm)
    finally:
        model.set_rollout_host(None)
    assert same(hr, want[0]) and same(hl, want[1])


def test_context_refusals(pkg, device, models, images11):
    model, b, L = models("f32"), pkg.binding, pkg.lib()
    n, nc, T = 2, 1000, model.tokens
    imgs = images11[:n]
    want, l0, _ = armed_device(pkg, model, imgs, 0)
    d_img, d_l = pkg.DeviceBuffer.from_numpy(imgs), pkg.DeviceBuffer(n * nc)
    d_r = pkg.DeviceBuffer(8 * T)
    spec = b.RolloutSpec(0)
    model.set_rollout(spec, rollout=d_r)
    try:
        # device form armed: the host forms refuse
        with pytest.raises(b.VitHipError, match="vit_hip_set_rollout"):
            model.forward(imgs)
        assert "rollout" in L.vh_last_error().decode()
        # refused re-arms keep the request: a misaligned buffer, no buffer, no buffers struct, a bad spec
        cs = spec.c_struct()
        assert L.vit_hip_set_rollout(model.ctx, C.byref(cs), C.byref(b.RolloutBuffers(d_r.ptr.value + 4))) == 1
        assert "aligned" in L.vh_last_error().decode()
        assert L.vit_hip_set_rollout(model.ctx, C.byref(cs), C.byref(b.RolloutBuffers(None))) == 1
        assert L.vit_hip_set_rollout(model.ctx, C.byref(cs), None) == 1
        for first in (12, -13):
            bad = b.RolloutSpecC(first)
            assert L.vit_hip_set_rollout(model.ctx, C.byref(bad), C.byref(b.RolloutBuffers(d_r.ptr))) == 1
            assert "first_layer" in L.vh_last_error().decode()
            assert L.vit_hip_set_rollout_host(model.ctx, C.byref(bad), C.byref(b.RolloutBuffers(d_r.ptr))) == 1
        model.forward_device(d_img.ptr, n, d_l.ptr)
        model.sync()
        assert same(d_r.to_numpy((8, T))[:n], want) and same(d_l.to_numpy((n, nc)), l0)
        # host form armed (which disarms the device form): the device forms refuse, nothing is launched
        hr = np.zeros_like(want)
        model.set_rollout_host(spec, rollout=hr)
        sentinel = np.full(n * nc, -7.0, np.float32)
        assert L.vh_h2d(d_l.ptr, sentinel.ctypes.data_as(C.c_void_p), sentinel.nbytes, None) == 0
        assert L.vh_memset(d_r.ptr, 0, d_r.count * 4, None) == 0
        assert L.vit_hip_forward_device(model.ctx, d_img.ptr, n, d_l.ptr, None, None) == 1
        assert "vit_hip_set_rollout_host" in L.vh_last_error().decode()
        model.sync()
        assert np.array_equal(d_l.to_numpy(), sentinel) and not d_r.to_numpy().any()
        hl, _ = model.forward(imgs)
        assert same(hr, want) and same(hl, l0)
        # the other three kinds keep their messages and their order: a feature request armed in the other form is named first
        d_cls = pkg.DeviceBuffer(8 * model.cfg.embed_dim)
        model.set_features(b.FeatureSpec(), cls=d_cls)
        with pytest.raises(b.VitHipError, match=r"armed for device feature buffers \(vit_hip_set_features\)"):
            model.forward(imgs)
        model.set_features(None)
    finally:
        model.set_features(None)
        model.set_rollout_host(None)
        model.set_rollout(None)
    # a head_dim the kernel does not take: refused when armed, not at the first forward
    odd = pkg.preset("vit_b_16")
    odd.img_size, odd.patch_size, odd.num_classes = 64, 16, 10
    odd.embed_dim, odd.depth, odd.num_heads, odd.mlp_hidden = 96, 1, 4, 192
    m = pkg.ViTHip(odd, pkg.synth_weights(odd, 21), device=0, max_batch=2)
    try:
        with pytest.raises(b.VitHipError, match="head_dim"):
            m.set_rollout(spec, rollout=pkg.DeviceBuffer(2 * m.tokens))
    finally:
        m.close()


# ---- the long-sequence plan ------------------------------------------------------------------------------------------------

def test_long_sequence(pkg, device):
    """vit_b_16_384 cut to two layers (T = 577, the plan's ATTN_LONG: Q|K|V as three-part planes), two images,
    first_layer 0: against rollout_ref on the oracle's Q|K|V of those layers the rollout meets the LAUNCHER's bound -- two
    layers in, what the layers in front add stays inside the margin the bound leaves over fp32 summation -- and logits are
    bit-identical to un-armed."""
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
        roll, l1, p1 = armed_device(pkg, model, imgs, 0)
        T, H = model.tokens, cfg.num_heads
    finally:
        model.close()
    assert same(l1, l0) and same(p1, p0) and T == 577 and stochastic(roll, 2, T)
    ok = True
    for i in range(2):
        layers = [qkv[(i, 0)], qkv[(i, 1)]]
        ref, bnd = rr.rollout(layers, 1, T, H), rr.bound(layers, 1, T, H)[-1][:, 0]
        rel = worst_ratio(roll[i:i + 1], ref, bnd)
        print(f"b16_384 image {i}: worst |rollout - oracle| / launcher bound = {rel:.4f}, "
              f"max |rollout - oracle| = {np.abs(roll[i] - ref[0]).max():.3e}")
        ok = ok and rel <= 1.0
    assert ok
