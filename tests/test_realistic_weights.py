"""CPU tests of the heavy-tailed weight set (tests/realistic_weights.py) and of the fixtures made with it: the set is
reproduced bit for bit, it looks like the reference's real tensors (tests/golden/ref_weight_stats.json) and not like the
uniform synthetic set, its recorded exposure is as hard as intended, and the port equals the reference's own ViT_seq.c on
it (tests/golden/b16_realistic.npz, oracle/make_golden.py realistic)."""
import json
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

import realistic_weights as rw

GOLDEN = Path(__file__).resolve().parent / "golden"
MATRICES = ("conv_w", "in_w", "out_w", "fc1_w", "fc2_w", "head_w")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN / "b16_realistic.npz")


@pytest.fixture(scope="module")
def b16_set(oracle, gold):
    cfg = oracle.cfg
    return rw.realistic_weights(cfg, int(gold["seed"]), offset=float(gold["offset"]), massive=float(gold["massive"]))


def test_realistic_weights_reproduce_the_stored_sha256(oracle, gold, b16_set):
    """A numpy (or libm) whose log1p / power rounds differently changes the set: it fails here, loudly, not as a parity miss."""
    assert rw.weights_sha256(b16_set) == str(gold["weights_sha256"])
    assert [a.size for a in b16_set] == [oracle.tensor_size(i) for i in range(oracle.num_tensors)]
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in b16_set)
    assert int(gold["dstar"]) == rw.plan(oracle.cfg, int(gold["seed"]))["dstar"]


def test_port_reproduces_the_reference_on_realistic_weights_bit_for_bit(oracle, gold, b16_set):
    """port_forward_image on the heavy-tailed set equals what the reference's own ViT_seq.c gave, for the three synthetic
    images and the real one (one thread per image: the port releases the GIL)."""
    real = np.load(GOLDEN / "b16_real_image.npz")["image"]
    images = [oracle.synth_image(int(i)) for i in gold["synth_images"]] + [np.ascontiguousarray(real)]
    with ThreadPoolExecutor(len(images)) as ex:
        out = list(ex.map(lambda im: oracle.forward(im, b16_set)[:2], images))
    for i, (logits, probs) in enumerate(out):
        assert np.array_equal(logits, gold["logits"][i]), f"image {i}: logits differ from the reference's"
        assert np.array_equal(probs, gold["probs"][i]), f"image {i}: probabilities differ from the reference's"


def test_recorded_exposure_is_in_the_intended_range(gold):
    """At the LayerNorm inputs (2 per layer, then the final one): max |mean|/std >= 3 at half of them at least, and the
    massive channel at >= 50x the row median in every one -- the GPU tests on this set are known to be hard."""
    ms, ratio = gold["exposure_mean_std_max"], gold["exposure_massive_ratio"]
    assert ms.shape == ratio.shape == (2 * 12 + 1,)
    assert (ms >= 3.0).sum() >= (ms.size + 1) // 2, ms
    assert (ms <= 8.0).all(), ms                               # 'about 3-6', not a degenerate row
    assert (ratio >= 50.0).all(), ratio
    assert np.median(gold["exposure_mean_std_median"]) < 1.0  # the offset sits on a quarter of the rows only


def test_recorded_exposure_is_what_the_pinned_set_gives(oracle, gold, b16_set):
    """The stored exposure arrays are recomputed from the pinned set and the same four images (float64 restatement):
    a golden regenerated with a broken exposure() fails here."""
    real = np.load(GOLDEN / "b16_real_image.npz")["image"]
    images = np.stack([oracle.synth_image(int(i)) for i in gold["synth_images"]] + [real])
    exp = rw.exposure(oracle.cfg, b16_set, images, int(gold["dstar"]))
    for key, v in exp.items():
        np.testing.assert_allclose(v, gold[f"exposure_{key}"], rtol=1e-9, err_msg=key)


def test_model_predictions_are_recorded_for_both_fold_settings(gold):
    for mode in ("bf16", "fp8"):
        for key in (f"pred_{mode}_fold1", f"pred_{mode}_fold0", f"pred_{mode}_fold_vs_separate"):
            v = gold[key]
            assert v.shape == (4,) and (v > 0).all() and np.isfinite(v).all(), key
    assert (gold["pred_fp8_fold1"] <= 0.15 / 1.3).all()      # the model predicts the mode's tolerance holds with the fold


def test_weight_statistics_inside_the_reference_ranges(oracle, b16_set):
    """The big matrices of the generated B/16 set are heavy-tailed (kurtosis >= 8, |max|/sigma 14-30), and where the
    reference has the same tensor (conv_proj, out_proj, head) its sigma is within 1.5x of the reference's; the shape
    statistics of conv_proj and out_proj sit inside the reference's range over those matrices.  The uniform set fails."""
    ref = {r["index"]: r for r in json.loads((GOLDEN / "ref_weight_stats.json").read_text())["tensors"]}
    assert len(ref) == 116 and ref[0]["name"] == "class_token"
    shape_ref = [r for r in ref.values() if r["name"] in ("conv_proj_weight",) or r["name"].endswith("out_proj_weight")]
    kmin, kmax = min(r["kurtosis"] for r in shape_ref), max(r["kurtosis"] for r in shape_ref)
    mmin, mmax = min(r["max_over_sigma"] for r in shape_ref), max(r["max_over_sigma"] for r in shape_ref)
    cfg = oracle.cfg
    uniform = oracle.synth_weights(0)
    checked = 0
    for idx, a in enumerate(b16_set):
        role = rw._role(cfg, idx)[0]
        if role not in MATRICES:
            continue
        st = rw.tensor_stats(a)
        assert st["kurtosis"] >= 8.0 and 14.0 <= st["max_over_sigma"] <= 30.0, (idx, role, st)
        assert rw.tensor_stats(uniform[idx])["kurtosis"] < 2.0                     # what the synthetic set has instead
        if idx in ref:
            assert 1 / 1.5 <= st["sigma"] / ref[idx]["sigma"] <= 1.5, (idx, st, ref[idx])
            if role in ("conv_w", "out_w"):
                assert kmin <= st["kurtosis"] <= kmax and mmin <= st["max_over_sigma"] <= mmax, (idx, st)
            checked += 1
    assert checked == 14                                       # conv_proj, 12 out_proj, head


def test_realistic_set_features(oracle, b16_set):
    """The features each keyword controls: d* not a multiple of 32 with both LayerNorm gammas <= 0.1x their median there,
    outlier input columns x8-16 in in_proj and fc1, a ~20 sigma class-token channel, the offset rows."""
    cfg = oracle.cfg
    E, D = cfg.embed_dim, cfg.depth
    pl = rw.plan(cfg, 0)
    ds = pl["dstar"]
    assert ds % 32 != 0 and 0 < ds < E
    for layer in range(D):
        for k in (0, 6):
            g = b16_set[4 + 12 * layer + k]
            assert abs(g[ds]) <= 0.1 * np.median(np.abs(g))
        for k in (2, 8):
            cols = np.sqrt((b16_set[4 + 12 * layer + k].reshape(-1, E).astype(np.float64) ** 2).mean(0))
            assert (cols >= 6.0 * np.median(cols)).sum() == len(rw.OUTLIER_GAINS)
    cls = b16_set[0].astype(np.float64)
    spike = int(np.argmax(np.abs(cls)))
    rest = np.delete(cls, spike)
    assert abs(cls[spike]) >= 15.0 * rest.std()                 # ~20 sigma of the tensor without it
    pos = b16_set[3].reshape(-1, E).astype(np.float64)
    assert pos[1::rw.OFFSET_ROW_PERIOD].mean() - pos[2::rw.OFFSET_ROW_PERIOD].mean() == pytest.approx(pl["c"], rel=1e-3)
    plain = rw.realistic_weights(cfg, 0, offset=0.0, massive=0.0, outliers=False, cls_spike=False)
    assert rw.weights_sha256(plain) != rw.weights_sha256(b16_set)
    assert abs(plain[3].reshape(-1, E).mean()) < 1e-3 and np.abs(plain[2]).max() < 1.0
