"""All six armed outputs at once through the host form's copy-back (pipeline_run over serving_staged,
csrc/vit_requests.h): 9 images on a context of max_batch 4 are three chunks -- both pinned slots used twice and a ragged last
chunk of one image -- with logits and probabilities asked for too.  Every array must have the bits the device forms give
with all six armed, run chunk by chunk on the same images."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MB, N, K, NL, OUT = 4, 9, 5, 21, (37, 50)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def test_host_form_of_all_six_is_the_device_form_chunk_by_chunk(pkg, device, weights):
    b = pkg.binding
    cfg = pkg.preset("vit_b_16")
    images = pkg.synth_images(cfg, 0, N)
    model = pkg.ViTHip(cfg, weights, device=0, max_batch=MB)
    try:
        T, E, H, nc = model.tokens, cfg.embed_dim, cfg.num_heads, cfg.num_classes
        rng = np.random.default_rng(31)
        d_rows = pkg.DeviceBuffer.from_numpy(rng.standard_normal((300, E)).astype(np.float32))
        head_w = (rng.standard_normal((NL, E)) / np.sqrt(E)).astype(np.float32)
        head_b = (0.1 * rng.standard_normal(NL)).astype(np.float32)
        # the last layer's pooled row, so that every chunk runs the last layer on all rows
        f_spec, t_spec, a_spec, r_spec = b.FeatureSpec((5, -1)), b.TopKSpec(K), b.AttentionSpec((3, -1)), b.RolloutSpec(0)
        shapes = {"cls": (2 * E, np.float32), "pooled": (2 * E, np.float32), "labels": (K, np.int32), "scores": (K, np.float32),
                  "heads": (2 * H * T, np.float32), "mean": (2 * T, np.float32), "rollout": (T, np.float32), "indices": (K, np.int32),
                  "gallery_scores": (K, np.float32), "dense_labels": (OUT[0] * OUT[1], np.uint8)}

        def arm(form, o):
            """all six, in the device ("") or the host ("_host") form, on the arrays o"""
            getattr(model, "set_features" + form)(f_spec, cls=o["cls"], pooled=o["pooled"])
            getattr(model, "set_topk" + form)(t_spec, labels=o["labels"], scores=o["scores"])
            getattr(model, "set_attention" + form)(a_spec, heads=o["heads"], mean=o["mean"])
            getattr(model, "set_rollout" + form)(r_spec, rollout=o["rollout"])
            getattr(model, "set_gallery" + form)(b.GallerySpec(K, "pooled"), d_rows, indices=o["indices"], scores=o["gallery_scores"])
            getattr(model, "set_dense" + form)(b.DenseSpec(0, OUT[0], OUT[1]), head_w, head_b, labels=o["dense_labels"])

        def disarm(form):
            for name in ("features", "topk", "attention", "rollout", "gallery", "dense"):
                getattr(model, f"set_{name}{form}")(None)

        # the device forms, chunk by chunk
        dev = {k: pkg.DeviceBuffer(MB * per, dt) for k, (per, dt) in shapes.items()}
        want = {k: np.empty((N, per), dt) for k, (per, dt) in shapes.items()}
        want["logits"], want["probs"] = np.empty((N, nc), np.float32), np.empty((N, nc), np.float32)
        d_l, d_p = pkg.DeviceBuffer(MB * nc), pkg.DeviceBuffer(MB * nc)
        arm("", dev)
        try:
            for first in range(0, N, MB):
                m = min(MB, N - first)
                d_img = pkg.DeviceBuffer.from_numpy(images[first:first + m])
                model.forward_device(d_img.ptr, m, d_l.ptr, d_p.ptr)
                model.sync()
                for k, (per, _) in shapes.items():
                    want[k][first:first + m] = dev[k].to_numpy((MB, per))[:m]
                want["logits"][first:first + m] = d_l.to_numpy((MB, nc))[:m]
                want["probs"][first:first + m] = d_p.to_numpy((MB, nc))[:m]
        finally:
            disarm("")

        # the host forms, one call
        got = {k: np.full((N, per), 0xEE if dt == np.uint8 else -7, dt) for k, (per, dt) in shapes.items()}
        arm("_host", got)
        try:
            got["logits"], got["probs"] = model.forward(images)
        finally:
            disarm("_host")
        for k in want:
            assert got[k].shape == want[k].shape and np.array_equal(bits(got[k]), bits(want[k])), k
        assert np.isfinite(want["logits"]).all() and len({r.tobytes() for r in want["logits"]}) == N   # nine different images
    finally:
        model.close()
