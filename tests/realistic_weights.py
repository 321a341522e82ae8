"""A seeded ViT weight set with the dynamic range of real checkpoints (a helper module of the tests, not a fixture file).

`vit_synth_tensor` (csrc/vit_config.c) fills every tensor with iid uniform values: |max|/sigma 1.73, kurtosis 1.8, no outlier
channels, residual rows with |mean|/std below 0.12.  The reference's real tensors are heavy-tailed (tests/golden/
ref_weight_stats.json: conv_proj |max|/sigma 14, out_proj up to 25, kurtosis up to 20, one class-token channel at 23 sigma).
`realistic_weights(cfg, seed)` returns the list layout of `synth_weights` with:

  * per-tensor sigma and offset of `vit_synth_tensor`, shaped heavy-tailed: a uniform value u of the
    splitmix stream (`vit_synth_fill`, bit-reproducible) becomes sign(u) (-ln(1 - |u|))^p, scaled to unit variance --
    p = 1.3 for the weight matrices (kurtosis ~12, |max|/sigma ~15 at B/16 sizes), p = 1 (Laplace) for the vectors;
  * `outliers`: four input columns of every in_proj and fc1 matrix scaled x8, x10, x12, x16 (outlier channels);
  * `cls_spike`: one class-token channel at 20 sigma;
  * `massive`: one residual channel d* (not a multiple of 32) carrying a large constant from conv bias and pos_embedding,
    fed on by amplified fc2 rows, with both LayerNorm gammas (and the final one) at 0.05 x their median on it;
  * `offset`: a row-mean offset -- a constant added to every channel of every fourth pos_embedding row, sized so that those
    rows' |mean|/std at the embedding is `offset`, and a small per-layer constant on the out_proj and fc2 biases.

Why the offset sits on a quarter of the rows: one residual row cannot show both exposures at once.  With mean c and a
channel of A, mean^2 + var >= A^2 / E, and median|x| is about |c| when the row is offset; |x[d*]| / median|x| >= 50 then
forces |mean|/std <= sqrt(E) / 50 (0.55 at E = 768).  So the offset rows carry the cancellation (max |mean|/std 3-6) and
the others the massive channel (median over rows of |x[d*]| / median|x| >= 50); d* sits in every row.

Only fixed float64 transforms, rounded to fp32 once; no np.random.  `weights_sha256` pins the result: a numpy whose log or
power rounds differently fails the stored digests on the CPU, not as a parity miss on a GPU."""
from __future__ import annotations

import hashlib
import math
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

P_MATRIX = 1.3
P_VECTOR = 1.0
OUTLIER_GAINS = (8.0, 10.0, 12.0, 16.0)
FC2_ROW_GAIN = 2.0
GAMMA_AT_DSTAR = 0.05          # x the median of the gamma vector
BIAS_DRIFT = 0.1               # per layer, on out_proj and fc2 biases, x the bulk sigma of an embedding row
MASSIVE_GROWTH = 0.1           # per layer, on fc2 bias at d*, x the massive value A
OFFSET_ROW_PERIOD = 4          # every 4th token row (1, 5, 9, ...) carries the offset
CLS_SPIKE_SIGMA = 20.0
IMAGE_SIGMA = 2.0 / math.sqrt(3.0)   # vit_synth_image: uniform in [-2, 2)

_ORACLE = None


def _uniform(count: int, seed: int) -> np.ndarray:
    """splitmix stream `seed` (vit_synth_fill, scale 1, offset 0): exact values in [-1, 1), float64"""
    global _ORACLE
    if _ORACLE is None:
        from oracle.oracle import Oracle
        _ORACLE = Oracle("vit_b_16")
    return _ORACLE.synth_fill(count, seed, 1.0, 0.0).astype(np.float64)


def _heavy(count: int, seed: int, p: float) -> np.ndarray:
    """unit-variance, symmetric, heavy-tailed: sign(s) E^p with E = -ln(1 - |s|) exponential, s uniform in (-1, 1)"""
    s = _uniform(count, seed) + 2.0 ** -24          # [-1, 1) -> (-1, 1): the tail stays finite (at most 16.6^p)
    return np.sign(s) * (-np.log1p(-np.abs(s))) ** p / math.sqrt(math.gamma(1.0 + 2.0 * p))


def _role(cfg, idx: int) -> tuple[str, float, float]:
    """(role, sigma, offset): vit_synth_tensor's uniform scale / sqrt(3) and its offset, per tensor index"""
    tail = 4 + 12 * cfg.depth
    table = {0: ("cls", 0.02, 0.0), 1: ("conv_w", 0.016, 0.0), 2: ("conv_b", 0.05, 0.0), 3: ("pos", 0.088, 0.0)}
    if idx in table:
        r, s, o = table[idx]
    elif idx >= tail:
        r, s, o = [("final_g", 0.2, 0.7), ("final_b", 0.05, 0.0), ("head_w", 0.064, 0.0), ("head_b", 0.035, 0.0)][idx - tail]
    else:
        r, s, o = [("ln1_g", 0.25, 0.3), ("ln1_b", 0.05, 0.0), ("in_w", 0.04, 0.0), ("in_b", 0.1, 0.0), ("out_w", 0.043, 0.0),
                   ("out_b", 0.035, 0.0), ("ln2_g", 0.25, 0.3), ("ln2_b", 0.05, 0.0), ("fc1_w", 0.04, 0.0),
                   ("fc1_b", 0.035, -0.026), ("fc2_w", 0.04, 0.0), ("fc2_b", 0.02, 0.0)][(idx - 4) % 12]
    return r, s / math.sqrt(3.0), o


def tensor_sizes(cfg) -> list[int]:
    E, F, P, C = cfg.embed_dim, cfg.mlp_hidden, cfg.patch_size, cfg.in_chans
    T = (cfg.img_size // P) ** 2 + 1
    layer = [E, E, 3 * E * E, 3 * E, E * E, E, E, E, F * E, F, E * F, E]
    return [E, E * C * P * P, E, T * E] + layer * cfg.depth + [E, E, cfg.num_classes * E, cfg.num_classes]


def massive_channel(cfg, seed: int = 0) -> int:
    """d*: a channel index that is not a multiple of 32 (fixed by the seed; its stream lies above every tensor index and
    every outlier stream, 0x5000 + idx and 0x6000 + idx + col)"""
    u = _uniform(2, (seed << 20) + 0xF000)
    block = int((u[0] + 1.0) * 0.5 * (cfg.embed_dim // 32))
    return 32 * block + 1 + int((u[1] + 1.0) * 0.5 * 31)


def embedding_sigma(cfg) -> float:
    """the standard deviation of an embedding row's bulk (no massive channel, no offset) on synthetic images"""
    K = cfg.in_chans * cfg.patch_size ** 2
    conv = math.sqrt(K) * IMAGE_SIGMA * _role(cfg, 1)[1]
    return math.sqrt(conv ** 2 + _role(cfg, 3)[1] ** 2 + _role(cfg, 2)[1] ** 2)


def plan(cfg, seed: int = 0, offset: float = 5.0, massive: float = 90.0) -> dict:
    """The constants the features use: d*, the massive value A, the offset rows' constant c and the per-layer drift."""
    sig = embedding_sigma(cfg)
    A = massive * 0.6745 * sig                                         # 0.6745 sigma: the median |x| of the bulk
    row_sd = math.sqrt(sig * sig + A * A / cfg.embed_dim)
    c = offset * row_sd
    return {"dstar": massive_channel(cfg, seed) if massive > 0 else -1, "A": A, "c": c, "drift": BIAS_DRIFT * sig,
            "bulk_sigma": sig}


def realistic_weights(cfg, seed: int = 0, *, offset: float = 5.0, massive: float = 90.0, outliers: bool = True,
                      cls_spike: bool = True) -> list[np.ndarray]:
    """-> float32 arrays in the layout of synth_weights(cfg, .).  offset: the offset rows' |mean|/std at the embedding
    (0: none); massive: |x[d*]| / median|x| at the embedding (0: no massive channel)."""
    E, F, D = cfg.embed_dim, cfg.mlp_hidden, cfg.depth
    pl = plan(cfg, seed, offset, massive)
    ds = pl["dstar"]
    T = (cfg.img_size // cfg.patch_size) ** 2 + 1
    out = []
    for idx, n in enumerate(tensor_sizes(cfg)):
        role, sig, off = _role(cfg, idx)
        stream = (seed << 20) + idx
        if role.endswith("_g"):                                    # LayerNorm gamma: the synthetic set's uniform shape
            v = off + sig * math.sqrt(3.0) * _uniform(n, stream)
            if ds >= 0:
                v[ds] = GAMMA_AT_DSTAR * float(np.median(np.abs(v)))
        else:
            is_matrix = role.endswith("_w")
            v = off + sig * _heavy(n, stream, P_MATRIX if is_matrix else P_VECTOR)
        if role == "cls" and cls_spike:
            v[(ds + E // 2) % E if ds >= 0 else E // 2] = CLS_SPIKE_SIGMA * sig
        if role in ("in_w", "fc1_w") and outliers:
            m = v.reshape(-1, E)
            pick = _uniform(len(OUTLIER_GAINS), stream + 0x5000)
            for g, u in zip(OUTLIER_GAINS, pick):
                col = int((u + 1.0) * 0.5 * E)
                if col == ds:
                    col = (col + 1) % E
                m[:, col] = g * sig * math.sqrt(3.0) * _uniform(m.shape[0], stream + 0x6000 + col)
        if ds >= 0:
            if role == "conv_b":
                v[ds] += 0.5 * pl["A"]
            elif role == "pos":
                p = v.reshape(T, E)
                p[1:, ds] += 0.5 * pl["A"]
                p[0, ds] += pl["A"]                               # the class row has no conv bias
            elif role == "fc2_w":
                v.reshape(E, F)[ds] *= FC2_ROW_GAIN
            elif role == "fc2_b":
                v[ds] += MASSIVE_GROWTH * pl["A"]                # the MLP keeps writing into d*, as in trained ViTs
        if offset:
            if role == "pos":
                v.reshape(T, E)[1::OFFSET_ROW_PERIOD] += pl["c"]
            elif role in ("out_b", "fc2_b"):
                v += pl["drift"]
        out.append(v.astype(np.float32))
    assert len(out) == 4 + 12 * D + 4
    return out


def weights_sha256(ws: list[np.ndarray]) -> str:
    h = hashlib.sha256()
    for a in ws:
        h.update(np.ascontiguousarray(a, dtype=np.float32).tobytes())
    return h.hexdigest()


def tensor_stats(a: np.ndarray) -> dict:
    a = np.asarray(a, dtype=np.float64).ravel()
    c = a - a.mean()
    s = math.sqrt(float((c * c).mean()))
    return {"sigma": s, "max_over_sigma": float(np.abs(a).max()) / s, "kurtosis": float((c ** 4).mean()) / s ** 4}


def exposure(cfg, ws: list[np.ndarray], images: np.ndarray, dstar: int) -> dict:
    """float64 restatement of ViT_seq.c up to every LayerNorm input (ln_1, ln_2 of each layer, then the final one):
    per LayerNorm input, over all rows of all images, max and median of |mean|/std and the median over rows of
    |x[d*]| / median|x|.  -> {"mean_std_max": [2 L + 1], "mean_std_median": [...], "massive_ratio": [...]}"""
    import torch
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))   # noqa: E731
    E, H, L, P = cfg.embed_dim, cfg.num_heads, cfg.depth, cfg.patch_size
    Dh = E // H
    w = [t(a) for a in ws]
    x = torch.nn.functional.conv2d(t(images), w[1].reshape(E, cfg.in_chans, P, P), w[2], stride=P).flatten(2).transpose(1, 2)
    x = torch.cat([w[0].reshape(1, 1, E).expand(x.shape[0], 1, E), x], dim=1) + w[3].reshape(1, -1, E)
    rec = {"mean_std_max": [], "mean_std_median": [], "massive_ratio": []}

    def note(x):
        r = x.reshape(-1, E)
        mean = r.mean(1)
        sd = ((r * r).mean(1) - mean * mean).clamp(min=0).sqrt()
        ms = (mean.abs() / sd).numpy()
        rec["mean_std_max"].append(float(ms.max()))
        rec["mean_std_median"].append(float(np.median(ms)))
        if dstar >= 0:
            ratio = r[:, dstar].abs() / r.abs().median(dim=1).values
            rec["massive_ratio"].append(float(ratio.median()))
        else:
            rec["massive_ratio"].append(0.0)

    def ln(x, g, b):
        mean = x.mean(-1, keepdim=True)
        var = (x * x).mean(-1, keepdim=True) - mean * mean
        return (x - mean) / (var + cfg.eps).sqrt() * g + b

    with torch.no_grad():
        for layer in range(L):
            lw = w[4 + 12 * layer: 16 + 12 * layer]
            note(x)
            qkv = ln(x, lw[0], lw[1]) @ lw[2].reshape(3 * E, E).T + lw[3]
            B, T, _ = qkv.shape
            q, k, v = (a.reshape(B, T, H, Dh).transpose(1, 2) for a in qkv.split(E, dim=2))
            a = (torch.softmax(q @ k.transpose(2, 3) / math.sqrt(Dh), dim=-1) @ v).transpose(1, 2).reshape(B, T, E)
            x = x + a @ lw[4].reshape(E, E).T + lw[5]
            note(x)
            h = ln(x, lw[6], lw[7]) @ lw[8].reshape(-1, E).T + lw[9]
            h = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
            x = x + h @ lw[10].reshape(E, -1).T + lw[11]
        note(x)
    return rec
