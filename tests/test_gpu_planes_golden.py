"""What vit_hip_export_planes writes, pinned section by section: a refactor of the file code (csrc/vit_planes_file.c), or a
change to a repack kernel that forgets to bump VIT_PLANES_LAYOUT_VERSION, must not alter a byte of it.  The golden
(tests/golden/planes_file_sha256.json, keyed by layout version) was recorded twice from the library of the commit BEFORE the
file code became a unit of its own, never from the code under test; a section whose bytes differed between those two
exports would be listed under "omitted" there and skipped here (none is)."""
import hashlib
import json
import struct
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "planes_file_sha256.json"
HEADER = "<8sIii8i4xd4QQiiQ"   # magic, header bytes, precision, n_tensors, 8 shape ints, eps, 3 slab sizes, scale floats, fold bytes, fold, version, checksum
SECTIONS = ("header", "scales", "slab_f32", "slab_operand", "slab_conv", "slab_fold")
# (file, precision, $VIT_HIP_LN_FOLD or None for the plan's own choice)
CASES = (("f32", "f32", None), ("f32_fp16x2", "f32_fp16x2", None), ("bf16", "bf16", None), ("fp8", "fp8", None), ("f32_fold", "f32", "1"))


def section_hashes(blob):
    """layout version and {section: sha256} of one planes file"""
    f = struct.unpack(HEADER, blob[:120])
    assert f[0] == b"VITPLN02" and f[1] == 120
    w_slab, operand, conv, scale_floats, fold_bytes, version = f[13], f[14], f[15], f[16], f[17], f[19]
    sizes = (120, 4 * scale_floats, w_slab, operand, conv, fold_bytes)
    assert sum(sizes) == len(blob)
    out, at = {}, 0
    for name, n in zip(SECTIONS, sizes):
        out[name] = hashlib.sha256(blob[at:at + n]).hexdigest() if n else None
        at += n
    return version, out


def export_all(pkg, monkeypatch, tmp_path):
    """{case: {section: sha256}} of the tiny shape "17 tokens, 4 heads of 64" (tests/test_gpu_configs.py) with the library's own
    synth_weights(cfg, 21), and the layout version the files carry"""
    cfg = pkg.preset("vit_b_16")
    cfg.img_size, cfg.patch_size, cfg.in_chans, cfg.num_classes = 64, 16, 3, 10
    cfg.embed_dim, cfg.depth, cfg.num_heads, cfg.mlp_hidden = 256, 2, 4, 512
    weights = pkg.synth_weights(cfg, 21)
    got, versions = {}, set()
    for name, precision, fold in CASES:
        if fold is None:
            monkeypatch.delenv("VIT_HIP_LN_FOLD", raising=False)
        else:
            monkeypatch.setenv("VIT_HIP_LN_FOLD", fold)
        m = pkg.ViTHip(cfg, weights, device=0, max_batch=2, precision=precision)
        path = tmp_path / f"{name}.planes"
        m.export_planes(path)
        m.close()
        version, got[name] = section_hashes(path.read_bytes())
        versions.add(version)
    assert len(versions) == 1
    return versions.pop(), got


def test_exported_planes_files_are_the_recorded_bytes(pkg, device, monkeypatch, tmp_path):
    golden = json.loads(GOLDEN.read_text())
    version, got = export_all(pkg, monkeypatch, tmp_path)
    assert str(version) in golden["layout_versions"], f"layout version {version} has no recorded golden: record one with the bump"
    want = golden["layout_versions"][str(version)]
    omitted = {tuple(o) for o in golden["omitted"]}
    assert not any(case in ("f32", "f32_fold", "bf16") for case, _ in omitted)   # the F32 and BF16 files at least are fully pinned
    assert set(want) == {c[0] for c in CASES}
    for case, sections in want.items():
        assert set(sections) == set(SECTIONS)
        for name in SECTIONS:
            if (case, name) not in omitted:
                assert got[case][name] == sections[name], f"{case}.planes: section {name} differs from the recording"
    # the four-slab files do hold four slabs (a fold's terms: F32 under the switch, bf16 and fp8 by default)
    assert all(want[c][s] for c in ("f32_fold", "bf16") for s in SECTIONS)
