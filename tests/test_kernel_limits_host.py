"""csrc/kernel_limits.h without a device: tests/kernel_limits_main.c prints every constant and every function of the header
over a sweep.  Built as C11 with -Wall -Wextra -Wpedantic (no warning) under AddressSanitizer and UBSan, and once more as
C++17, which must print the same.  The loaded library's exported sizing and limit entries (no device is touched) are held
against every line: each still forwards to the header.  The header's constants are held against the restatements the
Python references keep, and every launcher that refuses on one of them refuses limit + 1 before it touches a device."""
import subprocess
from pathlib import Path

import pytest

import attn_tiles_ref

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "vit-with-opencl_amd" / "csrc"
SRC = ROOT / "tests" / "kernel_limits_main.c"
INC = [f"-I{ROOT / 'include'}", f"-I{CSRC}"]
WARN = ["-Wall", "-Wextra", "-Wpedantic"]
FLAGS = ["-O1", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-ffp-contract=off", "-fsanitize=address,undefined",
         "-fno-omit-frame-pointer"]
ENV = {"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


def build_and_run(exe, compiler):
    build = subprocess.run([*compiler, *WARN, *INC, str(SRC), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    assert "warning" not in build.stderr, build.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    return r.stdout


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    """the program's lines as (name, arguments, results), and its constants by name"""
    out = build_and_run(tmp_path_factory.mktemp("limits") / "kernel_limits_main", ["gcc", *FLAGS])
    lines, consts = [], {}
    for ln in out.splitlines():
        left, right = ln.split(" : ")
        name, *args = left.split()
        if name == "const":
            consts[args[0]] = int(right)
        else:
            lines.append((name, tuple(map(int, args)), tuple(map(int, right.split()))))
    return out, lines, consts


def test_the_header_is_cxx17_too_and_says_the_same(sweep, tmp_path):
    assert build_and_run(tmp_path / "kernel_limits_main_cxx", ["g++", "-x", "c++", "-std=c++17"]) == sweep[0]


def test_the_constants_are_the_references(sweep):
    _, lines, c = sweep
    assert c["KL_LDS_BYTES"] == 160 * 1024
    assert c["KL_ATTN_HD64_MAX_TOKENS"] == attn_tiles_ref.HD64_LIMIT == max(t for _, t in attn_tiles_ref.HD64_TABLE)
    assert c["KL_ATTN_STREAMING_MAX_TOKENS"] == attn_tiles_ref.TILED_LIMIT == max(max(v) for v in attn_tiles_ref.TILED_TABLE.values())
    assert max(attn_tiles_ref.H16_T) <= c["KL_ATTN_HD80_MAX_TOKENS"] == 16 * 17
    assert (c["KL_FOLD_GROUP"], c["KL_FOLD_MAX_GROUPS"], c["KL_PATCH_PLANES_K_STEP"], c["KL_PATCH_ROWS_K_STEP"]) == (128, 16, 128, 32)
    assert (c["KL_CLS_ATTN_MAX_HEAD_DIM"], c["KL_GALLERY_ROW_TILE"], c["KL_GALLERY_MAX_EMBED"], c["KL_DENSE_MAX_EMBED"]) == (128, 128, 2048, 2048)
    assert (c["KL_ROLLOUT_QUERY_ROWS"], c["KL_ROLLOUT_KEY_CHUNK"], c["KL_READOUT_ROWS"], c["KL_LN_PLANES_ROWS"]) == (16, 64, 32, 16)
    got = {(name, args): res for name, args, res in lines}
    # what the public headers and DESIGN.md quote
    assert got[("ln_planes", (1,))] == (2048,) and got[("ln_planes", (3,))] == (1696,) and got[("ln_planes", (2,))] == (0,)
    assert got[("head_dim", (128,))] == (0, 1, 1856) and got[("head_dim", (64,))] == (1, 1, 2176) and got[("head_dim", (80,))][:2] == (1, 1)
    assert got[("head_dim", (144,))][:2] == (0, 0) and got[("head_dim", (24,))][:2] == (0, 0)
    # the most tokens of the rollout is the last whole key chunk whose score rows fit the LDS
    for (name, (T, D)), (stride, lds) in ((k, v) for k, v in got.items() if k[0] == "rollout_lds"):
        most = got[("head_dim", (D,))][2]
        assert stride == -(-T // 64) * 64 + 20 and lds == (16 * stride + 80 * (D + 4)) * 4
        assert (lds <= c["KL_LDS_BYTES"]) == (T <= most), (T, D)
    # B/16 gathers on load, H/14 goes through a workspace of zero-padded rows, K = 588 padded to 608
    assert got[("patch_rows", (16, 3, 224, 224, 16, 768))] == (1, 0)
    assert got[("patch_rows", (16, 3, 224, 224, 14, 1280))] == (0, (16 * 256 + 1280) * 608 * 4)
    assert got[("patch_rows", (16, 3, 224, 336, 14, 1280))] == (0, (16 * 16 * 24 + 1280) * 608 * 4)
    assert got[("patch_planes_k", (3, 14))] == (640,) and got[("patch_planes_k", (3, 16))] == (768,)
    # the cap on the gallery's splits takes over at 128 x 1024 rows
    assert got[("gallery", (3, 131072, 4, 0))] == got[("gallery", (3, 131073, 4, 0))] == got[("gallery", (3, 2147483647, 4, 0))] == (3 * 1024 * 4 * 8,)
    assert got[("gallery", (3, 130945, 4, 0))] == (3 * 1024 * 4 * 8,) and got[("gallery", (3, 130944, 4, 0))] == (3 * 1023 * 4 * 8,)


def test_every_exported_entry_forwards_to_the_header(sweep, pkg):
    L = pkg.lib()
    entry = {
        "ln_planes": lambda parts: (L.vh_layer_norm_planes_max_embed(parts),),
        "patch_planes_k": lambda chans, patch: (L.vh_patch_planes_k(chans, patch),),
        "mx_scale": lambda rows, cols: (L.vh_mx_act_scale_bytes(rows, cols),),
        "rollout_ws": lambda n, T: (L.vh_rollout_workspace(n, T),),
        "gallery": lambda q, n_rows, k, splits: (L.vh_gallery_workspace(q, n_rows, k, splits),),
        "readout": lambda n, T, E: (L.vh_feature_readout_scratch(n, T, E),),
        "stitch": lambda n, h, w, ids: (L.vh_dense_stitch_scratch(n, h, w, ids),),
    }
    seen = {}
    for name, args, res in sweep[1]:
        if name == "head_dim":      # (the long kernel's head dims have no entry of their own)
            assert (L.vh_cls_attention_head_dim_ok(*args), L.vh_rollout_max_tokens(*args)) == res[1:], (name, args)
        elif name == "patch_rows":  # the rectangular entry, and the square one wherever the image is square
            assert L.vh_patch_embed_workspace_hw(*args) == res[1], (name, args)
            n, chans, h, w, patch, E = args
            if h == w:
                assert L.vh_patch_embed_workspace(n, chans, h, patch, E) == res[1], (name, args)
                seen["patch_rows_square"] = seen.get("patch_rows_square", 0) + 1
        elif name == "rollout_lds":
            continue
        else:
            assert entry[name](*args) == res, (name, args)
        seen[name] = seen.get(name, 0) + 1
    assert set(seen) == set(entry) | {"head_dim", "patch_rows", "patch_rows_square"} and all(n >= 5 for n in seen.values()), seen
    assert sum(seen.values()) > 3000


A, B, C3 = 0x10000, 0x20000, 0x30000      # 16-byte aligned stand-ins for device pointers: a refusal reads none of them


@pytest.mark.parametrize("entry,name", [("vh_launch_attention_planes", "KL_ATTN_HD64_MAX_TOKENS"),
                                        ("vh_launch_attention_planes_f16", "KL_ATTN_HD64_MAX_TOKENS"),
                                        ("vh_launch_attention_planes_cls", "KL_ATTN_HD64_MAX_TOKENS"),
                                        ("vh_launch_attention_planes_f16_hd80", "KL_ATTN_HD80_MAX_TOKENS"),
                                        ("vh_launch_attention_planes_f16_hd80_operand", "KL_ATTN_HD80_MAX_TOKENS"),
                                        ("vh_launch_attention", "KL_ATTN_STREAMING_MAX_TOKENS"),
                                        ("vh_launch_cls_attention", "KL_CLS_ATTN_MAX_HEAD_DIM"),
                                        ("vh_launch_rollout_step", "rollout")])
def test_a_launcher_refuses_limit_plus_one_before_any_device_call(sweep, pkg, entry, name):
    """Every argument but the one past its limit is one the launcher takes (the limit itself passes these checks: the GPU
    suite launches it), and the argument checks of each of these launchers stand in front of its first device call."""
    L, c = pkg.lib(), sweep[2]
    if name == "rollout":
        limit = L.vh_rollout_max_tokens(64)
        assert limit == dict(((n, a), r) for n, a, r in sweep[1])[("head_dim", (64,))][2]
    else:
        limit = c[name]
    over = limit + 16 if name == "KL_CLS_ATTN_MAX_HEAD_DIM" else limit + 1      # the next multiple of 16: 144
    hd = 80 if "hd80" in entry else 64
    call = {
        "vh_launch_attention_planes": lambda: L.vh_launch_attention_planes(None, A, B, 2, over, 2 * hd, 2),
        "vh_launch_attention_planes_f16": lambda: L.vh_launch_attention_planes_f16(None, A, B, 1, 2, over, 2 * hd, 2),
        "vh_launch_attention_planes_cls": lambda: L.vh_launch_attention_planes_cls(None, A, B, C3, 2, over, 2 * hd, 2),
        "vh_launch_attention_planes_f16_hd80": lambda: L.vh_launch_attention_planes_f16_hd80(None, A, B, 2, over, 2 * hd, 2),
        "vh_launch_attention_planes_f16_hd80_operand":
            lambda: L.vh_launch_attention_planes_f16_hd80_operand(None, A, B, None, 1, 2, over, 2 * hd, 2),
        "vh_launch_attention": lambda: L.vh_launch_attention(None, A, B, 2, over, 2 * hd, 2),
        "vh_launch_cls_attention": lambda: L.vh_launch_cls_attention(None, A, 0, 2, 17, 2 * over, 2, 0, 1, B, C3),
        "vh_launch_rollout_step": lambda: L.vh_launch_rollout_step(None, A, 0, 2, over, 2 * hd, 2, B, C3, A + 0x100000),
    }[entry]
    L.vh_set_error(1, b"stale")
    assert call() == 1
    msg = L.vh_last_error().decode()
    what = "head_dim=" if name == "KL_CLS_ATTN_MAX_HEAD_DIM" else "tokens="
    assert (entry in msg or msg.startswith("vh_launch_attention:")) and f"{what}{over}" in msg, msg
    assert str(limit) in msg, msg              # the message quotes the limit
