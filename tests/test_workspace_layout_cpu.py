"""CPU (-m "not gpu"): the workspace layouts of csrc/, held to a recorded table and to a host
sanitizer run.

tests/data/workspace_bytes.json lists what every `unet_*_workspace_bytes` export answered over a
grid of arguments (tests/tools/make_workspace_table.py) before the layouts were written once per
workspace; the library under test answers every row alike, the rows that answer 0 included.

tests/tools/ws_layout_check.cpp drives the helper the layouts are written with (csrc/ws_layout.h)
under AddressSanitizer and UBSan: a few hundred region lists are measured, allocated with exactly
the measured size, carved and written through."""
import importlib.util
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _load("make_workspace_table")


def _table():
    with open(T.TABLE) as f:
        return json.load(f)


def test_table_covers_every_export_and_the_grid():
    tab = _table()
    with open(os.path.join(ROOT, "include", "unet_hip.h")) as f:
        header = f.read()
    import re
    exports = set(re.findall(r"\bsize_t (unet_\w+_workspace_bytes)\(", header))
    assert exports == set(tab), "an export without rows (or rows without an export)"
    grids = T.grids()
    for name, recorded in tab.items():
        assert [r[:-1] for r in recorded] == grids[name], f"{name}: the table is of another grid"
        assert any(r[-1] == 0 for r in recorded), f"{name}: no refused arguments in the grid"
        assert sum(1 for r in recorded if r[-1] > 0) > len(recorded) // 2, name
    # the bench shapes: 8 x 512 x 512 at 32 channels and the 16 x 16 stage at 512
    assert [8, 512 * 512, 32] in [r[:-1] for r in tab["unet_instnorm_workspace_bytes"]]
    assert [8, 16, 16, 512, 1] in [r[:-1] for r in tab["unet_conv_in_fwd_workspace_bytes"]]
    assert {r[2] for r in tab["unet_head1x1_in_bwd_fold_workspace_bytes"]} >= {2, 3, 4, 5, 21, 32}


def test_every_workspace_size_unchanged(ua):
    now = T.rows(ua.lib())
    for name, recorded in _table().items():
        bad = [(r, n[-1]) for r, n in zip(recorded, now[name]) if r != n]
        assert not bad, f"{name}: {len(bad)} sizes changed, first (row, now): {bad[0]}"


def test_fold_workspaces_are_the_pair_and_the_callee(ua):
    """The three fold exports are their callee's export plus the two [N][C] float2 blocks of the
    InstanceNorm backward, each rounded to 256 bytes - the whole of which the entry points now
    require, as their callers (ops.py sizes each by its export) have always passed."""
    lib = ua.lib()

    def up(x):
        return (x + 255) // 256 * 256

    for N in T.BATCHES:
        for s in T.SIDES:
            pair = 2 * up(N * 32 * 8)
            assert lib.unet_conv_in_bwd_weight_fold32_workspace_bytes(N, s, s) == \
                pair + lib.unet_conv3x3_bwd_weight_workspace_bytes(N, s, s, 32, 32, 1)
            assert lib.unet_stem_in_bwd_weight_fold_workspace_bytes(N, s, s, 32) == \
                pair + lib.unet_conv3x3_bwd_weight_workspace_bytes(N, s, s, 3, 32, 1)
            for K in T.CLASSES:
                assert lib.unet_head1x1_in_bwd_fold_workspace_bytes(N, s * s, K) == \
                    pair + up(lib.unet_head1x1_bwd_workspace_bytes(N, s * s, 32, K))


def test_bias_gradient_stage_fits_the_slab_workspace(ua):
    """conv_bwd_weight_impl stages the bias gradient (64 x Cout floats when N Ho Wo >= 4096) in
    the head of the slab workspace it has just checked against `need`, the size of the request's
    own plan.  Over the shapes of tests/data/wgrad_workspace_bytes.json, the three entry points
    that take `db` (fp32 tensors; fp32, bf16 and split matrix cores) are called with an empty
    workspace under each setting of the c32 switch and each chunk limit of the table: the refusal
    names `need`, and the stage fits it."""
    import re
    with open(os.path.join(ROOT, "tests", "data", "wgrad_workspace_bytes.json")) as f:
        rows = json.load(f)["conv3x3"]
    lib = ua.lib()
    P = 1 << 20       # a pointer no refused call reads
    seen, least = 0, None
    try:
        for N, H, W, Cx, Cout, stride, limit, nbytes, _ in rows:
            Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
            if N * Ho * Wo < 4096:
                continue
            lib.unet_debug_set_chunk_limit(limit)
            for name in ("unet_conv3x3_bwd_weight", "unet_conv3x3_bwd_weight_bf16",
                         "unet_conv3x3_bwd_weight_bf16x3"):
                for k in (0, 1, 2):
                    prev = lib.unet_set_c32_winograd(k)
                    rc = getattr(lib, name)(P, Cx, P, P, 0, Cx, P, P, 0, N, H, W, Cout, stride,
                                            None)
                    lib.unet_set_c32_winograd(prev)
                    assert rc != 0
                    m = re.search(r"workspace 0 < (\d+) bytes", lib.unet_last_error().decode())
                    assert m, (name, N, H, W, Cx, Cout, stride, lib.unet_last_error())
                    need = int(m.group(1))
                    if need == 0:       # one image exceeds the 2 GiB range: refused for good
                        continue
                    seen += 1
                    ratio = need / (64 * Cout * 4)
                    least = ratio if least is None else min(least, ratio)
                    assert need >= 64 * Cout * 4, (name, k, N, H, W, Cx, Cout, stride, limit, need)
    finally:
        lib.unet_debug_set_chunk_limit(0)
    assert seen > 1000
    print(f"bias-gradient stage: {seen} accepted requests, smallest need / stage = {least:.2f}")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs the HIP compiler")
def test_layout_helper_under_host_sanitizers(tmp_path):
    exe = tmp_path / "ws_layout_check"
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
             "-fno-sanitize-recover=undefined"]
    subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-x", "hip",
                    os.path.join(ROOT, "tests", "tools", "ws_layout_check.cpp"),
                    "-I", os.path.join(ROOT, "unet-implementations_amd", "csrc"),
                    *flags, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ws_layout_check ok" in out.stdout
