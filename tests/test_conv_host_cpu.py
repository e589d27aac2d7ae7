"""CPU (-m "not gpu"): the host side of the convolution forward / data-gradient entry points
(csrc/conv_igemm.hip), held to tables recorded from the library before that layer was rebuilt
around one operand-mode record, two IgemmParams builders, one chunk walk and one BSTATS binder.

tests/data/conv_host_cpu.json (tests/tools/make_conv_host_table.py) lists the answers of the pure
queries over the shape grid of the weight-gradient table, and one rejected call per validation
check reachable before the first launch: return code and `unet_last_error()` text.
tests/data/conv_host_gpu.json (tests/tools/make_conv_host_gpu_table.py) is held on the GPU by
tests/test_conv_host_gpu.py; here only its coverage is re-asserted.  The chunk walk, the builders
and the BSTATS binder themselves (csrc/conv_host.h, plain host code) run in a stand-alone program
under the host sanitizers (tests/tools/conv_host_check.cpp)."""
import importlib.util
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _load("make_conv_host_table")
G = _load("make_conv_host_gpu_table")

# Rejected calls whose error text may differ from the recording: functions this layer merged and
# whose messages differed only in the function name.  (None: the shared impl of
# unet_conv_up_in_fwd / unet_conv_up_in_fwd_b16 is given each export's name and wording.)
TEXT_EXCEPTIONS = {}


_table = T.load_table


def test_table_covers_the_grid():
    tab = _table()
    shapes = len(T.SIZES) * len(T.COUT) * 2 * len(T.BATCHES)       # x 2 chunk limits
    assert len(tab["up"]) == shapes * len(T.CX) * len(T.C1S)
    assert len(tab["workspace"]) == shapes * len(T.STRIDES)
    # supported and unsupported shapes of both fused up-sampling forwards, the c32 switch at
    # "when it fills the chip" and at "always", and chunked batches are in it
    assert {0, 0b100, 0b111} <= {r[7] for r in tab["up"]}
    assert {0, 1} == {r[8] for r in tab["up"]}
    assert {0, 0b100, 0b110} <= {r[9] for r in tab["up"]}
    assert any(r[6] and r[0] == 8 for r in tab["up"])
    assert all(r[6] > 0 for r in tab["workspace"])
    # every export of the layer has its rejected calls, none of which passed validation
    rej = tab["rejected"]
    assert sorted(r[:2] for r in rej) == sorted([n, c] for n in T.EXPORTS for c, _ in T.CASES[n])
    assert all(r[2] not in (T.UNET_OK, T.UNET_E_LAUNCH) for r in rej)
    for text in ("null pointer", "stride 3 unsupported", "kernel size 2 unsupported",
                 "must be a multiple of 32", "slice 32 of 32", "stride 2 needs even H, W",
                 "alpha without beta", "pre-split weight planes are null", "workspace too small",
                 "one image exceeds the 2 GiB", "has no fused-upsample tile"):
        assert any(text in r[3] for r in rej), text


def test_up_queries_unchanged(ua):
    recorded = _table()["up"]
    rows = list(T.up_rows(ua.lib()))
    assert [key for key, *_ in rows] == [r[:7] for r in recorded], "the table is of another grid"
    bad = [(r, now) for (_, *now), r in zip(rows, recorded) if now != r[7:]]
    assert not bad, f"{len(bad)} answers changed, first (row, now): {bad[0]}"


def test_conv_in_fwd_workspace_bytes_unchanged(ua):
    recorded = _table()["workspace"]
    rows = list(T.workspace_rows(ua.lib()))
    assert [key for key, _ in rows] == [r[:6] for r in recorded], "the table is of another grid"
    bad = [(r, n) for (_, n), r in zip(rows, recorded) if n != r[6]]
    assert not bad, f"{len(bad)} workspace sizes changed, first (row, now): {bad[0]}"


def test_rejected_calls_unchanged(ua):
    recorded = {tuple(r[:2]): r for r in _table()["rejected"]}
    rows = list(T.rejected_rows(ua.lib()))
    assert {tuple(key) for key, _, _ in rows} == set(recorded), "the table is of other calls"
    recorded = [recorded[tuple(key)] for key, _, _ in rows]
    bad = [(r, rc) for (_, rc, _), r in zip(rows, recorded) if rc != r[2]]
    assert not bad, f"{len(bad)} return codes changed, first (row, now): {bad[0]}"
    bad = [(r, text) for (key, _, text), r in zip(rows, recorded)
           if text != r[3] and tuple(key) not in TEXT_EXCEPTIONS]
    assert not bad, f"{len(bad)} error texts changed, first (row, now): {bad[0]}"
    assert len(TEXT_EXCEPTIONS) < 10


def test_switches_are_restored(ua):
    """The generators lower the debug chunk limit and turn the c32 switch; both are back."""
    lib = ua.lib()
    before = lib.unet_set_c32_winograd(1)
    lib.unet_set_c32_winograd(before)
    rows = T.up_rows(lib)
    next(rows)
    rows.close()
    assert lib.unet_set_c32_winograd(before) == before
    list(T.rejected_rows(lib))
    # (the Winograd weight gradient takes whole batches only: 1 = N = 8 runs in one launch)
    assert lib.unet_conv3x3_bwd_weight_is_winograd(8, 64, 64, 64, 64, 1) == 1


def test_gpu_table_covers_what_it_claims():
    G.assert_coverage(G.load_table())


def test_chunk_walk_builders_and_binder_under_host_sanitizers(tmp_path):
    """conv_host.h in a program of its own, AddressSanitizer + UBSan on the host side: the walk
    over N = 1, 3, 8 in one, two and three chunks with a remainder against a plain loop."""
    exe = str(tmp_path / "conv_host_check")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-g", "--offload-arch=gfx950",
                    "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "unet-implementations_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "tools", "conv_host_check.cpp"), "-o", exe],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "conv_host_check: ok" in run.stdout
