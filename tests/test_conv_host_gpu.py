"""GPU: the convolution forward / data-gradient entry points of csrc/conv_igemm.hip, held to
what the library did before their host side was rebuilt around one operand-mode record, two
IgemmParams builders, one chunk walk and one BSTATS binder.

tests/data/conv_host_gpu.json (tests/tools/make_conv_host_gpu_table.py, recorded on an MI355X from
a build of the parent commit; every row identical in two runs) lists per call the demangled launch
list, the reported stats_px / tiles_out and a CRC32 of every output the call writes.  The inputs
are seeded on the CPU and the kernels use no atomics, so the library under test reproduces all
three columns exactly: the same kernels on the same IgemmParams.  The output bits of the seven
rows that launch conv_patch_split_kernel were recorded again when that kernel moved its five
correction products into a second accumulator (launch lists and reports unchanged; the results
themselves are held to fp64 by tests/test_bf16x3_step_kernels_gpu.py).  One test per export family;
tests/test_conv_host_cpu.py re-asserts the coverage of the table."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load("make_conv_host_gpu_table")
_cache = {}


def _recorded():
    if not _cache:
        _cache.update({r["id"]: r for r in G.load_table()})
    return _cache


@pytest.mark.parametrize("fam", G.FAMILIES)
def test_launches_reports_and_output_bits_unchanged(ua, fam):
    recorded = _recorded()
    bad = []
    for row in G.ROWS:
        if row["fam"] != fam:
            continue
        names, report, crc = G.run_row(ua, row)
        want = recorded[row["id"]]
        if names != want["launches"]:
            bad.append((row, "launches", names, want["launches"]))
        elif report != want["report"]:
            bad.append((row, "stats_px / tiles_out", report, want["report"]))
        elif crc != want["crc"]:
            bad.append((row, "output bits", crc, want["crc"]))
    assert not bad, f"{len(bad)} rows changed, first (row, column, now, recorded): {bad[0]}"
