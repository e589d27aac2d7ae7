"""CPU (-m "not gpu"): the host-side plan selection of csrc/conv_wgrad.hip, held to a recorded
table.  tests/data/wgrad_workspace_bytes.json lists the answers of the workspace queries of the
3x3 and the up-sampled weight gradient, and of `unet_conv3x3_bwd_weight_is_winograd` under each
setting of the c32 switch, over shapes x chunk limits (tests/tools/
make_wgrad_workspace_table.py); the library under test answers every row alike.  Callers size
their workspaces by these numbers, so a changed row is a changed plan.  Rows recorded with
0 bytes (no plan) are listed but not compared."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _load("make_wgrad_workspace_table")


def _table():
    with open(T.TABLE) as f:
        return json.load(f)


def test_table_covers_the_grid():
    tab = _table()
    shapes = len(T.SIZES) * len(T.COUT) * 2 * len(T.BATCHES)       # x 2 chunk limits
    assert len(tab["conv3x3"]) == shapes * len(T.CX) * len(T.STRIDES)
    assert len(tab["up"]) == shapes * (len(T.CX) - 1)
    assert sum(1 for r in tab["conv3x3"] if r[7] > 0) > 0.9 * len(tab["conv3x3"])
    assert sum(1 for r in tab["up"] if r[6] > 0) > 0.9 * len(tab["up"])
    # both Winograd forms, the switch at "when it fills the chip" and at "always", and chunked
    # batches (which take neither form) are in it
    wino = {r[8] for r in tab["conv3x3"]}
    assert {0, 0b100, 0b110, 0b111} <= wino
    assert any(r[6] and r[0] == 8 for r in tab["conv3x3"])


def test_conv3x3_workspace_bytes_and_winograd_bit_unchanged(ua):
    lib = ua.lib()
    recorded = _table()["conv3x3"]
    rows = list(T.conv3x3_rows(lib))
    assert [key for key, _, _ in rows] == [r[:7] for r in recorded], "the table is of another grid"
    bad = [(r, nbytes) for (_, nbytes, _), r in zip(rows, recorded) if r[7] > 0 and nbytes != r[7]]
    assert not bad, f"{len(bad)} workspace sizes changed, first (row, now): {bad[0]}"
    bad = [(r, wino) for (_, _, wino), r in zip(rows, recorded) if wino != r[8]]
    assert not bad, f"{len(bad)} is_winograd answers changed, first (row, now): {bad[0]}"


def test_up_workspace_bytes_unchanged(ua):
    recorded = _table()["up"]
    rows = list(T.up_rows(ua.lib()))
    assert [key for key, _ in rows] == [r[:6] for r in recorded], "the table is of another grid"
    bad = [(r, nbytes) for (_, nbytes), r in zip(rows, recorded) if r[6] > 0 and nbytes != r[6]]
    assert not bad, f"{len(bad)} workspace sizes changed, first (row, now): {bad[0]}"


def test_chunk_limit_is_restored(ua):
    """The rows above lower the debug chunk limit; afterwards a batch runs in one launch again
    (the Winograd form takes whole batches only)."""
    lib = ua.lib()
    assert lib.unet_conv3x3_bwd_weight_is_winograd(8, 64, 64, 64, 64, 1) == 1
    with T.chunk_limit(lib, T.conv3x3_limit(64, 64, 64, 64, 1)):
        assert lib.unet_conv3x3_bwd_weight_is_winograd(8, 64, 64, 64, 64, 1) == 0
    assert lib.unet_conv3x3_bwd_weight_is_winograd(8, 64, 64, 64, 64, 1) == 1
