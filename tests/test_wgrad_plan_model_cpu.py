"""CPU (-m "not gpu"): tests/tools/wgrad_plan_model.py, the Python statement of the
weight-gradient plan rule of csrc/conv_wgrad.hip, held to what the library has answered, and the
table of tests/test_wgrad_fp64_gpu.py held to the model - so that a row with a wrong expected
kernel, a missing instantiation or an edge the plan does not have is found without a GPU.
  * every row of tests/data/wgrad_workspace_bytes.json (recorded from the library; unchanged):
    the model gives the recorded workspace bytes - the maximum over the seven requests of
    unet_conv3x3_bwd_weight_workspace_bytes, and the up query - and the recorded is_winograd
    bits.  That ties split, S and the form choice of the model to the library's answers;
  * the kernel column of the 31 CASES of tests/test_wgrad_defer_gpu.py, which has run on the
    MI355X, and the stage count each case queues;
  * every row of tests/test_wgrad_fp64_gpu.py::ROWS: the model gives the launches the row states;
  * the name set of the model's grid equals the name set of the table, and no name of
    UNREACHABLE is in it;
  * every edge a row is there for, from the model's plan fields."""
import importlib.util
import json
import os

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))


def _load(name, *where):
    spec = importlib.util.spec_from_file_location(name, os.path.join(TESTS, *where, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _load("test_wgrad_fp64_gpu")
M, ROWS, request = T.M, T.ROWS, T.request


def bias_launches(row):
    """conv_bwd_weight_impl: one bias_grad_kernel launch below 4096 pixels, two from there on"""
    Ho, Wo = (row.H - 1) // row.stride + 1, (row.W - 1) // row.stride + 1
    return ("bias_grad_kernel",) * ((2 if row.N * Ho * Wo >= 4096 else 1) if row.db else 0)


# --------------------------------------------------------------------------- against the library
def _table():
    with open(os.path.join(TESTS, "data", "wgrad_workspace_bytes.json")) as f:
        return json.load(f)


def test_model_reproduces_the_recorded_workspace_bytes():
    bad = []
    rows = _table()["conv3x3"]
    for N, H, W, Cx, Cout, stride, limit, nbytes, _ in rows:
        got = M.workspace_bytes(N, H, W, Cx, Cout, stride, limit)
        if got != nbytes:
            bad.append(((N, H, W, Cx, Cout, stride, limit), nbytes, got))
    assert len(rows) > 3000
    assert not bad, f"{len(bad)} of {len(rows)} rows differ, first (row, recorded, model): {bad[0]}"


def test_model_reproduces_the_recorded_winograd_bits():
    bad = []
    for N, H, W, Cx, Cout, stride, limit, _, wino in _table()["conv3x3"]:
        got = sum(M.is_winograd(N, H, W, Cx, Cout, stride, k, limit) << k for k in (0, 1, 2))
        if got != wino:
            bad.append(((N, H, W, Cx, Cout, stride, limit), wino, got))
    assert not bad, f"{len(bad)} rows differ, first (row, recorded, model): {bad[0]}"


def test_model_reproduces_the_recorded_up_workspace_bytes():
    bad = []
    rows = _table()["up"]
    for N, h, w, Cx, Cout, limit, nbytes in rows:
        got = M.up_workspace_bytes(N, h, w, Cx, Cout, limit)
        if got != nbytes:
            bad.append(((N, h, w, Cx, Cout, limit), nbytes, got))
    assert len(rows) > 1000
    assert not bad, f"{len(bad)} of {len(rows)} rows differ, first (row, recorded, model): {bad[0]}"


def _defer_cases():
    return _load("test_wgrad_defer_gpu").CASES


def _defer_request(s):
    mode = {"fp32": ("fp32", 0), "bf16": ("fp32", 1), "x3": ("fp32", 3), "b16": ("bf16", 1)}[s.mode]
    c32 = 2 if s.c32 == "always" else 1      # (Layer._call: True unless the case says)
    return M.Request(s.entry, mode[0], mode[1], s.entry in ("in", "up"), s.N, s.H, s.W, s.Cx,
                     s.Cout, s.stride, s.ks == 1, c32, s.chunk)


def test_model_reproduces_the_kernel_column_of_the_defer_cases():
    cases = _defer_cases()
    assert len(cases) == 31
    for name, s in cases.items():
        r = _defer_request(s)
        assert M.names(r) == s.kernel, f"{name}: the model launches {M.names(r)}"
        assert M.reduction_stages(r) == s.stages, name


# --------------------------------------------------------------------------- the table
@pytest.mark.parametrize("name", list(ROWS))
def test_row_states_the_launches_the_model_gives(name):
    row = ROWS[name]
    want = M.names(request(row)) + bias_launches(row)
    assert row.kernel == want, f"{name}: the model gives\n{want}\nplan {M.launches(request(row))}"
    assert name.split(":")[0] == T.family(row.kernel[0])


def _table_names():
    return {k for row in ROWS.values() for k in row.kernel if k != "bias_grad_kernel"}


def test_table_names_equal_the_grid_names():
    grid = set(M.grid_names())
    table = _table_names()
    assert not grid - table, f"instantiations of the grid without a row: {sorted(grid - table)}"
    assert not table - grid, f"rows for names the grid does not reach: {sorted(table - grid)}"
    assert len(grid) == 138
    # the tap entries (18) and the stem (6) are among them
    assert sum("taps" in n for n in grid) == 18 and sum("stem" in n for n in grid) == 6


def test_unreachable_names_are_not_reached():
    dead = [n for names in T.UNREACHABLE.values() for n in names]
    assert len(dead) == len(set(dead)) == 22
    assert not set(dead) & set(M.grid_names())
    # a wider sweep than the grid: larger and odd sizes, centre-tap requests, chunked batches
    seen = set()
    for entry, storage, cores, act in M.GRID_MODES + M.TAP_MODES:
        for stride in ((1,) if entry == "up" else (1, 2)):
            for Cx in (32, 64, 96, 128, 512):
                for Cout in (32, 64, 96, 128, 512):
                    for N, H, W in ((1, 2, 2), (1, 7, 9), (2, 50, 40), (8, 64, 64), (5, 33, 200),
                                    (8, 512, 512)):
                        for center in ((False,) if entry == "up" or stride == 2 else (False, True)):
                            for chunk in (0, 2):
                                if center and entry == "conv3x3":
                                    continue
                                r = M.Request(entry, storage, cores, act, N, H, W, Cx, Cout,
                                              stride, center, 1, chunk)
                                if M.wgrad_select(r).nmax >= 1:     # (an image within 2 GiB)
                                    seen.update(M.names(r))
    assert not set(dead) & seen


# --------------------------------------------------------------------------- the edges
def _launch(row):
    return M.launches(request(row))


def _out(row):
    return (row.H - 1) // row.stride + 1, (row.W - 1) // row.stride + 1


def _ragged(row, ls):
    """whole segments and then a short one: the tail behind full segments"""
    if row.entry in ("up", "stem", "u8"):      # segments of the flat pixel list (stem: 128)
        return all(l.total_segs > 1 and (l.N * row.H * row.W) % l.S != 0 for l in ls)
    return all(l.segs_per_row > 1 and _out(row)[1] % l.S != 0 for l in ls)


def _rows_of(row, l, Ho, Wo):
    """the launch walks l.N images of Ho rows of ceil(Wo / S) segments"""
    return l.segs_per_row == M.ceil_div(Wo, l.S) and l.total_segs == l.N * Ho * l.segs_per_row


EDGES = {
    "a ragged last segment": _ragged,
    "a short last workgroup":
        lambda row, ls: all(l.total_segs % l.segs_per_block != 0 and l.split > 1 for l in ls),
    "N = 3": lambda row, ls: len(ls) == 1 and ls[0].N == 3 and ls[0].total_segs == (
        M.ceil_div(3 * row.H * row.W, ls[0].S) if row.entry in ("up", "stem") else
        3 * (row.H // 2) * ls[0].segs_per_row if "wino_kernel" in ls[0].name else
        3 * (row.H // 8) * ls[0].segs_per_row if "wino32" in ls[0].name else
        3 * _out(row)[0] * ls[0].segs_per_row),
    "a column slice with off > 0 and extra > 0": lambda row, ls: row.off > 0 and row.extra > 0,
    "more than one column strip, the last one ragged":
        lambda row, ls: all(l.rg >= 1 and l.segs_per_row > 1 and
                            ((row.W - 1) // row.stride + 1) % l.S != 0 for l in ls),
    "a chunked batch, 2 + 1 images, activation on load":
        lambda row, ls: row.act and [l.N for l in ls] == [2, 1],
    "odd H and W at stride 2: Ho = 13, Wo = 21":
        lambda row, ls: row.stride == 2 and all(_rows_of(row, l, 13, 21) for l in ls),
    "odd W at stride 2, Wo = 21 (an odd Ho has no whole ring rounds)":
        lambda row, ls: row.stride == 2 and all(
            l.rg >= 1 and _rows_of(row, l, _out(row)[0], 21) for l in ls),
}
FAMILIES = ("fp32-4wave", "fp32-8wave", "wino", "wino32", "bf16x3", "bf16-cores", "b16-ring",
            "b16-segments", "b16-fp32cores", "taps-4wave", "taps-8wave", "taps-b16",
            "taps-b16-fp32cores", "stem")
STRIDE2 = ("fp32-4wave", "fp32-8wave", "b16-ring", "b16-segments", "b16-fp32cores")
# where an edge cannot occur, with the reason
NOT_APPLICABLE = {
    "a ragged last segment": {
        "wino": "wgrad_wino_ok takes W % 16 == 0 only", "wino32": "W % 32 == 0 only"},
    "a short last workgroup": {
        "b16-ring": "wgrad_ring_ok requires total_segs % segs_per_block == 0",
        "wino32": "segs_per_block = 1",
        "stem": "stem_spb = 1 below 1024 stages of 128 pixels (N H W = 131072)"},
    "a column slice with off > 0 and extra > 0": {
        "stem": "conv_bwd_weight_impl takes the stem with Cin_total == 3 and ci_offset == 0 only"},
    "a chunked batch, 2 + 1 images, activation on load": {
        "wino": "the Winograd forms take whole batches", "wino32": "as wino",
        "bf16-cores": "unet_conv3x3_bwd_weight_bf16 has no activation",
        "stem": "the stem is not walked in chunks and has no activation"},
}


def _families_with(edge):
    return {name.split(":")[0] for name, row in ROWS.items() if row.edge == edge}


@pytest.mark.parametrize("name", [n for n, r in ROWS.items() if r.edge in EDGES])
def test_row_has_the_edge_it_is_there_for(name):
    row = ROWS[name]
    assert EDGES[row.edge](row, _launch(row)), f"{name}: not '{row.edge}': {_launch(row)}"


@pytest.mark.parametrize("edge", ["a ragged last segment", "a short last workgroup", "N = 3",
                                  "a column slice with off > 0 and extra > 0",
                                  "a chunked batch, 2 + 1 images, activation on load"])
def test_edge_has_a_row_in_every_family(edge):
    have = _families_with(edge)
    na = NOT_APPLICABLE.get(edge, {})
    assert not have & set(na), "a row for an edge declared impossible"
    assert have | set(na) == set(FAMILIES), sorted(set(FAMILIES) - have - set(na))


def test_no_row_repeats_another():
    """an edge row is a case of its own: no two rows make the same call on the same operands"""
    seen = {}
    for name, row in ROWS.items():
        key = row._replace(edge="", kernel=())
        assert key not in seen, f"{name} repeats {seen[key]}"
        seen[key] = name


def test_instantiations_held_before_this_table():
    """The launch-asserted float64 verdicts that existed before: the kernel columns of the defer
    cases and of the three per-layer tables hold 38 weight-gradient instantiations, all among the
    138 of this table."""
    def short(n):
        return T.short_name(n.replace("unet_conv::(anonymous namespace)::", ""))

    held = {k for s in _defer_cases().values() for k in s.kernel}
    for mod in ("test_fp32_step_kernels_gpu", "test_bf16x3_step_kernels_gpu",
                "test_bf16_bench_layers_gpu"):
        held |= {short(n) for r in _load(mod).LAYERS for n in r[4]
                 if "wgrad" in n and "reduce" not in n}
    assert len(held) == 38
    assert held <= _table_names()


def test_remaining_edges():
    odd = _families_with("odd H and W at stride 2: Ho = 13, Wo = 21") | \
        _families_with("odd W at stride 2, Wo = 21 (an odd Ho has no whole ring rounds)")
    assert odd == set(STRIDE2)
    strips = [r for r in ROWS.values()
              if r.edge == "more than one column strip, the last one ragged"]
    assert {_launch(r)[0].rg for r in strips} == {1, 2}
    # a plan with split == 1 in every family (but wino: wgrad_wino_ok asks for >= 32 chunks,
    # which make_plan_wino splits at least four ways)
    assert {n.split(":")[0] for n, r in ROWS.items()
            if all(l.split == 1 for l in _launch(r))} == set(FAMILIES) - {"wino"}
    assert min(_launch(r)[0].split for n, r in ROWS.items() if n.startswith("wino:")) == 4
    # db on both paths of bias_grad_kernel
    assert {len(bias_launches(r)) for r in ROWS.values() if r.db} == {1, 2}
    # the chunked rows with activation on load: fp32, split bf16 and bf16 tensors
    assert {r.mode for r in ROWS.values() if r.chunk} == {"fp32", "x3", "b16"}
    # the centre-tap forms, through both entries
    assert {r.entry for r in ROWS.values() if r.ks == 1} == {"1x1", "in"}
    # the entries that land on an fp32 kernel (the eq32 rule)
    assert {(r.mode, r.stride) for r in ROWS.values() if r.edge.startswith("eq32")} == \
        {("x3", 1), ("x3", 2), ("bf16", 1), ("bf16", 2)}


def test_largest_row_and_its_reduction():
    """Nothing is larger than 3 x 40 x 136 pixels but the 2 x 128 x 128 row, whose 128 slabs are
    the longest reduction here: two stages.  Three stages take more than 256 slabs, which no
    request of this size has (tests/test_wgrad_defer_gpu.py holds them at 2 x 256 x 256)."""
    big = [n for n, r in ROWS.items() if r.N * r.H * r.W > 3 * 40 * 136]
    assert len(big) == 1
    row = ROWS[big[0]]
    assert (row.N, row.H, row.W, row.Cx, row.Cout) == (2, 128, 128, 32, 32)
    assert sum(l.split for l in _launch(row)) == 128 and M.reduction_stages(request(row)) == 2
    assert max(M.reduction_stages(request(r)) for r in ROWS.values()) == 2
