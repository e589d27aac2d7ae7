"""CPU (-m "not gpu"): the float64 references of tests/test_wgrad_fp64_gpu.py
(tests/tools/wgrad_refs.py), checked on their own for every row of its table:
  * each reference equals, to 1e-12, a nine-tap einsum written without
    torch.nn.grad.conv2d_weight;
  * AMBIGUITY: where the row's kernel rounds the activated operand to bf16, the two legitimate
    readings of that rounding - the activation in float64 and then the rounding (a fused
    multiply-add), or in unfused fp32 and then the rounding - give references that differ by at
    most a tenth of the row's bound.  This is a condition on the drawn inputs (an operand
    element next to a bf16 tie): a row that misses it gets another seed;
  * THE CHECK OF THE CHECK: the reference without the dy pixel (N - 1, Ho - 1, Wo - 1) differs
    from the full one by more than ten times the row's bound, so a kernel that dropped that
    pixel could not pass;
  * the rounding each family is said to apply matches the kernel names of its rows."""
import functools
import importlib.util
import os

TESTS = os.path.dirname(os.path.abspath(__file__))


def _load(name, *where):
    spec = importlib.util.spec_from_file_location(name, os.path.join(TESTS, *where, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _load("test_wgrad_fp64_gpu")
WR = T.WR
ROWS = T.ROWS


@functools.lru_cache(maxsize=None)
def _ops(name):
    return WR.Operands(ROWS[name])


@functools.lru_cache(maxsize=None)
def _ref(name):
    """(activated operand, dy, reference) of a row: computed once, shared, left unchanged"""
    ops = _ops(name)
    a, dy = ops.a64(), ops.dy64()
    return a, dy, WR.reference(ROWS[name], a, dy)


def test_references_equal_a_nine_tap_einsum():
    bad = []
    for name, row in ROWS.items():
        a, dy, ref = _ref(name)
        e = WR.rel(WR.einsum_reference(row, a, dy), ref)
        if not e <= 1e-12:
            bad.append(f"{name}: {e:.2e}")
    assert not bad, "\n".join(bad)


def test_rounding_follows_the_kernel_family():
    rounding = {n.split(":")[0] for n, r in ROWS.items() if WR.rounds_activation(r)}
    assert rounding == {"b16-ring", "b16-segments", "taps-b16"}
    for name, row in ROWS.items():
        if row.mode == "b16" and row.act:
            assert WR.rounds_activation(row) == \
                (name.split(":")[0] in ("b16-ring", "b16-segments", "taps-b16")), name


def test_bf16_rounding_leaves_the_reference_unambiguous():
    bad, worst, n = [], 0.0, 0
    for name, row in ROWS.items():
        if not WR.rounds_activation(row):
            continue
        a, dy, ref = _ref(name)
        amb = WR.rel(WR.reference(row, _ops(name).a64(act="fp32"), dy), ref)
        worst, n = max(worst, amb), n + 1
        if not amb <= T.tol(row) / 10:
            bad.append(f"{name}: ambiguity {amb:.2e} > {T.tol(row) / 10:.1e}: re-seed the row")
    assert n >= 20
    assert not bad, "\n".join(bad)
    print(f"largest ambiguity over {n} rows: {worst:.2e}")


def test_one_dropped_pixel_is_seen_by_every_row():
    bad = []
    for name, row in ROWS.items():
        a, dy, ref = _ref(name)
        d = WR.rel(WR.reference(row, a, _ops(name).dy64(drop_pixel=True)), ref)
        if not d > 10 * T.tol(row):
            bad.append(f"{name}: one dy pixel moves the reference by {d:.2e} only")
    assert not bad, "\n".join(bad)


def test_rows_draw_what_their_mode_stores():
    """bf16 tensors and the bf16 entry draw bf16 numbers (so the loaders' rounding of x and dy is
    exact); the RGB image stays fp32; fp32 and split rows draw fp32 numbers."""
    for name, row in ROWS.items():
        ops = _ops(name)
        exact = bool((WR.r16(ops.dy) == ops.dy).all())
        assert exact == (row.mode in ("b16", "bf16")), name
        if row.entry != "u8" and row.Cx != 3:
            assert bool((WR.r16(ops.x) == ops.x).all()) == (row.mode in ("b16", "bf16")), name
