"""GPU: every recorded convolution forward / data-gradient launch held against float64.

tests/data/conv_host_gpu.json lists 378 calls of the forward / data-gradient entry points of
csrc/conv_igemm.hip with the kernels each launches - 118 instantiations: every rung of every
ladder of csrc/conv_tiles.h, every chunk site, both stem forms, the c32 switch at 0 / 1 / 2.
tests/test_conv_host_gpu.py holds the library to the recorded launch list, report and output
bits: "nothing changed".  This file adds "it is right": one case per row
  1. builds the row's operands with weight planes derived from its fp32 weight
     (G.build_row(coherent=True)) and makes the call (G.call_row);
  2. asserts the launches and the reported stats_px / tiles_out are the recorded ones, so that the
     verdict belongs to the recorded instantiation;
  3. compares every output with the float64 reference of tests/tools/conv_host_refs.py, evaluated
     on the same operands rounded as the row's operand mode rounds them, one image at a time.
The per-tile side outputs are compared merged per image: the fused forward's (mean, M2) pairs as
mean and rstd = 1 / sqrt(var + eps) of the image, the BSTATS pairs as S1 / S2 of the image.  A row
that reports 0 or -1 (a short partial buffer, no unet_bwd_stats, a chunked call, a shape without
the epilogue) is held on y / dx alone - and to the recorded report.

Bounds, each relative to max |reference| of its tensor:
  fp32 tensors (plain, _bf16, _bf16x3 entries): the TOL_* of tests/tools/step_kernel_harness.py -
    TOL_Y for y and the merged mean, TOL_STAT for rstd / alpha / beta, TOL_DX for dx, TOL_UP for
    the g of the up-sampled operand's data gradient, TOL_BS for the merged S1 / S2;
  bf16 tensors: those of tests/test_bf16_bench_layers_gpu.py - one bf16 ulp of the tensor's max
    for stored results, 2e-3 for the merged mean / rstd (and the finalize's four results), 3e-3
    for the merged S1 / S2.
test_check_sees_one_missing_row is the check of the check: for one row per family and storage
type, one chunked row and one row of four per-class stride-2 launches, the same bounds must fail
against a reference evaluated with one row of one image zeroed.  test_bstats_definition pins the
reading of S1 / S2 against fp64 autograd.  tests/test_conv_host_refs_cpu.py checks the references
themselves and the closure (all 118 names are launched by a row parametrized here)."""
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load("make_conv_host_gpu_table")
C = _load("conv_host_refs")
HS = _load("step_kernel_harness")
R = HS.R

ULP = 2.0 ** -8          # one bf16 ulp of a tensor's max magnitude
B16_STAT, B16_BS = 2e-3, 3e-3
CASES = list(G.ROWS)
IDS = [f"{r['fam']}-{r['id']}-{r['fn'][len('unet_'):]}" for r in CASES]
_cache = {}


def recorded(row):
    if not _cache:
        _cache.update({r["id"]: r for r in G.load_table()})
    return _cache[row["id"]]


def bounds(row):
    """output class -> bound of the row's operand mode"""
    if row["fn"] in G.B16:
        return dict(y=ULP, dx=ULP, stat_mean=B16_STAT, stat_rstd=B16_STAT, S1=B16_BS, S2=B16_BS,
                    mean=B16_STAT, rstd=B16_STAT, alpha=B16_STAT, beta=B16_STAT)
    return dict(y=HS.TOL_Y, dx=HS.TOL_UP if row["fam"] == "upb" else HS.TOL_DX,
                stat_mean=HS.TOL_Y, stat_rstd=HS.TOL_STAT, S1=HS.TOL_BS, S2=HS.TOL_BS,
                mean=HS.TOL_Y, rstd=HS.TOL_STAT, alpha=HS.TOL_STAT, beta=HS.TOL_STAT)


def reference(row, built, drop=None):
    return C.REFS[row["fam"]](row, built["t"], C.mode_of(row["fn"], G.B16), drop)


def compare(row, report, outs, ref, only=None):
    """the metrics of every output of the call (`only`: of these) against the reference"""
    tol = bounds(row)
    got = {k: v for k, v in outs.items() if k not in ("stats", "partial")}
    if "stats" in outs:        # (mean, M2) per tile of `report` pixels -> per image
        mean, var = C.merge_tiles(C.tile_pairs(outs["stats"], row["N"], row["Cout"]), report)
        got.update(stat_mean=mean, stat_rstd=1.0 / torch.sqrt(var + C.EPS))
        ref = dict(ref, stat_rstd=1.0 / torch.sqrt(ref["stat_var"] + C.EPS))
    if "partial" in outs:      # (S1, S2) per tile -> per image
        got["S1"], got["S2"] = C.sum_tiles(C.tile_pairs(outs["partial"], row["N"], row["Ccols"]))
    return [R.metric(k, v, ref[k], tol[k]) for k, v in got.items() if only is None or k in only]


def run(ua, row):
    built = G.build_row(ua, row, coherent=True)
    names, report, outs = G.call_row(ua, row, built)
    want = recorded(row)
    assert names == want["launches"], f"launched {names}, recorded {want['launches']}"
    assert report == want["report"], f"reported {report}, recorded {want['report']}"
    assert set(outs) == set(want["crc"]), (sorted(outs), sorted(want["crc"]))
    return built, report, outs


@pytest.mark.parametrize("row", CASES, ids=IDS)
def test_row_against_fp64(ua, row):
    built, report, outs = run(ua, row)
    metrics = compare(row, report, outs, reference(row, built))
    print(R.report(metrics))
    bad = R.failures(metrics)
    assert not bad, f"{row}:\n" + "\n".join(bad)


# --------------------------------------------------------------------------- the check of the check
def _check_rows():
    """One row per (family, storage type) - the first of the table, for the finalize one that
    reads y itself - then the first chunked row and the first row of four per-class stride-2
    launches of each storage type."""
    picked, seen = [], set()

    def take(row, key):
        if key not in seen:
            seen.add(key)
            if row not in picked:
                picked.append(row)

    for row in G.ROWS:
        b16 = row["fn"] in G.B16
        if row["fam"] == "fin" and row["stats_px"]:
            continue
        take(row, (row["fam"], b16))
        if row.get("lim"):
            take(row, ("chunked", b16))
        if row["fam"] == "bs2" and len(recorded(row)["launches"]) == 4:
            take(row, ("per class", b16))
    return picked


_CHECK = _check_rows()
MAIN = {"fin": ("mean", "rstd", "alpha", "beta")}


@pytest.mark.parametrize("row", _CHECK, ids=[IDS[r["id"]] for r in _CHECK])
def test_check_sees_one_missing_row(ua, row):
    """The bounds still resolve the loss of one row of one image: the call passes against the
    reference and every bound of its main output fails against the reference evaluated with
    row 1 of the last image zeroed."""
    built, report, outs = run(ua, row)
    only = MAIN.get(row["fam"], ("y", "dx"))
    good = compare(row, report, outs, reference(row, built), only)
    bad = compare(row, report, outs, reference(row, built, drop=(row["N"] - 1, 1)), only)
    print(R.report(good), "| without the row:", R.report(bad))
    assert good and not R.failures(good), R.failures(good)
    assert len(R.failures(bad)) == len(bad), f"the check cannot see a missing row: {bad}"


def test_check_rows_cover_every_family_and_storage_type():
    keys = {(r["fam"], r["fn"] in G.B16) for r in G.ROWS}
    assert {(r["fam"], r["fn"] in G.B16) for r in _CHECK} == keys
    for b16 in (False, True):
        assert any(r.get("lim") and (r["fn"] in G.B16) == b16 for r in _CHECK)
        assert any(r["fam"] == "bs2" and len(recorded(r)["launches"]) == 4 and
                   (r["fn"] in G.B16) == b16 for r in _CHECK)


# --------------------------------------------------------------------------- S1 / S2
def test_bstats_definition():
    """C.bstats64 is the pair of reductions of the InstanceNorm + LeakyReLU + dropout backward:
    on a layer whose statistics are the true ones of y, sum_n S1 = dbeta and sum_n S2 = dgamma of
    fp64 autograd."""
    n, H, W, Cc = 2, 6, 10, 32
    y, st, gamma, beta, mask = R.norm_layer(n, H, W, Cc, 5)
    g = R.grand((n, H, W, Cc), 9)
    yd = y.double()
    mean = yd.mean(dim=(1, 2))                                 # (unrounded: the definition)
    rstd = 1.0 / torch.sqrt(yd.var(dim=(1, 2), unbiased=False) + R.EPS)
    s1, s2 = C.bstats64(R.nchw64(g), R.nchw64(y), mean, rstd, gamma, beta, mask)
    _, dgamma, dbeta = R.ref_in_bwd(g, y, gamma, beta, mask)
    assert (s1.sum(0) - dbeta).abs().max().item() <= 1e-10 * dbeta.abs().max().item()
    assert (s2.sum(0) - dgamma).abs().max().item() <= 1e-10 * dgamma.abs().max().item()
