"""CPU (-m "not gpu"): the tile choosers of csrc/conv_tiles.h (the gather-GEMM ladder and the
patch ladders, plain host code) held to what the library launched on the GPU before the ladders
were stated once: tests/data/conv_host_gpu.json records, per call, the kernel instantiation.

Every unchunked single-launch row of that table whose kernel is a patch or gather-GEMM kernel
picked by those ladders becomes a query of tests/tools/conv_tiles_check.cpp - a program of its
own, built with AddressSanitizer + UBSan on the host side, that builds the call's IgemmParams
with the csrc/conv_host.h builders and prints the chooser's pick.  The pick must be the template
arguments of the recorded kernel name, and the patch ladder a gather-GEMM row went past must have
answered "none" (or not apply).  Left out: the rungs that stay explicit conditions of the
dispatchers (the "channel taps" rows of the `upb` family: DENSE, the fp32 64 x 64 rung; WIDE)."""
import importlib.util
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load("make_conv_host_gpu_table")
T = G.T


def _ints(args):
    return [int(x) for x in re.findall(r"-?\d+", args)]


def _expect(kernel):
    """(chooser, pick, patch ladders the call went past) of a recorded kernel name, or None."""
    m = re.search(r"(conv_\w+_kernel)<([^>]*)>", kernel)
    if m:
        name, args = m.group(1), m.group(2)
        n, flags = _ints(args), re.findall(r"true|false", args)
    else:                      # bf16-tensor instantiations are recorded mangled
        m = re.search(r"\d+(conv_igemm_bf16_kernel)I((?:Li\d+E)+)DF16bDF16bLb([01])ELi(\d+)ELi(\d+)E", kernel)
        if not m:
            return None
        if int(m.group(5)) != 0:   # WIDE / DENSE: explicit rungs of dispatch_igemm_b16
            return None
        tile = " ".join(re.findall(r"Li(\d+)E", m.group(2)))
        went_past = ["b16", "b16_s2"] if m.group(3) == "1" else ["b16"]
        return "gemm_kg", f"{tile} {m.group(4)}", went_past
    tile = " ".join(str(x) for x in n[:4])
    if name == "conv_patch_f32_kernel":
        return "f32", tile, []
    if name == "conv_patch_up_kernel":
        return "up", tile, []
    if name == "conv_patch_s2_kernel":
        return "s2", tile, ["f32"]
    if name in ("conv_dgrad_s2_patch_kernel", "conv_dgrad_s2_patch_b16_kernel"):
        return "dgrad_s2", tile, []
    if name == "conv_patch_b16_kernel":     # <.., ACT, STATS, BSTATS, WB, UP, SD>
        return ("b16_up" if flags[4] == "true" else "b16_s2" if n[4] == 2 else "b16"), tile, []
    if name == "conv_patch_split_kernel":
        return ("split" if flags == ["false"] * 3 else "split_fused"), tile, []
    if name == "conv_igemm_kernel":         # <BM, BN, WM, WN, BK, FUSED, KG>
        return "gemm_kg", f"{tile} {n[5]}", ["f32", "s2"] if flags[0] == "true" else ["f32"]
    if name == "conv_igemm_bf16_kernel":    # bf16 cores on fp32 tensors: no patch form, KG = 1
        return "gemm", f"{tile} 1", []
    if name == "conv_igemm_split_kernel":
        return "gemm", f"{tile} 1", ["split"]
    return None


def _queries():
    """[(query line, expected answer)] over the rows of the GPU table."""
    out = []
    for row, rec in zip(G.ROWS, G.load_table()):
        if row.get("lim") or len(rec["launches"]) != 1 or row["fam"] == "upb":
            continue
        want = _expect(rec["launches"][0])
        if want is None:
            continue
        chooser, pick, went_past = want
        fn, keys = row["fn"], T.EXPORTS[row["fn"]]
        es = 2 if fn in G.B16 else 4
        if es == 2:
            w3 = int(fn in G.ONE_PLANE and row.get("w3", 1))
        else:
            w3 = int("bf16x3" in fn)
        if "dy" in keys:
            kind = "dgrad"
            a, b, c = row["Cout"], row["Ccols"], row.get("Cin_total", row["Ccols"])
            act = ""
            ksize = 3 if "stride" in keys else 1
        else:
            kind = "up" if "low" in keys else "fwd"
            a, b, c = row["C0"], row.get("C1", 0), row["Cout"]
            act = row.get("act", "01") if ("s0" in keys or "low" in keys) else ""
            ksize = row.get("ksize", 3) if "s0" in keys else (3 if ("stride" in keys or "low" in keys) else 1)
        shape = (f"{kind} {row['N']} {row['H']} {row['W']} {a} {b} {c} {row.get('stride', 1)} "
                 f"{ksize} {es} {w3} {int('0' in act)} {int('1' in act and b > 0)}")
        out.append((f"{row['id']} {chooser} {shape}", f"{row['id']} {chooser} {pick}"))
        for ladder in went_past:
            out.append((f"{row['id']} {ladder} {shape}", (row["id"], ladder)))
    return out


def test_choosers_pick_the_recorded_instantiations_under_host_sanitizers(tmp_path):
    queries = _queries()
    # every family of the tables and both ladders are asked, each rung of the patch tables once
    asked = {q.split()[1] for q, _ in queries}
    assert asked == {"f32", "up", "s2", "dgrad_s2", "b16", "b16_up", "b16_s2", "split_fused",
                     "split", "gemm_kg", "gemm"}
    picks = {w.split(" ", 1)[1] for _, w in queries if isinstance(w, str)}
    for fam, rungs in (("f32", 3), ("up", 3), ("s2", 2), ("dgrad_s2", 2), ("b16", 4), ("b16_up", 3),
                       ("b16_s2", 1), ("split_fused", 4), ("split", 5)):
        assert len({p for p in picks if p.startswith(fam + " ")}) == rungs, fam
    assert len({p for p in picks if p.startswith("gemm_kg ")}) == 6      # 4 tiles, KG 1 / 2 / 4
    assert len({p for p in picks if p.startswith("gemm ")}) == 4

    exe = str(tmp_path / "conv_tiles_check")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-g", "--offload-arch=gfx950",
                    "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "unet-implementations_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "tools", "conv_tiles_check.cpp"), "-o", exe],
                   check=True)
    run = subprocess.run([exe], input="".join(q + "\n" for q, _ in queries), capture_output=True,
                         text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert lines[-1] == f"conv_tiles_check: {len(queries)} answers", run.stdout[-2000:]
    bad = []
    for (query, want), got in zip(queries, lines):
        if isinstance(want, str):
            if got != want:
                bad.append((query, got, want))
        else:                                   # a patch ladder the call went past
            rid, ladder = want
            if got not in (f"{rid} {ladder} none", f"{rid} {ladder} n/a"):
                bad.append((query, got, "none or n/a"))
    assert not bad, f"{len(bad)} picks differ, first (query, pick, recorded): {bad[0]}"
