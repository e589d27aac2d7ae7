"""Writes tests/data/conv_host_cpu.json: what the host side of the convolution forward / data-
gradient entry points (csrc/conv_igemm.hip, from the builders to the end of the file) answers
without a GPU.  tests/test_conv_host_cpu.py holds the library under test to it row by row.

Regenerate it only from a library whose behaviour is the one to keep, e.g. a build of the parent
commit beside the product one (as tests/tools/make_wgrad_workspace_table.py describes):

    make -C unet-implementations_amd/csrc BUILD=build_parent OUT=../libunet_parent.so
    UNET_HIP_LIB=<that library> python tests/tools/make_conv_host_table.py

Tables, over the shape grid of the weight-gradient table (SIZES x CX x COUT x BATCHES), each shape
with the default chunk limit and with `unet_debug_set_chunk_limit` lowered to `limit`.  The file
holds the answers of one group of shapes side by side (`load_table` gives one row per call):
  up:        [H, W, C0, C1, limit, f32, b16, wino] - one digit per (Cout, chunk limit, N) in grid
             order.  f32 / wino: bit k set when unet_conv_up_in_fwd_supported /
             unet_conv_up_c32_is_winograd answer 1 with the thread's c32 switch
             (unet_set_c32_winograd) at k = 0, 1, 2; b16: the answer of
             unet_conv_up_in_fwd_b16_supported
  workspace: [H, W, Cout, stride, limit, [bytes per (chunk limit, N)]] of
             unet_conv_in_fwd_workspace_bytes
  rejected:  [case, rc, text, [exports]] - one call per export and validation check that is
             reachable before the first launch, made to fail exactly that check; exports that
             answer alike share a line.  The device pointers are dummy non-null integers: no row
             may pass validation, and a row whose return code is UNET_OK or UNET_E_LAUNCH is
             refused."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TABLE = os.path.join(ROOT, "tests", "data", "conv_host_cpu.json")

BATCHES = (1, 2, 8, 32)
SIZES = ((4, 4), (8, 16), (16, 24), (24, 40), (64, 64), (256, 192), (512, 512))
CX = (3, 32, 64, 96, 256, 512)
COUT = (32, 64, 96, 128, 512)
STRIDES = (1, 2)
C1S = (0, 32, 64)

UNET_OK, UNET_E_LAUNCH = 0, -2
P = 0x10000          # a dummy non-null device pointer: never dereferenced by a rejected call
BIG = 8192           # 9 * BIG * BIG * 4 bytes of weights exceed 2 GiB


class chunk_limit:
    """`with chunk_limit(lib, nbytes):` - the debug chunk limit lowered (0: left at its default)
    for the block and restored afterwards."""

    def __init__(self, lib, nbytes):
        self.lib, self.nbytes = lib, nbytes

    def __enter__(self):
        if self.nbytes:
            self.lib.unet_debug_set_chunk_limit(self.nbytes)

    def __exit__(self, *exc):
        self.lib.unet_debug_set_chunk_limit(0)
        return False


def _mask(lib, query, args):
    m = 0
    for k in (0, 1, 2):
        prev = lib.unet_set_c32_winograd(k)
        m |= query(*args) << k
        lib.unet_set_c32_winograd(prev)
    return m


def up_rows(lib):
    """Yields ([N, H, W, C0, C1, Cout, limit], f32, b16, wino) in table order."""
    for H, W in SIZES:
        for C0 in CX:
            for C1 in C1S:
                for Cout in COUT:
                    for limit in (0, 3 * H * W * max(C0, C1) * 4):
                        with chunk_limit(lib, limit):
                            for N in BATCHES:
                                a = (N, H, W, C0, C1, Cout)
                                yield (list(a) + [limit],
                                       _mask(lib, lib.unet_conv_up_in_fwd_supported, a),
                                       lib.unet_conv_up_in_fwd_b16_supported(*a),
                                       _mask(lib, lib.unet_conv_up_c32_is_winograd, a))


def workspace_rows(lib):
    """Yields ([N, H, W, Cout, stride, limit], bytes) in table order."""
    for H, W in SIZES:
        for Cout in COUT:
            for stride in STRIDES:
                for limit in (0, 3 * H * W * Cout * 4):
                    with chunk_limit(lib, limit):
                        for N in BATCHES:
                            yield ([N, H, W, Cout, stride, limit],
                                   lib.unet_conv_in_fwd_workspace_bytes(N, H, W, Cout, stride))


# ---- rejected calls ------------------------------------------------------------------------------
# An export is (argument names in ABI order); a case overrides some arguments of the family's
# valid base call.  Special names: "s0"/"s1"/"low"/"skip" are (x, C, alpha, beta) tuples or None,
# "bs" is None, "ws_short" takes bytes off the queried workspace size, "limit" lowers the chunk
# limit for the call.
FWD = "x0 C0 x1 C1 wf bias y N H W Cout stride".split()
FWD3 = "x0 C0 x1 C1 wf w3 bias y N H W Cout stride".split()
BWD = "dy wd Cin_total ci_offset dx N H W Cout Ccols stride accumulate".split()
BWD3 = "dy wd w3 Cin_total ci_offset dx N H W Cout Ccols stride accumulate".split()
UPB = "dy wd Cin_total ci_offset dx N H W Cout Ccols accumulate".split()
UPB3 = "dy wd w3 Cin_total ci_offset dx N H W Cout Ccols accumulate".split()
INF = "s0 s1 slope w bias ksize stride y ws ws_bytes px N H W Cout".split()
INF3 = "s0 s1 slope w w3 bias ksize stride y ws ws_bytes px N H W Cout".split()
FIN = "y ws ws_bytes stats_px gamma beta eps mask mean rstd alpha_out beta_out N HoWo Cout".split()
UPF = "low skip slope wf bias y ws ws_bytes px N H W Cout".split()
UPF3 = "low skip slope wf w3 bias y ws ws_bytes px N H W Cout".split()
U8 = "image mean3 std3 wf bias y ws ws_bytes px N H W Cout".split()

EXPORTS = {
    "unet_conv3x3_fwd": FWD, "unet_conv3x3_fwd_bf16": FWD, "unet_conv3x3_fwd_bf16x3": FWD3,
    "unet_conv3x3_bwd_data": BWD, "unet_conv3x3_bwd_data_bf16": BWD,
    "unet_conv3x3_bwd_data_b16": BWD, "unet_conv3x3_bwd_data_bf16x3": BWD3,
    "unet_conv3x3_bwd_data_bs": BWD + ["bs"], "unet_conv3x3_bwd_data_bs_b16": BWD + ["bs"],
    "unet_conv3x3_bwd_data_bs_b16_wb": BWD3 + ["bs"],
    "unet_conv3x3_bwd_data_bs_bf16x3": BWD3 + ["bs"],
    "unet_conv1x1_fwd": FWD[:-1], "unet_conv1x1_bwd_data": BWD[:10] + ["accumulate"],
    "unet_conv_in_fwd": INF, "unet_conv_in_fwd_b16": INF, "unet_conv_in_fwd_bf16x3": INF3,
    "unet_conv_in_fwd_b16_wb": INF3,
    "unet_conv_in_stats_finalize": FIN, "unet_conv_in_stats_finalize_b16": FIN,
    "unet_conv3x3_up_bwd_data": UPB, "unet_conv3x3_up_bwd_data_b16": UPB,
    "unet_conv3x3_up_bwd_data_bs": UPB + ["bs"], "unet_conv3x3_up_bwd_data_bs_b16": UPB + ["bs"],
    "unet_conv3x3_up_bwd_data_bs_b16_wb": UPB3 + ["bs"],
    "unet_conv_up_in_fwd": UPF, "unet_conv_up_in_fwd_b16": UPF3,
    "unet_stem_u8_fwd": U8, "unet_stem_u8_fwd_b16": U8,
}

BASE = dict(x0=P, C0=32, x1=None, C1=0, wf=P, w=P, w3=P, bias=P, y=P, N=1, H=8, W=8, Cout=32,
            stride=1, dy=P, wd=P, Cin_total=32, ci_offset=0, dx=P, Ccols=32, accumulate=0,
            bs=None, s0=(P, 32, None, None), s1=None, slope=0.01, ksize=3, ws=P, px=True,
            stats_px=0, gamma=P, beta=P, eps=1e-5, mask=None, mean=P, rstd=P, alpha_out=P,
            beta_out=P, HoWo=64, image=P, mean3=True, std3=True)
# the fused up-sampling forward needs a shape that has a tile (fp32: 512 tiles, bf16: 256)
UP_BASE = dict(low=(P, 32, P, P), skip=None, N=1, H=128, W=128, Cout=256)

ES = {"unet_conv3x3_bwd_data_b16": 2, "unet_conv3x3_bwd_data_bs_b16": 2,
      "unet_conv3x3_bwd_data_bs_b16_wb": 2, "unet_conv_in_fwd_b16": 2,
      "unet_conv_in_fwd_b16_wb": 2, "unet_conv3x3_up_bwd_data_b16": 2,
      "unet_conv3x3_up_bwd_data_bs_b16": 2, "unet_conv3x3_up_bwd_data_bs_b16_wb": 2}

FWD_CASES = [
    ("null x0", dict(x0=None)), ("null y", dict(y=None)), ("stride 3", dict(stride=3)),
    ("N 0", dict(N=0)), ("Cout 48", dict(Cout=48)), ("stem two sources", dict(C0=3, C1=32, x1=P)),
    ("stem stride 2", dict(C0=3, stride=2)), ("C0 48", dict(C0=48)),
    ("C1 48", dict(C1=48, x1=P)), ("null x1", dict(C1=32)),
    ("weights over 2 GiB", dict(C0=BIG, Cout=BIG)),
    ("one image over the limit", dict(limit=8 * 8 * 32 * 4 - 1)),
]
BWD_CASES = [
    ("null dy", dict(dy=None)), ("null dx", dict(dx=None)), ("stride 3", dict(stride=3)),
    ("Cout 48", dict(Cout=48)), ("Ccols 48", dict(Ccols=48, Cin_total=96)),
    ("slice past the end", dict(ci_offset=32)), ("negative slice", dict(ci_offset=-32)),
    ("odd H at stride 2", dict(H=7, stride=2)), ("odd W at stride 2", dict(W=7, stride=2)),
    ("weights over 2 GiB", dict(Cout=BIG, Cin_total=BIG)),
    ("one image over the limit", dict(limit="es*8*8*32-1")),
]
X1_CASES = [
    ("null x0", dict(x0=None)), ("N 0", dict(N=0)), ("Cout 48", dict(Cout=48)),
    ("C0 48", dict(C0=48)), ("null x1", dict(C1=32)),
    ("one image over the limit", dict(limit=8 * 8 * 32 * 4 - 1)),
]
B1_CASES = [
    ("null dx", dict(dx=None)), ("Cout 48", dict(Cout=48)), ("slice past the end", dict(ci_offset=32)),
    ("one image over the limit", dict(limit=8 * 8 * 32 * 4 - 1)),
]
INF_CASES = [
    ("null s0", dict(s0=None)), ("null s0.x", dict(s0=(None, 32, None, None))),
    ("null y", dict(y=None)), ("null workspace", dict(ws=None)), ("null stats_px_out", dict(px=False)),
    ("ksize 2", dict(ksize=2)), ("stride 3", dict(stride=3)),
    ("stride 2 at ksize 1", dict(stride=2, ksize=1)), ("N 0", dict(N=0)), ("Cout 48", dict(Cout=48)),
    ("workspace one byte short", dict(ws_short=1)),
    ("workspace one byte short, stride 2", dict(ws_short=1, stride=2)),
    ("stem two sources", dict(s0=(P, 3, None, None), s1=(P, 32, None, None))),
    ("stem activated", dict(s0=(P, 3, P, P))), ("stem ksize 1", dict(s0=(P, 3, None, None), ksize=1)),
    ("C0 48", dict(s0=(P, 48, None, None))), ("C1 48", dict(s1=(P, 48, None, None))),
    ("null s1.x", dict(s1=(None, 32, None, None))),
    ("alpha without beta", dict(s0=(P, 32, P, None))),
    ("alpha without beta, second source", dict(s1=(P, 32, P, None))),
    ("weights over 2 GiB", dict(s0=(P, BIG, None, None), Cout=BIG)),
    ("one image over the limit", dict(limit="es*8*8*32-1")),
    ("one image over the limit, ksize 1", dict(ksize=1, limit="es*8*8*32-1")),
]
FIN_CASES = [
    ("null y", dict(y=None)), ("null mean", dict(mean=None)), ("negative stats_px", dict(stats_px=-1)),
    ("tiles do not cover", dict(stats_px=48)),
]
UPB_CASES = [
    ("null dy", dict(dy=None)), ("null dx", dict(dx=None)), ("Cout 48", dict(Cout=48)),
    ("slice past the end", dict(ci_offset=32)), ("N 0", dict(N=0)),
    ("weights over 2 GiB", dict(Cout=BIG, Cin_total=BIG)),
    ("one image over the limit", dict(limit="es*8*8*9*32-1")),
]
UPF_CASES = [
    ("null low", dict(low=None)), ("null y", dict(y=None)), ("null stats_px_out", dict(px=False)),
    ("null skip.x", dict(skip=(None, 32, P, P))),
    ("unsupported shape", dict(H=8, W=32)), ("odd H", dict(H=127)), ("Cout 48", dict(Cout=48)),
    ("workspace one byte short", dict(ws_short=1)),
]
U8_CASES = [
    ("null image", dict(image=None)), ("null mean3", dict(mean3=False)), ("null y", dict(y=None)),
    ("W 100", dict(W=100)), ("Cout 48", dict(W=128, Cout=48)), ("N 0", dict(W=128, N=0)),
    ("workspace one byte short", dict(W=128, ws_short=1)),
]

CASES = {}
for _n in ("unet_conv3x3_fwd", "unet_conv3x3_fwd_bf16", "unet_conv3x3_fwd_bf16x3"):
    CASES[_n] = list(FWD_CASES)
CASES["unet_conv3x3_fwd_bf16x3"] += [("null w3", dict(w3=None))]
for _n in EXPORTS:
    if _n.startswith("unet_conv3x3_bwd_data"):
        CASES[_n] = list(BWD_CASES)
    if _n.startswith("unet_conv3x3_up_bwd_data"):
        CASES[_n] = list(UPB_CASES)
    if _n.startswith("unet_conv_in_fwd"):
        CASES[_n] = list(INF_CASES)
    if _n.startswith("unet_conv_in_stats_finalize"):
        CASES[_n] = list(FIN_CASES)
    if _n.startswith("unet_stem_u8"):
        CASES[_n] = list(U8_CASES)
CASES["unet_conv3x3_bwd_data_bf16x3"] += [("null w3", dict(w3=None))]
CASES["unet_conv3x3_bwd_data_bs_bf16x3"] += [("null w3", dict(w3=None))]
CASES["unet_conv_in_fwd_bf16x3"] += [("null w3", dict(w3=None))]
CASES["unet_conv1x1_fwd"] = X1_CASES
CASES["unet_conv1x1_bwd_data"] = B1_CASES
CASES["unet_conv_up_in_fwd"] = UPF_CASES + [("alpha without beta", dict(low=(P, 32, P, None)))]
CASES["unet_conv_up_in_fwd_b16"] = UPF_CASES + [
    ("null w3", dict(w3=None)), ("plain low source", dict(low=(P, 32, None, None))),
    ("plain skip source", dict(skip=(P, 32, None, None)))]
del _n


def _call(lib, name, over):
    """Makes the call `name` with the family's base arguments overridden by `over`; returns
    (rc, text of unet_last_error)."""
    from unet_implementations_amd._lib import ActSrc
    v = dict(BASE)
    if name.startswith("unet_conv_up_in_fwd"):
        v.update(UP_BASE)
    v.update(over)
    es = ES.get(name, 4)
    limit = v.pop("limit", 0)
    if isinstance(limit, str):
        limit = eval(limit, {"es": es})
    stride = v["stride"] if "stride" in EXPORTS[name] else 1
    v["ws_bytes"] = max(0, lib.unet_conv_in_fwd_workspace_bytes(
        v["N"], v["H"], v["W"], v["Cout"], stride) - v.pop("ws_short", 0))
    keep = []   # (ctypes objects must outlive the call)
    args = []
    for k in EXPORTS[name]:
        a = v[k]
        if k in ("s0", "s1", "low", "skip"):
            if a is not None:
                keep.append(ActSrc(*a))
                a = ctypes.byref(keep[-1])
        elif k == "px":
            keep.append(ctypes.c_int(-7))
            a = ctypes.byref(keep[-1]) if a else None
        elif k in ("mean3", "std3"):
            keep.append((ctypes.c_float * 3)(0.5, 0.5, 0.5))
            a = keep[-1] if a else None
        args.append(a)
    with chunk_limit(lib, limit):
        rc = getattr(lib, name)(*args, None)
    msg = lib.unet_last_error()
    return rc, (msg.decode() if msg else "")


def rejected_rows(lib):
    """Yields ([export, case], rc, text) in table order."""
    for name in EXPORTS:
        for case, over in CASES[name]:
            rc, text = _call(lib, name, over)
            yield [name, case], rc, text


UP_GROUP = len(COUT) * 2 * len(BATCHES)      # calls that share (H, W, C0, C1)
WS_GROUP = 2 * len(BATCHES)                  # calls that share (H, W, Cout, stride)


def pack(up, ws, rej):
    """The table as stored, from one row per call: up [N, H, W, C0, C1, Cout, limit, f32, b16,
    wino], ws [N, H, W, Cout, stride, limit, bytes], rej [export, case, rc, text]."""
    tab = {"up": [], "workspace": [], "rejected": []}
    for i in range(0, len(up), UP_GROUP):
        g = up[i:i + UP_GROUP]
        tab["up"].append(g[-1][1:5] + [g[-1][6]] +
                         ["".join(str(r[c]) for r in g) for c in (7, 8, 9)])
    for i in range(0, len(ws), WS_GROUP):
        g = ws[i:i + WS_GROUP]
        tab["workspace"].append(g[-1][1:6] + [[r[6] for r in g]])
    alike = {}
    for name, case, rc, text in rej:
        alike.setdefault((case, rc, text), []).append(name)
    tab["rejected"] = [list(k) + [names] for k, names in alike.items()]
    return tab


def load_table():
    """The committed table, one row per call (the layouts `pack` takes)."""
    with open(TABLE) as f:
        tab = json.load(f)
    up, ws = [], []
    for H, W, C0, C1, lowered, *answers in tab["up"]:
        assert all(len(a) == UP_GROUP for a in answers), (H, W, C0, C1)
        keys = [[N, H, W, C0, C1, Cout, limit]
                for Cout in COUT for limit in (0, lowered) for N in BATCHES]
        up += [key + [int(d) for d in digits] for key, *digits in zip(keys, *answers)]
    for H, W, Cout, stride, lowered, sizes in tab["workspace"]:
        assert len(sizes) == WS_GROUP, (H, W, Cout, stride)
        keys = [[N, H, W, Cout, stride, limit] for limit in (0, lowered) for N in BATCHES]
        ws += [key + [n] for key, n in zip(keys, sizes)]
    rej = [[name, case, rc, text] for case, rc, text, names in tab["rejected"] for name in names]
    return {"up": up, "workspace": ws, "rejected": rej}


def main():
    import unet_implementations_amd as ua
    lib = ua.lib()
    up = [key + [f, b, w] for key, f, b, w in up_rows(lib)]
    ws = [key + [n] for key, n in workspace_rows(lib)]
    rej = []
    for key, rc, text in rejected_rows(lib):
        if rc in (UNET_OK, UNET_E_LAUNCH):
            raise SystemExit(f"{key}: passed validation (rc {rc}, {text!r}): not a rejected call")
        rej.append(key + [rc, text])
    tab = pack(up, ws, rej)
    os.makedirs(os.path.dirname(TABLE), exist_ok=True)
    with open(TABLE, "w") as f:
        for i, (title, rows) in enumerate(tab.items()):
            f.write(('{' if i == 0 else ' ') + f'"{title}": [\n')
            f.write(",\n".join("  " + json.dumps(r) for r in rows))
            f.write("\n ]" + ("," if i < 2 else "\n}") + "\n")
    print(f"{TABLE}: {len(up)} up rows, {len(ws)} workspace rows, {len(rej)} rejected calls")


if __name__ == "__main__":
    main()
