"""The weight-gradient plan rule of csrc/conv_wgrad.hip, restated in plain Python: which kernel
instantiation a request launches, chunk by chunk, and with which plan.  No library, no GPU.

Every function below carries the name of the C++ function it restates (wgrad_tile, wgrad_split,
make_plan, make_plan_taps, make_plan_wino, make_plan_wino32, make_plan_stem, wgrad_wino_ok,
wgrad_wino32_ok, wgrad_ring_ok, wgrad_select, wgrad_ws_floats, and the ladders of
launch_wgrad_plan, launch_wgrad_taps_plan, launch_wgrad8_s and launch_wgrad_stem) and keeps its
order of tests, so the two read side by side.  tests/test_wgrad_plan_model_cpu.py holds the
restatement to answers recorded from the library (tests/data/wgrad_workspace_bytes.json) and to
the kernel column of tests/test_wgrad_defer_gpu.py, which has run on the hardware;
tests/test_wgrad_fp64_gpu.py asserts the names it gives against the recorded launches.

A request:
  entry    conv3x3 (ops.conv3x3_bwd_weight), in (ops.conv_in_bwd_weight), 1x1
           (ops.conv1x1_bwd_weight), stem (conv_in_bwd_weight on the fp32 RGB image), u8 (on a
           U8Image), up (ops.conv3x3_up_bwd_weight; H, W = the low-resolution size)
  storage  "fp32" or "bf16": the element type of x and dy (the RGB image is never bf16)
  cores    the matrix cores asked for: 0 fp32, 1 bf16, 3 split bf16 ("bf16x3")
  act      activation on load (alpha / beta given)
  N, H, W, Cx, Cout, stride
  center   centre tap only (conv1x1_bwd_weight, ksize = 1)
  c32      the thread's c32 Winograd switch: 0 never, 1 when it fills the chip, 2 always
  chunk    images per launch forced through unet_debug_set_chunk_limit (0: the default limit)
"""
import collections

Request = collections.namedtuple(
    "Request", "entry storage cores act N H W Cx Cout stride center c32 chunk",
    defaults=(1, False, 0, 0))
# one launch: the kernel's name as tests/test_wgrad_defer_gpu.py::short_name spells a recorded
# launch, and the plan fields the kernel walks by (stem: the stem_* fields in their place)
Launch = collections.namedtuple("Launch",
                                "name N S segs_per_row total_segs segs_per_block split rg")

K_SLAB_CHUNK = 16          # kSlabChunk
K_RING_DEPTH = 2           # kRingDepth
SW_PIX = 128               # pixels per stage of the stem kernels
DEFAULT_LIMIT = (1 << 31) - 1


def ceil_div(a, b):
    return -(-a // b)


def out_size(r):
    return (r.H - 1) // r.stride + 1, (r.W - 1) // r.stride + 1


# --------------------------------------------------------------------------- the record
def is_b16(r):
    return r.storage == "bf16"


def is_taps(r):
    return r.entry == "up"


def call_prec(r):
    """WgradCall::prec as the entry points set it."""
    if r.entry in ("1x1", "up"):
        return 0
    if r.entry in ("stem", "u8"):
        return 1 if is_b16(r) else 0          # (the stem ignores it)
    if is_b16(r):
        return 1                              # unet_conv_in_bwd_weight_b16
    if r.entry == "in" and r.cores == 3:      # unet_conv_in_bwd_weight_bf16x3
        return 3 if not r.center else 0
    return r.cores


def dy_channels(r):
    return 9 * r.Cout if is_taps(r) else r.Cout


def per_image_bytes(r):
    """wgrad_batch_chunk: an image of either tensor, four bytes an element for both storages"""
    Ho, Wo = out_size(r)
    return max(r.H * r.W * r.Cx * 4, Ho * Wo * dy_channels(r) * 4)


def chunk_limit_bytes(r):
    """The debug chunk limit under which the call takes r.chunk images a launch (as
    tests/test_wgrad_defer_gpu.py::Layer.chunk_limit_bytes)."""
    return int((r.chunk + 0.5) * per_image_bytes(r)) if r.chunk else 0


def batch_chunk(r, limit=None):
    """unet_conv::batch_chunk; limit: what unet_debug_set_chunk_limit was given (it keeps the
    default for values outside (0, 2^31))"""
    lim = limit or chunk_limit_bytes(r)
    lim = lim if 0 < lim < (1 << 31) else DEFAULT_LIMIT
    return min(lim // max(per_image_bytes(r), 1), r.N)


# --------------------------------------------------------------------------- plans
Plan = collections.namedtuple("Plan", "nw npp ci_t co_t S split segs_per_row total_segs "
                                      "segs_per_block rg ws_floats")


def slab_ws_floats(slabs, E):
    return slabs * E + 2 * ceil_div(slabs, K_SLAB_CHUNK) * E


def wgrad_tile(Cx, Cout):
    ci_t = 64 if Cx % 64 == 0 else 32
    co_t = 64 if Cout % 64 == 0 else 32
    if ci_t == 64 and co_t == 32:
        ci_t = 32
    return ci_t, co_t, (Cx // ci_t) * (Cout // co_t)


def wgrad_split(target_blocks, tiles, max_split):
    split = min(ceil_div(target_blocks, tiles), max_split)
    return max(split, 1)


def _with_slabs(nw, npp, ci_t, co_t, S, segs_per_row, total_segs, segs_per_block, rg, Cx, Cout):
    split = ceil_div(total_segs, segs_per_block)
    return Plan(nw, npp, ci_t, co_t, S, split, segs_per_row, total_segs, segs_per_block, rg,
                slab_ws_floats(split, 9 * Cx * Cout))


StemPlan = collections.namedtuple("StemPlan", "stem_stages stem_blocks stem_spb ws_floats")


def make_plan_stem(N, H, W, Cout):
    stages = ceil_div(N * H * W, SW_PIX)
    blocks = min(stages, 1024)                # stem_grid
    spb = ceil_div(stages, blocks)
    blocks = ceil_div(stages, spb)
    return StemPlan(stages, blocks, spb, slab_ws_floats(blocks, 27 * Cout))


def make_plan(N, H, W, Cx, Cout, stride, prec, wide, ring8, ring_s2):
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    ci_t, co_t, tiles = wgrad_tile(Cx, Cout)
    nsb = (ci_t // 32) * (co_t // 32)
    nw, rg = 4, 0
    if wide:
        nw, npp = 8, 8 // nsb
        smax = (128 if stride == 1 else 32) if nsb == 1 else \
            64 if nsb == 2 else (64 if stride == 1 else 32)
        S = 16
        while S < smax and S < Wo:
            S *= 2
    else:
        npp = 4 // nsb
        if Wo <= 16:
            S = 16
        elif ci_t == 64:
            S = 16 if (stride == 2 or prec == 3) else 32
        elif co_t == 64:
            S = 32
        else:
            S = 64 if (stride == 1 and Wo >= 64) else 32
    segs_per_row = ceil_div(Wo, S)
    total_segs = N * Ho * segs_per_row
    max_split = ceil_div(total_segs, 4)
    segs_per_block = ceil_div(total_segs, wgrad_split(256 if nw == 8 else 512, tiles, max_split))
    if ((prec == 1 and stride == 1) or (ring_s2 and stride == 2)) and nw == 4:
        def rows_for(target_blocks, g):
            r = ceil_div(total_segs, wgrad_split(target_blocks, tiles, max_split))
            q = K_RING_DEPTH * g
            while r < Ho and (Ho % r or r % q):
                r += 1
            return r if (r <= Ho and Ho % r == 0 and r % q == 0) else 0
        r2 = rows_for(256, 2) if ring8 else 0
        r1 = rows_for(512, 1)
        if r2:
            segs_per_block, rg = r2, 2
        elif r1:
            segs_per_block, rg = r1, 1
    return _with_slabs(nw, npp, ci_t, co_t, S, segs_per_row, total_segs, segs_per_block, rg,
                       Cx, Cout)


def wgrad_wino32_ok(N, H, W, Cx, Cout, stride, c32):
    if not (c32 and stride == 1 and Cx == 32 and Cout == 32 and H % 8 == 0 and W % 32 == 0 and
            N * H * W * 128 < (1 << 31)):
        return False
    return c32 == 2 or N * (H // 8) * (W // 32) >= 256


def make_plan_wino32(N, H, W):
    t = N * (H // 8) * (W // 32)
    split = min(t, 256)
    return Plan(8, 1, 32, 32, 16, split, W // 32, t, 1, 0, slab_ws_floats(split, 9 * 32 * 32))


def wgrad_wino_ok(N, H, W, Cx, Cout, stride):
    if stride != 1 or Cx % 64 or Cout % 64 or H % 2 or W % 16:
        return False
    chunks = N * (H // 2) * (W // 16)
    return 32 <= chunks < (1 << 30)


def make_plan_wino(N, H, W, Cx, Cout):
    total = N * (H // 2) * (W // 16)
    spb = ceil_div(total, wgrad_split(256, (Cx // 64) * (Cout // 64), ceil_div(total, 8)))
    return _with_slabs(8, 2, 64, 64, 16, W // 16, total, spb, 0, Cx, Cout)


def make_plan_taps(Q, Cx, Cout, wide, taps_b16):
    ci_t, co_t, tiles = wgrad_tile(Cx, Cout)
    nsb = (ci_t // 32) * (co_t // 32)
    nw = 8 if wide else 4
    S = (32 if nsb == 1 else 16) * (2 if wide else 1)
    if taps_b16 and nsb == 1:
        S = 64
    total = ceil_div(Q, S)
    spb = ceil_div(total, wgrad_split(256 if wide else 512, tiles, ceil_div(total, 4)))
    return _with_slabs(nw, nw // nsb, ci_t, co_t, S, 0, total, spb, 0, Cx, Cout)


# --------------------------------------------------------------------------- the selector
Sel = collections.namedtuple("Sel", "form prec wide ring8 ring_s2 taps_b16 nmax")


def wgrad_select(r, limit=None, cprec=None):
    """THE rule: form in ("STEM", "WINO", "WINO32", "DIRECT", "TAPS") and the plan options.
    cprec: WgradCall::prec where it is not the entry point's (the workspace queries)"""
    nmax = batch_chunk(r, limit)
    cprec, b16 = call_prec(r) if cprec is None else cprec, is_b16(r)
    fp32 = cprec == 0 and not b16
    wide = fp32 and r.Cx != 3 and wgrad_tile(r.Cx, r.Cout)[2] >= 4
    if is_taps(r):
        return Sel("TAPS", 0, wide, False, False, b16, nmax)
    if r.Cx == 3:
        return Sel("STEM", 0, wide, False, False, False, nmax)
    prec = cprec if r.stride == 1 else 0
    ring_s2 = b16 and cprec == 1 and r.stride == 2
    ring8 = b16 and (prec == 1 or ring_s2) and r.Cx % 64 == 0 and r.Cout % 64 == 0
    wino_able = fp32 and not r.center and nmax >= r.N
    if wino_able and wgrad_wino32_ok(r.N, r.H, r.W, r.Cx, r.Cout, r.stride, r.c32):
        form = "WINO32"
    elif wino_able and wgrad_wino_ok(r.N, r.H, r.W, r.Cx, r.Cout, r.stride):
        form = "WINO"
    else:
        form = "DIRECT"
    return Sel(form, prec, wide, ring8, ring_s2, False, nmax)


def wgrad_plan(r, s, nc, plain=False):
    """the plan of one launch over nc images; plain: with the ring / bf16-tap options off, as
    wgrad_ws_floats sizes the workspace"""
    ring8, ring_s2, taps_b16 = (False, False, False) if plain else (s.ring8, s.ring_s2, s.taps_b16)
    if s.form == "STEM":
        return make_plan_stem(nc, r.H, r.W, r.Cout)
    if s.form == "WINO":
        return make_plan_wino(nc, r.H, r.W, r.Cx, r.Cout)
    if s.form == "WINO32":
        return make_plan_wino32(nc, r.H, r.W)
    if s.form == "TAPS":
        return make_plan_taps(nc * r.H * r.W, r.Cx, r.Cout, s.wide, taps_b16)
    return make_plan(nc, r.H, r.W, r.Cx, r.Cout, r.stride, s.prec, s.wide, ring8, ring_s2)


def chunks_of(r, s):
    return [min(s.nmax, r.N - nb) for nb in range(0, r.N, s.nmax)] if s.nmax >= 1 else []


def wgrad_ws_floats(r, s):
    if s.form == "STEM":
        return wgrad_plan(r, s, r.N, plain=True).ws_floats
    slabs = sum(wgrad_plan(r, s, nc, plain=True).split for nc in chunks_of(r, s))
    return slab_ws_floats(slabs, 9 * r.Cx * r.Cout)


# the seven requests unet_conv3x3_bwd_weight_workspace_bytes sizes for: (storage, cores, centre
# tap, c32)
WS_REQUESTS = (("fp32", 0, False, 0), ("fp32", 0, False, 2), ("fp32", 0, True, 0),
               ("fp32", 3, False, 0), ("fp32", 1, False, 0), ("bf16", 0, False, 0),
               ("bf16", 1, False, 0))


def _select_raw(N, H, W, Cx, Cout, stride, b16, prec, center, c32, limit, taps=False):
    """A record with WgradCall::prec given, not derived from an entry point (the workspace query
    makes requests no entry point makes: bf16 storage with prec 0)."""
    r = Request("up" if taps else "conv3x3", "bf16" if b16 else "fp32", prec, False, N, H, W, Cx,
                Cout, stride, center, c32, 0)
    return r, wgrad_select(r, limit, prec)


def workspace_bytes(N, H, W, Cx, Cout, stride, limit=0):
    """unet_conv3x3_bwd_weight_workspace_bytes"""
    m = 0
    for storage, prec, center, c32 in WS_REQUESTS:
        r, s = _select_raw(N, H, W, Cx, Cout, stride, storage == "bf16", prec, center, c32, limit)
        m = max(m, wgrad_ws_floats(r, s))
    return 4 * m


def is_winograd(N, H, W, Cx, Cout, stride, c32, limit=0):
    """unet_conv3x3_bwd_weight_is_winograd under the switch c32"""
    if Cx <= 3 or stride != 1:
        return 0
    _, s = _select_raw(N, H, W, Cx, Cout, 1, False, 0, False, c32, limit)
    return 1 if s.form in ("WINO", "WINO32") else 0


def up_workspace_bytes(N, h, w, Cx, Cout, limit=0):
    """unet_conv3x3_up_bwd_weight_workspace_bytes"""
    m = 0
    for b16 in (False, True):
        r, s = _select_raw(N, h, w, Cx, Cout, 1, b16, 0, False, 0, limit, taps=True)
        m = max(m, wgrad_ws_floats(r, s))
    return 4 * m


# --------------------------------------------------------------------------- kernel names
def _b(v):
    return "true" if v else "false"


def _mangled(name, targs):
    """_ZN12_GLOBAL__N_1<name>I<targs>EEvNS_11WgradParamsE: a kernel of the anonymous namespace
    that takes WgradParams by value; targs: ints, bools and "bf16" (DF16b) in order.  The
    demangler gives up on __bf16 template arguments, so such launches are recorded mangled."""
    enc = "".join("DF16b" if a == "bf16" else f"Lb{int(a)}E" if isinstance(a, bool) else f"Li{a}E"
                  for a in targs)
    return f"_ZN12_GLOBAL__N_1{len(name)}{name}I{enc}EEvNS_11WgradParamsE"


def name_wgrad(ci, co, S, stride, act, b16, nw=4):
    """conv_wgrad_kernel<CI_T, CO_T, S, STRIDE, ACT, TX, TD, NW>"""
    if b16:
        return _mangled("conv_wgrad_kernel", (ci, co, S, stride, bool(act), "bf16", "bf16", nw))
    return f"conv_wgrad_kernel<{ci}, {co}, {S}, {stride}, {_b(act)}, float, float, {nw}>"


def name_bf16(ci, co, S, npl, sb, act, stride, b16):
    """conv_wgrad_bf16_kernel<CI_T, CO_T, S, NPL, SB, TX, TD, ACT, STRIDE>"""
    if b16:
        return _mangled("conv_wgrad_bf16_kernel",
                        (ci, co, S, npl, bool(sb), "bf16", "bf16", bool(act), stride))
    return (f"conv_wgrad_bf16_kernel<{ci}, {co}, {S}, {npl}, {_b(sb)}, float, float, {_b(act)}, "
            f"{stride}>")


def name_ring(ci, co, S, act, rg, stride):
    """conv_wgrad_b16_ring_kernel<CI_T, CO_T, S, ACT, DEPTH, RG, STRIDE>"""
    return f"conv_wgrad_b16_ring_kernel<{ci}, {co}, {S}, {_b(act)}, {K_RING_DEPTH}, {rg}, {stride}>"


def name_taps(ci, co, S, act, b16, nw=4):
    """conv_wgrad_taps_kernel<CI_T, CO_T, S, ACT, TX, TD, NW>"""
    if b16:
        return _mangled("conv_wgrad_taps_kernel", (ci, co, S, bool(act), "bf16", "bf16", nw))
    return f"conv_wgrad_taps_kernel<{ci}, {co}, {S}, {_b(act)}, float, float, {nw}>"


def name_taps_b16(ci, co, S, act):
    return f"conv_wgrad_taps_b16_kernel<{ci}, {co}, {S}, {_b(act)}>"


# the stem kernels take pointers, so their mangled names spell the parameter list
STEM_NAMES = {
    # (uint8 image, bf16 dy, raw-row form)
    (False, False, True): "conv_stem_wgrad_rows_kernel<float, float>",
    (True, False, True): "conv_stem_wgrad_rows_kernel<unsigned char, float>",
    (False, False, False): "conv_stem_wgrad_kernel<float>",
    (False, True, True): "_ZN12_GLOBAL__N_127conv_stem_wgrad_rows_kernelIfDF16bEEvPKT_PKT0_Pfiiiii"
                         "xNS_9StemNormWE",
    (True, True, True): "_ZN12_GLOBAL__N_127conv_stem_wgrad_rows_kernelIhDF16bEEvPKT_PKT0_Pfiiiii"
                        "xNS_9StemNormWE",
    (False, True, False): "_ZN12_GLOBAL__N_122conv_stem_wgrad_kernelIDF16bEEvPKfPKT_Pfiiiiix",
}


def wgrad_ring_ok(b16, pl, Ho, Cx, Cout, rg):
    return rg >= 1 and b16 and pl.segs_per_block % (K_RING_DEPTH * rg) == 0 and \
        Ho % pl.segs_per_block == 0 and pl.total_segs % pl.segs_per_block == 0 and \
        Cx % 8 == 0 and Cout % 8 == 0


def launch_wgrad8_s(ci, co, stride, S, act):
    nsb = (ci // 32) * (co // 32)
    smax = (128 if stride == 1 else 32) if nsb == 1 else \
        64 if nsb == 2 else (64 if stride == 1 else 32)
    if S in (128, 64) and smax >= S or S in (32, 16):
        return name_wgrad(ci, co, S, stride, act, False, nw=8)
    raise ValueError(f"conv_wgrad(8 waves): no instantiation for S={S}")


def launch_wgrad_taps_plan(pl, b16, act):
    if pl.nw == 8:
        if pl.ci_t == 64:
            return name_taps(64, 64, 32, act, False, nw=8)
        if pl.co_t == 64:
            return name_taps(32, 64, 32, act, False, nw=8)
        return name_taps(32, 32, 64, act, False, nw=8)
    if pl.ci_t == 64 and b16:
        return name_taps_b16(64, 64, 16, act)
    if pl.ci_t == 32 and pl.co_t == 32 and b16:
        return name_taps_b16(32, 32, 64, act)
    if pl.ci_t == 64:
        return name_taps(64, 64, 16, act, b16)
    if pl.co_t == 64:
        return name_taps(32, 64, 16, act, b16)
    return name_taps(32, 32, 32, act, b16)


def launch_wgrad_plan(pl, r, prec, act):
    """prec: WgradCall::prec (the call's, not the plan's)"""
    b16, stride = is_b16(r), r.stride
    ci, co, S = pl.ci_t, pl.co_t, pl.S
    Ho = out_size(r)[0]
    if pl.nw == 8:
        return launch_wgrad8_s(ci, co, stride, S, act)
    groups = (S // 16) % pl.npp == 0
    use_bf16 = prec != 0 and stride == 1 and groups and S >= 16
    ring_ok = wgrad_ring_ok(b16, pl, Ho, r.Cx, r.Cout, pl.rg)

    def bf16(ci, co, S, npl=1, sb=False):
        """launch_wgrad_bf16: bf16 tensors run the one-plane bf16-storage kernel of the tile"""
        if b16:
            return name_bf16(ci, co, S, 1, False, act, 1, True)
        if npl == 3 and act:
            return name_bf16(ci, co, S, 3, sb, True, 1, False)
        return name_bf16(ci, co, S, npl, sb, False, 1, False)

    if use_bf16 and prec == 3:
        if ci == 32 and co == 32:
            return bf16(32, 32, 64, 3, True)
        if ci == 32:
            return bf16(32, 64, 32, 3)
        return bf16(64, 64, 16, 3)
    if b16 and prec == 1 and stride == 2 and groups:
        if ring_ok:
            if ci == 64 and S == 16:
                return name_ring(64, 64, 16, act, pl.rg, 2)
            if ci == 32 and co == 64 and S == 32:
                return name_ring(32, 64, 32, act, pl.rg, 2)
        if ci == 64 and S == 16:
            return name_bf16(64, 64, 16, 1, False, act, 2, True)
        if ci == 32 and co == 64 and S == 32:
            return name_bf16(32, 64, 32, 1, False, act, 2, True)
    if use_bf16 and prec == 1 and ring_ok:
        if (ci, co, S) in ((32, 32, 64), (32, 64, 32)) or (ci == 64 and S in (32, 16)):
            return name_ring(ci, co, S, act, pl.rg, 1)
    if use_bf16 and prec == 1:
        if ci == 32 and co == 32:
            return bf16(32, 32, 64)
        if ci == 32:
            return bf16(32, 64, 32)
        return bf16(64, 64, 32) if S == 32 else bf16(64, 64, 16)
    if ci == 32 and co == 32:
        if stride == 1:
            return name_wgrad(32, 32, 64 if S == 64 else 32 if S == 32 else 16, 1, act, b16)
        return name_wgrad(32, 32, 32 if S == 32 else 16, 2, act, b16)
    if ci == 32 and co == 64:
        return name_wgrad(32, 64, 32 if S == 32 else 16, stride, act, b16)
    if stride == 1:
        return name_wgrad(64, 64, 32 if S == 32 else 16, 1, act, b16)
    return name_wgrad(64, 64, 16, 2, act, b16)


def launch_wgrad_stem(r):
    u8 = r.entry == "u8"
    if u8 and r.W % SW_PIX:
        raise ValueError("stem_u8_bwd_weight: needs W % 128 == 0")
    return STEM_NAMES[(u8, is_b16(r), u8 or r.W % SW_PIX == 0)]


# --------------------------------------------------------------------------- the whole call
def check(r):
    """what the entry points refuse"""
    assert r.stride in (1, 2) and r.Cout % 32 == 0
    assert r.Cx % 32 == 0 if r.entry not in ("stem", "u8") else r.Cx == 3
    if r.entry in ("stem", "u8"):
        assert r.stride == 1 and not r.act and not r.center
    if r.entry in ("conv3x3", "1x1"):
        assert not r.act and r.storage == "fp32", "plain fp32 operands"
    if r.entry == "1x1" or r.center:
        assert r.stride == 1
    if r.entry == "in":
        assert r.cores != 1 or is_b16(r), "activation on load: fp32, split or bf16 storage"
    if is_b16(r):
        assert r.entry in ("in", "up", "stem", "u8")


def launches(r):
    """-> one Launch per chunk, in launch order (the compute launches of the call)"""
    check(r)
    s = wgrad_select(r)
    assert s.nmax >= 1
    if s.form == "STEM":
        pl = make_plan_stem(r.N, r.H, r.W, r.Cout)
        return [Launch(launch_wgrad_stem(r), r.N, SW_PIX, 0, pl.stem_stages, pl.stem_spb,
                       pl.stem_blocks, 0)]
    out = []
    for nc in chunks_of(r, s):
        pl = wgrad_plan(r, s, nc)
        if s.form == "WINO32":
            name = f"conv_wgrad_wino32_kernel<{_b(r.act)}>"
        elif s.form == "WINO":
            name = f"conv_wgrad_wino_kernel<{_b(r.act)}>"
        elif s.form == "TAPS":
            name = launch_wgrad_taps_plan(pl, is_b16(r), r.act)
        else:
            name = launch_wgrad_plan(pl, r._replace(N=nc), call_prec(r), r.act)
        out.append(Launch(name, nc, pl.S, pl.segs_per_row, pl.total_segs, pl.segs_per_block,
                          pl.split, pl.rg))
    return out


def names(r):
    return tuple(l.name for l in launches(r))


def reduction_stages(r):
    """The reduction launches emit_wgrad_reduction queues for the call: 16-fold SLAB stages while
    more than 16 slabs remain, then the final job."""
    n = sum(l.split for l in launches(r))
    stages = 1
    while n > 16:
        n = ceil_div(n, K_SLAB_CHUNK)
        stages += 1
    return stages


# --------------------------------------------------------------------------- the grid
GRID_C = (32, 64, 96, 128, 256)
GRID_N = (1, 2, 3)
GRID_H = (4, 6, 8, 10, 12, 16, 20, 24, 25, 32, 40, 64)
GRID_W = (8, 16, 24, 32, 40, 48, 64, 80, 96, 128, 136)
# (entry, storage, cores, activation): storage x cores of the 3x3 entry points, activation on and
# off where the entry has both
GRID_MODES = (("conv3x3", "fp32", 0, False), ("in", "fp32", 0, True),
              ("conv3x3", "fp32", 1, False),
              ("conv3x3", "fp32", 3, False), ("in", "fp32", 3, True),
              ("in", "bf16", 1, False), ("in", "bf16", 1, True))
TAP_MODES = (("up", "fp32", 0, False), ("up", "fp32", 0, True),
             ("up", "bf16", 1, False), ("up", "bf16", 1, True))
STEM_MODES = (("stem", "fp32"), ("stem", "bf16"), ("u8", "fp32"), ("u8", "bf16"))


def grid_requests():
    """Every request of the grid tests/test_wgrad_fp64_gpu.py has to cover: the direct and
    Winograd forms over GRID_*, c32 at "always", then the tap entries over the same sizes and the
    stem over the same sizes with W = 128 and W = 24 (raw-row and generic form)."""
    for entry, storage, cores, act in GRID_MODES:
        for stride in (1, 2):
            for Cx in GRID_C:
                for Cout in GRID_C:
                    for N in GRID_N:
                        for H in GRID_H:
                            for W in GRID_W:
                                yield Request(entry, storage, cores, act, N, H, W, Cx, Cout,
                                              stride, False, 2, 0)
    for entry, storage, cores, act in TAP_MODES:
        for Cx in GRID_C:
            for Cout in GRID_C:
                for N, H, W in ((1, 4, 8), (2, 8, 16), (3, 25, 40)):
                    yield Request(entry, storage, cores, act, N, H, W, Cx, Cout, 1, False, 2, 0)
    for entry, storage in STEM_MODES:
        for W in ((128,) if entry == "u8" else (128, 24)):
            yield Request(entry, storage, 1 if storage == "bf16" else 0, False, 1, 4, W, 3, 32,
                          1, False, 2, 0)


def grid_names():
    """name -> the cheapest request of the grid that launches it (by N H W Cx Cout)"""
    best = {}
    for r in grid_requests():
        cost = r.N * r.H * r.W * r.Cx * r.Cout
        for l in launches(r):
            if l.name not in best or cost < best[l.name][0]:
                best[l.name] = (cost, r)
    return {k: v[1] for k, v in best.items()}


if __name__ == "__main__":
    for name, r in sorted(grid_names().items()):
        print(name, tuple(r), [tuple(l)[1:] for l in launches(r)])
