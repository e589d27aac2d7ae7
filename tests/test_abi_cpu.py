"""CPU (-m "not gpu"): libunet_hip.so loads, exports every symbol include/unet_hip.h declares,
and rejects bad arguments before any GPU work (no compute calls are made here); the ctypes binding
derived from the header has the rows and layouts pinned here, and the parser refuses what it does
not know."""
import ctypes
import os
import re
import struct

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unet_hip.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_expected_surface():
    names = declared_functions()
    for must in ["unet_conv3x3_fwd", "unet_conv3x3_bwd_data", "unet_conv3x3_bwd_weight",
                 "unet_instnorm_stats", "unet_instnorm_lrelu_drop_fwd",
                 "unet_instnorm_lrelu_drop_bwd", "unet_upsample2x_fwd", "unet_upsample2x_bwd",
                 "unet_head1x1_fwd", "unet_head1x1_bwd", "unet_dice_wce_loss_fwd_bwd",
                 "unet_sgd_nesterov_step", "unet_pack_conv3x3_weights", "unet_last_error"]:
        assert must in names


def test_library_exports_every_declared_symbol(ua):
    handle = ctypes.CDLL(ua.LIB_PATH)
    for name in declared_functions():
        assert hasattr(handle, name), f"{name} declared in unet_hip.h but not exported"


def test_python_binding_covers_every_declared_symbol(ua):
    assert sorted(ua._lib.SIGNATURES.keys()) == declared_functions()


# ---- the binding is derived from the header (_header.parse -> _lib.bind) -----------------------
_c = ctypes
_p, _i, _f, _d, _sz = _c.c_void_p, _c.c_int, _c.c_float, _c.c_double, _c.c_size_t
_pf, _pi = _c.POINTER(_c.c_float), _c.POINTER(_c.c_int)


def test_derived_rows_match_pinned_rows(ua):
    """A dozen rows spelled out by hand, covering every class of type the header uses."""
    L = ua._lib
    ps, pbs = _c.POINTER(L.ActSrc), _c.POINTER(L.BwdStats)
    pinned = {
        "unet_last_error": (_c.c_char_p, []),
        "unet_conv3x3_bwd_weight_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
        "unet_debug_set_chunk_limit": (_i, [_c.c_int64]),
        "unet_render_seg_panels": (_i, [_p, _i, _p, _p, _i, _p, _p, _i, _c.c_uint64, _p, _i, _i, _i,
                                        _p]),
        "unet_ssim_fwd": (_i, [_p, _p, _i, _pf, _f, _f, _p, _p, _p, _d, _d, _p, _sz, _i, _i, _i, _i,
                               _p]),
        "unet_conv_in_fwd": (_i, [ps, ps, _f, _p, _p, _i, _i, _p, _p, _sz, _pi, _i, _i, _i, _i,
                                  _p]),
        "unet_conv3x3_bwd_data_bs": (_i, [_p, _p, _i, _i, _p, _i, _i, _i, _i, _i, _i, _i, pbs, _p]),
        # the two tables are DEVICE memory (UNET_DEVICE): addresses, not POINTER(PackEntry)
        "unet_pack_conv3x3_weights_batched": (_i, [_p, _i, _i, _p]),
        "unet_pack_wino_weights_batched": (_i, [_p, _i, _i, _p]),
        "unet_stem_u8_fwd": (_i, [_p, _pf, _pf, _p, _p, _p, _p, _sz, _pi, _i, _i, _i, _i, _p]),
        "unet_sgd_nesterov_step": (_i, [_p, _p, _p, _c.c_int64, _f, _f, _f, _i, _f, _p]),
        "unet_debug_recorded_launches": (_sz, [_p, _sz]),
    }
    for name, (res, args) in pinned.items():
        got_res, got_args = L.SIGNATURES[name]
        assert got_res is res, name
        assert len(got_args) == len(args), name
        for k, (got, want) in enumerate(zip(got_args, args)):
            assert got is want, f"{name}: argument {k}"


def test_derived_struct_layouts(ua):
    L = ua._lib
    assert L.ActSrc._fields_ == [("x", _p), ("C", _i), ("alpha", _p), ("beta", _p)]
    assert L.BwdStats._fields_ == [
        ("y", _p), ("mean", _p), ("rstd", _p), ("gamma", _p), ("beta", _p), ("mask", _p),
        ("slope", _f), ("partial", _p), ("partial_bytes", _sz), ("tiles_out", _i)]
    assert [n for n, _ in L.PackEntry._fields_] == ["w", "wf", "wd", "wf3", "wd3", "Cout", "Cin",
                                                   "tile_begin", "reserved"]
    assert [n for n, _ in L.WinoPackEntry._fields_] == ["w", "uf", "ud", "Cout", "Cin",
                                                       "block_begin", "reserved"]
    # the records ops.PackTable uploads: the bytes of the "<5Q4i" / "<3Q4i" forms
    assert ctypes.sizeof(L.PackEntry) == 56 and ctypes.sizeof(L.WinoPackEntry) == 40
    v = (0x1122334455667788, 0x0102030405060708, 0x1112131415161718, 0x2122232425262728,
         0x3132333435363738, 96, 64, 12345, 1)
    assert bytes(L.PackEntry(*v)) == struct.pack("<5Q4i", *v)
    u = (0x1122334455667788, 0x0102030405060708, 0x1112131415161718, 128, 72, 54321, 7)
    assert bytes(L.WinoPackEntry(*u)) == struct.pack("<3Q4i", *u)
    # a null destination is written as 0
    assert bytes(L.WinoPackEntry(u[0], 0, 0, *u[3:])) == struct.pack("<3Q4i", u[0], 0, 0, *u[3:])


# (function, parameter) of every pointer the host dereferences: typed POINTER(c_float / c_int)
HOST_POINTERS = sorted(
    [(f, p) for f in ("unet_preprocess_u8", "unet_stem_u8_fwd", "unet_stem_u8_bwd_weight",
                      "unet_stem_u8_fwd_b16", "unet_stem_u8_bwd_weight_b16",
                      "unet_stem_in_bwd_weight_fold", "unet_perceptual_prep", "unet_vit_patchify")
     for p in ("mean3", "std3")] +
    [("unet_perceptual_stem_bwd_data", "std3"), ("unet_ssim_fwd", "gauss11"),
     ("unet_ssim_grad", "gauss11")] +
    [(f, "stats_px_out") for f in (
        "unet_conv_in_fwd", "unet_conv_in_fwd_bf16x3", "unet_conv_up_in_fwd", "unet_stem_u8_fwd",
        "unet_stem_u8_fwd_b16", "unet_conv_in_fwd_wino", "unet_conv_up_in_fwd_wino",
        "unet_conv_in_fwd_b16", "unet_conv_in_fwd_b16_wb", "unet_conv_up_in_fwd_b16")])


def test_unet_host_marks_exactly_the_host_pointers(ua):
    hdr = ua._lib._HDR
    marked = sorted((f, p) for f, (_, params) in hdr.functions.items()
                    for t, p in params if "UNET_HOST" in t.split())
    assert marked == HOST_POINTERS
    typed = sorted((f, p) for f, (_, params) in hdr.functions.items()
                   for (_, p), a in zip(params, ua._lib.SIGNATURES[f][1]) if a in (_pf, _pi))
    assert typed == HOST_POINTERS
    for f, p in HOST_POINTERS:
        k = [n for _, n in hdr.functions[f][1]].index(p)
        assert ua._lib.SIGNATURES[f][1][k] is (_pi if p == "stats_px_out" else _pf)
    device_tables = sorted((f, p) for f, (_, params) in hdr.functions.items()
                           for t, p in params if "UNET_DEVICE" in t.split())
    assert device_tables == [("unet_pack_conv3x3_weights_batched", "table_device"),
                             ("unet_pack_wino_weights_batched", "table_device")]


MINI_HEADER = """
#ifndef X_H_
#define X_H_
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#define UNET_ABI_VERSION 3
#define UNET_HOST
typedef void* unet_stream_t; /* hipStream_t */
typedef struct unet_rec {
  const float* x; /* a comment; with (punctuation) */
  int a, b;
} unet_rec;
const char* unet_name(void);
// a line comment with a unet_ghost(int) in it
int unet_f(const unet_rec* r, const float* UNET_HOST m, float* y, size_t n,
           unet_stream_t stream);
size_t unet_g(int64_t n);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_reads_the_subset_and_fails_loudly(ua):
    H = ua._lib._header
    hdr = H.parse(MINI_HEADER)
    assert hdr.version == 3
    assert hdr.structs == {"unet_rec": [("const float*", "x"), ("int", "a"), ("int", "b")]}
    assert hdr.functions == {
        "unet_name": ("const char*", []),
        "unet_f": ("int", [("const unet_rec*", "r"), ("const float* UNET_HOST", "m"),
                           ("float*", "y"), ("size_t", "n"), ("unet_stream_t", "stream")]),
        "unet_g": ("size_t", [("int64_t", "n")])}
    structs, sigs = ua._lib.bind(hdr)
    assert sigs["unet_f"] == (_i, [_c.POINTER(structs["unet_rec"]), _pf, _p, _sz, _p])
    assert sigs["unet_name"] == (_c.c_char_p, []) and sigs["unet_g"] == (_sz, [_c.c_int64])
    # a declaration removed from the text is a name missing from the binding
    without = MINI_HEADER.replace("size_t unet_g(int64_t n);", "")
    assert sorted(ua._lib.bind(H.parse(without))[1]) == ["unet_f", "unet_name"]

    def broken(old, new):
        assert old in MINI_HEADER
        return MINI_HEADER.replace(old, new)
    # an unknown type, in a parameter and in a struct
    with pytest.raises(H.HeaderError, match=r"unet_g.*long double"):
        H.parse(broken("int64_t n", "long double x"))
    with pytest.raises(H.HeaderError, match=r"unet_rec.*unsigned"):
        H.parse(broken("int a, b;", "unsigned a;"))
    # an unterminated declaration: at the end of the text, and in front of another one
    with pytest.raises(H.HeaderError, match=r"unterminated.*unet_g"):
        H.parse(broken("size_t unet_g(int64_t n);", "size_t unet_g(int64_t n)"))
    with pytest.raises(H.HeaderError, match=r"unet_name"):
        H.parse(broken("unet_name(void);", "unet_name(void)"))
    # a pointer to a struct the text never defines
    with pytest.raises(H.HeaderError, match=r"unet_f.*unet_foo\*.*does not define"):
        H.parse(broken("const unet_rec* r", "const unet_foo* r"))
    # things outside the subset are refused, not skipped
    for old, new, offender in [
            ("size_t unet_g(int64_t n);", "static int unet_h(int n) { return n; }", "unet_h"),
            ("size_t unet_g(int64_t n);", "size_t unet_g(int64_t);", "int64_t"),
            ("size_t unet_g(int64_t n);", "size_t unet_g(int64_t n); int unet_g(int n);", "unet_g"),
            ("#include <stddef.h>", "#pragma pack(1)", "pragma"),
            ("float* y", "float** y", r"float\*\*"),
            ("const float* UNET_HOST m", "const void* UNET_HOST m", "UNET_HOST"),
            ("#define UNET_ABI_VERSION 3", "", "UNET_ABI_VERSION")]:
        with pytest.raises(H.HeaderError, match=offender):
            H.parse(broken(old, new))


def test_missing_header_fails_loudly(ua, monkeypatch, tmp_path):
    monkeypatch.setattr(ua._lib, "HEADER", str(tmp_path / "nope.h"))
    with pytest.raises(ua.UNetHipError, match="nope.h"):
        ua._lib._parse_header()


def test_abi_version_and_device_count(ua):
    lib = ua.lib()
    header_version = int(re.search(r"#define\s+UNET_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert lib.unet_abi_version() == header_version == ua._lib.ABI_VERSION
    assert lib.unet_device_count() >= 0


def test_argument_validation_without_gpu(ua):
    lib = ua.lib()
    # null pointers / bad shapes are rejected by the host-side checks (no launch happens)
    rc = lib.unet_conv3x3_fwd(None, 32, None, 0, None, None, None, 1, 8, 8, 32, 1, None)
    assert rc == -1 and b"null" in lib.unet_last_error()
    rc = lib.unet_conv3x3_fwd(1, 32, None, 0, 1, None, 1, 1, 8, 8, 48, 1, None)
    assert rc == -1 and b"multiple of 32" in lib.unet_last_error()
    rc = lib.unet_conv3x3_fwd(1, 32, None, 0, 1, None, 1, 1, 8, 8, 32, 3, None)
    assert rc == -1 and b"stride" in lib.unet_last_error()
    rc = lib.unet_conv3x3_bwd_data(1, 1, 64, 48, 1, 1, 8, 8, 32, 32, 1, 0, None)
    assert rc == -1   # slice 48..80 exceeds Cin_total 64
    rc = lib.unet_head1x1_fwd(1, 1, 1, 1, 1, 64, 16, 3, None)
    assert rc == -1 and b"C == 32" in lib.unet_last_error()
    rc = lib.unet_sgd_nesterov_step(4, 16, 16, 100, 0.1, 0.9, 0.0, 1, 1.0, None)
    assert rc == -1 and b"aligned" in lib.unet_last_error()


def test_workspace_queries(ua):
    lib = ua.lib()
    assert lib.unet_conv3x3_bwd_weight_workspace_bytes(8, 512, 512, 32, 32, 1) > 9 * 32 * 32 * 4
    assert lib.unet_conv3x3_bwd_weight_workspace_bytes(8, 512, 512, 3, 32, 1) > 0
    assert lib.unet_conv3x3_bwd_weight_workspace_bytes(0, 512, 512, 32, 32, 1) == 0
    assert lib.unet_instnorm_workspace_bytes(8, 512 * 512, 32) > 0
    assert lib.unet_head1x1_bwd_workspace_bytes(8, 512 * 512, 32, 3) > 0
    assert lib.unet_dice_wce_loss_workspace_bytes(8, 512, 512) > 0


def test_missing_library_fails_loudly(ua, monkeypatch, tmp_path):
    monkeypatch.setattr(ua._lib, "_lib", None)
    monkeypatch.setattr(ua._lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(ua.UNetHipError, match="no CPU / eager fallback"):
        ua._lib.lib()
