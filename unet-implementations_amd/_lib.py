"""ctypes binding of libunet_hip.so, derived from the C ABI declared in include/unet_hip.h.

The header is the one description of the ABI: at import `_header.parse` reads it and the argument
types, the struct layouts and the ABI version below are built from what it declares.

The library is built in-tree by `build()` (hipcc, --offload-arch=gfx950) and is
the ONLY compute path of this package: there is no CPU or eager-PyTorch
fallback.  `lib()` raises if the shared object is missing.
"""
import ctypes
import os
import subprocess

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
# UNET_HIP_LIB selects an alternative in-tree build (A/B experiments of kernel variants)
LIB_PATH = os.environ.get("UNET_HIP_LIB") or os.path.join(_HERE, "libunet_hip.so")
CSRC = os.path.join(_HERE, "csrc")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "unet_hip.h")


class UNetHipError(RuntimeError):
    pass


def _parse_header():
    try:
        with open(HEADER) as f:
            return _header.parse(f.read())
    except OSError as e:
        raise UNetHipError(f"{HEADER} is missing or unreadable ({e}): the ctypes binding is "
                           "derived from it") from None


_CTYPES = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double,
           "size_t": ctypes.c_size_t, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
           "void*": ctypes.c_void_p, "char*": ctypes.c_char_p}


def bind(hdr):
    """A parsed header -> (its structs as ctypes classes by C name, name -> (restype, argtypes))."""
    structs, names = {}, frozenset(hdr.structs)

    def ctype(c, is_return=False):
        kind = _header.classify(c, names, is_return)
        if isinstance(kind, str):
            return _CTYPES[kind]
        # a UNET_HOST scalar the host dereferences, or one of the header's structs: typed
        # pointers, so that a device address passed as an int is rejected
        return ctypes.POINTER(_CTYPES[kind[1]] if kind[0] == "host" else structs[kind[1]])

    # `typedef struct unet_act_src` -> class ActSrc, fields in the header's order (the members
    # are scalars and untyped pointers: the parser refuses anything else)
    for name, fields in hdr.structs.items():
        structs[name] = type("".join(w.capitalize() for w in name.split("_")[1:]),
                             (ctypes.Structure,),
                             {"_fields_": [(field, ctype(c)) for c, field in fields],
                              "__doc__": f"`{name}` of include/unet_hip.h."})
    return structs, {name: (ctype(ret, is_return=True), [ctype(c) for c, _ in params])
                     for name, (ret, params) in hdr.functions.items()}


_HDR = _parse_header()
ABI_VERSION = _HDR.version
STRUCTS, SIGNATURES = bind(_HDR)
ActSrc = STRUCTS["unet_act_src"]
BwdStats = STRUCTS["unet_bwd_stats"]
PackEntry = STRUCTS["unet_pack_entry"]
WinoPackEntry = STRUCTS["unet_wino_pack_entry"]

_lib = None


def build(verbose=False):
    """Compile libunet_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    jobs = str(min(8, os.cpu_count() or 1))
    proc = subprocess.run(["make", "-C", CSRC, "-j", jobs], capture_output=True, text=True)
    if verbose or proc.returncode != 0:
        print(proc.stdout)
        print(proc.stderr)
    if proc.returncode != 0:
        raise UNetHipError("building libunet_hip.so failed (see output above)")
    return LIB_PATH


def lib():
    """Load (once) and return the ctypes handle; raises if the library is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise UNetHipError(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU / eager fallback for the HIP path)")
    # torch must be imported first so its bundled libamdhip64.so.7 (same soname) is the
    # one HIP runtime of the process: streams and device pointers are then shared.
    import torch  # noqa: F401
    handle = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(handle, name)  # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    if handle.unet_abi_version() != ABI_VERSION:
        raise UNetHipError("libunet_hip.so ABI version mismatch; rebuild")
    _lib = handle
    return _lib


def check(rc):
    if rc != 0:
        msg = lib().unet_last_error()
        raise UNetHipError(f"libunet_hip error {rc}: {msg.decode() if msg else '?'}")
