"""ctypes binding of libfvit_hip.so (C ABI declared in include/fvit_hip.h).

The function signatures are read from the header when the library is loaded (parse_header); only the structs and FVIT_* constants
are written out here, and tests/test_abi.py holds them to the header field by field.  A new entry point needs the header and its
kernel file, and this file only for a new struct or constant.

The product path has no CPU or eager-PyTorch fallback: if the HIP library is missing or fails to
load, everything that needs it raises RuntimeError.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import re
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC_DIR = os.path.join(_HERE, "csrc")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "fvit_hip.h")   # csrc/Makefile's ../../include/fvit_hip.h
DIAG = os.environ.get("FVIT_DIAG", "0") == "1"   # diagnosis build (scripts/timeline_*.py, scripts/poison_check.py, the poison test's subprocess)
LIB_PATH = os.path.join(CSRC_DIR, "libfvit_hip_diag.so" if DIAG else "libfvit_hip.so")
# A/B measurements only (scripts/r06_calls): another build of the same ABI, e.g. the previous round's kernels, selected per process
if os.environ.get("FVIT_LIB_PATH"):
    LIB_PATH = os.path.abspath(os.environ["FVIT_LIB_PATH"])

FVIT_ABI_VERSION = 10
FVIT_F32, FVIT_F16, FVIT_BF16 = 0, 1, 2
FVIT_U8 = 3   # FvitMapView.dtype of a uint8 image: the fvit_*_u8 entry points only
FVIT_TILE_N, FVIT_TILE_K = 128, 64
FVIT_MASK_BIAS = -30000.0
FVIT_MAX_DENSE_SEQ = 208   # longer window sequences use the online-softmax attention kernel with the compact bias table
FVIT_PROF_KINDS = 11
FVIT_DET_MAX_SETS = 16
FVIT_BOX_IOU, FVIT_BOX_GIOU = 0, 1
FVIT_RESIZE_BILINEAR, FVIT_RESIZE_BICUBIC = 1, 2
# fvit_image_resize_check's reason codes
FVIT_RESIZE_REASONS = {-16: "size", -17: "filter", -18: "window", -19: "slot", -20: "stride", -21: "tap limit", -22: "LDS limit"}
# EXPORTED_SYMBOLS / DIAG_SYMBOLS (module attributes, see __getattr__): the names the header declares outside / inside its #ifdef FVIT_DIAG
# section.  The second set is only in libfvit_hip_diag.so (the same sources with -DFVIT_DIAG; FVIT_DIAG=1 selects it); the shipped library
# exports none of them and compiles the ablation knobs out (tests/test_abi.py).


class FvitDebugRowhashRecord(C.Structure):
    _fields_ = [("tag", C.c_char * 24), ("offset", C.c_int64), ("rows", C.c_int64)]


class FvitStageDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "batch", "C", "heads", "dpad", "ws", "H", "W", "Hp", "Wp", "cw", "hier", "square", "hidden",
        "depth", "do_propagation", "operand_dtype", "spad", "gpad")] + [("qk_scale", C.c_float), ("weight_terms", C.c_int32)]


class FvitAttnWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("w_qkv", "b_qkv", "w_proj", "b_proj", "bias", "ln_w", "ln_b", "gamma",
                                                  "w_qkv_frag", "b_qkv_heads", "w_proj_frag", "rel_table")] + \
               [("rel_w", C.c_int32), ("rel_ng", C.c_int32)]


class FvitMlpWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("w_fc1", "b_fc1", "w_fc2", "b_fc2", "ln_w", "ln_b", "gamma", "w_fc1_frag", "w_fc2_frag")]


class FvitBlockWeights(C.Structure):
    _fields_ = [("attn", FvitAttnWeights), ("mlp", FvitMlpWeights), ("hat_attn", FvitAttnWeights),
                ("hat_mlp", FvitMlpWeights), ("pe_x", C.c_void_p), ("pe_ct", C.c_void_p),
                ("last", C.c_int32), ("_pad", C.c_int32)]


class FvitStageTables(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("ln1_src", "ln1_add", "ct_src", "up_idx")]


class FvitStageTail(C.Structure):
    _fields_ = [("ln_w", C.c_void_p), ("ln_b", C.c_void_p), ("pool_out", C.c_void_p), ("ln_eps", C.c_float), ("pool_dtype", C.c_int32)]


class FvitMapView(C.Structure):
    _fields_ = [("data", C.c_void_p), ("stride_b", C.c_int64), ("stride_c", C.c_int64), ("stride_h", C.c_int64),
                ("stride_w", C.c_int64), ("dtype", C.c_int32), ("_pad", C.c_int32)]


class FvitResizeDesc(C.Structure):
    _fields_ = [("src", C.c_void_p), ("row_stride", C.c_int64)] + \
               [(n, C.c_int32) for n in ("H", "W", "rh", "rw", "top", "left", "ch", "cw", "filter", "_pad")]


class FvitDetLabelSet(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("logits", "classes", "targets", "grad_logits")] + [(n, C.c_int32) for n in ("R", "Q", "B")] + [("scale", C.c_float)]


class FvitDetBoxSet(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("src", "tgt", "grad_src")] + [("M", C.c_int32), ("scale", C.c_float)]


class FvitDetAssignSet(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("cost", "src", "tgt")] + [(n, C.c_int32) for n in ("Q", "T", "n_pairs", "_pad")]


class FvitConvWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("classic", "dense", "band_frag")] + [("terms", C.c_int32), ("cin_valid", C.c_int32)]


class FvitConvCall(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("in_", "in_lo", "bias", "residual", "residual_lo", "out", "out_lo", "out_f32", "ln_w", "ln_b", "zeros")] + \
               [("ln_eps", C.c_float)] + [(n, C.c_int32) for n in ("B", "Hi", "Wi", "Cin", "Cout", "stride", "act", "px")]


class FvitProfEntry(C.Structure):
    _fields_ = [("launches", C.c_int64), ("ms", C.c_double), ("flops", C.c_double), ("bytes", C.c_double)]


class FvitProfRecord(C.Structure):
    _fields_ = [("kind", C.c_int32), ("grid", C.c_int32), ("ms", C.c_float), ("_pad", C.c_float), ("flops", C.c_double),
                ("bytes", C.c_double), ("name", C.c_char * 40)]


_lib = None


def build(verbose: bool = False) -> str:
    """Compile libfvit_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC_DIR, "-j4"]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose:
        print(res.stdout)
    if res.returncode != 0 or not os.path.isfile(LIB_PATH):
        raise RuntimeError("building libfvit_hip.so failed:\n" + res.stdout)
    return LIB_PATH


_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "size_t": C.c_size_t,
            "float": C.c_float, "double": C.c_double}
# parameters that are not bound as the header types them, by (function, parameter name)
_ARG_OVERRIDES = {
    # `const FvitResizeDesc* descs` is an array in DEVICE memory: callers pass descs.data_ptr(), never a host struct
    ("fvit_image_resize_u8", "descs"): C.c_void_p,
}


def ctype_of(decl: str, where: str):
    """(ctypes type, declared name or "") of one C return type, parameter or field: `int32_t S`, `const float* x`, `const FvitMapView* in`.
    Scalars by width, `const char*` as c_char_p, fvit_stream_t / void* / a pointer to a scalar as c_void_p, a pointer to a struct of this
    module as POINTER(struct); anything else raises RuntimeError naming `where`."""
    toks = [t for t in re.findall(r"\w+|[^\w\s]", decl) if t != "const"]
    name = toks.pop() if len(toks) > 1 and re.fullmatch(r"\w+", toks[-1]) else ""
    base, stars = (toks[0] if toks else ""), toks.count("*")
    struct, t = globals().get(base), None
    if len(toks) != 1 + stars or stars > 1:   # `unsigned int`, an array, a function pointer, a pointer to a pointer
        pass
    elif stars == 0:
        t = C.c_void_p if base == "fvit_stream_t" else _SCALARS.get(base)
    elif base == "char":
        t = C.c_char_p
    elif base == "void" or base in _SCALARS:
        t = C.c_void_p
    elif isinstance(struct, type) and issubclass(struct, C.Structure):
        t = C.POINTER(struct)
    if t is None:
        raise RuntimeError(f"include/fvit_hip.h: {where}: the binding has no ctypes type for `{' '.join(decl.split())}`")
    return t, name


def parse_header(text: str):
    """The prototypes of include/fvit_hip.h's text as two dicts {name: (restype, [argtypes])}: the product section, and the
    `#ifdef FVIT_DIAG` ... `#endif /* FVIT_DIAG */` section (libfvit_hip_diag.so only)."""
    a, b = text.index("#ifdef FVIT_DIAG"), text.index("#endif /* FVIT_DIAG */")
    sections = []
    for part in (text[:a] + text[b:], text[a:b]):
        part = re.sub(r"/\*.*?\*/|//[^\n]*", " ", part, flags=re.S)   # comments first: a #define's comment may run over several lines
        part = re.sub(r"^[ \t]*#.*$", "", part, flags=re.M)
        sigs = {}
        for ret, fn, params in re.findall(r"([\w\s*]+?)\b(fvit_\w+)\s*\(([^()]*)\)\s*;", part):
            restype, stray = ctype_of(ret, fn)
            if stray:
                raise RuntimeError(f"include/fvit_hip.h: {fn}: the binding cannot read the return type `{' '.join(ret.split())}`")
            argtypes = []
            for p in ([] if params.strip() in ("", "void") else params.split(",")):
                t, name = ctype_of(p, fn)
                argtypes.append(_ARG_OVERRIDES.get((fn, name), t))
            sigs[fn] = (restype, argtypes)
        sections.append(sigs)
    return tuple(sections)


@functools.lru_cache(maxsize=None)
def _signatures():
    if not os.path.isfile(HEADER_PATH):
        raise RuntimeError(f"{HEADER_PATH} not found: the ctypes signatures of libfvit_hip.so are read from it")
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


def __getattr__(name):
    if name in ("EXPORTED_SYMBOLS", "DIAG_SYMBOLS"):
        return tuple(_signatures()[name == "DIAG_SYMBOLS"])
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def lib():
    """Load (once) and return the ctypes handle; raises RuntimeError when the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the FasterViT HAT path has no CPU/eager fallback. Build it with "
            "`make -C fastervit_amd/csrc -j` (or `python -c 'import __graft_entry__ as g; g.build()'`).")
    try:
        handle = C.CDLL(LIB_PATH)
    except OSError as e:  # e.g. libamdhip64 missing
        raise RuntimeError(f"cannot load {LIB_PATH}: {e}") from e
    product, diag = _signatures()
    declared = {**product, **diag} if DIAG else product
    missing = [s for s in declared if not hasattr(handle, s)]
    if missing:
        raise RuntimeError(f"{LIB_PATH} lacks symbols {missing}; rebuild it")
    for name, (restype, argtypes) in declared.items():
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = restype, argtypes
    if handle.fvit_abi_version() != FVIT_ABI_VERSION:
        raise RuntimeError(f"ABI mismatch: library {handle.fvit_abi_version()} vs binding {FVIT_ABI_VERSION}")
    _lib = handle
    return _lib


def stream_ptr(device=None) -> int:
    """Raw hipStream_t of torch's current stream ON ``device`` (not on the thread's current device: a model moved with
    ``.to('cuda:1')`` and called while cuda:0 is current must launch on a cuda:1 stream)."""
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t):
    """The device pointer of a tensor, None (a null pointer) for None."""
    return t.data_ptr() if t is not None else None


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().fvit_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def tune(key: str, value: int) -> None:
    check(lib().fvit_tune(key.encode(), int(value)), "fvit_tune")


def prof_enable(on: bool) -> None:
    check(lib().fvit_prof_enable(1 if on else 0), "fvit_prof_enable")


def prof_collect() -> dict:
    """Return {kind_name: dict(launches, ms, flops, bytes)} for the launches since prof_enable(True)."""
    arr = (FvitProfEntry * FVIT_PROF_KINDS)()
    check(lib().fvit_prof_collect(arr), "fvit_prof_collect")
    out = {}
    for k in range(FVIT_PROF_KINDS):
        e = arr[k]
        out[lib().fvit_prof_kind_name(k).decode()] = dict(launches=int(e.launches), ms=float(e.ms), flops=float(e.flops),
                                                         bytes=float(e.bytes))
    return out


def prof_records(max_records: int = 65536) -> list:
    """Per-launch records since prof_enable(True): dicts(kind, name, grid, ms, flops, bytes) in launch order."""
    arr = (FvitProfRecord * max_records)()
    n = lib().fvit_prof_records(arr, max_records)
    if n < 0:
        check(n, "fvit_prof_records")
    kinds = [lib().fvit_prof_kind_name(k).decode() for k in range(FVIT_PROF_KINDS)]
    return [dict(kind=kinds[arr[i].kind] if 0 <= arr[i].kind < FVIT_PROF_KINDS else "other", name=arr[i].name.decode("utf-8", "replace"),
                 grid=int(arr[i].grid), ms=float(arr[i].ms), flops=float(arr[i].flops), bytes=float(arr[i].bytes)) for i in range(n)]
