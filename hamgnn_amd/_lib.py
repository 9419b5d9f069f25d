"""ctypes binding of libhamgnn_hip.so (the C ABI in include/hamgnn_hip.h).  There is NO CPU fallback: if the library is
missing or a call fails, this raises.  `call` is the typed way in: every argument is converted and checked against the prototype that
the header declares (parsed once, on load; no second table of signatures).  `lib()` is the raw handle with no argtypes (benches, HG_PROF reads)."""
from __future__ import annotations

import ctypes as C
import numbers
import os
import re
import subprocess

import numpy as np
import torch      # before the library: it must bind to the HIP runtime PyTorch already loaded (its bundled libamdhip64), not open a second copy

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HG_LIB_PATH", os.path.join(_HERE, "lib", "libhamgnn_hip.so"))   # override: kernel-variant A/B runs
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "hamgnn_hip.h")              # the file the C sources include
_lib = None
_bound: dict = {}            # entry point -> (typed function, converters, takes a stream); filled on load
_ops = None                  # hamgnn_amd.ops, for its _require_gpu (imported on load: ops imports this module)
_raw_stream, _cur_device = (getattr(torch._C, n, None) for n in ("_cuda_getCurrentRawStream", "_cuda_getDevice"))     # torch.cuda.current_stream().cuda_stream
#                            without building the Stream object (measured in profiles/abi_binding.md, section 1); the public expression where a torch build lacks either

EXPORTS = ["hg_last_error", "hg_version", "hg_scratch_bytes", "hg_edge_geometry", "hg_radial_basis", "hg_radial_hidden", "hg_rotate_gather", "hg_tp_fused", "hg_tp_is", "hg_tp_wgrad", "hg_row_program",
           "hg_segment_sum", "hg_gate", "hg_add_rows", "hg_to_planar", "hg_from_planar", "hg_embed_lookup", "hg_ham_merge",
           "hg_ham_finish", "hg_ham_readout", "hg_block_mean", "hg_soc_assemble", "hg_zero_point_shift", "hg_sym_contraction", "hg_sym_contraction3", "hg_sym_contraction_nu", "hg_sym_contraction_nu_backward", "hg_hk_assemble", "hg_hk_assemble_adjoint",
           "hg_attn_logits", "hg_attn_aggregate", "hg_linear_planar", "hg_linear_wgrad", "hg_block_gemm", "hg_gate_backward", "hg_radial_hidden_multi", "hg_mfma_probe", "hg_build_config", "hg_norm_act", "hg_norm_act_backward", "hg_w3_split_refill", "hg_kan_hidden",
           "hg_neighbour_bin", "hg_neighbour_pairs", "hg_neighbour_decode", "hg_mulliken_weights", "hg_dos_broaden", "hg_dos_tetra", "hg_bond_weights",
           "hg_density_rows", "hg_kgrad_elements"]


def build(verbose=False):
    """Compile the HIP extension in-tree (hipcc --offload-arch=gfx950)."""
    r = subprocess.run(["make", "-C", os.path.join(_HERE, "csrc"), "-j4"], capture_output=True, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout[-4000:], r.stderr[-4000:])
    if r.returncode != 0:
        raise RuntimeError("building libhamgnn_hip.so failed")
    return LIB_PATH


# ------------------------------------------------------------------------------------------------ the header as the source of the signatures
_INTS = {"int": C.c_int, "int64_t": C.c_int64}
_REALS = {"float": C.c_float, "double": C.c_double}
_ELEMS = {"float": (torch.float32, C.c_float), "double": (torch.float64, C.c_double), "int32_t": (torch.int32, C.c_int32),
          "int64_t": (torch.int64, C.c_int64), "void": (None, None)}             # pointee -> (tensor dtype, element of a host array)


def _kind(spelling):
    """(kind, base type) of a C type spelling of the header; a spelling that is not known is an error, never an unchecked argument"""
    if spelling in _INTS:
        return "int", spelling
    if spelling in _REALS:
        return "real", spelling
    if spelling == "const char*":
        return "str", None
    m = re.fullmatch(r"(?:const )?(\w+)\*( const\*)?", spelling)
    if m and m.group(1) in _ELEMS:
        return ("ptrs" if m.group(2) else "ptr"), m.group(1)
    raise ValueError(f"hamgnn_hip.h: unknown type spelling {spelling!r}")


def parse_header(text):
    """{entry point: (return type, [(C type, parameter name), ...])} of every hg_* prototype in the header text"""
    code = re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.M)
    norm = lambda t: " ".join(t.split()).replace(" *", "*")
    protos = {}
    for ret, name, plist in re.findall(r"([A-Za-z_][\w\s*]*?)\b(hg_\w+)\s*\(([^()]*)\)\s*;", code):
        if _kind(norm(ret))[0] not in ("int", "str"):
            raise ValueError(f"hamgnn_hip.h: {name} returns {norm(ret)!r}")
        params = []
        for p in ([] if plist.strip() == "void" else plist.split(",")):
            ctype, pname = re.fullmatch(r"\s*(.*?)(\w+)\s*", p, flags=re.S).groups()
            _kind(norm(ctype))
            params.append((norm(ctype), pname))
        protos[name] = (norm(ret), params)
    return protos


def host_arrays(text, protos):
    """predicate (C type, parameter name) -> the parameter is an array in HOST memory.  From the header's own words: the names its conventions block lists
    between backquotes as "host arrays", every parameter called *_host, and the arrays of pointers (`src`, `src_idx`: `T* const*`).  A listed name that
    is such a pointer array where it is meant (`src`) does not make a plain pointer of the same name elsewhere (hg_attn_logits' sender index) a host array."""
    m = re.search(r"EXCEPT the tiny\s+\W*host arrays(.*?)\(", text, flags=re.S)
    named = set(re.findall(r"`(\w+)`", m.group(1))) if m else set()
    params = [p for _, ps in protos.values() for p in ps]
    if not named or named - {n for _, n in params}:
        raise ValueError(f"hamgnn_hip.h: the conventions block no longer lists its host arrays as parameter names between backquotes (found {sorted(named)})")
    named -= {n for t, n in params if t.endswith("* const*")}
    return lambda ctype, name: ctype.endswith("* const*") or (ctype.endswith("*") and (name in named or name.endswith("_host")))


class strided:
    """marks a tensor argument of `call` as the pointer of a (pointer, row stride) pair: only its last stride has to be 1"""
    __slots__ = ("t",)

    def __init__(self, t):
        self.t = t


def _converter(entry, ctype, pname, host):
    """the function that checks one argument of `entry` against its declared type and returns what ctypes passes on"""
    kind, base = _kind(ctype)
    what = f"{entry}: {pname}"
    if kind == "int":
        bound = 1 << (C.sizeof(_INTS[base]) * 8 - 1)

        def conv(v):
            if type(v) is not int:
                if not isinstance(v, numbers.Integral):
                    raise TypeError(f"{what} ({ctype}) takes an integer, got {type(v).__name__}")
                v = int(v)
            if not -bound <= v < bound:
                raise ValueError(f"{what} = {v} does not fit {ctype}")
            return v
    elif kind == "real":
        def conv(v):
            if type(v) is float:
                return v
            if not isinstance(v, numbers.Real):
                raise TypeError(f"{what} ({ctype}) takes a real number, got {type(v).__name__}")
            return float(v)
    elif kind == "str":
        def conv(v):
            if v is not None and type(v) is not bytes:
                raise TypeError(f"{what} ({ctype}) takes bytes or None, got {type(v).__name__}")
            return v
    elif host:
        elem = C.c_void_p if kind == "ptrs" else _ELEMS[base][1]
        one = _converter(entry, ctype[:-len(" const*")], pname + "[.]", False) if kind == "ptrs" else None

        def conv(a):
            if a is None or (isinstance(a, C.Array) and a._type_ is elem):
                return a
            if one is not None and isinstance(a, (list, tuple)):      # an array of pointers from its tensors (None: NULL), each checked as a strided() one
                return (elem * len(a))(*[one(t, True) for t in a])
            if isinstance(a, np.ndarray) and a.flags.c_contiguous and a.dtype == np.dtype(elem):
                return a.ctypes.data
            raise ValueError(f"{what} is a host array: it takes a ctypes array or a C-contiguous numpy array of {elem.__name__}, got "
                             f"{type(a).__name__}{' ' + str(a.dtype) if hasattr(a, 'dtype') else ''}")
    else:
        dtype = _ELEMS[base][0]

        def conv(a, loose=False):
            t = a.t if type(a) is strided else a
            loose = loose or t is not a
            if t is None:
                return None
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{what} ({ctype}) is a device pointer: it takes a tensor or None, got {type(t).__name__}")
            if dtype is not None and t.dtype is not dtype:
                raise ValueError(f"{what} ({ctype}) must be {dtype}, got {t.dtype}")
            if not t.is_contiguous() and not (loose and t.dim() and t.stride(-1) == 1):
                raise ValueError(f"{what}: strided() needs a last stride of 1, got strides {tuple(t.stride())}" if loose else f"{what} must be contiguous")
            if not t.is_cuda:
                _ops._require_gpu(t)
            return t.data_ptr()
    return conv


def lib():
    global _lib, _ops
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(the MI355X hot path has no CPU fallback)")
        text = open(HEADER_PATH).read()
        protos = parse_header(text)
        if set(protos) != set(EXPORTS):
            raise RuntimeError(f"include/hamgnn_hip.h and _lib.EXPORTS differ: {sorted(set(protos) ^ set(EXPORTS))}")
        is_host = host_arrays(text, protos)
        L = C.CDLL(LIB_PATH)
        L.hg_last_error.restype = C.c_char_p
        from . import ops
        _ops = ops
        for name, (ret, params) in protos.items():
            getattr(L, name)             # fail loudly if a declared symbol is not exported
            fn = L[name]                 # a function object of its own: the argtypes below do not reach the raw handle's attributes
            fn.restype = C.c_char_p if ret == "const char*" else _INTS[ret]
            fn.argtypes = [_INTS.get(t) or _REALS.get(t) or (C.c_char_p if t == "const char*" else C.c_void_p) for t, _ in params]
            has_stream = bool(params) and params[-1] == ("void*", "stream")
            _bound[name] = (fn, [_converter(name, t, n, is_host(t, n)) for t, n in params[:len(params) - has_stream]], has_stream)
        _lib = L
    return _lib


def check(rc, what=""):
    if rc != 0:
        raise RuntimeError(f"{what}: libhamgnn_hip error {rc}: {lib().hg_last_error().decode()}")


def call(name, *args, stream=None):
    """run entry point `name` with every argument checked against the header's prototype: integers in range, reals, tensors of the pointee's dtype --
    contiguous or, wrapped as strided(t), with a unit last stride -- on the GPU (ops._require_gpu), None for NULL, host arrays where the header has them (an array of pointers
    also as the list of its tensors, each checked as a strided() one).
    The trailing `void* stream` is torch's current stream of the current device unless `stream` is given, and the status is checked.  The entry points
    without a stream (hg_version, hg_build_config, ...) return a value, not a status: it is handed back.  Only metadata is read: no sync, no allocation."""
    if _lib is None:
        lib()
    fn, convs, has_stream = _bound[name]
    if len(args) != len(convs):
        raise TypeError(f"{name} takes {len(convs)} arguments{' and the stream' if has_stream else ''}, got {len(args)}")
    argv = [c(a) for c, a in zip(convs, args)]
    if not has_stream:
        return fn(*argv)
    if stream is None and torch.cuda.is_initialized():        # (no tensor has reached a GPU before that: the NULL stream is the current one)
        stream = _raw_stream(_cur_device()) if _raw_stream and _cur_device else torch.cuda.current_stream().cuda_stream
    check(fn(*argv, stream), name)


def ptr(t):
    """device pointer of a (contiguous) torch tensor, or NULL -- for the raw handle (tests/bench_*.py); ops goes through `call`"""
    if t is None:
        return C.c_void_p(0)
    assert t.is_contiguous(), "non-contiguous tensor handed to the C ABI"
    return C.c_void_p(t.data_ptr())


def i64(v):
    return C.c_int64(int(v))


def i32(v):
    return C.c_int(int(v))


def f32(v):
    return C.c_float(float(v))
