"""Bindings of libubpl_hip.so (C-ABI declared in include/ubpl_hip.h).

Both bindings are derived from the header by its one parser, _abi.parse.
Compute entry points are called through their torch ops — libubpl_ops.so,
TORCH_LIBRARY(ubpl, m), generated at build time by _abi.gen: `ubpl::<name>`
per C entry, device pointers as tensors, enqueued on torch's current HIP
stream.  The host-only planning queries (workspace sizes, plan choices) and
the ABI checks of the CPU tests use ctypes on the C-ABI itself; load() builds
their signatures (SIGNATURES) from the same parse.

torch is imported first so that both libraries bind to the HIP runtime torch
already loaded (same SONAME, one runtime, one set of streams).  There is no
CPU fallback: a missing library or a missing GPU raises.
"""
import ctypes
import os

import torch

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# UBPL_LIB_DIR: another build of the same two libraries (same-box A/B of a kernel change)
_LIB_DIR = os.environ.get("UBPL_LIB_DIR") or _HERE
LIB_PATH = os.path.join(_LIB_DIR, "libubpl_hip.so")
OPS_PATH = os.path.join(_LIB_DIR, "libubpl_ops.so")

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "ubpl_hip.h")

_CTYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}

# name -> (restype, argtypes) of every entry include/ubpl_hip.h declares; filled by load()
SIGNATURES = {}

_lib = None


def signatures(header=HEADER_PATH):
    """name -> (restype, argtypes) of every entry the header declares: int, int64_t,
    float and double as their ctypes, any pointer as c_void_p."""
    if not os.path.exists(header):
        raise RuntimeError("ubpl_amd: %s not found — the bindings of libubpl_hip.so are derived from it" % header)
    return {name: (_CTYPES[ret], [ctypes.c_void_p if "*" in typ else _CTYPES[typ] for typ, _ in params])
            for ret, name, params, _ in _abi.parse(open(header).read())}


def load(path=LIB_PATH):
    """Load the library and bind every symbol the header declares (raises if any is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RuntimeError("ubpl_amd: %s not found — build it with `make -C ubpl-poseestimation_amd/csrc` "
                           "(or __graft_entry__.build()); there is no CPU fallback" % path)
    SIGNATURES.update(signatures())
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def lib():
    return _lib if _lib is not None else load()


def require_gpu(t=None):
    if not torch.cuda.is_available():
        raise RuntimeError("ubpl_amd: the HIP hot path needs an MI355X (gfx950) GPU; no CPU fallback")
    if t is not None and not t.is_cuda:
        raise RuntimeError("ubpl_amd: expected a device tensor, got %s" % t.device)


_ops = {}


def load_ops(path=OPS_PATH):
    """Register the ubpl torch ops (raises if the library is missing)."""
    if not _ops:
        lib()
        if not os.path.exists(path):
            raise RuntimeError("ubpl_amd: %s not found — build it with `make -C ubpl-poseestimation_amd/csrc` "
                               "(or __graft_entry__.build()); there is no CPU fallback" % path)
        torch.ops.load_library(path)
        _ops["loaded"] = True
    return torch.ops.ubpl


def op(name):
    """The torch op (OpOverload) of C-ABI entry `name`."""
    o = _ops.get(name)
    if o is None:
        o = _ops[name] = getattr(load_ops(), name[len("ubpl_"):]).default
    return o


def call(name, *args):
    """Enqueue C-ABI entry `name` through its torch op.  `args` follow the C
    signature (device pointers as tensors or None) without its trailing
    stream argument: the op enqueues on torch's current stream."""
    return op(name)(*args)
