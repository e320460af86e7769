"""ctypes binding of libtqdne_duration.so (include/tqdne_duration.h): Arias energy, Husid curve, threshold crossings and numpy's
gradient.  Fails loudly like ``_lib``: a GPU tensor never falls back to the host -- if the library is missing the callers raise."""

from __future__ import annotations

import ctypes as C
import os

from . import _build
from ._lib import TQ_ERR_ARG, TQ_ERR_SHAPE, TqError

_LIB = None

VP = C.c_void_p
I = C.c_int
F = C.c_float
D = C.c_double
I64 = C.c_int64

ABI_VERSION = 1   # include/tqdne_duration.h TQD_ABI_VERSION
TQD_MAX_FRACTIONS = 8

_PROTOS = {
    "tqd_abi_version": (I, []),
    "tqd_max_fractions": (I, []),
    "tqd_arias": (I, [VP, VP, VP, VP, VP, VP, I, I, I64, I64, D, VP, I, VP]),
    "tqd_gradient": (I, [VP, VP, I, I, I64, I64, F, VP]),
}


def lib_path() -> str:
    return _build.DURATION_LIBPATH


def load():
    """Load the shared library (once).  Raises RuntimeError if it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: the duration measures of GPU tensors in tqdne_amd are HIP-only (no PyTorch fallback). "
            "Build it with `python -m tqdne_amd._build` (needs hipcc, cross-compiles gfx950 without a GPU)."
        )
    lib = C.CDLL(path)
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)  # AttributeError = header/library mismatch: loud
        fn.restype = res
        fn.argtypes = args
    if lib.tqd_abi_version() != ABI_VERSION:
        raise RuntimeError("libtqdne_duration.so ABI version mismatch")
    _LIB = lib
    return lib


def exported_symbols():
    return sorted(_PROTOS)


def check(rc: int, what: str = ""):
    if rc != 0:
        kind = {TQ_ERR_ARG: "TQ_ERR_ARG", TQ_ERR_SHAPE: "TQ_ERR_SHAPE"}.get(rc, f"hipError_t {rc}")
        raise TqError(f"libtqdne_duration: {what} failed with {kind}")
