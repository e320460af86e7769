"""ctypes binding of libtqdne_series.so (include/tqdne_series.h): the conditioning kernels (causal IIR cascade, detrend, adaptive
envelope).  Fails loudly like ``_lib``: a GPU tensor never falls back to the host -- if the library is missing the callers raise."""

from __future__ import annotations

import ctypes as C
import os

from . import _build
from ._lib import TQ_ERR_ARG, TQ_ERR_SHAPE, TqError

_LIB = None

VP = C.c_void_p
I = C.c_int
F = C.c_float
I64 = C.c_int64

ABI_VERSION = 1   # include/tqdne_series.h TQS_ABI_VERSION
TQS_DETREND_NONE, TQS_DETREND_DEMEAN, TQS_DETREND_LINEAR = 0, 1, 2
TQS_SOSFILT_MAX_SECTIONS = 8

_PROTOS = {
    "tqs_abi_version": (I, []),
    "tqs_sosfilt_max_sections": (I, []),
    "tqs_sosfilt": (I, [VP, VP, VP, I, I, I64, I64, I, I, VP]),
    "tqs_hold_envelope": (I, [VP, VP, I, I, I64, I64, I, F, F, VP]),
}


def lib_path() -> str:
    return _build.SERIES_LIBPATH


def load():
    """Load the shared library (once).  Raises RuntimeError if it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: the conditioning of GPU tensors in tqdne_amd is HIP-only (no PyTorch fallback). "
            "Build it with `python -m tqdne_amd._build` (needs hipcc, cross-compiles gfx950 without a GPU)."
        )
    lib = C.CDLL(path)
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)  # AttributeError = header/library mismatch: loud
        fn.restype = res
        fn.argtypes = args
    if lib.tqs_abi_version() != ABI_VERSION:
        raise RuntimeError("libtqdne_series.so ABI version mismatch")
    _LIB = lib
    return lib


def exported_symbols():
    return sorted(_PROTOS)


def check(rc: int, what: str = ""):
    if rc != 0:
        kind = {TQ_ERR_ARG: "TQ_ERR_ARG", TQ_ERR_SHAPE: "TQ_ERR_SHAPE"}.get(rc, f"hipError_t {rc}")
        raise TqError(f"libtqdne_series: {what} failed with {kind}")
