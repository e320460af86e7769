"""ctypes binding of libtqdne_eval.so (include/tqdne_eval.h): the evaluation stage's spectra kernels.  Fails loudly like ``_lib``:
there is no host fallback behind these entry points -- if the library is missing the callers raise."""

from __future__ import annotations

import ctypes as C
import os

from . import _build
from ._lib import TQ_ERR_ARG, TQ_ERR_SHAPE, TqError

_LIB = None

VP = C.c_void_p
I = C.c_int
F = C.c_float
SZ = C.c_size_t

ABI_VERSION = 1   # include/tqdne_eval.h TQE_ABI_VERSION
TQE_RDFT_COMPLEX, TQE_RDFT_ABS, TQE_RDFT_LOG = 0, 1, 2
TQE_RDFT_MAX_LENGTH = 4096

_PROTOS = {
    "tqe_abi_version": (I, []),
    "tqe_rdft_max_length": (I, []),
    "tqe_rdft_table_floats": (SZ, [I]),
    "tqe_rdft_tables": (I, [I, VP]),
    "tqe_rdft": (I, [VP, VP, VP, I, I, C.c_int64, I, F, VP]),
    "tqe_spectral_filter": (I, [VP, VP, VP, VP, I, I, C.c_int64, VP]),
    "tqe_column_moments": (I, [VP, VP, VP, I, I, VP]),
}


def lib_path() -> str:
    return _build.EVAL_LIBPATH


def load():
    """Load the shared library (once).  Raises RuntimeError if it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: the spectra of tqdne_amd are HIP-only (no CPU / PyTorch fallback). "
            "Build it with `python -m tqdne_amd._build` (needs hipcc, cross-compiles gfx950 without a GPU)."
        )
    lib = C.CDLL(path)
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)  # AttributeError = header/library mismatch: loud
        fn.restype = res
        fn.argtypes = args
    if lib.tqe_abi_version() != ABI_VERSION:
        raise RuntimeError("libtqdne_eval.so ABI version mismatch")
    _LIB = lib
    return lib


def exported_symbols():
    return sorted(_PROTOS)


def check(rc: int, what: str = ""):
    if rc != 0:
        kind = {TQ_ERR_ARG: "TQ_ERR_ARG", TQ_ERR_SHAPE: "TQ_ERR_SHAPE"}.get(rc, f"hipError_t {rc}")
        raise TqError(f"libtqdne_eval: {what} failed with {kind}")
