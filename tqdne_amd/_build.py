"""Build libtqdne_hip.so (the model library), libtqdne_eval.so (the evaluation library, csrc_eval/) and libtqdne_series.so (the
conditioning library, csrc_series/) with hipcc, gfx950 only, in-tree under tqdne_amd/lib/.
libtqdne_duration.so (the Arias-intensity / duration library, csrc_duration/) is the fourth, built the same way."""

from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIBPATH = os.path.join(LIBDIR, "libtqdne_hip.so")
# (the conv kernel template, csrc/conv1d_kernel.hpp, is instantiated by seven translation units so that the build runs in parallel)
SOURCES = ["conv1d_fwd_k5a.hip", "conv1d_fwd_k5b.hip", "conv1d_fwd_k13.hip", "conv1d_resample.hip", "conv1d_dgrad.hip", "conv1d_mfma.hip",
           "conv1d_fwd_wide.hip", "conv1d_fwd_wide_k13.hip", "small_ops.hip", "attention.hip", "attention_hd.hip", "backward.hip", "ends_wide.hip", "boundary.hip",
           "resample_plain.hip", "classifier.hip", "spectrogram.hip", "intensity.hip"]
ARCH = "gfx950"
# the evaluation library (include/tqdne_eval.h): its own sources, its own staleness check, the model library's flags
CSRC_EVAL = os.path.join(HERE, "csrc_eval")
EVAL_LIBPATH = os.path.join(LIBDIR, "libtqdne_eval.so")
EVAL_SOURCES = ["spectra.hip"]
# the conditioning library (include/tqdne_series.h), built the same way
CSRC_SERIES = os.path.join(HERE, "csrc_series")
SERIES_LIBPATH = os.path.join(LIBDIR, "libtqdne_series.so")
SERIES_SOURCES = ["series.hip"]
# the duration library (include/tqdne_duration.h), built the same way
CSRC_DURATION = os.path.join(HERE, "csrc_duration")
DURATION_LIBPATH = os.path.join(LIBDIR, "libtqdne_duration.so")
DURATION_SOURCES = ["duration.hip"]


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def _deps():
    return [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(HERE, "..", "include", "tqdne_hip.h")]


def needs_build(path: str = None) -> bool:
    path = path or LIBPATH
    if not os.path.exists(path):
        return True
    t = os.path.getmtime(path)
    return any(os.path.getmtime(d) > t for d in _deps() if os.path.exists(d))


def _eval_deps():
    return [os.path.join(CSRC_EVAL, f) for f in os.listdir(CSRC_EVAL)] + [os.path.join(CSRC, "common.hpp"),
                                                                          os.path.join(HERE, "..", "include", "tqdne_eval.h")]


def eval_needs_build() -> bool:
    if not os.path.exists(EVAL_LIBPATH):
        return True
    t = os.path.getmtime(EVAL_LIBPATH)
    return any(os.path.getmtime(d) > t for d in _eval_deps() if os.path.exists(d))


def _series_deps():
    return [os.path.join(CSRC_SERIES, f) for f in os.listdir(CSRC_SERIES)] + [os.path.join(CSRC, "common.hpp"),
                                                                              os.path.join(HERE, "..", "include", "tqdne_series.h")]


def series_needs_build() -> bool:
    if not os.path.exists(SERIES_LIBPATH):
        return True
    t = os.path.getmtime(SERIES_LIBPATH)
    return any(os.path.getmtime(d) > t for d in _series_deps() if os.path.exists(d))


def _duration_deps():
    return [os.path.join(CSRC_DURATION, f) for f in os.listdir(CSRC_DURATION)] + [os.path.join(CSRC, "common.hpp"),
                                                                                  os.path.join(HERE, "..", "include", "tqdne_duration.h")]


def duration_needs_build() -> bool:
    if not os.path.exists(DURATION_LIBPATH):
        return True
    t = os.path.getmtime(DURATION_LIBPATH)
    return any(os.path.getmtime(d) > t for d in _duration_deps() if os.path.exists(d))


def build(force: bool = False, verbose: bool = True, extra_flags=(), out_name=None) -> str:
    """Compile every HIP source for gfx950 and link the C-ABI shared libraries; returns the model library's path.  ``out_name``: an
    A/B build of the model library alone under that name."""
    if out_name is None and (force or eval_needs_build()):
        _compile_and_link(CSRC_EVAL, EVAL_SOURCES, EVAL_LIBPATH, "", verbose, extra_flags)
    if out_name is None and (force or series_needs_build()):
        _compile_and_link(CSRC_SERIES, SERIES_SOURCES, SERIES_LIBPATH, "", verbose, extra_flags)
    if out_name is None and (force or duration_needs_build()):
        _compile_and_link(CSRC_DURATION, DURATION_SOURCES, DURATION_LIBPATH, "", verbose, extra_flags)
    global_out = LIBPATH if out_name is None else os.path.join(LIBDIR, out_name)
    if out_name is None and not force and not needs_build(global_out):
        return global_out
    tag = "" if out_name is None else "." + out_name.replace(".so", "")
    return _compile_and_link(CSRC, SOURCES, global_out, tag, verbose, extra_flags)


def _compile_and_link(csrc, sources, global_out, tag, verbose, extra_flags) -> str:
    os.makedirs(LIBDIR, exist_ok=True)
    objs = []
    procs = []
    for src in sources:
        path = os.path.join(csrc, src)
        if not os.path.exists(path):
            continue
        obj = os.path.join(LIBDIR, src.replace(".hip", tag + ".o"))
        cmd = [_hipcc(), f"--offload-arch={ARCH}", "-O3", "-fPIC", "-std=c++17", "-Wno-unused-value", "-Wno-ignored-attributes", "-Wno-cuda-compat", *extra_flags,
               "-c", path, "-o", obj]
        if verbose:
            print("[tqdne_amd build]", " ".join(cmd), flush=True)
        procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        objs.append(obj)
    for cmd, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), out))
        if verbose and out.strip():
            print(out)
    cmd = [_hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", global_out] + objs
    if verbose:
        print("[tqdne_amd build]", " ".join(cmd), flush=True)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("link failed:\n" + r.stdout)
    return global_out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
