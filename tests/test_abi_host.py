"""The C ABI of libtqdne_hip.so, stated once and held against its three hand-written statements: include/tqdne_hip.h, the ctypes
binding tqdne_amd/_lib.py (_PROTOS, the Structures, the TQ_* constants) and the stub printed in INTEGRATION.md.  A miscounted
argument list shows only when a kernel reads a shifted pointer on a device; here it shows without one.  Changing the surface means
editing SURFACE and ABI below."""

import ctypes
import functools
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ABI = 9
SURFACE = """
    tq_abi_version tq_adam_ema_step_clipped tq_adam_ema_step_guarded tq_attention_bwd_hd tq_attention_bwd_ws
    tq_attention_bwd_ws_kv tq_attention_fwd tq_attention_fwd_hd tq_attention_fwd_presplit tq_attention_hd_lds_bytes
    tq_attention_hd_workspace_bytes tq_attention_head_tile tq_attention_workspace_bytes tq_avg_pool2_bwd tq_avg_pool2_fwd
    tq_axpy_sigma tq_boundary_max_channels tq_btc_to_nct tq_classifier_head_bwd tq_classifier_head_bwd_workspace
    tq_classifier_head_fwd tq_classifier_head_max_channels tq_classifier_head_max_classes tq_cm_scalars tq_colsum
    tq_colsum_max_channels tq_concat_scale tq_conv1d_bwd_data tq_conv1d_bwd_weight tq_conv1d_bwd_weight_colsum
    tq_conv1d_bwd_weight_plan tq_conv1d_bwd_weight_workspace tq_conv1d_fwd tq_conv1d_fwd_qkv tq_conv1d_fwd_skip
    tq_conv1d_gn_fold_max_cin tq_conv1d_gn_table_entries tq_conv1d_max_cin tq_conv1d_max_cout tq_conv1d_wide_lds_bytes
    tq_conv_tile_co tq_conv_weight_pack_bytes tq_cross_entropy tq_ddpm_step tq_edm_loss tq_edm_noise_inject tq_edm_scalars
    tq_ema_swap tq_embed_fwd tq_envelope_fwd tq_envelope_inv tq_fourier_features tq_gemm_f32_jobs tq_gemm_tiles tq_gn_bwd_apply
    tq_gn_bwd_apply_colsum tq_gn_bwd_finalize tq_gn_finalize tq_grad_clip_coef tq_grad_sumsq tq_griffinlim
    tq_griffinlim_max_frames tq_head_conv_bwd_lds_bytes tq_head_conv_bwd_ws tq_head_conv_fwd tq_head_conv_lds_bytes
    tq_heun_churn tq_heun_correct tq_heun_euler tq_linear_fwd tq_mse_loss tq_nct_to_btc tq_nearest_up2_fwd
    tq_oscillator_table_floats tq_oscillator_tables tq_pack_conv_weight tq_pack_job_blocks tq_pack_jobs tq_pair_sum
    tq_pseudo_huber_loss tq_radam_ema_step_clipped tq_radam_ema_step_guarded tq_rotd_peaks tq_sampler_init tq_scale_add2
    tq_spectrogram_table_floats tq_spectrogram_tables tq_stem_conv_bwd_weight_ws tq_stem_conv_fwd tq_stem_conv_lds_bytes
    tq_stem_head_bwd_workspace tq_stft_fwd tq_upsample_poly_wgrad_fold tq_vae_reparam_bwd tq_vae_reparam_fwd tq_zero_stuff
""".split()
# TQ_* names of _lib.py that the header does not define (values derived in the binding alone): none.  TQ_AMAX_WORDS, a product of
# two others, is a #define of the header as well and is evaluated below like the rest.
LIB_ONLY_CONSTANTS = ()

_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
            "int64_t": ctypes.c_int64}


@functools.lru_cache(None)
def _built():
    """(binding module, loaded library, header text without comments)"""
    from tqdne_amd import _build, _lib
    _build.build(verbose=False)
    header = open(os.path.join(ROOT, "include", "tqdne_hip.h")).read()
    return _lib, _lib.load(), re.sub(r"/\*.*?\*/", "", header, flags=re.S)


@functools.lru_cache(None)
def _header_prototypes():
    """{name: (result type, [parameter text])} of every function the header declares"""
    protos = {}
    for res, name, params in re.findall(r"^(\w+)\s+(tq_\w+)\s*\((.*?)\)\s*;", _built()[2], re.S | re.M):
        assert name not in protos, name
        params = " ".join(params.split())
        protos[name] = (res, [] if params == "void" else [p.strip() for p in params.split(",")])
    return protos


def test_the_surface_is_the_list_in_the_header_the_binding_the_library_and_the_sources():
    _lib, lib, header = _built()
    assert SURFACE == sorted(set(SURFACE)) and len(SURFACE) == 96
    assert re.search(r"^#define TQ_ABI_VERSION %d$" % ABI, header, re.M) and _lib.ABI_VERSION == ABI and lib.tq_abi_version() == ABI
    assert set(_header_prototypes()) == set(SURFACE)
    assert set(_lib._PROTOS) == set(SURFACE) == set(_lib.exported_symbols())
    assert [n for n in SURFACE if not hasattr(lib, n)] == []
    defined = []
    for path in sorted(glob.glob(os.path.join(ROOT, "tqdne_amd", "csrc", "*"))):
        text = open(path).read()
        found = re.findall(r'extern "C"\s+(?:int|size_t)\s+(\w+)\s*\(', text)
        assert len(found) == text.count('extern "C"'), f"{path}: an extern \"C\" this scan does not read"
        defined += [n for n in found if not n.startswith("tq_debug_")]   # (the TQ_STAMP instrumentation, not built by default)
    assert sorted(set(defined)) == SURFACE


@pytest.mark.parametrize("name", SURFACE)
def test_binding_prototype_matches_the_header(name):
    """pointers and the stream travel as c_void_p (or a POINTER(struct)), scalars by their own C type"""
    _lib = _built()[0]
    h_res, h_params = _header_prototypes()[name]
    res, args = _lib._PROTOS[name]
    assert res is {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[h_res]
    assert len(args) == len(h_params), (len(args), h_params)
    for i, (p, a) in enumerate(zip(h_params, args)):
        if "*" in p or p.startswith("hipStream_t"):
            assert a is ctypes.c_void_p or issubclass(a, ctypes._Pointer), (i, p, a)
        else:
            assert a is _SCALARS[p.split()[0]], (i, p, a)


def test_binding_constants_match_the_header():
    _lib, _, header = _built()
    consts = {}
    for name, expr in re.findall(r"^#define\s+(TQ_\w+)[ \t]+(\S.*)$", header, re.M):
        consts[name] = eval(expr, {"__builtins__": {}}, dict(consts))
    assert len(consts) >= 30 and consts["TQ_ERR_ARG"] == -1 and consts["TQ_AMAX_WORDS"] == 512
    bound = {n: v for n, v in vars(_lib).items() if n.startswith("TQ_")}
    assert {"TQ_ERR_ARG", "TQ_ERR_SHAPE", "TQ_CONV_GN", "TQ_WFMT_F16_MX6", "TQ_ADAM_CHUNK", "TQ_WGRAD_H64"} <= set(bound)
    assert {n for n in bound if n not in consts} == set(LIB_ONLY_CONSTANTS)
    assert {n: v for n, v in bound.items() if n in consts and consts[n] != v} == {}


# The three statements of every C-ABI struct -- include/tqdne_hip.h, tqdne_amd/_lib.py (ctypes) and the maintainer's stub printed
# in INTEGRATION.md -- must describe the same bytes: a struct built from a stale stub is read past its end by the library.

_C_TYPES = {"int32_t": "c_int", "uint32_t": "c_uint", "float": "c_float", "uint64_t": "c_ulong", "int": "c_int",
            "unsigned long long": "c_ulong", "double": "c_double"}


def _header_struct_fields(name):
    """[(field, ctypes type)] of ``typedef struct <name> {...}`` in include/tqdne_hip.h (pointers -> c_void_p)"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _built()[2], re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.match(r"(?:const )?((?:unsigned long long|[A-Za-z_][A-Za-z0-9_]*))\s*(\*?)\s*(.*)$", decl)
        ctype, star, names = m.group(1), m.group(2), m.group(3)
        for n in names.split(","):
            n = n.strip()
            ptr = bool(star) or n.startswith("*")
            n = n.lstrip("* ")
            fields.append((n, ctypes.c_void_p if ptr else getattr(ctypes, _C_TYPES[ctype])))
    return fields


def _layout(struct):
    return [(n, getattr(struct, n).offset, getattr(struct, n).size) for n, *_ in struct._fields_], ctypes.sizeof(struct)


STRUCTS = ["TqConvDesc", "TqConvBwdDesc", "TqPackJob", "TqGnFold", "TqWgradPlan", "TqGemmJob", "TqAdamChunk"]


@pytest.mark.parametrize("name", STRUCTS)
def test_ctypes_structs_match_the_header(name):
    _lib, _, header = _built()
    assert sorted(re.findall(r"typedef struct (\w+) \{", header)) == sorted(STRUCTS)
    ref = type(name + "_h", (ctypes.Structure,), {"_fields_": _header_struct_fields(name)})
    assert _layout(getattr(_lib, name)) == _layout(ref)


def test_integration_md_stub_matches_the_header_and_the_binding():
    """INTEGRATION.md's ``class TqConvDesc(ctypes.Structure)`` (the stub a maintainer of the reference would copy) is executed as
    printed and held against the binding: same field names, offsets, sizes and total size."""
    _lib = _built()[0]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = re.findall(r"```python\n(.*?)```", doc, re.S)
    stub = next(b for b in blocks if "class TqConvDesc(ctypes.Structure)" in b)
    classes = re.findall(r"^(class (\w+)\(ctypes\.Structure\):.*?)(?=^\S)", stub, re.S | re.M)
    assert classes, "no ctypes.Structure in the stub"
    for src, name in classes:
        ns = {"ctypes": ctypes}
        exec(src, ns)
        assert _layout(ns[name]) == _layout(getattr(_lib, name)), name
    # the argument list the stub binds tq_conv1d_fwd with is the binding's
    n_ptr = int(re.search(r"tq_conv1d_fwd\.argtypes = \[ctypes\.POINTER\(TqConvDesc\)\] \+ \[ctypes\.c_void_p\] \* (\d+)", stub).group(1))
    assert n_ptr == len(_lib._PROTOS["tq_conv1d_fwd"][1]) - 1
