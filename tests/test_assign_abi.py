"""CPU checks of lsqr_assign_host / lsqr_assign / lsqr_refine and their Python mirror: liblsqr_hip.so exports the
symbols, the ctypes table gives them the header's argument lists, a null context and the host call's argument errors
are refused before anything is touched, and Context has the two methods with the documented parameters and defaults."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd.context import Context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPES = {"lsqr_ctx *": C.c_void_p, "const lsqr_model_cfg *": C.POINTER(L.ModelCfg), "const double *": C.c_void_p,
          "const void *": C.c_void_p, "size_t": C.c_size_t, "int": C.c_int, "double *": C.c_void_p,
          "uint64_t *": C.c_void_p, "lsqr_fit_info *": C.c_void_p, "int32_t *": C.c_void_p,
          "size_t *": C.POINTER(C.c_size_t), "int *": C.POINTER(C.c_int)}
NAMES = {
    "lsqr_assign_host": ["cfg", "params", "n_models", "record", "label_out", "residual_out"],
    "lsqr_assign": ["ctx", "params", "n_models", "on_device", "labels_out", "residuals_out", "counts_out"],
    "lsqr_refine": ["ctx", "params_inout", "n_models", "max_rounds", "on_device", "labels_out", "counts_out", "fits",
                    "status_out", "rounds_out", "converged_out"],
}


def _header_args(fn):
    """the declaration's argument types, comments stripped: [(type, name), ...]"""
    text = open(os.path.join(ROOT, "include", "lsqr_hip.h")).read()
    m = re.search(r"LSQR_API int %s\((.*?)\);" % fn, text, re.S)
    assert m, "include/lsqr_hip.h does not declare %s" % fn
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    out = []
    for a in args:
        t, name = re.match(r"(.*?)(\w+)$", a).groups()
        out.append((t.strip(), name))
    return out


def _same_ctype(a, b):
    # (the host call's label_out / residual_out are typed pointers in the table: same size and kind as the header's)
    return a is b or (C.sizeof(a) == C.sizeof(b) == C.sizeof(C.c_void_p))


@pytest.mark.parametrize("fn", sorted(NAMES))
def test_symbol_exported_with_the_headers_argument_list(fn):
    lib = L.load()
    f = getattr(lib, fn)
    res, args = L.SIGNATURES[fn]
    assert f.restype is res is C.c_int
    assert list(f.argtypes) == args
    decl = _header_args(fn)
    assert [n for _, n in decl] == NAMES[fn]
    assert len(args) == len(decl)
    for a, (t, name) in zip(args, decl):
        assert _same_ctype(a, CTYPES[t]), (fn, name, t, a)
        if t in ("size_t", "int"):
            assert a is CTYPES[t], (fn, name)


def test_null_context_is_refused_before_anything_is_touched():
    lib = L.load()
    params = np.full((3, 6), 42.0)
    labels = np.full(8, 42, dtype=np.int32)
    res = np.full(8, 42.0)
    counts = np.full(4, 42, dtype=np.uint64)
    status = np.full(3, 42, dtype=np.int32)
    fits = (L.FitInfo * 3)()
    C.memset(fits, 0x5A, C.sizeof(fits))
    rounds, conv = C.c_size_t(42), C.c_int(42)
    for n in (3, 0, 65):
        assert lib.lsqr_assign(None, L.ptr(params), n, 0, L.ptr(labels), L.ptr(res), L.ptr(counts)) == L.ERR_INVALID
        assert lib.lsqr_refine(None, L.ptr(params), n, 4, 0, L.ptr(labels), L.ptr(counts), fits, L.ptr(status),
                               C.byref(rounds), C.byref(conv)) == L.ERR_INVALID
        assert np.all(params == 42.0) and np.all(labels == 42) and np.all(res == 42.0) and np.all(counts == 42)
        assert np.all(status == 42) and bytes(fits) == b"\x5a" * C.sizeof(fits)
        assert rounds.value == 42 and conv.value == 42


def test_host_call_argument_checks():
    lib = L.load()
    cfg = L.ModelCfg(L.PLANE, 3, 0.5, L.LS_ALGEBRAIC, 0, 0.0)
    params = np.tile(np.array([0.0, 0.0, 1.0, 0.0, 0.0, 0.0]), (65, 1))
    rec = np.array([1.0, 2.0, 0.25])
    label, res = C.c_int32(42), C.c_double(42.0)

    def call(cfg_=cfg, params_=params, n=2, rec_=rec, label_=C.byref(label), res_=C.byref(res)):
        return lib.lsqr_assign_host(C.byref(cfg_) if cfg_ is not None else None, L.ptr(params_), n, L.ptr(rec_), label_,
                                    res_)

    def untouched():
        return label.value == 42 and res.value == 42.0

    assert call(n=0) == L.OK and untouched()                      # nothing to assign to: a no-op
    assert call(n=65) == L.ERR_INVALID and untouched()
    assert call(cfg_=None) == L.ERR_INVALID and untouched()
    assert call(params_=None) == L.ERR_INVALID and untouched()
    assert call(rec_=None) == L.ERR_INVALID and untouched()
    assert call(label_=None) == L.ERR_INVALID and untouched()
    for model, dim in ((L.DENSE, 8), (L.ABSOR, 3), (L.PIVOT, 3), (L.RAY, 3), (L.US_SINGLE, 0), (L.PHANTOM, 0),
                       (L.PLANE, 9), (L.PLANE, 1)):
        assert call(cfg_=L.ModelCfg(model, dim, 0.5, 0, 0, 0.0)) == L.ERR_INVALID and untouched(), (model, dim)
    # the residual is optional; 64 models are accepted
    assert call(res_=None) == L.OK and label.value == 0 and res.value == 42.0
    assert call(n=64) == L.OK and label.value == 0 and res.value == 0.25
    # the 2-D line's parameters carry a point: it has the call
    line2d = L.ModelCfg(L.LINE2D, 2, 0.5, 0, 0, 0.0)
    assert call(cfg_=line2d, params_=np.array([[0.0, 1.0, 5.0, 1.0]]), n=1, rec_=np.array([3.0, 1.125])) == L.OK
    assert label.value == 0 and res.value == 0.125


def test_context_methods():
    sig = inspect.signature(Context.assign)
    assert list(sig.parameters) == ["self", "params", "want_residuals", "labels_out"]
    par = sig.parameters
    assert par["params"].default is inspect.Parameter.empty
    assert par["want_residuals"].default is False and par["labels_out"].default is None
    sig = inspect.signature(Context.refine)
    assert list(sig.parameters) == ["self", "params", "max_rounds", "labels_out"]
    par = sig.parameters
    assert par["params"].default is inspect.Parameter.empty
    assert par["max_rounds"].default == 8 and par["labels_out"].default is None
    assert L.OK == 0 and L.EMPTY == 1 and L.ERR_INVALID == 2 and L.ERR_STATE == 5
