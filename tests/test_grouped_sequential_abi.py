"""CPU checks of lsqr_ransac_grouped_sequential's Python mirror: liblsqr_hip.so exports the symbol, the ctypes table
gives it the header's argument list, a null context is refused before anything is touched, and Context has the method
with the documented parameters and defaults."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd.context import Context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPES = {"lsqr_ctx *": C.c_void_p, "const int32_t *": C.c_void_p, "size_t": C.c_size_t, "int": C.c_int,
          "double": C.c_double, "const uint64_t *": C.c_void_p, "uint64_t": C.c_uint64, "double *": C.c_void_p,
          "uint64_t *": C.c_void_p, "lsqr_ransac_info *": C.c_void_p, "int32_t *": C.c_void_p,
          "size_t *": C.c_void_p}


def _header_args():
    """the declaration's argument types, comments stripped: [(type, name), ...]"""
    text = open(os.path.join(ROOT, "include", "lsqr_hip.h")).read()
    m = re.search(r"LSQR_API int lsqr_ransac_grouped_sequential\((.*?)\);", text, re.S)
    assert m, "include/lsqr_hip.h does not declare lsqr_ransac_grouped_sequential"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    out = []
    for a in args:
        t, name = re.match(r"(.*?)(\w+)$", a).groups()
        out.append((t.strip(), name))
    return out


def test_symbol_exported_with_the_headers_argument_list():
    lib = L.load()
    fn = lib.lsqr_ransac_grouped_sequential
    res, args = L.SIGNATURES["lsqr_ransac_grouped_sequential"]
    assert fn.restype is res is C.c_int
    assert list(fn.argtypes) == args
    decl = _header_args()
    assert [n for _, n in decl] == ["ctx", "groups", "n_groups", "on_device", "p", "seeds", "max_models", "min_votes",
                                    "params_out", "labels_out", "offsets_out", "infos", "status_out", "n_models_out"]
    assert args == [CTYPES[t] for t, _ in decl]


def test_null_context_is_refused_before_anything_is_touched():
    lib = L.load()
    groups = np.zeros(8, dtype=np.int32)
    seeds = np.arange(1, 7, dtype=np.uint64)
    params = np.full((6, 6), 42.0)
    labels = np.full(8, 42, dtype=np.int32)
    offs = np.full(3, 42, dtype=np.uint64)
    status = np.full(6, 42, dtype=np.int32)
    n_models = np.full(2, 42, dtype=np.uintp)
    infos = (L.RansacInfo * 6)()
    C.memset(infos, 0x5A, C.sizeof(infos))
    for n in (2, 0):
        assert lib.lsqr_ransac_grouped_sequential(None, L.ptr(groups), n, 0, 0.99, L.ptr(seeds), 3, 0, L.ptr(params),
                                                  L.ptr(labels), L.ptr(offs), infos, L.ptr(status),
                                                  L.ptr(n_models)) == L.ERR_INVALID
        assert np.all(params == 42.0) and np.all(labels == 42) and np.all(offs == 42) and np.all(status == 42)
        assert np.all(n_models == 42) and bytes(infos) == b"\x5a" * C.sizeof(infos)


def test_context_method():
    sig = inspect.signature(Context.ransac_grouped_sequential)
    assert list(sig.parameters) == ["self", "groups", "n_groups", "p", "max_models", "seeds", "min_votes",
                                    "want_labels", "labels_out"]
    par = sig.parameters
    assert par["seeds"].default is None and par["min_votes"].default == 0 and par["want_labels"].default is True
    assert par["labels_out"].default is None
    for name in ("groups", "n_groups", "p", "max_models"):
        assert par[name].default is inspect.Parameter.empty, name
