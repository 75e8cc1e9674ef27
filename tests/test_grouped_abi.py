"""CPU checks of lsqr_ransac_grouped's Python mirror: liblsqr_hip.so exports the symbol, the ctypes table gives it the
header's argument list, a null context is refused before anything is touched, and Context has the method with the
documented defaults."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd.context import Context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPES = {"lsqr_ctx *": C.c_void_p, "const int32_t *": C.c_void_p, "size_t": C.c_size_t, "int": C.c_int,
          "double": C.c_double, "const uint64_t *": C.c_void_p, "double *": C.c_void_p, "uint8_t *": C.c_void_p,
          "uint64_t *": C.c_void_p, "lsqr_ransac_info *": C.c_void_p, "int32_t *": C.c_void_p}


def _header_args():
    """the declaration's argument types, comments stripped: [(type, name), ...]"""
    text = open(os.path.join(ROOT, "include", "lsqr_hip.h")).read()
    m = re.search(r"LSQR_API int lsqr_ransac_grouped\((.*?)\);", text, re.S)
    assert m, "include/lsqr_hip.h does not declare lsqr_ransac_grouped"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    out = []
    for a in args:
        t, name = re.match(r"(.*?)(\w+)$", a).groups()
        out.append((t.strip(), name))
    return out


def test_symbol_exported_with_the_headers_argument_list():
    lib = L.load()
    fn = lib.lsqr_ransac_grouped
    res, args = L.SIGNATURES["lsqr_ransac_grouped"]
    assert fn.restype is res is C.c_int
    assert list(fn.argtypes) == args
    decl = _header_args()
    assert [n for _, n in decl] == ["ctx", "groups", "n_groups", "on_device", "p", "seeds", "params_out",
                                    "consensus_out", "offsets_out", "infos", "status_out"]
    assert args == [CTYPES[t] for t, _ in decl]


def test_null_context_is_refused_before_anything_is_touched():
    lib = L.load()
    groups = np.zeros(8, dtype=np.int32)
    seeds = np.arange(1, 3, dtype=np.uint64)
    params = np.full((2, 6), 42.0)
    cons = np.full(8, 42, dtype=np.uint8)
    offs = np.full(3, 42, dtype=np.uint64)
    status = np.full(2, 42, dtype=np.int32)
    infos = (L.RansacInfo * 2)()
    C.memset(infos, 0x5A, C.sizeof(infos))
    for n in (2, 0):
        assert lib.lsqr_ransac_grouped(None, L.ptr(groups), n, 0, 0.99, L.ptr(seeds), L.ptr(params), L.ptr(cons),
                                       L.ptr(offs), infos, L.ptr(status)) == L.ERR_INVALID
        assert np.all(params == 42.0) and np.all(cons == 42) and np.all(offs == 42) and np.all(status == 42)
        assert bytes(infos) == b"\x5a" * C.sizeof(infos)


def test_context_method():
    sig = inspect.signature(Context.ransac_grouped)
    assert list(sig.parameters) == ["self", "groups", "n_groups", "p", "seeds", "want_consensus", "consensus_out"]
    assert sig.parameters["seeds"].default is None and sig.parameters["want_consensus"].default is True
    assert sig.parameters["consensus_out"].default is None
