"""CPU checks of lsqr_ransac_many_sequential's Python mirror: liblsqr_hip.so exports the symbol, the ctypes table gives
it the header's argument types, a null context is refused before anything is touched, and Context has the method with
the documented defaults."""
import ctypes as C
import inspect

import numpy as np

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd.context import Context


def test_symbol_exported_with_argtypes():
    lib = L.load()
    fn = lib.lsqr_ransac_many_sequential
    res, args = L.SIGNATURES["lsqr_ransac_many_sequential"]
    assert fn.restype is res is C.c_int
    assert list(fn.argtypes) == args and len(args) == 14
    # (ctx, records, stride, offsets, n_problems, p, seeds, max_models, min_votes, params, labels, infos, status,
    #  n_models)
    assert args[2] is C.c_size_t and args[4] is C.c_size_t and args[5] is C.c_double
    assert args[7] is C.c_size_t and args[8] is C.c_uint64
    assert all(args[i] is C.c_void_p for i in (1, 3, 6, 9, 10, 11, 12, 13))


def test_null_context_is_refused_before_anything_is_touched():
    lib = L.load()
    offs = np.array([0, 4, 8], dtype=np.uint64)
    recs = np.zeros((8, 3))
    seeds = np.arange(1, 5, dtype=np.uint64)
    n_models = np.full(2, 7, dtype=np.uintp)
    status = np.full(4, 42, dtype=np.int32)
    labels = np.full(8, 42, dtype=np.int32)
    params = np.full((4, 6), 42.0)
    infos = (L.RansacInfo * 4)()
    C.memset(infos, 0x5A, C.sizeof(infos))
    for m in (2, 0):
        assert lib.lsqr_ransac_many_sequential(None, L.ptr(recs), 24, L.ptr(offs), 2, 0.99, L.ptr(seeds), m, 0,
                                               L.ptr(params), L.ptr(labels), infos, L.ptr(status),
                                               L.ptr(n_models)) == L.ERR_INVALID
        assert np.all(n_models == 7) and np.all(status == 42) and np.all(labels == 42) and np.all(params == 42.0)
        assert bytes(infos) == b"\x5a" * C.sizeof(infos)


def test_context_method():
    sig = inspect.signature(Context.ransac_many_sequential)
    assert list(sig.parameters) == ["self", "problems", "p", "max_models", "seeds", "min_votes", "want_labels"]
    assert sig.parameters["seeds"].default is None and sig.parameters["min_votes"].default == 0
    assert sig.parameters["want_labels"].default is True
