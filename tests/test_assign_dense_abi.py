"""CPU checks of lsqr_assign_dense_host / lsqr_assign_dense / lsqr_refine_dense and their Python mirror: the symbols
have the header's argument lists, the host call's argument errors write nothing, its agree bit is the oracle's dense
agree and its label the argmin of its own residuals with the smallest-m tie rule, and Context has the two methods."""
import ctypes as C
import inspect

import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd.context import Context
from oracle import pyoracle as O
from test_assign_abi import CTYPES, _header_args, _same_ctype

NAMES = {
    "lsqr_assign_dense_host": ["cfg", "params", "n_models", "record", "label_out", "residual_out"],
    "lsqr_assign_dense": ["ctx", "params", "n_models", "on_device", "labels_out", "residuals_out", "counts_out"],
    "lsqr_refine_dense": ["ctx", "params_inout", "n_models", "max_rounds", "on_device", "labels_out", "counts_out",
                          "fits", "status_out", "rounds_out", "converged_out"],
}


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
    params = np.full((3, 8), 42.0)
    labels = np.full(8, 42, dtype=np.int32)
    res = np.full(8, 42.0)
    counts = np.full(4, 42, dtype=np.uint64)
    status = np.full(3, 42, dtype=np.int32)
    fits = (L.FitInfo * 3)()
    C.memset(fits, 0x5A, C.sizeof(fits))
    rounds, conv = C.c_size_t(42), C.c_int(42)
    for n in (3, 0, 65):
        assert lib.lsqr_assign_dense(None, L.ptr(params), n, 0, L.ptr(labels), L.ptr(res),
                                     L.ptr(counts)) == L.ERR_INVALID
        assert lib.lsqr_refine_dense(None, L.ptr(params), n, 4, 0, L.ptr(labels), L.ptr(counts), fits, L.ptr(status),
                                     C.byref(rounds), C.byref(conv)) == L.ERR_INVALID
        assert np.all(params == 42.0) and np.all(labels == 42) and np.all(res == 42.0) and np.all(counts == 42)
        assert np.all(status == 42) and bytes(fits) == b"\x5a" * C.sizeof(fits)
        assert rounds.value == 42 and conv.value == 42


def _host(cfg, params, rec, n=None):
    """-> (status, label, residual) of lsqr_assign_dense_host"""
    label, res = C.c_int32(42), C.c_double(42.0)
    params = np.ascontiguousarray(params, dtype=np.float64)
    rec = np.ascontiguousarray(rec, dtype=np.float64)
    st = L.load().lsqr_assign_dense_host(C.byref(cfg), L.ptr(params), len(params) if n is None else n, L.ptr(rec),
                                         C.byref(label), C.byref(res))
    return st, label.value, res.value


def test_host_call_argument_checks():
    lib = L.load()
    cfg = L.ModelCfg(L.DENSE, 3, 0.5, 0, 0, 0.0)
    params = np.tile(np.array([1.0, 0.0, 0.0]), (65, 1))
    rec = np.array([2.25, 1.0, 1.0, 2.0])  # a . x - b = 0.25
    label, res = C.c_int32(42), C.c_double(42.0)

    def call(cfg_=cfg, params_=params, n=2, rec_=rec, label_=C.byref(label), res_=C.byref(res)):
        return lib.lsqr_assign_dense_host(C.byref(cfg_) if cfg_ is not None else None, L.ptr(params_), n, L.ptr(rec_),
                                          label_, res_)

    def untouched():
        return label.value == 42 and res.value == 42.0

    assert call(n=0) == L.OK and untouched()                      # nothing to assign to: a no-op
    assert call(n=65) == L.ERR_INVALID and untouched()
    assert call(cfg_=None) == L.ERR_INVALID and untouched()
    assert call(params_=None) == L.ERR_INVALID and untouched()
    assert call(rec_=None) == L.ERR_INVALID and untouched()
    assert call(label_=None) == L.ERR_INVALID and untouched()
    for model, dim in ((L.PLANE, 3), (L.LINE, 3), (L.SPHERE, 3), (L.LINE2D, 2), (L.ABSOR, 3), (L.PIVOT, 3), (L.RAY, 3),
                       (L.US_SINGLE, 0), (L.US_POINTER, 0), (L.PHANTOM, 0), (L.DENSE, 0), (L.DENSE, 65)):
        assert call(cfg_=L.ModelCfg(model, dim, 0.5, 0, 0, 0.0)) == L.ERR_INVALID and untouched(), (model, dim)
    # the residual is optional; 64 models are accepted
    assert call(res_=None) == L.OK and label.value == 0 and res.value == 42.0
    assert call(n=64) == L.OK and label.value == 0 and res.value == 0.25
    # lsqr_assign_host still refuses the dense model
    label.value, res.value = 42, 42.0
    assert lib.lsqr_assign_host(C.byref(cfg), L.ptr(params), 2, L.ptr(rec), C.byref(label),
                                C.byref(res)) == L.ERR_INVALID and untouched()


@pytest.mark.parametrize("n", [1, 3, 8, 9, 17, 64])
def test_host_decisions(n):
    rng = np.random.default_rng(100 + n)
    M, N, delta = 5, 200, 0.4
    params = rng.normal(size=(M, n))
    rows = np.empty((N, n + 1))
    rows[:, :n] = rng.normal(size=(N, n))
    owner = rng.integers(0, M, size=N)
    # near one regression, sometimes near two, sometimes near none
    rows[:, n] = np.einsum("ij,ij->i", rows[:, :n], params[owner]) + rng.normal(scale=0.3, size=N)
    cfg = L.ModelCfg(L.DENSE, n, delta, 0, 0, 0.0)
    ocfg = O.cfg(O.DENSE, n, delta)
    agree = np.stack([O.scan(ocfg, params[m], rows)[1] for m in range(M)], axis=1).astype(bool)  # the oracle's
    assert 0 < agree.sum() < agree.size and (agree.sum(axis=1) > 1).any() and (~agree.any(axis=1)).any()
    for i in range(N):
        res = np.empty(M)
        for m in range(M):  # the host residual of one regression alone: finite exactly where it agrees
            st, lab, res[m] = _host(cfg, params[m:m + 1], rows[i])
            assert st == L.OK and (lab == 0) == bool(agree[i, m]) == np.isfinite(res[m]), (i, m)
            if agree[i, m]:
                assert res[m] < delta
        st, lab, r = _host(cfg, params, rows[i])
        assert st == L.OK
        if agree[i].any():
            assert lab == int(np.argmin(res)) and r == res.min()  # argmin: the first minimum, the smallest m
        else:
            assert lab == -1 and r == np.inf


def test_host_tie_goes_to_the_smaller_model_and_delta_is_strict():
    n = 4
    cfg = L.ModelCfg(L.DENSE, n, 0.5, 0, 0, 0.0)
    x = np.array([1.0, -2.0, 0.5, 3.0])
    params = np.stack([x + 1.0, x, x, x + 1.0])
    rec = np.array([1.0, 1.0, 2.0, 1.0, 0.0])
    rec[n] = rec[:n] @ x - 0.125
    st, lab, r = _host(cfg, params, rec)
    assert (st, lab, r) == (L.OK, 1, 0.125)  # rows 1 and 2 are identical: the smaller m
    # residual == delta exactly: no agreement (strict '<'); one ulp inside: agreement
    a = np.array([1.0, 0.0, 0.0, 0.0, -0.5])  # a . 0 - b = 0.5
    assert _host(cfg, np.zeros((1, n)), a) == (L.OK, -1, np.inf)
    a[n] = -np.nextafter(0.5, 0.0)
    assert _host(cfg, np.zeros((1, n)), a) == (L.OK, 0, np.nextafter(0.5, 0.0))


@pytest.mark.parametrize("n", [1, 3, 9, 64])
def test_host_non_finite_slot_gives_minus_one(n):
    cfg = L.ModelCfg(L.DENSE, n, 0.5, 0, 0, 0.0)
    params = np.zeros((2, n))  # agrees with every finite row whose |b| < 0.5, whatever a holds
    rec = np.zeros(n + 1)
    assert _host(cfg, params, rec) == (L.OK, 0, 0.0)
    for bad in (np.nan, np.inf, -np.inf):
        for slot in range(n + 1):  # b included
            r = rec.copy()
            r[slot] = bad
            assert _host(cfg, params, r) == (L.OK, -1, np.inf), (bad, slot)


def test_context_methods():
    sig = inspect.signature(Context.assign_dense)
    assert list(sig.parameters) == ["self", "params", "want_residuals", "labels_out"]
    par = sig.parameters
    assert par["params"].default is inspect.Parameter.empty
    assert par["want_residuals"].default is False and par["labels_out"].default is None
    sig = inspect.signature(Context.refine_dense)
    assert list(sig.parameters) == ["self", "params", "max_rounds", "labels_out"]
    par = sig.parameters
    assert par["params"].default is inspect.Parameter.empty
    assert par["max_rounds"].default == 8 and par["labels_out"].default is None
    assert L.assign_dense_chunk(32) == 256 and L.assign_dense_chunk(33) == 128
