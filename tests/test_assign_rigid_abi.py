"""CPU checks of lsqr_assign_rigid_host / lsqr_assign_rigid / lsqr_refine_rigid and their Python mirror: liblsqr_hip.so
exports the symbols, the ctypes table gives them the header's argument lists, a null context and the host call's
argument errors are refused before anything is touched, the host call decides hand-computed records of the three models
as the header says, and Context has the two methods with the documented parameters and defaults."""
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
    "lsqr_assign_rigid_host": ["cfg", "params", "n_models", "record", "label_out", "residual_out"],
    "lsqr_assign_rigid": ["ctx", "params", "n_models", "on_device", "labels_out", "residuals_out", "counts_out"],
    "lsqr_refine_rigid": ["ctx", "params_inout", "n_models", "max_rounds", "on_device", "labels_out", "counts_out",
                          "fits", "status_out", "rounds_out", "converged_out"],
}
IDENTITY = [1.0, 0.0, 0.0, 0.0]  # quaternion [s, qx, qy, qz]


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
        assert a is CTYPES[t] or C.sizeof(a) == C.sizeof(CTYPES[t]) == C.sizeof(C.c_void_p), (fn, name, t, a)
        if t in ("size_t", "int"):
            assert a is CTYPES[t], (fn, name)


def test_the_rigid_pair_has_the_argument_lists_of_assign_and_refine():
    assert L.SIGNATURES["lsqr_assign_rigid"] == L.SIGNATURES["lsqr_assign"]
    assert L.SIGNATURES["lsqr_refine_rigid"] == L.SIGNATURES["lsqr_refine"]
    assert L.SIGNATURES["lsqr_assign_rigid_host"] == L.SIGNATURES["lsqr_assign_host"]


def test_null_context_is_refused_before_anything_is_touched():
    lib = L.load()
    params = np.full((3, 7), 42.0)
    labels = np.full(8, 42, dtype=np.int32)
    res = np.full(8, 42.0)
    counts = np.full(4, 42, dtype=np.uint64)
    status = np.full(3, 42, dtype=np.int32)
    fits = (L.FitInfo * 3)()
    C.memset(fits, 0x5A, C.sizeof(fits))
    rounds, conv = C.c_size_t(42), C.c_int(42)
    for n in (3, 0, 65):
        assert lib.lsqr_assign_rigid(None, L.ptr(params), n, 0, L.ptr(labels), L.ptr(res),
                                     L.ptr(counts)) == L.ERR_INVALID
        assert lib.lsqr_refine_rigid(None, L.ptr(params), n, 4, 0, L.ptr(labels), L.ptr(counts), fits, L.ptr(status),
                                     C.byref(rounds), C.byref(conv)) == L.ERR_INVALID
        assert np.all(params == 42.0) and np.all(labels == 42) and np.all(res == 42.0) and np.all(counts == 42)
        assert np.all(status == 42) and bytes(fits) == b"\x5a" * C.sizeof(fits)
        assert rounds.value == 42 and conv.value == 42


def _host(cfg, params, rec, n=None, want_res=True):
    """-> (status, label, residual) of lsqr_assign_rigid_host; label and residual start at 42"""
    params = np.ascontiguousarray(params, dtype=np.float64)
    rec = np.ascontiguousarray(rec, dtype=np.float64)
    label, res = C.c_int32(42), C.c_double(42.0)
    st = L.load().lsqr_assign_rigid_host(C.byref(cfg), L.ptr(params), len(params) if n is None else n, L.ptr(rec),
                                         C.byref(label), C.byref(res) if want_res else None)
    return st, label.value, res.value


def test_host_call_argument_checks():
    lib = L.load()
    cfg = L.ModelCfg(L.RAY, 3, 0.5, 0, 0, 0.0)
    params = np.tile(np.array([0.0, 0.0, 0.0]), (65, 1))
    rec = np.array([0.0, 0.125, -2.0, 0.0, 0.0, 1.0])  # the line x = 0, y = 0.125: it passes the origin at 0.125
    label, res = C.c_int32(42), C.c_double(42.0)

    def call(cfg_=cfg, params_=params, n=2, rec_=rec, label_=C.byref(label), res_=C.byref(res)):
        return lib.lsqr_assign_rigid_host(C.byref(cfg_) if cfg_ is not None else None, L.ptr(params_), n, L.ptr(rec_),
                                          label_, res_)

    def untouched():
        return label.value == 42 and res.value == 42.0

    assert call(n=0) == L.OK and untouched()                      # nothing to assign to: a no-op
    assert call(n=65) == L.ERR_INVALID and untouched()
    assert call(cfg_=None) == L.ERR_INVALID and untouched()
    assert call(params_=None) == L.ERR_INVALID and untouched()
    assert call(rec_=None) == L.ERR_INVALID and untouched()
    assert call(label_=None) == L.ERR_INVALID and untouched()
    for model, dim in ((L.PLANE, 3), (L.LINE, 3), (L.SPHERE, 3), (L.LINE2D, 2), (L.DENSE, 8), (L.US_SINGLE, 0),
                       (L.US_POINTER, 0), (L.PHANTOM, 0)):
        assert call(cfg_=L.ModelCfg(model, dim, 0.5, 0, 0, 0.0)) == L.ERR_INVALID and untouched(), (model, dim)
    assert call(cfg_=L.ModelCfg(L.ABSOR, 3, 0.5, 1, 0, 0.0)) == L.ERR_INVALID and untouched()  # ls_type 0 or 2 only
    # the residual is optional; 64 models are accepted
    assert call(res_=None) == L.OK and label.value == 0 and res.value == 42.0
    assert call(n=64) == L.OK and label.value == 0 and res.value == 0.125


def test_host_call_absolute_orientation_by_hand():
    cfg = L.ModelCfg(L.ABSOR, 3, 0.5, 0, 0, 0.0)
    ident = IDENTITY + [0.0, 0.0, 0.0]
    shifted = IDENTITY + [0.0, 0.0, 0.25]           # the identity rotation, then 0.25 along z
    pair = [1.0, 2.0, 3.0, 1.0, 2.0, 3.125]         # second = first + 0.125 z
    assert _host(cfg, [ident], pair) == (L.OK, 0, 0.125)
    assert _host(cfg, [shifted], pair) == (L.OK, 0, 0.125)
    assert _host(cfg, [ident, shifted], pair) == (L.OK, 0, 0.125)      # a tie: the smaller index
    assert _host(cfg, [shifted, ident], pair) == (L.OK, 0, 0.125)
    near = IDENTITY + [0.0, 0.0, 0.0625]
    assert _host(cfg, [ident, near], pair) == (L.OK, 1, 0.0625)        # the nearest, not the first
    assert _host(cfg, [ident, near], pair, want_res=False) == (L.OK, 1, 42.0)
    far = [1.0, 2.0, 3.0, 1.0, 2.0, 3.5]                               # 0.5 is not < delta
    assert _host(cfg, [ident], far) == (L.OK, -1, np.inf)
    # a quarter turn about z: (1, 0, 0) -> (0, 1, 0)
    h = np.sqrt(0.5)
    turn = [h, 0.0, 0.0, h, 10.0, 20.0, 30.0]
    st, label, res = _host(cfg, [ident, turn], [1.0, 0.0, 0.0, 10.0, 21.0, 30.0])
    assert (st, label) == (L.OK, 1) and res < 1e-13  # (a few ulps of the coordinates, which reach 30)
    # a NaN slot: -1 and +inf, whichever slot
    for k in range(6):
        bad = list(pair)
        bad[k] = np.nan
        assert _host(cfg, [ident], bad) == (L.OK, -1, np.inf), k
    bad = list(pair)
    bad[4] = np.inf
    assert _host(cfg, [ident], bad) == (L.OK, -1, np.inf)


def test_host_call_weight_slot_counts_only_with_ls_type_2():
    ident = IDENTITY + [0.0, 0.0, 0.0]
    pair = [1.0, 2.0, 3.0, 1.0, 2.0, 3.125]
    plain, weighted = L.ModelCfg(L.ABSOR, 3, 0.5, 0, 0, 0.0), L.ModelCfg(L.ABSOR, 3, 0.5, 2, 0, 0.0)
    assert _host(weighted, [ident], pair + [2.5]) == (L.OK, 0, 0.125)   # the weight does not enter the decision
    assert _host(weighted, [ident], pair + [np.nan]) == (L.OK, -1, np.inf)
    assert _host(weighted, [ident], pair + [np.inf]) == (L.OK, -1, np.inf)
    assert _host(plain, [ident], pair + [np.nan]) == (L.OK, 0, 0.125)   # records of 6 doubles: slot 6 is not read


def test_host_call_pivot_by_hand():
    cfg = L.ModelCfg(L.PIVOT, 3, 0.5, 0, 0, 0.0)
    frame = np.zeros(13)
    frame[[0, 4, 8]] = 1.0                      # the identity rotation
    frame[9:12] = [10.0, 20.0, 30.0]
    frame[12] = np.nan                          # the slot of outputFormat and padding is not a coordinate
    exact = [1.0, 2.0, 3.0, 11.0, 22.0, 33.0]   # R tip + t == pivot
    off = [1.0, 2.0, 3.0, 11.0, 22.0, 33.125]
    assert _host(cfg, [exact], frame) == (L.OK, 0, 0.0)
    assert _host(cfg, [off], frame) == (L.OK, 0, 0.125)
    assert _host(cfg, [off, exact], frame) == (L.OK, 1, 0.0)
    assert _host(cfg, [[1.0, 2.0, 3.0, 11.0, 22.0, 33.5]], frame) == (L.OK, -1, np.inf)
    for k in range(12):
        bad = frame.copy()
        bad[k] = np.nan
        assert _host(cfg, [exact], bad) == (L.OK, -1, np.inf), k


def test_host_call_ray_by_hand():
    cfg = L.ModelCfg(L.RAY, 3, 0.5, 0, 0, 0.0)
    through = [0.0, 0.0, -2.0, 0.0, 0.0, 1.0]      # a ray through the model's point
    beside = [0.0, 0.125, -2.0, 0.0, 0.0, 1.0]
    away = [0.0, 0.125, 2.0, 0.0, 0.0, 1.0]        # the same line, but the point lies behind the ray's origin
    assert _host(cfg, [[0.0, 0.0, 0.0]], through) == (L.OK, 0, 0.0)
    assert _host(cfg, [[0.0, 0.0, 0.0]], beside) == (L.OK, 0, 0.125)
    assert _host(cfg, [[0.0, 0.0, 0.0]], away) == (L.OK, -1, np.inf)           # agree() holds t >= 0
    assert _host(cfg, [[0.0, 0.0, 0.0], [0.0, 0.0625, 5.0]], beside) == (L.OK, 1, 0.0625)
    assert _host(cfg, [[0.0, 0.0, 0.0], [0.0, 0.0625, 5.0]], away) == (L.OK, 1, 0.0625)
    assert _host(cfg, [[0.0, 0.625, 0.0]], beside) == (L.OK, -1, np.inf)
    for k in range(6):
        bad = list(beside)
        bad[k] = np.nan
        assert _host(cfg, [[0.0, 0.0, 0.0]], bad) == (L.OK, -1, np.inf), k
    # aux (the estimator's parallelism threshold) is not used by the decision
    assert _host(L.ModelCfg(L.RAY, 3, 0.5, 0, 0, 0.3), [[0.0, 0.0, 0.0]], beside) == (L.OK, 0, 0.125)


def test_assign_host_keeps_refusing_the_three_models():
    lib = L.load()
    label, res = C.c_int32(42), C.c_double(42.0)
    params, rec = np.zeros((1, 7)), np.zeros(13)
    params[0, 0] = 1.0
    for model, ls in ((L.ABSOR, 0), (L.ABSOR, 2), (L.PIVOT, 0), (L.RAY, 0)):
        cfg = L.ModelCfg(model, 3, 0.5, ls, 0, 0.0)
        assert lib.lsqr_assign_host(C.byref(cfg), L.ptr(params), 1, L.ptr(rec), C.byref(label),
                                    C.byref(res)) == L.ERR_INVALID
        assert lib.lsqr_assign_dense_host(C.byref(cfg), L.ptr(params), 1, L.ptr(rec), C.byref(label),
                                          C.byref(res)) == L.ERR_INVALID
        assert label.value == 42 and res.value == 42.0
        assert lib.lsqr_assign_rigid_host(C.byref(cfg), L.ptr(params), 1, L.ptr(rec), C.byref(label), None) == L.OK
        label.value = 42


def test_context_methods():
    sig = inspect.signature(Context.assign_rigid)
    assert list(sig.parameters) == ["self", "params", "want_residuals", "labels_out"]
    par = sig.parameters
    assert par["params"].default is inspect.Parameter.empty
    assert par["want_residuals"].default is False and par["labels_out"].default is None
    sig = inspect.signature(Context.refine_rigid)
    assert list(sig.parameters) == ["self", "params", "max_rounds", "labels_out"]
    par = sig.parameters
    assert par["params"].default is inspect.Parameter.empty
    assert par["max_rounds"].default == 8 and par["labels_out"].default is None
