"""lsqr_assign_dense_grouped / lsqr_refine_dense_grouped: their arguments.  On the CPU: liblsqr_hip.so exports both
symbols, the ctypes table gives each the header's argument list (lsqr_assign_grouped's / lsqr_refine_grouped's), a null
context is refused before anything is touched, and Context.assign_dense_grouped / refine_dense_grouped have
assign_grouped's / refine_grouped's parameters and defaults.  On the GPU (a context needs a device): the order of the
checks, "every argument error writes nothing" with every output pre-filled, the model gate and its message, the state
errors, and max_models == 0."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd.context import Context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSIGN, REFINE = "lsqr_assign_dense_grouped", "lsqr_refine_dense_grouped"
CTYPES = {"lsqr_ctx *": C.c_void_p, "const int32_t *": C.c_void_p, "const size_t *": C.c_void_p, "size_t": C.c_size_t,
          "int": C.c_int, "double *": C.c_void_p, "const double *": C.c_void_p, "uint64_t *": C.c_void_p,
          "lsqr_fit_info *": C.c_void_p, "int32_t *": C.c_void_p, "size_t *": C.c_void_p}
ASSIGN_NAMES = ["ctx", "groups", "n_groups", "on_device", "params", "n_models", "max_models", "labels_out",
                "residuals_out", "counts_out", "offsets_out"]
REFINE_NAMES = ["ctx", "groups", "n_groups", "on_device", "params_inout", "n_models", "max_models", "max_rounds",
                "labels_out", "counts_out", "offsets_out", "fits", "status_out", "rounds_out", "converged_out"]
NG, MM, N, DIM, DELTA = 3, 2, 900, 5, 0.04


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


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


class Outputs:
    """every output of the two calls, pre-filled"""

    def __init__(self, n=N, ng=NG, mm=MM, p=DIM):
        self.params = np.full((ng, mm, p), 42.0)
        self.labels = np.full(n, 42, dtype=np.int32)
        self.res = np.full(n, 42.0)
        self.counts = np.full((ng, mm + 1), 42, dtype=np.uint64)
        self.offs = np.full(ng + 1, 42, dtype=np.uint64)
        self.status = np.full(ng * mm, 42, dtype=np.int32)
        self.fits = (L.FitInfo * (ng * mm))()
        C.memset(self.fits, 0x5A, C.sizeof(self.fits))
        self.rounds = np.full(ng, 42, dtype=np.uintp)
        self.conv = np.full(ng, 42, dtype=np.int32)

    def untouched(self):
        return (np.all(self.params == 42.0) and np.all(self.labels == 42) and np.all(self.res == 42.0)
                and np.all(self.counts == 42) and np.all(self.offs == 42) and np.all(self.status == 42)
                and bytes(self.fits) == b"\x5a" * C.sizeof(self.fits) and np.all(self.rounds == 42)
                and np.all(self.conv == 42))


def _calls(lib, o, groups, nmod):
    """the two entry points with every argument a keyword that may be replaced -> assign, refine"""

    def assign(h, groups_=groups, ng=NG, par_=o.params, nm_=nmod, mm=MM, labels_=o.labels):
        return getattr(lib, ASSIGN)(h, L.ptr(groups_), ng, 0, L.ptr(par_), L.ptr(nm_), mm, L.ptr(labels_), L.ptr(o.res),
                                    L.ptr(o.counts), L.ptr(o.offs))

    def refine(h, groups_=groups, ng=NG, par_=o.params, nm_=nmod, mm=MM, fits_=o.fits, status_=o.status,
               rounds_=o.rounds, conv_=o.conv):
        return getattr(lib, REFINE)(h, L.ptr(groups_), ng, 0, L.ptr(par_), L.ptr(nm_), mm, 4, L.ptr(o.labels),
                                    L.ptr(o.counts), L.ptr(o.offs), fits_, L.ptr(status_), L.ptr(rounds_), L.ptr(conv_))

    return assign, refine


# ---- CPU ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn, names, twin", [(ASSIGN, ASSIGN_NAMES, "lsqr_assign_grouped"),
                                             (REFINE, REFINE_NAMES, "lsqr_refine_grouped")])
def test_symbols_exported_with_the_headers_argument_lists(fn, names, twin):
    lib = L.load()
    f = getattr(lib, fn)
    res, args = L.SIGNATURES[fn]
    assert f.restype is res is C.c_int
    assert list(f.argtypes) == args
    decl = _header_args(fn)
    assert [n for _, n in decl] == names
    assert decl == _header_args(twin)  # the same call for another model
    assert args == L.SIGNATURES[twin][1]
    assert len(args) == len(decl)
    for a, (t, name) in zip(args, decl):
        assert a is CTYPES[t], (name, t, a)


def test_null_context_is_refused_before_anything_is_touched():
    lib = L.load()
    groups = np.zeros(N, dtype=np.int32)
    nm = np.full(NG, MM, dtype=np.uintp)
    o = Outputs()
    assign, refine = _calls(lib, o, groups, nm)
    for n, m in ((NG, MM), (0, MM), (NG, 65), (NG, 0)):
        assert assign(None, ng=n, mm=m) == L.ERR_INVALID and o.untouched()
        assert refine(None, ng=n, mm=m) == L.ERR_INVALID and o.untouched()


def test_context_methods():
    for name, twin, extra in (("assign_dense_grouped", "assign_grouped", ("want_residuals", False)),
                              ("refine_dense_grouped", "refine_grouped", ("max_rounds", 8))):
        sig = inspect.signature(getattr(Context, name))
        assert list(sig.parameters) == ["self", "groups", "n_groups", "params", "n_models", extra[0], "labels_out"]
        assert list(sig.parameters) == list(inspect.signature(getattr(Context, twin)).parameters)
        par = sig.parameters
        for p in ("groups", "n_groups", "params"):
            assert par[p].default is inspect.Parameter.empty
        assert par["n_models"].default is None and par["labels_out"].default is None
        assert par[extra[0]].default == extra[1] and type(par[extra[0]].default) is type(extra[1])


# ---- GPU ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _scene():
    """three groups of 300 rows of one regression each, interleaved; two start rows per group"""
    g = np.random.default_rng(0xD6A)
    X = g.normal(size=(NG, DIM))
    groups = np.tile(np.arange(NG, dtype=np.int32), N // NG)
    data = np.empty((N, DIM + 1))
    data[:, :DIM] = g.normal(size=(N, DIM))
    data[:, DIM] = np.einsum("ij,ij->i", data[:, :DIM], X[groups]) + 0.01 * g.normal(size=N)
    rows = np.zeros((NG, MM, DIM))
    rows[:, 0] = X + 0.001
    rows[:, 1] = X + 1e4
    return data, groups, rows


@pytest.mark.gpu
def test_argument_errors_in_order_write_nothing(ctx):
    lib = L.load()
    data, groups, rows = _scene()
    ctx.set_model(L.DENSE, DIM, DELTA).upload(data)
    o = Outputs()
    nmod = np.full(NG, MM, dtype=np.uintp)
    too_many = nmod.copy()
    too_many[NG - 1] = MM + 1
    assign, refine = _calls(lib, o, groups, nmod)
    h = ctx._h
    for call in (assign, refine):
        # n_groups == 0 is a no-op and comes before every argument check
        assert call(h, ng=0, mm=65, groups_=None) == L.OK and o.untouched()
        assert call(h, ng=0, par_=None, nm_=None) == L.OK and o.untouched()
        assert call(h, mm=65) == L.ERR_INVALID and o.untouched()
        assert call(h, ng=2 ** 31) == L.ERR_INVALID and o.untouched()
        # null required pointers
        assert call(h, groups_=None) == L.ERR_INVALID and o.untouched()
        assert call(h, par_=None) == L.ERR_INVALID and o.untouched()
        assert call(h, nm_=None) == L.ERR_INVALID and o.untouched()
        # an n_models[g] above max_models
        assert call(h, nm_=too_many) == L.ERR_INVALID and o.untouched()
        assert "n_models[%d]" % (NG - 1) in lib.lsqr_last_error(h).decode()
    assert assign(h, labels_=None) == L.ERR_INVALID and o.untouched()
    assert refine(h, fits_=None) == L.ERR_INVALID and o.untouched()
    assert refine(h, status_=None) == L.ERR_INVALID and o.untouched()
    assert refine(h, rounds_=None) == L.ERR_INVALID and o.untouched()
    assert refine(h, conv_=None) == L.ERR_INVALID and o.untouched()
    with Context(0) as empty:
        e = empty._h
        for call in (assign, refine):
            # the model comes first: no model is a state error even with n_groups == 0 and with bad arguments
            assert call(e) == L.ERR_STATE and call(e, ng=0) == L.ERR_STATE
            assert call(e, mm=65) == L.ERR_STATE and o.untouched()
        empty.set_model(L.DENSE, DIM, DELTA)
        for call in (assign, refine):
            # the arguments come before the records: no records is a state error only with good arguments
            assert call(e, mm=65) == L.ERR_INVALID and call(e, nm_=too_many) == L.ERR_INVALID
            assert call(e, par_=None) == L.ERR_INVALID
            assert call(e) == L.ERR_STATE and o.untouched()
            assert call(e, ng=0) == L.OK and o.untouched()
    # good arguments run; the optional outputs may be absent
    par = rows.copy()
    assert getattr(lib, REFINE)(h, L.ptr(groups), NG, 0, L.ptr(par), L.ptr(nmod), MM, 1, None, None, None, o.fits,
                                L.ptr(o.status), L.ptr(o.rounds), L.ptr(o.conv)) == L.OK
    assert np.all(o.rounds == 1) and np.all(o.labels == 42) and np.all(o.counts == 42) and np.all(o.offs == 42)
    got = ctx.refine_dense_grouped(groups, NG, rows, max_rounds=1)
    assert np.array_equal(bits(got["params"]), bits(par))
    assert [f.n_used for f in o.fits] == list(got["n_used"].ravel())
    assert getattr(lib, ASSIGN)(h, L.ptr(groups), NG, 0, L.ptr(par), L.ptr(nmod), MM, L.ptr(o.labels), None, None,
                                None) == L.OK
    assert np.array_equal(o.labels, ctx.assign_dense_grouped(groups, NG, par)["labels"]) and np.all(o.res == 42.0)


@pytest.mark.gpu
def test_max_models_zero(ctx):
    """LSQR_OK, every label -1, every residual +inf, zero outputs, the parameters not read"""
    lib = L.load()
    data, groups, rows = _scene()
    ctx.set_model(L.DENSE, DIM, DELTA).upload(data)
    o = Outputs()
    none = np.zeros(NG, dtype=np.uintp)
    par = np.full(1, 42.0)
    h = ctx._h
    assert getattr(lib, ASSIGN)(h, L.ptr(groups), NG, 0, L.ptr(par), L.ptr(none), 0, L.ptr(o.labels), L.ptr(o.res),
                                L.ptr(o.counts), L.ptr(o.offs)) == L.OK
    assert np.all(o.labels == -1) and np.all(np.isposinf(o.res)) and par[0] == 42.0
    assert list(o.counts.ravel()[:NG]) == [N // NG] * NG  # (max_models + 1 = 1 slot per group: the unassigned rows)
    assert list(o.offs) == [0, N // NG, 2 * N // NG, N]
    o.labels[:] = 42
    assert getattr(lib, REFINE)(h, L.ptr(groups), NG, 0, L.ptr(par), L.ptr(none), 0, 4, L.ptr(o.labels), None, None,
                                o.fits, L.ptr(o.status), L.ptr(o.rounds), L.ptr(o.conv)) == L.OK
    assert np.all(o.labels == -1) and not o.rounds.any() and not o.conv.any() and par[0] == 42.0
    assert np.all(o.status == 42) and bytes(o.fits) == b"\x5a" * C.sizeof(o.fits)  # no (group, model) entry exists


@pytest.mark.gpu
def test_model_gate_names_the_call_that_takes_the_model(ctx):
    lib = L.load()
    data, groups, rows = _scene()
    o = Outputs(p=8)
    nmod = np.full(NG, MM, dtype=np.uintp)
    assign, refine = _calls(lib, o, groups, nmod)
    for model, dim, ls in ((L.PLANE, 3, L.LS_ALGEBRAIC), (L.SPHERE, 3, L.LS_ALGEBRAIC), (L.SPHERE, 3, L.LS_GEOMETRIC),
                           (L.ABSOR, 3, 0)):
        ctx.set_model(model, dim, 0.5, ls)
        for call, fn in ((assign, ASSIGN), (refine, REFINE)):
            for ng, mm in ((NG, MM), (0, MM), (NG, 65)):  # the gate comes before n_groups == 0 and the arguments
                assert call(ctx._h, ng=ng, mm=mm) == L.ERR_INVALID, (model, fn, ng, mm)
                assert o.untouched(), (model, fn, ng, mm)
            msg = lib.lsqr_last_error(ctx._h).decode()
            assert fn in msg and "lsqr_assign_grouped / lsqr_refine_grouped" in msg, msg
    ctx.set_model(L.PLANE, 3, 0.5, L.LS_ALGEBRAIC).upload(np.zeros((N, 3)))
    for method in (ctx.assign_dense_grouped, ctx.refine_dense_grouped):
        with pytest.raises(L.LsqrError) as e:
            method(groups, NG, np.zeros((NG, MM, 6)))
        assert e.value.status == L.ERR_INVALID
    # the ungrouped dense pair and the grouped point pair keep their own gates and messages
    par = np.zeros((NG, MM, 6))
    assert lib.lsqr_assign_dense(ctx._h, L.ptr(par), 1, 0, L.ptr(o.labels), None, None) == L.ERR_INVALID
    assert "lsqr_assign / lsqr_refine take" in lib.lsqr_last_error(ctx._h).decode()
    ctx.set_model(L.DENSE, DIM, DELTA).upload(data)
    assert lib.lsqr_assign_grouped(ctx._h, L.ptr(groups), NG, 0, L.ptr(par), L.ptr(nmod), MM, L.ptr(o.labels), None,
                                   None, None) == L.ERR_INVALID
    assert o.untouched()
