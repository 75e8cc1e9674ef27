"""lsqr_refine_lm_grouped's arguments.  On the CPU: liblsqr_hip.so exports the symbol, the ctypes table gives it the
header's argument list (lsqr_refine_grouped's), a null context is refused before anything is touched, and
Context.refine_lm_grouped has refine_grouped's parameters and defaults.  On the GPU (a context needs a device): the
order of the checks, "every argument error writes nothing" with every output pre-filled, the model gate and its
message, and the state errors."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd import synth
from lsqrrecipes_amd.context import Context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FN = "lsqr_refine_lm_grouped"
CTYPES = {"lsqr_ctx *": C.c_void_p, "const int32_t *": C.c_void_p, "const size_t *": C.c_void_p, "size_t": C.c_size_t,
          "int": C.c_int, "double *": C.c_void_p, "uint64_t *": C.c_void_p, "lsqr_fit_info *": C.c_void_p,
          "int32_t *": C.c_void_p, "size_t *": C.c_void_p}
NAMES = ["ctx", "groups", "n_groups", "on_device", "params_inout", "n_models", "max_models", "max_rounds", "labels_out",
         "counts_out", "offsets_out", "fits", "status_out", "rounds_out", "converged_out"]
NG, MM, N, DELTA = 3, 2, 900, 0.5


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
    """every output of the call, pre-filled"""

    def __init__(self, n=N, ng=NG, mm=MM, p=4):
        self.params = np.full((ng, mm, p), 42.0)
        self.labels = np.full(n, 42, dtype=np.int32)
        self.counts = np.full((ng, mm + 1), 42, dtype=np.uint64)
        self.offs = np.full(ng + 1, 42, dtype=np.uint64)
        self.status = np.full(ng * mm, 42, dtype=np.int32)
        self.fits = (L.FitInfo * (ng * mm))()
        C.memset(self.fits, 0x5A, C.sizeof(self.fits))
        self.rounds = np.full(ng, 42, dtype=np.uintp)
        self.conv = np.full(ng, 42, dtype=np.int32)

    def untouched(self):
        return (np.all(self.params == 42.0) and np.all(self.labels == 42) and np.all(self.counts == 42)
                and np.all(self.offs == 42) and np.all(self.status == 42)
                and bytes(self.fits) == b"\x5a" * C.sizeof(self.fits) and np.all(self.rounds == 42)
                and np.all(self.conv == 42))


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_symbol_exported_with_the_headers_argument_list():
    lib = L.load()
    f = getattr(lib, FN)
    res, args = L.SIGNATURES[FN]
    assert f.restype is res is C.c_int
    assert list(f.argtypes) == args
    decl = _header_args(FN)
    assert [n for _, n in decl] == NAMES
    assert decl == _header_args("lsqr_refine_grouped")  # the same call for another model
    assert args == L.SIGNATURES["lsqr_refine_grouped"][1]
    assert len(args) == len(decl)
    for a, (t, name) in zip(args, decl):
        assert a is CTYPES[t], (name, t, a)


def test_null_context_is_refused_before_anything_is_touched():
    lib = L.load()
    groups = np.zeros(N, dtype=np.int32)
    nm = np.full(NG, MM, dtype=np.uintp)
    o = Outputs()
    for n, m in ((NG, MM), (0, MM), (NG, 65), (NG, 0)):
        assert getattr(lib, FN)(None, L.ptr(groups), n, 0, L.ptr(o.params), L.ptr(nm), m, 4, L.ptr(o.labels),
                                L.ptr(o.counts), L.ptr(o.offs), o.fits, L.ptr(o.status), L.ptr(o.rounds),
                                L.ptr(o.conv)) == L.ERR_INVALID
        assert o.untouched()


def test_context_method():
    sig = inspect.signature(Context.refine_lm_grouped)
    assert list(sig.parameters) == ["self", "groups", "n_groups", "params", "n_models", "max_rounds", "labels_out"]
    assert list(sig.parameters) == list(inspect.signature(Context.refine_grouped).parameters)
    par = sig.parameters
    for name in ("groups", "n_groups", "params"):
        assert par[name].default is inspect.Parameter.empty
    assert par["n_models"].default is None and par["max_rounds"].default == 8 and par["labels_out"].default is None


# ---- GPU ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _scene():
    """three groups of 300 records of one sphere each, interleaved; two start rows per group"""
    parts = [synth.sphere(N // NG, 0.2, seed=0x7A00 + g, sigma=0.1) for g in range(NG)]
    data = np.ascontiguousarray(np.stack([p[0] for p in parts], axis=1).reshape(N, 3))
    groups = np.tile(np.arange(NG, dtype=np.int32), N // NG)
    rows = np.zeros((NG, MM, 4))
    for g in range(NG):
        rows[g, 0] = parts[g][1]
        rows[g, 1] = parts[g][1] + 0.05
    return data, groups, rows


@pytest.mark.gpu
def test_argument_errors_in_order_write_nothing(ctx):
    lib = L.load()
    call_ = getattr(lib, FN)
    data, groups, rows = _scene()
    ctx.set_model(L.SPHERE, 3, DELTA, L.LS_GEOMETRIC).upload(data)
    o = Outputs()
    nmod = np.full(NG, MM, dtype=np.uintp)
    too_many = nmod.copy()
    too_many[NG - 1] = MM + 1

    def call(c=ctx, groups_=groups, ng=NG, par_=o.params, nm_=nmod, mm=MM, fits_=o.fits, status_=o.status,
             rounds_=o.rounds, conv_=o.conv):
        return call_(c._h, L.ptr(groups_), ng, 0, L.ptr(par_), L.ptr(nm_), mm, 4, L.ptr(o.labels), L.ptr(o.counts),
                     L.ptr(o.offs), fits_, L.ptr(status_), L.ptr(rounds_), L.ptr(conv_))

    # n_groups == 0 is a no-op and comes before every argument check
    assert call(ng=0, mm=65, groups_=None) == L.OK and o.untouched()
    assert call(ng=0, par_=None, nm_=None, fits_=None) == L.OK and o.untouched()
    assert call(mm=65) == L.ERR_INVALID and o.untouched()
    assert call(ng=2 ** 31) == L.ERR_INVALID and o.untouched()
    # null required pointers
    assert call(groups_=None) == L.ERR_INVALID and o.untouched()
    assert call(par_=None) == L.ERR_INVALID and o.untouched()
    assert call(nm_=None) == L.ERR_INVALID and o.untouched()
    assert call(fits_=None) == L.ERR_INVALID and o.untouched()
    assert call(status_=None) == L.ERR_INVALID and o.untouched()
    assert call(rounds_=None) == L.ERR_INVALID and o.untouched()
    assert call(conv_=None) == L.ERR_INVALID and o.untouched()
    # an n_models[g] above max_models
    assert call(nm_=too_many) == L.ERR_INVALID and o.untouched()
    assert "n_models[%d]" % (NG - 1) in lib.lsqr_last_error(ctx._h).decode()
    with Context(0) as empty:
        # the model comes first: no model is a state error even with n_groups == 0 and with bad arguments
        assert call(c=empty) == L.ERR_STATE and call(c=empty, ng=0) == L.ERR_STATE
        assert call(c=empty, mm=65) == L.ERR_STATE and o.untouched()
        empty.set_model(L.SPHERE, 3, DELTA, L.LS_GEOMETRIC)
        # the arguments come before the records: no records is a state error only with good arguments
        assert call(c=empty, mm=65) == L.ERR_INVALID and call(c=empty, nm_=too_many) == L.ERR_INVALID
        assert call(c=empty, fits_=None) == L.ERR_INVALID
        assert call(c=empty) == L.ERR_STATE and o.untouched()
        assert call(c=empty, ng=0) == L.OK and o.untouched()
    # good arguments run; the optional outputs may be absent
    par = rows.copy()
    assert call_(ctx._h, L.ptr(groups), NG, 0, L.ptr(par), L.ptr(nmod), MM, 1, None, None, None, o.fits, L.ptr(o.status),
                 L.ptr(o.rounds), L.ptr(o.conv)) == L.OK
    assert np.all(o.rounds == 1) and np.all(o.labels == 42) and np.all(o.counts == 42) and np.all(o.offs == 42)
    got = ctx.refine_lm_grouped(groups, NG, rows, max_rounds=1)
    assert np.array_equal(bits(got["params"]), bits(par))
    assert [f.lm_nfev for f in o.fits] == list(got["lm_nfev"].ravel())
    # max_models == 0: LSQR_OK, every label -1, zero outputs
    none = np.zeros(NG, dtype=np.uintp)
    assert call_(ctx._h, L.ptr(groups), NG, 0, L.ptr(par), L.ptr(none), 0, 4, L.ptr(o.labels), None, None, o.fits,
                 L.ptr(o.status), L.ptr(o.rounds), L.ptr(o.conv)) == L.OK
    assert np.all(o.labels == -1) and not o.rounds.any() and not o.conv.any()


@pytest.mark.gpu
def test_model_gate_names_the_call_that_takes_the_model(ctx):
    lib = L.load()
    data, groups, rows = _scene()
    ctx.set_model(L.SPHERE, 3, DELTA, L.LS_GEOMETRIC).upload(data)
    o = Outputs(p=8)
    nmod = np.full(NG, MM, dtype=np.uintp)
    for model, dim, ls in ((L.SPHERE, 3, L.LS_ALGEBRAIC), (L.PLANE, 3, L.LS_ALGEBRAIC), (L.ABSOR, 3, 0)):
        ctx.set_model(model, dim, DELTA, ls)
        for ng, mm in ((NG, MM), (0, MM), (NG, 65)):  # the gate comes before n_groups == 0 and before the arguments
            assert getattr(lib, FN)(ctx._h, L.ptr(groups), ng, 0, L.ptr(o.params), L.ptr(nmod), mm, 4, L.ptr(o.labels),
                                    L.ptr(o.counts), L.ptr(o.offs), o.fits, L.ptr(o.status), L.ptr(o.rounds),
                                    L.ptr(o.conv)) == L.ERR_INVALID, (model, ng, mm)
            assert o.untouched(), (model, ng, mm)
        msg = lib.lsqr_last_error(ctx._h).decode()
        assert FN in msg and "lsqr_refine_grouped" in msg.replace(FN, ""), msg
    ctx.set_model(L.PLANE, 3, DELTA, L.LS_ALGEBRAIC).upload(data)
    with pytest.raises(L.LsqrError) as e:
        ctx.refine_lm_grouped(groups, NG, np.zeros((NG, MM, 6)))
    assert e.value.status == L.ERR_INVALID
