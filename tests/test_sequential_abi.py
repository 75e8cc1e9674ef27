"""CPU checks of the sequential RANSAC entry point's Python mirror: liblsqr_hip.so exports lsqr_ransac_sequential, the
ctypes table gives it the header's argument types, and Context has the method with the documented defaults."""
import ctypes as C
import inspect

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd.context import Context


def test_symbol_exported_with_argtypes():
    lib = L.load()
    fn = lib.lsqr_ransac_sequential
    res, args = L.SIGNATURES["lsqr_ransac_sequential"]
    assert fn.restype is res is C.c_int
    assert list(fn.argtypes) == args and len(args) == 10
    # (ctx, p, seeds, max_models, min_votes, params, labels, infos, status, n_models)
    assert args[1] is C.c_double and args[3] is C.c_size_t and args[4] is C.c_uint64
    assert args[9] == C.POINTER(C.c_size_t)


def test_argument_checks_need_no_device():
    lib = L.load()
    n = C.c_size_t(7)
    # a null context is refused before anything is touched
    assert lib.lsqr_ransac_sequential(None, 0.99, None, 0, 0, None, None, None, None, C.byref(n)) == L.ERR_INVALID
    assert n.value == 7


def test_context_method():
    sig = inspect.signature(Context.ransac_sequential)
    assert list(sig.parameters) == ["self", "p", "max_models", "seeds", "min_votes", "want_labels"]
    assert sig.parameters["seeds"].default is None and sig.parameters["min_votes"].default == 0
    assert sig.parameters["want_labels"].default is True
