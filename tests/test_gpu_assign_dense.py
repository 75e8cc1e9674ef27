"""lsqr_assign_dense / lsqr_refine_dense (csrc/assign_dense.h) through Context.assign_dense / Context.refine_dense.

assign: labels and residuals bit-equal to lsqr_assign_dense_host row by row, and to the numpy argmin (first minimum)
over Context.residuals(row_m) masked by Context.mask(row_m) -- device paths that existed before this call.
refine, one round at a time: model m's new row against set_mask(L_0 == m) + ls_fit(use_mask=True) on the same context
at 1e-6 relative (the README's fit tolerance, the bar of tests/test_gpu_dense_cond.py); n_used, status and route equal;
the returned labels bit-equal to assign_dense of the returned parameters.
Shapes: both sides of every row class (8, 16, 32, 64), row counts around the pass's chunk, 1 to 64 models, tight and
padded stride, upload and rows attached from device memory with device labels."""
import ctypes as C
import threading

import numpy as np
import pytest

import linalg_families as F
from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd.context import Context
from oracle import pyoracle as O
from test_gpu_assign import DeviceArray

pytestmark = pytest.mark.gpu
DIMS = (1, 8, 9, 16, 17, 32, 33, 64)
SIGMA = 0.01
DELTA = 4 * SIGMA
REL = 1e-6  # the README's fit tolerance (tests/test_gpu_dense_cond.py:132)


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


def counts_of(labels, m):
    return np.array([np.sum(labels == k) for k in range(m)] + [np.sum(labels == -1)], dtype=np.uint64)


def mixture(n, N, M, seed):
    """N rows (a | b), a Gaussian, each on one of M planted regressions with noise SIGMA -> rows, X (M x n), owner"""
    g = np.random.default_rng([seed, n, N, M])
    X = g.normal(size=(M, n))
    rows = np.empty((N, n + 1))
    rows[:, :n] = g.normal(size=(N, n))
    owner = g.integers(0, M, size=N)
    rows[:, n] = np.einsum("ij,ij->i", rows[:, :n], X[owner]) + SIGMA * g.normal(size=N)
    return rows, X, owner


def put(ctx, n, rows, pad=0, delta=DELTA):
    """the rows on the context, `pad` doubles of filler after each"""
    wide = rows
    if pad:
        wide = np.full((len(rows), n + 1 + pad), -7.25)
        wide[:, :n + 1] = rows
    ctx.set_model(L.DENSE, n, delta).upload(wide)
    return ctx


def host_rows(n, params, rows, delta=DELTA):
    """lsqr_assign_dense_host row by row -> labels, residuals"""
    cfg = L.ModelCfg(L.DENSE, n, delta, 0, 0, 0.0)
    flat = np.ascontiguousarray(params, dtype=np.float64)
    label, res = C.c_int32(0), C.c_double(0.0)
    labels, residuals = np.empty(len(rows), dtype=np.int32), np.empty(len(rows))
    fn = L.load().lsqr_assign_dense_host
    for i, x in enumerate(rows):
        rec = np.ascontiguousarray(x)
        assert fn(C.byref(cfg), L.ptr(flat), len(flat), L.ptr(rec), C.byref(label), C.byref(res)) == L.OK
        labels[i], residuals[i] = label.value, res.value
    return labels, residuals


def device_argmin(ctx, params):
    """the existing device paths: one residual pass and one mask pass per model row, a numpy argmin (first minimum)"""
    res = np.array([ctx.residuals(p) for p in params])
    masks = np.array([ctx.mask(p)[0] for p in params])
    masked = np.where(masks != 0, res, np.inf)
    labels = np.where(masks.any(axis=0), np.argmin(masked, axis=0), -1).astype(np.int32)
    return labels, masked.min(axis=0)


def check_assign(ctx, n, rows, params, pad):
    put(ctx, n, rows, pad)
    got = ctx.assign_dense(params, want_residuals=True)
    hl, hr = host_rows(n, params, rows)
    dl, dr = device_argmin(ctx, params)
    what = (n, len(rows), len(params), pad)
    assert np.array_equal(got["labels"], hl) and np.array_equal(bits(got["residuals"]), bits(hr)), what
    assert np.array_equal(got["labels"], dl) and np.array_equal(bits(got["residuals"]), bits(dr)), what
    assert np.array_equal(got["counts"], counts_of(hl, len(params))), what
    zero = ctx.refine_dense(params, max_rounds=0)  # max_rounds = 0 is assign
    assert zero["rounds"] == 0 and not zero["converged"] and np.array_equal(zero["labels"], hl), what
    assert np.array_equal(bits(zero["params"]), bits(np.asarray(params, dtype=np.float64))), what
    assert np.array_equal(zero["counts"], got["counts"]) and np.all(zero["status"] == L.OK), what
    assert not np.any(zero["n_used"]) and not np.any(zero["route"]), what
    return got


# ---- assign ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", DIMS)
def test_assign_row_counts_around_the_chunk(ctx, n):
    chunk = L.assign_dense_chunk(n)
    base, X, _ = mixture(n, 3 * chunk + 5, 5, 1)
    base[1, n // 2] = np.nan  # non-finite rows: a NaN coefficient, an infinite right-hand side
    base[2, n] = np.inf
    for k, N in enumerate(sorted({1, max(n - 1, 1), chunk - 1, chunk, chunk + 1, 3 * chunk + 5})):
        got = check_assign(ctx, n, base[:N], X, pad=(0, 2)[k & 1])
        if N > 2:
            assert got["labels"][1] == -1 == got["labels"][2] and np.all(np.isinf(got["residuals"][1:3]))
    assert set(np.unique(got["labels"])) == {-1, 0, 1, 2, 3, 4}


@pytest.mark.parametrize("n", DIMS)
def test_assign_model_counts(ctx, n):
    chunk = L.assign_dense_chunk(n)
    N = 3 * chunk + 5
    for k, M in enumerate((1, 2, 5, 64)):
        rows, X, _ = mixture(n, N, min(M, 7), 2)
        params = X
        if M == 64:  # seven planted regressions among 57 that no row is near
            g = np.random.default_rng(64)
            params = X[g.integers(0, 7, size=64)] + 1e6
            where = [3, 9, 17, 30, 31, 50, 63]
            params[where] = X
        got = check_assign(ctx, n, rows, params, pad=(0, 3)[k & 1])
        if M == 64:
            assert all(got["counts"][m] == 0 for m in range(64) if m not in where)  # models with no rows
            assert all(got["counts"][m] > 0 for m in where)
    with pytest.raises(L.LsqrError) as e:
        ctx.assign_dense(np.vstack([params, params[:1]]))
    assert e.value.status == L.ERR_INVALID
    far = ctx.assign_dense(X + 1e6, want_residuals=True)  # all rows unassigned
    assert np.all(far["labels"] == -1) and np.all(np.isinf(far["residuals"])) and far["counts"][-1] == N
    empty = ctx.assign_dense(np.zeros((0, n)))
    assert np.all(empty["labels"] == -1) and list(empty["counts"]) == [N]


def test_assign_wide_band_ties_decided_by_the_residual(ctx):
    """a band that most rows share with several regressions, and two identical regressions: the smaller m"""
    n = 9
    rows, X, _ = mixture(n, 700, 4, 3)
    params = np.vstack([X, X[1:2]])  # model 4 is model 1 again
    put(ctx, n, rows, delta=6.0)
    got = ctx.assign_dense(params, want_residuals=True)
    hl, hr = host_rows(n, params, rows, delta=6.0)
    dl, dr = device_argmin(ctx, params)
    masks = np.array([ctx.mask(p)[0] for p in params])
    assert np.sum(masks.sum(axis=0) > 1) > 350
    assert np.array_equal(got["labels"], hl) and np.array_equal(bits(got["residuals"]), bits(hr))
    assert np.array_equal(got["labels"], dl) and np.array_equal(bits(got["residuals"]), bits(dr))
    assert got["counts"][4] == 0 and got["counts"][1] > 0


@pytest.mark.parametrize("n", [9, 64])
def test_attached_tensor_and_device_labels(ctx, n):
    """the rows attached from device memory at a padded stride, the labels into a device tensor: DeviceArray is a
    device allocation with the tensor attributes Context looks at (data_ptr, is_cuda, dtype, ...)"""
    N = 3 * L.assign_dense_chunk(n) + 5
    rows, X, _ = mixture(n, N, 3, 4)
    start = X + SIGMA / np.sqrt(n) * np.random.default_rng(5).normal(size=X.shape)
    put(ctx, n, rows)
    host = ctx.assign_dense(start, want_residuals=True)
    ref_host = ctx.refine_dense(start, max_rounds=2)
    wide = np.full((N, n + 3), -7.25)
    wide[:, :n + 1] = rows
    t = DeviceArray(wide)
    lab = DeviceArray(np.full(N, -9, dtype=np.int32))
    try:
        ctx.attach(t.data_ptr(), N, (n + 3) * 8, keepalive=t)
        dev = ctx.assign_dense(start, labels_out=lab)
        assert dev["labels"] is lab and np.array_equal(lab.get(), host["labels"])
        assert np.array_equal(dev["counts"], host["counts"])
        at = ctx.assign_dense(start, want_residuals=True)
        assert np.array_equal(at["labels"], host["labels"]) and np.array_equal(bits(at["residuals"]),
                                                                                bits(host["residuals"]))
        lab.put(np.full(N, -9, dtype=np.int32))
        ref_dev = ctx.refine_dense(start, max_rounds=2, labels_out=lab)
        ctx.synchronize()
        assert ref_dev["labels"] is lab and np.array_equal(lab.get(), ref_host["labels"])
        assert np.array_equal(bits(ref_dev["params"]), bits(ref_host["params"]))
        assert ref_dev["rounds"] == ref_host["rounds"] and np.array_equal(ref_dev["route"], ref_host["route"])
        with pytest.raises(ValueError):
            ctx.assign_dense(start, want_residuals=True, labels_out=lab)
        with pytest.raises(ValueError):
            ctx.assign_dense(start, labels_out=DeviceArray(np.zeros(N - 1, dtype=np.int32)))
        assert np.array_equal(bits(t.get()), bits(wide))  # the rows are only read
    finally:
        ctx.upload(np.zeros((4, n + 1)))  # let go of the attached buffer
        ctx._keep = None
        lab.free()
        t.free()


# ---- refit, one round at a time -------------------------------------------------------------------------------------
def one_round(ctx, n, params, rows=None, bar=None, parity=None):
    """refine_dense(max_rounds = 1) against set_mask(L_0 == m) + ls_fit(use_mask = 1) -> the call's dict, the fits.
    parity (default REL for every model): the bound per model on the difference to ls_fit"""
    params = np.asarray(params, dtype=np.float64)
    l0 = ctx.assign_dense(params)["labels"]
    got = ctx.refine_dense(params, max_rounds=1)
    assert got["rounds"] == 1
    fits = []
    for m in range(len(params)):
        mask = (l0 == m).astype(np.uint8)
        ctx.set_mask(mask)
        fit, info = ctx.ls_fit(use_mask=True)
        used = int(mask.sum())
        fits.append((fit, info.reserved, used))
        assert got["n_used"][m] == used, m
        if used >= n:
            assert got["status"][m] == (L.OK if len(fit) else L.EMPTY), m
            assert got["route"][m] == info.reserved, (m, got["route"][m], info.reserved)
        else:
            assert got["status"][m] == L.EMPTY and got["route"][m] == 0, m
        if used >= n and len(fit):
            assert rel(got["params"][m], fit) < (parity[m] if parity else REL), (m, rel(got["params"][m], fit))
            if rows is not None:  # and the oracle's least squares of the same rows
                want = O.ls(O.cfg(O.DENSE, n, DELTA), rows, mask)
                assert len(want) == n and rel(got["params"][m], want) < (bar or REL), (m, rel(got["params"][m], want))
        else:  # the row keeps its values
            assert np.array_equal(bits(got["params"][m]), bits(params[m])), m
    again = ctx.assign_dense(got["params"])
    assert np.array_equal(got["labels"], again["labels"]) and np.array_equal(got["counts"], again["counts"])
    return got, fits


def perturbed(X, n, seed):
    return X + SIGMA / np.sqrt(n) * np.random.default_rng(seed).normal(size=X.shape)


@pytest.mark.parametrize("n", DIMS)
def test_one_round_equals_masked_ls_fit(ctx, n):
    N = 3 * L.assign_dense_chunk(n) + 5
    rows, X, _ = mixture(n, N, 3, 6)
    for pad in (0, 2):
        put(ctx, n, rows, pad)
        got, fits = one_round(ctx, n, perturbed(X, n, 7), rows)
        assert np.all(got["status"] == L.OK) and np.all(got["route"] == 0) and np.all(got["n_used"] >= n)
        for m in range(3):  # the refit found the planted regression
            assert rel(got["params"][m], X[m]) < 0.05


def test_one_round_models_that_keep_their_row(ctx):
    n = 8
    rows, X, _ = mixture(n, 773, 3, 8)
    g = np.random.default_rng(9)
    x3, x4, x5 = g.normal(size=(3, n)) + 1e4
    few = g.normal(size=(n - 1, n + 1))  # n - 1 rows on regression 3: too few for a refit
    few[:, n] = few[:, :n] @ x3
    one = g.normal(size=n + 1)           # twenty copies of one row on regression 4: a Gram block of rank one
    one[n] = one[:n] @ x4
    rows = np.vstack([rows[:300], few, rows[300:600], np.tile(one, (20, 1)), rows[600:]])
    params = np.vstack([perturbed(X, n, 10), x3, x4, x5])  # regression 5 has no row at all
    put(ctx, n, rows)
    got, fits = one_round(ctx, n, params)
    assert list(got["n_used"][3:]) == [n - 1, 20, 0]
    assert list(got["status"]) == [L.OK] * 3 + [L.EMPTY] * 3
    assert len(fits[4][0]) == 0  # ls_fit says EMPTY as well
    assert np.array_equal(bits(got["params"][3:]), bits(params[3:]))
    # the three regressions with rows do not depend on the others being in the call
    alone, _ = one_round(ctx, n, params[:3])
    assert np.array_equal(bits(alone["params"]), bits(got["params"][:3]))


def _ill_scene(n=16):
    """three regressions; the rows of regression 2 have two nearly dependent columns: column 5 = column 2 + 2^-18 g
    (scaled by an exact power of two, as tests/linalg_families.py scales)"""
    rows, X, owner = mixture(n, 773, 3, 11)
    g = np.random.default_rng(12)
    sel = owner == 2
    rows[sel, 5] = rows[sel, 2] + F.scaled(g.normal(size=int(sel.sum())), -18)
    rows[sel, n] = rows[sel, :n] @ X[2] + SIGMA * g.normal(size=int(sel.sum()))
    return n, rows, X, sel


def test_one_round_ill_conditioned_model_takes_the_double_double_route(ctx):
    n, rows, X, sel = _ill_scene()
    cond = np.linalg.cond(rows[sel, :n])
    # tests/test_gpu_dense_cond.py: from cond 1e5 the elimination is refused; up to 1e6 the bar against the oracle's
    # SVD pseudo-inverse is 1e-6, noisy right-hand side or not
    assert 1e5 <= cond <= 1e6
    put(ctx, n, rows)
    got, fits = one_round(ctx, n, X, rows, bar=1e-6)
    assert list(got["route"]) == [0, 0, 1] and [f[1] for f in fits] == [0, 0, 1]
    assert np.all(got["status"] == L.OK)


def test_one_round_without_dense_dd_reports_route_two(ctx):
    """Without the double-double route both sides solve model 2 from their Gram block alone.  The two blocks are the
    same sums in another order, so they differ by rounding, eps |G| times a small constant, and the solutions of the
    two normal equations by cond(G) = cond(A)^2 times that: the parity bound of model 2 here is 10 eps cond(A)^2
    (8e-4 at cond(A) = 6e5), not the 1e-6 of a well-conditioned system.  The other two models keep 1e-6."""
    n, rows, X, sel = _ill_scene()
    cond = np.linalg.cond(rows[sel, :n])
    put(ctx, n, rows)
    ctx.set_option("dense_dd", 0)
    try:
        got, fits = one_round(ctx, n, X, parity=[REL, REL, 10 * np.finfo(float).eps * cond * cond])
    finally:
        ctx.set_option("dense_dd", 1)
    assert list(got["route"]) == [0, 0, 2] and [f[1] for f in fits] == [0, 0, 2]


# ---- loop -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 9, 33, 64])
def test_loop_converges_to_a_fixed_point(ctx, n):
    N = 3 * L.assign_dense_chunk(n) + 5
    rows, X, _ = mixture(n, N, 3, 13)
    put(ctx, n, rows)
    got = ctx.refine_dense(perturbed(X, n, 14), max_rounds=20)
    assert got["converged"] and 1 <= got["rounds"] <= 20
    assert int(got["counts"].sum()) == N and np.array_equal(got["counts"], counts_of(got["labels"], 3))
    # the fixed point: the returned rows are the refit of the returned labels
    for m in range(3):
        ctx.set_mask((got["labels"] == m).astype(np.uint8))
        fit, info = ctx.ls_fit(use_mask=True)
        assert len(fit) == n and rel(got["params"][m], fit) < REL and got["route"][m] == info.reserved
        assert got["n_used"][m] == np.sum(got["labels"] == m)
    one_round(ctx, n, got["params"])
    again = ctx.assign_dense(got["params"])
    assert np.array_equal(again["labels"], got["labels"])


# ---- independence and determinism -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 33, 64])
def test_same_bits_twice_under_permutation_and_beside_a_busy_context(ctx, n):
    N = 3 * L.assign_dense_chunk(n) + 5
    rows, X, _ = mixture(n, N, 3, 15)
    start = perturbed(X, n, 16)
    put(ctx, n, rows)
    a = ctx.refine_dense(start, max_rounds=1)
    b = ctx.refine_dense(start, max_rounds=1)
    for key in ("params", "labels", "counts", "n_used", "route", "status"):
        assert np.array_equal(bits(a[key]), bits(b[key])), key
    # [A, B, C] and [C, A, B]: the rows permuted bit for bit, the labels relabelled (the scene has no tie)
    perm = [2, 0, 1]
    p = ctx.refine_dense(start[perm], max_rounds=1)
    assert np.array_equal(bits(p["params"]), bits(a["params"][perm]))
    relabel = np.array([1, 2, 0, -1])  # old label -> its place in the permuted call; -1 stays
    assert np.array_equal(p["labels"], relabel[a["labels"]])
    assert np.array_equal(p["n_used"], a["n_used"][perm])
    # a second context working on the same device meanwhile
    stop = threading.Event()
    with Context(0) as other:
        big, Xb, _ = mixture(n, 20000, 3, 17)
        put(other, n, big)

        def work():
            while not stop.is_set():
                other.refine_dense(Xb, max_rounds=2)

        th = threading.Thread(target=work)
        th.start()
        try:
            c = [ctx.refine_dense(start, max_rounds=1) for _ in range(3)]
        finally:
            stop.set()
            th.join()
    for r in c:
        assert np.array_equal(bits(r["params"]), bits(a["params"])) and np.array_equal(r["labels"], a["labels"])


# ---- device checks --------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(ctx):
    lib = L.load()
    n = 8
    rows, X, _ = mixture(n, 300, 3, 18)
    put(ctx, n, rows)
    params = np.ascontiguousarray(X).copy()
    keep = params.copy()
    labels = np.full(300, 42, dtype=np.int32)
    counts = np.full(4, 42, dtype=np.uint64)
    status = np.full(3, 42, dtype=np.int32)
    fits = (L.FitInfo * 3)()
    C.memset(fits, 0x5A, C.sizeof(fits))
    rounds, conv = C.c_size_t(42), C.c_int(42)

    def refine(h=ctx._h, params_=params, m=3, fits_=fits, status_=status, rounds_=C.byref(rounds),
               conv_=C.byref(conv)):
        return lib.lsqr_refine_dense(h, L.ptr(params_), m, 4, 0, L.ptr(labels), L.ptr(counts), fits_, L.ptr(status_),
                                     rounds_, conv_)

    def assign(h=ctx._h, params_=params, m=3, labels_=labels):
        return lib.lsqr_assign_dense(h, L.ptr(params_), m, 0, L.ptr(labels_), None, L.ptr(counts))

    def untouched():
        return (np.array_equal(bits(params), bits(keep)) and np.all(labels == 42) and np.all(counts == 42)
                and np.all(status == 42) and bytes(fits) == b"\x5a" * C.sizeof(fits) and rounds.value == 42
                and conv.value == 42)

    assert refine(params_=None) == L.ERR_INVALID and untouched()
    assert refine(fits_=None) == L.ERR_INVALID and untouched()
    assert refine(status_=None) == L.ERR_INVALID and untouched()
    assert refine(rounds_=None) == L.ERR_INVALID and untouched()
    assert refine(conv_=None) == L.ERR_INVALID and untouched()
    assert refine(m=65) == L.ERR_INVALID and untouched()
    assert refine(m=0) == L.OK and untouched()
    assert assign(params_=None) == L.ERR_INVALID and untouched()
    assert assign(labels_=None) == L.ERR_INVALID and untouched()
    assert assign(m=0) == L.OK and untouched()
    # the order: the model before the count, the count before the pointers, the pointers before the records
    with Context(0) as empty:
        assert assign(h=empty._h) == L.ERR_STATE and refine(h=empty._h) == L.ERR_STATE  # no model set
        empty.set_model(L.PLANE, 3, 0.5)
        assert assign(h=empty._h, m=0) == L.ERR_INVALID and refine(h=empty._h, m=0) == L.ERR_INVALID  # not dense
        empty.set_model(L.DENSE, n, DELTA)
        assert assign(h=empty._h, m=0) == L.OK and assign(h=empty._h, m=65) == L.ERR_INVALID
        assert assign(h=empty._h, params_=None) == L.ERR_INVALID and refine(h=empty._h, fits_=None) == L.ERR_INVALID
        assert assign(h=empty._h) == L.ERR_STATE and refine(h=empty._h) == L.ERR_STATE  # no records
        assert untouched()
    # lsqr_assign / lsqr_refine keep refusing the dense model
    assert lib.lsqr_assign(ctx._h, L.ptr(params), 3, 0, L.ptr(labels), None, L.ptr(counts)) == L.ERR_INVALID
    assert lib.lsqr_refine(ctx._h, L.ptr(params), 3, 4, 0, L.ptr(labels), L.ptr(counts), fits, L.ptr(status),
                           C.byref(rounds), C.byref(conv)) == L.ERR_INVALID
    assert untouched()
    for model, dim in ((L.PLANE, 3), (L.SPHERE, 3), (L.LINE2D, 2), (L.ABSOR, 3)):  # and these refuse every other model
        with Context(0) as c2:
            c2.set_model(model, dim, 0.5, L.LS_ALGEBRAIC).upload(np.zeros((8, c2.ND)))
            assert assign(h=c2._h) == L.ERR_INVALID and refine(h=c2._h) == L.ERR_INVALID and untouched()
    # optional outputs may be absent
    assert lib.lsqr_refine_dense(ctx._h, L.ptr(params), 3, 1, 0, None, None, fits, L.ptr(status), C.byref(rounds),
                                 C.byref(conv)) == L.OK
    assert rounds.value == 1 and np.all(status == L.OK)


def test_context_is_untouched(ctx):
    n = 8
    rows, X, _ = mixture(n, 5000, 3, 19)
    put(ctx, n, rows)
    ctx.hypotheses_sample(7, 0, 256)
    ctx.scan()
    hyp_before = ctx.hypotheses()
    mask_before, cnt_before = ctx.mask(X[1])
    index_before = ctx.index_info()
    out = ctx.refine_dense(perturbed(X, n, 20))
    assert out["rounds"] >= 1
    fit_after, _ = ctx.ls_fit(use_mask=True)  # the mask of X[1] is still there
    assert ctx.index_info() == index_before
    for a, b in zip(hyp_before, ctx.hypotheses()):
        assert np.array_equal(bits(a), bits(b))
    ctx.mask(X[1])
    fit_want, _ = ctx.ls_fit(use_mask=True)
    assert cnt_before == mask_before.sum() and len(fit_want) == n
    assert np.array_equal(bits(fit_after), bits(fit_want))
