"""lsqr_assign / lsqr_refine (csrc/assign.h) through Context.assign / Context.refine.

assign: labels and residuals bit-equal to the numpy argmin over Context.residuals(row_m) masked by Context.mask(row_m)
(first minimum), the masks pinned to the oracle's scan; bit-equal to lsqr_assign_host record by record.
refine: round by round against the host loop (Context.assign, then per model set_mask(labels == m) + ls_fit(use_mask)):
the two differ in the fit origin and the summation tree only, so parameters at rtol 1e-9 / atol 1e-8 (the tolerance of
the sequential tests) and -- on scenes where no record sits within 1e-6 of a decision, which is asserted -- equal labels.
Refitted models are pinned to the oracle's least squares at 1e-6 relative (the README's fit tolerance)."""
import ctypes as C

import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd import synth
from lsqrrecipes_amd.context import Context
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu
P = 0.999
SMALL, LARGE = 300, 70_001  # below one chunk of the pass (2048 records) / several chunks, odd tail
EDGES = (1, 2047, 2048, 2049, 4096, 4097)  # prefixes of the LARGE scene that end at, before and after a chunk's end
MARGIN = 1e-6               # no record of a refine scene is this close to a decision
REL = 1e-6                  # the README's fit tolerance

# name -> (model, dim, delta, ls_type, planted(n, seed) -> inliers of one model, clutter(n, seed))
MODELS = {
    "plane": (L.PLANE, 3, 0.5, L.LS_ALGEBRAIC,
              lambda n, s: synth.plane(n, 0.0, seed=s, sigma=0.1)[0], lambda n, s: synth.plane(n, 1.0, seed=s)[0]),
    "line": (L.LINE, 3, 0.5, L.LS_ALGEBRAIC,
             lambda n, s: synth.line(n, 0.0, seed=s, sigma=0.1)[0], lambda n, s: synth.line(n, 1.0, seed=s)[0]),
    "sphere": (L.SPHERE, 3, 0.5, L.LS_ALGEBRAIC,
               lambda n, s: synth.sphere(n, 0.0, seed=s, sigma=0.1)[0], lambda n, s: synth.sphere(n, 1.0, seed=s)[0]),
    "plane5": (L.PLANE, 5, 0.5, L.LS_ALGEBRAIC,
               lambda n, s: synth.plane(n, 0.0, seed=s, dim=5, sigma=0.1)[0],
               lambda n, s: synth.plane(n, 1.0, seed=s, dim=5)[0]),
}
CASES = [(name, n) for name in MODELS for n in (SMALL, LARGE)]
_scenes, _starts = {}, {}


def scene(name, n):
    """three planted models of 30 % each plus clutter, shuffled with a fixed permutation; computed once, never changed"""
    if (name, n) not in _scenes:
        planted, clutter = MODELS[name][4], MODELS[name][5]
        m = (3 * n) // 10
        parts = [planted(m, 0x53000 + 7 * j) for j in range(3)] + [clutter(n - 3 * m, 0x53999)]
        data = np.ascontiguousarray(np.vstack(parts)[np.random.default_rng(12345).permutation(n)])
        data.setflags(write=False)
        _scenes[name, n] = data
    return _scenes[name, n]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _setup(ctx, name, ls_type=None):
    model, dim, delta, ls = MODELS[name][:4]
    ctx.set_model(model, dim, delta, ls if ls_type is None else ls_type)
    return ctx


def start(ctx, name, n):
    """the scene on the context and the three models ransac_sequential finds in it (computed once per scene)"""
    data = scene(name, n)
    _setup(ctx, name).upload(data)
    if (name, n) not in _starts:
        ctx.set_option("max_iterations", 20000)
        try:
            res = ctx.ransac_sequential(P, 4, seeds=11 + 3 * np.arange(4, dtype=np.uint64), min_votes=n // 10)
        finally:
            ctx.set_option("max_iterations", 0)
        assert res["n_models"] == 3, (res["n_models"], res["status"], res["best_votes"])
        rows = res["params"][:3].copy()
        rows.setflags(write=False)
        _starts[name, n] = rows
    return data, _starts[name, n]


def host_assign(ctx, rows):
    """the parent's entry points: M residual passes, M mask passes, a numpy argmin (first minimum)
    -> labels, residuals, masks, masked residual matrix"""
    res = np.array([ctx.residuals(r) for r in rows])
    masks = np.array([ctx.mask(r)[0] for r in rows])
    masked = np.where(masks != 0, res, np.inf)
    labels = np.where(masks.any(axis=0), np.argmin(masked, axis=0), -1).astype(np.int32)
    return labels, masked.min(axis=0), masks, masked


def counts_of(labels, m):
    return np.array([np.sum(labels == k) for k in range(m)] + [np.sum(labels == -1)], dtype=np.uint64)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- assign ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", CASES)
def test_assign_equals_argmin_of_the_parents_passes(ctx, name, n):
    data, rows = start(ctx, name, n)
    got = ctx.assign(rows, want_residuals=True)
    labels, res, masks, _ = host_assign(ctx, rows)
    oc = O.cfg(MODELS[name][0], MODELS[name][1], MODELS[name][2], O.LS_ALGEBRAIC)
    for m, row in enumerate(rows):
        assert np.array_equal(masks[m], O.scan(oc, row, data)[1]), m
    assert np.array_equal(got["labels"], labels)
    assert np.array_equal(bits(got["residuals"]), bits(res))
    assert np.array_equal(got["counts"], counts_of(labels, 3))
    assert set(np.unique(labels)) == {-1, 0, 1, 2} and got["residuals"].dtype == np.float64
    plain = ctx.assign(rows)
    assert plain["residuals"] is None and np.array_equal(plain["labels"], labels)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_assign_equals_the_host_call_record_by_record(ctx, name):
    data, rows = start(ctx, name, SMALL)
    model, dim, delta, ls = MODELS[name][:4]
    # a wide band as well: most records then agree with several models and the residual decides
    for d in (delta, 400.0):
        ctx.set_model(model, dim, d, ls).upload(data)
        got = ctx.assign(rows, want_residuals=True)
        cfg = L.ModelCfg(model, dim, d, ls, 0, 0.0)
        label, res = C.c_int32(0), C.c_double(0.0)
        flat = np.ascontiguousarray(rows)
        for i, x in enumerate(data):
            rec = np.ascontiguousarray(x)
            assert L.load().lsqr_assign_host(C.byref(cfg), L.ptr(flat), 3, L.ptr(rec), C.byref(label),
                                             C.byref(res)) == L.OK
            assert got["labels"][i] == label.value and bits(got["residuals"][i:i + 1]).tolist() == bits(
                np.array([res.value])).tolist(), (d, i)
        if d == 400.0:
            masks = np.array([ctx.mask(r)[0] for r in rows])
            assert np.sum(masks.sum(axis=0) > 1) > SMALL // 10
            assert np.array_equal(got["labels"], host_assign(ctx, rows)[0])


@pytest.mark.parametrize("n", EDGES)
@pytest.mark.parametrize("name", ["plane", "plane5"])
def test_assign_at_the_chunk_edges_equals_the_host_call(ctx, name, n):
    """a last chunk of 1, 2047 and 2048 records, in one, two and three chunks: every record against lsqr_assign_host"""
    rows = start(ctx, name, LARGE)[1]
    data = scene(name, LARGE)[:n]
    model, dim, delta, ls = MODELS[name][:4]
    _setup(ctx, name).upload(data)
    got = ctx.assign(rows, want_residuals=True)
    cfg = L.ModelCfg(model, dim, delta, ls, 0, 0.0)
    label, res = C.c_int32(0), C.c_double(0.0)
    flat = np.ascontiguousarray(rows)
    labels, residuals = np.empty(n, dtype=np.int32), np.empty(n)
    for i, x in enumerate(data):
        rec = np.ascontiguousarray(x)
        assert L.load().lsqr_assign_host(C.byref(cfg), L.ptr(flat), 3, L.ptr(rec), C.byref(label), C.byref(res)) == L.OK
        labels[i], residuals[i] = label.value, res.value
    assert np.array_equal(got["labels"], labels)
    assert np.array_equal(bits(got["residuals"]), bits(residuals))
    assert np.array_equal(got["counts"], counts_of(labels, 3))


class DeviceArray:
    """a device allocation of the HIP runtime the library itself runs on, with the handful of tensor attributes
    Context looks at (data_ptr, is_cuda, dtype, is_contiguous, numel): the device-pointer forms need no more"""
    _hip = None

    @classmethod
    def hip(cls):
        if cls._hip is None:
            L.load()
            path = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln][0]
            cls._hip = C.CDLL(path)  # (already loaded: the same runtime, the same device context)
        return cls._hip

    def __init__(self, host):
        self.host = np.ascontiguousarray(host)
        self.dtype, self.is_cuda = str(self.host.dtype), True
        p = C.c_void_p()
        assert self.hip().hipMalloc(C.byref(p), C.c_size_t(self.host.nbytes)) == 0
        self.ptr = p
        self.put(self.host)

    def put(self, host):
        assert self.hip().hipMemcpy(self.ptr, C.c_void_p(host.ctypes.data), C.c_size_t(host.nbytes), 1) == 0

    def get(self):
        out = np.empty_like(self.host)
        assert self.hip().hipMemcpy(C.c_void_p(out.ctypes.data), self.ptr, C.c_size_t(out.nbytes), 2) == 0
        return out

    def free(self):
        if self.ptr:
            self.hip().hipFree(self.ptr)
            self.ptr = None

    def data_ptr(self):
        return self.ptr.value

    def is_contiguous(self):
        return True

    def numel(self):
        return self.host.size


def test_device_labels_and_strided_attach(ctx):
    data, rows = start(ctx, "plane", LARGE)
    host = ctx.assign(rows, want_residuals=True)
    ref_host = ctx.refine(rows, max_rounds=2)
    lab = DeviceArray(np.full(LARGE, -9, dtype=np.int32))
    wide = np.full((LARGE, 4), -7.25)
    wide[:, :3] = data
    t = DeviceArray(wide)
    try:
        dev = ctx.assign(rows, labels_out=lab)
        assert dev["labels"] is lab and np.array_equal(lab.get(), host["labels"])
        assert np.array_equal(dev["counts"], host["counts"])
        lab.put(np.full(LARGE, -9, dtype=np.int32))
        ref_dev = ctx.refine(rows, max_rounds=2, labels_out=lab)
        assert ref_dev["labels"] is lab and np.array_equal(lab.get(), ref_host["labels"])
        assert np.array_equal(bits(ref_dev["params"]), bits(ref_host["params"]))
        with pytest.raises(ValueError):
            ctx.assign(rows, labels_out=DeviceArray(np.zeros(4, dtype=np.int64)))
        with pytest.raises(ValueError):
            ctx.assign(rows, labels_out=DeviceArray(np.zeros(LARGE - 1, dtype=np.int32)))
        with pytest.raises(ValueError):
            ctx.assign(rows, want_residuals=True, labels_out=lab)
        # the records at a stride of four doubles, attached: the same labels, residuals and refit, the buffer untouched
        ctx.attach(t.data_ptr(), LARGE, 32, keepalive=t)
        at = ctx.assign(rows, want_residuals=True)
        ref_at = ctx.refine(rows, max_rounds=2)
        ctx.synchronize()
        assert np.array_equal(at["labels"], host["labels"])
        assert np.array_equal(bits(at["residuals"]), bits(host["residuals"]))
        assert np.array_equal(bits(ref_at["params"]), bits(ref_host["params"]))
        assert np.array_equal(ref_at["labels"], ref_host["labels"]) and ref_at["rounds"] == ref_host["rounds"]
        assert np.array_equal(bits(t.get()), bits(wide))
    finally:
        ctx.upload(np.zeros((4, 3)))  # let go of the attached buffer
        ctx._keep = None
        lab.free()
        t.free()


def test_sixty_four_models_and_sixty_five(ctx):
    data, rows = start(ctx, "plane", LARGE)
    far = np.tile(rows, (22, 1))[:61].copy()
    far[:, 3:] += 1e7  # planes far from every record
    many = np.vstack([far[:20], rows[:1], far[20:40], rows[1:], far[40:]])  # the found planes at 20, 41 and 42
    where = {20: 0, 41: 1, 42: 2}
    base = ctx.assign(rows, want_residuals=True)
    got = ctx.assign(many, want_residuals=True)
    want = np.full(LARGE, -1, dtype=np.int32)
    for k, m in where.items():
        want[base["labels"] == m] = k
    assert np.array_equal(got["labels"], want)
    assert np.array_equal(bits(got["residuals"]), bits(base["residuals"]))
    assert np.array_equal(got["counts"], counts_of(want, 64))
    assert all(got["counts"][k] == 0 for k in range(64) if k not in where)
    # refine: the rows without records keep their bits and report EMPTY; the others are the three-model refit
    r3 = ctx.refine(rows, max_rounds=2)
    r64 = ctx.refine(many, max_rounds=2)
    assert r64["rounds"] == r3["rounds"] >= 1 and r64["converged"] == r3["converged"]
    for k in range(64):
        if k in where:
            m = where[k]
            assert r64["status"][k] == L.OK and r64["n_used"][k] == r3["n_used"][m]
            assert np.array_equal(bits(r64["params"][k]), bits(r3["params"][m]))
        else:
            assert r64["status"][k] == L.EMPTY and r64["n_used"][k] == 0
            assert np.array_equal(bits(r64["params"][k]), bits(many[k]))
    with pytest.raises(L.LsqrError) as e:
        ctx.assign(np.vstack([many, rows[:1]]))
    assert e.value.status == L.ERR_INVALID
    with pytest.raises(L.LsqrError) as e:
        ctx.refine(np.vstack([many, rows[:1]]))
    assert e.value.status == L.ERR_INVALID
    empty = ctx.assign(np.zeros((0, 6)))
    assert np.all(empty["labels"] == -1) and list(empty["counts"]) == [LARGE]


def test_geometric_sphere_assigns_but_does_not_refine(ctx):
    data, rows = start(ctx, "sphere", SMALL)
    alg = ctx.assign(rows, want_residuals=True)
    _setup(ctx, "sphere", L.LS_GEOMETRIC).upload(data)
    geo = ctx.assign(rows, want_residuals=True)
    assert np.array_equal(geo["labels"], alg["labels"]) and np.array_equal(bits(geo["residuals"]), bits(alg["residuals"]))
    keep = rows.copy()
    with pytest.raises(L.LsqrError) as e:
        ctx.refine(keep)
    assert e.value.status == L.ERR_INVALID
    assert b"lsqr_refine_lm" in ctx._lib.lsqr_last_error(ctx._h)
    ctx.set_model(L.ABSOR, 3, 2.0, 0)
    with pytest.raises(L.LsqrError) as e:
        ctx.assign(np.zeros((1, 7)))
    assert e.value.status == L.ERR_INVALID


def test_argument_errors_write_nothing(ctx):
    lib = L.load()
    data, rows = start(ctx, "plane", SMALL)
    params = np.ascontiguousarray(rows).copy()
    keep = params.copy()
    labels = np.full(SMALL, 42, dtype=np.int32)
    counts = np.full(4, 42, dtype=np.uint64)
    status = np.full(3, 42, dtype=np.int32)
    fits = (L.FitInfo * 3)()
    C.memset(fits, 0x5A, C.sizeof(fits))
    rounds, conv = C.c_size_t(42), C.c_int(42)

    def refine(params_=params, n=3, fits_=fits, status_=status, rounds_=C.byref(rounds), conv_=C.byref(conv)):
        return lib.lsqr_refine(ctx._h, L.ptr(params_), n, 4, 0, L.ptr(labels), L.ptr(counts), fits_, L.ptr(status_),
                               rounds_, conv_)

    def untouched():
        return (np.array_equal(bits(params), bits(keep)) and np.all(labels == 42) and np.all(counts == 42)
                and np.all(status == 42) and bytes(fits) == b"\x5a" * C.sizeof(fits) and rounds.value == 42
                and conv.value == 42)

    assert refine(params_=None) == L.ERR_INVALID and untouched()
    assert refine(fits_=None) == L.ERR_INVALID and untouched()
    assert refine(status_=None) == L.ERR_INVALID and untouched()
    assert refine(rounds_=None) == L.ERR_INVALID and untouched()
    assert refine(conv_=None) == L.ERR_INVALID and untouched()
    assert refine(n=65) == L.ERR_INVALID and untouched()
    assert refine(n=0) == L.OK and untouched()
    assert lib.lsqr_assign(ctx._h, None, 3, 0, L.ptr(labels), None, L.ptr(counts)) == L.ERR_INVALID and untouched()
    assert lib.lsqr_assign(ctx._h, L.ptr(params), 3, 0, None, None, L.ptr(counts)) == L.ERR_INVALID and untouched()
    assert lib.lsqr_assign(ctx._h, L.ptr(params), 0, 0, L.ptr(labels), None, L.ptr(counts)) == L.OK and untouched()
    with Context(0) as empty:  # no model / no records
        assert lib.lsqr_assign(empty._h, L.ptr(params), 3, 0, L.ptr(labels), None, L.ptr(counts)) == L.ERR_STATE
        empty.set_model(L.PLANE, 3, 0.5)
        assert lib.lsqr_assign(empty._h, L.ptr(params), 3, 0, L.ptr(labels), None, L.ptr(counts)) == L.ERR_STATE
        assert untouched()
    C.memset(fits, 0x5A, C.sizeof(fits))
    labels[:], counts[:], status[:] = 42, 42, 42
    rounds.value, conv.value = 42, 42
    params[:] = keep
    # optional outputs may be absent
    assert lib.lsqr_refine(ctx._h, L.ptr(params), 3, 1, 0, None, None, fits, L.ptr(status), C.byref(rounds),
                           C.byref(conv)) == L.OK
    assert rounds.value == 1 and np.all(status == L.OK)


# ---- refine ---------------------------------------------------------------------------------------------------------
def _blocks(name):
    model, dim = MODELS[name][:2]
    if model == L.SPHERE:
        return [(slice(0, dim + 1), False)]
    return [(slice(0, dim), True), (slice(dim, 2 * dim), False)]  # unit normal / direction, point


def assert_fit_close(name, got, want, what):
    """the README's fit tolerance, the sign of a unit vector normalised (as the fit tests do)"""
    for sl, unit in _blocks(name):
        g, w = np.asarray(got[sl]), np.asarray(want[sl])
        if unit:
            g = g * (np.sign(g @ w) or 1.0)
        tol = REL if unit else REL * max(1.0, np.abs(w).max())
        assert np.all(np.abs(g - w) <= tol), (what, got, want)


def host_round(ctx, name, rows):
    """one round of the host loop on the parent's entry points -> labels of `rows`, refitted rows, status, n_used.
    Asserts the scene condition: no record within MARGIN of delta, no record whose two smallest agreeing residuals
    are within MARGIN of each other."""
    labels = ctx.assign(rows)["labels"]
    _, _, masks, masked = host_assign(ctx, rows)
    delta = MODELS[name][2]
    res = np.array([ctx.residuals(r) for r in rows])
    assert np.min(np.abs(res - delta)) > MARGIN, "a record within 1e-6 of delta: choose another scene seed"
    two = np.sort(masked, axis=0)[:2]
    both = np.isfinite(two[1])
    assert not both.any() or np.min(two[1][both] - two[0][both]) > MARGIN, "a tie within 1e-6: choose another scene seed"
    new, status, used = np.array(rows, copy=True), [], []
    for m in range(len(rows)):
        mask = (labels == m).astype(np.uint8)
        used.append(int(mask.sum()))
        fit = np.zeros(0)
        if used[-1] >= ctx.K:
            ctx.set_mask(mask)
            fit, _ = ctx.ls_fit(use_mask=True)
        status.append(L.OK if len(fit) else L.EMPTY)
        if len(fit):
            new[m] = fit
    return labels, new, np.array(status), np.array(used)


def assert_rows_close(name, got, want, what):
    for m in range(len(want)):
        g = np.array(got[m])
        for sl, unit in _blocks(name):
            if unit:
                g[sl] *= (np.sign(g[sl] @ want[m][sl]) or 1.0)
        assert np.allclose(g, want[m], rtol=1e-9, atol=1e-8), (what, m, got[m], want[m])


@pytest.mark.parametrize("name,n", CASES)
def test_refine_against_the_host_loop_round_by_round(ctx, name, n):
    data, rows0 = start(ctx, name, n)
    oc = O.cfg(MODELS[name][0], MODELS[name][1], MODELS[name][2], O.LS_ALGEBRAIC)
    rows, prev = np.array(rows0), None
    r, max_rounds, converged = 0, 8, False
    while True:
        labels, new, status, used = host_round(ctx, name, rows)  # L_r of params_r, and params_{r+1}
        got = ctx.refine(rows0, max_rounds=r)
        print("%s n=%d round %d: counts %s changed %s" % (
            name, n, r, list(got["counts"]), None if prev is None else int(np.sum(prev != labels))))
        assert got["rounds"] == r and np.array_equal(got["labels"], labels), r
        assert_rows_close(name, got["params"], rows, "round %d" % r)
        assert np.array_equal(got["counts"], counts_of(labels, 3))
        if r > 0:
            assert np.array_equal(got["status"], last_status) and np.array_equal(got["n_used"], last_used), r
            for m in range(3):  # the oracle's least squares on the labelling the last refit used
                assert_fit_close(name, got["params"][m], O.ls(oc, data, (prev == m).astype(np.uint8)), (r, m))
        else:
            assert np.all(got["status"] == L.OK) and not np.any(got["n_used"])
            assert np.array_equal(bits(got["params"]), bits(rows0)) and not got["converged"]
        if r > 0 and np.array_equal(labels, prev):
            converged = True
            assert got["converged"]
            break
        if r == max_rounds:
            break
        assert r == 0 or not got["converged"]
        rows, prev, last_status, last_used = new, labels, status, used
        r += 1
    # the whole call: the same stop, and the labels are the assignment of the returned rows
    full = ctx.refine(rows0)
    assert full["rounds"] == r and full["converged"] == converged
    assert np.array_equal(full["labels"], labels)
    assert_rows_close(name, full["params"], rows, "full")
    assert r >= 1 and np.all(full["status"] == L.OK)


@pytest.mark.parametrize("n", [2049, 4096])
def test_refine_at_the_chunk_edges_against_the_host_loop(ctx, n):
    """a last chunk of one record and of 2048: the rounds of max_rounds = 2 against the host loop, as the test above
    (both prefixes of the scene meet host_round's MARGIN condition, which it asserts)"""
    rows0 = start(ctx, "plane", LARGE)[1]
    _setup(ctx, "plane").upload(scene("plane", LARGE)[:n])
    rows, prev = np.array(rows0), None
    for r in range(3):  # (rows: params_r; left at the last round's when the loop ends)
        labels, new, status, used = host_round(ctx, "plane", rows)
        got = ctx.refine(rows0, max_rounds=r)
        assert got["rounds"] == r and np.array_equal(got["labels"], labels), r
        assert_rows_close("plane", got["params"], rows, "round %d" % r)
        assert np.array_equal(got["counts"], counts_of(labels, 3))
        if r > 0:
            assert np.array_equal(got["status"], last_status) and np.array_equal(got["n_used"], last_used), r
        assert got["converged"] == (r > 0 and np.array_equal(labels, prev))
        if got["converged"] or r == 2:
            break
        rows, prev, last_status, last_used = new, labels, status, used
    assert r >= 1
    full = ctx.refine(rows0, max_rounds=2)
    assert full["rounds"] == r and np.array_equal(full["labels"], labels)
    assert_rows_close("plane", full["params"], rows, "full")


@pytest.mark.parametrize("name,n", CASES)
def test_refine_invariants(ctx, name, n):
    data, rows0 = start(ctx, name, n)
    for max_rounds in (1, 8):
        a = ctx.refine(rows0, max_rounds=max_rounds)
        b = ctx.refine(rows0, max_rounds=max_rounds)
        assert a["rounds"] == b["rounds"] and a["converged"] == b["converged"]
        assert np.array_equal(bits(a["params"]), bits(b["params"])) and np.array_equal(a["labels"], b["labels"])
        again = ctx.assign(a["params"])
        assert np.array_equal(again["labels"], a["labels"]) and np.array_equal(again["counts"], a["counts"])
        assert (max_rounds == 1 and a["rounds"] == 1) or a["converged"]
        assert np.all(a["n_used"] >= ctx.K) and np.all(a["status"] == L.OK)
    # a model with fewer than K records keeps its row and reports EMPTY; the others do not depend on it
    lone = np.array(rows0[0])
    if MODELS[name][0] == L.SPHERE:
        lone[:3] += 1e7
    else:
        lone[MODELS[name][1]:] += 1e7
    four = np.vstack([rows0, lone])
    c = ctx.refine(four, max_rounds=8)
    assert c["status"][3] == L.EMPTY and c["n_used"][3] == 0 and np.array_equal(bits(c["params"][3]), bits(lone))
    assert np.array_equal(bits(c["params"][:3]), bits(a["params"])) and np.array_equal(c["labels"], a["labels"])


def test_context_is_untouched(ctx):
    data, rows = start(ctx, "plane", LARGE)
    before = ctx.ransac(P, seed=9)
    mask_before, cnt_before = ctx.mask(rows[1])
    out = ctx.refine(rows)
    assert out["rounds"] >= 1
    fit_after, _ = ctx.ls_fit(use_mask=True)  # the mask of rows[1], and its point as the fit origin, are still there
    ctx.mask(rows[1])
    fit_want, _ = ctx.ls_fit(use_mask=True)
    assert cnt_before == mask_before.sum() and np.array_equal(bits(fit_after), bits(fit_want))
    after = ctx.ransac(P, seed=9)
    assert before["status"] == after["status"] == L.OK
    assert np.array_equal(before["consensus"], after["consensus"])
    assert np.array_equal(bits(before["params"]), bits(after["params"]))
    for key in ("fraction", "iterations", "best_index", "best_votes", "n_params"):
        assert getattr(before["info"], key) == getattr(after["info"], key), key
