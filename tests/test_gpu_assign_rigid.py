"""lsqr_assign_rigid / lsqr_refine_rigid (csrc/assign_rigid.h) through Context.assign_rigid / Context.refine_rigid:
absolute orientation (plain and weighted), pivot calibration and ray intersection.

assign: labels and residuals bit-equal to the numpy argmin over Context.residuals(row_m) masked by Context.mask(row_m)
(first minimum), the masks pinned to the oracle's scan; bit-equal to lsqr_assign_rigid_host record by record.
refine: round by round against the host loop (Context.assign_rigid, then per model set_mask(labels == m) +
ls_fit(use_mask)): the two differ in the fit origin and the summation tree only, so parameters at rtol 1e-9 / atol 1e-8
(the tolerance of the sequential tests; the quaternion up to its sign) and -- on scenes where no record sits within 1e-6
of a decision, which is asserted -- equal labels.  Refitted models are pinned to the oracle's least squares at 1e-6
relative (the README's fit tolerance)."""
import ctypes as C

import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd import synth
from lsqrrecipes_amd.context import Context
from oracle import pyoracle as O
from test_gpu_assign import DeviceArray, bits, counts_of

pytestmark = pytest.mark.gpu
SMALL, LARGE = 300, 9001    # below one chunk of the pass / several chunks of either size (2048, 1024), odd tail
EDGES = (1, 2, 3, 1023, 1024, 1025, 2047, 2048, 2049, 4097)  # prefixes of the LARGE scene: the chunk ends of both sizes
MARGIN = 1e-6               # no record of a refine scene is this close to a decision
REL = 1e-6                  # the README's fit tolerance
AUX = 0.017453292519943295  # the ray estimator's parallelism threshold: not used by assign or refine
PIVOT_SHIFT = np.array([[0.0, 0.0, 0.0], [50.0, -45.0, 55.0], [-55.0, 50.0, -48.0]])


def _absor(n, s):
    rec, truth, _ = synth.absolute_orientation(n, 0.0, seed=s)
    return rec, truth


def _absor_w(n, s):
    rec, truth = _absor(n, s)
    w = np.random.default_rng(s).uniform(0.25, 4.0, (n, 1))
    return np.hstack([rec, w]), truth


def _pivot(n, s):
    """synth.pivot's tool, its translations -- and so its pivot point -- moved by one of three offsets"""
    rec, truth, _ = synth.pivot(n, 0.0, seed=s)
    shift = PIVOT_SHIFT[s % 3]
    rec[:, 9:12] += shift
    truth = truth.copy()
    truth[3:] += shift
    return rec, truth


def _rays(n, s):
    rec, truth, _ = synth.rays(n, 0.0, seed=s)
    return rec, truth


def _clutter_w(n, s):
    rec = synth.absolute_orientation(n, 1.0, seed=s)[0]
    return np.hstack([rec, np.random.default_rng(s).uniform(0.25, 4.0, (n, 1))])


# name -> (model, oracle model, delta, ls_type, aux, wide delta, planted(n, seed) -> (inliers of one model, its
# parameters), clutter(n, seed), first scene seed)
MODELS = {
    "absor": (L.ABSOR, O.ABSOR, 2.0, 0, 0.0, 4000.0, _absor,
              lambda n, s: synth.absolute_orientation(n, 1.0, seed=s)[0], 0x57000),
    "absor_w": (L.ABSOR, O.ABSOR, 2.0, 2, 0.0, 4000.0, _absor_w, _clutter_w, 0x57100),
    "pivot": (L.PIVOT, O.PIVOT, 1.0, 0, 0.0, 400.0, _pivot, lambda n, s: synth.pivot(n, 1.0, seed=s)[0], 0x57201),
    "ray": (L.RAY, O.RAY, 2.0, 0, AUX, 3000.0, _rays, lambda n, s: synth.rays(n, 1.0, seed=s)[0], 0x57300),
}
NAMES = list(MODELS)
CASES = [(name, n) for name in NAMES for n in (SMALL, LARGE)]
_scenes = {}


def scene(name, n):
    """three planted models of 30 % each plus clutter, shuffled with a fixed permutation, and the planted parameters
    (the start rows); computed once, never changed"""
    if (name, n) not in _scenes:
        planted, clutter, seed = MODELS[name][6:9]
        m = (3 * n) // 10
        made = [planted(m, seed + 4 * j) for j in range(3)]  # (distinct seeds; mod 3 the pivot's offsets in turn)
        parts = [p[0] for p in made] + [clutter(n - 3 * m, seed + 0x99)]
        data = np.ascontiguousarray(np.vstack(parts)[np.random.default_rng(12345).permutation(n)])
        rows = np.ascontiguousarray([p[1] for p in made])
        data.setflags(write=False)
        rows.setflags(write=False)
        _scenes[name, n] = (data, rows)
    return _scenes[name, n]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _setup(ctx, name, delta=None):
    model, _, d, ls, aux = MODELS[name][:5]
    return ctx.set_model(model, 3, d if delta is None else delta, ls, aux=aux)


def _ocfg(name, delta=None):
    """the oracle decides absolute orientation's votes on the 6-double pairs (the weight only enters the fit)"""
    _, om, d, ls, aux = MODELS[name][:5]
    return O.cfg(om, 3, d if delta is None else delta, 0 if name == "absor_w" else ls, aux=aux)


def _orec(name, data):
    return np.ascontiguousarray(data[:, :6]) if name == "absor_w" else data


def _ols(name, data, mask):
    if name == "absor_w":
        m = np.asarray(mask, dtype=bool)
        return O.absor_weighted_ls(np.ascontiguousarray(data[m, :6]), np.ascontiguousarray(data[m, 6]))
    return O.ls(_ocfg(name), data, mask)


def host_assign(ctx, rows):
    """the parent's entry points: M residual passes, M mask passes, a numpy argmin (first minimum)
    -> labels, residuals, masks, masked residual matrix"""
    res = np.array([ctx.residuals(r) for r in rows])
    masks = np.array([ctx.mask(r)[0] for r in rows])
    masked = np.where(masks != 0, res, np.inf)
    labels = np.where(masks.any(axis=0), np.argmin(masked, axis=0), -1).astype(np.int32)
    return labels, masked.min(axis=0), masks, masked


def host_call(name, rows, data, delta=None):
    """lsqr_assign_rigid_host record by record -> labels, residuals"""
    model, _, d, ls, aux = MODELS[name][:5]
    cfg = L.ModelCfg(model, 3, d if delta is None else delta, ls, 0, aux)
    fn = L.load().lsqr_assign_rigid_host
    flat = np.ascontiguousarray(rows)
    label, res = C.c_int32(0), C.c_double(0.0)
    labels, residuals = np.empty(len(data), dtype=np.int32), np.empty(len(data))
    for i, x in enumerate(data):
        rec = np.ascontiguousarray(x)
        assert fn(C.byref(cfg), L.ptr(flat), len(flat), L.ptr(rec), C.byref(label), C.byref(res)) == L.OK
        labels[i], residuals[i] = label.value, res.value
    return labels, residuals


# ---- assign ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", CASES)
def test_assign_equals_argmin_of_the_parents_passes(ctx, name, n):
    data, rows = scene(name, n)
    _setup(ctx, name).upload(data)
    got = ctx.assign_rigid(rows, want_residuals=True)
    labels, res, masks, _ = host_assign(ctx, rows)
    for m, row in enumerate(rows):
        assert np.array_equal(masks[m], O.scan(_ocfg(name), row, _orec(name, data))[1]), m
    assert np.array_equal(got["labels"], labels)
    assert np.array_equal(bits(got["residuals"]), bits(res))
    assert np.array_equal(got["counts"], counts_of(labels, 3))
    assert set(np.unique(labels)) == {-1, 0, 1, 2} and got["residuals"].dtype == np.float64
    assert np.all(got["counts"][:3] >= (3 * n) // 10 - n // 50)  # the planted records, but for a few in the noise's tail
    plain = ctx.assign_rigid(rows)
    assert plain["residuals"] is None and np.array_equal(plain["labels"], labels)


@pytest.mark.parametrize("name", NAMES)
def test_assign_equals_the_host_call_record_by_record(ctx, name):
    data, rows = scene(name, SMALL)
    # a wide band as well: most records then agree with several models and the residual decides
    for d in (MODELS[name][2], MODELS[name][5]):
        _setup(ctx, name, d).upload(data)
        got = ctx.assign_rigid(rows, want_residuals=True)
        labels, res = host_call(name, rows, data, d)
        assert np.array_equal(got["labels"], labels) and np.array_equal(bits(got["residuals"]), bits(res)), d
        want, wres, masks, _ = host_assign(ctx, rows)
        assert np.array_equal(got["labels"], want) and np.array_equal(bits(got["residuals"]), bits(wres)), d
        for m, row in enumerate(rows):
            assert np.array_equal(masks[m], O.scan(_ocfg(name, d), row, _orec(name, data))[1]), (d, m)
        if d == MODELS[name][5]:
            assert np.sum(masks.sum(axis=0) > 1) > SMALL // 10
            assert len(set(labels.tolist())) >= 3


@pytest.mark.parametrize("n", EDGES)
@pytest.mark.parametrize("name", NAMES)
def test_assign_at_the_chunk_edges(ctx, name, n):
    """a last chunk of 1, 1023 / 2047 and 1024 / 2048 records, in one to five chunks: the argmin of the parent's passes,
    at the scene's delta and at the wide one"""
    full, rows = scene(name, LARGE)
    data = full[:n]
    for d in (MODELS[name][2], MODELS[name][5]):
        _setup(ctx, name, d).upload(data)
        got = ctx.assign_rigid(rows, want_residuals=True)
        labels, res, _, _ = host_assign(ctx, rows)
        assert np.array_equal(got["labels"], labels), d
        assert np.array_equal(bits(got["residuals"]), bits(res)), d
        assert np.array_equal(got["counts"], counts_of(labels, 3)), d


@pytest.mark.parametrize("name", NAMES)
def test_wide_band_on_the_large_scene(ctx, name):
    data, rows = scene(name, LARGE)
    _setup(ctx, name, MODELS[name][5]).upload(data)
    got = ctx.assign_rigid(rows, want_residuals=True)
    labels, res, masks, _ = host_assign(ctx, rows)
    assert np.sum(masks.sum(axis=0) > 1) > LARGE // 10
    assert np.array_equal(got["labels"], labels) and np.array_equal(bits(got["residuals"]), bits(res))
    assert np.array_equal(got["counts"], counts_of(labels, 3))


@pytest.mark.parametrize("name", NAMES)
def test_device_labels_equal_the_host_form(ctx, name):
    data, rows = scene(name, LARGE)
    _setup(ctx, name).upload(data)
    host = ctx.assign_rigid(rows)
    ref_host = ctx.refine_rigid(rows, max_rounds=2)
    lab = DeviceArray(np.full(LARGE, -9, dtype=np.int32))
    try:
        dev = ctx.assign_rigid(rows, labels_out=lab)
        assert dev["labels"] is lab and np.array_equal(lab.get(), host["labels"])
        assert np.array_equal(dev["counts"], host["counts"])
        lab.put(np.full(LARGE, -9, dtype=np.int32))
        ref_dev = ctx.refine_rigid(rows, max_rounds=2, labels_out=lab)
        assert ref_dev["labels"] is lab and np.array_equal(lab.get(), ref_host["labels"])
        assert np.array_equal(bits(ref_dev["params"]), bits(ref_host["params"]))
        with pytest.raises(ValueError):
            ctx.assign_rigid(rows, want_residuals=True, labels_out=lab)
    finally:
        lab.free()


def test_sixty_four_models_and_sixty_five(ctx):
    data, rows = scene("ray", LARGE)
    _setup(ctx, "ray").upload(data)
    far = np.tile(rows, (22, 1))[:61] + 1e7  # points far from every ray
    many = np.vstack([far[:20], rows[:1], far[20:40], rows[1:], far[40:]])  # the planted points at 20, 41 and 42
    where = {20: 0, 41: 1, 42: 2}
    base = ctx.assign_rigid(rows, want_residuals=True)
    got = ctx.assign_rigid(many, want_residuals=True)
    want = np.full(LARGE, -1, dtype=np.int32)
    for k, m in where.items():
        want[base["labels"] == m] = k
    assert np.array_equal(got["labels"], want)
    assert np.array_equal(bits(got["residuals"]), bits(base["residuals"]))
    assert np.array_equal(got["counts"], counts_of(want, 64))
    r3 = ctx.refine_rigid(rows, max_rounds=2)
    r64 = ctx.refine_rigid(many, max_rounds=2)
    assert r64["rounds"] == r3["rounds"] >= 1 and r64["converged"] == r3["converged"]
    for k in range(64):
        if k in where:
            m = where[k]
            assert r64["status"][k] == L.OK and r64["n_used"][k] == r3["n_used"][m]
            assert np.array_equal(bits(r64["params"][k]), bits(r3["params"][m]))
        else:
            assert r64["status"][k] == L.EMPTY and r64["n_used"][k] == 0
            assert np.array_equal(bits(r64["params"][k]), bits(many[k]))
    for call in (ctx.assign_rigid, ctx.refine_rigid):
        with pytest.raises(L.LsqrError) as e:
            call(np.vstack([many, rows[:1]]))
        assert e.value.status == L.ERR_INVALID
    empty = ctx.assign_rigid(np.zeros((0, 3)))
    assert np.all(empty["labels"] == -1) and list(empty["counts"]) == [LARGE]


# ---- refine ---------------------------------------------------------------------------------------------------------
def _blocks(name):
    """(slice, a unit vector up to its sign?) of the parameter vector"""
    if name in ("absor", "absor_w"):
        return [(slice(0, 4), True), (slice(4, 7), False)]
    return [(slice(0, 3 if name == "ray" else 6), False)]


def assert_fit_close(name, got, want, what):
    """the README's fit tolerance, the quaternion's sign normalised (as the fit tests do)"""
    assert len(want) == len(got), (what, got, want)
    for sl, unit in _blocks(name):
        g, w = np.asarray(got[sl]), np.asarray(want[sl])
        if unit:
            g = g * (np.sign(g @ w) or 1.0)
        tol = REL if unit else REL * max(1.0, np.abs(w).max())
        assert np.all(np.abs(g - w) <= tol), (what, got, want)


def assert_rows_close(name, got, want, what):
    for m in range(len(want)):
        g = np.array(got[m])
        for sl, unit in _blocks(name):
            if unit:
                g[sl] *= (np.sign(g[sl] @ want[m][sl]) or 1.0)
        assert np.allclose(g, want[m], rtol=1e-9, atol=1e-8), (what, m, got[m], want[m])


def host_round(ctx, name, rows, data, skip=()):
    """one round of the host loop on the parent's entry points -> labels of `rows`, refitted rows, status, n_used.
    Asserts the scene condition: no record within MARGIN of delta, no record whose two smallest agreeing residuals are
    within MARGIN of each other, no ray within MARGIN of beginning at the foot of a point it is near.
    skip: records that are not finite, which decide nothing"""
    labels = ctx.assign_rigid(rows)["labels"]
    _, _, masks, masked = host_assign(ctx, rows)
    delta = MODELS[name][2]
    res = np.array([ctx.residuals(r) for r in rows])
    keep = np.ones(len(data), bool)
    keep[list(skip)] = False
    assert np.min(np.abs(res[:, keep] - delta)) > MARGIN, "a record within 1e-6 of delta: choose another scene seed"
    two = np.sort(masked, axis=0)[:2]
    both = np.isfinite(two[1])
    assert not both.any() or np.min(two[1][both] - two[0][both]) > MARGIN, "a tie within 1e-6: choose another scene seed"
    if name == "ray":
        for r, row in enumerate(rows):
            t = np.einsum("ij,ij->i", data[:, 3:6], row[:3] - data[:, :3])
            near = keep & (res[r] < delta + MARGIN)
            assert not near.any() or np.min(np.abs(t[near])) > MARGIN, "a ray that begins at the point's foot"
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


def check_rounds(ctx, name, data, rows0, max_rounds, skip=(), oracle=True):
    """refine_rigid(max_rounds = 0, 1, ...) against the host loop, round by round, on the context's upload `data`
    -> rounds, converged, the last call's dict"""
    rows, prev = np.array(rows0), None
    r, converged = 0, False
    nm = len(rows0)
    while True:
        labels, new, status, used = host_round(ctx, name, rows, data, skip)  # L_r of params_r, and params_{r+1}
        got = ctx.refine_rigid(rows0, max_rounds=r)
        print("%s n=%d round %d: counts %s changed %s" % (
            name, len(data), r, list(got["counts"]), None if prev is None else int(np.sum(prev != labels))))
        assert got["rounds"] == r and np.array_equal(got["labels"], labels), r
        assert_rows_close(name, got["params"], rows, "round %d" % r)
        assert np.array_equal(got["counts"], counts_of(labels, nm))
        if r > 0:
            assert np.array_equal(got["status"], last_status) and np.array_equal(got["n_used"], last_used), r
            for m in range(nm if oracle else 0):  # the oracle's least squares on the labelling the last refit used
                if last_status[m] == L.OK:
                    assert_fit_close(name, got["params"][m], _ols(name, data, (prev == m).astype(np.uint8)), (r, m))
        else:
            assert np.all(got["status"] == L.OK) and not np.any(got["n_used"])
            assert np.array_equal(bits(got["params"]), bits(rows0)) and not got["converged"]
            a = ctx.assign_rigid(rows0)
            assert np.array_equal(a["labels"], got["labels"]) and np.array_equal(a["counts"], got["counts"])
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
    full = ctx.refine_rigid(rows0, max_rounds=max_rounds)
    assert full["rounds"] == r and full["converged"] == converged
    assert np.array_equal(full["labels"], labels)
    assert_rows_close(name, full["params"], rows, "full")
    again = ctx.assign_rigid(full["params"])
    assert np.array_equal(again["labels"], full["labels"]) and np.array_equal(again["counts"], full["counts"])
    return r, converged, full


@pytest.mark.parametrize("name,n", CASES)
def test_refine_against_the_host_loop_round_by_round(ctx, name, n):
    data, rows0 = scene(name, n)
    _setup(ctx, name).upload(data)
    r, converged, full = check_rounds(ctx, name, data, rows0, 8)
    assert r >= 1 and converged and np.all(full["status"] == L.OK) and np.all(full["n_used"] >= ctx.K)


@pytest.mark.parametrize("name", NAMES)
def test_refine_from_rows_moved_off_the_planted_ones(ctx, name):
    """the translation / pivot point / point of every start row moved by 0.4, inside the band: the first refit moves
    the rows back and records change hands on the way"""
    data, rows0 = scene(name, LARGE)
    moved = rows0.copy()
    moved[:, -3:] += [0.4, -0.4, 0.4]
    _setup(ctx, name).upload(data)
    r, converged, full = check_rounds(ctx, name, data, moved, 8)
    assert r >= 1 and converged and np.all(full["status"] == L.OK)
    assert np.all(np.abs(full["params"][:, -3:] - rows0[:, -3:]) < 0.1)


@pytest.mark.parametrize("n", EDGES)
@pytest.mark.parametrize("name", NAMES)
def test_refine_at_the_chunk_edges_against_the_host_loop(ctx, name, n):
    """prefixes that end at, before and after a chunk's end, and prefixes of one to three records, whose models have
    fewer than lsqr_min_subset records: they keep their rows and report what the host loop reports"""
    full, rows0 = scene(name, LARGE)
    data = full[:n]
    _setup(ctx, name).upload(data)
    r, _, got = check_rounds(ctx, name, data, rows0, 2, oracle=n > 3)
    assert r >= 1
    if n <= 3:
        few = got["n_used"] < ctx.K
        assert np.all(got["status"][few] == L.EMPTY) and np.array_equal(bits(got["params"][few]), bits(rows0[few]))
        assert got["n_used"].sum() <= n


@pytest.mark.parametrize("name", NAMES)
def test_refine_invariants(ctx, name):
    data, rows0 = scene(name, LARGE)
    _setup(ctx, name).upload(data)
    for max_rounds in (1, 8):
        a = ctx.refine_rigid(rows0, max_rounds=max_rounds)
        b = ctx.refine_rigid(rows0, max_rounds=max_rounds)
        assert a["rounds"] == b["rounds"] and a["converged"] == b["converged"]
        assert np.array_equal(bits(a["params"]), bits(b["params"])) and np.array_equal(a["labels"], b["labels"])
        assert np.array_equal(a["n_used"], b["n_used"]) and np.array_equal(a["status"], b["status"])
        assert (max_rounds == 1 and a["rounds"] == 1) or a["converged"]
        assert np.all(a["n_used"] >= ctx.K) and np.all(a["status"] == L.OK)
    # the rows of the call permuted: the results permuted, bit for bit
    for perm in ([2, 0, 1], [1, 2, 0], [0, 2, 1]):
        p = ctx.refine_rigid(rows0[perm], max_rounds=8)
        assert p["rounds"] == a["rounds"] and p["converged"] == a["converged"]
        assert np.array_equal(bits(p["params"]), bits(a["params"][perm]))
        assert np.array_equal(p["n_used"], a["n_used"][perm]) and np.array_equal(p["counts"][:3], a["counts"][perm])
        back = np.where(p["labels"] >= 0, np.array(perm)[np.maximum(p["labels"], 0)], -1)
        assert np.array_equal(back, a["labels"])
    # a model nothing agrees with at entry keeps its row and reports EMPTY; the others do not depend on it, wherever
    # it stands (for absolute orientation it is the model without an origin)
    lone = np.array(rows0[0])
    lone[-3:] += 1e7
    for at in (0, 2, 3):
        four = np.insert(rows0, at, lone, axis=0)
        rest = [k for k in range(4) if k != at]
        c = ctx.refine_rigid(four, max_rounds=8)
        assert c["status"][at] == L.EMPTY and c["n_used"][at] == 0 and c["counts"][at] == 0
        assert np.array_equal(bits(c["params"][at]), bits(lone))
        assert np.array_equal(bits(c["params"][rest]), bits(a["params"])) and c["rounds"] == a["rounds"]
        assert np.array_equal(c["n_used"][rest], a["n_used"]) and np.all(c["status"][rest] == L.OK)
        assert np.array_equal(np.where(c["labels"] > at, c["labels"] - 1, c["labels"]), a["labels"])


@pytest.mark.parametrize("kind", ["outlier", "nan"])
@pytest.mark.parametrize("name", NAMES)
def test_first_record_an_outlier_or_not_finite(ctx, name, kind):
    """record 0 of the upload at 1e6 from everything, or NaN: it has no say in the other records' models"""
    data, rows0 = scene(name, LARGE)
    data = data.copy()
    nd = 12 if name == "pivot" else 6
    if kind == "nan":
        data[0, nd - 2] = np.nan
    else:
        data[0, :nd] += 1e6
    _setup(ctx, name).upload(data)
    lab0 = ctx.assign_rigid(rows0)["labels"][0]
    assert lab0 == -1
    r, converged, full = check_rounds(ctx, name, data, rows0, 8, skip=(0,) if kind == "nan" else ())
    assert r >= 1 and converged and np.all(full["status"] == L.OK) and full["labels"][0] == -1
    assert np.all(np.isfinite(full["params"]))


def test_weighted_record_with_a_weight_that_is_not_finite(ctx):
    """ls_type 2: the weight is one of the record's loaded slots -- NaN there gives -1; with ls_type 0 the same pairs
    are decided without it"""
    data, rows0 = scene("absor_w", SMALL)
    data = data.copy()
    base = _setup(ctx, "absor_w").upload(data).assign_rigid(rows0)["labels"]
    hit = np.flatnonzero(base >= 0)[:5]
    data[hit, 6] = [np.nan, np.inf, -np.inf, np.nan, np.nan]
    got = _setup(ctx, "absor_w").upload(data).assign_rigid(rows0, want_residuals=True)
    want = base.copy()
    want[hit] = -1
    assert np.array_equal(got["labels"], want) and np.all(np.isinf(got["residuals"][hit]))
    labels, res = host_call("absor_w", rows0, data)
    assert np.array_equal(got["labels"], labels) and np.array_equal(bits(got["residuals"]), bits(res))
    fit = ctx.refine_rigid(rows0, max_rounds=2)
    assert np.all(np.isfinite(fit["params"])) and np.all(fit["labels"][hit] == -1)
    plain = _setup(ctx, "absor").upload(np.ascontiguousarray(data[:, :6])).assign_rigid(rows0)["labels"]
    assert np.array_equal(plain, base)


# ---- rows that must keep their values ----------------------------------------------------------------------------------
def test_rays_that_are_all_parallel_keep_the_row(ctx):
    data, rows0 = scene("ray", SMALL)
    point = np.array([5000.0, -4000.0, 3000.0])  # far from the scene's rays
    g = np.random.default_rng(77)
    par = np.zeros((40, 6))
    par[:, :3] = point + np.c_[g.uniform(-0.5, 0.5, (40, 2)), -g.uniform(10.0, 900.0, 40)]
    par[:, 3:] = [0.0, 0.0, 1.0]
    both = np.vstack([data[:150], par, data[150:]])
    rows = np.vstack([rows0[:1], point, rows0[1:]])
    _setup(ctx, "ray").upload(both)
    a = ctx.assign_rigid(rows)
    assert a["counts"][1] == 40 and np.all(a["labels"][150:190] == 1)
    r = ctx.refine_rigid(rows, max_rounds=3)
    assert r["rounds"] >= 1 and r["status"][1] == L.EMPTY and r["n_used"][1] == 40 and r["counts"][1] == 40
    assert np.array_equal(bits(r["params"][1]), bits(point))
    assert np.all(r["status"][[0, 2, 3]] == L.OK) and np.all(r["n_used"][[0, 2, 3]] >= 60)
    # and the host loop says the same of these rays
    ctx.set_mask((a["labels"] == 1).astype(np.uint8))
    assert len(ctx.ls_fit(use_mask=True)[0]) == 0


def test_frames_that_are_all_the_same_keep_the_row(ctx):
    data, rows0 = scene("pivot", SMALL)
    row = np.array([3.0, -2.0, 7.0, 2003.0, -1502.0, 4007.0])  # tip, pivot point: far from the scene's
    frame = np.zeros(13)
    frame[[0, 4, 8]] = 1.0
    frame[9:12] = row[3:] - row[:3]   # R tip + t == pivot point, exactly
    both = np.vstack([data[:150], np.tile(frame, (40, 1)), data[150:]])
    rows = np.vstack([rows0[:2], row, rows0[2:]])
    _setup(ctx, "pivot").upload(both)
    a = ctx.assign_rigid(rows, want_residuals=True)
    assert a["counts"][2] == 40 and np.all(a["labels"][150:190] == 2) and np.all(a["residuals"][150:190] == 0.0)
    r = ctx.refine_rigid(rows, max_rounds=3)
    assert r["rounds"] >= 1 and r["status"][2] == L.EMPTY and r["n_used"][2] == 40 and r["counts"][2] == 40
    assert np.array_equal(bits(r["params"][2]), bits(row))
    assert np.all(r["status"][[0, 1, 3]] == L.OK) and np.all(r["n_used"][[0, 1, 3]] >= 60)
    ctx.set_mask((a["labels"] == 2).astype(np.uint8))
    assert len(ctx.ls_fit(use_mask=True)[0]) == 0


# ---- the context and the arguments ---------------------------------------------------------------------------------
def test_context_is_untouched(ctx):
    data, rows = scene("absor", LARGE)
    _setup(ctx, "absor").upload(data)
    before = ctx.ransac(0.999, seed=9)
    mask_before, cnt_before = ctx.mask(rows[1])
    fit_want, _ = ctx.ls_fit(use_mask=True)
    ctx.mask(rows[1])
    out = ctx.refine_rigid(rows)
    assert out["rounds"] >= 1
    fit_after, _ = ctx.ls_fit(use_mask=True)  # the mask of rows[1] is still there
    assert cnt_before == mask_before.sum() and np.array_equal(bits(fit_after), bits(fit_want))
    after = ctx.ransac(0.999, seed=9)
    assert before["status"] == after["status"] == L.OK
    assert np.array_equal(before["consensus"], after["consensus"])
    assert np.array_equal(bits(before["params"]), bits(after["params"]))
    for key in ("fraction", "iterations", "best_index", "best_votes", "n_params"):
        assert getattr(before["info"], key) == getattr(after["info"], key), key


def test_the_other_entry_points_keep_refusing_these_models(ctx):
    for name in NAMES:
        data, rows = scene(name, SMALL)
        _setup(ctx, name).upload(data)
        for call in (ctx.assign, ctx.refine, ctx.refine_lm, ctx.assign_dense, ctx.refine_dense):
            with pytest.raises(L.LsqrError) as e:
                call(rows)
            assert e.value.status == L.ERR_INVALID, (name, call)
        groups = np.zeros(SMALL, dtype=np.int32)
        for call in (ctx.assign_grouped, ctx.refine_grouped):
            with pytest.raises(L.LsqrError) as e:
                call(groups, 1, rows[None], np.array([3], dtype=np.uintp))
            assert e.value.status == L.ERR_INVALID, (name, call)


def test_argument_errors_write_nothing(ctx):
    lib = L.load()
    data, rows = scene("absor", SMALL)
    _setup(ctx, "absor").upload(data)
    params = np.ascontiguousarray(rows).copy()
    keep = params.copy()
    labels = np.full(SMALL, 42, dtype=np.int32)
    counts = np.full(4, 42, dtype=np.uint64)
    status = np.full(3, 42, dtype=np.int32)
    fits = (L.FitInfo * 3)()
    C.memset(fits, 0x5A, C.sizeof(fits))
    rounds, conv = C.c_size_t(42), C.c_int(42)

    def refine(h=None, params_=params, n=3, fits_=fits, status_=status, rounds_=C.byref(rounds), conv_=C.byref(conv)):
        return lib.lsqr_refine_rigid(ctx._h if h is None else h, L.ptr(params_), n, 4, 0, L.ptr(labels), L.ptr(counts),
                                     fits_, L.ptr(status_), rounds_, conv_)

    def assign(h=None, params_=params, n=3, labels_=labels):
        return lib.lsqr_assign_rigid(ctx._h if h is None else h, L.ptr(params_), n, 0, L.ptr(labels_), None,
                                     L.ptr(counts))

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
    assert assign(params_=None) == L.ERR_INVALID and untouched()
    assert assign(labels_=None) == L.ERR_INVALID and untouched()
    assert assign(n=65) == L.ERR_INVALID and untouched()
    assert assign(n=0) == L.OK and untouched()
    with Context(0) as other:  # no model / no records / every other model
        assert assign(h=other._h) == L.ERR_STATE and refine(h=other._h) == L.ERR_STATE and untouched()
        other.set_model(L.ABSOR, 3, 2.0, 0)
        assert assign(h=other._h) == L.ERR_STATE and refine(h=other._h) == L.ERR_STATE and untouched()
        for model, dim, ls in ((L.PLANE, 3, 0), (L.LINE, 3, 0), (L.SPHERE, 3, L.LS_ALGEBRAIC),
                               (L.SPHERE, 3, L.LS_GEOMETRIC), (L.LINE2D, 2, 0), (L.DENSE, 6, 0),
                               (L.US_SINGLE, 0, L.LS_ANALYTIC), (L.US_POINTER, 0, L.LS_ANALYTIC), (L.PHANTOM, 0, 0),
                               (L.ABSOR, 3, 1)):
            other.set_model(model, dim, 0.5, ls)
            assert assign(h=other._h) == L.ERR_INVALID and refine(h=other._h) == L.ERR_INVALID, (model, dim, ls)
            assert untouched()
            assert b"lsqr_assign_rigid" in lib.lsqr_last_error(other._h) or b"lsqr_refine_rigid" in lib.lsqr_last_error(
                other._h)
    # optional outputs may be absent
    assert lib.lsqr_refine_rigid(ctx._h, L.ptr(params), 3, 1, 0, None, None, fits, L.ptr(status), C.byref(rounds),
                                 C.byref(conv)) == L.OK
    assert rounds.value == 1 and np.all(status == L.OK)
