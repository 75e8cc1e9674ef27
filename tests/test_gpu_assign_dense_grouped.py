"""lsqr_assign_dense_grouped / lsqr_refine_dense_grouped (csrc/assign_dense_grouped.h) through
Context.assign_dense_grouped / Context.refine_dense_grouped.

The contract is bit-identity per group, so every comparison here is a bit comparison (view(uint8)) against the existing
Context.assign_dense / Context.refine_dense on a second context that holds the host gather of one group, tightly packed,
with that group's rows of the parameters.  The references are computed once per scene and never changed.
Shapes: both sides of every row class (8, 16, 32, 64); groups of 1, n - 1, chunk - 1, chunk + 1 and 2 chunk + 5 rows
interleaved in one upload, so groups with one partial chunk, with exactly-not-a-chunk and with several chunks; an empty
group, a group without models, rows in no group; 1 to 5 and 64 models per group; tight and padded stride."""
import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd.context import Context
from test_gpu_assign import DeviceArray
from test_gpu_assign_dense import DELTA, SIGMA, _ill_scene, host_rows, mixture

pytestmark = pytest.mark.gpu
DIMS = (1, 8, 9, 17, 33, 64)
PAD = {1: 0, 8: 2, 9: 0, 17: 2, 33: 0, 64: 2}  # filler doubles after each row: half the cases
NG, MM = 7, 5
NM = np.array([1, 2, 3, 5, 4, 2, 0], dtype=np.uintp)  # models per group; group 5 has no rows, group 6 no models
G_EMPTY, G_NOMODEL, G_BIG, N_OUT = 5, 6, 4, 3
KEYS = ("params", "labels", "counts", "status", "n_used", "route", "rounds", "converged", "fits")


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx2():
    c = Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def sizes(n):
    chunk = L.assign_dense_chunk(n)
    return [1, max(n - 1, 1), chunk - 1, chunk + 1, 2 * chunk + 5, 0, 7]


_scenes, _refs = {}, {}


def scene(n):
    """-> rows (N x (n + 1)), groups (int32, interleaved; -3 and NG among them), planted X (NG, MM, n), start rows.
    Group g's rows lie on NM[g] regressions (group 6's on one that the call never sees)."""
    if n not in _scenes:
        g = np.random.default_rng([0xD6, n])
        sz = sizes(n)
        X = g.normal(size=(NG, MM, n))
        parts, labels = [], []
        for k in range(NG):
            rows, _, _ = mixture(n, sz[k], 1, 100 + k)
            owner = g.integers(0, max(int(NM[k]), 1), size=sz[k])
            rows[:, n] = np.einsum("ij,ij->i", rows[:, :n], X[k][owner]) + SIGMA * g.normal(size=sz[k])
            parts.append(rows)
            labels.append(np.full(sz[k], k, dtype=np.int32))
        parts[G_BIG][1, n // 2] = np.nan  # non-finite rows in one group: a NaN coefficient, an infinite right-hand side
        parts[G_BIG][2, n] = np.inf
        out, _, _ = mixture(n, 2 * N_OUT, 1, 99)  # rows in no group
        parts.append(out)
        labels.append(np.array([-3] * N_OUT + [NG] * N_OUT, dtype=np.int32))
        rows, groups = np.vstack(parts), np.concatenate(labels)
        order = g.permutation(len(rows))  # interleaved; a group's rows keep no particular place
        rows, groups = np.ascontiguousarray(rows[order]), np.ascontiguousarray(groups[order])
        # start rows moved off the planted ones inside the noise band; the big group's twice as far: a round more
        start = X + SIGMA / np.sqrt(n) * g.normal(size=X.shape)
        start[G_BIG] = X[G_BIG] + 2 * SIGMA / np.sqrt(n) * g.normal(size=X[G_BIG].shape)
        _scenes[n] = rows, groups, X, start
    return _scenes[n]


def put(c, n, rows, pad=0):
    wide = rows
    if pad:
        wide = np.full((len(rows), n + 1 + pad), -7.25)
        wide[:, :n + 1] = rows
    c.set_model(L.DENSE, n, DELTA).upload(wide)
    return c


FIT_FIELDS = ("n_params", "reserved", "n_used")  # what the contract names of lsqr_fit_info; the rest stays zero


def refine_grouped(c, groups, ng, params, nm, max_rounds):
    """Context.refine_dense_grouped, and the raw lsqr_fit_info records as "fits" (structured, (n_groups, max_models))"""
    out, f = c._refine_grouped(c._lib.lsqr_refine_dense_grouped, groups, ng, params, nm, max_rounds, None)
    out.update(route=f["reserved"].copy(), fits=f.copy())
    return out


def refine_one(c, params, max_rounds):
    """Context.refine_dense, with the raw lsqr_fit_info records as "fits" (structured, one per model)"""
    out, f = c._refine(c._lib.lsqr_refine_dense, params, max_rounds, None)
    out.update(route=f["reserved"].copy(), fits=f.copy())
    return out


def reference(ctx2, key, n, rows, groups, params, nm, what):
    """the ungrouped entry points on a fresh upload of every group that runs: what = "assign" or a max_rounds
    -> {g: dict}; computed once per key, never changed"""
    if (key, what) not in _refs:
        out = {}
        for g in range(len(nm)):
            own = np.ascontiguousarray(rows[groups == g])
            if len(own) == 0 or nm[g] == 0:
                continue
            put(ctx2, n, own)
            p = params[g, :nm[g]]
            out[g] = ctx2.assign_dense(p, want_residuals=True) if what == "assign" else refine_one(ctx2, p, what)
        _refs[key, what] = out
    return _refs[key, what]


def check_counts(got, g, ref_counts, nm):
    want = np.zeros(got["counts"].shape[1], dtype=np.uint64)
    want[:nm] = ref_counts[:nm]
    want[-1] = ref_counts[nm]
    assert np.array_equal(got["counts"][g], want), g


def check_refine(got, ref, groups, start, nm, ng, n, what=""):
    """every group of a refine_dense_grouped result against its reference (a group without one ran nothing)"""
    for g in range(ng):
        k = int(nm[g])
        sel = groups == g
        # the lsqr_fit_info records, every byte: the reference's for the models that are there, zeros for the others
        assert not bits(got["fits"][g, k:]).any(), (what, g)
        if g not in ref:
            assert not bits(got["fits"][g]).any(), (what, g)
            assert got["rounds"][g] == 0 and not got["converged"][g], (what, g)
            assert np.all(got["labels"][sel] == -1) and np.all(got["status"][g, :k] == L.OK), (what, g)
            assert not got["n_used"][g].any() and not got["route"][g].any(), (what, g)
            assert np.array_equal(bits(got["params"][g]), bits(start[g])), (what, g)
            assert got["counts"][g, -1] == sel.sum() and not got["counts"][g, :-1].any(), (what, g)
            continue
        r = ref[g]
        assert np.array_equal(bits(got["fits"][g, :k]), bits(r["fits"])), (what, g)
        for field in FIT_FIELDS:
            assert np.array_equal(got["fits"][field][g, :k], r["fits"][field]), (what, g, field)
        want_np = np.where(r["status"] == L.OK, n if r["rounds"] > 0 else 0, 0)  # n where the last refit gave a row
        assert np.array_equal(got["fits"]["n_params"][g, :k], want_np), (what, g)
        assert np.array_equal(bits(got["params"][g, :k]), bits(r["params"])), (what, g)
        assert np.array_equal(bits(got["params"][g, k:]), bits(start[g, k:])), (what, g)  # rows not there: as given
        assert np.array_equal(got["labels"][sel], r["labels"]), (what, g)
        check_counts(got, g, r["counts"], k)
        assert np.array_equal(got["status"][g, :k], r["status"]), (what, g)
        assert np.all(got["status"][g, k:] == L.ERR_STATE), (what, g)
        assert np.array_equal(got["n_used"][g, :k], r["n_used"]) and not got["n_used"][g, k:].any(), (what, g)
        assert np.array_equal(got["route"][g, :k], r["route"]) and not got["route"][g, k:].any(), (what, g)
        assert got["rounds"][g] == r["rounds"] and got["converged"][g] == r["converged"], (what, g, got["rounds"][g])


# ---- assign ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", DIMS)
def test_assign_equals_assign_dense_on_every_group(ctx, ctx2, n):
    rows, groups, X, start = scene(n)
    put(ctx, n, rows, PAD[n])
    ref = reference(ctx2, n, n, rows, groups, X, NM, "assign")
    got = ctx.assign_dense_grouped(groups, NG, X, NM, want_residuals=True)
    assert got["labels"].dtype == np.int32 and got["residuals"].dtype == np.float64
    assert np.array_equal(got["offsets"], np.concatenate([[0], np.cumsum(sizes(n))]).astype(np.uint64))
    assert sorted(ref) == [0, 1, 2, 3, 4]
    for g, r in ref.items():
        sel = groups == g
        assert np.array_equal(got["labels"][sel], r["labels"]), g
        assert np.array_equal(bits(got["residuals"][sel]), bits(r["residuals"])), g
        check_counts(got, g, r["counts"], int(NM[g]))
    dead = (groups < 0) | (groups >= NG) | (groups == G_NOMODEL)
    assert dead.sum() == 2 * N_OUT + 7
    assert np.all(got["labels"][dead] == -1) and np.all(np.isposinf(got["residuals"][dead]))
    assert got["counts"][G_NOMODEL, -1] == 7 and not got["counts"][G_NOMODEL, :-1].any()
    assert not got["counts"][G_EMPTY].any()
    # the non-finite rows of the big group
    big = np.flatnonzero(groups == G_BIG)
    bad = big[~np.isfinite(rows[big]).all(axis=1)]
    assert len(bad) == 2 and np.all(got["labels"][bad] == -1) and np.all(np.isposinf(got["residuals"][bad]))
    assert set(np.unique(got["labels"][big])) == {-1, 0, 1, 2, 3}
    # one small group against lsqr_assign_dense_host row by row
    sel = groups == 1
    hl, hr = host_rows(n, X[1, :NM[1]], rows[sel])
    assert np.array_equal(got["labels"][sel], hl) and np.array_equal(bits(got["residuals"][sel]), bits(hr))


@pytest.mark.parametrize("n", [9, 64])
def test_every_label_is_written_once(ctx, n):
    """the raw call into pre-filled buffers: no entry keeps its filler, -1 / +inf outside the groups that run"""
    rows, groups, X, _ = scene(n)
    put(ctx, n, rows, PAD[n])
    want = ctx.assign_dense_grouped(groups, NG, X, NM, want_residuals=True)
    labels = np.full(len(rows), 42, dtype=np.int32)
    res = np.full(len(rows), 42.0)
    par = np.ascontiguousarray(X)
    assert L.load().lsqr_assign_dense_grouped(ctx._h, L.ptr(groups), NG, 0, L.ptr(par), L.ptr(NM), MM, L.ptr(labels),
                                              L.ptr(res), None, None) == L.OK
    assert not np.any(labels == 42) and not np.any(res == 42.0)
    assert np.array_equal(labels, want["labels"]) and np.array_equal(bits(res), bits(want["residuals"]))


def _scene64():
    """n = 8, three groups, 64 rows of parameters each: a few planted regressions among rows that nothing is near"""
    n, ng = 8, 3
    g = np.random.default_rng(64)
    where = [3, 9, 17, 30, 31, 50, 63]
    sz = [300, 2 * 256 + 5, 255]
    params = np.empty((ng, 64, n))
    parts = []
    for k in range(ng):
        rows, X, _ = mixture(n, sz[k], 7, 200 + k)
        params[k] = X[g.integers(0, 7, size=64)] + 1e6
        params[k, where] = X
        parts.append(rows)
    groups = np.concatenate([np.full(s, k, dtype=np.int32) for k, s in enumerate(sz)])
    order = g.permutation(len(groups))
    return n, np.ascontiguousarray(np.vstack(parts)[order]), groups[order], params, where


def test_sixty_four_models_per_group(ctx, ctx2):
    n, rows, groups, params, where = _scene64()
    nm = np.array([64, 40, 64], dtype=np.uintp)  # group 1 sees the first 40 rows: four of its planted seven
    put(ctx, n, rows)
    got = ctx.assign_dense_grouped(groups, 3, params, nm, want_residuals=True)
    ref = reference(ctx2, "m64", n, rows, groups, params, nm, "assign")
    for g, r in ref.items():
        sel = groups == g
        assert np.array_equal(got["labels"][sel], r["labels"]) and np.array_equal(bits(got["residuals"][sel]),
                                                                                 bits(r["residuals"])), g
        check_counts(got, g, r["counts"], int(nm[g]))
        assert all(got["counts"][g, m] > 0 for m in where if m < nm[g])
        assert all(got["counts"][g, m] == 0 for m in range(64) if m not in where)
    start = params.copy()
    start[:, where] += SIGMA / np.sqrt(n) * np.random.default_rng(65).normal(size=(3, len(where), n))
    fit = refine_grouped(ctx, groups, 3, start, nm, 2)
    check_refine(fit, reference(ctx2, "m64r", n, rows, groups, start, nm, 2), groups, start, nm, 3, n)
    with pytest.raises(L.LsqrError) as e:
        ctx.assign_dense_grouped(groups, 3, np.zeros((3, 65, n)))
    assert e.value.status == L.ERR_INVALID
    # One round against numpy's least squares of the rows labelled m.  Models 31 and 63 own rows here: a presence word
    # whose bit 31 leaks into bits 32 .. 63 sends zero blocks of models that are not there over the next chunk's.
    # Gaussian rows, cond(A) < 10: the normal equations lose eps cond^2 ~ 1e-14; the bar is 1e-9.
    l0 = ctx.assign_dense_grouped(groups, 3, start, nm)["labels"]
    one =ctx.refine_dense_grouped(groups, 3, start, nm, max_rounds=1)
    for g in range(3):
        own = rows[groups == g]
        for m in where:
            sel = l0[groups == g] == m
            if m < nm[g]:
                assert sel.sum() >= n and one["n_used"][g, m] == sel.sum(), (g, m)
                want = np.linalg.lstsq(own[sel, :n], own[sel, n], rcond=None)[0]
                assert np.max(np.abs(one["params"][g, m] - want)) < 1e-9, (g, m)


# ---- refine ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_rounds", [0, 1, 8])
@pytest.mark.parametrize("n", DIMS)
def test_refine_equals_refine_dense_on_every_group(ctx, ctx2, n, max_rounds):
    rows, groups, X, start = scene(n)
    put(ctx, n, rows, PAD[n])
    ref = reference(ctx2, n, n, rows, groups, start, NM, max_rounds)
    got = refine_grouped(ctx, groups, NG, start, NM, max_rounds)
    print("n", n, "max_rounds", max_rounds, "rounds", list(got["rounds"]), "converged", list(got["converged"]))
    check_refine(got, ref, groups, start, NM, NG, n, (n, max_rounds))
    # the returned labels are the grouped assignment of the returned parameters
    again = ctx.assign_dense_grouped(groups, NG, got["params"], NM)
    assert np.array_equal(got["labels"], again["labels"]) and np.array_equal(got["counts"], again["counts"])
    if max_rounds == 0:
        assert not bits(got["fits"]).any()  # no refit ran: every record zero
        assert not got["rounds"].any() and not got["converged"].any() and not got["n_used"].any()
        assert np.array_equal(bits(got["params"]), bits(start))
    if max_rounds == 8:  # the groups stop on their own, at different rounds
        assert len(set(got["rounds"][:5])) > 1 and np.all(got["converged"][:5])
        assert np.all(got["rounds"][:5] >= 1) and got["rounds"][G_BIG] >= 2
    if max_rounds > 0 and n > 1:  # fewer than n rows on every model of groups 0 and 1: the rows stay, the round counts
        for g in (0, 1):
            assert np.array_equal(bits(got["params"][g]), bits(start[g])), g
            assert np.all(got["status"][g, :NM[g]] == L.EMPTY) and np.all(got["n_used"][g] < n), g
            assert not got["fits"]["n_params"][g].any(), g  # no row came back
            assert got["rounds"][g] == 1 and got["converged"][g], g


# ---- the double-double route ----------------------------------------------------------------------------------------
def _ill_grouped():
    """_ill_scene's 773 rows as group 1 between two ordinary groups, interleaved"""
    n, ill, X, sel = _ill_scene()
    a, Xa, _ = mixture(n, 300, 2, 31)
    b, Xb, _ = mixture(n, 2 * 256 + 9, 3, 32)
    rows = np.vstack([a, ill, b])
    groups = np.concatenate([np.zeros(len(a)), np.ones(len(ill)), np.full(len(b), 2)]).astype(np.int32)
    order = np.random.default_rng(33).permutation(len(rows))
    params = np.zeros((3, 3, n))
    params[0, :2], params[1], params[2] = Xa, X, Xb
    cond = np.linalg.cond(ill[sel, :n])
    assert 1e5 <= cond <= 1e6
    return n, np.ascontiguousarray(rows[order]), groups[order], params, np.array([2, 3, 3], dtype=np.uintp)


@pytest.mark.parametrize("dd, route", [(1, 1), (0, 2)])
def test_ill_conditioned_pair_takes_the_groups_own_route(ctx, ctx2, dd, route):
    """dense_dd 1: the flagged pair is solved again in double-double from ITS GROUP's rows, with the block count of the
    group's size; dense_dd 0: both sides solve from the same sums in the same order.  Bit-equal either way."""
    n, rows, groups, params, nm = _ill_grouped()
    put(ctx, n, rows)
    try:
        for c in (ctx, ctx2):
            c.set_option("dense_dd", dd)
        ref = reference(ctx2, ("ill", dd), n, rows, groups, params, nm, 1)
        got = refine_grouped(ctx, groups, 3, params, nm, 1)
    finally:
        for c in (ctx, ctx2):
            c.set_option("dense_dd", 1)
    assert [list(r) for r in got["route"]] == [[0, 0, 0], [0, 0, route], [0, 0, 0]]
    assert [list(r) for r in got["fits"]["n_params"]] == [[n, n, 0], [n, n, n], [n, n, n]]  # (group 0 has two models)
    assert np.all(got["status"][1] == L.OK) and np.all(got["rounds"] == 1)
    check_refine(got, ref, groups, params, nm, 3, n, dd)


# ---- independence and determinism -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [9, 33])
def test_groups_renumbered_one_dropped_and_the_same_call_twice(ctx, n):
    rows, groups, X, start = scene(n)
    put(ctx, n, rows, PAD[n])
    a = refine_grouped(ctx, groups, NG, start, NM, 8)
    b = refine_grouped(ctx, groups, NG, start, NM, 8)
    for key in KEYS:
        assert np.array_equal(bits(a[key]), bits(b[key])), key
    # old group -> new id; group 3 is dropped (its rows are in no group now), the others change places
    new_id = np.array([4, 2, 0, -1, 1, 3, 5, -1])  # (last entry: the label NG of the rows in no group)
    keep = [g for g in range(NG) if new_id[g] >= 0]
    groups2 = np.where(groups >= 0, new_id[np.clip(groups, 0, NG)], -1).astype(np.int32)
    start2, nm2 = np.zeros((NG - 1, MM, n)), np.zeros(NG - 1, dtype=np.uintp)
    for g in keep:
        start2[new_id[g]], nm2[new_id[g]] = start[g], NM[g]
    c = refine_grouped(ctx, groups2, NG - 1, start2, nm2, 8)
    for g in keep:
        h = new_id[g]
        sel = groups == g
        assert np.array_equal(c["labels"][sel], a["labels"][sel]), g
        for key in KEYS:
            if key != "labels":
                assert np.array_equal(bits(c[key][h]), bits(a[key][g])), (key, g)
    assert np.all(c["labels"][groups == 3] == -1)


# ---- the device form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [9, 64])
def test_device_groups_and_labels_on_attached_rows(ctx, n):
    rows, groups, X, start = scene(n)
    N = len(rows)
    put(ctx, n, rows)
    host_a = ctx.assign_dense_grouped(groups, NG, X, NM)
    host_r = ctx.refine_dense_grouped(groups, NG, start, NM, max_rounds=3)
    wide = np.full((N, n + 3), -7.25)
    wide[:, :n + 1] = rows
    t, grp = DeviceArray(wide), DeviceArray(groups)
    lab = DeviceArray(np.full(N, -9, dtype=np.int32))
    try:
        ctx.attach(t.data_ptr(), N, (n + 3) * 8, keepalive=t)
        dev = ctx.assign_dense_grouped(grp, NG, X, NM, labels_out=lab)
        assert dev["labels"] is lab and np.array_equal(lab.get(), host_a["labels"])
        assert np.array_equal(dev["counts"], host_a["counts"]) and np.array_equal(dev["offsets"], host_a["offsets"])
        lab.put(np.full(N, -9, dtype=np.int32))
        fit = ctx.refine_dense_grouped(grp, NG, start, NM, max_rounds=3, labels_out=lab)
        ctx.synchronize()
        assert fit["labels"] is lab and np.array_equal(lab.get(), host_r["labels"])
        for key in KEYS:
            if key not in ("labels", "fits"):
                assert np.array_equal(bits(fit[key]), bits(host_r[key])), key
        none = ctx.refine_dense_grouped(grp, NG, start, NM, max_rounds=3)  # the device form may leave labels_out out
        assert none["labels"] is None and np.array_equal(bits(none["params"]), bits(host_r["params"]))
        with pytest.raises(ValueError):
            ctx.assign_dense_grouped(grp, NG, X, NM, want_residuals=True, labels_out=lab)
        assert np.array_equal(bits(t.get()), bits(wide)) and np.array_equal(grp.get(), groups)  # only read
    finally:
        ctx.upload(np.zeros((4, n + 1)))  # let go of the attached buffer
        ctx._keep = None
        lab.free()
        grp.free()
        t.free()


# ---- the context ----------------------------------------------------------------------------------------------------
def test_context_is_untouched(ctx):
    n = 8
    rows, groups, X, start = scene(n)
    put(ctx, n, rows)
    ctx.hypotheses_sample(7, 0, 256)
    ctx.scan()
    hyp_before = ctx.hypotheses()
    mask_before, cnt_before = ctx.mask(X[G_BIG, 1])
    index_before = ctx.index_info()
    out = ctx.refine_dense_grouped(groups, NG, start, NM)
    assert out["rounds"][G_BIG] >= 1
    ctx.assign_dense_grouped(groups, NG, out["params"], NM, want_residuals=True)
    fit_after, _ = ctx.ls_fit(use_mask=True)  # the mask of that regression is still there
    assert ctx.index_info() == index_before
    for a, b in zip(hyp_before, ctx.hypotheses()):
        assert np.array_equal(bits(a), bits(b))
    ctx.mask(X[G_BIG, 1])
    fit_want, _ = ctx.ls_fit(use_mask=True)
    assert cnt_before == mask_before.sum() and len(fit_want) == n
    assert np.array_equal(bits(fit_after), bits(fit_want))
