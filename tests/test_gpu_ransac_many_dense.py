"""lsqr_ransac_many_dense / Context.ransac_many_dense and lsqr_dense_fit_many / Context.dense_fit_many: many robust
linear regressions (DenseLinearEquationSystemParametersEstimator<double,n>, n = 1..64) in one call
(csrc/many_dense.h).  Every problem is decided as Context.ransac decides it on a dense context holding its records
alone: bit-equal loop outcome, consensus set, fit.n_used and double-double flag (fit.reserved); parameters within
fp64 summation order.  A problem's result does not depend on the other problems, their order or the round cut."""
import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd import synth
from lsqrrecipes_amd.context import Context
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu
DELTA = 0.1
PART = 8192  # kManyPart: rows per workgroup of the finish


def stage(n):   # many_dense_stage<NR>: rows per LDS stage of the scan / finish
    return 4096 // _nr(n)


def seg(n):     # many_dense_seg<NR>: rows per scan tile
    return 131072 // _nr(n)


def _nr(n):
    return 8 if n <= 8 else 16 if n <= 16 else 32 if n <= 32 else 64


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _dense(ctx, n):
    return ctx.set_model(L.DENSE, n, DELTA)


def _out_frac(n):
    """outlier fractions that keep the adaptive bound at a few hundred hypotheses for k = n"""
    return 0.2 if n <= 9 else 0.1 if n <= 16 else 0.04 if n <= 33 else 0.02


def _problems(n, count, seed=0, lo=None, hi=3000):
    """sizes n - 1 and 0, then problems of lo..hi rows (synth.dense, noise well inside DELTA)"""
    g = np.random.default_rng(100 * n + seed)
    lo = max(3 * n, 40) if lo is None else lo
    probs = [np.zeros((n - 1, n + 1)), np.zeros((0, n + 1))]
    for _ in range(count - 2):
        m = int(g.integers(lo, hi + 1))
        probs.append(synth.dense(m, n, float(g.uniform(0.5, 1.0)) * _out_frac(n), seed=int(g.integers(1 << 30)),
                                 noise=1e-3)[0])
    return probs


def _check_against_single(ctx, n, probs, res, seeds, rtol=1e-9):
    offs = res["offsets"]
    for j in range(len(probs)):
        lo, hi = int(offs[j]), int(offs[j + 1])
        if len(probs[j]) < n:
            assert res["status"][j] == L.ERR_INVALID and res["fraction"][j] == 0.0, j
            assert not np.any(res["params"][j]) and res["iterations"][j] == 0, j
            continue
        _dense(ctx, n).upload(probs[j])
        r = ctx.ransac(0.999, seed=int(seeds[j]))
        i = r["info"]
        assert res["status"][j] == r["status"], (j, res["status"][j], r["status"])
        assert res["iterations"][j] == i.iterations, j
        assert res["best_index"][j] == i.best_index, j
        assert res["best_votes"][j] == i.best_votes, j
        assert res["fraction"][j] == i.fraction, j
        assert res["n_params"][j] == i.n_params and res["n_used"][j] == i.fit.n_used, j
        assert res["reserved"][j] == i.fit.reserved, (j, res["reserved"][j], i.fit.reserved)
        if i.best_votes > 0:
            assert np.array_equal(res["consensus"][lo:hi], r["consensus"]), j
        else:
            assert not np.any(res["consensus"][lo:hi]), j
        if r["status"] == L.OK:
            assert np.allclose(res["params"][j], r["params"], rtol=rtol, atol=rtol), (j, res["params"][j], r["params"])
        else:
            assert not np.any(res["params"][j]) and res["n_params"][j] == 0, j


# ---- 1. parity with the single-problem path ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 9, 16, 31, 33, 64])
def test_parity_with_single_problem_path(ctx, n):
    count = 24 if n <= 16 else 10
    probs = _problems(n, count, hi=3000 if n <= 33 else 1500)
    seeds = 3 + 7 * np.arange(len(probs), dtype=np.uint64)
    res = _dense(ctx, n).ransac_many_dense(probs, 0.999, seeds=seeds)
    st = res["status"]
    assert np.sum(st == L.ERR_INVALID) == 2 and np.sum(st == L.OK) >= count - 3, st
    _check_against_single(ctx, n, probs, res, seeds)


# ---- 2. the oracle (restated RANSAC.hxx with the counter sampler) -------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 5])
def test_parity_with_oracle(ctx, n):
    probs = _problems(n, 12, seed=1, hi=1200)
    seeds = 100 + np.arange(len(probs), dtype=np.uint64)
    res = _dense(ctx, n).ransac_many_dense(probs, 0.999, seeds=seeds)
    oc = O.cfg(O.DENSE, n, DELTA)
    offs = res["offsets"]
    checked = 0
    for j in range(len(probs)):
        if res["status"][j] != L.OK:
            continue
        w = O.ransac(oc, probs[j], 0.999, sampler="ctr", seed=int(seeds[j]))
        assert res["iterations"][j] == w["iters"] and res["best_votes"][j] == w["best_votes"], j
        assert res["best_index"][j] == w["best_iter"], j
        assert np.array_equal(res["consensus"][int(offs[j]):int(offs[j + 1])], w["consensus"]), j
        assert np.allclose(res["params"][j], w["params"], rtol=1e-6, atol=1e-6), (j, res["params"][j], w["params"])
        checked += 1
    assert checked >= 8


# ---- 3. independence ------------------------------------------------------------------------------------------------
def _same(a, b, ja, jb):
    for key in ("status", "fraction", "iterations", "best_index", "best_votes", "n_params", "n_used", "reserved"):
        assert np.array_equal(a[key][ja], b[key][jb]), key
    assert np.array_equal(a["params"][ja].view(np.uint64), b["params"][jb].view(np.uint64))
    for x, y in zip(ja, jb):
        assert np.array_equal(a["consensus"][a["offsets"][x]:a["offsets"][x + 1]],
                              b["consensus"][b["offsets"][y]:b["offsets"][y + 1]])


@pytest.mark.parametrize("n", [5, 20])
def test_independence_of_order_subset_and_rounds(ctx, n):
    probs = _problems(n, 40, seed=2, hi=2000)
    seeds = 9 + np.arange(len(probs), dtype=np.uint64)
    _dense(ctx, n)
    full = ctx.ransac_many_dense(probs, 0.999, seeds=seeds)
    k = len(probs)
    perm = np.random.default_rng(3).permutation(k)
    shuf = ctx.ransac_many_dense([probs[i] for i in perm], 0.999, seeds=seeds[perm])
    _same(full, shuf, perm, np.arange(k))
    sub = np.sort(np.random.default_rng(4).choice(k, k // 3, replace=False))
    part = ctx.ransac_many_dense([probs[i] for i in sub], 0.999, seeds=seeds[sub])
    _same(full, part, sub, np.arange(len(sub)))
    try:
        ctx.set_option("many_round_hypotheses", 700)
        small = ctx.ransac_many_dense(probs, 0.999, seeds=seeds)
    finally:
        ctx.set_option("many_round_hypotheses", 0)
    _same(full, small, np.arange(k), np.arange(k))


# ---- 4. sizes: N < n, N = n, empty problems, tails of the stage / part / segment --------------------------------
def _raw(ctx, fn, recs, offs, p, nd, np_=None):
    """the C call on prefilled outputs -> (status, per-problem status, infos, params, outputs unchanged?)"""
    n = len(offs) - 1 if np_ is None else np_
    m = max(n, 1)
    seeds = np.arange(1, m + 1, dtype=np.uint64)
    params = np.full((m, max(nd - 1, 1)), 7.0)   # (the dense model's n parameters per problem)
    cons = np.full(max(int(max(offs)) if len(offs) else 1, 1), 9, dtype=np.uint8)
    infos = (L.RansacInfo * m)()
    for i in infos:
        i.iterations = 1234
    status = np.full(m, 99, dtype=np.int32)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    recs = np.ascontiguousarray(recs, dtype=np.float64)
    st = fn(ctx._h, L.ptr(recs), nd * 8, L.ptr(offs), n, float(p), L.ptr(seeds), L.ptr(params), L.ptr(cons), infos,
            L.ptr(status))
    untouched = (np.all(params == 7.0) and np.all(cons == 9) and np.all(status == 99)
                 and all(i.iterations == 1234 for i in infos))
    return st, status, infos, params, untouched


def test_fewer_records_than_unknowns(ctx):
    n = 6
    _dense(ctx, n)
    good = synth.dense(200, n, 0.1, seed=4, noise=1e-3)[0]
    recs = np.vstack([good[:n - 1], good, good[:0]])
    offs = [0, n - 1, n - 1 + 200, n - 1 + 200]
    st, status, infos, params, _ = _raw(ctx, ctx._lib.lsqr_ransac_many_dense, recs, offs, 0.999, n + 1)
    assert st == L.OK
    assert status[0] == L.ERR_INVALID and status[2] == L.ERR_INVALID and status[1] == L.OK, status
    for j in (0, 2):
        assert infos[j].iterations == 0 and infos[j].best_votes == 0 and infos[j].fraction == 0.0, j
        assert np.all(params[j] == 7.0), j


@pytest.mark.parametrize("n", [8, 64])
def test_stage_part_and_segment_tails(ctx, n):
    """problems of n, n + 1 and one record either side of the LDS stage, the finish part and the scan segment:
    all-inlier problems vote N and fit as the oracle fits all records; with outliers, as the single path"""
    sizes = sorted({n, n + 1, stage(n) - 1, stage(n), stage(n) + 1, PART - 1, PART, PART + 1, seg(n) - 1, seg(n),
                    seg(n) + 1} - {0})
    sizes = [m for m in sizes if m >= n]
    clean = [synth.dense(m, n, 0.0, seed=40 + j, noise=0.0)[0] for j, m in enumerate(sizes)]
    seeds = 3 + np.arange(len(sizes), dtype=np.uint64)
    res = _dense(ctx, n).ransac_many_dense(clean, 0.999, seeds=seeds)
    oc = O.cfg(O.DENSE, n, DELTA)
    offs = res["offsets"]
    for j, m in enumerate(sizes):
        assert res["status"][j] == L.OK and res["best_votes"][j] == m and res["n_used"][j] == m, (m, res["best_votes"][j])
        assert np.all(res["consensus"][int(offs[j]):int(offs[j + 1])] == 1), m
        want = O.ls(oc, clean[j])
        assert np.allclose(res["params"][j], want, rtol=1e-6, atol=1e-6), (m, res["params"][j], want)
    _check_against_single(ctx, n, clean, res, seeds)
    noisy = [synth.dense(m, n, _out_frac(n), seed=60 + j, noise=1e-3)[0] for j, m in enumerate(sizes)]
    res = ctx.ransac_many_dense(noisy, 0.999, seeds=seeds)
    _check_against_single(ctx, n, noisy, res, seeds)


# ---- 5. degenerate and near-singular minimal subsets -------------------------------------------------------------
def _degenerate(n, m, seed):
    g = np.random.default_rng(seed)
    rows = synth.dense(m, n, 0.1, seed=seed, noise=1e-3)[0]
    dup = g.random(m) < 0.8                      # column 1 repeats column 0 on 80 % of the rows
    rows[dup, 1] = rows[dup, 0]
    near = rows.copy()                          # ... or nearly (a pivot near the elimination's threshold)
    near[dup, 1] = near[dup, 0] * (1.0 + 1e-12 * g.standard_normal(int(dup.sum())))
    zero = rows.copy()
    zero[:, n - 1] = 0.0                        # every subset singular
    return [rows, near, zero]


@pytest.mark.parametrize("fast", [1, 0])
def test_degenerate_minimal_subsets(ctx, fast):
    probs = []
    for n in (3, 5, 12):
        probs += [(n, p) for p in _degenerate(n, 400, 7 * n)]
    try:
        ctx.set_option("dense_fast_solve", fast)
        ctx.set_option("max_iterations", 1500)   # (the all-singular problems would run to the 2^22 no-model stop)
        for n in (3, 5, 12):
            ps = [p for (k, p) in probs if k == n]
            seeds = 11 + np.arange(len(ps), dtype=np.uint64)
            res = _dense(ctx, n).ransac_many_dense(ps, 0.999, seeds=seeds)
            # (the budget stops the loop at the end of the batch that reaches it: 256 + 1024 + 4096)
            assert res["status"][2] == L.EMPTY and res["iterations"][2] == 5376, (n, res["status"], res["iterations"])
            _check_against_single(ctx, n, ps, res, seeds)
    finally:
        ctx.set_option("dense_fast_solve", 1)
        ctx.set_option("max_iterations", 0)


# ---- 6. ill-conditioned finishes (the generator of test_gpu_dense_cond.py) -------------------------------------------
def system(m, n, cond, seed, resid):
    """A = U diag(s) V^T with singular values log-spaced from 10 down to 10 / cond; b = A x + resid * noise"""
    g = np.random.default_rng(seed)
    U = np.linalg.qr(g.standard_normal((m, n)))[0]
    V = np.linalg.qr(g.standard_normal((n, n)))[0]
    s = 10.0 * np.logspace(0.0, -np.log10(cond), n)
    A = (U * s) @ V.T
    x = g.uniform(-1.0, 1.0, n)
    b = A @ x + resid * g.standard_normal(m)
    return np.ascontiguousarray(np.hstack([A, b[:, None]])), x


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("n", [4, 16, 40])
def test_ill_conditioned_finishes(ctx, n):
    conds = [1e4, 1e8, 1e10]
    probs = [system(600 + 37 * i, n, c, 1000 * n + i, 0.0)[0] for i, c in enumerate(conds)]
    probs.append(synth.dense(700, n, 0.0, seed=5, noise=1e-3)[0])   # a well-conditioned one beside them
    seeds = 5 + np.arange(len(probs), dtype=np.uint64)
    res = _dense(ctx, n).ransac_many_dense(probs, 0.999, seeds=seeds)
    oc = O.cfg(O.DENSE, n, DELTA)
    assert res["reserved"][2] == 1 and res["reserved"][-1] == 0, res["reserved"]
    offs = res["offsets"]
    for j, rows in enumerate(probs):
        _dense(ctx, n).upload(rows)
        r = ctx.ransac(0.999, seed=int(seeds[j]))
        i = r["info"]
        assert res["status"][j] == r["status"] and res["reserved"][j] == i.fit.reserved, j
        assert res["iterations"][j] == i.iterations and res["best_votes"][j] == i.best_votes, j
        assert np.array_equal(res["consensus"][int(offs[j]):int(offs[j + 1])], r["consensus"]), j
        if r["status"] != L.OK:
            continue
        assert rel(res["params"][j], r["params"]) < 1e-6, (j, rel(res["params"][j], r["params"]))
        want = O.ls(oc, rows[r["consensus"] != 0])
        assert len(want) == n and rel(res["params"][j], want) < 1e-6, (j, want)


def test_dense_dd_off(ctx):
    """option dense_dd 0: the finish keeps the Gram block (no flags); the pseudo-inverse of the block decides where the
    elimination refuses, and fit.reserved is 2 there, as on the single path"""
    n = 12
    probs = [synth.dense(800, n, 0.0, seed=3, noise=1e-3)[0], system(700, n, 1e2, 31, 0.0)[0],
             system(900, n, 1e5, 32, 0.0)[0]]
    seeds = 40 + np.arange(len(probs), dtype=np.uint64)
    try:
        ctx.set_option("dense_dd", 0)
        res = _dense(ctx, n).ransac_many_dense(probs, 0.999, seeds=seeds)
        assert list(res["reserved"]) == [0, 0, 2], res["reserved"]
        offs = res["offsets"]
        for j, rows in enumerate(probs):
            _dense(ctx, n).upload(rows)
            r = ctx.ransac(0.999, seed=int(seeds[j]))
            i = r["info"]
            assert res["status"][j] == r["status"] == L.OK and res["reserved"][j] == i.fit.reserved, j
            assert res["iterations"][j] == i.iterations and res["best_index"][j] == i.best_index, j
            assert np.array_equal(res["consensus"][int(offs[j]):int(offs[j + 1])], r["consensus"]), j
            # (cond 1e5 through the normal equations: both paths carry eps cond(A)^2 ~ 1e-6)
            tol = 1e-4 if j == 2 else 1e-9
            assert rel(res["params"][j], r["params"]) < tol, (j, rel(res["params"][j], r["params"]))
        fit = ctx.dense_fit_many(probs)
        for j, rows in enumerate(probs):
            want, info = _single_fit(ctx, n, rows)
            assert fit["status"][j] == L.OK and fit["reserved"][j] == info.reserved, j
            assert rel(fit["params"][j], want) < (1e-4 if j == 2 else 1e-9), j
    finally:
        ctx.set_option("dense_dd", 1)


def test_svd_only_minimal_solves_at_64(ctx):
    """option dense_fast_solve 0 at n = 64: the w4 kernel only draws and every minimal system goes through the SVD
    list (not the register elimination); the outcome is the single path's"""
    n = 64
    g = np.random.default_rng(64)
    probs = [synth.dense(int(g.integers(300, 1200)), n, 0.02, seed=int(g.integers(1 << 30)), noise=1e-3)[0]
             for _ in range(4)]
    seeds = 70 + np.arange(len(probs), dtype=np.uint64)
    try:
        ctx.set_option("dense_fast_solve", 0)
        res = _dense(ctx, n).ransac_many_dense(probs, 0.999, seeds=seeds)
        assert np.all(res["status"] == L.OK), res["status"]
        _check_against_single(ctx, n, probs, res, seeds)
    finally:
        ctx.set_option("dense_fast_solve", 1)


# ---- 7. lsqr_dense_fit_many -------------------------------------------------------------------------------------
def _single_fit(ctx, n, rows, mask=None):
    _dense(ctx, n).upload(rows)
    if mask is not None:
        ctx.set_mask(mask)
    return ctx.ls_fit(use_mask=mask is not None)


@pytest.mark.parametrize("n", [3, 16, 64])
@pytest.mark.parametrize("masked", [False, True])
def test_dense_fit_many_against_ls_fit(ctx, n, masked):
    g = np.random.default_rng(n + 100 * masked)
    sizes = [n, n + 1, 500, PART - 1, PART + 1, 2 * PART + 3]
    sets = [synth.dense(m, n, 0.2, seed=200 + j, noise=1e-3)[0] for j, m in enumerate(sizes)]
    sets.append(system(900, n, 1e9, 7 * n, 0.0)[0])     # the double-double route
    masks = [(g.random(len(s)) < 0.7).astype(np.uint8) for s in sets] if masked else None
    if masked:
        masks[0][:] = 1
        masks[-1][:] = 1
    res = _dense(ctx, n).dense_fit_many(sets, masks=np.concatenate(masks) if masked else None)
    for j, rows in enumerate(sets):
        m = masks[j] if masked else None
        want, info = _single_fit(ctx, n, rows, m)
        used = int(m.sum()) if masked else len(rows)
        assert res["n_used"][j] == used and res["reserved"][j] == info.reserved, (j, res["reserved"][j], info.reserved)
        if len(want) == 0:
            assert res["status"][j] == L.EMPTY and res["n_params"][j] == 0, j
            continue
        assert res["status"][j] == L.OK and res["n_params"][j] == n, j
        tol = 1e-6 if j == len(sets) - 1 else 1e-9
        assert np.allclose(res["params"][j], want, rtol=tol, atol=tol), (j, res["params"][j], want)
    assert res["reserved"][-1] == 1


def test_dense_fit_many_empty_and_rank_deficient(ctx):
    n = 5
    a = synth.dense(300, n, 0.0, seed=1, noise=1e-3)[0]
    z = a.copy()
    z[:, 2] = 0.0                                   # rank deficient
    sets = [a, a[:0], a, z, a[:3]]                  # (3 rows < n: rank deficient too)
    masks = [np.ones(300, np.uint8), np.zeros(0, np.uint8), np.zeros(300, np.uint8), np.ones(300, np.uint8),
             np.ones(3, np.uint8)]
    lib = ctx._lib
    _dense(ctx, n)
    recs = np.ascontiguousarray(np.concatenate(sets))
    offs = np.zeros(len(sets) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in sets])
    m = np.ascontiguousarray(np.concatenate(masks))
    params = np.full((len(sets), n), 7.0)
    fits = (L.FitInfo * len(sets))()
    for f in fits:
        f.n_params = 77
    status = np.full(len(sets), 99, dtype=np.int32)
    st = lib.lsqr_dense_fit_many(ctx._h, L.ptr(recs), (n + 1) * 8, L.ptr(offs), len(sets), L.ptr(m), L.ptr(params),
                                 fits, L.ptr(status))
    assert st == L.OK
    assert list(status) == [L.OK, L.ERR_INVALID, L.ERR_INVALID, L.EMPTY, L.EMPTY], status
    for j in (1, 2):
        assert np.all(params[j] == 7.0) and fits[j].n_params == 77, j
    for j in (3, 4):
        assert np.all(params[j] == 7.0) and fits[j].n_params == 0, j
    want, _ = _single_fit(ctx, n, a)
    assert np.allclose(params[0], want, rtol=1e-9, atol=1e-9)
    res = ctx.dense_fit_many(sets)                 # without masks: the empty set alone is invalid
    assert list(res["status"]) == [L.OK, L.ERR_INVALID, L.OK, L.EMPTY, L.EMPTY], res["status"]


# ---- 8. contract edges ---------------------------------------------------------------------------------------------
def test_argument_errors_and_refused_models(ctx):
    lib = ctx._lib
    n = 4
    recs = synth.dense(300, n, 0.2, seed=9, noise=1e-3)[0]
    _dense(ctx, n)
    fn = lib.lsqr_ransac_many_dense
    for offs, p in [([0, 200, 100, 300], 0.99), ([5, 100, 300], 0.99), ([0, 100, 300], 0.0),
                    ([0, 100, 300], 1.0)]:
        st, _, _, _, untouched = _raw(ctx, fn, recs, offs, p, n + 1)
        assert st == L.ERR_INVALID and untouched, (offs, p)
        assert b"lsqr_ransac_many_dense" in lib.lsqr_last_error(ctx._h)
    st, _, _, _, untouched = _raw(ctx, fn, recs, [0], 0.99, n + 1, np_=0)
    assert st == L.OK and untouched
    st, _, _, _, untouched = _raw(ctx, fn, recs, [0, 100, 300], 0.99, n)   # stride below the record
    assert st == L.ERR_INVALID and untouched
    st, _, _, _, _ = _raw(ctx, fn, recs, [0, 100, 300], 0.99, n + 1)
    assert st == L.OK
    for model, dim, ls in [(L.SPHERE, 3, L.LS_ALGEBRAIC), (L.SPHERE, 3, L.LS_GEOMETRIC), (L.PLANE, 3, L.LS_ALGEBRAIC),
                           (L.LINE, 3, L.LS_ALGEBRAIC), (L.US_SINGLE, 3, L.LS_ANALYTIC), (L.ABSOR, 3, 0),
                           (L.PIVOT, 3, 0), (L.RAY, 3, 0), (L.LINE2D, 2, 0), (L.PHANTOM, 0, L.LS_ANALYTIC),
                           (L.US_POINTER, 0, L.LS_ITERATIVE)]:
        ctx.set_model(model, dim, DELTA, ls)
        nd = ctx.ND
        r = np.zeros((300, nd))
        st, _, _, _, untouched = _raw(ctx, fn, r, [0, 100, 300], 0.99, nd)
        assert st == L.ERR_INVALID and untouched, model
        assert b"lsqr_ransac_many_dense" in lib.lsqr_last_error(ctx._h)
        with pytest.raises(L.LsqrError):
            ctx.dense_fit_many([r[:100]])
    with Context(0) as fresh:   # no model set
        st, _, _, _, untouched = _raw(fresh, fn, recs, [0, 100, 300], 0.99, n + 1)
        assert st == L.ERR_STATE and untouched


@pytest.mark.parametrize("budget", [1, 255, 300])
def test_max_iterations_budget(ctx, budget):
    n = 10
    g = np.random.default_rng(budget)
    probs = [synth.dense(int(g.integers(100, 2000)), n, float(g.uniform(0.3, 0.5)), seed=int(g.integers(1 << 30)),
                         noise=1e-3)[0] for _ in range(8)]
    seeds = 21 + np.arange(len(probs), dtype=np.uint64)
    try:
        ctx.set_option("max_iterations", budget)
        res = _dense(ctx, n).ransac_many_dense(probs, 0.999, seeds=seeds)
        _check_against_single(ctx, n, probs, res, seeds)
    finally:
        ctx.set_option("max_iterations", 0)
    # (the budget stops a problem at the end of the batch that reaches it: 256, 1280, 5376 ...)
    assert np.all(res["iterations"] <= min(b for b in (256, 1280, 5376) if b >= budget))


def test_context_state_untouched(ctx):
    n = 12
    data = synth.dense(30_000, n, 0.1, seed=5, noise=1e-3)[0]
    _dense(ctx, n).upload(data)
    r1 = ctx.ransac(0.999, seed=3)
    lib = ctx._lib
    ctx.ransac_many_dense(_problems(n, 12, seed=6), 0.999)
    ctx.dense_fit_many([data[:500], data[500:900]])
    assert lib.lsqr_count(ctx._h) == 30_000
    r2 = ctx.ransac(0.999, seed=3)
    assert r1["status"] == r2["status"] == L.OK
    assert r1["info"].iterations == r2["info"].iterations and r1["info"].best_index == r2["info"].best_index
    assert np.array_equal(r1["consensus"], r2["consensus"])
    assert np.array_equal(r1["params"], r2["params"])
