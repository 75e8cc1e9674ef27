"""lsqr_ransac_many_lm / Context.ransac_many_lm and lsqr_lm_fit_many / Context.lm_fit_many: many RANSAC problems with
the geometric sphere's Levenberg-Marquardt finish, and many LM fits, in one call (csrc/many_lm.h).  Every problem is
decided as Context.ransac decides it on a geometric-sphere context holding its records alone: bit-equal loop outcome,
consensus set and fit.n_used; parameters and cost within the LM tolerances; the same LM info class and |d nfev| <= 3.
A problem's result, LM iterates included, does not depend on the other problems, their order or the round cut."""
import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd import synth
from lsqrrecipes_amd.context import Context
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu
DELTA = 0.5
PART = 8192  # kManyPart: inliers per workgroup of the LM pass


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _geo(ctx, dim):
    return ctx.set_model(L.SPHERE, dim, DELTA, L.LS_GEOMETRIC)


def _problems(dim, count=200, seed=0, out_lo=0.3, out_hi=0.7):
    """sizes k-1 and 0, then problems of 50..5000 records at out_lo..out_hi outliers"""
    k = dim + 1
    g = np.random.default_rng(50 * dim + seed)
    probs = [np.zeros((k - 1, dim)), np.zeros((0, dim))]
    for _ in range(count - 2):
        n = int(g.integers(50, 5001))
        probs.append(synth.sphere(n, float(g.uniform(out_lo, out_hi)), seed=int(g.integers(1 << 30)), dim=dim,
                                  box=100.0)[0])
    return probs, k


def _ok_class(info):
    return 1 <= int(info) <= 4


def _check_against_single(ctx, dim, probs, res, seeds, which=None):
    k = dim + 1
    offs = res["offsets"]
    for j in (range(len(probs)) if which is None else which):
        lo, hi = int(offs[j]), int(offs[j + 1])
        if len(probs[j]) < k:
            assert res["status"][j] == L.ERR_INVALID and res["fraction"][j] == 0.0, j
            assert not np.any(res["params"][j]) and res["iterations"][j] == 0, j
            continue
        _geo(ctx, dim).upload(probs[j])
        r = ctx.ransac(0.999, seed=int(seeds[j]))
        i = r["info"]
        assert res["status"][j] == r["status"], (j, res["status"][j], r["status"], i.fit.lm_info)
        assert res["iterations"][j] == i.iterations, j
        assert res["best_index"][j] == i.best_index, j
        assert res["best_votes"][j] == i.best_votes, j
        assert res["fraction"][j] == i.fraction, j
        assert res["n_params"][j] == i.n_params and res["n_used"][j] == i.fit.n_used, j
        if i.best_votes > 0:
            assert np.array_equal(res["consensus"][lo:hi], r["consensus"]), j
        else:
            assert not np.any(res["consensus"][lo:hi]), j
        assert _ok_class(res["lm_info"][j]) == _ok_class(i.fit.lm_info), (j, res["lm_info"][j], i.fit.lm_info)
        assert (res["lm_info"][j] == 0) == (i.fit.lm_info == 0), j   # both ran an LM, or neither
        assert abs(int(res["lm_nfev"][j]) - i.fit.lm_nfev) <= 3, (j, res["lm_nfev"][j], i.fit.lm_nfev)
        if i.fit.lm_info:
            assert np.isclose(res["cost"][j], i.fit.cost, rtol=1e-9, atol=1e-8), (j, res["cost"][j], i.fit.cost)
        if r["status"] == L.OK:
            assert np.allclose(res["params"][j], r["params"], rtol=1e-9, atol=1e-8), (j, res["params"][j], r["params"])
        else:
            assert not np.any(res["params"][j]) and res["n_params"][j] == 0, j


@pytest.mark.parametrize("dim,count,out_hi", [(2, 200, 0.7), (3, 200, 0.7), (5, 120, 0.5)])
def test_parity_with_single_problem_path(ctx, dim, count, out_hi):
    probs, k = _problems(dim, count=count, out_hi=out_hi)
    seeds = 3 + 5 * np.arange(len(probs), dtype=np.uint64)
    res = _geo(ctx, dim).ransac_many_lm(probs, 0.999, seeds=seeds)
    st = res["status"]
    assert np.sum(st == L.ERR_INVALID) == 2 and np.sum(st == L.OK) > 0.9 * count, st
    assert all(_ok_class(x) for x in res["lm_info"][st == L.OK])
    _check_against_single(ctx, dim, probs, res, seeds)


@pytest.mark.parametrize("dim", [2, 3])
def test_parity_with_oracle(ctx, dim):
    probs, k = _problems(dim, count=40, seed=1)
    seeds = 100 + np.arange(len(probs), dtype=np.uint64)
    res = _geo(ctx, dim).ransac_many_lm(probs, 0.999, seeds=seeds)
    offs = res["offsets"]
    checked = 0
    for j in range(len(probs)):
        if res["status"][j] != L.OK:
            continue
        pts = probs[j][res["consensus"][int(offs[j]):int(offs[j + 1])] != 0]
        want, winfo, _ = O.sphere_geometric(dim, pts, O.sphere_algebraic(dim, pts))
        assert _ok_class(winfo), j
        assert np.allclose(res["params"][j], want, rtol=1e-9, atol=1e-8), (j, res["params"][j], want)
        checked += 1
    assert checked > 30


def _same(a, b, ja, jb):
    for key in ("status", "fraction", "iterations", "best_index", "best_votes", "n_params", "n_used", "lm_info",
                "lm_nfev"):
        assert np.array_equal(a[key][ja], b[key][jb]), key
    for key in ("params", "cost"):
        assert np.array_equal(a[key][ja].view(np.uint64), b[key][jb].view(np.uint64)), key
    for x, y in zip(ja, jb):
        assert np.array_equal(a["consensus"][a["offsets"][x]:a["offsets"][x + 1]],
                              b["consensus"][b["offsets"][y]:b["offsets"][y + 1]])


def test_independence_of_order_subset_and_rounds(ctx):
    probs, _ = _problems(3, count=120, seed=2)
    seeds = 9 + np.arange(len(probs), dtype=np.uint64)
    _geo(ctx, 3)
    full = ctx.ransac_many_lm(probs, 0.999, seeds=seeds)
    n = len(probs)
    perm = np.random.default_rng(3).permutation(n)
    shuf = ctx.ransac_many_lm([probs[i] for i in perm], 0.999, seeds=seeds[perm])
    _same(full, shuf, perm, np.arange(n))
    sub = np.sort(np.random.default_rng(4).choice(n, n // 3, replace=False))
    part = ctx.ransac_many_lm([probs[i] for i in sub], 0.999, seeds=seeds[sub])
    _same(full, part, sub, np.arange(len(sub)))
    others, _ = _problems(3, count=60, seed=7)   # embedded among other problems
    emb = ctx.ransac_many_lm(others[:30] + probs + others[30:], 0.999,
                             seeds=np.concatenate([100 + np.arange(30, dtype=np.uint64), seeds,
                                                   200 + np.arange(30, dtype=np.uint64)]))
    _same(full, emb, np.arange(n), 30 + np.arange(n))
    try:
        ctx.set_option("many_round_hypotheses", 700)
        small = ctx.ransac_many_lm(probs, 0.999, seeds=seeds)
    finally:
        ctx.set_option("many_round_hypotheses", 0)
    _same(full, small, np.arange(n), np.arange(n))


def test_one_large_problem_among_many_small(ctx):
    big = synth.sphere(1_000_000, 0.5, seed=78, box=100.0)[0]
    small = [synth.sphere(200, 0.3 + 0.4 * (j % 2), seed=2000 + j, box=100.0)[0] for j in range(1000)]
    probs = small[:500] + [big] + small[500:]
    seeds = 1 + np.arange(len(probs), dtype=np.uint64)
    res = _geo(ctx, 3).ransac_many_lm(probs, 0.999, seeds=seeds)
    assert res["status"][500] == L.OK and res["n_used"][500] > 4 * PART
    _check_against_single(ctx, 3, probs, res, seeds, which=[500] + list(range(0, 1001, 97)))
    alone = ctx.ransac_many_lm(small, 0.999, seeds=np.delete(seeds, 500))
    idx = np.arange(1001) != 500
    _same(res, alone, np.nonzero(idx)[0], np.arange(1000))


def test_part_tails_and_degenerate_problems(ctx):
    """inlier counts of kManyPart +- 1 and 2 kManyPart +- 1 (all-inlier spheres), fewer than k records, a problem
    without a winner (collinear points: every minimal subset is degenerate), coplanar and nearly coplanar points
    (circles in a plane: no winner, or a winner whose consensus set makes the algebraic start ill-posed), all against
    the single path.  A RANSAC problem whose LM run ends outside info 1..4 could not be built: info 6..8 cannot fire
    before 1..4 with these tolerances (ftol, xtol, gtol > DBL_EPSILON), and no consensus set tried (nearly coplanar,
    clustered, small caps of large spheres) needed 500 evaluations from its algebraic fit; lm_fit_many covers that
    branch (test_lm_fit_many_evaluation_limit)."""
    sizes = [PART - 1, PART, PART + 1, 2 * PART - 1, 2 * PART, 2 * PART + 1]
    clean = [synth.sphere(n, 0.0, seed=60 + j, sigma=0.02, box=100.0)[0] for j, n in enumerate(sizes)]
    g = np.random.default_rng(5)
    line = np.outer(g.permutation(np.arange(1, 41, dtype=np.float64)), [1.0, 2.0, 3.0])
    t = g.uniform(0, 2 * np.pi, 80)
    circle = np.stack([10 * np.cos(t), 10 * np.sin(t), np.zeros(80)], 1)
    near = circle.copy()
    near[:, 2] = g.normal(0, 1e-12, 80)
    probs = clean + [np.zeros((3, 3)), np.zeros((0, 3)), line, circle, near]
    seeds = 11 + np.arange(len(probs), dtype=np.uint64)
    res = _geo(ctx, 3).ransac_many_lm(probs, 0.999, seeds=seeds)
    for j, n in enumerate(sizes):
        assert res["status"][j] == L.OK and res["best_votes"][j] == n and res["n_used"][j] == n, j
    assert res["status"][6] == res["status"][7] == L.ERR_INVALID
    assert res["status"][8] == L.EMPTY and res["best_votes"][8] == 0 and res["lm_info"][8] == 0
    _check_against_single(ctx, 3, probs, res, seeds)


def test_hostile_records(ctx):
    probs, _ = _problems(3, count=60, seed=8)
    g = np.random.default_rng(9)
    for j in range(2, len(probs)):
        p = probs[j]
        rows = g.choice(len(p), 5, replace=False)
        p[rows[0], 0] = np.nan
        p[rows[1], 1] = np.inf
        p[rows[2], 2] = -np.inf
        p[rows[3]] = np.nan
        p[rows[4], :] = [np.inf, -np.inf, np.nan]
    seeds = 1 + np.arange(len(probs), dtype=np.uint64)
    res = _geo(ctx, 3).ransac_many_lm(probs, 0.999, seeds=seeds)
    ok = res["status"] == L.OK
    assert np.sum(ok) > 40
    assert np.all(np.isfinite(res["params"][ok])) and np.all(np.isfinite(res["cost"][ok]))
    _check_against_single(ctx, 3, probs, res, seeds, which=range(0, len(probs), 4))


def _raw(ctx, fn, recs, offs, p, nd, np_=None):
    """lsqr_ransac_many_lm on prefilled outputs -> (status, outputs unchanged?)"""
    n = len(offs) - 1 if np_ is None else np_
    m = max(n, 1)
    seeds = np.arange(1, m + 1, dtype=np.uint64)
    params = np.full((m, 32), 7.0)
    cons = np.full(max(int(max(offs)) if len(offs) else 1, 1), 9, dtype=np.uint8)
    infos = (L.RansacInfo * m)()
    for i in infos:
        i.iterations = 1234
    status = np.full(m, 99, dtype=np.int32)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    st = fn(ctx._h, L.ptr(recs), nd * 8, L.ptr(offs), n, float(p), L.ptr(seeds), L.ptr(params), L.ptr(cons), infos,
            L.ptr(status))
    untouched = (np.all(params == 7.0) and np.all(cons == 9) and np.all(status == 99)
                 and all(i.iterations == 1234 for i in infos))
    return st, untouched


def test_argument_errors_and_refused_models(ctx):
    lib = ctx._lib
    recs = synth.sphere(300, 0.2, seed=9, box=100.0)[0]
    _geo(ctx, 3)
    for offs, p in [([0, 200, 100, 300], 0.99), ([5, 100, 300], 0.99), ([0, 100, 300], 0.0),
                    ([0, 100, 300], 1.0)]:
        st, untouched = _raw(ctx, lib.lsqr_ransac_many_lm, recs, offs, p, 3)
        assert st == L.ERR_INVALID and untouched, (offs, p)
    st, untouched = _raw(ctx, lib.lsqr_ransac_many_lm, recs, [0], 0.99, 3, np_=0)
    assert st == L.OK and untouched
    st, _ = _raw(ctx, lib.lsqr_ransac_many_lm, recs, [0, 100, 300], 0.99, 3)
    assert st == L.OK
    for model, dim, ls in [(L.SPHERE, 3, L.LS_ALGEBRAIC), (L.PLANE, 3, L.LS_ALGEBRAIC), (L.LINE, 3, L.LS_ALGEBRAIC),
                           (L.DENSE, 8, L.LS_ALGEBRAIC), (L.US_SINGLE, 3, L.LS_ANALYTIC),
                           (L.US_SINGLE, 3, L.LS_ITERATIVE), (L.ABSOR, 3, 0), (L.PIVOT, 3, 0), (L.RAY, 3, 0),
                           (L.LINE2D, 2, 0), (L.PHANTOM, 0, L.LS_ANALYTIC), (L.US_POINTER, 0, L.LS_ITERATIVE)]:
        ctx.set_model(model, dim, DELTA, ls)
        nd = ctx.ND
        r = np.zeros((300, nd))
        st, untouched = _raw(ctx, lib.lsqr_ransac_many_lm, r, [0, 100, 300], 0.99, nd)
        assert st == L.ERR_INVALID and untouched, model
        assert b"lsqr_ransac_many" in lib.lsqr_last_error(ctx._h)
        with pytest.raises(L.LsqrError):
            ctx.lm_fit_many([r[:100]], np.zeros((1, ctx.P)))
    with Context(0) as fresh:
        st, untouched = _raw(fresh, lib.lsqr_ransac_many_lm, recs, [0, 100, 300], 0.99, 3)
        assert st == L.ERR_STATE and untouched


def test_context_state_untouched(ctx):
    data = synth.sphere(30_000, 0.4, seed=5, box=100.0)[0]
    _geo(ctx, 3).upload(data)
    r1 = ctx.ransac(0.999, seed=3)
    lib = ctx._lib
    probs, _ = _problems(3, count=30, seed=6)
    ctx.ransac_many_lm(probs, 0.999)
    x0 = np.array([O.sphere_algebraic(3, p) if len(p) >= 4 else np.zeros(4) for p in probs[2:]])
    ctx.lm_fit_many(probs[2:], x0)
    assert lib.lsqr_count(ctx._h) == 30_000
    r2 = ctx.ransac(0.999, seed=3)
    assert r1["status"] == r2["status"] == L.OK
    assert r1["info"].iterations == r2["info"].iterations and r1["info"].best_index == r2["info"].best_index
    assert np.array_equal(r1["consensus"], r2["consensus"])
    assert np.array_equal(r1["params"], r2["params"])


# ---- lsqr_lm_fit_many ------------------------------------------------------------------------------------------
def _single_lm(ctx, dim, pts, mask=None):
    """upload + set_mask + ls_fit on an algebraic and on a geometric context: (algebraic start, LM params, FitInfo)"""
    ctx.set_model(L.SPHERE, dim, DELTA, L.LS_ALGEBRAIC).upload(pts)
    if mask is not None:
        ctx.set_mask(mask)
    x0, _ = ctx.ls_fit(use_mask=mask is not None)
    ctx.set_model(L.SPHERE, dim, DELTA, L.LS_GEOMETRIC).upload(pts)
    if mask is not None:
        ctx.set_mask(mask)
    got, info = ctx.ls_fit(use_mask=mask is not None)
    return x0, got, info


@pytest.mark.parametrize("dim", [2, 3, 5])
@pytest.mark.parametrize("masked", [False, True])
def test_lm_fit_many_against_single_set_path_and_oracle(ctx, dim, masked):
    g = np.random.default_rng(20 + dim + 7 * masked)
    sets = [synth.sphere(int(g.integers(30, 4000)), 0.0, seed=int(g.integers(1 << 30)), dim=dim, box=100.0,
                         sigma=0.3)[0] for _ in range(40)]
    sets.append(synth.sphere(2 * PART + 5, 0.0, seed=3, dim=dim, box=100.0)[0])
    masks = [(g.uniform(size=len(s)) < 0.7).astype(np.uint8) for s in sets] if masked else None
    starts, singles = [], []
    for j, s in enumerate(sets):
        x0, got, info = _single_lm(ctx, dim, s, masks[j] if masked else None)
        starts.append(x0)
        singles.append((got, info))
    res = _geo(ctx, dim).lm_fit_many(sets, np.array(starts), masks=np.concatenate(masks) if masked else None)
    for j, s in enumerate(sets):
        got, info = singles[j]
        pts = s[masks[j] != 0] if masked else s
        assert res["n_used"][j] == len(pts)
        assert res["status"][j] == (L.OK if _ok_class(info.lm_info) else L.EMPTY), j
        assert _ok_class(res["lm_info"][j]) == _ok_class(info.lm_info), j
        assert abs(int(res["lm_nfev"][j]) - info.lm_nfev) <= 3, (j, res["lm_nfev"][j], info.lm_nfev)
        assert np.isclose(res["cost"][j], info.cost, rtol=1e-9, atol=1e-8), j
        if res["status"][j] == L.OK:
            assert np.allclose(res["params"][j], got, rtol=1e-9, atol=1e-8), (j, res["params"][j], got)
            want, winfo, _ = O.sphere_geometric(dim, pts, starts[j])
            assert _ok_class(winfo)
            assert np.allclose(res["params"][j], want, rtol=1e-9, atol=1e-8), (j, res["params"][j], want)


def test_lm_fit_many_empty_sets_and_masks(ctx):
    s = synth.sphere(500, 0.0, seed=31, box=100.0)[0]
    x0 = O.sphere_algebraic(3, s)
    recs = np.concatenate([s, s])
    offs = np.array([0, 500, 500, 1000], dtype=np.uint64)
    mask = np.ones(1000, dtype=np.uint8)
    mask[500:] = 0  # set 2: empty mask
    _geo(ctx, 3)
    params = np.full((3, 4), 7.0)
    fits = (L.FitInfo * 3)()
    for f in fits:
        f.lm_nfev = 1234
    status = np.full(3, 99, dtype=np.int32)
    x0s = np.ascontiguousarray(np.tile(x0, (3, 1)))
    st = ctx._lib.lsqr_lm_fit_many(ctx._h, L.ptr(recs), 24, L.ptr(offs), 3, L.ptr(mask), L.ptr(x0s), L.ptr(params),
                                   fits, L.ptr(status))
    assert st == L.OK
    assert status[0] == L.OK and fits[0].n_used == 500 and 1 <= fits[0].lm_info <= 4
    for j in (1, 2):  # empty set, empty mask: ERR_INVALID, outputs untouched
        assert status[j] == L.ERR_INVALID and np.all(params[j] == 7.0) and fits[j].lm_nfev == 1234, j


def test_lm_fit_many_evaluation_limit(ctx):
    """tiny sets started far from the data: MINPACK stops at maxfev (info 5) -> EMPTY with n_params 0, as the
    single-set path (lsqr_lm_begin / lsqr_lm_step) and the oracle decide"""
    g = np.random.default_rng(1)
    sets, starts = [], []
    while len(sets) < 6:
        n = int(g.integers(4, 7))
        p = g.uniform(-1, 1, (n, 3))
        x0 = np.concatenate([g.uniform(-1, 1, 3) * 10.0 ** g.integers(3, 7), [g.uniform(0, 10) * 1e-3]])
        _, winfo, _ = O.sphere_geometric(3, p, x0)
        if winfo == 5:
            sets.append(p)
            starts.append(x0)
    res = _geo(ctx, 3).lm_fit_many(sets, np.array(starts))
    lib = ctx._lib
    hits = 0
    for j, p in enumerate(sets):
        ctx.upload(p)
        xt = np.zeros(4)
        lib.lsqr_lm_begin(ctx._h, L.ptr(np.ascontiguousarray(starts[j])), L.ptr(xt))
        while True:   # the single-set path, evaluation by evaluation (bounded by maxfev in lsqr_lm_step)
            blk = ctx.moments(xt, phase=1)
            cont = L.C.c_int(0)
            fi = L.FitInfo()
            out = np.zeros(32)
            st = lib.lsqr_lm_step(ctx._h, L.ptr(blk), L.ptr(xt), L.C.byref(cont), L.ptr(out), L.C.byref(fi))
            if not cont.value:
                break
        assert _ok_class(res["lm_info"][j]) == _ok_class(fi.lm_info), (j, res["lm_info"][j], fi.lm_info)
        assert (res["status"][j] == L.OK) == (st == L.OK), j
        if res["lm_info"][j] == 5:
            hits += 1
            assert res["status"][j] == L.EMPTY and not np.any(res["params"][j]) and res["lm_nfev"][j] == 500
    assert hits >= 1
