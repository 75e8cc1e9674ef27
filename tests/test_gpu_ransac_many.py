"""lsqr_ransac_many / Context.ransac_many: many independent RANSAC problems in one call (csrc/many.h).
Every problem is decided as Context.ransac decides it on its own records with the same seed (bit-equal loop
outcome and consensus set, parameters to reordered fp64 sums), independently of the other problems, of their
order and of how the rounds are cut; the context's own upload is not touched."""
import ctypes as C

import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd import synth
from lsqrrecipes_amd.context import Context
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu
GEN = {L.PLANE: synth.plane, L.SPHERE: synth.sphere, L.LINE: synth.line}
CASES = [(L.PLANE, 3), (L.PLANE, 2), (L.SPHERE, 3), (L.SPHERE, 2), (L.LINE, 3), (L.PLANE, 5)]
DELTA = 0.5


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _set(ctx, model, dim):
    return ctx.set_model(model, dim, DELTA, L.LS_ALGEBRAIC)


def _degenerate(model, dim, n, g):
    """records on which every minimal subset is degenerate: integer points on a line through the origin (3-D plane,
    sphere: exact zero cross product / determinant), one repeated point (line, 2-D plane, every model above 3-D)"""
    if model == L.LINE or dim > 3 or (model == L.PLANE and dim == 2):
        return np.tile(g.integers(-50, 50, dim).astype(np.float64), (n, 1))
    t = g.permutation(np.arange(1, n + 1, dtype=np.float64))
    return np.outer(t, np.arange(1, dim + 1, dtype=np.float64))


def _problems(model, dim, count=200, seed=0):
    """~count problems: sizes k-1, 0, k, a few degenerate sets, the rest in [k, 5000] with 10-100 % inliers"""
    k = dim if model == L.PLANE else (dim + 1 if model == L.SPHERE else 2)
    g = np.random.default_rng(1000 * model + 10 * dim + seed)
    lo = 0.1 if k <= 3 else 0.5   # keep numTries of the larger subsets modest
    probs = [np.zeros((k - 1, dim)), np.zeros((0, dim))]
    for j in range(count - 2):
        if j % 40 == 7:
            probs.append(_degenerate(model, dim, int(g.integers(k, 24)), g))
            continue
        n = k if j == 0 else int(g.integers(k, 5001))
        frac_in = float(g.uniform(lo, 1.0)) if j % 9 else 1.0
        data, _, _ = GEN[model](n, 1.0 - frac_in, seed=int(g.integers(1 << 30)), dim=dim)
        probs.append(data)
    return probs, k


def _align(model, dim, got, want):
    if model in (L.PLANE, L.LINE):
        s = np.sign(got[:dim] @ want[:dim]) or 1.0
        return np.concatenate([s * got[:dim], got[dim:]])
    return got


def _close(got, want, rel):
    return np.all(np.abs(got - want) <= rel * np.maximum(np.abs(want), 1.0))


def _check_against_single(ctx, model, dim, probs, k, res, seeds, which=None):
    offs = res["offsets"]
    for j in (range(len(probs)) if which is None else which):
        lo, hi = int(offs[j]), int(offs[j + 1])
        assert hi - lo == len(probs[j])
        if len(probs[j]) < k:
            assert res["status"][j] == L.ERR_INVALID and res["fraction"][j] == 0.0, j
            assert not np.any(res["params"][j]) and res["iterations"][j] == 0, j
            continue
        _set(ctx, model, dim).upload(probs[j])
        r = ctx.ransac(0.999, seed=int(seeds[j]))
        i = r["info"]
        assert res["status"][j] == r["status"], (j, res["status"][j], r["status"])
        assert res["iterations"][j] == i.iterations, j
        assert res["best_index"][j] == i.best_index, j
        assert res["best_votes"][j] == i.best_votes, j
        assert res["fraction"][j] == i.fraction, j
        assert res["n_params"][j] == i.n_params and res["n_used"][j] == i.fit.n_used, j
        if i.best_votes > 0:
            assert np.array_equal(res["consensus"][lo:hi], r["consensus"]), j
        else:
            assert not np.any(res["consensus"][lo:hi]), j
        if r["status"] == L.OK:
            got = _align(model, dim, res["params"][j], r["params"])
            assert _close(got, r["params"], 1e-9), (j, got, r["params"])
        else:
            assert not np.any(res["params"][j]), j


@pytest.mark.parametrize("model,dim", CASES)
def test_parity_with_single_problem_path(ctx, model, dim):
    probs, k = _problems(model, dim)
    seeds = 1 + 7 * np.arange(len(probs), dtype=np.uint64)
    res = _set(ctx, model, dim).ransac_many(probs, 0.999, seeds=seeds)
    st = res["status"]
    assert np.sum(st == L.ERR_INVALID) == 2 and np.sum(st == L.EMPTY) >= 4 and np.sum(st == L.OK) > 150, st
    _check_against_single(ctx, model, dim, probs, k, res, seeds)


@pytest.mark.parametrize("model,dim", [(L.PLANE, 3), (L.SPHERE, 3), (L.LINE, 3)])
def test_parity_with_oracle(ctx, model, dim):
    probs, k = _problems(model, dim, count=60, seed=1)
    seeds = 100 + np.arange(len(probs), dtype=np.uint64)
    res = _set(ctx, model, dim).ransac_many(probs, 0.999, seeds=seeds)
    oc = O.cfg(model, dim, DELTA, L.LS_ALGEBRAIC)
    offs = res["offsets"]
    checked = 0
    for j in range(len(probs)):
        if res["status"][j] != L.OK or checked == 20:
            continue
        w = O.ransac(oc, probs[j], 0.999, sampler="ctr", seed=int(seeds[j]))
        assert res["iterations"][j] == w["iters"], j
        assert np.array_equal(res["consensus"][int(offs[j]):int(offs[j + 1])], w["consensus"]), j
        got = _align(model, dim, res["params"][j], w["params"])
        assert _close(got, w["params"], 1e-6), (j, got, w["params"])
        checked += 1
    assert checked == 20


def _same(a, b, ja, jb):
    for key in ("status", "fraction", "iterations", "best_index", "best_votes", "n_params", "n_used"):
        assert np.array_equal(a[key][ja], b[key][jb]), key
    assert np.array_equal(a["params"][ja].view(np.uint64), b["params"][jb].view(np.uint64))
    for x, y in zip(ja, jb):
        assert np.array_equal(a["consensus"][a["offsets"][x]:a["offsets"][x + 1]],
                              b["consensus"][b["offsets"][y]:b["offsets"][y + 1]])


def test_independence_of_order_subset_and_rounds(ctx):
    probs, k = _problems(L.PLANE, 3, count=120, seed=2)
    seeds = 5 + np.arange(len(probs), dtype=np.uint64)
    _set(ctx, L.PLANE, 3)
    full = ctx.ransac_many(probs, 0.999, seeds=seeds)
    n = len(probs)
    perm = np.random.default_rng(3).permutation(n)
    shuf = ctx.ransac_many([probs[i] for i in perm], 0.999, seeds=seeds[perm])
    _same(full, shuf, perm, np.arange(n))
    sub = np.sort(np.random.default_rng(4).choice(n, n // 3, replace=False))
    part = ctx.ransac_many([probs[i] for i in sub], 0.999, seeds=seeds[sub])
    _same(full, part, sub, np.arange(len(sub)))
    try:
        ctx.set_option("many_round_hypotheses", 700)   # at most two first batches per round
        small = ctx.ransac_many(probs, 0.999, seeds=seeds)
    finally:
        ctx.set_option("many_round_hypotheses", 0)
    _same(full, small, np.arange(n), np.arange(n))
    assert np.array_equal(full["evaluated"], small["evaluated"])  # the same per-problem schedule


def test_one_large_problem_among_many_small(ctx):
    big, _, _ = synth.plane(1_000_000, 0.5, seed=77)
    small = [synth.plane(200, 0.3 + 0.4 * (j % 2), seed=1000 + j)[0] for j in range(1000)]
    probs = small[:500] + [big] + small[500:]
    seeds = 1 + np.arange(len(probs), dtype=np.uint64)
    res = _set(ctx, L.PLANE, 3).ransac_many(probs, 0.999, seeds=seeds)
    assert res["status"][500] == L.OK
    which = [500] + list(range(0, 1001, 53))
    _check_against_single(ctx, L.PLANE, 3, probs, 3, res, seeds, which=which)


def test_context_state_untouched(ctx):
    data, _, _ = synth.plane(30_000, 0.4, seed=5)
    _set(ctx, L.PLANE, 3).upload(data)
    r1 = ctx.ransac(0.999, seed=3)
    lib = ctx._lib
    assert lib.lsqr_count(ctx._h) == 30_000
    probs, _ = _problems(L.PLANE, 3, count=30, seed=6)
    ctx.ransac_many(probs, 0.999)
    assert lib.lsqr_count(ctx._h) == 30_000
    r2 = ctx.ransac(0.999, seed=3)
    assert r1["status"] == r2["status"] == L.OK
    assert r1["info"].iterations == r2["info"].iterations and r1["info"].best_index == r2["info"].best_index
    assert np.array_equal(r1["consensus"], r2["consensus"])
    assert np.array_equal(r1["params"], r2["params"])


def _raw(ctx, recs, offs, p, nd, np_=None):
    """lsqr_ransac_many on prefilled outputs -> (status, outputs unchanged?)"""
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
    st = ctx._lib.lsqr_ransac_many(ctx._h, L.ptr(recs), nd * 8, L.ptr(offs), n, float(p), L.ptr(seeds),
                                   L.ptr(params), L.ptr(cons), infos, L.ptr(status))
    untouched = (np.all(params == 7.0) and np.all(cons == 9) and np.all(status == 99)
                 and all(i.iterations == 1234 for i in infos))
    return st, untouched


def test_argument_errors(ctx):
    recs = synth.plane(300, 0.2, seed=9)[0]
    _set(ctx, L.PLANE, 3)
    for offs, p in [([0, 200, 100, 300], 0.99),    # decreasing
                    ([5, 100, 300], 0.99),          # offsets[0] != 0
                    ([0, 100, 300], 0.0),
                    ([0, 100, 300], 1.0)]:
        st, untouched = _raw(ctx, recs, offs, p, 3)
        assert st == L.ERR_INVALID and untouched, (offs, p)
    st, untouched = _raw(ctx, recs, [0], 0.99, 3, np_=0)
    assert st == L.OK and untouched
    st, _ = _raw(ctx, recs, [0, 100, 300], 0.99, 3)
    assert st == L.OK
    for model, dim, ls in [(L.DENSE, 8, L.LS_ALGEBRAIC), (L.US_SINGLE, 3, L.LS_ANALYTIC),
                           (L.SPHERE, 3, L.LS_GEOMETRIC)]:
        ctx.set_model(model, dim, DELTA, ls)
        nd = ctx.ND
        r = np.zeros((300, nd))
        st, untouched = _raw(ctx, r, [0, 100, 300], 0.99, nd)
        assert st == L.ERR_INVALID and untouched, model
        assert b"lsqr_ransac_many" in ctx._lib.lsqr_last_error(ctx._h)
    with Context(0) as fresh:   # no model set
        st, untouched = _raw(fresh, recs, [0, 100, 300], 0.99, 3)
        assert st == L.ERR_STATE and untouched


# ---- edges of the batched path: tile / part / segment tails, N-D models, the caller's budget ---------------------------
TAIL_SIZES = [255, 256, 257, 8191, 8192, 8193, 16383, 16384, 16385, 32769]  # kManyStage, kManyPart, kManySeg +- 1


def test_tile_and_part_tails(ctx):
    """problems one record either side of the LDS stage (256), the finish part (8192) and the scan segment (16384):
    all-inlier problems vote n and fit as the oracle fits all records; at 50 % outliers, as the single path"""
    k = 3
    sizes = [k, k + 1] + TAIL_SIZES
    clean = [synth.plane(n, 0.0, seed=40 + j, sigma=0.0)[0] for j, n in enumerate(sizes)]
    seeds = 3 + np.arange(len(sizes), dtype=np.uint64)
    res = _set(ctx, L.PLANE, 3).ransac_many(clean, 0.999, seeds=seeds)
    oc = O.cfg(L.PLANE, 3, DELTA, L.LS_ALGEBRAIC)
    offs = res["offsets"]
    for j, n in enumerate(sizes):
        assert res["status"][j] == L.OK and res["best_votes"][j] == n and res["n_used"][j] == n, (n, res["best_votes"][j])
        assert np.all(res["consensus"][int(offs[j]):int(offs[j + 1])] == 1), n
        want = O.ls(oc, clean[j])
        assert _close(_align(L.PLANE, 3, res["params"][j], want), want, 1e-6), (n, res["params"][j], want)
    noisy = [synth.plane(n, 0.5, seed=60 + j)[0] for j, n in enumerate(sizes)]
    res = ctx.ransac_many(noisy, 0.999, seeds=seeds)
    _check_against_single(ctx, L.PLANE, 3, noisy, k, res, seeds)


@pytest.mark.parametrize("dim", [4, 6, 8])
@pytest.mark.parametrize("model", [L.PLANE, L.SPHERE, L.LINE])
def test_nd_models(ctx, model, dim):
    """plane, sphere and line above 3-D (ManyModel<...N<D>>): every problem as the single path, a sample as the
    oracle"""
    probs, k = _problems(model, dim, count=24, seed=2)
    seeds = 9 + np.arange(len(probs), dtype=np.uint64)
    res = _set(ctx, model, dim).ransac_many(probs, 0.999, seeds=seeds)
    assert np.sum(res["status"] == L.OK) >= 15, res["status"]
    _check_against_single(ctx, model, dim, probs, k, res, seeds)
    oc = O.cfg(model, dim, DELTA, L.LS_ALGEBRAIC)
    offs = res["offsets"]
    for j in [j for j in range(len(probs)) if res["status"][j] == L.OK][:3]:
        w = O.ransac(oc, probs[j], 0.999, sampler="ctr", seed=int(seeds[j]))
        assert res["iterations"][j] == w["iters"] and res["best_votes"][j] == w["best_votes"], j
        assert np.array_equal(res["consensus"][int(offs[j]):int(offs[j + 1])], w["consensus"]), j
        assert _close(_align(model, dim, res["params"][j], w["params"]), w["params"], 1e-6), j


@pytest.mark.parametrize("budget", [1, 255, 256, 300, 5000])
def test_max_iterations_budget(ctx, budget):
    """the option max_iterations stops each problem where lsqr_ransac stops: iterations, evaluated hypotheses, winner
    and fit as Context.ransac under the same option"""
    g = np.random.default_rng(budget)
    probs = [synth.plane(int(g.integers(50, 3000)), float(g.uniform(0.6, 0.9)), seed=int(g.integers(1 << 30)))[0]
             for _ in range(12)]
    seeds = 21 + np.arange(len(probs), dtype=np.uint64)
    try:
        ctx.set_option("max_iterations", budget)
        res = _set(ctx, L.PLANE, 3).ransac_many(probs, 0.999, seeds=seeds)
        _check_against_single(ctx, L.PLANE, 3, probs, 3, res, seeds)
        for j, rec in enumerate(probs):
            _set(ctx, L.PLANE, 3).upload(rec)
            r = ctx.ransac(0.999, seed=int(seeds[j]))
            assert res["evaluated"][j] == r["info"].evaluated, j
    finally:
        ctx.set_option("max_iterations", 0)
    assert np.any(res["iterations"] >= min(budget, 256))
