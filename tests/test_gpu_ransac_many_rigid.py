"""lsqr_ransac_many / Context.ransac_many for the closed-form estimators whose records are not plain points:
absolute orientation (6-double pairs, or 7 with the weighted fit), pivot calibration (13-slot frames), ray
intersection (with its minimum angle) and the 2-D line.  As for the point models (test_gpu_ransac_many.py): every
problem is decided as Context.ransac decides it on its own records with the same seed, independently of the other
problems, of their order and of how the rounds are cut, and the context's own upload is not touched."""
import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd import synth
from lsqrrecipes_amd.context import Context
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu
AUX = 0.017453292519943295769236907684886  # 1 degree
WEIGHTED = "absor_w"
# name -> (model, dim, delta, ls_type, aux, k)
CASES = {
    "absor": (L.ABSOR, 3, 1.0, 0, 0.0, 3),
    WEIGHTED: (L.ABSOR, 3, 1.0, 2, 0.0, 3),
    "pivot": (L.PIVOT, 3, 1.0, 0, 0.0, 3),
    "ray": (L.RAY, 3, 1.0, 0, AUX, 2),
    "line2d": (L.LINE2D, 2, 0.5, 0, 0.0, 2),
}
ORACLE = {"absor": O.ABSOR, "pivot": O.PIVOT, "ray": O.RAY, "line2d": O.LINE2D}


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _set(ctx, name):
    model, dim, delta, ls, aux, _ = CASES[name]
    return ctx.set_model(model, dim, delta, ls, aux=aux)


def _generate(name, n, outlier_frac, seed):
    if name in ("absor", WEIGHTED):
        d = synth.absolute_orientation(n, outlier_frac, seed=seed)[0]
        if name == WEIGHTED:
            w = np.random.default_rng(seed).uniform(0.25, 4.0, (n, 1))
            d = np.ascontiguousarray(np.hstack([d, w]))
        return d
    if name == "pivot":
        return synth.pivot(n, outlier_frac, seed=seed)[0]
    if name == "ray":
        return synth.rays(n, outlier_frac, seed=seed)[0]
    return synth.plane(n, outlier_frac, seed=seed, dim=2)[0]


def _degenerate(name, n, g):
    """records on which every minimal subset is refused by estimate(): fiducials on an axis-parallel line through
    integer points (the triad's third axis is exactly zero), identical pivot frames (rank 3 of 6), parallel rays,
    one repeated 2-D point"""
    if name in ("absor", WEIGHTED):
        d = np.zeros((n, 7 if name == WEIGHTED else 6))
        d[:, :3] = g.integers(-50, 50, 3)
        d[:, int(g.integers(3))] += g.integers(-20, 20, n)
        d[:, 3:6] = g.uniform(-100, 100, (n, 3))
        if name == WEIGHTED:
            d[:, 6] = 1.0
        return d
    if name == "pivot":
        f = np.zeros((n, 13))
        f[:, [0, 4, 8]] = 1.0
        f[:, 9:12] = g.integers(-500, 500, 3)
        return f
    if name == "ray":
        r = np.zeros((n, 6))
        r[:, :3] = g.uniform(-100, 100, (n, 3))
        v = g.normal(size=3)
        r[:, 3:] = v / np.linalg.norm(v)
        return r
    return np.tile(g.integers(-50, 50, 2).astype(np.float64), (n, 1))


def _problems(name, count=150, seed=0, max_n=3000):
    """~count problems: sizes k-1, 0, k, a few degenerate sets, the rest in [k, max_n] with 10-100 % inliers"""
    k = CASES[name][5]
    g = np.random.default_rng(list(CASES).index(name) + 100 * seed)
    nd = 7 if name == WEIGHTED else {"pivot": 13, "line2d": 2}.get(name, 6)
    probs = [np.zeros((k - 1, nd)), np.zeros((0, nd))]
    degenerate = []
    for j in range(count - 2):
        if j % 50 == 7:
            degenerate.append(len(probs))
            probs.append(_degenerate(name, int(g.integers(k, 24)), g))
            continue
        n = k if j == 0 else int(g.integers(k, max_n + 1))
        frac_in = float(g.uniform(0.1, 1.0)) if j % 9 else 1.0
        probs.append(_generate(name, n, 1.0 - frac_in, int(g.integers(1 << 30))))
    return probs, k, degenerate


def _align(name, got, want):
    if name in ("absor", WEIGHTED):  # q and -q are the same rotation
        s = np.sign(got[:4] @ want[:4]) or 1.0
        return np.concatenate([s * got[:4], got[4:]])
    if name == "line2d":             # the normal's sign is arbitrary
        s = np.sign(got[:2] @ want[:2]) or 1.0
        return np.concatenate([s * got[:2], got[2:]])
    return got


def _close(got, want, rel):
    return np.all(np.abs(got - want) <= rel * np.maximum(np.abs(want), 1.0))


def _check_against_single(ctx, name, probs, k, res, seeds, which=None):
    offs = res["offsets"]
    for j in (range(len(probs)) if which is None else which):
        lo, hi = int(offs[j]), int(offs[j + 1])
        assert hi - lo == len(probs[j])
        if len(probs[j]) < k:
            assert res["status"][j] == L.ERR_INVALID and res["fraction"][j] == 0.0, j
            assert not np.any(res["params"][j]) and res["iterations"][j] == 0, j
            continue
        _set(ctx, name).upload(probs[j])
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
            got = _align(name, res["params"][j], r["params"])
            assert _close(got, r["params"], 1e-9), (j, got, r["params"])
        else:
            assert not np.any(res["params"][j]), j


@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_single_problem_path(ctx, name):
    probs, k, degenerate = _problems(name)
    seeds = 3 + 5 * np.arange(len(probs), dtype=np.uint64)
    res = _set(ctx, name).ransac_many(probs, 0.999, seeds=seeds)
    st = res["status"]
    assert np.sum(st == L.ERR_INVALID) == 2 and np.sum(st == L.OK) > 120, st
    assert np.all(st[degenerate] == L.EMPTY), st[degenerate]
    _check_against_single(ctx, name, probs, k, res, seeds)


@pytest.mark.parametrize("name", list(ORACLE))
def test_parity_with_oracle(ctx, name):
    probs, k, _ = _problems(name, count=40, seed=1, max_n=800)
    seeds = 100 + np.arange(len(probs), dtype=np.uint64)
    res = _set(ctx, name).ransac_many(probs, 0.999, seeds=seeds)
    model, dim, delta, ls, aux, _ = CASES[name]
    oc = O.cfg(ORACLE[name], dim, delta, ls, aux=aux)
    offs = res["offsets"]
    checked = 0
    for j in range(len(probs)):
        if res["status"][j] != L.OK or checked == 20:
            continue
        w = O.ransac(oc, probs[j], 0.999, sampler="ctr", seed=int(seeds[j]))
        assert res["iterations"][j] == w["iters"], j
        assert np.array_equal(res["consensus"][int(offs[j]):int(offs[j + 1])], w["consensus"]), j
        got = _align(name, res["params"][j], w["params"])
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


@pytest.mark.parametrize("name", ["ray", "absor"])
def test_independence_of_order_subset_and_rounds(ctx, name):
    probs, k, _ = _problems(name, count=120, seed=2)
    seeds = 5 + np.arange(len(probs), dtype=np.uint64)
    _set(ctx, name)
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


@pytest.mark.parametrize("name", ["ray", "pivot"])
def test_one_large_problem_among_many_small(ctx, name):
    big = _generate(name, 200_000, 0.5, 77)
    small = [_generate(name, 60, 0.3 + 0.4 * (j % 2), 1000 + j) for j in range(2000)]
    probs = small[:1000] + [big] + small[1000:]
    seeds = 1 + np.arange(len(probs), dtype=np.uint64)
    res = _set(ctx, name).ransac_many(probs, 0.999, seeds=seeds)
    assert res["status"][1000] == L.OK
    which = [1000] + list(range(0, 2001, 97))
    _check_against_single(ctx, name, probs, CASES[name][5], res, seeds, which=which)


def test_context_state_untouched(ctx):
    data = _generate("ray", 30_000, 0.4, 5)
    _set(ctx, "ray").upload(data)
    r1 = ctx.ransac(0.999, seed=3)
    lib = ctx._lib
    assert lib.lsqr_count(ctx._h) == 30_000
    probs, _, _ = _problems("ray", count=30, seed=6)
    ctx.ransac_many(probs, 0.999)
    assert lib.lsqr_count(ctx._h) == 30_000
    r2 = ctx.ransac(0.999, seed=3)
    assert r1["status"] == r2["status"] == L.OK
    assert r1["info"].iterations == r2["info"].iterations and r1["info"].best_index == r2["info"].best_index
    assert np.array_equal(r1["consensus"], r2["consensus"])
    assert np.array_equal(r1["params"], r2["params"])


def _raw(ctx, recs, offs, p, nd):
    """lsqr_ransac_many on prefilled outputs, records nd doubles apart -> (status, outputs unchanged?)"""
    n = len(offs) - 1
    seeds = np.arange(1, n + 1, dtype=np.uint64)
    params = np.full((n, 32), 7.0)
    cons = np.full(int(offs[-1]), 9, dtype=np.uint8)
    infos = (L.RansacInfo * n)()
    for i in infos:
        i.iterations = 1234
    status = np.full(n, 99, dtype=np.int32)
    recs = np.ascontiguousarray(recs, dtype=np.float64)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    st = ctx._lib.lsqr_ransac_many(ctx._h, L.ptr(recs), nd * 8, L.ptr(offs), n, float(p), L.ptr(seeds),
                                   L.ptr(params), L.ptr(cons), infos, L.ptr(status))
    untouched = (np.all(params == 7.0) and np.all(cons == 9) and np.all(status == 99)
                 and all(i.iterations == 1234 for i in infos))
    return st, untouched


def test_argument_errors(ctx):
    _set(ctx, WEIGHTED)
    assert ctx.ND == 7
    recs = _generate(WEIGHTED, 300, 0.2, 9)
    st, _ = _raw(ctx, recs, [0, 100, 300], 0.99, 7)
    assert st == L.OK
    st, untouched = _raw(ctx, recs[:, :6], [0, 100, 300], 0.99, 6)   # the weight slot missing
    assert st == L.ERR_INVALID and untouched
    assert b"lsqr_ransac_many" in ctx._lib.lsqr_last_error(ctx._h)
    for model, ls in [(L.PHANTOM, L.LS_ANALYTIC), (L.US_POINTER, L.LS_ITERATIVE)]:
        ctx.set_model(model, 0, 2.0, ls)
        nd = ctx.ND
        st, untouched = _raw(ctx, np.zeros((300, nd)), [0, 100, 300], 0.99, nd)
        assert st == L.ERR_INVALID and untouched, model
        assert b"lsqr_ransac_many" in ctx._lib.lsqr_last_error(ctx._h)


def _strided(ctx, recs, offs, seeds, pad):
    """lsqr_ransac_many through the C ABI with `pad` extra doubles between records (the strided repack) -> outputs"""
    n = len(offs) - 1
    nd = recs.shape[1]
    wide = np.full((recs.shape[0], nd + pad), np.nan)   # the padding must never be read
    wide[:, :nd] = recs
    params = np.zeros((n, ctx.P))
    cons = np.zeros(int(offs[-1]), dtype=np.uint8)
    infos = (L.RansacInfo * n)()
    status = np.zeros(n, dtype=np.int32)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    st = ctx._lib.lsqr_ransac_many(ctx._h, L.ptr(wide), (nd + pad) * 8, L.ptr(offs), n, 0.999, L.ptr(seeds),
                                   L.ptr(params), L.ptr(cons), infos, L.ptr(status))
    assert st == L.OK
    inf = np.ctypeslib.as_array(infos)
    return status, params, cons, inf["iterations"].copy(), inf["best_index"].copy(), inf["fit"]["n_used"].copy()


@pytest.mark.parametrize("name", ["absor", WEIGHTED, "pivot"])
def test_strided_records(ctx, name):
    """records further apart than their width (stride = W*8 + 8, + 24): the same results, bit for bit, as packed"""
    probs, k, _ = _problems(name, count=30, seed=3, max_n=600)
    seeds = 7 + np.arange(len(probs), dtype=np.uint64)
    _set(ctx, name)
    res = ctx.ransac_many(probs, 0.999, seeds=seeds)
    recs = np.ascontiguousarray(np.concatenate(probs))
    for pad in (1, 3):
        status, params, cons, iters, best, used = _strided(ctx, recs, res["offsets"], seeds, pad)
        assert np.array_equal(status, res["status"]) and np.array_equal(iters, res["iterations"])
        assert np.array_equal(best, res["best_index"]) and np.array_equal(used, res["n_used"])
        assert np.array_equal(cons, res["consensus"])
        params[status != L.OK] = 0.0
        assert np.array_equal(params.view(np.uint64), res["params"].view(np.uint64)), pad
