"""lsqr_ransac_many_exhaustive / Context.ransac_many_exhaustive: many independent problems of the exhaustive RANSAC
overload (every k-subset in lexicographic order, the first maximum wins) in one call (csrc/many_exhaustive.h).  Every
problem is decided as Context.ransac_exhaustive decides it on its records alone -- discrete fields and consensus bit
for bit, closed-form parameters within 1e-9 relative, the geometric sphere within the bounds of the batched LM stage --
whichever device path runs (one fused workgroup per small problem, or rounds), independently of the other problems, of
their order and of how the rounds are cut; the context's own upload is not touched."""
import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd import context as ctx_mod
from lsqrrecipes_amd import synth
from lsqrrecipes_amd.context import Context
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu
AUX = 0.017453292519943295769236907684886  # 1 degree
# name -> (model, dim, delta, ls_type, aux, k, record doubles, oracle model or None)
CASES = {
    "plane2": (L.PLANE, 2, 0.5, 0, 0.0, 2, 2, O.PLANE),
    "plane3": (L.PLANE, 3, 0.5, 0, 0.0, 3, 3, O.PLANE),
    "plane5": (L.PLANE, 5, 0.5, 0, 0.0, 5, 5, O.PLANE),
    "line3": (L.LINE, 3, 0.5, 0, 0.0, 2, 3, O.LINE),
    "sphere3": (L.SPHERE, 3, 0.5, L.LS_ALGEBRAIC, 0.0, 4, 3, O.SPHERE),
    "sphere3_geo": (L.SPHERE, 3, 0.5, L.LS_GEOMETRIC, 0.0, 4, 3, O.SPHERE),
    "absor": (L.ABSOR, 3, 1.0, 0, 0.0, 3, 6, O.ABSOR),
    "absor_w": (L.ABSOR, 3, 1.0, 2, 0.0, 3, 7, None),
    "pivot": (L.PIVOT, 3, 1.0, 0, 0.0, 3, 13, None),
    "ray": (L.RAY, 3, 1.0, 0, AUX, 2, 6, None),
    "line2d": (L.LINE2D, 2, 0.5, 0, 0.0, 2, 2, None),
}
POINT = ("plane2", "plane3", "plane5", "line3", "sphere3", "sphere3_geo", "line2d")
GEO = "sphere3_geo"
MAX_N = 40   # C(40, 4) x 40 agree() per problem: the oracle's loop takes some 10 ms
# ... except for the 5-D plane, whose minimal fit is an SVD: C(40, 5) of them take the oracle 7 s a problem, C(18, 5)
# 0.1 s.  The oracle test alone uses the smaller size; against the device's own single call the 5-D plane goes to 40
# records too, where C(27, 5) = 80 730 and more lie above the fused path's cap: the SVD model takes both paths.
ORACLE_MAX_N = {"plane5": 18}


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _set(ctx, name):
    model, dim, delta, ls, aux = CASES[name][:5]
    return ctx.set_model(model, dim, delta, ls, aux=aux)


def _generate(name, n, outlier_frac, seed):
    dim = CASES[name][1]
    if name in ("absor", "absor_w"):
        d = synth.absolute_orientation(n, outlier_frac, seed=seed)[0]
        if name == "absor_w":
            d = np.ascontiguousarray(np.hstack([d, np.random.default_rng(seed).uniform(0.25, 4.0, (n, 1))]))
        return d
    if name == "pivot":
        return synth.pivot(n, outlier_frac, seed=seed)[0]
    if name == "ray":
        return synth.rays(n, outlier_frac, seed=seed)[0]
    if name.startswith("sphere"):
        return synth.sphere(n, outlier_frac, seed=seed, dim=dim, box=100.0)[0]
    if name == "line3":
        return synth.line(n, outlier_frac, seed=seed, dim=dim)[0]
    return synth.plane(n, outlier_frac, seed=seed, dim=dim)[0]


def _degenerate(name, n, g):
    """records on which estimate() refuses every minimal subset: the collinear fiducials of
    test_gpu_parity.py::test_absolute_orientation_exhaustive_ransac_matches_oracle, identical pivot frames, parallel
    rays, one repeated point"""
    nd = CASES[name][6]
    if name in ("absor", "absor_w"):
        d = _generate(name, n, 0.25, 77)
        d[:, :3] = np.outer(np.arange(n), [1.0, 2.0, 3.0])
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
    return np.tile(g.integers(-50, 50, nd).astype(np.float64), (n, 1))


def _ties(name, g):
    """a problem whose hypotheses all tie.  Point models: k + 3 points spread over 1e5, so that every minimal subset
    gathers its own k points and nothing else (rank 0 must win); plane3 also gets integer points of the plane z = 0,
    where every valid subset gathers all of them.  The other models: records without a common answer."""
    k, nd = CASES[name][5], CASES[name][6]
    if name in POINT:
        return g.uniform(-1e5, 1e5, (k + 3, nd))
    return _generate(name, 6, 1.0, int(g.integers(1 << 30)))


def _problems(name, count=220, seed=0, max_n=MAX_N):
    """count problems: sizes k-1, 0, k, degenerate sets, ties, the rest k..max_n records with 0-60 % outliers
    -> (problems, k, indices of the degenerate ones, indices of the point models' tie problems)"""
    k, nd = CASES[name][5], CASES[name][6]
    g = np.random.default_rng(list(CASES).index(name) + 100 * seed)
    probs = [np.zeros((k - 1, nd)), np.zeros((0, nd)), _generate(name, k, 0.0, 5)]
    degenerate, ties = [], []
    for j in range(count - 3):
        if j % 40 == 7:
            degenerate.append(len(probs))
            probs.append(_degenerate(name, int(g.integers(k, 16)), g))
        elif j % 40 == 11:
            if name in POINT:
                ties.append(len(probs))
            probs.append(_ties(name, g))
        else:
            n = int(g.integers(k, max_n + 1))
            probs.append(_generate(name, n, float(g.uniform(0.0, 0.6)), int(g.integers(1 << 30))))
    if name == "plane3":
        flat = np.zeros((9, 3))
        flat[:, :2] = [[0, 0], [1, 0], [2, 0], [0, 1], [3, 2], [5, 1], [2, 2], [7, 7], [1, 5]]
        probs.append(flat)
    return probs, k, degenerate, ties


def _align(name, got, want):
    if name in ("absor", "absor_w"):  # q and -q are the same rotation
        s = np.sign(got[:4] @ want[:4]) or 1.0
        return np.concatenate([s * got[:4], got[4:]])
    if name in ("plane2", "plane3", "plane5", "line3", "line2d"):   # the normal's / direction's sign is arbitrary
        d = CASES[name][1]
        s = np.sign(got[:d] @ want[:d]) or 1.0
        return np.concatenate([s * got[:d], got[d:]])
    return got


def _close(got, want, rel):
    return np.all(np.abs(got - want) <= rel * np.maximum(np.abs(want), 1.0))


def _ok_class(info):
    return 1 <= int(info) <= 4


def _check_against_single(ctx, name, probs, k, res, which=None):
    """every problem (or those of `which`) against ransac_exhaustive on its records alone -> number compared"""
    offs = res["offsets"]
    compared = 0
    for j in (range(len(probs)) if which is None else which):
        lo, hi = int(offs[j]), int(offs[j + 1])
        n = len(probs[j])
        assert hi - lo == n
        compared += 1
        if n == 0:   # (an empty upload is refused before the single call could run: the contract's N < k)
            assert res["status"][j] == L.EMPTY and res["iterations"][j] == 0 and not np.any(res["params"][j]), j
            continue
        _set(ctx, name).upload(probs[j])
        r = ctx.ransac_exhaustive()
        i = r["info"]
        assert res["status"][j] == r["status"], (j, res["status"][j], r["status"])
        assert res["iterations"][j] == i.iterations == res["evaluated"][j] == i.evaluated, j
        if n >= k:
            assert i.iterations == ctx_mod.comb_count(n, k), j
        else:
            assert r["status"] == L.EMPTY and i.iterations == 0 and res["fraction"][j] == 0.0, j
        assert res["best_index"][j] == i.best_index, j
        assert res["best_votes"][j] == i.best_votes, j
        assert res["fraction"][j] == i.fraction, j
        assert res["n_params"][j] == i.n_params and res["n_used"][j] == i.fit.n_used, j
        if i.best_votes > 0:
            assert np.array_equal(res["consensus"][lo:hi], r["consensus"]), j
        else:
            assert not np.any(res["consensus"][lo:hi]), j
        if name == GEO:
            assert _ok_class(res["lm_info"][j]) == _ok_class(i.fit.lm_info), (j, res["lm_info"][j], i.fit.lm_info)
            assert (res["lm_info"][j] == 0) == (i.fit.lm_info == 0), j
            assert abs(int(res["lm_nfev"][j]) - i.fit.lm_nfev) <= 3, (j, res["lm_nfev"][j], i.fit.lm_nfev)
            if i.fit.lm_info:
                assert np.isclose(res["cost"][j], i.fit.cost, rtol=1e-9, atol=1e-8), (j, res["cost"][j], i.fit.cost)
        if r["status"] == L.OK:
            if name == GEO:
                assert np.allclose(res["params"][j], r["params"], rtol=1e-9, atol=1e-8), (j, res["params"][j])
            else:
                got = _align(name, res["params"][j], r["params"])
                assert _close(got, r["params"], 1e-9), (j, got, r["params"])
        else:
            assert not np.any(res["params"][j]), j
    return compared


KEYS = ("status", "fraction", "iterations", "best_index", "best_votes", "evaluated", "n_params", "n_used")


def _same(a, b, ja, jb, name=None):
    """problems ja of a and jb of b: the same bit patterns, parameters included"""
    for key in KEYS + (("lm_info", "lm_nfev") if name == GEO else ()):
        assert np.array_equal(a[key][ja], b[key][jb]), key
    assert np.array_equal(a["params"][ja].view(np.uint64), b["params"][jb].view(np.uint64))
    if name == GEO:
        assert np.array_equal(a["cost"][ja].view(np.uint64), b["cost"][jb].view(np.uint64))
    for x, y in zip(ja, jb):
        assert np.array_equal(a["consensus"][a["offsets"][x]:a["offsets"][x + 1]],
                              b["consensus"][b["offsets"][y]:b["offsets"][y + 1]])


def _both_paths(ctx, probs):
    """the call with many_exhaustive_fused 1 (default) and 0"""
    fused = ctx.ransac_many_exhaustive(probs)
    try:
        ctx.set_option("many_exhaustive_fused", 0)
        general = ctx.ransac_many_exhaustive(probs)
    finally:
        ctx.set_option("many_exhaustive_fused", 1)
    return fused, general


@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_single_problem_path_and_between_paths(ctx, name):
    probs, k, degenerate, ties = _problems(name)
    _set(ctx, name)
    res, general = _both_paths(ctx, probs)
    every = np.arange(len(probs))
    _same(res, general, every, every, name)
    st = res["status"]
    assert st[0] == L.EMPTY and st[1] == L.EMPTY and np.sum(st == L.ERR_INVALID) == 0, st
    assert np.sum(st == L.OK) > 120, st
    assert np.all(st[degenerate] == L.EMPTY) and not np.any(res["best_votes"][degenerate]), st[degenerate]
    if ties:
        assert np.all(res["best_index"][ties] == 0) and np.all(res["best_votes"][ties] == k), res["best_index"][ties]
    if name == "plane3":   # the flat problem: (0, 1, 2) is collinear, the first valid subset takes every point
        assert res["best_votes"][-1] == 9 and res["best_index"][-1] == 1 and st[-1] == L.OK
        assert list(ctx_mod.comb_unrank(9, 3, 1)) == [0, 1, 3]
    assert _check_against_single(ctx, name, probs, k, res) == len(probs)   # no problem left out


@pytest.mark.parametrize("name", [n for n in CASES if CASES[n][7] is not None])
def test_parity_with_oracle(ctx, name):
    probs, k, _, _ = _problems(name, count=120, seed=1, max_n=ORACLE_MAX_N.get(name, MAX_N))
    res = _set(ctx, name).ransac_many_exhaustive(probs)
    model, dim, delta, ls, aux = CASES[name][:5]
    oc = O.cfg(CASES[name][7], dim, delta, ls, aux=aux)
    offs = res["offsets"]
    for j in range(len(probs)):
        w = O.ransac_exhaustive(oc, probs[j])
        assert res["fraction"][j] == w["fraction"], j
        assert np.array_equal(res["consensus"][int(offs[j]):int(offs[j + 1])], w["consensus"]), j


def test_large_problem_takes_the_general_path_in_both_settings(ctx):
    """256 < N <= 600 (plane, k = 3): beyond the LDS stage, so rounds whatever the option says -- here cut so that the
    problem's C(N, 3) ranks span several rounds -- among small problems that take the fused path"""
    small, k, _, _ = _problems("plane3", count=40, seed=4)
    big = [synth.plane(n, 0.4, seed=300 + n)[0] for n in (257, 420, 600)]
    probs = small[:20] + big[:1] + small[20:] + big[1:]
    where = [20, len(probs) - 2, len(probs) - 1]
    _set(ctx, "plane3")
    try:
        ctx.set_option("many_round_hypotheses", 3_000_000)   # C(600, 3) = 35 820 200: twelve rounds
        res, general = _both_paths(ctx, probs)
    finally:
        ctx.set_option("many_round_hypotheses", 0)
    every = np.arange(len(probs))
    _same(res, general, every, every)
    assert np.all(res["status"][where] == L.OK)
    assert res["iterations"][where[2]] == 35_820_200
    assert _check_against_single(ctx, "plane3", probs, k, res, which=where + [0, 1, 2, 5, 30]) == 8


@pytest.mark.parametrize("name", ["ray", "absor", "sphere3_geo", "plane3"])
def test_independence_of_order_subset_and_rounds(ctx, name):
    probs, k, _, _ = _problems(name, count=120, seed=2)
    _set(ctx, name)
    full = ctx.ransac_many_exhaustive(probs)
    n = len(probs)
    perm = np.random.default_rng(3).permutation(n)
    shuf = ctx.ransac_many_exhaustive([probs[i] for i in perm])
    _same(full, shuf, perm, np.arange(n), name)
    sub = np.sort(np.random.default_rng(4).choice(n, n // 3, replace=False))
    part = ctx.ransac_many_exhaustive([probs[i] for i in sub])
    _same(full, part, sub, np.arange(len(sub)), name)
    # rounds far smaller than a problem: the largest has C(40, k) ranks, at least 780 = more than three rounds of 200
    # (the fused path off, or no problem would see a round)
    most = max(ctx_mod.comb_count(len(q), k) for q in probs if len(q) >= k)
    assert most >= 3 * 200
    try:
        ctx.set_option("many_exhaustive_fused", 0)
        ctx.set_option("many_round_hypotheses", 200)
        cut = ctx.ransac_many_exhaustive(probs)
        ctx.set_option("many_round_hypotheses", 977)
        cut2 = ctx.ransac_many_exhaustive(probs)
    finally:
        ctx.set_option("many_round_hypotheses", 0)
        ctx.set_option("many_exhaustive_fused", 1)
    _same(full, cut, np.arange(n), np.arange(n), name)
    _same(full, cut2, np.arange(n), np.arange(n), name)


def test_context_state_untouched(ctx):
    data = _generate("ray", 30_000, 0.4, 5)
    _set(ctx, "ray").upload(data)
    r1 = ctx.ransac(0.999, seed=3)
    lib = ctx._lib
    assert lib.lsqr_count(ctx._h) == 30_000
    m1 = ctx.mask(r1["params"])
    probs, _, _, _ = _problems("ray", count=30, seed=6)
    _both_paths(ctx, probs)
    assert lib.lsqr_count(ctx._h) == 30_000
    fit1, _ = ctx.ls_fit(use_mask=True)   # the context's own mask is still the one set before the batched calls
    r2 = ctx.ransac(0.999, seed=3)
    assert r1["status"] == r2["status"] == L.OK
    assert r1["info"].iterations == r2["info"].iterations and r1["info"].best_index == r2["info"].best_index
    assert np.array_equal(r1["consensus"], r2["consensus"])
    assert np.array_equal(r1["params"], r2["params"])
    m2 = ctx.mask(r1["params"])
    assert m1[1] == m2[1] and np.array_equal(m1[0], m2[0])
    fit2, _ = ctx.ls_fit(use_mask=True)
    assert np.array_equal(fit1, fit2)


def _raw(ctx, recs, offs, nd, n=None, null=None):
    """lsqr_ransac_many_exhaustive on prefilled outputs, records nd doubles apart -> (status, outputs unchanged?)"""
    n = len(offs) - 1 if n is None else n
    m = max(len(offs) - 1, 1)
    params = np.full((m, 32), 7.0)
    cons = np.full(max(int(offs[-1]), 1), 9, dtype=np.uint8)
    infos = (L.RansacInfo * m)()
    for i in infos:
        i.iterations = 1234
    status = np.full(m, 99, dtype=np.int32)
    recs = np.ascontiguousarray(recs, dtype=np.float64)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    args = dict(recs=L.ptr(recs), offs=L.ptr(offs), params=L.ptr(params), infos=infos, status=L.ptr(status))
    if null:
        args[null] = None
    st = ctx._lib.lsqr_ransac_many_exhaustive(ctx._h, args["recs"], nd * 8, args["offs"], n, args["params"],
                                              L.ptr(cons), args["infos"], args["status"])
    untouched = (np.all(params == 7.0) and np.all(cons == 9) and np.all(status == 99)
                 and all(i.iterations == 1234 for i in infos))
    return st, untouched


def test_refusals_and_argument_errors(ctx):
    _set(ctx, "absor_w")
    assert ctx.ND == 7
    recs = _generate("absor_w", 30, 0.2, 9)
    st, untouched = _raw(ctx, recs, [0, 10, 30], 7)
    assert st == L.OK and not untouched
    st, untouched = _raw(ctx, recs[:, :6], [0, 10, 30], 6)   # a short stride: the weight slot missing
    assert st == L.ERR_INVALID and untouched
    assert b"lsqr_ransac_many_exhaustive" in ctx._lib.lsqr_last_error(ctx._h)
    st, untouched = _raw(ctx, recs, [1, 10, 30], 7)          # offsets[0] != 0
    assert st == L.ERR_INVALID and untouched
    st, untouched = _raw(ctx, recs, [0, 20, 10], 7)          # decreasing offsets
    assert st == L.ERR_INVALID and untouched
    for null in ("recs", "offs", "params", "infos", "status"):
        st, untouched = _raw(ctx, recs, [0, 10, 30], 7, null=null)
        assert st == L.ERR_INVALID and untouched, null
    st, untouched = _raw(ctx, recs, [0, 10, 30], 7, n=0)     # no problems: a no-op
    assert st == L.OK and untouched
    st, untouched = _raw(ctx, recs, [0, 10, 30], 7, n=0, null="params")
    assert st == L.OK and untouched
    for model, dim, ls in [(L.DENSE, 6, 0), (L.US_SINGLE, 0, L.LS_ITERATIVE), (L.US_POINTER, 0, L.LS_ITERATIVE),
                           (L.PHANTOM, 0, L.LS_ANALYTIC)]:
        ctx.set_model(model, dim, 2.0, ls)
        nd = ctx.ND
        st, untouched = _raw(ctx, np.zeros((30, nd)), [0, 10, 30], nd)
        assert st == L.ERR_INVALID and untouched, model
        assert b"lsqr_ransac_many_exhaustive" in ctx._lib.lsqr_last_error(ctx._h)
        with pytest.raises(L.LsqrError) as e:
            ctx.ransac_many_exhaustive([np.zeros((10, nd))])
        assert e.value.status == L.ERR_INVALID


def _rot(g):
    q = g.normal(size=4)
    s, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - s * z), 2 * (x * z + s * y)],
                     [2 * (x * y + s * z), 1 - 2 * (x * x + z * z), 2 * (y * z - s * x)],
                     [2 * (x * z - s * y), 2 * (y * z + s * x), 1 - 2 * (x * x + y * y)]])


def _hostile(name, kind, seed, n=14):
    """n records of unit scale with a clear answer; record 0 is an outlier made hostile: NaN, +-Inf or 1e9 away"""
    g = np.random.default_rng(seed)
    out = g.random(n) < 0.25
    out[0] = True
    if name in ("absor", "absor_w"):
        R, t = _rot(g), g.uniform(-1, 1, 3)
        first = g.uniform(-1, 1, (n, 3))
        second = first @ R.T + t + g.normal(0, 1e-3, (n, 3))
        second[out] += g.uniform(2.0, 5.0, (out.sum(), 3))
        rec = np.hstack([first, second] + ([g.uniform(0.5, 2.0, (n, 1))] if name == "absor_w" else []))
        slots = [0, 1, 2]
    elif name == "ray":
        target = g.uniform(-0.5, 0.5, 3)
        dirs = g.normal(size=(n, 3))
        dirs /= np.linalg.norm(dirs, axis=1)[:, None]
        p = target + dirs * g.uniform(1.0, 3.0, (n, 1))
        aim = target + g.normal(0, 1e-3, (n, 3))
        aim[out] += g.uniform(2.0, 5.0, (out.sum(), 3))
        d = aim - p
        rec = np.hstack([p, d / np.linalg.norm(d, axis=1)[:, None]])
        slots = [0, 1, 2]
    else:   # pivot
        tip, piv = np.array([0.1, -0.2, 0.3]), g.uniform(-0.5, 0.5, 3)
        rec = np.zeros((n, 13))
        for i in range(n):
            R = _rot(g)
            rec[i, :9], rec[i, 9:12] = R.ravel(), piv - R @ tip + g.normal(0, 1e-3, 3) + (3.0 if out[i] else 0.0)
        slots = [9, 10, 11]
    if kind == "nan":
        rec[0, slots[0]] = np.nan
    elif kind in ("+inf", "-inf"):
        rec[0, slots[0]] = np.inf if kind == "+inf" else -np.inf
    else:
        rec[0, slots] += 1e9
    return np.ascontiguousarray(rec), out


@pytest.mark.parametrize("name", ["absor", "absor_w", "ray", "pivot"])
def test_hostile_first_records(ctx, name):
    """the models whose fit origin is a record of the winning subset: a NaN, an infinite or a far first record never
    gives LSQR_OK with a non-finite parameter, on either path, and the answer is that of the clean records"""
    kinds = ["nan", "+inf", "-inf", "far"]
    made = [_hostile(name, kind, 40 + j) for j, kind in enumerate(kinds * 2)]
    probs = [m[0] for m in made]
    _set(ctx, name)
    res, general = _both_paths(ctx, probs)
    every = np.arange(len(probs))
    _same(res, general, every, every)
    offs = res["offsets"]
    for j in range(len(probs)):
        assert res["status"][j] != L.OK or np.all(np.isfinite(res["params"][j])), (j, res["params"][j])
        assert res["status"][j] == L.OK, j
        cons = res["consensus"][int(offs[j]):int(offs[j + 1])].astype(bool)
        assert not cons[0] and cons.sum() >= np.sum(~made[j][1]) - 1, (j, cons)
    assert _check_against_single(ctx, name, probs, CASES[name][5], res) == len(probs)
