"""The dense minimal solves and the closed-form fits through the C ABI on structured and badly scaled input
(tests/linalg_families.py): permutations, triangular and +-1 matrices, zero pivots, graded rows and columns, Hilbert,
and every system times 2^k.  The rule of tests/test_gpu_fit_origin.py, extended from hostile records to hostile
structure and scale: an entry point answers correctly or says it cannot, and never reports OK with a wrong answer.

The oracle is the reference only where it is right: its own SVD (the reference's) fails from 2^255 on exactly as the
library's did, so scaled systems are checked against the exact solution, which does not depend on the scale."""
import numpy as np
import pytest

import linalg_families as F
from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd.context import Context
from oracle import pyoracle as O
from test_gpu_fit_origin import MODELS, _blocks, _cloud, _ref_fit, _assert_close, _set

pytestmark = pytest.mark.gpu
DELTA = 0.1
SCALES = (-20, 20, 100, 255, 300, 500)
OPTIONS = [(fast, wave) for fast in (1, 0) for wave in (3, 1, 0)]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.set_option("dense_fast_solve", 1)
    c.set_option("dense_wave_solve", 3)
    c.close()


def _stack(n, k, singular):
    """rows: the stacked [A | b] 2^k of every member; subsets: each system with its rows in order, reversed, and in
    one seeded permutation; per subset the member's name, matrix, exact solution (None: exactly singular)."""
    members = [(name, a, b, x) for name, a, b, x in F.square(n)]
    if singular:
        members += [(name, a, b, None) for name, a, b in F.singular_square(n)]
    rows = np.vstack([np.hstack([F.scaled(a, k), F.scaled(b, k)[:, None]]) for _, a, b, _ in members])
    perm = np.random.default_rng(500 + n).permutation(n)
    subs, who = [], []
    for i, mem in enumerate(members):
        base = i * n + np.arange(n)
        for order in (base, base[::-1], base[perm]):
            subs.append(order)
            who.append(mem)
    return np.ascontiguousarray(rows), np.array(subs, dtype=np.uint32), who


def _solve_all(ctx, n, rows, subs):
    """{(fast, wave): (params, valid)} over the options matrix"""
    ctx.set_model(L.DENSE, n, DELTA).upload(rows)
    out = {}
    for fast, wave in OPTIONS:
        ctx.set_option("dense_fast_solve", fast)
        ctx.set_option("dense_wave_solve", wave)
        ctx.hypotheses_from_subsets(subs)
        par, valid, _ = ctx.hypotheses(votes=False)
        out[(fast, wave)] = (par.copy(), valid.copy())
    return out


def _wave_settings_identical(out, what):
    for fast in (1, 0):
        p3, v3 = out[(fast, 3)]
        for wave in (1, 0):
            p, v = out[(fast, wave)]
            assert np.array_equal(v, v3), (what, fast, wave)
            assert np.array_equal(p[v > 0].view(np.uint64), p3[v3 > 0].view(np.uint64)), (what, fast, wave)


def _check_exact(out, who, n, what, must_be_valid=True):
    bad = []
    for (fast, wave), (par, valid) in out.items():
        for h, (name, a, b, x) in enumerate(who):
            if x is None:
                continue
            if not valid[h]:
                if must_be_valid:
                    bad.append("%s fast=%d wave=%d %s[%d]: invalid" % (what, fast, wave, name, h % 3))
                continue
            err, bound = float(np.max(np.abs(par[h, :n] - x))), F.pinv_bound(a, x)
            if not (np.all(np.isfinite(par[h, :n])) and err <= bound):
                bad.append("%s fast=%d wave=%d %s[%d]: %.3e > %.3e" % (what, fast, wave, name, h % 3, err, bound))
    return bad


@pytest.mark.parametrize("n", F.SQUARE_N)
def test_dense_minimal_solves_on_structured_systems(ctx, n):
    """At the systems' own scale: validity is the oracle's, every regular member is valid and within the bound of
    tests/test_small_linalg.py of its exact solution under every option, the three dense_wave_solve settings are
    bit-identical, and the votes are the oracle's scan of the device's own parameters."""
    rows, subs, who = _stack(n, 0, singular=True)
    oc = O.cfg(O.DENSE, n, DELTA)
    out = _solve_all(ctx, n, rows, subs)
    _wave_settings_identical(out, "n=%d" % n)
    want_valid = np.array([len(O.estimate(oc, np.ascontiguousarray(rows[s]))) > 0 for s in subs])
    assert np.array_equal(want_valid, np.array([x is not None for _, _, _, x in who])), "the oracle on the families"
    for key, (par, valid) in out.items():
        assert np.array_equal(valid > 0, want_valid), (n, key, [who[h][0] for h in np.flatnonzero((valid > 0) != want_valid)])
    bad = _check_exact(out, who, n, "n=%d" % n)
    assert not bad, "%d: %s" % (len(bad), "; ".join(bad[:6]))
    for fast in (1, 0):
        ctx.set_option("dense_fast_solve", fast)
        ctx.set_option("dense_wave_solve", 3)
        ctx.hypotheses_from_subsets(subs)
        ctx.scan()
        par, valid, votes = ctx.hypotheses()
        for h in np.flatnonzero(valid):
            assert votes[h] == O.scan(oc, par[h], rows)[0], (n, fast, who[h][0])


@pytest.mark.parametrize("n", F.SQUARE_N)
def test_dense_minimal_solves_are_scale_free(ctx, n):
    """2^k [A | b] has the solution of [A | b]: every system valid and within the same bound for k = -20 ... 500 (the
    eliminations hand over to the SVD above 1e150, and the SVD's rotation test must not overflow); at k = -40 the
    reference's absolute 2.2e-16 threshold on the singular values may refuse, and the oracle says where."""
    bad = []
    for k in SCALES:
        rows, subs, who = _stack(n, k, singular=False)
        out = _solve_all(ctx, n, rows, subs)
        _wave_settings_identical(out, "n=%d 2^%d" % (n, k))
        bad += _check_exact(out, who, n, "n=%d 2^%d" % (n, k))
    rows, subs, who = _stack(n, -40, singular=False)
    oc = O.cfg(O.DENSE, n, DELTA)
    out = _solve_all(ctx, n, rows, subs)
    want_valid = np.array([len(O.estimate(oc, np.ascontiguousarray(rows[s]))) > 0 for s in subs])
    for key, (par, valid) in out.items():
        assert np.array_equal(valid > 0, want_valid), (n, key, "2^-40")
    bad += _check_exact(out, who, n, "n=%d 2^-40" % n, must_be_valid=False)
    assert not bad, "%d: %s" % (len(bad), "; ".join(bad[:6]))


@pytest.mark.parametrize("n", F.SQUARE_N)
def test_dense_many_entry_points_on_structured_problems(ctx, n):
    """The well-conditioned members (cond2 <= 1e3) as problems of exactly n records through ransac_many_dense and
    dense_fit_many: status and consensus follow the oracle's RANSAC, parameters within the README's 1e-6 of the
    exact solution."""
    mem = [(name, a, b, x) for name, a, b, x in F.square(n) if np.linalg.cond(a) <= 1e3]
    assert len(mem) >= 5
    probs = [np.ascontiguousarray(np.hstack([a, b[:, None]])) for _, a, b, _ in mem]
    seeds = 1 + np.arange(len(probs), dtype=np.uint64)
    ctx.set_model(L.DENSE, n, DELTA)
    res = ctx.ransac_many_dense(probs, 0.999, seeds=seeds)
    fit = ctx.dense_fit_many(probs)
    oc = O.cfg(O.DENSE, n, DELTA)
    offs = res["offsets"]
    for j, (name, a, b, x) in enumerate(mem):
        w = O.ransac(oc, probs[j], 0.999, sampler="ctr", seed=int(seeds[j]))
        what = (n, name)
        assert (res["status"][j] == L.OK) == (len(w["params"]) > 0), what
        assert np.array_equal(res["consensus"][int(offs[j]):int(offs[j + 1])], w["consensus"]), what
        assert res["status"][j] == L.OK and fit["status"][j] == L.OK, what
        tol = 1e-6 * max(1.0, float(np.max(np.abs(x))))
        assert np.max(np.abs(res["params"][j, :n] - x)) <= tol, what
        assert np.max(np.abs(fit["params"][j, :n] - x)) <= tol, what


# ---- closed-form fits at scale ---------------------------------------------------------------------------------------
FIT_SCALES = (-300, -100, 0, 100, 300)
# where a fit of records times 2^+-300 is EMPTY, the threshold that refuses it (measured; anything else fails the test)
REFUSED_BY = {}


def _scaled_params(name, par, k):
    """the k = 0 parameters of the records times 2^k: directions and quaternion unchanged, points, translation and
    radius times 2^k"""
    out = np.array(par, dtype=np.float64)
    for sl, unit in _blocks(name, MODELS[name][2]):
        if not unit:
            out[sl] = np.ldexp(out[sl], k)
    return out


@pytest.mark.parametrize("name", ["plane3", "plane5", "line3", "absor", "sphere3"])
def test_closed_form_fits_are_scale_free(ctx, name):
    rec, _ = _cloud(name, 96, 4242)
    _set(ctx, name).upload(rec)
    base, info = ctx.ls_fit()
    assert len(base) > 0, name
    _assert_close(name, base, _ref_fit(name, rec), "k = 0")
    for k in FIT_SCALES:
        if k == 0:
            continue
        _set(ctx, name).upload(np.ldexp(rec, k))
        got, info = ctx.ls_fit()
        print("%s 2^%d: %s" % (name, k, "OK" if len(got) else "EMPTY"))
        if len(got) == 0:
            assert abs(k) > 100, (name, k, "the fit must succeed")
            assert (name, k) in REFUSED_BY, (name, k, "EMPTY, and no threshold of the library accounts for it")
            continue
        want = _scaled_params(name, base, k)
        assert np.all(np.isfinite(got)), (name, k, got)
        for sl, unit in _blocks(name, MODELS[name][2]):
            g, w = got[sl], want[sl]
            if unit:
                g = g * (np.sign(g @ w) or 1.0)
            tol = 1e-6 if unit else 1e-6 * float(np.max(np.abs(w)))
            assert np.all(np.abs(g - w) <= tol), (name, k, got, want)
