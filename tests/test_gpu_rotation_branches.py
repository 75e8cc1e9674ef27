"""The angle-threshold branches of the rotation estimators on the device (run with -m gpu): the estimate kernels of the
absolute orientation (frame_quaternion, csrc/rigid.h), of the two US calibrations (USModel::finish, csrc/us.h) and of
the plane phantom (PhantomModel::finish, csrc/phantom.h) on the inputs of tests/rotation_families.py, against the CPU
oracle.  tests/test_rotation_branches.py holds the same inputs to the oracle and the host build of the same headers;
what differs here is the device build: contraction, operation order, sqrt, acos, atan2.

The sharpest probe is the exact half turn: whether trace(R) + 1 rounds to -1e-16 (a valid model of four NaN) or to
+1e-16 depends on the last bit of a three-term sum, so the NaN pattern of 256 hypotheses per upload is compared with
the oracle's bit for bit."""
import ctypes as C

import numpy as np
import pytest

import rotation_families as RF
from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd.context import Context
from oracle import pyoracle as O
from test_gpu_phantom_estimate import _dist
from test_gpu_ransac_many_exhaustive import _check_against_single as check_exhaustive_against_single
from test_gpu_ransac_many_rigid import _check_against_single as check_many_against_single
from test_rotation_branches import N_IN, N_PAIRS, singular

pytestmark = pytest.mark.gpu

REL = 1e-6  # tests/test_gpu_parity.py: the tolerance for estimated parameters
H_ABSOR, H_US, H_PHANTOM = 256, 128, 64
US_FRAMES, US_OUTLIERS, PHANTOM_FRAMES = 200, 30, 400


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------- absolute orientation
def absor_upload(rot, cloud_name):
    """64 pairs, 48 exact and 16 outliers, and 256 triples over all of them"""
    data, truth, _ = RF.absor_pairs(rot, cloud_name, N_PAIRS, 0.0, N_PAIRS - N_IN, seed=1)
    subs = O.ctr_subsets(91 + list(RF.ROTATIONS).index(rot), 0, H_ABSOR, N_PAIRS, 3)
    return data, subs


def _quat_close(got, want, tol=REL):
    s = 1.0 if got[:4] @ want[:4] >= 0 else -1.0   # q and -q are the same rotation
    assert np.allclose(s * got[:4], want[:4], rtol=tol, atol=tol), (got, want)
    assert np.allclose(got[4:], want[4:], rtol=tol, atol=tol * max(1.0, np.abs(want[4:]).max())), (got, want)


def _estimate_host(cfg, recs):
    r = np.ascontiguousarray(recs, dtype=np.float64)
    out = np.zeros(64)
    n = C.c_int(-1)
    st = L.load().lsqr_estimate_host(C.byref(cfg), L.ptr(r), r.shape[0], r.shape[1] * 8, L.ptr(out), C.byref(n))
    return st, out[:max(n.value, 0)].copy()


def test_absor_hypotheses_votes_winner_and_fit(ctx):
    """Every rotation of the family on a generic and on an integer cloud: per hypothesis the oracle's validity, the
    oracle's bits (NaN masks equal where the oracle has NaN), the oracle's votes (0 for a NaN model); best() never names
    a NaN hypothesis; the winner's mask is the oracle's; the Horn fit on it within REL of the oracle's up to sign;
    lsqr_estimate_host gives the device's bits.  The device must reach every branch: the counts below are the device's.
    Counted on the oracle over the 28 uploads x 256 triples: 1611 in the singular range, 235 valid with NaN, 5322
    regular; the device's counts must be the same, since every hypothesis has the oracle's bits."""
    oc = O.cfg(O.ABSOR, 3, 1.0)
    n_singular = n_nan = n_regular = 0
    side = {}
    for rot in RF.ROTATIONS:
        for cl in ("generic", "integer"):
            data, subs = absor_upload(rot, cl)
            ctx.set_model(L.ABSOR, 3, 1.0).upload(data)
            ctx.hypotheses_from_subsets(subs)
            ctx.scan()
            par, valid, votes = ctx.hypotheses()
            nan_h = np.zeros(H_ABSOR, bool)
            for h in range(H_ABSOR):
                want = O.estimate(oc, data[subs[h]])
                assert bool(valid[h]) == (len(want) > 0), (rot, cl, h)
                st, host = _estimate_host(ctx.cfg, data[subs[h]])
                assert (st == L.OK) == bool(valid[h]) and (st == L.OK or st == L.EMPTY), (rot, cl, h, st)
                if not valid[h]:
                    assert votes[h] == 0, (rot, cl, h)
                    continue
                nan = np.isnan(want)
                assert np.array_equal(np.isnan(par[h]), nan), (rot, cl, h, par[h], want)
                assert np.array_equal(par[h][~nan], want[~nan]), (rot, cl, h, par[h], want)
                assert np.array_equal(host, par[h], equal_nan=True), (rot, cl, h, host, par[h])
                if nan.any():
                    nan_h[h] = True
                    n_nan += 1
                    assert votes[h] == 0, (rot, cl, h, votes[h])
                    continue
                assert votes[h] == O.scan(oc, want, data)[0], (rot, cl, h)
                sing = singular(par[h])
                n_singular += sing
                n_regular += not sing
                if np.all(subs[h] < N_IN):   # a triple of exact pairs takes the branch of the true angle
                    side.setdefault(rot, set()).add(sing)
            packed, bv, bi = ctx.best()
            vv = np.where((valid > 0) & ~nan_h, votes, 0)
            assert bv == vv.max() and bi == int(np.argmax(vv)) and not nan_h[bi], (rot, cl, bi, bv)
            if not RF.in_singular_range(RF.ROTATIONS[rot][1]):   # (inside it the model is the mirrored rotation)
                assert bv >= N_IN - 1, (rot, cl, bv)
            m, cnt = ctx.mask_from_hypothesis(bi)
            wcnt, wmask = O.scan(oc, par[bi], data)
            assert cnt == wcnt == bv and np.array_equal(m, wmask), (rot, cl)
            fit, _ = ctx.ls_fit(use_mask=True)
            _quat_close(fit, O.ls(oc, data, wmask))
    print("device: singular", n_singular, "valid with NaN", n_nan, "regular", n_regular)
    assert n_singular >= 100 and n_nan >= 50 and n_regular >= 100
    for outside, inside in RF.THRESHOLD_PAIRS:
        assert side[outside] == {False} and side[inside] == {True}, (side[outside], side[inside])


def _absor_problems():
    """all rotations x 3 clouds, the uploads of the test above and a coplanar cloud: 42 problems of 64 pairs"""
    return [RF.absor_pairs(rot, cl, N_PAIRS, 0.0, N_PAIRS - N_IN, seed=1)[0]
            for rot in RF.ROTATIONS for cl in ("generic", "integer", "coplanar_tilted")]


def test_absor_ransac_many_decides_as_single_and_as_the_oracle(ctx):
    """the same problems through k_estimate_many (csrc/many.h): each decided as Context.ransac on its records alone,
    and as the serial loop of the oracle on the same subset stream"""
    probs = _absor_problems()
    seeds = 11 + 3 * np.arange(len(probs), dtype=np.uint64)
    res = ctx.set_model(L.ABSOR, 3, 1.0).ransac_many(probs, 0.999, seeds=seeds)
    assert np.all(res["status"] == L.OK), res["status"]
    check_many_against_single(ctx, "absor", probs, 3, res, seeds)
    oc = O.cfg(O.ABSOR, 3, 1.0)
    offs = res["offsets"]
    for j, p in enumerate(probs):
        w = O.ransac(oc, p, 0.999, sampler="ctr", seed=int(seeds[j]))
        assert res["iterations"][j] == w["iters"] and res["best_index"][j] == w["best_iter"], j
        assert np.array_equal(res["consensus"][int(offs[j]):int(offs[j + 1])], w["consensus"]), j
        assert not np.isnan(res["params"][j]).any(), j
        _quat_close(res["params"][j], w["params"])


def test_absor_ransac_many_exhaustive_decides_as_single_and_as_the_oracle(ctx):
    """8 pairs per problem (6 exact, 2 outliers), all 56 triples, through csrc/many_exhaustive.h: as
    Context.ransac_exhaustive on the records alone, and the oracle's exhaustive loop: a NaN model never wins"""
    probs = [np.ascontiguousarray(np.vstack([p[:6], p[-2:]])) for p in _absor_problems()]
    ctx.set_model(L.ABSOR, 3, 1.0)
    res = ctx.ransac_many_exhaustive(probs)
    assert np.all(res["status"] == L.OK), res["status"]
    assert check_exhaustive_against_single(ctx, "absor", probs, 3, res) == len(probs)
    oc = O.cfg(O.ABSOR, 3, 1.0)
    offs = res["offsets"]
    for j, p in enumerate(probs):
        w = O.ransac_exhaustive(oc, p)
        assert res["fraction"][j] == w["fraction"], (j, res["fraction"][j], w["fraction"])
        assert np.array_equal(res["consensus"][int(offs[j]):int(offs[j + 1])], w["consensus"]), j
        assert not np.isnan(res["params"][j]).any(), j
        _quat_close(res["params"][j], w["params"])


# ------------------------------------------------------------------------------------------- US calibration
US_CASES = [(name, 0.0) for name in RF.OMEGA_Y] + [("plus_half_pi", 0.5), ("minus_half_pi", 0.5)]


def us_case(kind, name, sigma):
    """200 frames, the last 30 outliers, 128 minimal subsets -> (oracle model, records, subsets, k)"""
    model = O.US_SINGLE if kind == "single" else O.US_POINTER
    k = 4 if kind == "single" else 3
    rec, _, _ = RF.us_frames(kind, RF.omegas(name), US_FRAMES, sigma, US_OUTLIERS, seed=2)
    subs = O.ctr_subsets(23, 0, H_US, US_FRAMES, k)
    return model, rec, subs, k


def on_threshold(omega_y):
    """the oracle's omega_y within 1e-6 of the end of the gimbal range: either formula may be taken"""
    return abs(abs(abs(omega_y) - RF.HALF_PI) - RF.SMALL_ANGLE) < 1e-6


def us_deviation(o, got, want):
    """the largest deviation of the parameters in units of the tolerance of tests/test_gpu_parity.py
    (test_us_hypotheses_scan_mask: |got - want| <= REL max |want| + REL |want|), the three angles modulo 2 pi against
    REL max(1, |want|): within tolerance when <= 1"""
    ang = [o + 3, o + 4, o + 5]
    rest = [j for j in range(len(want)) if j not in ang]
    d = np.abs(got[rest] - want[rest]) / (REL * np.abs(want[rest]).max() + REL * np.abs(want[rest]))
    a = RF.angle_diff(got[ang], want[ang]) / (REL * np.maximum(1.0, np.abs(want[ang])))
    return float(max(d.max(), a.max()))


@pytest.mark.parametrize("name,sigma", US_CASES)
@pytest.mark.parametrize("kind", ["single", "pointer"])
def test_us_estimate_at_gimbal_lock(ctx, kind, name, sigma):
    """K1 of the US calibrations (both solvers: us_fast_solve 1 and 0) per hypothesis against the oracle: validity,
    the same branch (omega_z == 0.0 on both or on neither), parameters within REL, votes of the device's own
    parameters; then the analytic fit of the winner's consensus set against the oracle's, the same checks.
    Noise-free, every subset of inlier frames takes the branch of the true omega_y; with 0.5 px noise at +-pi/2 one
    batch holds both (on the oracle, of the 66 subsets of inlier frames of the single-target variant 36 / 34 gimbal and
    30 / 32 regular, of the pointer's 81 subsets 64 and 17).  A hypothesis whose omega_y the oracle puts within 1e-6 of
    the range's end is skipped; at most 2 % may be (0 of 128 on these seeds, in every case).
    Measured on an MI355X, worst over the 44 runs: hypotheses 3.3e-4 of the tolerance (3.3e-10 relative), fits 1.3e-7
    of it; the device took the oracle's branch on every hypothesis."""
    model, rec, subs, k = us_case(kind, name, sigma)
    o = 3 if kind == "single" else 0
    oc = O.cfg(model, 0, 3.0, 0)
    wants = [O.estimate(oc, rec[s]) for s in subs]
    inside_truth = RF.in_gimbal_range(RF.OMEGA_Y[name])
    for fast in (1, 0):
        try:
            ctx.set_option("us_fast_solve", fast)
            ctx.set_model(model, 0, 3.0, L.LS_ANALYTIC).upload(rec)
            ctx.hypotheses_from_subsets(subs)
            ctx.scan()
            par, valid, votes = ctx.hypotheses()
            _, bv, bi = ctx.best()
            m, cnt = ctx.mask_from_hypothesis(bi)
            fit, _ = ctx.ls_fit(use_mask=True)
        finally:
            ctx.set_option("us_fast_solve", 1)
        skipped = n_gimbal = n_regular = 0
        worst = 0.0
        for h in range(H_US):
            want = wants[h]
            assert bool(valid[h]) == (len(want) > 0), (kind, name, fast, h)
            if not valid[h]:
                assert votes[h] == 0
                continue
            assert votes[h] == O.scan(oc, par[h], rec)[0], (kind, name, fast, h)
            if on_threshold(want[o + 4]):
                skipped += 1
                continue
            gimbal = par[h][o + 3] == 0.0
            assert gimbal == (want[o + 3] == 0.0), (kind, name, fast, h, par[h][o + 3:o + 6], want[o + 3:o + 6])
            d = us_deviation(o, par[h], want)
            worst = max(worst, d)
            assert d <= 1.0, (kind, name, fast, h, d, par[h], want)
            if np.all(subs[h] < US_FRAMES - US_OUTLIERS):
                n_gimbal += gimbal
                n_regular += not gimbal
                if sigma == 0.0:
                    assert gimbal == inside_truth, (kind, name, fast, h)
        print(kind, name, sigma, "fast", fast, "inlier subsets: gimbal", n_gimbal, "regular", n_regular, "skipped", skipped,
              "worst deviation / tolerance", worst)
        assert skipped <= 0.02 * H_US
        assert n_gimbal + n_regular >= 40
        if sigma > 0:
            assert n_gimbal >= 15 and n_regular >= 15, (n_gimbal, n_regular)   # one batch mixes both branches
        # the winner and the analytic fit of its consensus set
        wcnt, wmask = O.scan(oc, par[bi], rec)
        assert cnt == wcnt == bv and np.array_equal(m, wmask) and bv >= 0.8 * (US_FRAMES - US_OUTLIERS)
        want = O.us_analytic(model, np.ascontiguousarray(rec[wmask.astype(bool)]))
        assert len(fit) == len(want) > 0, (kind, name, fast)
        if not on_threshold(want[o + 4]):
            assert (fit[o + 3] == 0.0) == (want[o + 3] == 0.0), (kind, name, fast, fit[o + 3:o + 6], want[o + 3:o + 6])
            d = us_deviation(o, fit, want)
            print(kind, name, sigma, "fast", fast, "fit deviation / tolerance", d)
            assert d <= 1.0, (kind, name, fast, d, fit, want)


# ------------------------------------------------------------------------------------------- plane phantom
@pytest.mark.parametrize("name", list(RF.OMEGA_Y))
def test_phantom_estimate_at_gimbal_lock(ctx, name):
    """the plane phantom's minimal solves, omega3_y over the family: the Jacobi SVD (phantom_fast_solve 0) and the LU
    path (1) against each other and against the oracle's SVD within 1e-7 (tests/test_gpu_phantom_estimate.py: _dist),
    the branch marker omega3_z == 0.0 alike on all three.  Measured on an MI355X: worst distance 1.7e-11 (at the two
    cases just outside the range, where omega3_z and omega3_x divide by cos omega3_y = 8.6e-3), 1.4e-12 elsewhere."""
    rec, truth, _ = RF.phantom_frames(RF.OMEGA1_YX, RF.omegas(name), PHANTOM_FRAMES, seed=6)
    oc = O.cfg(O.PHANTOM, 0, 2.0, 0)
    subs = O.ctr_subsets(29, 0, H_PHANTOM, PHANTOM_FRAMES, 31)
    out = []
    for fast in (0, 1):
        try:
            ctx.set_option("phantom_fast_solve", fast)
            ctx.set_model(L.PHANTOM, 0, 2.0, L.LS_ANALYTIC).upload(rec)
            ctx.hypotheses_from_subsets(subs)
            out.append(ctx.hypotheses(votes=False)[:2])
        finally:
            ctx.set_option("phantom_fast_solve", 1)
    (pj, vj), (pf, vf) = out
    assert np.array_equal(vj, vf) and vj.sum() >= H_PHANTOM - 2, (vj.sum(), vf.sum())
    inside = RF.in_gimbal_range(RF.OMEGA_Y[name])
    worst = 0.0
    for h in np.flatnonzero(vj):
        want = O.estimate(oc, rec[subs[h]])
        assert len(want) == 41, (name, h)
        assert (want[6] == 0.0) == inside and (pj[h][6] == 0.0) == inside and (pf[h][6] == 0.0) == inside, (name, h)
        d = max(_dist(want, pj[h]), _dist(want, pf[h]), _dist(pj[h], pf[h]))
        worst = max(worst, d)
        assert d < 1e-7, (name, h, d)
    print(name, "worst distance", worst)
