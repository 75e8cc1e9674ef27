"""The angle-threshold branches of the rotation estimators on the CPU: the product's headers compiled for the host
(tests/host_math/driver.cpp: csrc/rigid.h, us.h, phantom.h) against the oracle, and the oracle against an independent
reference, on the rotations of tests/rotation_families.py -- exact half turns, the 0.5 degree singular range of
Frame::getRotationQuaternion around them, and Euler angles with omega_y at +-pi/2.

What the reference does there, and the tests pin ("Rotations at half turns and at gimbal lock"):
  * at an exact half turn trace(R) + 1 rounds to about -1e-16 for some minimal triples: sqrt gives NaN, the NaN fails
    the range test, the regular formula divides by NaN, and estimate() reports success with four NaN entries;
  * inside the singular range the formula has no sign of s: a rotation by pi + x comes back as pi - x;
  * at omega_y ~ -pi/2 the Euler angles are taken by the +pi/2 formula and describe another rotation; the derived
    products that agree() reads are right."""
import ctypes as C

import numpy as np
import pytest

import rotation_families as RF
from lsqrrecipes_amd import synth
from oracle import pyoracle as O
from test_host_math import hm, _p  # noqa: F401  (the host build of the product's headers, as a fixture)

N_PAIRS, N_IN, N_TRIPLES = 64, 48, 100
TRIPLE_CLOUDS = ("generic", "integer")


def absor_problem(rot, cloud_name):
    """64 pairs, the last 16 outliers, and 100 triples of the 48 exact ones -> (records, truth, subsets)"""
    data, truth, _ = RF.absor_pairs(rot, cloud_name, N_PAIRS, 0.0, N_PAIRS - N_IN, seed=1)
    subs = O.ctr_subsets(41 + list(RF.ROTATIONS).index(rot), 0, N_TRIPLES, N_IN, 3)
    return data, truth, subs


def singular(par):
    """did frame_quaternion take the singular-range formula for this estimate (a NaN s takes the regular one)"""
    with np.errstate(invalid="ignore"):
        half = np.arccos(par[0])
    return bool(half > RF.HALF_PI - RF.SMALL_ANGLE and half < RF.HALF_PI + RF.SMALL_ANGLE)


@pytest.fixture(scope="module")
def oracle_estimates():
    """{(rotation, cloud): (records, truth, subsets, [oracle parameters per triple])}, computed once"""
    oc = O.cfg(O.ABSOR, 3, 1.0)
    out = {}
    for rot in RF.ROTATIONS:
        for cl in TRIPLE_CLOUDS:
            data, truth, subs = absor_problem(rot, cl)
            out[rot, cl] = (data, truth, subs, [O.estimate(oc, data[s]) for s in subs])
    return out


def test_absor_host_arithmetic_equals_the_oracle(hm, oracle_estimates):
    """rigid.h on the host == oracle/estimators.c: estimate() in validity, NaN pattern and bits, agree() masks, and
    the Horn fit on shifted moments within 1e-9 of the oracle's un-shifted one (quaternion up to sign).
    Branch coverage of the families, counted on the oracle (2800 triples: 14 rotations x 2 clouds x 100):
    singular range 1364, valid with NaN 236, regular 1200; worst |fit - oracle fit| 1.3e-15.
    (A host build with fused multiply-adds, -ffp-contract=fast, differs from the oracle in the NaN pattern of 189 of
    these triples and in the bits of 2522 more: the comparison does see contraction.)"""
    oc = O.cfg(O.ABSOR, 3, 1.0)
    n_singular = n_nan = n_regular = 0
    worst_ls = 0.0
    side = {}
    for (rot, cl), (data, truth, subs, wants) in oracle_estimates.items():
        for s, want in zip(subs, wants):
            recs = np.ascontiguousarray(data[s])
            got = np.full(7, 7.0)
            n = hm.hm_estimate(O.ABSOR, 3, C.c_double(1.0), _p(recs), _p(got))
            assert n == len(want), (rot, cl, s)
            if n == 0:
                continue
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan), (rot, cl, s, got, want)
            assert np.array_equal(got[~nan], want[~nan]), (rot, cl, s, got, want)
            mask = np.zeros(len(data), dtype=np.uint8)
            assert hm.hm_agree(O.ABSOR, 3, C.c_double(1.0), _p(got), _p(data), len(data), _p(mask))
            cnt, omask = O.scan(oc, want, data)
            assert np.array_equal(mask, omask), (rot, cl, s)
            if nan.any():
                n_nan += 1
                assert nan[:4].all() and cnt == 0   # the quaternion is lost as a whole; nothing agrees with it
                continue
            sing = singular(want)
            n_singular += sing
            n_regular += not sing
            side.setdefault(rot, set()).add(sing)
            assert cnt >= N_IN - 1 or sing, (rot, cl, s, cnt)   # a regular-range model of exact pairs holds them all
            if cnt < 3:
                continue
            want_ls = O.ls(oc, data, omask)
            got_ls = np.zeros(7)
            org = np.ascontiguousarray(data[s[0]])
            assert hm.hm_ls(O.ABSOR, 3, C.c_double(1.0), _p(data), len(data), _p(omask), _p(org), _p(got_ls), None) == 7
            sgn = 1.0 if got_ls[:4] @ want_ls[:4] >= 0 else -1.0
            d = max(np.abs(sgn * got_ls[:4] - want_ls[:4]).max(),
                    np.abs(got_ls[4:] - want_ls[4:]).max() / max(1.0, np.abs(want_ls[4:]).max()))
            worst_ls = max(worst_ls, d)
            assert d <= 1e-9, (rot, cl, s, got_ls, want_ls)
    print("singular", n_singular, "valid with NaN", n_nan, "regular", n_regular, "worst ls", worst_ls)
    assert n_singular >= 100 and n_nan >= 50 and n_regular >= 100
    for outside, inside in RF.THRESHOLD_PAIRS:
        assert side[outside] == {False} and side[inside] == {True}, (side[outside], side[inside])
    for rot, (q, theta) in RF.ROTATIONS.items():   # every family takes the branch its angle says
        if rot in side:
            assert side[rot] == {RF.in_singular_range(theta)}, (rot, side[rot])


def test_absor_library_host_estimate_equals_the_oracle(oracle_estimates):
    """lsqr_estimate_host (the library's own host build of rigid.h, what the C++ drop-in's estimate() calls): the
    oracle's bits and NaN pattern on every triple, LSQR_OK for the valid NaN models as the reference's "success\""""
    from lsqrrecipes_amd import _lib as L
    cfg = L.ModelCfg(L.ABSOR, 3, 1.0, 0, 0, 0.0)
    n_nan = 0
    for (rot, cl), (data, truth, subs, wants) in oracle_estimates.items():
        for s, want in zip(subs, wants):
            r = np.ascontiguousarray(data[s])
            out, n = np.zeros(16), C.c_int(-1)
            st = L.load().lsqr_estimate_host(C.byref(cfg), L.ptr(r), 3, 48, L.ptr(out), C.byref(n))
            assert (st == L.OK and n.value == 7) if len(want) else (st == L.EMPTY and n.value == 0), (rot, cl, s, st)
            if len(want):
                assert np.array_equal(out[:7], want, equal_nan=True), (rot, cl, s, out[:7], want)
                n_nan += bool(np.isnan(want).any())
    assert n_nan >= 50


def test_absor_estimate_rebuilds_the_rotation(oracle_estimates):
    """The rotation rebuilt from estimate()'s parameters against the truth: within 1e-9 outside the singular range.
    Inside it the bound is 2 |pi - theta| + 1e-6, and that is the reference's own loss, not rounding: the singular-range
    formula of Frame::getRotationQuaternion takes the vector part from the symmetric part of R, which cannot tell
    theta = pi + x from pi - x, and keeps s >= 0 -- the rotation comes back mirrored about the half turn (2 x apart),
    and at the half turn itself s = 0.5 sqrt(trace + 1) is the root of a rounding error (about 2e-8).
    Measured worst: 2.7e-11 outside (bound 1e-9); inside 8.1e-3 at theta = pi + 5e-3 (bound 1.0e-2 + 1e-6), 1.1e-7 at
    the exact half turns (bound 1e-6).  NaN models (236 of 2800) are excluded and counted."""
    worst_out = worst_in = worst_half = 0.0
    n_nan = n_checked = 0
    for (rot, cl), (data, truth, subs, wants) in oracle_estimates.items():
        theta = RF.ROTATIONS[rot][1]
        R = synth.quat_to_matrix(truth[:4])
        for want in wants:
            if len(want) == 0:
                continue
            if np.isnan(want).any():
                n_nan += 1
                continue
            n_checked += 1
            d = np.abs(synth.quat_to_matrix(want[:4]) - R).max()
            t = np.abs(want[4:] - truth[4:]).max()
            if singular(want):
                bound = 2.0 * abs(np.pi - theta) + 1e-6
                worst_in = max(worst_in, d)
                if rot in RF.HALF_TURNS:
                    worst_half = max(worst_half, d)
            else:
                bound = 1e-9
                worst_out = max(worst_out, d)
            assert d <= bound, (rot, cl, d, bound)
            assert t <= 200.0 * bound, (rot, cl, t)   # t = mean2 - R mean1, |mean1| <= 100 sqrt(3)
    print("outside", worst_out, "inside", worst_in, "half turns", worst_half, "NaN", n_nan, "checked", n_checked)
    assert n_nan >= 50 and n_checked >= 2000


def kabsch(first, second):
    """the least-squares rotation by the SVD of the centred cross-covariance, accumulated in longdouble
    -> (R, t, rms residual)"""
    l = first.astype(np.longdouble)
    r = second.astype(np.longdouble)
    ml, mr = l.mean(axis=0), r.mean(axis=0)
    H = ((l - ml).T @ (r - mr)).astype(np.float64)       # sum (l - ml)(r - mr)^T
    scale = np.abs(H).max()
    U, _, Vt = np.linalg.svd(H / scale)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    t = (mr - R.astype(np.longdouble) @ ml).astype(np.float64)
    return R, t, rms(R, t, first, second)


def rms(R, t, first, second):
    res = (first.astype(np.longdouble) @ R.astype(np.longdouble).T + t.astype(np.longdouble)) - second
    return float(np.sqrt((res * res).sum() / len(first)))


def test_oracle_horn_fit_against_kabsch():
    """The oracle's leastSquaresEstimate (Horn's quaternion method) against Kabsch's SVD with longdouble sums, for
    every rotation x cloud x n in {3, 4, 50} x sigma in {0, 0.3}: max |R - R_kabsch| <= 1e-9, | |q| - 1 | <= 1e-14,
    RMS residual not above Kabsch's by more than 1e-12 x extent.
    Measured worst: |R - R_kabsch| 4.4e-15 on the generic and integer clouds, 1.6e-13 on the coplanar and scaled ones;
    | |q| - 1 | 8.9e-16; excess RMS 3.5e-15 x extent."""
    oc = O.cfg(O.ABSOR, 3, 1.0)
    worst = {"plain": 0.0, "flat": 0.0}
    worst_q = worst_rms = 0.0
    for rot in RF.ROTATIONS:
        for cl in RF.CLOUDS:
            for n in (3, 4, 50):
                for sigma in (0.0, 0.3):
                    data, truth, _ = RF.absor_pairs(rot, cl, n, sigma, 0, seed=7 + n)
                    first, second = data[:, :3], data[:, 3:]
                    assert np.linalg.matrix_rank(first - first.mean(axis=0)) >= 2   # not collinear
                    got = O.ls(oc, data)
                    assert len(got) == 7, (rot, cl, n, sigma)
                    Rk, tk, rk = kabsch(first, second)
                    qn = np.linalg.norm(got[:4])
                    R = synth.quat_to_matrix(got[:4])
                    d = np.abs(R - Rk).max()
                    ext = RF.cloud_extent(cl)
                    excess = (rms(R, got[4:], first, second) - rk) / ext
                    key = "plain" if cl in ("generic", "integer") else "flat"
                    worst[key] = max(worst[key], d)
                    worst_q = max(worst_q, abs(qn - 1.0))
                    worst_rms = max(worst_rms, excess)
                    assert d <= 1e-9, (rot, cl, n, sigma, d)
                    assert abs(qn - 1.0) <= 1e-14, (rot, cl, n, sigma, qn)
                    assert excess <= 1e-12, (rot, cl, n, sigma, excess)
                    if sigma == 0.0:
                        assert np.abs(R - synth.quat_to_matrix(truth[:4])).max() <= 1e-9, (rot, cl, n)
    print("worst |R - R_kabsch|", worst, "| |q| - 1 |", worst_q, "excess rms / extent", worst_rms)


def _us_finish(hm, kind, x):
    par = np.zeros(20 if kind == "single" else 17)
    assert hm.hm_us_finish(int(kind == "single"), _p(np.ascontiguousarray(x)), _p(par)) == len(par)
    return par


def _euler_bound(omega_y, name):
    """max |euler_zyx(angles) - R| the reference's formulas allow at a POSITIVE omega_y.  Regular formulas and the
    exact quarter turn: rounding (1e-9).  Strictly inside the gimbal range the reference sets omega_z = 0 and takes
    omega_x = atan2(R01, R11), which is the rotation only for cos(omega_y) = 0: the first column and the last row
    (cos(omega_y) times sines and cosines of omega_z, omega_x against those of 0, omega_x') move by up to
    2 cos(omega_y), the other four entries by (1 - sin(omega_y)) <= cos(omega_y)^2 times a few."""
    c = abs(np.cos(omega_y))
    if not RF.in_gimbal_range(omega_y) or name == "plus_half_pi":
        return 1e-9
    return 2.0 * c + 4.0 * c * c + 1e-9


@pytest.mark.parametrize("kind", ["single", "pointer"])
def test_us_finish_at_gimbal_lock(hm, kind):
    """USModel::finish on the exact solution vector of every omega_y of the family: omega_z is exactly 0.0 inside the
    branch and non-zero outside; the derived products (what agree() reads) equal the truth to 1e-12 in both; at
    positive omega_y the angles rebuild R (1e-9 with the regular formulas and at the exact quarter turn, the
    reference's own O(cos omega_y) inside the range: _euler_bound).  At negative omega_y inside the range the angles
    are the oracle's -- and do NOT rebuild R: omega_x = atan2(R01, R11) is the +pi/2 formula (-(omega_x + omega_z)
    instead of omega_x + omega_z).
    Measured: products 1.7e-16; rebuilt R 0 (regular), 1.1e-16 (+pi/2), 6.4e-4 at pi/2 - 1e-3 (bound 2.0e-3), 5.6e-3
    at pi/2 - 8.6e-3 (bound 1.8e-2); at -pi/2 |euler(angles) - R| = 1.95; angles against the oracle's 7.9e-14."""
    model = O.US_SINGLE if kind == "single" else O.US_POINTER
    o = 3 if kind == "single" else 0
    reached = set()
    for name, wy in RF.OMEGA_Y.items():
        frames, truth, _ = RF.us_frames(kind, RF.omegas(name), 40, seed=3)
        par = _us_finish(hm, kind, RF.us_solution(kind, truth))
        R = synth.euler_zyx(*RF.omegas(name))
        inside = RF.in_gimbal_range(wy)
        assert (par[o + 3] == 0.0) == inside, (name, par[o + 3])
        reached.add((inside, wy > 0))
        prod = np.concatenate([RF.MX * R[:, 0], RF.MY * R[:, 1], R[:, 2]])
        dprod = np.abs(par[o + 8:o + 17] - prod).max()
        assert dprod <= 1e-12, (name, dprod)
        assert np.array_equal(par[:o + 3], truth[:o + 3]) and abs(par[o + 4] - wy) <= 1e-9
        assert np.allclose(par[o + 6:o + 8], [RF.MX, RF.MY], rtol=1e-12, atol=0)
        back = np.abs(synth.euler_zyx(*par[o + 3:o + 6]) - R).max()
        want = O.us_analytic(model, frames)             # the oracle on 40 exact frames of the same calibration
        assert len(want) == len(par)
        dang = RF.angle_diff(par[o + 3:o + 6], want[o + 3:o + 6]).max()
        print(kind, name, "products", dprod, "rebuilt R", back, "angles vs oracle", dang)
        assert (want[o + 3] == 0.0) == inside, name
        assert dang <= 1e-9, (name, par[o + 3:o + 6], want[o + 3:o + 6])
        if wy > 0 or not inside:
            assert back <= _euler_bound(wy, name), (name, back)
        else:
            assert back > 0.5, (name, back)             # the reference's angles describe another rotation
            assert abs(RF.angle_diff(par[o + 5], -(RF.OMEGA_X + RF.OMEGA_Z))) <= 2e-2, (name, par[o + 5])
    assert reached == {(True, True), (True, False), (False, True), (False, False)}


def test_phantom_finish_at_gimbal_lock(hm):
    """PhantomModel::finish on the exact null vector, omega3_y over the family, omega1 generic (0.4, 0.3): the same
    claims as for the US calibration; the derived products 11..40 to 1e-12 relative to max(1, |entry|) (the entries
    t3 R1 reach 100).
    Measured: products 2.8e-17; rebuilt R 1.7e-16 (regular), 6.4e-4 at pi/2 - 1e-3; at -pi/2 |euler(angles) - R| =
    1.95; angles against the oracle's 3.3e-13."""
    reached = set()
    for name, wy in RF.OMEGA_Y.items():
        frames, truth, _ = RF.phantom_frames(RF.OMEGA1_YX, RF.omegas(name), 80, seed=5)
        for sgn in (1.0, -1.0):
            out = np.zeros(41)
            assert hm.hm_phantom_finish(_p(np.ascontiguousarray(sgn * RF.phantom_solution(truth))), _p(out)) == 41
            R = synth.euler_zyx(*RF.omegas(name))
            inside = RF.in_gimbal_range(wy)
            assert (out[6] == 0.0) == inside, (name, out[6])
            reached.add((inside, wy > 0))
            dprod = (np.abs(sgn * out[11:41] - truth[11:41]) / np.maximum(1.0, np.abs(truth[11:41]))).max()
            assert dprod <= 1e-12, (name, dprod)
            assert np.allclose(out[3:6], truth[3:6], rtol=1e-12, atol=1e-12) and abs(out[7] - wy) <= 1e-9
            assert np.allclose(out[9:11], [RF.MX, RF.MY], rtol=1e-12, atol=0)
            back = np.abs(synth.euler_zyx(*out[6:9]) - R).max()
            if wy > 0 or not inside:
                assert back <= _euler_bound(wy, name), (name, back)
            else:
                assert back > 0.5, (name, back)
        want = O.phantom_analytic(frames)               # the oracle on 80 exact frames
        assert len(want) == 41
        dang = RF.angle_diff(out[6:9], want[6:9]).max()
        print(name, "products", dprod, "rebuilt R", back, "angles vs oracle", dang)
        assert (want[6] == 0.0) == inside, name
        assert dang <= 1e-9, (name, out[6:9], want[6:9])
    assert reached == {(True, True), (True, False), (False, True), (False, False)}


def test_rigid_models_host_arithmetic_on_generic_data(hm):
    """pivot calibration, ray intersection and the 2-D line through the host build (they had no CPU unit test):
    estimate() against the oracle (bit for bit where the arithmetic is restated literally, 1e-9 for the pivot's
    pseudo-inverse), agree() masks bit for bit, the fit within 1e-9."""
    aux = 0.017453292519943295
    hm.hm_set_aux.argtypes = [C.c_double]
    cases = [(O.PIVOT, 3, 1.0, synth.pivot(300, 0.3, seed=3)[0], 0.0, False),
             (O.RAY, 3, 1.0, synth.rays(300, 0.3, seed=4)[0], aux, True),
             (O.LINE2D, 2, 0.5, synth.plane(300, 0.3, seed=5, dim=2)[0], 0.0, True)]
    for model, dim, delta, data, a, exact in cases:
        hm.hm_set_aux(a)
        oc = O.cfg(model, dim, delta, 0, aux=a)
        k, P = O.lib().orc_min_subset(oc), O.lib().orc_num_params(oc)
        best, checked = None, 0
        for s in O.ctr_subsets(17, 0, 60, len(data), k):
            recs = np.ascontiguousarray(data[s])
            want = O.estimate(oc, recs)
            got = np.zeros(P)
            assert hm.hm_estimate(model, dim, C.c_double(delta), _p(recs), _p(got)) == len(want), (model, s)
            if len(want) == 0:
                continue
            if exact:
                assert np.array_equal(got, want), (model, s)
            else:
                assert np.allclose(got, want, rtol=1e-9, atol=1e-9), (model, s)
            mask = np.zeros(len(data), dtype=np.uint8)
            assert hm.hm_agree(model, dim, C.c_double(delta), _p(got), _p(data), len(data), _p(mask))
            cnt, omask = O.scan(oc, got, data)
            assert np.array_equal(mask, omask), (model, s)
            checked += 1
            if best is None or cnt > best[0]:
                best = (cnt, omask, s)
        assert checked >= 30 and best[0] > 150, (model, checked, best[0])
        want = O.ls(oc, data, best[1])
        got = np.zeros(P)
        org = np.ascontiguousarray(data[best[2][0]])
        assert hm.hm_ls(model, dim, C.c_double(delta), _p(data), len(data), _p(best[1]), _p(org), _p(got), None) == P
        if model == O.LINE2D:
            sgn = 1.0 if got[:2] @ want[:2] >= 0 else -1.0
            assert np.allclose(sgn * got[:2], want[:2], rtol=0, atol=1e-9)
            assert abs((got[2:] - want[2:]) @ want[:2]) <= 1e-9 * max(1.0, np.abs(want[2:]).max())
        else:
            assert np.allclose(got, want, rtol=1e-9, atol=1e-9), (model, got, want)
    hm.hm_set_aux(0.0)
