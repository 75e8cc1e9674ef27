"""Every driver of the iterative least-squares fit (lsqr_hip.hip: run_fit and its lm_fit_*), pinned on the same inputs.

The Levenberg-Marquardt fit of the geometric sphere and of the two US calibrations has five ways through the library:
one launch per evaluation with the host's step (the default once `lm_persist` is 0; its pass is the matrix-core kernel
over tiles, the matrix-core kernel over records (`lm_tiles` 0) or the per-lane kernel (`lm_mfma` 0, and every sphere)),
the host's step through staged copies (`lm_fused` 0), and the step in a device kernel (`lm_host` 0).  `mom_chunk` 1
cuts the moment passes of the algebraic start into the smallest blocks.  Each option set is held to the CPU oracle at
the tolerances of tests/test_gpu_parity.py (test_sphere_lm_info_and_cost, test_us_least_squares), and the option sets
are held to each other: to the bit where they walk through the same sums, else to the same MINPACK stopping code
(INFO_EXCEPTIONS lists the three runs that stop with another one).

Sizes: one record (no sphere through one point: an empty fit), one block less one / exactly / plus one record, several
blocks, and 1024 x 2048 + 1 records, where the per-lane pass reaches its cap of kMaxPartials blocks.  A masked sphere
fit starts THROUGH the mask and compacts the consensus set once eight evaluations are spent (lm_fit_fused:
kCompactAfter); the noisy cap below is the input that needs more than eight.  Four US cases start at gimbal lock
(omega_y = +-pi/2, tests/rotation_families.py), where the Jacobian is rank deficient to rounding."""
import ctypes as C

import numpy as np
import pytest

import rotation_families as RF
from lsqrrecipes_amd import _lib as L, synth
from lsqrrecipes_amd.context import Context
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu

REL = 1e-6  # tests/test_gpu_parity.py: the tolerance for estimated parameters

# every set on top of `lm_persist` 0 (the persistent kernel has tests/test_gpu_lm_persist.py)
OPTION_SETS = {
    "default": {},
    "lm_tiles0": {"lm_tiles": 0},
    "lm_mfma0": {"lm_mfma": 0},
    "lm_fused0": {"lm_fused": 0},
    "lm_host0": {"lm_host": 0},
    "mom_chunk1": {"mom_chunk": 1},
}
DEFAULTS = {"lm_persist": 1, "lm_tiles": 1, "lm_mfma": 1, "lm_fused": 1, "lm_host": 1, "mom_chunk": 0}

# Option sets that give the same bits -- params, last iterate, info, nfev, cost -- as observed before run_fit was split
# into its drivers, and why:
#   every input    `lm_fused` 0 and `lm_host` 0 evaluate through the same launch_moments and step through the same
#                  lm_core.h, on the host or on the device;
#   sphere         five (J | f) columns never take the matrix-core pass: `lm_tiles` and `lm_mfma` change nothing;
#   US, one block  up to 256 frames every pass and the algebraic start are one block whatever its cut, so the tiled and
#                  the record-major matrix-core pass and `mom_chunk` 1 sum in one order.
# Everything else sums in another order (k_moments' chunks against k_lm_pass', tiles against records, lanes against
# matrix cores, the algebraic start in smaller blocks) and is held to the stopping code and the oracle instead.
def same_bits_groups(family, n):
    groups = [("lm_fused0", "lm_host0")]
    if family == "sphere":
        groups.append(("default", "lm_tiles0", "lm_mfma0"))
    elif n <= 256:
        groups.append(("default", "lm_tiles0", "mom_chunk1"))
    return groups


# Every option set stops with the default set's MINPACK code on every input, but for the pairs listed here, as observed
# before run_fit was split.  The 64 frames of "fast64" run at the US calibration's tolerances of 1e-15, where WHICH
# success test fires first is decided inside the rounding of the sums: the matrix-core passes (default, `lm_tiles` 0,
# `mom_chunk` 1) stop with info 1 after 257 evaluations, the per-lane pass and k_moments (`lm_mfma` 0, `lm_fused` 0,
# `lm_host` 0) with info 2 after 235 / 231 / 231 -- at the same minimiser (REL, below).  (case, option set):
INFO_EXCEPTIONS = {("fast64", "lm_mfma0"), ("fast64", "lm_fused0"), ("fast64", "lm_host0")}

SPHERE_N = (1, 255, 256, 257, 3001, 1024 * 2048 + 1)
SPHERE_CASES = ["n%d" % n for n in SPHERE_N] + ["cap"]
US_CASES = ["single50", "pointer50", "single50_masked", "pointer50_masked", "fast64", "fast65", "fast3001",
            "fast20000_labels"]


def noisy_cap(n=3001, seed=5, half_angle=0.15):
    """a polar cap of a sphere under noise: a flat minimum, more than eight evaluations from the algebraic start"""
    g = np.random.Generator(np.random.Philox(seed))
    z = g.uniform(np.cos(half_angle), 1.0, n)
    az = g.uniform(0.0, 2.0 * np.pi, n)
    s = np.sqrt(1.0 - z * z)
    u = np.stack([s * np.cos(az), s * np.sin(az), z], axis=1)
    return np.ascontiguousarray(np.array([10.0, -20.0, 30.0]) + 200.0 * u + g.normal(0.0, 2.0, (n, 3)))


def sphere_input(name):
    return noisy_cap() if name == "cap" else synth.sphere(int(name[1:]), 0.0, seed=11)[0]


def _ones(m, name):
    return np.ones(m, np.uint8) if name.endswith("_masked") else None


def us_input(name):
    """-> (model, records, mask or None)"""
    if name.startswith("single50"):  # the 50 frames of tests/test_gpu_parity.py: test_us_least_squares
        return L.US_SINGLE, synth.us_single(50, 0.0, seed=21, pixel_sigma=1.0)[0], _ones(50, name)
    if name.startswith("pointer50"):
        return L.US_POINTER, synth.us_pointer(50, 0.0, seed=21, pixel_sigma=1.0)[0], _ones(50, name)
    if name == "fast20000_labels":
        data, _, lab = synth.us_single_fast(20_000, 0.3, seed=31)
        return L.US_SINGLE, data, lab.astype(np.uint8)
    m = int(name[4:])
    return L.US_SINGLE, synth.us_single_fast(m, 0.0, seed=100 + m)[0], np.ones(m, np.uint8)


def oracle_sphere(pts):
    """O.sphere_geometric from O.sphere_algebraic, with the row pointers built in one piece (two million rows)
    -> (params, info, nfev, cost); params empty when there is no algebraic start"""
    a = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    n = a.shape[0]
    rows = (a.ctypes.data + 24 * np.arange(n, dtype=np.uint64)).astype(np.uint64)
    ptrs = C.cast(rows.ctypes.data, C.POINTER(C.POINTER(C.c_double)))
    dp = C.POINTER(C.c_double)
    init, out = np.zeros(4), np.zeros(4)
    if O.lib().orc_sphere_algebraic(3, ptrs, n, init.ctypes.data_as(dp)) != 4:
        return np.zeros(0), 0, 0, 0.0
    info, nfev = C.c_int(0), C.c_int(0)
    got = O.lib().orc_sphere_geometric(3, ptrs, n, init.ctypes.data_as(dp), out.ctypes.data_as(dp), C.byref(info),
                                       C.byref(nfev))
    assert got == 4
    res = np.linalg.norm(a - out[:3], axis=1) - out[3]
    return out, info.value, nfev.value, float((res ** 2).sum())


def run(ctx, model, dim, delta, ls_type, data, mask, opts, persist=0):
    """one fit under one option set -> (params, last iterate, lm_info, lm_nfev, cost); the options are reset"""
    opts = dict(opts, lm_persist=persist)
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.set_model(model, dim, delta, ls_type).upload(data)
        if mask is not None:
            ctx.set_mask(mask)
        fit, info = ctx.ls_fit(mask is not None)
        return fit, ctx.last_iterate.copy(), info.lm_info, info.lm_nfev, info.cost
    finally:
        for k in opts:
            ctx.set_option(k, DEFAULTS[k])


def run_sphere(ctx, data, masked, opts, persist=0):
    return run(ctx, L.SPHERE, 3, 0.5, L.LS_GEOMETRIC, data, np.ones(len(data), np.uint8) if masked else None, opts,
               persist)


def run_us(ctx, model, data, mask, opts, persist=0):
    return run(ctx, model, 0, 3.0, L.LS_ITERATIVE, data, mask, opts, persist)


def same_bits(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]
            and (a[4] == b[4] or (np.isnan(a[4]) and np.isnan(b[4]))))


def check_between_sets(family, n, res, where):
    for group in same_bits_groups(family, n):
        for name in group[1:]:
            assert same_bits(res[group[0]], res[name]), (where, group[0], name, res[group[0]][2:], res[name][2:])
    for name, r in res.items():
        info, ref = r[2], res["default"][2]
        if (where, name) in INFO_EXCEPTIONS:  # both converged, by another of MINPACK's success tests
            assert 1 <= info <= 4 and 1 <= ref <= 4, (where, name, r[2:], res["default"][2:])
        else:
            assert info == ref, (where, name, r[2:], res["default"][2:])


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sphere_refs():
    """input and oracle fit of every sphere case, computed once"""
    out = {}
    for name in SPHERE_CASES:
        data = sphere_input(name)
        out[name] = (data,) + oracle_sphere(data)
    return out


@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
@pytest.mark.parametrize("name", SPHERE_CASES)
def test_sphere_every_driver(ctx, sphere_refs, name, masked):
    data, want, winfo, wnfev, wcost = sphere_refs[name]
    res = {k: run_sphere(ctx, data, masked, o) for k, o in OPTION_SETS.items()}
    for k, (fit, last, info, nfev, cost) in res.items():
        print(name, masked, k, info, nfev, repr(cost), fit)
        if len(want) == 0:  # one point: no algebraic start, the fit is empty (LSQR_EMPTY)
            assert len(fit) == 0, (name, k)
            continue
        assert 1 <= info <= 4 and 1 <= winfo <= 4, (name, k, info, winfo)
        assert abs(nfev - wnfev) <= 3, (name, k, nfev, wnfev)
        assert np.allclose(fit, want, rtol=1e-9, atol=1e-8), (name, k, fit, want)
        assert np.isclose(cost, wcost, rtol=1e-9), (name, k, cost, wcost)
        assert np.array_equal(fit, last), (name, k)
    if name == "cap":  # the compaction in the middle of a masked fit is only reached after eight evaluations
        assert wnfev > 8 and res["default"][3] > 8, (wnfev, res["default"][3])
    check_between_sets("sphere", len(data), res, (name, masked))


@pytest.mark.parametrize("name", US_CASES)
def test_us_every_driver(ctx, name):
    model, data, mask = us_input(name)
    res = {k: run_us(ctx, model, data, mask, o) for k, o in OPTION_SETS.items()}
    want = O.ls(O.cfg(model, 0, 3.0, 1), data) if "50" in name else None
    for k, (fit, last, info, nfev, cost) in res.items():
        print(name, k, info, nfev, repr(cost), last[:3])
        if want is not None:  # tests/test_gpu_parity.py: test_us_least_squares
            assert len(want) > 0 and len(fit) == len(want) and 1 <= info <= 4, (name, k, info)
            assert np.allclose(fit, want, rtol=REL, atol=REL * np.abs(want).max()), (name, k)
        # the same minimiser under every option set (large sets stop inside rounding noise: compare the last iterate)
        ref = res["default"][1]
        assert np.allclose(last, ref, rtol=REL, atol=REL * np.abs(ref).max()), (name, k, last, ref)
    check_between_sets("us", len(data), res, name)


# Calibrations with omega_y = +-pi/2 (tests/rotation_families.py), 200 frames under 0.5 px noise.  The analytic start has
# omega_z = 0 by the reference's gimbal formula -- at -pi/2 with an omega_x that describes another rotation -- and the
# Jacobian is rank deficient there: omega_z and omega_x turn about the same axis.
GIMBAL_CASES = ["single_plus_half_pi", "single_minus_half_pi", "pointer_plus_half_pi", "pointer_minus_half_pi"]
# Final cost against the oracle's, device / oracle - 1 over the six option sets, as first measured on an MI355X:
#   single +pi/2   +2.0e-11 .. +5.1e-11   (every driver and the oracle: info 5 after 5000 evaluations)
#   single -pi/2   -1.3e-4  .. +2.5e-4
#   pointer +pi/2  +2.0e-5  .. +3.4e-5    (info 2 after 420-439 evaluations, the oracle after 419)
#   pointer -pi/2  -6.3e-4  .. +7.3e-4    (info 2 after 27-28 evaluations, the oracle after 24)
# The library steps on (J | f)^T (J | f), the oracle on the QR factors of J: cond(J) ~ 7e7 squares to the reciprocal of
# the rounding unit, the step along the weak direction (omega_z against omega_x) is noise, and each minimiser comes to
# rest at another point of a valley that falls by parts in 1e4 -- below the oracle as often as above it.  The bound is
# ten times the worst excess.
GIMBAL_COST_MARGIN = 7.5e-3
# At -pi/2 the single-target variant (tolerances 1e-15) ends in two ways: the drivers whose passes are k_lm_pass' (the
# default, `lm_tiles` 0, `lm_mfma` 0, `mom_chunk` 1) spend the 5000 evaluations as the oracle does (info 5, no result);
# through k_moments' sums (`lm_fused` 0, `lm_host` 0) the trust region collapses below xtol after 1467 evaluations
# (info 2, a result, cost 2.5e-4 above the oracle's last iterate).  INTEGRATION.md, "Behavioural differences".
GIMBAL_CLASS_EXCEPTIONS = {("single_minus_half_pi", "lm_fused0"), ("single_minus_half_pi", "lm_host0")}


@pytest.mark.parametrize("name", GIMBAL_CASES)
def test_us_every_driver_from_a_gimbal_start(ctx, name):
    """Every driver from a start at gimbal lock: the same bits where the drivers walk through the same sums
    (same_bits_groups: the claim of the cases above, now on a rank-deficient Jacobian), every result finite, the outcome
    class of the oracle's lmder from the same start (a result, or none: info 5) under the default options and under
    every option set but GIMBAL_CLASS_EXCEPTIONS, which give a result where the oracle gives none, and a final cost
    not above the oracle's by more than GIMBAL_COST_MARGIN (relative; measurement and reasoning above)."""
    kind, wy = name.split("_", 1)
    model = L.US_SINGLE if kind == "single" else L.US_POINTER
    data = RF.us_frames(kind, RF.omegas(wy), 200, 0.5, 0, seed=1)[0]
    res = {k: run_us(ctx, model, data, None, o) for k, o in OPTION_SETS.items()}
    oc = O.cfg(model, 0, 3.0, 1)
    init = O.us_analytic(model, data)
    o = 3 if kind == "single" else 0
    assert len(init) > 0 and init[o + 3] == 0.0   # the start is on the gimbal branch
    want, winfo, wnfev = O.us_iterative(model, data, init)
    wcost = O.stats(oc, want, data)[3]
    for k, (fit, last, info, nfev, cost) in res.items():
        print(name, k, "info", info, winfo, "nfev", nfev, wnfev, "cost", repr(cost), repr(wcost), "excess", cost / wcost - 1.0)
        assert np.all(np.isfinite(last)) and np.isfinite(cost), (name, k, last, cost)
        assert (len(fit) > 0) == (1 <= info <= 4), (name, k, info, len(fit))
        if (name, k) in GIMBAL_CLASS_EXCEPTIONS:
            assert 1 <= info <= 4 and winfo == 5, (name, k, info, winfo)
        else:
            assert (1 <= info <= 4) == (1 <= winfo <= 4) and info == res["default"][2], (name, k, info, winfo)
        assert cost <= wcost * (1.0 + GIMBAL_COST_MARGIN), (name, k, cost, wcost)
    for group in same_bits_groups("us", len(data)):
        for k in group[1:]:
            assert same_bits(res[group[0]], res[k]), (name, group[0], k, res[group[0]][2:], res[k][2:])
