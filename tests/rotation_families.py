"""Rotations and calibration angles at which the rotation estimators change formula (csrc/rigid.h frame_quaternion,
csrc/us.h USModel::finish, csrc/phantom.h PhantomModel::finish): half turns, the 0.5 degree "singular range" around
them, and Euler angles with omega_y at +-pi/2 (gimbal lock).  lsqrrecipes_amd.synth draws its truths at random and
(almost) never lands there.  A plain module, imported by the CPU tests (tests/test_rotation_branches.py) and the GPU
tests (tests/test_gpu_rotation_branches.py, tests/test_gpu_lm_paths.py), so that every layer sees the same inputs.
Every generator is seeded and returns float64 arrays in the record layouts of lsqrrecipes_amd.synth."""
import numpy as np

from lsqrrecipes_amd import synth

SMALL_ANGLE = 0.008726535498373935  # 0.5 degrees: common/Frame.cxx:955, ...USCalibrationParametersEstimator.cxx
HALF_PI = np.pi / 2.0
AXIS = (0.3, -0.5, 0.8)


def _rng(*key):
    return np.random.default_rng([20261, *key])


def axis_angle(axis, theta):
    """[s, qx, qy, qz] of the rotation by theta about axis"""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([[np.cos(theta / 2.0)], np.sin(theta / 2.0) * a])


# name -> (quaternion [s, qx, qy, qz], rotation angle theta in [0, 2 pi))
ROTATIONS = {
    "identity": (np.array([1.0, 0.0, 0.0, 0.0]), 0.0),
    # exact half turns: s = 0 exactly, trace(R) + 1 = 0 up to the last bit
    "half_x": (np.array([0.0, 1.0, 0.0, 0.0]), np.pi),
    "half_y": (np.array([0.0, 0.0, 1.0, 0.0]), np.pi),
    "half_z": (np.array([0.0, 0.0, 0.0, 1.0]), np.pi),
    "half_111": (np.concatenate([[0.0], np.ones(3) / np.sqrt(3.0)]), np.pi),
    "half_axis": (np.concatenate([[0.0], np.array(AXIS) / np.linalg.norm(AXIS)]), np.pi),
    "perm_120": (np.array([0.5, 0.5, 0.5, 0.5]), 2.0 * np.pi / 3.0),  # x -> y -> z -> x: a permutation matrix
    "quarter_z": (np.array([np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)]), np.pi / 2.0),
    "tiny": (axis_angle((1.0, 2.0, 3.0), 1e-9), 1e-9),
    "negative_s": (-axis_angle((0.2, 0.9, -0.4), 1.1), 1.1),
    # inside the singular range on either side of the half turn (the far side has s < 0)
    "near_pi_below": (axis_angle(AXIS, np.pi - 5e-3), np.pi - 5e-3),
    "near_pi_above": (axis_angle(AXIS, np.pi + 5e-3), np.pi + 5e-3),
    # the half angle 1e-4 outside / inside the start of the singular range
    "threshold_outside": (axis_angle(AXIS, np.pi - 2.0 * SMALL_ANGLE - 2e-4), np.pi - 2.0 * SMALL_ANGLE - 2e-4),
    "threshold_inside": (axis_angle(AXIS, np.pi - 2.0 * SMALL_ANGLE + 2e-4), np.pi - 2.0 * SMALL_ANGLE + 2e-4),
}
HALF_TURNS = ("half_x", "half_y", "half_z", "half_111", "half_axis")
THRESHOLD_PAIRS = (("threshold_outside", "threshold_inside"),)  # (regular formula, singular-range formula)
CLOUDS = ("generic", "integer", "coplanar_z0", "coplanar_tilted", "scale_1e-3")


def in_singular_range(theta):
    """does frame_quaternion take the singular-range formula for a rotation by theta (half angle folded into
    [0, pi / 2], as acos of the non-negative s it computes)"""
    half = (theta % (2.0 * np.pi)) / 2.0
    half = min(half, np.pi - half)
    return half > HALF_PI - SMALL_ANGLE


def cloud(name, n, seed):
    """n first points (n, 3)"""
    g = _rng(1, CLOUDS.index(name), seed)
    if name == "generic":
        return g.uniform(-100.0, 100.0, (n, 3))
    if name == "integer":
        return g.integers(-50, 51, (n, 3)).astype(np.float64)
    if name == "coplanar_z0":
        p = g.uniform(-100.0, 100.0, (n, 3))
        p[:, 2] = 0.0
        return p
    if name == "coplanar_tilted":
        p = g.uniform(-100.0, 100.0, (n, 3))
        normal = np.array([0.48, -0.6, 0.64])
        return p - np.outer(p @ normal, normal) + 7.0 * normal
    if name == "scale_1e-3":
        return g.uniform(-1e-3, 1e-3, (n, 3))
    raise KeyError(name)


def cloud_extent(name):
    return {"integer": 50.0, "scale_1e-3": 1e-3}.get(name, 100.0)


def absor_pairs(rotation, cloud_name, n, sigma=0.0, n_outliers=0, seed=0):
    """second = R first + t (+ noise of sigma times extent / 100) -> (records (n, 6), [s, qx, qy, qz, t], is_inlier).
    The translation is a multiple of 1/4 (of the cloud's extent / 100), so that integer clouds under the axis-parallel
    and the permutation rotations give exact pairs.  Outliers are the last n_outliers records, shifted by up to the
    extent."""
    q = ROTATIONS[rotation][0] if isinstance(rotation, str) else np.asarray(rotation, dtype=np.float64)
    key = list(ROTATIONS).index(rotation) if isinstance(rotation, str) else 99
    g = _rng(2, key, CLOUDS.index(cloud_name), seed)
    unit = cloud_extent(cloud_name) / 100.0
    first = cloud(cloud_name, n, seed)
    t = g.integers(-400, 401, 3) / 4.0 * unit
    second = first @ synth.quat_to_matrix(q).T + t
    if sigma > 0:
        second = second + g.normal(0.0, sigma * unit, (n, 3))
    lab = np.ones(n, bool)
    if n_outliers:
        shift = g.uniform(20.0, 100.0, (n_outliers, 3)) * g.choice([-1.0, 1.0], (n_outliers, 3)) * unit
        second[n - n_outliers:] += shift
        lab[n - n_outliers:] = False
    return np.ascontiguousarray(np.hstack([first, second])), np.concatenate([q, t]), lab


# omega_y of the US calibration (omega3_y of the plane phantom): name -> angle
OMEGA_Y = {
    "plus_half_pi": HALF_PI,
    "minus_half_pi": -HALF_PI,
    "plus_1e-3": HALF_PI - 1e-3,
    "minus_1e-3": -(HALF_PI - 1e-3),
    "plus_inside": HALF_PI - SMALL_ANGLE + 1e-4,
    "minus_inside": -(HALF_PI - SMALL_ANGLE + 1e-4),
    "plus_outside": HALF_PI - SMALL_ANGLE - 1e-4,
    "minus_outside": -(HALF_PI - SMALL_ANGLE - 1e-4),
    "control": 0.3,
}
OMEGA_Z, OMEGA_X = 0.7, 1.1   # the other two angles: generic, omega_x +- omega_z no multiple of pi / 2
OMEGA1_YX = (0.4, 0.3)        # the phantom plane's two angles stay generic
MX, MY = 0.143, 0.139


def in_gimbal_range(omega_y):
    return not (abs(omega_y - HALF_PI) > SMALL_ANGLE and abs(omega_y + HALF_PI) > SMALL_ANGLE)


def omegas(name):
    return (OMEGA_Z, OMEGA_Y[name], OMEGA_X)


def _frame_rotations(g, m):
    w2 = g.uniform(0.0, np.pi, (m, 3))
    return np.stack([synth.euler_zyx(*w) for w in w2])


def us_frames(kind, omega_zyx, m, sigma=0.0, n_outliers=0, seed=0):
    """the geometry of synth.us_single / synth.us_pointer with the calibration's Euler angles prescribed
    -> (records (m, 15) single / (m, 18) pointer, truth (11 / 8: [t1,] t3, omega_z, omega_y, omega_x, m_x, m_y),
    is_inlier); sigma: pixel noise; the outliers are the last n_outliers frames"""
    single = kind == "single"
    g = _rng(3, int(single), seed)
    t3 = g.uniform(-100.0, 100.0, 3)
    t1 = g.uniform(-100.0, 100.0, 3)
    R3 = synth.euler_zyx(*omega_zyx)
    uv = np.stack([g.uniform(0.0, 640.0, m), g.uniform(0.0, 480.0, m)], axis=1)
    R2 = _frame_rotations(g, m)
    q3 = np.stack([MX * uv[:, 0], MY * uv[:, 1], np.zeros(m)], axis=1) @ R3.T + t3
    rec = np.zeros((m, 15 if single else 18))
    rec[:, 0:9] = R2.reshape(m, 9)
    lab = np.ones(m, bool)
    lab[m - n_outliers:] = n_outliers == 0
    if single:
        rec[:, 9:12] = t1 - np.einsum("mij,mj->mi", R2, q3)
        if n_outliers:
            rec[m - n_outliers:, 9:12] = g.uniform(-100.0, 100.0, (n_outliers, 3))
    else:
        t2 = g.uniform(-100.0, 100.0, (m, 3))
        rec[:, 9:12] = t2
        rec[:, 15:18] = np.einsum("mij,mj->mi", R2, q3) + t2
        if n_outliers:
            rec[m - n_outliers:, 15:18] = g.uniform(-100.0, 100.0, (n_outliers, 3))
    rec[:, 13:15] = uv + (g.normal(0.0, sigma, (m, 2)) if sigma > 0 else 0.0)
    truth = np.concatenate([t1 if single else [], t3, omega_zyx, [MX, MY]])
    return np.ascontiguousarray(rec), truth, lab


def us_solution(kind, truth):
    """the exact solution vector of the analytic system, as USModel::finish takes it:
    [m_x R3(:,1), m_y R3(:,2), t3 (, t1)]"""
    single = kind == "single"
    o = 3 if single else 0
    R3 = synth.euler_zyx(*truth[o + 3:o + 6])
    x = np.concatenate([truth[o + 6] * R3[:, 0], truth[o + 7] * R3[:, 1], truth[o:o + 3]])
    return np.concatenate([x, truth[:3]]) if single else x


def phantom_frames(omega1_yx, omega3_zyx, n, sigma=0.0, n_outliers=0, seed=0):
    """the geometry of synth.plane_phantom with the angles of T1 and T3 prescribed
    -> (records (n, 15), true 41-vector, is_inlier); the outliers are the last n_outliers frames"""
    g = _rng(4, seed)
    t3 = g.uniform(-100.0, 100.0, 3)
    t1 = g.uniform(-100.0, 100.0, 3)
    R3 = synth.euler_zyx(*omega3_zyx)
    R1 = synth.euler_zyx(g.uniform(0.0, np.pi), omega1_yx[0], omega1_yx[1])  # omega1_z is not observable
    truth = synth.phantom_params(list(omega1_yx), t1[2], t3, list(omega3_zyx), MX, MY)
    uv = np.stack([g.uniform(0.0, 640.0, n), g.uniform(0.0, 480.0, n)], axis=1)
    on_plane = np.stack([g.uniform(-100.0, 100.0, n), g.uniform(-100.0, 100.0, n), np.zeros(n)], axis=1)
    lab = np.ones(n, bool)
    if n_outliers:
        lab[n - n_outliers:] = False
        on_plane[n - n_outliers:, 2] = g.uniform(20.0, 100.0, n_outliers) * g.choice([-1.0, 1.0], n_outliers)
    R2 = _frame_rotations(g, n)
    q3 = np.stack([MX * uv[:, 0], MY * uv[:, 1], np.zeros(n)], axis=1) @ R3.T + t3
    rec = np.zeros((n, 15))
    rec[:, 0:9] = R2.reshape(n, 9)
    rec[:, 9:12] = (on_plane - t1) @ R1 - np.einsum("mij,mj->mi", R2, q3)
    rec[:, 13:15] = uv + (g.normal(0.0, sigma, (n, 2)) if sigma > 0 else 0.0)
    return np.ascontiguousarray(rec), truth, lab


def phantom_solution(truth):
    """the unit null vector of the homogeneous system, as PhantomModel::finish takes it"""
    e = np.r_[truth[11:41], truth[2]]
    return np.ascontiguousarray(e / np.linalg.norm(e))


def angle_diff(a, b):
    """|a - b| modulo 2 pi"""
    d = np.abs(np.asarray(a) - np.asarray(b)) % (2.0 * np.pi)
    return np.minimum(d, 2.0 * np.pi - d)
