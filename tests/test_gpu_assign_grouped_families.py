"""The five grouped assign / refine calls in turn on ONE context.

The families of the grouped round loop (csrc/assign_grouped.h: AssignGrpClosed, AssignGrpLm, AssignGrpDense) share one
core on the context -- the pinned block, d_rows, the counter words, the presence words -- and lay it out differently:
other row widths, other counter blocks, one or two going words, other bytes of their own.  So the sequence below runs
them one after the other on a single Context, model set and upload included, growing the buffers on the way, and every
result must equal, byte for byte, the result of the same call on a fresh Context: labels, params, counts, offsets,
rounds, converged, status, n_used and the raw lsqr_fit_info records (for the assignment: labels, residuals, counts,
offsets).

Small scenes: six groups of 0 to 400 records interleaved in one upload, one of them empty, one with records and no
models, a few records in no group.  The scene builders of the three grouped test files have their sizes (up to 13 000
records a group) built in, so the scenes here are made from what those builders are made from -- synth.plane /
synth.sphere with their recipe of three planted models and clutter per group, and test_gpu_assign_dense.mixture, the
generator test_gpu_assign_dense_grouped.scene calls -- at this test's sizes."""
import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd import synth
from lsqrrecipes_amd.context import Context
from test_gpu_assign_dense import DELTA, SIGMA, mixture

pytestmark = pytest.mark.gpu

NG, ROUNDS = 6, 3
SIZES = [0, 40, 400, 123, 300, 7]      # group 0 is empty
SIZES_SMALL = [0, 20, 150, 60, 100, 7]  # the first call's: the later ones grow every buffer
NM = np.array([3, 3, 3, 0, 2, 3], dtype=np.uintp)    # group 3 has records and no models
NM64 = np.array([3, 3, 64, 0, 2, 3], dtype=np.uintp)
N_OUT = 10  # records labelled -1, and as many labelled NG + 1


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _interleave(parts, width, seed):
    labels = [np.full(len(p), g, dtype=np.int32) for g, p in enumerate(parts)]
    labels[-1] = np.array([-1] * N_OUT + [NG + 1] * N_OUT, dtype=np.int32)  # (the last part: in no group)
    data, groups = np.vstack(parts), np.concatenate(labels)
    assert data.shape == (sum(len(p) for p in parts), width)
    order = np.random.default_rng(seed).permutation(len(data))
    return np.ascontiguousarray(data[order]), np.ascontiguousarray(groups[order])


def point_scene(gen, dim, is_sphere, seed):
    """-> data, groups, start rows (NG, 3, P): per group three planted models of 3/10 of its records each, the rest
    clutter; the start rows are the planted truth moved a little, further in some groups than in others"""
    rng = np.random.default_rng(seed)
    kw = {} if dim == 3 else {"dim": dim}
    parts, params = [], None
    for g, n in enumerate(SIZES):
        m = max((3 * n) // 10, 1 if n else 0)
        planted = [gen(max(m, 2), 0.0, seed=seed * 4096 + 16 * g + j, sigma=0.1, **kw) for j in range(3)]
        if params is None:
            params = np.zeros((NG, 3, len(planted[0][1])))
        clutter = gen(max(n - 3 * m, 1), 1.0, seed=seed * 4096 + 999 + g, **kw)[0][:n - 3 * m]
        parts.append(np.vstack([p[0][:m] for p in planted] + [clutter])[:n])
        scale = 1.0 + g % 3
        for j, p in enumerate(planted):
            row = np.array(p[1], dtype=np.float64)
            if is_sphere:
                row[:dim] += 0.08 * scale * rng.standard_normal(dim)
                row[dim] += 0.05 * scale * rng.standard_normal()
            else:
                v = row[:dim] + 2e-4 * scale * rng.standard_normal(dim)
                row[:dim] = v / np.linalg.norm(v)
                row[dim:] += 0.08 * scale * rng.standard_normal(dim)
            params[g, j] = row
    parts.append(gen(2 * N_OUT, 1.0, seed=seed * 4096 + 2000, **kw)[0])
    return _interleave(parts, dim, seed) + (params,)


def dense_scene(n, sizes, nm, max_models, seed):
    """-> rows (a | b), groups, start rows (NG, max_models, n): group g's rows lie on max(nm[g], 1) regressions"""
    rng = np.random.default_rng([seed, n])
    parts, params = [], np.zeros((NG, max_models, n))
    for g, size in enumerate(sizes):
        rows, X, _ = mixture(n, size, max(int(nm[g]), 1), seed * 100 + g)
        parts.append(rows)
        params[g, :len(X)] = X + (1 + g % 2) * SIGMA / np.sqrt(n) * rng.normal(size=X.shape)
    parts.append(mixture(n, 2 * N_OUT, 1, seed * 100 + 99)[0])
    return _interleave(parts, n + 1, seed) + (params,)


def steps():
    """the sequence: (model, scene, call, n_models)"""
    plane = point_scene(synth.plane, 3, False, 1)
    sphere = point_scene(synth.sphere, 3, True, 2)
    line2d = point_scene(synth.plane, 2, False, 3)
    return [
        ((L.DENSE, 9, DELTA), dense_scene(9, SIZES_SMALL, NM, 3, 4), "refine_dense_grouped", NM),
        ((L.PLANE, 3, 0.5), plane, "refine_grouped", NM),
        ((L.SPHERE, 3, 0.5, L.LS_GEOMETRIC), sphere, "refine_lm_grouped", NM),
        ((L.DENSE, 64, DELTA), dense_scene(64, SIZES, NM64, 64, 5), "refine_dense_grouped", NM64),
        ((L.LINE2D, 2, 0.5), line2d, "assign_grouped", NM),
        ((L.PLANE, 3, 0.5), plane, "refine_grouped", NM),
    ]


def run(c, step):
    """set the model, upload, call -> the call's outputs, every one a numpy array"""
    model, (data, groups, params), call, nm = step
    c.set_model(*model).upload(data)
    if call == "assign_grouped":
        return c.assign_grouped(groups, NG, params, nm, want_residuals=True)
    out, fits = c._refine_grouped(getattr(c._lib, "lsqr_" + call), groups, NG, params, nm, ROUNDS, None)
    out["fits"] = fits.copy()
    return out


def test_the_families_in_turn_on_one_context_equal_fresh_contexts():
    seq = steps()
    with Context(0) as one:
        got = [run(one, s) for s in seq]
    for k, (step, g) in enumerate(zip(seq, got)):
        with Context(0) as fresh:
            want = run(fresh, step)
        what = "step %d (%s, model %d)" % (k + 1, step[2], step[0][0])
        # the reference did something: records were assigned, and a refit ran in a group or more
        assert (want["labels"] >= 0).any(), what
        assert np.all(want["labels"][np.isin(step[1][1], (-1, 3, NG + 1))] == -1), what
        if "rounds" in want:
            assert want["rounds"].max() > 0 and (want["status"] == L.OK).any(), what
        assert sorted(g) == sorted(want), what
        for key in sorted(want):
            assert g[key].dtype == want[key].dtype and g[key].shape == want[key].shape, (what, key)
            assert np.array_equal(bits(g[key]), bits(want[key])), (what, key)
