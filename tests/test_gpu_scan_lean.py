"""The lean forms of the counted two-level scan (csrc/cells.h; option "scan_lean", default 1): the count-only counting
pass (k_cells_bounds, BoundsForm::Count: survivor counts from level 1's own compare mask, nothing else computed or written)
and, for the plane, k_scan_pairs, PairsForm::Lean: share arithmetic on the scalar unit, one Hyp that is refilled for the next
group as soon as level 1 has read it, and the pair loop's two addends stored twice in the LDS broadcast area.  Not a
single vote may change: with the option 1 and 0 the votes of every hypothesis are identical to each other and to the
exhaustive fp64 kernel (scan_index 0), winner, fit and consensus set are equal, a 64-hypothesis sample equals the
oracle's count, and the counted work (lsqr_scan_workload) does not depend on the option.

Shapes: 200 k points plus eight far corner points = 391 cells = 3 x 128 + 7: the 7-cell tail of the last chunk runs
the four-at-a-time loop of the counting pass and its single-cell tail, and several workgroups share the scan.  H = 1024
(the FULL_COUNT_PAIRS threshold), 1100 (last group of 64 partial, an odd number of groups) and 4200 (second launch;
h_off > 0 in the bounded selection), in 3-D and 2-D, with the injected NaN / far / degenerate rows of
test_gpu_prepared_rows.  One sphere case: the count-only counting pass serves the sphere's and the line's counted
scans as well."""
import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L, synth
from lsqrrecipes_amd.context import Context
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu
N = 200_000
SEED = 0xBEEF


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.set_option("scan_lean", 1)
    c.close()


def _with_far(data, dim):
    g = np.random.default_rng(dim)
    far = np.where(g.random((8, dim)) < 0.5, -1.0, 1.0) * 4000.0 + g.normal(0, 0.3, (8, dim))
    return np.ascontiguousarray(np.vstack([data, far]))


@pytest.fixture(scope="module")
def clouds():
    """dim -> the points, with eight far corner points appended (they set absmax) for the injected rows"""
    return {dim: _with_far(synth.plane(N, 0.5, dim=dim)[0], dim) for dim in (3, 2)}


def _subsets(n, k, H):
    """the sampler's subsets with rows replaced by: degenerate subsets (estimate() refuses them: NaN parameters, not
    valid), subsets of the far corner points (|n.a| near absmax) and mixed near / far subsets -- spread over the first,
    a middle and the last group of 64"""
    s = O.ctr_subsets(SEED, 0, H, n, k).astype(np.uint32)
    far = np.arange(n - 8, n, dtype=np.uint32)
    for base in (0, (H // 2) & ~63, H - 7):
        s[base + 1] = s[base + 1][0]                  # one point, dim times
        s[base + 2] = far[:k]
        s[base + 3] = far[8 - k:]
        s[base + 4, 0] = far[3]                       # one far point, the rest from the cloud
        s[base + 5, :2] = s[base + 5, 0]              # two equal points
    return s


def _scan(ctx, subsets, index, lean, workload=False):
    ctx.set_option("scan_index", index)
    ctx.set_option("scan_lean", lean)
    ctx.hypotheses_from_subsets(subsets)
    ctx.scan()
    par, valid, votes = ctx.hypotheses()
    valid, votes = valid.copy(), votes.copy()
    built = ctx.index_info()["built"]
    wl = ctx.scan_workload() if workload else None
    ctx.set_option("scan_index", 1)
    ctx.set_option("scan_lean", 1)
    return par, valid, votes, built, wl


@pytest.mark.parametrize("H", [1024, 1100, 4200])
@pytest.mark.parametrize("dim", [3, 2])
def test_full_count_votes_do_not_depend_on_the_lean_forms(ctx, clouds, dim, H):
    data = clouds[dim]
    ctx.set_model(L.PLANE, dim, 0.5).upload(data)
    subsets = _subsets(len(data), ctx.K, H)
    par, valid, exact, built, _ = _scan(ctx, subsets, 0, 1)
    assert not built
    _, v1, on, built, w1 = _scan(ctx, subsets, 2, 1, workload=True)
    assert built
    if dim == 3:
        assert ctx.index_info()["cells"] == 391            # 3 x 128 + 7: both loops of the counting pass run
    _, v0, off, built, w0 = _scan(ctx, subsets, 2, 0, workload=True)
    assert built
    assert np.array_equal(v1, valid) and np.array_equal(v0, valid)
    assert not valid[1] and not valid[H - 6] and np.isnan(par[1]).all()       # the injected NaN rows are there
    assert valid[2] and valid[H - 5] and np.abs(par[2][dim:]).max() > 3900.0  # ... and the far ones
    assert np.array_equal(on, off), np.flatnonzero(on != off)[:8]
    assert np.array_equal(on, exact), np.flatnonzero(on != exact)[:8]
    # (the batch holds near-model hypotheses, whose cells take the exact path: half the points are inliers with
    # sigma 0.4, 79 % of them within 0.5 of the true plane; a three-point model keeps well over half of those)
    assert exact.max() > 0.2 * N
    assert w1["pairs_counted"] == w0["pairs_counted"] and w1["pairs"] == w0["pairs"] and w1["pairs"] > 0
    # the oracle on a sample: the injected rows of the first group, the winner, and every (H // 55)-th hypothesis
    pick = np.unique(np.concatenate([np.arange(8), [int(np.argmax(exact))], np.arange(8, H, H // 55)]))[:64]
    want = O.scan_many(O.cfg(O.PLANE, dim, 0.5), par[pick], valid[pick], data)
    assert np.array_equal(np.where(valid[pick] > 0, on[pick], 0), want)


def _batches(ctx, H, bound, lean, firsts):
    ctx.set_option("scan_bound", bound)
    ctx.set_option("scan_lean", lean)
    out = []
    for first in firsts:
        r = ctx.batch_fit(SEED, first, H, want_consensus=True)
        _, valid, votes = ctx.hypotheses(params=False)
        out.append((int(r["info"].best_index), int(r["info"].best_votes), r["params"].copy(), r["consensus"].copy(),
                    valid.copy(), votes.copy()))
    ctx.set_option("scan_lean", 1)
    return out


@pytest.mark.parametrize("H", [1024, 1100, 4200])
@pytest.mark.parametrize("dim", [3, 2])
def test_batches_counted_and_bounded_with_and_without_the_lean_forms(ctx, clouds, dim, H):
    """lsqr_batch_fit, two consecutive batches on one context, every hypothesis counted (scan_bound 0) and the bounded
    scan (its compacted selection is counted through the same two kernels, from h_off > 0 at H = 4200): winner, votes,
    consensus set and fit do not depend on scan_lean; the counted votes equal the exhaustive kernel's"""
    data = clouds[dim]
    ctx.set_model(L.PLANE, dim, 0.5).upload(data)
    firsts = (0, H)
    ctx.set_option("scan_index", 0)
    exact = _batches(ctx, H, 0, 1, firsts)
    assert not ctx.index_info()["built"]
    ctx.set_option("scan_index", 2)
    res = {(b, p): _batches(ctx, H, b, p, firsts) for b in (0, 1) for p in (1, 0)}
    assert ctx.index_info()["built"]
    ctx.set_option("scan_index", 1)
    ctx.set_option("scan_bound", 1)
    for k in range(len(firsts)):
        for b in (0, 1):
            on, off = res[(b, 1)][k], res[(b, 0)][k]
            assert on[:2] == off[:2] and all(np.array_equal(x, y) for x, y in zip(on[2:], off[2:])), (b, k)
            # winner, votes of the winner, fit and consensus set are the exhaustive kernel's
            assert on[:2] == exact[k][:2] and np.array_equal(on[2], exact[k][2]) and np.array_equal(on[3], exact[k][3])
        assert np.array_equal(res[(0, 1)][k][5], exact[k][5])       # every vote of the full count
        bounded, full = res[(1, 1)][k][5], exact[k][5]              # bounded: exact or provably not the winner
        assert np.all((bounded == full) | (bounded < full.max()))


def test_sphere_full_count_votes_do_not_depend_on_the_lean_forms(ctx):
    H = 1100
    data = synth.sphere(N, 0.5)[0]
    ctx.set_model(L.SPHERE, 3, 0.5).upload(data)
    subsets = O.ctr_subsets(SEED, 0, H, len(data), ctx.K).astype(np.uint32)
    _, valid, exact, built, _ = _scan(ctx, subsets, 0, 1)
    assert not built
    _, v1, on, built, _ = _scan(ctx, subsets, 2, 1)
    assert built
    _, v0, off, built, _ = _scan(ctx, subsets, 2, 0)
    assert built
    assert np.array_equal(v1, valid) and np.array_equal(v0, valid)
    assert np.array_equal(on, off), np.flatnonzero(on != off)[:8]
    assert np.array_equal(on, exact), np.flatnonzero(on != exact)[:8]
    assert exact.max() > 0
