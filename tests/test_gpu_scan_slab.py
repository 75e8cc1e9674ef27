"""The slab test of the 3-D plane's counting pass (csrc/cells.h: PlaneCell::slab, k_cells_bounds' mask form; csrc/axis.h:
k_cell_slabs; option "scan_slab"): a (hypothesis, cell) pair the box test keeps is dropped when the cell's oriented slab
proves that no observation of the cell can agree.  A dropped pair held no vote, so not a single vote may change: with
the option 1 and 0 the votes of every hypothesis are identical to each other and to the oracle's count, while the pairs
handed to the second level (lsqr_scan_pairs_counted) shrink.

Upload: 70 001 points (137 cells of 512, the last one ragged; the structure's cells are plates ~270 wide and 2.4 thick),
batches of 1024 hypotheses -- the smallest batch the counted scan takes --, every hypothesis counted (scan_bound 0) and
the bounded scan (scan_bound 1: its second pass goes through the same masks).  The bounded scan by design reports 0
for hypotheses that provably cannot win (tests/test_gpu_scan_recheck.py): there the two option values are compared
with each other for every hypothesis, and against the oracle every vote is the oracle's count or an admissible 0."""
import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L, synth
from lsqrrecipes_amd.context import Context
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu
H = 1024
SEED = 8
DEFAULTS = {"scan_slab": 1, "scan_index": 1, "scan_bound": 1, "scan_cell": 0, "scan_pack": 1, "scan_pairs": 0}  # the library's


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _restore(ctx):
    yield
    for name, value in DEFAULTS.items():
        ctx.set_option(name, value)


@pytest.fixture(scope="module")
def cloud():
    return synth.plane(70_001, 0.5, seed=8)[0]


def _batch(ctx, bound, slab):
    ctx.set_option("scan_bound", bound)
    ctx.set_option("scan_slab", slab)
    r = ctx.batch_fit(SEED, 0, H)
    par, valid, votes = ctx.hypotheses()
    return (int(r["info"].best_index), int(r["info"].best_votes), par.copy(), valid.copy(), votes.copy(),
            ctx.scan_pairs_counted())


@pytest.mark.parametrize("delta", [1e-4, 0.5, 40.0])
def test_votes_do_not_depend_on_the_slab_test(ctx, cloud, delta):
    ctx.set_model(L.PLANE, 3, delta).upload(cloud)
    ctx.set_option("scan_index", 2)
    res = {(b, s): _batch(ctx, b, s) for b in (0, 1) for s in (0, 1)}
    assert ctx.index_info()["built"] and ctx.index_info()["cells"] == 137
    par, valid = res[(0, 1)][2], res[(0, 1)][3]
    want = O.scan_many(O.cfg(O.PLANE, 3, delta), par, valid, cloud)
    for b in (0, 1):
        on, off = res[(b, 1)], res[(b, 0)]
        print("delta %g scan_bound %d: pairs handed to level 2: %d (box test) %d (box + slab)"
              % (delta, b, off[5]["pairs"], on[5]["pairs"]))
        assert on[5]["masks"] and off[5]["masks"] and on[5]["slab"] and not off[5]["slab"]
        assert on[5]["pairs"] <= off[5]["pairs"]
        assert on[:2] == off[:2]
        assert np.array_equal(on[2], par, equal_nan=True) and np.array_equal(on[3], valid)
        assert np.array_equal(on[4], off[4]), (b, np.flatnonzero(on[4] != off[4])[:8])
        assert (on[0], on[1]) == (int(np.argmax(want)), int(want.max()))         # first maximum, exact votes
    for s in (0, 1):
        full = np.where(valid > 0, res[(0, s)][4], 0)
        assert np.array_equal(full, want), (s, np.flatnonzero(full != want)[:8])
        # the bounded scan: a hypothesis is counted to the end -- the oracle's count, exactly -- or skipped: it reports
        # 0, and its true count could not have become the running maximum at its index (first maximum: ties lose)
        bounded = np.where(valid > 0, res[(1, s)][4], 0)
        skipped = bounded != want
        assert np.all(bounded[skipped] == 0), (s, np.flatnonzero(skipped & (bounded != 0))[:8])
        runmax = np.maximum.accumulate(want)
        at = np.flatnonzero(skipped)
        assert not skipped[0] and np.all(want[at] <= runmax[at - 1]), (s, at[:8])
        assert np.count_nonzero(~skipped & (want > 0)) > 0                              # the winner at the least


def test_the_slab_drops_pairs(ctx, cloud):
    """delta = 0.5: the structure's plates are two orders of magnitude thinner than their boxes, so pairs go.  Without
    the test the table holds exactly the box test's pairs, which lsqr_scan_workload counts with another kernel."""
    ctx.set_model(L.PLANE, 3, 0.5).upload(cloud)
    ctx.set_option("scan_index", 2)
    off = _batch(ctx, 0, 0)[5]
    box_pairs = ctx.scan_workload()["pairs"]
    on = _batch(ctx, 0, 1)[5]
    print("pairs of 1024 hypotheses x 137 cells: box test %d, box + slab %d (%.1f %% dropped)"
          % (off["pairs"], on["pairs"], 100.0 * (off["pairs"] - on["pairs"]) / off["pairs"]))
    assert off["pairs"] == box_pairs > 0
    assert 0 < on["pairs"] < off["pairs"]
    assert ctx.scan_workload()["pairs"] == box_pairs          # ... which does not depend on the option


def _degenerate(subsets):
    """one point three times and two equal points (NaN parameters, not valid) in the first, a middle and the last group"""
    for base in (0, 512, H - 7):
        subsets[base + 1] = subsets[base + 1][0]
        subsets[base + 5, :2] = subsets[base + 5, 0]
    return subsets


def _axis_aligned(n, seed):
    """half the points on z = 123.25 with sigma 0.4, half uniform and at least 20 away: every structure cell's axis is
    (0, 0, 1) up to noise and its slab is its box"""
    g = np.random.default_rng(seed)
    inl = g.uniform(-1000.0, 1000.0, (n // 2, 3))
    inl[:, 2] = 123.25 + g.normal(0.0, 0.4, n // 2)
    out = g.uniform(-1000.0, 1000.0, (2 * n, 3))
    out = out[np.abs(out[:, 2] - 123.25) >= 20.0][:n - n // 2]
    pts = np.vstack([inl, out])
    return np.ascontiguousarray(pts[g.permutation(len(pts))])


def _stress(case, cloud):
    if case == "offset_1e6":
        return np.ascontiguousarray(cloud + np.array([1.0e6, -2.0e6, 3.0e6])), 1e-6, 0
    if case == "tiny_delta":
        return cloud, 1e-9, 0
    if case == "axis_aligned":
        return _axis_aligned(70_001, 11), 0.5, 0
    if case == "no_structure":
        return synth.plane(70_001, 1.0, seed=9)[0], 0.5, 0
    if case == "cells_of_256":
        return cloud, 0.5, 256
    assert case == "last_cell_of_17"
    return np.ascontiguousarray(cloud[:4 * 512 + 17]), 0.5, 0


@pytest.mark.parametrize("case", ["offset_1e6", "tiny_delta", "axis_aligned", "no_structure", "cells_of_256",
                                  "last_cell_of_17"])
def test_stress_votes_equal_the_oracle(ctx, cloud, case):
    """every batch carries degenerate rows in three groups; votes equal the oracle's with the option 1 and 0"""
    data, delta, cell = _stress(case, cloud)
    ctx.set_option("scan_cell", cell)
    ctx.set_model(L.PLANE, 3, delta).upload(data)
    ctx.set_option("scan_index", 2)
    subsets = _degenerate(O.ctr_subsets(SEED, 0, H, len(data), 3).astype(np.uint32))
    votes, pairs = {}, {}
    for slab in (1, 0):
        ctx.set_option("scan_slab", slab)
        ctx.hypotheses_from_subsets(subsets)
        ctx.scan()
        par, valid, v = ctx.hypotheses()
        votes[slab] = np.where(valid > 0, v, 0)
        w = ctx.scan_pairs_counted()
        pairs[slab] = w["pairs"]
        assert ctx.index_info()["built"] and w["masks"] and w["slab"] == bool(slab)
    info = ctx.index_info()
    if case == "cells_of_256":
        assert info["cell_points"] == 256 and info["cells"] == 274
    if case == "last_cell_of_17":
        assert info["cells"] == 5 and info["observations"] - 4 * info["cell_points"] == 17
    print("%s: pairs %d (box test) %d (box + slab)" % (case, pairs[0], pairs[1]))
    assert not valid[1] and not valid[H - 6]
    want = O.scan_many(O.cfg(O.PLANE, 3, delta), par, valid, data)
    assert want.max() >= 3                                  # a hypothesis' own three points at the least
    assert np.array_equal(votes[1], want), np.flatnonzero(votes[1] != want)[:8]
    assert np.array_equal(votes[0], want), np.flatnonzero(votes[0] != want)[:8]
    assert pairs[1] <= pairs[0]
    assert ctx.scan_workload()["pairs"] == pairs[0]


@pytest.mark.parametrize("case", ["plane2", "sphere3", "plane3_scan_pack_0"])
def test_the_option_is_inert_elsewhere(ctx, case):
    """the 2-D plane (masks without an axis-sorted index), the sphere (count bytes) and the 3-D plane per group (scan_pack
    0: count bytes): votes and counted pairs do not depend on the option, and the test is reported as not run"""
    model, dim, gen = {"plane2": (L.PLANE, 2, synth.plane), "sphere3": (L.SPHERE, 3, synth.sphere),
                       "plane3_scan_pack_0": (L.PLANE, 3, synth.plane)}[case]
    data = gen(70_001, 0.5, seed=8, dim=dim)[0]
    ctx.set_model(model, dim, 0.5, L.LS_ALGEBRAIC if model == L.SPHERE else L.LS_GEOMETRIC).upload(data)
    ctx.set_option("scan_index", 2)
    ctx.set_option("scan_pairs", 1)                         # the counted scan whatever the model's own choice is
    ctx.set_option("scan_pack", 0 if case == "plane3_scan_pack_0" else 1)
    ctx.hypotheses_sample(SEED, 0, H)
    got = {}
    for slab in (0, 1):
        ctx.set_option("scan_slab", slab)
        ctx.scan()
        _, valid, v = ctx.hypotheses()
        got[slab] = (v.copy(), valid.copy(), ctx.scan_pairs_counted())
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    assert got[0][0].max() > 0
    assert got[0][2] == got[1][2] and not got[1][2]["slab"] and got[1][2]["pairs"] > 0
    assert got[1][2]["masks"] == (case == "plane2")
    assert got[1][2]["pairs"] == ctx.scan_workload()["pairs"]


def test_option_values(ctx):
    ctx.set_option("scan_slab", 0)
    ctx.set_option("scan_slab", 1)
    with pytest.raises(L.LsqrError) as e:
        ctx.set_option("scan_slab", 2)
    assert e.value.status == L.ERR_INVALID
    for bad in (0, 9):
        with pytest.raises(L.LsqrError) as e:
            ctx.set_option("scan_slab_gate", bad)
        assert e.value.status == L.ERR_INVALID
    ctx.set_option("scan_slab_gate", 3)
