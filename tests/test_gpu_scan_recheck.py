"""The exact path of the plane's packed counted scan (csrc/cells.h: cells_survivors, Exact::Band; PairsForm::PackedRecheck; option
"scan_recheck"): a (hypothesis, cell) pair one of whose observations falls into the fp32 filter's band re-evaluates the
fp64 predicate for the observations in the band alone (1, the default) instead of for the whole cell (0).  The vote of
every observation comes from the same predicate either way, so not a single vote may change: with the option 1 and 0
the votes of every hypothesis are identical to each other and to the oracle's count.

Upload: 70 001 points (137 cells of 512, the last one ragged), batches of 1024 hypotheses -- the smallest batch the
counted scan takes --, every hypothesis counted (scan_bound 0) and the bounded scan (scan_bound 1: its compacted
selections go through the same kernel).  delta 1e-4 (next to nothing agrees, the band is most of the threshold), 0.5
(the noise level: the band is crossed all the time) and 40 (everything near the structure agrees).  The bounded scan
by design does not count hypotheses that provably cannot win and reports 0 for them (tests/test_gpu_parity.py:
test_bounded_scan_keeps_winner_and_replay): there the two option values are compared with each other for every
hypothesis, and against the oracle every vote is either the oracle's count or 0, a 0 only where the oracle's count
does not exceed the running maximum of the hypotheses before it."""
import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L, synth
from lsqrrecipes_amd.context import Context
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu
H = 1024
SEED = 8
DEFAULTS = {"scan_recheck": 1, "scan_index": 1, "scan_bound": 1}  # the library's


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


def _batch(ctx, bound, recheck):
    ctx.set_option("scan_bound", bound)
    ctx.set_option("scan_recheck", recheck)
    r = ctx.batch_fit(SEED, 0, H)
    par, valid, votes = ctx.hypotheses()
    return (int(r["info"].best_index), int(r["info"].best_votes), par.copy(), valid.copy(), votes.copy(),
            ctx.scan_work())


@pytest.mark.parametrize("delta", [1e-4, 0.5, 40.0])
def test_votes_do_not_depend_on_the_recheck(ctx, cloud, delta):
    ctx.set_model(L.PLANE, 3, delta).upload(cloud)
    ctx.set_option("scan_index", 2)
    res = {(b, r): _batch(ctx, b, r) for b in (0, 1) for r in (0, 1)}
    assert ctx.index_info()["built"] and ctx.index_info()["cells"] == 137
    par, valid = res[(0, 1)][2], res[(0, 1)][3]
    want = O.scan_many(O.cfg(O.PLANE, 3, delta), par, valid, cloud)
    for b in (0, 1):
        on, off = res[(b, 1)], res[(b, 0)]
        print("delta %g scan_bound %d: ambiguous pairs %d (whole cell) %d (per value), band records %d"
              % (delta, b, off[5]["ambiguous_pairs"], on[5]["ambiguous_pairs"], on[5]["band_records"]))
        assert on[:2] == off[:2]
        assert np.array_equal(on[2], par, equal_nan=True) and np.array_equal(on[3], valid)
        assert np.array_equal(on[4], off[4]), (b, np.flatnonzero(on[4] != off[4])[:8])
        # the same pairs are ambiguous whichever way they are re-checked
        assert on[5]["ambiguous_pairs"] == off[5]["ambiguous_pairs"]
        assert on[5]["band_records"] >= on[5]["ambiguous_pairs"] and off[5]["band_records"] == 0
        assert (on[0], on[1]) == (int(np.argmax(want)), int(want.max()))         # first maximum, exact votes
    for r in (0, 1):
        full = np.where(valid > 0, res[(0, r)][4], 0)
        assert np.array_equal(full, want), (r, np.flatnonzero(full != want)[:8])
        # the bounded scan: a hypothesis is counted to the end -- the oracle's count, exactly -- or skipped: it reports
        # 0, and its true count could not have become the running maximum at its index (first maximum: ties lose)
        bounded = np.where(valid > 0, res[(1, r)][4], 0)
        skipped = bounded != want
        assert np.all(bounded[skipped] == 0), (r, np.flatnonzero(skipped & (bounded != 0))[:8])
        runmax = np.maximum.accumulate(want)
        at = np.flatnonzero(skipped)
        assert not skipped[0] and np.all(want[at] <= runmax[at - 1]), (r, at[:8])
        assert np.count_nonzero(~skipped & (want > 0)) > 0                              # the winner at the least


def test_the_exact_path_is_taken(ctx, cloud):
    """delta = 0.5 is the inlier noise's scale: of 140 000 (hypothesis, cell) pairs some hold an observation with
    ||s| - delta| below the band's half-width (~2e-5 on these cells); the counters say so, for the full count and for
    the bounded scan's selections"""
    ctx.set_model(L.PLANE, 3, 0.5).upload(cloud)
    ctx.set_option("scan_index", 2)
    for bound in (0, 1):
        w = _batch(ctx, bound, 1)[5]
        assert w["ambiguous_pairs"] > 0 and w["band_records"] >= w["ambiguous_pairs"], (bound, w)
        # a handful of observations per ambiguous pair, not the cell's 512
        assert w["band_records"] < 8 * w["ambiguous_pairs"], (bound, w)
    # a scan that does not go through the counted kernel reports none
    ctx.set_option("scan_index", 0)
    ctx.hypotheses_sample(SEED, 0, 64)
    ctx.scan()
    w = ctx.scan_work()
    assert w["ambiguous_pairs"] == 0 and w["band_records"] == 0


@pytest.mark.parametrize("case", ["offset_1e6", "tiny_delta"])
def test_nothing_certain_in_any_cell(ctx, cloud, case):
    """hypotheses whose filter has no certain inliers in any cell (t_in <= 0: a = 0, every d is non-negative): every
    observation that can agree at all is in the band and goes the exact way, in all eight value slots of a lane.  A
    translation by 1e6 (the band's absolute term 3e-12 X exceeds delta = 1e-6) and delta = 1e-9; the batch holds the
    degenerate rows of the other stress tests (one point three times: NaN parameters, not valid; their votes are
    masked out, they only have to pass through the kernel).  NOT reached here, nor by any hypothesis estimate() makes:
    the filter switched off altogether (band = 0xFFFFFFFF), which the plane has for |n_i| > 1 only -- there NaN and
    sign-bit patterns count as in the band too and all eight slots run in every lane; that case rests on the reasoning
    in cells.h (cells_survivors), not on a test."""
    data, delta = (cloud + np.array([1.0e6, -2.0e6, 3.0e6]), 1e-6) if case == "offset_1e6" else (cloud, 1e-9)
    data = np.ascontiguousarray(data)
    ctx.set_model(L.PLANE, 3, delta).upload(data)
    ctx.set_option("scan_index", 2)
    subsets = O.ctr_subsets(SEED, 0, H, len(data), 3).astype(np.uint32)
    for base in (0, 512, H - 7):
        subsets[base + 1] = subsets[base + 1][0]
        subsets[base + 5, :2] = subsets[base + 5, 0]
    votes = {}
    for recheck in (1, 0):
        ctx.set_option("scan_recheck", recheck)
        ctx.hypotheses_from_subsets(subsets)
        ctx.scan()
        par, valid, v = ctx.hypotheses()
        votes[recheck] = np.where(valid > 0, v, 0)
        work = ctx.scan_work()
        assert ctx.index_info()["built"] and work["ambiguous_pairs"] > 0
    assert not valid[1] and not valid[H - 6]
    want = O.scan_many(O.cfg(O.PLANE, 3, delta), par, valid, data)
    assert want.max() >= 3                                  # a hypothesis' own three points at the least
    assert np.array_equal(votes[1], want), np.flatnonzero(votes[1] != want)[:8]
    assert np.array_equal(votes[0], want), np.flatnonzero(votes[0] != want)[:8]


def test_option_values(ctx):
    ctx.set_option("scan_recheck", 0)
    ctx.set_option("scan_recheck", 1)
    with pytest.raises(L.LsqrError) as e:
        ctx.set_option("scan_recheck", 2)
    assert e.value.status == L.ERR_INVALID
