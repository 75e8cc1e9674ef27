"""The fp32 tiles of the spatial index (csrc/cells.h: k_build_tiles, cells_load_tile; option "scan_tiles"): what a wave
of the two-level scans computes when it opens a cell -- the cell's observations relative to its centre as packed fp32
pairs, NaN rows past the end, the sphere's |x'|^2 -- is computed once behind the index build and read back.  The tile
holds bit for bit what cells_load gives, so not a single vote may change: with the option 0 and 1 the votes of every
hypothesis are identical to each other and to the oracle's count.

Uploads of 3 * 512 + 17 = 1553 points (cells of 512: a last cell of 17; cells of 256: six whole ones and the 17), plane
in 3-D and 2-D, sphere and line; 1024 hypotheses (the smallest batch the counted scan k_scan_pairs takes) and 64
(k_scan_cells); delta 1e-4, 0.5 and 40; every hypothesis counted (lsqr_scan, and lsqr_batch_fit with scan_bound 0) and
the bounded scan (scan_bound 1), which by design reports 0 for hypotheses that provably cannot win."""
import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L, synth
from lsqrrecipes_amd.context import Context
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu
N = 3 * 512 + 17
SEED = 21
DEFAULTS = {"scan_tiles": 1, "scan_index": 1, "scan_bound": 1, "scan_cell": 0}  # the library's
MODELS = {
    "plane3": (L.PLANE, O.PLANE, 3, synth.plane),
    "plane2": (L.PLANE, O.PLANE, 2, synth.plane),
    "sphere": (L.SPHERE, O.SPHERE, 3, synth.sphere),
    "line": (L.LINE, O.LINE, 3, synth.line),
}
TILE_BYTES = {"plane3": 12, "plane2": 8, "sphere": 16, "line": 12}  # per record


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


_CLOUDS = {}


def _cloud(tag):
    if tag not in _CLOUDS:
        _, _, dim, make = MODELS[tag]
        _CLOUDS[tag] = np.ascontiguousarray(make(N, 0.5, seed=31, dim=dim)[0])
    return _CLOUDS[tag]


def _prepare(ctx, tag, data, delta, cell):
    lm, _, dim, _ = MODELS[tag]
    ctx.set_option("scan_tiles", 1)
    ctx.set_option("scan_cell", cell)
    ctx.set_option("scan_index", 2)
    ctx.set_model(lm, dim, delta).upload(data)


def _scan(ctx, H, tiles):
    ctx.set_option("scan_tiles", tiles)
    ctx.hypotheses_sample(SEED, 0, H)
    ctx.scan()
    par, valid, votes = ctx.hypotheses()
    return par.copy(), valid.copy(), votes.copy()


def _check_tiles(ctx, tag, cell, n=N):
    """the builder: every cell opened from its tile and from the sorted copy, compared bit for bit on the device"""
    info, t = ctx.index_info(), ctx.scan_tiles_check()
    assert info["built"] and info["cell_points"] == cell and info["cells"] == (n + cell - 1) // cell
    assert t["cell_points"] == cell and t["cells"] == info["cells"]
    assert t["bytes"] == info["cells"] * cell * TILE_BYTES[tag]
    assert t["words_differing"] == 0
    return t


@pytest.mark.parametrize("delta", [1e-4, 0.5, 40.0])
@pytest.mark.parametrize("cell", [512, 256])
@pytest.mark.parametrize("tag", list(MODELS))
def test_votes_of_a_scan_do_not_depend_on_the_tiles(ctx, tag, cell, delta):
    data = _cloud(tag)
    oc = O.cfg(MODELS[tag][1], MODELS[tag][2], delta)
    _prepare(ctx, tag, data, delta, cell)
    for H in (1024, 64):
        par, valid, off = _scan(ctx, H, 0)
        par1, valid1, on = _scan(ctx, H, 1)
        _check_tiles(ctx, tag, cell)
        assert np.array_equal(par, par1, equal_nan=True) and np.array_equal(valid, valid1)
        assert np.array_equal(on, off), (H, np.flatnonzero(on != off)[:8])
        want = O.scan_many(oc, par, valid, data)
        assert valid.sum() > 0 and want.max() > 0
        assert np.array_equal(np.where(valid > 0, on, 0), want), (H, np.flatnonzero(np.where(valid > 0, on, 0) != want)[:8])


def _batch(ctx, bound, tiles):
    ctx.set_option("scan_bound", bound)
    ctx.set_option("scan_tiles", tiles)
    r = ctx.batch_fit(SEED, 0, 1024)
    par, valid, votes = ctx.hypotheses()
    return int(r["info"].best_index), int(r["info"].best_votes), par.copy(), valid.copy(), votes.copy()


@pytest.mark.parametrize("delta", [1e-4, 0.5, 40.0])
@pytest.mark.parametrize("cell", [512, 256])
@pytest.mark.parametrize("tag", list(MODELS))
def test_votes_of_a_batch_counted_and_bounded(ctx, tag, cell, delta):
    data = _cloud(tag)
    oc = O.cfg(MODELS[tag][1], MODELS[tag][2], delta)
    _prepare(ctx, tag, data, delta, cell)
    res = {(b, t): _batch(ctx, b, t) for b in (0, 1) for t in (0, 1)}
    _check_tiles(ctx, tag, cell)
    par, valid = res[(0, 1)][2], res[(0, 1)][3]
    want = O.scan_many(oc, par, valid, data)
    for b in (0, 1):
        on, off = res[(b, 1)], res[(b, 0)]
        assert on[:2] == off[:2]
        assert np.array_equal(on[2], par, equal_nan=True) and np.array_equal(on[3], valid)
        assert np.array_equal(on[4], off[4]), (b, np.flatnonzero(on[4] != off[4])[:8])
        assert (on[0], on[1]) == (int(np.argmax(want)), int(want.max()))         # first maximum, exact votes
    full = np.where(valid > 0, res[(0, 1)][4], 0)
    assert np.array_equal(full, want), np.flatnonzero(full != want)[:8]
    # the bounded scan: a hypothesis is counted to the end -- the oracle's count, exactly -- or skipped: it reports 0,
    # and its true count could not have become the running maximum at its index (first maximum: ties lose)
    bounded = np.where(valid > 0, res[(1, 1)][4], 0)
    skipped = bounded != want
    assert np.all(bounded[skipped] == 0), np.flatnonzero(skipped & (bounded != 0))[:8]
    runmax = np.maximum.accumulate(want)
    at = np.flatnonzero(skipped)
    assert not skipped[0] and np.all(want[at] <= runmax[at - 1]), at[:8]


@pytest.mark.parametrize("tag", list(MODELS))
def test_an_upload_a_million_away_from_the_origin(ctx, tag):
    """the tile holds fl32(x - centre) with the subtraction in fp64, as cells_load has it: coordinates of 1e6 lose nothing"""
    dim = MODELS[tag][2]
    data = np.ascontiguousarray(_cloud(tag) + np.array([1.0e6, -2.0e6, 3.0e6])[:dim])
    oc = O.cfg(MODELS[tag][1], dim, 0.5)
    _prepare(ctx, tag, data, 0.5, 0)
    for H in (1024, 64):
        par, valid, off = _scan(ctx, H, 0)
        _, _, on = _scan(ctx, H, 1)
        assert np.array_equal(on, off), (H, np.flatnonzero(on != off)[:8])
        assert np.array_equal(np.where(valid > 0, on, 0), O.scan_many(oc, par, valid, data))
    assert ctx.scan_tiles_check()["words_differing"] == 0 and ctx.scan_tiles_check()["cell_points"] > 0


def test_the_option_builds_keeps_and_drops_the_tiles(ctx):
    """0 before the index: nothing is built; 1 later: built in front of the next scan without touching the index; 0
    again: the tiles stay in place unread; a new upload drops them with the index.  Values other than 0 and 1 are refused."""
    data = _cloud("plane3")
    ctx.set_option("scan_tiles", 0)
    ctx.set_option("scan_index", 2)
    ctx.set_model(L.PLANE, 3, 0.5).upload(data)
    _, _, off = _scan(ctx, 1024, 0)
    assert ctx.index_info()["built"] and ctx.scan_tiles_check()["cell_points"] == 0
    _, _, on = _scan(ctx, 1024, 1)
    assert _check_tiles(ctx, "plane3", 512)["bytes"] == 4 * 512 * 12
    assert np.array_equal(on, off)
    _, _, off2 = _scan(ctx, 64, 0)
    assert ctx.scan_tiles_check()["cell_points"] == 512
    _, _, on2 = _scan(ctx, 64, 1)
    assert np.array_equal(on2, off2)
    ctx.upload(data[:600])
    assert ctx.scan_tiles_check()["cell_points"] == 0
    _, _, small = _scan(ctx, 64, 1)
    assert _check_tiles(ctx, "plane3", 512, n=600)["cells"] == 2
    for bad in (-1, 2):
        with pytest.raises(L.LsqrError) as e:
            ctx.set_option("scan_tiles", bad)
        assert e.value.status == L.ERR_INVALID and "scan_tiles" in str(e.value)
