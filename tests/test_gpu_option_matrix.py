"""The arrangements that lsqr_set_option selects and no other test does (include/lsqr_hip.h, "tuning knobs"): the contract
is that no answer depends on a knob, so every arrangement's votes and validity flags equal, bit for bit, those of the
exhaustive fp64 kernel on the same context (scan_index 0, scan_filter 0), and a sample of at most 64 hypotheses per
case -- hypothesis 0, the argmax, the last one, every injected row -- equals the oracle's count.

  scan_hsplit        k_scan_cells with the hypothesis range of a tile cut into segments of whole 64-groups (segments
                     starting past H leave at once) and the blockIdx.y segments of k_scan_us_f32
  scan_pairs 1 / 2   full counts of sphere, line and the small-batch plane through the counted, statically balanced
                     k_scan_pairs; plane and sphere batches of >= 1024 through k_scan_cells
  scan_hyp_order     the plane's full count of 1024..4096 hypotheses in sampling order against the key order
  scan_pairs_waves   k_scan_pairs' equal-share split with fewer workgroups than a quarter of the cells
  scan_presorted     an index whose cells are runs of the upload order
  dense_mask_ring    k_mask_syrk_dense<4, 2> at n = 64
  upload_threads     the staged upload's ring of pinned chunks, slot reuse included

Sizes are the smallest that reach each branch: 70 001 points = 137 cells of 512 / 274 cells of 256 with a ragged last
cell; H = 200 = three whole groups of 64 and one of 8; H = 1100 = 18 groups, the last partial."""
import contextlib
from types import SimpleNamespace

import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L, synth
from lsqrrecipes_amd.context import Context
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu
N = 70_001
SEED = 0x0A7C

# every option this module touches, with the library's default
DEFAULTS = {"scan_index": 1, "scan_filter": 1, "scan_hsplit": 0, "scan_pairs": 0, "scan_hyp_order": 1,
            "scan_pairs_waves": 0, "scan_presorted": 0, "scan_block": 0, "scan_cell": 0, "scan_bound": 1,
            "scan_ppl": 0, "us_mfma": 1, "dense_mask_ring": 4, "upload_threads": -1}

# name -> model, dimension, ls_type, generator
POINT = {"plane3": (L.PLANE, 3, L.LS_GEOMETRIC, synth.plane), "plane2": (L.PLANE, 2, L.LS_GEOMETRIC, synth.plane),
         "sphere3": (L.SPHERE, 3, L.LS_ALGEBRAIC, synth.sphere),
         "line3": (L.LINE, 3, L.LS_GEOMETRIC, synth.line), "line2": (L.LINE, 2, L.LS_GEOMETRIC, synth.line)}


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    for k, v in DEFAULTS.items():
        c.set_option(k, v)
    c.close()


@contextlib.contextmanager
def _options(ctx, **opts):
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k in opts:
            ctx.set_option(k, DEFAULTS[k])


_CLOUDS, _REFS = {}, {}


def _cloud(case, n=N):
    if (case, n) not in _CLOUDS:
        model, dim, ls, gen = POINT[case]
        _CLOUDS[(case, n)] = gen(n, 0.5, dim=dim)[0]
    return _CLOUDS[(case, n)]


def _upload(ctx, case, data=None):
    model, dim, ls, _ = POINT[case]
    data = _cloud(case) if data is None else data
    ctx.set_model(model, dim, 0.5, ls).upload(data)
    return data, O.cfg(model, dim, 0.5, ls)


def _bases(H):
    return (0, (H // 2) & ~63, H - 7)


def _subsets(n, k, H):
    """the sampler's subsets with a degenerate subset and a two-equal-points subset (the rows test_gpu_scan_lean
    injects; estimate() refuses them: NaN parameters, not valid) in the first, a middle and the last group of 64"""
    s = O.ctr_subsets(SEED, 0, H, n, k).astype(np.uint32)
    for base in _bases(H):
        s[base + 1] = s[base + 1][0]                  # one point, k times
        s[base + 5, :2] = s[base + 5, 0]              # two equal points
    return s


def _pick(H, votes, injected=()):
    """at most 64 hypotheses for the oracle: 0, the argmax, the last one, the injected rows, the rest spread evenly"""
    must = np.unique(np.r_[0, int(np.argmax(votes)), H - 1, np.asarray(injected, dtype=np.int64)]).astype(np.int64)
    rest = np.setdiff1d(np.arange(0, H, max(1, H // 50)), must)[:64 - len(must)]
    pick = np.unique(np.r_[must, rest])
    assert len(pick) <= 64
    return pick


def _scan(ctx, subsets, workload=False, **opts):
    with _options(ctx, **opts):
        ctx.hypotheses_from_subsets(subsets)
        ctx.scan()
        par, valid, votes = ctx.hypotheses()
        info = ctx.index_info()
        wl = ctx.scan_workload() if workload else None
    return SimpleNamespace(par=par, valid=valid.copy(), votes=votes.copy(), info=info, wl=wl)


def _reference(ctx, tag, data, oc, H):
    """the exhaustive fp64 kernel's votes of the injected batch on the context's current upload (computed once per
    upload and H), checked against the oracle on the sample"""
    if (tag, H) not in _REFS:
        subsets = _subsets(len(data), ctx.K, H)
        r = _scan(ctx, subsets, scan_index=0, scan_filter=0)
        injected = [b + d for b in _bases(H) for d in (1, 5)]
        for b in _bases(H):                            # invalid hypotheses with NaN parameters in three groups of 64
            assert not r.valid[b + 1] and np.isnan(r.par[b + 1]).all()
            if ctx.K <= 3:
                assert not r.valid[b + 5] and np.isnan(r.par[b + 5]).all()
        assert r.valid.sum() >= H - 6 and r.votes.max() > 0.1 * len(data)      # ... among near-model hypotheses
        r.subsets, r.pick = subsets, _pick(H, r.votes, injected)
        r.want = O.scan_many(oc, r.par[r.pick], r.valid[r.pick], data)
        assert np.array_equal(np.where(r.valid[r.pick] > 0, r.votes[r.pick], 0), r.want)
        _REFS[(tag, H)] = r
    return _REFS[(tag, H)]


def _indexed(ctx, ref, workload=False, **opts):
    """one scan over the index (scan_index 2) under `opts`, compared with the reference"""
    got = _scan(ctx, ref.subsets, workload=workload, scan_index=2, **opts)
    assert got.info["built"], opts
    assert got.info["cells"] == -(-got.info["observations"] // got.info["cell_points"]), got.info
    assert np.array_equal(got.valid, ref.valid), opts
    assert not got.valid[1] and np.isnan(got.par[1]).all(), opts
    assert np.array_equal(got.votes, ref.votes), (opts, np.flatnonzero(got.votes != ref.votes)[:8])
    assert np.array_equal(np.where(got.valid[ref.pick] > 0, got.votes[ref.pick], 0), ref.want), opts
    return got


# ---- 1. two-level scan arrangements ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(POINT))
def test_hypothesis_segments_of_the_tiled_scan(ctx, case):
    """k_scan_cells with hsplit > 1.  H = 200 (4 groups, the last of 8): the host caps the value at the groups, so 128
    is 4; with 3, hseg = 128 and the third segment starts at 256 >= H and leaves.  H = 1100 with scan_pairs 2 (plane
    and sphere would take k_scan_pairs there): 18 groups in 5 segments of 256, the last one [1024, 1100).  Each with
    the hypothesis broadcast by v_readlane (256) and through LDS (257), and with the model's own choice (0)."""
    data, oc = _upload(ctx, case)
    ref = _reference(ctx, case, data, oc, 200)
    for block in (0, 256, 257):
        for hs in (1, 2, 3, 4, 128):
            got = _indexed(ctx, ref, scan_hsplit=hs, scan_block=block)
            assert got.info["cells"] == (274 if POINT[case][0] == L.LINE else 137)
    ref = _reference(ctx, case, data, oc, 1100)
    for block in (0, 256, 257):
        _indexed(ctx, ref, scan_pairs=2, scan_hsplit=5, scan_block=block)


@pytest.mark.parametrize("case,H", [("sphere3", 200), ("sphere3", 1100), ("line3", 200), ("line3", 1100),
                                    ("line2", 200), ("line2", 1100), ("plane3", 200), ("plane2", 200)])
def test_full_count_through_the_counted_pairs_kernels(ctx, case, H):
    """scan_pairs 1: a full count (h_dev null, h_off 0) through run_scan_pairs -- counting pass, k_tile_costs,
    k_scan_pairs<SphereCell / LineCell / PlaneCell>, k_votes_reduce -- where the default is k_scan_cells: line at any H,
    sphere and plane below 1024.  Cells of the model's size and of 256, both broadcasts.  Level 1 does not depend on
    the level-2 kernel: the surviving (hypothesis, cell) pairs equal those under scan_pairs 2."""
    data, oc = _upload(ctx, case)
    ref = _reference(ctx, case, data, oc, H)
    for cell in (0, 256):
        tiled = _indexed(ctx, ref, workload=True, scan_pairs=2, scan_cell=cell)
        for block in (256, 257):
            got = _indexed(ctx, ref, workload=True, scan_pairs=1, scan_cell=cell, scan_block=block)
            if cell:
                assert got.info["cell_points"] == 256 and got.info["cells"] == 274
            assert got.wl["pairs"] == tiled.wl["pairs"] and got.wl["pairs"] > 0
            assert got.wl["cells"] == tiled.wl["cells"] == got.info["cells"]


@pytest.mark.parametrize("H", [1024, 1100, 4096])
def test_plane_full_count_in_sampling_order_and_in_key_order(ctx, H):
    """scan_hyp_order 0 (run_scan_pairs on the batch as sampled) against 1 (k_plane_order, k_gather_rows, k_scatter_perm
    around it) at the same H: 1024 is the threshold, 1100 pads the bitonic network, 4096 = kOrderCap fills it.  The NaN
    rows sort to the end of the key order and come back to their own positions: validity and votes are equal."""
    data, oc = _upload(ctx, "plane3")
    ref = _reference(ctx, "plane3", data, oc, H)
    off = _indexed(ctx, ref, scan_hyp_order=0)
    on = _indexed(ctx, ref, scan_hyp_order=1)
    assert np.array_equal(on.votes, off.votes) and np.array_equal(on.valid, off.valid)
    for b in _bases(H):
        assert not on.valid[b + 1] and not off.valid[b + 1] and on.votes[b + 1] == 0 == off.votes[b + 1]


def _batch(ctx, H):
    r = ctx.batch_fit(SEED, 0, H, want_consensus=True)
    par, valid, votes = ctx.hypotheses()
    return SimpleNamespace(best=(int(r["info"].best_index), int(r["info"].best_votes)), params=r["params"].copy(),
                           consensus=r["consensus"].copy(), par=par, valid=valid.copy(), votes=votes.copy())


def test_pairs_kernel_with_fewer_workgroups_than_cell_quarters(ctx):
    """scan_pairs_waves: 300 000 points in cells of 256 = 1172 cells, so n_cells / 4 = 293 workgroups would run; with
    1 workgroup per CU the grid is capped at 256 and k_scan_pairs' equal-share split hands every workgroup a share that
    is not a whole number of cells (as at the 10 M-point workload, where the cap always binds).  Plain scans and whole
    batches, counted (scan_bound 0) and bounded."""
    H, HB = 1100, 2048
    data = _cloud("plane3", 300_000)
    _, oc = _upload(ctx, "plane3", data)
    ref = _reference(ctx, "plane3@300k", data, oc, H)
    with _options(ctx, scan_index=0, scan_filter=0, scan_bound=0):
        exact = _batch(ctx, HB)
    pick = _pick(HB, exact.votes)
    assert np.array_equal(np.where(exact.valid[pick] > 0, exact.votes[pick], 0),
                          O.scan_many(oc, exact.par[pick], exact.valid[pick], data))
    runmax = np.maximum.accumulate(np.where(exact.valid > 0, exact.votes, 0))
    for waves in (0, 1, 2):
        got = _indexed(ctx, ref, scan_cell=256, scan_pairs_waves=waves)
        assert got.info["cells"] > 1024 and got.info["cell_points"] == 256
        with _options(ctx, scan_index=2, scan_cell=256, scan_pairs_waves=waves, scan_bound=0):
            full = _batch(ctx, HB)
            ctx.set_option("scan_bound", 1)
            bounded = _batch(ctx, HB)
        for r in (full, bounded):
            assert r.best == exact.best and np.array_equal(r.consensus, exact.consensus), waves
            assert np.array_equal(r.params, exact.params) and np.array_equal(r.valid, exact.valid), waves
        assert np.array_equal(full.votes, exact.votes), (waves, np.flatnonzero(full.votes != exact.votes)[:8])
        # the bounded scan: a hypothesis is counted exactly, or reports 0 and could not have become the running maximum
        idx = np.flatnonzero(bounded.votes != exact.votes)
        assert np.all(bounded.votes[idx] == 0), waves
        assert np.all(exact.votes[idx[idx > 0]] <= runmax[idx[idx > 0] - 1]) and (0 not in idx or exact.votes[0] == 0)
        assert 0 < len(idx) < HB


@pytest.mark.parametrize("order", ["upload_random", "upload_sorted_by_x"])
@pytest.mark.parametrize("case", ["plane3", "sphere3", "line3"])
def test_index_over_cells_cut_from_the_upload_order(ctx, case, order):
    """scan_presorted 1, set before the first scan of the upload: build_index without Morton sort and k-d refinement.
    In the generator's random order every box spans the scene and (nearly) every (hypothesis, cell) pair survives
    level 1; ordered by x the cells are thin slabs.  Setting the option back drops the index: the next scan builds the
    usual one, and the votes are the same."""
    data = _cloud(case)
    if order == "upload_sorted_by_x":
        data = np.ascontiguousarray(data[np.argsort(data[:, 0])])
    Hs = (200, 1100) if case == "plane3" else (200,)
    pairs = {}
    try:
        _, oc = _upload(ctx, case, data)
        ctx.set_option("scan_presorted", 1)
        assert not ctx.index_info()["built"]
        refs = {H: _reference(ctx, case + "/" + order, data, oc, H) for H in Hs}
        for presorted in (1, 0):
            ctx.set_option("scan_presorted", presorted)
            assert not ctx.index_info()["built"]
            for H in Hs:
                got = _indexed(ctx, refs[H], workload=True)
                pairs[(presorted, H)] = got.wl["pairs"] / (float(H) * got.wl["cells"])
    finally:
        ctx.set_option("scan_presorted", 0)
    for H in Hs:
        print("scan_presorted %s %s H=%d: share of (hypothesis, cell) pairs that survive level 1: %.4f, with the "
              "option 0: %.4f" % (case, order, H, pairs[(1, H)], pairs[(0, H)]))
        assert 0.0 < pairs[(0, H)] <= 1.0 and 0.0 < pairs[(1, H)] <= 1.0
        if order == "upload_random":
            assert pairs[(1, H)] > pairs[(0, H)]


# ---- 2. US / phantom: packed fp32 filter with blockIdx.y segments -------------------------------------------------
@pytest.mark.parametrize("kind", ["single", "phantom"])
def test_us_packed_filter_with_hypothesis_segments(ctx, kind):
    """k_scan_us_f32 (us_mfma 0) with gridDim.y > 1: hseg = ceil(H / gridDim.y) is no multiple of anything.  H = 97 in
    2, 3 (segments from 33 and 66) and 7 segments; H = 600 with the automatic value (2: no other test reaches it) and
    in 5; two pairs of frames per lane (scan_ppl 0) and one (scan_ppl 2)."""
    if kind == "single":
        data, model, delta = synth.us_single_fast(4_133, 0.3, seed=45)[0], L.US_SINGLE, 3.0
    else:
        data, model, delta = synth.plane_phantom_fast(4_133, 0.05, seed=46, pixel_sigma=0.05)[0], L.PHANTOM, 2.0
    oc = O.cfg(model, 0, delta, L.LS_ANALYTIC)
    ctx.set_model(model, 0, delta, L.LS_ANALYTIC).upload(data)

    def scan(H, **opts):
        with _options(ctx, **opts):
            ctx.hypotheses_sample(47, 0, H)
            ctx.scan()
            par, valid, votes = ctx.hypotheses()
        return par, valid.copy(), votes.copy()

    for H, splits in ((97, (2, 3, 7)), (600, (0, 5))):
        par, valid, exact = scan(H, scan_filter=0)
        assert valid.sum() > 0 and exact.max() > 0
        pick = _pick(H, exact)
        want = O.scan_many(oc, par[pick], valid[pick], data)
        assert np.array_equal(np.where(valid[pick] > 0, exact[pick], 0), want)
        for ppl in (0, 2):
            for hs in splits:
                _, v, votes = scan(H, us_mfma=0, scan_ppl=ppl, scan_hsplit=hs)
                assert np.array_equal(v, valid), (H, ppl, hs)
                assert np.array_equal(votes, exact), (H, ppl, hs, np.flatnonzero(votes != exact)[:8])
                assert np.array_equal(np.where(v[pick] > 0, votes[pick], 0), want), (H, ppl, hs)
    err = ctx._lib.lsqr_last_error(ctx._h)
    assert b"filter used" not in err and b"kernel used" not in err, err      # no fallback took the count over


# ---- 3. dense: fused mask + normal equations with two tile buffers per wave at n = 64 ----------------------------
@pytest.mark.parametrize("m", [70_001, 5_000, 63])
def test_dense_fused_mask_with_two_and_four_tile_buffers(ctx, m):
    """dense_mask_ring 2 at n = 64 is k_mask_syrk_dense<4, 2> (otherwise only n = 49..63 reach it), 4 is <4, 4>: the
    inputs and the two bounds of test_fused_mask_and_block_equal_the_two_kernel_path"""
    n = 64
    rows, x_true, _ = synth.dense(m, n, 0.1, seed=3)
    x = x_true * (1 + 1e-3 * np.random.default_rng(1).standard_normal(n))
    want_cnt, want_mask = O.scan(O.cfg(O.DENSE, n, 0.1), x, rows)
    res = {}
    for ring in (2, 4):
        with _options(ctx, dense_mask_ring=ring):
            ctx.set_model(L.DENSE, n, 0.1, 0).upload(rows)
            mask, cnt = ctx.mask(x)
            fit, info = ctx.ls_fit(use_mask=True)
            batch = ctx.batch_fit(7, 0, 64, want_consensus=True) if m >= n else None
            res[ring] = (mask.copy(), cnt, fit.copy(), info.n_used, batch)
        assert cnt == want_cnt and np.array_equal(mask, want_mask), ring
    (_, _, f2, u2, b2), (_, _, f4, u4, b4) = res[2], res[4]
    assert u2 == u4 and (len(f2) == 0) == (len(f4) == 0)
    if len(f4):
        assert np.abs(f2 - f4).max() <= 1e-9 * max(1.0, np.abs(f4).max())
        if want_cnt >= 4 * n:
            sel = rows[want_mask.astype(bool)]
            want = np.linalg.lstsq(sel[:, :n], sel[:, n], rcond=None)[0]
            for f in (f2, f4):
                assert np.abs(f - want).max() <= 1e-6 * max(1.0, np.abs(want).max())
    if b4 is not None:
        assert b2["info"].best_index == b4["info"].best_index and b2["info"].best_votes == b4["info"].best_votes
        assert np.array_equal(b2["consensus"], b4["consensus"])
        assert (len(b2["params"]) == 0) == (len(b4["params"]) == 0)
        if len(b4["params"]):
            assert np.abs(b2["params"] - b4["params"]).max() <= 1e-9 * max(1.0, np.abs(b4["params"]).max())
            if b4["info"].best_votes >= 4 * n:
                sel = rows[b4["consensus"].astype(bool)]
                want = np.linalg.lstsq(sel[:, :n], sel[:, n], rcond=None)[0]
                for b in (b2, b4):
                    assert np.abs(b["params"] - want).max() <= 1e-6 * max(1.0, np.abs(want).max())


# ---- 4. staged upload --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1_400_003, 2_800_001])
def test_staged_upload_delivers_every_record(ctx, n):
    """upload_threads > 0 on >= 32 MiB: staged_upload's ring of 8 pinned 8 MiB chunks.  1 400 003 points = 33.6 MB = five
    chunks, the last partial; 2 800 001 = 67.2 MB = nine, the ninth reusing slot 0 behind its event.  1, 3 and 16 host
    threads.  Integrity without the plain path: the plane's residual (kernels.h: k_residuals, PlaneModel::residual =
    |n . (x - a)|) for the unit normal e_i through the origin is |x_i| exactly -- the other two products are zeros --
    so it must equal abs(data[:, i]) over all records; the buffer holds zeros before each staged upload (it is reused,
    and would otherwise still hold the right values from the upload before).  Then the votes of 64 sampled hypotheses against the plain
    upload's and the oracle's."""
    data = synth.plane(n, 0.5, seed=SEED)[0]
    assert data.shape == (n, 3) and np.isfinite(data).all() and data.nbytes >= 32 << 20
    oc = O.cfg(O.PLANE, 3, 0.5)
    ctx.set_model(L.PLANE, 3, 0.5)

    def votes_of_64():
        ctx.hypotheses_sample(SEED, 0, 64)
        ctx.scan()
        par, valid, votes = ctx.hypotheses()
        return par, valid.copy(), votes.copy()

    with _options(ctx, upload_threads=0):
        ctx.upload(data)
    par, valid, plain = votes_of_64()
    assert valid.all() and plain.max() > 0.1 * n
    assert np.array_equal(plain, O.scan_many(oc, par, valid, data))
    absdata = np.abs(data)
    zeros = np.zeros_like(data)
    for threads in (1, 3, 16):
        with _options(ctx, upload_threads=0):
            ctx.upload(zeros)                         # a byte that the staged upload leaves out must not hold its value
        assert not ctx.residuals(np.r_[1.0, np.zeros(5)]).any()
        with _options(ctx, upload_threads=threads):
            ctx.upload(data)
        for i in range(3):
            e = np.zeros(6)
            e[i] = 1.0
            got = ctx.residuals(e)
            assert np.array_equal(got, absdata[:, i]), (threads, i, np.flatnonzero(got != absdata[:, i])[:8])
        _, v, votes = votes_of_64()
        assert np.array_equal(v, valid) and np.array_equal(votes, plain), threads
