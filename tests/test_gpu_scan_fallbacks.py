"""The fallback chains behind the matrix-core filters' worklist checks (lsqrrecipes_amd/csrc/lsqr_hip.hip: worklist_check).
A worklist segment never overflows on real data, so `scan_test_overflow` 1 makes every check answer "overflowed": the
dense scan then goes fp16 / fp32 filter -> fp64 filter -> exact kernel, the US calibrations and the plane phantom go
fp16 filter -> packed fp32 filter, and the early-exit drivers of the batch entry points hand over to the same chains.
Every path counts with the reference's exact predicate in the end, so the votes (and a batch's winner and fit) must not
change.  lsqr_last_error keeps the note of the last site that fell back (it is never cleared: unforced runs come first).
Sizes: the smallest that reach each path, ragged."""
import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L, synth
from lsqrrecipes_amd.context import Context

pytestmark = pytest.mark.gpu


def _first(data):
    return data[0] if isinstance(data, tuple) else data


def _err(ctx):
    return ctx._lib.lsqr_last_error(ctx._h)


def _scan(ctx, seed, H):
    ctx.hypotheses_sample(seed, 0, H)
    ctx.scan()
    _, valid, votes = ctx.hypotheses()
    return valid, votes


def _check_scan(ctx, seed, H, note, fp16):
    """votes unforced, forced and of the exact kernel (scan_filter 0); the site's note only in the forced run"""
    v0, c0 = _scan(ctx, seed, H)
    assert note not in _err(ctx), _err(ctx)
    if fp16:  # (the filter under test really ran)
        assert b"fp32 filter used" not in _err(ctx), _err(ctx)
    ctx.set_option("scan_test_overflow", 1)
    try:
        v1, c1 = _scan(ctx, seed, H)
        assert note in _err(ctx), _err(ctx)
    finally:
        ctx.set_option("scan_test_overflow", 0)
    ctx.set_option("scan_filter", 0)
    try:
        vx, cx = _scan(ctx, seed, H)
    finally:
        ctx.set_option("scan_filter", 1)
    assert v0.sum() > 0 and c0.max() > 0
    assert np.array_equal(v0, v1) and np.array_equal(v0, vx)
    assert np.array_equal(c0, c1)
    assert np.array_equal(c0, cx)


@pytest.mark.parametrize("ncols,dense_f32", [(64, 2), (64, 1), (16, 2)])
def test_dense_filters_fall_back_to_the_exact_kernel(ncols, dense_f32):
    """64 columns: fp16 (dense_f32 2) or fp32 (1) filter -> fp64 filter -> exact kernel; 16 columns: the fp64 filter is
    the only one.  The chain ends at the fp64 filter's check either way, whose note is the one that stays."""
    data = synth.dense(4_099, ncols, 0.05, seed=41)[0]
    with Context(0) as ctx:
        ctx.set_option("dense_f32", dense_f32)
        ctx.set_model(L.DENSE, ncols, 0.1, L.LS_ALGEBRAIC).upload(data)
        _check_scan(ctx, 43, 65, b"exact kernel used", fp16=ncols == 64 and dense_f32 == 2)


@pytest.mark.parametrize("kind", ["single", "phantom"])
def test_us_fp16_filter_falls_back_to_the_packed_fp32_filter(kind):
    if kind == "single":
        data, model, delta = _first(synth.us_single_fast(4_133, 0.3, seed=45)), L.US_SINGLE, 3.0
    else:
        data, model, delta = synth.plane_phantom_fast(4_133, 0.05, seed=46, pixel_sigma=0.05)[0], L.PHANTOM, 2.0
    with Context(0) as ctx:
        ctx.set_model(model, 0, delta, L.LS_ANALYTIC).upload(data)
        _check_scan(ctx, 47, 97, b"US fp16 filter: worklist segment overflow", fp16=True)


@pytest.mark.parametrize("kind", ["dense", "us"])
def test_early_exit_scans_fall_back_inside_batch_fit(kind):
    """lsqr_batch_fit's chunked early exit: dense -> the plain filters' chain above; US -> the early exit again on the
    packed fp32 filter.  Winner and fit equal the unforced batch's and the full count's (scan_bound 0)."""
    if kind == "dense":
        data, model, dim, delta, ls, H = synth.dense(70_001, 64, 0.05, seed=51)[0], L.DENSE, 64, 0.1, L.LS_ALGEBRAIC, 128
        note = b"exact kernel used"
    else:
        data, model, dim, delta, ls, H = _first(synth.us_single_fast(70_001, 0.3, seed=52)), L.US_SINGLE, 0, 3.0, L.LS_ANALYTIC, 256
        note = b"US fp16 filter: worklist segment overflow"
    with Context(0) as ctx:
        ctx.set_model(model, dim, delta, ls).upload(data)
        want = ctx.batch_fit(53, 0, H)
        assert note not in _err(ctx) and b"fp32 filter used" not in _err(ctx), _err(ctx)
        ctx.set_option("scan_test_overflow", 1)
        try:
            forced = ctx.batch_fit(53, 0, H)
            assert note in _err(ctx), _err(ctx)
        finally:
            ctx.set_option("scan_test_overflow", 0)
        ctx.set_option("scan_bound", 0)
        try:
            full = ctx.batch_fit(53, 0, H)
        finally:
            ctx.set_option("scan_bound", 1)
        assert want["status"] == L.OK and want["info"].best_votes > 0
        for got in (forced, full):
            assert got["status"] == want["status"], kind
            gi, wi = got["info"], want["info"]
            assert (gi.best_votes, gi.best_index, gi.fit.n_used) == (wi.best_votes, wi.best_index, wi.fit.n_used)
            assert np.allclose(got["params"], want["params"], rtol=1e-9, atol=1e-12), kind
