"""Chunked early exit of the dense / US scans (csrc/earlyexit.h; run with -m gpu): the batch entry points stop counting a
hypothesis that can no longer become the running maximum -- winner, consensus set, fit and the replay of the adaptive
loop must equal those of counting everything (scan_bound 0) and the serial oracle's."""
import numpy as np
import pytest
import torch  # (before the library loads its own HIP runtime: the leak test reads the device's free memory through torch)

from lsqrrecipes_amd import _lib as L, synth
from lsqrrecipes_amd.context import Context, replay

pytestmark = pytest.mark.gpu


def _ctx(model, dim, delta, ls, data):
    c = Context(0)
    c.set_model(model, dim, delta, ls).upload(data)
    return c


def _both(model, dim, delta, ls, data, H, seed=0xC0FFEE, first=0):
    out = []
    for bound in (1, 0):
        with _ctx(model, dim, delta, ls, data) as c:
            c.set_option("scan_bound", bound)
            r = c.batch_fit(seed, first, H, want_consensus=True)
            _, valid, votes = c.hypotheses(params=False)
            out.append((r, valid.copy(), votes.copy(), c.scan_work()))
    return out


def _check_pair(ee, full, H, n):
    (r1, valid1, v1, w1), (r0, valid0, v0, w0) = ee, full
    assert w1["early_exit"] and not w0["early_exit"]
    assert w0["row_hypothesis_pairs"] == w0["row_hypothesis_pairs_all"] == H * n
    assert w1["row_hypothesis_pairs"] <= H * n + 16 * 4096 * H // 16
    # same winner, same consensus set, same fit
    assert r1["info"].best_index == r0["info"].best_index and r1["info"].best_votes == r0["info"].best_votes
    assert np.array_equal(r1["consensus"], r0["consensus"])
    assert np.array_equal(r1["params"], r0["params"])
    assert np.array_equal(valid1, valid0)
    # an abandoned hypothesis reports a partial count: never more than the full count, and never a new running maximum
    assert np.all(v1 <= v0)
    run = np.maximum.accumulate(np.where(valid0 > 0, v0, 0))
    prev = np.concatenate([[0], run[:-1]])
    partial = v1 != v0
    assert np.all(v0[partial] <= prev[partial])          # it was not a record of the serial loop ...
    assert np.all(v1[partial] <= prev[partial])          # ... and its reported count is inert as well
    # the records of the serial loop (strict '>') carry their exact counts
    rec = (valid0 > 0) & (v0 > prev)
    assert np.array_equal(v1[rec], v0[rec])
    return partial.sum()


@pytest.mark.parametrize("frac,H", [(0.05, 1024), (0.02, 256), (0.3, 512)])
def test_dense_early_exit_equals_full_count(frac, H):
    m = 300_000
    rows = synth.dense(m, 64, frac, seed=11)[0]
    ee, full = _both(L.DENSE, 64, 0.1, 0, rows, H)
    _check_pair(ee, full, H, m)
    if frac <= 0.05:   # a good 64-row sample exists (it agrees with ~30 % of the rows): the wrong solves are abandoned
        assert ee[3]["dropped_first"] > H // 2 and ee[3]["row_hypothesis_pairs"] < 0.9 * H * m, ee[3]  # once fewer rows remain
    # the replay of the adaptive loop over the batch is the same either way
    s = np.zeros((H, 64), dtype=np.uint32)
    a = replay(m, 64, 0.999, s, ee[1], ee[2], dedup=False)
    b = replay(m, 64, 0.999, s, full[1], full[2], dedup=False)
    assert (a["best_index"], a["best_votes"], a["num_tries"], a["i"]) == (b["best_index"], b["best_votes"], b["num_tries"], b["i"])


@pytest.mark.parametrize("frac,H,n", [(0.5, 4096, 200_000), (0.3, 1024, 100_000), (0.8, 2048, 150_000)])
def test_us_early_exit_equals_full_count(frac, H, n):
    rec = synth.us_single_fast(n, frac, seed=5)[0]
    ee, full = _both(L.US_SINGLE, 0, 3.0, L.LS_ANALYTIC, rec, H)
    _check_pair(ee, full, H, n)
    if frac <= 0.5:   # (a wrong model without votes reports 0 either way: the selection's own count says what was dropped)
        assert ee[3]["dropped_first"] > H // 2 and ee[3]["row_hypothesis_pairs"] < 0.8 * H * n, ee[3]


def test_us_pointer_and_phantom_early_exit():
    rec = synth.us_pointer(120_000, 0.4, seed=3)[0]
    ee, full = _both(L.US_POINTER, 0, 3.0, L.LS_ANALYTIC, rec, 1024)
    _check_pair(ee, full, 1024, 120_000)
    ph = synth.plane_phantom_fast(100_000, 0.03, seed=4, pixel_sigma=0.05)[0]
    ee, full = _both(L.PHANTOM, 0, 2.0, L.LS_ANALYTIC, ph, 512)
    _check_pair(ee, full, 512, 100_000)


def test_adaptive_ransac_is_unchanged_by_the_early_exit():
    """lsqr_ransac (RANSAC<T,S>::compute): iteration count, winner and consensus set with and without the early exit,
    with the running maximum of earlier batches as the bound"""
    n = 150_000
    rec = synth.us_single_fast(n, 0.7, seed=9)[0]      # 0.3^4: ~1 % good samples -> several batches
    res = []
    for bound in (1, 0):
        with _ctx(L.US_SINGLE, 0, 3.0, L.LS_ANALYTIC, rec) as c:
            c.set_option("scan_bound", bound)
            r = c.ransac(0.999, seed=77)
            res.append(r)
    a, b = res
    assert a["info"].iterations == b["info"].iterations and a["info"].best_index == b["info"].best_index
    assert a["info"].best_votes == b["info"].best_votes and np.array_equal(a["consensus"], b["consensus"])
    assert np.array_equal(a["params"], b["params"])
    assert a["info"].iterations > 256          # more than the first batch


def test_early_exit_against_the_serial_oracle():
    from oracle import pyoracle as O
    n, H = 70_000, 256
    rec = synth.us_single_fast(n, 0.5, seed=21)[0]
    with _ctx(L.US_SINGLE, 0, 3.0, L.LS_ANALYTIC, rec) as c:
        r = c.batch_fit(123, 0, H, want_consensus=True)
        assert c.scan_work()["early_exit"]
        subs = O.ctr_subsets(123, 0, H, n, 4)
        oc = O.cfg(O.US_SINGLE, 3, 3.0, O.LS_ALGEBRAIC)
        best, bi, bpar = 0, -1, None
        for i, s in enumerate(subs):            # the serial loop's winner: first maximum, strict '>'
            par = O.estimate(oc, rec[s])
            if not len(par):
                continue
            v = O.scan(oc, par, rec)[0]
            if v > best:
                best, bi, bpar = v, i, par
        assert abs(int(r["info"].best_votes) - best) <= 2 and (r["info"].best_index == bi or abs(int(r["info"].best_votes) - best) > 0)
        if r["info"].best_index == bi:
            cnt, mask = O.scan(oc, c.hypothesis(bi)[0], rec)
            assert np.array_equal(mask, r["consensus"])


def test_contexts_release_their_device_memory():
    """A context that took the early-exit path owns the scan's device scratch (lsqr_hip.hip: ee_buffers) and gives it
    back when it is destroyed.  The scratch used to be missing from the destroy list: 2 344 192 bytes lost per context.
    The bound is half of what that leak costs over the cycles measured."""
    n, dim, H, cycles = 65_536, 64, 128, 16     # the smallest upload / batch whose dense scan takes the early exit
    ee_cap = 8192                                # hypotheses the selection kernels handle (kEeCap)
    ee_bytes = 256 + 3 * ee_cap * 4 + (4 + 64) * (ee_cap + 64) * 4   # [state | three selections | thresholds + rows]
    assert ee_bytes == 2_344_192
    rows = synth.dense(n, dim, 0.05, seed=11)[0]

    def cycle():
        with _ctx(L.DENSE, dim, 0.1, 0, rows) as c:
            c.batch_fit(0xC0FFEE, 0, H)
            assert c.scan_work()["early_exit"]   # the scratch was allocated

    cycle()                                      # warm-up: code objects, the runtime's own pools
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    for _ in range(cycles):
        cycle()
    torch.cuda.synchronize()
    drop = before - torch.cuda.mem_get_info()[0]
    print("free device memory dropped by %d bytes over %d contexts" % (drop, cycles))
    assert drop < cycles * ee_bytes // 2, drop
