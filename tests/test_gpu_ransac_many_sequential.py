"""lsqr_ransac_many_sequential / Context.ransac_many_sequential: sequential RANSAC over many problems in one call, every
round one batched search on the survivors, which a segmented partition compacts on the device
(csrc/many_sequential.h).  The yardstick is the single-set path, never the new code: for every problem j,
Context.upload(problem j) + Context.ransac_sequential(p, max_models, seeds[j], min_votes) must give the same n_models,
status, iterations, best_index, best_votes, fraction, n_params, n_used and labels, bit for bit; parameters and cost
within rtol 1e-9 / atol 1e-8 (fits that differ at most in summation order); LM fields by the rules of
test_gpu_ransac_many_lm.py (same info class, |d nfev| <= 3).  A problem of zero records cannot be uploaded to a
context: it is held against the header's words instead (no round, n_models 0, every entry ERR_STATE / zero)."""
import ctypes as C

import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd import synth
from lsqrrecipes_amd.context import Context

pytestmark = pytest.mark.gpu
P = 0.999
TILE = 256         # records per tile of the partition (kBlock: one lane per record)
CHUNK = 16 * TILE  # records per part of the partition (kSeqChunk: one workgroup)
EXACT_KEYS = ("status", "iterations", "best_index", "best_votes", "fraction", "n_params", "n_used")
INFO_KEYS = EXACT_KEYS[1:] + ("lm_info", "lm_nfev", "cost")  # (evaluated depends on the batch schedule)


def _dense_clutter(n, seed):
    g = np.random.Generator(np.random.Philox(seed))
    return np.hstack([g.uniform(-1.0, 1.0, (n, 6)), g.uniform(-20.0, 20.0, (n, 1))])


# name -> (model, dim, delta, ls_type, planted(n, seed) -> inliers of one model, clutter(n, seed), max_iterations)
MODELS = {
    "plane": (L.PLANE, 3, 0.5, L.LS_ALGEBRAIC,
              lambda n, s: synth.plane(n, 0.0, seed=s, sigma=0.1)[0], lambda n, s: synth.plane(n, 1.0, seed=s)[0], 4096),
    "line": (L.LINE, 3, 0.5, L.LS_ALGEBRAIC,
             lambda n, s: synth.line(n, 0.0, seed=s, sigma=0.1)[0], lambda n, s: synth.line(n, 1.0, seed=s)[0], 4096),
    "sphere_geo": (L.SPHERE, 3, 0.5, L.LS_GEOMETRIC,
                   lambda n, s: synth.sphere(n, 0.0, seed=s, sigma=0.1)[0],
                   lambda n, s: synth.sphere(n, 1.0, seed=s)[0], 4096),
    "dense6": (L.DENSE, 6, 0.1, L.LS_ALGEBRAIC,
               lambda n, s: synth.dense(n, 6, outlier_frac=0.0, seed=s, noise=0.01)[0], _dense_clutter, 20000),
    "absor": (L.ABSOR, 3, 2.0, 0,
              lambda n, s: synth.absolute_orientation(n, 0.0, seed=s)[0],
              lambda n, s: synth.absolute_orientation(n, 1.0, seed=s)[0], 4096),
}
WIDTH = {"plane": 3, "line": 3, "sphere_geo": 3, "dense6": 7, "absor": 6}


def scene(name, n, planted_models=3, salt=0, share=(3, 10)):
    """planted models of share[0] / share[1] of the records each plus clutter, shuffled with a fixed permutation (the
    scene() of test_gpu_ransac_sequential.py, for any n: a part of no records is left out)"""
    planted, clutter = MODELS[name][4], MODELS[name][5]
    m = (share[0] * n) // share[1]
    parts = [planted(m, 0x51000 + 7 * j + 1000 * salt) for j in range(planted_models) if m > 0]
    rest = n - m * planted_models
    if rest > 0:
        parts.append(clutter(rest, 0x51999 + 1000 * salt))
    if not parts:
        return np.zeros((0, WIDTH[name]))
    data = np.vstack(parts)[np.random.default_rng(12345 + salt).permutation(n)]
    return np.ascontiguousarray(data)


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _setup(ctx, name, max_iterations=None):
    model, dim, delta, ls = MODELS[name][:4]
    ctx.set_model(model, dim, delta, ls)
    ctx.set_option("max_iterations", MODELS[name][6] if max_iterations is None else max_iterations)
    return ctx


def _reset(ctx):
    ctx.set_option("max_iterations", 0)
    ctx.set_option("many_round_hypotheses", 0)


def _ok_class(info):
    return 1 <= int(info) <= 4


def _single(ctx, probs, seeds, max_models, min_votes):
    """the yardstick: every problem alone through upload + ransac_sequential (None for a problem of no records)"""
    out = []
    for j, d in enumerate(probs):
        if len(d) == 0:
            out.append(None)
            continue
        ctx.upload(d)
        out.append(ctx.ransac_sequential(P, max_models, seeds=seeds[j], min_votes=min_votes))
    return out


def _check_against_single(res, singles, max_models):
    offs = res["offsets"]
    for j, w in enumerate(singles):
        lo, hi = int(offs[j]), int(offs[j + 1])
        if w is None:  # no records: no round runs
            assert hi == lo and res["n_models"][j] == 0 and np.all(res["status"][j] == L.ERR_STATE), j
            for key in INFO_KEYS + ("evaluated",):
                assert not np.any(res[key][j]), (j, key)
            assert not np.any(res["params"][j]), j
            continue
        print("problem %d: n=%d n_models %d/%d status %s/%s votes %s/%s nfev %s/%s" % (
            j, hi - lo, res["n_models"][j], w["n_models"], res["status"][j], w["status"], res["best_votes"][j],
            w["best_votes"], res["lm_nfev"][j], w["lm_nfev"]))
        assert res["n_models"][j] == w["n_models"], j
        for key in EXACT_KEYS:
            a, b = np.ascontiguousarray(res[key][j]), np.ascontiguousarray(w[key])
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (j, key, a, b)
        assert np.array_equal(res["labels"][lo:hi], w["labels"]), j
        for r in range(max_models):
            a, b = res["lm_info"][j][r], w["lm_info"][r]
            assert _ok_class(a) == _ok_class(b) and (a == 0) == (b == 0), (j, r, a, b)
            assert abs(int(res["lm_nfev"][j][r]) - int(w["lm_nfev"][r])) <= 3, (j, r)
            assert np.isclose(res["cost"][j][r], w["cost"][r], rtol=1e-9, atol=1e-8), (j, r, res["cost"][j][r], w["cost"][r])
            assert np.allclose(res["params"][j][r], w["params"][r], rtol=1e-9, atol=1e-8), (
                j, r, res["params"][j][r], w["params"][r])
            if w["status"][r] == L.ERR_STATE:  # a round that did not run: zeroed infos, no parameters
                for key in INFO_KEYS + ("evaluated",):
                    assert not np.any(res[key][j][r]), (j, r, key)
                assert not np.any(res["params"][j][r]), (j, r)


# ---- partition edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_partition_edges(ctx, name):
    max_models, min_votes = 4, 8
    try:
        _setup(ctx, name)
        k = ctx.K
        sizes = [0, k - 1, k, 40, TILE, TILE + 1, CHUNK, CHUNK + 1, 3 * CHUNK + 123]
        probs = [scene(name, n, salt=i) for i, n in enumerate(sizes)]
        seeds = (11 + 3 * np.arange(len(sizes) * max_models, dtype=np.uint64)).reshape(len(sizes), max_models)
        res = ctx.ransac_many_sequential(probs, P, max_models, seeds=seeds, min_votes=min_votes)
        singles = _single(ctx, probs, seeds, max_models, min_votes)
        assert [int(res["offsets"][i + 1] - res["offsets"][i]) for i in range(len(sizes))] == sizes
        # the partition ran: some problem went through more than one round, some problem of several parts among them
        assert max(w["n_models"] for w in singles if w is not None) >= 2 and singles[-1]["n_models"] >= 2
        assert res["n_models"][1] == 0 and np.all(res["status"][1] == L.ERR_STATE)  # k - 1 records: no round
        assert np.all(res["labels"][int(res["offsets"][1]):int(res["offsets"][2])] == -1)
        _check_against_single(res, singles, max_models)
    finally:
        _reset(ctx)


# ---- shrinking active set -------------------------------------------------------------------------------------------
SHRINK_MODELS, SHRINK_MIN_VOTES = 4, 75
_shrink = {}


def _shrink_problems():
    """24 plane problems of about 600 records with 0, 1, 2 or 3 planted planes of a quarter each, interleaved so that
    stopped problems lie between running ones; computed once, never changed"""
    if "probs" not in _shrink:
        planted = [0, 3, 1, 2, 3, 0, 2, 1, 1, 0, 3, 2, 2, 3, 0, 1, 3, 1, 0, 2, 0, 2, 3, 1]
        probs = [scene("plane", 580 + 3 * j, planted_models=m, salt=100 + j, share=(1, 4)) for j, m in enumerate(planted)]
        for d in probs:
            d.setflags(write=False)
        _shrink["probs"] = probs
        _shrink["seeds"] = (1000 + np.arange(len(probs) * SHRINK_MODELS, dtype=np.uint64)).reshape(-1, SHRINK_MODELS)
    return _shrink["probs"], _shrink["seeds"]


def _shrink_singles(ctx):
    if "singles" not in _shrink:
        probs, seeds = _shrink_problems()
        _shrink["singles"] = _single(ctx, probs, seeds, SHRINK_MODELS, SHRINK_MIN_VOTES)
    return _shrink["singles"]


def test_shrinking_active_set(ctx):
    probs, seeds = _shrink_problems()
    try:
        _setup(ctx, "plane")
        singles = _shrink_singles(ctx)
        nm = [w["n_models"] for w in singles]
        print("single path n_models:", nm)
        # a condition on the inputs: the mix of problems that stop at different rounds is there
        assert len(set(nm)) >= 3 and 0 in nm, nm
        res = ctx.ransac_many_sequential(probs, P, SHRINK_MODELS, seeds=seeds, min_votes=SHRINK_MIN_VOTES)
        _check_against_single(res, singles, SHRINK_MODELS)
        # rounds that did not run are ERR_STATE with zeroed infos
        ran = np.sum(res["status"] != L.ERR_STATE, axis=1)
        assert np.all(ran >= res["n_models"]) and np.all(ran <= res["n_models"] + 1) and np.any(ran < SHRINK_MODELS)
        for j in range(len(probs)):
            assert np.all(res["status"][j][ran[j]:] == L.ERR_STATE), j
            for key in INFO_KEYS + ("evaluated",):
                assert not np.any(res[key][j][ran[j]:]), (j, key)
        # the labels are the claims: round r of problem j labelled best_votes records
        for j in range(len(probs)):
            lab = res["labels"][int(res["offsets"][j]):int(res["offsets"][j + 1])]
            assert lab.min() >= -1 and lab.max() < res["n_models"][j], j
            for r in range(res["n_models"][j]):
                assert np.sum(lab == r) == res["best_votes"][j][r], (j, r)
    finally:
        _reset(ctx)


# ---- independence ---------------------------------------------------------------------------------------------------
def _problem_bytes(res, j):
    lo, hi = int(res["offsets"][j]), int(res["offsets"][j + 1])
    out = [np.int64(res["n_models"][j]).tobytes(), res["labels"][lo:hi].tobytes()]
    for key in INFO_KEYS + ("status", "params"):
        out.append(np.ascontiguousarray(res[key][j]).tobytes())
    return out


def test_independence(ctx):
    probs, seeds = _shrink_problems()
    n = len(probs)
    try:
        _setup(ctx, "plane")
        base = ctx.ransac_many_sequential(probs, P, SHRINK_MODELS, seeds=seeds, min_votes=SHRINK_MIN_VOTES)
        assert len(set(base["n_models"].tolist())) >= 3
        perm = np.random.default_rng(7).permutation(n)
        a = ctx.ransac_many_sequential([probs[i] for i in perm], P, SHRINK_MODELS, seeds=seeds[perm],
                                       min_votes=SHRINK_MIN_VOTES)
        sub = [1, 4, 5, 12, 20, 23]
        b = ctx.ransac_many_sequential([probs[i] for i in sub], P, SHRINK_MODELS, seeds=seeds[sub],
                                       min_votes=SHRINK_MIN_VOTES)
        ctx.set_option("many_round_hypotheses", 700)  # a first round of 24 x 256 hypotheses is cut in nine
        c = ctx.ransac_many_sequential(probs, P, SHRINK_MODELS, seeds=seeds, min_votes=SHRINK_MIN_VOTES)
        for q, i in enumerate(perm):
            assert _problem_bytes(a, q) == _problem_bytes(base, i), i
        for q, i in enumerate(sub):
            assert _problem_bytes(b, q) == _problem_bytes(base, i), i
        for i in range(n):
            assert _problem_bytes(c, i) == _problem_bytes(base, i), i
    finally:
        _reset(ctx)


# ---- strided input --------------------------------------------------------------------------------------------------
def _raw(ctx, recs, stride, offs, seeds, max_models, min_votes, fill=None):
    """the C call on caller-made buffers -> (status, n_models, params, labels, status_out, infos bytes)"""
    lib = L.load()
    n, m = len(offs) - 1, max_models
    rows = max(n * m, 1)
    params = np.zeros((rows, ctx.P)) if fill is None else np.full((rows, ctx.P), float(fill))
    labels = np.full(max(int(offs[-1]), 1), -1 if fill is None else fill, dtype=np.int32)
    infos = (L.RansacInfo * rows)()
    status = np.full(rows, L.ERR_STATE if fill is None else fill, dtype=np.int32)
    n_models = np.full(max(n, 1), 0 if fill is None else fill, dtype=np.uintp)
    if fill is not None:
        C.memset(infos, 0x5A, C.sizeof(infos))
    st = lib.lsqr_ransac_many_sequential(ctx._h, L.ptr(recs), stride, L.ptr(offs), n, P, L.ptr(seeds), m, min_votes,
                                         L.ptr(params), L.ptr(labels), infos, L.ptr(status), L.ptr(n_models))
    return st, n_models, params, labels, status, bytes(infos)


@pytest.mark.parametrize("name", ["plane", "absor"])
def test_strided_input(ctx, name):
    sizes = [40, TILE + 1, CHUNK + 1, 700]
    probs = [scene(name, n, salt=50 + i) for i, n in enumerate(sizes)]
    W = WIDTH[name]
    offs = np.zeros(len(sizes) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(sizes)
    tight = np.ascontiguousarray(np.vstack(probs))
    padded = np.full((len(tight), W + 1), np.nan)
    padded[:, :W] = tight
    seeds = np.arange(5, 5 + 3 * len(sizes), dtype=np.uint64)
    try:
        _setup(ctx, name)
        want = _raw(ctx, tight, W * 8, offs, seeds, 3, 8)
        got = _raw(ctx, padded, (W + 1) * 8, offs, seeds, 3, 8)
        assert want[0] == got[0] == L.OK and np.max(want[1]) >= 2
        for a, b in zip(want[1:5], got[1:5]):
            assert a.tobytes() == b.tobytes()
        assert want[5] == got[5]
    finally:
        _reset(ctx)


# ---- contract -------------------------------------------------------------------------------------------------------
def test_contract(ctx):
    probs, seeds = _shrink_problems()
    probs, seeds = probs[:6], seeds[:6]
    lib = L.load()
    try:
        _setup(ctx, "plane")
        own = scene("plane", 3000, salt=77)
        ctx.upload(own)
        first = ctx.ransac(P, seed=9)
        seq_first = ctx.ransac_sequential(P, 3, min_votes=100)
        res = ctx.ransac_many_sequential(probs, P, SHRINK_MODELS, seeds=seeds, min_votes=SHRINK_MIN_VOTES)
        # the shared tile body: lsqr_ransac_sequential on the same context answers as before the call, and so does
        # the context's own upload
        seq_again = ctx.ransac_sequential(P, 3, min_votes=100)
        again = ctx.ransac(P, seed=9)
        assert seq_first["n_models"] == seq_again["n_models"] >= 2
        for key in INFO_KEYS + ("status", "params", "labels", "evaluated"):
            assert np.ascontiguousarray(seq_first[key]).tobytes() == np.ascontiguousarray(seq_again[key]).tobytes(), key
        assert first["status"] == again["status"] == L.OK and len(first["consensus"]) == 3000
        assert np.array_equal(first["consensus"], again["consensus"])
        assert first["params"].tobytes() == again["params"].tobytes()
        for key in ("fraction", "iterations", "best_index", "best_votes", "n_params"):
            assert getattr(first["info"], key) == getattr(again["info"], key), key
        # want_labels=False: the same decisions without the label buffer
        nolab = ctx.ransac_many_sequential(probs, P, SHRINK_MODELS, seeds=seeds, min_votes=SHRINK_MIN_VOTES,
                                           want_labels=False)
        assert nolab["labels"] is None and np.array_equal(nolab["n_models"], res["n_models"])
        for key in INFO_KEYS + ("status", "params"):
            assert nolab[key].tobytes() == res[key].tobytes(), key
        # max_models == 0 zeroes n_models and runs nothing
        zero = ctx.ransac_many_sequential(probs, P, 0)
        assert zero["status"].shape == (6, 0) and not np.any(zero["n_models"]) and np.all(zero["labels"] == -1)
        recs = np.ascontiguousarray(np.vstack(probs))
        offs = res["offsets"]
        st, n_models, params, labels, status, infos = _raw(ctx, recs, 24, offs, seeds, 0, 0, fill=42)
        assert st == L.OK and not np.any(n_models)
        assert np.all(params == 42.0) and np.all(labels == 42) and np.all(status == 42) and infos == b"\x5a" * len(infos)
        # null arguments with max_models > 0: nothing written
        n_models = np.full(6, 42, dtype=np.uintp)
        status = np.full(6 * SHRINK_MODELS, 42, dtype=np.int32)
        params = np.full((6 * SHRINK_MODELS, ctx.P), 42.0)
        infos = (L.RansacInfo * (6 * SHRINK_MODELS))()
        args = dict(seeds=seeds, params=params, infos=infos, status=status, n_models=n_models)
        for missing in args:
            a = dict(args, **{missing: None})
            p_ = lambda x: None if x is None else (x if x is infos else L.ptr(x))
            assert lib.lsqr_ransac_many_sequential(ctx._h, L.ptr(recs), 24, L.ptr(offs), 6, P, p_(a["seeds"]),
                                                   SHRINK_MODELS, 0, p_(a["params"]), None, p_(a["infos"]),
                                                   p_(a["status"]), p_(a["n_models"])) == L.ERR_INVALID, missing
            assert np.all(n_models == 42) and np.all(status == 42) and np.all(params == 42.0), missing
        # a US calibration: ERR_INVALID, outputs untouched
        ctx.set_model(L.US_SINGLE, 0, 3.0, L.LS_ANALYTIC)
        us = np.zeros((64, ctx.ND))
        uoffs = np.array([0, 32, 64], dtype=np.uint64)
        st, n_models, params, labels, status, infos = _raw(ctx, us, ctx.ND * 8, uoffs, seeds[:2, :2].copy(), 2, 0, fill=42)
        assert st == L.ERR_INVALID and np.all(n_models == 42)
        assert np.all(params == 42.0) and np.all(labels == 42) and np.all(status == 42) and infos == b"\x5a" * len(infos)
        with pytest.raises(L.LsqrError):
            ctx.ransac_many_sequential((us, uoffs), P, 2)
    finally:
        _setup(ctx, "plane")
        _reset(ctx)
