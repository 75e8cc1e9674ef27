"""lsqr_ransac_grouped_sequential / Context.ransac_grouped_sequential: several models per label over the records the
context holds on the device -- grouped there (csrc/grouped.h), the rounds of lsqr_ransac_many_sequential on the packed
copy (csrc/many_sequential.h), the round labels scattered back to upload order.  The yardstick is the existing path,
never the new code: the records are gathered by label on the host (np.argsort(kind="stable") on the in-range labels),
Context.ransac_many_sequential runs on that with the same seeds and the context's model and options as they are, and
its labels are permuted back to upload order (-1 for records in no group).  n_models, status, fraction, iterations,
best_index, best_votes, n_params, n_used, params, cost, lm_info, lm_nfev, offsets and labels must be equal bit for bit,
dtype and shape too (evaluated alone depends on the batch schedule).  Every test first asserts on the yardstick's
output that what it is about really occurs."""
import ctypes as C

import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd import synth
from lsqrrecipes_amd.context import Context

pytestmark = pytest.mark.gpu
P = 0.999
INT32_MIN = -2 ** 31
TILE = 256         # records per tile of the partition (kBlock)
CHUNK = 16 * TILE  # records per part of the partition (kSeqChunk)
MAX_MODELS, MIN_VOTES = 4, 8
KEYS = ("n_models", "status", "fraction", "iterations", "best_index", "best_votes", "n_params", "n_used", "params",
        "cost", "lm_info", "lm_nfev", "offsets")


def _dense_clutter(n, seed):
    g = np.random.Generator(np.random.Philox(seed))
    return np.hstack([g.uniform(-1.0, 1.0, (n, 6)), g.uniform(-20.0, 20.0, (n, 1))])


def _pivot(n, outlier_frac, seed):
    """pivot frames whose 13th slot (an int and padding in the C++ Frame) holds a bit pattern that is a NaN with a
    payload when read as a double: it has to travel through the gather and every partition as it is.  synth.pivot
    has one tip and one pivot point whatever the seed; the frames are moved by an offset of the seed's, which moves the
    pivot point with them, so that planted sets of different seeds are different models"""
    d = synth.pivot(n, outlier_frac, seed=seed)[0]
    d[:, 9:12] += np.random.default_rng(seed).uniform(-500.0, 500.0, 3)
    d[:, 12] = (0x7FF8000000000000 + np.arange(n, dtype=np.uint64)).view(np.float64)
    return d


def _pivot_clutter(n, seed):
    """frames off every model, yet near one: the translations of a pivot set moved by up to 3 units per axis (three
    times the threshold).  Among a thousand of them a search finds a loose set of a few dozen that agree, among a few
    dozen it finds none: on the large groups the round after the planted models is accepted, so that max_models is
    reached, and on the small ones it is rejected"""
    d = _pivot(n, 0.0, seed)
    d[:, 9:12] += np.random.default_rng(seed + 1).uniform(-3.0, 3.0, (n, 3))
    return d


# name -> (model, dim, delta, ls_type, planted(n, seed) -> inliers of one model, clutter(n, seed), max_iterations)
MODELS = {
    "plane": (L.PLANE, 3, 0.5, L.LS_ALGEBRAIC,
              lambda n, s: synth.plane(n, 0.0, seed=s, sigma=0.1)[0], lambda n, s: synth.plane(n, 1.0, seed=s)[0], 4096),
    "sphere_geo": (L.SPHERE, 3, 0.5, L.LS_GEOMETRIC,
                   lambda n, s: synth.sphere(n, 0.0, seed=s, sigma=0.1)[0],
                   lambda n, s: synth.sphere(n, 1.0, seed=s)[0], 4096),
    "dense6": (L.DENSE, 6, 0.1, L.LS_ALGEBRAIC,
               lambda n, s: synth.dense(n, 6, outlier_frac=0.0, seed=s, noise=0.01)[0], _dense_clutter, 20000),
    "absor": (L.ABSOR, 3, 2.0, 0,
              lambda n, s: synth.absolute_orientation(n, 0.0, seed=s)[0],
              lambda n, s: synth.absolute_orientation(n, 1.0, seed=s)[0], 4096),
    "pivot": (L.PIVOT, 3, 1.0, 0, lambda n, s: _pivot(n, 0.0, s), _pivot_clutter, 4096),
}
WIDTH = {"plane": 3, "sphere_geo": 3, "dense6": 7, "absor": 6, "pivot": 13}


def scene(name, n, planted_models=3, salt=0, share=(3, 10)):
    """planted models of share[0] / share[1] of the records each plus clutter, shuffled with a fixed permutation (the
    scenes of test_gpu_ransac_grouped.py, rebuilt here)"""
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
    import torch
    torch.cuda.init()  # torch carries its own HIP runtime, which has to come up before the library's
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


def interleave(name, sizes, extra_labels=(), salt=0):
    """group g = scene(name, sizes[g]); three clutter records for every label of extra_labels (labels of no group); all
    of it shuffled by one fixed permutation, so that the groups are interleaved -> (records, int32 labels)"""
    recs = [scene(name, n, salt=salt + g) for g, n in enumerate(sizes)]
    labels = [np.full(n, g, dtype=np.int64) for g, n in enumerate(sizes)]
    for q, lab in enumerate(extra_labels):
        recs.append(MODELS[name][5](3, 0x77000 + q))
        labels.append(np.full(3, lab, dtype=np.int64))
    recs, labels = np.vstack(recs), np.concatenate(labels).astype(np.int32)
    perm = np.random.default_rng(777 + salt).permutation(len(labels))
    return np.ascontiguousarray(recs[perm]), np.ascontiguousarray(labels[perm])


def yardstick(ctx, data, labels, n_groups, seeds, max_models=MAX_MODELS, min_votes=MIN_VOTES):
    """the existing path: stable gather by label on the host + ransac_many_sequential, the labels permuted back to
    upload order -- the context's model and options as they are"""
    idx = np.flatnonzero((labels >= 0) & (labels < n_groups))
    order = idx[np.argsort(labels[idx], kind="stable")]
    offs = np.zeros(n_groups + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(np.bincount(labels[idx], minlength=n_groups))
    w = ctx.ransac_many_sequential((np.ascontiguousarray(data[order]), offs), P, max_models, seeds=seeds,
                                   min_votes=min_votes)
    lab = np.full(len(labels), -1, dtype=np.int32)
    lab[order] = w["labels"]
    w["labels"] = lab
    return w


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(res, w, keys=KEYS + ("labels",)):
    for key in keys:
        a, b = np.asarray(res[key]), np.asarray(w[key])
        assert a.dtype == b.dtype and a.shape == b.shape, (key, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(_bits(a), _bits(b)), (key, a, b)


def _ran(w):
    """rounds that ran, per group"""
    return np.sum(w["status"] != L.ERR_STATE, axis=1)


_EDGE = {}


def edge_sizes(k):
    return [0, k - 1, k, 40, TILE, TILE + 1, CHUNK, CHUNK + 1, 3 * CHUNK + 123]


def edge_case(ctx, name):
    """the edge-size call of one model and its yardstick, computed once and left unchanged:
    (data, labels, n_groups, seeds, sizes, yardstick)"""
    if name not in _EDGE:
        _setup(ctx, name)
        sizes = edge_sizes(ctx.K)
        n_groups = len(sizes)
        data, labels = interleave(name, sizes, extra_labels=(-1, n_groups, INT32_MIN, n_groups + 5))
        seeds = (11 + 3 * np.arange(n_groups * MAX_MODELS, dtype=np.uint64)).reshape(n_groups, MAX_MODELS)
        w = yardstick(ctx, data, labels, n_groups, seeds)
        for a in (data, labels, seeds):
            a.setflags(write=False)
        _EDGE[name] = (data, labels, n_groups, seeds, sizes, w)
    return _EDGE[name]


def _assert_edge_not_vacuous(w, sizes, k):
    """on the yardstick: some group accepts >= 2 rounds (among them one of several parts, so the partition and the
    labels of later rounds are in play), some group's last round is rejected, and some group stops because fewer than k
    records remain or max_models is reached"""
    nm, ran = w["n_models"], _ran(w)
    print("yardstick n_models", nm, "ran", ran, "votes", w["best_votes"].tolist())
    assert nm.max() >= 2 and nm[-1] >= 2, nm
    assert np.any(ran > nm), (ran, nm)  # a round ran and was not accepted
    left = np.array(sizes) - np.where(np.arange(MAX_MODELS)[None, :] < nm[:, None], w["best_votes"], 0).sum(axis=1)
    assert np.any((nm == MAX_MODELS) | ((nm > 0) & (ran == nm) & (left < k))), (nm, ran, left)
    assert np.any(w["labels"] >= 1)


# ---- group sizes around the partition's tiles and chunks, labels of no group ----------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_edge_sizes(ctx, name):
    try:
        data, labels, n_groups, seeds, sizes, w = edge_case(ctx, name)
        k = _setup(ctx, name).K
        _assert_edge_not_vacuous(w, sizes, k)
        if name == "pivot":  # the payloads are there
            assert np.all(np.isnan(data[:, 12])) and len(np.unique(data[:, 12].view(np.uint64))) > 1000
        ctx.upload(data)
        res = ctx.ransac_grouped_sequential(labels, n_groups, P, MAX_MODELS, seeds=seeds, min_votes=MIN_VOTES)
        print(name, "n_models", res["n_models"], "nfev", res["lm_nfev"].tolist())
        assert [int(res["offsets"][g + 1] - res["offsets"][g]) for g in range(n_groups)] == sizes
        same(res, w)
        # 0 and k - 1 records: no round
        assert not np.any(res["n_models"][:2]) and np.all(res["status"][:2] == L.ERR_STATE)
        outside = (labels < 0) | (labels >= n_groups)
        assert outside.sum() == 12 and np.all(res["labels"][outside] == -1)
        assert np.all(res["labels"][labels == 1] == -1) and (labels == 1).sum() == k - 1
        for g in range(n_groups):  # the labels are the claims
            lab = res["labels"][labels == g]
            assert len(lab) == sizes[g] and (len(lab) == 0 or (lab.min() >= -1 and lab.max() < res["n_models"][g]))
            for r in range(res["n_models"][g]):
                assert np.sum(lab == r) == res["best_votes"][g][r], (g, r)
    finally:
        _reset(ctx)


# ---- many small groups: a key wider than one radix digit, an active set that shrinks --------------------------------
def _small_groups(n_groups=2000):
    """2000 plane groups of 24 .. 60 records: group g holds g % 4 planes of 3/10 of its records each (cut from 64
    planes, so that the scene takes a few synth calls) and clutter, so that a quarter of the groups stops after every
    round; the groups are interleaved by one fixed permutation"""
    pool = [synth.plane(4000, 0.0, seed=0x61000 + q, sigma=0.1)[0] for q in range(64)]
    clutter = synth.plane(100000, 1.0, seed=0x61999)[0]
    sizes = [24 + (g * 7) % 37 for g in range(n_groups)]
    recs, labels, used, c0 = [], [], [0] * 64, 0
    for g, n in enumerate(sizes):
        m = (3 * n) // 10
        for j in range(g % 4):
            q = (3 * g + j) % 64
            recs.append(pool[q][used[q]:used[q] + m])
            used[q] += m
        rest = n - (g % 4) * m
        recs.append(clutter[c0:c0 + rest])
        c0 += rest
        labels.append(np.full(n, g, dtype=np.int32))
    assert max(used) <= 4000 and c0 + 6 <= len(clutter)
    recs.append(clutter[c0:c0 + 6])
    labels.append(np.array([n_groups, -7, n_groups, -7, INT32_MIN, n_groups + 1], dtype=np.int32))
    recs, labels = np.vstack(recs), np.concatenate(labels)
    perm = np.random.default_rng(4242).permutation(len(labels))
    return np.ascontiguousarray(recs[perm]), np.ascontiguousarray(labels[perm]), sizes


def test_many_small_groups(ctx):
    try:
        _setup(ctx, "plane")
        data, labels, sizes = _small_groups()
        n_groups = len(sizes)
        assert min(sizes) == 24 and max(sizes) == 60
        seeds = 1 + np.arange(n_groups * 3, dtype=np.uint64).reshape(n_groups, 3)  # the default seeds
        w = yardstick(ctx, data, labels, n_groups, seeds, max_models=3, min_votes=6)
        per_round = np.sum(w["status"] != L.ERR_STATE, axis=0)
        print("groups per round", per_round, "n_models histogram", np.bincount(w["n_models"], minlength=4))
        # the active set shrinks from round to round, and every number of models occurs
        assert per_round[0] == n_groups and per_round[0] > per_round[1] > per_round[2] > 0, per_round
        assert np.all(np.bincount(w["n_models"], minlength=4) > 0)
        ctx.upload(data)
        res = ctx.ransac_grouped_sequential(labels, n_groups, P, 3, min_votes=6)
        same(res, w)
    finally:
        _reset(ctx)


def test_one_group_holds_every_record(ctx):
    try:
        _setup(ctx, "plane")
        data = scene("plane", 5000, salt=60)
        labels = np.zeros(5000, dtype=np.int32)
        seeds = np.array([[5, 6, 7, 8]], dtype=np.uint64)
        w = yardstick(ctx, data, labels, 1, seeds)
        assert w["n_models"][0] >= 2 and np.array_equal(w["offsets"], [0, 5000])
        ctx.upload(data)
        res = ctx.ransac_grouped_sequential(labels, 1, P, MAX_MODELS, seeds=seeds, min_votes=MIN_VOTES)
        same(res, w)
        # the gather of one group is the upload itself: the call equals the plain many-problem call on the records
        plain = ctx.ransac_many_sequential([data], P, MAX_MODELS, seeds=seeds, min_votes=MIN_VOTES)
        same(res, plain)
        # int64 labels
        again = ctx.ransac_grouped_sequential(labels.astype(np.int64), 1, P, MAX_MODELS, seeds=seeds,
                                              min_votes=MIN_VOTES)
        same(again, w)
    finally:
        _reset(ctx)


def test_every_record_ungrouped(ctx):
    try:
        _setup(ctx, "plane")
        data = scene("plane", 600, salt=61)
        labels = np.where(np.arange(600) % 3 == 0, -1, np.where(np.arange(600) % 3 == 1, 3, INT32_MIN)).astype(np.int32)
        w = yardstick(ctx, data, labels, 3, None, max_models=2)
        assert not np.any(w["offsets"]) and not np.any(w["n_models"]) and np.all(w["status"] == L.ERR_STATE)
        ctx.upload(data)
        res = ctx.ransac_grouped_sequential(labels, 3, P, 2, min_votes=MIN_VOTES)
        same(res, w)
        assert len(res["labels"]) == 600 and np.all(res["labels"] == -1)
        assert not np.any(res["params"]) and not np.any(res["best_votes"]) and not np.any(res["evaluated"])
    finally:
        _reset(ctx)


# ---- device form: attached strided tensor, group labels and round labels on the device ------------------------------
@pytest.mark.parametrize("name", ["plane", "pivot"])
def test_attached_strided_tensor_device_labels(ctx, name):
    import torch
    data, labels, n_groups, seeds, sizes, w = edge_case(ctx, name)
    N, W = data.shape
    stride = {"plane": 5, "pivot": 16}[name]
    assert stride > W and w["n_models"].max() >= 2 and np.any(w["labels"] >= 1)
    try:
        _setup(ctx, name).upload(data)
        host = ctx.ransac_grouped_sequential(labels, n_groups, P, MAX_MODELS, seeds=seeds, min_votes=MIN_VOTES)
        t = torch.full((N, stride), float("nan"), dtype=torch.float64, device="cuda:0")
        t[:, :W] = torch.from_numpy(np.array(data))
        g = torch.from_numpy(np.array(labels)).to("cuda:0")
        out = torch.full((N,), 0x7EEE, dtype=torch.int32, device="cuda:0")  # no fill precedes the scatter
        before, g_before = t.clone(), g.clone()
        torch.cuda.synchronize()
        ctx.attach(t.data_ptr(), N, stride * 8, keepalive=t)
        dev = ctx.ransac_grouped_sequential(g, n_groups, P, MAX_MODELS, seeds=seeds, min_votes=MIN_VOTES,
                                            labels_out=out)
        ctx.synchronize()
        assert dev["labels"] is out
        dev = dict(dev, labels=out.cpu().numpy())
        same(dev, host)
        same(dev, w)
        # the records, padding included, and the group labels are only read (compared as bits: NaN padding, payloads)
        assert torch.equal(t.view(torch.int64), before.view(torch.int64)) and torch.equal(g, g_before)
        none = ctx.ransac_grouped_sequential(g, n_groups, P, MAX_MODELS, seeds=seeds, min_votes=MIN_VOTES)
        assert none["labels"] is None
        same(none, w, KEYS)
        out.fill_(0x7EEE)
        off = ctx.ransac_grouped_sequential(g, n_groups, P, MAX_MODELS, seeds=seeds, min_votes=MIN_VOTES,
                                            want_labels=False, labels_out=out)
        ctx.synchronize()
        assert off["labels"] is None and bool(torch.all(out == 0x7EEE))
        same(off, w, KEYS)
    finally:
        _reset(ctx)
        ctx.upload(np.zeros((4, W)))  # let go of the tensor


# ---- independence: label numbering and round cuts -------------------------------------------------------------------
def test_label_numbering_and_round_cap(ctx):
    try:
        data, labels, n_groups, seeds, sizes, w = edge_case(ctx, "plane")
        assert len(set(w["n_models"].tolist())) >= 3  # groups that differ, so that a mix-up would show
        _setup(ctx, "plane").upload(data)
        renum = np.random.default_rng(99).permutation(n_groups)  # group g is called renum[g]
        assert np.any(renum != np.arange(n_groups))
        inside = (labels >= 0) & (labels < n_groups)
        labels2 = labels.copy()
        labels2[inside] = renum[labels[inside]]
        seeds2 = np.zeros_like(seeds)
        seeds2[renum] = seeds
        res = ctx.ransac_grouped_sequential(labels2, n_groups, P, MAX_MODELS, seeds=seeds2, min_votes=MIN_VOTES)
        for key in KEYS[:-1]:
            a, b = np.asarray(res[key])[renum], np.asarray(w[key])
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), key
        assert np.array_equal(np.diff(res["offsets"].astype(np.int64))[renum], sizes)
        same(res, w, ("labels",))
        # the rounds' jobs cut into pieces of 512 hypotheses
        ctx.set_option("many_round_hypotheses", 512)
        cut = ctx.ransac_grouped_sequential(labels, n_groups, P, MAX_MODELS, seeds=seeds, min_votes=MIN_VOTES)
        same(cut, w)
    finally:
        _reset(ctx)


# ---- no labels wanted -----------------------------------------------------------------------------------------------
def test_no_labels_wanted(ctx):
    try:
        data, labels, n_groups, seeds, sizes, w = edge_case(ctx, "plane")
        assert w["n_models"].max() >= 2
        _setup(ctx, "plane").upload(data)
        res = ctx.ransac_grouped_sequential(labels, n_groups, P, MAX_MODELS, seeds=seeds, min_votes=MIN_VOTES,
                                            want_labels=False)
        assert res["labels"] is None
        same(res, w, KEYS)
    finally:
        _reset(ctx)


# ---- the context's own state ----------------------------------------------------------------------------------------
def test_context_state_untouched(ctx):
    try:
        data, labels, n_groups, seeds, sizes, w = edge_case(ctx, "plane")
        assert w["n_models"].max() >= 2  # partitions ran in between
        _setup(ctx, "plane").upload(data)
        before = ctx.ransac(P, seed=3)
        assert before["status"] == L.OK
        ctx.hypotheses_sample(5, 0, 64)
        ctx.scan()
        hyp = ctx.hypotheses()
        assert np.any(hyp[1]) and np.any(hyp[2])
        _, count = ctx.mask(before["params"], want_mask=False)  # the context's mask: the consensus of that model
        fit = ctx.ls_fit(use_mask=True)
        assert count == before["info"].best_votes and len(fit[0]) > 0
        ctx.ransac_grouped_sequential(labels, n_groups, P, MAX_MODELS, seeds=seeds, min_votes=MIN_VOTES)
        assert ctx._lib.lsqr_count(ctx._h) == len(data)
        for a, b in zip(hyp, ctx.hypotheses()):
            assert a.shape == b.shape and a.tobytes() == b.tobytes()
        again = ctx.ls_fit(use_mask=True)  # the same mask: the same fit, bit for bit
        assert again[0].tobytes() == fit[0].tobytes() and again[1].cost == fit[1].cost
        after = ctx.ransac(P, seed=3)
        assert after["status"] == before["status"] == L.OK
        assert np.array_equal(after["consensus"], before["consensus"])
        assert np.array_equal(after["params"].view(np.uint64), before["params"].view(np.uint64))
        for key in ("fraction", "iterations", "best_index", "best_votes", "n_params"):
            assert getattr(after["info"], key) == getattr(before["info"], key), key
    finally:
        _reset(ctx)


# ---- argument errors and refused models write nothing ---------------------------------------------------------------
def _raw(ctx, groups, n_groups, p, n_records, max_models=3, drop=(), on_device=0):
    """the C call with every output pre-filled with a sentinel -> (status, outputs untouched?, n_models).  on_device:
    the group labels and the round labels are device tensors; the other arguments are the host's either way"""
    n = max(int(min(n_groups, 8)), 1)
    rows = n * min(max(max_models, 1), 8)  # (a max_models beyond that is refused before anything is read)
    seeds = np.arange(1, rows + 1, dtype=np.uint64)
    params = np.full((rows, 64), 42.0)
    offs = np.full(n + 1, 42, dtype=np.uint64)
    infos = (L.RansacInfo * rows)()
    C.memset(infos, 0x5A, C.sizeof(infos))
    status = np.full(rows, 42, dtype=np.int32)
    n_models = np.full(n, 42, dtype=np.uintp)
    if on_device:
        import torch
        t_groups = torch.from_numpy(np.ascontiguousarray(groups, dtype=np.int32)).to("cuda:0")
        t_lab = torch.full((max(n_records, 1),), 42, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        p_groups, p_lab = C.c_void_p(t_groups.data_ptr()), C.c_void_p(t_lab.data_ptr())
    else:
        lab = np.full(max(n_records, 1), 42, dtype=np.int32)
        p_groups, p_lab = L.ptr(groups), L.ptr(lab)
    a = dict(groups=p_groups, seeds=L.ptr(seeds), params=L.ptr(params), infos=infos, status=L.ptr(status),
             n_models=L.ptr(n_models))
    for name in drop:
        a[name] = None
    st = ctx._lib.lsqr_ransac_grouped_sequential(ctx._h, a["groups"], n_groups, on_device, p, a["seeds"], max_models, 0,
                                                 a["params"], p_lab, L.ptr(offs), a["infos"], a["status"],
                                                 a["n_models"])
    if on_device:
        ctx.synchronize()
        lab = t_lab.cpu().numpy()
    clean = (np.all(params == 42.0) and np.all(lab == 42) and np.all(offs == 42) and np.all(status == 42)
             and bytes(infos) == b"\x5a" * C.sizeof(infos))
    return st, bool(clean), n_models


def test_errors_write_nothing(ctx):
    try:
        _setup(ctx, "plane")
        data = scene("plane", 200, salt=70)
        labels = (np.arange(200) % 4).astype(np.int32)
        ctx.upload(data)
        untouched = lambda r, st: r[0] == st and r[1] and np.all(r[2] == 42)
        for dev in (0, 1):  # the host form, and the device form (group and round labels in device memory)
            for p in (0.0, 1.0, -0.5, 1.5, float("nan")):
                assert untouched(_raw(ctx, labels, 4, p, 200, on_device=dev), L.ERR_INVALID), (dev, p)
            for missing in ("groups", "seeds", "params", "infos", "status", "n_models"):
                assert untouched(_raw(ctx, labels, 4, P, 200, drop=(missing,), on_device=dev), L.ERR_INVALID), \
                    (dev, missing)
            assert untouched(_raw(ctx, labels, 2 ** 31, P, 200, on_device=dev), L.ERR_INVALID), dev
            assert untouched(_raw(ctx, labels, 4, P, 200, max_models=2 ** 31, on_device=dev), L.ERR_INVALID), dev
            assert untouched(_raw(ctx, labels, 0, P, 200, on_device=dev), L.OK), dev  # no groups: a no-op
            # max_models == 0: n_models zeroed, nothing else written -- also with the other pointers null
            st, clean, n_models = _raw(ctx, labels, 4, P, 200, max_models=0, on_device=dev)
            assert st == L.OK and clean and not np.any(n_models), dev
            st, clean, n_models = _raw(ctx, labels, 4, P, 200, max_models=0, on_device=dev,
                                       drop=("seeds", "params", "infos", "status"))
            assert st == L.OK and clean and not np.any(n_models), dev
            st, clean, n_models = _raw(ctx, labels, 4, P, 200, on_device=dev)  # (the same, complete, run)
            assert st == L.OK and not clean and np.all(n_models <= 3), dev
        with pytest.raises(ValueError):
            ctx.ransac_grouped_sequential(labels[:-1], 4, P, 2)
        with pytest.raises(ValueError):
            ctx.ransac_grouped_sequential(labels.astype(np.float64), 4, P, 2)
        with pytest.raises(ValueError):
            ctx.ransac_grouped_sequential(labels, 4, P, 2, seeds=np.arange(4, dtype=np.uint64))
        with pytest.raises(ValueError):
            ctx.ransac_grouped_sequential(labels, 4, P, -1)
        zero = ctx.ransac_grouped_sequential(labels, 4, P, 0)
        assert zero["status"].shape == (4, 0) and not np.any(zero["n_models"]) and np.all(zero["labels"] == -1)
        # refused models
        for model, ls in ((L.US_SINGLE, L.LS_ANALYTIC), (L.US_POINTER, L.LS_ITERATIVE), (L.PHANTOM, L.LS_ANALYTIC)):
            ctx.set_model(model, 0, 3.0, ls)
            ctx.upload(np.zeros((200, ctx.ND)))
            assert untouched(_raw(ctx, labels, 4, P, 200), L.ERR_INVALID), model
            assert untouched(_raw(ctx, labels, 4, P, 200, on_device=1), L.ERR_INVALID), model
            with pytest.raises(L.LsqrError) as e:
                ctx.ransac_grouped_sequential(labels, 4, P, 2)
            assert e.value.status == L.ERR_INVALID
        # the dense system with 20 unknowns: records of 21 doubles
        ctx.set_model(L.DENSE, 20, 0.1, L.LS_ALGEBRAIC)
        assert ctx.ND == 21
        ctx.upload(np.zeros((200, 21)))
        assert untouched(_raw(ctx, labels, 4, P, 200), L.ERR_INVALID)
        assert untouched(_raw(ctx, labels, 4, P, 200, on_device=1), L.ERR_INVALID)
        # no model, no records
        with Context(0) as fresh:
            assert untouched(_raw(fresh, labels, 4, P, 200), L.ERR_STATE)
            _setup(fresh, "plane")
            assert untouched(_raw(fresh, labels, 4, P, 200), L.ERR_STATE)
    finally:
        _setup(ctx, "plane")
        _reset(ctx)
