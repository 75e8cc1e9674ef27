"""lsqr_ransac_grouped / Context.ransac_grouped: one RANSAC problem per label over the records the context holds on the
device, grouped there (csrc/grouped.h).  The yardstick is the existing path, never the new code: the records are
gathered by label on the host (np.argsort(kind="stable") on the in-range labels), Context.ransac_many / _lm / _dense
runs on that with the same seeds, and status, fraction, iterations, best_index, best_votes, n_params, n_used, params,
cost, lm_info, lm_nfev, offsets and the consensus bytes (permuted back to upload order, 0 for records in no group)
must be equal bit for bit (evaluated alone depends on the batch schedule)."""
import ctypes as C

import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd import synth
from lsqrrecipes_amd.context import Context

pytestmark = pytest.mark.gpu
P = 0.999
INT32_MIN = -2 ** 31
KEYS = ("status", "fraction", "iterations", "best_index", "best_votes", "n_params", "n_used", "params", "cost",
        "lm_info", "lm_nfev", "offsets")
FIT_KEYS = ("lm_info", "lm_nfev", "cost", "reserved")


def _dense_clutter(n, seed):
    g = np.random.Generator(np.random.Philox(seed))
    return np.hstack([g.uniform(-1.0, 1.0, (n, 6)), g.uniform(-20.0, 20.0, (n, 1))])


def _pivot(n, outlier_frac, seed):
    """pivot frames whose 13th slot (an int and padding in the C++ Frame) holds a bit pattern that is a NaN with a
    payload when read as a double: it has to travel through the gather as it is"""
    d = synth.pivot(n, outlier_frac, seed=seed)[0]
    d[:, 12] = (0x7FF8000000000000 + np.arange(n, dtype=np.uint64)).view(np.float64)
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
    "pivot": (L.PIVOT, 3, 1.0, 0, lambda n, s: _pivot(n, 0.0, s), lambda n, s: _pivot(n, 1.0, s), 4096),
}
WIDTH = {"plane": 3, "sphere_geo": 3, "dense6": 7, "absor": 6, "pivot": 13}


def scene(name, n, planted_models=3, salt=0, share=(3, 10)):
    """planted models of share[0] / share[1] of the records each plus clutter, shuffled with a fixed permutation (the
    scenes of test_gpu_ransac_many_sequential.py, rebuilt here)"""
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


def yardstick(ctx, data, labels, n_groups, seeds):
    """the existing path: stable gather by label on the host + ransac_many / _lm / _dense (with every fit field), the
    consensus permuted back to upload order -- the context's model and options as they are"""
    idx = np.flatnonzero((labels >= 0) & (labels < n_groups))
    order = idx[np.argsort(labels[idx], kind="stable")]
    offs = np.zeros(n_groups + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(np.bincount(labels[idx], minlength=n_groups))
    cfg = ctx.cfg
    fn = (ctx._lib.lsqr_ransac_many_dense if cfg.model == L.DENSE else
          ctx._lib.lsqr_ransac_many_lm if cfg.model == L.SPHERE and cfg.ls_type == L.LS_GEOMETRIC else
          ctx._lib.lsqr_ransac_many)
    w = ctx._ransac_many(fn, (np.ascontiguousarray(data[order]), offs), P, seeds, True, extra=FIT_KEYS)
    cons = np.zeros(len(labels), dtype=np.uint8)
    cons[order] = w["consensus"]
    w["consensus"] = cons
    return w


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(res, w, keys=KEYS + ("reserved", "consensus")):
    for key in keys:
        a, b = np.asarray(res[key]), np.asarray(w[key])
        assert a.dtype == b.dtype and a.shape == b.shape, (key, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(_bits(a), _bits(b)), (key, a, b)


_EDGE = {}


def edge_case(ctx, name):
    """the edge-size call of one model and its yardstick, computed once: (data, labels, n_groups, seeds, yardstick)"""
    if name not in _EDGE:
        _setup(ctx, name)
        k = ctx.K
        sizes = [0, k - 1, k, 40, 255, 256, 257, 4096, 4097]
        n_groups = len(sizes)
        data, labels = interleave(name, sizes, extra_labels=(-1, n_groups, INT32_MIN, n_groups + 5))
        seeds = 11 + 3 * np.arange(n_groups, dtype=np.uint64)
        _EDGE[name] = (data, labels, n_groups, seeds, sizes, yardstick(ctx, data, labels, n_groups, seeds))
    return _EDGE[name]


# ---- group sizes around the kernels' tiles, labels of no group ------------------------------------------------------
@pytest.mark.parametrize("name", list(MODELS))
def test_edge_sizes(ctx, name):
    try:
        data, labels, n_groups, seeds, sizes, w = edge_case(ctx, name)
        _setup(ctx, name).upload(data)
        res = ctx.ransac_grouped(labels, n_groups, P, seeds=seeds)
        print(name, "status", res["status"], "votes", res["best_votes"], "/", w["best_votes"], "nfev", res["lm_nfev"])
        assert [int(res["offsets"][g + 1] - res["offsets"][g]) for g in range(n_groups)] == sizes
        same(res, w)
        k = ctx.K
        assert res["status"][0] == res["status"][1] == L.ERR_INVALID  # 0 and k - 1 records
        assert np.all(res["status"][-2:] == L.OK), res["status"]  # the large groups' planted models are found
        outside = (labels < 0) | (labels >= n_groups)
        assert outside.sum() == 12 and not np.any(res["consensus"][outside])
        assert not np.any(res["consensus"][labels == 1]) and (labels == 1).sum() == k - 1
        assert res["consensus"].sum() == res["best_votes"][res["n_used"] > 0].sum() > 0
    finally:
        _reset(ctx)


# ---- a key wider than one radix digit -------------------------------------------------------------------------------
def test_many_small_groups(ctx):
    try:
        _setup(ctx, "plane")
        sizes = [8 + (g * 7) % 5 for g in range(300)]  # 8 .. 12
        data, labels = interleave("plane", sizes, extra_labels=(300, -7), salt=50)
        ctx.upload(data)
        res = ctx.ransac_grouped(labels, 300, P)
        w = yardstick(ctx, data, labels, 300, 1 + np.arange(300, dtype=np.uint64))  # the default seeds
        same(res, w)
        assert min(sizes) == 8 and max(sizes) == 12 and np.all(res["status"] != L.ERR_INVALID)
    finally:
        _reset(ctx)


def test_one_group_holds_every_record(ctx):
    try:
        _setup(ctx, "plane")
        data = scene("plane", 1000, salt=60)
        labels = np.zeros(1000, dtype=np.int32)
        ctx.upload(data)
        res = ctx.ransac_grouped(labels, 1, P, seeds=np.array([5], dtype=np.uint64))
        w = yardstick(ctx, data, labels, 1, np.array([5], dtype=np.uint64))
        same(res, w)
        assert res["status"][0] == L.OK and list(res["offsets"]) == [0, 1000]
        # int64 labels, and no consensus asked for
        again = ctx.ransac_grouped(labels.astype(np.int64), 1, P, seeds=np.array([5], dtype=np.uint64),
                                   want_consensus=False)
        assert again["consensus"] is None
        same(again, w, KEYS)
    finally:
        _reset(ctx)


def test_every_record_ungrouped(ctx):
    try:
        _setup(ctx, "plane")
        data = scene("plane", 600, salt=61)
        labels = np.where(np.arange(600) % 3 == 0, -1, np.where(np.arange(600) % 3 == 1, 3, INT32_MIN)).astype(np.int32)
        ctx.upload(data)
        res = ctx.ransac_grouped(labels, 3, P)
        assert np.all(res["status"] == L.ERR_INVALID) and not np.any(res["consensus"]) and len(res["consensus"]) == 600
        assert not np.any(res["offsets"]) and not np.any(res["params"]) and not np.any(res["best_votes"])
        same(res, yardstick(ctx, data, labels, 3, 1 + np.arange(3, dtype=np.uint64)))
    finally:
        _reset(ctx)


# ---- device form: attached strided tensor, labels and consensus on the device ---------------------------------------
@pytest.mark.parametrize("name", ["plane", "pivot"])
def test_attached_strided_tensor_device_labels(ctx, name):
    import torch
    data, labels, n_groups, seeds, sizes, w = edge_case(ctx, name)
    N, W = data.shape
    try:
        _setup(ctx, name).upload(data)
        host = ctx.ransac_grouped(labels, n_groups, P, seeds=seeds)
        t = torch.full((N, W + 1), float("nan"), dtype=torch.float64, device="cuda:0")
        t[:, :W] = torch.from_numpy(np.array(data))
        g = torch.from_numpy(labels).to("cuda:0")
        out = torch.full((N,), 0xEE, dtype=torch.uint8, device="cuda:0")
        before, g_before = t.clone(), g.clone()
        torch.cuda.synchronize()
        ctx.attach(t.data_ptr(), N, (W + 1) * 8, keepalive=t)
        dev = ctx.ransac_grouped(g, n_groups, P, seeds=seeds, consensus_out=out)
        ctx.synchronize()
        assert dev["consensus"] is out
        dev = dict(dev, consensus=out.cpu().numpy())
        same(dev, host)
        same(dev, w)
        # the records and the labels are only read (compared as bits: the padding is NaN)
        assert torch.equal(t.view(torch.int64), before.view(torch.int64)) and torch.equal(g, g_before)
        none = ctx.ransac_grouped(g, n_groups, P, seeds=seeds)  # the device form without a consensus tensor
        assert none["consensus"] is None
        same(none, w, KEYS)
    finally:
        _reset(ctx)
        ctx.upload(np.zeros((4, W)))  # let go of the tensor


# ---- independence: label numbering and round cuts -------------------------------------------------------------------
def test_label_numbering_and_round_cap(ctx):
    try:
        data, labels, n_groups, seeds, sizes, w = edge_case(ctx, "plane")
        _setup(ctx, "plane").upload(data)
        renum = np.random.default_rng(99).permutation(n_groups)  # group g is called renum[g]
        inside = (labels >= 0) & (labels < n_groups)
        labels2 = labels.copy()
        labels2[inside] = renum[labels[inside]]
        seeds2 = np.zeros_like(seeds)
        seeds2[renum] = seeds
        ctx.set_option("many_round_hypotheses", 1024)
        res = ctx.ransac_grouped(labels2, n_groups, P, seeds=seeds2)
        for key in KEYS[:-1] + ("reserved",):
            assert np.array_equal(_bits(res[key][renum]), _bits(w[key])), key
        assert np.array_equal(np.diff(res["offsets"].astype(np.int64))[renum], sizes)
        assert np.array_equal(res["consensus"], w["consensus"])
    finally:
        _reset(ctx)


# ---- the context's own state ----------------------------------------------------------------------------------------
def test_context_state_untouched(ctx):
    try:
        data, labels, n_groups, seeds, sizes, w = edge_case(ctx, "plane")
        _setup(ctx, "plane").upload(data)
        ctx.ransac_grouped(labels, n_groups, P, seeds=seeds)
        after = ctx.ransac(P, seed=3)
        with Context(0) as fresh:
            _setup(fresh, "plane").upload(data)
            want = fresh.ransac(P, seed=3)
        assert after["status"] == want["status"] == L.OK
        assert np.array_equal(after["consensus"], want["consensus"])
        assert np.array_equal(after["params"].view(np.uint64), want["params"].view(np.uint64))
        for key in ("fraction", "iterations", "best_index", "best_votes", "n_params"):
            assert getattr(after["info"], key) == getattr(want["info"], key), key
        assert ctx._lib.lsqr_count(ctx._h) == len(data)
    finally:
        _reset(ctx)


# ---- argument errors and refused models write nothing ---------------------------------------------------------------
def _raw(ctx, groups, n_groups, p, n_records, drop=(), on_device=0):
    """the C call with every output pre-filled with a sentinel -> (status, outputs untouched?).  on_device: the labels
    and the consensus are device tensors, as the device form takes them; the other arguments are the host's either
    way"""
    n = max(int(min(n_groups, 8)), 1)
    seeds = np.arange(1, n + 1, dtype=np.uint64)
    params = np.full((n, 64), 42.0)
    offs = np.full(n + 1, 42, dtype=np.uint64)
    infos = (L.RansacInfo * n)()
    C.memset(infos, 0x5A, C.sizeof(infos))
    status = np.full(n, 42, dtype=np.int32)
    if on_device:
        import torch
        t_groups = torch.from_numpy(np.ascontiguousarray(groups, dtype=np.int32)).to("cuda:0")
        t_cons = torch.full((max(n_records, 1),), 42, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        p_groups, p_cons = C.c_void_p(t_groups.data_ptr()), C.c_void_p(t_cons.data_ptr())
    else:
        cons = np.full(max(n_records, 1), 42, dtype=np.uint8)
        p_groups, p_cons = L.ptr(groups), L.ptr(cons)
    a = dict(groups=p_groups, seeds=L.ptr(seeds), params=L.ptr(params), infos=infos, status=L.ptr(status))
    for name in drop:
        a[name] = None
    st = ctx._lib.lsqr_ransac_grouped(ctx._h, a["groups"], n_groups, on_device, p, a["seeds"], a["params"],
                                      p_cons, L.ptr(offs), a["infos"], a["status"])
    if on_device:
        ctx.synchronize()
        cons = t_cons.cpu().numpy()
    clean = (np.all(params == 42.0) and np.all(cons == 42) and np.all(offs == 42) and np.all(status == 42)
             and bytes(infos) == b"\x5a" * C.sizeof(infos))
    return st, clean


def test_errors_write_nothing(ctx):
    try:
        _setup(ctx, "plane")
        data = scene("plane", 200, salt=70)
        labels = (np.arange(200) % 4).astype(np.int32)
        ctx.upload(data)
        for dev in (0, 1):  # the host form, and the device form (labels and consensus in device memory)
            for p in (0.0, 1.0, -0.5, 1.5, float("nan")):
                assert _raw(ctx, labels, 4, p, 200, on_device=dev) == (L.ERR_INVALID, True), (dev, p)
            for missing in ("groups", "seeds", "params", "infos", "status"):
                assert _raw(ctx, labels, 4, P, 200, drop=(missing,), on_device=dev) == (L.ERR_INVALID, True), \
                    (dev, missing)
            assert _raw(ctx, labels, 2 ** 31, P, 200, on_device=dev) == (L.ERR_INVALID, True), dev
            assert _raw(ctx, labels, 0, P, 200, on_device=dev) == (L.OK, True), dev  # no groups: a no-op
            assert _raw(ctx, labels, 4, P, 200, on_device=dev) == (L.OK, False), dev  # (the same, complete, run)
        with pytest.raises(ValueError):
            ctx.ransac_grouped(labels[:-1], 4, P)
        with pytest.raises(ValueError):
            ctx.ransac_grouped(labels.astype(np.float64), 4, P)
        with pytest.raises(ValueError):
            ctx.ransac_grouped(labels, 4, P, seeds=np.arange(3, dtype=np.uint64))
        # refused models
        for model, ls in ((L.US_SINGLE, L.LS_ANALYTIC), (L.US_POINTER, L.LS_ITERATIVE), (L.PHANTOM, L.LS_ANALYTIC)):
            ctx.set_model(model, 0, 3.0, ls)
            ctx.upload(np.zeros((200, ctx.ND)))
            assert _raw(ctx, labels, 4, P, 200) == (L.ERR_INVALID, True), model
            assert _raw(ctx, labels, 4, P, 200, on_device=1) == (L.ERR_INVALID, True), model
            with pytest.raises(L.LsqrError) as e:
                ctx.ransac_grouped(labels, 4, P)
            assert e.value.status == L.ERR_INVALID
        # no records, no model
        with Context(0) as fresh:
            assert _raw(fresh, labels, 4, P, 200) == (L.ERR_STATE, True)
            _setup(fresh, "plane")
            assert _raw(fresh, labels, 4, P, 200) == (L.ERR_STATE, True)
    finally:
        _reset(ctx)
