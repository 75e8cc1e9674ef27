"""lsqr_refine_lm (csrc/assign_lm.h) through Context.refine_lm: lsqr_refine's loop for the geometric sphere, the refit
a Levenberg-Marquardt run per model on the device.

Round by round against the host loop on the entry points the library had before (Context.assign, then per model
set_mask(labels == m) + ls_fit(use_mask) on a geometric context): the two differ in the origin of the algebraic start
and the order of the fp64 sums only, so parameters and cost at rtol 1e-9 / atol 1e-8 (the LM tolerance of
tests/test_gpu_ransac_many_lm.py), lm_info in the same class, lm_nfev within 3, n_used equal and -- on scenes where no
record sits within MARGIN of a decision, which is asserted from Context.residuals -- equal labels, counts, rounds and
stop.  A CPU simulation of the scenes (numpy assignment + the oracle's geometric fit) gave: smallest distance of a
residual to delta 1.76e-5 (3-D, n = 70 001, all rounds), 9.2e-4 / 5.4e-5 (its prefixes), 1.4e-3 (2-D), 1.3e-4 (5-D);
smallest gap between a record's two best residuals 4.1e-4.  Agreement of the parameters at the tolerance above moves a
residual by about 2e-6.  The seeds of the 3-D scene serve the 2-D and 5-D scenes as well."""
import ctypes as C

import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd import synth
from lsqrrecipes_amd.context import Context
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu
SMALL, LARGE = 300, 70_001   # below one chunk of the pass (2048 records) / 35 chunks, odd tail
MID = 5000                   # the 2-D and 5-D scenes above one chunk
EDGES = (2047, 2048, 2049, 4097)
DELTA = 0.5
MARGIN = 1e-5                # no record of a scene is this close to a decision
REL = 1e-6                   # the README's fit tolerance
_scenes, _chains = {}, {}


def scene(dim, n):
    """three planted spheres of 30 % each plus clutter, shuffled with a fixed permutation, and the start rows: the
    planted truths with +0.1 on every centre coordinate and +0.2 on the radius; computed once, never changed"""
    if (dim, n) not in _scenes:
        m = (3 * n) // 10
        planted = [synth.sphere(m, 0.0, seed=0x53000 + 7 * j, sigma=0.1, dim=dim) for j in range(3)]
        parts = [p[0] for p in planted] + [synth.sphere(n - 3 * m, 1.0, seed=0x53999, dim=dim)[0]]
        data = np.ascontiguousarray(np.vstack(parts)[np.random.default_rng(12345).permutation(n)])
        rows = np.array([p[1] for p in planted])
        rows[:, :dim] += 0.1
        rows[:, dim] += 0.2
        data.setflags(write=False)
        rows.setflags(write=False)
        _scenes[dim, n] = (data, rows)
    return _scenes[dim, n]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def load(ctx, data, dim=3, ls_type=L.LS_GEOMETRIC):
    ctx.set_model(L.SPHERE, dim, DELTA, ls_type).upload(data)
    return ctx


def counts_of(labels, m):
    return np.array([np.sum(labels == k) for k in range(m)] + [np.sum(labels == -1)], dtype=np.uint64)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def host_round(ctx, rows):
    """one round of the host loop -> the labels of `rows`, the refitted rows, and per model status, n_used, lm_info,
    lm_nfev, cost.  Asserts the scene condition: no record within MARGIN of delta, no record whose two smallest
    agreeing residuals are within MARGIN of each other."""
    labels = ctx.assign(rows)["labels"]
    res = np.array([ctx.residuals(r) for r in rows])
    assert np.min(np.abs(res - DELTA)) > MARGIN, "a record within MARGIN of delta: choose another scene seed"
    two = np.sort(np.where(res < DELTA, res, np.inf), axis=0)[:2]
    both = np.isfinite(two[1])
    assert not both.any() or np.min(two[1][both] - two[0][both]) > MARGIN, "a tie within MARGIN: choose another seed"
    new = np.array(rows, copy=True)
    out = dict(status=[], n_used=[], lm_info=[], lm_nfev=[], cost=[])
    for m in range(len(rows)):
        mask = (labels == m).astype(np.uint8)
        used, fit, info = int(mask.sum()), np.zeros(0), L.FitInfo()
        if used >= ctx.K:
            ctx.set_mask(mask)
            fit, info = ctx.ls_fit(use_mask=True)
        if len(fit):  # (an EMPTY fit keeps the row)
            new[m] = fit
        for key, v in (("status", L.OK if len(fit) else L.EMPTY), ("n_used", used), ("lm_info", info.lm_info),
                       ("lm_nfev", info.lm_nfev), ("cost", info.cost)):
            out[key].append(v)
    return labels, new, {k: np.array(v) for k, v in out.items()}


def host_loop(ctx, key, rows0, max_rounds):
    """lsqr_refine's loop on the host loop's rounds; the rounds of a scene are computed once (key) and shared"""
    chain = _chains.setdefault(key, [])  # chain[r] = host_round(params_r)
    rows, prev, r = np.array(rows0), None, 0
    while True:
        if len(chain) == r:
            chain.append(host_round(ctx, rows))
        labels, new, fits = chain[r]
        if r > 0 and np.array_equal(labels, prev):
            return dict(params=rows, labels=labels, rounds=r, converged=True, fits=chain[r - 1][2])
        if r == max_rounds:
            return dict(params=rows, labels=labels, rounds=r, converged=False, fits=chain[r - 1][2] if r else None)
        rows, prev, r = new, labels, r + 1


def assert_equals_host_loop(got, want, what):
    m = len(want["params"])
    print(what, "rounds", got["rounds"], "converged", got["converged"], "counts", list(got["counts"]), "lm_info",
          list(got["lm_info"]), "lm_nfev", list(got["lm_nfev"]), "host lm_nfev",
          None if want["fits"] is None else list(want["fits"]["lm_nfev"]), "cost", list(got["cost"]))
    assert got["rounds"] == want["rounds"] and got["converged"] == want["converged"], what
    assert np.allclose(got["params"], want["params"], rtol=1e-9, atol=1e-8), (what, got["params"], want["params"])
    assert np.array_equal(got["labels"], want["labels"]), what
    assert np.array_equal(got["counts"], counts_of(want["labels"], m)), what
    f = want["fits"]
    if f is None:  # no refit ran
        assert np.all(got["status"] == L.OK) and not np.any(got["n_used"]) and not np.any(got["lm_info"]), what
        assert not np.any(got["lm_nfev"]) and not np.any(got["cost"]), what
        return
    assert np.array_equal(got["status"], f["status"]) and np.array_equal(got["n_used"], f["n_used"]), what
    ok = lambda info: (info >= 1) & (info <= 4)  # noqa: E731
    assert np.array_equal(ok(got["lm_info"]), ok(f["lm_info"])), (what, got["lm_info"], f["lm_info"])
    assert np.all(np.abs(got["lm_nfev"].astype(np.int64) - f["lm_nfev"]) <= 3), (what, got["lm_nfev"], f["lm_nfev"])
    assert np.allclose(got["cost"], f["cost"], rtol=1e-9, atol=1e-8), (what, got["cost"], f["cost"])
    assert np.all(got["stall"] >= 1) and np.all(got["stall"] <= got["lm_nfev"]), what


# ---- 1, 2, 7: round by round against the host loop ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [SMALL, LARGE])
def test_refine_lm_against_the_host_loop_round_by_round(ctx, n):
    data, rows0 = scene(3, n)
    load(ctx, data)
    for max_rounds in (1, 2, 3):
        want = host_loop(ctx, (3, n), rows0, max_rounds)
        got = ctx.refine_lm(rows0, max_rounds=max_rounds)
        assert_equals_host_loop(got, want, "n=%d max_rounds=%d" % (n, max_rounds))
        assert np.all(got["status"] == L.OK) and np.all((got["lm_info"] >= 1) & (got["lm_info"] <= 4))
    assert got["converged"] and got["rounds"] == (2 if n == SMALL else 3)  # (the simulation's rounds)


@pytest.mark.parametrize("n", EDGES)
def test_refine_lm_at_the_chunk_edges_against_the_host_loop(ctx, n):
    """a last chunk of 2047, 2048, 1 and 1 records, in one, two and three chunks"""
    data, rows0 = scene(3, LARGE)
    load(ctx, data[:n])
    want = host_loop(ctx, (3, LARGE, n), rows0, 1)
    assert_equals_host_loop(ctx.refine_lm(rows0, max_rounds=1), want, "prefix %d" % n)


@pytest.mark.parametrize("dim,n", [(2, SMALL), (2, MID), (5, SMALL), (5, MID)])
def test_refine_lm_in_other_dimensions_against_the_host_loop(ctx, dim, n):
    data, rows0 = scene(dim, n)
    load(ctx, data, dim)
    want = host_loop(ctx, (dim, n), rows0, 1)
    got = ctx.refine_lm(rows0, max_rounds=1)
    assert_equals_host_loop(got, want, "dim=%d n=%d" % (dim, n))
    assert got["rounds"] == 1 and np.all(got["status"] == L.OK)


# ---- 3: invariants -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [SMALL, LARGE])
def test_refine_lm_invariants(ctx, n):
    data, rows0 = scene(3, n)
    load(ctx, data)
    zero = ctx.refine_lm(rows0, max_rounds=0)
    plain = ctx.assign(rows0)
    assert zero["rounds"] == 0 and not zero["converged"] and np.array_equal(bits(zero["params"]), bits(rows0))
    assert np.array_equal(zero["labels"], plain["labels"]) and np.array_equal(zero["counts"], plain["counts"])
    assert np.all(zero["status"] == L.OK) and not np.any(zero["n_used"]) and not np.any(zero["lm_info"])
    for max_rounds in (1, 8):
        a = ctx.refine_lm(rows0, max_rounds=max_rounds)
        again = ctx.assign(a["params"])
        assert np.array_equal(again["labels"], a["labels"]) and np.array_equal(again["counts"], a["counts"])
        assert (max_rounds == 1 and a["rounds"] == 1) or a["converged"]
    # at convergence every model is the geometric fit of its own records
    oc = O.cfg(O.SPHERE, 3, DELTA, O.LS_GEOMETRIC)
    for m in range(3):
        want = O.ls(oc, data, (a["labels"] == m).astype(np.uint8))
        assert len(want) == 4
        assert np.all(np.abs(a["params"][m] - want) <= REL * max(1.0, np.abs(want).max())), (m, a["params"][m], want)
    if n == LARGE:  # some records agree with two spheres: the nearest is not the first everywhere
        masks = np.array([ctx.mask(r)[0] for r in a["params"]])
        first = np.where(masks.any(axis=0), np.argmax(masks != 0, axis=0), -1)
        assert np.sum(first != a["labels"]) >= 1 and np.sum(masks.sum(axis=0) > 1) >= 1


# ---- 4: determinism and independence, bit for bit ----------------------------------------------------------------------
def test_refine_lm_twice_and_among_sixty_four_rows(ctx):
    data, rows0 = scene(3, LARGE)
    load(ctx, data)
    r3 = ctx.refine_lm(rows0, max_rounds=2)
    again = ctx.refine_lm(rows0, max_rounds=2)
    for key in ("params", "labels", "counts", "status", "n_used", "lm_info", "lm_nfev", "cost", "stall"):
        assert np.array_equal(bits(r3[key]), bits(again[key])), key
    far = np.tile(rows0, (22, 1))[:61].copy()
    far[:, :3] += 1e7  # spheres far from every record
    many = np.vstack([far[:20], rows0[:1], far[20:40], rows0[1:], far[40:]])  # the three rows at 20, 41 and 42
    where = {20: 0, 41: 1, 42: 2}
    r64 = ctx.refine_lm(many, max_rounds=2)
    assert r64["rounds"] == r3["rounds"] == 2 and r64["converged"] == r3["converged"]
    want = np.full(LARGE, -1, dtype=np.int32)
    for k, m in where.items():
        want[r3["labels"] == m] = k
    assert np.array_equal(r64["labels"], want)
    for k in range(64):
        if k in where:
            m = where[k]
            assert r64["status"][k] == L.OK and r64["n_used"][k] == r3["n_used"][m]
            assert np.array_equal(bits(r64["params"][k]), bits(r3["params"][m])), k
            assert r64["lm_nfev"][k] == r3["lm_nfev"][m] and r64["lm_info"][k] == r3["lm_info"][m]
            assert np.array_equal(bits(r64["cost"][k:k + 1]), bits(r3["cost"][m:m + 1])), k
        else:
            assert r64["status"][k] == L.EMPTY and r64["n_used"][k] == 0 and r64["lm_info"][k] == 0
            assert np.array_equal(bits(r64["params"][k]), bits(many[k]))
    with pytest.raises(L.LsqrError) as e:
        ctx.refine_lm(np.vstack([many, rows0[:1]]))
    assert e.value.status == L.ERR_INVALID


# ---- 5: a refit that gives no result keeps the row it had before the round -----------------------------------------------
def test_refine_lm_keeps_the_row_when_the_fit_fails(ctx):
    """four records on a circle, far from the scene, and a row through them: four coplanar records give the algebraic
    start no result (the reference's fit of that set is empty, checked with the oracle), so the row must come back with
    the bits it went in with -- not the round's intermediate -- and EMPTY; the other rows are refitted as without it"""
    scene_data, rows0 = scene(3, SMALL)
    c = np.array([5e4, 5e4, 5e4])
    four = c + np.array([[10.0, 10.0, 0.0], [10.0, -10.0, 0.0], [-10.0, 10.0, 0.0], [-10.0, -10.0, 0.0]])
    data = np.vstack([scene_data[:150], four[:2], scene_data[150:], four[2:]])
    row = np.concatenate([c, [np.sqrt(200.0)]])
    own = np.zeros(len(data), dtype=np.uint8)
    own[[150, 151, len(data) - 2, len(data) - 1]] = 1
    assert len(O.ls(O.cfg(O.SPHERE, 3, DELTA, O.LS_GEOMETRIC), data, own)) == 0
    load(ctx, data)
    rows = np.vstack([rows0[:1], row[None], rows0[1:]])
    labels = ctx.assign(rows)["labels"]
    assert np.array_equal(labels == 1, own != 0)
    base = ctx.refine_lm(rows0, max_rounds=2)
    got = ctx.refine_lm(rows, max_rounds=2)
    assert got["rounds"] == base["rounds"] == 2 and got["converged"] == base["converged"]
    assert got["status"][1] == L.EMPTY and got["n_used"][1] == 4 and got["lm_info"][1] == 0 and got["lm_nfev"][1] == 0
    assert np.array_equal(bits(got["params"][1]), bits(row))
    keep = [0, 2, 3]
    assert np.all(got["status"][keep] == L.OK) and np.array_equal(bits(got["params"][keep]), bits(base["params"]))
    assert np.array_equal(got["n_used"][keep], base["n_used"]) and np.array_equal(got["lm_nfev"][keep], base["lm_nfev"])
    assert not np.array_equal(bits(got["params"][keep]), bits(rows0))  # (they were refitted)
    assert np.array_equal(ctx.assign(got["params"])["labels"], got["labels"])


# ---- 6: device labels and a strided attach -----------------------------------------------------------------------------
class DeviceArray:
    """a device allocation of the HIP runtime the library itself runs on, with the handful of tensor attributes
    Context looks at (data_ptr, is_cuda, dtype, is_contiguous, numel): the device-pointer forms need no more"""
    _hip = None

    @classmethod
    def hip(cls):
        if cls._hip is None:
            L.load()
            path = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln][0]
            cls._hip = C.CDLL(path)  # (already loaded: the same runtime, the same device context)
        return cls._hip

    def __init__(self, host):
        self.host = np.ascontiguousarray(host)
        self.dtype, self.is_cuda = str(self.host.dtype), True
        p = C.c_void_p()
        assert self.hip().hipMalloc(C.byref(p), C.c_size_t(self.host.nbytes)) == 0
        self.ptr = p
        self.put(self.host)

    def put(self, host):
        assert self.hip().hipMemcpy(self.ptr, C.c_void_p(host.ctypes.data), C.c_size_t(host.nbytes), 1) == 0

    def get(self):
        out = np.empty_like(self.host)
        assert self.hip().hipMemcpy(C.c_void_p(out.ctypes.data), self.ptr, C.c_size_t(out.nbytes), 2) == 0
        return out

    def free(self):
        if self.ptr:
            self.hip().hipFree(self.ptr)
            self.ptr = None

    def data_ptr(self):
        return self.ptr.value

    def is_contiguous(self):
        return True

    def numel(self):
        return self.host.size


def test_refine_lm_device_labels_and_strided_attach(ctx):
    data, rows0 = scene(3, LARGE)
    load(ctx, data)
    host = ctx.refine_lm(rows0, max_rounds=2)
    lab = DeviceArray(np.full(LARGE, -9, dtype=np.int32))
    wide = np.full((LARGE, 4), -7.25)
    wide[:, :3] = data
    t = DeviceArray(wide)
    try:
        dev = ctx.refine_lm(rows0, max_rounds=2, labels_out=lab)
        assert dev["labels"] is lab and np.array_equal(lab.get(), host["labels"])
        assert np.array_equal(bits(dev["params"]), bits(host["params"]))
        assert np.array_equal(dev["counts"], host["counts"]) and dev["rounds"] == host["rounds"]
        # the records at a stride of four doubles, attached: the same bits, the buffer untouched
        ctx.attach(t.data_ptr(), LARGE, 32, keepalive=t)
        at = ctx.refine_lm(rows0, max_rounds=2)
        ctx.synchronize()
        assert np.array_equal(bits(at["params"]), bits(host["params"]))
        assert np.array_equal(at["labels"], host["labels"]) and at["rounds"] == host["rounds"]
        assert np.array_equal(at["lm_nfev"], host["lm_nfev"]) and np.array_equal(bits(at["cost"]), bits(host["cost"]))
        assert np.array_equal(bits(t.get()), bits(wide))
    finally:
        ctx.upload(np.zeros((4, 3)))  # let go of the attached buffer
        ctx._keep = None
        lab.free()
        t.free()


# ---- 8: the gate and the argument errors write nothing -----------------------------------------------------------------
def test_refine_lm_gate_and_argument_errors_write_nothing(ctx):
    lib = L.load()
    data, rows0 = scene(3, SMALL)
    load(ctx, data)
    params = np.ascontiguousarray(rows0).copy()
    keep = params.copy()
    labels = np.full(SMALL, 42, dtype=np.int32)
    counts = np.full(4, 42, dtype=np.uint64)
    status = np.full(3, 42, dtype=np.int32)
    fits = (L.FitInfo * 3)()
    C.memset(fits, 0x5A, C.sizeof(fits))
    rounds, conv = C.c_size_t(42), C.c_int(42)

    def refine(h=None, params_=params, n=3, fits_=fits, status_=status, rounds_=C.byref(rounds), conv_=C.byref(conv)):
        return lib.lsqr_refine_lm(ctx._h if h is None else h, L.ptr(params_), n, 4, 0, L.ptr(labels), L.ptr(counts),
                                  fits_, L.ptr(status_), rounds_, conv_)

    def untouched():
        return (np.array_equal(bits(params), bits(keep)) and np.all(labels == 42) and np.all(counts == 42)
                and np.all(status == 42) and bytes(fits) == b"\x5a" * C.sizeof(fits) and rounds.value == 42
                and conv.value == 42)

    assert refine(params_=None) == L.ERR_INVALID and untouched()
    assert refine(fits_=None) == L.ERR_INVALID and untouched()
    assert refine(status_=None) == L.ERR_INVALID and untouched()
    assert refine(rounds_=None) == L.ERR_INVALID and untouched()
    assert refine(conv_=None) == L.ERR_INVALID and untouched()
    assert refine(n=65) == L.ERR_INVALID and untouched()
    assert refine(n=0) == L.OK and untouched()
    # the gate: the geometric sphere alone; the message names the call that takes the others
    wide = np.zeros((3, 8))
    for model, dim, ls in ((L.SPHERE, 3, L.LS_ALGEBRAIC), (L.PLANE, 3, L.LS_ALGEBRAIC), (L.ABSOR, 3, 0)):
        ctx.set_model(model, dim, DELTA, ls)
        for n in (3, 0, 65):
            assert refine(params_=wide, n=n) == L.ERR_INVALID and untouched() and not wide.any(), (model, n)
        assert "lsqr_refine" in lib.lsqr_last_error(ctx._h).decode().replace("lsqr_refine_lm", "")
    with Context(0) as empty:  # no model / no records
        assert refine(h=empty._h) == L.ERR_STATE and untouched()
        empty.set_model(L.SPHERE, 3, DELTA, L.LS_GEOMETRIC)
        assert refine(h=empty._h) == L.ERR_STATE and untouched()
    # optional outputs may be absent
    load(ctx, data)
    assert lib.lsqr_refine_lm(ctx._h, L.ptr(params), 3, 1, 0, None, None, fits, L.ptr(status), C.byref(rounds),
                              C.byref(conv)) == L.OK
    assert rounds.value == 1 and np.all(status == L.OK) and not np.array_equal(bits(params), bits(keep))
    got = ctx.refine_lm(rows0, max_rounds=1)
    assert np.array_equal(bits(got["params"]), bits(params))
    assert [f.lm_nfev for f in fits] == list(got["lm_nfev"]) and [f.n_params for f in fits] == [4, 4, 4]
