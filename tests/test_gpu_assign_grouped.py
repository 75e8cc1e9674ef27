"""lsqr_assign_grouped / lsqr_refine_grouped (csrc/assign_grouped.h) through Context.assign_grouped / refine_grouped.

The reference is the contract itself: for every group a fresh upload of data[groups == g] on a second context, then
Context.assign(rows_g, want_residuals=True) and Context.refine(rows_g, max_rounds) -- the ungrouped entry points.
Everything is compared bit for bit (view(np.uint8)): labels at the group's places, residuals, counts, and for refine
the parameters, status, n_used, rounds and converged.

The scene: ten groups whose sizes sit where the pass can go wrong (0, 2, 300, exactly one chunk of 2048, 2049, 5000
and larger), interleaved with a fixed permutation, some records labelled -1 and n_groups + 3, two records with a NaN /
Inf coordinate; one group without models, one with one, one of 300 records with 64 rows (bit 63 of the presence mask).
Start rows: the planted truth plus a perturbation whose size differs from group to group, so that the groups stop at
different rounds -- which is asserted on the reference results alone."""
import ctypes as C

import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd import synth
from lsqrrecipes_amd.context import Context

pytestmark = pytest.mark.gpu

NG, MM = 10, 3
# records / models of group g
SIZES = [0, 2, 300, 2048, 2049, 5000, 300, 3000, 4000, 13000]
NMODELS = [3, 3, 3, 3, 3, 3, 64, 0, 1, 3]
G_EMPTY, G_TWO, G_64, G_NOMODEL, G_ONE = 0, 1, 6, 7, 8
N_OUT = 150  # records labelled -1, and as many labelled NG + 3
# the size of the start rows' perturbation per group (0: the planted truth)
SCALE = [1.0, 1.0, 0.0, 1.0, 3.0, 2.0, 1.0, 1.0, 2.0, 3.0]

# name -> (model, dim, delta, ls_type, synth generator, its dim keyword)
MODELS = {
    "plane": (L.PLANE, 3, 0.5, L.LS_ALGEBRAIC, synth.plane, {}),
    "line": (L.LINE, 3, 0.5, L.LS_ALGEBRAIC, synth.line, {}),
    "sphere": (L.SPHERE, 3, 0.5, L.LS_ALGEBRAIC, synth.sphere, {}),
    "plane5": (L.PLANE, 5, 0.5, L.LS_ALGEBRAIC, synth.plane, {"dim": 5}),
    "sphere_geo": (L.SPHERE, 3, 0.5, L.LS_GEOMETRIC, synth.sphere, {}),
}
REFINE = ["plane", "line", "sphere", "plane5"]
_scenes, _refs = {}, {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _perturb(name, truth, scale, rng):
    """a start row: the point moved by 0.08 * scale, the unit vector turned by 2e-4 * scale (0.1 * scale at the far end
    of the scene), the radius changed by 0.05 * scale -- inside the band of 0.5 for most records, outside for some"""
    model, dim = MODELS[name][:2]
    row = np.array(truth, dtype=np.float64)
    if model == L.SPHERE:
        row[:dim] += 0.08 * scale * rng.standard_normal(dim)
        row[dim] += 0.05 * scale * rng.standard_normal()
    else:
        v = row[:dim] + 2e-4 * scale * rng.standard_normal(dim)
        row[:dim] = v / np.linalg.norm(v)
        row[dim:] += 0.08 * scale * rng.standard_normal(dim)
    return row


def _point(name):
    model, dim = MODELS[name][:2]
    return slice(0, dim) if model == L.SPHERE else slice(dim, 2 * dim)


def scene(name):
    """-> data (N x dim), groups (N, int32), params (NG x 64 x P), n_models (NG); computed once, never changed"""
    if name not in _scenes:
        gen, kw = MODELS[name][4], MODELS[name][5]
        rng = np.random.default_rng(20240611)
        parts, labels = [], []
        params = None
        for g, n in enumerate(SIZES):
            m = max((3 * n) // 10, 1 if n else 0)
            planted = [gen(max(m, 2), 0.0, seed=0x61000 + 16 * g + j, sigma=0.1, **kw) for j in range(3)]
            truth = [p[1] for p in planted]
            if params is None:
                params = np.zeros((NG, 64, len(truth[0])))
            if n == 2:
                recs = planted[0][0][:2]
            elif n:
                clutter = gen(n - 3 * m, 1.0, seed=0x61999 + g, **kw)[0]
                recs = np.vstack([p[0][:m] for p in planted] + [clutter])
            else:
                recs = np.zeros((0, planted[0][0].shape[1]))
            assert recs.shape[0] == n
            parts.append(recs)
            labels.append(np.full(n, g, dtype=np.int32))
            start = [_perturb(name, t, SCALE[g], rng) for t in truth]
            for k in range(64):  # (rows k >= 3 matter for the 64-row group alone: the three at small offsets)
                params[g, k] = start[k % 3]
                if k >= 3:
                    params[g, k, _point(name)] += 0.02 * rng.standard_normal(params[g, k, _point(name)].shape)
        dim = parts[1].shape[1]
        out = gen(2 * N_OUT, 1.0, seed=0x61AAA, **kw)[0]
        parts.append(out)
        labels.append(np.concatenate([np.full(N_OUT, -1, dtype=np.int32), np.full(N_OUT, NG + 3, dtype=np.int32)]))
        data, groups = np.vstack(parts), np.concatenate(labels)
        perm = np.random.default_rng(424242).permutation(data.shape[0])
        data, groups = np.ascontiguousarray(data[perm]), np.ascontiguousarray(groups[perm])
        data[np.flatnonzero(groups == 5)[7], 1] = np.nan
        data[np.flatnonzero(groups == 9)[2500], dim - 1] = np.inf
        nm = np.array(NMODELS, dtype=np.uintp)
        for a in (data, groups, params, nm):
            a.setflags(write=False)
        assert 29000 < data.shape[0] < 31000
        _scenes[name] = (data, groups, params, nm)
    return _scenes[name]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx2():
    c = Context(0)
    yield c
    c.close()


def _setup(c, name):
    model, dim, delta, ls = MODELS[name][:4]
    c.set_model(model, dim, delta, ls)
    return c


def put(ctx, name):
    data, groups, params, nm = scene(name)
    _setup(ctx, name).upload(data)
    return data, groups, params, nm


def reference(ctx2, name, what):
    """the ungrouped entry points on a fresh upload of every group that runs: what = "assign" or a max_rounds
    -> {g: dict}; computed once, never changed"""
    if (name, what) not in _refs:
        data, groups, params, nm = scene(name)
        out = {}
        for g in range(NG):
            rows = params[g, :nm[g]]
            if SIZES[g] == 0 or nm[g] == 0:
                continue
            _setup(ctx2, name).upload(np.ascontiguousarray(data[groups == g]))
            out[g] = ctx2.assign(rows, want_residuals=True) if what == "assign" else ctx2.refine(rows, max_rounds=what)
        _refs[name, what] = out
    return _refs[name, what]


def check_outside(groups, labels, residuals=None):
    """a record in no group, or in a group that runs nothing: -1 and +inf"""
    dead = (groups < 0) | (groups >= NG) | (groups == G_NOMODEL)
    assert dead.sum() == 2 * N_OUT + SIZES[G_NOMODEL]
    assert np.all(labels[dead] == -1)
    if residuals is not None:
        assert np.all(np.isposinf(residuals[dead]))


def check_counts(got, g, ref_counts, nm):
    """counts row g: the reference's nm + 1 counts, zeros for the rows that are not there, the unassigned last"""
    want = np.zeros(got["counts"].shape[1], dtype=np.uint64)
    want[:nm] = ref_counts[:nm]
    want[-1] = ref_counts[nm]
    assert np.array_equal(got["counts"][g], want), g


# ---- assign ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODELS))
def test_assign_grouped_equals_assign_on_every_group(ctx, ctx2, name):
    data, groups, params, nm = put(ctx, name)
    ref = reference(ctx2, name, "assign")
    got = ctx.assign_grouped(groups, NG, params, nm, want_residuals=True)
    assert got["labels"].dtype == np.int32 and got["residuals"].dtype == np.float64
    assert np.array_equal(got["offsets"], np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint64))
    for g, r in ref.items():
        at = groups == g
        assert np.array_equal(got["labels"][at], r["labels"]), g
        assert np.array_equal(bits(got["residuals"][at]), bits(r["residuals"])), g
        check_counts(got, g, r["counts"], int(nm[g]))
    check_outside(groups, got["labels"], got["residuals"])
    # what runs nothing: zero counts, the group's records unassigned
    assert not got["counts"][G_EMPTY].any()
    assert not got["counts"][G_NOMODEL][:-1].any() and got["counts"][G_NOMODEL][-1] == SIZES[G_NOMODEL]
    # the scene does what it is for
    assert set(np.unique(ref[9]["labels"])) == {-1, 0, 1, 2} and ref[G_64]["labels"].max() > 3
    assert np.all(got["labels"][np.any(~np.isfinite(data), axis=1)] == -1)
    plain = ctx.assign_grouped(groups, NG, params, nm)
    assert plain["residuals"] is None and np.array_equal(plain["labels"], got["labels"])


def test_assign_grouped_equals_the_host_call(ctx):
    data, groups, params, nm = put(ctx, "plane")
    got = ctx.assign_grouped(groups, NG, params, nm, want_residuals=True)
    cfg = L.ModelCfg(*MODELS["plane"][:4], 0, 0.0)
    lib = L.load()
    inside = np.flatnonzero((groups >= 0) & (groups < NG) & (groups != G_NOMODEL))
    sample = np.random.default_rng(99).choice(inside, 200, replace=False)
    nonfinite = np.flatnonzero(np.any(~np.isfinite(data), axis=1))
    assert len(nonfinite) == 2
    label, res = C.c_int32(0), C.c_double(0.0)
    for i in np.concatenate([sample, nonfinite]):
        g = groups[i]
        rows, rec = np.ascontiguousarray(params[g, :nm[g]]), np.ascontiguousarray(data[i])
        assert lib.lsqr_assign_host(C.byref(cfg), L.ptr(rows), int(nm[g]), L.ptr(rec), C.byref(label),
                                    C.byref(res)) == L.OK
        assert got["labels"][i] == label.value, i
        assert bits(got["residuals"][i:i + 1]).tolist() == bits(np.array([res.value])).tolist(), i
    check_outside(groups, got["labels"], got["residuals"])
    assert np.all(got["labels"][nonfinite] == -1) and np.all(np.isposinf(got["residuals"][nonfinite]))


# ---- refine ---------------------------------------------------------------------------------------------------------
def check_refine(got, ref, groups, params, nm):
    for g, r in ref.items():
        n = int(nm[g])
        assert np.array_equal(got["labels"][groups == g], r["labels"]), g
        check_counts(got, g, r["counts"], n)
        assert np.array_equal(bits(got["params"][g, :n]), bits(r["params"])), g
        assert np.array_equal(got["status"][g, :n], r["status"]), g
        assert np.array_equal(got["n_used"][g, :n], r["n_used"]), g
        assert got["rounds"][g] == r["rounds"] and bool(got["converged"][g]) == r["converged"], g
    for g in range(NG):
        n = int(nm[g])
        # rows that are not there: never written, "model not there"
        assert np.array_equal(bits(got["params"][g, n:]), bits(params[g, n:got["params"].shape[1]])), g
        assert np.all(got["status"][g, n:] == L.ERR_STATE) and not got["n_used"][g, n:].any(), g
        if g not in ref:  # runs nothing
            assert got["rounds"][g] == 0 and not got["converged"][g]
            assert np.all(got["status"][g, :n] == L.OK) and not got["n_used"][g].any()
            assert np.array_equal(bits(got["params"][g]), bits(params[g, :got["params"].shape[1]]))
    check_outside(groups, got["labels"])


@pytest.mark.parametrize("max_rounds", [0, 1, 8])
@pytest.mark.parametrize("name", REFINE)
def test_refine_grouped_equals_refine_on_every_group(ctx, ctx2, name, max_rounds):
    data, groups, params, nm = put(ctx, name)
    ref = reference(ctx2, name, max_rounds)
    # the reference alone shows that the groups stop at different rounds
    rounds = {g: r["rounds"] for g, r in ref.items()}
    print(name, max_rounds, "rounds", rounds, "converged", {g: r["converged"] for g, r in ref.items()})
    if max_rounds == 8:
        assert len(set(rounds.values())) >= 2, rounds
        assert any(r["converged"] and r["rounds"] >= 2 for r in ref.values()), rounds
    if max_rounds == 1:
        assert any(not r["converged"] for r in ref.values())
    got = ctx.refine_grouped(groups, NG, params, nm, max_rounds=max_rounds)
    check_refine(got, ref, groups, params, nm)
    if max_rounds == 0:
        same = ctx.assign_grouped(groups, NG, params, nm)
        assert np.array_equal(same["labels"], got["labels"]) and np.array_equal(same["counts"], got["counts"])
    else:  # the returned labels are the grouped assignment of the returned parameters
        again = ctx.assign_grouped(groups, NG, got["params"], nm)
        assert np.array_equal(again["labels"], got["labels"]) and np.array_equal(again["counts"], got["counts"])


def test_refine_grouped_refuses_the_geometric_sphere(ctx):
    data, groups, params, nm = put(ctx, "sphere_geo")
    with pytest.raises(L.LsqrError) as e:
        ctx.refine_grouped(groups, NG, params, nm)
    assert e.value.status == L.ERR_INVALID


# ---- forms and independence -------------------------------------------------------------------------------------------
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


def test_device_form_equals_host_form_and_writes_every_label(ctx):
    data, groups, params, nm = put(ctx, "plane")
    n = data.shape[0]
    host_a = ctx.assign_grouped(groups, NG, params, nm, want_residuals=True)
    host_r = ctx.refine_grouped(groups, NG, params, nm, max_rounds=8)
    grp = DeviceArray(groups)
    lab = DeviceArray(np.full(n, -9, dtype=np.int32))
    res = DeviceArray(np.full(n, -9.0))
    try:
        dev = ctx.assign_grouped(grp, NG, params, nm, labels_out=lab)
        assert dev["labels"] is lab and np.array_equal(lab.get(), host_a["labels"])  # no -9 left: -1 is a label
        assert np.array_equal(dev["counts"], host_a["counts"]) and np.array_equal(dev["offsets"], host_a["offsets"])
        # the residuals of the device form (the C ABI: Context leaves them out)
        lab.put(np.full(n, -9, dtype=np.int32))
        p = np.ascontiguousarray(params)
        assert L.load().lsqr_assign_grouped(ctx._h, grp.data_ptr(), NG, 1, L.ptr(p), L.ptr(nm), 64, lab.data_ptr(),
                                            res.data_ptr(), None, None) == L.OK
        assert np.array_equal(lab.get(), host_a["labels"])
        assert np.array_equal(bits(res.get()), bits(host_a["residuals"]))
        lab.put(np.full(n, -9, dtype=np.int32))
        dev = ctx.refine_grouped(grp, NG, params, nm, max_rounds=8, labels_out=lab)
        assert dev["labels"] is lab and np.array_equal(lab.get(), host_r["labels"])
        for key in ("params", "counts", "status", "n_used", "rounds", "converged", "offsets"):
            assert np.array_equal(bits(dev[key]), bits(host_r[key])), key
        none = ctx.refine_grouped(grp, NG, params, nm, max_rounds=8)  # the labels are optional
        assert none["labels"] is None and np.array_equal(bits(none["params"]), bits(host_r["params"]))
    finally:
        grp.free()
        lab.free()
        res.free()


def test_groups_do_not_depend_on_each_other_or_on_their_numbering(ctx):
    data, groups, params, nm = put(ctx, "plane")
    base = ctx.refine_grouped(groups, NG, params, nm, max_rounds=8)
    base_a = ctx.assign_grouped(groups, NG, params, nm, want_residuals=True)
    twice = ctx.refine_grouped(groups, NG, params, nm, max_rounds=8)
    for key in ("params", "labels", "counts", "status", "n_used", "rounds", "converged", "offsets"):
        assert np.array_equal(bits(twice[key]), bits(base[key])), key
    twice_a = ctx.assign_grouped(groups, NG, params, nm, want_residuals=True)
    assert np.array_equal(twice_a["labels"], base_a["labels"])
    assert np.array_equal(bits(twice_a["residuals"]), bits(base_a["residuals"]))

    def compare(new_of_old, n_new):
        """new_of_old[g]: group g's id in the new call, or -1 when it is dropped"""
        lut = np.full(NG + 4, -1, dtype=np.int32)
        lut[:NG] = new_of_old
        g2 = np.where(groups >= 0, lut[np.clip(groups, 0, NG + 3)], -1).astype(np.int32)
        p2 = np.zeros((n_new,) + params.shape[1:])
        nm2 = np.zeros(n_new, dtype=np.uintp)
        for g in range(NG):
            if new_of_old[g] >= 0:
                p2[new_of_old[g]], nm2[new_of_old[g]] = params[g], nm[g]
        r = ctx.refine_grouped(g2, n_new, p2, nm2, max_rounds=8)
        a = ctx.assign_grouped(g2, n_new, p2, nm2, want_residuals=True)
        for g in range(NG):
            h = new_of_old[g]
            at = groups == g
            if h < 0:
                assert np.all(r["labels"][at] == -1) and np.all(np.isposinf(a["residuals"][at]))
                continue
            assert np.array_equal(r["labels"][at], base["labels"][at]), g
            for key in ("params", "counts", "status", "n_used", "rounds", "converged"):
                assert np.array_equal(bits(r[key][h]), bits(base[key][g])), (key, g)
            assert np.array_equal(a["labels"][at], base_a["labels"][at]), g
            assert np.array_equal(bits(a["residuals"][at]), bits(base_a["residuals"][at])), g
            assert np.array_equal(a["counts"][h], base_a["counts"][g]), g

    compare(np.random.default_rng(5).permutation(NG).astype(np.int32), NG)
    half = np.full(NG, -1, dtype=np.int32)
    half[[1, 4, 5, 6, 9]] = np.arange(5)
    compare(half, 5)


# ---- arguments and side effects -----------------------------------------------------------------------------------------
def test_argument_errors_in_order_write_nothing(ctx):
    lib = L.load()
    data, groups, params, nm = put(ctx, "plane")
    n = data.shape[0]
    par = np.ascontiguousarray(params[:, :MM]).copy()
    keep = par.copy()
    nmod = np.minimum(nm, MM).astype(np.uintp)
    labels = np.full(n, 42, dtype=np.int32)
    res = np.full(n, 42.0)
    counts = np.full((NG, MM + 1), 42, dtype=np.uint64)
    offs = np.full(NG + 1, 42, dtype=np.uint64)
    status = np.full(NG * MM, 42, dtype=np.int32)
    fits = (L.FitInfo * (NG * MM))()
    C.memset(fits, 0x5A, C.sizeof(fits))
    rounds = np.full(NG, 42, dtype=np.uintp)
    conv = np.full(NG, 42, dtype=np.int32)

    def assign(c=ctx, groups_=groups, ng=NG, par_=par, nm_=nmod, mm=MM, labels_=labels):
        return lib.lsqr_assign_grouped(c._h, L.ptr(groups_), ng, 0, L.ptr(par_), L.ptr(nm_), mm, L.ptr(labels_),
                                       L.ptr(res), L.ptr(counts), L.ptr(offs))

    def refine(c=ctx, groups_=groups, ng=NG, par_=par, nm_=nmod, mm=MM, fits_=fits, status_=status, rounds_=rounds,
               conv_=conv):
        return lib.lsqr_refine_grouped(c._h, L.ptr(groups_), ng, 0, L.ptr(par_), L.ptr(nm_), mm, 4, L.ptr(labels),
                                       L.ptr(counts), L.ptr(offs), fits_, L.ptr(status_), L.ptr(rounds_), L.ptr(conv_))

    def untouched():
        return (np.array_equal(bits(par), bits(keep)) and np.all(labels == 42) and np.all(res == 42.0)
                and np.all(counts == 42) and np.all(offs == 42) and np.all(status == 42)
                and bytes(fits) == b"\x5a" * C.sizeof(fits) and np.all(rounds == 42) and np.all(conv == 42))

    too_many = nmod.copy()
    too_many[NG - 1] = MM + 1
    for call in (assign, refine):
        # n_groups == 0 comes before every argument check
        assert call(ng=0, mm=65, groups_=None) == L.OK and untouched()
        assert call(mm=65) == L.ERR_INVALID and untouched()
        assert call(ng=2 ** 31) == L.ERR_INVALID and untouched()
        assert call(groups_=None) == L.ERR_INVALID and untouched()
        assert call(par_=None) == L.ERR_INVALID and untouched()
        assert call(nm_=None) == L.ERR_INVALID and untouched()
        assert call(nm_=too_many) == L.ERR_INVALID and untouched()
    assert assign(labels_=None) == L.ERR_INVALID and untouched()
    assert refine(fits_=None) == L.ERR_INVALID and untouched()
    assert refine(status_=None) == L.ERR_INVALID and untouched()
    assert refine(rounds_=None) == L.ERR_INVALID and untouched()
    assert refine(conv_=None) == L.ERR_INVALID and untouched()
    with Context(0) as empty:
        for call in (assign, refine):
            # the model comes first: no model is a state error even with n_groups == 0 and with bad arguments
            assert call(c=empty) == L.ERR_STATE and call(c=empty, ng=0) == L.ERR_STATE
            assert call(c=empty, mm=65) == L.ERR_STATE and untouched()
        empty.set_model(L.ABSOR, 3, 2.0, 0)
        for call in (assign, refine):
            assert call(c=empty, ng=0) == L.ERR_INVALID and untouched()
        empty.set_model(L.PLANE, 3, 0.5, L.LS_ALGEBRAIC)
        for call in (assign, refine):
            # the arguments come before the records: no records is a state error only with good arguments
            assert call(c=empty, mm=65) == L.ERR_INVALID and call(c=empty, nm_=too_many) == L.ERR_INVALID
            assert call(c=empty) == L.ERR_STATE and untouched()
    # max_models == 0: LSQR_OK, -1 / +inf, zero outputs
    none = np.zeros(NG, dtype=np.uintp)
    counts0 = np.full((NG, 1), 42, dtype=np.uint64)
    assert lib.lsqr_assign_grouped(ctx._h, L.ptr(groups), NG, 0, L.ptr(par), L.ptr(none), 0, L.ptr(labels), L.ptr(res),
                                   L.ptr(counts0), L.ptr(offs)) == L.OK
    assert np.all(labels == -1) and np.all(np.isposinf(res))
    assert np.array_equal(counts0[:, 0], np.array(SIZES, dtype=np.uint64))
    assert np.array_equal(offs, np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint64))
    labels[:] = 42
    assert lib.lsqr_refine_grouped(ctx._h, L.ptr(groups), NG, 0, L.ptr(par), L.ptr(none), 0, 4, L.ptr(labels), None,
                                   None, fits, L.ptr(status), L.ptr(rounds), L.ptr(conv)) == L.OK
    assert np.all(labels == -1) and not rounds.any() and not conv.any() and np.array_equal(bits(par), bits(keep))
    # optional outputs may be absent
    assert lib.lsqr_refine_grouped(ctx._h, L.ptr(groups), NG, 0, L.ptr(par), L.ptr(nmod), MM, 1, None, None, None, fits,
                                   L.ptr(status), L.ptr(rounds), L.ptr(conv)) == L.OK
    assert rounds[2] == 1 and rounds[G_NOMODEL] == 0 and rounds[G_EMPTY] == 0


def test_context_is_untouched(ctx):
    data, groups, params, nm = put(ctx, "plane")
    n = int(L.load().lsqr_count(ctx._h))
    ctx.hypotheses_sample(17, 0, 256)
    ctx.scan()
    hyp_before = ctx.hypotheses()
    row = params[9, 1]
    mask_before, cnt_before = ctx.mask(row)
    out = ctx.refine_grouped(groups, NG, params, nm, max_rounds=8)
    assert out["rounds"].max() >= 1
    ctx.assign_grouped(groups, NG, params, nm, want_residuals=True)
    fit_after, _ = ctx.ls_fit(use_mask=True)  # the mask of `row`, and its point as the fit origin, are still there
    assert int(L.load().lsqr_count(ctx._h)) == n == data.shape[0]
    for a, b in zip(hyp_before, ctx.hypotheses()):
        assert np.array_equal(bits(a), bits(b))
    mask_after, cnt_after = ctx.mask(row)
    fit_want, _ = ctx.ls_fit(use_mask=True)
    assert cnt_before == cnt_after == mask_before.sum() and np.array_equal(mask_before, mask_after)
    assert np.array_equal(bits(fit_after), bits(fit_want))
