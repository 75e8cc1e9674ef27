"""lsqr_refine_lm_grouped (csrc/assign_lm_grouped.h) through Context.refine_lm_grouped: lsqr_refine_grouped's loop for
the geometric sphere, the refit a Levenberg-Marquardt run per (group, model) on the device.

The reference is the contract itself: for every group a fresh upload of data[groups == g] on a second context, then
Context.refine_lm(rows_g, max_rounds) -- the ungrouped entry point.  Everything is compared bit for bit
(view(np.uint8)): the labels at the group's places, the counts, the parameters, status, rounds, converged and the whole
lsqr_fit_info of every model (n_params, lm_info, lm_nfev, reserved = the stall evaluation, n_used, cost).

The scene is built as tests/test_gpu_assign_grouped.py builds "sphere_geo": ten groups whose sizes sit where the
kernels can go wrong (0, 2, 300, exactly one chunk of 2048, 2049, 5000 and larger), interleaved with a fixed
permutation, 150 records labelled -1 and 150 labelled n_groups + 3, two records with a NaN / Inf coordinate; one group
without models, one with one, one of 300 records with 64 rows.  Start rows: the planted truth plus a perturbation
whose size differs from group to group, so that the groups stop at different rounds and their LM runs take different
numbers of evaluations -- asserted on the reference results alone.  A CPU simulation of the 3-D scene (numpy
assignment + the oracle's geometric fit per model, the loop of tests/test_gpu_refine_lm.py's docstring) gave at
max_rounds = 8 the rounds {1: 1, 2: 1, 3: 2, 4: 2, 5: 2, 6: 7, 8: 2, 9: 2}, every group converged, and at max_rounds = 1
groups 1 and 2 converged and the six others not; in 2-D and 5-D at max_rounds = 1 one refit round in every group, the
group of 300 records converged, the two others not."""
import ctypes as C

import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd import synth
from lsqrrecipes_amd.context import Context
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu

DELTA = 0.5
# the 3-D scene: records / models / the size of the start rows' perturbation of group g (0: the planted truth)
SIZES = [0, 2, 300, 2048, 2049, 5000, 300, 3000, 4000, 13000]
NMODELS = [3, 3, 3, 3, 3, 3, 64, 0, 1, 3]
SCALE = [1.0, 1.0, 0.0, 1.0, 3.0, 2.0, 1.0, 1.0, 2.0, 3.0]
G_EMPTY, G_TWO, G_64, G_NOMODEL, G_ONE = 0, 1, 6, 7, 8
# the 2-D and 5-D scenes: below one chunk, one chunk plus one record, several chunks with an odd tail
SIZES_D = [300, 2049, 5000]
NMODELS_D = [3, 3, 3]
SCALE_D = [1.0, 3.0, 2.0]
N_OUT = 150  # records labelled -1, and as many labelled n_groups + 3
KEYS = ("params", "counts", "status", "n_used", "rounds", "converged", "lm_info", "lm_nfev", "cost", "stall")
_scenes, _refs = {}, {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _perturb(dim, truth, scale, rng):
    """a start row: the centre moved by 0.08 * scale, the radius changed by 0.05 * scale -- inside the band of 0.5 for
    most records, outside for some"""
    row = np.array(truth, dtype=np.float64)
    row[:dim] += 0.08 * scale * rng.standard_normal(dim)
    row[dim] += 0.05 * scale * rng.standard_normal()
    return row


def scene(dim):
    """-> data (N x dim), groups (N, int32), params (NG x 64 x P), n_models (NG), sizes; computed once, never changed"""
    if dim not in _scenes:
        sizes, nmodels, scale = (SIZES, NMODELS, SCALE) if dim == 3 else (SIZES_D, NMODELS_D, SCALE_D)
        ng = len(sizes)
        kw = {} if dim == 3 else {"dim": dim}
        rng = np.random.default_rng(20240611)
        parts, labels = [], []
        params = np.zeros((ng, 64, dim + 1))
        for g, n in enumerate(sizes):
            m = max((3 * n) // 10, 1 if n else 0)
            planted = [synth.sphere(max(m, 2), 0.0, seed=0x61000 + 16 * g + j, sigma=0.1, **kw) for j in range(3)]
            truth = [p[1] for p in planted]
            if n == 2:
                recs = planted[0][0][:2]
            elif n:
                clutter = synth.sphere(n - 3 * m, 1.0, seed=0x61999 + g, **kw)[0]
                recs = np.vstack([p[0][:m] for p in planted] + [clutter])
            else:
                recs = np.zeros((0, dim))
            assert recs.shape == (n, dim)
            parts.append(recs)
            labels.append(np.full(n, g, dtype=np.int32))
            start = [_perturb(dim, t, scale[g], rng) for t in truth]
            for k in range(64):  # (rows k >= 3 matter for the 64-row group alone: the three at small offsets)
                params[g, k] = start[k % 3]
                if k >= 3:
                    params[g, k, :dim] += 0.02 * rng.standard_normal(dim)
        out = synth.sphere(2 * N_OUT, 1.0, seed=0x61AAA, **kw)[0]
        parts.append(out)
        labels.append(np.concatenate([np.full(N_OUT, -1, dtype=np.int32), np.full(N_OUT, ng + 3, dtype=np.int32)]))
        data, groups = np.vstack(parts), np.concatenate(labels)
        perm = np.random.default_rng(424242).permutation(data.shape[0])
        data, groups = np.ascontiguousarray(data[perm]), np.ascontiguousarray(groups[perm])
        if dim == 3:
            data[np.flatnonzero(groups == 5)[7], 1] = np.nan
            data[np.flatnonzero(groups == 9)[2500], dim - 1] = np.inf
        nm = np.array(nmodels, dtype=np.uintp)
        for a in (data, groups, params, nm):
            a.setflags(write=False)
        _scenes[dim] = (data, groups, params, nm, sizes)
    return _scenes[dim]


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


def put(ctx, dim):
    data, groups, params, nm, sizes = scene(dim)
    ctx.set_model(L.SPHERE, dim, DELTA, L.LS_GEOMETRIC).upload(data)
    return data, groups, params, nm, sizes


def refine_lm_with_fits(c, rows, max_rounds):
    """Context.refine_lm, and the models' whole lsqr_fit_info (a structured array)"""
    out, f = c._refine(c._lib.lsqr_refine_lm, rows, max_rounds, None)
    out.update(lm_info=f["lm_info"].copy(), lm_nfev=f["lm_nfev"].copy(), cost=f["cost"].copy(),
               stall=f["reserved"].copy(), fits=f.copy())
    return out


def grouped_with_fits(c, groups, n_groups, params, nm, max_rounds, labels_out=None):
    """Context.refine_lm_grouped, and every model's whole lsqr_fit_info ((n_groups, max_models), structured)"""
    out, f = c._refine_grouped(c._lib.lsqr_refine_lm_grouped, groups, n_groups, params, nm, max_rounds, labels_out)
    out.update(lm_info=f["lm_info"].copy(), lm_nfev=f["lm_nfev"].copy(), cost=f["cost"].copy(),
               stall=f["reserved"].copy(), fits=f.copy())
    return out


def reference_of(ctx2, dim, data, groups, params, nm, max_rounds):
    """lsqr_refine_lm on a fresh upload of every group that runs -> {g: dict}"""
    out = {}
    for g in range(len(nm)):
        at = groups == g
        if not at.any() or nm[g] == 0:
            continue
        ctx2.set_model(L.SPHERE, dim, DELTA, L.LS_GEOMETRIC).upload(np.ascontiguousarray(data[at]))
        out[g] = refine_lm_with_fits(ctx2, params[g, :nm[g]], max_rounds)
    return out


def reference(ctx2, dim, max_rounds):
    """the scene's reference; computed once, never changed"""
    if (dim, max_rounds) not in _refs:
        data, groups, params, nm, _ = scene(dim)
        _refs[dim, max_rounds] = reference_of(ctx2, dim, data, groups, params, nm, max_rounds)
    return _refs[dim, max_rounds]


def check_group(got, g, r, at, n):
    """group g of the grouped call against the ungrouped call r on the group's gather, bit for bit"""
    assert np.array_equal(got["labels"][at], r["labels"]), g
    want = np.zeros(got["counts"].shape[1], dtype=np.uint64)
    want[:n] = r["counts"][:n]
    want[-1] = r["counts"][n]
    assert np.array_equal(got["counts"][g], want), g
    assert np.array_equal(bits(got["params"][g, :n]), bits(r["params"])), g
    assert np.array_equal(got["status"][g, :n], r["status"]), g
    assert got["rounds"][g] == r["rounds"] and bool(got["converged"][g]) == r["converged"], g
    for key in ("n_used", "lm_info", "lm_nfev", "stall"):
        assert np.array_equal(got[key][g, :n], r[key]), (key, g, got[key][g, :n], r[key])
    assert np.array_equal(bits(got["cost"][g, :n]), bits(r["cost"])), g
    assert np.array_equal(got["fits"]["n_params"][g, :n], r["fits"]["n_params"]), g
    assert np.array_equal(bits(got["fits"][g, :n]), bits(r["fits"])), g  # every field of lsqr_fit_info


def check_all(got, ref, groups, params, nm):
    ng = len(nm)
    for g, r in ref.items():
        check_group(got, g, r, groups == g, int(nm[g]))
    zero = bytes(C.sizeof(L.FitInfo))
    for g in range(ng):
        n = int(nm[g])
        # rows that are not there: never written, "model not there" with a zeroed fit
        assert np.array_equal(bits(got["params"][g, n:]), bits(params[g, n:got["params"].shape[1]])), g
        assert np.all(got["status"][g, n:] == L.ERR_STATE), g
        assert all(bytes(f) == zero for f in got["fits"][g, n:]), g
        if g not in ref:  # runs nothing
            assert got["rounds"][g] == 0 and not got["converged"][g]
            assert np.all(got["status"][g, :n] == L.OK) and all(bytes(f) == zero for f in got["fits"][g]), g
            assert np.array_equal(bits(got["params"][g]), bits(params[g, :got["params"].shape[1]]))
    # a record in no group, or in a group that runs nothing: -1
    dead = (groups < 0) | (groups >= ng) | ~np.isin(groups, list(ref))
    assert dead.sum() >= 2 * N_OUT and np.all(got["labels"][dead] == -1)


# ---- 1: equality with lsqr_refine_lm on every group ---------------------------------------------------------------------
@pytest.mark.parametrize("max_rounds", [0, 1, 8])
def test_refine_lm_grouped_equals_refine_lm_on_every_group(ctx, ctx2, max_rounds):
    data, groups, params, nm, sizes = put(ctx, 3)
    ng = len(nm)
    ref = reference(ctx2, 3, max_rounds)
    assert sorted(ref) == [1, 2, 3, 4, 5, 6, 8, 9]
    rounds = {g: r["rounds"] for g, r in ref.items()}
    print("max_rounds", max_rounds, "rounds", rounds, "converged", {g: r["converged"] for g, r in ref.items()},
          "lm_nfev", {g: list(r["lm_nfev"][:3]) for g, r in ref.items()})
    # the reference alone shows that the scene does its job
    if max_rounds == 8:
        assert len(set(rounds.values())) >= 2, rounds
        assert any(r["converged"] and r["rounds"] >= 2 for r in ref.values()), rounds
    if max_rounds == 1:
        assert any(not r["converged"] for r in ref.values())
        # one refit round for every group: the groups' LM runs take different numbers of evaluations
        three = [tuple(r["lm_nfev"]) for g, r in ref.items() if nm[g] == 3 and r["rounds"] == 1 and sizes[g] > 2]
        assert len(three) >= 2 and len(set(three)) >= 2, three
    if max_rounds > 0:
        assert ref[G_TWO]["rounds"] >= 1 and not ref[G_TWO]["lm_info"].any()  # fewer than K records: no run starts
        assert np.all(ref[G_TWO]["status"] == L.EMPTY)
    else:
        assert ref[G_64]["labels"].max() > 3 and set(np.unique(ref[9]["labels"])) == {-1, 0, 1, 2}
    got = grouped_with_fits(ctx, groups, ng, params, nm, max_rounds)
    assert got["labels"].dtype == np.int32
    assert np.array_equal(got["offsets"], np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64))
    check_all(got, ref, groups, params, nm)
    assert np.all(got["labels"][np.any(~np.isfinite(data), axis=1)] == -1)
    assert not got["counts"][G_EMPTY].any()
    assert not got["counts"][G_NOMODEL][:-1].any() and got["counts"][G_NOMODEL][-1] == sizes[G_NOMODEL]
    # Context.refine_lm_grouped is that call
    plain = ctx.refine_lm_grouped(groups, ng, params, nm, max_rounds=max_rounds)
    for key in KEYS + ("labels", "offsets"):
        assert np.array_equal(bits(plain[key]), bits(got[key])), key
    assert plain["lm_info"].shape == plain["lm_nfev"].shape == plain["cost"].shape == plain["stall"].shape == (ng, 64)


# ---- 2: other dimensions (NMOM_LM differs: the lane-per-moment paths) ----------------------------------------------------
@pytest.mark.parametrize("dim", [2, 5])
def test_refine_lm_grouped_in_other_dimensions(ctx, ctx2, dim):
    data, groups, params, nm, sizes = put(ctx, dim)
    ref = reference(ctx2, dim, 1)
    assert sorted(ref) == [0, 1, 2] and all(r["rounds"] == 1 for r in ref.values())
    assert all(np.any((r["lm_info"] >= 1) & (r["lm_info"] <= 4)) for r in ref.values())
    got = grouped_with_fits(ctx, groups, len(nm), params, nm, 1)
    check_all(got, ref, groups, params, nm)


# ---- 3: the labels are the grouped assignment of the returned parameters ---------------------------------------------------
def test_labels_are_the_grouped_assignment_of_the_returned_parameters(ctx):
    data, groups, params, nm, sizes = put(ctx, 3)
    ng = len(nm)
    zero = ctx.refine_lm_grouped(groups, ng, params, nm, max_rounds=0)
    same = ctx.assign_grouped(groups, ng, params, nm)
    assert np.array_equal(zero["labels"], same["labels"]) and np.array_equal(zero["counts"], same["counts"])
    assert not zero["rounds"].any() and not zero["converged"].any() and not zero["lm_info"].any()
    assert np.array_equal(bits(zero["params"]), bits(params))
    for max_rounds in (1, 8):
        got = ctx.refine_lm_grouped(groups, ng, params, nm, max_rounds=max_rounds)
        again = ctx.assign_grouped(groups, ng, got["params"], nm)
        assert np.array_equal(again["labels"], got["labels"]) and np.array_equal(again["counts"], got["counts"])
        assert not np.array_equal(bits(got["params"][9, :3]), bits(params[9, :3]))  # (they were refitted)


# ---- 4: independence and determinism ---------------------------------------------------------------------------------------
def test_groups_do_not_depend_on_each_other_or_on_their_numbering(ctx):
    data, groups, params, nm, sizes = put(ctx, 3)
    ng = len(nm)
    base = grouped_with_fits(ctx, groups, ng, params, nm, 8)
    twice = grouped_with_fits(ctx, groups, ng, params, nm, 8)
    for key in KEYS + ("labels", "offsets", "fits"):
        assert np.array_equal(bits(twice[key]), bits(base[key])), key

    def compare(new_of_old, n_new):
        """new_of_old[g]: group g's id in the new call, or -1 when it is dropped"""
        lut = np.full(ng + 4, -1, dtype=np.int32)
        lut[:ng] = new_of_old
        g2 = np.where(groups >= 0, lut[np.clip(groups, 0, ng + 3)], -1).astype(np.int32)
        p2 = np.zeros((n_new,) + params.shape[1:])
        nm2 = np.zeros(n_new, dtype=np.uintp)
        for g in range(ng):
            if new_of_old[g] >= 0:
                p2[new_of_old[g]], nm2[new_of_old[g]] = params[g], nm[g]
        r = grouped_with_fits(ctx, g2, n_new, p2, nm2, 8)
        for g in range(ng):
            h = new_of_old[g]
            at = groups == g
            if h < 0:
                assert np.all(r["labels"][at] == -1)
                continue
            assert np.array_equal(r["labels"][at], base["labels"][at]), g
            for key in KEYS + ("fits",):
                assert np.array_equal(bits(r[key][h]), bits(base[key][g])), (key, g)

    compare(np.random.default_rng(5).permutation(ng).astype(np.int32), ng)
    half = np.full(ng, -1, dtype=np.int32)
    half[[1, 4, 5, 6, 9]] = np.arange(5)
    compare(half, 5)


# ---- 5: a refit that gives no result keeps the row it had before the round ---------------------------------------------------
def test_a_failed_fit_keeps_its_row(ctx):
    """four records on a circle, far from the scene, in group 2, and a row through them as the group's row 1: four
    coplanar records give the algebraic start no result (the reference's fit of that set is empty, checked with the
    oracle), so the row must come back with the bits it went in with and EMPTY; the group's other rows and the other
    groups are refitted as without it"""
    data0, groups0, params0, nm0, sizes = scene(3)
    ng = len(nm0)
    c = np.array([5e4, 5e4, 5e4])
    four = c + np.array([[10.0, 10.0, 0.0], [10.0, -10.0, 0.0], [-10.0, 10.0, 0.0], [-10.0, -10.0, 0.0]])
    data = np.vstack([data0[:1000], four[:2], data0[1000:], four[2:]])
    groups = np.concatenate([groups0[:1000], [2, 2], groups0[1000:], [2, 2]]).astype(np.int32)
    row = np.concatenate([c, [np.sqrt(200.0)]])
    g_data = np.ascontiguousarray(data[groups == 2])
    own = np.all(np.abs(g_data - c) < 20.0, axis=1).astype(np.uint8)
    assert own.sum() == 4
    assert len(O.ls(O.cfg(O.SPHERE, 3, DELTA, O.LS_GEOMETRIC), g_data, own)) == 0
    ctx.set_model(L.SPHERE, 3, DELTA, L.LS_GEOMETRIC).upload(data)
    params = np.array(params0)
    params[2, :4] = np.vstack([params0[2, :1], row[None], params0[2, 1:3]])
    nm = np.array(nm0)
    nm[2] = 4
    base = grouped_with_fits(ctx, groups, ng, params0, nm0, 2)
    got = grouped_with_fits(ctx, groups, ng, params, nm, 2)
    labels = ctx.assign_grouped(groups, ng, params, nm)["labels"]
    assert np.array_equal(labels[groups == 2] == 1, own != 0)
    assert got["rounds"][2] == base["rounds"][2] >= 1 and got["converged"][2] == base["converged"][2]
    assert got["status"][2, 1] == L.EMPTY and got["n_used"][2, 1] == 4
    assert got["lm_info"][2, 1] == 0 and got["lm_nfev"][2, 1] == 0 and got["fits"]["n_params"][2, 1] == 0
    assert np.array_equal(bits(got["params"][2, 1]), bits(row))
    keep = [0, 2, 3]
    assert np.all(got["status"][2, keep] == L.OK)
    assert not np.array_equal(bits(got["params"][2, keep]), bits(params0[2, :3]))  # (they were refitted)
    for key in ("params", "status", "n_used", "lm_info", "lm_nfev", "cost", "stall", "fits"):
        assert np.array_equal(bits(got[key][2, keep]), bits(base[key][2, :3])), key
        for g in range(ng):
            if g != 2:
                assert np.array_equal(bits(got[key][g]), bits(base[key][g])), (key, g)
    assert np.array_equal(got["labels"][groups != 2], base["labels"][groups != 2])
    assert np.array_equal(got["rounds"], base["rounds"]) and np.array_equal(got["converged"], base["converged"])


# ---- 6: device groups and labels, a strided attach -------------------------------------------------------------------------
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


def test_device_form_and_strided_attach(ctx):
    data, groups, params, nm, sizes = put(ctx, 3)
    ng, n = len(nm), data.shape[0]
    host = grouped_with_fits(ctx, groups, ng, params, nm, 8)
    grp = DeviceArray(groups)
    lab = DeviceArray(np.full(n, -9, dtype=np.int32))
    wide = np.full((n, 4), -7.25)
    wide[:, :3] = data
    t = DeviceArray(wide)
    try:
        dev = grouped_with_fits(ctx, grp, ng, params, nm, 8, labels_out=lab)
        assert dev["labels"] is lab and np.array_equal(lab.get(), host["labels"])  # no -9 left: -1 is a label
        for key in KEYS + ("offsets", "fits"):
            assert np.array_equal(bits(dev[key]), bits(host[key])), key
        none = ctx.refine_lm_grouped(grp, ng, params, nm, max_rounds=8)  # the labels are optional
        assert none["labels"] is None and np.array_equal(bits(none["params"]), bits(host["params"]))
        # the records at a stride of four doubles, attached: the same bits, the buffer untouched
        ctx.attach(t.data_ptr(), n, 32, keepalive=t)
        lab.put(np.full(n, -9, dtype=np.int32))
        at = grouped_with_fits(ctx, grp, ng, params, nm, 8, labels_out=lab)
        ctx.synchronize()
        assert np.array_equal(lab.get(), host["labels"])
        for key in KEYS + ("offsets", "fits"):
            assert np.array_equal(bits(at[key]), bits(host[key])), key
        at_host = ctx.refine_lm_grouped(groups, ng, params, nm, max_rounds=8)
        assert np.array_equal(at_host["labels"], host["labels"])
        assert np.array_equal(bits(t.get()), bits(wide))
        assert np.array_equal(grp.get(), groups)
    finally:
        ctx.upload(np.zeros((4, 3)))  # let go of the attached buffer
        ctx._keep = None
        grp.free()
        lab.free()
        t.free()


# ---- 7, 8: side effects, and the call that keeps refusing ---------------------------------------------------------------------
def test_context_is_untouched(ctx):
    data, groups, params, nm, sizes = put(ctx, 3)
    n = int(L.load().lsqr_count(ctx._h))
    ctx.hypotheses_sample(17, 0, 256)
    ctx.scan()
    hyp_before = ctx.hypotheses()
    index_before = ctx.index_info()
    row = params[9, 1]
    mask_before, cnt_before = ctx.mask(row)
    out = ctx.refine_lm_grouped(groups, len(nm), params, nm, max_rounds=8)
    assert out["rounds"].max() >= 1
    fit_after, _ = ctx.ls_fit(use_mask=True)  # the mask of `row`, and its parameters as the fit's start, are still there
    assert int(L.load().lsqr_count(ctx._h)) == n == data.shape[0]
    for a, b in zip(hyp_before, ctx.hypotheses()):
        assert np.array_equal(bits(a), bits(b))
    assert ctx.index_info() == index_before
    mask_after, cnt_after = ctx.mask(row)
    fit_want, _ = ctx.ls_fit(use_mask=True)
    assert cnt_before == cnt_after == mask_before.sum() and np.array_equal(mask_before, mask_after)
    assert np.array_equal(bits(fit_after), bits(fit_want))


def test_refine_grouped_still_refuses_the_geometric_sphere(ctx):
    data, groups, params, nm, sizes = put(ctx, 3)
    with pytest.raises(L.LsqrError) as e:
        ctx.refine_grouped(groups, len(nm), params, nm)
    assert e.value.status == L.ERR_INVALID
