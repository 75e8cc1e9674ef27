"""Context.refine (lsqr_refine: one pass over the records per round, on the device) against the same rounds done with
the entry points that existed before it: per model lsqr_mask (N bytes down), lsqr_set_mask (N bytes up) and lsqr_ls_fit
-- M mask passes, M moment passes and 2 M PCIe transfers per round.  That baseline is the greedy round (a record may
sit in several masks); it leaves out the M residual passes and the numpy argmin a nearest-model round would add, so it
flatters the baseline.

Scene: --n points (default 10 M) in 3-D, four planes of 20 % each plus 20 % clutter, shuffled; plane model, delta 0.5.
Models: M = 4, 16, 64 rows -- the four planes, each repeated M / 4 times at small offsets along its normal, so that
every row has records and the rounds move records between rows.  The timed lsqr_refine calls ask for no labels
(labels_out = NULL: nothing per record crosses PCIe); assign_call_ms is Context.assign with its 4 N bytes to the host.

ms per refine round = (t(max_rounds = R2) - t(max_rounds = R1)) / (rounds done at R2 - rounds done at R1): the
parameter upload, the last assignment pass and the label copy are in both and cancel.  Every timed call ends with
host results (the stream has drained).  One warm call of each kind, then --reps repetitions, the three kinds
alternating; median and min .. max are reported.  hbm_fraction = n x 24 B / round time / 8 TB/s (the records' bytes
alone over the HBM3E peak: the label traffic, 8 B per record, is not counted).
One JSON line per M on stdout; --out FILE also writes them to FILE.

--model {plane,line,sphere,line2d} / --dim D: another model's kernels on a scene of lsqrrecipes_amd.synth -- four planted
models of 20 % each (sigma 0.4) and 20 % clutter, shuffled -- from the planted rows; M = 4 only.  With --grouped: split
(a), one group, alone.

--grouped: Context.refine_grouped (lsqr_refine_grouped: one model set per label) on the same --n plane records in three
splits: (a) 1 group of 4 models, (b) 1 000 groups of n / 1 000 records with 4 models each, (c) 50 000 groups of
n / 50 000 records with 3 models each.  Every group has its own planes (models / (models + 1) of its records, the rest clutter) and
starts from the planted rows moved off by a different amount, so the groups stop at different rounds; the labels are
shuffled over the upload.  The group labels live on the device and the timed calls ask for no labels: nothing per
record crosses PCIe.
ms per grouped round = (t(R2) - t(R1)) / (record-rounds done at R2 - at R1) x n, a record-round being one record of a
group in one refit round of that group: the time of a round in which every group is still going.  The sort, the gather
and the first pass are in both calls and cancel; grouped_call_ms is the whole call at R2 with them.
The parent's only route, loop_call_ms: per group a host gather (from one stable sort of the labels, not timed), upload, Context.refine(max_rounds = R2) and the labels
written back, timed on the first --loop-groups groups and scaled by n_groups / groups timed (the scaling is stated in
the line).  For (a) refine_round_ms is Context.refine on the same records and rows: what the sort, the gather and
the scatter cost is grouped_call_ms - refine_call_ms.  lane_share = records / (workgroups x 2048): the share of the
pass's lanes that hold a record.

--lm: Context.refine_lm (lsqr_refine_lm: the geometric sphere, a Levenberg-Marquardt run per model on the device) on the
--model sphere scene in 3-D: M = 4 and 64 rows, the four planted spheres moved off by 0.05 per centre coordinate, each
M / 4 times with radii up to +-0.4 apart.  Three kinds alternate in one process: refine_lm_round_ms as refine_round_ms
above; host_round_ms, the round the entry points allowed before -- Context.assign with its labels to the host, then per
model set_mask(labels == m) + ls_fit(use_mask=True) on the same geometric context --; and alg_refine_round_ms,
Context.refine on an algebraic context over the same records and rows, for scale.  lm_nfev: the evaluations per model
in the last refit round of the R2 call (a round costs about 1 + max(lm_nfev) passes over the records).

--grouped --lm: Context.refine_lm_grouped (lsqr_refine_lm_grouped: the geometric sphere with one model set per label).
Scene: --groups groups (default 3 000) of 300 .. 3 000 records each (--n is not used), every group three spheres of a
quarter of its records each (sigma 0.1) and a quarter clutter, its start rows the planted ones moved off by up to 0.05
per centre coordinate, per group its own size; the labels shuffled over the upload and resident on the device; the
timed calls ask for no labels.  Three kinds alternate: the call at max_rounds 0 (the sort, the gather and one pass),
at 1 (one refit round more) and at R2; then loop_call_ms, what a caller must do without the call: per group a host
gather (from one stable sort of the labels, not timed), upload, Context.refine_lm(max_rounds = R2) and the labels
written back, timed on the first --loop-groups groups and scaled by n_groups / groups timed.
evaluations: the LM evaluations of refit round 1, max(lm_nfev) over all models of the max_rounds = 1 call;
round1_ms = t(1) - t(0): that round, with its solve, its init and the assignment pass after it; eval_ms_upper =
round1_ms / evaluations.  idle_share[j - 1]: the share of the (group, chunk) workgroups of evaluation j of round 1 that
return at once -- no record of a model still live --, from the labels of the start rows and the models' lm_nfev.

--model dense --dim n: Context.refine_dense (lsqr_refine_dense: a mixture of linear regressions) on --n rows (default
1 M here) of n + 1 doubles: M planted regressions (--models, default 4 and 16) of 1 / (M + 1) of the rows each, Gaussian
a, noise 0.01 on b, the rest clutter; delta 0.04; the start rows are the planted ones moved off inside the noise band.
Two kinds alternate in one process: refine_round_ms as above, and baseline_round_ms, the round the entry points allowed
before: M x (lsqr_mask + lsqr_set_mask + lsqr_ls_fit).  rows_read_per_round: how often a round reads each row -- once
for the new call, 2 M times for the baseline (a mask pass and a Gram pass per model); partial_bytes: the call's device
scratch for the chunk blocks, which a round writes once and reads once.

--model dense --grouped: Context.refine_dense_grouped (lsqr_refine_dense_grouped: one regression set per label) on --n
rows split into --groups groups of n / groups rows each, every group its own dense_scene: --models (the first value)
planted regressions of 1 / (M + 1) of its rows each and clutter, the start rows moved off inside the noise band by a
different amount per group, so the groups stop at different rounds; the labels are shuffled over the upload and live
on the device, and the timed calls ask for no labels.  grouped_round_ms, grouped_call_ms and loop_call_ms (per group a
host gather, upload, Context.refine_dense(max_rounds = R2) and the labels written back) as for --grouped above.  With
--groups 1 also refine_round_ms / refine_call_ms, Context.refine_dense on the same rows: the per-round difference is
the price of the (group, chunk) indirection, the whole-call difference the sort, the gather and the scatter.
lane_share = rows / (workgroups x chunk).

--model {absor,absor_w,pivot,ray}: Context.refine_rigid (lsqr_refine_rigid: absolute orientation, plain or with weighted
pairs, pivot calibration, ray intersection) on --n records (default 2 M here) of 6 / 7 / 13 / 6 doubles: four planted
models of 20 % each and 20 % clutter, shuffled; M = --models rows (default 4 and 64), every planted model M / 4 times
with its translation / pivot point / point moved by up to +-0.3, inside the noise band.  Two kinds alternate in one
process: refine_round_ms as above, and baseline_round_ms, the round the entry points allowed before: M x (lsqr_mask +
lsqr_set_mask + lsqr_ls_fit).  entry_ms = t(max_rounds = R1) - t(max_rounds = 0) - rounds done at R1 x refine_round_ms:
what a refine call costs once beside its rounds -- for absolute orientation the origin pre-pass (one more read of the
records); for the pivot and the ray, which have none, the same difference as a control."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lsqrrecipes_amd import _lib as L  # noqa: E402
from lsqrrecipes_amd import synth  # noqa: E402
from lsqrrecipes_amd.context import Context  # noqa: E402

DELTA = 0.5
HBM_PEAK = 8.0e12  # B/s


def scene(n, seed=20261019, box=1000.0, sigma=0.4):
    """-> points, the four planes as rows [n, a]"""
    g = np.random.default_rng(seed)
    m = n // 5
    parts, rows = [], []
    for _ in range(4):
        q, _r = np.linalg.qr(g.normal(size=(3, 3)))
        a = g.uniform(-box / 2, box / 2, 3)
        st = g.uniform(-box, box, (m, 2))
        parts.append(a + st[:, :1] * q[:, 0] + st[:, 1:] * q[:, 1] + g.normal(0.0, sigma, (m, 1)) * q[:, 2])
        rows.append(np.concatenate([q[:, 2], a]))
    parts.append(g.uniform(-box, box, (n - 4 * m, 3)))
    pts = np.concatenate(parts)
    return np.ascontiguousarray(pts[g.permutation(n)]), np.array(rows)


# --model: (the library's model, the generator of lsqrrecipes_amd.synth whose params are that model's rows)
SYNTH = {"plane": (L.PLANE, synth.plane), "line": (L.LINE, synth.line), "sphere": (L.SPHERE, synth.sphere),
         "line2d": (L.LINE2D, synth.plane)}


def synth_scene(n, model, dim, seed=20261021):
    """-> points, the four planted models as rows"""
    gen = SYNTH[model][1]
    m = n // 5
    parts, rows = [], []
    for j in range(4):
        pts, row, _ = gen(m, 0.0, seed=seed + 7 * j, dim=dim)
        parts.append(pts)
        rows.append(row)
    parts.append(gen(n - 4 * m, 1.0, seed=seed + 999, dim=dim)[0])
    pts = np.concatenate(parts)
    return np.ascontiguousarray(pts[np.random.default_rng(seed).permutation(n)]), np.array(rows)


def models(rows, m):
    """m rows: every plane m / 4 times, shifted along its normal by up to +-0.4 (inside the noise band)"""
    k = m // 4
    out = []
    for r in rows:
        for j in range(k):
            s = 0.0 if k == 1 else -0.4 + 0.8 * j / (k - 1)
            out.append(np.concatenate([r[:3], r[3:] + s * r[:3]]))
    return np.array(out)


def baseline_round(ctx, rows):
    """M x (lsqr_mask + lsqr_set_mask + lsqr_ls_fit) -> the refitted rows"""
    new = rows.copy()
    for m, r in enumerate(rows):
        mask, cnt = ctx.mask(r)
        if cnt < ctx.K:
            continue
        ctx.set_mask(mask)
        fit, _ = ctx.ls_fit(use_mask=True)
        if len(fit):
            new[m] = fit
    return new


def refine_rounds(ctx, rows, max_rounds, lm=False, nfev=None, dense=False, rigid=False):
    """lsqr_refine (lm: lsqr_refine_lm, dense: lsqr_refine_dense, rigid: lsqr_refine_rigid) without labels_out -> rounds
    done; nfev (a list): gets the models' lm_nfev"""
    import ctypes as C
    par = np.array(rows, dtype=np.float64, order="C")
    m = par.shape[0]
    fits = (L.FitInfo * m)()
    status = np.zeros(m, dtype=np.int32)
    rounds, conv = C.c_size_t(0), C.c_int(0)
    call = (ctx._lib.lsqr_refine_lm if lm else ctx._lib.lsqr_refine_dense if dense
            else ctx._lib.lsqr_refine_rigid if rigid else ctx._lib.lsqr_refine)
    ctx._chk(call(ctx._h, L.ptr(par), m, max_rounds, 0, None, None, fits, L.ptr(status), C.byref(rounds),
                  C.byref(conv)))
    if nfev is not None:
        nfev[:] = [int(f.lm_nfev) for f in fits]
    return int(rounds.value)


def sphere_models(rows, m):
    """m rows: every sphere m / 4 times, the radii up to +-0.4 apart (inside the noise band), the centres moved off"""
    k = m // 4
    out = []
    for r in rows:
        for j in range(k):
            s = 0.0 if k == 1 else -0.4 + 0.8 * j / (k - 1)
            out.append(np.concatenate([r[:3] + 0.05, [r[3] + s]]))
    return np.array(out)


def host_lm_round(ctx, rows):
    """Context.assign, then per model set_mask(labels == m) + ls_fit(use_mask=True) -> the refitted rows"""
    labels = ctx.assign(rows)["labels"]
    new = rows.copy()
    for m in range(len(rows)):
        mask = (labels == m).astype(np.uint8)
        if int(mask.sum()) < ctx.K:
            continue
        ctx.set_mask(mask)
        fit, _ = ctx.ls_fit(use_mask=True)
        if len(fit):
            new[m] = fit
    return new


def lm_main(a):
    r1, r2 = a.rounds
    ms = lambda v: [round(1e3 * float(f(v)), 4) for f in (np.median, np.min, np.max)]
    data, spheres = synth_scene(a.n, "sphere", 3)
    lines = []
    with Context(0) as ctx, Context(0) as alg:
        ctx.set_model(L.SPHERE, 3, DELTA, L.LS_GEOMETRIC).upload(data)
        alg.set_model(L.SPHERE, 3, DELTA, L.LS_ALGEBRAIC).upload(data)
        for m in a.models:
            rows = sphere_models(spheres, m)
            t_lo, t_hi, t_alo, t_ahi, t_host, done, nfev = [], [], [], [], [], None, []
            for rep in range(-1, a.reps):  # rep -1 warms every kind
                t0 = time.perf_counter()
                lo = refine_rounds(ctx, rows, r1, lm=True)
                t1 = time.perf_counter()
                hi = refine_rounds(ctx, rows, r2, lm=True, nfev=nfev)
                t2 = time.perf_counter()
                if rep < a.baseline_reps:
                    host_lm_round(ctx, rows)
                t3 = time.perf_counter()
                alo = refine_rounds(alg, rows, r1)
                t4 = time.perf_counter()
                ahi = refine_rounds(alg, rows, r2)
                t5 = time.perf_counter()
                if hi <= lo or ahi <= alo:
                    raise SystemExit("converged after %d / %d rounds: nothing to time" % (hi, ahi))
                if done is not None and done != (lo, hi, alo, ahi):
                    raise SystemExit("the rounds done differ between repetitions")
                done = (lo, hi, alo, ahi)
                if rep >= 0:
                    t_lo.append(t1 - t0)
                    t_hi.append(t2 - t1)
                    if rep < a.baseline_reps:
                        t_host.append(t3 - t2)
                    t_alo.append(t4 - t3)
                    t_ahi.append(t5 - t4)
            per = [(h - l) / (done[1] - done[0]) for h, l in zip(t_hi, t_lo)]
            aper = [(h - l) / (done[3] - done[2]) for h, l in zip(t_ahi, t_alo)]
            rnd = float(np.median(per))
            row = dict(model="sphere", ls="geometric", dim=3, n=a.n, models=m, reps=a.reps, rounds_done=list(done[:2]),
                       alg_rounds_done=list(done[2:]), lm_nfev=[min(nfev), max(nfev)], refine_lm_round_ms=ms(per),
                       refine_lm_call_ms=ms(t_hi), host_round_ms=ms(t_host), host_reps=len(t_host),
                       alg_refine_round_ms=ms(aper), ratio_host=round(float(np.median(t_host)) / rnd, 1),
                       ratio_alg=round(rnd / float(np.median(aper)), 2),
                       passes_per_s=round((1 + max(nfev)) / rnd, 1))
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


DENSE_SIGMA = 0.01


def dense_scene(n, dim, m, seed=20261023):
    """-> rows (a | b) shuffled, the start regressions: m planted ones of n / (m + 1) rows each, the rest clutter"""
    g = np.random.default_rng([seed, dim, m])
    x = g.normal(size=(m, dim))
    rows = np.empty((n, dim + 1))
    rows[:, :dim] = g.normal(size=(n, dim))
    owner = np.arange(n) % (m + 1)  # m: clutter
    on = owner < m
    rows[:, dim] = np.einsum("ij,ij->i", rows[:, :dim], x[np.minimum(owner, m - 1)]) + DENSE_SIGMA * g.normal(size=n)
    rows[~on, dim] = g.uniform(-10.0, 10.0, int((~on).sum()))
    start = x + DENSE_SIGMA / np.sqrt(dim) * g.normal(size=x.shape)
    return np.ascontiguousarray(rows[g.permutation(n)]), start


def dense_main(a):
    r1, r2 = a.rounds
    ms = lambda v: [round(1e3 * float(f(v)), 4) for f in (np.median, np.min, np.max)]
    lines = []
    dim = a.dim
    with Context(0) as ctx:
        for m in a.models:
            data, rows = dense_scene(a.n, dim, m)
            ctx.set_model(L.DENSE, dim, 4 * DENSE_SIGMA).upload(data)
            t_lo, t_hi, t_asg, t_base, done = [], [], [], [], None
            for rep in range(-1, a.reps):  # rep -1 warms every kind
                t0 = time.perf_counter()
                asg = ctx.assign_dense(rows)
                t1 = time.perf_counter()
                lo = refine_rounds(ctx, rows, r1, dense=True)
                t2 = time.perf_counter()
                hi = refine_rounds(ctx, rows, r2, dense=True)
                t3 = time.perf_counter()
                if rep < a.baseline_reps:
                    baseline_round(ctx, rows)
                t4 = time.perf_counter()
                if hi <= lo:
                    raise SystemExit("converged after %d rounds: nothing to time" % hi)
                if done is not None and done != (lo, hi):
                    raise SystemExit("the rounds done differ between repetitions")
                done = (lo, hi)
                if rep >= 0:
                    t_asg.append(t1 - t0)
                    t_lo.append(t2 - t1)
                    t_hi.append(t3 - t2)
                    if rep < a.baseline_reps:
                        t_base.append(t4 - t3)
            per = [(h - l) / (done[1] - done[0]) for h, l in zip(t_hi, t_lo)]
            rnd = float(np.median(per))
            chunk = L.assign_dense_chunk(dim)
            ps = ((dim + 1) * (dim + 2) // 2 + 1 + 7) & ~7
            row = dict(model="dense", dim=dim, n=a.n, models=m, reps=a.reps, rounds_done=list(done),
                       counts_assigned=int(a.n - asg["counts"][-1]), refine_round_ms=ms(per), assign_call_ms=ms(t_asg),
                       baseline_round_ms=ms(t_base), baseline_reps=len(t_base),
                       ratio=round(float(np.median(t_base)) / rnd, 2), rows_read_per_round=dict(refine=1, baseline=2 * m),
                       chunk=chunk, partial_bytes=int((a.n + chunk - 1) // chunk * m * ps * 8),
                       record_bytes_per_s=round(a.n * 8 * (dim + 1) / rnd, 0),
                       hbm_fraction=round(a.n * 8 * (dim + 1) / rnd / HBM_PEAK, 4))
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


# --model: (the library's model, ls_type, delta, doubles per record, the chunk of the pass)
RIGID = {"absor": (L.ABSOR, 0, 2.0, 6, 2048), "absor_w": (L.ABSOR, 2, 2.0, 7, 2048), "pivot": (L.PIVOT, 0, 1.0, 13, 1024),
         "ray": (L.RAY, 0, 2.0, 6, 2048)}


def _rotations(g, n):
    """n random rotation matrices (n, 3, 3) from unit quaternions"""
    q = g.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    s, x, y, z = q.T
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - s * z), 2 * (x * z + s * y)],
                  [2 * (x * y + s * z), 1 - 2 * (x * x + z * z), 2 * (y * z - s * x)],
                  [2 * (x * z - s * y), 2 * (y * z + s * x), 1 - 2 * (x * x + y * y)]])
    return np.moveaxis(R, 2, 0), q


def rigid_scene(n, kind, seed=20261025):
    """-> records (shuffled), the four planted models as rows: 20 % of the records each, the rest clutter"""
    g = np.random.default_rng([seed, sorted(RIGID).index(kind)])
    owner = np.arange(n) % 5  # 4: clutter
    jj = np.minimum(owner, 3)
    off = owner == 4
    if kind in ("absor", "absor_w"):
        R, q = _rotations(g, 4)
        t = g.uniform(-1000.0, 1000.0, (4, 3))
        first = g.uniform(-100.0, 100.0, (n, 3))
        second = np.einsum("nij,nj->ni", R[jj], first) + t[jj] + g.normal(0.0, 0.5, (n, 3))
        second[off] = g.uniform(-1500.0, 1500.0, (int(off.sum()), 3))
        cols = [first, second] + ([g.uniform(0.25, 4.0, (n, 1))] if kind == "absor_w" else [])
        rec, rows = np.hstack(cols), np.hstack([q, t])
    elif kind == "ray":
        target = g.uniform(-1000.0, 1000.0, (4, 3))
        p = g.uniform(-1000.0, 1000.0, (n, 3))
        aim = target[jj] + g.normal(0.0, 0.3, (n, 3))
        aim[off] = g.uniform(-1000.0, 1000.0, (int(off.sum()), 3))
        d = aim - p
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        rec, rows = np.hstack([p, d]), target
    else:
        tip = np.array([-17.0, 1.0, -157.0])
        piv = g.uniform(-1000.0, 1000.0, (4, 3))
        R, _ = _rotations(g, n)
        t = piv[jj] - R @ tip + g.normal(0.0, 0.15, (n, 3))
        t[off] += g.uniform(-400.0, 400.0, (int(off.sum()), 3))
        rec = np.zeros((n, 13))
        rec[:, :9], rec[:, 9:12] = R.reshape(n, 9), t
        rows = np.hstack([np.tile(tip, (4, 1)), piv])
    return np.ascontiguousarray(rec[g.permutation(n)]), rows


def rigid_models(rows, m):
    """m rows: every planted model m / 4 times, its last three slots moved by up to +-0.3 (inside the noise band)"""
    k = m // 4
    out = []
    for r in rows:
        for j in range(k):
            s = 0.05 if k == 1 else -0.3 + 0.6 * j / (k - 1)
            out.append(np.concatenate([r[:-3], r[-3:] + s]))
    return np.array(out)


def rigid_main(a):
    r1, r2 = a.rounds
    ms = lambda v: [round(1e3 * float(f(v)), 4) for f in (np.median, np.min, np.max)]
    model, ls, delta, width, chunk = RIGID[a.model]
    data, planted = rigid_scene(a.n, a.model)
    lines = []
    with Context(0) as ctx:
        ctx.set_model(model, 3, delta, ls, aux=0.017453292519943295 if a.model == "ray" else 0.0).upload(data)
        for m in a.models:
            rows = rigid_models(planted, m)
            t_0, t_lo, t_hi, t_asg, t_base, done = [], [], [], [], [], None
            for rep in range(-1, a.reps):  # rep -1 warms every kind
                t0 = time.perf_counter()
                asg = ctx.assign_rigid(rows)
                t1 = time.perf_counter()
                refine_rounds(ctx, rows, 0, rigid=True)
                t2 = time.perf_counter()
                lo = refine_rounds(ctx, rows, r1, rigid=True)
                t3 = time.perf_counter()
                hi = refine_rounds(ctx, rows, r2, rigid=True)
                t4 = time.perf_counter()
                if rep < a.baseline_reps:
                    baseline_round(ctx, rows)
                t5 = time.perf_counter()
                if hi <= lo:
                    raise SystemExit("converged after %d rounds: nothing to time" % hi)
                if done is not None and done != (lo, hi):
                    raise SystemExit("the rounds done differ between repetitions")
                done = (lo, hi)
                if rep >= 0:
                    t_asg.append(t1 - t0)
                    t_0.append(t2 - t1)
                    t_lo.append(t3 - t2)
                    t_hi.append(t4 - t3)
                    if rep < a.baseline_reps:
                        t_base.append(t5 - t4)
            per = [(h - l) / (done[1] - done[0]) for h, l in zip(t_hi, t_lo)]
            rnd = float(np.median(per))
            entry = [l - z - done[0] * rnd for l, z in zip(t_lo, t_0)]
            row = dict(model=a.model, n=a.n, models=m, reps=a.reps, rounds_done=list(done),
                       counts_assigned=int(a.n - asg["counts"][-1]), refine_round_ms=ms(per), assign_call_ms=ms(t_asg),
                       call0_ms=ms(t_0), entry_ms=ms(entry), baseline_round_ms=ms(t_base), baseline_reps=len(t_base),
                       ratio=round(float(np.median(t_base)) / rnd, 1), record_bytes=8 * width, chunk=chunk,
                       workgroups=(a.n + chunk - 1) // chunk, record_bytes_per_s=round(a.n * 8 * width / rnd, 0),
                       hbm_fraction=round(a.n * 8 * width / rnd / HBM_PEAK, 4))
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def dense_grouped_scene(n, n_groups, dim, m, seed=20261024):
    """-> rows (a | b) shuffled, labels, start rows (n_groups, m, dim): every group a dense_scene of n / n_groups rows"""
    g = np.random.default_rng([seed, dim, m, n_groups])
    per = n // n_groups
    x = g.normal(size=(n_groups, m, dim))
    grp = np.repeat(np.arange(n_groups, dtype=np.int32), per)
    owner = np.tile(np.arange(per) % (m + 1), n_groups)  # m: clutter
    on = owner < m
    rows = np.empty((grp.size, dim + 1))
    rows[:, :dim] = g.normal(size=(grp.size, dim))
    rows[:, dim] = (np.einsum("ij,ij->i", rows[:, :dim], x[grp, np.minimum(owner, m - 1)])
                    + DENSE_SIGMA * g.normal(size=grp.size))
    rows[~on, dim] = g.uniform(-10.0, 10.0, int((~on).sum()))
    size = g.uniform(0.5, 2.0, (n_groups, 1, 1))  # per group its own distance from the planted rows
    start = x + size * DENSE_SIGMA / np.sqrt(dim) * g.normal(size=x.shape)
    perm = g.permutation(grp.size)
    return np.ascontiguousarray(rows[perm]), np.ascontiguousarray(grp[perm]), np.ascontiguousarray(start)


def dense_grouped_main(a):
    r1, r2 = a.rounds
    ms = lambda v: [round(1e3 * float(f(v)), 4) for f in (np.median, np.min, np.max)]
    dim, n_groups, k = a.dim, a.groups, a.models[0]
    data, grp, rows = dense_grouped_scene(a.n, n_groups, dim, k)
    n = data.shape[0]
    sizes = np.bincount(grp, minlength=n_groups)
    order = np.argsort(grp, kind="stable")
    first = np.concatenate([[0], np.cumsum(sizes)])
    loop_groups = min(n_groups, a.loop_groups)
    with Context(0) as ctx, Context(0) as one:
        ctx.set_model(L.DENSE, dim, 4 * DENSE_SIGMA).upload(data)
        one.set_model(L.DENSE, dim, 4 * DENSE_SIGMA)
        dev = DeviceArray(grp)
        t_lo, t_hi, t_loop, t_ref_lo, t_ref_hi, done, ref_done = [], [], [], [], [], None, None
        for rep in range(-1, a.reps):  # rep -1 warms every kind
            t0 = time.perf_counter()
            lo = ctx.refine_dense_grouped(dev, n_groups, rows, max_rounds=r1)
            t1 = time.perf_counter()
            hi = ctx.refine_dense_grouped(dev, n_groups, rows, max_rounds=r2)
            t2 = time.perf_counter()
            if rep < a.baseline_reps:  # the only route without the call, on the first groups
                labels = np.full(n, -1, dtype=np.int32)
                for g in range(loop_groups):
                    at = order[first[g]:first[g + 1]]
                    one.upload(np.ascontiguousarray(data[at]))
                    labels[at] = one.refine_dense(rows[g], max_rounds=r2)["labels"]
            t3 = time.perf_counter()
            if n_groups == 1:
                ref = (refine_rounds(ctx, rows[0], r1, dense=True), None)
                t4 = time.perf_counter()
                ref = (ref[0], refine_rounds(ctx, rows[0], r2, dense=True))
                t5 = time.perf_counter()
                ref_done = ref
            work = (int((sizes * lo["rounds"]).sum()), int((sizes * hi["rounds"]).sum()))
            if work[1] <= work[0]:
                raise SystemExit("every group has stopped after %d rounds: nothing to time" % r1)
            if done is not None and done != work:
                raise SystemExit("the rounds done differ between repetitions")
            done = work
            if rep >= 0:
                t_lo.append(t1 - t0)
                t_hi.append(t2 - t1)
                if rep < a.baseline_reps:
                    t_loop.append((t3 - t2) * n_groups / loop_groups)
                if n_groups == 1:
                    t_ref_lo.append(t4 - t3)
                    t_ref_hi.append(t5 - t4)
        dev.free()
    per = [(h - l) / (done[1] - done[0]) * n for h, l in zip(t_hi, t_lo)]
    rnd = float(np.median(per))
    chunk = L.assign_dense_chunk(dim)
    wgs = int(np.sum((sizes[sizes > 0] + chunk - 1) // chunk))
    ps = ((dim + 1) * (dim + 2) // 2 + 1 + 7) & ~7
    row = dict(model="dense", grouped=True, dim=dim, n=n, groups=n_groups, models=k, reps=a.reps, rounds=[r1, r2],
               record_rounds_done=list(done), rounds_hist=np.bincount(hi["rounds"]).tolist(),
               converged=int(hi["converged"].sum()), route_hist=np.bincount(hi["route"].ravel()).tolist(),
               grouped_round_ms=ms(per), grouped_call_ms=ms(t_hi), chunk=chunk, workgroups=wgs,
               lane_share=round(n / (wgs * float(chunk)), 4), partial_bytes=int(wgs * k * ps * 8),
               hbm_fraction=round(n * 8 * (dim + 1) / rnd / HBM_PEAK, 4))
    if t_loop:
        row.update(loop_call_ms=ms(t_loop), loop_groups_timed=loop_groups, loop_scaled_by=n_groups / loop_groups,
                   loop_reps=len(t_loop), ratio_call=round(float(np.median(t_loop) / np.median(t_hi)), 1))
    if n_groups == 1:
        row["refine_round_ms"] = ms([(h - l) / (ref_done[1] - ref_done[0]) for h, l in zip(t_ref_hi, t_ref_lo)])
        row["refine_call_ms"] = ms(t_ref_hi)
        row["refine_rounds_done"] = list(ref_done)
    line = json.dumps(row)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


class DeviceArray:
    """a device allocation of the HIP runtime the library runs on, with the tensor attributes Context looks at"""

    def __init__(self, host):
        import ctypes as C
        L.load()
        path = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln][0]
        self._hip, self._C = C.CDLL(path), C
        self.host = np.ascontiguousarray(host)
        self.dtype, self.is_cuda = str(self.host.dtype), True
        self.ptr = C.c_void_p()
        assert self._hip.hipMalloc(C.byref(self.ptr), C.c_size_t(self.host.nbytes)) == 0
        assert self._hip.hipMemcpy(self.ptr, C.c_void_p(self.host.ctypes.data), C.c_size_t(self.host.nbytes), 1) == 0

    def free(self):
        self._hip.hipFree(self.ptr)

    def data_ptr(self):
        return self.ptr.value

    def is_contiguous(self):
        return True

    def numel(self):
        return self.host.size


def grouped_scene(n, n_groups, k, seed=20261020, box=1000.0, sigma=0.4):
    """-> points (shuffled), labels, start rows (n_groups, k, 6): every group k planes of 1 / (k + 1) of its records each"""
    g = np.random.default_rng(seed)
    per = n // n_groups
    nrm = g.normal(size=(n_groups, k, 3))
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    u = np.cross(nrm, np.roll(nrm, 1, axis=2) + 0.5)
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    v = np.cross(nrm, u)
    a = g.uniform(-box / 2, box / 2, (n_groups, k, 3))
    grp = np.repeat(np.arange(n_groups, dtype=np.int32), per)
    j = np.tile(np.arange(per) % (k + 1), n_groups)  # model of the record; k: clutter
    on = j < k
    jj = np.minimum(j, k - 1)
    st = g.uniform(-box, box, (grp.size, 2))
    pts = (a[grp, jj] + st[:, :1] * u[grp, jj] + st[:, 1:] * v[grp, jj]
           + g.normal(0.0, sigma, (grp.size, 1)) * nrm[grp, jj])
    pts[~on] = g.uniform(-box, box, (int((~on).sum()), 3))
    # the start: the normal turned by up to 3e-4, the point moved by up to 0.3 along the normal, per group its own size
    size = g.uniform(0.2, 1.0, (n_groups, 1, 1))
    n0 = nrm + 3e-4 * size * g.normal(size=nrm.shape)
    n0 /= np.linalg.norm(n0, axis=2, keepdims=True)
    rows = np.concatenate([n0, a + 0.3 * size * g.normal(size=(n_groups, k, 1)) * nrm], axis=2)
    perm = g.permutation(grp.size)
    return np.ascontiguousarray(pts[perm]), np.ascontiguousarray(grp[perm]), np.ascontiguousarray(rows)


def grouped_sphere_scene(n_groups, k=3, seed=20261022, box=1000.0, sigma=0.1):
    """-> points (shuffled), labels, start rows (n_groups, k, 4): group g has sizes[g] in 300 .. 3 000 records, k
    spheres of 1 / (k + 1) of them each, the rest clutter"""
    g = np.random.default_rng(seed)
    sizes = g.integers(300, 3001, n_groups)
    grp = np.repeat(np.arange(n_groups, dtype=np.int32), sizes)
    first = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    j = (np.arange(grp.size) - first[grp]) % (k + 1)  # model of the record; k: clutter
    on = j < k
    jj = np.minimum(j, k - 1)
    c = g.uniform(-box / 2, box / 2, (n_groups, k, 3))
    r = g.uniform(50.0, 300.0, (n_groups, k))
    u = g.normal(size=(grp.size, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    pts = c[grp, jj] + r[grp, jj][:, None] * u + g.normal(0.0, sigma, (grp.size, 3))
    pts[~on] = g.uniform(-box, box, (int((~on).sum()), 3))
    size = g.uniform(0.2, 1.0, (n_groups, 1, 1))
    rows = np.concatenate([c + 0.05 * size * g.choice([-1.0, 1.0], (n_groups, k, 3)), r[:, :, None] + 0.1 * size], axis=2)
    perm = g.permutation(grp.size)
    return np.ascontiguousarray(pts[perm]), np.ascontiguousarray(grp[perm]), np.ascontiguousarray(rows)


def grouped_lm_main(a):
    r2 = a.rounds[1]
    ms = lambda v: [round(1e3 * float(f(v)), 4) for f in (np.median, np.min, np.max)]
    n_groups, k = a.groups, 3
    data, grp, rows = grouped_sphere_scene(n_groups, k)
    n = data.shape[0]
    sizes = np.bincount(grp, minlength=n_groups)
    order = np.argsort(grp, kind="stable")
    first = np.concatenate([[0], np.cumsum(sizes)])
    loop_groups = min(n_groups, a.loop_groups)
    with Context(0) as ctx, Context(0) as one:
        ctx.set_model(L.SPHERE, 3, DELTA, L.LS_GEOMETRIC).upload(data)
        one.set_model(L.SPHERE, 3, DELTA, L.LS_GEOMETRIC)
        dev = DeviceArray(grp)
        t_0, t_1, t_hi, t_loop, done = [], [], [], [], None
        for rep in range(-1, a.reps):  # rep -1 warms every kind
            t0 = time.perf_counter()
            ctx.refine_lm_grouped(dev, n_groups, rows, max_rounds=0)
            t1 = time.perf_counter()
            lo = ctx.refine_lm_grouped(dev, n_groups, rows, max_rounds=1)
            t2 = time.perf_counter()
            hi = ctx.refine_lm_grouped(dev, n_groups, rows, max_rounds=r2)
            t3 = time.perf_counter()
            if rep < a.baseline_reps:  # what a caller must do without the call, on the first groups
                labels = np.full(n, -1, dtype=np.int32)
                for g in range(loop_groups):
                    at = order[first[g]:first[g + 1]]
                    one.upload(np.ascontiguousarray(data[at]))
                    labels[at] = one.refine_lm(rows[g], max_rounds=r2)["labels"]
            t4 = time.perf_counter()
            work = (int(lo["rounds"].sum()), int(hi["rounds"].sum()))
            if done is not None and done != work:
                raise SystemExit("the rounds done differ between repetitions")
            done = work
            if rep >= 0:
                t_0.append(t1 - t0)
                t_1.append(t2 - t1)
                t_hi.append(t3 - t2)
                if rep < a.baseline_reps:
                    t_loop.append((t4 - t3) * n_groups / loop_groups)
        dev.free()
        # round 1: its evaluations, and the workgroups that hold no record of a model still live
        evals = int(lo["lm_nfev"].max())
        lab0 = ctx.assign_grouped(grp, n_groups, rows)["labels"]
        pos = np.empty(n, dtype=np.int64)
        pos[order] = np.arange(n) - first[grp[order]]
        chunk_first = np.concatenate([[0], np.cumsum((sizes + 2047) // 2048)])
        wg = chunk_first[grp] + pos // 2048
        wg_nfev = np.zeros(int(chunk_first[-1]), dtype=np.int64)
        has = lab0 >= 0
        np.maximum.at(wg_nfev, wg[has], lo["lm_nfev"][grp[has], lab0[has]])
        idle = [round(float(np.mean(wg_nfev < j)), 4) for j in range(1, evals + 1)]
    round1 = [b - c for b, c in zip(t_1, t_0)]
    row = dict(model="sphere", ls="geometric", dim=3, n=n, groups=n_groups, models=k, reps=a.reps, rounds=[0, 1, r2],
               rounds_hist=np.bincount(hi["rounds"]).tolist(), converged=int(hi["converged"].sum()),
               lm_ok=int(((hi["lm_info"] >= 1) & (hi["lm_info"] <= 4)).sum()), call0_ms=ms(t_0), call1_ms=ms(t_1),
               grouped_call_ms=ms(t_hi), round1_ms=ms(round1), evaluations=evals,
               lm_nfev_hist=np.bincount(lo["lm_nfev"].ravel()).tolist(),
               eval_ms_upper=round(1e3 * float(np.median(round1)) / max(evals, 1), 4),
               workgroups=int(chunk_first[-1]), idle_share=idle)
    if t_loop:
        row.update(loop_call_ms=ms(t_loop), loop_groups_timed=loop_groups, loop_scaled_by=n_groups / loop_groups,
                   loop_reps=len(t_loop), ratio_call=round(float(np.median(t_loop) / np.median(t_hi)), 1))
    line = json.dumps(row)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def grouped_main(a):
    r1, r2 = a.rounds
    ms = lambda v: [round(1e3 * float(f(v)), 4) for f in (np.median, np.min, np.max)]
    lines = []
    for name, n_groups, k in (("a", 1, 4), ("b", 1000, 4), ("c", 50000, 3)):
        if name not in a.splits:
            continue
        if a.synth:  # one group: the ungrouped scene and rows
            data, rows = synth_scene(a.n, a.model, a.dim)
            grp, rows = np.zeros(a.n, dtype=np.int32), rows[None]
        else:
            data, grp, rows = grouped_scene(a.n, n_groups, k)
        n = data.shape[0]
        sizes = np.bincount(grp, minlength=n_groups)
        order = np.argsort(grp, kind="stable")
        first = np.concatenate([[0], np.cumsum(sizes)])
        loop_groups = min(n_groups, a.loop_groups)
        with Context(0) as ctx, Context(0) as one:
            ctx.set_model(a.model_id, a.dim, DELTA, L.LS_ALGEBRAIC).upload(data)
            one.set_model(a.model_id, a.dim, DELTA, L.LS_ALGEBRAIC)
            dev = DeviceArray(grp)
            t_lo, t_hi, t_loop, t_ref_lo, t_ref_hi, done, ref_done = [], [], [], [], [], None, None
            for rep in range(-1, a.reps):  # rep -1 warms every kind
                t0 = time.perf_counter()
                lo = ctx.refine_grouped(dev, n_groups, rows, max_rounds=r1)
                t1 = time.perf_counter()
                hi = ctx.refine_grouped(dev, n_groups, rows, max_rounds=r2)
                t2 = time.perf_counter()
                if rep < a.baseline_reps:  # the parent's route on the first groups
                    labels = np.full(n, -1, dtype=np.int32)
                    for g in range(loop_groups):
                        at = order[first[g]:first[g + 1]]
                        one.upload(np.ascontiguousarray(data[at]))
                        labels[at] = one.refine(rows[g], max_rounds=r2)["labels"]
                t3 = time.perf_counter()
                if n_groups == 1:
                    ref = (refine_rounds(ctx, rows[0], r1), None)
                    t4 = time.perf_counter()
                    ref = (ref[0], refine_rounds(ctx, rows[0], r2))
                    t5 = time.perf_counter()
                    ref_done = ref
                work = (int((sizes * lo["rounds"]).sum()), int((sizes * hi["rounds"]).sum()))
                if work[1] <= work[0]:
                    raise SystemExit("every group has stopped after %d rounds: nothing to time" % r1)
                if done is not None and done != work:
                    raise SystemExit("the rounds done differ between repetitions")
                done = work
                if rep >= 0:
                    t_lo.append(t1 - t0)
                    t_hi.append(t2 - t1)
                    if rep < a.baseline_reps:
                        t_loop.append((t3 - t2) * n_groups / loop_groups)
                    if n_groups == 1:
                        t_ref_lo.append(t4 - t3)
                        t_ref_hi.append(t5 - t4)
            dev.free()
            per = [(h - l) / (done[1] - done[0]) * n for h, l in zip(t_hi, t_lo)]
            rnd = float(np.median(per))
            wgs = int(np.sum((sizes[sizes > 0] + 2047) // 2048))
            row = dict(split=name, model=a.model, dim=a.dim, n=n, groups=n_groups, models=k, reps=a.reps, rounds=[r1, r2],
                       record_rounds_done=list(done), rounds_hist=np.bincount(hi["rounds"]).tolist(),
                       converged=int(hi["converged"].sum()), grouped_round_ms=ms(per), grouped_call_ms=ms(t_hi),
                       workgroups=wgs, lane_share=round(n / (wgs * 2048.0), 4),
                       hbm_fraction=round(n * 8 * a.dim / rnd / HBM_PEAK, 4))
            if t_loop:
                row.update(loop_call_ms=ms(t_loop), loop_groups_timed=loop_groups,
                           loop_scaled_by=n_groups / loop_groups, loop_reps=len(t_loop),
                           ratio_call=round(float(np.median(t_loop) / np.median(t_hi)), 1))
            if n_groups == 1:
                row["refine_round_ms"] = ms([(h - l) / (ref_done[1] - ref_done[0]) for h, l in zip(t_ref_hi, t_ref_lo)])
                row["refine_call_ms"] = ms(t_ref_hi)
                row["refine_rounds_done"] = list(ref_done)
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--models", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, nargs=2, default=[1, 5], metavar=("R1", "R2"))
    ap.add_argument("--baseline-reps", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--grouped", action="store_true", help="time Context.refine_grouped instead (see above)")
    ap.add_argument("--splits", nargs="+", default=["a", "b", "c"], choices=["a", "b", "c"])
    ap.add_argument("--loop-groups", type=int, default=200, help="--grouped: groups the per-group loop is timed on")
    ap.add_argument("--model", choices=sorted(SYNTH) + ["dense"] + sorted(RIGID), default="plane")
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--lm", action="store_true", help="time Context.refine_lm on the sphere scene instead (see above)")
    ap.add_argument("--groups", type=int, default=3000, help="--grouped --lm, --model dense --grouped: the groups of the scene")
    a = ap.parse_args()
    if a.model in RIGID:
        if a.lm or a.grouped:
            raise SystemExit("--model %s goes with neither --lm nor --grouped" % a.model)
        a.n = 2_000_000 if a.n == 10_000_000 else a.n
        a.models = [4, 64] if a.models == [4, 16, 64] else a.models
        return rigid_main(a)
    if a.lm and a.grouped:
        return grouped_lm_main(a)
    if a.lm:
        a.models = [4, 64] if a.models == [4, 16, 64] else a.models
        return lm_main(a)
    if a.model == "dense":
        if a.lm:
            raise SystemExit("--model dense does not go with --lm")
        a.n = 1_000_000 if a.n == 10_000_000 else a.n
        if a.grouped:
            a.models = [4] if a.models == [4, 16, 64] else a.models
            return dense_grouped_main(a)
        a.models = [4, 16] if a.models == [4, 16, 64] else a.models
        return dense_main(a)
    a.model_id = SYNTH[a.model][0]
    a.synth = (a.model, a.dim) != ("plane", 3)  # the default scene is this tool's own
    if a.synth:
        a.dim = 2 if a.model == "line2d" else a.dim
        a.models, a.splits = [4], ["a"]
    if a.grouped:
        return grouped_main(a)
    data, planes = synth_scene(a.n, a.model, a.dim) if a.synth else scene(a.n)
    r1, r2 = a.rounds
    lines = []
    with Context(0) as ctx:
        ctx.set_model(a.model_id, a.dim, DELTA, L.LS_ALGEBRAIC).upload(data)
        for m in a.models:
            rows = planes if a.synth else models(planes, m)
            t_lo, t_hi, t_asg, t_base, done = [], [], [], [], None
            for rep in range(-1, a.reps):  # rep -1 warms every kind
                t0 = time.perf_counter()
                asg = ctx.assign(rows)
                t1 = time.perf_counter()
                lo = refine_rounds(ctx, rows, r1)
                t2 = time.perf_counter()
                hi = refine_rounds(ctx, rows, r2)
                t3 = time.perf_counter()
                if rep < a.baseline_reps:
                    baseline_round(ctx, rows)
                t4 = time.perf_counter()
                if hi <= lo:
                    raise SystemExit("converged after %d rounds: nothing to time" % hi)
                if done is not None and done != (lo, hi):
                    raise SystemExit("the rounds done differ between repetitions")
                done = (lo, hi)
                if rep >= 0:
                    t_asg.append(t1 - t0)
                    t_lo.append(t2 - t1)
                    t_hi.append(t3 - t2)
                    if rep < a.baseline_reps:
                        t_base.append(t4 - t3)
            per = [(h - l) / (done[1] - done[0]) for h, l in zip(t_hi, t_lo)]
            ms = lambda v: [round(1e3 * float(f(v)), 4) for f in (np.median, np.min, np.max)]
            rnd = float(np.median(per))
            row = dict(model=a.model, dim=a.dim, n=a.n, models=m, reps=a.reps, rounds_done=list(done), counts_assigned=int(a.n - asg["counts"][-1]),
                       refine_round_ms=ms(per), assign_call_ms=ms(t_asg), baseline_round_ms=ms(t_base),
                       baseline_reps=len(t_base), ratio=round(float(np.median(t_base)) / rnd, 1),
                       record_bytes_per_s=round(a.n * 8 * a.dim / rnd, 0),
                       hbm_fraction=round(a.n * 8 * a.dim / rnd / HBM_PEAK, 4))
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
