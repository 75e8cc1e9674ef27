"""Context.ransac_many (lsqr_ransac_many) against the per-problem Context.ransac loop on the same problems.

Shapes (the loop is timed on the first --loop problems and extrapolated when the set is larger; the output says so):
  plane  3-D  10 000 problems x  1 000 records, 50 % inliers
  sphere 3-D   1 000 problems x 10 000 records (algebraic), 50 % inliers
  line   3-D 100 000 problems x    100 records, 50 % inliers
and the single-call latency of Context.ransac (upload + compute) at N = 100 / 1 000 / 10 000.  --shapes picks the
shapes (default: the three above); the closed-form estimators' shapes (--shapes rigid: all four; the latency rows
are skipped when no point shape is listed):
  rays       100 000 problems x     12 rays,   70 % inliers, 1 degree minimum angle
  absor       10 000 problems x     20 pairs,  70 % inliers (unweighted)
  pivot        1 000 problems x    300 frames, 70 % inliers
  line2d     100 000 problems x    200 points, 50 % inliers
and the geometric (Levenberg-Marquardt) sphere, Context.ransac_many_lm against the loop on a geometric context
(--shapes geometric: both):
  sphere_lm         1 000 problems x 10 000 records, 50 % inliers
  sphere_lm_small  10 000 problems x    300 records, 50 % inliers
and the dense linear system (robust linear regression), Context.ransac_many_dense against the loop on a dense
context (--shapes dense: all three; delta 0.1, 1e-3 relative noise on b, outliers' b scaled by 20 as synth.dense):
  dense6   n =  6  10 000 problems x    500 rows, 20 % outliers
  dense16  n = 16   1 000 problems x  5 000 rows, 10 % outliers
  dense64  n = 64     100 problems x 20 000 rows,  3 % outliers
and the exhaustive search, Context.ransac_many_exhaustive against the Context.ransac_exhaustive loop, with the fused
path on (many_ms, the default) and off (general_ms: every problem through the rounds):
  python tools/many_time.py --shapes exhaustive
  ex_rays     100 000 problems x  12 rays,        C(12,2) =     66 subsets each
  ex_absor     10 000 problems x  20 point pairs, C(20,3) =  1 140
  ex_plane     10 000 problems x  40 points,      C(40,3) =  9 880
  ex_plane300     100 problems x 300 points,      C(300,3) = 4 455 100 (N > 256: the general path in both settings)
Each row also gives the loop's time per problem (loop_ms_per_problem).  Every timed call
ends in a device synchronisation (both entry points return host results); each shape is warmed first; the two
paths alternate in one process.  --quick: one repetition, small loop (for a kernel-trace run under rocprofv3).
One JSON line per shape and size on stdout; --out FILE also writes them all to FILE."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lsqrrecipes_amd import _lib as L  # noqa: E402
from lsqrrecipes_amd.context import Context  # noqa: E402


def gen(model, n_prob, n_rec, inl, seed):
    """(records (n_prob * n_rec, 3), offsets): one random plane / sphere / line per problem, sigma 0.2 inliers,
    uniform outliers in the problem's 200-unit box"""
    g = np.random.default_rng(seed)
    P, N = n_prob, n_rec
    c = g.uniform(-500, 500, (P, 1, 3))
    out = c + g.uniform(-100, 100, (P, N, 3))
    if model == L.PLANE:
        u, v = g.normal(size=(P, 1, 3)), g.normal(size=(P, 1, 3))
        pts = c + g.uniform(-100, 100, (P, N, 1)) * u + g.uniform(-100, 100, (P, N, 1)) * v
    elif model == L.SPHERE:
        d = g.normal(size=(P, N, 3))
        pts = c + g.uniform(20, 80, (P, 1, 1)) * d / np.linalg.norm(d, axis=2, keepdims=True)
    else:
        u = g.normal(size=(P, 1, 3))
        pts = c + g.uniform(-100, 100, (P, N, 1)) * u / np.linalg.norm(u, axis=2, keepdims=True)
    pts = pts + g.normal(0, 0.2, pts.shape)
    is_out = g.random((P, N)) >= inl
    pts[is_out] = out[is_out]
    offs = np.arange(P + 1, dtype=np.uint64) * N
    return np.ascontiguousarray(pts.reshape(-1, 3)), offs


def gen_dense(n, n_prob, n_rec, inl, seed):
    """(rows (n_prob * n_rec, n + 1), offsets): one random x per problem, a uniform in [-1, 1]^n, b = a.x with 1e-3
    relative noise, the outliers' b scaled by 20 (synth.dense's model)"""
    g = np.random.default_rng(seed)
    rows = np.empty((n_prob, n_rec, n + 1))
    for j in range(n_prob):
        A = g.uniform(-1.0, 1.0, (n_rec, n))
        b = (A @ g.uniform(-1.0, 1.0, n)) * (1.0 + g.uniform(-1e-3, 1e-3, n_rec))
        b[g.random(n_rec) >= inl] *= 20.0
        rows[j, :, :n], rows[j, :, n] = A, b
    offs = np.arange(n_prob + 1, dtype=np.uint64) * n_rec
    return rows.reshape(n_prob * n_rec, n + 1), offs


def random_rotations(g, shape):
    """uniform random rotation matrices (shape + (3, 3)) from unit quaternions [s, qx, qy, qz]"""
    q = g.normal(size=shape + (4,))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    s, x, y, z = (q[..., i] for i in range(4))
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - s * z), 2 * (x * z + s * y),
                  2 * (x * y + s * z), 1 - 2 * (x * x + z * z), 2 * (y * z - s * x),
                  2 * (x * z - s * y), 2 * (y * z + s * x), 1 - 2 * (x * x + y * y)], axis=-1)
    return R.reshape(shape + (3, 3))


def gen_rigid(name, n_prob, n_rec, inl, seed):
    """(records (n_prob * n_rec, W), offsets) for the closed-form estimators, one random truth per problem:
    rays aimed at a point (sigma 0.3), point pairs under a rigid motion (sigma 0.2), pivoting frames (sigma 0.15),
    points near a 2-D line (sigma 0.2); outliers as in synth.py"""
    g = np.random.default_rng(seed)
    P, N = n_prob, n_rec
    is_out = g.random((P, N)) >= inl
    if name == "rays":
        target = g.uniform(-1000, 1000, (P, 1, 3))
        p = g.uniform(-1000, 1000, (P, N, 3))
        aim = np.where(is_out[..., None], g.uniform(-1000, 1000, (P, N, 3)), target + g.normal(0, 0.3, (P, N, 3)))
        d = aim - p
        d /= np.linalg.norm(d, axis=2, keepdims=True)
        recs = np.concatenate([p, d], axis=2)
    elif name == "absor":
        R, t = random_rotations(g, (P,)), g.uniform(-1000, 1000, (P, 1, 3))
        first = g.uniform(-100, 100, (P, N, 3))
        second = np.einsum("pij,pnj->pni", R, first) + t + g.normal(0, 0.2, (P, N, 3))
        second[is_out] += g.uniform(5, 50, (int(is_out.sum()), 3))
        recs = np.concatenate([first, second], axis=2)
    elif name == "pivot":
        tip, piv = g.uniform(-200, 200, (P, 1, 3)), g.uniform(-1000, 1000, (P, 1, 3))
        R = random_rotations(g, (P, N))
        t = piv - np.einsum("pnij,pnj->pni", R, np.broadcast_to(tip, (P, N, 3))) + g.normal(0, 0.15, (P, N, 3))
        t[is_out] += g.uniform(-40, 40, (int(is_out.sum()), 3))
        recs = np.concatenate([R.reshape(P, N, 9), t, np.zeros((P, N, 1))], axis=2)
    else:
        a, ang = g.uniform(-500, 500, (P, 1, 2)), g.uniform(0, np.pi, (P, 1))
        u = np.stack([np.cos(ang), np.sin(ang)], axis=-1)
        pts = a + g.uniform(-100, 100, (P, N, 1)) * u + g.normal(0, 0.2, (P, N, 2))
        pts[is_out] = (a + g.uniform(-100, 100, (P, N, 2)))[is_out]
        recs = pts
    offs = np.arange(P + 1, dtype=np.uint64) * N
    return np.ascontiguousarray(recs.reshape(P * N, -1)), offs


POINT_SHAPES = {"plane": (L.PLANE, 10_000, 1_000), "sphere": (L.SPHERE, 1_000, 10_000), "line": (L.LINE, 100_000, 100)}
# name -> (model, problems, records, inlier share, delta, aux)
RIGID_SHAPES = {"rays": (L.RAY, 100_000, 12, 0.7, 1.0, np.pi / 180), "absor": (L.ABSOR, 10_000, 20, 0.7, 1.0, 0.0),
                "pivot": (L.PIVOT, 1_000, 300, 0.7, 1.0, 0.0), "line2d": (L.LINE2D, 100_000, 200, 0.5, 0.5, 0.0)}
GEOMETRIC_SHAPES = {"sphere_lm": (1_000, 10_000), "sphere_lm_small": (10_000, 300)}
# name -> (n, problems, rows, inlier share)
DENSE_SHAPES = {"dense6": (6, 10_000, 500, 0.8), "dense16": (16, 1_000, 5_000, 0.9), "dense64": (64, 100, 20_000, 0.97)}
# name -> (generator's name, model, problems, records, inlier share, delta, aux)
EXHAUSTIVE_SHAPES = {"ex_rays": ("rays", L.RAY, 100_000, 12, 0.7, 1.0, np.pi / 180),
                     "ex_absor": ("absor", L.ABSOR, 10_000, 20, 0.7, 1.0, 0.0),
                     "ex_plane": ("plane", L.PLANE, 10_000, 40, 0.5, 0.5, 0.0),
                     "ex_plane300": ("plane", L.PLANE, 100, 300, 0.5, 0.5, 0.0)}


def timed(f, reps):
    t = []
    r = None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = f()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), r


def exhaustive(ctx, name, reps, loop_n):
    """one exhaustive shape: the batched call with the fused path on and off against the ransac_exhaustive loop"""
    kind, model, P, N, inl, delta, aux = EXHAUSTIVE_SHAPES[name]
    recs, offs = gen(model, P, N, inl, seed=model + N) if kind == "plane" else gen_rigid(kind, P, N, inl, seed=model)
    ctx.set_model(model, 3, delta, 0, aux=aux)
    m = min(loop_n, P, max(3, 200_000 // N ** 2))   # (a 300-point problem is 4.5 M hypotheses on its own)

    def many(fused):
        ctx.set_option("many_exhaustive_fused", fused)
        try:
            return ctx.ransac_many_exhaustive((recs, offs))
        finally:
            ctx.set_option("many_exhaustive_fused", 1)

    def loop():
        it = 0
        for j in range(m):
            ctx.upload(recs[int(offs[j]):int(offs[j + 1])])
            it += ctx.ransac_exhaustive()["info"].iterations
        return it
    res = many(1)   # warm
    many(0)
    loop()
    t_fused, t_general, t_loop = [], [], []
    for _ in range(reps):  # alternate the paths
        t_fused.append(timed(lambda: many(1), 1)[0])
        t_general.append(timed(lambda: many(0), 1)[0])
        t_loop.append(timed(loop, 1)[0])
    tm, tg, tl = float(np.median(t_fused)), float(np.median(t_general)), float(np.median(t_loop)) * P / m
    ev = res["evaluated"].astype(np.float64)
    return dict(shape=name, problems=P, records=N, many_ms=1e3 * tm, general_ms=1e3 * tg, loop_ms=1e3 * tl,
                loop_ms_per_problem=1e3 * tl / P, loop_extrapolated_from=m if m < P else None, speedup=tl / tm,
                speedup_general=tl / tg, fused_over_general=tg / tm, ok=int(np.sum(res["status"] == L.OK)),
                hypotheses_scanned=float(ev.sum()), agree_evaluations=float((ev * N).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--loop", type=int, default=1000, help="problems of the per-problem loop (extrapolated)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the results as one JSON file")
    ap.add_argument("--shapes", default="plane,sphere,line",
                    help="comma-separated shapes (%s), or 'rigid' / 'geometric' / 'dense' / 'exhaustive' for the "
                         "closed-form estimators' / the LM sphere's / the dense system's / the exhaustive search's"
                         % ", ".join(list(POINT_SHAPES) + list(RIGID_SHAPES) + list(GEOMETRIC_SHAPES) + list(DENSE_SHAPES)
                                     + list(EXHAUSTIVE_SHAPES)))
    a = ap.parse_args()
    names = {"rigid": list(RIGID_SHAPES), "geometric": list(GEOMETRIC_SHAPES),
             "dense": list(DENSE_SHAPES), "exhaustive": list(EXHAUSTIVE_SHAPES)}.get(a.shapes, a.shapes.split(","))
    for name in names:
        if (name not in POINT_SHAPES and name not in RIGID_SHAPES and name not in GEOMETRIC_SHAPES
                and name not in DENSE_SHAPES and name not in EXHAUSTIVE_SHAPES):
            ap.error("unknown shape %r" % name)
    reps = 1 if a.quick else a.reps
    loop_n = 100 if a.quick else a.loop
    ctx = Context(0)
    out = dict(shapes=[], latency=[])
    for name in names:
        batched = ctx.ransac_many
        if name in EXHAUSTIVE_SHAPES:
            row = exhaustive(ctx, name, reps, loop_n)
            out["shapes"].append(row)
            print(json.dumps(row), flush=True)
            continue
        if name in POINT_SHAPES:
            model, P, N = POINT_SHAPES[name]
            recs, offs = gen(model, P, N, 0.5, seed=model)
            ctx.set_model(model, 3, 0.5, L.LS_ALGEBRAIC)
        elif name in GEOMETRIC_SHAPES:
            model, (P, N) = L.SPHERE, GEOMETRIC_SHAPES[name]
            recs, offs = gen(model, P, N, 0.5, seed=model + N)
            ctx.set_model(model, 3, 0.5, L.LS_GEOMETRIC)
            batched = ctx.ransac_many_lm
        elif name in DENSE_SHAPES:
            n, P, N, inl = DENSE_SHAPES[name]
            recs, offs = gen_dense(n, P, N, inl, seed=n)
            ctx.set_model(L.DENSE, n, 0.1)
            batched = ctx.ransac_many_dense
        else:
            model, P, N, inl, delta, aux = RIGID_SHAPES[name]
            recs, offs = gen_rigid(name, P, N, inl, seed=model)
            ctx.set_model(model, 2 if model == L.LINE2D else 3, delta, 0, aux=aux)
        seeds = 1 + np.arange(P, dtype=np.uint64)
        many = lambda: batched((recs, offs), 0.999, seeds=seeds)
        m = min(loop_n, P)

        def loop():
            it = 0
            for j in range(m):
                ctx.upload(recs[int(offs[j]):int(offs[j + 1])])
                it += ctx.ransac(0.999, seed=int(seeds[j]))["info"].iterations
            return it
        many()   # warm
        loop()
        t_many, t_loop = [], []
        for _ in range(reps):  # alternate the two paths
            t, res = timed(many, 1)
            t_many.append(t)
            t, _ = timed(loop, 1)
            t_loop.append(t)
        tm, tl = float(np.median(t_many)), float(np.median(t_loop)) * P / m
        ev = res["evaluated"].astype(np.float64)
        row = dict(shape=name, problems=P, records=N, many_ms=1e3 * tm, loop_ms=1e3 * tl,
                   loop_ms_per_problem=1e3 * tl / P,
                   loop_extrapolated_from=m if m < P else None, speedup=tl / tm,
                   ok=int(np.sum(res["status"] == L.OK)), mean_iterations=float(np.mean(res["iterations"])),
                   hypotheses_scanned=float(ev.sum()), agree_evaluations=float((ev * N).sum()))
        out["shapes"].append(row)
        print(json.dumps(row), flush=True)
    for n in ((100, 1_000, 10_000) if any(nm in POINT_SHAPES for nm in names) else ()):
        recs, _ = gen(L.PLANE, 1, n, 0.5, seed=n)
        ctx.set_model(L.PLANE, 3, 0.5)

        def one(s=[0]):
            s[0] += 1
            ctx.upload(recs)
            return ctx.ransac(0.999, seed=s[0])
        one()
        t, r = timed(one, 5 if a.quick else 50)
        row = dict(n=n, single_call_ms=1e3 * t, iterations=int(r["info"].iterations))
        out["latency"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
