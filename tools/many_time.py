"""Context.ransac_many (lsqr_ransac_many) against the per-problem Context.ransac loop on the same problems.

Shapes (the loop is timed on the first --loop problems and extrapolated when the set is larger; the output says so):
  plane  3-D  10 000 problems x  1 000 records, 50 % inliers
  sphere 3-D   1 000 problems x 10 000 records (algebraic), 50 % inliers
  line   3-D 100 000 problems x    100 records, 50 % inliers
and the single-call latency of Context.ransac (upload + compute) at N = 100 / 1 000 / 10 000.  Every timed call
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


def timed(f, reps):
    t = []
    r = None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = f()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--loop", type=int, default=1000, help="problems of the per-problem loop (extrapolated)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the results as one JSON file")
    a = ap.parse_args()
    reps = 1 if a.quick else a.reps
    loop_n = 100 if a.quick else a.loop
    ctx = Context(0)
    out = dict(shapes=[], latency=[])
    shapes = [("plane", L.PLANE, 10_000, 1_000), ("sphere", L.SPHERE, 1_000, 10_000), ("line", L.LINE, 100_000, 100)]
    for name, model, P, N in shapes:
        recs, offs = gen(model, P, N, 0.5, seed=model)
        seeds = 1 + np.arange(P, dtype=np.uint64)
        ctx.set_model(model, 3, 0.5, L.LS_ALGEBRAIC)
        many = lambda: ctx.ransac_many((recs, offs), 0.999, seeds=seeds)
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
                   loop_extrapolated_from=m if m < P else None, speedup=tl / tm,
                   ok=int(np.sum(res["status"] == L.OK)), mean_iterations=float(np.mean(res["iterations"])),
                   hypotheses_scanned=float(ev.sum()), agree_evaluations=float((ev * N).sum()))
        out["shapes"].append(row)
        print(json.dumps(row), flush=True)
    for n in (100, 1_000, 10_000):
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
