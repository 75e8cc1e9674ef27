"""Context.ransac_many_sequential (lsqr_ransac_many_sequential: every round one batched search, the survivors of all
problems compacted on the device) against the host loop it replaces (Context.ransac_many, numpy removal of every
problem's consensus set, the survivors handed to the next ransac_many call from pageable memory).

Workload: --problems (default 4096) problems of --points (default 2048) points in 3-D, three planes of 25 % each plus
25 % uniform clutter, shuffled; plane model, delta 0.5, p = 0.999, max_models 4, min_votes a tenth of a problem.  Both
paths start from the packed host records and must take the same decisions (n_models and best_votes per problem and
round are compared; a mismatch is an error).  The two paths alternate in one process after one warm pass of each;
every timed call ends with host results.  Medians over --reps repetitions.  --quick: one repetition and no host loop
(for a `rocprofv3 --kernel-trace --stats` run that prices k_mseq_count / k_mseq_write).  One JSON line on stdout;
--out FILE also writes it to FILE."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lsqrrecipes_amd import _lib as L  # noqa: E402
from lsqrrecipes_amd.context import Context  # noqa: E402

P, MODELS, DELTA = 0.999, 4, 0.5


def scene(n_problems, n, seed=20261017, box=1000.0, sigma=0.4):
    """-> records (n_problems * n, 3), every problem shuffled on its own"""
    g = np.random.default_rng(seed)
    m = n // 4
    out = np.empty((n_problems, n, 3))
    for j in range(n_problems):
        parts = []
        for _ in range(3):
            q, _r = np.linalg.qr(g.normal(size=(3, 3)))
            a = g.uniform(-box / 2, box / 2, 3)
            st = g.uniform(-box, box, (m, 2))
            parts.append(a + st[:, :1] * q[:, 0] + st[:, 1:] * q[:, 1] + g.normal(0.0, sigma, (m, 1)) * q[:, 2])
        parts.append(g.uniform(-box, box, (n - 3 * m, 3)))
        out[j] = np.concatenate(parts)[g.permutation(n)]
    return np.ascontiguousarray(out.reshape(-1, 3))


def host_loop(ctx, recs, offs, seeds, min_votes):
    """-> (n_models, best_votes (n, MODELS), seconds in ransac_many, in numpy removal)"""
    n = len(offs) - 1
    n_models = np.zeros(n, dtype=np.int64)
    votes = np.zeros((n, MODELS), dtype=np.uint32)
    active = np.arange(n)
    t_r = t_n = 0.0
    for r in range(MODELS):
        if len(active) == 0:
            break
        t0 = time.perf_counter()
        w = ctx.ransac_many((recs, offs), P, seeds=np.ascontiguousarray(seeds[active, r]))
        t1 = time.perf_counter()
        t_r += t1 - t0
        votes[active, r] = w["best_votes"]
        ok = (w["status"] == L.OK) & (w["best_votes"] >= max(min_votes, 1))
        n_models[active[ok]] = r + 1
        if r + 1 < MODELS:
            sizes = np.diff(offs.astype(np.int64))
            prob_of = np.repeat(np.arange(len(active)), sizes)
            unclaimed = w["consensus"] == 0
            left = np.bincount(prob_of[unclaimed], minlength=len(active))  # every problem's survivors
            go = ok & (left >= ctx.K)
            recs = np.ascontiguousarray(recs[unclaimed & go[prob_of]])
            active = active[go]
            offs = np.zeros(len(active) + 1, dtype=np.uint64)
            offs[1:] = np.cumsum(left[go])
        t_n += time.perf_counter() - t1
    return n_models, votes, t_r, t_n


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--problems", type=int, default=4096)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--no-labels", action="store_true", help="time the call without the label array")
    ap.add_argument("--out")
    a = ap.parse_args()
    recs = scene(a.problems, a.points)
    offs = (np.arange(a.problems + 1, dtype=np.uint64) * np.uint64(a.points))
    seeds = 1 + np.arange(a.problems * MODELS, dtype=np.uint64).reshape(a.problems, MODELS)
    min_votes = a.points // 10
    reps = 1 if a.quick else a.reps
    seq_s, loop_s, parts = [], [], []
    with Context(0) as ctx:
        ctx.set_model(L.PLANE, 3, DELTA, L.LS_ALGEBRAIC)
        for rep in range(-1, reps):  # rep -1 warms both paths
            t0 = time.perf_counter()
            res = ctx.ransac_many_sequential((recs, offs), P, MODELS, seeds=seeds, min_votes=min_votes,
                                             want_labels=not a.no_labels)
            t1 = time.perf_counter()
            if a.quick:
                if rep >= 0:
                    seq_s.append(t1 - t0)
                continue
            t2 = time.perf_counter()
            n_models, votes, t_r, t_n = host_loop(ctx, recs, offs, seeds, min_votes)
            t3 = time.perf_counter()
            if not np.array_equal(n_models, res["n_models"]) or not np.array_equal(votes, res["best_votes"]):
                raise SystemExit("the two paths disagree")
            if rep >= 0:
                seq_s.append(t1 - t0)
                loop_s.append(t3 - t2)
                parts.append((t_r, t_n))
    med = lambda v: float(np.median(v)) * 1e3 if len(v) else None
    hist = np.bincount(res["n_models"], minlength=MODELS + 1).tolist()
    row = dict(problems=a.problems, points=a.points, max_models=MODELS, n_models_histogram=hist, reps=reps,
               labels=not a.no_labels, many_sequential_ms=med(seq_s), host_loop_ms=med(loop_s),
               host_loop_ransac_many_ms=med([p[0] for p in parts]), host_loop_numpy_ms=med([p[1] for p in parts]),
               many_sequential_ms_all=[round(1e3 * s, 3) for s in seq_s],
               host_loop_ms_all=[round(1e3 * s, 3) for s in loop_s])
    line = json.dumps(row)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
