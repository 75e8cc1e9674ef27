"""Context.ransac_sequential (lsqr_ransac_sequential: the survivors of every round compacted on the device) against
the host loop it replaces (Context.ransac, numpy removal of the consensus set, Context.upload of what is left).

Scene: --n points (default 10 M) in 3-D, four planes of 20 % each plus 20 % uniform clutter, shuffled; plane model,
delta 0.5, p = 0.999, max_models 4, seeds 1..4.  Both paths start from the scene already uploaded and must produce the
same models (iterations, best_index and best_votes per round are compared; a mismatch is an error).  The two paths
alternate in one process after one warm pass of each; every timed call ends with host results (a device
synchronisation); the scene is uploaded again, untimed, after every host loop.  Medians over --reps repetitions.
--quick: one repetition and no host loop (for a `rocprofv3 --kernel-trace --stats` run that prices k_seq_count /
k_seq_scan / k_seq_write).  One JSON line on stdout; --out FILE also writes it to FILE."""
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


def scene(n, seed=20261017, box=1000.0, sigma=0.4):
    g = np.random.default_rng(seed)
    m = n // 5
    parts = []
    for _ in range(4):
        q, _r = np.linalg.qr(g.normal(size=(3, 3)))
        a = g.uniform(-box / 2, box / 2, 3)
        st = g.uniform(-box, box, (m, 2))
        parts.append(a + st[:, :1] * q[:, 0] + st[:, 1:] * q[:, 1] + g.normal(0.0, sigma, (m, 1)) * q[:, 2])
    parts.append(g.uniform(-box, box, (n - 4 * m, 3)))
    pts = np.concatenate(parts)
    return np.ascontiguousarray(pts[g.permutation(n)])


def host_loop(ctx, data, seeds):
    """-> (rounds [(iterations, best_index, best_votes)], seconds in ransac, in numpy removal, in upload)"""
    rounds, t_r, t_n, t_u = [], 0.0, 0.0, 0.0
    cur = data
    for r, seed in enumerate(seeds):
        t0 = time.perf_counter()
        w = ctx.ransac(P, seed=int(seed))
        t1 = time.perf_counter()
        t_r += t1 - t0
        i = w["info"]
        rounds.append((int(i.iterations), int(i.best_index), int(i.best_votes)))
        if w["status"] != L.OK or r + 1 == len(seeds):
            break
        cur = cur[w["consensus"] == 0]
        t2 = time.perf_counter()
        ctx.upload(cur)
        t3 = time.perf_counter()
        t_n += t2 - t1
        t_u += t3 - t2
    return rounds, t_r, t_n, t_u


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--no-labels", action="store_true", help="time the call without the label array")
    ap.add_argument("--out")
    a = ap.parse_args()
    data = scene(a.n)
    seeds = 1 + np.arange(MODELS, dtype=np.uint64)
    reps = 1 if a.quick else a.reps
    seq_s, loop_s, parts = [], [], []
    with Context(0) as ctx:
        ctx.set_model(L.PLANE, 3, DELTA).upload(data)
        for rep in range(-1, reps):  # rep -1 warms both paths
            t0 = time.perf_counter()
            res = ctx.ransac_sequential(P, MODELS, seeds=seeds, want_labels=not a.no_labels)
            t1 = time.perf_counter()
            got = [(int(res["iterations"][r]), int(res["best_index"][r]), int(res["best_votes"][r]))
                   for r in range(res["n_models"])]
            if a.quick and rep >= 0:
                seq_s.append(t1 - t0)
                continue
            t2 = time.perf_counter()
            rounds, t_r, t_n, t_u = host_loop(ctx, data, seeds)
            t3 = time.perf_counter()
            ctx.upload(data)  # untimed: the scene again for the next repetition
            if got != rounds:
                raise SystemExit("the two paths disagree: %r against %r" % (got, rounds))
            if rep >= 0:
                seq_s.append(t1 - t0)
                loop_s.append(t3 - t2)
                parts.append((t_r, t_n, t_u))
    med = lambda v: float(np.median(v)) * 1e3 if len(v) else None
    row = dict(n=a.n, models=len(got), best_votes=[g[2] for g in got], iterations=[g[0] for g in got], reps=reps,
               labels=not a.no_labels, sequential_ms=med(seq_s), host_loop_ms=med(loop_s),
               host_loop_ransac_ms=med([p[0] for p in parts]), host_loop_numpy_ms=med([p[1] for p in parts]),
               host_loop_upload_ms=med([p[2] for p in parts]),
               sequential_ms_all=[round(1e3 * s, 3) for s in seq_s], host_loop_ms_all=[round(1e3 * s, 3) for s in loop_s])
    line = json.dumps(row)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
