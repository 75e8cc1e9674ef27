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
One JSON line per M on stdout; --out FILE also writes them to FILE."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lsqrrecipes_amd import _lib as L  # noqa: E402
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


def refine_rounds(ctx, rows, max_rounds):
    """lsqr_refine without labels_out -> rounds done"""
    import ctypes as C
    par = np.array(rows, dtype=np.float64, order="C")
    m = par.shape[0]
    fits = (L.FitInfo * m)()
    status = np.zeros(m, dtype=np.int32)
    rounds, conv = C.c_size_t(0), C.c_int(0)
    ctx._chk(ctx._lib.lsqr_refine(ctx._h, L.ptr(par), m, max_rounds, 0, None, None, fits, L.ptr(status),
                                  C.byref(rounds), C.byref(conv)))
    return int(rounds.value)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--models", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, nargs=2, default=[1, 5], metavar=("R1", "R2"))
    ap.add_argument("--baseline-reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    data, planes = scene(a.n)
    r1, r2 = a.rounds
    lines = []
    with Context(0) as ctx:
        ctx.set_model(L.PLANE, 3, DELTA, L.LS_ALGEBRAIC).upload(data)
        for m in a.models:
            rows = models(planes, m)
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
            row = dict(n=a.n, models=m, reps=a.reps, rounds_done=list(done), counts_assigned=int(a.n - asg["counts"][-1]),
                       refine_round_ms=ms(per), assign_call_ms=ms(t_asg), baseline_round_ms=ms(t_base),
                       baseline_reps=len(t_base), ratio=round(float(np.median(t_base)) / rnd, 1),
                       record_bytes_per_s=round(a.n * 24 / rnd, 0), hbm_fraction=round(a.n * 24 / rnd / HBM_PEAK, 4))
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
