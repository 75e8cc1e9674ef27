"""Context.ransac_grouped_sequential (lsqr_ransac_grouped_sequential) with device labels against what a caller has to do
without it when the records are an attached device tensor with interleaved integer labels and every label needs several
models:
  1. download the records;  2. stable gather by label on the host;  3. Context.ransac_many_sequential on the gather;
  4. scatter the round labels back to record order on the host.
Workload: --records (default 1 000 000) plane records on an attached tensor, --groups (default 4096) interleaved labels,
every group three planes of 3/10 of its records each and 1/10 clutter, max_models = 3, p = 0.999.
The two paths alternate in one process after a warm-up of each; every timed call ends in a device synchronisation (both
return host results).  Reported per path: median, minimum and maximum of --reps repetitions, and the host path's four
steps.  The split of the new call comes from two more variants of it, alternating with the others:
  grouping  the call with every label -1: keys, sort, offsets and the one synchronisation at full size; nothing is
            gathered (the gather proper moves 2 x 24 bytes per record) and no round runs
  rounds    the call without labels_out (no label buffer, no label-only partition parts, no scatter) minus grouping
  labels    the full call minus the call without labels_out
One JSON line on stdout; --out FILE also writes it to FILE.  The outputs of the two paths are compared bit for bit
before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lsqrrecipes_amd import _lib as L  # noqa: E402
from lsqrrecipes_amd.context import Context  # noqa: E402

P, MAX_MODELS, MIN_VOTES = 0.999, 3, 8


def gen(n_records, n_groups, seed):
    """(records (n, 3), int32 labels): the labels are a seeded shuffle of arange(n) % n_groups; group g holds three
    random planes (sigma 0.2) in its own 200-unit box, about 3/10 of its records on each, and uniform clutter"""
    g = np.random.default_rng(seed)
    labels = (np.arange(n_records) % n_groups).astype(np.int32)
    g.shuffle(labels)
    which = g.integers(0, 10, n_records)  # 0..8: plane which // 3; 9: clutter
    c = g.uniform(-500, 500, (n_groups, 3))
    u, v = g.normal(size=(n_groups, 3, 3)), g.normal(size=(n_groups, 3, 3))
    a = c[:, None, :] + g.uniform(-100, 100, (n_groups, 3, 3))
    q = np.minimum(which // 3, 2)
    s, t = g.uniform(-100, 100, (n_records, 1)), g.uniform(-100, 100, (n_records, 1))
    pts = a[labels, q] + s * u[labels, q] + t * v[labels, q] + g.normal(0, 0.2, (n_records, 3))
    clutter = c[labels] + g.uniform(-100, 100, (n_records, 3))
    pts[which == 9] = clutter[which == 9]
    return np.ascontiguousarray(pts), labels


def host_path(ctx, t, labels, n_groups, seeds, times=None):
    """the four steps -> ransac_many_sequential's dict with the labels in record order"""
    t0 = time.perf_counter()
    data = t.cpu().numpy()  # (synchronises)
    t1 = time.perf_counter()
    idx = np.flatnonzero((labels >= 0) & (labels < n_groups))
    order = idx[np.argsort(labels[idx], kind="stable")]
    offs = np.zeros(n_groups + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(np.bincount(labels[idx], minlength=n_groups))
    packed = np.ascontiguousarray(data[order])
    t2 = time.perf_counter()
    w = ctx.ransac_many_sequential((packed, offs), P, MAX_MODELS, seeds=seeds, min_votes=MIN_VOTES)
    t3 = time.perf_counter()
    lab = np.full(len(labels), -1, dtype=np.int32)
    lab[order] = w["labels"]
    w["labels"] = lab
    t4 = time.perf_counter()
    if times is not None:
        for key, dt in zip(("download", "gather", "many_sequential", "scatter", "total"),
                           (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t4 - t0)):
            times.setdefault(key, []).append(1e3 * dt)
    return w


def timed(ctx, fn, bucket):
    ctx.synchronize()
    t0 = time.perf_counter()
    r = fn()
    ctx.synchronize()
    bucket.append(1e3 * (time.perf_counter() - t0))
    return r


def spread(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), reps=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--groups", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("grouped_sequential_time.py needs a GPU: a timing without one says nothing")
    data, labels = gen(a.records, a.groups, 20261)
    seeds = 1 + np.arange(a.groups * MAX_MODELS, dtype=np.uint64).reshape(a.groups, MAX_MODELS)
    t = torch.from_numpy(data).to("cuda:0")
    g = torch.from_numpy(labels).to("cuda:0")
    none = torch.full_like(g, -1)
    out = torch.empty_like(g)
    torch.cuda.synchronize()
    with Context(0) as ctx:
        ctx.set_model(L.PLANE, 3, 0.5, L.LS_ALGEBRAIC)
        ctx.attach(t.data_ptr(), a.records, 24, keepalive=t)
        full = lambda: ctx.ransac_grouped_sequential(g, a.groups, P, MAX_MODELS, seeds=seeds, min_votes=MIN_VOTES,
                                                     labels_out=out)
        nolab = lambda: ctx.ransac_grouped_sequential(g, a.groups, P, MAX_MODELS, seeds=seeds, min_votes=MIN_VOTES)
        group = lambda: ctx.ransac_grouped_sequential(none, a.groups, P, MAX_MODELS, seeds=seeds, min_votes=MIN_VOTES)
        # warm-up of every shape, and the outputs compared
        w = host_path(ctx, t, labels, a.groups, seeds)
        r = full()
        ctx.synchronize()
        lab = out.cpu().numpy()
        for key in ("n_models", "status", "fraction", "iterations", "best_index", "best_votes", "n_params", "n_used",
                    "params", "cost", "offsets"):
            assert np.ascontiguousarray(r[key]).tobytes() == np.ascontiguousarray(w[key]).tobytes(), key
        assert lab.tobytes() == w["labels"].tobytes()
        nolab(), group()
        ms = dict(full=[], nolab=[], group=[])
        steps = {}
        for _ in range(a.reps):  # alternating
            timed(ctx, full, ms["full"])
            host_path(ctx, t, labels, a.groups, seeds, steps)
            timed(ctx, nolab, ms["nolab"])
            timed(ctx, group, ms["group"])
    med = {k: float(np.median(v)) for k, v in ms.items()}
    row = dict(workload=dict(records=a.records, groups=a.groups, max_models=MAX_MODELS, min_votes=MIN_VOTES, p=P,
                             models_found=int(w["n_models"].sum()), rounds_run=int(np.sum(w["status"] != L.ERR_STATE)),
                             records_claimed=int(np.sum(w["labels"] >= 0))),
               grouped_sequential_device_labels=spread(ms["full"]),
               host_path=dict(spread(steps["total"]), steps_median_ms={k: float(np.median(v)) for k, v in steps.items()
                                                                       if k != "total"}),
               speedup_median=float(np.median(steps["total"]) / med["full"]),
               split=dict(without_labels=spread(ms["nolab"]), every_label_minus_one=spread(ms["group"]),
                          grouping_ms=med["group"], rounds_ms=med["nolab"] - med["group"],
                          labels_ms=med["full"] - med["nolab"]))
    line = json.dumps(row)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
