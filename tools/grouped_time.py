"""Context.ransac_grouped (lsqr_ransac_grouped: records and labels stay on the device, grouped there) against the host
path it replaces: .cpu() of the records and the labels, a numpy stable gather by label, Context.ransac_many (which
uploads the gathered records), the consensus permuted back to record order and sent up with .to(device).

Workload: --groups (default 4096) groups of --points (default 2048) points in 3-D, one plane of 60 % plus uniform
clutter per group, all records interleaved by one permutation; plane model, delta 0.5, p = 0.999.  The records, the
int32 labels and the uint8 consensus are torch tensors on the device.  Both paths must take the same decisions (status,
best_votes and the consensus bytes are compared; a mismatch is an error).  The two paths alternate in one process after
one warm pass of each; every timed call ends synchronised, with host results and the consensus on the device.  Medians
over --reps repetitions, and the host path's parts.  --quick: one repetition and no host path (for a
`rocprofv3 --kernel-trace --stats` run that prices k_grp_keys / the sort / k_grp_offsets / k_grp_gather /
k_grp_scatter).  Also printed: the bytes each grouping kernel has to move, computed from the shapes, to set against the
trace's kernel times.  One JSON line on stdout; --out FILE also writes it to FILE."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lsqrrecipes_amd import _lib as L  # noqa: E402
from lsqrrecipes_amd.context import Context  # noqa: E402

P, DELTA = 0.999, 0.5


def scene(n_groups, n, seed=20261018, box=1000.0, sigma=0.4):
    """-> records (n_groups * n, 3) and int32 labels, interleaved by one permutation"""
    g = np.random.default_rng(seed)
    m = (6 * n) // 10
    out = np.empty((n_groups, n, 3))
    for j in range(n_groups):
        q, _r = np.linalg.qr(g.normal(size=(3, 3)))
        a = g.uniform(-box / 2, box / 2, 3)
        st = g.uniform(-box, box, (m, 2))
        out[j, :m] = a + st[:, :1] * q[:, 0] + st[:, 1:] * q[:, 1] + g.normal(0.0, sigma, (m, 1)) * q[:, 2]
        out[j, m:] = g.uniform(-box, box, (n - m, 3))
    labels = np.repeat(np.arange(n_groups, dtype=np.int32), n)
    perm = g.permutation(n_groups * n)
    return np.ascontiguousarray(out.reshape(-1, 3)[perm]), np.ascontiguousarray(labels[perm])


def host_path(ctx, t_rec, t_lab, n_groups, seeds, t_out):
    """-> (ransac_many's dict, seconds of: the copies down, the numpy gather, ransac_many, the permute + copy up)"""
    import torch
    t0 = time.perf_counter()
    recs, labels = t_rec.cpu().numpy(), t_lab.cpu().numpy()
    t1 = time.perf_counter()
    idx = np.flatnonzero((labels >= 0) & (labels < n_groups))
    order = idx[np.argsort(labels[idx], kind="stable")]
    offs = np.zeros(n_groups + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(np.bincount(labels[idx], minlength=n_groups))
    gathered = np.ascontiguousarray(recs[order])
    t2 = time.perf_counter()
    w = ctx.ransac_many((gathered, offs), P, seeds=seeds)
    t3 = time.perf_counter()
    cons = np.zeros(len(labels), dtype=np.uint8)
    cons[order] = w["consensus"]
    t_out.copy_(torch.from_numpy(cons).to(t_out.device))
    torch.cuda.synchronize()
    t4 = time.perf_counter()
    return w, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--groups", type=int, default=4096)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    recs, labels = scene(a.groups, a.points)
    N, W = recs.shape
    seeds = 1 + np.arange(a.groups, dtype=np.uint64)
    reps = 1 if a.quick else a.reps
    t_rec = torch.from_numpy(recs).to("cuda:0")
    t_lab = torch.from_numpy(labels).to("cuda:0")
    out_g = torch.zeros(N, dtype=torch.uint8, device="cuda:0")
    out_h = torch.zeros(N, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    grp_s, host_s, parts = [], [], []
    with Context(0) as ctx:
        ctx.set_model(L.PLANE, 3, DELTA, L.LS_ALGEBRAIC)
        ctx.attach(t_rec.data_ptr(), N, W * 8, keepalive=t_rec)
        for rep in range(-1, reps):  # rep -1 warms both paths
            t0 = time.perf_counter()
            res = ctx.ransac_grouped(t_lab, a.groups, P, seeds=seeds, consensus_out=out_g)  # (returns synchronised)
            t1 = time.perf_counter()
            if a.quick:
                if rep >= 0:
                    grp_s.append(t1 - t0)
                continue
            t2 = time.perf_counter()
            w, pt = host_path(ctx, t_rec, t_lab, a.groups, seeds, out_h)
            t3 = time.perf_counter()
            if (not np.array_equal(res["status"], w["status"]) or not np.array_equal(res["best_votes"], w["best_votes"])
                    or not np.array_equal(res["params"].view(np.uint64), w["params"].view(np.uint64))
                    or not torch.equal(out_g, out_h)):
                raise SystemExit("the two paths disagree")
            if rep >= 0:
                grp_s.append(t1 - t0)
                host_s.append(t3 - t2)
                parts.append(pt)
    med = lambda v: float(np.median(v)) * 1e3 if len(v) else None
    part = lambda k: med([p[k] for p in parts])
    # what the grouping kernels move, from the shapes: keys (label in, key + index out), the sort's passes (pairs in
    # and out per 8-bit digit at least), the gather (index + record in, record out), the scatter (key, index, flag's
    # byte and mask byte in, one byte out)
    bits = max(int(a.groups).bit_length(), 1)
    moved = dict(k_grp_keys=12 * N, sort_min=16 * N * ((bits + 7) // 8), k_grp_gather=(4 + 16 * W) * N,
                 k_grp_scatter=11 * N, k_grp_offsets_out=8 * (a.groups + 1))
    row = dict(groups=a.groups, points=a.points, records=N, reps=reps, ok_groups=int((res["status"] == L.OK).sum()),
               grouped_ms=med(grp_s), host_path_ms=med(host_s), host_cpu_copies_ms=part(0), host_numpy_gather_ms=part(1),
               host_ransac_many_ms=part(2), host_permute_upload_ms=part(3),
               grouped_ms_all=[round(1e3 * s, 3) for s in grp_s], host_path_ms_all=[round(1e3 * s, 3) for s in host_s],
               bytes_moved=moved)
    line = json.dumps(row)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
