"""The small dense solvers ON THE DEVICE (tools/linalg_probe, built by build()) on the families of
tests/linalg_families.py.

The thread-per-problem routines of small_linalg.h are the source the host tests compile, with contraction off on both
sides: their results are compared bit for bit with the host build's, and the accuracy checks of tests/test_small_linalg.py
run on the device's output too.  The wave-cooperative solvers of wave_linalg.h are device only: the three eliminations
are compared with each other (they are declared bit-identical by one pivot rule, which only a tie or an exact zero can
put to the test), with a plain NumPy elimination by the same rule for what they refuse, and with exact solutions.

Every test writes one input file, runs the probe once as a child process, and reads one output file."""
import os
import subprocess

import numpy as np
import pytest

import linalg_families as F
import test_small_linalg as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "linalg_probe")
SYM_EIG, SVD, PINV, CHOL, SPD_EIG, SINCOS, GEPP, WPINV, JACOBI, NULLVEC = 1, 2, 3, 4, 5, 6, 10, 11, 12, 13


def probe(tmp_path, sections):
    """sections: [(routine, m, n, variant, tol, problems as a count x in_stride array)] -> [count x out_stride arrays]"""
    assert os.path.exists(PROBE), "tools/linalg_probe is missing: build() compiles it"
    fin, fout = str(tmp_path / "probe_in.bin"), str(tmp_path / "probe_out.bin")
    with open(fin, "wb") as f:
        for routine, m, n, variant, tol, prob in sections:
            prob = np.ascontiguousarray(prob, dtype=np.float64)
            assert prob.ndim == 2 and n <= 64 and len(prob) <= 4096 or routine == SINCOS
            np.array([routine, len(prob), m, n, variant, tol, 0, 0], dtype=np.float64).tofile(f)
            prob.tofile(f)
    r = subprocess.run([PROBE, fin, fout], timeout=60, capture_output=True, text=True)
    assert r.returncode == 0, "linalg_probe exit %d: %s" % (r.returncode, r.stderr[-2000:])
    raw = np.fromfile(fout, dtype=np.float64)
    out, at = [], 0
    for routine, m, n, variant, tol, prob in sections:
        count, stride = int(raw[at]), int(raw[at + 1])
        assert count == len(prob)
        out.append(raw[at + 2:at + 2 + count * stride].reshape(count, stride))
        at += 2 + count * stride
    assert at == len(raw)
    return out


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64),
                          np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return T.build_host(tmp_path_factory)


def scaled_members(members, n_of, parts):
    """[(tag, member, k, scaled parts)] for every admissible scale of every member."""
    out = []
    for mem in members:
        for k in T.scales_for(n_of(mem)):
            sc = [F.scaled(p(mem), k) for p in parts]
            if all(s is not None for s in sc):
                out.append((mem, k, sc))
    return out


@pytest.mark.parametrize("size", sorted(set(m[0] for m in F.symmetric_all())))
def test_device_sym_eig_matches_host_bits_and_bounds(tmp_path, host, size):
    items = scaled_members([m for m in F.symmetric_all() if m[0] == size], lambda m: m[0], [lambda m: m[2]])
    sizes = [size]
    outs = probe(tmp_path, [(SYM_EIG, n, n, 0, 0.0, np.array([sc[0].ravel() for m, _, sc in items if m[0] == n])) for n in sizes])
    wc = T.Worst()
    for n, o in zip(sizes, outs):
        for (m, k, sc), row in zip([it for it in items if it[0][0] == n], o):
            tag = "device sym_eig n=%d %s 2^%d" % (n, m[1], k)
            w, v = row[:n], row[n:].reshape(n, n)
            hw, hv = host.sym_eig(sc[0])
            wc.require(bits_equal(w, hw) and bits_equal(v, hv), tag, "bits differ from the host build's")
            T.check_sym_eig(wc, tag, sc[0], w, v)
    wc.done()


def test_device_svd_jacobi_matches_host_bits_and_bounds(tmp_path, host):
    items = scaled_members(F.tall_all(), lambda m: m[1], [lambda m: m[3]])
    shapes = list(F.TALL_SHAPES)
    outs = probe(tmp_path, [(SVD, m, n, 0, 0.0, np.array([sc[0].ravel() for mem, _, sc in items if mem[:2] == (m, n)]))
                            for m, n in shapes])
    wc = T.Worst()
    for (m, n), o in zip(shapes, outs):
        for (mem, k, sc), row in zip([it for it in items if it[0][:2] == (m, n)], o):
            tag = "device svd %dx%d %s 2^%d" % (m, n, mem[2], k)
            u, s, v = row[:m * n].reshape(m, n), row[m * n:m * n + n], row[m * n + n:].reshape(n, n)
            hu, hs, hv = host.svd(sc[0])
            wc.require(bits_equal(u, hu) and bits_equal(s, hs) and bits_equal(v, hv), tag, "bits differ from the host build's")
            T.check_svd(wc, tag, sc[0], u, s, v, mem[4])
    wc.done()


def _square_items(ns, scales_of=T.scales_for):
    items = []
    for n in ns:
        for name, a, b, x in F.square(n):
            for k in scales_of(n):
                ak, bk = F.scaled(a, k), F.scaled(b, k)
                if ak is not None and bk is not None:
                    items.append((n, name, k, ak, bk, x))
    return items


def _systems(items, n):
    return np.array([np.concatenate([a.ravel(), b]) for nn, _, _, a, b, _ in items if nn == n])


def test_device_pinv_solve_matches_host_bits_and_bounds(tmp_path, host):
    items = _square_items(F.SQUARE_N)
    outs = probe(tmp_path, [(PINV, n, n, 0, T.SV_EPS, _systems(items, n)) for n in F.SQUARE_N])
    wc = T.Worst()
    for n, o in zip(F.SQUARE_N, outs):
        for (_, name, k, a, b, x_exact), row in zip([it for it in items if it[0] == n], o):
            tag = "device pinv_solve n=%d %s 2^%d" % (n, name, k)
            hr, hx = host.pinv_solve(a, b)
            wc.require(int(row[0]) == hr and bits_equal(row[1:], hx), tag, "rank or bits differ from the host build's")
            want, near = T.expected_rank(a)
            if near:
                continue
            wc.require(int(row[0]) == want, tag, "rank %d, by the 2.2e-16 threshold %d" % (row[0], want))
            if int(row[0]) == n:
                T.check_solution(wc, tag, a, row[1:], x_exact)
    wc.done()


def test_device_spd_solvers_match_host_bits_and_bounds(tmp_path, host):
    scales = (-600, -300, 0, 300, 500)
    items = [(n, name, k, F.scaled(g, k), F.scaled(rhs, k)) for n, name, g, rhs, r, x0 in T.spd_members() for k in scales]
    items = [it for it in items if it[3] is not None and it[4] is not None]
    sizes = sorted(set(it[0] for it in items))
    rho = T.rho_family()
    rho_sys = np.array([[1.0, r, r, 1.0, 1.0, 2.0] for r in rho])
    sections = []
    for n in sizes:
        sys_n = np.array([np.concatenate([g.ravel(), rhs]) for nn, _, _, g, rhs in items if nn == n])
        sections += [(CHOL, n, n, 0, 7.5, sys_n), (SPD_EIG, n, n, 0, 1e-13, sys_n)]
    sections.append((CHOL, 2, 2, 0, -3.25, rho_sys))
    outs = probe(tmp_path, sections)
    dev_chol, dev_eig = {}, {}
    wc = T.Worst()
    for i, n in enumerate(sizes):
        for (_, name, k, g, rhs), rc, re in zip([it for it in items if it[0] == n], outs[2 * i], outs[2 * i + 1]):
            tag = "device spd n=%d %s 2^%d" % (n, name, k)
            ok, xc = host.spd_solve_chol(g, rhs, 7.5)
            rank, xe = host.spd_solve_eig(g, rhs)
            wc.require(bool(rc[0]) == ok and bits_equal(rc[1:], xc), tag, "spd_solve_chol differs from the host build's")
            wc.require(int(re[0]) == rank and bits_equal(re[1:], xe), tag, "spd_solve_eig differs from the host build's")
            dev_chol[g.tobytes()], dev_eig[g.tobytes()] = (bool(rc[0]), rc[1:]), (int(re[0]), re[1:])
    wc.done()
    # the accuracy checks of the host test on the device's answers
    T.run_spd(lambda g, rhs, fill: dev_chol[g.tobytes()], lambda g, rhs: dev_eig[g.tobytes()], scales).done()
    rows = iter(outs[-1])
    T.run_chol_threshold(lambda g, rhs, fill: (lambda r: (bool(r[0]), r[1:]))(next(rows))).done()


def test_device_sincos_matches_host_bits_and_bound(tmp_path, host):
    sets = T.sincos_sets()
    special = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2e-308, -2.2e-308, 1e-300, -1e-300, np.pi / 4, -np.pi / 4])
    x = np.concatenate([v for v in sets.values()] + [special])
    x = np.concatenate([x, -x])
    x = x[np.abs(x) < 8.2e5]  # beyond it the platform's functions answer, and the platforms differ
    (o,) = probe(tmp_path, [(SINCOS, 1, 1, 0, 0.0, x[:, None])])
    hs, hc = host.sincos(x)
    d = (o[:, 0].view(np.uint64) != hs.view(np.uint64)) | (o[:, 1].view(np.uint64) != hc.view(np.uint64))
    assert not d.any(), "%d of %d arguments differ from the host build, first %r" % (d.sum(), len(x), x[d][:4])
    es, ec = T.ulp_error(o[:, 0], np.sin(x.astype(T.LD))), T.ulp_error(o[:, 1], np.cos(x.astype(T.LD)))
    print("device lsqr_sincos: worst %.3f ulp (sin), %.3f ulp (cos) over %d arguments" % (es.max(), ec.max(), len(x)))
    assert es.max() < T.SINCOS_ULP and ec.max() < T.SINCOS_ULP
    (o,) = probe(tmp_path, [(SINCOS, 1, 1, 0, 0.0, np.array([[np.inf], [-np.inf], [np.nan]]))])
    assert np.all(np.isnan(o))


# ---- wave_linalg.h ---------------------------------------------------------------------------------------------------
def test_eliminations_agree_on_ties_swaps_and_zero_pivots(tmp_path):
    """block_gepp_solve<256>, wave_gepp_solve and (n = 64) wave_gepp_solve_reg64: the same accept / refuse and the same x
    bits on every member -- the +-1 matrices (every pivot column all ties), the permutations (a swap at every step) and
    the zero pivots are where the pivot rule decides.  They refuse exactly when a pivot is <= 1e-8 max(1, max|A|), by a
    NumPy elimination with the same rule; a matrix beyond 1e150 is refused outright."""
    items = _square_items(F.SQUARE_N, lambda n: (0,))
    huge = _square_items((4, 64), lambda n: (500,))
    sections = []
    for n in F.SQUARE_N:
        for variant in (0, 1) + ((2,) if n == 64 else ()):
            sections.append((GEPP, n, n, variant, 0.0, _systems(items + huge, n)))
    outs = iter(probe(tmp_path, sections))
    wc = T.Worst()
    skipped = []
    for n in F.SQUARE_N:
        res = [next(outs) for _ in range(3 if n == 64 else 2)]
        for i, (_, name, k, a, b, x_exact) in enumerate([it for it in items + huge if it[0] == n]):
            tag = "elimination n=%d %s 2^%d" % (n, name, k)
            ok = [bool(r[i, 0]) for r in res]
            wc.require(len(set(ok)) == 1, tag, "accepted by some, refused by others: %r" % (ok,))
            wc.require(all(bits_equal(r[i, 1:], res[0][i, 1:]) for r in res[1:]), tag, "x bits differ among the eliminations")
            if k:
                wc.require(not any(ok), tag, "accepted although max|A| > 1e150")
                continue
            piv = F.gepp_pivots(a)
            tol = 1e-8 * max(1.0, float(np.max(np.abs(a))))
            if np.any((piv > tol / 4) & (piv < tol * 4)):
                skipped.append(tag)
                continue
            wc.require(ok[0] == bool(np.all(piv > tol)), tag, "accepted %s, smallest pivot %.3e, threshold %.3e" % (ok[0], piv.min(), tol))
            if ok[0]:
                T.check_solution(wc, tag, a, res[0][i, 1:], x_exact)
    assert len(skipped) <= 2, skipped
    wc.done()


BLOCK_SCALES = (-20, 0, 255, 500)  # (at 2^-100 and below every singular value is under the absolute 2.2e-16: rank 0 by design)


@pytest.mark.parametrize("size", F.SQUARE_N + (12,))
def test_block_pinv_solve_against_exact_solutions(tmp_path, size):
    """block_pinv_solve<256> and <64> (generic) on the square families, and the US kernels' <64, 12, 12> / <64, 9, 9>
    with LDA 13, at scales inside and outside the band of block_jacobi_prescale.

    What Hilbert 7 (cond2 4.8e8) found: with the rotation threshold 4e-15 at every size max|x - x_exact| was 1.614e-06
    against 10 eps cond2 = 1.056e-06; the threshold now follows the column length below 16 rows (jacobi_cos_floor)."""
    items = _square_items((size,), lambda n: BLOCK_SCALES)
    sections, keys = [], []
    for n in (size,):
        for variant in (0, 1) + ((2,) if n == 12 else (3,) if n == 9 else ()):
            sections.append((WPINV, n, n, variant, T.SV_EPS, _systems(items, n)))
            keys.append((n, variant))
    outs = probe(tmp_path, sections)
    wc = T.Worst()
    for (n, variant), o in zip(keys, outs):
        for (_, name, k, a, b, x_exact), row in zip([it for it in items if it[0] == n], o):
            tag = "block_pinv_solve variant %d n=%d %s 2^%d" % (variant, n, name, k)
            want, near = T.expected_rank(a)
            if near:
                continue
            wc.require(int(row[0]) == want, tag, "rank %d, by the 2.2e-16 threshold %d" % (row[0], want))
            if int(row[0]) == n:
                T.check_solution(wc, tag, a, row[1:1 + n], x_exact)
    wc.done()


def _jacobi_items(n):
    """the regular square members of size n and the rank-deficient ones (b = 0), at their own scale"""
    items = _square_items((n,), lambda n: (0,))
    if n >= 2:
        items += [(n, name, 0, a, np.zeros(n), None) for name, a in F.rank_deficient_by_one(n)]
    return items


def test_fixed_jacobi_is_the_generic_one(tmp_path):
    """block_jacobi_svd_fixed: "same arithmetic in the same order as block_jacobi_svd".  The order of a column pair's
    partial sums is set by the lanes per pair, so each fixed instantiation is compared with the generic code run with
    as many: <64, 12, 12> and <64, 9, 9> (8 lanes) with 256 threads, the plane phantom's <64, 31, 31> (4) with 128 and
    <256, 31, 31> (16) with 512.  Same sweep count, same U S and V bits, same rank and x bits -- also where the two
    forms of the rotation test, |ga| > f sqrt(al be) and ga^2 > f^2 al be, could part at a borderline."""
    sections, keys = [], []
    for n, generic, fixed in ((12, 0, 2), (9, 0, 3), (31, 6, 4), (31, 7, 5)):
        items = _jacobi_items(n)
        for routine in (JACOBI, WPINV):
            for variant in (generic, fixed):
                sections.append((routine, n, n, variant, T.SV_EPS, _systems(items, n)))
                keys.append((n, routine, variant, items))
    outs = probe(tmp_path, sections)
    wc = T.Worst()
    for i in range(0, len(keys), 2):
        n, routine, _, items = keys[i]
        for j, (_, name, k, a, b, x) in enumerate(items):
            tag = "%s n=%d variant %d %s" % ("sweeps" if routine == JACOBI else "pinv", n, keys[i + 1][2], name)
            g, f = outs[i][j], outs[i + 1][j]
            wc.require(g[0] == f[0], tag, "generic %d, fixed %d (%s)" % (g[0], f[0], "sweeps" if routine == JACOBI else "rank"))
            wc.require(bits_equal(g[1:], f[1:]), tag, "bits differ between generic and fixed")
    wc.done()


def test_jacobi_sweeps_end_before_the_limit(tmp_path):
    """The rotation threshold follows the column length below 16 rows (jacobi_cos_floor: 2.5e-16 m, at least 1.6e-15;
    without that floor a 3 x 3 matrix of rank 2 ran all 60 sweeps).  A threshold under the rounding floor would re-rotate noise up to the limit of 60 sweeps and only cost
    time, silently (a stalled run always reaches the limit): every member of every size ends before it, in the generic
    code and in the fixed sizes."""
    sections, keys = [], []
    for n in F.SQUARE_N + (12,):
        items = _jacobi_items(n)
        for variant in (0, 1) + {12: (2,), 9: (3,), 31: (4, 5)}.get(n, ()):
            sections.append((JACOBI, n, n, variant, 0.0, _systems(items, n)))
            keys.append((n, variant, items))
    outs = probe(tmp_path, sections)
    worst = {}
    bad = []
    for (n, variant, items), o in zip(keys, outs):
        worst[n] = max(worst.get(n, 0), int(o[:, 0].max()))
        bad += ["n=%d variant %d %s: %d sweeps" % (n, variant, it[1], sw) for it, sw in zip(items, o[:, 0]) if not sw < 60]
    print("block Jacobi, most sweeps per size:", worst)
    assert not bad, bad[:8]


def test_block_null_vector_on_rank_deficient_integers(tmp_path):
    """||A x|| <= C n eps ||A|| (infinity norms) and ||x||_2 = 1 on integer matrices of rank exactly n - 1: the generic
    code with 256 and 64 threads, and the plane phantom's <T, 31, 31> with LDA 31."""
    ns = [n for n in F.SQUARE_N if n >= 2]
    sections, keys = [], []
    for n in ns:
        mats = F.rank_deficient_by_one(n)
        sysn = np.array([np.concatenate([a.ravel(), np.zeros(n)]) for _, a in mats])
        for variant in (0, 1) + ((2, 3) if n == 31 else ()):
            sections.append((NULLVEC, n, n, variant, 0.0, sysn))
            keys.append((n, variant, mats))
    outs = probe(tmp_path, sections)
    wc = T.Worst()
    for (n, variant, mats), o in zip(keys, outs):
        for (name, a), row in zip(mats, o):
            tag = "block_null_vector variant %d n=%d %s" % (variant, n, name)
            x = row[1:].astype(T.LD)
            unit = n * F.EPS * float(np.max(np.sum(np.abs(a), axis=1)))
            wc.check("A x", tag, float(np.max(np.abs(a.astype(T.LD) @ x))), T.CJ * unit, unit)
            wc.check("|x| - 1", tag, abs(float(np.sqrt(x @ x)) - 1.0), T.CJ * n * F.EPS, n * F.EPS)
    wc.done()
