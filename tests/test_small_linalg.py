"""The small dense solvers of lsqrrecipes_amd/csrc/small_linalg.h, compiled for the host (tests/host_math/driver.cpp,
-ffp-contract=off), on the structured and badly scaled families of tests/linalg_families.py: a solver answers
correctly or says it cannot -- it never reports success with a wrong answer.

The bounds are the backward-error bounds of cyclic Jacobi, C n eps max|A| with C = 8, checked in long double so that
the check's own rounding stays out of them.  tests/test_gpu_small_linalg.py runs the same checks on the device's output
and compares its bits with this host build's.

Measured, identically on the host and on the device (worst over all members and scales, in units of n eps max|A|,
bound 8): sym_eig orthogonality 3.1, residual 2.1, eigenvalues 6.5 (n = 64, clustered); svd_jacobi V orthogonality 1.3,
reconstruction 1.6, singular values 0.6; spd_solve_eig residual 0.33.  lsqr_sincos against 80-bit long double:
1.46 ulp (sin) and 1.42 ulp (cos) over +-8.2e5, 1.34 / 1.41 over +-4; the header states 2.

What n = 64 found: sym_eig's test off <= 1e-34 dg is below the rounding floor of a matrix with a repeated eigenvalue
(off / dg settles at 2e-34 ... 6e-34), so the all-ones and the clustered matrix ran to the 64-sweep limit -- 125 000
rotations of noise -- and reached 10.7 n eps in V^T V - I and 11.8 in the eigenvalues.  sym_eig now stops when a sweep
below 1e-30 dg gains less than a factor 4."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import linalg_families as F

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "lsqrrecipes_amd", "csrc")

CJ = 8  # the constant of every Jacobi bound below: C n eps max|A|
EPS = F.EPS
LD = np.longdouble
SV_EPS = 2.2e-16  # the reference's absolute rank threshold (zero_out_absolute)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Host:
    """small_linalg.h through the host driver; every call works on copies."""

    def __init__(self, lib):
        self.lib = lib
        lib.hm_sym_eig.restype = None
        lib.hm_svd_jacobi.restype = None
        lib.hm_sincos.restype = None

    def sym_eig(self, a):
        n = a.shape[0]
        a = np.ascontiguousarray(a, dtype=np.float64).copy()
        w, v = np.zeros(n), np.zeros((n, n))
        self.lib.hm_sym_eig(n, _p(a), _p(w), _p(v))
        return w, v

    def svd(self, a):
        m, n = a.shape
        u = np.ascontiguousarray(a, dtype=np.float64).copy()
        s, v = np.zeros(n), np.zeros((n, n))
        self.lib.hm_svd_jacobi(m, n, _p(u), _p(s), _p(v))
        return u, s, v

    def pinv_solve(self, a, b, tol=SV_EPS):
        m, n = a.shape
        a = np.ascontiguousarray(a, dtype=np.float64).copy()
        b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.zeros(n)
        rank = self.lib.hm_pinv_solve(m, n, _p(a), _p(b), C.c_double(tol), _p(x))
        return rank, x

    def spd_solve_chol(self, g, rhs, fill=np.nan):
        n = g.shape[0]
        g = np.ascontiguousarray(g, dtype=np.float64)
        rhs = np.ascontiguousarray(rhs, dtype=np.float64)
        x = np.full(n, fill)
        ok = self.lib.hm_spd_solve_chol(n, _p(g), _p(rhs), _p(x))
        return bool(ok), x

    def spd_solve_eig(self, g, rhs, rtol=1e-13):
        n = g.shape[0]
        g = np.ascontiguousarray(g, dtype=np.float64).copy()
        rhs = np.ascontiguousarray(rhs, dtype=np.float64)
        x = np.zeros(n)
        rank = self.lib.hm_spd_solve_eig(n, _p(g), _p(rhs), C.c_double(rtol), _p(x))
        return rank, x

    def sincos(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        s, c = np.zeros_like(x), np.zeros_like(x)
        self.lib.hm_sincos(_p(x), C.c_size_t(len(x)), _p(s), _p(c))
        return s, c


_HOST = {}


def build_host(tmp_path_factory, csrc=CSRC):
    """The host driver against the headers in csrc, built once per session in pytest's own temporary directory
    (tests/test_gpu_small_linalg.py shares it)."""
    if csrc not in _HOST:
        out = str(tmp_path_factory.mktemp("hostmath") / "libhostmath.so")
        subprocess.check_call(["g++", "-std=c++20", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-w",
                               "-I", csrc, "-o", out, os.path.join(HERE, "host_math", "driver.cpp")])
        _HOST[csrc] = Host(C.CDLL(out))
    return _HOST[csrc]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory)


# ---- the checks, shared with the device tests ------------------------------------------------------------------------
class Worst:
    """Collects failures (so that one run names every failing member) and the worst figure per quantity."""

    def __init__(self):
        self.fail, self.worst = [], {}

    def check(self, what, tag, value, bound, unit=None):
        if unit:
            self.worst[what] = max(self.worst.get(what, 0.0), float(value) / unit)
        if not value <= bound:
            self.fail.append("%s %s: %.3e > %.3e" % (tag, what, value, bound))

    def require(self, cond, tag, what):
        if not cond:
            self.fail.append("%s %s" % (tag, what))

    def done(self):
        print("worst, in units of the bound's n eps max|A|:", {k: round(v, 3) for k, v in self.worst.items()})
        assert not self.fail, "%d failures, first: %s" % (len(self.fail), "; ".join(self.fail[:8]))


def check_sym_eig(wc, tag, a, w, v):
    """a as given to sym_eig (any scale), its w and v."""
    n = a.shape[0]
    au, e = F.unit_scale(a)
    amax = float(np.max(np.abs(au)))
    unit = n * EPS * max(amax, 1.0) if amax == 0.0 else n * EPS * amax
    wc.require(np.all(np.isfinite(w)) and np.all(np.isfinite(v)), tag, "not finite")
    if not (np.all(np.isfinite(w)) and np.all(np.isfinite(v))):
        return
    wu = np.ldexp(w, -e)
    wc.require(np.all(np.diff(w) >= 0), tag, "w not ascending")
    vl, al = v.astype(LD), au.astype(LD)
    wc.check("orthogonality", tag, float(np.max(np.abs(vl.T @ vl - np.eye(n)))), CJ * n * EPS, n * EPS)
    wc.check("residual", tag, float(np.max(np.abs(al @ vl - vl * wu.astype(LD)[None, :]))), CJ * unit, unit)
    wc.check("eigenvalues", tag, float(np.max(np.abs(wu - np.linalg.eigvalsh(au)))), CJ * unit, unit)


def check_svd(wc, tag, a, u, s, v, info):
    m, n = a.shape
    au, e = F.unit_scale(a)
    amax = float(np.max(np.abs(au)))
    unit = n * EPS * amax
    ok = np.all(np.isfinite(u)) and np.all(np.isfinite(s)) and np.all(np.isfinite(v))
    wc.require(ok, tag, "not finite")
    if not ok:
        return
    su = np.ldexp(s, -e)
    smax = float(np.max(su))
    ul, vl = u.astype(LD), v.astype(LD)
    wc.check("V orthogonality", tag, float(np.max(np.abs(vl.T @ vl - np.eye(n)))), CJ * n * EPS, n * EPS)
    # a column whose singular value is rounding noise (a duplicated column's partner) has a direction that is noise too
    live = su > CJ * n * EPS * smax
    ug = ul[:, live]
    wc.check("U orthonormality", tag, float(np.max(np.abs(ug.T @ ug - np.eye(ug.shape[1])))) if ug.size else 0.0,
             CJ * max(m, n) * EPS, max(m, n) * EPS)
    wc.check("reconstruction", tag, float(np.max(np.abs((ul * su.astype(LD)[None, :]) @ vl.T - au.astype(LD)))),
             CJ * unit, unit)
    sref = np.linalg.svd(au, compute_uv=False)
    wc.check("singular values", tag, float(np.max(np.abs(np.sort(su)[::-1] - sref))), CJ * n * EPS * smax, n * EPS * smax)
    if "zero_column" in info:
        wc.require(s[info["zero_column"]] == 0.0 and np.all(u[:, info["zero_column"]] == 0.0), tag, "zero column: s != 0")
    if info.get("duplicated"):
        wc.check("duplicated s_min", tag, float(np.min(su)), CJ * n * EPS * smax)


def check_solution(wc, tag, a, x, x_exact, what="x"):
    ok = np.all(np.isfinite(x))
    wc.require(ok, tag, what + " not finite")
    if ok:
        wc.check(what, tag, float(np.max(np.abs(x - x_exact))), F.pinv_bound(a, x_exact))


def expected_rank(a, tol=SV_EPS):
    """(rank by the absolute threshold from LAPACK's singular values, whether one of them is within 2x of it)."""
    au, e = F.unit_scale(a)
    with np.errstate(over="ignore", under="ignore"):
        s = np.ldexp(np.linalg.svd(au, compute_uv=False), e)
    return int(np.sum(s > tol)), bool(np.any((s > tol / 2) & (s < tol * 2)))


def scales_for(n):
    return F.SCALES  # every scale at every size; F.scaled() drops the ones a member cannot take


def ulp_error(got, ref_ld):
    ref = ref_ld.astype(np.float64)
    return np.abs(got.astype(LD) - ref_ld) / np.spacing(np.maximum(np.abs(ref), F.TINY)).astype(LD)


# ---- sym_eig ---------------------------------------------------------------------------------------------------------
def run_sym_eig(sym_eig, members, scales_of=scales_for):
    wc = Worst()
    for n, name, a, _ in members:
        w0, v0 = sym_eig(a)
        for k in scales_of(n):
            ak = F.scaled(a, k)
            if ak is None:
                continue
            tag = "sym_eig n=%d %s 2^%d" % (n, name, k)
            w, v = (w0, v0) if k == 0 else sym_eig(ak)
            check_sym_eig(wc, tag, ak, w, v)
            if k:
                wc.require(np.array_equal(v, v0), tag, "v differs from the unscaled run's")
                with np.errstate(under="ignore"):
                    wk = np.ldexp(w0, k)
                exact = (np.abs(wk) >= F.TINY) | (w0 == 0)
                wc.require(np.array_equal(w[exact], wk[exact]), tag, "w is not 2^k times the unscaled run's")
    return wc


@pytest.mark.parametrize("n", sorted(set(m[0] for m in F.symmetric_all())))
def test_sym_eig_families_and_scales(host, n):
    run_sym_eig(host.sym_eig, [m for m in F.symmetric_all() if m[0] == n]).done()


def test_sym_eig_clustered_subspace(host):
    """A clustered spectrum pins invariant subspaces, not vectors: the projector on each cluster's vectors is the exact
    one to the bound of the residual over the gap (Davis-Kahan), here gap = 1."""
    wc = Worst()
    for n in F.SYM_N:
        if n < 4:
            continue
        lam = F.clustered_spectrum(n)
        a = dict((nm, m) for nm, m, _ in F.symmetric(n))["clustered"]
        w, v = host.sym_eig(a)
        wref, vref = np.linalg.eigh(a)
        for val in np.unique(lam):
            sel = np.abs(wref - val) < 0.25
            got = np.abs(w - val) < 0.25
            wc.require(sel.sum() == got.sum(), "n=%d cluster %g" % (n, val), "multiplicity differs")
            if sel.sum() == got.sum():
                pr, pg = vref[:, sel] @ vref[:, sel].T, v[:, got] @ v[:, got].T
                wc.check("projector", "n=%d cluster %g" % (n, val), float(np.max(np.abs(pr - pg))), 4 * CJ * n * EPS * 5.0)
    wc.done()


# ---- svd_jacobi ------------------------------------------------------------------------------------------------------
def run_svd(svd, members, scales_of=scales_for):
    wc = Worst()
    for m, n, name, a, info in members:
        u0, s0, v0 = svd(a)
        for k in scales_of(n):
            ak = F.scaled(a, k)
            if ak is None:
                continue
            tag = "svd %dx%d %s 2^%d" % (m, n, name, k)
            u, s, v = (u0, s0, v0) if k == 0 else svd(ak)
            check_svd(wc, tag, ak, u, s, v, info)
            if k:
                wc.require(np.array_equal(v, v0) and np.array_equal(u, u0), tag, "u or v differs from the unscaled run's")
    return wc


def test_svd_jacobi_families_and_scales(host):
    run_svd(host.svd, F.tall_all()).done()


# ---- pinv_solve ------------------------------------------------------------------------------------------------------
def test_numpy_solve_meets_the_bound_on_every_member():
    """The bound asked of the solvers is one a backward-stable solve can meet: LAPACK's does, on every member."""
    wc = Worst()
    for n in F.SQUARE_N:
        for name, a, b, x in F.square(n):
            check_solution(wc, "n=%d %s" % (n, name), a, np.linalg.solve(a, b), x)
    wc.done()


def run_pinv(pinv_solve, ns=F.SQUARE_N, scales_of=scales_for):
    wc = Worst()
    for n in ns:
        for name, a, b, x_exact in F.square(n):
            for k in scales_of(n):
                ak, bk = F.scaled(a, k), F.scaled(b, k)
                if ak is None or bk is None:
                    continue
                tag = "pinv_solve n=%d %s 2^%d" % (n, name, k)
                want, near = expected_rank(ak)
                if near:
                    continue
                rank, x = pinv_solve(ak, bk)
                wc.require(rank == want, tag, "rank %d, by the 2.2e-16 threshold %d" % (rank, want))
                if k >= 0:
                    wc.require(want == n, tag, "a regular member below the threshold at its own scale")
                if rank == n:
                    check_solution(wc, tag, ak, x, x_exact)
    return wc


def test_pinv_solve_square_families_and_scales(host):
    run_pinv(host.pinv_solve).done()


# ---- spd_solve_chol / spd_solve_eig ----------------------------------------------------------------------------------
def ld_solve(g, rhs):
    """Gaussian elimination with partial pivoting in long double."""
    n = len(rhs)
    m = np.hstack([g.astype(LD), rhs.astype(LD)[:, None]])
    for k in range(n):
        p = k + int(np.argmax(np.abs(m[k:, k])))
        m[[k, p]] = m[[p, k]]
        m[k + 1:] -= (m[k + 1:, k] / m[k, k])[:, None] * m[k][None, :]
    x = np.zeros(n, dtype=LD)
    for k in range(n - 1, -1, -1):
        x[k] = (m[k, n] - m[k, k + 1:n] @ x[k + 1:]) / m[k, k]
    return x


def spd_members():
    """[(n, name, G, rhs, exact rank, x0)]: the integer Gram matrices with a consistent right-hand side G x0."""
    out = []
    for n, name, a, info in F.symmetric_all():
        if "gram" in info:
            x0 = F._rng(6, n).integers(-3, 4, size=n).astype(np.float64)
            out.append((n, name, a, a @ x0, info["rank"], x0))
    return out


def run_spd(chol, eig, scales=(-600, -300, 0, 300, 500)):
    wc = Worst()
    for n, name, g, rhs, r, x0 in spd_members():
        for k in scales:
            gk, rk = F.scaled(g, k), F.scaled(rhs, k)
            if gk is None or rk is None:
                continue
            tag = "spd n=%d %s 2^%d" % (n, name, k)
            rank, x = eig(gk, rk)
            wc.require(rank == r, tag, "spd_solve_eig rank %d, exact %d" % (rank, r))
            gu = F.unit_scale(g)[0].astype(LD)
            ru = np.ldexp(rhs, -F.unit_scale(g)[1]).astype(LD)
            unit = n * EPS * float(np.max(np.sum(np.abs(gu), axis=1))) * max(float(np.max(np.abs(x))), F.TINY)
            wc.check("eig residual", tag, float(np.max(np.abs(gu @ x.astype(LD) - ru))), CJ * unit, unit)
            ok, xc = chol(gk, rk, 7.5)
            if r < n:
                wc.require(not ok and np.all(xc == 7.5), tag, "spd_solve_chol accepted a singular matrix or wrote x")
                continue
            d = 1.0 / np.sqrt(np.diag(g))
            cond = np.linalg.cond(g * d[:, None] * d[None, :])
            ref = ld_solve(F.unit_scale(g)[0], np.ldexp(rhs, -F.unit_scale(g)[1]))
            bound = 10 * EPS * cond * float(np.max(np.abs(ref))) * float(np.max(d) / np.min(d))
            wc.check("eig solution", tag, float(np.max(np.abs(x.astype(LD) - ref))), bound)
            if cond < 1e6:  # every pivot of the unit-diagonal matrix is >= its smallest eigenvalue >= 1 / cond
                wc.require(ok, tag, "spd_solve_chol refused a well-conditioned matrix")
            if ok:
                wc.check("chol solution", tag, float(np.max(np.abs(xc.astype(LD) - ref))), bound)
    return wc


def test_spd_solvers_on_gram_families(host):
    run_spd(host.spd_solve_chol, host.spd_solve_eig).done()


def rho_family():
    """[[1, rho], [rho, 1]]: the second pivot is 1 - rho^2 in exactly this arithmetic."""
    rhos = [0.0, 0.5, -0.5]
    for t in (4e-8, 1.0000001e-8, 1.000000000001e-8, 1e-8, 0.999999999999e-8, 0.9999999e-8, 2.5e-9, 1e-12):
        r = np.sqrt(1.0 - t)
        rhos += [r, -r, np.nextafter(r, 0.0), np.nextafter(r, 1.0)]
    rhos += [1.0, -1.0]
    return np.array(rhos)


def run_chol_threshold(chol):
    wc = Worst()
    accepted = refused = 0
    for rho in rho_family():
        g = np.array([[1.0, rho], [rho, 1.0]])
        rhs = np.array([1.0, 2.0])
        want = (1.0 - rho * rho) > 1e-8
        ok, x = chol(g, rhs, -3.25)
        tag = "chol rho=%.17g" % rho
        wc.require(ok == want, tag, "accepted %s, pivot 1 - rho^2 = %.17g" % (ok, 1.0 - rho * rho))
        if ok:
            accepted += 1
            ref = np.array([1.0 - 2.0 * rho, 2.0 - rho], dtype=LD) / (LD(1.0) - LD(rho) * LD(rho))
            wc.check("x", tag, float(np.max(np.abs(x - ref))), 10 * EPS * (1 + abs(rho)) / (1 - abs(rho)) * float(np.max(np.abs(ref))))
        else:
            refused += 1
            wc.require(np.all(x == -3.25), tag, "x written although refused")
    assert accepted >= 10 and refused >= 10
    return wc


def test_spd_solve_chol_refuses_exactly_at_the_pivot_threshold(host):
    run_chol_threshold(host.spd_solve_chol).done()


# ---- lsqr_sincos -----------------------------------------------------------------------------------------------------
SINCOS_ULP = 2.0  # small_linalg.h: "Error < 2 ulp for |x| < 8.2e5"


def sincos_sets():
    g = F._rng(7)
    k = np.arange(-520000, 520001, 37, dtype=np.float64)
    near = k * (np.pi / 2)
    moved = []
    for d in range(-3, 4):
        x = near.copy()
        for _ in range(abs(d)):
            x = np.nextafter(x, np.inf if d > 0 else -np.inf)
        moved.append(x)
    q = np.pi / 4
    quarter = [q]
    for _ in range(4):
        quarter = [np.nextafter(quarter[0], 0.0)] + quarter + [np.nextafter(quarter[-1], 1.0)]
    quarter = np.array(quarter)
    return {
        "uniform +-8.2e5": g.uniform(-8.2e5, 8.2e5, size=400_000),
        "uniform +-4": g.uniform(-4.0, 4.0, size=400_000),
        "k pi/2 +-3 ulp": np.concatenate(moved),
        "neighbours of +-pi/4": np.concatenate([quarter, -quarter]),
        "just under 8.2e5": np.array([np.nextafter(8.2e5, 0.0), -np.nextafter(8.2e5, 0.0), 8.1e5, 819999.5]),
    }


def run_sincos(sincos):
    worst = {}
    fail = []
    for name, x in sincos_sets().items():
        x = x[np.abs(x) < 8.2e5]
        s, c = sincos(x)
        es, ec = ulp_error(s, np.sin(x.astype(LD))), ulp_error(c, np.cos(x.astype(LD)))
        worst[name] = (float(es.max()), float(ec.max()))
        if not (es.max() < SINCOS_ULP and ec.max() < SINCOS_ULP):
            i = int(np.argmax(np.maximum(es, ec)))
            fail.append("%s: %.3f / %.3f ulp, worst at x = %r" % (name, es.max(), ec.max(), float(x[i])))
        s2, c2 = sincos(-x)
        if not (np.array_equal(s2.view(np.uint64), (-s).view(np.uint64)) and np.array_equal(c2.view(np.uint64), c.view(np.uint64))):
            fail.append("%s: sin(-x) = -sin(x), cos(-x) = cos(x) not bit for bit" % name)
    print("lsqr_sincos, worst ulp error (sin, cos):", {k: (round(a, 3), round(b, 3)) for k, (a, b) in worst.items()})
    # zeros keep their sign; subnormals and tiny arguments return themselves
    z = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2e-308, -2.2e-308, 1e-300, -1e-300])
    s, c = sincos(z)
    if not np.array_equal(s.view(np.uint64), z.view(np.uint64)):
        fail.append("sin of zeros / subnormals: %r" % (s,))
    if not np.all(c == 1.0):
        fail.append("cos of zeros / subnormals: %r" % (c,))
    # 8.2e5 and beyond: the platform's functions, which are good to an ulp
    big = np.array([8.2e5, -8.2e5, np.nextafter(8.2e5, np.inf), 1e6, -3e9, 1e22, 1e300])
    s, c = sincos(big)
    es, ec = ulp_error(s, np.sin(big.astype(LD))), ulp_error(c, np.cos(big.astype(LD)))
    if not (es.max() < 1.0 and ec.max() < 1.0):
        fail.append("beyond 8.2e5: %.3f / %.3f ulp" % (es.max(), ec.max()))
    with np.errstate(invalid="ignore"):
        s, c = sincos(np.array([np.inf, -np.inf, np.nan]))
    if not (np.all(np.isnan(s)) and np.all(np.isnan(c))):
        fail.append("inf / nan: %r %r" % (s, c))
    return worst, fail


def test_lsqr_sincos_meets_the_bound_of_its_header(host):
    with open(os.path.join(CSRC, "small_linalg.h")) as f:
        assert "Error < 2 ulp for |x| < 8.2e5" in f.read()  # SINCOS_ULP is the header's figure
    worst, fail = run_sincos(host.sincos)
    assert not fail, "; ".join(fail)
