"""Matrix families for the small dense solvers (csrc/small_linalg.h, csrc/wave_linalg.h): structure and scale
at which an elimination or a Jacobi iteration goes wrong without a random matrix ever noticing.  A plain module,
imported by the CPU tests (tests/test_small_linalg.py) and the GPU tests (tests/test_gpu_small_linalg.py,
tests/test_gpu_dense_structured.py), so that every layer sees the same inputs.  Every generator is seeded and returns
float64 arrays; the square systems come with their exact solution."""
from fractions import Fraction

import numpy as np

EPS = np.finfo(np.float64).eps
TINY = np.finfo(np.float64).tiny

SYM_N = (1, 2, 3, 4, 6, 8, 13, 31, 64)
SQUARE_N = (1, 2, 3, 4, 7, 8, 9, 31, 32, 33, 63, 64)
TALL_SHAPES = ((3, 2), (9, 6), (12, 12), (70, 7), (64, 64))
SCALES = (-600, -520, -300, -100, 0, 100, 255, 300, 500, 530)


def scaled(a, k):
    """2^k a, or None when the product is not exact: an entry overflows, or a non-zero entry leaves the normal range."""
    with np.errstate(over="ignore", under="ignore"):
        s = np.ldexp(np.asarray(a, dtype=np.float64), k)
    nz = s != 0
    if not np.all(np.isfinite(s)) or np.any((np.asarray(a) != 0) & ~nz) or np.any(np.abs(s[nz]) < TINY):
        return None
    return s


def unit_scale(a):
    """(a 2^-e, e) with max|a 2^-e| in [1, 2); e = 0 for a zero matrix."""
    amax = float(np.max(np.abs(a))) if a.size else 0.0
    if amax == 0.0 or not np.isfinite(amax):
        return a.copy(), 0
    e = int(np.frexp(amax)[1]) - 1
    return np.ldexp(a, -e), e


def _rng(*key):
    return np.random.default_rng([20260, *key])


def _orth(g, n):
    q, r = np.linalg.qr(g.normal(size=(n, n)))
    return q * np.sign(np.diag(r))


def _from_spectrum(g, lam):
    q = _orth(g, len(lam))
    a = (q * np.asarray(lam, dtype=np.float64)) @ q.T
    return (a + a.T) / 2


def clustered_spectrum(n):
    """(1, 1, 1, 1, 2, 2, 2, 5) at n = 8 and its analogue elsewhere: half ones, the rest twos, one five."""
    lam = np.ones(n)
    lam[n // 2:] = 2.0
    lam[-1] = 5.0 if n > 1 else 1.0
    return lam


def wilkinson(m=10):
    """W(2m+1)+: diagonal |m|, ..., 1, 0, 1, ..., |m|, ones beside it; its largest eigenvalues come in close pairs."""
    n = 2 * m + 1
    a = np.diag(np.abs(np.arange(-m, m + 1)).astype(np.float64))
    a += np.diag(np.ones(n - 1), 1) + np.diag(np.ones(n - 1), -1)
    return a


def int_matrix_of_rank(g, rows, cols, r, lo=-3, hi=3):
    """rows x cols small integers of rank exactly r (r <= min(rows, cols)): an r-row block and integer combinations."""
    for _ in range(100):
        base = g.integers(lo, hi + 1, size=(r, cols)).astype(np.float64)
        if np.linalg.matrix_rank(base) != r:
            continue
        if rows == r:
            return base
        mix = g.integers(-1, 2, size=(rows - r, r)).astype(np.float64)
        b = np.vstack([base, mix @ base])
        if np.linalg.matrix_rank(b) == r:
            return b
    raise AssertionError("no integer matrix of rank %d found" % r)


def symmetric(n):
    """[(name, A, info)]: info['rank'] where the exact rank is known (integer Gram matrices), info['gram'] = B."""
    g = _rng(1, n)
    out = []
    b = g.normal(size=(n, n))
    out.append(("random", b + b.T, {}))
    out.append(("diagonal", np.diag(g.normal(size=n) * 3.0), {}))
    out.append(("ones", np.ones((n, n)), {"rank": 1}))
    out.append(("zero", np.zeros((n, n)), {"rank": 0}))
    u = g.integers(-3, 4, size=n).astype(np.float64)
    u[0] = 2.0
    out.append(("rank_one", np.outer(u, u), {"rank": 1}))
    out.append(("clustered", _from_spectrum(g, clustered_spectrum(n)), {}))
    out.append(("negative", _from_spectrum(g, -np.linspace(0.5, 3.0, n)), {}))
    if n >= 2:
        out.append(("exchange", np.fliplr(np.eye(n)), {}))  # [[0, 1], [1, 0]] at n = 2
        out.append(("graded", _from_spectrum(g, np.logspace(-12, 9, n)), {}))
        out.append(("mixed_signs", _from_spectrum(g, np.linspace(-3.0, 2.0, n)), {}))
        r = max(1, n // 2)
        bb = int_matrix_of_rank(g, r, n, r)
        out.append(("gram_rank%d" % r, bb.T @ bb, {"rank": r, "gram": bb}))
    bb = int_matrix_of_rank(g, n + 2, n, n)  # two rows more than columns: SPD with a moderate condition number
    out.append(("gram_full", bb.T @ bb, {"rank": n, "gram": bb}))
    return out


def symmetric_all():
    """[(n, name, A, info)] over SYM_N, plus Wilkinson's W21+."""
    out = [(n, name, a, info) for n in SYM_N for name, a, info in symmetric(n)]
    out.append((21, "wilkinson21", wilkinson(10), {}))
    return out


def hadamard(n):
    h = np.ones((1, 1))
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    assert h.shape[0] == n
    return h


def _regular_ints(g, n, lo, hi, fix=None, values=None):
    for _ in range(1000):
        a = (g.choice(values, size=(n, n)) if values is not None else g.integers(lo, hi + 1, size=(n, n))).astype(np.float64)
        if fix is not None:
            fix(a)
        if np.linalg.cond(a) < 1e6:
            return a
    raise AssertionError("no regular integer matrix found")


def fraction_solve(a, b):
    """The exact solution of the float system a x = b by elimination in rationals, rounded to float64 at the end."""
    n = len(b)
    m = [[Fraction(float(a[i, j])) for j in range(n)] + [Fraction(float(b[i]))] for i in range(n)]
    for k in range(n):
        p = next(i for i in range(k, n) if m[i][k] != 0)
        m[k], m[p] = m[p], m[k]
        for i in range(k + 1, n):
            f = m[i][k] / m[k][k]
            if f:
                m[i] = [u - f * v for u, v in zip(m[i], m[k])]
    x = [Fraction(0)] * n
    for k in range(n - 1, -1, -1):
        x[k] = (m[k][n] - sum(m[k][j] * x[j] for j in range(k + 1, n))) / m[k][k]
    return np.array([float(v) for v in x])


def square(n):
    """[(name, A, b, x_exact)]: regular n x n systems.  Except for Hilbert, entries and solution are small integers
    (times powers of two in the graded members), so b = A @ x is exact in float64."""
    g = _rng(2, n)
    x = g.integers(1, 4, size=n).astype(np.float64) * g.choice([-1.0, 1.0], size=n)
    mats = [("identity", np.eye(n)),
            ("permutation", np.eye(n)[g.permutation(n)]),
            ("reversal", np.fliplr(np.eye(n))),
            ("lower_ones", np.tril(np.ones((n, n)))),
            ("upper_ones", np.triu(np.ones((n, n))))]
    if n & (n - 1) == 0:
        mats.append(("hadamard", hadamard(n)))
    else:
        mats.append(("pm_one", _regular_ints(g, n, 0, 0, values=[-1.0, 1.0])))
    ints = _regular_ints(g, n, -4, 4)
    mats.append(("integers", ints))
    if n >= 2:
        def zero00(a):
            a[0, 0] = 0.0
        mats.append(("zero_pivot", _regular_ints(g, n, -4, 4, fix=zero00)))
    if n >= 4:
        def zero_block(a):
            a[:2, :2] = 0.0
        mats.append(("zero_block", _regular_ints(g, n, -4, 4, fix=zero_block)))
    if n >= 2:
        # two levels, 2^+20 and 2^-20, alternating: the small pivots (~4e-6) are four orders below the eliminations'
        # threshold 1e-8 max|A| (4e-2), so what they refuse does not hang on a rounding
        e = np.where(np.arange(n) % 2 == 0, 20, -20)
        mats.append(("row_graded", np.ldexp(ints, e[:, None])))
        mats.append(("col_graded", np.ldexp(ints, e[None, :])))
    out = []
    for name, a in mats:
        b = a @ x
        out.append((name, a, b, x.copy()))
    if 2 <= n <= 7:
        i = np.arange(n)
        h = 1.0 / (i[:, None] + i[None, :] + 1.0)
        b = h @ np.ones(n)
        out.append(("hilbert", h, b, fraction_solve(h, b)))
    return out


def singular_square(n):
    """[(name, A, b)]: the two exactly singular systems the dense tests admit -- a zero column and a repeated row."""
    g = _rng(3, n)
    a = _regular_ints(g, n, -4, 4)
    x = g.integers(1, 4, size=n).astype(np.float64)
    z = a.copy()
    z[:, n // 2] = 0.0
    r = a.copy()
    r[n - 1] = r[0]
    return [("zero_column", z, z @ x), ("repeated_row", r, r @ x)] if n >= 2 else [("zero_column", z, z @ x)]


def rank_deficient_by_one(n):
    """[(name, A)]: n x n small integers of rank exactly n - 1 (for the null vector), n >= 2."""
    g = _rng(4, n)
    a = int_matrix_of_rank(g, n, n, n - 1)
    out = [("dependent_rows", a[g.permutation(n)]), ("dependent_columns", a.T.copy())]
    z = _regular_ints(g, n, -4, 4)
    z[:, n // 3] = 0.0
    if np.linalg.matrix_rank(z) == n - 1:
        out.append(("zero_column", z))
    return out


def tall(m, n):
    """[(name, A, info)] for the one-sided Jacobi SVD: info names the structure to assert on."""
    g = _rng(5, m, n)
    out = [("random", g.normal(size=(m, n)), {})]
    a = g.integers(-4, 5, size=(m, n)).astype(np.float64)
    out.append(("integers", a, {}))
    z = a.copy()
    z[:, n // 2] = 0.0
    out.append(("zero_column", z, {"zero_column": n // 2}))
    d = a.copy()
    d[:, n - 1] = d[:, 0]
    out.append(("duplicated_column", d, {"duplicated": True}))
    q, _ = np.linalg.qr(g.normal(size=(m, n)))
    out.append(("orthogonal", q * np.arange(1, n + 1), {}))
    sel = np.zeros((m, n))
    sel[g.permutation(m)[:n], np.arange(n)] = np.arange(1, n + 1) * g.choice([-1.0, 1.0], size=n)
    out.append(("orthogonal_exact", sel, {}))  # one entry per column: no rotation at all
    return out


def tall_all():
    return [(m, n, name, a, info) for m, n in TALL_SHAPES for name, a, info in tall(m, n)]


def gepp_pivots(a):
    """|pivots| of Gaussian elimination with partial pivoting by the solvers' rule: the entry of largest |a| in the
    column at or below the diagonal, ties to the lower row.  Plain float64, no fma: within rounding of the device's."""
    a = np.array(a, dtype=np.float64)
    n = a.shape[0]
    piv = np.zeros(n)
    for k in range(n):
        col = np.abs(a[k:, k])
        p = k + int(np.argmax(col))  # argmax returns the first of equal maxima: the lower row
        piv[k] = col[p - k]
        if piv[k] == 0.0:
            break
        if p != k:
            a[[k, p]] = a[[p, k]]
        f = a[k + 1:, k] / a[k, k]
        a[k + 1:, k:] -= f[:, None] * a[k, k:][None, :]
    return piv


def pinv_bound(a, x_exact):
    """The bound on max|x - x_exact| of the pseudo-inverse solves and the eliminations: the suite's own 1e-8
    (_dense_close) or 10 eps cond2(A) (tests/test_gpu_dense_cond.py), relative to max(1, max|x_exact|)."""
    au, _ = unit_scale(a)
    return max(1e-8, 10 * EPS * np.linalg.cond(au)) * max(1.0, float(np.max(np.abs(x_exact))))
