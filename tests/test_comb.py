"""CPU checks of the combination ranking behind lsqr_ransac_many_exhaustive (csrc/comb.h through the host-only
lsqr_comb_count / lsqr_comb_unrank): the order is the lexicographic order of the exhaustive overload
(computeAllChoices, RANSAC.hxx:197-213) = itertools.combinations, the counts are exact up to 64 bits, and a value that
does not fit is refused rather than wrapped."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

from lsqrrecipes_amd import _lib as L
from lsqrrecipes_amd import context as ctx_mod


def test_small_cases_enumerate_like_itertools():
    for n in range(1, 13):
        for k in range(1, min(n, 5) + 1):
            total = ctx_mod.comb_count(n, k)
            assert total == math.comb(n, k), (n, k)
            want = list(itertools.combinations(range(n), k))
            got = [tuple(int(x) for x in ctx_mod.comb_unrank(n, k, r)) for r in range(total)]
            assert got == want, (n, k)


@pytest.mark.parametrize("n,k", [(4_000_000, 3), (200, 9), (67, 33), (67, 34), (64, 64), (2 ** 32, 2), (100, 1)])
def test_large_counts_are_exact(n, k):
    assert math.comb(n, k) < 2 ** 64
    assert ctx_mod.comb_count(n, k) == math.comb(n, k)


@pytest.mark.parametrize("n,k", [(68, 34), (2 ** 32 - 17, 8), (2 ** 63, 3)])
def test_not_representable_is_refused(n, k):
    assert math.comb(n, k) >= 2 ** 64
    out = C.c_uint64(123)
    assert L.load().lsqr_comb_count(n, k, C.byref(out)) == L.ERR_INVALID
    with pytest.raises(L.LsqrError):
        ctx_mod.comb_count(n, k)
    sub = np.zeros(k, dtype=np.uint32)
    if n <= 2 ** 32:
        assert L.load().lsqr_comb_unrank(n, k, 0, L.ptr(sub)) == L.ERR_INVALID


def test_argument_errors():
    lib = L.load()
    out = C.c_uint64(0)
    sub = np.zeros(64, dtype=np.uint32)
    assert lib.lsqr_comb_count(10, 0, C.byref(out)) == L.ERR_INVALID
    assert lib.lsqr_comb_count(100, 65, C.byref(out)) == L.ERR_INVALID
    assert lib.lsqr_comb_count(10, 3, None) == L.ERR_INVALID
    assert lib.lsqr_comb_count(3, 5, C.byref(out)) == L.OK and out.value == 0   # k > n: no subset
    assert lib.lsqr_comb_unrank(10, 3, 120, L.ptr(sub)) == L.ERR_INVALID        # rank == C(10, 3)
    assert lib.lsqr_comb_unrank(3, 5, 0, L.ptr(sub)) == L.ERR_INVALID
    assert lib.lsqr_comb_unrank(10, 3, 0, None) == L.ERR_INVALID
    assert lib.lsqr_comb_unrank(2 ** 32 + 1, 1, 0, L.ptr(sub)) == L.ERR_INVALID  # indices are 32-bit


def _rank(n, sub):
    """lexicographic rank of an increasing k-subset of range(n), with Python integers"""
    k, r, prev = len(sub), 0, -1
    for i, a in enumerate(sub):
        for x in range(prev + 1, a) if a - prev < 64 else ():
            r += math.comb(n - 1 - x, k - 1 - i)
        if a - prev >= 64:   # the closed form of the same sum
            r += math.comb(n - 1 - prev, k - i) - math.comb(n - a, k - i)
        prev = a
    return r


@pytest.mark.parametrize("n,k", [(4_000_000, 3), (200, 9), (67, 33), (256, 4), (2 ** 32, 2), (5000, 5)])
def test_large_cases_first_last_and_round_trip(n, k):
    total = math.comb(n, k)
    assert list(ctx_mod.comb_unrank(n, k, 0)) == list(range(k))
    assert list(ctx_mod.comb_unrank(n, k, total - 1)) == list(range(n - k, n))
    g = np.random.default_rng(n % 1000 + k)
    ranks = [1, total - 2, total // 2, total // 3] + [int(g.integers(0, total, dtype=np.uint64)) for _ in range(200)]
    for r in ranks:
        sub = [int(x) for x in ctx_mod.comb_unrank(n, k, r)]
        assert all(0 <= a < n for a in sub) and all(a < b for a, b in zip(sub, sub[1:])), (r, sub)
        assert _rank(n, sub) == r, (r, sub)
    # consecutive ranks are consecutive subsets
    r0 = total // 2
    a, b = ctx_mod.comb_unrank(n, k, r0), ctx_mod.comb_unrank(n, k, r0 + 1)
    assert tuple(a) < tuple(b)
