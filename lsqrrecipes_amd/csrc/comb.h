// comb.h -- ranking of k-subsets for the exhaustive RANSAC overload (RANSAC.hxx:150-249), compiled for host and device
// like ctr_subset.  computeAllChoices (RANSAC.hxx:197-213) visits the k-subsets of {0..n-1} in lexicographic order
// with increasing indices; comb_unrank returns the rank-th of them directly, so that a lane can take hypothesis
// `rank` without the walk from rank 0 and the host can turn a winner's rank back into its subset.
//
// Arithmetic: 64-bit only (no 128-bit products or divisions, which the device has no library for).  C(n,k) is built
// as C(n-k+i, i), i = 1..k, each step dividing before it multiplies: with g = gcd(m, i), m = n-k+i, the old value is
// divisible by i/g, so the step is (c / (i/g)) * (m/g), exact, and its one product overflows exactly when C(n-k+i, i)
// does.  These values grow with i, so no intermediate exceeds the result: "does not fit" is reported when, and only
// when, C(n,k) itself does not fit.
#pragma once
#include <stdint.h>

#include "sampler.h"

namespace lsqr {

// C(n,k) -> *out; false when it does not fit in 64 bits (k > n: 0)
LSQR_HD bool comb_count(uint64_t n, int k, uint64_t *out) {
  if (k < 0 || (uint64_t)k > n) {
    *out = 0;
    return true;
  }
  if ((uint64_t)k > n - (uint64_t)k) k = (int)(n - (uint64_t)k);  // C(n,k) = C(n,n-k): the shorter product
  uint64_t c = 1;
  for (int i = 1; i <= k; i++) {
    uint64_t m = n - (uint64_t)k + (uint64_t)i;
    uint64_t a = m % (uint64_t)i, b = (uint64_t)i;  // gcd(m, i)
    while (a) {
      const uint64_t t = b % a;
      b = a;
      a = t;
    }
    m /= b;
    c /= (uint64_t)i / b;
    if (mulhi64(c, m)) return false;
    c *= m;
  }
  *out = c;
  return true;
}

// the rank-th k-subset of {0..n-1} (rank < C(n,k), which fits in 64 bits; 1 <= k <= 64) in lexicographic order,
// idx[0] < idx[1] < ... .  With r' = C(n,k) - 1 - rank the subset is the combinatorial number system's
// r' = C(c_k, k) + ... + C(c_1, 1), c_k > ... > c_1 >= 0, mirrored: idx[k - j] = n - 1 - c_j.  c_j is the largest c
// below c_{j+1} with C(c, j) <= r', found by bisection (a C(c, j) that does not fit is larger than r').
LSQR_HD void comb_unrank(uint64_t n, int k, uint64_t rank, uint32_t *idx) {
  uint64_t total = 0;
  comb_count(n, k, &total);
  uint64_t r = total - 1 - rank;
  uint64_t top = n;  // c_j < top
  for (int j = k; j >= 1; j--) {
    uint64_t lo = (uint64_t)j - 1, hi = top - 1;  // C(j-1, j) = 0 <= r always; the answer lies in [lo, hi]
    uint64_t clo = 0;
    if (j == 1) {  // C(c, 1) = c
      lo = r < hi ? r : hi;
      clo = lo;
    }
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo + 1) / 2;
      uint64_t cm;
      if (comb_count(mid, j, &cm) && cm <= r) {
        lo = mid;
        clo = cm;
      } else {
        hi = mid - 1;
      }
    }
    r -= clo;
    top = lo;
    idx[k - j] = (uint32_t)(n - 1 - lo);
  }
}

// comb_unrank from a table of binomials, for a caller that unranks many subsets of one n: tab[c * k + (j - 1)] =
// C(c, j) for c < n, 1 <= j <= k (every entry fits: c < n, and the caller's C(n,k) does); total = C(n,k).  The same
// bisection over the same values, so the same subset, with lookups in place of comb_count's divisions.
LSQR_HD void comb_unrank_tab(uint32_t n, int k, uint64_t rank, uint64_t total, const uint64_t *tab, uint32_t *idx) {
  uint64_t r = total - 1 - rank;
  uint32_t top = n;
  for (int j = k; j >= 1; j--) {
    uint32_t lo = (uint32_t)j - 1, hi = top - 1;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo + 1) / 2;
      if (tab[(size_t)mid * k + (j - 1)] <= r) lo = mid;
      else hi = mid - 1;
    }
    r -= tab[(size_t)lo * k + (j - 1)];
    top = lo;
    idx[k - j] = n - 1 - lo;
  }
}

}  // namespace lsqr
