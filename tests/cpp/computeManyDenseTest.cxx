// computeManyDenseTest -- RANSAC<T,S>::computeMany against compute() for DenseLinearEquationSystemParametersEstimator
// <double,3> and <double,20>: problem j of one computeMany call must give what compute() gives on data[j] after
// seed(seed() + j) -- fraction and consensus set exactly, parameters within 1e-9 relative (the final fit's fp64 sums
// are ordered differently) -- including a problem too small for a minimal subset.
// Exit code 0 == all passed.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "DenseLinearEquationSystemParametersEstimator.h"
#include "RANSAC.h"

using namespace lsqrRecipes;

static int failures = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                   \
    }                                                               \
  } while (0)

static std::mt19937_64 gen(2026);
static double U(double a, double b) { return std::uniform_real_distribution<double>(a, b)(gen); }

// rows a^T x = b (1e-3 relative noise on b), a share of the right-hand sides scaled by 20 (outliers)
template <unsigned N>
static std::vector<AugmentedRow<double, N> > rows(size_t m, double inliers) {
  double x[N];
  for (unsigned i = 0; i < N; i++) x[i] = U(-1, 1);
  std::vector<AugmentedRow<double, N> > r(m);
  for (size_t k = 0; k < m; k++) {
    double a[N], b = 0;
    for (unsigned i = 0; i < N; i++) a[i] = U(-1, 1), b += a[i] * x[i];
    b *= 1.0 + U(-1e-3, 1e-3);
    if (U(0, 1) > inliers) b *= 20.0;
    r[k].set(a, b);
  }
  return r;
}

template <unsigned N>
static void compare(const char *name, int count, double out_max) {
  typedef AugmentedRow<double, N> RT;
  DenseLinearEquationSystemParametersEstimator<double, N> est(0.1);
  std::vector<std::vector<RT> > data;
  data.push_back(std::vector<RT>(N - 1));  // too small (k = n): 0, parameters untouched
  for (int j = 0; j < count; j++) data.push_back(rows<N>(3 * N + 61 * (size_t)j, 1.0 - out_max * (j % 5) / 4.0));
  std::vector<std::vector<double> > params;
  std::vector<std::vector<bool> > sets;
  params.resize(1);
  params[0].assign(3, 42.0);
  RANSAC<RT, double>::seed() = 7;
  std::vector<double> frac = RANSAC<RT, double>::computeMany(params, &est, data, 0.999, &sets);
  CHECK(frac.size() == data.size() && params.size() == data.size() && sets.size() == data.size());
  CHECK(frac[0] == 0.0 && params[0].size() == 3 && params[0][0] == 42.0);
  int ok = 0;
  for (size_t j = 1; j < data.size(); j++) {
    RANSAC<RT, double>::seed() = 7 + j;
    std::vector<double> p1;
    std::vector<bool> s1;
    const double f1 = RANSAC<RT, double>::compute(p1, &est, data[j], 0.999, &s1);
    CHECK(f1 == frac[j]);
    CHECK(s1 == sets[j]);
    CHECK(p1.size() == params[j].size());
    if (p1.size() != params[j].size()) continue;
    bool close = true;
    for (size_t i = 0; i < p1.size(); i++)
      close = close && std::fabs(params[j][i] - p1[i]) <= 1e-9 * std::fmax(1.0, std::fabs(p1[i]));
    CHECK(close);
    ok += (int)(p1.size() == N);
  }
  CHECK(ok > count - 3);
  RANSAC<RT, double>::seed() = 1;
  std::printf("%s: %d of %zu problems fitted, computeMany == compute\n", name, ok, data.size() - 1);
}

int main() {
  compare<3>("dense n = 3", 40, 0.3);
  compare<20>("dense n = 20", 16, 0.08);
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
