// computeManyGeometricTest -- RANSAC<T,S>::computeMany against compute() for default-constructed (GEOMETRIC)
// SphereParametersEstimator<3> and <2>: problem j of one computeMany call must give what compute() gives on data[j]
// after seed(seed() + j) -- fraction and consensus set exactly, parameters within 1e-9 relative (the LM runs from
// fits whose fp64 sums are ordered differently) -- including a problem too small for a minimal subset.
// Exit code 0 == all passed.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "RANSAC.h"
#include "SphereParametersEstimator.h"

using namespace lsqrRecipes;

static int failures = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                   \
    }                                                               \
  } while (0)

static std::mt19937_64 gen(2025);
static double U(double a, double b) { return std::uniform_real_distribution<double>(a, b)(gen); }

// points near a D-sphere, a share of them replaced by uniform outliers
template <unsigned D>
static std::vector<Point<double, D> > cloud(size_t n, double inliers) {
  double c[D];
  for (unsigned i = 0; i < D; i++) c[i] = U(-100, 100);
  const double r = U(10, 50);
  std::vector<Point<double, D> > pts(n);
  for (size_t m = 0; m < n; m++) {
    double d[D], len = 0;
    for (unsigned i = 0; i < D; i++) d[i] = U(-1, 1), len += d[i] * d[i];
    const bool out = U(0, 1) > inliers;
    for (unsigned i = 0; i < D; i++) {
      double x = c[i] + r * d[i] / std::sqrt(len) + U(-0.1, 0.1);
      if (out) x = c[i] + U(-80, 80);
      pts[m][i] = x;
    }
  }
  return pts;
}

template <unsigned D>
static void compare(const char *name) {
  typedef Point<double, D> PT;
  SphereParametersEstimator<D> est(0.5);  // lsType = GEOMETRIC, the reference's default
  std::vector<std::vector<PT> > data;
  data.push_back(std::vector<PT>(D));  // too small (k = D + 1): 0, parameters untouched
  for (int j = 0; j < 40; j++) data.push_back(cloud<D>(50 + 97 * (size_t)j, 0.45 + 0.012 * j));
  std::vector<std::vector<double> > params;
  std::vector<std::vector<bool> > sets;
  params.resize(1);
  params[0].assign(3, 42.0);
  RANSAC<PT, double>::seed() = 7;
  std::vector<double> frac = RANSAC<PT, double>::computeMany(params, &est, data, 0.999, &sets);
  CHECK(frac.size() == data.size() && params.size() == data.size() && sets.size() == data.size());
  CHECK(frac[0] == 0.0 && params[0].size() == 3 && params[0][0] == 42.0);
  int ok = 0;
  for (size_t j = 1; j < data.size(); j++) {
    RANSAC<PT, double>::seed() = 7 + j;
    std::vector<double> p1;
    std::vector<bool> s1;
    const double f1 = RANSAC<PT, double>::compute(p1, &est, data[j], 0.999, &s1);
    CHECK(f1 == frac[j]);
    CHECK(s1 == sets[j]);
    CHECK(p1.size() == params[j].size());
    if (p1.size() != params[j].size()) continue;
    bool close = true;
    for (size_t i = 0; i < p1.size(); i++)
      close = close && std::fabs(params[j][i] - p1[i]) <= 1e-9 * std::fmax(1.0, std::fabs(p1[i]));
    CHECK(close);
    ok += !p1.empty();
  }
  CHECK(ok > 30);
  RANSAC<PT, double>::seed() = 1;
  std::printf("%s: %d of %zu problems fitted, computeMany == compute\n", name, ok, data.size() - 1);
}

int main() {
  compare<3>("sphere (geometric)");
  compare<2>("circle (geometric)");
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
