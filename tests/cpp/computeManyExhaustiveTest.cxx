// computeManyExhaustiveTest -- the exhaustive RANSAC<T,S>::computeMany (no probability argument) against the
// exhaustive compute(): for the plane, the line and the default (GEOMETRIC) sphere, problem j of one computeMany call
// must give what compute(parameters, estimator, data[j], consensusSet) gives -- fraction and consensus set exactly,
// parameters to reordered fp64 sums (sphere: within the LM tolerances) -- including problems too small for a minimal
// subset (0, parameters cleared) and the loop taken under forceHostLoop().  Exit code 0 == all passed.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "LineParametersEstimator.h"
#include "PlaneParametersEstimator.h"
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

typedef Point<double, 3> P3;
static std::mt19937_64 gen(2026);
static double U(double a, double b) { return std::uniform_real_distribution<double>(a, b)(gen); }

// points near a plane (kind 0), a sphere (1) or a line (2), a share of them replaced by uniform outliers
static std::vector<P3> cloud(int kind, size_t n, double inliers) {
  double a[3], u[3], v[3];
  for (int i = 0; i < 3; i++) a[i] = U(-100, 100), u[i] = U(-1, 1), v[i] = U(-1, 1);
  const double r = U(10, 50);
  std::vector<P3> pts(n);
  for (size_t m = 0; m < n; m++) {
    const double s = U(-50, 50), t = U(-50, 50);
    double d[3];
    double len = 0;
    for (int i = 0; i < 3; i++) d[i] = U(-1, 1), len += d[i] * d[i];
    const bool out = U(0, 1) > inliers;
    for (int i = 0; i < 3; i++) {
      double x = kind == 0 ? a[i] + s * u[i] + t * v[i] : kind == 1 ? a[i] + r * d[i] / std::sqrt(len) : a[i] + s * u[i];
      x += U(-0.1, 0.1);
      if (out) x = U(-150, 150);
      pts[m][i] = x;
    }
  }
  return pts;
}

template <class Est>
static void compare(const char *name, Est &est, int kind, bool hostLoop) {
  std::vector<std::vector<P3> > data;
  const size_t k = est.numForEstimate();
  data.push_back(std::vector<P3>(k - 1));  // too small: 0, parameters cleared (RANSAC.hxx:165-169)
  data.push_back(std::vector<P3>());
  for (int j = 0; j < (hostLoop ? 6 : 60); j++) data.push_back(cloud(kind, k + (size_t)(j % 30), 0.5 + 0.008 * j));
  std::vector<std::vector<double> > params;
  std::vector<std::vector<bool> > sets;
  params.resize(2);
  params[0].assign(3, 42.0);
  params[1].assign(3, 42.0);
  RANSAC<P3, double>::forceHostLoop() = hostLoop;
  std::vector<double> frac = RANSAC<P3, double>::computeMany(params, &est, data, &sets);
  CHECK(frac.size() == data.size() && params.size() == data.size() && sets.size() == data.size());
  CHECK(frac[0] == 0.0 && params[0].empty() && frac[1] == 0.0 && params[1].empty());
  int ok = 0;
  for (size_t j = 2; j < data.size(); j++) {
    std::vector<double> p1;
    std::vector<bool> s1;
    const double f1 = RANSAC<P3, double>::compute(p1, &est, data[j], &s1);
    CHECK(f1 == frac[j]);
    CHECK(s1 == sets[j]);
    CHECK(p1.size() == params[j].size());
    if (p1.size() != params[j].size()) continue;
    double sgn = 1.0;
    if (kind != 1) {  // plane normal / line direction: the sign is arbitrary
      double dot = 0;
      for (int i = 0; i < 3; i++) dot += p1[i] * params[j][i];
      sgn = dot < 0 ? -1.0 : 1.0;
    }
    bool close = true;
    for (size_t i = 0; i < p1.size(); i++) {
      const double got = (kind != 1 && i < 3) ? sgn * params[j][i] : params[j][i];
      // (sphere: the LM bounds of the batched geometric fit, rtol 1e-9 and atol 1e-8)
      const double tol = kind == 1 ? 1e-9 * std::fabs(p1[i]) + 1e-8 : 1e-9 * std::fmax(1.0, std::fabs(p1[i]));
      close = close && std::fabs(got - p1[i]) <= tol;
    }
    CHECK(close);
    ok += !p1.empty();
  }
  RANSAC<P3, double>::forceHostLoop() = false;
  CHECK(ok > (hostLoop ? 3 : 30));
  std::printf("%s%s: %d of %zu problems fitted, computeMany == compute\n", name, hostLoop ? " (host loop)" : "", ok,
              data.size() - 2);
}

int main() {
  PlaneParametersEstimator<3> plane(0.5);
  LineParametersEstimator<3> line(0.5);
  SphereParametersEstimator<3> sphere(0.5);  // lsType = GEOMETRIC, the reference's default
  compare("plane", plane, 0, false);
  compare("line", line, 2, false);
  compare("sphere (geometric)", sphere, 1, false);
  compare("plane", plane, 0, true);
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
