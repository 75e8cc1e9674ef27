// computeManyRigidTest -- RANSAC<T,S>::computeMany against compute() for the closed-form estimators with record types
// of their own: absolute orientation (std::pair<Point3D,Point3D>), pivot calibration (Frame), ray intersection (Ray3D)
// and the 2-D line (Point2D).  Problem j of one computeMany call must give what compute() gives on data[j] after
// seed(seed() + j) -- fraction, consensus set and parameters (the latter to reordered fp64 sums) -- including a
// problem too small for a minimal subset.  Exit code 0 == all passed.
#include <cmath>
#include <cstdio>
#include <random>
#include <utility>
#include <vector>

#include "AbsoluteOrientationParametersEstimator.h"
#include "Line2DParametersEstimator.h"
#include "PivotCalibrationParametersEstimator.h"
#include "RANSAC.h"
#include "RayIntersectionParametersEstimator.h"

using namespace lsqrRecipes;

static int failures = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                   \
    }                                                               \
  } while (0)

static std::mt19937_64 gen(4051);
static double U(double a, double b) { return std::uniform_real_distribution<double>(a, b)(gen); }
static double G(double s) { return std::normal_distribution<double>(0.0, s)(gen); }

// a random unit quaternion [s, qx, qy, qz] and its rotation matrix (Frame.cxx's formula)
static void random_rotation(double q[4], double R[9]) {
  double n = 0;
  for (int i = 0; i < 4; i++) q[i] = G(1.0), n += q[i] * q[i];
  n = std::sqrt(n);
  for (int i = 0; i < 4; i++) q[i] /= n;
  const double s = q[0], x = q[1], y = q[2], z = q[3];
  const double M[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - s * z),     2 * (x * z + s * y),
                       2 * (x * y + s * z),     1 - 2 * (x * x + z * z), 2 * (y * z - s * x),
                       2 * (x * z - s * y),     2 * (y * z + s * x),     1 - 2 * (x * x + y * y)};
  for (int i = 0; i < 9; i++) R[i] = M[i];
}

typedef std::pair<Point3D, Point3D> PairT;

static std::vector<PairT> absor_problem(size_t n, double inliers) {
  double q[4], R[9], t[3];
  random_rotation(q, R);
  for (int i = 0; i < 3; i++) t[i] = U(-500, 500);
  std::vector<PairT> d(n);
  for (size_t m = 0; m < n; m++) {
    for (int i = 0; i < 3; i++) d[m].first[i] = U(-100, 100);
    const bool out = U(0, 1) > inliers;
    for (int i = 0; i < 3; i++) {
      double v = t[i] + G(0.2);
      for (int k = 0; k < 3; k++) v += R[3 * i + k] * d[m].first[k];
      d[m].second[i] = out ? v + U(5, 50) : v;
    }
  }
  return d;
}

static std::vector<Frame> pivot_problem(size_t n, double inliers) {
  const double tip[3] = {-17.0, 1.0, -157.0}, piv[3] = {147.0, -63.0, -1042.0};
  std::vector<Frame> d(n);
  for (size_t m = 0; m < n; m++) {
    double q[4], R[9], t[3];
    random_rotation(q, R);
    const bool out = U(0, 1) > inliers;
    for (int i = 0; i < 3; i++) {
      t[i] = piv[i] + G(0.15) + (out ? U(-40, 40) : 0.0);
      for (int k = 0; k < 3; k++) t[i] -= R[3 * i + k] * tip[k];
    }
    d[m] = Frame(t[0], t[1], t[2], q[0], q[1], q[2], q[3]);
  }
  return d;
}

static std::vector<Ray3D> ray_problem(size_t n, double inliers) {
  double target[3];
  for (int i = 0; i < 3; i++) target[i] = U(-1000, 1000);
  std::vector<Ray3D> d(n);
  for (size_t m = 0; m < n; m++) {
    const bool out = U(0, 1) > inliers;
    Vector3D dir;
    for (int i = 0; i < 3; i++) {
      d[m].p[i] = U(-1000, 1000);
      dir[i] = (out ? U(-1000, 1000) : target[i] + G(0.3)) - d[m].p[i];
    }
    dir.normalize();
    d[m].n = dir;
  }
  return d;
}

static std::vector<Point2D> line2d_problem(size_t n, double inliers) {
  const double a[2] = {U(-100, 100), U(-100, 100)}, ang = U(0, 3.14159265358979);
  std::vector<Point2D> d(n);
  for (size_t m = 0; m < n; m++) {
    const double s = U(-200, 200);
    const bool out = U(0, 1) > inliers;
    d[m][0] = out ? U(-300, 300) : a[0] + s * std::cos(ang) + G(0.1);
    d[m][1] = out ? U(-300, 300) : a[1] + s * std::sin(ang) + G(0.1);
  }
  return d;
}

// kind: 0 absolute orientation (q ~ -q), 1 pivot, 2 ray, 3 2-D line (the normal's sign is arbitrary)
template <class T, class Est, class Gen>
static void compare(const char *name, Est &est, int kind, Gen make) {
  std::vector<std::vector<T> > data;
  const size_t k = est.numForEstimate();
  data.push_back(make(k - 1, 1.0));  // too small: 0, parameters untouched
  for (int j = 0; j < 40; j++) data.push_back(make(k + 37 * (size_t)j, 0.5 + 0.012 * j));
  std::vector<std::vector<double> > params;
  std::vector<std::vector<bool> > sets;
  params.resize(1);
  params[0].assign(3, 42.0);
  RANSAC<T, double>::seed() = 11;
  std::vector<double> frac = RANSAC<T, double>::computeMany(params, &est, data, 0.999, &sets);
  CHECK(frac.size() == data.size() && params.size() == data.size() && sets.size() == data.size());
  CHECK(frac[0] == 0.0 && params[0].size() == 3 && params[0][0] == 42.0);
  int ok = 0;
  for (size_t j = 1; j < data.size(); j++) {
    RANSAC<T, double>::seed() = 11 + j;
    std::vector<double> p1;
    std::vector<bool> s1;
    const double f1 = RANSAC<T, double>::compute(p1, &est, data[j], 0.999, &s1);
    CHECK(f1 == frac[j]);
    CHECK(s1 == sets[j]);
    CHECK(p1.size() == params[j].size());
    if (p1.size() != params[j].size()) continue;
    const int ns = kind == 0 ? 4 : kind == 3 ? 2 : 0;  // leading entries whose joint sign is arbitrary
    double dot = 0;
    for (int i = 0; i < ns && i < (int)p1.size(); i++) dot += p1[i] * params[j][i];
    const double sgn = dot < 0 ? -1.0 : 1.0;
    bool close = true;
    for (size_t i = 0; i < p1.size(); i++) {
      const double g = (int)i < ns ? sgn * params[j][i] : params[j][i];
      close = close && std::fabs(g - p1[i]) <= 1e-9 * std::fmax(1.0, std::fabs(p1[i]));
    }
    CHECK(close);
    ok += !p1.empty();
  }
  CHECK(ok > 30);
  RANSAC<T, double>::seed() = 1;
  std::printf("%s: %d of %zu problems fitted, computeMany == compute\n", name, ok, data.size() - 1);
}

int main() {
  AbsoluteOrientationParametersEstimator absor(1.0);
  PivotCalibrationEstimator pivot(1.0);
  RayIntersectionParametersEstimator ray(1.0, 0.017453292519943295);
  Line2DParametersEstimator line2d(0.5);
  compare<PairT>("absolute orientation", absor, 0, absor_problem);
  compare<Frame>("pivot calibration", pivot, 1, pivot_problem);
  compare<Ray3D>("ray intersection", ray, 2, ray_problem);
  compare<Point2D>("2-D line", line2d, 3, line2d_problem);
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
