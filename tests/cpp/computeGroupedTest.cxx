// computeGroupedTest -- RANSAC<T,S>::computeGrouped against the call it replaces: computeMany on the per-group vectors
// (the stable gather by label of the resident records) with the same seed().  Fractions, parameters and the consensus
// (scattered back to record order) must be equal, exactly: the device call runs the same batched job on the same packed
// bytes.  Plane, the default (geometric) sphere, a user-defined estimator without a device model (the host loop), labels
// outside [0, nGroups), an empty group and a group below the minimal subset.  Exit code 0 == all passed.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

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
static std::mt19937_64 gen(2027);
static double U(double a, double b) { return std::uniform_real_distribution<double>(a, b)(gen); }

// nGroups planes (kind 0) or spheres (kind 1), one per label, 70 % of a group's records on its model; the labels are
// interleaved; group 1 is empty, group 2 has two records; every 97th record carries a label outside [0, nGroups)
static void scene(int kind, size_t n, size_t nGroups, std::vector<P3> &pts, std::vector<int> &groups) {
  std::vector<double> a(3 * nGroups), u(3 * nGroups), v(3 * nGroups), r(nGroups);
  for (size_t j = 0; j < nGroups; j++) {
    for (int i = 0; i < 3; i++) a[3 * j + i] = U(-100, 100), u[3 * j + i] = U(-1, 1), v[3 * j + i] = U(-1, 1);
    r[j] = U(20, 60);
  }
  pts.resize(n);
  groups.resize(n);
  size_t in2 = 0;
  for (size_t m = 0; m < n; m++) {
    size_t j = (m * 7 + m / 13) % nGroups;
    if (j == 1) j = 0;
    if (j == 2 && in2++ >= 2) j = 3;
    groups[m] = m % 97 == 5 ? (m % 2 ? -1 : (int)nGroups + (int)(m % 3)) : (int)j;
    double d[3], len = 0;
    const double s = U(-80, 80), t = U(-80, 80);
    for (int i = 0; i < 3; i++) d[i] = U(-1, 1), len += d[i] * d[i];
    for (int i = 0; i < 3; i++) {
      if (m % 10 >= 7) pts[m][i] = U(-200, 200);
      else if (kind == 0) pts[m][i] = a[3 * j + i] + s * u[3 * j + i] + t * v[3 * j + i] + U(-0.1, 0.1);
      else pts[m][i] = a[3 * j + i] + r[j] * d[i] / std::sqrt(len) + U(-0.1, 0.1);
    }
  }
}

// a user-defined estimator (no device model): a 2-D line [n, a] on the user's own point type
struct UserPoint2D {
  double x, y;
};
class UserLine2D : public ParametersEstimator<UserPoint2D, double> {
 public:
  UserLine2D(double delta) : ParametersEstimator<UserPoint2D, double>(2), d2(delta * delta) {}
  virtual void estimate(std::vector<UserPoint2D *> &data, std::vector<double> &p) {
    p.clear();
    if (data.size() < 2) return;
    double nx = data[1]->y - data[0]->y, ny = data[0]->x - data[1]->x;
    double norm = std::sqrt(nx * nx + ny * ny);
    if (norm < 2.220446049250313e-16) return;
    p.push_back(nx / norm);
    p.push_back(ny / norm);
    p.push_back(data[0]->x);
    p.push_back(data[0]->y);
  }
  virtual void estimate(std::vector<UserPoint2D> &data, std::vector<double> &p) {
    std::vector<UserPoint2D *> q;
    for (size_t i = 0; i < data.size(); i++) q.push_back(&data[i]);
    estimate(q, p);
  }
  virtual void leastSquaresEstimate(std::vector<UserPoint2D *> &data, std::vector<double> &p) {
    p.clear();
    if (data.size() < 2) return;
    double mx = 0, my = 0, sxx = 0, sxy = 0, syy = 0;
    for (size_t i = 0; i < data.size(); i++) mx += data[i]->x, my += data[i]->y;
    mx /= data.size(), my /= data.size();
    for (size_t i = 0; i < data.size(); i++) {
      double dx = data[i]->x - mx, dy = data[i]->y - my;
      sxx += dx * dx, sxy += dx * dy, syy += dy * dy;
    }
    double th = 0.5 * std::atan2(2 * sxy, sxx - syy);
    p.push_back(-std::sin(th));
    p.push_back(std::cos(th));
    p.push_back(mx);
    p.push_back(my);
  }
  virtual void leastSquaresEstimate(std::vector<UserPoint2D> &data, std::vector<double> &p) {
    std::vector<UserPoint2D *> q;
    for (size_t i = 0; i < data.size(); i++) q.push_back(&data[i]);
    leastSquaresEstimate(q, p);
  }
  virtual bool agree(std::vector<double> &p, UserPoint2D &d) {
    double s = p[0] * (d.x - p[2]) + p[1] * (d.y - p[3]);
    return s * s < d2;
  }
  double d2;
};

// computeGrouped on the resident records against computeMany on the per-group vectors
template <class T, class Est>
static void compare(const char *name, Est &est, const std::vector<T> &data, const std::vector<int> &groups,
                    size_t nGroups, uint64_t seed0) {
  std::vector<std::vector<T> > sets(nGroups);
  std::vector<std::vector<size_t> > index(nGroups);
  for (size_t i = 0; i < data.size(); i++)
    if (groups[i] >= 0 && (size_t)groups[i] < nGroups) {
      sets[(size_t)groups[i]].push_back(data[i]);
      index[(size_t)groups[i]].push_back(i);
    }
  RANSAC<T, double>::seed() = seed0;
  std::vector<std::vector<double> > pm, pg;
  std::vector<std::vector<bool> > cm;
  std::vector<double> fm = RANSAC<T, double>::computeMany(pm, &est, sets, 0.999, &cm);
  std::vector<bool> want(data.size(), false), cg;
  for (size_t g = 0; g < nGroups; g++)
    for (size_t q = 0; q < cm[g].size(); q++) want[index[g][q]] = cm[g][q];
  ResidentData<T> res(data);
  size_t found = 0;
  for (int rep = 0; rep < 2; rep++) {  // (the second call finds the records and the buffers in place)
    std::vector<double> fg = RANSAC<T, double>::computeGrouped(pg, &est, res, groups, nGroups, 0.999, &cg);
    CHECK(fg == fm);
    CHECK(pg == pm);
    CHECK(cg == want);
  }
  for (size_t g = 0; g < nGroups; g++) found += pm[g].empty() ? 0 : 1;
  CHECK(found >= nGroups - 2);                      // every group but the empty and the two-record one
  CHECK(pm[1].empty() && fm[1] == 0 && fm[2] == 0);
  CHECK((RANSAC<T, double>::seed() == seed0));
  // invalid input: nothing runs
  std::vector<double> fz = RANSAC<T, double>::computeGrouped(pg, &est, res, groups, nGroups, 1.5, &cg);
  CHECK(fz == std::vector<double>(nGroups, 0.0) && cg == std::vector<bool>(data.size(), false));
  std::printf("%s: %zu groups, %zu models, computeGrouped == computeMany on the gather\n", name, nGroups, found);
  RANSAC<T, double>::seed() = 1;
}

int main() {
  PlaneParametersEstimator<3> plane(0.5);
  SphereParametersEstimator<3> sphere(0.5);  // lsType = GEOMETRIC, the reference's default
  std::vector<P3> pts;
  std::vector<int> groups;
  scene(0, 6007, 9, pts, groups);
  compare("plane", plane, pts, groups, 9, 5);
  scene(1, 6007, 9, pts, groups);
  compare("sphere (geometric)", sphere, pts, groups, 9, 7);
  // the host loop: a user-defined estimator on three lines, labels by line
  std::vector<UserPoint2D> l2(3001);
  std::vector<int> g2(l2.size());
  const double nx[3] = {0.6, -0.8, 0.0}, ny[3] = {0.8, 0.6, 1.0}, ax[3] = {5, -40, 0}, ay[3] = {-7, 30, 90};
  for (size_t m = 0; m < l2.size(); m++) {
    const int j = (int)(m % 4);  // 1 is left empty, 2 gets one record (below the line's two)
    g2[m] = m % 97 == 5 ? -1 : (j == 1 ? 0 : (j == 2 && m > 4 ? 3 : j));
    const int line = g2[m] < 0 ? 0 : g2[m] % 3;
    double x = U(-300, 300), y = U(-300, 300);
    if (m % 10 < 7) {
      const double d = (x - ax[line]) * nx[line] + (y - ay[line]) * ny[line];
      x += -d * nx[line] + U(-0.1, 0.1), y += -d * ny[line] + U(-0.1, 0.1);
    }
    l2[m].x = x, l2[m].y = y;
  }
  UserLine2D user(0.5);
  compare("user-defined 2-D line (host loop)", user, l2, g2, 4, 9);
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
