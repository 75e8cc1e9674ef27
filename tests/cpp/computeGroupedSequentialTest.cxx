// computeGroupedSequentialTest -- RANSAC<T,S>::computeGroupedSequential against the call it replaces:
// computeManySequential on the per-group vectors (the stable gather by label of the resident records) with the same
// seed().  Fractions, parameters and the labels (scattered back to record order) must be equal, exactly: the device
// call runs the same rounds on the same packed bytes.  Plane (batched: one device call), a user-defined estimator
// without a device model (the fallback through computeManySequential), labels outside [0, nGroups), an empty group
// and a group below the minimal subset.  Exit code 0 == all passed.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "PlaneParametersEstimator.h"
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

typedef Point<double, 3> P3;
static std::mt19937_64 gen(2028);
static double U(double a, double b) { return std::uniform_real_distribution<double>(a, b)(gen); }

// every group holds three planes of 3/10 of its records each and 1/10 clutter; the labels are interleaved; group 1 is
// empty, group 2 has two records; every 97th record carries a label outside [0, nGroups)
static void planes(size_t n, size_t nGroups, std::vector<P3> &pts, std::vector<int> &groups) {
  std::vector<double> a(9 * nGroups), u(9 * nGroups), v(9 * nGroups);
  for (size_t e = 0; e < 9 * nGroups; e++) a[e] = U(-100, 100), u[e] = U(-1, 1), v[e] = U(-1, 1);
  pts.resize(n);
  groups.resize(n);
  size_t in2 = 0;
  for (size_t m = 0; m < n; m++) {
    size_t j = (m * 7 + m / 13) % nGroups;
    if (j == 1) j = 0;
    if (j == 2 && in2++ >= 2) j = 3;
    groups[m] = m % 97 == 5 ? (m % 2 ? -1 : (int)nGroups + (int)(m % 3)) : (int)j;
    const size_t which = (m / nGroups) % 10;  // 0..8: plane which / 3 of the group; 9: clutter
    const size_t q = 9 * j + 3 * (which / 3);
    const double s = U(-80, 80), t = U(-80, 80);
    for (int i = 0; i < 3; i++)
      pts[m][i] = which == 9 ? U(-200, 200) : a[q + i] + s * u[q + i] + t * v[q + i] + U(-0.1, 0.1);
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

// computeGroupedSequential on the resident records against computeManySequential on the per-group vectors
template <class T, class Est>
static void compare(const char *name, Est &est, const std::vector<T> &data, const std::vector<int> &groups,
                    size_t nGroups, uint64_t seed0, size_t maxModels, size_t minVotes) {
  typedef RANSAC<T, double> R;
  std::vector<std::vector<T> > sets(nGroups);
  std::vector<std::vector<size_t> > index(nGroups);
  for (size_t i = 0; i < data.size(); i++)
    if (groups[i] >= 0 && (size_t)groups[i] < nGroups) {
      sets[(size_t)groups[i]].push_back(data[i]);
      index[(size_t)groups[i]].push_back(i);
    }
  R::seed() = seed0;
  std::vector<std::vector<std::vector<double> > > pm, pg;
  std::vector<std::vector<int> > lm;
  std::vector<std::vector<double> > fm = R::computeManySequential(pm, &est, sets, 0.999, maxModels, minVotes, &lm);
  std::vector<int> want(data.size(), -1), lg;
  for (size_t g = 0; g < nGroups; g++)
    for (size_t q = 0; q < lm[g].size(); q++) want[index[g][q]] = lm[g][q];
  ResidentData<T> res(data);
  for (int rep = 0; rep < 2; rep++) {  // (the second call finds the records and the buffers in place)
    std::vector<std::vector<double> > fg =
        R::computeGroupedSequential(pg, &est, res, groups, nGroups, 0.999, maxModels, minVotes, &lg);
    CHECK(fg == fm);
    CHECK(pg == pm);
    CHECK(lg == want);
  }
  // without labels: the same decisions
  std::vector<std::vector<std::vector<double> > > pn;
  CHECK(R::computeGroupedSequential(pn, &est, res, groups, nGroups, 0.999, maxModels, minVotes) == fm && pn == pm);
  size_t several = 0, models = 0, claimed = 0;
  for (size_t g = 0; g < nGroups; g++) several += pm[g].size() >= 2 ? 1 : 0, models += pm[g].size();
  for (size_t i = 0; i < want.size(); i++) claimed += want[i] >= 1 ? 1 : 0;
  CHECK(several >= nGroups - 2);  // every group but the empty and the too small one yields several models
  CHECK(claimed > 0);             // and rounds after the first claimed records
  CHECK(pm[1].empty() && fm[1].empty() && pm[2].empty() && fm[2].empty());
  CHECK((R::seed() == seed0));
  // invalid input and maxModels == 0: nothing runs
  std::vector<std::vector<double> > fz =
      R::computeGroupedSequential(pg, &est, res, groups, nGroups, 1.5, maxModels, minVotes, &lg);
  CHECK(fz == std::vector<std::vector<double> >(nGroups) && lg == std::vector<int>(data.size(), -1));
  CHECK(pg == std::vector<std::vector<std::vector<double> > >(nGroups));
  fz = R::computeGroupedSequential(pg, &est, res, groups, nGroups, 0.999, 0, minVotes, &lg);
  CHECK(fz == std::vector<std::vector<double> >(nGroups) && lg == std::vector<int>(data.size(), -1));
  bool threw = false;
  try {
    std::vector<int> fewer(groups.begin(), groups.end() - 1);
    R::computeGroupedSequential(pg, &est, res, fewer, nGroups, 0.999, maxModels, minVotes);
  } catch (const std::invalid_argument &) {
    threw = true;
  }
  CHECK(threw);
  threw = false;
  try {
    R::computeGroupedSequential(pg, (Est *)NULL, res, groups, nGroups, 0.999, maxModels, minVotes);
  } catch (const std::invalid_argument &) {
    threw = true;
  }
  CHECK(threw);
  std::printf("%s: %zu groups, %zu models, computeGroupedSequential == computeManySequential on the gather\n", name,
              nGroups, models);
  R::seed() = 1;
}

int main() {
  PlaneParametersEstimator<3> plane(0.5);
  std::vector<P3> pts;
  std::vector<int> groups;
  planes(9011, 9, pts, groups);
  compare("plane", plane, pts, groups, 9, 5, 4, 50);
  // the fallback: a user-defined estimator, every group three lines of 3/10 of its records each
  std::vector<UserPoint2D> l2(3001);
  std::vector<int> g2(l2.size());
  const double nx[3] = {0.6, -0.8, 0.0}, ny[3] = {0.8, 0.6, 1.0}, ax[3] = {5, -40, 0}, ay[3] = {-7, 30, 90};
  for (size_t m = 0; m < l2.size(); m++) {
    const int j = (int)(m % 4);  // 1 is left empty, 2 gets one record (below the line's two)
    g2[m] = m % 97 == 5 ? -1 : (j == 1 ? 0 : (j == 2 && m > 4 ? 3 : j));
    const size_t which = (m / 4) % 10;
    double x = U(-300, 300), y = U(-300, 300);
    if (which < 9) {
      const size_t line = which / 3;
      const double d = (x - ax[line]) * nx[line] + (y - ay[line]) * ny[line];
      x += -d * nx[line] + U(-0.1, 0.1), y += -d * ny[line] + U(-0.1, 0.1);
    }
    l2[m].x = x, l2[m].y = y;
  }
  UserLine2D user(0.5);
  compare("user-defined 2-D line (fallback)", user, l2, g2, 4, 9, 4, 50);
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
