// computeManySequentialTest -- RANSAC<T,S>::computeManySequential against computeSequential per problem: problem j
// after seed(seed() + j * maxModels).  Fractions, labels and the number of models must be equal, the parameters within
// 1e-9 relative (fits that differ at most in summation order), for the plane (one lsqr_ransac_many_sequential call) and
// a user-defined estimator without a device model (the host loop).  Exit code 0 == all passed.
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
static std::mt19937_64 gen(2027);
static double U(double a, double b) { return std::uniform_real_distribution<double>(a, b)(gen); }

// `planes` planes of a quarter of the records each, the rest uniform clutter, interleaved
static std::vector<P3> scene(size_t n, int planes) {
  double a[3][3], u[3][3], v[3][3];
  for (int j = 0; j < 3; j++)
    for (int i = 0; i < 3; i++) a[j][i] = U(-100, 100), u[j][i] = U(-1, 1), v[j][i] = U(-1, 1);
  std::vector<P3> pts(n);
  for (size_t m = 0; m < n; m++) {
    const int j = (int)(m % 4);
    const double s = U(-80, 80), t = U(-80, 80);
    for (int i = 0; i < 3; i++) {
      if (j >= planes) pts[m][i] = U(-200, 200);
      else pts[m][i] = a[j][i] + s * u[j][i] + t * v[j][i] + U(-0.1, 0.1);
    }
  }
  return pts;
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

static std::vector<UserPoint2D> lines2d(size_t n, int lines) {
  std::vector<UserPoint2D> pts(n);
  const double nx[3] = {0.6, -0.8, 0.0}, ny[3] = {0.8, 0.6, 1.0}, ax[3] = {5, -40, 0}, ay[3] = {-7, 30, 90};
  for (size_t m = 0; m < n; m++) {
    const int j = (int)(m % 4);
    double x = U(-300, 300), y = U(-300, 300);
    if (j < lines) {
      const double d = (x - ax[j]) * nx[j] + (y - ay[j]) * ny[j];
      x += -d * nx[j] + U(-0.1, 0.1), y += -d * ny[j] + U(-0.1, 0.1);
    }
    pts[m].x = x, pts[m].y = y;
  }
  return pts;
}

static bool close(const std::vector<double> &a, const std::vector<double> &b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++)
    if (!(std::fabs(a[i] - b[i]) <= 1e-9 * std::fmax(1.0, std::fabs(b[i])))) return false;
  return true;
}

// computeManySequential on `data` == computeSequential on every data[j] with its seeds
template <class T, class Est>
static void compare(const char *name, Est &est, std::vector<std::vector<T> > &data, size_t maxModels, size_t minVotes,
                    size_t wantDistinct) {
  typedef RANSAC<T, double> R;
  const uint64_t s0 = 7;
  R::seed() = s0;
  std::vector<std::vector<std::vector<double> > > pm;
  std::vector<std::vector<int> > lm;
  std::vector<std::vector<double> > fm = R::computeManySequential(pm, &est, data, 0.999, maxModels, minVotes, &lm);
  CHECK(R::seed() == s0);
  CHECK(fm.size() == data.size() && pm.size() == data.size() && lm.size() == data.size());
  std::vector<size_t> seen;
  for (size_t j = 0; j < data.size(); j++) {
    std::vector<std::vector<double> > ps;
    std::vector<int> ls;
    R::seed() = s0 + j * maxModels;
    std::vector<double> fs = R::computeSequential(ps, &est, data[j], 0.999, maxModels, minVotes, &ls);
    CHECK(fm[j] == fs);
    CHECK(lm[j] == ls);
    CHECK(pm[j].size() == ps.size());
    for (size_t r = 0; r < ps.size() && r < pm[j].size(); r++) CHECK(close(pm[j][r], ps[r]));
    bool fresh = true;
    for (size_t q = 0; q < seen.size(); q++) fresh = fresh && seen[q] != ps.size();
    if (fresh) seen.push_back(ps.size());
  }
  R::seed() = 1;
  CHECK(seen.size() >= wantDistinct);  // the problems stop at different rounds
  // nothing runs on invalid input or with no models asked for
  fm = R::computeManySequential(pm, &est, data, 1.5, maxModels, minVotes, &lm);
  CHECK(fm.size() == data.size() && fm[0].empty() && pm[0].empty() && lm[0].size() == data[0].size() && lm[0][0] == -1);
  fm = R::computeManySequential(pm, &est, data, 0.999, 0, minVotes, &lm);
  CHECK(fm.size() == data.size() && fm[0].empty() && pm[0].empty());
  std::printf("%s: %zu problems, computeManySequential == computeSequential per problem\n", name, data.size());
}

int main() {
  PlaneParametersEstimator<3> plane(0.5);
  std::vector<std::vector<P3> > planes;
  const int planted[8] = {3, 0, 2, 1, 0, 3, 1, 2};
  for (int j = 0; j < 8; j++) planes.push_back(scene(600 + 11 * (size_t)j, planted[j]));
  planes.push_back(scene(2, 0));  // fewer records than a minimal subset
  planes.push_back(std::vector<P3>());
  planes.push_back(scene(5003, 3));  // more than one part of the partition
  compare("plane", plane, planes, 4, 60, 4);
  UserLine2D line(0.5);
  std::vector<std::vector<UserPoint2D> > lines;
  for (int j = 0; j < 4; j++) lines.push_back(lines2d(800 + 13 * (size_t)j, j));
  compare("user-defined 2-D line (host loop)", line, lines, 4, 80, 3);
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
