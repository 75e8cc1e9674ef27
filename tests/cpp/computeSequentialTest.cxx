// computeSequentialTest -- RANSAC<T,S>::computeSequential against the loop it replaces: compute() with seed() + r on
// the records that are left, the consensus set erased after every accepted round.  Fractions, labels and the number
// of models must be equal, the parameters within 1e-9 relative (fits that differ at most in summation order), for the
// plane, the default (geometric) sphere, a user-defined estimator without a device model and the ResidentData
// overload.  Exit code 0 == all passed.
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
static std::mt19937_64 gen(2026);
static double U(double a, double b) { return std::uniform_real_distribution<double>(a, b)(gen); }

// three planes (kind 0) or spheres (kind 1) of 30 % each plus 10 % uniform clutter, interleaved
static std::vector<P3> scene(int kind, size_t n) {
  double a[3][3], u[3][3], v[3][3], r[3];
  for (int j = 0; j < 3; j++) {
    for (int i = 0; i < 3; i++) a[j][i] = U(-100, 100), u[j][i] = U(-1, 1), v[j][i] = U(-1, 1);
    r[j] = U(20, 60);
  }
  std::vector<P3> pts(n);
  for (size_t m = 0; m < n; m++) {
    const int j = (int)(m % 10) / 3;  // 0, 1, 2, and 3 = clutter for m % 10 == 9
    double d[3], len = 0;
    const double s = U(-80, 80), t = U(-80, 80);
    for (int i = 0; i < 3; i++) d[i] = U(-1, 1), len += d[i] * d[i];
    for (int i = 0; i < 3; i++) {
      if (j == 3) pts[m][i] = U(-200, 200);
      else if (kind == 0) pts[m][i] = a[j][i] + s * u[j][i] + t * v[j][i] + U(-0.1, 0.1);
      else pts[m][i] = a[j][i] + r[j] * d[i] / std::sqrt(len) + U(-0.1, 0.1);
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

static std::vector<UserPoint2D> lines2d(size_t n) {
  std::vector<UserPoint2D> pts(n);
  const double nx[3] = {0.6, -0.8, 0.0}, ny[3] = {0.8, 0.6, 1.0}, ax[3] = {5, -40, 0}, ay[3] = {-7, 30, 90};
  for (size_t m = 0; m < n; m++) {
    const int j = (int)(m % 10) / 3;
    double x = U(-300, 300), y = U(-300, 300);
    if (j < 3) {
      const double d = (x - ax[j]) * nx[j] + (y - ay[j]) * ny[j];
      x += -d * nx[j] + U(-0.1, 0.1), y += -d * ny[j] + U(-0.1, 0.1);
    }
    pts[m].x = x, pts[m].y = y;
  }
  return pts;
}

// the loop computeSequential replaces
template <class T, class Est>
static void loop(Est &est, const std::vector<T> &data, uint64_t seed0, size_t maxModels, size_t minVotes,
                 std::vector<std::vector<double> > &params, std::vector<double> &frac, std::vector<int> &labels) {
  std::vector<T> cur(data);
  std::vector<size_t> orig(data.size());
  for (size_t i = 0; i < orig.size(); i++) orig[i] = i;
  labels.assign(data.size(), -1);
  params.clear();
  frac.clear();
  for (size_t r = 0; r < maxModels && cur.size() >= est.numForEstimate(); r++) {
    RANSAC<T, double>::seed() = seed0 + r;
    std::vector<double> p;
    std::vector<bool> cons;
    frac.push_back(RANSAC<T, double>::compute(p, &est, cur, 0.999, &cons));
    const size_t votes = RANSAC<T, double>::lastInfo().best_votes;
    if (p.empty() || votes < (minVotes > 1 ? minVotes : 1)) break;
    params.push_back(p);
    std::vector<T> next;
    std::vector<size_t> nextOrig;
    for (size_t i = 0; i < cur.size(); i++) {
      if (cons[i]) labels[orig[i]] = (int)r;
      else next.push_back(cur[i]), nextOrig.push_back(orig[i]);
    }
    cur.swap(next);
    orig.swap(nextOrig);
  }
  RANSAC<T, double>::seed() = seed0;
}

static bool close(const std::vector<double> &a, const std::vector<double> &b, int signed_head) {
  if (a.size() != b.size()) return false;
  double dot = 0;
  for (int i = 0; i < signed_head; i++) dot += a[(size_t)i] * b[(size_t)i];
  const double sgn = dot < 0 ? -1.0 : 1.0;  // a normal's sign is arbitrary
  for (size_t i = 0; i < a.size(); i++) {
    const double g = (int)i < signed_head ? sgn * a[i] : a[i];
    if (!(std::fabs(g - b[i]) <= 1e-9 * std::fmax(1.0, std::fabs(b[i])))) return false;
  }
  return true;
}

template <class T>
static void same(const char *name, const std::vector<std::vector<double> > &pa, const std::vector<double> &fa,
                 const std::vector<int> &la, const std::vector<std::vector<double> > &pb,
                 const std::vector<double> &fb, const std::vector<int> &lb, size_t models, int signed_head) {
  CHECK(pa.size() == models && pb.size() == models);
  CHECK(fa == fb);
  CHECK(la == lb);
  for (size_t r = 0; r < pa.size() && r < pb.size(); r++) CHECK(close(pa[r], pb[r], signed_head));
  std::printf("%s: %zu models, %zu rounds, computeSequential == loop of compute()\n", name, pa.size(), fa.size());
}

template <class Est>
static void compare(const char *name, Est &est, int kind, int signed_head) {
  std::vector<P3> data = scene(kind, 20011);
  std::vector<std::vector<double> > pl, ps, pr;
  std::vector<double> fl, fs, fr;
  std::vector<int> ll, ls, lr;
  loop(est, data, 5, 4, 2000, pl, fl, ll);
  RANSAC<P3, double>::seed() = 5;
  fs = RANSAC<P3, double>::computeSequential(ps, &est, data, 0.999, 4, 2000, &ls);
  same<P3>(name, ps, fs, ls, pl, fl, ll, 3, signed_head);
  CHECK(fs.size() == 4);  // the round on the clutter ran and was rejected
  CHECK((RANSAC<P3, double>::lastInfo().best_votes < 2000));
  // resident records: the same call without the upload, twice (the records are still there)
  ResidentData<P3> res(data);
  for (int rep = 0; rep < 2; rep++) {
    fr = RANSAC<P3, double>::computeSequential(pr, &est, res, 0.999, 4, 2000, &lr);
    CHECK(fr == fs && lr == ls && pr == ps);
  }
  // maxModels cuts the search short; nothing runs on invalid input
  fr = RANSAC<P3, double>::computeSequential(pr, &est, data, 0.999, 2, 2000, &lr);
  CHECK(fr.size() == 2 && pr.size() == 2 && fr[0] == fs[0] && fr[1] == fs[1]);
  for (size_t i = 0; i < lr.size(); i++) CHECK(lr[i] == (ls[i] < 2 ? ls[i] : -1));
  fr = RANSAC<P3, double>::computeSequential(pr, &est, data, 1.5, 4, 0, &lr);
  CHECK(fr.empty() && pr.empty() && lr.size() == data.size() && lr[0] == -1);
  RANSAC<P3, double>::seed() = 1;
}

static void plugin() {
  std::vector<UserPoint2D> data = lines2d(3001);
  UserLine2D est(0.5);
  std::vector<std::vector<double> > pl, ps;
  std::vector<double> fl, fs;
  std::vector<int> ll, ls;
  loop(est, data, 9, 4, 300, pl, fl, ll);
  RANSAC<UserPoint2D, double>::seed() = 9;
  fs = RANSAC<UserPoint2D, double>::computeSequential(ps, &est, data, 0.999, 4, 300, &ls);
  same<UserPoint2D>("user-defined 2-D line (host loop)", ps, fs, ls, pl, fl, ll, 3, 2);
  RANSAC<UserPoint2D, double>::seed() = 1;
}

int main() {
  PlaneParametersEstimator<3> plane(0.5);
  SphereParametersEstimator<3> sphere(0.5);  // lsType = GEOMETRIC, the reference's default
  compare("plane", plane, 0, 3);
  compare("sphere (geometric)", sphere, 1, 0);
  plugin();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
