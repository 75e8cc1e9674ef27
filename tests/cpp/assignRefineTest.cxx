// assignRefineTest -- RANSAC<T,S>::assignToModels / refineModels.  For the plane (device path) they must equal the
// C ABI calls they wrap, lsqr_assign and lsqr_refine on a context of the caller's own: the same labels, rounds and
// stop, parameters bit for bit; the labels are the assignment of the returned models; a user-defined estimator without
// a device model, and forceHostLoop(), run the host loop (first agreeing model).  Exit code 0 == all passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>
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

// three planes through a common region (they cross inside the cloud) of 30 % each plus 10 % clutter, interleaved
static std::vector<P3> planes(size_t n) {
  double a[3][3], u[3][3], v[3][3];
  for (int j = 0; j < 3; j++)
    for (int i = 0; i < 3; i++) a[j][i] = U(-10, 10), u[j][i] = U(-1, 1), v[j][i] = U(-1, 1);
  std::vector<P3> pts(n);
  for (size_t m = 0; m < n; m++) {
    const int j = (int)(m % 10) / 3;  // 0, 1, 2, and 3 = clutter for m % 10 == 9
    const double s = U(-80, 80), t = U(-80, 80);
    for (int i = 0; i < 3; i++)
      pts[m][i] = j == 3 ? U(-200, 200) : a[j][i] + s * u[j][i] + t * v[j][i] + U(-0.1, 0.1);
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

template <class T, class Est>
static void firstAgreeing(Est &est, std::vector<std::vector<double> > models, std::vector<T> &data,
                          const std::vector<int> &labels) {
  size_t bad = 0;
  for (size_t i = 0; i < data.size(); i++) {
    int want = -1;
    for (size_t m = 0; m < models.size() && want < 0; m++)
      if (est.agree(models[m], data[i])) want = (int)m;
    bad += labels[i] != want;
  }
  CHECK(bad == 0);
}

static void plane() {
  typedef RANSAC<P3, double> R;
  std::vector<P3> data = planes(20011);
  PlaneParametersEstimator<3> est(0.5);
  std::vector<std::vector<double> > found;
  std::vector<int> greedy;
  R::seed() = 5;
  R::computeSequential(found, &est, data, 0.999, 4, 2000, &greedy);
  R::seed() = 1;
  CHECK(found.size() == 3);
  if (found.size() != 3) return;

  // the C ABI on a context of our own
  lsqr_model_cfg cfg;
  CHECK(est.deviceModel(cfg));
  lsqr_ctx *ctx = NULL;
  CHECK(lsqr_ctx_create(0, &ctx) == LSQR_OK);
  CHECK(lsqr_set_model(ctx, &cfg) == LSQR_OK);
  CHECK(lsqr_upload(ctx, &data[0], data.size(), sizeof(P3)) == LSQR_OK);
  const size_t N = data.size(), P = 6;
  std::vector<double> par(3 * P);
  for (size_t m = 0; m < 3; m++)
    for (size_t j = 0; j < P; j++) par[m * P + j] = found[m][j];
  std::vector<int32_t> lab(N), status(3);
  std::vector<lsqr_fit_info> fits(3);
  uint64_t counts[4];
  CHECK(lsqr_assign(ctx, &par[0], 3, 0, &lab[0], NULL, counts) == LSQR_OK);

  std::vector<int> labels;
  R::assignToModels(found, &est, data, labels);
  CHECK(labels.size() == N && std::equal(labels.begin(), labels.end(), lab.begin()));
  size_t moved = 0, unassigned = 0;
  for (size_t i = 0; i < N; i++) moved += labels[i] != greedy[i], unassigned += labels[i] < 0;
  CHECK(moved > 0);  // the planes cross inside the cloud: greedy labels are not the nearest model everywhere
  CHECK(unassigned == counts[3] && counts[0] + counts[1] + counts[2] + counts[3] == N);

  for (size_t maxRounds = 1; maxRounds <= 8; maxRounds += 7) {
    std::vector<double> q(par);
    size_t rounds = 0;
    int conv = 0;
    CHECK(lsqr_refine(ctx, &q[0], 3, maxRounds, 0, &lab[0], counts, &fits[0], &status[0], &rounds, &conv) == LSQR_OK);
    std::vector<std::vector<double> > models(found);
    bool converged = false;
    const size_t r = R::refineModels(models, &est, data, maxRounds, labels, &converged);
    CHECK(r == rounds && converged == (conv != 0) && r >= 1 && (maxRounds == 1 ? r == 1 : converged));
    CHECK(std::equal(labels.begin(), labels.end(), lab.begin()));
    for (size_t m = 0; m < 3; m++) {
      CHECK(models[m].size() == P && std::memcmp(&models[m][0], &q[m * P], sizeof(double) * P) == 0);
      CHECK(status[m] == LSQR_OK && fits[m].n_used >= 3);
    }
    std::vector<int> again;
    R::assignToModels(models, &est, data, again);
    CHECK(again == labels);  // the labels are the assignment of the returned models
    std::printf("plane: maxRounds %zu -> %zu refits, converged %d, refineModels == lsqr_refine\n", maxRounds, r,
                (int)converged);
  }
  lsqr_ctx_destroy(ctx);

  // the host loop on the same estimator: first agreeing model
  R::forceHostLoop() = true;
  R::assignToModels(found, &est, data, labels);
  firstAgreeing(est, found, data, labels);
  std::vector<std::vector<double> > models(found);
  bool converged = false;
  const size_t r = R::refineModels(models, &est, data, 8, labels, &converged);
  firstAgreeing(est, models, data, labels);
  CHECK(r >= 1 && converged);
  R::forceHostLoop() = false;

  // argument errors
  std::vector<std::vector<double> > many(65, found[0]), shortRow(found);
  shortRow[1].pop_back();
  bool threw = false;
  try {
    R::assignToModels(many, &est, data, labels);
  } catch (const std::invalid_argument &) {
    threw = true;
  }
  CHECK(threw);
  threw = false;
  try {
    R::refineModels(shortRow, &est, data, 2, labels);
  } catch (const std::invalid_argument &) {
    threw = true;
  }
  CHECK(threw);
  std::vector<std::vector<double> > none;
  R::assignToModels(none, &est, data, labels);
  CHECK(labels.size() == N && labels[0] == -1 && labels[N - 1] == -1);
  CHECK(R::refineModels(none, &est, data, 4, labels) == 0);
}

// the geometric sphere: assigned on the device, refitted by the host loop (its fit is iterative)
static void sphere() {
  typedef RANSAC<P3, double> R;
  std::vector<P3> data(3000);
  const double c[2][3] = {{0, 0, 0}, {70, 0, 0}}, rad[2] = {50, 40};
  for (size_t m = 0; m < data.size(); m++) {
    double d[3], len = 0;
    for (int i = 0; i < 3; i++) d[i] = U(-1, 1), len += d[i] * d[i];
    const int j = (int)(m % 2);
    for (int i = 0; i < 3; i++) data[m][i] = c[j][i] + rad[j] * d[i] / std::sqrt(len) + U(-0.05, 0.05);
  }
  SphereParametersEstimator<3> est(0.5);  // lsType = GEOMETRIC
  std::vector<std::vector<double> > models(2);
  for (int j = 0; j < 2; j++) {
    models[j].assign(c[j], c[j] + 3);
    models[j].push_back(rad[j] + 0.2);
  }
  std::vector<int> labels;
  R::assignToModels(models, &est, data, labels);
  size_t n0 = 0, n1 = 0;
  for (size_t i = 0; i < labels.size(); i++) n0 += labels[i] == 0, n1 += labels[i] == 1;
  CHECK(n0 > 1000 && n1 > 1000);
  bool converged = false;
  const size_t r = R::refineModels(models, &est, data, 8, labels, &converged);
  CHECK(r >= 1 && converged && std::fabs(models[0][3] - 50) < 0.05 && std::fabs(models[1][3] - 40) < 0.05);
  firstAgreeing(est, models, data, labels);
  std::printf("sphere (geometric): assigned on the device, %zu refits on the host\n", r);
}

static void plugin() {
  typedef RANSAC<UserPoint2D, double> R;
  std::vector<UserPoint2D> data = lines2d(3001);
  UserLine2D est(0.5);
  std::vector<std::vector<double> > models;
  std::vector<int> greedy, labels;
  R::seed() = 9;
  R::computeSequential(models, &est, data, 0.999, 4, 300, &greedy);
  R::seed() = 1;
  CHECK(models.size() == 3);
  R::assignToModels(models, &est, data, labels);
  firstAgreeing(est, models, data, labels);
  bool converged = false;
  const size_t r = R::refineModels(models, &est, data, 8, labels, &converged);
  CHECK(r >= 1 && converged);
  firstAgreeing(est, models, data, labels);
  std::vector<int> again;
  R::assignToModels(models, &est, data, again);
  CHECK(again == labels);
  std::printf("user-defined 2-D line (host loop): %zu refits, converged %d\n", r, (int)converged);
}

int main() {
  plane();
  sphere();
  plugin();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
