// assignRefineGroupedTest -- RANSAC<T,S>::assignToModelsGrouped / refineModelsGrouped.  For the plane (device path)
// they must equal the C ABI calls they wrap, lsqr_assign_grouped and lsqr_refine_grouped on a context of the caller's
// own: the same labels, rounds and stops, parameters bit for bit, and per group what refineModels gives on the gather;
// a user-defined estimator without a device model, and forceHostLoop(), equal the loop over refineModels on the
// per-group gathers.  Exit code 0 == all passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>
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

static std::vector<UserPoint2D> lines2d(size_t n, double shift) {
  std::vector<UserPoint2D> pts(n);
  const double nx[3] = {0.6, -0.8, 0.0}, ny[3] = {0.8, 0.6, 1.0}, ax[3] = {5, -40, 0}, ay[3] = {-7, 30, 90};
  for (size_t m = 0; m < n; m++) {
    const int j = (int)(m % 10) / 3;
    double x = U(-300, 300), y = U(-300, 300);
    if (j < 3) {
      const double d = (x - ax[j] - shift) * nx[j] + (y - ay[j]) * ny[j];
      x += -d * nx[j] + U(-0.1, 0.1), y += -d * ny[j] + U(-0.1, 0.1);
    }
    pts[m].x = x, pts[m].y = y;
  }
  return pts;
}

// the sets interleaved record by record; every 97th record goes to no group (-1 and nGroups + 2 in turn)
template <class T>
static void interleave(const std::vector<std::vector<T> > &sets, std::vector<T> &data, std::vector<int> &groups) {
  std::vector<size_t> at(sets.size(), 0);
  size_t left = 0, k = 0;
  for (size_t g = 0; g < sets.size(); g++) left += sets[g].size();
  while (left) {
    for (size_t g = 0; g < sets.size(); g++) {
      if (at[g] == sets[g].size()) continue;
      data.push_back(sets[g][at[g]++]);
      left--;
      k++;
      groups.push_back(k % 97 == 0 ? (k % 2 ? -1 : (int)sets.size() + 2) : (int)g);
    }
  }
}

// what the per-group loop over refineModels gives: the reference of both paths
template <class T, class Est>
static void loopOverGroups(Est &est, const std::vector<T> &data, const std::vector<int> &groups, size_t n,
                           std::vector<std::vector<std::vector<double> > > &models, size_t maxRounds,
                           std::vector<int> &labels, std::vector<size_t> &rounds, std::vector<bool> &converged) {
  typedef RANSAC<T, double> R;
  labels.assign(data.size(), -1);
  rounds.assign(n, 0);
  converged.assign(n, false);
  for (size_t g = 0; g < n; g++) {
    std::vector<T> set;
    std::vector<size_t> index;
    for (size_t i = 0; i < data.size(); i++)
      if (groups[i] == (int)g) set.push_back(data[i]), index.push_back(i);
    std::vector<int> lab;
    bool conv = false;
    rounds[g] = R::refineModels(models[g], &est, set, maxRounds, lab, &conv);
    converged[g] = conv;
    for (size_t q = 0; q < lab.size(); q++) labels[index[q]] = lab[q];
  }
}

static bool sameModels(const std::vector<std::vector<std::vector<double> > > &a,
                       const std::vector<std::vector<std::vector<double> > > &b) {
  if (a.size() != b.size()) return false;
  for (size_t g = 0; g < a.size(); g++) {
    if (a[g].size() != b[g].size()) return false;
    for (size_t m = 0; m < a[g].size(); m++)
      if (a[g][m].size() != b[g][m].size() ||
          std::memcmp(&a[g][m][0], &b[g][m][0], sizeof(double) * a[g][m].size()) != 0)
        return false;
  }
  return true;
}

static void plane() {
  typedef RANSAC<P3, double> R;
  const size_t n = 4, P = 6;
  std::vector<std::vector<P3> > sets(n);
  sets[0] = planes(5003);
  sets[1] = planes(2049);
  sets[3] = planes(700);  // (group 2 has no records)
  std::vector<P3> data;
  std::vector<int> groups;
  interleave(sets, data, groups);
  const size_t N = data.size();
  PlaneParametersEstimator<3> est(0.5);
  ResidentData<P3> res(data);
  std::vector<std::vector<std::vector<double> > > found;
  R::seed() = 5;
  R::computeGroupedSequential(found, &est, res, groups, n, 0.999, 4, 60);
  R::seed() = 1;
  CHECK(found.size() == n && found[0].size() == 3 && found[1].size() == 3 && found[2].empty() && found[3].size() == 3);
  if (failures) return;

  // the C ABI on a context of our own
  lsqr_model_cfg cfg;
  CHECK(est.deviceModel(cfg));
  lsqr_ctx *ctx = NULL;
  CHECK(lsqr_ctx_create(0, &ctx) == LSQR_OK);
  CHECK(lsqr_set_model(ctx, &cfg) == LSQR_OK);
  CHECK(lsqr_upload(ctx, &data[0], N, sizeof(P3)) == LSQR_OK);
  const size_t MM = 3;
  std::vector<double> par(n * MM * P, 0.0);
  std::vector<size_t> nModels(n);
  for (size_t g = 0; g < n; g++) {
    nModels[g] = found[g].size();
    for (size_t m = 0; m < found[g].size(); m++)
      for (size_t j = 0; j < P; j++) par[(g * MM + m) * P + j] = found[g][m][j];
  }
  std::vector<int32_t> glab(groups.begin(), groups.end()), lab(N), status(n * MM), conv(n);
  std::vector<lsqr_fit_info> fits(n * MM);
  std::vector<size_t> rounds(n);
  CHECK(lsqr_assign_grouped(ctx, &glab[0], n, 0, &par[0], &nModels[0], MM, &lab[0], NULL, NULL, NULL) == LSQR_OK);

  std::vector<int> labels;
  R::assignToModelsGrouped(found, &est, res, groups, n, labels);
  CHECK(labels.size() == N && std::equal(labels.begin(), labels.end(), lab.begin()));
  size_t outside = 0, assigned = 0;
  for (size_t i = 0; i < N; i++) {
    if (groups[i] < 0 || groups[i] >= (int)n) outside += labels[i] == -1;
    else assigned += labels[i] >= 0;
  }
  CHECK(outside == N / 97 && assigned > N / 2);

  for (size_t maxRounds = 1; maxRounds <= 8; maxRounds += 7) {
    std::vector<double> q(par);
    CHECK(lsqr_refine_grouped(ctx, &glab[0], n, 0, &q[0], &nModels[0], MM, maxRounds, &lab[0], NULL, NULL, &fits[0],
                              &status[0], &rounds[0], &conv[0]) == LSQR_OK);
    std::vector<std::vector<std::vector<double> > > models(found);
    std::vector<bool> converged;
    const std::vector<size_t> r = R::refineModelsGrouped(models, &est, res, groups, n, maxRounds, labels, &converged);
    CHECK(r == rounds && std::equal(labels.begin(), labels.end(), lab.begin()));
    CHECK(r[2] == 0 && !converged[2] && r[0] >= 1 && r[1] >= 1 && r[3] >= 1);
    for (size_t g = 0; g < n; g++) {
      CHECK(converged[g] == (conv[g] != 0));
      for (size_t m = 0; m < found[g].size(); m++)
        CHECK(models[g][m].size() == P && std::memcmp(&models[g][m][0], &q[(g * MM + m) * P], sizeof(double) * P) == 0);
    }
    // the drop-in's own contract: per group what refineModels gives on the gather
    std::vector<std::vector<std::vector<double> > > want(found);
    std::vector<int> wantLabels;
    std::vector<size_t> wantRounds;
    std::vector<bool> wantConv;
    loopOverGroups(est, data, groups, n, want, maxRounds, wantLabels, wantRounds, wantConv);
    CHECK(sameModels(models, want) && labels == wantLabels && r == wantRounds && converged == wantConv);
    std::vector<int> again;
    R::assignToModelsGrouped(models, &est, res, groups, n, again);
    CHECK(again == labels);  // the labels are the assignment of the returned models
    std::printf("plane: maxRounds %zu -> %zu / %zu / %zu / %zu refits, refineModelsGrouped == lsqr_refine_grouped\n",
                maxRounds, r[0], r[1], r[2], r[3]);
  }
  lsqr_ctx_destroy(ctx);

  // forceHostLoop(): the loop over refineModels on the per-group gathers, itself under forceHostLoop()
  R::forceHostLoop() = true;
  {
    std::vector<std::vector<std::vector<double> > > models(found), want(found);
    std::vector<bool> converged, wantConv;
    std::vector<int> wantLabels;
    std::vector<size_t> wantRounds;
    const std::vector<size_t> r = R::refineModelsGrouped(models, &est, res, groups, n, 8, labels, &converged);
    loopOverGroups(est, data, groups, n, want, 8, wantLabels, wantRounds, wantConv);
    CHECK(sameModels(models, want) && labels == wantLabels && r == wantRounds && converged == wantConv);
    CHECK(r[0] >= 1 && converged[0] && r[2] == 0);
    std::vector<int> again;
    R::assignToModelsGrouped(models, &est, res, groups, n, again);
    CHECK(again == labels);
  }
  R::forceHostLoop() = false;

  // argument errors
  std::vector<std::vector<std::vector<double> > > many(found), shortRow(found), fewer(found);
  many[1].assign(65, found[1][0]);
  shortRow[3][1].pop_back();
  fewer.pop_back();
  for (int k = 0; k < 3; k++) {
    bool threw = false;
    try {
      if (k == 0) R::assignToModelsGrouped(many, &est, res, groups, n, labels);
      if (k == 1) R::refineModelsGrouped(shortRow, &est, res, groups, n, 2, labels);
      if (k == 2) R::refineModelsGrouped(fewer, &est, res, groups, n, 2, labels);
    } catch (const std::invalid_argument &) {
      threw = true;
    }
    CHECK(threw);
  }
  std::vector<std::vector<std::vector<double> > > none(n);
  R::assignToModelsGrouped(none, &est, res, groups, n, labels);
  CHECK(labels.size() == N && labels[0] == -1 && labels[N - 1] == -1);
  const std::vector<size_t> zero = R::refineModelsGrouped(none, &est, res, groups, n, 4, labels);
  CHECK(zero == std::vector<size_t>(n, 0));
}

static void plugin() {
  typedef RANSAC<UserPoint2D, double> R;
  const size_t n = 3;
  std::vector<std::vector<UserPoint2D> > sets(n);
  sets[0] = lines2d(3001, 0.0);
  sets[1] = lines2d(1200, 25.0);
  sets[2] = lines2d(640, -60.0);
  std::vector<UserPoint2D> data;
  std::vector<int> groups;
  interleave(sets, data, groups);
  UserLine2D est(0.5);
  ResidentData<UserPoint2D> res(data);
  std::vector<std::vector<std::vector<double> > > found;
  R::seed() = 9;
  R::computeGroupedSequential(found, &est, res, groups, n, 0.999, 4, 100);
  R::seed() = 1;
  CHECK(found.size() == n && found[0].size() == 3 && found[1].size() == 3 && found[2].size() == 3);
  if (failures) return;
  std::vector<std::vector<std::vector<double> > > models(found), want(found);
  std::vector<int> labels, wantLabels;
  std::vector<bool> converged, wantConv;
  std::vector<size_t> wantRounds;
  const std::vector<size_t> r = R::refineModelsGrouped(models, &est, res, groups, n, 8, labels, &converged);
  loopOverGroups(est, data, groups, n, want, 8, wantLabels, wantRounds, wantConv);
  CHECK(sameModels(models, want) && labels == wantLabels && r == wantRounds && converged == wantConv);
  CHECK(r[0] >= 1 && r[1] >= 1 && r[2] >= 1 && converged[0] && converged[1] && converged[2]);
  std::vector<int> again;
  R::assignToModelsGrouped(models, &est, res, groups, n, again);
  CHECK(again == labels);
  std::printf("user-defined 2-D line (host loop): %zu / %zu / %zu refits\n", r[0], r[1], r[2]);
}

int main() {
  plane();
  plugin();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
