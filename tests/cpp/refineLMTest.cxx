// refineLMTest -- RANSAC<T,S>::refineModelsLM, the device refine of the geometric sphere.  It must equal the C ABI call
// it wraps, lsqr_refine_lm on a context of the caller's own: the same labels, rounds and stop, parameters bit for bit;
// it converges on the two planted spheres; any other estimator is refused.  Exit code 0 == all passed.
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

// the two-sphere scene of assignRefineTest.cxx: radii 50 and 40, centres 70 apart, the records interleaved
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
  std::vector<std::vector<double> > start(2);
  for (int j = 0; j < 2; j++) {
    start[j].assign(c[j], c[j] + 3);
    start[j].push_back(rad[j] + 0.2);
  }

  // the C ABI on a context of our own
  lsqr_model_cfg cfg;
  CHECK(est.deviceModel(cfg));
  CHECK(cfg.model == LSQR_MODEL_SPHERE && cfg.ls_type == LSQR_LS_GEOMETRIC);
  lsqr_ctx *ctx = NULL;
  CHECK(lsqr_ctx_create(0, &ctx) == LSQR_OK);
  CHECK(lsqr_set_model(ctx, &cfg) == LSQR_OK);
  CHECK(lsqr_upload(ctx, &data[0], data.size(), sizeof(P3)) == LSQR_OK);
  const size_t N = data.size(), P = 4;
  std::vector<double> par(2 * P);
  for (size_t m = 0; m < 2; m++)
    for (size_t j = 0; j < P; j++) par[m * P + j] = start[m][j];
  std::vector<int32_t> lab(N), status(2);
  std::vector<lsqr_fit_info> fits(2);

  for (size_t maxRounds = 1; maxRounds <= 8; maxRounds += 7) {
    std::vector<double> q(par);
    size_t rounds = 0;
    int conv = 0;
    CHECK(lsqr_refine_lm(ctx, &q[0], 2, maxRounds, 0, &lab[0], NULL, &fits[0], &status[0], &rounds, &conv) == LSQR_OK);
    std::vector<std::vector<double> > models(start);
    std::vector<int> labels;
    bool converged = false;
    const size_t r = R::refineModelsLM(models, &est, data, maxRounds, labels, &converged);
    CHECK(r == rounds && converged == (conv != 0) && r >= 1 && (maxRounds == 1 ? r == 1 : converged));
    CHECK(labels.size() == N && std::equal(labels.begin(), labels.end(), lab.begin()));
    for (size_t m = 0; m < 2; m++) {
      CHECK(models[m].size() == P && std::memcmp(&models[m][0], &q[m * P], sizeof(double) * P) == 0);
      CHECK(status[m] == LSQR_OK && fits[m].lm_info >= 1 && fits[m].lm_info <= 4 && fits[m].n_used > 1000);
    }
    CHECK(std::fabs(models[0][3] - 50) < 0.05 && std::fabs(models[1][3] - 40) < 0.05);
    std::vector<int> again;
    R::assignToModels(models, &est, data, again);
    CHECK(again == labels);  // the labels are the assignment of the returned models
    std::printf("sphere (geometric): maxRounds %zu -> %zu refits, converged %d, refineModelsLM == lsqr_refine_lm\n",
                maxRounds, r, (int)converged);
  }
  lsqr_ctx_destroy(ctx);

  // any other estimator is refused
  PlaneParametersEstimator<3> plane(0.5);
  std::vector<std::vector<double> > pm(1, std::vector<double>(6, 0.0));
  pm[0][0] = 1.0;
  std::vector<int> labels;
  bool threw = false;
  try {
    R::refineModelsLM(pm, &plane, data, 2, labels);
  } catch (const std::invalid_argument &) {
    threw = true;
  }
  CHECK(threw);
  SphereParametersEstimator<3> algebraic(0.5, SphereParametersEstimator<3>::ALGEBRAIC);
  std::vector<std::vector<double> > sm(start);
  threw = false;
  try {
    R::refineModelsLM(sm, &algebraic, data, 2, labels);
  } catch (const std::invalid_argument &) {
    threw = true;
  }
  CHECK(threw);
}

int main() {
  sphere();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
