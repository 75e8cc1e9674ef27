// refineLMGroupedTest -- RANSAC<T,S>::refineModelsLMGrouped, the grouped device refine of the geometric sphere.  On
// three groups of two spheres each it must equal the per-group loop of refineModelsLM on the gathers: the same labels,
// rounds and stops, parameters bit for bit; and the C ABI call it wraps.  Any other estimator is refused.
// Exit code 0 == all passed.
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
static std::mt19937_64 gen(2029);
static double U(double a, double b) { return std::uniform_real_distribution<double>(a, b)(gen); }

// the two-sphere scene of refineLMTest.cxx, moved by `shift`: radii 50 and 40, centres 70 apart, interleaved
static std::vector<P3> spheres(size_t n, double shift) {
  std::vector<P3> data(n);
  const double c[2][3] = {{shift, 0, 0}, {shift + 70, 0, 0}}, rad[2] = {50, 40};
  for (size_t m = 0; m < n; m++) {
    double d[3], len = 0;
    for (int i = 0; i < 3; i++) d[i] = U(-1, 1), len += d[i] * d[i];
    const int j = (int)(m % 2);
    for (int i = 0; i < 3; i++) data[m][i] = c[j][i] + rad[j] * d[i] / std::sqrt(len) + U(-0.05, 0.05);
  }
  return data;
}

static void sphere() {
  typedef RANSAC<P3, double> R;
  const size_t n = 4, P = 4, MM = 2;
  const size_t sizes[n] = {3001, 2049, 0, 700};  // (group 2 has no records)
  const double shift[n] = {0.0, 300.0, 0.0, -250.0}, off[n] = {0.2, 0.3, 0.0, 0.1};
  std::vector<std::vector<P3> > sets(n);
  std::vector<std::vector<std::vector<double> > > start(n);
  for (size_t g = 0; g < n; g++) {
    sets[g] = spheres(sizes[g], shift[g]);
    if (!sizes[g]) continue;
    start[g].resize(2);
    for (int j = 0; j < 2; j++) {
      const double row[4] = {shift[g] + 70.0 * j + off[g], off[g], -off[g], (j ? 40.0 : 50.0) + off[g]};
      start[g][j].assign(row, row + 4);
    }
  }
  // interleaved record by record; every 97th record goes to no group
  std::vector<P3> data;
  std::vector<int> groups;
  {
    std::vector<size_t> at(n, 0);
    size_t left = 0, k = 0;
    for (size_t g = 0; g < n; g++) left += sets[g].size();
    while (left)
      for (size_t g = 0; g < n; g++) {
        if (at[g] == sets[g].size()) continue;
        data.push_back(sets[g][at[g]++]);
        left--;
        k++;
        groups.push_back(k % 97 == 0 ? (k % 2 ? -1 : (int)n + 2) : (int)g);
      }
  }
  const size_t N = data.size();
  SphereParametersEstimator<3> est(0.5);  // lsType = GEOMETRIC
  ResidentData<P3> res(data);

  // the C ABI on a context of our own
  lsqr_model_cfg cfg;
  CHECK(est.deviceModel(cfg));
  CHECK(cfg.model == LSQR_MODEL_SPHERE && cfg.ls_type == LSQR_LS_GEOMETRIC);
  lsqr_ctx *ctx = NULL;
  CHECK(lsqr_ctx_create(0, &ctx) == LSQR_OK);
  CHECK(lsqr_set_model(ctx, &cfg) == LSQR_OK);
  CHECK(lsqr_upload(ctx, &data[0], N, sizeof(P3)) == LSQR_OK);
  std::vector<double> par(n * MM * P, 0.0);
  std::vector<size_t> nModels(n);
  for (size_t g = 0; g < n; g++) {
    nModels[g] = start[g].size();
    for (size_t m = 0; m < start[g].size(); m++)
      for (size_t j = 0; j < P; j++) par[(g * MM + m) * P + j] = start[g][m][j];
  }
  std::vector<int32_t> glab(groups.begin(), groups.end()), lab(N), status(n * MM), conv(n);
  std::vector<lsqr_fit_info> fits(n * MM);
  std::vector<size_t> rounds(n);

  for (size_t maxRounds = 1; maxRounds <= 8; maxRounds += 7) {
    std::vector<double> q(par);
    CHECK(lsqr_refine_lm_grouped(ctx, &glab[0], n, 0, &q[0], &nModels[0], MM, maxRounds, &lab[0], NULL, NULL, &fits[0],
                                 &status[0], &rounds[0], &conv[0]) == LSQR_OK);
    std::vector<std::vector<std::vector<double> > > models(start);
    std::vector<int> labels;
    std::vector<bool> converged;
    const std::vector<size_t> r = R::refineModelsLMGrouped(models, &est, res, groups, n, maxRounds, labels, &converged);
    CHECK(r == rounds && labels.size() == N && std::equal(labels.begin(), labels.end(), lab.begin()));
    CHECK(r[2] == 0 && !converged[2] && r[0] >= 1 && r[1] >= 1 && r[3] >= 1);
    // per group what refineModelsLM gives on the gather
    for (size_t g = 0; g < n; g++) {
      CHECK(converged[g] == (conv[g] != 0));
      std::vector<P3> set;
      std::vector<size_t> index;
      for (size_t i = 0; i < N; i++)
        if (groups[i] == (int)g) set.push_back(data[i]), index.push_back(i);
      std::vector<std::vector<double> > want(start[g]);
      std::vector<int> wantLabels;
      bool wantConv = false;
      const size_t wantRounds = R::refineModelsLM(want, &est, set, maxRounds, wantLabels, &wantConv);
      CHECK(r[g] == wantRounds && converged[g] == wantConv && models[g].size() == want.size());
      for (size_t m = 0; m < want.size(); m++) {
        CHECK(models[g][m].size() == P && std::memcmp(&models[g][m][0], &want[m][0], sizeof(double) * P) == 0);
        CHECK(std::memcmp(&models[g][m][0], &q[(g * MM + m) * P], sizeof(double) * P) == 0);
        CHECK(status[g * MM + m] == LSQR_OK && fits[g * MM + m].lm_info >= 1 && fits[g * MM + m].lm_info <= 4);
        CHECK(std::fabs(models[g][m][3] - (m ? 40 : 50)) < 0.05);
      }
      for (size_t k = 0; k < index.size(); k++) CHECK(labels[index[k]] == wantLabels[k]);
    }
    for (size_t i = 0; i < N; i++)
      if (groups[i] < 0 || groups[i] >= (int)n) CHECK(labels[i] == -1);
    std::vector<int> again;
    R::assignToModelsGrouped(models, &est, res, groups, n, again);
    CHECK(again == labels);  // the labels are the grouped assignment of the returned models
    std::printf("sphere (geometric): maxRounds %zu -> %zu / %zu / %zu / %zu refits, refineModelsLMGrouped == the loop "
                "over refineModelsLM\n", maxRounds, r[0], r[1], r[2], r[3]);
  }
  lsqr_ctx_destroy(ctx);

  // any other estimator is refused
  PlaneParametersEstimator<3> plane(0.5);
  std::vector<std::vector<std::vector<double> > > pm(n, std::vector<std::vector<double> >(1, std::vector<double>(6, 0.0)));
  std::vector<int> labels;
  bool threw = false;
  try {
    R::refineModelsLMGrouped(pm, &plane, res, groups, n, 2, labels);
  } catch (const std::invalid_argument &) {
    threw = true;
  }
  CHECK(threw);
  SphereParametersEstimator<3> algebraic(0.5, SphereParametersEstimator<3>::ALGEBRAIC);
  std::vector<std::vector<std::vector<double> > > sm(start);
  threw = false;
  try {
    R::refineModelsLMGrouped(sm, &algebraic, res, groups, n, 2, labels);
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
