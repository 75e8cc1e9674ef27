// assignRefineDenseGroupedTest -- RANSAC<T,S>::assignToModelsDenseGrouped / refineModelsDenseGrouped, the grouped device
// assign and refine of the dense linear system.  On three groups of two regressions each (n = 3) they must equal the
// per-group loop of assignToModelsDense / refineModelsDense on the gathers -- the same labels, rounds and stops,
// parameters bit for bit -- and the C ABI calls they wrap.  Any other estimator is refused.
// Exit code 0 == all passed.
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>
#include <vector>

#include "DenseLinearEquationSystemParametersEstimator.h"
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

static const size_t DIM = 3;
typedef AugmentedRow<double, 3> RT;
typedef RANSAC<RT, double> R;
static std::mt19937_64 gen(2031);
static double G(double s) { return std::normal_distribution<double>(0.0, s)(gen); }

static void dense() {
  const size_t n = 3, MM = 2;
  const size_t sizes[n] = {700, 255, 1100};  // chunks of 256 rows: three, one short of one, five
  const double sigma = 0.01, delta = 4 * sigma;
  std::vector<std::vector<RT> > sets(n);
  std::vector<std::vector<std::vector<double> > > start(n);
  for (size_t g = 0; g < n; g++) {
    double x[2][DIM];
    start[g].resize(MM);
    for (size_t m = 0; m < MM; m++) {
      start[g][m].resize(DIM);
      for (size_t j = 0; j < DIM; j++) {
        x[m][j] = G(1.0);
        start[g][m][j] = x[m][j] + G(0.5 * sigma);  // off the planted regression, inside the noise band
      }
    }
    sets[g].resize(sizes[g]);
    for (size_t i = 0; i < sizes[g]; i++) {
      double a[DIM], b = G(sigma);
      for (size_t j = 0; j < DIM; j++) a[j] = G(1.0), b += a[j] * x[i % 2][j];
      sets[g][i].set(a, b);
    }
  }
  // interleaved row by row; every 89th row goes to no group
  std::vector<RT> data;
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
        groups.push_back(k % 89 == 0 ? (k % 2 ? -1 : (int)n + 2) : (int)g);
      }
  }
  const size_t N = data.size();
  DenseLinearEquationSystemParametersEstimator<double, 3> est(delta);
  ResidentData<RT> res(data);

  // the C ABI on a context of our own
  lsqr_model_cfg cfg;
  CHECK(est.deviceModel(cfg));
  CHECK(cfg.model == LSQR_MODEL_DENSE && cfg.dim == (int32_t)DIM);
  lsqr_ctx *ctx = NULL;
  CHECK(lsqr_ctx_create(0, &ctx) == LSQR_OK);
  CHECK(lsqr_set_model(ctx, &cfg) == LSQR_OK);
  CHECK(lsqr_upload(ctx, &data[0], N, sizeof(RT)) == LSQR_OK);
  std::vector<double> par(n * MM * DIM, 0.0);
  std::vector<size_t> nModels(n, MM);
  for (size_t g = 0; g < n; g++)
    for (size_t m = 0; m < MM; m++)
      for (size_t j = 0; j < DIM; j++) par[(g * MM + m) * DIM + j] = start[g][m][j];
  std::vector<int32_t> glab(groups.begin(), groups.end()), lab(N), status(n * MM), conv(n);
  std::vector<lsqr_fit_info> fits(n * MM);
  std::vector<size_t> rounds(n);

  // the per-group gathers
  std::vector<std::vector<RT> > own(n);
  std::vector<std::vector<size_t> > index(n);
  for (size_t i = 0; i < N; i++)
    if (groups[i] >= 0 && groups[i] < (int)n) own[groups[i]].push_back(data[i]), index[groups[i]].push_back(i);

  {  // assignToModelsDenseGrouped
    CHECK(lsqr_assign_dense_grouped(ctx, &glab[0], n, 0, &par[0], &nModels[0], MM, &lab[0], NULL, NULL, NULL) == LSQR_OK);
    std::vector<int> labels;
    R::assignToModelsDenseGrouped(start, &est, res, groups, n, labels);
    CHECK(labels.size() == N && std::equal(labels.begin(), labels.end(), lab.begin()));
    for (size_t g = 0; g < n; g++) {
      std::vector<int> want;
      R::assignToModelsDense(start[g], &est, own[g], want);
      CHECK(want.size() == index[g].size());
      for (size_t k = 0; k < index[g].size(); k++) CHECK(labels[index[g][k]] == want[k]);
    }
    for (size_t i = 0; i < N; i++)
      if (groups[i] < 0 || groups[i] >= (int)n) CHECK(labels[i] == -1);
    std::printf("dense: assignToModelsDenseGrouped == the loop over assignToModelsDense\n");
  }

  for (size_t maxRounds = 1; maxRounds <= 8; maxRounds += 7) {
    std::vector<double> q(par);
    CHECK(lsqr_refine_dense_grouped(ctx, &glab[0], n, 0, &q[0], &nModels[0], MM, maxRounds, &lab[0], NULL, NULL,
                                    &fits[0], &status[0], &rounds[0], &conv[0]) == LSQR_OK);
    std::vector<std::vector<std::vector<double> > > models(start);
    std::vector<int> labels;
    std::vector<bool> converged;
    const std::vector<size_t> r = R::refineModelsDenseGrouped(models, &est, res, groups, n, maxRounds, labels, &converged);
    CHECK(r == rounds && labels.size() == N && std::equal(labels.begin(), labels.end(), lab.begin()));
    for (size_t g = 0; g < n; g++) {
      CHECK(r[g] >= 1 && converged[g] == (conv[g] != 0));
      std::vector<std::vector<double> > want(start[g]);
      std::vector<int> wantLabels;
      bool wantConv = false;
      const size_t wantRounds = R::refineModelsDense(want, &est, own[g], maxRounds, wantLabels, &wantConv);
      CHECK(r[g] == wantRounds && converged[g] == wantConv && models[g].size() == want.size());
      for (size_t m = 0; m < want.size(); m++) {
        CHECK(models[g][m].size() == DIM && std::memcmp(&models[g][m][0], &want[m][0], sizeof(double) * DIM) == 0);
        CHECK(std::memcmp(&models[g][m][0], &q[(g * MM + m) * DIM], sizeof(double) * DIM) == 0);
        CHECK(status[g * MM + m] == LSQR_OK && fits[g * MM + m].n_params == (int32_t)DIM);
        CHECK(fits[g * MM + m].reserved == 0 && fits[g * MM + m].n_used >= DIM);
      }
      for (size_t k = 0; k < index[g].size(); k++) CHECK(labels[index[g][k]] == wantLabels[k]);
    }
    for (size_t i = 0; i < N; i++)
      if (groups[i] < 0 || groups[i] >= (int)n) CHECK(labels[i] == -1);
    std::vector<int> again;
    R::assignToModelsDenseGrouped(models, &est, res, groups, n, again);
    CHECK(again == labels);  // the labels are the grouped assignment of the returned models
    std::printf("dense: maxRounds %zu -> %zu / %zu / %zu refits, refineModelsDenseGrouped == the loop over "
                "refineModelsDense\n", maxRounds, r[0], r[1], r[2]);
  }
  lsqr_ctx_destroy(ctx);

  // any other estimator is refused
  typedef Point<double, 3> P3;
  PlaneParametersEstimator<3> plane(0.5);
  std::vector<P3> pts(8);
  ResidentData<P3> pres(pts);
  std::vector<int> pg(8, 0), pl;
  std::vector<std::vector<std::vector<double> > > pm(1, std::vector<std::vector<double> >(1, std::vector<double>(6, 0.0)));
  pm[0][0][0] = 1.0;
  int refused = 0;
  try {
    RANSAC<P3, double>::refineModelsDenseGrouped(pm, &plane, pres, pg, 1, 2, pl);
  } catch (const std::invalid_argument &) {
    refused++;
  }
  try {
    RANSAC<P3, double>::assignToModelsDenseGrouped(pm, &plane, pres, pg, 1, pl);
  } catch (const std::invalid_argument &) {
    refused++;
  }
  CHECK(refused == 2);
}

int main() {
  dense();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
