// refineDenseTest -- RANSAC<T,S>::assignToModelsDense / refineModelsDense of the drop-in headers on a mixture of linear
// regressions with n = 3, read from a file so that tests/test_cpp_assign_refine_dense.py can run Context.refine_dense on
// the same rows and compare bit for bit.
//   usage: refineDenseTest FILE DELTA MAX_ROUNDS
//   FILE: uint64 N, uint64 M, N rows of 4 doubles (a[0..3), b), M start regressions of 3 doubles
//   prints: "rounds R converged C", "labels l0 l1 ...", "assign l0 l1 ..." (assignToModelsDense of the returned
//   models), one "model m 0x... 0x... 0x..." line per regression (the doubles' bit patterns) and "refused 1" when any
//   other estimator is turned away.  Exit code 0 == the calls ran.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "DenseLinearEquationSystemParametersEstimator.h"
#include "PlaneParametersEstimator.h"
#include "RANSAC.h"

using namespace lsqrRecipes;

int main(int argc, char **argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: %s FILE DELTA MAX_ROUNDS\n", argv[0]);
    return 2;
  }
  typedef AugmentedRow<double, 3> RT;
  typedef RANSAC<RT, double> R;
  std::FILE *f = std::fopen(argv[1], "rb");
  uint64_t head[2];
  if (!f || std::fread(head, sizeof(uint64_t), 2, f) != 2) return 2;
  const size_t N = (size_t)head[0], M = (size_t)head[1];
  std::vector<double> raw(4 * N + 3 * M);
  if (std::fread(&raw[0], sizeof(double), raw.size(), f) != raw.size()) return 2;
  std::fclose(f);
  std::vector<RT> data(N);
  for (size_t i = 0; i < N; i++) data[i].set(&raw[4 * i], raw[4 * i + 3]);
  std::vector<std::vector<double> > models(M);
  for (size_t m = 0; m < M; m++) models[m].assign(&raw[4 * N + 3 * m], &raw[4 * N + 3 * m] + 3);

  DenseLinearEquationSystemParametersEstimator<double, 3> est(std::atof(argv[2]));
  std::vector<int> labels, again;
  bool converged = false;
  const size_t rounds = R::refineModelsDense(models, &est, data, (size_t)std::atol(argv[3]), labels, &converged);
  R::assignToModelsDense(models, &est, data, again);
  std::printf("rounds %zu converged %d\nlabels", rounds, (int)converged);
  for (size_t i = 0; i < labels.size(); i++) std::printf(" %d", labels[i]);
  std::printf("\nassign");
  for (size_t i = 0; i < again.size(); i++) std::printf(" %d", again[i]);
  std::printf("\n");
  for (size_t m = 0; m < M; m++) {
    std::printf("model %zu", m);
    for (size_t j = 0; j < models[m].size(); j++) {
      uint64_t u;
      std::memcpy(&u, &models[m][j], sizeof u);
      std::printf(" 0x%016llx", (unsigned long long)u);
    }
    std::printf("\n");
  }

  // any other estimator is refused
  typedef Point<double, 3> P3;
  PlaneParametersEstimator<3> plane(0.5);
  std::vector<P3> pts(8);
  std::vector<std::vector<double> > pm(1, std::vector<double>(6, 0.0));
  pm[0][0] = 1.0;
  std::vector<int> pl;
  int refused = 0;
  try {
    RANSAC<P3, double>::refineModelsDense(pm, &plane, pts, 2, pl);
  } catch (const std::invalid_argument &) {
    refused++;
  }
  try {
    RANSAC<P3, double>::assignToModelsDense(pm, &plane, pts, pl);
  } catch (const std::invalid_argument &) {
    refused++;
  }
  std::printf("refused %d\n", refused == 2 ? 1 : 0);
  return 0;
}
