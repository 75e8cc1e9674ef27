// refineRigidTest -- RANSAC<T,S>::assignToModelsRigid / refineModelsRigid of the drop-in headers for absolute
// orientation (std::pair<Point3D,Point3D>), pivot calibration (Frame) and ray intersection (Ray3D), on a scene read from
// a file so that tests/test_cpp_assign_refine_rigid.py can run Context.refine_rigid on the same records and compare bit
// for bit.
//   usage: refineRigidTest refuse
//          refineRigidTest absor|pivot|ray FILE DELTA MAX_ROUNDS
//   FILE: uint64 N, uint64 M, N records of 6 / 13 / 6 doubles, M start models of 7 / 6 / 3 doubles
//   prints: "rounds R converged C", "labels l0 l1 ...", "assign l0 l1 ..." (assignToModelsRigid of the returned
//   models) and one "model m 0x... ..." line per model (the doubles' bit patterns).  `refuse` touches no device: it
//   prints "refused 1" when every other estimator is turned away with std::invalid_argument, and "empty 1" when no
//   models or no records give labels of -1 and no rounds.  Exit code 0 == the calls ran.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "AbsoluteOrientationParametersEstimator.h"
#include "DenseLinearEquationSystemParametersEstimator.h"
#include "PivotCalibrationParametersEstimator.h"
#include "PlaneParametersEstimator.h"
#include "RANSAC.h"
#include "RayIntersectionParametersEstimator.h"
#include "SphereParametersEstimator.h"

using namespace lsqrRecipes;

typedef std::pair<Point3D, Point3D> PairT;

static void fill(PairT &r, const double *x) {
  for (int i = 0; i < 3; i++) r.first[i] = x[i], r.second[i] = x[3 + i];
}
static void fill(Frame &r, const double *x) {
  r.setRotationMatrix(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], x[8]);
  r.setTranslation(x[9], x[10], x[11]);
}
static void fill(Ray3D &r, const double *x) {
  for (int i = 0; i < 3; i++) r.p[i] = x[i], r.n[i] = x[3 + i];
}

template <class T, class Est>
static int run(Est &est, int width, int P, const char *file, size_t maxRounds) {
  typedef RANSAC<T, double> R;
  std::FILE *f = std::fopen(file, "rb");
  uint64_t head[2];
  if (!f || std::fread(head, sizeof(uint64_t), 2, f) != 2) return 2;
  const size_t N = (size_t)head[0], M = (size_t)head[1];
  std::vector<double> raw(width * N + P * M);
  if (std::fread(&raw[0], sizeof(double), raw.size(), f) != raw.size()) return 2;
  std::fclose(f);
  std::vector<T> data(N);
  for (size_t i = 0; i < N; i++) fill(data[i], &raw[width * i]);
  std::vector<std::vector<double> > models(M);
  for (size_t m = 0; m < M; m++) models[m].assign(&raw[width * N + P * m], &raw[width * N + P * m] + P);

  std::vector<int> labels, again;
  bool converged = false;
  const size_t rounds = R::refineModelsRigid(models, &est, data, maxRounds, labels, &converged);
  R::assignToModelsRigid(models, &est, data, again);
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
  return 0;
}

// both calls must throw std::invalid_argument for this estimator
template <class T, class Est>
static int refused(Est *est, size_t P) {
  std::vector<T> pts(8);
  std::vector<std::vector<double> > pm(1, std::vector<double>(P, 0.0));
  std::vector<int> pl;
  int n = 0;
  try {
    RANSAC<T, double>::refineModelsRigid(pm, est, pts, 2, pl);
  } catch (const std::invalid_argument &) {
    n++;
  }
  try {
    RANSAC<T, double>::assignToModelsRigid(pm, est, pts, pl);
  } catch (const std::invalid_argument &) {
    n++;
  }
  return n == 2 ? 1 : 0;
}

static int refuse() {
  typedef Point<double, 3> P3;
  PlaneParametersEstimator<3> plane(0.5);
  SphereParametersEstimator<3> sphere(0.5);
  DenseLinearEquationSystemParametersEstimator<double, 3> dense(0.5);
  int ok = refused<P3>(&plane, 6) + refused<P3>(&sphere, 4) + refused<AugmentedRow<double, 3> >(&dense, 3);
  ok += refused<P3>((PlaneParametersEstimator<3> *)NULL, 6);  // a null estimator
  std::printf("refused %d\n", ok == 4 ? 1 : 0);

  // nothing to do: labels of -1, no rounds, and no device call (this mode must run without a GPU)
  RayIntersectionParametersEstimator ray(1.0, 0.017453292519943295);
  std::vector<Ray3D> rays(5), none;
  std::vector<std::vector<double> > noModels, one(1, std::vector<double>(3, 0.0));
  std::vector<int> labels(3, 7);
  bool converged = true;
  int empty = 0;
  empty += RANSAC<Ray3D, double>::refineModelsRigid(noModels, &ray, rays, 4, labels, &converged) == 0 &&
           labels == std::vector<int>(5, -1) && !converged;
  RANSAC<Ray3D, double>::assignToModelsRigid(noModels, &ray, rays, labels);
  empty += labels == std::vector<int>(5, -1);
  empty += RANSAC<Ray3D, double>::refineModelsRigid(one, &ray, none, 4, labels, &converged) == 0 && labels.empty();
  std::printf("empty %d\n", empty == 3 ? 1 : 0);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && std::string(argv[1]) == "refuse") return refuse();
  if (argc != 5) {
    std::fprintf(stderr, "usage: %s refuse | absor|pivot|ray FILE DELTA MAX_ROUNDS\n", argv[0]);
    return 2;
  }
  const std::string kind = argv[1];
  const double delta = std::atof(argv[3]);
  const size_t maxRounds = (size_t)std::atol(argv[4]);
  if (kind == "absor") {
    AbsoluteOrientationParametersEstimator est(delta);
    return run<PairT>(est, 6, 7, argv[2], maxRounds);
  }
  if (kind == "pivot") {
    PivotCalibrationEstimator est(delta);
    return run<Frame>(est, 13, 6, argv[2], maxRounds);
  }
  if (kind == "ray") {
    RayIntersectionParametersEstimator est(delta, 0.017453292519943295);
    return run<Ray3D>(est, 6, 3, argv[2], maxRounds);
  }
  return 2;
}
