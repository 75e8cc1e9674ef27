// RANSAC.h -- drop-in for the reference's parametersEstimators/RANSAC.h(.hxx): the same two static
// compute() overloads, argument meaning, return value (fraction of the data in the winning
// consensus set) and failure conventions, with the work done on an MI355X through the C ABI of
// include/lsqr_hip.h (hypothesis batches -> minimal solves -> agree() scan -> first-max winner ->
// consensus mask -> leastSquaresEstimate, and a host replay of the serial adaptive loop so that the
// result equals the serial algorithm's for the same subset stream).
//
// Differences a maintainer should know about:
//  * the subset stream comes from a seeded counter-based sampler instead of srand(time(NULL))/rand()
//    (RANSAC.hxx:44,59): runs are reproducible; RANSAC<T,S>::seed() sets the stream;
//  * estimators that expose a device model (ParametersEstimator::deviceModel -- every estimator this
//    library ships) run on the MI355X and nowhere else: without a usable device compute() throws.
//    A USER-DEFINED ParametersEstimator subclass (the plugin use the reference advertises,
//    readme.txt:40-72) has no device model; for it compute() runs the reference's serial loop
//    (RANSAC.hxx:49-139) over the estimator's own virtuals on the host, fed by the same counter-based
//    subset stream and the same replay of the adaptive stopping rule (lsqr_sample_subsets /
//    lsqr_replay), so a user estimator that restates a built-in one reaches the same iteration count,
//    winner and consensus set as the device path.
#ifndef _RANSAC_H_
#define _RANSAC_H_

#include <algorithm>
#include <set>
#include <stdexcept>
#include <vector>

#include "LsqrDevice.h"
#include "ParametersEstimator.h"

namespace lsqrRecipes {

template <class T, class S>
class RANSAC {
 public:
  // probabilistic search, reference RANSAC.h:75-79
  static double compute(std::vector<S> &parameters, ParametersEstimator<T, S> *paramEstimator,
                        std::vector<T> &data, double desiredProbabilityForNoOutliers,
                        std::vector<bool> *consensusSet = NULL) {
    lsqr_model_cfg cfg;
    if (!paramEstimator) throw std::invalid_argument("lsqrRecipes::RANSAC: null estimator");
    // RANSAC.hxx:16-19: invalid input returns 0 and leaves `parameters` untouched
    if (data.size() < paramEstimator->numForEstimate() || desiredProbabilityForNoOutliers >= 1.0 ||
        desiredProbabilityForNoOutliers <= 0.0)
      return 0;
    if (!paramEstimator->deviceModel(cfg) || forceHostLoop())
      return pluginCompute(parameters, paramEstimator, data, desiredProbabilityForNoOutliers, consensusSet);
    detail::Device &d = detail::Device::instance();
    std::vector<double> p(64);
    std::vector<uint8_t> cons(consensusSet ? data.size() : 0);
    lsqr_ransac_info info;
    bool ok;
    if (lsqr_multi *m = d.multi()) {  // LSQR_DEVICES lists several devices: batches sharded over them
      d.checkMulti(lsqr_multi_set_model(m, &cfg));
      d.checkMulti(lsqr_multi_upload(m, &data[0], data.size(), sizeof(T)));
      parameters.clear();
      ok = d.checkMulti(lsqr_multi_ransac(m, desiredProbabilityForNoOutliers, seed(), &p[0],
                                          consensusSet ? &cons[0] : NULL, &info));
      lastInfo() = info;
      return finish(ok, info, p, cons, parameters, consensusSet);
    }
    d.model(cfg);
    d.check(lsqr_upload(d.ctx(), &data[0], data.size(), sizeof(T)));
    parameters.clear();  // RANSAC.hxx:43
    ok = d.check(lsqr_ransac(d.ctx(), desiredProbabilityForNoOutliers, seed(), NULL, 0, &p[0],
                             consensusSet ? &cons[0] : NULL, &info));
    lastInfo() = info;
    return finish(ok, info, p, cons, parameters, consensusSet);
  }

  // the same on records that are already resident on the device (lsqrRecipes::ResidentData, LsqrDevice.h): no
  // upload; repeat with other thresholds / probabilities / seeds / estimators of the same record type
  static double compute(std::vector<S> &parameters, ParametersEstimator<T, S> *paramEstimator,
                        ResidentData<T> &data, double desiredProbabilityForNoOutliers,
                        std::vector<bool> *consensusSet = NULL) {
    lsqr_model_cfg cfg;
    if (!paramEstimator) throw std::invalid_argument("lsqrRecipes::RANSAC: null estimator");
    if (data.size() < paramEstimator->numForEstimate() || desiredProbabilityForNoOutliers >= 1.0 ||
        desiredProbabilityForNoOutliers <= 0.0)
      return 0;
    if (!paramEstimator->deviceModel(cfg))
      throw std::invalid_argument("lsqrRecipes::RANSAC: ResidentData needs an estimator with a device model");
    lsqr_ctx *ctx = data.attach(cfg);
    std::vector<double> p(64);
    std::vector<uint8_t> cons(consensusSet ? data.size() : 0);
    lsqr_ransac_info info;
    parameters.clear();
    bool ok = data.check(lsqr_ransac(ctx, desiredProbabilityForNoOutliers, seed(), NULL, 0, &p[0],
                                     consensusSet ? &cons[0] : NULL, &info));
    lastInfo() = info;
    return finish(ok, info, p, cons, parameters, consensusSet);
  }

  // exhaustive search over all subsets, reference RANSAC.h:111-113
  static double compute(std::vector<S> &parameters, ParametersEstimator<T, S> *paramEstimator,
                        std::vector<T> &data, std::vector<bool> *consensusSet = NULL) {
    lsqr_model_cfg cfg;
    if (!paramEstimator) throw std::invalid_argument("lsqrRecipes::RANSAC: null estimator");
    parameters.clear();  // RANSAC.hxx:165 clears before the size check
    if (data.size() < paramEstimator->numForEstimate()) return 0;
    if (!paramEstimator->deviceModel(cfg) || forceHostLoop())
      return pluginComputeExhaustive(parameters, paramEstimator, data, consensusSet);
    detail::Device &d = detail::Device::instance();
    d.model(cfg);
    d.check(lsqr_upload(d.ctx(), &data[0], data.size(), sizeof(T)));
    std::vector<double> p(64);
    std::vector<uint8_t> cons(consensusSet ? data.size() : 0);
    lsqr_ransac_info info;
    bool ok = d.check(lsqr_ransac_exhaustive(d.ctx(), &p[0], consensusSet ? &cons[0] : NULL, &info));
    lastInfo() = info;
    return finish(ok, info, p, cons, parameters, consensusSet);
  }

  // Many independent probabilistic searches (not in the reference): problem j is data[j] and walks sampler stream
  // seed() + j, so computeMany(...)[j] equals compute() on data[j] after seed(seed() + j).  Per problem as
  // compute(): invalid input returns 0 and leaves parameters[j] untouched, a search that finds nothing clears it.
  // Plane, line, algebraic sphere, absolute orientation, pivot calibration, ray intersection and the 2-D line run in
  // ONE device call (lsqr_ransac_many: one upload, batched rounds, one finish; the records are packed sizeof(T)
  // apart, as compute() uploads them); the geometric sphere (SphereParametersEstimator's default) runs in one
  // lsqr_ransac_many_lm call, its LM finish batched on the device too, and the dense linear system
  // (DenseLinearEquationSystemParametersEstimator) in one lsqr_ransac_many_dense call.  Estimators without a device
  // model loop over the plugin path, other device estimators (US calibrations, plane phantom) over compute(), with
  // the same seeds.
  // Under LSQR_DEVICES the batched call runs on the first listed device's context (problems are not sharded over
  // devices).  lastInfo() is not updated.
  static std::vector<double> computeMany(std::vector<std::vector<S> > &parameters,
                                         ParametersEstimator<T, S> *paramEstimator,
                                         const std::vector<std::vector<T> > &data, double desiredProbabilityForNoOutliers,
                                         std::vector<std::vector<bool> > *consensusSets = NULL) {
    if (!paramEstimator) throw std::invalid_argument("lsqrRecipes::RANSAC: null estimator");
    const size_t n = data.size();
    const double p = desiredProbabilityForNoOutliers;
    parameters.resize(n);
    if (consensusSets) consensusSets->resize(n);
    std::vector<double> fraction(n, 0.0);
    if (n == 0 || p >= 1.0 || p <= 0.0) return fraction;  // RANSAC.hxx:16-19 for every problem
    lsqr_model_cfg cfg;
    const bool device = paramEstimator->deviceModel(cfg) && !forceHostLoop();
    // the geometric sphere's LM finish: lsqr_ransac_many_lm; the closed-form fits: lsqr_ransac_many
    const bool lm = device && cfg.model == LSQR_MODEL_SPHERE && cfg.ls_type == LSQR_LS_GEOMETRIC;
    const bool dense = device && cfg.model == LSQR_MODEL_DENSE;  // lsqr_ransac_many_dense
    const bool batched = device && (cfg.model == LSQR_MODEL_PLANE || cfg.model == LSQR_MODEL_LINE ||
                                    cfg.model == LSQR_MODEL_SPHERE || cfg.model == LSQR_MODEL_DENSE ||
                                    cfg.model == LSQR_MODEL_ABSOR || cfg.model == LSQR_MODEL_PIVOT ||
                                    cfg.model == LSQR_MODEL_RAY || cfg.model == LSQR_MODEL_LINE2D);
    if (!batched) {
      const uint64_t s0 = seed();
      for (size_t j = 0; j < n; j++) {
        seed() = s0 + j;
        // (compute() reads the records only; it takes them by non-const reference as the reference does)
        fraction[j] = compute(parameters[j], paramEstimator, const_cast<std::vector<T> &>(data[j]), p,
                              consensusSets ? &(*consensusSets)[j] : NULL);
      }
      seed() = s0;
      return fraction;
    }
    std::vector<uint64_t> offsets(n + 1, 0), seeds(n);
    for (size_t j = 0; j < n; j++) {
      offsets[j + 1] = offsets[j] + data[j].size();
      seeds[j] = seed() + j;
    }
    std::vector<T> records;
    records.reserve((size_t)offsets[n]);
    for (size_t j = 0; j < n; j++) records.insert(records.end(), data[j].begin(), data[j].end());
    detail::Device &d = detail::Device::instance();
    lsqr_ctx *ctx = d.ctx();
    if (lsqr_multi *m = d.multi()) ctx = lsqr_multi_ctx(m, 0);
    d.check(lsqr_set_model(ctx, &cfg));
    const int P = lsqr_num_params(&cfg);
    std::vector<double> par(n * (size_t)P);
    std::vector<uint8_t> cons(consensusSets ? (size_t)offsets[n] : 0);
    std::vector<lsqr_ransac_info> info(n);
    std::vector<int32_t> status(n);
    d.check((lm ? lsqr_ransac_many_lm : dense ? lsqr_ransac_many_dense : lsqr_ransac_many)(
        ctx, records.empty() ? NULL : &records[0], sizeof(T), &offsets[0], n, p, &seeds[0], &par[0],
        cons.empty() ? NULL : &cons[0], &info[0], &status[0]));
    for (size_t j = 0; j < n; j++) {
      if (status[j] == LSQR_ERR_INVALID) continue;  // fewer records than a minimal subset: untouched, 0
      parameters[j].clear();  // RANSAC.hxx:43
      if (info[j].best_votes > 0 && consensusSets)
        (*consensusSets)[j].assign(cons.begin() + (size_t)offsets[j], cons.begin() + (size_t)offsets[j + 1]);
      if (status[j] == LSQR_OK) parameters[j].assign(&par[j * P], &par[j * P] + info[j].n_params);
      fraction[j] = info[j].fraction;
    }
    return fraction;
  }

  // Grouped RANSAC on resident records (not in the reference): problem g is the records i of `data` with
  // groups[i] == g, in their order; a label that is negative or >= nGroups puts the record in no problem.  Problem g
  // walks sampler stream seed() + g, so computeGrouped(...)[g] and parameters[g] equal what computeMany returns / leaves
  // for the per-group vectors; consensus (optional, one entry per record of `data`) is set where the record is in its
  // problem's consensus set.  The estimators computeMany batches run in ONE device call (lsqr_ransac_grouped: the
  // records are grouped on the device, where they already are; only the labels go up and the consensus comes down).
  // The estimators computeMany sends through its loop, and forceHostLoop(), go through computeMany itself on the
  // per-group vectors, gathered from the vector `data` was made from.  THAT VECTOR MUST THEN STILL BE ALIVE AND
  // UNCHANGED: ResidentData keeps a pointer to it, not a copy, and this is the one call that reads it after the
  // upload (the batched path never does).
  static std::vector<double> computeGrouped(std::vector<std::vector<S> > &parameters,
                                            ParametersEstimator<T, S> *paramEstimator, ResidentData<T> &data,
                                            const std::vector<int> &groups, size_t nGroups,
                                            double desiredProbabilityForNoOutliers,
                                            std::vector<bool> *consensus = NULL) {
    if (!paramEstimator) throw std::invalid_argument("lsqrRecipes::RANSAC: null estimator");
    if (groups.size() != data.size()) throw std::invalid_argument("lsqrRecipes::RANSAC: one group label per record");
    const size_t n = nGroups, N = data.size();
    const double p = desiredProbabilityForNoOutliers;
    parameters.resize(n);
    if (consensus) consensus->assign(N, false);
    std::vector<double> fraction(n, 0.0);
    if (n == 0 || N == 0 || p >= 1.0 || p <= 0.0) return fraction;  // RANSAC.hxx:16-19 for every problem
    lsqr_model_cfg cfg;
    const bool device = paramEstimator->deviceModel(cfg) && !forceHostLoop();
    const bool batched = device && (cfg.model == LSQR_MODEL_PLANE || cfg.model == LSQR_MODEL_LINE ||
                                    cfg.model == LSQR_MODEL_SPHERE || cfg.model == LSQR_MODEL_DENSE ||
                                    cfg.model == LSQR_MODEL_ABSOR || cfg.model == LSQR_MODEL_PIVOT ||
                                    cfg.model == LSQR_MODEL_RAY || cfg.model == LSQR_MODEL_LINE2D);
    if (!batched) {
      const T *host = data.hostRecords();
      std::vector<std::vector<T> > sets(n);
      std::vector<std::vector<size_t> > index(n);
      for (size_t i = 0; i < N; i++)
        if (groups[i] >= 0 && (size_t)groups[i] < n) {
          sets[(size_t)groups[i]].push_back(host[i]);
          index[(size_t)groups[i]].push_back(i);
        }
      std::vector<std::vector<bool> > cons;
      fraction = computeMany(parameters, paramEstimator, sets, p, consensus ? &cons : NULL);
      if (consensus)
        for (size_t g = 0; g < n; g++)
          for (size_t q = 0; q < cons[g].size(); q++) (*consensus)[index[g][q]] = cons[g][q];
      return fraction;
    }
    std::vector<uint64_t> seeds(n);
    for (size_t g = 0; g < n; g++) seeds[g] = seed() + g;
    std::vector<int32_t> labels(groups.begin(), groups.end());
    lsqr_ctx *ctx = data.attach(cfg);
    const int P = lsqr_num_params(&cfg);
    std::vector<double> par(n * (size_t)P);
    std::vector<uint8_t> cons(consensus ? N : 0);
    std::vector<lsqr_ransac_info> info(n);
    std::vector<int32_t> status(n);
    data.check(lsqr_ransac_grouped(ctx, &labels[0], n, 0, p, &seeds[0], &par[0], cons.empty() ? NULL : &cons[0], NULL,
                                   &info[0], &status[0]));
    for (size_t g = 0; g < n; g++) {
      if (status[g] == LSQR_ERR_INVALID) continue;  // fewer records than a minimal subset: untouched, 0
      parameters[g].clear();  // RANSAC.hxx:43
      if (status[g] == LSQR_OK) parameters[g].assign(&par[g * P], &par[g * P] + info[g].n_params);
      fraction[g] = info[g].fraction;
    }
    if (consensus)
      for (size_t i = 0; i < N; i++) (*consensus)[i] = cons[i] != 0;
    return fraction;
  }

  // Many independent exhaustive searches (not in the reference): the overload next to the probabilistic computeMany,
  // as the two compute() overloads stand side by side.  computeMany(...)[j] equals the exhaustive compute() on data[j]:
  // parameters[j] is cleared first, a problem of fewer records than a minimal subset returns 0.  Plane, line, sphere
  // (algebraic and geometric), absolute orientation, pivot calibration, ray intersection and the 2-D line run in ONE
  // device call (lsqr_ransac_many_exhaustive); the dense linear system, the other device estimators, estimators
  // without a device model and forceHostLoop() loop over compute().  lastInfo() is not updated by the batched call.
  static std::vector<double> computeMany(std::vector<std::vector<S> > &parameters,
                                         ParametersEstimator<T, S> *paramEstimator,
                                         const std::vector<std::vector<T> > &data,
                                         std::vector<std::vector<bool> > *consensusSets = NULL) {
    if (!paramEstimator) throw std::invalid_argument("lsqrRecipes::RANSAC: null estimator");
    const size_t n = data.size();
    parameters.resize(n);
    if (consensusSets) consensusSets->resize(n);
    std::vector<double> fraction(n, 0.0);
    if (n == 0) return fraction;
    lsqr_model_cfg cfg;
    const bool device = paramEstimator->deviceModel(cfg) && !forceHostLoop();
    const bool batched = device && (cfg.model == LSQR_MODEL_PLANE || cfg.model == LSQR_MODEL_LINE ||
                                    cfg.model == LSQR_MODEL_SPHERE || cfg.model == LSQR_MODEL_ABSOR ||
                                    cfg.model == LSQR_MODEL_PIVOT || cfg.model == LSQR_MODEL_RAY ||
                                    cfg.model == LSQR_MODEL_LINE2D);
    if (!batched) {
      for (size_t j = 0; j < n; j++)
        fraction[j] = compute(parameters[j], paramEstimator, const_cast<std::vector<T> &>(data[j]),
                              consensusSets ? &(*consensusSets)[j] : NULL);
      return fraction;
    }
    std::vector<uint64_t> offsets(n + 1, 0);
    for (size_t j = 0; j < n; j++) offsets[j + 1] = offsets[j] + data[j].size();
    std::vector<T> records;
    records.reserve((size_t)offsets[n]);
    for (size_t j = 0; j < n; j++) records.insert(records.end(), data[j].begin(), data[j].end());
    detail::Device &d = detail::Device::instance();
    lsqr_ctx *ctx = d.ctx();
    if (lsqr_multi *m = d.multi()) ctx = lsqr_multi_ctx(m, 0);
    d.check(lsqr_set_model(ctx, &cfg));
    const int P = lsqr_num_params(&cfg);
    std::vector<double> par(n * (size_t)P);
    std::vector<uint8_t> cons(consensusSets ? (size_t)offsets[n] : 0);
    std::vector<lsqr_ransac_info> info(n);
    std::vector<int32_t> status(n);
    d.check(lsqr_ransac_many_exhaustive(ctx, records.empty() ? NULL : &records[0], sizeof(T), &offsets[0], n, &par[0],
                                        cons.empty() ? NULL : &cons[0], &info[0], &status[0]));
    for (size_t j = 0; j < n; j++) {
      parameters[j].clear();  // RANSAC.hxx:165 clears before the size check
      if (info[j].best_votes > 0 && consensusSets)
        (*consensusSets)[j].assign(cons.begin() + (size_t)offsets[j], cons.begin() + (size_t)offsets[j + 1]);
      if (status[j] == LSQR_OK) parameters[j].assign(&par[j * P], &par[j * P] + info[j].n_params);
      fraction[j] = info[j].fraction;
    }
    return fraction;
  }

  // Sequential RANSAC (not in the reference): find the best model, take its consensus set out of the data, search
  // what is left, up to maxModels times.  Round r walks sampler stream seed() + r and is decided as compute() would
  // decide it on the records no earlier round claimed, in their original order; it is accepted when it yields
  // parameters and its consensus set has at least max(minVotes, 1) records.  The first round that is not accepted is
  // the last one and claims nothing; no round runs on fewer records than a minimal subset.
  //   parameters: one vector per ACCEPTED round.  Return value: the fraction of every round that RAN, each relative to
  //   the records that were left for it -- one entry more than `parameters` when the last round was rejected.
  //   labels (optional): per record of `data` the round that claimed it, else -1.  lastInfo(): the last round that ran.
  //   Invalid input (as compute(): too few records, p outside (0, 1)) or maxModels == 0: nothing runs, both are empty.
  // Estimators with a device model run in ONE device call (lsqr_ransac_sequential: one upload, the survivors of every
  // round compacted on the device); estimators without one, and forceHostLoop(), run the same loop on the host over
  // the plugin path with the consensus set erased, on the same seeds.  Under LSQR_DEVICES the call runs on the first
  // listed device's context.
  static std::vector<double> computeSequential(std::vector<std::vector<S> > &parameters,
                                               ParametersEstimator<T, S> *paramEstimator, std::vector<T> &data,
                                               double desiredProbabilityForNoOutliers, size_t maxModels,
                                               size_t minVotes, std::vector<int> *labels = NULL) {
    lsqr_model_cfg cfg;
    if (!paramEstimator) throw std::invalid_argument("lsqrRecipes::RANSAC: null estimator");
    const double p = desiredProbabilityForNoOutliers;
    parameters.clear();
    if (labels) labels->assign(data.size(), -1);
    if (maxModels == 0 || data.size() < paramEstimator->numForEstimate() || p >= 1.0 || p <= 0.0)
      return std::vector<double>();
    if (!paramEstimator->deviceModel(cfg) || forceHostLoop())
      return pluginComputeSequential(parameters, paramEstimator, data, p, maxModels, minVotes, labels);
    detail::Device &d = detail::Device::instance();
    lsqr_ctx *ctx = d.ctx();
    if (lsqr_multi *m = d.multi()) ctx = lsqr_multi_ctx(m, 0);
    d.check(lsqr_set_model(ctx, &cfg));
    d.check(lsqr_upload(ctx, &data[0], data.size(), sizeof(T)));
    return sequentialOn(d, ctx, cfg, data.size(), parameters, p, maxModels, minVotes, labels);
  }

  // the same on resident records (lsqrRecipes::ResidentData): no upload; the records are only read
  static std::vector<double> computeSequential(std::vector<std::vector<S> > &parameters,
                                               ParametersEstimator<T, S> *paramEstimator, ResidentData<T> &data,
                                               double desiredProbabilityForNoOutliers, size_t maxModels,
                                               size_t minVotes, std::vector<int> *labels = NULL) {
    lsqr_model_cfg cfg;
    if (!paramEstimator) throw std::invalid_argument("lsqrRecipes::RANSAC: null estimator");
    const double p = desiredProbabilityForNoOutliers;
    parameters.clear();
    if (labels) labels->assign(data.size(), -1);
    if (maxModels == 0 || data.size() < paramEstimator->numForEstimate() || p >= 1.0 || p <= 0.0)
      return std::vector<double>();
    if (!paramEstimator->deviceModel(cfg))
      throw std::invalid_argument("lsqrRecipes::RANSAC: ResidentData needs an estimator with a device model");
    lsqr_ctx *ctx = data.attach(cfg);
    return sequentialOn(data, ctx, cfg, data.size(), parameters, p, maxModels, minVotes, labels);
  }

  // Nearest-model assignment (not in the reference), the follow-up of computeSequential: labels[i] is the model of
  // `models` that record i goes to, else -1.  Estimators whose device model lsqr_assign takes (plane, line, sphere,
  // 2-D line) run ONE device pass (lsqr_assign): the model with the smallest residual among those the record agrees
  // with, ties to the smaller index.  Every other estimator -- a user-defined one without a device model, the device
  // models lsqr_assign refuses, forceHostLoop() -- runs a plain host loop over the estimator's agree() virtual, the
  // FIRST agreeing model winning: the interface has no residual to compare (this mirrors the plugin path of
  // compute()).  No models, or no records: every label is -1.  More than 64 models on the device path, or a model
  // vector of the wrong length, throw std::invalid_argument.
  static void assignToModels(const std::vector<std::vector<S> > &models, ParametersEstimator<T, S> *paramEstimator,
                             std::vector<T> &data, std::vector<int> &labels) {
    lsqr_model_cfg cfg;
    if (!paramEstimator) throw std::invalid_argument("lsqrRecipes::RANSAC: null estimator");
    labels.assign(data.size(), -1);
    if (models.empty() || data.empty()) return;
    if (!paramEstimator->deviceModel(cfg) || forceHostLoop() || !assignOnDevice(cfg, false)) {
      pluginAssign(models, paramEstimator, data, labels);
      return;
    }
    detail::Device &d = detail::Device::instance();
    lsqr_ctx *ctx = d.ctx();
    if (lsqr_multi *m = d.multi()) ctx = lsqr_multi_ctx(m, 0);
    d.check(lsqr_set_model(ctx, &cfg));
    d.check(lsqr_upload(ctx, &data[0], data.size(), sizeof(T)));
    std::vector<double> par = packModels(models, cfg);
    std::vector<int32_t> lab(data.size());
    d.check(lsqr_assign(ctx, &par[0], models.size(), 0, &lab[0], NULL, NULL));
    labels.assign(lab.begin(), lab.end());
  }

  // Assignment and least-squares refit in turn: L_r = assignToModels(models_r); stop when r > 0 and L_r == L_{r-1}
  // (*converged = true) or r == maxRounds; else every model is fitted again on its own records (leastSquaresEstimate;
  // a model with fewer than numForEstimate() records, or whose fit comes back empty, keeps its parameters), r += 1.
  // -> the refits done; `models` and `labels` are models_r and L_r, so the labels are always the assignment of the
  // returned models.  The device path is ONE call (lsqr_refine: a round is one pass over the records on the device);
  // the host loop, taken as in assignToModels and for the geometric sphere (its fit is iterative), assigns by the
  // first agreeing model.  refineModelsLM (below) is the device path of the geometric sphere.
  static size_t refineModels(std::vector<std::vector<S> > &models, ParametersEstimator<T, S> *paramEstimator,
                             std::vector<T> &data, size_t maxRounds, std::vector<int> &labels,
                             bool *converged = NULL) {
    lsqr_model_cfg cfg;
    if (!paramEstimator) throw std::invalid_argument("lsqrRecipes::RANSAC: null estimator");
    labels.assign(data.size(), -1);
    if (converged) *converged = false;
    if (models.empty() || data.empty()) return 0;
    if (!paramEstimator->deviceModel(cfg) || forceHostLoop() || !assignOnDevice(cfg, true))
      return pluginRefine(models, paramEstimator, data, maxRounds, labels, converged);
    return refineOnDevice(lsqr_refine, cfg, models, data, maxRounds, labels, converged);
  }

  // refineModels for the sphere estimator with the geometric least-squares fit (its default), on the device: ONE call
  // (lsqr_refine_lm).  The loop, the stop rules and what comes back are refineModels'; the assignment is the device's
  // (the NEAREST agreeing model, not the first), and the refit of a model is a Levenberg-Marquardt run over its own
  // records from their algebraic fit, as SphereParametersEstimator::leastSquaresEstimate runs one; a model whose run
  // gives no result keeps its parameters.  Any other estimator throws std::invalid_argument: refineModels takes it.
  static size_t refineModelsLM(std::vector<std::vector<S> > &models, ParametersEstimator<T, S> *paramEstimator,
                               std::vector<T> &data, size_t maxRounds, std::vector<int> &labels,
                               bool *converged = NULL) {
    lsqr_model_cfg cfg;
    if (!paramEstimator) throw std::invalid_argument("lsqrRecipes::RANSAC: null estimator");
    if (!paramEstimator->deviceModel(cfg) || cfg.model != LSQR_MODEL_SPHERE || cfg.ls_type != LSQR_LS_GEOMETRIC)
      throw std::invalid_argument("lsqrRecipes::RANSAC: refineModelsLM takes the geometric sphere only");
    labels.assign(data.size(), -1);
    if (converged) *converged = false;
    if (models.empty() || data.empty()) return 0;
    return refineOnDevice(lsqr_refine_lm, cfg, models, data, maxRounds, labels, converged);
  }

  // assignToModels / refineModels for DenseLinearEquationSystemParametersEstimator<double,n> (a mixture of linear
  // regressions), which those two send to the host loop: ONE device call each (lsqr_assign_dense / lsqr_refine_dense).
  // The assignment is the device's -- the regression with the smallest |a . x - b| among those the row agrees with,
  // ties to the smaller index --, the loop, the stop rules and what comes back are refineModels', and the refit of a
  // regression is the least-squares solution over its own rows as leastSquaresEstimate computes it; a regression with
  // fewer than n rows, or whose rows do not have full rank, keeps its parameters.  Any other estimator throws
  // std::invalid_argument; more than 64 models, or a model vector of the wrong length, likewise.
  static void assignToModelsDense(const std::vector<std::vector<S> > &models,
                                  ParametersEstimator<T, S> *paramEstimator, std::vector<T> &data,
                                  std::vector<int> &labels) {
    lsqr_model_cfg cfg;
    denseOnly(paramEstimator, cfg, "assignToModelsDense");
    labels.assign(data.size(), -1);
    if (models.empty() || data.empty()) return;
    detail::Device &d = detail::Device::instance();
    lsqr_ctx *ctx = d.ctx();
    if (lsqr_multi *m = d.multi()) ctx = lsqr_multi_ctx(m, 0);
    d.check(lsqr_set_model(ctx, &cfg));
    d.check(lsqr_upload(ctx, &data[0], data.size(), sizeof(T)));
    std::vector<double> par = packModels(models, cfg);
    std::vector<int32_t> lab(data.size());
    d.check(lsqr_assign_dense(ctx, &par[0], models.size(), 0, &lab[0], NULL, NULL));
    labels.assign(lab.begin(), lab.end());
  }

  static size_t refineModelsDense(std::vector<std::vector<S> > &models, ParametersEstimator<T, S> *paramEstimator,
                                  std::vector<T> &data, size_t maxRounds, std::vector<int> &labels,
                                  bool *converged = NULL) {
    lsqr_model_cfg cfg;
    denseOnly(paramEstimator, cfg, "refineModelsDense");
    labels.assign(data.size(), -1);
    if (converged) *converged = false;
    if (models.empty() || data.empty()) return 0;
    return refineOnDevice(lsqr_refine_dense, cfg, models, data, maxRounds, labels, converged);
  }

  // assignToModels / refineModels for AbsoluteOrientationParametersEstimator (weighted or not),
  // PivotCalibrationEstimator and RayIntersectionParametersEstimator, which those two send to the host loop: ONE device
  // call each (lsqr_assign_rigid / lsqr_refine_rigid).  The assignment is the device's -- the NEAREST agreeing model,
  // ties to the smaller index --, the loop, the stop rules and what comes back are refineModels', and the refit of a
  // model is its closed-form fit over its own records as leastSquaresEstimate computes it; a model with fewer than
  // numForEstimate() records, or whose fit comes back empty (rays all parallel, frames all the same), keeps its
  // parameters.  Any other estimator throws std::invalid_argument; more than 64 models, or a model vector of the wrong
  // length, likewise.
  static void assignToModelsRigid(const std::vector<std::vector<S> > &models,
                                  ParametersEstimator<T, S> *paramEstimator, std::vector<T> &data,
                                  std::vector<int> &labels) {
    lsqr_model_cfg cfg;
    rigidOnly(paramEstimator, cfg, "assignToModelsRigid");
    labels.assign(data.size(), -1);
    if (models.empty() || data.empty()) return;
    bool converged = false;
    std::vector<std::vector<S> > same(models);  // (no refit runs: maxRounds = 0 is the assignment)
    refineOnDevice(lsqr_refine_rigid, cfg, same, data, 0, labels, &converged);
  }

  static size_t refineModelsRigid(std::vector<std::vector<S> > &models, ParametersEstimator<T, S> *paramEstimator,
                                  std::vector<T> &data, size_t maxRounds, std::vector<int> &labels,
                                  bool *converged = NULL) {
    lsqr_model_cfg cfg;
    rigidOnly(paramEstimator, cfg, "refineModelsRigid");
    labels.assign(data.size(), -1);
    if (converged) *converged = false;
    if (models.empty() || data.empty()) return 0;
    return refineOnDevice(lsqr_refine_rigid, cfg, models, data, maxRounds, labels, converged);
  }

  // assignToModels with one model set per label on resident records (not in the reference), the follow-up of
  // computeGroupedSequential: `models` is what that call leaves in `parameters` (models[g]: the models of group g;
  // models.size() must be nGroups), `groups` and `data` are its own.  labels[i] is the model of models[groups[i]] that
  // record i goes to, as assignToModels decides it on the records of the group alone; -1 when none agrees, for a
  // record in no group (a negative label or one >= nGroups) and for a group without models.
  // The estimators assignToModels sends to the device run ONE device call for all groups (lsqr_assign_grouped: the
  // records are grouped on the device, where they already are; only the group labels go up and the labels come
  // down).  The others, and forceHostLoop(), loop over assignToModels on the per-group vectors, gathered from the vector
  // `data` was made from.  THAT VECTOR MUST THEN STILL BE ALIVE AND UNCHANGED (see computeGrouped).
  static void assignToModelsGrouped(const std::vector<std::vector<std::vector<S> > > &models,
                                    ParametersEstimator<T, S> *paramEstimator, ResidentData<T> &data,
                                    const std::vector<int> &groups, size_t nGroups, std::vector<int> &labels) {
    lsqr_model_cfg cfg;
    groupedArgs(models.size(), paramEstimator, data, groups, nGroups);
    const size_t n = nGroups, N = data.size();
    labels.assign(N, -1);
    if (n == 0 || N == 0) return;
    if (!paramEstimator->deviceModel(cfg) || forceHostLoop() || !assignOnDevice(cfg, false)) {
      std::vector<std::vector<T> > sets;
      std::vector<std::vector<size_t> > index;
      gatherGroups(data, groups, n, sets, index);
      for (size_t g = 0; g < n; g++) {
        std::vector<int> lab;
        assignToModels(models[g], paramEstimator, sets[g], lab);
        for (size_t q = 0; q < lab.size(); q++) labels[index[g][q]] = lab[q];
      }
      return;
    }
    size_t maxModels = 0;
    std::vector<size_t> nModels;
    std::vector<double> par = packGroupedModels(models, cfg, maxModels, nModels);
    if (maxModels == 0) return;
    std::vector<int32_t> glab(groups.begin(), groups.end()), lab(N);
    lsqr_ctx *ctx = data.attach(cfg);
    data.check(lsqr_assign_grouped(ctx, &glab[0], n, 0, &par[0], &nModels[0], maxModels, &lab[0], NULL, NULL, NULL));
    labels.assign(lab.begin(), lab.end());
  }

  // refineModels with one model set per label on resident records: every group runs refineModels' loop on its own
  // records and models and stops on its own.  -> the refits done per group; `models` and `labels` are every group's
  // models_r and L_r; (*converged)[g] says which stop it was.  A group without records or without models runs
  // nothing: 0 rounds, not converged.  Arguments and paths as for assignToModelsGrouped; the device path is ONE call
  // (lsqr_refine_grouped), the host path loops over refineModels (also for the geometric sphere, as there).
  static std::vector<size_t> refineModelsGrouped(std::vector<std::vector<std::vector<S> > > &models,
                                                 ParametersEstimator<T, S> *paramEstimator, ResidentData<T> &data,
                                                 const std::vector<int> &groups, size_t nGroups, size_t maxRounds,
                                                 std::vector<int> &labels, std::vector<bool> *converged = NULL) {
    lsqr_model_cfg cfg;
    groupedArgs(models.size(), paramEstimator, data, groups, nGroups);
    const size_t n = nGroups, N = data.size();
    labels.assign(N, -1);
    std::vector<size_t> rounds(n, 0);
    if (converged) converged->assign(n, false);
    if (n == 0 || N == 0) return rounds;
    if (!paramEstimator->deviceModel(cfg) || forceHostLoop() || !assignOnDevice(cfg, true)) {
      std::vector<std::vector<T> > sets;
      std::vector<std::vector<size_t> > index;
      gatherGroups(data, groups, n, sets, index);
      for (size_t g = 0; g < n; g++) {
        std::vector<int> lab;
        bool conv = false;
        rounds[g] = refineModels(models[g], paramEstimator, sets[g], maxRounds, lab, &conv);
        if (converged) (*converged)[g] = conv;
        for (size_t q = 0; q < lab.size(); q++) labels[index[g][q]] = lab[q];
      }
      return rounds;
    }
    return refineGroupedOnDevice(lsqr_refine_grouped, cfg, models, data, groups, n, maxRounds, labels, rounds,
                                 converged);
  }

  // refineModelsGrouped for the sphere estimator with the geometric least-squares fit (its default), on the device: ONE
  // call (lsqr_refine_lm_grouped).  Arguments and return value are refineModelsGrouped's; every group is decided as
  // refineModelsLM decides it on the records of the group alone.  Any other estimator throws std::invalid_argument:
  // refineModelsGrouped takes it.
  static std::vector<size_t> refineModelsLMGrouped(std::vector<std::vector<std::vector<S> > > &models,
                                                   ParametersEstimator<T, S> *paramEstimator, ResidentData<T> &data,
                                                   const std::vector<int> &groups, size_t nGroups, size_t maxRounds,
                                                   std::vector<int> &labels, std::vector<bool> *converged = NULL) {
    lsqr_model_cfg cfg;
    groupedArgs(models.size(), paramEstimator, data, groups, nGroups);
    if (!paramEstimator->deviceModel(cfg) || cfg.model != LSQR_MODEL_SPHERE || cfg.ls_type != LSQR_LS_GEOMETRIC)
      throw std::invalid_argument("lsqrRecipes::RANSAC: refineModelsLMGrouped takes the geometric sphere only");
    const size_t n = nGroups, N = data.size();
    labels.assign(N, -1);
    std::vector<size_t> rounds(n, 0);
    if (converged) converged->assign(n, false);
    if (n == 0 || N == 0) return rounds;
    return refineGroupedOnDevice(lsqr_refine_lm_grouped, cfg, models, data, groups, n, maxRounds, labels, rounds,
                                 converged);
  }

  // assignToModelsGrouped / refineModelsGrouped for DenseLinearEquationSystemParametersEstimator<double,n>, which
  // those two send to the host loop: ONE device call each for all groups (lsqr_assign_dense_grouped /
  // lsqr_refine_dense_grouped), on the rows where they already are.  Arguments and what comes back are
  // assignToModelsGrouped's / refineModelsGrouped's; every group is decided as assignToModelsDense / refineModelsDense
  // decide it on the rows of the group alone.  Any other estimator throws std::invalid_argument.
  static void assignToModelsDenseGrouped(const std::vector<std::vector<std::vector<S> > > &models,
                                         ParametersEstimator<T, S> *paramEstimator, ResidentData<T> &data,
                                         const std::vector<int> &groups, size_t nGroups, std::vector<int> &labels) {
    lsqr_model_cfg cfg;
    groupedArgs(models.size(), paramEstimator, data, groups, nGroups);
    denseOnly(paramEstimator, cfg, "assignToModelsDenseGrouped");
    const size_t n = nGroups, N = data.size();
    labels.assign(N, -1);
    if (n == 0 || N == 0) return;
    size_t maxModels = 0;
    std::vector<size_t> nModels;
    std::vector<double> par = packGroupedModels(models, cfg, maxModels, nModels);
    if (maxModels == 0) return;
    std::vector<int32_t> glab(groups.begin(), groups.end()), lab(N);
    lsqr_ctx *ctx = data.attach(cfg);
    data.check(lsqr_assign_dense_grouped(ctx, &glab[0], n, 0, &par[0], &nModels[0], maxModels, &lab[0], NULL, NULL,
                                         NULL));
    labels.assign(lab.begin(), lab.end());
  }

  static std::vector<size_t> refineModelsDenseGrouped(std::vector<std::vector<std::vector<S> > > &models,
                                                      ParametersEstimator<T, S> *paramEstimator,
                                                      ResidentData<T> &data, const std::vector<int> &groups,
                                                      size_t nGroups, size_t maxRounds, std::vector<int> &labels,
                                                      std::vector<bool> *converged = NULL) {
    lsqr_model_cfg cfg;
    groupedArgs(models.size(), paramEstimator, data, groups, nGroups);
    denseOnly(paramEstimator, cfg, "refineModelsDenseGrouped");
    const size_t n = nGroups, N = data.size();
    labels.assign(N, -1);
    std::vector<size_t> rounds(n, 0);
    if (converged) converged->assign(n, false);
    if (n == 0 || N == 0) return rounds;
    return refineGroupedOnDevice(lsqr_refine_dense_grouped, cfg, models, data, groups, n, maxRounds, labels, rounds,
                                 converged);
  }

  // Sequential RANSAC over many independent problems (not in the reference): problem j is data[j], and
  // computeManySequential(...)[j], parameters[j] and (*labels)[j] equal what computeSequential returns / leaves on
  // data[j] after seed(seed() + j * maxModels) -- round r of problem j walks sampler stream seed() + j * maxModels + r.
  // Per problem as computeSequential: invalid input (too few records, p outside (0, 1)) or maxModels == 0 runs
  // nothing and leaves both empty, the labels -1.
  // The models computeMany batches (plane, line, both sphere fits, the dense linear system up to 17 unknowns, absolute
  // orientation, pivot calibration, ray intersection, 2-D line) run in ONE device call
  // (lsqr_ransac_many_sequential: one upload, every round one batched search over the problems still going, the
  // survivors compacted on the device); estimators without a device model, the other device estimators and
  // forceHostLoop() loop over computeSequential with the same seeds.  Under LSQR_DEVICES the batched call runs on the
  // first listed device's context.  lastInfo() is not updated by the batched call.
  static std::vector<std::vector<double> > computeManySequential(
      std::vector<std::vector<std::vector<S> > > &parameters, ParametersEstimator<T, S> *paramEstimator,
      const std::vector<std::vector<T> > &data, double desiredProbabilityForNoOutliers, size_t maxModels,
      size_t minVotes, std::vector<std::vector<int> > *labels = NULL) {
    if (!paramEstimator) throw std::invalid_argument("lsqrRecipes::RANSAC: null estimator");
    const size_t n = data.size();
    const double p = desiredProbabilityForNoOutliers;
    parameters.resize(n);
    if (labels) labels->resize(n);
    std::vector<std::vector<double> > fraction(n);
    for (size_t j = 0; j < n; j++) {
      parameters[j].clear();
      if (labels) (*labels)[j].assign(data[j].size(), -1);
    }
    if (n == 0 || maxModels == 0 || p >= 1.0 || p <= 0.0) return fraction;
    lsqr_model_cfg cfg;
    const bool device = paramEstimator->deviceModel(cfg) && !forceHostLoop();
    const bool batched =
        device && lsqr_record_doubles(&cfg) <= 18 &&
        (cfg.model == LSQR_MODEL_PLANE || cfg.model == LSQR_MODEL_LINE || cfg.model == LSQR_MODEL_SPHERE ||
         cfg.model == LSQR_MODEL_DENSE || cfg.model == LSQR_MODEL_ABSOR || cfg.model == LSQR_MODEL_PIVOT ||
         cfg.model == LSQR_MODEL_RAY || cfg.model == LSQR_MODEL_LINE2D);
    if (!batched) {
      const uint64_t s0 = seed();
      for (size_t j = 0; j < n; j++) {
        seed() = s0 + j * maxModels;
        // (computeSequential reads the records only; it takes them by non-const reference as compute() does)
        fraction[j] = computeSequential(parameters[j], paramEstimator, const_cast<std::vector<T> &>(data[j]), p,
                                        maxModels, minVotes, labels ? &(*labels)[j] : NULL);
      }
      seed() = s0;
      return fraction;
    }
    std::vector<uint64_t> offsets(n + 1, 0), seeds(n * maxModels);
    for (size_t j = 0; j < n; j++) offsets[j + 1] = offsets[j] + data[j].size();
    for (size_t e = 0; e < n * maxModels; e++) seeds[e] = seed() + e;
    std::vector<T> records;
    records.reserve((size_t)offsets[n]);
    for (size_t j = 0; j < n; j++) records.insert(records.end(), data[j].begin(), data[j].end());
    detail::Device &d = detail::Device::instance();
    lsqr_ctx *ctx = d.ctx();
    if (lsqr_multi *m = d.multi()) ctx = lsqr_multi_ctx(m, 0);
    d.check(lsqr_set_model(ctx, &cfg));
    const int P = lsqr_num_params(&cfg);
    std::vector<double> par(n * maxModels * (size_t)P);
    std::vector<int32_t> lab(labels ? (size_t)offsets[n] : 0), status(n * maxModels);
    std::vector<lsqr_ransac_info> info(n * maxModels);
    std::vector<size_t> nModels(n, 0);
    d.check(lsqr_ransac_many_sequential(ctx, records.empty() ? NULL : &records[0], sizeof(T), &offsets[0], n, p,
                                        &seeds[0], maxModels, minVotes, &par[0], lab.empty() ? NULL : &lab[0],
                                        &info[0], &status[0], &nModels[0]));
    for (size_t j = 0; j < n; j++) {
      for (size_t r = 0; r < maxModels && status[j * maxModels + r] != LSQR_ERR_STATE; r++) {  // the rounds that ran
        const size_t e = j * maxModels + r;
        fraction[j].push_back(info[e].fraction);
        if (r < nModels[j]) parameters[j].push_back(std::vector<S>(&par[e * P], &par[e * P] + info[e].n_params));
      }
      if (labels && !lab.empty())
        (*labels)[j].assign(lab.begin() + (std::ptrdiff_t)offsets[j], lab.begin() + (std::ptrdiff_t)offsets[j + 1]);
    }
    return fraction;
  }

  // Grouped sequential RANSAC on resident records (not in the reference): several models per label.  Group g is the
  // records i of `data` with groups[i] == g, in their order; a label that is negative or >= nGroups puts the record in
  // no group.  Round r of group g walks sampler stream seed() + g * maxModels + r, so computeGroupedSequential(...)[g]
  // and parameters[g] equal what computeManySequential returns / leaves for the per-group vectors, and labels
  // (optional, one entry per record of `data`: the round that claimed the record inside its group, else -1) hold its
  // per-group labels at the records' own places.  Invalid p or maxModels == 0 runs nothing, as there.
  // The estimators computeManySequential batches run in ONE device call (lsqr_ransac_grouped_sequential: the records
  // are grouped on the device, where they already are; only the group labels go up and the round labels come down).
  // The others, and forceHostLoop(), go through computeManySequential itself on the per-group vectors, gathered from
  // the vector `data` was made from.  THAT VECTOR MUST THEN STILL BE ALIVE AND UNCHANGED: ResidentData keeps a pointer
  // to it, not a copy (see computeGrouped).
  static std::vector<std::vector<double> > computeGroupedSequential(
      std::vector<std::vector<std::vector<S> > > &parameters, ParametersEstimator<T, S> *paramEstimator,
      ResidentData<T> &data, const std::vector<int> &groups, size_t nGroups, double desiredProbabilityForNoOutliers,
      size_t maxModels, size_t minVotes, std::vector<int> *labels = NULL) {
    if (!paramEstimator) throw std::invalid_argument("lsqrRecipes::RANSAC: null estimator");
    if (groups.size() != data.size()) throw std::invalid_argument("lsqrRecipes::RANSAC: one group label per record");
    const size_t n = nGroups, N = data.size();
    const double p = desiredProbabilityForNoOutliers;
    parameters.resize(n);
    for (size_t g = 0; g < n; g++) parameters[g].clear();
    if (labels) labels->assign(N, -1);
    std::vector<std::vector<double> > fraction(n);
    if (n == 0 || N == 0 || maxModels == 0 || p >= 1.0 || p <= 0.0) return fraction;
    lsqr_model_cfg cfg;
    const bool device = paramEstimator->deviceModel(cfg) && !forceHostLoop();
    const bool batched =
        device && lsqr_record_doubles(&cfg) <= 18 &&
        (cfg.model == LSQR_MODEL_PLANE || cfg.model == LSQR_MODEL_LINE || cfg.model == LSQR_MODEL_SPHERE ||
         cfg.model == LSQR_MODEL_DENSE || cfg.model == LSQR_MODEL_ABSOR || cfg.model == LSQR_MODEL_PIVOT ||
         cfg.model == LSQR_MODEL_RAY || cfg.model == LSQR_MODEL_LINE2D);
    if (!batched) {
      const T *host = data.hostRecords();
      std::vector<std::vector<T> > sets(n);
      std::vector<std::vector<size_t> > index(n);
      for (size_t i = 0; i < N; i++)
        if (groups[i] >= 0 && (size_t)groups[i] < n) {
          sets[(size_t)groups[i]].push_back(host[i]);
          index[(size_t)groups[i]].push_back(i);
        }
      std::vector<std::vector<int> > lab;
      fraction = computeManySequential(parameters, paramEstimator, sets, p, maxModels, minVotes, labels ? &lab : NULL);
      if (labels)
        for (size_t g = 0; g < n; g++)
          for (size_t q = 0; q < lab[g].size(); q++) (*labels)[index[g][q]] = lab[g][q];
      return fraction;
    }
    std::vector<uint64_t> seeds(n * maxModels);
    for (size_t e = 0; e < n * maxModels; e++) seeds[e] = seed() + e;
    std::vector<int32_t> glab(groups.begin(), groups.end());
    lsqr_ctx *ctx = data.attach(cfg);
    const int P = lsqr_num_params(&cfg);
    std::vector<double> par(n * maxModels * (size_t)P);
    std::vector<int32_t> lab(labels ? N : 0), status(n * maxModels);
    std::vector<lsqr_ransac_info> info(n * maxModels);
    std::vector<size_t> nModels(n, 0);
    data.check(lsqr_ransac_grouped_sequential(ctx, &glab[0], n, 0, p, &seeds[0], maxModels, minVotes, &par[0],
                                              lab.empty() ? NULL : &lab[0], NULL, &info[0], &status[0], &nModels[0]));
    for (size_t g = 0; g < n; g++)
      for (size_t r = 0; r < maxModels && status[g * maxModels + r] != LSQR_ERR_STATE; r++) {  // the rounds that ran
        const size_t e = g * maxModels + r;
        fraction[g].push_back(info[e].fraction);
        if (r < nModels[g]) parameters[g].push_back(std::vector<S>(&par[e * P], &par[e * P] + info[e].n_params));
      }
    if (labels) labels->assign(lab.begin(), lab.end());
    return fraction;
  }

  // sampler stream of the probabilistic overload (default 1); set it to vary the hypotheses
  static uint64_t &seed() {
    static thread_local uint64_t s = 1;
    return s;
  }
  // diagnostics of the last compute() on this thread (iterations, hypotheses scanned, LM info)
  static lsqr_ransac_info &lastInfo() {
    static thread_local lsqr_ransac_info i;
    return i;
  }

 // route an estimator that HAS a device model through the plugin loop as well (tests: both paths must
  // agree on iterations, winner and consensus set); default false
  static bool &forceHostLoop() {
    static thread_local bool f = false;
    return f;
  }

 private:
  // ---- plugin path: estimators without a device model -------------------------------------------------
  // One hypothesis of the serial loop (RANSAC.hxx:84-99): exact fit of the subset, then the agree() pass
  // with the reference's early exit -- a hypothesis that can no longer overtake the best one is
  // abandoned, which never changes the winner (its final count would stay below the best).
  static bool tryHypothesis(ParametersEstimator<T, S> *est, std::vector<T> &data,
                            const std::vector<uint32_t> &subset, uint64_t bestVotes,
                            std::vector<S> &model, std::vector<char> &agrees, uint32_t &votes,
                            bool earlyExit) {
    std::vector<T *> minimal(subset.size());
    for (size_t l = 0; l < subset.size(); l++) minimal[l] = &data[subset[l]];  // draw order, RANSAC.hxx:65
    est->estimate(minimal, model);
    votes = 0;
    if (model.empty()) return false;  // degenerate subset, RANSAC.hxx:87-88
    const long long N = (long long)data.size();
    std::fill(agrees.begin(), agrees.end(), 0);
    for (long long m = 0; m < N; m++) {
      if (earlyExit && (long long)bestVotes - (long long)votes >= N - m + 1) break;  // RANSAC.hxx:94
      if (est->agree(model, data[(size_t)m])) {
        agrees[(size_t)m] = 1;
        votes++;
      }
    }
    return true;
  }

  static double pluginFinish(std::vector<S> &parameters, ParametersEstimator<T, S> *est,
                             std::vector<T> &data, const std::vector<char> &best, uint64_t bestVotes,
                             uint64_t iterations, uint64_t bestIndex, std::vector<bool> *consensusSet) {
    lsqr_ransac_info &info = lastInfo();
    info = lsqr_ransac_info();
    info.iterations = iterations;
    info.evaluated = iterations;
    info.best_index = bestIndex;
    info.best_votes = (uint32_t)bestVotes;
    info.fraction = (double)bestVotes / (double)data.size();
    if (bestVotes > 0) {  // RANSAC.hxx:129-139
      std::vector<T *> inliers;
      inliers.reserve((size_t)bestVotes);
      for (size_t m = 0; m < data.size(); m++)
        if (best[m]) inliers.push_back(&data[m]);
      if (consensusSet) consensusSet->assign(best.begin(), best.end());
      est->leastSquaresEstimate(inliers, parameters);
      info.n_params = (int32_t)parameters.size();
      info.fit.n_params = info.n_params;
      info.fit.n_used = bestVotes;
    }
    return info.fraction;
  }

  static double pluginCompute(std::vector<S> &parameters, ParametersEstimator<T, S> *est,
                              std::vector<T> &data, double p, std::vector<bool> *consensusSet) {
    const size_t N = data.size();
    const int k = (int)est->numForEstimate();
    parameters.clear();  // RANSAC.hxx:43
    uint64_t st[6];      // {i, numTries, best votes, best index, has best, done}: lsqr_replay's state
    lsqr_replay_init(N, k, p, st);
    std::set<std::vector<uint32_t> > drawn;  // sorted index tuples already tried, RANSAC.hxx:33-34,79
    std::vector<uint32_t> subset((size_t)k), key((size_t)k);
    std::vector<S> model;
    std::vector<char> cur(N, 0), best(N, 0);
    for (uint64_t it = 0; !st[5]; it++) {
      if (lsqr_sample_subsets(seed(), it, 1, N, k, &subset[0]) != LSQR_OK)
        throw std::runtime_error("lsqrRecipes::RANSAC: subset sampler failed");
      key = subset;
      std::sort(key.begin(), key.end());
      uint8_t valid = 0;
      uint32_t votes = 0;
      if (drawn.insert(key).second)  // a repeated subset still consumes the iteration, RANSAC.hxx:114-116
        valid = tryHypothesis(est, data, subset, st[2], model, cur, votes, true) ? 1 : 0;
      const uint64_t hadBest = st[4], bestBefore = st[3];
      // strict '>' update and the adaptive bound on numTries (RANSAC.hxx:100-111), shared with the device path
      if (lsqr_replay(N, k, p, &subset[0], &valid, &votes, 1, it, NULL, st) == 0) break;
      if (st[4] && (!hadBest || st[3] != bestBefore)) best.swap(cur);
    }
    return pluginFinish(parameters, est, data, best, st[4] ? st[2] : 0, st[0], st[3], consensusSet);
  }

  // exhaustive overload (RANSAC.hxx:150-249): every k-subset in lexicographic order, full agree() passes,
  // first maximum wins
  static double pluginComputeExhaustive(std::vector<S> &parameters, ParametersEstimator<T, S> *est,
                                        std::vector<T> &data, std::vector<bool> *consensusSet) {
    const size_t N = data.size();
    const int k = (int)est->numForEstimate();
    std::vector<uint32_t> subset((size_t)k);
    for (int l = 0; l < k; l++) subset[(size_t)l] = (uint32_t)l;
    std::vector<S> model;
    std::vector<char> cur(N, 0), best(N, 0);
    uint64_t bestVotes = 0, bestIndex = 0, index = 0;
    if (k == 0) return pluginFinish(parameters, est, data, best, 0, 0, 0, consensusSet);
    for (bool more = true; more; index++) {
      uint32_t votes = 0;
      if (tryHypothesis(est, data, subset, bestVotes, model, cur, votes, false) && votes > bestVotes) {
        bestVotes = votes;  // RANSAC.hxx:245 strict
        bestIndex = index;
        best.swap(cur);
      }
      int l = k - 1;  // next combination
      while (l >= 0 && subset[(size_t)l] == (uint32_t)(N - (size_t)k + (size_t)l)) l--;
      if (l < 0) more = false;
      else {
        subset[(size_t)l]++;
        for (int j = l + 1; j < k; j++) subset[(size_t)j] = subset[(size_t)j - 1] + 1;
      }
    }
    return pluginFinish(parameters, est, data, best, bestVotes, index, bestIndex, consensusSet);
  }

  // one lsqr_ransac_sequential call on a context that holds the records; `chk` turns a failure status into its throw
  template <class Checker>
  static std::vector<double> sequentialOn(Checker &chk, lsqr_ctx *ctx, const lsqr_model_cfg &cfg, size_t N,
                                          std::vector<std::vector<S> > &parameters, double p, size_t maxModels,
                                          size_t minVotes, std::vector<int> *labels) {
    const int P = lsqr_num_params(&cfg);
    std::vector<uint64_t> seeds(maxModels);
    for (size_t r = 0; r < maxModels; r++) seeds[r] = seed() + r;
    std::vector<double> par(maxModels * (size_t)P);
    std::vector<int32_t> lab(labels ? N : 0), status(maxModels);
    std::vector<lsqr_ransac_info> info(maxModels);
    size_t nModels = 0;
    chk.check(lsqr_ransac_sequential(ctx, p, &seeds[0], maxModels, minVotes, &par[0], labels ? &lab[0] : NULL,
                                     &info[0], &status[0], &nModels));
    std::vector<double> fraction;
    for (size_t r = 0; r < maxModels && status[r] != LSQR_ERR_STATE; r++) {  // the rounds that ran
      fraction.push_back(info[r].fraction);
      lastInfo() = info[r];
      if (r < nModels) parameters.push_back(std::vector<S>(&par[r * P], &par[r * P] + info[r].n_params));
    }
    if (labels) labels->assign(lab.begin(), lab.end());
    return fraction;
  }

  // the host loop of computeSequential: pluginCompute on the records that are left, the consensus set erased
  static std::vector<double> pluginComputeSequential(std::vector<std::vector<S> > &parameters,
                                                     ParametersEstimator<T, S> *est, std::vector<T> &data, double p,
                                                     size_t maxModels, size_t minVotes, std::vector<int> *labels) {
    std::vector<T> cur(data);
    std::vector<size_t> orig(data.size());
    for (size_t i = 0; i < orig.size(); i++) orig[i] = i;
    std::vector<double> fraction;
    const uint64_t s0 = seed();
    for (size_t r = 0; r < maxModels && cur.size() >= est->numForEstimate(); r++) {
      std::vector<S> model;
      std::vector<bool> cons;
      seed() = s0 + r;
      fraction.push_back(pluginCompute(model, est, cur, p, &cons));
      seed() = s0;
      const uint64_t votes = lastInfo().best_votes;
      if (model.empty() || votes < std::max<uint64_t>(minVotes, 1)) break;  // rejected: claims nothing
      parameters.push_back(model);
      size_t w = 0;
      for (size_t i = 0; i < cur.size(); i++) {
        if (cons[i]) {
          if (labels) (*labels)[orig[i]] = (int)r;
        } else {
          if (w != i) cur[w] = cur[i];  // (guarded: no self-assignment of a record)
          orig[w++] = orig[i];
        }
      }
      cur.erase(cur.begin() + (std::ptrdiff_t)w, cur.end());  // (T need not be default-constructible)
      orig.resize(w);
    }
    return fraction;
  }

  // ---- assignToModels / refineModels -------------------------------------------------------------------------
  // the device models lsqr_assign (refit: lsqr_refine) takes
  static bool assignOnDevice(const lsqr_model_cfg &cfg, bool refit) {
    if (cfg.model == LSQR_MODEL_SPHERE) return !refit || cfg.ls_type == LSQR_LS_ALGEBRAIC;
    return cfg.model == LSQR_MODEL_PLANE || cfg.model == LSQR_MODEL_LINE || cfg.model == LSQR_MODEL_LINE2D;
  }

  // assignToModelsDense / refineModelsDense and their grouped forms: the estimator's device model must be the dense
  // linear system
  static void denseOnly(ParametersEstimator<T, S> *paramEstimator, lsqr_model_cfg &cfg, const char *fn) {
    if (!paramEstimator) throw std::invalid_argument("lsqrRecipes::RANSAC: null estimator");
    if (!paramEstimator->deviceModel(cfg) || cfg.model != LSQR_MODEL_DENSE)
      throw std::invalid_argument(std::string("lsqrRecipes::RANSAC: ") + fn + " takes the dense linear system only");
  }

  // assignToModelsRigid / refineModelsRigid: the estimator's device model must be absolute orientation, pivot
  // calibration or ray intersection
  static void rigidOnly(ParametersEstimator<T, S> *paramEstimator, lsqr_model_cfg &cfg, const char *fn) {
    if (!paramEstimator) throw std::invalid_argument("lsqrRecipes::RANSAC: null estimator");
    if (!paramEstimator->deviceModel(cfg) ||
        !(cfg.model == LSQR_MODEL_ABSOR || cfg.model == LSQR_MODEL_PIVOT || cfg.model == LSQR_MODEL_RAY))
      throw std::invalid_argument(std::string("lsqrRecipes::RANSAC: ") + fn +
                                  " takes absolute orientation, pivot calibration and ray intersection only");
  }

  // the device path of refineModels (lsqr_refine), refineModelsLM (lsqr_refine_lm), refineModelsDense and the rigid
  // pair (lsqr_refine_rigid)
  typedef int (*RefineCall)(lsqr_ctx *, double *, size_t, size_t, int, int32_t *, uint64_t *, lsqr_fit_info *,
                            int32_t *, size_t *, int *);
  static size_t refineOnDevice(RefineCall call, lsqr_model_cfg &cfg, std::vector<std::vector<S> > &models,
                               std::vector<T> &data, size_t maxRounds, std::vector<int> &labels, bool *converged) {
    detail::Device &d = detail::Device::instance();
    lsqr_ctx *ctx = d.ctx();
    if (lsqr_multi *m = d.multi()) ctx = lsqr_multi_ctx(m, 0);
    d.check(lsqr_set_model(ctx, &cfg));
    d.check(lsqr_upload(ctx, &data[0], data.size(), sizeof(T)));
    const size_t M = models.size(), P = (size_t)lsqr_num_params(&cfg);
    std::vector<double> par = packModels(models, cfg);
    std::vector<int32_t> lab(data.size()), status(M);
    std::vector<lsqr_fit_info> fits(M);
    size_t rounds = 0;
    int conv = 0;
    d.check(call(ctx, &par[0], M, maxRounds, 0, &lab[0], NULL, &fits[0], &status[0], &rounds, &conv));
    for (size_t m = 0; m < M; m++) models[m].assign(&par[m * P], &par[m * P] + P);
    labels.assign(lab.begin(), lab.end());
    if (converged) *converged = conv != 0;
    return rounds;
  }

  // the models as rows of lsqr_num_params doubles
  static std::vector<double> packModels(const std::vector<std::vector<S> > &models, const lsqr_model_cfg &cfg) {
    const size_t P = (size_t)lsqr_num_params(&cfg);
    if (models.size() > 64) throw std::invalid_argument("lsqrRecipes::RANSAC: more than 64 models");
    std::vector<double> par(models.size() * P);
    for (size_t m = 0; m < models.size(); m++) {
      if (models[m].size() != P) throw std::invalid_argument("lsqrRecipes::RANSAC: model vector of the wrong length");
      for (size_t j = 0; j < P; j++) par[m * P + j] = (double)models[m][j];
    }
    return par;
  }

  // ---- assignToModelsGrouped / refineModelsGrouped ---------------------------------------------------------------
  static void groupedArgs(size_t nSets, ParametersEstimator<T, S> *paramEstimator, ResidentData<T> &data,
                          const std::vector<int> &groups, size_t nGroups) {
    if (!paramEstimator) throw std::invalid_argument("lsqrRecipes::RANSAC: null estimator");
    if (groups.size() != data.size()) throw std::invalid_argument("lsqrRecipes::RANSAC: one group label per record");
    if (nSets != nGroups) throw std::invalid_argument("lsqrRecipes::RANSAC: one model set per group");
  }

  // the device path of refineModelsGrouped (lsqr_refine_grouped), refineModelsLMGrouped (lsqr_refine_lm_grouped) and
  // refineModelsDenseGrouped (lsqr_refine_dense_grouped); labels, rounds and *converged hold the answer for "nothing
  // ran"
  typedef int (*RefineGroupedCall)(lsqr_ctx *, const int32_t *, size_t, int, double *, const size_t *, size_t, size_t,
                                   int32_t *, uint64_t *, uint64_t *, lsqr_fit_info *, int32_t *, size_t *, int32_t *);
  static std::vector<size_t> refineGroupedOnDevice(RefineGroupedCall call, lsqr_model_cfg &cfg,
                                                   std::vector<std::vector<std::vector<S> > > &models,
                                                   ResidentData<T> &data, const std::vector<int> &groups, size_t n,
                                                   size_t maxRounds, std::vector<int> &labels,
                                                   std::vector<size_t> &rounds, std::vector<bool> *converged) {
    const size_t N = data.size();
    size_t maxModels = 0;
    std::vector<size_t> nModels;
    std::vector<double> par = packGroupedModels(models, cfg, maxModels, nModels);
    if (maxModels == 0) return rounds;
    const size_t P = (size_t)lsqr_num_params(&cfg);
    std::vector<int32_t> glab(groups.begin(), groups.end()), lab(N), status(n * maxModels), conv(n, 0);
    std::vector<lsqr_fit_info> fits(n * maxModels);
    lsqr_ctx *ctx = data.attach(cfg);
    data.check(call(ctx, &glab[0], n, 0, &par[0], &nModels[0], maxModels, maxRounds, &lab[0], NULL, NULL, &fits[0],
                    &status[0], &rounds[0], &conv[0]));
    for (size_t g = 0; g < n; g++) {
      for (size_t m = 0; m < nModels[g]; m++) {
        const double *row = &par[(g * maxModels + m) * P];
        models[g][m].assign(row, row + P);
      }
      if (converged) (*converged)[g] = conv[g] != 0;
    }
    labels.assign(lab.begin(), lab.end());
    return rounds;
  }

  // the per-group vectors of the host loops (as computeGroupedSequential gathers them), and every record's own place
  static void gatherGroups(ResidentData<T> &data, const std::vector<int> &groups, size_t n,
                           std::vector<std::vector<T> > &sets, std::vector<std::vector<size_t> > &index) {
    const T *host = data.hostRecords();
    sets.assign(n, std::vector<T>());
    index.assign(n, std::vector<size_t>());
    for (size_t i = 0; i < data.size(); i++)
      if (groups[i] >= 0 && (size_t)groups[i] < n) {
        sets[(size_t)groups[i]].push_back(host[i]);
        index[(size_t)groups[i]].push_back(i);
      }
  }

  // the model sets as lsqr_assign_grouped's rows: row g * maxModels + m is models[g][m]; maxModels: the largest set
  static std::vector<double> packGroupedModels(const std::vector<std::vector<std::vector<S> > > &models,
                                               const lsqr_model_cfg &cfg, size_t &maxModels,
                                               std::vector<size_t> &nModels) {
    const size_t P = (size_t)lsqr_num_params(&cfg), n = models.size();
    nModels.assign(n, 0);
    maxModels = 0;
    for (size_t g = 0; g < n; g++) {
      nModels[g] = models[g].size();
      if (nModels[g] > maxModels) maxModels = nModels[g];
    }
    if (maxModels > 64) throw std::invalid_argument("lsqrRecipes::RANSAC: more than 64 models");
    std::vector<double> par(n * maxModels * P + 1, 0.0);  // (+ 1: never empty)
    for (size_t g = 0; g < n; g++)
      for (size_t m = 0; m < nModels[g]; m++) {
        if (models[g][m].size() != P) throw std::invalid_argument("lsqrRecipes::RANSAC: model vector of the wrong length");
        for (size_t j = 0; j < P; j++) par[(g * maxModels + m) * P + j] = (double)models[g][m][j];
      }
    return par;
  }

  // the host loop of assignToModels: the first model whose agree() holds
  static void pluginAssign(const std::vector<std::vector<S> > &models, ParametersEstimator<T, S> *est,
                           std::vector<T> &data, std::vector<int> &labels) {
    std::vector<std::vector<S> > rows(models);  // (agree() takes its parameters by non-const reference)
    for (size_t i = 0; i < data.size(); i++) {
      labels[i] = -1;
      for (size_t m = 0; m < rows.size() && labels[i] < 0; m++)
        if (!rows[m].empty() && est->agree(rows[m], data[i])) labels[i] = (int)m;
    }
  }

  // the host loop of refineModels
  static size_t pluginRefine(std::vector<std::vector<S> > &models, ParametersEstimator<T, S> *est,
                             std::vector<T> &data, size_t maxRounds, std::vector<int> &labels, bool *converged) {
    std::vector<int> prev;
    size_t r = 0;
    for (;;) {
      pluginAssign(models, est, data, labels);
      if (r > 0 && labels == prev) {
        if (converged) *converged = true;
        break;
      }
      if (r == maxRounds) break;
      for (size_t m = 0; m < models.size(); m++) {
        std::vector<T *> own;
        for (size_t i = 0; i < data.size(); i++)
          if (labels[i] == (int)m) own.push_back(&data[i]);
        if (own.size() < est->numForEstimate()) continue;
        std::vector<S> fit;
        est->leastSquaresEstimate(own, fit);
        if (!fit.empty()) models[m] = fit;
      }
      prev = labels;
      r++;
    }
    return r;
  }

  static double finish(bool ok, const lsqr_ransac_info &info, const std::vector<double> &p,
                       const std::vector<uint8_t> &cons, std::vector<S> &parameters,
                       std::vector<bool> *consensusSet) {
    if (info.best_votes > 0 && consensusSet) {  // RANSAC.hxx:129-137: only when a set was found
      consensusSet->clear();
      consensusSet->insert(consensusSet->begin(), cons.begin(), cons.end());
    }
    if (ok) parameters.assign(p.begin(), p.begin() + info.n_params);
    return info.fraction;
  }
};

}  // namespace lsqrRecipes
#endif
