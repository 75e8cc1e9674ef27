/*
 * lsqr_hip.h -- C ABI of the MI355X-native RANSAC + least-squares hot path
 * (liblsqr_hip.so, built from lsqrrecipes_amd/csrc/ with hipcc --offload-arch=gfx950).
 *
 * This is the drop-in boundary for the one hot path of zivy/LSQRRecipes:
 *     RANSAC<T,S>::compute()                      parametersEstimators/RANSAC.h:75-79,111-113
 *       -> ParametersEstimator<T,S>::estimate()   parametersEstimators/ParametersEstimator.h:41-43
 *       -> ParametersEstimator<T,S>::agree()      parametersEstimators/ParametersEstimator.h:55
 *       -> ...::leastSquaresEstimate()            parametersEstimators/ParametersEstimator.h:51-53
 * for the Plane / Sphere / Line / DenseLinearEquationSystem / SinglePointTargetUSCalibration
 * estimators (and AbsoluteOrientation / PivotCalibration).  Plain C types only: no STL, no exceptions, no torch types cross this ABI.  Every
 * entry point returns an lsqr_status; LSQR_OK == 0.  The reference's "empty parameters vector"
 * failure convention (RANSAC.h:54-63) maps to LSQR_EMPTY (a normal outcome, not an error).
 *
 * The C++ header shim (lsqrrecipes_amd/include/RANSAC.h, ...Estimator.h) and the Python mirror
 * (lsqrrecipes_amd/ python modules) are thin callers of exactly these functions.  There is no CPU
 * fallback behind this ABI: without a usable HIP device lsqr_ctx_create fails with
 * LSQR_ERR_NO_DEVICE.
 *
 * All records are fp64, array-of-structures, exactly as the reference lays them out:
 *   Point<double,d>            d doubles                         common/Point.h:127
 *   AugmentedRow<double,n>     n+1 doubles (aValues[n], bValue)  .../DenseLinear...Estimator.h:133-134
 *   SingleUnknown DataType     15 slots = Frame{rotation[3][3], translation[3], int outputFormat
 *                              (+4 B pad)} + Point2D             .../SinglePointTarget...h:45-48,
 *                                                                common/Frame.h:30-31,41
 *   CalibratedPointer DataType 18 slots (+ Point3D p)            .../SinglePointTarget...h:335-339
 *   pair<Point3D,Point3D>      6 doubles (first, second)         .../AbsoluteOrientation...h:14-15
 *                              (ls_type 2 = weightedLeastSquaresEstimate, .h:86: 7 doubles, slot 6 = weight)
 *   Frame                      13 slots (104 B)                  common/Frame.h:30-31,41
 *   Ray3D                      6 doubles (Point3D p, Vector3D n) common/Ray3D.h:23-24
 * A caller's std::vector<T> is passed as (pointer, count, stride in bytes) without repacking.
 */
#ifndef LSQR_HIP_H
#define LSQR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define LSQR_API __attribute__((visibility("default")))
#else
#define LSQR_API
#endif

typedef enum {
  LSQR_OK = 0,
  LSQR_EMPTY = 1,          /* reference's empty-vector outcome: degenerate data / LS failed */
  LSQR_ERR_INVALID = 2,    /* bad argument */
  LSQR_ERR_NO_DEVICE = 3,  /* no HIP device / runtime unusable */
  LSQR_ERR_HIP = 4,        /* a HIP call failed; see lsqr_last_error */
  LSQR_ERR_STATE = 5       /* call order (no data uploaded, no hypotheses, ...) */
} lsqr_status;

typedef enum {
  LSQR_MODEL_PLANE = 1,      /* PlaneParametersEstimator<dim>       params [n(dim), a(dim)]   */
  LSQR_MODEL_SPHERE = 2,     /* SphereParametersEstimator<dim>      params [c(dim), r]        */
  LSQR_MODEL_LINE = 3,       /* LineParametersEstimator<dim>        params [dir(dim), a(dim)] */
  LSQR_MODEL_DENSE = 4,      /* DenseLinearEquationSystemParametersEstimator<double,n>, dim=n */
  LSQR_MODEL_US_SINGLE = 5,  /* SingleUnknownPointTargetUSCalibrationParametersEstimator      */
  LSQR_MODEL_US_POINTER = 6, /* CalibratedPointerTargetUSCalibrationParametersEstimator       */
  LSQR_MODEL_ABSOR = 7,      /* AbsoluteOrientationParametersEstimator  params [s,qx,qy,qz,t(3)] */
  LSQR_MODEL_PIVOT = 8,      /* PivotCalibrationEstimator               params [DRF^t(3), W^t(3)] */
  LSQR_MODEL_RAY = 9,        /* RayIntersectionParametersEstimator      params [x, y, z]          */
  LSQR_MODEL_LINE2D = 10,    /* Line2DParametersEstimator               params [n_x, n_y, a_x, a_y] */
  LSQR_MODEL_PHANTOM = 11    /* PlanePhantomUSCalibrationParametersEstimator  31 frames, 41 params */
} lsqr_model;

/* SphereParametersEstimator::LeastSquaresType (SphereParametersEstimator.h:28) and the US
 * estimators' {ANALYTIC, ITERATIVE} (SinglePointTarget...h:57) */
enum { LSQR_LS_ALGEBRAIC = 0, LSQR_LS_GEOMETRIC = 1, LSQR_LS_ANALYTIC = 0, LSQR_LS_ITERATIVE = 1 };

/* What the reference passes to an estimator's constructor / setters. */
typedef struct {
  int32_t model;   /* lsqr_model */
  int32_t dim;     /* point dimension (plane/sphere/line: 2 or 3), n for DENSE (1..64) */
  double delta;    /* constructor argument, NOT squared (PlaneParametersEstimator.hxx:13-17) */
  int32_t ls_type; /* sphere / US; ABSOR: 2 = records carry a weight in slot 6 (weighted fit) */
  int32_t reserved;
  double aux;      /* RAY: minimalAngularDeviation in radians (RayIntersection...Estimator.h:34-35);
                      unused by the other models */
} lsqr_model_cfg;

typedef struct lsqr_ctx lsqr_ctx; /* owns a device, a stream and all device buffers */

/* Result block of a final fit (leastSquaresEstimate). */
typedef struct {
  int32_t n_params;     /* 0 when status is LSQR_EMPTY */
  int32_t lm_info;      /* MINPACK info code of the LM run (0 when no LM) */
  int32_t lm_nfev;      /* LM function evaluations (= device passes) */
  int32_t reserved;     /* LM runs: the evaluation after which the cost never again fell by more than 1e-7
                           relative (diagnostics: where a run that ends at the evaluation limit stopped gaining).
                           Dense system: 1 = the elimination on the normal equations was refused and the fit was taken
                           from the rows in double-double (the reference's SVD route, csrc/dense.h); 2 = only the summed
                           block was at hand (lsqr_solve_moments, lsqr_step_finish*) and a pivot fell below 1e-6 max|G|:
                           the result carries eps cond(A)^2 -- a caller that holds the rows should fit again from them
                           (lsqr_mask + lsqr_ls_fit; lsqr_multi_* and distributed.ShardedRansac do, so that an N-GPU
                           fit equals the one-GPU fit on ill-conditioned systems too) */
  uint64_t n_used;      /* observations that entered the fit */
  double cost;          /* final sum of squared residuals where the model defines one, else 0 */
} lsqr_fit_info;

/* Outcome of RANSAC<T,S>::compute(). */
typedef struct {
  double fraction;        /* return value: |consensus| / N (RANSAC.hxx:144) */
  uint64_t iterations;    /* loop iterations consumed, duplicates and degenerates included */
  uint64_t evaluated;     /* hypotheses scanned on the device (>= the serial count) */
  uint64_t best_index;    /* iteration index of the winner */
  uint32_t best_votes;
  int32_t n_params;       /* 0 -> parameters empty */
  lsqr_fit_info fit;
} lsqr_ransac_info;

/* ---- library / device -------------------------------------------------------------------- */
LSQR_API const char *lsqr_version(void);
LSQR_API int lsqr_device_count(int *count);
LSQR_API const char *lsqr_status_string(int status);

/* ---- context ------------------------------------------------------------------------------ */
LSQR_API int lsqr_ctx_create(int device, lsqr_ctx **out);
LSQR_API void lsqr_ctx_destroy(lsqr_ctx *ctx);
LSQR_API const char *lsqr_last_error(const lsqr_ctx *ctx);
LSQR_API int lsqr_synchronize(lsqr_ctx *ctx);

/* ---- model description (host only) -------------------------------------------------------- */
LSQR_API int lsqr_min_subset(const lsqr_model_cfg *cfg);     /* numForEstimate() */
LSQR_API int lsqr_num_params(const lsqr_model_cfg *cfg);     /* length of the parameters vector */
LSQR_API int lsqr_record_doubles(const lsqr_model_cfg *cfg); /* tight record size in doubles */
LSQR_API int lsqr_set_model(lsqr_ctx *ctx, const lsqr_model_cfg *cfg);

/* ---- observations -------------------------------------------------------------------------- */
/* Copies `count` host records (std::vector<T>::data(), stride sizeof(T)) to the device.
 * Replaces: the `std::vector<T> &data` argument of RANSAC.h:75-79. */
LSQR_API int lsqr_upload(lsqr_ctx *ctx, const void *host_records, size_t count,
                         size_t stride_bytes);
/* Adopts records already resident in device memory (no copy; caller keeps ownership). */
LSQR_API int lsqr_attach(lsqr_ctx *ctx, const void *device_records, size_t count,
                         size_t stride_bytes);
LSQR_API size_t lsqr_count(const lsqr_ctx *ctx);

/* ---- hypotheses: minimal-subset solve (estimate(), ParametersEstimator.h:41) ---------------- */
/* Explicit subsets: H tuples of k record indices in DRAW order (RANSAC.hxx:65). */
LSQR_API int lsqr_hypotheses_from_subsets(lsqr_ctx *ctx, const uint32_t *subsets, size_t H);
/* Counter-based device sampler: hypothesis i uses stream element first_index + i of `seed`
 * (replaces RANSAC.hxx:51-68; same "rank-th not yet chosen" selection rule, O(k^2) not O(N)).
 * subsets_out (nullable) receives the H*k indices. */
LSQR_API int lsqr_hypotheses_sample(lsqr_ctx *ctx, uint64_t seed, uint64_t first_index, size_t H,
                                    uint32_t *subsets_out);
/* The same sampler stream evaluated on the HOST (no context, no device): subsets_out receives hypotheses
 * [first_index, first_index + H) of stream `seed` for n observations and subsets of k (1..64) indices, draw
 * order.  Used by RANSAC<T,S>::compute() for user-defined estimators without a device model (the plugin path
 * of lsqrrecipes_amd/include/RANSAC.h), so that host and device paths walk one subset stream. */
LSQR_API int lsqr_sample_subsets(uint64_t seed, uint64_t first_index, size_t H, uint64_t n, int k,
                                 uint32_t *subsets_out);
/* ---- single-datum calls, evaluated on the HOST (no context, no device) --------------------------------
 * ParametersEstimator<T,S>::agree(parameters, datum) (ParametersEstimator.h:55; a ten-flop inline in the reference,
 * PlaneParametersEstimator.hxx:196-203) and estimate() of one minimal subset (ParametersEstimator.h:41-43) for the
 * closed-form models: the library's own per-model code (the code the kernels run, compiled for the host; bit-identical
 * results) without an upload and a kernel launch per call.  record(s): the caller's record(s) as laid out for
 * lsqr_upload.  lsqr_estimate_host: `count` >= lsqr_min_subset records in draw order; returns LSQR_EMPTY
 * (*n_params_out = 0) for a degenerate subset.  Both return LSQR_ERR_INVALID when the model has no host form for
 * the call (minimal solves of the dense system, the US calibrations and the plane phantom are device kernels). */
LSQR_API int lsqr_agree_host(const lsqr_model_cfg *cfg, const double *params, const void *record, int *agree_out);
LSQR_API int lsqr_estimate_host(const lsqr_model_cfg *cfg, const void *records, size_t count, size_t stride_bytes,
                                double *params_out, int *n_params_out);
/* The decision of lsqr_assign (below) for ONE record, on the host: params holds n_models rows of lsqr_num_params
 * doubles; *label_out is the model the record goes to, or -1; *residual_out (nullable) its residual to that model,
 * +infinity for -1.  The code the assignment kernel runs, compiled for the host: bit-identical labels and residuals.
 * Models as for lsqr_assign; n_models == 0 returns LSQR_OK and writes nothing; n_models > 64 or a null cfg, params,
 * record or label_out returns LSQR_ERR_INVALID. */
LSQR_API int lsqr_assign_host(const lsqr_model_cfg *cfg, const double *params, size_t n_models, const void *record,
                              int32_t *label_out, double *residual_out /* nullable */);
/* The same for lsqr_assign_dense (below): cfg is LSQR_MODEL_DENSE with dim n = 1..64, params holds n_models rows of n
 * doubles, record is one row (a[0..n), b) of n + 1 doubles.  The code the kernel of lsqr_assign_dense runs, compiled
 * for the host: the residual is the running sum in slot order, sum += a[i] * x[i], then - b, bit for bit.  A record
 * with a non-finite slot among its n + 1 gets -1 and +infinity.  n_models == 0 returns LSQR_OK and writes nothing;
 * every other model, dim 0 or above 64, n_models > 64 or a null cfg, params, record or label_out returns
 * LSQR_ERR_INVALID and writes nothing.  lsqr_assign_host keeps refusing LSQR_MODEL_DENSE. */
LSQR_API int lsqr_assign_dense_host(const lsqr_model_cfg *cfg, const double *params, size_t n_models,
                                    const void *record, int32_t *label_out, double *residual_out /* nullable */);
/* The same for lsqr_assign_rigid (below): cfg is LSQR_MODEL_ABSOR (ls_type 0: record = a pair of 6 doubles; ls_type 2:
 * 7 doubles, slot 6 the weight), LSQR_MODEL_PIVOT (a frame of 13 slots) or LSQR_MODEL_RAY (6 doubles); params holds
 * n_models rows of lsqr_num_params doubles.  The code the kernel of lsqr_assign_rigid runs, compiled for the host:
 * bit-identical labels and residuals.  A record with a non-finite slot among those the model loads -- the weight
 * included with ls_type 2 -- gets -1 and +infinity.  n_models == 0 returns LSQR_OK and writes nothing; every other
 * model, n_models > 64 or a null cfg, params, record or label_out returns LSQR_ERR_INVALID and writes nothing.
 * lsqr_assign_host keeps refusing these three models. */
LSQR_API int lsqr_assign_rigid_host(const lsqr_model_cfg *cfg, const double *params, size_t n_models,
                                    const void *record, int32_t *label_out, double *residual_out /* nullable */);

/* ---- agree() scan over all observations (RANSAC.hxx:94-99, without the early exit) ---------- */
LSQR_API int lsqr_scan(lsqr_ctx *ctx);
/* Results of the current batch: any pointer may be NULL.  params: H*P doubles; valid: H bytes
 * (0 = degenerate subset, estimate() returned an empty vector); votes: H counts. */
LSQR_API int lsqr_get_hypotheses(lsqr_ctx *ctx, double *params, uint8_t *valid, uint32_t *votes);
LSQR_API size_t lsqr_num_hypotheses(const lsqr_ctx *ctx);
/* parameters (P doubles) and validity of one hypothesis of the current batch */
LSQR_API int lsqr_get_hypothesis(lsqr_ctx *ctx, size_t hypothesis, double *params, uint8_t *valid);
/* First-max winner of the current batch packed as (votes << 32) | (0xFFFFFFFF - index), so that a
 * max-reduction over ranks (RCCL all-reduce) keeps the earliest best hypothesis (RANSAC.hxx:100). */
LSQR_API int lsqr_best(lsqr_ctx *ctx, uint64_t *packed);

/* ---- consensus mask (RANSAC.hxx:129-137) ----------------------------------------------------- */
/* mask[i] = agree(params, data[i]) for i in [begin, end); kept on the device for lsqr_ls_fit.
 * mask_out (nullable) receives end-begin bytes.  count_out (nullable) the number of inliers. */
LSQR_API int lsqr_mask(lsqr_ctx *ctx, const double *params, size_t begin, size_t end,
                       uint8_t *mask_out, uint64_t *count_out);
LSQR_API int lsqr_mask_from_hypothesis(lsqr_ctx *ctx, size_t hypothesis, uint8_t *mask_out,
                                       uint64_t *count_out);
LSQR_API int lsqr_set_mask(lsqr_ctx *ctx, const uint8_t *mask); /* N bytes from the host */

/* ---- final fit (leastSquaresEstimate(), ParametersEstimator.h:51) ---------------------------- */
/* use_mask = 0 fits all observations, 1 only those in the device mask.  LSQR_EMPTY = the reference's empty
 * vector (info->n_params == 0); after a failed Levenberg-Marquardt run (info->lm_info outside 1..4) params_out
 * still receives the last iterate, for diagnostics only. */
LSQR_API int lsqr_ls_fit(lsqr_ctx *ctx, int use_mask, double *params_out, lsqr_fit_info *info);
/* Building blocks for multi-GPU fits: the normal-equation / moment block of [begin,end) and the
 * small solve from a (summed) block.  lsqr_moments_len gives the block length in doubles. */
LSQR_API int lsqr_moments_len(const lsqr_model_cfg *cfg, int phase);
/* phase 0: the model's linear LS block about the origin x (ND doubles: any point near the model,
 * identical on every rank); phase 1: the LM block {sum f^2, J^T J, J^T f} at the trial point x. */
LSQR_API int lsqr_moments(lsqr_ctx *ctx, int use_mask, size_t begin, size_t end, int phase,
                          const double *x, double *block_out);
/* Small solve (on the device) from a summed phase-0 block taken about `origin`. */
LSQR_API int lsqr_solve_moments(lsqr_ctx *ctx, const double *block, const double *origin,
                                double *params_out, lsqr_fit_info *info);
/* Multi-GPU step, per rank, one host synchronisation: hypothesis `stream_index` of sampler stream
 * `seed` (the global winner, re-derived locally -- the sampler is stateless) -> consensus mask over
 * [begin, end) -> phase-0 block of that slice about the model's own point (plane / line: a, sphere: c,
 * else zeros).  params_out: lsqr_num_params doubles; origin_out: 32 doubles (pass it to
 * lsqr_solve_moments together with the summed block); block_out: lsqr_moments_len(cfg, 0) doubles;
 * count_out: inliers of the slice.  LSQR_EMPTY if the subset is degenerate. */
LSQR_API int lsqr_winner_moments(lsqr_ctx *ctx, uint64_t seed, uint64_t stream_index, size_t begin,
                                 size_t end, double *params_out, double *origin_out,
                                 double *block_out, uint64_t *count_out);
/* lsqr_moments with the block left in device memory and no synchronisation (the caller all-reduces it in
 * place on the context's stream, see lsqr_set_stream, and reads it back once).  x is staged in one of four
 * pinned slots, each guarded by an event: calls may be issued back to back. */
LSQR_API int lsqr_moments_dev(lsqr_ctx *ctx, int use_mask, size_t begin, size_t end, int phase,
                              const double *x, double *block_dev);
/* Levenberg-Marquardt over summed phase-1 blocks (MINPACK lmder control flow on the device):
 *   lsqr_lm_begin(x0) -> x_trial;  repeat { block = sum over ranks of lsqr_moments(phase 1,
 *   x_trial);  lsqr_lm_step(block) -> cont, x_trial }  until !cont.  On the last step params_out
 *   receives the full parameter vector (status LSQR_EMPTY if LM did not converge).
 *   LSQR_MODEL_PHANTOM: every residual is linear in 31 functions of the parameters, so the phase-1
 *   block is the phase-0 Gram block (independent of x_trial) and the first lsqr_lm_step runs the whole
 *   minimisation from x0 on it (cont = 0). */
LSQR_API int lsqr_lm_begin(lsqr_ctx *ctx, const double *x0, double *x_trial_out);
LSQR_API int lsqr_lm_step(lsqr_ctx *ctx, const double *block, double *x_trial_out, int *cont,
                          double *params_out, lsqr_fit_info *info);
/* residual statistics as getDistanceStatistics() (SphereParametersEstimator.hxx:341-377):
 * out = {min, max, mean, sum of squares} */
LSQR_API int lsqr_stats(lsqr_ctx *ctx, const double *params, int use_mask, double out[4]);
/* the residual of every record in [begin, end) under `params`, in record order: the `distances`
 * vector of PlanePhantomUSCalibrationParametersEstimator::getDistanceStatistics (.cxx:455-549);
 * defined for every model (the quantity lsqr_stats summarises).  out: end - begin doubles (host). */
LSQR_API int lsqr_residuals(lsqr_ctx *ctx, const double *params, size_t begin, size_t end,
                            double *out);

/* ---- whole path: RANSAC<T,S>::compute() ------------------------------------------------------ */
/* Probabilistic overload (RANSAC.h:75-79).  Subsets come from `subsets` (n_subsets tuples, draw
 * order) when non-NULL, else from the device sampler stream `seed`.  Hypotheses are evaluated in
 * batches on the device and the serial loop of RANSAC.hxx:49-117 (duplicate filter, adaptive
 * numTries, strict-> best update) is replayed over the batch results, so the outcome equals
 * the serial reference's for the same subset stream.  params_out: lsqr_num_params doubles;
 * consensus_out (nullable): N bytes.  Invalid input (N < k, p outside (0,1)) returns
 * LSQR_ERR_INVALID with info->fraction = 0 and params_out untouched (RANSAC.hxx:16-19). */
LSQR_API int lsqr_ransac(lsqr_ctx *ctx, double p, uint64_t seed, const uint32_t *subsets,
                         size_t n_subsets, double *params_out, uint8_t *consensus_out,
                         lsqr_ransac_info *info);
/* Sequential RANSAC: up to max_models models from the context's current upload / attach of N records, the records
 * staying on the device between the rounds.  Round r is decided exactly as lsqr_ransac(ctx2, p, seeds[r], NULL, 0, ...)
 * would decide it on a fresh context ctx2 with the same model and options that holds only the records no earlier round
 * claimed, in their original order, tightly packed: every model lsqr_ransac accepts (the Levenberg-Marquardt fits
 * included), the option "max_iterations" and the 2^22 no-model stop apply per round.  There is no caller-supplied
 * subset stream.
 *   Accepting: round r is accepted when it returns LSQR_OK with best_votes >= max(min_votes, 1); it then claims its
 *     consensus set.  The first round that is not accepted is the last one; it claims nothing and *n_models_out = r.
 *     infos[r], status_out[r] and row r of params_out (lsqr_num_params doubles) are written as lsqr_ransac returns /
 *     writes them for every round that ran, the rejected one included (the caller sees the rejected candidate).
 *   Rounds that did not run: before the first round every status_out entry is set to LSQR_ERR_STATE ("round not run")
 *     and every infos entry is zeroed.  A round does not run when r == max_models or when fewer than lsqr_min_subset
 *     records remain.
 *   labels_out (nullable, N entries in upload order): r where round r claimed the record, else -1; copied to the host
 *     once, at the end.  infos[r].fraction is votes / records that remained in round r, as the fresh-context call
 *     reports it; infos[r].best_index and the fit origin of the first-record models refer to the compacted records.
 *   Argument errors (LSQR_ERR_INVALID, nothing written): p outside (0, 1); with max_models > 0 a null seeds,
 *     params_out, infos, status_out or n_models_out.  max_models == 0 returns LSQR_OK and sets *n_models_out = 0.  No
 *     model or no records: LSQR_ERR_STATE.  A round that fails outright (LSQR_ERR_HIP) ends the call with that status.
 *   Afterwards the context holds the caller's original records again -- same pointer, count and stride, exactly as
 *     after lsqr_upload / lsqr_attach: hypotheses and mask are void, the spatial index is dropped.  The caller's
 *     records are only read: attached (caller-owned) device memory is never written; the survivors of a round are
 *     compacted (stable, with their upload indices) into buffers the context owns (csrc/sequential.h), and the context
 *     is re-pointed at them by the path lsqr_attach takes.  The work runs on the context's stream (lsqr_set_stream).
 *   lsqr_multi handles have no sequential form: call it on one device's context. */
LSQR_API int lsqr_ransac_sequential(lsqr_ctx *ctx, double p, const uint64_t *seeds /* max_models */, size_t max_models,
                                    uint64_t min_votes, double *params_out /* max_models * lsqr_num_params */,
                                    int32_t *labels_out /* nullable: N entries, upload order */,
                                    lsqr_ransac_info *infos /* max_models */, int32_t *status_out /* max_models */,
                                    size_t *n_models_out);
/* Sequential RANSAC over many independent problems in one call: lsqr_ransac_sequential's loop for every record set of
 * an lsqr_ransac_many upload.  Problem j is records [offsets[j], offsets[j+1]) of host_records (laid out as for
 * lsqr_ransac_many) and is decided exactly as lsqr_ransac_sequential(ctx2, p, seeds + j * max_models, max_models,
 * min_votes, ...) decides it on a fresh context ctx2, with the same model and options, that holds those records alone.
 *   Rounds: round r of problem j is the lsqr_ransac decision with seed seeds[j * max_models + r] on the records of j no
 *     earlier round claimed, in their original order.  It is accepted when it is LSQR_OK with best_votes >=
 *     max(min_votes, 1) and then claims its consensus set.  The first round that is not accepted is the problem's last:
 *     infos[j * max_models + r], status_out[j * max_models + r] and row j * max_models + r of params_out
 *     (lsqr_num_params doubles; written where the status is LSQR_OK) are still written, and it claims nothing.
 *     n_models_out[j]: the accepted rounds of problem j.
 *   Rounds that did not run: before the first round every status_out entry is set to LSQR_ERR_STATE and every infos
 *     entry is zeroed.  A round does not run when r == max_models or when fewer than lsqr_min_subset records of the
 *     problem remain.  A problem that starts with fewer than lsqr_min_subset records, zero included, runs no round:
 *     n_models_out[j] = 0, its labels are -1, and the other problems are unaffected.
 *   labels_out (nullable, offsets[n_problems] entries in the caller's record order): the round that claimed the
 *     record, else -1; copied to the host once, at the end.  infos[j][r].fraction is votes / the records of j that
 *     remained in round r; best_index and the fit origin of the first-record models refer to problem j's compacted
 *     records, as in lsqr_ransac_sequential.
 *   Models, taken from the context's lsqr_set_model: every model lsqr_ransac_many, lsqr_ransac_many_lm (the geometric
 *     sphere: every round ends in the batched Levenberg-Marquardt stage) or lsqr_ransac_many_dense accepts; a round is
 *     one job of the run those entry points use, on the survivors.  LSQR_MODEL_US_SINGLE, LSQR_MODEL_US_POINTER and
 *     LSQR_MODEL_PHANTOM return LSQR_ERR_INVALID and write nothing.  Records wider than 18 doubles (the dense system
 *     with dim > 17) and more than 2^32 - 16 records in all are refused with LSQR_ERR_INVALID, nothing written, as
 *     lsqr_ransac_sequential refuses them.
 *   Argument errors (LSQR_ERR_INVALID, nothing written) and the n_problems == 0 no-op are lsqr_ransac_many's; in
 *     addition, with max_models > 0, a null seeds, params_out, infos, status_out or n_models_out.  max_models == 0
 *     returns LSQR_OK and zeroes n_models_out (where given).  A null context is refused before anything is touched.
 *   Per round and problem, against that lsqr_ransac_sequential call: bit-identical n_models, status, iterations,
 *     best_index, best_votes, fraction, n_params, fit.n_used and labels; parameters and fit.cost up to the fp64
 *     summation order of the final fit; the LM fields as lsqr_ransac_many_lm states them.  The options
 *     "max_iterations" and the 2^22 no-model stop apply per problem and per round.
 *   Independence: problem j's results, parameters and labels included, are bit-identical whichever other problems
 *     share the call, in whatever order, and however "many_round_hypotheses" cuts the rounds.
 *   The records are uploaded once; between two rounds the unclaimed records of the problems that go on are compacted
 *     on the device (csrc/many_sequential.h), and the consensus bytes never cross to the host.  The context's own
 *     upload, hypotheses and mask are not touched; the work runs on the context's stream (lsqr_set_stream). */
LSQR_API int lsqr_ransac_many_sequential(lsqr_ctx *ctx, const void *host_records, size_t stride_bytes,
                                         const uint64_t *offsets /* n_problems + 1 */, size_t n_problems, double p,
                                         const uint64_t *seeds /* n_problems * max_models, seeds[j * max_models + r] */,
                                         size_t max_models, uint64_t min_votes,
                                         double *params_out /* n_problems * max_models * lsqr_num_params */,
                                         int32_t *labels_out /* nullable: offsets[n_problems] entries, record order */,
                                         lsqr_ransac_info *infos /* n_problems * max_models */,
                                         int32_t *status_out /* n_problems * max_models */,
                                         size_t *n_models_out /* n_problems */);
/* Grouped RANSAC: one problem per label over the records the context already holds on the device.  It works on the
 * context's current upload or attach (lsqr_upload / lsqr_attach), as lsqr_ransac_sequential does: the records are
 * lsqr_count(ctx) records at the context's pointer and stride; they are only read, and attached (caller-owned) memory
 * is never written.  groups[i] is the label of record i: problem g is the records with groups[i] == g, in upload
 * order; a record whose label is negative or >= n_groups belongs to no problem.
 *   on_device = 1: groups and consensus_out are device pointers (say, tensors beside the attached records); 0: host
 *     pointers -- then the labels go up and the consensus comes down by one copy each.  seeds, params_out,
 *     offsets_out, infos and status_out are host pointers in both forms.
 *   Contract: problem g is decided exactly as the matching batched entry point decides problem g of a host call whose
 *     records are the stable gather by label of the context's records, tightly packed, with offsets the prefix sums of
 *     the group sizes and the same seeds: lsqr_ransac_many for the closed-form models, lsqr_ransac_many_lm for the
 *     geometric sphere, lsqr_ransac_many_dense for LSQR_MODEL_DENSE.  The records are grouped on the device (keys, a
 *     stable radix sort, a gather of lsqr_record_doubles 8-byte words per record copied as integers:
 *     csrc/grouped.h), and the search is the same job -- the run those entry points use, unchanged -- on the same
 *     packed bytes under the same offsets.  So everything those entry points write is bit-identical, parameters,
 *     fit.cost and the LM fields included; only info.evaluated is exempt, as it is between two calls of theirs.
 *   Outputs: status_out[g], infos[g] and row g of params_out follow those entry points' rules, N_g < k ->
 *     LSQR_ERR_INVALID for that group included.  consensus_out (nullable, lsqr_count(ctx) bytes in upload order):
 *     the consensus byte of record i in its problem, as those entry points report it; 0 for a record in no problem and
 *     for every record of a problem without a winner; every byte is written.  offsets_out (nullable, host,
 *     n_groups + 1): the prefix sums of the group sizes.
 *   Models, taken from the context's lsqr_set_model: every model the three entry points accept; the dense system up
 *     to dim 64.  LSQR_MODEL_US_SINGLE, LSQR_MODEL_US_POINTER and LSQR_MODEL_PHANTOM return LSQR_ERR_INVALID and write
 *     nothing.
 *   Argument errors (LSQR_ERR_INVALID, nothing written): p outside (0, 1); with n_groups > 0 a null groups, seeds,
 *     params_out, infos or status_out; n_groups > 2^31 - 1; more than 2^32 - 16 records.  No model, or no records in
 *     the context: LSQR_ERR_STATE.  n_groups == 0 is a no-op returning LSQR_OK.  A null context is refused before
 *     anything is touched.
 *   The context's upload, hypotheses, mask and spatial index are untouched; the work runs on the context's stream
 *     (lsqr_set_stream), and the call returns after it has finished.  One synchronisation precedes the search: the
 *     n_groups + 1 offsets cross to the host, where the batched job plans its rounds.  The options "max_iterations",
 *     "many_round_hypotheses", "dense_fast_solve", "dense_dd" and the 2^22 no-model stop apply per problem as in the
 *     batched entry points.  lsqr_multi handles have no grouped form. */
LSQR_API int lsqr_ransac_grouped(lsqr_ctx *ctx, const int32_t *groups /* lsqr_count(ctx) entries, upload order */,
                                 size_t n_groups, int on_device /* 1: groups, consensus_out on the device; 0: host */,
                                 double p, const uint64_t *seeds /* host, n_groups */,
                                 double *params_out      /* host, n_groups * lsqr_num_params */,
                                 uint8_t *consensus_out  /* nullable: lsqr_count(ctx) bytes, upload order */,
                                 uint64_t *offsets_out   /* nullable, host: n_groups + 1 */,
                                 lsqr_ransac_info *infos /* host, n_groups */,
                                 int32_t *status_out     /* host, n_groups */);
/* Grouped sequential RANSAC: several models per label over the records the context already holds on the device --
 * lsqr_ransac_grouped's records and labels, lsqr_ransac_many_sequential's rounds.  It works on the context's current
 * upload or attach: lsqr_count(ctx) records at the context's pointer and stride, which are only read; attached
 * (caller-owned) memory is never written.  Labels as in lsqr_ransac_grouped: group g is the records with
 * groups[i] == g, in upload order; a record whose label is negative or >= n_groups belongs to no group.
 *   on_device = 1: groups and labels_out are device pointers, and nothing per-record crosses to the host; 0: host
 *     pointers -- then the labels go up and the result comes down by one copy each.  seeds, params_out, offsets_out,
 *     infos, status_out and n_models_out are host pointers in both forms.
 *   Contract: group g is decided exactly as lsqr_ransac_many_sequential decides problem g of a host call whose records
 *     are the stable gather by label of the context's records, tightly packed, with offsets the prefix sums of the
 *     group sizes and the same seeds (seeds[g * max_models + r]), max_models, min_votes, p, model and options.  The
 *     records are grouped on the device as in lsqr_ransac_grouped (integer copies); round 0 runs on the same packed
 *     bytes under the same offsets through the same job, and every later round is that entry point's own code
 *     (csrc/grouped.h, csrc/many_sequential.h).  So everything that call writes is bit-identical, parameters, fit.cost
 *     and the LM fields included; only info.evaluated is exempt, as it is between two calls of the existing entry
 *     points.
 *   labels_out (nullable, lsqr_count(ctx) entries in upload order): the round that claimed record i inside its group;
 *     -1 for an unclaimed record and for a record in no group.  Every entry is written exactly once (no fill of the
 *     caller's buffer precedes it).  offsets_out (nullable, host, n_groups + 1): the prefix sums of the group sizes.
 *   Outputs: infos[g * max_models + r], status_out[g * max_models + r], row g * max_models + r of params_out and
 *     n_models_out[g] follow lsqr_ransac_many_sequential's rules: LSQR_ERR_STATE and a zeroed info for a round that did
 *     not run; the rejected round's row is written; a group of fewer than lsqr_min_subset records runs no round.
 *     best_index and the fit origin of the first-record models refer to the group's compacted records, as there.
 *   Models, taken from the context's lsqr_set_model: those of lsqr_ransac_many_sequential.  LSQR_MODEL_US_SINGLE,
 *     LSQR_MODEL_US_POINTER and LSQR_MODEL_PHANTOM return LSQR_ERR_INVALID; so do records outside 2 .. 18 doubles (the
 *     dense system with dim > 17); nothing is written, as there.
 *   Checks, in this order: a null context is refused before anything is touched; the model; n_groups == 0 is a no-op
 *     returning LSQR_OK; with max_models > 0 a null groups, seeds, params_out, infos, status_out or n_models_out
 *     (LSQR_ERR_INVALID); p outside (0, 1) (LSQR_ERR_INVALID); n_groups or max_models > 2^31 - 1 (LSQR_ERR_INVALID); no
 *     model, or no records in the context (LSQR_ERR_STATE); more than 2^32 - 16 records (LSQR_ERR_INVALID);
 *     max_models == 0 returns LSQR_OK, zeroes n_models_out where given and writes nothing else.  Every argument error
 *     writes nothing.
 *   The context's upload, hypotheses, mask and spatial index are untouched; the work runs on the context's stream
 *     (lsqr_set_stream), and the call returns after it has finished.  One synchronisation precedes round 0 (the
 *     n_groups + 1 offsets cross to the host); then come those of the rounds.  The options "max_iterations",
 *     "many_round_hypotheses", "dense_fast_solve", "dense_dd" and the 2^22 no-model stop apply per group and round, as
 *     in the entry points it is made of.  lsqr_multi handles have no such form. */
LSQR_API int lsqr_ransac_grouped_sequential(
    lsqr_ctx *ctx, const int32_t *groups /* lsqr_count(ctx) entries, upload order */, size_t n_groups,
    int on_device /* 1: groups, labels_out on the device; 0: host */, double p,
    const uint64_t *seeds /* host, n_groups * max_models, seeds[g * max_models + r] */, size_t max_models,
    uint64_t min_votes, double *params_out /* host, n_groups * max_models * lsqr_num_params */,
    int32_t *labels_out /* nullable: lsqr_count(ctx) entries, upload order */,
    uint64_t *offsets_out /* nullable, host: n_groups + 1 */, lsqr_ransac_info *infos /* host, n_groups * max_models */,
    int32_t *status_out /* host, n_groups * max_models */, size_t *n_models_out /* host, n_groups */);
/* ---- nearest-model assignment and refit on the device (csrc/assign.h) ---------------------------------------------
 * The multi-model entry points above stop at greedy labels: round r claims every record that agrees with model r, and
 * each model is fitted once, on what earlier rounds left.  These two finish the job on the records where they are.
 * lsqr_assign: params holds n_models (<= 64) rows of lsqr_num_params doubles; each row becomes a scan row exactly as
 *   lsqr_mask makes one.  For every record x of the context's upload / attach
 *     label(x) = the smallest m in [0, n_models) that minimises residual(row_m, x) among the m with agree(row_m, x);
 *                -1 when no m agrees
 *   (ties go to the smaller m; a record with a non-finite coordinate agrees with nothing).  labels_out[i] is the
 *   label of record i in upload order; residuals_out[i] (nullable) its residual to that model, +infinity for -1: the
 *   values lsqr_mask and lsqr_residuals give for that row, bit for bit.  counts_out (nullable, host, n_models + 1):
 *   the records per model, then the unassigned ones.  on_device = 1: labels_out and residuals_out are device
 *   pointers; 0: host.
 * lsqr_refine: assignment and least-squares refit in turn,
 *     r = 0
 *     loop: L_r = assign(params_r)
 *           if r > 0 and L_r == L_{r-1}: converged, stop
 *           if r == max_rounds: stop
 *           params_{r+1} = refit(L_r);  r += 1
 *   A round is ONE pass over the records (the pass that makes L_r also sums the moments of L_r, per model, about the
 *   model's own point: the plane's and the line's point, the sphere's centre), one small solve launch and one 8-byte
 *   read of the changed-counter.  On return *rounds_out = r, the refits done; params_inout = params_r; labels_out
 *   (nullable) = L_r; counts_out (nullable) the counts of L_r; *converged_out says which stop it was.  So the
 *   returned labels are always exactly lsqr_assign of the returned parameters, and max_rounds == 0 is lsqr_assign.
 *   Refit of model m: with at least lsqr_min_subset records labelled m and a solve that gives a result the row is
 *   replaced, otherwise it keeps its values for that round.  status_out[m]: LSQR_OK or LSQR_EMPTY for the last refit
 *   round (LSQR_OK if no refit ran); fits[m].n_used: the records behind the last refit attempt; fits[m].n_params as
 *   lsqr_ls_fit reports it (0 with LSQR_EMPTY, and where no refit ran).  No sum is a floating-point atomic: the same
 *   call twice gives the same bits.
 *   Models, taken from the context's lsqr_set_model: LSQR_MODEL_PLANE, LSQR_MODEL_LINE and LSQR_MODEL_SPHERE in every
 *     dimension lsqr_set_model accepts for them, and LSQR_MODEL_LINE2D, whose parameters [n, a] carry a point: it is
 *     accepted by both.  lsqr_assign takes the sphere with either ls_type; lsqr_refine refuses the geometric sphere
 *     (its fit is Levenberg-Marquardt) with LSQR_ERR_INVALID: lsqr_refine_lm, below, takes it.  Every other model
 *     returns LSQR_ERR_INVALID.
 *   Checks, in this order: a null context is refused before anything is touched; the model (none set: LSQR_ERR_STATE);
 *     n_models == 0 is a no-op returning LSQR_OK; n_models > 64, or a null params or labels_out (lsqr_assign), a null
 *     params_inout, fits, status_out, rounds_out or converged_out (lsqr_refine) (LSQR_ERR_INVALID); no records in the
 *     context (LSQR_ERR_STATE); more than 2^32 - 16 records (LSQR_ERR_INVALID).  Every argument error writes nothing.
 *   The records are only read, at any stride; the context's hypotheses, mask, spatial index and the parameters of its
 *     last mask are left as they were; the work runs on the context's stream (lsqr_set_stream), and the call returns
 *     after it has finished.  lsqr_multi handles have no such form. */
LSQR_API int lsqr_assign(lsqr_ctx *ctx, const double *params /* host, n_models * lsqr_num_params */, size_t n_models,
                         int on_device /* 1: labels_out, residuals_out are device pointers */,
                         int32_t *labels_out /* lsqr_count(ctx) entries, upload order */,
                         double *residuals_out /* nullable */,
                         uint64_t *counts_out /* nullable, host: n_models + 1, last = unassigned */);
LSQR_API int lsqr_refine(lsqr_ctx *ctx, double *params_inout /* host, n_models * lsqr_num_params */, size_t n_models,
                         size_t max_rounds, int on_device /* 1: labels_out is a device pointer */,
                         int32_t *labels_out /* nullable */, uint64_t *counts_out /* nullable, host: n_models + 1 */,
                         lsqr_fit_info *fits /* host, n_models */, int32_t *status_out /* host, n_models */,
                         size_t *rounds_out, int *converged_out);
/* ---- lsqr_refine for the geometric sphere: a Levenberg-Marquardt run per model (csrc/assign_lm.h) ------------------
 * lsqr_refine_lm is lsqr_refine -- its arguments, its loop, its stop rules, rounds_out / converged_out / counts_out /
 * labels_out, the order of its checks, "every argument error writes nothing" -- for the one model lsqr_refine refuses.
 * So here too the returned labels are always exactly lsqr_assign of the returned parameters, and max_rounds == 0 is
 * lsqr_assign.
 *   Models: LSQR_MODEL_SPHERE with LSQR_LS_GEOMETRIC (the default of lsqr_set_model's callers and of the reference) in
 *     every dimension lsqr_set_model accepts (2..8).  Every other model, the algebraic sphere included, returns
 *     LSQR_ERR_INVALID and writes nothing: lsqr_refine takes the fits in closed form.
 *   Refit of model m in a round: with at least lsqr_min_subset records labelled m, the algebraic fit of those records
 *     about the model's centre -- bit for bit the row lsqr_refine writes on an algebraic context -- is the START of a
 *     Levenberg-Marquardt run over the same records, with the settings and the control flow of lsqr_ls_fit's geometric
 *     sphere.  An evaluation is one pass over the records where they are, under the labels of the round, for all models
 *     still running at once, one step launch and one 4-byte read.  The row is replaced only when the algebraic solve
 *     gave a result AND the run ended with lm_info in 1..4; otherwise it keeps the values it had BEFORE the round (the
 *     algebraic intermediate is never returned: the reference returns an empty vector and the caller keeps its model).
 *   fits[m] and status_out[m] describe the last refit round: n_params (lsqr_num_params or 0), lm_info, lm_nfev,
 *     reserved (the stall evaluation, as lsqr_ls_fit), cost, n_used; lm_info = 0 where no run started (too few records,
 *     or no algebraic start).  status_out[m]: LSQR_OK or LSQR_EMPTY; LSQR_OK with a zeroed fit when no refit ran.
 *   Round by round, model m's new row agrees within the LM tolerances with lsqr_set_mask(L_r == m) + lsqr_ls_fit(
 *     use_mask = 1) on a geometric-sphere context over the same records: only the origin of the algebraic start and the
 *     order of the fp64 sums differ.  No sum is a floating-point atomic: the same call twice gives the same bits.  Model
 *     m's iterates are a function of its own records, their positions in the upload and its own trial points: the
 *     other rows of the call, and where m sits among them, change nothing.
 *   The context's hypotheses, mask, spatial index and the parameters of its last mask are left as they were; the work
 *     runs on the context's stream.  The options lm_persist and lm_host do not apply (the step runs on the device, as
 *     in lsqr_ransac_many_lm).  lsqr_refine_lm_grouped, below, is the form with one model set per label; lsqr_multi
 *     handles have no such form. */
LSQR_API int lsqr_refine_lm(lsqr_ctx *ctx, double *params_inout /* host, n_models * lsqr_num_params */,
                            size_t n_models, size_t max_rounds, int on_device /* 1: labels_out is a device pointer */,
                            int32_t *labels_out /* nullable */,
                            uint64_t *counts_out /* nullable, host: n_models + 1 */,
                            lsqr_fit_info *fits /* host, n_models */, int32_t *status_out /* host, n_models */,
                            size_t *rounds_out, int *converged_out);
/* ---- lsqr_assign / lsqr_refine for the dense linear system (csrc/assign_dense.h) -----------------------------------
 * A mixture of linear regressions: every row (a | b) goes to the nearest of up to 64 regressions x_m it agrees with,
 * and every regression is fitted again on its own rows.  lsqr_assign_dense / lsqr_refine_dense are lsqr_assign /
 * lsqr_refine -- their arguments, their loop and its stop rules, rounds_out / converged_out / counts_out / labels_out,
 * the order of their checks, "every argument error writes nothing" -- with the model changed; lsqr_assign and
 * lsqr_refine keep refusing the dense model, as lsqr_ransac_many refuses it beside lsqr_ransac_many_dense.
 *   Model: LSQR_MODEL_DENSE, dim n = 1..64, rows of n + 1 doubles (a[0..n), b) at any stride >= the record, from
 *     lsqr_upload or lsqr_attach.  Every other model returns LSQR_ERR_INVALID and writes nothing.  n_models <= 64;
 *     params holds n_models rows of n doubles.
 *   Decision: label(x) = the smallest m that minimises |a . x_m - b| among the m with |a . x_m - b| < delta (strict
 *     '<' while m walks upwards: ties go to the smaller m); -1 when none agrees, and for a row with a non-finite slot
 *     among its n + 1.  The dot product is the reference's running sum in slot order, sum += a[i] * x[i], then - b, not
 *     reassociated and not contracted, so labels_out[i] and residuals_out[i] (+infinity for -1) equal, bit for bit,
 *     what lsqr_mask and lsqr_residuals give for that row of params on the same context, and what
 *     lsqr_assign_dense_host gives.
 *   Loop: lsqr_refine's.  max_rounds == 0 is lsqr_assign_dense, and the returned labels are always exactly
 *     lsqr_assign_dense of the returned parameters.
 *   Refit of model m in a round: with at least lsqr_min_subset (= n) rows labelled m, the least-squares solution over
 *     those rows by lsqr_ls_fit's route: the packed block sum z z^T, z = (a | b); the elimination under the options
 *     dense_fast_solve and dense_dd; where it meets a pivot below 1e-6 max|G| and dense_dd is on, the double-double
 *     solve from the rows labelled m.  The row is replaced only when the solve gives a result, otherwise it keeps its
 *     values.  status_out[m]: LSQR_OK or LSQR_EMPTY (LSQR_OK when no refit ran); fits[m] for the last refit round:
 *     n_params (n or 0), n_used (the rows behind the attempt) and reserved, the route as lsqr_ls_fit reports it (0: the
 *     elimination, 1: double-double from the rows, 2: dense_dd 0 and a pivot below 1e-6); zeroed where none ran.
 *     Model m's new row agrees with lsqr_set_mask(L_r == m) + lsqr_ls_fit(use_mask = 1) on the same context up to the
 *     order of the fp64 sums.
 *   Sums: none is a floating-point atomic; the same call twice gives the same bits.  A model's block is a function of
 *     its own rows, their positions in the upload and the fixed chunking (256 rows per chunk up to n = 32, 128 above;
 *     within a chunk in row order, the chunks in order): not of the grid, of the other models of the call, or of where
 *     m sits among them.
 *   Per round the rows are read once (by the one pass that labels them and sums the blocks from the same on-chip
 *     copy), and the host reads the changed-counter with the counts and, with dense_dd, the models' flags, in one copy.
 *   Device scratch of a refine call: ceil(N / chunk) * n_models * ((n+1)(n+2)/2 + 1, rounded up to 8) doubles of
 *     partial blocks, two label arrays, one word per chunk.  If it cannot be allocated the call returns LSQR_ERR_HIP
 *     with the allocation in lsqr_last_error; there is no other path.
 *   Checks, in this order: a null context; the model (none set: LSQR_ERR_STATE; not dense: LSQR_ERR_INVALID);
 *     n_models == 0 is a no-op returning LSQR_OK; n_models > 64, or a null params or labels_out (lsqr_assign_dense), a
 *     null params_inout, fits, status_out, rounds_out or converged_out (lsqr_refine_dense) (LSQR_ERR_INVALID); no
 *     records in the context (LSQR_ERR_STATE); more than 2^32 - 16 records (LSQR_ERR_INVALID).
 *   The context's hypotheses, mask, spatial index, fp16 fragment copies and the parameters of its last mask are left
 *     as they were; the work runs on the context's stream, and the call returns after it has finished.
 *     lsqr_assign_dense_grouped / lsqr_refine_dense_grouped, below, are the forms with one regression set per label;
 *     lsqr_multi handles have no such form. */
LSQR_API int lsqr_assign_dense(lsqr_ctx *ctx, const double *params /* host, n_models * n */, size_t n_models,
                               int on_device /* 1: labels_out, residuals_out are device pointers */,
                               int32_t *labels_out /* lsqr_count(ctx) entries, upload order */,
                               double *residuals_out /* nullable */,
                               uint64_t *counts_out /* nullable, host: n_models + 1, last = unassigned */);
LSQR_API int lsqr_refine_dense(lsqr_ctx *ctx, double *params_inout /* host, n_models * n */, size_t n_models,
                               size_t max_rounds, int on_device /* 1: labels_out is a device pointer */,
                               int32_t *labels_out /* nullable */,
                               uint64_t *counts_out /* nullable, host: n_models + 1 */,
                               lsqr_fit_info *fits /* host, n_models */, int32_t *status_out /* host, n_models */,
                               size_t *rounds_out, int *converged_out);
/* ---- lsqr_assign / lsqr_refine for absolute orientation, pivot and ray (csrc/assign_rigid.h) -------------------------
 * Several rigid motions between two point sets, several tools pivoted in one recording, several targets triangulated
 * from one bundle of rays: every record goes to the nearest of up to 64 models it agrees with, and every model is
 * fitted again on its own records.  lsqr_assign_rigid / lsqr_refine_rigid are lsqr_assign / lsqr_refine -- their
 * arguments, their loop and its stop rules, rounds_out / converged_out / counts_out / labels_out, the order of their
 * checks, "every argument error writes nothing" -- with the model changed; lsqr_assign, lsqr_refine, lsqr_assign_host
 * and every grouped form keep refusing these models.
 *   Models: LSQR_MODEL_ABSOR with ls_type 0 (records of 6 doubles: first, second) or ls_type 2 (7 doubles, slot 6 the
 *     weight: the weighted fit); LSQR_MODEL_PIVOT (frames of 13 slots); LSQR_MODEL_RAY (6 doubles: p, n; aux is not
 *     used here).  Every other model returns LSQR_ERR_INVALID and writes nothing.  n_models <= 64; params holds
 *     n_models rows of lsqr_num_params doubles (7 / 6 / 3).
 *   Decision: label(x) = the smallest m that minimises residual(row_m, x) among the m with agree(row_m, x) (strict '<'
 *     while m walks upwards: ties go to the smaller m); -1 when none agrees, and for a record with a non-finite slot
 *     among those the model loads, the weight included with ls_type 2.  row_m is the scan row lsqr_mask makes of
 *     params[m], so labels_out[i] and residuals_out[i] (+infinity for -1) equal, bit for bit, the first argmin over
 *     lsqr_mask / lsqr_residuals of the same rows on the same context, and what lsqr_assign_rigid_host gives.  The
 *     ray's agree() holds t >= 0 beside the distance; its residual is the distance to the ray's LINE.
 *   Loop: lsqr_refine's.  max_rounds == 0 is lsqr_assign_rigid, and the returned labels are always exactly
 *     lsqr_assign_rigid of the returned parameters.
 *   Refit of model m in a round: with at least lsqr_min_subset (3 / 3 / 2) records labelled m, the moment block of
 *     those records and the model's closed-form solve (Horn's quaternion, weighted with ls_type 2; the pivot's 6 x 6
 *     normal equations; the rays' 3 x 3 system).  The row is replaced only when the solve gives a result -- rays that
 *     are all parallel, or frames that are all the same, give none --, otherwise it keeps its values.  status_out[m],
 *     fits[m].n_params and fits[m].n_used as lsqr_refine reports them.  Model m's new row agrees with
 *     lsqr_set_mask(L_r == m) + lsqr_ls_fit(use_mask = 1) on the same context up to the origin and the order of the
 *     fp64 sums (the quaternion up to its sign).
 *   Origin of model m's moment block (these parameters hold no point, so it is part of the contract):
 *     ray    the model's own point, params[m], as for the plane; it moves with the row from round to round;
 *     pivot  none: the block is not shifted;
 *     absolute orientation   the pair (first, second) of the lowest-index record that is finite and agrees with row m
 *            AS PASSED IN, fixed for the whole call: lsqr_ls_fit's "first record whose mask bit is set" for the mask
 *            of the entry row.  One pre-pass finds it, once per lsqr_refine_rigid call with max_rounds > 0 and never
 *            for lsqr_assign_rigid, with integer minima only.  It lies among the model's data even when record 0 is an
 *            outlier or not finite.  A model no record agrees with at entry can never receive one (rows change only by
 *            a refit), so it has no origin and needs none.
 *   Sums: none is a floating-point atomic; the same call twice gives the same bits.  A model's block is a function of
 *     its own records, their positions in the upload, its own row and origin, and the fixed chunking (2048 records per
 *     chunk for absolute orientation and the ray, 1024 for the pivot; within a chunk by lane and wave in a fixed tree,
 *     the chunks in order): not of the grid, of the other rows of the call, or of where m sits among them.
 *   Checks, in this order: a null context; the model (none set: LSQR_ERR_STATE; not one of the three:
 *     LSQR_ERR_INVALID); n_models == 0 is a no-op returning LSQR_OK; n_models > 64, or a null params or labels_out
 *     (lsqr_assign_rigid), a null params_inout, fits, status_out, rounds_out or converged_out (lsqr_refine_rigid)
 *     (LSQR_ERR_INVALID); no records in the context (LSQR_ERR_STATE); more than 2^32 - 16 records (LSQR_ERR_INVALID).
 *   The context's hypotheses, mask, spatial index and the parameters of its last mask are left as they were; the work
 *     runs on the context's stream, and the call returns after it has finished.  There is no grouped form and no
 *     lsqr_multi form; the US calibrations and the phantom are refused. */
LSQR_API int lsqr_assign_rigid(lsqr_ctx *ctx, const double *params /* host, n_models * lsqr_num_params */,
                               size_t n_models, int on_device /* 1: labels_out, residuals_out are device pointers */,
                               int32_t *labels_out /* lsqr_count(ctx) entries, upload order */,
                               double *residuals_out /* nullable */,
                               uint64_t *counts_out /* nullable, host: n_models + 1, last = unassigned */);
LSQR_API int lsqr_refine_rigid(lsqr_ctx *ctx, double *params_inout /* host, n_models * lsqr_num_params */,
                               size_t n_models, size_t max_rounds, int on_device /* 1: labels_out is a device pointer */,
                               int32_t *labels_out /* nullable */,
                               uint64_t *counts_out /* nullable, host: n_models + 1 */,
                               lsqr_fit_info *fits /* host, n_models */, int32_t *status_out /* host, n_models */,
                               size_t *rounds_out, int *converged_out);
/* ---- the same with ONE MODEL SET PER LABEL (csrc/assign_grouped.h) -------------------------------------------------
 * lsqr_assign_grouped / lsqr_refine_grouped take what lsqr_ransac_grouped_sequential leaves -- params_out and
 * n_models_out, unchanged -- over the same groups array and the same resident records: row g * max_models + m of params
 * is model m of group g; rows with m >= n_models[g] are never read and never written.  groups follows
 * lsqr_ransac_grouped's rules: group g is the records with groups[i] == g, in upload order; a negative label or one
 * >= n_groups puts the record in no group.  on_device = 1: groups, labels_out and residuals_out are device pointers;
 * 0: host pointers, one copy up and one copy down.
 *   Contract: group g is decided bit for bit as lsqr_assign / lsqr_refine decide it on a fresh context with the same
 *     model and options that holds the stable gather of group g's records, tightly packed, and is given rows
 *     g * max_models .. + n_models[g].  Bit-identical: labels_out[i] (the model index inside the record's group, or
 *     -1), residuals_out[i], the counts; for lsqr_refine_grouped also the returned parameters, status_out,
 *     fits[].n_used, fits[].n_params, rounds_out[g] and converged_out[g].  The sums keep lsqr_refine's order per
 *     group (chunks of 2048 of the group's packed records), nothing is summed with a floating-point atomic, so a
 *     group's results do not depend on the other groups of the call, on how the ids are numbered, or on the run.
 *   Each group runs lsqr_refine's loop on its own: it stops when r > 0 and its labels did not change, or when
 *     r == max_rounds; once stopped it is passed over, and its rows and labels stay as its last pass left them.  The
 *     host reads one 8-byte word per round (the groups still going).  max_rounds == 0 is lsqr_assign_grouped, and the
 *     returned labels are always exactly the grouped assignment of the returned parameters.
 *   What does not run: a record in no group, and every record of a group with n_models[g] == 0, gets label -1 and
 *     residual +infinity; every entry of labels_out / residuals_out is written exactly once (no fill of the caller's
 *     buffer precedes it).  A group with no records or with n_models[g] == 0 has rounds_out[g] = 0,
 *     converged_out[g] = 0, status_out LSQR_OK with zeroed fits for m < n_models[g], and untouched rows.  Entries
 *     with m >= n_models[g]: status_out LSQR_ERR_STATE (model not there) and a zeroed fit.
 *     counts_out[g * (max_models + 1) + m]: the records of group g labelled m (0 for m >= n_models[g]); slot
 *     max_models: the group's unassigned records.  offsets_out: the prefix sums of the group sizes.
 *   Models: those of lsqr_assign / lsqr_refine; lsqr_refine_grouped refuses the geometric sphere (LSQR_ERR_INVALID):
 *     lsqr_refine_lm_grouped, below, takes it.
 *   Checks, in this order: a null context is refused before anything is touched; the model (none set: LSQR_ERR_STATE;
 *     one the call does not take: LSQR_ERR_INVALID); n_groups == 0 is a no-op returning LSQR_OK; max_models > 64,
 *     n_groups > 2^31 - 1, a null groups, params, n_models or labels_out (assign), a null groups, params_inout,
 *     n_models, fits, status_out, rounds_out or converged_out (refine), any n_models[g] > max_models
 *     (LSQR_ERR_INVALID); no records in the context (LSQR_ERR_STATE); more than 2^32 - 16 records (LSQR_ERR_INVALID);
 *     max_models == 0 returns LSQR_OK after writing the -1 / +infinity labels and the zero outputs above.  Every
 *     argument error writes nothing.
 *   The context's upload, hypotheses, mask, spatial index and the parameters of its last mask are left as they were;
 *     the work runs on the context's stream, and the call returns after it has finished.  One synchronisation precedes
 *     the first pass (the n_groups + 1 offsets cross to the host); then one per round.  lsqr_multi handles have no
 *     such form. */
LSQR_API int lsqr_assign_grouped(lsqr_ctx *ctx, const int32_t *groups /* lsqr_count(ctx), upload order */,
                                 size_t n_groups, int on_device,
                                 const double *params /* host, n_groups * max_models * lsqr_num_params */,
                                 const size_t *n_models /* host, n_groups; each <= max_models */,
                                 size_t max_models /* <= 64 */,
                                 int32_t *labels_out /* lsqr_count(ctx) entries, upload order */,
                                 double *residuals_out /* nullable */,
                                 uint64_t *counts_out /* nullable, host: n_groups * (max_models + 1) */,
                                 uint64_t *offsets_out /* nullable, host: n_groups + 1 */);
LSQR_API int lsqr_refine_grouped(lsqr_ctx *ctx, const int32_t *groups, size_t n_groups, int on_device,
                                 double *params_inout /* host, n_groups * max_models * lsqr_num_params */,
                                 const size_t *n_models, size_t max_models, size_t max_rounds,
                                 int32_t *labels_out /* nullable */, uint64_t *counts_out /* nullable */,
                                 uint64_t *offsets_out /* nullable */,
                                 lsqr_fit_info *fits /* host, n_groups * max_models */,
                                 int32_t *status_out /* host, n_groups * max_models */,
                                 size_t *rounds_out /* host, n_groups */,
                                 int32_t *converged_out /* host, n_groups */);
/* ---- lsqr_refine_grouped for the geometric sphere: LM fits per group on the device (csrc/assign_lm_grouped.h) ------
 * lsqr_refine_lm_grouped is lsqr_refine_grouped -- its arguments and their shapes, on_device, the groups' rules, each
 * group's own loop and stop, what does not run, counts_out / offsets_out, the order of its checks, "every argument error
 * writes nothing" -- for the one model lsqr_refine_grouped refuses, with lsqr_refine_lm's refit.
 *   Models: LSQR_MODEL_SPHERE with LSQR_LS_GEOMETRIC in every dimension lsqr_set_model accepts (2..8).  Every other
 *     model, the algebraic sphere included, returns LSQR_ERR_INVALID and writes nothing: lsqr_refine_grouped takes the
 *     fits in closed form.
 *   Contract: group g -- the records with groups[i] == g, in upload order, with rows g * max_models .. + n_models[g] --
 *     is decided bit for bit as lsqr_refine_lm decides it on a fresh context with the same model and options that
 *     holds the stable gather of group g's records, tightly packed, with the same max_rounds.  Bit-identical per
 *     group: labels_out (the model index inside the group, or -1) and the counts; the returned parameters and
 *     status_out; every field of fits[] (n_params, lm_info, lm_nfev, reserved: the stall evaluation, n_used, cost);
 *     rounds_out[g] and converged_out[g].  A model whose run gives no result (too few records, no algebraic start,
 *     lm_info outside 1..4) keeps the row it had before the round; the algebraic intermediate never comes back.
 *   Groups that run nothing, records in no group and rows m >= n_models[g] behave as lsqr_refine_grouped documents
 *     them: -1 labels, LSQR_ERR_STATE with a zeroed fit, untouched rows.  max_rounds == 0 is lsqr_assign_grouped, and
 *     the returned labels are always exactly the grouped assignment of the returned parameters.
 *   An evaluation is one pass over the packed records of the groups still going, for all their live models at once,
 *     one step launch and one 4-byte read for all groups together; a refit round lasts as many evaluations as its
 *     slowest model needs.  Nothing is summed with a floating-point atomic: a group's results do not depend on the
 *     other groups of the call, on how the ids are numbered, or on the run.
 *   The context's upload, hypotheses, mask, spatial index and the parameters of its last mask are left as they were
 *     (as lsqr_refine_grouped leaves them); the work runs on the context's stream, and the call returns after it has
 *     finished.  The options lm_persist and lm_host do not apply.  lsqr_multi handles have no such form. */
LSQR_API int lsqr_refine_lm_grouped(lsqr_ctx *ctx, const int32_t *groups, size_t n_groups, int on_device,
                                    double *params_inout /* host, n_groups * max_models * lsqr_num_params */,
                                    const size_t *n_models, size_t max_models, size_t max_rounds,
                                    int32_t *labels_out /* nullable */, uint64_t *counts_out /* nullable */,
                                    uint64_t *offsets_out /* nullable */,
                                    lsqr_fit_info *fits /* host, n_groups * max_models */,
                                    int32_t *status_out /* host, n_groups * max_models */,
                                    size_t *rounds_out /* host, n_groups */,
                                    int32_t *converged_out /* host, n_groups */);
/* ---- lsqr_assign_grouped / lsqr_refine_grouped for the dense linear system (csrc/assign_dense_grouped.h) ----------
 * lsqr_assign_dense_grouped / lsqr_refine_dense_grouped are lsqr_assign_grouped / lsqr_refine_grouped -- their
 * arguments and their shapes, on_device, the groups' rules, each group's own loop and stop, what does not run,
 * counts_out / offsets_out, max_models == 0, "every entry of labels_out is written exactly once", the order of their
 * checks, "every argument error writes nothing", what is left untouched on the context, the stream -- for the model
 * they refuse, with lsqr_refine_dense's refit.  They finish lsqr_ransac_grouped_sequential on this model, and take
 * n up to 64 whatever that call's record limit is.
 *   Model: LSQR_MODEL_DENSE, dim n = 1..64, any stride, from lsqr_upload or lsqr_attach; a parameter row is n
 *     doubles.  Every other model returns LSQR_ERR_INVALID and writes nothing: lsqr_assign_grouped /
 *     lsqr_refine_grouped take the plane, line, sphere and 2-D line.
 *   Contract: group g -- the rows with groups[i] == g, in upload order, with parameter rows g * max_models .. +
 *     n_models[g] -- is decided bit for bit as lsqr_assign_dense / lsqr_refine_dense decide it on a fresh context with
 *     the same model and options (dense_fast_solve, dense_dd) that holds the stable gather of group g's rows, tightly
 *     packed, with the same max_rounds.  Bit-identical per group: labels_out (the model index inside the group, or
 *     -1), residuals_out, the counts; the returned parameters, status_out, fits[].n_used, fits[].n_params and
 *     fits[].reserved (the route 0 / 1 / 2), rounds_out[g] and converged_out[g].
 *   Sums: lsqr_refine_dense's order with the chunks (256 rows up to n = 32, 128 above) counted inside the group's
 *     packed rows; none is a floating-point atomic, so a group's results do not depend on the other groups of the
 *     call, on how the ids are numbered, or on the run.  The double-double solve of a flagged (group, model) pair
 *     runs over that group's packed rows alone, as the fresh context's does.
 *   Per round the host waits once and reads two words: the groups still going and the flagged pairs; the list of
 *     flagged pairs crosses only when there is one.
 *   Device scratch of a refine call: sum over the groups of ceil(rows_g / chunk) * n_models[g] * ((n+1)(n+2)/2 + 1,
 *     rounded up to 8) doubles of partial blocks; that many doubles once more and a 544-byte result block per (group,
 *     model) pair; two packed label arrays; one word per (group, chunk); with dense_dd and a flagged pair one byte per
 *     packed row and 9 MiB.  If it cannot be allocated the call returns LSQR_ERR_HIP with the allocation in
 *     lsqr_last_error; there is no other path.  lsqr_multi handles have no such form. */
LSQR_API int lsqr_assign_dense_grouped(lsqr_ctx *ctx, const int32_t *groups /* lsqr_count(ctx), upload order */,
                                       size_t n_groups, int on_device,
                                       const double *params /* host, n_groups * max_models * n */,
                                       const size_t *n_models /* host, n_groups; each <= max_models */,
                                       size_t max_models /* <= 64 */,
                                       int32_t *labels_out /* lsqr_count(ctx) entries, upload order */,
                                       double *residuals_out /* nullable */,
                                       uint64_t *counts_out /* nullable, host: n_groups * (max_models + 1) */,
                                       uint64_t *offsets_out /* nullable, host: n_groups + 1 */);
LSQR_API int lsqr_refine_dense_grouped(lsqr_ctx *ctx, const int32_t *groups, size_t n_groups, int on_device,
                                       double *params_inout /* host, n_groups * max_models * n */,
                                       const size_t *n_models, size_t max_models, size_t max_rounds,
                                       int32_t *labels_out /* nullable */, uint64_t *counts_out /* nullable */,
                                       uint64_t *offsets_out /* nullable */,
                                       lsqr_fit_info *fits /* host, n_groups * max_models */,
                                       int32_t *status_out /* host, n_groups * max_models */,
                                       size_t *rounds_out /* host, n_groups */,
                                       int32_t *converged_out /* host, n_groups */);
/* Many independent RANSAC<T,S>::compute() problems (probabilistic overload, RANSAC.h:75-79) in one call.
 * Problem j is records [offsets[j], offsets[j+1]) of host_records (stride_bytes apart, laid out as for
 * lsqr_upload), walks sampler stream seeds[j] and is decided exactly as lsqr_ransac(ctx, p, seeds[j], NULL, 0, ...)
 * would decide it on those records alone.
 *   Models, taken from the context's lsqr_set_model (none set: LSQR_ERR_STATE):
 *     accepted: LSQR_MODEL_PLANE, LSQR_MODEL_LINE and LSQR_MODEL_SPHERE with ls_type = LSQR_LS_ALGEBRAIC, in every
 *       dimension lsqr_set_model accepts for them; LSQR_MODEL_ABSOR (ls_type 0, or 2: weighted, records of 7
 *       doubles), LSQR_MODEL_PIVOT (Frame records of 13 slots), LSQR_MODEL_RAY (with its aux minimum angle) and
 *       LSQR_MODEL_LINE2D.  Records are lsqr_record_doubles(cfg) wide, as for lsqr_upload.
 *     refused with LSQR_ERR_INVALID for the call: LSQR_MODEL_DENSE, LSQR_MODEL_US_SINGLE, LSQR_MODEL_US_POINTER,
 *       LSQR_MODEL_PHANTOM and the geometric (LM) sphere.
 *   Per-problem outcome in status_out[j]: N_j < k -> LSQR_ERR_INVALID (info zeroed, fraction 0, params untouched,
 *     RANSAC.hxx:16-19); no valid hypothesis or a failed fit -> LSQR_EMPTY (params untouched); else LSQR_OK with
 *     params_out[j * lsqr_num_params .. + lsqr_num_params) written.
 *   Bad arguments (offsets[0] != 0 or decreasing, a problem of more than 2^32 - 16 records, p outside (0, 1), a null
 *     required pointer, stride_bytes below the record) return LSQR_ERR_INVALID and write nothing.  n_problems == 0
 *     is a no-op returning LSQR_OK.  Otherwise the call returns LSQR_OK.
 *   Bit-identical to that lsqr_ransac call: status, iterations, best_index, best_votes, fraction, n_params,
 *     fit.n_used and the consensus bytes (consensus_out, nullable: offsets[n_problems] bytes in record order;
 *     0 for every record of a problem without a winner).  The parameters agree up to the order of the fp64 sums of
 *     the final fit.  info.evaluated depends on the batch schedule.  The options max_iterations and the 2^22
 *     no-model safety stop of lsqr_ransac apply per problem.
 *   Independence: problem j's results, parameters included, are bit-identical whichever other problems share the
 *     call, in whatever order, and however the rounds are cut (option "many_round_hypotheses": hypotheses per round,
 *     0 = default 2^21; a problem whose batch alone exceeds it gets a round of its own).
 *   The context's own upload, hypotheses and mask are not touched; the work runs on the context's current stream
 *   (lsqr_set_stream).  lsqr_multi handles have no batched form: call it on one device's context. */
LSQR_API int lsqr_ransac_many(lsqr_ctx *ctx, const void *host_records, size_t stride_bytes,
                              const uint64_t *offsets /* n_problems + 1, offsets[0] == 0, non-decreasing */,
                              size_t n_problems, double p, const uint64_t *seeds /* n_problems */,
                              double *params_out      /* n_problems * lsqr_num_params */,
                              uint8_t *consensus_out  /* nullable: offsets[n_problems] bytes, record order */,
                              lsqr_ransac_info *infos /* n_problems */,
                              int32_t *status_out     /* n_problems: LSQR_OK / LSQR_EMPTY / LSQR_ERR_INVALID */);
/* RANSAC<T,S>::compute() with an iterative (Levenberg-Marquardt) final fit, many problems in one call.  Same
 * arguments and per-problem contract as lsqr_ransac_many; models: the geometric sphere (LSQR_MODEL_SPHERE with
 * ls_type LSQR_LS_GEOMETRIC), dim 2..8.  Any other model returns LSQR_ERR_INVALID and writes nothing (the closed-form
 * fits are batched by lsqr_ransac_many).
 *   Problem j against lsqr_ransac(ctx, p, seeds[j], NULL, 0, ...) on a geometric-sphere context holding its records
 *     alone: bit-identical status, iterations, best_index, best_votes, fraction, consensus bytes and fit.n_used; the
 *     parameters and fit.cost agree within the LM tolerances (only the fp64 summation order of the moment blocks
 *     differs), fit.lm_info, fit.lm_nfev and fit.reserved (stall) are those of the batched LM run.
 *   LSQR_EMPTY when there is no winner, the algebraic start fails (then fit.lm_info = 0) or the LM run ends with
 *     fit.lm_info outside 1..4 (then n_params = 0 and the parameters are untouched), as on the single path.
 *   Independence as for lsqr_ransac_many, carried through the LM: problem j's results, parameters and lm_nfev
 *     included, are bit-identical whatever the other problems, their order, or "many_round_hypotheses". */
LSQR_API int lsqr_ransac_many_lm(lsqr_ctx *ctx, const void *host_records, size_t stride_bytes,
                                 const uint64_t *offsets, size_t n_problems, double p, const uint64_t *seeds,
                                 double *params_out, uint8_t *consensus_out, lsqr_ransac_info *infos,
                                 int32_t *status_out);
/* SphereParametersEstimator::geometricLeastSquaresEstimate over many record sets: set j is records
 * [offsets[j], offsets[j+1]) (laid out as for lsqr_ransac_many) restricted to masks (nullable: all records;
 * else offsets[n_sets] bytes, record order), started at x0 + j * lsqr_num_params.  Geometric sphere only, as
 * lsqr_ransac_many_lm.  Per set, as lsqr_upload + lsqr_set_mask + lsqr_lm_begin / lsqr_lm_step within the LM
 * tolerances: status_out[j] LSQR_OK (params_out[j * P ..] written) or LSQR_EMPTY (lm_info outside 1..4, parameters
 * untouched); fits[j] carries n_params, lm_info, lm_nfev, reserved (the stall evaluation, as lsqr_ls_fit), cost and
 * n_used.  An empty set or mask: LSQR_ERR_INVALID for that set, its parameters and fit untouched.  Argument errors
 * as lsqr_ransac_many; the context's own upload is not touched; the work runs on the context's stream. */
LSQR_API int lsqr_lm_fit_many(lsqr_ctx *ctx, const void *host_records, size_t stride_bytes,
                              const uint64_t *offsets, size_t n_sets, const uint8_t *masks, const double *x0,
                              double *params_out, lsqr_fit_info *fits, int32_t *status_out);
/* DenseLinearEquationSystemParametersEstimator<double,n> (robust linear regression), many problems in one call.
 * Same arguments and per-problem contract as lsqr_ransac_many; model: LSQR_MODEL_DENSE only, dim 1..64, records of
 * n + 1 doubles (AugmentedRow: a[0..n), b).  Any other model returns LSQR_ERR_INVALID and writes nothing
 * (lsqr_ransac_many and lsqr_ransac_many_lm keep refusing the dense model).
 *   Problem j against lsqr_ransac(ctx, p, seeds[j], NULL, 0, ...) on a dense context holding its records alone:
 *     bit-identical status, iterations, best_index, best_votes, fraction, fit.n_used and consensus bytes (the
 *     minimal solves are the single path's elimination / SVD pseudo-inverse, the votes its exact running sum); the
 *     parameters agree up to the fp64 summation order of the final fit's normal equations.  fit.reserved = 1 when
 *     the finish took the double-double route (a pivot below 1e-6 max|A^T A|: the system is solved again from its
 *     consensus rows, as lsqr_ransac does), else 0; with option "dense_dd" 0 the block's pseudo-inverse decides and
 *     reserved is 2 where lsqr_ransac reports 2.  Options "dense_fast_solve", "dense_dd", "max_iterations" and the
 *     2^22 no-model stop apply per problem as in lsqr_ransac.
 *   Independence as for lsqr_ransac_many: problem j's results, parameters included, are bit-identical whatever the
 *     other problems, their order, or "many_round_hypotheses".  Its default (0) here is the number of hypotheses
 *     whose rows (n padded to 8 / 16 / 32 / 64 doubles), subsets and flags fit in 256 MiB, at most 2^21: 2^21 up
 *     to n = 8, 1.3 to 1.5 million at n = 9..16, 343 000 at n = 64.
 *   The context's own upload, hypotheses and mask are not touched; the work runs on the context's stream. */
LSQR_API int lsqr_ransac_many_dense(lsqr_ctx *ctx, const void *host_records, size_t stride_bytes,
                                    const uint64_t *offsets, size_t n_problems, double p, const uint64_t *seeds,
                                    double *params_out, uint8_t *consensus_out, lsqr_ransac_info *infos,
                                    int32_t *status_out);
/* DenseLinearEquationSystemParametersEstimator::leastSquaresEstimate over many row sets: set j is records
 * [offsets[j], offsets[j+1]) (laid out as for lsqr_ransac_many_dense) restricted to masks (nullable: all records;
 * else offsets[n_sets] bytes, record order).  Dense model only, as lsqr_ransac_many_dense.  Per set, as lsqr_upload +
 * lsqr_set_mask + lsqr_ls_fit within fp64 summation order: status_out[j] LSQR_OK (params_out[j * n ..] written) or
 * LSQR_EMPTY (rank deficient, parameters untouched); fits[j] carries n_params, reserved (as lsqr_ls_fit: 1 = the
 * double-double route) and n_used (the set's rows in use).  An empty set or mask: LSQR_ERR_INVALID for that set, its
 * parameters and fit untouched.  Argument errors as lsqr_ransac_many; the context's own upload is not touched. */
LSQR_API int lsqr_dense_fit_many(lsqr_ctx *ctx, const void *host_records, size_t stride_bytes,
                                 const uint64_t *offsets, size_t n_sets, const uint8_t *masks /* nullable */,
                                 double *params_out, lsqr_fit_info *fits, int32_t *status_out);
/* Many independent RANSAC<T,S>::compute() problems of the EXHAUSTIVE overload (RANSAC.h:111-113, RANSAC.hxx:150-249:
 * every k-subset in lexicographic order, the first maximum wins) in one call: no p, no seeds, deterministic.
 * Arguments, record layout, argument errors (LSQR_ERR_INVALID, nothing written; n_problems == 0 is a no-op returning
 * LSQR_OK) and the rule "the context's own upload, hypotheses and mask are not touched; the work runs on the context's
 * stream" are lsqr_ransac_many's.
 *   Models: every model lsqr_ransac_many accepts, and the geometric sphere (LSQR_LS_GEOMETRIC), whose winners get the
 *     batched Levenberg-Marquardt stage of lsqr_ransac_many_lm after the algebraic finish.  LSQR_MODEL_DENSE,
 *     LSQR_MODEL_US_SINGLE, LSQR_MODEL_US_POINTER and LSQR_MODEL_PHANTOM return LSQR_ERR_INVALID and write nothing.
 *   Problem j is decided as lsqr_ransac_exhaustive decides it on a context holding its records alone:
 *     N_j < k -> status_out[j] = LSQR_EMPTY, info zeroed, parameters untouched (RANSAC.hxx:165-169; NOT the
 *       probabilistic overload's LSQR_ERR_INVALID);
 *     C(N_j, k) not representable in 64 bits -> status_out[j] = LSQR_ERR_INVALID, info zeroed, parameters untouched,
 *       the other problems unaffected;
 *     no valid hypothesis with at least one vote, or a failed fit (the geometric sphere: fit.lm_info outside 1..4)
 *       -> LSQR_EMPTY, parameters untouched; else LSQR_OK.
 *   Bit-identical to that call: status, iterations (= evaluated = C(N_j, k)), best_index (the winner's lexicographic
 *     rank: lsqr_comb_unrank turns it back into the subset), best_votes, fraction, n_params, fit.n_used and the
 *     consensus bytes (0 for every record of a problem without a winner).  Closed-form parameters agree up to the order
 *     of the fp64 sums of the final fit; the geometric sphere's parameters and fit.cost within the LM tolerances, as for
 *     lsqr_ransac_many_lm.  The option max_iterations does not apply, as in lsqr_ransac_exhaustive.
 *   Independence: problem j's results, parameters included, are bit-identical whichever other problems share the
 *     call, in whatever order, however "many_round_hypotheses" cuts the rounds, and whichever device path runs: a
 *     problem of at most 256 records and at most 65536 subsets is searched by one workgroup in one launch shared by
 *     all such problems; every other problem in rounds of at most "many_round_hypotheses" hypotheses (0 = default
 *     2^21, at most 2^30; a problem with more subsets spans several rounds).  Option "many_exhaustive_fused" 0 sends
 *     every problem through the rounds (default 1). */
LSQR_API int lsqr_ransac_many_exhaustive(lsqr_ctx *ctx, const void *host_records, size_t stride_bytes,
                                         const uint64_t *offsets, size_t n_problems, double *params_out,
                                         uint8_t *consensus_out /* nullable */, lsqr_ransac_info *infos,
                                         int32_t *status_out);
/* Host only (no context, no device).  lsqr_comb_count: C(n, k) exactly; LSQR_ERR_INVALID when k < 1, k > 64 or the
 * value does not fit in 64 bits (k > n: 0).  lsqr_comb_unrank: the rank-th k-subset of {0..n-1} in the order of the
 * exhaustive overload (computeAllChoices, RANSAC.hxx:197-213: lexicographic, increasing indices), k values in
 * subset_out; LSQR_ERR_INVALID when k < 1, k > 64, n > 2^32, C(n, k) does not fit or rank >= C(n, k). */
LSQR_API int lsqr_comb_count(uint64_t n, int k, uint64_t *count_out);
LSQR_API int lsqr_comb_unrank(uint64_t n, int k, uint64_t rank, uint32_t *subset_out);
/* One fixed-size batch of the same loop without the adaptive stopping rule: hypotheses
 * [first_index, first_index + H) of the sampler stream `seed` are solved and scanned, the first
 * hypothesis with the maximal vote count wins (the strict '>' of RANSAC.hxx:100), its consensus set
 * (RANSAC.hxx:129-137) is fitted (leastSquaresEstimate, :138).  All device work is chained on the
 * context's stream; the host synchronises once.  info->iterations = H, info->best_index is the
 * stream index of the winner.  Returns LSQR_EMPTY when no hypothesis was valid or the fit failed. */
LSQR_API int lsqr_batch_fit(lsqr_ctx *ctx, uint64_t seed, uint64_t first_index, size_t H,
                            double *params_out, uint8_t *consensus_out, lsqr_ransac_info *info);
/* lsqr_batch_fit split in two for pipelining: _enqueue chains the whole batch (sample .. fit and the copies
 * of the results into a pinned slot) and returns without waiting; _wait blocks on that slot's event and returns
 * what lsqr_batch_fit returns (no consensus copy: read it with lsqr_mask_* before the slot's lane gets its next
 * batch if it is needed).  The next batches can be enqueued before the previous ones are read: the host's latency
 * between steps disappears behind the device's work.
 * Slots and lanes: the context runs L = option "batch_lanes" (1..4, default 4) LANES -- HIP streams with their own
 * hypothesis / vote / mask buffers and their own spatial index, all reading the context's records -- and has 2 L
 * slots: slot s is batch depth s / L (0 or 1) of lane s % L.  Batches on one lane execute in order; batches on
 * different lanes OVERLAP on the device, which fills the time the dozen one-workgroup kernels of a batch (selection,
 * winner, solve) and the tails of the large ones leave the chip idle: plane, 10 M points, 4096 hypotheses per
 * batch: 0.81 ms per batch on one lane, 0.64 on two, 0.56 on four.  A caller that only uses slots 0 and 1 gets two
 * lanes.  Results do not depend on the number of lanes (tests/test_gpu_parity.py::test_batch_lanes_*).  Replacing the
 * records or the model (lsqr_upload / lsqr_attach / lsqr_set_model) waits for the lanes and voids unread slots.
 * Closed-form fits only (LSQR_ERR_INVALID for the iterative fits and the plane phantom, whose final fit keeps the
 * host in the loop). */
LSQR_API int lsqr_batch_fit_enqueue(lsqr_ctx *ctx, uint64_t seed, uint64_t first_index, size_t H, int slot);
LSQR_API int lsqr_batch_fit_wait(lsqr_ctx *ctx, int slot, double *params_out, lsqr_ransac_info *info);
/* ---- multi-GPU step with device-resident exchange buffers ------------------------------------------
 * One rank's part of a step of `world` x H hypotheses, all device work chained on the context's stream and
 * ONE host synchronisation (lsqr_step_finish); the two exchanges are collectives on the caller's device
 * buffers between the calls (RCCL: all-reduce MAX of packed_dev[0] as int64, all-reduce SUM of block_dev):
 *   lsqr_step_scan    hypotheses [first, first + H) of the stream: sample, solve, scan; packed_dev[0] =
 *                     (votes << 32) | (0xFFFFFFFF - (index_base + index)) of the first best one, 0 if none
 *   lsqr_step_winner  the winner (stream index batch_first + in-batch index taken from packed_dev) is
 *                     re-derived on the device, its consensus mask taken over observations [begin, end)
 *                     and block_dev[0 .. len) = phase-0 moment block of the slice, block_dev[len] = its
 *                     inlier count (len = lsqr_moments_len(cfg, 0))
 *   lsqr_step_finish  final fit from the (summed) block; winner_out: the winner's lsqr_num_params
 *                     parameters; info->best_votes / best_index (in-batch index) from packed_dev,
 *                     info->evaluated = 1 when the batch had a valid hypothesis (else 0),
 *                     info->fit.n_used = the summed count.  LSQR_EMPTY: no valid hypothesis / fit failed.
 * Host synchronisations of a step: lsqr_step_finish / _wait is the one every model has.  The dense system and the
 * US / plane-phantom calibrations add ONE inside lsqr_step_scan: their matrix-core filters decide the band of every
 * batch from per-workgroup worklists, and the host reads the fullest segment's fill right after the scan so that an
 * overflow (never seen) re-runs it on the exact kernels before the winner is packed -- the packed winner feeds a
 * collective and cannot be taken back afterwards.  lsqr_batch_fit_enqueue, whose results stay local until
 * lsqr_batch_fit_wait, defers that check to the wait and never blocks (r05).
 * lsqr_set_stream(external = 1) makes the context enqueue on the caller's HIP stream (the stream the
 * collectives are ordered with, e.g. torch's current stream; NULL = the default stream); external = 0
 * restores the context's own (non-blocking) stream. */
LSQR_API int lsqr_set_stream(lsqr_ctx *ctx, void *hip_stream, int external);
LSQR_API int lsqr_step_scan(lsqr_ctx *ctx, uint64_t seed, uint64_t first, size_t H, uint32_t index_base,
                            uint64_t *packed_dev);
LSQR_API int lsqr_step_winner(lsqr_ctx *ctx, uint64_t seed, uint64_t batch_first,
                              const uint64_t *packed_dev, size_t begin, size_t end, double *block_dev);
LSQR_API int lsqr_step_finish(lsqr_ctx *ctx, const uint64_t *packed_dev, const double *block_dev,
                              double *winner_out, double *params_out, lsqr_ransac_info *info);
/* lsqr_step_finish in two halves (as lsqr_batch_fit_enqueue / _wait): the solve and the copies of the step's
 * results into pinned slot `slot` (0 or 1) are enqueued, the next step can be enqueued on the same exchange
 * buffers (stream order keeps this step's copies ahead of the next step's writes), and _wait blocks on the
 * slot's event.  The phantom's host-side solve runs in _wait and uses one staging area: do not pipeline it. */
LSQR_API int lsqr_step_finish_enqueue(lsqr_ctx *ctx, const uint64_t *packed_dev, const double *block_dev,
                                      int slot);
LSQR_API int lsqr_step_finish_wait(lsqr_ctx *ctx, int slot, double *winner_out, double *params_out,
                                   lsqr_ransac_info *info);
/* ---- several devices from one process ------------------------------------------------------------------
 * north_star: "hypothesis batches shard trivially across the 8 GPUs of one node".  One lsqr_ctx per entry of
 * `devices` (an entry may repeat: several contexts on one device -- the tests run two on the box's one GPU).
 * Observations are uploaded to the first device once and replicated device-to-device (peer copies: xGMI inside a
 * node); a batch of n * H hypotheses is scanned in n contiguous slices; the earliest best hypothesis is picked by
 * a max over the packed (votes, ~index) words and its consensus mask + moment block are taken slice-wise and
 * summed in rank order -- both exchanges are peer copies into the first device's gather area (8 B and <= 17 KB:
 * latency-bound either way) followed by a reduction kernel there; between PROCESSES (bench.py --gpus N, one rank
 * per GPU) the same two exchanges are RCCL all-reduces.  Results: winner, consensus set and iteration count equal
 * the single-device entry points bit for bit; the final fit agrees to rounding (different summation tree). */
typedef struct lsqr_multi lsqr_multi;
LSQR_API int lsqr_multi_create(const int *devices, int n, lsqr_multi **out);
LSQR_API void lsqr_multi_destroy(lsqr_multi *m);
/* The transport of the handle's two exchanges: "peer-copy" (default: hipMemcpyPeerAsync into the first device's gather
 * area + a fixed-order reduction kernel there) or "rccl" (environment LSQR_MULTI_TRANSPORT=rccl at lsqr_multi_create:
 * one RCCL communicator per device -- ncclCommInitAll; librccl is dlopen'ed --, the winner as ncclAllReduce MAX of the
 * packed 64-bit word, the moment blocks as ncclAllReduce SUM on fixed buffers, each on its context's stream; needs
 * DISTINCT devices, lsqr_multi_create fails with LSQR_ERR_INVALID otherwise).  *bringup_seconds (nullable): what
 * creating and proving the communicators took. */
LSQR_API const char *lsqr_multi_transport(const lsqr_multi *m, double *bringup_seconds);
LSQR_API int lsqr_multi_size(const lsqr_multi *m);
LSQR_API lsqr_ctx *lsqr_multi_ctx(lsqr_multi *m, int rank); /* per-device options / profiling */
LSQR_API const char *lsqr_multi_last_error(const lsqr_multi *m);
LSQR_API int lsqr_multi_set_model(lsqr_multi *m, const lsqr_model_cfg *cfg);
LSQR_API int lsqr_multi_upload(lsqr_multi *m, const void *host_records, size_t count, size_t stride_bytes);
/* lsqr_batch_fit over n devices: hypotheses [first, first + n * H_per_device) of the stream; info->best_index is
 * the stream index of the winner */
LSQR_API int lsqr_multi_batch_fit(lsqr_multi *m, uint64_t seed, uint64_t first_index, size_t H_per_device,
                                  double *params_out, uint8_t *consensus_out, lsqr_ransac_info *info);
/* lsqr_ransac (RANSAC<T,S>::compute, probabilistic overload) over n devices, device sampler stream `seed` */
LSQR_API int lsqr_multi_ransac(lsqr_multi *m, double p, uint64_t seed, double *params_out,
                               uint8_t *consensus_out, lsqr_ransac_info *info);

/* Exhaustive overload (RANSAC.h:111-113): all C(N,k) subsets in lexicographic order. */
LSQR_API int lsqr_ransac_exhaustive(lsqr_ctx *ctx, double *params_out, uint8_t *consensus_out,
                                    lsqr_ransac_info *info);
/* Host-side replay of RANSAC.hxx:79-112 over batch results (exposed for tests and for the
 * multi-GPU driver).  state is 6 uint64: {i, numTries, best_votes, best_index, has_best, done};
 * initialise with lsqr_replay_init.  Returns the number of batch entries consumed. */
LSQR_API int lsqr_replay_init(size_t n, int k, double p, uint64_t state[6]);
LSQR_API size_t lsqr_replay(size_t n, int k, double p, const uint32_t *subsets,
                            const uint8_t *valid, const uint32_t *votes, size_t H,
                            uint64_t base_index, void *dedup_set, uint64_t state[6]);
LSQR_API void *lsqr_dedup_create(int k);
LSQR_API void lsqr_dedup_destroy(void *set);

/* ---- tuning knobs (A/B measurements inside one process; defaults are the tuned values) --------- */
/* The complete list -- every name with its default, the values it accepts and one line on what it does -- is the table
 * in lsqrrecipes_amd/csrc/options.h; the options a caller is most likely to want are described at length here.
 * "scan_ppl": observations per lane in k_scan (2, 4 or 8; 0 = model default);
 * "scan_filter": 1 = cheap pre-filter with a proven error band + exact fp64 re-evaluation of the
 *                ambiguous observations (bit-identical votes): packed fp32 for plane / sphere / line
 *                and the US estimators, fp64 MFMA for the dense system; 0 = plain fp64 scan; 2 / 3 =
 *                as 1 with the re-evaluation forced per packed pair / per tile (US: 2 = the fused
 *                fp64 filter);
 * "upload_threads": host threads lsqr_upload uses to stage a large pageable buffer through pinned chunks
 *                while earlier chunks are already in flight (0 = one plain hipMemcpy: the default, measured
 *                faster on the MI355X box -- 56 GB/s; -1 = LSQR_UPLOAD_THREADS or 0);
 * "max_iterations": stop lsqr_ransac after this many loop iterations even if the adaptive bound
 *                asks for more (0 = the reference's behaviour: up to C(N,k));
 * "lm_persist": 1 (default) = an iterative US fit (SinglePointTarget...Estimator.cxx:272-329, :926-971) is ONE launch
 *               when this context is the only one of the process that has been fitting on the device lately: the
 *               workgroups stay resident, every evaluation's pass over the compacted consensus set, the sum of the block
 *               partials and the hand-over of the next trial point happen inside it (csrc/lm_persist.h), MINPACK's step
 *               runs on the host between tagged granules in pinned memory (measured r05: 26 against 30 us per
 *               evaluation); with several contexts fitting at once the launch path is taken (their passes overlap each
 *               other's host round trips: the better aggregate); 3 = the persistent kernel always; 2 = persistent with
 *               the step on the device too (no host in the loop at all: 230 us per step on one lane -- measured, kept
 *               for the record); 0 = two launches per evaluation (r02-r04).  Same iterates, lm_info and lm_nfev every way.  "lm_persist_wgs": resident workgroups (0 = the device's compute units divided
 *               by the contexts alive on it, at most four ways); "lm_persist_timeout_ms": bound of every wait inside
 *               the kernel (2000) -- when it expires the fit is run again on the launch path;
 * "lm_host": 1 (default) = the Levenberg-Marquardt control flow between device passes runs on the
 *                host, 0 = in a single-lane device kernel (same lm_core.h code either way);
 * "scan_index":  two-level scan of the point models over a spatial index of the observations
 *                (Morton-sorted copy, re-partitioned as a k-d tree inside runs of 8192 records, + one fp32 bounding
 *                box per cell of 256 / 512 observations, built on the device once per upload): 1 (default) = built
 *                when it pays -- the upload holds >= 65536 observations and >= 768 hypotheses have been scanned on
 *                it or are still announced by the adaptive bound (the build costs about as much as 700 exhaustive
 *                hypothesis scans) --,
 *                0 = never, 2 = always.  Votes are
 *                bit-identical either way;  "scan_cell": observations per cell (256 or 512; 0 = the
 *                model's default), "scan_cpt": cells per wave tile (1; 0 = default, also 1), "scan_block":
 *                256 threads per workgroup either way -- 256 = hypotheses broadcast by v_readlane, 257 = through LDS
 *                (0 = the model's choice), "scan_hsplit": hypothesis segments per tile (0..128; 0 = auto; A/B knobs).
 *                Any other value of these is refused with LSQR_ERR_INVALID;
 * "scan_bound":  1 (default) = the batch entry points (lsqr_batch_fit*, lsqr_step_scan, lsqr_ransac) over an indexed
 *                upload count only hypotheses that can still become the running maximum (an upper bound on every
 *                hypothesis' votes from the cell boxes, a few early candidates counted first); the others
 *                report 0 votes -- winner, consensus set and iteration count are unchanged (RANSAC.hxx:94 abandons
 *                exactly such hypotheses).  Dense system (n > 32) and US calibrations: the observations are scanned in
 *                chunks and a hypothesis stops being counted once it cannot win any more (lsqr_scan_work; it reports
 *                its partial count).  0 = every hypothesis is counted.  lsqr_scan always counts all;
 * "scan_refine": 1 (default) = the index build re-partitions every run of 8192 Morton-ordered records as a k-d tree
 *                (median splits along the widest extent; csrc/cells.h: k_refine_runs) so that cells are compact:
 *                15 % (plane) to 40 % (sphere) fewer (hypothesis, cell) pairs reach the second level of the scan;
 *                0 = plain Morton runs (A/B knob).  "scan_presorted": 1 = cells are runs of the UPLOAD order (experiments
 *                with other spatial orders: tools/ab_order_kd.py).  Votes are identical whatever the order;
 * "scan_kd_levels": k-d levels ABOVE those runs, each one radix sort of (segment, coordinate) pairs (default 7: runs of
 *               1 M records; 0 = the Morton order above the runs, as until r05).  5 - 12 % fewer surviving pairs for
 *               ~0.6 ms per level and 10 M records; built by the first scan after the upload has been asked to scan
 * "scan_kd_after" hypotheses (default 16384; 0 = with the first index) -- the first index of an upload keeps the
 *               cheaper order.  Votes do not depend on either.
 * "batch_lanes": streams (1..4, default 4) the slots of lsqr_batch_fit_enqueue / _wait are spread over (see there);
 * "scan_pairs":  plain (unbounded) scans of an indexed upload: 0 (default) = the model's measured choice (plane, batches
 *                of >= 1024: the statically balanced kernel of the bounded scan, k_scan_pairs; else k_scan_cells),
 *                1 = always k_scan_pairs, 2 = always k_scan_cells (A/B knob); "scan_pairs_waves": workgroups
 *                per CU of that kernel (0 = what fits); "scan_bound_merge": cells per box of the vote bounds
 *                (0 = default: 4 while >= 4096 boxes remain, 1 = the cells themselves, 2 / 4 / 8);
 * "dense_f32":   dense scan filter at n > 32: 2 (default) = fp16 matrix cores (two-way splits), 1 = fp32 matrix cores,
 *                hypothesis fragments prefetched through an LDS ring (global_load_lds) and the next tile of rows in
 *                registers, 0 = fp64 matrix cores.  Votes are identical (the band is decided exactly);
 * "dense_fast_solve": 1 (default) = the n x n minimal solves of the dense system use elimination with
 *                partial pivoting and only fall back to the SVD pseudo-inverse near the rank decision,
 *                0 = always the SVD pseudo-inverse (and, for the dense least-squares fit, always the double-double
 *                route below);
 * "dense_dd":    dense least-squares fit (leastSquaresEstimate, DenseLinear...Estimator.hxx:64-96): 1 (default) = when
 *                the elimination on the normal equations A^T A meets a pivot below 1e-6 max|A^T A| (cond(A) beyond
 *                ~1e3) the system is solved again FROM THE ROWS: augmented Gram matrix in double-double, its Cholesky
 *                factor (= R and Q^T b of A's QR decomposition) in double-double, x = pinv(R) z by a Jacobi SVD with
 *                the reference's ABSOLUTE rank threshold 2.2e-16 -- the singular values, rank decision and solution
 *                of the reference's SVD pseudo-inverse of A, to 1e-6 up to cond(A) ~ 1e10 (tests/test_gpu_dense_cond.py);
 *                0 = the pseudo-inverse of the Gram block with a relative rank test 1e-13 (what entry points that only
 *                hold the block -- lsqr_solve_moments, the multi-GPU sum -- always do);
 * "scan_axis":   plane in 3-D over an indexed upload: 1 (default) = every cell also gets the direction of least spread
 *                of its observations, which are re-sorted inside the cell along it, and the bounded scan ("scan_bound")
 *                takes upper AND lower vote bounds of its candidates by rank from that order (csrc/axis.h: no
 *                observation is evaluated; what is counted exactly shrinks from ~500 to ~170 of 4096 hypotheses at
 *                10 M points); 0 = box-population bounds and pilots only.  Results are identical either way;
 * "scan_hyp_order": plane in 3-D, full counts (scan_bound 0 / lsqr_scan) of 1024..4096 hypotheses over an indexed
 *                upload: 1 (default) = the batch is walked in the order of a Morton key of (normal direction, offset)
 *                so that the 64 hypotheses of a group miss the same cells (csrc/cells.h: k_plane_order); 0 = sampling
 *                order.  Votes are identical;
 * "scan_prepared": cell models whose per-hypothesis state does not depend on the cell (plane): 1 (default) = it is
 *                written once per batch (csrc/cells.h: k_prepare_hyps) and read back by the counted two-level scan; 0 = it
 *                is rebuilt for every (cell, group of 64 hypotheses) (A/B knob).  Votes are identical;
 * "scan_lean":   the counted two-level scan of the cell models (plane, sphere, line): 1 (default) = its counting pass
 *                runs a count-only form (csrc/cells.h: k_cells_bounds, BoundsForm::Count: survivor counts and nothing else) and,
 *                where the hypotheses are prepared (plane, "scan_prepared" 1), k_scan_pairs keeps its share arithmetic
 *                on the scalar unit, refills its one prepared hypothesis for the next group as soon as level 1 has
 *                read it and reads the pair loop's addends as stored; 0 = the general forms of both kernels (A/B knob).
 *                Votes are identical;
 * "scan_pack":   the lean counted scan of the prepared cell models (plane, 3-D and 2-D; "scan_prepared" 1 and
 *                "scan_lean" 1): 1 (default) = the counting pass stores level 1's 64-bit survivor mask of every (cell, group of 64
 *                hypotheses) instead of a count, and k_scan_pairs repeats level 1 on packed blocks of 64 consecutive
 *                survivors of a cell, gathered through a per-wave id list in LDS (csrc/cells.h: k_scan_pairs, PairsForm::Packed),
 *                instead of on every group of 64 that holds a survivor; 0 = per group (A/B knob).  Accepted values 0 and 1;
 *                without effect on other models and with either of the two other options 0.  Votes are identical;
 * "scan_recheck": the exact path of the 3-D plane's packed counted scan ("scan_pack" 1 with the LDS broadcast area, the
 *                default): a (hypothesis, cell) pair one of whose observations falls into the fp32 filter's band of
 *                uncertainty re-evaluates the fp64 predicate 1 (default) = for the observations in the band alone, each
 *                lane loading its own; 0 = for all observations of the cell (A/B knob).  Accepted values 0 and 1;
 *                without effect on other kernels.  Votes are identical;
 * "scan_slab":   the counting pass of the 3-D plane's packed counted scan ("scan_pack" 1) over an axis-sorted index
 *                ("scan_axis" 1, cells of 256 / 512): 1 (default) = a (hypothesis, cell) pair the box test keeps is
 *                dropped again when the cell's oriented slab -- its axis of least spread and the interval of its
 *                observations along it, built with the index (csrc/axis.h: k_cell_slabs) -- proves that no observation
 *                of the cell can agree (csrc/cells.h: PlaneCell::slab); 0 = the plain box-test masks (A/B knob).
 *                Accepted values 0 and 1; without effect on the 2-D plane, sphere, line, the non-packed forms and an
 *                index without axes.  Votes are identical.  "scan_slab_gate": 1..8 (default 3), the slab of a cell is
 *                tested only where its width is at most value / 4 of the box's extent along the axis (A/B knob; the
 *                index is rebuilt);
 * "scan_tiles":  the two-level scans (k_scan_pairs, k_scan_cells) open a cell 1 (default) = from fp32 tiles of the
 *                index: the cell's observations relative to its centre as packed fp32 pairs (and the sphere's |x'|^2),
 *                computed once behind the index build (csrc/cells.h: k_build_tiles; 12 bytes a record for plane and
 *                line in 3-D, 16 for the sphere) and bit for bit what a wave would have computed; 0 = from the fp64
 *                sorted copy, converted by every wave for every cell it opens.  Accepted values 0 and 1; keeps the
 *                index, and with 0 set before the index is built no tiles are built.  Read by the forms a default
 *                path reaches (plane: the packed counted forms, sphere and line: the general one, k_scan_cells; each
 *                with the model's default "scan_block"; not by the 3-D plane's k_scan_cells and "scan_recheck" 0 form
 *                over 512-record cells, which have no register for it); the exact fp64 paths keep reading the sorted
 *                copy.  Votes are identical;
 * "dense_mask_ring": LDS tile buffers per wave of the dense final fit's fused mask + normal-equations pass: 4 (default at
 *                n = 64) = one workgroup per CU with three tiles in flight, 2 = two workgroups per CU (A/B knob);
 * "mom_chunk":   records per workgroup of the mask / moment passes in units of 256 (0 = default: 4, wide US / phantom
 *                records 16; A/B knob -- the fixed-order sums, and with them the last bits of a fit, depend on it). */
LSQR_API int lsqr_set_option(lsqr_ctx *ctx, const char *name, int value);

/* State of the spatial index of the current upload ("scan_index"): out = {built (0/1), indexed
 * (finite) observations, cells, observations per cell}. */
LSQR_API int lsqr_index_info(const lsqr_ctx *ctx, uint64_t out[4]);

/* Debug: the fp32 tiles of the index ("scan_tiles") against the sorted copy.  Every cell is opened both ways on the
 * device (csrc/cells.h: cells_load, cells_load_tile) and the results are compared as bit patterns:
 * out = {observations per cell the tiles in place were built for (0: no tiles), cells, 32-bit words that differ,
 * bytes the tiles occupy}. */
LSQR_API int lsqr_scan_tiles_check(lsqr_ctx *ctx, uint64_t out[4]);

/* Work of the two-level scan for the CURRENT batch of hypotheses over the indexed upload: runs level 1 (the
 * cell-box test) alone.  out[0..7] = {surviving (hypothesis, cell) pairs of ALL hypotheses, (64-hypothesis group,
 * cell) level-1 evaluations of one pass over all hypotheses, cells, observations per cell, 1 if the batch was last
 * scanned by the bounded scan ("scan_bound"), its pilots, its second-pass hypotheses, surviving pairs of the
 * hypotheses it actually counted (= out[0] when not bounded)}; bound_out (nullable, H entries) receives per
 * hypothesis the summed population of its surviving cells: an upper bound on its votes.  LSQR_ERR_STATE when the
 * upload has no index.  Used by bench.py to price the scan against the instruction-issue roof. */
LSQR_API int lsqr_scan_workload(lsqr_ctx *ctx, uint32_t *bound_out, uint64_t out[8]);

/* Work of the LAST scan of the current batch for the models without a spatial index (dense system, US calibrations,
 * plane phantom).  The batch entry points (lsqr_batch_fit*, lsqr_step_scan, lsqr_ransac) scan the observations in
 * chunks and stop counting a hypothesis once  votes so far + observations still to come  cannot exceed a lower bound
 * of the running maximum at its index (option "scan_bound" 1, the batched form of RANSAC.hxx:94; csrc/earlyexit.h) --
 * winner, consensus set and iteration count are unchanged, an abandoned hypothesis reports its partial count.
 * out[0..5] = {1 if that path ran (0: every pair was evaluated), (observation, hypothesis) pairs handed to the scan
 * kernels, pairs of a full scan = H * N, candidates counted to the end first, hypotheses abandoned at the first
 * selection, hypotheses still alive after the last one}.  Used by bench.py to price the scan.
 * out[6..7]: when the last scan went through the counted two-level scan of the 3-D plane (k_scan_pairs), the
 * (hypothesis, cell) pairs that took the exact fp64 path because an observation fell into the fp32 filter's band, and
 * the observations that were in the band (counted by the per-value re-check, "scan_recheck" 1, only); 0 otherwise. */
LSQR_API int lsqr_scan_work(lsqr_ctx *ctx, uint64_t out[8]);

/* The table of the LAST counting launch of the counted two-level scan (k_scan_pairs' cost table; for the bounded scan
 * that is its second pass): out[0..3] = {(hypothesis, cell) pairs in the table -- what level 2 was handed, after the
 * slab test where it ran; lsqr_scan_workload keeps reporting the pairs of the box test alone --, 1 if the table holds
 * survivor masks ("scan_pack"), 1 if the slab test ran ("scan_slab"), cells x hypotheses of the launch}.
 * LSQR_ERR_STATE when the last scan did not go through that kernel. */
LSQR_API int lsqr_scan_pairs_counted(lsqr_ctx *ctx, uint64_t out[4]);

/* The LAST persistent Levenberg-Marquardt fit of this context (option "lm_persist"; csrc/lm_persist.h):
 * out[0..7] = {mode (1 / 3: MINPACK's step on the host between granules in pinned memory, 2: on the device), resident
 * workgroups, evaluations, end state (2: finished, 3: a bounded wait expired and the launch path took over), kernel
 * time in microseconds by the device's 100 MHz clock, fits of this context that fell back to the launch path, host
 * nanoseconds spent waiting for moment blocks, host nanoseconds spent in MINPACK's step (mode 1)}.
 * trace (nullable, 4 * trace_cap entries): per evaluation (the first 64) workgroup 0's clock in 10 ns ticks at
 * {own pass done, every workgroup arrived, partial blocks summed, step done / the host's reply in};
 * *trace_n = evaluations written.  Used by bench.py and tools/lm_persist_time.py. */
LSQR_API int lsqr_lm_persist_info(const lsqr_ctx *ctx, uint64_t out[8], uint64_t *trace, uint32_t trace_cap,
                                  uint32_t *trace_n);

/* ---- measurement ------------------------------------------------------------------------------ */
/* Per-kernel HIP-event timing on the context's stream.  kernel ids: 0 sample, 1 estimate,
 * 2 scan, 3 mask, 4 moments, 5 solve, 6 spatial-index build (once per upload), 7 the max-|coordinate| pass
 * of the fp32 filters (once per upload). */
LSQR_API int lsqr_profile_enable(lsqr_ctx *ctx, int on);
LSQR_API int lsqr_profile_get(lsqr_ctx *ctx, int kernel_id, uint64_t *launches, double *total_ms);
LSQR_API int lsqr_profile_reset(lsqr_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* LSQR_HIP_H */
