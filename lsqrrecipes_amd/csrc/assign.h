// assign.h -- lsqr_assign / lsqr_refine: every record of the context's upload goes to the NEAREST of up to 64 models it
// agrees with, and (refine) every model is fitted again on its own records, round after round, on the device.
//
// The decision for one record (assign_one; the kernel and lsqr_assign_host run the same code):
//   label(x) = the smallest m in [0, M) that minimises M::residual(row_m, x) among the m with M::agree(row_m, x);
//              -1 when no m agrees, and for a record with a non-finite coordinate.  Strict '<' while m walks upwards.
//   row_m is the scan row of the caller's parameters exactly as lsqr_mask makes one: zero-padded, then M::prepare.
//
// The grouped calls (assign_grouped.h: one model set per label) run the code of this file: assign_pass_chunk, the pass
// over one chunk, is the body of k_assign_moments and of k_asg_grp_pass, which only locate their chunk; assign_refit is
// what both solve kernels do with a model's summed moments; k_assign_prepare is launched by both drivers.
//
//   k_assign_prepare   one lane per row that is there: parameters -> scan rows
//   assign_pass_chunk  ONE pass over a chunk.  A workgroup of kBlock lanes takes the chunk's (at most) kAssignChunk
//                      consecutive records, kAssignPerLane per lane, and keeps them in registers.  The chunk's base is
//                      folded into the (uniform) pointers, so the record indices are 32-bit and local to the chunk.
//                      The M rows are read at wave-uniform addresses (scalar loads, the scalar cache serves every wave
//                      of the chip), row by row, each row against the lane's records.  The lane writes labels[i] (and
//                      residuals[i]); the workgroup counts labels[i] != old[i] and the records per model (ballots, LDS
//                      integer adds, then one 64-bit integer atomic per counter and workgroup).  WITH_MOMENTS: for
//                      every model m present in the chunk (one 64-bit presence mask per chunk) the phase-0 moment
//                      block of the records labelled m about model m's own point (fit_origin_offset), by
//                      AccLs<M>::acc, reduced as k_many_mask_moments reduces: the lane's records in index order, the
//                      __shfl_down tree, the four waves in index order; one barrier per model, the wave sums in two
//                      alternating LDS buffers; -> the chunk's partials [m][AccLs<M>::N].  A model absent from the
//                      chunk gets zeros.  It must be inlined: as a called function it keeps its arrays in memory.
//   k_assign_moments   chunk blockIdx.x of the upload: counters in the ASG_ words, partials[chunk][m][N]
//   assign_refit       lane 0, after a solve kernel's sum: solve_small<M> about the model's own point (the body of
//                      k_many_solve); a model with at least lsqr_min_subset records and a solve that succeeded gets
//                      its new scan row, any other keeps its row
//   assign_sum_chunks  a model's blocks summed in chunk order by one lane per moment (the four waves stage them
//                      through LDS): k_assign_solve's sum, and k_assign_lm_step's
//   k_assign_solve     one workgroup per model: assign_sum_chunks, then assign_refit
//
// assign_rounds<F> is the round loop of all eight ungrouped calls, written once; a family F says what differs -- its
// buffers, how parameters become scan rows and come back, which kernels make the pass, what the refit enqueues, its
// counter words and what it adds to a fit record.  AssignClosed<M> (here) is lsqr_assign's and lsqr_refine's.
// AssignLm<M> (assign_lm.h, the geometric sphere: lsqr_refine_lm) is AssignClosed<M> whose pass also stores every
// chunk's presence word, whose solve writes into a side array of start rows and whose refit is an LM stage.
// AssignDense<NR> (assign_dense.h) is the dense linear system's, with kernels of its own.  AssignRigid<M>
// (assign_rigid.h: absolute orientation, pivot, ray) is AssignClosed<M> with a chunk size of its own and, for the pass
// body and assign_refit, an origin that need not be the model's own point.
//
// Order of the sums: kAssignChunk fixes it, as kManyPart does for the batched finish.  Nothing is summed with a
// floating-point atomic, so two runs of one call give the same bits.
//
// Budget (launch bounds kBlock = 4 waves): records 8 x REC doubles, labels 8, residuals 8 doubles, one moment block
// (AccLs<M>::N <= 55 doubles) and its origin per lane -- the 3-D models take 84 .. 110 VGPRs (4 or 5 waves per SIMD), the
// 8-D ones 164 and more (1 to 3 waves per SIMD); no kernel spills.  LDS of the pass: two buffers of 4 x N doubles for
// the wave sums (3.4 KiB at N = 55), 64 counters, the four waves' presence masks -- under 4 KiB, no limit on occupancy.
// The 64 x 45 doubles of an 8-D plane's accumulators never exist at once: one model's block at a time lives in
// registers.  k_assign_solve: one tile of partials and SolveOut, 22 .. 62 KiB of LDS, one workgroup per model
// (DESIGN.md section 14).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "devbuf.h"
#include "host_entry.h"
#include "kernels.h"
#include "many.h"

namespace lsqr {

constexpr int kAssignMaxModels = 64;                        // one presence bit per model
constexpr int kAssignPerLane = 8;                           // records a lane keeps in registers
constexpr uint32_t kAssignChunk = kAssignPerLane * kBlock;  // records per workgroup (fixes the moment sums' order)

inline uint32_t assign_chunks(uint64_t n) { return (uint32_t)((n + kAssignChunk - 1) / kAssignChunk); }

// the models lsqr_assign takes: their parameters hold a point (fit_origin_offset >= 0)
template <class M> struct AssignModel { static constexpr bool value = false; };
template <int D> struct AssignModel<PlaneModel<D>> { static constexpr bool value = true; };
template <int D> struct AssignModel<LineModel<D>> { static constexpr bool value = true; };
template <int D> struct AssignModel<SphereModel<D>> { static constexpr bool value = true; };
template <int D> struct AssignModel<PlaneModelN<D>> { static constexpr bool value = true; };
template <int D> struct AssignModel<LineModelN<D>> { static constexpr bool value = true; };
template <int D> struct AssignModel<SphereModelN<D>> { static constexpr bool value = true; };
template <> struct AssignModel<Line2DModel> { static constexpr bool value = true; };  // [n, a]: a is its point

inline bool assign_model_ok(const lsqr_model_cfg &cfg) {
  return dispatch(cfg, [](auto tag) -> int {
           return AssignModel<typename decltype(tag)::type>::value ? LSQR_OK : LSQR_ERR_INVALID;
         }) == LSQR_OK;
}

// parameters -> scan row, as lsqr_mask makes one
template <class M>
LSQR_HD void assign_make_row(const double *params, const ModelConsts &mc, double *row) {
  for (int j = 0; j < (int)M::SP; j++) row[j] = j < (int)M::P ? params[j] : 0.0;
  M::prepare(row, mc);
}

template <class M>
LSQR_HD bool assign_finite(const double *x) {
  bool fin = true;
  for (int d = 0; d < (int)M::REC; d++) fin = fin && (x[d] - x[d] == 0.0);  // false for NaN and +-Inf
  return fin;
}

// model m against the record: the running (label, residual) of the walk m = 0, 1, ...
template <class M>
LSQR_HD void assign_step(const double *row, int32_t m, const double *x, const ModelConsts &mc, int32_t &label,
                         double &res) {
  if (M::agree(row, x, mc)) {
    const double r = M::residual(row, x, mc);
    if (r < res) {
      res = r;
      label = m;
    }
  }
}

// the decision for ONE record; rows: n_models scan rows of M::SP doubles.  -> label, *res_out (nullable) its residual
template <class M>
LSQR_HD int32_t assign_one(const double *rows, int n_models, const double *x, const ModelConsts &mc, double *res_out) {
  int32_t label = -1;
  double res = __builtin_inf();
  if (assign_finite<M>(x))
    for (int m = 0; m < n_models; m++) assign_step<M>(rows + (size_t)m * M::SP, m, x, mc, label, res);
  if (res_out) *res_out = res;
  return label;
}

// The models lsqr_assign_rigid / lsqr_refine_rigid take (assign_rigid.h): closed-form fits whose parameters hold no
// point to sum about.  A gate of its own: lsqr_assign, lsqr_refine and the grouped calls keep refusing them.
template <class M> struct AssignRigidModel { static constexpr bool value = false; };
template <> struct AssignRigidModel<AbsOrModel> { static constexpr bool value = true; };
template <> struct AssignRigidModel<PivotModel> { static constexpr bool value = true; };
template <> struct AssignRigidModel<RayModel> { static constexpr bool value = true; };

inline bool assign_rigid_model_ok(const lsqr_model_cfg &cfg) {
  // absolute orientation: records of 6 doubles (ls_type 0) or of 7 with a weight (ls_type 2), nothing else
  if (cfg.model == LSQR_MODEL_ABSOR && cfg.ls_type != 0 && cfg.ls_type != 2) return false;
  return dispatch(cfg, [](auto tag) -> int {
           return AssignRigidModel<typename decltype(tag)::type>::value ? LSQR_OK : LSQR_ERR_INVALID;
         }) == LSQR_OK;
}

// which models a single-record host call takes
enum AssignHostKind { ASSIGN_HOST_POINT, ASSIGN_HOST_DENSE, ASSIGN_HOST_RIGID };
template <AssignHostKind KIND, class M>
constexpr bool kAssignHostTakes = KIND == ASSIGN_HOST_DENSE   ? (bool)M::IS_DENSE
                                  : KIND == ASSIGN_HOST_RIGID ? AssignRigidModel<M>::value
                                                              : AssignModel<M>::value;

// lsqr_assign_host, (ASSIGN_HOST_DENSE) lsqr_assign_dense_host and (ASSIGN_HOST_RIGID) lsqr_assign_rigid_host: no
// context, no device.  DENSE takes the dense linear system alone, whose parameters are cfg->dim coefficients; its scan
// rows (assign_dense.h) are zero beyond them
template <AssignHostKind KIND>
int host_assign_host(const lsqr_model_cfg *cfg, const double *params, size_t n_models, const void *record,
                     int32_t *label_out, double *residual_out) {
  constexpr bool DENSE = KIND == ASSIGN_HOST_DENSE;
  if (!cfg || !cfg_supported(*cfg) ||
      !(DENSE ? cfg->model == LSQR_MODEL_DENSE
              : KIND == ASSIGN_HOST_RIGID ? assign_rigid_model_ok(*cfg) : assign_model_ok(*cfg)))
    return LSQR_ERR_INVALID;
  if (n_models == 0) return LSQR_OK;
  if (n_models > (size_t)kAssignMaxModels || !params || !record || !label_out) return LSQR_ERR_INVALID;
  ModelConsts mc;
  model_consts(*cfg, &mc);
  return dispatch(*cfg, [&](auto tag) -> int {
    typedef typename decltype(tag)::type M;
    if constexpr (kAssignHostTakes<KIND, M>) {
      const size_t p = DENSE ? (size_t)cfg->dim : (size_t)M::P;
      std::vector<double> rows(n_models * M::SP, 0.0);  // scan rows, as lsqr_mask makes one (assign_make_row)
      for (size_t m = 0; m < n_models; m++) {
        for (size_t j = 0; j < p; j++) rows[m * M::SP + j] = params[m * p + j];
        M::prepare(&rows[m * M::SP], mc);
      }
      double x[M::REC];
      M::load((const double *)record, mc, x);
      *label_out = assign_one<M>(rows.data(), (int)n_models, x, mc, residual_out);
      return LSQR_OK;
    } else {
      return LSQR_ERR_INVALID;
    }
  });
}

// the words of the call's device counters
enum {
  ASG_CHANGED = 0,                           // labels[i] != old[i]
  ASG_COUNT = 1,                             // records per model of the last pass
  ASG_USED = ASG_COUNT + kAssignMaxModels,   // records behind the last refit attempt
  ASG_OK = ASG_USED + kAssignMaxModels,      // 1: that refit gave the model a new row
  ASG_WORDS = ASG_OK + kAssignMaxModels
};

#if defined(__HIPCC__)
// v, the same in every lane of the wave, as a scalar: loops over its bits then stay on the scalar unit.  (The builtin
// returns int: each half goes back through uint32_t, or a set bit 31 -- model 31 -- would smear over bits 32 .. 63.)
__device__ __forceinline__ unsigned long long wave_uniform64(unsigned long long v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

// params: n_rows rows of M::P, row e of group e / max_models; nm (nullable: every row is there): the rows of each group
// that are there.  A row that is not there is never read and never written.
template <class M>
__global__ __launch_bounds__(kBlock) void k_assign_prepare(const double *__restrict__ params,
                                                           const int32_t *__restrict__ nm, uint64_t n_rows,
                                                           int max_models, ModelConsts mc, double *__restrict__ rows) {
  for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < n_rows; e += (uint64_t)gridDim.x * kBlock) {
    const uint64_t g = e / (uint32_t)max_models;
    if (nm && (int)(e - g * (uint32_t)max_models) >= nm[g]) continue;
    double p[M::P], row[M::SP];
    for (int j = 0; j < (int)M::P; j++) p[j] = params[e * M::P + j];
    assign_make_row<M>(p, mc, row);
    for (int j = 0; j < (int)M::SP; j++) rows[e * M::SP + j] = row[j];
  }
}

// The pass over ONE chunk, by one workgroup of kBlock lanes: the body of k_assign_moments and of k_asg_grp_pass.  The
// chunk's base is in the pointers, so its records are [0, n), n <= kAssignChunk, and every index is 32-bit.
// data: the chunk's records, `stride` doubles apart; rows: the n_models scan rows of the chunk's model set; labels /
// residuals (nullable) / old (nullable): the chunk's n entries; changed: the word that counts labels[i] != old[i];
// counts: one word per model; partials (WITH_MOMENTS): the chunk's [model][AccLs<M>::N]; presence (WITH_MOMENTS,
// nullable): the chunk's word for the mask of the models that own a record of the chunk.
// R: the records a lane keeps, so n <= R * kBlock (assign_rigid.h takes fewer of the pivot's wide frames); org_tab
// (nullable: null for every family but the rigid one): the origins [model][kAssignOrigin<M>] of the moment blocks,
// taken instead of the model's own point at rows[m][org_off ..]
template <class M> constexpr int kAssignOrigin = M::ND;  // the origin's doubles
template <> constexpr int kAssignOrigin<RayModel> = 3;   // (a ray's record is [p, n]: its origin is a point)
template <> constexpr int kAssignOrigin<PivotModel> = 0; // (PivotModel::accumulate reads none)

template <class M, bool WITH_MOMENTS, int R = kAssignPerLane>
__device__ __forceinline__ void assign_pass_chunk(const double *__restrict__ data, size_t stride, uint32_t n,
                                                  const double *__restrict__ rows, int n_models, int org_off,
                                                  const ModelConsts &mc, int32_t *__restrict__ labels,
                                                  double *__restrict__ residuals, const int32_t *__restrict__ old,
                                                  unsigned long long *__restrict__ changed,
                                                  unsigned long long *__restrict__ counts,
                                                  double *__restrict__ partials,
                                                  unsigned long long *__restrict__ presence,
                                                  const double *__restrict__ org_tab = nullptr) {
  typedef AccLs<M> A;
  static_assert(A::N <= 64, "one lane per moment");
  constexpr int W = kBlock / 64;
  __shared__ double s_m[2][W][WITH_MOMENTS ? (int)A::N : 1];
  __shared__ unsigned long long s_p[W];
  __shared__ uint32_t s_chg[W];
  __shared__ uint32_t s_cnt[kAssignMaxModels];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double qnan = __builtin_nan("");
  if (threadIdx.x < kAssignMaxModels) s_cnt[threadIdx.x] = 0;

  double x[R][M::REC], res[R];
  int32_t lab[R];
#pragma unroll
  for (int j = 0; j < R; j++) {
    const uint32_t i = (uint32_t)j * kBlock + threadIdx.x;
    const bool in = i < n;
    M::load(data + (size_t)(in ? i : 0) * stride, mc, x[j]);
    if (!in || !assign_finite<M>(x[j])) {
#pragma unroll
      for (int d = 0; d < (int)M::REC; d++) x[j][d] = qnan;  // NaN agrees with nothing
    }
    lab[j] = -1;
    res[j] = __builtin_inf();
  }
  for (int m = 0; m < n_models; m++) {
    const double *row = rows + (size_t)m * M::SP;  // wave-uniform: scalar loads
#pragma unroll
    for (int j = 0; j < R; j++) assign_step<M>(row, m, x[j], mc, lab[j], res[j]);
  }

  uint32_t chg = 0;
  unsigned long long pres = 0;
#pragma unroll
  for (int j = 0; j < R; j++) {
    const uint32_t i = (uint32_t)j * kBlock + threadIdx.x;
    if (i >= n) continue;
    labels[i] = lab[j];
    if (residuals) residuals[i] = res[j];
    if (old) chg += old[i] != lab[j] ? 1u : 0u;
    if (lab[j] >= 0) pres |= 1ull << lab[j];
  }
  for (int o = 32; o > 0; o >>= 1) {
    chg += __shfl_xor(chg, o);
    pres |= __shfl_xor(pres, o);
  }
  if (lane == 0) {
    s_p[wave] = pres;
    s_chg[wave] = chg;
  }
  __syncthreads();
  unsigned long long all = 0;
  for (int w = 0; w < W; w++) all |= s_p[w];
  // (uniform by construction; the scalar copies keep the model loop's control flow on the scalar unit)
  const unsigned long long present = wave_uniform64(all);
  const unsigned long long mine = wave_uniform64(pres);

  int it = 0;
  for (unsigned long long rest = present; rest; rest &= rest - 1, it++) {
    const int m = __builtin_ctzll(rest);
    const bool here = (mine >> m) & 1ull;  // this wave holds records of model m
    if (here) {
      uint32_t cnt = 0;
#pragma unroll
      for (int j = 0; j < R; j++) cnt += (uint32_t)__popcll(__ballot(lab[j] == m));
      if (lane == 0) atomicAdd(&s_cnt[m], cnt);
    }
    if constexpr (WITH_MOMENTS) {
      double(*buf)[A::N] = s_m[it & 1];
      if (here) {
        constexpr int NC = M::P > M::REC ? M::P : M::REC;
        double cv[NC], acc[A::N];
        const double *org = org_tab ? org_tab + (size_t)m * kAssignOrigin<M> : rows + (size_t)m * M::SP + org_off;
#pragma unroll
        for (int k = 0; k < NC; k++) cv[k] = k < kAssignOrigin<M> ? org[k] : 0.0;
#pragma unroll
        for (int k = 0; k < (int)A::N; k++) acc[k] = 0.0;
#pragma unroll
        for (int j = 0; j < R; j++)
          if (lab[j] == m) A::acc(x[j], cv, acc);
#pragma unroll
        for (int k = 0; k < (int)A::N; k++) {
          double v = acc[k];
          for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
          if (lane == 0) buf[wave][k] = v;
        }
      } else if (lane < (int)A::N) {
        buf[wave][lane] = 0.0;
      }
      // one barrier per model: the buffer written two models on is this one again, and no wave gets there before
      // every wave has passed the barrier in between, that is, after this model's sums have been read
      __syncthreads();
      if (threadIdx.x < A::N) {
        double t = 0.0;
        for (int w = 0; w < W; w++) t += buf[w][threadIdx.x];
        partials[(size_t)m * A::N + threadIdx.x] = t;
      }
    }
  }
  if constexpr (WITH_MOMENTS) {
    for (uint32_t e = threadIdx.x; e < (uint32_t)n_models * A::N; e += kBlock)
      if (!((present >> (e / A::N)) & 1ull)) partials[e] = 0.0;
    if (presence && threadIdx.x == 0) *presence = present;
  }
  __syncthreads();
  if ((int)threadIdx.x < n_models && s_cnt[threadIdx.x])
    atomicAdd(&counts[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < W; w++) t += s_chg[w];
    if (t) atomicAdd(changed, t);
  }
}

// The least waves per SIMD a pass kernel is compiled for.  Left alone, the scheduler settles the 4-D plane's pass with
// moments on 162 VGPRs (3 waves) where 126 do without scratch; no other instantiation is told anything
template <class M, bool WITH_MOMENTS> constexpr int kAssignPassWaves = 1;
template <> constexpr int kAssignPassWaves<PlaneModelN<4>, true> = 4;

// chunk blockIdx.x of the context's n records.  data: `stride` doubles apart; labels: n entries; residuals, old:
// nullable; counters: the ASG_ words, zeroed by the caller; partials (WITH_MOMENTS): [chunk][model][AccLs<M>::N];
// presence (WITH_MOMENTS, nullable): one word per chunk (the LM stage of assign_lm.h reads it)
template <class M, bool WITH_MOMENTS>
__global__ __launch_bounds__(kBlock, (kAssignPassWaves<M, WITH_MOMENTS>)) void k_assign_moments(
    const double *__restrict__ data, size_t stride, uint32_t n, const double *__restrict__ rows, int n_models,
    int org_off, ModelConsts mc, int32_t *__restrict__ labels, double *__restrict__ residuals,
    const int32_t *__restrict__ old, unsigned long long *__restrict__ counters, double *__restrict__ partials,
    unsigned long long *__restrict__ presence) {
  const uint32_t c0 = blockIdx.x * kAssignChunk, left = n - c0;  // (c0 < n: no wrap)
  if constexpr (WITH_MOMENTS) partials += (size_t)blockIdx.x * n_models * AccLs<M>::N;
  assign_pass_chunk<M, WITH_MOMENTS>(data + (size_t)c0 * stride, stride, left < kAssignChunk ? left : kAssignChunk, rows,
                                     n_models, org_off, mc, labels + c0, residuals ? residuals + c0 : nullptr,
                                     old ? old + c0 : nullptr, counters + ASG_CHANGED, counters + ASG_COUNT, partials,
                                     presence ? presence + blockIdx.x : nullptr);
}

// What lane 0 of a solve kernel does with a model's summed moments: the refit about the model's own point (the body of
// k_many_solve), or nothing.  row_m becomes the new model's scan row, and the answer is true, when the model had at
// least M::K records (cnt) and the solve gave a result; any other model keeps its row.  org_m (nullable: null for
// every family but the rigid one): the model's origin of kAssignOrigin<M> doubles, taken instead of row_m[org_off ..]
template <class M>
__device__ __forceinline__ bool assign_refit(const double *mom, double *row_m, unsigned long long cnt, int org_off,
                                             const ModelConsts &mc, double *ws, SolveOut *so,
                                             const double *org_m = nullptr) {
  if (cnt < (unsigned long long)M::K) return false;
  constexpr int NC = M::P > M::REC ? M::P : M::REC;
  double org[NC];
  const double *o = org_m ? org_m : row_m + org_off;
  for (int j = 0; j < NC; j++) org[j] = j < kAssignOrigin<M> ? o[j] : 0.0;
  solve_small<M>(mom, org, mc, ws, so);
  if (!so->ok) return false;
  double p[M::P], row[M::SP];
  for (int j = 0; j < (int)M::P; j++) p[j] = so->params[j];
  assign_make_row<M>(p, mc, row);
  for (int j = 0; j < (int)M::SP; j++) row_m[j] = row[j];
  return true;
}

// One model's blocks of N sums, `qs` doubles apart from chunk to chunk, summed in chunk order by a workgroup of kBlock
// lanes: mom[k] = sum over the chunks of src[chunk * qs + k], then a barrier.  A strictly serial sum of thousands of
// partials is bound by memory latency if one lane loads what it adds, so the four waves stage tiles of kTile chunks
// through LDS (s_t: kTile * N doubles) -- every lane a few loads, all in flight at once, the next tile's issued before
// this one is summed -- and lane k of wave 0 adds column k of the tile in chunk order.
template <int N, int kTile>
__device__ __forceinline__ void assign_sum_chunks(const double *__restrict__ src, size_t qs, uint32_t chunks,
                                                  double *s_t, double *mom) {
  constexpr int E = (kTile * N + kBlock - 1) / kBlock;  // elements of a tile per lane
  static_assert(N <= 64, "one lane per moment");
  const int k = threadIdx.x;
  double pre[E], t = 0.0;
  auto fetch = [&](uint32_t q0) {  // tile [q0, q0 + kTile) -> registers
    const uint32_t cnt = chunks - q0 < (uint32_t)kTile ? chunks - q0 : (uint32_t)kTile;
#pragma unroll
    for (int u = 0; u < E; u++) {
      const uint32_t e = (uint32_t)u * kBlock + threadIdx.x, q = e / N;
      pre[u] = q < cnt ? src[(size_t)(q0 + q) * qs + (e - q * N)] : 0.0;
    }
  };
  if (chunks) fetch(0);
  for (uint32_t q0 = 0; q0 < chunks; q0 += kTile) {
    const uint32_t cnt = chunks - q0 < (uint32_t)kTile ? chunks - q0 : (uint32_t)kTile;
    __syncthreads();  // the tile before has been summed
#pragma unroll
    for (int u = 0; u < E; u++) {
      const uint32_t e = (uint32_t)u * kBlock + threadIdx.x;
      if (e < (uint32_t)(kTile * N)) s_t[e] = pre[u];
    }
    __syncthreads();
    if (q0 + kTile < chunks) fetch(q0 + kTile);
    if (k < N)
      for (uint32_t q = 0; q < cnt; q++) t += s_t[q * N + k];
  }
  if (k < N) mom[k] = t;
  __syncthreads();
}

// one workgroup per model m: the partials of its `chunks` chunks summed in chunk order (assign_sum_chunks), then
// assign_refit.  counters[ASG_USED + m] and counters[ASG_OK + m] say what happened.  start (nullable): n_models rows
// of M::SP; given, row m of `rows` is only read, and row m of `start` gets what `rows` would have got: the new scan
// row where assign_refit says true, a copy of the old one where not (the LM stage of assign_lm.h starts from it)
template <class M>
__global__ __launch_bounds__(kBlock) void k_assign_solve(const double *__restrict__ partials, uint32_t chunks,
                                                         int n_models, int org_off, ModelConsts mc, double *rows,
                                                         unsigned long long *counters, double *start) {
  constexpr int N = M::NMOM;
  constexpr int kTile = N <= 16 ? 512 : 128;  // chunks per tile: 40 KiB of LDS at N = 10, 55 KiB at N = 55
  __shared__ double s_t[kTile * N];
  __shared__ double mom[MOM_MAX];
  __shared__ double ws[M::NMOM > 40 ? 512 : 8];
  __shared__ SolveOut so;
  const int m = blockIdx.x;
  assign_sum_chunks<N, kTile>(partials + (size_t)m * N, (size_t)n_models * N, chunks, s_t, mom);
  if (threadIdx.x != 0) return;
  const unsigned long long cnt = counters[ASG_COUNT + m];
  counters[ASG_USED + m] = cnt;
  double *row_m = rows + (size_t)m * M::SP;
  if (start) {
    for (int j = 0; j < (int)M::SP; j++) start[(size_t)m * M::SP + j] = row_m[j];
    row_m = start + (size_t)m * M::SP;
  }
  counters[ASG_OK + m] = assign_refit<M>(mom, row_m, cnt, org_off, mc, ws, &so) ? 1 : 0;
}

// ---- host side -----------------------------------------------------------------------------------------------------
struct AssignLmOut {  // lsqr_refine_lm: what the LM run of one model's last refit left (zero where none ran)
  int lm_info, lm_nfev, stall, pad;
  double cost;
};

// what every family of the round loop holds: the scan rows, the chunk partials, the labels of this round and of the one
// before, the residuals, the counter words, and their pinned staging
struct AssignCore {
  DevBuf<double> d_rows, d_partials, d_res;
  DevBuf<int32_t> d_labels[2];
  DevBuf<unsigned long long> d_cnt;
  PinBuf<char> h_pin;  // the family's AssignPin
};

// h_pin: kAssignMaxModels rows of at most ROW_MAX doubles, the counter words -- ASG_CHANGED, then 1 + BLOCKS blocks of
// kAssignMaxModels (ASG_COUNT, ASG_USED, ASG_OK, ...) --, then OWN bytes of the family's own
template <int ROW_MAX, int BLOCKS, size_t OWN>
struct AssignPin {
  static constexpr int row_max = ROW_MAX;
  static constexpr size_t words = ASG_USED + (size_t)BLOCKS * kAssignMaxModels;
  static constexpr size_t cnt = sizeof(double) * kAssignMaxModels * ROW_MAX;
  static constexpr size_t own = cnt + sizeof(unsigned long long) * words;
  static constexpr size_t bytes = own + OWN;
};

struct AssignBufs {  // owned by the context (lsqr_ctx::assign), grown on demand
  AssignCore core;
  DevBuf<double> d_par;
  // the LM stage of lsqr_refine_lm (assign_lm.h)
  DevBuf<double> d_start, d_lm_partials;
  DevBuf<unsigned long long> d_presence, d_lm_mask;  // one word per chunk; the bits of the models whose LM goes on
  DevBuf<uint32_t> d_lm_live;                         // their number
  DevBuf<LmState> d_lm_state;
  DevBuf<AssignLmOut> d_lm_out;
  // the origin pre-pass of lsqr_refine_rigid (assign_rigid.h): a record index and an origin per model
  DevBuf<unsigned long long> d_first;
  DevBuf<double> d_org;
};

struct AssignJob {
  hipStream_t stream = nullptr;
  lsqr_model_cfg cfg{};
  ModelConsts mc{};
  const double *data = nullptr;  // the context's records: n of them, `stride` doubles apart
  size_t stride = 0;
  uint32_t n = 0;
  // the call
  double *params = nullptr;  // host, n_models rows of the model's parameters: read, and written when a refit ran
  size_t n_models = 0, max_rounds = 0;
  int on_device = 0;
  int32_t *labels_out = nullptr;
  double *residuals_out = nullptr;
  uint64_t *counts_out = nullptr;
  lsqr_fit_info *fits = nullptr;
  int32_t *status_out = nullptr;
  size_t rounds = 0;
  int converged = 0;
  char err[256] = {0};
};

// a refine call's answer for one model of a set that ran `rounds` refit rounds; okf, used: the ASG_OK and ASG_USED
// words of its last refit; n_params: what a model that was fitted reports
inline void assign_fit_out(size_t rounds, unsigned long long okf, unsigned long long used, int32_t n_params,
                           int32_t *status, lsqr_fit_info *fit) {
  const bool ok = rounds == 0 || okf != 0;
  *status = ok ? LSQR_OK : LSQR_EMPTY;
  memset(fit, 0, sizeof *fit);
  if (rounds > 0) {
    fit->n_params = ok ? n_params : 0;
    fit->n_used = used;
  }
}

// THE round loop of the eight ungrouped calls (an assign call: max_rounds == 0).  Round r: the pass -- labels L_r and,
// unless it is the last round allowed, whatever the refit needs of L_r --, the 8-byte changed-counter (with the counts:
// one copy) to the host, one synchronisation, then the refit under L_r.  Returns after the stream has drained; the
// outputs are written only then.  What differs from call to call is the family F (by value: a few references):
//   F::Pin, F::SP        its AssignPin, and the doubles of one of its scan rows
//   core()               the AssignCore among its buffers
//   chunks_of(n)         its chunks of n records
//   reserve(J, refine)   grows its own buffers (and d_partials, whose size is its own)
//   rows_up(J, h_rows)   enqueues the caller's parameters -> d_rows, staged through h_rows
//   pass(J, last, lab, res, old)   enqueues the pass of this round, with all that has to be under way before the sync
//   refit(J, lab)        after the sync: enqueues the refit under the labels lab; it leaves the new rows in d_rows
//   results(J)           enqueues its own result copies (the rows and the counter words are copied here)
//   rows_down(J, h_rows) the rows that came back -> the caller's parameters
//   n_params(J)          what a fitted model's record reports
//   fit_more(J, m, h_cnt, fit)   what it adds to model m's record after a refit ran
// AssignClosed<M> is lsqr_assign's and lsqr_refine's, AssignLm<M> (assign_lm.h) lsqr_refine_lm's, AssignDense<NR>
// (assign_dense.h) the dense pair's, AssignRigid<M> (assign_rigid.h) the rigid pair's.
template <class F>
int assign_rounds(AssignJob &J, F fam) {
  typedef typename F::Pin Pin;
  AssignCore &C = fam.core();
  const int nm = (int)J.n_models;
  const uint32_t n = J.n;
  const bool refine = J.max_rounds > 0;
  // no refit and device pointers: the kernel writes the caller's buffers
  const bool direct = !refine && J.on_device && J.labels_out;
  static_assert(F::SP <= Pin::row_max, "pinned staging of the rows");
  if (!C.h_pin.get()) MANYCHK(C.h_pin.alloc(Pin::bytes));
  MANYCHK(many_grow(C.d_rows, (size_t)kAssignMaxModels * Pin::row_max));
  MANYCHK(many_grow(C.d_cnt, Pin::words));
  if (!direct) MANYCHK(many_grow(C.d_labels[0], (size_t)n));
  if (J.residuals_out && !J.on_device) MANYCHK(many_grow(C.d_res, (size_t)n));
  if (refine) MANYCHK(many_grow(C.d_labels[1], (size_t)n));
  int st = fam.reserve(J, refine);
  if (st != LSQR_OK) return st;
  double *h_rows = (double *)C.h_pin.get();
  unsigned long long *h_cnt = (unsigned long long *)(C.h_pin.get() + Pin::cnt);

  if ((st = fam.rows_up(J, h_rows)) != LSQR_OK) return st;
  MANYCHK(hipMemsetAsync(C.d_cnt, 0, sizeof(unsigned long long) * Pin::words, J.stream));

  int cur = 0;
  size_t r = 0;
  bool converged = false;
  for (;;) {
    const bool last = r == J.max_rounds;
    int32_t *lab = direct ? J.labels_out : C.d_labels[cur].get();
    double *res = !J.residuals_out ? nullptr : J.on_device ? J.residuals_out : C.d_res.get();
    const int32_t *old = r > 0 ? C.d_labels[cur ^ 1].get() : nullptr;
    if (r > 0)
      MANYCHK(hipMemsetAsync(C.d_cnt, 0, sizeof(unsigned long long) * (ASG_COUNT + kAssignMaxModels), J.stream));
    if ((st = fam.pass(J, last, lab, res, old)) != LSQR_OK) return st;
    MANYCHK(hipMemcpyAsync(h_cnt, C.d_cnt, sizeof(unsigned long long) * (ASG_COUNT + kAssignMaxModels),
                          hipMemcpyDeviceToHost, J.stream));
    MANYCHK(hipStreamSynchronize(J.stream));
    if (r > 0 && h_cnt[ASG_CHANGED] == 0) {
      converged = true;
      break;
    }
    if (last) break;
    if ((st = fam.refit(J, lab)) != LSQR_OK) return st;
    r++;
    cur ^= 1;
  }

  // results: the rows and what the last refit did, then the labels of the last pass
  if (r > 0) {
    MANYCHK(hipMemcpyAsync(h_rows, C.d_rows, sizeof(double) * (size_t)nm * F::SP, hipMemcpyDeviceToHost, J.stream));
    MANYCHK(hipMemcpyAsync(h_cnt + ASG_USED, C.d_cnt + ASG_USED, sizeof(unsigned long long) * (Pin::words - ASG_USED),
                          hipMemcpyDeviceToHost, J.stream));
    if ((st = fam.results(J)) != LSQR_OK) return st;
  }
  if (J.labels_out && !direct)
    MANYCHK(hipMemcpyAsync(J.labels_out, C.d_labels[cur], sizeof(int32_t) * (size_t)n,
                          J.on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, J.stream));
  if (J.residuals_out && !J.on_device)
    MANYCHK(hipMemcpyAsync(J.residuals_out, C.d_res, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, J.stream));
  MANYCHK(hipStreamSynchronize(J.stream));
  if (r > 0) fam.rows_down(J, h_rows);
  if (J.counts_out) {
    uint64_t sum = 0;
    for (int m = 0; m < nm; m++) sum += (J.counts_out[m] = h_cnt[ASG_COUNT + m]);
    J.counts_out[nm] = (uint64_t)n - sum;
  }
  if (J.fits)  // the refine calls
    for (int m = 0; m < nm; m++) {
      assign_fit_out(r, h_cnt[ASG_OK + m], h_cnt[ASG_USED + m], fam.n_params(J), &J.status_out[m], &J.fits[m]);
      if (r > 0) fam.fit_more(J, m, h_cnt, J.fits[m]);
    }
  J.rounds = r;
  J.converged = converged ? 1 : 0;
  return LSQR_OK;
}

// The closed form: lsqr_assign, and lsqr_refine, whose refit is one k_assign_solve launch.  Its h_pin has room for what
// AssignLm<M> (assign_lm.h) reads back -- an AssignLmOut per model and the live counter --, since both run on
// lsqr_ctx::assign and whichever comes first allocates it.
template <class M>
struct AssignClosed {
  typedef AssignPin<16, 2, sizeof(AssignLmOut) * kAssignMaxModels + sizeof(unsigned long long)> Pin;
  static constexpr int SP = M::SP;
  static_assert(Pin::words == ASG_WORDS, "the counter words");
  static_assert(M::P <= 16, "pinned staging of the parameters");
  AssignBufs &B;

  AssignCore &core() { return B.core; }
  static uint32_t chunks_of(uint32_t n) { return assign_chunks(n); }
  int reserve(AssignJob &J, bool refine) {
    MANYCHK(many_grow(B.d_par, (size_t)kAssignMaxModels * 16));
    if (refine) MANYCHK(many_grow(B.core.d_partials, (size_t)chunks_of(J.n) * J.n_models * M::NMOM));
    return LSQR_OK;
  }
  int rows_up(AssignJob &J, double *h_rows) {  // upload, then k_assign_prepare
    const int nm = (int)J.n_models;
    memcpy(h_rows, J.params, sizeof(double) * (size_t)nm * M::P);
    MANYCHK(hipMemcpyAsync(B.d_par, h_rows, sizeof(double) * (size_t)nm * M::P, hipMemcpyHostToDevice, J.stream));
    hipLaunchKernelGGL((k_assign_prepare<M>), dim3(1), dim3(kBlock), 0, J.stream, B.d_par, nullptr, (uint64_t)nm, nm,
                       J.mc, B.core.d_rows);  // one group, every row there
    MANYCHK(hipGetLastError());
    return LSQR_OK;
  }
  // presence: where a pass with moments leaves every chunk's word (nullable)
  int pass_to(AssignJob &J, bool last, int32_t *lab, double *res, const int32_t *old, unsigned long long *presence) {
    const int nm = (int)J.n_models, org_off = fit_origin_offset<M>(J.cfg);
    const uint32_t chunks = chunks_of(J.n);
    AssignCore &C = B.core;
    if (last)
      hipLaunchKernelGGL((k_assign_moments<M, false>), dim3(chunks), dim3(kBlock), 0, J.stream, J.data, J.stride, J.n,
                         C.d_rows, nm, org_off, J.mc, lab, res, old, C.d_cnt, nullptr, nullptr);
    else
      hipLaunchKernelGGL((k_assign_moments<M, true>), dim3(chunks), dim3(kBlock), 0, J.stream, J.data, J.stride, J.n,
                         C.d_rows, nm, org_off, J.mc, lab, res, old, C.d_cnt, C.d_partials, presence);
    MANYCHK(hipGetLastError());
    return LSQR_OK;
  }
  int pass(AssignJob &J, bool last, int32_t *lab, double *res, const int32_t *old) {
    return pass_to(J, last, lab, res, old, nullptr);
  }
  // start (nullable): see k_assign_solve
  int solve_to(AssignJob &J, double *start) {
    const int nm = (int)J.n_models;
    hipLaunchKernelGGL((k_assign_solve<M>), dim3(nm), dim3(kBlock), 0, J.stream, B.core.d_partials, chunks_of(J.n), nm,
                       fit_origin_offset<M>(J.cfg), J.mc, B.core.d_rows, B.core.d_cnt, start);
    MANYCHK(hipGetLastError());
    return LSQR_OK;
  }
  int refit(AssignJob &J, const int32_t *) { return solve_to(J, nullptr); }
  int results(AssignJob &) { return LSQR_OK; }
  void rows_down(AssignJob &J, const double *h_rows) {
    for (size_t m = 0; m < J.n_models; m++)
      for (int j = 0; j < (int)M::P; j++) J.params[m * M::P + j] = h_rows[m * M::SP + j];
  }
  static int32_t n_params(const AssignJob &) { return (int32_t)M::P; }
  void fit_more(AssignJob &, int, const unsigned long long *, lsqr_fit_info &) {}
};
#endif  // __HIPCC__

}  // namespace lsqr
