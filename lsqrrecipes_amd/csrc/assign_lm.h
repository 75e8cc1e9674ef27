// assign_lm.h -- lsqr_refine_lm: the round loop (assign.h: assign_rounds) for the sphere with LSQR_LS_GEOMETRIC, as the
// family AssignLm<M>.  The refit of a round is the algebraic refit of assign.h, kept aside as the START, and then one
// Levenberg-Marquardt run per model over the records labelled with it, all models in lock-step evaluation rounds, the
// records read where they are.
//
//   k_assign_moments<M, true>   as in lsqr_refine; it also stores every chunk's presence word
//   k_assign_solve              as in lsqr_refine, but into the start rows (its `start` argument): the round's rows stay
//   k_assign_lm_init            one lane per model: lm_init from its start row where the algebraic refit gave one; the
//                               mask of the live models and their number; ASG_OK cleared (the LM decides it)
//   per evaluation:
//   assign_lm_pass_chunk        ONE evaluation over a chunk, by a workgroup of kBlock lanes with assign_pass_chunk's
//                               mapping of lanes to records: kAssignPerLane records and their labels per lane, loaded
//                               once.  For every model that is in the chunk AND live, in ascending order: xtrial at a
//                               wave-uniform address, M::accumulate_lm on the lane's records with that label in index
//                               order, the __shfl_down tree, the wave sums in two alternating LDS buffers, one barrier
//                               per model, the four waves in index order -> the chunk's partials [m][M::NMOM_LM].  It
//                               must be inlined: as a called function it keeps the lane's records in memory.
//   k_assign_lm_pass            chunk blockIdx.x; a chunk that holds no live model's record returns at once
//   k_assign_lm_step            one workgroup per live model: its column of partials summed in chunk order
//                               (assign_sum_chunks, as k_assign_solve), LmState staged in LDS, lane 0 runs lm_advance.
//                               A model that finishes writes its AssignLmOut and, with info in 1..4, its new scan row
//                               by assign_make_row -- the bits k_assign_prepare makes from the returned parameters --
//                               and ASG_OK; then it leaves the live mask and the live counter, which the host reads (4
//                               bytes) after every evaluation.
//
// A model absent from a chunk has zeros there: the partials are cleared once per refit round (the labels, and so the
// presence words, are fixed for the round), and the pass writes only the blocks of models that are present and live.
// A finished model's column is never read again.
//
// Determinism: model m's block in every evaluation is a function of its own records, their positions in the upload
// (kAssignChunk fixes which chunk and lane holds a record) and its own trial point.  Nothing is summed with a
// floating-point atomic.  So the iterates of m do not depend on the other rows of the call or on where m sits.
//
// Budget: see DESIGN.md section 14.2.  LDS of the pass: two buffers of 4 x NMOM_LM doubles (3.4 KiB at D = 8); of the
// step: one tile of partials (30 KiB at NMOM_LM <= 16, else up to 55 KiB), the moment block and LmState (1.7 KiB).
//
// assign_lm_start, assign_lm_stage and assign_lm_finish are the pieces of the init and step kernels that the grouped
// call's kernels (assign_lm_grouped.h) run too, and assign_lm_evals is the evaluation loop of both drivers.
#pragma once
#include "assign.h"
#include "lm_core.h"

namespace lsqr {

#if defined(__HIPCC__)
// The pieces that k_assign_lm_init / k_assign_lm_step share with k_asg_grp_lm_init / k_asg_grp_lm_step
// (assign_lm_grouped.h), so that a group's models start, advance and finish by the code of lsqr_refine_lm's.
//
// One lane per model of a set, the whole wave calling.  there: the lane has a model; okf, out, st, start (read and
// written only where `there`): its answer from the algebraic refit (cleared: the LM decides it), its AssignLmOut, its
// LmState and its start row.  -> the mask of the models whose LM run starts
template <class M>
__device__ __forceinline__ unsigned long long assign_lm_start(bool there, unsigned long long *okf, AssignLmOut *out,
                                                              LmState *st, const double *start, int n, double ftol,
                                                              double xtol, double gtol, int maxfev) {
  const bool go = there && *okf != 0;
  if (there) {
    *okf = 0;
    *out = AssignLmOut{0, 0, 0, 0, 0.0};
  }
  if (go) lm_init(*st, n, start, ftol, xtol, gtol, maxfev, 100.0);
  return __ballot(go);
}

// an LmState between global memory and LDS, word by word, by a workgroup of WG lanes
template <int WG>
__device__ __forceinline__ void assign_lm_stage(const LmState *from, LmState *to) {
  constexpr int NW = (int)(sizeof(LmState) / sizeof(int));
  const int *src = (const int *)from;
  int *dst = (int *)to;
  for (int i = threadIdx.x; i < NW; i += WG) dst[i] = src[i];
}

// One lane, after lm_advance said that model m's run is over: its AssignLmOut and, with info in 1..4, its new scan row
// by assign_make_row and its ok word; then it leaves its set's live mask and the live counter
template <class M>
__device__ __forceinline__ void assign_lm_finish(const LmState &S, const ModelConsts &mc, int m, double *row,
                                                 unsigned long long *okf, AssignLmOut *out, unsigned long long *mask,
                                                 uint32_t *live) {
  *out = AssignLmOut{S.info, S.nfev, S.stall, 0, S.fnorm * S.fnorm};
  if (S.info >= 1 && S.info <= 4) {  // vnl_levenberg_marquardt::minimize -> true
    double p[LM_NMAX], r[M::SP];
    M::lm_finalize(S.x, p);
    assign_make_row<M>(p, mc, r);
    for (int j = 0; j < (int)M::SP; j++) row[j] = r[j];
    *okf = 1;
  }
  atomicAnd(mask, ~(1ull << m));
  atomicSub(live, 1u);
}

// start: the n_models start rows k_assign_solve left; counters[ASG_OK + m]: its answer, cleared here
template <class M>
__global__ __launch_bounds__(64) void k_assign_lm_init(const double *__restrict__ start, int n_models, int n,
                                                       double ftol, double xtol, double gtol, int maxfev,
                                                       unsigned long long *__restrict__ counters,
                                                       LmState *__restrict__ st, AssignLmOut *__restrict__ out,
                                                       unsigned long long *__restrict__ mask,
                                                       uint32_t *__restrict__ live) {
  const int m = threadIdx.x;
  const unsigned long long all = assign_lm_start<M>(m < n_models, counters + ASG_OK + m, out + m, st + m,
                                                    start + (size_t)m * M::SP, n, ftol, xtol, gtol, maxfev);
  if (m == 0) {
    *mask = all;
    *live = (uint32_t)__popcll(all);
  }
}

// One evaluation over ONE chunk.  The chunk's base is in the pointers, so its records are [0, n), n <= kAssignChunk.
// labels: the chunk's n labels of this round; todo (workgroup-uniform, not zero): the models in the chunk and live;
// st: the LmState of every model; partials: the chunk's [model][M::NMOM_LM]
template <class M>
__device__ __forceinline__ void assign_lm_pass_chunk(const double *__restrict__ data, size_t stride, uint32_t n,
                                                     const int32_t *__restrict__ labels, unsigned long long todo,
                                                     const LmState *__restrict__ st, const ModelConsts &mc,
                                                     double *__restrict__ partials) {
  constexpr int R = kAssignPerLane, W = kBlock / 64, N = M::NMOM_LM, D = M::ND;
  static_assert(N <= 64, "one lane per moment");
  __shared__ double s_m[2][W][N];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;

  double x[R][M::REC];
  int32_t lab[R];
  unsigned long long pres = 0;
#pragma unroll
  for (int j = 0; j < R; j++) {
    const uint32_t i = (uint32_t)j * kBlock + threadIdx.x;
    const bool in = i < n;
    M::load(data + (size_t)(in ? i : 0) * stride, mc, x[j]);
    lab[j] = in ? labels[i] : -1;  // (a record with a non-finite coordinate has label -1)
    if (lab[j] >= 0) pres |= 1ull << lab[j];
  }
  for (int o = 32; o > 0; o >>= 1) pres |= __shfl_xor(pres, o);
  const unsigned long long mine = wave_uniform64(pres);

  int it = 0;
  for (unsigned long long rest = todo; rest; rest &= rest - 1, it++) {
    const int m = __builtin_ctzll(rest);
    double(*buf)[N] = s_m[it & 1];
    if ((mine >> m) & 1ull) {  // this wave holds records of model m
      double xk[D + 1], acc[N];
      const double *xt = st[m].xtrial;  // wave-uniform: scalar loads
#pragma unroll
      for (int k = 0; k <= D; k++) xk[k] = xt[k];
#pragma unroll
      for (int k = 0; k < N; k++) acc[k] = 0.0;
#pragma unroll
      for (int j = 0; j < R; j++)
        if (lab[j] == m) M::accumulate_lm(x[j], xk, acc);
#pragma unroll
      for (int k = 0; k < N; k++) {
        double v = acc[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
        if (lane == 0) buf[wave][k] = v;
      }
    } else if (lane < N) {
      buf[wave][lane] = 0.0;
    }
    // one barrier per model, two buffers: as the moment phase of assign_pass_chunk
    __syncthreads();
    if (threadIdx.x < N) {
      double t = 0.0;
      for (int w = 0; w < W; w++) t += buf[w][threadIdx.x];
      partials[(size_t)m * N + threadIdx.x] = t;
    }
  }
}

// chunk blockIdx.x of the context's n records under the round's labels; presence: one word per chunk; mask: the live
// models; partials: [chunk][model][M::NMOM_LM], cleared at the start of the refit round
template <class M>
__global__ __launch_bounds__(kBlock) void k_assign_lm_pass(const double *__restrict__ data, size_t stride, uint32_t n,
                                                           const int32_t *__restrict__ labels,
                                                           const unsigned long long *__restrict__ presence,
                                                           const unsigned long long *__restrict__ mask,
                                                           const LmState *__restrict__ st, int n_models, ModelConsts mc,
                                                           double *__restrict__ partials) {
  const unsigned long long t = presence[blockIdx.x] & *mask;  // (uniform addresses)
  const unsigned long long todo = wave_uniform64(t);
  if (!todo) return;
  const uint32_t c0 = blockIdx.x * kAssignChunk, left = n - c0;  // (c0 < n: no wrap)
  assign_lm_pass_chunk<M>(data + (size_t)c0 * stride, stride, left < kAssignChunk ? left : kAssignChunk, labels + c0,
                          todo, st, mc, partials + (size_t)blockIdx.x * n_models * M::NMOM_LM);
}

// one workgroup per model m that is still live: the evaluation's block, then lm_advance
template <class M>
__global__ __launch_bounds__(kBlock) void k_assign_lm_step(const double *__restrict__ partials, uint32_t chunks,
                                                           int n_models, ModelConsts mc, LmState *__restrict__ st,
                                                           double *__restrict__ rows,
                                                           unsigned long long *__restrict__ counters,
                                                           AssignLmOut *__restrict__ out, unsigned long long *mask,
                                                           uint32_t *live) {
  constexpr int N = M::NMOM_LM;
  constexpr int kTile = N <= 16 ? 256 : 128;  // chunks per tile: 30 KiB of LDS at N = 15, 55 KiB at N = 55
  __shared__ double s_t[kTile * N];
  __shared__ double mom[LM_MOM_MAX];
  __shared__ LmState S;
  const int m = blockIdx.x;
  if (!((*mask >> m) & 1ull)) return;  // finished, or never started (uniform over the workgroup)
  assign_sum_chunks<N, kTile>(partials + (size_t)m * N, (size_t)n_models * N, chunks, s_t, mom);
  assign_lm_stage<kBlock>(&st[m], &S);
  __syncthreads();
  if (threadIdx.x == 0 && !lm_advance(S, mom))
    assign_lm_finish<M>(S, mc, m, rows + (size_t)m * M::SP, counters + ASG_OK + m, out + m, mask, live);
  __syncthreads();
  assign_lm_stage<kBlock>(&S, &st[m]);
}

// ---- host side -----------------------------------------------------------------------------------------------------
// The evaluations of one refit round's LM stage, lsqr_refine_lm's and lsqr_refine_lm_grouped's: pass() and step() each
// enqueue one launch; then one 4-byte read of the live counter and one synchronisation.  Every lm_advance call consumes
// one evaluation and stops at maxfev, so maxfev evaluations finish every model (many_lm_run's bound).
template <class Pass, class Step>
int assign_lm_evals(hipStream_t stream, int maxfev, const uint32_t *d_live, uint32_t *h_live, char (&err)[256],
                    Pass pass, Step step) {
  struct {
    char (&err)[256];
  } J{err};  // (MANYCHK reports into J.err)
  for (int round = 0;; round++) {
    if (round > maxfev) {
      snprintf(err, sizeof err, "LM stage: %u models still live after %d evaluations", *h_live, round);
      return LSQR_ERR_HIP;
    }
    pass();
    MANYCHK(hipGetLastError());
    step();
    MANYCHK(hipGetLastError());
    MANYCHK(hipMemcpyAsync(h_live, d_live, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    MANYCHK(hipStreamSynchronize(stream));
    if (*h_live == 0) break;
  }
  return LSQR_OK;
}

// lsqr_refine_lm's family: AssignClosed<M> whose pass also leaves the presence words and whose refit is the LM stage.
// The pass has left the moments of the labels `lab` in d_partials and the presence words in d_presence; the refit is
// the algebraic solve into the start rows, k_assign_lm_init, the partials cleared, then the evaluations.
template <class M>
struct AssignLm : AssignClosed<M> {
  typedef AssignClosed<M> Base;
  using Base::B;
  using Base::chunks_of;

  int reserve(AssignJob &J, bool refine) {
    const int st = Base::reserve(J, refine);
    if (st != LSQR_OK || !refine) return st;
    const uint32_t chunks = chunks_of(J.n);
    MANYCHK(many_grow(B.d_start, (size_t)kAssignMaxModels * 16));
    MANYCHK(many_grow(B.d_presence, (size_t)chunks));
    MANYCHK(many_grow(B.d_lm_partials, (size_t)chunks * J.n_models * M::NMOM_LM));
    MANYCHK(many_grow(B.d_lm_mask, 1));
    MANYCHK(many_grow(B.d_lm_live, 1));
    MANYCHK(many_grow(B.d_lm_state, (size_t)kAssignMaxModels));
    MANYCHK(many_grow(B.d_lm_out, (size_t)kAssignMaxModels));
    return LSQR_OK;
  }
  int pass(AssignJob &J, bool last, int32_t *lab, double *res, const int32_t *old) {
    return Base::pass_to(J, last, lab, res, old, B.d_presence.get());
  }
  int refit(AssignJob &J, const int32_t *lab) {
    const int nm = (int)J.n_models;
    const uint32_t chunks = chunks_of(J.n);
    int n = 0, maxfev = 0;
    double ftol = 0, xtol = 0, gtol = 0;
    lm_settings(J.cfg, &n, &ftol, &xtol, &gtol, &maxfev);
    const int st = Base::solve_to(J, B.d_start);
    if (st != LSQR_OK) return st;
    hipLaunchKernelGGL((k_assign_lm_init<M>), dim3(1), dim3(64), 0, J.stream, B.d_start, nm, n, ftol, xtol, gtol,
                       maxfev, B.core.d_cnt, B.d_lm_state, B.d_lm_out, B.d_lm_mask, B.d_lm_live);
    MANYCHK(hipGetLastError());
    MANYCHK(hipMemsetAsync(B.d_lm_partials, 0, sizeof(double) * (size_t)chunks * nm * M::NMOM_LM, J.stream));
    return assign_lm_evals(
        J.stream, maxfev, B.d_lm_live, (uint32_t *)(h_lm() + kAssignMaxModels), J.err,
        [&] {
          hipLaunchKernelGGL((k_assign_lm_pass<M>), dim3(chunks), dim3(kBlock), 0, J.stream, J.data, J.stride, J.n, lab,
                             B.d_presence, B.d_lm_mask, B.d_lm_state, nm, J.mc, B.d_lm_partials);
        },
        [&] {
          hipLaunchKernelGGL((k_assign_lm_step<M>), dim3(nm), dim3(kBlock), 0, J.stream, B.d_lm_partials, chunks, nm,
                             J.mc, B.d_lm_state, B.core.d_rows, B.core.d_cnt, B.d_lm_out, B.d_lm_mask, B.d_lm_live);
        });
  }
  int results(AssignJob &J) {
    MANYCHK(hipMemcpyAsync(h_lm(), B.d_lm_out, sizeof(AssignLmOut) * J.n_models, hipMemcpyDeviceToHost, J.stream));
    return LSQR_OK;
  }
  void fit_more(AssignJob &, int m, const unsigned long long *, lsqr_fit_info &fit) {
    const AssignLmOut &o = h_lm()[m];
    fit.lm_info = o.lm_info;
    fit.lm_nfev = o.lm_nfev;
    fit.reserved = o.stall;
    fit.cost = o.cost;
  }
  // the family's own of h_pin: an AssignLmOut per model, then the live counter's copy
  AssignLmOut *h_lm() { return (AssignLmOut *)(B.core.h_pin.get() + Base::Pin::own); }
};
#endif  // __HIPCC__

}  // namespace lsqr
