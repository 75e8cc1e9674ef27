// assign_lm.h -- lsqr_refine_lm: lsqr_refine's loop (assign.h: assign_run) for the sphere with LSQR_LS_GEOMETRIC.  The
// refit of a round is the algebraic refit of assign.h, kept aside as the START, and then one Levenberg-Marquardt run per
// model over the records labelled with it, all models in lock-step evaluation rounds, the records read where they are.
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
// Included by assign.h's users after it; assign_run<M, true> calls assign_lm_reserve and assign_lm_run.
#pragma once
#include "assign.h"
#include "lm_core.h"

namespace lsqr {

#if defined(__HIPCC__)
// start: the n_models start rows k_assign_solve left; counters[ASG_OK + m]: its answer, cleared here
template <class M>
__global__ __launch_bounds__(64) void k_assign_lm_init(const double *__restrict__ start, int n_models, int n,
                                                       double ftol, double xtol, double gtol, int maxfev,
                                                       unsigned long long *__restrict__ counters,
                                                       LmState *__restrict__ st, AssignLmOut *__restrict__ out,
                                                       unsigned long long *__restrict__ mask,
                                                       uint32_t *__restrict__ live) {
  const int m = threadIdx.x;
  const bool there = m < n_models;
  const bool go = there && counters[ASG_OK + m] != 0;
  if (there) {
    counters[ASG_OK + m] = 0;
    out[m] = AssignLmOut{0, 0, 0, 0, 0.0};
  }
  if (go) lm_init(st[m], n, start + (size_t)m * M::SP, ftol, xtol, gtol, maxfev, 100.0);
  const unsigned long long all = __ballot(go);
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
  const unsigned long long mine = ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(pres >> 32)) << 32) |
                                  __builtin_amdgcn_readfirstlane((uint32_t)pres);

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
  const unsigned long long todo = ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(t >> 32)) << 32) |
                                  __builtin_amdgcn_readfirstlane((uint32_t)t);
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
  constexpr int NW = (int)(sizeof(LmState) / sizeof(int));
  __shared__ double s_t[kTile * N];
  __shared__ double mom[LM_MOM_MAX];
  __shared__ LmState S;
  const int m = blockIdx.x;
  if (!((*mask >> m) & 1ull)) return;  // finished, or never started (uniform over the workgroup)
  assign_sum_chunks<N, kTile>(partials + (size_t)m * N, (size_t)n_models * N, chunks, s_t, mom);
  {
    const int *src = (const int *)&st[m];
    int *dst = (int *)&S;
    for (int i = threadIdx.x; i < NW; i += kBlock) dst[i] = src[i];
  }
  __syncthreads();
  if (threadIdx.x == 0 && !lm_advance(S, mom)) {
    out[m] = AssignLmOut{S.info, S.nfev, S.stall, 0, S.fnorm * S.fnorm};
    if (S.info >= 1 && S.info <= 4) {  // vnl_levenberg_marquardt::minimize -> true
      double p[LM_NMAX], row[M::SP];
      M::lm_finalize(S.x, p);
      assign_make_row<M>(p, mc, row);
      for (int j = 0; j < (int)M::SP; j++) rows[(size_t)m * M::SP + j] = row[j];
      counters[ASG_OK + m] = 1;
    }
    atomicAnd(mask, ~(1ull << m));
    atomicSub(live, 1u);
  }
  __syncthreads();
  {
    const int *src = (const int *)&S;
    int *dst = (int *)&st[m];
    for (int i = threadIdx.x; i < NW; i += kBlock) dst[i] = src[i];
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------
template <class M>
int assign_lm_reserve(AssignJob &J, uint32_t chunks) {
  AssignBufs &B = *J.B;
  MANYCHK(many_grow(B.d_start, (size_t)kAssignMaxModels * 16));
  MANYCHK(many_grow(B.d_presence, (size_t)chunks));
  MANYCHK(many_grow(B.d_lm_partials, (size_t)chunks * J.n_models * M::NMOM_LM));
  MANYCHK(many_grow(B.d_lm_mask, 1));
  MANYCHK(many_grow(B.d_lm_live, 1));
  MANYCHK(many_grow(B.d_lm_state, (size_t)kAssignMaxModels));
  MANYCHK(many_grow(B.d_lm_out, (size_t)kAssignMaxModels));
  return LSQR_OK;
}

// The refit of one round.  The pass has left the moments of the labels `lab` in B.d_partials and the presence words in
// B.d_presence.  Per evaluation: one pass, one step, one 4-byte read of the live counter.  Every lm_advance call
// consumes one evaluation and stops at maxfev, so maxfev evaluations finish every model (many_lm_run's bound).
template <class M>
int assign_lm_run(AssignJob &J, const int32_t *lab, uint32_t chunks) {
  AssignBufs &B = *J.B;
  const int nm = (int)J.n_models, org_off = fit_origin_offset<M>(J.cfg);
  int n = 0, maxfev = 0;
  double ftol = 0, xtol = 0, gtol = 0;
  lm_settings(J.cfg, &n, &ftol, &xtol, &gtol, &maxfev);
  uint32_t *h_live = (uint32_t *)(B.h_pin.get() + kAssignPinLive);
  hipLaunchKernelGGL((k_assign_solve<M>), dim3(nm), dim3(kBlock), 0, J.stream, B.d_partials, chunks, nm, org_off, J.mc,
                     B.d_rows, B.d_cnt, B.d_start);
  MANYCHK(hipGetLastError());
  hipLaunchKernelGGL((k_assign_lm_init<M>), dim3(1), dim3(64), 0, J.stream, B.d_start, nm, n, ftol, xtol, gtol, maxfev,
                     B.d_cnt, B.d_lm_state, B.d_lm_out, B.d_lm_mask, B.d_lm_live);
  MANYCHK(hipGetLastError());
  MANYCHK(hipMemsetAsync(B.d_lm_partials, 0, sizeof(double) * (size_t)chunks * nm * M::NMOM_LM, J.stream));
  for (int round = 0;; round++) {
    if (round > maxfev) {
      snprintf(J.err, sizeof J.err, "LM stage: %u models still live after %d evaluations", *h_live, round);
      return LSQR_ERR_HIP;
    }
    hipLaunchKernelGGL((k_assign_lm_pass<M>), dim3(chunks), dim3(kBlock), 0, J.stream, J.data, J.stride, J.n, lab,
                       B.d_presence, B.d_lm_mask, B.d_lm_state, nm, J.mc, B.d_lm_partials);
    MANYCHK(hipGetLastError());
    hipLaunchKernelGGL((k_assign_lm_step<M>), dim3(nm), dim3(kBlock), 0, J.stream, B.d_lm_partials, chunks, nm, J.mc,
                       B.d_lm_state, B.d_rows, B.d_cnt, B.d_lm_out, B.d_lm_mask, B.d_lm_live);
    MANYCHK(hipGetLastError());
    MANYCHK(hipMemcpyAsync(h_live, B.d_lm_live, sizeof(uint32_t), hipMemcpyDeviceToHost, J.stream));
    MANYCHK(hipStreamSynchronize(J.stream));
    if (*h_live == 0) break;
  }
  return LSQR_OK;
}
#endif  // __HIPCC__

}  // namespace lsqr
