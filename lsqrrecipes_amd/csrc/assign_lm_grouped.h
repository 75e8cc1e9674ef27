// assign_lm_grouped.h -- lsqr_refine_lm_grouped: the grouped round loop (assign_grouped.h: assign_grouped_rounds) for
// the sphere with LSQR_LS_GEOMETRIC, as the family AssignGrpLm<M>.  Group g is decided bit for bit as lsqr_refine_lm
// (assign_lm.h) decides it on a fresh context that holds the group's records alone.  The refit of a round is the
// algebraic refit of every group still going, kept aside as the START, and then one Levenberg-Marquardt run per
// (group, model), all of them in lock-step evaluation rounds over the packed records.
//
//   k_asg_grp_pass<M, true>   as in lsqr_refine_grouped; it also stores the presence word of every (group, chunk)
//   k_asg_grp_solve<M, true>  as in lsqr_refine_grouped, but into the start rows (its START flag): the rows stay
//   k_asg_grp_lm_init         one wave per group still going, one lane per model: lm_init from its start row where the
//                             algebraic refit gave one; the group's live mask; the live models of all groups added into
//                             ONE counter; ok[g][m] cleared (the LM decides it)
//   per evaluation:
//   k_asg_grp_lm_pass         one workgroup per (group, chunk): todo = presence[wg] & mask[g]; a workgroup whose group
//                             has stopped, or whose chunk holds no record of a live model, returns at once; any other
//                             runs assign_lm_pass_chunk (assign_lm.h) on the group's packed chunk with the group's
//                             LmState block -> partials [gbase[g] + q * nm[g] + m][M::NMOM_LM]
//   k_asg_grp_lm_step         one wave per (group, model) whose bit is live: the blocks of the group's chunks summed in
//                             chunk order by one lane per moment (sixteen loads in flight, added in order, as
//                             k_asg_grp_solve), LmState staged in LDS, lane 0 runs lm_advance.  A model that finishes
//                             writes its AssignLmOut and, with info in 1..4, its new scan row by assign_make_row and
//                             ok[g][m]; then it leaves the group's mask and the live counter, which the host reads (4
//                             bytes) after every evaluation, for all groups together.
//
// Why the bits are lsqr_refine_lm's.  The pass body is the same function, assign_lm_pass_chunk, on the same records at
// the same positions inside their chunk (chunk q of the group is chunk q of the fresh context), with the same trial
// point.  The step's sum starts from 0.0 and adds the chunks' blocks one by one in chunk order: that is the order of
// assign_sum_chunks, which k_assign_lm_step uses -- tiles through LDS there, sixteen registers here, the additions the
// same; the two sums are the only code of the stage that exists twice.  A model starts in assign_lm_start, its LmState
// travels by assign_lm_stage, and it finishes in assign_lm_finish (lm_finalize, assign_make_row, the ok word): both
// pairs of kernels call these functions of assign_lm.h, and both drivers run assign_lm_evals.  Nothing is summed with a
// floating-point atomic; the one counter that all groups share is an integer.  So a group's results depend on its own
// records and rows alone.
//
// A model absent from a chunk has zeros there: the LM partials are cleared once per refit round (the labels, and so the
// presence words, are fixed for the round), and the pass writes only the blocks of models that are present and live.
// A stopped group keeps its rows, its ok / used words and its AssignLmOut as its last refit left them.
//
// Budget: LDS of the pass 2 x 4 x NMOM_LM doubles (3.4 KiB at D = 8); of the step the moment block and LmState (2.3
// KiB).  Registers of the pass: assign_lm_pass_chunk's, plus the workgroup's table entries in
// scalar registers.  See DESIGN.md section 14.3.
//
// AssignGrpLm<M> derives from AssignGrpClosed<M> as AssignLm<M> (assign_lm.h) does from AssignClosed<M>: its reserve
// adds the stage's buffers, its pass hands over d_presence, and its refit is the stage.
#pragma once
#include "assign_grouped.h"
#include "assign_lm.h"

namespace lsqr {

#if defined(__HIPCC__)
// group blockIdx.x.  start: the start rows k_asg_grp_solve left; okf[g][m]: its answer, cleared here; *live (zeroed by
// the caller) += the models that start
template <class M>
__global__ __launch_bounds__(64) void k_asg_grp_lm_init(AsgGrpTab T, const double *__restrict__ start, int max_models,
                                                        int n, double ftol, double xtol, double gtol, int maxfev,
                                                        unsigned long long *__restrict__ okf,
                                                        LmState *__restrict__ st, AssignLmOut *__restrict__ out,
                                                        unsigned long long *__restrict__ mask,
                                                        uint32_t *__restrict__ live) {
  const uint32_t g = blockIdx.x;
  if (T.state[g]) return;
  const int m = threadIdx.x;
  const size_t e = (size_t)g * max_models + m;  // (read only where the row is there)
  const unsigned long long all =
      assign_lm_start<M>(m < T.nm[g], okf + e, out + e, st + e, start + e * M::SP, n, ftol, xtol, gtol, maxfev);
  if (m == 0) {
    mask[g] = all;
    if (all) atomicAdd(live, (uint32_t)__popcll(all));
  }
}

// workgroup blockIdx.x = (group, chunk) wgs[blockIdx.x].  data, labels: packed order; presence: one word per
// workgroup; mask: one word per group; st: [group][max_models]; partials: cleared at the start of the refit round
template <class M>
__global__ __launch_bounds__(kBlock) void k_asg_grp_lm_pass(const double *__restrict__ data, size_t stride,
                                                            const uint2 *__restrict__ wgs, AsgGrpTab T,
                                                            const int32_t *__restrict__ labels,
                                                            const unsigned long long *__restrict__ presence,
                                                            const unsigned long long *__restrict__ mask,
                                                            const LmState *__restrict__ st, int max_models,
                                                            ModelConsts mc, double *__restrict__ partials) {
  const uint2 wg = wgs[blockIdx.x];  // workgroup-uniform: the group, its chunk
  const uint32_t g = wg.x;
  if (T.state[g]) return;
  const unsigned long long t = presence[blockIdx.x] & mask[g];  // (uniform addresses)
  const unsigned long long todo = wave_uniform64(t);
  if (!todo) return;
  const int n_models = T.nm[g];
  const uint64_t c0 = T.offsets[g] + (uint64_t)wg.y * kAssignChunk, left = T.offsets[g + 1] - c0;
  assign_lm_pass_chunk<M>(data + c0 * stride, stride, left < kAssignChunk ? (uint32_t)left : kAssignChunk, labels + c0,
                          todo, st + (size_t)g * max_models, mc,
                          partials + (T.gbase[g] + (uint64_t)wg.y * n_models) * M::NMOM_LM);
}

// one wave per (group, model) pair: the evaluation's block of a model that is still live, then lm_advance
template <class M>
__global__ __launch_bounds__(64) void k_asg_grp_lm_step(const uint2 *__restrict__ pairs, AsgGrpTab T,
                                                        const double *__restrict__ partials, int max_models,
                                                        ModelConsts mc, LmState *__restrict__ st,
                                                        double *__restrict__ rows, unsigned long long *__restrict__ okf,
                                                        AssignLmOut *__restrict__ out, unsigned long long *mask,
                                                        uint32_t *live) {
  constexpr int N = M::NMOM_LM, U = 16;
  static_assert(N <= 64, "one lane per moment");
  __shared__ double mom[LM_MOM_MAX];
  __shared__ LmState S;
  const uint2 pr = pairs[blockIdx.x];
  const uint32_t g = pr.x, m = pr.y;
  if (T.state[g]) return;
  if (!((mask[g] >> m) & 1ull)) return;  // finished, or never started (uniform over the wave)
  const int k = threadIdx.x;
  const size_t e = (size_t)g * max_models + m;
  if (k < N) {
    const uint32_t chunks = (uint32_t)((T.offsets[g + 1] - T.offsets[g] + kAssignChunk - 1) / kAssignChunk);
    const size_t qs = (size_t)T.nm[g] * N;  // from one chunk's block of model m to the next chunk's
    const double *src = partials + (T.gbase[g] + m) * N + k;
    double t = 0.0;
    uint32_t q = 0;
    for (; q + U <= chunks; q += U) {  // U loads in flight, added in chunk order
      double v[U];
#pragma unroll
      for (int u = 0; u < U; u++) v[u] = src[(size_t)(q + u) * qs];
#pragma unroll
      for (int u = 0; u < U; u++) t += v[u];
    }
    for (; q < chunks; q++) t += src[(size_t)q * qs];
    mom[k] = t;
  }
  assign_lm_stage<64>(&st[e], &S);
  __syncthreads();
  if (k == 0 && !lm_advance(S, mom))
    assign_lm_finish<M>(S, mc, (int)m, rows + e * M::SP, okf + e, out + e, mask + g, live);
  __syncthreads();
  assign_lm_stage<64>(&S, &st[e]);
}

// ---- host side -----------------------------------------------------------------------------------------------------
// lsqr_refine_lm_grouped's family: AssignGrpClosed<M> whose pass also leaves the presence words and whose refit is the
// LM stage, for every group still going.  The pass has left the moments of the packed labels `lab` in d_partials and
// the presence words in d_presence; the refit is the algebraic solve into the start rows, k_asg_grp_lm_init, the LM
// partials cleared, then the evaluations (assign_lm_evals, assign_lm.h).
template <class M>
struct AssignGrpLm : AssignGrpClosed<M> {
  typedef AssignGrpClosed<M> Base;
  using Base::B;

  // the family's own of h_pin: the live counter's copy, then an AssignLmOut per (group, model)
  static size_t pin_own(const AssignGrpLayout &L) { return sizeof(unsigned long long) + sizeof(AssignLmOut) * L.NE; }
  static AssignLmOut *h_lm(const AssignGrpLayout &L) { return (AssignLmOut *)(L.h(L.v_own) + 8); }

  int reserve(AssignGrpJob &J, bool moments) {
    const int st = Base::reserve(J, moments);
    if (st != LSQR_OK || !moments) return st;
    const AssignGrpLayout &L = J.L;
    MANYCHK(many_grow(B.d_start, L.NE * M::SP));
    MANYCHK(many_grow(B.core.d_presence, L.NW));
    MANYCHK(many_grow(B.d_lm_partials, (size_t)L.pblocks * M::NMOM_LM));
    MANYCHK(many_grow(B.d_lm_mask, L.NG));
    MANYCHK(many_grow(B.d_lm_live, 1));
    MANYCHK(many_grow(B.d_lm_state, L.NE));
    MANYCHK(many_grow(B.d_lm_out, L.NE));
    return LSQR_OK;
  }
  int pass(AssignGrpJob &J, bool last, int32_t *lab, double *res, const int32_t *old) {
    return Base::pass_to(J, last, lab, res, old, B.core.d_presence.get());
  }
  int refit(AssignGrpJob &J, const int32_t *lab) {
    const AssignGrpLayout &L = J.L;
    AssignGrpCore &C = B.core;
    hipStream_t stream = J.pack.stream;
    unsigned long long *d_ok = L.d(L.c_ok);
    const int MM = (int)J.max_models;
    int n = 0, maxfev = 0;
    double ftol = 0, xtol = 0, gtol = 0;
    lm_settings(J.cfg, &n, &ftol, &xtol, &gtol, &maxfev);
    const int st = Base::template solve_to<true>(J, B.d_start.get());
    if (st != LSQR_OK) return st;
    MANYCHK(hipMemsetAsync(B.d_lm_live, 0, sizeof(uint32_t), stream));
    hipLaunchKernelGGL((k_asg_grp_lm_init<M>), dim3((unsigned)L.NG), dim3(64), 0, stream, L.T, B.d_start.get(), MM, n,
                       ftol, xtol, gtol, maxfev, d_ok, B.d_lm_state.get(), B.d_lm_out.get(), B.d_lm_mask.get(),
                       B.d_lm_live.get());
    MANYCHK(hipGetLastError());
    MANYCHK(hipMemsetAsync(B.d_lm_partials, 0, sizeof(double) * (size_t)L.pblocks * M::NMOM_LM, stream));
    return assign_lm_evals(
        stream, maxfev, B.d_lm_live.get(), (uint32_t *)L.h(L.v_own), J.err,
        [&] {
          hipLaunchKernelGGL((k_asg_grp_lm_pass<M>), dim3((unsigned)L.NW), dim3(kBlock), 0, stream,
                             J.pack.buf->d_data.get(), (size_t)J.pack.W, C.d_wgs.get(), L.T, lab, C.d_presence.get(),
                             B.d_lm_mask.get(), B.d_lm_state.get(), MM, J.mc, B.d_lm_partials.get());
        },
        [&] {
          hipLaunchKernelGGL((k_asg_grp_lm_step<M>), dim3((unsigned)L.NP), dim3(64), 0, stream, C.d_pairs.get(), L.T,
                             B.d_lm_partials.get(), MM, J.mc, B.d_lm_state.get(), C.d_rows.get(), d_ok,
                             B.d_lm_out.get(), B.d_lm_mask.get(), B.d_lm_live.get());
        });
  }
  int results(AssignGrpJob &J) {
    MANYCHK(hipMemcpyAsync(h_lm(J.L), B.d_lm_out, sizeof(AssignLmOut) * J.L.NE, hipMemcpyDeviceToHost, J.pack.stream));
    return LSQR_OK;
  }
  void fit_more(AssignGrpJob &J, size_t e, const unsigned long long *, lsqr_fit_info &fit) {
    const AssignLmOut &o = h_lm(J.L)[e];
    fit.lm_info = o.lm_info;
    fit.lm_nfev = o.lm_nfev;
    fit.reserved = o.stall;
    fit.cost = o.cost;
  }
};
#endif  // __HIPCC__

}  // namespace lsqr
