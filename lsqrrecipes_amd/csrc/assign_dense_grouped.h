// assign_dense_grouped.h -- lsqr_assign_dense_grouped / lsqr_refine_dense_grouped: lsqr_assign_dense / lsqr_refine_dense
// (assign_dense.h) with ONE REGRESSION SET PER LABEL over the rows the context already holds.  Group g -- the rows with
// groups[i] == g, in upload order -- is decided bit for bit as a fresh context holding just those rows, tightly packed,
// decides it with parameter rows g * max_models .. + n_models[g], the same options and the same max_rounds.
//
//   (grouped.h)           grouped_pack, once per call; every round reads the packed copy at stride n + 1.
//   k_asd_grp_pass<NR>    one workgroup of 256 lanes per (group, chunk): chunk q of group g is the group's packed rows
//                         [q * kAssignDenseChunk<NR>, (q + 1) * kAssignDenseChunk<NR>).  It finds its chunk through the
//                         (group, chunk) list, as k_asg_grp_pass (assign_grouped.h) does, and runs asd_pass_chunk
//                         (assign_dense.h), the body of k_asd_pass, on it: the changed-count and the counts per group,
//                         the partials at gbase[g] + q * n_models[g] + m, one presence word per workgroup.  The group is
//                         uniform inside a workgroup, so its scan rows are read with scalar loads.  A workgroup whose
//                         group has stopped exits at once.
//   (assign_grouped.h)    k_asg_grp_decide, one lane per group after each pass.
//   k_asd_grp_sum         per (group, model) pair of a group still going: asd_sum_entry (assign_dense.h), k_asd_sum's
//                         loop -- the chunk blocks added in chunk order, one thread per entry, 0.0 where the chunk's
//                         presence word says the model is not there; the count from the integer counter -> mom[pair][ps]
//   k_asd_grp_solve       one workgroup per pair: asd_solve_one, k_asd_solve's body -- solve_dense_wg (dense.h) where
//                         the model has at least n rows; with dense_dd a pivot below 1e-6 max|G| raises the pair's flag
//   k_asd_grp_flagged     the flagged pairs -> a device list and their number
//   (assign_dense.h, dense.h)  per flagged pair: k_asd_label_mask over the GROUP's packed range, then k_gram_dd_dense<32>
//                         + k_dense_dd_solve on that range with min(kDdBlocks, (ng + 31) / 32) blocks, ng the group's
//                         rows -- what the fresh context runs on them
//   k_asd_grp_apply       asd_apply_one, k_asd_apply's body, per pair: the new scan row, and the used / ok / route words;
//                         it zeroes the pair's count for the group's next pass
//   (grouped.h)           k_grp_scatter_labels / k_grp_scatter_f64: packed order -> upload order, every entry once.
//
// Order of the sums, per group: assign_dense.h's, with "chunk" counted inside the group -- a model's block is the sum, in
// chunk order, of its chunk blocks, each the sum in row order of its own rows.  No floating-point atomic.  A group's
// results depend on its own rows, parameter rows and n_models alone.
//
// The host side is AssignGrpDense<NR>, a family of assign_grouped.h's round loop (assign_grouped_rounds).
//
// Host traffic per round: one synchronisation and one read of two words -- the groups still going and the flagged
// pairs.  The sum, the solve and the flag list are enqueued BEFORE that read; all of them pass over the groups the
// decision has just stopped, so a converged group's solve never runs.  The list itself crosses only when it is not
// empty.  Groups stop at different rounds; what assign_grouped.h says about the two label buffers, about the groups
// that run nothing and about the records in no group holds here word for word.
//
// Device scratch: partials of sum_g chunks_g * n_models[g] * ps doubles; a moment block (ps doubles), a SolveOut and a
// flag per pair; two packed label arrays; the words; with dense_dd and a flagged pair one mask byte per packed row and
// the 9 MiB of k_gram_dd_dense's partials.  A buffer that cannot be had ends the call with LSQR_ERR_HIP.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "assign_dense.h"
#include "assign_grouped.h"

namespace lsqr {

#if defined(__HIPCC__)
// data: the packed rows, `stride` doubles apart; wgs: (group, chunk) per workgroup; rows: n_groups * max_models scan
// rows of NR doubles; labels / residuals (nullable) / old (nullable): packed order; changed: one word per group; counts:
// max_models words per group, zero for every group still going; partials (WITH_MOMENTS): [gbase[g] + q * nm[g] + m][ps];
// presence (WITH_MOMENTS): one word per workgroup.  Dynamic LDS: kAssignDenseChunk<NR> * (NR + 1) doubles.
template <int NR, bool WITH_MOMENTS>
__global__ __launch_bounds__(kAsdBlock) void k_asd_grp_pass(
    const double *__restrict__ data, size_t stride, const uint2 *__restrict__ wgs, AsgGrpTab T,
    const double *__restrict__ rows, int max_models, int dim, ModelConsts mc, int32_t *__restrict__ labels,
    double *__restrict__ residuals, const int32_t *__restrict__ old, unsigned long long *__restrict__ changed,
    unsigned long long *__restrict__ counts, double *__restrict__ partials, int ps,
    unsigned long long *__restrict__ presence) {
  constexpr uint32_t CH = kAssignDenseChunk<NR>;
  const uint2 wg = wgs[blockIdx.x];  // workgroup-uniform: the group, its chunk
  const uint32_t g = wg.x;
  if (T.state[g]) return;
  const int n_models = T.nm[g];
  const uint64_t c0 = T.offsets[g] + (uint64_t)wg.y * CH, left = T.offsets[g + 1] - c0;
  if constexpr (WITH_MOMENTS) {
    partials += (T.gbase[g] + (uint64_t)wg.y * n_models) * ps;
    presence += blockIdx.x;
  }
  asd_pass_chunk<NR, WITH_MOMENTS>(data + c0 * stride, stride, left < CH ? (uint32_t)left : CH, dim,
                                   rows + (size_t)g * max_models * NR, n_models, mc, labels + c0,
                                   residuals ? residuals + c0 : nullptr, old ? old + c0 : nullptr, changed + g,
                                   counts + (size_t)g * max_models, partials, ps, presence);
}

// pair blockIdx.x = (group, model) of a group still going, entries blockIdx.y * 256 + tid: the blocks of the group's
// chunks (`ch` rows each) added in chunk order; wbase[g]: the group's first workgroup, whose presence words follow
__global__ __launch_bounds__(kAsdBlock) void k_asd_grp_sum(const uint2 *__restrict__ pairs, AsgGrpTab T,
                                                           const uint64_t *__restrict__ wbase, uint32_t ch,
                                                           const double *__restrict__ partials,
                                                           const unsigned long long *__restrict__ presence,
                                                           int max_models, int n, int ps,
                                                           const unsigned long long *__restrict__ counts,
                                                           double *__restrict__ mom) {
  const uint2 pr = pairs[blockIdx.x];
  const uint32_t g = pr.x, m = pr.y;
  if (T.state[g]) return;
  const int e = blockIdx.y * kAsdBlock + threadIdx.x, ne = (n + 1) * (n + 2) / 2;
  if (e > ne) return;
  double *out = mom + (size_t)blockIdx.x * ps;
  if (e == ne) {
    out[ne] = (double)counts[(size_t)g * max_models + m];
    return;
  }
  const uint32_t chunks = (uint32_t)((T.offsets[g + 1] - T.offsets[g] + ch - 1) / ch);
  // (from one chunk's block of model m to the next chunk's: nm[g] blocks)
  out[e] = asd_sum_entry(partials + (T.gbase[g] + m) * ps + e, (size_t)T.nm[g] * ps, presence + wbase[g], (int)m,
                         chunks);
}

// one workgroup per pair.  flags (nullable: dense_dd 0, the block alone decides): one per pair, zeroed by the caller.
// Dynamic LDS: many_dense_lds(n).
__global__ __launch_bounds__(256) void k_asd_grp_solve(const uint2 *__restrict__ pairs,
                                                       const uint32_t *__restrict__ state,
                                                       const double *__restrict__ mom, int ps, int n, int fast,
                                                       SolveOut *__restrict__ out, int *__restrict__ flags) {
  const uint32_t p = blockIdx.x;
  if (state[pairs[p].x]) return;
  asd_solve_one(mom + (size_t)p * ps, n, fast, out + p, flags ? flags + p : nullptr);
}

// the flagged pairs of this round -> list (in no particular order: each is solved on its own), *n_list (zeroed by the
// caller) their number
__global__ __launch_bounds__(kAsdBlock) void k_asd_grp_flagged(const int *__restrict__ flags, uint32_t n_pairs,
                                                               uint32_t *__restrict__ list,
                                                               unsigned long long *__restrict__ n_list) {
  for (uint64_t p = (uint64_t)blockIdx.x * kAsdBlock + threadIdx.x; p < n_pairs; p += (uint64_t)gridDim.x * kAsdBlock)
    if (flags[p]) list[atomicAdd(n_list, 1ull)] = (uint32_t)p;
}

// pair blockIdx.x: what its refit gave -> its scan row (nr doubles, zero beyond n) and its used / okf / route words;
// counts[g][m] is read as the rows behind this refit attempt and zeroed for the group's next pass
__global__ __launch_bounds__(64) void k_asd_grp_apply(const uint2 *__restrict__ pairs,
                                                      const uint32_t *__restrict__ state,
                                                      const SolveOut *__restrict__ out, int n, int nr, int max_models,
                                                      double *__restrict__ rows, unsigned long long *counts,
                                                      unsigned long long *__restrict__ used,
                                                      unsigned long long *__restrict__ okf,
                                                      unsigned long long *__restrict__ route) {
  const uint32_t p = blockIdx.x;
  const uint2 pr = pairs[p];
  if (state[pr.x]) return;
  const size_t e = (size_t)pr.x * max_models + pr.y;
  const unsigned long long cnt = counts[e];
  asd_apply_one(out + p, cnt, n, nr, rows + e * nr, used + e, okf + e, route + e);
  if (threadIdx.x == 0) counts[e] = 0;
}

// ---- host side -----------------------------------------------------------------------------------------------------
struct AssignDenseGrpBufs {  // owned by the context (lsqr_ctx::assign_dense_grp), beside AssignGrpBufs, grown on demand
  DevBuf<double> d_mom, d_ddpart;
  DevBuf<SolveOut> d_out;
  DevBuf<int> d_flags;
  DevBuf<uint32_t> d_list;
  DevBuf<uint8_t> d_mask;
};

// The dense system's family of the grouped round loop (assign_grouped.h: assign_grouped_rounds), both calls.  Its own
// counter block is route; its second going word counts the flagged pairs; of h_pin it keeps their list.  Before the
// round's synchronisation it enqueues the sum, the solve and the flag list; the refit solves the flagged pairs again
// from their group's rows in double-double, then k_asd_grp_apply makes the refit decision.
template <int NR>
struct AssignGrpDense {
  static constexpr int UP = NR, SP = NR, BLOCKS = 1, GOING = 2;
  static constexpr bool WBASE = true;
  static constexpr uint32_t CH = kAssignDenseChunk<NR>;
  static constexpr size_t lds_pass = sizeof(double) * CH * (NR + 1);
  AssignGrpCore &C;       // the grouped calls' (lsqr_ctx::assign_grp)
  AssignDenseGrpBufs &D;  // this file's
  int dense_fast, dense_dd;  // the context's options
  int dim, ps;               // n, and many_dense_ps(n): the doubles of a moment block
  bool dd_ready = false;     // the double-double detour's buffers are there

  AssignGrpCore &core() { return C; }
  static uint32_t chunks_of(uint64_t n) { return (uint32_t)((n + CH - 1) / CH); }
  static size_t pin_own(const AssignGrpLayout &L) { return sizeof(uint32_t) * L.NP; }
  int reserve(AssignGrpJob &J, bool moments) {
    if (moments) {
      const size_t NP = J.L.NP;
      MANYCHK(many_grow(C.d_partials, (size_t)J.L.pblocks * ps));
      MANYCHK(many_grow(C.d_presence, J.L.NW));
      MANYCHK(many_grow(D.d_mom, NP * (size_t)ps));
      MANYCHK(many_grow(D.d_out, NP));
      if (dense_dd) {
        MANYCHK(many_grow(D.d_flags, NP));
        MANYCHK(many_grow(D.d_list, NP));
      }
      (void)hipFuncSetAttribute((const void *)k_asd_grp_solve, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)many_dense_lds(64));
      (void)hipFuncSetAttribute((const void *)(k_asd_grp_pass<NR, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds_pass);
    }
    (void)hipFuncSetAttribute((const void *)(k_asd_grp_pass<NR, false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds_pass);
    return LSQR_OK;
  }
  int rows_up(AssignGrpJob &J, double *h_rows) {  // the zero-padded scan rows (AssignDense::rows_up)
    const size_t MM = J.max_models, n = (size_t)dim;
    for (size_t g = 0; g < J.n_groups; g++)
      for (size_t m = 0; m < MM; m++)
        for (size_t j = 0; j < (size_t)NR; j++)
          h_rows[(g * MM + m) * NR + j] = m < J.n_models[g] && j < n ? J.params[(g * MM + m) * n + j] : 0.0;
    MANYCHK(hipMemcpyAsync(C.d_rows, h_rows, sizeof(double) * J.L.NE * NR, hipMemcpyHostToDevice, J.pack.stream));
    return LSQR_OK;
  }
  int prepare(AssignGrpJob &) { return LSQR_OK; }
  int pass(AssignGrpJob &J, bool last, int32_t *lab, double *res, const int32_t *old) {
    const AssignGrpLayout &L = J.L;
    const size_t W = (size_t)J.pack.W;  // n + 1
    const int MM = (int)J.max_models;
    if (last)
      hipLaunchKernelGGL((k_asd_grp_pass<NR, false>), dim3((unsigned)L.NW), dim3(kAsdBlock), lds_pass, J.pack.stream,
                         J.pack.buf->d_data, W, C.d_wgs, L.T, C.d_rows, MM, dim, J.mc, lab, res, old, L.d(0),
                         L.d(L.c_counts), nullptr, ps, nullptr);
    else
      hipLaunchKernelGGL((k_asd_grp_pass<NR, true>), dim3((unsigned)L.NW), dim3(kAsdBlock), lds_pass, J.pack.stream,
                         J.pack.buf->d_data, W, C.d_wgs, L.T, C.d_rows, MM, dim, J.mc, lab, res, old, L.d(0),
                         L.d(L.c_counts), C.d_partials, ps, C.d_presence);
    MANYCHK(hipGetLastError());
    return LSQR_OK;
  }
  // the sum and the solve of the groups that go on, under way before the host knows which those are
  int before_sync(AssignGrpJob &J) {
    const AssignGrpLayout &L = J.L;
    hipStream_t stream = J.pack.stream;
    const size_t NP = L.NP;
    const int ne = (dim + 1) * (dim + 2) / 2;
    hipLaunchKernelGGL(k_asd_grp_sum, dim3((unsigned)NP, (ne + 1 + kAsdBlock - 1) / kAsdBlock), dim3(kAsdBlock), 0,
                       stream, C.d_pairs, L.T, C.d_wbase, CH, C.d_partials, C.d_presence, (int)J.max_models, dim, ps,
                       L.d(L.c_counts), D.d_mom);
    MANYCHK(hipGetLastError());
    if (dense_dd) MANYCHK(hipMemsetAsync(D.d_flags, 0, sizeof(int) * NP, stream));
    hipLaunchKernelGGL(k_asd_grp_solve, dim3((unsigned)NP), dim3(256), many_dense_lds(dim), stream, C.d_pairs,
                       L.T.state, D.d_mom, ps, dim, dense_fast, D.d_out, dense_dd ? D.d_flags.get() : (int *)nullptr);
    MANYCHK(hipGetLastError());
    if (dense_dd) {
      hipLaunchKernelGGL(k_asd_grp_flagged, dim3(grp_grid(NP)), dim3(kAsdBlock), 0, stream, D.d_flags, (uint32_t)NP,
                         D.d_list, L.d(L.c_going) + 1);
      MANYCHK(hipGetLastError());
    }
    return LSQR_OK;
  }
  int refit(AssignGrpJob &J, const int32_t *lab) {
    const AssignGrpLayout &L = J.L;
    hipStream_t stream = J.pack.stream;
    const size_t W = (size_t)J.pack.W;
    // the ill-conditioned pairs again from their group's rows, in double-double
    if (const size_t nf = ((const unsigned long long *)L.h(L.v_going))[1]) {
      const uint32_t *h_list = (const uint32_t *)L.h(L.v_own);
      MANYCHK(hipMemcpyAsync(L.h(L.v_own), D.d_list, sizeof(uint32_t) * nf, hipMemcpyDeviceToHost, stream));
      MANYCHK(hipStreamSynchronize(stream));
      if (!dd_ready) {
        MANYCHK(many_grow(D.d_ddpart, (size_t)2 * kDdNe * kDdBlocks));
        MANYCHK(many_grow(D.d_mask, (size_t)L.off[L.NG]));
        (void)hipFuncSetAttribute((const void *)k_dense_dd_solve, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)dense_dd_lds(64));
        dd_ready = true;
      }
      for (size_t f = 0; f < nf; f++) {
        const uint32_t p = h_list[f];
        if (p >= L.NP) {
          snprintf(J.err, sizeof J.err, "flagged pair out of range");
          return LSQR_ERR_HIP;
        }
        const uint32_t g = L.pairs[p].x, m = L.pairs[p].y;
        const uint32_t ng = (uint32_t)(L.off[g + 1] - L.off[g]);
        const int nb = (int)std::min<size_t>(kDdBlocks, ((size_t)ng + 31) / 32);
        uint8_t *mask = D.d_mask.get() + L.off[g];
        hipLaunchKernelGGL(k_asd_label_mask, dim3(std::min<uint32_t>((ng + 255) / 256, 4096u)), dim3(256), 0, stream,
                           lab + L.off[g], ng, (int32_t)m, mask);
        MANYCHK(hipGetLastError());
        hipLaunchKernelGGL((k_gram_dd_dense<32>), dim3(nb), dim3(256), 0, stream,
                           J.pack.buf->d_data.get() + L.off[g] * W, W, (size_t)0, (size_t)ng, dim, mask, D.d_flags + p,
                           D.d_ddpart);
        MANYCHK(hipGetLastError());
        hipLaunchKernelGGL(k_dense_dd_solve, dim3(1), dim3(256), dense_dd_lds(dim), stream, D.d_ddpart, nb, dim,
                           D.d_mom + (size_t)p * ps, D.d_flags + p, D.d_out + p);
        MANYCHK(hipGetLastError());
      }
    }
    hipLaunchKernelGGL(k_asd_grp_apply, dim3((unsigned)L.NP), dim3(64), 0, stream, C.d_pairs, L.T.state, D.d_out, dim,
                       NR, (int)J.max_models, C.d_rows, L.d(L.c_counts), L.d(L.c_used), L.d(L.c_ok), L.d(L.c_own));
    MANYCHK(hipGetLastError());
    return LSQR_OK;
  }
  int results(AssignGrpJob &) { return LSQR_OK; }
  int32_t n_params(const AssignGrpJob &) const { return dim; }
  void fit_more(AssignGrpJob &J, size_t e, const unsigned long long *h_cnt, lsqr_fit_info &fit) {
    fit.reserved = (int32_t)h_cnt[J.L.c_own + e];  // the route
  }
};
#endif  // __HIPCC__

#undef MANYCHK

}  // namespace lsqr
