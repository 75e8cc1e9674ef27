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
struct AssignDenseGrpBufs {  // owned by the context, beside AssignGrpBufs, grown on demand
  DevBuf<double> d_mom, d_ddpart;
  DevBuf<SolveOut> d_out;
  DevBuf<int> d_flags;
  DevBuf<uint32_t> d_list;
  DevBuf<uint8_t> d_mask;
  DevBuf<uint64_t> d_wbase;
};

// Both calls (J.refine says which).  Returns after the stream has drained; the outputs are written only then.  J.B: the
// grouped calls' buffers; D: this file's; dense_fast, dense_dd: the context's options.
template <int NR>
int assign_dense_grouped_run(AssignGrpJob &J, AssignDenseGrpBufs &D, int dense_fast, int dense_dd) {
  typedef unsigned long long ull;
  constexpr uint32_t CH = kAssignDenseChunk<NR>;
  constexpr size_t lds_pass = sizeof(double) * CH * (NR + 1);
  AssignGrpBufs &B = *J.B;
  ManyBufs &P = *J.pack.buf;
  hipStream_t stream = J.pack.stream;
  const size_t NG = J.n_groups, MM = J.max_models, N = J.n, NRW = NG * MM;
  const size_t W = (size_t)J.pack.W;  // n + 1
  const int dim = (int)J.cfg.dim, ps = many_dense_ps(dim), ne = (dim + 1) * (dim + 2) / 2;

  std::vector<uint64_t> off;
  const int st = grouped_pack(J.pack, J.data, J.stride, N, J.groups, J.on_device, off);
  if (st != LSQR_OK) {
    memcpy(J.err, J.pack.err, sizeof J.err);
    return st;
  }
  const uint64_t NT = off[NG];
  const uint32_t *perm = P.d_grp_vals[1];

  // the layout: the (group, chunk) workgroups, each group's place in the partials and among the workgroups, the
  // (group, model) pairs
  std::vector<uint2> wgs, pairs;
  std::vector<uint64_t> gbase(NG, 0), wbase(NG, 0);
  uint64_t pblocks = 0;
  bool dead_records = false;  // rows of a group that runs nothing
  for (size_t g = 0; g < NG; g++) {
    const uint64_t ng = off[g + 1] - off[g];
    const size_t nm = J.n_models[g];
    if (ng && !nm) dead_records = true;
    if (!ng || !nm) continue;
    const uint32_t chunks = (uint32_t)((ng + CH - 1) / CH);
    gbase[g] = pblocks;
    wbase[g] = wgs.size();
    pblocks += (uint64_t)chunks * nm;
    for (uint32_t q = 0; q < chunks; q++) wgs.push_back(make_uint2((uint32_t)g, q));
    for (size_t m = 0; m < nm; m++) pairs.push_back(make_uint2((uint32_t)g, (uint32_t)m));
  }
  const size_t NW = wgs.size(), NP = pairs.size();
  const bool moments = J.refine && J.max_rounds > 0 && NW > 0;

  // device words: changed[NG], counts / used / ok / route [NRW] each, rounds[NG], going, flagged
  const size_t c_counts = NG, c_used = c_counts + NRW, c_ok = c_used + NRW, c_route = c_ok + NRW,
               c_rounds = c_route + NRW, c_going = c_rounds + NG, c_words = c_going + 2;
  // pinned: what goes up, then what comes down
  const size_t u_rows = 0, u_gbase = u_rows + sizeof(double) * NRW * NR, u_wbase = u_gbase + sizeof(uint64_t) * NG,
               u_wgs = u_wbase + sizeof(uint64_t) * NG, u_pairs = u_wgs + sizeof(uint2) * NW,
               u_nm = u_pairs + sizeof(uint2) * NP, u_state = u_nm + asg_grp_up8(sizeof(int32_t) * NG),
               v_going = u_state + asg_grp_up8(sizeof(uint32_t) * NG), v_rows = v_going + 2 * sizeof(ull),
               v_cnt = v_rows + sizeof(double) * NRW * NR, v_conv = v_cnt + sizeof(ull) * c_words,
               v_list = v_conv + asg_grp_up8(sizeof(uint32_t) * NG), pin_bytes = v_list + sizeof(uint32_t) * NP;
  MANYCHK(many_grow_pinned(B.h_pin, pin_bytes));  // (every earlier call ended in a synchronisation)
  char *pin = B.h_pin.get();
  double *h_up = (double *)(pin + u_rows);
  int32_t *h_nm = (int32_t *)(pin + u_nm);
  uint32_t *h_state = (uint32_t *)(pin + u_state);
  const ull *h_going = (const ull *)(pin + v_going);  // [0]: the groups still going; [1]: the flagged pairs
  const double *h_rows = (const double *)(pin + v_rows);
  const ull *h_cnt = (const ull *)(pin + v_cnt);
  const uint32_t *h_conv = (const uint32_t *)(pin + v_conv);
  const uint32_t *h_list = (const uint32_t *)(pin + v_list);
  for (size_t g = 0; g < NG; g++) {
    const size_t nm = J.n_models[g];
    h_nm[g] = (int32_t)nm;
    h_state[g] = (off[g + 1] > off[g] && nm) ? 0u : 1u;
    for (size_t m = 0; m < MM; m++)  // the zero-padded scan rows (AssignDense::rows_up)
      for (size_t j = 0; j < (size_t)NR; j++)
        h_up[(g * MM + m) * NR + j] = m < nm && j < (size_t)dim ? J.params[(g * MM + m) * dim + j] : 0.0;
  }
  memcpy(pin + u_gbase, gbase.data(), sizeof(uint64_t) * NG);
  memcpy(pin + u_wbase, wbase.data(), sizeof(uint64_t) * NG);
  if (NW) memcpy(pin + u_wgs, wgs.data(), sizeof(uint2) * NW);
  if (NP) memcpy(pin + u_pairs, pairs.data(), sizeof(uint2) * NP);

  MANYCHK(many_grow(B.d_nm, NG));
  MANYCHK(many_grow(B.d_gbase, NG));
  MANYCHK(many_grow(D.d_wbase, NG));
  MANYCHK(many_grow(B.d_state, 2 * NG));  // state, converged
  MANYCHK(many_grow(B.d_cnt, c_words));
  MANYCHK(many_grow(B.d_rows, std::max<size_t>(NRW * NR, 1)));
  MANYCHK(many_grow(B.d_wgs, std::max<size_t>(NW, 1)));
  MANYCHK(many_grow(B.d_pairs, std::max<size_t>(NP, 1)));
  MANYCHK(many_grow(B.d_labels[0], std::max<size_t>(NT, 1)));
  if (J.refine) MANYCHK(many_grow(B.d_labels[1], std::max<size_t>(NT, 1)));
  if (J.residuals_out) MANYCHK(many_grow(B.d_res, std::max<size_t>(NT, 1)));
  if (moments) {
    MANYCHK(many_grow(B.d_partials, (size_t)pblocks * ps));
    MANYCHK(many_grow(B.d_presence, NW));
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
  if (!J.on_device && J.labels_out) MANYCHK(many_grow(B.d_lab_out, N));
  if (!J.on_device && J.residuals_out) MANYCHK(many_grow(B.d_res_out, N));
  ull *d_changed = B.d_cnt, *d_counts = B.d_cnt + c_counts, *d_used = B.d_cnt + c_used, *d_ok = B.d_cnt + c_ok,
      *d_route = B.d_cnt + c_route, *d_rounds = B.d_cnt + c_rounds, *d_going = B.d_cnt + c_going;
  uint32_t *d_state = B.d_state, *d_conv = B.d_state + NG;

  MANYCHK(hipMemcpyAsync(B.d_nm, h_nm, sizeof(int32_t) * NG, hipMemcpyHostToDevice, stream));
  MANYCHK(hipMemcpyAsync(B.d_gbase, pin + u_gbase, sizeof(uint64_t) * NG, hipMemcpyHostToDevice, stream));
  MANYCHK(hipMemcpyAsync(D.d_wbase, pin + u_wbase, sizeof(uint64_t) * NG, hipMemcpyHostToDevice, stream));
  MANYCHK(hipMemcpyAsync(d_state, h_state, sizeof(uint32_t) * NG, hipMemcpyHostToDevice, stream));
  MANYCHK(hipMemsetAsync(d_conv, 0, sizeof(uint32_t) * NG, stream));
  MANYCHK(hipMemsetAsync(B.d_cnt, 0, sizeof(ull) * c_words, stream));
  if (NW) {
    MANYCHK(hipMemcpyAsync(B.d_rows, h_up, sizeof(double) * NRW * NR, hipMemcpyHostToDevice, stream));
    MANYCHK(hipMemcpyAsync(B.d_wgs, pin + u_wgs, sizeof(uint2) * NW, hipMemcpyHostToDevice, stream));
    MANYCHK(hipMemcpyAsync(B.d_pairs, pin + u_pairs, sizeof(uint2) * NP, hipMemcpyHostToDevice, stream));
  }
  if (dead_records && NT) {  // no pass writes them
    MANYCHK(hipMemsetAsync(B.d_labels[0], 0xFF, sizeof(int32_t) * NT, stream));
    if (J.refine) MANYCHK(hipMemsetAsync(B.d_labels[1], 0xFF, sizeof(int32_t) * NT, stream));
    if (J.residuals_out) {
      hipLaunchKernelGGL(k_asg_grp_fill, dim3(grp_grid(NT)), dim3(kBlock), 0, stream, B.d_res, (uint64_t)NT,
                         __builtin_inf());
      MANYCHK(hipGetLastError());
    }
  }

  const AsgGrpTab T{P.d_grp_off, B.d_gbase, B.d_nm, d_state};
  int cur = 0;
  size_t r = 0;
  bool dd_ready = false;
  while (NW) {
    const bool last = r == J.max_rounds;
    int32_t *lab = B.d_labels[cur];
    double *res = J.residuals_out ? B.d_res.get() : nullptr;
    const int32_t *old = r > 0 ? B.d_labels[cur ^ 1].get() : nullptr;
    if (last)
      hipLaunchKernelGGL((k_asd_grp_pass<NR, false>), dim3((unsigned)NW), dim3(kAsdBlock), lds_pass, stream, P.d_data, W,
                         B.d_wgs, T, B.d_rows, (int)MM, dim, J.mc, lab, res, old, d_changed, d_counts, nullptr, ps,
                         nullptr);
    else
      hipLaunchKernelGGL((k_asd_grp_pass<NR, true>), dim3((unsigned)NW), dim3(kAsdBlock), lds_pass, stream, P.d_data, W,
                         B.d_wgs, T, B.d_rows, (int)MM, dim, J.mc, lab, res, old, d_changed, d_counts, B.d_partials, ps,
                         B.d_presence);
    MANYCHK(hipGetLastError());
    if (last) break;  // every group still going stops here: nothing to read
    MANYCHK(hipMemsetAsync(d_going, 0, 2 * sizeof(ull), stream));
    hipLaunchKernelGGL(k_asg_grp_decide, dim3(grp_grid(NG)), dim3(kBlock), 0, stream, (uint32_t)NG, (ull)r, 0,
                       d_changed, d_state, d_rounds, d_conv, d_going);
    MANYCHK(hipGetLastError());
    // the sum and the solve of the groups that go on, under way before the host knows which those are
    hipLaunchKernelGGL(k_asd_grp_sum, dim3((unsigned)NP, (ne + 1 + kAsdBlock - 1) / kAsdBlock), dim3(kAsdBlock), 0,
                       stream, B.d_pairs, T, D.d_wbase, CH, B.d_partials, B.d_presence, (int)MM, dim, ps, d_counts,
                       D.d_mom);
    MANYCHK(hipGetLastError());
    if (dense_dd) MANYCHK(hipMemsetAsync(D.d_flags, 0, sizeof(int) * NP, stream));
    hipLaunchKernelGGL(k_asd_grp_solve, dim3((unsigned)NP), dim3(256), many_dense_lds(dim), stream, B.d_pairs, d_state,
                       D.d_mom, ps, dim, dense_fast, D.d_out, dense_dd ? D.d_flags.get() : (int *)nullptr);
    MANYCHK(hipGetLastError());
    if (dense_dd) {
      hipLaunchKernelGGL(k_asd_grp_flagged, dim3(grp_grid(NP)), dim3(kAsdBlock), 0, stream, D.d_flags, (uint32_t)NP,
                         D.d_list, d_going + 1);
      MANYCHK(hipGetLastError());
    }
    MANYCHK(hipMemcpyAsync(pin + v_going, d_going, 2 * sizeof(ull), hipMemcpyDeviceToHost, stream));
    MANYCHK(hipStreamSynchronize(stream));  // the two words of the round
    if (h_going[0] == 0) break;
    if (h_going[1]) {  // the ill-conditioned pairs again from their group's rows, in double-double
      const size_t nf = (size_t)h_going[1];
      MANYCHK(hipMemcpyAsync(pin + v_list, D.d_list, sizeof(uint32_t) * nf, hipMemcpyDeviceToHost, stream));
      MANYCHK(hipStreamSynchronize(stream));
      if (!dd_ready) {
        MANYCHK(many_grow(D.d_ddpart, (size_t)2 * kDdNe * kDdBlocks));
        MANYCHK(many_grow(D.d_mask, (size_t)NT));
        (void)hipFuncSetAttribute((const void *)k_dense_dd_solve, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)dense_dd_lds(64));
        dd_ready = true;
      }
      for (size_t f = 0; f < nf; f++) {
        const uint32_t p = h_list[f];
        if (p >= NP) {
          snprintf(J.err, sizeof J.err, "flagged pair out of range");
          return LSQR_ERR_HIP;
        }
        const uint32_t g = pairs[p].x, m = pairs[p].y;
        const uint32_t ng = (uint32_t)(off[g + 1] - off[g]);
        const int nb = (int)std::min<size_t>(kDdBlocks, ((size_t)ng + 31) / 32);
        uint8_t *mask = D.d_mask.get() + off[g];
        hipLaunchKernelGGL(k_asd_label_mask, dim3(std::min<uint32_t>((ng + 255) / 256, 4096u)), dim3(256), 0, stream,
                           lab + off[g], ng, (int32_t)m, mask);
        MANYCHK(hipGetLastError());
        hipLaunchKernelGGL((k_gram_dd_dense<32>), dim3(nb), dim3(256), 0, stream, P.d_data.get() + off[g] * W, W,
                           (size_t)0, (size_t)ng, dim, mask, D.d_flags + p, D.d_ddpart);
        MANYCHK(hipGetLastError());
        hipLaunchKernelGGL(k_dense_dd_solve, dim3(1), dim3(256), dense_dd_lds(dim), stream, D.d_ddpart, nb, dim,
                           D.d_mom + (size_t)p * ps, D.d_flags + p, D.d_out + p);
        MANYCHK(hipGetLastError());
      }
    }
    hipLaunchKernelGGL(k_asd_grp_apply, dim3((unsigned)NP), dim3(64), 0, stream, B.d_pairs, d_state, D.d_out, dim, NR,
                       (int)MM, B.d_rows, d_counts, d_used, d_ok, d_route);
    MANYCHK(hipGetLastError());
    r++;
    cur ^= 1;
  }
  if (NW && r == J.max_rounds) {  // the last pass allowed: its decision needs no answer
    hipLaunchKernelGGL(k_asg_grp_decide, dim3(grp_grid(NG)), dim3(kBlock), 0, stream, (uint32_t)NG, (ull)r, 1,
                       d_changed, d_state, d_rounds, d_conv, d_going);
    MANYCHK(hipGetLastError());
  }

  // results: the labels of the last pass in upload order, then the rows and the per-group words
  if (J.labels_out) {
    int32_t *d_lab = J.on_device ? J.labels_out : B.d_lab_out.get();
    hipLaunchKernelGGL(k_grp_scatter_labels, dim3(grp_grid(N)), dim3(kBlock), 0, stream, perm, (uint32_t)N,
                       (uint32_t)NT, B.d_labels[cur].get(), d_lab);
    MANYCHK(hipGetLastError());
    if (!J.on_device)
      MANYCHK(hipMemcpyAsync(J.labels_out, d_lab, sizeof(int32_t) * N, hipMemcpyDeviceToHost, stream));
  }
  if (J.residuals_out) {
    double *d_r = J.on_device ? J.residuals_out : B.d_res_out.get();
    hipLaunchKernelGGL(k_grp_scatter_f64, dim3(grp_grid(N)), dim3(kBlock), 0, stream, perm, (uint32_t)N, (uint32_t)NT,
                       B.d_res.get(), __builtin_inf(), d_r);
    MANYCHK(hipGetLastError());
    if (!J.on_device)
      MANYCHK(hipMemcpyAsync(J.residuals_out, d_r, sizeof(double) * N, hipMemcpyDeviceToHost, stream));
  }
  if (r > 0) MANYCHK(hipMemcpyAsync(pin + v_rows, B.d_rows, sizeof(double) * NRW * NR, hipMemcpyDeviceToHost, stream));
  MANYCHK(hipMemcpyAsync(pin + v_cnt, B.d_cnt, sizeof(ull) * c_words, hipMemcpyDeviceToHost, stream));
  MANYCHK(hipMemcpyAsync(pin + v_conv, d_conv, sizeof(uint32_t) * NG, hipMemcpyDeviceToHost, stream));
  MANYCHK(hipStreamSynchronize(stream));

  for (size_t g = 0; g < NG; g++) {
    const size_t nm = J.n_models[g];
    const uint64_t ng = off[g + 1] - off[g];
    const size_t rg = (size_t)h_cnt[c_rounds + g];
    if (rg > 0)
      for (size_t m = 0; m < nm; m++)
        for (int j = 0; j < dim; j++) J.params[(g * MM + m) * dim + j] = h_rows[(g * MM + m) * NR + j];
    if (J.counts_out) {
      uint64_t sum = 0, *c = J.counts_out + g * (MM + 1);
      for (size_t m = 0; m < MM; m++) sum += (c[m] = m < nm ? h_cnt[c_counts + g * MM + m] : 0);
      c[MM] = ng - sum;
    }
    if (!J.refine) continue;
    J.rounds_out[g] = rg;
    J.converged_out[g] = (int32_t)h_conv[g];
    for (size_t m = 0; m < MM; m++) {
      const size_t e = g * MM + m;
      if (m < nm) {
        assign_fit_out(rg, h_cnt[c_ok + e], h_cnt[c_used + e], (int32_t)dim, &J.status_out[e], &J.fits[e]);
        if (rg > 0) J.fits[e].reserved = (int32_t)h_cnt[c_route + e];
      } else {
        J.status_out[e] = LSQR_ERR_STATE;  // model not there
        memset(&J.fits[e], 0, sizeof(lsqr_fit_info));
      }
    }
  }
  if (J.offsets_out) memcpy(J.offsets_out, off.data(), sizeof(uint64_t) * (NG + 1));
  return LSQR_OK;
}
#endif  // __HIPCC__

#undef MANYCHK

}  // namespace lsqr
