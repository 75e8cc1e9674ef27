// assign_grouped.h -- lsqr_assign_grouped / lsqr_refine_grouped: lsqr_assign / lsqr_refine (assign.h) with ONE MODEL SET
// PER LABEL over the records the context already holds.  Group g -- the records with groups[i] == g, in upload order --
// is decided bit for bit as a fresh context holding just those records, tightly packed, decides it with rows
// g * max_models .. + n_models[g].
//
//   (grouped.h)           grouped_pack, once per call: keys, the stable radix sort, offsets, its one synchronisation, the
//                         gather into the packed buffer.  Every round reads that copy (stride = the record's doubles).
//   (assign.h)            k_assign_prepare with the groups' model counts: one lane per (group, model) row that is there
//   k_asg_grp_pass        one workgroup per (group, chunk): chunk q of group g is the group's packed records
//                         [q * kAssignChunk, (q + 1) * kAssignChunk).  The host lays the (group, chunk) list out from the
//                         offsets.  The kernel finds its chunk -- the group is uniform inside a workgroup, so the group's
//                         rows are still read at wave-uniform addresses -- and runs assign_pass_chunk (assign.h) on it,
//                         with the changed-count and the counts per group and the partials at gbase[g] + q *
//                         n_models[g].  A workgroup whose group has stopped exits at once.
//   k_asg_grp_decide      one lane per group after each pass: converged (r > 0 and nothing changed), stopped at
//                         max_rounds, or going on; rounds[g]; the groups still going summed into the ONE word the host
//                         reads per round.
//   k_asg_grp_solve       one wave per (group, model) of a group still going: the partials of the group's chunks summed
//                         in chunk order by one lane per moment (sixteen loads in flight, added in order), then
//                         assign_refit (assign.h), as k_assign_solve.  No tile staging: 1.3 KiB of LDS (the moment
//                         block, the small workspace, SolveOut).
//   (grouped.h)           k_grp_scatter_labels / k_grp_scatter_f64: packed order -> upload order, every entry once.
//
// Order of the sums, per group: the lane's records j * kBlock + tid in index order, the __shfl_down tree, the four
// waves in index order, the chunks in chunk order -- assign.h's, with "chunk" counted inside the group.  No
// floating-point atomic.  A group's results depend on its own records, rows and n_models alone.
//
// Groups stop at different rounds.  Pass r writes label buffer r & 1 and compares with the other.  A converged group has
// the same labels in both; every group that stops at max_rounds stops in the same, last, pass; so the buffer of the last
// pass holds every group's final labels.  A stopped group is passed over by later passes and solves: its rows, counts
// and labels stay as its last pass left them.
//
// Groups that run nothing (no records, or n_models[g] == 0) have no workgroups and start stopped.  Their records, and
// the records in no group, get label -1 and residual +infinity: the packed buffers are filled with those first when such
// a group has records, and the scatter writes them for the records past the grouped total.
//
// lsqr_refine_lm_grouped (assign_lm_grouped.h, the geometric sphere) runs this file's loop, assign_grouped_run<M, true>:
// the pass also stores every workgroup's presence word, the solve writes into a side array of start rows, and the
// refit is a grouped LM stage.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <vector>

#include "assign.h"
#include "grouped.h"

namespace lsqr {

#if defined(__HIPCC__)
struct AsgGrpTab {  // the call's per-group tables, on the device
  const uint64_t *offsets;  // n_groups + 1 (grouped_pack)
  const uint64_t *gbase;    // first (chunk, model) block of the group's partials
  const int32_t *nm;        // n_models[g]
  uint32_t *state;          // 0: going; 1: stopped
};

// data: the packed records, `stride` doubles apart; wgs: (group, chunk) per workgroup; rows: n_groups * max_models scan
// rows; labels / residuals (nullable) / old (nullable): packed order; changed: one word per group; counts: max_models
// words per group, zero for every group still going; partials (WITH_MOMENTS): [gbase[g] + q * nm[g] + m][AccLs<M>::N];
// presence (WITH_MOMENTS, nullable): one word per workgroup (the LM stage of assign_lm_grouped.h reads it)
template <class M, bool WITH_MOMENTS>
__global__ __launch_bounds__(kBlock, (kAssignPassWaves<M, WITH_MOMENTS>)) void k_asg_grp_pass(
    const double *__restrict__ data, size_t stride, const uint2 *__restrict__ wgs, AsgGrpTab T,
    const double *__restrict__ rows, int max_models, int org_off, ModelConsts mc, int32_t *__restrict__ labels,
    double *__restrict__ residuals, const int32_t *__restrict__ old, unsigned long long *__restrict__ changed,
    unsigned long long *__restrict__ counts, double *__restrict__ partials,
    unsigned long long *__restrict__ presence) {
  const uint2 wg = wgs[blockIdx.x];  // workgroup-uniform: the group, its chunk
  const uint32_t g = wg.x;
  if (T.state[g]) return;
  const int n_models = T.nm[g];
  const uint64_t c0 = T.offsets[g] + (uint64_t)wg.y * kAssignChunk, left = T.offsets[g + 1] - c0;
  if constexpr (WITH_MOMENTS) partials += (T.gbase[g] + (uint64_t)wg.y * n_models) * AccLs<M>::N;
  assign_pass_chunk<M, WITH_MOMENTS>(data + c0 * stride, stride, left < kAssignChunk ? (uint32_t)left : kAssignChunk,
                                     rows + (size_t)g * max_models * M::SP, n_models, org_off, mc, labels + c0,
                                     residuals ? residuals + c0 : nullptr, old ? old + c0 : nullptr, changed + g,
                                     counts + (size_t)g * max_models, partials,
                                     presence ? presence + blockIdx.x : nullptr);
}

// after pass r (last: r == max_rounds): every group still going converges, stops, or goes on with a zeroed
// changed-count; *going (zeroed by the caller) += the groups that go on
__global__ __launch_bounds__(kBlock) void k_asg_grp_decide(uint32_t n_groups, unsigned long long r, int last,
                                                           unsigned long long *__restrict__ changed,
                                                           uint32_t *__restrict__ state,
                                                           unsigned long long *__restrict__ rounds,
                                                           uint32_t *__restrict__ conv,
                                                           unsigned long long *__restrict__ going) {
  uint32_t cnt = 0;
  for (uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g < n_groups; g += (uint64_t)gridDim.x * kBlock) {
    if (state[g]) continue;
    if (r > 0 && changed[g] == 0) {
      conv[g] = 1;
      rounds[g] = r;
      state[g] = 1;
    } else if (last) {
      rounds[g] = r;
      state[g] = 1;
    } else {
      changed[g] = 0;
      cnt++;
    }
  }
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(going, (unsigned long long)cnt);
}

// one wave per (group, model) pair of the groups that had work.  counts[g][m] is read as the records behind this
// refit attempt and zeroed for the group's next pass; used / okf: what k_assign_solve leaves in ASG_USED / ASG_OK;
// START (start: n_groups * max_models rows, else not read): as k_assign_solve's `start` -- `rows` is only read, and row
// e of `start` gets what `rows` would have got.  A template flag and not a nullable pointer: the pointer test moved the
// registers of 18 of the 22 instantiations, and the algebraic path keeps its code
template <class M, bool START = false>
__global__ __launch_bounds__(64) void k_asg_grp_solve(const uint2 *__restrict__ pairs, AsgGrpTab T,
                                                      const double *__restrict__ partials, int max_models, int org_off,
                                                      ModelConsts mc, double *rows, unsigned long long *counts,
                                                      unsigned long long *__restrict__ used,
                                                      unsigned long long *__restrict__ okf, double *start) {
  constexpr int N = M::NMOM, U = 16;
  static_assert(N <= 64, "one lane per moment");
  __shared__ double mom[MOM_MAX];
  __shared__ double ws[M::NMOM > 40 ? 512 : 8];
  __shared__ SolveOut so;
  const uint2 pr = pairs[blockIdx.x];
  const uint32_t g = pr.x, m = pr.y;
  if (T.state[g]) return;
  const int k = threadIdx.x;
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
  __syncthreads();
  if (k != 0) return;
  const size_t e = (size_t)g * max_models + m;
  const unsigned long long cnt = counts[e];
  counts[e] = 0;
  used[e] = cnt;
  double *row_m = rows + e * M::SP;
  if constexpr (START) {
    for (int j = 0; j < (int)M::SP; j++) start[e * M::SP + j] = row_m[j];
    row_m = start + e * M::SP;
  }
  okf[e] = assign_refit<M>(mom, row_m, cnt, org_off, mc, ws, &so) ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void k_asg_grp_fill(double *__restrict__ p, uint64_t n, double v) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) p[i] = v;
}

// ---- host side -----------------------------------------------------------------------------------------------------
struct AssignGrpBufs {  // owned by the context, grown on demand (the sort and the packed copy are ManyBufs')
  DevBuf<double> d_par, d_rows, d_partials, d_res, d_res_out;
  DevBuf<int32_t> d_labels[2], d_lab_out, d_nm;
  DevBuf<unsigned long long> d_cnt;
  DevBuf<uint64_t> d_gbase;
  DevBuf<uint32_t> d_state;
  DevBuf<uint2> d_wgs, d_pairs;
  PinBuf<char> h_pin;
  // the LM stage of lsqr_refine_lm_grouped (assign_lm_grouped.h)
  DevBuf<double> d_start, d_lm_partials;
  DevBuf<unsigned long long> d_presence, d_lm_mask;  // one word per (group, chunk); per group, the models whose LM goes on
  DevBuf<uint32_t> d_lm_live;                         // their number over all groups
  DevBuf<LmState> d_lm_state;                         // per (group, model)
  DevBuf<AssignLmOut> d_lm_out;
};

struct AssignGrpJob {
  ManyJob pack;  // grouped_pack's view of the call: stream, W, buf, n = n_groups (lsqr_hip.hip fills it)
  lsqr_model_cfg cfg{};
  ModelConsts mc{};
  const double *data = nullptr;  // the context's records: n of them, `stride` doubles apart
  size_t stride = 0, n = 0;
  AssignGrpBufs *B = nullptr;
  // the call
  const int32_t *groups = nullptr;
  size_t n_groups = 0, max_models = 0, max_rounds = 0;
  int on_device = 0;
  bool refine = false;
  double *params = nullptr;  // host, n_groups * max_models rows of M::P: read, and written where a refit ran
  const size_t *n_models = nullptr;
  int32_t *labels_out = nullptr;
  double *residuals_out = nullptr;
  uint64_t *counts_out = nullptr, *offsets_out = nullptr;
  lsqr_fit_info *fits = nullptr;
  int32_t *status_out = nullptr;
  size_t *rounds_out = nullptr;
  int32_t *converged_out = nullptr;
  char err[256] = {0};
};

inline size_t asg_grp_up8(size_t b) { return (b + 7) & ~(size_t)7; }

// what the LM stage of a round needs of the call's layout
struct AsgGrpLmView {
  AsgGrpTab T;
  const uint2 *wgs, *pairs;
  size_t n_wgs, n_pairs, n_groups, max_models;
  uint64_t pblocks;    // (chunk, model) blocks of all groups
  const double *data;  // the packed records
  size_t stride;
  double *rows;
  unsigned long long *counts, *used, *ok;
  uint32_t *h_live;  // pinned: the live counter's copy
};

// the LM stage of lsqr_refine_lm_grouped's round (assign_lm_grouped.h): its buffers, and the refit of every model of
// every group still going from the moments and the presence words the pass has just left, under the packed labels
// `lab`; it leaves the new rows in B.d_rows
template <class M> int assign_lm_grp_reserve(AssignGrpJob &J, const AsgGrpLmView &V);
template <class M> int assign_lm_grp_run(AssignGrpJob &J, const AsgGrpLmView &V, const int32_t *lab);

// All three calls.  Returns after the stream has drained; the outputs are written only then.
// LM (lsqr_refine_lm_grouped, the geometric sphere): the same loop; the refit is assign_lm_grp_run, and the fits carry
// its record.
template <class M, bool LM = false>
int assign_grouped_run(AssignGrpJob &J) {
  typedef unsigned long long ull;
  AssignGrpBufs &B = *J.B;
  ManyBufs &P = *J.pack.buf;
  hipStream_t stream = J.pack.stream;
  const size_t NG = J.n_groups, MM = J.max_models, N = J.n, NR = NG * MM;
  const size_t W = (size_t)J.pack.W;
  const int org_off = fit_origin_offset<M>(J.cfg);

  std::vector<uint64_t> off;
  const int st = grouped_pack(J.pack, J.data, J.stride, N, J.groups, J.on_device, off);
  if (st != LSQR_OK) {
    memcpy(J.err, J.pack.err, sizeof J.err);
    return st;
  }
  const uint64_t NT = off[NG];
  const uint32_t *perm = P.d_grp_vals[1];

  // the layout: the (group, chunk) workgroups, each group's place in the partials, the (group, model) pairs
  std::vector<uint2> wgs, pairs;
  std::vector<uint64_t> gbase(NG, 0);
  uint64_t pblocks = 0;
  bool dead_records = false;  // records of a group that runs nothing
  for (size_t g = 0; g < NG; g++) {
    const uint64_t ng = off[g + 1] - off[g];
    const size_t nm = J.n_models[g];
    if (ng && !nm) dead_records = true;
    if (!ng || !nm) continue;
    const uint32_t chunks = assign_chunks(ng);
    gbase[g] = pblocks;
    pblocks += (uint64_t)chunks * nm;
    for (uint32_t q = 0; q < chunks; q++) wgs.push_back(make_uint2((uint32_t)g, q));
    for (size_t m = 0; m < nm; m++) pairs.push_back(make_uint2((uint32_t)g, (uint32_t)m));
  }
  const size_t NW = wgs.size(), NP = pairs.size();
  const bool moments = J.refine && J.max_rounds > 0 && NW > 0;

  // device words: changed[NG], counts / used / ok [NR] each, rounds[NG], going
  const size_t c_counts = NG, c_used = c_counts + NR, c_ok = c_used + NR, c_rounds = c_ok + NR, c_going = c_rounds + NG,
               c_words = c_going + 1;
  // pinned: what goes up, then what comes down
  const size_t u_par = 0, u_gbase = u_par + sizeof(double) * NR * M::P, u_wgs = u_gbase + sizeof(uint64_t) * NG,
               u_pairs = u_wgs + sizeof(uint2) * NW, u_nm = u_pairs + sizeof(uint2) * NP,
               u_state = u_nm + asg_grp_up8(sizeof(int32_t) * NG), v_going = u_state + asg_grp_up8(sizeof(uint32_t) * NG),
               v_rows = v_going + sizeof(ull), v_cnt = v_rows + sizeof(double) * NR * M::SP,
               v_conv = v_cnt + sizeof(ull) * c_words, v_live = v_conv + asg_grp_up8(sizeof(uint32_t) * NG),
               v_lm = v_live + (LM ? sizeof(ull) : 0), pin_bytes = v_lm + (LM ? sizeof(AssignLmOut) * NR : 0);
  MANYCHK(many_grow_pinned(B.h_pin, pin_bytes));  // (every earlier call ended in a synchronisation)
  char *pin = B.h_pin.get();
  double *h_par = (double *)(pin + u_par);
  int32_t *h_nm = (int32_t *)(pin + u_nm);
  uint32_t *h_state = (uint32_t *)(pin + u_state);
  const ull *h_going = (const ull *)(pin + v_going);
  const double *h_rows = (const double *)(pin + v_rows);
  const ull *h_cnt = (const ull *)(pin + v_cnt);
  const uint32_t *h_conv = (const uint32_t *)(pin + v_conv);
  [[maybe_unused]] const AssignLmOut *h_lm = (const AssignLmOut *)(pin + v_lm);
  for (size_t g = 0; g < NG; g++) {
    const size_t nm = J.n_models[g];
    h_nm[g] = (int32_t)nm;
    h_state[g] = (off[g + 1] > off[g] && nm) ? 0u : 1u;
    if (nm) memcpy(h_par + g * MM * M::P, J.params + g * MM * M::P, sizeof(double) * nm * M::P);
  }
  memcpy(pin + u_gbase, gbase.data(), sizeof(uint64_t) * NG);
  if (NW) memcpy(pin + u_wgs, wgs.data(), sizeof(uint2) * NW);
  if (NP) memcpy(pin + u_pairs, pairs.data(), sizeof(uint2) * NP);

  MANYCHK(many_grow(B.d_nm, NG));
  MANYCHK(many_grow(B.d_gbase, NG));
  MANYCHK(many_grow(B.d_state, 2 * NG));  // state, converged
  MANYCHK(many_grow(B.d_cnt, c_words));
  MANYCHK(many_grow(B.d_par, std::max<size_t>(NR * M::P, 1)));
  MANYCHK(many_grow(B.d_rows, std::max<size_t>(NR * M::SP, 1)));
  MANYCHK(many_grow(B.d_wgs, std::max<size_t>(NW, 1)));
  MANYCHK(many_grow(B.d_pairs, std::max<size_t>(NP, 1)));
  MANYCHK(many_grow(B.d_labels[0], std::max<size_t>(NT, 1)));
  if (J.refine) MANYCHK(many_grow(B.d_labels[1], std::max<size_t>(NT, 1)));
  if (J.residuals_out) MANYCHK(many_grow(B.d_res, std::max<size_t>(NT, 1)));
  if (moments) MANYCHK(many_grow(B.d_partials, (size_t)pblocks * M::NMOM));
  if (!J.on_device && J.labels_out) MANYCHK(many_grow(B.d_lab_out, N));
  if (!J.on_device && J.residuals_out) MANYCHK(many_grow(B.d_res_out, N));
  ull *d_changed = B.d_cnt, *d_counts = B.d_cnt + c_counts, *d_used = B.d_cnt + c_used, *d_ok = B.d_cnt + c_ok,
      *d_rounds = B.d_cnt + c_rounds, *d_going = B.d_cnt + c_going;
  uint32_t *d_state = B.d_state, *d_conv = B.d_state + NG;

  MANYCHK(hipMemcpyAsync(B.d_nm, h_nm, sizeof(int32_t) * NG, hipMemcpyHostToDevice, stream));
  MANYCHK(hipMemcpyAsync(B.d_gbase, pin + u_gbase, sizeof(uint64_t) * NG, hipMemcpyHostToDevice, stream));
  MANYCHK(hipMemcpyAsync(d_state, h_state, sizeof(uint32_t) * NG, hipMemcpyHostToDevice, stream));
  MANYCHK(hipMemsetAsync(d_conv, 0, sizeof(uint32_t) * NG, stream));
  MANYCHK(hipMemsetAsync(B.d_cnt, 0, sizeof(ull) * c_words, stream));
  if (NW) {
    MANYCHK(hipMemcpyAsync(B.d_par, h_par, sizeof(double) * NR * M::P, hipMemcpyHostToDevice, stream));
    MANYCHK(hipMemcpyAsync(B.d_wgs, pin + u_wgs, sizeof(uint2) * NW, hipMemcpyHostToDevice, stream));
    MANYCHK(hipMemcpyAsync(B.d_pairs, pin + u_pairs, sizeof(uint2) * NP, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL((k_assign_prepare<M>), dim3(grp_grid(NR)), dim3(kBlock), 0, stream, B.d_par, B.d_nm.get(),
                       (uint64_t)NR, (int)MM, J.mc, B.d_rows);
    MANYCHK(hipGetLastError());
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
  [[maybe_unused]] const AsgGrpLmView V{T,        B.d_wgs, B.d_pairs, NW,       NP,     NG,   MM, pblocks,
                                        P.d_data, W,       B.d_rows,  d_counts, d_used, d_ok, (uint32_t *)(pin + v_live)};
  if constexpr (LM)
    if (moments) {
      const int st = assign_lm_grp_reserve<M>(J, V);
      if (st != LSQR_OK) return st;
    }
  int cur = 0;
  size_t r = 0;
  while (NW) {
    const bool last = r == J.max_rounds;
    int32_t *lab = B.d_labels[cur];
    double *res = J.residuals_out ? B.d_res.get() : nullptr;
    const int32_t *old = r > 0 ? B.d_labels[cur ^ 1].get() : nullptr;
    if (last)
      hipLaunchKernelGGL((k_asg_grp_pass<M, false>), dim3((unsigned)NW), dim3(kBlock), 0, stream, P.d_data, W,
                         B.d_wgs, T, B.d_rows, (int)MM, org_off, J.mc, lab, res, old, d_changed, d_counts, nullptr,
                         nullptr);
    else
      hipLaunchKernelGGL((k_asg_grp_pass<M, true>), dim3((unsigned)NW), dim3(kBlock), 0, stream, P.d_data, W, B.d_wgs,
                         T, B.d_rows, (int)MM, org_off, J.mc, lab, res, old, d_changed, d_counts, B.d_partials,
                         LM ? B.d_presence.get() : nullptr);
    MANYCHK(hipGetLastError());
    if (last) break;  // every group still going stops here: nothing to read
    MANYCHK(hipMemsetAsync(d_going, 0, sizeof(ull), stream));
    hipLaunchKernelGGL(k_asg_grp_decide, dim3(grp_grid(NG)), dim3(kBlock), 0, stream, (uint32_t)NG, (ull)r, 0,
                       d_changed, d_state, d_rounds, d_conv, d_going);
    MANYCHK(hipGetLastError());
    MANYCHK(hipMemcpyAsync(pin + v_going, d_going, sizeof(ull), hipMemcpyDeviceToHost, stream));
    MANYCHK(hipStreamSynchronize(stream));  // the one word of the round
    if (*h_going == 0) break;
    if constexpr (LM) {
      const int st = assign_lm_grp_run<M>(J, V, lab);
      if (st != LSQR_OK) return st;
    } else {
      hipLaunchKernelGGL((k_asg_grp_solve<M>), dim3((unsigned)NP), dim3(64), 0, stream, B.d_pairs, T, B.d_partials,
                         (int)MM, org_off, J.mc, B.d_rows, d_counts, d_used, d_ok, nullptr);
      MANYCHK(hipGetLastError());
    }
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
  if (r > 0) MANYCHK(hipMemcpyAsync(pin + v_rows, B.d_rows, sizeof(double) * NR * M::SP, hipMemcpyDeviceToHost, stream));
  MANYCHK(hipMemcpyAsync(pin + v_cnt, B.d_cnt, sizeof(ull) * c_words, hipMemcpyDeviceToHost, stream));
  MANYCHK(hipMemcpyAsync(pin + v_conv, d_conv, sizeof(uint32_t) * NG, hipMemcpyDeviceToHost, stream));
  if constexpr (LM)
    if (r > 0)
      MANYCHK(hipMemcpyAsync(pin + v_lm, B.d_lm_out, sizeof(AssignLmOut) * NR, hipMemcpyDeviceToHost, stream));
  MANYCHK(hipStreamSynchronize(stream));

  for (size_t g = 0; g < NG; g++) {
    const size_t nm = J.n_models[g];
    const uint64_t ng = off[g + 1] - off[g];
    const size_t rg = (size_t)h_cnt[c_rounds + g];
    if (rg > 0)
      for (size_t m = 0; m < nm; m++)
        for (int j = 0; j < (int)M::P; j++)
          J.params[(g * MM + m) * M::P + j] = h_rows[(g * MM + m) * M::SP + j];
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
        assign_fit_out(rg, h_cnt[c_ok + e], h_cnt[c_used + e], (int32_t)M::P, &J.status_out[e], &J.fits[e]);
        if constexpr (LM)
          if (rg > 0) {
            J.fits[e].lm_info = h_lm[e].lm_info;
            J.fits[e].lm_nfev = h_lm[e].lm_nfev;
            J.fits[e].reserved = h_lm[e].stall;
            J.fits[e].cost = h_lm[e].cost;
          }
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

}  // namespace lsqr
