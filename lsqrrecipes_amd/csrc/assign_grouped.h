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
// All five grouped calls run this file's round loop, assign_grouped_rounds<F> (below, with what a family F supplies), as
// the ungrouped calls run assign_rounds (assign.h).
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
// what every family of the grouped round loop holds: the scan rows, the chunk partials and the presence word of every
// (group, chunk), the packed labels of this round and of the one before, the residuals, the per-group tables, the
// counter words, the outputs in upload order, and the pinned staging (the sort and the packed copy are ManyBufs')
struct AssignGrpCore {
  DevBuf<double> d_rows, d_partials, d_res, d_res_out;
  DevBuf<int32_t> d_labels[2], d_lab_out, d_nm;
  DevBuf<unsigned long long> d_cnt, d_presence;
  DevBuf<uint64_t> d_gbase, d_wbase;
  DevBuf<uint32_t> d_state;  // state, converged
  DevBuf<uint2> d_wgs, d_pairs;
  PinBuf<char> h_pin;  // AssignGrpLayout's u_ and v_ areas
};

struct AssignGrpBufs {  // owned by the context (lsqr_ctx::assign_grp), grown on demand
  AssignGrpCore core;
  DevBuf<double> d_par;
  // the LM stage of lsqr_refine_lm_grouped (assign_lm_grouped.h)
  DevBuf<double> d_start, d_lm_partials;
  DevBuf<unsigned long long> d_lm_mask;  // per group, the models whose LM goes on
  DevBuf<uint32_t> d_lm_live;            // their number over all groups
  DevBuf<LmState> d_lm_state;            // per (group, model)
  DevBuf<AssignLmOut> d_lm_out;
};

// One call's layout: its workgroups and pairs, the blocks of counter words in d_cnt and the areas of h_pin.
// assign_grouped_rounds builds it before the first hook runs; the families read it.
struct AssignGrpLayout {
  typedef unsigned long long ull;
  size_t NG = 0, NE = 0;               // groups, and groups * max_models: the (group, model) entries
  std::vector<uint64_t> off;           // grouped_pack's offsets, NG + 1
  std::vector<uint2> wgs, pairs;       // the (group, chunk) workgroups; the (group, model) pairs whose row is there
  std::vector<uint64_t> gbase, wbase;  // per group: its first (chunk, model) block of the partials, its first workgroup
  size_t NW = 0, NP = 0;               // workgroups, pairs
  uint64_t pblocks = 0;                // (chunk, model) blocks of all groups
  // words of d_cnt: changed[NG], counts / used / ok [NE] each, the family's blocks of NE, rounds[NG], the going words
  size_t c_counts = 0, c_used = 0, c_ok = 0, c_own = 0, c_rounds = 0, c_going = 0, c_words = 0;
  // bytes of h_pin: what goes up, then what comes down, then the family's own
  size_t u_rows = 0, u_gbase = 0, u_wbase = 0, u_wgs = 0, u_pairs = 0, u_nm = 0, u_state = 0, v_going = 0, v_rows = 0,
         v_cnt = 0, v_conv = 0, v_own = 0, bytes = 0;
  AsgGrpTab T{};
  ull *d_cnt = nullptr;  // d(c_counts): the counts on the device, and so on
  char *pin = nullptr;   // h(v_going): the round's going words on the host; h(v_own): the family's own bytes
  ull *d(size_t c) const { return d_cnt + c; }
  char *h(size_t o) const { return pin + o; }

  // up, sp: doubles of an uploaded row and of a scan row; blocks, going, own: the family's counter blocks, going words
  // and pinned bytes
  void place(size_t up, size_t sp, size_t blocks, size_t going, size_t own) {
    const auto up8 = [](size_t b) { return (b + 7) & ~(size_t)7; };
    c_counts = NG, c_used = c_counts + NE, c_ok = c_used + NE, c_own = c_ok + NE, c_rounds = c_own + blocks * NE,
    c_going = c_rounds + NG, c_words = c_going + going;
    u_rows = 0, u_gbase = u_rows + sizeof(double) * NE * up, u_wbase = u_gbase + sizeof(uint64_t) * NG,
    u_wgs = u_wbase + sizeof(uint64_t) * NG, u_pairs = u_wgs + sizeof(uint2) * NW, u_nm = u_pairs + sizeof(uint2) * NP,
    u_state = u_nm + up8(sizeof(int32_t) * NG), v_going = u_state + up8(sizeof(uint32_t) * NG),
    v_rows = v_going + sizeof(ull) * going, v_cnt = v_rows + sizeof(double) * NE * sp,
    v_conv = v_cnt + sizeof(ull) * c_words, v_own = v_conv + up8(sizeof(uint32_t) * NG), bytes = v_own + own;
  }
};

struct AssignGrpJob {
  ManyJob pack;  // grouped_pack's view of the call: stream, W, buf, n = n_groups (lsqr_hip.hip fills it)
  lsqr_model_cfg cfg{};
  ModelConsts mc{};
  const double *data = nullptr;  // the context's records: n of them, `stride` doubles apart
  size_t stride = 0, n = 0;
  AssignGrpLayout L;  // (assign_grouped_rounds fills it)
  // the call
  const int32_t *groups = nullptr;
  size_t n_groups = 0, max_models = 0, max_rounds = 0;
  int on_device = 0;
  bool refine = false;
  double *params = nullptr;  // host, n_groups * max_models rows of parameters: read, and written where a refit ran
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

// THE round loop of the five grouped calls (an assign call: max_rounds == 0).  Round r: the pass of every group still
// going -- labels L_r and, unless it is the last round allowed, whatever the refit needs of L_r --, k_asg_grp_decide,
// the going words to the host, one synchronisation, then the refit under L_r of the groups that go on.  The device
// decides per group; the host only learns whether any group is left.  Returns after the stream has drained; the outputs
// are written only then.  What differs from call to call is the family F (by value: a few references):
//   F::UP, F::SP         the doubles of an uploaded row in h_pin, and of a scan row in d_rows
//   F::BLOCKS, F::GOING  its own blocks of NE counter words after ok (L.c_own), and the words the host reads per round
//   F::WBASE             it wants L.wbase on the device (d_wbase)
//   core()               the AssignGrpCore among its buffers
//   chunks_of(n)         its chunks of a group of n records
//   pin_own(L)           the bytes of h_pin it keeps for itself (L.v_own)
//   reserve(J, moments)  grows its own buffers (and d_partials and d_presence, whose use is its own)
//   rows_up(J, h_rows)   enqueues the caller's parameters' way to the device, staged through h_rows
//   prepare(J)           after the tables are up: enqueues what is left to make d_rows of the upload
//   pass(J, last, lab, res, old)   enqueues the pass of this round
//   before_sync(J)       enqueues what has to be under way before the round's synchronisation
//   refit(J, lab)        after it: enqueues the refit under the packed labels lab; it leaves the new rows in d_rows
//   results(J)           enqueues its own result copies (the rows, the counter words and converged are copied here)
//   n_params(J)          what a fitted model's record reports: the leading doubles of a scan row are the parameters
//   fit_more(J, e, h_cnt, fit)   what it adds to entry e's record after a refit ran
// (rows_up and prepare are two hooks so that the copies of wgs and pairs stay between them, where they have always
// been.)  AssignGrpClosed<M> is lsqr_assign_grouped's and lsqr_refine_grouped's, AssignGrpLm<M> (assign_lm_grouped.h)
// lsqr_refine_lm_grouped's, AssignGrpDense<NR> (assign_dense_grouped.h) the dense pair's.
template <class F>
int assign_grouped_rounds(AssignGrpJob &J, F fam) {
  typedef unsigned long long ull;
  AssignGrpCore &C = fam.core();
  AssignGrpLayout &L = J.L;
  ManyBufs &P = *J.pack.buf;
  hipStream_t stream = J.pack.stream;
  const size_t NG = J.n_groups, MM = J.max_models, N = J.n, NE = NG * MM;

  std::vector<uint64_t> &off = L.off;
  int st = grouped_pack(J.pack, J.data, J.stride, N, J.groups, J.on_device, off);
  if (st != LSQR_OK) {
    memcpy(J.err, J.pack.err, sizeof J.err);
    return st;
  }
  const uint64_t NT = off[NG];
  const uint32_t *perm = P.d_grp_vals[1];

  // the layout: the (group, chunk) workgroups, each group's place in the partials and among the workgroups, the
  // (group, model) pairs
  L.NG = NG, L.NE = NE, L.pblocks = 0;
  L.wgs.clear(), L.pairs.clear();  // (a job used twice starts over)
  L.gbase.assign(NG, 0), L.wbase.assign(NG, 0);
  bool dead_records = false;  // records of a group that runs nothing
  for (size_t g = 0; g < NG; g++) {
    const uint64_t ng = off[g + 1] - off[g];
    const size_t nm = J.n_models[g];
    if (ng && !nm) dead_records = true;
    if (!ng || !nm) continue;
    const uint32_t chunks = fam.chunks_of(ng);
    L.gbase[g] = L.pblocks;
    L.wbase[g] = L.wgs.size();
    L.pblocks += (uint64_t)chunks * nm;
    for (uint32_t q = 0; q < chunks; q++) L.wgs.push_back(make_uint2((uint32_t)g, q));
    for (size_t m = 0; m < nm; m++) L.pairs.push_back(make_uint2((uint32_t)g, (uint32_t)m));
  }
  const size_t NW = L.NW = L.wgs.size(), NP = L.NP = L.pairs.size();
  const bool moments = J.refine && J.max_rounds > 0 && NW > 0;
  L.place(F::UP, F::SP, F::BLOCKS, F::GOING, fam.pin_own(L));

  MANYCHK(many_grow_pinned(C.h_pin, L.bytes));  // (every earlier call ended in a synchronisation)
  char *pin = C.h_pin.get();
  int32_t *h_nm = (int32_t *)(pin + L.u_nm);
  uint32_t *h_state = (uint32_t *)(pin + L.u_state);
  const double *h_rows = (const double *)(pin + L.v_rows);
  const ull *h_cnt = (const ull *)(pin + L.v_cnt);
  const uint32_t *h_conv = (const uint32_t *)(pin + L.v_conv);
  for (size_t g = 0; g < NG; g++) {
    h_nm[g] = (int32_t)J.n_models[g];
    h_state[g] = (off[g + 1] > off[g] && J.n_models[g]) ? 0u : 1u;
  }
  memcpy(pin + L.u_gbase, L.gbase.data(), sizeof(uint64_t) * NG);
  memcpy(pin + L.u_wbase, L.wbase.data(), sizeof(uint64_t) * NG);
  if (NW) memcpy(pin + L.u_wgs, L.wgs.data(), sizeof(uint2) * NW);
  if (NP) memcpy(pin + L.u_pairs, L.pairs.data(), sizeof(uint2) * NP);

  // (many_grow gives an empty buffer its least size even when asked for nothing)
  MANYCHK(many_grow(C.d_nm, NG));
  MANYCHK(many_grow(C.d_gbase, NG));
  if (F::WBASE) MANYCHK(many_grow(C.d_wbase, NG));
  MANYCHK(many_grow(C.d_state, 2 * NG));  // state, converged
  MANYCHK(many_grow(C.d_cnt, L.c_words));
  MANYCHK(many_grow(C.d_rows, NE * F::SP));
  MANYCHK(many_grow(C.d_wgs, NW));
  MANYCHK(many_grow(C.d_pairs, NP));
  MANYCHK(many_grow(C.d_labels[0], (size_t)NT));
  if (J.refine) MANYCHK(many_grow(C.d_labels[1], (size_t)NT));
  if (J.residuals_out) MANYCHK(many_grow(C.d_res, (size_t)NT));
  if (!J.on_device && J.labels_out) MANYCHK(many_grow(C.d_lab_out, N));
  if (!J.on_device && J.residuals_out) MANYCHK(many_grow(C.d_res_out, N));
  if ((st = fam.reserve(J, moments)) != LSQR_OK) return st;
  uint32_t *d_state = C.d_state, *d_conv = C.d_state + NG;
  L.d_cnt = C.d_cnt, L.pin = pin;
  ull *d_changed = L.d(0), *d_rounds = L.d(L.c_rounds), *d_going = L.d(L.c_going);
  L.T = AsgGrpTab{P.d_grp_off, C.d_gbase, C.d_nm, d_state};

  MANYCHK(hipMemcpyAsync(C.d_nm, h_nm, sizeof(int32_t) * NG, hipMemcpyHostToDevice, stream));
  MANYCHK(hipMemcpyAsync(C.d_gbase, pin + L.u_gbase, sizeof(uint64_t) * NG, hipMemcpyHostToDevice, stream));
  if (F::WBASE)
    MANYCHK(hipMemcpyAsync(C.d_wbase, pin + L.u_wbase, sizeof(uint64_t) * NG, hipMemcpyHostToDevice, stream));
  MANYCHK(hipMemcpyAsync(d_state, h_state, sizeof(uint32_t) * NG, hipMemcpyHostToDevice, stream));
  MANYCHK(hipMemsetAsync(d_conv, 0, sizeof(uint32_t) * NG, stream));
  MANYCHK(hipMemsetAsync(C.d_cnt, 0, sizeof(ull) * L.c_words, stream));
  if (NW) {
    if ((st = fam.rows_up(J, (double *)(pin + L.u_rows))) != LSQR_OK) return st;
    MANYCHK(hipMemcpyAsync(C.d_wgs, pin + L.u_wgs, sizeof(uint2) * NW, hipMemcpyHostToDevice, stream));
    MANYCHK(hipMemcpyAsync(C.d_pairs, pin + L.u_pairs, sizeof(uint2) * NP, hipMemcpyHostToDevice, stream));
    if ((st = fam.prepare(J)) != LSQR_OK) return st;
  }
  if (dead_records && NT) {  // no pass writes them
    MANYCHK(hipMemsetAsync(C.d_labels[0], 0xFF, sizeof(int32_t) * NT, stream));
    if (J.refine) MANYCHK(hipMemsetAsync(C.d_labels[1], 0xFF, sizeof(int32_t) * NT, stream));
    if (J.residuals_out) {
      hipLaunchKernelGGL(k_asg_grp_fill, dim3(grp_grid(NT)), dim3(kBlock), 0, stream, C.d_res, (uint64_t)NT,
                         __builtin_inf());
      MANYCHK(hipGetLastError());
    }
  }

  int cur = 0;
  size_t r = 0;
  while (NW) {
    const bool last = r == J.max_rounds;
    int32_t *lab = C.d_labels[cur];
    double *res = J.residuals_out ? C.d_res.get() : nullptr;
    const int32_t *old = r > 0 ? C.d_labels[cur ^ 1].get() : nullptr;
    if ((st = fam.pass(J, last, lab, res, old)) != LSQR_OK) return st;
    if (last) break;  // every group still going stops here: nothing to read
    MANYCHK(hipMemsetAsync(d_going, 0, sizeof(ull) * F::GOING, stream));
    hipLaunchKernelGGL(k_asg_grp_decide, dim3(grp_grid(NG)), dim3(kBlock), 0, stream, (uint32_t)NG, (ull)r, 0,
                       d_changed, d_state, d_rounds, d_conv, d_going);
    MANYCHK(hipGetLastError());
    if ((st = fam.before_sync(J)) != LSQR_OK) return st;
    MANYCHK(hipMemcpyAsync(pin + L.v_going, d_going, sizeof(ull) * F::GOING, hipMemcpyDeviceToHost, stream));
    MANYCHK(hipStreamSynchronize(stream));  // the going words of the round
    if (*(const ull *)(pin + L.v_going) == 0) break;
    if ((st = fam.refit(J, lab)) != LSQR_OK) return st;
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
    int32_t *d_lab = J.on_device ? J.labels_out : C.d_lab_out.get();
    hipLaunchKernelGGL(k_grp_scatter_labels, dim3(grp_grid(N)), dim3(kBlock), 0, stream, perm, (uint32_t)N,
                       (uint32_t)NT, C.d_labels[cur].get(), d_lab);
    MANYCHK(hipGetLastError());
    if (!J.on_device)
      MANYCHK(hipMemcpyAsync(J.labels_out, d_lab, sizeof(int32_t) * N, hipMemcpyDeviceToHost, stream));
  }
  if (J.residuals_out) {
    double *d_r = J.on_device ? J.residuals_out : C.d_res_out.get();
    hipLaunchKernelGGL(k_grp_scatter_f64, dim3(grp_grid(N)), dim3(kBlock), 0, stream, perm, (uint32_t)N, (uint32_t)NT,
                       C.d_res.get(), __builtin_inf(), d_r);
    MANYCHK(hipGetLastError());
    if (!J.on_device)
      MANYCHK(hipMemcpyAsync(J.residuals_out, d_r, sizeof(double) * N, hipMemcpyDeviceToHost, stream));
  }
  if (r > 0)
    MANYCHK(hipMemcpyAsync(pin + L.v_rows, C.d_rows, sizeof(double) * NE * F::SP, hipMemcpyDeviceToHost, stream));
  MANYCHK(hipMemcpyAsync(pin + L.v_cnt, C.d_cnt, sizeof(ull) * L.c_words, hipMemcpyDeviceToHost, stream));
  MANYCHK(hipMemcpyAsync(pin + L.v_conv, d_conv, sizeof(uint32_t) * NG, hipMemcpyDeviceToHost, stream));
  if (r > 0 && (st = fam.results(J)) != LSQR_OK) return st;
  MANYCHK(hipStreamSynchronize(stream));

  const size_t np = (size_t)fam.n_params(J);
  for (size_t g = 0; g < NG; g++) {
    const size_t nm = J.n_models[g];
    const uint64_t ng = off[g + 1] - off[g];
    const size_t rg = (size_t)h_cnt[L.c_rounds + g];
    if (rg > 0)
      for (size_t m = 0; m < nm; m++)
        for (size_t j = 0; j < np; j++) J.params[(g * MM + m) * np + j] = h_rows[(g * MM + m) * F::SP + j];
    if (J.counts_out) {
      uint64_t sum = 0, *c = J.counts_out + g * (MM + 1);
      for (size_t m = 0; m < MM; m++) sum += (c[m] = m < nm ? h_cnt[L.c_counts + g * MM + m] : 0);
      c[MM] = ng - sum;
    }
    if (!J.refine) continue;
    J.rounds_out[g] = rg;
    J.converged_out[g] = (int32_t)h_conv[g];
    for (size_t m = 0; m < MM; m++) {
      const size_t e = g * MM + m;
      if (m < nm) {
        assign_fit_out(rg, h_cnt[L.c_ok + e], h_cnt[L.c_used + e], (int32_t)np, &J.status_out[e], &J.fits[e]);
        if (rg > 0) fam.fit_more(J, e, h_cnt, J.fits[e]);
      } else {
        J.status_out[e] = LSQR_ERR_STATE;  // model not there
        memset(&J.fits[e], 0, sizeof(lsqr_fit_info));
      }
    }
  }
  if (J.offsets_out) memcpy(J.offsets_out, off.data(), sizeof(uint64_t) * (NG + 1));
  return LSQR_OK;
}

// The closed form: lsqr_assign_grouped, and lsqr_refine_grouped, whose refit is one k_asg_grp_solve launch.
template <class M>
struct AssignGrpClosed {
  static constexpr int UP = M::P, SP = M::SP, BLOCKS = 0, GOING = 1;
  static constexpr bool WBASE = false;
  AssignGrpBufs &B;

  AssignGrpCore &core() { return B.core; }
  static uint32_t chunks_of(uint64_t n) { return assign_chunks(n); }
  static size_t pin_own(const AssignGrpLayout &) { return 0; }
  int reserve(AssignGrpJob &J, bool moments) {
    MANYCHK(many_grow(B.d_par, J.L.NE * M::P));
    if (moments) MANYCHK(many_grow(B.core.d_partials, (size_t)J.L.pblocks * M::NMOM));
    return LSQR_OK;
  }
  int rows_up(AssignGrpJob &J, double *h_rows) {  // the rows that are there, as they are
    const size_t MM = J.max_models;
    for (size_t g = 0; g < J.n_groups; g++)
      if (J.n_models[g])
        memcpy(h_rows + g * MM * M::P, J.params + g * MM * M::P, sizeof(double) * J.n_models[g] * M::P);
    MANYCHK(hipMemcpyAsync(B.d_par, h_rows, sizeof(double) * J.L.NE * M::P, hipMemcpyHostToDevice, J.pack.stream));
    return LSQR_OK;
  }
  int prepare(AssignGrpJob &J) {  // k_assign_prepare with the groups' model counts
    hipLaunchKernelGGL((k_assign_prepare<M>), dim3(grp_grid(J.L.NE)), dim3(kBlock), 0, J.pack.stream, B.d_par,
                       B.core.d_nm.get(), (uint64_t)J.L.NE, (int)J.max_models, J.mc, B.core.d_rows);
    MANYCHK(hipGetLastError());
    return LSQR_OK;
  }
  // presence: where a pass with moments leaves every workgroup's word (nullable)
  int pass_to(AssignGrpJob &J, bool last, int32_t *lab, double *res, const int32_t *old,
              unsigned long long *presence) {
    const AssignGrpLayout &L = J.L;
    AssignGrpCore &C = B.core;
    const size_t W = (size_t)J.pack.W;
    const int MM = (int)J.max_models, org_off = fit_origin_offset<M>(J.cfg);
    if (last)
      hipLaunchKernelGGL((k_asg_grp_pass<M, false>), dim3((unsigned)L.NW), dim3(kBlock), 0, J.pack.stream,
                         J.pack.buf->d_data, W, C.d_wgs, L.T, C.d_rows, MM, org_off, J.mc, lab, res, old, L.d(0),
                         L.d(L.c_counts), nullptr, nullptr);
    else
      hipLaunchKernelGGL((k_asg_grp_pass<M, true>), dim3((unsigned)L.NW), dim3(kBlock), 0, J.pack.stream,
                         J.pack.buf->d_data, W, C.d_wgs, L.T, C.d_rows, MM, org_off, J.mc, lab, res, old, L.d(0),
                         L.d(L.c_counts), C.d_partials, presence);
    MANYCHK(hipGetLastError());
    return LSQR_OK;
  }
  int pass(AssignGrpJob &J, bool last, int32_t *lab, double *res, const int32_t *old) {
    return pass_to(J, last, lab, res, old, nullptr);
  }
  int before_sync(AssignGrpJob &) { return LSQR_OK; }
  // START, start: see k_asg_grp_solve
  template <bool START>
  int solve_to(AssignGrpJob &J, double *start) {
    const AssignGrpLayout &L = J.L;
    hipLaunchKernelGGL((k_asg_grp_solve<M, START>), dim3((unsigned)L.NP), dim3(64), 0, J.pack.stream, B.core.d_pairs,
                       L.T, B.core.d_partials, (int)J.max_models, fit_origin_offset<M>(J.cfg), J.mc, B.core.d_rows,
                       L.d(L.c_counts), L.d(L.c_used), L.d(L.c_ok), start);
    MANYCHK(hipGetLastError());
    return LSQR_OK;
  }
  int refit(AssignGrpJob &J, const int32_t *) { return solve_to<false>(J, nullptr); }
  int results(AssignGrpJob &) { return LSQR_OK; }
  static int32_t n_params(const AssignGrpJob &) { return (int32_t)M::P; }
  void fit_more(AssignGrpJob &, size_t, const unsigned long long *, lsqr_fit_info &) {}
};
#endif  // __HIPCC__

}  // namespace lsqr
