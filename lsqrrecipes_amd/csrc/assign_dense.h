// assign_dense.h -- lsqr_assign_dense / lsqr_refine_dense: lsqr_assign / lsqr_refine (assign.h) for the dense linear
// system, DenseLinearEquationSystemParametersEstimator<double,n>, n = 1..64: every row (a | b) of the context's upload
// goes to the NEAREST of up to 64 regressions it agrees with, and (refine) every regression is fitted again on its own
// rows, round after round, on the device.  The rounds are assign.h's loop, assign_rounds, with the family
// AssignDense<NR> of this file.
//
// The decision for one row is assign_one<DenseModel<NR>> (assign.h): the kernel and lsqr_assign_dense_host run that
// code, so the residual is the reference's running sum in slot order, sum += x[i] * sp[i], then - b, and the label
// the smallest m that minimises it among the m that agree.  The padding slots n .. NR - 1 of a row and of a regression
// are zero: their 0.0 * 0.0 terms leave the running sum bit-identical (dense.h).
//
// assign_pass_chunk (assign.h) cannot take this model: it keeps eight records and one model's moment block in a
// lane's registers, and a dense row is up to 65 doubles, its block up to 2145.  Here the chunk lives in LDS:
//
//   k_asd_pass<NR>      one workgroup of 256 lanes per chunk of kAssignDenseChunk<NR> consecutive rows.  The chunk's
//                       rows are staged ONCE into LDS (NR coefficient slots, zero beyond n, then b: pitch NR + 1
//                       doubles, odd, so the lanes' row reads fall on distinct banks), and both steps read that image:
//                       label step   lane r < rows takes row r into registers and walks the M scan rows, which are
//                                    read at wave-uniform addresses (scalar loads); it writes labels[i] (and
//                                    residuals[i]), the workgroup counts labels[i] != old[i] and the rows per model
//                                    (ballots, then one 64-bit integer atomic per counter and workgroup)
//                       order        a stable counting sort of the chunk's row numbers by label (ballot ranks, the
//                                    waves in order), so that the rows of model m are a run of s_order in row order
//                       moment step  WITH_MOMENTS: for every model present in the chunk (one 64-bit presence word),
//                                    in ascending m, the packed upper triangle of sum z z^T, z = (a | b), over the
//                                    model's run; entry e = tid + 256 u is summed by one thread in row order (the
//                                    thread-per-entry form of k_many_dense_mask_moments) -> partials[chunk][m][ps].
//                                    A model absent from the chunk costs nothing: its slot is not written and the
//                                    chunk's presence word tells k_asd_sum to take 0.0 for it.
//                       Its body is asd_pass_chunk, which k_asd_grp_pass (assign_dense_grouped.h: one regression set
//                       per label) runs too; the kernels only locate their chunk.
//   k_asd_sum           model m's blocks added in chunk order, one thread per entry; the count comes from the
//                       integer counter -> mom[m][ps] (the block, then the count: solve_dense_wg's layout)
//   k_asd_solve         one workgroup per model: solve_dense_wg (dense.h) where the model has at least n rows, with
//                       the options dense_fast_solve and dense_dd as lsqr_ls_fit takes them; with dense_dd a pivot
//                       below 1e-6 max|G| raises the model's flag instead
//   k_asd_label_mask    a flagged model's byte mask label == m, for k_gram_dd_dense + k_dense_dd_solve (dense.h),
//                       launched per flagged model as many_dense_finish launches them, over the whole upload with
//                       launch_solve_dense's grid (what lsqr_set_mask + lsqr_ls_fit run on that mask)
//   k_asd_apply         the refit decision: a model with at least n rows and a solve that gave a result gets the new
//                       row, any other keeps its row; the ASG_USED / ASG_OK / ASD_ROUTE words say what happened
//
// Order of the sums: kAssignDenseChunk<NR> fixes it, as kAssignChunk does for assign.h.  A model's block is the sum,
// in chunk order, of its chunk blocks, each the sum in row order of its own rows; 0.0 stands for a chunk without the
// model, and t + 0.0 == t bit for bit for every t such a sum can hold (it starts at +0.0 and so never is -0.0).  So
// the block depends on the model's own rows, their positions in the upload and the chunking alone -- not on the grid,
// on the other models of the call or on where m sits among them.  Nothing is summed with a floating-point atomic.
//
// Device scratch of a refine call: partials = chunks x n_models x ps doubles, chunks = ceil(N / kAssignDenseChunk<NR>),
// ps = many_dense_ps(n) = (n+1)(n+2)/2 + 1 rounded up to 8 (n = 64, 16 models: 2152 x 16 x 8 B = 269 KiB per 128
// rows); two label arrays of N int32; one presence word per chunk; with dense_dd and a flagged model N mask bytes and
// the 9 MiB of k_gram_dd_dense's partials.  A buffer that cannot be had ends the call with LSQR_ERR_HIP.
//
// Budget (DESIGN.md section 14.4 has the table): the pass keeps one row (NR + 1 doubles) per lane in the label step
// and U = ceil((NR+1)(NR+2)/2 / 256) accumulators with their slot pairs in the moment step; no instantiation spills.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "assign.h"
#include "dense.h"
#include "many_dense.h"

namespace lsqr {

// rows per workgroup of k_asd_pass (fixes the order of the moment sums): the LDS image is chunk x (NR + 1) doubles --
// 18, 34, 66 and 65 KiB -- so the wide classes still run two workgroups per CU beside it
template <int NR> constexpr uint32_t kAssignDenseChunk = NR <= 32 ? 256u : 128u;
constexpr int kAsdBlock = 256;

enum { ASD_ROUTE = ASG_WORDS, ASD_WORDS = ASD_ROUTE + kAssignMaxModels };  // SolveOut::pad of the last refit

#if defined(__HIPCC__)
// The pass over ONE chunk, by one workgroup of kAsdBlock lanes: the body of k_asd_pass and of k_asd_grp_pass
// (assign_dense_grouped.h), which only locate their chunk.  The chunk's base is in the pointers, so its rows are
// [0, cnt), cnt <= kAssignDenseChunk<NR>.  src: the chunk's rows, `stride` doubles apart, dim + 1 doubles each; rows:
// the n_models scan rows of NR doubles of the chunk's model set; labels / residuals (nullable) / old (nullable): the
// chunk's cnt entries; changed: the word that counts labels[i] != old[i]; counts: one word per model; partials
// (WITH_MOMENTS): the chunk's [model][ps]; presence (WITH_MOMENTS): the chunk's word.
// Dynamic LDS: kAssignDenseChunk<NR> * (NR + 1) doubles.  It must be inlined, as assign_pass_chunk (assign.h).
template <int NR, bool WITH_MOMENTS>
__device__ __forceinline__ void asd_pass_chunk(const double *__restrict__ src, size_t stride, uint32_t cnt, int dim,
                                               const double *__restrict__ rows, int n_models, const ModelConsts &mc,
                                               int32_t *__restrict__ labels, double *__restrict__ residuals,
                                               const int32_t *__restrict__ old,
                                               unsigned long long *__restrict__ changed,
                                               unsigned long long *__restrict__ counts,
                                               double *__restrict__ partials, int ps,
                                               unsigned long long *__restrict__ presence) {
  typedef DenseModel<NR> M;
  constexpr uint32_t CH = kAssignDenseChunk<NR>;
  constexpr int PITCH = NR + 1, W = kAsdBlock / 64, U = ((NR + 1) * (NR + 2) / 2 + kAsdBlock - 1) / kAsdBlock;
  static_assert(CH <= (uint32_t)kAsdBlock, "one row per lane");
  extern __shared__ double s_rec[];  // CH x PITCH
  __shared__ uint32_t s_wc[W][kAssignMaxModels];  // rows of model m in wave w
  __shared__ uint32_t s_base[kAssignMaxModels], s_tot[kAssignMaxModels];
  __shared__ uint16_t s_order[CH];
  __shared__ unsigned long long s_p[W];
  __shared__ uint32_t s_chg[W];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;

  for (uint32_t q = tid; q < cnt * PITCH; q += kAsdBlock) {  // the chunk's rows -> LDS, zero-padded
    const uint32_t r = q / PITCH, k = q - r * PITCH;
    s_rec[q] = (int)k < dim ? src[(size_t)r * stride + k] : (k == NR ? src[(size_t)r * stride + dim] : 0.0);
  }
  s_wc[wave][lane] = 0;
  __syncthreads();

  // ---- label step: one row per lane
  const bool in = (uint32_t)tid < cnt;
  int32_t lab = -1;
  if (in) {
    double x[M::REC], res;
#pragma unroll
    for (int k = 0; k < (int)M::REC; k++) x[k] = s_rec[tid * PITCH + k];
    lab = assign_one<M>(rows, n_models, x, mc, &res);
    labels[tid] = lab;
    if (residuals) residuals[tid] = res;
  }
  uint32_t chg = in && old && old[tid] != lab ? 1u : 0u;
  unsigned long long pres = lab >= 0 ? 1ull << lab : 0ull;
  for (int o = 32; o > 0; o >>= 1) {
    chg += __shfl_xor(chg, o);
    pres |= __shfl_xor(pres, o);
  }
  // (uniform by construction; the scalar copies keep the model loops' control flow on the scalar unit)
  const unsigned long long mine = wave_uniform64(pres);
  uint32_t rank = 0;  // rows of the lane's model before it in its wave
  for (unsigned long long rest = mine; rest; rest &= rest - 1) {
    const int m = __builtin_ctzll(rest);
    const unsigned long long b = __ballot(lab == m);
    if (lab == m) rank = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) s_wc[wave][m] = (uint32_t)__popcll(b);
  }
  if (lane == 0) {
    s_p[wave] = mine;
    s_chg[wave] = chg;
  }
  __syncthreads();
  if (tid < 64) {  // rows per model, and where each model's run begins in s_order
    uint32_t t = 0;
    for (int w = 0; w < W; w++) t += s_wc[w][tid];
    uint32_t incl = t;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    s_tot[tid] = t;
    s_base[tid] = incl - t;
    if (tid < n_models && t) atomicAdd(&counts[tid], (unsigned long long)t);
  }
  if (tid == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < W; w++) t += s_chg[w];
    if (t) atomicAdd(changed, t);
  }
  if constexpr (WITH_MOMENTS) {
    unsigned long long all = 0;
    for (int w = 0; w < W; w++) all |= s_p[w];
    const unsigned long long present = wave_uniform64(all);
    __syncthreads();
    if (lab >= 0) {
      uint32_t pos = s_base[lab] + rank;
      for (int w = 0; w < wave; w++) pos += s_wc[w][lab];
      s_order[pos] = (uint16_t)tid;
    }
    // ---- moment step: this thread's entries e = tid + 256 u of the packed upper triangle -> the LDS slots of (a, b)
    const int nz = dim + 1, ne = nz * (nz + 1) / 2;
    int ea[U], eb[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int e = tid + kAsdBlock * u;
      ea[u] = eb[u] = 0;
      if (e < ne) {
        int a = 0, rem = e;
        while (rem >= nz - a) rem -= nz - a++;
        const int b = a + rem;
        ea[u] = a < dim ? a : NR;
        eb[u] = b < dim ? b : NR;
      }
    }
    __syncthreads();
    for (unsigned long long rest = present; rest; rest &= rest - 1) {
      const int m = __builtin_ctzll(rest);
      const uint32_t q0 = s_base[m], q1 = q0 + s_tot[m];
      double acc[U];
#pragma unroll
      for (int u = 0; u < U; u++) acc[u] = 0.0;
      for (uint32_t q = q0; q < q1; q++) {
        const double *z = s_rec + (uint32_t)s_order[q] * PITCH;
#pragma unroll
        for (int u = 0; u < U; u++) acc[u] += z[ea[u]] * z[eb[u]];
      }
      double *out = partials + (size_t)m * ps;
#pragma unroll
      for (int u = 0; u < U; u++)
        if (tid + kAsdBlock * u < ne) out[tid + kAsdBlock * u] = acc[u];
    }
    if (tid == 0) *presence = present;
  }
}

// chunk blockIdx.x of the context's n rows.  data: `stride` doubles apart, dim + 1 doubles each; rows: n_models scan
// rows of NR doubles; labels: n entries; residuals, old: nullable; counters: the ASG_ words, zeroed by the caller;
// partials (WITH_MOMENTS): [chunk][model][ps]; presence (WITH_MOMENTS): one word per chunk.
// Dynamic LDS: kAssignDenseChunk<NR> * (NR + 1) doubles.
template <int NR, bool WITH_MOMENTS>
__global__ __launch_bounds__(kAsdBlock) void k_asd_pass(const double *__restrict__ data, size_t stride, uint32_t n,
                                                        int dim, const double *__restrict__ rows, int n_models,
                                                        ModelConsts mc, int32_t *__restrict__ labels,
                                                        double *__restrict__ residuals,
                                                        const int32_t *__restrict__ old,
                                                        unsigned long long *__restrict__ counters,
                                                        double *__restrict__ partials, int ps,
                                                        unsigned long long *__restrict__ presence) {
  constexpr uint32_t CH = kAssignDenseChunk<NR>;
  const uint32_t c0 = blockIdx.x * CH, left = n - c0;  // (c0 < n: no wrap)
  if constexpr (WITH_MOMENTS) {
    partials += (size_t)blockIdx.x * n_models * ps;
    presence += blockIdx.x;
  }
  asd_pass_chunk<NR, WITH_MOMENTS>(data + (size_t)c0 * stride, stride, left < CH ? left : CH, dim, rows, n_models, mc,
                                   labels + c0, residuals ? residuals + c0 : nullptr, old ? old + c0 : nullptr,
                                   counters + ASG_CHANGED, counters + ASG_COUNT, partials, ps, presence);
}

// One entry of one model's block: the chunk blocks added in chunk order, 32 loads in flight, 0.0 where the chunk's
// presence word says the model is not there.  src: the entry in the model's block of chunk 0, `qs` doubles from chunk
// to chunk; pw: the presence words of the `chunks` chunks.  The sum of k_asd_sum and of k_asd_grp_sum
// (assign_dense_grouped.h): the bit-identity of the grouped calls rests on both running THIS loop.
__device__ __forceinline__ double asd_sum_entry(const double *__restrict__ src, size_t qs,
                                                const unsigned long long *__restrict__ pw, int m, uint32_t chunks) {
  constexpr int PF = 32;
  double t = 0.0;
  for (uint32_t q0 = 0; q0 < chunks; q0 += PF) {
    double v[PF];
#pragma unroll
    for (int u = 0; u < PF; u++) {
      const uint32_t q = q0 + u;
      v[u] = q < chunks && ((pw[q] >> m) & 1ull) ? src[(size_t)q * qs] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < PF; u++) t += v[u];
  }
  return t;
}

// model blockIdx.x, entries blockIdx.y * 256 + tid: its chunk blocks added in chunk order (asd_sum_entry); entry ne is
// the count
__global__ __launch_bounds__(kAsdBlock) void k_asd_sum(const double *__restrict__ partials,
                                                       const unsigned long long *__restrict__ presence,
                                                       uint32_t chunks, int n_models, int n, int ps,
                                                       const unsigned long long *__restrict__ counters,
                                                       double *__restrict__ mom) {
  const int m = blockIdx.x, e = blockIdx.y * kAsdBlock + threadIdx.x, ne = (n + 1) * (n + 2) / 2;
  if (e > ne) return;
  if (e == ne) {
    mom[(size_t)m * ps + ne] = (double)counters[ASG_COUNT + m];
    return;
  }
  mom[(size_t)m * ps + e] = asd_sum_entry(partials + (size_t)m * ps + e, (size_t)n_models * ps, presence, m, chunks);
}

// One model's solve, by one workgroup of 256 lanes: solve_dense_wg on its block mm where it has at least n rows.  flag
// (nullable: dense_dd 0, the block alone decides): the model's, zeroed by the caller.  The body of k_asd_solve and of
// k_asd_grp_solve (assign_dense_grouped.h).  Dynamic LDS: many_dense_lds(n).
__device__ __forceinline__ void asd_solve_one(const double *__restrict__ mm, int n, int fast,
                                              SolveOut *__restrict__ out, int *__restrict__ flag) {
  if (mm[(n + 1) * (n + 2) / 2] < (double)n) {  // fewer than lsqr_min_subset rows: no refit (workgroup-uniform)
    if (threadIdx.x == 0) {
      out->ok = 0;
      out->n_params = 0;
      out->pad = 0;
    }
    return;
  }
  solve_dense_wg(mm, n, fast, out, flag);
}

// flags (nullable): one per model.  Dynamic LDS: many_dense_lds(n).
__global__ __launch_bounds__(256) void k_asd_solve(const double *__restrict__ mom, int ps, int n, int fast,
                                                   SolveOut *__restrict__ out, int *__restrict__ flags) {
  const uint32_t m = blockIdx.x;
  asd_solve_one(mom + (size_t)m * ps, n, fast, out + m, flags ? flags + m : nullptr);
}

__global__ __launch_bounds__(256) void k_asd_label_mask(const int32_t *__restrict__ labels, uint32_t n, int32_t m,
                                                        uint8_t *__restrict__ mask) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) mask[i] = labels[i] == m ? 1 : 0;
}

// The refit decision for one model, by one wave (lane t): cnt rows were behind the attempt `out`; a model with at
// least n rows and a solve that gave a result gets the new scan row (nr doubles, zero beyond n), any other keeps its
// row; *used / *okf / *route say what happened.  The body of k_asd_apply and of k_asd_grp_apply
// (assign_dense_grouped.h).
__device__ __forceinline__ void asd_apply_one(const SolveOut *__restrict__ out, unsigned long long cnt, int n, int nr,
                                              double *__restrict__ row, unsigned long long *used,
                                              unsigned long long *okf, unsigned long long *route) {
  const int t = threadIdx.x;
  const bool ran = cnt >= (unsigned long long)n, ok = ran && out->ok != 0;
  if (ok && t < nr) row[t] = t < n ? out->params[t] : 0.0;
  if (t == 0) {
    *used = cnt;
    *okf = ok ? 1 : 0;
    *route = ran ? (unsigned long long)out->pad : 0;
  }
}

// model blockIdx.x: what its refit gave -> its scan row and the ASG_ / ASD_ words
__global__ __launch_bounds__(64) void k_asd_apply(const SolveOut *__restrict__ out, int n, int nr,
                                                  double *__restrict__ rows,
                                                  unsigned long long *__restrict__ counters) {
  const int m = blockIdx.x;
  asd_apply_one(out + m, counters[ASG_COUNT + m], n, nr, rows + (size_t)m * nr, counters + ASG_USED + m,
                counters + ASG_OK + m, counters + ASD_ROUTE + m);
}

// ---- host side -----------------------------------------------------------------------------------------------------
struct AssignDenseBufs {  // owned by the context (lsqr_ctx::assign_dense), grown on demand
  AssignCore core;
  DevBuf<double> d_mom, d_ddpart;
  DevBuf<unsigned long long> d_presence;
  DevBuf<SolveOut> d_out;
  DevBuf<int> d_flags;
  DevBuf<uint8_t> d_mask;
};

// The dense system's family of the round loop (assign.h: assign_rounds).  Before the round's synchronisation its pass
// enqueues, unless the round is the last one allowed, the sum and the solve of every model as well, and with dense_dd
// the copy of the flags: ONE wait brings the changed-counter, the counts and the flags.  (So the solve is enqueued
// before the host knows whether L_r == L_{r-1}; on convergence its result is not applied.)  The refit solves the
// flagged models again from their rows in double-double; k_asd_apply makes the refit decision.
template <int NR>
struct AssignDense {
  typedef AssignPin<64, 3, sizeof(int) * kAssignMaxModels> Pin;  // the ASD_ROUTE block; its own: the flags
  static_assert(Pin::words == ASD_WORDS, "the counter words");
  static constexpr int SP = NR;
  static constexpr uint32_t CH = kAssignDenseChunk<NR>;
  static constexpr size_t lds_pass = sizeof(double) * CH * (NR + 1);
  AssignDenseBufs &B;
  int dense_fast, dense_dd;  // the context's options

  AssignCore &core() { return B.core; }
  static uint32_t chunks_of(uint32_t n) { return (uint32_t)(((uint64_t)n + CH - 1) / CH); }
  int reserve(AssignJob &J, bool refine) {
    if (refine) {
      const size_t nm = J.n_models, ps = (size_t)many_dense_ps((int)J.cfg.dim), chunks = chunks_of(J.n);
      MANYCHK(many_grow(B.core.d_partials, chunks * nm * ps));
      MANYCHK(many_grow(B.d_presence, chunks));
      MANYCHK(many_grow(B.d_mom, nm * ps));
      MANYCHK(many_grow(B.d_out, (size_t)kAssignMaxModels));
      MANYCHK(many_grow(B.d_flags, (size_t)kAssignMaxModels));
      (void)hipFuncSetAttribute((const void *)k_asd_solve, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)many_dense_lds(64));
      (void)hipFuncSetAttribute((const void *)(k_asd_pass<NR, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds_pass);
    }
    (void)hipFuncSetAttribute((const void *)(k_asd_pass<NR, false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds_pass);
    return LSQR_OK;
  }
  int rows_up(AssignJob &J, double *h_rows) {  // the zero-padded copy
    const size_t nm = J.n_models, dim = J.cfg.dim;
    for (size_t m = 0; m < nm; m++)
      for (size_t j = 0; j < (size_t)NR; j++) h_rows[m * NR + j] = j < dim ? J.params[m * dim + j] : 0.0;
    MANYCHK(hipMemcpyAsync(B.core.d_rows, h_rows, sizeof(double) * nm * NR, hipMemcpyHostToDevice, J.stream));
    return LSQR_OK;
  }
  int pass(AssignJob &J, bool last, int32_t *lab, double *res, const int32_t *old) {
    const int nm = (int)J.n_models, dim = (int)J.cfg.dim, ps = many_dense_ps(dim), ne = (dim + 1) * (dim + 2) / 2;
    const uint32_t chunks = chunks_of(J.n);
    AssignCore &C = B.core;
    if (last) {
      hipLaunchKernelGGL((k_asd_pass<NR, false>), dim3(chunks), dim3(kAsdBlock), lds_pass, J.stream, J.data, J.stride,
                         J.n, dim, C.d_rows, nm, J.mc, lab, res, old, C.d_cnt, nullptr, ps, nullptr);
      MANYCHK(hipGetLastError());
      return LSQR_OK;
    }
    hipLaunchKernelGGL((k_asd_pass<NR, true>), dim3(chunks), dim3(kAsdBlock), lds_pass, J.stream, J.data, J.stride, J.n,
                       dim, C.d_rows, nm, J.mc, lab, res, old, C.d_cnt, C.d_partials, ps, B.d_presence);
    MANYCHK(hipGetLastError());
    hipLaunchKernelGGL(k_asd_sum, dim3(nm, (ne + 1 + kAsdBlock - 1) / kAsdBlock), dim3(kAsdBlock), 0, J.stream,
                       C.d_partials, B.d_presence, chunks, nm, dim, ps, C.d_cnt, B.d_mom);
    MANYCHK(hipGetLastError());
    if (dense_dd) MANYCHK(hipMemsetAsync(B.d_flags, 0, sizeof(int) * kAssignMaxModels, J.stream));
    hipLaunchKernelGGL(k_asd_solve, dim3(nm), dim3(256), many_dense_lds(dim), J.stream, B.d_mom, ps, dim, dense_fast,
                       B.d_out, dense_dd ? B.d_flags.get() : (int *)nullptr);
    MANYCHK(hipGetLastError());
    if (dense_dd)
      MANYCHK(hipMemcpyAsync(h_flags(), B.d_flags, sizeof(int) * (size_t)nm, hipMemcpyDeviceToHost, J.stream));
    return LSQR_OK;
  }
  int refit(AssignJob &J, const int32_t *lab) {
    const int nm = (int)J.n_models, dim = (int)J.cfg.dim, ps = many_dense_ps(dim);
    const uint32_t n = J.n;
    if (dense_dd) {  // the ill-conditioned ones again from their rows, in double-double (launch_solve_dense's route)
      bool any = false;
      for (int m = 0; m < nm; m++) {
        if (!h_flags()[m]) continue;
        if (!any) {
          MANYCHK(many_grow(B.d_ddpart, (size_t)2 * kDdNe * kDdBlocks));
          MANYCHK(many_grow(B.d_mask, (size_t)n));
          (void)hipFuncSetAttribute((const void *)k_dense_dd_solve, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)dense_dd_lds(64));
          any = true;
        }
        const int nb = (int)std::min<size_t>(kDdBlocks, ((size_t)n + 31) / 32);
        hipLaunchKernelGGL(k_asd_label_mask, dim3(std::min<uint32_t>((n + 255) / 256, 4096u)), dim3(256), 0, J.stream,
                           lab, n, (int32_t)m, B.d_mask);
        MANYCHK(hipGetLastError());
        hipLaunchKernelGGL((k_gram_dd_dense<32>), dim3(nb), dim3(256), 0, J.stream, J.data, J.stride, (size_t)0,
                           (size_t)n, dim, B.d_mask, B.d_flags + m, B.d_ddpart);
        MANYCHK(hipGetLastError());
        hipLaunchKernelGGL(k_dense_dd_solve, dim3(1), dim3(256), dense_dd_lds(dim), J.stream, B.d_ddpart, nb, dim,
                           B.d_mom + (size_t)m * ps, B.d_flags + m, B.d_out + m);
        MANYCHK(hipGetLastError());
      }
    }
    hipLaunchKernelGGL(k_asd_apply, dim3(nm), dim3(64), 0, J.stream, B.d_out, dim, NR, B.core.d_rows, B.core.d_cnt);
    MANYCHK(hipGetLastError());
    return LSQR_OK;
  }
  int results(AssignJob &) { return LSQR_OK; }
  void rows_down(AssignJob &J, const double *h_rows) {
    const size_t dim = J.cfg.dim;
    for (size_t m = 0; m < J.n_models; m++)
      for (size_t j = 0; j < dim; j++) J.params[m * dim + j] = h_rows[m * NR + j];
  }
  static int32_t n_params(const AssignJob &J) { return (int32_t)J.cfg.dim; }
  void fit_more(AssignJob &, int m, const unsigned long long *h_cnt, lsqr_fit_info &fit) {
    fit.reserved = (int32_t)h_cnt[ASD_ROUTE + m];
  }
  int *h_flags() { return (int *)(B.core.h_pin.get() + Pin::own); }
};
#endif  // __HIPCC__

}  // namespace lsqr
