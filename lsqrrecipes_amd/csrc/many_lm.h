// many_lm.h -- the batched Levenberg-Marquardt stage of lsqr_ransac_many_lm and lsqr_lm_fit_many: many small geometric
// sphere fits (SphereParametersEstimator::geometricLeastSquaresEstimate, the single path's lm_core.h control flow) in
// lock-step evaluation rounds, each problem stepping on its own.
//
//   k_many_lm_count   one workgroup per compaction part (<= kManyPart records of one problem): its masked records
//   k_many_lm_write   the same parts: the masked records, in record order, into the packed inlier array at the
//                     problem's offset + the counts of the problem's earlier parts
//   k_many_lm_init    one lane per problem: lm_init from its start
//   per evaluation round:
//   k_many_lm_pass    one workgroup per LM part (<= kManyPart inliers of one problem): M::accumulate_lm at the
//                     problem's trial point (its LmState in global memory), wave shuffles + LDS in a fixed order,
//                     one NMOM_LM block per part; the parts of finished problems return at once
//   k_many_lm_step    one wave per problem: its parts' blocks summed in part order, LmState and block staged in LDS,
//                     lane 0 runs lm_advance (k_lm_advance); a finished problem writes its ManyLmOut and leaves the
//                     live counter, which the host reads (4 bytes) after every round
//
// Determinism: a problem's block in every evaluation is a function of its own inliers and its own trial point only --
// its parts are fixed by its inlier count, the sums run in a fixed order within a part and across parts -- so its
// iterates do not depend on the other problems of the call, their order, or how the RANSAC rounds were cut.
//
// Included by many.h, whose kManyPart, many_grow and MANYCHK it uses; many_run and many_lm_fit there call the stage.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "devbuf.h"
#include "kernels.h"
#include "lm_core.h"

namespace lsqr {

constexpr int kManyLmWaves = 4;  // problems per workgroup of k_many_lm_step (LDS: 4 x (LmState + block) = 9 KB)

struct ManyLmProb {  // one LM problem: its records in the packed upload, its inliers in the packed inlier array
  uint64_t rec, n;   // records [rec, rec + n) of the upload
  uint64_t c0, cnt;  // inliers [c0, c0 + cnt) of the packed inlier array
  uint32_t xsrc;     // its start: row xsrc of the start array
  uint32_t pbeg;     // its LM parts [pbeg, next problem's pbeg)
};
struct ManyLmRaw {   // compaction work item: records [r0, r1) of problem q; first: q's first compaction part
  uint64_t r0, r1;
  uint32_t q, first;
};
struct ManyLmPart {  // evaluation work item: inliers [c0, c1) of problem q
  uint64_t c0, c1;
  uint32_t q, pad;
};
struct ManyLmOut {   // a finished problem (SolveOut's LM fields)
  int ok, n_params, lm_info, lm_nfev, stall, pad;
  double cost;
  double params[LM_NMAX];
};

// device and pinned buffers of the stage, owned by the context (ManyBufs) and grown on demand
struct ManyLmBufs {
  DevBuf<double> d_rec, d_partials;
  DevBuf<ManyLmProb> d_prob;
  DevBuf<ManyLmRaw> d_raw;
  DevBuf<ManyLmPart> d_parts;
  DevBuf<uint32_t> d_rcount, d_live;
  DevBuf<int> d_flag;
  DevBuf<LmState> d_state;
  DevBuf<ManyLmOut> d_out;
  PinBuf<uint32_t> h_live;
};

#if defined(__HIPCC__)
// the record flag of the compaction: inside the part and (no mask, or) its mask byte set
__device__ inline bool many_lm_in(const uint8_t *mask, uint64_t i, uint64_t r1) {
  return i < r1 && (!mask || mask[i] != 0);
}

__global__ __launch_bounds__(kBlock) void k_many_lm_count(const ManyLmRaw *__restrict__ raw,
                                                          const uint8_t *__restrict__ mask,
                                                          uint32_t *__restrict__ rcount) {
  __shared__ uint32_t s_c[kBlock / 64];
  const ManyLmRaw t = raw[blockIdx.x];
  uint32_t c = 0;
  for (uint64_t i = t.r0 + threadIdx.x; i < t.r1; i += kBlock) c += many_lm_in(mask, i, t.r1) ? 1u : 0u;
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
  if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int w = 0; w < kBlock / 64; w++) s += s_c[w];
    rcount[blockIdx.x] = s;
  }
}

// stable: the masked records of the part keep their order; D doubles per record in and out
template <int D>
__global__ __launch_bounds__(kBlock) void k_many_lm_write(const double *__restrict__ data,
                                                          const ManyLmRaw *__restrict__ raw,
                                                          const ManyLmProb *__restrict__ prob,
                                                          const uint8_t *__restrict__ mask,
                                                          const uint32_t *__restrict__ rcount,
                                                          double *__restrict__ out) {
  __shared__ uint32_t s_w[kBlock / 64];
  __shared__ uint64_t s_base;
  const ManyLmRaw t = raw[blockIdx.x];
  if (threadIdx.x == 0) {  // the problem's earlier parts (bounded by the problem's part count)
    uint64_t b = prob[t.q].c0;
    for (uint32_t k = t.first; k < blockIdx.x; k++) b += rcount[k];
    s_base = b;
  }
  __syncthreads();
  uint64_t base = s_base;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (uint64_t r = t.r0; r < t.r1; r += kBlock) {
    const uint64_t i = r + threadIdx.x;
    const bool in = many_lm_in(mask, i, t.r1);
    const uint64_t bal = __ballot(in);
    const uint32_t below = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) s_w[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t off = 0, tot = 0;
    for (int w = 0; w < kBlock / 64; w++) {
      if (w < wave) off += s_w[w];
      tot += s_w[w];
    }
    if (in) {
      const uint64_t d = base + off + below;
      for (int k = 0; k < D; k++) out[d * D + k] = data[i * D + k];
    }
    base += tot;
    __syncthreads();  // s_w is rewritten by the next chunk
  }
}

__global__ __launch_bounds__(kBlock) void k_many_lm_init(const ManyLmProb *__restrict__ prob, int Q,
                                                         const double *__restrict__ x0, size_t x0_stride, int n,
                                                         double ftol, double xtol, double gtol, int maxfev,
                                                         LmState *__restrict__ st, int *__restrict__ flag) {
  const int q = blockIdx.x * kBlock + threadIdx.x;
  if (q >= Q) return;
  lm_init(st[q], n, x0 + (size_t)prob[q].xsrc * x0_stride, ftol, xtol, gtol, maxfev, 100.0);
  flag[q] = 1;
}

// k_lm_pass over one part of one problem, at the problem's own trial point
template <class M>
__global__ __launch_bounds__(kBlock) void k_many_lm_pass(const double *__restrict__ rec,
                                                         const ManyLmPart *__restrict__ parts,
                                                         const LmState *__restrict__ st,
                                                         const int *__restrict__ flag,
                                                         double *__restrict__ partials) {
  constexpr int N = M::NMOM_LM, D = M::ND;
  __shared__ double s_m[kBlock / 64][N];
  const ManyLmPart t = parts[blockIdx.x];
  if (!flag[t.q]) return;  // finished problem (uniform over the workgroup)
  double xk[D + 1];
  for (int j = 0; j <= D; j++) xk[j] = st[t.q].xtrial[j];
  double acc[N];
#pragma unroll
  for (int k = 0; k < N; k++) acc[k] = 0.0;
  for (uint64_t i = t.c0 + threadIdx.x; i < t.c1; i += kBlock) {
    double x[D];
    for (int j = 0; j < D; j++) x[j] = rec[i * D + j];
    M::accumulate_lm(x, xk, acc);
  }
#pragma unroll
  for (int k = 0; k < N; k++) {
    double v = acc[k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    double s = 0.0;
    for (int w = 0; w < kBlock / 64; w++) s += s_m[w][threadIdx.x];
    partials[(size_t)blockIdx.x * N + threadIdx.x] = s;
  }
}

// k_lm_advance for kManyLmWaves problems per workgroup, one wave each
template <class M>
__global__ __launch_bounds__(64 * kManyLmWaves) void k_many_lm_step(LmState *__restrict__ st, int *__restrict__ flag,
                                                                    const ManyLmProb *__restrict__ prob, int Q,
                                                                    uint32_t n_parts,
                                                                    const double *__restrict__ partials,
                                                                    ManyLmOut *__restrict__ out,
                                                                    uint32_t *__restrict__ live) {
  constexpr int N = M::NMOM_LM;
  static_assert(N <= 64, "one lane per moment");
  __shared__ LmState s[kManyLmWaves];
  __shared__ double m[kManyLmWaves][N];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int q = blockIdx.x * kManyLmWaves + w;
  const bool active = q < Q && flag[q] != 0;
  constexpr int NW = (int)(sizeof(LmState) / sizeof(int));
  if (active) {
    const uint32_t p0 = prob[q].pbeg, p1 = q + 1 < Q ? prob[q + 1].pbeg : n_parts;
    if (lane < N) {
      double t = 0.0;
      for (uint32_t p = p0; p < p1; p++) t += partials[(size_t)p * N + lane];
      m[w][lane] = t;
    }
    const int *src = (const int *)&st[q];
    int *dst = (int *)&s[w];
    for (int i = lane; i < NW; i += 64) dst[i] = src[i];
  }
  __syncthreads();
  if (active && lane == 0) {
    LmState &S = s[w];
    if (!lm_advance(S, m[w])) {
      ManyLmOut &o = out[q];
      const bool ok = S.info >= 1 && S.info <= 4;  // vnl_levenberg_marquardt::minimize -> true
      o.ok = ok ? 1 : 0;
      o.lm_info = S.info;
      o.lm_nfev = S.nfev;
      o.stall = S.stall;
      o.pad = 0;
      o.cost = S.fnorm * S.fnorm;
      for (int j = 0; j < LM_NMAX; j++) o.params[j] = 0.0;
      const int np = M::lm_finalize(S.x, o.params);
      o.n_params = ok ? np : 0;
      flag[q] = 0;
      atomicSub(live, 1u);
    }
  }
  __syncthreads();
  if (active) {
    const int *src = (const int *)&s[w];
    int *dst = (int *)&st[q];
    for (int i = lane; i < NW; i += 64) dst[i] = src[i];
  }
}

// One call of the stage (filled by many_lm_job, many.h).  The records (D doubles each, packed) and the mask (nullable:
// every record) are on the device; problem q's start is row prob[q].xsrc of x0 (x0_stride doubles apart, on the
// device).  The host fills rec, n, cnt (> 0: its masked records) and xsrc; the stage fills c0 and pbeg.
struct ManyLmJob {
  hipStream_t stream;
  const double *d_data;
  const uint8_t *d_mask;
  const double *d_x0;
  size_t x0_stride;
  int n, maxfev;  // lm_settings
  double ftol, xtol, gtol;
  ManyLmBufs *buf;
  char (&err)[256];  // the ManyJob's, where MANYCHK (many.h) reports
};

template <class M>
int many_lm_run(ManyLmJob &J, std::vector<ManyLmProb> &prob, std::vector<ManyLmOut> &res) {
  constexpr int D = M::ND, N = M::NMOM_LM;
  ManyLmBufs &B = *J.buf;
  const int Q = (int)prob.size();
  res.assign(Q, ManyLmOut());
  if (Q == 0) return LSQR_OK;
  // the packed inlier array, the compaction parts and the evaluation parts: all fixed by each problem's counts
  std::vector<ManyLmRaw> raw;
  std::vector<ManyLmPart> parts;
  uint64_t c = 0;
  for (int q = 0; q < Q; q++) {
    ManyLmProb &P = prob[q];
    P.c0 = c;
    c += P.cnt;
    const uint32_t first = (uint32_t)raw.size();
    for (uint64_t r = 0; r < P.n; r += kManyPart)
      raw.push_back(ManyLmRaw{P.rec + r, P.rec + std::min<uint64_t>(P.n, r + kManyPart), (uint32_t)q, first});
    P.pbeg = (uint32_t)parts.size();
    for (uint64_t r = 0; r < P.cnt; r += kManyPart)
      parts.push_back(ManyLmPart{P.c0 + r, P.c0 + std::min<uint64_t>(P.cnt, r + kManyPart), (uint32_t)q, 0});
  }
  const uint64_t C = c;
  MANYCHK(many_grow(B.d_rec, std::max<uint64_t>(C, 1) * D));
  MANYCHK(many_grow(B.d_prob, (size_t)Q));
  MANYCHK(many_grow(B.d_raw, raw.size()));
  MANYCHK(many_grow(B.d_rcount, raw.size()));
  MANYCHK(many_grow(B.d_parts, parts.size()));
  MANYCHK(many_grow(B.d_partials, parts.size() * N));
  MANYCHK(many_grow(B.d_flag, (size_t)Q));
  MANYCHK(many_grow(B.d_state, (size_t)Q));
  MANYCHK(many_grow(B.d_out, (size_t)Q));
  MANYCHK(many_grow(B.d_live, 1));
  if (!B.h_live) MANYCHK(B.h_live.alloc(16));
  // (the host vectors are pageable: these copies complete before the calls return)
  MANYCHK(hipMemcpyAsync(B.d_prob, prob.data(), sizeof(ManyLmProb) * Q, hipMemcpyHostToDevice, J.stream));
  MANYCHK(hipMemcpyAsync(B.d_raw, raw.data(), sizeof(ManyLmRaw) * raw.size(), hipMemcpyHostToDevice, J.stream));
  MANYCHK(hipMemcpyAsync(B.d_parts, parts.data(), sizeof(ManyLmPart) * parts.size(), hipMemcpyHostToDevice,
                           J.stream));
  hipLaunchKernelGGL(k_many_lm_count, dim3((unsigned)raw.size()), dim3(kBlock), 0, J.stream, B.d_raw, J.d_mask,
                     B.d_rcount);
  MANYCHK(hipGetLastError());
  hipLaunchKernelGGL((k_many_lm_write<D>), dim3((unsigned)raw.size()), dim3(kBlock), 0, J.stream, J.d_data, B.d_raw,
                     B.d_prob, J.d_mask, B.d_rcount, B.d_rec);
  MANYCHK(hipGetLastError());
  hipLaunchKernelGGL(k_many_lm_init, dim3((unsigned)((Q + kBlock - 1) / kBlock)), dim3(kBlock), 0, J.stream, B.d_prob,
                     Q, J.d_x0, J.x0_stride, J.n, J.ftol, J.xtol, J.gtol, J.maxfev, B.d_state, B.d_flag);
  MANYCHK(hipGetLastError());
  *B.h_live = (uint32_t)Q;
  MANYCHK(hipMemcpyAsync(B.d_live, B.h_live, sizeof(uint32_t), hipMemcpyHostToDevice, J.stream));
  MANYCHK(hipStreamSynchronize(J.stream));  // (h_live is written again below)

  // diagnostics (LSQR_MANY_TRACE): per round the live problems, the parts launched, pass / step time, device wait
  static const bool trace = getenv("LSQR_MANY_TRACE") != nullptr;
  typedef std::chrono::steady_clock Clock;
  Event ev[3];
  if (trace)
    for (auto &e : ev) MANYCHK(e.create());
  uint32_t live = (uint32_t)Q;
  const unsigned n_steps = (unsigned)((Q + kManyLmWaves - 1) / kManyLmWaves);
  // every lm_advance call consumes one evaluation and stops at maxfev: maxfev rounds finish every problem
  int round = 0;
  for (; live > 0; round++) {
    if (round > J.maxfev) {
      snprintf(J.err, sizeof J.err, "LM stage: %u problems still live after %d rounds", live, round);
      return LSQR_ERR_HIP;
    }
    if (trace) MANYCHK(hipEventRecord(ev[0], J.stream));
    hipLaunchKernelGGL((k_many_lm_pass<M>), dim3((unsigned)parts.size()), dim3(kBlock), 0, J.stream, B.d_rec,
                       B.d_parts, B.d_state, B.d_flag, B.d_partials);
    MANYCHK(hipGetLastError());
    if (trace) MANYCHK(hipEventRecord(ev[1], J.stream));
    hipLaunchKernelGGL((k_many_lm_step<M>), dim3(n_steps), dim3(64 * kManyLmWaves), 0, J.stream, B.d_state, B.d_flag,
                       B.d_prob, Q, (uint32_t)parts.size(), B.d_partials, B.d_out, B.d_live);
    MANYCHK(hipGetLastError());
    if (trace) MANYCHK(hipEventRecord(ev[2], J.stream));
    MANYCHK(hipMemcpyAsync(B.h_live, B.d_live, sizeof(uint32_t), hipMemcpyDeviceToHost, J.stream));
    const Clock::time_point t0 = Clock::now();
    MANYCHK(hipStreamSynchronize(J.stream));
    const double wait = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
    const uint32_t now = *B.h_live;
    if (trace) {
      float t_pass = 0.f, t_step = 0.f;
      MANYCHK(hipEventElapsedTime(&t_pass, ev[0], ev[1]));
      MANYCHK(hipEventElapsedTime(&t_step, ev[1], ev[2]));
      fprintf(stderr, "ransac_many lm round %d: %u live problems, %zu parts, pass %.3f ms, step %.3f ms, wait %.3f ms\n",
              round, live, parts.size(), t_pass, t_step, wait);
    }
    if (now > live) {
      snprintf(J.err, sizeof J.err, "LM stage: live counter rose from %u to %u", live, now);
      return LSQR_ERR_HIP;
    }
    live = now;
  }
  MANYCHK(hipMemcpyAsync(res.data(), B.d_out, sizeof(ManyLmOut) * Q, hipMemcpyDeviceToHost, J.stream));
  MANYCHK(hipStreamSynchronize(J.stream));
  return LSQR_OK;
}
#endif

}  // namespace lsqr
