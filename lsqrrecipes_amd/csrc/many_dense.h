// many_dense.h -- lsqr_ransac_many_dense: many independent RANSAC<T,S>::compute() problems of
// DenseLinearEquationSystemParametersEstimator<double,n> (n = 1..64, records of n + 1 doubles) in one call, and
// lsqr_dense_fit_many: the least-squares finish alone over many row sets.  The host frame is lsqr_ransac_many's
// (many.h: many_begin, many_rounds -- packed upload, 256 -> 1024 -> 4096 batches, host_replay with one DedupSet per
// problem, k = n --, many_plan_finish .. many_end; many_fit_begin / many_write_fits for the fit alone); here are
// many_dense_run's round kernels, many_dense_finish and the dense single path's arithmetic, per problem:
//
//   k_many_dense_estimate_w4   one wave per (problem, hypothesis), four per workgroup: the subset drawn by the wave
//                              (k_sample_wave's rule = ctr_subset) on the problem's stream, the n x n system gathered
//                              from rec + idx into the wave's LDS area, wave_gepp_solve (= k_estimate_dense_w4)
//   k_many_dense_estimate_r64  n = 64: the same with the system in registers, lane = row (= k_estimate_dense_r64)
//   k_many_dense_svd           the systems the elimination refused (all of them with dense_fast_solve 0), from a
//                              device list: one workgroup each, block_pinv_solve (= k_estimate_dense's SVD path)
//   k_many_dense_scan<NR>      one workgroup per tile (<= 256 hypotheses x <= many_dense_seg<NR> rows of one
//                              problem); lane = hypothesis, its NR parameters in registers; the rows staged through
//                              LDS (many_dense_stage<NR> rows, zero-padded to NR slots + b) and read at the same
//                              address by every lane; the vote is DenseModel::agree's running sum, exact
//   k_many_dense_mask_moments  one workgroup per part (<= kManyPart rows of one problem): consensus mask (or the
//                              caller's mask) + the packed (n+1)(n+2)/2 block of sum z z^T, z = (a | b), over the rows
//                              in use, each entry summed by one thread in row order; + the part's count
//   k_many_dense_sum           one workgroup per finishing problem: its parts' blocks summed in part order
//   k_many_dense_solve         one workgroup per finishing problem: k_solve_dense's body (solve_dense_wg) with a
//                              flag per problem; flagged problems (pivot below 1e-6 max|G|: ill-conditioned) are
//                              solved again from their rows by k_gram_dd_dense + k_dense_dd_solve over the problem's
//                              row range and mask -- the single path's kernels, launched per flagged problem
//
// Padding: the parameters are NR in {8, 16, 32, 64} doubles (n .. NR - 1 zero), the rows NR coefficient slots (zero
// beyond n) + b; the 0.0 * 0.0 terms leave the running sum bit-identical (dense.h).
// Independence: a problem's hypotheses, votes (integer sums over its tiles), moment block (fixed parts, fixed order)
// and solve depend on its own records alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "dense.h"
#include "many.h"

namespace lsqr {

template <int NR> constexpr int many_dense_stage() { return 4096 / NR; }       // rows per LDS stage (33-40 KiB)
template <int NR> constexpr uint64_t many_dense_seg() { return 131072 / NR; }  // rows per scan tile
constexpr int kManyDenseWaves = 4;                   // minimal solves per workgroup of k_many_dense_estimate_w4
constexpr size_t kManyDenseRoundBytes = 256u << 20;  // device memory of a round's hypotheses (default round cap)
constexpr unsigned kManyDenseSvdGrid = 2048;         // workgroups of k_many_dense_svd (a loop over the list)

// the default round cap of the dense call: hypotheses whose parameters, subsets, votes and flags fit in
// kManyDenseRoundBytes, at most lsqr_ransac_many's 2^21 (2^21 up to n = 8, n = 16: 1.3 M, n = 64: 343 000)
inline size_t many_dense_round_cap(int n, int NR) {
  const size_t per = sizeof(double) * NR + sizeof(uint32_t) * n + 14;
  return std::min<size_t>(kManyRoundDefault, kManyDenseRoundBytes / per);
}
// dynamic LDS of k_many_dense_solve / k_many_dense_svd (dense_lds_bytes of the single path)
inline size_t many_dense_lds(int n) { return sizeof(double) * ((size_t)2 * n * (n | 1) + 3 * n); }
// packed moment block: (n+1)(n+2)/2 entries + the count, padded to 8 doubles
inline int many_dense_ps(int n) { return ((n + 1) * (n + 2) / 2 + 1 + 7) & ~7; }

#if defined(__HIPCC__)
// the item of round row h (the last with h0 <= h)
__device__ inline ManyItem many_item_of(const ManyItem *__restrict__ items, int n_items, uint32_t h) {
  int lo = 0, hi = n_items - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (items[mid].h0 <= h) lo = mid;
    else hi = mid - 1;
  }
  return items[lo];
}

// draw `lane` of hypothesis h of stream `seed` over n records (k_sample_wave: the rule of ctr_subset); the calling
// wave is converged, lanes >= K get 0
__device__ inline uint32_t many_dense_draw(uint64_t seed, uint64_t h, uint64_t n, int K) {
  const int lane = threadIdx.x & 63;
  uint32_t sorted = 0xFFFFFFFFu, mine = 0;
  for (int l = 0; l < K; l++) {
    const uint64_t u = mix64(seed + 0x9E3779B97F4A7C15ULL * (h * 64ULL + (uint64_t)l + 1ULL));
    const uint32_t rank = (uint32_t)mulhi64(u, n - (uint64_t)l);
    uint32_t v = rank, cnt = 0;
    for (;;) {
      cnt = (uint32_t)__builtin_popcountll(__ballot(sorted <= v));
      const uint32_t nv = rank + cnt;
      if (nv == v) break;
      v = nv;
    }
    const uint32_t up = __shfl_up(sorted, 1);
    if ((uint32_t)lane == cnt) sorted = v;
    else if ((uint32_t)lane > cnt) sorted = up;
    if (lane == l) mine = v;
  }
  return mine;
}

// the outcome of one minimal solve: ok -> valid 1; refused -> valid 2 and onto the SVD list
__device__ inline void many_dense_mark(uint32_t h, bool ok, uint8_t *__restrict__ valid, uint32_t *__restrict__ marked,
                                       uint32_t *__restrict__ n_marked) {
  valid[h] = ok ? 1 : 2;
  if (!ok) marked[atomicAdd(n_marked, 1u)] = h;
}

// fast == 0: draw only, every system to the SVD list.  LDS: kManyDenseWaves x (n (n | 1) + 2 n) doubles.
__global__ __launch_bounds__(64 * kManyDenseWaves) void k_many_dense_estimate_w4(
    const double *__restrict__ data, const ManyItem *__restrict__ items, int n_items, uint32_t H, int n, int sp,
    int fast, uint32_t *__restrict__ sub, double *__restrict__ hparams, uint8_t *__restrict__ valid,
    uint32_t *__restrict__ marked, uint32_t *__restrict__ n_marked) {
  extern __shared__ double sm[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t h = blockIdx.x * kManyDenseWaves + wave;
  if (h >= H) return;  // wave-uniform; no workgroup barrier below
  const ManyItem it = many_item_of(items, n_items, h);
  const uint32_t mine = many_dense_draw(it.seed, it.first + (h - it.h0), it.n, n);
  if (lane < n) sub[(size_t)h * n + lane] = mine;
  bool ok = false;
  if (fast) {
    const int lda = n | 1, w = n + 1;
    double *A = sm + (size_t)wave * (n * lda + 2 * n), *b = A + n * lda, *x = b + n;
    for (int l = 0; l < n; l++) {  // lane = column: one coalesced read of a row's n doubles (k_estimate_dense_w4)
      const uint64_t i = it.rec + (uint32_t)__shfl((int)mine, l);
      if (lane < n) A[lane * lda + l] = data[i * w + lane];
      if (lane == 0) b[l] = data[i * w + n];
    }
    __builtin_amdgcn_wave_barrier();
    ok = wave_gepp_solve(n, A, lda, b, x);
    __builtin_amdgcn_wave_barrier();
    const double qnan = __builtin_nan("");
    for (int j = lane; j < sp; j += 64) hparams[(size_t)h * sp + j] = j < n ? (ok ? x[j] : qnan) : 0.0;
  }
  if (lane == 0) many_dense_mark(h, ok, valid, marked, n_marked);
}

// n = 64, dense_fast_solve: one wave per hypothesis, the system in registers (k_estimate_dense_r64)
__global__ __launch_bounds__(64) void k_many_dense_estimate_r64(const double *__restrict__ data,
                                                                const ManyItem *__restrict__ items, int n_items,
                                                                uint32_t H, uint32_t *__restrict__ sub,
                                                                double *__restrict__ hparams,
                                                                uint8_t *__restrict__ valid,
                                                                uint32_t *__restrict__ marked,
                                                                uint32_t *__restrict__ n_marked) {
  const int lane = threadIdx.x;
  const uint32_t h = blockIdx.x;
  if (h >= H) return;
  const ManyItem it = many_item_of(items, n_items, h);
  const uint32_t mine = many_dense_draw(it.seed, it.first + (h - it.h0), it.n, 64);
  sub[(size_t)h * 64 + lane] = mine;
  const double *row = data + (it.rec + mine) * 65;
  double a[64], xv;
#pragma unroll
  for (int c = 0; c < 64; c++) a[c] = row[c];
  const bool ok = wave_gepp_solve_reg64(a, row[64], xv);
  hparams[(size_t)h * 64 + lane] = ok ? xv : __builtin_nan("");
  if (lane == 0) many_dense_mark(h, ok, valid, marked, n_marked);
}

// the listed systems through the SVD pseudo-inverse, x = pinv(A) b, singular if any sigma <= EPS
// (DenseLinear...Estimator.hxx:17-49; k_estimate_dense).  LDS: many_dense_lds(n).
__global__ __launch_bounds__(256) void k_many_dense_svd(const double *__restrict__ data,
                                                        const ManyItem *__restrict__ items, int n_items,
                                                        const uint32_t *__restrict__ sub,
                                                        const uint32_t *__restrict__ marked,
                                                        const uint32_t *__restrict__ n_marked, int n, int sp,
                                                        double *__restrict__ hparams, uint8_t *__restrict__ valid) {
  extern __shared__ double sm[];
  const int tid = threadIdx.x, lda = n | 1, w = n + 1;
  double *A = sm, *V = A + n * lda, *b = V + n * lda, *cw = b + n, *x = cw + n;
  const uint32_t cnt = *n_marked;
  const double qnan = __builtin_nan("");
  for (uint32_t q = blockIdx.x; q < cnt; q += gridDim.x) {
    const uint32_t h = marked[q];
    const ManyItem it = many_item_of(items, n_items, h);
    const uint32_t *s = sub + (size_t)h * n;
    __syncthreads();  // the previous system has been read
    for (int idx = tid; idx < n * n; idx += 256) {
      const int l = idx / n, c = idx % n;
      A[c * lda + l] = data[(it.rec + s[l]) * w + c];
    }
    for (int l = tid; l < n; l += 256) b[l] = data[(it.rec + s[l]) * w + n];
    __syncthreads();
    const int rank = block_pinv_solve<256>(n, n, A, lda, V, lda, b, kEPS, 0.0, x, cw);
    __syncthreads();
    const bool ok = rank == n;
    for (int j = tid; j < sp; j += 256) hparams[(size_t)h * sp + j] = j < n ? (ok ? x[j] : qnan) : 0.0;
    if (tid == 0) valid[h] = ok ? 1 : 0;
  }
}

// rows [r0, r0 + m) of the packed upload (n + 1 doubles each) -> LDS: NR coefficient slots (zero beyond n), b in slot
// NR, slot NR + 1 zero
template <int NR>
__device__ inline void many_dense_stage_rows(const double *__restrict__ data, int n, uint64_t r0, uint32_t m,
                                             double *__restrict__ s_rec) {
  constexpr int PITCH = NR + 2;
  const int w = n + 1;
  const double *src = data + r0 * w;
  for (uint32_t q = threadIdx.x; q < m * PITCH; q += blockDim.x) {
    const uint32_t r = q / PITCH, k = q - r * PITCH;
    s_rec[q] = (int)k < n ? src[(size_t)r * w + k] : (k == NR ? src[(size_t)r * w + n] : 0.0);
  }
}

// DenseModel::agree: the reference's running sum over the NR slots, then - b
template <int NR>
__device__ inline bool many_dense_agree(const double *__restrict__ row, const double (&x)[NR], double delta) {
  double sum = 0.0;
#pragma unroll
  for (int k = 0; k < NR; k++) sum += row[k] * x[k];
  sum -= row[NR];
  return fabs(sum) < delta;
}

template <int NR>
__global__ __launch_bounds__(kManyBlock) void k_many_dense_scan(const double *__restrict__ data, int n,
                                                                const ManyTile *__restrict__ tiles,
                                                                const double *__restrict__ hparams,
                                                                const uint8_t *__restrict__ valid, double delta,
                                                                uint32_t *__restrict__ votes) {
  constexpr int S = many_dense_stage<NR>(), PITCH = NR + 2;
  __shared__ double s_rec[S * PITCH];
  const ManyTile t = tiles[blockIdx.x];
  const uint32_t lane = threadIdx.x;
  const bool live = lane < t.nh && valid[t.h0 + lane];
  double x[NR];
#pragma unroll
  for (int k = 0; k < NR; k++) x[k] = live ? hparams[(size_t)(t.h0 + lane) * NR + k] : 0.0;
  uint32_t c = 0;
  for (uint64_t r0 = t.r0; r0 < t.r1; r0 += S) {
    const uint32_t m = (uint32_t)(t.r1 - r0 < (uint64_t)S ? t.r1 - r0 : (uint64_t)S);
    __syncthreads();  // the previous stage has been read
    many_dense_stage_rows<NR>(data, n, r0, m, s_rec);
    __syncthreads();
    if (live)
      for (uint32_t i = 0; i < m; i++) c += many_dense_agree<NR>(s_rec + i * PITCH, x, delta) ? 1u : 0u;
  }
  if (live && c) atomicAdd(&votes[t.h0 + lane], c);
}

// best (nullable): the winners' rows (NR doubles per problem) -> consensus mask into mask_out; without best the rows
// in use are those of mask_in (nullable: all).  partials[part][ps]: the block, then the part's count.
template <int NR>
__global__ __launch_bounds__(256) void k_many_dense_mask_moments(const double *__restrict__ data, int n,
                                                                 const ManyPart *__restrict__ parts,
                                                                 const double *__restrict__ best, double delta,
                                                                 const uint8_t *__restrict__ mask_in,
                                                                 uint8_t *__restrict__ mask_out,
                                                                 unsigned long long *__restrict__ counts,
                                                                 double *__restrict__ partials, int ps) {
  constexpr int S = many_dense_stage<NR>(), PITCH = NR + 2, U = ((NR + 1) * (NR + 2) / 2 + 255) / 256;
  __shared__ double s_rec[S * PITCH];
  __shared__ uint8_t s_use[S];
  __shared__ uint32_t s_c[4];
  const ManyPart pt = parts[blockIdx.x];
  const int tid = threadIdx.x, nz = n + 1, ne = nz * (nz + 1) / 2;
  double x[NR];
#pragma unroll
  for (int k = 0; k < NR; k++) x[k] = best ? best[(size_t)pt.j * NR + k] : 0.0;
  // this thread's entries e = tid + 256 u of the packed upper triangle -> the LDS slots of (a, b); beyond ne the zero
  // slot NR + 1
  int ea[U], eb[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int e = tid + 256 * u;
    ea[u] = eb[u] = NR + 1;
    if (e < ne) {
      int a = 0, rem = e;
      while (rem >= nz - a) rem -= nz - a++;
      const int b = a + rem;
      ea[u] = a < n ? a : NR;
      eb[u] = b < n ? b : NR;
    }
  }
  double acc[U];
#pragma unroll
  for (int u = 0; u < U; u++) acc[u] = 0.0;
  uint32_t local = 0;
  for (uint64_t r0 = pt.r0; r0 < pt.r1; r0 += S) {
    const uint32_t m = (uint32_t)(pt.r1 - r0 < (uint64_t)S ? pt.r1 - r0 : (uint64_t)S);
    __syncthreads();  // the previous stage has been read
    many_dense_stage_rows<NR>(data, n, r0, m, s_rec);
    __syncthreads();
    for (uint32_t r = tid; r < m; r += 256) {
      bool a;
      if (best) {
        a = many_dense_agree<NR>(s_rec + r * PITCH, x, delta);
        mask_out[r0 + r] = a ? 1 : 0;
      } else {
        a = !mask_in || mask_in[r0 + r] != 0;
      }
      s_use[r] = a ? 1 : 0;
      local += a ? 1u : 0u;
    }
    __syncthreads();
    for (uint32_t r = 0; r < m; r++) {
      if (!s_use[r]) continue;  // workgroup-uniform
      const double *z = s_rec + r * PITCH;
#pragma unroll
      for (int u = 0; u < U; u++) acc[u] += z[ea[u]] * z[eb[u]];
    }
  }
  for (int o = 32; o > 0; o >>= 1) local += __shfl_down(local, o);
  if ((tid & 63) == 0) s_c[tid >> 6] = local;
  double *out = partials + (size_t)blockIdx.x * ps;
#pragma unroll
  for (int u = 0; u < U; u++)
    if (tid + 256 * u < ne) out[tid + 256 * u] = acc[u];
  __syncthreads();
  if (tid == 0) {
    const uint32_t t = s_c[0] + s_c[1] + s_c[2] + s_c[3];
    out[ne] = (double)t;
    if (t) atomicAdd(&counts[pt.f], (unsigned long long)t);
  }
}

// finishing problem f: the blocks of its parts [pbeg[f], pbeg[f+1]) summed in part order -> mom[f]
__global__ __launch_bounds__(256) void k_many_dense_sum(const double *__restrict__ partials,
                                                        const uint32_t *__restrict__ pbeg, int n, int ps,
                                                        double *__restrict__ mom) {
  const uint32_t f = blockIdx.x;
  const int ne = (n + 1) * (n + 2) / 2;
  for (int e = threadIdx.x; e <= ne; e += 256) {
    double t = 0.0;
    for (uint32_t q = pbeg[f]; q < pbeg[f + 1]; q++) t += partials[(size_t)q * ps + e];
    mom[(size_t)f * ps + e] = t;
  }
}

// flags (nullable: dense_dd 0, the block alone decides): one per problem, zeroed by the caller
__global__ __launch_bounds__(256) void k_many_dense_solve(const double *__restrict__ mom, int ps, int n, int fast,
                                                          SolveOut *__restrict__ out, int *__restrict__ flags) {
  const uint32_t f = blockIdx.x;
  solve_dense_wg(mom + (size_t)f * ps, n, fast, out + f, flags ? flags + f : nullptr);
}
#endif

// ---- host side -------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
// The finish of F's slots: mask / moments -> solve, the double-double route for the flagged ones.  best: the winners'
// rows (the consensus mask is written to B.d_mask) or nullptr (mask_in, nullable, on the device).  The counts and fits
// stay on the device for many_fetch_finish.
template <int NR>
int many_dense_finish(ManyJob &J, const ManyFinish &F, const double *best, const uint8_t *mask_in) {
  ManyBufs &B = *J.buf;
  const int n = (int)J.cfg.dim, ps = many_dense_ps(n);
  const size_t NF = F.size();
  int st;
  if (NF == 0) return LSQR_OK;
  if ((st = many_stage_finish(J, F, false)) != LSQR_OK) return st;  // (no kernel here reads fin)
  MANYCHK(many_grow(B.d_flags, NF));
  MANYCHK(many_grow(B.d_mom, NF * ps));
  MANYCHK(many_grow(B.d_partials, F.parts.size() * ps));
  MANYCHK(hipMemsetAsync(B.d_flags, 0, sizeof(int) * NF, J.stream));
  hipLaunchKernelGGL((k_many_dense_mask_moments<NR>), dim3((unsigned)F.parts.size()), dim3(256), 0, J.stream, B.d_data,
                     n, B.d_parts, best, J.mc.delta, mask_in, B.d_mask, B.d_counts, B.d_partials, ps);
  MANYCHK(hipGetLastError());
  hipLaunchKernelGGL(k_many_dense_sum, dim3((unsigned)NF), dim3(256), 0, J.stream, B.d_partials, B.d_pbeg, n, ps,
                     B.d_mom);
  MANYCHK(hipGetLastError());
  (void)hipFuncSetAttribute((const void *)k_many_dense_solve, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)many_dense_lds(64));
  hipLaunchKernelGGL(k_many_dense_solve, dim3((unsigned)NF), dim3(256), many_dense_lds(n), J.stream, B.d_mom, ps, n,
                     J.dense_fast, B.d_out, J.dense_dd ? B.d_flags : (int *)nullptr);
  MANYCHK(hipGetLastError());
  std::vector<int> flags(NF, 0);
  if (J.dense_dd) {
    MANYCHK(hipMemcpyAsync(flags.data(), B.d_flags, sizeof(int) * NF, hipMemcpyDeviceToHost, J.stream));
    MANYCHK(hipStreamSynchronize(J.stream));
    // the ill-conditioned ones again from their rows, in double-double (launch_solve_dense's route, per problem)
    bool any = false;
    for (size_t f = 0; f < NF; f++) {
      if (!flags[f]) continue;
      if (!any) {
        MANYCHK(many_grow(B.d_ddpart, (size_t)2 * kDdNe * kDdBlocks));
        (void)hipFuncSetAttribute((const void *)k_dense_dd_solve, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)dense_dd_lds(64));
        any = true;
      }
      const uint64_t begin = J.offsets[F.fin[f]], end = J.offsets[F.fin[f] + 1];
      const int nb = (int)std::min<uint64_t>(kDdBlocks, (end - begin + 31) / 32);
      const uint8_t *mk = best ? B.d_mask : mask_in;
      hipLaunchKernelGGL((k_gram_dd_dense<32>), dim3(nb), dim3(256), 0, J.stream, B.d_data, (size_t)(n + 1),
                         (size_t)begin, (size_t)end, n, mk, B.d_flags + f, B.d_ddpart);
      MANYCHK(hipGetLastError());
      hipLaunchKernelGGL(k_dense_dd_solve, dim3(1), dim3(256), dense_dd_lds(n), J.stream, B.d_ddpart, nb, n,
                         B.d_mom + f * ps, B.d_flags + f, B.d_out + f);
      MANYCHK(hipGetLastError());
    }
  }
  return LSQR_OK;
}

template <int NR>
int many_dense_run(ManyJob &J) {
  ManyBufs &B = *J.buf;
  const int n = (int)J.cfg.dim, K = n;
  int st0;
  if (J.round_cap == 0) J.round_cap = many_dense_round_cap(n, NR);
  std::vector<ManyProb> pr;
  if ((st0 = many_begin(J, n + 1, K, NR, pr)) != LSQR_OK) return st0;
  const size_t lds_w4 = sizeof(double) * kManyDenseWaves * ((size_t)n * (n | 1) + 2 * n);
  (void)hipFuncSetAttribute((const void *)k_many_dense_estimate_w4, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(sizeof(double) * kManyDenseWaves * (64 * 65 + 128)));
  (void)hipFuncSetAttribute((const void *)k_many_dense_svd, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)many_dense_lds(64));
  if ((st0 = many_rounds(J, pr, K, NR, many_dense_seg<NR>(), [&](size_t n_items, uint64_t Ht, size_t n_tiles) -> int {
         MANYCHK(many_grow(B.d_sub, Ht * n));
         MANYCHK(many_grow(B.d_marked, Ht + 1));
         uint32_t *d_cnt = B.d_marked + Ht;  // the list's length, after the list
         MANYCHK(hipMemsetAsync(d_cnt, 0, sizeof(uint32_t), J.stream));
         if (n == 64 && J.dense_fast)
           hipLaunchKernelGGL(k_many_dense_estimate_r64, dim3((unsigned)Ht), dim3(64), 0, J.stream, B.d_data,
                              B.d_items, (int)n_items, (uint32_t)Ht, B.d_sub, B.d_hparams, B.d_valid, B.d_marked,
                              d_cnt);
         else
           hipLaunchKernelGGL(k_many_dense_estimate_w4,
                              dim3((unsigned)((Ht + kManyDenseWaves - 1) / kManyDenseWaves)),
                              dim3(64 * kManyDenseWaves), J.dense_fast ? lds_w4 : 0, J.stream, B.d_data, B.d_items,
                              (int)n_items, (uint32_t)Ht, n, NR, J.dense_fast, B.d_sub, B.d_hparams, B.d_valid,
                              B.d_marked, d_cnt);
         MANYCHK(hipGetLastError());
         hipLaunchKernelGGL(k_many_dense_svd, dim3((unsigned)std::min<uint64_t>(Ht, kManyDenseSvdGrid)), dim3(256),
                            many_dense_lds(n), J.stream, B.d_data, B.d_items, (int)n_items, B.d_sub, B.d_marked,
                            d_cnt, n, NR, B.d_hparams, B.d_valid);
         MANYCHK(hipGetLastError());
         hipLaunchKernelGGL((k_many_dense_scan<NR>), dim3((unsigned)n_tiles), dim3(kManyBlock), 0, J.stream,
                            B.d_data, n, B.d_tiles, B.d_hparams, B.d_valid, J.mc.delta, B.d_votes);
         MANYCHK(hipGetLastError());
         return LSQR_OK;
       })) != LSQR_OK)
    return st0;

  // ---- finish: finish_ransac for every problem with a winner (the dense moments have no origin) -------------------
  ManyFinish F = many_plan_finish(J, pr, K, [](size_t, const ManyProb &) -> uint64_t { return 0; });
  if (F.size()) MANYCHK(many_grow(B.d_mask, J.offsets[J.n]));
  if ((st0 = many_dense_finish<NR>(J, F, B.d_best, nullptr)) != LSQR_OK) return st0;
  if ((st0 = many_fetch_finish(J, F, true)) != LSQR_OK) return st0;
  // fit.reserved = SolveOut::pad: 1: the double-double route (2: dense_dd 0 and a pivot below 1e-6, as lsqr_ransac);
  // solve_dense_wg and k_dense_dd_solve write it, and lm_info = lm_nfev = 0, on every path
  many_end(J, F, n);
  return LSQR_OK;
}

// lsqr_dense_fit_many: set j = records [offsets[j], offsets[j+1]) where masks (nullable: every record) is set; the
// single-set path's result (lsqr_upload + lsqr_set_mask + lsqr_ls_fit)
template <int NR>
int many_dense_fit(ManyJob &J, const uint8_t *masks, lsqr_fit_info *fits) {
  const int n = (int)J.cfg.dim;
  std::vector<uint32_t> sets;
  std::vector<uint64_t> used;
  int st;
  if ((st = many_fit_begin(J, n + 1, masks, sets, used)) != LSQR_OK || sets.empty()) return st;
  ManyFinish F;
  for (uint32_t j : sets) F.add(j, J.offsets[j], J.offsets[j + 1], 0);
  if ((st = many_dense_finish<NR>(J, F, nullptr, masks ? J.buf->d_mask : nullptr)) != LSQR_OK) return st;
  if ((st = many_fetch_finish(J, F, false)) != LSQR_OK) return st;
  many_write_fits(J, fits, n, sets, used, F.outs);
  return LSQR_OK;
}
#endif

}  // namespace lsqr
