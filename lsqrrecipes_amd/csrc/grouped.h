// grouped.h -- lsqr_ransac_grouped: one RANSAC problem per label over the records the context already holds on the
// device (its upload or attach), the labels interleaved.  The records are grouped by label on the device, stably, into
// the packed buffer of the batched calls; ONE batched RANSAC job -- the unchanged many_run / many_dense_run, told that
// its records are resident -- runs on that copy; the consensus bytes go back in the caller's record order.
//
//   k_grp_keys     one lane per record: key = its label, or n_groups for a record in no problem (a negative label or
//                  one >= n_groups: those sort last); value = the record's index
//   (sort.h)       stable radix sort of the pairs over the key bits [0, bits(n_groups)); stability keeps every
//                  problem's records in upload order, which is what its subset indices refer to
//   k_grp_offsets  one lane per g in 0 .. n_groups: the first position of a key >= g in the sorted keys (binary search)
//   k_grp_gather   row r of the packed buffer = record perm[r], W 8-byte words copied as integers from the context's
//                  stride; lane = word of the packed buffer, so the writes are coalesced and the reads are runs of W
//                  words
//   k_grp_scatter  one lane per sorted position r: consensus[perm[r]] = the job's mask byte of r where r's problem has
//                  a winner, else 0 (also for the records in no problem); perm is a permutation, so every byte of the
//                  consensus is written exactly once
//   k_grp_scatter_labels  (lsqr_ransac_grouped_sequential) one lane per sorted position r: labels[perm[r]] = the round
//                  label of packed position r, or -1 for the records in no problem (r >= the grouped total); written
//                  exactly once, as the consensus is
//   k_grp_scatter_f64     (lsqr_assign_grouped) the same for a packed array of doubles, with a fill value
//
// "A problem with a winner" is one whose search took a finishing slot (fit.n_used > 0), NOT "status LSQR_OK": a winner
// whose final least-squares fit fails ends LSQR_EMPTY with its hypothesis' consensus in the mask, and lsqr_ransac_many
// hands those bytes out.  So does this call: an LSQR_EMPTY group can carry non-zero consensus bytes, as problem g of
// the host call on the gather does.  Every other status without a winner (LSQR_ERR_INVALID for N_g < k, no hypothesis
// accepted) has all its records' bytes 0.
//
// The n_groups + 1 offsets cross to the host once, and the call synchronises there: the batched job plans its rounds
// on the host (many_begin, many_rounds) from host offsets.  The job's own mask is defined only for the problems with a
// winner (many_finish / many_dense_run write it for the finishing problems alone), so the per-problem winner flag
// goes back up before the scatter.  No workgroup waits on another; the order between the kernels is the stream's; no
// atomics.
//
// Why the call equals lsqr_ransac_many on the gather: the job's records are the stable gather by label of the
// context's records, tightly packed, bit for bit (integer copies), under the prefix sums of the group sizes -- the
// bytes a host that had gathered them would upload -- and its kernels and host replay are many_run's /
// many_dense_run's.
//
// lsqr_ransac_grouped_sequential (grouped_seq_run) is the same front half -- grouped_pack: keys, sort, offsets, the one
// synchronisation, the gather -- followed by many_seq_run (many_sequential.h) on the resident packed buffer instead of
// one job: round 0 reads what the gather wrote, the later rounds are many_seq_run's own, and its round labels, which
// it leaves on the device in packed order, go back to upload order through k_grp_scatter_labels.  It equals
// lsqr_ransac_many_sequential on the gather for the reason above, applied to round 0; every later round is the same
// code on the same bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "many.h"
#include "many_dense.h"
#include "many_sequential.h"
#include "sort.h"

namespace lsqr {

constexpr unsigned kGrpMaxGrid = 1u << 16;  // workgroups per launch; the kernels stride over the rest

#if defined(__HIPCC__)
__global__ __launch_bounds__(kBlock) void k_grp_keys(const int32_t *__restrict__ groups, uint32_t n,
                                                     uint32_t n_groups, uint32_t *__restrict__ keys,
                                                     uint32_t *__restrict__ vals) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const uint32_t g = (uint32_t)groups[i];  // (a negative label is above every n_groups <= 2^31 - 1)
    keys[i] = g < n_groups ? g : n_groups;
    vals[i] = (uint32_t)i;
  }
}

__global__ __launch_bounds__(kBlock) void k_grp_offsets(const uint32_t *__restrict__ keys, uint32_t n,
                                                        uint32_t n_groups, uint64_t *__restrict__ offsets) {
  for (uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g <= n_groups; g += (uint64_t)gridDim.x * kBlock) {
    uint32_t lo = 0, hi = n;  // the first position in [0, n] whose key is >= g
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (keys[mid] < (uint32_t)g) lo = mid + 1;
      else hi = mid;
    }
    offsets[g] = lo;
  }
}

// src: the context's records, stride words apart; dst: total rows of W words, packed
__global__ __launch_bounds__(kBlock) void k_grp_gather(const unsigned long long *__restrict__ src, size_t stride,
                                                       const uint32_t *__restrict__ perm, uint32_t W, uint64_t total,
                                                       unsigned long long *__restrict__ dst) {
  const uint64_t words = total * W;
  for (uint64_t b0 = (uint64_t)blockIdx.x * kBlock; b0 < words; b0 += (uint64_t)gridDim.x * kBlock) {
    const uint64_t r0 = b0 / W;  // workgroup-uniform
    const uint32_t q = (uint32_t)(b0 - r0 * W) + threadIdx.x;  // < W + kBlock
    const uint64_t r = r0 + q / W;
    const uint32_t k = q % W;
    if (r < total) dst[r * W + k] = src[(size_t)perm[r] * stride + k];
  }
}

// keys / perm: the sorted pairs; flag[g]: problem g has a winner (mask holds its consensus bytes, in sorted order)
__global__ __launch_bounds__(kBlock) void k_grp_scatter(const uint32_t *__restrict__ keys,
                                                        const uint32_t *__restrict__ perm, uint32_t n,
                                                        uint32_t n_groups, const uint8_t *__restrict__ flag,
                                                        const uint8_t *__restrict__ mask,
                                                        uint8_t *__restrict__ consensus) {
  for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += (uint64_t)gridDim.x * kBlock) {
    const uint32_t g = keys[r];
    uint8_t v = 0;
    if (g < n_groups && flag[g]) v = mask[r];
    consensus[perm[r]] = v;
  }
}

// perm: the sorted record indices; packed: the round labels of the first total sorted positions (the grouped records,
// in packed order; unread where total is 0); labels: n entries in upload order
__global__ __launch_bounds__(kBlock) void k_grp_scatter_labels(const uint32_t *__restrict__ perm, uint32_t n,
                                                               uint32_t total, const int32_t *__restrict__ packed,
                                                               int32_t *__restrict__ labels) {
  for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += (uint64_t)gridDim.x * kBlock)
    labels[perm[r]] = r < total ? packed[r] : -1;
}

// its sibling for doubles (lsqr_assign_grouped's residuals): `fill` for the records in no problem
__global__ __launch_bounds__(kBlock) void k_grp_scatter_f64(const uint32_t *__restrict__ perm, uint32_t n,
                                                            uint32_t total, const double *__restrict__ packed,
                                                            double fill, double *__restrict__ out) {
  for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += (uint64_t)gridDim.x * kBlock)
    out[perm[r]] = r < total ? packed[r] : fill;
}

inline unsigned grp_grid(uint64_t lanes) {
  return (unsigned)std::min<uint64_t>(std::max<uint64_t>((lanes + kBlock - 1) / kBlock, 1), kGrpMaxGrid);
}

// The front half of both calls: the records grouped by label into B.d_data.  J: the job as the entry point has filled
// it from the context (stream, W, buf; n = n_groups).  data / stride / N: the context's records (stride in doubles).
// groups: a device pointer with on_device, else host.  offsets: the n_groups + 1 prefix sums of the group sizes, on
// the host after the call's one synchronisation.  The sorted pairs stay in B.d_grp_keys[1] / B.d_grp_vals[1].
inline int grouped_pack(ManyJob &J, const double *data, size_t stride, size_t N, const int32_t *groups, int on_device,
                        std::vector<uint64_t> &offsets) {
  ManyBufs &B = *J.buf;
  const size_t NG = J.n;
  const uint32_t n = (uint32_t)N, ng = (uint32_t)NG;
  const size_t W = (size_t)J.W;
  unsigned bits = 0;  // of the largest key, n_groups
  while (bits < 32 && (NG >> bits) != 0) bits++;

  size_t tmp_bytes = 0;
  MANYCHK(sort_pairs_u32(nullptr, &tmp_bytes, nullptr, nullptr, nullptr, nullptr, N, bits, J.stream));
  MANYCHK(many_grow(B.d_grp_keys[0], N));
  MANYCHK(many_grow(B.d_grp_keys[1], N));
  MANYCHK(many_grow(B.d_grp_vals[0], N));
  MANYCHK(many_grow(B.d_grp_vals[1], N));
  MANYCHK(many_grow(B.d_grp_tmp, std::max<size_t>(tmp_bytes, 1)));
  MANYCHK(many_grow(B.d_grp_off, NG + 1));
  MANYCHK(many_grow(B.d_grp_flag, NG));
  const size_t o_flag = sizeof(uint64_t) * (NG + 1);
  MANYCHK(many_grow_pinned(B.h_grp, o_flag + NG));  // (every earlier call ended in a synchronisation)
  const int32_t *d_groups = groups;
  if (!on_device) {
    MANYCHK(many_grow(B.d_grp_labels, N));
    MANYCHK(hipMemcpyAsync(B.d_grp_labels, groups, sizeof(int32_t) * N, hipMemcpyHostToDevice, J.stream));
    d_groups = B.d_grp_labels;
  }

  // keys, sort, offsets
  hipLaunchKernelGGL(k_grp_keys, dim3(grp_grid(N)), dim3(kBlock), 0, J.stream, d_groups, n, ng, B.d_grp_keys[0],
                     B.d_grp_vals[0]);
  MANYCHK(hipGetLastError());
  MANYCHK(sort_pairs_u32(B.d_grp_tmp, &tmp_bytes, B.d_grp_keys[0], B.d_grp_keys[1], B.d_grp_vals[0], B.d_grp_vals[1],
                         N, bits, J.stream));
  const uint32_t *keys = B.d_grp_keys[1], *perm = B.d_grp_vals[1];
  hipLaunchKernelGGL(k_grp_offsets, dim3(grp_grid(NG + 1)), dim3(kBlock), 0, J.stream, keys, n, ng, B.d_grp_off);
  MANYCHK(hipGetLastError());
  uint64_t *h_off = (uint64_t *)B.h_grp.get();
  MANYCHK(hipMemcpyAsync(h_off, B.d_grp_off, sizeof(uint64_t) * (NG + 1), hipMemcpyDeviceToHost, J.stream));
  MANYCHK(hipStreamSynchronize(J.stream));  // the one wait before the search: its rounds are planned from host offsets
  offsets.assign(h_off, h_off + NG + 1);
  if (offsets[0] != 0 || offsets[NG] > N) {
    snprintf(J.err, sizeof J.err, "group offsets out of range");
    return LSQR_ERR_HIP;
  }
  for (size_t g = 0; g < NG; g++)
    if (offsets[g + 1] < offsets[g]) {
      snprintf(J.err, sizeof J.err, "group offsets decrease at %zu", g);
      return LSQR_ERR_HIP;
    }
  const uint64_t NT = offsets[NG];

  // the packed copy
  if (NT) {
    MANYCHK(many_grow(B.d_data, (size_t)NT * W));
    hipLaunchKernelGGL(k_grp_gather, dim3(grp_grid(NT * W)), dim3(kBlock), 0, J.stream,
                       (const unsigned long long *)data, stride, perm, (uint32_t)W, NT,
                       (unsigned long long *)B.d_data.get());
    MANYCHK(hipGetLastError());
  }
  return LSQR_OK;
}

// lsqr_ransac_grouped.  J: the job of the batched search as the entry point has filled it from the context (stream,
// model, options, seeds, the host outputs; resident, no consensus_out, n = n_groups); its offsets are set here.
// data / stride / N, groups: as grouped_pack.  consensus_out (nullable): a device pointer with on_device, else host.
// offsets_out: nullable.  run(J): many_run<M> or many_dense_run<NR>.
template <class Run>
int grouped_run(ManyJob &J, const double *data, size_t stride, size_t N, const int32_t *groups, int on_device,
                uint8_t *consensus_out, uint64_t *offsets_out, Run &&run) {
  ManyBufs &B = *J.buf;
  const size_t NG = J.n;
  const uint32_t n = (uint32_t)N, ng = (uint32_t)NG;
  int st;
  std::vector<uint64_t> offsets;
  if ((st = grouped_pack(J, data, stride, N, groups, on_device, offsets)) != LSQR_OK) return st;
  const uint32_t *keys = B.d_grp_keys[1], *perm = B.d_grp_vals[1];
  // the batched search on the packed copy
  J.offsets = offsets.data();
  if ((st = run(J)) != LSQR_OK) return st;
  // (the job ended in a synchronisation: B.d_mask holds every winner's consensus bytes in packed order)
  if (offsets_out) memcpy(offsets_out, offsets.data(), sizeof(uint64_t) * (NG + 1));
  if (!consensus_out) return LSQR_OK;

  // a problem with a winner is one that took a finishing slot: many_end has set its fit's records in use, which
  // many_begin had zeroed for every problem.  (LSQR_OK, and the LSQR_EMPTY of a winner whose final fit failed: see
  // the head of this file.)
  uint8_t *h_flag = (uint8_t *)B.h_grp.get() + sizeof(uint64_t) * (NG + 1);
  for (size_t g = 0; g < NG; g++)
    h_flag[g] = J.infos[g].fit.n_used > 0 ? 1 : 0;
  MANYCHK(hipMemcpyAsync(B.d_grp_flag, h_flag, NG, hipMemcpyHostToDevice, J.stream));
  uint8_t *d_cons = consensus_out;
  if (!on_device) {
    MANYCHK(many_grow(B.d_grp_cons, N));
    d_cons = B.d_grp_cons;
  }
  hipLaunchKernelGGL(k_grp_scatter, dim3(grp_grid(N)), dim3(kBlock), 0, J.stream, keys, perm, n, ng, B.d_grp_flag,
                     B.d_mask, d_cons);
  MANYCHK(hipGetLastError());
  if (!on_device) MANYCHK(hipMemcpyAsync(consensus_out, d_cons, N, hipMemcpyDeviceToHost, J.stream));
  MANYCHK(hipStreamSynchronize(J.stream));  // the consensus is the caller's; h_grp is free again
  return LSQR_OK;
}

// lsqr_ransac_grouped_sequential.  J: filled from the context as for grouped_run (its seeds and outputs stay unset:
// many_seq_run's rounds have their own).  K / P, seeds ... n_models_out, run(S): many_seq_run's.  labels_out
// (nullable): N entries in upload order, a device pointer with on_device, else host.
template <class Run>
int grouped_seq_run(ManyJob &J, const double *data, size_t stride, size_t N, const int32_t *groups, int on_device,
                    int K, int P, const uint64_t *seeds, size_t max_models, uint64_t min_votes, double *params_out,
                    int32_t *labels_out, uint64_t *offsets_out, lsqr_ransac_info *infos, int32_t *status_out,
                    size_t *n_models_out, Run &&run) {
  ManyBufs &B = *J.buf;
  const size_t NG = J.n;
  int st;
  if (J.W < 2 || J.W > kSeqMaxD) {  // (many_seq_run's check, before any work)
    snprintf(J.err, sizeof J.err, "records of %d doubles (2 .. %d)", J.W, kSeqMaxD);
    return LSQR_ERR_INVALID;
  }
  std::vector<uint64_t> offsets;
  if ((st = grouped_pack(J, data, stride, N, groups, on_device, offsets)) != LSQR_OK) return st;
  const uint32_t *perm = B.d_grp_vals[1];
  const uint64_t NT = offsets[NG];
  // the rounds on the packed copy; with labels wanted they stay in B.d_seq_labels, in packed order
  J.offsets = offsets.data();
  if ((st = many_seq_run(J, K, P, seeds, max_models, min_votes, params_out, nullptr, labels_out != nullptr, infos,
                         status_out, n_models_out, run)) != LSQR_OK)
    return st;
  if (offsets_out) memcpy(offsets_out, offsets.data(), sizeof(uint64_t) * (NG + 1));
  if (labels_out) {
    int32_t *d_lab = labels_out;
    if (!on_device) {
      MANYCHK(many_grow(B.d_grp_lab, N));
      d_lab = B.d_grp_lab;
    }
    hipLaunchKernelGGL(k_grp_scatter_labels, dim3(grp_grid(N)), dim3(kBlock), 0, J.stream, perm, (uint32_t)N,
                       (uint32_t)NT, NT ? B.d_seq_labels : nullptr, d_lab);
    MANYCHK(hipGetLastError());
    if (!on_device) MANYCHK(hipMemcpyAsync(labels_out, d_lab, sizeof(int32_t) * N, hipMemcpyDeviceToHost, J.stream));
  }
  MANYCHK(hipStreamSynchronize(J.stream));  // the labels are the caller's; the last partition has read h_seq
  return LSQR_OK;
}
#endif

}  // namespace lsqr
