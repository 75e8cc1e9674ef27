// many_sequential.h -- lsqr_ransac_many_sequential: sequential RANSAC (lsqr_ransac_sequential: find a model, take its
// consensus set out, search what is left) over many independent problems in one call.  The records go up once
// (many_upload); round r is ONE batched RANSAC job -- the unchanged many_run / many_dense_run, told that its records
// are resident -- over the problems still going, on their unclaimed records; between two rounds a segmented stable
// partition packs those records, problem after problem, into the other of two device buffers.
//
//   k_mseq_count   one workgroup per part (<= kSeqChunk records of one problem that goes on): its survivors
//   k_mseq_write   one workgroup per part.  A part of a problem that goes on: its offset in the problem is the sum of
//                  the counts of the problem's parts before it (read by the whole workgroup; no scan launch: most
//                  problems are one part), then tile by tile seq_write_tile (sequential.h: lane = element on the load
//                  side, survivors packed in LDS, one contiguous run out at problem base + offset, upload indices
//                  beside them, labels[upload index] = round for the claimed records), every store clamped to the
//                  problem's end in the destination.  A part of a problem whose accepted round nothing follows:
//                  the labels alone.
//
// A problem that stopped has no part: its records are neither read nor copied, and the next round's buffer holds the
// continuing problems only.  The host needs nothing back for the partition: the survivors of problem j are n_j -
// best_votes_j, which many_fetch_finish has checked against the mask, so every problem's base in the destination is a
// host-side prefix sum.  The consensus bytes stay on the device (the rounds' jobs have no consensus_out).  No workgroup
// waits on another: the order between count, write and the next round is the stream's.
//
// Why a round equals lsqr_ransac_many on the survivors: the sub-job's records are exactly the unclaimed records of
// its problems, in their original order, tightly packed, with offsets of its own -- the input lsqr_ransac_many would
// get from a host that had compacted them -- and its kernels and host replay are many_run's.  Independence is
// lsqr_ransac_many's: which problems share a round's job does not enter any problem's result.
//
// "Upload indices" in this file are positions in the round-0 buffer: the caller's packed host records for
// lsqr_ransac_many_sequential, the label-sorted packed copy for lsqr_ransac_grouped_sequential (grouped.h), which maps
// the labels from there to its own record order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include "many.h"
#include "many_dense.h"
#include "many_exhaustive.h"
#include "sequential.h"

namespace lsqr {

struct ManySeqPart {  // partition work item: records [r0, r1) of the current buffer, all of one problem
  uint64_t r0, r1;
  uint32_t first;  // the problem's first part
  uint32_t base;   // copy: the problem's first slot in the destination
  uint32_t lim;    // copy: one past its last (base + survivors)
  int32_t round;   // the round that claimed the records whose mask byte is set
  uint32_t copy;   // 1: the problem goes on to round + 1; 0: labels only
  uint32_t pad;
};

#if defined(__HIPCC__)
__global__ __launch_bounds__(kBlock) void k_mseq_count(const ManySeqPart *__restrict__ parts,
                                                       const uint8_t *__restrict__ mask,
                                                       uint32_t *__restrict__ counts) {
  __shared__ uint32_t s_c[kBlock / 64];
  const ManySeqPart pt = parts[blockIdx.x];
  uint32_t c = 0;
  if (pt.copy)
    for (uint64_t i = pt.r0 + threadIdx.x; i < pt.r1; i += kBlock) c += mask[i] == 0 ? 1u : 0u;
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
  if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int w = 0; w < kBlock / 64; w++) s += s_c[w];
    counts[blockIdx.x] = s;
  }
}

// data: the current buffer, records of D doubles, packed; mask: the round's consensus bytes in buffer order; orig_in
// (nullable: identity, the buffer is the upload): the records' upload indices; out / orig_out: the destination, every
// problem's run clamped to [base, lim); labels (nullable): n_labels entries.  Dynamic LDS: kBlock * D doubles.
__global__ __launch_bounds__(kBlock) void k_mseq_write(const double *__restrict__ data, int D,
                                                       const ManySeqPart *__restrict__ parts,
                                                       const uint8_t *__restrict__ mask,
                                                       const uint32_t *__restrict__ orig_in,
                                                       const uint32_t *__restrict__ counts, double *__restrict__ out,
                                                       uint32_t *__restrict__ orig_out, int32_t *__restrict__ labels,
                                                       uint32_t n_labels) {
  extern __shared__ double s_buf[];
  __shared__ SeqTileLds s;
  __shared__ uint32_t s_pre[kBlock / 64];
  const ManySeqPart pt = parts[blockIdx.x];
  if (!pt.copy) {  // workgroup-uniform
    if (!labels) return;
    for (uint64_t i = pt.r0 + threadIdx.x; i < pt.r1; i += kBlock) {
      if (mask[i] == 0) continue;
      const uint32_t o = orig_in ? orig_in[i] : (uint32_t)i;
      if (o < n_labels) labels[o] = pt.round;
    }
    return;
  }
  uint32_t pre = 0;  // survivors of the problem's parts before this one
  for (uint32_t q = pt.first + threadIdx.x; q < blockIdx.x; q += kBlock) pre += counts[q];
  for (int o = 32; o > 0; o >>= 1) pre += __shfl_down(pre, o);
  if ((threadIdx.x & 63) == 0) s_pre[threadIdx.x >> 6] = pre;
  __syncthreads();
  uint32_t base = pt.base;
  for (int w = 0; w < kBlock / 64; w++) base += s_pre[w];
  const uint32_t uD = (uint32_t)D;
  const uint32_t magic = 0xFFFFFFFFu / uD + 1u;  // ceil(2^32 / D), as k_seq_write
  for (uint64_t t0 = pt.r0; t0 < pt.r1; t0 += kBlock)
    base += seq_write_tile(data, (size_t)uD, t0, pt.r1, uD, magic, mask, orig_in, pt.round, labels, n_labels, base,
                           pt.lim, out, orig_out, s_buf, s);
}

// One problem's place in the call
struct ManySeqProb {
  uint64_t n = 0;  // its unclaimed records
  bool going = false;
};

// The call.  J: the job many_call has filled (host records, the caller's offsets; its seeds / outputs are unused: the
// rounds' jobs have their own), or grouped.h's with J.resident set: nothing is uploaded, and round 0 reads the packed
// records that lie in B.d_data.  K / P: the model's minimal subset and parameter count; seeds [j * max_models + r];
// params_out, infos, status_out: rows [j][r]; labels_out nullable, host; keep_labels: the labels are made and left
// on the device -- B.d_seq_labels, offsets[n] entries in the order of the round-0 buffer, -1-filled (unmade where
// offsets[n] is 0) -- and the call ends without a synchronisation: the caller's work follows on the stream, and the
// caller waits.  run(sub): many_run<M> or many_dense_run<NR>.
template <class Run>
int many_seq_run(ManyJob &J, int K, int P, const uint64_t *seeds, size_t max_models, uint64_t min_votes,
                 double *params_out, int32_t *labels_out, bool keep_labels, lsqr_ransac_info *infos,
                 int32_t *status_out, size_t *n_models_out, Run &&run) {
  ManyBufs &B = *J.buf;
  const size_t N = J.n, MM = max_models;
  const uint64_t NT = J.offsets[N];
  const int W = J.W;
  int st;
  // (the upload indices and the destination slots are 32-bit; D = 1 would wrap seq_write_tile's reciprocal)
  if (NT > 0xFFFFFFF0ull) {
    snprintf(J.err, sizeof J.err, "more than 2^32 - 16 records in all");
    return LSQR_ERR_INVALID;
  }
  if (W < 2 || W > kSeqMaxD) {
    snprintf(J.err, sizeof J.err, "records of %d doubles (2 .. %d)", W, kSeqMaxD);
    return LSQR_ERR_INVALID;
  }
  for (size_t e = 0; e < N * MM; e++) status_out[e] = LSQR_ERR_STATE;  // round not run
  memset(infos, 0, sizeof(lsqr_ransac_info) * N * MM);
  for (size_t j = 0; j < N; j++) n_models_out[j] = 0;

  if ((st = many_upload(J)) != LSQR_OK) return st;
  int32_t *d_labels = nullptr;
  if ((labels_out || keep_labels) && NT) {
    MANYCHK(many_grow(B.d_seq_labels, (size_t)NT));
    MANYCHK(hipMemsetAsync(B.d_seq_labels, 0xFF, sizeof(int32_t) * NT, J.stream));  // -1
    d_labels = B.d_seq_labels;
  }

  std::vector<ManySeqProb> pr(N);
  for (size_t j = 0; j < N; j++) {
    pr[j].n = J.offsets[j + 1] - J.offsets[j];
    pr[j].going = pr[j].n >= (uint64_t)K;
  }
  // round 0 runs on the upload itself, under the caller's offsets: the problems too small to run lie between the
  // others and are many_begin's LSQR_ERR_INVALID, which stays in the scratch outputs; a later round's job holds the
  // problems still going alone
  std::vector<uint32_t> sub_prob;
  std::vector<uint64_t> sub_off, sub_seeds;
  std::vector<double> sub_params;
  std::vector<lsqr_ransac_info> sub_infos;
  std::vector<int32_t> sub_status;
  std::vector<ManySeqPart> parts;
  const uint32_t *orig = nullptr;  // upload indices of the current buffer's records (null: it is the upload)
  int cur = -1;
  for (size_t r = 0; r < MM; r++) {
    sub_prob.clear();
    sub_off.assign(1, 0);
    for (size_t j = 0; j < N; j++) {
      if (r > 0 && !pr[j].going) continue;
      sub_prob.push_back((uint32_t)j);
      sub_off.push_back(r == 0 ? J.offsets[j + 1] : sub_off.back() + pr[j].n);
    }
    size_t going = 0;
    for (size_t j = 0; j < N; j++) going += pr[j].going ? 1 : 0;
    if (going == 0) break;
    const size_t NS = sub_prob.size();
    sub_seeds.resize(NS);
    for (size_t q = 0; q < NS; q++) sub_seeds[q] = seeds[(size_t)sub_prob[q] * MM + r];
    sub_params.assign(NS * P, 0.0);
    sub_infos.assign(NS, lsqr_ransac_info());
    sub_status.assign(NS, LSQR_ERR_STATE);
    ManyJob S;
    S.stream = J.stream;
    S.cfg = J.cfg;
    S.mc = J.mc;
    S.resident = true;
    S.offsets = sub_off.data();
    S.n = NS;
    S.W = W;
    S.p = J.p;
    S.seeds = sub_seeds.data();
    S.params_out = sub_params.data();
    S.infos = sub_infos.data();
    S.status_out = sub_status.data();
    S.max_iter = J.max_iter;
    S.round_cap = J.round_cap;
    S.lm = J.lm;
    S.lm_n = J.lm_n;
    S.lm_maxfev = J.lm_maxfev;
    S.lm_ftol = J.lm_ftol;
    S.lm_xtol = J.lm_xtol;
    S.lm_gtol = J.lm_gtol;
    S.dense_fast = J.dense_fast;
    S.dense_dd = J.dense_dd;
    S.buf = J.buf;
    if ((st = run(S)) != LSQR_OK) {
      memcpy(J.err, S.err, sizeof J.err);
      return st;
    }
    // (the job ended in a synchronisation: B.d_mask holds every winner's consensus bytes in buffer order)

    // the rounds' rows, who goes on, and the partition's parts
    parts.clear();
    uint64_t next_total = 0;
    for (size_t q = 0; q < NS; q++) {
      const uint32_t j = sub_prob[q];
      ManySeqProb &pj = pr[j];
      if (!pj.going) continue;  // (round 0: too small to run)
      const size_t row = (size_t)j * MM + r;
      infos[row] = sub_infos[q];
      status_out[row] = sub_status[q];
      if (sub_status[q] == LSQR_OK) memcpy(params_out + row * P, &sub_params[q * P], sizeof(double) * P);
      pj.going = false;
      const uint64_t votes = sub_infos[q].best_votes;
      if (sub_status[q] != LSQR_OK || votes < std::max<uint64_t>(min_votes, 1)) continue;  // rejected: claims nothing
      n_models_out[j] = r + 1;
      const uint64_t survivors = pj.n - votes;
      const bool copy = r + 1 < MM && survivors >= (uint64_t)K;
      if (copy || d_labels) {
        const uint32_t first = (uint32_t)parts.size();
        const uint64_t r0 = sub_off[q], r1 = sub_off[q + 1];
        for (uint64_t a = r0; a < r1; a += kSeqChunk)
          parts.push_back(ManySeqPart{a, std::min<uint64_t>(r1, a + kSeqChunk), first, (uint32_t)next_total,
                                      (uint32_t)(next_total + (copy ? survivors : 0)), (int32_t)r, copy ? 1u : 0u,
                                      0u});
      }
      if (copy) {
        pj.going = true;
        pj.n = survivors;
        next_total += survivors;
      }
    }
    if (parts.empty()) break;
    const int dst = cur == 0 ? 1 : 0;
    const size_t b_parts = sizeof(ManySeqPart) * parts.size();
    MANYCHK(many_grow_pinned(B.h_seq, b_parts));  // (the round's job ended in a synchronisation)
    memcpy(B.h_seq, parts.data(), b_parts);
    MANYCHK(many_grow(B.d_seq_parts, b_parts));
    MANYCHK(many_grow(B.d_seq_counts, parts.size()));
    MANYCHK(many_grow(B.d_seq_rec, (size_t)std::max<uint64_t>(next_total, 1) * W));
    MANYCHK(many_grow(B.d_seq_orig[dst], (size_t)std::max<uint64_t>(next_total, 1)));
    MANYCHK(hipMemcpyAsync(B.d_seq_parts, B.h_seq, b_parts, hipMemcpyHostToDevice, J.stream));
    const ManySeqPart *d_parts = (const ManySeqPart *)B.d_seq_parts.get();
    if (next_total) {
      hipLaunchKernelGGL(k_mseq_count, dim3((unsigned)parts.size()), dim3(kBlock), 0, J.stream, d_parts, B.d_mask,
                         B.d_seq_counts);
      MANYCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_mseq_write, dim3((unsigned)parts.size()), dim3(kBlock), sizeof(double) * kBlock * (size_t)W,
                       J.stream, B.d_data, W, d_parts, B.d_mask, orig, B.d_seq_counts, B.d_seq_rec, B.d_seq_orig[dst],
                       d_labels, (uint32_t)NT);
    MANYCHK(hipGetLastError());
    if (next_total == 0) break;  // labels only: no round follows
    std::swap(B.d_data, B.d_seq_rec);  // the next round's job reads the survivors as its upload
    orig = B.d_seq_orig[dst];
    cur = dst;
  }
  if (keep_labels) return LSQR_OK;
  if (d_labels) MANYCHK(hipMemcpyAsync(labels_out, d_labels, sizeof(int32_t) * NT, hipMemcpyDeviceToHost, J.stream));
  MANYCHK(hipStreamSynchronize(J.stream));  // the labels; the last partition has read h_seq
  return LSQR_OK;
}
#endif

}  // namespace lsqr

