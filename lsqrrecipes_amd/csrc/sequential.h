// sequential.h -- the device side of lsqr_ransac_sequential: between two rounds the records no round has claimed yet
// are copied, in order and tightly packed, into a scratch buffer of the context, so that the next round's search runs
// on them exactly as on a fresh upload -- without the records leaving the device.
//
// A stable partition of the current record buffer by the consensus mask of the round that just ended (d_mask, one
// byte per record in buffer order), as three launches on the context's stream:
//
//   k_seq_count   one workgroup per chunk of kSeqChunk records: its survivors (mask byte 0)
//   k_seq_scan    ONE workgroup: exclusive prefix sum of the chunk counts, in place (2442 counts at 10 M records)
//   k_seq_write   one workgroup per chunk, tile by tile (kBlock records): wave ballots give every survivor its slot
//                 in the tile, the survivors are packed in LDS -- element e of the tile's D-double records is read by
//                 lane e, so that neighbouring lanes read neighbouring doubles whatever the input stride -- and leave
//                 as ONE contiguous run of doubles at the chunk's offset.  The survivor's index in the caller's
//                 upload travels in a parallel uint32 map (identity while the source is the upload itself); a claimed
//                 record writes labels[its upload index] = round.
//   k_seq_label   the last round, which nothing follows: the labels alone.
//
// The tile body of k_seq_write is seq_write_tile, shared with the segmented partition of lsqr_ransac_many_sequential
// (many_sequential.h: k_mseq_write).
//
// No workgroup waits for another one: the order between the three steps is the stream's.  The host needs no count back:
// the survivors are n - best_votes, and finish_ransac has checked best_votes against the mask.  k_seq_write clamps its
// stores to that count all the same, so a mask that disagreed could not write past the destination.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace lsqr {

constexpr uint32_t kSeqChunk = 16 * kBlock;  // records per workgroup of the count and the write
constexpr int kSeqMaxD = 18;                 // the widest record (lsqr_record_doubles: 2 .. 18)

inline uint32_t seq_chunks(uint64_t n) { return (uint32_t)((n + kSeqChunk - 1) / kSeqChunk); }

#if defined(__HIPCC__)
__global__ __launch_bounds__(kBlock) void k_seq_count(const uint8_t *__restrict__ mask, uint32_t n,
                                                      uint32_t *__restrict__ counts) {
  __shared__ uint32_t s_c[kBlock / 64];
  const uint64_t c0 = (uint64_t)blockIdx.x * kSeqChunk;
  const uint32_t c1 = (uint32_t)(c0 + kSeqChunk < n ? c0 + kSeqChunk : n);
  uint32_t c = 0;
  for (uint64_t i = c0 + threadIdx.x; i < c1; i += kBlock) c += mask[i] == 0 ? 1u : 0u;
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
  if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int w = 0; w < kBlock / 64; w++) s += s_c[w];
    counts[blockIdx.x] = s;
  }
}

// counts[i] -> the sum of counts[0 .. i), one workgroup walking the array in tiles of kBlock with a running carry
__global__ __launch_bounds__(kBlock) void k_seq_scan(uint32_t *__restrict__ counts, uint32_t n_chunks) {
  __shared__ uint32_t s_w[kBlock / 64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t carry = 0;
  for (uint32_t t0 = 0; t0 < n_chunks; t0 += kBlock) {
    const uint32_t i = t0 + threadIdx.x;
    const uint32_t v = i < n_chunks ? counts[i] : 0u;
    uint32_t inc = v;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t up = __shfl_up(inc, o);
      if (lane >= o) inc += up;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t off = 0, tot = 0;
    for (int w = 0; w < kBlock / 64; w++) {
      if (w < wave) off += s_w[w];
      tot += s_w[w];
    }
    if (i < n_chunks) counts[i] = carry + off + inc - v;
    carry += tot;
    __syncthreads();  // s_w is rewritten by the next tile
  }
}

// LDS of one workgroup of the write kernels (k_seq_write here, k_mseq_write in many_sequential.h); buf: the dynamic
// part, kBlock * D doubles
struct SeqTileLds {
  uint32_t slot[kBlock], orig[kBlock], w[kBlock / 64];
};

// One tile of the stable partition, by a whole workgroup of kBlock lanes: records [t0, min(t0 + kBlock, c1)) of `data`
// (D doubles each, `stride` doubles apart; mask and orig_in -- nullable: identity -- indexed like the records).  The
// survivors (mask byte 0) leave as one contiguous run at slot `base` of out / orig_out, clamped to slot `lim`; a
// claimed record writes labels[its upload index] = round (labels nullable, n_labels entries).  magic: ceil(2^32 / D).
// -> the tile's survivors.  Ends in a barrier: the LDS may be rewritten at once.
__device__ __forceinline__ uint32_t seq_write_tile(const double *__restrict__ data, size_t stride, uint64_t t0,
                                                   uint64_t c1, uint32_t uD, uint32_t magic,
                                                   const uint8_t *__restrict__ mask,
                                                   const uint32_t *__restrict__ orig_in, int32_t round,
                                                   int32_t *__restrict__ labels, uint32_t n_labels, uint32_t base,
                                                   uint32_t lim, double *__restrict__ out,
                                                   uint32_t *__restrict__ orig_out, double *s_buf, SeqTileLds &s) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t i = t0 + threadIdx.x;
  const bool in_range = i < c1;
  const bool keep = in_range && mask[i] == 0;
  const uint32_t o = in_range ? (orig_in ? orig_in[i] : (uint32_t)i) : 0u;
  if (in_range && !keep && labels && o < n_labels) labels[o] = round;
  const uint64_t bal = __ballot(keep);
  const uint32_t below = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) s.w[wave] = (uint32_t)__popcll(bal);
  __syncthreads();
  uint32_t off = 0, tot = 0;
  for (int w = 0; w < kBlock / 64; w++) {
    if (w < wave) off += s.w[w];
    tot += s.w[w];
  }
  s.slot[threadIdx.x] = keep ? off + below : 0xFFFFFFFFu;
  if (keep) s.orig[off + below] = o;
  __syncthreads();
  const uint32_t cnt = (uint32_t)(c1 - t0 < (uint64_t)kBlock ? c1 - t0 : (uint64_t)kBlock);
  for (uint32_t e = threadIdx.x; e < cnt * uD; e += kBlock) {
    const uint32_t rec = __umulhi(e, magic), k = e - rec * uD;
    const uint32_t sl = s.slot[rec];
    if (sl != 0xFFFFFFFFu) s_buf[sl * uD + k] = data[(t0 + rec) * stride + k];
  }
  __syncthreads();
  const uint32_t room = base < lim ? lim - base : 0u;
  const uint32_t run = tot < room ? tot : room;
  double *dst = out + (uint64_t)base * uD;
  for (uint32_t e = threadIdx.x; e < run * uD; e += kBlock) dst[e] = s_buf[e];
  if (threadIdx.x < run) orig_out[base + threadIdx.x] = s.orig[threadIdx.x];
  __syncthreads();  // slot, orig, w and s_buf are rewritten by the next tile
  return tot;
}

// data: n records of D doubles, `stride` doubles apart; orig_in (nullable: identity): their indices in the caller's
// upload; offsets: k_seq_scan's result; out / orig_out: room for n_out records; labels (nullable): n_labels entries.
// Dynamic LDS: kBlock * D doubles.
__global__ __launch_bounds__(kBlock) void k_seq_write(const double *__restrict__ data, size_t stride, uint32_t n, int D,
                                                      const uint8_t *__restrict__ mask,
                                                      const uint32_t *__restrict__ orig_in,
                                                      const uint32_t *__restrict__ offsets, uint32_t n_out,
                                                      int32_t round, double *__restrict__ out,
                                                      uint32_t *__restrict__ orig_out, int32_t *__restrict__ labels,
                                                      uint32_t n_labels) {
  extern __shared__ double s_buf[];
  __shared__ SeqTileLds s;
  const uint64_t c0 = (uint64_t)blockIdx.x * kSeqChunk;
  const uint32_t c1 = (uint32_t)(c0 + kSeqChunk < n ? c0 + kSeqChunk : n);
  const uint32_t uD = (uint32_t)D;
  const uint32_t magic = 0xFFFFFFFFu / uD + 1u;  // ceil(2^32 / D): __umulhi(e, magic) == e / D for e < 2^32 / D
  uint32_t base = offsets[blockIdx.x];
  for (uint64_t t0 = c0; t0 < c1; t0 += kBlock)
    base += seq_write_tile(data, stride, t0, c1, uD, magic, mask, orig_in, round, labels, n_labels, base, n_out, out,
                           orig_out, s_buf, s);
}

__global__ __launch_bounds__(kBlock) void k_seq_label(const uint8_t *__restrict__ mask, uint32_t n,
                                                      const uint32_t *__restrict__ orig_in, int32_t round,
                                                      int32_t *__restrict__ labels, uint32_t n_labels) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n || mask[i] == 0) return;
  const uint32_t o = orig_in ? orig_in[i] : (uint32_t)i;
  if (o < n_labels) labels[o] = round;
}

// The partition of `n` records into out / orig_out (room for n_out = the survivors), three launches on `stream`.
// counts: seq_chunks(n) entries.
inline hipError_t seq_partition(hipStream_t stream, const double *data, size_t stride, uint32_t n, int D,
                                const uint8_t *mask, const uint32_t *orig_in, uint32_t *counts, uint32_t n_out,
                                int32_t round, double *out, uint32_t *orig_out, int32_t *labels, uint32_t n_labels) {
  if (D < 2 || D > kSeqMaxD) return hipErrorInvalidValue;  // (D = 1 would wrap k_seq_write's reciprocal)
  const uint32_t chunks = seq_chunks(n);
  if (chunks == 0) return hipSuccess;
  hipLaunchKernelGGL(k_seq_count, dim3(chunks), dim3(kBlock), 0, stream, mask, n, counts);
  hipLaunchKernelGGL(k_seq_scan, dim3(1), dim3(kBlock), 0, stream, counts, chunks);
  hipLaunchKernelGGL(k_seq_write, dim3(chunks), dim3(kBlock), sizeof(double) * kBlock * (size_t)D, stream, data, stride,
                     n, D, mask, orig_in, counts, n_out, round, out, orig_out, labels, n_labels);
  return hipGetLastError();
}

inline hipError_t seq_label(hipStream_t stream, const uint8_t *mask, uint32_t n, const uint32_t *orig_in, int32_t round,
                            int32_t *labels, uint32_t n_labels) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_seq_label, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, mask, n, orig_in, round,
                     labels, n_labels);
  return hipGetLastError();
}
#endif  // __HIPCC__

}  // namespace lsqr
