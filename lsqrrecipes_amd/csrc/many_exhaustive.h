// many_exhaustive.h -- lsqr_ransac_many_exhaustive: many independent RANSAC<T,S>::compute() problems of the EXHAUSTIVE
// overload (RANSAC.hxx:150-249: every k-subset in lexicographic order, first maximum wins) in one call.  Hypothesis
// `rank` of a problem is comb_unrank's subset (comb.h), so the whole schedule is known before the first launch and the
// first-max rule (RANSAC.hxx:245, strict '>') is a max-reduction of (votes, smallest rank): the host reads nothing
// back until every problem has its winner.  The finish is lsqr_ransac_many's (many.h: many_finish).
//
// Fused path, a problem of N <= kManyStage records and C(N,k) <= kManyExFusedRanks:
//   k_many_ex_small<M>     one workgroup per problem: the records and the binomials C(c, j), c < N, j <= K, staged in
//                          LDS once; ranks 256 at a time, lane = hypothesis: unrank by table, gather from LDS,
//                          M::estimate / M::prepare, scan of all N records from LDS (same address in every lane); a
//                          workgroup max of the packed key carries the running first maximum over the chunks; the
//                          winner's row, votes and rank are written once
// General path, every other problem, in rounds of at most round_cap hypotheses (a problem with more subsets is cut into
// consecutive rank ranges, at most one per round, in increasing rank order):
//   k_many_ex_estimate<M>  k_many_sample_estimate with comb_unrank in place of ctr_subset
//   k_many_scan<M>         (many.h, unchanged)
//   k_many_ex_best         one workgroup per item: max of (votes << 32) | (0xFFFFFFFF - row) over the item's valid rows;
//                          where the votes exceed the problem's running best, the votes, the rank and the row are stored.
//                          Stream order serialises a problem's rounds, so that earlier ranks win ties.
// Both paths unrank the same subset (comb_unrank / comb_unrank_tab: one bisection over the same binomials) and call
// many_ex_hypothesis<M> and the scan's M::load / M::agree on the same values: the rows, the votes and
// so everything after them are bit-identical whichever path a problem takes.
#pragma once
#include "comb.h"
#include "many.h"

namespace lsqr {

// The fused path's cap on ranks per problem: 256 chunks of kManyBlock.  An estimate, not a tuned value (DESIGN.md
// section 11.4 has the arithmetic and the timings of both paths): a lane's chunk is K table bisections, one estimate
// and N agree, some 2 000 instructions at N = 40, of which a wave issues one fp64 instruction per four cycles -- a
// few microseconds a chunk, five times that at N = 256 -- so a workgroup is held for milliseconds at most.  Beyond
// that a problem's hypotheses are better spread over the device by the general path's tiles (C(256,9) would pin one
// workgroup for longer than the device lives).  Every shape the call was written for lies below it: C(12,2) = 66,
// C(20,3) = 1140, C(40,3) = 9880, C(64,3) = 41664, C(256,2) = 32640.
constexpr uint64_t kManyExFusedRanks = 65536;

struct ManyExItem {   // general path: ranks [first, first + H) of problem prob = rows [h0, h0 + H) of the round
  uint64_t rec, n, first;
  uint32_t h0, H, prob, pad;
};
struct ManyExSmall {  // fused path: one problem
  uint64_t rec, count;  // its first record in the packed upload; C(n, K)
  uint32_t n, prob;
};

#if defined(__HIPCC__)
// the hypothesis of the exhaustive search on subset idx of the records at rec (w doubles each; global memory or LDS):
// the gathered records, and from there on as k_estimate -> its scan row sp; false: degenerate
template <class M>
__device__ __forceinline__ bool many_ex_hypothesis(const double *rec, int w, const uint32_t *idx,
                                                   const ModelConsts &mc, double *sp) {
  double r[M::K][M::ND];
  for (int l = 0; l < M::K; l++)
    for (int j = 0; j < M::ND; j++) r[l][j] = rec[(size_t)idx[l] * w + j];
  double par[M::P];
  const bool ok = M::estimate(r, mc, par);
  const double qnan = __builtin_nan("");
  for (int j = 0; j < M::P; j++) sp[j] = ok ? par[j] : qnan;
  for (int j = M::P; j < M::SP; j++) sp[j] = 0.0;
  M::prepare(sp, mc);
  return ok;
}

// the largest key of the workgroup (kManyBlock lanes), in every lane; s_key: one slot per wave.  The caller separates
// two calls by a __syncthreads.
__device__ __forceinline__ unsigned long long many_ex_block_max(unsigned long long key, unsigned long long *s_key) {
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o);
    key = other > key ? other : key;
  }
  if ((threadIdx.x & 63) == 0) s_key[threadIdx.x >> 6] = key;
  __syncthreads();
  unsigned long long m = s_key[0];
  for (int w = 1; w < kManyBlock / 64; w++) m = s_key[w] > m ? s_key[w] : m;
  return m;
}

template <class M>
__global__ __launch_bounds__(kBlock) void k_many_ex_estimate(const double *__restrict__ data, int W,
                                                             const ManyExItem *__restrict__ items, int n_items,
                                                             uint32_t H, ModelConsts mc,
                                                             double *__restrict__ hparams,
                                                             uint8_t *__restrict__ valid) {
  const uint32_t h = blockIdx.x * kBlock + threadIdx.x;
  if (h >= H) return;
  int lo = 0, hi = n_items - 1;  // the last item with h0 <= h
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (items[mid].h0 <= h) lo = mid;
    else hi = mid - 1;
  }
  const ManyExItem it = items[lo];
  const int w = many_width<M>(W);
  uint32_t idx[M::K];
  comb_unrank(it.n, M::K, it.first + (h - it.h0), idx);
  double sp[M::SP];
  const bool ok = many_ex_hypothesis<M>(data + it.rec * w, w, idx, mc, sp);
  for (int j = 0; j < M::SP; j++) hparams[(size_t)h * M::SP + j] = sp[j];
  valid[h] = ok ? 1 : 0;
}

// exbest: {votes, rank} per problem, zeroed before the first round
__global__ __launch_bounds__(kManyBlock) void k_many_ex_best(const ManyExItem *__restrict__ items,
                                                             const uint32_t *__restrict__ votes,
                                                             const uint8_t *__restrict__ valid, int sp,
                                                             const double *__restrict__ hparams,
                                                             double *__restrict__ best,
                                                             unsigned long long *__restrict__ exbest) {
  __shared__ unsigned long long s_key[kManyBlock / 64];
  const ManyExItem it = items[blockIdx.x];
  const unsigned long long cur = exbest[2 * (size_t)it.prob];  // (read by every lane before lane 0 may write it)
  unsigned long long key = 0;
  for (uint32_t row = threadIdx.x; row < it.H; row += kManyBlock)
    if (valid[it.h0 + row]) {
      const unsigned long long k = ((unsigned long long)votes[it.h0 + row] << 32) | (0xFFFFFFFFu - row);
      key = k > key ? k : key;
    }
  key = many_ex_block_max(key, s_key);
  const uint32_t v = (uint32_t)(key >> 32), row = 0xFFFFFFFFu - (uint32_t)key;
  if (key == 0 || v <= (uint32_t)cur) return;  // RANSAC.hxx:245: strictly more votes than every earlier rank
  for (int j = threadIdx.x; j < sp; j += kManyBlock)
    best[(size_t)it.prob * sp + j] = hparams[(size_t)(it.h0 + row) * sp + j];
  if (threadIdx.x == 0) {
    exbest[2 * (size_t)it.prob] = v;
    exbest[2 * (size_t)it.prob + 1] = it.first + row;
  }
}

template <class M>
__global__ __launch_bounds__(kManyBlock) void k_many_ex_small(const double *__restrict__ data, int W,
                                                              const ManyExSmall *__restrict__ probs, ModelConsts mc,
                                                              double *__restrict__ best,
                                                              unsigned long long *__restrict__ exbest) {
  __shared__ double s_rec[kManyStage * many_wmax<M>()];
  static_assert(M::K <= 10, "the table's entries fit in 64 bits");
  __shared__ uint64_t s_tab[kManyStage * M::K];  // C(c, j), c < n, 1 <= j <= K (comb_unrank_tab)
  __shared__ double s_row[M::SP];
  __shared__ unsigned long long s_key[kManyBlock / 64];
  const int w = many_width<M>(W);
  const ManyExSmall q = probs[blockIdx.x];  // q.n <= kManyStage
  const uint32_t lane = threadIdx.x;
  const double *src = data + q.rec * w;
  for (uint32_t t = lane; t < q.n * w; t += kManyBlock) s_rec[t] = src[t];
  for (uint32_t t = lane; t < q.n * M::K; t += kManyBlock) {
    uint64_t c = 0;
    comb_count(t / M::K, (int)(t % M::K) + 1, &c);  // (fits: c < 256 and j <= 10, at most C(255, 10) < 2^58)
    s_tab[t] = c;
  }
  __syncthreads();
  uint32_t run_votes = 0;
  uint64_t run_rank = 0;
  for (uint64_t base = 0; base < q.count; base += kManyBlock) {
    double sp[M::SP];
    bool ok = base + lane < q.count;
    if (ok) {
      uint32_t idx[M::K];
      comb_unrank_tab(q.n, M::K, base + lane, q.count, s_tab, idx);
      ok = many_ex_hypothesis<M>(s_rec, w, idx, mc, sp);
    }
    uint32_t c = 0;
    if (ok) {
      for (uint32_t i = 0; i < q.n; i++) {
        double x[M::REC];
        M::load(s_rec + i * w, mc, x);  // same address in every lane: broadcast
        c += M::agree(sp, x, mc) ? 1u : 0u;
      }
    }
    const unsigned long long key =
        many_ex_block_max(ok ? ((unsigned long long)c << 32) | (0xFFFFFFFFu - lane) : 0ull, s_key);
    const uint32_t v = (uint32_t)(key >> 32), wl = 0xFFFFFFFFu - (uint32_t)key;
    if (key != 0 && v > run_votes) {  // uniform: RANSAC.hxx:245 over the chunks, the smallest rank within one
      run_votes = v;
      run_rank = base + wl;
      if (lane == wl)
        for (int j = 0; j < M::SP; j++) s_row[j] = sp[j];
    }
    __syncthreads();  // s_key has been read, s_row is written
  }
  if (run_votes == 0) return;  // exbest stays {0, 0}
  for (int j = lane; j < M::SP; j += kManyBlock) best[(size_t)q.prob * M::SP + j] = s_row[j];
  if (lane == 0) {
    exbest[2 * (size_t)q.prob] = run_votes;
    exbest[2 * (size_t)q.prob + 1] = run_rank;
  }
}

// ---- host side -------------------------------------------------------------------------------------------------
// pinned staging buffer `slot` of the call, at least `bytes` long, once the copies that last read it are done
inline int many_ex_stage(ManyJob &J, int slot, size_t bytes, char **out) {
  ManyBufs &B = *J.buf;
  if (!B.ev_ex[slot]) MANYCHK(B.ev_ex[slot].create(hipEventDisableTiming));
  else MANYCHK(hipEventSynchronize(B.ev_ex[slot]));
  MANYCHK(many_grow_pinned(B.h_ex[slot], bytes));
  *out = B.h_ex[slot];
  return LSQR_OK;
}

template <class M>
int many_ex_run(ManyJob &J) {
  constexpr int K = M::K, SP = M::SP;
  const int W = many_width<M>(J.W);
  ManyBufs &B = *J.buf;
  const int org_off = fit_origin_offset<M>(J.cfg);
  const size_t NP = J.n;
  int st;
  static const bool trace = getenv("LSQR_MANY_TRACE") != nullptr;
  // (rows are 32-bit: a round of at most 2^30 hypotheses)
  const uint64_t cap = std::min<uint64_t>(J.round_cap ? J.round_cap : kManyRoundDefault, 1ull << 30);
  if ((st = many_check_width(J, W)) != LSQR_OK) return st;

  // every problem's C(N,k) and its path: none (N < k, or C(N,k) beyond 64 bits: refused), fused or general
  std::vector<uint64_t> count(NP, 0);
  std::vector<uint32_t> general, refused;
  std::vector<ManyExSmall> small;
  for (size_t j = 0; j < NP; j++) {
    memset(&J.infos[j], 0, sizeof(lsqr_ransac_info));
    const uint64_t n = J.offsets[j + 1] - J.offsets[j];
    if (n < (uint64_t)K) continue;
    if (!comb_count(n, K, &count[j])) refused.push_back((uint32_t)j);
    else if (J.ex_fused && n <= (uint64_t)kManyStage && count[j] <= kManyExFusedRanks)
      small.push_back(ManyExSmall{J.offsets[j], count[j], (uint32_t)n, (uint32_t)j});
    else general.push_back((uint32_t)j);
  }
  if ((st = many_upload(J)) != LSQR_OK) return st;
  MANYCHK(many_grow(B.d_best, NP * SP));
  MANYCHK(many_grow(B.d_exbest, 2 * NP));
  MANYCHK(hipMemsetAsync(B.d_exbest, 0, sizeof(unsigned long long) * 2 * NP, J.stream));

  int slot = 0;
  char *h;
  if (!small.empty()) {  // the fused path: one launch
    const size_t bytes = sizeof(ManyExSmall) * small.size();
    if ((st = many_ex_stage(J, slot, bytes, &h)) != LSQR_OK) return st;
    memcpy(h, small.data(), bytes);
    MANYCHK(many_grow(B.d_exsmall, bytes));
    MANYCHK(hipMemcpyAsync(B.d_exsmall, h, bytes, hipMemcpyHostToDevice, J.stream));
    MANYCHK(hipEventRecord(B.ev_ex[slot], J.stream));
    slot ^= 1;
    hipLaunchKernelGGL((k_many_ex_small<M>), dim3((unsigned)small.size()), dim3(kManyBlock), 0, J.stream, B.d_data, W,
                       (const ManyExSmall *)B.d_exsmall.get(), J.mc, B.d_best, B.d_exbest);
    MANYCHK(hipGetLastError());
  }

  // The general path's rounds, laid out from the counts alone.  Their buffers are sized once, for the largest round
  // there can be (the cap, or everything if that is less; no more items than problems; an item's tiles are its
  // 256-row blocks times its record segments), so that no round waits for the device to free one.
  if (!general.empty()) {
    uint64_t all = 0, seg_max = 0, seg_sum = 0;
    for (uint32_t j : general) {
      all = count[j] > cap - std::min(all, cap) ? cap : all + count[j];
      const uint64_t segs = (J.offsets[j + 1] - J.offsets[j] + kManySeg - 1) / kManySeg;
      seg_max = std::max(seg_max, segs);
      seg_sum += segs;
    }
    MANYCHK(many_grow(B.d_exitems, sizeof(ManyExItem) * general.size()));
    MANYCHK(many_grow(B.d_tiles, (size_t)((all / kManyBlock) * seg_max + seg_sum)));
    MANYCHK(many_grow(B.d_hparams, (size_t)all * SP));
    MANYCHK(many_grow(B.d_valid, (size_t)all));
    MANYCHK(many_grow(B.d_votes, (size_t)all));
  }
  std::vector<ManyExItem> items;
  std::vector<ManyTile> tiles;
  size_t g = 0, rounds = 0;
  uint64_t pos = 0, total = 0;
  while (g < general.size()) {
    items.clear();
    uint64_t Ht = 0;
    while (g < general.size() && Ht < cap) {
      const uint32_t j = general[g];
      const uint64_t H = std::min<uint64_t>(cap - Ht, count[j] - pos);
      items.push_back(ManyExItem{J.offsets[j], J.offsets[j + 1] - J.offsets[j], pos, (uint32_t)Ht, (uint32_t)H, j, 0});
      Ht += H;
      pos += H;
      if (pos < count[j]) break;  // the round is full: the problem goes on in the next one
      g++;
      pos = 0;
    }
    tiles.clear();  // as many_rounds: largest cost first
    for (const ManyExItem &it : items)
      for (uint32_t r0 = 0; r0 < it.H; r0 += kManyBlock)
        for (uint64_t r = 0; r < it.n; r += kManySeg) {
          ManyTile t;
          t.r0 = it.rec + r;
          t.r1 = it.rec + std::min<uint64_t>(it.n, r + kManySeg);
          t.h0 = it.h0 + r0;
          t.nh = std::min<uint32_t>(kManyBlock, it.H - r0);
          tiles.push_back(t);
        }
    std::stable_sort(tiles.begin(), tiles.end(), [](const ManyTile &a, const ManyTile &b) {
      return (uint64_t)a.nh * (a.r1 - a.r0) > (uint64_t)b.nh * (b.r1 - b.r0);
    });
    const size_t b_items = sizeof(ManyExItem) * items.size(), b_tiles = sizeof(ManyTile) * tiles.size();
    const size_t o_tiles = (b_items + 15) & ~(size_t)15;
    if ((st = many_ex_stage(J, slot, o_tiles + b_tiles, &h)) != LSQR_OK) return st;
    memcpy(h, items.data(), b_items);
    memcpy(h + o_tiles, tiles.data(), b_tiles);
    if (b_items > B.d_exitems.cap() || tiles.size() > B.d_tiles.cap() || Ht > B.d_votes.cap()) {
      snprintf(J.err, sizeof J.err, "round %zu exceeds the buffers sized for it", rounds);
      return LSQR_ERR_HIP;
    }
    MANYCHK(hipMemcpyAsync(B.d_exitems, h, b_items, hipMemcpyHostToDevice, J.stream));
    MANYCHK(hipMemcpyAsync(B.d_tiles, h + o_tiles, b_tiles, hipMemcpyHostToDevice, J.stream));
    MANYCHK(hipEventRecord(B.ev_ex[slot], J.stream));
    slot ^= 1;
    MANYCHK(hipMemsetAsync(B.d_votes, 0, sizeof(uint32_t) * Ht, J.stream));
    const ManyExItem *d_items = (const ManyExItem *)B.d_exitems.get();
    hipLaunchKernelGGL((k_many_ex_estimate<M>), dim3((unsigned)((Ht + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       J.stream, B.d_data, W, d_items, (int)items.size(), (uint32_t)Ht, J.mc, B.d_hparams, B.d_valid);
    MANYCHK(hipGetLastError());
    hipLaunchKernelGGL((k_many_scan<M>), dim3((unsigned)tiles.size()), dim3(kManyBlock), 0, J.stream, B.d_data, W,
                       B.d_tiles, B.d_hparams, B.d_valid, J.mc, B.d_votes);
    MANYCHK(hipGetLastError());
    hipLaunchKernelGGL(k_many_ex_best, dim3((unsigned)items.size()), dim3(kManyBlock), 0, J.stream, d_items,
                       B.d_votes, B.d_valid, (int)SP, B.d_hparams, B.d_best, B.d_exbest);
    MANYCHK(hipGetLastError());
    rounds++;
    total += Ht;
  }
  if (trace)
    fprintf(stderr, "ransac_many exhaustive: %zu problems, %zu fused, %zu general in %zu rounds of %llu hypotheses\n",
            NP, small.size(), general.size(), rounds, (unsigned long long)total);

  // every problem's winner: the one copy and the one wait before the finish
  std::vector<unsigned long long> exbest(2 * NP);
  MANYCHK(hipMemcpyAsync(exbest.data(), B.d_exbest, sizeof(unsigned long long) * 2 * NP, hipMemcpyDeviceToHost,
                         J.stream));
  MANYCHK(hipStreamSynchronize(J.stream));
  std::vector<ManyProb> pr(NP);
  for (size_t j = 0; j < NP; j++) {
    uint64_t *rs = pr[j].rs;
    for (int k = 0; k < 6; k++) rs[k] = 0;
    rs[RS_I] = pr[j].evaluated = count[j];  // iterations = evaluated = C(N,k)
    rs[RS_BEST] = exbest[2 * j];
    rs[RS_BEST_IDX] = exbest[2 * j + 1];
    rs[RS_HAS] = exbest[2 * j] != 0;
  }
  st = many_finish<M>(J, pr, [&](size_t j, const ManyProb &q) {
    uint64_t org = J.offsets[j];  // (unused with org_off >= 0)
    if (org_off < 0) {  // the first, smallest index of the winning combination (lsqr_ransac_exhaustive: win_rec)
      uint32_t idx[K];
      comb_unrank(J.offsets[j + 1] - J.offsets[j], K, q.rs[RS_BEST_IDX], idx);
      org += idx[0];
    }
    return org;
  });
  if (st != LSQR_OK) return st;
  // the problems that did not run (their info is still zero): N < k is RANSAC.hxx:165-169 (cleared, returns 0)
  for (size_t j = 0; j < NP; j++)
    if (J.offsets[j + 1] - J.offsets[j] < (uint64_t)K) J.status_out[j] = LSQR_EMPTY;
  for (uint32_t j : refused) J.status_out[j] = LSQR_ERR_INVALID;
  return LSQR_OK;
}
#endif

}  // namespace lsqr
