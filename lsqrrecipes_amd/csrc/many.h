// many.h -- lsqr_ransac_many: many independent RANSAC<T,S>::compute() problems (plane, line, algebraic sphere, absolute
// orientation, pivot calibration, ray intersection, 2-D line) in one call.  The problems' records are uploaded once,
// packed; then ROUNDS: every unfinished problem gets its next batch of hypotheses (the schedule of lsqr_ransac: 256 ->
// 1024 -> 4096, capped by the adaptive bound), the host replays each problem's serial loop over its votes
// (host_entry.h: host_replay + one DedupSet per problem), and the rows of the problems whose best changed are copied
// into a per-problem best array on the device.  When every problem is done, one segmented consensus mask + moment pass
// and one batched small solve finish them all.
//
//   k_many_sample_estimate  one lane per (problem, hypothesis) of the round: ctr_subset on the problem's stream at
//                           its running index, M::estimate on the gathered records, M::prepare -> scan row
//   k_many_scan             one workgroup per tile (problem, <= 256 hypotheses, <= kManySeg records); lane =
//                           hypothesis with its scan row in registers; the records are staged through LDS and
//                           read by every lane at the same address (broadcast); exact fp64 M::agree
//   k_many_gather           winners' scan rows -> best[problem]
//   k_many_mask_moments     consensus mask + phase-0 moment block about the winner's own point, one workgroup per
//                           kManyPart records of a problem
//   k_many_solve            one wave per problem: fixed-order sum of its parts, then solve_small (= k_solve)
//
// Records: W = lsqr_record_doubles(cfg) doubles each (the context's record width, packed on upload), read through
// M::load as the single path reads them: absolute orientation's weight slot (W = 7 with ls_type 2), the pivot
// frame's 12 doubles of 13.  Fit origin: set_fit_origin's rule for a RANSAC finish -- the winner's own point
// (fit_origin_offset), or for the ORIGIN_FIRST models the first drawn record of the winning minimal subset.
//
// Independence: every quantity a problem's result depends on is a function of that problem's records alone: its
// hypotheses (its own stream), its votes (integer sums), its moment block (parts of kManyPart records in record
// order, reduced in part order).  The round cap only decides which problems share a round.
//
// Host side: the frame of a batched call -- many_begin, many_rounds, many_plan_finish, many_stage_finish,
// many_fetch_finish, many_end for a RANSAC job; many_fit_begin, many_write_fits for a *_fit_many job -- is here, for
// many_run, the LM stage (many_lm.h) and the dense system (many_dense.h), which add their kernels and what is theirs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include "devbuf.h"
#include "host_entry.h"
#include "kernels.h"

namespace lsqr {

constexpr int kManyBlock = 256;            // hypotheses per scan tile: four waves, one lane each
constexpr int kManyStage = 256;            // records per LDS stage (8-D: 16 KiB, pivot frames: 26 KiB)
constexpr uint64_t kManySeg = 16384;       // records per scan tile: longer problems are split, votes summed exactly
constexpr uint64_t kManyPart = 8192;       // records per workgroup of the finish (fixes the moment sums' order)
constexpr size_t kManyRoundDefault = 1u << 21;  // hypotheses per round (option many_round_hypotheses = 0)

#if defined(__HIPCC__)
// a device buffer of the batched calls, grown on demand
template <class T>
hipError_t many_grow(DevBuf<T> &b, size_t n) {
  const size_t want = grow_quarter(b, n, 64);
  return want ? b.alloc(want) : hipSuccess;
}
// pinned host memory; the caller has synchronised the stream if an old buffer may still be read by a copy
inline hipError_t many_grow_pinned(PinBuf<char> &b, size_t bytes) {
  const size_t want = grow_quarter(b, bytes, 1 << 16);
  return want ? b.alloc(want) : hipSuccess;
}
#endif
}  // namespace lsqr

// a HIP call of the batched host code (many.h, many_lm.h, many_dense.h, many_exhaustive.h, many_sequential.h,
// grouped.h, assign.h, assign_dense.h, assign_lm.h, assign_grouped.h, assign_lm_grouped.h, assign_dense_grouped.h;
// undefined at the end of the last): J is the job at hand -- a ManyJob, the LM stage's ManyLmJob, whose err is the
// ManyJob's, an AssignJob or an AssignGrpJob
#define MANYCHK(call)                                                                                \
  do {                                                                                               \
    hipError_t e_ = (call);                                                                          \
    if (e_ != hipSuccess) {                                                                          \
      snprintf(J.err, sizeof J.err, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
               __LINE__);                                                                            \
      return LSQR_ERR_HIP;                                                                           \
    }                                                                                                \
  } while (0)

#include "many_lm.h"  // the LM stage of lsqr_ransac_many_lm (its parts are kManyPart inliers)

namespace lsqr {

struct ManyItem {   // one problem's batch in a round
  uint64_t rec;     // first record of the problem in the packed upload
  uint64_t n;       // its record count
  uint64_t seed;    // its sampler stream
  uint64_t first;   // stream index of the batch's first hypothesis
  uint32_t h0, H;   // rows [h0, h0 + H) of the round's hypothesis arrays
};
struct ManyTile {   // scan work item: rows [h0, h0 + nh) against records [r0, r1)
  uint64_t r0, r1;
  uint32_t h0, nh;
};
struct ManyPart {   // finish work item: records [r0, r1) of problem j (finishing slot f); org: its fit origin's record
  uint64_t r0, r1, org;
  uint32_t j, f;
};

// the models lsqr_ransac_many runs: plane, line and sphere in every dimension (sphere: algebraic fit only), and the
// closed-form estimators of rigid.h.  Their estimate / agree / solve read only the call-independent ModelConsts
// fields (delta, delta_sq, ls_type, aux); absmax / absmax_rot belong to the context's own upload and are read by
// the fp32 filters alone (prepare_f32), which this path does not run.
template <class M> struct ManyModel { static constexpr bool value = false; };
template <int D> struct ManyModel<PlaneModel<D>> { static constexpr bool value = true; };
template <int D> struct ManyModel<LineModel<D>> { static constexpr bool value = true; };
template <int D> struct ManyModel<SphereModel<D>> { static constexpr bool value = true; };
template <int D> struct ManyModel<PlaneModelN<D>> { static constexpr bool value = true; };
template <int D> struct ManyModel<LineModelN<D>> { static constexpr bool value = true; };
template <int D> struct ManyModel<SphereModelN<D>> { static constexpr bool value = true; };
template <> struct ManyModel<AbsOrModel> { static constexpr bool value = true; };
template <> struct ManyModel<PivotModel> { static constexpr bool value = true; };
template <> struct ManyModel<RayModel> { static constexpr bool value = true; };
template <> struct ManyModel<Line2DModel> { static constexpr bool value = true; };  // (not matched as PlaneModel<2>)

// doubles per record: ND, except absolute orientation, whose records carry a weight with ls_type 2 (W = 6 or 7, a
// call's value); the LDS stage of the scan holds the widest
template <class M> constexpr int many_wmax() { return M::REC > M::ND ? M::REC : M::ND; }
template <class M> LSQR_HD int many_width(int W) { return M::REC > M::ND ? W : (int)M::ND; }

// where the fit origin lies in a scan-parameter row (the rule of set_fit_origin): the model's own point -- the
// sphere's centre, the plane's / line's point --, or -1 for the models whose parameters hold no point (their origin is
// the first drawn record of the winning minimal subset)
template <class M>
inline int fit_origin_offset(const lsqr_model_cfg &cfg) {
  if constexpr (requires { M::ORIGIN_FIRST; }) return -1;
  else return cfg.model == LSQR_MODEL_SPHERE ? 0 : (int)M::ND;
}

#if defined(__HIPCC__)
template <class M>
__global__ __launch_bounds__(kBlock) void k_many_sample_estimate(const double *__restrict__ data, int W,
                                                                 const ManyItem *__restrict__ items, int n_items,
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
  const ManyItem it = items[lo];
  uint32_t idx[M::K], sorted[M::K];
  ctr_subset(it.seed, it.first + (h - it.h0), it.n, M::K, idx, sorted);
  const int w = many_width<M>(W);
  double r[M::K][M::ND];
  for (int l = 0; l < M::K; l++)
    for (int j = 0; j < M::ND; j++) r[l][j] = data[(it.rec + idx[l]) * w + j];
  // from here on as k_estimate
  double par[M::P];
  const bool ok = M::estimate(r, mc, par);
  const double qnan = __builtin_nan("");
  double sp[M::SP];
  for (int j = 0; j < M::P; j++) sp[j] = ok ? par[j] : qnan;
  for (int j = M::P; j < M::SP; j++) sp[j] = 0.0;
  M::prepare(sp, mc);
  for (int j = 0; j < M::SP; j++) hparams[(size_t)h * M::SP + j] = sp[j];
  valid[h] = ok ? 1 : 0;
}

template <class M>
__global__ __launch_bounds__(kManyBlock) void k_many_scan(const double *__restrict__ data, int W,
                                                          const ManyTile *__restrict__ tiles,
                                                          const double *__restrict__ hparams,
                                                          const uint8_t *__restrict__ valid, ModelConsts mc,
                                                          uint32_t *__restrict__ votes) {
  __shared__ double s_rec[kManyStage * many_wmax<M>()];
  const int w = many_width<M>(W);
  const ManyTile t = tiles[blockIdx.x];
  const uint32_t lane = threadIdx.x;
  const bool live = lane < t.nh && valid[t.h0 + lane];
  double sp[M::SP];
#pragma unroll
  for (int j = 0; j < M::SP; j++) sp[j] = live ? hparams[(size_t)(t.h0 + lane) * M::SP + j] : 0.0;
  uint32_t c = 0;
  for (uint64_t r0 = t.r0; r0 < t.r1; r0 += kManyStage) {
    const uint32_t m = (uint32_t)(t.r1 - r0 < (uint64_t)kManyStage ? t.r1 - r0 : (uint64_t)kManyStage);
    __syncthreads();  // the previous stage has been read
    const double *src = data + r0 * w;
    for (uint32_t q = threadIdx.x; q < m * w; q += kManyBlock) s_rec[q] = src[q];
    __syncthreads();
    if (live) {
      for (uint32_t i = 0; i < m; i++) {
        double x[M::REC];
        M::load(s_rec + i * w, mc, x);  // same address in every lane: broadcast
        c += M::agree(sp, x, mc) ? 1u : 0u;
      }
    }
  }
  if (live && c) atomicAdd(&votes[t.h0 + lane], c);
}

__global__ __launch_bounds__(kBlock) void k_many_gather(const uint32_t *__restrict__ pairs, uint32_t n_pairs, int sp,
                                                        const double *__restrict__ hparams,
                                                        double *__restrict__ best) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= n_pairs * (uint32_t)sp) return;
  const uint32_t w = t / sp, k = t % sp;  // pair w = (problem, round row)
  best[(size_t)pairs[2 * w] * sp + k] = hparams[(size_t)pairs[2 * w + 1] * sp + k];
}

// k_mask_moments for a part of one problem: the same per-thread order, shuffle tree and wave sum
template <class M>
__global__ __launch_bounds__(kBlock) void k_many_mask_moments(const double *__restrict__ data, int W,
                                                              const ManyPart *__restrict__ parts,
                                                              const double *__restrict__ best, int org_off,
                                                              ModelConsts mc, uint8_t *__restrict__ mask,
                                                              unsigned long long *__restrict__ counts,
                                                              double *__restrict__ partials) {
  typedef AccLs<M> A;
  __shared__ double s_m[kBlock / 64][A::N];
  __shared__ uint32_t s_c[kBlock / 64];
  const ManyPart pt = parts[blockIdx.x];
  double acc[A::N];
#pragma unroll
  for (int k = 0; k < A::N; k++) acc[k] = 0.0;
  double sp[M::SP];
  for (int j = 0; j < M::SP; j++) sp[j] = best[(size_t)pt.j * M::SP + j];
  constexpr int NC = M::P > M::REC ? M::P : M::REC;
  double cv[NC];
  const int w = many_width<M>(W);
  // (ORIGIN_FIRST: the first drawn record of the winning subset; both from global memory, so that sp stays in
  // registers)
  const double *org = org_off < 0 ? data + pt.org * w : best + (size_t)pt.j * M::SP + org_off;
  for (int k = 0; k < NC; k++) cv[k] = k < M::ND ? org[k] : 0.0;
  uint32_t local = 0;
  for (uint64_t i = pt.r0 + threadIdx.x; i < pt.r1; i += kBlock) {
    double x[M::REC];
    M::load(data + i * w, mc, x);
    const bool a = M::agree(sp, x, mc);
    mask[i] = a ? 1 : 0;
    if (!a) continue;
    local++;
    A::acc(x, cv, acc);
  }
#pragma unroll
  for (int k = 0; k < A::N; k++) {
    double v = acc[k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6][k] = v;
  }
  for (int o = 32; o > 0; o >>= 1) local += __shfl_down(local, o);
  if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x < A::N) {
    double t = 0.0;
    for (int w = 0; w < kBlock / 64; w++) t += s_m[w][threadIdx.x];
    partials[(size_t)blockIdx.x * A::N + threadIdx.x] = t;
  }
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < kBlock / 64; w++) t += s_c[w];
    if (t) atomicAdd(&counts[pt.f], t);
  }
}

// one wave per finishing problem f: its parts [pbeg[f], pbeg[f+1]) summed in part order, then the solve of k_solve
template <class M>
__global__ __launch_bounds__(64) void k_many_solve(const double *__restrict__ data, int W,
                                                   const ManyPart *__restrict__ parts,
                                                   const double *__restrict__ partials,
                                                   const uint32_t *__restrict__ pbeg,
                                                   const uint32_t *__restrict__ fin, const double *__restrict__ best,
                                                   int org_off, ModelConsts mc, SolveOut *__restrict__ out) {
  __shared__ double m[MOM_MAX];
  __shared__ double ws[M::NMOM > 40 ? 512 : 8];
  const uint32_t f = blockIdx.x;
  for (int k = threadIdx.x; k < (int)M::NMOM; k += 64) {
    double t = 0.0;
    for (uint32_t q = pbeg[f]; q < pbeg[f + 1]; q++) t += partials[(size_t)q * M::NMOM + k];
    m[k] = t;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  constexpr int NC = M::P > M::REC ? M::P : M::REC;
  double org[NC];
  const double *o = org_off < 0 ? data + parts[pbeg[f]].org * many_width<M>(W)
                                 : best + (size_t)fin[f] * M::SP + org_off;
  for (int k = 0; k < NC; k++) org[k] = k < M::ND ? o[k] : 0.0;
  solve_small<M>(m, org, mc, ws, out + f);
}
#endif

// ---- host side -------------------------------------------------------------------------------------------------
// device and pinned buffers of the call, owned by the context and grown on demand; deleting the set frees them all
#if defined(__HIPCC__)
struct ManyBufs {
  DevBuf<double> d_data, d_hparams, d_best, d_partials;
  DevBuf<ManyItem> d_items;
  DevBuf<ManyTile> d_tiles;
  DevBuf<ManyPart> d_parts;
  DevBuf<uint8_t> d_valid, d_mask;
  DevBuf<uint32_t> d_votes, d_pairs, d_pbeg, d_fin;
  DevBuf<unsigned long long> d_counts;
  DevBuf<SolveOut> d_out;
  PinBuf<char> h_stage, h_pairs;  // pinned: the round's tables and results / the winner pairs
  ManyLmBufs lm;  // the LM stage of lsqr_ransac_many_lm / lsqr_lm_fit_many (many_lm.h)
  // lsqr_ransac_many_dense / lsqr_dense_fit_many (many_dense.h): the round's subsets, the minimal systems the
  // elimination refused, the problems' moment blocks, their double-double flags and the double-double Gram partials
  DevBuf<uint32_t> d_sub, d_marked;
  DevBuf<double> d_mom, d_ddpart;
  DevBuf<int> d_flags;
  // lsqr_ransac_many_exhaustive (many_exhaustive.h): the round's items, the fused path's problems, every problem's
  // running {votes, rank}, and two pinned staging buffers with the events that guard their reuse
  DevBuf<char> d_exitems, d_exsmall;
  DevBuf<unsigned long long> d_exbest;
  PinBuf<char> h_ex[2];
  Event ev_ex[2];
  // lsqr_ransac_many_sequential (many_sequential.h): the record buffer the survivors of a round are packed into (it
  // and d_data change places after every partition), the survivors' upload indices (two, in turn), the labels, the
  // partition's parts and their survivor counts, and the pinned staging of the parts
  DevBuf<double> d_seq_rec;
  DevBuf<uint32_t> d_seq_orig[2], d_seq_counts;
  DevBuf<int32_t> d_seq_labels;
  DevBuf<char> d_seq_parts;
  PinBuf<char> h_seq;
  // lsqr_ransac_grouped (grouped.h): the (label key, record index) pairs before and after the sort, the sort's
  // temporaries, the group offsets, the winner flags, the labels and the consensus of the host form, and the pinned
  // staging of the offsets and flags
  DevBuf<uint32_t> d_grp_keys[2], d_grp_vals[2];
  DevBuf<char> d_grp_tmp;
  PinBuf<char> h_grp;
  DevBuf<uint64_t> d_grp_off;
  DevBuf<uint8_t> d_grp_flag, d_grp_cons;
  DevBuf<int32_t> d_grp_labels;
  DevBuf<int32_t> d_grp_lab;  // lsqr_ransac_grouped_sequential, host form: the round labels in upload order
};

// One batched call.  The entry point fills it from the context (lsqr_hip.hip: many_call); p, seeds, consensus_out and
// infos are a RANSAC call's and stay unset in a *_fit_many job, which reads none of them.
struct ManyJob {
  hipStream_t stream = nullptr;
  lsqr_model_cfg cfg = {};
  ModelConsts mc = {};
  const char *host = nullptr;  // records, stride bytes apart
  // the records lie in buf->d_data already, packed (a round of many_sequential.h on the survivors of the last one):
  // many_upload copies nothing and host stays unread
  bool resident = false;
  size_t stride = 0;
  const uint64_t *offsets = nullptr;
  size_t n = 0;  // problems
  int W = 0;     // doubles per record (lsqr_record_doubles)
  double p = 0;
  const uint64_t *seeds = nullptr;
  double *params_out = nullptr;
  uint8_t *consensus_out = nullptr;
  lsqr_ransac_info *infos = nullptr;
  int32_t *status_out = nullptr;
  long long max_iter = 0;  // option max_iterations
  // hypotheses per round (a problem whose batch alone exceeds it gets a round of its own): option
  // many_round_hypotheses; 0: the path's default, resolved by many_run / many_dense_run
  size_t round_cap = 0;
  bool lm = false;  // the geometric sphere: many_run ends in the LM fit from the algebraic one (many_lm.h)
  int lm_n = 0, lm_maxfev = 0;  // lm_settings
  double lm_ftol = 0, lm_xtol = 0, lm_gtol = 0;
  int dense_fast = 1, dense_dd = 1;  // options dense_fast_solve / dense_dd (many_dense.h)
  int ex_fused = 1;                  // option many_exhaustive_fused (many_exhaustive.h)
  ManyBufs *buf = nullptr;
  std::vector<double> packed;  // many_upload's staging copy of strided records
  char err[256] = "";
};

// The record width the model's kernels read against the job's.  It cannot differ (J.W is the context's own ND for the
// same cfg); it is tested once, before anything is written.
inline int many_check_width(ManyJob &J, int W) {
  if (W == J.W) return LSQR_OK;
  snprintf(J.err, sizeof J.err, "record width %d != the model's %d doubles", J.W, W);
  return LSQR_ERR_INVALID;
}

// one upload of every problem's records, packed (W doubles per record, copied as raw bytes: the pivot frame's int slot
// travels as it is)
inline int many_upload(ManyJob &J) {
  ManyBufs &B = *J.buf;
  const uint64_t NT = J.offsets[J.n];
  const size_t W = J.W;
  const double *src = (const double *)J.host;
  if (NT > 0 && !J.resident) {
    MANYCHK(many_grow(B.d_data, NT * W));
    if (J.stride != sizeof(double) * W) {
      J.packed.resize(NT * W);
      for (uint64_t i = 0; i < NT; i++) memcpy(&J.packed[i * W], J.host + i * J.stride, sizeof(double) * W);
      src = J.packed.data();
    }
    MANYCHK(hipMemcpyAsync(B.d_data, src, sizeof(double) * W * NT, hipMemcpyHostToDevice, J.stream));
  }
  return LSQR_OK;
}

// the per-problem state of lsqr_ransac's loop
struct ManyProb {
  uint64_t rs[6];
  uint64_t base = 0, evaluated = 0;
  size_t batch = 256;
  bool live = false;
  std::unique_ptr<DedupSet> dedup;
};

// host replay of items [i0, i1) of a round: lsqr_ransac's loop body after the batch's votes are in.  Subsets are
// regenerated on the host (the same ctr_subset), piece by piece, only as far as the replay consumes them.
// K: the minimal subset's size (<= 64: the dense system's n)
inline void many_replay(const ManyJob &J, std::vector<ManyProb> &pr, const std::vector<uint32_t> &item_prob,
                        const ManyItem *items, size_t i0, size_t i1, const uint32_t *votes, const uint8_t *valid,
                        std::vector<uint32_t> *pairs, int K) {
  constexpr size_t kPiece = 64;
  std::vector<uint32_t> sub(kPiece * K), sorted(K);
  for (size_t t = i0; t < i1; t++) {
    const ManyItem &it = items[t];
    const uint32_t j = item_prob[t];
    ManyProb &q = pr[j];
    if (!q.dedup) q.dedup.reset(new DedupSet(1024));
    const uint64_t prev_best_idx = q.rs[RS_BEST_IDX];
    const bool had = q.rs[RS_HAS] != 0;
    size_t used = 0;
    while (used < it.H) {  // host_replay over the batch, fed in pieces: the same sequential loop
      const size_t m = std::min<size_t>(kPiece, it.H - used);
      for (size_t e = 0; e < m; e++)
        ctr_subset(it.seed, it.first + used + e, it.n, K, sub.data() + e * K, sorted.data());
      const size_t u = host_replay(it.n, K, J.p, sub.data(), valid + it.h0 + used, votes + it.h0 + used, m,
                                   it.first + used, q.dedup.get(), q.rs);
      used += u;
      if (u < m) break;
    }
    q.evaluated += it.H;
    if (q.rs[RS_HAS] && (!had || q.rs[RS_BEST_IDX] != prev_best_idx)) {
      pairs->push_back(j);
      pairs->push_back(it.h0 + (uint32_t)(q.rs[RS_BEST_IDX] - it.first));
    }
    q.base += used;
    bool done = q.rs[RS_DONE] != 0 || used < it.H;
    q.batch = std::min<size_t>(q.batch * 4, 4096);
    // lsqr_ransac's safety stop (2^22 iterations without any model) and the caller's budget
    if (!q.rs[RS_HAS] && q.base >= (1ull << 22)) done = true;
    if (J.max_iter > 0 && q.base >= (uint64_t)J.max_iter) done = true;
    if (done) {
      q.live = false;
      q.dedup.reset();
    }
  }
}

// lsqr_ransac_many's rounds over the live problems of pr (host_replay_init done): per round the batches, the scan
// tiles (<= kManyBlock hypotheses x <= seg records, largest first), launch(n_items, Ht, n_tiles) -- the model's
// kernels: B.d_items / B.d_tiles in, B.d_hparams (SP doubles per hypothesis), B.d_valid and B.d_votes (zeroed) out --,
// the host replay (K: the minimal subset's size) and the gather of the winners' rows into B.d_best
template <class Launch>
int many_rounds(ManyJob &J, std::vector<ManyProb> &pr, int K, int SP, uint64_t seg, Launch &&launch) {
  ManyBufs &B = *J.buf;
  const size_t NP = J.n;
  int st;
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  // diagnostics (LSQR_MANY_TRACE): per round the batches, hypotheses, tiles, device wait and host replay time
  static const bool trace = getenv("LSQR_MANY_TRACE") != nullptr;
  typedef std::chrono::steady_clock Clock;
  int round = 0;
  std::vector<uint32_t> live, item_prob;
  std::vector<ManyItem> items;
  std::vector<ManyTile> tiles;
  size_t cursor = 0;
  for (;;) {
    live.clear();
    for (size_t j = 0; j < NP; j++)
      if (pr[j].live) live.push_back((uint32_t)j);
    if (live.empty()) break;
    // this round's batches: lsqr_ransac's loop head per problem; problems beyond the cap wait for the next round
    items.clear();
    item_prob.clear();
    uint64_t Ht = 0;
    const size_t L = live.size();
    size_t taken = 0;
    for (; taken < L; taken++) {
      const uint32_t j = live[(cursor + taken) % L];
      ManyProb &q = pr[j];
      size_t H = q.batch;
      const uint64_t remaining = q.rs[RS_TRIES] - q.base;
      if (remaining < H) H = (size_t)remaining;
      if (H == 0) {
        q.live = false;
        q.dedup.reset();
        continue;
      }
      if (!items.empty() && Ht + H > J.round_cap) break;
      ManyItem it;
      it.rec = J.offsets[j];
      it.n = J.offsets[j + 1] - J.offsets[j];
      it.seed = J.seeds[j];
      it.first = q.base;
      it.h0 = (uint32_t)Ht;
      it.H = (uint32_t)H;
      items.push_back(it);
      item_prob.push_back(j);
      Ht += H;
    }
    cursor = L ? (cursor + taken) % L : 0;
    if (items.empty()) continue;
    // scan tiles, largest cost first, so that one long problem does not set the tail
    tiles.clear();
    for (const ManyItem &it : items)
      for (uint32_t h = 0; h < it.H; h += kManyBlock)
        for (uint64_t r = 0; r < it.n; r += seg) {
          ManyTile t;
          t.r0 = it.rec + r;
          t.r1 = it.rec + std::min<uint64_t>(it.n, r + seg);
          t.h0 = it.h0 + h;
          t.nh = std::min<uint32_t>(kManyBlock, it.H - h);
          tiles.push_back(t);
        }
    std::stable_sort(tiles.begin(), tiles.end(), [](const ManyTile &a, const ManyTile &b) {
      return (uint64_t)a.nh * (a.r1 - a.r0) > (uint64_t)b.nh * (b.r1 - b.r0);
    });
    const size_t b_items = sizeof(ManyItem) * items.size(), b_tiles = sizeof(ManyTile) * tiles.size();
    const size_t o_tiles = (b_items + 15) & ~(size_t)15, o_votes = (o_tiles + b_tiles + 15) & ~(size_t)15;
    const size_t o_valid = o_votes + sizeof(uint32_t) * Ht;
    MANYCHK(many_grow_pinned(B.h_stage, o_valid + Ht));  // the previous round ended in a sync
    memcpy(B.h_stage, items.data(), b_items);
    memcpy(B.h_stage + o_tiles, tiles.data(), b_tiles);
    MANYCHK(many_grow(B.d_items, items.size()));
    MANYCHK(many_grow(B.d_tiles, tiles.size()));
    MANYCHK(many_grow(B.d_hparams, Ht * SP));
    MANYCHK(many_grow(B.d_valid, Ht));
    MANYCHK(many_grow(B.d_votes, Ht));
    MANYCHK(hipMemcpyAsync(B.d_items, B.h_stage, b_items, hipMemcpyHostToDevice, J.stream));
    MANYCHK(hipMemcpyAsync(B.d_tiles, B.h_stage + o_tiles, b_tiles, hipMemcpyHostToDevice, J.stream));
    MANYCHK(hipMemsetAsync(B.d_votes, 0, sizeof(uint32_t) * Ht, J.stream));
    if ((st = launch(items.size(), Ht, tiles.size())) != LSQR_OK) return st;
    uint32_t *h_votes = (uint32_t *)(B.h_stage + o_votes);
    uint8_t *h_valid = (uint8_t *)(B.h_stage + o_valid);
    MANYCHK(hipMemcpyAsync(h_votes, B.d_votes, sizeof(uint32_t) * Ht, hipMemcpyDeviceToHost, J.stream));
    MANYCHK(hipMemcpyAsync(h_valid, B.d_valid, Ht, hipMemcpyDeviceToHost, J.stream));
    const Clock::time_point t_sync = Clock::now();
    MANYCHK(hipStreamSynchronize(J.stream));
    const Clock::time_point t_replay = Clock::now();
    // replay, problems spread over host threads (each item touches its own problem's state only); an item's cost
    // grows as K^2 (ctr_subset), so the dense system's large subsets take threads at fewer items
    const size_t NI = items.size();
    const size_t per_item = std::max<size_t>((size_t)K * K / 64, 1);
    const unsigned T = (unsigned)std::min<size_t>(std::min<unsigned>(hw, 16), (NI * per_item + 127) / 128);
    std::vector<std::vector<uint32_t>> pairs(std::max(1u, T));
    if (T <= 1) {
      many_replay(J, pr, item_prob, items.data(), 0, NI, h_votes, h_valid, &pairs[0], K);
    } else {
      std::vector<std::thread> th;
      for (unsigned w = 0; w < T; w++)
        th.emplace_back([&, w] {
          many_replay(J, pr, item_prob, items.data(), NI * w / T, NI * (w + 1) / T, h_votes, h_valid, &pairs[w],
                      K);
        });
      for (auto &x : th) x.join();
    }
    size_t np = 0;
    for (auto &v : pairs) np += v.size();
    if (trace)
      fprintf(stderr, "ransac_many round %d: %zu batches, %llu hypotheses, %zu tiles, wait %.3f ms, replay %.3f ms\n",
              round, NI, (unsigned long long)Ht, tiles.size(),
              std::chrono::duration<double, std::milli>(t_replay - t_sync).count(),
              std::chrono::duration<double, std::milli>(Clock::now() - t_replay).count());
    round++;
    if (np) {  // winner rows -> best[problem], on the device, before the next round overwrites the rows
      MANYCHK(many_grow_pinned(B.h_pairs, sizeof(uint32_t) * np));
      size_t o = 0;
      for (auto &v : pairs) {
        memcpy((uint32_t *)B.h_pairs.get() + o, v.data(), sizeof(uint32_t) * v.size());
        o += v.size();
      }
      MANYCHK(many_grow(B.d_pairs, np));
      MANYCHK(hipMemcpyAsync(B.d_pairs, B.h_pairs, sizeof(uint32_t) * np, hipMemcpyHostToDevice, J.stream));
      const uint32_t npairs = (uint32_t)(np / 2);
      hipLaunchKernelGGL(k_many_gather, dim3((unsigned)((npairs * SP + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                         J.stream, B.d_pairs, npairs, (int)SP, B.d_hparams, B.d_best);
      MANYCHK(hipGetLastError());
      // the next round writes h_pairs only after its own synchronisation, which follows this copy
    }
  }

  return LSQR_OK;
}

// ---- the frame of a batched call, shared by the closed-form models (many_run), their LM stage and the dense system
// (many_dense.h).  A RANSAC job: many_begin, many_rounds, many_plan_finish, many_stage_finish + the model's finish
// kernels, many_fetch_finish, many_end.  A *_fit_many job: many_fit_begin, the model's fit, many_write_fits. --------

// The start of a RANSAC job: every problem's loop state (K: the minimal subset's size; the dense system's is known at
// run time only), the upload, and room for the winners' rows (SP doubles per problem).  A problem of fewer than K
// records is RANSAC.hxx:16-19's "return 0": info cleared, status ERR_INVALID, every other output untouched.
inline int many_begin(ManyJob &J, int W, int K, int SP, std::vector<ManyProb> &pr) {
  int st;
  if ((st = many_check_width(J, W)) != LSQR_OK) return st;
  pr.resize(J.n);
  for (size_t j = 0; j < J.n; j++) {
    memset(&J.infos[j], 0, sizeof(lsqr_ransac_info));
    const uint64_t n = J.offsets[j + 1] - J.offsets[j];
    if (n < (uint64_t)K) {
      J.status_out[j] = LSQR_ERR_INVALID;
      continue;
    }
    host_replay_init(n, K, J.p, pr[j].rs);
    pr[j].live = !pr[j].rs[RS_DONE];
  }
  if ((st = many_upload(J)) != LSQR_OK) return st;
  MANYCHK(many_grow(J.buf->d_best, std::max<size_t>(J.n, 1) * SP));
  return LSQR_OK;
}

// The finish of a job.  The problems (sets) with something to fit take the finishing slots f = 0, 1, ... in problem
// order: slot f is problem fin[f], and its work items are parts [pbeg[f], pbeg[f + 1]), kManyPart records each.
// counts / outs: each slot's records in use and its fit, after many_fetch_finish.
struct ManyFinish {
  std::vector<uint32_t> fin, pbeg = {0};
  std::vector<ManyPart> parts;
  std::vector<unsigned long long> counts;
  std::vector<SolveOut> outs;
  size_t size() const { return fin.size(); }
  // problem j = records [r0, r1), its moments summed about record org (where the model's kernels read one)
  void add(uint32_t j, uint64_t r0, uint64_t r1, uint64_t org) {
    const uint32_t f = (uint32_t)fin.size();
    fin.push_back(j);
    for (uint64_t r = r0; r < r1; r += kManyPart)
      parts.push_back(ManyPart{r, std::min<uint64_t>(r1, r + kManyPart), org, j, f});
    pbeg.push_back((uint32_t)parts.size());
  }
};

// The plan of a RANSAC job's finish, after the rounds: finish_ransac's info fields of every problem that ran; status
// EMPTY where there is no winner or no vote; a finishing slot for the others.  org(j, q): the origin record of
// problem j's parts.
template <class Org>
ManyFinish many_plan_finish(ManyJob &J, const std::vector<ManyProb> &pr, int K, Org &&org) {
  ManyFinish F;
  for (size_t j = 0; j < J.n; j++) {
    const uint64_t n = J.offsets[j + 1] - J.offsets[j];
    if (n < (uint64_t)K) continue;
    const ManyProb &q = pr[j];
    lsqr_ransac_info &info = J.infos[j];
    info.iterations = q.rs[RS_I];
    info.best_index = q.rs[RS_BEST_IDX];
    info.evaluated = q.evaluated;
    info.best_votes = (uint32_t)q.rs[RS_BEST];
    info.fraction = (double)info.best_votes / (double)n;
    info.n_params = 0;
    if (!q.rs[RS_HAS] || info.best_votes == 0) {
      J.status_out[j] = LSQR_EMPTY;
      continue;
    }
    F.add((uint32_t)j, J.offsets[j], J.offsets[j + 1], org(j, q));
  }
  return F;
}

// The finish tables of F (not empty) onto the device, staged through h_stage: parts, pbeg and, where a kernel reads it
// (with_fin), fin; room for the slots' counts and fits, the counts zeroed.
inline int many_stage_finish(ManyJob &J, const ManyFinish &F, bool with_fin) {
  ManyBufs &B = *J.buf;
  const size_t NF = F.size();
  const size_t b_parts = sizeof(ManyPart) * F.parts.size(), b_pbeg = sizeof(uint32_t) * F.pbeg.size();
  const size_t o_pbeg = (b_parts + 15) & ~(size_t)15, o_fin = (o_pbeg + b_pbeg + 15) & ~(size_t)15;
  MANYCHK(many_grow(B.d_parts, F.parts.size()));
  MANYCHK(many_grow(B.d_pbeg, F.pbeg.size()));
  if (with_fin) MANYCHK(many_grow(B.d_fin, NF));
  MANYCHK(many_grow(B.d_counts, NF));
  MANYCHK(many_grow(B.d_out, NF));
  MANYCHK(many_grow_pinned(B.h_stage, with_fin ? o_fin + sizeof(uint32_t) * NF : o_pbeg + b_pbeg));
  memcpy(B.h_stage, F.parts.data(), b_parts);
  memcpy(B.h_stage + o_pbeg, F.pbeg.data(), b_pbeg);
  MANYCHK(hipMemcpyAsync(B.d_parts, B.h_stage, b_parts, hipMemcpyHostToDevice, J.stream));
  MANYCHK(hipMemcpyAsync(B.d_pbeg, B.h_stage + o_pbeg, b_pbeg, hipMemcpyHostToDevice, J.stream));
  if (with_fin) {
    memcpy(B.h_stage + o_fin, F.fin.data(), sizeof(uint32_t) * NF);
    MANYCHK(hipMemcpyAsync(B.d_fin, B.h_stage + o_fin, sizeof(uint32_t) * NF, hipMemcpyHostToDevice, J.stream));
  }
  MANYCHK(hipMemsetAsync(B.d_counts, 0, sizeof(unsigned long long) * NF, J.stream));
  return LSQR_OK;
}

// The slots' counts and fits back from the device, behind the finish kernels, and the job's synchronisation.  A RANSAC
// job (ransac) also takes the consensus bytes from B.d_mask and checks, as finish_ransac does, that every winner's
// mask count is its scan's vote.
inline int many_fetch_finish(ManyJob &J, ManyFinish &F, bool ransac) {
  ManyBufs &B = *J.buf;
  const size_t NF = F.size();
  const uint64_t NT = J.offsets[J.n];
  F.counts.assign(NF, 0);
  F.outs.assign(NF, SolveOut());
  if (NF) {
    MANYCHK(hipMemcpyAsync(F.counts.data(), B.d_counts, sizeof(unsigned long long) * NF, hipMemcpyDeviceToHost,
                           J.stream));
    MANYCHK(hipMemcpyAsync(F.outs.data(), B.d_out, sizeof(SolveOut) * NF, hipMemcpyDeviceToHost, J.stream));
    if (ransac && J.consensus_out && NT)
      MANYCHK(hipMemcpyAsync(J.consensus_out, B.d_mask, NT, hipMemcpyDeviceToHost, J.stream));
  }
  MANYCHK(hipStreamSynchronize(J.stream));
  for (size_t f = 0; f < NF; f++) {
    const uint32_t j = F.fin[f];
    if (ransac && F.counts[f] != J.infos[j].best_votes) {
      snprintf(J.err, sizeof J.err, "problem %u: consensus mask count %llu != scan votes %u", j, F.counts[f],
               J.infos[j].best_votes);
      return LSQR_ERR_HIP;
    }
  }
  return LSQR_OK;
}

// The end of a RANSAC job: finish_ransac's outputs of every finishing problem from its final fit F.outs[f], whose
// lm_info / lm_nfev / pad go to fit.lm_info / lm_nfev / reserved (the caller has set what its solve does not write);
// P parameters per problem; a failed fit is EMPTY with fit.n_params 0.  The problems without a winner have no
// consensus set: their bytes are zeroed.
inline void many_end(ManyJob &J, const ManyFinish &F, int P) {
  std::vector<uint8_t> has_mask(J.n, 0);
  for (size_t f = 0; f < F.size(); f++) {
    const uint32_t j = F.fin[f];
    const SolveOut &o = F.outs[f];
    lsqr_ransac_info &info = J.infos[j];
    has_mask[j] = 1;
    info.fit.n_params = o.ok ? o.n_params : 0;
    info.fit.lm_info = o.lm_info;
    info.fit.lm_nfev = o.lm_nfev;
    info.fit.reserved = o.pad;
    info.fit.n_used = F.counts[f];
    info.fit.cost = o.cost;
    if (!o.ok) {
      J.status_out[j] = LSQR_EMPTY;
      continue;
    }
    info.n_params = o.n_params;
    for (int k = 0; k < P; k++) J.params_out[(size_t)j * P + k] = o.params[k];
    J.status_out[j] = LSQR_OK;
  }
  if (J.consensus_out)
    for (size_t j = 0; j < J.n; j++)
      if (!has_mask[j] && J.offsets[j + 1] > J.offsets[j])
        memset(J.consensus_out + J.offsets[j], 0, J.offsets[j + 1] - J.offsets[j]);
}

// The plan of a *_fit_many job: set j = records [offsets[j], offsets[j+1]) where masks (nullable: every record) is
// set.  sets / used: the sets with something to fit and their records in use; a set with none has status ERR_INVALID
// and its outputs untouched.  With a set to fit, the records go up, and the masks to B.d_mask.
inline int many_fit_begin(ManyJob &J, int W, const uint8_t *masks, std::vector<uint32_t> &sets,
                          std::vector<uint64_t> &used) {
  ManyBufs &B = *J.buf;
  const uint64_t NT = J.offsets[J.n];
  int st;
  if ((st = many_check_width(J, W)) != LSQR_OK) return st;
  for (size_t j = 0; j < J.n; j++) {
    const uint64_t r0 = J.offsets[j], r1 = J.offsets[j + 1];
    uint64_t cnt = r1 - r0;
    if (masks) {
      cnt = 0;
      for (uint64_t i = r0; i < r1; i++) cnt += masks[i] != 0;
    }
    if (cnt == 0) {
      J.status_out[j] = LSQR_ERR_INVALID;
      continue;
    }
    sets.push_back((uint32_t)j);
    used.push_back(cnt);
  }
  if (sets.empty()) return LSQR_OK;
  if ((st = many_upload(J)) != LSQR_OK) return st;
  if (masks) {
    MANYCHK(many_grow(B.d_mask, NT));
    MANYCHK(hipMemcpyAsync(B.d_mask, masks, NT, hipMemcpyHostToDevice, J.stream));
  }
  return LSQR_OK;
}

// The end of a *_fit_many job: the lsqr_fit_info, status and parameters (P per set) of the fitted sets from their fits
// outs[q] (lm_info / lm_nfev / pad as in many_end).  n_params is the solver's even where the fit failed; a failed fit
// is EMPTY and hands out no parameters (lsqr_lm_step, lsqr_ls_fit).
inline void many_write_fits(ManyJob &J, lsqr_fit_info *fits, int P, const std::vector<uint32_t> &sets,
                            const std::vector<uint64_t> &used, const std::vector<SolveOut> &outs) {
  for (size_t q = 0; q < sets.size(); q++) {
    const uint32_t j = sets[q];
    const SolveOut &o = outs[q];
    lsqr_fit_info &fi = fits[j];
    memset(&fi, 0, sizeof fi);
    fi.n_params = o.n_params;
    fi.lm_info = o.lm_info;
    fi.lm_nfev = o.lm_nfev;
    fi.reserved = o.pad;
    fi.n_used = used[q];
    fi.cost = o.cost;
    if (!o.ok) {
      J.status_out[j] = LSQR_EMPTY;
      continue;
    }
    for (int k = 0; k < o.n_params; k++) J.params_out[(size_t)j * P + k] = o.params[k];
    J.status_out[j] = LSQR_OK;
  }
}

// The LM stage's job over J's upload: the mask (nullable: every record) and the starts (x0_stride doubles apart), both
// on the device.  A finished LM problem is read as the SolveOut of the shared frame (pad: the stall diagnostic).
inline ManyLmJob many_lm_job(ManyJob &J, const uint8_t *d_mask, const double *d_x0, size_t x0_stride) {
  return ManyLmJob{J.stream, J.buf->d_data, d_mask,    d_x0,      x0_stride, J.lm_n,
                   J.lm_maxfev, J.lm_ftol,    J.lm_xtol, J.lm_gtol, &J.buf->lm, J.err};
}
inline SolveOut many_lm_solve_out(const ManyLmOut &r) {
  SolveOut o = {};
  o.ok = r.ok;
  o.n_params = r.n_params;
  o.lm_info = r.lm_info;
  o.lm_nfev = r.lm_nfev;
  o.pad = r.stall;
  o.cost = r.cost;
  for (int k = 0; k < LM_NMAX; k++) o.params[k] = r.params[k];
  return o;
}

// The finish of a RANSAC job of the closed-form models, after the rounds have left every winner's scan row in
// B.d_best and its votes and index in pr: finish_ransac for every problem with a winner (many_plan_finish .. many_end),
// and the LM stage for the geometric sphere.  org(j, q): the record of problem j's fit origin (read where
// fit_origin_offset is negative: the first record of the winning minimal subset).  Shared by many_run and the
// exhaustive search (many_exhaustive.h).
template <class M, class Org>
int many_finish(ManyJob &J, const std::vector<ManyProb> &pr, Org &&org) {
  constexpr int K = M::K, P = M::P;
  const int W = many_width<M>(J.W);
  ManyBufs &B = *J.buf;
  const int org_off = fit_origin_offset<M>(J.cfg);
  static_assert(M::NMOM <= 64, "one lane per moment in k_many_solve");
  int st0;
  ManyFinish F = many_plan_finish(J, pr, K, org);
  const size_t NF = F.size();
  if (NF) {
    if ((st0 = many_stage_finish(J, F, true)) != LSQR_OK) return st0;
    MANYCHK(many_grow(B.d_partials, F.parts.size() * M::NMOM));
    MANYCHK(many_grow(B.d_mask, J.offsets[J.n]));
    hipLaunchKernelGGL((k_many_mask_moments<M>), dim3((unsigned)F.parts.size()), dim3(kBlock), 0, J.stream, B.d_data,
                       W, B.d_parts, B.d_best, org_off, J.mc, B.d_mask, B.d_counts, B.d_partials);
    MANYCHK(hipGetLastError());
    hipLaunchKernelGGL((k_many_solve<M>), dim3((unsigned)NF), dim3(64), 0, J.stream, B.d_data, W, B.d_parts,
                       B.d_partials, B.d_pbeg, B.d_fin, B.d_best, org_off, J.mc, B.d_out);
    MANYCHK(hipGetLastError());
  }
  if ((st0 = many_fetch_finish(J, F, true)) != LSQR_OK) return st0;
  for (SolveOut &o : F.outs) o.lm_info = o.lm_nfev = o.pad = 0;  // a closed-form fit's (solve_small writes no pad)
  // lsqr_ransac_many_lm: the LM fit of every consensus set whose algebraic fit succeeded, started there (run_fit:
  // Sphere...hxx:231-232 -- a failed algebraic fit is the empty result); its result replaces the algebraic one
  // (finish_ransac after run_fit's LM branch)
  if constexpr (requires { M::NMOM_LM; }) {
    if (J.lm) {
      std::vector<ManyLmProb> lp;
      for (size_t f = 0; f < NF; f++) {
        const uint32_t j = F.fin[f];
        if (F.outs[f].ok)
          lp.push_back(ManyLmProb{J.offsets[j], J.offsets[j + 1] - J.offsets[j], 0, F.counts[f], (uint32_t)f, 0});
      }
      ManyLmJob L = many_lm_job(J, B.d_mask, (const double *)((const char *)B.d_out.get() + offsetof(SolveOut, params)),
                                sizeof(SolveOut) / sizeof(double));
      std::vector<ManyLmOut> res;
      if ((st0 = many_lm_run<M>(L, lp, res)) != LSQR_OK) return st0;
      for (size_t q = 0; q < lp.size(); q++) F.outs[lp[q].xsrc] = many_lm_solve_out(res[q]);
    }
  }
  many_end(J, F, P);
  return LSQR_OK;
}

template <class M>
int many_run(ManyJob &J) {
  constexpr int K = M::K, SP = M::SP;
  const int W = many_width<M>(J.W);
  ManyBufs &B = *J.buf;
  const int org_off = fit_origin_offset<M>(J.cfg);
  int st0;
  if (J.round_cap == 0) J.round_cap = kManyRoundDefault;
  std::vector<ManyProb> pr;
  if ((st0 = many_begin(J, W, K, SP, pr)) != LSQR_OK) return st0;

  if ((st0 = many_rounds(J, pr, K, SP, kManySeg, [&](size_t n_items, uint64_t Ht, size_t n_tiles) -> int {
         hipLaunchKernelGGL((k_many_sample_estimate<M>), dim3((unsigned)((Ht + kBlock - 1) / kBlock)), dim3(kBlock),
                            0, J.stream, B.d_data, W, B.d_items, (int)n_items, (uint32_t)Ht, J.mc, B.d_hparams,
                            B.d_valid);
         MANYCHK(hipGetLastError());
         hipLaunchKernelGGL((k_many_scan<M>), dim3((unsigned)n_tiles), dim3(kManyBlock), 0, J.stream, B.d_data, W,
                            B.d_tiles, B.d_hparams, B.d_valid, J.mc, B.d_votes);
         MANYCHK(hipGetLastError());
         return LSQR_OK;
       })) != LSQR_OK)
    return st0;

  return many_finish<M>(J, pr, [&](size_t j, const ManyProb &q) {
    uint64_t org = J.offsets[j];  // (unused with org_off >= 0)
    if (org_off < 0) {  // the winner's first drawn record, as lsqr_ransac reads it from d_subsets
      uint32_t idx[K], sorted[K];
      ctr_subset(J.seeds[j], q.rs[RS_BEST_IDX], J.offsets[j + 1] - J.offsets[j], K, idx, sorted);
      org += idx[0];
    }
    return org;
  });
}

// lsqr_lm_fit_many: set j = records [offsets[j], offsets[j+1]) where masks (nullable: every record) is set, fitted
// by the LM stage from x0 + j * P; the single-set path's result (lsqr_lm_begin / lsqr_lm_step)
template <class M>
int many_lm_fit(ManyJob &J, const uint8_t *masks, const double *x0, lsqr_fit_info *fits) {
  constexpr int P = M::P;
  ManyBufs &B = *J.buf;
  std::vector<uint32_t> sets;
  std::vector<uint64_t> used;
  int st;
  if ((st = many_fit_begin(J, many_width<M>(J.W), masks, sets, used)) != LSQR_OK || sets.empty()) return st;
  std::vector<ManyLmProb> lp;
  for (size_t q = 0; q < sets.size(); q++) {
    const uint32_t j = sets[q];
    lp.push_back(ManyLmProb{J.offsets[j], J.offsets[j + 1] - J.offsets[j], 0, used[q], j, 0});
  }
  MANYCHK(many_grow(B.d_best, J.n * P));  // the starts (no RANSAC rounds run here)
  MANYCHK(hipMemcpyAsync(B.d_best, x0, sizeof(double) * J.n * P, hipMemcpyHostToDevice, J.stream));
  ManyLmJob L = many_lm_job(J, masks ? B.d_mask : nullptr, B.d_best, P);
  std::vector<ManyLmOut> res;
  if ((st = many_lm_run<M>(L, lp, res)) != LSQR_OK) return st;
  std::vector<SolveOut> outs;
  for (const ManyLmOut &r : res) outs.push_back(many_lm_solve_out(r));
  many_write_fits(J, fits, P, sets, used, outs);
  return LSQR_OK;
}
#endif

}  // namespace lsqr
