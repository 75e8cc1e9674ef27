// lsqr_hip.hip -- C ABI (include/lsqr_hip.h) over the HIP kernels in kernels.h.
// Host code here is plumbing: buffer ownership, launches on the context's stream, the serial
// replay of RANSAC.hxx's adaptive loop over batch results.  No CPU implementation of the scan
// or the fits exists in this library: without a device every entry point fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <set>
#include <thread>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/lsqr_hip.h"
#include "devbuf.h"
#include "options.h"
#include "kernels.h"
#include "models_nd.h"
#include "dense.h"
#include "dense_h16.h"
#include "us_kernels.h"
#include "us_h16.h"
#include "phantom_h16.h"
#include "cells.h"
#include "earlyexit.h"
#include "axis.h"
#include "sort.h"
#include "rigid.h"
#include "phantom.h"
#include "lm_persist.h"
#include "host_entry.h"
#include "many.h"
#include "many_dense.h"
#include "many_exhaustive.h"
#include "sequential.h"
#include "many_sequential.h"
#include "grouped.h"
#include "assign.h"
#include "assign_dense.h"
#include "assign_lm.h"
#include "assign_rigid.h"
#include "assign_grouped.h"
#include "assign_lm_grouped.h"
#include "assign_dense_grouped.h"

#include <condition_variable>
#include <mutex>

#include <dlfcn.h>
#include <rccl/rccl.h>  // types and prototypes only: librccl is dlopen'ed when LSQR_MULTI_TRANSPORT=rccl asks for it

using namespace lsqr;

// ---- the pinned staging buffer (lsqr_ctx::h_pin) ---------------------------------------------------------------
// One 64 KiB allocation per context.  Every area has one user, or users that never overlap in time on a context;
// the members are padded so that each area sits where it always has.
struct BatchSlot {  // lsqr_batch_fit_enqueue -> lsqr_batch_fit_wait
  unsigned long long head[2], pad0[2];  // {inliers, packed winner}
  unsigned long long ovf_fill, pad1[3];  // fullest worklist segment of the slot's scan (deferred overflow check)
  SolveOut out;
  char pad2[2048 - 64 - sizeof(SolveOut)];
};
struct StepSlot {  // lsqr_step_finish_enqueue -> lsqr_step_finish_wait
  unsigned long long packed;
  double count;
  uint8_t valid, pad0[47];
  double winner[64], pad1[128 - 8 - 64];
  SolveOut out;
  char pad2[2048 - 1024 - sizeof(SolveOut)];
};
struct WinnerPin {  // lsqr_winner_moments
  uint8_t valid, pad0[7];
  unsigned long long count;
  double params[64], origin[32];
};
struct PinLayout {
  union {  // general scratch of the blocking entry points: what is staged here is read before the call returns
    char scratch[8192];
    double scratch_f64[1024];
    unsigned long long scratch_u64[1024];
  };
  unsigned long long mask_head[2], pad0[1024 - 2];  // {inliers, packed winner} of a blocking finish: survives run_fit
  WinnerPin winner;
  char pad1[16384 - sizeof(WinnerPin)];
  LmpCtl lmp;  // lm_persist_fit: the persistent kernel's control block after the fit
  char pad2[8192 - sizeof(LmpCtl)];
  double phantom_block[1024];  // the phantom's Gram block of a step (one area: phantom steps are not pipelined)
  BatchSlot batch[2];
  StepSlot step[2];
  double mdev_x[4][64];  // lsqr_moments_dev: staging slots of x
  char pad3[(1 << 16) - 57344 - sizeof(double) * 4 * 64];
};
static_assert(sizeof(PinLayout) == 1 << 16, "h_pin is 64 KiB");
static_assert(std::is_trivially_copyable_v<SolveOut> && std::is_trivially_copyable_v<LmpCtl> &&
              std::is_trivially_copyable_v<BoundsRow>, "staged with memcpy");
static_assert(offsetof(PinLayout, mask_head) == 8192 && offsetof(PinLayout, winner) == 16384 &&
              offsetof(PinLayout, lmp) == 32768 && offsetof(PinLayout, phantom_block) == 40960 &&
              offsetof(PinLayout, batch) == 49152 && offsetof(PinLayout, step) == 53248 &&
              offsetof(PinLayout, mdev_x) == 57344, "areas stay where they were");
static_assert(sizeof(BatchSlot) == 2048 && offsetof(BatchSlot, ovf_fill) == 32 && offsetof(BatchSlot, out) == 64 &&
              sizeof(StepSlot) == 2048 && offsetof(StepSlot, valid) == 16 && offsetof(StepSlot, winner) == 64 &&
              offsetof(StepSlot, out) == 1024 && offsetof(WinnerPin, params) == 16 && offsetof(WinnerPin, origin) == 528);
// the largest things staged in the scratch area: a SolveOut, the bounds row, the LM loop's {x[64] | block}, the
// compacted count behind 200 doubles, and the phantom's Gram block (checked at dense_ne)
static_assert(sizeof(SolveOut) <= 8192 && sizeof(BoundsRow) <= 8192 && sizeof(double) * (64 + LM_MOM_MAX) <= 8192 &&
              sizeof(double) * 201 <= sizeof(PinLayout::scratch));

// The eight words of lsqr_ctx::d_counter.  Two pairs of names share storage; both are safe by stream order:
//   CNT_ABSMAX is a PAIR (words 5 and 6), so its second word is CNT_FIRST.  The absmax pass of an upload or a model
//     change writes the pair and synchronises before it returns; set_fit_origin(ORG_MASK) writes and consumes
//     CNT_FIRST inside one fit, enqueued later on the same stream.
//   CNT_FLAG is shared by halves: the low word is k_plane_order's count (plane scans), the high word the dense
//     solve's double-double flag (dense fits).  A context has one model, and each user sets its half before use.
enum {
  CNT_MASK = 0,    // inliers of the last mask pass
  CNT_BEST = 1,    // k_best's packed winner {votes | ~index}: CNT_MASK and CNT_BEST are read back as one pair
  CNT_SUM = 2,     // lsqr_scan_workload: surviving cells of the selected hypotheses
  CNT_OVF = 3,     // fullest worklist segment of a matrix-core filter
  CNT_PAIRS = 4,   // surviving (cell, hypothesis) pairs of level 1
  CNT_ABSMAX = 5,  // {absmax, absmax_rot}
  CNT_FIRST = 6,   // first masked record
  CNT_FLAG = 7
};

// ---- host-side halves of the pinned slots and of the selection records ---------------------------------------------
struct BatchSlotState {  // of PinLayout::batch[i]: lsqr_batch_fit_enqueue -> lsqr_batch_fit_wait
  bool busy = false;
  uint64_t first = 0, H = 0, seed = 0;  // the batch: for its info, and to run it again without the filter
  uint32_t ovf_cap = 0;   // segment size the deferred worklist check compares BatchSlot::ovf_fill against (0: no worklist)
  int bsel_rec = -1;      // the selection record of the slot's scan (-1: none) ...
  uint64_t bsel_seq = 0;  // ... which is still that scan's while the record's sequence number is this one
  Event ev;
};
struct StepSlotState {  // of PinLayout::step[i]: lsqr_step_finish_enqueue -> lsqr_step_finish_wait
  bool busy = false;
  int bsel_rec = -1;  // the record of the step's scan (lsqr_step_scan), as in BatchSlotState
  uint64_t bsel_seq = 0;
  Event ev;
};
struct BselRecord {  // of one of the two BoundSel of lsqr_ctx::h_bsel
  Event ev;              // the copy into the record
  bool pending = false;  // written by a scan the host has not folded yet
  uint64_t seq = 0;      // that scan's sequence number (lsqr_ctx::bsel_seq) ...
  uint32_t H = 0;        // ... and batch size
};

// ------------------------------------------------------------------------------------------------
struct lsqr_ctx {
  // ---- device, stream, options, model ----
  int device = 0;
  hipStream_t stream = nullptr;      // the stream all work is enqueued on
  hipStream_t own_stream = nullptr;  // created with the context (stream == own_stream unless lsqr_set_stream)
  bool external_stream = false;
  Options opt;  // lsqr_set_option (options.h: every knob, its default and its rule)
  lsqr_model_cfg cfg{};
  ModelConsts mc{};
  bool has_model = false;
  int K = 0, P = 0, ND = 0, HS = 0;  // HS: row stride (doubles) of d_hparams

  // ---- records ----
  const double *d_data = nullptr;  // observations (owned or attached)
  DevBuf<double> d_data_owned;
  size_t n = 0, stride = 0;  // stride in doubles
  uint64_t data_epoch = 1;   // bumped whenever the records or the model change
  bool absmax_valid = false;
  // k_bounds of the current upload (min / max per dimension, max |coordinate|, non-finite count): serves both
  // the fp32 filters' absmax and the Morton grid of the index
  BoundsRow h_bounds{};
  bool bounds_valid = false;
  uint64_t hyp_since_upload = 0;  // hypotheses scanned on this upload (index build heuristic)
  uint64_t hyp_expected = 0;      // hypotheses the caller still expects to scan on this upload (lsqr_ransac: numTries)
  DevBuf<double> d_rows;  // plane phantom: the data rows a_i as an n x 32 matrix (phantom.h)
  bool rows_valid = false;
  // staged upload (lsqr_upload of large pageable buffers): ring of pinned chunks filled by a few host threads
  // while earlier chunks are in flight to the device
  static constexpr int kUpSlots = 8;
  static constexpr size_t kUpChunk = (size_t)8 << 20;
  PinBuf<char> h_up[kUpSlots];
  Event up_ev[kUpSlots];
  double last_upload_ms = 0.0;

  // ---- hypotheses ----
  size_t H = 0, H_cap = 0;
  DevBuf<uint32_t> d_subsets;
  DevBuf<double> d_hparams;
  DevBuf<float> d_hparams_f32;
  DevBuf<uint8_t> d_valid;
  DevBuf<uint32_t> d_votes;
  DevBuf<uint8_t> d_refused;  // k_estimate_phantom_lu: hypotheses left to the Jacobi kernel
  bool scanned = false;

  // ---- spatial index of the point models (cells.h): Morton-sorted copy + one fp32 box per 128 records ----
  DevBuf<double> d_sorted;
  DevBuf<uint32_t> d_queues;  // work-queue counters of k_scan_cells
  DevBuf<CellBox> d_boxes;   // [n_cells cell boxes | merged boxes of the bounds pass (k_super_boxes)]
  uint32_t super_merge = 0;     // cells per merged box the second part currently holds (0: not built)
  size_t n_sorted = 0;      // finite records (non-finite ones never agree and are left out)
  uint32_t n_cells = 0, cell_pts = 0;
  bool index_valid = false;
  bool index_failed = false;  // build failed on this upload: stay on the exhaustive kernels
  DevBuf<char> d_idx_scratch;  // keys / permutation / radix-sort temporaries of the index build (kept)
  int kd_build_levels = 0, index_kd_levels = 0;  // k-d levels of the build in progress / of the index in place
  // axis-sorted cells (axis.h; plane, 3-D): per-cell axis, the cells' sorted projections
  DevBuf<CellAxis> d_axis;
  DevBuf<float> d_cellT;
  bool axis_valid = false;
  DevBuf<CellSlab> d_slab;        // per-cell oriented slab (axis.h: k_cell_slabs), built with d_axis
  // fp32 tiles of the index (cells.h: k_build_tiles): what cells_load makes of every cell, built once behind the index
  DevBuf<float> d_tiles;
  uint32_t tiles_pts = 0;    // cell size the tiles in place were built for (0: none; dropped with the index)
  bool tiles_nomem = false;  // no room for the tiles on this upload: the scans keep reading the sorted copy
  // option "scan_tiles" (1: build and read the tiles).  Kept here and not in options.h: it keeps the index and is
  // handed on to the lanes like a row of the table (apply_option)
  bool use_tiles = true;

  // ---- two-level scan and its counted forms ----
  DevBuf<uint32_t> d_ub;  // per-hypothesis vote bound of the two-level scan's first level (k_cells_bounds)
  // the table of the last counting launch of run_scan_pairs (lsqr_scan_pairs_counted)
  struct {
    bool valid = false, packed = false, slab = false;
    uint32_t H = 0, h_off = 0, gstride = 0;
    const uint32_t *h_dev = nullptr;
  } last_count;
  DevBuf<uint8_t> d_paircnt;   // k_scan_pairs: survivors per (cell, group of 64 hypotheses)
  DevBuf<uint32_t> d_paircost; // [n_cells cell costs | chunk sums]
  DevBuf<uint32_t> d_vpart;    // per-workgroup partial votes of k_scan_pairs
  DevBuf<float4> d_hyps;       // k_prepare_hyps: CM::Hyp of every hypothesis of the batch k_scan_pairs is counting
  DevBuf<unsigned long long> d_pairmask;  // PairsForm::Packed: level 1's survivor mask per (cell, group of 64 hypotheses)
  DevBuf<unsigned long long> d_ambcnt;  // k_scan_pairs: kAmbSlots x {ambiguous pairs, band observations} of the last scan
  bool amb_reset = false;         // the next k_tile_costs zeroes d_ambcnt: the scan's first k_scan_pairs
  bool amb_counted = false;       // the last scan went through k_scan_pairs: d_ambcnt holds its counts

  // ---- bounded scan (cells.h: k_pick_*): the selected hypotheses as a compact batch ----
  DevBuf<uint32_t> d_sel;        // [kPilots pilots | H_cap rest]
  DevBuf<BoundSel> d_bsel;
  DevBuf<double> d_hparams2;
  DevBuf<float> d_hparams2_f32;
  DevBuf<uint32_t> d_votes2;     // [kPilots | H_cap]
  DevBuf<uint32_t> d_ub2;  // rank bounds: [upper | lower] of the candidates (compact order) | lower per hypothesis
  uint32_t best_before = 0;         // exact votes of the best hypothesis of earlier batches (lsqr_ransac)
  bool allow_bound = false;         // set by the batch entry points around run_scan (lsqr_scan always counts all)
  uint64_t last_bound[4] = {0, 0, 0, 0};  // diagnostics of the last bounded scan: {used, pilots, rest, H}
  bool merge_off = false;       // this upload: merged boxes let too many hypotheses through, bounds stay on the cells
  // Selection counts of the bounded scans come back through pinned memory and steer the NEXT batches' launch sequence
  // (merged boxes or cells; pilot pass or not).  Two records, written alternately; a record is folded into
  // `bsel_known` only at a point where the host HAS synchronised with the batch that wrote it -- a ..._wait of its
  // slot, the end of a blocking entry point, or right before the record is reused (two bounded scans later) -- so the
  // launch sequence of a batch follows from the call sequence, never from host / device timing.
  PinBuf<BoundSel> h_bsel;   // pinned [2], 64 B apart
  BselRecord bsel[2];
  uint64_t bsel_seq = 0;        // bounded scans issued on this context
  int bsel_last_rec = -1;       // record the last bounded scan writes
  BoundSel bsel_known{};        // counts of the latest bounded scan the host has synchronised with ...
  uint32_t bsel_known_H = 0;    // ... its batch size (0: nothing known on this upload / model) ...
  uint64_t bsel_known_seq = 0;  // ... and its sequence number

  // ---- matrix-core filters of the dense / US / phantom scans ----
  DevBuf<unsigned long long> d_amb;  // worklist of the dense MFMA filter
  unsigned dense_amb_max = 0;  // fullest worklist segment of the last fp32 dense scan (diagnostics)
  // dense_h16.h: the rows as fp16 fragment pairs (8 KiB per 32 rows) + the scaled right-hand sides, once per upload
  DevBuf<uint4> d_h16;
  DevBuf<float> d_h16_bs;
  bool h16_valid = false, h16_attr = false, h16_nomem = false;  // nomem: no room for the fragments on this upload
  int h16_unit = 0;       // 0: this device's matrix unit not probed yet, 1: keeps dense_h16.h's accumulation assumption, -1: not
  double h16_unit_dev = 0.0;  // the probe's worst deviation (u of the sum of magnitudes)
  double h16_pa = 1.0;
  DevBuf<float> d_h16_thr;  // (-a, band, -ph, 0) per hypothesis of the batch
  // us_h16.h: the frames as fp16 fragment pairs (6 KiB per 32 frames), once per upload; the batch's hypothesis fragments
  DevBuf<uint4> d_us16, d_us16_x;
  bool us16_valid = false, us16_attr = false, us16_nomem = false;
  Us16Scales us16_sc{};
  // chunked early exit of the dense / US scans (earlyexit.h)
  DevBuf<char> d_ee;             // [EeState | sel_c | sel_o x 2 | compact thresholds | compact fp32 rows]
  PinBuf<EeState> h_ee;          // pinned copy of the last early-exit scan's state (diagnostics: read after a synchronisation, lsqr_scan_work)
  bool ee_last = false;             // the last scan of this context took the early-exit path
  uint64_t ee_H = 0, ee_n = 0;      // its batch size and observation count
  // The filters decide their band from per-workgroup worklists; a segment that overflowed (never seen) means "scan
  // again without the filter".  The blocking entry points read the fill right after the scan (one host
  // synchronisation); lsqr_batch_fit_enqueue must not wait, so there the scan only notes the segment size (ovf_cap),
  // the fill travels with the slot's pinned record and lsqr_batch_fit_wait runs the batch again without the filter if
  // it ever exceeds it.
  bool defer_ovf = false;        // set around run_scan_batch by lsqr_batch_fit_enqueue
  uint32_t ovf_cap = 0;          // segment size the deferred check compares against (0: this scan has no worklist)
  uint64_t ovf_reruns = 0;       // batches run again because a worklist segment overflowed (diagnostics)

  // ---- lanes and slots ----
  // lsqr_batch_fit_enqueue / _wait run on LANES: independent contexts on the same device, each with its own stream
  // and buffers, attached to this context's records.  Batches of different lanes overlap on the device: the dozen
  // one-workgroup kernels of a batch (selection, winner, solve) and the tails of the big ones no longer leave the
  // chip idle (measured, plane 10 M x 4096: 0.72 ms per batch on one lane, 0.56 on two, 0.51 on three).
  // Lane 0 is this context itself.
  static constexpr int kMaxLanes = 4;
  lsqr_ctx *lanes[kMaxLanes] = {nullptr, nullptr, nullptr, nullptr};
  bool is_lane = false;
  uint64_t lane_epoch = 0;   // (lanes) the epoch of the parent this lane is attached to
  BatchSlotState slots[2];   // lsqr_batch_fit_enqueue / _wait
  StepSlotState steps[2];    // lsqr_step_finish_enqueue / _wait
  Event mdev_ev[4];  // lsqr_moments_dev: staging slots of x
  unsigned mdev_next = 0;

  // ---- fit: mask, moments, solve ----
  DevBuf<uint8_t> d_mask;
  bool mask_valid = false;
  DevBuf<double> d_partials;  // kMaxPartials * MOM_MAX
  DevBuf<double> d_mom;       // MOM_MAX
  DevBuf<double> d_vec;       // 32 doubles: origin / parameter vector handed to kernels
  DevBuf<double> d_par;       // 32 doubles: model parameters for mask/stats
  DevBuf<double> d_best;      // scan-parameter row of the best hypothesis so far (lsqr_ransac*)
  DevBuf<SolveOut> d_out;
  DevBuf<unsigned long long> d_counter;  // CNT_* words
  bool origin_valid = false;  // d_par holds the parameters the device mask was made from (set_fit_origin)
  uint64_t win_rec = 0;       // first drawn record of the winning minimal subset (lsqr_ransac*, set_fit_origin)
  DevBuf<double> d_ddpart;  // partial double-double Gram blocks of k_gram_dd_dense (allocated on first use)
  PinBuf<PinLayout> h_pin;  // pinned staging
  PinBuf<char> h_batch;  // pinned results of a lsqr_ransac batch (grown on demand)
  std::unique_ptr<ManyBufs> many;  // lsqr_ransac_many's buffers (its own: the context's upload is not touched)
  std::unique_ptr<AssignBufs> assign;  // lsqr_assign / lsqr_refine / lsqr_refine_lm (assign.h, assign_lm.h)
  std::unique_ptr<AssignDenseBufs> assign_dense;  // lsqr_assign_dense / lsqr_refine_dense (assign_dense.h)
  // lsqr_assign_grouped / lsqr_refine_grouped / lsqr_refine_lm_grouped (assign_grouped.h, assign_lm_grouped.h)
  std::unique_ptr<AssignGrpBufs> assign_grp;
  // what lsqr_assign_dense_grouped / lsqr_refine_dense_grouped hold beside it (assign_dense_grouped.h)
  std::unique_ptr<AssignDenseGrpBufs> assign_dense_grp;
  // lsqr_ransac_sequential (sequential.h): the survivors of a round go from the current buffer into the OTHER of two
  // owned buffers (never into the caller's upload), their upload indices beside them; labels in upload order
  DevBuf<double> d_seq_rec[2];
  DevBuf<uint32_t> d_seq_orig[2];
  DevBuf<int32_t> d_seq_labels;
  DevBuf<uint32_t> d_seq_counts;

  // ---- iterative (LM) fits ----
  DevBuf<LmState> d_lm;
  LmState h_lm;  // host copy of the LM state (opt.lm_host)
  DevBuf<double> d_lmrec;  // consensus set copied tight and in order for the iterative fits (k_compact_*)
  PinBufCoherent<unsigned long long> h_lmres;  // pinned, device-visible: tagged granules written by k_lm_publish
  uint32_t lm_seq = 0;        // sequence number of the last evaluation (the tag the host polls for)
  // lm_persist.h: a whole matrix-core LM fit in one launch (opt.lm_persist)
  DevBuf<LmpCtl> d_lmp;
  PinBufCoherent<unsigned long long> h_lmcmd;  // pinned, device-visible: the host's reply (coefficient granules + command)
  bool counted = false;  // this context counts among the device's root contexts (lmp_pool: the share of a persistent fit)
  // diagnostics of the last persistent fit: {mode, G, evaluations, status, kernel us, fallbacks, host ns waiting, host ns stepping}
  uint64_t lmp_last[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t lmp_trace[LMP_TRACE][4];
  uint32_t lmp_trace_n = 0;

  // ---- profiling ----
  bool prof = false;
  Event ev0, ev1;
  // HIP-event pairs of profiled launches; resolved lazily (lsqr_profile_get) so that profiling
  // adds no host synchronisation between kernels
  std::vector<Event> ev_pool;
  std::vector<std::pair<int, int>> ev_pending;  // (kernel id, pair index)
  int ev_next = 0;
  uint64_t launches[8] = {0};
  double ms[8] = {0};

  char err[512] = {0};
};

namespace {

enum { KID_SAMPLE = 0, KID_ESTIMATE = 1, KID_SCAN = 2, KID_MASK = 3, KID_MOMENTS = 4, KID_SOLVE = 5,
       KID_INDEX = 6, KID_ABSMAX = 7 };

int fail(lsqr_ctx *c, int status, const char *fmt, ...) {
  if (c) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(c->err, sizeof c->err, fmt, ap);
    va_end(ap);
  }
  return status;
}

#define HIPCHK(c, call)                                                                   \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail((c), LSQR_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                  __FILE__, __LINE__);                                                    \
  } while (0)

void prof_flush(lsqr_ctx *c) {
  for (auto &pe : c->ev_pending) {
    float t = 0;
    hipEvent_t e0 = c->ev_pool[2 * pe.second], e1 = c->ev_pool[2 * pe.second + 1];
    if (hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&t, e0, e1) == hipSuccess) {
      c->launches[pe.first]++;
      c->ms[pe.first] += t;
    }
  }
  c->ev_pending.clear();
  c->ev_next = 0;
}

struct ProfScope {
  lsqr_ctx *c;
  int id, pair = -1;
  ProfScope(lsqr_ctx *c, int id) : c(c), id(id) {
    if (!c->prof) return;
    constexpr int kPairs = 512;
    if (c->ev_next >= kPairs) prof_flush(c);
    if ((int)c->ev_pool.size() < 2 * (c->ev_next + 1)) {
      Event a, b;
      if (a.create() != hipSuccess || b.create() != hipSuccess) return;
      c->ev_pool.push_back(std::move(a));
      c->ev_pool.push_back(std::move(b));
    }
    pair = c->ev_next++;
    (void)hipEventRecord(c->ev_pool[2 * pair], c->stream);
  }
  ~ProfScope() {
    if (pair < 0) return;
    (void)hipEventRecord(c->ev_pool[2 * pair + 1], c->stream);
    c->ev_pending.push_back({id, pair});
  }
};
// no scopes of their own for the launches below one "whole" ProfScope (restored when the guard goes)
struct ProfMute {
  lsqr_ctx *c;
  bool was;
  explicit ProfMute(lsqr_ctx *c) : c(c), was(c->prof) { c->prof = false; }
  ~ProfMute() { c->prof = was; }
};

size_t dense_lds_bytes(int n) { return sizeof(double) * ((size_t)2 * n * (n | 1) + 3 * n); }
constexpr int dense_ne(int n) { return (n + 1) * (n + 2) / 2; }
// the phantom's Gram block (30 columns + right-hand side, and the count) fits its own area and the scratch area
static_assert(sizeof(double) * (dense_ne(30) + 1) <= sizeof(PinLayout::phantom_block) &&
              sizeof(double) * (dense_ne(30) + 1) <= sizeof(PinLayout::scratch));
constexpr int kDenseBlocks = 256;
constexpr size_t kPartialsBytes = sizeof(double) * 2 * kDenseBlocks * 2160;  // lsqr_ctx::d_partials
int dense_pstride(int n) { return (dense_ne(n) + 1 + 7) & ~7; }

template <class T>
int ensure(lsqr_ctx *c, DevBuf<T> &buf, size_t need) {
  if (const size_t ncap = grow_double(buf, need)) HIPCHK(c, buf.alloc(ncap));
  return LSQR_OK;
}

int ensure_hyp(lsqr_ctx *c, size_t H) {
  if (H <= c->H_cap) return LSQR_OK;
  size_t cap = std::max<size_t>(H, 4096);
  c->H_cap = 0;
  // everything goes before anything comes back: the old and the new batch never have to fit side by side
  c->d_subsets.reset(), c->d_hparams.reset(), c->d_hparams_f32.reset(), c->d_valid.reset(), c->d_votes.reset();
  c->d_ub.reset(), c->d_sel.reset(), c->d_bsel.reset(), c->d_hparams2.reset(), c->d_hparams2_f32.reset();
  c->d_votes2.reset();
  c->d_ub2.reset();  // (allocated by the first bounded scan with rank bounds, sized from H_cap)
  HIPCHK(c, c->d_subsets.alloc(cap * 64));
  HIPCHK(c, c->d_hparams.alloc(cap * 64));
  HIPCHK(c, c->d_hparams_f32.alloc(cap * 32));  // M::SPF <= 32
  HIPCHK(c, c->d_valid.alloc(cap));
  HIPCHK(c, c->d_votes.alloc(cap));
  HIPCHK(c, c->d_ub.alloc(cap));
  HIPCHK(c, c->d_sel.alloc(cap + kPilots));
  HIPCHK(c, c->d_bsel.alloc(1));
  HIPCHK(c, c->d_hparams2.alloc((cap + kPilots) * 64));
  HIPCHK(c, c->d_hparams2_f32.alloc((cap + kPilots) * 32));
  HIPCHK(c, c->d_votes2.alloc(cap + kPilots));
  c->H_cap = cap;
  return LSQR_OK;
}

int need_ready(lsqr_ctx *c, bool need_data) {
  if (!c) return LSQR_ERR_INVALID;
  if (!c->has_model) return fail(c, LSQR_ERR_STATE, "lsqr_set_model has not been called");
  if (need_data && (!c->d_data || c->n == 0))
    return fail(c, LSQR_ERR_STATE, "no observations uploaded");
  HIPCHK(c, hipSetDevice(c->device));
  return LSQR_OK;
}

// smallest chunk per block of the mask / moment passes (kernels.h: kMomChunk)
static inline int mom_chunk(const lsqr_ctx *c) {
  if (c->opt.mom_chunk > 0) return c->opt.mom_chunk * kBlock;
  const int m = c->cfg.model;
  return (m == LSQR_MODEL_US_SINGLE || m == LSQR_MODEL_US_POINTER || m == LSQR_MODEL_PHANTOM) ? kMomChunkWide : kMomChunk;
}

// ---- hypotheses ---------------------------------------------------------------------------------
template <int D>
int run_bounds(lsqr_ctx *c);

// ---- selection feedback of the bounded scan (see lsqr_ctx::h_bsel) ----------------------------------------------
static BoundSel *bsel_rec(lsqr_ctx *c, int r) { return (BoundSel *)((char *)c->h_bsel.get() + 64 * r); }
// the host has synchronised with the batch that wrote record r
static void bsel_fold(lsqr_ctx *c, int r) {
  if (r < 0 || !c->h_bsel || !c->bsel[r].pending) return;
  BselRecord &b = c->bsel[r];
  b.pending = false;
  if (c->bsel_known_H && b.seq < c->bsel_known_seq) return;  // an older batch than the one known
  c->bsel_known = *bsel_rec(c, r);
  c->bsel_known_H = b.H;
  c->bsel_known_seq = b.seq;
}
// the host has synchronised with everything enqueued on the context's stream
static void bsel_host_synced(lsqr_ctx *c) {
  if (!c->h_bsel) return;
  const int first = c->bsel[0].seq <= c->bsel[1].seq ? 0 : 1;
  bsel_fold(c, first);
  bsel_fold(c, first ^ 1);
}
// new records / new model: nothing is known; copies still in flight are waited for, not abandoned
static void bsel_reset(lsqr_ctx *c) {
  for (BselRecord &b : c->bsel)
    if (b.pending && b.ev) {
      (void)hipEventSynchronize(b.ev);
      b.pending = false;
    }
  c->bsel_known = BoundSel{};
  c->bsel_known_H = 0;
  for (int s = 0; s < 2; s++) c->slots[s].bsel_rec = c->steps[s].bsel_rec = -1;
  c->bsel_last_rec = -1;
}

// the host waits for everything enqueued on the context's stream: also the point where the selection feedback folds
static hipError_t sync_stream(lsqr_ctx *c) {
  hipError_t e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) bsel_host_synced(c);
  return e;
}

int ensure_absmax(lsqr_ctx *c) {
  if (c->absmax_valid) return LSQR_OK;
  const int m = c->cfg.model;
  if ((m == LSQR_MODEL_PLANE || m == LSQR_MODEL_SPHERE || m == LSQR_MODEL_LINE || m == LSQR_MODEL_LINE2D) &&
      c->ND <= 3) {
    // point models: one pass gives max |coordinate| AND the bounds the index build needs (cells.h: k_bounds; the
    // profile scope is around the kernel itself in run_bounds: r03 timed the final reduction, the copy back and the
    // synchronisation with it and reported 67 us for a 45 us pass)
    int st = c->ND == 3 ? run_bounds<3>(c) : run_bounds<2>(c);
    if (st != LSQR_OK) return st;
    double am;
    memcpy(&am, &c->h_bounds.amax, sizeof am);
    if (c->h_bounds.nonfinite) am = std::numeric_limits<double>::infinity();  // as k_absmax: switches the filters off
    c->mc.absmax = am;
    c->mc.absmax_rot = am;
    c->absmax_valid = true;
    return LSQR_OK;
  }
  HIPCHK(c, hipMemsetAsync(c->d_counter + CNT_ABSMAX, 0, 2 * sizeof(unsigned long long), c->stream));
  int grid = grid_for(c->n, kBlock * 16, 1024);
  const bool us = c->cfg.model == LSQR_MODEL_US_SINGLE || c->cfg.model == LSQR_MODEL_US_POINTER ||
                  c->cfg.model == LSQR_MODEL_PHANTOM;  // Frame records: int slot 12, rotation first
  {
    ProfScope ps(c, KID_ABSMAX);
    hipLaunchKernelGGL(k_absmax, dim3(grid), dim3(kBlock), 0, c->stream, c->d_data, c->stride, c->n,
                       c->ND, us ? 12 : -1, us ? 9 : (c->cfg.model == LSQR_MODEL_DENSE ? c->ND - 1 : c->ND),
                       c->d_counter + CNT_ABSMAX);  // dense: the coefficient columns separately from the right-hand side
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipMemcpyAsync(c->h_pin->scratch, c->d_counter + CNT_ABSMAX, 2 * sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, sync_stream(c));
  memcpy(&c->mc.absmax, c->h_pin->scratch, sizeof(double));
  memcpy(&c->mc.absmax_rot, c->h_pin->scratch + 8, sizeof(double));
  c->absmax_valid = true;
  return LSQR_OK;
}

int run_estimate(lsqr_ctx *c) {
  return dispatch(c->cfg, [&](auto tag) -> int {
    typedef typename decltype(tag)::type M;
    if constexpr (requires { M::SPF; } || M::IS_US) {
      int st = ensure_absmax(c);
      if (st != LSQR_OK) return st;
    }
    ProfScope ps(c, KID_ESTIMATE);
    if constexpr (requires { M::IS_PHANTOM; }) {
      // one wave per hypothesis (measured 1.76 ms per 4096 against 1.96 / 2.53 ms with 128 / 256 threads:
      // the sweeps are bound by instruction issue, and a single-wave workgroup lands on any SIMD)
      if (c->opt.phantom_fast) {
        // r05: LU + inverse iteration (phantom.h: k_estimate_phantom_lu), the Jacobi SVD for what it refuses
        int st = ensure(c, c->d_refused, std::max<size_t>(c->H, 1));
        if (st != LSQR_OK) return st;
        uint8_t *d_ref = c->d_refused;
        static const bool dbg_on = getenv("LSQR_PHANTOM_DEBUG") != nullptr;
        DevBuf<unsigned long long> d_dbg;
        if (dbg_on) (void)d_dbg.alloc(4 * c->H);
        hipLaunchKernelGGL(k_estimate_phantom_lu, dim3((unsigned)((c->H + 3) / 4)), dim3(256), 0, c->stream, c->d_data,
                           c->stride, c->n, c->d_subsets, (uint32_t)c->H, c->d_hparams, c->d_valid, d_ref,
                           c->opt.phantom_fast > 1 ? c->opt.phantom_fast : 96, d_dbg);
        if (d_dbg) {  // diagnostics (LSQR_PHANTOM_DEBUG): iterations and 10-ns ticks per phase and hypothesis
          std::vector<unsigned long long> hd(4 * c->H);
          (void)hipStreamSynchronize(c->stream);
          (void)hipMemcpy(hd.data(), d_dbg, hd.size() * 8, hipMemcpyDeviceToHost);
          double sit = 0, slu = 0, sitr = 0, sfin = 0, mit = 0, mitr = 0, spcg = 0, mpcg = 0;
          size_t nref = 0, nconv = 0;
          for (size_t h = 0; h < c->H; h++) {
            const double it = (double)(hd[4 * h] & 0xFFFFFFFFu);
            sit += it, slu += (double)hd[4 * h + 1], sitr += (double)hd[4 * h + 2], sfin += (double)hd[4 * h + 3];
            mit = std::max(mit, it), mitr = std::max(mitr, (double)hd[4 * h + 2]);
            spcg += (double)((hd[4 * h] >> 40) & 0xFF), mpcg = std::max(mpcg, (double)((hd[4 * h] >> 40) & 0xFF));
            nref += (hd[4 * h] >> 32) & 1, nconv += (hd[4 * h] >> 33) & 1;
          }
          fprintf(stderr, "phantom_lu: H %zu mean it %.1f max %.0f, correction steps mean %.2f max %.0f, refused %zu converged %zu; mean us: setup+LU %.1f iter %.1f (max %.1f) finish %.1f\n",
                  c->H, sit / c->H, mit, spcg / c->H, mpcg, nref, nconv, slu / c->H / 100, sitr / c->H / 100, mitr / 100, sfin / c->H / 100);
        }
        hipLaunchKernelGGL(k_estimate_phantom<64>, dim3((unsigned)std::min<size_t>(c->H, 512)), dim3(64), 0, c->stream,
                           c->d_data, c->stride, c->n, c->d_subsets, (uint32_t)c->H, c->d_hparams, c->d_valid,
                           (const uint8_t *)d_ref);
      } else if (c->opt.block == 256)
        hipLaunchKernelGGL(k_estimate_phantom<256>, dim3((unsigned)c->H), dim3(256), 0, c->stream, c->d_data,
                           c->stride, c->n, c->d_subsets, (uint32_t)c->H, c->d_hparams, c->d_valid, (const uint8_t *)nullptr);
      else
        hipLaunchKernelGGL(k_estimate_phantom<64>, dim3((unsigned)c->H), dim3(64), 0, c->stream, c->d_data,
                           c->stride, c->n, c->d_subsets, (uint32_t)c->H, c->d_hparams, c->d_valid, (const uint8_t *)nullptr);
      hipLaunchKernelGGL((k_prepare_f32_us<M>), dim3((unsigned)((c->H + 255) / 256)), dim3(256), 0,
                         c->stream, c->d_hparams, (uint32_t)c->H, c->mc, c->d_hparams_f32);
    } else if constexpr (M::IS_DENSE) {
      const int n = (int)c->cfg.dim;
      if (c->opt.dense_fast && c->opt.dense_wave) {
        // fast path: four hypotheses per workgroup, one wave each (dense.h: k_estimate_dense_w4); what its elimination
        // refuses is marked and taken through the SVD pseudo-inverse by the workgroup kernel behind it
        const int wpb = c->opt.dense_wave == 2 ? 2 : 4;   // systems per workgroup (2: 68 KB of LDS at n = 64, A/B)
        const size_t lds = sizeof(double) * wpb * ((size_t)n * (n | 1) + 2 * n);
        // (unconditionally: the attribute belongs to the (kernel, device) pair, and a flag per process or per context
        // misses the second device / the second kernel; the call is cheap)
        (void)hipFuncSetAttribute((const void *)k_estimate_dense_w4, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(sizeof(double) * 4 * (64 * 65 + 128)));
        if (n == 64 && c->opt.dense_wave == 3)  // the system in registers, one wave per hypothesis (k_estimate_dense_r64)
          hipLaunchKernelGGL(k_estimate_dense_r64, dim3((unsigned)c->H), dim3(64), 0, c->stream, c->d_data, c->stride, c->n,
                             c->d_subsets, (uint32_t)c->H, (int)M::SP, c->d_hparams, c->d_valid);
        else
        hipLaunchKernelGGL(k_estimate_dense_w4, dim3((unsigned)((c->H + wpb - 1) / wpb)), dim3(64 * wpb), lds, c->stream, c->d_data,
                           c->stride, c->n, c->d_subsets, (uint32_t)c->H, n, (int)M::SP, c->d_hparams, c->d_valid);
        hipLaunchKernelGGL(k_estimate_dense, dim3((unsigned)c->H), dim3(256), dense_lds_bytes(n), c->stream, c->d_data,
                           c->stride, c->n, c->d_subsets, (uint32_t)c->H, n, (int)M::SP, 0, c->d_hparams, c->d_valid, 1);
      } else {
        hipLaunchKernelGGL(k_estimate_dense, dim3((unsigned)c->H), dim3(256), dense_lds_bytes(n), c->stream, c->d_data,
                           c->stride, c->n, c->d_subsets, (uint32_t)c->H, n, (int)M::SP, c->opt.dense_fast,
                           c->d_hparams, c->d_valid, 0);
      }
    } else if constexpr (M::IS_US) {
      hipLaunchKernelGGL((k_estimate_us<(M::K == 4)>), dim3((unsigned)c->H), dim3(64), 0,
                         c->stream, c->d_data, c->stride, c->n, c->d_subsets, (uint32_t)c->H,
                         c->mc, c->d_hparams, c->d_valid, c->opt.us_fast);
      hipLaunchKernelGGL((k_prepare_f32_us<M>), dim3((unsigned)((c->H + 255) / 256)),
                         dim3(256), 0, c->stream, c->d_hparams, (uint32_t)c->H, c->mc,
                         c->d_hparams_f32);
    } else {
      int grid = (int)((c->H + kBlock - 1) / kBlock);
      hipLaunchKernelGGL((k_estimate<M>), dim3(grid), dim3(kBlock), 0, c->stream, c->d_data,
                         c->stride, c->n, c->d_subsets, (uint32_t)c->H, c->mc, c->d_hparams,
                         c->d_hparams_f32, c->d_valid);
    }
    HIPCHK(c, hipGetLastError());
    return LSQR_OK;
  });
}

constexpr uint32_t kScanChunk = 8192;  // hypotheses per scan launch (LDS counters: 32 KiB)

template <class M, int PPL>
int run_scan_ppl(lsqr_ctx *c) {
  HIPCHK(c, hipMemsetAsync(c->d_votes, 0, c->H * sizeof(uint32_t), c->stream));
  size_t tiles = (c->n + (size_t)kBlock * PPL - 1) / ((size_t)kBlock * PPL);
  for (size_t h0 = 0; h0 < c->H; h0 += kScanChunk) {
    uint32_t hc = (uint32_t)std::min<size_t>(kScanChunk, c->H - h0);
    size_t lds = (size_t)hc * sizeof(uint32_t);
    int per_cu = (int)std::min<size_t>(8, (160 * 1024) / std::max<size_t>(lds, 1));
    if (per_cu < 1) per_cu = 1;
    size_t max_blocks = (size_t)256 * per_cu;
    size_t tpb = (tiles + max_blocks - 1) / max_blocks;
    int grid = (int)((tiles + tpb - 1) / tpb);
    ProfScope ps(c, KID_SCAN);
    if (c->opt.filter)
      hipLaunchKernelGGL((k_scan<M, PPL, true>), dim3(grid), dim3(kBlock), lds, c->stream, c->d_data,
                         c->stride, c->n, c->d_hparams + h0 * M::SP, hc, c->mc, c->d_votes + h0);
    else
      hipLaunchKernelGGL((k_scan<M, PPL, false>), dim3(grid), dim3(kBlock), lds, c->stream,
                         c->d_data, c->stride, c->n, c->d_hparams + h0 * M::SP, hc, c->mc,
                         c->d_votes + h0);
    HIPCHK(c, hipGetLastError());
  }
  return LSQR_OK;
}

template <class M, int PPL, int GRAN = 0>
int run_scan_f32(lsqr_ctx *c) {
  HIPCHK(c, hipMemsetAsync(c->d_votes, 0, c->H * sizeof(uint32_t), c->stream));
  size_t tiles = (c->n + (size_t)kBlock * PPL - 1) / ((size_t)kBlock * PPL);
  for (size_t h0 = 0; h0 < c->H; h0 += kScanChunk) {
    uint32_t hc = (uint32_t)std::min<size_t>(kScanChunk, c->H - h0);
    size_t lds = (size_t)hc * sizeof(uint32_t);
    int per_cu = (int)std::min<size_t>(8, (160 * 1024) / std::max<size_t>(lds, 1));
    if (per_cu < 1) per_cu = 1;
    size_t max_blocks = (size_t)256 * per_cu;
    size_t tpb = (tiles + max_blocks - 1) / max_blocks;
    int grid = (int)((tiles + tpb - 1) / tpb);
    ProfScope ps(c, KID_SCAN);
    hipLaunchKernelGGL((k_scan_f32<M, PPL, GRAN>), dim3(grid), dim3(kBlock), lds, c->stream,
                       c->d_data, c->stride, c->n, c->d_hparams + h0 * M::SP,
                       c->d_hparams_f32 + h0 * M::SPF, hc, c->mc, c->d_votes + h0);
    HIPCHK(c, hipGetLastError());
  }
  return LSQR_OK;
}


// cell model of a point model (cells.h); models without one keep the exhaustive kernels
template <class M>
struct CellOf {};
template <int D>
struct CellOf<PlaneModel<D>> {
  typedef PlaneCell<D> type;
};
template <>
struct CellOf<Line2DModel> {  // same agree() as the 2-D hyperplane
  typedef PlaneCell<2> type;
};
template <int D>
struct CellOf<SphereModel<D>> {
  typedef SphereCell<D> type;
};
template <int D>
struct CellOf<LineModel<D>> {
  typedef LineCell<D> type;
};

// ---- spatial index (cells.h) ------------------------------------------------------------------------
// invalidates the index; its buffers are kept (a later upload of similar size rebuilds into them: hipMalloc /
// hipFree of a few hundred MB cost milliseconds, several times the build's 0.65 ms of kernel time)
// ---- lanes (lsqr_batch_fit_enqueue / _wait) -------------------------------------------------------------------
// nothing of any lane may still be reading this context's records
void lanes_quiesce(lsqr_ctx *c) {
  for (int i = 1; i < lsqr_ctx::kMaxLanes; i++)
    if (c->lanes[i]) {
      (void)hipStreamSynchronize(c->lanes[i]->stream);
      for (BatchSlotState &s : c->lanes[i]->slots) s.busy = false;  // results of a replaced upload are void
    }
}

void drop_index(lsqr_ctx *c) {
  c->h16_valid = false;  // (derived from the records alone, like the index)
  c->us16_valid = false;
  c->h16_nomem = c->us16_nomem = false;
  c->n_sorted = 0;
  c->n_cells = 0;
  c->index_valid = false;
  c->index_kd_levels = 0;
  c->axis_valid = false;
  c->tiles_pts = 0;
  c->tiles_nomem = false;
  c->last_count.valid = false;
}

// k_bounds over the current upload (point models): min / max per dimension, max |coordinate|, non-finite count
template <int D>
int run_bounds(lsqr_ctx *c) {
  if (c->bounds_valid) return LSQR_OK;
  const int nb = grid_for(c->n, 256 * 16, 1024);
  BoundsRow *rows = (BoundsRow *)c->d_partials.get();  // scratch: 1024 rows x 64 B (d_partials holds 4.4 MB)
  static_assert(sizeof(BoundsRow) == 64, "BoundsRow is 8 words");
  {
    ProfScope ps(c, KID_ABSMAX);
    hipLaunchKernelGGL((k_bounds<D>), dim3(nb), dim3(256), 0, c->stream, c->d_data, c->stride, c->n, rows);
  }
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_bounds_final, dim3(1), dim3(256), 0, c->stream, rows, nb, rows + 1024);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(c->h_pin->scratch, rows + 1024, sizeof(BoundsRow), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, sync_stream(c));
  memcpy(&c->h_bounds, c->h_pin->scratch, sizeof(BoundsRow));
  c->bounds_valid = true;
  return LSQR_OK;
}

template <int D>
int build_index(lsqr_ctx *c, uint32_t cell_pts) {
  drop_index(c);
  c->cell_pts = cell_pts;
  if (getenv("LSQR_TEST_FAIL_INDEX"))  // test hook: behave as if the sorted copy could not be allocated
    return fail(c, LSQR_ERR_HIP, "index build failure requested by LSQR_TEST_FAIL_INDEX");
  const size_t n = c->n;
#define IDXCHK(call)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      drop_index(c);                                                                          \
      return fail(c, LSQR_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),     \
                  __FILE__, __LINE__);                                                        \
    }                                                                                         \
  } while (0)
  int st = run_bounds<D>(c);  // (usually already there: the fp32 filters asked for max |x| when the hypotheses came)
  if (st != LSQR_OK) return st;
  const BoundsRow &hb = c->h_bounds;
  if (hb.mn[0] == ~0ULL) {  // no finite record at all: nothing can agree
    c->index_valid = true;
    return LSQR_OK;
  }
  IndexGrid g;
  memset(&g, 0, sizeof g);
  int total = 0;
  while (total < 24 && ((size_t)4 << (total + 1)) <= n) total++;  // about 4 records per bin
  int bits = total / D;
  if (bits < 1) bits = 1;
  if (D == 3 && bits > 8) bits = 8;
  if (D == 2 && bits > 12) bits = 12;
  g.bits = (uint32_t)bits;
  g.nbins = 1u << (bits * D);
  for (int d = 0; d < D; d++) {
    double lo = ord_u64_inv(hb.mn[d]), hi = ord_u64_inv(hb.mx[d]);
    double sc = hi > lo ? (double)(1u << bits) / (hi - lo) : 0.0;
    if (!(sc >= 0.0) || !(sc <= 1.7976931348623157e308)) sc = 0.0;
    g.lo[d] = lo;
    g.scale[d] = sc;
  }
  if (hb.nonfinite > n) return fail(c, LSQR_ERR_HIP, "index build: inconsistent bounds pass");
  // scratch: keys, permutation (in / out) + the radix sort's temporaries; kept with the context
  const size_t words = (n + 63) & ~(size_t)63;
  size_t tmp_bytes = 0;
  IDXCHK(sort_pairs_u32(nullptr, &tmp_bytes, nullptr, nullptr, nullptr, nullptr, n, (unsigned)(bits * D + 1),
                        c->stream));
  {  // the k-d levels above the runs sort (segment, coordinate) keys: up to 16 + 12 bits
    size_t tb2 = 0;
    IDXCHK(sort_pairs_u32(nullptr, &tb2, nullptr, nullptr, nullptr, nullptr, n, 28u, c->stream));
    tmp_bytes = std::max(tmp_bytes, tb2);
  }
  constexpr size_t kSegExtBytes = 4096 * sizeof(SegExtent);
  // (+ one more index array and the compact fp32 copy of the coordinates for the k-d levels: 16 B per record)
  const size_t need = (5 + D) * words * sizeof(uint32_t) + tmp_bytes + 256 + kSegExtBytes;
  if (need > c->d_idx_scratch.cap()) IDXCHK(c->d_idx_scratch.alloc(need));
  if ((st = ensure(c, c->d_sorted, std::max<size_t>(n, 1) * D)) != LSQR_OK) return st;
  const size_t n_sorted = n - (size_t)hb.nonfinite;  // the non-finite records carry the largest key: they sort to the tail
  const uint32_t n_cells = (uint32_t)((n_sorted + cell_pts - 1) / cell_pts);
  if ((st = ensure(c, c->d_boxes, std::max<size_t>((size_t)n_cells + n_cells / 2 + 2, 1))) != LSQR_OK)
    return st;
  c->super_merge = 0;
  // every buffer is in place (kept across uploads): from here on the build is device work only
  ProfScope ps(c, KID_INDEX);
  uint32_t *k_in = (uint32_t *)c->d_idx_scratch.get(), *v_in = k_in + words, *k_out = v_in + words,
           *v_out = k_out + words;
  uint32_t *q_b = v_out + words;
  float *xyz = (float *)(q_b + words);
  void *tmp = (void *)(xyz + (size_t)D * words);
  uint32_t *perm = v_out;  // the order the cells are cut from
  const unsigned gn = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL((k_keys<D>), dim3(gn), dim3(256), 0, c->stream, c->d_data, c->stride, n, g, k_in, v_in,
                     c->opt.presorted);
  IDXCHK(hipGetLastError());
  IDXCHK(sort_pairs_u32(tmp, &tmp_bytes, k_in, k_out, v_in, v_out, n, (unsigned)(bits * D + 1), c->stream));
  c->n_sorted = n_sorted;
  c->n_cells = n_cells;
  // k-d levels above the runs (cells.h: k_seg_extent / k_seg_keys + one radix sort per level), then the local k-d
  // refinement of every run (k_refine_runs): compact cells, fewer surviving pairs
  if (c->opt.refine && !c->opt.presorted && n_sorted > cell_pts && cell_pts >= 128 && cell_pts < kRunPts &&
      (cell_pts & (cell_pts - 1)) == 0) {
    SegExtent *d_ext = (SegExtent *)((char *)tmp + ((tmp_bytes + 255) & ~(size_t)255));
    uint32_t *q_a = v_in;  // (k_in / v_in are free after the Morton sort) positions into the Morton-ordered copy
    uint32_t top_shift = 13 + (uint32_t)std::max(0, std::min(c->kd_build_levels, 12));  // S = 8192 << levels
    while (top_shift > 14 && ((size_t)1 << (top_shift - 1)) >= n_sorted) top_shift--;  // one segment holds everything
    bool any = false;
    for (uint32_t sh = top_shift; sh > 13; sh--) {
      const uint32_t nseg = (uint32_t)((n_sorted + ((size_t)1 << sh) - 1) >> sh);
      if (nseg + 1 > 4096) continue;  // (more segments than the extent table: this level is left to the Morton order)
      if (!any) {
        hipLaunchKernelGGL((k_seg_gather<D>), dim3(gn), dim3(256), 0, c->stream, c->d_data, c->stride, v_out, n, n_sorted,
                           xyz, q_a);
        any = true;
      }
      unsigned segbits = 1;
      while ((1u << segbits) < nseg + 1) segbits++;
      hipLaunchKernelGGL(k_seg_extent_init, dim3((nseg + 255) / 256), dim3(256), 0, c->stream, d_ext, nseg);
      hipLaunchKernelGGL((k_seg_extent<D>), dim3((unsigned)((n_sorted + 1023) / 1024)), dim3(256), 0, c->stream, xyz, q_a,
                         n_sorted, sh, d_ext);
      hipLaunchKernelGGL((k_seg_keys<D>), dim3(gn), dim3(256), 0, c->stream, xyz, q_a, n, n_sorted, sh, nseg, d_ext, k_in,
                         q_b);
      IDXCHK(hipGetLastError());
      // sort (k_in, q_b) -> (k_out, q_a): the old order's buffer takes the new one
      IDXCHK(sort_pairs_u32(tmp, &tmp_bytes, k_in, k_out, q_b, q_a, n, 16u + segbits, c->stream));
    }
    if (any) {  // positions -> record indices
      hipLaunchKernelGGL(k_seg_compose, dim3(gn), dim3(256), 0, c->stream, v_out, q_a, n, q_b);
      IDXCHK(hipGetLastError());
      perm = q_b;
    }
    (void)hipFuncSetAttribute((const void *)k_refine_runs<D>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)refine_lds_bytes(D));
    const unsigned runs = (unsigned)((n_sorted + kRunPts - 1) / kRunPts);
    hipLaunchKernelGGL((k_refine_runs<D>), dim3(runs), dim3(1024), refine_lds_bytes(D), c->stream, c->d_data, c->stride,
                       perm, n_sorted, cell_pts);
    IDXCHK(hipGetLastError());
  }
  if (c->n_cells) {
    hipLaunchKernelGGL((k_gather_boxes<D>), dim3((c->n_cells + 3) / 4), dim3(256), 0, c->stream, c->d_data,
                       c->stride, perm, c->n_sorted, c->n_cells, cell_pts, c->d_sorted, c->d_boxes);
    IDXCHK(hipGetLastError());
  }
  // axis-sorted cells (axis.h): plane in 3-D, cells of 256 / 512 records
  c->axis_valid = false;
  if (D == 3 && c->opt.axis && c->cfg.model == LSQR_MODEL_PLANE && c->n_cells && (cell_pts == 512 || cell_pts == 256)) {
    if ((st = ensure(c, c->d_axis, (size_t)c->n_cells)) != LSQR_OK) return st;
    if ((st = ensure(c, c->d_cellT, (size_t)c->n_cells * cell_pts)) != LSQR_OK) return st;
    if ((st = ensure(c, c->d_slab, (size_t)c->n_cells)) != LSQR_OK) return st;
    double *d_cmom = (double *)c->d_idx_scratch.get();  // 80 B per cell: the sort's scratch is free again (16 B per record)
    if ((size_t)c->n_cells * 10 * sizeof(double) <= c->d_idx_scratch.cap()) {
      const unsigned gc = (c->n_cells + 3) / 4;
      if (cell_pts == 512) {
        hipLaunchKernelGGL((k_cell_moments<8>), dim3(gc), dim3(256), 0, c->stream, c->d_sorted, c->n_sorted, c->n_cells,
                           c->d_boxes, d_cmom);
      } else {
        hipLaunchKernelGGL((k_cell_moments<4>), dim3(gc), dim3(256), 0, c->stream, c->d_sorted, c->n_sorted, c->n_cells,
                           c->d_boxes, d_cmom);
      }
      const unsigned ngrp = (c->n_cells + kAxisGroup - 1) / kAxisGroup;
      hipLaunchKernelGGL(k_cell_axes, dim3((ngrp + 255) / 256), dim3(256), 0, c->stream, d_cmom, c->d_boxes, c->n_cells,
                         c->d_axis);
      if (cell_pts == 512)
        hipLaunchKernelGGL((k_cell_sort<8>), dim3(gc), dim3(256), 0, c->stream, c->d_sorted, c->n_sorted, c->n_cells,
                           c->d_boxes, c->d_axis, c->d_cellT);
      else
        hipLaunchKernelGGL((k_cell_sort<4>), dim3(gc), dim3(256), 0, c->stream, c->d_sorted, c->n_sorted, c->n_cells,
                           c->d_boxes, c->d_axis, c->d_cellT);
      {  // the cells' slabs for the counting pass (option "scan_slab"), from the sorted T[]
        double xabs;
        memcpy(&xabs, &hb.amax, sizeof xabs);  // (k_bounds: the bit pattern of max |coordinate|)
        hipLaunchKernelGGL(k_cell_slabs, dim3((c->n_cells + 255) / 256), dim3(256), 0, c->stream, c->d_boxes, c->d_axis,
                           c->d_cellT, c->n_sorted, c->n_cells, cell_pts, xabs, (uint32_t)c->opt.slab_gate, c->d_slab);
      }
      IDXCHK(hipGetLastError());
      c->axis_valid = true;
    }
  }
#undef IDXCHK
  c->index_kd_levels = c->kd_build_levels;
  c->index_valid = true;
  return LSQR_OK;
}

// ---- fp32 tiles of the index (cells.h: k_build_tiles; option "scan_tiles") ----
// Built (build_tiles, below) on the stream right behind an index build (scan_index_ready), or in front of the first
// scan that finds the option on and no tiles for the index in place; dropped with the index.  An accelerator like the index itself: without room for
// them the scans keep opening their cells from the sorted copy.
// the tiles a scan over cells of `cell_pts` records reads, or nullptr: it opens its cells with cells_load
inline const float *scan_tiles(const lsqr_ctx *c, uint32_t cell_pts) {
  return c->use_tiles && c->tiles_pts == cell_pts && c->cell_pts == cell_pts ? c->d_tiles.get() : nullptr;
}
// Which instantiations are built with the tile reader: the forms a default path reaches -- the packed forms of the
// prepared models, General of the others, k_scan_cells, each with the model's default broadcast mode ("scan_block" 256 /
// 257 and the forms behind "scan_pack", "scan_lean", "scan_prepared" 0 are A/B knobs) -- but for two kernels of the 3-D
// plane over 512-record cells that sit at their 80 registers (6 waves) and go to scratch with it, 12 bytes a lane:
// k_scan_cells and the packed form without the re-check ("scan_recheck" 0).  They keep cells_load.
template <class CM, int PP>
constexpr bool kTileSpills = std::is_same<CM, PlaneCell<3>>::value && PP == 4;
template <class CM, int PP, int CPT, bool LDSB>
constexpr bool kTileScanCells = CPT == 1 && LDSB == (CM::LDS_BROADCAST != 0) && !kTileSpills<CM, PP>;
template <class CM, int PP, bool LDSB, bool LDSB_DEFAULT, PairsForm F>
constexpr bool kTileScanPairs = (cell_prepared<CM>() ? packed(F) : F == PairsForm::General) && LDSB == LDSB_DEFAULT &&
                                !(kTileSpills<CM, PP> && F == PairsForm::Packed);

// a batch of hypotheses handed to the two-level scan: the context's current batch, or a compacted selection of it
struct ScanBatch {
  const double *sp;       // fp64 scan parameters, M::SP per hypothesis
  const float *spf;       // fp32 block, M::SPF per hypothesis
  size_t H;               // hypotheses (capacity when h_dev is set)
  uint32_t *votes;        // zeroed by the caller when h_dev is set
  const uint32_t *h_dev;  // device-side count (bounded scan) or null
  uint32_t h_off = 0;     // the batch starts at hypothesis h_off of the device-side selection (k_scan_pairs chunks)
};

template <class CM, int PP, int CPT, int BS, bool LDSB = false>
int launch_scan_cells(lsqr_ctx *c, const ScanBatch &b) {
  typedef typename CM::M M;
  const CellConsts cc = cell_consts((const CM *)nullptr, c->mc);
  HIPCHK(c, hipMemsetAsync(b.votes, 0, b.H * sizeof(uint32_t), c->stream));
  if (c->n_cells == 0) return LSQR_OK;
  const size_t wtiles = ((size_t)c->n_cells + CPT - 1) / CPT;
  constexpr int wpb = BS / 64;  // waves per workgroup
  if (!c->d_queues) HIPCHK(c, c->d_queues.alloc(kQueues * kQueuePitch));
  uint32_t *d_next = c->d_queues;
  // kern: the kernel, `tiles`: nothing, or the index's tiles for the form that reads them
  auto chunk = [&](auto kern, const size_t h0, auto... tiles) -> int {
    uint32_t hc = (uint32_t)std::min<size_t>(kScanChunk, b.H - h0);
    size_t lds = (size_t)((hc + 3) & ~3u) * sizeof(uint32_t) + (LDSB ? (size_t)wpb * 2048 : 0);
    int per_cu = (int)std::min<size_t>(32 / wpb, (160 * 1024) / std::max<size_t>(lds, 1));
    {  // persistent waves pulling tiles from the queues: launch exactly what is resident at once
      int occ = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, BS, lds) == hipSuccess && occ >= 1)
        per_cu = std::min(per_cu, occ);
      else
        (void)hipGetLastError();
    }
    if (per_cu < 1) per_cu = 1;
    size_t blocks = std::min<size_t>((wtiles + wpb - 1) / wpb, (size_t)256 * per_cu);
    // a unit is a whole tile by default: splitting the hypothesis range of a tile into segments
    // (scan_hsplit) evens the load but every extra unit start measured ~20 us of exposed memory
    // waiting (2.4 ms instead of 1.6 ms at 4 segments)
    const size_t waves = blocks * wpb, groups = (hc + 63) / 64;
    uint32_t hsplit = 1;
    if (c->opt.hsplit > 0) hsplit = (uint32_t)std::min<size_t>(groups, (size_t)c->opt.hsplit);
    const size_t units = wtiles * hsplit;
    const uint32_t grab = (uint32_t)std::min<size_t>(8, std::max<size_t>(1, units / (32 * waves)));
    ProfScope ps(c, KID_SCAN);
    HIPCHK(c, hipMemsetAsync(d_next, 0, kQueues * kQueuePitch * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(BS), lds,
                       c->stream, c->d_sorted.get(), c->n_sorted, c->d_boxes.get(), c->n_cells,
                       b.sp + h0 * M::SP,
                       CM::ROW_F32 ? b.spf + h0 * M::SPF : (const float *)(b.sp + h0 * M::SP),
                       b.spf + h0 * M::SPF, hc, c->mc, cc, b.votes + h0, d_next, grab, hsplit, b.h_dev, tiles...);
    HIPCHK(c, hipGetLastError());
    return LSQR_OK;
  };
  [[maybe_unused]] const float *tiles = scan_tiles(c, (uint32_t)(128 * PP));
  for (size_t h0 = 0; h0 < b.H; h0 += kScanChunk) {
    int st;
    if constexpr (kTileScanCells<CM, PP, CPT, LDSB>) {
      st = tiles ? chunk(k_scan_cells<CM, PP, CPT, BS, LDSB, const float *>, h0, tiles)
                 : chunk(k_scan_cells<CM, PP, CPT, BS, LDSB>, h0);
    } else {
      st = chunk(k_scan_cells<CM, PP, CPT, BS, LDSB>, h0);
    }
    if (st != LSQR_OK) return st;
  }
  return LSQR_OK;
}
template <class CM, int PP, int CPT>
int run_scan_cells(lsqr_ctx *c, const ScanBatch &b) {
  // hypothesis broadcast to the survivors: v_readlane, or (scan_block 257 / the model's choice)
  // uniform-address LDS reads.  (1024-thread workgroups measured 3-5 % slower and are no longer built.)
  if (c->opt.block == 257 || (c->opt.block == 0 && CM::LDS_BROADCAST))
    return launch_scan_cells<CM, PP, CPT, 256, true>(c, b);
  return launch_scan_cells<CM, PP, CPT, 256>(c, b);
}
template <class CM, int PP, int CPT>
int run_scan_cells(lsqr_ctx *c) {
  const ScanBatch b = {c->d_hparams, c->d_hparams_f32, c->H, c->d_votes, nullptr};
  return run_scan_cells<CM, PP, CPT>(c, b);
}

// cell size -> packed pairs per lane (PP = cell / 128); 1024-point cells only where the cell model is built for them
template <class CM, class F>
int with_pp(uint32_t cell_pts, F &&f) {
  if constexpr (requires { CM::MAX_PP; }) {
    if (cell_pts == 1024) return f(std::integral_constant<int, 8>{});
  }
  if (cell_pts == 512) return f(std::integral_constant<int, 4>{});
  return f(std::integral_constant<int, 2>{});
}

// the index's fp32 tiles (see scan_tiles above)
template <class CM>
int build_tiles(lsqr_ctx *c) {
  if (!c->use_tiles || !c->index_valid || c->n_cells == 0 || c->tiles_pts == c->cell_pts || c->tiles_nomem) return LSQR_OK;
  const size_t need = (size_t)c->n_cells * tile_cell_floats<CM>((int)(c->cell_pts / 128));
  if (need > c->d_tiles.cap() && c->d_tiles.alloc(need) != hipSuccess) {
    (void)hipGetLastError();
    c->tiles_nomem = true;
    return LSQR_OK;
  }
  // (not timed under KID_INDEX: that id counts index builds, one launch scope each)
  const int st = with_pp<CM>(c->cell_pts, [&](auto pp) -> int {
    hipLaunchKernelGGL((k_build_tiles<CM, decltype(pp)::value>), dim3((c->n_cells + 3) / 4), dim3(256), 0, c->stream,
                       c->d_sorted.get(), c->n_sorted, c->d_boxes.get(), c->n_cells, c->d_tiles.get());
    HIPCHK(c, hipGetLastError());
    return LSQR_OK;
  });
  if (st == LSQR_OK) c->tiles_pts = c->cell_pts;
  return st;
}

// level 1 of the two-level scan alone over the current batch: d_ub[h] = vote bound, d_counter[CNT_PAIRS] = surviving pairs
template <class CM, int PP>
int run_cells_bounds(lsqr_ctx *c, uint32_t *d_ub, uint32_t *d_nc = nullptr) {
  typedef typename CM::M M;
  const CellConsts cc = cell_consts((const CM *)nullptr, c->mc);
  HIPCHK(c, hipMemsetAsync(d_ub, 0, c->H * sizeof(uint32_t), c->stream));
  if (d_nc) HIPCHK(c, hipMemsetAsync(d_nc, 0, c->H * sizeof(uint32_t), c->stream));
  if (d_nc) HIPCHK(c, hipMemsetAsync(c->d_counter + CNT_PAIRS, 0, sizeof(unsigned long long), c->stream));
  if (c->n_cells == 0) return LSQR_OK;
  // The bounds of the bounded scan are taken on merged boxes (a quarter of the tests; the bound stays valid);
  // the diagnostics (d_nc: lsqr_scan_workload) count the surviving CELLS and stay on the cells.
  // ... as long as a few thousand boxes remain: on a small upload coarse boxes cost the selection its teeth (300 k
  // points in 147 boxes: 261 of 2048 hypotheses skipped instead of 1800)
  // ... and as long as the looser bound still prunes: a random plane cuts ~13 % of the cells but ~25 % of the merged
  // boxes, and with few inliers (80 % outliers and up) that population exceeds the best model's votes -- every
  // hypothesis would be counted.  The selection counts of earlier batches come back through pinned memory
  // (bsel_known: the latest batch the host has synchronised with; an older value only delays the switch): once a
  // second pass held more than a third of its batch, the bounds of this upload stay on the cells.
  uint32_t merge = c->opt.bound_merge ? (uint32_t)c->opt.bound_merge : (uint32_t)CM::BOUND_MERGE;
  if (!c->opt.bound_merge) {
    while (merge > 1 && c->n_cells / merge < 4096) merge /= 2;
    if (c->bsel_known_H && (uint64_t)c->bsel_known.n_rest * 3 > c->bsel_known_H) c->merge_off = true;
    if (c->merge_off) merge = 1;
  }
  if (d_nc || merge < 2 || c->n_cells < 4 * merge) merge = 1;
  const CellBox *boxes = c->d_boxes;
  uint32_t nbox = c->n_cells;
  if (merge > 1) {
    nbox = (c->n_cells + merge - 1) / merge;
    if (c->super_merge != merge) {
      hipLaunchKernelGGL((k_super_boxes<M::ND>), dim3((nbox + 255) / 256), dim3(256), 0, c->stream, c->d_boxes,
                         c->n_cells, c->d_boxes + c->n_cells, nbox, merge);
      HIPCHK(c, hipGetLastError());
      c->super_merge = merge;
    }
    boxes = c->d_boxes + c->n_cells;
  }
  const unsigned gy = (unsigned)((c->H + 255) / 256);
  unsigned gx = std::max(1u, std::min<unsigned>(nbox, 2048u / gy));
  const uint32_t per = (nbox + gx - 1) / gx;
  gx = (nbox + per - 1) / per;
  hipLaunchKernelGGL((k_cells_bounds<CM, PP, BoundsForm::General>), dim3(gx, gy), dim3(256), 0, c->stream, boxes, nbox,
                     c->n_sorted,
                     CM::ROW_F32 ? c->d_hparams_f32 : (const float *)c->d_hparams.get(), c->d_hparams_f32,
                     (uint32_t)c->H, cc, per, d_ub, d_nc ? c->d_counter + CNT_PAIRS : (unsigned long long *)nullptr, d_nc,
                     (uint8_t *)nullptr, 0u, (const uint32_t *)nullptr, 0u,  // (pair total: diagnostics only -- 8192
                     (uint32_t)(128 * PP) * merge, (const float4 *)nullptr,   // atomics on one address are ~100 us)
                     (const CellSlab *)nullptr);
  HIPCHK(c, hipGetLastError());
  return LSQR_OK;
}

// The form of the counted scan (cells.h: PairsForm) a launch takes, from the cell model, the broadcast mode and the
// options "scan_prepared", "scan_lean", "scan_pack", "scan_recheck"; which forms exist for a cell model and a broadcast
// mode is cells.h' rule (pairs_form_exists).
template <class CM>
PairsForm pairs_form(bool ldsb, bool opt_prepared, bool opt_lean, bool opt_pack, bool opt_recheck) {
  if (!cell_prepared<CM>() || !opt_prepared) return PairsForm::General;
  if (!opt_lean) return PairsForm::Prepared;
  if (!opt_pack) return PairsForm::Lean;
  const bool can_recheck = ldsb && pairs_form_exists<CM, true, PairsForm::PackedRecheck>();
  return can_recheck && opt_recheck ? PairsForm::PackedRecheck : PairsForm::Packed;
}
// f(form, ldsb) with both as compile-time constants, for the forms that exist (pairs_form_exists): PackedRecheck for the
// 3-D plane with the broadcast area, the other prepared forms for the cell models with PREPARED, General for every one
template <class CM, class F>
int with_pairs_form(PairsForm form, bool ldsb, F &&f) {
  auto go = [&](auto fc) { return ldsb ? f(fc, std::true_type{}) : f(fc, std::false_type{}); };
  if constexpr (cell_prepared<CM>()) {
    if constexpr (pairs_form_exists<CM, true, PairsForm::PackedRecheck>()) {
      if (form == PairsForm::PackedRecheck && ldsb)
        return f(std::integral_constant<PairsForm, PairsForm::PackedRecheck>{}, std::true_type{});
    }
    if (form == PairsForm::Packed) return go(std::integral_constant<PairsForm, PairsForm::Packed>{});
    if (form == PairsForm::Lean) return go(std::integral_constant<PairsForm, PairsForm::Lean>{});
    if (form == PairsForm::Prepared) return go(std::integral_constant<PairsForm, PairsForm::Prepared>{});
  }
  if (form == PairsForm::General) return go(std::integral_constant<PairsForm, PairsForm::General>{});
  return LSQR_ERR_INVALID;  // (pairs_form() does not choose a form that is not built)
}

// Level 2 of a (compacted) batch in statically balanced pieces (cells.h, "statically balanced level 2"): count the
// survivors per (cell, group), sum them per cell and per chunk, then k_scan_pairs.  Chained on the stream.
template <class CM, int PP>
int run_scan_pairs(lsqr_ctx *c, const ScanBatch &b0) {
  typedef typename CM::M M;
  // k_scan_pairs holds a cell's groups in the 64 lanes of a wave: batches of more than 4096 hypotheses are counted
  // 4096 at a time (rare: the bounded scan's second pass is sized for the whole batch but holds ~1/8 of it, so the
  // later launches find an empty cost table and return at once)
  constexpr size_t kPairsChunk = 4096;  // 64 groups of 64
  if (b0.H > kPairsChunk) {
    for (size_t h0 = 0; h0 < b0.H; h0 += kPairsChunk) {
      ScanBatch sub = {b0.sp + h0 * M::SP, b0.spf + h0 * M::SPF, std::min<size_t>(kPairsChunk, b0.H - h0),
                       b0.votes + h0, b0.h_dev, (uint32_t)(b0.h_off + h0)};
      int st = run_scan_pairs<CM, PP>(c, sub);
      if (st != LSQR_OK) return st;
    }
    return LSQR_OK;
  }
  const ScanBatch &b = b0;
  const CellConsts cc = cell_consts((const CM *)nullptr, c->mc);
  if (c->n_cells == 0 || b.H == 0) {
    HIPCHK(c, hipMemsetAsync(b.votes, 0, b.H * sizeof(uint32_t), c->stream));
    return LSQR_OK;
  }
  const uint32_t Hc = (uint32_t)b.H, groups = (Hc + 63) / 64;
  const uint32_t gstride = groups <= 1 ? 1u : (groups + 15) / 16 * 16;  // 16-byte rows for k_tile_costs
  const uint32_t nchunks = (c->n_cells + kChunkCells - 1) / kChunkCells;
  int st;
  if ((st = ensure(c, c->d_paircnt, (size_t)c->n_cells * gstride)) != LSQR_OK) return st;
  if ((st = ensure(c, c->d_paircost, (size_t)c->n_cells + nchunks)) != LSQR_OK) return st;
  uint32_t *d_cost = c->d_paircost, *d_csum = c->d_paircost + c->n_cells;
  const float *rows = CM::ROW_F32 ? b.spf : (const float *)b.sp;
  constexpr bool kLdsbDefault = [] {
    if constexpr (requires { CM::LDS_BROADCAST_PAIRS; }) return CM::LDS_BROADCAST_PAIRS != 0;
    else return CM::LDS_BROADCAST != 0;
  }();
  const bool ldsb = c->opt.block == 257 || (c->opt.block == 0 && kLdsbDefault);
  // the form, once: the counting pass, k_tile_costs, the LDS size and k_scan_pairs below all read it
  const PairsForm form = pairs_form<CM>(ldsb, c->opt.prepared, c->opt.lean, c->opt.pack, c->opt.recheck);
  // the hypothesis-only part of level 1 once per batch instead of once per (cell, group): both kernels below read it
  if constexpr (cell_prepared<CM>()) {
    if (prepared(form)) {
      const uint32_t slots = (Hc + 63) & ~63u;  // whole groups
      if ((st = ensure(c, c->d_hyps, (size_t)slots * HypWords<CM>::N4)) != LSQR_OK) return st;
      hipLaunchKernelGGL((k_prepare_hyps<CM>), dim3((slots + 255) / 256), dim3(256), 0, c->stream, rows, b.spf, Hc, cc,
                         b.h_dev, b.h_off, c->d_hyps);
      HIPCHK(c, hipGetLastError());
    }
  }
  const float4 *hyps = prepared(form) ? c->d_hyps : nullptr;
  // packed blocks (cells.h: pairs_cell_packed): the counting pass leaves survivor masks instead of counts
  if (packed(form) && (st = ensure(c, c->d_pairmask, (size_t)c->n_cells * gstride)) != LSQR_OK) return st;
  uint8_t *d_cnt = packed(form) ? (uint8_t *)c->d_pairmask.get() : c->d_paircnt.get();
  constexpr int BS = 256, wpb = BS / 64;
  const size_t lds = (size_t)((Hc + 3) & ~3u) * sizeof(uint32_t) + (ldsb ? (size_t)wpb * 2048 : 0) +
                     (packed(form) ? (size_t)wpb * 256 : 0);  // votes | broadcast areas | id lists of the packed blocks
  return with_pairs_form<CM>(form, ldsb, [&](auto form_c, auto ldsb_c) -> int {
    constexpr PairsForm F = decltype(form_c)::value;
    constexpr bool LDSB = decltype(ldsb_c)::value;
    {  // counting pass: waves past the device-side H leave at once, so the grid is cut finely in x
      const unsigned gy = (Hc + 255) / 256;
      const uint32_t per = std::max<uint32_t>(8, (c->n_cells + 1023) / 1024);
      const unsigned gx = (c->n_cells + per - 1) / per;
      // the slab test (option "scan_slab"): the masks of the 3-D plane over an axis-sorted index of this cell size
      const CellSlab *slabs = nullptr;
      if constexpr (packed(F) && cell_slab<CM>()) {
        if (c->opt.slab && c->axis_valid && c->cell_pts == (uint32_t)(128 * PP)) slabs = c->d_slab;
      }
      c->last_count.valid = true, c->last_count.packed = packed(F), c->last_count.slab = slabs != nullptr;
      c->last_count.H = Hc, c->last_count.h_off = b.h_off, c->last_count.gstride = gstride, c->last_count.h_dev = b.h_dev;
      auto count = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(gx, gy), dim3(256), 0, c->stream, c->d_boxes, c->n_cells, c->n_sorted, rows, b.spf,
                           Hc, cc, per, (uint32_t *)nullptr, (unsigned long long *)nullptr, (uint32_t *)nullptr,
                           d_cnt, gstride, b.h_dev, b.h_off, (uint32_t)(128 * PP), hyps, slabs);
      };
      // (General alone has two counting forms, and "scan_lean" says which: an option's value cannot be a template
      // argument, so it is read once more here; for the other forms both branches name the same kernel)
      if (c->opt.lean)  // masks, or cnt, and nothing else
        count(k_cells_bounds<CM, PP, bounds_form(F, true)>);
      else
        count(k_cells_bounds<CM, PP, bounds_form(F, false)>);
      HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(k_tile_costs<packed(F)>, dim3(nchunks), dim3(kChunkCells), 0, c->stream, (const uint8_t *)d_cnt,
                       gstride, Hc, b.h_dev, c->n_cells, d_cost, d_csum, b.votes, b.h_off,  // (zeroes the batch's votes)
                       c->amb_reset ? c->d_ambcnt.get() : (unsigned long long *)nullptr);
    c->amb_reset = false;
    c->amb_counted = cell_prepared<CM>() && M::ND == 3;  // (k_scan_pairs counts for the 3-D plane)
    HIPCHK(c, hipGetLastError());
    // kern: the kernel, `tiles`: nothing, or the index's tiles for the form that reads them
    auto scan = [&](auto kern, auto... tiles) -> int {
      int per_cu = (int)std::min<size_t>(32 / wpb, (160 * 1024) / std::max<size_t>(lds, 1)), occ = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, BS, lds) == hipSuccess && occ >= 1)
        per_cu = std::min(per_cu, occ);
      else
        (void)hipGetLastError();
      if (per_cu < 1) per_cu = 1;
      if (c->opt.pairs_waves > 0) per_cu = std::min(per_cu, c->opt.pairs_waves);
      const unsigned blocks = (unsigned)std::min<size_t>(((size_t)c->n_cells + wpb - 1) / wpb, (size_t)256 * per_cu);
      int st2 = ensure(c, c->d_vpart, (size_t)blocks * Hc);
      if (st2 != LSQR_OK) return st2;
      ProfScope ps(c, KID_SCAN);
      hipLaunchKernelGGL(kern, dim3(blocks), dim3(BS), lds, c->stream, c->d_sorted.get(), c->n_sorted, c->d_boxes.get(),
                         c->n_cells, b.sp, rows, b.spf, Hc, c->mc, cc, c->d_vpart.get(), Hc, b.h_dev, (const uint8_t *)d_cnt,
                         gstride, (const uint32_t *)d_cost, (const uint32_t *)d_csum, nchunks, b.h_off, hyps,
                         c->d_ambcnt.get(), tiles...);
      HIPCHK(c, hipGetLastError());
      hipLaunchKernelGGL(k_votes_reduce, dim3((Hc + 63) / 64, 48), dim3(256), 0, c->stream,
                         (const uint32_t *)c->d_vpart, Hc, (uint32_t)blocks, Hc, b.h_dev, b.votes, b.h_off);
      HIPCHK(c, hipGetLastError());
      return LSQR_OK;
    };
    if constexpr (kTileScanPairs<CM, PP, LDSB, kLdsbDefault, F>) {
      if (const float *tiles = scan_tiles(c, (uint32_t)(128 * PP)))
        return scan(k_scan_pairs<CM, PP, BS, LDSB, F, const float *>, tiles);
    }
    return scan(k_scan_pairs<CM, PP, BS, LDSB, F>);
  });
}

// Vote bounds by rank (axis.h; plane in 3-D over axis-sorted cells) on top of the box-population bounds in d_ub:
// candidates -> their upper AND lower vote bounds by rank (k_bound_axis: no observation is evaluated) -> d_ub refined
// in place, *lo_out = per-hypothesis lower bounds for the selections of the bounded scan.
template <int PP>
int run_rank_bounds(lsqr_ctx *c, const uint32_t **lo_out) {
  typedef PlaneCell<3> CM;
  typedef typename CM::M M;
  const uint32_t H = (uint32_t)c->H;
  int st;
  if (!c->d_ub2) HIPCHK(c, c->d_ub2.alloc(3 * c->H_cap));  // [ub2 | lb2 | lo]
  uint32_t *ub2 = c->d_ub2, *lb2 = c->d_ub2 + c->H_cap, *lo = c->d_ub2 + 2 * c->H_cap;
  const CellConsts cc = cell_consts((const CM *)nullptr, c->mc);
  // (the candidate list and their rows use the second pass's areas: free until the pilots have been counted)
  uint32_t *cand = c->d_sel + kPilots;
  double *sp_b = c->d_hparams2 + (size_t)kPilots * M::SP;
  float *spf_b = c->d_hparams2_f32 + (size_t)kPilots * M::SPF;
  hipLaunchKernelGGL(k_pick_cands, dim3(1), dim3(1024), 0, c->stream, c->d_ub, c->d_valid, H, c->best_before, cand,
                     c->d_bsel, c->d_votes, ub2, lb2, lo);
  hipLaunchKernelGGL(k_gather_rows, dim3((H + 3) / 4), dim3(256), 0, c->stream, cand, &c->d_bsel->n_cand, H,
                     c->d_hparams, (int)M::SP, c->d_hparams_f32, (int)M::SPF, sp_b, spf_b);
  HIPCHK(c, hipGetLastError());
  const unsigned gy = (H + 511) / 512;  // (workgroups past the device-side candidate count return at once)
  const uint32_t per = std::max<uint32_t>(8, ((c->n_cells + 3071) / 3072 + 7) / 8 * 8);
  const unsigned gx = (c->n_cells + per - 1) / per;
  float thr_up = (float)c->mc.thr, thr_dn = thr_up;
  if ((double)thr_up < c->mc.thr) thr_up = nextafterf(thr_up, INFINITY);
  if ((double)thr_dn > c->mc.thr) thr_dn = nextafterf(thr_dn, -INFINITY);
  float xabs = (float)c->mc.absmax;
  if ((double)xabs < c->mc.absmax) xabs = nextafterf(xabs, INFINITY);
  hipLaunchKernelGGL((k_bound_axis<PP>), dim3(gx, gy), dim3(512), 0, c->stream, c->d_boxes, c->d_axis, c->d_cellT,
                     c->n_sorted, c->n_cells, (const float *)sp_b, H, &c->d_bsel->n_cand, cc, thr_up, thr_dn, xabs, per,
                     ub2, lb2);
  hipLaunchKernelGGL(k_refine_bounds, dim3((H + 255) / 256), dim3(256), 0, c->stream, cand, c->d_bsel, ub2, lb2,
                     c->d_ub, lo);
  HIPCHK(c, hipGetLastError());
  (void)st;
  *lo_out = lo;
  return LSQR_OK;
}

// The bounded scan of the current batch over the index (cells.h, "bounded scan"): bounds, pilots counted exactly,
// then only the hypotheses that can still become the running maximum.  Everything is chained on the stream.
template <class CM, int PP>
int run_scan_bounded(lsqr_ctx *c) {
  typedef typename CM::M M;
  // profiling: ONE scope over the whole scan phase (bounds, selections, both counting launches)
  ProfScope whole(c, KID_SCAN);
  ProfMute mute(c);
  // the record this scan will write: whatever it still holds (the scan two back) has to have landed before it is
  // reused, and is folded here at the latest
  if (!c->h_bsel) {
    HIPCHK(c, c->h_bsel.alloc(128 / sizeof(BoundSel)));
    memset(c->h_bsel, 0, 128);
    for (BselRecord &r : c->bsel) HIPCHK(c, r.ev.create(hipEventDisableTiming));
  }
  const int rec = (int)(c->bsel_seq & 1);
  BselRecord &b = c->bsel[rec];
  if (b.pending) {
    HIPCHK(c, hipEventSynchronize(b.ev));
    bsel_fold(c, rec);
  }
  int st = run_cells_bounds<CM, PP>(c, c->d_ub);
  if (st != LSQR_OK) return st;
  const uint32_t H = (uint32_t)c->H;
  uint32_t *sel_a = c->d_sel, *sel_b = c->d_sel + kPilots;
  uint32_t *votes_a = c->d_votes2, *votes_b = c->d_votes2 + kPilots;
  double *sp_a = c->d_hparams2, *sp_b = c->d_hparams2 + (size_t)kPilots * M::SP;
  float *spf_a = c->d_hparams2_f32, *spf_b = c->d_hparams2_f32 + (size_t)kPilots * M::SPF;
  const uint32_t *lo = nullptr;  // lower vote bounds (rank bounds of the plane), or none
  if constexpr (std::is_same<CM, PlaneCell<3>>::value && (PP == 4 || PP == 2)) {
    if (c->axis_valid && c->opt.axis && c->cell_pts == (uint32_t)(128 * PP))
      if ((st = run_rank_bounds<PP>(c, &lo)) != LSQR_OK) return st;
  }
  // The pilot pass is five launches that find nothing to do when a lower bound of the running maximum is known
  // without pilots (rank bounds, or the best of earlier batches).  Whether it was is reported back through pinned
  // memory (bsel_known: the latest batch the host has synchronised with -- one or two batches back): after a batch of
  // this upload and model that needed no pilots the pass is not launched -- k_pick_pilots then selects none; if that
  // batch would have needed them after all, its second pass counts more hypotheses (never wrongly: L[h] is a lower
  // bound either way) and a later batch gets its pilots back.
  const bool no_pilots = c->bsel_known_H == H && c->bsel_known.known != 0;
  hipLaunchKernelGGL(k_pick_pilots, dim3(1), dim3(1024), 0, c->stream, c->d_ub, c->d_valid, H, sel_a, c->d_bsel,
                     c->d_votes, c->best_before, lo, no_pilots ? 1 : 0);  // (also zeroes the batch's votes)
  if (!no_pilots) {
    hipLaunchKernelGGL(k_gather_rows, dim3(kPilots / 4), dim3(256), 0, c->stream, sel_a, &c->d_bsel->n_pilot,
                       (uint32_t)kPilots, c->d_hparams, (int)M::SP, c->d_hparams_f32, (int)M::SPF, sp_a, spf_a);
    HIPCHK(c, hipGetLastError());
    const ScanBatch pa = {sp_a, spf_a, (size_t)kPilots, votes_a, &c->d_bsel->n_pilot};
    if ((st = run_scan_pairs<CM, PP>(c, pa)) != LSQR_OK) return st;
  }

  hipLaunchKernelGGL(k_pick_rest, dim3(1), dim3(1024), 0, c->stream, c->d_ub, c->d_valid, H, sel_a, votes_a,
                     c->best_before, sel_b, c->d_bsel, lo);
  hipLaunchKernelGGL(k_gather_rows, dim3((H + 3) / 4), dim3(256), 0, c->stream, sel_b, &c->d_bsel->n_rest, H,
                     c->d_hparams, (int)M::SP, c->d_hparams_f32, (int)M::SPF, sp_b, spf_b);
  HIPCHK(c, hipGetLastError());
  const ScanBatch pb = {sp_b, spf_b, (size_t)H, votes_b, &c->d_bsel->n_rest};
  if ((st = run_scan_pairs<CM, PP>(c, pb)) != LSQR_OK) return st;

  hipLaunchKernelGGL(k_scatter_votes, dim3((H + 255) / 256 + 1), dim3(256), 0, c->stream, sel_a, &c->d_bsel->n_pilot,
                     votes_a, sel_b, &c->d_bsel->n_rest, votes_b, c->d_votes);
  HIPCHK(c, hipGetLastError());
  c->last_bound[0] = 1;
  c->last_bound[3] = H;
  HIPCHK(c, hipMemcpyAsync(bsel_rec(c, rec), c->d_bsel, sizeof(BoundSel), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipEventRecord(b.ev, c->stream));
  b.pending = true;
  b.seq = ++c->bsel_seq;
  b.H = H;
  c->bsel_last_rec = rec;
  return LSQR_OK;
}

// ---- chunked early exit (earlyexit.h) ---------------------------------------------------------------------
constexpr size_t kEeCap = kSelCap;  // hypotheses per batch the selection kernels handle (models.h)
static_assert(kEeCap <= kSelCap && kScanChunk <= kSelCap, "selection kernels: 1024 threads x 8 hypotheses");
struct EeBuf {
  EeState *st;
  uint32_t *sel_c, *sel_o[2];
  float *thr_c, *rows_c;
};
int ee_buffers(lsqr_ctx *c, EeBuf *b) {
  const size_t bytes = 256 + 3 * kEeCap * sizeof(uint32_t) + (4 + 64) * (kEeCap + 64) * sizeof(float);
  if (!c->d_ee) HIPCHK(c, c->d_ee.alloc(bytes));
  if (!c->h_ee) {
    HIPCHK(c, c->h_ee.alloc(1));
    memset(c->h_ee, 0, sizeof(EeState));
  }
  char *p = c->d_ee;
  b->st = (EeState *)p;
  b->sel_c = (uint32_t *)(p + 256);
  b->sel_o[0] = b->sel_c + kEeCap;
  b->sel_o[1] = b->sel_o[0] + kEeCap;
  b->thr_c = (float *)(b->sel_o[1] + kEeCap);
  b->rows_c = b->thr_c + 4 * (kEeCap + 64);  // (the fp16 filter keeps 4 floats per hypothesis, the fp32 filter 2)
  return LSQR_OK;
}
// scan(row_begin, row_end, range_dev, h_dev, sel): sel == null -> the context's whole batch over [row_begin, row_end),
// else the compact selection the last gather(sel, n_dev) produced, over the device-side range range_dev (launch sized
// for [row_begin, row_end)).  Everything is chained on the stream; no host round trip.
template <class Scan, class Gather>
int run_early_exit(lsqr_ctx *c, size_t align, const EeBuf &b, Scan &&scan, Gather &&gather) {
  const size_t n = c->n;
  const uint32_t H = (uint32_t)c->H;
  size_t b1 = (n / 16 + align - 1) / align * align;
  if (b1 > n) b1 = n;
  int st;
  HIPCHK(c, hipMemsetAsync(c->d_votes, 0, H * sizeof(uint32_t), c->stream));
  // A: the first sixteenth, every hypothesis
  if ((st = scan(0, b1, (const uint32_t *)nullptr, (const uint32_t *)nullptr, (const uint32_t *)nullptr)) != LSQR_OK)
    return st;
  hipLaunchKernelGGL(k_ee_split, dim3(1), dim3(1024), 0, c->stream, c->d_votes, c->d_valid, H, b.sel_c, b.sel_o[0], b.st,
                     (uint32_t)b1, (uint32_t)n);
  HIPCHK(c, hipGetLastError());
  if (b1 < n) {
    // B: the candidates to the end
    if ((st = gather(b.sel_c, &b.st->n_cand)) != LSQR_OK) return st;
    if ((st = scan(b1, n, &b.st->rng[0][0], &b.st->n_cand, b.sel_c)) != LSQR_OK) return st;
    hipLaunchKernelGGL(k_ee_plan, dim3(1), dim3(1024), 0, c->stream, c->d_votes, b.sel_c, b.st, c->best_before,
                       (uint32_t)b1, (uint32_t)n, (uint32_t)align);
    HIPCHK(c, hipGetLastError());
    // C: the others over the planned ranges
    int cur = 0;
    for (int k = 1; k <= kEeChunksC; k++) {
      if ((st = gather(b.sel_o[cur], &b.st->n_alive)) != LSQR_OK) return st;
      if ((st = scan(b1, n, &b.st->rng[k][0], &b.st->n_alive, b.sel_o[cur])) != LSQR_OK) return st;
      if (k < kEeChunksC) {
        hipLaunchKernelGGL(k_ee_select, dim3(1), dim3(1024), 0, c->stream, c->d_votes, c->d_valid, H, (uint32_t)n, k,
                           c->best_before, b.sel_o[cur], b.sel_o[cur ^ 1], b.st);
        HIPCHK(c, hipGetLastError());
        cur ^= 1;
      }
    }
  }
  HIPCHK(c, hipMemcpyAsync(c->h_ee, b.st, sizeof(EeState), hipMemcpyDeviceToHost, c->stream));
  c->ee_last = true;
  c->ee_H = H;
  c->ee_n = n;
  return LSQR_OK;
}

// ---- scratch and worklist of the matrix-core filters ------------------------------------------------------
// The fp16 / fp32 filters of the dense, US and phantom scans keep their per-batch operands and the fill of their
// worklist segments in d_partials (the fits use it between scans); the fp64 dense filter keeps its thresholds there.
constexpr size_t kFilterHypCap = 8192;         // hypotheses per batch of the fp16 / fp32 filters
constexpr size_t kSegWords = 1024;             // segment counters (one per filter workgroup: <= 512 in use)
constexpr uint32_t kSegCap = kAmbCap / 1024;   // worklist entries per segment
struct FilterScratchLayout {
  float thr32[2 * kFilterHypCap];   // 2 floats per hypothesis
  float sp32[64 * kFilterHypCap];   // 64 floats per hypothesis (2 MB); the fp16 filter's rows live here too
  unsigned int segcnt[kSegWords];
};
static_assert(offsetof(FilterScratchLayout, sp32) == sizeof(float) * 2 * 8192 &&
              offsetof(FilterScratchLayout, segcnt) == sizeof(float) * (2 * 8192 + 64 * 8192), "areas stay where they were");
static_assert(sizeof(FilterScratchLayout) <= kPartialsBytes && kSegWords * kSegCap <= kAmbCap, "d_partials / d_amb hold it");
struct FilterScratch {
  float *thr32, *sp32;
  unsigned int *segcnt;
  double *thr;  // the fp64 filter: 2 doubles per hypothesis (H checked by its caller)
};
FilterScratch filter_scratch(lsqr_ctx *c) {
  FilterScratchLayout *l = (FilterScratchLayout *)c->d_partials.get();
  return {l->thr32, l->sp32, l->segcnt, c->d_partials};
}
// before a filter's launches: no segment holds anything, no fill recorded (fs == null: the fp64 filter's one worklist)
int worklist_reset(lsqr_ctx *c, const FilterScratch *fs) {
  if (fs) HIPCHK(c, hipMemsetAsync(fs->segcnt, 0, kSegWords * sizeof(unsigned int), c->stream));
  HIPCHK(c, hipMemsetAsync(c->d_counter + CNT_OVF, 0, sizeof(unsigned long long), c->stream));
  return LSQR_OK;
}
// after them: did the fullest segment stay within seg_cap?  lsqr_batch_fit_enqueue (defer_ovf) must not wait: the scan only
// notes seg_cap, lsqr_batch_fit_wait compares; everyone else synchronises here.  "scan_test_overflow": always OVERFLOWED.
struct WorklistFill {
  enum { DEFERRED, FITS, OVERFLOWED } state;
  unsigned int fill;
};
int worklist_check(lsqr_ctx *c, uint32_t seg_cap, WorklistFill *w) {
  *w = {WorklistFill::DEFERRED, 0};
  if (c->defer_ovf) {
    c->ovf_cap = seg_cap;
    return LSQR_OK;
  }
  HIPCHK(c, hipMemcpyAsync(c->h_pin->scratch, c->d_counter + CNT_OVF, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, sync_stream(c));
  w->fill = *(unsigned int *)c->h_pin->scratch;
  w->state = w->fill > seg_cap || c->opt.test_overflow ? WorklistFill::OVERFLOWED : WorklistFill::FITS;
  return LSQR_OK;
}

// once per context: does this device's matrix unit align the products of one instruction as the fp16 filters'
// thresholds assume (dense_h16.h: k_dense_h16_probe)?  c->h16_unit = 1 / -1.
int h16_probe_unit(lsqr_ctx *c) {
  if (c->h16_unit != 0) return LSQR_OK;
  if (!c->d_h16_thr) HIPCHK(c, c->d_h16_thr.alloc(4 * 8192));
  float *d_probe = c->d_h16_thr;  // (the batch's threshold block: not in use yet)
  hipLaunchKernelGGL(k_dense_h16_probe, dim3(1), dim3(64), 0, c->stream, d_probe);
  // ... and 64 instructions of random operands (65 536 sums of 16 products and an addend against fp64)
  hipLaunchKernelGGL(k_dense_h16_probe_random, dim3(1), dim3(64), 0, c->stream, d_probe + kH16ProbeVariants, 64);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(c->h_pin->scratch, d_probe, sizeof(float) * (kH16ProbeVariants + 1), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, sync_stream(c));
  c->h16_unit_dev = dense_h16_probe_worst((const float *)c->h_pin->scratch);
  {
    const double rnd = (double)((const float *)c->h_pin->scratch)[kH16ProbeVariants];
    if (!(rnd <= c->h16_unit_dev)) c->h16_unit_dev = rnd;  // (a NaN is the worst)
  }
  c->h16_unit = c->h16_unit_dev <= kH16ProbeLimit ? 1 : -1;
  if (c->h16_unit < 0)
    (void)fail(c, LSQR_OK, "fp16 matrix-core filters: this device's matrix unit loses %.1f u per instruction (limit %.1f): fp32 filter used",
               c->h16_unit_dev, kH16ProbeLimit);
  return LSQR_OK;
}

// US calibrations: the frames as fp16 fragment pairs for us_h16.h's filter, once per upload (1 M frames: 192 MB).
// *ok = false when the filter cannot be used (magnitudes, the device's matrix unit): the packed fp32 filter scans.
template <class M>
constexpr bool kHasUsH16 = M::IS_US || requires { M::IS_PHANTOM; };
template <class M>
int ensure_us_h16(lsqr_ctx *c, bool *ok) {
  *ok = false;
  constexpr bool PH = requires { M::IS_PHANTOM; };
  constexpr bool SINGLE = PH || M::K == 4;
  const double X = c->mc.absmax, Rm = c->mc.absmax_rot;
  if (!c->absmax_valid || !(X > 0.0) || !(X < 1e15) || !(Rm > 0.0) || !(Rm < 1e15) || c->us16_nomem) return LSQR_OK;
  int st = h16_probe_unit(c);
  if (st != LSQR_OK) return st;
  if (c->h16_unit < 0) return LSQR_OK;
  const Us16Scales sc = us16_scales<SINGLE>(X, Rm);
  if (!c->us16_valid || memcmp(&sc, &c->us16_sc, sizeof sc) != 0) {
    const size_t n_tiles = (c->n + 31) / 32 + 2;
    constexpr size_t kTileElems = kUs16FrameTile / sizeof(uint4);
    if (n_tiles * kTileElems > c->d_us16.cap() && c->d_us16.alloc(n_tiles * kTileElems) != hipSuccess) {
      (void)hipGetLastError();  // (no room for the fragments: not an error -- the packed fp32 filter scans the records)
      c->us16_nomem = true;
      return LSQR_OK;
    }
    if constexpr (PH)  // (4 KiB per 32 frames of the 6 KiB the allocation holds)
      hipLaunchKernelGGL(k_phantom_rows_h16, dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, c->stream, c->d_data, c->stride,
                         c->n, sc, c->d_us16, n_tiles);
    else
      hipLaunchKernelGGL((k_us_rows_h16<SINGLE>), dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, c->stream, c->d_data,
                         c->stride, c->n, sc, c->d_us16, n_tiles);
    HIPCHK(c, hipGetLastError());
    c->us16_valid = true;
    c->us16_sc = sc;
  }
  if (!c->d_us16_x) HIPCHK(c, c->d_us16_x.alloc((size_t)(8192 / 32) * 4096 / sizeof(uint4)));
  if (!c->d_h16_thr) HIPCHK(c, c->d_h16_thr.alloc(4 * 8192));
  if (!c->d_amb) HIPCHK(c, c->d_amb.alloc(kAmbCap));
  if constexpr (PH)  // (every time: one flag per context served two kernels and missed the second)
    (void)hipFuncSetAttribute((const void *)k_scan_phantom_h16, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)phantom_h16_lds(kPh16HypChunk));
  else
    (void)hipFuncSetAttribute((const void *)k_scan_us_h16<SINGLE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)us_h16_lds(kUs16HypChunk));
  *ok = true;
  return LSQR_OK;
}
// frames [rb, re) against the H hypotheses whose scan parameters are `sp` (the batch or a compact selection): split of
// the unknowns, the filter in launches of 1024 hypotheses, the exact decision of the band
template <class M>
int launch_us_h16(lsqr_ctx *c, size_t rb, size_t re, const double *sp, uint32_t H, const uint32_t *h_dev,
                  const uint32_t *sel, const uint32_t *range_dev) {
  constexpr bool PH = requires { M::IS_PHANTOM; };
  constexpr bool SINGLE = PH || M::K == 4;
  unsigned int *d_segcnt = filter_scratch(c).segcnt;
  if constexpr (PH)
    hipLaunchKernelGGL(k_phantom_prep_h16, dim3((H + 31 + 255) / 256), dim3(256), 0, c->stream, sp, (int)M::SP, H,
                       sqrt(c->mc.delta_sq), c->mc.absmax, c->mc.absmax_rot, c->us16_sc, c->d_us16_x, c->d_h16_thr);
  else
    hipLaunchKernelGGL((k_us_prep_h16<SINGLE>), dim3((H + 31 + 255) / 256), dim3(256), 0, c->stream, sp, (int)M::SP, H,
                       c->mc.delta_sq, c->mc.absmax, c->mc.absmax_rot, c->us16_sc, c->d_us16_x, c->d_h16_thr);
  HIPCHK(c, hipGetLastError());
  const size_t passes = (re - rb + kUs16Wg - 1) / kUs16Wg;
  const unsigned nblk = (unsigned)std::min<size_t>(passes, 256);  // one workgroup (eight waves) per CU
  for (size_t h0 = 0; h0 < H; h0 += kUs16HypChunk) {
    const uint32_t hc = (uint32_t)std::min<size_t>(kUs16HypChunk, H - h0);
    if constexpr (PH)
      hipLaunchKernelGGL(k_scan_phantom_h16, dim3(nblk), dim3(kPh16Wg), phantom_h16_lds(hc), c->stream, c->d_us16, c->n, rb, re,
                         c->d_us16_x + (h0 / 32) * 256, c->d_h16_thr + 4 * h0, hc, c->d_votes, c->d_amb, d_segcnt, kSegCap,
                         (uint32_t)h0, h_dev, sel, range_dev);
    else
      hipLaunchKernelGGL((k_scan_us_h16<SINGLE>), dim3(nblk), dim3(kUs16Wg), us_h16_lds(hc), c->stream, c->d_us16, c->n, rb,
                         re, c->d_us16_x + (h0 / 32) * 128, c->d_h16_thr + 4 * h0, hc, c->d_votes, c->d_amb, d_segcnt, kSegCap,
                         (uint32_t)h0, h_dev, sel, range_dev);
    HIPCHK(c, hipGetLastError());
    // the exact decision of the band: the phantom after every launch (its 31-term sums leave ~3e-4 of the pairs there,
    // a workgroup's segment holds one launch's share, not four), the calibrations once
    if (PH || h0 + kUs16HypChunk >= H) {
      hipLaunchKernelGGL((k_us_recheck_seg<M>), dim3(256), dim3(1024), 0, c->stream, c->d_data, c->stride, c->d_hparams,
                         (int)M::SP, c->mc, c->d_amb, d_segcnt, kSegCap, c->d_votes, (unsigned int *)(c->d_counter + CNT_OVF));
      HIPCHK(c, hipGetLastError());
    }
  }
  return LSQR_OK;
}

// dense system, n = 64: the rows as fp16 fragment pairs for dense_h16.h's filter, once per upload (2 M x 64: 0.5 GB,
// ~1.9 ms).  *ok = false when the magnitudes do not fit the filter's scaling (the fp32 filter takes the scan).
int ensure_dense_h16(lsqr_ctx *c, bool *ok) {
  *ok = false;
  const double amax = c->mc.absmax_rot, bmax = c->mc.absmax;
  if (!(amax > 0.0) || !(amax < 1e15) || !(bmax < 1e15)) return LSQR_OK;
  const double pa = 32768.0 / amax;
  if (!(pa < 1e30) || !(bmax * pa < 1e18) || c->h16_nomem) return LSQR_OK;
  int stp = h16_probe_unit(c);
  if (stp != LSQR_OK) return stp;
  if (c->h16_unit < 0) return LSQR_OK;
  if (!c->h16_valid || c->h16_pa != pa) {
    const size_t n_tiles = (c->n + 31) / 32 + 8;  // a workgroup pass reads up to 255 rows past its last one
    if (n_tiles * 32 > c->d_h16_bs.cap()) {  // (the two grow together)
      c->d_h16.reset(), c->d_h16_bs.reset();
      // (no room for the second copy of the rows: not an error -- the fp32 filter scans the fp64 rows)
      if (c->d_h16.alloc(n_tiles * (kH16TileBytes / sizeof(uint4))) != hipSuccess ||
          c->d_h16_bs.alloc(n_tiles * 32) != hipSuccess) {
        (void)hipGetLastError();
        c->d_h16.reset(), c->d_h16_bs.reset();
        c->h16_nomem = true;
        return LSQR_OK;
      }
    }
    hipLaunchKernelGGL(k_dense_rows_h16, dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, c->stream, c->d_data,
                       c->stride, c->n, (int)c->cfg.dim, pa, c->d_h16, c->d_h16_bs, n_tiles);
    HIPCHK(c, hipGetLastError());
    c->h16_valid = true;
    c->h16_pa = pa;
  }
  if (!c->d_h16_thr) HIPCHK(c, c->d_h16_thr.alloc(4 * 8192));
  if (!c->h16_attr) {  // (per context: the attribute belongs to the device the context lives on)
    c->h16_attr = true;
    (void)hipFuncSetAttribute((const void *)k_scan_dense_h16<64>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)dense_h16_lds(1024));
  }
  *ok = true;
  return LSQR_OK;
}
// rows [rb, re) against hypotheses of `xh` / `thr4` (the batch itself or a compact selection), in launches of 1024
int launch_dense_h16(lsqr_ctx *c, size_t rb, size_t re, const _Float16 *xh, const float *thr4, uint32_t H,
                     const uint32_t *h_dev, const uint32_t *sel, const uint32_t *range_dev, size_t *nblk_out) {
  const size_t passes = (re - rb + kH16RowsPerWg - 1) / kH16RowsPerWg;
  const size_t nb = std::min<size_t>(passes, 512);  // two workgroups per CU
  const size_t rpb = (passes + nb - 1) / nb * kH16RowsPerWg;
  const size_t nblk = (re - rb + rpb - 1) / rpb;
  if (nblk_out) *nblk_out = nblk;
  for (size_t h0 = 0; h0 < H; h0 += 1024) {
    const uint32_t hc = (uint32_t)std::min<size_t>(1024, H - h0);
    hipLaunchKernelGGL((k_scan_dense_h16<64>), dim3((unsigned)nblk), dim3(256), dense_h16_lds(hc), c->stream, c->d_h16,
                       c->d_h16_bs, rb, re, rpb, xh + h0 * 128, thr4 + 4 * h0, hc, c->d_votes, c->d_amb,
                       filter_scratch(c).segcnt, kSegCap, (uint32_t)h0, h_dev, sel, range_dev);
    HIPCHK(c, hipGetLastError());
  }
  return LSQR_OK;
}

// rows [rb, re) against hypotheses of `rows` / `thr` (the batch itself or a compact selection): the fp32 filter (dense.h:
// k_scan_dense_mfma32r), hypothesis fragments prefetched through an LDS ring, in launches of 1024
int launch_dense_f32(lsqr_ctx *c, size_t rb, size_t re, const float *rows, const float *thr, uint32_t H,
                     const uint32_t *h_dev, const uint32_t *sel, const uint32_t *range_dev, size_t *nblk_out) {
  // two waves per SIMD (the A fragments live in registers): exactly two workgroups per CU
  const size_t tiles = (re - rb + 63) / 64;
  const size_t nb2 = std::min<size_t>(tiles, 512);
  const size_t rpb = (tiles + nb2 - 1) / nb2 * 64;
  const size_t nblk = (re - rb + rpb - 1) / rpb;
  if (nblk_out) *nblk_out = nblk;
  constexpr size_t kRingChunk = 1024;  // 62.7 KiB of LDS per workgroup: two per CU
  for (size_t h0 = 0; h0 < H; h0 += kRingChunk) {
    const uint32_t hc = (uint32_t)std::min<size_t>(kRingChunk, H - h0);
    const uint32_t nhb2 = (((hc + 63) / 64) + 1) & ~1u;
    const size_t lds = sizeof(float) * (8192 + 64 * kDmPitch32 + 64 + 128 * nhb2) + sizeof(uint32_t) * (hc + 1);
    hipLaunchKernelGGL((k_scan_dense_mfma32r<64>), dim3((unsigned)nblk), dim3(256), lds, c->stream, c->d_data,
                       c->stride, rb, re, rpb, rows + h0 * 64, thr + 2 * h0, hc, (int)c->cfg.dim, c->d_votes,
                       c->d_amb, filter_scratch(c).segcnt, kSegCap, (uint32_t)h0, h_dev, sel, range_dev);
    HIPCHK(c, hipGetLastError());
  }
  return LSQR_OK;
}
// the exact decision of the band the fp16 / fp32 filter left in its segments
int launch_dense_recheck_seg(lsqr_ctx *c, size_t nblk) {
  hipLaunchKernelGGL((k_dense_recheck_seg<64>), dim3((unsigned)nblk), dim3(256), 0, c->stream, c->d_data, c->stride,
                     c->d_hparams, c->mc, c->d_amb, filter_scratch(c).segcnt, kSegCap, c->d_votes,
                     (unsigned int *)(c->d_counter + CNT_OVF));
  HIPCHK(c, hipGetLastError());
  return LSQR_OK;
}
// the batch's operands of the fp16 (dense_h16.h) or the fp32 filter
int dense_filter_prep(lsqr_ctx *c, const FilterScratch &fs, bool h16) {
  const uint32_t H = (uint32_t)c->H;
  if (h16)  // the fp16 filter's rows live where the fp32 filter keeps its own (256 B per hypothesis either way)
    hipLaunchKernelGGL(k_dense_prep_h16, dim3((H + 3) / 4), dim3(256), 0, c->stream, c->d_hparams, H, (int)c->cfg.dim,
                       64, c->mc.delta, c->mc.absmax_rot, c->mc.absmax, c->h16_pa, (_Float16 *)fs.sp32, c->d_h16_thr);
  else
    hipLaunchKernelGGL(k_dense_thresholds32, dim3((H + 255) / 256), dim3(256), 0, c->stream, c->d_hparams, H,
                       (int)c->cfg.dim, 64, c->mc.delta, c->mc.absmax_rot, c->mc.absmax, fs.thr32, fs.sp32);
  HIPCHK(c, hipGetLastError());
  return LSQR_OK;
}
// diagnostics (LSQR_DENSE_DEBUG): how full the dense scan's worklist got (the exact kernel has emptied the segments by
// now: the fullest one is what it recorded; a launch's total is about that times the filter's workgroups)
static void dense_worklist_debug(lsqr_ctx *c) {
  static const bool dbg_on = getenv("LSQR_DENSE_DEBUG") != nullptr;
  if (dbg_on)
    fprintf(stderr, "dense scan: fullest worklist segment %u of %u (%zu rows x %zu hypotheses)\n", c->dense_amb_max, kSegCap,
            (size_t)c->n, (size_t)c->H);
}
// the dense fp16 / fp32 filter's worklist check: *fits = false (and the note) when the fp64 filter has to count instead
int dense_worklist_check(lsqr_ctx *c, bool *fits) {
  WorklistFill w;
  int st = worklist_check(c, kSegCap, &w);
  if (st != LSQR_OK) return st;
  *fits = w.state != WorklistFill::OVERFLOWED;
  if (w.state == WorklistFill::DEFERRED) return LSQR_OK;
  c->dense_amb_max = w.fill;
  dense_worklist_debug(c);
  if (!*fits)
    (void)fail(c, LSQR_OK, "dense fp16 / fp32 filter: worklist segment overflow (fill %u > %u), fp64 filter used",
               c->dense_amb_max, kSegCap);
  return LSQR_OK;
}

// dense system, n > 32: the fp32 matrix-core filter (dense.h: k_scan_dense_mfma32r) over row chunks and compacted
// selections; the band of every chunk is decided exactly (k_dense_recheck_seg) before the next selection looks at the
// votes.  Returns LSQR_OK with *done = false when a worklist segment overflowed (the caller counts everything with
// the fp64 filter instead).
int run_scan_dense_ee(lsqr_ctx *c, bool *done) {
  *done = false;
  EeBuf b;
  int st = ee_buffers(c, &b);
  if (st != LSQR_OK) return st;
  const uint32_t H = (uint32_t)c->H;
  const FilterScratch fs = filter_scratch(c);
  ProfScope whole(c, KID_SCAN);
  ProfMute mute(c);
  if ((st = worklist_reset(c, &fs)) != LSQR_OK) return st;
  bool h16 = false;
  if (c->opt.dense_f32 == 2 && (st = ensure_dense_h16(c, &h16)) != LSQR_OK) return st;
  if ((st = dense_filter_prep(c, fs, h16)) != LSQR_OK) return st;
  auto scan = [&](size_t rb, size_t re, const uint32_t *range_dev, const uint32_t *h_dev, const uint32_t *sel) -> int {
    if (rb >= re) return LSQR_OK;
    int s2 = h16 ? launch_dense_h16(c, rb, re, (const _Float16 *)(sel ? b.rows_c : fs.sp32), sel ? b.thr_c : c->d_h16_thr, H,
                                    h_dev, sel, range_dev, nullptr)
                 : launch_dense_f32(c, rb, re, sel ? b.rows_c : fs.sp32, sel ? b.thr_c : fs.thr32, H, h_dev, sel, range_dev,
                                    nullptr);
    return s2 != LSQR_OK ? s2 : launch_dense_recheck_seg(c, 512);
  };
  auto gather = [&](const uint32_t *sel, const uint32_t *n_dev) -> int {
    // (fp16: positions past the selection are never read, the scan takes its size from *n_dev)
    hipLaunchKernelGGL(k_ee_gather_f32, dim3((H + 3) / 4), dim3(256), 0, c->stream, sel, n_dev, H, (const float *)fs.sp32, 64,
                       b.rows_c, (const float *)(h16 ? c->d_h16_thr : fs.thr32), h16 ? 4 : 2, b.thr_c, h16 ? 0.0f : -1.0f);
    HIPCHK(c, hipGetLastError());
    return LSQR_OK;
  };
  if ((st = run_early_exit(c, 64, b, scan, gather)) != LSQR_OK) return st;
  if ((st = dense_worklist_check(c, done)) != LSQR_OK) return st;
  if (!*done) c->ee_last = false;
  return LSQR_OK;
}

// k_scan_us_f32 (the packed fp32 filter of the US calibrations / plane phantom): frames [rb, re) against the hc
// hypotheses of sp / spf, votes to `votes`
template <class M>
int launch_us_f32(lsqr_ctx *c, size_t rb, size_t re, const double *sp, const float *spf, uint32_t hc, uint32_t *votes,
                  const uint32_t *h_dev, const uint32_t *sel, const uint32_t *range_dev) {
  const int np = c->opt.ppl == 2 ? 1 : 2;  // pairs of frames per lane (scan_ppl 2 / 4)
  const size_t tile = (size_t)kBlock * 2 * np;
  const size_t tiles = (re - rb + tile - 1) / tile;
  const size_t lds = (size_t)hc * sizeof(uint32_t);
  int per_cu = (int)std::min<size_t>(8, (160 * 1024) / std::max<size_t>(lds, 1));
  if (per_cu < 1) per_cu = 1;
  const size_t max_blocks = (size_t)256 * per_cu;
  const size_t tpb = (tiles + max_blocks - 1) / max_blocks;
  const int grid = (int)((tiles + tpb - 1) / tpb);
  // few tiles (1 M frames = 977): split the hypothesis range over blockIdx.y to fill the chip
  unsigned ysplit = (unsigned)std::min<size_t>(std::max<size_t>(1, (size_t)256 * 5 / (size_t)grid),
                                               std::max<size_t>(1, hc / 256));
  if (c->opt.hsplit > 0) ysplit = (unsigned)c->opt.hsplit;
  if (np == 1)
    hipLaunchKernelGGL((k_scan_us_f32<M, 1>), dim3(grid, ysplit), dim3(kBlock), lds, c->stream, c->d_data, c->stride,
                       rb, re, sp, spf, hc, c->mc, votes, h_dev, sel, range_dev);
  else
    hipLaunchKernelGGL((k_scan_us_f32<M, 2>), dim3(grid, ysplit), dim3(kBlock), lds, c->stream, c->d_data, c->stride,
                       rb, re, sp, spf, hc, c->mc, votes, h_dev, sel, range_dev);
  HIPCHK(c, hipGetLastError());
  return LSQR_OK;
}

// US calibrations / plane phantom: k_scan_us_f32 over frame chunks and compacted selections
template <class M>
int run_scan_us_ee(lsqr_ctx *c) {
  EeBuf b;
  int st = ee_buffers(c, &b);
  if (st != LSQR_OK) return st;
  const uint32_t H = (uint32_t)c->H;
  const size_t tile = (size_t)kBlock * 2 * (c->opt.ppl == 2 ? 1 : 2);
  ProfScope whole(c, KID_SCAN);
  ProfMute mute(c);
  bool h16 = false;
  if constexpr (kHasUsH16<M>) {
    if (c->opt.us_h16 && H <= kFilterHypCap) {
      if ((st = ensure_us_h16<M>(c, &h16)) != LSQR_OK) return st;
      const FilterScratch fs = filter_scratch(c);
      if (h16 && (st = worklist_reset(c, &fs)) != LSQR_OK) return st;
    }
  }
  auto scan = [&](size_t rb, size_t re, const uint32_t *range_dev, const uint32_t *h_dev, const uint32_t *sel) -> int {
    if (rb >= re) return LSQR_OK;
    if constexpr (kHasUsH16<M>) {
      if (h16)  // fp16 matrix cores (us_h16.h); the band of every chunk is decided exactly before the next selection
        return launch_us_h16<M>(c, rb, re, sel ? c->d_hparams2 : c->d_hparams, H, h_dev, sel, range_dev);
    }
    return launch_us_f32<M>(c, rb, re, sel ? c->d_hparams2 : c->d_hparams, sel ? c->d_hparams2_f32 : c->d_hparams_f32, H,
                            c->d_votes, h_dev, sel, range_dev);
  };
  auto gather = [&](const uint32_t *sel, const uint32_t *n_dev) -> int {
    hipLaunchKernelGGL(k_gather_rows, dim3((H + 3) / 4), dim3(256), 0, c->stream, sel, n_dev, H, c->d_hparams,
                       (int)M::SP, c->d_hparams_f32, (int)M::SPF, c->d_hparams2, c->d_hparams2_f32);
    HIPCHK(c, hipGetLastError());
    return LSQR_OK;
  };
  if ((st = run_early_exit(c, tile, b, scan, gather)) != LSQR_OK) return st;
  if (!h16) return LSQR_OK;
  WorklistFill w;
  if ((st = worklist_check(c, kSegCap, &w)) != LSQR_OK) return st;
  if (w.state != WorklistFill::OVERFLOWED) return LSQR_OK;
  // a worklist segment that overflowed (not seen): everything again with the packed fp32 filter
  (void)fail(c, LSQR_OK, "US fp16 filter: worklist segment overflow (fill %u > %u), fp32 filter used", w.fill, kSegCap);
  const int keep = c->opt.us_h16;
  c->opt.us_h16 = 0;
  c->prof = mute.was;
  st = run_scan_us_ee<M>(c);
  c->opt.us_h16 = keep;
  return st;
}

// ---- the scan families: each either counts the batch (*done = true) or leaves it to the next one (run_scan) --------
// dense system, fp64 matrix-core filter + exact recheck of the ambiguous pairs; a worklist overflow leaves the batch
// to the exact kernel
template <class M>
int scan_dense_f64(lsqr_ctx *c, bool *done) {
  int st = worklist_reset(c, nullptr);
  if (st != LSQR_OK) return st;
  double *d_thr = filter_scratch(c).thr;  // scratch: 2 doubles per hypothesis (H <= 2^20 checked)
  if (c->H * 2 > (size_t)kDenseBlocks * 2160) return fail(c, LSQR_ERR_INVALID, "batch too large");
  size_t tiles = (c->n + 63) / 64;
  size_t nblk = std::min<size_t>(tiles, 768);  // 3 workgroups per CU
  size_t rpb = (tiles + nblk - 1) / nblk * 64;
  nblk = (c->n + rpb - 1) / rpb;
  {
    ProfScope ps(c, KID_SCAN);
    hipLaunchKernelGGL(k_dense_thresholds, dim3((unsigned)((c->H + 255) / 256)), dim3(256), 0, c->stream, c->d_hparams,
                       (uint32_t)c->H, (int)c->cfg.dim, (int)M::NR, c->mc.delta, c->mc.absmax, d_thr);
    HIPCHK(c, hipGetLastError());
    for (size_t h0 = 0; h0 < c->H; h0 += kDmHypChunk) {
      uint32_t hc = (uint32_t)std::min<size_t>(kDmHypChunk, c->H - h0);
      if constexpr (M::NR == 64) {
        {  // n = 64: B fragments in registers, no barriers per block
          size_t lds2 = sizeof(double) * (64 * kDmPitch + 64) + sizeof(uint32_t) * hc;
          hipLaunchKernelGGL((k_scan_dense_mfma2<64>), dim3((unsigned)nblk), dim3(256), lds2, c->stream, c->d_data,
                             c->stride, c->n, rpb, c->d_hparams + h0 * M::NR, d_thr + 2 * h0, hc, (int)c->cfg.dim,
                             c->d_votes + h0, c->d_amb, (unsigned int *)(c->d_counter + CNT_OVF), (uint32_t)h0);
          HIPCHK(c, hipGetLastError());
          continue;
        }
      }
      size_t lds = sizeof(double) * (2 * 64 * kDmPitch + 3 * 64) + sizeof(uint32_t) * hc;
      hipLaunchKernelGGL((k_scan_dense_mfma<M::NR>), dim3((unsigned)nblk), dim3(256), lds, c->stream, c->d_data,
                         c->stride, c->n, rpb, c->d_hparams + h0 * M::NR, d_thr + 2 * h0, hc, (int)c->cfg.dim,
                         c->d_votes + h0, c->d_amb, (unsigned int *)(c->d_counter + CNT_OVF), (uint32_t)h0);
      HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL((k_dense_recheck<M::NR>), dim3(64), dim3(256), 0, c->stream, c->d_data, c->stride, c->d_hparams,
                       c->mc, c->d_amb, (const unsigned int *)(c->d_counter + CNT_OVF), c->d_votes);
    HIPCHK(c, hipGetLastError());
  }
  // worklist overflow (never seen: ~1e-13 of the pairs are ambiguous) -> exact kernel
  WorklistFill w;
  if ((st = worklist_check(c, kAmbCap, &w)) != LSQR_OK) return st;
  *done = w.state != WorklistFill::OVERFLOWED;
  if (!*done)
    (void)fail(c, LSQR_OK, "dense fp64 filter: worklist overflow (fill %u > %u), exact kernel used", w.fill, kAmbCap);
  return LSQR_OK;
}
// default at n > 32: the filter in fp32 on the matrix cores (twice the fp64 MFMA rate); its band holds
// ~1e-4 of the pairs, decided exactly from a per-workgroup worklist.  A segment overflow (not seen)
// leaves the batch to the fp64 filter.
int scan_dense_f32(lsqr_ctx *c, bool *done) {
  const FilterScratch fs = filter_scratch(c);
  int st = worklist_reset(c, &fs);
  if (st != LSQR_OK) return st;
  bool h16 = false;  // fp16 matrix cores on two-way splits (dense_h16.h)
  if (c->opt.dense_f32 == 2 && (st = ensure_dense_h16(c, &h16)) != LSQR_OK) return st;
  {
    ProfScope ps(c, KID_SCAN);
    if ((st = dense_filter_prep(c, fs, h16)) != LSQR_OK) return st;
    size_t nblk = 0;
    st = h16 ? launch_dense_h16(c, 0, c->n, (const _Float16 *)fs.sp32, c->d_h16_thr, (uint32_t)c->H, nullptr, nullptr,
                                nullptr, &nblk)
             : launch_dense_f32(c, 0, c->n, fs.sp32, fs.thr32, (uint32_t)c->H, nullptr, nullptr, nullptr, &nblk);
    if (st != LSQR_OK || (st = launch_dense_recheck_seg(c, nblk)) != LSQR_OK) return st;
  }
  return dense_worklist_check(c, done);
}
// dense system.  default: MFMA filter + exact recheck of ambiguous pairs
template <class M>
int scan_dense(lsqr_ctx *c, bool *done) {
  if (!c->opt.filter) return LSQR_OK;
  int st = ensure_absmax(c);
  if (st != LSQR_OK) return st;
  if (!c->d_amb) HIPCHK(c, c->d_amb.alloc(kAmbCap));
  if (!(c->mc.absmax <= 1e100)) return LSQR_OK;  // finite, sane magnitudes: the filter's bound applies
  if constexpr (M::NR == 64) {
    // batch entry points: chunked early exit (earlyexit.h) -- hypotheses that can no longer become the running
    // maximum stop being counted
    if (c->allow_bound && c->opt.bound && c->opt.dense_f32 && c->H >= 128 &&
        c->H <= kEeCap && c->n >= 65536 && c->mc.absmax < 1e15)
      if ((st = run_scan_dense_ee(c, done)) != LSQR_OK || *done) return st;
  }
  HIPCHK(c, hipMemsetAsync(c->d_votes, 0, c->H * sizeof(uint32_t), c->stream));
  if constexpr (M::NR == 64) {
    if (c->opt.dense_f32 && c->H <= kFilterHypCap && c->mc.absmax < 1e15) {
      if ((st = scan_dense_f32(c, done)) != LSQR_OK || *done) return st;
      HIPCHK(c, hipMemsetAsync(c->d_votes, 0, c->H * sizeof(uint32_t), c->stream));   // overflow: fp64 filter
    }
  }
  return scan_dense_f64<M>(c, done);
}

// US calibrations / plane phantom: packed fp32 pre-filter (scan_filter 1); US: 2 = the fused fp64 filter
template <class M>
int scan_us(lsqr_ctx *c, bool *done) {
  if (!(c->opt.filter == 1 && c->absmax_valid && c->mc.absmax <= 1e15)) return LSQR_OK;
  *done = true;
  c->ee_last = false;
  if (c->allow_bound && c->opt.bound && c->H >= 256 && c->H <= kEeCap && c->n >= 65536)
    return run_scan_us_ee<M>(c);  // batch entry points: chunked early exit (earlyexit.h)
  int st;
  HIPCHK(c, hipMemsetAsync(c->d_votes, 0, c->H * sizeof(uint32_t), c->stream));
  if constexpr (kHasUsH16<M>) {
    if (c->opt.us_h16 && c->H >= 32 && c->H <= kFilterHypCap && c->n >= 4096) {  // fp16 matrix cores (us_h16.h)
      bool h16 = false;
      if ((st = ensure_us_h16<M>(c, &h16)) != LSQR_OK) return st;
      if (h16) {
        const FilterScratch fs = filter_scratch(c);
        if ((st = worklist_reset(c, &fs)) != LSQR_OK) return st;
        {
          ProfScope ps(c, KID_SCAN);
          if ((st = launch_us_h16<M>(c, 0, c->n, c->d_hparams, (uint32_t)c->H, nullptr, nullptr, nullptr)) != LSQR_OK) return st;
        }
        WorklistFill w;
        if ((st = worklist_check(c, kSegCap, &w)) != LSQR_OK) return st;
        if (w.state != WorklistFill::OVERFLOWED) return LSQR_OK;
        (void)fail(c, LSQR_OK, "US fp16 filter: worklist segment overflow (fill %u > %u), fp32 filter used", w.fill, kSegCap);
        HIPCHK(c, hipMemsetAsync(c->d_votes, 0, c->H * sizeof(uint32_t), c->stream));
      }
    }
  }
  for (size_t h0 = 0; h0 < c->H; h0 += kScanChunk) {
    uint32_t hc = (uint32_t)std::min<size_t>(kScanChunk, c->H - h0);
    ProfScope ps(c, KID_SCAN);
    if ((st = launch_us_f32<M>(c, 0, c->n, c->d_hparams + h0 * M::SP, c->d_hparams_f32 + h0 * M::SPF, hc, c->d_votes + h0,
                               nullptr, nullptr, nullptr)) != LSQR_OK)
      return st;
  }
  return LSQR_OK;
}

// plane, sphere, line: magnitudes the fp32 copies cannot hold (or NaN) go to the plain fp64 kernel
static bool f32_magnitudes_ok(const lsqr_ctx *c) { return c->absmax_valid && c->mc.absmax <= 1e15; }
// two-level scan over the spatial index; auto: built once an upload has seen enough
// hypotheses to pay for the build (a few HBM passes).  Returns whether this batch scans over the index (built here
// if need be) and its cell size.
template <class M>
bool scan_index_ready(lsqr_ctx *c, uint32_t *cell_pts_out) {
  typedef typename CellOf<M>::type CM;
  const bool tuned_defaults = c->opt.filter == 1 && c->opt.ppl == 0;  // A/B knobs untouched
  // Cost model of the build (auto mode).  Per (hypothesis, observation) the exhaustive filter kernel costs
  // ~1.9e-13 s and the two-level scan ~0.2e-13 s (10 M points x 4096 hypotheses: 7.6 ms against 0.8 ms);
  // the build costs ~1.2e-10 s per observation (radix sort + k-d refinement + gather; r03 without the
  // refinement: 0.7e-10).  It pays for itself once
  //   hypotheses still to come  >  1.2e-10 / 1.7e-13  ~  700,
  // and "still to come" is estimated by the larger of what the caller announced (lsqr_ransac: the current
  // numTries bound) and what this upload has been asked to scan so far, this batch included.
  constexpr uint64_t kIndexPaysAfter = 768;
  const uint64_t to_come = std::max<uint64_t>(c->hyp_expected, c->hyp_since_upload);
  const bool want = c->opt.filter && f32_magnitudes_ok(c) && c->mc.absmax >= 1e-10 && !c->index_failed &&
                    (c->opt.index == 2 ||
                     (c->opt.index == 1 && tuned_defaults &&
                      (c->index_valid || (c->n >= 65536 && to_come >= kIndexPaysAfter))));
  if (!want) return false;
  uint32_t cell_pts = c->opt.cell ? (uint32_t)c->opt.cell : (uint32_t)CM::DEFAULT_CELL;
  if constexpr (!requires { CM::MAX_PP; }) cell_pts = cell_pts > 512 ? 512 : cell_pts;
  *cell_pts_out = cell_pts;
  // the k-d levels above the runs: 5 - 12 % fewer surviving pairs for 4.5 ms more per build (10 M records) -- worth
  // it once an upload has been scanned by "scan_kd_after" hypotheses (what the caller announced does not count
  // here: the adaptive bound of a RANSAC run starts in the millions and collapses within a few batches)
  int kd_now = c->opt.refine && c->hyp_since_upload >= (uint64_t)c->opt.kd_after ? c->opt.kd_levels : 0;
  if constexpr (std::is_same<CM, PlaneCell<3>>::value) {
    // ... except for the plane's BOUNDED scan: its axis bound (axis.h: k_bound_axis) is tighter on the flat
    // Morton runs than on the more cubical k-d regions (166 against 207 of 4096 hypotheses reach the exact
    // count: 0.30 against 0.32 ms), while the full count gains 8 % from the levels.  So a bounded batch never
    // asks for them (an index that has them keeps them: no rebuilding back and forth), a counting one does.
    if (CM::USE_BOUND && c->allow_bound && c->opt.bound) kd_now = c->index_kd_levels;
  }
  if (!c->index_valid || c->cell_pts != cell_pts || kd_now > c->index_kd_levels) {
    c->kd_build_levels = kd_now;
    // the index is an accelerator: if it cannot be built (typically no memory for the sorted
    // copy) this upload keeps the exhaustive kernels instead of failing the scan
    if (build_index<M::ND>(c, cell_pts) != LSQR_OK) {
      (void)hipGetLastError();
      c->index_failed = true;
      return false;
    }
  }
  // the fp32 tiles of the index in place (nothing to do when they are there; a failed launch leaves the scans on
  // the sorted copy)
  if (build_tiles<CM>(c) != LSQR_OK) (void)hipGetLastError();
  return true;
}
// the plane's full count with the batch in key order (cells.h: k_plane_order): similar planes share a 64-group
template <class M>
int scan_plane_key_order(lsqr_ctx *c, uint32_t cell_pts) {
  typedef typename CellOf<M>::type CM;
  const uint32_t H = (uint32_t)c->H;
  uint32_t *perm = c->d_sel + kPilots, *cnt = (uint32_t *)(c->d_counter + CNT_FLAG);
  double *sp_b = c->d_hparams2 + (size_t)kPilots * M::SP;
  float *spf_b = c->d_hparams2_f32 + (size_t)kPilots * M::SPF;
  uint32_t *votes_b = c->d_votes2 + kPilots;
  hipLaunchKernelGGL((k_plane_order<M::SP>), dim3(1), dim3(1024), 0, c->stream, c->d_hparams, H, c->mc.absmax, perm, cnt);
  hipLaunchKernelGGL(k_gather_rows, dim3((H + 3) / 4), dim3(256), 0, c->stream, perm, cnt, H, c->d_hparams, (int)M::SP,
                     c->d_hparams_f32, (int)M::SPF, sp_b, spf_b);
  HIPCHK(c, hipGetLastError());
  const ScanBatch pb = {sp_b, spf_b, (size_t)H, votes_b, nullptr};
  int st2 = with_pp<CM>(cell_pts, [&](auto pp) { return run_scan_pairs<CM, decltype(pp)::value>(c, pb); });
  if (st2 != LSQR_OK) return st2;
  hipLaunchKernelGGL(k_scatter_perm, dim3((H + 255) / 256), dim3(256), 0, c->stream, perm, H, votes_b, c->d_votes);
  HIPCHK(c, hipGetLastError());
  return LSQR_OK;
}
// plane, sphere, line over the index: bounded, statically balanced or dynamically tiled
template <class M>
int scan_indexed(lsqr_ctx *c, bool *done) {
  typedef typename CellOf<M>::type CM;
  uint32_t cell_pts = 0;
  if (!scan_index_ready<M>(c, &cell_pts)) return LSQR_OK;
  // one cell per wave tile; several cells per tile and 128-record cells were measured dead ends
  //  and are no longer instantiated
  *done = true;
  c->last_bound[0] = 0;
  // batch entry points: hypotheses that cannot become the running maximum are not counted (the extra
  // launches only pay for batches of >= 1024; the selection kernels handle <= 8192)
  if (CM::USE_BOUND && c->allow_bound && c->opt.bound && c->H >= 1024 && c->H <= kSelCap && c->n_cells > 0)
    return with_pp<CM>(cell_pts, [&](auto pp) { return run_scan_bounded<CM, decltype(pp)::value>(c); });
  // plain scans of a large batch: the statically balanced kernel where it measured faster (plane, 10 M x
  // 4096: 1.13 against 1.24 ms; sphere and line are faster with tiles handed out dynamically);
  // "scan_pairs" 1 / 2 force one or the other (A/B)
  bool full_pairs = false;
  if constexpr (requires { CM::FULL_COUNT_PAIRS; }) full_pairs = c->opt.pairs == 0 && c->H >= 1024;
  if (c->opt.pairs == 1 || full_pairs) {
    if constexpr (std::is_same<CM, PlaneCell<3>>::value) {
      if (c->opt.hyp_order && c->H >= 1024 && c->H <= kOrderCap) return scan_plane_key_order<M>(c, cell_pts);
    }
    const ScanBatch b = {c->d_hparams, c->d_hparams_f32, c->H, c->d_votes, nullptr};
    return with_pp<CM>(cell_pts, [&](auto pp) { return run_scan_pairs<CM, decltype(pp)::value>(c, b); });
  }
  return with_pp<CM>(cell_pts, [&](auto pp) { return run_scan_cells<CM, decltype(pp)::value, 1>(c); });
}
// plane, sphere, line: fp32 pre-filter + exact re-evaluation
template <class M>
int scan_f32(lsqr_ctx *c, bool *done) {
  if (!(c->opt.filter && f32_magnitudes_ok(c))) return LSQR_OK;
  *done = true;
  int ppl = c->opt.ppl ? c->opt.ppl : 4;  // measured best (tools/ab_scan.py)
  // re-check granularity: per packed pair (line: wide band, ambiguous tiles are common) or per
  // tile; scan_filter 2 / 3 force one or the other for A/B runs
  const bool pair = c->opt.filter == 2 || (c->opt.filter == 1 && M::FGRAN == 1);
  if (pair) {
    if (ppl == 8) return run_scan_f32<M, 8, 1>(c);
    return run_scan_f32<M, 4, 1>(c);
  }
  if (ppl == 8) return run_scan_f32<M, 8>(c);
  if (ppl == 16) return run_scan_f32<M, 16>(c);
  return run_scan_f32<M, 4>(c);
}
// the exact kernels: every model, every magnitude
template <class M>
int scan_exact(lsqr_ctx *c) {
  if constexpr (M::REC <= 3) {  // point models: PPL is tunable
    int ppl = c->opt.ppl ? c->opt.ppl : 8;
    if (ppl == 2) return run_scan_ppl<M, 2>(c);
    if (ppl == 8) return run_scan_ppl<M, 8>(c);
    return run_scan_ppl<M, 4>(c);
  } else {
    return run_scan_ppl<M, M::PPL>(c);
  }
}

// the votes of the current batch: the first family that takes the batch (model, options, magnitudes) counts it
int run_scan(lsqr_ctx *c) {
  c->hyp_since_upload += c->H;
  c->ee_last = false;
  c->amb_reset = true;
  c->amb_counted = false;
  c->last_count.valid = false;
  return dispatch(c->cfg, [&](auto tag) -> int {
    typedef typename decltype(tag)::type M;
    bool done = false;
    int st = LSQR_OK;
    if constexpr (M::IS_DENSE) st = scan_dense<M>(c, &done);
    if (st != LSQR_OK || done) return st;
    if constexpr (requires { M::NF32; }) {
      st = scan_us<M>(c, &done);
    } else if constexpr (requires { M::SPF; }) {
      if constexpr (requires { typename CellOf<M>::type; }) st = scan_indexed<M>(c, &done);
      if (st == LSQR_OK && !done) st = scan_f32<M>(c, &done);
    }
    if (st != LSQR_OK || done) return st;
    return scan_exact<M>(c);
  });
}

// run_scan for the entry points that only need the first-max winner (and, for lsqr_ransac's replay, exact votes
// of the hypotheses that become the running maximum): the bounded scan may leave the rest uncounted
int run_scan_batch(lsqr_ctx *c, uint32_t best_before) {
  c->allow_bound = true;
  c->best_before = best_before;
  int st = run_scan(c);
  c->allow_bound = false;
  c->best_before = 0;
  return st;
}

// ---- moments / solves ---------------------------------------------------------------------------
// phase 0: the model's LS moment block about d_vec (origin); phase 1: LM block at d_vec (x trial)
// sum z z^T over rows [begin, end) of a row-major matrix whose rows hold n + 1 entries z
int launch_syrk(lsqr_ctx *c, const double *data, size_t stride, int n, int use_mask, size_t begin,
                size_t end, int *nmom) {
  const int ne = dense_ne(n), ps = dense_pstride(n);
  const auto [nb, chunk] = pass_shape(end - begin, kSyrkTile * 8, kDenseBlocks, kSyrkTile);
  *nmom = ne + 1;
  {
    ProfScope ps_(c, KID_MOMENTS);
    if (c->opt.filter) {  // default: matrix-core SYRK
      if (c->opt.syrk_diag == 1)  // diagnostics (tools/syrk_ab.py): loads only / MFMAs only
        hipLaunchKernelGGL(k_syrk_mfma<1>, dim3(nb), dim3(256), 0, c->stream, data, stride,
                           begin, end, chunk, n, c->d_mask, use_mask, ps, c->d_partials);
      else if (c->opt.syrk_diag == 2)
        hipLaunchKernelGGL(k_syrk_mfma<2>, dim3(nb), dim3(256), 0, c->stream, data, stride,
                           begin, end, chunk, n, c->d_mask, use_mask, ps, c->d_partials);
      else if (n + 1 <= 32)  // the plane phantom's 31 + 1 columns: two of the five column blocks
        hipLaunchKernelGGL((k_syrk_mfma<0, 2, 10>), dim3(nb), dim3(256), 0, c->stream, data, stride,
                           begin, end, chunk, n, c->d_mask, use_mask, ps, c->d_partials);
      else
        hipLaunchKernelGGL(k_syrk_mfma<0>, dim3(nb), dim3(256), 0, c->stream, data, stride,
                           begin, end, chunk, n, c->d_mask, use_mask, ps, c->d_partials);
    } else {
      size_t lds = sizeof(double) * kSyrkTile * ((n + 1) | 1) + kSyrkTile;
      hipLaunchKernelGGL(k_syrk_dense, dim3(nb), dim3(256), lds, c->stream, data, stride,
                         begin, end, chunk, n, c->d_mask, use_mask, ps, c->d_partials);
    }
    HIPCHK(c, hipGetLastError());
  }
  {
    ProfScope ps_(c, KID_SOLVE);
    hipLaunchKernelGGL(k_reduce, dim3(*nmom), dim3(64), 0, c->stream, c->d_partials, nb, ps, *nmom,
                       c->d_mom);
    HIPCHK(c, hipGetLastError());
  }
  return LSQR_OK;
}

int launch_moments_dense(lsqr_ctx *c, int use_mask, size_t begin, size_t end, int *nmom) {
  return launch_syrk(c, c->d_data, c->stride, (int)c->cfg.dim, use_mask, begin, end, nmom);
}

void phantom_to_out(const PhantomFit &f, SolveOut *out) {
  memset(out, 0, sizeof *out);
  out->ok = f.ok;
  out->n_params = f.ok ? PhantomModel::P : 0;
  out->lm_info = f.lm_info;
  out->lm_nfev = f.lm_nfev;
  out->cost = f.cost;
  for (int j = 0; j < PhantomModel::P; j++) out->params[j] = f.params[j];
}

// plane phantom: the Gram matrix of the data rows (upper triangle, 496 sums) + the row count.  The rows
// are materialised once per upload (256 B per frame) and summed on the matrix cores by the dense SYRK.
int launch_moments_phantom(lsqr_ctx *c, int use_mask, size_t begin, size_t end, int *nmom) {
  if (!c->rows_valid) {
    int st = ensure(c, c->d_rows, std::max<size_t>(c->n, 1) * 32);
    if (st != LSQR_OK) return st;
    ProfScope ps(c, KID_MOMENTS);
    hipLaunchKernelGGL(k_phantom_rows, dim3((unsigned)((c->n * 8 + 255) / 256)), dim3(256), 0, c->stream,
                       c->d_data, c->stride, c->n, c->d_rows);
    HIPCHK(c, hipGetLastError());
    c->rows_valid = true;
  }
  return launch_syrk(c, c->d_rows, 32, 30, use_mask, begin, end, nmom);
}

// plane phantom: both fits from the Gram block on the host (phantom.h)
void phantom_solve_block(const lsqr_model_cfg &cfg, const double *blk, SolveOut *out) {
  PhantomFit f;
  phantom_fit_block(blk, cfg.ls_type == LSQR_LS_ITERATIVE, &f);
  phantom_to_out(f, out);
}

// rows: the records the block in d_mom was summed over are at hand -- rows [begin, end) of the upload, those of the
// mask when use_mask -- so a system the elimination refuses is solved again from them in double-double (dense.h:
// k_gram_dd_dense / k_dense_dd_solve: the reference's SVD pseudo-inverse of A with its absolute rank test).  Without
// rows (lsqr_solve_moments, the multi-GPU sum of blocks) the pseudo-inverse of the Gram block decides.
int launch_solve_dense(lsqr_ctx *c, bool rows = false, int use_mask = 0, size_t begin = 0, size_t end = 0) {
  ProfScope ps(c, KID_SOLVE);
  const int n = (int)c->cfg.dim;
  int *flag = (int *)(c->d_counter + CNT_FLAG) + 1;  // (the low word of the slot is k_plane_order's count: another model's)
  rows = rows && c->opt.dense_dd && end > begin;
  if (rows) HIPCHK(c, hipMemsetAsync(flag, 0, sizeof(int), c->stream));
  hipLaunchKernelGGL(k_solve_dense, dim3(1), dim3(256), dense_lds_bytes(n), c->stream, c->d_mom, n,
                     c->opt.dense_fast, c->d_out, rows ? flag : (int *)nullptr);
  HIPCHK(c, hipGetLastError());
  if (!rows) return LSQR_OK;
  if (!c->d_ddpart) HIPCHK(c, c->d_ddpart.alloc((size_t)2 * kDdNe * kDdBlocks));
  const int nb = (int)std::min<size_t>(kDdBlocks, (end - begin + 31) / 32);
  hipLaunchKernelGGL((k_gram_dd_dense<32>), dim3(nb), dim3(256), 0, c->stream, c->d_data, c->stride, begin, end, n,
                     use_mask ? c->d_mask : (const uint8_t *)nullptr, flag, c->d_ddpart);
  HIPCHK(c, hipGetLastError());
  (void)hipFuncSetAttribute((const void *)k_dense_dd_solve, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)dense_dd_lds(64));
  hipLaunchKernelGGL(k_dense_dd_solve, dim3(1), dim3(256), dense_dd_lds(n), c->stream, c->d_ddpart, nb, n, c->d_mom,
                     flag, c->d_out);
  HIPCHK(c, hipGetLastError());
  return LSQR_OK;
}

// the closed-form solve of the block in d_mom about d_vec -> d_out (rows, use_mask, begin, end: launch_solve_dense)
template <class M>
int launch_solve(lsqr_ctx *c, bool rows = false, int use_mask = 0, size_t begin = 0, size_t end = 0) {
  if constexpr (M::IS_DENSE) {
    return launch_solve_dense(c, rows, use_mask, begin, end);
  } else {
    ProfScope ps(c, KID_SOLVE);
    hipLaunchKernelGGL((k_solve<M>), dim3(1), dim3(64), 0, c->stream, c->d_mom, c->d_vec, c->mc, c->d_out);
    HIPCHK(c, hipGetLastError());
    return LSQR_OK;
  }
}

template <class M>
int launch_moments(lsqr_ctx *c, int use_mask, size_t begin, size_t end, int phase, int *nmom) {
  if constexpr (requires { M::IS_PHANTOM; }) {
    (void)phase;  // the LM block at any x is a function of the Gram block
    return launch_moments_phantom(c, use_mask, begin, end, nmom);
  } else if constexpr (M::IS_DENSE) {
    if (phase != 0) return fail(c, LSQR_ERR_INVALID, "dense model has no iterative phase");
    return launch_moments_dense(c, use_mask, begin, end, nmom);
  } else {
    const auto [nb, chunk] = pass_shape(end - begin, mom_chunk(c), kMaxPartials, kBlock);
    {
      ProfScope ps(c, KID_MOMENTS);
      if (phase == 0) {
        *nmom = M::NMOM;
        if (use_mask)
          hipLaunchKernelGGL((k_moments<M, AccLs<M>, true>), dim3(nb), dim3(kBlock), 0, c->stream,
                             c->d_data, c->stride, begin, end, chunk, c->d_mask, c->d_vec, c->mc,
                             c->d_partials);
        else
          hipLaunchKernelGGL((k_moments<M, AccLs<M>, false>), dim3(nb), dim3(kBlock), 0, c->stream,
                             c->d_data, c->stride, begin, end, chunk, c->d_mask, c->d_vec, c->mc,
                             c->d_partials);
      } else {
        if constexpr (requires { M::NMOM_LM; }) {
          *nmom = M::NMOM_LM;
          if (use_mask)
            hipLaunchKernelGGL((k_moments<M, AccLm<M>, true>), dim3(nb), dim3(kBlock), 0, c->stream,
                               c->d_data, c->stride, begin, end, chunk, c->d_mask, c->d_vec, c->mc,
                               c->d_partials);
          else
            hipLaunchKernelGGL((k_moments<M, AccLm<M>, false>), dim3(nb), dim3(kBlock), 0,
                               c->stream, c->d_data, c->stride, begin, end, chunk, c->d_mask,
                               c->d_vec, c->mc, c->d_partials);
        } else {
          return fail(c, LSQR_ERR_INVALID, "model has no iterative phase");
        }
      }
      HIPCHK(c, hipGetLastError());
    }
    {
      ProfScope ps(c, KID_SOLVE);
      hipLaunchKernelGGL(k_reduce, dim3(*nmom), dim3(64), 0, c->stream, c->d_partials, nb,
                         (int)MOM_MAX, *nmom, c->d_mom);
      HIPCHK(c, hipGetLastError());
    }
    return LSQR_OK;
  }
}

int read_out(lsqr_ctx *c, SolveOut *o) {
  HIPCHK(c, hipMemcpyAsync(c->h_pin->scratch, c->d_out, sizeof(SolveOut), hipMemcpyDeviceToHost,
                           c->stream));
  HIPCHK(c, sync_stream(c));
  memcpy(o, c->h_pin->scratch, sizeof(SolveOut));
  return LSQR_OK;
}

// ---- the fit origin ------------------------------------------------------------------------------------------------
// The closed-form fits accumulate their moments about an origin and add it back in solve (rigid.h, models.h); the
// shift keeps the sums free of cancellation.  The origin must be finite and near the records that are summed, or it
// decides the result: a NaN / Inf origin makes every parameter NaN, a far one loses the rotation in rounding.  The
// rule, for every entry point (many.h takes the same records):
//   RANSAC finish (ORG_WINNER: the winner is known on the host, ORG_WINNER_DEV: k_best's packed value on the device)
//     - plane, line, sphere: the winner's own point in its scan row (fit_origin_offset);
//     - absolute orientation, ray, pivot (ORIGIN_FIRST: the parameters hold no point): the first drawn record of the
//       winning minimal subset -- finite and in the inlier cloud whenever the winner has votes;
//   masked fit without a winner (ORG_MASK: lsqr_set_mask, or an ORIGIN_FIRST model after lsqr_mask): the first record
//     whose mask bit is set; plane / line / sphere after a device mask: the point of the parameters it was made from;
//   unmasked fit (ORG_ALL): the first record, which is summed anyway.
enum FitOrigin { ORG_WINNER, ORG_WINNER_DEV, ORG_MASK, ORG_ALL };

// ORG_WINNER_DEV: the first drawn record of the subset of the packed winner (zeros without a winner: nothing agrees)
__global__ void k_winner_origin(const unsigned long long *__restrict__ packed, const uint32_t *__restrict__ subsets,
                                int K, const double *__restrict__ data, size_t stride, int nd,
                                double *__restrict__ org) {
  const unsigned long long pk = *packed;
  const int t = threadIdx.x;
  if (t >= nd) return;
  if (pk == 0) {
    org[t] = 0.0;
    return;
  }
  const size_t e = 0xFFFFFFFFull - (pk & 0xFFFFFFFFull);
  org[t] = data[(size_t)subsets[e * K] * stride + t];
}

// ORG_MASK: the smallest i < n with mask[i] != 0 -> *first (the caller sets it to ~0 first)
__global__ __launch_bounds__(kBlock) void k_first_masked(const uint8_t *__restrict__ mask, size_t n,
                                                         unsigned long long *__restrict__ first) {
  unsigned long long mine = ~0ull;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock)
    if (mask[i]) {  // ascending per lane: the lane's first hit is its smallest
      mine = i;
      break;
    }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long v = __shfl_down(mine, o);
    mine = v < mine ? v : mine;
  }
  if ((threadIdx.x & 63) == 0 && mine != ~0ull) atomicMin(first, mine);
}

// record *idx -> org (zeros for ~0: an empty mask, the fit comes out empty)
__global__ void k_record_origin(const unsigned long long *__restrict__ idx, const double *__restrict__ data,
                                size_t stride, int nd, double *__restrict__ org) {
  const int t = threadIdx.x;
  if (t >= nd) return;
  const unsigned long long i = *idx;
  org[t] = i == ~0ull ? 0.0 : data[(size_t)i * stride + t];
}

// the fit origin -> d_vec (ORG_WINNER: d_par holds the winner's scan row and c->win_rec its first drawn record;
// ORG_WINNER_DEV: d_counter[CNT_BEST] its packed value and d_subsets the batch's subsets)
int set_fit_origin(lsqr_ctx *c, FitOrigin how) {
  return dispatch(c->cfg, [&](auto tag) -> int {
    typedef typename decltype(tag)::type M;
    if constexpr (M::IS_DENSE || requires { M::IS_PHANTOM; }) {
      return LSQR_OK;
    } else {
      const int off = fit_origin_offset<M>(c->cfg);  // (many.h: lsqr_ransac_many takes the same origin)
      const bool own_point = how == ORG_WINNER || how == ORG_WINNER_DEV || (how == ORG_MASK && c->origin_valid);
      if (off >= 0 && own_point) {
        HIPCHK(c, hipMemcpyAsync(c->d_vec, c->d_par + off, sizeof(double) * M::ND, hipMemcpyDeviceToDevice,
                                 c->stream));
      } else if (how == ORG_WINNER || how == ORG_ALL) {
        const size_t r = how == ORG_WINNER ? (size_t)c->win_rec : 0;
        if (r >= c->n) return fail(c, LSQR_ERR_STATE, "fit origin: record %zu of %zu", r, c->n);
        HIPCHK(c, hipMemcpyAsync(c->d_vec, c->d_data + r * c->stride, sizeof(double) * M::ND,
                                 hipMemcpyDeviceToDevice, c->stream));
      } else if (how == ORG_WINNER_DEV) {
        hipLaunchKernelGGL(k_winner_origin, dim3(1), dim3(64), 0, c->stream, c->d_counter + CNT_BEST, c->d_subsets, c->K,
                           c->d_data, c->stride, (int)M::ND, c->d_vec);
        HIPCHK(c, hipGetLastError());
      } else {  // ORG_MASK
        unsigned long long *first = c->d_counter + CNT_FIRST;
        HIPCHK(c, hipMemsetAsync(first, 0xFF, sizeof(unsigned long long), c->stream));
        hipLaunchKernelGGL(k_first_masked, dim3(grid_for(c->n, kBlock * 16, 1024)), dim3(kBlock), 0, c->stream,
                           c->d_mask, c->n, first);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(k_record_origin, dim3(1), dim3(64), 0, c->stream, first, c->d_data, c->stride,
                           (int)M::ND, c->d_vec);
        HIPCHK(c, hipGetLastError());
      }
      return LSQR_OK;
    }
  });
}

// the closed-form part of run_fit without the read-back: moments + solve chained on the stream, result in
// d_out.  Models whose fit needs the host in the loop (LM, the phantom's Gram solve) are refused.
// have_origin: the caller has put the fit origin into d_vec (set_fit_origin)
template <class M>
int enqueue_closed_fit(lsqr_ctx *c, int use_mask, bool have_moments, bool have_origin) {
  int nmom = 0, st;
  if constexpr (M::IS_DENSE) {
    if (!have_moments && (st = launch_moments_dense(c, use_mask, 0, c->n, &nmom)) != LSQR_OK) return st;
  } else if (!have_moments) {
    if (!have_origin && (st = set_fit_origin(c, use_mask ? ORG_MASK : ORG_ALL)) != LSQR_OK) return st;
    if ((st = launch_moments<M>(c, use_mask, 0, c->n, 0, &nmom)) != LSQR_OK) return st;
  }
  return launch_solve<M>(c, true, use_mask, 0, c->n);
}
int enqueue_fit(lsqr_ctx *c, int use_mask, bool have_moments = false, bool have_origin = false) {
  if (wants_lm(c->cfg) || c->cfg.model == LSQR_MODEL_PHANTOM)
    return fail(c, LSQR_ERR_INVALID, "this fit needs the host between device passes");
  return dispatch(c->cfg, [&](auto tag) -> int {
    return enqueue_closed_fit<typename decltype(tag)::type>(c, use_mask, have_moments, have_origin);
  });
}

// ---- persistent LM fit (lm_persist.h) -------------------------------------------------------------------------------
// Compute-unit tokens: the persistent kernels of this process never ask for more workgroups than the device holds
// (one per compute unit: the kernel's LDS request), so none of them can wait for a workgroup that another one keeps
// from becoming resident.  A fit draws G tokens before it launches and returns them when its kernel has ended.
struct LmpPool {
  std::mutex mu;
  std::condition_variable cv;
  int cus[16] = {0}, free_[16] = {0}, live[16] = {0};  // per device: compute units, free tokens, root contexts alive
  // contexts that started a persistent fit lately: how many ways the device is shared (a process with four contexts
  // of which one is fitting gives that one the whole device)
  std::vector<std::pair<const void *, double>> recent[16];
};
LmpPool &lmp_pool() {
  static LmpPool p;
  return p;
}
void lmp_ctx_count(int device, int d, const void *who = nullptr) {
  if (device < 0 || device >= 16) return;
  LmpPool &p = lmp_pool();
  std::lock_guard<std::mutex> lk(p.mu);
  p.live[device] += d;
  if (who) {  // a context that is gone is not fitting any more
    auto &rec = p.recent[device];
    for (auto it = rec.begin(); it != rec.end();) it = it->first == who ? rec.erase(it) : it + 1;
  }
}
int lmp_acquire(int device, const void *who, int forced, int need_max, bool only_if_alone) {
  LmpPool &p = lmp_pool();
  std::unique_lock<std::mutex> lk(p.mu);
  if (device < 0 || device >= 16) return 0;
  if (!p.cus[device]) {
    int cu = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cu <= 0) return 0;
    p.cus[device] = p.free_[device] = cu;
  }
  int G = forced;
  {  // the device shared evenly by the contexts that have been fitting in the last half second (up to eight)
    const double now = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    auto &rec = p.recent[device];
    bool mine = false;
    int active = 0;
    for (auto it = rec.begin(); it != rec.end();) {
      if (it->first == who) {
        it->second = now;
        mine = true;
      }
      if (now - it->second > 0.5) {
        it = rec.erase(it);
        continue;
      }
      active++;
      ++it;
    }
    if (!mine) {
      rec.push_back({who, now});
      active++;
    }
    // "lm_persist" 1 (the default): several fits in flight are served better by the launch path -- their passes overlap
    // each other's host round trips and the aggregate is HBM-bound either way (r05: 70 k hypotheses/s on eight streams
    // of launches against 36 - 60 k on four to eight persistent fits) --, a fit alone on the device by the persistent
    // kernel (31 k against 26 - 27 k)
    if (only_if_alone && active > 1) return 0;
    if (G <= 0) {
      const int share = std::max(1, std::min(8, active));
      G = p.cus[device] / share;
      int pw = 1;
      while (2 * pw <= G) pw *= 2;
      G = pw;
    }
  }
  G = std::max(1, std::min({G, p.cus[device], need_max}));
  p.cv.wait(lk, [&] { return p.free_[device] >= G; });
  p.free_[device] -= G;
  return G;
}
void lmp_release(int device, int G) {
  LmpPool &p = lmp_pool();
  {
    std::lock_guard<std::mutex> lk(p.mu);
    p.free_[device] += G;
  }
  p.cv.notify_all();
}

// The moment block of evaluation `tag` out of the pinned granules `res` (host_entry.h: lm_granule_decode), polled in
// order.  LM_LEFT: the stream has drained and the block is not there -- whatever was to publish it has ended without
// doing so; LM_STREAM_ERROR: the stream reports *err.
enum LmWait { LM_GOT, LM_LEFT, LM_STREAM_ERROR };
LmWait lm_wait_block(lsqr_ctx *c, const volatile unsigned long long *res, uint32_t tag, int nmom, double *blk,
                     hipError_t *err) {
  unsigned long long spins = 0;
  for (int j = 0; j < nmom; j++)
    while (!lm_granule_decode(res, j, tag, &blk[j])) {
      if ((++spins & 0xFFFF) != 0) continue;  // every 65 k polls: is the stream still alive?
      const hipError_t q = hipStreamQuery(c->stream);
      if (q != hipSuccess && q != hipErrorNotReady) {
        *err = q;
        return LM_STREAM_ERROR;
      }
      if (q == hipSuccess && !lm_granule_decode(res, j, tag, &blk[j])) return LM_LEFT;
    }
  return LM_GOT;
}

struct LmSet {  // lm_settings of the model
  int n, maxfev;
  double ftol, xtol, gtol;
};

// *done = true: finished, `s` holds the final state; false: not run or given up (the caller takes the launch path)
template <class M>
int lm_persist_fit(lsqr_ctx *c, const double *tiles, size_t cnt, int nb, LmState &s, const double *x0, const LmSet &t,
                   bool *done) {
  *done = false;
  static const bool shared_gpu = getenv("LSQR_SHARE_GPU") != nullptr;  // several processes on one device: no tokens across them
  if (!c->opt.lm_persist || shared_gpu || c->is_lane) return LSQR_OK;
  typedef typename M::LmCoef Coef;
  constexpr int NCW = (int)(sizeof(Coef) / 8), NMOM = (int)M::NMOM_LM;
  if (!c->d_lmp) {
    if (c->d_lmp.alloc(1) != hipSuccess) return LSQR_OK;
    if (c->h_lmcmd.alloc(256) != hipSuccess) {
      c->d_lmp.reset();
      return LSQR_OK;
    }
    memset(c->h_lmcmd, 0, sizeof(unsigned long long) * 256);
  }
  if (c->lm_seq > 0xF0000000u) {  // tags would wrap: start again from clean granules (nothing is in flight here)
    HIPCHK(c, sync_stream(c));
    memset(c->h_lmcmd, 0, sizeof(unsigned long long) * 256);
    memset(c->h_lmres, 0, sizeof(unsigned long long) * 256);
    c->lm_seq = 0;
  }
  const int host_step = c->opt.lm_persist != 2;
  // one round of virtual blocks when the device is ours alone (512-thread workgroups: two blocks at a time each)
  const int G = lmp_acquire(c->device, c, c->opt.lm_persist_wgs, (nb + 1) / 2, c->opt.lm_persist == 1);  // tokens held
  if (G <= 0) return LSQR_OK;
  // workgroups of eight waves (two virtual blocks at a time) when the tokens cover all blocks in one round -- the pass
  // then spreads over twice the compute units --, else sixteen waves (four blocks at a time)
  const int threads = G * 2 >= nb ? 512 : 1024;
  const int Gl = threads == 512 ? G : std::min(G, (nb + 3) / 4);  // workgroups launched
  const size_t lds = std::max<size_t>((size_t)(threads / 64) * 64 * 17 * sizeof(double), (size_t)96 << 10);
  // a fit that has the device to itself in one round keeps its tiles in registers (k_lm_persist<M, 4>: 512 threads)
  const bool resident = host_step && threads == 512 && (size_t)Gl * 2 >= (size_t)nb && c->opt.lm_persist_resident;
  auto give_up = [&](int rc) {  // every way out before the kernel has ended and the tokens have gone back
    lmp_release(c->device, G);
    return rc;
  };
  if (hipFuncSetAttribute((const void *)k_lm_persist<M, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 << 10) !=
          hipSuccess ||
      hipFuncSetAttribute((const void *)k_lm_persist<M, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 << 10) !=
          hipSuccess)
    return give_up(LSQR_OK);
  LmpInit init{};
  init.n = t.n;
  init.maxfev = t.maxfev;
  init.ftol = t.ftol;
  init.xtol = t.xtol;
  init.gtol = t.gtol;
  init.factor = 100.0;
  for (int j = 0; j < LM_NMAX; j++) init.x0[j] = j < t.n ? x0[j] : 0.0;
  const uint32_t seq0 = c->lm_seq;
  c->lm_seq += (uint32_t)t.maxfev + 8;
  const unsigned long long timeout = (unsigned long long)std::max(1, c->opt.lm_persist_timeout_ms) * 100000ULL;  // 100 MHz
  if (hipMemsetAsync(c->d_lmp, 0, sizeof(LmpCtl), c->stream) != hipSuccess) return give_up(LSQR_OK);
  {
    ProfScope ps(c, KID_MOMENTS);
    auto launch = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(Gl), dim3(threads), lds, c->stream, tiles, cnt, nb, c->d_lmp, c->d_partials,
                         c->h_lmres, c->h_lmcmd, c->d_lm, c->d_out, init, seq0, host_step, timeout,
                         (uint32_t)c->opt.lm_persist_test_abort);
    };
    if (resident) launch(k_lm_persist<M, 4>);
    else launch(k_lm_persist<M, 0>);
  }
  if (hipGetLastError() != hipSuccess) return give_up(LSQR_OK);
  bool gave_up = false;
  uint64_t host_wait_ns = 0, host_step_ns = 0;
  if (host_step) {
    lm_init(s, t.n, x0, t.ftol, t.xtol, t.gtol, t.maxfev, 100.0);
    volatile unsigned long long *cmd = c->h_lmcmd;
    for (uint32_t e = 1;; e++) {
      const uint32_t tag = seq0 + e;
      double blk[LM_MOM_MAX];
      hipError_t q = hipSuccess;
      const auto tw0 = std::chrono::steady_clock::now();
      const LmWait w = lm_wait_block(c, c->h_lmres, tag, NMOM, blk, &q);
      if (w == LM_STREAM_ERROR)
        return give_up(fail(c, LSQR_ERR_HIP, "persistent LM kernel failed: %s", hipGetErrorString(q)));
      if (w == LM_LEFT) {  // the kernel left (a bounded wait expired) without this evaluation
        gave_up = true;
        break;
      }
      const auto tw1 = std::chrono::steady_clock::now();
      const bool cont = lm_advance(s, blk);
      uint32_t words[2 * LMP_MAXCOEF] = {0};
      if (cont) {
        Coef k;
        M::lm_coef(s.xtrial, k);
        memcpy(words, &k, sizeof(Coef));
      }
      for (int i = 0; i < 2 * NCW; i++) cmd[i] = ((unsigned long long)words[i ^ 1] << 32) | tag;
      std::atomic_thread_fence(std::memory_order_release);  // the command granule is what the device polls: written last
      cmd[2 * NCW] = ((unsigned long long)(cont ? LMP_EVAL : LMP_FIN) << 32) | tag;
      host_wait_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(tw1 - tw0).count();
      host_step_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - tw1).count();
      if (!cont) break;
    }
  }
  hipError_t se = sync_stream(c);
  lmp_release(c->device, G);
  if (se != hipSuccess) return fail(c, LSQR_ERR_HIP, "persistent LM kernel: %s", hipGetErrorString(se));
  LmpCtl *hc = &c->h_pin->lmp;  // (an area of its own, PinLayout: finish_ransac reads mask_head after the fit)
  HIPCHK(c, hipMemcpy(hc, c->d_lmp, sizeof(LmpCtl), hipMemcpyDeviceToHost));
  c->lmp_last[0] = (uint64_t)c->opt.lm_persist;
  c->lmp_last[1] = (uint64_t)Gl;
  c->lmp_last[2] = hc->evals;
  c->lmp_last[3] = hc->status;
  c->lmp_last[4] = (hc->t_end - hc->t_begin) / 100;  // us
  c->lmp_last[6] = host_wait_ns;
  c->lmp_last[7] = host_step_ns;
  c->lmp_trace_n = std::min<uint32_t>(hc->evals, LMP_TRACE);
  memcpy(c->lmp_trace, hc->trace, sizeof(hc->trace));
  if (gave_up || hc->status != LMP_FIN) {
    c->lmp_last[5]++;
    return LSQR_OK;
  }
  if (!host_step) HIPCHK(c, hipMemcpy(&s, c->d_lm, sizeof(LmState), hipMemcpyDeviceToHost));
  *done = true;
  return LSQR_OK;
}

// ---- the iterative fit: three drivers of one minimisation (lm_core.h) -------------------------------------------------
// the matrix-core pass pays when the (J | f) rows are wide (US: 12 / 9 columns, 78 / 45 sums); for the sphere's 5
// columns the 16 x 16 tile is mostly padding and the instruction time alone (25 us at 3.8 M points) exceeds the
// per-lane version's whole pass
template <class M>
bool lm_mfma_pass(const lsqr_ctx *c) {
  return c->opt.lm_mfma && M::NLM >= 8;
}

// what an evaluation of the fused driver reads -- the upload, through the mask or not, or the compacted consensus
// set -- and how the pass is cut into blocks
struct LmPassSet {
  const double *data;
  size_t stride, cnt;
  bool through_mask;
  bool tiles;  // compacted in tiles of 64 records, field-major (kernels.h: k_compact_write_tiles)
  int nb;
  size_t chunk;
};

// the consensus set, tight and in order (every evaluation then streams n_in records, all lanes busy) -> d_lmrec
template <class M>
int lm_compact(lsqr_ctx *c, LmPassSet &w) {
  const bool tile_layout = lm_mfma_pass<M>(c) && c->opt.lm_tiles;
  double *pin = c->h_pin->scratch_f64;
  const auto [cb, cchunk] = pass_shape(c->n, kBlock * 8, 1024, kBlock);  // (c->n > 0: need_ready(c, true))
  uint32_t *d_cnt = (uint32_t *)c->d_partials.get(), *d_off = d_cnt + 1024;  // scratch (4.4 MB buffer)
  hipLaunchKernelGGL(k_compact_count, dim3(cb), dim3(kBlock), 0, c->stream, c->d_mask, c->n, cchunk, d_cnt);
  hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, c->stream, d_cnt, cb, d_off);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(pin + 200, d_off + cb, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, sync_stream(c));
  w.cnt = *(const uint32_t *)(pin + 200);
  int st = ensure(c, c->d_lmrec, ((std::max<size_t>(w.cnt, 1) + 63) & ~(size_t)63) * M::ND);
  if (st != LSQR_OK) return st;
  if (tile_layout)  // the matrix-core pass reads tiles of 64 records stored field-major (kernels.h)
    hipLaunchKernelGGL((k_compact_write_tiles<M::ND>), dim3(cb), dim3(kBlock), 0, c->stream, c->d_data, c->stride,
                       c->d_mask, c->n, cchunk, d_off, c->d_lmrec);
  else
    hipLaunchKernelGGL((k_compact_write<M::ND>), dim3(cb), dim3(kBlock), 0, c->stream, c->d_data, c->stride,
                       c->d_mask, c->n, cchunk, d_off, c->d_lmrec);
  HIPCHK(c, hipGetLastError());
  w.data = c->d_lmrec;
  w.stride = M::ND;
  w.through_mask = false;
  w.tiles = tile_layout;
  return LSQR_OK;
}

void lm_shape(LmPassSet &w, bool mfma_pass) {
  if (w.tiles) {  // four tiles per wave and more: one in flight behind the one being evaluated
    w.nb = (int)std::min<size_t>(512, std::max<size_t>(1, (w.cnt + 1023) / 1024));
    w.chunk = 0;
    return;
  }
  const PassShape ps = pass_shape(w.cnt, kBlock * (mfma_pass ? 2 : 8), kMaxPartials, kBlock);
  w.nb = ps.nb;
  w.chunk = ps.chunk;
}

// the sums of one evaluation at xk -> d_partials (w.nb blocks)
template <class M>
int lm_launch_pass(lsqr_ctx *c, const LmPassSet &w, const LmX &xk) {
  bool launched = false;
  if constexpr (requires { typename M::LmCoef; }) {
    if (lm_mfma_pass<M>(c)) {
      typename M::LmCoef coef;
      M::lm_coef(xk.x, coef);
      if (w.tiles)
        hipLaunchKernelGGL((k_lm_pass_mfma_t<M>), dim3(w.nb), dim3(kBlock), 0, c->stream, w.data, w.cnt, coef,
                           c->d_partials);
      else
        hipLaunchKernelGGL((k_lm_pass_mfma<M>), dim3(w.nb), dim3(kBlock), 0, c->stream, w.data, w.stride, w.cnt, coef,
                           c->mc, c->d_partials);
      launched = true;
    }
  }
  if (!launched) {
    auto launch = [&](auto kern, const uint8_t *mask) {
      hipLaunchKernelGGL(kern, dim3(w.nb), dim3(kBlock), 0, c->stream, w.data, w.stride, (size_t)0, w.cnt, w.chunk, mask,
                         xk, c->mc, c->d_partials);
    };
    if (w.through_mask) launch(k_lm_pass<M, true>, (const uint8_t *)c->d_mask);
    else launch(k_lm_pass<M, false>, (const uint8_t *)nullptr);
  }
  HIPCHK(c, hipGetLastError());
  return LSQR_OK;
}

// The host's step and one launch per evaluation: trial point by value, block sums + final sum in the same kernel, the
// result lands in pinned host memory and the host polls its sequence flag (no stream synchronisation, no staging
// copies): per evaluation = the pass + one launch latency + a few hundred host flops.
// Compacting the consensus set costs about as much as six evaluations through the mask save (10 M records, 38 %
// inliers: count + scan + host read-back + write = 130 us; a pass over the compacted set is 23 us against 43 us), and
// the sphere's geometric fit from the algebraic start typically needs three: the per-lane pass starts THROUGH THE MASK
// and the set is compacted once `kCompactAfter` evaluations have been spent.  The matrix-core pass (US: thousands of
// evaluations) reads compacted records only and compacts at once.
template <class M>
int lm_fit_fused(lsqr_ctx *c, int use_mask, const LmSet &t, const double *x0, LmState &s) {
  constexpr int kCompactAfter = 8;
  const bool mfma_pass = lm_mfma_pass<M>(c);
  LmPassSet w{c->d_data, c->stride, c->n, use_mask != 0, false, 1, 0};
  int st;
  if (use_mask && mfma_pass && (st = lm_compact<M>(c, w)) != LSQR_OK) return st;
  lm_shape(w, mfma_pass);
  bool persist_done = false;
  if constexpr (requires { typename M::LmCoef; }) {
    if (mfma_pass && w.tiles) {  // the whole fit in one launch (lm_persist.h); falls through when it gives up
      if ((st = lm_persist_fit<M>(c, w.data, w.cnt, w.nb, s, x0, t, &persist_done)) != LSQR_OK) return st;
    }
  }
  if (!persist_done) lm_init(s, t.n, x0, t.ftol, t.xtol, t.gtol, t.maxfev, 100.0);
  while (!persist_done) {
    if (w.through_mask && s.nfev >= kCompactAfter) {
      if ((st = lm_compact<M>(c, w)) != LSQR_OK) return st;
      lm_shape(w, mfma_pass);
    }
    LmX xk;
    for (int j = 0; j < LM_NMAX; j++) xk.x[j] = j < t.n ? s.xtrial[j] : 0.0;
    uint32_t seq = ++c->lm_seq;
    if (seq == 0) seq = c->lm_seq = 1;  // (the zero-initialised granules carry tag 0)
    // profiling: every 16th evaluation carries event pairs (four event records per evaluation would cost
    // more host time than the evaluation's own launches); lsqr_profile_get's averages are unaffected
    const bool timed = c->prof && (s.nfev & 15) == 0;
    const bool prof_saved = c->prof;
    c->prof = timed;
    {
      ProfScope ps(c, KID_MOMENTS);
      if ((st = lm_launch_pass<M>(c, w, xk)) != LSQR_OK) return st;
    }
    {
      ProfScope ps(c, KID_SOLVE);
      hipLaunchKernelGGL(k_lm_publish, dim3((unsigned)M::NMOM_LM), dim3(64), 0, c->stream, c->d_partials, w.nb,
                         (int)M::NMOM_LM, c->h_lmres, seq);
      HIPCHK(c, hipGetLastError());
    }
    c->prof = prof_saved;
    double blk[LM_MOM_MAX];
    hipError_t q = hipSuccess;
    switch (lm_wait_block(c, c->h_lmres, seq, (int)M::NMOM_LM, blk, &q)) {
      case LM_STREAM_ERROR: return fail(c, LSQR_ERR_HIP, "LM pass failed: %s", hipGetErrorString(q));
      case LM_LEFT: return fail(c, LSQR_ERR_HIP, "LM pass finished without publishing its result");
      case LM_GOT: break;
    }
    if (!lm_advance(s, blk)) break;
  }
  HIPCHK(c, sync_stream(c));
  return LSQR_OK;
}

// the host's step through staged copies ("lm_fused" 0): trial point up, launch_moments, block down, per evaluation
template <class M>
int lm_fit_staged(lsqr_ctx *c, int use_mask, const LmSet &t, const double *x0, LmState &s) {
  lm_init(s, t.n, x0, t.ftol, t.xtol, t.gtol, t.maxfev, 100.0);
  double *pin = c->h_pin->scratch_f64;
  for (;;) {
    int nmom = 0, st;
    for (int j = 0; j < t.n; j++) pin[j] = s.xtrial[j];
    HIPCHK(c, hipMemcpyAsync(c->d_vec, pin, sizeof(double) * t.n, hipMemcpyHostToDevice, c->stream));
    if ((st = launch_moments<M>(c, use_mask, 0, c->n, 1, &nmom)) != LSQR_OK) return st;
    HIPCHK(c, hipMemcpyAsync(pin + 64, c->d_mom, sizeof(double) * nmom, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, sync_stream(c));
    if (!lm_advance(s, pin + 64)) return LSQR_OK;
  }
}

// the step in a device kernel ("lm_host" 0), from the algebraic result in d_out; every evaluation reads `out` back
template <class M>
int lm_fit_on_device(lsqr_ctx *c, int use_mask, const LmSet &t, SolveOut *out) {
  hipLaunchKernelGGL(k_lm_init, dim3(1), dim3(64), 0, c->stream, c->d_lm, c->d_out, t.n, t.ftol, t.xtol, t.gtol,
                     t.maxfev, 100.0);
  HIPCHK(c, hipGetLastError());
  for (;;) {
    int nmom = 0, st;
    HIPCHK(c, hipMemcpyAsync(c->d_vec, (const char *)c->d_lm.get() + offsetof(LmState, xtrial), sizeof(double) * t.n,
                             hipMemcpyDeviceToDevice, c->stream));
    if ((st = launch_moments<M>(c, use_mask, 0, c->n, 1, &nmom)) != LSQR_OK) return st;
    {
      ProfScope ps(c, KID_SOLVE);
      hipLaunchKernelGGL((k_lm_advance<M>), dim3(1), dim3(64), 0, c->stream, c->d_lm, c->d_mom, c->d_out);
      HIPCHK(c, hipGetLastError());
    }
    if ((st = read_out(c, out)) != LSQR_OK) return st;
    if (!out->cont) return LSQR_OK;
  }
}

// the plane phantom: both fits from the Gram block, on the host
int fit_phantom(lsqr_ctx *c, int use_mask, SolveOut *out) {
  int nmom = 0, st;
  if ((st = launch_moments_phantom(c, use_mask, 0, c->n, &nmom)) != LSQR_OK) return st;
  HIPCHK(c, hipMemcpyAsync(c->h_pin->scratch, c->d_mom, sizeof(double) * nmom, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, sync_stream(c));
  phantom_solve_block(c->cfg, c->h_pin->scratch_f64, out);
  return LSQR_OK;
}

// leastSquaresEstimate over [0,n) (single device).  Leaves the result in d_out.
// have_moments: d_mom already holds the phase-0 block about d_vec (launch_mask_moments)
// have_origin: the caller has put the fit origin into d_vec (set_fit_origin)
int run_fit(lsqr_ctx *c, int use_mask, SolveOut *out, bool have_moments = false, bool have_origin = false) {
  return dispatch(c->cfg, [&](auto tag) -> int {
    typedef typename decltype(tag)::type M;
    if constexpr (requires { M::IS_PHANTOM; }) {
      return fit_phantom(c, use_mask, out);
    } else {
      int st;
      if ((st = enqueue_closed_fit<M>(c, use_mask, have_moments, have_origin)) != LSQR_OK) return st;
      if ((st = read_out(c, out)) != LSQR_OK) return st;
      if constexpr (requires { M::NMOM_LM; }) {  // (every model wants_lm can name today has an LM block)
        if (!wants_lm(c->cfg) || !out->ok) return LSQR_OK;  // algebraic initialiser failed -> empty (Sphere...hxx:231-232)
        LmSet t;
        lm_settings(c->cfg, &t.n, &t.ftol, &t.xtol, &t.gtol, &t.maxfev);
        if (c->opt.lm_host) {
          // MINPACK's control flow between device passes runs on the host (like the RANSAC replay):
          // a few hundred flops per evaluation; every N-scale operation stays a device pass.
          LmState &s = c->h_lm;
          st = c->opt.lm_fused ? lm_fit_fused<M>(c, use_mask, t, out->params, s)
                               : lm_fit_staged<M>(c, use_mask, t, out->params, s);
          if (st != LSQR_OK) return st;
          static const bool dbg_on = getenv("LSQR_LM_DEBUG") != nullptr;
          if (dbg_on)
            fprintf(stderr, "lm: info %d nfev %d outer iterations %d (accepted steps %d) cost %.17g stall %d par %.3g delta %.3g\n",
                    s.info, s.nfev, s.iter, s.iter - 1, s.fnorm * s.fnorm, s.stall, s.par, s.delta);
          lm_fill_result(s, M::lm_finalize(s.x, out->params), out);
          return LSQR_OK;
        }
        return lm_fit_on_device<M>(c, use_mask, t, out);
      } else {
        if (wants_lm(c->cfg) && out->ok) return fail(c, LSQR_ERR_INVALID, "model has no iterative phase");
        return LSQR_OK;
      }
    }
  });
}

int launch_mask(lsqr_ctx *c, size_t begin, size_t end) {
  int st = ensure(c, c->d_mask, c->n);
  if (st != LSQR_OK) return st;
  st = dispatch(c->cfg, [&](auto tag) -> int {
    typedef typename decltype(tag)::type M;
    HIPCHK(c, hipMemsetAsync(c->d_counter + CNT_MASK, 0, sizeof(unsigned long long), c->stream));
    if constexpr (M::SP > M::P && !M::IS_DENSE) {
      hipLaunchKernelGGL((k_prepare<M>), dim3(1), dim3(64), 0, c->stream, c->d_par, c->mc);
      HIPCHK(c, hipGetLastError());
    }
    ProfScope ps(c, KID_MASK);
    if constexpr (M::IS_DENSE) {  // wide rows: LDS-staged, coalesced
      const int n = c->cfg.dim;
      const size_t lds = sizeof(double) * 4 * 32 * ((n + 1) | 1);
      int grid = grid_for(end - begin, 4 * 32 * 4, 256 * 4);
      hipLaunchKernelGGL((k_mask_dense<M::NR>), dim3(grid), dim3(256), lds, c->stream, c->d_data,
                         c->stride, begin, end, n, c->d_par, c->mc.delta, c->d_mask, c->d_counter + CNT_MASK);
      HIPCHK(c, hipGetLastError());
      return LSQR_OK;
    }
    int grid = grid_for(end - begin, kBlock * 8, 256 * 8);
    hipLaunchKernelGGL((k_mask<M>), dim3(grid), dim3(kBlock), 0, c->stream, c->d_data, c->stride,
                       begin, end, c->d_par, c->mc, c->d_mask, c->d_counter + CNT_MASK);
    HIPCHK(c, hipGetLastError());
    return LSQR_OK;
  });
  if (st != LSQR_OK) return st;
  c->mask_valid = true;
  c->origin_valid = true;
  return LSQR_OK;
}

int launch_mask_moments(lsqr_ctx *c, size_t begin, size_t end, int *nmom, bool *fused);
int run_mask(lsqr_ctx *c, size_t begin, size_t end, uint8_t *mask_out, uint64_t *count_out) {
  int st, nm = 0;
  bool fused = false;
  // dense system: the one-pass kernel (mask + block of sums, dense.h: k_mask_syrk_dense) is the faster mask as well
  if (c->cfg.model == LSQR_MODEL_DENSE && (st = launch_mask_moments(c, begin, end, &nm, &fused)) != LSQR_OK) return st;
  if (!fused && (st = launch_mask(c, begin, end)) != LSQR_OK) return st;
  HIPCHK(c, hipMemcpyAsync(c->h_pin->scratch, c->d_counter + CNT_MASK, sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, c->stream));
  if (mask_out)
    HIPCHK(c, hipMemcpyAsync(mask_out, c->d_mask + begin, end - begin, hipMemcpyDeviceToHost,
                             c->stream));
  HIPCHK(c, sync_stream(c));
  if (count_out) *count_out = *c->h_pin->scratch_u64;
  return LSQR_OK;
}

// mask of d_par over [begin, end) and the phase-0 moment block of the agreeing records about d_vec (set by the
// caller) in ONE pass; -> d_mask, d_counter[CNT_MASK], d_mom.  *fused = false (nothing launched) for the models
// whose moments are not a per-record accumulate (dense: SYRK on the matrix cores; phantom: Gram of the rows).
int launch_mask_moments(lsqr_ctx *c, size_t begin, size_t end, int *nmom, bool *fused) {
  *fused = false;
  if (c->cfg.model == LSQR_MODEL_PHANTOM || !c->opt.fuse_mask) return LSQR_OK;
  int st = ensure(c, c->d_mask, c->n);
  if (st != LSQR_OK) return st;
  if (c->cfg.model == LSQR_MODEL_DENSE) {
    // dense system: mask + sum z z^T of the agreeing rows in one pass (dense.h: k_mask_syrk_dense); tight records
    // and the matrix-core path only -- anything else keeps the two kernels
    const int n = c->cfg.dim, nz = n + 1;
    if (c->stride != (size_t)nz || !c->opt.filter || c->opt.syrk_diag || end <= begin ||
        ((uintptr_t)c->d_data & 15) != 0 || ((begin * (size_t)nz) & 1) != 0)  // 16-byte pieces from the first row on
      return LSQR_OK;
    if ((st = ensure_absmax(c)) != LSQR_OK) return st;  // magnitudes for the band of the four-chain evaluation
    HIPCHK(c, hipMemsetAsync(c->d_counter + CNT_MASK, 0, sizeof(unsigned long long), c->stream));
    const int nbuf = (c->opt.mask_ring == 4 && n == 64) ? 4 : 2;
    // two workgroups per CU / one; whole rounds of the four waves' 16-row tiles (end > begin: checked above)
    const PassShape shape = pass_shape(end - begin, 64 * 4, nbuf == 2 ? 512 : 256, 64);
    const int nb = shape.nb;
    const size_t chunk = shape.chunk;
    const int ps = dense_pstride(n), na16 = (n + 15) / 16;
    // ring + model + waiting rows while streaming; the fold area afterwards
    const size_t lds = std::max<size_t>(sizeof(double) * (4 * nbuf * 16 * nz + 64 + 4 * 3 * nz),
                                        sizeof(double) * (10 * 256 + 80));
    if ((size_t)nb * ps > (size_t)2 * kDenseBlocks * 2160) return LSQR_OK;  // (partials area: 512 x 2160 doubles)
    *nmom = dense_ne(n) + 1;
    {
      ProfScope ps_(c, KID_MASK);
      auto launch = [&](auto kern) {
        (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kern, dim3(nb), dim3(256), lds, c->stream, c->d_data, begin, end, chunk, n, c->d_par,
                           c->mc.delta, c->d_mask, c->d_counter + CNT_MASK, ps, c->d_partials, c->mc.absmax_rot, c->mc.absmax,
                           c->opt.mask_band > 0 ? (double)c->opt.mask_band : 1.0, c->opt.mask_diag);
      };
      if (nbuf == 4) {
        launch(k_mask_syrk_dense<4, 4>);   // n = 64: one workgroup per CU, three tiles in flight per wave
      } else {
        switch (na16) {
          case 1: launch(k_mask_syrk_dense<1, 2>); break;
          case 2: launch(k_mask_syrk_dense<2, 2>); break;
          case 3: launch(k_mask_syrk_dense<3, 2>); break;
          default: launch(k_mask_syrk_dense<4, 2>); break;
        }
      }
      HIPCHK(c, hipGetLastError());
    }
    {
      ProfScope ps_(c, KID_SOLVE);
      hipLaunchKernelGGL(k_reduce, dim3(*nmom), dim3(64), 0, c->stream, c->d_partials, nb, ps, *nmom, c->d_mom);
      HIPCHK(c, hipGetLastError());
    }
    c->mask_valid = true;
    c->origin_valid = true;
    *fused = true;
    return LSQR_OK;
  }
  st = dispatch(c->cfg, [&](auto tag) -> int {
    typedef typename decltype(tag)::type M;
    if constexpr (M::IS_DENSE || requires { M::IS_PHANTOM; }) {
      return LSQR_ERR_INVALID;
    } else {
      HIPCHK(c, hipMemsetAsync(c->d_counter + CNT_MASK, 0, sizeof(unsigned long long), c->stream));
      if constexpr (M::SP > M::P) {
        hipLaunchKernelGGL((k_prepare<M>), dim3(1), dim3(64), 0, c->stream, c->d_par, c->mc);
        HIPCHK(c, hipGetLastError());
      }
      const size_t cnt = end - begin;
      const PassShape shape = pass_shape(cnt, mom_chunk(c), kMaxPartials, kBlock);  // as launch_moments
      int nb = shape.nb;
      const size_t chunk = shape.chunk;
      *nmom = M::NMOM;
      bool done = false;
      if constexpr (M::IS_US) {
        // US calibrations with tight records: rows of the agreeing frames to the fp64 matrix cores (kernels.h)
        if (c->opt.us_mask_mfma && c->stride == (size_t)M::REC && cnt > 0) {
          nb = (int)std::min<size_t>(1024, (cnt + 4 * 64 * 2 - 1) / (4 * 64 * 2));  // >= two tiles per wave: one in flight
          if (nb < 1) nb = 1;
          ProfScope ps(c, KID_MASK);
          hipLaunchKernelGGL((k_mask_moments_us_mfma<M>), dim3(nb), dim3(kBlock), 0, c->stream, c->d_data, begin, end,
                             c->d_par, c->mc, c->d_mask, c->d_counter + CNT_MASK, c->d_partials);
          HIPCHK(c, hipGetLastError());
          done = true;
        }
      }
      if (!done) {
        ProfScope ps(c, KID_MASK);
        hipLaunchKernelGGL((k_mask_moments<M>), dim3(nb), dim3(kBlock), 0, c->stream, c->d_data, c->stride,
                           begin, end, chunk, c->d_par, c->d_vec, c->mc, c->d_mask, c->d_counter + CNT_MASK,
                           c->d_partials);
        HIPCHK(c, hipGetLastError());
      }
      ProfScope ps(c, KID_SOLVE);
      hipLaunchKernelGGL(k_reduce, dim3(*nmom), dim3(64), 0, c->stream, c->d_partials, nb, (int)MOM_MAX,
                         *nmom, c->d_mom);
      HIPCHK(c, hipGetLastError());
      return LSQR_OK;
    }
  });
  if (st != LSQR_OK) return st;
  c->mask_valid = true;
  c->origin_valid = true;
  *fused = true;
  return LSQR_OK;
}

// the winner's scan parameters -> d_par, on the device (no host round trip between scan and mask)
__global__ void k_take_best(const unsigned long long *__restrict__ packed,
                            const double *__restrict__ hparams, int hs, double *__restrict__ par) {
  const unsigned long long pk = *packed;
  const int t = threadIdx.x;
  for (int k = hs + t; k < 128; k += blockDim.x) par[k] = 0.0;  // (the block holds 128 doubles)
  if (t >= hs) return;
  if (pk == 0) {
    par[t] = __builtin_nan("");  // no valid hypothesis: nothing agrees
    return;
  }
  const size_t idx = 0xFFFFFFFFull - (pk & 0xFFFFFFFFull);
  par[t] = hparams[idx * (size_t)hs + t];
}

}  // namespace

// =================================================================================================
extern "C" {

const char *lsqr_version(void) {
#ifdef LSQR_DEV_SUBSET
  return "lsqrrecipes_amd 0.2 (gfx950) DEVELOPMENT SUBSET BUILD";
#else
  return "lsqrrecipes_amd 0.2 (gfx950)";
#endif
}

const char *lsqr_status_string(int s) {
  switch (s) {
    case LSQR_OK: return "ok";
    case LSQR_EMPTY: return "empty result (degenerate data or failed fit)";
    case LSQR_ERR_INVALID: return "invalid argument";
    case LSQR_ERR_NO_DEVICE: return "no usable HIP device";
    case LSQR_ERR_HIP: return "HIP runtime error";
    case LSQR_ERR_STATE: return "call order error";
  }
  return "unknown status";
}

int lsqr_device_count(int *count) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (count) *count = (e == hipSuccess) ? n : 0;
  return e == hipSuccess ? LSQR_OK : LSQR_ERR_NO_DEVICE;
}

int lsqr_ctx_create(int device, lsqr_ctx **out) {
  if (!out) return LSQR_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n)
    return LSQR_ERR_NO_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return LSQR_ERR_NO_DEVICE;
  lsqr_ctx *c = new lsqr_ctx();
  c->device = device;
  bool ok = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) == hipSuccess &&
            c->ev0.create() == hipSuccess && c->ev1.create() == hipSuccess &&
            c->d_partials.alloc(kPartialsBytes / sizeof(double)) == hipSuccess &&
            c->d_mom.alloc(4096) == hipSuccess && c->d_vec.alloc(128) == hipSuccess &&
            c->d_par.alloc(128) == hipSuccess && c->d_best.alloc(128) == hipSuccess &&
            c->d_lm.alloc(1) == hipSuccess && c->d_out.alloc(1) == hipSuccess &&
            c->d_counter.alloc(8) == hipSuccess &&  // CNT_* words
            c->d_ambcnt.alloc(2 * kAmbSlots) == hipSuccess &&
            c->h_pin.alloc(1) == hipSuccess && c->h_lmres.alloc(256) == hipSuccess;
  if (ok) {
    memset(c->h_lmres, 0, sizeof(unsigned long long) * 256);
    ok = hipMemsetAsync(c->d_counter, 0, 64, c->own_stream) == hipSuccess &&
         hipMemsetAsync(c->d_ambcnt, 0, 2 * kAmbSlots * sizeof(unsigned long long), c->own_stream) == hipSuccess;
  }
  c->stream = c->own_stream;
  if (!ok) {
    lsqr_ctx_destroy(c);
    return LSQR_ERR_HIP;
  }
  *out = c;
  lmp_ctx_count(device, +1);
  c->counted = true;
  return LSQR_OK;
}

void lsqr_ctx_destroy(lsqr_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  lmp_ctx_count(c->device, c->counted ? -1 : 0, c);
  for (int i = 1; i < lsqr_ctx::kMaxLanes; i++)
    if (c->lanes[i]) {
      lsqr_ctx_destroy(c->lanes[i]);
      c->lanes[i] = nullptr;
    }
  (void)hipStreamSynchronize(c->stream);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;  // every buffer and event is a member: gone with the context
}

const char *lsqr_last_error(const lsqr_ctx *c) { return c ? c->err : "null context"; }

int lsqr_synchronize(lsqr_ctx *c) {
  if (!c) return LSQR_ERR_INVALID;
  HIPCHK(c, sync_stream(c));
  for (int i = 1; i < lsqr_ctx::kMaxLanes; i++)
    if (c->lanes[i]) HIPCHK(c, hipStreamSynchronize(c->lanes[i]->stream));
  return LSQR_OK;
}

// ---- model description ---------------------------------------------------------------------------
// ---- entry points that need no device: host_entry.h -------------------------------------------------------------------
int lsqr_min_subset(const lsqr_model_cfg *cfg) { return host_min_subset(cfg); }
int lsqr_num_params(const lsqr_model_cfg *cfg) { return host_num_params(cfg); }
int lsqr_record_doubles(const lsqr_model_cfg *cfg) { return host_record_doubles(cfg); }
int lsqr_sample_subsets(uint64_t seed, uint64_t first, size_t H, uint64_t n, int k, uint32_t *out) {
  return host_sample_subsets(seed, first, H, n, k, out);
}
void *lsqr_dedup_create(int k) { return host_dedup_create(k); }
void lsqr_dedup_destroy(void *s) { host_dedup_destroy(s); }
int lsqr_replay_init(size_t n, int k, double p, uint64_t st[6]) { return host_replay_init(n, k, p, st); }
size_t lsqr_replay(size_t n, int k, double p, const uint32_t *subsets, const uint8_t *valid, const uint32_t *votes,
                   size_t H, uint64_t base_index, void *dedup, uint64_t st[6]) {
  return host_replay(n, k, p, subsets, valid, votes, H, base_index, dedup, st);
}
int lsqr_agree_host(const lsqr_model_cfg *cfg, const double *params, const void *record, int *agree_out) {
  return host_agree_host(cfg, params, record, agree_out);
}
int lsqr_estimate_host(const lsqr_model_cfg *cfg, const void *records, size_t count, size_t stride_bytes,
                       double *params_out, int *n_params_out) {
  return host_estimate_host(cfg, records, count, stride_bytes, params_out, n_params_out);
}
int lsqr_assign_host(const lsqr_model_cfg *cfg, const double *params, size_t n_models, const void *record,
                     int32_t *label_out, double *residual_out) {
  return host_assign_host<ASSIGN_HOST_POINT>(cfg, params, n_models, record, label_out, residual_out);
}
int lsqr_assign_dense_host(const lsqr_model_cfg *cfg, const double *params, size_t n_models, const void *record,
                           int32_t *label_out, double *residual_out) {
  return host_assign_host<ASSIGN_HOST_DENSE>(cfg, params, n_models, record, label_out, residual_out);
}
int lsqr_assign_rigid_host(const lsqr_model_cfg *cfg, const double *params, size_t n_models, const void *record,
                           int32_t *label_out, double *residual_out) {
  return host_assign_host<ASSIGN_HOST_RIGID>(cfg, params, n_models, record, label_out, residual_out);
}

int lsqr_set_model(lsqr_ctx *c, const lsqr_model_cfg *cfg) {
  if (!c || !cfg) return LSQR_ERR_INVALID;
  if (!cfg_supported(*cfg))
    return fail(c, LSQR_ERR_INVALID, "unsupported model %d / dim %d", cfg->model, cfg->dim);
  if (cfg->model == LSQR_MODEL_SPHERE && cfg->ls_type != LSQR_LS_ALGEBRAIC &&
      cfg->ls_type != LSQR_LS_GEOMETRIC)  // SphereParametersEstimator.hxx:17-18 throws
    return fail(c, LSQR_ERR_INVALID, "invalid sphere least squares type %d", cfg->ls_type);
  lanes_quiesce(c);
  c->data_epoch++;
  // The same estimator type with another threshold / fit type (RANSAC<T,S>::compute() again on resident records,
  // lsqrRecipes::ResidentData): what was derived from the records alone -- their bounds and magnitudes, the spatial
  // index -- stays valid.
  const bool same_shape = c->has_model && c->cfg.model == cfg->model && c->cfg.dim == cfg->dim;
  const double absmax_keep = c->mc.absmax, absrot_keep = c->mc.absmax_rot;
  c->cfg = *cfg;
  model_consts(*cfg, &c->mc);
  c->K = lsqr_min_subset(cfg);
  c->P = lsqr_num_params(cfg);
  c->ND = lsqr_record_doubles(cfg);
  c->HS = dispatch(*cfg, [](auto tag) { return (int)decltype(tag)::type::SP; });
  c->has_model = true;
  if (c->n && c->stride < (size_t)c->ND) c->n = 0;  // the resident records cannot be read as this model's
  if (same_shape && c->n) {
    c->mc.absmax = absmax_keep;
    c->mc.absmax_rot = absrot_keep;
  } else {
    drop_index(c);
    c->absmax_valid = false;
    c->bounds_valid = false;
  }
  c->rows_valid = false;
  c->H = 0;
  c->scanned = false;
  c->mask_valid = false;
  c->origin_valid = false;
  c->merge_off = false;   // selection feedback belongs to one model (threshold included) on one upload
  bsel_reset(c);
  return LSQR_OK;
}

// ---- observations ----------------------------------------------------------------------------------
static int set_data_common(lsqr_ctx *c, size_t count, size_t stride_bytes) {
  if (stride_bytes % sizeof(double) != 0 || stride_bytes / sizeof(double) < (size_t)c->ND)
    return fail(c, LSQR_ERR_INVALID, "record stride %zu B does not hold %d doubles", stride_bytes,
                c->ND);
  if (count > 0xFFFFFFF0ull) return fail(c, LSQR_ERR_INVALID, "too many observations");
  lanes_quiesce(c);  // lanes read the records this call is about to replace
  c->data_epoch++;
  c->merge_off = false;
  bsel_reset(c);
  c->n = count;
  c->absmax_valid = false;
  c->bounds_valid = false;
  c->rows_valid = false;
  drop_index(c);
  c->index_failed = false;
  c->hyp_since_upload = 0;
  c->hyp_expected = 0;
  c->stride = stride_bytes / sizeof(double);
  c->H = 0;
  c->scanned = false;
  c->mask_valid = false;
  c->origin_valid = false;
  return LSQR_OK;
}

// Host -> device copy of a large pageable buffer.  A plain hipMemcpy stages pageable memory through the
// runtime's own bounce buffers with one host thread (measured ~5 GB/s: 50 ms for the 240 MB of 10 M points);
// here a few threads copy 8 MiB chunks into a ring of pinned slots and enqueue each slot's DMA as soon as it is
// filled, so the host copies and the PCIe transfers overlap.
static int staged_upload(lsqr_ctx *c, void *dst, const void *src, size_t bytes, int threads) {
  for (int i = 0; i < lsqr_ctx::kUpSlots; i++) {
    if (!c->h_up[i]) HIPCHK(c, c->h_up[i].alloc(lsqr_ctx::kUpChunk));
    if (!c->up_ev[i]) HIPCHK(c, c->up_ev[i].create(hipEventDisableTiming));
  }
  const size_t chunk = lsqr_ctx::kUpChunk, nchunks = (bytes + chunk - 1) / chunk;
  std::atomic<size_t> next{0};
  std::atomic<int> err{(int)hipSuccess};
  // chunk i uses slot i % kUpSlots; it may be overwritten once chunk i - kUpSlots has left it (its event)
  std::vector<std::atomic<int>> issued(nchunks);
  for (auto &f : issued) f.store(0);
  auto work = [&]() {
    if (hipSetDevice(c->device) != hipSuccess) {
      err.store((int)hipErrorInvalidDevice);
      return;
    }
    for (;;) {
      const size_t i = next.fetch_add(1);
      if (i >= nchunks || err.load() != (int)hipSuccess) return;
      const int slot = (int)(i % lsqr_ctx::kUpSlots);
      if (i >= (size_t)lsqr_ctx::kUpSlots) {
        const size_t prev = i - lsqr_ctx::kUpSlots;
        while (!issued[prev].load(std::memory_order_acquire)) std::this_thread::yield();
        hipError_t e = hipEventSynchronize(c->up_ev[slot]);
        if (e != hipSuccess) {
          err.store((int)e);
          issued[i].store(1, std::memory_order_release);
          return;
        }
      }
      const size_t off = i * chunk, len = std::min(chunk, bytes - off);
      memcpy(c->h_up[slot].get(), (const char *)src + off, len);
      hipError_t e = hipMemcpyAsync((char *)dst + off, c->h_up[slot], len, hipMemcpyHostToDevice, c->stream);
      if (e == hipSuccess) e = hipEventRecord(c->up_ev[slot], c->stream);
      if (e != hipSuccess) err.store((int)e);
      issued[i].store(1, std::memory_order_release);
    }
  };
  std::vector<std::thread> pool;
  const int nt = (int)std::min<size_t>((size_t)threads, nchunks);
  for (int t = 1; t < nt; t++) pool.emplace_back(work);
  work();
  for (auto &t : pool) t.join();
  if (err.load() != (int)hipSuccess)
    return fail(c, LSQR_ERR_HIP, "staged upload failed: %s", hipGetErrorString((hipError_t)err.load()));
  return LSQR_OK;
}

int lsqr_upload(lsqr_ctx *c, const void *host, size_t count, size_t stride_bytes) {
  int st = need_ready(c, false);
  if (st != LSQR_OK) return st;
  if (!host && count) return fail(c, LSQR_ERR_INVALID, "null records");
  if ((st = set_data_common(c, count, stride_bytes)) != LSQR_OK) return st;
  size_t doubles = std::max<size_t>(count * c->stride, 1);
  if ((st = ensure(c, c->d_data_owned, doubles)) != LSQR_OK) return st;
  const size_t bytes = count * stride_bytes;
  // measured on the MI355X box (bench.py cold_call, 240 MB from a pageable numpy buffer): one plain
  // hipMemcpy 4.3 ms = 56 GB/s, the staged ring with 4 threads 5.1 ms -- so the plain copy is the default and
  // the staged path stays an option for hosts whose runtime stages pageable memory slowly
  int threads = c->opt.upload_threads;
  if (threads < 0) {
    const char *e = getenv("LSQR_UPLOAD_THREADS");
    threads = e ? atoi(e) : 0;
  }
  threads = std::max(0, std::min(threads, 16));
  const auto t0 = std::chrono::steady_clock::now();
  if (bytes >= ((size_t)32 << 20) && threads > 0) {
    if ((st = staged_upload(c, c->d_data_owned, host, bytes, threads)) != LSQR_OK) return st;
  } else if (count) {
    HIPCHK(c, hipMemcpyAsync(c->d_data_owned, host, bytes, hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, sync_stream(c));
  c->last_upload_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  c->d_data = c->d_data_owned;
  return LSQR_OK;
}

int lsqr_attach(lsqr_ctx *c, const void *dev, size_t count, size_t stride_bytes) {
  int st = need_ready(c, false);
  if (st != LSQR_OK) return st;
  if (!dev && count) return fail(c, LSQR_ERR_INVALID, "null records");
  if ((st = set_data_common(c, count, stride_bytes)) != LSQR_OK) return st;
  c->d_data = (const double *)dev;
  return LSQR_OK;
}

size_t lsqr_count(const lsqr_ctx *c) { return c ? c->n : 0; }

// ---- hypotheses ------------------------------------------------------------------------------------
int lsqr_hypotheses_from_subsets(lsqr_ctx *c, const uint32_t *subsets, size_t H) {
  int st = need_ready(c, true);
  if (st != LSQR_OK) return st;
  if (!subsets || H == 0 || H > (1u << 20)) return fail(c, LSQR_ERR_INVALID, "bad subset batch");
  if (c->n < (size_t)c->K) return fail(c, LSQR_ERR_INVALID, "fewer observations than a subset");
  if ((st = ensure_hyp(c, H)) != LSQR_OK) return st;
  c->H = H;
  c->scanned = false;
  HIPCHK(c, hipMemcpyAsync(c->d_subsets, subsets, H * c->K * sizeof(uint32_t),
                           hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, sync_stream(c));  // caller may free `subsets` on return
  return run_estimate(c);
}

int lsqr_hypotheses_sample(lsqr_ctx *c, uint64_t seed, uint64_t first, size_t H,
                           uint32_t *subsets_out) {
  int st = need_ready(c, true);
  if (st != LSQR_OK) return st;
  if (H == 0 || H > (1u << 20)) return fail(c, LSQR_ERR_INVALID, "bad batch size");
  if (c->n < (size_t)c->K) return fail(c, LSQR_ERR_INVALID, "fewer observations than a subset");
  if ((st = ensure_hyp(c, H)) != LSQR_OK) return st;
  c->H = H;
  c->scanned = false;
  {
    ProfScope ps(c, KID_SAMPLE);
    int grid = (int)((H + kBlock - 1) / kBlock);
    if (c->K <= 4)
      hipLaunchKernelGGL((k_sample<4>), dim3(grid), dim3(kBlock), 0, c->stream, seed, first,
                         (uint32_t)H, (uint64_t)c->n, c->K, c->d_subsets);
    else  // large subsets: one wave per hypothesis
      hipLaunchKernelGGL(k_sample_wave, dim3((unsigned)H), dim3(64), 0, c->stream, seed, first,
                         (uint32_t)H, (uint64_t)c->n, c->K, c->d_subsets);
    HIPCHK(c, hipGetLastError());
  }
  if ((st = run_estimate(c)) != LSQR_OK) return st;
  if (subsets_out) {
    HIPCHK(c, hipMemcpyAsync(subsets_out, c->d_subsets, H * c->K * sizeof(uint32_t),
                             hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, sync_stream(c));
  }
  return LSQR_OK;
}

int lsqr_scan(lsqr_ctx *c) {
  int st = need_ready(c, true);
  if (st != LSQR_OK) return st;
  if (c->H == 0) return fail(c, LSQR_ERR_STATE, "no hypotheses to scan");
  if ((st = run_scan(c)) != LSQR_OK) return st;
  c->scanned = true;
  return LSQR_OK;
}

size_t lsqr_num_hypotheses(const lsqr_ctx *c) { return c ? c->H : 0; }

int lsqr_get_hypotheses(lsqr_ctx *c, double *params, uint8_t *valid, uint32_t *votes) {
  int st = need_ready(c, true);
  if (st != LSQR_OK) return st;
  if (c->H == 0) return fail(c, LSQR_ERR_STATE, "no hypotheses");
  if (votes && !c->scanned) return fail(c, LSQR_ERR_STATE, "lsqr_scan has not run");
  if (params)
    HIPCHK(c, hipMemcpy2DAsync(params, c->P * sizeof(double), c->d_hparams,
                               c->HS * sizeof(double), c->P * sizeof(double), c->H,
                               hipMemcpyDeviceToHost, c->stream));
  if (valid)
    HIPCHK(c, hipMemcpyAsync(valid, c->d_valid, c->H, hipMemcpyDeviceToHost, c->stream));
  if (votes)
    HIPCHK(c, hipMemcpyAsync(votes, c->d_votes, c->H * sizeof(uint32_t), hipMemcpyDeviceToHost,
                             c->stream));
  HIPCHK(c, sync_stream(c));
  return LSQR_OK;
}

int lsqr_get_hypothesis(lsqr_ctx *c, size_t h, double *params, uint8_t *valid) {
  int st = need_ready(c, true);
  if (st != LSQR_OK) return st;
  if (h >= c->H) return fail(c, LSQR_ERR_INVALID, "hypothesis index out of range");
  double *hp = c->h_pin->scratch_f64;
  HIPCHK(c, hipMemcpyAsync(hp, c->d_hparams + h * c->HS, sizeof(double) * c->P,
                           hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(hp + 64, c->d_valid + h, 1, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, sync_stream(c));
  if (params) memcpy(params, hp, sizeof(double) * c->P);
  if (valid) *valid = *(uint8_t *)(hp + 64);
  return LSQR_OK;
}

int lsqr_best(lsqr_ctx *c, uint64_t *packed) {
  int st = need_ready(c, true);
  if (st != LSQR_OK) return st;
  if (!packed || !c->scanned) return fail(c, LSQR_ERR_STATE, "lsqr_scan has not run");
  hipLaunchKernelGGL(k_best, dim3(1), dim3(kBlock), 0, c->stream, c->d_votes, c->d_valid,
                     (uint32_t)c->H, c->d_counter + CNT_BEST);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(c->h_pin->scratch, c->d_counter + CNT_BEST, sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, sync_stream(c));
  *packed = *c->h_pin->scratch_u64;
  return LSQR_OK;
}

// ---- mask ----------------------------------------------------------------------------------------
int lsqr_mask(lsqr_ctx *c, const double *params, size_t begin, size_t end, uint8_t *mask_out,
              uint64_t *count_out) {
  int st = need_ready(c, true);
  if (st != LSQR_OK) return st;
  if (!params || begin > end || end > c->n) return fail(c, LSQR_ERR_INVALID, "bad mask range");
  HIPCHK(c, hipMemsetAsync(c->d_par, 0, sizeof(double) * 128, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_par, params, sizeof(double) * c->P, hipMemcpyHostToDevice,
                           c->stream));
  HIPCHK(c, sync_stream(c));
  return run_mask(c, begin, end, mask_out, count_out);
}

int lsqr_mask_from_hypothesis(lsqr_ctx *c, size_t h, uint8_t *mask_out, uint64_t *count_out) {
  int st = need_ready(c, true);
  if (st != LSQR_OK) return st;
  if (h >= c->H) return fail(c, LSQR_ERR_INVALID, "hypothesis index out of range");
  HIPCHK(c, hipMemcpyAsync(c->d_par, c->d_hparams + h * c->HS, sizeof(double) * c->HS,
                           hipMemcpyDeviceToDevice, c->stream));
  return run_mask(c, 0, c->n, mask_out, count_out);
}

int lsqr_set_mask(lsqr_ctx *c, const uint8_t *mask) {
  int st = need_ready(c, true);
  if (st != LSQR_OK) return st;
  if (!mask) return fail(c, LSQR_ERR_INVALID, "null mask");
  if ((st = ensure(c, c->d_mask, c->n)) != LSQR_OK) return st;
  HIPCHK(c, hipMemcpyAsync(c->d_mask, mask, c->n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, sync_stream(c));
  c->mask_valid = true;
  c->origin_valid = false;
  return LSQR_OK;
}

// ---- the result tail of the fit entry points -----------------------------------------------------------------------
static void fill_info(const SolveOut &out, lsqr_fit_info *info) {
  if (!info) return;
  memset(info, 0, sizeof *info);
  info->n_params = out.n_params;
  info->lm_info = out.lm_info;
  info->lm_nfev = out.lm_nfev;
  info->reserved = out.pad;  // LM: stall evaluation; dense: 1 = the double-double route produced the result
  info->cost = out.cost;
}

// the parameters of a fit that has a result, LSQR_EMPTY otherwise
static int deliver_params(const SolveOut &out, double *params_out) {
  if (!out.ok) return LSQR_EMPTY;
  if (params_out)
    for (int j = 0; j < out.n_params; j++) params_out[j] = out.params[j];
  return LSQR_OK;
}

static int deliver_fit(const SolveOut &out, double *params_out, lsqr_fit_info *info) {
  fill_info(out, info);
  return deliver_params(out, params_out);
}

// the fit record of a RANSAC result (n_params is 0 without a result); lm_fields = false: lm_info, lm_nfev, reserved stay
static void fill_ransac_fit(const SolveOut &out, uint64_t n_used, bool lm_fields, lsqr_fit_info *fit) {
  fit->n_params = out.ok ? out.n_params : 0;
  if (lm_fields) {
    fit->lm_info = out.lm_info;
    fit->lm_nfev = out.lm_nfev;
    fit->reserved = out.pad;
  }
  fit->n_used = n_used;
  fit->cost = out.cost;
}

// lsqr_ransac_info of one batch (pk: k_best's packed winner, first: the batch's stream index, cnt: the mask's inliers)
static void fill_ransac_info(lsqr_ransac_info *info, unsigned long long pk, uint64_t first, uint64_t H, uint64_t cnt,
                             size_t n, const SolveOut &out, bool lm_fields = true) {
  if (!info) return;
  memset(info, 0, sizeof *info);
  info->fraction = n ? (double)cnt / (double)n : 0.0;
  info->iterations = H;
  info->evaluated = H;
  info->best_votes = (uint32_t)(pk >> 32);
  info->best_index = pk ? first + (0xFFFFFFFFull - (pk & 0xFFFFFFFFull)) : 0;
  fill_ransac_fit(out, cnt, lm_fields, &info->fit);
  info->n_params = info->fit.n_params;
}

// ---- final fit -------------------------------------------------------------------------------------
int lsqr_ls_fit(lsqr_ctx *c, int use_mask, double *params_out, lsqr_fit_info *info) {
  int st = need_ready(c, true);
  if (st != LSQR_OK) return st;
  if (use_mask && !c->mask_valid) return fail(c, LSQR_ERR_STATE, "no mask on the device");
  if (!use_mask) c->origin_valid = false;
  SolveOut out;
  memset(&out, 0, sizeof out);
  if ((st = run_fit(c, use_mask, &out)) != LSQR_OK) return st;
  fill_info(out, info);
  // a Levenberg-Marquardt run that MINPACK reports as failed (the reference then returns an empty vector):
  // the last iterate is still handed out for diagnostics -- status LSQR_EMPTY and info->n_params == 0 say
  // that it is not a result
  if (!out.ok && params_out && out.lm_info != 0)
    for (int j = 0; j < c->P; j++) params_out[j] = out.params[j];
  return deliver_params(out, params_out);
}

int lsqr_moments_len(const lsqr_model_cfg *cfg, int phase) {
  if (!cfg) return 0;
  return dispatch(*cfg, [&](auto tag) -> int {
    typedef typename decltype(tag)::type M;
    if constexpr (requires { M::IS_PHANTOM; }) {
      return phase == 0 || phase == 1 ? dense_ne(30) + 1 : 0;  // phase 1: the same block (lsqr_hip.h)
    } else if constexpr (M::IS_DENSE) {
      return phase == 0 ? dense_ne(cfg->dim) + 1 : 0;
    } else {
      if (phase == 0) return (int)M::NMOM;
      if constexpr (requires { M::NMOM_LM; }) return (int)M::NMOM_LM;
      return 0;
    }
  });
}

// lsqr_moments and lsqr_moments_dev: the checks, x -> d_vec, the block of [begin, end) -> d_mom (*nmom doubles).
// staged: x goes through pinned memory (the copy stays asynchronous) -- four slots in rotation, each guarded by an
// event, so that a call issued before an earlier call's copy has executed cannot overwrite that copy's source
static int enqueue_moments(lsqr_ctx *c, int use_mask, size_t begin, size_t end, int phase, const double *x,
                           const double *block, bool staged, int *nmom) {
  int st = need_ready(c, true);
  if (st != LSQR_OK) return st;
  if (begin > end || end > c->n || !block) return fail(c, LSQR_ERR_INVALID, "bad range");
  if (use_mask && !c->mask_valid) return fail(c, LSQR_ERR_STATE, "no mask on the device");
  if (!x) return fail(c, LSQR_ERR_INVALID, "moments need an origin / evaluation point");
  const int slot = staged ? c->mdev_next++ & 3 : 0;
  if (staged) {
    if (!c->mdev_ev[slot]) HIPCHK(c, c->mdev_ev[slot].create(hipEventDisableTiming));
    else HIPCHK(c, hipEventSynchronize(c->mdev_ev[slot]));
    memcpy(c->h_pin->mdev_x[slot], x, sizeof(double) * 32);
    x = c->h_pin->mdev_x[slot];
  }
  HIPCHK(c, hipMemcpyAsync(c->d_vec, x, sizeof(double) * 32, hipMemcpyHostToDevice, c->stream));
  if (staged) HIPCHK(c, hipEventRecord(c->mdev_ev[slot], c->stream));
  return dispatch(c->cfg, [&](auto tag) -> int {
    typedef typename decltype(tag)::type M;
    return launch_moments<M>(c, use_mask, begin, end, phase, nmom);
  });
}

int lsqr_moments(lsqr_ctx *c, int use_mask, size_t begin, size_t end, int phase, const double *x,
                 double *block_out) {
  int nmom = 0, st = enqueue_moments(c, use_mask, begin, end, phase, x, block_out, false, &nmom);
  if (st != LSQR_OK) return st;
  HIPCHK(c, hipMemcpyAsync(block_out, c->d_mom, sizeof(double) * nmom, hipMemcpyDeviceToHost,
                           c->stream));
  HIPCHK(c, sync_stream(c));
  return LSQR_OK;
}

// lsqr_moments with the block left in DEVICE memory (no synchronisation): the multi-GPU LM loop all-reduces
// it in place and reads it back once
int lsqr_moments_dev(lsqr_ctx *c, int use_mask, size_t begin, size_t end, int phase, const double *x,
                     double *block_dev) {
  int nmom = 0, st = enqueue_moments(c, use_mask, begin, end, phase, x, block_dev, true, &nmom);
  if (st != LSQR_OK) return st;
  HIPCHK(c, hipMemcpyAsync(block_dev, c->d_mom, sizeof(double) * nmom, hipMemcpyDeviceToDevice, c->stream));
  return LSQR_OK;
}

int lsqr_solve_moments(lsqr_ctx *c, const double *block, const double *origin, double *params_out,
                       lsqr_fit_info *info) {
  int st = need_ready(c, false);
  if (st != LSQR_OK) return st;
  if (!block || !origin) return fail(c, LSQR_ERR_INVALID, "null argument");
  int nmom = lsqr_moments_len(&c->cfg, 0);
  if (c->cfg.model == LSQR_MODEL_PHANTOM) {  // solved on the host from the Gram block
    SolveOut out;
    phantom_solve_block(c->cfg, block, &out);
    return deliver_fit(out, params_out, info);
  }
  HIPCHK(c, hipMemcpyAsync(c->d_mom, block, sizeof(double) * nmom, hipMemcpyHostToDevice,
                           c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_vec, origin, sizeof(double) * std::min(c->ND, 32),
                           hipMemcpyHostToDevice, c->stream));
  st = dispatch(c->cfg, [&](auto tag) -> int {
    typedef typename decltype(tag)::type M;
    return launch_solve<M>(c);
  });
  if (st != LSQR_OK) return st;
  SolveOut out;
  if ((st = read_out(c, &out)) != LSQR_OK) return st;
  return deliver_fit(out, params_out, info);
}

int lsqr_lm_begin(lsqr_ctx *c, const double *x0, double *x_trial_out) {
  int st = need_ready(c, false);
  if (st != LSQR_OK) return st;
  if (!wants_lm(c->cfg)) return fail(c, LSQR_ERR_INVALID, "model/ls_type has no iterative fit");
  if (!x0) return fail(c, LSQR_ERR_INVALID, "null x0");
  int n, maxfev;
  double ftol, xtol, gtol;
  lm_settings(c->cfg, &n, &ftol, &xtol, &gtol, &maxfev);
  if (c->opt.lm_host || c->cfg.model == LSQR_MODEL_PHANTOM) {
    lm_init(c->h_lm, n, x0, ftol, xtol, gtol, maxfev, 100.0);
    if (x_trial_out)
      for (int j = 0; j < n; j++) x_trial_out[j] = x0[j];
    return LSQR_OK;
  }
  SolveOut seed;
  memset(&seed, 0, sizeof seed);
  for (int j = 0; j < n; j++) seed.params[j] = x0[j];
  memcpy(c->h_pin->scratch, &seed, sizeof seed);
  HIPCHK(c, hipMemcpyAsync(c->d_out, c->h_pin->scratch, sizeof seed, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_lm_init, dim3(1), dim3(64), 0, c->stream, c->d_lm, c->d_out, n, ftol, xtol,
                     gtol, maxfev, 100.0);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, sync_stream(c));
  if (x_trial_out)
    for (int j = 0; j < n; j++) x_trial_out[j] = x0[j];
  return LSQR_OK;
}

int lsqr_lm_step(lsqr_ctx *c, const double *block, double *x_trial_out, int *cont,
                 double *params_out, lsqr_fit_info *info) {
  int st = need_ready(c, false);
  if (st != LSQR_OK) return st;
  if (!block || !cont) return fail(c, LSQR_ERR_INVALID, "null argument");
  int nmom = lsqr_moments_len(&c->cfg, 1);
  if (nmom <= 0) return fail(c, LSQR_ERR_INVALID, "model has no iterative phase");
  if (c->cfg.model == LSQR_MODEL_PHANTOM) {  // the whole minimisation on the (summed) Gram block
    double G[31 * 31];
    SolveOut out;
    PhantomFit f;
    phantom_unpack(block, G);
    phantom_lm(G, c->h_lm, &f);
    phantom_to_out(f, &out);
    *cont = 0;
    return deliver_fit(out, params_out, info);
  }
  if (c->opt.lm_host) {
    LmState &s = c->h_lm;
    bool go = lm_advance(s, block);
    *cont = go ? 1 : 0;
    SolveOut out;  // the record run_fit's host-stepped drivers leave
    memset(&out, 0, sizeof out);
    if (go) {
      lm_fill_result(s, 0, &out);
      if (x_trial_out)
        for (int j = 0; j < s.n; j++) x_trial_out[j] = s.xtrial[j];
      fill_info(out, info);
      return LSQR_OK;
    }
    const int np = dispatch(c->cfg, [&](auto tag) -> int {
      typedef typename decltype(tag)::type M;
      if constexpr (requires { M::NMOM_LM; }) return M::lm_finalize(s.x, out.params);
      else return 0;
    });
    lm_fill_result(s, np, &out);
    return deliver_fit(out, params_out, info);
  }
  HIPCHK(c, hipMemcpyAsync(c->d_mom, block, sizeof(double) * nmom, hipMemcpyHostToDevice,
                           c->stream));
  st = dispatch(c->cfg, [&](auto tag) -> int {
    typedef typename decltype(tag)::type M;
    if constexpr (requires { M::NMOM_LM; }) {
      ProfScope ps(c, KID_SOLVE);
      hipLaunchKernelGGL((k_lm_advance<M>), dim3(1), dim3(64), 0, c->stream, c->d_lm, c->d_mom,
                         c->d_out);
      HIPCHK(c, hipGetLastError());
      return LSQR_OK;
    } else {
      return LSQR_ERR_INVALID;
    }
  });
  if (st != LSQR_OK) return st;
  SolveOut out;
  if ((st = read_out(c, &out)) != LSQR_OK) return st;
  *cont = out.cont;
  fill_info(out, info);
  if (out.cont) {
    if (x_trial_out) {
      HIPCHK(c, hipMemcpyAsync(c->h_pin->scratch, (const char *)c->d_lm.get() + offsetof(LmState, xtrial),
                               sizeof(double) * LM_NMAX, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, sync_stream(c));
      memcpy(x_trial_out, c->h_pin->scratch, sizeof(double) * c->P);
    }
    return LSQR_OK;
  }
  return deliver_params(out, params_out);
}

int lsqr_stats(lsqr_ctx *c, const double *params, int use_mask, double out[4]) {
  int st = need_ready(c, true);
  if (st != LSQR_OK) return st;
  if (!params || !out) return fail(c, LSQR_ERR_INVALID, "null argument");
  if (use_mask && !c->mask_valid) return fail(c, LSQR_ERR_STATE, "no mask on the device");
  HIPCHK(c, hipMemsetAsync(c->d_par, 0, sizeof(double) * 128, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_par, params, sizeof(double) * c->P, hipMemcpyHostToDevice,
                           c->stream));
  const PassShape shape = pass_shape(c->n, mom_chunk(c), kMaxPartials, kBlock);  // (c->n > 0: need_ready(c, true))
  const int nb = shape.nb;
  const size_t chunk = shape.chunk;
  st = dispatch(c->cfg, [&](auto tag) -> int {
    typedef typename decltype(tag)::type M;
    if (use_mask)
      hipLaunchKernelGGL((k_stats<M, true>), dim3(nb), dim3(kBlock), 0, c->stream, c->d_data,
                         c->stride, c->n, chunk, c->d_mask, c->d_par, c->mc, c->d_partials);
    else
      hipLaunchKernelGGL((k_stats<M, false>), dim3(nb), dim3(kBlock), 0, c->stream, c->d_data,
                         c->stride, c->n, chunk, c->d_mask, c->d_par, c->mc, c->d_partials);
    HIPCHK(c, hipGetLastError());
    return LSQR_OK;
  });
  if (st != LSQR_OK) return st;
  std::vector<double> part((size_t)nb * 8);
  HIPCHK(c, hipMemcpyAsync(part.data(), c->d_partials, part.size() * sizeof(double),
                           hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, sync_stream(c));
  double mn = INFINITY, mx = -INFINITY, sum = 0, sq = 0, cnt = 0;
  for (int b = 0; b < nb; b++) {  // fixed order
    mn = std::min(mn, part[b * 8 + 0]);
    mx = std::max(mx, part[b * 8 + 1]);
    sum += part[b * 8 + 2];
    sq += part[b * 8 + 3];
    cnt += part[b * 8 + 4];
  }
  if (cnt == 0) return LSQR_EMPTY;
  out[0] = mn;
  out[1] = mx;
  out[2] = sum / cnt;
  out[3] = sq;
  return LSQR_OK;
}

int lsqr_residuals(lsqr_ctx *c, const double *params, size_t begin, size_t end, double *out) {
  int st = need_ready(c, true);
  if (st != LSQR_OK) return st;
  if (!params || !out || begin > end || end > c->n) return fail(c, LSQR_ERR_INVALID, "bad argument");
  if (begin == end) return LSQR_OK;
  // staged through d_rows (the phantom's row matrix is rebuilt on the next fit)
  c->rows_valid = false;
  if ((st = ensure(c, c->d_rows, end - begin)) != LSQR_OK) return st;
  HIPCHK(c, hipMemsetAsync(c->d_par, 0, sizeof(double) * 128, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_par, params, sizeof(double) * c->P, hipMemcpyHostToDevice, c->stream));
  st = dispatch(c->cfg, [&](auto tag) -> int {
    typedef typename decltype(tag)::type M;
    int grid = grid_for(end - begin, kBlock, 256 * 8);
    hipLaunchKernelGGL((k_residuals<M>), dim3(grid), dim3(kBlock), 0, c->stream, c->d_data, c->stride,
                       begin, end, c->d_par, c->mc, c->d_rows);
    HIPCHK(c, hipGetLastError());
    return LSQR_OK;
  });
  if (st != LSQR_OK) return st;
  HIPCHK(c, hipMemcpyAsync(out, c->d_rows, sizeof(double) * (end - begin), hipMemcpyDeviceToHost,
                           c->stream));
  HIPCHK(c, sync_stream(c));
  return LSQR_OK;
}

// ---- the finish of a winner ------------------------------------------------------------------------------------
// first-max winner of the scanned batch -> d_counter[CNT_BEST], its scan row -> d_par
static int enqueue_take_best(lsqr_ctx *c) {
  hipLaunchKernelGGL(k_best, dim3(1), dim3(kBlock), 0, c->stream, c->d_votes, c->d_valid,
                     (uint32_t)c->H, c->d_counter + CNT_BEST, 0u);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_take_best, dim3(1), dim3(64), 0, c->stream, c->d_counter + CNT_BEST, c->d_hparams,
                     c->HS, c->d_par);
  HIPCHK(c, hipGetLastError());
  return LSQR_OK;
}

// The winner's scan row is in d_par: its fit origin -> d_vec, its consensus mask over all records with the fit's moment
// block in the same pass where the model has one (*fused), the inlier count -> pin_head[0]; ORG_WINNER_DEV (the winner
// is known on the device only): its packed value -> pin_head[1] as well.
static int enqueue_winner_finish(lsqr_ctx *c, FitOrigin how, unsigned long long *pin_head, bool *fused) {
  int st, nm = 0;
  *fused = false;
  if ((st = set_fit_origin(c, how)) != LSQR_OK) return st;
  if ((st = launch_mask_moments(c, 0, c->n, &nm, fused)) != LSQR_OK) return st;
  if (!*fused && (st = launch_mask(c, 0, c->n)) != LSQR_OK) return st;
  static_assert(CNT_BEST == CNT_MASK + 1, "{inliers, packed winner} is one copy");
  HIPCHK(c, hipMemcpyAsync(pin_head, c->d_counter + CNT_MASK, (how == ORG_WINNER_DEV ? 2 : 1) * sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, c->stream));
  return LSQR_OK;
}

// the blocking finish: the head -> h_pin->mask_head, the consensus mask to the caller, the fit (which synchronises)
static int run_winner_finish(lsqr_ctx *c, FitOrigin how, uint8_t *consensus_out, SolveOut *out) {
  int st;
  bool fused = false;
  if ((st = enqueue_winner_finish(c, how, c->h_pin->mask_head, &fused)) != LSQR_OK) return st;
  if (consensus_out)
    HIPCHK(c, hipMemcpyAsync(consensus_out, c->d_mask, c->n, hipMemcpyDeviceToHost, c->stream));
  memset(out, 0, sizeof *out);
  return run_fit(c, 1, out, fused, true);
}

// The winner's scan row is in d_hparams[0]: its mask over the slice [begin, end) and the slice's phase-0 moment block
// about the model's own point -> d_mask, d_counter[CNT_MASK], d_mom (*nmom doubles).
static int enqueue_winner_slice(lsqr_ctx *c, size_t begin, size_t end, int *nmom) {
  int st;
  HIPCHK(c, hipMemsetAsync(c->d_par, 0, sizeof(double) * 128, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_par, c->d_hparams, sizeof(double) * c->HS, hipMemcpyDeviceToDevice,
                           c->stream));
  // the origin by this path's own rule, not set_fit_origin's: plane / line: a, sphere: c, zeros for every other model
  HIPCHK(c, hipMemsetAsync(c->d_vec, 0, sizeof(double) * 32, c->stream));
  const int m = c->cfg.model;
  if (m == LSQR_MODEL_PLANE || m == LSQR_MODEL_LINE || m == LSQR_MODEL_SPHERE)
    HIPCHK(c, hipMemcpyAsync(c->d_vec, c->d_par + (m == LSQR_MODEL_SPHERE ? 0 : c->ND),
                             sizeof(double) * c->ND, hipMemcpyDeviceToDevice, c->stream));
  bool fused = false;
  if ((st = launch_mask_moments(c, begin, end, nmom, &fused)) != LSQR_OK) return st;
  if (fused) return LSQR_OK;
  if ((st = launch_mask(c, begin, end)) != LSQR_OK) return st;
  return dispatch(c->cfg, [&](auto tag) -> int {
    typedef typename decltype(tag)::type M;
    return launch_moments<M>(c, 1, begin, end, 0, nmom);
  });
}

// ---- RANSAC<T,S>::compute ------------------------------------------------------------------------------
// RANSAC.hxx:129-139 for the winner stashed in d_best (its full scan-parameter row): consensus mask + the
// moment block of its least squares fit in one pass, the fit, one host synchronisation (LM fits: one more per
// evaluation).  The mask count must reproduce the scan's vote count.
static int finish_ransac(lsqr_ctx *c, bool has_best, uint32_t best_votes, double *params_out,
                         uint8_t *consensus_out, lsqr_ransac_info *info) {
  info->best_votes = best_votes;
  info->fraction = (double)best_votes / (double)c->n;
  info->n_params = 0;
  if (!has_best || best_votes == 0) return LSQR_EMPTY;  // RANSAC.hxx:129: nothing written, nothing enqueued
  int st;
  HIPCHK(c, hipMemsetAsync(c->d_par, 0, sizeof(double) * 128, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_par, c->d_best, sizeof(double) * c->HS, hipMemcpyDeviceToDevice, c->stream));
  SolveOut out;
  if ((st = run_winner_finish(c, ORG_WINNER, consensus_out, &out)) != LSQR_OK) return st;
  const unsigned long long cnt = c->h_pin->mask_head[0];
  if (cnt != best_votes)
    return fail(c, LSQR_ERR_HIP, "consensus mask count %llu != scan votes %u", cnt, best_votes);
  fill_ransac_fit(out, cnt, true, &info->fit);
  info->n_params = info->fit.n_params;
  return deliver_params(out, params_out);
}

int lsqr_ransac(lsqr_ctx *c, double p, uint64_t seed, const uint32_t *subsets, size_t n_subsets,
                double *params_out, uint8_t *consensus_out, lsqr_ransac_info *info) {
  lsqr_ransac_info local;
  if (!info) info = &local;
  memset(info, 0, sizeof *info);
  int st = need_ready(c, false);
  if (st != LSQR_OK) return st;
  const int k = c->K;
  // RANSAC.hxx:16-19: return 0, parameters untouched
  if (c->n < (size_t)k || !(p < 1.0) || !(p > 0.0)) return LSQR_ERR_INVALID;
  if ((st = need_ready(c, true)) != LSQR_OK) return st;
  uint64_t rs[6];
  lsqr_replay_init(c->n, k, p, rs);
  DedupSet dedup;
  uint64_t base = 0;
  size_t batch = 256;
  while (!rs[RS_DONE]) {
    size_t H = batch;
    if (subsets) {
      if (base >= n_subsets) break;  // caller's stream exhausted
      H = std::min<size_t>(H, n_subsets - base);
    }
    uint64_t remaining = rs[RS_TRIES] - base;
    if (remaining < H) H = (size_t)remaining;
    if (H == 0) break;
    // batch results land in pinned memory with one synchronisation: {votes[H], subsets[H*k], valid[H]}
    const size_t need = H * sizeof(uint32_t) * (1 + (size_t)k) + H;
    if (need > c->h_batch.cap()) HIPCHK(c, c->h_batch.alloc(std::max<size_t>(need, 1 << 16)));
    uint32_t *p_votes = (uint32_t *)c->h_batch.get(), *p_sub = p_votes + H;
    uint8_t *p_valid = (uint8_t *)(p_sub + H * k);
    if (subsets) {
      memcpy(p_sub, subsets + base * k, H * k * sizeof(uint32_t));
      st = lsqr_hypotheses_from_subsets(c, p_sub, H);
    } else {
      st = lsqr_hypotheses_sample(c, seed, base, H, nullptr);
    }
    if (st != LSQR_OK) return st;
    // what the adaptive bound still asks for (saturated: a poor start leaves it at C(N,k)); the index build
    // heuristic weighs it against the cost of the build
    c->hyp_expected = has_any_best(rs) ? std::min<uint64_t>(rs[RS_TRIES] - base, 1u << 20) : 0;
    if ((st = run_scan_batch(c, has_any_best(rs) ? (uint32_t)rs[RS_BEST] : 0u)) != LSQR_OK) return st;
    c->scanned = true;
    if (!subsets)
      HIPCHK(c, hipMemcpyAsync(p_sub, c->d_subsets, H * k * sizeof(uint32_t), hipMemcpyDeviceToHost,
                               c->stream));
    if ((st = lsqr_get_hypotheses(c, nullptr, p_valid, p_votes)) != LSQR_OK) return st;  // synchronises
    uint64_t prev_best_idx = rs[RS_BEST_IDX];
    bool had = rs[RS_HAS] != 0;
    size_t used = lsqr_replay(c->n, k, p, p_sub, p_valid, p_votes, H, base, &dedup, rs);
    info->evaluated += H;
    if (rs[RS_HAS] && (!had || rs[RS_BEST_IDX] != prev_best_idx)) {
      size_t e = (size_t)(rs[RS_BEST_IDX] - base);
      // the winner's row stays on the device (the next batch overwrites d_hparams): no host round trip
      HIPCHK(c, hipMemcpyAsync(c->d_best, c->d_hparams + e * c->HS, sizeof(double) * c->HS,
                               hipMemcpyDeviceToDevice, c->stream));
      c->win_rec = p_sub[e * k];  // its first drawn record: the fit origin of the ORIGIN_FIRST models
    }
    base += used;
    if (used < H) break;
    batch = std::min<size_t>(batch * 4, 4096);
    // Safety stop (deviation from the reference, which would keep drawing up to C(N,k) subsets):
    // if 2^22 consecutive iterations produced no model at all the data are degenerate.
    if (!rs[RS_HAS] && base >= (1ull << 22)) break;
    if (c->opt.max_iter > 0 && base >= (uint64_t)c->opt.max_iter) break;  // caller's budget
  }
  c->hyp_expected = 0;
  info->iterations = rs[RS_I];
  info->best_index = rs[RS_BEST_IDX];
  return finish_ransac(c, rs[RS_HAS] != 0, (uint32_t)rs[RS_BEST], params_out,
                       consensus_out, info);
}

// ---- sequential RANSAC: several models from one upload (sequential.h) ----------------------------------------------
// Round r is lsqr_ransac itself on the records no earlier round claimed.  Between rounds the survivors are compacted on
// the device and the context is re-pointed at them through set_data_common -- the path of lsqr_upload / lsqr_attach --
// so that everything derived from the records (index, bounds, absmax, fp16 fragments, lanes, selection feedback, the
// win / origin state) starts over as after a real upload.  The caller's records are only read; they are put back, the
// same way, whatever the outcome.
int lsqr_ransac_sequential(lsqr_ctx *c, double p, const uint64_t *seeds, size_t max_models, uint64_t min_votes,
                           double *params_out, int32_t *labels_out, lsqr_ransac_info *infos, int32_t *status_out,
                           size_t *n_models_out) {
  int st = need_ready(c, false);
  if (st != LSQR_OK) return st;
  if (!(p > 0.0) || !(p < 1.0)) return fail(c, LSQR_ERR_INVALID, "lsqr_ransac_sequential: p must lie in (0, 1)");
  if (max_models > 0 && (!seeds || !params_out || !infos || !status_out || !n_models_out))
    return fail(c, LSQR_ERR_INVALID, "lsqr_ransac_sequential: null argument");
  if (max_models == 0) {
    if (n_models_out) *n_models_out = 0;
    return LSQR_OK;
  }
  if (max_models > 0x7FFFFFFFull) return fail(c, LSQR_ERR_INVALID, "lsqr_ransac_sequential: too many models");
  if ((st = need_ready(c, true)) != LSQR_OK) return st;
  if (c->ND < 2 || c->ND > kSeqMaxD) return fail(c, LSQR_ERR_INVALID, "lsqr_ransac_sequential: records of %d doubles", c->ND);
  for (size_t r = 0; r < max_models; r++) status_out[r] = LSQR_ERR_STATE;  // round not run
  memset(infos, 0, sizeof(lsqr_ransac_info) * max_models);
  *n_models_out = 0;

  const double *const data0 = c->d_data;
  const size_t n0 = c->n, stride0 = c->stride;
  const int W = c->ND;
  if (labels_out) {
    if ((st = ensure(c, c->d_seq_labels, n0)) != LSQR_OK) return st;
    HIPCHK(c, hipMemsetAsync(c->d_seq_labels, 0xFF, sizeof(int32_t) * n0, c->stream));  // -1
  }
  int32_t *const d_labels = labels_out ? c->d_seq_labels : nullptr;
  const uint32_t *orig = nullptr;  // upload indices of the current records (null: they are the upload)
  int cur = -1;                    // the owned buffer the context reads (-1: the caller's records)
  size_t r = 0;
  int result = LSQR_OK;
  while (r < max_models && c->n >= (size_t)c->K) {
    st = lsqr_ransac(c, p, seeds[r], nullptr, 0, params_out + r * (size_t)c->P, nullptr, &infos[r]);
    status_out[r] = st;
    if (st != LSQR_OK && st != LSQR_EMPTY) {  // a failure, not an outcome: c->err is lsqr_ransac's
      result = st;
      break;
    }
    if (st != LSQR_OK || (uint64_t)infos[r].best_votes < std::max<uint64_t>(min_votes, 1)) break;  // rejected: claims nothing
    const size_t n_cur = c->n, survivors = n_cur - infos[r].best_votes;
    const int32_t round = (int32_t)r++;
    hipError_t e = hipSuccess;
    if (r == max_models || survivors < (size_t)c->K) {  // no round follows: the labels alone
      if (d_labels) e = seq_label(c->stream, c->d_mask, (uint32_t)n_cur, orig, round, d_labels, (uint32_t)n0);
      if (e != hipSuccess) result = fail(c, LSQR_ERR_HIP, "lsqr_ransac_sequential: %s", hipGetErrorString(e));
      break;
    }
    const int dst = cur == 0 ? 1 : 0;
    if ((st = ensure(c, c->d_seq_rec[dst], survivors * (size_t)W)) != LSQR_OK ||
        (st = ensure(c, c->d_seq_orig[dst], survivors)) != LSQR_OK ||
        (st = ensure(c, c->d_seq_counts, (size_t)seq_chunks(n_cur))) != LSQR_OK) {
      result = st;
      break;
    }
    e = seq_partition(c->stream, c->d_data, c->stride, (uint32_t)n_cur, W, c->d_mask, orig, c->d_seq_counts,
                      (uint32_t)survivors, round, c->d_seq_rec[dst], c->d_seq_orig[dst], d_labels, (uint32_t)n0);
    if (e != hipSuccess) {
      result = fail(c, LSQR_ERR_HIP, "lsqr_ransac_sequential: %s", hipGetErrorString(e));
      break;
    }
    if ((st = set_data_common(c, survivors, sizeof(double) * (size_t)W)) != LSQR_OK) {
      result = st;
      break;
    }
    c->d_data = c->d_seq_rec[dst];
    orig = c->d_seq_orig[dst];
    cur = dst;
  }
  *n_models_out = r;
  if (result == LSQR_OK && labels_out) {
    hipError_t e = hipMemcpyAsync(labels_out, d_labels, sizeof(int32_t) * n0, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = sync_stream(c);
    if (e != hipSuccess) result = fail(c, LSQR_ERR_HIP, "lsqr_ransac_sequential: %s", hipGetErrorString(e));
  } else if (result != LSQR_OK) {
    (void)sync_stream(c);  // nothing of this call is left in flight on the scratch buffers
  }
  // the caller's records again, as after lsqr_upload / lsqr_attach (hypotheses, mask and index are void)
  char keep[sizeof c->err];
  memcpy(keep, c->err, sizeof keep);
  st = set_data_common(c, n0, sizeof(double) * stride0);
  c->d_data = data0;
  if (result != LSQR_OK) memcpy(c->err, keep, sizeof keep);
  return result != LSQR_OK ? result : st;
}

// ---- many independent problems in one call (many.h, many_lm.h, many_dense.h, many_exhaustive.h) --------------------
// What the seven batched entry points share.  The checks, in the contract's order: the context is ready; the entry
// point's model gate (gate(): LSQR_OK, or its own fail()); n == 0 is LSQR_OK with every output untouched; null
// arguments (args: the entry point's own pointers are all there); p, where given (the RANSAC kind); offsets; records;
// stride.  Then the job from the context -- the caller has set what its kind alone has: p, the seeds and the outputs
// -- and run(J, tag), dispatched on the model.  J.lm is the geometric sphere, which only the _lm gates let through.
extern "C++" {
// what every batched job takes from the context: the stream, the model, the options and the context's ManyBufs.  The
// one place where an option reaches a job, for many_call's entry points and for lsqr_ransac_grouped alike.
static void many_job_from_ctx(lsqr_ctx *c, ManyJob &J) {
  if (!c->many) c->many.reset(new ManyBufs());
  J.stream = c->stream;
  J.cfg = c->cfg;
  J.mc = c->mc;
  J.W = c->ND;  // lsqr_record_doubles(cfg)
  J.max_iter = c->opt.max_iter;
  J.round_cap = c->opt.many_round > 0 ? (size_t)c->opt.many_round : 0;
  J.lm = c->cfg.model == LSQR_MODEL_SPHERE && c->cfg.ls_type == LSQR_LS_GEOMETRIC;
  lm_settings(c->cfg, &J.lm_n, &J.lm_ftol, &J.lm_xtol, &J.lm_gtol, &J.lm_maxfev);
  J.dense_fast = c->opt.dense_fast ? 1 : 0;
  J.dense_dd = c->opt.dense_dd ? 1 : 0;
  J.ex_fused = c->opt.many_ex_fused ? 1 : 0;
  J.buf = c->many.get();
}

template <class Gate, class Run>
static int many_call(lsqr_ctx *c, const char *fn, ManyJob &J, const void *host_records, size_t stride_bytes,
                     const uint64_t *offsets, size_t n, bool args, const double *p, Gate &&gate, Run &&run) {
  int st = need_ready(c, false);
  if (st != LSQR_OK) return st;
  if ((st = gate()) != LSQR_OK) return st;
  if (n == 0) return LSQR_OK;
  if (!offsets || !args) return fail(c, LSQR_ERR_INVALID, "%s: null argument", fn);
  if (p && (!(*p > 0.0) || !(*p < 1.0))) return fail(c, LSQR_ERR_INVALID, "%s: p must lie in (0, 1)", fn);
  if (offsets[0] != 0) return fail(c, LSQR_ERR_INVALID, "%s: offsets[0] must be 0", fn);
  for (size_t j = 0; j < n; j++) {
    if (offsets[j + 1] < offsets[j]) return fail(c, LSQR_ERR_INVALID, "%s: offsets decrease at %zu", fn, j);
    if (offsets[j + 1] - offsets[j] > 0xFFFFFFF0ull)
      return fail(c, LSQR_ERR_INVALID, "%s: problem %zu has more than 2^32 - 16 records", fn, j);
  }
  if (offsets[n] > 0 && !host_records) return fail(c, LSQR_ERR_INVALID, "%s: null records", fn);
  if (stride_bytes < sizeof(double) * (size_t)c->ND)
    return fail(c, LSQR_ERR_INVALID, "%s: stride %zu below the record's %zu bytes", fn, stride_bytes,
                sizeof(double) * (size_t)c->ND);
  many_job_from_ctx(c, J);
  J.host = (const char *)host_records;
  J.stride = stride_bytes;
  J.offsets = offsets;
  J.n = n;
  st = dispatch(c->cfg, [&](auto tag) -> int { return run(J, tag); });
  if (st != LSQR_OK) return fail(c, st, "%s: %s", fn, J.err[0] ? J.err : "model not in this build");
  return LSQR_OK;
}

// the RANSAC kind: lsqr_ransac_many, _lm and _dense take the same arguments
template <class Gate, class Run>
static int many_ransac_call(lsqr_ctx *c, const char *fn, const void *host_records, size_t stride_bytes,
                            const uint64_t *offsets, size_t n_problems, double p, const uint64_t *seeds,
                            double *params_out, uint8_t *consensus_out, lsqr_ransac_info *infos, int32_t *status_out,
                            Gate &&gate, Run &&run) {
  ManyJob J;
  J.p = p;
  J.seeds = seeds;
  J.params_out = params_out;
  J.consensus_out = consensus_out;
  J.infos = infos;
  J.status_out = status_out;
  return many_call(c, fn, J, host_records, stride_bytes, offsets, n_problems,
                   seeds && params_out && infos && status_out, &p, gate, run);
}
}  // extern "C++"

// many independent RANSAC<T,S>::compute() problems of the closed-form models (many.h)
int lsqr_ransac_many(lsqr_ctx *c, const void *host_records, size_t stride_bytes, const uint64_t *offsets,
                     size_t n_problems, double p, const uint64_t *seeds, double *params_out, uint8_t *consensus_out,
                     lsqr_ransac_info *infos, int32_t *status_out) {
  return many_ransac_call(
      c, "lsqr_ransac_many", host_records, stride_bytes, offsets, n_problems, p, seeds, params_out, consensus_out,
      infos, status_out,
      [&]() -> int {
        const lsqr_model_cfg &cfg = c->cfg;
        if (cfg.model != LSQR_MODEL_PLANE && cfg.model != LSQR_MODEL_LINE && cfg.model != LSQR_MODEL_SPHERE &&
            cfg.model != LSQR_MODEL_ABSOR && cfg.model != LSQR_MODEL_PIVOT && cfg.model != LSQR_MODEL_RAY &&
            cfg.model != LSQR_MODEL_LINE2D)
          return fail(c, LSQR_ERR_INVALID,
                      "lsqr_ransac_many: plane, line, algebraic sphere, absolute orientation, pivot, ray and 2-D line "
                      "only (model %d)", cfg.model);
        if (cfg.model == LSQR_MODEL_SPHERE && cfg.ls_type != LSQR_LS_ALGEBRAIC)
          return fail(c, LSQR_ERR_INVALID,
                      "lsqr_ransac_many: the geometric (LM) sphere fit is not batched; use LSQR_LS_ALGEBRAIC");
        return LSQR_OK;
      },
      [](ManyJob &J, auto tag) -> int {
        typedef typename decltype(tag)::type M;
        if constexpr (ManyModel<M>::value) return many_run<M>(J);
        else return LSQR_ERR_INVALID;
      });
}

// the same with the geometric sphere's Levenberg-Marquardt finish (many.h + many_lm.h)
int lsqr_ransac_many_lm(lsqr_ctx *c, const void *host_records, size_t stride_bytes, const uint64_t *offsets,
                        size_t n_problems, double p, const uint64_t *seeds, double *params_out,
                        uint8_t *consensus_out, lsqr_ransac_info *infos, int32_t *status_out) {
  return many_ransac_call(
      c, "lsqr_ransac_many_lm", host_records, stride_bytes, offsets, n_problems, p, seeds, params_out, consensus_out,
      infos, status_out,
      [&]() -> int {
        if (c->cfg.model == LSQR_MODEL_SPHERE && c->cfg.ls_type == LSQR_LS_GEOMETRIC) return LSQR_OK;
        return fail(c, LSQR_ERR_INVALID,
                    "lsqr_ransac_many_lm: the geometric sphere only (model %d, ls_type %d); the closed-form fits are "
                    "batched by lsqr_ransac_many", c->cfg.model, c->cfg.ls_type);
      },
      [](ManyJob &J, auto tag) -> int {
        typedef typename decltype(tag)::type M;
        if constexpr (ManyModel<M>::value && requires { M::NMOM_LM; }) return many_run<M>(J);
        else return LSQR_ERR_INVALID;
      });
}

int lsqr_lm_fit_many(lsqr_ctx *c, const void *host_records, size_t stride_bytes, const uint64_t *offsets,
                     size_t n_sets, const uint8_t *masks, const double *x0, double *params_out, lsqr_fit_info *fits,
                     int32_t *status_out) {
  ManyJob J;
  J.params_out = params_out;
  J.status_out = status_out;
  return many_call(
      c, "lsqr_lm_fit_many", J, host_records, stride_bytes, offsets, n_sets, x0 && params_out && fits && status_out,
      nullptr,
      [&]() -> int {
        if (c->cfg.model == LSQR_MODEL_SPHERE && c->cfg.ls_type == LSQR_LS_GEOMETRIC) return LSQR_OK;
        return fail(c, LSQR_ERR_INVALID,
                    "lsqr_lm_fit_many: the geometric sphere only (model %d, ls_type %d); the closed-form fits of many "
                    "problems are batched by lsqr_ransac_many", c->cfg.model, c->cfg.ls_type);
      },
      [&](ManyJob &J, auto tag) -> int {
        typedef typename decltype(tag)::type M;
        if constexpr (ManyModel<M>::value && requires { M::NMOM_LM; }) return many_lm_fit<M>(J, masks, x0, fits);
        else return LSQR_ERR_INVALID;
      });
}

// the same for the dense linear system (many_dense.h)
int lsqr_ransac_many_dense(lsqr_ctx *c, const void *host_records, size_t stride_bytes, const uint64_t *offsets,
                           size_t n_problems, double p, const uint64_t *seeds, double *params_out,
                           uint8_t *consensus_out, lsqr_ransac_info *infos, int32_t *status_out) {
  return many_ransac_call(
      c, "lsqr_ransac_many_dense", host_records, stride_bytes, offsets, n_problems, p, seeds, params_out,
      consensus_out, infos, status_out,
      [&]() -> int {
        if (c->cfg.model == LSQR_MODEL_DENSE) return LSQR_OK;
        return fail(c, LSQR_ERR_INVALID,
                    "lsqr_ransac_many_dense: the dense linear system only (model %d); the other models are batched by "
                    "lsqr_ransac_many / lsqr_ransac_many_lm", c->cfg.model);
      },
      [](ManyJob &J, auto tag) -> int {
        typedef typename decltype(tag)::type M;
        if constexpr (M::IS_DENSE) return many_dense_run<M::NR>(J);
        else return LSQR_ERR_INVALID;
      });
}

int lsqr_dense_fit_many(lsqr_ctx *c, const void *host_records, size_t stride_bytes, const uint64_t *offsets,
                        size_t n_sets, const uint8_t *masks, double *params_out, lsqr_fit_info *fits,
                        int32_t *status_out) {
  ManyJob J;
  J.params_out = params_out;
  J.status_out = status_out;
  return many_call(
      c, "lsqr_dense_fit_many", J, host_records, stride_bytes, offsets, n_sets, params_out && fits && status_out,
      nullptr,
      [&]() -> int {
        if (c->cfg.model == LSQR_MODEL_DENSE) return LSQR_OK;
        return fail(c, LSQR_ERR_INVALID, "lsqr_dense_fit_many: the dense linear system only (model %d)",
                    c->cfg.model);
      },
      [&](ManyJob &J, auto tag) -> int {
        typedef typename decltype(tag)::type M;
        if constexpr (M::IS_DENSE) return many_dense_fit<M::NR>(J, masks, fits);
        else return LSQR_ERR_INVALID;
      });
}

// many independent problems of the exhaustive overload (many_exhaustive.h); the geometric sphere's winners get the
// LM stage, as in lsqr_ransac_many_lm
int lsqr_ransac_many_exhaustive(lsqr_ctx *c, const void *host_records, size_t stride_bytes, const uint64_t *offsets,
                                size_t n_problems, double *params_out, uint8_t *consensus_out,
                                lsqr_ransac_info *infos, int32_t *status_out) {
  ManyJob J;
  J.params_out = params_out;
  J.consensus_out = consensus_out;
  J.infos = infos;
  J.status_out = status_out;
  return many_call(
      c, "lsqr_ransac_many_exhaustive", J, host_records, stride_bytes, offsets, n_problems,
      params_out && infos && status_out, nullptr,
      [&]() -> int {
        const lsqr_model_cfg &cfg = c->cfg;
        if (cfg.model == LSQR_MODEL_PLANE || cfg.model == LSQR_MODEL_LINE || cfg.model == LSQR_MODEL_SPHERE ||
            cfg.model == LSQR_MODEL_ABSOR || cfg.model == LSQR_MODEL_PIVOT || cfg.model == LSQR_MODEL_RAY ||
            cfg.model == LSQR_MODEL_LINE2D)
          return LSQR_OK;
        return fail(c, LSQR_ERR_INVALID,
                    "lsqr_ransac_many_exhaustive: plane, line, sphere, absolute orientation, pivot, ray and 2-D line "
                    "only (model %d)", cfg.model);
      },
      [](ManyJob &J, auto tag) -> int {
        typedef typename decltype(tag)::type M;
        if constexpr (ManyModel<M>::value) return many_ex_run<M>(J);
        else return LSQR_ERR_INVALID;
      });
}

// sequential RANSAC over many problems (many_sequential.h): every round is one job of many_run / many_dense_run on the
// survivors, which stay on the device
int lsqr_ransac_many_sequential(lsqr_ctx *c, const void *host_records, size_t stride_bytes, const uint64_t *offsets,
                                size_t n_problems, double p, const uint64_t *seeds, size_t max_models,
                                uint64_t min_votes, double *params_out, int32_t *labels_out, lsqr_ransac_info *infos,
                                int32_t *status_out, size_t *n_models_out) {
  const char *fn = "lsqr_ransac_many_sequential";
  ManyJob J;
  J.p = p;
  return many_call(
      c, fn, J, host_records, stride_bytes, offsets, n_problems,
      max_models == 0 || (seeds && params_out && infos && status_out && n_models_out), &p,
      [&]() -> int {
        const lsqr_model_cfg &cfg = c->cfg;
        if (cfg.model == LSQR_MODEL_US_SINGLE || cfg.model == LSQR_MODEL_US_POINTER || cfg.model == LSQR_MODEL_PHANTOM)
          return fail(c, LSQR_ERR_INVALID,
                      "%s: the models of lsqr_ransac_many, lsqr_ransac_many_lm and lsqr_ransac_many_dense only "
                      "(model %d)", fn, cfg.model);
        if (max_models > 0x7FFFFFFFull) return fail(c, LSQR_ERR_INVALID, "%s: too many models", fn);
        return LSQR_OK;
      },
      [&](ManyJob &J, auto tag) -> int {
        typedef typename decltype(tag)::type M;
        if (max_models == 0) {
          if (n_models_out) memset(n_models_out, 0, sizeof(size_t) * n_problems);
          return LSQR_OK;
        }
        if constexpr (M::IS_DENSE) {
          const int n = (int)J.cfg.dim;
          return many_seq_run(J, n, n, seeds, max_models, min_votes, params_out, labels_out, false, infos, status_out,
                              n_models_out, [](ManyJob &S) -> int { return many_dense_run<M::NR>(S); });
        } else if constexpr (ManyModel<M>::value) {
          // (the sphere: J.lm says whether the rounds end in the LM stage, as lsqr_ransac_many_lm)
          return many_seq_run(J, (int)M::K, (int)M::P, seeds, max_models, min_votes, params_out, labels_out, false,
                              infos, status_out, n_models_out, [](ManyJob &S) -> int { return many_run<M>(S); });
        } else {
          return LSQR_ERR_INVALID;
        }
      });
}

// one problem per label over the context's own records (grouped.h): grouped on the device into the batched calls'
// packed buffer, one job of many_run / many_dense_run on that copy, the consensus back in upload order
int lsqr_ransac_grouped(lsqr_ctx *c, const int32_t *groups, size_t n_groups, int on_device, double p,
                        const uint64_t *seeds, double *params_out, uint8_t *consensus_out, uint64_t *offsets_out,
                        lsqr_ransac_info *infos, int32_t *status_out) {
  const char *fn = "lsqr_ransac_grouped";
  int st = need_ready(c, false);
  if (st != LSQR_OK) return st;
  const lsqr_model_cfg &cfg = c->cfg;
  if (cfg.model == LSQR_MODEL_US_SINGLE || cfg.model == LSQR_MODEL_US_POINTER || cfg.model == LSQR_MODEL_PHANTOM)
    return fail(c, LSQR_ERR_INVALID,
                "%s: the models of lsqr_ransac_many, lsqr_ransac_many_lm and lsqr_ransac_many_dense only (model %d)",
                fn, cfg.model);
  if (n_groups == 0) return LSQR_OK;  // (the order of many_call's checks)
  if (!groups || !seeds || !params_out || !infos || !status_out)
    return fail(c, LSQR_ERR_INVALID, "%s: null argument", fn);
  if (!(p > 0.0) || !(p < 1.0)) return fail(c, LSQR_ERR_INVALID, "%s: p must lie in (0, 1)", fn);
  if (n_groups > 0x7FFFFFFFull) return fail(c, LSQR_ERR_INVALID, "%s: more than 2^31 - 1 groups", fn);
  if ((st = need_ready(c, true)) != LSQR_OK) return st;
  if (c->n > 0xFFFFFFF0ull) return fail(c, LSQR_ERR_INVALID, "%s: more than 2^32 - 16 records", fn);
  ManyJob J;
  many_job_from_ctx(c, J);  // (the same fill as many_call's: the bit-identity rests on it)
  J.resident = true;
  J.n = n_groups;
  J.p = p;
  J.seeds = seeds;
  J.params_out = params_out;
  J.infos = infos;
  J.status_out = status_out;
  const double *data = c->d_data;
  const size_t stride = c->stride, N = c->n;
  st = dispatch(c->cfg, [&](auto tag) -> int {
    typedef typename decltype(tag)::type M;
    if constexpr (M::IS_DENSE)
      return grouped_run(J, data, stride, N, groups, on_device, consensus_out, offsets_out,
                         [](ManyJob &S) -> int { return many_dense_run<M::NR>(S); });
    else if constexpr (ManyModel<M>::value)  // (the sphere: J.lm says whether the job ends in the LM stage)
      return grouped_run(J, data, stride, N, groups, on_device, consensus_out, offsets_out,
                         [](ManyJob &S) -> int { return many_run<M>(S); });
    else
      return LSQR_ERR_INVALID;
  });
  if (st != LSQR_OK) return fail(c, st, "%s: %s", fn, J.err[0] ? J.err : "model not in this build");
  return LSQR_OK;
}

// several models per label over the context's own records (grouped.h): the front half of lsqr_ransac_grouped, then
// the rounds of lsqr_ransac_many_sequential on the resident packed copy, the round labels back in upload order
int lsqr_ransac_grouped_sequential(lsqr_ctx *c, const int32_t *groups, size_t n_groups, int on_device, double p,
                                   const uint64_t *seeds, size_t max_models, uint64_t min_votes, double *params_out,
                                   int32_t *labels_out, uint64_t *offsets_out, lsqr_ransac_info *infos,
                                   int32_t *status_out, size_t *n_models_out) {
  const char *fn = "lsqr_ransac_grouped_sequential";
  int st = need_ready(c, false);
  if (st != LSQR_OK) return st;
  const lsqr_model_cfg &cfg = c->cfg;
  if (cfg.model == LSQR_MODEL_US_SINGLE || cfg.model == LSQR_MODEL_US_POINTER || cfg.model == LSQR_MODEL_PHANTOM)
    return fail(c, LSQR_ERR_INVALID,
                "%s: the models of lsqr_ransac_many, lsqr_ransac_many_lm and lsqr_ransac_many_dense only (model %d)",
                fn, cfg.model);
  if (n_groups == 0) return LSQR_OK;  // (the order of lsqr_ransac_grouped's checks, then lsqr_ransac_many_sequential's)
  if (max_models > 0 && (!groups || !seeds || !params_out || !infos || !status_out || !n_models_out))
    return fail(c, LSQR_ERR_INVALID, "%s: null argument", fn);
  if (!(p > 0.0) || !(p < 1.0)) return fail(c, LSQR_ERR_INVALID, "%s: p must lie in (0, 1)", fn);
  if (n_groups > 0x7FFFFFFFull) return fail(c, LSQR_ERR_INVALID, "%s: more than 2^31 - 1 groups", fn);
  if (max_models > 0x7FFFFFFFull) return fail(c, LSQR_ERR_INVALID, "%s: too many models", fn);
  if ((st = need_ready(c, true)) != LSQR_OK) return st;
  if (c->n > 0xFFFFFFF0ull) return fail(c, LSQR_ERR_INVALID, "%s: more than 2^32 - 16 records", fn);
  if (max_models == 0) {
    if (n_models_out) memset(n_models_out, 0, sizeof(size_t) * n_groups);
    return LSQR_OK;
  }
  ManyJob J;
  many_job_from_ctx(c, J);  // (the same fill as many_call's: the bit-identity rests on it)
  J.resident = true;
  J.n = n_groups;
  J.p = p;
  const double *data = c->d_data;
  const size_t stride = c->stride, N = c->n;
  st = dispatch(c->cfg, [&](auto tag) -> int {
    typedef typename decltype(tag)::type M;
    if constexpr (M::IS_DENSE) {
      const int n = (int)J.cfg.dim;
      return grouped_seq_run(J, data, stride, N, groups, on_device, n, n, seeds, max_models, min_votes, params_out,
                             labels_out, offsets_out, infos, status_out, n_models_out,
                             [](ManyJob &S) -> int { return many_dense_run<M::NR>(S); });
    } else if constexpr (ManyModel<M>::value) {  // (the sphere: J.lm says whether the rounds end in the LM stage)
      return grouped_seq_run(J, data, stride, N, groups, on_device, (int)M::K, (int)M::P, seeds, max_models, min_votes,
                             params_out, labels_out, offsets_out, infos, status_out, n_models_out,
                             [](ManyJob &S) -> int { return many_run<M>(S); });
    } else {
      return LSQR_ERR_INVALID;
    }
  });
  if (st != LSQR_OK) return fail(c, st, "%s: %s", fn, J.err[0] ? J.err : "model not in this build");
  return LSQR_OK;
}

// ---- nearest-model assignment and refit (assign.h, assign_dense.h, assign_rigid.h, assign_grouped.h, ...) -----------
// What the fourteen entry points share.  The checks, in the contract's order: the context; the model gate (AssignGate:
// which models the entry point takes, and what it does with the geometric sphere, whose fit is iterative); count == 0
// (n_models, or n_groups of the grouped calls) is LSQR_OK with every output untouched; more than 64 models; own(), the
// entry point's own arguments; the context holds a model and records; their count.  Then run(tag), the run function
// on the model -- it has waited for the stream when it returns.  The context's upload, hypotheses, mask, index and
// d_par are not touched: the calls have buffers of their own (lsqr_ctx::assign, assign_dense, assign_grp,
// assign_dense_grp).
extern "C++" {
enum AssignGate {
  ASSIGN_GATE_ANY,     // the assignments: every model of assign_model_ok
  ASSIGN_GATE_CLOSED,  // the refits in closed form: not the geometric sphere
  ASSIGN_GATE_LM,      // lsqr_refine_lm, lsqr_refine_lm_grouped: the geometric sphere alone
  ASSIGN_GATE_DENSE,   // lsqr_assign_dense, lsqr_refine_dense and their grouped forms: the dense linear system alone
  ASSIGN_GATE_RIGID    // lsqr_assign_rigid, lsqr_refine_rigid: absolute orientation, pivot and ray (no grouped form)
};
// the entry point that takes what the gate refuses, [grouped][gate]
static const char *const kAssignTakes[2][5] = {
    {"", "lsqr_refine_lm", "lsqr_refine", "lsqr_assign / lsqr_refine", "lsqr_assign / lsqr_refine"},
    {"", "lsqr_refine_lm_grouped", "lsqr_refine_grouped", "lsqr_assign_grouped / lsqr_refine_grouped", ""}};
// the models run(tag) is compiled for
template <AssignGate G, class M>
constexpr bool kAssignTakesModel = G == ASSIGN_GATE_DENSE   ? (bool)M::IS_DENSE
                                   : G == ASSIGN_GATE_RIGID ? AssignRigidModel<M>::value
                                                            : AssignModel<M>::value;

template <AssignGate G, class Own, class Run>
static int assign_frame(lsqr_ctx *c, const char *fn, bool grouped, size_t count, size_t max_models, const char *err,
                        Own own, Run run) {
  const char *takes = kAssignTakes[grouped][G];
  int st = need_ready(c, false);
  if (st != LSQR_OK) return st;
  if (G == ASSIGN_GATE_DENSE) {
    if (c->cfg.model != LSQR_MODEL_DENSE)
      return fail(c, LSQR_ERR_INVALID, "%s: the dense linear system only (model %d); %s take "
                  "the plane, line, sphere and 2-D line", fn, c->cfg.model, takes);
  } else if (G == ASSIGN_GATE_RIGID) {
    if (!assign_rigid_model_ok(c->cfg))
      return fail(c, LSQR_ERR_INVALID, "%s: absolute orientation, pivot calibration and ray intersection only (model "
                  "%d); %s take the plane, line, sphere and 2-D line", fn, c->cfg.model, takes);
  } else if (G == ASSIGN_GATE_LM) {
    if (!(c->cfg.model == LSQR_MODEL_SPHERE && c->cfg.ls_type == LSQR_LS_GEOMETRIC))
      return fail(c, LSQR_ERR_INVALID, "%s: the sphere with LSQR_LS_GEOMETRIC only (model %d); %s takes the fits in "
                  "closed form", fn, c->cfg.model, takes);
  } else {
    if (!assign_model_ok(c->cfg))
      return fail(c, LSQR_ERR_INVALID, "%s: plane, line, sphere and 2-D line only (model %d)", fn, c->cfg.model);
    if (G == ASSIGN_GATE_CLOSED && wants_lm(c->cfg))
      return fail(c, LSQR_ERR_INVALID, "%s: the geometric sphere's fit is iterative; %s takes it", fn, takes);
  }
  if (count == 0) return LSQR_OK;
  if (max_models > (size_t)kAssignMaxModels) return fail(c, LSQR_ERR_INVALID, "%s: more than 64 models", fn);
  if ((st = own()) != LSQR_OK) return st;
  if ((st = need_ready(c, true)) != LSQR_OK) return st;
  if (c->n > 0xFFFFFFF0ull) return fail(c, LSQR_ERR_INVALID, "%s: more than 2^32 - 16 records", fn);
  st = dispatch(c->cfg, [&](auto tag) -> int {
    if constexpr (kAssignTakesModel<G, typename decltype(tag)::type>) return run(tag);
    else return LSQR_ERR_INVALID;
  });
  if (st != LSQR_OK) {
    (void)sync_stream(c);  // nothing of this call is left in flight on its buffers
    return fail(c, st, "%s: %s", fn, err[0] ? err : "model not in this build");
  }
  bsel_host_synced(c);
  return LSQR_OK;
}

// the eight ungrouped calls: the round loop (assign_rounds) with the gate's family; args: the entry point's own
// pointers are all there
template <AssignGate G>
static int assign_call(lsqr_ctx *c, const char *fn, bool args, AssignJob &J) {
  return assign_frame<G>(
      c, fn, false, J.n_models, J.n_models, J.err,
      [&]() -> int { return args ? LSQR_OK : fail(c, LSQR_ERR_INVALID, "%s: null argument", fn); },
      [&](auto tag) -> int {
        J.stream = c->stream;
        J.cfg = c->cfg;
        J.mc = c->mc;
        J.data = c->d_data;
        J.stride = c->stride;
        J.n = (uint32_t)c->n;
        typedef typename decltype(tag)::type M;
        if constexpr (G == ASSIGN_GATE_DENSE) {
          if (!c->assign_dense) c->assign_dense.reset(new AssignDenseBufs());
          const int fast = c->opt.dense_fast ? 1 : 0, dd = c->opt.dense_dd ? 1 : 0;
          return assign_rounds(J, AssignDense<M::NR>{*c->assign_dense, fast, dd});
        } else {
          if (!c->assign) c->assign.reset(new AssignBufs());
          if constexpr (G == ASSIGN_GATE_RIGID) return assign_rounds(J, AssignRigid<M>{{*c->assign}});
          else if constexpr (G != ASSIGN_GATE_LM) return assign_rounds(J, AssignClosed<M>{*c->assign});
          else if constexpr (requires { M::NMOM_LM; }) return assign_rounds(J, AssignLm<M>{{*c->assign}});  // (the sphere)
          else return LSQR_ERR_INVALID;
        }
      });
}

// lsqr_assign, lsqr_assign_dense and lsqr_assign_rigid
template <AssignGate G>
static int assign_only_call(lsqr_ctx *c, const char *fn, const double *params, size_t n_models, int on_device,
                            int32_t *labels_out, double *residuals_out, uint64_t *counts_out) {
  AssignJob J;
  J.params = const_cast<double *>(params);  // (read only: no refit runs)
  J.n_models = n_models;
  J.max_rounds = 0;
  J.on_device = on_device ? 1 : 0;
  J.labels_out = labels_out;
  J.residuals_out = residuals_out;
  J.counts_out = counts_out;
  return assign_call<G>(c, fn, params && labels_out, J);
}

// lsqr_refine, lsqr_refine_lm, lsqr_refine_dense and lsqr_refine_rigid
template <AssignGate G>
static int refine_call(lsqr_ctx *c, const char *fn, double *params_inout, size_t n_models, size_t max_rounds,
                       int on_device, int32_t *labels_out, uint64_t *counts_out, lsqr_fit_info *fits,
                       int32_t *status_out, size_t *rounds_out, int *converged_out) {
  AssignJob J;
  J.params = params_inout;
  J.n_models = n_models;
  J.max_rounds = max_rounds;
  J.on_device = on_device ? 1 : 0;
  J.labels_out = labels_out;
  J.counts_out = counts_out;
  J.fits = fits;
  J.status_out = status_out;
  const bool args = params_inout && fits && status_out && rounds_out && converged_out;
  const int st = assign_call<G>(c, fn, args, J);
  if (st == LSQR_OK && n_models > 0) {
    *rounds_out = J.rounds;
    *converged_out = J.converged;
  }
  return st;
}
}  // extern "C++"

int lsqr_assign(lsqr_ctx *c, const double *params, size_t n_models, int on_device, int32_t *labels_out,
                double *residuals_out, uint64_t *counts_out) {
  return assign_only_call<ASSIGN_GATE_ANY>(c, "lsqr_assign", params, n_models, on_device, labels_out, residuals_out,
                                           counts_out);
}

int lsqr_refine(lsqr_ctx *c, double *params_inout, size_t n_models, size_t max_rounds, int on_device,
                int32_t *labels_out, uint64_t *counts_out, lsqr_fit_info *fits, int32_t *status_out,
                size_t *rounds_out, int *converged_out) {
  return refine_call<ASSIGN_GATE_CLOSED>(c, "lsqr_refine", params_inout, n_models, max_rounds, on_device, labels_out,
                                         counts_out, fits, status_out, rounds_out, converged_out);
}

int lsqr_refine_lm(lsqr_ctx *c, double *params_inout, size_t n_models, size_t max_rounds, int on_device,
                   int32_t *labels_out, uint64_t *counts_out, lsqr_fit_info *fits, int32_t *status_out,
                   size_t *rounds_out, int *converged_out) {
  return refine_call<ASSIGN_GATE_LM>(c, "lsqr_refine_lm", params_inout, n_models, max_rounds, on_device, labels_out,
                                     counts_out, fits, status_out, rounds_out, converged_out);
}

int lsqr_assign_dense(lsqr_ctx *c, const double *params, size_t n_models, int on_device, int32_t *labels_out,
                      double *residuals_out, uint64_t *counts_out) {
  return assign_only_call<ASSIGN_GATE_DENSE>(c, "lsqr_assign_dense", params, n_models, on_device, labels_out,
                                             residuals_out, counts_out);
}

int lsqr_refine_dense(lsqr_ctx *c, double *params_inout, size_t n_models, size_t max_rounds, int on_device,
                      int32_t *labels_out, uint64_t *counts_out, lsqr_fit_info *fits, int32_t *status_out,
                      size_t *rounds_out, int *converged_out) {
  return refine_call<ASSIGN_GATE_DENSE>(c, "lsqr_refine_dense", params_inout, n_models, max_rounds, on_device,
                                        labels_out, counts_out, fits, status_out, rounds_out, converged_out);
}

int lsqr_assign_rigid(lsqr_ctx *c, const double *params, size_t n_models, int on_device, int32_t *labels_out,
                      double *residuals_out, uint64_t *counts_out) {
  return assign_only_call<ASSIGN_GATE_RIGID>(c, "lsqr_assign_rigid", params, n_models, on_device, labels_out,
                                             residuals_out, counts_out);
}

int lsqr_refine_rigid(lsqr_ctx *c, double *params_inout, size_t n_models, size_t max_rounds, int on_device,
                      int32_t *labels_out, uint64_t *counts_out, lsqr_fit_info *fits, int32_t *status_out,
                      size_t *rounds_out, int *converged_out) {
  return refine_call<ASSIGN_GATE_RIGID>(c, "lsqr_refine_rigid", params_inout, n_models, max_rounds, on_device,
                                        labels_out, counts_out, fits, status_out, rounds_out, converged_out);
}

// lsqr_assign_grouped, lsqr_refine_grouped, lsqr_refine_lm_grouped and the dense pair: the grouped round loop
// (assign_grouped_rounds) with the gate's family.  The sort and the packed copy live in the batched calls' buffers
// (lsqr_ctx::many), as lsqr_ransac_grouped's do.  (The dense gate serves an assignment and a refit: J.refine is its
// caller's.)
extern "C++" {
template <AssignGate G>
static int assign_grouped_call(lsqr_ctx *c, const char *fn, bool args, AssignGrpJob &J) {
  if (G != ASSIGN_GATE_DENSE) J.refine = G != ASSIGN_GATE_ANY;
  return assign_frame<G>(
      c, fn, true, J.n_groups, J.max_models, J.err,
      [&]() -> int {
        if (J.n_groups > 0x7FFFFFFFull) return fail(c, LSQR_ERR_INVALID, "%s: more than 2^31 - 1 groups", fn);
        if (!args || !J.groups || !J.params || !J.n_models) return fail(c, LSQR_ERR_INVALID, "%s: null argument", fn);
        for (size_t g = 0; g < J.n_groups; g++)
          if (J.n_models[g] > J.max_models)
            return fail(c, LSQR_ERR_INVALID, "%s: n_models[%zu] is above max_models", fn, g);
        return LSQR_OK;
      },
      [&](auto tag) -> int {
        if (!c->assign_grp) c->assign_grp.reset(new AssignGrpBufs());
        many_job_from_ctx(c, J.pack);
        J.pack.resident = true;
        J.pack.n = J.n_groups;
        J.cfg = c->cfg;
        J.mc = c->mc;
        J.data = c->d_data;
        J.stride = c->stride;
        J.n = c->n;
        typedef typename decltype(tag)::type M;
        if constexpr (G == ASSIGN_GATE_DENSE) {
          if (!c->assign_dense_grp) c->assign_dense_grp.reset(new AssignDenseGrpBufs());
          const int dim = (int)c->cfg.dim;
          return assign_grouped_rounds(J, AssignGrpDense<M::NR>{c->assign_grp->core, *c->assign_dense_grp,
                                                                J.pack.dense_fast, J.pack.dense_dd, dim,
                                                                many_dense_ps(dim)});
        } else {
          AssignGrpBufs &B = *c->assign_grp;
          if constexpr (G != ASSIGN_GATE_LM) return assign_grouped_rounds(J, AssignGrpClosed<M>{B});
          else if constexpr (requires { M::NMOM_LM; }) return assign_grouped_rounds(J, AssignGrpLm<M>{{B}});  // (sphere)
          else return LSQR_ERR_INVALID;
        }
      });
}

// lsqr_refine_grouped, lsqr_refine_lm_grouped and lsqr_refine_dense_grouped
template <AssignGate G>
static int refine_grouped_call(lsqr_ctx *c, const char *fn, const int32_t *groups, size_t n_groups,
                               int on_device, double *params_inout, const size_t *n_models, size_t max_models,
                               size_t max_rounds, int32_t *labels_out, uint64_t *counts_out, uint64_t *offsets_out,
                               lsqr_fit_info *fits, int32_t *status_out, size_t *rounds_out, int32_t *converged_out) {
  AssignGrpJob J;
  J.groups = groups;
  J.n_groups = n_groups;
  J.on_device = on_device ? 1 : 0;
  J.params = params_inout;
  J.n_models = n_models;
  J.max_models = max_models;
  J.max_rounds = max_rounds;
  J.labels_out = labels_out;
  J.counts_out = counts_out;
  J.offsets_out = offsets_out;
  J.fits = fits;
  J.status_out = status_out;
  J.rounds_out = rounds_out;
  J.converged_out = converged_out;
  J.refine = true;
  return assign_grouped_call<G>(c, fn, fits && status_out && rounds_out && converged_out, J);
}

// lsqr_assign_grouped and lsqr_assign_dense_grouped
template <AssignGate G>
static int assign_only_grouped_call(lsqr_ctx *c, const char *fn, const int32_t *groups, size_t n_groups, int on_device,
                                    const double *params, const size_t *n_models, size_t max_models,
                                    int32_t *labels_out, double *residuals_out, uint64_t *counts_out,
                                    uint64_t *offsets_out) {
  AssignGrpJob J;
  J.groups = groups;
  J.n_groups = n_groups;
  J.on_device = on_device ? 1 : 0;
  J.params = const_cast<double *>(params);  // (read only: no refit runs)
  J.n_models = n_models;
  J.max_models = max_models;
  J.max_rounds = 0;
  J.labels_out = labels_out;
  J.residuals_out = residuals_out;
  J.counts_out = counts_out;
  J.offsets_out = offsets_out;
  J.refine = false;
  return assign_grouped_call<G>(c, fn, labels_out != nullptr, J);
}
}  // extern "C++"

int lsqr_assign_grouped(lsqr_ctx *c, const int32_t *groups, size_t n_groups, int on_device, const double *params,
                        const size_t *n_models, size_t max_models, int32_t *labels_out, double *residuals_out,
                        uint64_t *counts_out, uint64_t *offsets_out) {
  return assign_only_grouped_call<ASSIGN_GATE_ANY>(c, "lsqr_assign_grouped", groups, n_groups, on_device, params,
                                                   n_models, max_models, labels_out, residuals_out, counts_out,
                                                   offsets_out);
}

int lsqr_refine_grouped(lsqr_ctx *c, const int32_t *groups, size_t n_groups, int on_device, double *params_inout,
                        const size_t *n_models, size_t max_models, size_t max_rounds, int32_t *labels_out,
                        uint64_t *counts_out, uint64_t *offsets_out, lsqr_fit_info *fits, int32_t *status_out,
                        size_t *rounds_out, int32_t *converged_out) {
  return refine_grouped_call<ASSIGN_GATE_CLOSED>(c, "lsqr_refine_grouped", groups, n_groups, on_device, params_inout,
                                             n_models, max_models, max_rounds, labels_out, counts_out, offsets_out,
                                             fits, status_out, rounds_out, converged_out);
}

int lsqr_refine_lm_grouped(lsqr_ctx *c, const int32_t *groups, size_t n_groups, int on_device, double *params_inout,
                           const size_t *n_models, size_t max_models, size_t max_rounds, int32_t *labels_out,
                           uint64_t *counts_out, uint64_t *offsets_out, lsqr_fit_info *fits, int32_t *status_out,
                           size_t *rounds_out, int32_t *converged_out) {
  return refine_grouped_call<ASSIGN_GATE_LM>(c, "lsqr_refine_lm_grouped", groups, n_groups, on_device, params_inout,
                                             n_models, max_models, max_rounds, labels_out, counts_out, offsets_out,
                                             fits, status_out, rounds_out, converged_out);
}

int lsqr_assign_dense_grouped(lsqr_ctx *c, const int32_t *groups, size_t n_groups, int on_device, const double *params,
                              const size_t *n_models, size_t max_models, int32_t *labels_out, double *residuals_out,
                              uint64_t *counts_out, uint64_t *offsets_out) {
  return assign_only_grouped_call<ASSIGN_GATE_DENSE>(c, "lsqr_assign_dense_grouped", groups, n_groups, on_device,
                                                     params, n_models, max_models, labels_out, residuals_out,
                                                     counts_out, offsets_out);
}

int lsqr_refine_dense_grouped(lsqr_ctx *c, const int32_t *groups, size_t n_groups, int on_device, double *params_inout,
                              const size_t *n_models, size_t max_models, size_t max_rounds, int32_t *labels_out,
                              uint64_t *counts_out, uint64_t *offsets_out, lsqr_fit_info *fits, int32_t *status_out,
                              size_t *rounds_out, int32_t *converged_out) {
  return refine_grouped_call<ASSIGN_GATE_DENSE>(c, "lsqr_refine_dense_grouped", groups, n_groups, on_device,
                                                params_inout, n_models, max_models, max_rounds, labels_out, counts_out,
                                                offsets_out, fits, status_out, rounds_out, converged_out);
}

// C(n,k) and the rank-th k-subset in the exhaustive overload's order (comb.h); host only
int lsqr_comb_count(uint64_t n, int k, uint64_t *count_out) {
  if (!count_out || k < 1 || k > 64) return LSQR_ERR_INVALID;
  return comb_count(n, k, count_out) ? LSQR_OK : LSQR_ERR_INVALID;
}
int lsqr_comb_unrank(uint64_t n, int k, uint64_t rank, uint32_t *subset_out) {
  uint64_t count = 0;
  if (!subset_out || k < 1 || k > 64 || n > 0x100000000ull) return LSQR_ERR_INVALID;
  if (!comb_count(n, k, &count) || rank >= count) return LSQR_ERR_INVALID;
  comb_unrank(n, k, rank, subset_out);
  return LSQR_OK;
}

int lsqr_ransac_exhaustive(lsqr_ctx *c, double *params_out, uint8_t *consensus_out,
                           lsqr_ransac_info *info) {
  lsqr_ransac_info local;
  if (!info) info = &local;
  memset(info, 0, sizeof *info);
  int st = need_ready(c, false);
  if (st != LSQR_OK) return st;
  const int k = c->K;
  if (c->n < (size_t)k) return LSQR_EMPTY;  // RANSAC.hxx:165-169: cleared, returns 0
  if ((st = need_ready(c, true)) != LSQR_OK) return st;
  // all C(N,k) tuples in lexicographic order (RANSAC.hxx:197-213), in batches
  std::vector<uint32_t> comb((size_t)k), sub, votes;
  std::vector<uint8_t> valid;
  for (int l = 0; l < k; l++) comb[l] = (uint32_t)l;
  bool more = true, has = false;
  uint32_t best = 0;
  uint64_t index = 0, best_idx = 0;
  const size_t B = 4096;
  while (more) {
    sub.clear();
    size_t H = 0;
    while (more && H < B) {
      sub.insert(sub.end(), comb.begin(), comb.end());
      H++;
      int l = k - 1;
      while (l >= 0 && comb[l] == (uint32_t)(c->n - k + l)) l--;
      if (l < 0) more = false;
      else {
        comb[l]++;
        for (int j = l + 1; j < k; j++) comb[j] = comb[j - 1] + 1;
      }
    }
    if ((st = lsqr_hypotheses_from_subsets(c, sub.data(), H)) != LSQR_OK) return st;
    if ((st = lsqr_scan(c)) != LSQR_OK) return st;
    votes.resize(H);
    valid.resize(H);
    if ((st = lsqr_get_hypotheses(c, nullptr, valid.data(), votes.data())) != LSQR_OK) return st;
    long winner = -1;
    for (size_t e = 0; e < H; e++)
      if (valid[e] && votes[e] > best) {  // :245 strict
        best = votes[e];
        winner = (long)e;
        best_idx = index + e;
        has = true;
      }
    if (winner >= 0) {
      HIPCHK(c, hipMemcpyAsync(c->d_best, c->d_hparams + (size_t)winner * c->HS, sizeof(double) * c->HS,
                               hipMemcpyDeviceToDevice, c->stream));
      c->win_rec = sub[(size_t)winner * k];
    }
    index += H;
    info->evaluated += H;
  }
  info->iterations = index;
  info->best_index = best_idx;
  return finish_ransac(c, has, best, params_out, consensus_out, info);
}

// One fixed-size batch end to end, everything chained on the stream: sample -> solve -> scan ->
// first-max winner -> consensus mask -> final fit; the host synchronises once (LM fits: once per
// evaluation).
int lsqr_batch_fit(lsqr_ctx *c, uint64_t seed, uint64_t first, size_t H, double *params_out,
                   uint8_t *consensus_out, lsqr_ransac_info *info) {
  int st = lsqr_hypotheses_sample(c, seed, first, H, nullptr);
  if (st != LSQR_OK) return st;
  if ((st = run_scan_batch(c, 0)) != LSQR_OK) return st;
  c->scanned = true;
  if ((st = enqueue_take_best(c)) != LSQR_OK) return st;
  SolveOut out;
  if ((st = run_winner_finish(c, ORG_WINNER_DEV, consensus_out, &out)) != LSQR_OK) return st;
  const unsigned long long cnt = c->h_pin->mask_head[0], pk = c->h_pin->mask_head[1];
  fill_ransac_info(info, pk, first, H, cnt, c->n, out);
  return pk == 0 ? LSQR_EMPTY : deliver_params(out, params_out);
}

// Second half of a multi-GPU step on one rank, chained on the stream with one synchronisation: the
// winner is re-derived from its index in the (stateless) sampler stream, its consensus mask is taken
// over this rank's observation slice [begin, end) and the slice's phase-0 moment block is reduced about
// the model's own point (plane / line: a, sphere: c; zeros for the other models).
int lsqr_winner_moments(lsqr_ctx *c, uint64_t seed, uint64_t stream_index, size_t begin, size_t end,
                        double *params_out, double *origin_out, double *block_out,
                        uint64_t *count_out) {
  int st = lsqr_hypotheses_sample(c, seed, stream_index, 1, nullptr);
  if (st != LSQR_OK) return st;
  if (begin > end || end > c->n || !block_out) return fail(c, LSQR_ERR_INVALID, "bad range");
  int nmom = 0;
  if ((st = enqueue_winner_slice(c, begin, end, &nmom)) != LSQR_OK) return st;  // (its own origin rule)
  WinnerPin *pin = &c->h_pin->winner;
  HIPCHK(c, hipMemcpyAsync(&pin->valid, c->d_valid, 1, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&pin->count, c->d_counter + CNT_MASK, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                           c->stream));
  HIPCHK(c, hipMemcpyAsync(pin->params, c->d_hparams, sizeof(double) * c->P, hipMemcpyDeviceToHost,
                           c->stream));
  HIPCHK(c, hipMemcpyAsync(pin->origin, c->d_vec, sizeof(double) * 32, hipMemcpyDeviceToHost,
                           c->stream));
  HIPCHK(c, hipMemcpyAsync(block_out, c->d_mom, sizeof(double) * nmom, hipMemcpyDeviceToHost,
                           c->stream));
  HIPCHK(c, sync_stream(c));
  if (pin->valid == 0) return LSQR_EMPTY;  // degenerate subset: not a possible winner
  if (count_out) *count_out = pin->count;
  if (params_out) memcpy(params_out, pin->params, sizeof(double) * c->P);
  if (origin_out) memcpy(origin_out, pin->origin, sizeof(double) * 32);
  return LSQR_OK;
}

// ---- pipelined batches: enqueue now, read later ------------------------------------------------------------
// slot s of a context with L lanes: lane s % L, that lane's own slot s / L (0 or 1)
static int lane_count(const lsqr_ctx *c) {
  return c->is_lane ? 1 : std::max(1, std::min(c->opt.lanes, (int)lsqr_ctx::kMaxLanes));
}
// the lane context, created on first use and (re-)attached to the parent's model, options and records
static int lane_get(lsqr_ctx *c, int li, lsqr_ctx **out) {
  if (li == 0) {
    *out = c;
    return LSQR_OK;
  }
  lsqr_ctx *&l = c->lanes[li];
  if (!l) {
    int st = lsqr_ctx_create(c->device, &l);
    if (st != LSQR_OK) return fail(c, st, "cannot create lane %d", li);
    l->is_lane = true;
    if (l->counted) {  // lanes never run a persistent fit: they do not take a share of the device
      lmp_ctx_count(l->device, -1);
      l->counted = false;
    }
    l->prof = c->prof;
  }
  if (l->lane_epoch != c->data_epoch) {
    if (!c->has_model || !c->d_data) return fail(c, LSQR_ERR_STATE, "no model / records");
    HIPCHK(c, hipStreamSynchronize(l->stream));
    int st = lsqr_set_model(l, &c->cfg);
    l->opt = c->opt;  // (an option that drops the index needs no more here: lsqr_attach drops it)
    l->use_tiles = c->use_tiles;
    if (st == LSQR_OK) st = lsqr_attach(l, c->d_data, c->n, c->stride * sizeof(double));
    if (st != LSQR_OK) return fail(c, st, "lane %d: %s", li, lsqr_last_error(l));
    HIPCHK(c, sync_stream(c));  // an upload still in flight on the parent's stream
    l->lane_epoch = c->data_epoch;
  }
  *out = l;
  return LSQR_OK;
}

int lsqr_batch_fit_enqueue(lsqr_ctx *c, uint64_t seed, uint64_t first, size_t H, int slot) {
  if (!c) return LSQR_ERR_INVALID;
  if (!c->is_lane) {
    const int L = lane_count(c);
    if (slot < 0 || slot >= 2 * L) return fail(c, LSQR_ERR_INVALID, "slot %d of %d", slot, 2 * L);
    if (slot % L != 0 || slot / L != slot) {
      lsqr_ctx *l = nullptr;
      int st = lane_get(c, slot % L, &l);
      if (st != LSQR_OK) return st;
      if (l != c) {
        st = lsqr_batch_fit_enqueue(l, seed, first, H, slot / L);
        return st == LSQR_OK ? st : fail(c, st, "lane %d: %s", slot % L, lsqr_last_error(l));
      }
      slot = slot / L;
    }
  }
  if (slot < 0 || slot > 1) return LSQR_ERR_INVALID;
  BatchSlotState &s = c->slots[slot];
  if (s.busy) return fail(c, LSQR_ERR_STATE, "slot %d holds an unread result", slot);
  if (c->has_model && (wants_lm(c->cfg) || c->cfg.model == LSQR_MODEL_PHANTOM))
    return fail(c, LSQR_ERR_INVALID, "this model's fit needs the host between device passes");
  int st = lsqr_hypotheses_sample(c, seed, first, H, nullptr);
  if (st != LSQR_OK) return st;
  const uint64_t seq_before = c->bsel_seq;
  c->defer_ovf = true;  // no host synchronisation inside the scan: the worklist fill is checked by lsqr_batch_fit_wait
  c->ovf_cap = 0;
  st = run_scan_batch(c, 0);
  c->defer_ovf = false;
  if (st != LSQR_OK) return st;
  s.ovf_cap = c->ovf_cap;
  s.seed = seed;
  if (c->ovf_cap)  // {fullest worklist segment of this batch's scan} beside the slot's results
    HIPCHK(c, hipMemcpyAsync(&c->h_pin->batch[slot].ovf_fill, c->d_counter + CNT_OVF, sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, c->stream));
  s.bsel_rec = c->bsel_seq != seq_before ? c->bsel_last_rec : -1;  // this batch's selection record
  s.bsel_seq = c->bsel_seq;
  c->scanned = true;
  if ((st = enqueue_take_best(c)) != LSQR_OK) return st;
  BatchSlot *pin = &c->h_pin->batch[slot];
  bool fused = false;
  if ((st = enqueue_winner_finish(c, ORG_WINNER_DEV, pin->head, &fused)) != LSQR_OK) return st;
  if ((st = enqueue_fit(c, 1, fused, true)) != LSQR_OK) return st;
  HIPCHK(c, hipMemcpyAsync(&pin->out, c->d_out, sizeof(SolveOut), hipMemcpyDeviceToHost, c->stream));
  if (!s.ev) HIPCHK(c, s.ev.create(hipEventDisableTiming));
  HIPCHK(c, hipEventRecord(s.ev, c->stream));
  s.first = first;
  s.H = H;
  s.busy = true;
  return LSQR_OK;
}

int lsqr_batch_fit_wait(lsqr_ctx *c, int slot, double *params_out, lsqr_ransac_info *info) {
  if (!c) return LSQR_ERR_INVALID;
  if (!c->is_lane) {
    const int L = lane_count(c);
    if (slot < 0 || slot >= 2 * L) return fail(c, LSQR_ERR_INVALID, "slot %d of %d", slot, 2 * L);
    const int li = slot % L;
    slot = slot / L;
    if (li != 0) {
      lsqr_ctx *l = c->lanes[li];
      if (!l) return fail(c, LSQR_ERR_STATE, "slot has nothing in flight");
      int st = lsqr_batch_fit_wait(l, slot, params_out, info);
      return (st == LSQR_OK || st == LSQR_EMPTY) ? st : fail(c, st, "lane %d: %s", li, lsqr_last_error(l));
    }
  }
  if (slot < 0 || slot > 1) return LSQR_ERR_INVALID;
  BatchSlotState &s = c->slots[slot];
  if (!s.busy) return fail(c, LSQR_ERR_STATE, "slot %d has nothing in flight", slot);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventSynchronize(s.ev));
  s.busy = false;
  if (s.bsel_rec >= 0 && c->bsel[s.bsel_rec].seq == s.bsel_seq)
    bsel_fold(c, s.bsel_rec);  // the host has synchronised with this batch: its selection counts count
  s.bsel_rec = -1;
  const BatchSlot *pin = &c->h_pin->batch[slot];
  if (s.ovf_cap) {
    unsigned int fill = 0;
    memcpy(&fill, &pin->ovf_fill, sizeof fill);
    if (fill > s.ovf_cap || c->opt.test_overflow) {
      // a worklist segment of the matrix-core filter overflowed (never seen outside the tests): the batch again, blocking,
      // on the exact kernels
      (void)fail(c, LSQR_OK, "worklist segment overflow in slot %d (fill %u > %u): batch run again without the filter",
                 slot, fill, s.ovf_cap);
      c->ovf_reruns++;
      const int keep = c->opt.filter;
      c->opt.filter = 0;
      const int st2 = lsqr_batch_fit(c, s.seed, s.first, (size_t)s.H, params_out, nullptr, info);
      c->opt.filter = keep;
      return st2;
    }
  }
  const SolveOut out = pin->out;
  const unsigned long long cnt = pin->head[0], pk = pin->head[1];
  // unlike lsqr_batch_fit, fit.lm_info, lm_nfev and reserved stay 0 here (kept as it is: a behaviour change of its own)
  fill_ransac_info(info, pk, s.first, s.H, cnt, c->n, out, false);
  return pk == 0 ? LSQR_EMPTY : deliver_params(out, params_out);
}

// ---- multi-GPU step with device-resident exchange buffers (lsqr_hip.h) ----------------------------------
int lsqr_set_stream(lsqr_ctx *c, void *hip_stream, int external) {
  if (!c) return LSQR_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, sync_stream(c));  // nothing of ours may still be in flight on the old stream
  // profiling events recorded on the old stream stay valid (events are not bound to a stream)
  // external: the caller's stream as given -- NULL is the (legacy) default stream, which torch uses unless
  // told otherwise
  c->stream = external ? (hipStream_t)hip_stream : c->own_stream;
  c->external_stream = external != 0;
  return LSQR_OK;
}

int lsqr_step_scan(lsqr_ctx *c, uint64_t seed, uint64_t first, size_t H, uint32_t index_base,
                   uint64_t *packed_dev) {
  if (!packed_dev) return c ? fail(c, LSQR_ERR_INVALID, "null exchange buffer") : LSQR_ERR_INVALID;
  int st = lsqr_hypotheses_sample(c, seed, first, H, nullptr);
  if (st != LSQR_OK) return st;
  if ((st = run_scan_batch(c, 0)) != LSQR_OK) return st;
  c->scanned = true;
  hipLaunchKernelGGL(k_best, dim3(1), dim3(kBlock), 0, c->stream, c->d_votes, c->d_valid,
                     (uint32_t)c->H, (unsigned long long *)packed_dev, index_base);
  HIPCHK(c, hipGetLastError());
  return LSQR_OK;
}

int lsqr_step_winner(lsqr_ctx *c, uint64_t seed, uint64_t batch_first, const uint64_t *packed_dev,
                     size_t begin, size_t end, double *block_dev) {
  int st = need_ready(c, true);
  if (st != LSQR_OK) return st;
  if (!packed_dev || !block_dev || begin > end || end > c->n) return fail(c, LSQR_ERR_INVALID, "bad argument");
  if ((st = ensure_hyp(c, 1)) != LSQR_OK) return st;
  c->H = 1;
  c->scanned = false;
  {
    ProfScope ps(c, KID_SAMPLE);
    hipLaunchKernelGGL(k_winner_subset, dim3(1), dim3(64), 0, c->stream, seed, batch_first,
                       (const unsigned long long *)packed_dev, (uint64_t)c->n, c->K, c->d_subsets);
    HIPCHK(c, hipGetLastError());
  }
  if ((st = run_estimate(c)) != LSQR_OK) return st;
  int nmom = 0;
  if ((st = enqueue_winner_slice(c, begin, end, &nmom)) != LSQR_OK) return st;  // (its own origin rule)
  hipLaunchKernelGGL(k_pack_block, dim3(1), dim3(256), 0, c->stream, c->d_mom, nmom, c->d_counter + CNT_MASK,
                     block_dev);
  HIPCHK(c, hipGetLastError());
  return LSQR_OK;
}

int lsqr_step_finish_enqueue(lsqr_ctx *c, const uint64_t *packed_dev, const double *block_dev, int slot) {
  int st = need_ready(c, true);
  if (st != LSQR_OK) return st;
  if (!packed_dev || !block_dev || slot < 0 || slot > 1) return fail(c, LSQR_ERR_INVALID, "bad argument");
  StepSlotState &s = c->steps[slot];
  if (s.busy) return fail(c, LSQR_ERR_STATE, "step slot %d holds an unread result", slot);
  const int nmom = lsqr_moments_len(&c->cfg, 0);
  StepSlot *pin = &c->h_pin->step[slot];  // (results of a step are staged per slot)
  HIPCHK(c, hipMemcpyAsync(&pin->packed, packed_dev, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&pin->count, block_dev + nmom, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&pin->valid, c->d_valid, 1, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(pin->winner, c->d_hparams, sizeof(double) * c->P, hipMemcpyDeviceToHost, c->stream));
  if (c->cfg.model == LSQR_MODEL_PHANTOM) {  // solved on the host from the Gram block (in _wait)
    HIPCHK(c, hipMemcpyAsync(c->h_pin->phantom_block, block_dev, sizeof(double) * nmom, hipMemcpyDeviceToHost,
                             c->stream));
  } else {
    HIPCHK(c, hipMemcpyAsync(c->d_mom, block_dev, sizeof(double) * nmom, hipMemcpyDeviceToDevice,
                             c->stream));
    st = dispatch(c->cfg, [&](auto tag) -> int {
      typedef typename decltype(tag)::type M;
      return launch_solve<M>(c);
    });
    if (st != LSQR_OK) return st;
    HIPCHK(c, hipMemcpyAsync(&pin->out, c->d_out, sizeof(SolveOut), hipMemcpyDeviceToHost, c->stream));
  }
  if (!s.ev) HIPCHK(c, s.ev.create(hipEventDisableTiming));
  HIPCHK(c, hipEventRecord(s.ev, c->stream));
  s.bsel_rec = c->bsel_last_rec;   // the step's scan (lsqr_step_scan) came before on this stream
  s.bsel_seq = c->bsel_last_rec >= 0 ? c->bsel[c->bsel_last_rec].seq : 0;
  s.busy = true;
  return LSQR_OK;
}

int lsqr_step_finish_wait(lsqr_ctx *c, int slot, double *winner_out, double *params_out,
                          lsqr_ransac_info *info) {
  if (!c || slot < 0 || slot > 1) return LSQR_ERR_INVALID;
  StepSlotState &s = c->steps[slot];
  if (!s.busy) return fail(c, LSQR_ERR_STATE, "step slot %d has nothing in flight", slot);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventSynchronize(s.ev));  // the one synchronisation of the step
  s.busy = false;
  if (s.bsel_rec >= 0 && c->bsel[s.bsel_rec].seq == s.bsel_seq)
    bsel_fold(c, s.bsel_rec);
  s.bsel_rec = -1;
  const StepSlot *pin = &c->h_pin->step[slot];
  const unsigned long long pk = pin->packed;
  SolveOut out;
  memset(&out, 0, sizeof out);
  if (c->cfg.model == LSQR_MODEL_PHANTOM)
    phantom_solve_block(c->cfg, c->h_pin->phantom_block, &out);
  else
    out = pin->out;
  // (the count travels as a double behind the summed block: a whole number; evaluated = a winner exists)
  fill_ransac_info(info, pk, 0, pk != 0, (uint64_t)(pin->count + 0.5), c->n, out);
  if (info) info->iterations = 0;
  if (pk == 0 || !pin->valid) return LSQR_EMPTY;
  if (winner_out) memcpy(winner_out, pin->winner, sizeof(double) * c->P);
  return deliver_params(out, params_out);
}

int lsqr_step_finish(lsqr_ctx *c, const uint64_t *packed_dev, const double *block_dev,
                     double *winner_out, double *params_out, lsqr_ransac_info *info) {
  if (c && c->steps[0].busy) return fail(c, LSQR_ERR_STATE, "step slot 0 holds an unread result");
  int st = lsqr_step_finish_enqueue(c, packed_dev, block_dev, 0);
  if (st != LSQR_OK) return st;
  return lsqr_step_finish_wait(c, 0, winner_out, params_out, info);
}

// ---- several devices from ONE process (lsqr_hip.h: lsqr_multi_*) ------------------------------------------------
// The hypothesis stream is sharded over n contexts, one per listed device, exactly as bench.py's ranks shard it
// (lsqr_step_scan / _winner / _finish per context); the two exchanges of a step -- 8 B winner, <= 17 KB moment
// block -- are peer copies into rank 0's gather area (hipMemcpyPeerAsync: xGMI between GPUs of a node), a
// fixed-order reduction kernel there, and a peer copy of the winner back.  Streams are chained with events; the
// host synchronises once per step.  (Between PROCESSES the same exchanges are RCCL all-reduces: distributed.py.)
}  // extern "C"

namespace {
constexpr int kMultiBlk = 2304;  // >= dense_ne(64) + 1 + count, in doubles

__global__ void k_multi_max(const unsigned long long *__restrict__ g, int n, unsigned long long *__restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  unsigned long long b = 0;
  for (int r = 0; r < n; r++) b = g[r] > b ? g[r] : b;
  *out = b;
}
__global__ void k_multi_sum(const double *__restrict__ g, int n, int len, int pitch, double *__restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= len) return;
  double t = 0.0;
  for (int r = 0; r < n; r++) t += g[(size_t)r * pitch + k];  // rank order: deterministic
  out[k] = t;
}
}  // namespace

struct lsqr_multi {
  int n = 0;
  std::vector<lsqr_ctx *> ctx;
  std::vector<unsigned long long *> packed;  // per rank: the step's packed winner (device)
  std::vector<double *> block;               // per rank: moment block + count (device)
  unsigned long long *g_packed = nullptr;    // rank 0: gather areas
  double *g_block = nullptr;
  std::vector<hipEvent_t> ev;                // per rank: "my contribution has been sent"
  hipEvent_t ev_root = nullptr;              // rank 0: "the reduced value is on its way back"
  // LSQR_MULTI_TRANSPORT=rccl: the two exchanges as RCCL all-reduces over xGMI (one communicator per device,
  // ncclCommInitAll) instead of peer copies into rank 0 + a reduction kernel
  bool rccl = false;
  std::vector<ncclComm_t> comm;
  double rccl_bringup_s = 0.0;
  char err[512] = {0};
};

namespace {
int mfail(lsqr_multi *m, int st, const char *what, lsqr_ctx *c = nullptr) {
  if (m) snprintf(m->err, sizeof m->err, "%s%s%s", what, c ? ": " : "", c ? c->err : "");
  return st;
}
#define MHIP(m, call)                                                                                     \
  do {                                                                                                    \
    hipError_t e_ = (call);                                                                               \
    if (e_ != hipSuccess) {                                                                               \
      snprintf((m)->err, sizeof(m)->err, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
               __LINE__);                                                                                 \
      return LSQR_ERR_HIP;                                                                                \
    }                                                                                                     \
  } while (0)

// librccl, loaded on first use and only when asked for (a process that also imports PyTorch carries PyTorch's own copy
// of the library: RTLD_LOCAL keeps the two apart)
struct RcclApi {
  void *lib = nullptr;
  decltype(&ncclCommInitAll) CommInitAll = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclAllReduce) AllReduce = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  decltype(&ncclGetVersion) GetVersion = nullptr;
  bool ok = false;
};
RcclApi &rccl_api() {
  static RcclApi a;
  static std::once_flag once;
  std::call_once(once, [] {
    const char *names[] = {getenv("LSQR_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so"};
    for (const char *nm : names) {
      if (!nm || !*nm) continue;
      a.lib = dlopen(nm, RTLD_NOW | RTLD_LOCAL);
      if (a.lib) break;
    }
    if (!a.lib) return;
    a.CommInitAll = (decltype(a.CommInitAll))dlsym(a.lib, "ncclCommInitAll");
    a.CommDestroy = (decltype(a.CommDestroy))dlsym(a.lib, "ncclCommDestroy");
    a.AllReduce = (decltype(a.AllReduce))dlsym(a.lib, "ncclAllReduce");
    a.GroupStart = (decltype(a.GroupStart))dlsym(a.lib, "ncclGroupStart");
    a.GroupEnd = (decltype(a.GroupEnd))dlsym(a.lib, "ncclGroupEnd");
    a.GetErrorString = (decltype(a.GetErrorString))dlsym(a.lib, "ncclGetErrorString");
    a.GetVersion = (decltype(a.GetVersion))dlsym(a.lib, "ncclGetVersion");
    a.ok = a.CommInitAll && a.CommDestroy && a.AllReduce && a.GroupStart && a.GroupEnd && a.GetErrorString;
  });
  return a;
}
#define MNCCL(m, call)                                                                                       \
  do {                                                                                                       \
    ncclResult_t r_ = (call);                                                                                \
    if (r_ != ncclSuccess) {                                                                                 \
      snprintf((m)->err, sizeof(m)->err, "%s failed: %s (%s:%d)", #call, rccl_api().GetErrorString(r_), __FILE__, \
               __LINE__);                                                                                    \
      return LSQR_ERR_HIP;                                                                                   \
    }                                                                                                        \
  } while (0)

// RCCL transport: buf[r] (count elements on rank r's device) <- op over all ranks, in place, each on its own stream
int multi_allreduce(lsqr_multi *m, const std::vector<void *> &buf, size_t count, ncclDataType_t type, ncclRedOp_t op) {
  RcclApi &a = rccl_api();
  MNCCL(m, a.GroupStart());
  for (int r = 0; r < m->n; r++) {
    ncclResult_t e = a.AllReduce(buf[r], buf[r], count, type, op, m->comm[r], m->ctx[r]->stream);
    if (e != ncclSuccess) {
      (void)a.GroupEnd();
      snprintf(m->err, sizeof m->err, "ncclAllReduce failed on rank %d: %s", r, a.GetErrorString(e));
      return LSQR_ERR_HIP;
    }
  }
  MNCCL(m, a.GroupEnd());
  MHIP(m, hipSetDevice(m->ctx[0]->device));
  return LSQR_OK;
}

// every rank's `src[r]` (bytes) -> rank 0's gather area at r * pitch; rank 0's stream waits for all of them
int multi_gather(lsqr_multi *m, const std::vector<const void *> &src, void *gather, size_t bytes, size_t pitch) {
  lsqr_ctx *c0 = m->ctx[0];
  for (int r = 0; r < m->n; r++) {
    lsqr_ctx *c = m->ctx[r];
    MHIP(m, hipSetDevice(c->device));
    MHIP(m, hipMemcpyPeerAsync((char *)gather + (size_t)r * pitch, c0->device, src[r], c->device, bytes, c->stream));
    if (r) {
      MHIP(m, hipEventRecord(m->ev[r], c->stream));
      MHIP(m, hipSetDevice(c0->device));
      MHIP(m, hipStreamWaitEvent(c0->stream, m->ev[r], 0));
    }
  }
  MHIP(m, hipSetDevice(c0->device));
  return LSQR_OK;
}

// rank 0's `src` (bytes) -> every other rank's dst[r]; their streams wait for it
int multi_bcast(lsqr_multi *m, const void *src, const std::vector<void *> &dst, size_t bytes) {
  lsqr_ctx *c0 = m->ctx[0];
  MHIP(m, hipSetDevice(c0->device));
  for (int r = 1; r < m->n; r++)
    MHIP(m, hipMemcpyPeerAsync(dst[r], m->ctx[r]->device, src, c0->device, bytes, c0->stream));
  MHIP(m, hipEventRecord(m->ev_root, c0->stream));
  for (int r = 1; r < m->n; r++) {
    MHIP(m, hipSetDevice(m->ctx[r]->device));
    MHIP(m, hipStreamWaitEvent(m->ctx[r]->stream, m->ev_root, 0));
  }
  MHIP(m, hipSetDevice(c0->device));
  return LSQR_OK;
}

void slice_of(size_t n, int r, int w, size_t *lo, size_t *hi) {
  *lo = n * (size_t)r / (size_t)w;
  *hi = n * (size_t)(r + 1) / (size_t)w;
}

// winner known on every rank (packed[r] holds it, in-batch index relative to batch_first): masks of the slices,
// summed moment block, final fit on rank 0 (LM fits: one summed block per evaluation), consensus slices to host
int multi_finish(lsqr_multi *m, uint64_t seed, uint64_t batch_first, double *params_out, uint8_t *consensus_out,
                 lsqr_ransac_info *info) {
  const int n = m->n;
  lsqr_ctx *c0 = m->ctx[0];
  const int len = lsqr_moments_len(&c0->cfg, 0);
  if (len + 1 > kMultiBlk) return mfail(m, LSQR_ERR_INVALID, "moment block too large");
  std::vector<size_t> lo(n), hi(n);
  std::vector<const void *> src(n);
  int st;
  for (int r = 0; r < n; r++) {
    slice_of(c0->n, r, n, &lo[r], &hi[r]);
    if ((st = lsqr_step_winner(m->ctx[r], seed, batch_first, (const uint64_t *)m->packed[r], lo[r], hi[r],
                               m->block[r])) != LSQR_OK)
      return mfail(m, st, "lsqr_step_winner", m->ctx[r]);
    src[r] = m->block[r];
  }
  if (m->rccl) {  // one all-reduce SUM of [moment block, inlier count]: every rank ends up with the summed block
    std::vector<void *> buf(n);
    for (int r = 0; r < n; r++) buf[r] = m->block[r];
    if ((st = multi_allreduce(m, buf, (size_t)len + 1, ncclDouble, ncclSum)) != LSQR_OK) return st;
  } else {
  if ((st = multi_gather(m, src, m->g_block, sizeof(double) * (len + 1), sizeof(double) * kMultiBlk)) != LSQR_OK)
    return st;
  hipLaunchKernelGGL(k_multi_sum, dim3((len + 1 + 255) / 256), dim3(256), 0, c0->stream, m->g_block, n, len + 1,
                     kMultiBlk, m->block[0]);
  MHIP(m, hipGetLastError());
  }
  double winner[64], fit[64];
  lsqr_ransac_info local;
  if (!info) info = &local;
  st = lsqr_step_finish(c0, (const uint64_t *)m->packed[0], m->block[0], winner, fit, info);  // synchronises rank 0
  if (st != LSQR_OK && st != LSQR_EMPTY) return mfail(m, st, "lsqr_step_finish", c0);
  info->fraction = c0->n ? (double)info->fit.n_used / (double)c0->n : 0.0;
  if (info->evaluated == 0) return LSQR_EMPTY;  // no valid hypothesis
  if (consensus_out)
    for (int r = 0; r < n; r++) {
      lsqr_ctx *c = m->ctx[r];
      MHIP(m, hipSetDevice(c->device));
      if (hi[r] > lo[r])
        MHIP(m, hipMemcpyAsync(consensus_out + lo[r], c->d_mask + lo[r], hi[r] - lo[r], hipMemcpyDeviceToHost,
                               c->stream));
    }
  if (c0->cfg.model == LSQR_MODEL_DENSE && info->fit.reserved == 2 && c0->opt.dense_dd) {
    // the summed Gram block is ill-conditioned (a pivot below 1e-6 max|G|): its solution carries eps cond(A)^2, and a
    // one-device fit of the same rows would have taken the double-double route.  The records are replicated, so rank 0
    // masks the whole upload with the winner and fits from the rows -- the N-device fit IS the one-device fit then.
    MHIP(m, hipSetDevice(c0->device));
    uint64_t cnt = 0;
    int st2 = lsqr_mask(c0, winner, 0, c0->n, nullptr, &cnt);
    lsqr_fit_info fi;
    if (st2 == LSQR_OK) st2 = lsqr_ls_fit(c0, 1, fit, &fi);
    if (st2 != LSQR_OK && st2 != LSQR_EMPTY) return mfail(m, st2, "refit of an ill-conditioned dense system from the rows", c0);
    const uint64_t used = info->fit.n_used;
    info->fit = fi;
    info->fit.n_used = used;
    info->n_params = st2 == LSQR_OK ? fi.n_params : 0;
    st = st2;
  }
  if (st == LSQR_OK && wants_lm(c0->cfg) && c0->cfg.model != LSQR_MODEL_PHANTOM) {
    // Levenberg-Marquardt over the sharded consensus set: per evaluation every rank reduces its slice at the trial
    // point, the blocks are summed on rank 0, MINPACK's control flow runs there (lsqr_lm_begin / lsqr_lm_step)
    const int n1 = lsqr_moments_len(&c0->cfg, 1);
    double xt[64] = {0}, x0[64] = {0}, blk[LM_MOM_MAX + 8];
    for (int j = 0; j < info->n_params && j < 64; j++) x0[j] = fit[j];
    if ((st = lsqr_lm_begin(c0, x0, xt)) != LSQR_OK) return mfail(m, st, "lsqr_lm_begin", c0);
    for (;;) {
      for (int r = 0; r < n; r++) {
        if ((st = lsqr_moments_dev(m->ctx[r], 1, lo[r], hi[r], 1, xt, m->block[r])) != LSQR_OK)
          return mfail(m, st, "lsqr_moments_dev", m->ctx[r]);
        src[r] = m->block[r];
      }
      if (m->rccl) {  // one all-reduce SUM of the {sum f^2, J^T J, J^T f} block per evaluation
        std::vector<void *> buf(n);
        for (int r = 0; r < n; r++) buf[r] = m->block[r];
        if ((st = multi_allreduce(m, buf, (size_t)n1, ncclDouble, ncclSum)) != LSQR_OK) return st;
      } else {
      if ((st = multi_gather(m, src, m->g_block, sizeof(double) * n1, sizeof(double) * kMultiBlk)) != LSQR_OK)
        return st;
      hipLaunchKernelGGL(k_multi_sum, dim3((n1 + 255) / 256), dim3(256), 0, c0->stream, m->g_block, n, n1,
                         kMultiBlk, m->block[0]);
      MHIP(m, hipGetLastError());
      }
      MHIP(m, hipMemcpyAsync(c0->h_pin->scratch, m->block[0], sizeof(double) * n1, hipMemcpyDeviceToHost, c0->stream));
      for (int r = 0; r < n; r++) {  // every rank's x staging must be consumed before the next trial point
        MHIP(m, hipSetDevice(m->ctx[r]->device));
        MHIP(m, hipStreamSynchronize(m->ctx[r]->stream));
      }
      memcpy(blk, c0->h_pin->scratch, sizeof(double) * n1);
      int cont = 0;
      lsqr_fit_info fi;
      st = lsqr_lm_step(c0, blk, xt, &cont, fit, &fi);
      if (st != LSQR_OK && st != LSQR_EMPTY) return mfail(m, st, "lsqr_lm_step", c0);
      if (!cont) {
        const uint64_t used = info->fit.n_used;
        info->fit = fi;
        info->fit.n_used = used;
        info->n_params = fi.n_params;
        break;
      }
    }
  }
  for (int r = 0; r < n; r++) {
    MHIP(m, hipSetDevice(m->ctx[r]->device));
    MHIP(m, hipStreamSynchronize(m->ctx[r]->stream));
  }
  MHIP(m, hipSetDevice(c0->device));
  if (st != LSQR_OK) return st;
  if (params_out)
    for (int j = 0; j < info->n_params; j++) params_out[j] = fit[j];
  return LSQR_OK;
}
}  // namespace

extern "C" {

int lsqr_multi_create(const int *devices, int n, lsqr_multi **out) {
  if (!out || !devices || n < 1 || n > 64) return LSQR_ERR_INVALID;
  *out = nullptr;
  lsqr_multi *m = new lsqr_multi();
  m->n = n;
  int st = LSQR_OK;
  for (int r = 0; r < n && st == LSQR_OK; r++) {
    lsqr_ctx *c = nullptr;
    st = lsqr_ctx_create(devices[r], &c);
    if (st != LSQR_OK) break;
    m->ctx.push_back(c);
    unsigned long long *p = nullptr;
    double *b = nullptr;
    hipEvent_t e = nullptr;
    if (hipMalloc((void **)&p, 64) != hipSuccess || hipMalloc((void **)&b, sizeof(double) * kMultiBlk) != hipSuccess ||
        hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess)
      st = LSQR_ERR_HIP;
    m->packed.push_back(p);
    m->block.push_back(b);
    m->ev.push_back(e);
    for (int q = 0; q < r && st == LSQR_OK; q++)  // peer access both ways where the devices differ
      if (devices[q] != devices[r]) {
        int can = 0;
        (void)hipDeviceCanAccessPeer(&can, devices[r], devices[q]);
        if (can) {
          (void)hipSetDevice(devices[r]);
          (void)hipDeviceEnablePeerAccess(devices[q], 0);
          (void)hipSetDevice(devices[q]);
          (void)hipDeviceEnablePeerAccess(devices[r], 0);
          (void)hipGetLastError();  // "already enabled" is fine
        }
      }
  }
  if (st == LSQR_OK) {
    (void)hipSetDevice(devices[0]);
    if (hipMalloc((void **)&m->g_packed, sizeof(unsigned long long) * 64) != hipSuccess ||
        hipMalloc((void **)&m->g_block, sizeof(double) * kMultiBlk * n) != hipSuccess ||
        hipEventCreateWithFlags(&m->ev_root, hipEventDisableTiming) != hipSuccess)
      st = LSQR_ERR_HIP;
  }
  const char *tr = getenv("LSQR_MULTI_TRANSPORT");
  if (st == LSQR_OK && tr && !strcmp(tr, "rccl")) {
    // RCCL wants one communicator per DISTINCT device of the process; anything else keeps the peer copies
    bool distinct = true;
    for (int r = 0; r < n; r++)
      for (int q = 0; q < r; q++) distinct = distinct && devices[q] != devices[r];
    RcclApi &a = rccl_api();
    if (!a.ok || !distinct) {
      snprintf(m->err, sizeof m->err, "LSQR_MULTI_TRANSPORT=rccl: %s", !a.ok ? "librccl could not be loaded" : "the same device is listed twice");
      lsqr_multi_destroy(m);
      return LSQR_ERR_INVALID;
    }
    const auto t0 = std::chrono::steady_clock::now();
    m->comm.assign((size_t)n, nullptr);
    ncclResult_t e = a.CommInitAll(m->comm.data(), n, devices);
    if (e != ncclSuccess) {
      m->comm.clear();
      lsqr_multi_destroy(m);
      return LSQR_ERR_HIP;
    }
    m->rccl = true;
    // prove the communicators with one small all-reduce before anything is timed
    std::vector<void *> buf((size_t)n);
    for (int r = 0; r < n; r++) {
      buf[(size_t)r] = m->packed[(size_t)r];
      (void)hipSetDevice(devices[r]);
      (void)hipMemsetAsync(m->packed[(size_t)r], 0, 8, m->ctx[(size_t)r]->stream);
    }
    st = multi_allreduce(m, buf, 1, ncclUint64, ncclMax);
    for (int r = 0; r < n && st == LSQR_OK; r++) {
      (void)hipSetDevice(devices[r]);
      if (hipStreamSynchronize(m->ctx[(size_t)r]->stream) != hipSuccess) st = LSQR_ERR_HIP;
    }
    (void)hipSetDevice(devices[0]);
    m->rccl_bringup_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  if (st != LSQR_OK) {
    lsqr_multi_destroy(m);
    return st;
  }
  *out = m;
  return LSQR_OK;
}

const char *lsqr_multi_transport(const lsqr_multi *m, double *bringup_seconds) {
  if (bringup_seconds) *bringup_seconds = m ? m->rccl_bringup_s : 0.0;
  return !m ? "none" : m->rccl ? "rccl" : "peer-copy";
}

void lsqr_multi_destroy(lsqr_multi *m) {
  if (!m) return;
  for (ncclComm_t cm : m->comm)
    if (cm) (void)rccl_api().CommDestroy(cm);
  m->comm.clear();
  for (size_t r = 0; r < m->ctx.size(); r++) {
    (void)hipSetDevice(m->ctx[r]->device);
    (void)hipStreamSynchronize(m->ctx[r]->stream);
    if (r < m->packed.size() && m->packed[r]) (void)hipFree(m->packed[r]);
    if (r < m->block.size() && m->block[r]) (void)hipFree(m->block[r]);
    if (r < m->ev.size() && m->ev[r]) (void)hipEventDestroy(m->ev[r]);
  }
  if (!m->ctx.empty()) (void)hipSetDevice(m->ctx[0]->device);
  if (m->g_packed) (void)hipFree(m->g_packed);
  if (m->g_block) (void)hipFree(m->g_block);
  if (m->ev_root) (void)hipEventDestroy(m->ev_root);
  for (lsqr_ctx *c : m->ctx) lsqr_ctx_destroy(c);
  delete m;
}

int lsqr_multi_size(const lsqr_multi *m) { return m ? m->n : 0; }
lsqr_ctx *lsqr_multi_ctx(lsqr_multi *m, int rank) { return (m && rank >= 0 && rank < m->n) ? m->ctx[rank] : nullptr; }
const char *lsqr_multi_last_error(const lsqr_multi *m) { return m ? m->err : "null handle"; }

int lsqr_multi_set_model(lsqr_multi *m, const lsqr_model_cfg *cfg) {
  if (!m || !cfg) return LSQR_ERR_INVALID;
  for (lsqr_ctx *c : m->ctx) {
    int st = lsqr_set_model(c, cfg);
    if (st != LSQR_OK) return mfail(m, st, "lsqr_set_model", c);
  }
  return LSQR_OK;
}

int lsqr_multi_upload(lsqr_multi *m, const void *host, size_t count, size_t stride_bytes) {
  if (!m) return LSQR_ERR_INVALID;
  lsqr_ctx *c0 = m->ctx[0];
  int st = lsqr_upload(c0, host, count, stride_bytes);  // ONE host -> device transfer
  if (st != LSQR_OK) return mfail(m, st, "lsqr_upload", c0);
  for (int r = 1; r < m->n; r++) {  // replicas: device to device
    lsqr_ctx *c = m->ctx[r];
    if ((st = need_ready(c, false)) != LSQR_OK) return mfail(m, st, "context not ready", c);
    if ((st = set_data_common(c, count, stride_bytes)) != LSQR_OK) return mfail(m, st, "bad records", c);
    if ((st = ensure(c, c->d_data_owned, std::max<size_t>(count * c->stride, 1))) != LSQR_OK)
      return mfail(m, st, "replica allocation", c);
    if (count) MHIP(m, hipMemcpyPeerAsync(c->d_data_owned, c->device, c0->d_data, c0->device, count * stride_bytes,
                                           c->stream));
    c->d_data = c->d_data_owned;
  }
  for (int r = 1; r < m->n; r++) {
    MHIP(m, hipSetDevice(m->ctx[r]->device));
    MHIP(m, hipStreamSynchronize(m->ctx[r]->stream));
  }
  MHIP(m, hipSetDevice(c0->device));
  return LSQR_OK;
}

int lsqr_multi_batch_fit(lsqr_multi *m, uint64_t seed, uint64_t first, size_t H, double *params_out,
                         uint8_t *consensus_out, lsqr_ransac_info *info) {
  if (!m || H == 0 || H * (size_t)m->n > 0xFFFFFFF0ull) return LSQR_ERR_INVALID;
  const int n = m->n;
  lsqr_ctx *c0 = m->ctx[0];
  int st;
  std::vector<const void *> src(n);
  std::vector<void *> dst(n);
  for (int r = 0; r < n; r++) {
    if ((st = lsqr_step_scan(m->ctx[r], seed, first + (uint64_t)r * H, H, (uint32_t)((size_t)r * H),
                             (uint64_t *)m->packed[r])) != LSQR_OK)
      return mfail(m, st, "lsqr_step_scan", m->ctx[r]);
    src[r] = m->packed[r];
    dst[r] = m->packed[r];
  }
  if (m->rccl) {  // all-reduce MAX of the packed (votes << 32) | ~index: the earliest best hypothesis, on every rank
    if ((st = multi_allreduce(m, dst, 1, ncclUint64, ncclMax)) != LSQR_OK) return st;
  } else {
  if ((st = multi_gather(m, src, m->g_packed, 8, 8)) != LSQR_OK) return st;
  hipLaunchKernelGGL(k_multi_max, dim3(1), dim3(64), 0, c0->stream, m->g_packed, n, m->packed[0]);
  MHIP(m, hipGetLastError());
  if ((st = multi_bcast(m, m->packed[0], dst, 8)) != LSQR_OK) return st;
  }
  lsqr_ransac_info local;
  if (!info) info = &local;
  st = multi_finish(m, seed, first, params_out, consensus_out, info);
  info->iterations = H * (uint64_t)n;
  info->evaluated = info->evaluated ? H * (uint64_t)n : 0;
  if (info->best_votes) info->best_index += first;  // stream index of the winner
  return st;
}

// RANSAC<T,S>::compute() over several devices: every batch of the adaptive loop is sharded (rank r scans the r-th
// contiguous part), the replay runs on the host over the batch in stream order -- same winner, iteration count and
// consensus set as lsqr_ransac on one device.
int lsqr_multi_ransac(lsqr_multi *m, double p, uint64_t seed, double *params_out, uint8_t *consensus_out,
                      lsqr_ransac_info *info) {
  lsqr_ransac_info local;
  if (!info) info = &local;
  memset(info, 0, sizeof *info);
  if (!m) return LSQR_ERR_INVALID;
  const int n = m->n;
  lsqr_ctx *c0 = m->ctx[0];
  int st = need_ready(c0, false);
  if (st != LSQR_OK) return mfail(m, st, "context not ready", c0);
  const int k = c0->K;
  if (c0->n < (size_t)k || !(p < 1.0) || !(p > 0.0)) return LSQR_ERR_INVALID;  // RANSAC.hxx:16-19
  uint64_t rs[6];
  lsqr_replay_init(c0->n, k, p, rs);
  DedupSet dedup;
  uint64_t base = 0;
  size_t per = 256;  // hypotheses per device per batch
  std::vector<uint32_t> votes, subs;
  std::vector<uint8_t> valid;
  while (!rs[RS_DONE]) {
    uint64_t remaining = rs[RS_TRIES] - base;
    size_t total = (size_t)std::min<uint64_t>(remaining, (uint64_t)per * n);
    if (total == 0) break;
    votes.resize(total);
    valid.resize(total);
    subs.resize(total * k);
    std::vector<size_t> off(n + 1, 0);
    for (int r = 0; r < n; r++) off[r + 1] = std::min(total, off[r] + per);
    for (int r = 0; r < n; r++) {
      const size_t h = off[r + 1] - off[r];
      if (!h) continue;
      lsqr_ctx *c = m->ctx[r];
      c->hyp_expected = rs[RS_HAS] ? std::min<uint64_t>(remaining / n, 1u << 20) : 0;
      if ((st = lsqr_hypotheses_sample(c, seed, base + off[r], h, nullptr)) != LSQR_OK ||
          (st = lsqr_scan(c)) != LSQR_OK)
        return mfail(m, st, "batch scan", c);
    }
    for (int r = 0; r < n; r++) {
      const size_t h = off[r + 1] - off[r];
      if (!h) continue;
      lsqr_ctx *c = m->ctx[r];
      MHIP(m, hipSetDevice(c->device));
      MHIP(m, hipMemcpyAsync(subs.data() + off[r] * k, c->d_subsets, h * k * sizeof(uint32_t), hipMemcpyDeviceToHost,
                             c->stream));
      if ((st = lsqr_get_hypotheses(c, nullptr, valid.data() + off[r], votes.data() + off[r])) != LSQR_OK)
        return mfail(m, st, "lsqr_get_hypotheses", c);
    }
    size_t used = lsqr_replay(c0->n, k, p, subs.data(), valid.data(), votes.data(), total, base, &dedup, rs);
    info->evaluated += total;
    base += used;
    if (used < total) break;
    per = std::min<size_t>(per * 4, 4096);
    if (!rs[RS_HAS] && base >= (1ull << 22)) break;
    if (c0->opt.max_iter > 0 && base >= (uint64_t)c0->opt.max_iter) break;
  }
  info->iterations = rs[RS_I];
  info->best_index = rs[RS_BEST_IDX];
  info->best_votes = (uint32_t)rs[RS_BEST];
  info->fraction = (double)rs[RS_BEST] / (double)c0->n;
  if (!rs[RS_HAS] || rs[RS_BEST] == 0) return LSQR_EMPTY;  // RANSAC.hxx:129: nothing written
  // the winner, as a packed value relative to its own stream index, on every rank
  const unsigned long long pk = ((unsigned long long)rs[RS_BEST] << 32) | 0xFFFFFFFFull;
  for (int r = 0; r < n; r++) {
    lsqr_ctx *c = m->ctx[r];
    MHIP(m, hipSetDevice(c->device));
    MHIP(m, hipMemcpyAsync(m->packed[r], &pk, 8, hipMemcpyHostToDevice, c->stream));
    MHIP(m, hipStreamSynchronize(c->stream));  // pk lives on this stack frame
  }
  const uint64_t iters = info->iterations, eval = info->evaluated, bidx = info->best_index;
  const uint32_t bv = info->best_votes;
  st = multi_finish(m, seed, rs[RS_BEST_IDX], params_out, consensus_out, info);
  info->iterations = iters;
  info->evaluated = eval;
  info->best_index = bidx;
  info->best_votes = bv;
  if ((st == LSQR_OK || st == LSQR_EMPTY) && info->fit.n_used != bv)
    return mfail(m, LSQR_ERR_HIP, "consensus count of the slices differs from the winner's votes");
  return st;
}

// options.h holds the names, rules and defaults; what needs the context is here
static int apply_option(lsqr_ctx *c, const char *name, int value) {
  // "scan_tiles" is the context's own (lsqr_ctx::use_tiles): 0 or 1, keeps the index; tiles in place stay and are
  // read again when the option comes back to 1
  if (!strcmp(name, "scan_tiles")) {
    if (value < 0 || value > 1)
      return fail(c, LSQR_ERR_INVALID, "scan_tiles does not accept %d (0 or 1: the scans open a cell from the index's fp32 tiles)", value);
    c->use_tiles = value != 0;
    return LSQR_OK;
  }
  bool drops_index = false;
  char why[256];
  const int st = options_set(c->opt, name, value, &drops_index, why, sizeof why);
  if (st == kOptUnknown) return fail(c, LSQR_ERR_INVALID, "unknown option %s", name);
  if (st != LSQR_OK) return fail(c, st, "%s", why);
  if (drops_index) drop_index(c);
  return LSQR_OK;
}
int lsqr_set_option(lsqr_ctx *c, const char *name, int value) {
  if (!c || !name) return LSQR_ERR_INVALID;
  static_assert(lsqr_ctx::kMaxLanes == 4, "the range of batch_lanes' row");
  const bool lanes = !strcmp(name, "batch_lanes");  // the one option that is the parent's alone
  if (lanes && value >= 1 && value <= lsqr_ctx::kMaxLanes) {  // (a value out of range is the row's to refuse)
    bool busy = c->slots[0].busy || c->slots[1].busy;
    for (int i = 1; i < lsqr_ctx::kMaxLanes; i++)
      if (c->lanes[i]) busy = busy || c->lanes[i]->slots[0].busy || c->lanes[i]->slots[1].busy;
    if (busy) return fail(c, LSQR_ERR_STATE, "batches in flight");
  }
  const int st = apply_option(c, name, value);
  if (st != LSQR_OK || c->is_lane || lanes) return st;
  for (int i = 1; i < lsqr_ctx::kMaxLanes; i++)
    if (c->lanes[i]) (void)apply_option(c->lanes[i], name, value);
  return LSQR_OK;
}

int lsqr_scan_workload(lsqr_ctx *c, uint32_t *bound_out, uint64_t out[8]) {
  int st = need_ready(c, true);
  if (st != LSQR_OK) return st;
  if (!out) return fail(c, LSQR_ERR_INVALID, "null argument");
  if (c->H == 0) return fail(c, LSQR_ERR_STATE, "no hypotheses");
  if (!c->index_valid) return fail(c, LSQR_ERR_STATE, "this upload has no spatial index (scan_index)");
  uint32_t *d_nc = c->d_votes2 + kPilots;  // scratch: per-hypothesis surviving cells (the batch has been read)
  const bool bounded = c->last_bound[0] != 0 && c->last_bound[3] == c->H;
  uint32_t h_sel[2] = {0, 0};
  if (bounded) {  // the selection of the bounded scan that just ran is still on the device
    HIPCHK(c, hipMemcpyAsync(c->h_pin->scratch, c->d_bsel, sizeof(BoundSel), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, sync_stream(c));
    memcpy(h_sel, c->h_pin->scratch, sizeof h_sel);
  }
  st = dispatch(c->cfg, [&](auto tag) -> int {
    typedef typename decltype(tag)::type M;
    if constexpr (requires { typename CellOf<M>::type; }) {
      typedef typename CellOf<M>::type CM;
      return with_pp<CM>(c->cell_pts,
                         [&](auto pp) { return run_cells_bounds<CM, decltype(pp)::value>(c, c->d_ub, d_nc); });
    } else {
      return fail(c, LSQR_ERR_INVALID, "model has no two-level scan");
    }
  });
  if (st != LSQR_OK) return st;
  HIPCHK(c, hipMemsetAsync(c->d_counter + CNT_SUM, 0, sizeof(unsigned long long), c->stream));
  if (bounded) {
    hipLaunchKernelGGL(k_sum_selected, dim3(1), dim3(256), 0, c->stream, c->d_sel, &c->d_bsel->n_pilot, d_nc,
                       c->d_counter + CNT_SUM);
    hipLaunchKernelGGL(k_sum_selected, dim3(8), dim3(256), 0, c->stream, c->d_sel + kPilots, &c->d_bsel->n_rest, d_nc,
                       c->d_counter + CNT_SUM);
    HIPCHK(c, hipGetLastError());
  }
  unsigned long long *pin = c->h_pin->scratch_u64;
  HIPCHK(c, hipMemcpyAsync(pin, c->d_counter + CNT_PAIRS, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(pin + 1, c->d_counter + CNT_SUM, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  if (bound_out)
    HIPCHK(c, hipMemcpyAsync(bound_out, c->d_ub, c->H * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, sync_stream(c));
  out[0] = pin[0];
  out[1] = (uint64_t)c->n_cells * ((c->H + 63) / 64);
  out[2] = c->n_cells;
  out[3] = c->cell_pts;
  out[4] = bounded ? 1 : 0;
  out[5] = h_sel[0];
  out[6] = h_sel[1];
  out[7] = bounded ? pin[1] : pin[0];
  return LSQR_OK;
}

int lsqr_lm_persist_info(const lsqr_ctx *c, uint64_t out[8], uint64_t *trace, uint32_t trace_cap, uint32_t *trace_n) {
  if (!c || !out) return LSQR_ERR_INVALID;
  for (int i = 0; i < 8; i++) out[i] = c->lmp_last[i];
  uint32_t nt = 0;
  if (trace) {
    nt = std::min(trace_cap, c->lmp_trace_n);
    memcpy(trace, c->lmp_trace, sizeof(uint64_t) * 4 * nt);
  }
  if (trace_n) *trace_n = nt;
  return LSQR_OK;
}

int lsqr_scan_work(lsqr_ctx *c, uint64_t out[8]) {
  int st = need_ready(c, true);
  if (st != LSQR_OK) return st;
  if (!out) return fail(c, LSQR_ERR_INVALID, "null argument");
  if (c->H == 0 || !c->scanned) return fail(c, LSQR_ERR_STATE, "no scanned batch");
  unsigned long long *pin = c->h_pin->scratch_u64;
  if (c->amb_counted)
    HIPCHK(c, hipMemcpyAsync(pin, c->d_ambcnt, 2 * kAmbSlots * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, sync_stream(c));  // the state of the last early-exit scan has landed in h_ee
  const uint64_t all = (uint64_t)c->H * (uint64_t)c->n;
  memset(out, 0, 8 * sizeof(uint64_t));
  if (c->amb_counted)
    for (int k = 0; k < kAmbSlots; k++) out[6] += pin[2 * k], out[7] += pin[2 * k + 1];
  out[2] = all;
  if (c->ee_last && c->h_ee && c->ee_H == c->H && c->ee_n == c->n) {
    out[0] = 1;
    out[1] = c->h_ee->work;
    out[3] = c->h_ee->n_cand;
    out[4] = c->h_ee->n_drop_first;
    out[5] = c->h_ee->n_alive;
  } else {
    out[1] = all;
    bsel_host_synced(c);
    if (c->last_bound[0] && c->last_bound[3] == c->H && c->bsel_known_H == c->H)
      out[3] = c->bsel_known.n_cand;  // bounded plane scan with rank bounds: the hypotheses whose bounds were refined
  }
  return LSQR_OK;
}

int lsqr_scan_pairs_counted(lsqr_ctx *c, uint64_t out[4]) {
  int st = need_ready(c, true);
  if (st != LSQR_OK) return st;
  if (!out) return fail(c, LSQR_ERR_INVALID, "null argument");
  if (!c->scanned || !c->last_count.valid || !c->index_valid || c->n_cells == 0)
    return fail(c, LSQR_ERR_STATE, "no counted scan over this index");
  const auto &lc = c->last_count;
  unsigned long long *d_sum = c->d_counter + CNT_SUM;
  if (lc.packed)
    hipLaunchKernelGGL(k_pairs_in_table<true>, dim3(1), dim3(1024), 0, c->stream, (const uint8_t *)nullptr, 0u, 0u,
                       (const uint32_t *)nullptr, 0u, c->n_cells, (const uint32_t *)c->d_paircost.get(), d_sum);
  else
    hipLaunchKernelGGL(k_pairs_in_table<false>, dim3(1), dim3(1024), 0, c->stream, (const uint8_t *)c->d_paircnt.get(),
                       lc.gstride, lc.H, lc.h_dev, lc.h_off, c->n_cells, (const uint32_t *)nullptr, d_sum);
  HIPCHK(c, hipGetLastError());
  unsigned long long *pin = c->h_pin->scratch_u64;
  HIPCHK(c, hipMemcpyAsync(pin, d_sum, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, sync_stream(c));
  out[0] = pin[0];
  out[1] = lc.packed ? 1 : 0;
  out[2] = lc.slab ? 1 : 0;
  out[3] = (uint64_t)c->n_cells * lc.H;
  return LSQR_OK;
}

int lsqr_index_info(const lsqr_ctx *c, uint64_t out[4]) {
  if (!c || !out) return LSQR_ERR_INVALID;
  out[0] = c->index_valid ? 1 : 0;
  out[1] = c->n_sorted;
  out[2] = c->n_cells;
  out[3] = c->cell_pts;
  return LSQR_OK;
}

int lsqr_scan_tiles_check(lsqr_ctx *c, uint64_t out[4]) {
  int st = need_ready(c, true);
  if (st != LSQR_OK) return st;
  if (!out) return fail(c, LSQR_ERR_INVALID, "null argument");
  out[0] = c->index_valid ? c->tiles_pts : 0;
  out[1] = c->n_cells;
  out[2] = out[3] = 0;
  if (!out[0] || c->n_cells == 0) return LSQR_OK;
  unsigned long long *d_bad = c->d_counter + CNT_SUM;
  HIPCHK(c, hipMemsetAsync(d_bad, 0, sizeof(unsigned long long), c->stream));
  st = dispatch(c->cfg, [&](auto tag) -> int {
    typedef typename decltype(tag)::type M;
    if constexpr (requires { typename CellOf<M>::type; }) {
      typedef typename CellOf<M>::type CM;
      out[3] = (uint64_t)c->n_cells * tile_cell_floats<CM>((int)(c->tiles_pts / 128)) * sizeof(float);
      return with_pp<CM>(c->tiles_pts, [&](auto pp) -> int {
        hipLaunchKernelGGL((k_check_tiles<CM, decltype(pp)::value>), dim3((c->n_cells + 3) / 4), dim3(256), 0, c->stream,
                           c->d_sorted.get(), c->n_sorted, c->d_boxes.get(), c->n_cells, c->d_tiles.get(), d_bad);
        HIPCHK(c, hipGetLastError());
        return LSQR_OK;
      });
    } else {
      return fail(c, LSQR_ERR_INVALID, "model has no two-level scan");
    }
  });
  if (st != LSQR_OK) return st;
  unsigned long long *pin = c->h_pin->scratch_u64;
  HIPCHK(c, hipMemcpyAsync(pin, d_bad, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, sync_stream(c));
  out[2] = pin[0];
  return LSQR_OK;
}

// ---- measurement ------------------------------------------------------------------------------------------
// (the lanes of lsqr_batch_fit_enqueue are profiled with their context: launches and times add up)
int lsqr_profile_enable(lsqr_ctx *c, int on) {
  if (!c) return LSQR_ERR_INVALID;
  prof_flush(c);
  c->prof = on != 0;
  for (int i = 1; i < lsqr_ctx::kMaxLanes; i++)
    if (c->lanes[i]) lsqr_profile_enable(c->lanes[i], on);
  return LSQR_OK;
}
int lsqr_profile_get(lsqr_ctx *c, int id, uint64_t *launches, double *total_ms) {
  if (!c || id < 0 || id >= 8) return LSQR_ERR_INVALID;
  prof_flush(c);
  uint64_t n = c->launches[id];
  double ms = c->ms[id];
  for (int i = 1; i < lsqr_ctx::kMaxLanes; i++)
    if (c->lanes[i]) {
      uint64_t ln = 0;
      double lms = 0.0;
      lsqr_profile_get(c->lanes[i], id, &ln, &lms);
      n += ln;
      ms += lms;
    }
  if (launches) *launches = n;
  if (total_ms) *total_ms = ms;
  return LSQR_OK;
}
int lsqr_profile_reset(lsqr_ctx *c) {
  if (!c) return LSQR_ERR_INVALID;
  prof_flush(c);
  memset(c->launches, 0, sizeof c->launches);
  memset(c->ms, 0, sizeof c->ms);
  for (int i = 1; i < lsqr_ctx::kMaxLanes; i++)
    if (c->lanes[i]) lsqr_profile_reset(c->lanes[i]);
  return LSQR_OK;
}

}  // extern "C"
