// options.h -- the knobs of lsqr_set_option: one struct of values, one table of rows, one interpreter.
// Host only and free of HIP, so that every rule is tested on the CPU (tests/cpp/options_test.cpp).  A new knob is a
// member of Options with its default and a row of kOptions with its name, rule and one line of documentation; the
// table is the complete list of option names (tests/test_option_coverage.py reads it).
#pragma once
#include <climits>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "../../include/lsqr_hip.h"

namespace lsqr {

// The defaults live here and nowhere else; what a value means is in the member's row.  Every member is an int because
// lsqr_set_option's value is one: the users of max_iter and many_round widen before they compare with 64-bit counts.
struct Options {
  int index = 1, cell = 0, refine = 1, kd_levels = 7, kd_after = 16384, presorted = 0, slab_gate = 3;  // spatial index
  int cpt = 0, block = 0, hsplit = 0, ppl = 0, pairs = 0, pairs_waves = 0;                             // two-level scan
  int prepared = 1, lean = 1, pack = 1, recheck = 1, slab = 1, hyp_order = 1;                          // ... counted forms
  int bound = 1, bound_merge = 0, axis = 1;                                                            // bounded scan
  int filter = 1, dense_f32 = 2, us_h16 = 1, test_overflow = 0;               // matrix-core filters and their worklists
  int dense_fast = 1, us_fast = 1, phantom_fast = 1, dense_wave = 3;          // minimal solves
  int fuse_mask = 1, us_mask_mfma = 1, mom_chunk = 0, syrk_diag = 0, dense_dd = 1;  // mask, moments, direct fits
  int mask_ring = 4, mask_diag = 0, mask_band = 0;                                  // ... k_mask_syrk_dense
  int lm_host = 1, lm_mfma = 1, lm_fused = 1, lm_tiles = 1;                         // iterative (LM) fits
  int lm_persist = 1, lm_persist_wgs = 0, lm_persist_timeout_ms = 2000, lm_persist_resident = 0, lm_persist_test_abort = 0;
  int max_iter = 0, many_round = 0, many_ex_fused = 1;  // RANSAC drivers
  int lanes = 4;                                        // (ignored on a lane)
  int upload_threads = -1;
};

enum OptRule : unsigned char {
  OPT_FLAG,     // stores value != 0
  OPT_ANY,      // stores the value
  OPT_RANGE,    // lo <= value <= hi, or invalid (hi == INT_MAX: open end)
  OPT_ONE_OF,   // one of set[], or invalid (every set holds 0, which also fills the unused places)
  OPT_CLAMP,    // stores the value clamped to lo .. hi
  OPT_FILTER,   // scan_filter alone: below 0 stores 0, above 3 stores 1 (not 3)
  OPT_REMOVED,  // 0 is accepted and stores nothing, anything else is invalid
};
struct OptionRow {
  const char *name;
  int Options::*member;  // nullptr: OPT_REMOVED
  OptRule rule;
  int lo, hi;
  bool drops_index;  // a successful set invalidates the spatial index, also when the value does not change
  const char *doc;
  int set[5] = {0, 0, 0, 0, 0};
};
constexpr bool kKeepsIndex = false, kDropsIndex = true;

// One row per option.  batch_lanes is a row like the others; that no batch may be in flight while it changes, and
// that it is not handed on to the lanes, is the caller's part (lsqr_set_option).
inline constexpr OptionRow kOptions[] = {
    // ---- spatial index of the point models (cells.h, axis.h) ----
    {"scan_index", &Options::index, OPT_RANGE, 0, 2, kKeepsIndex, "0 off, 1 auto, 2 always"},
    {"scan_cell", &Options::cell, OPT_ONE_OF, 0, 0, kKeepsIndex, "observations per cell: 256, 512 or 0 (default)", {0, 256, 512}},
    {"scan_refine", &Options::refine, OPT_FLAG, 0, 1, kDropsIndex, "index build: k-d refinement of the Morton order inside runs of 8192 records; 0: plain Morton runs (A/B)"},
    {"scan_kd_levels", &Options::kd_levels, OPT_RANGE, 0, 12, kDropsIndex, "0..12 k-d levels above the runs by segmented sorts (runs of 8192 << levels; 0: Morton order above them)"},
    {"scan_kd_after", &Options::kd_after, OPT_RANGE, 0, INT_MAX, kKeepsIndex, ">= 0: hypotheses an upload is scanned by before those levels are built (its first index keeps the cheaper order)"},
    {"scan_presorted", &Options::presorted, OPT_FLAG, 0, 1, kDropsIndex, "index build: cells are runs of the UPLOAD order (experiments with other spatial orders)"},
    {"scan_slab_gate", &Options::slab_gate, OPT_RANGE, 1, 8, kDropsIndex, "1..8: kappa of the slabs' gate in quarters (axis.h: k_cell_slabs; A/B)"},
    // ---- two-level scan and its counted forms (cells.h) ----
    {"scan_cpt", &Options::cpt, OPT_RANGE, 0, 1, kKeepsIndex, "0 or 1: cells per wave tile"},
    {"scan_block", &Options::block, OPT_ONE_OF, 0, 0, kKeepsIndex, "workgroup size: 256, 257 (256 + LDS broadcast) or 0 (default)", {0, 256, 257}},
    {"scan_hsplit", &Options::hsplit, OPT_RANGE, 0, 128, kKeepsIndex, "0..128 hypothesis segments per tile (0: auto)"},
    {"scan_ppl", &Options::ppl, OPT_ONE_OF, 0, 0, kKeepsIndex, "observations per lane of the filtered scans: 2, 4, 8, 16 or 0 (the measured best)", {0, 2, 4, 8, 16}},
    {"scan_pairs", &Options::pairs, OPT_ANY, 0, 0, kKeepsIndex, "plain scans of an indexed upload: 0 the model's measured choice, 1 always k_scan_pairs, 2 always k_scan_cells"},
    {"scan_pairs_waves", &Options::pairs_waves, OPT_ANY, 0, 0, kKeepsIndex, "workgroups per CU of k_scan_pairs (0: what fits)"},
    {"scan_pairs_mfma", nullptr, OPT_REMOVED, 0, 0, kKeepsIndex, "removed, only 0 is accepted: level 2 of the plane on the fp16 matrix cores, measured 25 % slower (tools/attic/cells_h16.h)"},
    {"scan_prepared", &Options::prepared, OPT_FLAG, 0, 1, kKeepsIndex, "cell models with PREPARED read Hyp from d_hyps; 0: load() per (cell, group) (A/B)"},
    {"scan_lean", &Options::lean, OPT_FLAG, 0, 1, kKeepsIndex, "count-only counting pass, PairsForm::Lean for prepared models; 0: the general forms (A/B)"},
    {"scan_pack", &Options::pack, OPT_RANGE, 0, 1, kKeepsIndex, "0 or 1: level 1 of the lean k_scan_pairs on packed blocks of 64 survivors; 0: per group (A/B)"},
    {"scan_recheck", &Options::recheck, OPT_RANGE, 0, 1, kKeepsIndex, "0 or 1: the packed k_scan_pairs re-checks the band's observations alone; 0: the whole cell"},
    {"scan_slab", &Options::slab, OPT_RANGE, 0, 1, kKeepsIndex, "0 or 1: the mask-storing counting pass of the 3-D plane tests the cell's slab too (PlaneCell::slab)"},
    {"scan_hyp_order", &Options::hyp_order, OPT_FLAG, 0, 1, kKeepsIndex, "a full count of the plane walks the batch in key order (k_plane_order: similar planes share a group)"},
    // ---- bounded scan ----
    {"scan_bound", &Options::bound, OPT_FLAG, 0, 1, kKeepsIndex, "batch entry points skip hypotheses that cannot win (exact winner); 0: count all"},
    {"scan_bound_merge", &Options::bound_merge, OPT_ONE_OF, 0, 0, kKeepsIndex, "cells per box of the bounds pass: 1 (the cells themselves), 2, 4, 8 or 0 (default)", {0, 1, 2, 4, 8}},
    {"scan_axis", &Options::axis, OPT_FLAG, 0, 1, kKeepsIndex, "the bounded scan of the 3-D plane takes its vote bounds by rank over axis-sorted cells (k_bound_axis)"},
    // ---- matrix-core filters of the scans ----
    {"scan_filter", &Options::filter, OPT_FILTER, 0, 3, kKeepsIndex, "filter in front of the exact predicate: 0 off, 1 on, 2 / 3 force the pair / tile re-check"},
    {"dense_f32", &Options::dense_f32, OPT_CLAMP, 0, 2, kKeepsIndex, "dense scan filter at n = 64: 2 fp16 matrix cores on two-way splits (dense_h16.h), 1 fp32 matrix cores, 0 fp64"},
    {"us_mfma", &Options::us_h16, OPT_FLAG, 0, 1, kKeepsIndex, "US calibrations: agree() scan on the fp16 matrix cores (us_h16.h); 0: packed fp32 filter"},
    {"scan_test_overflow", &Options::test_overflow, OPT_FLAG, 0, 1, kKeepsIndex, "tests: worklist_check and lsqr_batch_fit_wait treat the worklist as overflowed"},
    // ---- minimal solves ----
    {"dense_fast_solve", &Options::dense_fast, OPT_FLAG, 0, 1, kKeepsIndex, "elimination first, SVD when near the rank decision; 0: always the SVD pseudo-inverse"},
    {"us_fast_solve", &Options::us_fast, OPT_FLAG, 0, 1, kKeepsIndex, "US calibrations' minimal solves likewise (k_estimate_us)"},
    {"phantom_fast_solve", &Options::phantom_fast, OPT_CLAMP, 0, INT_MAX, kKeepsIndex, "plane phantom: LU + inverse iteration (> 1: its iteration limit), Jacobi SVD for the rest; 0: Jacobi only"},
    {"dense_wave_solve", &Options::dense_wave, OPT_ANY, 0, 0, kKeepsIndex, "3: one wave per system in registers (n = 64; else as 1), 1 / 2: in LDS, four / two per workgroup, 0: one workgroup per system"},
    // ---- mask, moments and the direct fits ----
    {"fuse_mask", &Options::fuse_mask, OPT_FLAG, 0, 1, kKeepsIndex, "winner's mask + moment block in one pass; 0: two kernels (A/B)"},
    {"us_mask_mfma", &Options::us_mask_mfma, OPT_FLAG, 0, 1, kKeepsIndex, "US calibrations: mask + analytic moment block on the fp64 matrix cores; 0: per-lane accumulators (A/B)"},
    {"mom_chunk", &Options::mom_chunk, OPT_ANY, 0, 0, kKeepsIndex, "chunk of the mask / moment passes in units of kBlock records (0: default; A/B)"},
    {"syrk_diag", &Options::syrk_diag, OPT_ANY, 0, 0, kKeepsIndex, "timing diagnostics of the dense SYRK (wrong sums): 1 loads only, 2 MFMAs only"},
    {"dense_dd", &Options::dense_dd, OPT_FLAG, 0, 1, kKeepsIndex, "dense fit: systems the elimination refuses are solved again from the rows in double-double; 0: stay on the Gram block"},
    {"dense_mask_ring", &Options::mask_ring, OPT_ANY, 0, 0, kKeepsIndex, "k_mask_syrk_dense: tile buffers per wave (2: two workgroups per CU; 4: one, three tiles in flight)"},
    {"dense_mask_diag", &Options::mask_diag, OPT_ANY, 0, 0, kKeepsIndex, "timing diagnostics of k_mask_syrk_dense (wrong results): 1 no matrix instructions, 2 no row evaluation"},
    {"dense_mask_band", &Options::mask_band, OPT_ANY, 0, 0, kKeepsIndex, "tests: scale factor of the dense fused mask's band (forces its serial re-evaluation path)"},
    // ---- iterative (LM) fits ----
    {"lm_host", &Options::lm_host, OPT_FLAG, 0, 1, kKeepsIndex, "MINPACK's step on the host between device passes (lsqr_ctx::h_lm); 0: on the device"},
    {"lm_mfma", &Options::lm_mfma, OPT_FLAG, 0, 1, kKeepsIndex, "the LM pass accumulates (J | f)^T (J | f) on the matrix cores; 0: per-lane sums + shuffle trees"},
    {"lm_fused", &Options::lm_fused, OPT_FLAG, 0, 1, kKeepsIndex, "one launch per LM evaluation, result polled in pinned memory; 0: the r01 path"},
    {"lm_tiles", &Options::lm_tiles, OPT_FLAG, 0, 1, kKeepsIndex, "matrix-core LM pass: compacted consensus set in field-major tiles, next tile in flight; 0: record-major (A/B)"},
    {"lm_persist", &Options::lm_persist, OPT_RANGE, 0, 3, kKeepsIndex, "0..3: 0 two launches per evaluation; 1 one persistent launch per fit if alone on the device, 3 always; 2 step on the device"},
    {"lm_persist_wgs", &Options::lm_persist_wgs, OPT_RANGE, 0, 1024, kKeepsIndex, "0..1024 resident workgroups of the persistent fit (0: 256 / 128 / 64 by the contexts on the device)"},
    {"lm_persist_timeout_ms", &Options::lm_persist_timeout_ms, OPT_RANGE, 1, 60000, kKeepsIndex, "1..60000: bound of every wait inside the persistent kernel"},
    {"lm_persist_resident", &Options::lm_persist_resident, OPT_FLAG, 0, 1, kKeepsIndex, "a fit alone on the device keeps its tiles in registers (k_lm_persist<M, 4>): no faster"},
    {"lm_persist_test_abort", &Options::lm_persist_test_abort, OPT_CLAMP, 0, INT_MAX, kKeepsIndex, "tests: workgroup 0 gives up at this evaluation (the fallback path)"},
    // ---- RANSAC drivers, lanes, upload ----
    {"max_iterations", &Options::max_iter, OPT_ANY, 0, 0, kKeepsIndex, "budget of lsqr_ransac (<= 0: the reference's bound, numTries <= C(N, k))"},
    {"many_round_hypotheses", &Options::many_round, OPT_RANGE, 0, INT_MAX, kKeepsIndex, ">= 0: lsqr_ransac_many's hypotheses per round (0: kManyRoundDefault)"},
    {"many_exhaustive_fused", &Options::many_ex_fused, OPT_FLAG, 0, 1, kKeepsIndex, "lsqr_ransac_many_exhaustive: small problems take one fused launch (k_many_ex_small)"},
    {"batch_lanes", &Options::lanes, OPT_RANGE, 1, 4, kKeepsIndex, "1..4 streams the pipelined batch entry points spread their slots over"},
    {"upload_threads", &Options::upload_threads, OPT_ANY, 0, 0, kKeepsIndex, "host threads of the staged upload (0: one plain hipMemcpy, -1: LSQR_UPLOAD_THREADS or 0)"},
};

constexpr int kOptUnknown = -1;  // options_set: no row has this name (every other return value is an lsqr_status)

// The whole interpreter: look the row up, apply its rule, store.  LSQR_OK: stored, and *drops_index says whether the
// caller has to invalidate its index; LSQR_ERR_INVALID: the rule refuses the value, nothing is stored and `why` says
// so with the row's documentation; kOptUnknown: no such option, nothing written.
inline int options_set(Options &o, const char *name, int value, bool *drops_index, char *why, size_t why_len) {
  *drops_index = false;
  const OptionRow *r = nullptr;
  for (const OptionRow &row : kOptions)
    if (!strcmp(name, row.name)) r = &row;
  if (!r) return kOptUnknown;
  bool ok = true;
  int v = value;
  switch (r->rule) {
    case OPT_FLAG: v = value != 0; break;
    case OPT_ANY: break;
    case OPT_RANGE: ok = value >= r->lo && value <= r->hi; break;
    case OPT_ONE_OF:
      ok = false;
      for (int s : r->set) ok = ok || value == s;
      break;
    case OPT_CLAMP: v = value < r->lo ? r->lo : value > r->hi ? r->hi : value; break;
    case OPT_FILTER: v = value < 0 ? 0 : value > 3 ? 1 : value; break;
    case OPT_REMOVED: ok = value == 0; break;
  }
  if (!ok) {
    snprintf(why, why_len, "%s does not accept %d (%s)", r->name, value, r->doc);
    return LSQR_ERR_INVALID;
  }
  if (r->member) o.*(r->member) = v;
  *drops_index = r->drops_index;
  return LSQR_OK;
}

}  // namespace lsqr
