// The rules of csrc/options.h, on the CPU.  What every option of lsqr_set_option accepts, stores and defaults to is
// written out below from the rule table of the change that introduced options.h (itself read off the hand-written
// branches it replaced) and checked through options_set alone.  Built with the address and undefined-behaviour
// sanitizers by tests/test_options.py.
#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

#include "options.h"

using lsqr::Options;

namespace {

int failures = 0;
#define CHECK(cond, ...)                                     \
  do {                                                       \
    if (!(cond)) {                                           \
      failures++;                                            \
      printf("%s:%d: CHECK(%s) failed: ", __FILE__, __LINE__, #cond); \
      printf(__VA_ARGS__);                                   \
      printf("\n");                                          \
    }                                                        \
  } while (0)

enum Kind { FLAG, ANY, RANGE, ONE_OF, CLAMP, FILTER, REMOVED };
struct Expect {
  const char *name;
  int Options::*member;  // nullptr: stores nothing
  int def;               // default of the member
  Kind kind;
  int lo, hi;            // RANGE, CLAMP
  std::vector<int> set;  // ONE_OF
  bool drops;
};
const int OPEN = INT_MAX;

const std::vector<Expect> kExpect = {
    // flag
    {"many_exhaustive_fused", &Options::many_ex_fused, 1, FLAG, 0, 0, {}, false},
    {"scan_bound", &Options::bound, 1, FLAG, 0, 0, {}, false},
    {"lm_mfma", &Options::lm_mfma, 1, FLAG, 0, 0, {}, false},
    {"lm_fused", &Options::lm_fused, 1, FLAG, 0, 0, {}, false},
    {"lm_host", &Options::lm_host, 1, FLAG, 0, 0, {}, false},
    {"scan_prepared", &Options::prepared, 1, FLAG, 0, 0, {}, false},
    {"scan_lean", &Options::lean, 1, FLAG, 0, 0, {}, false},
    {"scan_axis", &Options::axis, 1, FLAG, 0, 0, {}, false},
    {"scan_hyp_order", &Options::hyp_order, 1, FLAG, 0, 0, {}, false},
    {"us_mfma", &Options::us_h16, 1, FLAG, 0, 0, {}, false},
    {"fuse_mask", &Options::fuse_mask, 1, FLAG, 0, 0, {}, false},
    {"us_fast_solve", &Options::us_fast, 1, FLAG, 0, 0, {}, false},
    {"dense_fast_solve", &Options::dense_fast, 1, FLAG, 0, 0, {}, false},
    {"scan_test_overflow", &Options::test_overflow, 0, FLAG, 0, 0, {}, false},
    {"lm_persist_resident", &Options::lm_persist_resident, 0, FLAG, 0, 0, {}, false},
    {"lm_tiles", &Options::lm_tiles, 1, FLAG, 0, 0, {}, false},
    {"us_mask_mfma", &Options::us_mask_mfma, 1, FLAG, 0, 0, {}, false},
    {"dense_dd", &Options::dense_dd, 1, FLAG, 0, 0, {}, false},
    {"scan_refine", &Options::refine, 1, FLAG, 0, 0, {}, true},
    {"scan_presorted", &Options::presorted, 0, FLAG, 0, 0, {}, true},
    // any
    {"upload_threads", &Options::upload_threads, -1, ANY, 0, 0, {}, false},
    {"max_iterations", &Options::max_iter, 0, ANY, 0, 0, {}, false},
    {"syrk_diag", &Options::syrk_diag, 0, ANY, 0, 0, {}, false},
    {"scan_pairs", &Options::pairs, 0, ANY, 0, 0, {}, false},
    {"mom_chunk", &Options::mom_chunk, 0, ANY, 0, 0, {}, false},
    {"scan_pairs_waves", &Options::pairs_waves, 0, ANY, 0, 0, {}, false},
    {"dense_mask_ring", &Options::mask_ring, 4, ANY, 0, 0, {}, false},
    {"dense_mask_diag", &Options::mask_diag, 0, ANY, 0, 0, {}, false},
    {"dense_mask_band", &Options::mask_band, 0, ANY, 0, 0, {}, false},
    {"dense_wave_solve", &Options::dense_wave, 3, ANY, 0, 0, {}, false},
    // range
    {"scan_index", &Options::index, 1, RANGE, 0, 2, {}, false},
    {"scan_cpt", &Options::cpt, 0, RANGE, 0, 1, {}, false},
    {"scan_pack", &Options::pack, 1, RANGE, 0, 1, {}, false},
    {"scan_recheck", &Options::recheck, 1, RANGE, 0, 1, {}, false},
    {"scan_slab", &Options::slab, 1, RANGE, 0, 1, {}, false},
    {"scan_slab_gate", &Options::slab_gate, 3, RANGE, 1, 8, {}, true},
    {"scan_hsplit", &Options::hsplit, 0, RANGE, 0, 128, {}, false},
    {"scan_kd_levels", &Options::kd_levels, 7, RANGE, 0, 12, {}, true},
    {"lm_persist", &Options::lm_persist, 1, RANGE, 0, 3, {}, false},
    {"lm_persist_wgs", &Options::lm_persist_wgs, 0, RANGE, 0, 1024, {}, false},
    {"lm_persist_timeout_ms", &Options::lm_persist_timeout_ms, 2000, RANGE, 1, 60000, {}, false},
    {"many_round_hypotheses", &Options::many_round, 0, RANGE, 0, OPEN, {}, false},
    {"scan_kd_after", &Options::kd_after, 16384, RANGE, 0, OPEN, {}, false},
    {"batch_lanes", &Options::lanes, 4, RANGE, 1, 4, {}, false},
    // one-of
    {"scan_ppl", &Options::ppl, 0, ONE_OF, 0, 0, {0, 2, 4, 8, 16}, false},
    {"scan_bound_merge", &Options::bound_merge, 0, ONE_OF, 0, 0, {0, 1, 2, 4, 8}, false},
    {"scan_block", &Options::block, 0, ONE_OF, 0, 0, {0, 256, 257}, false},
    {"scan_cell", &Options::cell, 0, ONE_OF, 0, 0, {0, 256, 512}, false},
    // clamp
    {"dense_f32", &Options::dense_f32, 2, CLAMP, 0, 2, {}, false},
    {"phantom_fast_solve", &Options::phantom_fast, 1, CLAMP, 0, OPEN, {}, false},
    {"lm_persist_test_abort", &Options::lm_persist_test_abort, 0, CLAMP, 0, OPEN, {}, false},
    {"scan_filter", &Options::filter, 1, FILTER, 0, 0, {}, false},  // below 0 -> 0, above 3 -> 1
    // removed
    {"scan_pairs_mfma", nullptr, 0, REMOVED, 0, 0, {}, false},
};

const int kValues[] = {INT_MIN, -2, -1, 0, 1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 128, 129, 256, 257, 512, 1024, 1025, 60000, 60001, INT_MAX};

// what the rule of e does with v: accepted or not, and the value stored
bool model(const Expect &e, int v, int *stored) {
  *stored = v;
  switch (e.kind) {
    case FLAG: *stored = v != 0 ? 1 : 0; return true;
    case ANY: return true;
    case RANGE: return v >= e.lo && v <= e.hi;
    case ONE_OF:
      for (int s : e.set)
        if (s == v) return true;
      return false;
    case CLAMP: *stored = v < e.lo ? e.lo : v > e.hi ? e.hi : v; return true;
    case FILTER: *stored = v < 0 ? 0 : v > 3 ? 1 : v; return true;
    case REMOVED: return v == 0;
  }
  return false;
}

bool same(const Options &a, const Options &b) {
  for (const Expect &e : kExpect)
    if (e.member && a.*(e.member) != b.*(e.member)) return false;
  return true;
}

void test_table_shape() {
  const size_t rows = sizeof lsqr::kOptions / sizeof lsqr::kOptions[0];
  CHECK(rows == kExpect.size(), "%zu rows, %zu expectations", rows, kExpect.size());
  CHECK(rows == 53, "%zu rows", rows);
  size_t members = 0;
  for (size_t i = 0; i < rows; i++) {
    const lsqr::OptionRow &r = lsqr::kOptions[i];
    CHECK(r.doc && strlen(r.doc) > 10, "%s has no documentation", r.name);
    members += r.member != nullptr;
    for (size_t j = i + 1; j < rows; j++) {
      CHECK(strcmp(r.name, lsqr::kOptions[j].name) != 0, "two rows named %s", r.name);
      CHECK(!r.member || r.member != lsqr::kOptions[j].member, "%s and %s share a member", r.name, lsqr::kOptions[j].name);
    }
    bool expected = false;
    for (const Expect &e : kExpect) expected = expected || (!strcmp(e.name, r.name) && e.member == r.member);
    CHECK(expected, "row %s: not expected, or on another member", r.name);
  }
  // every member of Options has a row: a struct of `members` ints and nothing else
  CHECK(sizeof(Options) == members * sizeof(int), "%zu bytes, %zu members with a row", sizeof(Options), members);
}

void test_defaults() {
  const Options o;
  for (const Expect &e : kExpect)
    if (e.member) CHECK(o.*(e.member) == e.def, "%s defaults to %d, expected %d", e.name, o.*(e.member), e.def);
}

void test_rules() {
  int drops_seen = 0;
  for (const Expect &e : kExpect) {
    bool any_drop = false;
    for (int v : kValues) {
      Options o;
      const Options before = o;
      bool drops = true;
      char why[256] = "";
      const int st = lsqr::options_set(o, e.name, v, &drops, why, sizeof why);
      int stored = 0;
      if (model(e, v, &stored)) {
        CHECK(st == LSQR_OK, "%s = %d: status %d", e.name, v, st);
        if (e.member) {
          CHECK(o.*(e.member) == stored, "%s = %d stored %d, expected %d", e.name, v, o.*(e.member), stored);
          o.*(e.member) = e.def;
        }
        CHECK(same(o, before), "%s = %d touched another member", e.name, v);
        CHECK(drops == e.drops, "%s = %d: drops_index %d", e.name, v, (int)drops);
        any_drop = any_drop || drops;
      } else {
        CHECK(st == LSQR_ERR_INVALID, "%s = %d: status %d, expected LSQR_ERR_INVALID", e.name, v, st);
        CHECK(same(o, before), "%s = %d refused, but a member changed", e.name, v);
        CHECK(why[0] != 0, "%s = %d refused without a message", e.name, v);
        CHECK(!drops, "%s = %d refused, but drops the index", e.name, v);
      }
    }
    drops_seen += any_drop;
    // a set that changes nothing drops the index all the same
    if (e.drops) {
      Options o;
      bool drops = false;
      char why[64];
      CHECK(lsqr::options_set(o, e.name, e.def, &drops, why, sizeof why) == LSQR_OK && drops, "%s", e.name);
    }
  }
  CHECK(drops_seen == 4, "%d options drop the index", drops_seen);
}

void test_a_failed_set_keeps_an_earlier_value() {
  Options o;
  bool drops = false;
  char why[256] = "";
  CHECK(lsqr::options_set(o, "scan_hsplit", 128, &drops, why, sizeof why) == LSQR_OK && o.hsplit == 128, "set");
  CHECK(lsqr::options_set(o, "scan_hsplit", 129, &drops, why, sizeof why) == LSQR_ERR_INVALID && o.hsplit == 128, "kept");
  CHECK(strstr(why, "scan_hsplit") != nullptr, "the message names the option: %s", why);
}

void test_unknown_names() {
  for (const char *name : {"", "no_such_option", "scan_ppl ", "SCAN_PPL", "opt_ppl", "ppl"}) {
    Options o;
    const Options before = o;
    bool drops = true;
    char why[64] = "";
    const int st = lsqr::options_set(o, name, 1, &drops, why, sizeof why);
    CHECK(st == lsqr::kOptUnknown, "\"%s\": status %d", name, st);
    CHECK(st != LSQR_OK && st != LSQR_EMPTY && st != LSQR_ERR_INVALID && st != LSQR_ERR_NO_DEVICE && st != LSQR_ERR_HIP &&
              st != LSQR_ERR_STATE, "the status of an unknown name is no lsqr_status");
    CHECK(same(o, before) && !drops, "\"%s\" changed something", name);
  }
}

}  // namespace

int main() {
  test_table_shape();
  test_defaults();
  test_rules();
  test_a_failed_set_keeps_an_earlier_value();
  test_unknown_names();
  if (failures) {
    printf("options test: %d failures\n", failures);
    return 1;
  }
  printf("options test ok: %zu options\n", kExpect.size());
  return 0;
}
