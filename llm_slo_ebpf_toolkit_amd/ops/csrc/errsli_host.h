// Host side of the error SLI tracker (errsli.h) that needs no device: the outcome class of a span's
// flags, the burn compare, the budget, the LDS table's key, the configuration and argument checks and
// the result block's layout. Plain C++ (no HIP header), so it builds and runs on its own under the host
// sanitizers (tests/native/errsli_host_check.cpp); the kernels use the same helpers.
// pipeline/errsli.py carries the same constants and rules in numpy. Everything is in integers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <stdexcept>
#include <utility>
#include <vector>

#include "onset_host.h"      // lds_hash, kLdsSlots, kLdsProbes: the observe kernel's table is onset's
#include "slisketch_host.h"  // MISLO_SK_HD
#include "steplane_host.h"   // Range, plan_ranges, kSpanBytes

namespace mislo {
namespace errsli {

constexpr uint32_t kOutcomeShift = 4;      // Span::flags bits 4-7: the request's outcome class, 0 = ok
constexpr uint32_t kOutcomeMask = 0xF0u;   // collector/records.py SPAN_OUTCOME_MASK
constexpr uint32_t kSkipMask = 4u | 8u;    // first-token and start records: not a finished request
constexpr int kClasses = 8;                // ok client cancelled throttled timeout unavailable server other
constexpr int kMaxPairs = 4;               // (long window, short window, factor) pairs, at most
constexpr int kPairWords = 4;              // n_long, bad_long, n_short, bad_short
constexpr int kPairLane0 = kClasses;       // the roll kernel's lane 8 + 2 p + which owns pair p's window
constexpr uint32_t kBadAllowed = 0xFEu;    // ok can never burn the budget
constexpr uint32_t kBadDefault = 0xF8u;    // throttled, timeout, unavailable, server, other
constexpr uint64_t kBurnScale = 1000000000ull;  // factor_milli * budget_ppm is in 10^-9
constexpr int kLdsSlots = onset::kLdsSlots;
constexpr int kLdsProbes = onset::kLdsProbes;

// per-step statistics (uint32 each), pipeline/errsli.py STATS in the same order
enum Stat {
  kObserved = 0,    // finished requests counted under their class
  kOutOfGroup = 1,  // group_id >= n_groups
  kReserved = 2,    // class 8-15: never written by the receiver
  kStats = 8
};

MISLO_SK_HD inline uint32_t outcome_of(uint32_t flags) { return (flags >> kOutcomeShift) & 15u; }
MISLO_SK_HD inline uint32_t pack_outcome(uint32_t c) { return (c & 15u) << kOutcomeShift; }

// Does a window of n requests, `bad` of them against the budget, burn at `thr` = factor_milli *
// budget_ppm? bad / n >= factor * budget, in integers: bad * 10^9 >= thr * n. validate() keeps
// thr <= 10^9 < 2^30 and span_cap * windows < 2^32, so n and bad stay below 2^32 and both products
// below 2^62: the compare fits 64 bits (the host check verifies it against unsigned __int128 at
// n = bad = 2^32 - 1, thr = 10^9). Equality burns; an empty window never does.
MISLO_SK_HD inline bool burns(uint32_t n, uint32_t bad, uint32_t min_requests, uint64_t thr) {
  return n >= min_requests && n > 0u && (uint64_t)bad * kBurnScale >= thr * (uint64_t)n;
}

// the error budget in millionths: round half up, clamped to 1 .. 10^6
inline uint32_t budget_ppm(double target) {
  const double x = (1.0 - target) * 1e6 + 0.5;
  if (!(x >= 1.0)) return 1u;
  return x >= 1e6 ? 1000000u : (uint32_t)x;
}

MISLO_SK_HD inline uint32_t next_age(uint32_t age, uint32_t firing) {
  return firing == 0u ? 0u : (age == 0xffffffffu ? age : age + 1u);
}

// The LDS table's key of (service, class). Never 0.
MISLO_SK_HD inline uint64_t lds_key(uint32_t g, uint32_t c) { return ((uint64_t)(g + 1u) << 16) | (uint64_t)c; }
MISLO_SK_HD inline uint32_t lds_group(uint64_t key) { return (uint32_t)(key >> 16) - 1u; }
MISLO_SK_HD inline uint32_t lds_class(uint64_t key) { return (uint32_t)key & 0xffffu; }

struct Pair {
  int long_windows = 0;
  int short_windows = 0;
  int64_t factor_milli = 0;
};

struct Config {
  int device = 0;
  int span_cap = 16384;          // span records per step
  int group_cap = 64;            // services (incident groups), at most
  int windows = 3600;            // the rolling horizon W, in steps
  int n_buffers = 3;             // steps whose results stay readable
  double target = 0.999;         // the availability target; the budget is 1 - target
  std::vector<Pair> pairs{{3600, 300, 14400}};
  int64_t min_requests = 20;     // fewest requests in a window X for it to burn
  uint32_t bad_mask = kBadDefault;
  bool lds = true;               // pre-aggregate every workgroup's records in LDS (off: the measurement's other side)
};

// words of device state per service: a row of the horizon; the pairs' rolling sums and the age
constexpr size_t kRowWords = kClasses;
constexpr size_t kSumWords = (size_t)kMaxPairs * kPairWords;

// The result block of one step, in uint32 words, every array on 16 bytes, G = group_cap:
//   counts[G][8]  counts_roll[G][8]  pair_sums[G][4][4]  firing[G]  age[G]  stats[8]
struct Layout {
  size_t counts = 0, counts_roll = 0, pair_sums = 0, firing = 0, age = 0, stats = 0, words = 0;
};
inline Layout layout(int group_cap) {
  const size_t g = (size_t)group_cap, one = (g + 3) & ~size_t(3);
  Layout l;
  l.counts = 0;
  l.counts_roll = l.counts + kRowWords * g;
  l.pair_sums = l.counts_roll + kRowWords * g;
  l.firing = l.pair_sums + kSumWords * g;
  l.age = l.firing + one;
  l.stats = l.age + one;
  l.words = l.stats + kStats;
  return l;
}

// spans, the horizon's rows + the rolling row + the step's row, the pairs' sums and the age, the block
inline uint64_t device_bytes(const Config& c) {
  return (uint64_t)c.span_cap * kSpanBytes + ((uint64_t)c.windows + 2) * (uint64_t)c.group_cap * kRowWords * 4 +
         (uint64_t)c.group_cap * (kSumWords + 1) * 4 + (uint64_t)layout(c.group_cap).words * 4;
}

// What an image of this tracker's state depends on (steplane_host.h lane::Fingerprint): every field that
// shapes the state or its meaning, and the layout's constants; not device, n_buffers, span_cap or lds.
inline lane::Fingerprint fingerprint(const Config& c) {
  using lane::field;
  static const char* const pair_names[kMaxPairs][3] = {{"pair 0 long", "pair 0 short", "pair 0 factor_milli"},
                                                       {"pair 1 long", "pair 1 short", "pair 1 factor_milli"},
                                                       {"pair 2 long", "pair 2 short", "pair 2 factor_milli"},
                                                       {"pair 3 long", "pair 3 short", "pair 3 factor_milli"}};
  lane::Fingerprint f;
  f.kind = lane::kErrSli;
  f.fields = {field("group_cap", c.group_cap), field("windows", c.windows), lane::real_field("target", c.target),
              field("min_requests", c.min_requests), field("bad_mask", c.bad_mask), field("pairs", (int64_t)c.pairs.size()),
              field("classes", kClasses)};
  for (size_t p = 0; p < c.pairs.size() && p < (size_t)kMaxPairs; ++p) {
    f.fields.push_back(field(pair_names[p][0], c.pairs[p].long_windows));
    f.fields.push_back(field(pair_names[p][1], c.pairs[p].short_windows));
    f.fields.push_back(field(pair_names[p][2], c.pairs[p].factor_milli));
  }
  return f;
}

inline void validate(const Config& c) {
  if (c.windows < 1 || c.windows > 32768) throw std::invalid_argument("error sli: windows must be in [1, 32768]");
  if (c.group_cap < 1 || c.group_cap > 65536) throw std::invalid_argument("error sli: group_cap must be in [1, 65536]");
  if (c.span_cap < 1) throw std::invalid_argument("error sli: span_cap must be >= 1");
  if ((uint64_t)c.span_cap * (uint64_t)c.windows >= (uint64_t(1) << 32))
    throw std::invalid_argument("error sli: span_cap * windows must stay below 2^32 (a rolling counter would wrap)");
  if (c.n_buffers < 1 || c.n_buffers > 64) throw std::invalid_argument("error sli: n_buffers out of range");
  if (!std::isfinite(c.target) || c.target < 0.0 || !(c.target < 1.0))
    throw std::invalid_argument("error sli: target must be finite and in [0, 1)");
  if (c.pairs.empty() || c.pairs.size() > (size_t)kMaxPairs) throw std::invalid_argument("error sli: 1 to 4 burn pairs");
  const uint64_t budget = budget_ppm(c.target);
  for (const Pair& p : c.pairs) {
    if (p.short_windows < 1 || p.short_windows > p.long_windows || p.long_windows > c.windows)
      throw std::invalid_argument("error sli: a pair needs 1 <= short <= long <= windows");
    if (p.factor_milli < 1) throw std::invalid_argument("error sli: a pair's factor_milli must be >= 1");
    if ((uint64_t)p.factor_milli > kBurnScale || (uint64_t)p.factor_milli * budget > kBurnScale)
      throw std::invalid_argument("error sli: factor * budget above 1 asks for more failures than requests");
  }
  if (c.min_requests < 0 || c.min_requests > (int64_t)0xffffffffll)
    throw std::invalid_argument("error sli: min_requests must be in [0, 2^32)");
  if (c.bad_mask == 0u || (c.bad_mask & ~kBadAllowed)) throw std::invalid_argument("error sli: bad_mask must be non-zero and within 0xFE");
  if (device_bytes(c) > (uint64_t(1) << 31)) throw std::invalid_argument("error sli: the horizon needs more than 2 GiB");
}

using mislo::Range;
inline size_t plan_ranges(const std::vector<Range>& ranges, int span_cap) {
  return mislo::plan_ranges(ranges, span_cap, "error sli");
}

inline void check_step(int n_groups, int group_cap) {
  if (n_groups < 0 || n_groups > group_cap) throw std::invalid_argument("error sli step: n_groups out of range");
}

}  // namespace errsli
}  // namespace mislo
