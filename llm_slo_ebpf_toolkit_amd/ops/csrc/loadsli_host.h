// Host side of the load SLI tracker (loadsli.h) that needs no device: the time and duration rules,
// the placement of a request's interval in the ring, the cell, the scan operator, the classification,
// the per-service row, the configuration and argument checks, the result block's layout and the bound
// on the ring's population. Plain C++ (no HIP header), so it builds and runs on its own under the host
// sanitizers (tests/native/loadsli_host_check.cpp); the kernels use the same helpers. The bins, slots
// and the advance are the breach-onset tracker's (onset_host.h), here in microseconds.
// pipeline/loadsli.py carries the same constants and rules in numpy.
//
// Why every product fits 64 bits. validate() requires ring_records_max * bins * bin_us <= 2^53 and the
// host refuses a step that would put more than ring_records_max spans into the ring. A request adds at
// most bin_us of busy time to a bin and at most bin_us of idle time to each of two cells, so every
// idle cell, every bin's active * bin_us and every busy sum stay at or below 2^53, and busy * 1000 <
// 2^63. A concurrency in thousandths is at most records * 1000 < 2^41, times factor_milli (< 2^16)
// below 2^57. The arrival compares multiply a count (< 2^31), a number of bins (<= 2^13) and
// factor_milli (< 2^16) or 1000: below 2^60. The host check verifies the compares against unsigned
// __int128 at these extremes.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <stdexcept>
#include <utility>
#include <vector>

#include "onset_host.h"
#include "steplane_host.h"  // Range, plan_ranges, kSpanBytes

namespace mislo {
namespace loadsli {

using onset::kLdsProbes;
using onset::kLdsSlots;
using onset::kMaxBins;
using onset::kMinBins;
using onset::kNoBin;
using onset::lds_hash;

constexpr int64_t kMinBinUs = 1000ll;
constexpr int64_t kMaxBinUs = 60000000ll;
constexpr float kMaxLatencyMs = 86400000.f;  // a day; exact in float32
constexpr int64_t kMaxRingRecords = 2147483647ll;  // 2^31 - 1: a cell's starts cannot carry into its ends
constexpr int64_t kMaxProduct = int64_t(1) << 53;  // ring_records_max * bins * bin_us, at most
constexpr int64_t kMinFactorMilli = 1001, kMaxFactorMilli = 64000;
constexpr int64_t kMaxMinRequests = 2147483647ll;
constexpr int64_t kMaxMinConcMilli = 1000000000ll;
constexpr int kRowBytes = 80;
constexpr int kRowWords = kRowBytes / 4;
// records that do not end a request: first-token records (bit 2) and start records (bit 3)
constexpr uint32_t kSpanFirstTokenBit = 4u, kSpanStartBit = 8u;
constexpr uint32_t kNotAnEnd = kSpanFirstTokenBit | kSpanStartBit;
constexpr uint32_t kCarrySlot = 0x2000u;  // the LDS key's slot of a service's carry increments (a ring slot is < 2^13)

// per-step statistics (uint32 each), pipeline/loadsli.py STATS in the same order
enum Stat {
  kObserved = 0,    // finishing records with a service, a valid duration and a start time
  kOutOfGroup = 1,  // finishing records with group_id >= n_groups
  kInvalid = 2,     // latency_ms NaN, negative or above a day
  kNoTime = 3,      // ts_ns <= 0
  kFuture = 4,      // observed, starting or ending beyond q_hi: moved or cut to q_hi
  kTooOld = 5,      // observed, ended before the ring's oldest bin: placed nowhere
  kClipped = 6,     // observed, started before the ring's oldest bin: only its end is placed
  kLong = 7,        // observed, longer than the settle time
  kStats = 8
};

enum State : uint32_t { kSteady = 0, kSurge = 1, kSlowdown = 2, kDrop = 3, kWarming = 4 };
constexpr uint32_t kArrUp = 1u, kConcUp = 2u, kArrDown = 4u;  // Row::flags

// One service (pipeline/loadsli.py LOAD_ROW).
struct Row {
  uint32_t state, age;
  int64_t peak_q;  // the first bin of the ring with the largest active, -1 for an empty ring
  uint64_t busy_recent, busy_base, busy_ring;  // in-flight time, microseconds
  uint32_t arr_recent, arr_base, done_recent, done_base;
  uint32_t peak_active, base_bins;
  uint32_t arr_ring, flags;
  uint32_t pad[2];
};
static_assert(sizeof(Row) == kRowBytes, "a load row is 80 bytes");

// ---- times ------------------------------------------------------------------------------------
MISLO_ON_HD inline int64_t ts_us_of(int64_t ts_ns) { return ts_ns / 1000; }
// a valid latency_ms (0 <= v <= a day) in whole microseconds: one IEEE double multiply, truncated
MISLO_ON_HD inline int64_t dur_us_of(float latency_ms) { return (int64_t)((double)latency_ms * 1000.0); }
MISLO_ON_HD inline bool latency_valid(float v) { return v >= 0.f && v <= kMaxLatencyMs; }  // NaN fails both

// ---- cell -------------------------------------------------------------------------------------
// (service, slot) has two u64 cells: counts = starts in the low word, ends in the high one; idle_us
constexpr uint64_t kStartAdd = 1ull, kEndAdd = 1ull << 32;
MISLO_ON_HD inline uint32_t cell_starts(uint64_t c) { return (uint32_t)c; }
MISLO_ON_HD inline uint32_t cell_ends(uint64_t c) { return (uint32_t)(c >> 32); }
MISLO_ON_HD inline int64_t cell_delta(uint64_t c) { return (int64_t)cell_starts(c) - (int64_t)cell_ends(c); }

// ---- placement --------------------------------------------------------------------------------
enum PlaceBits : uint32_t { kPFuture = 1u, kPTooOld = 2u, kPClipped = 4u, kPStart = 8u, kPEnd = 16u };
struct Placement {
  uint32_t bits;       // PlaceBits
  int64_t qs, qe;      // the bins of the start (kPStart) and of the end (kPEnd)
  uint64_t idle_s, idle_e;  // idle time the start adds at qs, the end at qe
};
// Where an observed request [ts_us, ts_us + dur_us) goes in a ring of `bins` bins ending at q_hi.
MISLO_ON_HD inline Placement place(int64_t ts_us, int64_t dur_us, int64_t bin_us, int64_t q_hi, uint32_t bins) {
  Placement p{0u, 0, 0, 0ull, 0ull};
  int64_t te_us = ts_us + dur_us;
  int64_t qs = ts_us / bin_us, qe = te_us / bin_us;
  const int64_t oldest = onset::oldest_bin(q_hi, bins);
  if (qs > q_hi) {  // a clock ahead of the agent: a zero-length request in q_hi
    p.bits |= kPFuture;
    qs = qe = q_hi;
    ts_us = te_us = q_hi * bin_us;
  } else if (qe > q_hi) {
    p.bits |= kPFuture;
    te_us = (q_hi + 1) * bin_us;
    qe = q_hi;
  }
  if (qe < oldest) {
    p.bits |= kPTooOld;
    return p;
  }
  if (qs < oldest) {
    p.bits |= kPClipped;
  } else {
    p.bits |= kPStart;
    p.qs = qs;
    p.idle_s = (uint64_t)(ts_us - qs * bin_us);
  }
  p.bits |= kPEnd;
  p.qe = qe;
  p.idle_e = (uint64_t)((qe + 1) * bin_us - te_us);
  return p;
}

// ---- the scan ---------------------------------------------------------------------------------
// Requests in flight after a run of bins = before it + the run's sum of (starts - ends): the scan
// operator is the plain sum, its identity 0.
MISLO_ON_HD inline int64_t combine(int64_t a, int64_t b) { return a + b; }
// a bin from the requests in flight before it: those touching it, and their time inside it
MISLO_ON_HD inline int64_t bin_active(int64_t a_before, uint64_t counts) { return a_before + (int64_t)cell_starts(counts); }
MISLO_ON_HD inline int64_t bin_busy(int64_t active, int64_t bin_us, uint64_t idle_us) { return active * bin_us - (int64_t)idle_us; }

// ---- ranges -----------------------------------------------------------------------------------
struct Ranges {
  int64_t oldest, lo;        // the ring's oldest bin; the first bin with whole history: max(oldest, q_first)
  int64_t recent_lo, recent_hi;  // recent = [recent_lo, recent_hi]
  int64_t base_lo, base_hi;      // base = [base_lo, base_hi], empty when base_bins == 0
  uint32_t base_bins;
  bool warming;
};
MISLO_ON_HD inline Ranges ranges_of(int64_t q_hi, int64_t q_first, uint32_t bins, int settle, int recent, int min_base_bins) {
  Ranges r;
  r.oldest = onset::oldest_bin(q_hi, bins);
  r.lo = r.oldest > q_first ? r.oldest : q_first;
  r.recent_hi = q_hi - settle;
  r.recent_lo = r.recent_hi - recent + 1;
  r.base_lo = r.lo;
  r.base_hi = r.recent_lo - 1;
  const int64_t nb = r.base_hi - r.base_lo + 1;
  r.base_bins = nb > 0 ? (uint32_t)nb : 0u;
  r.warming = r.recent_lo < r.lo || r.base_bins < (uint32_t)min_base_bins;
  return r;
}

// ---- classification ---------------------------------------------------------------------------
struct Sums {
  uint64_t busy_recent, busy_base;
  uint32_t arr_recent, arr_base;
};
// busy time over `nbins` bins as a concurrency in thousandths (floor)
MISLO_ON_HD inline uint64_t conc_milli(uint64_t busy_us, uint32_t nbins, int64_t bin_us) {
  return busy_us * 1000ull / ((uint64_t)nbins * (uint64_t)bin_us);
}
// the three predicates (kArrUp | kConcUp | kArrDown) of a row that is not warming: nb >= 1, nr >= 1
MISLO_ON_HD inline uint32_t predicates(const Sums& s, uint32_t nb, uint32_t nr, int64_t bin_us, int64_t f, int64_t min_requests,
                                       int64_t min_conc_milli) {
  const uint64_t ar = s.arr_recent, ab = s.arr_base, F = (uint64_t)f;
  uint32_t flags = 0u;
  if (ar >= (uint64_t)min_requests && ar * nb * 1000ull >= F * ab * nr) flags |= kArrUp;
  if (ab * nr >= (uint64_t)min_requests * nb && ar * nb * F <= 1000ull * ab * nr) flags |= kArrDown;
  const uint64_t cr = conc_milli(s.busy_recent, nr, bin_us), cb = conc_milli(s.busy_base, nb, bin_us);
  if (cr >= (uint64_t)min_conc_milli && cr * 1000ull >= F * cb) flags |= kConcUp;
  return flags;
}
MISLO_ON_HD inline uint32_t state_of(uint32_t flags) {
  return (flags & kArrUp) ? kSurge : (flags & kConcUp) ? kSlowdown : (flags & kArrDown) ? kDrop : kSteady;
}
// consecutive steps in the same state among surge, slowdown and drop; saturating
MISLO_ON_HD inline uint32_t age_of(uint32_t state, uint32_t prev_state, uint32_t prev_age) {
  if (state < kSurge || state > kDrop) return 0u;
  if (state != prev_state) return 1u;
  return prev_age == 0xffffffffu ? prev_age : prev_age + 1u;
}

// the LDS table's key of (service, slot): never 0; slot < 2^13, or kCarrySlot
MISLO_ON_HD inline uint64_t lds_key(uint32_t g, uint32_t slot) { return ((uint64_t)(g + 1u) << 16) | (uint64_t)slot; }
MISLO_ON_HD inline uint32_t lds_group(uint64_t key) { return (uint32_t)(key >> 16) - 1u; }
MISLO_ON_HD inline uint32_t lds_slot(uint64_t key) { return (uint32_t)key & 0xffffu; }

// the largest ring_records_max the 2^53 bound allows, capped at 2^31 - 1
inline int64_t default_ring_records_max(int bins, int64_t bin_us) {
  const int64_t m = kMaxProduct / ((int64_t)bins * bin_us);
  return m < kMaxRingRecords ? m : kMaxRingRecords;
}

struct Config {
  int device = 0;
  int bins = 1024;                 // B: ring bins per service, a power of two
  int64_t bin_us = 500000ll;       // a 2 s window over 4 bins
  int settle_bins = 30;            // newest bins left out: requests still in flight are invisible
  int recent_bins = 30;            // R
  int min_base_bins = 60;          // base bins before a row stops warming
  int64_t factor_milli = 1500;     // f, thousandths
  int64_t min_requests = 20;
  int64_t min_conc_milli = 1000;
  int span_cap = 16384;            // span records per step
  int group_cap = 64;              // services (incident groups), at most
  int n_buffers = 3;               // steps whose results stay readable
  int64_t ring_records_max = default_ring_records_max(1024, 500000ll);  // spans offered by the steps the ring still holds, at most
  bool lds = true;                 // pre-aggregate every workgroup's records in LDS (off: the measurement's other side)
};

// The result block of one step, in uint32 words: rows[group_cap] (20 words each), then stats[8];
// every array starts on 16 bytes.
struct Layout {
  size_t rows = 0, stats = 0, words = 0;
};
inline Layout layout(int group_cap) {
  Layout l;
  l.rows = 0;
  l.stats = (size_t)group_cap * kRowWords;  // 80 bytes a row: a multiple of 16
  l.words = (l.stats + kStats + 3) & ~size_t(3);
  return l;
}

// spans, the two cell arrays, carry + age + previous state, the block
inline uint64_t device_bytes(int bins, int span_cap, int group_cap) {
  return (uint64_t)span_cap * kSpanBytes + (uint64_t)group_cap * (uint64_t)bins * 16 + (uint64_t)group_cap * 12 +
         (uint64_t)layout(group_cap).words * 4;
}
inline uint64_t device_bytes(const Config& c) { return device_bytes(c.bins, c.span_cap, c.group_cap); }

// What an image of this tracker's state depends on (steplane_host.h lane::Fingerprint): every field that
// shapes the state or its meaning, and the layout's constants; not device, n_buffers, span_cap or lds.
inline lane::Fingerprint fingerprint(const Config& c) {
  using lane::field;
  lane::Fingerprint f;
  f.kind = lane::kLoadSli;
  f.fields = {field("group_cap", c.group_cap),
              field("bins", c.bins),
              field("bin_us", c.bin_us),
              field("settle_bins", c.settle_bins),
              field("recent_bins", c.recent_bins),
              field("min_base_bins", c.min_base_bins),
              field("factor_milli", c.factor_milli),
              field("min_requests", c.min_requests),
              field("min_conc_milli", c.min_conc_milli),
              field("ring_records_max", c.ring_records_max)};
  return f;
}

inline void validate(const Config& c) {
  if (c.bins < kMinBins || c.bins > kMaxBins || (c.bins & (c.bins - 1)) != 0)
    throw std::invalid_argument("load sli: bins must be a power of two in [64, 8192]");
  if (c.bin_us < kMinBinUs || c.bin_us > kMaxBinUs) throw std::invalid_argument("load sli: bin_us must be in [1000, 60000000]");
  if (c.settle_bins < 0) throw std::invalid_argument("load sli: settle_bins must be >= 0");
  if (c.recent_bins < 1) throw std::invalid_argument("load sli: recent_bins must be >= 1");
  if (c.min_base_bins < 1) throw std::invalid_argument("load sli: min_base_bins must be >= 1");
  if ((int64_t)c.settle_bins + c.recent_bins + c.min_base_bins > c.bins)
    throw std::invalid_argument("load sli: settle_bins + recent_bins + min_base_bins must fit the ring's bins");
  if (c.factor_milli < kMinFactorMilli || c.factor_milli > kMaxFactorMilli)
    throw std::invalid_argument("load sli: factor_milli must be in [1001, 64000]");
  if (c.min_requests < 1 || c.min_requests > kMaxMinRequests)
    throw std::invalid_argument("load sli: min_requests must be in [1, 2^31 - 1]");
  if (c.min_conc_milli < 1 || c.min_conc_milli > kMaxMinConcMilli)
    throw std::invalid_argument("load sli: min_conc_milli must be in [1, 1000000000]");
  if (c.group_cap < 1 || c.group_cap > 65536) throw std::invalid_argument("load sli: group_cap must be in [1, 65536]");
  if (c.span_cap < 1) throw std::invalid_argument("load sli: span_cap must be >= 1");
  if (c.n_buffers < 1 || c.n_buffers > 64) throw std::invalid_argument("load sli: n_buffers out of range");
  if (device_bytes(c) > (uint64_t(1) << 31)) throw std::invalid_argument("load sli: the ring needs more than 2 GiB");
  if (c.ring_records_max < 1 || c.ring_records_max > default_ring_records_max(c.bins, c.bin_us))
    throw std::invalid_argument("load sli: ring_records_max * bins * bin_us must be in [1, 2^53], ring_records_max <= 2^31 - 1");
}

using mislo::Range;
inline size_t plan_ranges(const std::vector<Range>& ranges, int span_cap) {
  return mislo::plan_ranges(ranges, span_cap, "load sli");
}

inline void check_step(int64_t cut_ns, int n_groups, int group_cap) {
  if (cut_ns <= 0) throw std::invalid_argument("load sli step: cut_ns must be > 0");
  if (n_groups < 0 || n_groups > group_cap) throw std::invalid_argument("load sli step: n_groups out of range");
}

// The bound that keeps the ring exact: the breach-onset tracker's deque of (q_hi of the step, spans
// offered); a step that would pass ring_records_max is refused before anything changes.
class Population {
 public:
  Population(uint32_t bins, int64_t max) : held_(bins, max), max_(max) {}
  int64_t after(int64_t q_hi, size_t n) const { return held_.after(q_hi, n); }
  void check(int64_t q_hi, size_t n) const {
    if (after(q_hi, n) > max_) throw std::invalid_argument("load sli step: the ring would hold more than ring_records_max spans");
  }
  void take(int64_t q_hi, size_t n) { held_.take(q_hi, n); }
  size_t steps() const { return held_.steps(); }

 private:
  onset::Population held_;
  int64_t max_;
};

}  // namespace loadsli
}  // namespace mislo
