// Host side of the saturation curve tracker (satcurve.h) that needs no device: the level of a bin, the
// third cell, the fold of evicted bins into two generations, the knee rule, the state, the per-service
// row, the configuration and argument checks, the result block's layout and the two population bounds.
// Plain C++ (no HIP header), so it builds and runs on its own under the host sanitizers
// (tests/native/satcurve_host_check.cpp); the kernels use the same helpers. The time and duration
// rules, place(), bin_active, bin_busy and the LDS key are the load tracker's (loadsli_host.h); the
// bins, slots and the advance are the breach-onset tracker's (onset_host.h); the level is the decode
// tracker's bucket rule (decodesli_host.h); the budget is the error tracker's (errsli_host.h).
// pipeline/satcurve.py carries the same constants and rules in numpy.
//
// Why every quantity fits 64 bits. The ring keeps the load tracker's bound: ring_records_max * bins *
// bin_us <= 2^53, so every bin's busy time is at most 2^53 and busy * 8 <= 2^56. For the curve the host
// keeps (epoch of the step's q_hi, spans offered) and refuses a step when the spans offered in the
// current epoch and the two before it would pass curve_records_max <= 2^40. A step places records only
// in bins of its own ring, (q' - bins, q'] for its q_hi q', and bins <= epoch_bins: a bin of epoch x got
// its records from steps of epoch x or x + 1. The merged curve reads the ring and the generations of
// epoch x_now and x_now - 1, where x_now = epoch(q_hi - bins) >= epoch(q_hi) - 1. So every request in it
// was offered by a step of an epoch in [x_now - 1, epoch(q_hi)], within the current epoch and the two
// before it. Hence every curve n (and b <= n) is at most 2^40, |d_l| = |b_l * 10^6 - budget_ppm * n_l|
// < 2^60 with 10^6 < 2^20, and because the n_l sum to at most 2^40 as well, every suffix sum |S_l| <
// 2^61. The host check compares knee_of against __int128 at these extremes.
//
// Why the knee has data of its own. The knee k is the largest level at which S attains its maximum,
// and that maximum is > 0. S_k = d_k + S_{k+1} (S_K = 0, the empty suffix). S_{k+1} <= max = S_k, and
// S_{k+1} != S_k: otherwise k + 1 would attain the maximum too (for k = K - 1: S_K = 0 < S_k). So
// d_k > 0, hence b_k > 0 and n_k >= b_k > 0.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <deque>
#include <stdexcept>
#include <utility>
#include <vector>

#include "decodesli_host.h"
#include "errsli_host.h"
#include "loadsli_host.h"
#include "onset_host.h"
#include "steplane_host.h"  // Range, plan_ranges, kSpanBytes

namespace mislo {
namespace satcurve {

using loadsli::kCarrySlot;
using loadsli::kEndAdd;
using loadsli::kNotAnEnd;
using loadsli::kStartAdd;
using onset::kLdsProbes;
using onset::kLdsSlots;
using onset::kMaxBins;
using onset::kMinBins;
using onset::kNoBin;
using onset::lds_hash;

constexpr int kK = 160;                    // levels: decodesli::bucket_of(0 .. 8191)
constexpr uint32_t kMaxU = 8191u;          // eighths of a request, clamped: level 159
constexpr uint32_t kNone = 0xffffffffu;    // no knee, no top level
constexpr int kPerLane = 3;                // the scan's lane l owns levels 3 l .. 3 l + 2
constexpr int64_t kMillion = 1000000ll;
constexpr int64_t kMaxEpochBins = 2147483647ll;
constexpr int64_t kMaxMinRequests = 2147483647ll;
constexpr int64_t kMaxCurveRecords = int64_t(1) << 40;
constexpr int kRowBytes = 64;
constexpr int kRowWords = kRowBytes / 4;
constexpr int kCurveWords = kK * 4;  // a row's merged curve: kK x (u64 n, u64 b)
static_assert(kK <= 64 * kPerLane, "one wave owns every level");

// per-step statistics (uint32 each), pipeline/satcurve.py STATS in the same order
enum Stat {
  kObserved = 0,    // finishing records with a service, a valid duration and a start time
  kOutOfGroup = 1,  // finishing records with group_id >= n_groups
  kInvalid = 2,     // latency_ms NaN, negative or above a day
  kNoTime = 3,      // ts_ns <= 0
  kFuture = 4,      // observed, starting or ending beyond q_hi: moved or cut to q_hi
  kTooOld = 5,      // observed, ended before the ring's oldest bin: placed nowhere
  kClipped = 6,     // observed, started before the ring's oldest bin: only its end is placed
  kNoTtft = 7,      // observed, ttft_ms NaN or negative: occupies its interval, not in the curve
  kStats = 8
};

enum State : uint32_t { kUnknown = 0, kNoKnee = 1, kBelow = 2, kSaturated = 3 };

// One service (pipeline/satcurve.py SAT_ROW).
struct Row {
  uint32_t state, knee_level, recent_u, top_level;
  uint64_t n_total, b_total;
  uint64_t n_knee, b_knee;
  uint64_t busy_recent;
  uint32_t age, pad;
};
static_assert(sizeof(Row) == kRowBytes, "a saturation row is 64 bytes");

// ---- the third cell ---------------------------------------------------------------------------
// sli: requests with a TTFT that started in the bin in the low word, those above the SLO in the high one
MISLO_ON_HD inline bool has_ttft(float ttft_ms) { return ttft_ms >= 0.f; }  // NaN fails
MISLO_ON_HD inline uint64_t sli_add(float ttft_ms, float slo_ms) { return 1ull + ((uint64_t)(ttft_ms > slo_ms ? 1u : 0u) << 32); }
MISLO_ON_HD inline uint64_t sli_n(uint64_t c) { return c & 0xffffffffull; }
MISLO_ON_HD inline uint64_t sli_b(uint64_t c) { return c >> 32; }

// ---- a bin's level ----------------------------------------------------------------------------
// busy time over `span_us` as a concurrency in eighths of a request, clamped to kMaxU
MISLO_ON_HD inline uint32_t u_of(int64_t busy_us, int64_t span_us) {
  if (busy_us <= 0) return 0u;
  const uint64_t u = (uint64_t)busy_us * 8ull / (uint64_t)span_us;
  return u > kMaxU ? kMaxU : (uint32_t)u;
}
MISLO_ON_HD inline uint32_t level_of_u(uint32_t u) { return decodesli::bucket_of(u); }
// the level of a bin from the requests in flight before it and its two load cells
MISLO_ON_HD inline uint32_t level_of(int64_t a_before, uint64_t counts, uint64_t idle_us, int64_t bin_us) {
  return level_of_u(u_of(loadsli::bin_busy(loadsli::bin_active(a_before, counts), bin_us, idle_us), bin_us));
}
// a level's concurrency is lower(level) / 8
MISLO_ON_HD inline uint32_t lower_u(uint32_t level) { return decodesli::lower(level); }

// ---- the fold ---------------------------------------------------------------------------------
// What an advance from `prev` to `q_hi` evicts: the `count` oldest bins of the old ring from `first`,
// ascending; those from `lo` on (>= q_first, the bins with whole history) fold into their epoch's
// generation, `lo > hi`: none. The bins span at most two epochs because epoch_bins >= bins.
struct Fold {
  int64_t first;
  uint32_t count;
  int64_t lo, hi;
};
MISLO_ON_HD inline Fold fold_of(int64_t prev, int64_t q_hi, int64_t q_first, uint32_t bins) {
  Fold f{0, 0u, 0, -1};
  if (prev == kNoBin || q_hi <= prev) return f;  // an empty ring, or no advance
  f.count = onset::cleared(prev, q_hi, bins);
  f.first = onset::oldest_bin(prev, bins);
  f.hi = f.first + (int64_t)f.count - 1;
  f.lo = f.first > q_first ? f.first : q_first;
  return f;
}
MISLO_ON_HD inline int64_t epoch_of(int64_t q, int64_t epoch_bins) { return q / epoch_bins; }  // q >= 0
// the epoch whose generations the merged curve reads, with the one before it
MISLO_ON_HD inline int64_t epoch_now(int64_t oldest, int64_t epoch_bins) { return (oldest > 1 ? oldest - 1 : 0) / epoch_bins; }
MISLO_ON_HD inline bool gen_live(int64_t gen_epoch, int64_t x_now) { return gen_epoch >= 0 && (gen_epoch == x_now || gen_epoch + 1 == x_now); }

// The two generations' epochs, tracker-wide. begin() says which generations a fold invalidates and
// takes their new epochs: bit p set = clear generation p in every row before folding.
struct Generations {
  int64_t epoch[2] = {-1, -1};
  uint32_t begin(const Fold& f, int64_t epoch_bins) {
    uint32_t clear = 0u;
    if (f.lo > f.hi) return clear;
    for (int64_t x = epoch_of(f.lo, epoch_bins); x <= epoch_of(f.hi, epoch_bins); ++x)
      if (epoch[x & 1] != x) epoch[x & 1] = x, clear |= 1u << (x & 1);
    return clear;
  }
  uint32_t live(int64_t x_now) const { return (gen_live(epoch[0], x_now) ? 1u : 0u) | (gen_live(epoch[1], x_now) ? 2u : 0u); }
};

// ---- the knee ---------------------------------------------------------------------------------
MISLO_ON_HD inline int64_t score(uint64_t n, uint64_t b, int64_t budget_ppm) { return (int64_t)b * kMillion - budget_ppm * (int64_t)n; }
struct Knee {
  uint32_t level;  // kNone: no level's suffix is over budget
  uint64_t n, b;   // the suffix sums at the knee
  bool valid;      // n >= min_requests
};
// curve: kK x (n, b). The largest level at which the suffix sum of score attains its maximum, if > 0.
inline Knee knee_of(const uint64_t* curve, int64_t budget_ppm, int64_t min_requests) {
  Knee k{kNone, 0ull, 0ull, false};
  int64_t s = 0, best = 0;
  uint64_t n = 0, b = 0;
  for (int l = kK - 1; l >= 0; --l) {
    s += score(curve[2 * l], curve[2 * l + 1], budget_ppm);
    n += curve[2 * l], b += curve[2 * l + 1];
    if (s > best) best = s, k.level = (uint32_t)l, k.n = n, k.b = b;
  }
  k.valid = k.level != kNone && k.n >= (uint64_t)min_requests;
  return k;
}

// ---- state ------------------------------------------------------------------------------------
MISLO_ON_HD inline uint32_t state_of(bool recent_known, uint64_t n_total, int64_t min_requests, bool knee_valid,
                                     uint32_t recent_level, uint32_t knee_level) {
  if (!recent_known || n_total < (uint64_t)min_requests) return kUnknown;
  if (!knee_valid) return kNoKnee;
  return recent_level < knee_level ? kBelow : kSaturated;
}
// consecutive saturated steps; saturating
MISLO_ON_HD inline uint32_t age_of(uint32_t state, uint32_t prev_age) {
  if (state != kSaturated) return 0u;
  return prev_age == 0xffffffffu ? prev_age : prev_age + 1u;
}

// ---- ranges -----------------------------------------------------------------------------------
struct Ranges {
  int64_t oldest, lo;            // the ring's oldest bin; the first bin with whole history: max(oldest, q_first)
  int64_t settled_hi;            // the curve's ring part = [lo, settled_hi]
  int64_t recent_lo, recent_hi;  // recent = [recent_lo, recent_hi]
  bool recent_known;             // recent does not reach below lo
};
MISLO_ON_HD inline Ranges ranges_of(int64_t q_hi, int64_t q_first, uint32_t bins, int settle, int recent) {
  const loadsli::Ranges l = loadsli::ranges_of(q_hi, q_first, bins, settle, recent, 1);
  return Ranges{l.oldest, l.lo, l.recent_hi, l.recent_lo, l.recent_hi, l.recent_lo >= l.lo};
}

struct Config {
  int device = 0;
  int bins = 1024;                 // B: ring bins per service, a power of two
  int64_t bin_us = 500000ll;       // a 2 s window over 4 bins
  int settle_bins = 30;            // newest bins left out: requests still in flight are invisible
  int recent_bins = 30;            // R
  int64_t epoch_bins = 43200;      // a generation's length in bins (6 h), at least `bins`
  int64_t budget_ppm = 10000;      // the SLO's error budget in millionths (errsli::budget_ppm of a 99 % target)
  int64_t min_requests = 200;      // fewest requests at or above a knee, and in the whole curve
  double slo_ms = 800.0;           // a TTFT above it (float32 compare) is a breach
  int span_cap = 16384;            // span records per step
  int group_cap = 64;              // services (incident groups), at most
  int n_buffers = 3;               // steps whose results stay readable
  int64_t ring_records_max = loadsli::default_ring_records_max(1024, 500000ll);
  int64_t curve_records_max = kMaxCurveRecords;  // spans offered in the current epoch and the two before, at most
  bool lds = true;                 // pre-aggregate every workgroup's records in LDS (off: the measurement's other side)
};

// The result block of one step, in uint32 words: rows[group_cap] (16 words each), then
// curve[group_cap][kK][2] u64, then stats[8]; every array starts on 16 bytes.
struct Layout {
  size_t rows = 0, curve = 0, stats = 0, words = 0;
};
inline Layout layout(int group_cap) {
  Layout l;
  l.rows = 0;
  l.curve = (size_t)group_cap * kRowWords;
  l.stats = l.curve + (size_t)group_cap * kCurveWords;
  l.words = (l.stats + kStats + 3) & ~size_t(3);
  return l;
}

// spans, the three cell arrays, carry + age, the two generations, the block
inline uint64_t device_bytes(int bins, int span_cap, int group_cap) {
  return (uint64_t)span_cap * kSpanBytes + (uint64_t)group_cap * (uint64_t)bins * 24 + (uint64_t)group_cap * 8 +
         (uint64_t)group_cap * 2 * kK * 16 + (uint64_t)layout(group_cap).words * 4;
}
inline uint64_t device_bytes(const Config& c) { return device_bytes(c.bins, c.span_cap, c.group_cap); }

// What an image of this tracker's state depends on (steplane_host.h lane::Fingerprint): every field that
// shapes the state or its meaning, and the layout's constants; not device, n_buffers, span_cap or lds.
inline lane::Fingerprint fingerprint(const Config& c) {
  using lane::field;
  using lane::real_field;
  lane::Fingerprint f;
  f.kind = lane::kSatCurve;
  f.fields = {field("group_cap", c.group_cap),
              field("bins", c.bins),
              field("bin_us", c.bin_us),
              field("settle_bins", c.settle_bins),
              field("recent_bins", c.recent_bins),
              field("epoch_bins", c.epoch_bins),
              field("budget_ppm", c.budget_ppm),
              field("min_requests", c.min_requests),
              real_field("slo_ms", c.slo_ms),
              field("ring_records_max", c.ring_records_max),
              field("curve_records_max", c.curve_records_max),
              field("levels", kK)};
  return f;
}

inline void validate(const Config& c) {
  if (c.bins < kMinBins || c.bins > kMaxBins || (c.bins & (c.bins - 1)) != 0)
    throw std::invalid_argument("saturation curve: bins must be a power of two in [64, 8192]");
  if (c.bin_us < loadsli::kMinBinUs || c.bin_us > loadsli::kMaxBinUs)
    throw std::invalid_argument("saturation curve: bin_us must be in [1000, 60000000]");
  if (c.settle_bins < 0) throw std::invalid_argument("saturation curve: settle_bins must be >= 0");
  if (c.recent_bins < 1) throw std::invalid_argument("saturation curve: recent_bins must be >= 1");
  if ((int64_t)c.settle_bins + c.recent_bins > c.bins)
    throw std::invalid_argument("saturation curve: settle_bins + recent_bins must fit the ring's bins");
  if (c.epoch_bins < c.bins || c.epoch_bins > kMaxEpochBins)
    throw std::invalid_argument("saturation curve: epoch_bins must be in [bins, 2^31 - 1]");
  if (c.budget_ppm < 1 || c.budget_ppm > kMillion - 1) throw std::invalid_argument("saturation curve: budget_ppm must be in [1, 999999]");
  if (c.min_requests < 1 || c.min_requests > kMaxMinRequests)
    throw std::invalid_argument("saturation curve: min_requests must be in [1, 2^31 - 1]");
  if (!std::isfinite(c.slo_ms) || c.slo_ms < 0.0) throw std::invalid_argument("saturation curve: slo_ms must be finite and >= 0");
  if (c.group_cap < 1 || c.group_cap > 65536) throw std::invalid_argument("saturation curve: group_cap must be in [1, 65536]");
  if (c.span_cap < 1) throw std::invalid_argument("saturation curve: span_cap must be >= 1");
  if (c.n_buffers < 1 || c.n_buffers > 64) throw std::invalid_argument("saturation curve: n_buffers out of range");
  if (device_bytes(c) > (uint64_t(1) << 31)) throw std::invalid_argument("saturation curve: the ring needs more than 2 GiB");
  if ((uint64_t)layout(c.group_cap).words * 4 > (uint64_t(1) << 31))
    throw std::invalid_argument("saturation curve: a result block needs more than 2 GiB");
  if (c.ring_records_max < 1 || c.ring_records_max > loadsli::default_ring_records_max(c.bins, c.bin_us))
    throw std::invalid_argument("saturation curve: ring_records_max * bins * bin_us must be in [1, 2^53], ring_records_max <= 2^31 - 1");
  if (c.curve_records_max < 1 || c.curve_records_max > kMaxCurveRecords)
    throw std::invalid_argument("saturation curve: curve_records_max must be in [1, 2^40]");
}

using mislo::Range;
inline size_t plan_ranges(const std::vector<Range>& ranges, int span_cap) {
  return mislo::plan_ranges(ranges, span_cap, "saturation curve");
}

inline void check_step(int64_t cut_ns, int n_groups, int group_cap) {
  if (cut_ns <= 0) throw std::invalid_argument("saturation curve step: cut_ns must be > 0");
  if (n_groups < 0 || n_groups > group_cap) throw std::invalid_argument("saturation curve step: n_groups out of range");
}

// The ring's bound: the load tracker's, with this tracker's message.
class RingPopulation {
 public:
  RingPopulation(uint32_t bins, int64_t max) : held_(bins, max), max_(max) {}
  int64_t after(int64_t q_hi, size_t n) const { return held_.after(q_hi, n); }
  void check(int64_t q_hi, size_t n) const {
    if (after(q_hi, n) > max_) throw std::invalid_argument("saturation curve step: the ring would hold more than ring_records_max spans");
  }
  void take(int64_t q_hi, size_t n) { held_.take(q_hi, n); }

 private:
  onset::Population held_;
  int64_t max_;
};

// The curve's bound: (epoch of the step's q_hi, spans offered); a step is refused, before anything
// changes, when the current epoch and the two before it would have been offered more than `max` spans.
class CurvePopulation {
 public:
  CurvePopulation(int64_t epoch_bins, int64_t max) : epoch_bins_(epoch_bins), max_(max) {}
  int64_t after(int64_t q_hi, size_t n) const {
    const int64_t x = epoch_of(q_hi, epoch_bins_);
    int64_t sum = (int64_t)n;
    for (const auto& e : held_)
      if (e.first >= x - 2) sum += e.second;
    return sum;
  }
  void check(int64_t q_hi, size_t n) const {
    if (after(q_hi, n) > max_) throw std::invalid_argument("saturation curve step: the curve would hold more than curve_records_max spans");
  }
  void take(int64_t q_hi, size_t n) {
    const int64_t x = epoch_of(q_hi, epoch_bins_);
    while (!held_.empty() && held_.front().first < x - 2) held_.pop_front();
    if (!n) return;
    if (!held_.empty() && held_.back().first == x)
      held_.back().second += (int64_t)n;
    else
      held_.emplace_back(x, (int64_t)n);
  }
  size_t epochs() const { return held_.size(); }

 private:
  int64_t epoch_bins_, max_;
  std::deque<std::pair<int64_t, int64_t>> held_;  // (epoch, spans offered), epoch ascending
};

}  // namespace satcurve
}  // namespace mislo
