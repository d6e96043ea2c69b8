// Host side of the breach-onset tracker (onset.h) that needs no device: the bin rule and the ring
// slot, the CUSUM's scan operator, the per-service row, the configuration and argument checks, the
// result block's layout and the bound on the ring's population. Plain C++ (no HIP header), so it
// builds and runs on its own under the host sanitizers (tests/native/onset_host_check.cpp); the
// kernels use the same helpers. pipeline/onset.py carries the same constants and rules in numpy.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <deque>
#include <stdexcept>
#include <utility>
#include <vector>

#include "steplane_host.h"  // Range, plan_ranges, kSpanBytes

#if defined(__HIPCC__)
#define MISLO_ON_HD __host__ __device__
#else
#define MISLO_ON_HD
#endif

namespace mislo {
namespace onset {

constexpr int kMinBins = 64;           // one bin a lane of the scan's wave at least
constexpr int kMaxBins = 8192;
constexpr int64_t kMinBinNs = 1000000ll;
constexpr int64_t kMaxBinNs = 60000000000ll;
constexpr int64_t kMillion = 1000000ll;  // the CUSUM counts in millionths of a breach
constexpr int64_t kMaxRingRecords = 2147483647ll;  // 2^31 - 1: a cell's request count cannot carry into its breaches
constexpr int kRowBytes = 64;
constexpr int kRowWords = kRowBytes / 4;
constexpr int kLdsSlots = 256;         // the observe kernel's per-workgroup table (16 B a slot, 4 KB)
constexpr int kLdsProbes = 8;          // LDS probes before a record goes to the ring itself
constexpr int64_t kNoBin = -1;         // q_hi before the first step; onset_q / alarm_q without one

// per-step statistics (uint32 each), pipeline/onset.py STATS in the same order
enum Stat {
  kObserved = 0,    // records of the observed set (the sketch's): the five below are among them or beside them
  kInvalid = 1,     // counted by the engine, ttft NaN or negative
  kOutOfGroup = 2,  // SLI records with group_id >= n_groups
  kNoTime = 3,      // observed, ts_ns <= 0: in no bin
  kFuture = 4,      // observed, bin beyond q_hi: placed in q_hi
  kTooOld = 5,      // observed, bin at or before q_hi - B: placed nowhere
  kStats = 8
};

enum State : uint32_t { kQuiet = 0, kExcursion = 1, kAlarm = 2 };
constexpr uint32_t kClipped = 1u;  // Row::flags bit 0: no zero of S in the ring

// One service (pipeline/onset.py ONSET_ROW).
struct Row {
  uint32_t state, flags;
  int64_t onset_q;  // 1 + the last bin with S == 0 (the ring's oldest bin when clipped), -1 when quiet
  int64_t alarm_q;  // the first bin >= onset_q with S >= h, or -1
  int64_t s_now;    // S at q_hi
  int64_t s_peak;   // its maximum since onset_q
  uint32_t n_exc, b_exc;    // requests and breaches since onset_q
  uint32_t n_ring, b_ring;  // and in the whole ring
  uint32_t pad[2];
};
static_assert(sizeof(Row) == kRowBytes, "an onset row is 64 bytes");

// ---- bins -------------------------------------------------------------------------------------
// the absolute bin of a start time > 0 (a time <= 0 has none)
MISLO_ON_HD inline int64_t bin_of(int64_t ts_ns, int64_t bin_ns) { return ts_ns / bin_ns; }
// the ring slot of a bin (bins: a power of two); two's complement, so bins below 0 have slots too
MISLO_ON_HD inline uint32_t slot_of(int64_t q, uint32_t bins) { return (uint32_t)((uint64_t)q & (uint64_t)(bins - 1u)); }
// the ring's oldest bin
MISLO_ON_HD inline int64_t oldest_bin(int64_t q_hi, uint32_t bins) { return q_hi - (int64_t)bins + 1; }
// q_hi after a step with this cut: it never moves back
MISLO_ON_HD inline int64_t advance(int64_t q_hi, int64_t cut_ns, int64_t bin_ns) {
  const int64_t q = bin_of(cut_ns, bin_ns);
  return q > q_hi ? q : q_hi;
}
// slots the advance clears: the bins (prev, q_hi], all of them from a jump of `bins` on
MISLO_ON_HD inline uint32_t cleared(int64_t prev, int64_t q_hi, uint32_t bins) {
  const int64_t d = q_hi - prev;
  return d >= (int64_t)bins ? bins : (uint32_t)d;
}

enum Place : int { kPlaced = 0, kPlacedFuture = 1, kDroppedOld = 2, kDroppedNoTime = 3 };
// Where an observed record goes: *q is its bin when placed (q_hi for a record ahead of it).
MISLO_ON_HD inline Place place(int64_t ts_ns, int64_t bin_ns, int64_t q_hi, uint32_t bins, int64_t* q) {
  if (ts_ns <= 0) return kDroppedNoTime;
  const int64_t b = bin_of(ts_ns, bin_ns);
  if (b > q_hi) {
    *q = q_hi;
    return kPlacedFuture;
  }
  if (b <= q_hi - (int64_t)bins) return kDroppedOld;
  *q = b;
  return kPlaced;
}

// ---- cell and CUSUM ---------------------------------------------------------------------------
// one u64 per (service, slot): requests in the low word, breaches in the high one
MISLO_ON_HD inline uint64_t cell_add(uint32_t breach) { return ((uint64_t)breach << 32) | 1ull; }
MISLO_ON_HD inline uint32_t cell_n(uint64_t c) { return (uint32_t)c; }
MISLO_ON_HD inline uint32_t cell_b(uint64_t c) { return (uint32_t)(c >> 32); }
// a bin's CUSUM increment: breaches over the reference rate, in millionths
MISLO_ON_HD inline int64_t excess(uint64_t c, int64_t ref_ppm) {
  return (int64_t)cell_b(c) * kMillion - (int64_t)cell_n(c) * ref_ppm;
}

// A run of bins as (sum of x, minimum inclusive prefix capped at 0); with P the prefix sum from the
// ring's oldest bin and M = min(0, min P), S_t = max(0, S_{t-1} + x_t) = P_t - M_t.
struct Run {
  int64_t s, m;
};
MISLO_ON_HD inline Run run_identity() { return Run{0, 0}; }
MISLO_ON_HD inline Run run_of(int64_t x) { return Run{x, x < 0 ? x : 0}; }
// `a` then `b`: associative, not commutative
MISLO_ON_HD inline Run combine(Run a, Run b) {
  const int64_t m = a.s + b.m;
  return Run{a.s + b.s, a.m < m ? a.m : m};
}

// the LDS table's key of (service, slot): never 0; slot < 2^13
MISLO_ON_HD inline uint64_t lds_key(uint32_t g, uint32_t slot) { return ((uint64_t)(g + 1u) << 16) | (uint64_t)slot; }
MISLO_ON_HD inline uint32_t lds_group(uint64_t key) { return (uint32_t)(key >> 16) - 1u; }
MISLO_ON_HD inline uint32_t lds_slot(uint64_t key) { return (uint32_t)key & 0xffffu; }
// the first LDS slot probed: Fibonacci hashing, the top 8 bits
MISLO_ON_HD inline uint32_t lds_hash(uint64_t key) { return (uint32_t)((key * 0x9e3779b97f4a7c15ull) >> 56); }
static_assert(kLdsSlots == 256, "lds_hash yields 8 bits");

struct Config {
  int device = 0;
  int bins = 1024;                  // B: ring bins per service, a power of two
  int64_t bin_ns = 125000000ll;     // a 2 s window over 16 bins
  int64_t ref_ppm = 20000;          // reference breach rate, in millionths: twice the budget of a 99 % SLO
  int64_t alarm = 3;                // excess breaches over the reference rate that count as an alarm
  int span_cap = 16384;             // span records per step
  int group_cap = 64;               // services (incident groups), at most
  int n_buffers = 3;                // steps whose results stay readable
  double slo_ms = 800.0;            // a TTFT above it (float32 compare) is a breach
  int64_t ring_records_max = kMaxRingRecords;  // spans offered by the steps the ring still holds, at most
  bool lds = true;                  // pre-aggregate every workgroup's records in LDS (off: the measurement's other side)
};

// The result block of one step, in uint32 words: rows[group_cap] (16 words each), then stats[8].
struct Layout {
  size_t rows = 0, stats = 0, words = 0;
};
inline Layout layout(int group_cap) {
  Layout l;
  l.rows = 0;
  l.stats = (size_t)group_cap * kRowWords;
  l.words = (l.stats + kStats + 3) & ~size_t(3);
  return l;
}

// spans, the ring, the block
inline uint64_t device_bytes(const Config& c) {
  return (uint64_t)c.span_cap * kSpanBytes + (uint64_t)c.group_cap * (uint64_t)c.bins * 8 +
         (uint64_t)layout(c.group_cap).words * 4;
}

// What an image of this tracker's state depends on (steplane_host.h lane::Fingerprint): every field that
// shapes the state or its meaning, and the layout's constants; not device, n_buffers, span_cap or lds.
inline lane::Fingerprint fingerprint(const Config& c) {
  using lane::field;
  using lane::real_field;
  lane::Fingerprint f;
  f.kind = lane::kOnset;
  f.fields = {field("group_cap", c.group_cap),
              field("bins", c.bins),
              field("bin_ns", c.bin_ns),
              field("ref_ppm", c.ref_ppm),
              field("alarm", c.alarm),
              real_field("slo_ms", c.slo_ms),
              field("ring_records_max", c.ring_records_max)};
  return f;
}

inline void validate(const Config& c) {
  if (c.bins < kMinBins || c.bins > kMaxBins || (c.bins & (c.bins - 1)) != 0)
    throw std::invalid_argument("breach onset: bins must be a power of two in [64, 8192]");
  if (c.bin_ns < kMinBinNs || c.bin_ns > kMaxBinNs)
    throw std::invalid_argument("breach onset: bin_ns must be in [1000000, 60000000000]");
  if (c.ref_ppm < 1 || c.ref_ppm > kMillion - 1) throw std::invalid_argument("breach onset: ref_ppm must be in [1, 999999]");
  if (c.alarm < 1 || c.alarm > kMillion) throw std::invalid_argument("breach onset: alarm must be in [1, 1000000]");
  if (c.group_cap < 1 || c.group_cap > 65536) throw std::invalid_argument("breach onset: group_cap must be in [1, 65536]");
  if (c.span_cap < 1) throw std::invalid_argument("breach onset: span_cap must be >= 1");
  if (c.n_buffers < 1 || c.n_buffers > 64) throw std::invalid_argument("breach onset: n_buffers out of range");
  if (!std::isfinite(c.slo_ms) || c.slo_ms < 0.0) throw std::invalid_argument("breach onset: slo_ms must be finite and >= 0");
  if (device_bytes(c) > (uint64_t(1) << 31)) throw std::invalid_argument("breach onset: the ring needs more than 2 GiB");
  if (c.ring_records_max < 1 || c.ring_records_max > kMaxRingRecords)
    throw std::invalid_argument("breach onset: ring_records_max must be in [1, 2^31 - 1]");
}

using mislo::Range;
inline size_t plan_ranges(const std::vector<Range>& ranges, int span_cap) {
  return mislo::plan_ranges(ranges, span_cap, "breach onset");
}

inline void check_step(int64_t cut_ns, int n_groups, int group_cap) {
  if (cut_ns <= 0) throw std::invalid_argument("breach onset step: cut_ns must be > 0");
  if (n_groups < 0 || n_groups > group_cap) throw std::invalid_argument("breach onset step: n_groups out of range");
}

// The bound that keeps the ring exact: the spans offered by every step whose records may still be
// in the ring. A step's records lie in bins <= its q_hi, so a step with q_hi <= current q_hi - B is
// cleared. Under the bound no cell's requests reach 2^31 and every CUSUM quantity stays below 2^52.
class Population {
 public:
  Population(uint32_t bins, int64_t max) : bins_(bins), max_(max) {}
  // the population after a step of `n` spans at `q_hi`, without taking it
  int64_t after(int64_t q_hi, size_t n) const {
    int64_t sum = (int64_t)n;
    for (const auto& e : held_)
      if (e.first > q_hi - (int64_t)bins_) sum += e.second;
    return sum;
  }
  // throws, changing nothing, when the step would pass the bound
  void check(int64_t q_hi, size_t n) const {
    if (after(q_hi, n) > max_) throw std::invalid_argument("breach onset step: the ring would hold more than ring_records_max spans");
  }
  void take(int64_t q_hi, size_t n) {
    while (!held_.empty() && held_.front().first <= q_hi - (int64_t)bins_) held_.pop_front();
    if (n) held_.emplace_back(q_hi, (int64_t)n);
  }
  size_t steps() const { return held_.size(); }

 private:
  uint32_t bins_;
  int64_t max_;
  std::deque<std::pair<int64_t, int64_t>> held_;  // (q_hi of the step, spans offered), q_hi ascending
};

}  // namespace onset
}  // namespace mislo
