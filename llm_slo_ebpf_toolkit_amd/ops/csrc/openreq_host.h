// Host side of the open-request tracker (openreq.h) that needs no device: the configuration
// and argument checks, the result block's layout and the bookkeeping of the result slots. Plain
// C++ (no HIP header), so it builds and runs on its own under the host sanitizers
// (tests/native/openreq_host_check.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace mislo {
namespace openreq {

constexpr int kMaxProbes = 64;    // linear probes per lookup / insert
constexpr int kLdsGroups = 1024;  // groups whose counters the kernels keep in LDS (decode.hip kSliLds)
constexpr int kSpanBytes = 64;    // collector/records.py SPAN

// entry states; kEmpty doubles as "being inserted by this launch", kDead marks an entry removed
// in this step (the key stays until the step's end, so probe chains stay whole)
enum State : uint32_t { kEmpty = 0, kOpen = 1, kCounted = 2, kResolved = 3, kDead = 4 };

// per-step statistics (uint32 each), pipeline/openreq.py STATS in the same order
enum Stat {
  kDupStart = 0,       // start records of a request already open or counted
  kStartAfterSli = 1,  // start records dropped by a marker (the SLI came first)
  kDroppedFull = 2,    // starts (or surviving entries) that found no slot within kMaxProbes
  kExpired = 3,        // counted requests that never reported within ttl
  kFalseDeadline = 4,  // counted at the deadline, then reported a TTFT within the SLO
  kLiveOpen = 5,
  kLiveCounted = 6,
  kLiveResolved = 7,
  kStarts = 8,         // start records taken
  kResolves = 9,       // counted records looked up
  kMarkerDropped = 10, // markers that found no slot within kMaxProbes
  kStats = 16
};

struct Config {
  int device = 0;
  int64_t cap = 1 << 20;  // table entries, a power of two
  int span_cap = 16384;   // span records per step
  int group_cap = 64;     // incident groups, at most
  int n_buffers = 3;      // steps whose results stay readable
  double slo_ms = 800.0;
  double ttl_ms = 120000.0;
  double reorder_ms = 2000.0;
};

inline int64_t ms_to_ns(double ms) { return (int64_t)std::llround(ms * 1e6); }

inline void validate(const Config& c) {
  if (c.cap < kMaxProbes || c.cap > (int64_t(1) << 28) || (c.cap & (c.cap - 1)) != 0)
    throw std::invalid_argument("open-request table: cap must be a power of two in [64, 2^28]");
  if (c.span_cap <= 0 || c.span_cap > (1 << 24)) throw std::invalid_argument("open-request table: span_cap out of range");
  if (c.group_cap <= 0 || c.group_cap > (1 << 20)) throw std::invalid_argument("open-request table: group_cap out of range");
  if (c.n_buffers < 1 || c.n_buffers > 64) throw std::invalid_argument("open-request table: n_buffers out of range");
  auto ok = [](double ms) { return std::isfinite(ms) && ms > 0.0 && ms < 1e12; };
  if (!ok(c.slo_ms) || !ok(c.ttl_ms) || !ok(c.reorder_ms))
    throw std::invalid_argument("open-request table: slo_ms, ttl_ms and reorder_ms must be positive");
}

// the result block of one step, in uint32 words: dl[group_cap][2], dup[group_cap][3], stats
struct Layout {
  size_t dl = 0, dup = 0, stats = 0, words = 0;
};
inline Layout layout(int group_cap) {
  Layout l;
  l.dl = 0;
  l.dup = l.dl + 2 * (size_t)group_cap;
  l.stats = l.dup + 3 * (size_t)group_cap;
  l.words = (l.stats + kStats + 3) & ~size_t(3);  // whole 16-byte stores
  return l;
}

using Range = std::pair<uintptr_t, size_t>;  // (host address, bytes)

// the span records in `ranges`; throws when they are not whole records or exceed span_cap
inline size_t plan_ranges(const std::vector<Range>& ranges, int span_cap) {
  size_t n = 0;
  for (const Range& r : ranges) {
    if (r.second == 0) continue;
    if (r.first == 0) throw std::invalid_argument("open-request step: null range");
    if (r.second % kSpanBytes) throw std::invalid_argument("open-request step: a range is not whole 64-byte spans");
    if (r.second / kSpanBytes > (size_t)span_cap - n) throw std::invalid_argument("open-request step: more spans than span_cap");
    n += r.second / kSpanBytes;
  }
  return n;
}

inline void check_step(int64_t cut_ns, int64_t prev_cut_ns, int n_groups, int group_cap) {
  if (cut_ns <= 0) throw std::invalid_argument("open-request step: cut_ns must be > 0");
  if (prev_cut_ns < 0 || prev_cut_ns > cut_ns) throw std::invalid_argument("open-request step: prev_cut_ns must be in [0, cut_ns]");
  if (n_groups < 0 || n_groups > group_cap) throw std::invalid_argument("open-request step: n_groups out of range");
}

// Result slots: step i writes slot i % n; its results stay readable until step i + n takes the slot.
class SlotRing {
 public:
  explicit SlotRing(int n) : idx_((size_t)(n > 0 ? n : 1), -1) {}
  int size() const { return (int)idx_.size(); }
  int64_t next() const { return next_; }
  // the slot of the next step (its index is next()); the step it held before is forgotten
  int begin() {
    const int s = (int)(next_ % (int64_t)idx_.size());
    idx_[(size_t)s] = next_++;
    return s;
  }
  bool holds(int64_t i) const { return i >= 0 && i < next_ && idx_[(size_t)(i % (int64_t)idx_.size())] == i; }
  int slot_of(int64_t i) const {
    if (!holds(i))
      throw std::out_of_range("open-request step " + std::to_string(i) + " is not held (only the last " +
                              std::to_string(idx_.size()) + ")");
    return (int)(i % (int64_t)idx_.size());
  }

 private:
  std::vector<int64_t> idx_;
  int64_t next_ = 0;
};

}  // namespace openreq
}  // namespace mislo
