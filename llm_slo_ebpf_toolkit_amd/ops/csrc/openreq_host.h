// Host side of the open-request tracker (openreq.h) that needs no device: the configuration
// and argument checks and the result block's layout (the result slots are steplane_host.h's). Plain
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

#include "steplane_host.h"  // Range, plan_ranges, kSpanBytes

namespace mislo {
namespace openreq {

constexpr int kMaxProbes = 64;    // linear probes per lookup / insert
constexpr int kLdsGroups = 1024;  // groups whose counters the kernels keep in LDS (decode.hip kSliLds)

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

// What an image of this tracker's state depends on (steplane_host.h lane::Fingerprint): every field that
// shapes the state or its meaning, and the layout's constants; not device, n_buffers, span_cap.
inline lane::Fingerprint fingerprint(const Config& c) {
  using lane::field;
  using lane::real_field;
  lane::Fingerprint f;
  f.kind = lane::kOpenReq;
  f.fields = {field("cap", c.cap),
              field("group_cap", c.group_cap),
              real_field("slo_ms", c.slo_ms),
              real_field("ttl_ms", c.ttl_ms),
              real_field("reorder_ms", c.reorder_ms),
              field("max_probes", kMaxProbes)};
  return f;
}

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

using mislo::Range;
inline size_t plan_ranges(const std::vector<Range>& ranges, int span_cap) {
  return mislo::plan_ranges(ranges, span_cap, "open-request");
}

inline void check_step(int64_t cut_ns, int64_t prev_cut_ns, int n_groups, int group_cap) {
  if (cut_ns <= 0) throw std::invalid_argument("open-request step: cut_ns must be > 0");
  if (prev_cut_ns < 0 || prev_cut_ns > cut_ns) throw std::invalid_argument("open-request step: prev_cut_ns must be in [0, cut_ns]");
  if (n_groups < 0 || n_groups > group_cap) throw std::invalid_argument("open-request step: n_groups out of range");
}

using mislo::SlotRing;  // the result slots; "open-request" is its own default name

}  // namespace openreq
}  // namespace mislo
