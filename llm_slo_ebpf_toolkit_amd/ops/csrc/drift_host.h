// Host side of the TTFT drift tracker (drift.h) that needs no device: the decision arithmetic, the
// LDS table's key, the configuration and argument checks and the result block's layout. Plain C++
// (no HIP header), so it builds and runs on its own under the host sanitizers
// (tests/native/drift_host_check.cpp); the kernels use the same helpers. The bucket rule, the rank
// rule and the row stride are the TTFT sketch's (slisketch_host.h). pipeline/drift.py carries the
// same rules in numpy; docs/TTFT_DRIFT.md is the contract.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <stdexcept>
#include <utility>
#include <vector>

#include "onset_host.h"      // lds_hash, kLdsSlots, kLdsProbes: the observe kernel's table is onset's
#include "slisketch_host.h"  // bucket_of_bits, rank_of, quantile_permille, kK, kRowStride, kPerLane, kEmpty
#include "steplane_host.h"  // Range, plan_ranges, kSpanBytes

namespace mislo {
namespace drift {

using slisketch::kEmpty;
using slisketch::kK;
using slisketch::kPerLane;
using slisketch::kQuantiles;
using slisketch::kRowStride;

constexpr int kRowLanes = kRowStride / kPerLane;  // lanes of the roll kernel's wave that own buckets
constexpr int kLdsSlots = onset::kLdsSlots;
constexpr int kLdsProbes = onset::kLdsProbes;
constexpr int kP50 = 0, kP90 = 1;  // the quantiles of slisketch::quantile_permille the shift condition reads
static_assert(kRowLanes * kPerLane == kRowStride && kRowLanes <= 64 && kK <= kRowStride, "a row is one wave");
static_assert(kK <= 512, "the wave reduction packs a bucket into 9 bits");

// a service's published state, a bit set
constexpr uint32_t kSlow = 1u;     // recent is significantly and materially slower than the baseline
constexpr uint32_t kFast = 2u;     // the mirror image
constexpr uint32_t kWarming = 4u;  // too few records or baseline windows to decide: no direction bit
constexpr uint32_t kRebased = 8u;  // hold reached hold_max in this step: the baseline was dropped

// per-step statistics (uint32 each), pipeline/drift.py STATS in the same order
enum Stat {
  kObserved = 0,    // records in the window's histograms
  kInvalid = 1,     // counted by the engine, ttft NaN or negative
  kOutOfGroup = 2,  // SLI records with group_id >= n_groups
  kAdmitted = 3,    // rows whose window left the gap and entered the baseline
  kWithheld = 4,    // rows whose non-empty window left the gap while the service was slow
  kRebasedRows = 5, // rows whose baseline was dropped
  kStats = 8
};

// crit_q = round(c^2 * 2^32), saturating
inline uint64_t crit_q(double c2) {
  const double x = std::floor(c2 * 4294967296.0 + 0.5);
  if (!(x >= 0.0)) return 0u;
  return x >= 18446744073709551616.0 ? ~uint64_t(0) : (uint64_t)x;
}

struct Thresholds {
  uint64_t crit_q = uint64_t(4) << 32;
  uint32_t min_shift = 2;
  uint32_t min_recent = 30, min_base = 100, min_base_windows = 10;
};

// One direction of the decision: `num` is that direction's numerator, (q50, q90) the quantile buckets
// of the row that should be the slower one, (o50, o90) the other's. n_r, n_b >= 1 and
// num <= n_r * n_b < 2^44 (validate), so every product stays in 64 bits: Dq <= 2^16, n_e < 2^32.
MISLO_SK_HD inline bool significant(uint64_t num, uint64_t n_r, uint64_t n_b, uint64_t crit) {
  const uint64_t nn = n_r * n_b;
  const uint64_t dq = (num << 16) / nn;
  const uint64_t ne = nn / (n_r + n_b);
  return dq * dq * ne > crit;
}
MISLO_SK_HD inline bool shifted(uint32_t q50, uint32_t q90, uint32_t o50, uint32_t o90, uint32_t s) {
  return (uint64_t)q50 >= (uint64_t)o50 + s || (uint64_t)q90 >= (uint64_t)o90 + s;
}

// The state bits of one service before hold and reset: kWarming alone, or any of kSlow / kFast.
MISLO_SK_HD inline uint32_t decide(uint32_t n_r, uint32_t n_b, uint32_t base_fill, uint64_t slow_num, uint64_t fast_num,
                                   const uint32_t* q_recent, const uint32_t* q_base, const Thresholds& t) {
  if (n_r == 0u || n_b == 0u || n_r < t.min_recent || n_b < t.min_base || base_fill < t.min_base_windows) return kWarming;
  uint32_t st = 0u;
  if (significant(slow_num, n_r, n_b, t.crit_q) && shifted(q_recent[kP50], q_recent[kP90], q_base[kP50], q_base[kP90], t.min_shift))
    st |= kSlow;
  if (significant(fast_num, n_r, n_b, t.crit_q) && shifted(q_base[kP50], q_base[kP90], q_recent[kP50], q_recent[kP90], t.min_shift))
    st |= kFast;
  return st;
}

// The wave reduction's operand: the larger numerator wins, of equal ones the lower bucket.
MISLO_SK_HD inline uint64_t pack_max(uint64_t num, uint32_t bucket) { return (num << 9) | (uint64_t)(511u - bucket); }
MISLO_SK_HD inline uint64_t packed_num(uint64_t key) { return key >> 9; }
MISLO_SK_HD inline uint32_t packed_bucket(uint64_t key) { return 511u - (uint32_t)(key & 511u); }

// The LDS table's key of (service, bucket). Never 0.
MISLO_SK_HD inline uint64_t lds_key(uint32_t g, uint32_t b) { return ((uint64_t)(g + 1u) << 16) | (uint64_t)b; }
MISLO_SK_HD inline uint32_t lds_group(uint64_t key) { return (uint32_t)(key >> 16) - 1u; }
MISLO_SK_HD inline uint32_t lds_bucket(uint64_t key) { return (uint32_t)key & 0xffffu; }

struct Config {
  int device = 0;
  int span_cap = 16384;       // span records per step
  int group_cap = 64;         // services (incident groups), at most
  int recent = 10;            // R: windows of the recent histogram
  int gap = 10;               // L: windows between the recent histogram and the baseline
  int baseline = 300;         // B: calm, non-empty windows of the baseline
  int n_buffers = 3;          // steps whose results stay readable
  double crit = 4.0;          // c^2: Dq^2 n_e above crit_q(c^2) is significant
  int min_shift = 2;          // s: buckets p50 or p90 must have moved
  int64_t min_recent = 30;    // records of the recent row before a decision
  int64_t min_base = 100;     // records of the baseline before a decision
  int min_base_windows = 10;  // windows of the baseline before a decision
  int64_t hold_max = 1200;    // consecutive slow steps after which the baseline is dropped
  bool lds = true;            // pre-aggregate every workgroup's records in LDS (off: the measurement's other side)
};

inline Thresholds thresholds(const Config& c) {
  Thresholds t;
  t.crit_q = crit_q(c.crit);
  t.min_shift = (uint32_t)c.min_shift;
  t.min_recent = (uint32_t)c.min_recent;
  t.min_base = (uint32_t)c.min_base;
  t.min_base_windows = (uint32_t)c.min_base_windows;
  return t;
}

// histogram rows of the state: near[R + L], recent, base, the step's row, base_ring[B]
inline uint64_t state_rows(const Config& c) { return (uint64_t)c.recent + c.gap + c.baseline + 3; }

// The result block of one step, in uint32 words, every array on 16 bytes, G = group_cap:
//   n_win[G] n_recent[G] n_base[G] base_fill[G] q_recent[G][4] q_base[G][4] slow_num[G][2] fast_num[G][2]
//   slow_at[G] fast_at[G] state[G] hold[G] stats[8]
// numerators are (low, high); q_* and *_at are bucket indices (kEmpty: an empty row, a zero numerator).
struct Layout {
  size_t n_win = 0, n_recent = 0, n_base = 0, base_fill = 0, q_recent = 0, q_base = 0, slow_num = 0, fast_num = 0,
         slow_at = 0, fast_at = 0, state = 0, hold = 0, stats = 0, words = 0;
};
inline Layout layout(int group_cap) {
  const size_t g = (size_t)group_cap, one = (g + 3) & ~size_t(3), pair = (2 * g + 3) & ~size_t(3);
  Layout l;
  l.n_win = 0;
  l.n_recent = l.n_win + one;
  l.n_base = l.n_recent + one;
  l.base_fill = l.n_base + one;
  l.q_recent = l.base_fill + one;
  l.q_base = l.q_recent + (size_t)kQuantiles * g;
  l.slow_num = l.q_base + (size_t)kQuantiles * g;
  l.fast_num = l.slow_num + pair;
  l.slow_at = l.fast_num + pair;
  l.fast_at = l.slow_at + one;
  l.state = l.fast_at + one;
  l.hold = l.state + one;
  l.stats = l.hold + one;
  l.words = l.stats + kStats;
  return l;
}

// the histogram rows, the spans, the block
inline uint64_t device_bytes(const Config& c) {
  return state_rows(c) * (uint64_t)c.group_cap * (uint64_t)kRowStride * 4 + (uint64_t)c.span_cap * kSpanBytes +
         (uint64_t)layout(c.group_cap).words * 4;
}

// What an image of this tracker's state depends on (steplane_host.h lane::Fingerprint): every field that
// shapes the state or its meaning, and the layout's constants; not device, n_buffers, span_cap or lds.
inline lane::Fingerprint fingerprint(const Config& c) {
  using lane::field;
  using lane::real_field;
  lane::Fingerprint f;
  f.kind = lane::kDrift;
  f.fields = {field("group_cap", c.group_cap),
              field("recent", c.recent),
              field("gap", c.gap),
              field("baseline", c.baseline),
              real_field("crit", c.crit),
              field("min_shift", c.min_shift),
              field("min_recent", c.min_recent),
              field("min_base", c.min_base),
              field("min_base_windows", c.min_base_windows),
              field("hold_max", c.hold_max),
              field("row_stride", kRowStride)};
  return f;
}

inline void validate(const Config& c) {
  if (c.recent < 1 || c.recent > 1024) throw std::invalid_argument("ttft drift: recent windows must be in [1, 1024]");
  if (c.gap < 1 || c.gap > 1024) throw std::invalid_argument("ttft drift: gap windows must be in [1, 1024]");
  if (c.baseline < 1 || c.baseline > 4096) throw std::invalid_argument("ttft drift: baseline windows must be in [1, 4096]");
  if (c.group_cap < 1 || c.group_cap > 65536) throw std::invalid_argument("ttft drift: group_cap must be in [1, 65536]");
  if (c.span_cap < 1) throw std::invalid_argument("ttft drift: span_cap must be >= 1");
  // span_cap < 2^22 first, so the product below cannot itself wrap
  if ((uint64_t)c.span_cap >= (uint64_t(1) << 22) ||
      (uint64_t)c.span_cap * (uint64_t)c.span_cap * (uint64_t)c.recent * (uint64_t)c.baseline >= (uint64_t(1) << 44))
    throw std::invalid_argument("ttft drift: span_cap^2 * recent * baseline must stay below 2^44 (slow_num << 16 would wrap)");
  if (c.n_buffers < 1 || c.n_buffers > 64) throw std::invalid_argument("ttft drift: n_buffers out of range");
  if (!std::isfinite(c.crit) || !(c.crit > 0.0)) throw std::invalid_argument("ttft drift: crit must be finite and > 0");
  if (c.min_shift < 0 || c.min_shift > kK - 1) throw std::invalid_argument("ttft drift: min_shift must be in [0, 385]");
  if (c.min_recent < 1 || c.min_recent > 0xffffffffll || c.min_base < 1 || c.min_base > 0xffffffffll || c.min_base_windows < 1)
    throw std::invalid_argument("ttft drift: min_recent, min_base and min_base_windows must be >= 1");
  if (c.hold_max < 1 || c.hold_max > 0xffffffffll) throw std::invalid_argument("ttft drift: hold_max must be >= 1");
  if (device_bytes(c) > (uint64_t(1) << 31)) throw std::invalid_argument("ttft drift: the rings need more than 2 GiB");
}

using mislo::Range;
inline size_t plan_ranges(const std::vector<Range>& ranges, int span_cap) {
  return mislo::plan_ranges(ranges, span_cap, "ttft drift");
}

inline void check_step(int n_groups, int group_cap) {
  if (n_groups < 0 || n_groups > group_cap) throw std::invalid_argument("ttft drift step: n_groups out of range");
}

}  // namespace drift
}  // namespace mislo
