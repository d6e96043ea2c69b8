// Host side of the decode-phase SLI tracker (decodesli.h) that needs no device: the TPOT field of
// a span's flags, the bucket rule, the 2x2 table's cell, the LDS table's key, the configuration and
// argument checks and the result block's layout. Plain C++ (no HIP header), so it builds and runs on
// its own under the host sanitizers (tests/native/decodesli_host_check.cpp); the kernels use the same
// helpers. pipeline/decodesli.py carries the same constants and rules in numpy.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <stdexcept>
#include <utility>
#include <vector>

#include "onset_host.h"      // lds_hash, kLdsSlots, kLdsProbes: the observe kernel's table is onset's
#include "slisketch_host.h"  // rank_of, quantile_permille, kQuantiles, kEmpty
#include "steplane_host.h"  // Range, plan_ranges, kSpanBytes

namespace mislo {
namespace decodesli {

using slisketch::kEmpty;
using slisketch::kQuantiles;

constexpr uint32_t kTpotShift = 8;               // Span::flags bits 8-31: TPOT in microseconds, 0 = none
constexpr uint32_t kTpotMax = (1u << 24) - 1u;   // collector/records.py SPAN_TPOT_MAX
constexpr uint32_t kSkipMask = 4u | 8u;          // first-token and start records: not a finished request
constexpr int kK = 336;                          // buckets: 16 exact ones, then 16 per octave up to 2^24
constexpr int kPerLane = 6;                      // 56 lanes x 6 consecutive buckets
constexpr int kRowLanes = kK / kPerLane;
constexpr int kCells = 4;                        // the table (TTFT breach, TPOT breach): cell = tb + 2 db
constexpr int kLdsSlots = onset::kLdsSlots;
constexpr int kLdsProbes = onset::kLdsProbes;
static_assert(kRowLanes * kPerLane == kK && kRowLanes <= 64 && kK % 4 == 0, "a row is 6 buckets per lane of one wave");

// per-step statistics (uint32 each), pipeline/decodesli.py STATS in the same order
enum Stat {
  kObserved = 0,    // finished requests in the histograms and the table
  kInvalid = 1,     // a TPOT and a group, ttft NaN or negative
  kOutOfGroup = 2,  // a TPOT, group_id >= n_groups
  kNoDecode = 3,    // a finished request without a TPOT (whatever its group)
  kStats = 8
};

MISLO_SK_HD inline uint32_t tpot_of(uint32_t flags) { return flags >> kTpotShift; }

// The bucket of a TPOT u in 1 .. 2^24 - 1 microseconds, read off the integer: exact below 16, then
// the octave and the top 4 bits below the leading one (16 linear sub-buckets per octave).
MISLO_SK_HD inline uint32_t bucket_of(uint32_t u) {
  if (u < 16u) return u;
  const uint32_t e = 31u - (uint32_t)__builtin_clz(u);
  return 16u * (e - 3u) + ((u >> (e - 4u)) & 15u);
}
// the smallest u of bucket b (b = kK: one past the last bucket's largest)
MISLO_SK_HD inline uint32_t lower(uint32_t b) { return b < 16u ? b : (16u + (b & 15u)) << ((b >> 4) - 1u); }
// The microseconds a bucket stands for: the midpoint of the integers it holds. Exact below 16; a
// bucket above holds lower / 16 integers, so it lies within v / 32 of every v in it.
inline double representative(uint32_t b) { return 0.5 * ((double)lower(b) + (double)(lower(b + 1u) - 1u)); }

// the SLO in the record's unit: round half up, clamped to the field's range
inline uint32_t tpot_slo_us(double tpot_slo_ms) {
  const double x = tpot_slo_ms * 1000.0 + 0.5;
  if (!(x >= 1.0)) return 1u;
  return x >= (double)kTpotMax ? kTpotMax : (uint32_t)x;
}

MISLO_SK_HD inline uint32_t cell_of(float ttft_ms, float slo_ms, uint32_t u, uint32_t slo_us) {
  return (ttft_ms > slo_ms ? 1u : 0u) + (u > slo_us ? 2u : 0u);
}

// The LDS table's key of (service, what): what = a bucket, kK + a cell, or kSum. Never 0.
constexpr uint32_t kSum = kK + kCells;
MISLO_SK_HD inline uint64_t lds_key(uint32_t g, uint32_t what) { return ((uint64_t)(g + 1u) << 16) | (uint64_t)what; }
MISLO_SK_HD inline uint32_t lds_group(uint64_t key) { return (uint32_t)(key >> 16) - 1u; }
MISLO_SK_HD inline uint32_t lds_what(uint64_t key) { return (uint32_t)key & 0xffffu; }

struct Config {
  int device = 0;
  int span_cap = 16384;        // span records per step
  int group_cap = 64;          // services (incident groups), at most
  int windows = 150;           // the rolling horizon W, in steps
  int n_buffers = 3;           // steps whose results stay readable
  double slo_ms = 800.0;       // a TTFT above it (float32 compare) is a TTFT breach
  double tpot_slo_ms = 100.0;  // a TPOT above tpot_slo_us() of it is a TPOT breach
  bool lds = true;             // pre-aggregate every workgroup's records in LDS (off: the measurement's other side)
};

// words of device state per service and row of the horizon: the histogram, the table, the 64-bit sum
constexpr size_t kStateWords = (size_t)kK + kCells + 2;

// The result block of one step, in uint32 words, every array on 16 bytes, G = group_cap:
//   cells[G][4]  cells_roll[G][4]  sum_us[G][2]  sum_us_roll[G][2]  q_win[G][4]  q_roll[G][4]  stats[8]
// sums are (low, high); q_* are bucket indices (kEmpty for a service without a record).
struct Layout {
  size_t cells = 0, cells_roll = 0, sum = 0, sum_roll = 0, q_win = 0, q_roll = 0, stats = 0, words = 0;
};
inline Layout layout(int group_cap) {
  const size_t g = (size_t)group_cap, pair = (2 * g + 3) & ~size_t(3);
  Layout l;
  l.cells = 0;
  l.cells_roll = l.cells + kCells * g;
  l.sum = l.cells_roll + kCells * g;
  l.sum_roll = l.sum + pair;
  l.q_win = l.sum_roll + pair;
  l.q_roll = l.q_win + (size_t)kQuantiles * g;
  l.stats = l.q_roll + (size_t)kQuantiles * g;
  l.words = l.stats + kStats;
  return l;
}

// spans, the horizon's rows + the rolling row + the step's row, the block
inline uint64_t device_bytes(const Config& c) {
  return (uint64_t)c.span_cap * kSpanBytes + ((uint64_t)c.windows + 2) * (uint64_t)c.group_cap * kStateWords * 4 +
         (uint64_t)layout(c.group_cap).words * 4;
}

// What an image of this tracker's state depends on (steplane_host.h lane::Fingerprint): every field that
// shapes the state or its meaning, and the layout's constants; not device, n_buffers, span_cap or lds.
inline lane::Fingerprint fingerprint(const Config& c) {
  using lane::field;
  using lane::real_field;
  lane::Fingerprint f;
  f.kind = lane::kDecodeSli;
  f.fields = {field("group_cap", c.group_cap),
              field("windows", c.windows),
              real_field("slo_ms", c.slo_ms),
              real_field("tpot_slo_ms", c.tpot_slo_ms),
              field("buckets", kK)};
  return f;
}

inline void validate(const Config& c) {
  if (c.windows < 1 || c.windows > 4096) throw std::invalid_argument("decode sli: windows must be in [1, 4096]");
  if (c.group_cap < 1 || c.group_cap > 65536) throw std::invalid_argument("decode sli: group_cap must be in [1, 65536]");
  if (c.span_cap < 1) throw std::invalid_argument("decode sli: span_cap must be >= 1");
  if ((uint64_t)c.span_cap * (uint64_t)c.windows >= (uint64_t(1) << 32))
    throw std::invalid_argument("decode sli: span_cap * windows must stay below 2^32 (a rolling counter would wrap)");
  if (c.n_buffers < 1 || c.n_buffers > 64) throw std::invalid_argument("decode sli: n_buffers out of range");
  if (!std::isfinite(c.slo_ms) || c.slo_ms < 0.0) throw std::invalid_argument("decode sli: slo_ms must be finite and >= 0");
  if (!std::isfinite(c.tpot_slo_ms) || !(c.tpot_slo_ms > 0.0))
    throw std::invalid_argument("decode sli: tpot_slo_ms must be finite and > 0");
  if (device_bytes(c) > (uint64_t(1) << 31)) throw std::invalid_argument("decode sli: the horizon needs more than 2 GiB");
}

using mislo::Range;
inline size_t plan_ranges(const std::vector<Range>& ranges, int span_cap) {
  return mislo::plan_ranges(ranges, span_cap, "decode sli");
}

inline void check_step(int n_groups, int group_cap) {
  if (n_groups < 0 || n_groups > group_cap) throw std::invalid_argument("decode sli step: n_groups out of range");
}

}  // namespace decodesli
}  // namespace mislo
