// Host side of the TTFT phase split tracker (retrsli.h) that needs no device: the unit conversions, the
// breach-phase cell, the verdict, the LDS table's key, the configuration and argument checks and the
// result block's layout. Plain C++ (no HIP header), so it builds and runs on its own under the host
// sanitizers (tests/native/retrsli_host_check.cpp); the kernels use the same helpers.
// pipeline/retrsli.py carries the same constants and rules in numpy. Everything after the two
// conversions of a record's float32 times is in integers.
//
// Every product of the verdict fits 64 bits: validate() keeps span_cap * windows < 2^32, so every
// count over the horizon (each cell, their sum n, B, M, R and sli) is < 2^32, and every ppm value
// (budget, coverage, dominance, and the scale 10^6 itself) is <= 10^6 < 2^20. Each side of each compare
// is one count times one ppm value, so it is < 2^32 * 2^20 = 2^52 (the host check verifies the compares
// against unsigned __int128 at counts of 2^32 - 1 and ppm values of 10^6).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <stdexcept>
#include <utility>
#include <vector>

#include "decodesli_host.h"  // bucket_of, lower, representative, kK, kPerLane, kRowLanes: the histograms' rule
#include "errsli_host.h"     // budget_ppm: the error budget of an SLO target, in millionths
#include "slisketch_host.h"  // rank_of, quantile_permille, kQuantiles, kEmpty
#include "steplane_host.h"  // Range, plan_ranges, kSpanBytes

namespace mislo {
namespace retrsli {

using slisketch::kEmpty;
using slisketch::kQuantiles;

constexpr int kK = decodesli::kK;                // buckets of each histogram (retrieval time, model time)
constexpr int kPerLane = decodesli::kPerLane;
constexpr int kRowLanes = decodesli::kRowLanes;
constexpr double kUnitsPerMs = 100.0;            // 10 us, decode.hip's kAppUnitsPerMs
constexpr uint32_t kUnitMax = (1u << 24) - 1u;   // a time in units, clamped: the bucket rule's range
constexpr float kRetrMaxMs = 1e7f;               // decode.hip k_decode_spans: 0 < retr_ms < 1e7 is a breakdown
constexpr uint32_t kSpanNoSli = 2u;              // collector/records.py SPAN_NO_SLI
constexpr uint32_t kSpanStart = 8u;              // collector/records.py SPAN_START
constexpr int kCells = 6;                        // ok ok_slow_retrieval model model_slow_retrieval retrieval combined
constexpr int kCellStride = 8;                   // a service's counters: the six cells, sli, one spare word
constexpr int kSliWord = 6;
constexpr int kStates = 5;                       // unknown ok retrieval_bound model_bound mixed
constexpr uint64_t kPpm = 1000000ull;
constexpr int kLdsBits = 10;
constexpr int kLdsSlots = 1 << kLdsBits;         // the observe kernel's per-workgroup table (16 B a slot, 16 KB)
constexpr int kLdsProbes = onset::kLdsProbes;    // LDS probes before an add goes to global memory itself

enum Cell { kOk = 0, kOkSlowRetrieval = 1, kModel = 2, kModelSlowRetrieval = 3, kRetrieval = 4, kCombined = 5 };
enum State { kUnknown = 0, kStateOk = 1, kRetrievalBound = 2, kModelBound = 3, kMixed = 4 };

// per-step statistics (uint32 each), pipeline/retrsli.py STATS in the same order
enum Stat {
  kObserved = 0,     // records in the histograms, the cells and the sums
  kOutOfGroup = 1,   // group_id >= n_groups
  kInvalid = 2,      // ttft NaN or negative
  kNoBreakdown = 3,  // a valid record without a retrieval time
  kExtra = 4,        // observed records that carry SPAN_NO_SLI: a breakdown that arrived after the first record
  kExceedsTtft = 5,  // observed records whose retrieval time is above their TTFT
  kStats = 8
};

// A record's time in units of 10 us: rint (half to even, np.rint) of the float32 value times 100 in
// double, clamped. A negative or NaN value (never a record's: the checks come first) gives 0.
MISLO_SK_HD inline uint32_t units_of_ms(float ms) {
  const double x = rint((double)ms * kUnitsPerMs);
  if (!(x >= 0.0)) return 0u;
  return x >= (double)kUnitMax ? kUnitMax : (uint32_t)x;
}
// retrieval's own budget in units: the same expression on the flag's double, clamped to [1, 2^24 - 1]
inline uint32_t budget_units(double budget_ms) {
  const double x = rint(budget_ms * kUnitsPerMs);
  if (!(x >= 1.0)) return 1u;
  return x >= (double)kUnitMax ? kUnitMax : (uint32_t)x;
}
// the model time: TTFT minus retrieval, 0 where retrieval is the larger
MISLO_SK_HD inline uint32_t model_units(uint32_t t, uint32_t r) { return t > r ? t - r : 0u; }

// The breach-phase cell of an observed record: tb = ttft_ms > slo_ms (float32, the caller's compare), r its
// retrieval time and m its model time in units. Without a TTFT breach: ok, or ok with a slow retrieval.
// With one: the model alone breaches (m > slo_u) with or without a slow retrieval; else retrieval is over
// its budget (the model alone is inside the SLO); else each phase is within its limit and the sum is over.
MISLO_SK_HD inline uint32_t cell_of(bool tb, uint32_t r, uint32_t m, uint32_t slo_u, uint32_t budget_u) {
  const bool rb = r > budget_u;
  if (!tb) return rb ? kOkSlowRetrieval : kOk;
  if (m > slo_u) return rb ? kModelSlowRetrieval : kModel;
  return rb ? kRetrieval : kCombined;
}

struct Thresholds {
  uint32_t min_requests = 200;     // fewest observed requests over the horizon for a verdict
  uint32_t coverage_ppm = 500000;  // fewest observed requests as a share of the SLI records
  uint32_t budget_ppm = 10000;     // the TTFT SLO's error budget
  uint32_t dominance_ppm = 667000; // the share of the breaches one phase needs to be named
};

// The verdict over a service's rolling cells c[6] and its rolling SLI count (the header's comment has the
// widths). dominance_ppm > 500,000 keeps retrieval_bound and model_bound apart.
MISLO_SK_HD inline uint32_t state_of(const uint32_t* c, uint32_t sli, const Thresholds& th) {
  const uint64_t n = (uint64_t)c[0] + c[1] + c[2] + c[3] + c[4] + c[5];
  if (n < (uint64_t)th.min_requests || n * kPpm < (uint64_t)th.coverage_ppm * (uint64_t)sli) return kUnknown;
  const uint64_t M = (uint64_t)c[kModel] + c[kModelSlowRetrieval], R = c[kRetrieval], B = M + R + c[kCombined];
  if (B * kPpm <= (uint64_t)th.budget_ppm * n) return kStateOk;
  if (R * kPpm >= (uint64_t)th.dominance_ppm * B) return kRetrievalBound;
  if (M * kPpm >= (uint64_t)th.dominance_ppm * B) return kModelBound;
  return kMixed;
}

// consecutive steps with the same verdict, this one included; saturates
MISLO_SK_HD inline uint32_t age_of(uint32_t state, uint32_t prev_state, uint32_t prev_age) {
  if (state != prev_state) return 1u;
  return prev_age == 0xffffffffu ? prev_age : prev_age + 1u;
}

// The LDS table's key of (service, what): what = a retrieval bucket, kK + a model bucket, 2 kK + a cell,
// then the two sums and the SLI count. Never 0.
constexpr uint32_t kWhatModel = kK;
constexpr uint32_t kWhatCell = 2 * kK;
constexpr uint32_t kWhatSumR = kWhatCell + kCells;
constexpr uint32_t kWhatSumT = kWhatSumR + 1;
constexpr uint32_t kWhatSli = kWhatSumT + 1;
MISLO_SK_HD inline uint64_t lds_key(uint32_t g, uint32_t what) { return ((uint64_t)(g + 1u) << 16) | (uint64_t)what; }
MISLO_SK_HD inline uint32_t lds_group(uint64_t key) { return (uint32_t)(key >> 16) - 1u; }
MISLO_SK_HD inline uint32_t lds_what(uint64_t key) { return (uint32_t)key & 0xffffu; }
MISLO_SK_HD inline uint32_t lds_hash(uint64_t key) { return (uint32_t)((key * 0x9e3779b97f4a7c15ull) >> (64 - kLdsBits)); }

struct Config {
  int device = 0;
  int span_cap = 16384;                // span records per step
  int group_cap = 64;                  // services (incident groups), at most
  int windows = 150;                   // the rolling horizon W, in steps
  int n_buffers = 3;                   // steps whose results stay readable
  double slo_ms = 800.0;               // a TTFT above it (float32 compare) is a TTFT breach
  double retrieval_budget_ms = 200.0;  // a retrieval time above budget_units() of it is slow
  int64_t budget_ppm = 10000;          // the TTFT SLO's error budget, in millionths (errsli::budget_ppm of the target)
  int64_t coverage_ppm = 500000;
  int64_t dominance_ppm = 667000;
  int64_t min_requests = 200;
  bool lds = true;                     // pre-aggregate every workgroup's records in LDS (off: the measurement's other side)
};

inline Thresholds thresholds(const Config& c) {
  Thresholds t;
  t.min_requests = (uint32_t)c.min_requests;
  t.coverage_ppm = (uint32_t)c.coverage_ppm;
  t.budget_ppm = (uint32_t)c.budget_ppm;
  t.dominance_ppm = (uint32_t)c.dominance_ppm;
  return t;
}

// words of device state per service and row of the horizon: two histograms, the counters, two 64-bit sums
constexpr size_t kStateWords = 2 * (size_t)kK + kCellStride + 4;

// The result block of one step, in uint32 words, every array on 16 bytes, G = group_cap:
//   cells[G][8]  cells_roll[G][8]  sum_r[G][2]  sum_t[G][2]  sum_r_roll[G][2]  sum_t_roll[G][2]  sli[G]  sli_roll[G]
//   q_r_win[G][4]  q_r_roll[G][4]  q_m_win[G][4]  q_m_roll[G][4]  state[G]  age[G]  stats[8]
// cells hold six counts and two zero words; sums are (low, high); q_* are bucket indices (kEmpty for a
// service without a record).
struct Layout {
  size_t cells = 0, cells_roll = 0, sum_r = 0, sum_t = 0, sum_r_roll = 0, sum_t_roll = 0, sli = 0, sli_roll = 0, q_r_win = 0,
         q_r_roll = 0, q_m_win = 0, q_m_roll = 0, state = 0, age = 0, stats = 0, words = 0;
};
inline Layout layout(int group_cap) {
  const size_t g = (size_t)group_cap, pair = (2 * g + 3) & ~size_t(3), one = (g + 3) & ~size_t(3), q = (size_t)kQuantiles * g;
  Layout l;
  l.cells = 0;
  l.cells_roll = l.cells + kCellStride * g;
  l.sum_r = l.cells_roll + kCellStride * g;
  l.sum_t = l.sum_r + pair;
  l.sum_r_roll = l.sum_t + pair;
  l.sum_t_roll = l.sum_r_roll + pair;
  l.sli = l.sum_t_roll + pair;
  l.sli_roll = l.sli + one;
  l.q_r_win = l.sli_roll + one;
  l.q_r_roll = l.q_r_win + q;
  l.q_m_win = l.q_r_roll + q;
  l.q_m_roll = l.q_m_win + q;
  l.state = l.q_m_roll + q;
  l.age = l.state + one;
  l.stats = l.age + one;
  l.words = l.stats + kStats;
  return l;
}

inline uint64_t block_bytes(int group_cap) { return (uint64_t)layout(group_cap).words * 4; }

// spans, the horizon's rows + the rolling row + the step's row, the verdict and its age, the block
inline uint64_t device_bytes(const Config& c) {
  return (uint64_t)c.span_cap * kSpanBytes + ((uint64_t)c.windows + 2) * (uint64_t)c.group_cap * kStateWords * 4 +
         (uint64_t)c.group_cap * 2 * 4 + block_bytes(c.group_cap);
}

// What an image of this tracker's state depends on (steplane_host.h lane::Fingerprint): every field that
// shapes the state or its meaning, and the layout's constants; not device, n_buffers, span_cap or lds.
inline lane::Fingerprint fingerprint(const Config& c) {
  using lane::field;
  using lane::real_field;
  lane::Fingerprint f;
  f.kind = lane::kRetrSli;
  f.fields = {field("group_cap", c.group_cap),
              field("windows", c.windows),
              real_field("slo_ms", c.slo_ms),
              real_field("retrieval_budget_ms", c.retrieval_budget_ms),
              field("budget_ppm", c.budget_ppm),
              field("coverage_ppm", c.coverage_ppm),
              field("dominance_ppm", c.dominance_ppm),
              field("min_requests", c.min_requests),
              field("buckets", kK),
              field("cell_stride", kCellStride)};
  return f;
}

inline void validate(const Config& c) {
  if (c.windows < 1 || c.windows > 4096) throw std::invalid_argument("retrieval sli: windows must be in [1, 4096]");
  if (c.group_cap < 1 || c.group_cap > 65536) throw std::invalid_argument("retrieval sli: group_cap must be in [1, 65536]");
  if (c.span_cap < 1) throw std::invalid_argument("retrieval sli: span_cap must be >= 1");
  if ((uint64_t)c.span_cap * (uint64_t)c.windows >= (uint64_t(1) << 32))
    throw std::invalid_argument("retrieval sli: span_cap * windows must stay below 2^32 (a rolling counter would wrap)");
  if (c.n_buffers < 1 || c.n_buffers > 64) throw std::invalid_argument("retrieval sli: n_buffers out of range");
  if (!std::isfinite(c.slo_ms) || c.slo_ms < 0.0) throw std::invalid_argument("retrieval sli: slo_ms must be finite and >= 0");
  if (!std::isfinite(c.retrieval_budget_ms) || !(c.retrieval_budget_ms > 0.0))
    throw std::invalid_argument("retrieval sli: retrieval_budget_ms must be finite and > 0");
  if (c.budget_ppm < 1 || c.budget_ppm > 999999) throw std::invalid_argument("retrieval sli: budget_ppm must be in [1, 999999]");
  if (c.coverage_ppm < 0 || c.coverage_ppm > 1000000)
    throw std::invalid_argument("retrieval sli: coverage_ppm must be in [0, 1000000]");
  if (c.dominance_ppm <= 500000 || c.dominance_ppm > 1000000)
    throw std::invalid_argument("retrieval sli: dominance_ppm must be in (500000, 1000000]");
  if (c.min_requests < 1 || c.min_requests > (int64_t)0x7fffffffll)
    throw std::invalid_argument("retrieval sli: min_requests must be in [1, 2^31 - 1]");
  if (device_bytes(c) > (uint64_t(1) << 31)) throw std::invalid_argument("retrieval sli: the horizon needs more than 2 GiB");
  if (block_bytes(c.group_cap) > (uint64_t(1) << 31))
    throw std::invalid_argument("retrieval sli: a result block needs more than 2 GiB");
}

using mislo::Range;
inline size_t plan_ranges(const std::vector<Range>& ranges, int span_cap) {
  return mislo::plan_ranges(ranges, span_cap, "retrieval sli");
}

inline void check_step(int n_groups, int group_cap) {
  if (n_groups < 0 || n_groups > group_cap) throw std::invalid_argument("retrieval sli step: n_groups out of range");
}

}  // namespace retrsli
}  // namespace mislo
