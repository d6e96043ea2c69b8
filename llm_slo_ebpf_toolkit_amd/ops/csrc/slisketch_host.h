// Host side of the TTFT sketch (slisketch.h) that needs no device: the bucket rule and its
// constants, the configuration and argument checks and the result block's layout. Plain C++ (no
// HIP header), so it builds and runs on its own under the host sanitizers
// (tests/native/slisketch_host_check.cpp); the kernels use the same bucket helpers.
// pipeline/slisketch.py carries the same constants and rules in numpy.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cstring>
#include <stdexcept>
#include <utility>
#include <vector>

#include "steplane_host.h"  // Range, plan_ranges, kSpanBytes

#if defined(__HIPCC__)
#define MISLO_SK_HD __host__ __device__
#else
#define MISLO_SK_HD
#endif

namespace mislo {
namespace slisketch {

// The bucket of a TTFT is read off its float32 image: key = exponent and the top 4 mantissa bits,
// 16 linear sub-buckets per octave, no logarithm -- host and device cannot differ.
constexpr uint32_t kKeyShift = 19;
constexpr uint32_t kLo = (127u - 3u) << 4;  // key of 0.125 ms
constexpr int kNB = 384;                    // 24 octaves: [0.125 ms, 2^21 ms)
constexpr int kK = kNB + 2;                 // + underflow (bucket 0) and overflow (bucket kK - 1)
constexpr int kRowStride = 392;             // words per histogram row: 56 lanes x 7, whole 16-byte units
constexpr int kPerLane = 7;
constexpr float kMaxMs = 2097152.0f;        // 2^21: the overflow bucket's edge, the sum's clamp
constexpr int kEdges = 7;                   // REF's llm_slo_ttft_ms boundaries
constexpr int kLe = kEdges + 1;             // + the +Inf slot
constexpr int kQuantiles = 4;
constexpr uint32_t kEmpty = 0xffffffffu;    // quantile of a group without a record

MISLO_SK_HD inline float le_edge(int j) {
  return j == 0 ? 50.f : j == 1 ? 100.f : j == 2 ? 200.f : j == 3 ? 400.f : j == 4 ? 800.f : j == 5 ? 1200.f : 2000.f;
}
MISLO_SK_HD inline uint32_t quantile_permille(int j) { return j == 0 ? 500u : j == 1 ? 900u : j == 2 ? 950u : 990u; }

// per-step statistics (uint32 each), pipeline/slisketch.py STATS in the same order
enum Stat {
  kObserved = 0,    // records in the histograms
  kInvalid = 1,     // counted by the engine, ttft NaN or negative: in no histogram
  kUnderflow = 2,   // observed, below 0.125 ms (bucket 0)
  kOverflow = 3,    // observed, at or above 2^21 ms (bucket kK - 1)
  kOutOfGroup = 4,  // SLI records with group_id >= n_groups
  kStats = 8
};

// the bucket of a float32's bits (sign masked off: -0.0 is 0)
MISLO_SK_HD inline uint32_t bucket_of_bits(uint32_t bits) {
  const uint32_t key = (bits & 0x7fffffffu) >> kKeyShift;
  if (key < kLo) return 0u;
  if (key >= kLo + (uint32_t)kNB) return (uint32_t)kK - 1u;
  return key - kLo + 1u;
}

// the `le` slot: the first edge with v <= edge (a float32 compare), else +Inf's
MISLO_SK_HD inline int le_slot(float v) {
  for (int j = 0; j < kEdges; ++j)
    if (v <= le_edge(j)) return j;
  return kEdges;
}

// nearest rank of `permille` among n records: max(1, ceil(q * n / 1000))
MISLO_SK_HD inline uint64_t rank_of(uint32_t permille, uint64_t n) {
  const uint64_t r = ((uint64_t)permille * n + 999u) / 1000u;
  return r < 1u ? 1u : r;
}

inline uint32_t bucket_of(float v) {
  uint32_t bits;
  std::memcpy(&bits, &v, 4);
  return bucket_of_bits(bits);
}

// lower edge of bucket b in 1..kNB (and of the overflow bucket at kNB + 1), exact in float32
inline float bucket_lower(int b) {
  const uint32_t bits = (kLo + (uint32_t)(b - 1)) << kKeyShift;
  float f;
  std::memcpy(&f, &bits, 4);
  return f;
}

// The value a bucket stands for: the midpoint of its edges in float64, 0 for the underflow and
// 2^21 for the overflow bucket. A value v >= lo of bucket [lo, lo + w), w <= lo / 16, lies within
// w / 2 <= lo / 32 <= v / 32 of it.
inline double representative(int b) {
  if (b <= 0) return 0.0;
  if (b >= kK - 1) return (double)kMaxMs;
  return 0.5 * ((double)bucket_lower(b) + (double)bucket_lower(b + 1));
}

struct Config {
  int device = 0;
  int span_cap = 16384;  // span records per step
  int group_cap = 64;    // services (incident groups), at most
  int windows = 150;     // the rolling horizon W, in steps
  int n_buffers = 3;     // steps whose results stay readable
};

inline size_t device_bytes(const Config& c) {
  return ((size_t)c.windows + 2) * (size_t)c.group_cap * (size_t)kRowStride * 4;
}

// What an image of this tracker's state depends on (steplane_host.h lane::Fingerprint): every field that
// shapes the state or its meaning, and the layout's constants; not device, n_buffers, span_cap.
inline lane::Fingerprint fingerprint(const Config& c) {
  using lane::field;
  lane::Fingerprint f;
  f.kind = lane::kSliSketch;
  f.fields = {field("group_cap", c.group_cap),
              field("windows", c.windows),
              field("row_stride", kRowStride)};
  return f;
}

inline void validate(const Config& c) {
  if (c.windows < 1 || c.windows > 4096) throw std::invalid_argument("ttft sketch: windows must be in [1, 4096]");
  if (c.span_cap <= 0 || c.span_cap > (1 << 24)) throw std::invalid_argument("ttft sketch: span_cap out of range");
  if ((uint64_t)c.span_cap * (uint64_t)c.windows >= (uint64_t(1) << 32))
    throw std::invalid_argument("ttft sketch: span_cap * windows must stay below 2^32 (a rolling counter would wrap)");
  if (c.group_cap < 1 || c.group_cap > 65536)
    throw std::invalid_argument("ttft sketch: group_cap must be in [1, 65536]");
  if (c.n_buffers < 1 || c.n_buffers > 64) throw std::invalid_argument("ttft sketch: n_buffers out of range");
  if (device_bytes(c) > (size_t(1) << 31))
    throw std::invalid_argument("ttft sketch: the histograms of windows x group_cap need more than 2 GiB");
}

// The result block of one step, in uint32 words, G = group_cap:
//   n[G]  sum_milli[G][2] (low, high)  le[G][8]  q_win[G][4]  n_roll[G]  q_roll[G][4]  stats[8]
// n / sum_milli / le are the window's; q_* are bucket indices (kEmpty for an empty group).
struct Layout {
  size_t n = 0, sum = 0, le = 0, q_win = 0, n_roll = 0, q_roll = 0, stats = 0, words = 0;
};
inline Layout layout(int group_cap) {
  const size_t g = (size_t)group_cap;
  Layout l;
  l.n = 0;
  l.sum = l.n + g;
  l.le = l.sum + 2 * g;
  l.q_win = l.le + (size_t)kLe * g;
  l.n_roll = l.q_win + (size_t)kQuantiles * g;
  l.q_roll = l.n_roll + g;
  l.stats = l.q_roll + (size_t)kQuantiles * g;
  l.words = (l.stats + kStats + 3) & ~size_t(3);  // whole 16-byte stores
  return l;
}

using mislo::Range;
inline size_t plan_ranges(const std::vector<Range>& ranges, int span_cap) {
  return mislo::plan_ranges(ranges, span_cap, "ttft sketch");
}

inline void check_step(int n_groups, int group_cap) {
  if (n_groups < 0 || n_groups > group_cap) throw std::invalid_argument("ttft sketch step: n_groups out of range");
}

}  // namespace slisketch
}  // namespace mislo
