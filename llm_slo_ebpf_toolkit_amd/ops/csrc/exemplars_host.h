// Host side of the request-exemplar tracker (exemplars.h) that needs no device: the two order keys,
// the exemplar row, the configuration and argument checks and the result block's layout. Plain C++
// (no HIP header), so it builds and runs on its own under the host sanitizers
// (tests/native/exemplars_host_check.cpp); the kernels use the same key helpers.
// pipeline/exemplars.py carries the same constants and rules in numpy.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cstring>
#include <stdexcept>
#include <utility>
#include <vector>

#include "steplane_host.h"  // Range, plan_ranges, kSpanBytes

#if defined(__HIPCC__)
#define MISLO_EX_HD __host__ __device__
#else
#define MISLO_EX_HD
#endif

namespace mislo {
namespace exemplars {

constexpr int kMaxK = 8;        // exemplars per service and list
constexpr int kMaxH = 16;       // windows of the horizon: H * K <= 128 = two candidates per lane of one wave
constexpr int kLdsGroups = 64;  // groups whose K slots the select kernel keeps in LDS ([64][8] u64 = 4 KB)
constexpr int kRowBytes = 64;
constexpr int kRowWords = kRowBytes / 4;

// per-step statistics (uint32 each), pipeline/exemplars.py STATS in the same order
enum Stat {
  kObserved = 0,    // records that competed for a slot
  kInvalid = 1,     // counted by the engine, ttft NaN or negative
  kOutOfGroup = 2,  // SLI records with group_id >= n_groups
  kStats = 8
};

// One exemplar (pipeline/exemplars.py EXEMPLAR).
struct Row {
  int64_t ts_ns;
  uint64_t trace_h, span_h;
  float ttft_ms, latency_ms, retr_ms;
  uint32_t pod_id, pid, flags;
  uint32_t age;    // windows ago; 0 in a window row
  uint32_t index;  // the record's index in its step
  uint32_t pad[2];
};
static_assert(sizeof(Row) == kRowBytes, "an exemplar row is 64 bytes");

// the value order of the accepted TTFTs (>= 0, +inf highest): the float's bits without the sign, so
// -0.0 ranks as 0 and not above +inf
MISLO_EX_HD inline uint32_t ord_of_bits(uint32_t bits) { return bits & 0x7fffffffu; }

// Within a window: larger TTFT first, equal TTFTs to the earlier record. 0 = empty; no real key is
// 0, since an index stays below 2^31.
MISLO_EX_HD inline uint64_t window_key(uint32_t ttft_bits, uint32_t index) {
  return ((uint64_t)ord_of_bits(ttft_bits) << 32) | (uint64_t)(0xffffffffu - index);
}
MISLO_EX_HD inline uint32_t index_of_key(uint64_t key) { return 0xffffffffu - (uint32_t)key; }

// Across windows: larger TTFT first, then the newer window, then the earlier position in its
// window's list. Bit 16 keeps a real key from being 0.
MISLO_EX_HD inline uint64_t recent_key(uint32_t ttft_bits, uint32_t age, uint32_t pos) {
  return ((uint64_t)ord_of_bits(ttft_bits) << 32) | (1u << 16) | ((15u - age) << 8) | (7u - pos);
}

inline uint32_t bits_of(float v) {
  uint32_t b;
  std::memcpy(&b, &v, 4);
  return b;
}

struct Config {
  int device = 0;
  int k = 3;             // exemplars per service and list
  int windows = 3;       // the horizon H, in steps
  int span_cap = 16384;  // span records per step
  int group_cap = 64;    // services (incident groups), at most
  int n_buffers = 3;     // steps whose results stay readable
  bool lds = true;       // privatise the groups below kLdsGroups in LDS (off: the measurement's other side)
};

// the device rows: the horizon's H slots and the block's two lists
inline uint64_t device_bytes(const Config& c) {
  return ((uint64_t)c.windows + 2) * (uint64_t)c.group_cap * (uint64_t)c.k * kRowBytes;
}

// What an image of this tracker's state depends on (steplane_host.h lane::Fingerprint): every field that
// shapes the state or its meaning, and the layout's constants; not device, n_buffers, span_cap or lds.
inline lane::Fingerprint fingerprint(const Config& c) {
  using lane::field;
  lane::Fingerprint f;
  f.kind = lane::kExemplars;
  f.fields = {field("group_cap", c.group_cap),
              field("windows", c.windows),
              field("k", c.k),
              field("row_bytes", kRowBytes)};
  return f;
}

inline void validate(const Config& c) {
  if (c.k < 1 || c.k > kMaxK) throw std::invalid_argument("request exemplars: k must be in [1, 8]");
  if (c.windows < 1 || c.windows > kMaxH) throw std::invalid_argument("request exemplars: windows must be in [1, 16]");
  if (c.group_cap < 1 || c.group_cap > 65536)
    throw std::invalid_argument("request exemplars: group_cap must be in [1, 65536]");
  if (c.span_cap < 1) throw std::invalid_argument("request exemplars: span_cap must be in [1, 2^31)");
  if (c.n_buffers < 1 || c.n_buffers > 64) throw std::invalid_argument("request exemplars: n_buffers out of range");
  if (device_bytes(c) > (uint64_t(1) << 31))
    throw std::invalid_argument("request exemplars: the rows of windows x group_cap x k need more than 2 GiB");
}

// The result block of one step, in uint32 words, G = group_cap:
//   n[G]  k_win[G]  k_recent[G]  (pad to 16 bytes)  win[G][K] rows  recent[G][K] rows  stats[8]
// Valid rows come first and are sorted; rows past the count are all zero.
struct Layout {
  size_t n = 0, k_win = 0, k_recent = 0, win = 0, recent = 0, stats = 0, words = 0;
};
inline Layout layout(int group_cap, int k) {
  const size_t g = (size_t)group_cap, rows = g * (size_t)k * kRowWords;
  Layout l;
  l.n = 0;
  l.k_win = l.n + g;
  l.k_recent = l.k_win + g;
  l.win = (l.k_recent + g + 3) & ~size_t(3);  // rows are written with 16-byte stores
  l.recent = l.win + rows;
  l.stats = l.recent + rows;
  l.words = (l.stats + kStats + 3) & ~size_t(3);
  return l;
}

using mislo::Range;
inline size_t plan_ranges(const std::vector<Range>& ranges, int span_cap) {
  return mislo::plan_ranges(ranges, span_cap, "request exemplars");
}

inline void check_step(int n_groups, int group_cap) {
  if (n_groups < 0 || n_groups > group_cap) throw std::invalid_argument("request exemplars step: n_groups out of range");
}

}  // namespace exemplars
}  // namespace mislo
