// Host side of the per-pod breach breakdown (podrank.h) that needs no device: the pair key and its
// slot hash, the ranking key, the pod row, the configuration and argument checks and the result
// block's layout. Plain C++ (no HIP header), so it builds and runs on its own under the host
// sanitizers (tests/native/podrank_host_check.cpp); the kernels use the same helpers.
// pipeline/podrank.py carries the same constants and rules in numpy.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <stdexcept>
#include <utility>
#include <vector>

#include "steplane_host.h"  // Range, plan_ranges, kSpanBytes

#if defined(__HIPCC__)
#define MISLO_PR_HD __host__ __device__
#else
#define MISLO_PR_HD
#endif

namespace mislo {
namespace podrank {

constexpr int kMaxK = 8;               // ranked pods per service and scope
constexpr int kMaxH = 16;              // windows of the horizon
constexpr int kPodBits = 20;           // pods at or above 2^20 count in no pod row
constexpr uint32_t kPodLimit = 1u << kPodBits;
constexpr int kCountBits = 22;         // requests and breaches of one pair over the horizon stay below 2^22
constexpr uint32_t kCountLimit = 1u << kCountBits;
constexpr int kMaxPairCap = 1 << 20;
constexpr float kMaxMs = 2097152.0f;   // 2^21: the sum's clamp (the TTFT sketch's)
constexpr int kRowBytes = 32;
constexpr int kRowWords = kRowBytes / 4;
constexpr int kLdsSlots = 256;         // the observe kernel's per-workgroup table (28 B a slot, 7 KB)
constexpr int kLdsGroups = 64;         // services whose totals, pod counts and K slots the kernels keep in LDS
constexpr int kLdsProbes = 16;         // LDS probes before a record goes to the global table itself

// per-step statistics (uint32 each), pipeline/podrank.py STATS in the same order
enum Stat {
  kObserved = 0,       // records counted in n / b
  kInvalid = 1,        // counted by the engine, ttft NaN or negative
  kOutOfGroup = 2,     // SLI records with group_id >= n_groups
  kPodOutOfRange = 3,  // observed, pod_id >= 2^20: in n / b, in no pod row
  kPairOverflow = 4,   // observed records whose pair found no place among the window's pair_cap
  kStats = 8
};

// One ranked pod (pipeline/podrank.py POD_ROW).
struct Row {
  uint32_t pod_id, n, b;
  uint32_t max_ttft;   // float32 bits of the largest TTFT (the sign masked: -0.0 reads +0.0)
  uint64_t sum_milli;  // exact sum of min(ttft, 2^21) in 1/1000 ms
  uint32_t pad[2];
};
static_assert(sizeof(Row) == kRowBytes, "a pod row is 32 bytes");

// the value order of the accepted TTFTs (>= 0, +inf highest): the float's bits without the sign
MISLO_PR_HD inline uint32_t ord_of_bits(uint32_t bits) { return bits & 0x7fffffffu; }

// The table key of a (service, pod) pair; 0 = empty slot.
MISLO_PR_HD inline uint64_t pair_key(uint32_t g, uint32_t pod) { return ((uint64_t)(g + 1u) << 32) | (uint64_t)pod; }
MISLO_PR_HD inline uint32_t group_of_pair(uint64_t key) { return (uint32_t)(key >> 32) - 1u; }
MISLO_PR_HD inline uint32_t pod_of_pair(uint64_t key) { return (uint32_t)key; }

// murmur3's 64-bit finalizer
MISLO_PR_HD inline uint64_t fmix64(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}
// the first slot probed for a pair in a table of `slots` (a power of two); then slot + 1, wrapping
MISLO_PR_HD inline uint32_t slot_of(uint32_t g, uint32_t pod, uint32_t slots) {
  return (uint32_t)(fmix64(pair_key(g, pod)) & (uint64_t)(slots - 1u));
}

// Ranking within a service: more breaches first, then fewer requests, then the lower pod id.
// b >= 1, so no real key is 0 (= empty); b and n stay below 2^22, pod below 2^20.
MISLO_PR_HD inline uint64_t rank_key(uint32_t b, uint32_t n, uint32_t pod) {
  return ((uint64_t)b << 42) | ((uint64_t)(kCountLimit - 1u - n) << 20) | (uint64_t)(kPodLimit - 1u - pod);
}
MISLO_PR_HD inline uint32_t b_of_rank(uint64_t key) { return (uint32_t)(key >> 42); }
MISLO_PR_HD inline uint32_t n_of_rank(uint64_t key) { return kCountLimit - 1u - ((uint32_t)(key >> 20) & (kCountLimit - 1u)); }
MISLO_PR_HD inline uint32_t pod_of_rank(uint64_t key) { return kPodLimit - 1u - ((uint32_t)key & (kPodLimit - 1u)); }

inline uint32_t pow2_at_least(uint64_t v) {
  uint32_t p = 1;
  while ((uint64_t)p < v) p <<= 1;
  return p;
}

struct Config {
  int device = 0;
  int k = 3;             // ranked pods per service and scope
  int windows = 3;       // the horizon H, in steps
  int pair_cap = 4096;   // distinct (service, pod) pairs one window may hold
  int span_cap = 16384;  // span records per step
  int group_cap = 64;    // services (incident groups), at most
  int n_buffers = 3;     // steps whose results stay readable
  double slo_ms = 800.0; // a TTFT above it (float32 compare) is a breach
  bool lds = true;       // pre-aggregate every workgroup's records in LDS (off: the measurement's other side)
};

// slots of the window's table and of the recent table (the horizon's H * pair_cap pairs at most)
inline uint32_t window_slots(const Config& c) { return pow2_at_least(2ull * (uint64_t)c.pair_cap); }
inline uint32_t recent_slots(const Config& c) { return pow2_at_least(2ull * (uint64_t)c.pair_cap * (uint64_t)c.windows); }

constexpr uint64_t kEntryBytes = 8 + 4 + 4 + 4 + 8;  // key, n, b, max, sum (structure of arrays)

// The result block of one step, in uint32 words; G4 = group_cap rounded up to 4, so every array
// starts on 16 bytes. Two scopes (0 = window, 1 = recent), each
//   n[G4] b[G4] pods[G4] pods_b[G4] k_top[G4]
// then top[2][G][K] rows, then stats[8]. Rows past k_top are all zero.
struct Layout {
  size_t n[2] = {0, 0}, b[2] = {0, 0}, pods[2] = {0, 0}, pods_b[2] = {0, 0}, k_top[2] = {0, 0}, top[2] = {0, 0};
  size_t stats = 0, words = 0;
};
inline Layout layout(int group_cap, int k) {
  const size_t g4 = ((size_t)group_cap + 3) & ~size_t(3), rows = (size_t)group_cap * (size_t)k * kRowWords;
  Layout l;
  size_t at = 0;
  for (int s = 0; s < 2; ++s) {
    l.n[s] = at, at += g4;
    l.b[s] = at, at += g4;
    l.pods[s] = at, at += g4;
    l.pods_b[s] = at, at += g4;
    l.k_top[s] = at, at += g4;
  }
  for (int s = 0; s < 2; ++s) l.top[s] = at, at += rows;  // 8 words a row: 16-byte aligned
  l.stats = at, at += kStats;
  l.words = (at + 3) & ~size_t(3);
  return l;
}

// spans, both tables, the horizon's lists, totals and their history, the two key lists, the block
inline uint64_t device_bytes(const Config& c) {
  const uint64_t G = (uint64_t)c.group_cap, H = (uint64_t)c.windows;
  return (uint64_t)c.span_cap * kSpanBytes + ((uint64_t)window_slots(c) + recent_slots(c)) * kEntryBytes +
         H * (uint64_t)c.pair_cap * kEntryBytes + (2 + 2 * H) * G * 4 + 2 * G * (uint64_t)c.k * 8 +
         (uint64_t)layout(c.group_cap, c.k).words * 4 + (H + 1) * 4;
}

// What an image of this tracker's state depends on (steplane_host.h lane::Fingerprint): every field that
// shapes the state or its meaning, and the layout's constants; not device, n_buffers, span_cap or lds.
inline lane::Fingerprint fingerprint(const Config& c) {
  using lane::field;
  using lane::real_field;
  lane::Fingerprint f;
  f.kind = lane::kPodRank;
  f.fields = {field("group_cap", c.group_cap),
              field("windows", c.windows),
              field("k", c.k),
              field("pair_cap", c.pair_cap),
              real_field("slo_ms", c.slo_ms),
              field("entry_bytes", (int64_t)kEntryBytes)};
  return f;
}

inline void validate(const Config& c) {
  if (c.k < 1 || c.k > kMaxK) throw std::invalid_argument("pod breakdown: k must be in [1, 8]");
  if (c.windows < 1 || c.windows > kMaxH) throw std::invalid_argument("pod breakdown: windows must be in [1, 16]");
  if (c.pair_cap < 1 || c.pair_cap > kMaxPairCap) throw std::invalid_argument("pod breakdown: pair_cap must be in [1, 2^20]");
  if (c.group_cap < 1 || c.group_cap > 65536) throw std::invalid_argument("pod breakdown: group_cap must be in [1, 65536]");
  if (c.span_cap < 1 || (uint64_t)c.span_cap * (uint64_t)c.windows >= kCountLimit)
    throw std::invalid_argument("pod breakdown: span_cap must be >= 1 and span_cap * windows < 2^22");
  if (c.n_buffers < 1 || c.n_buffers > 64) throw std::invalid_argument("pod breakdown: n_buffers out of range");
  if (!std::isfinite(c.slo_ms) || c.slo_ms < 0.0) throw std::invalid_argument("pod breakdown: slo_ms must be finite and >= 0");
  if (device_bytes(c) > (uint64_t(1) << 31)) throw std::invalid_argument("pod breakdown: the tables need more than 2 GiB");
}

using mislo::Range;
inline size_t plan_ranges(const std::vector<Range>& ranges, int span_cap) {
  return mislo::plan_ranges(ranges, span_cap, "pod breakdown");
}

inline void check_step(int n_groups, int group_cap) {
  if (n_groups < 0 || n_groups > group_cap) throw std::invalid_argument("pod breakdown step: n_groups out of range");
}

}  // namespace podrank
}  // namespace mislo
