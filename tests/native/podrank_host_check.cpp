// The pod-breakdown tracker's host side (ops/csrc/podrank_host.h: the ranking key against a sorted
// reference over the field extremes, the pair key and its slot hash, the row, the configuration and
// argument checks, the result block's layout, and a host model of the open-addressing insert whose
// probing wraps past the table's end) on its own, for the host sanitizers: tests/test_podrank.py
// builds this with -fsanitize=address,undefined, runs it and compares the slot_of lines it prints
// with pipeline/podrank.py's.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <tuple>
#include <vector>

#include "podrank_host.h"

using namespace mislo::podrank;

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      std::fprintf(stderr, "check failed at line %d: %s\n", __LINE__, #x); \
      std::exit(1);                                                    \
    }                                                                  \
  } while (0)

template <class E, class F>
bool throws(F f) {
  try {
    f();
  } catch (const E&) {
    return true;
  }
  return false;
}

// the device's insert-or-add (podrank.hip pair_add) on the host: claim the first empty slot from
// slot_of on, wrapping; returns the slot, or `slots` when the table is full
static uint32_t host_insert(std::vector<uint64_t>& keys, std::vector<uint32_t>& n, uint32_t g, uint32_t pod) {
  const uint32_t slots = (uint32_t)keys.size(), mask = slots - 1;
  const uint64_t key = pair_key(g, pod);
  uint32_t s = slot_of(g, pod, slots);
  for (uint32_t probe = 0; probe <= mask; ++probe, s = (s + 1u) & mask) {
    if (keys[s] == 0) keys[s] = key;
    if (keys[s] == key) {
      ++n[s];
      return s;
    }
  }
  return slots;
}

int main() {
  // the ranking key against a sorted reference over the field extremes
  {
    using T = std::tuple<uint32_t, uint32_t, uint32_t>;  // b, n, pod
    const std::vector<uint32_t> bs = {1u, 2u, kCountLimit - 2u, kCountLimit - 1u};
    const std::vector<uint32_t> ns = {1u, 2u, 4096u, kCountLimit - 1u};
    const std::vector<uint32_t> pods = {0u, 1u, 77u, kPodLimit - 2u, kPodLimit - 1u};
    std::vector<T> all;
    for (uint32_t b : bs)
      for (uint32_t n : ns)
        for (uint32_t p : pods) all.emplace_back(b, n, p);
    // the rule: more breaches first, then fewer requests, then the lower pod
    std::vector<T> by_rule = all;
    std::sort(by_rule.begin(), by_rule.end(), [](const T& x, const T& y) {
      if (std::get<0>(x) != std::get<0>(y)) return std::get<0>(x) > std::get<0>(y);
      if (std::get<1>(x) != std::get<1>(y)) return std::get<1>(x) < std::get<1>(y);
      return std::get<2>(x) < std::get<2>(y);
    });
    std::vector<T> by_key = all;
    std::sort(by_key.begin(), by_key.end(), [](const T& x, const T& y) {
      return rank_key(std::get<0>(x), std::get<1>(x), std::get<2>(x)) > rank_key(std::get<0>(y), std::get<1>(y), std::get<2>(y));
    });
    CHECK(by_rule == by_key);
    for (const T& t : all) {
      const uint64_t k = rank_key(std::get<0>(t), std::get<1>(t), std::get<2>(t));
      CHECK(k != 0 && b_of_rank(k) == std::get<0>(t) && n_of_rank(k) == std::get<1>(t) && pod_of_rank(k) == std::get<2>(t));
    }
    CHECK(rank_key(1, kCountLimit - 1, kPodLimit - 1) == (1ull << 42));  // the smallest real key
    CHECK(rank_key(kCountLimit - 1, 0, 0) == ~0ull);                      // the fields fill the word exactly
  }
  // the pair key: never 0, round trip; the hash is murmur3's finalizer
  CHECK(pair_key(0, 0) == (1ull << 32) && group_of_pair(pair_key(65535, 9)) == 65535 && pod_of_pair(pair_key(3, 0xfffffu)) == 0xfffffu);
  CHECK(fmix64(0) == 0 && fmix64(1) == 0xb456bcfc34c2cb2cull);
  CHECK(ord_of_bits(0x80000000u) == 0 && ord_of_bits(0x7f800000u) == 0x7f800000u);
  CHECK(pow2_at_least(1) == 1 && pow2_at_least(2) == 2 && pow2_at_least(3) == 4 && pow2_at_least(8192) == 8192 &&
        pow2_at_least(8193) == 16384);
  // the row
  CHECK(sizeof(Row) == 32 && offsetof(Row, pod_id) == 0 && offsetof(Row, n) == 4 && offsetof(Row, b) == 8);
  CHECK(offsetof(Row, max_ttft) == 12 && offsetof(Row, sum_milli) == 16 && offsetof(Row, pad) == 24);
  // the configuration checks, both sides of every bound
  Config ok;
  validate(ok);
  CHECK(ok.k == 3 && ok.windows == 3 && ok.pair_cap == 4096 && window_slots(ok) == 8192 && recent_slots(ok) == 32768);
  CHECK(device_bytes(ok) == 16384ull * 64 + (8192ull + 32768 + 3 * 4096) * 28 + 8 * 64 * 4 + 2 * 64 * 3 * 8 +
                                layout(64, 3).words * 4 + 16);
  auto bad = [&](auto set) {
    Config c;
    c.span_cap = 64, c.pair_cap = 64;
    set(c);
    return throws<std::invalid_argument>([&] { validate(c); });
  };
  CHECK(bad([](Config& c) { c.k = 0; }) && bad([](Config& c) { c.k = 9; }));
  CHECK(!bad([](Config& c) { c.k = 1; }) && !bad([](Config& c) { c.k = 8; }));
  CHECK(bad([](Config& c) { c.windows = 0; }) && bad([](Config& c) { c.windows = 17; }));
  CHECK(!bad([](Config& c) { c.windows = 1; }) && !bad([](Config& c) { c.windows = 16; }));
  CHECK(bad([](Config& c) { c.pair_cap = 0; }) && bad([](Config& c) { c.pair_cap = (1 << 20) + 1; }));
  CHECK(!bad([](Config& c) { c.pair_cap = 1; }) && !bad([](Config& c) { c.pair_cap = 1 << 20; }));
  CHECK(bad([](Config& c) { c.group_cap = 0; }) && bad([](Config& c) { c.group_cap = 65537; }));
  CHECK(!bad([](Config& c) { c.group_cap = 1; }) && !bad([](Config& c) { c.group_cap = 65536; }));
  CHECK(bad([](Config& c) { c.span_cap = 0; }) && bad([](Config& c) { c.span_cap = -1; }));
  CHECK(!bad([](Config& c) { c.span_cap = 1; }) && !bad([](Config& c) { c.span_cap = (1 << 22) / 3, c.windows = 3; }));
  CHECK(bad([](Config& c) { c.span_cap = (1 << 22) / 3 + 1, c.windows = 3; }));
  CHECK(bad([](Config& c) { c.span_cap = 1 << 18, c.windows = 16; }) && !bad([](Config& c) { c.span_cap = (1 << 18) - 1, c.windows = 16; }));
  CHECK(bad([](Config& c) { c.span_cap = 1 << 22, c.windows = 1; }) && !bad([](Config& c) { c.span_cap = (1 << 22) - 1, c.windows = 1; }));
  CHECK(bad([](Config& c) { c.n_buffers = 0; }) && bad([](Config& c) { c.n_buffers = 65; }));
  CHECK(!bad([](Config& c) { c.n_buffers = 1; }) && !bad([](Config& c) { c.n_buffers = 64; }));
  CHECK(bad([](Config& c) { c.slo_ms = -1.0; }) && bad([](Config& c) { c.slo_ms = std::nan(""); }));
  CHECK(bad([](Config& c) { c.slo_ms = std::numeric_limits<double>::infinity(); }) && !bad([](Config& c) { c.slo_ms = 0.0; }));
  {
    // the largest shape the other bounds allow stays below 2 GiB: the bound holds the formula
    Config c;
    c.k = 8, c.windows = 16, c.pair_cap = 1 << 20, c.span_cap = (1 << 18) - 1, c.group_cap = 65536;
    CHECK(!throws<std::invalid_argument>([&] { validate(c); }) && device_bytes(c) < (1ull << 31));
    CHECK(window_slots(c) == (1u << 21) && recent_slots(c) == (1u << 25));
  }
  // the result block: every array on 16 bytes, in order, none overlapping
  for (int g : {1, 3, 5, 64, 65536})
    for (int k : {1, 3, 8}) {
      const Layout l = layout(g, k);
      const size_t g4 = ((size_t)g + 3) & ~size_t(3), rows = (size_t)g * k * kRowWords;
      std::vector<std::pair<size_t, size_t>> parts;  // (offset, words)
      for (int s = 0; s < 2; ++s)
        for (size_t at : {l.n[s], l.b[s], l.pods[s], l.pods_b[s], l.k_top[s]}) parts.emplace_back(at, (size_t)g);
      for (int s = 0; s < 2; ++s) parts.emplace_back(l.top[s], rows);
      parts.emplace_back(l.stats, (size_t)kStats);
      CHECK(parts.front().first == 0);
      for (size_t i = 0; i < parts.size(); ++i) {
        CHECK(parts[i].first % 4 == 0);
        if (i + 1 < parts.size()) CHECK(parts[i].first + parts[i].second <= parts[i + 1].first);
      }
      CHECK(l.top[0] == 10 * g4 && l.top[1] == l.top[0] + rows && l.stats == l.top[1] + rows);
      CHECK(l.words >= l.stats + kStats && l.words % 4 == 0 && l.words < l.stats + kStats + 4);
    }
  // the step's arguments
  std::vector<char> buf(64 * 8);
  const uintptr_t a = reinterpret_cast<uintptr_t>(buf.data());
  CHECK(plan_ranges({}, 4) == 0 && plan_ranges({{a, 128}, {0, 0}, {a + 128, 128}}, 4) == 4);
  CHECK(throws<std::invalid_argument>([&] { plan_ranges({{a, 128}, {a + 128, 192}}, 4); }));
  CHECK(throws<std::invalid_argument>([&] { plan_ranges({{a, 63}}, 4); }));
  CHECK(throws<std::invalid_argument>([&] { plan_ranges({{0, 64}}, 4); }));
  check_step(0, 3);
  check_step(3, 3);
  CHECK(throws<std::invalid_argument>([&] { check_step(4, 3); }));
  CHECK(throws<std::invalid_argument>([&] { check_step(-1, 3); }));
  // the insert: 16 slots filled to 8 pairs that all hash to the last slot, so probing wraps
  {
    std::vector<uint64_t> keys(16, 0);
    std::vector<uint32_t> n(16, 0);
    std::vector<uint32_t> pods;
    for (uint32_t p = 1; pods.size() < 8; ++p)
      if (slot_of(0, p, 16) == 15) pods.push_back(p);
    for (size_t i = 0; i < pods.size(); ++i) CHECK(host_insert(keys, n, 0, pods[i]) == (15 + (uint32_t)i) % 16);
    for (size_t i = 0; i < pods.size(); ++i) CHECK(host_insert(keys, n, 0, pods[i]) == (15 + (uint32_t)i) % 16);  // found again
    CHECK(keys[15] == pair_key(0, pods[0]) && keys[0] == pair_key(0, pods[1]) && keys[6] == pair_key(0, pods[7]) && keys[7] == 0);
    for (uint32_t s = 0; s < 16; ++s) CHECK(n[s] == (keys[s] ? 2u : 0u));
    // filled to the brim, a ninth .. sixteenth pair still lands, a seventeenth finds the table full
    uint32_t extra = 0;
    for (uint32_t p = 1u << 19; extra < 8; ++p, ++extra) CHECK(host_insert(keys, n, 1, p) < 16);
    CHECK(host_insert(keys, n, 2, 5) == 16);
  }
  const uint32_t probe[][3] = {{0, 0, 2},        {0, 1, 16},          {0, 5, 16},         {3, 77, 8192}, {63, (1u << 20) - 1, 32768},
                               {65535, 12345, 1u << 21}, {1, 0xfffffu, 16}, {7, 7, 1u << 25}};
  for (const auto& p : probe) std::printf("slot_of %u %u %u %u\n", p[0], p[1], p[2], slot_of(p[0], p[1], p[2]));
  std::puts("podrank host ok");
  return 0;
}
