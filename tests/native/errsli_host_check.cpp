// The host side of the error SLI tracker (ops/csrc/errsli_host.h) on its own: the class field over
// every value, the burn compare against unsigned __int128 at the bounds, the budget, the age, the LDS
// key, validate, layout, plan_ranges and check_step. Built with the host sanitizers by tests/test_errsli.py.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>

#include "errsli_host.h"

using namespace mislo::errsli;

#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      return 1;                                                          \
    }                                                                    \
  } while (0)

template <class F>
static bool throws(F f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

// the compare without any thought for width
static bool wide_burns(uint32_t n, uint32_t bad, uint32_t min_requests, uint64_t thr) {
  const unsigned __int128 lhs = (unsigned __int128)bad * 1000000000u, rhs = (unsigned __int128)thr * n;
  return n >= min_requests && n > 0 && lhs >= rhs;
}

int main() {
  // the class field: bits 4-7 and nothing else
  for (uint32_t c = 0; c < 16; ++c) {
    CHECK(pack_outcome(c) == c << 4 && (pack_outcome(c) & ~kOutcomeMask) == 0);
    for (uint32_t rest : {0u, 0xFFFFFF0Fu, 0x0000010Fu, 0xABCDEF03u}) CHECK(outcome_of(rest | pack_outcome(c)) == c);
  }
  CHECK(outcome_of(0xFFFFFF0Fu) == 0 && outcome_of(0xF0u) == 15 && kOutcomeShift == 4 && kSkipMask == 12u);

  // the burn compare at the bounds: n = bad = 2^32 - 1 with the largest product allowed stays below 2^63
  const uint32_t top = 0xFFFFFFFFu;
  const uint64_t thrs[] = {1ull, 1000ull, 14400000ull, 100000000ull, 999999999ull, kBurnScale};
  const uint32_t ns[] = {0u, 1u, 9u, 10u, 11u, 1000u, 1u << 31, top - 1u, top};
  for (uint64_t thr : thrs)
    for (uint32_t n : ns)
      for (uint32_t bad : ns) {
        if (bad > n) continue;
        for (uint32_t mn : {0u, 10u, top}) CHECK(burns(n, bad, mn, thr) == wide_burns(n, bad, mn, thr));
      }
  CHECK((unsigned __int128)top * kBurnScale < ((unsigned __int128)1 << 63));
  CHECK(burns(top, top, top, kBurnScale) && !burns(top, top - 1u, 0u, kBurnScale) && burns(top, 5u, 0u, 1ull) &&
        !burns(top, 4u, 0u, 1ull));
  CHECK(burns(10, 1, 0, 100000000ull) && !burns(11, 1, 0, 100000000ull) && burns(9, 1, 0, 100000000ull));
  CHECK(!burns(0, 0, 0, 1ull) && !burns(9, 9, 10, 1ull) && burns(10, 10, 10, kBurnScale));

  CHECK(budget_ppm(0.999) == 1000u && budget_ppm(0.9) == 100000u && budget_ppm(0.99) == 10000u && budget_ppm(0.0) == 1000000u);
  CHECK(budget_ppm(0.9999999) == 1u && budget_ppm(0.5) == 500000u && budget_ppm(0.9995) == 500u);
  CHECK(next_age(0, 0) == 0 && next_age(7, 0) == 0 && next_age(0, 1) == 1 && next_age(7, 8) == 8 && next_age(top, 1) == top);

  for (uint32_t g : {0u, 1u, 63u, 65535u})
    for (uint32_t c = 0; c < (uint32_t)kClasses; ++c) {
      const uint64_t k = lds_key(g, c);
      CHECK(k != 0 && lds_group(k) == g && lds_class(k) == c && mislo::onset::lds_hash(k) < (uint32_t)kLdsSlots);
    }

  // layout: every array on 16 bytes, none overlapping, whole 16-byte stores
  for (int g : {1, 2, 3, 5, 8, 64, 65536}) {
    const Layout l = layout(g);
    const size_t at[] = {l.counts, l.counts_roll, l.pair_sums, l.firing, l.age, l.stats, l.words};
    const size_t need[] = {8u * g, 8u * g, 16u * g, (size_t)g, (size_t)g, (size_t)kStats};
    for (int i = 0; i < 6; ++i) CHECK(at[i] % 4 == 0 && at[i] + need[i] <= at[i + 1]);
    CHECK(l.counts == 0 && l.words % 4 == 0);
    std::printf("layout %d %zu %zu %zu %zu %zu %zu %zu\n", g, l.counts, l.counts_roll, l.pair_sums, l.firing, l.age, l.stats,
                l.words);
  }

  Config ok;
  validate(ok);
  const auto bad = [&](auto set) {
    Config c;
    c.windows = 4;
    c.pairs = {{2, 1, 1000}};
    c.target = 0.9;
    set(c);
    return throws([&] { validate(c); });
  };
  CHECK(!bad([](Config&) {}));
  CHECK(bad([](Config& c) { c.windows = 0; }) && bad([](Config& c) { c.windows = 32769; }));
  CHECK(bad([](Config& c) { c.group_cap = 0; }) && bad([](Config& c) { c.group_cap = 65537; }));
  CHECK(bad([](Config& c) { c.span_cap = 0; }) && bad([](Config& c) { c.n_buffers = 0; }) && bad([](Config& c) { c.n_buffers = 65; }));
  CHECK(bad([](Config& c) { c.target = 1.0; }) && bad([](Config& c) { c.target = -0.1; }));
  CHECK(bad([](Config& c) { c.target = std::numeric_limits<double>::quiet_NaN(); }));
  CHECK(bad([](Config& c) { c.target = std::numeric_limits<double>::infinity(); }));
  CHECK(bad([](Config& c) { c.pairs.clear(); }) && bad([](Config& c) { c.pairs.assign(5, Pair{1, 1, 1000}); }));
  CHECK(bad([](Config& c) { c.pairs = {{5, 1, 1000}}; }) && bad([](Config& c) { c.pairs = {{2, 3, 1000}}; }));
  CHECK(bad([](Config& c) { c.pairs = {{2, 0, 1000}}; }) && bad([](Config& c) { c.pairs = {{2, 1, 0}}; }));
  CHECK(bad([](Config& c) { c.pairs = {{2, 1, 10001}}; }) && !bad([](Config& c) { c.pairs = {{2, 1, 10000}}; }));
  CHECK(bad([](Config& c) { c.pairs = {{2, 1, std::numeric_limits<int64_t>::max()}}; }));
  CHECK(bad([](Config& c) { c.min_requests = -1; }) && bad([](Config& c) { c.min_requests = int64_t(1) << 32; }));
  CHECK(bad([](Config& c) { c.bad_mask = 0; }) && bad([](Config& c) { c.bad_mask = 0xF9; }) && bad([](Config& c) { c.bad_mask = 0x1F8; }));
  CHECK(bad([](Config& c) { c.span_cap = 1 << 21, c.windows = 2048; }));   // span_cap * windows = 2^32
  CHECK(bad([](Config& c) { c.group_cap = 65536, c.windows = 32768; }));  // far beyond 2 GiB
  CHECK(!bad([](Config& c) { c.windows = 1, c.group_cap = 1, c.span_cap = 1, c.n_buffers = 1, c.target = 0.0, c.pairs = {{1, 1, 1}}, c.bad_mask = 2; }));
  CHECK(!bad([](Config& c) { c.windows = 32768, c.pairs = {{32768, 32768, 1000}}; }));
  CHECK(!bad([](Config& c) { c.pairs.assign(4, Pair{4, 4, 1}); }));
  {
    Config c;
    CHECK(device_bytes(c) == 16384ull * 64 + 3602ull * 64 * 32 + 64ull * 17 * 4 + layout(64).words * 4);
    std::printf("device_bytes %llu\n", (unsigned long long)device_bytes(c));
  }

  // ranges
  static unsigned char buf[64 * 8];
  const uintptr_t a = reinterpret_cast<uintptr_t>(buf);
  CHECK(plan_ranges({}, 4) == 0 && plan_ranges({{a, 0}, {0, 0}}, 4) == 0);
  CHECK(plan_ranges({{a, 128}, {a + 128, 0}, {a + 128, 128}}, 4) == 4);
  CHECK(throws([&] { plan_ranges({{a, 63}}, 4); }) && throws([&] { plan_ranges({{0, 64}}, 4); }));
  CHECK(throws([&] { plan_ranges({{a, 128}, {a, 192}}, 4); }) && throws([&] { plan_ranges({{a, 320}}, 4); }));
  check_step(0, 4);
  check_step(4, 4);
  CHECK(throws([] { check_step(-1, 4); }) && throws([] { check_step(5, 4); }));

  std::printf("errsli host ok\n");
  return 0;
}
