// The request-exemplar tracker's host side (ops/csrc/exemplars_host.h: the two order keys at their
// edge values, the row, the configuration and argument checks, the result block's layout) on its
// own, for the host sanitizers: tests/test_exemplars.py builds this with
// -fsanitize=address,undefined and runs it.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "exemplars_host.h"

using namespace mislo::exemplars;

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

static uint64_t wk(float v, uint32_t i) { return window_key(bits_of(v), i); }

int main() {
  const float inf = std::numeric_limits<float>::infinity();
  // the window key: the value order of the accepted TTFTs, ascending here
  const std::vector<float> asc = {0.0f,   1e-40f, std::nextafterf(0.125f, 0.0f), 0.125f, 437.5f, std::nextafterf(800.0f, 0.0f),
                                  800.0f, std::nextafterf(800.0f, inf), 2097152.0f, std::numeric_limits<float>::max(), inf};
  for (size_t a = 0; a + 1 < asc.size(); ++a) {
    CHECK(asc[a] < asc[a + 1]);
    CHECK(wk(asc[a], 0) < wk(asc[a + 1], 0x7ffffffeu));  // the value decides before the index
  }
  // -0.0 ranks as 0, not above +inf; among equal values the earlier record is larger
  CHECK(ord_of_bits(bits_of(-0.0f)) == 0u && wk(-0.0f, 5) == wk(0.0f, 5) && wk(-0.0f, 0) < wk(inf, 0x7ffffffeu));
  CHECK(wk(0.0f, 4) > wk(-0.0f, 5) && wk(437.5f, 0) > wk(437.5f, 1) && wk(inf, 7) > wk(inf, 8));
  // no real key is 0 (an index stays below 2^31); the index round-trips
  CHECK(wk(0.0f, 0x7ffffffeu) != 0 && wk(0.0f, 0) == 0xffffffffull);
  for (uint32_t i : {0u, 1u, 16382u, 0x7ffffffeu}) CHECK(index_of_key(wk(437.5f, i)) == i);
  // the cross-window key: the value, then the newer window, then the earlier position; never 0
  CHECK(recent_key(bits_of(900.0f), 15, 7) > recent_key(bits_of(800.0f), 0, 0));
  CHECK(recent_key(bits_of(800.0f), 0, 7) > recent_key(bits_of(800.0f), 1, 0));
  CHECK(recent_key(bits_of(800.0f), 2, 3) > recent_key(bits_of(800.0f), 2, 4));
  CHECK(recent_key(bits_of(-0.0f), 15, 7) == (1ull << 16) && recent_key(bits_of(-0.0f), 2, 1) == recent_key(0u, 2, 1));
  {
    std::vector<uint64_t> all;
    for (uint32_t age = 0; age < (uint32_t)kMaxH; ++age)
      for (uint32_t p = 0; p < (uint32_t)kMaxK; ++p) all.push_back(recent_key(bits_of(437.5f), age, p));
    std::sort(all.begin(), all.end());
    CHECK(std::adjacent_find(all.begin(), all.end()) == all.end() && all.size() == 128);
  }
  // the row
  CHECK(sizeof(Row) == 64 && offsetof(Row, trace_h) == 8 && offsetof(Row, span_h) == 16 && offsetof(Row, ttft_ms) == 24);
  CHECK(offsetof(Row, retr_ms) == 32 && offsetof(Row, pod_id) == 36 && offsetof(Row, flags) == 44);
  CHECK(offsetof(Row, age) == 48 && offsetof(Row, index) == 52 && offsetof(Row, pad) == 56);
  // the configuration checks
  Config ok;
  validate(ok);
  CHECK(ok.k == 3 && ok.windows == 3 && device_bytes(ok) == 5ull * 64 * 3 * 64);
  auto bad = [&](auto set) {
    Config c;
    set(c);
    return throws<std::invalid_argument>([&] { validate(c); });
  };
  CHECK(bad([](Config& c) { c.k = 0; }) && bad([](Config& c) { c.k = 9; }));
  CHECK(bad([](Config& c) { c.windows = 0; }) && bad([](Config& c) { c.windows = 17; }));
  CHECK(bad([](Config& c) { c.group_cap = 0; }) && bad([](Config& c) { c.group_cap = 65537; }));
  CHECK(bad([](Config& c) { c.span_cap = 0; }) && bad([](Config& c) { c.span_cap = -1; }));
  CHECK(bad([](Config& c) { c.n_buffers = 0; }) && bad([](Config& c) { c.n_buffers = 65; }));
  CHECK(!bad([](Config& c) { c.k = 8, c.windows = 16, c.group_cap = 1, c.span_cap = 0x7fffffff, c.n_buffers = 64; }));
  // (16 + 2) * 65536 * 8 * 64 is 576 MiB; no allowed shape passes 2 GiB, the bound holds the formula
  CHECK(!bad([](Config& c) { c.k = 8, c.windows = 16, c.group_cap = 65536; }));
  {
    Config c;
    c.k = 8, c.windows = 16, c.group_cap = 65536;
    CHECK(device_bytes(c) == 18ull * 65536 * 8 * 64 && device_bytes(c) <= (1ull << 31));
  }
  // the result block
  for (int g : {1, 3, 64, 65536})
    for (int k : {1, 3, 8}) {
      const Layout l = layout(g, k);
      CHECK(l.n == 0 && l.k_win == (size_t)g && l.k_recent == 2 * (size_t)g && l.win >= 3 * (size_t)g && l.win % 4 == 0);
      CHECK(l.win < 3 * (size_t)g + 4 && l.recent == l.win + (size_t)g * k * 16 && l.stats == l.recent + (size_t)g * k * 16);
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
  std::puts("exemplars host ok");
  return 0;
}
