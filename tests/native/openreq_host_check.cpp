// The open-request tracker's host side (ops/csrc/openreq_host.h: configuration and argument
// checks, the result block's layout, the result slots' bookkeeping) on its own, for the host
// sanitizers: tests/test_openreq.py builds this with -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "openreq_host.h"

using namespace mislo::openreq;

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

int main() {
  // configuration
  Config ok;
  validate(ok);
  for (int64_t cap : {int64_t(0), int64_t(63), int64_t(100), (int64_t(1) << 28) + 1, int64_t(-64)}) {
    Config c;
    c.cap = cap;
    CHECK(throws<std::invalid_argument>([&] { validate(c); }));
  }
  {
    Config c;
    c.cap = 64;
    validate(c);
    c.cap = int64_t(1) << 28;
    validate(c);
    c.slo_ms = 0.0;
    CHECK(throws<std::invalid_argument>([&] { validate(c); }));
    c.slo_ms = 800.0;
    c.ttl_ms = std::nan("");
    CHECK(throws<std::invalid_argument>([&] { validate(c); }));
    c.ttl_ms = 1.0;
    c.n_buffers = 0;
    CHECK(throws<std::invalid_argument>([&] { validate(c); }));
    c.n_buffers = 3;
    c.group_cap = 0;
    CHECK(throws<std::invalid_argument>([&] { validate(c); }));
    c.group_cap = 4;
    c.span_cap = -1;
    CHECK(throws<std::invalid_argument>([&] { validate(c); }));
  }
  CHECK(ms_to_ns(800.0) == 800000000 && ms_to_ns(0.0005) == 500 && ms_to_ns(120000.0) == 120000000000LL);

  // the result block: dl, dup, stats back to back, a whole number of 16-byte stores
  for (int g : {1, 3, 64, 1024, 1025}) {
    const Layout l = layout(g);
    CHECK(l.dl == 0 && l.dup == 2 * (size_t)g && l.stats == 5 * (size_t)g);
    CHECK(l.words >= l.stats + kStats && l.words % 4 == 0 && l.words - (l.stats + kStats) < 4);
    std::vector<uint32_t> block(l.words, 0u);  // every word of it is addressable
    block[l.dl + 2 * (size_t)(g - 1) + 1] = 1;
    block[l.dup + 3 * (size_t)(g - 1) + 2] = 2;
    block[l.stats + kMarkerDropped] = 3;
    block[l.words - 1] += 4;
    CHECK(block[l.stats - 1] == 2);
  }

  // span ranges
  std::vector<uint8_t> ring(64 * 8);
  const uintptr_t base = reinterpret_cast<uintptr_t>(ring.data());
  CHECK(plan_ranges({}, 4) == 0);
  CHECK(plan_ranges({{base, 128}, {0, 0}, {base + 256, 64}}, 4) == 3);
  CHECK(plan_ranges({{base, 256}}, 4) == 4);
  CHECK(throws<std::invalid_argument>([&] { plan_ranges({{base, 320}}, 4); }));
  CHECK(throws<std::invalid_argument>([&] { plan_ranges({{base, 192}, {base, 128}}, 4); }));
  CHECK(throws<std::invalid_argument>([&] { plan_ranges({{base, 63}}, 4); }));
  CHECK(throws<std::invalid_argument>([&] { plan_ranges({{0, 64}}, 4); }));
  CHECK(throws<std::invalid_argument>([&] { plan_ranges({{base, ~size_t(0) & ~size_t(63)}}, 4); }));

  // step arguments
  check_step(10, 0, 0, 4);
  check_step(10, 10, 4, 4);
  CHECK(throws<std::invalid_argument>([] { check_step(0, 0, 1, 4); }));
  CHECK(throws<std::invalid_argument>([] { check_step(-5, 0, 1, 4); }));
  CHECK(throws<std::invalid_argument>([] { check_step(10, 11, 1, 4); }));
  CHECK(throws<std::invalid_argument>([] { check_step(10, -1, 1, 4); }));
  CHECK(throws<std::invalid_argument>([] { check_step(10, 0, 5, 4); }));
  CHECK(throws<std::invalid_argument>([] { check_step(10, 0, -1, 4); }));

  // result slots: the last n steps stay readable, older ones and future ones are refused
  for (int n : {1, 2, 3, 7}) {
    SlotRing r(n);
    CHECK(r.size() == n && r.next() == 0 && !r.holds(0) && !r.holds(-1));
    CHECK(throws<std::out_of_range>([&] { r.slot_of(0); }));
    for (int64_t i = 0; i < 50; ++i) {
      CHECK(r.next() == i);
      const int s = r.begin();
      CHECK(s == (int)(i % n) && r.slot_of(i) == s);
      for (int64_t j = -2; j <= i + 2; ++j) {
        const bool held = j >= 0 && j <= i && j > i - n;
        CHECK(r.holds(j) == held);
        if (held) CHECK(r.slot_of(j) == (int)(j % n));
        else CHECK(throws<std::out_of_range>([&] { r.slot_of(j); }));
      }
    }
  }
  SlotRing z(0);  // a size the configuration check refuses: still one slot, never none
  CHECK(z.size() == 1 && z.begin() == 0 && z.holds(0));
  std::printf("openreq host ok\n");
  return 0;
}
