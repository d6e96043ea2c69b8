// The TTFT sketch's host side (ops/csrc/slisketch_host.h: the bucket rule at its edge values, the
// configuration and argument checks, the result block's layout) and the result slots it shares
// with the open-request tracker, on their own, for the host sanitizers: tests/test_slisketch.py
// builds this with -fsanitize=address,undefined and runs it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "openreq_host.h"
#include "slisketch_host.h"

using namespace mislo::slisketch;

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
  const float inf = std::numeric_limits<float>::infinity();
  // the bucket rule at its edges
  CHECK(kK == 386 && kLo == 1984u && kRowStride >= kK && kRowStride % 4 == 0 && kRowStride % kPerLane == 0);
  CHECK(bucket_of(0.0f) == 0 && bucket_of(-0.0f) == 0 && bucket_of(1e-40f) == 0);
  CHECK(bucket_of(std::nextafterf(0.125f, 0.0f)) == 0 && bucket_of(0.125f) == 1);
  CHECK(bucket_of(std::nextafterf(0.125f, 1.0f)) == 1);
  CHECK(bucket_of(800.0f) == bucket_of(std::nextafterf(800.0f, inf)));
  CHECK(bucket_of(std::nextafterf(800.0f, 0.0f)) == bucket_of(800.0f) - 1);  // 800 = 1.5625 * 2^9: a bucket edge
  CHECK(bucket_of(std::nextafterf(kMaxMs, 0.0f)) == (uint32_t)kNB && bucket_of(kMaxMs) == (uint32_t)kK - 1);
  CHECK(bucket_of(std::nextafterf(kMaxMs, inf)) == (uint32_t)kK - 1 && bucket_of(inf) == (uint32_t)kK - 1);
  CHECK(bucket_lower(1) == 0.125f && bucket_lower(kNB + 1) == kMaxMs);
  for (int b = 1; b <= kNB; ++b) {
    const float lo = bucket_lower(b), hi = bucket_lower(b + 1);
    CHECK(lo < hi && bucket_of(lo) == (uint32_t)b && bucket_of(std::nextafterf(hi, 0.0f)) == (uint32_t)b);
    const double rep = representative(b);
    CHECK(rep > lo && rep < hi);
    // every value of the bucket lies within 1/32 of its representative
    CHECK(std::fabs(rep - (double)lo) <= (double)lo / 32.0);
    CHECK(std::fabs((double)std::nextafterf(hi, 0.0f) - rep) <= (double)lo / 32.0);
  }
  CHECK(representative(0) == 0.0 && representative(kK - 1) == 2097152.0);

  // `le` slots: exact Prometheus semantics, v <= edge
  CHECK(le_slot(0.0f) == 0 && le_slot(50.0f) == 0 && le_slot(std::nextafterf(50.0f, inf)) == 1);
  CHECK(le_slot(800.0f) == 4 && le_slot(std::nextafterf(800.0f, inf)) == 5 && le_slot(2000.0f) == 6);
  CHECK(le_slot(std::nextafterf(2000.0f, inf)) == kEdges && le_slot(inf) == kEdges);

  // nearest ranks
  CHECK(rank_of(500, 1) == 1 && rank_of(990, 1) == 1 && rank_of(500, 2) == 1 && rank_of(900, 10) == 9);
  CHECK(rank_of(950, 100) == 95 && rank_of(990, 101) == 100 && rank_of(500, 0) == 1);
  CHECK(rank_of(990, 0xffffffffull) == (990ull * 0xffffffffull + 999ull) / 1000ull);
  CHECK(quantile_permille(0) == 500 && quantile_permille(3) == 990 && le_edge(6) == 2000.0f);

  // configuration
  Config ok;
  validate(ok);
  auto bad = [](auto set) {
    Config c;
    set(c);
    return throws<std::invalid_argument>([&] { validate(c); });
  };
  CHECK(bad([](Config& c) { c.windows = 0; }) && bad([](Config& c) { c.windows = 4097; }));
  CHECK(bad([](Config& c) { c.group_cap = 0; }) && bad([](Config& c) { c.group_cap = 65537; }));
  CHECK(bad([](Config& c) { c.n_buffers = 0; }) && bad([](Config& c) { c.n_buffers = 65; }));
  CHECK(bad([](Config& c) { c.span_cap = 0; }) && bad([](Config& c) { c.span_cap = (1 << 24) + 1; }));
  CHECK(bad([](Config& c) { c.span_cap = 1 << 20, c.windows = 4096, c.group_cap = 1; }));  // 2^32: would wrap
  CHECK(!bad([](Config& c) { c.span_cap = (1 << 20) - 1, c.windows = 4096, c.group_cap = 1; }));
  CHECK(bad([](Config& c) { c.windows = 4096, c.group_cap = 512, c.span_cap = 16; }));     // > 2 GiB
  CHECK(!bad([](Config& c) { c.windows = 1, c.group_cap = 65536; }) && !bad([](Config& c) { c.windows = 4096; }));
  {
    Config c;
    c.windows = 300, c.group_cap = 64;
    CHECK(device_bytes(c) == size_t(302) * 64 * kRowStride * 4);
  }

  // the result block: its parts back to back, a whole number of 16-byte stores
  for (int g : {1, 3, 64, 1500, 65536}) {
    const Layout l = layout(g);
    const size_t G = (size_t)g;
    CHECK(l.n == 0 && l.sum == G && l.le == 3 * G && l.q_win == 11 * G && l.n_roll == 15 * G && l.q_roll == 16 * G);
    CHECK(l.stats == 20 * G && l.words >= l.stats + kStats && l.words % 4 == 0 && l.words - (l.stats + kStats) < 4);
    std::vector<uint32_t> block(l.words, 0u);  // every word of it is addressable
    block[l.q_roll + kQuantiles * (G - 1) + kQuantiles - 1] = 1;
    block[l.stats + kOutOfGroup] = 2;
    block[l.words - 1] += 3;
    CHECK(block[l.stats - 1] == 1);
  }

  // span ranges and step arguments
  std::vector<uint8_t> ring(64 * 8);
  const uintptr_t base = reinterpret_cast<uintptr_t>(ring.data());
  CHECK(plan_ranges({}, 4) == 0);
  CHECK(plan_ranges({{base, 128}, {0, 0}, {base + 256, 64}}, 4) == 3);
  CHECK(plan_ranges({{base, 64}, {base + 64, 128}, {base + 192, 64}}, 4) == 4);
  CHECK(throws<std::invalid_argument>([&] { plan_ranges({{base, 320}}, 4); }));
  CHECK(throws<std::invalid_argument>([&] { plan_ranges({{base, 192}, {base, 128}}, 4); }));
  CHECK(throws<std::invalid_argument>([&] { plan_ranges({{base, 63}}, 4); }));
  CHECK(throws<std::invalid_argument>([&] { plan_ranges({{0, 64}}, 4); }));
  CHECK(throws<std::invalid_argument>([&] { plan_ranges({{base, ~size_t(0) & ~size_t(63)}}, 4); }));
  check_step(0, 4);
  check_step(4, 4);
  CHECK(throws<std::invalid_argument>([] { check_step(5, 4); }));
  CHECK(throws<std::invalid_argument>([] { check_step(-1, 4); }));

  // the result slots (openreq::SlotRing): the last n steps stay readable
  for (int n : {1, 3}) {
    mislo::openreq::SlotRing r(n);
    for (int64_t i = 0; i < 20; ++i) {
      CHECK(r.begin() == (int)(i % n));
      for (int64_t j = -1; j <= i + 1; ++j) CHECK(r.holds(j) == (j >= 0 && j <= i && j > i - n));
    }
    CHECK(throws<std::out_of_range>([&] { r.slot_of(19 - n); }));
  }
  std::printf("slisketch host ok\n");
  return 0;
}
