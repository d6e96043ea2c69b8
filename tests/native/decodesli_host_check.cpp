// The host side of the decode SLI tracker (ops/csrc/decodesli_host.h) on its own: the bucket and
// lower rules over the whole range, the representative, the SLO's unit, the table's cell, the LDS key,
// validate, layout, plan_ranges and check_step. Built with the host sanitizers by tests/test_decodesli.py.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>

#include "decodesli_host.h"

using namespace mislo::decodesli;

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

int main() {
  // every value: inside its bucket's edges, buckets never go back, 336 of them
  uint32_t prev = 0;
  for (uint32_t u = 1; u <= kTpotMax; ++u) {
    const uint32_t b = bucket_of(u);
    CHECK(b < (uint32_t)kK && b >= prev && b <= prev + 1);
    CHECK(lower(b) <= u && u < lower(b + 1));
    prev = b;
  }
  CHECK(prev == (uint32_t)kK - 1 && lower(kK) == (1u << 24));
  for (uint32_t b = 0; b < (uint32_t)kK; ++b) CHECK(bucket_of(lower(b)) == b || b == 0);
  CHECK(bucket_of(100000) == 216 && lower(216) == 98304 && lower(217) == 102400);
  CHECK(bucket_of(15) == 15 && bucket_of(16) == 16 && bucket_of(31) == 31 && bucket_of(32) == 32 && bucket_of(33) == 32);
  for (uint32_t b = 1; b < 16; ++b) CHECK(representative(b) == (double)b);
  for (uint32_t b = 16; b < (uint32_t)kK; ++b) {
    const double r = representative(b), lo = lower(b), hi = lower(b + 1) - 1;
    CHECK(r >= lo && r <= hi && r - lo <= lo / 32.0 && hi - r <= lo / 32.0);
  }
  CHECK(tpot_of(0xffffffffu) == kTpotMax && tpot_of(0xffu) == 0 && tpot_of((100000u << kTpotShift) | 0xfu) == 100000u);

  CHECK(tpot_slo_us(100.0) == 100000 && tpot_slo_us(0.0001) == 1 && tpot_slo_us(0.0014) == 1 && tpot_slo_us(0.0016) == 2);
  CHECK(tpot_slo_us(16777.2144) == 16777214u && tpot_slo_us(16777.215) == kTpotMax && tpot_slo_us(1e12) == kTpotMax);
  CHECK(cell_of(800.f, 800.f, 100000, 100000) == 0 && cell_of(800.0001f, 800.f, 100000, 100000) == 1);
  CHECK(cell_of(0.f, 800.f, 100001, 100000) == 2 && cell_of(1e9f, 800.f, kTpotMax, 100000) == 3);
  CHECK(cell_of(std::numeric_limits<float>::infinity(), 800.f, 1, 1) == 1);

  for (uint32_t g : {0u, 1u, 63u, 65535u})
    for (uint32_t w : {0u, 335u, 336u, 339u, kSum}) {
      const uint64_t k = lds_key(g, w);
      CHECK(k != 0 && lds_group(k) == g && lds_what(k) == w && mislo::onset::lds_hash(k) < (uint32_t)kLdsSlots);
      std::printf("lds_hash %u %u %u\n", g, w, mislo::onset::lds_hash(k));
    }

  // layout: every array on 16 bytes, none overlapping, whole 16-byte stores
  for (int g : {1, 2, 3, 5, 8, 64, 65536}) {
    const Layout l = layout(g);
    const size_t at[] = {l.cells, l.cells_roll, l.sum, l.sum_roll, l.q_win, l.q_roll, l.stats, l.words};
    const size_t need[] = {4u * g, 4u * g, 2u * g, 2u * g, 4u * g, 4u * g, (size_t)kStats};
    for (int i = 0; i < 7; ++i) CHECK(at[i] % 4 == 0 && at[i] + need[i] <= at[i + 1]);
    CHECK(l.cells == 0 && l.words % 4 == 0);
    std::printf("layout %d %zu %zu %zu %zu %zu %zu %zu %zu\n", g, l.cells, l.cells_roll, l.sum, l.sum_roll, l.q_win, l.q_roll,
                l.stats, l.words);
  }

  Config ok;
  validate(ok);
  const auto bad = [&](auto set) {
    Config c;
    set(c);
    return throws([&] { validate(c); });
  };
  CHECK(bad([](Config& c) { c.windows = 0; }) && bad([](Config& c) { c.windows = 4097; }));
  CHECK(bad([](Config& c) { c.group_cap = 0; }) && bad([](Config& c) { c.group_cap = 65537; }));
  CHECK(bad([](Config& c) { c.span_cap = 0; }) && bad([](Config& c) { c.n_buffers = 0; }) && bad([](Config& c) { c.n_buffers = 65; }));
  CHECK(bad([](Config& c) { c.slo_ms = -1.0; }) && bad([](Config& c) { c.slo_ms = std::numeric_limits<double>::quiet_NaN(); }));
  CHECK(bad([](Config& c) { c.slo_ms = std::numeric_limits<double>::infinity(); }));
  CHECK(bad([](Config& c) { c.tpot_slo_ms = 0.0; }) && bad([](Config& c) { c.tpot_slo_ms = -3.0; }));
  CHECK(bad([](Config& c) { c.tpot_slo_ms = std::numeric_limits<double>::quiet_NaN(); }));
  CHECK(bad([](Config& c) { c.tpot_slo_ms = std::numeric_limits<double>::infinity(); }));
  CHECK(bad([](Config& c) { c.span_cap = 1 << 21, c.windows = 2048; }));  // span_cap * windows = 2^32
  CHECK(bad([](Config& c) { c.group_cap = 65536, c.windows = 4096; }));   // far beyond 2 GiB
  CHECK(!bad([](Config& c) { c.windows = 1, c.group_cap = 1, c.span_cap = 1, c.n_buffers = 1, c.slo_ms = 0.0; }));
  CHECK(!bad([](Config& c) { c.windows = 4096, c.group_cap = 64; }));
  {
    Config c;
    CHECK(device_bytes(c) == 16384ull * 64 + 152ull * 64 * kStateWords * 4 + layout(64).words * 4);
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

  std::printf("decodesli host ok\n");
  return 0;
}
