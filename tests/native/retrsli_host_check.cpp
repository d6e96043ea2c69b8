// The host side of the TTFT phase split tracker (ops/csrc/retrsli_host.h) on its own: the unit conversions,
// the cell, the verdict (its 64-bit products against unsigned __int128 at the extremes), the age, the LDS
// key, validate, layout, plan_ranges and check_step. Given a file of questions (one a line: "u <float32
// bits, hex>", "b <double>", "c <tb> <r> <m> <slo_u> <budget_u>", "s <six cells> <sli> <min_requests>
// <coverage_ppm> <budget_ppm> <dominance_ppm>") it prints one answer a line, which the test compares with
// its own brute force. Built with the host sanitizers by tests/test_retrsli.py.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>

#include "retrsli_host.h"

using namespace mislo::retrsli;

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

// the verdict with every product in 128 bits
static uint32_t state_wide(const uint32_t* c, uint32_t sli, const Thresholds& th) {
  typedef unsigned __int128 u128;
  const u128 ppm = 1000000;
  u128 n = 0;
  for (int j = 0; j < kCells; ++j) n += c[j];
  if (n < th.min_requests || n * ppm < (u128)th.coverage_ppm * sli) return kUnknown;
  const u128 M = (u128)c[2] + c[3], R = c[4], B = M + R + c[5];
  if (B * ppm <= (u128)th.budget_ppm * n) return kStateOk;
  if (R * ppm >= (u128)th.dominance_ppm * B) return kRetrievalBound;
  if (M * ppm >= (u128)th.dominance_ppm * B) return kModelBound;
  return kMixed;
}

static int answer(const char* path) {
  std::FILE* f = std::fopen(path, "r");
  if (!f) return 1;
  char line[512];
  while (std::fgets(line, sizeof line, f)) {
    if (line[0] == 'u') {
      uint32_t bits = 0;
      if (std::sscanf(line + 1, "%" SCNx32, &bits) != 1) return 1;
      float ms;
      std::memcpy(&ms, &bits, 4);
      std::printf("u %u\n", units_of_ms(ms));
    } else if (line[0] == 'b') {
      double ms = 0;
      if (std::sscanf(line + 1, "%lf", &ms) != 1) return 1;
      std::printf("b %u\n", budget_units(ms));
    } else if (line[0] == 'c') {
      uint32_t tb, r, m, slo_u, budget_u;
      if (std::sscanf(line + 1, "%u %u %u %u %u", &tb, &r, &m, &slo_u, &budget_u) != 5) return 1;
      std::printf("c %u\n", cell_of(tb != 0, r, m, slo_u, budget_u));
    } else if (line[0] == 's') {
      uint32_t c[kCells], sli;
      Thresholds th;
      if (std::sscanf(line + 1, "%u %u %u %u %u %u %u %u %u %u %u", &c[0], &c[1], &c[2], &c[3], &c[4], &c[5], &sli,
                      &th.min_requests, &th.coverage_ppm, &th.budget_ppm, &th.dominance_ppm) != 11)
        return 1;
      if (state_of(c, sli, th) != state_wide(c, sli, th)) return 1;
      std::printf("s %u\n", state_of(c, sli, th));
    }
  }
  std::fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  // units: half to even, the clamp, what no record brings
  CHECK(units_of_ms(0.125f) == 12 && units_of_ms(0.375f) == 38 && units_of_ms(0.625f) == 62 && units_of_ms(800.f) == 80000);
  CHECK(units_of_ms(0.f) == 0 && units_of_ms(-0.f) == 0 && units_of_ms(0.004f) == 0 && units_of_ms(0.01f) == 1);
  CHECK(units_of_ms(1e7f) == kUnitMax && units_of_ms(std::numeric_limits<float>::infinity()) == kUnitMax);
  CHECK(units_of_ms(-1.f) == 0 && units_of_ms(std::numeric_limits<float>::quiet_NaN()) == 0);
  CHECK(budget_units(200.0) == 20000 && budget_units(1e-9) == 1 && budget_units(0.004) == 1 && budget_units(0.125) == 12 && budget_units(0.375) == 38);
  CHECK(budget_units(1e12) == kUnitMax && budget_units(167772.15) == kUnitMax && budget_units(167772.14) == kUnitMax - 1);
  CHECK(model_units(5, 5) == 0 && model_units(5, 6) == 0 && model_units(6, 5) == 1 && model_units(kUnitMax, 0) == kUnitMax);
  // rint is monotone: a TTFT at or below the SLO never converts above slo_u
  for (float slo : {0.f, 0.005f, 799.995f, 800.f, 1e6f}) {
    float v = slo;
    for (int i = 0; i < 64; ++i, v = std::nextafterf(v, 0.f)) CHECK(units_of_ms(v) <= units_of_ms(slo));
  }

  // cells
  CHECK(cell_of(false, 20000, 1, 80000, 20000) == kOk && cell_of(false, 20001, 1, 80000, 20000) == kOkSlowRetrieval);
  CHECK(cell_of(true, 20000, 80001, 80000, 20000) == kModel && cell_of(true, 20001, 80001, 80000, 20000) == kModelSlowRetrieval);
  CHECK(cell_of(true, 20001, 80000, 80000, 20000) == kRetrieval && cell_of(true, 20000, 80000, 80000, 20000) == kCombined);
  CHECK(cell_of(true, kUnitMax, 0, kUnitMax, kUnitMax) == kCombined && cell_of(true, kUnitMax, kUnitMax, 0, 1) == kModelSlowRetrieval);

  // the verdict at the extremes: counts of 2^32 - 1 (one cell at a time: their sum stays below 2^32), ppm values of 10^6
  const uint32_t big = 0xffffffffu;
  for (int hot = 0; hot < kCells; ++hot)
    for (uint32_t sli : {0u, 1u, big})
      for (uint32_t cov : {0u, 1u, 999999u, 1000000u})
        for (uint32_t bud : {1u, 999999u})
          for (uint32_t dom : {500001u, 1000000u})
            for (uint32_t mr : {1u, 0x7fffffffu}) {
              uint32_t c[kCells] = {0, 0, 0, 0, 0, 0};
              c[hot] = big;
              Thresholds th;
              th.min_requests = mr, th.coverage_ppm = cov, th.budget_ppm = bud, th.dominance_ppm = dom;
              CHECK(state_of(c, sli, th) == state_wide(c, sli, th));
              c[hot] = big - 5, c[(hot + 1) % kCells] = 5;
              CHECK(state_of(c, sli, th) == state_wide(c, sli, th));
            }
  {
    const uint32_t c[kCells] = {0, 0, 0, 0, big, 0};
    Thresholds th;
    th.coverage_ppm = 1000000;
    CHECK(state_of(c, big, th) == kRetrievalBound);
    CHECK((uint64_t)big * kPpm < (uint64_t(1) << 52));
  }
  CHECK(age_of(2, 2, 7) == 8 && age_of(2, 3, 7) == 1 && age_of(0, 0, 0) == 1 && age_of(1, 1, big) == big && age_of(1, 1, big - 1) == big);

  for (uint32_t g : {0u, 1u, 63u, 65535u})
    for (uint32_t w : {0u, 335u, 336u, 671u, kWhatCell, kWhatCell + 5u, kWhatSumR, kWhatSumT, kWhatSli}) {
      const uint64_t k = lds_key(g, w);
      CHECK(k != 0 && lds_group(k) == g && lds_what(k) == w && lds_hash(k) < (uint32_t)kLdsSlots);
    }
  CHECK(kLdsSlots == 1024 && kWhatSli == 680 && kStateWords == 684);

  // layout: every array on 16 bytes, none overlapping, whole 16-byte stores
  for (int g : {1, 2, 3, 5, 8, 64, 65536}) {
    const Layout l = layout(g);
    const size_t at[] = {l.cells, l.cells_roll, l.sum_r, l.sum_t, l.sum_r_roll, l.sum_t_roll, l.sli, l.sli_roll, l.q_r_win,
                         l.q_r_roll, l.q_m_win, l.q_m_roll, l.state, l.age, l.stats, l.words};
    const size_t G = (size_t)g;
    const size_t need[] = {8 * G, 8 * G, 2 * G, 2 * G, 2 * G, 2 * G, G, G, 4 * G, 4 * G, 4 * G, 4 * G, G, G, (size_t)kStats};
    for (int i = 0; i < 15; ++i) CHECK(at[i] % 4 == 0 && at[i] + need[i] <= at[i + 1]);
    CHECK(l.cells == 0 && l.words % 4 == 0);
    std::printf("layout %d", g);
    for (size_t x : at) std::printf(" %zu", x);
    std::printf("\n");
  }

  Config ok;
  validate(ok);
  const auto bad = [&](auto set) {
    Config c;
    set(c);
    return throws([&] { validate(c); });
  };
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  CHECK(bad([](Config& c) { c.windows = 0; }) && bad([](Config& c) { c.windows = 4097; }));
  CHECK(bad([](Config& c) { c.group_cap = 0; }) && bad([](Config& c) { c.group_cap = 65537; }));
  CHECK(bad([](Config& c) { c.span_cap = 0; }) && bad([](Config& c) { c.n_buffers = 0; }) && bad([](Config& c) { c.n_buffers = 65; }));
  CHECK(bad([](Config& c) { c.slo_ms = -1.0; }) && bad([&](Config& c) { c.slo_ms = nan; }) && bad([&](Config& c) { c.slo_ms = inf; }));
  CHECK(bad([](Config& c) { c.retrieval_budget_ms = 0.0; }) && bad([](Config& c) { c.retrieval_budget_ms = -3.0; }));
  CHECK(bad([&](Config& c) { c.retrieval_budget_ms = nan; }) && bad([&](Config& c) { c.retrieval_budget_ms = inf; }));
  CHECK(bad([](Config& c) { c.budget_ppm = 0; }) && bad([](Config& c) { c.budget_ppm = 1000000; }));
  CHECK(bad([](Config& c) { c.coverage_ppm = -1; }) && bad([](Config& c) { c.coverage_ppm = 1000001; }));
  CHECK(bad([](Config& c) { c.dominance_ppm = 500000; }) && bad([](Config& c) { c.dominance_ppm = 1000001; }));
  CHECK(bad([](Config& c) { c.min_requests = 0; }) && bad([](Config& c) { c.min_requests = int64_t(1) << 31; }));
  CHECK(bad([](Config& c) { c.span_cap = 1 << 21, c.windows = 2048; }));  // span_cap * windows = 2^32
  CHECK(bad([](Config& c) { c.group_cap = 65536, c.windows = 4096; }));   // far beyond 2 GiB
  CHECK(!bad([](Config& c) { c.windows = 1, c.group_cap = 1, c.span_cap = 1, c.n_buffers = 1, c.slo_ms = 0.0; }));
  CHECK(!bad([](Config& c) { c.budget_ppm = 1, c.coverage_ppm = 0, c.dominance_ppm = 500001, c.min_requests = 1; }));
  CHECK(!bad([](Config& c) { c.budget_ppm = 999999, c.coverage_ppm = 1000000, c.dominance_ppm = 1000000, c.min_requests = 0x7fffffff; }));
  CHECK(!bad([](Config& c) { c.windows = 4096, c.group_cap = 64; }));
  {
    Config c;
    CHECK(device_bytes(c) == 16384ull * 64 + 152ull * 64 * kStateWords * 4 + 64 * 2 * 4 + layout(64).words * 4);
    CHECK(thresholds(c).min_requests == 200 && thresholds(c).dominance_ppm == 667000);
    CHECK(mislo::errsli::budget_ppm(0.99) == 10000);
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

  if (argc > 1 && answer(argv[1]) != 0) {
    std::fprintf(stderr, "a question was not answered\n");
    return 1;
  }
  std::printf("retrsli host ok\n");
  return 0;
}
