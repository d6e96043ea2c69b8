// Stand-alone check of the TTFT drift tracker's host side (ops/csrc/drift_host.h), built with
// -fsanitize=address,undefined by tests/test_drift.py: the layout's offsets (printed, compared with
// the Python mirror), validate() and its messages, the range and step checks, the wave reduction's
// packing and the decision arithmetic at the edges of 64 bits. No device, no Python.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>

#include "drift_host.h"

using namespace mislo::drift;

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

template <class F>
static std::string refused(F f) {
  try {
    f();
  } catch (const std::invalid_argument& e) {
    return e.what();
  }
  return "";
}

static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

int main() {
  // the layout: every array on 16 bytes, in the documented order
  for (int g : {1, 2, 3, 4, 5, 64, 65536}) {
    const Layout l = layout(g);
    std::printf("layout %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", g, l.n_win, l.n_recent, l.n_base,
                l.base_fill, l.q_recent, l.q_base, l.slow_num, l.fast_num, l.slow_at, l.fast_at, l.state, l.hold, l.stats,
                l.words);
    for (size_t at : {l.n_win, l.n_recent, l.n_base, l.base_fill, l.q_recent, l.q_base, l.slow_num, l.fast_num, l.slow_at,
                      l.fast_at, l.state, l.hold, l.stats, l.words})
      CHECK(at % 4 == 0);
    CHECK(l.n_recent - l.n_win >= (size_t)g && l.fast_num - l.slow_num >= 2 * (size_t)g && l.words == l.stats + kStats);
  }
  CHECK(kK == 386 && kRowStride == 392 && kPerLane == 7 && kRowLanes == 56 && kLdsSlots == 256);

  // validate
  Config ok;
  validate(ok);
  CHECK(state_rows(ok) == 323 && device_bytes(ok) == 323ull * 64 * 392 * 4 + 16384ull * 64 + layout(64).words * 4);
  auto bad = [&](auto set, const char* what) {
    Config c;
    set(c);
    const std::string m = refused([&] { validate(c); });
    if (!has(m, what)) std::fprintf(stderr, "expected '%s' in '%s'\n", what, m.c_str());
    CHECK(has(m, what));
  };
  bad([](Config& c) { c.recent = 0; }, "recent windows");
  bad([](Config& c) { c.recent = 1025; }, "recent windows");
  bad([](Config& c) { c.gap = 0; }, "gap windows");
  bad([](Config& c) { c.gap = 1025; }, "gap windows");
  bad([](Config& c) { c.baseline = 0; }, "baseline windows");
  bad([](Config& c) { c.baseline = 4097; }, "baseline windows");
  bad([](Config& c) { c.group_cap = 0; }, "group_cap");
  bad([](Config& c) { c.group_cap = 65537; }, "group_cap");
  bad([](Config& c) { c.span_cap = 0; }, "span_cap");
  bad([](Config& c) { c.span_cap = 1 << 16; c.recent = 64; c.baseline = 64; }, "slow_num << 16 would wrap");
  bad([](Config& c) { c.span_cap = std::numeric_limits<int>::max(); c.recent = 1; c.baseline = 1; }, "below 2^44");
  bad([](Config& c) { c.n_buffers = 0; }, "n_buffers");
  bad([](Config& c) { c.n_buffers = 65; }, "n_buffers");
  bad([](Config& c) { c.crit = 0.0; }, "crit");
  bad([](Config& c) { c.crit = -1.0; }, "crit");
  bad([](Config& c) { c.crit = std::numeric_limits<double>::quiet_NaN(); }, "crit");
  bad([](Config& c) { c.crit = std::numeric_limits<double>::infinity(); }, "crit");
  bad([](Config& c) { c.min_shift = -1; }, "min_shift");
  bad([](Config& c) { c.min_shift = 386; }, "min_shift");
  bad([](Config& c) { c.min_recent = 0; }, "min_recent");
  bad([](Config& c) { c.min_base = 0; }, "min_recent");
  bad([](Config& c) { c.min_base_windows = 0; }, "min_recent");
  bad([](Config& c) { c.hold_max = 0; }, "hold_max");
  bad([](Config& c) { c.group_cap = 65536; c.baseline = 4096; }, "2 GiB");
  {
    Config c;  // one below the wrap bound: 2^16 squared x 64 x 63 < 2^44
    c.span_cap = 1 << 16;
    c.recent = 64;
    c.baseline = 63;
    c.group_cap = 1;
    validate(c);
    c.recent = c.gap = 1;
    c.baseline = 1;
    c.span_cap = (1 << 22) - 1;
    c.min_shift = 385;
    c.n_buffers = 64;
    validate(c);
  }

  // ranges and steps
  std::vector<Range> r = {{0x1000, 64 * 10}, {0x2000, 0}, {0, 0}, {0x3000, 64 * 6}};
  CHECK(plan_ranges(r, 16) == 16);
  CHECK(has(refused([&] { plan_ranges(r, 15); }), "more spans than span_cap"));
  CHECK(has(refused([&] { plan_ranges({{0x1000, 63}}, 16); }), "not whole 64-byte spans"));
  CHECK(has(refused([&] { plan_ranges({{0, 64}}, 16); }), "null range"));
  check_step(0, 4);
  check_step(4, 4);
  CHECK(has(refused([&] { check_step(5, 4); }), "n_groups out of range"));
  CHECK(has(refused([&] { check_step(-1, 4); }), "n_groups out of range"));

  // the reduction's operand: larger numerator first, then the lower bucket; exact at the largest numerator
  const uint64_t top = (uint64_t(1) << 44) - 1;
  CHECK(pack_max(5, 10) > pack_max(5, 11) && pack_max(6, 385) > pack_max(5, 0) && pack_max(1, 385) > pack_max(0, 0));
  for (uint32_t b : {0u, 6u, 7u, 385u})
    for (uint64_t n : {uint64_t(1), uint64_t(12345), top}) CHECK(packed_num(pack_max(n, b)) == n && packed_bucket(pack_max(n, b)) == b);
  CHECK(lds_group(lds_key(65535, 385)) == 65535 && lds_bucket(lds_key(65535, 385)) == 385 && lds_key(0, 0) != 0);

  // crit_q: round(c^2 2^32), saturating
  CHECK(crit_q(4.0) == (uint64_t(4) << 32) && crit_q(5.0 - 1.0 / 4294967296.0) == (uint64_t(5) << 32) - 1);
  CHECK(crit_q(1e-12) == 0 && crit_q(1e30) == ~uint64_t(0) && crit_q(0.25 / 4294967296.0) == 0 && crit_q(0.5 / 4294967296.0) == 1);

  // the decision: disjoint rows of 10 give Dq = 2^16, n_e = 5, Dq Dq n_e = 5 * 2^32
  Thresholds t;
  t.min_recent = t.min_base = 2;
  t.min_base_windows = 1;
  const uint32_t lo[4] = {100, 100, 100, 100}, hi[4] = {200, 200, 200, 200};
  t.crit_q = uint64_t(5) << 32;
  CHECK(!significant(100, 10, 10, t.crit_q) && decide(10, 10, 1, 100, 0, hi, lo, t) == 0);
  t.crit_q -= 1;
  CHECK(significant(100, 10, 10, t.crit_q) && decide(10, 10, 1, 100, 0, hi, lo, t) == kSlow);
  CHECK(decide(10, 10, 1, 0, 100, lo, hi, t) == kFast && decide(10, 10, 1, 100, 100, hi, lo, t) == kSlow);
  CHECK(decide(1, 10, 1, 10, 0, hi, lo, t) == kWarming && decide(10, 1, 1, 10, 0, hi, lo, t) == kWarming);
  CHECK(decide(10, 10, 0, 100, 0, hi, lo, t) == kWarming && decide(0, 0, 5, 0, 0, hi, lo, t) == kWarming);
  // the shift condition: p50 or p90, at s - 1, s, s + 1; kEmpty-sized sums do not wrap
  const uint32_t a1[4] = {101, 100, 0, 0}, a2[4] = {102, 100, 0, 0}, p2[4] = {100, 102, 0, 0}, p3[4] = {100, 103, 0, 0};
  CHECK(decide(10, 10, 1, 100, 0, a1, lo, t) == 0 && decide(10, 10, 1, 100, 0, a2, lo, t) == kSlow);
  CHECK(decide(10, 10, 1, 100, 0, p2, lo, t) == kSlow && decide(10, 10, 1, 100, 0, p3, lo, t) == kSlow);
  CHECK(!shifted(0, 0, kEmpty, kEmpty, 385) && shifted(kEmpty, 0, kEmpty - 1, 0, 1));
  // the largest operands validate() admits: n_r n_b just below 2^44, the numerator all of it
  const uint32_t nr = (1u << 22) - 1, nb = 1u << 22;
  const uint64_t nn = (uint64_t)nr * nb;
  CHECK(nn < (uint64_t(1) << 44) && ((nn << 16) >> 16) == nn);
  t.crit_q = ~uint64_t(0) - 1;
  CHECK(!significant(nn, nr, nb, t.crit_q));  // Dq = 2^16, n_e < 2^22: the product stays below 2^54
  t.crit_q = (uint64_t(1) << 32) * ((nn / ((uint64_t)nr + nb))) - 1;
  CHECK(significant(nn, nr, nb, t.crit_q) && !significant(nn, nr, nb, t.crit_q + 1) && !significant(0, nr, nb, 0));
  t.min_recent = t.min_base = 0xffffffffu;
  CHECK(decide(0xfffffffeu, 0xffffffffu, 1, 0, 0, hi, lo, t) == kWarming);

  std::printf("drift host ok\n");
  return 0;
}
