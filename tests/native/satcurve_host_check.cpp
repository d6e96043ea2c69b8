// The saturation curve tracker's host side (ops/csrc/satcurve_host.h: the placement it takes from the load
// tracker at its boundaries, the level rule over every u against lower(), the fold's order by lanes against
// the recurrence, the generations' epochs, the knee against __int128 at the bounds' extremes, the state,
// age, the row, the configuration and argument checks, the result block's layout and both population
// bounds) on its own, for the host sanitizers: tests/test_satcurve.py builds this with
// -fsanitize=address,undefined, runs it and compares the lines it prints with pipeline/satcurve.py's.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "satcurve_host.h"

using namespace mislo::satcurve;
namespace loadsli = mislo::loadsli;
namespace onset = mislo::onset;
namespace decodesli = mislo::decodesli;
namespace errsli = mislo::errsli;

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

typedef __int128 i128;

// the knee in 128 bits, every level tried directly
static Knee wide(const uint64_t* c, int64_t budget, int64_t min_requests) {
  i128 S[kK + 1];
  S[kK] = 0;
  for (int l = kK - 1; l >= 0; --l) S[l] = S[l + 1] + (i128)c[2 * l + 1] * 1000000 - (i128)budget * (i128)c[2 * l];
  i128 top = 0;
  for (int l = 0; l < kK; ++l) top = S[l] > top ? S[l] : top;
  Knee k{kNone, 0, 0, false};
  if (top <= 0) return k;
  for (int l = 0; l < kK; ++l)
    if (S[l] == top) k.level = (uint32_t)l;
  for (int l = (int)k.level; l < kK; ++l) k.n += c[2 * l], k.b += c[2 * l + 1];
  k.valid = k.n >= (uint64_t)min_requests;
  return k;
}

static bool same(const Knee& a, const Knee& b) { return a.level == b.level && a.n == b.n && a.b == b.b && a.valid == b.valid; }

static uint64_t rnd(uint64_t& x) {  // splitmix64
  uint64_t z = (x += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

int main() {
  const int64_t bin = 1000;
  const uint32_t B = 64;
  // the placement decides where the third cell goes: only with kPStart
  {
    const int64_t q_hi = 1000, oldest = q_hi - 63;
    loadsli::Placement p = loadsli::place(q_hi * bin + 5, 300, bin, q_hi, B);
    CHECK(p.bits == (loadsli::kPStart | loadsli::kPEnd) && p.qs == q_hi && p.qe == q_hi);
    p = loadsli::place((q_hi + 2) * bin, 10, bin, q_hi, B);  // a future start: placed at q_hi
    CHECK(p.bits == (loadsli::kPFuture | loadsli::kPStart | loadsli::kPEnd) && p.qs == q_hi && p.idle_s + p.idle_e == (uint64_t)bin);
    p = loadsli::place((q_hi - 1) * bin + 300, 5000, bin, q_hi, B);  // a future end
    CHECK(p.bits == (loadsli::kPFuture | loadsli::kPStart | loadsli::kPEnd) && p.qs == q_hi - 1 && p.qe == q_hi);
    p = loadsli::place((oldest - 7) * bin, 2000, bin, q_hi, B);
    CHECK(p.bits == loadsli::kPTooOld);
    p = loadsli::place((oldest - 7) * bin + 500, 10000, bin, q_hi, B);  // clipped: no start, so no sli
    CHECK(p.bits == (loadsli::kPClipped | loadsli::kPEnd) && p.qe == oldest + 3);
    p = loadsli::place(oldest * bin, 0, bin, q_hi, B);
    CHECK(p.bits == (loadsli::kPStart | loadsli::kPEnd) && p.qs == oldest);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    CHECK(!has_ttft(nan) && !has_ttft(-1.f) && !has_ttft(-inf) && has_ttft(-0.f) && has_ttft(0.f) && has_ttft(inf));
    CHECK(sli_add(800.f, 800.f) == 1ull && sli_add(std::nextafter(800.f, inf), 800.f) == ((1ull << 32) | 1ull));
    CHECK(sli_n((7ull << 32) | 9ull) == 9 && sli_b((7ull << 32) | 9ull) == 7);
  }
  // the level rule over every u: monotone, onto 0 .. kK - 1, lower() its inverse on the left edges
  {
    uint32_t prev = 0;
    for (uint32_t u = 0; u <= kMaxU; ++u) {
      const uint32_t l = level_of_u(u);
      CHECK(l < (uint32_t)kK && l >= prev && l <= prev + 1 && lower_u(l) <= u && u < lower_u(l + 1));
      if (u < 16) CHECK(l == u);
      prev = l;
    }
    CHECK(prev == kK - 1 && level_of_u(15) == 15 && level_of_u(16) == 16 && level_of_u(17) == 17 && level_of_u(31) == 31 &&
          level_of_u(32) == 32 && level_of_u(33) == 32 && level_of_u(kMaxU) == 159 && lower_u(kK) == kMaxU + 1);
    for (uint32_t l = 0; l < (uint32_t)kK; ++l) CHECK(level_of_u(lower_u(l)) == l);
    // u from a busy time: floor, clamped; the bound's extreme does not overflow
    CHECK(u_of(1874, 1000) == 14 && u_of(1875, 1000) == 15 && u_of(1999, 1000) == 15 && u_of(2000, 1000) == 16);
    CHECK(u_of(1023874, 1000) == 8190 && u_of(1023875, 1000) == 8191 && u_of(1100000, 1000) == 8191 && u_of(0, 1000) == 0);
    CHECK(u_of(-3, 1000) == 0 && u_of(int64_t(1) << 53, 1000) == kMaxU && u_of(int64_t(1) << 53, int64_t(1) << 53) == 8);
    CHECK(level_of(2, loadsli::kStartAdd, 125, 1000) == level_of_u(23));  // 3 active, 125 us idle: busy 2875
    for (const int64_t b : {int64_t(1000), int64_t(500000), int64_t(60000000)})
      std::printf("level %lld %u %u %u\n", (long long)b, u_of(b * 3 / 2, b), level_of_u(u_of(b * 37, b)), level_of_u(u_of(b * 2000, b)));
  }
  // the fold's order: lanes owning consecutive evicted bins, an inclusive scan of starts - ends from carry,
  // against the plain recurrence, for every count
  {
    uint64_t seed = 11;
    for (uint32_t count = 1; count <= 2 * B; count += (count < 70 ? 1 : 13)) {
      std::vector<uint64_t> counts(count), idle(count);
      std::vector<uint32_t> want(count), got(count);
      int64_t A = 5 + (int64_t)(rnd(seed) % 4), carry = A;
      for (uint32_t j = 0; j < count; ++j) {
        const uint32_t starts = (uint32_t)(rnd(seed) % 5), ends = (uint32_t)(rnd(seed) % (uint64_t)(A + starts + 1));
        counts[j] = (uint64_t)starts * loadsli::kStartAdd + (uint64_t)ends * loadsli::kEndAdd;
        idle[j] = rnd(seed) % (uint64_t)((starts + ends) * bin + 1) % (uint64_t)((A + starts) * bin + 1);
        want[j] = level_of(A, counts[j], idle[j], bin);
        A += loadsli::cell_delta(counts[j]);
      }
      const uint32_t per = (count + 63) / 64;
      int64_t run[64];
      for (uint32_t lane = 0; lane < 64; ++lane) {
        run[lane] = 0;
        for (uint32_t j = std::min(lane * per, count); j < std::min(lane * per + per, count); ++j) run[lane] += loadsli::cell_delta(counts[j]);
      }
      for (int d = 1; d < 64; d <<= 1)  // the wave's inclusive scan, every lane reading the old values
        for (int lane = 63; lane >= d; --lane) run[lane] += run[lane - d];
      for (uint32_t lane = 0; lane < 64; ++lane) {
        int64_t a = carry + (lane ? run[lane - 1] : 0);
        for (uint32_t j = std::min(lane * per, count); j < std::min(lane * per + per, count); ++j) {
          got[j] = level_of(a, counts[j], idle[j], bin);
          a += loadsli::cell_delta(counts[j]);
        }
      }
      CHECK(got == want && carry + run[63] == A);
    }
  }
  // what an advance evicts and folds; the generations' epochs
  {
    const int64_t q = 6400;  // an epoch edge of 64 and of 128
    Fold f = fold_of(kNoBin, q, kNoBin, B);
    CHECK(f.count == 0 && f.lo > f.hi);
    f = fold_of(q, q, q, B);
    CHECK(f.count == 0 && f.lo > f.hi);
    f = fold_of(q, q + 1, q, B);
    CHECK(f.count == 1 && f.first == q - 63 && f.hi == q - 63 && f.lo > f.hi);  // evicted, before q_first: not folded
    f = fold_of(q + 63, q + 65, q, B);
    CHECK(f.count == 2 && f.first == q && f.lo == q && f.hi == q + 1);          // exactly q_first folds
    f = fold_of(q + 62, q + 64, q, B);
    CHECK(f.count == 2 && f.first == q - 1 && f.lo == q && f.hi == q);          // one bin before it does not
    f = fold_of(q + 70, q + 500, q, B);
    CHECK(f.count == B && f.first == q + 7 && f.lo == q + 7 && f.hi == q + 70);  // a jump: the whole ring
    Generations g;
    CHECK(g.begin(fold_of(q, q + 1, q, B), 64) == 0 && g.epoch[0] == -1);
    CHECK(g.begin(fold_of(q + 40, q + 83, q, B), 64) == 1u && g.epoch[0] == 100 && g.epoch[1] == -1);
    CHECK(g.begin(fold_of(q + 83, q + 146, q, B), 64) == 2u && g.epoch[0] == 100 && g.epoch[1] == 101);  // both epochs, one new
    CHECK(g.live(epoch_now(q + 146 - 63, 64)) == 3u && g.live(102) == 2u && g.live(103) == 0u && g.live(100) == 1u);
    CHECK(g.begin(fold_of(q + 146, q + 200, q, B), 64) == 1u && g.epoch[0] == 102);
    Generations h;
    CHECK(h.begin(fold_of(q + 120, q + 200, q + 10, B), 64) == 3u && h.epoch[0] == 100 && h.epoch[1] == 101);
    CHECK(h.begin(fold_of(q + 200, q + 201, q + 10, B), 64) == 1u && h.epoch[0] == 102);
    CHECK(epoch_now(0, 64) == 0 && epoch_now(1, 64) == 0 && epoch_now(65, 64) == 1 && epoch_now(64, 64) == 0);
    CHECK(!gen_live(-1, 0) && gen_live(0, 0) && gen_live(0, 1) && !gen_live(0, 2) && !gen_live(2, 1));
  }
  // the knee: hand-built curves, then 64 bits against 128 at random and at the bounds' extremes
  {
    std::vector<uint64_t> c(kK * 2, 0);
    CHECK(same(knee_of(c.data(), 100000, 1), Knee{kNone, 0, 0, false}));
    c[2 * 40] = 10, c[2 * 40 + 1] = 1;  // d = 0: inside the budget at equality
    CHECK(knee_of(c.data(), 100000, 1).level == kNone && knee_of(c.data(), 99999, 1).level == 40);
    c[2 * 80] = 8, c[2 * 80 + 1] = 2, c[2 * 60] = 4, c[2 * 20] = 6, c[2 * 20 + 1] = 1;  // S = 12 at 80 and at 20
    Knee k = knee_of(c.data(), 100000, 8);
    CHECK(k.level == 80 && k.n == 8 && k.b == 2 && k.valid && !knee_of(c.data(), 100000, 9).valid);
    CHECK(score(10, 1, 100000) == 0 && score(0, 0, 5) == 0 && score(1, 1, 999999) == 1);
    uint64_t seed = 3;
    for (int it = 0; it < 4000; ++it) {
      std::fill(c.begin(), c.end(), 0);
      const bool extreme = it % 4 == 0;
      uint64_t left = kMaxCurveRecords;
      const int levels = 1 + (int)(rnd(seed) % 12);
      for (int i = 0; i < levels && left; ++i) {
        const int l = i == 0 && extreme ? kK - 1 : (int)(rnd(seed) % kK);
        const uint64_t n = extreme ? (i == 0 ? left - (left > 1 ? rnd(seed) % 2 : 0) : rnd(seed) % (left + 1)) : rnd(seed) % 1000;
        if (c[2 * l] || !n) continue;
        left -= extreme ? n : 0;
        c[2 * l] = n;
        const uint64_t r = rnd(seed) % 4;
        c[2 * l + 1] = r == 0 ? 0 : r == 1 ? n : r == 2 ? n / 10 : rnd(seed) % (n + 1);
      }
      const int64_t budget = it % 3 == 0 ? 1 : it % 3 == 1 ? 999999 : 1 + (int64_t)(rnd(seed) % 999999);
      const int64_t min_requests = 1 + (int64_t)(rnd(seed) % 2000);
      CHECK(same(knee_of(c.data(), budget, min_requests), wide(c.data(), budget, min_requests)));
    }
    std::fill(c.begin(), c.end(), 0);
    c[2 * 159] = c[2 * 159 + 1] = kMaxCurveRecords;  // 2^40 breaches at budget 1: S just under 2^60
    k = knee_of(c.data(), 1, kMaxMinRequests);
    CHECK(same(k, wide(c.data(), 1, kMaxMinRequests)) && k.level == 159 && k.n == (uint64_t)kMaxCurveRecords && k.valid);
    c[2 * 159 + 1] = 0;  // 2^40 clean requests at the largest budget: S just above -2^60, no knee
    CHECK(same(knee_of(c.data(), 999999, 1), wide(c.data(), 999999, 1)) && knee_of(c.data(), 999999, 1).level == kNone);
  }
  // state and age
  {
    CHECK(state_of(false, 100, 4, true, 9, 5) == kUnknown && state_of(true, 3, 4, true, 9, 5) == kUnknown);
    CHECK(state_of(true, 4, 4, false, 9, kNone) == kNoKnee && state_of(true, 4, 4, true, 4, 5) == kBelow);
    CHECK(state_of(true, 4, 4, true, 5, 5) == kSaturated && state_of(true, 4, 4, true, 6, 5) == kSaturated);
    CHECK(age_of(kSaturated, 0) == 1 && age_of(kSaturated, 7) == 8 && age_of(kSaturated, 0xffffffffu) == 0xffffffffu &&
          age_of(kSaturated, 0xfffffffeu) == 0xffffffffu && age_of(kBelow, 7) == 0 && age_of(kUnknown, 7) == 0 &&
          age_of(kNoKnee, 7) == 0);
    const Ranges r = ranges_of(1000, 987, B, 2, 4);
    CHECK(r.oldest == 937 && r.lo == 987 && r.settled_hi == 998 && r.recent_lo == 995 && r.recent_hi == 998 && r.recent_known);
    CHECK(!ranges_of(1000, 996, B, 2, 4).recent_known && ranges_of(1000, 995, B, 2, 4).recent_known);
    CHECK(errsli::budget_ppm(0.99) == 10000);
  }
  // the row, the layout, the configuration and argument checks
  {
    CHECK(offsetof(Row, n_total) == 16 && offsetof(Row, n_knee) == 32 && offsetof(Row, busy_recent) == 48 && offsetof(Row, age) == 56);
    for (const int g : {1, 3, 4, 5, 64, 1000, 65536}) {
      const Layout l = layout(g);
      CHECK(l.rows == 0 && l.curve * 4 % 16 == 0 && l.stats * 4 % 16 == 0 && l.words % 4 == 0 && l.words >= l.stats + kStats);
      std::printf("layout %d %zu %zu %zu %zu\n", g, l.rows, l.curve, l.stats, l.words);
    }
    std::printf("device_bytes %llu\n", (unsigned long long)device_bytes(1024, 16384, 64));
    Config ok;
    validate(ok);
    auto bad = [](auto edit) {
      Config c;
      edit(c);
      return throws<std::invalid_argument>([&] { validate(c); });
    };
    CHECK(bad([](Config& c) { c.bins = 32; }) && bad([](Config& c) { c.bins = 96; }) && bad([](Config& c) { c.bins = 16384; }));
    CHECK(bad([](Config& c) { c.bin_us = 999; }) && bad([](Config& c) { c.bin_us = 60000001; }));
    CHECK(bad([](Config& c) { c.settle_bins = -1; }) && bad([](Config& c) { c.recent_bins = 0; }));
    CHECK(bad([](Config& c) { c.settle_bins = 995; }) && !bad([](Config& c) { c.settle_bins = 994; }));
    CHECK(bad([](Config& c) { c.epoch_bins = 1023; }) && !bad([](Config& c) { c.epoch_bins = 1024; }) &&
          bad([](Config& c) { c.epoch_bins = int64_t(1) << 31; }) && !bad([](Config& c) { c.epoch_bins = kMaxEpochBins; }));
    CHECK(bad([](Config& c) { c.budget_ppm = 0; }) && bad([](Config& c) { c.budget_ppm = 1000000; }) &&
          !bad([](Config& c) { c.budget_ppm = 999999; }));
    CHECK(bad([](Config& c) { c.min_requests = 0; }) && bad([](Config& c) { c.min_requests = int64_t(1) << 31; }));
    CHECK(bad([](Config& c) { c.slo_ms = -1.0; }) && bad([](Config& c) { c.slo_ms = std::numeric_limits<double>::quiet_NaN(); }));
    CHECK(bad([](Config& c) { c.group_cap = 0; }) && bad([](Config& c) { c.group_cap = 65537; }) && bad([](Config& c) { c.span_cap = 0; }));
    CHECK(bad([](Config& c) { c.n_buffers = 0; }) && bad([](Config& c) { c.n_buffers = 65; }));
    CHECK(bad([](Config& c) { c.group_cap = 16384, c.bins = 8192, c.epoch_bins = 8192, c.ring_records_max = 1; }));  // 2 GiB
    CHECK(bad([](Config& c) { c.ring_records_max = 0; }) && bad([](Config& c) { c.ring_records_max = 17592187; }) &&
          !bad([](Config& c) { c.ring_records_max = 17592186; }));
    CHECK(bad([](Config& c) { c.curve_records_max = 0; }) && bad([](Config& c) { c.curve_records_max = kMaxCurveRecords + 1; }));
    int x = 0;
    const uintptr_t a = (uintptr_t)&x;
    CHECK(plan_ranges({{a, 64}, {a, 0}, {0, 0}, {a, 128}}, 3) == 3);
    CHECK(throws<std::invalid_argument>([&] { plan_ranges({{a, 63}}, 8); }));
    CHECK(throws<std::invalid_argument>([&] { plan_ranges({{0, 64}}, 8); }));
    CHECK(throws<std::invalid_argument>([&] { plan_ranges({{a, 128}, {a, 128}}, 3); }));
    CHECK(throws<std::invalid_argument>([] { check_step(0, 1, 4); }) && throws<std::invalid_argument>([] { check_step(5, 5, 4); }) &&
          throws<std::invalid_argument>([] { check_step(5, -1, 4); }));
    check_step(1, 4, 4);
  }
  // the two bounds
  {
    RingPopulation ring(B, 300);
    ring.take(1000, 128), ring.take(1008, 128);
    CHECK(ring.after(1016, 44) == 300 && ring.after(1016, 45) == 301 && ring.after(1064, 128) == 256);
    CHECK(throws<std::invalid_argument>([&] { ring.check(1016, 45); }));
    ring.check(1016, 44);
    CurvePopulation curve(64, 300);  // epochs of 64 bins: 6400 is an edge
    curve.take(6400, 100), curve.take(6410, 28), curve.take(6464, 128);
    CHECK(curve.epochs() == 2 && curve.after(6528, 44) == 300 && curve.after(6528, 45) == 301);
    CHECK(throws<std::invalid_argument>([&] { curve.check(6528, 45); }));
    curve.check(6528, 44);
    CHECK(curve.after(6592, 128) == 256 && curve.after(6656, 300) == 300);  // one, then two epochs later
    curve.take(6592, 0);
    CHECK(curve.epochs() == 1);
    std::printf("curve_records_max %lld\n", (long long)kMaxCurveRecords);
  }
  std::printf("satcurve host ok\n");
  return 0;
}
