// The load SLI tracker's host side (ops/csrc/loadsli_host.h: the duration rule on boundary bit patterns,
// the placement at its boundaries, the scan by runs of bins against the recurrence, the ranges, the
// three compares against unsigned __int128 at the bounds' extremes, age, the row, the configuration and
// argument checks, the result block's layout and the ring-population bound) on its own, for the host
// sanitizers: tests/test_loadsli.py builds this with -fsanitize=address,undefined, runs it and compares
// the lines it prints with pipeline/loadsli.py's.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "loadsli_host.h"

using namespace mislo::loadsli;
namespace onset = mislo::onset;

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

typedef unsigned __int128 u128;

// the three predicates in 128 bits
static uint32_t wide(const Sums& s, uint32_t nb, uint32_t nr, int64_t bin_us, int64_t f, int64_t min_requests,
                     int64_t min_conc_milli) {
  const u128 ar = s.arr_recent, ab = s.arr_base, F = (u128)f;
  uint32_t flags = 0;
  if (ar >= (u128)min_requests && ar * nb * 1000 >= F * ab * nr) flags |= kArrUp;
  if (ab * nr >= (u128)min_requests * nb && ar * nb * F <= (u128)1000 * ab * nr) flags |= kArrDown;
  const u128 cr = (u128)s.busy_recent * 1000 / ((u128)nr * (u128)bin_us), cb = (u128)s.busy_base * 1000 / ((u128)nb * (u128)bin_us);
  if (cr >= (u128)min_conc_milli && cr * 1000 >= F * cb) flags |= kConcUp;
  return flags;
}

static uint64_t rnd(uint64_t& x) {  // splitmix64
  uint64_t z = (x += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

int main() {
  const int64_t bin = 1000;
  const uint32_t B = 64;
  // the duration rule on boundary bit patterns: one double multiply, truncated
  {
    const float v[] = {0.f, 1e-4f, 0.9995f, 1.0005f, 799.9999f, 3.3333333f, 86400000.f};
    const int64_t want[] = {0, 0, 999, 1000, 799999, 3333, 86400000000ll};
    for (int i = 0; i < 7; ++i) {
      CHECK(latency_valid(v[i]) && dur_us_of(v[i]) == want[i]);
      std::printf("dur %a %lld\n", (double)v[i], (long long)dur_us_of(v[i]));
    }
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    CHECK(!latency_valid(nan) && !latency_valid(-1.f) && !latency_valid(inf) && !latency_valid(-inf));
    CHECK(!latency_valid(std::nextafter(86400000.f, inf)) && latency_valid(-0.f) && dur_us_of(-0.f) == 0);
    CHECK(ts_us_of(999) == 0 && ts_us_of(1000) == 1 && ts_us_of(1700000000123456789ll) == 1700000000123456ll);
  }
  // placement at its boundaries
  {
    const int64_t q_hi = 1700000000000ll + 100, oldest = q_hi - B + 1;
    CHECK(oldest == onset::oldest_bin(q_hi, B));
    Placement p = place((q_hi - 5) * bin + 100, 500, bin, q_hi, B);  // inside one bin
    CHECK(p.bits == (kPStart | kPEnd) && p.qs == q_hi - 5 && p.qe == q_hi - 5 && p.idle_s == 100 && p.idle_e == 400);
    p = place((q_hi - 5) * bin + 600, 2000, bin, q_hi, B);  // over three bins
    CHECK(p.bits == (kPStart | kPEnd) && p.qs == q_hi - 5 && p.qe == q_hi - 3 && p.idle_s == 600 && p.idle_e == 400);
    p = place((q_hi - 5) * bin + 500, 500, bin, q_hi, B);  // ends on the boundary: in the next bin, none of it busy
    CHECK(p.bits == (kPStart | kPEnd) && p.qe == q_hi - 4 && p.idle_s == 500 && p.idle_e == (uint64_t)bin);
    p = place((q_hi - 5) * bin + 250, 0, bin, q_hi, B);  // zero duration: idle for the whole bin
    CHECK(p.bits == (kPStart | kPEnd) && p.qs == p.qe && p.idle_s + p.idle_e == (uint64_t)bin);
    p = place((q_hi + 1) * bin, 700, bin, q_hi, B);  // a future start: zero-length in q_hi
    CHECK(p.bits == (kPFuture | kPStart | kPEnd) && p.qs == q_hi && p.qe == q_hi && p.idle_s == 0 && p.idle_e == (uint64_t)bin);
    p = place((q_hi + 1) * bin - 1, 0, bin, q_hi, B);  // the last microsecond of q_hi is not ahead
    CHECK(p.bits == (kPStart | kPEnd) && p.qs == q_hi && p.idle_s == 999 && p.idle_e == 1);
    p = place((q_hi - 1) * bin + 300, 5000, bin, q_hi, B);  // a future end: cut at the end of q_hi
    CHECK(p.bits == (kPFuture | kPStart | kPEnd) && p.qs == q_hi - 1 && p.qe == q_hi && p.idle_s == 300 && p.idle_e == 0);
    p = place((q_hi + 1) * bin - 1, 1, bin, q_hi, B);  // ends exactly at the end of q_hi: its end bin is q_hi + 1
    CHECK(p.bits == (kPFuture | kPStart | kPEnd) && p.qe == q_hi && p.idle_e == 0);
    p = place((oldest - 1) * bin, 999, bin, q_hi, B);  // ended before the oldest bin
    CHECK(p.bits == kPTooOld);
    p = place((oldest - 1) * bin + 999, 1, bin, q_hi, B);  // ends on the oldest bin's edge: clipped, no busy time
    CHECK(p.bits == (kPClipped | kPEnd) && p.qe == oldest && p.idle_e == (uint64_t)bin);
    p = place((oldest - 7) * bin + 500, 10000, bin, q_hi, B);
    CHECK(p.bits == (kPClipped | kPEnd) && p.qe == oldest + 3 && p.idle_e == 500);
    p = place(oldest * bin, 1, bin, q_hi, B);  // the oldest bin's first microsecond is kept whole
    CHECK(p.bits == (kPStart | kPEnd) && p.qs == oldest && p.idle_s == 0 && p.idle_e == 999);
    p = place((oldest - 3) * bin, 86400000000ll, bin, q_hi, B);  // before the ring and beyond it
    CHECK(p.bits == (kPFuture | kPClipped | kPEnd) && p.qe == q_hi && p.idle_e == 0);
    p = place(1, 0, bin, 0, B);  // the very first bin
    CHECK(p.bits == (kPStart | kPEnd) && p.qs == 0 && p.qe == 0);
  }
  // cells; the scan by runs of bins (what the wave does) against the recurrence
  {
    CHECK(cell_starts(kStartAdd * 5 + kEndAdd * 3) == 5 && cell_ends(kStartAdd * 5 + kEndAdd * 3) == 3);
    CHECK(cell_delta(kStartAdd * 2 + kEndAdd * 9) == -7 && combine(combine(3, -5), 7) == combine(3, combine(-5, 7)));
    uint64_t seed = 11;
    for (uint32_t bins : {64u, 128u, 1024u}) {
      const uint32_t per = bins / 64;
      std::vector<uint64_t> counts(bins), idle(bins);
      const int64_t carry = (int64_t)(rnd(seed) % 5);
      int64_t in_flight = carry;
      for (uint32_t t = 0; t < bins; ++t) {  // a consistent ring: never more ends than requests in flight
        const uint32_t s = (uint32_t)(rnd(seed) % 4), e = (uint32_t)(rnd(seed) % (uint64_t)(in_flight + s + 1));
        counts[t] = kStartAdd * s + kEndAdd * e;
        idle[t] = rnd(seed) % ((uint64_t)(s + e) * bin + 1);
        in_flight += (int64_t)s - (int64_t)e;
      }
      // the recurrence
      std::vector<int64_t> active(bins), busy(bins);
      int64_t A = carry;
      for (uint32_t t = 0; t < bins; ++t) {
        active[t] = A + cell_starts(counts[t]);
        busy[t] = active[t] * bin - (int64_t)idle[t];
        A += cell_delta(counts[t]);
        CHECK(A >= 0);
      }
      // by lanes: each lane's run, an inclusive scan over the lanes, then each lane's own pass
      std::vector<int64_t> run(64, 0);
      for (uint32_t l = 0; l < 64; ++l)
        for (uint32_t j = 0; j < per; ++j) run[l] = combine(run[l], cell_delta(counts[l * per + j]));
      for (uint32_t d = 1; d < 64; d <<= 1) {
        std::vector<int64_t> next(run);
        for (uint32_t l = d; l < 64; ++l) next[l] = combine(run[l - d], run[l]);
        run = next;
      }
      for (uint32_t l = 0; l < 64; ++l) {
        int64_t a = carry + (l ? run[l - 1] : 0);
        for (uint32_t j = 0; j < per; ++j) {
          const uint32_t t = l * per + j;
          CHECK(bin_active(a, counts[t]) == active[t] && bin_busy(active[t], bin, idle[t]) == busy[t]);
          a += cell_delta(counts[t]);
        }
      }
      CHECK(carry + run[63] == A);
    }
  }
  // ranges
  {
    Ranges r = ranges_of(1000, 900, 64, 2, 4, 8);  // the ring's oldest bin 937 is past q_first
    CHECK(r.oldest == 937 && r.lo == 937 && r.recent_hi == 998 && r.recent_lo == 995 && r.base_lo == 937 && r.base_hi == 994);
    CHECK(r.base_bins == 58 && !r.warming);
    r = ranges_of(1000, 987, 64, 2, 4, 8);
    CHECK(r.lo == 987 && r.base_bins == 8 && !r.warming);
    r = ranges_of(1000, 988, 64, 2, 4, 8);
    CHECK(r.base_bins == 7 && r.warming);
    r = ranges_of(1000, 996, 64, 2, 4, 8);  // recent reaches below q_first
    CHECK(r.base_bins == 0 && r.warming);
    r = ranges_of(1000, 1000, 64, 2, 4, 8);
    CHECK(r.base_bins == 0 && r.warming);
    r = ranges_of(1000, 0, 64, 0, 1, 63);
    CHECK(r.base_bins == 63 && !r.warming && r.recent_lo == 1000 && r.recent_hi == 1000);
  }
  // the compares: equality satisfies each; against 128 bits at the bounds' extremes and at random
  {
    Sums s{0, 0, 6, 8};
    CHECK(predicates(s, 8, 4, bin, 1500, 4, 500) == kArrUp && predicates(s, 8, 4, bin, 1501, 4, 500) == 0);
    CHECK(predicates(s, 8, 4, bin, 1500, 7, 500) == 0);
    s = Sums{0, 0, 4, 12};
    CHECK(predicates(s, 8, 4, bin, 1500, 4, 500) == kArrDown && predicates(s, 8, 4, bin, 1501, 4, 500) == 0);
    s = Sums{0, 0, 0, 8};
    CHECK(predicates(s, 8, 4, bin, 1500, 4, 500) == kArrDown && predicates(s, 8, 4, bin, 1500, 5, 500) == 0);
    s = Sums{6000, 8000, 8, 8};
    CHECK(predicates(s, 8, 4, bin, 1500, 100, 500) == kConcUp && predicates(s, 8, 4, bin, 1501, 100, 500) == 0);
    CHECK(predicates(s, 8, 4, bin, 1500, 100, 1500) == kConcUp && predicates(s, 8, 4, bin, 1500, 100, 1501) == 0);
    CHECK(predicates(s, 8, 4, bin, 1500, 4, 500) == (kArrUp | kConcUp) && state_of(kArrUp | kConcUp | kArrDown) == kSurge);
    CHECK(state_of(kConcUp | kArrDown) == kSlowdown && state_of(kArrDown) == kDrop && state_of(0) == kSteady);
    CHECK(conc_milli(1999, 4, 1000) == 499 && conc_milli(2000, 4, 1000) == 500);
    // the extremes: 2^31 - 1 requests, 8191 bins, f at both ends, busy sums up to what the bound allows: at most
    // 2^53, and at most every request in flight for the whole range
    const uint64_t top = uint64_t(1) << 53;
    const uint32_t n31 = 2147483647u;
    auto cap = [&](uint32_t nbins, int64_t bu) {
      const u128 all = (u128)n31 * nbins * (u128)bu;
      return all < top ? (uint64_t)all : top;
    };
    const uint32_t counts[] = {0u, 1u, 19u, 20u, n31 - 1, n31};
    const uint32_t nbs[] = {1u, 2u, 60u, 8190u, 8191u};
    const int64_t fs[] = {kMinFactorMilli, 1500, kMaxFactorMilli};
    for (uint32_t ar : counts)
      for (uint32_t ab : counts)
        for (uint32_t nb : nbs)
          for (uint32_t nr : nbs)
            for (int64_t f : fs)
              for (int64_t bu : {kMinBinUs, kMaxBinUs}) {
                const uint64_t cr = cap(nr, bu), cb = cap(nb, bu);
                const uint64_t br[] = {0, 1, cr / 3, cr - 1, cr}, bb[] = {cb, cb - 1, cb / 3 * 2, 1, 0};
                for (int i = 0; i < 5; ++i)
                  for (int j = 0; j < 5; ++j) {
                    const Sums x{br[i], bb[j], ar, ab};
                    CHECK(predicates(x, nb, nr, bu, f, 20, 1000) == wide(x, nb, nr, bu, f, 20, 1000));
                    CHECK(predicates(x, nb, nr, bu, f, kMaxMinRequests, kMaxMinConcMilli) ==
                          wide(x, nb, nr, bu, f, kMaxMinRequests, kMaxMinConcMilli));
                  }
              }
    uint64_t seed = 5;
    for (int i = 0; i < 20000; ++i) {
      const uint32_t nb = 1 + (uint32_t)(rnd(seed) % 8191), nr = 1 + (uint32_t)(rnd(seed) % 8191);
      const int64_t bu = kMinBinUs + (int64_t)(rnd(seed) % (uint64_t)(kMaxBinUs - kMinBinUs + 1));
      const Sums x{rnd(seed) % (cap(nr, bu) + 1), rnd(seed) % (cap(nb, bu) + 1), (uint32_t)(rnd(seed) % ((uint64_t)n31 + 1)),
                   (uint32_t)(rnd(seed) % ((uint64_t)n31 + 1))};
      const int64_t f = kMinFactorMilli + (int64_t)(rnd(seed) % (uint64_t)(kMaxFactorMilli - kMinFactorMilli + 1));
      const int64_t mr = 1 + (int64_t)(rnd(seed) % (uint64_t)kMaxMinRequests), mc = 1 + (int64_t)(rnd(seed) % (uint64_t)kMaxMinConcMilli);
      CHECK(predicates(x, nb, nr, bu, f, mr, mc) == wide(x, nb, nr, bu, f, mr, mc));
    }
  }
  // age
  CHECK(age_of(kSurge, kSteady, 0) == 1 && age_of(kSurge, kSurge, 1) == 2 && age_of(kDrop, kSurge, 9) == 1);
  CHECK(age_of(kSteady, kSteady, 7) == 0 && age_of(kWarming, kWarming, 7) == 0 && age_of(kSlowdown, kSlowdown, 0xfffffffeu) == 0xffffffffu);
  CHECK(age_of(kSlowdown, kSlowdown, 0xffffffffu) == 0xffffffffu);
  // the row and the LDS key
  CHECK(offsetof(Row, peak_q) == 8 && offsetof(Row, busy_recent) == 16 && offsetof(Row, busy_ring) == 32);
  CHECK(offsetof(Row, arr_recent) == 40 && offsetof(Row, peak_active) == 56 && offsetof(Row, arr_ring) == 64 && offsetof(Row, pad) == 72);
  CHECK(lds_key(0, 0) != 0 && lds_group(lds_key(65535, 8191)) == 65535 && lds_slot(lds_key(65535, 8191)) == 8191);
  CHECK(lds_slot(lds_key(7, kCarrySlot)) == kCarrySlot && lds_group(lds_key(7, kCarrySlot)) == 7 && lds_hash(lds_key(3, 5)) < (uint32_t)kLdsSlots);
  // configuration
  {
    Config ok;
    validate(ok);
    CHECK(ok.ring_records_max == default_ring_records_max(1024, 500000) && ok.ring_records_max == (int64_t(1) << 53) / (1024 * 500000ll));
    CHECK(default_ring_records_max(64, 1000) == kMaxRingRecords && default_ring_records_max(8192, 60000000) == 18325);
    auto bad = [&](auto set) {
      Config c;
      set(c);
      return throws<std::invalid_argument>([&] { validate(c); });
    };
    CHECK(bad([](Config& c) { c.bins = 32; }) && bad([](Config& c) { c.bins = 16384; }) && bad([](Config& c) { c.bins = 96; }));
    CHECK(bad([](Config& c) { c.bin_us = 999; }) && bad([](Config& c) { c.bin_us = 60000001; }));
    CHECK(bad([](Config& c) { c.settle_bins = -1; }) && bad([](Config& c) { c.recent_bins = 0; }) && bad([](Config& c) { c.min_base_bins = 0; }));
    CHECK(bad([](Config& c) { c.settle_bins = 1000; }) && !bad([](Config& c) { c.settle_bins = 934; }) && bad([](Config& c) { c.settle_bins = 935; }));
    CHECK(bad([](Config& c) { c.factor_milli = 1000; }) && bad([](Config& c) { c.factor_milli = 64001; }));
    CHECK(bad([](Config& c) { c.min_requests = 0; }) && bad([](Config& c) { c.min_requests = int64_t(1) << 31; }));
    CHECK(bad([](Config& c) { c.min_conc_milli = 0; }) && bad([](Config& c) { c.min_conc_milli = 1000000001; }));
    CHECK(bad([](Config& c) { c.group_cap = 0; }) && bad([](Config& c) { c.group_cap = 65537; }) && bad([](Config& c) { c.span_cap = 0; }));
    CHECK(bad([](Config& c) { c.n_buffers = 0; }) && bad([](Config& c) { c.n_buffers = 65; }));
    CHECK(bad([](Config& c) { c.ring_records_max = 0; }) && bad([](Config& c) { c.ring_records_max += 1; }));
    CHECK(bad([](Config& c) { c.group_cap = 32768, c.bins = 8192, c.ring_records_max = 1; }));  // 4 GiB of cells
    CHECK(!bad([](Config& c) { c.bins = 64, c.bin_us = 1000, c.settle_bins = 2, c.recent_bins = 4, c.min_base_bins = 58, c.ring_records_max = kMaxRingRecords; }));
  }
  // the layout: every array on 16 bytes
  for (int g : {1, 2, 3, 4, 64, 1000, 65536}) {
    const Layout l = layout(g);
    CHECK(l.rows == 0 && l.stats == (size_t)g * kRowWords && l.stats % 4 == 0 && l.words % 4 == 0 && l.words >= l.stats + kStats);
    std::printf("layout %d %zu %zu %zu\n", g, l.rows, l.stats, l.words);
  }
  std::printf("device_bytes %llu\n", (unsigned long long)device_bytes(1024, 16384, 64));
  std::printf("ring_records_max %lld\n", (long long)default_ring_records_max(1024, 500000));
  // ranges and steps
  {
    std::vector<uint8_t> buf(64 * 8);
    const uintptr_t a = (uintptr_t)buf.data();
    CHECK(plan_ranges({}, 8) == 0 && plan_ranges({{a, 64 * 3}, {0, 0}, {a, 0}, {a + 64 * 3, 64 * 5}}, 8) == 8);
    CHECK(throws<std::invalid_argument>([&] { plan_ranges({{a, 63}}, 8); }));
    CHECK(throws<std::invalid_argument>([&] { plan_ranges({{0, 64}}, 8); }));
    CHECK(throws<std::invalid_argument>([&] { plan_ranges({{a, 64 * 8}, {a, 64}}, 8); }));
    check_step(1, 0, 4), check_step(1, 4, 4);
    CHECK(throws<std::invalid_argument>([] { check_step(0, 1, 4); }) && throws<std::invalid_argument>([] { check_step(-3, 1, 4); }));
    CHECK(throws<std::invalid_argument>([] { check_step(1, 5, 4); }) && throws<std::invalid_argument>([] { check_step(1, -1, 4); }));
  }
  // the ring-population bound
  {
    Population p(64, 300);
    p.check(100, 128), p.take(100, 128);
    p.check(108, 128), p.take(108, 128);
    CHECK(p.after(116, 44) == 300 && p.after(116, 45) == 301 && p.steps() == 2);
    CHECK(throws<std::invalid_argument>([&] { p.check(116, 45); }) && p.steps() == 2);
    p.check(116, 44), p.take(116, 44);
    CHECK(p.after(163, 0) == 300 && p.after(164, 0) == 172 && p.after(172, 128) == 172);
    p.take(180, 0);
    CHECK(p.steps() == 0);
  }
  std::printf("loadsli host ok\n");
  return 0;
}
