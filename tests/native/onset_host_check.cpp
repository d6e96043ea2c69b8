// The breach-onset tracker's host side (ops/csrc/onset_host.h: the bin rule at its boundaries, the ring
// slot, the scan operator's associativity on fixed triples with negative sums, the CUSUM by runs
// against the recurrence, the row, the configuration and argument checks, the result block's layout
// and the ring-population bound) on its own, for the host sanitizers: tests/test_onset.py builds this
// with -fsanitize=address,undefined, runs it and compares the lines it prints with pipeline/onset.py's.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "onset_host.h"

using namespace mislo::onset;

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

static bool same(Run a, Run b) { return a.s == b.s && a.m == b.m; }

int main() {
  const int64_t bin = 10000000ll;
  const uint32_t B = 64;
  // the bin rule at its boundaries
  {
    const int64_t q_hi = 170000000000ll + 16;
    int64_t q = -7;
    CHECK(place(0, bin, q_hi, B, &q) == kDroppedNoTime && place(-5, bin, q_hi, B, &q) == kDroppedNoTime && q == -7);
    CHECK(place(q_hi * bin, bin, q_hi, B, &q) == kPlaced && q == q_hi);
    CHECK(place(q_hi * bin - 1, bin, q_hi, B, &q) == kPlaced && q == q_hi - 1);
    CHECK(place((q_hi + 1) * bin - 1, bin, q_hi, B, &q) == kPlaced && q == q_hi);
    CHECK(place((q_hi + 1) * bin, bin, q_hi, B, &q) == kPlacedFuture && q == q_hi);
    q = -7;
    CHECK(place((q_hi - B) * bin + 7, bin, q_hi, B, &q) == kDroppedOld && place((q_hi - B + 1) * bin - 1, bin, q_hi, B, &q) == kDroppedOld);
    CHECK(q == -7);
    CHECK(place((q_hi - B + 1) * bin, bin, q_hi, B, &q) == kPlaced && q == q_hi - B + 1 && q == oldest_bin(q_hi, B));
    CHECK(place(1, bin, 0, B, &q) == kPlaced && q == 0 && place(bin, bin, 0, B, &q) == kPlacedFuture && q == 0);
    // slots: the ring covers every slot once; bins below 0 have slots too
    std::vector<int> seen(B, 0);
    for (int64_t b = oldest_bin(q_hi, B); b <= q_hi; ++b) ++seen[slot_of(b, B)];
    for (int v : seen) CHECK(v == 1);
    CHECK(slot_of(-1, B) == B - 1 && slot_of(-(int64_t)B, B) == 0 && slot_of(0, 8192) == 0 && slot_of(8191, 8192) == 8191);
    // q_hi never moves back; what an advance clears
    CHECK(advance(kNoBin, 5, bin) == 0 && advance(kNoBin, q_hi * bin + 3, bin) == q_hi && advance(q_hi, (q_hi - 4) * bin, bin) == q_hi);
    CHECK(advance(q_hi, (q_hi + 1) * bin, bin) == q_hi + 1 && advance(q_hi, (q_hi + 1) * bin - 1, bin) == q_hi);
    CHECK(cleared(q_hi, q_hi + 1, B) == 1 && cleared(q_hi, q_hi + B - 1, B) == B - 1 && cleared(q_hi, q_hi + B, B) == B);
    CHECK(cleared(kNoBin, q_hi, B) == B && cleared(kNoBin, 0, B) == 1 && cleared(q_hi, q_hi + 5 * (int64_t)B, 8192) == 5 * B);
  }
  // the cell and the increment: the extremes stay inside 2^52
  {
    uint64_t c = 0;
    c += cell_add(1), c += cell_add(0), c += cell_add(1);
    CHECK(cell_n(c) == 3 && cell_b(c) == 2 && excess(c, 250000) == 2 * kMillion - 750000);
    const uint64_t full = ((uint64_t)kMaxRingRecords << 32) | (uint64_t)kMaxRingRecords;
    CHECK(excess(full, 1) == kMaxRingRecords * (kMillion - 1) && excess(full, 1) < (int64_t(1) << 52));
    CHECK(excess((uint64_t)kMaxRingRecords, kMillion - 1) == -kMaxRingRecords * (kMillion - 1));
  }
  // the scan operator: identity, associativity on fixed triples (negative sums among them), not commutative
  {
    const Run t[] = {run_of(750000), run_of(-250000), run_of(-3000000), run_of(0), Run{-5, -9}, Run{4, -2}, Run{1000000, 0},
                     Run{-kMaxRingRecords * 999999ll, -kMaxRingRecords * 999999ll}};
    const int n = (int)(sizeof(t) / sizeof(t[0]));
    for (int i = 0; i < n; ++i) {
      CHECK(same(combine(run_identity(), t[i]), t[i]) && same(combine(t[i], run_identity()), t[i]));
      for (int j = 0; j < n; ++j)
        for (int k = 0; k < n; ++k) CHECK(same(combine(combine(t[i], t[j]), t[k]), combine(t[i], combine(t[j], t[k]))));
    }
    CHECK(!same(combine(t[0], t[2]), combine(t[2], t[0])));
    CHECK(run_of(-3).m == -3 && run_of(3).m == 0);
    // the CUSUM by runs of 1, 2 and 5 bins against the recurrence
    const int64_t x[] = {0, 750000, -250000, -250000, -250000, -250000, 750000, 750000, -2000000, 5, -5, 0, 1000000, -1, 0};
    const int len = (int)(sizeof(x) / sizeof(x[0]));
    int64_t S = 0;
    std::vector<int64_t> want;
    for (int i = 0; i < len; ++i) want.push_back(S = (S + x[i] > 0 ? S + x[i] : 0));
    for (int per : {1, 2, 5}) {
      Run before = run_identity();
      for (int first = 0; first < len; first += per) {
        Run mine = run_identity();
        int64_t P = before.s, M = before.m;
        for (int j = first; j < first + per && j < len; ++j) {
          mine = combine(mine, run_of(x[j]));
          P += x[j];
          M = P < M ? P : M;
          CHECK(P - M == want[(size_t)j]);
        }
        before = combine(before, mine);
        CHECK(before.s == P && before.m == M);
      }
    }
  }
  // the row and the LDS key
  CHECK(sizeof(Row) == 64 && offsetof(Row, state) == 0 && offsetof(Row, flags) == 4 && offsetof(Row, onset_q) == 8);
  CHECK(offsetof(Row, alarm_q) == 16 && offsetof(Row, s_now) == 24 && offsetof(Row, s_peak) == 32 && offsetof(Row, n_exc) == 40);
  CHECK(offsetof(Row, b_exc) == 44 && offsetof(Row, n_ring) == 48 && offsetof(Row, b_ring) == 52 && offsetof(Row, pad) == 56);
  CHECK(lds_key(0, 0) != 0 && lds_group(lds_key(65535, 8191)) == 65535 && lds_slot(lds_key(65535, 8191)) == 8191);
  CHECK(lds_group(lds_key(0, 0)) == 0 && lds_slot(lds_key(7, 0)) == 0);
  // the configuration checks, both sides of every bound
  Config ok;
  validate(ok);
  CHECK(ok.bins == 1024 && ok.bin_ns == 125000000 && ok.ref_ppm == 20000 && ok.alarm == 3 && ok.ring_records_max == 2147483647ll);
  CHECK(device_bytes(ok) == 16384ull * 64 + 64ull * 1024 * 8 + layout(64).words * 4);
  auto bad = [&](auto set) {
    Config c;
    c.group_cap = 4;
    set(c);
    return throws<std::invalid_argument>([&] { validate(c); });
  };
  CHECK(bad([](Config& c) { c.bins = 32; }) && bad([](Config& c) { c.bins = 16384; }) && bad([](Config& c) { c.bins = 96; }));
  CHECK(bad([](Config& c) { c.bins = 0; }) && bad([](Config& c) { c.bins = -64; }));
  CHECK(!bad([](Config& c) { c.bins = 64; }) && !bad([](Config& c) { c.bins = 8192; }));
  CHECK(bad([](Config& c) { c.bin_ns = 999999; }) && bad([](Config& c) { c.bin_ns = 60000000001ll; }));
  CHECK(!bad([](Config& c) { c.bin_ns = 1000000; }) && !bad([](Config& c) { c.bin_ns = 60000000000ll; }));
  CHECK(bad([](Config& c) { c.ref_ppm = 0; }) && bad([](Config& c) { c.ref_ppm = 1000000; }));
  CHECK(!bad([](Config& c) { c.ref_ppm = 1; }) && !bad([](Config& c) { c.ref_ppm = 999999; }));
  CHECK(bad([](Config& c) { c.alarm = 0; }) && bad([](Config& c) { c.alarm = 1000001; }));
  CHECK(!bad([](Config& c) { c.alarm = 1; }) && !bad([](Config& c) { c.alarm = 1000000; }));
  CHECK(bad([](Config& c) { c.group_cap = 0; }) && bad([](Config& c) { c.group_cap = 65537; }));
  CHECK(!bad([](Config& c) { c.group_cap = 1; }) && !bad([](Config& c) { c.group_cap = 65536, c.bins = 64; }));
  CHECK(bad([](Config& c) { c.span_cap = 0; }) && !bad([](Config& c) { c.span_cap = 1; }));
  CHECK(bad([](Config& c) { c.n_buffers = 0; }) && bad([](Config& c) { c.n_buffers = 65; }));
  CHECK(!bad([](Config& c) { c.n_buffers = 1; }) && !bad([](Config& c) { c.n_buffers = 64; }));
  CHECK(bad([](Config& c) { c.slo_ms = -1.0; }) && bad([](Config& c) { c.slo_ms = std::nan(""); }));
  CHECK(bad([](Config& c) { c.slo_ms = std::numeric_limits<double>::infinity(); }) && !bad([](Config& c) { c.slo_ms = 0.0; }));
  CHECK(bad([](Config& c) { c.ring_records_max = 0; }) && bad([](Config& c) { c.ring_records_max = 2147483648ll; }));
  CHECK(!bad([](Config& c) { c.ring_records_max = 1; }) && !bad([](Config& c) { c.ring_records_max = 2147483647ll; }));
  // 2 GiB: 65536 services of 8192 bins are 4 GiB of cells; 32768 of 8192 with the spans and the block pass it too
  CHECK(bad([](Config& c) { c.group_cap = 65536, c.bins = 8192; }) && bad([](Config& c) { c.group_cap = 32768, c.bins = 8192; }));
  CHECK(!bad([](Config& c) { c.group_cap = 32768, c.bins = 4096; }));
  CHECK(bad([](Config& c) { c.span_cap = 1 << 25; }) && !bad([](Config& c) { c.span_cap = 1 << 24; }));
  // the result block: rows then stats, every array on 16 bytes
  for (int g : {1, 3, 5, 64, 65536}) {
    const Layout l = layout(g);
    CHECK(l.rows == 0 && l.stats == (size_t)g * 16 && l.stats % 4 == 0 && l.words == l.stats + 8 && l.words % 4 == 0);
  }
  // the step's arguments
  std::vector<char> buf(64 * 8);
  const uintptr_t a = reinterpret_cast<uintptr_t>(buf.data());
  CHECK(plan_ranges({}, 4) == 0 && plan_ranges({{a, 128}, {0, 0}, {a + 128, 128}}, 4) == 4);
  CHECK(throws<std::invalid_argument>([&] { plan_ranges({{a, 128}, {a + 128, 192}}, 4); }));
  CHECK(throws<std::invalid_argument>([&] { plan_ranges({{a, 63}}, 4); }));
  CHECK(throws<std::invalid_argument>([&] { plan_ranges({{0, 64}}, 4); }));
  check_step(1, 0, 3);
  check_step(1, 3, 3);
  CHECK(throws<std::invalid_argument>([&] { check_step(1, 4, 3); }) && throws<std::invalid_argument>([&] { check_step(1, -1, 3); }));
  CHECK(throws<std::invalid_argument>([&] { check_step(0, 1, 3); }) && throws<std::invalid_argument>([&] { check_step(-9, 1, 3); }));
  // the population bound on both sides, and old steps expiring
  {
    Population p(B, 100);
    p.check(10, 100);
    CHECK(throws<std::invalid_argument>([&] { p.check(10, 101); }) && p.steps() == 0);
    p.take(10, 60);
    p.take(20, 40);
    CHECK(p.after(20, 0) == 100 && p.steps() == 2);
    p.check(20, 0);
    CHECK(throws<std::invalid_argument>([&] { p.check(20, 1); }) && p.steps() == 2);
    CHECK(throws<std::invalid_argument>([&] { p.check(10 + B - 1, 1); }));  // the step at 10 still holds bin 10
    p.check(10 + B, 60);                                                      // at q_hi = 10 + B its records are cleared
    CHECK(throws<std::invalid_argument>([&] { p.check(10 + B, 61); }));
    p.take(10 + B, 60);
    CHECK(p.steps() == 2 && p.after(10 + B, 0) == 100);
    p.take(20 + B, 0);  // an empty step still expires the old ones
    CHECK(p.steps() == 1 && p.after(20 + B, 0) == 60);
  }
  const int64_t keys[][2] = {{0, 0}, {0, 1}, {1, 0}, {63, 1023}, {65535, 8191}, {7, 4242}};
  for (const auto& k : keys)
    std::printf("lds_hash %lld %lld %u\n", (long long)k[0], (long long)k[1], lds_hash(lds_key((uint32_t)k[0], (uint32_t)k[1])));
  const int64_t ts[][2] = {{1, 1000000}, {999999, 1000000}, {1000000, 1000000}, {1700000000123456789ll, 125000000},
                           {1700000000123456789ll, 60000000000ll}, {59999999999ll, 60000000000ll}};
  for (const auto& t : ts)
    std::printf("bin_of %lld %lld %lld %u\n", (long long)t[0], (long long)t[1], (long long)bin_of(t[0], t[1]),
                slot_of(bin_of(t[0], t[1]), 1024));
  std::puts("onset host ok");
  return 0;
}
