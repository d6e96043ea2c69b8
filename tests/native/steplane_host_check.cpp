// The step lane's host side (ops/csrc/steplane_host.h: the span ranges of a step and the result slots'
// bookkeeping, under every side tracker's name) on its own, for the host sanitizers:
// tests/test_steplane.py builds this with -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "decodesli_host.h"
#include "drift_host.h"
#include "errsli_host.h"
#include "exemplars_host.h"
#include "loadsli_host.h"
#include "onset_host.h"
#include "openreq_host.h"
#include "podrank_host.h"
#include "retrsli_host.h"
#include "satcurve_host.h"
#include "slisketch_host.h"
#include "steplane_host.h"

using namespace mislo;

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      std::fprintf(stderr, "check failed at line %d: %s\n", __LINE__, #x); \
      std::exit(1);                                                    \
    }                                                                  \
  } while (0)

// the message of the E that f throws; "<none>" when it throws nothing (another type escapes)
template <class E, class F>
std::string message(F f) {
  try {
    f();
  } catch (const E& e) {
    return e.what();
  }
  return "<none>";
}

using Plan = size_t (*)(const std::vector<Range>&, int);

// one tracker's name: the shared plan_ranges and the tracker's own forwarder, which must agree
static void check_ranges(const std::string& who, Plan own) {
  alignas(64) static unsigned char buf[64 * 16];
  const uintptr_t base = reinterpret_cast<uintptr_t>(buf);
  const char* w = who.c_str();
  for (int via = 0; via < 2; ++via) {
    auto plan = [&](const std::vector<Range>& r, int cap) { return via ? own(r, cap) : plan_ranges(r, cap, w); };
    CHECK(plan({}, 8) == 0);
    CHECK(plan({{base, 64}}, 8) == 1);
    // empty ranges are skipped wherever they stand, a null one included
    CHECK(plan({{0, 0}, {base, 128}, {base + 512, 0}, {base + 128, 64}, {0, 0}}, 8) == 3);
    // exactly span_cap, in one range and over several; one more is refused
    CHECK(plan({{base, 64 * 8}}, 8) == 8);
    CHECK(plan({{base, 64 * 5}, {0, 0}, {base + 64 * 5, 64 * 3}}, 8) == 8);
    CHECK(plan({{base, 64}}, 1) == 1);
    const std::string over = who + " step: more spans than span_cap";
    CHECK(message<std::invalid_argument>([&] { plan({{base, 64 * 9}}, 8); }) == over);
    CHECK(message<std::invalid_argument>([&] { plan({{base, 64 * 8}, {base, 64}}, 8); }) == over);
    CHECK(message<std::invalid_argument>([&] { plan({{base, 128}}, 1); }) == over);
    // a length near SIZE_MAX neither wraps the count nor passes
    CHECK(message<std::invalid_argument>([&] { plan({{base, 64}, {base, ~size_t(0) & ~size_t(63)}}, 8); }) == over);
    CHECK(message<std::invalid_argument>([&] { plan({{0, 64}}, 8); }) == who + " step: null range");
    const std::string whole = who + " step: a range is not whole 64-byte spans";
    CHECK(message<std::invalid_argument>([&] { plan({{base, 63}}, 8); }) == whole);
    CHECK(message<std::invalid_argument>([&] { plan({{base, 64}, {base + 64, 65}}, 8); }) == whole);
    // the checks of a range come in this order: null, whole, count
    CHECK(message<std::invalid_argument>([&] { plan({{0, 63}}, 0); }) == who + " step: null range");
    CHECK(message<std::invalid_argument>([&] { plan({{base, 64 * 9 + 1}}, 8); }) == whole);
  }
}

static void check_slots(const std::string& who, int n) {
  SlotRing r(n, who.c_str());
  auto refused = [&](int64_t i) {
    return message<std::out_of_range>([&] { r.slot_of(i); }) ==
           who + " step " + std::to_string(i) + " is not held (only the last " + std::to_string(n) + ")";
  };
  // before any step nothing is held, not even step 0
  CHECK(r.size() == n && r.next() == 0);
  for (int64_t i : {int64_t(-1), int64_t(0), int64_t(1), int64_t(n)}) CHECK(!r.holds(i) && refused(i));
  // across the wrap: after n, n + 1 and 2 n steps (and every count between) exactly the last n are held
  for (int64_t steps = 1; steps <= 2 * (int64_t)n + 1; ++steps) {
    CHECK(r.next() == steps - 1);
    const int s = r.begin();
    CHECK(s == (int)((steps - 1) % n) && r.next() == steps);
    for (int64_t j = -2; j <= steps + 1; ++j) {
      const bool held = j >= 0 && j < steps && j >= steps - n;
      CHECK(r.holds(j) == held);
      if (held) CHECK(r.slot_of(j) == (int)(j % n));
      else CHECK(refused(j));
    }
  }
  CHECK(refused(INT64_MIN) && refused(INT64_MAX));
}

int main() {
  static_assert(kSpanBytes == 64, "collector/records.py SPAN");
  const struct {
    const char* who;
    Plan own;
  } trackers[] = {
      {"open-request", openreq::plan_ranges},    {"ttft sketch", slisketch::plan_ranges},
      {"request exemplars", exemplars::plan_ranges}, {"pod breakdown", podrank::plan_ranges},
      {"breach onset", onset::plan_ranges},      {"decode sli", decodesli::plan_ranges},
      {"ttft drift", drift::plan_ranges},        {"error sli", errsli::plan_ranges},
      {"load sli", loadsli::plan_ranges},        {"saturation curve", satcurve::plan_ranges},
      {"retrieval sli", retrsli::plan_ranges},
  };
  for (const auto& t : trackers) {
    check_ranges(t.who, t.own);
    for (int n : {1, 2, 3, 7}) check_slots(t.who, n);
  }
  // the ring's own name is the open-request tracker's (openreq::SlotRing is this class)
  openreq::SlotRing d(2);
  CHECK(message<std::out_of_range>([&] { d.slot_of(0); }) == "open-request step 0 is not held (only the last 2)");
  SlotRing z(0, "x");  // a size the configuration checks refuse: still one slot, never none
  CHECK(z.size() == 1 && z.begin() == 0 && z.holds(0));
  // checked() is the tracker's validate(): it passes a good configuration through and refuses a bad one
  errsli::Config good, bad;
  bad.windows = 0;
  CHECK(&checked(good) == &good);
  CHECK(message<std::invalid_argument>([&] { checked(bad); }) == "error sli: windows must be in [1, 32768]");
  std::printf("steplane host ok\n");
  return 0;
}
