// Copy ahead's host arithmetic (ops/csrc/copylanes.h) on its own, for the host sanitizers:
// tests/test_copy_ahead.py builds this with -fsanitize=address,undefined and runs it.
//
// A model of the engine's protocol stands in for the device, as in copylanes_host_check.cpp, with
// what copying ahead changed: window k's copy-side events live in slot k % (2 nb); the copy phase
// of window k synchronises the event of window k - nb and only then records its own slot; a
// window counts for h2d_done from its copy phase on. Checked for 1 and 2 lanes and 2..5 buffers --
// and, beyond what the engine does today, for a lane count that goes from one to two at some
// window k0 in mid-run (the windows before k0 all on lane 0), which the account survives because
// every lane stays in order: that no event is consulted after a
// later window re-recorded its slot, that the windows whose timing may still be asked for (k - nb
// .. k at the copy phase of window k) all own their slots, that what reused() claims holds, that
// "done" is reported never early, never late and for good -- under every completion order of the
// windows in flight.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "copylanes.h"

using namespace mislo;

#define CHECK(x)                                                          \
  do {                                                                    \
    if (!(x)) {                                                           \
      std::fprintf(stderr, "check failed at line %d: %s\n", __LINE__, #x); \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

namespace {

struct Model {
  int nb;
  int64_t two_from;  // the first window of the two-lane schedule (the engine's lanes_ = 2 from there)
  int64_t copied_windows = 0;
  std::vector<char> copied;     // by window: its DMAs ended (the device's truth)
  std::vector<int> lane;        // by window: the lane its DMAs were queued on
  std::vector<int64_t> owner;   // by slot: the window that recorded the events last
  std::vector<char> said_done;  // by window: h2d_done(k) has returned true
  CopiedUpTo acc;
  long consulted = 0;

  Model(int nb_, int64_t two_from_, int64_t windows)
      : nb(nb_), two_from(two_from_), copied(windows, 0), lane(windows, -1), owner(copy_mark_slots(nb_), -1),
        said_done(windows, 0) {}

  int lanes() const { return copied_windows > two_from ? 2 : 1; }  // as the engine holds it after its last copy phase
  bool all_copied_to(int64_t k) const {
    for (int64_t w = 0; w <= k; ++w)
      if (!copied[w]) return false;
    return true;
  }
  int64_t oldest(int on) const {  // the oldest window of lane `on` still being copied, or -1
    for (int64_t w = 0; w < copied_windows; ++w)
      if (!copied[w] && lane[w] == on) return w;
    return -1;
  }
  void complete_lane_to(int64_t k) {  // a host wait for window k's event: its lane is in order
    for (int64_t w = 0; w <= k; ++w)
      if (lane[w] == lane[k]) copied[w] = 1;
  }
  void submit_copy() {
    const int64_t k = copied_windows;
    const int n_lanes = k >= two_from ? 2 : 1;
    if (k >= nb) {
      CHECK(owner[copy_mark_slot(k - nb, nb)] == k - nb);  // the event waited for is that window's
      complete_lane_to(k - nb);
      acc.reused(k, nb);
      CHECK(all_copied_to(k - nb));  // what reused() claims, across the change of lanes too
    }
    const int slot = copy_mark_slot(k, nb);
    CHECK(owner[slot] < 0 || owner[slot] == k - copy_mark_slots(nb));
    CHECK(owner[slot] < acc.n);  // the window losing its slot is known copied: never asked about again
    owner[slot] = k;
    lane[k] = copy_lane(k, n_lanes);
    ++copied_windows;
    // window_ms / copy_ms of every window that may be uncollected now read their own records
    for (int64_t w = k > nb ? k - nb : 0; w <= k; ++w) CHECK(owner[copy_mark_slot(w, nb)] == w);
    if (k >= 1) CHECK(owner[copy_mark_slot(k - 1, nb)] == k - 1);  // copy_ms(k)'s gap
  }
  bool h2d_done(int64_t k) {
    if (k >= copied_windows) return false;
    const int64_t before = acc.n;
    const bool r = acc.done(k, lanes(), [&](int64_t w) {
      ++consulted;
      CHECK(w >= before && w < copied_windows && w <= k && w >= k - 1);
      CHECK(owner[copy_mark_slot(w, nb)] == w);  // no stale answer
      return (bool)copied[w];
    });
    CHECK(acc.n >= before);
    CHECK(r == all_copied_to(k));  // never early, never late
    if (said_done[k]) CHECK(r);
    if (r) {
      said_done[k] = 1;
      CHECK(acc.n >= k + 1);
    }
    return r;
  }
  void poll() {  // newest first, as the ring source's reap may
    for (int64_t k = copied_windows - 1; k >= 0 && k >= copied_windows - nb - 2; --k) {
      const bool newer = k + 1 < copied_windows ? h2d_done(k + 1) : false;
      const bool mine = h2d_done(k);
      CHECK(!(newer && !mine));
    }
  }
};

void explore(Model m, long& leaves) {  // every completion order of the windows in flight
  m.poll();
  bool any = false;
  for (int on = 0; on < 2; ++on) {
    const int64_t w = m.oldest(on);
    if (w < 0) continue;
    any = true;
    Model next = m;
    next.copied[w] = 1;
    explore(next, leaves);
  }
  if (!any) {
    CHECK(m.acc.n == m.copied_windows);
    ++leaves;
  }
}

}  // namespace

int main() {
  for (int nb = 2; nb <= 6; ++nb)
    for (int64_t k = 0; k < 200; ++k) {
      CHECK(copy_mark_slots(nb) == 2 * nb);
      CHECK(copy_mark_slot(k, nb) >= 0 && copy_mark_slot(k, nb) < copy_mark_slots(nb));
      CHECK(copy_mark_slot(k, nb) == copy_mark_slot(k + 2 * nb, nb));
      for (int d = 1; d < 2 * nb; ++d) CHECK(copy_mark_slot(k, nb) != copy_mark_slot(k + d, nb));
    }
  long leaves = 0, consulted = 0;
  const int64_t windows = 120;
  const int64_t never = INT64_MAX;
  for (int nb = 2; nb <= 5; ++nb) {
    const int64_t starts[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 40, 41, never};
    for (int64_t two_from : starts) {
      Model m(nb, two_from, windows);
      uint32_t rng = 4321u + 977u * nb + (uint32_t)(two_from & 0xFF);
      while (m.copied_windows < windows) {
        m.submit_copy();
        if (m.copied_windows >= nb && m.copied_windows < 60) explore(m, leaves);
        rng = rng * 1664525u + 1013904223u;
        for (uint32_t i = 0, steps = (rng >> 24) % 4; i < steps; ++i) {
          rng = rng * 1664525u + 1013904223u;
          const int64_t w = m.oldest((int)((rng >> 16) & 1));
          if (w >= 0) m.copied[w] = 1;
          if ((rng >> 8) & 1) m.poll();
        }
      }
      for (int on = 0; on < 2; ++on)
        for (int64_t w; (w = m.oldest(on)) >= 0;) m.copied[w] = 1;
      m.poll();
      CHECK(m.acc.n == windows);
      consulted += m.consulted;
    }
  }
  CHECK(leaves > 1000 && consulted > 1000);
  std::printf("copyahead host ok: %ld completion orders\n", leaves);
  return 0;
}
