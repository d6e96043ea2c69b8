// The copy lanes' host arithmetic (ops/csrc/copylanes.h) on its own, for the host sanitizers:
// tests/test_copy_lanes.py builds this with -fsanitize=address,undefined and runs it.
//
// A model of the engine's protocol stands in for the device: window k's completion event lives in
// buffer k % nb, a lane completes its windows in order, and submit(k) synchronises the event of
// window k - nb before window k records it again. Checked for 1 and 2 lanes, 2..6 buffers and a
// few hundred windows: the lane of every window, the windows h2d_done(k) consults, that no event
// is consulted after a later window re-recorded it, that "done" is never reported for a window
// while an earlier one is still being copied, that it is reported as soon as every window up to
// it is copied, and that it stays reported -- under every completion order of the windows in
// flight.
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
  int nb, lanes;
  int64_t submitted = 0;
  std::vector<char> copied;      // by window: its DMAs ended (the device's truth)
  std::vector<int64_t> owner;    // by buffer: the window that recorded the event last
  std::vector<char> said_done;   // by window: h2d_done(k) has returned true
  CopiedUpTo acc;
  long consulted = 0;

  Model(int nb_, int lanes_, int64_t windows) : nb(nb_), lanes(lanes_), copied(windows, 0), owner(nb_, -1),
                                                said_done(windows, 0) {}

  bool all_copied_to(int64_t k) const {
    for (int64_t w = 0; w <= k; ++w)
      if (!copied[w]) return false;
    return true;
  }
  // the oldest window of `lane` still being copied, or -1
  int64_t oldest(int lane) const {
    for (int64_t w = 0; w < submitted; ++w)
      if (!copied[w] && copy_lane(w, lanes) == lane) return w;
    return -1;
  }
  void complete_lane_to(int64_t k) {  // a host wait for window k's event: its lane is in order
    for (int64_t w = k; w >= 0; w -= lanes) copied[w] = 1;
  }
  void submit() {
    const int64_t k = submitted;
    if (k >= nb) {
      CHECK(owner[k % nb] == k - nb);
      complete_lane_to(k - nb);  // hipEventSynchronize(buf.h2d_done)
      acc.reused(k, nb);
      CHECK(all_copied_to(k - nb));  // what reused() claims
    }
    owner[k % nb] = k;
    ++submitted;
  }
  bool h2d_done(int64_t k) {
    const int64_t before = acc.n;
    int64_t want[kMaxCopyLanes];
    const int n_want = copy_consults(k, lanes, want);
    int seen = 0;
    const bool r = acc.done(k, lanes, [&](int64_t w) {
      ++consulted;
      bool listed = false;
      for (int i = 0; i < n_want; ++i) listed = listed || want[i] == w;
      CHECK(listed);                       // only the windows copy_consults names
      CHECK(w >= before && w < submitted);  // never a window already known copied
      CHECK(owner[w % nb] == w);           // the event is still that window's: no stale answer
      ++seen;
      return (bool)copied[w];
    });
    CHECK(seen <= n_want);
    CHECK(acc.n >= before);                 // only forward
    CHECK(r == all_copied_to(k));           // never early, never late
    if (said_done[k]) CHECK(r);             // and it stays
    if (r) {
      said_done[k] = 1;
      CHECK(acc.n >= k + 1);
    }
    return r;
  }
  // query the windows in flight newest first (k + 1 before k), as the ring source's reap may
  void poll() {
    for (int64_t k = submitted - 1; k >= 0 && k >= submitted - nb - 1; --k) {
      const bool newer = k + 1 < submitted ? h2d_done(k + 1) : false;
      const bool mine = h2d_done(k);
      CHECK(!(newer && !mine));
    }
  }
};

// every completion order of the windows in flight (each lane in order), polling after every step
void explore(Model m, long& leaves) {
  m.poll();
  bool any = false;
  for (int lane = 0; lane < m.lanes; ++lane) {
    const int64_t w = m.oldest(lane);
    if (w < 0) continue;
    any = true;
    Model next = m;
    next.copied[w] = 1;
    explore(next, leaves);
  }
  if (!any) {
    CHECK(m.acc.n == m.submitted);
    ++leaves;
  }
}

}  // namespace

int main() {
  // lanes and consulted windows, spelled out
  for (int64_t k = 0; k < 400; ++k) {
    int64_t w[kMaxCopyLanes] = {-7, -7};
    CHECK(copy_lane(k, 1) == 0 && copy_lane(k, 2) == (int)(k & 1));
    CHECK(copy_consults(k, 1, w) == 1 && w[0] == k);
    const int n = copy_consults(k, 2, w);
    CHECK(n == (k ? 2 : 1) && w[0] == k && (k == 0 || w[1] == k - 1));
    if (k) CHECK(copy_lane(w[0], 2) != copy_lane(w[1], 2));  // one window of each lane
  }
  long leaves = 0, consulted = 0;
  const int64_t windows = 300;
  for (int lanes = 1; lanes <= kMaxCopyLanes; ++lanes) {
    for (int nb = 2; nb <= 6; ++nb) {
      // a long run: submit as far ahead as the buffers allow, complete and poll in a fixed
      // pseudo-random order; at every window, every completion order of the windows in flight
      Model m(nb, lanes, windows);
      uint32_t rng = 12345u + 977u * nb + lanes;
      while (m.submitted < windows) {
        m.submit();
        if (m.submitted >= nb) explore(m, leaves);
        rng = rng * 1664525u + 1013904223u;
        for (uint32_t i = 0, steps = (rng >> 24) % 4; i < steps; ++i) {
          rng = rng * 1664525u + 1013904223u;
          const int64_t w = m.oldest((int)((rng >> 16) % lanes));
          if (w >= 0) m.copied[w] = 1;
          if ((rng >> 8) & 1) m.poll();
        }
      }
      for (int lane = 0; lane < lanes; ++lane)
        for (int64_t w; (w = m.oldest(lane)) >= 0;) m.copied[w] = 1;
      m.poll();
      CHECK(m.acc.n == windows);
      consulted += m.consulted;
    }
  }
  CHECK(leaves > 1000 && consulted > 1000);
  std::printf("copylanes host ok: %ld completion orders\n", leaves);
  return 0;
}
