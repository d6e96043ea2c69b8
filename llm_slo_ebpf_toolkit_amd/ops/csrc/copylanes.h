// Copy lanes: which copy stream a window's DMAs go to, and the host-side account of how far the
// windows have been copied. Pure host arithmetic (no HIP), shared by the engine and by
// tests/native/copylanes_host_check.cpp and copyahead_host_check.cpp.
//
// A lane is one in-order copy stream. With two lanes window k's DMAs go to lane k & 1, so a lane
// completes its windows in order (k, k - 2, k - 4, ...) but the two lanes complete in any order
// relative to each other. "Copied up to k" (h2d_done(k), wait_h2d(k)) means every window <= k: the
// rings release space by count, so a later window that finishes first must not report done while
// an earlier one is still being read.
#pragma once

#include <cstdint>

namespace mislo {

constexpr int kMaxCopyLanes = 2;

// the lane of window k's DMAs
inline int copy_lane(int64_t k, int lanes) { return lanes > 1 ? (int)(k % lanes) : 0; }

// The windows whose completion events answer "every window up to k has been copied": the newest
// window of every lane at or before k, i.e. k and, with two lanes, k - 1 (older windows follow
// from lane order). Newest first; returns how many.
inline int copy_consults(int64_t k, int lanes, int64_t out[kMaxCopyLanes]) {
  int n = 0;
  for (int i = 0; i < (lanes > 1 ? lanes : 1) && k - i >= 0; ++i) out[n++] = k - i;
  return n;
}

// The copy-side events of window k (the marker before its first DMA and its completion event)
// live in slot k % (2 nb): the copy phase of window k + nb may run while window k has not been
// collected, and that window's timing (window_ms, copy_ms) must still read its own records.
inline int copy_mark_slots(int nb) { return 2 * nb; }
inline int copy_mark_slot(int64_t k, int nb) { return (int)(k % copy_mark_slots(nb)); }

// Every window below `n` is known copied; `n` only moves forward.
//
// A window's completion event lives in its slot and is recorded again by window k + 2 nb. The
// copy phase of window k + nb synchronises it first (the buffer's pinned head and staging are
// rewritten then) and calls reused(): so the event of a window >= n still belongs to that window,
// and a window < n is never asked about again -- no stale answer.
// tests/native/copyahead_host_check.cpp walks this protocol.
struct CopiedUpTo {
  int64_t n = 0;

  // the copy phase of window k synchronised window k - nb's event, as that of window k - 1 did
  // window k - 1 - nb's: with every lane in order, every window <= k - nb has been copied
  void reused(int64_t k, int nb) {
    if (k - nb + 1 > n) n = k - nb + 1;
  }

  // ready(w): window w's event has completed (queried or waited for by the caller). Consulted
  // only for windows >= n.
  template <class Ready>
  bool done(int64_t k, int lanes, Ready&& ready) {
    if (k < n) return true;
    int64_t w[kMaxCopyLanes];
    const int c = copy_consults(k, lanes, w);
    for (int i = 0; i < c; ++i)
      if (w[i] >= n && !ready(w[i])) return false;
    n = k + 1;
    return true;
  }
};

}  // namespace mislo
