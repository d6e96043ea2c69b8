// Breach onset per service: when the current run of TTFT breaches began, at sub-window resolution.
//
// Every other reduction is per window, so the finest time known for a fault is the window it first
// scored in, and a breach exported late counts in the window it arrives in. This side tracker bins
// the counted span records by their own start time (Span::ts_ns) into a ring of B absolute time bins
// per service (onset_host.h: bin_of, slot_of, place), one u64 cell of (requests, breaches) a bin, and
// recomputes an integer CUSUM over the whole ring every step, so a late record revises the past.
// Per service it yields the onset of the current excursion, the bin an online detector would have
// fired in, and the excess since then (onset_host.h Row). Nothing is kept between steps but the ring:
// the result is a pure function of the ring and the parameters. Integers only, so host and device
// agree bit for bit. The engine, its graphs and its streams are not touched. pipeline/onset.py holds
// the same rules in numpy (the oracle, and what the CPU engine uses).
//
// Native, no PyTorch, plain launches (no graphs) on a step lane of its own (steplane.h: the stream, the
// copy of the window's span ranges, the result slots, the publish). One step per window with a timed cut, between the
// lane's copy and its publish:
//   advance  clear the slots of the bins (previous q_hi, q_hi] in every row; not launched when q_hi
//            did not move,
//   observe  one thread per record: one 64-bit add into its (service, slot) cell; with `lds` every
//            workgroup aggregates its cells in an LDS table first,
//   scan     one wave per service row, every row of group_cap: the CUSUM as a wave scan of
//            (sum, minimum prefix) pairs (onset_host.h combine), then onset, alarm, peak and counts.
#pragma once

#include <hip/hip_runtime.h>

#include <stdexcept>
#include <vector>

#include "mislo_common.h"
#include "onset_host.h"
#include "steplane.h"

namespace mislo {

namespace onset {

// the whole ring as the host reads it back, bins in slot order
struct Resident {
  std::vector<unsigned long long> cells;  // [group_cap][bins]
  int64_t q_hi = kNoBin;
};

}  // namespace onset

class OnsetTracker {
 public:
  explicit OnsetTracker(const onset::Config& cfg);

  // One window cut at cut_ns (> 0); returns the step's index. The ranges are read before it returns.
  int64_t step(const std::vector<onset::Range>& spans, int64_t cut_ns, int n_groups);
  bool query(int64_t i) { return lane_.query(i); }
  // the step's result block (onset::layout), valid until n_buffers later steps; waits for it
  const uint32_t* results(int64_t i) { return lane_.results(i); }
  // device time of the step: (copy + kernels, kernels alone, the observe kernel alone), ms
  std::vector<float> step_ms(int64_t i);
  // the ring and q_hi (synchronous; tests)
  onset::Resident resident();
  void sync() { lane_.sync(); }
  // checkpoint (steplane.h): the lane, and the host integers kept between steps: q_hi and the spans the
  // ring's bound counts (restored as if all of them had come with the last step: never fewer than were)
  StepLane& lane() { return lane_; }
  std::vector<int64_t> host_words() const { return {q_hi_, q_hi_ == onset::kNoBin ? 0 : pop_.after(q_hi_, 0)}; }
  void set_host_words(const int64_t* w, int n) {
    if (n != 2 || w[1] < 0) throw std::invalid_argument("breach onset image: host words");
    q_hi_ = w[0];
    if (q_hi_ != onset::kNoBin) pop_.take(q_hi_, (size_t)w[1]);
  }
  int64_t q_hi() const { return q_hi_; }
  const onset::Config& config() const { return cfg_; }
  const onset::Layout& result_layout() const { return lay_; }

 private:
  onset::Config cfg_;
  onset::Layout lay_;
  onset::Population pop_;
  int64_t q_hi_ = onset::kNoBin;
  StepLane lane_;
  unsigned long long* ring_ = nullptr;  // [group_cap][bins] cells, the lane's
};

}  // namespace mislo
