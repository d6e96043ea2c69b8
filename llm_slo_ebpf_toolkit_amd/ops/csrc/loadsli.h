// Load SLI per service: arrivals, completions, requests in flight and the exact busy time over a ring
// of absolute time bins, and whether the recent bins show a surge (more arrivals), a slowdown (more
// in flight at the same arrivals) or a drop against the bins before them.
//
// Every record that ends a request carries its start (Span::ts_ns) and its duration (Span::latency_ms):
// an interval [start, end). Per (service, bin) the ring keeps two u64 cells (loadsli_host.h): the
// starts and ends counted in the bin, and the time of the bin its starting and ending requests did
// not spend in flight. Per service `carry` is the number in flight before the ring's oldest bin. A
// prefix sum of starts - ends from carry gives the requests touching every bin, and from the idle time
// the exact in-flight time inside it -- a late record revises the past. Integers only, so host and
// device agree bit for bit. The engine, its graphs and its streams are not touched.
// pipeline/loadsli.py holds the same rules in numpy (the oracle, and what the CPU engine uses).
//
// Native, no PyTorch, plain launches (no graphs) on a step lane of its own (steplane.h: the stream, the
// copy of the window's span ranges, the result slots, the publish). One step per window with a timed cut, between the
// lane's copy and its publish:
//   advance  one wave per row: fold the evicted bins' starts - ends into carry and clear their slots;
//            not launched when q_hi did not move,
//   observe  one thread per record, at most two cell updates; with `lds` every workgroup aggregates
//            its cells, carry increments and statistics in an LDS table first,
//   scan     one wave per service row, every row of group_cap: a wave scan of starts - ends, then the
//            three ranges' sums and the peak in one pass; lane 0 classifies and stores the row.
#pragma once

#include <hip/hip_runtime.h>

#include <stdexcept>
#include <vector>

#include "loadsli_host.h"
#include "mislo_common.h"
#include "steplane.h"

namespace mislo {

namespace loadsli {

// everything kept between steps as the host reads it back, bins in slot order
struct Resident {
  std::vector<unsigned long long> counts, idle_us;  // [group_cap][bins]
  std::vector<int32_t> carry;                       // [group_cap]
  std::vector<uint32_t> age, prev_state;            // [group_cap]
  int64_t q_hi = kNoBin, q_first = kNoBin;
};

}  // namespace loadsli

class LoadSliTracker {
 public:
  explicit LoadSliTracker(const loadsli::Config& cfg);

  // One window cut at cut_ns (> 0); returns the step's index. The ranges are read before it returns.
  int64_t step(const std::vector<loadsli::Range>& spans, int64_t cut_ns, int n_groups);
  bool query(int64_t i) { return lane_.query(i); }
  // the step's result block (loadsli::layout), valid until n_buffers later steps; waits for it
  const uint32_t* results(int64_t i) { return lane_.results(i); }
  // device time of the step: (copy + kernels, kernels alone, the observe kernel alone), ms
  std::vector<float> step_ms(int64_t i);
  // the ring and what goes with it (synchronous; tests)
  loadsli::Resident resident();
  void sync() { lane_.sync(); }
  // checkpoint (steplane.h): the lane, and the host integers kept between steps: q_hi, q_first and the
  // spans the ring's bound counts (restored as if all of them had come with the last step: never fewer)
  StepLane& lane() { return lane_; }
  std::vector<int64_t> host_words() const {
    return {q_hi_, q_first_, q_hi_ == loadsli::kNoBin ? 0 : pop_.after(q_hi_, 0)};
  }
  void set_host_words(const int64_t* w, int n) {
    if (n != 3 || w[2] < 0) throw std::invalid_argument("load sli image: host words");
    q_hi_ = w[0], q_first_ = w[1];
    if (q_hi_ != loadsli::kNoBin) pop_.take(q_hi_, (size_t)w[2]);
  }
  int64_t q_hi() const { return q_hi_; }
  const loadsli::Config& config() const { return cfg_; }
  const loadsli::Layout& result_layout() const { return lay_; }

 private:
  loadsli::Config cfg_;
  loadsli::Layout lay_;
  loadsli::Population pop_;
  int64_t q_hi_ = loadsli::kNoBin, q_first_ = loadsli::kNoBin;
  StepLane lane_;
  // the lane's
  unsigned long long* counts_ = nullptr;  // [group_cap][bins]
  unsigned long long* idle_ = nullptr;    // [group_cap][bins]
  int32_t* carry_ = nullptr;              // [group_cap]
  uint32_t* age_ = nullptr;               // [group_cap] age, then [group_cap] previous state
};

}  // namespace mislo
