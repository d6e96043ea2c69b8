// Saturation curve per service: requests and TTFT breaches by the concurrency of the time bin the
// request arrived in, the concurrency above which the SLO's error budget is exceeded (the knee), and
// whether the service's recent concurrency is below it.
//
// The load tracker's ring (loadsli.h) gives every bin its exact busy time, hence a concurrency level
// (satcurve_host.h: 160 levels, exact to 1/8 below 2, 16 per octave above). A third u64 cell per
// (service, bin), `sli`, counts the requests with a TTFT that started in the bin and those above the
// SLO. A bin that leaves the ring is final: its (requests, breaches) are folded into the generation of
// its epoch under its level; two generations per service alternate, so the curve forgets after one to
// two epochs without halving anything. Every step the settled ring bins are merged with the live
// generations into a curve of 160 x (n, b); the knee is the maximum-suffix-sum change point of
// b * 10^6 - budget_ppm * n. Integers only, so host and device agree bit for bit. The engine, its
// graphs and its streams are not touched; the load tracker's ring is not shared.
// pipeline/satcurve.py holds the same rules in numpy (the oracle, and what the CPU engine uses).
//
// Native, no PyTorch, plain launches (no graphs) on a step lane of its own (steplane.h: the stream, the
// copy of the window's span ranges, the result slots, the publish). One step per window with a timed cut, between the
// lane's copy and its publish:
//   clear    the generations the step's evicted epochs invalidate (the host keeps their epochs),
//   fold     one wave per row: a wave scan of the evicted bins' starts - ends from carry gives every
//            evicted bin its level; bins with whole history add their sli into the row's generation,
//            the three cells are cleared, carry moves on; not launched when q_hi did not move,
//   observe  one thread per record, at most two cell updates and one sli add; with `lds` every
//            workgroup aggregates its cells, carry increments and statistics in an LDS table first,
//   scan     one wave per service row, every row of group_cap: the load tracker's scan, the settled
//            bins' sli into a wave-private LDS histogram by level, the recent busy time; then three
//            levels a lane: the live generations added, the suffix scan of the scores, the arg-max,
//            the suffix counts at the knee; lane 0 decides the state and stores the row.
// The lane's publish clears the statistics alone: the rows and the curve are rewritten whole by every scan.
#pragma once

#include <hip/hip_runtime.h>

#include <stdexcept>
#include <vector>

#include "mislo_common.h"
#include "satcurve_host.h"
#include "steplane.h"

namespace mislo {

namespace satcurve {

// everything kept between steps as the host reads it back, bins in slot order
struct Resident {
  std::vector<unsigned long long> counts, idle_us, sli;  // [group_cap][bins]
  std::vector<int32_t> carry;                            // [group_cap]
  std::vector<unsigned long long> gen;                   // [2][group_cap][kK][2]: (n, b), a generation contiguous
  std::vector<uint32_t> age;                             // [group_cap]
  int64_t gen_epoch[2] = {-1, -1};
  int64_t q_hi = kNoBin, q_first = kNoBin;
};

}  // namespace satcurve

class SaturationTracker {
 public:
  explicit SaturationTracker(const satcurve::Config& cfg);

  // One window cut at cut_ns (> 0); returns the step's index. The ranges are read before it returns.
  int64_t step(const std::vector<satcurve::Range>& spans, int64_t cut_ns, int n_groups);
  bool query(int64_t i) { return lane_.query(i); }
  // the step's result block (satcurve::layout), valid until n_buffers later steps; waits for it
  const uint32_t* results(int64_t i) { return lane_.results(i); }
  // device time of the step: (copy + kernels, kernels alone, the observe kernel alone), ms
  std::vector<float> step_ms(int64_t i);
  // the ring, the generations and what goes with them (synchronous; tests)
  satcurve::Resident resident();
  void sync() { lane_.sync(); }
  // checkpoint (steplane.h): the lane, and the host integers kept between steps: q_hi, q_first, the two
  // generations' epochs and the spans the two bounds count (restored as if all of them had come with the
  // last step: never fewer than were)
  StepLane& lane() { return lane_; }
  std::vector<int64_t> host_words() const {
    const bool none = q_hi_ == satcurve::kNoBin;
    return {q_hi_, q_first_, gens_.epoch[0], gens_.epoch[1], none ? 0 : ring_pop_.after(q_hi_, 0),
            none ? 0 : curve_pop_.after(q_hi_, 0)};
  }
  void set_host_words(const int64_t* w, int n) {
    if (n != 6 || w[4] < 0 || w[5] < 0) throw std::invalid_argument("saturation curve image: host words");
    q_hi_ = w[0], q_first_ = w[1], gens_.epoch[0] = w[2], gens_.epoch[1] = w[3];
    if (q_hi_ != satcurve::kNoBin) ring_pop_.take(q_hi_, (size_t)w[4]), curve_pop_.take(q_hi_, (size_t)w[5]);
  }
  int64_t q_hi() const { return q_hi_; }
  const satcurve::Config& config() const { return cfg_; }
  const satcurve::Layout& result_layout() const { return lay_; }

 private:
  satcurve::Config cfg_;
  satcurve::Layout lay_;
  satcurve::RingPopulation ring_pop_;
  satcurve::CurvePopulation curve_pop_;
  satcurve::Generations gens_;
  int64_t q_hi_ = satcurve::kNoBin, q_first_ = satcurve::kNoBin;
  StepLane lane_;
  // the lane's
  unsigned long long* counts_ = nullptr;  // [group_cap][bins]
  unsigned long long* idle_ = nullptr;    // [group_cap][bins]
  unsigned long long* sli_ = nullptr;     // [group_cap][bins]
  unsigned long long* gen_ = nullptr;     // [2][group_cap][kK][2]
  int32_t* carry_ = nullptr;              // [group_cap]
  uint32_t* age_ = nullptr;               // [group_cap]
};

}  // namespace mislo
