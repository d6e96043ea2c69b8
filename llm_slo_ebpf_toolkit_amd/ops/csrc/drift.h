// TTFT drift: per service, is the recent TTFT distribution stochastically slower (or faster) than a
// trailing baseline of calm windows?
//
// Every decision about a service is a function of its breach count, so a fault that moves its TTFT
// towards the SLO without crossing it is invisible. This side tracker keeps, per service, a recent
// histogram (the last R windows), a baseline histogram (the last B calm, non-empty windows, trailing
// the recent one by a gap of L windows) and decides every window, in integers, by a one-sided
// two-sample Kolmogorov-Smirnov test with a minimum quantile shift (docs/TTFT_DRIFT.md is the
// contract). The bucket rule, the rank rule and the row layout are the TTFT sketch's
// (slisketch_host.h). The engine, its graphs and its streams are not touched. pipeline/drift.py holds
// the same rules in numpy (the oracle, and what the CPU engine uses).
//
// Native, no PyTorch, plain launches (no graphs) on a step lane of its own (steplane.h: the stream, the
// copy of the window's span ranges, the result slots, the publish). One step per window, between the
// lane's copy and its publish:
//   observe  one thread per record: an add into its (service, bucket) cell of the step's row. One
//            service's TTFTs share few buckets: with `lds` every workgroup aggregates in an LDS table
//            first. Not launched for an empty step,
//   roll     one wave per service row, every row of group_cap: the three ring updates, two wave scans,
//            the two cross-multiplied maxima with their first bucket, the ranks, then lane 0 decides,
//            counts the hold and drops the baseline when it is reached.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "drift_host.h"
#include "mislo_common.h"
#include "steplane.h"

namespace mislo {

namespace drift {

// the rolling state as the host reads it back
struct Resident {
  std::vector<uint32_t> recent;     // [group_cap][kRowStride]
  std::vector<uint32_t> base;       // [group_cap][kRowStride]
  std::vector<uint32_t> base_fill;  // [group_cap]
  std::vector<uint32_t> base_pos;   // [group_cap]
  std::vector<uint32_t> hold;       // [group_cap]
  int64_t pos = 0;                  // the near-ring row the next step replaces: steps % (R + L)
};

// per-service words beside the histograms: base_fill, base_pos, hold, the state of the step before
struct Words {
  uint32_t* base_fill;
  uint32_t* base_pos;
  uint32_t* hold;
  uint32_t* prev;
};

}  // namespace drift

class DriftTracker {
 public:
  explicit DriftTracker(const drift::Config& cfg);

  // One window; returns the step's index. The ranges are read before it returns.
  int64_t step(const std::vector<drift::Range>& spans, int n_groups);
  bool query(int64_t i) { return lane_.query(i); }
  // the step's result block (drift::layout), valid until n_buffers later steps; waits for it
  const uint32_t* results(int64_t i) { return lane_.results(i); }
  // device time of the step: (copy + kernels, kernels alone, the observe kernel alone), ms
  std::vector<float> step_ms(int64_t i);
  // the recent and baseline rows, fill, position, hold and the ring position (synchronous; tests)
  drift::Resident resident();
  void sync() { lane_.sync(); }
  // checkpoint (steplane.h): the lane; this tracker keeps no host integers between steps
  StepLane& lane() { return lane_; }
  std::vector<int64_t> host_words() const { return {}; }
  void set_host_words(const int64_t*, int) {}
  const drift::Config& config() const { return cfg_; }
  const drift::Layout& result_layout() const { return lay_; }

 private:
  // row `which` of the state: [0, R + L) the near ring, then recent, base, this step's, base_ring[B]
  uint32_t* row(size_t which) const { return hist_ + which * (size_t)cfg_.group_cap * drift::kRowStride; }

  drift::Config cfg_;
  drift::Layout lay_;
  StepLane lane_;
  uint32_t* hist_ = nullptr;   // the lane's, like words_
  uint32_t* words_ = nullptr;  // [4][group_cap]: drift::Words
};

}  // namespace mislo
