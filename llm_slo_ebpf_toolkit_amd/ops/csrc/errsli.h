// Error SLI: per-service requests by outcome class, and the burn of the availability error budget.
//
// Every other reduction is a latency. A finished request's span also carries how it ended, as a class
// in bits 4-7 of Span::flags (errsli_host.h outcome_of; 0 = ok). This side tracker keeps, per service,
// the requests by class for the window and for a rolling horizon of W windows, and evaluates up to four
// (long window, short window, factor) pairs of the multi-window, multi-burn-rate rule every window, in
// integers: a pair fires when both its windows spend the budget at least `factor` times as fast as the
// target allows; `age` counts the consecutive windows something fires. The engine, its graphs and its
// streams are not touched. pipeline/errsli.py holds the same rules in numpy (the oracle, and what the
// CPU engine uses).
//
// Native, no PyTorch, plain launches (no graphs) on a step lane of its own (steplane.h: the stream, the
// copy of the window's span ranges, the result slots and the publish). One step per window, between the
// lane's copy and its publish:
//   observe  one thread per record: an add into its (service, class) cell. A service's requests fall
//            into one or two classes, so with `lds` every workgroup aggregates in an LDS table first.
//            Not launched for an empty step,
//   roll     one wave per service row, every row of group_cap: lanes 0-7 roll the class counts (the
//            window of W steps ago leaves, this one enters and takes its place, the step's row is
//            cleared), lanes 8-15 each keep one pair window's rolling (n, bad) and compare it; a ballot
//            gives the firing pairs.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "errsli_host.h"
#include "mislo_common.h"
#include "steplane.h"

namespace mislo {

namespace errsli {

// the rolling state as the host reads it back
struct Resident {
  std::vector<uint32_t> counts;  // [group_cap][8]
  std::vector<uint32_t> sums;    // [group_cap][4][4]
  std::vector<uint32_t> age;     // [group_cap]
  int64_t pos = 0;               // the horizon row the next step replaces: steps % W
};

}  // namespace errsli

class ErrorSliTracker {
 public:
  explicit ErrorSliTracker(const errsli::Config& cfg);

  // One window; returns the step's index. The ranges are read before it returns.
  int64_t step(const std::vector<errsli::Range>& spans, int n_groups);
  bool query(int64_t i) { return lane_.query(i); }
  // the step's result block (errsli::layout), valid until n_buffers later steps; waits for it
  const uint32_t* results(int64_t i) { return lane_.results(i); }
  // device time of the step: (copy + kernels, kernels alone, the observe kernel alone), ms
  std::vector<float> step_ms(int64_t i);
  // the rolling counts, the pairs' sums, the ages and the ring position (synchronous; tests)
  errsli::Resident resident();
  void sync() { lane_.sync(); }
  // checkpoint (steplane.h): the lane; this tracker keeps no host integers between steps
  StepLane& lane() { return lane_; }
  std::vector<int64_t> host_words() const { return {}; }
  void set_host_words(const int64_t*, int) {}
  const errsli::Config& config() const { return cfg_; }
  const errsli::Layout& result_layout() const { return lay_; }
  uint32_t budget_ppm() const { return budget_; }

 private:
  // row `which` of the state: [0, W) the horizon's windows, W the rolling row, W + 1 this step's
  uint32_t* row(size_t which) const { return rows_ + which * (size_t)cfg_.group_cap * errsli::kRowWords; }

  errsli::Config cfg_;
  errsli::Layout lay_;
  uint32_t budget_ = 0;
  StepLane lane_;
  uint32_t* rows_ = nullptr;  // the lane's, like the two below
  uint32_t* sums_ = nullptr;  // [group_cap][4][4]
  uint32_t* age_ = nullptr;   // [group_cap]
};

}  // namespace mislo
