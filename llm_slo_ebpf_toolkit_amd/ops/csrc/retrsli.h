// TTFT phase split: per-service retrieval time against model time, and the TTFT breaches by phase.
//
// A trace's first record carries its TTFT and, where the application reports a breakdown, the sum of its
// retrieval times (Span::retr_ms; collector/otlp.py). The posterior sees a group mean of it; this side
// tracker keeps the distribution. Per service, for the window and for a rolling horizon of W windows: a
// histogram of the retrieval time and one of the model time (TTFT minus retrieval), both in units of 10 us
// with the decode SLI's bucket rule (decodesli_host.h bucket_of: read off the integer, so host and device
// agree bit for bit) and their p50 / p90 / p95 / p99 buckets; the exact sums of retrieval time and of
// TTFT; six counters of requests by breach phase (retrsli_host.h cell_of); the SLI-counting records seen
// (the coverage's denominator); and a verdict over the horizon decided here in integers (state_of) with
// the steps it has held. The engine, its graphs and its streams are not touched. pipeline/retrsli.py holds
// the same rules in numpy (the oracle, and what the CPU engine uses).
//
// Native, no PyTorch, plain launches (no graphs) on a step lane of its own (steplane.h: the stream, the
// copy of the window's span ranges, the result slots, the publish). One step per window, between the
// lane's copy and its publish:
//   observe  one thread per record: up to six adds per observed record (its retrieval bucket, its model
//            bucket, its cell, the two 64-bit sums, the SLI count). With `lds` every workgroup aggregates
//            in an LDS table first and sends each key once. Not launched for an empty step,
//   roll     two waves per service row, one per histogram, every row of group_cap: the window of W steps
//            ago leaves the rolling row, this one enters and takes its place, the step's row is cleared;
//            the four ranks of the window's and the rolling row by a wave scan; the wave of the retrieval
//            histogram rolls the counters and the sums alike and its lane 0 decides the verdict.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "mislo_common.h"
#include "retrsli_host.h"
#include "steplane.h"

namespace mislo {

namespace retrsli {

// the rolling state as the host reads it back
struct Resident {
  std::vector<uint32_t> rows_r;           // [group_cap][kK]
  std::vector<uint32_t> rows_m;           // [group_cap][kK]
  std::vector<uint32_t> cells;            // [group_cap][kCellStride]: six cells, sli, a spare word
  std::vector<unsigned long long> sums;   // [group_cap][2]: retrieval, TTFT
  std::vector<uint32_t> state;            // [group_cap]
  std::vector<uint32_t> age;              // [group_cap]
  int64_t pos = 0;                        // the horizon row the next step replaces: steps % W
};

}  // namespace retrsli

class RetrievalSliTracker {
 public:
  explicit RetrievalSliTracker(const retrsli::Config& cfg);

  // One window; returns the step's index. The ranges are read before it returns.
  int64_t step(const std::vector<retrsli::Range>& spans, int n_groups);
  bool query(int64_t i) { return lane_.query(i); }
  // the step's result block (retrsli::layout), valid until n_buffers later steps; waits for it
  const uint32_t* results(int64_t i) { return lane_.results(i); }
  // device time of the step: (copy + kernels, kernels alone, the observe kernel alone), ms
  std::vector<float> step_ms(int64_t i);
  // the rolling rows, counters, sums, verdicts and the ring position (synchronous; tests)
  retrsli::Resident resident();
  void sync() { lane_.sync(); }
  // checkpoint (steplane.h): the lane; this tracker keeps no host integers between steps
  StepLane& lane() { return lane_; }
  std::vector<int64_t> host_words() const { return {}; }
  void set_host_words(const int64_t*, int) {}
  const retrsli::Config& config() const { return cfg_; }
  const retrsli::Layout& result_layout() const { return lay_; }
  uint32_t slo_units() const { return slo_u_; }
  uint32_t budget_units() const { return budget_u_; }

 private:
  // row `which` of the state: [0, W) the horizon's windows, W the rolling row, W + 1 this step's
  uint32_t* hist_r(size_t which) const { return hist_r_ + which * (size_t)cfg_.group_cap * retrsli::kK; }
  uint32_t* hist_m(size_t which) const { return hist_m_ + which * (size_t)cfg_.group_cap * retrsli::kK; }
  uint32_t* cells(size_t which) const { return cells_ + which * (size_t)cfg_.group_cap * retrsli::kCellStride; }
  unsigned long long* sums(size_t which) const { return sum_ + which * (size_t)cfg_.group_cap * 2; }

  retrsli::Config cfg_;
  retrsli::Layout lay_;
  uint32_t slo_u_ = 0, budget_u_ = 0;
  StepLane lane_;
  uint32_t* hist_r_ = nullptr;  // the lane's, like the four below
  uint32_t* hist_m_ = nullptr;
  uint32_t* cells_ = nullptr;
  unsigned long long* sum_ = nullptr;
  uint32_t* verdict_ = nullptr;  // [2][group_cap]: state, age
};

}  // namespace mislo
