// TTFT sketch: per-service TTFT distributions of the window and of a rolling horizon.
//
// k_decode_spans reduces every TTFT to (requests, breaches) per service and window; this side
// tracker keeps the value: a histogram per service with 16 linear sub-buckets per octave over
// [0.125 ms, 2^21 ms) (slisketch_host.h: the bucket is read off the float's bits, so host and device
// agree bit for bit), the last W windows' histograms and their running sum, and per step the
// p50 / p90 / p95 / p99 buckets of both, exact `le` counts at REF's llm_slo_ttft_ms boundaries, the
// count and an exact fixed-point sum. The engine, its graphs and its streams are not touched.
// pipeline/slisketch.py holds the same rules in numpy (the oracle, and what the CPU engine uses).
//
// Native, no PyTorch, plain launches (no graphs) on a step lane of its own (steplane.h: the stream, the
// copy of the window's span ranges, the result slots, the publish). One step per window, between the
// lane's copy and its publish:
//   observe  one thread per record: integer atomics into the window's histogram row, the `le`
//            counts and the 64-bit milli-unit sum (no float atomics: bit-reproducible),
//   roll     one wave per service row: rolling += this window - the window of W steps ago (every
//            row of group_cap, so a service absent from this step is still evicted), a cross-lane
//            inclusive scan of the window's and the rolling row, the four ranks of each.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "mislo_common.h"
#include "slisketch_host.h"
#include "steplane.h"

namespace mislo {

namespace slisketch {

// slisketch.hip launchers (plain pointers + stream)
void launch_observe(const Span* sp, int n, int n_groups, uint32_t* cur, uint32_t* le, unsigned long long* sum,
                    uint32_t* stats, hipStream_t st);
void launch_roll(uint32_t* cur, uint32_t* slot, uint32_t* roll, unsigned long long* sum, uint32_t* block, Layout lay,
                 int group_cap, hipStream_t st);

}  // namespace slisketch

class SliSketch {
 public:
  explicit SliSketch(const slisketch::Config& cfg);

  // One window; returns the step's index. The ranges are read before it returns.
  int64_t step(const std::vector<slisketch::Range>& spans, int n_groups);
  bool query(int64_t i) { return lane_.query(i); }
  // the step's result block (slisketch::layout), valid until n_buffers later steps; waits for it
  const uint32_t* results(int64_t i) { return lane_.results(i); }
  // device time of the step: (copy + kernels, kernels alone), ms
  std::pair<float, float> step_ms(int64_t i);
  // the rolling histogram / the last step's window histogram, [group_cap][kK] (synchronous; tests)
  std::vector<uint32_t> rolling();
  std::vector<uint32_t> window_hist();
  void sync() { lane_.sync(); }
  // checkpoint (steplane.h): the lane; this tracker keeps no host integers between steps
  StepLane& lane() { return lane_; }
  std::vector<int64_t> host_words() const { return {}; }
  void set_host_words(const int64_t*, int) {}
  const slisketch::Config& config() const { return cfg_; }
  const slisketch::Layout& result_layout() const { return lay_; }
  int64_t steps() const { return lane_.steps(); }

 private:
  uint32_t* rows(size_t which) const { return hist_ + which * row_words_; }
  std::vector<uint32_t> read_rows(const uint32_t* dev);

  slisketch::Config cfg_;
  slisketch::Layout lay_;
  size_t row_words_ = 0;  // group_cap * kRowStride
  StepLane lane_;
  // the lane's
  uint32_t* hist_ = nullptr;  // [windows] the horizon's windows, [windows] rolling, [windows + 1] this step's
  unsigned long long* sum_ = nullptr;
};

}  // namespace mislo
