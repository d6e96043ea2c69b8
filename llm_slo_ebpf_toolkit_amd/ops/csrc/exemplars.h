// Request exemplars: per service, the records with the largest TTFT of the window and of the last
// H windows.
//
// k_decode_spans reduces every TTFT to counters and the TTFT sketch to histograms: neither can name
// a request. This side tracker keeps, per service (incident group) and step, the K records with the
// largest TTFT of the window and the K largest over a horizon of H steps, each as a 64-byte row
// (exemplars_host.h Row: trace, span id, TTFT, latency, retrieval time, pod, pid). Order and ties
// are one 64-bit key (exemplars_host.h), so host and device agree bit for bit. The engine, its graphs
// and its streams are not touched. pipeline/exemplars.py holds the same rules in numpy (the oracle,
// and what the CPU engine uses).
//
// Native, no PyTorch, plain launches (no graphs) on a step lane of its own (steplane.h: the stream, the
// copy of the window's span ranges, the result slots, the publish). One step per window, between the
// lane's copy and its publish:
//   select   one thread per record: the key cascades into the group's K sorted slots by atomicMax
//            (integer atomics only), privatised in LDS for the groups below kLdsGroups,
//   merge    one wave per service row, every row of group_cap: lanes < K gather the window's rows
//            from the span buffer into the horizon's slot step % H and the block, the wave ranks the
//            H * K resident candidates and writes the K best with their age.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "exemplars_host.h"
#include "mislo_common.h"
#include "steplane.h"

namespace mislo {

namespace exemplars {

// exemplars.hip launchers (plain pointers + stream)
void launch_select(const Span* sp, int n, int n_groups, int k, bool lds, unsigned long long* keys, uint32_t* count,
                   uint32_t* stats, hipStream_t st);
void launch_merge(const Span* sp, int n, unsigned long long* keys, uint32_t* count, Row* horizon, uint32_t* held,
                  uint32_t* block, Layout lay, int group_cap, int k, int windows, int cur, hipStream_t st);

}  // namespace exemplars

class ExemplarTracker {
 public:
  explicit ExemplarTracker(const exemplars::Config& cfg);

  // One window; returns the step's index. The ranges are read before it returns.
  int64_t step(const std::vector<exemplars::Range>& spans, int n_groups);
  bool query(int64_t i) { return lane_.query(i); }
  // the step's result block (exemplars::layout), valid until n_buffers later steps; waits for it
  const uint32_t* results(int64_t i) { return lane_.results(i); }
  // device time of the step: (copy + kernels, kernels alone, the select kernel alone), ms
  std::vector<float> step_ms(int64_t i);
  // the horizon's rows [windows][group_cap][k] and their valid counts [windows][group_cap]
  // (synchronous; tests)
  std::pair<std::vector<exemplars::Row>, std::vector<uint32_t>> resident();
  void sync() { lane_.sync(); }
  // checkpoint (steplane.h): the lane; this tracker keeps no host integers between steps
  StepLane& lane() { return lane_; }
  std::vector<int64_t> host_words() const { return {}; }
  void set_host_words(const int64_t*, int) {}
  const exemplars::Config& config() const { return cfg_; }
  const exemplars::Layout& result_layout() const { return lay_; }
  int64_t steps() const { return lane_.steps(); }

 private:
  exemplars::Config cfg_;
  exemplars::Layout lay_;
  StepLane lane_;
  // the lane's
  unsigned long long* keys_ = nullptr;  // [group_cap][k] the step's sorted slots, 0 = empty
  uint32_t* count_ = nullptr;           // [group_cap] records observed in the step
  exemplars::Row* horizon_ = nullptr;   // [windows][group_cap][k]
  uint32_t* held_ = nullptr;            // [windows][group_cap] valid rows
};

}  // namespace mislo
