// Per-pod TTFT breach breakdown: per service, how many pods were seen, how many of them breached,
// and the K pods with the most breaches, of the window and of the last H windows.
//
// Every other reduction is keyed by service alone, so one bad replica and a service-wide stall look
// the same. This side tracker aggregates the window's counted span records under the composite key
// (service, pod) in an open-addressing table (podrank_host.h: pair_key, slot_of), keeps the horizon
// as H compact per-window pair lists, rebuilds the `recent` table from them every step and ranks the
// pairs of both scopes by one 64-bit key (rank_key), so host and device agree bit for bit. Integer
// atomics only. The engine, its graphs and its streams are not touched. pipeline/podrank.py holds
// the same rules in numpy (the oracle, and what the CPU engine uses).
//
// Native, no PyTorch, plain launches (no graphs) on a step lane of its own (steplane.h: the stream, the
// copy of the window's span ranges, the result slots, the publish). One step per window, between the
// lane's copy and its publish:
//   observe  one thread per record: insert or add into the window's table and the service totals;
//            with `lds` every workgroup aggregates its pairs and totals in LDS first,
//   rank     one thread per window-table slot: append the pair to the horizon's list step % H,
//            count the service's pods, cascade the pair's rank key into the service's K slots
//            (per workgroup in LDS for the first services, then into the global slots),
//   roll     one thread per entry of the H lists: insert or add into the recent table,
//   rank     the same over the recent table,
//   gather   one wave per service row, every row of group_cap: keys into rows by probing the
//            tables, the totals of the window and of the horizon,
//   publish  this tracker's own kernel in place of the lane's: the result block into its pinned host block
//            (vector stores); clears the block and both tables. Then the lane's finish().
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "mislo_common.h"
#include "podrank_host.h"
#include "steplane.h"

namespace mislo {

namespace podrank {

// a pair table or list, structure of arrays
struct Pairs {
  unsigned long long* key = nullptr;  // pair_key, 0 = empty
  uint32_t* n = nullptr;
  uint32_t* b = nullptr;
  uint32_t* max = nullptr;            // ord bits of the largest TTFT
  unsigned long long* sum = nullptr;  // milli units
};

// one horizon list's pairs as the host reads them back
struct PairList {
  std::vector<unsigned long long> key, sum;
  std::vector<uint32_t> n, b, max;
};

}  // namespace podrank

class PodRankTracker {
 public:
  explicit PodRankTracker(const podrank::Config& cfg);

  // One window; returns the step's index. The ranges are read before it returns.
  int64_t step(const std::vector<podrank::Range>& spans, int n_groups);
  bool query(int64_t i) { return lane_.query(i); }
  // the step's result block (podrank::layout), valid until n_buffers later steps; waits for it
  const uint32_t* results(int64_t i) { return lane_.results(i); }
  // device time of the step: (copy + kernels, kernels alone, the observe kernel alone), ms
  std::vector<float> step_ms(int64_t i);
  // the horizon's H pair lists, slot = step % windows, in no particular order (synchronous; tests)
  std::vector<podrank::PairList> resident();
  void sync() { lane_.sync(); }
  // checkpoint (steplane.h): the lane; this tracker keeps no host integers between steps
  StepLane& lane() { return lane_; }
  std::vector<int64_t> host_words() const { return {}; }
  void set_host_words(const int64_t*, int) {}
  const podrank::Config& config() const { return cfg_; }
  const podrank::Layout& result_layout() const { return lay_; }

 private:
  podrank::Pairs zeroed_pairs(size_t n);

  podrank::Config cfg_;
  podrank::Layout lay_;
  uint32_t wslots_ = 0, rslots_ = 0;
  StepLane lane_;
  // the lane's
  podrank::Pairs win_, rec_, lists_;     // [wslots] [rslots] [windows][pair_cap]
  uint32_t* ctrl_ = nullptr;             // [0] pairs claimed in the window's table, [1 + h] length of list h
  uint32_t* tot_ = nullptr;              // [2][group_cap] the step's n and b per service
  uint32_t* hist_ = nullptr;             // [windows][2][group_cap] the same of the horizon's steps
  unsigned long long* top_ = nullptr;    // [2][group_cap][k] the scopes' rank keys, 0 = empty
};

}  // namespace mislo
