// Decode-phase SLI: per-service time per output token (TPOT), and requests by (TTFT breach, TPOT breach).
//
// Every other reduction is a view of TTFT. A finished request's span also carries its TPOT, as integer
// microseconds in bits 8-31 of Span::flags (decodesli_host.h tpot_of; 0 = none). This side tracker
// keeps, per service, for the window and for a rolling horizon of W windows: a histogram of TPOT with
// 16 buckets per octave read off the integer (bucket_of: no float, so host and device agree bit for
// bit) and its p50 / p90 / p95 / p99 buckets, the exact sum in microseconds, and the 2x2 table of
// requests by (TTFT > slo, TPOT > slo). Cell 0, neither breached, is the service's goodput; the
// off-diagonal cells tell a prefill problem from a decode problem. The engine, its graphs and its
// streams are not touched. pipeline/decodesli.py holds the same rules in numpy (the oracle, and what
// the CPU engine uses).
//
// Native, no PyTorch, plain launches (no graphs) on a step lane of its own (steplane.h: the stream, the
// copy of the window's span ranges, the result slots, the publish). One step per window, between the
// lane's copy and its publish:
//   observe  one thread per record: an add into its (service, bucket) cell, its (service, table cell)
//            and the service's 64-bit sum. All requests of a service run one model on one machine, so
//            their TPOTs share a few buckets: with `lds` every workgroup aggregates in an LDS table
//            first. Not launched for an empty step,
//   roll     one wave per service row, every row of group_cap: the window of W steps ago leaves the
//            rolling row, this one enters and takes its place, the step's row is cleared; the four
//            ranks of the window's and the rolling row by a wave scan; table and sum roll alike.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "decodesli_host.h"
#include "mislo_common.h"
#include "steplane.h"

namespace mislo {

namespace decodesli {

// the rolling state as the host reads it back
struct Resident {
  std::vector<uint32_t> rows;             // [group_cap][kK]
  std::vector<uint32_t> cells;            // [group_cap][4]
  std::vector<unsigned long long> sums;   // [group_cap]
  int64_t pos = 0;                        // the horizon row the next step replaces: steps % W
};

}  // namespace decodesli

class DecodeSliTracker {
 public:
  explicit DecodeSliTracker(const decodesli::Config& cfg);

  // One window; returns the step's index. The ranges are read before it returns.
  int64_t step(const std::vector<decodesli::Range>& spans, int n_groups);
  bool query(int64_t i) { return lane_.query(i); }
  // the step's result block (decodesli::layout), valid until n_buffers later steps; waits for it
  const uint32_t* results(int64_t i) { return lane_.results(i); }
  // device time of the step: (copy + kernels, kernels alone, the observe kernel alone), ms
  std::vector<float> step_ms(int64_t i);
  // the rolling rows, table and sums and the ring position (synchronous; tests)
  decodesli::Resident resident();
  void sync() { lane_.sync(); }
  // checkpoint (steplane.h): the lane; this tracker keeps no host integers between steps
  StepLane& lane() { return lane_; }
  std::vector<int64_t> host_words() const { return {}; }
  void set_host_words(const int64_t*, int) {}
  const decodesli::Config& config() const { return cfg_; }
  const decodesli::Layout& result_layout() const { return lay_; }
  uint32_t tpot_slo_us() const { return slo_us_; }

 private:
  // row `which` of the state: [0, W) the horizon's windows, W the rolling row, W + 1 this step's
  uint32_t* hist(size_t which) const { return hist_ + which * (size_t)cfg_.group_cap * decodesli::kK; }
  uint32_t* cells(size_t which) const { return cells_ + which * (size_t)cfg_.group_cap * decodesli::kCells; }
  unsigned long long* sums(size_t which) const { return sum_ + which * (size_t)cfg_.group_cap; }

  decodesli::Config cfg_;
  decodesli::Layout lay_;
  uint32_t slo_us_ = 0;
  StepLane lane_;
  uint32_t* hist_ = nullptr;  // the lane's, like the two below
  uint32_t* cells_ = nullptr;
  unsigned long long* sum_ = nullptr;
};

}  // namespace mislo
