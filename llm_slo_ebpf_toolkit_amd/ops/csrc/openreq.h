// Open-request tracker: the agent as the TTFT deadline clock.
//
// A service says "request started" once (a start record: a 64-byte Span with kSpanStart |
// kSpanNoSli, ttft NaN); the tracker keeps the open requests in a device hash table and, at every
// window cut, counts the requests whose start + SLO has passed with no SLI record yet -- once --
// and un-counts them from the window their late record finally lands in. It produces per-group
// corrections to the window engine's sli / late counts (pipeline/window.py applies them on the
// host); the engine, its graphs and its streams are not touched. pipeline/openreq.py holds the
// same rules on the host (the oracle, and what the CPU engine uses).
//
// Native, no PyTorch, plain launches (no graphs) on a step lane of its own (steplane.h: the stream, the
// copy of the window's span ranges, the result slots, the publish). One step per window, between the
// lane's copy and its publish:
//   insert every start record: absent -> OPEN; OPEN / COUNTED -> dup_start; marker -> start_after_sli,
//   resolve every record the engine counts: OPEN -> removed; COUNTED -> removed + a correction
//          (dup); absent -> a RESOLVED marker (a start that arrives after its SLI is dropped),
//   sweep  the table: OPEN past its deadline -> counted (dl) and COUNTED; COUNTED past ttl and
//          markers past reorder -> removed; the survivors move into the cleared other table, so
//          no tombstone outlives a step and probe chains stay whole within one.
#pragma once

#include <hip/hip_runtime.h>

#include <stdexcept>
#include <vector>

#include "mislo_common.h"
#include "openreq_host.h"
#include "steplane.h"

namespace mislo {

constexpr uint32_t kSpanStart = 8u;  // Span::flags bit 3 (collector/records.py SPAN_START)

namespace openreq {

// structure of arrays: the sweep reads the keys of every slot, the rest of the live ones only
struct Table {
  unsigned long long* key;  // trace hash, 0 = empty
  int64_t* t;               // start time (OPEN, COUNTED) or the cut a marker was born at
  uint32_t* grp;
  uint32_t* state;
};

struct StepArgs {
  int64_t cut_ns, prev_cut_ns, slo_ns, ttl_ns, reorder_ns;
  float slo_ms;
  int n_groups;
  uint64_t mask;  // cap - 1
};

// openreq.hip launchers (plain pointers + stream)
void launch_insert(const Span* sp, int n, Table tb, StepArgs a, uint32_t* stats, hipStream_t st);
void launch_resolve(const Span* sp, int n, Table tb, StepArgs a, uint32_t* dup, uint32_t* stats, hipStream_t st);
void launch_sweep(Table cur, Table nxt, int64_t cap, StepArgs a, uint32_t* dl, uint32_t* stats, hipStream_t st);

}  // namespace openreq

class OpenRequests {
 public:
  explicit OpenRequests(const openreq::Config& cfg);

  // One window; returns the step's index. The ranges are read before it returns.
  int64_t step(const std::vector<openreq::Range>& spans, int64_t cut_ns, int64_t prev_cut_ns, int n_groups);
  bool query(int64_t i) { return lane_.query(i); }
  void wait(int64_t i) { lane_.results(i); }
  // the step's result block (openreq::layout), valid until n_buffers later steps; waits for it
  const uint32_t* results(int64_t i) { return lane_.results(i); }
  // device time of the step: (copy + kernels, kernels alone), ms
  std::pair<float, float> step_ms(int64_t i);
  // live entries sorted by trace hash (synchronous; tests)
  void entries(std::vector<uint64_t>& key, std::vector<int64_t>& t, std::vector<uint32_t>& grp,
               std::vector<uint32_t>& state);
  void sync() { lane_.sync(); }
  // checkpoint (steplane.h): the lane, and the host integer kept between steps: which table is current
  StepLane& lane() { return lane_; }
  std::vector<int64_t> host_words() const { return {cur_}; }
  void set_host_words(const int64_t* w, int n) {
    if (n != 1 || (w[0] != 0 && w[0] != 1)) throw std::invalid_argument("open-request image: host words");
    cur_ = (int)w[0];
  }
  const openreq::Config& config() const { return cfg_; }
  const openreq::Layout& result_layout() const { return lay_; }
  int64_t steps() const { return lane_.steps(); }

 private:
  openreq::Config cfg_;
  openreq::Layout lay_;
  StepLane lane_;
  openreq::Table tb_[2] = {};  // the lane's arrays
  int cur_ = 0;
};

}  // namespace mislo
