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
// Native, no PyTorch, its own stream, plain launches (no graphs). One step per window:
//   copy   the window's span ranges into the tracker's own device buffer (complete when step()
//          returns: the rings' release contract stays the engine's),
//   insert every start record: absent -> OPEN; OPEN / COUNTED -> dup_start; marker -> start_after_sli,
//   resolve every record the engine counts: OPEN -> removed; COUNTED -> removed + a correction
//          (dup); absent -> a RESOLVED marker (a start that arrives after its SLI is dropped),
//   sweep  the table: OPEN past its deadline -> counted (dl) and COUNTED; COUNTED past ttl and
//          markers past reorder -> removed; the survivors move into the cleared other table, so
//          no tombstone outlives a step and probe chains stay whole within one,
//   publish the counters into the step's pinned host block (vector stores) and clear them.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "mislo_common.h"
#include "openreq_host.h"

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
void launch_publish(uint32_t* counters, uint32_t* host, size_t words, hipStream_t st);

}  // namespace openreq

class OpenRequests {
 public:
  explicit OpenRequests(const openreq::Config& cfg);
  ~OpenRequests();
  OpenRequests(const OpenRequests&) = delete;
  OpenRequests& operator=(const OpenRequests&) = delete;

  // One window; returns the step's index. The ranges are read before it returns.
  int64_t step(const std::vector<openreq::Range>& spans, int64_t cut_ns, int64_t prev_cut_ns, int n_groups);
  bool query(int64_t i);
  void wait(int64_t i);
  // the step's result block (openreq::layout), valid until n_buffers later steps; waits for it
  const uint32_t* results(int64_t i);
  // device time of the step: (copy + kernels, kernels alone), ms
  std::pair<float, float> step_ms(int64_t i);
  // live entries sorted by trace hash (synchronous; tests)
  void entries(std::vector<uint64_t>& key, std::vector<int64_t>& t, std::vector<uint32_t>& grp,
               std::vector<uint32_t>& state);
  void sync();
  const openreq::Config& config() const { return cfg_; }
  const openreq::Layout& result_layout() const { return lay_; }
  int64_t steps() const { return slots_.next(); }

 private:
  openreq::Config cfg_;
  openreq::Layout lay_;
  openreq::SlotRing slots_;
  hipStream_t st_ = nullptr;
  openreq::Table tb_[2] = {};
  int cur_ = 0;
  Span* spans_ = nullptr;
  uint32_t* counters_ = nullptr;
  std::vector<uint32_t*> host_;
  std::vector<hipEvent_t> ev_begin_, ev_copied_, ev_end_;
};

}  // namespace mislo
