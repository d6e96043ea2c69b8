// Step lane: what a side tracker's step needs that is not the tracker's own.
//
// Every side tracker (openreq.h, slisketch.h, exemplars.h, podrank.h, onset.h, decodesli.h, drift.h,
// errsli.h, loadsli.h, satcurve.h, retrsli.h) runs one step per window on a stream of its own: copy the
// window's span ranges, run its kernels, publish a result block. The lane owns that frame -- the device,
// the non-blocking stream, the span buffer, the device result block, the last n_buffers result blocks in
// pinned host memory (coherent and mapped) with their slots (steplane_host.h SlotRing) and per slot the
// events begin / copied / end plus the marks the tracker asks for -- and every further zeroed device
// array the tracker takes through zeroed(). All of it is released by the lane's destructor, also when
// the tracker's constructor throws half way.
//
// A tracker's constructor builds the lane, takes its arrays with zeroed() and ends with ready(), which
// allocates the result block, its pinned copies and the events and waits for the memsets. The result
// block comes after the tracker's arrays on purpose: the observe kernels' atomics are sensitive to where
// the arrays lie (with the block in front of them the onset and load observe kernels measured 2-4 %
// slower or faster from one process to the next; behind them, as it always was, they do not move:
// profiles/step_lane/README.md).
//
// A step, in stream order:
//   begin    hipSetDevice, take the slot, record `begin`, copy the ranges (empty ones skipped) into the
//            span buffer, record `copied`,
//   ...      the tracker's kernels, with mark() where it times one,
//   publish  k_lane_publish: the result block into the slot's pinned host block by vector stores, the
//            block cleared from `clear_from16` on for the next step; then finish(),
//   finish   hipGetLastError, record `end`, wait for `copied`: the ranges belong to the caller again.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "mislo_common.h"
#include "steplane_host.h"

#define HIPCHECK(x)                                                                                  \
  do {                                                                                               \
    hipError_t _e = (x);                                                                             \
    if (_e != hipSuccess) throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(_e) + \
                                                   " at " #x);                                       \
  } while (0)

namespace mislo {

// blocks of `per_block` items for n items, at least one and at most max_blocks
inline int grid_for(int64_t n, int per_block, int max_blocks) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(max_blocks, (n + per_block - 1) / per_block));
}

class StepLane {
 public:
  // a slot's events: the lane records the first three, mark() the tracker's own (n_marks of them)
  enum Event { kBegin = 0, kCopied = 1, kEnd = 2, kObserved = 3, kAdvanced = 4 };
  struct Step {
    int64_t index;
    int slot;
  };

  // block_words: uint32 words of the result block, whole 16-byte stores
  StepLane(const char* who, int device, int n_buffers, int span_cap, size_t block_words, int n_marks);
  ~StepLane();
  StepLane(const StepLane&) = delete;
  StepLane& operator=(const StepLane&) = delete;

  // `count` zeroed T on the device (the memset is on the lane's stream: sync() before the host relies
  // on it); freed with the lane
  template <class T>
  T* zeroed(size_t count) {
    return static_cast<T*>(zeroed_bytes(count * sizeof(T)));
  }

  // the result block, the pinned host blocks and the events, after the tracker's zeroed() arrays; waits
  // for every memset. Steps from here on
  void ready();
  Step begin(const std::vector<Range>& ranges);
  void mark(int slot, Event e) { HIPCHECK(hipEventRecord(event(slot, e), st_)); }
  void publish(int slot, int max_blocks, size_t clear_from16 = 0);
  void finish(int slot);

  bool query(int64_t i);
  // step i's pinned host block, valid until n_buffers later steps; waits for it
  const uint32_t* results(int64_t i);
  // device time from one event of step i to another, ms; waits for the step
  float ms(int64_t i, Event from, Event to);
  void sync();

  int64_t steps() const { return slots_.next(); }
  hipStream_t stream() const { return st_; }
  Span* spans() const { return spans_; }
  uint32_t* block() const { return block_; }
  uint32_t* host(int slot) const { return host_[(size_t)slot]; }

 private:
  void* zeroed_bytes(size_t bytes);
  hipEvent_t event(int slot, Event e) const {
    if ((int)e >= per_slot_) throw std::logic_error("step lane: an event the tracker did not ask for");
    return events_[(size_t)slot * (size_t)per_slot_ + (size_t)e];
  }
  void release();

  int device_;
  int per_slot_;  // events per slot
  size_t block_words_;
  SlotRing slots_;
  hipStream_t st_ = nullptr;
  Span* spans_ = nullptr;
  uint32_t* block_ = nullptr;
  std::vector<void*> arrays_;  // zeroed(), in allocation order (the result block is the last)
  std::vector<uint32_t*> host_;
  std::vector<hipEvent_t> events_;  // [slot][per_slot_]
};

}  // namespace mislo
