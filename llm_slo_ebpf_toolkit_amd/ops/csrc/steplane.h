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
//
// Checkpoint (steplane_host.h namespace lane, docs/TRACKER_CHECKPOINT.md). Everything a tracker keeps
// between steps on the device is an array it took with zeroed(), so the lane can save and restore it
// without knowing the tracker. zeroed_bytes records (pointer, bytes rounded up to 16); ready() puts one
// (pointer, image offset, chunks) entry per array but the result block into a segment table in device
// memory, and the checkpoint kernels index by that table alone -- never by a size or offset read from an
// image.
//   snapshot  on the lane's stream, after the last step: k_lane_snapshot gathers the arrays into one
//             device staging image by 16-byte loads and stores and folds the payload's digest in the same
//             pass; a copy stream of the lane's waits for that kernel's event and brings staging and digest
//             to a pinned host image in one hipMemcpyAsync. A step issued right after neither waits for
//             the transfer nor shows in the image. One snapshot may be pending.
//   restore   before the first step only: the host checks the header (no HIP call before that), uploads
//             the payload to staging, k_lane_digest digests it there, the host compares, and only then
//             k_lane_restore scatters staging into the arrays. A refused restore has changed nothing.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <functional>
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
  // one array of the checkpoint image: where it lies, where its copy lies in the payload, its 16-byte chunks
  struct Segment {
    uint4* ptr;
    unsigned long long off16, n16;
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

  // ---- checkpoint ----
  // who the image belongs to, and how many host integers the tracker keeps between steps; before ready()
  void identify(const lane::Fingerprint& fp, int n_host = 0) { fp_ = fp, n_host_ = n_host; }
  // Enqueue a snapshot behind the steps issued so far; `host_words` are the tracker's own integers as they
  // stand after those steps. Returns a ticket. Refused while an earlier snapshot is unread.
  int64_t snapshot(const std::vector<int64_t>& host_words = {});
  bool snapshot_ready(int64_t ticket);
  // the image (header and payload), `image_bytes()` long, valid until the next snapshot; waits for it
  const uint8_t* snapshot_image(int64_t ticket);
  size_t image_bytes() const { return sizeof(lane::ImageHeader) + payload_bytes_; }
  // device time of the last snapshot's gather and digest kernel, ms; after snapshot_image()
  float snapshot_kernel_ms();
  // Take an image: only before the first step. Throws std::invalid_argument, with nothing changed, when
  // the image is not this lane's, its digest fails or `accept` (the tracker's check of its host words,
  // called before anything is scattered) throws; returns the header (step index, host words).
  lane::ImageHeader restore(const void* image, size_t bytes, const std::function<void(const lane::ImageHeader&)>& accept);
  // blocks of the checkpoint kernels, at most (tests: 1 forces the grid-stride path)
  void set_checkpoint_blocks(int max_blocks);
  const lane::Fingerprint& fingerprint() const { return fp_; }

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
  void ensure_staging();

  int device_;
  int per_slot_;  // events per slot
  size_t block_words_;
  SlotRing slots_;
  hipStream_t st_ = nullptr;
  Span* spans_ = nullptr;
  uint32_t* block_ = nullptr;
  std::vector<void*> arrays_;  // zeroed(), in allocation order (the result block is the last)
  std::vector<size_t> array_bytes_;  // of each, rounded up to 16
  // checkpoint
  lane::Fingerprint fp_;
  int n_host_ = 0;
  lane::ImageHeader mine_;       // what this lane's images carry (ready())
  Segment* table_ = nullptr;     // device: one entry per array but the result block
  int n_segments_ = 0;
  size_t payload_bytes_ = 0;
  uint8_t* staging_ = nullptr;   // device: payload, then the digest's 16 bytes (first snapshot or restore)
  uint8_t* image_ = nullptr;     // pinned host: header, payload, digest
  hipStream_t copy_st_ = nullptr;
  hipEvent_t snap_begin_ = nullptr, snap_gathered_ = nullptr, snap_done_ = nullptr;
  int64_t tickets_ = 0;          // snapshots taken
  bool pending_ = false, stepped_ = false;
  int ckpt_blocks_ = 1024;
  std::vector<uint32_t*> host_;
  std::vector<hipEvent_t> events_;  // [slot][per_slot_]
};

}  // namespace mislo
