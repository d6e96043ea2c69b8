// Step lane (steplane.h): the publish kernel and the host class.
#include "steplane.h"

namespace mislo {

namespace {

constexpr int kNT = 256;

// the step's result block into its pinned host block; the block cleared from clear_from on for the
// next step (what lies before it the tracker rewrites whole every step)
__global__ __launch_bounds__(kNT) void k_lane_publish(uint4* __restrict__ block, uint4* __restrict__ host, size_t n16,
                                                      size_t clear_from) {
  for (size_t i = blockIdx.x * (size_t)kNT + threadIdx.x; i < n16; i += (size_t)gridDim.x * kNT) {
    host[i] = block[i];
    if (i >= clear_from) block[i] = make_uint4(0u, 0u, 0u, 0u);
  }
}

}  // namespace

StepLane::StepLane(const char* who, int device, int n_buffers, int span_cap, size_t block_words, int n_marks)
    : device_(device), per_slot_(3 + n_marks), block_words_(block_words), slots_(n_buffers, who) {
  try {
    HIPCHECK(hipSetDevice(device));
    HIPCHECK(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
    HIPCHECK(hipMalloc(reinterpret_cast<void**>(&spans_), (size_t)span_cap * sizeof(Span)));
  } catch (...) {
    release();
    throw;
  }
}

void StepLane::ready() {
  block_ = zeroed<uint32_t>(block_words_);
  for (int i = 0; i < slots_.size(); ++i) {
    void* h = nullptr;
    HIPCHECK(hipHostMalloc(&h, block_words_ * 4, hipHostMallocCoherent | hipHostMallocMapped));
    host_.push_back(static_cast<uint32_t*>(h));
    std::fill_n(host_.back(), block_words_, 0u);
    for (int e = 0; e < per_slot_; ++e) {
      hipEvent_t ev;
      HIPCHECK(hipEventCreate(&ev));
      events_.push_back(ev);
    }
  }
  sync();
}

StepLane::~StepLane() { release(); }

void StepLane::release() {
  (void)hipSetDevice(device_);
  if (st_) (void)hipStreamSynchronize(st_);
  for (void* p : arrays_) (void)hipFree(p);
  (void)hipFree(spans_);
  for (uint32_t* h : host_) (void)hipHostFree(h);
  for (hipEvent_t e : events_) (void)hipEventDestroy(e);
  if (st_) (void)hipStreamDestroy(st_);
}

void* StepLane::zeroed_bytes(size_t bytes) {
  arrays_.reserve(arrays_.size() + 1);  // so that what hipMalloc returns cannot be lost to a failed push_back
  void* p = nullptr;
  HIPCHECK(hipMalloc(&p, bytes));
  arrays_.push_back(p);
  HIPCHECK(hipMemsetAsync(p, 0, bytes, st_));
  return p;
}

StepLane::Step StepLane::begin(const std::vector<Range>& ranges) {
  if (!block_) throw std::logic_error("step lane: begin() before ready()");
  HIPCHECK(hipSetDevice(device_));
  const int64_t idx = slots_.next();
  const int s = slots_.begin();
  HIPCHECK(hipEventRecord(event(s, kBegin), st_));
  size_t off = 0;
  for (const Range& r : ranges) {
    if (!r.second) continue;
    HIPCHECK(hipMemcpyAsync(reinterpret_cast<uint8_t*>(spans_) + off, reinterpret_cast<const void*>(r.first), r.second,
                            hipMemcpyHostToDevice, st_));
    off += r.second;
  }
  HIPCHECK(hipEventRecord(event(s, kCopied), st_));
  return {idx, s};
}

void StepLane::publish(int slot, int max_blocks, size_t clear_from16) {
  const size_t n16 = block_words_ / 4;
  hipLaunchKernelGGL(k_lane_publish, dim3(grid_for((int64_t)n16, kNT, max_blocks)), dim3(kNT), 0, st_,
                     reinterpret_cast<uint4*>(block_), reinterpret_cast<uint4*>(host(slot)), n16, clear_from16);
  finish(slot);
}

void StepLane::finish(int slot) {
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipEventRecord(event(slot, kEnd), st_));
  // the ranges belong to the caller again once this returns
  HIPCHECK(hipEventSynchronize(event(slot, kCopied)));
}

bool StepLane::query(int64_t i) {
  const hipError_t e = hipEventQuery(event(slots_.slot_of(i), kEnd));
  if (e == hipSuccess) return true;
  if (e != hipErrorNotReady) HIPCHECK(e);
  return false;
}

const uint32_t* StepLane::results(int64_t i) {
  const int s = slots_.slot_of(i);
  HIPCHECK(hipEventSynchronize(event(s, kEnd)));
  return host(s);
}

float StepLane::ms(int64_t i, Event from, Event to) {
  const int s = slots_.slot_of(i);
  HIPCHECK(hipEventSynchronize(event(s, kEnd)));
  float ms = 0.f;
  HIPCHECK(hipEventElapsedTime(&ms, event(s, from), event(s, to)));
  return ms;
}

void StepLane::sync() {
  HIPCHECK(hipSetDevice(device_));
  HIPCHECK(hipStreamSynchronize(st_));
}

}  // namespace mislo
