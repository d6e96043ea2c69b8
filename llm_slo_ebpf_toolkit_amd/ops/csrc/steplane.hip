// Step lane (steplane.h): the publish kernel, the three checkpoint kernels and the host class.
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

using u64 = unsigned long long;
constexpr int kWaveLanes = 64;

// a thread's share of the digest into *digest: the wave's sum by shuffles, the workgroup's waves through
// LDS, one atomic add a workgroup (the sum is mod 2^64, so the order does not matter)
__device__ __forceinline__ void fold_digest(u64 sum, u64* digest) {
  __shared__ u64 part[kNT / kWaveLanes];
  for (int d = kWaveLanes / 2; d > 0; d >>= 1) sum += __shfl_xor(sum, d, kWaveLanes);
  if ((threadIdx.x & (kWaveLanes - 1)) == 0) part[threadIdx.x / kWaveLanes] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 all = 0;
    for (int w = 0; w < kNT / kWaveLanes; ++w) all += part[w];
    atomicAdd(digest, all);
  }
}

// The three checkpoint kernels walk the lane's own segment table (n_seg entries, built by ready()): array s
// is table[s].n16 chunks at table[s].ptr, and its copy lies at chunk table[s].off16 of the staging image.
// Nothing else gives them an address or a length.

// The payload's digest (lane::chunk_digest over every chunk the table names) into *digest. kGather: the
// chunks are read from the arrays and stored into the staging image on the way; otherwise they are read from
// the staging image.
template <bool kGather>
__device__ __forceinline__ void digest_payload(const StepLane::Segment* __restrict__ table, int n_seg, uint4* __restrict__ staging,
                                               u64* __restrict__ digest) {
  const size_t t0 = blockIdx.x * (size_t)kNT + threadIdx.x, stride = (size_t)gridDim.x * kNT;
  u64 sum = 0;
  for (int s = 0; s < n_seg; ++s) {
    const StepLane::Segment seg = table[s];
    for (size_t j = t0; j < seg.n16; j += stride) {
      const uint4 v = kGather ? seg.ptr[j] : staging[seg.off16 + j];
      if (kGather) staging[seg.off16 + j] = v;
      sum += lane::chunk_digest((u64)v.x | ((u64)v.y << 32), (u64)v.z | ((u64)v.w << 32), seg.off16 + j);
    }
  }
  fold_digest(sum, digest);
}

// every array into the staging image, and the payload's digest on the way
__global__ __launch_bounds__(kNT) void k_lane_snapshot(const StepLane::Segment* __restrict__ table, int n_seg,
                                                       uint4* __restrict__ staging, u64* __restrict__ digest) {
  digest_payload<true>(table, n_seg, staging, digest);
}

// the digest of a staged payload (restore: before anything is scattered)
__global__ __launch_bounds__(kNT) void k_lane_digest(const StepLane::Segment* __restrict__ table, int n_seg,
                                                     uint4* __restrict__ staging, u64* __restrict__ digest) {
  digest_payload<false>(table, n_seg, staging, digest);
}

// the staged payload into the arrays
__global__ __launch_bounds__(kNT) void k_lane_restore(const StepLane::Segment* __restrict__ table, int n_seg,
                                                      const uint4* __restrict__ staging) {
  const size_t t0 = blockIdx.x * (size_t)kNT + threadIdx.x, stride = (size_t)gridDim.x * kNT;
  for (int s = 0; s < n_seg; ++s) {
    const StepLane::Segment seg = table[s];
    for (size_t j = t0; j < seg.n16; j += stride) seg.ptr[j] = staging[seg.off16 + j];
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
  // the checkpoint's segment table: every array taken so far, which is every array but the result block
  std::vector<Segment> table;
  std::vector<size_t> seg_bytes;
  size_t off16 = 0;
  for (size_t a = 0; a < arrays_.size(); ++a) {
    table.push_back(Segment{static_cast<uint4*>(arrays_[a]), (u64)off16, (u64)(array_bytes_[a] / lane::kChunk)});
    seg_bytes.push_back(array_bytes_[a]);
    off16 += array_bytes_[a] / lane::kChunk;
  }
  mine_ = lane::make_header(fp_, seg_bytes);
  mine_.n_host = (uint32_t)n_host_;
  n_segments_ = (int)table.size();
  payload_bytes_ = off16 * lane::kChunk;
  block_ = zeroed<uint32_t>(block_words_);
  if (n_segments_) {
    HIPCHECK(hipMalloc(reinterpret_cast<void**>(&table_), table.size() * sizeof(Segment)));
    HIPCHECK(hipMemcpy(table_, table.data(), table.size() * sizeof(Segment), hipMemcpyHostToDevice));
  }
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
  if (copy_st_) (void)hipStreamSynchronize(copy_st_);
  for (void* p : arrays_) (void)hipFree(p);
  (void)hipFree(table_);
  (void)hipFree(staging_);
  if (image_) (void)hipHostFree(image_);
  for (hipEvent_t e : {snap_begin_, snap_gathered_, snap_done_})
    if (e) (void)hipEventDestroy(e);
  if (copy_st_) (void)hipStreamDestroy(copy_st_);
  (void)hipFree(spans_);
  for (uint32_t* h : host_) (void)hipHostFree(h);
  for (hipEvent_t e : events_) (void)hipEventDestroy(e);
  if (st_) (void)hipStreamDestroy(st_);
}

void* StepLane::zeroed_bytes(size_t bytes) {
  // whole 16-byte chunks, the tail zero for good: the checkpoint moves and digests chunks
  bytes = lane::round16(bytes);
  arrays_.reserve(arrays_.size() + 1);  // so that what hipMalloc returns cannot be lost to a failed push_back
  array_bytes_.reserve(array_bytes_.size() + 1);
  void* p = nullptr;
  HIPCHECK(hipMalloc(&p, bytes));
  arrays_.push_back(p);
  array_bytes_.push_back(bytes);
  HIPCHECK(hipMemsetAsync(p, 0, bytes, st_));
  return p;
}

StepLane::Step StepLane::begin(const std::vector<Range>& ranges) {
  if (!block_) throw std::logic_error("step lane: begin() before ready()");
  HIPCHECK(hipSetDevice(device_));
  stepped_ = true;
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

// ---- checkpoint ---------------------------------------------------------------------------------
void StepLane::set_checkpoint_blocks(int max_blocks) {
  if (max_blocks < 1 || max_blocks > 65535) throw std::invalid_argument("step lane: checkpoint blocks must be in [1, 65535]");
  ckpt_blocks_ = max_blocks;
}

void StepLane::ensure_staging() {
  if (!block_) throw std::logic_error("step lane: checkpoint before ready()");
  if (fp_.kind == lane::kNoKind) throw std::logic_error("step lane: checkpoint of a lane nobody identified");
  if (staging_) return;
  HIPCHECK(hipSetDevice(device_));
  HIPCHECK(hipStreamCreateWithFlags(&copy_st_, hipStreamNonBlocking));
  HIPCHECK(hipEventCreate(&snap_begin_));
  HIPCHECK(hipEventCreate(&snap_gathered_));
  HIPCHECK(hipEventCreateWithFlags(&snap_done_, hipEventDisableTiming));
  void* h = nullptr;
  HIPCHECK(hipHostMalloc(&h, sizeof(lane::ImageHeader) + payload_bytes_ + lane::kChunk, hipHostMallocDefault));
  image_ = static_cast<uint8_t*>(h);
  HIPCHECK(hipMalloc(reinterpret_cast<void**>(&staging_), payload_bytes_ + lane::kChunk));
}

int64_t StepLane::snapshot(const std::vector<int64_t>& host_words) {
  if (pending_) throw std::logic_error(std::string(lane::kind_name(fp_.kind)) + ": a snapshot is pending, read it first");
  if (host_words.size() != (size_t)n_host_) throw std::logic_error("step lane: not the host words the tracker announced");
  ensure_staging();
  HIPCHECK(hipSetDevice(device_));
  lane::ImageHeader h = mine_;
  h.step = slots_.next();
  h.n_host = (uint32_t)host_words.size();
  std::copy(host_words.begin(), host_words.end(), h.host);
  std::memcpy(image_, &h, sizeof(h));
  u64* const digest = reinterpret_cast<u64*>(staging_ + payload_bytes_);
  HIPCHECK(hipMemsetAsync(digest, 0, lane::kChunk, st_));
  HIPCHECK(hipEventRecord(snap_begin_, st_));
  hipLaunchKernelGGL(k_lane_snapshot, dim3(grid_for((int64_t)(payload_bytes_ / lane::kChunk), kNT, ckpt_blocks_)), dim3(kNT), 0,
                     st_, table_, n_segments_, reinterpret_cast<uint4*>(staging_), digest);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipEventRecord(snap_gathered_, st_));
  // the transfer runs beside the steps that follow: they write the arrays, never the staging image
  HIPCHECK(hipStreamWaitEvent(copy_st_, snap_gathered_, 0));
  HIPCHECK(hipMemcpyAsync(image_ + sizeof(lane::ImageHeader), staging_, payload_bytes_ + lane::kChunk, hipMemcpyDeviceToHost,
                          copy_st_));
  HIPCHECK(hipEventRecord(snap_done_, copy_st_));
  pending_ = true;
  return ++tickets_;
}

bool StepLane::snapshot_ready(int64_t ticket) {
  if (!pending_ || ticket != tickets_) throw std::out_of_range(std::string(lane::kind_name(fp_.kind)) + ": no such snapshot is pending");
  const hipError_t e = hipEventQuery(snap_done_);
  if (e == hipSuccess) return true;
  if (e != hipErrorNotReady) HIPCHECK(e);
  return false;
}

const uint8_t* StepLane::snapshot_image(int64_t ticket) {
  if (ticket != tickets_ || ticket < 1) throw std::out_of_range(std::string(lane::kind_name(fp_.kind)) + ": no such snapshot");
  if (pending_) {
    HIPCHECK(hipEventSynchronize(snap_done_));
    // the device's digest, behind the payload, into the header
    std::memcpy(image_ + offsetof(lane::ImageHeader, digest), image_ + sizeof(lane::ImageHeader) + payload_bytes_, sizeof(uint64_t));
    pending_ = false;
  }
  return image_;
}

float StepLane::snapshot_kernel_ms() {
  if (tickets_ < 1 || pending_) throw std::logic_error("step lane: no snapshot was read");
  float ms = 0.f;
  HIPCHECK(hipEventElapsedTime(&ms, snap_begin_, snap_gathered_));
  return ms;
}

lane::ImageHeader StepLane::restore(const void* image, size_t bytes,
                                    const std::function<void(const lane::ImageHeader&)>& accept) {
  const std::string who = std::string(lane::kind_name(fp_.kind)) + " image: ";
  if (stepped_) throw std::logic_error(std::string(lane::kind_name(fp_.kind)) + ": restore is only possible before the first step");
  if (pending_) throw std::logic_error(std::string(lane::kind_name(fp_.kind)) + ": a snapshot is pending, read it first");
  if (!block_) throw std::logic_error("step lane: checkpoint before ready()");
  const lane::ImageHeader h = lane::check_image(image, bytes, fp_, mine_);  // no HIP call up to here
  ensure_staging();
  HIPCHECK(hipSetDevice(device_));
  u64* const digest = reinterpret_cast<u64*>(staging_ + payload_bytes_);
  const dim3 grid(grid_for((int64_t)(payload_bytes_ / lane::kChunk), kNT, ckpt_blocks_));
  HIPCHECK(hipMemcpyAsync(staging_, static_cast<const uint8_t*>(image) + sizeof(lane::ImageHeader), payload_bytes_,
                          hipMemcpyHostToDevice, st_));
  HIPCHECK(hipMemsetAsync(digest, 0, lane::kChunk, st_));
  hipLaunchKernelGGL(k_lane_digest, grid, dim3(kNT), 0, st_, table_, n_segments_, reinterpret_cast<uint4*>(staging_), digest);
  HIPCHECK(hipGetLastError());
  uint64_t got = 0;
  HIPCHECK(hipMemcpyAsync(&got, digest, sizeof(got), hipMemcpyDeviceToHost, st_));
  HIPCHECK(hipStreamSynchronize(st_));
  if (got != h.digest) throw std::invalid_argument(who + "the payload's digest differs from the header's (damaged)");
  if (accept) accept(h);
  hipLaunchKernelGGL(k_lane_restore, grid, dim3(kNT), 0, st_, table_, n_segments_, reinterpret_cast<const uint4*>(staging_));
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(st_));
  slots_.resume(h.step);
  return h;
}

}  // namespace mislo
