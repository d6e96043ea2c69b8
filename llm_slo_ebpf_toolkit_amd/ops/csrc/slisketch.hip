// TTFT sketch (slisketch.h): the kernels and the host class.
#include "slisketch.h"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace mislo {
namespace slisketch {

namespace {

constexpr int kNT = 256;
constexpr int kWave = 64;
constexpr int kRowsPerBlock = kNT / kWave;
constexpr int kRowLanes = kRowStride / kPerLane;  // lanes that own buckets

static_assert(kRowLanes * kPerLane == kRowStride && kRowLanes <= kWave && kRowStride >= kK && kRowStride % 4 == 0,
              "a row is kPerLane consecutive buckets per lane of one wave");

// One thread per record: the records k_decode_spans counts (no kSpanNoSli, a group below
// n_groups) with a TTFT >= 0 (NaN and negatives fail the compare) enter the window's histogram
// row, the `le` counts and the sum. Same-address adds of a wave are folded by the compiler.
__global__ __launch_bounds__(kNT) void k_sketch_observe(const Span* __restrict__ sp, int n, int n_groups,
                                                        uint32_t* __restrict__ cur, uint32_t* __restrict__ le,
                                                        unsigned long long* __restrict__ sum,
                                                        uint32_t* __restrict__ stats) {
  __shared__ uint32_t s_stats[kStats];
  if (threadIdx.x < kStats) s_stats[threadIdx.x] = 0;
  __syncthreads();
  for (int i = blockIdx.x * kNT + threadIdx.x; i < n; i += gridDim.x * kNT) {
    if (sp[i].flags & kSpanNoSli) continue;
    const uint32_t g = sp[i].group_id;
    if (g >= (uint32_t)n_groups) {
      atomicAdd(&s_stats[kOutOfGroup], 1u);
      continue;
    }
    const float v = sp[i].ttft_ms;
    if (!(v >= 0.f)) {
      atomicAdd(&s_stats[kInvalid], 1u);
      continue;
    }
    const uint32_t b = bucket_of_bits(__float_as_uint(v));  // <= kK - 1 < kRowStride
    atomicAdd(&cur[(size_t)g * kRowStride + b], 1u);
    atomicAdd(&le[(size_t)g * kLe + le_slot(v)], 1u);
    atomicAdd(&sum[g], milli_units(fminf(v, kMaxMs)));
    atomicAdd(&s_stats[kObserved], 1u);
    if (b == 0u) atomicAdd(&s_stats[kUnderflow], 1u);
    if (b == (uint32_t)kK - 1u) atomicAdd(&s_stats[kOverflow], 1u);
  }
  __syncthreads();
  if (threadIdx.x < kStats && s_stats[threadIdx.x]) atomicAdd(&stats[threadIdx.x], s_stats[threadIdx.x]);
}

// inclusive scan across the wave's lanes
__device__ __forceinline__ uint32_t wave_scan(uint32_t x, int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint32_t t = __shfl_up(x, d, kWave);
    if (lane >= d) x += t;
  }
  return x;
}

// The four quantile buckets of one row: `h` this lane's buckets, `incl` the inclusive scan of the
// lanes' totals, `n` the row's total. The lane whose buckets hold rank r writes the first bucket
// whose cumulative count reaches it.
__device__ __forceinline__ void pick_ranks(const uint32_t (&h)[kPerLane], uint32_t incl, uint32_t mine, uint32_t n,
                                           int lane, uint32_t* __restrict__ out) {
  const uint32_t excl = incl - mine;
#pragma unroll
  for (int q = 0; q < kQuantiles; ++q) {
    if (n == 0u) {
      if (lane == 0) out[q] = kEmpty;
      continue;
    }
    const uint64_t r = rank_of(quantile_permille(q), n);
    if ((uint64_t)excl < r && r <= (uint64_t)incl) {
      uint64_t cum = excl;
      int j = 0;
      for (; j < kPerLane - 1; ++j) {
        cum += h[j];
        if (cum >= r) break;
      }
      out[q] = (uint32_t)(lane * kPerLane + j);
    }
  }
}

// One wave per service row, every row of group_cap: the window of W steps ago leaves the rolling
// row, this one enters and takes its place in the horizon, the step's row is cleared; then the
// ranks of the window's and the rolling row. Lane l owns buckets [7 l, 7 l + 7).
__global__ __launch_bounds__(kNT) void k_sketch_roll(uint32_t* __restrict__ cur, uint32_t* __restrict__ slot,
                                                     uint32_t* __restrict__ roll,
                                                     unsigned long long* __restrict__ sum,
                                                     uint32_t* __restrict__ block, Layout lay, int group_cap) {
  const int lane = threadIdx.x & (kWave - 1);
  const int g = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (g >= group_cap) return;  // the whole wave
  uint32_t c[kPerLane], r[kPerLane];
  uint32_t tc = 0, tr = 0;
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) c[j] = r[j] = 0u;
  if (lane < kRowLanes) {
    const size_t at = (size_t)g * kRowStride + (size_t)lane * kPerLane;
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
      c[j] = cur[at + j];
      r[j] = roll[at + j] + c[j] - slot[at + j];
      roll[at + j] = r[j];
      slot[at + j] = c[j];
      cur[at + j] = 0u;
      tc += c[j];
      tr += r[j];
    }
  }
  const uint32_t ic = wave_scan(tc, lane), ir = wave_scan(tr, lane);
  const uint32_t n = __shfl(ic, kWave - 1, kWave), n_roll = __shfl(ir, kWave - 1, kWave);
  pick_ranks(c, ic, tc, n, lane, block + lay.q_win + (size_t)g * kQuantiles);
  pick_ranks(r, ir, tr, n_roll, lane, block + lay.q_roll + (size_t)g * kQuantiles);
  if (lane == 0) {
    const unsigned long long s = sum[g];
    sum[g] = 0ull;
    block[lay.n + g] = n;
    block[lay.n_roll + g] = n_roll;
    block[lay.sum + 2 * (size_t)g] = (uint32_t)s;
    block[lay.sum + 2 * (size_t)g + 1] = (uint32_t)(s >> 32);
  }
}

}  // namespace

void launch_observe(const Span* sp, int n, int n_groups, uint32_t* cur, uint32_t* le, unsigned long long* sum,
                    uint32_t* stats, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_sketch_observe, dim3(grid_for(n, kNT, 1024)), dim3(kNT), 0, st, sp, n, n_groups, cur, le, sum,
                     stats);
}

void launch_roll(uint32_t* cur, uint32_t* slot, uint32_t* roll, unsigned long long* sum, uint32_t* block, Layout lay,
                 int group_cap, hipStream_t st) {
  hipLaunchKernelGGL(k_sketch_roll, dim3(grid_for(group_cap, kRowsPerBlock, 1 << 20)), dim3(kNT), 0, st, cur, slot,
                     roll, sum, block, lay, group_cap);
}

}  // namespace slisketch

using namespace slisketch;

SliSketch::SliSketch(const Config& cfg)
    : cfg_(cfg),
      lay_(layout(cfg.group_cap)),
      lane_("ttft sketch", checked(cfg).device, cfg.n_buffers, cfg.span_cap, lay_.words, 0) {
  lane_.identify(slisketch::fingerprint(cfg));
  row_words_ = (size_t)cfg.group_cap * kRowStride;
  hist_ = lane_.zeroed<uint32_t>(device_bytes(cfg) / 4);
  sum_ = lane_.zeroed<unsigned long long>((size_t)cfg.group_cap);
  lane_.ready();
}

int64_t SliSketch::step(const std::vector<Range>& spans, int n_groups) {
  check_step(n_groups, cfg_.group_cap);
  const size_t n = plan_ranges(spans, cfg_.span_cap);
  const auto [idx, s] = lane_.begin(spans);
  const hipStream_t st = lane_.stream();
  uint32_t* const blk = lane_.block();
  const size_t W = (size_t)cfg_.windows;
  uint32_t* cur = rows(W + 1);
  launch_observe(lane_.spans(), (int)n, n_groups, cur, blk + lay_.le, sum_, blk + lay_.stats, st);
  launch_roll(cur, rows((size_t)(idx % (int64_t)W)), rows(W), sum_, blk, lay_, cfg_.group_cap, st);
  lane_.publish(s, 64);
  return idx;
}

std::pair<float, float> SliSketch::step_ms(int64_t i) {
  return {lane_.ms(i, StepLane::kBegin, StepLane::kEnd), lane_.ms(i, StepLane::kCopied, StepLane::kEnd)};
}

std::vector<uint32_t> SliSketch::read_rows(const uint32_t* dev) {
  std::vector<uint32_t> out((size_t)cfg_.group_cap * kK, 0u);
  if (!dev) return out;
  sync();
  std::vector<uint32_t> raw(row_words_);
  HIPCHECK(hipMemcpy(raw.data(), dev, row_words_ * 4, hipMemcpyDeviceToHost));
  for (size_t g = 0; g < (size_t)cfg_.group_cap; ++g)
    std::copy_n(raw.data() + g * kRowStride, kK, out.data() + g * kK);
  return out;
}

std::vector<uint32_t> SliSketch::rolling() { return read_rows(rows((size_t)cfg_.windows)); }

std::vector<uint32_t> SliSketch::window_hist() {
  const int64_t n = lane_.steps();
  return read_rows(n ? rows((size_t)((n - 1) % (int64_t)cfg_.windows)) : nullptr);
}

}  // namespace mislo
