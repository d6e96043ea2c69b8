// Decode-phase SLI (decodesli.h): the kernels and the host class.
#include "decodesli.h"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace mislo {
namespace decodesli {

namespace {

constexpr int kNT = 256;
constexpr int kWave = 64;
constexpr int kRowsPerBlock = kNT / kWave;

static_assert(kLdsSlots == kNT, "observe flushes its LDS table one slot per thread");

using u64 = unsigned long long;

// `add` into the workgroup's table under `key`: claim-by-CAS, a bounded probe. False: no slot found.
__device__ __forceinline__ bool lds_add(u64* s_key, u64* s_val, u64 key, u64 add) {
  uint32_t s = onset::lds_hash(key);
  for (int probe = 0; probe < kLdsProbes; ++probe, s = (s + 1u) & (kLdsSlots - 1)) {
    u64 k = __hip_atomic_load(&s_key[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k == 0ull) {
      k = atomicCAS(&s_key[s], 0ull, key);
      if (k == 0ull) k = key;
    }
    if (k == key) {
      atomicAdd(&s_val[s], add);
      return true;
    }
  }
  return false;
}

// an aggregate of (service g, what) into the step's row; g < n_groups <= group_cap, what <= kSum
__device__ __forceinline__ void global_add(uint32_t g, uint32_t what, u64 add, uint32_t* __restrict__ hist,
                                           uint32_t* __restrict__ cells, u64* __restrict__ sum) {
  if (what < (uint32_t)kK)
    atomicAdd(&hist[(size_t)g * kK + what], (uint32_t)add);
  else if (what < kSum)
    atomicAdd(&cells[(size_t)g * kCells + (what - (uint32_t)kK)], (uint32_t)add);
  else
    atomicAdd(&sum[g], add);
}

// One thread per record, the checks in the rules' order: a start or first-token record is skipped;
// a record without a TPOT is no_decode; a group at or above n_groups out_of_group; a TTFT that is
// not >= 0 (NaN and negatives fail the compare) invalid; the rest is observed: one add each into its
// (service, bucket), its (service, table cell) and the service's sum of microseconds. With kLds the
// workgroup aggregates the three in an LDS table of kLdsSlots keyed (service, what) and sends each key
// to the step's row once; an add that finds no slot within kLdsProbes goes there itself.
template <bool kLds>
__global__ __launch_bounds__(kNT) void k_decode_observe(const Span* __restrict__ sp, int n, int n_groups, float slo,
                                                        uint32_t slo_us, uint32_t* __restrict__ hist,
                                                        uint32_t* __restrict__ cells, u64* __restrict__ sum,
                                                        uint32_t* __restrict__ stats) {
  __shared__ u64 s_key[kLds ? kLdsSlots : 1];
  __shared__ u64 s_val[kLds ? kLdsSlots : 1];
  __shared__ uint32_t s_stats[kStats];
  if (kLds) s_key[threadIdx.x] = 0ull, s_val[threadIdx.x] = 0ull;
  if (threadIdx.x < kStats) s_stats[threadIdx.x] = 0u;
  __syncthreads();
  for (size_t i = blockIdx.x * (size_t)kNT + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * kNT) {
    const uint32_t flags = sp[i].flags;
    if (flags & kSkipMask) continue;
    const uint32_t u = tpot_of(flags);
    if (u == 0u) {
      atomicAdd(&s_stats[kNoDecode], 1u);
      continue;
    }
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
    atomicAdd(&s_stats[kObserved], 1u);
    const uint32_t what[3] = {bucket_of(u), (uint32_t)kK + cell_of(v, slo, u, slo_us), kSum};
    const u64 add[3] = {1ull, 1ull, (u64)u};
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (!kLds || !lds_add(s_key, s_val, lds_key(g, what[j]), add[j])) global_add(g, what[j], add[j], hist, cells, sum);
  }
  __syncthreads();
  if (kLds) {
    const u64 key = s_key[threadIdx.x];
    if (key != 0ull) global_add(lds_group(key), lds_what(key), s_val[threadIdx.x], hist, cells, sum);
  }
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
    const uint64_t r = slisketch::rank_of(slisketch::quantile_permille(q), n);
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

// One state row of [group_cap] services: the histograms, the tables, the sums.
struct Rows {
  uint32_t* hist;
  uint32_t* cells;
  u64* sum;
};

// One wave per service row, every row of group_cap: the window of W steps ago (`slot`) leaves the
// rolling row, this one (`cur`) enters and takes its place in the horizon, the step's row is
// cleared; then the ranks of the window's and the rolling row. Lane l owns buckets [6 l, 6 l + 6);
// lanes 0-3 roll the table's cells, lane 4 the sum.
__global__ __launch_bounds__(kNT) void k_decode_roll(Rows cur, Rows slot, Rows roll, uint32_t* __restrict__ block,
                                                     Layout lay, int group_cap) {
  const int lane = threadIdx.x & (kWave - 1);
  const int g = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (g >= group_cap) return;  // the whole wave
  uint32_t c[kPerLane], r[kPerLane];
  uint32_t tc = 0, tr = 0;
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) c[j] = r[j] = 0u;
  if (lane < kRowLanes) {
    const size_t at = (size_t)g * kK + (size_t)lane * kPerLane;
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
      c[j] = cur.hist[at + j];
      r[j] = roll.hist[at + j] + c[j] - slot.hist[at + j];
      roll.hist[at + j] = r[j];
      slot.hist[at + j] = c[j];
      cur.hist[at + j] = 0u;
      tc += c[j];
      tr += r[j];
    }
  }
  const uint32_t ic = wave_scan(tc, lane), ir = wave_scan(tr, lane);
  const uint32_t n = __shfl(ic, kWave - 1, kWave), n_roll = __shfl(ir, kWave - 1, kWave);
  pick_ranks(c, ic, tc, n, lane, block + lay.q_win + (size_t)g * kQuantiles);
  pick_ranks(r, ir, tr, n_roll, lane, block + lay.q_roll + (size_t)g * kQuantiles);
  if (lane < kCells) {
    const size_t at = (size_t)g * kCells + lane;
    const uint32_t w = cur.cells[at], h = roll.cells[at] + w - slot.cells[at];
    roll.cells[at] = h;
    slot.cells[at] = w;
    cur.cells[at] = 0u;
    block[lay.cells + at] = w;
    block[lay.cells_roll + at] = h;
  } else if (lane == kCells) {
    const u64 w = cur.sum[g], h = roll.sum[g] + w - slot.sum[g];
    roll.sum[g] = h;
    slot.sum[g] = w;
    cur.sum[g] = 0ull;
    block[lay.sum + 2 * (size_t)g] = (uint32_t)w;
    block[lay.sum + 2 * (size_t)g + 1] = (uint32_t)(w >> 32);
    block[lay.sum_roll + 2 * (size_t)g] = (uint32_t)h;
    block[lay.sum_roll + 2 * (size_t)g + 1] = (uint32_t)(h >> 32);
  }
}

}  // namespace
}  // namespace decodesli

using namespace decodesli;

DecodeSliTracker::DecodeSliTracker(const Config& cfg)
    : cfg_(cfg),
      lay_(layout(cfg.group_cap)),
      lane_("decode sli", checked(cfg).device, cfg.n_buffers, cfg.span_cap, lay_.words, 1) {
  lane_.identify(decodesli::fingerprint(cfg));
  slo_us_ = decodesli::tpot_slo_us(cfg.tpot_slo_ms);
  const size_t rows = (size_t)cfg.windows + 2, G = (size_t)cfg.group_cap;
  hist_ = lane_.zeroed<uint32_t>(rows * G * kK);
  cells_ = lane_.zeroed<uint32_t>(rows * G * kCells);
  sum_ = lane_.zeroed<unsigned long long>(rows * G);
  lane_.ready();
}

int64_t DecodeSliTracker::step(const std::vector<Range>& spans, int n_groups) {
  check_step(n_groups, cfg_.group_cap);
  const size_t n = plan_ranges(spans, cfg_.span_cap);
  // nothing has changed up to here
  const auto [idx, s] = lane_.begin(spans);
  const hipStream_t st = lane_.stream();
  uint32_t* const blk = lane_.block();
  const size_t W = (size_t)cfg_.windows, at = (size_t)(idx % (int64_t)W);
  const Rows cur{hist(W + 1), cells(W + 1), sums(W + 1)};
  const dim3 block(kNT);
  if (n) {
    const dim3 og(grid_for((int64_t)n, kNT, 1024));
    const float slo = (float)cfg_.slo_ms;
    uint32_t* stats = blk + lay_.stats;
    if (cfg_.lds)
      hipLaunchKernelGGL(k_decode_observe<true>, og, block, 0, st, lane_.spans(), (int)n, n_groups, slo, slo_us_, cur.hist,
                         cur.cells, cur.sum, stats);
    else
      hipLaunchKernelGGL(k_decode_observe<false>, og, block, 0, st, lane_.spans(), (int)n, n_groups, slo, slo_us_, cur.hist,
                         cur.cells, cur.sum, stats);
  }
  lane_.mark(s, StepLane::kObserved);
  hipLaunchKernelGGL(k_decode_roll, dim3(grid_for(cfg_.group_cap, kRowsPerBlock, 1 << 20)), block, 0, st, cur,
                     Rows{hist(at), cells(at), sums(at)}, Rows{hist(W), cells(W), sums(W)}, blk, lay_, cfg_.group_cap);
  lane_.publish(s, 64);
  return idx;
}

std::vector<float> DecodeSliTracker::step_ms(int64_t i) {
  return {lane_.ms(i, StepLane::kBegin, StepLane::kEnd), lane_.ms(i, StepLane::kCopied, StepLane::kEnd),
          lane_.ms(i, StepLane::kCopied, StepLane::kObserved)};
}

Resident DecodeSliTracker::resident() {
  sync();
  const size_t W = (size_t)cfg_.windows, G = (size_t)cfg_.group_cap;
  Resident out;
  out.pos = lane_.steps() % (int64_t)W;
  out.rows.resize(G * kK);
  out.cells.resize(G * kCells);
  out.sums.resize(G);
  HIPCHECK(hipMemcpy(out.rows.data(), hist(W), out.rows.size() * 4, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(out.cells.data(), cells(W), out.cells.size() * 4, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(out.sums.data(), sums(W), out.sums.size() * 8, hipMemcpyDeviceToHost));
  return out;
}

}  // namespace mislo
