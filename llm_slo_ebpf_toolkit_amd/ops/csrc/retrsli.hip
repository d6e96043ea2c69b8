// TTFT phase split (retrsli.h): the kernels and the host class.
#include "retrsli.h"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace mislo {
namespace retrsli {

namespace {

constexpr int kNT = 256;
constexpr int kWave = 64;
constexpr int kRowsPerBlock = kNT / (2 * kWave);  // two waves per service row
constexpr int kSlotsPerThread = kLdsSlots / kNT;

static_assert(kLdsSlots % kNT == 0, "observe clears and flushes its LDS table kSlotsPerThread slots per thread");
static_assert(kCells + 1 <= kCellStride && kCellStride + 2 <= kWave, "the roll kernel's lanes 0-6 own the counters, 8 and 9 the sums");

using u64 = unsigned long long;

// One state row of [group_cap] services: the two histograms, the counters (six cells, sli), the sums.
struct Rows {
  uint32_t* hist_r;
  uint32_t* hist_m;
  uint32_t* cells;
  u64* sum;
};

// `add` into the workgroup's table under `key`: claim-by-CAS, a bounded probe. False: no slot found.
__device__ __forceinline__ bool lds_add(u64* s_key, u64* s_val, u64 key, u64 add) {
  uint32_t s = lds_hash(key);
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

// an aggregate of (service g, what) into the step's row; g < n_groups <= group_cap, what <= kWhatSli
__device__ __forceinline__ void global_add(uint32_t g, uint32_t what, u64 add, const Rows& cur) {
  if (what < kWhatModel)
    atomicAdd(&cur.hist_r[(size_t)g * kK + what], (uint32_t)add);
  else if (what < kWhatCell)
    atomicAdd(&cur.hist_m[(size_t)g * kK + (what - kWhatModel)], (uint32_t)add);
  else if (what < kWhatSumR)
    atomicAdd(&cur.cells[(size_t)g * kCellStride + (what - kWhatCell)], (uint32_t)add);
  else if (what == kWhatSli)
    atomicAdd(&cur.cells[(size_t)g * kCellStride + kSliWord], (uint32_t)add);
  else
    atomicAdd(&cur.sum[(size_t)g * 2 + (what - kWhatSumR)], add);
}

// One thread per record, the checks in the rules' order: a start record is skipped; a group at or above
// n_groups is out_of_group; a TTFT that is not >= 0 (NaN and negatives fail the compare) invalid; a record
// without SPAN_NO_SLI counts in the service's sli; a retrieval time outside (0, 1e7) ms (NaN fails the
// compare) is no_breakdown; the rest is observed: one add each into its retrieval bucket, its model
// bucket, its cell and the two sums. With kLds the workgroup aggregates them in an LDS table of kLdsSlots
// keyed (service, what) and sends each key to the step's row once; an add that finds no slot within
// kLdsProbes goes there itself.
template <bool kLds>
__global__ __launch_bounds__(kNT) void k_retr_observe(const Span* __restrict__ sp, int n, int n_groups, float slo,
                                                      uint32_t slo_u, uint32_t budget_u, Rows cur,
                                                      uint32_t* __restrict__ stats) {
  __shared__ u64 s_key[kLds ? kLdsSlots : 1];
  __shared__ u64 s_val[kLds ? kLdsSlots : 1];
  __shared__ uint32_t s_stats[kStats];
  if (kLds) {
#pragma unroll
    for (int j = 0; j < kSlotsPerThread; ++j) s_key[j * kNT + threadIdx.x] = 0ull, s_val[j * kNT + threadIdx.x] = 0ull;
  }
  if (threadIdx.x < kStats) s_stats[threadIdx.x] = 0u;
  __syncthreads();
  for (size_t i = blockIdx.x * (size_t)kNT + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * kNT) {
    const uint32_t flags = sp[i].flags;
    if (flags & kSpanStart) continue;
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
    if (!(flags & kSpanNoSli))
      if (!kLds || !lds_add(s_key, s_val, lds_key(g, kWhatSli), 1ull)) global_add(g, kWhatSli, 1ull, cur);
    const float rm = sp[i].retr_ms;
    if (!(rm > 0.f && rm < kRetrMaxMs)) {
      atomicAdd(&s_stats[kNoBreakdown], 1u);
      continue;
    }
    atomicAdd(&s_stats[kObserved], 1u);
    if (flags & kSpanNoSli) atomicAdd(&s_stats[kExtra], 1u);
    const uint32_t r = units_of_ms(rm), t = units_of_ms(v), m = model_units(t, r);
    if (r > t) atomicAdd(&s_stats[kExceedsTtft], 1u);
    const uint32_t what[5] = {decodesli::bucket_of(r), kWhatModel + decodesli::bucket_of(m),
                              kWhatCell + cell_of(v > slo, r, m, slo_u, budget_u), kWhatSumR, kWhatSumT};
    const u64 add[5] = {1ull, 1ull, 1ull, (u64)r, (u64)t};
#pragma unroll
    for (int j = 0; j < 5; ++j)
      if (!kLds || !lds_add(s_key, s_val, lds_key(g, what[j]), add[j])) global_add(g, what[j], add[j], cur);
  }
  __syncthreads();
  if (kLds) {
#pragma unroll
    for (int j = 0; j < kSlotsPerThread; ++j) {
      const u64 key = s_key[j * kNT + threadIdx.x];
      if (key != 0ull) global_add(lds_group(key), lds_what(key), s_val[j * kNT + threadIdx.x], cur);
    }
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

// Two waves per service row, every row of group_cap: the even wave owns the retrieval histogram, the odd
// one the model histogram. The window of W steps ago (`slot`) leaves the rolling row, this one (`cur`)
// enters and takes its place in the horizon, the step's row is cleared; then the ranks of the window's
// and the rolling row. Lane l owns buckets [6 l, 6 l + 6). The even wave's lanes 0-5 roll the cells, lane
// 6 the SLI count, lanes 8 and 9 the sums; its lane 0 then decides the verdict over the rolling counters
// and the steps it has held (`verdict` = [2][group_cap]: state, age).
__global__ __launch_bounds__(kNT) void k_retr_roll(Rows cur, Rows slot, Rows roll, uint32_t* __restrict__ verdict,
                                                   uint32_t* __restrict__ block, Layout lay, Thresholds th,
                                                   int group_cap) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const int g = blockIdx.x * kRowsPerBlock + (wave >> 1);
  const bool model = wave & 1;
  if (g >= group_cap) return;  // the whole wave
  uint32_t* __restrict__ hc = model ? cur.hist_m : cur.hist_r;
  uint32_t* __restrict__ hs = model ? slot.hist_m : slot.hist_r;
  uint32_t* __restrict__ hr = model ? roll.hist_m : roll.hist_r;
  uint32_t c[kPerLane], r[kPerLane];
  uint32_t tc = 0, tr = 0;
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) c[j] = r[j] = 0u;
  if (lane < kRowLanes) {
    const size_t at = (size_t)g * kK + (size_t)lane * kPerLane;
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
      c[j] = hc[at + j];
      r[j] = hr[at + j] + c[j] - hs[at + j];
      hr[at + j] = r[j];
      hs[at + j] = c[j];
      hc[at + j] = 0u;
      tc += c[j];
      tr += r[j];
    }
  }
  const uint32_t ic = wave_scan(tc, lane), ir = wave_scan(tr, lane);
  const uint32_t n = __shfl(ic, kWave - 1, kWave), n_roll = __shfl(ir, kWave - 1, kWave);
  pick_ranks(c, ic, tc, n, lane, block + (model ? lay.q_m_win : lay.q_r_win) + (size_t)g * kQuantiles);
  pick_ranks(r, ir, tr, n_roll, lane, block + (model ? lay.q_m_roll : lay.q_r_roll) + (size_t)g * kQuantiles);
  if (model) return;  // the whole wave
  uint32_t h = 0u;
  if (lane <= kSliWord) {
    const size_t at = (size_t)g * kCellStride + lane;
    const uint32_t w = cur.cells[at];
    h = roll.cells[at] + w - slot.cells[at];
    roll.cells[at] = h;
    slot.cells[at] = w;
    cur.cells[at] = 0u;
    if (lane < kCells) {
      block[lay.cells + at] = w;
      block[lay.cells_roll + at] = h;
    } else {
      block[lay.sli + g] = w;
      block[lay.sli_roll + g] = h;
    }
  } else if (lane == kCellStride || lane == kCellStride + 1) {
    const int k = lane - kCellStride;  // 0: retrieval, 1: TTFT
    const size_t at = (size_t)g * 2 + k;
    const u64 w = cur.sum[at], s = roll.sum[at] + w - slot.sum[at];
    roll.sum[at] = s;
    slot.sum[at] = w;
    cur.sum[at] = 0ull;
    const size_t win = (k ? lay.sum_t : lay.sum_r) + 2 * (size_t)g, hor = (k ? lay.sum_t_roll : lay.sum_r_roll) + 2 * (size_t)g;
    block[win] = (uint32_t)w;
    block[win + 1] = (uint32_t)(w >> 32);
    block[hor] = (uint32_t)s;
    block[hor + 1] = (uint32_t)(s >> 32);
  }
  uint32_t rolled[kCells];
#pragma unroll
  for (int j = 0; j < kCells; ++j) rolled[j] = __shfl(h, j, kWave);
  const uint32_t sli = __shfl(h, kSliWord, kWave);
  if (lane == 0) {
    const uint32_t state = state_of(rolled, sli, th), age = age_of(state, verdict[g], verdict[(size_t)group_cap + g]);
    verdict[g] = state;
    verdict[(size_t)group_cap + g] = age;
    block[lay.state + g] = state;
    block[lay.age + g] = age;
  }
}

}  // namespace
}  // namespace retrsli

using namespace retrsli;

RetrievalSliTracker::RetrievalSliTracker(const Config& cfg)
    : cfg_(cfg),
      lay_(layout(cfg.group_cap)),
      lane_("retrieval sli", checked(cfg).device, cfg.n_buffers, cfg.span_cap, lay_.words, 1) {
  lane_.identify(retrsli::fingerprint(cfg));
  slo_u_ = units_of_ms((float)cfg.slo_ms);
  budget_u_ = retrsli::budget_units(cfg.retrieval_budget_ms);
  const size_t rows = (size_t)cfg.windows + 2, G = (size_t)cfg.group_cap;
  hist_r_ = lane_.zeroed<uint32_t>(rows * G * kK);
  hist_m_ = lane_.zeroed<uint32_t>(rows * G * kK);
  cells_ = lane_.zeroed<uint32_t>(rows * G * kCellStride);
  sum_ = lane_.zeroed<unsigned long long>(rows * G * 2);
  verdict_ = lane_.zeroed<uint32_t>(2 * G);
  lane_.ready();
}

int64_t RetrievalSliTracker::step(const std::vector<Range>& spans, int n_groups) {
  check_step(n_groups, cfg_.group_cap);
  const size_t n = plan_ranges(spans, cfg_.span_cap);
  // nothing has changed up to here
  const auto [idx, s] = lane_.begin(spans);
  const hipStream_t st = lane_.stream();
  uint32_t* const blk = lane_.block();
  const size_t W = (size_t)cfg_.windows, at = (size_t)(idx % (int64_t)W);
  const Rows cur{hist_r(W + 1), hist_m(W + 1), cells(W + 1), sums(W + 1)};
  const dim3 block(kNT);
  if (n) {
    const dim3 og(grid_for((int64_t)n, kNT, 1024));
    const float slo = (float)cfg_.slo_ms;
    uint32_t* stats = blk + lay_.stats;
    if (cfg_.lds)
      hipLaunchKernelGGL(k_retr_observe<true>, og, block, 0, st, lane_.spans(), (int)n, n_groups, slo, slo_u_, budget_u_, cur,
                         stats);
    else
      hipLaunchKernelGGL(k_retr_observe<false>, og, block, 0, st, lane_.spans(), (int)n, n_groups, slo, slo_u_, budget_u_, cur,
                         stats);
  }
  lane_.mark(s, StepLane::kObserved);
  hipLaunchKernelGGL(k_retr_roll, dim3(grid_for(cfg_.group_cap, kRowsPerBlock, 1 << 20)), block, 0, st, cur,
                     Rows{hist_r(at), hist_m(at), cells(at), sums(at)}, Rows{hist_r(W), hist_m(W), cells(W), sums(W)}, verdict_,
                     blk, lay_, thresholds(cfg_), cfg_.group_cap);
  lane_.publish(s, 64);
  return idx;
}

std::vector<float> RetrievalSliTracker::step_ms(int64_t i) {
  return {lane_.ms(i, StepLane::kBegin, StepLane::kEnd), lane_.ms(i, StepLane::kCopied, StepLane::kEnd),
          lane_.ms(i, StepLane::kCopied, StepLane::kObserved)};
}

Resident RetrievalSliTracker::resident() {
  sync();
  const size_t W = (size_t)cfg_.windows, G = (size_t)cfg_.group_cap;
  Resident out;
  out.pos = lane_.steps() % (int64_t)W;
  out.rows_r.resize(G * kK);
  out.rows_m.resize(G * kK);
  out.cells.resize(G * kCellStride);
  out.sums.resize(G * 2);
  out.state.resize(G);
  out.age.resize(G);
  HIPCHECK(hipMemcpy(out.rows_r.data(), hist_r(W), out.rows_r.size() * 4, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(out.rows_m.data(), hist_m(W), out.rows_m.size() * 4, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(out.cells.data(), cells(W), out.cells.size() * 4, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(out.sums.data(), sums(W), out.sums.size() * 8, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(out.state.data(), verdict_, G * 4, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(out.age.data(), verdict_ + G, G * 4, hipMemcpyDeviceToHost));
  return out;
}

}  // namespace mislo
