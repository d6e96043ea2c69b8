// Error SLI (errsli.h): the kernels and the host class.
#include "errsli.h"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace mislo {
namespace errsli {

namespace {

constexpr int kNT = 256;
constexpr int kWave = 64;
constexpr int kRowsPerBlock = kNT / kWave;
constexpr int kPairLanes = 2 * kMaxPairs;

static_assert(kLdsSlots == kNT, "observe flushes its LDS table one slot per thread");
static_assert(kPairLane0 + kPairLanes <= kWave && kSumWords == (size_t)kPairLanes * 2, "a pair window per lane");

using u64 = unsigned long long;

// `add` into the workgroup's table under `key`: claim-by-CAS, a bounded probe. False: no slot found.
__device__ __forceinline__ bool lds_add(u64* s_key, uint32_t* s_val, u64 key, uint32_t add) {
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

// One thread per record, the checks in the rules' order: a start or first-token record is skipped; a
// group at or above n_groups is out_of_group; a class of 8-15 reserved; the rest is observed: one add
// into its (service, class) cell of the step's row. With kLds the workgroup aggregates in an LDS table
// of kLdsSlots keyed (service, class) and sends each key to the step's row once; an add that finds no
// slot within kLdsProbes goes there itself. g < n_groups <= group_cap and c < 8 bound every index.
template <bool kLds>
__global__ __launch_bounds__(kNT) void k_err_observe(const Span* __restrict__ sp, int n, int n_groups,
                                                     uint32_t* __restrict__ cur, uint32_t* __restrict__ stats) {
  __shared__ u64 s_key[kLds ? kLdsSlots : 1];
  __shared__ uint32_t s_val[kLds ? kLdsSlots : 1];
  __shared__ uint32_t s_stats[kStats];
  if (kLds) s_key[threadIdx.x] = 0ull, s_val[threadIdx.x] = 0u;
  if (threadIdx.x < kStats) s_stats[threadIdx.x] = 0u;
  __syncthreads();
  for (size_t i = blockIdx.x * (size_t)kNT + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * kNT) {
    const uint32_t flags = sp[i].flags;
    if (flags & kSkipMask) continue;
    const uint32_t g = sp[i].group_id;
    if (g >= (uint32_t)n_groups) {
      atomicAdd(&s_stats[kOutOfGroup], 1u);
      continue;
    }
    const uint32_t c = outcome_of(flags);
    if (c >= (uint32_t)kClasses) {
      atomicAdd(&s_stats[kReserved], 1u);
      continue;
    }
    atomicAdd(&s_stats[kObserved], 1u);
    if (!kLds || !lds_add(s_key, s_val, lds_key(g, c), 1u)) atomicAdd(&cur[(size_t)g * kClasses + c], 1u);
  }
  __syncthreads();
  if (kLds) {
    const u64 key = s_key[threadIdx.x];
    if (key != 0ull) atomicAdd(&cur[(size_t)lds_group(key) * kClasses + lds_class(key)], s_val[threadIdx.x]);
  }
  if (threadIdx.x < kStats && s_stats[threadIdx.x]) atomicAdd(&stats[threadIdx.x], s_stats[threadIdx.x]);
}

// What the roll kernel's pair lanes need: lane 8 + i owns pair i / 2's long (i even) or short window.
struct RollArgs {
  const uint32_t* leave[kPairLanes];  // the horizon row of X steps ago; null while the ring fills
  u64 thr[kMaxPairs];                 // factor_milli * budget_ppm
  uint32_t n_pairs, min_requests, bad_mask;
};

// One wave per service row, every row of group_cap. Lanes 0-7 own a class: the window of W steps ago
// (`slot`) leaves the rolling row, this one (`cur`) enters and takes its place, the step's row is
// cleared. Lanes 8-15 own one window of one pair: each reads the 8 words of the row that leaves its
// window itself, adds the entering row's (n, bad) -- a reduction over lanes 0-7 under bad_mask --
// to its rolling sums and compares. A pair whose long window is the horizon loses the very row `slot`
// that the entering row is written to, so every lane reads before the barrier and writes after it.
__global__ __launch_bounds__(kNT) void k_err_roll(uint32_t* __restrict__ cur, uint32_t* slot, uint32_t* __restrict__ roll,
                                                  uint32_t* __restrict__ sums, uint32_t* __restrict__ age,
                                                  uint32_t* __restrict__ block, Layout lay, RollArgs a, int group_cap) {
  const int lane = threadIdx.x & (kWave - 1);
  const int g = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  const bool live = g < group_cap;  // the whole wave
  const int pl = lane - kPairLane0;
  const bool is_class = live && lane < kClasses;
  const bool is_pair = live && pl >= 0 && pl < 2 * (int)a.n_pairs;
  const size_t at = (size_t)(live ? g : 0) * kClasses + (size_t)(lane & (kClasses - 1));
  const size_t sat = (size_t)(live ? g : 0) * kSumWords + (size_t)((pl & (kPairLanes - 1)) * 2);
  uint32_t c = 0u, old = 0u, r = 0u, ln = 0u, lb = 0u, sn = 0u, sb = 0u;
  u64 thr = 0ull;
  if (is_class) c = cur[at], old = slot[at], r = roll[at];
  if (is_pair) {
    const uint32_t* lv = nullptr;
#pragma unroll
    for (int i = 0; i < kPairLanes; ++i)
      if (pl == i) lv = a.leave[i], thr = a.thr[i >> 1];
    if (lv != nullptr) {
#pragma unroll
      for (int j = 0; j < kClasses; ++j) {
        const uint32_t w = lv[(size_t)g * kClasses + j];
        ln += w;
        if ((a.bad_mask >> j) & 1u) lb += w;
      }
    }
    sn = sums[sat], sb = sums[sat + 1];
  }
  __syncthreads();
  if (is_class) {
    r = r + c - old;
    roll[at] = r;
    slot[at] = c;
    cur[at] = 0u;
    block[lay.counts + at] = c;
    block[lay.counts_roll + at] = r;
  }
  uint32_t en = is_class ? c : 0u, eb = (is_class && ((a.bad_mask >> lane) & 1u)) ? c : 0u;
#pragma unroll
  for (int d = kClasses / 2; d >= 1; d >>= 1) {
    en += __shfl_xor(en, d, kWave);
    eb += __shfl_xor(eb, d, kWave);
  }
  en = __shfl(en, 0, kWave);
  eb = __shfl(eb, 0, kWave);
  bool burn = false;
  if (is_pair) {
    sn = sn + en - ln;
    sb = sb + eb - lb;
    sums[sat] = sn;
    sums[sat + 1] = sb;
    block[lay.pair_sums + sat] = sn;
    block[lay.pair_sums + sat + 1] = sb;
    burn = burns(sn, sb, a.min_requests, thr);
  }
  const u64 m = __ballot(burn) >> kPairLane0;
  if (live && lane == 0) {
    uint32_t firing = 0u;
#pragma unroll
    for (int p = 0; p < kMaxPairs; ++p)
      if (((m >> (2 * p)) & 3ull) == 3ull) firing |= 1u << p;
    const uint32_t ag = next_age(age[g], firing);
    age[g] = ag;
    block[lay.firing + g] = firing;
    block[lay.age + g] = ag;
  }
}

}  // namespace
}  // namespace errsli

using namespace errsli;

ErrorSliTracker::ErrorSliTracker(const Config& cfg)
    : cfg_(cfg),
      lay_(layout(cfg.group_cap)),
      lane_("error sli", checked(cfg).device, cfg.n_buffers, cfg.span_cap, lay_.words, 1) {
  lane_.identify(errsli::fingerprint(cfg));
  budget_ = errsli::budget_ppm(cfg.target);
  const size_t rows = (size_t)cfg.windows + 2, G = (size_t)cfg.group_cap;
  rows_ = lane_.zeroed<uint32_t>(rows * G * kRowWords);
  sums_ = lane_.zeroed<uint32_t>(G * kSumWords);
  age_ = lane_.zeroed<uint32_t>(G);
  lane_.ready();
}

int64_t ErrorSliTracker::step(const std::vector<Range>& spans, int n_groups) {
  check_step(n_groups, cfg_.group_cap);
  const size_t n = plan_ranges(spans, cfg_.span_cap);
  // nothing has changed up to here
  const auto [idx, s] = lane_.begin(spans);
  const hipStream_t st = lane_.stream();
  uint32_t* const blk = lane_.block();
  const int64_t W = cfg_.windows;
  const size_t at = (size_t)(idx % W);
  uint32_t* cur = row((size_t)W + 1);
  const dim3 block(kNT);
  if (n) {
    const dim3 og(grid_for((int64_t)n, kNT, 1024));
    uint32_t* stats = blk + lay_.stats;
    if (cfg_.lds)
      hipLaunchKernelGGL(k_err_observe<true>, og, block, 0, st, lane_.spans(), (int)n, n_groups, cur, stats);
    else
      hipLaunchKernelGGL(k_err_observe<false>, og, block, 0, st, lane_.spans(), (int)n, n_groups, cur, stats);
  }
  lane_.mark(s, StepLane::kObserved);
  RollArgs a{};
  a.n_pairs = (uint32_t)cfg_.pairs.size();
  a.min_requests = (uint32_t)cfg_.min_requests;
  a.bad_mask = cfg_.bad_mask;
  for (size_t p = 0; p < cfg_.pairs.size(); ++p) {
    a.thr[p] = (u64)cfg_.pairs[p].factor_milli * (u64)budget_;
    const int64_t x[2] = {cfg_.pairs[p].long_windows, cfg_.pairs[p].short_windows};
    // the step x before this one filled row (idx - x) % W, and nothing has replaced it since (x <= W)
    for (int k = 0; k < 2; ++k) a.leave[2 * p + k] = idx >= x[k] ? row((size_t)((idx - x[k]) % W)) : nullptr;
  }
  hipLaunchKernelGGL(k_err_roll, dim3(grid_for(cfg_.group_cap, kRowsPerBlock, 1 << 20)), block, 0, st, cur, row(at),
                     row((size_t)W), sums_, age_, blk, lay_, a, cfg_.group_cap);
  lane_.publish(s, 64);
  return idx;
}

std::vector<float> ErrorSliTracker::step_ms(int64_t i) {
  return {lane_.ms(i, StepLane::kBegin, StepLane::kEnd), lane_.ms(i, StepLane::kCopied, StepLane::kEnd),
          lane_.ms(i, StepLane::kCopied, StepLane::kObserved)};
}

Resident ErrorSliTracker::resident() {
  sync();
  const size_t W = (size_t)cfg_.windows, G = (size_t)cfg_.group_cap;
  Resident out;
  out.pos = lane_.steps() % (int64_t)W;
  out.counts.resize(G * kRowWords);
  out.sums.resize(G * kSumWords);
  out.age.resize(G);
  HIPCHECK(hipMemcpy(out.counts.data(), row(W), out.counts.size() * 4, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(out.sums.data(), sums_, out.sums.size() * 4, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(out.age.data(), age_, out.age.size() * 4, hipMemcpyDeviceToHost));
  return out;
}

}  // namespace mislo
