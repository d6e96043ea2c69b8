// Load SLI per service (loadsli.h): the kernels and the host class.
#include "loadsli.h"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace mislo {
namespace loadsli {

namespace {

constexpr int kNT = 256;
constexpr int kWave = 64;
constexpr int kRowsPerBlock = kNT / kWave;

static_assert(kLdsSlots == kNT, "observe flushes its LDS table one slot per thread");
static_assert(kMinBins == kWave, "scan: every lane owns bins / 64 >= 1 bins");
static_assert(kMaxBins <= (int)kCarrySlot, "the carry key's slot is no ring slot");

using u64 = unsigned long long;

__device__ __forceinline__ int64_t shfl_up64(int64_t v, int d) { return (int64_t)__shfl_up((long long)v, (unsigned)d, kWave); }
__device__ __forceinline__ int64_t wave_max64(int64_t v) {
  for (int d = kWave / 2; d; d >>= 1) {
    const int64_t o = (int64_t)__shfl_xor((long long)v, d, kWave);
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ int64_t wave_min64(int64_t v) {
  for (int d = kWave / 2; d; d >>= 1) {
    const int64_t o = (int64_t)__shfl_xor((long long)v, d, kWave);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ int64_t wave_sum64(int64_t v) {
  for (int d = kWave / 2; d; d >>= 1) v += (int64_t)__shfl_xor((long long)v, d, kWave);
  return v;
}
__device__ __forceinline__ uint32_t wave_sum32(uint32_t v) {
  for (int d = kWave / 2; d; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, kWave);
  return v;
}

// One wave per row of group_cap: the bins (prev, prev + count] enter the ring, count = min(bins,
// q_hi - prev) >= 1; the bins they evict sit in the same slots. The wave sums the evicted bins'
// starts - ends, clears both cells of every such slot, and lane 0 adds the sum to the row's carry
// (the row's only writer). g < group_cap and slot < bins: every access lies inside the arrays.
__global__ __launch_bounds__(kNT) void k_load_advance(u64* __restrict__ counts, u64* __restrict__ idle,
                                                      int32_t* __restrict__ carry, int group_cap, uint32_t bins, int64_t prev,
                                                      uint32_t count) {
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
  const int g = blockIdx.x * kRowsPerBlock + w;
  if (g >= group_cap) return;  // the whole wave; no barrier below
  u64* crow = counts + (size_t)g * bins;
  u64* irow = idle + (size_t)g * bins;
  int64_t d = 0;
  for (uint32_t j = (uint32_t)lane; j < count; j += kWave) {
    const uint32_t s = onset::slot_of(prev + 1 + (int64_t)j, bins);
    d += cell_delta(crow[s]);
    crow[s] = 0ull;
    irow[s] = 0ull;
  }
  d = wave_sum64(d);
  if (lane == 0 && d != 0) carry[g] += (int32_t)d;
}

// One thread per record. A record that ends a request (neither a start nor a first-token record) with
// a service below n_groups, a latency in [0, a day] and a start time is observed: place() says where
// its start and its end go; each is one add into `counts` and one into `idle_us` of its (service,
// slot), merged into one update when both fall into the same bin. Ends pile onto the newest few bins
// of a busy service: with kLds the workgroup aggregates in an LDS table of kLdsSlots keyed (service,
// slot) -- a slot claimed by a 64-bit compare-and-swap, kLdsProbes probes, then the ring itself -- and
// flushes every key once. A clipped record's carry increment goes through the same table under the
// slot kCarrySlot. g < n_groups <= group_cap and slot < bins: every add lies inside the arrays.
template <bool kLds>
__global__ __launch_bounds__(kNT) void k_load_observe(const Span* __restrict__ sp, int n, int n_groups, int64_t bin_us,
                                                      int64_t q_hi, uint32_t bins, int64_t long_us, u64* __restrict__ counts,
                                                      u64* __restrict__ idle, int32_t* __restrict__ carry,
                                                      uint32_t* __restrict__ stats) {
  __shared__ u64 s_key[kLds ? kLdsSlots : 1];
  __shared__ u64 s_cnt[kLds ? kLdsSlots : 1];
  __shared__ u64 s_idle[kLds ? kLdsSlots : 1];
  __shared__ uint32_t s_stats[kStats];
  if (kLds) s_key[threadIdx.x] = 0ull, s_cnt[threadIdx.x] = 0ull, s_idle[threadIdx.x] = 0ull;
  if (threadIdx.x < kStats) s_stats[threadIdx.x] = 0u;
  __syncthreads();
  // one update of (g, slot): `c` into counts (or carry, slot == kCarrySlot), `i` into idle_us
  auto update = [&](uint32_t g, uint32_t slot, u64 c, u64 i) {
    if (kLds) {
      const u64 key = lds_key(g, slot);
      uint32_t s = lds_hash(key);
      for (int probe = 0; probe < kLdsProbes; ++probe, s = (s + 1u) & (kLdsSlots - 1)) {
        u64 k = __hip_atomic_load(&s_key[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (k == 0ull) {
          k = atomicCAS(&s_key[s], 0ull, key);
          if (k == 0ull) k = key;
        }
        if (k == key) {
          atomicAdd(&s_cnt[s], c);
          if (i) atomicAdd(&s_idle[s], i);
          return;
        }
      }
    }
    if (slot == kCarrySlot) {
      atomicAdd(carry + g, (int32_t)c);
      return;
    }
    atomicAdd(counts + (size_t)g * bins + slot, c);
    if (i) atomicAdd(idle + (size_t)g * bins + slot, i);
  };
  for (size_t i = blockIdx.x * (size_t)kNT + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * kNT) {
    if (sp[i].flags & kNotAnEnd) continue;
    const uint32_t g = sp[i].group_id;
    if (g >= (uint32_t)n_groups) {
      atomicAdd(&s_stats[kOutOfGroup], 1u);
      continue;
    }
    const float v = sp[i].latency_ms;
    if (!latency_valid(v)) {
      atomicAdd(&s_stats[kInvalid], 1u);
      continue;
    }
    const int64_t ts_ns = sp[i].ts_ns;
    if (ts_ns <= 0) {
      atomicAdd(&s_stats[kNoTime], 1u);
      continue;
    }
    atomicAdd(&s_stats[kObserved], 1u);
    const int64_t dur_us = dur_us_of(v);
    if (dur_us > long_us) atomicAdd(&s_stats[kLong], 1u);
    const Placement p = place(ts_us_of(ts_ns), dur_us, bin_us, q_hi, bins);
    if (p.bits & kPFuture) atomicAdd(&s_stats[kFuture], 1u);
    if (p.bits & kPTooOld) {
      atomicAdd(&s_stats[kTooOld], 1u);
      continue;
    }
    if (p.bits & kPClipped) {
      atomicAdd(&s_stats[kClipped], 1u);
      update(g, kCarrySlot, 1ull, 0ull);
    }
    if ((p.bits & kPStart) && p.qs == p.qe) {
      update(g, onset::slot_of(p.qe, bins), kStartAdd + kEndAdd, p.idle_s + p.idle_e);
    } else {
      if (p.bits & kPStart) update(g, onset::slot_of(p.qs, bins), kStartAdd, p.idle_s);
      update(g, onset::slot_of(p.qe, bins), kEndAdd, p.idle_e);
    }
  }
  __syncthreads();
  if (kLds) {
    const u64 key = s_key[threadIdx.x];
    if (key != 0ull) {
      const uint32_t g = lds_group(key), slot = lds_slot(key);
      if (slot == kCarrySlot) {
        atomicAdd(carry + g, (int32_t)s_cnt[threadIdx.x]);
      } else {
        atomicAdd(counts + (size_t)g * bins + slot, s_cnt[threadIdx.x]);
        if (s_idle[threadIdx.x]) atomicAdd(idle + (size_t)g * bins + slot, s_idle[threadIdx.x]);
      }
    }
  }
  if (threadIdx.x < kStats && s_stats[threadIdx.x]) atomicAdd(&stats[threadIdx.x], s_stats[threadIdx.x]);
}

struct ScanParams {
  int64_t q_hi, q_first, bin_us, factor_milli, min_requests, min_conc_milli;
  uint32_t bins;
  int settle, recent, min_base_bins, group_cap;
};

// One wave per service row, every row of group_cap. In ring order (index 0 = the oldest bin
// q_hi - bins + 1) lane l owns the bins / 64 consecutive bins from l * bins / 64. It sums their
// starts - ends; the wave's inclusive scan of the sums (__shfl_up), shifted by one lane and started at
// carry, gives the lane the requests in flight before its first bin. In one pass over its bins it then
// has every bin's active and busy, and accumulates the ring's, the recent range's and the base range's
// sums and its own peak (the first bin with its largest active). Wave reductions give the sums and the
// peak, ties broken by the smaller bin; lane 0 classifies, updates age and the previous state and
// stores the row as five 16-byte stores.
__global__ __launch_bounds__(kNT) void k_load_scan(const u64* __restrict__ counts, const u64* __restrict__ idle,
                                                   const int32_t* __restrict__ carry, uint32_t* __restrict__ age,
                                                   uint32_t* __restrict__ prev_state, ScanParams P,
                                                   uint32_t* __restrict__ block, size_t rows_at) {
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
  const int g = blockIdx.x * kRowsPerBlock + w;
  if (g >= P.group_cap) return;  // the whole wave; no barrier below
  const uint32_t bins = P.bins;
  const u64* crow = counts + (size_t)g * bins;
  const u64* irow = idle + (size_t)g * bins;
  const uint32_t per = bins >> 6;
  const Ranges r = ranges_of(P.q_hi, P.q_first, bins, P.settle, P.recent, P.min_base_bins);
  const int64_t first = r.oldest + (int64_t)lane * per;
  int64_t run = 0;
  for (uint32_t j = 0; j < per; ++j) run = combine(run, cell_delta(crow[onset::slot_of(first + j, bins)]));
  for (int d = 1; d < kWave; d <<= 1) {
    const int64_t before = shfl_up64(run, d);
    if (lane >= d) run = combine(before, run);
  }
  int64_t A = shfl_up64(run, 1);
  if (lane == 0) A = 0;
  A += (int64_t)carry[g];
  int64_t busy_ring = 0, busy_rec = 0, busy_base = 0, pk = 0, pk_q = INT64_MAX;
  uint32_t arr_ring = 0, arr_rec = 0, arr_base = 0, done_rec = 0, done_base = 0;
  for (uint32_t j = 0; j < per; ++j) {
    const int64_t q = first + j;
    const uint32_t s = onset::slot_of(q, bins);
    const u64 c = crow[s];
    const int64_t active = bin_active(A, c), busy = bin_busy(active, P.bin_us, irow[s]);
    A += cell_delta(c);
    arr_ring += cell_starts(c), busy_ring += busy;
    if (active > pk) pk = active, pk_q = q;
    if (!r.warming) {
      if (q >= r.recent_lo && q <= r.recent_hi) arr_rec += cell_starts(c), done_rec += cell_ends(c), busy_rec += busy;
      if (q >= r.base_lo && q <= r.base_hi) arr_base += cell_starts(c), done_base += cell_ends(c), busy_base += busy;
    }
  }
  const int64_t peak = wave_max64(pk);
  const int64_t peak_q = wave_min64(pk == peak && peak > 0 ? pk_q : INT64_MAX);
  busy_ring = wave_sum64(busy_ring), busy_rec = wave_sum64(busy_rec), busy_base = wave_sum64(busy_base);
  arr_ring = wave_sum32(arr_ring), arr_rec = wave_sum32(arr_rec), arr_base = wave_sum32(arr_base);
  done_rec = wave_sum32(done_rec), done_base = wave_sum32(done_base);
  if (lane == 0) {
    uint32_t flags = 0u, state = kWarming;
    if (!r.warming) {
      const Sums sums{(uint64_t)busy_rec, (uint64_t)busy_base, arr_rec, arr_base};
      flags = predicates(sums, r.base_bins, (uint32_t)P.recent, P.bin_us, P.factor_milli, P.min_requests, P.min_conc_milli);
      state = state_of(flags);
    }
    const uint32_t a = age_of(state, prev_state[g], age[g]);
    age[g] = a;
    prev_state[g] = state;
    // the Row, word by word: state age peak_q | busy_recent busy_base | busy_ring arr_recent arr_base |
    // done_recent done_base peak_active base_bins | arr_ring flags pad pad
    const uint64_t pq = (uint64_t)(peak > 0 ? peak_q : kNoBin), br = (uint64_t)busy_rec, bb = (uint64_t)busy_base,
                   bg = (uint64_t)busy_ring;
    uint4* out = reinterpret_cast<uint4*>(block + rows_at) + (size_t)g * (kRowBytes / 16);
    out[0] = make_uint4(state, a, (uint32_t)pq, (uint32_t)(pq >> 32));
    out[1] = make_uint4((uint32_t)br, (uint32_t)(br >> 32), (uint32_t)bb, (uint32_t)(bb >> 32));
    out[2] = make_uint4((uint32_t)bg, (uint32_t)(bg >> 32), arr_rec, arr_base);
    out[3] = make_uint4(done_rec, done_base, (uint32_t)peak, r.warming ? 0u : r.base_bins);
    out[4] = make_uint4(arr_ring, flags, 0u, 0u);
  }
}

}  // namespace
}  // namespace loadsli

using namespace loadsli;

LoadSliTracker::LoadSliTracker(const Config& cfg)
    : cfg_(cfg),
      lay_(layout(cfg.group_cap)),
      pop_((uint32_t)cfg.bins, cfg.ring_records_max),
      lane_("load sli", checked(cfg).device, cfg.n_buffers, cfg.span_cap, lay_.words, 2) {
  lane_.identify(loadsli::fingerprint(cfg), 3);
  const size_t cells = (size_t)cfg.group_cap * (size_t)cfg.bins, G = (size_t)cfg.group_cap;
  counts_ = lane_.zeroed<unsigned long long>(cells);
  idle_ = lane_.zeroed<unsigned long long>(cells);
  carry_ = lane_.zeroed<int32_t>(G);
  age_ = lane_.zeroed<uint32_t>(2 * G);
  lane_.ready();
}

int64_t LoadSliTracker::step(const std::vector<Range>& spans, int64_t cut_ns, int n_groups) {
  check_step(cut_ns, n_groups, cfg_.group_cap);
  const size_t n = plan_ranges(spans, cfg_.span_cap);
  const int64_t prev = q_hi_, q_hi = onset::advance(prev, ts_us_of(cut_ns), cfg_.bin_us);
  pop_.check(q_hi, n);
  // nothing has changed up to here
  pop_.take(q_hi, n);
  q_hi_ = q_hi;
  const uint32_t bins = (uint32_t)cfg_.bins;
  if (prev == kNoBin || q_hi - prev >= (int64_t)bins) q_first_ = q_hi;
  const auto [idx, s] = lane_.begin(spans);
  const hipStream_t st = lane_.stream();
  uint32_t* const blk = lane_.block();
  const int G = cfg_.group_cap;
  uint32_t* stats = blk + lay_.stats;
  const dim3 block(kNT), rows(grid_for(G, kRowsPerBlock, 1 << 20));
  if (q_hi > prev)
    hipLaunchKernelGGL(k_load_advance, rows, block, 0, st, counts_, idle_, carry_, G, bins, prev,
                       onset::cleared(prev, q_hi, bins));
  lane_.mark(s, StepLane::kAdvanced);
  if (n) {
    const dim3 og(grid_for((int64_t)n, kNT, 1024));
    const int64_t long_us = (int64_t)cfg_.settle_bins * cfg_.bin_us;
    if (cfg_.lds)
      hipLaunchKernelGGL(k_load_observe<true>, og, block, 0, st, lane_.spans(), (int)n, n_groups, cfg_.bin_us, q_hi, bins,
                         long_us, counts_, idle_, carry_, stats);
    else
      hipLaunchKernelGGL(k_load_observe<false>, og, block, 0, st, lane_.spans(), (int)n, n_groups, cfg_.bin_us, q_hi, bins,
                         long_us, counts_, idle_, carry_, stats);
  }
  lane_.mark(s, StepLane::kObserved);
  ScanParams P;
  P.q_hi = q_hi, P.q_first = q_first_, P.bin_us = cfg_.bin_us, P.factor_milli = cfg_.factor_milli;
  P.min_requests = cfg_.min_requests, P.min_conc_milli = cfg_.min_conc_milli, P.bins = bins;
  P.settle = cfg_.settle_bins, P.recent = cfg_.recent_bins, P.min_base_bins = cfg_.min_base_bins, P.group_cap = G;
  hipLaunchKernelGGL(k_load_scan, rows, block, 0, st, counts_, idle_, carry_, age_, age_ + G, P, blk, lay_.rows);
  lane_.publish(s, 1024);
  return idx;
}

std::vector<float> LoadSliTracker::step_ms(int64_t i) {
  return {lane_.ms(i, StepLane::kBegin, StepLane::kEnd), lane_.ms(i, StepLane::kCopied, StepLane::kEnd),
          lane_.ms(i, StepLane::kAdvanced, StepLane::kObserved)};
}

Resident LoadSliTracker::resident() {
  sync();
  Resident out;
  out.q_hi = q_hi_;
  out.q_first = q_first_;
  const size_t cells = (size_t)cfg_.group_cap * (size_t)cfg_.bins, G = (size_t)cfg_.group_cap;
  out.counts.resize(cells);
  out.idle_us.resize(cells);
  out.carry.resize(G);
  out.age.resize(G);
  out.prev_state.resize(G);
  HIPCHECK(hipMemcpy(out.counts.data(), counts_, cells * 8, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(out.idle_us.data(), idle_, cells * 8, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(out.carry.data(), carry_, G * 4, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(out.age.data(), age_, G * 4, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(out.prev_state.data(), age_ + G, G * 4, hipMemcpyDeviceToHost));
  return out;
}

}  // namespace mislo
