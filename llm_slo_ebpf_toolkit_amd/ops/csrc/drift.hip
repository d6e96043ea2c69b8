// TTFT drift (drift.h): the kernels and the host class.
#include "drift.h"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace mislo {
namespace drift {

namespace {

constexpr int kNT = 256;
constexpr int kWave = 64;
constexpr int kRowsPerBlock = kNT / kWave;

static_assert(kLdsSlots == kNT, "observe flushes its LDS table one slot per thread");

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

// One thread per record, the TTFT sketch's rules: a record without kSpanNoSli and with a group below
// n_groups counts; of those a TTFT >= 0 (NaN and negatives fail the compare) is observed: one add into
// its (service, bucket) cell of the step's row. With kLds the workgroup aggregates in an LDS table of
// kLdsSlots keyed (service, bucket) and sends each key to the step's row once; an add that finds no
// slot within kLdsProbes goes there itself. The statistics are merged in LDS, one flush per workgroup.
template <bool kLds>
__global__ __launch_bounds__(kNT) void k_drift_observe(const Span* __restrict__ sp, int n, int n_groups,
                                                       uint32_t* __restrict__ cur, uint32_t* __restrict__ stats) {
  __shared__ u64 s_key[kLds ? kLdsSlots : 1];
  __shared__ uint32_t s_val[kLds ? kLdsSlots : 1];
  __shared__ uint32_t s_stats[kStats];
  if (kLds) s_key[threadIdx.x] = 0ull, s_val[threadIdx.x] = 0u;
  if (threadIdx.x < kStats) s_stats[threadIdx.x] = 0u;
  __syncthreads();
  for (size_t i = blockIdx.x * (size_t)kNT + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * kNT) {
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
    atomicAdd(&s_stats[kObserved], 1u);
    const uint32_t b = slisketch::bucket_of_bits(__float_as_uint(v));  // <= kK - 1 < kRowStride; g < n_groups <= group_cap
    if (!kLds || !lds_add(s_key, s_val, lds_key(g, b), 1u)) atomicAdd(&cur[(size_t)g * kRowStride + b], 1u);
  }
  __syncthreads();
  if (kLds) {
    const u64 key = s_key[threadIdx.x];
    if (key != 0ull) atomicAdd(&cur[(size_t)lds_group(key) * kRowStride + lds_bucket(key)], s_val[threadIdx.x]);
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

__device__ __forceinline__ u64 wave_max(u64 x) {
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) {
    const u64 t = __shfl_xor(x, d, kWave);
    x = t > x ? t : x;
  }
  return x;
}

// One quantile bucket of a row, in every lane: `h` this lane's buckets, `incl` the inclusive scan of
// the lanes' totals, `n` the row's total (the same in every lane). The one lane whose buckets hold the
// rank finds the first bucket whose cumulative count reaches it; the wave reads it from that lane.
__device__ __forceinline__ uint32_t rank_bucket(const uint32_t (&h)[kPerLane], uint32_t incl, uint32_t mine, uint32_t n,
                                                int lane, int q) {
  if (n == 0u) return kEmpty;
  const uint32_t excl = incl - mine;
  const uint64_t r = slisketch::rank_of(slisketch::quantile_permille(q), n);
  const bool own = (uint64_t)excl < r && r <= (uint64_t)incl;
  uint32_t v = 0u;
  if (own) {
    uint64_t cum = excl;
    int j = 0;
    for (; j < kPerLane - 1; ++j) {
      cum += h[j];
      if (cum >= r) break;
    }
    v = (uint32_t)(lane * kPerLane + j);
  }
  const u64 m = __ballot(own);
  return __shfl(v, __ffsll((long long)m) - 1, kWave);
}

struct RollArgs {
  uint32_t* cur;        // this step's row, cleared here
  uint32_t* recent;
  uint32_t* base;
  uint32_t* near_out;   // the window of R steps ago, leaving `recent`; null before step R
  uint32_t* near_slot;  // the near ring's row of this step: the window of R + L steps ago, replaced by this one
  uint32_t* ring;       // base_ring[B]
  size_t ring_stride;   // words of one ring row: group_cap * kRowStride
  uint32_t B;
  uint32_t hold_max;
  int leaves_gap;       // step >= R + L: near_slot holds a window that leaves the gap now
  Thresholds t;
};

// One wave per service row, every row of group_cap; lane l owns buckets [7 l, 7 l + 7). In the rules'
// order: the window enters `recent` and the one of R steps ago leaves it; the window that leaves the gap
// is admitted to the baseline when the service was not slow in the step before and the window is not
// empty (a full baseline ring gives up its oldest row); the window takes its place in the near ring and
// the step's row is cleared. Then the statistic of (recent, base): two scans of the lanes' totals, each
// lane walks its buckets and forms the two cross products, a wave maximum over (numerator, lowest
// bucket); the ranks; the decision, the hold and the reset, the same in every lane. Lane 0 writes the
// row's words.
__global__ __launch_bounds__(kNT) void k_drift_roll(RollArgs a, Words w, uint32_t* __restrict__ block, Layout lay,
                                                    int group_cap) {
  const int lane = threadIdx.x & (kWave - 1);
  const int g = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (g >= group_cap) return;  // the whole wave
  const uint32_t prev = w.prev[g], fill = w.base_fill[g], pos = w.base_pos[g];
  uint32_t hold = w.hold[g];
  uint32_t c[kPerLane], r[kPerLane], x[kPerLane], b[kPerLane];
  uint32_t tc = 0, tr = 0, tx = 0, tb = 0;
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) c[j] = r[j] = x[j] = b[j] = 0u;
  const size_t at = (size_t)g * kRowStride + (size_t)lane * kPerLane;
  if (lane < kRowLanes) {
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
      c[j] = a.cur[at + j];
      r[j] = a.recent[at + j] + c[j] - (a.near_out ? a.near_out[at + j] : 0u);
      x[j] = a.leaves_gap ? a.near_slot[at + j] : 0u;
      b[j] = a.base[at + j];
      tc += c[j];
      tr += r[j];
      tx += x[j];
    }
  }
  const uint32_t n_x = __shfl(wave_scan(tx, lane), kWave - 1, kWave);
  const bool leaves = a.leaves_gap && n_x > 0u;
  const bool admit = leaves && !(prev & kSlow);
  uint32_t new_fill = fill;
  if (admit) {
    if (lane < kRowLanes) {
      uint32_t* ring = a.ring + (size_t)(pos % a.B) * a.ring_stride + at;
#pragma unroll
      for (int j = 0; j < kPerLane; ++j) {
        if (fill == a.B) b[j] -= ring[j];
        b[j] += x[j];
        ring[j] = x[j];
      }
    }
    if (fill < a.B) new_fill = fill + 1u;
  }
  if (lane < kRowLanes) {
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
      a.recent[at + j] = r[j];
      a.near_slot[at + j] = c[j];
      a.cur[at + j] = 0u;
      tb += b[j];
    }
  }
  const uint32_t ir = wave_scan(tr, lane), ib = wave_scan(tb, lane);
  const uint32_t n_win = __shfl(wave_scan(tc, lane), kWave - 1, kWave);
  const uint32_t n_r = __shfl(ir, kWave - 1, kWave), n_b = __shfl(ib, kWave - 1, kWave);
  // C_b(k) n_r - C_r(k) n_b and its mirror at this lane's buckets; the padding of a row adds nothing
  u64 cr = ir - tr, cb = ib - tb, ks = 0ull, kf = 0ull;
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    cr += r[j];
    cb += b[j];
    const u64 pb = cb * (u64)n_r, pr = cr * (u64)n_b;
    const uint32_t k = (uint32_t)(lane * kPerLane + j);
    if (pb > pr) {
      const u64 key = pack_max(pb - pr, k);
      ks = key > ks ? key : ks;
    } else if (pr > pb) {
      const u64 key = pack_max(pr - pb, k);
      kf = key > kf ? key : kf;
    }
  }
  ks = wave_max(ks);
  kf = wave_max(kf);
  const u64 slow_num = packed_num(ks), fast_num = packed_num(kf);
  uint32_t qr[kQuantiles], qb[kQuantiles];
#pragma unroll
  for (int q = 0; q < kQuantiles; ++q) {
    qr[q] = rank_bucket(r, ir, tr, n_r, lane, q);
    qb[q] = rank_bucket(b, ib, tb, n_b, lane, q);
  }
  uint32_t st = decide(n_r, n_b, new_fill, slow_num, fast_num, qr, qb, a.t);
  hold = (st & kSlow) ? hold + 1u : 0u;
  const bool rebase = hold >= a.hold_max;
  if (rebase) {
    st = kWarming | kRebased;
    hold = 0u;
  }
  if (lane < kRowLanes) {
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) a.base[at + j] = rebase ? 0u : b[j];
  }
  if (lane == 0) {
    w.prev[g] = st;
    w.hold[g] = hold;
    w.base_fill[g] = rebase ? 0u : new_fill;
    if (admit) w.base_pos[g] = pos + 1u;
    // the row as it was decided on: a rebased row still shows the baseline it dropped
    block[lay.n_win + g] = n_win;
    block[lay.n_recent + g] = n_r;
    block[lay.n_base + g] = n_b;
    block[lay.base_fill + g] = new_fill;
#pragma unroll
    for (int q = 0; q < kQuantiles; ++q) {
      block[lay.q_recent + (size_t)g * kQuantiles + q] = qr[q];
      block[lay.q_base + (size_t)g * kQuantiles + q] = qb[q];
    }
    block[lay.slow_num + 2 * (size_t)g] = (uint32_t)slow_num;
    block[lay.slow_num + 2 * (size_t)g + 1] = (uint32_t)(slow_num >> 32);
    block[lay.fast_num + 2 * (size_t)g] = (uint32_t)fast_num;
    block[lay.fast_num + 2 * (size_t)g + 1] = (uint32_t)(fast_num >> 32);
    block[lay.slow_at + g] = slow_num ? packed_bucket(ks) : kEmpty;
    block[lay.fast_at + g] = fast_num ? packed_bucket(kf) : kEmpty;
    block[lay.state + g] = st;
    block[lay.hold + g] = hold;
    if (admit) atomicAdd(&block[lay.stats + kAdmitted], 1u);
    if (leaves && !admit) atomicAdd(&block[lay.stats + kWithheld], 1u);
    if (rebase) atomicAdd(&block[lay.stats + kRebasedRows], 1u);
  }
}

}  // namespace
}  // namespace drift

using namespace drift;

DriftTracker::DriftTracker(const Config& cfg)
    : cfg_(cfg),
      lay_(layout(cfg.group_cap)),
      lane_("ttft drift", checked(cfg).device, cfg.n_buffers, cfg.span_cap, lay_.words, 1) {
  lane_.identify(drift::fingerprint(cfg));
  const size_t G = (size_t)cfg.group_cap;
  hist_ = lane_.zeroed<uint32_t>((size_t)state_rows(cfg) * G * kRowStride);
  words_ = lane_.zeroed<uint32_t>(4 * G);
  lane_.ready();
}

int64_t DriftTracker::step(const std::vector<Range>& spans, int n_groups) {
  check_step(n_groups, cfg_.group_cap);
  const size_t n = plan_ranges(spans, cfg_.span_cap);
  // nothing has changed up to here
  const auto [idx, s] = lane_.begin(spans);
  const hipStream_t st = lane_.stream();
  uint32_t* const blk = lane_.block();
  const int64_t R = cfg_.recent, near = R + cfg_.gap;
  const size_t G = (size_t)cfg_.group_cap;
  RollArgs a;
  a.recent = row((size_t)near);
  a.base = row((size_t)near + 1);
  a.cur = row((size_t)near + 2);
  a.ring = row((size_t)near + 3);
  a.ring_stride = G * kRowStride;
  a.near_out = idx >= R ? row((size_t)((idx - R) % near)) : nullptr;
  a.near_slot = row((size_t)(idx % near));
  a.B = (uint32_t)cfg_.baseline;
  a.hold_max = (uint32_t)cfg_.hold_max;
  a.leaves_gap = idx >= near ? 1 : 0;
  a.t = thresholds(cfg_);
  const Words w{words_, words_ + G, words_ + 2 * G, words_ + 3 * G};
  const dim3 block(kNT);
  if (n) {
    const dim3 og(grid_for((int64_t)n, kNT, 1024));
    uint32_t* stats = blk + lay_.stats;
    if (cfg_.lds)
      hipLaunchKernelGGL(k_drift_observe<true>, og, block, 0, st, lane_.spans(), (int)n, n_groups, a.cur, stats);
    else
      hipLaunchKernelGGL(k_drift_observe<false>, og, block, 0, st, lane_.spans(), (int)n, n_groups, a.cur, stats);
  }
  lane_.mark(s, StepLane::kObserved);
  hipLaunchKernelGGL(k_drift_roll, dim3(grid_for(cfg_.group_cap, kRowsPerBlock, 1 << 20)), block, 0, st, a, w, blk, lay_,
                     cfg_.group_cap);
  lane_.publish(s, 64);
  return idx;
}

std::vector<float> DriftTracker::step_ms(int64_t i) {
  return {lane_.ms(i, StepLane::kBegin, StepLane::kEnd), lane_.ms(i, StepLane::kCopied, StepLane::kEnd),
          lane_.ms(i, StepLane::kCopied, StepLane::kObserved)};
}

Resident DriftTracker::resident() {
  sync();
  const size_t G = (size_t)cfg_.group_cap, near = (size_t)cfg_.recent + (size_t)cfg_.gap;
  Resident out;
  out.pos = lane_.steps() % (int64_t)near;
  out.recent.resize(G * kRowStride);
  out.base.resize(G * kRowStride);
  out.base_fill.resize(G);
  out.base_pos.resize(G);
  out.hold.resize(G);
  HIPCHECK(hipMemcpy(out.recent.data(), row(near), out.recent.size() * 4, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(out.base.data(), row(near + 1), out.base.size() * 4, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(out.base_fill.data(), words_, G * 4, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(out.base_pos.data(), words_ + G, G * 4, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(out.hold.data(), words_ + 2 * G, G * 4, hipMemcpyDeviceToHost));
  return out;
}

}  // namespace mislo
