// Per-pod TTFT breach breakdown (podrank.h): the kernels and the host class.
#include "podrank.h"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace mislo {
namespace podrank {

namespace {

constexpr int kNT = 256;
constexpr int kWave = 64;
constexpr int kRowsPerBlock = kNT / kWave;

static_assert(kLdsSlots == kNT, "observe flushes its LDS table one slot per thread");
static_assert(2 * kMaxK <= 32, "gather: the window's keys in lanes 0.., the recent ones in lanes 32..");

using u64 = unsigned long long;

__device__ __forceinline__ u64 load_key(const u64* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Insert-or-add of one pair's (n, b, max, sum) into an open-addressing table of mask + 1 slots:
// a slot is claimed by a 64-bit compare-and-swap, then linear probing; keys never leave a table
// within a step, so a probe chain only grows. kCapped (the window's table): `claimed` counts the
// slots taken, and an empty slot is not claimed once it has reached pair_cap. The count is read
// before the slot is read again: with at most pair_cap distinct pairs in the window, a count at
// pair_cap means every pair has its slot already, so a slot that still reads empty proves this pair
// is missing, which cannot be; the refusal therefore only happens past the capacity. Returns false
// when the pair found no place (the caller counts the records in kPairOverflow).
template <bool kCapped>
__device__ __forceinline__ bool pair_add(const Pairs& t, uint32_t mask, u64 key, uint32_t n, uint32_t b, uint32_t mx,
                                         u64 sum, uint32_t* claimed, uint32_t pair_cap) {
  uint32_t s = (uint32_t)(fmix64(key) & (u64)mask);
  for (uint32_t probe = 0; probe <= mask; ++probe, s = (s + 1u) & mask) {
    u64 k = load_key(t.key + s);
    if (k == 0ull) {
      if (kCapped && __hip_atomic_load(claimed, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) >= pair_cap) {
        k = load_key(t.key + s);
        if (k == 0ull) return false;
      } else {
        k = atomicCAS(t.key + s, 0ull, key);
        if (k == 0ull) {
          if (kCapped) atomicAdd(claimed, 1u);
          k = key;
        }
      }
    }
    if (k == key) {
      atomicAdd(t.n + s, n);
      if (b) atomicAdd(t.b + s, b);
      atomicMax(t.max + s, mx);
      atomicAdd(t.sum + s, sum);
      return true;
    }
  }
  return false;
}

// the slot of `key` in a table, or mask + 1 when it is not there
__device__ __forceinline__ uint32_t pair_find(const u64* keys, uint32_t mask, u64 key) {
  uint32_t s = (uint32_t)(fmix64(key) & (u64)mask);
  for (uint32_t probe = 0; probe <= mask; ++probe, s = (s + 1u) & mask) {
    const u64 k = keys[s];
    if (k == key) return s;
    if (k == 0ull) break;
  }
  return mask + 1u;
}

// One thread per record: the records k_decode_spans counts (no kSpanNoSli, a group below n_groups)
// with a TTFT >= 0 (NaN and negatives fail the compare) add to their service's totals and, with a
// pod below 2^20, to their (service, pod) pair. With kLds the workgroup aggregates its pairs in an
// LDS table of kLdsSlots, and the totals of the services below kLdsGroups in LDS counters, and sends
// each to global memory once: a hot pair or a hot service costs one global atomic per workgroup and
// field, not one per record. A record that finds no LDS slot within kLdsProbes goes to the global
// table itself. Block 0 resets the length of the horizon list this step refills.
template <bool kLds>
__global__ __launch_bounds__(kNT) void k_podrank_observe(const Span* __restrict__ sp, int n, int n_groups, float slo,
                                                         Pairs win, uint32_t wmask, uint32_t pair_cap,
                                                         uint32_t* __restrict__ ctrl, int cur, uint32_t* __restrict__ tot,
                                                         int group_cap, uint32_t* __restrict__ stats) {
  __shared__ u64 s_key[kLds ? kLdsSlots : 1];
  __shared__ u64 s_sum[kLds ? kLdsSlots : 1];
  __shared__ uint32_t s_n[kLds ? kLdsSlots : 1], s_b[kLds ? kLdsSlots : 1], s_max[kLds ? kLdsSlots : 1];
  __shared__ uint32_t s_tot[kLds ? 2 * kLdsGroups : 1];
  __shared__ uint32_t s_stats[kStats];
  const uint32_t lg = kLds ? (uint32_t)min(n_groups, kLdsGroups) : 0u;  // services counted in LDS
  if (kLds) {
    s_key[threadIdx.x] = 0ull, s_sum[threadIdx.x] = 0ull;
    s_n[threadIdx.x] = 0u, s_b[threadIdx.x] = 0u, s_max[threadIdx.x] = 0u;
    if (threadIdx.x < 2 * kLdsGroups) s_tot[threadIdx.x] = 0u;
  }
  if (threadIdx.x < kStats) s_stats[threadIdx.x] = 0u;
  if (blockIdx.x == 0 && threadIdx.x == 0) ctrl[1 + cur] = 0u;
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
    const uint32_t pod = sp[i].pod_id;
    const uint32_t breach = v > slo ? 1u : 0u;
    if (g < lg) {
      atomicAdd(&s_tot[g], 1u);
      if (breach) atomicAdd(&s_tot[kLdsGroups + g], 1u);
    } else {  // g < n_groups <= group_cap
      atomicAdd(&tot[g], 1u);
      if (breach) atomicAdd(&tot[group_cap + g], 1u);
    }
    if (pod >= kPodLimit) {
      atomicAdd(&s_stats[kPodOutOfRange], 1u);
      continue;
    }
    const u64 key = pair_key(g, pod);
    const uint32_t mx = ord_of_bits(__float_as_uint(v));
    const u64 milli = milli_units(fminf(v, kMaxMs));
    bool done = false;
    if (kLds) {
      uint32_t s = (uint32_t)(fmix64(key) >> 32) & (kLdsSlots - 1);
      for (int probe = 0; probe < kLdsProbes && !done; ++probe, s = (s + 1u) & (kLdsSlots - 1)) {
        u64 k = __hip_atomic_load(&s_key[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (k == 0ull) {
          k = atomicCAS(&s_key[s], 0ull, key);
          if (k == 0ull) k = key;
        }
        if (k == key) {
          atomicAdd(&s_n[s], 1u);
          if (breach) atomicAdd(&s_b[s], 1u);
          atomicMax(&s_max[s], mx);
          atomicAdd(&s_sum[s], milli);
          done = true;
        }
      }
    }
    if (!done) {
      if (!pair_add<true>(win, wmask, key, 1u, breach, mx, milli, ctrl, pair_cap)) atomicAdd(&s_stats[kPairOverflow], 1u);
    }
  }
  __syncthreads();
  if (kLds) {
    const u64 key = s_key[threadIdx.x];
    if (key != 0ull) {
      const uint32_t pn = s_n[threadIdx.x];
      if (!pair_add<true>(win, wmask, key, pn, s_b[threadIdx.x], s_max[threadIdx.x], s_sum[threadIdx.x], ctrl, pair_cap))
        atomicAdd(&s_stats[kPairOverflow], pn);
    }
    if (threadIdx.x < lg) {
      const uint32_t tn = s_tot[threadIdx.x], tb = s_tot[kLdsGroups + threadIdx.x];
      if (tn) atomicAdd(&tot[threadIdx.x], tn);
      if (tb) atomicAdd(&tot[group_cap + threadIdx.x], tb);
    }
    __syncthreads();
  }
  if (threadIdx.x < kStats && s_stats[threadIdx.x]) atomicAdd(&stats[threadIdx.x], s_stats[threadIdx.x]);
}

// Concurrent insertion into K sorted slots (exemplars.hip topk_insert): each atomicMax keeps the
// larger of (slot, key) in the slot and the smaller carries on down, so the final slots are the K
// largest keys in order whatever the arrival order.
__device__ __forceinline__ void topk_insert(u64* slot, int K, u64 key) {
  if (key <= __atomic_load_n(slot + K - 1, __ATOMIC_RELAXED)) return;
  for (int j = 0; j < K; ++j) {
    const u64 old = atomicMax(slot + j, key);
    if (old == 0ull) return;
    key = old < key ? old : key;
  }
}

// One thread per slot of a pair table: an occupied slot counts as a pod of its service (and as a
// breaching one with b >= 1, whose rank key cascades into the service's K slots). For the window's
// table (list.key != nullptr) the pair is first appended to the horizon's list `cur`, one counter add
// per wave; a pair past pair_cap is left out of the list, the counts and the ranking, and its
// records go to kPairOverflow. The counts and K slots of the services below kLdsGroups are
// privatised per workgroup in LDS (exemplars.hip's select does the same), whose survivors go to the
// global slots by the same cascade: a service with thousands of pods does not send every pair to
// the same K + 2 global words. Thread 0 resets the window table's claim count for the next step.
__global__ __launch_bounds__(kNT) void k_podrank_rank(Pairs t, uint32_t slots, u64* __restrict__ top, int K,
                                                      uint32_t* __restrict__ pods, uint32_t* __restrict__ pods_b,
                                                      Pairs list, uint32_t* __restrict__ ctrl, int cur, uint32_t pair_cap,
                                                      int group_cap, uint32_t* __restrict__ stats) {
  __shared__ u64 s_top[kLdsGroups * kMaxK];
  __shared__ uint32_t s_pods[2 * kLdsGroups];
  const bool append = list.key != nullptr;
  const int lane = threadIdx.x & (kWave - 1);
  const int lg = min(group_cap, kLdsGroups);  // services in LDS
  for (int i = threadIdx.x; i < lg * K; i += kNT) s_top[i] = 0ull;
  if (threadIdx.x < 2 * kLdsGroups) s_pods[threadIdx.x] = 0u;
  if (append && blockIdx.x == 0 && threadIdx.x == 0) ctrl[0] = 0u;
  __syncthreads();
  // every thread of a block makes the same number of turns, so the ballots see whole waves
  for (size_t base = blockIdx.x * (size_t)kNT; base < (size_t)slots; base += (size_t)gridDim.x * kNT) {
    const size_t i = base + threadIdx.x;
    const u64 key = i < (size_t)slots ? t.key[i] : 0ull;
    bool occ = key != 0ull;
    uint32_t n = 0u, b = 0u;
    if (occ) n = t.n[i], b = t.b[i];
    if (append) {
      const u64 m = __ballot(occ);
      if (m != 0ull) {
        const int leader = __ffsll(m) - 1;
        uint32_t first = 0u;
        if (lane == leader) first = atomicAdd(&ctrl[1 + cur], (uint32_t)__popcll(m));
        first = __shfl(first, leader);
        if (occ) {
          const uint32_t pos = first + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
          if (pos < pair_cap) {
            const size_t at = (size_t)cur * pair_cap + pos;
            list.key[at] = key, list.n[at] = n, list.b[at] = b, list.max[at] = t.max[i], list.sum[at] = t.sum[i];
          } else {
            atomicAdd(&stats[kPairOverflow], n);
            occ = false;  // stays in the table (probe chains stay whole) but is never ranked, so never gathered
          }
        }
      }
    }
    if (occ) {
      const uint32_t g = group_of_pair(key);  // below the group_cap of the step that inserted it
      const u64 rk = b ? rank_key(b, n, pod_of_pair(key)) : 0ull;
      if ((int)g < lg) {
        atomicAdd(&s_pods[g], 1u);
        if (b) {
          atomicAdd(&s_pods[kLdsGroups + g], 1u);
          topk_insert(s_top + g * K, K, rk);
        }
      } else {
        atomicAdd(&pods[g], 1u);
        if (b) {
          atomicAdd(&pods_b[g], 1u);
          topk_insert(top + (size_t)g * K, K, rk);
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < lg * K; i += kNT) {
    const u64 rk = s_top[i];
    if (rk) topk_insert(top + (size_t)(i / K) * K, K, rk);
  }
  if ((int)threadIdx.x < lg) {
    const uint32_t p = s_pods[threadIdx.x], pb = s_pods[kLdsGroups + threadIdx.x];
    if (p) atomicAdd(&pods[threadIdx.x], p);
    if (pb) atomicAdd(&pods_b[threadIdx.x], pb);
  }
}

// One thread per entry of the horizon's H lists: insert or add into the recent table, which holds
// every list's pairs at a load of one half at most, so it cannot overflow.
__global__ __launch_bounds__(kNT) void k_podrank_roll(Pairs list, const uint32_t* __restrict__ ctrl, int H,
                                                      uint32_t pair_cap, Pairs rec, uint32_t rmask) {
  const size_t total = (size_t)H * pair_cap;
  for (size_t i = blockIdx.x * (size_t)kNT + threadIdx.x; i < total; i += (size_t)gridDim.x * kNT) {
    const uint32_t h = (uint32_t)(i / pair_cap), j = (uint32_t)(i - (size_t)h * pair_cap);
    if (j >= min(ctrl[1 + h], pair_cap)) continue;
    pair_add<false>(rec, rmask, list.key[i], list.n[i], list.b[i], list.max[i], list.sum[i], nullptr, 0u);
  }
}

// One wave per service row, every row of group_cap (so a service absent from the step still ages):
// lanes 0..K-1 turn the window's rank keys into rows, lanes 32..32+K-1 the recent ones, by probing
// the scope's table for (service, pod); lane 0 moves the step's totals into the horizon's slot `cur`
// and writes the window's and the horizon's n / b. The key slots and totals are cleared.
__global__ __launch_bounds__(kNT) void k_podrank_gather(Pairs win, uint32_t wmask, Pairs rec, uint32_t rmask,
                                                        u64* __restrict__ top, uint32_t* __restrict__ tot,
                                                        uint32_t* __restrict__ hist, uint32_t* __restrict__ block,
                                                        Layout lay, int group_cap, int K, int H, int cur) {
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
  const int g = blockIdx.x * kRowsPerBlock + w;
  if (g >= group_cap) return;  // the whole wave; no barrier below
  const int sc = lane >> 5, j = lane & 31;
  bool found = false;
  if (j < K) {
    const size_t at = ((size_t)sc * group_cap + g) * K + j;
    const u64 rk = top[at];
    top[at] = 0ull;
    if (rk != 0ull) {
      const Pairs& t = sc ? rec : win;
      const uint32_t mask = sc ? rmask : wmask, pod = pod_of_rank(rk);
      const uint32_t s = pair_find(t.key, mask, pair_key((uint32_t)g, pod));
      if (s <= mask) {
        const u64 sum = t.sum[s];
        uint4* row = reinterpret_cast<uint4*>(block + lay.top[sc]) + ((size_t)g * K + j) * 2;
        row[0] = make_uint4(pod, t.n[s], t.b[s], t.max[s]);
        row[1] = make_uint4((uint32_t)sum, (uint32_t)(sum >> 32), 0u, 0u);
        found = true;
      }
    }
  }
  const u64 m = __ballot(found);
  if (j == 0) block[lay.k_top[sc] + g] = (uint32_t)__popcll(sc ? (m >> 32) : (m & 0xffffffffull));
  if (lane < 2) {  // lane 0: requests, lane 1: breaches
    const size_t at = (size_t)lane * group_cap + g;
    const uint32_t v = tot[at];
    tot[at] = 0u;
    hist[(size_t)cur * 2 * group_cap + at] = v;
    uint32_t all = 0u;
    for (int h = 0; h < H; ++h) all += hist[(size_t)h * 2 * group_cap + at];
    block[(lane ? lay.b[0] : lay.n[0]) + g] = v;
    block[(lane ? lay.b[1] : lay.n[1]) + g] = all;
  }
}

// the step's result block into its pinned host block; the block and both tables cleared for the next step
__global__ __launch_bounds__(kNT) void k_podrank_publish(uint4* __restrict__ block, uint4* __restrict__ host, size_t n16,
                                                         Pairs win, uint32_t wslots, Pairs rec, uint32_t rslots) {
  const size_t first = blockIdx.x * (size_t)kNT + threadIdx.x, stride = (size_t)gridDim.x * kNT;
  for (size_t i = first; i < n16; i += stride) {
    host[i] = block[i];
    block[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  for (size_t i = first; i < (size_t)wslots; i += stride)
    win.key[i] = 0ull, win.n[i] = 0u, win.b[i] = 0u, win.max[i] = 0u, win.sum[i] = 0ull;
  for (size_t i = first; i < (size_t)rslots; i += stride)
    rec.key[i] = 0ull, rec.n[i] = 0u, rec.b[i] = 0u, rec.max[i] = 0u, rec.sum[i] = 0ull;
}

}  // namespace
}  // namespace podrank

using namespace podrank;

Pairs PodRankTracker::zeroed_pairs(size_t n) {
  Pairs p;
  p.key = lane_.zeroed<unsigned long long>(n);
  p.sum = lane_.zeroed<unsigned long long>(n);
  p.n = lane_.zeroed<uint32_t>(n);
  p.b = lane_.zeroed<uint32_t>(n);
  p.max = lane_.zeroed<uint32_t>(n);
  return p;
}

PodRankTracker::PodRankTracker(const Config& cfg)
    : cfg_(cfg),
      lay_(layout(cfg.group_cap, cfg.k)),
      lane_("pod breakdown", checked(cfg).device, cfg.n_buffers, cfg.span_cap, lay_.words, 1) {
  lane_.identify(podrank::fingerprint(cfg));
  wslots_ = window_slots(cfg), rslots_ = recent_slots(cfg);
  const size_t G = (size_t)cfg.group_cap, K = (size_t)cfg.k, H = (size_t)cfg.windows;
  win_ = zeroed_pairs(wslots_);
  rec_ = zeroed_pairs(rslots_);
  lists_ = zeroed_pairs(H * (size_t)cfg.pair_cap);
  ctrl_ = lane_.zeroed<uint32_t>(1 + H);
  tot_ = lane_.zeroed<uint32_t>(2 * G);
  hist_ = lane_.zeroed<uint32_t>(H * 2 * G);
  top_ = lane_.zeroed<unsigned long long>(2 * G * K);
  lane_.ready();
}

int64_t PodRankTracker::step(const std::vector<Range>& spans, int n_groups) {
  check_step(n_groups, cfg_.group_cap);
  const size_t n = plan_ranges(spans, cfg_.span_cap);
  const auto [idx, s] = lane_.begin(spans);
  const hipStream_t st = lane_.stream();
  uint32_t* const blk = lane_.block();
  const int G = cfg_.group_cap, K = cfg_.k, H = cfg_.windows, cur = (int)(idx % (int64_t)H);
  const uint32_t cap = (uint32_t)cfg_.pair_cap, wmask = wslots_ - 1u, rmask = rslots_ - 1u;
  uint32_t* stats = blk + lay_.stats;
  u64* wtop = top_;
  u64* rtop = top_ + (size_t)G * K;
  // an empty step still launches: block 0 resets the list this step refills
  const dim3 block(kNT), og(grid_for((int64_t)n, kNT, 1024));
  const float slo = (float)cfg_.slo_ms;
  if (cfg_.lds)
    hipLaunchKernelGGL(k_podrank_observe<true>, og, block, 0, st, lane_.spans(), (int)n, n_groups, slo, win_, wmask, cap,
                       ctrl_, cur, tot_, G, stats);
  else
    hipLaunchKernelGGL(k_podrank_observe<false>, og, block, 0, st, lane_.spans(), (int)n, n_groups, slo, win_, wmask, cap,
                       ctrl_, cur, tot_, G, stats);
  lane_.mark(s, StepLane::kObserved);
  hipLaunchKernelGGL(k_podrank_rank, dim3(grid_for(wslots_, kNT, 1024)), block, 0, st, win_, wslots_, wtop, K,
                     blk + lay_.pods[0], blk + lay_.pods_b[0], lists_, ctrl_, cur, cap, G, stats);
  hipLaunchKernelGGL(k_podrank_roll, dim3(grid_for((int64_t)H * cap, kNT, 1024)), block, 0, st, lists_, ctrl_, H, cap, rec_,
                     rmask);
  hipLaunchKernelGGL(k_podrank_rank, dim3(grid_for(rslots_, kNT, 1024)), block, 0, st, rec_, rslots_, rtop, K,
                     blk + lay_.pods[1], blk + lay_.pods_b[1], Pairs(), ctrl_, cur, cap, G, stats);
  hipLaunchKernelGGL(k_podrank_gather, dim3(grid_for(G, kRowsPerBlock, 1 << 20)), block, 0, st, win_, wmask, rec_, rmask,
                     top_, tot_, hist_, blk, lay_, G, K, H, cur);
  const size_t n16 = lay_.words / 4;
  hipLaunchKernelGGL(k_podrank_publish, dim3(grid_for((int64_t)std::max<size_t>(n16, rslots_), kNT, 1024)), block, 0, st,
                     reinterpret_cast<uint4*>(blk), reinterpret_cast<uint4*>(lane_.host(s)), n16, win_, wslots_, rec_, rslots_);
  lane_.finish(s);
  return idx;
}

std::vector<float> PodRankTracker::step_ms(int64_t i) {
  return {lane_.ms(i, StepLane::kBegin, StepLane::kEnd), lane_.ms(i, StepLane::kCopied, StepLane::kEnd),
          lane_.ms(i, StepLane::kCopied, StepLane::kObserved)};
}

std::vector<PairList> PodRankTracker::resident() {
  const size_t H = (size_t)cfg_.windows, cap = (size_t)cfg_.pair_cap;
  sync();
  std::vector<uint32_t> ctrl(1 + H);
  HIPCHECK(hipMemcpy(ctrl.data(), ctrl_, ctrl.size() * 4, hipMemcpyDeviceToHost));
  std::vector<PairList> out(H);
  for (size_t h = 0; h < H; ++h) {
    const size_t len = std::min<size_t>(ctrl[1 + h], cap), at = h * cap;
    PairList& l = out[h];
    l.key.resize(len), l.sum.resize(len), l.n.resize(len), l.b.resize(len), l.max.resize(len);
    if (!len) continue;
    HIPCHECK(hipMemcpy(l.key.data(), lists_.key + at, len * 8, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(l.sum.data(), lists_.sum + at, len * 8, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(l.n.data(), lists_.n + at, len * 4, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(l.b.data(), lists_.b + at, len * 4, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(l.max.data(), lists_.max + at, len * 4, hipMemcpyDeviceToHost));
  }
  return out;
}

}  // namespace mislo
