// Open-request tracker (openreq.h): the device table's kernels and the host class.
#include "openreq.h"

#include <algorithm>
#include <numeric>
#include <stdexcept>
#include <string>

namespace mislo {
namespace openreq {

namespace {

constexpr int kNT = 256;

// Words other workgroups write in the same launch (keys, states) are read and written with
// agent-scope atomics: a plain load may be served from this CU's L1. A stale key can only read as
// empty (keys are set once per step and cleared between launches), and an empty slot is always
// settled by the compare-and-swap.
__device__ __forceinline__ unsigned long long ld_key(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t ld_state(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_state(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The slot holding key h, or an empty slot claimed for it (claimed = true); -1 when neither
// turns up within kMaxProbes slots of the key's home.
__device__ __forceinline__ int64_t find_or_claim(const Table& tb, uint64_t mask, unsigned long long h, bool& claimed) {
  claimed = false;
  uint64_t s = splitmix64(h) & mask;
  for (int p = 0; p < kMaxProbes; ++p, s = (s + 1) & mask) {
    unsigned long long k = ld_key(tb.key + s);
    if (k == 0ull) {
      k = atomicCAS(tb.key + s, 0ull, h);
      if (k == 0ull) {
        claimed = true;
        return (int64_t)s;
      }
    }
    if (k == h) return (int64_t)s;
  }
  return -1;
}

__device__ __forceinline__ void flush_stats(const uint32_t* s_stats, uint32_t* stats) {
  for (int i = threadIdx.x; i < kStats; i += kNT)
    if (s_stats[i]) atomicAdd(&stats[i], s_stats[i]);
}

// Start records: absent -> OPEN; present -> counted as a duplicate, or as a start after its SLI
// when the entry is a marker. A key found in this launch's own insert reads state kEmpty or
// kOpen: a duplicate either way (markers were all written by earlier launches).
__global__ __launch_bounds__(kNT) void k_openreq_insert(const Span* __restrict__ sp, int n, Table tb, StepArgs a,
                                                        uint32_t* __restrict__ stats) {
  __shared__ uint32_t s_stats[kStats];
  for (int i = threadIdx.x; i < kStats; i += kNT) s_stats[i] = 0;
  __syncthreads();
  for (int i = blockIdx.x * kNT + threadIdx.x; i < n; i += gridDim.x * kNT) {
    const Span s = sp[i];
    if (!(s.flags & kSpanStart) || s.trace_h == 0 || s.group_id >= (uint32_t)a.n_groups || s.ts_ns <= 0) continue;
    atomicAdd(&s_stats[kStarts], 1u);
    bool claimed;
    const int64_t slot = find_or_claim(tb, a.mask, s.trace_h, claimed);
    if (slot < 0) {
      atomicAdd(&s_stats[kDroppedFull], 1u);
    } else if (claimed) {
      tb.t[slot] = s.ts_ns;
      tb.grp[slot] = s.group_id;
      st_state(tb.state + slot, kOpen);
    } else {
      atomicAdd(&s_stats[ld_state(tb.state + slot) == kResolved ? kStartAfterSli : kDupStart], 1u);
    }
  }
  __syncthreads();
  flush_stats(s_stats, stats);
}

// Records the engine counts (no kSpanStart, no kSpanNoSli): OPEN -> removed; COUNTED -> removed
// and the engine's count of this record un-counted (dup), classified as k_decode_spans does;
// absent -> a marker. Removal marks the entry kDead (the key stays until the sweep). A second
// counted record of one trace in the step finds kDead and leaves the marker the first would have
// left had they come in order.
__global__ __launch_bounds__(kNT) void k_openreq_resolve(const Span* __restrict__ sp, int n, Table tb, StepArgs a,
                                                         uint32_t* __restrict__ dup, uint32_t* __restrict__ stats) {
  __shared__ uint32_t s_stats[kStats];
  __shared__ uint32_t s_dup[3 * kLdsGroups];
  const bool lds = a.n_groups <= kLdsGroups;
  for (int i = threadIdx.x; i < kStats; i += kNT) s_stats[i] = 0;
  if (lds)
    for (int i = threadIdx.x; i < 3 * a.n_groups; i += kNT) s_dup[i] = 0;
  __syncthreads();
  uint32_t* cnt = lds ? s_dup : dup;
  for (int i = blockIdx.x * kNT + threadIdx.x; i < n; i += gridDim.x * kNT) {
    const Span s = sp[i];
    if ((s.flags & (kSpanStart | kSpanNoSli)) || s.trace_h == 0) continue;
    atomicAdd(&s_stats[kResolves], 1u);
    bool claimed;
    const int64_t slot = find_or_claim(tb, a.mask, s.trace_h, claimed);
    if (slot < 0) {
      atomicAdd(&s_stats[kMarkerDropped], 1u);
      continue;
    }
    if (claimed) {
      tb.t[slot] = a.cut_ns;
      tb.grp[slot] = s.group_id;
      st_state(tb.state + slot, kResolved);
      continue;
    }
    uint32_t st = ld_state(tb.state + slot);
    for (;;) {
      if (st == kOpen) {
        const uint32_t o = atomicCAS(tb.state + slot, (uint32_t)kOpen, (uint32_t)kDead);
        if (o == kOpen) break;
        st = o;
      } else if (st == kCounted) {
        const uint32_t o = atomicCAS(tb.state + slot, (uint32_t)kCounted, (uint32_t)kDead);
        if (o == kCounted) {
          const bool breach = s.ttft_ms > a.slo_ms;
          const uint32_t g = s.group_id;
          if (g < (uint32_t)a.n_groups) {  // the engine counted it in this group
            if (breach && (s.flags & kSpanLate)) {
              atomicAdd(&cnt[3 * g + 2], 1u);
            } else {
              atomicAdd(&cnt[3 * g], 1u);
              if (breach) atomicAdd(&cnt[3 * g + 1], 1u);
            }
          }
          if (!breach) atomicAdd(&s_stats[kFalseDeadline], 1u);
          break;
        }
        st = o;
      } else if (st == kDead) {
        const uint32_t o = atomicCAS(tb.state + slot, (uint32_t)kDead, (uint32_t)kResolved);
        if (o == kDead) {
          tb.t[slot] = a.cut_ns;
          break;
        }
        st = o;
      } else {
        break;  // a marker (kResolved, or kEmpty: being written by this launch) stays
      }
    }
  }
  __syncthreads();
  flush_stats(s_stats, stats);
  if (lds)
    for (int i = threadIdx.x; i < 3 * a.n_groups; i += kNT)
      if (s_dup[i]) atomicAdd(&dup[i], s_dup[i]);
}

// The deadline pass and the move into the other table, one read of `cur`: every non-empty slot
// is cleared behind it (nobody probes `cur` in this launch), the survivors are claimed in `nxt`
// (distinct keys: every probe ends in a claim).
__global__ __launch_bounds__(kNT) void k_openreq_sweep(Table cur, Table nxt, int64_t cap, StepArgs a,
                                                       uint32_t* __restrict__ dl, uint32_t* __restrict__ stats) {
  __shared__ uint32_t s_stats[kStats];
  __shared__ uint32_t s_dl[2 * kLdsGroups];
  const bool lds = a.n_groups <= kLdsGroups;
  for (int i = threadIdx.x; i < kStats; i += kNT) s_stats[i] = 0;
  if (lds)
    for (int i = threadIdx.x; i < 2 * a.n_groups; i += kNT) s_dl[i] = 0;
  __syncthreads();
  uint32_t* cnt = lds ? s_dl : dl;
  for (int64_t i = blockIdx.x * (int64_t)kNT + threadIdx.x; i < cap; i += (int64_t)gridDim.x * kNT) {
    const unsigned long long k = cur.key[i];
    if (k == 0ull) continue;
    uint32_t st = cur.state[i];
    const int64_t t = cur.t[i];
    const uint32_t g = cur.grp[i];
    cur.key[i] = 0ull;
    cur.state[i] = kEmpty;
    if (st == kOpen) {
      if (t + a.slo_ns < a.cut_ns) {
        if (g < (uint32_t)a.n_groups) atomicAdd(&cnt[2 * g + (t + a.slo_ns >= a.prev_cut_ns ? 0 : 1)], 1u);
        st = kCounted;
      }
    } else if (st == kCounted) {
      if (a.cut_ns - t >= a.ttl_ns) {
        atomicAdd(&s_stats[kExpired], 1u);
        st = kDead;
      }
    } else if (st == kResolved) {
      if (a.cut_ns - t >= a.reorder_ns) st = kDead;
    }
    if (st != kOpen && st != kCounted && st != kResolved) continue;
    bool claimed;
    const int64_t slot = find_or_claim(nxt, a.mask, k, claimed);
    if (slot < 0 || !claimed) {
      atomicAdd(&s_stats[kDroppedFull], 1u);
      continue;
    }
    nxt.t[slot] = t;
    nxt.grp[slot] = g;
    nxt.state[slot] = st;
    atomicAdd(&s_stats[kLiveOpen + (int)st - (int)kOpen], 1u);
  }
  __syncthreads();
  flush_stats(s_stats, stats);
  if (lds)
    for (int i = threadIdx.x; i < 2 * a.n_groups; i += kNT)
      if (s_dl[i]) atomicAdd(&dl[i], s_dl[i]);
}

}  // namespace

static_assert(kLiveCounted == kLiveOpen + 1 && kLiveResolved == kLiveOpen + 2 && kCounted == kOpen + 1 &&
                  kResolved == kOpen + 2,
              "live counts are indexed by state");

void launch_insert(const Span* sp, int n, Table tb, StepArgs a, uint32_t* stats, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_openreq_insert, dim3(grid_for(n, kNT, 1024)), dim3(kNT), 0, st, sp, n, tb, a, stats);
}

void launch_resolve(const Span* sp, int n, Table tb, StepArgs a, uint32_t* dup, uint32_t* stats, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_openreq_resolve, dim3(grid_for(n, kNT, 1024)), dim3(kNT), 0, st, sp, n, tb, a, dup, stats);
}

void launch_sweep(Table cur, Table nxt, int64_t cap, StepArgs a, uint32_t* dl, uint32_t* stats, hipStream_t st) {
  hipLaunchKernelGGL(k_openreq_sweep, dim3(grid_for(cap, kNT, 2048)), dim3(kNT), 0, st, cur, nxt, cap, a, dl, stats);
}

}  // namespace openreq

using namespace openreq;

OpenRequests::OpenRequests(const Config& cfg)
    : cfg_(cfg),
      lay_(layout(cfg.group_cap)),
      lane_("open-request", checked(cfg).device, cfg.n_buffers, cfg.span_cap, lay_.words, 0) {
  lane_.identify(openreq::fingerprint(cfg), 1);
  const size_t cap = (size_t)cfg.cap;
  for (Table& tb : tb_) {
    tb.key = lane_.zeroed<unsigned long long>(cap);
    tb.t = lane_.zeroed<int64_t>(cap);
    tb.grp = lane_.zeroed<uint32_t>(cap);
    tb.state = lane_.zeroed<uint32_t>(cap);
  }
  lane_.ready();
}

int64_t OpenRequests::step(const std::vector<Range>& spans, int64_t cut_ns, int64_t prev_cut_ns, int n_groups) {
  check_step(cut_ns, prev_cut_ns, n_groups, cfg_.group_cap);
  const size_t n = plan_ranges(spans, cfg_.span_cap);
  const auto [idx, s] = lane_.begin(spans);
  const hipStream_t st = lane_.stream();
  StepArgs a;
  a.cut_ns = cut_ns;
  a.prev_cut_ns = prev_cut_ns;
  a.slo_ns = ms_to_ns(cfg_.slo_ms);
  a.ttl_ns = ms_to_ns(cfg_.ttl_ms);
  a.reorder_ns = ms_to_ns(cfg_.reorder_ms);
  a.slo_ms = (float)cfg_.slo_ms;
  a.n_groups = n_groups;
  a.mask = (uint64_t)cfg_.cap - 1;
  uint32_t* c = lane_.block();
  const Table cur = tb_[cur_], nxt = tb_[cur_ ^ 1];
  launch_insert(lane_.spans(), (int)n, cur, a, c + lay_.stats, st);
  launch_resolve(lane_.spans(), (int)n, cur, a, c + lay_.dup, c + lay_.stats, st);
  launch_sweep(cur, nxt, cfg_.cap, a, c + lay_.dl, c + lay_.stats, st);
  lane_.publish(s, 64);
  cur_ ^= 1;
  return idx;
}

std::pair<float, float> OpenRequests::step_ms(int64_t i) {
  return {lane_.ms(i, StepLane::kBegin, StepLane::kEnd), lane_.ms(i, StepLane::kCopied, StepLane::kEnd)};
}

void OpenRequests::entries(std::vector<uint64_t>& key, std::vector<int64_t>& t, std::vector<uint32_t>& grp,
                           std::vector<uint32_t>& state) {
  sync();
  const size_t cap = (size_t)cfg_.cap;
  std::vector<uint64_t> k(cap);
  std::vector<int64_t> tt(cap);
  std::vector<uint32_t> g(cap), s(cap);
  const Table& tb = tb_[cur_];
  HIPCHECK(hipMemcpy(k.data(), tb.key, cap * 8, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(tt.data(), tb.t, cap * 8, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(g.data(), tb.grp, cap * 4, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(s.data(), tb.state, cap * 4, hipMemcpyDeviceToHost));
  std::vector<size_t> live;
  for (size_t i = 0; i < cap; ++i)
    if (k[i] != 0) live.push_back(i);
  std::sort(live.begin(), live.end(), [&](size_t x, size_t y) { return k[x] < k[y]; });
  key.clear(), t.clear(), grp.clear(), state.clear();
  for (size_t i : live) {
    key.push_back(k[i]);
    t.push_back(tt[i]);
    grp.push_back(g[i]);
    state.push_back(s[i]);
  }
}

}  // namespace mislo
