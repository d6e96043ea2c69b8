// Request exemplars (exemplars.h): the kernels and the host class.
#include "exemplars.h"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace mislo {
namespace exemplars {

namespace {

constexpr int kNT = 256;
constexpr int kWave = 64;
constexpr int kRowsPerBlock = kNT / kWave;
constexpr int kTtftWord = 6;  // Row::ttft_ms, in words

static_assert(kMaxH * kMaxK <= 2 * kWave, "the horizon's candidates are two per lane of one wave");
static_assert(offsetof(Row, ttft_ms) == 4 * kTtftWord && offsetof(Row, age) == 48, "row layout");

using u64 = unsigned long long;

// Concurrent insertion into K sorted slots (join.hip top3_insert, by maximum): each atomicMax keeps
// the larger of (slot, key) in the slot and the smaller carries on down; the multiset is preserved
// and every slot only grows, so the final slots are the K largest keys in order whatever the arrival
// order. A key at or below the last slot cannot enter: the slot only grows, so a stale read is safe.
__device__ __forceinline__ void topk_insert(u64* slot, int K, u64 key) {
  if (key <= __atomic_load_n(slot + K - 1, __ATOMIC_RELAXED)) return;
  for (int j = 0; j < K; ++j) {
    const u64 old = atomicMax(slot + j, key);
    if (old == 0ull) return;  // the slot was empty, and so is every slot below it
    key = old < key ? old : key;
  }
}

// One thread per record: the records k_decode_spans counts (no kSpanNoSli, a group below n_groups)
// with a TTFT >= 0 (NaN and negatives fail the compare) compete for their group's K slots. With
// kLds the groups below kLdsGroups are privatised per workgroup, whose survivors go to the global
// slots by the same cascade: a window of a few services does not send every record to the same K
// global words.
template <bool kLds>
__global__ __launch_bounds__(kNT) void k_exemplar_select(const Span* __restrict__ sp, int n, int n_groups, int K,
                                                         u64* __restrict__ keys, uint32_t* __restrict__ count,
                                                         uint32_t* __restrict__ stats) {
  __shared__ u64 s_keys[kLds ? kLdsGroups * kMaxK : 1];
  __shared__ uint32_t s_count[kLds ? kLdsGroups : 1];
  __shared__ uint32_t s_stats[kStats];
  const int lg = kLds ? min(n_groups, kLdsGroups) : 0;  // groups in LDS
  for (int t = threadIdx.x; t < lg * K; t += kNT) s_keys[t] = 0ull;
  for (int t = threadIdx.x; t < lg; t += kNT) s_count[t] = 0u;
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
    const u64 key = window_key(__float_as_uint(v), (uint32_t)i);
    if ((int)g < lg) {
      atomicAdd(&s_count[g], 1u);
      topk_insert(s_keys + g * K, K, key);
    } else {  // g < n_groups <= group_cap
      atomicAdd(&count[g], 1u);
      topk_insert(keys + (size_t)g * K, K, key);
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < lg * K; t += kNT) {
    const u64 key = s_keys[t];
    if (key) topk_insert(keys + (size_t)(t / K) * K, K, key);
  }
  for (int t = threadIdx.x; t < lg; t += kNT)
    if (s_count[t]) atomicAdd(&count[t], s_count[t]);
  if (threadIdx.x < kStats && s_stats[threadIdx.x]) atomicAdd(&stats[threadIdx.x], s_stats[threadIdx.x]);
}

// One wave per service row, every row of group_cap (so a service absent from the step still ages):
// lanes < K turn the window's keys into rows (four 16-byte loads of the record) and store them in
// the horizon's slot `cur` and the block's `win`; then the wave ranks the H * K candidates of the
// resident slots by recent_key, two per lane through an LDS table, and the candidates of rank < K
// write `recent` with their age. The step's key slots and count are cleared for the next step.
__global__ __launch_bounds__(kNT) void k_exemplar_merge(const Span* __restrict__ sp, int n, u64* __restrict__ keys,
                                                        uint32_t* __restrict__ count, Row* __restrict__ horizon,
                                                        uint32_t* __restrict__ held, uint32_t* __restrict__ block,
                                                        Layout lay, int group_cap, int K, int H, int cur) {
  __shared__ uint4 s_row[kRowsPerBlock][kMaxK][4];
  __shared__ u64 s_ck[kRowsPerBlock][2 * kWave];
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
  const int g = blockIdx.x * kRowsPerBlock + w;
  const bool live = g < group_cap;  // the whole wave; every wave reaches the barriers
  u64 key = 0ull;
  if (live && lane < K) {
    const size_t at = (size_t)g * K + lane;
    key = keys[at];
    keys[at] = 0ull;
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    uint4 r0 = z, r1 = z, r2 = z, r3 = z;
    const uint32_t idx = index_of_key(key);
    if (key != 0ull && idx < (uint32_t)n) {
      const uint4* s = reinterpret_cast<const uint4*>(sp + idx);
      const uint4 a = s[0], b = s[1], c = s[2], d = s[3];
      r0 = a;                                  // ts_ns, trace_h
      r1 = make_uint4(d.x, d.y, c.z, c.w);     // span_h, ttft_ms, latency_ms
      r2 = make_uint4(d.z, b.w, b.z, d.w);     // retr_ms, pod_id, pid, flags
      r3 = make_uint4(0u, idx, 0u, 0u);        // age, index, pad
    } else {
      key = 0ull;
    }
    uint4* hz = reinterpret_cast<uint4*>(horizon + ((size_t)cur * group_cap + g) * K + lane);
    uint4* bw = reinterpret_cast<uint4*>(block + lay.win) + at * 4;
    hz[0] = r0, hz[1] = r1, hz[2] = r2, hz[3] = r3;
    bw[0] = r0, bw[1] = r1, bw[2] = r2, bw[3] = r3;
    s_row[w][lane][0] = r0, s_row[w][lane][1] = r1, s_row[w][lane][2] = r2, s_row[w][lane][3] = r3;
  }
  const uint32_t k_win = (uint32_t)__popcll(__ballot(key != 0ull));
  __syncthreads();
  // this lane's two candidates: c = slot * K + position
  const int HK = H * K;
  u64 ck[2];
  const uint32_t* src[2];
  uint32_t age[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = lane + j * kWave;
    ck[j] = 0ull;
    src[j] = nullptr;
    age[j] = 0u;
    if (live && c < HK) {
      const int s = c / K, p = c - s * K;
      const uint32_t have = s == cur ? k_win : held[(size_t)s * group_cap + g];
      if ((uint32_t)p < have) {
        src[j] = s == cur ? reinterpret_cast<const uint32_t*>(&s_row[w][p][0])
                          : reinterpret_cast<const uint32_t*>(horizon + ((size_t)s * group_cap + g) * K + p);
        age[j] = (uint32_t)((cur - s + H) % H);
        ck[j] = recent_key(src[j][kTtftWord], age[j], (uint32_t)p);
      }
      s_ck[w][c] = ck[j];
    }
  }
  const uint32_t n_cand = (uint32_t)(__popcll(__ballot(ck[0] != 0ull)) + __popcll(__ballot(ck[1] != 0ull)));
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (ck[j] == 0ull) continue;
    int rank = 0;
    for (int c = 0; c < HK; ++c) rank += s_ck[w][c] > ck[j];
    if (rank < K) {
      const uint4* s = reinterpret_cast<const uint4*>(src[j]);
      uint4 r3 = s[3];
      r3.x = age[j];
      uint4* br = reinterpret_cast<uint4*>(block + lay.recent) + ((size_t)g * K + rank) * 4;
      br[0] = s[0], br[1] = s[1], br[2] = s[2], br[3] = r3;
    }
  }
  if (live && lane == 0) {
    block[lay.n + g] = count[g];
    count[g] = 0u;
    block[lay.k_win + g] = k_win;
    block[lay.k_recent + g] = min(n_cand, (uint32_t)K);
    held[(size_t)cur * group_cap + g] = k_win;
  }
}

}  // namespace

void launch_select(const Span* sp, int n, int n_groups, int k, bool lds, u64* keys, uint32_t* count, uint32_t* stats,
                   hipStream_t st) {
  if (n <= 0) return;
  const dim3 grid(grid_for(n, kNT, 1024));
  if (lds)
    hipLaunchKernelGGL(k_exemplar_select<true>, grid, dim3(kNT), 0, st, sp, n, n_groups, k, keys, count, stats);
  else
    hipLaunchKernelGGL(k_exemplar_select<false>, grid, dim3(kNT), 0, st, sp, n, n_groups, k, keys, count, stats);
}

void launch_merge(const Span* sp, int n, u64* keys, uint32_t* count, Row* horizon, uint32_t* held, uint32_t* block,
                  Layout lay, int group_cap, int k, int windows, int cur, hipStream_t st) {
  hipLaunchKernelGGL(k_exemplar_merge, dim3(grid_for(group_cap, kRowsPerBlock, 1 << 20)), dim3(kNT), 0, st, sp, n, keys,
                     count, horizon, held, block, lay, group_cap, k, windows, cur);
}

}  // namespace exemplars

using namespace exemplars;

ExemplarTracker::ExemplarTracker(const Config& cfg)
    : cfg_(cfg),
      lay_(layout(cfg.group_cap, cfg.k)),
      lane_("request exemplars", checked(cfg).device, cfg.n_buffers, cfg.span_cap, lay_.words, 1) {
  lane_.identify(exemplars::fingerprint(cfg));
  const size_t G = (size_t)cfg.group_cap, K = (size_t)cfg.k, H = (size_t)cfg.windows;
  keys_ = lane_.zeroed<unsigned long long>(G * K);
  count_ = lane_.zeroed<uint32_t>(G);
  horizon_ = lane_.zeroed<Row>(H * G * K);
  held_ = lane_.zeroed<uint32_t>(H * G);
  lane_.ready();
}

int64_t ExemplarTracker::step(const std::vector<Range>& spans, int n_groups) {
  check_step(n_groups, cfg_.group_cap);
  const size_t n = plan_ranges(spans, cfg_.span_cap);
  const auto [idx, s] = lane_.begin(spans);
  const hipStream_t st = lane_.stream();
  uint32_t* const blk = lane_.block();
  launch_select(lane_.spans(), (int)n, n_groups, cfg_.k, cfg_.lds, keys_, count_, blk + lay_.stats, st);
  lane_.mark(s, StepLane::kObserved);  // the select kernel is this tracker's observe
  launch_merge(lane_.spans(), (int)n, keys_, count_, horizon_, held_, blk, lay_, cfg_.group_cap, cfg_.k, cfg_.windows,
               (int)(idx % (int64_t)cfg_.windows), st);
  lane_.publish(s, 64);
  return idx;
}

std::vector<float> ExemplarTracker::step_ms(int64_t i) {
  return {lane_.ms(i, StepLane::kBegin, StepLane::kEnd), lane_.ms(i, StepLane::kCopied, StepLane::kEnd),
          lane_.ms(i, StepLane::kCopied, StepLane::kObserved)};
}

std::pair<std::vector<Row>, std::vector<uint32_t>> ExemplarTracker::resident() {
  const size_t G = (size_t)cfg_.group_cap, K = (size_t)cfg_.k, H = (size_t)cfg_.windows;
  sync();
  std::vector<Row> rows(H * G * K);
  std::vector<uint32_t> held(H * G);
  HIPCHECK(hipMemcpy(rows.data(), horizon_, rows.size() * sizeof(Row), hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(held.data(), held_, held.size() * 4, hipMemcpyDeviceToHost));
  return {std::move(rows), std::move(held)};
}

}  // namespace mislo
