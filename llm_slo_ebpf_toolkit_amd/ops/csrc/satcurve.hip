// Saturation curve per service (satcurve.h): the kernels and the host class.
#include "satcurve.h"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace mislo {
namespace satcurve {

namespace {

constexpr int kNT = 256;
constexpr int kWave = 64;
constexpr int kRowsPerBlock = kNT / kWave;

static_assert(kLdsSlots == kNT, "observe flushes its LDS table one slot per thread");
static_assert(kMinBins == kWave, "scan: every lane owns bins / 64 >= 1 bins");
static_assert(kMaxBins <= (int)kCarrySlot, "the carry key's slot is no ring slot");

using u64 = unsigned long long;
using loadsli::cell_delta;

__device__ __forceinline__ int64_t shfl_up64(int64_t v, int d) { return (int64_t)__shfl_up((long long)v, (unsigned)d, kWave); }
__device__ __forceinline__ int64_t shfl_down64(int64_t v, int d) { return (int64_t)__shfl_down((long long)v, (unsigned)d, kWave); }
__device__ __forceinline__ int64_t wave_sum64(int64_t v) {
  for (int d = kWave / 2; d; d >>= 1) v += (int64_t)__shfl_xor((long long)v, d, kWave);
  return v;
}
__device__ __forceinline__ int wave_max32(int v) {
  for (int d = kWave / 2; d; d >>= 1) {
    const int o = __shfl_xor(v, d, kWave);
    v = o > v ? o : v;
  }
  return v;
}

// One wave per row of group_cap. The advance evicts the `count` oldest bins of the old ring, from
// `first` ascending (1 <= count <= bins); lane l owns the `per` consecutive ones from l * per. The wave's
// inclusive scan of the lanes' sums of starts - ends (__shfl_up), shifted by one lane and started at
// carry, gives a lane the requests in flight before its first bin, so every evicted bin has its level.
// A bin >= fold_lo (whole history; fold_lo >= 0) with a non-empty sli cell adds it into generation
// epoch & 1 of the row under that level; lanes of one wave may hit one level, hence the atomics. All
// three cells of every evicted slot are cleared and lane 0 moves carry on (the row's only writer).
// g < group_cap, slot < bins, level < kK: every access lies inside the arrays.
__global__ __launch_bounds__(kNT) void k_sat_fold(u64* __restrict__ counts, u64* __restrict__ idle, u64* __restrict__ sli,
                                                  u64* __restrict__ gen, int32_t* __restrict__ carry, int group_cap,
                                                  uint32_t bins, int64_t first, uint32_t count, int64_t fold_lo,
                                                  int64_t bin_us, int64_t epoch_bins) {
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
  const int g = blockIdx.x * kRowsPerBlock + w;
  if (g >= group_cap) return;  // the whole wave; no barrier below
  u64* crow = counts + (size_t)g * bins;
  u64* irow = idle + (size_t)g * bins;
  u64* srow = sli + (size_t)g * bins;
  const uint32_t per = (count + kWave - 1) / kWave;
  const uint32_t j0 = min((uint32_t)lane * per, count), j1 = min(j0 + per, count);
  int64_t run = 0;
  for (uint32_t j = j0; j < j1; ++j) run += cell_delta(crow[onset::slot_of(first + (int64_t)j, bins)]);
  for (int d = 1; d < kWave; d <<= 1) {
    const int64_t before = shfl_up64(run, d);
    if (lane >= d) run += before;
  }
  int64_t A = shfl_up64(run, 1);
  if (lane == 0) A = 0;
  const int64_t total = (int64_t)__shfl((long long)run, kWave - 1, kWave);
  A += (int64_t)carry[g];
  for (uint32_t j = j0; j < j1; ++j) {
    const int64_t e = first + (int64_t)j;
    const uint32_t s = onset::slot_of(e, bins);
    const u64 c = crow[s], x = srow[s];
    if (e >= fold_lo && x != 0ull) {
      const uint32_t level = level_of(A, c, irow[s], bin_us);
      u64* at = gen + (((size_t)(epoch_of(e, epoch_bins) & 1) * group_cap + g) * kK + level) * 2;
      atomicAdd(at, (u64)sli_n(x));
      if (sli_b(x)) atomicAdd(at + 1, (u64)sli_b(x));
    }
    A += cell_delta(c);
    crow[s] = 0ull;
    irow[s] = 0ull;
    srow[s] = 0ull;
  }
  if (lane == 0 && total != 0) carry[g] += (int32_t)total;
}

// One thread per record: the load tracker's observe with the third cell. An observed record with a
// TTFT adds 1 + (breach << 32) into `sli` wherever place() places its start; the same LDS table
// carries the three values of a (service, slot), and a clipped record's carry increment under the slot
// kCarrySlot. g < n_groups <= group_cap and slot < bins: every add lies inside the arrays.
template <bool kLds>
__global__ __launch_bounds__(kNT) void k_sat_observe(const Span* __restrict__ sp, int n, int n_groups, int64_t bin_us,
                                                     int64_t q_hi, uint32_t bins, float slo_ms, u64* __restrict__ counts,
                                                     u64* __restrict__ idle, u64* __restrict__ sli,
                                                     int32_t* __restrict__ carry, uint32_t* __restrict__ stats) {
  __shared__ u64 s_key[kLds ? kLdsSlots : 1];
  __shared__ u64 s_cnt[kLds ? kLdsSlots : 1];
  __shared__ u64 s_idle[kLds ? kLdsSlots : 1];
  __shared__ u64 s_sli[kLds ? kLdsSlots : 1];
  __shared__ uint32_t s_stats[kStats];
  if (kLds) s_key[threadIdx.x] = 0ull, s_cnt[threadIdx.x] = 0ull, s_idle[threadIdx.x] = 0ull, s_sli[threadIdx.x] = 0ull;
  if (threadIdx.x < kStats) s_stats[threadIdx.x] = 0u;
  __syncthreads();
  // one update of (g, slot): `c` into counts (or carry, slot == kCarrySlot), `i` into idle_us, `x` into sli
  auto update = [&](uint32_t g, uint32_t slot, u64 c, u64 i, u64 x) {
    if (kLds) {
      const u64 key = loadsli::lds_key(g, slot);
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
          if (x) atomicAdd(&s_sli[s], x);
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
    if (x) atomicAdd(sli + (size_t)g * bins + slot, x);
  };
  for (size_t i = blockIdx.x * (size_t)kNT + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * kNT) {
    if (sp[i].flags & kNotAnEnd) continue;
    const uint32_t g = sp[i].group_id;
    if (g >= (uint32_t)n_groups) {
      atomicAdd(&s_stats[kOutOfGroup], 1u);
      continue;
    }
    const float v = sp[i].latency_ms;
    if (!loadsli::latency_valid(v)) {
      atomicAdd(&s_stats[kInvalid], 1u);
      continue;
    }
    const int64_t ts_ns = sp[i].ts_ns;
    if (ts_ns <= 0) {
      atomicAdd(&s_stats[kNoTime], 1u);
      continue;
    }
    atomicAdd(&s_stats[kObserved], 1u);
    const float ttft = sp[i].ttft_ms;
    u64 x = 0ull;
    if (has_ttft(ttft))
      x = sli_add(ttft, slo_ms);
    else
      atomicAdd(&s_stats[kNoTtft], 1u);
    const loadsli::Placement p = loadsli::place(loadsli::ts_us_of(ts_ns), loadsli::dur_us_of(v), bin_us, q_hi, bins);
    if (p.bits & loadsli::kPFuture) atomicAdd(&s_stats[kFuture], 1u);
    if (p.bits & loadsli::kPTooOld) {
      atomicAdd(&s_stats[kTooOld], 1u);
      continue;
    }
    if (p.bits & loadsli::kPClipped) {
      atomicAdd(&s_stats[kClipped], 1u);
      update(g, kCarrySlot, 1ull, 0ull, 0ull);
    }
    if ((p.bits & loadsli::kPStart) && p.qs == p.qe) {
      update(g, onset::slot_of(p.qe, bins), kStartAdd + kEndAdd, p.idle_s + p.idle_e, x);
    } else {
      if (p.bits & loadsli::kPStart) update(g, onset::slot_of(p.qs, bins), kStartAdd, p.idle_s, x);
      update(g, onset::slot_of(p.qe, bins), kEndAdd, p.idle_e, 0ull);
    }
  }
  __syncthreads();
  if (kLds) {
    const u64 key = s_key[threadIdx.x];
    if (key != 0ull) {
      const uint32_t g = loadsli::lds_group(key), slot = loadsli::lds_slot(key);
      if (slot == kCarrySlot) {
        atomicAdd(carry + g, (int32_t)s_cnt[threadIdx.x]);
      } else {
        atomicAdd(counts + (size_t)g * bins + slot, s_cnt[threadIdx.x]);
        if (s_idle[threadIdx.x]) atomicAdd(idle + (size_t)g * bins + slot, s_idle[threadIdx.x]);
        if (s_sli[threadIdx.x]) atomicAdd(sli + (size_t)g * bins + slot, s_sli[threadIdx.x]);
      }
    }
  }
  if (threadIdx.x < kStats && s_stats[threadIdx.x]) atomicAdd(&stats[threadIdx.x], s_stats[threadIdx.x]);
}

struct ScanParams {
  int64_t q_hi, q_first, bin_us, epoch_bins, budget_ppm, min_requests;
  uint32_t bins, live;  // live: bit p = generation p belongs to the merged curve
  int settle, recent, group_cap;
};

// One wave per service row, every row of group_cap; a workgroup's four waves share only the barriers.
// In ring order lane l owns the bins / 64 consecutive bins from l * bins / 64: the load tracker's scan
// gives it the requests in flight before its first bin, and one pass over its bins every bin's busy
// time and level. A settled bin with whole history adds its sli into the wave's own LDS histogram of
// kK x (n, b) -- lanes of one wave may hit one level, hence LDS atomics -- and a recent bin its busy
// time into the lane's sum. Then lane l owns the levels 3 l .. 3 l + 2 (lanes 0 .. 53): histogram plus
// the live generations is the merged curve, stored as one 16-byte store a level; the lane's scores and
// an inclusive __shfl_down suffix scan of the lanes' totals give S at each of its levels; a wave
// arg-max, the larger level winning ties, finds the knee, and wave sums the suffix counts at it, the
// totals and the top level. Lane 0 decides the state and the age and stores the row as four 16-byte
// stores. g < group_cap, slot < bins, level < kK: every access lies inside the arrays and the block.
__global__ __launch_bounds__(kNT) void k_sat_scan(const u64* __restrict__ counts, const u64* __restrict__ idle,
                                                  const u64* __restrict__ sli, const u64* __restrict__ gen,
                                                  const int32_t* __restrict__ carry, uint32_t* __restrict__ age, ScanParams P,
                                                  uint32_t* __restrict__ block, size_t rows_at, size_t curve_at) {
  __shared__ u64 s_hist[kRowsPerBlock][kK * 2];
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
  const int g = blockIdx.x * kRowsPerBlock + w;
  const bool on = g < P.group_cap;  // a whole wave; every wave reaches both barriers
  for (int i = lane; i < kK * 2; i += kWave) s_hist[w][i] = 0ull;
  __syncthreads();
  const uint32_t bins = P.bins;
  const Ranges r = ranges_of(P.q_hi, P.q_first, bins, P.settle, P.recent);
  int64_t busy_rec = 0;
  if (on) {
    const u64* crow = counts + (size_t)g * bins;
    const u64* irow = idle + (size_t)g * bins;
    const u64* srow = sli + (size_t)g * bins;
    const uint32_t per = bins >> 6;
    const int64_t first = r.oldest + (int64_t)lane * per;
    int64_t run = 0;
    for (uint32_t j = 0; j < per; ++j) run += cell_delta(crow[onset::slot_of(first + j, bins)]);
    for (int d = 1; d < kWave; d <<= 1) {
      const int64_t before = shfl_up64(run, d);
      if (lane >= d) run += before;
    }
    int64_t A = shfl_up64(run, 1);
    if (lane == 0) A = 0;
    A += (int64_t)carry[g];
    for (uint32_t j = 0; j < per; ++j) {
      const int64_t q = first + j;
      const uint32_t s = onset::slot_of(q, bins);
      const u64 c = crow[s];
      const int64_t busy = loadsli::bin_busy(loadsli::bin_active(A, c), P.bin_us, irow[s]);
      A += cell_delta(c);
      if (q >= r.lo && q <= r.settled_hi) {
        const u64 x = srow[s];
        if (x != 0ull) {
          const uint32_t level = level_of_u(u_of(busy, P.bin_us));
          atomicAdd(&s_hist[w][2 * level], (u64)sli_n(x));
          if (sli_b(x)) atomicAdd(&s_hist[w][2 * level + 1], (u64)sli_b(x));
        }
      }
      if (r.recent_known && q >= r.recent_lo && q <= r.recent_hi) busy_rec += busy;
    }
  }
  __syncthreads();
  if (!on) return;
  busy_rec = wave_sum64(busy_rec);
  // the lane's three levels, from the highest down: s[k] = the lane's own suffix of scores at level 3 l + k
  u64 n[kPerLane], b[kPerLane];
  int64_t s[kPerLane];
  int64_t mine = 0;
  uint64_t n_lane = 0, b_lane = 0;
  int top = -1;
  uint4* cout = reinterpret_cast<uint4*>(block + curve_at) + (size_t)g * kK;
  for (int k = kPerLane - 1; k >= 0; --k) {
    const int level = lane * kPerLane + k;
    n[k] = b[k] = 0ull;
    if (level < kK) {
      n[k] = s_hist[w][2 * level], b[k] = s_hist[w][2 * level + 1];
      for (int p = 0; p < 2; ++p)
        if (P.live >> p & 1u) {
          const u64* at = gen + (((size_t)p * P.group_cap + g) * kK + level) * 2;
          n[k] += at[0], b[k] += at[1];
        }
      cout[level] = make_uint4((uint32_t)n[k], (uint32_t)(n[k] >> 32), (uint32_t)b[k], (uint32_t)(b[k] >> 32));
      if (n[k] != 0ull && level > top) top = level;
    }
    mine += score(n[k], b[k], P.budget_ppm);
    s[k] = mine;
    n_lane += n[k], b_lane += b[k];
  }
  int64_t suffix = mine;  // inclusive over lanes >= this one
  for (int d = 1; d < kWave; d <<= 1) {
    const int64_t after = shfl_down64(suffix, d);
    if (lane + d < kWave) suffix += after;
  }
  const int64_t above = suffix - mine;  // the lanes above this one
  int64_t best = INT64_MIN;
  int best_l = -1;
  for (int k = kPerLane - 1; k >= 0; --k) {  // strict: the larger level keeps a tie
    const int level = lane * kPerLane + k;
    if (level < kK && above + s[k] > best) best = above + s[k], best_l = level;
  }
  for (int d = kWave / 2; d; d >>= 1) {
    const int64_t ob = (int64_t)__shfl_xor((long long)best, d, kWave);
    const int ol = __shfl_xor(best_l, d, kWave);
    if (ob > best || (ob == best && ol > best_l)) best = ob, best_l = ol;
  }
  const bool knee = best > 0;  // best_l in 0 .. kK - 1 then
  uint64_t nk = 0, bk = 0;
  if (knee)
    for (int k = 0; k < kPerLane; ++k)
      if (lane * kPerLane + k >= best_l) nk += n[k], bk += b[k];
  nk = (uint64_t)wave_sum64((int64_t)nk), bk = (uint64_t)wave_sum64((int64_t)bk);
  const uint64_t n_total = (uint64_t)wave_sum64((int64_t)n_lane), b_total = (uint64_t)wave_sum64((int64_t)b_lane);
  top = wave_max32(top);
  if (lane == 0) {
    const bool valid = knee && nk >= (uint64_t)P.min_requests;
    const uint32_t recent_u = u_of(busy_rec, (int64_t)P.recent * P.bin_us);
    const uint32_t state = state_of(r.recent_known, n_total, P.min_requests, valid, level_of_u(recent_u), (uint32_t)best_l);
    const uint32_t a = age_of(state, age[g]);
    age[g] = a;
    const bool known = state != kUnknown, shown = known && valid;
    const uint64_t on_ = shown ? nk : 0ull, ob_ = shown ? bk : 0ull, br = known ? (uint64_t)busy_rec : 0ull;
    uint4* out = reinterpret_cast<uint4*>(block + rows_at) + (size_t)g * (kRowBytes / 16);
    out[0] = make_uint4(state, shown ? (uint32_t)best_l : kNone, known ? recent_u : 0u, top < 0 ? kNone : (uint32_t)top);
    out[1] = make_uint4((uint32_t)n_total, (uint32_t)(n_total >> 32), (uint32_t)b_total, (uint32_t)(b_total >> 32));
    out[2] = make_uint4((uint32_t)on_, (uint32_t)(on_ >> 32), (uint32_t)ob_, (uint32_t)(ob_ >> 32));
    out[3] = make_uint4((uint32_t)br, (uint32_t)(br >> 32), a, 0u);
  }
}

}  // namespace
}  // namespace satcurve

using namespace satcurve;

SaturationTracker::SaturationTracker(const Config& cfg)
    : cfg_(cfg),
      lay_(layout(cfg.group_cap)),
      ring_pop_((uint32_t)cfg.bins, cfg.ring_records_max),
      curve_pop_(cfg.epoch_bins, cfg.curve_records_max),
      lane_("saturation curve", checked(cfg).device, cfg.n_buffers, cfg.span_cap, lay_.words, 2) {
  lane_.identify(satcurve::fingerprint(cfg), 6);
  const size_t cells = (size_t)cfg.group_cap * (size_t)cfg.bins, G = (size_t)cfg.group_cap;
  counts_ = lane_.zeroed<u64>(cells);
  idle_ = lane_.zeroed<u64>(cells);
  sli_ = lane_.zeroed<u64>(cells);
  gen_ = lane_.zeroed<u64>(G * 2 * kK * 2);
  carry_ = lane_.zeroed<int32_t>(G);
  age_ = lane_.zeroed<uint32_t>(G);
  lane_.ready();
}

int64_t SaturationTracker::step(const std::vector<Range>& spans, int64_t cut_ns, int n_groups) {
  check_step(cut_ns, n_groups, cfg_.group_cap);
  const size_t n = plan_ranges(spans, cfg_.span_cap);
  const int64_t prev = q_hi_, q_hi = onset::advance(prev, loadsli::ts_us_of(cut_ns), cfg_.bin_us);
  ring_pop_.check(q_hi, n);
  curve_pop_.check(q_hi, n);
  // nothing has changed up to here
  ring_pop_.take(q_hi, n);
  curve_pop_.take(q_hi, n);
  const uint32_t bins = (uint32_t)cfg_.bins;
  const Fold fold = fold_of(prev, q_hi, q_first_, bins);  // against the old q_first
  const uint32_t clear = gens_.begin(fold, cfg_.epoch_bins);
  q_hi_ = q_hi;
  if (prev == kNoBin || q_hi - prev >= (int64_t)bins) q_first_ = q_hi;
  const auto [idx, s] = lane_.begin(spans);
  const hipStream_t st = lane_.stream();
  uint32_t* const blk = lane_.block();
  const int G = cfg_.group_cap;
  uint32_t* stats = blk + lay_.stats;
  const size_t gen_words = (size_t)G * kK * 2;  // one generation, every row
  for (int p = 0; p < 2; ++p)
    if (clear >> p & 1u) HIPCHECK(hipMemsetAsync(gen_ + (size_t)p * gen_words, 0, gen_words * 8, st));
  const dim3 block(kNT), rows(grid_for(G, kRowsPerBlock, 1 << 20));
  if (fold.count)
    hipLaunchKernelGGL(k_sat_fold, rows, block, 0, st, counts_, idle_, sli_, gen_, carry_, G, bins, fold.first, fold.count,
                       fold.lo, cfg_.bin_us, cfg_.epoch_bins);
  lane_.mark(s, StepLane::kAdvanced);
  if (n) {
    const dim3 og(grid_for((int64_t)n, kNT, 1024));
    const float slo = (float)cfg_.slo_ms;
    if (cfg_.lds)
      hipLaunchKernelGGL(k_sat_observe<true>, og, block, 0, st, lane_.spans(), (int)n, n_groups, cfg_.bin_us, q_hi, bins, slo,
                         counts_, idle_, sli_, carry_, stats);
    else
      hipLaunchKernelGGL(k_sat_observe<false>, og, block, 0, st, lane_.spans(), (int)n, n_groups, cfg_.bin_us, q_hi, bins,
                         slo, counts_, idle_, sli_, carry_, stats);
  }
  lane_.mark(s, StepLane::kObserved);
  ScanParams P;
  P.q_hi = q_hi, P.q_first = q_first_, P.bin_us = cfg_.bin_us, P.epoch_bins = cfg_.epoch_bins;
  P.budget_ppm = cfg_.budget_ppm, P.min_requests = cfg_.min_requests, P.bins = bins;
  P.live = gens_.live(epoch_now(onset::oldest_bin(q_hi, bins), cfg_.epoch_bins));
  P.settle = cfg_.settle_bins, P.recent = cfg_.recent_bins, P.group_cap = G;
  hipLaunchKernelGGL(k_sat_scan, rows, block, 0, st, counts_, idle_, sli_, gen_, carry_, age_, P, blk, lay_.rows, lay_.curve);
  lane_.publish(s, 1024, lay_.stats / 4);
  return idx;
}

std::vector<float> SaturationTracker::step_ms(int64_t i) {
  return {lane_.ms(i, StepLane::kBegin, StepLane::kEnd), lane_.ms(i, StepLane::kCopied, StepLane::kEnd),
          lane_.ms(i, StepLane::kAdvanced, StepLane::kObserved)};
}

Resident SaturationTracker::resident() {
  sync();
  Resident out;
  out.q_hi = q_hi_;
  out.q_first = q_first_;
  out.gen_epoch[0] = gens_.epoch[0], out.gen_epoch[1] = gens_.epoch[1];
  const size_t cells = (size_t)cfg_.group_cap * (size_t)cfg_.bins, G = (size_t)cfg_.group_cap;
  out.counts.resize(cells);
  out.idle_us.resize(cells);
  out.sli.resize(cells);
  out.gen.resize(G * 2 * kK * 2);
  out.carry.resize(G);
  out.age.resize(G);
  HIPCHECK(hipMemcpy(out.counts.data(), counts_, cells * 8, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(out.idle_us.data(), idle_, cells * 8, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(out.sli.data(), sli_, cells * 8, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(out.gen.data(), gen_, out.gen.size() * 8, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(out.carry.data(), carry_, G * 4, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(out.age.data(), age_, G * 4, hipMemcpyDeviceToHost));
  return out;
}

}  // namespace mislo
