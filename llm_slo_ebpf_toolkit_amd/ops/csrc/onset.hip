// Breach onset per service (onset.h): the kernels and the host class.
#include "onset.h"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace mislo {
namespace onset {

namespace {

constexpr int kNT = 256;
constexpr int kWave = 64;
constexpr int kRowsPerBlock = kNT / kWave;

static_assert(kLdsSlots == kNT, "observe flushes its LDS table one slot per thread");
static_assert(kMinBins == kWave, "scan: every lane owns bins / 64 >= 1 bins");

using u64 = unsigned long long;

// One thread per (row, newly exposed bin): the slots of the bins (prev, prev + count] of every row
// of group_cap are cleared; count = min(bins, q_hi - prev) >= 1.
__global__ __launch_bounds__(kNT) void k_onset_advance(u64* __restrict__ ring, int group_cap, uint32_t bins, int64_t prev,
                                                       uint32_t count) {
  const size_t total = (size_t)group_cap * count;
  for (size_t i = blockIdx.x * (size_t)kNT + threadIdx.x; i < total; i += (size_t)gridDim.x * kNT) {
    const size_t row = i / count;
    const uint32_t j = (uint32_t)(i - row * count);
    ring[row * bins + slot_of(prev + 1 + (int64_t)j, bins)] = 0ull;
  }
}

// One thread per record: the records k_decode_spans counts (no kSpanNoSli, a group below n_groups)
// with a TTFT >= 0 (NaN and negatives fail the compare) are observed; one with a start time goes to
// the bin of that time (place()), as one 64-bit add of (breach << 32 | 1) into its (service, slot)
// cell. A window spans only window / bin_ns bins, so a busy service puts thousands of adds on a few
// addresses: with kLds the workgroup aggregates its cells in an LDS table of kLdsSlots keyed
// (service, slot) and sends each to the ring once. A record that finds no LDS slot within kLdsProbes
// goes to the ring itself. g < n_groups <= group_cap and slot < bins: every add lies inside the ring.
template <bool kLds>
__global__ __launch_bounds__(kNT) void k_onset_observe(const Span* __restrict__ sp, int n, int n_groups, float slo,
                                                       int64_t bin_ns, int64_t q_hi, uint32_t bins, u64* __restrict__ ring,
                                                       uint32_t* __restrict__ stats) {
  __shared__ u64 s_key[kLds ? kLdsSlots : 1];
  __shared__ u64 s_val[kLds ? kLdsSlots : 1];
  __shared__ uint32_t s_stats[kStats];
  if (kLds) s_key[threadIdx.x] = 0ull, s_val[threadIdx.x] = 0ull;
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
    int64_t q = 0;
    const Place where = place(sp[i].ts_ns, bin_ns, q_hi, bins, &q);
    if (where == kDroppedNoTime) {
      atomicAdd(&s_stats[kNoTime], 1u);
      continue;
    }
    if (where == kDroppedOld) {
      atomicAdd(&s_stats[kTooOld], 1u);
      continue;
    }
    if (where == kPlacedFuture) atomicAdd(&s_stats[kFuture], 1u);
    const uint32_t slot = slot_of(q, bins);
    const u64 add = cell_add(v > slo ? 1u : 0u);
    bool done = false;
    if (kLds) {
      const u64 key = lds_key(g, slot);
      uint32_t s = lds_hash(key);
      for (int probe = 0; probe < kLdsProbes && !done; ++probe, s = (s + 1u) & (kLdsSlots - 1)) {
        u64 k = __hip_atomic_load(&s_key[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (k == 0ull) {
          k = atomicCAS(&s_key[s], 0ull, key);
          if (k == 0ull) k = key;
        }
        if (k == key) {
          atomicAdd(&s_val[s], add);
          done = true;
        }
      }
    }
    if (!done) atomicAdd(ring + (size_t)g * bins + slot, add);
  }
  __syncthreads();
  if (kLds) {
    const u64 key = s_key[threadIdx.x];
    if (key != 0ull) atomicAdd(ring + (size_t)lds_group(key) * bins + lds_slot(key), s_val[threadIdx.x]);
  }
  if (threadIdx.x < kStats && s_stats[threadIdx.x]) atomicAdd(&stats[threadIdx.x], s_stats[threadIdx.x]);
}

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
__device__ __forceinline__ uint32_t wave_sum32(uint32_t v) {
  for (int d = kWave / 2; d; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, kWave);
  return v;
}

// One wave per service row, every row of group_cap. In ring order (index 0 = the oldest bin
// q_hi - bins + 1) lane l owns the bins / 64 consecutive bins from l * bins / 64. It reduces them
// to a Run (sum, minimum prefix capped at 0); the wave's exclusive scan of the runs under combine()
// gives the lane the prefix sum P and its running minimum M before its first bin, and S = P - M
// bin by bin in a second pass. In that pass the lane keeps, since its last zero of S (or its first
// bin): the peak, the first bin at or above h and the counts. The wave's last zero Z is the
// maximum of the lanes'; the excursion is the lane that holds Z (after it) and every lane past it,
// none of which has a zero, so their values since their own last zero are the excursion's.
__global__ __launch_bounds__(kNT) void k_onset_scan(const u64* __restrict__ ring, uint32_t bins, int64_t q_hi,
                                                    int64_t ref_ppm, int64_t h, uint32_t* __restrict__ block,
                                                    size_t rows_at, int group_cap) {
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
  const int g = blockIdx.x * kRowsPerBlock + w;
  if (g >= group_cap) return;  // the whole wave; no barrier below
  const u64* row = ring + (size_t)g * bins;
  const uint32_t per = bins >> 6;
  const int64_t q0 = oldest_bin(q_hi, bins);
  const int64_t first = (int64_t)lane * per;
  Run run = run_identity();
  for (uint32_t j = 0; j < per; ++j) run = combine(run, run_of(excess(row[slot_of(q0 + first + j, bins)], ref_ppm)));
  for (int d = 1; d < kWave; d <<= 1) {
    const Run before{shfl_up64(run.s, d), shfl_up64(run.m, d)};
    if (lane >= d) run = combine(before, run);
  }
  Run ex{shfl_up64(run.s, 1), shfl_up64(run.m, 1)};
  if (lane == 0) ex = run_identity();
  int64_t P = ex.s, M = ex.m, S = 0, zero = -1, peak = 0, alarm = -1;
  uint32_t n_e = 0, b_e = 0, n_all = 0, b_all = 0;
  for (uint32_t j = 0; j < per; ++j) {
    const u64 c = row[slot_of(q0 + first + j, bins)];
    P += excess(c, ref_ppm);
    M = P < M ? P : M;
    S = P - M;
    n_all += cell_n(c), b_all += cell_b(c);
    if (S == 0) {
      zero = first + j, peak = 0, alarm = -1, n_e = 0, b_e = 0;
    } else {
      n_e += cell_n(c), b_e += cell_b(c);
      peak = S > peak ? S : peak;
      if (alarm < 0 && S >= h) alarm = first + j;
    }
  }
  const int64_t Z = wave_max64(zero);  // -1: no zero in the ring (clipped)
  const bool in = first > Z || zero == Z;
  const int64_t s_now = (int64_t)__shfl((long long)S, kWave - 1, kWave);
  const int64_t s_peak = wave_max64(in ? peak : 0);
  const int64_t a_min = wave_min64(in && alarm >= 0 ? alarm : (int64_t)bins);
  const uint32_t n_exc = wave_sum32(in ? n_e : 0u), b_exc = wave_sum32(in ? b_e : 0u);
  const uint32_t n_ring = wave_sum32(n_all), b_ring = wave_sum32(b_all);
  if (lane == 0) {
    // the Row, word by word: state flags onset_q | alarm_q s_now | s_peak n_exc b_exc | n_ring b_ring pad pad
    const bool open = s_now != 0, fired = open && a_min < (int64_t)bins;
    const uint64_t onset_q = (uint64_t)(open ? q0 + Z + 1 : kNoBin), alarm_q = (uint64_t)(fired ? q0 + a_min : kNoBin);
    const uint64_t now = (uint64_t)s_now, pk = (uint64_t)(open ? s_peak : 0);
    uint4* out = reinterpret_cast<uint4*>(block + rows_at) + (size_t)g * (kRowBytes / 16);
    out[0] = make_uint4(fired ? kAlarm : (open ? kExcursion : kQuiet), open && Z < 0 ? kClipped : 0u, (uint32_t)onset_q,
                        (uint32_t)(onset_q >> 32));
    out[1] = make_uint4((uint32_t)alarm_q, (uint32_t)(alarm_q >> 32), (uint32_t)now, (uint32_t)(now >> 32));
    out[2] = make_uint4((uint32_t)pk, (uint32_t)(pk >> 32), open ? n_exc : 0u, open ? b_exc : 0u);
    out[3] = make_uint4(n_ring, b_ring, 0u, 0u);
  }
}

}  // namespace
}  // namespace onset

using namespace onset;

OnsetTracker::OnsetTracker(const Config& cfg)
    : cfg_(cfg),
      lay_(layout(cfg.group_cap)),
      pop_((uint32_t)cfg.bins, cfg.ring_records_max),
      lane_("breach onset", checked(cfg).device, cfg.n_buffers, cfg.span_cap, lay_.words, 2) {
  lane_.identify(onset::fingerprint(cfg), 2);
  ring_ = lane_.zeroed<unsigned long long>((size_t)cfg.group_cap * (size_t)cfg.bins);
  lane_.ready();
}

int64_t OnsetTracker::step(const std::vector<Range>& spans, int64_t cut_ns, int n_groups) {
  check_step(cut_ns, n_groups, cfg_.group_cap);
  const size_t n = plan_ranges(spans, cfg_.span_cap);
  const int64_t prev = q_hi_, q_hi = advance(prev, cut_ns, cfg_.bin_ns);
  pop_.check(q_hi, n);
  // nothing has changed up to here
  pop_.take(q_hi, n);
  q_hi_ = q_hi;
  const auto [idx, s] = lane_.begin(spans);
  const hipStream_t st = lane_.stream();
  uint32_t* const blk = lane_.block();
  const int G = cfg_.group_cap;
  const uint32_t bins = (uint32_t)cfg_.bins;
  uint32_t* stats = blk + lay_.stats;
  const dim3 block(kNT);
  if (q_hi > prev) {
    const uint32_t count = cleared(prev, q_hi, bins);
    hipLaunchKernelGGL(k_onset_advance, dim3(grid_for((int64_t)G * count, kNT, 1024)), block, 0, st, ring_, G, bins, prev,
                       count);
  }
  lane_.mark(s, StepLane::kAdvanced);
  if (n) {
    const dim3 og(grid_for((int64_t)n, kNT, 1024));
    const float slo = (float)cfg_.slo_ms;
    if (cfg_.lds)
      hipLaunchKernelGGL(k_onset_observe<true>, og, block, 0, st, lane_.spans(), (int)n, n_groups, slo, cfg_.bin_ns, q_hi,
                         bins, ring_, stats);
    else
      hipLaunchKernelGGL(k_onset_observe<false>, og, block, 0, st, lane_.spans(), (int)n, n_groups, slo, cfg_.bin_ns, q_hi,
                         bins, ring_, stats);
  }
  lane_.mark(s, StepLane::kObserved);
  hipLaunchKernelGGL(k_onset_scan, dim3(grid_for(G, kRowsPerBlock, 1 << 20)), block, 0, st, ring_, bins, q_hi, cfg_.ref_ppm,
                     cfg_.alarm * kMillion, blk, lay_.rows, G);
  lane_.publish(s, 1024);
  return idx;
}

std::vector<float> OnsetTracker::step_ms(int64_t i) {
  return {lane_.ms(i, StepLane::kBegin, StepLane::kEnd), lane_.ms(i, StepLane::kCopied, StepLane::kEnd),
          lane_.ms(i, StepLane::kAdvanced, StepLane::kObserved)};
}

Resident OnsetTracker::resident() {
  sync();
  Resident out;
  out.q_hi = q_hi_;
  out.cells.resize((size_t)cfg_.group_cap * (size_t)cfg_.bins);
  HIPCHECK(hipMemcpy(out.cells.data(), ring_, out.cells.size() * 8, hipMemcpyDeviceToHost));
  return out;
}

}  // namespace mislo
