// Native per-GPU window engine (engine.h) and its small glue kernels.
#include "engine.h"
#include "mislo_packet_kernels.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>

namespace mislo {

namespace {

#define HIPCHECK(x)                                                                                  \
  do {                                                                                               \
    hipError_t _e = (x);                                                                             \
    if (_e != hipSuccess) throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(_e) + \
                                                   " at " #x);                                       \
  } while (0)

#define NCCLCHECK(x)                                                                                        \
  do {                                                                                                      \
    ncclResult_t _r = (x);                                                                                  \
    if (_r != ncclSuccess) throw std::runtime_error(std::string("RCCL error: ") + ncclGetErrorString(_r) + \
                                                    " at " #x);                                             \
  } while (0)

// totals += packet, and the packet stored straight into its pinned host block
__global__ void k_accumulate(const double* __restrict__ packet, double* __restrict__ totals, int n,
                             double* __restrict__ host) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const double v = packet[i];
    totals[i] += v;
    host[i] = v;
  }
}

// The tail of a single-GPU window in one dispatch (it was three: pack, results copy, accumulate):
// the packet from the accumulators -- kept on the device for the prequential refit --, added to
// the run's totals and stored into its pinned host block; the per-incident results block copied
// to its pinned host block.
__global__ __launch_bounds__(256) void k_window_end(const uint32_t* hist, const uint32_t* status,
                                                    const unsigned long long* misc, const unsigned long long* dbg,
                                                    const uint32_t* confusion, const double* stats, const double* count,
                                                    const uint32_t* ring, double* __restrict__ packet,
                                                    double* __restrict__ totals, double* __restrict__ packet_host,
                                                    const uint4* __restrict__ res, uint4* __restrict__ res_host,
                                                    size_t res16) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  if (t < (size_t)kPacketLen) {
    const double v = packet_value((int)t, hist, status, misc, dbg, confusion, stats, count, ring);
    packet[t] = v;
    totals[t] += v;
    packet_host[t] = v;
  }
  for (size_t i = t; i < res16; i += stride) res_host[i] = res[i];
}

// Small copies between device memory and pinned host memory, by a kernel (loads or stores over
// PCIe). A small hipMemcpyAsync is served by the host through the BAR, which blocks the issuing
// thread until the stream reaches the copy -- for the results D2H the whole window's compute
// (measured: ~480 us per window of host time in submit) -- where a kernel is queued like any
// other launch.
__global__ void k_to_host(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n16) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x)
    dst[i] = src[i];
}

void to_host(const void* src, void* dst, size_t bytes, hipStream_t st) {
  const size_t n16 = (bytes + 15) / 16;
  const int g = (int)std::min<size_t>(64, (n16 + 255) / 256);
  hipLaunchKernelGGL(k_to_host, dim3(g > 0 ? g : 1), dim3(256), 0, st, static_cast<const uint4*>(src),
                     static_cast<uint4*>(dst), n16);
}

constexpr int kCopyAheadDefault = 1;  // MISLO_COPY_AHEAD where windows overlap (profiles/copy_ahead/README.md)
constexpr unsigned kEvWait = hipEventDisableTiming | hipEventBlockingSync;  // events the host sleeps on
// an integer environment knob, `unset` where it is not set
int env_int(const char* name, int unset) {
  const char* v = getenv(name);
  return v ? atoi(v) : unset;
}

// laps of a steady clock, each added to an accumulator in microseconds
struct Lap {
  using clock = std::chrono::steady_clock;
  clock::time_point t = clock::now();
  void operator()(double& acc) {
    const auto n = clock::now();
    acc += std::chrono::duration<double, std::micro>(n - t).count();
    t = n;
  }
};

}  // namespace

void engine_set_tables(const Tables& t) { set_tables(&t); }

// What the engine creates is recorded in own_, which destroys it: events, memory, streams.
template <class T>
T* WindowEngine::dalloc(size_t n, bool zero) {
  void* p = nullptr;
  HIPCHECK(hipMalloc(&p, n * sizeof(T) + 64));
  own_.dev.push_back(p);
  if (zero) HIPCHECK(hipMemset(p, 0, n * sizeof(T)));
  return static_cast<T*>(p);
}

void* WindowEngine::host_alloc(size_t bytes, unsigned flags) {
  void* h = nullptr;
  HIPCHECK(hipHostMalloc(&h, bytes, flags));
  own_.host.push_back(h);
  return h;
}

// pinned, device-visible host memory the kernels store into (uncached on the device side)
void* WindowEngine::host_block(size_t bytes) {
  void* h = host_alloc((bytes + 15) & ~size_t(15), hipHostMallocCoherent | hipHostMallocMapped);
  std::memset(h, 0, bytes);
  return h;
}

hipEvent_t WindowEngine::mk_event(unsigned flags) {
  hipEvent_t e;
  HIPCHECK(hipEventCreateWithFlags(&e, flags));
  own_.events.push_back(e);
  return e;
}

hipStream_t WindowEngine::mk_stream(bool high_priority) {
  hipStream_t s;
  int lo = 0, hi = 0;
  if (high_priority) {
    HIPCHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIPCHECK(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, hi));
  } else {
    HIPCHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  }
  own_.streams.push_back(s);
  return s;
}

void WindowEngine::Owner::free_dev(void* p) {
  if (!p) return;
  dev.erase(std::find(dev.begin(), dev.end(), p));
  HIPCHECK(hipFree(p));
}

WindowEngine::Owner::~Owner() {
  for (hipEvent_t e : events) (void)hipEventDestroy(e);
  for (void* p : host) (void)hipHostFree(p);
  for (void* p : dev) (void)hipFree(p);
  for (hipStream_t s : streams) (void)hipStreamDestroy(s);
}

WindowEngine::WindowEngine(const EngineConfig& cfg) : cfg_(cfg) {
  if (cfg.sig_cap <= 0 || cfg.span_cap <= 0 || cfg.group_cap <= 0 || cfg.group_cap > 4096)
    throw std::invalid_argument("capacities out of range");
  if (cfg.sig_cap >= (1 << 27)) throw std::invalid_argument("sig_cap must be < 2^27 (top-3 key packing)");
  nb_ = std::max(2, cfg.n_buffers);
  max_ahead_ = std::min(nb_, std::max(1, cfg.max_ahead));
  if (cfg.user_cap <= 0 || cfg.user_cap > cfg.sig_cap) throw std::invalid_argument("user_cap must be in [1, sig_cap]");
  if (cfg.import_cap < 0 || cfg.xchg_cap < 0 || cfg.halo_ms < 0) throw std::invalid_argument("negative import sizes");
  if (cfg.halo_windows < 1 || cfg.halo_windows >= kMaxGens)
    throw std::invalid_argument("halo_windows must be in [1, 3] (resident generations)");
  gens_ = cfg.halo_ms > 0 ? 1 + cfg.halo_windows : 1;
  if (2LL * gens_ * ((long long)cfg.sig_cap + cfg.import_cap) >= (1LL << 27))
    throw std::invalid_argument("2 x generations x (sig_cap + import_cap) must be < 2^27 (top-3 key packing)");
  HIPCHECK(hipSetDevice(cfg.device));
  set_join_params(cfg.window_ms, cfg.threshold, cfg.fanout, cfg.group_mode);
  alloc();
}

void WindowEngine::set_join_params(double window_ms, double threshold, int fanout, int group_mode) {
  const int64_t ms = 1000000;
  int64_t outer = (int64_t)llround(window_ms * ms);
  if (outer <= 0) outer = 2000 * ms;
  if (outer >= (1LL << 35)) throw std::invalid_argument("window too large for top-3 key packing (< 34 s)");
  jp_.outer_ns = outer;
  const int64_t tw[4] = {outer, 100 * ms, 250 * ms, 500 * ms};
  for (int k = 0; k < 4; ++k) jp_.win_ns[k] = std::min(outer, tw[k]);
  const float cf[4] = {1.0f, 0.9f, 0.8f, 0.65f};
  for (int k = 0; k < 4; ++k) jp_.conf[k] = cf[k];
  jp_.threshold = threshold > 0 ? (float)threshold : 0.7f;
  if (fanout <= 0) fanout = 3;
  if (fanout > 3) throw std::invalid_argument("GPU join keeps at most 3 candidates per span");
  jp_.fanout = fanout;
  jp_.group_mode = group_mode;
  graphs_.clear();  // captured launches hold the old parameters
}

void WindowEngine::alloc() {
  const int64_t S = cfg_.span_cap, G = cfg_.group_cap;
  n_rows_ = cfg_.sig_cap + cfg_.import_cap;  // the join's rows: the window's records + imported rows
  const int64_t N = n_rows_;
  nblk_sig_ = decode_grid((int)N);
  nblk_span_ = decode_grid((int)S);
  // MISLO_ONE_STREAM=1: the window's copies on the compute stream (one HIP stream). With one
  // hardware queue (the agent's GPU_MAX_HW_QUEUES=1) the two streams' commands run in order on
  // that queue anyway, and the copy stream's first use maps another ~173 MB queue save area
  // (tools/rss_probe.py); the bench keeps the two streams (copy / compute overlap on 4 queues).
  const bool one_stream = env_int("MISLO_ONE_STREAM", 0) == 1;
  compute_ = mk_stream();
  copy_[0] = one_stream ? compute_ : mk_stream();
  spin_ = env_int("MISLO_SPIN_WAIT", 0) == 1;  // wait() polls its event instead of sleeping on it
  // Window overlap (engine.h): the front stage on a stream of its own. Not for an engine sized
  // for the exchange (its windows run the two-part serial chain), and switched off by init_comm.
  overlap_ = env_int("MISLO_WINDOW_OVERLAP", !one_stream) == 1 && !one_stream &&
             !(cfg_.xchg_cap > 0 && cfg_.import_cap > 0);
  if (overlap_) front_ = mk_stream();
  // Copy ahead (engine.h, submit_copy): window k's DMAs issued before window k - nb's results
  // are collected, behind a host wait for that window's front stage only. Overlapped windows only
  // (front_done exists there, and every reader of the data regions is joined into front_ before
  // it); MISLO_COPY_AHEAD=0|1 overrides the default.
  copy_ahead_ = overlap_ && env_int("MISLO_COPY_AHEAD", kCopyAheadDefault) == 1;
  // Copy lanes (engine.h, copylanes.h): a second copy stream, windows alternating, where windows
  // overlap. A window's own DMAs stay on one stream (one window split over the two streams
  // measured slower). Two lanes pay where a lane holds a backlog, i.e. where window k's DMAs are
  // queued a whole window before the link gets to them. With four buffers they are (the host
  // collects window k - 3 before it stages window k + 1: 0.399-0.403 ms per window against
  // 0.423-0.431 with one lane, profiles/copy_lanes/README.md): two lanes from the start. With
  // three they are only for a caller that runs the copy phase ahead of that collect (0.394-0.406
  // against the parent's 0.420-0.443 over three sessions; copying ahead on one lane, and two
  // lanes behind the collect, both tied with the parent: profiles/copy_ahead/README.md). So an
  // engine with three buffers starts on one lane, as every caller of submit() has it, and a
  // caller that will copy ahead says so once with take_copy_lanes() (lane_on_request_), before
  // its windows. MISLO_COPY_LANES=1|2 fixes the count either way.
  const char* lanes_env = getenv("MISLO_COPY_LANES");
  lanes_ = overlap_ && (lanes_env ? atoi(lanes_env) == 2 : nb_ >= 4) ? 2 : 1;
  lane_on_request_ = copy_ahead_ && !lanes_env && lanes_ == 1 && nb_ >= 3;
  copy_[1] = lanes_ == 2 ? mk_stream(env_int("MISLO_COPY_LANE_PRIO", 1) != 0) : copy_[0];
  slots_ = gens_ + (overlap_ ? 1 : 0);
  {
    // The span side of the chain (decode, partition, sort, the probe's work list) on a second
    // stream, overlapping the signal side's decode: on by default in the serial chain where the
    // streams have hardware queues to overlap on (not with MISLO_ONE_STREAM, the one-queue
    // agent); MISLO_SPAN_STREAM=0/1 overrides. At the default priority it measured 0.521-0.526
    // against 0.539-0.546 ms per window (K = 100, profiles/r5_probe/README.md); a high-priority
    // side stream (MISLO_SPAN_STREAM_PRIO=1, its own hardware-queue pool) measured 0.65.
    // With overlapped windows it is off by default: the front stage is off the critical path,
    // and a graph with a forked branch replays the branch on a stream of the runtime's own, so
    // copy, front, compute, side and those no longer fit the four hardware queues one each --
    // streams that share a queue wait for each other's copies and event waits. Measured 0.60
    // with the branch against 0.48 ms per window without (profiles/window_overlap/README.md).
    if (env_int("MISLO_SPAN_STREAM", !one_stream && !overlap_) == 1) enable_span_branch();
  }
  // one GPU: the window's tail (packet accumulate, timing) runs on the compute stream; a comm
  // stream of its own exists only with a communicator (init_comm). Every stream backs a
  // hardware queue, and each MI355X queue pins ~173 MB of host memory (its context save area,
  // measured: tools/rss_probe.py), so a single-GPU agent does without it.
  comm_stream_ = compute_;
  // device input block per buffer: [head (counts + labels) | framed ring records | user records | spans]
  const size_t head = (kHeadBytes + 4 * (size_t)G + 63) & ~size_t(63);
  off_kern_ = head;
  off_user_ = (off_kern_ + kern_bytes() + 63) & ~size_t(63);
  off_span_ = off_user_ + 64 * (size_t)cfg_.user_cap;
  in_bytes_ = off_span_ + 64 * (size_t)S;
  // per buffer: the comm stream gathers window k's results while window k + 1 computes
  const ResultLayout lay = layout();
  bufs_.assign(nb_, Buf{});
  for (Buf& buf : bufs_) {
    buf.in = dalloc<uint8_t>(in_bytes_, true);
    buf.head_host = static_cast<uint8_t*>(host_block(head));
    buf.packet_dev = dalloc<double>(kPacketLen, true);
    buf.packet_host = static_cast<double*>(host_block(kPacketLen * sizeof(double)));
    for (hipEvent_t* e : {&buf.head_done, &buf.compute_done, &buf.comm_done, &buf.front_done, &buf.xchg_done})
      *e = mk_event(kEvWait);
    for (hipEvent_t* e : {&buf.t_comp0, &buf.t_comp1, &buf.t_end}) *e = mk_event(hipEventDefault);  // timing
    buf.res_host = static_cast<uint8_t*>(host_block(lay.bytes()));
    buf.res_dev = dalloc<uint8_t>(lay.bytes(), true);
    buf.res = lay.view(buf.res_dev);
    buf.imp = cfg_.import_cap ? dalloc<SigRec>(cfg_.import_cap) : nullptr;
  }
  marks_.assign((size_t)copy_mark_slots(nb_), CopyMark{});
  for (CopyMark& m : marks_) {
    m.t_start = mk_event(hipEventDefault);
    m.h2d_done = mk_event(hipEventBlockingSync);  // the host sleeps on it, and it ends the copy's timed span
  }
  warm_.assign(kStageSlots * nb_, false);
  // pod metadata, ring accounting, the trace id -> hash table
  pod_sn_ = dalloc<uint32_t>(kPodRows, true);
  pod_host_ = static_cast<uint32_t*>(host_alloc(kPodRows * 4, hipHostMallocDefault));
  std::memset(pod_host_, 0, kPodRows * 4);
  trace_hash_ = dalloc<unsigned long long>(kTraceIdRows, true);
  // other GPUs' trace rows and the selection of this GPU's; the generations' state
  tmax_ = dalloc<unsigned long long>(1, true);
  remote_n_ = dalloc<uint32_t>(nb_, true);
  // the state both stages of a window touch: per buffer with overlapped windows, else one set
  for (int i = 0; i < (overlap_ ? nb_ : 1); ++i) {
    BufSet s{};
    s.rows = dalloc<int>(16, true);
    s.ring_state = dalloc<uint32_t>(kRsLen);
    s.gen = dalloc<GenMeta>(1);
    GenMeta g{};
    g.cur = (uint32_t)slots_ - 1;  // the first window's k_window_begin moves to slot 0
    for (int a = 0; a < kMaxGens; ++a) g.cut[a] = INT64_MAX;
    HIPCHECK(hipMemcpy(s.gen, &g, sizeof(g), hipMemcpyHostToDevice));
    s.s_part = dalloc<PartCodes>(S);
    s.s_part_base = dalloc<uint32_t>(kKeyTypes * kParts + 1);
    s.s_items = dalloc<uint32_t>(kKeyTypes * S);
    s.s_pre = dalloc<PreSpan>((size_t)kKeyTypes * S);
    s.s_rec = dalloc<SpanRec>(S);
    s.probe_work = dalloc<uint32_t>(kProbeWorkLen, true);
    s.top3 = dalloc<unsigned long long>(3 * S);
    s.cnt = dalloc<uint32_t>(S);
    s.gsum = dalloc<unsigned long long>((size_t)kGroupStripes * G * kSlots);
    s.gcnt = dalloc<uint32_t>((size_t)kGroupStripes * G * kSlots);
    s.hist = dalloc<uint32_t>(kSlots * kBuckets);
    s.status = dalloc<uint32_t>(kSlots * 3);
    s.misc = dalloc<unsigned long long>(kPacketMisc);
    s.dbg = dalloc<unsigned long long>(kPacketDbg);
    s.confusion = dalloc<uint32_t>(kMaxDomains * kMaxDomains);
    s.stats = dalloc<double>(32 * 32);
    s.stats_count = dalloc<double>(kMaxDomains);
    sets_.push_back(s);
  }
  for (int b = 0; b < nb_; ++b) {  // sets_ is complete: its elements no longer move
    bufs_[b].b = b;
    bufs_[b].set = &sets_[overlap_ ? b : 0];
    bufs_[b].gen_prev = sets_[overlap_ ? (b + nb_ - 1) % nb_ : 0].gen;
    bufs_[b].remote_n = remote_n_ + b;
  }
  sel_cnt_ = dalloc<uint32_t>(1024);
  sel_off_ = dalloc<uint32_t>(1024);
  xstride_ = sizeof(XRec) * (1 + (size_t)cfg_.xchg_cap);  // [24-byte header: row count | XRec rows]
  if (cfg_.xchg_cap) {
    xsend_ = dalloc<uint8_t>(xstride_, true);
    if (env_int("MISLO_SEL_TWO_PASS", 0) != 1) {  // the fused selection's ballot masks (segment 0's decode geometry)
      sel_stride_ = decode_sel_stride(n_rows_);
      sel_mask_ = dalloc<unsigned long long>((size_t)decode_grid(n_rows_) * (size_t)sel_stride_);
    }
  }
  // context table: every id the kernel or the host encoder can assign, HBM-resident
  ctx_tab_ = dalloc<uint32_t>((size_t)kCtxRows * 4, true);
  totals_ = dalloc<double>(kPacketLen, true);
  stats_acc_ = dalloc<double>(kStatsLen, true);
  p0_ = dalloc<double>(2 * kSlots * 16, true);  // the Beta prior's table, then the likelihood floor
  model_dev_ = dalloc<uint8_t>(sizeof(PosteriorModel), true);
  app_dev_ = dalloc<AppModel>(1, true);  // on = 0: no application evidence until set
  for (int i = 0; i < max_ahead_ + 2; ++i)
    model_host_.push_back(static_cast<uint8_t*>(host_alloc(sizeof(PosteriorModel), hipHostMallocDefault)));
  g_status_ = dalloc<uint8_t>(N);
  g_part_ = dalloc<PartCodes>(N);
  // other GPUs' rows decode in blocks of their own (<= 7 peers' exchange blocks)
  nblk_imp_ = cfg_.xchg_cap ? decode_grid(7 * cfg_.xchg_cap) : 0;
  g_part_blk_ = dalloc<uint32_t>((size_t)(nblk_sig_ + nblk_imp_) * kKeyTypes * kParts);
  g_part_off_ = dalloc<uint32_t>((size_t)(nblk_sig_ + nblk_imp_) * kKeyTypes * kParts);
  g_part_tot_ = dalloc<uint32_t>(kKeyTypes * kParts);
  // resident generations: rows, partition lists, list keys and offsets of the last gens_ windows,
  // over slots_ physical slots (one spare with overlapped windows: the next window's front stage
  // decodes into it while this window's back stage still reads the other gens_)
  g_part_base_ = dalloc<uint32_t>((size_t)slots_ * kBaseLen);
  g_items_ = dalloc<uint32_t>((size_t)slots_ * kKeyTypes * N);
  g_keys_ = dalloc<KeyTs>((size_t)slots_ * kKeyTypes * N);
  g_rec_ = dalloc<SigRec>((size_t)slots_ * N);
  // front-stage scratch (one window's front stage at a time, in stream order) and back-stage
  // scratch (likewise) stay single
  s_part_blk_ = dalloc<uint32_t>((size_t)nblk_span_ * kKeyTypes * kParts);
  s_part_off_ = dalloc<uint32_t>((size_t)nblk_span_ * kKeyTypes * kParts);
  s_part_tot_ = dalloc<uint32_t>(kKeyTypes * kParts);
  attrs_ = dalloc<float>(S * kSlots);
  conf_ = dalloc<float>(S);
  kernel_ms_ = dalloc<float>(S);
  HIPCHECK(hipDeviceSynchronize());
}

WindowEngine::~WindowEngine() {
  (void)hipDeviceSynchronize();
  for (auto& kv : graphs_) (void)hipGraphExecDestroy(kv.second);
  for (auto g : graph_defs_) (void)hipGraphDestroy(g);
  if (xcomm_) ncclCommDestroy(xcomm_);
  if (comm_) ncclCommDestroy(comm_);
  for (auto& r : registered_) (void)hipHostUnregister(const_cast<uint8_t*>(r.first));
}  // then own_: events, memory, streams

void WindowEngine::enable_span_branch() {
  if (branch_) return;
  side_ = mk_stream(env_int("MISLO_SPAN_STREAM_PRIO", 0) == 1);  // 1 = the highest priority
  for (hipEvent_t* e : {&ev_fork_, &ev_sigbase_, &ev_spans_}) *e = mk_event(hipEventDisableTiming);
  xspan_ = env_int("MISLO_XCHG_SPAN_SIDE", 1) != 0;  // 0: the exchange path's span side in part 2
  branch_ = true;
}

SignalCols WindowEngine::sig_cols(const Buf& buf) const {
  return SignalCols{g_rec_, g_status_, g_part_, g_items_, g_keys_, g_part_base_, buf.set->gen, (int64_t)n_rows_, gens_,
                    slots_};
}
SpanCols WindowEngine::span_cols(const Buf& buf) const { return SpanCols{buf.set->s_rec, buf.set->s_part}; }

bool WindowEngine::register_host(const void* ptr, size_t bytes) {
  if (!ptr || !bytes) return false;
  if (registered(ptr, bytes)) return true;
  if (hipHostRegister(const_cast<void*>(ptr), bytes, hipHostRegisterDefault) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  registered_.emplace_back(static_cast<const uint8_t*>(ptr), bytes);
  return true;
}

bool WindowEngine::registered(const void* p, size_t n) const {
  const uint8_t* q = static_cast<const uint8_t*>(p);
  for (const auto& r : registered_)
    if (q >= r.first && q + n <= r.first + r.second) return true;
  return false;
}

// DMA a window's segments of one kind back to back into dst (device); unregistered segments go
// through pinned staging (one host memcpy, then the DMA). Returns the bytes placed.
size_t WindowEngine::dma(const std::vector<Seg>& segs, uint8_t* dst, size_t cap, uint8_t*& staging, size_t& st_off,
                         hipStream_t st) {
  size_t off = 0;
  for (const Seg& s : segs) {
    if (!s.bytes) continue;
    if (off + s.bytes > cap) throw std::invalid_argument("window input exceeds the engine's capacity");
    const void* src = s.ptr;
    if (!registered(s.ptr, s.bytes)) {
      if (!staging) staging = static_cast<uint8_t*>(host_alloc(in_bytes_ - off_kern_, hipHostMallocDefault));
      std::memcpy(staging + st_off, s.ptr, s.bytes);
      src = staging + st_off;
      st_off += s.bytes;
      staged_bytes_ += s.bytes;
    } else {
      direct_bytes_ += s.bytes;
    }
    HIPCHECK(hipMemcpyAsync(dst + off, src, s.bytes, hipMemcpyHostToDevice, st));
    off += s.bytes;
  }
  return off;
}

// Window w's completion event, for a window copied_ does not know copied yet: its slot's event
// is still its own (CopiedUpTo, copylanes.h; a slot is recorded again 2 nb windows on, CopyMark).
bool WindowEngine::copied_ready(int64_t w, bool block) {
  const hipEvent_t ev = mark(w).h2d_done;
  if (block) {
    HIPCHECK(hipEventSynchronize(ev));
    return true;
  }
  const hipError_t e = hipEventQuery(ev);
  if (e == hipErrorNotReady) return false;
  HIPCHECK(e);
  return true;
}

bool WindowEngine::h2d_done(int64_t k) {
  if (k < 0 || k >= copied_windows()) return false;  // not queued: nothing of it has been copied
  return copied_.done(k, lanes_, [this](int64_t w) { return copied_ready(w, false); });
}

void WindowEngine::wait_h2d(int64_t k) {
  if (k < 0 || k >= copied_windows()) throw std::invalid_argument("wait_h2d: the window has not been submitted");
  copied_.done(k, lanes_, [this](int64_t w) { return copied_ready(w, true); });
}

// The head of a window: the accumulators reset, the next generation slot, the window's rows.
void WindowEngine::run_begin(const Buf& buf, hipStream_t st) {
  const BufSet& s = *buf.set;
  const int S = cfg_.span_cap, G = cfg_.group_cap;
  FillList fl{};
  auto add = [&](void* p, size_t bytes, uint32_t v) { fl.seg[fl.count++] = FillSeg{(uint32_t*)p, (uint32_t)(bytes / 4), v}; };
  add(s.hist, kSlots * kBuckets * 4, 0);
  add(s.status, kSlots * 3 * 4, 0);
  add(s.misc, kPacketMisc * 8, 0);
  add(s.dbg, kPacketDbg * 8, 0);
  add(s.confusion, kMaxDomains * kMaxDomains * 4, 0);
  add(s.stats, 32 * 32 * 8, 0);
  add(s.stats_count, kMaxDomains * 8, 0);
  add(s.top3, 3 * (size_t)S * 8, 0xFFFFFFFFu);
  add(s.cnt, (size_t)S * 4, 0);
  add(s.gsum, (size_t)kGroupStripes * G * kSlots * 8, 0);
  add(s.gcnt, (size_t)kGroupStripes * G * kSlots * 4, 0);
  add(buf.res.sli, (size_t)G * 6 * 4, 0);  // + the application retrieval counts (app) and late breaches (late)
  // + the next generation slot and the halo cut-offs (the finished window's tmax is read before
  // its reset), the ring state, no other GPUs' rows until merged, the window's rows
  launch_window_begin(fl, s.gen, buf.gen_prev, tmax_, gens_, slots_, (long long)llround(cfg_.halo_ms * 1e6),
                      s.ring_state, buf.remote_n, buf.counts(), n_rows_, s.rows, st);
}

// Part 1 of a window: accumulators, definitions, the decode of the window's records and the
// halo it imported; with the GPU exchange, this window's trace-tagged rows for the others.
void WindowEngine::run_part1(const Buf& buf, hipStream_t st, bool xchg) {
  const BufSet& s = *buf.set;
  const int* counts = buf.counts();
  const int N = n_rows_;
  if (!(xchg && xspan_)) run_begin(buf, st);  // else its own launch (submit: Stage::XchgHead)
  // the span branch in the one-GPU chain: forked inside the window's graph and joined before the
  // probe. With the exchange, forked inside part 1's graph and joined before the exchange it
  // measured 0.76 against 0.62 ms per window (bench.py --rccl-self); there the span side is a
  // graph of its own on side_ instead (xspan_, submit: Stage::XchgHead and Stage::XchgSpans)
  if (branch_ && !xchg) run_span_branch(buf, st);
  const TraceIds tt{trace_hash_, kTraceIdRows};
  launch_ring_defs(buf.in + off_kern_, counts, cfg_.sig_cap, ctx_tab_, kCtxRows, pod_sn_, kPodRows, tt, s.ring_state,
                   st);
  const bool fused_sel = xchg && sel_mask_;  // the selection's count and masks left by the decode
  launch_decode_window(buf.in + off_kern_, buf.in + off_user_, counts, s.rows, N, buf.imp, ctx_tab_, (int)kCtxRows, tt,
                       s.ring_state, tmax_, pod_sn_, kPodRows, sig_cols(buf), s.hist, s.status, g_part_blk_, s.misc, st,
                       0, 0, 0, rec_shard_rank(), rec_shard_world(), fused_sel ? sel_cnt_ : nullptr,
                       fused_sel ? sel_mask_ : nullptr, sel_stride_);
  // this window's warn-level trace-tagged rows, as the other GPUs will import them
  if (fused_sel)
    launch_select_masked(sig_cols(buf), s.rows, N, sel_cnt_, sel_off_, sel_mask_, sel_stride_,
                         reinterpret_cast<XRec*>(xsend_ + sizeof(XRec)), reinterpret_cast<uint32_t*>(xsend_),
                         (uint32_t)cfg_.xchg_cap, st, s.dbg + kDbgXchgDropped);
  else if (xchg)
    launch_select(sig_cols(buf), s.rows, counts, N, sel_cnt_, sel_off_, reinterpret_cast<XRec*>(xsend_ + sizeof(XRec)),
                  reinterpret_cast<uint32_t*>(xsend_), (uint32_t)cfg_.xchg_cap, st, s.dbg + kDbgXchgDropped);
}

// Part 2, first half: [the other GPUs' rows] -> partition -> spans (unless they ran beside part 1).
void WindowEngine::run_join_front(const Buf& buf, hipStream_t st, bool xchg) {
  const BufSet& s = *buf.set;
  const int N = n_rows_;
  if (xchg) {
    const TraceIds tt{trace_hash_, kTraceIdRows};
    launch_decode_window(buf.in + off_kern_, buf.in + off_user_, buf.counts(), s.rows, N, buf.imp, ctx_tab_,
                         (int)kCtxRows, tt, s.ring_state, tmax_, pod_sn_, kPodRows, sig_cols(buf), s.hist, s.status,
                         g_part_blk_, s.misc, st, 1, nblk_imp_, nblk_sig_, rec_shard_rank(), rec_shard_world());
  }
  const bool branched = branch_ && !xchg;
  // with the span branch: the signal bases are what the branch's probe work list waits for
  hipEvent_t sig_base = branched ? ev_sigbase_ : nullptr;
  // without the span branch: the span side first, so the signal scatter's launch can build the
  // probe's work list next to it (it needs both sides' list offsets); with the exchange and
  // xspan_ the span side ran on side_ next to part 1 (submit: Stage::XchgSpans)
  if (!branched && !(xchg && xspan_)) run_spans(buf, st);
  const uint32_t* wspan = branched ? nullptr : s.s_part_base;
  const JoinParams* wjp = branched ? nullptr : &jp_;
  uint32_t* wlist = branched ? nullptr : s.probe_work;
  launch_partition_sig(sig_cols(buf), s.rows, N, nblk_sig_ + (xchg ? nblk_imp_ : 0), g_part_blk_, g_part_off_,
                       g_part_tot_, st, xchg ? nblk_sig_ : 0, sig_base, wspan, wjp, wlist);
  if (branched) {  // the work list needs the signal bases just recorded; then join
    HIPCHECK(hipStreamWaitEvent(side_, ev_sigbase_, 0));
    launch_probe_work(s.s_part_base, sig_cols(buf), jp_, s.probe_work, side_);
    HIPCHECK(hipEventRecord(ev_spans_, side_));
    HIPCHECK(hipStreamWaitEvent(st, ev_spans_, 0));  // spans sorted, work list built
  }
}

// Part 2, second half: join (this window's spans x every generation's visible rows) ->
// posterior -> packet.
void WindowEngine::run_join_back(const Buf& buf, int n_groups, bool with_labels, bool learn, hipStream_t st) {
  const BufSet& s = *buf.set;
  const ResultViewT<uint8_t>& r = buf.res;
  const int* counts = buf.counts();
  const int32_t* labels = reinterpret_cast<const int32_t*>(buf.in + kHeadBytes);
  const int S = cfg_.span_cap, G = cfg_.group_cap;
  launch_probe(span_cols(buf), s.s_items, s.s_part_base, sig_cols(buf), S, jp_, s.top3, s.cnt, n_groups, s.gsum, s.gcnt,
               s.dbg, s.probe_work, s.s_pre, st);
  launch_finalize(counts + 1, S, s.top3, s.cnt, sig_cols(buf), span_cols(buf), jp_, nullptr, attrs_, conf_, kernel_ms_,
                  n_groups, s.gsum, s.gcnt, r.feat, s.dbg, st);
  const PosteriorModel* pm = reinterpret_cast<const PosteriorModel*>(model_dev_);
  if (learn)
    launch_posterior_stats(r.feat, counts + 2, G, pm, with_labels ? labels : nullptr, r.post, r.pred, r.gconf, r.evbits,
                           s.confusion, labels, nullptr, s.stats, s.stats_count, st, app_dev_, r.app);
  else
    launch_posterior(r.feat, counts + 2, G, pm, with_labels ? labels : nullptr, r.post, r.pred, r.gconf, r.evbits,
                     s.confusion, st, app_dev_, r.app);
  if (!comm_) {  // one GPU: the whole tail here (see k_window_end)
    const size_t res16 = (result_bytes() + 15) / 16;
    const int g = (int)std::max<size_t>((kPacketLen + 255) / 256, std::min<size_t>(64, (res16 + 255) / 256));
    hipLaunchKernelGGL(k_window_end, dim3(g), dim3(256), 0, st, s.hist, s.status, s.misc, s.dbg, s.confusion, s.stats,
                       s.stats_count, s.ring_state, buf.packet_dev, totals_, buf.packet_host,
                       reinterpret_cast<const uint4*>(buf.res_dev), reinterpret_cast<uint4*>(buf.res_host), res16);
    return;
  }
  hipLaunchKernelGGL(k_pack, dim3((kPacketLen + 255) / 256), dim3(256), 0, st, s.hist, s.status, s.misc, s.dbg,
                     s.confusion, s.stats, s.stats_count, s.ring_state, buf.packet_dev);
}

// The span side of the chain: decode, partition, span sort (inputs: the span DMA and the reset
// accumulators only).
void WindowEngine::run_spans(const Buf& buf, hipStream_t st) {
  const BufSet& s = *buf.set;
  const int* counts = buf.counts();
  const int S = cfg_.span_cap, G = cfg_.group_cap;
  const SpanMap sm{1, buf.res.sli, G, cfg_.ttft_slo_ms, cfg_.shard_rank, cfg_.shard_world,
                   s.gen, buf.res.app, buf.res.late};
  launch_decode_spans(buf.in + off_span_, counts + 1, S, span_cols(buf), s_part_blk_, ctx_tab_, (int)kCtxRows, st, &sm);
  launch_partition(s.s_part, counts + 1, S, nblk_span_, s_part_blk_, s_part_off_, s_part_tot_, s.s_part_base, s.s_items,
                   st);
  launch_span_sort(span_cols(buf), s.s_items, s.s_part_base, s.s_pre, st);
}

// Fork from `st` (after k_window_begin): the span side on side_. run_join_front continues the
// branch once the signal side's partition bases exist -- the probe work list reads both sides'
// bases and time ranges -- and joins it before the probe (ev_spans_). Native 64-byte spans never
// read the context table, so the branch does not wait for k_ring_defs.
void WindowEngine::run_span_branch(const Buf& buf, hipStream_t st) {
  HIPCHECK(hipEventRecord(ev_fork_, st));
  HIPCHECK(hipStreamWaitEvent(side_, ev_fork_, 0));
  run_spans(buf, side_);
}

// Launch a chain part eagerly, or through its captured graph (captured on the buffer's second
// use; the first use runs eagerly so lazily initialised state is out of the capture).
void WindowEngine::launch_part(Stage part, const Buf& buf, int n_groups, bool with_labels, bool learn) {
  // the stream the part runs (and is captured) on
  hipStream_t cs = part == Stage::XchgSpans ? side_ : part == Stage::Front ? front_ : compute_;
  auto run = [&] {
    switch (part) {
      case Stage::Window:  // the whole window in one graph (no exchange)
        run_part1(buf, cs, false);
        run_join_front(buf, cs, false);
        return run_join_back(buf, n_groups, with_labels, learn, cs);
      case Stage::Records: return run_part1(buf, cs, true);
      case Stage::Join:
        run_join_front(buf, cs, true);
        return run_join_back(buf, n_groups, with_labels, learn, cs);
      case Stage::XchgSpans: return run_spans(buf, cs);
      case Stage::XchgHead: return run_begin(buf, cs);
      case Stage::Front:
        run_part1(buf, cs, false);
        return run_join_front(buf, cs, false);
      case Stage::Back: return run_join_back(buf, n_groups, with_labels, learn, cs);
    }
  };
  if (!cfg_.use_graphs) return run();
  // the front stage does not depend on the incident groups, the labels or the learning flag
  const int slot = buf.b * kStageSlots + (int)part;
  auto key = part == Stage::Front ? std::make_tuple(slot, 0, false, false)
                                  : std::make_tuple(slot, n_groups, with_labels, learn);
  auto it = graphs_.find(key);
  if (it == graphs_.end() && !warm_[slot]) {
    run();
    warm_[slot] = true;
    return;
  }
  if (it == graphs_.end()) {
    hipGraph_t g;
    HIPCHECK(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
    run();
    HIPCHECK(hipStreamEndCapture(cs, &g));
    hipGraphExec_t ex;
    HIPCHECK(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
    graph_defs_.push_back(g);
    it = graphs_.emplace(key, ex).first;
  }
  HIPCHECK(hipGraphLaunch(it->second, cs));
}

void WindowEngine::merge_remote(const Buf& buf, const uint8_t* blocks, size_t stride, int world, int me,
                                hipStream_t st) {
  launch_remote_merge(blocks, stride, world, me, buf.imp, buf.remote_n, (uint32_t)cfg_.import_cap, cfg_.xchg_cap, st,
                      buf.set->dbg + kDbgXchgDropped);
  launch_window_rows(buf.counts(), buf.remote_n, n_rows_, buf.set->rows, buf.set->gen, st);
}

void WindowEngine::refit(const double* add) {
  launch_refit_nb(stats_acc_, add, p0_, cfg_.alpha, cfg_.prior_pseudo, cfg_.n_dom,
                  reinterpret_cast<PosteriorModel*>(model_dev_), compute_, cfg_.inv_temp, cfg_.min_count,
                  p0_ + kSlots * 16, cfg_.cap_dom, cfg_.lik_ceil);
}

// The second lane for a caller that copies ahead (alloc()): created here, so an engine that never
// copies ahead keeps its hardware queue and memory. The first large DMA that runs while the other
// lane's is still in flight goes to a DMA engine the process has not used yet, and setting that up
// blocks the issuing thread for ~6 ms once (profiles/copy_lanes/README.md: "the second lane's
// first large DMA"; a warm-up copy on the idle lane alone did not absorb it,
// profiles/copy_ahead/README.md). A lane used from the engine's first windows pays that in the
// caller's warm-up; this lane would pay it in the first window copied ahead, so it pays here:
// window-sized copies into scratch on both lanes at once. Windows before this call all ran on
// lane 0 in order, so "copied up to k" keeps following from windows k and k - 1
// (tests/native/copyahead_host_check.cpp).
bool WindowEngine::take_copy_lanes() {
  if (!lane_on_request_ || copy_open_) return lanes_ == 2;
  lane_on_request_ = false;
  HIPCHECK(hipSetDevice(cfg_.device));
  const hipStream_t lane = mk_stream(env_int("MISLO_COPY_LANE_PRIO", 1) != 0);
  const size_t n = std::min<size_t>(in_bytes_ - off_kern_, size_t(64) << 20);
  void *h = nullptr, *d = nullptr;
  hipError_t e = hipHostMalloc(&h, 2 * n, hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc(&d, 2 * n);
  if (e == hipSuccess) {
    std::memset(h, 0, 2 * n);
    uint8_t *hp = static_cast<uint8_t*>(h), *dp = static_cast<uint8_t*>(d);
    for (int round = 0; round < 2 && e == hipSuccess; ++round) {
      e = hipMemcpyAsync(dp, hp, n, hipMemcpyHostToDevice, copy_[0]);
      if (e == hipSuccess) e = hipMemcpyAsync(dp + n, hp + n, n, hipMemcpyHostToDevice, lane);
    }
    const hipError_t e0 = hipStreamSynchronize(copy_[0]), e1 = hipStreamSynchronize(lane);
    if (e == hipSuccess) e = e0 != hipSuccess ? e0 : e1;
  }
  if (d) (void)hipFree(d);
  if (h) (void)hipHostFree(h);
  HIPCHECK(e);
  copy_[1] = lane;
  lanes_ = 2;
  return true;
}

void WindowEngine::submit(int64_t k, const WindowInput& in, bool with_labels, bool learn) {
  submit_copy(k, in);
  submit_chain(k, in.n_groups, with_labels, learn);
}

void WindowEngine::submit_copy(int64_t k, const WindowInput& in) {
  Lap whole;
  if (k != submitted_) throw std::invalid_argument("windows must be submitted in order");
  if (copy_open_) throw std::logic_error("submit_copy: the window's chain phase has not been queued");
  const int n_groups = in.n_groups;
  if (n_groups < 0 || n_groups > cfg_.group_cap) throw std::invalid_argument("n_groups exceeds group capacity");
  size_t kb = 0, ub = 0, sb = 0;
  for (const Seg& s : in.kernel) kb += s.bytes;
  for (const Seg& s : in.user) ub += s.bytes;
  for (const Seg& s : in.spans) sb += s.bytes;
  // what the kernels will assume, checked on the host before anything is queued
  if (in.user_rec != 64 && in.user_rec != 32 && in.user_rec != 24 && in.user_rec != 16)
    throw std::invalid_argument("user records are 64, 32, 24 or 16 bytes");
  if (kb % kRecStride || ub % in.user_rec || sb % 64) throw std::invalid_argument("segments must hold whole records");
  // kernel rows: every slot of every batch record (definitions and pads become holes)
  const size_t n_k = kb / kRecStride * kBatchSlots, n_u = ub / in.user_rec, n_s = sb / 64;
  if (n_k + n_u > (size_t)cfg_.sig_cap || n_u > (size_t)cfg_.user_cap || n_s > (size_t)cfg_.span_cap)
    throw std::invalid_argument("window exceeds the engine's capacity (events / user records / spans)");
  Buf& buf = bufs_[k % nb_];
  const CopyMark& mk = mark(k);
  // host back-pressure: at most max_ahead windows queued beyond the one computing. Copying ahead
  // leaves it to the chain phase: the DMAs below collide with the front stage of window k - nb only
  Lap phase;
  if (!copy_ahead_ && k >= max_ahead_) HIPCHECK(hipEventSynchronize(bufs_[(k - max_ahead_) % nb_].compute_done));
  // the pinned head / staging of the buffer were last read by the DMAs of window k - nb (on
  // whichever lane they ran) and by its head load; those DMAs also wrote the device block last
  if (k >= nb_) {
    HIPCHECK(hipEventSynchronize(mark(k - nb_).h2d_done));
    copied_.reused(k, nb_);  // every window <= k - nb has been copied (their slots are re-recorded later still)
    HIPCHECK(hipEventSynchronize(buf.head_done));
    // the data regions of the device block (ring bytes, user records, spans) are read by the
    // front stage alone -- definitions, decode, span decode; a span branch is joined into front_
    // before the event -- and the back stage reads the head only, which the head load writes on
    // front_ behind its own wait for the back stage of window k - 2
    if (copy_ahead_) HIPCHECK(hipEventSynchronize(buf.front_done));
  }
  phase(wait_us_);
  int32_t* c = reinterpret_cast<int32_t*>(buf.head_host);
  std::memset(c, 0, kHeadBytes);
  c[0] = (int32_t)(n_k + n_u);
  c[1] = (int32_t)n_s;
  c[2] = n_groups;
  c[4] = (int32_t)(uint32_t)(uint64_t)in.bases[0];
  c[5] = (int32_t)(uint32_t)((uint64_t)in.bases[0] >> 32);
  c[6] = in.user_rec;  // user-space record bytes
  c[7] = 64;           // 64-byte spans
  for (int q = 1; q < 4; ++q) {
    c[8 + 2 * (q - 1)] = (int32_t)(uint32_t)(uint64_t)in.bases[q];
    c[9 + 2 * (q - 1)] = (int32_t)(uint32_t)((uint64_t)in.bases[q] >> 32);
  }
  c[15] = (int32_t)n_k;
  int32_t* lab = reinterpret_cast<int32_t*>(buf.head_host + kHeadBytes);
  for (int g = 0; g < cfg_.group_cap; ++g) lab[g] = (in.labels && g < n_groups) ? in.labels[g] : -1;
  // The window's DMAs: the BPF ring's bytes, the user-space records and the spans, back to back
  // on the window's copy lane between one start marker and one completion event; the head is
  // loaded on the compute stream (submit_chain). The copy stream waits for nothing on the device:
  // the regions' previous reader, window k - nb, is through with them, because the host waited
  // above -- for its front_done when copying ahead, else for compute_done of window
  // k - max_ahead_, max_ahead_ <= nb_ (constructor), and every stage that reads the block (front_,
  // side_) is joined into the in-order compute stream before that event. A wait on the copy
  // stream costs a queue hand-off with the link idle.
  const hipStream_t cs = copy_[copy_lane(k, lanes_)];
  HIPCHECK(hipEventRecord(mk.t_start, cs));
  size_t st_off = 0;
  Lap part;  // DMA issue: ring bytes, head (nothing: not on the copy stream), user records, spans
  dma(in.kernel, buf.in + off_kern_, kern_bytes(), buf.staging, st_off, cs);
  part(split_us_[0]);
  part(split_us_[1]);
  dma(in.user, buf.in + off_user_, 64 * (size_t)cfg_.user_cap, buf.staging, st_off, cs);
  part(split_us_[2]);
  dma(in.spans, buf.in + off_span_, 64 * (size_t)cfg_.span_cap, buf.staging, st_off, cs);
  part(split_us_[3]);
  HIPCHECK(hipEventRecord(mk.h2d_done, cs));
  phase(dma_us_);
  copy_open_ = true;
  copy_groups_ = n_groups;
  whole(issue_us_);
}

void WindowEngine::submit_chain(int64_t k, int n_groups, bool with_labels, bool learn) {
  Lap whole;
  if (!copy_open_ || k != submitted_) throw std::logic_error("submit_chain: not the window submit_copy queued last");
  if (n_groups != copy_groups_) throw std::invalid_argument("submit_chain: n_groups differs from the copy phase's");
  Buf& buf = bufs_[k % nb_];
  const CopyMark& mk = mark(k);
  Lap phase;
  // host back-pressure (see submit_copy, which waited already unless it copied ahead)
  if (copy_ahead_ && k >= max_ahead_) HIPCHECK(hipEventSynchronize(bufs_[(k - max_ahead_) % nb_].compute_done));
  phase(wait_us_);
  // the stream of the window's head and front half: front_ with overlapped windows (never with
  // the exchange: overlap_ is off for an engine sized for it or holding a communicator). It waits
  // for this window's own DMAs only, whatever the other lane is doing.
  hipStream_t fs = overlap_ ? front_ : compute_;
  HIPCHECK(hipStreamWaitEvent(fs, mk.h2d_done, 0));
  // overlapped: the front stage of window k starts once the back stage of window k - 2 ended. It
  // overwrites the generation slot that stage probed as its oldest, and (two buffers) the buffer
  // set and the head that stage read; with it at most one window's back stage runs beside a front.
  if (overlap_ && k >= 2) HIPCHECK(hipStreamWaitEvent(fs, bufs_[(k - 2) % nb_].compute_done, 0));
  HIPCHECK(hipStreamWaitEvent(compute_, buf.comm_done, 0));  // the buffer's packet no longer reduced / read
  const bool injected = !inject_.empty();
  if (injected) {
    // rows as the other GPUs would have delivered them (tests, replays): on the device before the
    // window's timed chain (the all-gather they stand for is not the chain's), after window k-1's
    // merge read the receive buffer (compute stream order); the host copy is released below
    HIPCHECK(hipMemcpyAsync(xrecv_, inject_.data(), inject_.size(), hipMemcpyHostToDevice, compute_));
    HIPCHECK(hipStreamSynchronize(compute_));
  }
  HIPCHECK(hipEventRecord(buf.t_comp0, fs));
  // the head (counts, epoch bases, labels: < 1 KiB) by a kernel load from pinned host memory on
  // the compute stream (the front stream with overlapped windows): a small hipMemcpyAsync H2D is
  // written by the host through the BAR and blocks this thread, and a kernel on the copy stream
  // put ~25 us of queue hand-offs between the window's DMAs (measured); the compute stream has
  // the slack
  to_host(buf.head_host, buf.in, off_kern_, fs);
  HIPCHECK(hipEventRecord(buf.head_done, fs));
  if (cfg_.device_refit && k >= nb_) {
    // fold window k - nb's all-reduced statistics (the buffer's last packet) and refit before
    // window k: a deterministic prequential lag of nb, identical on every rank
    refit(buf.packet_dev + kStatsOff);
    ++folded_;
  }
  const bool xchg = exchange() || injected;
  phase(pre_us_);
  if (overlap_) {
    if (xchg) throw std::logic_error("the exchange path does not run with overlapped windows");
    // two stages, two graphs: the front on front_, the back on compute_ once the front ended
    launch_part(Stage::Front, buf, n_groups, with_labels, learn);
    HIPCHECK(hipEventRecord(buf.front_done, front_));
    HIPCHECK(hipStreamWaitEvent(compute_, buf.front_done, 0));
    launch_part(Stage::Back, buf, n_groups, with_labels, learn);
  } else if (!xchg) {
    launch_part(Stage::Window, buf, n_groups, with_labels, learn);
  } else {
    if (xspan_) {
      // the window head, then the span side (decode, partition, sort: it reads only the span DMA
      // and the reset accumulators) on side_ while part 1 decodes the records; joined before part 2
      launch_part(Stage::XchgHead, buf, n_groups, with_labels, learn);
      HIPCHECK(hipEventRecord(ev_fork_, compute_));
      HIPCHECK(hipStreamWaitEvent(side_, ev_fork_, 0));
      launch_part(Stage::XchgSpans, buf, n_groups, with_labels, learn);
      HIPCHECK(hipEventRecord(ev_spans_, side_));
    }
    launch_part(Stage::Records, buf, n_groups, with_labels, learn);
    // the exchange sits between the window's two halves: every GPU's trace rows of THIS window
    if (injected) {  // rows as the other GPUs would have delivered them (copied above)
      merge_remote(buf, xrecv_, inject_stride_, inject_world_, inject_me_, compute_);
      inject_.clear();
    } else if (xcomm_) {
      // on the compute stream, over the exchange's own communicator (each communicator is used
      // on one stream only, so each keeps one issue order on every rank): part 2 follows the
      // merge in stream order, with no hand-off between hardware queues on the window's critical
      // path (each such hop idled the compute queue 20-45 us, profiles/r5_multigpu/)
      NCCLCHECK(ncclAllGather(xsend_, xrecv_, xstride_, ncclUint8, xcomm_, compute_));
      merge_remote(buf, xrecv_, xstride_, world_, rank_, compute_);
    } else {
      // MISLO_XCHG_STREAM=comm: the exchange on the comm stream with the window's other
      // collectives: the compute stream hands over after part 1 and waits for the merge
      HIPCHECK(hipEventRecord(buf.xchg_done, compute_));
      HIPCHECK(hipStreamWaitEvent(comm_stream_, buf.xchg_done, 0));
      NCCLCHECK(ncclAllGather(xsend_, xrecv_, xstride_, ncclUint8, comm_, comm_stream_));
      merge_remote(buf, xrecv_, xstride_, world_, rank_, comm_stream_);
      HIPCHECK(hipEventRecord(buf.xchg_done, comm_stream_));
      HIPCHECK(hipStreamWaitEvent(compute_, buf.xchg_done, 0));
    }
    if (xspan_) HIPCHECK(hipStreamWaitEvent(compute_, ev_spans_, 0));
    launch_part(Stage::Join, buf, n_groups, with_labels, learn);
  }
  phase(launch_us_);
  // per-incident results of this window (the buffers are reused by the next window); one GPU:
  // copied by the graph's k_window_end
  const size_t res_bytes = result_bytes();
  if (comm_) to_host(buf.res_dev, buf.res_host, res_bytes, compute_);
  HIPCHECK(hipEventRecord(buf.t_comp1, compute_));
  HIPCHECK(hipEventRecord(buf.compute_done, compute_));
  HIPCHECK(hipStreamWaitEvent(comm_stream_, buf.compute_done, 0));
  if (comm_) {
    // one group: the node-wide packet and the node-wide incident list. The ring accounting at
    // the packet's tail stays this GPU's own (each GPU is a consumer of its rings: its first busy
    // record, its records), so it is left out of the sum.
    NCCLCHECK(ncclGroupStart());
    NCCLCHECK(ncclAllReduce(buf.packet_dev, buf.packet_dev, kPacketLen - kPacketRing, ncclFloat64, ncclSum, comm_,
                            comm_stream_));
    NCCLCHECK(ncclAllGather(buf.res_dev, buf.res_all_dev, res_bytes, ncclUint8, comm_, comm_stream_));
    NCCLCHECK(ncclGroupEnd());
    to_host(buf.res_all_dev, buf.res_all_host, res_bytes * world_, comm_stream_);
    hipLaunchKernelGGL(k_accumulate, dim3((kPacketLen + 255) / 256), dim3(256), 0, comm_stream_, buf.packet_dev,
                       totals_, kPacketLen, buf.packet_host);
  }
  HIPCHECK(hipEventRecord(buf.t_end, comm_stream_));
  HIPCHECK(hipEventRecord(buf.comm_done, comm_stream_));
  ++submitted_;
  copy_open_ = false;
  phase(tail_us_);
  whole(issue_us_);
  ++issue_n_;
}

bool WindowEngine::query(int64_t k) {
  const hipError_t e = hipEventQuery(bufs_[k % nb_].comm_done);
  if (e == hipSuccess) return true;
  if (e == hipErrorNotReady) return false;
  HIPCHECK(e);
  return false;
}

void WindowEngine::wait(int64_t k) {
  if (spin_) {  // poll: no interrupt wake-up latency (flat-out benchmarking; costs a core)
    while (!query(k)) {
    }
    return;
  }
  HIPCHECK(hipEventSynchronize(bufs_[k % nb_].comm_done));
}

std::vector<float> WindowEngine::copy_ms(int64_t k) {
  // [window k's DMA span, window k-1's last DMA's end to window k's first DMA's start]. One lane:
  // the copy's duration and the copy stream's idle time before it. Two lanes: windows k-1 and k
  // copy side by side and share the link, so the span is longer than the bytes alone would take
  // and the second value is negative where they overlap.
  const CopyMark& mk = mark(k);
  float dur = 0.f, gap = -1.f;
  HIPCHECK(hipEventSynchronize(mk.h2d_done));
  HIPCHECK(hipEventElapsedTime(&dur, mk.t_start, mk.h2d_done));
  if (k >= 1) HIPCHECK(hipEventElapsedTime(&gap, mark(k - 1).h2d_done, mk.t_start));
  return {dur, gap};
}

std::pair<float, float> WindowEngine::window_ms(int64_t k) {
  const Buf& buf = bufs_[k % nb_];
  float total = 0.f, comp = 0.f;
  HIPCHECK(hipEventSynchronize(buf.t_end));
  HIPCHECK(hipEventElapsedTime(&total, mark(k).t_start, buf.t_end));
  HIPCHECK(hipEventElapsedTime(&comp, buf.t_comp0, buf.t_comp1));
  return {total, comp};
}

void WindowEngine::set_model_bytes(const void* bytes, size_t n) {
  if (n != sizeof(PosteriorModel)) throw std::invalid_argument("model image must be POSTERIOR_MODEL_BYTES bytes");
  // a pinned staging slot not read by any queued copy: at most max_ahead windows are queued
  uint8_t* h = model_host_[model_slot_++ % model_host_.size()];
  std::memcpy(h, bytes, n);
  HIPCHECK(hipMemcpyAsync(model_dev_, h, n, hipMemcpyHostToDevice, compute_));
}

void WindowEngine::set_app_model(const void* bytes, size_t n) {
  if (n != sizeof(AppModel)) throw std::invalid_argument("application model must be APP_MODEL_BYTES bytes");
  uint8_t* h = model_host_[model_slot_++ % model_host_.size()];  // pinned slots hold a PosteriorModel
  static_assert(sizeof(AppModel) <= sizeof(PosteriorModel), "the staging slots fit the application model");
  std::memcpy(h, bytes, n);
  HIPCHECK(hipMemcpyAsync(app_dev_, h, n, hipMemcpyHostToDevice, compute_));
}

void WindowEngine::set_p0(const double* p0, size_t n) {
  if (n != (size_t)kSlots * 16 && n != 2 * (size_t)kSlots * 16) throw std::invalid_argument("p0 must be f64[256] or [512]");
  HIPCHECK(hipMemset(p0_ + kSlots * 16, 0, kSlots * 16 * sizeof(double)));  // [256]: no floor
  HIPCHECK(hipMemcpy(p0_, p0, n * sizeof(double), hipMemcpyHostToDevice));
}

void WindowEngine::set_refit(double alpha, double prior_pseudo, double inv_temp, double min_count, int cap_dom,
                             double ceil) {
  if (!(alpha > 0.0) || !(prior_pseudo >= 0.0) || !(inv_temp > 0.0) || !(min_count >= 0.0) || cap_dom >= cfg_.n_dom ||
      !(ceil > 0.0 && ceil <= 1.0))
    throw std::invalid_argument("refit parameters");
  cfg_.lik_ceil = ceil;
  cfg_.cap_dom = cap_dom < 0 ? -1 : cap_dom;
  cfg_.alpha = alpha;
  cfg_.prior_pseudo = prior_pseudo;
  cfg_.inv_temp = inv_temp;
  cfg_.min_count = min_count;
}

void WindowEngine::refit_now() { refit(nullptr); }

void WindowEngine::score_features(const float* feat, int n, const int32_t* labels, double* post, int32_t* pred,
                                  double* conf, uint32_t* evbits, uint32_t* confusion, const uint32_t* app_cnt) {
  if (n < 0) throw std::invalid_argument("n");
  sync();
  if (n == 0) return;
  // one scratch block: [n][16] f32 features | n | labels | post | pred | conf | evbits | confusion |
  // application counts [n][2]
  const size_t o_n = (size_t)n * 16 * 4, o_lab = o_n + 64, o_post = (o_lab + (size_t)n * 4 + 63) & ~size_t(63);
  const size_t o_pred = o_post + (size_t)n * 16 * 8, o_conf = (o_pred + (size_t)n * 4 + 63) & ~size_t(63);
  const size_t o_ev = o_conf + (size_t)n * 8, o_cm = o_ev + (size_t)n * 16 * 4, o_app = o_cm + 16 * 16 * 4;
  const size_t bytes = o_app + (size_t)n * 2 * 4;
  uint8_t* d = dalloc<uint8_t>(bytes, true);
  HIPCHECK(hipMemcpy(d, feat, o_n, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(d + o_n, &n, sizeof(int), hipMemcpyHostToDevice));
  if (labels) HIPCHECK(hipMemcpy(d + o_lab, labels, (size_t)n * 4, hipMemcpyHostToDevice));
  if (app_cnt) HIPCHECK(hipMemcpy(d + o_app, app_cnt, (size_t)n * 2 * 4, hipMemcpyHostToDevice));
  launch_posterior(reinterpret_cast<const float*>(d), reinterpret_cast<const int*>(d + o_n), n,
                   reinterpret_cast<const PosteriorModel*>(model_dev_),
                   labels ? reinterpret_cast<const int32_t*>(d + o_lab) : nullptr, reinterpret_cast<double*>(d + o_post),
                   reinterpret_cast<int32_t*>(d + o_pred), reinterpret_cast<double*>(d + o_conf),
                   reinterpret_cast<uint32_t*>(d + o_ev), reinterpret_cast<uint32_t*>(d + o_cm), compute_,
                   app_cnt ? app_dev_ : nullptr, app_cnt ? reinterpret_cast<const uint32_t*>(d + o_app) : nullptr);
  HIPCHECK(hipStreamSynchronize(compute_));
  HIPCHECK(hipMemcpy(post, d + o_post, (size_t)n * 16 * 8, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(pred, d + o_pred, (size_t)n * 4, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(conf, d + o_conf, (size_t)n * 8, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(evbits, d + o_ev, (size_t)n * 16 * 4, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(confusion, d + o_cm, 16 * 16 * 4, hipMemcpyDeviceToHost));
  own_.free_dev(d);
}

void WindowEngine::set_pods(const uint32_t* pods, const uint32_t* svcnode, size_t n) {
  // the host mirror is only written between the previous upload's completion (compute stream
  // order: the upload precedes later windows) and this call; uploads are rare (pod churn). The
  // table is read by the definitions and the decode: the front stage's stream with overlapped
  // windows, so the upload takes effect at the next submitted window there as well.
  hipStream_t st = overlap_ ? front_ : compute_;
  HIPCHECK(hipStreamSynchronize(st));
  for (size_t i = 0; i < n; ++i)
    if (pods[i] < kPodRows) pod_host_[pods[i]] = svcnode[i];
  HIPCHECK(hipMemcpyAsync(pod_sn_, pod_host_, kPodRows * 4, hipMemcpyHostToDevice, st));
}

std::vector<uint8_t> WindowEngine::sent_block() {
  sync();
  std::vector<uint8_t> out(xsend_ ? xstride_ : 0);
  if (xsend_) HIPCHECK(hipMemcpy(out.data(), xsend_, xstride_, hipMemcpyDeviceToHost));
  return out;
}

std::vector<int64_t> WindowEngine::import_state() {
  sync();
  int rows[2];
  unsigned long long tmax = 0;
  GenMeta g{};
  std::vector<uint32_t> r(nb_);
  const BufSet& s = *bufs_[submitted_ ? (submitted_ - 1) % nb_ : 0].set;  // the latest window's set
  HIPCHECK(hipMemcpy(rows, s.rows, sizeof(rows), hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(&tmax, tmax_, 8, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(&g, s.gen, sizeof(g), hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(r.data(), remote_n_, 4 * nb_, hipMemcpyDeviceToHost));
  // rows[0..1], tmax, generations, current slot, windows held, per age: cut-off and rows, per
  // buffer: other GPUs' rows
  std::vector<int64_t> out{rows[0], rows[1], (int64_t)tmax, gens_, g.cur, g.filled};
  for (int a = 0; a < kMaxGens; ++a) out.push_back(g.cut[a]);
  for (int a = 0; a < kMaxGens; ++a) out.push_back(a < gens_ ? g.n_rows[(g.cur + slots_ - a) % slots_] : 0);
  for (int b = 0; b < nb_; ++b) out.push_back(r[b]);
  return out;
}

void WindowEngine::inject_remote(const void* blocks, size_t stride, int world, int me) {
  if (!cfg_.import_cap || !cfg_.xchg_cap) throw std::logic_error("inject_remote needs import_cap and xchg_cap > 0");
  if (world < 1 || me < 0 || me >= world || stride < sizeof(XRec)) throw std::invalid_argument("bad exchange blocks");
  const uint8_t* h = static_cast<const uint8_t*>(blocks);
  for (int r = 0; r < world; ++r) {  // the merge kernel trusts each block's header: check it here
    uint32_t c;
    std::memcpy(&c, h + (size_t)r * stride, 4);
    if ((size_t)c * sizeof(XRec) + sizeof(XRec) > stride) throw std::invalid_argument("block row count exceeds stride");
    if (r != me && c > (uint32_t)cfg_.xchg_cap) throw std::invalid_argument("block holds more rows than xchg_cap");
  }
  if (stride * world > xrecv_bytes_) {
    sync();
    own_.free_dev(xrecv_);  // outgrown
    xrecv_ = dalloc<uint8_t>(stride * world);
    xrecv_bytes_ = stride * world;
  }
  inject_.assign(h, h + stride * world);  // consumed by the next submit, between its two halves
  inject_stride_ = stride;
  inject_world_ = world;
  inject_me_ = me;
}

void WindowEngine::init_comm(const ncclUniqueId& id, int rank, int world) {
  if (comm_) throw std::logic_error("communicator already initialised");
  // world 1 is a real communicator too: every collective of the window chain runs (on one rank),
  // which is how a one-GPU box exercises the multi-GPU path (tests/test_rccl_single.py)
  if (world < 1 || rank < 0 || rank >= world) throw std::invalid_argument("communicator rank / world");
  if (submitted_ || copy_open_) throw std::logic_error("init_comm before the first window");
  HIPCHECK(hipSetDevice(cfg_.device));
  if (overlap_) {  // the windows of an engine with a communicator run the serial chain on compute_
    HIPCHECK(hipStreamSynchronize(front_));  // a pod table upload queued there
    overlap_ = false;
    copy_ahead_ = lane_on_request_ = false;
    lanes_ = 1;  // no window has been submitted: lane 1 stays idle
    // the serial chain's default again: the span side on its own stream
    if (!getenv("MISLO_SPAN_STREAM")) enable_span_branch();
  }
  NCCLCHECK(ncclCommInitRank(&comm_, world, id, rank));
  {
    // the comm stream at its own priority: streams of one priority share that priority's
    // hardware queues (GPU_MAX_HW_QUEUES, 4 by default), and a comm stream landing on the copy
    // stream's queue held window k+1's DMAs behind window k's collectives -- which wait for window
    // k's compute -- so no two windows overlapped (measured with a one-rank communicator,
    // tools/rccl_overlap.py: copy-engine idle 0.65-0.75 ms per window, 1.27-1.35 ms per window
    // against 0.77 ms without a communicator). MISLO_COMM_STREAM_PRIO=0: the default priority.
    comm_stream_ = mk_stream(env_int("MISLO_COMM_STREAM_PRIO", 1) != 0);
  }
  rank_ = rank;
  world_ = world;
  for (Buf& buf : bufs_) {
    buf.res_all_dev = dalloc<uint8_t>(result_bytes() * world);
    buf.res_all_host = static_cast<uint8_t*>(host_block(result_bytes() * world));
  }
  if (cfg_.xchg_cap) {
    if (world > 8) throw std::invalid_argument("the exchange is sized for <= 8 GPUs per node");
    own_.free_dev(xrecv_);  // one sized by inject_remote
    xrecv_bytes_ = xstride_ * world;
    xrecv_ = dalloc<uint8_t>(xrecv_bytes_, true);
    // The exchange runs on the comm stream with the window's other collectives: one communicator,
    // one stream, one issue order on every rank. MISLO_XCHG_STREAM=compute puts it on the compute
    // stream over a communicator of its own (ncclCommSplit: 0.60 against 0.62 ms per window in the
    // one-rank rehearsal, profiles/r5_multigpu/); two communicators then run collectives on two
    // streams at once, which no run with world >= 2 has exercised yet, so it is opt-in. Rank 0's
    // choice is broadcast first: ncclCommSplit is collective, and ranks with another env must
    // neither hang in it nor skip it.
    const char* xv = getenv("MISLO_XCHG_STREAM");
    int split = (xv && std::strcmp(xv, "compute") == 0) ? 1 : 0;
    int* d_split = dalloc<int>(1);
    HIPCHECK(hipMemcpy(d_split, &split, sizeof(int), hipMemcpyHostToDevice));
    NCCLCHECK(ncclBroadcast(d_split, d_split, 1, ncclInt32, 0, comm_, comm_stream_));
    HIPCHECK(hipStreamSynchronize(comm_stream_));
    HIPCHECK(hipMemcpy(&split, d_split, sizeof(int), hipMemcpyDeviceToHost));
    own_.free_dev(d_split);
    if (split) NCCLCHECK(ncclCommSplit(comm_, 0, rank, &xcomm_, nullptr));
  }
}

void WindowEngine::totals(double* out) {
  sync();
  HIPCHECK(hipMemcpy(out, totals_, kPacketLen * sizeof(double), hipMemcpyDeviceToHost));
}

void WindowEngine::reset_totals() {
  sync();
  HIPCHECK(hipMemset(totals_, 0, kPacketLen * sizeof(double)));
}

void WindowEngine::stats_acc(double* out) {
  sync();
  HIPCHECK(hipMemcpy(out, stats_acc_, kStatsLen * sizeof(double), hipMemcpyDeviceToHost));
}

void WindowEngine::restore(const double* stats, const void* model, size_t n, int64_t folded) {
  if (n && n != sizeof(PosteriorModel)) throw std::invalid_argument("model image must be POSTERIOR_MODEL_BYTES bytes");
  sync();
  HIPCHECK(hipMemcpy(stats_acc_, stats, kStatsLen * sizeof(double), hipMemcpyHostToDevice));
  if (n) {
    HIPCHECK(hipMemcpy(model_dev_, model, n, hipMemcpyHostToDevice));
  } else {  // the learned model from the restored statistics, by the device refit itself
    refit(nullptr);
    HIPCHECK(hipStreamSynchronize(compute_));
  }
  folded_ = folded;
}

void WindowEngine::model_bytes(void* out) {
  sync();
  HIPCHECK(hipMemcpy(out, model_dev_, sizeof(PosteriorModel), hipMemcpyDeviceToHost));
}

void WindowEngine::sync() {
  HIPCHECK(hipStreamSynchronize(copy_[0]));
  if (copy_[1] != copy_[0]) HIPCHECK(hipStreamSynchronize(copy_[1]));
  if (front_) HIPCHECK(hipStreamSynchronize(front_));  // the front stages (and a pod table upload)
  HIPCHECK(hipStreamSynchronize(compute_));
  HIPCHECK(hipStreamSynchronize(comm_stream_));
}

}  // namespace mislo
