// Native per-GPU window engine: the agent's executor, with no Python or PyTorch on the
// per-window path. One process drives one MI355X; window k uses buffer b = k % nb (nb = 3):
//
//   host           : cut the window (ring positions) and hand the engine the byte ranges; the
//                    host never reads or rewrites a record
//   copy stream    : DMA of the window's ring bytes straight from the (registered) rings into
//                    device block b: the BPF ring's framed records as the kernel wrote them,
//                    the user-space producers' 64-byte records, the spans. With overlapped
//                    windows there can be two of them (copy lanes, below at copy_): window k's
//                    DMAs then go to lane k & 1
//   compute stream : [device refit from window k - nb's all-reduced statistics]
//                    graph(b): reset accumulators -> ring definitions (context rows, trace
//                    map) -> K1 decode (framed + user records) -> partition -> spans -> K2 LDS
//                    join -> finalize -> K3 MFMA posterior (+ confusion, + MFMA sufficient
//                    statistics when learning) -> pack(packet b) -> D2H of the per-incident
//                    results into pinned results b
//   comm stream    : one RCCL group over xGMI when the node has several GPUs: all-reduce(packet
//                    b), all-gather of the window's incident results (node-wide incident list),
//                    all-gather of the trace-tagged rows (merged into window k+1's imports) ->
//                    totals += packet b -> D2H(packet b, all ranks' results)
//
// Halo and imported rows: window k also joins (never counts) the rows of up to halo_windows
// earlier windows that lie within halo_ms of each later window's latest record -- kept resident
// where their own window decoded and partitioned them -- and the other GPUs' trace-tagged rows of
// window k (exchange.hip), so joins across window and GPU boundaries match.
//
// The streams run side by side, so the DMA of window k+1 and the node-wide all-reduce of window k
// run under the kernels of window k+1. The whole compute chain of a buffer is captured once into
// a HIP graph and replayed (one launch per window). Host waits use blocking-sync events (no
// spin: the agent's CPU budget, REF pkg/safety/overhead_guard.go:77-107, counts this process).
//
// One GPU without the exchange: the graph is split at the probe into a front stage on a front
// stream and a back stage on the compute stream, and window k+1's front runs beside window k's
// back (window overlap, below at front_).
//
// Everything indexed by b is one record (Buf), built by alloc() / init_comm() and never
// re-pointed; every run_* is handed the buffer it works on.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <map>
#include <tuple>
#include <type_traits>
#include <vector>

#include "copylanes.h"
#include "mislo_launch.h"
#include "mislo_packet.h"

namespace mislo {

constexpr uint32_t kCtxRows = 1u << 24;                 // device context table rows (256 MiB)
constexpr uint32_t kPodRows = 1u << 20;                 // device pod table: pod id -> svc<<16|node
constexpr uint32_t kTraceIdRows = 1u << 24;             // device trace id -> hash table (128 MiB)
constexpr int kHeadBytes = 64;                          // counts int32[16] (labels follow)

// A host byte range to DMA (a ring segment): registered memory goes straight to the device,
// anything else through the engine's pinned staging.
struct Seg {
  const void* ptr;
  size_t bytes;
};

struct EngineConfig {
  int device = 0;
  int sig_cap = 1 << 20, span_cap = 16384, group_cap = 64;
  int user_cap = 1 << 18;  // user-space (64-byte) records per window; sig_cap bounds framed + user
  int n_buffers = 3, max_ahead = 3;
  double window_ms = 2000.0, threshold = 0.7;
  int fanout = 3, group_mode = 1;
  bool use_graphs = true;
  bool device_refit = true;  // learned naive Bayes refit on the device from accumulated statistics
  double alpha = 2.0, prior_pseudo = 1.0;
  double inv_temp = 1.0, min_count = 0.0;  // refit calibration (posterior.hip k_refit_nb)
  int cap_dom = -1;                         // refit: the domain whose prior is capped (-1: none)
  double lik_ceil = 1.0;                    // refit: every likelihood capped here (models/train.py lik_ceil)
  int n_dom = 10;
  float ttft_slo_ms = 800.0f;  // per-incident SLO impact: spans with TTFT above this breach
  double halo_ms = 0.0;        // later windows also join rows this close to every later window's latest record
  int halo_windows = 3;        // earlier windows whose rows stay resident for the halo (1..3)
  int import_cap = 0;          // other GPUs' trace rows per window; 0 = none
  int xchg_cap = 0;            // trace-tagged rows each GPU exchanges per window (RCCL); 0 = none
  // group sharding of one node's stream over the node's GPUs (agent --gpus N): this GPU counts and
  // joins only its services' records and incident groups (decode.hip shard_owns); 1 = whole stream
  int shard_rank = 0, shard_world = 1;
  // split rings (agent --gpus N with per-worker rings): the producers already routed every record
  // to the ring of the worker owning its service, so the records are not filtered again here (a
  // record routed before its pod's service was known is counted where it landed, never twice);
  // spans keep the ownership filter (it also maps global groups to this GPU's local ones)
  bool split_rings = false;
};

// per-incident results of a window, in one block (one D2H): views into a block of `Byte`s (the
// device block the kernels write, or a const pinned host block)
template <class Byte>
struct ResultViewT {
  template <class T>
  using P = std::conditional_t<std::is_const_v<Byte>, const T, T>*;
  P<double> post;     // [G][16]
  P<double> gconf;    // [G]
  P<float> feat;      // [G][16]
  P<int32_t> pred;    // [G]
  P<uint32_t> evbits; // [G][16]
  P<uint32_t> sli;    // [G][2]: spans, TTFT-SLO breaches
  P<uint32_t> app;    // [G][2]: spans with an application retrieval time, its sum (10 us units)
  P<uint32_t> late;   // [G][2]: breaches of earlier windows reported in this one (SpanMap::grp_late), spare
};
using ResultView = ResultViewT<const uint8_t>;

// The block's byte layout for G incident groups, columns in ResultViewT's order (sli, app and
// late are adjacent: one fill resets the three)
struct ResultLayout {
  size_t G;
  size_t gconf() const { return 16 * G * 8; }
  size_t feat() const { return gconf() + G * 8; }
  size_t pred() const { return feat() + 16 * G * 4; }
  size_t evbits() const { return pred() + G * 4; }
  size_t sli() const { return evbits() + 16 * G * 4; }
  size_t bytes() const { return sli() + 6 * G * 4; }
  template <class Byte>
  ResultViewT<Byte> view(Byte* r) const {
    ResultViewT<Byte> v;
    auto set = [r](auto& p, size_t off) { p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(r + off); };
    set(v.post, 0), set(v.gconf, gconf()), set(v.feat, feat()), set(v.pred, pred()), set(v.evbits, evbits());
    set(v.sli, sli()), set(v.app, sli() + 2 * G * 4), set(v.late, sli() + 4 * G * 4);
    return v;
  }
};

// The window's inputs: ring byte ranges (as the rings hold them) and the window metadata.
struct WindowInput {
  std::vector<Seg> kernel;  // framed BPF ring batch records (136-byte stride), in ring order
  std::vector<Seg> user;    // user-space producers' records: 64-byte EVENT or 32-byte User32
  int user_rec = 64;        // their size
  std::vector<Seg> spans;   // 64-byte SPAN records
  int n_groups = 0;
  const int32_t* labels = nullptr;  // [n_groups] ground-truth domain (replay / evaluation) or null
  int64_t bases[4] = {0, 0, 0, 0};  // epoch bases by tag
};

class WindowEngine {
 public:
  explicit WindowEngine(const EngineConfig& cfg);
  ~WindowEngine();
  WindowEngine(const WindowEngine&) = delete;
  WindowEngine& operator=(const WindowEngine&) = delete;

  const EngineConfig& config() const { return cfg_; }
  int buffers() const { return nb_; }

  // Page-lock a host range (a ring's mapping) so its bytes DMA straight to the device; false if
  // the driver refuses (those ranges then go through pinned staging).
  bool register_host(const void* ptr, size_t bytes);
  // Queue window k (in order). Returns when its DMAs and kernels are queued; the ring bytes
  // must stay untouched until h2d_done(k). The two phases below, back to back.
  void submit(int64_t k, const WindowInput& in, bool with_labels, bool learn);
  // The two phases of submit, for a caller that reads the oldest window's results between them.
  // Copy phase: the checks, the buffer's pinned head and staging, the window's DMAs on its copy
  // lane. With copy_ahead() it does not wait for compute_done(k - max_ahead): the DMAs write only
  // the data regions of the device block, which the front stage of window k - nb read last, so it
  // waits for that window's front_done (and, as ever, its h2d_done and head_done) and the DMAs go
  // out while windows k - nb .. k - 1 may still be computing. Window k - nb's packet and results
  // stay readable until submit_chain(k).
  void submit_copy(int64_t k, const WindowInput& in);
  // Chain phase: the back-pressure on compute_done(k - max_ahead), the stream waits, the head
  // load, the refit, the window's graphs and tail. It overwrites window k - nb's packet and
  // results. n_groups as given to the copy phase.
  void submit_chain(int64_t k, int n_groups, bool with_labels, bool learn);
  // The copy phase may run ahead of the oldest window's results: overlapped windows only (not the
  // serial chain, an engine sized for the exchange, after init_comm, MISLO_ONE_STREAM);
  // MISLO_COPY_AHEAD=0|1 overrides the default where it is available.
  bool copy_ahead() const { return copy_ahead_; }
  // the input DMAs of every window up to k completed (their ring space may be freed): never true
  // for a window while an earlier one is still being read, whichever lane finishes first. A window
  // counts from its copy phase on.
  bool h2d_done(int64_t k);
  void wait_h2d(int64_t k);
  int copy_lanes() const { return lanes_; }
  // A caller that will run the copy phase ahead (submit_copy, then the oldest window's results,
  // then submit_chain) asks for the second lane where the engine left it to that: three buffers
  // with copy_ahead() and no MISLO_COPY_LANES. Opens and warms the lane (a few ms, once: call it
  // before the windows that matter); from the next window on window k copies on lane k & 1.
  // Returns whether two lanes are in use; does nothing anywhere else.
  bool take_copy_lanes();
  bool query(int64_t k);      // window k's results are in host memory
  void wait(int64_t k);
  const double* packet(int64_t k) const { return bufs_[k % nb_].packet_host; }
  ResultView results(int64_t k) const { return layout().view<const uint8_t>(bufs_[k % nb_].res_host); }
  ResultLayout layout() const { return ResultLayout{(size_t)cfg_.group_cap}; }
  // device time of window k (ms): DMA start -> results in host memory, and the compute stream's share.
  // Like copy_ms, for any window whose buffer's chain has not been queued again (k > newest - nb):
  // the copy-side marks are kept 2 nb deep, so window k + nb's copy phase does not disturb them.
  std::pair<float, float> window_ms(int64_t k);
  // window k's DMA span (first DMA's start to the last one's end: with two lanes it shares the
  // link with its neighbours' DMAs) and the time from window k - 1's last DMA to window k's first
  // (negative when they overlap)
  std::vector<float> copy_ms(int64_t k);

  void set_model_bytes(const void* bytes, size_t n);  // stream-ordered before the next window
  // device refit parameters (smoothing, prior pseudo-count, 1 / temperature, minimum labelled mass
  // of an active domain), and a refit of the model from the accumulated statistics now
  // (stream-ordered before the next window)
  void set_refit(double alpha, double prior_pseudo, double inv_temp, double min_count, int cap_dom = -1,
                 double ceil = 1.0);
  void refit_now();
  // stop (or resume) the per-window prequential refit: the model on the device stays frozen
  void set_device_refit(bool on) { cfg_.device_refit = on; }
  // Score n incidents' features [n][16] with the model on the device (the K3 posterior kernel;
  // synchronous, drains the engine first): post [n][16], pred [n], conf [n], evbits [n][16], and
  // the confusion of labels (label_code, may be null) x predictions [16][16].
  // app_cnt (optional, [n][2]): the incidents' application retrieval counts for the application
  // evidence (set_app_model)
  void score_features(const float* feat, int n, const int32_t* labels, double* post, int32_t* pred, double* conf,
                      uint32_t* evbits, uint32_t* confusion, const uint32_t* app_cnt = nullptr);
  // the application evidence model (mislo_launch.h AppModel), stream-ordered before the next window
  void set_app_model(const void* bytes, size_t n);
  // device refit: [16 x 16] Beta-prior table, optionally followed by a [16 x 16] likelihood floor
  void set_p0(const double* p0, size_t n);
  void set_pods(const uint32_t* pods, const uint32_t* svcnode, size_t n);  // pod metadata (stream-ordered)
  // other GPUs' rows for the next window, as their exchange blocks would arrive over RCCL (world
  // blocks of [24-byte header: uint32 row count | XRec rows], this rank's block skipped); the
  // next submit runs the exchange path (decode part 1, merge, part 2) with them
  void inject_remote(const void* blocks, size_t stride, int world, int me);
  void set_join_params(double window_ms, double threshold, int fanout, int group_mode);
  void init_comm(const ncclUniqueId& id, int rank, int world);
  bool has_comm() const { return comm_ != nullptr; }
  int rank() const { return rank_; }
  int world() const { return world_; }
  // all ranks' per-incident results of window k ([world] blocks of result_bytes(); this rank's
  // alone without a communicator)
  const uint8_t* results_all(int64_t k) const { return comm_ ? bufs_[k % nb_].res_all_host : bufs_[k % nb_].res_host; }
  size_t result_bytes() const { return layout().bytes(); }

  void totals(double* out);           // accumulated (all-reduced) packets (synchronous)
  void reset_totals();
  void stats_acc(double* out);        // the device refit's accumulated statistics (synchronous)
  // restore a checkpoint: accumulated statistics, the model image (model_bytes = 0: refit it
  // on the device from the statistics) and the folded-window count
  void restore(const double* stats, const void* model, size_t model_bytes, int64_t folded);
  void model_bytes(void* out);        // the model currently on the device (synchronous)
  void sync();
  // device-side import state (synchronous; diagnostics and tests): rows[0..1], tmax, the
  // generations (count, current slot, windows held, per-age cut-offs and rows), per buffer the
  // other-GPU row counts
  std::vector<int64_t> import_state();
  // this GPU's exchange block of the last window (header: row count | XRec rows; empty without
  // the exchange): what the all-gather delivers to the other GPUs (tests)
  std::vector<uint8_t> sent_block();
  int64_t windows_folded() const { return folded_; }
  size_t staged_bytes() const { return staged_bytes_; }
  size_t direct_bytes() const { return direct_bytes_; }
  size_t graphs() const { return graphs_.size(); }
  double host_issue_us() const { return issue_n_ ? issue_us_ / issue_n_ : 0.0; }
  // of which: blocked on back-pressure events, and issuing the window's DMAs
  double host_wait_us() const { return issue_n_ ? wait_us_ / issue_n_ : 0.0; }
  double host_dma_issue_us() const { return issue_n_ ? dma_us_ / issue_n_ : 0.0; }
  double host_launch_us() const { return issue_n_ ? launch_us_ / issue_n_ : 0.0; }  // the chain's launch
  double host_pre_us() const { return issue_n_ ? pre_us_ / issue_n_ : 0.0; }     // stream waits + refit
  double host_tail_us() const { return issue_n_ ? tail_us_ / issue_n_ : 0.0; }   // results D2H + comm stream

 private:
  // the record ownership filter's (rank, world): none with split rings (EngineConfig::split_rings)
  int rec_shard_rank() const { return cfg_.split_rings ? 0 : cfg_.shard_rank; }
  int rec_shard_world() const { return cfg_.split_rings ? 1 : cfg_.shard_world; }
  struct Buf;
  // The parts a window's chain is launched (and captured) in. One GPU: the whole window, or with
  // overlapped windows its front and back stage. With the exchange: the records (part 1), the
  // exchange, the join (part 2), and with xspan_ the window head and the span side on their own.
  enum class Stage : int { Window, Records, Join, XchgSpans, XchgHead, Front, Back };
  static constexpr int kStageSlots = 8;  // graph key and warm_ index: b * kStageSlots + stage
  void alloc();
  void enable_span_branch();  // side_, its events, branch_ (alloc; init_comm leaving the overlap)
  void run_begin(const Buf& buf, hipStream_t st);
  void run_part1(const Buf& buf, hipStream_t st, bool xchg);
  // part 2's two halves: up to the signal scatter and the probe's work list (the end of a
  // window's front stage), and from the probe to the packet (its back stage)
  void run_join_front(const Buf& buf, hipStream_t st, bool xchg);
  void run_join_back(const Buf& buf, int n_groups, bool with_labels, bool learn, hipStream_t st);
  // the window's span side (decode, partition, probe work list, span sort) on side_, forked
  // from `st` after the accumulators are reset and joined before the probe (one-GPU chain)
  void run_span_branch(const Buf& buf, hipStream_t st);
  void run_spans(const Buf& buf, hipStream_t st);
  void launch_part(Stage part, const Buf& buf, int n_groups, bool with_labels, bool learn);
  // the other GPUs' rows of this window (exchange blocks) into the buffer's imports, then its rows
  void merge_remote(const Buf& buf, const uint8_t* blocks, size_t stride, int world, int me, hipStream_t st);
  void refit(const double* add);  // fold `add` (or nothing) into the statistics and refit the model
  SignalCols sig_cols(const Buf& buf) const;
  SpanCols span_cols(const Buf& buf) const;
  bool registered(const void* p, size_t n) const;
  size_t dma(const std::vector<Seg>& segs, uint8_t* dst, size_t cap, uint8_t*& staging, size_t& st_off,
             hipStream_t st);
  // What the engine created; destroyed after the graphs and the communicators, in this order
  struct Owner {
    std::vector<hipEvent_t> events;
    std::vector<void*> dev, host;
    std::vector<hipStream_t> streams;
    void free_dev(void* p);  // a block released early: scratch, an outgrown xrecv_
    ~Owner();
  } own_;
  template <class T>
  T* dalloc(size_t n, bool zero = false);
  void* host_alloc(size_t bytes, unsigned flags);
  void* host_block(size_t bytes);  // zeroed, device-visible: the kernels store into it
  hipEvent_t mk_event(unsigned flags);
  hipStream_t mk_stream(bool high_priority = false);

  EngineConfig cfg_;
  int nb_, max_ahead_;
  size_t off_kern_ = 0, off_user_ = 0, off_span_ = 0, in_bytes_ = 0;  // device input block layout
  // the BPF ring bytes a window of sig_cap rows can hold: whole batch records
  size_t kern_bytes() const { return (size_t)kRecStride * (((size_t)cfg_.sig_cap + kBatchSlots - 1) / kBatchSlots); }
  std::vector<std::pair<const uint8_t*, size_t>> registered_;
  size_t staged_bytes_ = 0, direct_bytes_ = 0;
  uint32_t *pod_sn_ = nullptr, *pod_host_ = nullptr;
  unsigned long long* trace_hash_ = nullptr;  // kernel trace id -> hash
  AppModel* app_dev_ = nullptr;     // the application evidence model (device)
  int n_rows_ = 0;                 // rows per generation = sig_cap + import_cap
  int gens_ = 1;                   // resident generations (1 + halo_windows with a halo)
  int slots_ = 1;                  // physical generation slots: gens_, + 1 with overlapped windows
  unsigned long long* tmax_ = nullptr;
  KeyTs* g_keys_ = nullptr;        // [gens][kKeyTypes * n_rows] partition list keys
  uint32_t *remote_n_ = nullptr, *sel_cnt_ = nullptr, *sel_off_ = nullptr;  // remote_n_: [nb], Buf::remote_n
  unsigned long long* sel_mask_ = nullptr;  // the fused selection's ballot masks (nullptr: two passes)
  int sel_stride_ = 0;
  uint8_t *xsend_ = nullptr, *xrecv_ = nullptr;
  size_t xstride_ = 0, xrecv_bytes_ = 0;
  int nblk_imp_ = 0;                    // decode blocks of the other GPUs' rows
  bool spin_ = false;
  std::vector<uint8_t> inject_;         // exchange blocks for the next window (inject_remote)
  size_t inject_stride_ = 0;
  int inject_world_ = 0, inject_me_ = 0;
  int rank_ = 0, world_ = 1;
  // span branch: a second compute stream, overlapping the span side of the chain (~50 us of
  // small kernels, plus the one-workgroup probe work list) with the signal side's decode and
  // scatter, joined before the probe: the one-GPU chain only (with the exchange the window runs
  // as two graphs on the compute stream). On by default in the serial chain, off with
  // MISLO_ONE_STREAM (the one-queue agent), MISLO_SPAN_STREAM=0 (profiles/r5_probe/README.md) and,
  // unless MISLO_SPAN_STREAM=1, with overlapped windows (profiles/window_overlap/README.md).
  hipStream_t side_ = nullptr;
  // Window overlap (one-GPU chain only): a window runs as two stages, each a captured graph of
  // its own -- the front stage (head load, accumulator reset, definitions, decode, span side,
  // signal scatter, probe work list) on front_, the back stage (probe .. k_window_end) on
  // compute_ -- so window k + 1's bandwidth-leaning front runs beside window k's latency-bound
  // back. Front(k) waits for back(k - 2) (compute_done), which bounds the overlap to one window;
  // every array both stages touch is per buffer (BufSet) or per physical generation slot
  // (slots_ = gens_ + 1): docs/ARCHITECTURE.md, "Window overlap". On where the span branch would
  // be (not with MISLO_ONE_STREAM), never with the exchange or a communicator;
  // MISLO_WINDOW_OVERLAP=0/1 overrides. The span branch is then off unless MISLO_SPAN_STREAM=1:
  // copy, front and compute with branch-free graphs keep one hardware queue each (the second
  // copy lane draws its queue from the other priority's pool, at copy_).
  hipStream_t front_ = nullptr;
  bool overlap_ = false;
  // The state both stages of a window touch, one set per buffer with overlapped windows (else
  // one set, shared by every buffer): reached through Buf::set.
  struct BufSet {
    GenMeta* gen;  // generation slots, halo cut-offs, time ranges
    int* rows;     // rows of the window
    uint32_t *ring_state, *hist, *status, *confusion, *cnt, *gcnt;
    unsigned long long *misc, *dbg, *top3, *gsum;
    double *stats, *stats_count;
    SpanRec* s_rec;
    PartCodes* s_part;
    uint32_t *s_items, *s_part_base, *probe_work;
    PreSpan* s_pre;  // the probe's per-window sorted span lists (k_span_sort)
  };
  std::vector<BufSet> sets_;
  // Everything of buffer b (window k uses b = k % nb). Built by alloc(), the res_all blocks by
  // init_comm(); afterwards only `staging` changes, once, on the first unregistered range.
  struct Buf {
    int b;
    uint8_t* in;         // device: [head | framed | user | spans]
    uint8_t* head_host;  // pinned: counts + labels
    uint8_t* staging;    // pinned staging for unregistered ranges (allocated on first use)
    double *packet_dev, *packet_host;
    uint8_t *res_dev, *res_host;          // per-incident results block and its pinned copy
    uint8_t *res_all_dev, *res_all_host;  // every rank's (with a communicator)
    ResultViewT<uint8_t> res;             // views into res_dev
    SigRec* imp;                          // other GPUs' rows, imported after this window's records
    uint32_t* remote_n;                   // their count
    const BufSet* set;
    const GenMeta* gen_prev;  // the previous window's: buffer b - 1's set (or this one's own)
    hipEvent_t head_done, front_done, compute_done, comm_done, xchg_done;
    hipEvent_t t_comp0, t_comp1, t_end;
    const int* counts() const { return reinterpret_cast<const int*>(in); }
  };
  std::vector<Buf> bufs_;
  // The copy side's events of window k, in slot k % (2 nb): the copy phase of window k + nb runs
  // while window k may still be uncollected, and window_ms(k) / copy_ms(k) need k's own records.
  // t_start: before the window's first DMA. h2d_done: its last DMA ended (the host sleeps on it,
  // the front stream waits for it, and it ends the window's timed copy span). A slot is recorded
  // again by window k + 2 nb, long after the copy phase of k + nb synchronised it (CopiedUpTo).
  struct CopyMark {
    hipEvent_t t_start, h2d_done;
  };
  std::vector<CopyMark> marks_;
  const CopyMark& mark(int64_t k) const { return marks_[copy_mark_slot(k, nb_)]; }
  hipEvent_t ev_fork_ = nullptr, ev_sigbase_ = nullptr, ev_spans_ = nullptr;
  bool branch_ = false;
  bool xspan_ = false;  // with the exchange: Stage::XchgHead, and Stage::XchgSpans on side_
  bool exchange() const { return comm_ && cfg_.xchg_cap > 0 && cfg_.import_cap > 0; }
  JoinParams jp_{};
  int nblk_sig_ = 1, nblk_span_ = 1;
  // Copy lanes (copylanes.h): window k's three DMAs go back to back to copy_[k & 1] when there
  // are two, so one lane's DMAs are already queued on its engine while the other hands a finished
  // window over to its end marker and the next window's start marker. Two with overlapped windows
  // and four or more buffers; with three and copy_ahead(), once the caller asked for them
  // (take_copy_lanes(): until then, and for a caller of submit() alone, one lane as before);
  // MISLO_COPY_LANES=1|2 overrides where windows overlap (alloc()). One with MISLO_ONE_STREAM,
  // with the exchange sized in, and from init_comm on. The second lane is created at the highest stream priority, which draws its
  // hardware queue from the other pool than copy, front and compute (MISLO_COPY_LANE_PRIO=0:
  // default priority).
  hipStream_t copy_[kMaxCopyLanes] = {nullptr, nullptr};
  int lanes_ = 1;
  bool copy_ahead_ = false;
  bool lane_on_request_ = false;  // three buffers, copy-ahead, no MISLO_COPY_LANES: take_copy_lanes() adds the lane
  // submit_copy(submitted_) has run and its submit_chain has not: the window's DMAs are queued
  // (h2d_done / wait_h2d answer for it), nothing else of it is
  bool copy_open_ = false;
  int copy_groups_ = 0;  // its n_groups
  int64_t copied_windows() const { return submitted_ + (copy_open_ ? 1 : 0); }
  CopiedUpTo copied_;
  bool copied_ready(int64_t w, bool block);
  hipStream_t compute_ = nullptr, comm_stream_ = nullptr;
  ncclComm_t comm_ = nullptr;
  ncclComm_t xcomm_ = nullptr;  // the trace-row exchange's communicator (compute stream; init_comm)
  // device buffers shared by every window
  uint32_t* ctx_tab_ = nullptr;
  double *totals_ = nullptr, *stats_acc_ = nullptr, *p0_ = nullptr;
  uint8_t* model_dev_ = nullptr;
  std::vector<uint8_t*> model_host_;
  int model_slot_ = 0;
  uint8_t* g_status_ = nullptr;
  PartCodes* g_part_ = nullptr;
  uint32_t *g_part_blk_ = nullptr, *g_part_off_ = nullptr, *g_part_tot_ = nullptr, *g_part_base_ = nullptr,
           *g_items_ = nullptr;
  SigRec* g_rec_ = nullptr;
  uint32_t *s_part_blk_ = nullptr, *s_part_off_ = nullptr, *s_part_tot_ = nullptr;
  float *attrs_ = nullptr, *conf_ = nullptr, *kernel_ms_ = nullptr;
  std::map<std::tuple<int, int, bool, bool>, hipGraphExec_t> graphs_;
  std::vector<bool> warm_;
  std::vector<hipGraph_t> graph_defs_;
  int64_t submitted_ = 0, folded_ = 0;
  double issue_us_ = 0, wait_us_ = 0, dma_us_ = 0, launch_us_ = 0, pre_us_ = 0, tail_us_ = 0;
  double split_us_[4] = {0, 0, 0, 0};  // DMA issue: ring bytes, head, user records, spans

 public:
  std::vector<double> host_dma_split_us() const {
    std::vector<double> v;
    for (double x : split_us_) v.push_back(issue_n_ ? x / issue_n_ : 0.0);
    return v;
  }

 private:
  int64_t issue_n_ = 0;
};

void engine_set_tables(const Tables& t);

}  // namespace mislo
