// pybind11 module `_mislo_agent`: the native window engine (engine.h) for the agent daemon and
// the benchmark. No PyTorch: the agent process links the HIP runtime, RCCL and these kernels
// only (its resident set is part of the overhead budget, REF docs/benchmarks targets <= 250 MB).
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>
#include <memory>
#include <stdexcept>

#include "decodesli.h"
#include "drift.h"
#include "engine.h"
#include "errsli.h"
#include "exemplars.h"
#include "loadsli.h"
#include "satcurve.h"
#include "onset.h"
#include "openreq.h"
#include "podrank.h"
#include "retrsli.h"
#include "slisketch.h"

namespace py = pybind11;
using namespace mislo;

namespace {

template <class T>
py::array_t<T> copy_array(const T* p, std::vector<py::ssize_t> shape) {
  py::array_t<T> a(shape);
  size_t n = 1;
  for (auto s : shape) n *= (size_t)s;
  if (n) std::memcpy(a.mutable_data(), p, n * sizeof(T));
  return a;
}

void set_tables_np(py::array_t<int8_t, py::array::c_style | py::array::forcecast> type_slot,
                   py::array_t<float, py::array::c_style | py::array::forcecast> scale,
                   py::array_t<float, py::array::c_style | py::array::forcecast> warn,
                   py::array_t<float, py::array::c_style | py::array::forcecast> err,
                   py::array_t<float, py::array::c_style | py::array::forcecast> edges) {
  Tables t;
  std::memset(&t, 0, sizeof(t));
  if (type_slot.size() != kMaxTypes || scale.size() != kSlots || warn.size() != kSlots || err.size() != kSlots ||
      edges.size() != kSlots * kBuckets)
    throw std::invalid_argument("table shapes");
  std::memcpy(t.type_slot, type_slot.data(), sizeof(t.type_slot));
  std::memcpy(t.scale, scale.data(), sizeof(t.scale));
  std::memcpy(t.warn, warn.data(), sizeof(t.warn));
  std::memcpy(t.err, err.data(), sizeof(t.err));
  std::memcpy(t.edges, edges.data(), sizeof(t.edges));
  engine_set_tables(t);
}

}  // namespace

class PyEngine {
 public:
  PyEngine(int device, int sig_cap, int span_cap, int group_cap, int user_cap, int n_buffers, int max_ahead,
           double window_ms, double threshold, int fanout, int group_mode, bool use_graphs, bool device_refit,
           int n_dom, float ttft_slo_ms, double halo_ms, int import_cap, int xchg_cap, int shard_rank,
           int shard_world, int halo_windows, bool split_rings) {
    if (shard_world < 1 || shard_rank < 0 || shard_rank >= shard_world) throw std::invalid_argument("shard rank / world");
    EngineConfig c;
    c.device = device;
    c.sig_cap = sig_cap;
    c.span_cap = span_cap;
    c.group_cap = group_cap;
    c.user_cap = user_cap;
    c.n_buffers = n_buffers;
    c.max_ahead = max_ahead;
    c.window_ms = window_ms;
    c.threshold = threshold;
    c.fanout = fanout;
    c.group_mode = group_mode;
    c.use_graphs = use_graphs;
    c.device_refit = device_refit;
    c.n_dom = n_dom;
    c.ttft_slo_ms = ttft_slo_ms;
    c.halo_ms = halo_ms;
    c.halo_windows = halo_windows;
    c.import_cap = import_cap;
    c.xchg_cap = xchg_cap;
    c.shard_rank = shard_rank;
    c.shard_world = shard_world;
    c.split_rings = split_rings;
    e_ = std::make_unique<WindowEngine>(c);
  }
  bool register_host(uintptr_t addr, size_t bytes) {
    return e_->register_host(reinterpret_cast<const void*>(addr), bytes);
  }
  // segments: lists of (host address, bytes) in ring order
  using Ranges = std::vector<std::pair<uintptr_t, size_t>>;
  void submit(int64_t k, const Ranges& kernel, const Ranges& user, const Ranges& spans, int n_groups,
              py::object labels, std::vector<int64_t> bases, bool with_labels, bool learn, int user_rec) {
    std::vector<int32_t> lab;
    const WindowInput in = window_input(kernel, user, spans, n_groups, labels, std::move(bases), user_rec, lab);
    py::gil_scoped_release nogil;
    e_->submit(k, in, with_labels, learn);
  }
  // the two phases of submit (engine.h): the window's DMAs, then its chain
  void submit_copy(int64_t k, const Ranges& kernel, const Ranges& user, const Ranges& spans, int n_groups,
                   py::object labels, std::vector<int64_t> bases, int user_rec) {
    std::vector<int32_t> lab;
    const WindowInput in = window_input(kernel, user, spans, n_groups, labels, std::move(bases), user_rec, lab);
    py::gil_scoped_release nogil;
    e_->submit_copy(k, in);
  }
  void submit_chain(int64_t k, int n_groups, bool with_labels, bool learn) {
    py::gil_scoped_release nogil;
    e_->submit_chain(k, n_groups, with_labels, learn);
  }
  // `lab` holds the labels the returned input points to
  static WindowInput window_input(const Ranges& kernel, const Ranges& user, const Ranges& spans, int n_groups,
                                  py::object labels, std::vector<int64_t> bases, int user_rec,
                                  std::vector<int32_t>& lab) {
    WindowInput in;
    auto conv = [](const std::vector<std::pair<uintptr_t, size_t>>& v, std::vector<Seg>& out) {
      for (auto& p : v) out.push_back(Seg{reinterpret_cast<const void*>(p.first), p.second});
    };
    conv(kernel, in.kernel);
    conv(user, in.user);
    conv(spans, in.spans);
    in.n_groups = n_groups;
    in.user_rec = user_rec;
    if (!labels.is_none()) {
      auto arr = labels.cast<py::array_t<int32_t, py::array::c_style | py::array::forcecast>>();
      lab.assign(arr.data(), arr.data() + arr.size());
      lab.resize(std::max<size_t>(lab.size(), (size_t)std::max(0, n_groups)), -1);
      in.labels = lab.data();
    }
    bases.resize(4, 0);
    for (int q = 0; q < 4; ++q) in.bases[q] = bases[q];
    return in;
  }
  bool h2d_done(int64_t k) { return e_->h2d_done(k); }
  void wait_h2d(int64_t k) {
    py::gil_scoped_release nogil;
    e_->wait_h2d(k);
  }
  bool query(int64_t k) { return e_->query(k); }
  void wait(int64_t k) {
    py::gil_scoped_release nogil;
    e_->wait(k);
  }
  py::array_t<double> packet(int64_t k) { return copy_array(e_->packet(k), {kPacketLen}); }
  py::dict results(int64_t k, int n_groups) {
    if (n_groups < 0 || n_groups > eng().config().group_cap) throw std::invalid_argument("n_groups");
    return result_dict(e_->results(k), n_groups);
  }
  // every rank's results of window k (the node-wide incident list, all-gathered over RCCL)
  py::list results_all(int64_t k, int n_groups) {
    WindowEngine& e = eng();
    if (n_groups < 0 || n_groups > e.config().group_cap) throw std::invalid_argument("n_groups");
    const ResultLayout lay = e.layout();
    const uint8_t* base = e.results_all(k);
    py::list out;
    const int w = e.has_comm() ? e.world() : 1;
    for (int r = 0; r < w; ++r) out.append(result_dict(lay.view(base + (size_t)r * lay.bytes()), n_groups));
    return out;
  }
  static py::dict result_dict(const ResultView& r, int n_groups) {
    const py::ssize_t G = n_groups;
    py::dict d;
    d["post"] = copy_array(r.post, {G, 16});
    d["conf"] = copy_array(r.gconf, {G});
    d["feat"] = copy_array(r.feat, {G, 16});
    d["pred"] = copy_array(r.pred, {G});
    d["evbits"] = copy_array(r.evbits, {G, 16});
    d["sli"] = copy_array(r.sli, {G, 2});
    d["app"] = copy_array(r.app, {G, 2});
    d["late"] = copy_array(r.late, {G, 2});
    return d;
  }
  py::tuple window_ms(int64_t k) {
    std::pair<float, float> t;
    {
      py::gil_scoped_release nogil;
      t = e_->window_ms(k);
    }
    return py::make_tuple(t.first, t.second);
  }
  void set_model_bytes(py::array_t<uint8_t, py::array::c_style | py::array::forcecast> b) {
    e_->set_model_bytes(b.data(), (size_t)b.size());
  }
  void set_app_model(py::array_t<uint8_t, py::array::c_style | py::array::forcecast> b) {
    e_->set_app_model(b.data(), (size_t)b.size());
  }
  void set_refit(double alpha, double prior_pseudo, double inv_temp, double min_count, int cap_dom, double ceil) {
    eng().set_refit(alpha, prior_pseudo, inv_temp, min_count, cap_dom, ceil);
  }
  void refit_now() { eng().refit_now(); }
  // K3 on given features (REF's 55 rows, offline evaluation) with the model on the device
  py::dict score(py::array_t<float, py::array::c_style | py::array::forcecast> feat, py::object labels,
                 py::object app) {
    if (feat.ndim() != 2 || feat.shape(1) != 16) throw std::invalid_argument("feat must be float32 [n, 16]");
    const int n = (int)feat.shape(0);
    std::vector<int32_t> lab;
    if (!labels.is_none()) {
      auto a = labels.cast<py::array_t<int32_t, py::array::c_style | py::array::forcecast>>();
      if (a.size() != n) throw std::invalid_argument("labels must have n entries");
      lab.assign(a.data(), a.data() + n);
    }
    std::vector<uint32_t> appc;
    if (!app.is_none()) {
      auto a = app.cast<py::array_t<uint32_t, py::array::c_style | py::array::forcecast>>();
      if (a.size() != 2 * (py::ssize_t)n) throw std::invalid_argument("app must be uint32 [n, 2]");
      appc.assign(a.data(), a.data() + 2 * (size_t)n);
    }
    std::vector<double> post((size_t)n * 16), conf(n);
    std::vector<int32_t> pred(n);
    std::vector<uint32_t> ev((size_t)n * 16), cm(256);
    {
      py::gil_scoped_release nogil;
      eng().score_features(feat.data(), n, lab.empty() ? nullptr : lab.data(), post.data(), pred.data(), conf.data(),
                           ev.data(), cm.data(), appc.empty() ? nullptr : appc.data());
    }
    py::dict d;
    d["post"] = copy_array(post.data(), {n, 16});
    d["pred"] = copy_array(pred.data(), {n});
    d["conf"] = copy_array(conf.data(), {n});
    d["evbits"] = copy_array(ev.data(), {n, 16});
    d["confusion"] = copy_array(cm.data(), {16, 16});
    return d;
  }
  void set_p0(py::array_t<double, py::array::c_style | py::array::forcecast> p0) {
    if (p0.size() != kSlots * 16 && p0.size() != 2 * kSlots * 16)
      throw std::invalid_argument("p0 must be f64[256] (table) or f64[512] (table, floor)");
    e_->set_p0(p0.data(), (size_t)p0.size());
  }
  void set_pods(py::array_t<uint32_t, py::array::c_style | py::array::forcecast> pods,
                py::array_t<uint32_t, py::array::c_style | py::array::forcecast> sn) {
    if (pods.size() != sn.size()) throw std::invalid_argument("pods / svcnode size mismatch");
    e_->set_pods(pods.data(), sn.data(), (size_t)pods.size());
  }
  void inject_remote(py::buffer blocks, size_t stride, int world, int me) {
    py::buffer_info bi = blocks.request();
    if ((size_t)(bi.size * bi.itemsize) < stride * (size_t)std::max(world, 0)) throw std::invalid_argument("blocks too small");
    py::gil_scoped_release nogil;
    eng().inject_remote(bi.ptr, stride, world, me);
  }
  void set_join_params(double window_ms, double threshold, int fanout, int group_mode) {
    e_->set_join_params(window_ms, threshold, fanout, group_mode);
  }
  void init_comm(py::bytes id, int rank, int world) {
    std::string s = id;
    if (s.size() != sizeof(ncclUniqueId)) throw std::invalid_argument("unique id size");
    ncclUniqueId u;
    std::memcpy(&u, s.data(), sizeof(u));
    py::gil_scoped_release nogil;
    e_->init_comm(u, rank, world);
  }
  py::array_t<double> totals() {
    std::vector<double> t(kPacketLen);
    {
      py::gil_scoped_release nogil;
      e_->totals(t.data());
    }
    return copy_array(t.data(), {kPacketLen});
  }
  void reset_totals() {
    py::gil_scoped_release nogil;
    e_->reset_totals();
  }
  py::array_t<double> stats_acc() {
    std::vector<double> t(kStatsLen);
    {
      py::gil_scoped_release nogil;
      e_->stats_acc(t.data());
    }
    return copy_array(t.data(), {kStatsLen});
  }
  void restore(py::array_t<double, py::array::c_style | py::array::forcecast> stats,
               py::array_t<uint8_t, py::array::c_style | py::array::forcecast> model, int64_t folded) {
    if (stats.size() != kStatsLen) throw std::invalid_argument("stats must be f64[STATS_LEN]");
    eng().restore(stats.data(), model.data(), (size_t)model.size(), folded);
  }
  py::array_t<uint8_t> model_bytes() {
    std::vector<uint8_t> t(sizeof(PosteriorModel));
    {
      py::gil_scoped_release nogil;
      e_->model_bytes(t.data());
    }
    return copy_array(t.data(), {(py::ssize_t)t.size()});
  }
  void sync() {
    py::gil_scoped_release nogil;
    e_->sync();
  }
  std::vector<int64_t> import_state() {
    py::gil_scoped_release nogil;
    return eng().import_state();
  }
  py::bytes sent_block() {
    std::vector<uint8_t> b;
    {
      py::gil_scoped_release nogil;
      b = eng().sent_block();
    }
    return py::bytes(reinterpret_cast<const char*>(b.data()), b.size());
  }
  void close() {
    if (e_) {
      py::gil_scoped_release nogil;
      e_->sync();
      e_.reset();
    }
  }
  WindowEngine& eng() {
    if (!e_) throw std::logic_error("engine closed");
    return *e_;
  }
  int buffers() { return eng().buffers(); }
  int64_t folded() { return eng().windows_folded(); }
  size_t graphs() { return eng().graphs(); }
  double host_issue_us() { return eng().host_issue_us(); }
  double host_wait_us() { return eng().host_wait_us(); }
  double host_dma_issue_us() { return eng().host_dma_issue_us(); }
  double host_launch_us() { return eng().host_launch_us(); }
  bool has_comm() { return eng().has_comm(); }
  size_t staged_bytes() { return eng().staged_bytes(); }
  size_t direct_bytes() { return eng().direct_bytes(); }

 private:
  std::unique_ptr<WindowEngine> e_;
};

// What the bindings of every side tracker share: the tracker itself (gone after close()) and the calls that
// need nothing of the tracker's own. The GIL is released around everything that can wait for the device.
template <class T>
class PyLane {
 public:
  explicit PyLane(const char* name) : name_(name) {}
  T& t() {
    if (!t_) throw std::logic_error(std::string(name_) + " closed");
    return *t_;
  }
  bool query(int64_t i) { return t().query(i); }
  // the whole result block of step i as it left the device (uint32 words)
  py::array_t<uint32_t> block(int64_t i) {
    T& tr = t();
    const uint32_t* r;
    {
      py::gil_scoped_release nogil;
      r = tr.results(i);
    }
    return copy_array(r, {(py::ssize_t)tr.result_layout().words});
  }
  // the tracker's step_ms as a tuple of as many floats
  py::tuple step_ms(int64_t i) {
    decltype(std::declval<T&>().step_ms(i)) ms;
    {
      py::gil_scoped_release nogil;
      ms = t().step_ms(i);
    }
    return py::tuple(py::cast(ms));
  }
  void sync() {
    py::gil_scoped_release nogil;
    t().sync();
  }
  // ---- checkpoint (steplane.h): the same four calls for every tracker ----
  // enqueue a snapshot behind the steps issued so far; returns its ticket
  int64_t snapshot() {
    T& tr = t();
    py::gil_scoped_release nogil;
    return tr.lane().snapshot(tr.host_words());
  }
  bool snapshot_ready(int64_t ticket) { return t().lane().snapshot_ready(ticket); }
  // header and payload as bytes; waits for the transfer
  py::bytes snapshot_image(int64_t ticket) {
    T& tr = t();
    const uint8_t* p;
    {
      py::gil_scoped_release nogil;
      p = tr.lane().snapshot_image(ticket);
    }
    return py::bytes(reinterpret_cast<const char*>(p), tr.lane().image_bytes());
  }
  float snapshot_kernel_ms() { return t().lane().snapshot_kernel_ms(); }
  size_t image_bytes() { return t().lane().image_bytes(); }
  // Take an image, before the first step only; ValueError names what does not fit, with nothing changed.
  // Returns the index the next step gets.
  int64_t restore(py::buffer image) {
    T& tr = t();
    const py::buffer_info bi = image.request();
    if (bi.ndim != 1 || bi.strides[0] != bi.itemsize) throw std::invalid_argument("restore: a contiguous one-dimensional buffer");
    const size_t bytes = (size_t)bi.size * (size_t)bi.itemsize;
    py::gil_scoped_release nogil;
    return tr.lane().restore(bi.ptr, bytes, [&tr](const lane::ImageHeader& h) { tr.set_host_words(h.host, (int)h.n_host); }).step;
  }
  // blocks of the checkpoint kernels, at most (tests: 1 forces the grid-stride path)
  void set_checkpoint_blocks(int max_blocks) { t().lane().set_checkpoint_blocks(max_blocks); }
  void close() {
    if (t_) {
      py::gil_scoped_release nogil;
      t_.reset();
    }
  }
  // the checkpoint calls of a tracker's class, once for all eleven
  template <class PyT>
  static void def_checkpoint(py::class_<PyT>& c) {
    c.def("snapshot", &PyT::snapshot)
        .def("snapshot_ready", &PyT::snapshot_ready)
        .def("snapshot_image", &PyT::snapshot_image)
        .def("snapshot_kernel_ms", &PyT::snapshot_kernel_ms)
        .def("image_bytes", &PyT::image_bytes)
        .def("restore", &PyT::restore)
        .def("set_checkpoint_blocks", &PyT::set_checkpoint_blocks);
  }

 protected:
  std::unique_ptr<T> t_;

 private:
  const char* name_;
};

// The open-request tracker (openreq.h): one step per window over the same span ranges the engine
// gets; results per step index.
class PyOpenRequests : public PyLane<OpenRequests> {
 public:
  PyOpenRequests(int device, int64_t cap, int span_cap, int group_cap, int n_buffers, double slo_ms, double ttl_ms,
                 double reorder_ms)
      : PyLane("open-request tracker") {
    openreq::Config c;
    c.device = device;
    c.cap = cap;
    c.span_cap = span_cap;
    c.group_cap = group_cap;
    c.n_buffers = n_buffers;
    c.slo_ms = slo_ms;
    c.ttl_ms = ttl_ms;
    c.reorder_ms = reorder_ms;
    openreq::validate(c);
    t_ = std::make_unique<OpenRequests>(c);
  }
  int64_t step(const std::vector<std::pair<uintptr_t, size_t>>& spans, int64_t cut_ns, int64_t prev_cut_ns,
               int n_groups) {
    OpenRequests& tr = t();
    py::gil_scoped_release nogil;
    return tr.step(spans, cut_ns, prev_cut_ns, n_groups);
  }
  py::dict results(int64_t i, int n_groups) {
    OpenRequests& tr = t();
    if (n_groups < 0 || n_groups > tr.config().group_cap) throw std::invalid_argument("n_groups");
    const uint32_t* r;
    {
      py::gil_scoped_release nogil;
      r = tr.results(i);
    }
    const openreq::Layout& l = tr.result_layout();
    py::dict d;
    d["dl"] = copy_array(r + l.dl, {n_groups, 2});
    d["dup"] = copy_array(r + l.dup, {n_groups, 3});
    d["stats"] = copy_array(r + l.stats, {openreq::kStats});
    return d;
  }
  py::tuple entries() {
    std::vector<uint64_t> k;
    std::vector<int64_t> tt;
    std::vector<uint32_t> g, s;
    {
      py::gil_scoped_release nogil;
      t().entries(k, tt, g, s);
    }
    const py::ssize_t n = (py::ssize_t)k.size();
    return py::make_tuple(copy_array(k.data(), {n}), copy_array(tt.data(), {n}), copy_array(g.data(), {n}),
                          copy_array(s.data(), {n}));
  }
};

// The TTFT sketch (slisketch.h): one step per window over the same span ranges the engine gets;
// results per step index.
class PySliSketch : public PyLane<SliSketch> {
 public:
  PySliSketch(int device, int span_cap, int group_cap, int windows, int n_buffers)
      : PyLane("ttft sketch") {
    slisketch::Config c;
    c.device = device;
    c.span_cap = span_cap;
    c.group_cap = group_cap;
    c.windows = windows;
    c.n_buffers = n_buffers;
    slisketch::validate(c);
    t_ = std::make_unique<SliSketch>(c);
  }
  int64_t step(const std::vector<std::pair<uintptr_t, size_t>>& spans, int n_groups) {
    SliSketch& sk = t();
    py::gil_scoped_release nogil;
    return sk.step(spans, n_groups);
  }
  py::dict results(int64_t i, int n_groups) {
    SliSketch& sk = t();
    if (n_groups < 0 || n_groups > sk.config().group_cap) throw std::invalid_argument("n_groups");
    const uint32_t* r;
    {
      py::gil_scoped_release nogil;
      r = sk.results(i);
    }
    const slisketch::Layout& l = sk.result_layout();
    const py::ssize_t G = n_groups;
    std::vector<uint64_t> sum((size_t)G);
    for (py::ssize_t g = 0; g < G; ++g)
      sum[(size_t)g] = (uint64_t)r[l.sum + 2 * g] | ((uint64_t)r[l.sum + 2 * g + 1] << 32);
    py::dict d;
    d["n"] = copy_array(r + l.n, {G});
    d["sum_milli"] = copy_array(sum.data(), {G});
    d["le"] = copy_array(r + l.le, {G, slisketch::kLe});
    d["q_win"] = copy_array(r + l.q_win, {G, slisketch::kQuantiles});
    d["n_roll"] = copy_array(r + l.n_roll, {G});
    d["q_roll"] = copy_array(r + l.q_roll, {G, slisketch::kQuantiles});
    d["stats"] = copy_array(r + l.stats, {slisketch::kStats});
    return d;
  }
  py::array_t<uint32_t> rolling() { return rows(true); }
  py::array_t<uint32_t> window_hist() { return rows(false); }

 private:
  py::array_t<uint32_t> rows(bool roll) {
    SliSketch& sk = t();
    std::vector<uint32_t> h;
    {
      py::gil_scoped_release nogil;
      h = roll ? sk.rolling() : sk.window_hist();
    }
    return copy_array(h.data(), {sk.config().group_cap, slisketch::kK});
  }
};

// The request-exemplar tracker (exemplars.h): one step per window over the same span ranges the
// engine gets; results per step index. Rows leave as bytes [.., 64] (pipeline/exemplars.py EXEMPLAR).
class PyExemplarTracker : public PyLane<ExemplarTracker> {
 public:
  PyExemplarTracker(int device, int k, int windows, int64_t span_cap, int group_cap, int n_buffers, bool lds)
      : PyLane("request exemplars") {
    if (span_cap < 1 || span_cap >= (int64_t(1) << 31))
      throw std::invalid_argument("request exemplars: span_cap must be in [1, 2^31)");
    exemplars::Config c;
    c.device = device;
    c.k = k;
    c.windows = windows;
    c.span_cap = (int)span_cap;
    c.group_cap = group_cap;
    c.n_buffers = n_buffers;
    c.lds = lds;
    exemplars::validate(c);
    t_ = std::make_unique<ExemplarTracker>(c);
  }
  int64_t step(const std::vector<std::pair<uintptr_t, size_t>>& spans, int n_groups) {
    ExemplarTracker& ex = t();
    py::gil_scoped_release nogil;
    return ex.step(spans, n_groups);
  }
  py::dict results(int64_t i, int n_groups) {
    ExemplarTracker& ex = t();
    if (n_groups < 0 || n_groups > ex.config().group_cap) throw std::invalid_argument("n_groups");
    const uint32_t* r;
    {
      py::gil_scoped_release nogil;
      r = ex.results(i);
    }
    const exemplars::Layout& l = ex.result_layout();
    const py::ssize_t G = n_groups, K = ex.config().k;
    py::dict d;
    d["n"] = copy_array(r + l.n, {G});
    d["k_win"] = copy_array(r + l.k_win, {G});
    d["k_recent"] = copy_array(r + l.k_recent, {G});
    d["win"] = copy_array(reinterpret_cast<const uint8_t*>(r + l.win), {G, K, exemplars::kRowBytes});
    d["recent"] = copy_array(reinterpret_cast<const uint8_t*>(r + l.recent), {G, K, exemplars::kRowBytes});
    d["stats"] = copy_array(r + l.stats, {exemplars::kStats});
    return d;
  }
  py::tuple resident() {
    ExemplarTracker& ex = t();
    std::pair<std::vector<exemplars::Row>, std::vector<uint32_t>> h;
    {
      py::gil_scoped_release nogil;
      h = ex.resident();
    }
    const py::ssize_t H = ex.config().windows, G = ex.config().group_cap, K = ex.config().k;
    return py::make_tuple(copy_array(reinterpret_cast<const uint8_t*>(h.first.data()), {H, G, K, exemplars::kRowBytes}),
                          copy_array(h.second.data(), {H, G}));
  }
};

// The per-pod breach breakdown (podrank.h): one step per window over the same span ranges the
// engine gets; results per step index. Rows leave as bytes [.., 32] (pipeline/podrank.py POD_ROW).
class PyPodRankTracker : public PyLane<PodRankTracker> {
 public:
  PyPodRankTracker(int device, int k, int windows, int64_t pair_cap, int64_t span_cap, int group_cap, int n_buffers,
                   double slo_ms, bool lds)
      : PyLane("pod breakdown") {
    if (span_cap < 1 || span_cap >= (int64_t(1) << 31))
      throw std::invalid_argument("pod breakdown: span_cap must be >= 1 and span_cap * windows < 2^22");
    if (pair_cap < 1 || pair_cap > podrank::kMaxPairCap)
      throw std::invalid_argument("pod breakdown: pair_cap must be in [1, 2^20]");
    podrank::Config c;
    c.device = device;
    c.k = k;
    c.windows = windows;
    c.pair_cap = (int)pair_cap;
    c.span_cap = (int)span_cap;
    c.group_cap = group_cap;
    c.n_buffers = n_buffers;
    c.slo_ms = slo_ms;
    c.lds = lds;
    podrank::validate(c);
    t_ = std::make_unique<PodRankTracker>(c);
  }
  int64_t step(const std::vector<std::pair<uintptr_t, size_t>>& spans, int n_groups) {
    PodRankTracker& pr = t();
    py::gil_scoped_release nogil;
    return pr.step(spans, n_groups);
  }
  py::dict results(int64_t i, int n_groups) {
    PodRankTracker& pr = t();
    if (n_groups < 0 || n_groups > pr.config().group_cap) throw std::invalid_argument("n_groups");
    const uint32_t* r;
    {
      py::gil_scoped_release nogil;
      r = pr.results(i);
    }
    const podrank::Layout& l = pr.result_layout();
    const py::ssize_t G = n_groups, K = pr.config().k;
    static const char* scope[2] = {"win", "rec"};
    py::dict d;
    for (int s = 0; s < 2; ++s) {
      const std::string p = std::string(scope[s]) + "_";
      d[py::str(p + "n")] = copy_array(r + l.n[s], {G});
      d[py::str(p + "b")] = copy_array(r + l.b[s], {G});
      d[py::str(p + "pods")] = copy_array(r + l.pods[s], {G});
      d[py::str(p + "pods_b")] = copy_array(r + l.pods_b[s], {G});
      d[py::str(p + "k_top")] = copy_array(r + l.k_top[s], {G});
      d[py::str(p + "top")] = copy_array(reinterpret_cast<const uint8_t*>(r + l.top[s]), {G, K, podrank::kRowBytes});
    }
    d["stats"] = copy_array(r + l.stats, {podrank::kStats});
    return d;
  }
  // per horizon slot: (pair keys u64, n, b, max bits, sum_milli u64)
  py::list resident() {
    PodRankTracker& pr = t();
    std::vector<podrank::PairList> h;
    {
      py::gil_scoped_release nogil;
      h = pr.resident();
    }
    py::list out;
    for (const podrank::PairList& l : h) {
      const py::ssize_t n = (py::ssize_t)l.key.size();
      out.append(py::make_tuple(copy_array(reinterpret_cast<const uint64_t*>(l.key.data()), {n}), copy_array(l.n.data(), {n}),
                                copy_array(l.b.data(), {n}), copy_array(l.max.data(), {n}),
                                copy_array(reinterpret_cast<const uint64_t*>(l.sum.data()), {n})));
    }
    return out;
  }
};

// The breach-onset tracker (onset.h): one step per timed window cut over the same span ranges the
// engine gets; results per step index. Rows leave as bytes [G, 64] (pipeline/onset.py ONSET_ROW).
class PyOnsetTracker : public PyLane<OnsetTracker> {
 public:
  PyOnsetTracker(int device, int64_t bins, int64_t bin_ns, int64_t ref_ppm, int64_t alarm, int64_t span_cap, int group_cap,
                 int n_buffers, double slo_ms, int64_t ring_records_max, bool lds)
      : PyLane("breach onset") {
    if (bins < onset::kMinBins || bins > onset::kMaxBins)
      throw std::invalid_argument("breach onset: bins must be a power of two in [64, 8192]");
    if (span_cap < 1) throw std::invalid_argument("breach onset: span_cap must be >= 1");
    if (span_cap >= (int64_t(1) << 31)) throw std::invalid_argument("breach onset: the ring needs more than 2 GiB");
    onset::Config c;
    c.device = device;
    c.bins = (int)bins;
    c.bin_ns = bin_ns;
    c.ref_ppm = ref_ppm;
    c.alarm = alarm;
    c.span_cap = (int)span_cap;
    c.group_cap = group_cap;
    c.n_buffers = n_buffers;
    c.slo_ms = slo_ms;
    c.ring_records_max = ring_records_max;
    c.lds = lds;
    onset::validate(c);
    t_ = std::make_unique<OnsetTracker>(c);
  }
  int64_t step(const std::vector<std::pair<uintptr_t, size_t>>& spans, int64_t cut_ns, int n_groups) {
    OnsetTracker& on = t();
    py::gil_scoped_release nogil;
    return on.step(spans, cut_ns, n_groups);
  }
  py::dict results(int64_t i, int n_groups) {
    OnsetTracker& on = t();
    if (n_groups < 0 || n_groups > on.config().group_cap) throw std::invalid_argument("n_groups");
    const uint32_t* r;
    {
      py::gil_scoped_release nogil;
      r = on.results(i);
    }
    const onset::Layout& l = on.result_layout();
    py::dict d;
    d["rows"] = copy_array(reinterpret_cast<const uint8_t*>(r + l.rows), {(py::ssize_t)n_groups, onset::kRowBytes});
    d["stats"] = copy_array(r + l.stats, {onset::kStats});
    return d;
  }
  // (cells u64 [group_cap, bins] in slot order, q_hi)
  py::tuple resident() {
    OnsetTracker& on = t();
    onset::Resident h;
    {
      py::gil_scoped_release nogil;
      h = on.resident();
    }
    return py::make_tuple(copy_array(reinterpret_cast<const uint64_t*>(h.cells.data()),
                                     {(py::ssize_t)on.config().group_cap, (py::ssize_t)on.config().bins}),
                          h.q_hi);
  }
};

// The decode-phase SLI tracker (decodesli.h): one step per window over the same span ranges the
// engine gets; results per step index (pipeline/decodesli.py RESULT_FIELDS).
class PyDecodeSliTracker : public PyLane<DecodeSliTracker> {
 public:
  PyDecodeSliTracker(int device, int64_t span_cap, int group_cap, int windows, int n_buffers, double slo_ms,
                     double tpot_slo_ms, bool lds)
      : PyLane("decode sli") {
    if (span_cap < 1) throw std::invalid_argument("decode sli: span_cap must be >= 1");
    if (span_cap >= (int64_t(1) << 31)) throw std::invalid_argument("decode sli: the horizon needs more than 2 GiB");
    decodesli::Config c;
    c.device = device;
    c.span_cap = (int)span_cap;
    c.group_cap = group_cap;
    c.windows = windows;
    c.n_buffers = n_buffers;
    c.slo_ms = slo_ms;
    c.tpot_slo_ms = tpot_slo_ms;
    c.lds = lds;
    decodesli::validate(c);
    t_ = std::make_unique<DecodeSliTracker>(c);
  }
  int64_t step(const std::vector<std::pair<uintptr_t, size_t>>& spans, int n_groups) {
    DecodeSliTracker& ds = t();
    py::gil_scoped_release nogil;
    return ds.step(spans, n_groups);
  }
  py::dict results(int64_t i, int n_groups) {
    DecodeSliTracker& ds = t();
    if (n_groups < 0 || n_groups > ds.config().group_cap) throw std::invalid_argument("n_groups");
    const uint32_t* r;
    {
      py::gil_scoped_release nogil;
      r = ds.results(i);
    }
    const decodesli::Layout& l = ds.result_layout();
    const py::ssize_t G = n_groups;
    py::dict d;
    d["cells"] = copy_array(r + l.cells, {G, decodesli::kCells});
    d["cells_roll"] = copy_array(r + l.cells_roll, {G, decodesli::kCells});
    d["sum_us"] = copy_array(reinterpret_cast<const uint64_t*>(r + l.sum), {G});
    d["sum_us_roll"] = copy_array(reinterpret_cast<const uint64_t*>(r + l.sum_roll), {G});
    d["q_win"] = copy_array(r + l.q_win, {G, decodesli::kQuantiles});
    d["q_roll"] = copy_array(r + l.q_roll, {G, decodesli::kQuantiles});
    d["stats"] = copy_array(r + l.stats, {decodesli::kStats});
    return d;
  }
  // (rolling rows u32 [group_cap, K], rolling cells u32 [group_cap, 4], rolling sums u64 [group_cap], ring position)
  py::tuple resident() {
    DecodeSliTracker& ds = t();
    decodesli::Resident h;
    {
      py::gil_scoped_release nogil;
      h = ds.resident();
    }
    const py::ssize_t G = ds.config().group_cap;
    return py::make_tuple(copy_array(h.rows.data(), {G, decodesli::kK}), copy_array(h.cells.data(), {G, decodesli::kCells}),
                          copy_array(reinterpret_cast<const uint64_t*>(h.sums.data()), {G}), h.pos);
  }
};

// The TTFT drift tracker (drift.h): one step per window over the same span ranges the engine gets;
// results per step index (pipeline/drift.py RESULT_FIELDS).
class PyDriftTracker : public PyLane<DriftTracker> {
 public:
  PyDriftTracker(int device, int64_t span_cap, int group_cap, int recent, int gap, int baseline, int n_buffers, double crit,
                 int min_shift, int64_t min_recent, int64_t min_base, int min_base_windows, int64_t hold_max, bool lds)
      : PyLane("ttft drift") {
    if (span_cap < 1) throw std::invalid_argument("ttft drift: span_cap must be >= 1");
    if (span_cap >= (int64_t(1) << 31))
      throw std::invalid_argument("ttft drift: span_cap^2 * recent * baseline must stay below 2^44 (slow_num << 16 would wrap)");
    drift::Config c;
    c.device = device;
    c.span_cap = (int)span_cap;
    c.group_cap = group_cap;
    c.recent = recent;
    c.gap = gap;
    c.baseline = baseline;
    c.n_buffers = n_buffers;
    c.crit = crit;
    c.min_shift = min_shift;
    c.min_recent = min_recent;
    c.min_base = min_base;
    c.min_base_windows = min_base_windows;
    c.hold_max = hold_max;
    c.lds = lds;
    drift::validate(c);
    t_ = std::make_unique<DriftTracker>(c);
  }
  int64_t step(const std::vector<std::pair<uintptr_t, size_t>>& spans, int n_groups) {
    DriftTracker& dt = t();
    py::gil_scoped_release nogil;
    return dt.step(spans, n_groups);
  }
  py::dict results(int64_t i, int n_groups) {
    DriftTracker& dt = t();
    if (n_groups < 0 || n_groups > dt.config().group_cap) throw std::invalid_argument("n_groups");
    const uint32_t* r;
    {
      py::gil_scoped_release nogil;
      r = dt.results(i);
    }
    const drift::Layout& l = dt.result_layout();
    const py::ssize_t G = n_groups;
    py::dict d;
    d["n_win"] = copy_array(r + l.n_win, {G});
    d["n_recent"] = copy_array(r + l.n_recent, {G});
    d["n_base"] = copy_array(r + l.n_base, {G});
    d["base_fill"] = copy_array(r + l.base_fill, {G});
    d["q_recent"] = copy_array(r + l.q_recent, {G, drift::kQuantiles});
    d["q_base"] = copy_array(r + l.q_base, {G, drift::kQuantiles});
    d["slow_num"] = copy_array(reinterpret_cast<const uint64_t*>(r + l.slow_num), {G});
    d["fast_num"] = copy_array(reinterpret_cast<const uint64_t*>(r + l.fast_num), {G});
    d["slow_at"] = copy_array(r + l.slow_at, {G});
    d["fast_at"] = copy_array(r + l.fast_at, {G});
    d["state"] = copy_array(r + l.state, {G});
    d["hold"] = copy_array(r + l.hold, {G});
    d["stats"] = copy_array(r + l.stats, {drift::kStats});
    return d;
  }
  // (recent u32 [group_cap, row stride], base alike, base_fill, base_pos, hold u32 [group_cap], near-ring position)
  py::tuple resident() {
    DriftTracker& dt = t();
    drift::Resident h;
    {
      py::gil_scoped_release nogil;
      h = dt.resident();
    }
    const py::ssize_t G = dt.config().group_cap;
    return py::make_tuple(copy_array(h.recent.data(), {G, drift::kRowStride}), copy_array(h.base.data(), {G, drift::kRowStride}),
                          copy_array(h.base_fill.data(), {G}), copy_array(h.base_pos.data(), {G}),
                          copy_array(h.hold.data(), {G}), h.pos);
  }
};

// The error SLI tracker (errsli.h): one step per window over the same span ranges the engine gets;
// results per step index (pipeline/errsli.py RESULT_FIELDS).
errsli::Config errsli_config(int device, int64_t span_cap, int group_cap, int windows, int n_buffers, double target,
                             const std::vector<std::tuple<int64_t, int64_t, int64_t>>& pairs, int64_t min_requests,
                             int64_t bad_mask, bool lds) {
  if (span_cap < 1) throw std::invalid_argument("error sli: span_cap must be >= 1");
  if (span_cap >= (int64_t(1) << 31)) throw std::invalid_argument("error sli: the horizon needs more than 2 GiB");
  if (bad_mask < 0 || bad_mask > 0xffffffffll) throw std::invalid_argument("error sli: bad_mask must be non-zero and within 0xFE");
  errsli::Config c;
  c.device = device;
  c.span_cap = (int)span_cap;
  c.group_cap = group_cap;
  c.windows = windows;
  c.n_buffers = n_buffers;
  c.target = target;
  c.pairs.clear();
  for (const auto& p : pairs) {
    const int64_t l = std::get<0>(p), s = std::get<1>(p);
    if (l < 1 || l > (int64_t(1) << 30) || s < 1 || s > (int64_t(1) << 30))
      throw std::invalid_argument("error sli: a pair needs 1 <= short <= long <= windows");
    c.pairs.push_back(errsli::Pair{(int)l, (int)s, std::get<2>(p)});
  }
  c.min_requests = min_requests;
  c.bad_mask = (uint32_t)bad_mask;
  c.lds = lds;
  errsli::validate(c);
  return c;
}

class PyErrorSliTracker : public PyLane<ErrorSliTracker> {
 public:
  PyErrorSliTracker(int device, int64_t span_cap, int group_cap, int windows, int n_buffers, double target,
                    const std::vector<std::tuple<int64_t, int64_t, int64_t>>& pairs, int64_t min_requests, int64_t bad_mask,
                    bool lds)
      : PyLane("error sli") {
    t_ = std::make_unique<ErrorSliTracker>(
        errsli_config(device, span_cap, group_cap, windows, n_buffers, target, pairs, min_requests, bad_mask, lds));
  }
  int64_t step(const std::vector<std::pair<uintptr_t, size_t>>& spans, int n_groups) {
    ErrorSliTracker& es = t();
    py::gil_scoped_release nogil;
    return es.step(spans, n_groups);
  }
  uint32_t budget_ppm() { return t().budget_ppm(); }
  py::dict results(int64_t i, int n_groups) {
    ErrorSliTracker& es = t();
    if (n_groups < 0 || n_groups > es.config().group_cap) throw std::invalid_argument("n_groups");
    const uint32_t* r;
    {
      py::gil_scoped_release nogil;
      r = es.results(i);
    }
    const errsli::Layout& l = es.result_layout();
    const py::ssize_t G = n_groups;
    py::dict d;
    d["counts"] = copy_array(r + l.counts, {G, errsli::kClasses});
    d["counts_roll"] = copy_array(r + l.counts_roll, {G, errsli::kClasses});
    d["pair_sums"] = copy_array(r + l.pair_sums, {G, errsli::kMaxPairs, errsli::kPairWords});
    d["firing"] = copy_array(r + l.firing, {G});
    d["age"] = copy_array(r + l.age, {G});
    d["stats"] = copy_array(r + l.stats, {errsli::kStats});
    return d;
  }
  // (rolling counts u32 [group_cap, 8], pair sums u32 [group_cap, 4, 4], ages u32 [group_cap], ring position)
  py::tuple resident() {
    ErrorSliTracker& es = t();
    errsli::Resident h;
    {
      py::gil_scoped_release nogil;
      h = es.resident();
    }
    const py::ssize_t G = es.config().group_cap;
    return py::make_tuple(copy_array(h.counts.data(), {G, errsli::kClasses}),
                          copy_array(h.sums.data(), {G, errsli::kMaxPairs, errsli::kPairWords}),
                          copy_array(h.age.data(), {G}), h.pos);
  }
};

// The load SLI tracker (loadsli.h): one step per timed window cut over the same span ranges the
// engine gets; results per step index. Rows leave as bytes [G, 80] (pipeline/loadsli.py LOAD_ROW).
class PyLoadSliTracker : public PyLane<LoadSliTracker> {
 public:
  PyLoadSliTracker(int device, int64_t bins, int64_t bin_us, int64_t settle_bins, int64_t recent_bins, int64_t min_base_bins,
                   int64_t factor_milli, int64_t min_requests, int64_t min_conc_milli, int64_t span_cap, int group_cap,
                   int n_buffers, int64_t ring_records_max, bool lds)
      : PyLane("load sli") {
    if (bins < loadsli::kMinBins || bins > loadsli::kMaxBins)
      throw std::invalid_argument("load sli: bins must be a power of two in [64, 8192]");
    if (span_cap < 1) throw std::invalid_argument("load sli: span_cap must be >= 1");
    if (span_cap >= (int64_t(1) << 31)) throw std::invalid_argument("load sli: the ring needs more than 2 GiB");
    auto small = [](int64_t v) { return v < -1 ? -1 : (v > (int64_t(1) << 30) ? (1 << 30) : (int)v); };
    loadsli::Config c;
    c.device = device;
    c.bins = (int)bins;
    c.bin_us = bin_us;
    c.settle_bins = small(settle_bins);
    c.recent_bins = small(recent_bins);
    c.min_base_bins = small(min_base_bins);
    c.factor_milli = factor_milli;
    c.min_requests = min_requests;
    c.min_conc_milli = min_conc_milli;
    c.span_cap = (int)span_cap;
    c.group_cap = group_cap;
    c.n_buffers = n_buffers;
    c.ring_records_max = ring_records_max;
    c.lds = lds;
    loadsli::validate(c);
    t_ = std::make_unique<LoadSliTracker>(c);
  }
  int64_t step(const std::vector<std::pair<uintptr_t, size_t>>& spans, int64_t cut_ns, int n_groups) {
    LoadSliTracker& ls = t();
    py::gil_scoped_release nogil;
    return ls.step(spans, cut_ns, n_groups);
  }
  py::dict results(int64_t i, int n_groups) {
    LoadSliTracker& ls = t();
    if (n_groups < 0 || n_groups > ls.config().group_cap) throw std::invalid_argument("n_groups");
    const uint32_t* r;
    {
      py::gil_scoped_release nogil;
      r = ls.results(i);
    }
    const loadsli::Layout& l = ls.result_layout();
    py::dict d;
    d["rows"] = copy_array(reinterpret_cast<const uint8_t*>(r + l.rows), {(py::ssize_t)n_groups, loadsli::kRowBytes});
    d["stats"] = copy_array(r + l.stats, {loadsli::kStats});
    return d;
  }
  // the step's whole result block, uint32 words
  // (counts u64, idle_us u64 [group_cap, bins] in slot order, carry, age, previous state, q_hi, q_first)
  py::tuple resident() {
    LoadSliTracker& ls = t();
    loadsli::Resident h;
    {
      py::gil_scoped_release nogil;
      h = ls.resident();
    }
    const py::ssize_t G = ls.config().group_cap, B = ls.config().bins;
    return py::make_tuple(copy_array(reinterpret_cast<const uint64_t*>(h.counts.data()), {G, B}),
                          copy_array(reinterpret_cast<const uint64_t*>(h.idle_us.data()), {G, B}),
                          copy_array(h.carry.data(), {G}), copy_array(h.age.data(), {G}),
                          copy_array(h.prev_state.data(), {G}), h.q_hi, h.q_first);
  }
};

// The saturation curve tracker (satcurve.h): one step per timed window cut over the same span ranges
// the engine gets; results per step index. Rows leave as bytes [G, 64] (pipeline/satcurve.py SAT_ROW),
// the merged curve as u64 [G, 160, 2].
class PySaturationTracker : public PyLane<SaturationTracker> {
 public:
  PySaturationTracker(int device, int64_t bins, int64_t bin_us, int64_t settle_bins, int64_t recent_bins, int64_t epoch_bins,
                      int64_t budget_ppm, int64_t min_requests, double slo_ms, int64_t span_cap, int group_cap, int n_buffers,
                      int64_t ring_records_max, int64_t curve_records_max, bool lds)
      : PyLane("saturation curve") {
    if (bins < satcurve::kMinBins || bins > satcurve::kMaxBins)
      throw std::invalid_argument("saturation curve: bins must be a power of two in [64, 8192]");
    if (span_cap < 1) throw std::invalid_argument("saturation curve: span_cap must be >= 1");
    if (span_cap >= (int64_t(1) << 31)) throw std::invalid_argument("saturation curve: the ring needs more than 2 GiB");
    auto small = [](int64_t v) { return v < -1 ? -1 : (v > (int64_t(1) << 30) ? (1 << 30) : (int)v); };
    satcurve::Config c;
    c.device = device;
    c.bins = (int)bins;
    c.bin_us = bin_us;
    c.settle_bins = small(settle_bins);
    c.recent_bins = small(recent_bins);
    c.epoch_bins = epoch_bins;
    c.budget_ppm = budget_ppm;
    c.min_requests = min_requests;
    c.slo_ms = slo_ms;
    c.span_cap = (int)span_cap;
    c.group_cap = group_cap;
    c.n_buffers = n_buffers;
    c.ring_records_max = ring_records_max;
    c.curve_records_max = curve_records_max;
    c.lds = lds;
    satcurve::validate(c);
    t_ = std::make_unique<SaturationTracker>(c);
  }
  int64_t step(const std::vector<std::pair<uintptr_t, size_t>>& spans, int64_t cut_ns, int n_groups) {
    SaturationTracker& st = t();
    py::gil_scoped_release nogil;
    return st.step(spans, cut_ns, n_groups);
  }
  py::dict results(int64_t i, int n_groups) {
    SaturationTracker& st = t();
    if (n_groups < 0 || n_groups > st.config().group_cap) throw std::invalid_argument("n_groups");
    const uint32_t* r;
    {
      py::gil_scoped_release nogil;
      r = st.results(i);
    }
    const satcurve::Layout& l = st.result_layout();
    py::dict d;
    d["rows"] = copy_array(reinterpret_cast<const uint8_t*>(r + l.rows), {(py::ssize_t)n_groups, satcurve::kRowBytes});
    d["curve"] = copy_array(reinterpret_cast<const uint64_t*>(r + l.curve), {(py::ssize_t)n_groups, satcurve::kK, 2});
    d["stats"] = copy_array(r + l.stats, {satcurve::kStats});
    return d;
  }
  // the step's whole result block, uint32 words
  // (counts, idle_us, sli u64 [group_cap, bins] in slot order, carry, gen u64 [2, group_cap, 160, 2], gen_epoch, age,
  // q_hi, q_first)
  py::tuple resident() {
    SaturationTracker& st = t();
    satcurve::Resident h;
    {
      py::gil_scoped_release nogil;
      h = st.resident();
    }
    const py::ssize_t G = st.config().group_cap, B = st.config().bins;
    return py::make_tuple(copy_array(reinterpret_cast<const uint64_t*>(h.counts.data()), {G, B}),
                          copy_array(reinterpret_cast<const uint64_t*>(h.idle_us.data()), {G, B}),
                          copy_array(reinterpret_cast<const uint64_t*>(h.sli.data()), {G, B}), copy_array(h.carry.data(), {G}),
                          copy_array(reinterpret_cast<const uint64_t*>(h.gen.data()), {2, G, satcurve::kK, 2}),
                          py::make_tuple(h.gen_epoch[0], h.gen_epoch[1]), copy_array(h.age.data(), {G}), h.q_hi, h.q_first);
  }
};

// The TTFT phase split tracker (retrsli.h): one step per window over the same span ranges the engine
// gets; results per step index (pipeline/retrsli.py RESULT_FIELDS).
class PyRetrievalSliTracker : public PyLane<RetrievalSliTracker> {
 public:
  PyRetrievalSliTracker(int device, int64_t span_cap, int group_cap, int windows, int n_buffers, double slo_ms,
                        double retrieval_budget_ms, int64_t budget_ppm, int64_t coverage_ppm, int64_t dominance_ppm,
                        int64_t min_requests, bool lds)
      : PyLane("retrieval sli") {
    if (span_cap < 1) throw std::invalid_argument("retrieval sli: span_cap must be >= 1");
    if (span_cap >= (int64_t(1) << 31)) throw std::invalid_argument("retrieval sli: the horizon needs more than 2 GiB");
    retrsli::Config c;
    c.device = device;
    c.span_cap = (int)span_cap;
    c.group_cap = group_cap;
    c.windows = windows;
    c.n_buffers = n_buffers;
    c.slo_ms = slo_ms;
    c.retrieval_budget_ms = retrieval_budget_ms;
    c.budget_ppm = budget_ppm;
    c.coverage_ppm = coverage_ppm;
    c.dominance_ppm = dominance_ppm;
    c.min_requests = min_requests;
    c.lds = lds;
    retrsli::validate(c);
    t_ = std::make_unique<RetrievalSliTracker>(c);
  }
  int64_t step(const std::vector<std::pair<uintptr_t, size_t>>& spans, int n_groups) {
    RetrievalSliTracker& rs = t();
    py::gil_scoped_release nogil;
    return rs.step(spans, n_groups);
  }
  py::dict results(int64_t i, int n_groups) {
    RetrievalSliTracker& rs = t();
    if (n_groups < 0 || n_groups > rs.config().group_cap) throw std::invalid_argument("n_groups");
    const uint32_t* r;
    {
      py::gil_scoped_release nogil;
      r = rs.results(i);
    }
    const retrsli::Layout& l = rs.result_layout();
    const py::ssize_t G = n_groups;
    const auto sums = [&](size_t at) { return copy_array(reinterpret_cast<const uint64_t*>(r + at), {G}); };
    py::dict d;
    d["cells"] = cut_cells(r + l.cells, G);
    d["cells_roll"] = cut_cells(r + l.cells_roll, G);
    d["sum_r"] = sums(l.sum_r);
    d["sum_t"] = sums(l.sum_t);
    d["sum_r_roll"] = sums(l.sum_r_roll);
    d["sum_t_roll"] = sums(l.sum_t_roll);
    d["sli"] = copy_array(r + l.sli, {G});
    d["sli_roll"] = copy_array(r + l.sli_roll, {G});
    d["q_r_win"] = copy_array(r + l.q_r_win, {G, retrsli::kQuantiles});
    d["q_r_roll"] = copy_array(r + l.q_r_roll, {G, retrsli::kQuantiles});
    d["q_m_win"] = copy_array(r + l.q_m_win, {G, retrsli::kQuantiles});
    d["q_m_roll"] = copy_array(r + l.q_m_roll, {G, retrsli::kQuantiles});
    d["state"] = copy_array(r + l.state, {G});
    d["age"] = copy_array(r + l.age, {G});
    d["stats"] = copy_array(r + l.stats, {retrsli::kStats});
    return d;
  }
  // (rolling retrieval rows u32 [group_cap, K], rolling model rows, rolling cells u32 [group_cap, 6], rolling sli u32
  // [group_cap], rolling sums u64 [group_cap, 2], state, age, ring position)
  py::tuple resident() {
    RetrievalSliTracker& rs = t();
    retrsli::Resident h;
    {
      py::gil_scoped_release nogil;
      h = rs.resident();
    }
    const py::ssize_t G = rs.config().group_cap;
    py::array_t<uint32_t> sli({G});
    for (py::ssize_t g = 0; g < G; ++g) sli.mutable_data()[g] = h.cells[(size_t)g * retrsli::kCellStride + retrsli::kSliWord];
    return py::make_tuple(copy_array(h.rows_r.data(), {G, retrsli::kK}), copy_array(h.rows_m.data(), {G, retrsli::kK}),
                          cut_cells(h.cells.data(), G), sli, copy_array(reinterpret_cast<const uint64_t*>(h.sums.data()), {G, 2}),
                          copy_array(h.state.data(), {G}), copy_array(h.age.data(), {G}), h.pos);
  }

 private:
  // [G][kCellStride] words -> the six cells of each row
  static py::array_t<uint32_t> cut_cells(const uint32_t* p, py::ssize_t G) {
    py::array_t<uint32_t> a({G, (py::ssize_t)retrsli::kCells});
    for (py::ssize_t g = 0; g < G; ++g)
      std::memcpy(a.mutable_data() + g * retrsli::kCells, p + g * retrsli::kCellStride, retrsli::kCells * sizeof(uint32_t));
    return a;
  }
};

py::bytes unique_id() {
  ncclUniqueId u;
  const ncclResult_t r = ncclGetUniqueId(&u);
  if (r != ncclSuccess) throw std::runtime_error(std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
  return py::bytes(reinterpret_cast<const char*>(&u), sizeof(u));
}

PYBIND11_MODULE(_mislo_agent, m) {
  m.doc() = "MI355X LLM-SLO native window engine (HIP + RCCL, no PyTorch)";
  m.def("set_tables", &set_tables_np);
  m.def("unique_id", &unique_id);
  m.def("device_count", []() {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
  });
  m.attr("PACKET_LEN") = kPacketLen;
  m.attr("PACKET_LAYOUT") = py::make_tuple(kPacketHist, kPacketStatus, kPacketMisc, kPacketDbg, kPacketConf,
                                           kPacketStats, kPacketCount, kPacketRing);
  m.attr("STATS_OFF") = kStatsOff;
  m.attr("STATS_LEN") = kStatsLen;
  m.attr("POSTERIOR_MODEL_BYTES") = (int64_t)sizeof(PosteriorModel);
  m.attr("APP_MODEL_BYTES") = (int64_t)sizeof(AppModel);
  m.attr("APP_EVIDENCE_BIT") = kAppBit;
  m.attr("CTX_ROWS") = kCtxRows;
  m.attr("REC_STRIDE") = kRecStride;
  m.attr("SIGREC_BYTES") = (int)sizeof(SigRec);
  m.attr("RING_STATE") =
      py::make_tuple("first_busy", "foreign", "def_ctx", "def_trace", "discarded", "events", "other_shard");
  // the checkpoint image of a side tracker (steplane_host.h namespace lane)
  m.attr("LANE_IMAGE_HEADER_BYTES") = (int64_t)sizeof(lane::ImageHeader);
  m.attr("LANE_IMAGE_VERSION") = lane::kVersion;
  m.def("lane_digest", [](py::buffer payload) {
    const py::buffer_info bi = payload.request();
    if (bi.ndim != 1 || bi.strides[0] != bi.itemsize) throw std::invalid_argument("lane_digest: a contiguous one-dimensional buffer");
    const size_t bytes = (size_t)bi.size * (size_t)bi.itemsize;
    if (bytes % lane::kChunk) throw std::invalid_argument("lane_digest: whole 16-byte chunks");
    return lane::digest(bi.ptr, bytes);
  });
  // (kind, fingerprint, step, [array bytes], [field values], [host words], payload bytes, digest) of an image's header
  m.def("lane_image_header", [](py::buffer image) {
    const py::buffer_info bi = image.request();
    if (bi.ndim != 1 || bi.strides[0] != bi.itemsize || (size_t)bi.size * (size_t)bi.itemsize < sizeof(lane::ImageHeader))
      throw std::invalid_argument("lane_image_header: shorter than a header");
    lane::ImageHeader h;
    std::memcpy(&h, bi.ptr, sizeof(h));
    if (h.magic != lane::kMagic || h.n_segments > (uint32_t)lane::kMaxSegments || h.n_fields > (uint32_t)lane::kMaxFields ||
        h.n_host > (uint32_t)lane::kHostWords)
      throw std::invalid_argument("lane_image_header: not an image header");
    return py::make_tuple(std::string(lane::kind_name(h.kind)), h.fingerprint, h.step,
                          std::vector<uint64_t>(h.seg_bytes, h.seg_bytes + h.n_segments),
                          std::vector<int64_t>(h.fields, h.fields + h.n_fields), std::vector<int64_t>(h.host, h.host + h.n_host),
                          h.payload_bytes, h.digest);
  });
  m.attr("OPENREQ_LDS_GROUPS") = openreq::kLdsGroups;
  m.attr("OPENREQ_MAX_PROBES") = openreq::kMaxProbes;
  m.attr("OPENREQ_STATS") = (int)openreq::kStats;
  PyOpenRequests::def_checkpoint(py::class_<PyOpenRequests>(m, "OpenRequests")
      .def(py::init<int, int64_t, int, int, int, double, double, double>(), py::arg("device") = 0,
           py::arg("cap") = (int64_t)1 << 20, py::arg("span_cap") = 16384, py::arg("group_cap") = 64,
           py::arg("n_buffers") = 3, py::arg("slo_ms") = 800.0, py::arg("ttl_ms") = 120000.0,
           py::arg("reorder_ms") = 2000.0)
      .def("step", &PyOpenRequests::step, py::arg("spans"), py::arg("cut_ns"), py::arg("prev_cut_ns"),
           py::arg("n_groups"))
      .def("query", &PyOpenRequests::query)
      .def("results", &PyOpenRequests::results)
      .def("step_ms", &PyOpenRequests::step_ms)
      .def("entries", &PyOpenRequests::entries)
      .def("sync", &PyOpenRequests::sync)
      .def("close", &PyOpenRequests::close));
  m.attr("SLISKETCH_K") = slisketch::kK;
  m.attr("SLISKETCH_LO_KEY") = slisketch::kLo;
  m.attr("SLISKETCH_STATS") = (int)slisketch::kStats;
  {
    py::list edges, q;
    for (int j = 0; j < slisketch::kEdges; ++j) edges.append((double)slisketch::le_edge(j));
    for (int j = 0; j < slisketch::kQuantiles; ++j) q.append(slisketch::quantile_permille(j));
    m.attr("SLISKETCH_EDGES") = py::tuple(edges);
    m.attr("SLISKETCH_PERMILLE") = py::tuple(q);
  }
  PySliSketch::def_checkpoint(py::class_<PySliSketch>(m, "SliSketch")
      .def(py::init<int, int, int, int, int>(), py::arg("device") = 0, py::arg("span_cap") = 16384,
           py::arg("group_cap") = 64, py::arg("windows") = 150, py::arg("n_buffers") = 3)
      .def("step", &PySliSketch::step, py::arg("spans"), py::arg("n_groups"))
      .def("query", &PySliSketch::query)
      .def("results", &PySliSketch::results)
      .def("step_ms", &PySliSketch::step_ms)
      .def("rolling", &PySliSketch::rolling)
      .def("window_hist", &PySliSketch::window_hist)
      .def("sync", &PySliSketch::sync)
      .def("close", &PySliSketch::close));
  m.attr("EXEMPLAR_MAX_K") = exemplars::kMaxK;
  m.attr("EXEMPLAR_MAX_H") = exemplars::kMaxH;
  m.attr("EXEMPLAR_LDS_GROUPS") = exemplars::kLdsGroups;
  m.attr("EXEMPLAR_ROW_BYTES") = exemplars::kRowBytes;
  m.attr("EXEMPLAR_STATS") = (int)exemplars::kStats;
  PyExemplarTracker::def_checkpoint(py::class_<PyExemplarTracker>(m, "ExemplarTracker")
      .def(py::init<int, int, int, int64_t, int, int, bool>(), py::arg("device") = 0, py::arg("k") = 3,
           py::arg("windows") = 3, py::arg("span_cap") = 16384, py::arg("group_cap") = 64, py::arg("n_buffers") = 3,
           py::arg("lds") = true)
      .def("step", &PyExemplarTracker::step, py::arg("spans"), py::arg("n_groups"))
      .def("query", &PyExemplarTracker::query)
      .def("results", &PyExemplarTracker::results)
      .def("step_ms", &PyExemplarTracker::step_ms)
      .def("resident", &PyExemplarTracker::resident)
      .def("sync", &PyExemplarTracker::sync)
      .def("close", &PyExemplarTracker::close));
  m.attr("PODRANK_MAX_K") = podrank::kMaxK;
  m.attr("PODRANK_MAX_H") = podrank::kMaxH;
  m.attr("PODRANK_ROW_BYTES") = podrank::kRowBytes;
  m.attr("PODRANK_STATS") = (int)podrank::kStats;
  m.attr("PODRANK_LDS_SLOTS") = podrank::kLdsSlots;
  m.def("podrank_slot_of", [](uint32_t g, uint32_t pod, uint32_t slots) { return podrank::slot_of(g, pod, slots); });
  PyPodRankTracker::def_checkpoint(py::class_<PyPodRankTracker>(m, "PodRankTracker")
      .def(py::init<int, int, int, int64_t, int64_t, int, int, double, bool>(), py::arg("device") = 0, py::arg("k") = 3,
           py::arg("windows") = 3, py::arg("pair_cap") = 4096, py::arg("span_cap") = 16384, py::arg("group_cap") = 64,
           py::arg("n_buffers") = 3, py::arg("slo_ms") = 800.0, py::arg("lds") = true)
      .def("step", &PyPodRankTracker::step, py::arg("spans"), py::arg("n_groups"))
      .def("query", &PyPodRankTracker::query)
      .def("results", &PyPodRankTracker::results)
      .def("step_ms", &PyPodRankTracker::step_ms)
      .def("resident", &PyPodRankTracker::resident)
      .def("sync", &PyPodRankTracker::sync)
      .def("close", &PyPodRankTracker::close));
  m.attr("ONSET_ROW_BYTES") = onset::kRowBytes;
  m.attr("ONSET_STATS") = (int)onset::kStats;
  m.attr("ONSET_LDS_SLOTS") = onset::kLdsSlots;
  m.attr("ONSET_BINS") = py::make_tuple(onset::kMinBins, onset::kMaxBins);
  PyOnsetTracker::def_checkpoint(py::class_<PyOnsetTracker>(m, "OnsetTracker")
      .def(py::init<int, int64_t, int64_t, int64_t, int64_t, int64_t, int, int, double, int64_t, bool>(),
           py::arg("device") = 0, py::arg("bins") = 1024, py::arg("bin_ns") = (int64_t)125000000,
           py::arg("ref_ppm") = (int64_t)20000, py::arg("alarm") = (int64_t)3, py::arg("span_cap") = 16384,
           py::arg("group_cap") = 64, py::arg("n_buffers") = 3, py::arg("slo_ms") = 800.0,
           py::arg("ring_records_max") = onset::kMaxRingRecords, py::arg("lds") = true)
      .def("step", &PyOnsetTracker::step, py::arg("spans"), py::arg("cut_ns"), py::arg("n_groups"))
      .def("query", &PyOnsetTracker::query)
      .def("results", &PyOnsetTracker::results)
      .def("step_ms", &PyOnsetTracker::step_ms)
      .def("resident", &PyOnsetTracker::resident)
      .def("sync", &PyOnsetTracker::sync)
      .def("close", &PyOnsetTracker::close));
  m.attr("DECODESLI_K") = decodesli::kK;
  m.attr("DECODESLI_STATS") = (int)decodesli::kStats;
  m.attr("DECODESLI_LDS_SLOTS") = decodesli::kLdsSlots;
  m.attr("DECODESLI_PER_LANE") = decodesli::kPerLane;
  m.def("decodesli_bucket_of", [](uint32_t u) { return decodesli::bucket_of(u); });
  m.def("decodesli_tpot_slo_us", [](double ms) { return decodesli::tpot_slo_us(ms); });
  PyDecodeSliTracker::def_checkpoint(py::class_<PyDecodeSliTracker>(m, "DecodeSliTracker")
      .def(py::init<int, int64_t, int, int, int, double, double, bool>(), py::arg("device") = 0,
           py::arg("span_cap") = 16384, py::arg("group_cap") = 64, py::arg("windows") = 150, py::arg("n_buffers") = 3,
           py::arg("slo_ms") = 800.0, py::arg("tpot_slo_ms") = 100.0, py::arg("lds") = true)
      .def("step", &PyDecodeSliTracker::step, py::arg("spans"), py::arg("n_groups"))
      .def("query", &PyDecodeSliTracker::query)
      .def("results", &PyDecodeSliTracker::results)
      .def("block", &PyDecodeSliTracker::block)
      .def("step_ms", &PyDecodeSliTracker::step_ms)
      .def("resident", &PyDecodeSliTracker::resident)
      .def("sync", &PyDecodeSliTracker::sync)
      .def("close", &PyDecodeSliTracker::close));
  m.attr("DRIFT_K") = drift::kK;
  m.attr("DRIFT_ROW_STRIDE") = drift::kRowStride;
  m.attr("DRIFT_STATS") = (int)drift::kStats;
  m.attr("DRIFT_LDS_SLOTS") = drift::kLdsSlots;
  m.attr("DRIFT_PER_LANE") = drift::kPerLane;
  m.attr("DRIFT_SLOW") = drift::kSlow;
  m.attr("DRIFT_FAST") = drift::kFast;
  m.attr("DRIFT_WARMING") = drift::kWarming;
  m.attr("DRIFT_REBASED") = drift::kRebased;
  m.def("drift_crit_q", [](double c2) { return drift::crit_q(c2); });
  // the state bits of one service before hold and reset (drift_host.h decide), for a host-side cross-check
  m.def(
      "drift_decide",
      [](uint32_t n_r, uint32_t n_b, uint32_t base_fill, uint64_t slow_num, uint64_t fast_num,
         const std::vector<uint32_t>& q_recent, const std::vector<uint32_t>& q_base, double crit, uint32_t min_shift,
         uint32_t min_recent, uint32_t min_base, uint32_t min_base_windows) {
        if (q_recent.size() != (size_t)drift::kQuantiles || q_base.size() != (size_t)drift::kQuantiles)
          throw std::invalid_argument("drift_decide: four quantile buckets a row");
        if ((uint64_t)n_r * n_b >= (uint64_t(1) << 44) || slow_num > (uint64_t)n_r * n_b || fast_num > (uint64_t)n_r * n_b)
          throw std::invalid_argument("drift_decide: n_r * n_b must stay below 2^44 and bound the numerators");
        drift::Thresholds t;
        t.crit_q = drift::crit_q(crit);
        t.min_shift = min_shift;
        t.min_recent = min_recent;
        t.min_base = min_base;
        t.min_base_windows = min_base_windows;
        return drift::decide(n_r, n_b, base_fill, slow_num, fast_num, q_recent.data(), q_base.data(), t);
      },
      py::arg("n_r"), py::arg("n_b"), py::arg("base_fill"), py::arg("slow_num"), py::arg("fast_num"), py::arg("q_recent"),
      py::arg("q_base"), py::arg("crit") = 4.0, py::arg("min_shift") = 2, py::arg("min_recent") = 30,
      py::arg("min_base") = 100, py::arg("min_base_windows") = 10);
  PyDriftTracker::def_checkpoint(py::class_<PyDriftTracker>(m, "DriftTracker")
      .def(py::init<int, int64_t, int, int, int, int, int, double, int, int64_t, int64_t, int, int64_t, bool>(),
           py::arg("device") = 0, py::arg("span_cap") = 16384, py::arg("group_cap") = 64, py::arg("recent") = 10,
           py::arg("gap") = 10, py::arg("baseline") = 300, py::arg("n_buffers") = 3, py::arg("crit") = 4.0,
           py::arg("min_shift") = 2, py::arg("min_recent") = 30, py::arg("min_base") = 100,
           py::arg("min_base_windows") = 10, py::arg("hold_max") = 1200, py::arg("lds") = true)
      .def("step", &PyDriftTracker::step, py::arg("spans"), py::arg("n_groups"))
      .def("query", &PyDriftTracker::query)
      .def("results", &PyDriftTracker::results)
      .def("block", &PyDriftTracker::block)
      .def("step_ms", &PyDriftTracker::step_ms)
      .def("resident", &PyDriftTracker::resident)
      .def("sync", &PyDriftTracker::sync)
      .def("close", &PyDriftTracker::close));
  m.attr("ERRSLI_CLASSES") = errsli::kClasses;
  m.attr("ERRSLI_MAX_PAIRS") = errsli::kMaxPairs;
  m.attr("ERRSLI_STATS") = (int)errsli::kStats;
  m.attr("ERRSLI_LDS_SLOTS") = errsli::kLdsSlots;
  m.attr("ERRSLI_BAD_DEFAULT") = errsli::kBadDefault;
  m.def("errsli_outcome_of", [](uint32_t flags) { return errsli::outcome_of(flags); });
  m.def("errsli_pack_outcome", [](uint32_t c) { return errsli::pack_outcome(c); });
  m.def("errsli_budget_ppm", [](double target) { return errsli::budget_ppm(target); });
  m.def("errsli_burns", [](uint32_t n, uint32_t bad, uint32_t min_requests, uint64_t thr) {
    return errsli::burns(n, bad, min_requests, thr);
  });
  m.def("errsli_next_age", [](uint32_t age, uint32_t firing) { return errsli::next_age(age, firing); });
  m.def("errsli_layout", [](int group_cap) {
    const errsli::Layout l = errsli::layout(group_cap);
    py::dict d;
    d["counts"] = l.counts, d["counts_roll"] = l.counts_roll, d["pair_sums"] = l.pair_sums, d["firing"] = l.firing;
    d["age"] = l.age, d["stats"] = l.stats, d["words"] = l.words;
    return d;
  });
  m.def("errsli_device_bytes", [](int64_t span_cap, int group_cap, int windows) {
    errsli::Config c;
    c.span_cap = (int)span_cap, c.group_cap = group_cap, c.windows = windows;
    return errsli::device_bytes(c);
  });
  PyErrorSliTracker::def_checkpoint(py::class_<PyErrorSliTracker>(m, "ErrorSliTracker")
      .def(py::init<int, int64_t, int, int, int, double, const std::vector<std::tuple<int64_t, int64_t, int64_t>>&, int64_t,
                    int64_t, bool>(),
           py::arg("device") = 0, py::arg("span_cap") = 16384, py::arg("group_cap") = 64, py::arg("windows") = 3600,
           py::arg("n_buffers") = 3, py::arg("target") = 0.999,
           py::arg("pairs") = std::vector<std::tuple<int64_t, int64_t, int64_t>>{{3600, 300, 14400}},
           py::arg("min_requests") = 20, py::arg("bad_mask") = (int64_t)errsli::kBadDefault, py::arg("lds") = true)
      .def("step", &PyErrorSliTracker::step, py::arg("spans"), py::arg("n_groups"))
      .def("query", &PyErrorSliTracker::query)
      .def("budget_ppm", &PyErrorSliTracker::budget_ppm)
      .def("results", &PyErrorSliTracker::results)
      .def("block", &PyErrorSliTracker::block)
      .def("step_ms", &PyErrorSliTracker::step_ms)
      .def("resident", &PyErrorSliTracker::resident)
      .def("sync", &PyErrorSliTracker::sync)
      .def("close", &PyErrorSliTracker::close));
  m.attr("LOADSLI_ROW_BYTES") = loadsli::kRowBytes;
  m.attr("LOADSLI_STATS") = (int)loadsli::kStats;
  m.attr("LOADSLI_LDS_SLOTS") = loadsli::kLdsSlots;
  m.attr("LOADSLI_BINS") = py::make_tuple(loadsli::kMinBins, loadsli::kMaxBins);
  // -1 for a latency the tracker counts as invalid
  m.def("loadsli_dur_us", [](float latency_ms) {
    return loadsli::latency_valid(latency_ms) ? loadsli::dur_us_of(latency_ms) : (int64_t)-1;
  });
  m.def("loadsli_place", [](int64_t ts_us, int64_t dur_us, int64_t bin_us, int64_t q_hi, uint32_t bins) {
    const loadsli::Placement p = loadsli::place(ts_us, dur_us, bin_us, q_hi, bins);
    return py::make_tuple(p.bits, p.qs, p.qe, p.idle_s, p.idle_e);
  });
  // (flags, state) of a row that is not warming
  m.def("loadsli_classify", [](uint64_t busy_recent, uint64_t busy_base, uint32_t arr_recent, uint32_t arr_base,
                               uint32_t base_bins, uint32_t recent_bins, int64_t bin_us, int64_t factor_milli,
                               int64_t min_requests, int64_t min_conc_milli) {
    if (base_bins < 1 || recent_bins < 1 || bin_us < 1) throw std::invalid_argument("load sli classify: empty range");
    const loadsli::Sums s{busy_recent, busy_base, arr_recent, arr_base};
    const uint32_t f = loadsli::predicates(s, base_bins, recent_bins, bin_us, factor_milli, min_requests, min_conc_milli);
    return py::make_tuple(f, loadsli::state_of(f));
  });
  m.def("loadsli_age", [](uint32_t state, uint32_t prev_state, uint32_t prev_age) {
    return loadsli::age_of(state, prev_state, prev_age);
  });
  m.def("loadsli_layout", [](int group_cap) {
    const loadsli::Layout l = loadsli::layout(group_cap);
    py::dict d;
    d["rows"] = l.rows, d["stats"] = l.stats, d["words"] = l.words;
    return d;
  });
  m.def("loadsli_device_bytes", [](int bins, int64_t span_cap, int group_cap) {
    return loadsli::device_bytes(bins, (int)span_cap, group_cap);
  });
  m.def("loadsli_ring_records_max", [](int bins, int64_t bin_us) { return loadsli::default_ring_records_max(bins, bin_us); });
  PyLoadSliTracker::def_checkpoint(py::class_<PyLoadSliTracker>(m, "LoadSliTracker")
      .def(py::init<int, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int, int, int64_t,
                    bool>(),
           py::arg("device") = 0, py::arg("bins") = 1024, py::arg("bin_us") = 500000, py::arg("settle_bins") = 30,
           py::arg("recent_bins") = 30, py::arg("min_base_bins") = 60, py::arg("factor_milli") = 1500,
           py::arg("min_requests") = 20, py::arg("min_conc_milli") = 1000, py::arg("span_cap") = 16384,
           py::arg("group_cap") = 64, py::arg("n_buffers") = 3,
           py::arg("ring_records_max") = loadsli::default_ring_records_max(1024, 500000), py::arg("lds") = true)
      .def("step", &PyLoadSliTracker::step, py::arg("spans"), py::arg("cut_ns"), py::arg("n_groups"))
      .def("query", &PyLoadSliTracker::query)
      .def("results", &PyLoadSliTracker::results)
      .def("block", &PyLoadSliTracker::block)
      .def("step_ms", &PyLoadSliTracker::step_ms)
      .def("resident", &PyLoadSliTracker::resident)
      .def("sync", &PyLoadSliTracker::sync)
      .def("close", &PyLoadSliTracker::close));
  m.attr("SATCURVE_ROW_BYTES") = satcurve::kRowBytes;
  m.attr("SATCURVE_STATS") = (int)satcurve::kStats;
  m.attr("SATCURVE_LEVELS") = satcurve::kK;
  m.attr("SATCURVE_LDS_SLOTS") = satcurve::kLdsSlots;
  m.attr("SATCURVE_BINS") = py::make_tuple(satcurve::kMinBins, satcurve::kMaxBins);
  m.attr("SATCURVE_CURVE_RECORDS_MAX") = satcurve::kMaxCurveRecords;
  // (u, level) of a busy time over a span of time, and a level's smallest u
  m.def("satcurve_level", [](int64_t busy_us, int64_t span_us) {
    if (span_us < 1) throw std::invalid_argument("saturation curve level: empty span");
    const uint32_t u = satcurve::u_of(busy_us, span_us);
    return py::make_tuple(u, satcurve::level_of_u(u));
  });
  m.def("satcurve_lower", [](uint32_t level) { return satcurve::lower_u(level); });
  // (level or 0xffffffff, n, b, valid) of a curve u64 [160, 2]
  m.def("satcurve_knee", [](py::array_t<uint64_t, py::array::c_style | py::array::forcecast> curve, int64_t budget_ppm,
                            int64_t min_requests) {
    if (curve.size() != satcurve::kK * 2) throw std::invalid_argument("saturation curve knee: the curve is [160, 2]");
    const satcurve::Knee k = satcurve::knee_of(curve.data(), budget_ppm, min_requests);
    return py::make_tuple(k.level, k.n, k.b, k.valid);
  });
  m.def("satcurve_state", [](bool recent_known, uint64_t n_total, int64_t min_requests, bool knee_valid, uint32_t recent_level,
                             uint32_t knee_level) {
    return satcurve::state_of(recent_known, n_total, min_requests, knee_valid, recent_level, knee_level);
  });
  m.def("satcurve_age", [](uint32_t state, uint32_t prev_age) { return satcurve::age_of(state, prev_age); });
  // (first, count, lo, hi) of the bins an advance evicts and of those it folds
  m.def("satcurve_fold", [](int64_t prev, int64_t q_hi, int64_t q_first, uint32_t bins) {
    const satcurve::Fold f = satcurve::fold_of(prev, q_hi, q_first, bins);
    return py::make_tuple(f.first, f.count, f.lo, f.hi);
  });
  m.def("satcurve_layout", [](int group_cap) {
    const satcurve::Layout l = satcurve::layout(group_cap);
    py::dict d;
    d["rows"] = l.rows, d["curve"] = l.curve, d["stats"] = l.stats, d["words"] = l.words;
    return d;
  });
  m.def("satcurve_device_bytes", [](int bins, int64_t span_cap, int group_cap) {
    return satcurve::device_bytes(bins, (int)span_cap, group_cap);
  });
  // the two bounds: the population after a list of (q_hi, spans) steps and one more
  m.def("satcurve_ring_after", [](uint32_t bins, const std::vector<std::pair<int64_t, int64_t>>& steps, int64_t q_hi, int64_t n) {
    satcurve::RingPopulation p(bins, INT64_MAX);
    for (const auto& s : steps) p.take(s.first, (size_t)s.second);
    return p.after(q_hi, (size_t)n);
  });
  m.def("satcurve_curve_after", [](int64_t epoch_bins, const std::vector<std::pair<int64_t, int64_t>>& steps, int64_t q_hi,
                                   int64_t n) {
    if (epoch_bins < 1) throw std::invalid_argument("saturation curve: epoch_bins");
    satcurve::CurvePopulation p(epoch_bins, INT64_MAX);
    for (const auto& s : steps) p.take(s.first, (size_t)s.second);
    return p.after(q_hi, (size_t)n);
  });
  PySaturationTracker::def_checkpoint(py::class_<PySaturationTracker>(m, "SaturationTracker")
      .def(py::init<int, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, double, int64_t, int, int, int64_t,
                    int64_t, bool>(),
           py::arg("device") = 0, py::arg("bins") = 1024, py::arg("bin_us") = 500000, py::arg("settle_bins") = 30,
           py::arg("recent_bins") = 30, py::arg("epoch_bins") = 43200, py::arg("budget_ppm") = 10000,
           py::arg("min_requests") = 200, py::arg("slo_ms") = 800.0, py::arg("span_cap") = 16384, py::arg("group_cap") = 64,
           py::arg("n_buffers") = 3, py::arg("ring_records_max") = loadsli::default_ring_records_max(1024, 500000),
           py::arg("curve_records_max") = satcurve::kMaxCurveRecords, py::arg("lds") = true)
      .def("step", &PySaturationTracker::step, py::arg("spans"), py::arg("cut_ns"), py::arg("n_groups"))
      .def("query", &PySaturationTracker::query)
      .def("results", &PySaturationTracker::results)
      .def("block", &PySaturationTracker::block)
      .def("step_ms", &PySaturationTracker::step_ms)
      .def("resident", &PySaturationTracker::resident)
      .def("sync", &PySaturationTracker::sync)
      .def("close", &PySaturationTracker::close));
  m.attr("RETRSLI_K") = retrsli::kK;
  m.attr("RETRSLI_STATS") = (int)retrsli::kStats;
  m.attr("RETRSLI_CELLS") = retrsli::kCells;
  m.attr("RETRSLI_LDS_SLOTS") = retrsli::kLdsSlots;
  m.attr("RETRSLI_UNIT_MAX") = retrsli::kUnitMax;
  m.def("retrsli_units_of_ms", [](float ms) { return retrsli::units_of_ms(ms); });
  m.def("retrsli_budget_units", [](double ms) { return retrsli::budget_units(ms); });
  m.def("retrsli_cell_of", [](bool tb, uint32_t r, uint32_t m_u, uint32_t slo_u, uint32_t budget_u) {
    return retrsli::cell_of(tb, r, m_u, slo_u, budget_u);
  });
  m.def("retrsli_state_of", [](const std::vector<uint32_t>& cells, uint32_t sli, uint32_t min_requests, uint32_t coverage_ppm,
                               uint32_t budget_ppm, uint32_t dominance_ppm) {
    if (cells.size() != (size_t)retrsli::kCells) throw std::invalid_argument("retrieval sli: six cells");
    retrsli::Thresholds th;
    th.min_requests = min_requests;
    th.coverage_ppm = coverage_ppm;
    th.budget_ppm = budget_ppm;
    th.dominance_ppm = dominance_ppm;
    return retrsli::state_of(cells.data(), sli, th);
  });
  m.def("retrsli_age_of", [](uint32_t state, uint32_t prev_state, uint32_t prev_age) {
    return retrsli::age_of(state, prev_state, prev_age);
  });
  m.def("retrsli_layout", [](int group_cap) {
    const retrsli::Layout l = retrsli::layout(group_cap);
    return std::vector<size_t>{l.cells, l.cells_roll, l.sum_r, l.sum_t, l.sum_r_roll, l.sum_t_roll, l.sli, l.sli_roll, l.q_r_win,
                               l.q_r_roll, l.q_m_win, l.q_m_roll, l.state, l.age, l.stats, l.words};
  });
  PyRetrievalSliTracker::def_checkpoint(py::class_<PyRetrievalSliTracker>(m, "RetrievalSliTracker")
      .def(py::init<int, int64_t, int, int, int, double, double, int64_t, int64_t, int64_t, int64_t, bool>(),
           py::arg("device") = 0, py::arg("span_cap") = 16384, py::arg("group_cap") = 64, py::arg("windows") = 150,
           py::arg("n_buffers") = 3, py::arg("slo_ms") = 800.0, py::arg("retrieval_budget_ms") = 200.0,
           py::arg("budget_ppm") = 10000, py::arg("coverage_ppm") = 500000, py::arg("dominance_ppm") = 667000,
           py::arg("min_requests") = 200, py::arg("lds") = true)
      .def("step", &PyRetrievalSliTracker::step, py::arg("spans"), py::arg("n_groups"))
      .def("query", &PyRetrievalSliTracker::query)
      .def("results", &PyRetrievalSliTracker::results)
      .def("block", &PyRetrievalSliTracker::block)
      .def("step_ms", &PyRetrievalSliTracker::step_ms)
      .def("resident", &PyRetrievalSliTracker::resident)
      .def("sync", &PyRetrievalSliTracker::sync)
      .def("close", &PyRetrievalSliTracker::close));
  py::class_<PyEngine>(m, "WindowEngine")
      .def(py::init<int, int, int, int, int, int, int, double, double, int, int, bool, bool, int, float, double, int,
                    int, int, int, int, bool>(),
           py::arg("device") = 0, py::arg("sig_cap") = 1 << 20, py::arg("span_cap") = 16384, py::arg("group_cap") = 64,
           py::arg("user_cap") = 1 << 18, py::arg("n_buffers") = 3, py::arg("max_ahead") = 3,
           py::arg("window_ms") = 2000.0, py::arg("threshold") = 0.7, py::arg("fanout") = 3, py::arg("group_mode") = 1,
           py::arg("use_graphs") = true, py::arg("device_refit") = true, py::arg("n_dom") = 10,
           py::arg("ttft_slo_ms") = 800.0f, py::arg("halo_ms") = 0.0, py::arg("import_cap") = 0,
           py::arg("xchg_cap") = 0, py::arg("shard_rank") = 0, py::arg("shard_world") = 1,
           py::arg("halo_windows") = 3, py::arg("split_rings") = false)
      .def("register_host", &PyEngine::register_host)
      .def("submit", &PyEngine::submit, py::arg("k"), py::arg("kernel"), py::arg("user"), py::arg("spans"),
           py::arg("n_groups"), py::arg("labels") = py::none(), py::arg("bases") = std::vector<int64_t>{},
           py::arg("with_labels") = true, py::arg("learn") = false, py::arg("user_rec") = 64)
      .def("submit_copy", &PyEngine::submit_copy, py::arg("k"), py::arg("kernel"), py::arg("user"), py::arg("spans"),
           py::arg("n_groups"), py::arg("labels") = py::none(), py::arg("bases") = std::vector<int64_t>{},
           py::arg("user_rec") = 64)
      .def("submit_chain", &PyEngine::submit_chain, py::arg("k"), py::arg("n_groups"), py::arg("with_labels") = true,
           py::arg("learn") = false)
      .def("h2d_done", &PyEngine::h2d_done)
      .def("wait_h2d", &PyEngine::wait_h2d)
      .def("query", &PyEngine::query)
      .def("wait", &PyEngine::wait)
      .def("packet", &PyEngine::packet)
      .def("results", &PyEngine::results)
      .def("window_ms", &PyEngine::window_ms)
      .def("copy_ms", [](PyEngine& p, int64_t k) {
        py::gil_scoped_release nogil;
        return p.eng().copy_ms(k);
      })
      .def("set_model_bytes", &PyEngine::set_model_bytes)
      .def("set_app_model", &PyEngine::set_app_model)
      .def("set_p0", &PyEngine::set_p0)
      .def("set_refit", &PyEngine::set_refit, py::arg("alpha") = 2.0, py::arg("prior_pseudo") = 1.0,
           py::arg("inv_temp") = 1.0, py::arg("min_count") = 0.0, py::arg("cap_dom") = -1, py::arg("ceil") = 1.0)
      .def("refit_now", &PyEngine::refit_now)
      .def("set_device_refit", [](PyEngine& p, bool on) { p.eng().set_device_refit(on); })
      .def("score", &PyEngine::score, py::arg("feat"), py::arg("labels") = py::none(), py::arg("app") = py::none())
      .def("set_pods", &PyEngine::set_pods)
      .def("inject_remote", &PyEngine::inject_remote)
      .def("results_all", &PyEngine::results_all)
      .def("set_join_params", &PyEngine::set_join_params)
      .def("init_comm", &PyEngine::init_comm)
      .def("totals", &PyEngine::totals)
      .def("reset_totals", &PyEngine::reset_totals)
      .def("stats_acc", &PyEngine::stats_acc)
      .def("model_bytes", &PyEngine::model_bytes)
      .def("restore", &PyEngine::restore)
      .def("sync", &PyEngine::sync)
      .def("import_state", &PyEngine::import_state)
      .def("sent_block", &PyEngine::sent_block)
      .def("close", &PyEngine::close)
      .def_property_readonly("buffers", &PyEngine::buffers)
      .def_property_readonly("copy_lanes", [](PyEngine& p) { return p.eng().copy_lanes(); })
      .def_property_readonly("copy_ahead", [](PyEngine& p) { return p.eng().copy_ahead(); })
      .def("take_copy_lanes", [](PyEngine& p) {
        py::gil_scoped_release nogil;
        return p.eng().take_copy_lanes();
      })
      .def_property_readonly("windows_folded", &PyEngine::folded)
      .def_property_readonly("graphs", &PyEngine::graphs)
      .def_property_readonly("host_issue_us", &PyEngine::host_issue_us)
      .def_property_readonly("host_wait_us", &PyEngine::host_wait_us)
      .def_property_readonly("host_dma_issue_us", &PyEngine::host_dma_issue_us)
      .def_property_readonly("host_launch_us", &PyEngine::host_launch_us)
      .def_property_readonly("host_pre_us", [](PyEngine& p) { return p.eng().host_pre_us(); })
      .def_property_readonly("host_dma_split_us", [](PyEngine& p) { return p.eng().host_dma_split_us(); })
      .def_property_readonly("host_tail_us", [](PyEngine& p) { return p.eng().host_tail_us(); })
      .def_property_readonly("has_comm", &PyEngine::has_comm)
      .def_property_readonly("rank", [](PyEngine& p) { return p.eng().rank(); })
      .def_property_readonly("world", [](PyEngine& p) { return p.eng().world(); })
      .def_property_readonly("staged_bytes", &PyEngine::staged_bytes)
      .def_property_readonly("direct_bytes", &PyEngine::direct_bytes);
}
