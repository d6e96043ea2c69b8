// The window engine's copy schedule alone on one MI355X: per window three H2D DMAs (BPF ring
// bytes, user records, spans) from shared-memory mappings page-locked with hipHostRegister, at
// bench.py's per-window sizes and with moving source offsets (a range that wraps is two DMAs,
// as the rings hand them over), into one of three device input blocks. No kernels at all: a
// second stream only stands in for the front stage's dependency (it waits for a window's
// completion event). The host keeps at most three windows queued, as the engine does.
//
// Variants, 200 windows after 20 warm-ups each:
//   a  one stream, 2 event waits + start record, 3 DMAs, 3 end records (the engine before copy lanes)
//   b  one stream, start record, 3 DMAs, 1 completion record
//   c  pattern b on two streams, windows alternating
//   d  pattern b, user records and spans on a second stream (the former MISLO_COPY_STREAMS=2)
//   e  pattern c, a window's lane starting once the previous window's ring DMA has ended
// Prints per variant the period per window (device events across the run), GB/s, the median
// span of one window's DMAs (its latency: with two lanes windows share the link), and the host
// time inside hipMemcpyAsync per DMA kind (median / max): whether a second stream blocks the
// issuing thread.
//
// Build: hipcc --offload-arch=gfx950 -O2 tools/native/window_dma.hip -o build/window_dma -lrt
// The whole run is under a time limit (alarm); any failed HIP call exits non-zero at once.
#include <hip/hip_runtime.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define CK(x)                                                                              \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess) {                                                                \
      std::fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
      std::exit(1);                                                                        \
    }                                                                                      \
  } while (0)

namespace {

constexpr int kNb = 3, kWarm = 20, kWindows = 200, kKinds = 3;
// bench.py's window: 18.63 B per event of kernel ring, USER16 records, 64-byte spans
constexpr size_t kBytes[kKinds] = {15700000 / 136 * 136, 3300000 / 16 * 16, 1000000 / 64 * 64};
const char* const kKind[kKinds] = {"ring", "user", "spans"};

struct Ring {  // a page-locked shm mapping read at a moving offset
  std::string name;
  uint8_t* base = nullptr;
  size_t cap = 0, pos = 0;
};

Ring make_ring(const char* tag, size_t window_bytes) {
  Ring r;
  r.name = std::string("/mislo-window-dma-") + tag + "-" + std::to_string((long)getpid());
  r.cap = ((window_bytes * 7 / 2) + 4095) & ~size_t(4095);  // 3.5 windows: every fourth range wraps
  shm_unlink(r.name.c_str());
  const int fd = shm_open(r.name.c_str(), O_CREAT | O_RDWR, 0600);
  if (fd < 0 || ftruncate(fd, (off_t)r.cap) != 0) {
    std::perror("shm");
    std::exit(1);
  }
  void* p = mmap(nullptr, r.cap, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
  close(fd);
  shm_unlink(r.name.c_str());  // the mapping keeps it
  if (p == MAP_FAILED) {
    std::perror("mmap");
    std::exit(1);
  }
  std::memset(p, 0x5a, r.cap);
  CK(hipHostRegister(p, r.cap, hipHostRegisterDefault));
  r.base = static_cast<uint8_t*>(p);
  return r;
}

struct Timer {
  std::vector<double> us[kKinds];
};

// one kind's DMA(s) of a window: [pos, pos + n) of the ring, two copies where it wraps
void dma(Ring& r, uint8_t* dst, size_t n, hipStream_t st, std::vector<double>* us) {
  size_t idx = r.pos % r.cap, left = n, off = 0;
  while (left) {
    const size_t take = std::min(left, r.cap - idx);
    const auto t0 = std::chrono::steady_clock::now();
    CK(hipMemcpyAsync(dst + off, r.base + idx, take, hipMemcpyHostToDevice, st));
    if (us) us->push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    off += take;
    left -= take;
    idx = 0;
  }
  r.pos += n;
}

struct Buf {
  uint8_t* in[kKinds];
  hipEvent_t t_start, part, done, t_end, comp;
};

void run(char variant, Ring* rings, Buf* bufs, hipStream_t* copy, hipStream_t front) {
  Timer tm;
  hipEvent_t first, last[2];
  CK(hipEventCreate(&first));
  for (auto& e : last) CK(hipEventCreate(&e));
  const int lanes = variant == 'c' || variant == 'e' ? 2 : 1;
  std::vector<double> span_us;  // a window's start marker to its completion event (d: the ring DMA's stream)
  auto span = [&](Buf& b) {
    float m = 0.f;
    CK(hipEventElapsedTime(&m, b.t_start, b.done));
    span_us.push_back(1e3 * m);
  };
  for (int w = 0; w < kWarm + kWindows; ++w) {
    Buf& b = bufs[w % kNb];
    if (w >= kNb) {
      CK(hipEventSynchronize(b.comp));  // the buffer's previous window is through
      if (w - kNb >= kWarm) span(b);
    }
    const bool timed = w >= kWarm;
    hipStream_t s0 = copy[lanes == 2 ? (w & 1) : 0];
    hipStream_t s1 = variant == 'd' ? copy[1] : s0;  // user records and spans
    if (variant == 'a') {
      CK(hipStreamWaitEvent(s0, b.comp, 0));
      CK(hipStreamWaitEvent(s1, b.comp, 0));
    }
    // e: this lane starts once the previous window's ring DMA (on the other lane) has ended, so
    // this window fills the link while that one hands over between its DMAs and at its end
    if (variant == 'e' && w >= 1) CK(hipStreamWaitEvent(s0, bufs[(w - 1) % kNb].part, 0));
    if (w == kWarm) CK(hipEventRecord(first, s0));
    CK(hipEventRecord(b.t_start, s0));
    dma(rings[0], b.in[0], kBytes[0], s0, timed ? &tm.us[0] : nullptr);
    if (variant == 'e') CK(hipEventRecord(b.part, s0));
    dma(rings[1], b.in[1], kBytes[1], s1, timed ? &tm.us[1] : nullptr);
    dma(rings[2], b.in[2], kBytes[2], s1, timed ? &tm.us[2] : nullptr);
    if (variant == 'a' || variant == 'd') CK(hipEventRecord(b.part, s1));
    CK(hipEventRecord(b.done, s0));
    if (variant == 'a') CK(hipEventRecord(b.t_end, s1));
    if (w >= kWarm + kWindows - 2) CK(hipEventRecord(last[w & 1], s0));  // the end of each lane's last window
    // the front stage's stand-in: waits for the window's copy, then frees the buffer
    CK(hipStreamWaitEvent(front, b.done, 0));
    if (variant == 'a' || variant == 'd') CK(hipStreamWaitEvent(front, b.part, 0));
    CK(hipEventRecord(b.comp, front));
  }
  for (int i = 0; i < 2; ++i) CK(hipStreamSynchronize(copy[i]));
  CK(hipStreamSynchronize(front));
  for (int w = kWarm + kWindows - kNb; w < kWarm + kWindows; ++w) span(bufs[w % kNb]);
  std::sort(span_us.begin(), span_us.end());
  float ms = 0.f;
  for (auto& e : last) {
    float m = 0.f;
    CK(hipEventElapsedTime(&m, first, e));
    ms = std::max(ms, m);
  }
  if (variant == 'd') {  // the second stream's tail: the last window's user / span DMAs
    float m = 0.f;
    CK(hipEventElapsedTime(&m, first, bufs[(kWarm + kWindows - 1) % kNb].part));
    ms = std::max(ms, m);
  }
  const double period = ms / kWindows;
  const double bytes = (double)(kBytes[0] + kBytes[1] + kBytes[2]);
  std::printf("variant %c  period %.4f ms/window  %.1f GB/s  window span %.0f us  hipMemcpyAsync host us (median/max):",
              variant, period, bytes / (period * 1e-3) / 1e9, span_us[span_us.size() / 2]);
  for (int k = 0; k < kKinds; ++k) {
    std::vector<double>& v = tm.us[k];
    std::sort(v.begin(), v.end());
    std::printf("  %s %.1f/%.1f", kKind[k], v[v.size() / 2], v.back());
  }
  std::printf("\n");
  std::fflush(stdout);
  CK(hipEventDestroy(first));
  for (auto& e : last) CK(hipEventDestroy(e));
}

}  // namespace

int main(int argc, char** argv) {
  alarm(120);  // the whole run: SIGALRM ends the process
  CK(hipSetDevice(0));
  Ring rings[kKinds] = {make_ring("k", kBytes[0]), make_ring("u", kBytes[1]), make_ring("s", kBytes[2])};
  hipStream_t copy[2], front;
  for (auto& s : copy) CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  CK(hipStreamCreateWithFlags(&front, hipStreamNonBlocking));
  Buf bufs[kNb];
  for (Buf& b : bufs) {
    for (int k = 0; k < kKinds; ++k) CK(hipMalloc(reinterpret_cast<void**>(&b.in[k]), kBytes[k]));
    for (hipEvent_t* e : {&b.t_start, &b.part, &b.done, &b.t_end}) CK(hipEventCreate(e));
    CK(hipEventCreateWithFlags(&b.comp, hipEventDisableTiming | hipEventBlockingSync));
  }
  std::printf("window: ring %zu + user %zu + spans %zu = %zu bytes, %d windows after %d warm-ups\n", kBytes[0], kBytes[1],
              kBytes[2], kBytes[0] + kBytes[1] + kBytes[2], kWindows, kWarm);
  const char* which = argc > 1 ? argv[1] : "abcde";
  for (const char* v = which; *v; ++v) {
    if (!std::strchr("abcde", *v)) {
      std::fprintf(stderr, "unknown variant %c\n", *v);
      return 2;
    }
    run(*v, rings, bufs, copy, front);
  }
  for (Buf& b : bufs) {
    for (int k = 0; k < kKinds; ++k) CK(hipFree(b.in[k]));
    for (hipEvent_t e : {b.t_start, b.part, b.done, b.t_end, b.comp}) CK(hipEventDestroy(e));
  }
  for (auto& s : copy) CK(hipStreamDestroy(s));
  CK(hipStreamDestroy(front));
  for (Ring& r : rings) {
    CK(hipHostUnregister(r.base));
    munmap(r.base, r.cap);
  }
  return 0;
}
