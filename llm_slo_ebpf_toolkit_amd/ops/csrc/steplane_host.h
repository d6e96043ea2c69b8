// Host side of the step lane (steplane.h) that needs no device: what every side tracker's step shares
// before it touches the GPU -- the span ranges of a window and the bookkeeping of the result slots -- and
// the lane's checkpoint image: its digest, its header and the header's checks (namespace lane, below).
// Plain C++ (no HIP header), so it builds and runs on its own under the host sanitizers
// (tests/native/steplane_host_check.cpp). `who` is the tracker's name as its messages spell it
// ("open-request", "ttft sketch", "error sli", ...).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define MISLO_LANE_HD __host__ __device__
#else
#define MISLO_LANE_HD
#endif

namespace mislo {

constexpr int kSpanBytes = 64;  // collector/records.py SPAN

using Range = std::pair<uintptr_t, size_t>;  // (host address, bytes)

// the span records in `ranges`; throws when they are not whole records or exceed span_cap
inline size_t plan_ranges(const std::vector<Range>& ranges, int span_cap, const char* who) {
  const std::string step = std::string(who) + " step: ";
  size_t n = 0;
  for (const Range& r : ranges) {
    if (r.second == 0) continue;
    if (r.first == 0) throw std::invalid_argument(step + "null range");
    if (r.second % kSpanBytes) throw std::invalid_argument(step + "a range is not whole 64-byte spans");
    if (r.second / kSpanBytes > (size_t)span_cap - n) throw std::invalid_argument(step + "more spans than span_cap");
    n += r.second / kSpanBytes;
  }
  return n;
}

// Result slots: step i writes slot i % n; its results stay readable until step i + n takes the slot.
class SlotRing {
 public:
  explicit SlotRing(int n, const char* who = "open-request") : idx_((size_t)(n > 0 ? n : 1), -1), who_(who) {}
  int size() const { return (int)idx_.size(); }
  int64_t next() const { return next_; }
  // the slot of the next step (its index is next()); the step it held before is forgotten
  int begin() {
    const int s = (int)(next_ % (int64_t)idx_.size());
    idx_[(size_t)s] = next_++;
    return s;
  }
  // continue at step `next` (a restored checkpoint): no step before it is held
  void resume(int64_t next) {
    if (next < 0) throw std::invalid_argument(std::string(who_) + ": a step index below 0");
    std::fill(idx_.begin(), idx_.end(), (int64_t)-1);
    next_ = next;
  }
  bool holds(int64_t i) const { return i >= 0 && i < next_ && idx_[(size_t)(i % (int64_t)idx_.size())] == i; }
  int slot_of(int64_t i) const {
    if (!holds(i))
      throw std::out_of_range(std::string(who_) + " step " + std::to_string(i) + " is not held (only the last " +
                              std::to_string(idx_.size()) + ")");
    return (int)(i % (int64_t)idx_.size());
  }

 private:
  std::vector<int64_t> idx_;
  const char* who_;
  int64_t next_ = 0;
};

// `c` once its tracker's validate() has passed it: lets a constructor refuse a configuration in its
// initialiser list, before a member that touches the device is built from it
template <class Config>
const Config& checked(const Config& c) {
  validate(c);
  return c;
}

// ---- the checkpoint image -----------------------------------------------------------------------
// A lane's image is an ImageHeader and then the payload: every array the tracker took with zeroed(), in
// allocation order, each a whole number of 16-byte chunks; the result block is not part of it (every step
// rewrites or clears it whole). docs/TRACKER_CHECKPOINT.md has the rules.
namespace lane {

constexpr uint64_t kMagic = 0x31474d49454e414cull;  // "LANEIMG1", little endian
constexpr uint32_t kVersion = 1;
constexpr int kMaxSegments = 32;  // arrays of one tracker, at most (the pod breakdown takes 19)
constexpr int kMaxFields = 24;    // configuration fields of one fingerprint, at most
constexpr int kHostWords = 8;     // host integers a tracker keeps between steps, at most
constexpr size_t kChunk = 16;

enum Kind : uint32_t {
  kNoKind = 0, kOpenReq = 1, kSliSketch = 2, kExemplars = 3, kPodRank = 4, kOnset = 5, kDecodeSli = 6, kDrift = 7,
  kErrSli = 8, kLoadSli = 9, kSatCurve = 10, kRetrSli = 11, kKinds = 12
};
inline const char* kind_name(uint32_t k) {
  static const char* const names[kKinds] = {"no tracker", "open-request", "ttft sketch", "request exemplars",
                                            "pod breakdown", "breach onset", "decode sli", "ttft drift", "error sli",
                                            "load sli", "saturation curve", "retrieval sli"};
  return k < kKinds ? names[k] : "unknown tracker";
}

constexpr size_t round16(size_t bytes) { return (bytes + (kChunk - 1)) & ~(kChunk - 1); }

// ---- the digest ---------------------------------------------------------------------------------
// splitmix64's finaliser
MISLO_LANE_HD inline uint64_t mix64(uint64_t x) {
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}
constexpr uint64_t kGolden = 0x9e3779b97f4a7c15ull;
// Chunk i of the payload, its two 64-bit halves lo (bytes 0-7) and hi (bytes 8-15): each half is mixed with
// its own position, so a zero chunk counts too and two chunks that change places change the sum.
MISLO_LANE_HD inline uint64_t chunk_digest(uint64_t lo, uint64_t hi, uint64_t i) {
  return mix64(lo + kGolden * (2 * i + 1)) + mix64(hi + kGolden * (2 * i + 2));
}
// The payload's digest: the chunk values summed mod 2^64 -- in any order, so the device's partial sums can
// be merged by atomic adds. Guards against truncation, bit rot and a wrong layout, not against an adversary.
inline uint64_t digest(const void* payload, size_t bytes) {
  const unsigned char* p = static_cast<const unsigned char*>(payload);
  uint64_t sum = 0;
  for (size_t i = 0; i < bytes / kChunk; ++i) {
    uint64_t h[2];
    std::memcpy(h, p + i * kChunk, kChunk);
    sum += chunk_digest(h[0], h[1], (uint64_t)i);
  }
  return sum;
}

// ---- the fingerprint ----------------------------------------------------------------------------
// Every Config field that shapes a tracker's state or its meaning, by name (each tracker's *_host.h
// fingerprint()); device, n_buffers, span_cap and lds are not among them.
struct Field {
  const char* name;
  int64_t value;
  bool real;  // `value` holds a double's bits
};
inline Field field(const char* name, int64_t v) { return Field{name, v, false}; }
inline Field real_field(const char* name, double v) {
  int64_t b;
  std::memcpy(&b, &v, sizeof(b));
  return Field{name, b, true};
}
struct Fingerprint {
  uint32_t kind = kNoKind;
  std::vector<Field> fields;
  uint64_t hash() const {
    uint64_t h = mix64(kGolden ^ (uint64_t)kind);
    for (size_t i = 0; i < fields.size(); ++i) h = mix64(h ^ mix64((uint64_t)fields[i].value + kGolden * (uint64_t)(i + 1)));
    return h;
  }
};

struct ImageHeader {
  uint64_t magic;
  uint32_t version, kind;
  uint64_t fingerprint;
  int64_t step;  // the index of the next step
  uint32_t n_segments, n_fields, n_host, pad;
  uint64_t seg_bytes[kMaxSegments];
  int64_t fields[kMaxFields];  // the fingerprint's values, so that a refusal can name what differs
  int64_t host[kHostWords];
  uint64_t payload_bytes;
  uint64_t digest;
};
static_assert(sizeof(ImageHeader) == 576 && sizeof(ImageHeader) % kChunk == 0, "an image header is 36 chunks");

inline std::string show(const Field& f, int64_t v) {
  char b[48];
  if (f.real) {
    double d;
    std::memcpy(&d, &v, sizeof(d));
    std::snprintf(b, sizeof(b), "%g", d);
  } else {
    std::snprintf(b, sizeof(b), "%lld", (long long)v);
  }
  return b;
}

// The header a lane of `fp` with arrays of `seg_bytes` writes; step, host words and digest are the snapshot's.
inline ImageHeader make_header(const Fingerprint& fp, const std::vector<size_t>& seg_bytes) {
  if (seg_bytes.size() > (size_t)kMaxSegments) throw std::logic_error("step lane: more arrays than an image header holds");
  if (fp.fields.size() > (size_t)kMaxFields) throw std::logic_error("step lane: more fields than an image header holds");
  static_assert(kHostWords == 8, "ImageHeader::host");
  ImageHeader h;
  std::memset(&h, 0, sizeof(h));
  h.magic = kMagic;
  h.version = kVersion;
  h.kind = fp.kind;
  h.fingerprint = fp.hash();
  h.n_segments = (uint32_t)seg_bytes.size();
  h.n_fields = (uint32_t)fp.fields.size();
  for (size_t i = 0; i < seg_bytes.size(); ++i) h.seg_bytes[i] = seg_bytes[i], h.payload_bytes += seg_bytes[i];
  for (size_t i = 0; i < fp.fields.size(); ++i) h.fields[i] = fp.fields[i].value;
  return h;
}

// Whether `image` of `bytes` is an image this lane (`fp`, `mine` from make_header) can take: throws
// std::invalid_argument naming what differs. Reads nothing past `bytes`; touches no device.
inline ImageHeader check_image(const void* image, size_t bytes, const Fingerprint& fp, const ImageHeader& mine) {
  const std::string who = std::string(kind_name(fp.kind)) + " image: ";
  if (image == nullptr || bytes < sizeof(ImageHeader))
    throw std::invalid_argument(who + std::to_string(bytes) + " bytes are shorter than a header");
  ImageHeader h;
  std::memcpy(&h, image, sizeof(h));
  if (h.magic != kMagic) throw std::invalid_argument(who + "bad magic");
  if (h.version != kVersion)
    throw std::invalid_argument(who + "format version " + std::to_string(h.version) + ", this build reads " + std::to_string(kVersion));
  if (h.kind != fp.kind)
    throw std::invalid_argument(who + "kind " + kind_name(h.kind) + ", this tracker " + kind_name(fp.kind));
  if (h.n_fields != mine.n_fields)
    throw std::invalid_argument(who + "fields " + std::to_string(h.n_fields) + ", this tracker " + std::to_string(mine.n_fields));
  for (uint32_t i = 0; i < mine.n_fields; ++i)
    if (h.fields[i] != mine.fields[i])
      throw std::invalid_argument(who + fp.fields[i].name + " " + show(fp.fields[i], h.fields[i]) + ", this tracker " +
                                  show(fp.fields[i], mine.fields[i]));
  if (h.fingerprint != mine.fingerprint) throw std::invalid_argument(who + "fingerprint differs from this tracker's");
  if (h.n_segments != mine.n_segments)
    throw std::invalid_argument(who + "arrays " + std::to_string(h.n_segments) + ", this tracker " + std::to_string(mine.n_segments));
  for (uint32_t i = 0; i < mine.n_segments; ++i)
    if (h.seg_bytes[i] != mine.seg_bytes[i])
      throw std::invalid_argument(who + "array " + std::to_string(i) + " of " + std::to_string(h.seg_bytes[i]) +
                                  " bytes, this tracker " + std::to_string(mine.seg_bytes[i]));
  if (h.payload_bytes != mine.payload_bytes)
    throw std::invalid_argument(who + "payload of " + std::to_string(h.payload_bytes) + " bytes, this tracker " +
                                std::to_string(mine.payload_bytes));
  if (bytes != sizeof(ImageHeader) + (size_t)mine.payload_bytes)
    throw std::invalid_argument(who + std::to_string(bytes) + " bytes, header and payload are " +
                                std::to_string(sizeof(ImageHeader) + (size_t)mine.payload_bytes));
  if (h.n_host != mine.n_host)
    throw std::invalid_argument(who + "host words " + std::to_string(h.n_host) + ", this tracker " + std::to_string(mine.n_host));
  if (h.step < 0) throw std::invalid_argument(who + "a step index below 0");
  return h;
}

}  // namespace lane

}  // namespace mislo
