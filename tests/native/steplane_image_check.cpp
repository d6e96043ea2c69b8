// The step lane's checkpoint image on the host (ops/csrc/steplane_host.h namespace lane: the digest, the
// header and its checks, every tracker's fingerprint) and SlotRing::resume, on their own for the host
// sanitizers: tests/test_steplane_image.py builds this with -fsanitize=address,undefined and runs it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "decodesli_host.h"
#include "drift_host.h"
#include "errsli_host.h"
#include "exemplars_host.h"
#include "loadsli_host.h"
#include "onset_host.h"
#include "openreq_host.h"
#include "podrank_host.h"
#include "retrsli_host.h"
#include "satcurve_host.h"
#include "slisketch_host.h"
#include "steplane_host.h"

using namespace mislo;

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      std::fprintf(stderr, "check failed at line %d: %s\n", __LINE__, #x); \
      std::exit(1);                                                    \
    }                                                                  \
  } while (0)

// the message of the E that f throws; "<none>" when it throws nothing (another type escapes)
template <class E, class F>
std::string message(F f) {
  try {
    f();
  } catch (const E& e) {
    return e.what();
  }
  return "<none>";
}

static bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

// ---- the digest -----------------------------------------------------------------------------------
// Worked out by hand (Python integers, the definition in steplane_host.h written down again):
//   mix64(x): x ^= x >> 30; x *= 0xbf58476d1ce4e5b9; x ^= x >> 27; x *= 0x94d049bb133111eb; x ^= x >> 31
//   G = 0x9e3779b97f4a7c15; chunk i with halves lo, hi counts mix64(lo + G (2i + 1)) + mix64(hi + G (2i + 2))
//   mix64(G) = 0xe220a8397b1dcdaf (splitmix64's first output for seed 0), mix64(2G) = 0x6e789e6aa1b965f4,
//   mix64(3G) = 0x06c45d188009454f, mix64(4G) = 0xf88bb8a8724c81ec
//   a zero chunk 0: mix64(G) + mix64(2G)   = 0x509946a41cd733a3
//   a zero chunk 1: mix64(3G) + mix64(4G)  = 0xff5015c0f255c73b
//   the bytes 00 01 .. 0f (lo = 0x0706050403020100, hi = 0x0f0e0d0c0b0a0908): as chunk 0 0x32b9034c9765933f,
//   as chunk 1 0xc3dfc1c04bf3e61a
static void digest_checks() {
  CHECK(lane::mix64(lane::kGolden) == 0xe220a8397b1dcdafull);
  CHECK(lane::mix64(2 * lane::kGolden) == 0x6e789e6aa1b965f4ull);
  CHECK(lane::mix64(3 * lane::kGolden) == 0x06c45d188009454full);
  CHECK(lane::mix64(4 * lane::kGolden) == 0xf88bb8a8724c81ecull);
  CHECK(lane::chunk_digest(0, 0, 0) == 0x509946a41cd733a3ull);
  CHECK(lane::chunk_digest(0, 0, 1) == 0xff5015c0f255c73bull);
  CHECK(lane::chunk_digest(0x0706050403020100ull, 0x0f0e0d0c0b0a0908ull, 0) == 0x32b9034c9765933full);
  CHECK(lane::chunk_digest(0x0706050403020100ull, 0x0f0e0d0c0b0a0908ull, 1) == 0xc3dfc1c04bf3e61aull);

  unsigned char zeros[32] = {0}, ramp[16];
  for (int i = 0; i < 16; ++i) ramp[i] = (unsigned char)i;
  CHECK(lane::digest(zeros, 0) == 0ull);
  CHECK(lane::digest(zeros, 16) == 0x509946a41cd733a3ull);
  CHECK(lane::digest(zeros, 32) == 0x4fe95c650f2cfadeull);  // the two sums above, mod 2^64
  CHECK(lane::digest(ramp, 16) == 0x32b9034c9765933full);
  unsigned char two[32];
  std::memcpy(two, zeros, 16), std::memcpy(two + 16, ramp, 16);
  CHECK(lane::digest(two, 32) == 0x1479086468cb19bdull);  // zero chunk 0 + the ramp as chunk 1
  std::memcpy(two, ramp, 16), std::memcpy(two + 16, zeros, 16);
  CHECK(lane::digest(two, 32) == 0x3209190d89bb5a7aull);  // the ramp as chunk 0 + zero chunk 1: places count
  // truncation by one chunk and one flipped bit change it
  CHECK(lane::digest(two, 16) != lane::digest(two, 32));
  two[21] ^= 0x10;
  CHECK(lane::digest(two, 32) != 0x3209190d89bb5a7aull);

  // the sum does not depend on the order the chunks are visited in: every permutation of 5 chunks, and a
  // split into partial sums the way wave and workgroup sums are merged
  std::vector<unsigned char> p(5 * 16);
  for (size_t i = 0; i < p.size(); ++i) p[i] = (unsigned char)(i * 37 + 11);
  const uint64_t whole = lane::digest(p.data(), p.size());
  std::vector<int> order(5);
  std::iota(order.begin(), order.end(), 0);
  int perms = 0;
  do {
    uint64_t sum = 0, part[2] = {0, 0};
    for (int k = 0; k < 5; ++k) {
      uint64_t h[2];
      std::memcpy(h, p.data() + (size_t)order[(size_t)k] * 16, 16);
      const uint64_t v = lane::chunk_digest(h[0], h[1], (uint64_t)order[(size_t)k]);
      sum += v;
      part[k & 1] += v;
    }
    CHECK(sum == whole && part[0] + part[1] == whole);
    ++perms;
  } while (std::next_permutation(order.begin(), order.end()));
  CHECK(perms == 120);
}

// ---- the header -----------------------------------------------------------------------------------
static std::vector<unsigned char> image_of(const lane::ImageHeader& h, size_t payload) {
  std::vector<unsigned char> img(sizeof(h) + payload, 0);
  std::memcpy(img.data(), &h, sizeof(h));
  return img;
}

static void header_checks() {
  errsli::Config c;
  c.windows = 300, c.pairs = {{300, 30, 14400}};
  const lane::Fingerprint fp = errsli::fingerprint(c);
  const std::vector<size_t> segs = {lane::round16(8), lane::round16(100), 4096};  // 16 + 112 + 4096
  CHECK(lane::round16(0) == 0 && lane::round16(1) == 16 && lane::round16(16) == 16 && lane::round16(17) == 32);
  lane::ImageHeader mine = lane::make_header(fp, segs);
  mine.n_host = 2;
  CHECK(mine.payload_bytes == 4224 && mine.n_segments == 3 && mine.kind == lane::kErrSli);
  lane::ImageHeader h = mine;
  h.step = 7, h.host[0] = 41, h.host[1] = -1, h.digest = 99;
  std::vector<unsigned char> img = image_of(h, 4224);
  const lane::ImageHeader got = lane::check_image(img.data(), img.size(), fp, mine);
  CHECK(got.step == 7 && got.host[0] == 41 && got.host[1] == -1 && got.digest == 99 && got.n_host == 2);

  auto refused = [&](const std::vector<unsigned char>& im, size_t bytes) {
    return message<std::invalid_argument>([&] { lane::check_image(im.data(), bytes, fp, mine); });
  };
  // a short buffer: nothing of it is read (the vector holds just those bytes, for the sanitizer)
  for (size_t n : {size_t(0), size_t(1), sizeof(lane::ImageHeader) - 1}) {
    std::vector<unsigned char> cut(img.begin(), img.begin() + (long)n);
    CHECK(has(refused(cut, n), "shorter than a header"));
  }
  CHECK(has(message<std::invalid_argument>([&] { lane::check_image(nullptr, 4096, fp, mine); }), "shorter than a header"));
  {  // truncated by one chunk, and one chunk too long
    std::vector<unsigned char> cut(img.begin(), img.end() - 16);
    CHECK(has(refused(cut, cut.size()), "header and payload are 4800"));
    std::vector<unsigned char> more = img;
    more.resize(img.size() + 16);
    CHECK(has(refused(more, more.size()), "header and payload are 4800"));
  }
  auto with = [&](auto change) {
    lane::ImageHeader x = h;
    change(x);
    return refused(image_of(x, 4224), sizeof(x) + 4224);
  };
  CHECK(has(with([](lane::ImageHeader& x) { x.magic ^= 1; }), "bad magic"));
  CHECK(has(with([](lane::ImageHeader& x) { x.version = 2; }), "format version 2, this build reads 1"));
  CHECK(with([](lane::ImageHeader& x) { x.kind = lane::kDrift; }) == "error sli image: kind ttft drift, this tracker error sli");
  CHECK(has(with([](lane::ImageHeader& x) { x.kind = 77; }), "kind unknown tracker"));
  CHECK(has(with([](lane::ImageHeader& x) { x.n_segments = 2; }), "arrays 2, this tracker 3"));
  CHECK(has(with([](lane::ImageHeader& x) { x.n_segments = 0xffffffffu; }), "arrays 4294967295, this tracker 3"));
  CHECK(has(with([](lane::ImageHeader& x) { x.seg_bytes[1] = 128; }), "array 1 of 128 bytes, this tracker 112"));
  CHECK(has(with([](lane::ImageHeader& x) { x.payload_bytes = 4240; }), "payload of 4240 bytes, this tracker 4224"));
  CHECK(has(with([](lane::ImageHeader& x) { x.n_host = 3; }), "host words 3, this tracker 2"));
  CHECK(has(with([](lane::ImageHeader& x) { x.n_fields = 0xffffffffu; }), "fields 4294967295"));
  CHECK(has(with([](lane::ImageHeader& x) { x.step = -1; }), "a step index below 0"));
  CHECK(has(with([](lane::ImageHeader& x) { x.fingerprint ^= 1; }), "fingerprint differs"));

  // another configuration is refused by the field's name
  errsli::Config d = c;
  d.windows = 150, d.pairs = {{150, 30, 14400}};
  const lane::Fingerprint fpd = errsli::fingerprint(d);
  const lane::ImageHeader other = lane::make_header(fpd, segs);
  CHECK(other.fingerprint != mine.fingerprint);
  lane::ImageHeader o2 = other;
  o2.n_host = 2;
  CHECK(refused(image_of(o2, 4224), sizeof(o2) + 4224) == "error sli image: windows 150, this tracker 300");
  d = c;
  d.target = 0.99;
  o2 = lane::make_header(errsli::fingerprint(d), segs);
  CHECK(refused(image_of(o2, 4224), sizeof(o2) + 4224) == "error sli image: target 0.99, this tracker 0.999");
  d = c;
  d.group_cap = 32;
  o2 = lane::make_header(errsli::fingerprint(d), segs);
  CHECK(refused(image_of(o2, 4224), sizeof(o2) + 4224) == "error sli image: group_cap 32, this tracker 64");

  // too many arrays or fields for a header are the lane's own mistake
  CHECK(has(message<std::logic_error>([&] { lane::make_header(fp, std::vector<size_t>(lane::kMaxSegments + 1, 16)); }),
            "more arrays"));
}

// every tracker's fingerprint: its kind, what it leaves out (device, n_buffers, span_cap, lds) and that it
// fits a header
template <class Config, class F>
static void fingerprint_of(uint32_t kind, F fingerprint) {
  Config a, b;
  b.device = 3, b.n_buffers = 7, b.span_cap = 99;
  const lane::Fingerprint fa = fingerprint(a), fb = fingerprint(b);
  CHECK(fa.kind == kind && fa.hash() == fb.hash() && fa.fields.size() <= (size_t)lane::kMaxFields && !fa.fields.empty());
  Config g;
  g.group_cap = a.group_cap / 2;
  CHECK(fingerprint(g).hash() != fa.hash());
  CHECK(std::string(fa.fields[0].name) == "group_cap" || std::string(fa.fields[1].name) == "group_cap");
}

static void fingerprint_checks() {
  fingerprint_of<openreq::Config>(lane::kOpenReq, openreq::fingerprint);
  fingerprint_of<slisketch::Config>(lane::kSliSketch, slisketch::fingerprint);
  fingerprint_of<exemplars::Config>(lane::kExemplars, exemplars::fingerprint);
  fingerprint_of<podrank::Config>(lane::kPodRank, podrank::fingerprint);
  fingerprint_of<onset::Config>(lane::kOnset, onset::fingerprint);
  fingerprint_of<decodesli::Config>(lane::kDecodeSli, decodesli::fingerprint);
  fingerprint_of<drift::Config>(lane::kDrift, drift::fingerprint);
  fingerprint_of<errsli::Config>(lane::kErrSli, errsli::fingerprint);
  fingerprint_of<loadsli::Config>(lane::kLoadSli, loadsli::fingerprint);
  fingerprint_of<satcurve::Config>(lane::kSatCurve, satcurve::fingerprint);
  fingerprint_of<retrsli::Config>(lane::kRetrSli, retrsli::fingerprint);
  // lds is left out where a tracker has it; slo_ms is covered
  decodesli::Config a, b;
  b.lds = !a.lds;
  CHECK(decodesli::fingerprint(a).hash() == decodesli::fingerprint(b).hash());
  b.slo_ms = 900.0;
  CHECK(decodesli::fingerprint(a).hash() != decodesli::fingerprint(b).hash());
  // the same fields under another kind are another fingerprint
  lane::Fingerprint x = slisketch::fingerprint(slisketch::Config()), y = x;
  y.kind = lane::kExemplars;
  CHECK(x.hash() != y.hash());
}

// ---- SlotRing::resume -------------------------------------------------------------------------------
static void resume_checks() {
  SlotRing r(3, "error sli");
  r.resume(7);
  CHECK(r.next() == 7);
  for (int64_t i = -1; i <= 8; ++i) CHECK(!r.holds(i));  // nothing below the resumed index is held, nor it yet
  CHECK(has(message<std::out_of_range>([&] { r.slot_of(6); }), "error sli step 6 is not held (only the last 3)"));
  CHECK(r.begin() == 7 % 3 && r.holds(7) && !r.holds(6) && !r.holds(4) && r.slot_of(7) == 1);
  CHECK(r.begin() == 8 % 3 && r.begin() == 9 % 3 && r.holds(7) && r.holds(8) && r.holds(9));
  CHECK(r.begin() == 10 % 3 && !r.holds(7) && r.holds(10) && r.slot_of(10) == 1 && r.next() == 11);
  // a ring that has stepped forgets what it held
  SlotRing s(2, "load sli");
  s.begin(), s.begin();
  CHECK(s.holds(0) && s.holds(1));
  s.resume(1000000000000ll);
  CHECK(!s.holds(0) && !s.holds(1) && s.begin() == 0 && s.holds(1000000000000ll));
  s.resume(0);
  CHECK(s.next() == 0 && !s.holds(0) && s.begin() == 0 && s.holds(0));
  CHECK(has(message<std::invalid_argument>([&] { s.resume(-1); }), "below 0"));
}

int main() {
  digest_checks();
  header_checks();
  fingerprint_checks();
  resume_checks();
  std::printf("steplane image ok\n");
  return 0;
}
