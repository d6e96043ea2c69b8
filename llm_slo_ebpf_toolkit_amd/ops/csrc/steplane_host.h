// Host side of the step lane (steplane.h) that needs no device: what every side tracker's step shares
// before it touches the GPU -- the span ranges of a window and the bookkeeping of the result slots.
// Plain C++ (no HIP header), so it builds and runs on its own under the host sanitizers
// (tests/native/steplane_host_check.cpp). `who` is the tracker's name as its messages spell it
// ("open-request", "ttft sketch", "error sli", ...).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

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

}  // namespace mislo
