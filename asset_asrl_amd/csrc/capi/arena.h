// One allocation carved into arrays, with a size that cannot disagree with the carving: take() is the ONLY place an array's
// length is written, total() is the sum of what was taken, and bind() gives every array its place in the allocation.  Pure
// arithmetic on sizes and pointers -- no HIP call, no allocation of its own -- so that it can be tested without a device
// (tests/test_arena_cpu.py), like capi/propagate_plan.h and capi/kkt_map.h.
//
// Slots lie in the order they were taken, without padding: slot k starts at the sum of the counts before it.  A count of 0 is
// legal: the slot starts where the next one does and is never dereferenced.  An array a call does without is taken with a null
// destination (its pointer stays as the caller set it, nullptr for the kernels) and with the count 0.
#pragma once
#include <cstddef>
#include <vector>

namespace asset_hip {

template <class T>
class Arena {
 public:
  // `count` elements behind those taken so far; returns their offset.  *dest (where given) is set by bind().
  std::size_t take(T** dest, std::size_t count) {
    const std::size_t offset = total_;
    if (count > (std::size_t(-1) / sizeof(T) - total_)) overflow_ = true, count = 0;   // (total() * sizeof(T) stays a size_t)
    slots_.push_back(Slot{dest, offset});
    total_ += count;
    return offset;
  }
  std::size_t take(const T** dest, std::size_t count) { return take(const_cast<T**>(dest), count); }
  std::size_t take(std::size_t count) { return take(static_cast<T**>(nullptr), count); }

  std::size_t total() const { return total_; }
  bool overflowed() const { return overflow_; }   // a sum that left size_t: the caller refuses instead of allocating
  // every destination = base + its offset (base: an allocation of total() elements)
  void bind(T* base) const {
    for (const Slot& s : slots_)
      if (s.dest) *s.dest = base + s.offset;
  }

 private:
  struct Slot { T** dest; std::size_t offset; };
  std::vector<Slot> slots_;
  std::size_t total_ = 0;
  bool overflow_ = false;
};

}  // namespace asset_hip
