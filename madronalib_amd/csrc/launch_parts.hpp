// launch_parts.hpp — the HOST bookkeeping of a bank launch that goes out in two parts ("Launch parts"): where a
// bank's voices are cut, and what the engine remembers of the part that runs on its side stream until the two streams meet again.
// Plain C++ that never touches a device: built and tested without any HIP header; capi.hip is the caller.
//
// A plain launch of a bank's V voices may go out as two kernels, voices [0, v0) on the engine's stream and [v0, V) on a side stream.
// Consecutive launches of the bank depend on each other only through each voice's own state, so each part is serial on its own
// stream and the parts need not meet while the host keeps making such launches of the same bank. The engine JOINS the streams
// lazily: before anything else it enqueues. What decides "anything else" is here.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mlparts
{
// chain_kernel deals its workgroups to the XCDs in whole rounds of 8 (mldsp_kernels.hpp: remapped_block); a part whose workgroup
// count is a multiple of 8 keeps that remap whole. 8 workgroups of 256 lanes:
constexpr size_t kSplitUnit = 8 * 256;
constexpr size_t kMaxPendingOutputs = 8;

// mlgpu_engine_set_launch_parts
enum Mode
{
  kAuto = 0,   // two parts when each still puts a workgroup on every CU
  kNever = 1,  // one launch, always
  kHalves = 2  // two parts whenever there is a second part to make (tests)
};

// Where a launch of V voices is cut: v0, a multiple of kSplitUnit with 0 < v0 < V, or 0 for "one launch".
// The first part is the whole units of V / 2 (at least one), the second part the rest, ragged or not.
size_t splitPoint(size_t V, int mode, size_t cuCount, size_t lanesPerWorkgroup);

// An output signal a pending launch writes: [base, base + bytes) in some layout over T DSPVectors. Two launches of the same bank
// with the same base, layout and T write, part by part, exactly the same addresses.
struct Output
{
  uintptr_t base;
  size_t bytes;
  int layout;
  size_t T;
};

inline bool sameOutput(const Output& a, const Output& b) { return a.base == b.base && a.bytes == b.bytes && a.layout == b.layout && a.T == b.T; }
inline bool disjoint(const Output& a, const Output& b)  // (no sum of an address and a size: nothing wraps)
{
  return a.base >= b.base ? a.base - b.base >= b.bytes : b.base - a.base >= a.bytes;
}

// What is in flight on the side stream since the streams last met: parts of `owner`'s launches, into `outputs`.
class Pending
{
 public:
  bool any() const { return owner_ != nullptr; }
  const void* owner() const { return owner_; }
  size_t outputs() const { return n_; }

  // May a two-part launch of `owner` into `out` go out with no join before it? Only if it is the pending owner's and `out` is
  // one of the pending outputs exactly (each part then follows, on its own stream, the part that wrote those addresses before)
  // or lies apart from all of them, with room left to remember it. Nothing pending admits nothing: there is a fork to make.
  bool admits(const void* owner, const Output& out) const;

  // a two-part launch of `owner` into `out` has gone out (after admits(), or after a join and a fork)
  void launched(const void* owner, const Output& out);

  // the streams have met
  void joined()
  {
    owner_ = nullptr;
    n_ = 0;
  }

 private:
  const void* owner_{nullptr};
  size_t n_{0};
  Output out_[kMaxPendingOutputs]{};
};
}  // namespace mlparts
