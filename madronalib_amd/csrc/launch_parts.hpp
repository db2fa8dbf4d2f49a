// launch_parts.hpp — the HOST bookkeeping of a bank launch that goes out in parts ("Launch parts"): where a
// bank's voices are cut, what the engine remembers of the parts that run on its side stream until the two streams meet again, and
// the two-stream rule itself (Streams<Api>, below): the fork, the lazy join and the order the parts go out in, with the two raw
// streams, which nothing outside it can reach. Plain C++ that never touches a device: built and tested without any HIP header
// (mlgpu_internal.hpp binds Streams to HIP; tests/cpp/launch_streams_test.cpp to a fake); capi.hip is the caller.
//
// A plain launch of a bank's V voices may go out as two kernels, voices [0, v0) on the engine's stream and [v0, V) on a side stream.
// Consecutive launches of the bank depend on each other only through each voice's own state, so each part is serial on its own
// stream and the parts need not meet while the host keeps making such launches of the same bank. The engine JOINS the streams
// lazily: before anything else it enqueues. What decides "anything else" is here. Each stream's window of voices may be cut once
// more (splitPlan): up to four kernels, two per stream, which write between them exactly the addresses the two wrote.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mlparts
{
// chain_kernel deals its workgroups to the XCDs in whole rounds of 8 (mldsp_kernels.hpp: remapped_block); a part whose workgroup
// count is a multiple of 8 keeps that remap whole. 8 workgroups of 256 lanes:
constexpr size_t kLanesPerWorkgroup = 256;  // (mldsp_kernels.hpp: kChainBlock; chains.hip asserts they agree)
constexpr size_t kSplitUnit = 8 * kLanesPerWorkgroup;
constexpr size_t kMaxPendingOutputs = 8;
constexpr int kMaxParts = 4;
// More than two kernels per launch only where the smallest of them still works on this many voice-samples (automatic mode). From the
// two shapes measured (profiles/bank_launch_plan.md): quarters of 65 536 voices x 30 DSPVectors (2^26.9 voice-samples each) ran 7 %
// faster than halves, quarters of 262 144 voices x 1 DSPVector (2^24) 13 % slower; nothing in between was measured, so the threshold
// is the power of two next to the shape that gained.
constexpr size_t kMinSamplesPerQuarter = (size_t)1 << 26;

// mlgpu_engine_set_launch_parts
enum Mode
{
  kAuto = 0,   // by size: two parts, or four, when each still puts a workgroup on every CU (four: and has kMinSamplesPerQuarter)
  kNever = 1,  // one launch, always
  kHalves = 2,   // two parts whenever there is a second part to make (tests)
  kQuarters = 3  // ... and each stream's part cut once more whenever it has a second unit, sizes notwithstanding (tests)
};
inline bool validMode(int mode) { return mode >= kAuto && mode <= kQuarters; }

// Where a launch of V voices is cut: v0, a multiple of kSplitUnit with 0 < v0 < V, or 0 for "one launch".
// The first part is the whole units of V / 2 (at least one), the second part the rest, ragged or not.
// (kQuarters cuts the streams where kHalves does.)
size_t splitPoint(size_t V, int mode, size_t cuCount, size_t lanesPerWorkgroup);

// The kernels of one launch of V voices over T DSPVectors: part i is voices [cut[i], cut[i + 1]); parts [0, firstSide) go on the
// engine's stream, parts [firstSide, n) on the side stream. n == 1 (firstSide == 1) is one launch. The boundary between the streams,
// cut[firstSide], is splitPoint(V, mode, ...), whatever else the plan does: the side stream writes what it writes in two parts. A
// stream's window is cut once more at the whole units of half its size (at least one) if it has more than one unit and, in the
// automatic mode, if each resulting kernel still has a workgroup for every CU and kMinSamplesPerQuarter voice-samples to work on.
struct Plan
{
  size_t cut[kMaxParts + 1];
  int n;
  int firstSide;
};
Plan splitPlan(size_t V, size_t T, int mode, size_t cuCount, size_t lanesPerWorkgroup);

// Is the kernel of a part of `voices` voices at most one workgroup per CU? Such a kernel is expected to have one wavefront on each
// SIMD it uses - the dispatcher deals a kernel's workgroups out over the CUs, it does not promise to - and then takes no turns at the
// priority levels (MLGPU_KFLAG_LONE_WAVEFRONTS, mlgpu_device_args.hpp). Only speed depends on the expectation: the bits are the
// same with and without the turns.
inline bool atMostAWorkgroupPerCu(size_t voices, size_t cuCount, size_t lanesPerWorkgroup)
{
  return voices / lanesPerWorkgroup + (voices % lanesPerWorkgroup != 0) <= cuCount;
}

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

// The two streams themselves: the engine's main stream (adopted: made and destroyed by the engine), the side stream and the fork and
// join events (made here on first use, destroyed here), the Pending book, and the one order in which they are used. The raw handles
// have no accessor: stream() is the only way to the main stream and joins first, launch() the only way to the side stream, and
// then only for the parts of a plan. `Api` supplies the stream and event calls (mlgpu_internal.hpp binds HIP,
// tests/cpp/launch_streams_test.cpp a fake that logs every call and fails on demand):
//   Stream, Event, Error;  static constexpr Error kSuccess;
//   Error priority(Stream, int&);  Error createStream(Stream&, int priority) (non-blocking);  void destroyStream(Stream);
//   Error createEvent(Event&) (no timing);  void destroyEvent(Event);  Error record(Event, Stream);  Error wait(Stream, Event);
//   Error synchronize(Stream).
template <class Api>
class Streams
{
 public:
  using Stream = typename Api::Stream;
  using Error = typename Api::Error;

  explicit Streams(Stream main) : main_(main) {}
  Streams(const Streams&) = delete;
  Streams& operator=(const Streams&) = delete;
  ~Streams()
  {
    if (!made_) return;
    Api::destroyStream(side_);
    Api::destroyEvent(joinEvent_);
    Api::destroyEvent(forkEvent_);
  }

  // The main stream, for everything that is enqueued on it, waits for it or hands it out: it first waits for what is pending on the
  // side stream, so nobody can forget the join.
  Stream stream()
  {
    if (pending_.any()) join();
    return main_;
  }

  // One launch of `owner` into `out` as the kernels of `plan` (n > 1): launchPart(i, stream) -> Error enqueues part i. Where the
  // pending launches do not admit this one the streams meet and part again first. The streams' kernels go out in turn - main 0,
  // side 0, main 1, side 1 - so that both streams have work from the start, up to the first that fails; `call` names the caller for
  // the report of what a later join cannot hand over (takeSideError). inParts false: no side stream to be had; nothing is pending,
  // nothing was counted or launched, and the caller launches in one part on stream(), as it always could.
  struct Launched
  {
    bool inParts;
    Error error;
  };
  template <class LaunchPart>
  Launched launch(const Plan& plan, const void* owner, const Output& out, const char* call, LaunchPart&& launchPart)
  {
    if (!pending_.admits(owner, out))
    {
      stream();  // (the main stream waits for what is pending, if anything is)
      if (fork() != Api::kSuccess) return {false, Api::kSuccess};
    }
    pending_.launched(owner, out);
    call_ = call;
    Error err = Api::kSuccess;
    for (int i = 0; err == Api::kSuccess && (i < plan.firstSide || plan.firstSide + i < plan.n); ++i)
    {
      if (i < plan.firstSide) err = launchPart(i, main_);
      const int j = plan.firstSide + i;
      if (err == Api::kSuccess && j < plan.n) err = launchPart(j, side_);
    }
    ++splitLaunches_;
    return {true, err};
  }

  // What a join could not hand to the main stream, and the call whose part was pending then: told once, kSuccess from then on.
  Error takeSideError(const char** call)
  {
    const Error err = sideError_;
    sideError_ = Api::kSuccess;
    *call = sideErrorCall_;
    return err;
  }

  const Pending& pending() const { return pending_; }  // what runs on the side stream since the streams last met
  uint64_t splitLaunches() const { return splitLaunches_; }  // launches (calls, not kernels) that went out in parts
  uint64_t joins() const { return joins_; }                  // how often the streams met

 private:
  // The side stream takes up where the main stream is now. It is made on first use, with the main stream's priority, together with
  // the two events: all three or none, so a failure leaves nothing half made and the next call tries again.
  Error fork()
  {
    Error err = Api::kSuccess;
    if (!made_)
    {
      int priority = 0;
      Stream side{};
      typename Api::Event forkEvent{}, joinEvent{};
      if ((err = Api::priority(main_, priority)) != Api::kSuccess) return err;
      if ((err = Api::createStream(side, priority)) != Api::kSuccess) return err;
      if ((err = Api::createEvent(forkEvent)) != Api::kSuccess)
      {
        Api::destroyStream(side);
        return err;
      }
      if ((err = Api::createEvent(joinEvent)) != Api::kSuccess)
      {
        Api::destroyStream(side);
        Api::destroyEvent(forkEvent);
        return err;
      }
      side_ = side;
      forkEvent_ = forkEvent;
      joinEvent_ = joinEvent;
      made_ = true;
    }
    if ((err = Api::record(forkEvent_, main_)) != Api::kSuccess) return err;
    return Api::wait(side_, forkEvent_);
  }
  // The main stream waits for the side stream's work; where the event cannot carry that, the host waits instead, and what failed is
  // kept for takeSideError.
  void join()
  {
    Error err = Api::record(joinEvent_, side_);
    if (err == Api::kSuccess) err = Api::wait(main_, joinEvent_);
    if (err != Api::kSuccess)
    {
      const Error waited = Api::synchronize(side_);
      sideError_ = waited != Api::kSuccess ? waited : err;
      sideErrorCall_ = call_;
    }
    pending_.joined();
    ++joins_;
  }

  Stream main_;
  Stream side_{};
  typename Api::Event forkEvent_{}, joinEvent_{};
  bool made_{false};  // the side stream and the two events
  Pending pending_;
  const char* call_{""};  // the call whose part is pending
  Error sideError_{Api::kSuccess};
  const char* sideErrorCall_{""};
  uint64_t splitLaunches_{0}, joins_{0};
};
}  // namespace mlparts
