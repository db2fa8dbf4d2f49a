// staging_turns.hpp — the turn-taking rule of the pinned staging sets that host uploads go through ("Staging
// turns"). Plain C++ with no HIP include: `Api` supplies the event calls (mlgpu_internal.hpp binds HIP, tests/cpp/staging_turns_test.cpp
// a fake that counts and fails on demand):
//   Event, Stream;  bool create(Event&);  void destroy(Event);  bool wait(Event);  bool record(Event, Stream);  void drain(Stream).
#pragma once

namespace mlstage
{
// One staging set's turn: the event behind the last work enqueued that reads or writes the set, and whether it is still to be waited
// for. A set that does not look pending has nothing in flight: that is what every call site relies on.
template <class Api>
class Turn
{
 public:
  Turn() = default;
  Turn(const Turn&) = delete;
  Turn& operator=(const Turn&) = delete;
  ~Turn() { reset(); }

  bool create()  // the event, unless there is one
  {
    if (!made_) made_ = Api::create(event_);
    return made_;
  }
  void reset()  // the event given up now
  {
    if (made_) Api::destroy(event_);
    made_ = pending_ = false;
  }
  bool wait()  // for what was submitted last, if that is still pending (it stays pending when the wait fails)
  {
    if (pending_ && !Api::wait(event_)) return false;
    pending_ = false;
    return true;
  }
  // Work that uses the set was enqueued on `stream` - or may have been: this is called after a failed copy or launch too. If the event
  // cannot be recorded the stream is drained instead.
  void submitted(typename Api::Stream stream)
  {
    pending_ = made_ && Api::record(event_, stream);
    if (!pending_) Api::drain(stream);
  }
  void drained() { pending_ = false; }  // the caller has synchronised the stream itself
  bool pending() const { return pending_; }

 private:
  typename Api::Event event_{};
  bool made_{false}, pending_{false};
};

// Two sets that take turns, so that a call waits only for its own call before last. `Set` is the caller's payload (buffers, sizes).
template <class Api, class Set>
struct Turns
{
  struct Slot : Set
  {
    Turn<Api> turn;
  };
  Slot set[2];
  int next{0};

  Slot* take()  // the set whose turn it is, free to write; null (and the same set next time) if the wait for it fails
  {
    Slot& s = set[next];
    if (!s.turn.wait()) return nullptr;
    next ^= 1;
    return &s;
  }
  bool create() { return set[0].turn.create() && set[1].turn.create(); }
  void reset()
  {
    for (Slot& s : set) s.turn.reset();
  }
  void drained()
  {
    for (Slot& s : set) s.turn.drained();
  }
};
}  // namespace mlstage
