// The two-stream rule of launches that go out in parts (mlparts::Streams, madronalib_amd/csrc/launch_parts.hpp) without a device:
// built by g++ from the header and launch_parts.cpp, under the address and undefined-behaviour sanitizers, by
// tests/test_launch_streams_cpu.py. A fake stream API logs every call with its arguments and fails the n-th call of a kind on
// demand; the failure paths - a fork that fails at any of its steps, a join that falls back to a host wait, a part that does not
// launch - are the ones no healthy device shows.
#include <cstdio>
#include <vector>

#include "../../madronalib_amd/csrc/launch_parts.hpp"

namespace
{
enum Kind
{
  kPriority,       // a: stream
  kCreateStream,   // a: the new stream (0: failed), b: priority
  kDestroyStream,  // a: stream
  kCreateEvent,    // a: the new event (0: failed)
  kDestroyEvent,   // a: event
  kRecord,         // a: event, b: stream
  kWait,           // a: stream, b: event
  kSynchronize,    // a: stream
  kLaunch,         // a: part, b: stream (the test's launchPart, not an Api call)
  kKinds
};
const char* const kKindNames[kKinds] = {"priority", "createStream", "destroyStream", "createEvent", "destroyEvent",
                                        "record",   "wait",         "synchronize",   "launch"};
struct Call
{
  Kind kind;
  int a, b;
  bool operator==(const Call& o) const { return kind == o.kind && a == o.a && b == o.b; }
};
using Log = std::vector<Call>;

struct FakeApi
{
  struct Handle
  {
    int id{0};
    int* live{nullptr};  // heap memory per stream and event: a leak, a double destroy or a use after destroy is the sanitizer's to find
  };
  using Stream = Handle;
  using Event = Handle;
  using Error = int;
  static constexpr Error kSuccess = 0;

  static Log log;
  static int count[kKinds], failAt[kKinds], nextId, liveStreams, liveEvents;
  static const int kMainPriority = -3;

  static void clear()
  {
    log.clear();
    for (int k = 0; k < kKinds; ++k) count[k] = failAt[k] = 0;
    nextId = 10;
    liveStreams = liveEvents = 0;
  }
  static void failNth(Kind kind, int n) { failAt[kind] = count[kind] + n; }  // the n-th call of `kind` from now fails with errorOf(kind)
  static Error errorOf(Kind kind) { return 100 + (int)kind; }
  static Error called(Kind kind, int a, int b = 0)
  {
    log.push_back({kind, a, b});
    return ++count[kind] == failAt[kind] ? errorOf(kind) : kSuccess;
  }

  static int id(const Handle& h) { return h.id + 0 * *(volatile int*)h.live; }  // (reads the handle's memory: it must be alive)

  static Error priority(Stream stream, int& priority)
  {
    const Error err = called(kPriority, id(stream));
    if (err == kSuccess) priority = kMainPriority;
    return err;
  }
  static Error createStream(Stream& stream, int priority)
  {
    const bool fails = count[kCreateStream] + 1 == failAt[kCreateStream];
    const Error err = called(kCreateStream, fails ? 0 : nextId, priority);
    if (err != kSuccess) return err;
    stream = {nextId++, new int(0)};
    ++liveStreams;
    return kSuccess;
  }
  static void destroyStream(Stream stream)
  {
    called(kDestroyStream, stream.id);
    delete stream.live;
    --liveStreams;
  }
  static Error createEvent(Event& ev)
  {
    const bool fails = count[kCreateEvent] + 1 == failAt[kCreateEvent];
    const Error err = called(kCreateEvent, fails ? 0 : nextId);
    if (err != kSuccess) return err;
    ev = {nextId++, new int(0)};
    ++liveEvents;
    return kSuccess;
  }
  static void destroyEvent(Event ev)
  {
    called(kDestroyEvent, ev.id);
    delete ev.live;
    --liveEvents;
  }
  static Error record(Event ev, Stream stream) { return called(kRecord, id(ev), id(stream)); }
  static Error wait(Stream stream, Event ev) { return called(kWait, id(stream), id(ev)); }
  static Error synchronize(Stream stream) { return called(kSynchronize, id(stream)); }
};
Log FakeApi::log;
int FakeApi::count[kKinds], FakeApi::failAt[kKinds], FakeApi::nextId, FakeApi::liveStreams, FakeApi::liveEvents;

using Streams = mlparts::Streams<FakeApi>;

int failures = 0;
#define CHECK(cond)                                              \
  do                                                             \
  {                                                              \
    if (!(cond))                                                 \
    {                                                            \
      ++failures;                                                \
      printf("FAILED line %d: %s\n", __LINE__, #cond);           \
    }                                                            \
  } while (0)

void print(const char* name, const Log& log)
{
  printf("  %s:", name);
  for (const Call& c : log) printf(" %s(%d, %d)", kKindNames[c.kind], c.a, c.b);
  printf("\n");
}
// the log is exactly `want`, and is cleared
#define CHECK_LOG(...)                                           \
  do                                                             \
  {                                                              \
    const Log want = __VA_ARGS__;                                \
    if (!(FakeApi::log == want))                                 \
    {                                                            \
      ++failures;                                                \
      printf("FAILED line %d: the log\n", __LINE__);             \
      print("want", want);                                       \
      print("got ", FakeApi::log);                               \
    }                                                            \
    FakeApi::log.clear();                                        \
  } while (0)

Log operator+(Log a, const Log& b)
{
  a.insert(a.end(), b.begin(), b.end());
  return a;
}

// the engine's stream: made and destroyed by the test, as the engine makes and destroys its own
const int kMain = 1, kSide = 10, kFork = 11, kJoin = 12;  // (the ids the fake hands out on a first fork)
const int kPrio = FakeApi::kMainPriority;
struct Main
{
  FakeApi::Stream stream{kMain, new int(0)};
  ~Main() { delete stream.live; }
};

const int kOwner = 1, kOther = 2;  // (their addresses are the owners)
const mlparts::Output kOut{0x1000, 0x100, 0, 3};
const mlparts::Output kApart{0x2000, 0x100, 0, 3};
const mlparts::Output kOverlapping{0x1080, 0x100, 0, 3};

mlparts::Plan planOf(int n, int firstSide)
{
  mlparts::Plan p{};
  for (int i = 0; i <= n; ++i) p.cut[i] = (size_t)i * mlparts::kSplitUnit;
  p.n = n;
  p.firstSide = firstSide;
  return p;
}
// launchPart: logs, and fails at part `failPart`
const int kLaunchError = 77;
auto launcher(int failPart = -1)
{
  return [failPart](int part, FakeApi::Stream stream) {
    FakeApi::log.push_back({kLaunch, part, FakeApi::id(stream)});
    return part == failPart ? kLaunchError : FakeApi::kSuccess;
  };
}

// the order the kernels of a plan go out in, written out: main 0, side 0, main 1, side 1
struct Shape
{
  int n, firstSide;
  Log launches;
};
const Shape kShapes[4] = {
    {2, 1, {{kLaunch, 0, kMain}, {kLaunch, 1, kSide}}},
    {4, 2, {{kLaunch, 0, kMain}, {kLaunch, 2, kSide}, {kLaunch, 1, kMain}, {kLaunch, 3, kSide}}},
    {3, 1, {{kLaunch, 0, kMain}, {kLaunch, 1, kSide}, {kLaunch, 2, kSide}}},
    {3, 2, {{kLaunch, 0, kMain}, {kLaunch, 2, kSide}, {kLaunch, 1, kMain}}},
};
const Log kMake = {{kPriority, kMain, 0}, {kCreateStream, kSide, kPrio}, {kCreateEvent, kFork, 0}, {kCreateEvent, kJoin, 0}};
const Log kForkLog = {{kRecord, kFork, kMain}, {kWait, kSide, kFork}};
const Log kJoinLog = {{kRecord, kJoin, kSide}, {kWait, kMain, kJoin}};
const Log kNothing = {};

bool counters(const Streams& s, uint64_t splitLaunches, uint64_t joins) { return s.splitLaunches() == splitLaunches && s.joins() == joins; }

// 1.-4. a first launch makes the side stream and forks; a second one of the same owner, into the same output or one apart from it,
// only launches; stream() joins once
void launchesAndTheLazyJoin()
{
  for (const Shape& shape : kShapes)
  {
    FakeApi::clear();
    Main main;
    {
      Streams s(main.stream);
      const mlparts::Plan plan = planOf(shape.n, shape.firstSide);
      CHECK(!s.pending().any() && counters(s, 0, 0));
      Streams::Launched l = s.launch(plan, &kOwner, kOut, "bank_process", launcher());
      CHECK(l.inParts && l.error == FakeApi::kSuccess);
      CHECK_LOG(kMake + kForkLog + shape.launches);
      CHECK(counters(s, 1, 0) && s.pending().owner() == &kOwner && s.pending().outputs() == 1);

      l = s.launch(plan, &kOwner, kOut, "bank_process", launcher());
      CHECK(l.inParts && l.error == FakeApi::kSuccess);
      CHECK_LOG(shape.launches);
      CHECK(counters(s, 2, 0) && s.pending().owner() == &kOwner && s.pending().outputs() == 1);

      l = s.launch(plan, &kOwner, kApart, "bank_process", launcher());
      CHECK(l.inParts && l.error == FakeApi::kSuccess);
      CHECK_LOG(shape.launches);
      CHECK(counters(s, 3, 0) && s.pending().owner() == &kOwner && s.pending().outputs() == 2);

      CHECK(s.stream().id == kMain);
      CHECK_LOG(kJoinLog);
      CHECK(counters(s, 3, 1) && !s.pending().any() && s.pending().outputs() == 0);
      CHECK(s.stream().id == kMain);
      CHECK_LOG(kNothing);
      CHECK(counters(s, 3, 1));

      // the streams part again with what they have: no priority query, no create
      l = s.launch(plan, &kOwner, kOut, "bank_process", launcher());
      CHECK(l.inParts && l.error == FakeApi::kSuccess);
      CHECK_LOG(kForkLog + shape.launches);
      CHECK(counters(s, 4, 1) && s.pending().any());
      CHECK(FakeApi::liveStreams == 1 && FakeApi::liveEvents == 2);
    }
    // 10. the side stream and the two events go with the object, each once; the main stream is the engine's
    CHECK_LOG({{kDestroyStream, kSide, 0}, {kDestroyEvent, kJoin, 0}, {kDestroyEvent, kFork, 0}});
    CHECK(FakeApi::liveStreams == 0 && FakeApi::liveEvents == 0);
  }
  // ... and an object that never forked destroys nothing
  FakeApi::clear();
  Main main;
  {
    Streams s(main.stream);
    CHECK(s.stream().id == kMain && counters(s, 0, 0));
  }
  CHECK_LOG(kNothing);
}

// 5. a launch the pending ones do not admit - another owner, or an output that overlaps a pending one at another base: the streams
// meet, part again (record and wait, nothing created) and the launches follow
void notAdmitted()
{
  for (int other = 0; other < 2; ++other)
  {
    FakeApi::clear();
    Main main;
    Streams s(main.stream);
    const mlparts::Plan plan = planOf(4, 2);
    s.launch(plan, &kOwner, kOut, "bank_process", launcher());
    FakeApi::log.clear();
    const Streams::Launched l = other ? s.launch(plan, &kOther, kOut, "bank_process", launcher()) : s.launch(plan, &kOwner, kOverlapping, "bank_process", launcher());
    CHECK(l.inParts && l.error == FakeApi::kSuccess);
    CHECK_LOG(kJoinLog + kForkLog + kShapes[1].launches);
    CHECK(counters(s, 2, 1) && s.pending().owner() == (other ? &kOther : &kOwner) && s.pending().outputs() == 1);
  }
}

// 6. fork() failing at each of its six calls: one part, no launch, nothing pending, nothing counted, nothing left half made; the next
// launch tries again - the whole sequence where nothing was made, the record and the wait where the stream and the events stand
void forkFails()
{
  const Call made[4] = {kMake[0], kMake[1], kMake[2], kMake[3]};
  const Log failing[6] = {
      {made[0]},
      {made[0], {kCreateStream, 0, kPrio}},
      {made[0], made[1], {kCreateEvent, 0, 0}, {kDestroyStream, kSide, 0}},
      {made[0], made[1], made[2], {kCreateEvent, 0, 0}, {kDestroyStream, kSide, 0}, {kDestroyEvent, kFork, 0}},
      kMake + Log{kForkLog[0]},
      kMake + kForkLog,
  };
  const Kind kind[6] = {kPriority, kCreateStream, kCreateEvent, kCreateEvent, kRecord, kWait};
  const int nth[6] = {1, 1, 1, 2, 1, 1};
  for (int step = 0; step < 6; ++step)
  {
    FakeApi::clear();
    Main main;
    Streams s(main.stream);
    const mlparts::Plan plan = planOf(4, 2);
    FakeApi::failNth(kind[step], nth[step]);
    Streams::Launched l = s.launch(plan, &kOwner, kOut, "bank_process", launcher());
    CHECK(!l.inParts);
    CHECK_LOG(failing[step]);
    CHECK(!s.pending().any() && counters(s, 0, 0));
    const bool stands = step >= 4;  // all three were made before the record
    CHECK(FakeApi::liveStreams == (stands ? 1 : 0) && FakeApi::liveEvents == (stands ? 2 : 0));
    CHECK(s.stream().id == kMain);  // (where the caller launches its one part)
    CHECK_LOG(kNothing);

    l = s.launch(plan, &kOwner, kOut, "bank_process", launcher());
    CHECK(l.inParts && l.error == FakeApi::kSuccess);
    if (stands)
      CHECK_LOG(kForkLog + kShapes[1].launches);
    else
    {
      // (the fake numbers on: what failed half way took ids with it)
      const Log& got = FakeApi::log;
      CHECK(got.size() == 10 && got[0] == kMake[0] && got[1].kind == kCreateStream && got[1].b == kPrio && got[2].kind == kCreateEvent &&
            got[3].kind == kCreateEvent && got[4].kind == kRecord && got[4].a == got[2].a && got[4].b == kMain && got[5].kind == kWait &&
            got[5].a == got[1].a && got[5].b == got[2].a);
      for (int i = 0; i < 4 && got.size() == 10; ++i)
        CHECK(got[6 + i].kind == kLaunch && got[6 + i].a == kShapes[1].launches[i].a && got[6 + i].b == (i % 2 ? got[1].a : kMain));
      FakeApi::log.clear();
    }
    CHECK(counters(s, 1, 0) && s.pending().owner() == &kOwner);
    CHECK(FakeApi::liveStreams == 1 && FakeApi::liveEvents == 2);
  }
  CHECK(FakeApi::liveStreams == 0 && FakeApi::liveEvents == 0);

  // a fork that fails behind a join: the streams have met and stay met
  FakeApi::clear();
  Main main;
  Streams s(main.stream);
  const mlparts::Plan plan = planOf(2, 1);
  s.launch(plan, &kOwner, kOut, "bank_process", launcher());
  FakeApi::log.clear();
  FakeApi::failNth(kRecord, 2);  // (the join's is the first)
  const Streams::Launched l = s.launch(plan, &kOther, kOut, "bank_process", launcher());
  CHECK(!l.inParts);
  CHECK_LOG(kJoinLog + Log{kForkLog[0]});
  CHECK(!s.pending().any() && counters(s, 1, 1));
  const char* call = nullptr;
  CHECK(s.takeSideError(&call) == FakeApi::kSuccess);
}

// 7. launchPart failing at part k of four: no later part goes out, the error comes back, the launch is counted and the owner is
// pending - parts may be running - so the next stream() joins
void partFails()
{
  const Log& order = kShapes[1].launches;  // main 0, side 2, main 1, side 3
  for (int at = 0; at < 4; ++at)
  {
    FakeApi::clear();
    Main main;
    Streams s(main.stream);
    const Streams::Launched l = s.launch(planOf(4, 2), &kOwner, kOut, "bank_process", launcher(order[at].a));
    CHECK(l.inParts && l.error == kLaunchError);
    CHECK_LOG(kMake + kForkLog + Log(order.begin(), order.begin() + at + 1));
    CHECK(counters(s, 1, 0) && s.pending().owner() == &kOwner && s.pending().outputs() == 1);
    CHECK(s.stream().id == kMain);
    CHECK_LOG(kJoinLog);
    CHECK(counters(s, 1, 1) && !s.pending().any());
  }
}

// 8. join() with the record failing, and with the wait failing: the host waits for the side stream once; the kept error is the first
// one, or the synchronise's own if that fails too; it is taken once, with the call's name; pending is cleared and the join counted
void joinFails()
{
  for (int which = 0; which < 2; ++which)
    for (int syncFails = 0; syncFails < 2; ++syncFails)
    {
      FakeApi::clear();
      Main main;
      Streams s(main.stream);
      static const char kCall[] = "bank_process";
      s.launch(planOf(2, 1), &kOwner, kOut, kCall, launcher());
      FakeApi::log.clear();
      const Kind kind = which ? kWait : kRecord;
      FakeApi::failNth(kind, 1);
      if (syncFails) FakeApi::failNth(kSynchronize, 1);
      CHECK(s.stream().id == kMain);
      const Call sync{kSynchronize, kSide, 0};
      if (which)
        CHECK_LOG(kJoinLog + Log{sync});
      else
        CHECK_LOG({kJoinLog[0], sync});
      CHECK(!s.pending().any() && counters(s, 1, 1));
      CHECK(s.stream().id == kMain);
      CHECK_LOG(kNothing);
      const char* call = nullptr;
      CHECK(s.takeSideError(&call) == FakeApi::errorOf(syncFails ? kSynchronize : kind) && call == kCall);
      CHECK(s.takeSideError(&call) == FakeApi::kSuccess);
      // and the streams part and meet again as ever
      CHECK(s.launch(planOf(2, 1), &kOwner, kOut, kCall, launcher()).inParts);
      CHECK_LOG(kForkLog + kShapes[0].launches);
      s.stream();
      CHECK_LOG(kJoinLog);
      CHECK(counters(s, 2, 2) && s.takeSideError(&call) == FakeApi::kSuccess);
    }
}
}  // namespace

int main()
{
  launchesAndTheLazyJoin();
  notAdmitted();
  forkFails();
  partFails();
  joinFails();
  if (failures == 0) printf("All tests passed\n");
  return failures ? 1 : 0;
}
