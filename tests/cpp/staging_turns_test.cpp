// The turn-taking rule of the pinned staging sets (madronalib_amd/csrc/staging_turns.hpp) without a device: built by g++ from the
// header alone, under the address and undefined-behaviour sanitizers, by tests/test_staging_turns_cpu.py. A fake event API counts
// every call and fails on demand; the failure paths - a record or a wait that fails - are the ones no healthy device shows.
#include <cstdio>

#include "../../madronalib_amd/csrc/staging_turns.hpp"

namespace
{
struct FakeApi
{
  struct Event
  {
    int* live{nullptr};  // heap memory per event: a leak, a double destroy or a use after destroy is the sanitizer's to find
  };
  using Stream = int;
  static int creates, destroys, waits, records, drains, lastStream;
  static bool failCreate, failWait, failRecord;
  static void clear()
  {
    creates = destroys = waits = records = drains = 0;
    lastStream = -1;
    failCreate = failWait = failRecord = false;
  }
  static bool create(Event& ev)
  {
    if (failCreate) return false;
    ++creates;
    ev.live = new int(0);
    return true;
  }
  static void destroy(Event ev)
  {
    ++destroys;
    delete ev.live;
  }
  static bool wait(Event ev)
  {
    ++waits;
    return !failWait && *ev.live >= 0;
  }
  static bool record(Event ev, Stream stream)
  {
    ++records;
    lastStream = stream;
    if (failRecord) return false;
    ++*ev.live;
    return true;
  }
  static void drain(Stream stream)
  {
    ++drains;
    lastStream = stream;
  }
};
int FakeApi::creates, FakeApi::destroys, FakeApi::waits, FakeApi::records, FakeApi::drains, FakeApi::lastStream;
bool FakeApi::failCreate, FakeApi::failWait, FakeApi::failRecord;

struct Payload
{
  int tag{0};
};
using Turn = mlstage::Turn<FakeApi>;
using Turns = mlstage::Turns<FakeApi, Payload>;

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

const int kStream = 7;

// 1. take() then submitted(), five times: sets 0, 1, 0, 1, 0; 3 waits (none on the first use of either set), 5 records
void alternation()
{
  FakeApi::clear();
  Turns t;
  CHECK(t.create() && FakeApi::creates == 2);
  const int want[5] = {0, 1, 0, 1, 0}, waitsAfter[5] = {0, 0, 1, 2, 3};
  for (int i = 0; i < 5; ++i)
  {
    Turns::Slot* s = t.take();
    CHECK(s == &t.set[want[i]]);
    CHECK(FakeApi::waits == waitsAfter[i]);
    CHECK(s && !s->turn.pending());  // a set that was taken is free to write
    if (s) s->turn.submitted(kStream);
    CHECK(s && s->turn.pending());
  }
  CHECK(FakeApi::waits == 3 && FakeApi::records == 5 && FakeApi::drains == 0 && FakeApi::lastStream == kStream);
}

// 2. a take() with nothing submitted in between waits for nothing
void nothingSubmitted()
{
  FakeApi::clear();
  Turns t;
  t.create();
  for (int i = 0; i < 4; ++i) CHECK(t.take() == &t.set[i & 1]);
  CHECK(FakeApi::waits == 0 && FakeApi::records == 0);
  t.take()->turn.submitted(kStream);  // set 0
  CHECK(t.take() == &t.set[1] && FakeApi::waits == 0);  // set 1 was never submitted
  CHECK(t.take() == &t.set[0] && FakeApi::waits == 1);
  CHECK(t.take() == &t.set[1] && t.take() == &t.set[0] && FakeApi::waits == 1);  // waited for once
}

// 3. a failing record: exactly one drain, pending() false, the next take() of that set does not wait
void recordFails()
{
  FakeApi::clear();
  Turns t;
  t.create();
  Turns::Slot* s0 = t.take();
  FakeApi::failRecord = true;
  s0->turn.submitted(kStream);
  FakeApi::failRecord = false;
  CHECK(FakeApi::records == 1 && FakeApi::drains == 1 && FakeApi::lastStream == kStream && !s0->turn.pending());
  t.take()->turn.submitted(kStream);  // set 1, recorded
  CHECK(FakeApi::drains == 1);
  CHECK(t.take() == s0 && FakeApi::waits == 0);
  CHECK(t.take() == &t.set[1] && FakeApi::waits == 1);
  // a turn without an event cannot record: submitted() drains, whatever the stream holds is over before the set looks free
  FakeApi::clear();
  Turn bare;
  bare.submitted(kStream);
  CHECK(FakeApi::records == 0 && FakeApi::drains == 1 && !bare.pending());
}

// 4. a failing wait: take() returns null, the index has not moved, the set is still pending, a later take() returns the same set
void waitFails()
{
  FakeApi::clear();
  Turns t;
  t.create();
  Turns::Slot* s0 = t.take();
  s0->turn.submitted(kStream);
  t.take()->turn.submitted(kStream);
  FakeApi::failWait = true;
  const int before = t.next;
  CHECK(t.take() == nullptr && FakeApi::waits == 1);
  CHECK(t.next == before && s0->turn.pending());
  CHECK(t.take() == nullptr && FakeApi::waits == 2 && t.next == before && s0->turn.pending());
  FakeApi::failWait = false;
  CHECK(t.take() == s0 && FakeApi::waits == 3 && !s0->turn.pending());
  CHECK(t.take() == &t.set[1] && FakeApi::waits == 4);
  // the same on a single turn: it stays pending until a wait succeeds
  Turn one;
  one.create();
  one.submitted(kStream);
  FakeApi::failWait = true;
  CHECK(!one.wait() && one.pending());
  FakeApi::failWait = false;
  CHECK(one.wait() && !one.pending());
}

// 5. drained() clears pending on both sets without a wait
void drainedByTheCaller()
{
  FakeApi::clear();
  Turns t;
  t.create();
  t.take()->turn.submitted(kStream);
  t.take()->turn.submitted(kStream);
  CHECK(t.set[0].turn.pending() && t.set[1].turn.pending());
  t.drained();
  CHECK(!t.set[0].turn.pending() && !t.set[1].turn.pending());
  CHECK(FakeApi::waits == 0 && FakeApi::drains == 0);  // (the caller synchronised: no call of the rule's own)
  CHECK(t.take() == &t.set[0] && t.take() == &t.set[1] && FakeApi::waits == 0);
}

// 6. create() twice creates one event; reset() destroys it once and clears pending; create() after reset() creates again
void eventLifetime()
{
  FakeApi::clear();
  {
    Turn one;
    CHECK(one.create() && one.create() && FakeApi::creates == 1);
    one.submitted(kStream);
    one.reset();
    CHECK(FakeApi::destroys == 1 && !one.pending());
    one.reset();
    CHECK(FakeApi::destroys == 1);
    CHECK(one.wait() && FakeApi::waits == 0);  // nothing pending: the destroyed event is not touched
    CHECK(one.create() && FakeApi::creates == 2);
    one.submitted(kStream);
    CHECK(one.pending() && FakeApi::records == 2);
    FakeApi::failCreate = true;
    Turn none;
    CHECK(!none.create() && FakeApi::creates == 2);
    FakeApi::failCreate = false;
    CHECK(none.create() && FakeApi::creates == 3);
  }
  CHECK(FakeApi::destroys == 3);  // a turn that goes takes its event with it
  FakeApi::clear();
  {
    Turns t;
    CHECK(t.create() && t.create() && FakeApi::creates == 2);
    t.take()->turn.submitted(kStream);
    t.reset();
    CHECK(FakeApi::destroys == 2 && !t.set[0].turn.pending());
    FakeApi::failCreate = true;
    CHECK(!t.create());
    FakeApi::failCreate = false;
    CHECK(t.create() && FakeApi::creates == 4);
  }
  CHECK(FakeApi::destroys == 4);
}

// 7. a single turn the way a round trip uses it: its own alternation, wait() before the set is written and before its data is read
void roundTrip()
{
  FakeApi::clear();
  Turn one;
  one.create();
  CHECK(one.wait() && FakeApi::waits == 0);  // nothing pending: a no-op
  one.submitted(kStream);
  CHECK(one.pending() && FakeApi::records == 1);
  CHECK(one.wait() && FakeApi::waits == 1 && !one.pending());
  CHECK(one.wait() && FakeApi::waits == 1);  // waited for once
  // a block that failed half way (the copy in went, the copy out did not): submitted all the same, and waited for before the next use
  one.submitted(kStream);
  CHECK(one.wait() && FakeApi::waits == 2);
  // ... and when the record fails as well the stream is drained: nothing pending, nothing in flight
  FakeApi::failRecord = true;
  one.submitted(kStream);
  FakeApi::failRecord = false;
  CHECK(FakeApi::drains == 1 && one.wait() && FakeApi::waits == 2);
}
}  // namespace

int main()
{
  alternation();
  nothingSubmitted();
  recordFails();
  waitFails();
  drainedByTheCaller();
  eventLifetime();
  roundTrip();
  if (failures == 0) printf("All tests passed\n");
  return failures ? 1 : 0;
}
