// tests/cpp/events_sounding_test.cpp — the host event router's sounding set and its routing ahead of the launch
// (madronalib_amd/csrc/events_router.cpp: EventRouter::soundingVoices, routeAhead), built with g++ from that one file, no HIP header
// on the include path (tests/test_events_sounding_cpp.py). Hand-written small performances, polyphony 2 and 4; after each routed
// launch the exact set: every voice the launch holds a record for, and every voice that holds a non-zero velocity at its end. The
// first event of an instrument sends a REC_AWAKE record to each of its voices, so its first launch lists them all.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../madronalib_amd/csrc/events_router.hpp"

using namespace mlev;

static int failures = 0;
#define REQUIRE(cond)                                                 \
  do                                                                  \
  {                                                                   \
    if (!(cond))                                                      \
    {                                                                 \
      printf("REQUIRE failed at line %d: %s\n", __LINE__, #cond);     \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

typedef std::vector<uint32_t> Set;

static mlgpu_event event(int type, int sourceIdx, int time, float v1 = 0.f, float v2 = 0.f)
{
  mlgpu_event e{};
  e.type = (uint8_t)type;
  e.channel = 1;
  e.source_idx = (uint16_t)sourceIdx;
  e.time = time;
  e.value1 = v1;
  e.value2 = v2;
  return e;
}
static mlgpu_event noteOn(int key, int time, float vel = 0.5f) { return event(MLGPU_EVENT_NOTE_ON, key, time, (float)(key - 60) / 12.f, vel); }
static mlgpu_event noteOff(int key, int time) { return event(MLGPU_EVENT_NOTE_OFF, key, time); }
static mlgpu_event pedal(int time, float value) { return event(MLGPU_EVENT_SUSTAIN_PEDAL, 0, time, value); }

static Set sounding(const EventRouter& r)
{
  Set s(r.instruments() * (size_t)r.polyphony(), 0xDEADu);
  size_t n = 0;
  REQUIRE(r.soundingVoices(s.data(), s.size(), &n));
  REQUIRE(n <= s.size());
  for (size_t i = n; i < s.size(); ++i) REQUIRE(s[i] == 0xDEADu);  // nothing written past the set
  s.resize(n);
  return s;
}
// one host block: the events added (to `instrument`), routed as nVectors DSPVectors, cleared; the sounding set of that launch
static Set block(EventRouter& r, const std::vector<mlgpu_event>& events, size_t nVectors = 1, size_t instrument = 0)
{
  for (const mlgpu_event& e : events) REQUIRE(r.addEvent(instrument, e));
  REQUIRE(r.route(nVectors, 0));
  r.clearEvents();
  return sounding(r);
}
static bool same(const Set& got, const Set& want, int line)
{
  if (got == want) return true;
  printf("sounding sets differ (line %d): got {", line);
  for (uint32_t v : got) printf(" %u", v);
  printf(" }, want {");
  for (uint32_t v : want) printf(" %u", v);
  printf(" }\n");
  ++failures;
  return false;
}
#define EXPECT_SET(got, ...) same(got, Set __VA_ARGS__, __LINE__)

// poly 2: a note on, held over launches without events, its note-off in a later launch, silence after it
static void noteOnAndLaterOff()
{
  EventRouter r(3, 2);
  EXPECT_SET(sounding(r), ({}));                             // before any route
  EXPECT_SET(block(r, {}), ({}));                            // a launch with no events, nobody awake
  EXPECT_SET(block(r, {noteOn(60, 3)}, 1, 1), ({2, 3}));     // instrument 1: voice 2 plays, voice 3 has its awake record
  EXPECT_SET(block(r, {}), ({2}));                           // no events: the held voice
  EXPECT_SET(block(r, {}, 3), ({2}));
  EXPECT_SET(block(r, {noteOff(60, 70)}, 2, 1), ({2}));      // the note-off's record, in the launch's second vector
  EXPECT_SET(block(r, {}), ({}));
  // on and off inside one launch of two vectors: in that launch's set by its records, held by nobody at its end
  EXPECT_SET(block(r, {noteOn(64, 5), noteOff(64, 100)}, 2, 2), ({4, 5}));
  EXPECT_SET(block(r, {}), ({}));
  // a note-on of velocity 0 holds nothing
  EXPECT_SET(block(r, {noteOn(61, 0, 0.f)}, 1, 1), ({3}));   // (the allocator's next free voice)
  EXPECT_SET(block(r, {}), ({}));
}

// poly 2: the third note steals the voice nearest by key; the stolen voice goes on sounding under its new key
static void stolenVoice()
{
  EventRouter r(1, 2);
  EXPECT_SET(block(r, {noteOn(60, 0), noteOn(72, 1)}), ({0, 1}));
  EXPECT_SET(block(r, {noteOn(61, 20)}), ({0, 1}));           // voice 0 retriggered (a record), voice 1 held
  EXPECT_SET(block(r, {noteOff(60, 2)}), ({0, 1}));           // key 60 owns no voice any more: no record, both held
  EXPECT_SET(block(r, {noteOff(72, 2)}), ({0, 1}));           // voice 1's note-off record; voice 0 held
  EXPECT_SET(block(r, {}), ({0}));
  EXPECT_SET(block(r, {noteOff(61, 9)}), ({0}));
  EXPECT_SET(block(r, {}), ({}));
}

// poly 4, unison: every voice of the instrument plays the note; the other instrument stays out of the set
static void unison()
{
  EventRouter r(2, 4);
  r.setUnison(true);
  EXPECT_SET(block(r, {noteOn(50, 0)}, 1, 1), ({4, 5, 6, 7}));
  EXPECT_SET(block(r, {}), ({4, 5, 6, 7}));
  EXPECT_SET(block(r, {noteOn(64, 8)}, 1, 1), ({4, 5, 6, 7}));
  EXPECT_SET(block(r, {noteOff(64, 4)}, 1, 1), ({4, 5, 6, 7}));  // back to the older key, the velocity kept
  EXPECT_SET(block(r, {}), ({4, 5, 6, 7}));
  EXPECT_SET(block(r, {noteOff(50, 6)}, 1, 1), ({4, 5, 6, 7}));  // the note-offs' records
  EXPECT_SET(block(r, {}), ({}));
}

// poly 4: a key released under the pedal goes on sounding until the pedal's release, which makes the note-off
static void pedalSustainedKey()
{
  EventRouter r(1, 4);
  EXPECT_SET(block(r, {pedal(0, 1.f), noteOn(60, 5), noteOn(67, 6)}), ({0, 1, 2, 3}));  // (awake records)
  EXPECT_SET(block(r, {noteOff(60, 20)}), ({0, 1}));        // under the pedal: no record, still held
  EXPECT_SET(block(r, {}), ({0, 1}));
  EXPECT_SET(block(r, {pedal(40, 0.f)}), ({0, 1}));         // voice 0: the release's note-off record; voice 1: its key is still down
  EXPECT_SET(block(r, {}), ({1}));
  EXPECT_SET(block(r, {noteOff(67, 0)}), ({1}));
  EXPECT_SET(block(r, {}), ({}));
}

// a capacity too small: the size is reported, nothing is written; MPE has no such set; clear() empties it
static void capacityProtocolClear()
{
  EventRouter r(2, 2);
  block(r, {noteOn(60, 0), noteOn(62, 1)}, 1, 1);
  uint32_t out[4] = {9, 9, 9, 9};
  size_t n = 77;
  REQUIRE(!r.soundingVoices(out, 1, &n) && n == 2 && out[0] == 9 && out[1] == 9);
  REQUIRE(!r.soundingVoices(nullptr, 0, &n) && n == 2);
  REQUIRE(r.soundingVoices(out, 2, &n) && n == 2 && out[0] == 2 && out[1] == 3 && out[2] == 9);
  r.clear();
  EXPECT_SET(sounding(r), ({}));  // clear() resets the object: the routed launch's records go with the held voices, before any route
  EXPECT_SET(block(r, {}), ({}));
  // routed under MPE - lanes instrument * 32 + slot for polyphony 16, far past the 6 x 16 voices' bitmap -, then back to MIDI
  // (setProtocol is followed by clear): an empty set, before and after the next route
  EventRouter p(6, 16);
  p.setProtocol(true);
  p.clear();
  for (size_t i = 0; i < 6; ++i) REQUIRE(p.addEvent(i, noteOn(60, 0)) && p.addEvent(i, noteOn(64, 1)));
  REQUIRE(p.route(1, 0) && p.dirtyLaneCount() > 0);
  p.clearEvents();
  p.setProtocol(false);
  p.clear();
  REQUIRE(p.dirtyLaneCount() == 0 && p.recordCount() == 0);
  EXPECT_SET(sounding(p), ({}));
  EXPECT_SET(block(p, {}), ({}));
  EXPECT_SET(block(p, {noteOn(60, 0)}, 1, 5), ({80}));  // (awake records went out under MPE; the voice index is MIDI's again)
  EventRouter m(1, 2);
  m.setProtocol(true);
  m.clear();
  n = 77;
  REQUIRE(!m.soundingVoices(out, 4, &n) && n == 0);
}

struct Packed
{
  std::vector<Rec> recs;
  std::vector<LaneRange> lanes;
  bool operator==(const Packed& o) const
  {
    return recs.size() == o.recs.size() && lanes.size() == o.lanes.size() && (recs.empty() || !memcmp(recs.data(), o.recs.data(), sizeof(Rec) * recs.size())) &&
           (lanes.empty() || !memcmp(lanes.data(), o.lanes.data(), sizeof(LaneRange) * lanes.size()));
  }
};
static Packed packed(const EventRouter& r)
{
  Packed p;
  p.recs.resize(r.recordCount());
  p.lanes.resize(r.dirtyLaneCount());
  r.pack(p.recs.data(), p.lanes.data());
  return p;
}

// routeAhead followed by the process-side route gives the records a single route gives; a mismatch is reported and consumes nothing
static void routeAhead()
{
  const std::vector<mlgpu_event> first = {noteOn(60, 3), noteOn(72, 70), noteOn(61, 100)}, second = {noteOff(72, 5), noteOn(40, 64)};
  EventRouter a(2, 2), b(2, 2);
  for (const mlgpu_event& e : first) REQUIRE(a.addEvent(1, e) && b.addEvent(1, e));
  REQUIRE(!a.aheadPending());
  REQUIRE(a.routeAhead(2, 0) && a.aheadPending() && a.aheadIs(2, 0) && !a.aheadIs(2, 64) && !a.aheadIs(1, 0));
  EXPECT_SET(sounding(a), ({2, 3}));
  const Packed ahead = packed(a);
  REQUIRE(ahead.recs.size() == 5);  // awake x 2, on, on, retrig
  // while the launch is pending: other values, more events and a second routeAhead are refused, and change nothing
  REQUIRE(!a.route(3, 0) && !a.route(2, 64) && !a.routeAhead(2, 0) && !a.addEvent(1, noteOn(50, 0)) && a.aheadPending());
  REQUIRE(packed(a) == ahead);
  EXPECT_SET(sounding(a), ({2, 3}));
  // the launch's own route takes the records over as they are
  REQUIRE(a.route(2, 0) && !a.aheadPending());
  REQUIRE(b.route(2, 0));
  REQUIRE(packed(a) == ahead && packed(b) == ahead);
  EXPECT_SET(sounding(b), ({2, 3}));
  a.clearEvents(), b.clearEvents();
  // ... and the routers are in the same state: the next block, routed ahead in one and in one go in the other
  for (const mlgpu_event& e : second) REQUIRE(a.addEvent(1, e) && b.addEvent(1, e));
  REQUIRE(a.routeAhead(2, 0) && a.route(2, 0) && b.route(2, 0));
  REQUIRE(packed(a) == packed(b) && packed(a).recs.size() == 2);
  EXPECT_SET(sounding(a), ({2, 3}));
  EXPECT_SET(sounding(b), ({2, 3}));
  // clear() cancels a pending launch
  REQUIRE(a.routeAhead(1, 0) && a.aheadPending());
  a.clear();
  REQUIRE(!a.aheadPending() && a.addEvent(0, noteOn(60, 0)) && a.route(4, 0));
}

int main()
{
  noteOnAndLaterOff();
  stolenVoice();
  unison();
  pedalSustainedKey();
  capacityProtocolClear();
  routeAhead();
  if (failures) printf("%d FAILED\n", failures);
  else printf("All tests passed\n");
  return failures ? 1 : 0;
}
