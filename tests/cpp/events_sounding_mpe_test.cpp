// tests/cpp/events_sounding_mpe_test.cpp — the host event router's sounding set as GRAPH voice indices, in either protocol
// (madronalib_amd/csrc/events_router.cpp: EventRouter::soundingGraphVoices), built with g++ from that one file, no HIP header on the
// include path (tests/test_events_sounding_mpe_cpp.py). Hand-written MPE performances at polyphony 2 and 5 - an instrument is G = 4
// and G = 8 lanes: lane 0 its main voice, lanes 1..polyphony its playing voices, the rest padding - with the exact set after each
// routed launch: `held` goes by voice index, a lane with records is mapped back to instrument * polyphony + slot - 1, the main voice's
// lane and the padding add nothing. Under MIDI every set is also compared with soundingVoices'.
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

static mlgpu_event event(int type, int channel, int sourceIdx, int time, float v1 = 0.f, float v2 = 0.f)
{
  mlgpu_event e{};
  e.type = (uint8_t)type;
  e.channel = (uint8_t)channel;
  e.source_idx = (uint16_t)sourceIdx;
  e.time = time;
  e.value1 = v1;
  e.value2 = v2;
  return e;
}
// MPE: a note's key is its channel (2 and up: the member channels)
static mlgpu_event noteOn(int channel, int key, int time, float vel = 0.5f) { return event(MLGPU_EVENT_NOTE_ON, channel, key, time, (float)(key - 60) / 12.f, vel); }
static mlgpu_event noteOff(int channel, int key, int time) { return event(MLGPU_EVENT_NOTE_OFF, channel, key, time); }
static mlgpu_event bend(int channel, int time, float value) { return event(MLGPU_EVENT_PITCH_BEND, channel, 0, time, value); }
static mlgpu_event allNotesOff(int time) { return event(MLGPU_EVENT_CONTROLLER, 1, 123, time, 0.f); }

static Set sounding(const EventRouter& r)
{
  Set s(r.instruments() * (size_t)r.polyphony(), 0xDEADu);
  size_t n = 0;
  REQUIRE(r.soundingGraphVoices(s.data(), s.size(), &n));
  REQUIRE(n <= s.size());
  for (size_t i = n; i < s.size(); ++i) REQUIRE(s[i] == 0xDEADu);  // nothing written past the set
  s.resize(n);
  for (size_t i = 1; i < s.size(); ++i) REQUIRE(s[i - 1] < s[i]);  // ascending
  // soundingVoices is what it was: under MIDI the same set, under MPE refused with *n = 0
  Set m(r.instruments() * (size_t)r.polyphony(), 0xDEADu);
  size_t nm = 77;
  if (r.mpe()) REQUIRE(!r.soundingVoices(m.data(), m.size(), &nm) && nm == 0 && m[0] == 0xDEADu);
  else
  {
    REQUIRE(r.soundingVoices(m.data(), m.size(), &nm) && nm == n);
    m.resize(nm);
    REQUIRE(m == s);
  }
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

static EventRouter mpeRouter(size_t instruments, int polyphony)
{
  EventRouter r(instruments, polyphony);
  r.setProtocol(true);
  r.clear();
  return r;
}

// poly 2, G = 4: the first event's awake records, a note on a member channel, its note-off in a later launch, channel-1 bends
static void noteOnLaterOffAndMainVoiceBends()
{
  EventRouter r = mpeRouter(3, 2);
  REQUIRE(r.group() == 4 && r.slotBase() == 0 && r.lanes() == 12);
  EXPECT_SET(sounding(r), ({}));                                // before any route
  EXPECT_SET(block(r, {}), ({}));                               // a launch with no events, nobody awake
  // instrument 1's first event: awake records to its main lane 4 and its voices' lanes 5 and 6 - voices 2 and 3; voice 2 plays
  EXPECT_SET(block(r, {noteOn(2, 60, 3)}, 1, 1), ({2, 3}));
  REQUIRE(r.dirtyLaneCount() == 3);                             // (the main lane has a record and is no voice)
  EXPECT_SET(block(r, {}), ({2}));                              // no events: the held voice
  EXPECT_SET(block(r, {}, 3), ({2}));
  // a channel-1 bend alone: a record of the main lane only - it adds no voice once the instrument is awake
  EXPECT_SET(block(r, {bend(1, 9, 0.5f)}, 1, 1), ({2}));
  REQUIRE(r.dirtyLaneCount() == 1 && r.recordCount() == 1);
  EXPECT_SET(block(r, {noteOff(2, 60, 70)}, 2, 1), ({2}));      // the note-off's record, in the launch's second vector
  EXPECT_SET(block(r, {}), ({}));
  EXPECT_SET(block(r, {bend(1, 0, -0.25f)}, 1, 1), ({}));       // nobody held, the main lane's record: an empty set
  REQUIRE(r.dirtyLaneCount() == 1);
  // a member channel's bend reaches the voice its channel plays: a record of that voice's lane (the allocator's next free voice: 3)
  EXPECT_SET(block(r, {noteOn(3, 64, 5)}, 1, 1), ({3}));
  EXPECT_SET(block(r, {bend(3, 1, 0.1f), bend(1, 2, 0.2f)}, 1, 1), ({3}));
  REQUIRE(r.dirtyLaneCount() == 2);
  // on and off inside one launch of two vectors, instrument 2 (lanes 8..11): in the set by its records - the awake records' too -, held
  // by nobody at its end
  EXPECT_SET(block(r, {noteOn(2, 64, 5), noteOff(2, 64, 100)}, 2, 2), ({3, 4, 5}));
  EXPECT_SET(block(r, {}), ({3}));
  // instrument 0 (lanes 0..3): voices 0 and 1
  EXPECT_SET(block(r, {noteOn(5, 40, 0)}, 1, 0), ({0, 1, 3}));
  EXPECT_SET(block(r, {}), ({0, 3}));
}

// poly 2: the third channel steals the voice nearest by key; the stolen voice goes on sounding under its new channel
static void stolenVoice()
{
  EventRouter r = mpeRouter(1, 2);
  EXPECT_SET(block(r, {noteOn(2, 60, 0), noteOn(3, 72, 1)}), ({0, 1}));
  EXPECT_SET(block(r, {noteOn(4, 61, 20)}), ({0, 1}));          // one voice retriggered (a record), the other held
  const int stolen = r.newestVoice(0);                          // voices[] index 1 or 2
  REQUIRE(stolen == 1 || stolen == 2);
  const int stolenChannel = stolen == 1 ? 2 : 3, keptChannel = stolen == 1 ? 3 : 2;
  const uint32_t stolenVoice = (uint32_t)stolen - 1, keptVoice = 1u - stolenVoice;
  EXPECT_SET(block(r, {noteOff(stolenChannel, 0, 2)}), ({0, 1}));  // that channel owns no voice any more: no record, both held
  REQUIRE(r.dirtyLaneCount() == 0);
  EXPECT_SET(block(r, {noteOff(keptChannel, 0, 2)}), ({0, 1}));    // the kept voice's note-off record; the stolen one held
  EXPECT_SET(block(r, {}), ({stolenVoice}));
  EXPECT_SET(block(r, {noteOff(4, 61, 9)}), ({stolenVoice}));
  EXPECT_SET(block(r, {}), ({}));
  (void)keptVoice;
}

// poly 5, G = 8: lanes 0 (main), 1..5 (voices), 6 and 7 (padding); all-notes-off; the second instrument's lanes start at 8
static void fiveVoicesAndAllNotesOff()
{
  EventRouter r = mpeRouter(2, 5);
  REQUIRE(r.group() == 8 && r.lanes() == 16);
  // instrument 1's first event: awake records to lanes 8..13 - its main lane and its five voices, neither padding lane
  EXPECT_SET(block(r, {noteOn(2, 60, 3)}, 1, 1), ({5, 6, 7, 8, 9}));
  REQUIRE(r.dirtyLaneCount() == 6);
  EXPECT_SET(block(r, {noteOn(3, 62, 0), noteOn(4, 65, 70)}, 2, 1), ({5, 6, 7}));
  EXPECT_SET(block(r, {}), ({5, 6, 7}));
  EXPECT_SET(block(r, {bend(1, 0, 0.3f)}, 1, 1), ({5, 6, 7}));  // the main voice's bend changes their pitch rows: they are in the set as held
  // all notes off (controller 123 on channel 1): a note-off record for the main voice and every voice; nobody held after it
  EXPECT_SET(block(r, {allNotesOff(10)}, 1, 1), ({5, 6, 7, 8, 9}));
  REQUIRE(r.dirtyLaneCount() == 6);
  EXPECT_SET(block(r, {}), ({}));
  EXPECT_SET(block(r, {noteOn(2, 50, 0)}, 1, 0), ({0, 1, 2, 3, 4}));  // instrument 0 wakes
  // instrument 1 again: one voice with a record (the allocator's next free voice, the fourth), instrument 0's held voice beside it
  EXPECT_SET(block(r, {noteOn(2, 51, 0)}, 1, 1), ({0, 8}));
  REQUIRE(r.dirtyLaneCount() == 1);
}

// a capacity too small: the size is reported, nothing is written; clear() empties the set; a protocol switch and back
static void capacityClearProtocol()
{
  EventRouter r = mpeRouter(2, 2);
  block(r, {noteOn(2, 60, 0), noteOn(3, 62, 1)}, 1, 1);
  uint32_t out[4] = {9, 9, 9, 9};
  size_t n = 77;
  REQUIRE(!r.soundingGraphVoices(out, 1, &n) && n == 2 && out[0] == 9 && out[1] == 9);
  REQUIRE(!r.soundingGraphVoices(nullptr, 0, &n) && n == 2);
  REQUIRE(r.soundingGraphVoices(out, 2, &n) && n == 2 && out[0] == 2 && out[1] == 3 && out[2] == 9);
  r.clear();
  EXPECT_SET(sounding(r), ({}));  // clear() resets the object: the routed launch's records go with the held voices
  EXPECT_SET(block(r, {}), ({}));
  // polyphony 16, G = 32: routed under MPE - lanes instrument * 32 + slot, far past the 6 x 16 voices' bitmap - every lane comes back
  // as a voice below 96
  EventRouter p = mpeRouter(6, 16);
  for (size_t i = 0; i < 6; ++i) REQUIRE(p.addEvent(i, noteOn(2, 60, 0)) && p.addEvent(i, noteOn(3, 64, 1)));
  REQUIRE(p.route(1, 0) && p.dirtyLaneCount() == 6 * 17);
  p.clearEvents();
  Set all;
  for (uint32_t v = 0; v < 96; ++v) all.push_back(v);
  same(sounding(p), all, __LINE__);
  EXPECT_SET(block(p, {}), ({0, 1, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81}));
  // to MIDI (setProtocol is followed by clear): an empty set before and after the next route; the voice index is the MIDI lane
  p.setProtocol(false);
  p.clear();
  REQUIRE(p.dirtyLaneCount() == 0 && p.recordCount() == 0);
  EXPECT_SET(sounding(p), ({}));
  EXPECT_SET(block(p, {}), ({}));
  EXPECT_SET(block(p, {noteOn(1, 60, 0)}, 1, 5), ({80}));  // (awake records went out under MPE)
  EXPECT_SET(block(p, {noteOn(1, 62, 0)}, 1, 5), ({80, 81}));
  // ... and back to MPE: the same voices by another lane
  p.setProtocol(true);
  p.clear();
  EXPECT_SET(sounding(p), ({}));
  EXPECT_SET(block(p, {noteOn(2, 60, 0)}, 1, 5), ({80}));
  REQUIRE(p.dirtyLaneCount() == 1);
  EXPECT_SET(block(p, {bend(1, 0, 0.5f)}, 1, 5), ({80}));
}

// MIDI: every set above the MIDI router gives is soundingVoices' (sounding() compares them): notes, a steal, the pedal
static void midiEqualsSoundingVoices()
{
  EventRouter r(2, 2);
  EXPECT_SET(block(r, {noteOn(1, 60, 3)}, 1, 1), ({2, 3}));
  EXPECT_SET(block(r, {}), ({2}));
  EXPECT_SET(block(r, {noteOn(1, 72, 0), noteOn(1, 61, 5)}, 1, 1), ({2, 3}));
  EXPECT_SET(block(r, {bend(1, 0, 0.5f)}, 1, 1), ({2, 3}));     // MIDI: a bend goes to every voice
  EXPECT_SET(block(r, {event(MLGPU_EVENT_SUSTAIN_PEDAL, 1, 0, 0, 1.f), noteOff(1, 72, 9)}, 1, 1), ({2, 3}));
  EXPECT_SET(block(r, {allNotesOff(0)}, 1, 1), ({2, 3}));
  EXPECT_SET(block(r, {}), ({}));
  EXPECT_SET(block(r, {noteOn(1, 40, 0)}, 1, 0), ({0, 1}));
}

// routeAhead: the set is that of the launch to come, and stays while the launch is pending
static void routeAheadUnderMpe()
{
  EventRouter a = mpeRouter(2, 5);
  REQUIRE(a.addEvent(1, noteOn(2, 60, 3)) && a.addEvent(1, noteOn(3, 72, 70)));
  REQUIRE(a.routeAhead(2, 0) && a.aheadPending());
  EXPECT_SET(sounding(a), ({5, 6, 7, 8, 9}));
  REQUIRE(!a.addEvent(1, noteOn(4, 50, 0)) && !a.route(3, 0));
  EXPECT_SET(sounding(a), ({5, 6, 7, 8, 9}));
  REQUIRE(a.route(2, 0) && !a.aheadPending());
  a.clearEvents();
  EXPECT_SET(sounding(a), ({5, 6, 7, 8, 9}));
  EXPECT_SET(block(a, {}), ({5, 6}));
}

int main()
{
  noteOnLaterOffAndMainVoiceBends();
  stolenVoice();
  fiveVoicesAndAllNotesOff();
  capacityClearProtocol();
  midiEqualsSoundingVoices();
  routeAheadUnderMpe();
  if (failures) printf("%d FAILED\n", failures);
  else printf("All tests passed\n");
  return failures ? 1 : 0;
}
