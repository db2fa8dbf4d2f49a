// events_router.hpp — the HOST half of EventsToSignals (source/app/MLEventsToSignals.{h,cpp}): key states, voice allocation and
// stealing, unison, the sustain pedal, the MIDI / MPE channel rules, controller inputs (processEvent & co, :445-870;
// findFreeVoice / findNearestVoice :892-935) for N independent instruments. Integer bookkeeping that never touches a device:
// plain C++, built and tested without any HIP header. A block's events go in, per-lane record lists in the format of
// mlev_format.hpp come out, packed straight into the caller's (pinned) upload buffers; events.hip is the caller.
//
// One instrument occupies `group` consecutive lanes: MIDI - one lane per playing voice (slotBase 1); MPE - nextpow2(polyphony + 1)
// lanes with the main voice (voices[0] in the reference) at lane 0 (slotBase 0).
#pragma once
#include <stddef.h>

#include <algorithm>
#include <vector>

#include "../../include/mlgpu.h"
#include "mlev_format.hpp"

namespace mlev
{
inline Rec makeRec(uint32_t vec, uint32_t type, int time, uint32_t flags, float v1, float v2)
{
  const uint32_t t = (uint32_t)std::min(std::max(time, 0), 64);  // destTime = clamp(e.time, 0, 64) (:121)
  return Rec{vec, type | (t << 8) | (flags << 16), v1, v2};
}

struct KeyState
{
  int state{0};  // 0 off, 1 on, 2 sustained
  float pitch{0.f};
  uint32_t noteOnIndex{0};
};
struct HostVoice
{
  size_t creatorKeyIdx{0};
  float currentVelocity{0.f};
  int nextFrame{0};  // Voice::nextFrameToProcess inside the vector being routed (0 at its start: beginProcess, :115)
};
struct Instrument
{
  std::vector<mlgpu_event> events;  // time-sorted (addEvent, :367-372)
  KeyState keys[kMaxPhysicalKeys];
  HostVoice voices[kMaxVoices + 1];
  int lastFreeVoiceFound{-1};
  int newestVoice{-1};
  bool sustainPedal{false};
  uint32_t currentNoteOnIndex{0};
  bool awake{false}, awakeSent{false};
  std::vector<float> ctlInput;  // controllers[n].inputValue (:744), from the first controller event on
};

class EventRouter
{
 public:
  EventRouter() { unwatch(); }
  EventRouter(size_t nInstruments, int polyphony);  // 1+ instruments, polyphony 1..kMaxVoices; MIDI protocol

  size_t instruments() const { return inst.size(); }
  int polyphony() const { return polyphony_; }
  int group() const { return group_; }
  int slotBase() const { return slotBase_; }
  bool mpe() const { return mpe_; }
  bool awakeSent(size_t instrument) const { return inst[instrument].awakeSent; }  // its awake records have gone out: they go out once
  size_t lanes() const { return inst.size() * (size_t)group_; }
  size_t maxLanes() const { return laneRecs.size(); }  // lanes() of the wider protocol (MPE)

  void setProtocol(bool mpe);  // the caller clears (setProtocol, :92-96)
  void setUnison(bool on) { unison = on; }
  void setModCC(int cc) { voiceModCC = cc; }
  void clear();  // EventsToSignals::clear, :330-340

  // addEvent, :367-372; instrument < instruments(). false, and nothing added: a launch routed ahead is pending (routeAhead)
  bool addEvent(size_t instrument, const mlgpu_event& e);
  void clearEvents();
  int newestVoice(size_t instrument) const { return inst[instrument].newestVoice; }  // voices[] index (1..polyphony), -1: none yet

  // watched controllers: slot i is controller numbers[i] (0..kNumControllers-1, no number twice); lane = slot * instruments + instrument
  void watch(const int* numbers, int n);
  void unwatch();
  const std::vector<int>& watched() const { return watched_; }
  size_t ctlLanes() const { return watched_.size() * inst.size(); }

  // Everything of processVector (:376-466) that happens on the host for nVectors DSPVectors starting at frame startOffset of the
  // event times: the block's events routed into per-lane records. Afterwards, until the next route():
  // false, and nothing consumed: a launch routed ahead is pending and these are not its values (with them: its records stay, the
  // launch is no longer pending).
  bool route(size_t nVectors, int startOffset);
  // route() now, for the launch to come: the host reads the records' consequences (soundingVoices) before that launch is made. Until
  // a route() with the same values has taken the records over, addEvent and a second routeAhead are refused (false, nothing changed).
  bool routeAhead(size_t nVectors, int startOffset);
  bool aheadPending() const { return ahead_; }
  bool aheadIs(size_t nVectors, int startOffset) const { return ahead_ && nVectors == aheadVectors && startOffset == aheadOffset; }
  size_t recordCount() const { return nRecs; }
  size_t dirtyLaneCount() const { return dirtyLanes.size(); }
  void pack(Rec* dst, LaneRange* lanes) const;  // recordCount() records grouped by lane, lanes ascending; dirtyLaneCount() ranges
  size_t ctlRecordCount() const { return nCtlRecs; }
  void packControllers(CtlRec* dst, uint32_t* recStart) const;  // ctlRecordCount() records; recStart[ctlLanes() + 1]
  // The voices that sound in the routed launch, ascending, as voice indices instrument * polyphony + voice (MIDI protocol: the lane):
  // every voice the launch holds a record for, and every voice whose held velocity is non-zero at the launch's end - so every voice
  // whose gate is non-zero anywhere in the launch. The held voices are a bitmap kept where a note writes a velocity; the query costs
  // the bitmap's words and the launch's lanes with records, not a walk over the voices. *n: the set's size, also when it is larger than
  // `capacity` (false then, and nothing written). MIDI protocol only (false under MPE with *n = 0).
  bool soundingVoices(uint32_t* voices, size_t capacity, size_t* n) const;
  // The same set in either protocol, as GRAPH voice indices instrument * polyphony + voice, ascending: `held` goes by voice index in
  // both protocols, and a lane with records is mapped back - instrument l / group, slot l % group + slotBase; a slot in 1..polyphony
  // is voice instrument * polyphony + slot - 1, slot 0 (the MPE main voice) and the padding lanes add nothing. Under MIDI exactly
  // soundingVoices' set. The same scratch bitmap, no allocation, the same rule for `capacity`.
  // The guarantee: every voice whose GATE row is non-zero anywhere in the routed launch is in the set - a gate rises by a note record
  // of the voice's own lane and stays up only while its velocity is held, and the gate row gets nothing added from the main voice.
  // What an MPE channel-1 event (bend, pressure, controllers 74 / 73 / mod on the main voice) means for the host: it is a record of
  // the main lane alone and adds no voice. It changes the pitch, z, x, y and mod rows of the instrument's voices that are ON: those
  // that are held are in the set already, those in a release tail are the host's tails - the host keeps listing a released voice
  // until its peak has died away, and while it does the voice reads the main voice's rows like any listed voice.
  bool soundingGraphVoices(uint32_t* voices, size_t capacity, size_t* n) const;

  void initialVoiceState(std::vector<uint32_t>& st) const;       // [kStateWords][lanes()]: freshly constructed / reset voices
  void initialControllerState(std::vector<uint32_t>& st) const;  // [kCtlWords][ctlLanes()]: smoothers settled on the current inputs

 private:
  friend struct Router;
  std::vector<Instrument> inst;
  int polyphony_{0}, group_{1}, slotBase_{1};
  bool mpe_{false}, unison{false};
  int voiceModCC{16};
  std::vector<std::vector<Rec>> laneRecs;  // per lane, this launch
  std::vector<uint32_t> dirtyLanes;        // lanes with records (most have none), ascending after route()
  std::vector<int> watched_;
  int slotOf[kNumControllers];
  std::vector<std::vector<CtlRec>> ctlLaneRecs;
  std::vector<uint32_t> ctlDirty;
  size_t nRecs{0}, nCtlRecs{0};
  bool ahead_{false};  // routeAhead's launch has not been taken over by route() yet
  size_t aheadVectors{0};
  int aheadOffset{0};
  std::vector<uint64_t> held;             // bit v: HostVoice::currentVelocity of voice index v is non-zero
  mutable std::vector<uint64_t> sounding;  // soundingVoices' scratch: held, and the lanes with records
  void setHeld(size_t instrument, int voice, bool on)  // voices[] index 1..polyphony
  {
    if (voice < 1 || voice > polyphony_) return;
    const size_t v = instrument * (size_t)polyphony_ + (size_t)(voice - 1);
    if (on) held[v >> 6] |= (uint64_t)1 << (v & 63);
    else held[v >> 6] &= ~((uint64_t)1 << (v & 63));
  }
  void pushCtl(size_t instrument, int slot, uint32_t vec, uint32_t kind, float value)
  {
    const size_t l = (size_t)slot * inst.size() + instrument;
    if (ctlLaneRecs[l].empty()) ctlDirty.push_back((uint32_t)l);
    ctlLaneRecs[l].push_back(CtlRec{(vec << 1) | kind, value});
  }
};
}  // namespace mlev
