// events_router.cpp — the host event router of EventsToSignals (events_router.hpp). Line references (:NNN) are to the reference's
// source/app/MLEventsToSignals.cpp.
#include "events_router.hpp"

#include <stdlib.h>
#include <string.h>

#include <algorithm>

namespace mlev
{
namespace
{
bool soonerThan(const mlgpu_event& a, const mlgpu_event& b)  // :356-364
{
  if (a.time != b.time) return a.time < b.time;
  return a.type < b.type;
}
}  // namespace

struct Router  // one instrument, one vector
{
  EventRouter& er;
  Instrument& in;
  size_t instIdx;
  uint32_t vec;
  int keyIndex(const mlgpu_event& e) const { return er.mpe_ ? e.channel : e.source_idx; }  // getKeyIndex, :21-42
  void push(int voice, const Rec& r)
  {
    if (voice < 0 || voice > er.polyphony_) return;  // voices the device does not simulate (beyond the polyphony)
    if (voice < er.slotBase_) return;  // MIDI mode: the MPE main voice is not simulated (its signals are not used, :437-445)
    std::vector<Rec>& lr = er.laneRecs[instIdx * (size_t)er.group_ + (size_t)(voice - er.slotBase_)];
    if (lr.empty()) er.dirtyLanes.push_back((uint32_t)(instIdx * (size_t)er.group_ + (size_t)(voice - er.slotBase_)));
    lr.push_back(r);
  }
  // Voice::writeNoteEvent's host-visible effects (:115-216): creatorKeyIdx_ and currentVelocity
  void note(int v, const mlgpu_event& e, uint32_t type, int keyIdx, bool doGlide, bool doReset)
  {
    HostVoice& hv = in.voices[v];
    // writeNoteEvent ends with nextFrameToProcess = its own frame (:141, :204) - also when that lies BEFORE the frame the voice's
    // previous note event of this vector ended on. Events come sorted by time, so only an event the reference makes up itself can do
    // that: the note-off of a sustain-pedal release, built with Event's default time 0 (:833-836). The frames written so far are then
    // written again by what follows; the record says so (REC_FLAG_REWIND) and the kernels replay it (mlev::note_rewind).
    int dest = std::min(std::max((int)e.time, 0), MLGPU_FLOATS_PER_DSPVECTOR);
    if (type == MLGPU_EVENT_NOTE_RETRIG && dest == 0) dest = 1;
    const uint32_t rewind = (type == MLGPU_EVENT_NOTE_ON || type == MLGPU_EVENT_NOTE_RETRIG || type == MLGPU_EVENT_NOTE_OFF) && dest == 0 && hv.nextFrame > 0 ? (uint32_t)REC_FLAG_REWIND : 0u;
    if (type == MLGPU_EVENT_NOTE_ON || type == MLGPU_EVENT_NOTE_RETRIG)
    {
      hv.creatorKeyIdx = (size_t)keyIdx;
      hv.currentVelocity = e.value2;
      er.setHeld(instIdx, v, e.value2 != 0.f);
      hv.nextFrame = dest;
      push(v, makeRec(vec, type == MLGPU_EVENT_NOTE_ON ? REC_NOTE_ON : REC_NOTE_RETRIG, e.time, (doGlide ? 1u : 0u) | (doReset ? 2u : 0u) | rewind, e.value1, e.value2));
    }
    else if (type == MLGPU_EVENT_NOTE_OFF)
    {
      hv.creatorKeyIdx = 0;
      hv.currentVelocity = 0.f;
      er.setHeld(instIdx, v, false);
      hv.nextFrame = dest;
      push(v, makeRec(vec, REC_NOTE_OFF, e.time, rewind, 0.f, 0.f));
    }
    // kNoteSustain and everything else: no change (default:, :211-213)
  }
  size_t countHeldNotes() const  // :471-482
  {
    size_t n = 0;
    for (int i = 0; i < kMaxPhysicalKeys; ++i) n += (in.keys[i].state == 1);
    return n;
  }
  int findFreeVoice()  // :892-912
  {
    const int highest = er.polyphony_ + 1;
    int t = in.lastFreeVoiceFound;
    for (int i = 1; i < er.polyphony_ + 1; ++i)
    {
      t++;
      if (t >= highest) t = 1;
      if (in.voices[t].creatorKeyIdx == 0)
      {
        in.lastFreeVoiceFound = t;
        return t;
      }
    }
    return -1;
  }
  int findNearestVoice(int note)  // :922-937
  {
    int r = 0;
    size_t minDist = 128;
    for (int v = 1; v < er.polyphony_ + 1; ++v)
    {
      const size_t dist = (size_t)std::abs(note - (int)in.voices[v].creatorKeyIdx);
      if (dist < minDist)
      {
        minDist = dist;
        r = v;
      }
    }
    return r;
  }
  void noteOn(const mlgpu_event& e)  // :519-560
  {
    const int k = keyIndex(e) & (kMaxPhysicalKeys - 1);
    in.keys[k].state = 1;
    in.keys[k].noteOnIndex = in.currentNoteOnIndex++;
    in.keys[k].pitch = e.value1;
    if (er.unison)
    {
      const bool firstNote = (countHeldNotes() == 1);
      for (int v = 1; v < er.polyphony_ + 1; ++v) note(v, e, MLGPU_EVENT_NOTE_ON, k, !firstNote, firstNote);
    }
    else
    {
      int v = findFreeVoice();
      if (v >= 1) note(v, e, MLGPU_EVENT_NOTE_ON, k, true, true);
      else
      {
        v = findNearestVoice(e.source_idx);  // findVoiceToSteal, :914-918
        note(v, e, MLGPU_EVENT_NOTE_RETRIG, k, true, true);
      }
      in.newestVoice = v;
    }
  }
  void noteOff(const mlgpu_event& e)  // :562-632
  {
    const int k = keyIndex(e) & (kMaxPhysicalKeys - 1);
    in.keys[k].state = in.sustainPedal ? 2 : 0;
    if (er.unison)
    {
      if (countHeldNotes() == 0)
      {
        for (int v = 1; v < er.polyphony_ + 1; ++v) note(v, e, MLGPU_EVENT_NOTE_OFF, 0, true, true);
      }
      else if ((size_t)k == in.voices[1].creatorKeyIdx)
      {
        mlgpu_event f = e;  // change note without retriggering the envelope, keeping the current velocity
        f.value2 = in.voices[1].currentVelocity;
        uint32_t maxIdx = 0, mostRecent = 0;
        for (int i = 0; i < kMaxPhysicalKeys; ++i)
          if (in.keys[i].state == 1 && in.keys[i].noteOnIndex > maxIdx)
          {
            maxIdx = in.keys[i].noteOnIndex;
            mostRecent = (uint32_t)i;
          }
        f.value1 = in.keys[mostRecent].pitch;
        for (int v = 1; v < er.polyphony_ + 1; ++v) note(v, f, MLGPU_EVENT_NOTE_ON, (int)mostRecent, true, true);
      }
    }
    else if (!in.sustainPedal)
    {
      for (int v = 1; v < er.polyphony_ + 1; ++v)
        if (in.voices[v].creatorKeyIdx == (size_t)k) note(v, e, MLGPU_EVENT_NOTE_OFF, k, true, true);
    }
  }
  void setAll(uint32_t rec, float val)
  {
    for (int v = 1; v < er.polyphony_ + 1; ++v) push(v, makeRec(vec, rec, 0, 0, val, 0.f));
  }
  void setMatching(uint32_t rec, int channel, float val)
  {
    for (int v = 1; v < er.polyphony_ + 1; ++v)
      if (in.voices[v].creatorKeyIdx == (size_t)channel) push(v, makeRec(vec, rec, 0, 0, val, 0.f));
  }
  void setControllerInput(size_t ctrl, float val)  // controllers[ctrl].inputValue = val (:650, :744)
  {
    if (in.ctlInput.empty()) in.ctlInput.assign(kNumControllers, 0.f);  // kept from the first controller event on, watched or not
    in.ctlInput[ctrl] = val;
    if (er.slotOf[ctrl] >= 0) er.pushCtl(instIdx, er.slotOf[ctrl], vec, 0u, val);
  }
  void controller(const mlgpu_event& e)  // :735-822
  {
    const float val = e.value1;
    const size_t ctrl = std::min((size_t)e.source_idx, (size_t)kNumControllers - 1);
    setControllerInput(ctrl, val);
    if (ctrl == kChannelPressureControllerIdx)  // controllers[128].inputValue is what MIDI channel pressure writes too
      for (int v = 0; v < er.polyphony_ + 1; ++v) push(v, makeRec(vec, REC_SET_CHANNEL_PRESSURE, 0, 0, val, 0.f));
    if (ctrl == 120) return;  // "all sound off" clears the event buffer it is iterating in the reference (:749-755): not reproduced
    if (ctrl == 123)
    {
      if (val == 0)  // all notes off, :757-769
        for (int v = 0; v < kMaxVoices + 1; ++v) note(v, e, MLGPU_EVENT_NOTE_OFF, 0, false, true);
      return;
    }
    for (int v = 1; v < er.polyphony_ + 1; ++v)
    {
      if (er.mpe_ && in.voices[v].creatorKeyIdx != (size_t)e.channel) continue;
      if ((int)ctrl == er.voiceModCC) push(v, makeRec(vec, REC_SET_MOD, 0, 0, val, 0.f));
      if (ctrl == 73) push(v, makeRec(vec, REC_SET_X, 0, 0, val, 0.f));
      else if (ctrl == 74) push(v, makeRec(vec, REC_SET_Y, 0, 0, val, 0.f));
    }
  }
  void process(const mlgpu_event& e)  // processEvent, :485-515
  {
    switch (e.type)
    {
      case MLGPU_EVENT_NOTE_ON: noteOn(e); break;
      case MLGPU_EVENT_NOTE_OFF: noteOff(e); break;
      case MLGPU_EVENT_CONTROLLER: controller(e); break;
      case MLGPU_EVENT_PITCH_BEND:  // :700-731
        if (!er.mpe_) setAll(REC_SET_BEND, e.value1);
        else if (e.channel == 1) push(0, makeRec(vec, REC_SET_BEND, 0, 0, e.value1, 0.f));
        else if (e.channel != 0) setMatching(REC_SET_BEND, e.channel, e.value1);
        break;
      case MLGPU_EVENT_NOTE_PRESSURE:  // :676-698: per-key pressure in MIDI mode, ignored in MPE mode
        if (!er.mpe_) setMatching(REC_SET_Z, e.source_idx, e.value1);
        break;
      case MLGPU_EVENT_CHANNEL_PRESSURE:  // :637-674
        if (!er.mpe_)
        {
          setControllerInput(kChannelPressureControllerIdx, e.value1);
          for (int v = 0; v < er.polyphony_ + 1; ++v) push(v, makeRec(vec, REC_SET_CHANNEL_PRESSURE, 0, 0, e.value1, 0.f));
        }
        else if (e.channel == 1) push(0, makeRec(vec, REC_SET_Z, 0, 0, e.value1, 0.f));
        else if (e.channel != 0) setMatching(REC_SET_Z, e.channel, e.value1);
        break;
      case MLGPU_EVENT_SUSTAIN_PEDAL:  // :824-842
        in.sustainPedal = (e.value1 > 0.5f);
        if (!in.sustainPedal)
          for (int i = 1; i < er.polyphony_ + 1; ++i)
            if (in.keys[in.voices[i].creatorKeyIdx & (kMaxPhysicalKeys - 1)].state == 2)
            {
              mlgpu_event off{};
              off.type = MLGPU_EVENT_NOTE_OFF;
              note(i, off, MLGPU_EVENT_NOTE_OFF, 0, true, true);
            }
        break;
      default: break;
    }
  }
};

EventRouter::EventRouter(size_t nInstruments, int polyphony) : inst(nInstruments), polyphony_(polyphony)
{
  int pow2 = 1;
  while (pow2 < polyphony + 1) pow2 <<= 1;
  laneRecs.resize(nInstruments * (size_t)pow2);
  held.assign((nInstruments * (size_t)polyphony + 63) / 64, 0);
  sounding.assign(held.size(), 0);
  unwatch();
  setProtocol(false);
  clear();  // setPolyphony calls clear() (:316-321)
}

void EventRouter::setProtocol(bool mpe)
{
  mpe_ = mpe;
  if (mpe_)
  {
    group_ = 1;
    while (group_ < polyphony_ + 1) group_ <<= 1;
    slotBase_ = 0;
  }
  else
  {
    group_ = polyphony_;
    slotBase_ = 1;
  }
}

void EventRouter::clear()
{
  for (Instrument& in : inst)
  {
    in.events.clear();
    for (HostVoice& v : in.voices) v = HostVoice();
    in.lastFreeVoiceFound = 0;
  }
  std::fill(held.begin(), held.end(), (uint64_t)0);
  ahead_ = false;
  // the routed launch goes with the rest: its lane indices are the protocol's that routed it (setProtocol is followed by clear), and
  // soundingVoices reads them
  for (uint32_t l : dirtyLanes) laneRecs[l].clear();
  dirtyLanes.clear();
  for (uint32_t l : ctlDirty) ctlLaneRecs[l].clear();
  ctlDirty.clear();
  nRecs = nCtlRecs = 0;
}

bool EventRouter::addEvent(size_t instrument, const mlgpu_event& e)
{
  if (ahead_) return false;
  Instrument& in = inst[instrument];
  in.awake = true;
  in.events.insert(std::lower_bound(in.events.begin(), in.events.end(), e, soonerThan), e);
  return true;
}

void EventRouter::clearEvents()
{
  for (Instrument& in : inst) in.events.clear();
}

void EventRouter::unwatch()
{
  watched_.clear();
  ctlLaneRecs.clear();
  ctlDirty.clear();
  nCtlRecs = 0;
  for (int& x : slotOf) x = -1;
}

void EventRouter::watch(const int* numbers, int n)
{
  unwatch();
  watched_.assign(numbers, numbers + n);
  for (int i = 0; i < n; ++i) slotOf[numbers[i]] = i;
  ctlLaneRecs.resize(ctlLanes());
}

bool EventRouter::routeAhead(size_t nVectors, int startOffset)
{
  if (ahead_) return false;
  route(nVectors, startOffset);
  ahead_ = true;
  aheadVectors = nVectors;
  aheadOffset = startOffset;
  return true;
}

bool EventRouter::soundingVoices(uint32_t* voices, size_t capacity, size_t* n) const
{
  *n = 0;
  if (mpe_) return false;
  sounding = held;  // (same size: no allocation)
  const size_t nVoices = inst.size() * (size_t)polyphony_;  // (MIDI: a lane is a voice index; nothing else is ever set)
  for (uint32_t l : dirtyLanes)
    if (l < nVoices) sounding[l >> 6] |= (uint64_t)1 << (l & 63);
  size_t count = 0;
  for (uint64_t w : sounding) count += (size_t)__builtin_popcountll(w);
  *n = count;
  if (count > capacity) return false;
  for (size_t i = 0; i < sounding.size(); ++i)
    for (uint64_t w = sounding[i]; w; w &= w - 1) *voices++ = (uint32_t)(i * 64 + (size_t)__builtin_ctzll(w));
  return true;
}

bool EventRouter::soundingGraphVoices(uint32_t* voices, size_t capacity, size_t* n) const
{
  *n = 0;
  sounding = held;  // (same size: no allocation; held goes by voice index in both protocols - setHeld)
  for (uint32_t l : dirtyLanes)
  {
    const size_t instrument = (size_t)l / (size_t)group_;
    const int slot = (int)((size_t)l % (size_t)group_) + slotBase_;  // voices[] index: 0 the MPE main voice, above polyphony the padding
    if (slot < 1 || slot > polyphony_ || instrument >= inst.size()) continue;
    const size_t v = instrument * (size_t)polyphony_ + (size_t)(slot - 1);
    sounding[v >> 6] |= (uint64_t)1 << (v & 63);
  }
  size_t count = 0;
  for (uint64_t w : sounding) count += (size_t)__builtin_popcountll(w);
  *n = count;
  if (count > capacity) return false;
  for (size_t i = 0; i < sounding.size(); ++i)
    for (uint64_t w = sounding[i]; w; w &= w - 1) *voices++ = (uint32_t)(i * 64 + (size_t)__builtin_ctzll(w));
  return true;
}

bool EventRouter::route(size_t nVectors, int startOffset)
{
  if (ahead_)  // routed already: the records stand as routeAhead left them
  {
    if (!aheadIs(nVectors, startOffset)) return false;
    ahead_ = false;
    return true;
  }
  for (uint32_t l : dirtyLanes) laneRecs[l].clear();
  dirtyLanes.clear();
  for (uint32_t l : ctlDirty) ctlLaneRecs[l].clear();
  ctlDirty.clear();
  for (size_t i = 0; i < inst.size(); ++i)
  {
    Instrument& in = inst[i];
    if (!in.awake) continue;
    if (in.events.empty() && in.awakeSent) continue;  // nothing to route: the voices just keep gliding on the device
    for (size_t t = 0; t < nVectors; ++t)
    {
      Router r{*this, in, i, (uint32_t)t};
      for (int v = 0; v < kMaxVoices + 1; ++v) in.voices[v].nextFrame = 0;
      if (!in.awakeSent)
      {
        for (int v = 0; v < polyphony_ + 1; ++v) r.push(v, makeRec((uint32_t)t, REC_AWAKE, 0, 0, 0.f, 0.f));
        for (size_t sl = 0; sl < watched_.size(); ++sl) pushCtl(i, (int)sl, (uint32_t)t, 1u, 0.f);
        in.awakeSent = true;
      }
      const int start = startOffset + (int)t * MLGPU_FLOATS_PER_DSPVECTOR, end = start + MLGPU_FLOATS_PER_DSPVECTOR;
      for (const mlgpu_event& evt : in.events)
        if (evt.time >= start && evt.time < end)
        {
          mlgpu_event local = evt;
          local.time -= start;
          r.process(local);
        }
    }
  }
  std::sort(dirtyLanes.begin(), dirtyLanes.end());
  std::sort(ctlDirty.begin(), ctlDirty.end());
  nRecs = nCtlRecs = 0;
  for (uint32_t l : dirtyLanes) nRecs += laneRecs[l].size();
  for (uint32_t l : ctlDirty) nCtlRecs += ctlLaneRecs[l].size();
  return true;
}

void EventRouter::pack(Rec* dst, LaneRange* lanes) const
{
  size_t n = 0;
  for (uint32_t l : dirtyLanes)
  {
    const std::vector<Rec>& lr = laneRecs[l];
    memcpy(dst + n, lr.data(), sizeof(Rec) * lr.size());
    *lanes++ = LaneRange{l, (uint32_t)n, (uint32_t)(n + lr.size()), 0u};
    n += lr.size();
  }
}

void EventRouter::packControllers(CtlRec* dst, uint32_t* recStart) const
{
  size_t next = 0, n = 0;
  for (uint32_t l : ctlDirty)
  {
    for (; next <= l; ++next) recStart[next] = (uint32_t)n;
    const std::vector<CtlRec>& lr = ctlLaneRecs[l];
    memcpy(dst + n, lr.data(), sizeof(CtlRec) * lr.size());
    n += lr.size();
  }
  for (; next <= ctlLanes(); ++next) recStart[next] = (uint32_t)n;
}

// the state of freshly constructed / reset voices (EventsToSignals ctor :290-305, Voice::reset :58-84)
void EventRouter::initialVoiceState(std::vector<uint32_t>& st) const
{
  const size_t lanes = this->lanes();
  st.assign((size_t)kStateWords * lanes, 0u);
  auto W = [&](int word, size_t lane) -> uint32_t& { return st[(size_t)word * lanes + lane]; };
  const uint32_t minusOne = 0xFFFFFFFFu;
  for (size_t lane = 0; lane < lanes; ++lane)
  {
    const int slot = (int)(lane % (size_t)group_) + slotBase_;
    W(S_PG_REMAINING, lane) = minusOne;       // SampleAccurateLinearGlide defaults, MLDSPGens.h:519-524
    W(S_PG_PER_GLIDE, lane) = 32;
    const float dy = 1.f / 32;
    memcpy(&W(S_PG_DY, lane), &dy, 4);
    W(S_DRIFT_SEED, lane) = (uint32_t)(slot * 232);  // driftSource.seed_ = voiceIndex * 232, :60
    W(S_RECALC, lane) = 1u;
    for (int gl = 0; gl < kNumGlides; ++gl)
    {
      const int base = S_GLIDES + gl * kGlideWords;
      // reset() calls setValue(0) on bend / mod / x / y / z: remaining = 0; the drift and controller glides are
      // default-constructed: remaining = -1 (MLDSPGens.h:441)
      W(base + 2, lane) = (gl <= 4) ? 0u : minusOne;
      W(base + 3, lane) = 1u;  // mCurrVec is all zeros: uniform
    }
  }
}

// A smoother that starts being watched now starts settled on its controller's current value (the reference's has been
// running all along: the same thing 20 ms after the controller last moved); an instrument that has not seen an event yet
// is asleep and gives zeros (:386).
void EventRouter::initialControllerState(std::vector<uint32_t>& st) const
{
  const size_t lanes = ctlLanes();
  st.assign((size_t)kCtlWords * lanes, 0u);
  auto W = [&](int word, size_t lane) -> uint32_t& { return st[(size_t)word * lanes + lane]; };
  for (size_t sl = 0; sl < watched_.size(); ++sl)
    for (size_t i = 0; i < inst.size(); ++i)
    {
      const size_t lane = sl * inst.size() + i;
      const float v = inst[i].ctlInput.empty() ? 0.f : inst[i].ctlInput[(size_t)watched_[sl]];
      uint32_t bits;
      memcpy(&bits, &v, 4);
      W(C_AWAKE, lane) = inst[i].awakeSent ? 1u : 0u;
      W(C_INPUT, lane) = bits;
      W(C_GLIDE + 0, lane) = bits;         // target
      W(C_GLIDE + 2, lane) = 0xFFFFFFFFu;  // remaining = -1: holding (MLDSPGens.h:441)
      W(C_GLIDE + 3, lane) = 1u;           // mCurrVec is one value
      W(C_GLIDE + 4, lane) = bits;
    }
}
}  // namespace mlev
