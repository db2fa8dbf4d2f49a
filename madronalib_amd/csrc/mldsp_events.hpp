// mldsp_events.hpp — the device side of EventsToSignals (source/app/MLEventsToSignals.{h,cpp}) shared by the events kernel
// (events.hip: all 8 rows into HBM) and the run-time fused graph kernels (graph.hip: pitch and gate as source nodes of a voice
// graph, never written to memory): the kernels' arguments (the record format and the state layout are mlev_format.hpp), LinearGlide
// with its 64 slots, note_frame - one frame of a vector that holds note records - and the two objects of a voice kernel: CtlVoiceOf<MPE>,
// the control records of e2s_ctl_kernel expanded to the pitch and gate rows, one quad of frames at a time, and CtlRowsOf<MASK, MPE>,
// which reads the rows vox, z, x, y and mod that the control kernel makes for a graph that has them as source nodes. Each is one
// definition with two instances: CtlVoice and CtlRows<MASK> (MPE = false) for an events object in the MIDI protocol, a voice's own
// lane; CtlVoiceMpe and CtlRowsMpe<MASK> (MPE = true; mlgpu_graph_enable_mpe_events) for an events object in either protocol, a voice's
// lane and its instrument's main lane.
#pragma once
#include "mlgpu_device_args.hpp"
#include "mldsp_math.hpp"
#include "mldsp_procs.hpp"  // Proc<MLGPU_PROC_SAMPLE_ACCURATE_LINEAR_GLIDE>: the pitch glide
#include "mlev_format.hpp"  // the records, the state words: what the host router shares with this file

namespace mlev
{
using namespace mldev;

struct E2SArgs
{
  uint32_t* state;            // [kStateWords][lanes]
  const Rec* recs;            // all records of this launch, grouped by lane, time-ordered inside a lane
  uint2* recRange;            // [lanes]: a lane's records of this launch are recs[x .. y); a kernel that read them writes {0, 0} back
  SignalView out[8];          // pitch, gate, vox, z, x, y, mod, elapsed time: V = instruments * polyphony voices
  size_t lanes, T;
  int group, polyphony, slotBase;  // lane = instrument * group + (voice slot - slotBase)
  uint32_t rowMask;                // rows that are computed (mlgpu_events_set_wanted_rows); bit r = row r of `out`
  uint32_t flags;                  // MLGPU_KFLAG_*
  E2SSettings s;
};

// LinearGlide (MLDSPGens.h:433-515) with one shortcut that does not change results: between glides mCurrVec is a
// broadcast of one value, kept in a register instead of 64 words of HBM. `st` is this glide's first word for this lane
// (stride = lanes); it is passed in instead of stored to keep the register count of seven glides down.
struct Glide
{
  float target, step, uniformValue, startValue;
  int32_t remaining;
  int modeFlags;  // bits 0-1: mode (0 hold, 1 end, 2 start, 3 continue); bit 2: mCurrVec is uniform
  MLD bool isUniform() const { return (modeFlags & 4) != 0; }
  MLD int mode() const { return modeFlags & 3; }
  MLD void load(const uint32_t* st, size_t stride)
  {
    target = u2f(st[0]);
    step = u2f(st[stride]);
    remaining = (int32_t)st[2 * stride];
    modeFlags = st[3 * stride] ? 4 : 0;
    uniformValue = u2f(st[4 * stride]);
    startValue = 0.f;
  }
  MLD void store(uint32_t* st, size_t stride) const
  {
    st[0] = f2u(target);
    st[stride] = f2u(step);
    st[2 * stride] = (uint32_t)remaining;
    st[3 * stride] = isUniform() ? 1u : 0u;
    st[4 * stride] = f2u(uniformValue);
  }
  // beginVector for a caller that knows what mCurrVec[63] holds (it has the slots in registers): no memory access
  MLD void beginVectorKnown(float f, int32_t perGlide, float dyPerVector, float slot63)
  {
    beginVectorFrom(f, perGlide, dyPerVector, [=] { return slot63; });
  }
  MLD void beginVector(const uint32_t* st, size_t stride, float f, int32_t perGlide, float dyPerVector)
  {
    beginVectorFrom(f, perGlide, dyPerVector, [=] { return u2f(st[(size_t)(5 + 63) * stride]); });
  }
  // mCurrVec[n] is read and rewritten at sample n only, so a quad's four slots can be fetched together (and a quad ahead):
  // a load per sample in the middle of the load -> add -> store chain made the whole kernel wait out a memory round trip
  // per sample (62 us per DSPVector per wavefront).
  MLD bool readsCurrVec() const { return !isUniform() && (mode() == 0 || mode() == 3); }
  MLD void preload(const uint32_t* st, size_t stride, int q, float cur[4]) const
  {
    if (readsCurrVec())
    {
#pragma unroll
      for (int k = 0; k < 4; ++k) cur[k] = u2f(st[(size_t)(5 + 4 * q + k) * stride]);
    }
  }
  MLD float next(uint32_t* st, size_t stride, int n) const  // one sample at a time (the record-walking path)
  {
    return nextWith(st, stride, n, readsCurrVec() ? u2f(st[(size_t)(5 + n) * stride]) : 0.f);
  }
  MLD float nextWith(uint32_t* st, size_t stride, int n, float cur) const  // cur: what preload fetched for slot n
  {
    const int m = mode();
    if (m == 0) return isUniform() ? uniformValue : cur;
    if (m == 1) return target;
    float c;
    if (m == 2) c = startValue + ((float)(n + 1) * 0.015625f) * step;
    else c = (isUniform() ? uniformValue : cur) + step;
    st[(size_t)(5 + n) * stride] = f2u(c);
    return c;
  }
  MLD void endVector()
  {
    const int m = mode();
    if (m == 1)
    {
      modeFlags = 4;
      uniformValue = target;
    }
    else if (m >= 2)
      modeFlags = 0;
    else
      modeFlags &= 4;
  }

 private:
  // the start of a vector of LinearGlide::operator()(f) (:457-505), for both forms above. slot63() is asked only when a glide starts
  // from a non-uniform mCurrVec: a load of slot 63 on every vector would add memory traffic to every vector.
  template <class Slot63>
  MLD void beginVectorFrom(float f, int32_t perGlide, float dyPerVector, Slot63 slot63)
  {
    if (f != target)
    {
      target = f;
      remaining = perGlide;
    }
    int m;
    if (remaining < 0) m = 0;
    else if (remaining == 0)
    {
      m = 1;
      step = 0.f;
      remaining--;
    }
    else if (remaining == perGlide)
    {
      m = 2;
      startValue = isUniform() ? uniformValue : slot63();
      step = (target - startValue) * dyPerVector;
      remaining--;
    }
    else
    {
      m = 3;
      remaining--;
    }
    modeFlags = (modeFlags & 4) | m;
  }
};


// The sample-accurate pitch glide of a voice (SampleAccurateLinearGlide, MLDSPGens.h:517-590): its state words are S_PG_*, its
// nextSample is PitchGlide::next.
typedef Proc<MLGPU_PROC_SAMPLE_ACCURATE_LINEAR_GLIDE> PitchGlide;
MLD void set_pitch_glide_time(PitchGlide& pg, int32_t t)  // SampleAccurateLinearGlide::setGlideTimeInSamples, MLDSPGens.h:527-532
{
  pg.perGlide = t < 1 ? 1 : t;
  pg.dyPerSample = 1.0f / (float)pg.perGlide;
}

// The drift random walk of Voice::beginProcess (:115-126): once per DSPVector; at the change time a new value and the time of the change
// after it, two draws of RandomScalarSource::getFloat (MLDSPScalarMath.h:189-202).
MLD void drift_step(uint32_t& seed, int32_t& counter, int32_t& next, float& value, double sr)
{
  counter += MLGPU_FLOATS_PER_DSPVECTOR;
  if (counter >= next)
  {
    auto draw = [&] {
      seed = seed * 0x0019660Du + 0x3C6EF35Fu;
      return u2f(((seed >> 9) & 0x007FFFFFu) | 0x3F800000u) * 2.f - 3.f;
    };
    const float d = draw();
    const float nextTimeMul = 1.0f + abs_ps(draw());
    value = d;
    counter = 0;
    next = (int32_t)(sr * (double)nextTimeMul * (double)8.0f);
  }
}

// Voice::beginProcess (:75-126): the pitch glide's time if setSampleRate / setPitchGlideInSeconds asked for it (S_RECALC; the caller
// clears its flag after this), then the drift random walk
MLD void begin_process(const E2SSettings& s, bool needsRecalc, bool inhibit, PitchGlide& pg, uint32_t& seed, int32_t& counter, int32_t& next,
                       float& value)
{
  if (needsRecalc && !inhibit) set_pitch_glide_time(pg, s.pitchGlideSamples);
  drift_step(seed, counter, next, value, s.sr);
}

// A note record's own bookkeeping (writeNoteEvent, :115-216), done on the first frame that sees the record; flags = typeTimeFlags >> 16.
// A macro, not a function: a function is optimised on its own before it is inlined, and every form of it tried cost e2s_ctl_kernel 47-51
// and e2s_kernel 43-119 more instructions than this bookkeeping written in place.
#define MLEV_NOTE_START(type, flags, pitchGlideSamples, age, ageStep, inhibit, pg)  \
  do                                                                              \
  {                                                                               \
    if ((type) != REC_NOTE_OFF)                                                   \
    {                                                                             \
      if ((flags) & 2) (age) = 0; /* doReset */                                   \
      (ageStep) = 1;                                                              \
    }                                                                             \
    if ((type) == REC_NOTE_ON)                                                    \
    {                                                                             \
      (inhibit) = !((flags) & 1);                                                 \
      set_pitch_glide_time((pg), ((flags) & 1) ? (pitchGlideSamples) : 0);        \
    }                                                                             \
  } while (0)

// One frame of a vector that holds note records: writeNoteEvent (:115-216) and its neighbours walked frame by frame - the note
// records that end on frame n are applied, the gate, the sample-accurate pitch glide and the event age take their step. Shared by
// e2s_kernel (all rows) and e2s_ctl_kernel (pitch and gate for a voice graph). The caller's state comes in by reference; vTime is written
// when wantTime.
// The frames of a vector look at the same pending record again and again (a note that starts at frame 40 is read by frames 0..40):
// one record kept in registers, fetched again only when another index is asked for. Without it every frame is a memory round trip
// behind the stores of the frame before (loads and stores of a wavefront complete in issue order).
struct RecCache
{
  uint32_t idx{0xFFFFFFFFu};
  Rec r;
  MLD const Rec& at(const Rec* recs, uint32_t i)
  {
    if (i != idx)
    {
      r = recs[i];
      idx = i;
    }
    return r;
  }
};

MLD void note_frame(const Rec* recs, RecCache& cache, uint32_t& nc, uint32_t vend, int n, bool& preApplied, float& velocity, float& pitch, uint32_t& age, uint32_t& ageStep,
                    bool& inhibit, PitchGlide& pg, int32_t pitchGlideSamples, bool wantTime, double srD, float& vPitch, float& vGate, float& vTime)
{
  bool retrigFrame = false;
  while (nc < vend)
  {
    const Rec rc = cache.at(recs, nc);
    const uint32_t type = rc.typeTimeFlags & 0xFF;
    if (type != REC_NOTE_ON && type != REC_NOTE_RETRIG && type != REC_NOTE_OFF)
    {
      ++nc;
      continue;
    }
    int dest = (int)((rc.typeTimeFlags >> 8) & 0xFF);
    if (!preApplied)
    {
      MLEV_NOTE_START(type, rc.typeTimeFlags >> 16, pitchGlideSamples, age, ageStep, inhibit, pg);
      preApplied = true;
    }
    if (type == REC_NOTE_RETRIG)
    {
      if (dest == 0) dest = 1;                 // make room for the retrigger frame, :163-167
      if (n == dest - 1) retrigFrame = true;   // gate 0 for one frame, :171-175
    }
    if (dest == n)
    {
      if (type == REC_NOTE_OFF) velocity = 0.f;
      else
      {
        pitch = rc.v1;
        velocity = rc.v2;
      }
      ++nc;
      preApplied = false;
      continue;
    }
    break;
  }
  vGate = retrigFrame ? 0.f : velocity;
  vPitch = pg.next(pitch);
  age += ageStep;
  if (wantTime) vTime = (float)((double)age / srD);
  // A retrigger that lands on the frame where the previous note event of this voice ended (a note-on and a steal of
  // the same voice on one frame) makes the reference REWRITE frame dest - 1, which that previous event had already
  // written (:163-175): the glide is stepped and the event age counted once more, with the previous event's new
  // pitch. Look ahead for exactly that pattern and redo this frame the same way.
  while (nc < vend)
  {
    uint32_t pi = nc;
    while (pi < vend && ((cache.at(recs, pi).typeTimeFlags & 0xFF) < REC_NOTE_ON || (cache.at(recs, pi).typeTimeFlags & 0xFF) > REC_NOTE_OFF)) ++pi;
    if (pi >= vend) break;
    const Rec P = cache.at(recs, pi);
    const uint32_t ptype = P.typeTimeFlags & 0xFF;
    int pdest = (int)((P.typeTimeFlags >> 8) & 0xFF);
    if (ptype == REC_NOTE_RETRIG && pdest == 0) pdest = 1;
    if (pdest != n + 1) break;
    uint32_t ri = pi + 1;
    while (ri < vend && ((recs[ri].typeTimeFlags & 0xFF) < REC_NOTE_ON || (recs[ri].typeTimeFlags & 0xFF) > REC_NOTE_OFF)) ++ri;
    if (ri >= vend) break;
    const Rec R = recs[ri];
    int rdest = (int)((R.typeTimeFlags >> 8) & 0xFF);
    // (a retrigger on frame 0 makes room on frame 1 like every other, :163-167 - two steals of one voice on a vector's first frame
    // are this pattern too; without this line the second one's reset of the event age came a frame late: tools/events_soak.py)
    if ((R.typeTimeFlags & 0xFF) == REC_NOTE_RETRIG && rdest == 0) rdest = 1;
    if ((R.typeTimeFlags & 0xFF) != REC_NOTE_RETRIG || rdest != n + 1) break;
    if (!preApplied) MLEV_NOTE_START(ptype, P.typeTimeFlags >> 16, pitchGlideSamples, age, ageStep, inhibit, pg);  // P's own bookkeeping, if this frame is the first one it sees
    if (ptype == REC_NOTE_OFF) velocity = 0.f;  // P's new values
    else
    {
      pitch = P.v1;
      velocity = P.v2;
    }
    nc = ri;                                    // R is the current note record now, its bookkeeping done here
    if ((R.typeTimeFlags >> 16) & 2) age = 0;
    ageStep = 1;
    preApplied = true;
    vGate = 0.f;                                // the retrigger frame
    vPitch = pg.next(pitch);
    age += ageStep;
    if (wantTime) vTime = (float)((double)age / srD);
  }
}

// A vector that holds a note record flagged REC_FLAG_REWIND: a record on frame 0 for a voice whose earlier note records of the same
// vector ended later than that. Events reach the reference sorted by time, so only an event it makes up itself can be such a record: the
// note-off of a sustain-pedal release, built with Event's default time 0 (MLEventsToSignals.cpp:833-836). writeNoteEvent then sets
// nextFrameToProcess BACK to 0 (writeOutputFrames ends with `nextFrameToProcess = endFrame`, :141), and every frame the earlier records
// had written is written AGAIN by what follows - the pitch glide and the event age stepping on from where the first pass left them.
// note_rewind is that first pass, record by record as the reference walks them (values discarded, state kept):
//   note-on / note-off on frame d: the frames [next, d) step, the record's values apply, next = d           (:146-166, :185-193)
//   retrigger on frame d (>= 1): the frames [next, d - 1) step, then frame d - 1 - always, also when next == d - steps, next = d  (:169-183)
// up to the LAST flagged record of the vector; nc is left there and the caller walks the vector from frame 0 as usual.
// Found by tools/events_soak.py (8 of 2 100 random configurations: a note, then the pedal's release and the note's end in one DSPVector).
MLD void note_rewind(const Rec* recs, uint32_t& nc, uint32_t vend, float& velocity, float& pitch, uint32_t& age, uint32_t& ageStep, bool& inhibit,
                     PitchGlide& pg, int32_t pitchGlideSamples)
{
  uint32_t last = vend;
  for (uint32_t j = nc; j < vend; ++j)
  {
    const uint32_t w = recs[j].typeTimeFlags;
    if ((w & 0xFF) >= REC_NOTE_ON && (w & 0xFF) <= REC_NOTE_OFF && ((w >> 16) & REC_FLAG_REWIND)) last = j;
  }
  if (last == vend) return;
  int next = 0;
  for (; nc < last; ++nc)
  {
    const Rec rc = recs[nc];
    const uint32_t type = rc.typeTimeFlags & 0xFF;
    if (type != REC_NOTE_ON && type != REC_NOTE_RETRIG && type != REC_NOTE_OFF) continue;
    int dest = (int)((rc.typeTimeFlags >> 8) & 0xFF);
    MLEV_NOTE_START(type, rc.typeTimeFlags >> 16, pitchGlideSamples, age, ageStep, inhibit, pg);
    int steps;
    if (type == REC_NOTE_RETRIG)
    {
      if (dest == 0) dest = 1;
      steps = (dest - 1 > next ? dest - 1 - next : 0) + 1;
    }
    else
      steps = dest > next ? dest - next : 0;
    for (int i = 0; i < steps; ++i)
    {
      (void)pg.next(pitch);
      age += ageStep;
    }
    if (type == REC_NOTE_OFF) velocity = 0.f;
    else
    {
      pitch = rc.v1;
      velocity = rc.v2;
    }
    next = dest;
  }
}

// ---- EventsToSignals inside a fused voice graph ------------------------------------------------------------------------------
// The pitch and gate rows of one voice as source nodes of a graph kernel, never written to memory as signals. Round 5 splits the
// work by RATE (the round-4 form walked records, three glides and the drift random walk inside the voice kernel: 0.35 scalar and
// branch instructions per vector instruction, 134 spilled registers):
//   * e2s_ctl_kernel (events.hip) runs everything that happens once per DSPVector or once per note event - the record walk, the
//     drift random walk, the bend glide, the sample-accurate pitch glide, Voice::beginProcess / writeNoteEvent / endProcess
//     (:75-262) - and emits ONE CONTROL RECORD of kCtlRecWords words per voice and DSPVector: the pitch before drift, the held gate,
//     the drift glide's input of this vector, flags. A vector in which the pitch or the gate moves inside the vector (a note event,
//     a portamento in progress, a moving bend: a few per cent of all vectors) is flagged CF_ROWS and its 64 frames of pitch-before-
//     drift and gate are written to two side signals, which only the flagged lanes read back.
//   * the voice kernel (CtlVoiceOf below) expands a record to audio rate. The one per-sample state machine left to it is the drift
//     LinearGlide (8 s per glide, a new target every 8-16 s: moving most of the time in most wavefronts, its mCurrVec slots
//     read and rewritten every vector - 8 B per voice-sample, what reading the two rows used to cost): pitch[n] = P[n] +
//     (drift[n] * driftAmount) * kDriftScale, the reference's own operation order (:244, :247).
// Same operations on the same values as e2s_kernel (both use note_frame, note_rewind, PitchGlide and drift_step): a launch of either form
// leaves the state words the other expects.
enum : int
{
  C_PITCH = 0,   // float: the pitch glide at rest + the held bend term (vPitch after :244), the same for all 64 frames
  C_GATE,        // float: the held velocity
  C_DRIFT_IN,    // float: currentDriftValue, the drift glide's input for this vector (:241)
  C_FLAGS,       // CF_*
  kCtlRecWords
};
constexpr uint32_t CF_ON = 1u;    // the voice's instrument is awake: processVector is not a no-op (:383-386)
constexpr uint32_t CF_ROWS = 2u;  // the pitch before drift of this vector is in the side signal, frame by frame
constexpr uint32_t CF_GATE_ROW = 4u;  // ... and so is the gate (a vector with a note event)
// controller row r (3 z, 4 x, 5 y, 6 mod) of this vector is in its side signal, frame by frame: its glide moves inside the vector
constexpr uint32_t CF_ROW(int r) { return 8u << (r - 3); }
constexpr uint32_t kCtlRowsMask = 0x78u;  // the rows of a graph that are glides of e2s_ctl_kernel: bits 3..6
// row r's place among the rows of `mask` in the plane of held values (EventsDev::held)
constexpr int ctl_row_rank(uint32_t mask, int r) { return __builtin_popcount(mask & kCtlRowsMask & ((1u << r) - 1u)); }
constexpr int ctl_row_count(uint32_t mask) { return __builtin_popcount(mask & kCtlRowsMask); }

// Memory of this object is addressed the CDNA way: a 128-bit buffer descriptor in scalar registers (built from kernel arguments
// only, so provably wave-uniform), ONE 32-bit per-lane byte offset in a vector register, and a scalar offset per access
// (buffer_load_dword v, v_off, s[rsrc], s_off offen). With plain pointers the compiler keeps a 64-bit address per lane and access
// stream in vector registers - 59 such loads, 46 spilled registers in the instrument bank's voice kernel - and those are what a
// generated voice kernel is short of (128 per lane at four wavefronts per SIMD).
typedef __amdgpu_buffer_rsrc_t BufRsrc;
MLD BufRsrc lane_buffer(const void* uniformBase, size_t bytes)
{
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(uniformBase), (short)0, (int)(bytes > 0xFFFFFFFFull ? 0xFFFFFFFFull : bytes), 0x00020000);
}

// The parameter MPE of the two objects below. false (CtlVoice, CtlRows): an events object in the MIDI protocol, one lane per playing
// voice, lane == voice index. true (CtlVoiceMpe, CtlRowsMpe; mlgpu_graph_enable_mpe_events): an events object in either protocol.
// The protocol is data (E2SSettings::mpe, group, slotBase: a host switches it at run time), so a voice is no longer a lane:
//   lane of graph voice v = (v / polyphony) * group + (1 + v % polyphony) - slotBase,   its instrument's first lane = (v / polyphony) * group
// which is v itself under MIDI (group = polyphony, slotBase = 1) and skips the main voice's lane and the padding under MPE (group =
// nextpow2(polyphony + 1), slotBase = 0). Records, side signals, the held plane and the drift glide's words go by lane; vox stays
// v % polyphony. Under MPE (:447-458, e2s_kernel's withMain) the main voice's pitch, z, x, y and mod are added to every playing voice
// that is on: the main lane's record of a vector (e2s_ctl_mpe_kernel: its COMPLETE pitch row, drift term included, in C_PITCH or, where
// it moves, in rowP), its flags and its held words are fetched with the voice's own; its frames are read only where the main lane is
// flagged (asked wave-uniformly: several instruments share a wavefront, one may straddle two). All voices of an instrument read the
// same addresses: one fetch from cache. Nothing new is stored. What MPE adds is compiled into the `true` instance alone
// (`if constexpr (MPE)`) and there sits behind a scalar of EventsDev (`d.s.mpe`): the operations on a voice's own values are the same
// in both instances and under either protocol. (The members are laid out for the register allocator as much as for the reader: a
// generated kernel's code follows the order of the members its instance uses - profiles/event_structs_one_definition.md.)
template <bool MPE>
struct CtlVoiceOf
{
  typedef float f32x4e __attribute__((ext_vector_type(4)));
  // Per lane this object keeps the lane's byte offset, the drift glide's few words, the vector's pitch and gate and ONE set of four
  // words that holds, in turn, the coming quad's mCurrVec slots and - during a vector's last quad - the next vector's control record.
  EventsDev d;    // (uniform: scalar registers / kernel arguments)
  size_t T;
  BufRsrc glide;  // the drift glide's words [kGlideWords][lanes]
  uint32_t rowBytes;   // 4 * lanes: one word of every lane
  uint32_t laneBytes;  // 4 * the voice's lane
  uint32_t mainBytes;  // 4 * its instrument's main lane (this and the other words of the main voice: the MPE instance's alone)
  Glide gd;
  float P, gate;
  bool on, rows, gateRow, moving, fetch, ramp;
  bool anyRows, anyRamp, anyOff, anyFetch;  // wave-uniform
  float nd[4];
  float mP, nmP;       // the main voice's held pitch of this vector / of the next one
  uint32_t nmF;        // ... and the next one's flags
  bool mRows, anyMainRows;  // the main voice's pitch of this vector is in rowP; (wave-uniform) ... for some lane

  MLD uint32_t glideWord(int w) const { return __builtin_amdgcn_raw_buffer_load_b32(glide, (int)laneBytes, (int)((uint32_t)w * rowBytes), 0); }
  MLD void setGlideWord(int w, uint32_t x) const { __builtin_amdgcn_raw_buffer_store_b32(x, glide, (int)laneBytes, (int)((uint32_t)w * rowBytes), 0); }
  MLD void fetchRecord(size_t t)  // into nd[]: C_PITCH, C_GATE, C_DRIFT_IN, C_FLAGS; MPE: the main lane's C_PITCH and C_FLAGS
  {
    const BufRsrc rec = lane_buffer(d.ctl + t * (size_t)kCtlRecWords * d.lanes, (size_t)kCtlRecWords * rowBytes);
#pragma unroll
    for (int k = 0; k < 4; ++k) nd[k] = u2f(__builtin_amdgcn_raw_buffer_load_b32(rec, (int)laneBytes, (int)((uint32_t)k * rowBytes), 0));
    if constexpr (MPE)
    {
      if (d.s.mpe)
      {
        nmP = u2f(__builtin_amdgcn_raw_buffer_load_b32(rec, (int)mainBytes, (int)((uint32_t)C_PITCH * rowBytes), 0));
        nmF = __builtin_amdgcn_raw_buffer_load_b32(rec, (int)mainBytes, (int)((uint32_t)C_FLAGS * rowBytes), 0);
      }
    }
  }
  MLD void load(const EventsDev& a, size_t voice, size_t nVectors)
  {
    d = a;
    T = nVectors;
    rowBytes = (uint32_t)d.lanes * 4u;
    if constexpr (MPE)
    {
      const uint32_t inst = (uint32_t)voice / (uint32_t)d.s.polyphony;  // (the one division of a launch)
      const uint32_t main = inst * (uint32_t)d.group;
      mainBytes = main * 4u;
      laneBytes = (main + 1u + ((uint32_t)voice - inst * (uint32_t)d.s.polyphony) - (uint32_t)d.slotBase) * 4u;
      mP = nmP = 0.f;
      nmF = 0u;
      mRows = anyMainRows = false;
    }
    else
      laneBytes = (uint32_t)voice * 4u;  // (no division)
    glide =lane_buffer(d.state + (size_t)(S_GLIDES + 5 * kGlideWords) * d.lanes, (size_t)kGlideWords * rowBytes);  // glide 5: drift
    gd.target = u2f(glideWord(0));
    gd.step = u2f(glideWord(1));
    gd.remaining = (int32_t)glideWord(2);
    gd.modeFlags = glideWord(3) ? 4 : 0;
    gd.uniformValue = u2f(glideWord(4));
    gd.startValue = 0.f;
    fetchRecord(0);
  }
  MLD void store() const
  {
    setGlideWord(0, f2u(gd.target));
    setGlideWord(1, f2u(gd.step));
    setGlideWord(2, (uint32_t)gd.remaining);
    setGlideWord(3, gd.isUniform() ? 1u : 0u);
    setGlideWord(4, f2u(gd.uniformValue));
  }

  MLD void begin_vector(size_t t)
  {
    (void)t;
    const uint32_t f = f2u(nd[C_FLAGS]);
    const float din = nd[C_DRIFT_IN];
    on = (f & CF_ON) != 0;
    rows = (f & CF_ROWS) != 0;
    gateRow = (f & CF_GATE_ROW) != 0;
    P = on ? nd[C_PITCH] : 0.f;
    gate = on ? nd[C_GATE] : 0.f;
    if constexpr (MPE)
    {
      if (d.s.mpe)
      {
        mP = nmP;  // (0 while the main voice is not on: e2s_ctl_mpe_kernel writes it so)
        mRows = (nmF & CF_ROWS) != 0;
        anyMainRows = __builtin_amdgcn_ballot_w64(mRows) != 0;
      }
    }
    // a glide that starts from a non-uniform mCurrVec reads its slot 63 - this lane's own store of the vector before (once per
    // 8-16 s and voice: asked wave-uniformly)
    float slot63 = 0.f;
    const bool starts = on && ((din != gd.target) || gd.remaining == d.s.driftGlideVectors) && !gd.isUniform();
    if (__builtin_amdgcn_ballot_w64(starts) != 0)
    {
      if (starts) slot63 = u2f(glideWord(5 + 63));
    }
    if (on) gd.beginVectorKnown(din, d.s.driftGlideVectors, d.s.driftGlideDy, slot63);
    const int m = gd.mode();  // (a lane that is not on keeps mode 0 from the end of its last vector)
    moving = on && m >= 2;
    ramp = on && m == 2;
    fetch = on && gd.readsCurrVec();
    const float hv = (m == 1) ? gd.target : gd.uniformValue;
    anyRows = __builtin_amdgcn_ballot_w64(rows) != 0;
    anyRamp = __builtin_amdgcn_ballot_w64(ramp) != 0;
    anyOff = __builtin_amdgcn_ballot_w64(!on) != 0;
    anyFetch = __builtin_amdgcn_ballot_w64(fetch) != 0;
    nd[0] = nd[1] = nd[2] = nd[3] = hv;
    if (anyFetch)
    {
      if (fetch)
      {
#pragma unroll
        for (int k = 0; k < 4; ++k) nd[k] = u2f(glideWord(5 + k));
      }
    }
  }

  MLD void quad(size_t t, int q, f32x4e& oPitch, f32x4e& oGate)
  {
    const float prev[4] = {nd[0], nd[1], nd[2], nd[3]};
    if (q < 15)
    {
      if (anyFetch)
      {
        if (fetch)
        {
#pragma unroll
          for (int k = 0; k < 4; ++k) nd[k] = u2f(glideWord(5 + 4 * q + 4 + k));
        }
      }
    }
    else if (t + 1 < T)
      fetchRecord(t + 1);
    f32x4e Pq = {P, P, P, P};
    oGate = f32x4e{gate, gate, gate, gate};
    if (anyRows)
    {
      if (rows)
      {
        const size_t at = (t * 16 + (size_t)q) * d.lanes + (size_t)(laneBytes >> 2);
        Pq = __builtin_nontemporal_load((const f32x4e*)d.rowP + at);
        if (gateRow) oGate = __builtin_nontemporal_load((const f32x4e*)d.rowG + at);
      }
    }
    // (the rare questions are asked once per quad, not once per sample: a wave-uniform branch is a scalar compare, a branch and a
    // possible fetch stall, and scalar issue is not hidden on this chip)
    float c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = prev[k] + gd.step;  // a continuing glide: mCurrVec[n] += step (LinearGlide, MLDSPGens.h:497-505)
    if (anyRamp)  // a glide's first vector ramps from its start value (:481-495); once per 8-16 s and voice
    {
#pragma unroll
      for (int k = 0; k < 4; ++k)
      {
        const float r = gd.startValue + ((float)(4 * q + k + 1) * 0.015625f) * gd.step;
        c[k] = ramp ? r : c[k];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
    {
      const float driftSig = moving ? c[k] : prev[k];
      oPitch[k] = Pq[k] + (driftSig * d.s.driftAmount) * 0.02f;  // kDriftScale, :247
    }
    if constexpr (MPE)
    {
      if (d.s.mpe)  // the main voice's pitch row, added to every playing voice that is on (:447-458)
      {
        f32x4e M = {mP, mP, mP, mP};
        if (anyMainRows)
        {
          if (mRows) M = *((const f32x4e*)d.rowP + ((t * 16 + (size_t)q) * d.lanes + (size_t)(mainBytes >> 2)));
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) oPitch[k] = on ? oPitch[k] + M[k] : oPitch[k];
      }
    }
    if (anyOff)  // voices of instruments that have not seen an event yet: processVector is a no-op, the rows are zero (:383-386)
    {
#pragma unroll
      for (int k = 0; k < 4; ++k) oPitch[k] = on ? oPitch[k] : 0.f;
    }
    if (moving)
    {
#pragma unroll
      for (int k = 0; k < 4; ++k) setGlideWord(5 + 4 * q + k, f2u(c[k]));
    }
  }

  MLD void end_vector()
  {
    if (on) gd.endVector();
  }
};
typedef CtlVoiceOf<false> CtlVoice;
typedef CtlVoiceOf<true> CtlVoiceMpe;

// The rows vox, z, x, y and mod (2..6) of one voice as source nodes of a graph kernel; MASK has bit r for each row r the graph reads.
// Unlike the drift glide these glides belong to e2s_ctl_kernel: it runs them for every lane in every call, so this object only READS -
// per vector one held value per row (EventsDev::held) and the vector's flags, and for a row whose glide moves inside the vector
// (CF_ROW(r): the ~15 vectors after a controller event) the 64 frames of its side signal. Nothing is stored, nothing is carried over
// from launch to launch: a voice that was off a voice list has the bits of one that never was. vox is a constant of the voice (:302).
// Memory is addressed as CtlVoice does: a buffer descriptor per plane and the lane's 32-bit byte offset; the side signals, read by
// the flagged lanes only, through a pointer made inside the rare branch.
//
// The reader is written for ONE lane, L: 0 is the voice's own lane, 1 its instrument's main lane, which the MPE instance reads as well
// and adds to the voice's rows where the voice is on. Its words are the [L] entries of the members below; the MIDI instance has L = 0
// alone. The side signals of the voice's own lane are read once and stream past the caches (nontemporal loads); the main lane's are
// read by every voice of its instrument and should stay in them (plain loads).
template <uint32_t MASK, bool MPE>
struct CtlRowsOf
{
  typedef float f32x4e __attribute__((ext_vector_type(4)));
  static constexpr int N = ctl_row_count(MASK);
  static constexpr int NA = N ? N : 1;
  static constexpr int LANES = MPE ? 2 : 1;
  EventsDev d;  // (uniform)
  size_t T;
  uint32_t rowBytes, laneBytes[LANES];  // 4 * lanes: one word of every lane; 4 * the lane
  float vox;
  // (in this order - the held values of all lanes, then the flags of all lanes, then `any` - the compiler allocates the registers of a
  // kernel: another order is another kernel)
  struct
  {
    float now[NA], next[NA];
  } held[LANES];  // the held values of this vector / of the next one (fetched during this vector's last quad)
  struct
  {
    uint32_t now, next;
  } flags[LANES];       // C_FLAGS of the two
  bool any[LANES][NA];  // wave-uniform: some lane has the row flagged in this vector

  template <int L>
  MLD void clearLane()
  {
    flags[L].now = flags[L].next = 0u;
#pragma unroll
    for (int k = 0; k < NA; ++k)
    {
      held[L].now[k] = held[L].next[k] = 0.f;
      any[L][k] = false;
    }
  }
  template <int L>
  MLD void fetchLane(size_t t)
  {
    const BufRsrc rec = lane_buffer(d.ctl + (t * (size_t)kCtlRecWords + (size_t)C_FLAGS) * d.lanes, rowBytes);
    flags[L].next = __builtin_amdgcn_raw_buffer_load_b32(rec, (int)laneBytes[L], 0, 0);
    const BufRsrc plane = lane_buffer(d.held + t * (size_t)N * d.lanes, (size_t)N * rowBytes);
#pragma unroll
    for (int k = 0; k < N; ++k) held[L].next[k] = u2f(__builtin_amdgcn_raw_buffer_load_b32(plane, (int)laneBytes[L], (int)((uint32_t)k * rowBytes), 0));
  }
  template <int L>
  MLD void beginLane()
  {
    flags[L].now = flags[L].next;
#pragma unroll
    for (int k = 0; k < N; ++k) held[L].now[k] = held[L].next[k];
#pragma unroll
    for (int r = 3; r <= 6; ++r)
      if ((MASK >> r) & 1u) any[L][ctl_row_rank(MASK, r)] = __builtin_amdgcn_ballot_w64((flags[L].now & CF_ROW(r)) != 0) != 0;
  }
  template <int L, int R>
  MLD f32x4e laneRow(size_t t, int q) const
  {
    constexpr int k = ctl_row_rank(MASK, R);
    f32x4e v = {held[L].now[k], held[L].now[k], held[L].now[k], held[L].now[k]};
    if (any[L][k])
    {
      if (flags[L].now & CF_ROW(R))
      {
        const f32x4e* const at = (const f32x4e*)d.rowC[R - 3] + ((t * 16 + (size_t)q) * d.lanes + (size_t)(laneBytes[L] >> 2));
        if constexpr (L == 0) v = __builtin_nontemporal_load(at);
        else v = *at;
      }
    }
    return v;
  }

  MLD void fetch(size_t t)
  {
    if constexpr (N > 0)
    {
      fetchLane<0>(t);
      if constexpr (MPE)
      {
        if (d.s.mpe) fetchLane<1>(t);
      }
    }
  }
  MLD void load(const EventsDev& a, size_t voice, size_t nVectors)
  {
    d = a;
    T = nVectors;
    rowBytes = (uint32_t)d.lanes * 4u;
    if constexpr (MPE)
    {
      const uint32_t inst = (uint32_t)voice / (uint32_t)d.s.polyphony;
      const uint32_t slot0 = (uint32_t)voice - inst * (uint32_t)d.s.polyphony;
      const uint32_t main = inst * (uint32_t)d.group;
      laneBytes[1] = main * 4u;
      laneBytes[0] = (main + 1u + slot0 - (uint32_t)d.slotBase) * 4u;
      vox = (float)slot0;
    }
    else
    {
      laneBytes[0] = (uint32_t)voice * 4u;
      vox = (float)((uint32_t)voice % (uint32_t)d.s.polyphony);
    }
    clearLane<0>();
    if constexpr (MPE) clearLane<1>();
    fetch(0);
  }
  MLD void begin_vector(size_t t)
  {
    (void)t;
    if constexpr (N > 0)
    {
      beginLane<0>();
      if constexpr (MPE)
      {
        if (d.s.mpe) beginLane<1>();
      }
    }
  }
  MLD void quad(size_t t, int q)
  {
    if (q == 15 && t + 1 < T) fetch(t + 1);
  }
  template <int R>
  MLD f32x4e row(size_t t, int q) const
  {
    static_assert(R >= 2 && R <= 6 && ((MASK >> R) & 1u), "a row of this graph");
    if constexpr (R == 2) return f32x4e{vox, vox, vox, vox};
    else
    {
      f32x4e v = laneRow<0, R>(t, q);
      if constexpr (MPE)
      {
        if (d.s.mpe)  // the main voice's row, added where the voice is on (:447-458)
        {
          const f32x4e m = laneRow<1, R>(t, q);
          if (flags[0].now & CF_ON) v = v + m;
        }
      }
      return v;
    }
  }
};
template <uint32_t MASK>
using CtlRows = CtlRowsOf<MASK, false>;
template <uint32_t MASK>
using CtlRowsMpe = CtlRowsOf<MASK, true>;

}  // namespace mlev
