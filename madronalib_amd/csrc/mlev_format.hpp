// mlev_format.hpp — what the host half and the device half of EventsToSignals agree on: the records the host router
// (events_router.cpp) produces, the per-voice and per-controller state words, the reference's fixed sizes. Plain C++ on
// <stdint.h> alone: read by the host compiler, by hipcc and by hiprtc (through mldsp_events.hpp in a generated graph kernel).
#pragma once
#include <stdint.h>

namespace mlev
{
constexpr int kMaxVoices = 16;        // EventsToSignals::kMaxVoices, MLEventsToSignals.h:48
constexpr int kMaxPhysicalKeys = 128;
constexpr int kNumControllers = 129;
constexpr int kChannelPressureControllerIdx = 128;

// ---- records ------------------------------------------------------------------------------------------------------
enum RecType : uint32_t
{
  REC_AWAKE = 0,      // the instrument received its first event: processVector stops being a no-op (:383-386)
  REC_NOTE_ON = 1,    // writeNoteEvent kNoteOn (:129-152):   v1 pitch, v2 velocity, flags bit0 doGlide bit1 doReset
  REC_NOTE_RETRIG = 2,
  REC_NOTE_OFF = 3,
  REC_SET_BEND = 4,   // currentPitchBend = v1 (:700-731)
  REC_SET_MOD = 5,
  REC_SET_X = 6,
  REC_SET_Y = 7,
  REC_SET_Z = 8,
  REC_SET_CHANNEL_PRESSURE = 9  // controllers[128].inputValue (MIDI mode, :620-626)
};
struct Rec
{
  uint32_t vec;    // DSPVector index inside this launch
  uint32_t typeTimeFlags;  // type | time << 8 | flags << 16
  float v1, v2;
};
// flags of a note record (typeTimeFlags >> 16): bit 0 doGlide, bit 1 doReset, bit 2 REC_FLAG_REWIND
constexpr uint32_t REC_FLAG_REWIND = 4u;

// a lane that has records in the coming launch: recs[first .. last). The kernels read it as a uint4 {x, y, z, w}.
struct LaneRange
{
  uint32_t lane, first, last, pad;
};

// ---- device state layout (uint32 words per voice, SoA [word][lanes]) --------------------------------------------------
enum : int
{
  S_AWAKE = 0, S_VELOCITY, S_PITCH, S_BEND, S_MOD, S_X, S_Y, S_Z, S_CHANPRESS, S_AGE, S_AGE_STEP, S_INHIBIT_GLIDE,
  S_PG_CURR, S_PG_STEP, S_PG_TARGET, S_PG_REMAINING, S_PG_PER_GLIDE, S_PG_DY,
  S_DRIFT_SEED, S_DRIFT_COUNTER, S_DRIFT_VALUE, S_DRIFT_NEXT,
  S_RECALC,  // Voice::recalcNeeded (:45-54): set by setSampleRate / setPitchGlideInSeconds, consumed by the next beginProcess
  S_GLIDES  // 7 glides follow: bend, mod, x, y, z, drift, channel pressure
};
constexpr int kNumGlides = 7;
constexpr int kGlideWords = 5 + 64;  // target, step, remaining, isUniform, uniformValue, currVec[64]
constexpr int kStateWords = S_GLIDES + kNumGlides * kGlideWords;

// ---- smoothed controller signals (SmoothedController, MLEventsToSignals.h:170-180, .cpp:264-281; read by a process function
// through AudioContext::getInputController, MLAudioContext.cpp:129) ----------------------------------------------------------
// One signal per instrument per WATCHED controller number (mlgpu_events_watch_controllers): one lane per (slot, instrument).
// Per DSPVector of an awake instrument: output = glide(inputValue), inputValue = the value of the last controller event of
// that vector or before (:744, :431-436). The records are (vector, value) pairs; lanes without records just keep gliding.
struct CtlRec
{
  uint32_t vecKind;  // vector index inside this launch << 1 | kind (0: inputValue = value, 1: the instrument woke up)
  float value;
};
enum : int { C_AWAKE = 0, C_INPUT, C_GLIDE, kCtlWords = C_GLIDE + kGlideWords };
}  // namespace mlev
