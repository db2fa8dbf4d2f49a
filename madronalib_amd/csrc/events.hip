// events.hip — EventsToSignals (source/app/MLEventsToSignals.{h,cpp}) for N independent instruments.
//
// The reference turns a time-sorted list of performance events (note on/off, controllers, pitch bend, pressure,
// sustain pedal) into 8 control signals per voice — pitch, gate, vox, z, x, y, mod, elapsed time
// (VoiceOutputSignals, MLEventsToSignals.h:15-26) — one DSPVector at a time on the audio thread. Split here as
// SURVEY §8f-1 prescribes:
//   HOST   the event routing: key states, voice allocation and stealing, unison, sustain pedal, MIDI / MPE channel
//          rules (processEvent & co, MLEventsToSignals.cpp:445-870; findFreeVoice / findNearestVoice :892-935).
//          Integer bookkeeping on a handful of events per block; it produces, per voice, a short list of timed
//          records ("note on at frame 17 with pitch p, velocity v", "pitch bend is now b", ...). That program is
//          mlev::EventRouter (events_router.cpp, plain C++ without a HIP header); this file owns the device memory,
//          packs the router's records into pinned staging buffers and uploads them.
//   DEVICE everything per sample: Voice::beginProcess / writeNoteEvent / endProcess (:75-262) — the sample-accurate
//          pitch glide, event age -> seconds, five vector-rate glides, the drift random walk, channel pressure and
//          the MPE main-voice sums — one wavefront lane per voice, all state in HBM between launches only.
// Uploading the signals themselves would cost 8 x 256 B per voice per DSPVector; the records are a few bytes per event.
//
// One instrument occupies G = nextpow2(polyphony + 1) consecutive lanes: lane 0 is the MPE main voice (voices[0] in the
// reference), lanes 1..polyphony the playing voices, so the main voice's signals reach the others with one wave shuffle.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "mlgpu_internal.hpp"
#include "mldsp_math.hpp"
#include "mldsp_events.hpp"
#include "events_router.hpp"

using namespace mldev;
using namespace mlev;

namespace
{
// ROWS01: only the pitch and gate rows are wanted (what a Synth's voices usually read): an instance of the kernel without the controller
// rows, the voice-index row and the elapsed-time row. Those are half of the general loop's code and registers; without them the
// instance keeps its state in registers instead of scratch, and its loop has fewer memory round trips per DSPVector.
template <bool ROWS01>
__global__ __launch_bounds__(256, 4) void e2s_kernel(const E2SArgs aIn)
{
  E2SArgs a = aIn;
  if constexpr (ROWS01) a.rowMask &= 3u;
  apply_fp_mode(a.flags);
  // XCD-aware workgroup -> lane mapping (as the voice-bank kernels): every XCD writes one contiguous eighth of each row
  size_t blk = blockIdx.x;
  const size_t nbFull = (size_t)gridDim.x & ~(size_t)7;
  if (blk < nbFull) blk = (blk & 7) * (nbFull >> 3) + (blk >> 3);
  const size_t lane = blk * 256 + threadIdx.x;
  const bool live = lane < a.lanes;
  const size_t L = live ? lane : 0;
  const int slot = (int)(L % (size_t)a.group) + a.slotBase;  // 0 = MPE main voice (MPE mode only), 1..polyphony = playing voices
  const bool isVoice = live && slot >= 1 && slot <= a.polyphony;
  const bool active = live && slot <= a.polyphony;       // lanes beyond polyphony are padding
  const size_t outVoice = (L / (size_t)a.group) * (size_t)a.polyphony + (size_t)(slot > 0 ? slot - 1 : 0);
  uint32_t* S = a.state + L;  // reassigned before the final stores
  const size_t ln = a.lanes;
#define SW(i) S[(size_t)(i) * ln]

  bool awake = SW(S_AWAKE) != 0;
  float velocity = u2f(SW(S_VELOCITY)), pitch = u2f(SW(S_PITCH)), bend = u2f(SW(S_BEND)), mod = u2f(SW(S_MOD));
  float cx = u2f(SW(S_X)), cy = u2f(SW(S_Y)), cz = u2f(SW(S_Z)), chanPress = u2f(SW(S_CHANPRESS));
  uint32_t age = SW(S_AGE), ageStep = SW(S_AGE_STEP);
  bool inhibit = SW(S_INHIBIT_GLIDE) != 0, needsRecalc = SW(S_RECALC) != 0;
  PitchGlide pg;
  pg.curr = u2f(SW(S_PG_CURR)), pg.step = u2f(SW(S_PG_STEP)), pg.target = u2f(SW(S_PG_TARGET)), pg.dyPerSample = u2f(SW(S_PG_DY));
  pg.remaining = (int32_t)SW(S_PG_REMAINING), pg.perGlide = (int32_t)SW(S_PG_PER_GLIDE);
  uint32_t driftSeed = SW(S_DRIFT_SEED);
  int32_t driftCounter = (int32_t)SW(S_DRIFT_COUNTER), driftNext = (int32_t)SW(S_DRIFT_NEXT);
  float driftValue = u2f(SW(S_DRIFT_VALUE));
  // the seven glides stay in HBM between uses: each row loop loads the one or two it needs (5 words), so their
  // registers are not live everywhere
#define GS(i) (S + (size_t)(S_GLIDES + (i) * kGlideWords) * ln)

  const uint2 recRange = live ? a.recRange[L] : make_uint2(0u, 0u);  // this lane's records of this launch: [x, y)
  uint32_t cursor = recRange.x;
  const uint32_t recEnd = recRange.y;
  const float pitchBendScale = (a.s.mpe && slot != 0) ? a.s.mpePitchBendRange : a.s.pitchBendRange;  // :417-423
  const double srD = (double)(float)a.s.sr;  // samplesToSeconds(uint32_t, float sr), :13-19
  const unsigned mainLane = (unsigned)((threadIdx.x & 63) / (unsigned)a.group) * (unsigned)a.group;
  const bool wantTime = !ROWS01 && (a.rowMask & (1u << 7)) != 0;  // the elapsed-time row costs an f64 division per sample

  // ---- blocks of vectors in which nothing happens ------------------------------------------------------------------------------
  // The duration of a launch is the duration of its slowest wavefront, and memory operations of a wavefront complete in issue
  // order: every load behind a store waits for that store's acknowledgement (several microseconds while the chip writes rows at
  // its ceiling). The general vector loop below has a dozen such round trips per DSPVector - glide state, slots a quad at a
  // time, records - and a wavefront that carried a note event used to run it for all its vectors, ~40 us each, long after the
  // others were done (profiles/archive/r03_e2s_latency.txt). So: kBlock vectors at a time, where no lane of the wavefront has a record, the
  // bend and the wanted controllers are at rest, take this path - ONE round trip: the glide words and all 64 slots of the drift
  // glide (8 s per glide: always moving) are fetched together, the block is computed in time order in registers (the pitch glide may
  // be moving: it is stepped sample by sample as ever; what each vector does to the drift glide - hold / end / start / continue -
  // depends on the drift counter alone), rows are written as they come, the slots go back once. Same operations on the same
  // values as the general loop (drift_step, PitchGlide::next); the state variables are this kernel's own, so the two forms alternate freely.
  constexpr int kBlock = 4;
  typedef float f32x4b __attribute__((ext_vector_type(4)));
  for (size_t t = 0; t < a.T; ++t)
  {
    if (!a.s.mpe && t + kBlock <= a.T)
    {
      const bool onB = awake && active;
      bool ok = (cursor >= recEnd) || (a.recs[cursor].vec >= (uint32_t)(t + kBlock));
      float heldBend = 0.f, heldMod = 0.f, heldX = 0.f, heldY = 0.f, heldZ = 0.f;
      const float czEff = (velocity == 0.f) ? 0.f : cz;  // :238-241 with finalVelocity == velocity
      if (ok && onB)
      {
        auto rests = [&](int gi, float value, float& held) {  // glide gi holds `value` with a broadcast mCurrVec: its vectors change nothing
          Glide g;
          g.load(GS(gi), ln);
          held = g.uniformValue;
          return g.remaining < 0 && g.isUniform() && g.target == value;
        };
        ok = !needsRecalc && rests(0, bend, heldBend);
        if (!ROWS01 && (a.rowMask & (1u << 6))) ok = ok && rests(1, mod, heldMod);
        if (!ROWS01 && (a.rowMask & (1u << 4))) ok = ok && rests(2, cx, heldX);
        if (!ROWS01 && (a.rowMask & (1u << 5))) ok = ok && rests(3, cy, heldY);
        if (!ROWS01 && (a.rowMask & (1u << 3)))
        {
          float heldP = 0.f;
          ok = ok && rests(4, czEff, heldZ) && rests(6, chanPress, heldP);
          heldZ = heldZ + heldP;  // MIDI mode: z adds the smoothed channel pressure (:437-445)
        }
      }
      if (__builtin_amdgcn_ballot_w64(!ok) == 0)
      {
        uint32_t* gs = GS(5);
        Glide gd;
        gd.load(gs, ln);
        const bool slotsLive = onB && !gd.isUniform();  // mCurrVec is in memory as the block starts
        if (onB) cz = czEff;
        auto rowOfOne = [&](int row, float value) {  // one value per lane for the whole block
          const SignalView& sv = a.out[row];
          if ((ROWS01 && row > 1) || !((a.rowMask >> row) & 1u) || !sv.base || !isVoice) return;
          f32x4b* p = (f32x4b*)sv.base + t * sv.strideT + outVoice * sv.strideV;
          const f32x4b v = {value, value, value, value};
          for (int b = 0; b < kBlock; ++b, p += sv.strideT)
          {
            f32x4b* pq = p;
#pragma unroll 4
            for (int q = 0; q < 16; ++q, pq += sv.strideQ) __builtin_nontemporal_store(v, pq);
          }
        };
        rowOfOne(1, onB ? velocity : 0.f);
        rowOfOne(2, (float)(slot - 1));
        rowOfOne(3, onB ? heldZ : 0.f);
        rowOfOne(4, onB ? heldX : 0.f);
        rowOfOne(5, onB ? heldY : 0.f);
        rowOfOne(6, onB ? heldMod : 0.f);
        if (wantTime && a.out[7].base && isVoice)
        {
          const SignalView& sv = a.out[7];
          f32x4b* p = (f32x4b*)sv.base + t * sv.strideT + outVoice * sv.strideV;
          uint32_t ageNow = age;
          for (int b = 0; b < kBlock; ++b, p += sv.strideT)
          {
            f32x4b* pq = p;
            for (int q = 0; q < 16; ++q, pq += sv.strideQ)
            {
              f32x4b v;
#pragma unroll
              for (int k = 0; k < 4; ++k) v[k] = onB ? (float)((double)(ageNow + (uint32_t)(q * 4 + k + 1) * ageStep) / srD) : 0.f;
              __builtin_nontemporal_store(v, pq);
            }
            ageNow += (uint32_t)MLGPU_FLOATS_PER_DSPVECTOR * ageStep;
          }
        }
        if (onB) age += (uint32_t)(kBlock * MLGPU_FLOATS_PER_DSPVECTOR) * ageStep;
        // ---- the pitch row ----
        // What each of the block's vectors does to the drift glide, worked out first (it needs slot 63 only: what a starting
        // glide reads). Then the 64 slots in two halves of 32: a half's slots are fetched together, stepped through the kBlock
        // vectors in registers and written back. The pitch glide is a per-sample recurrence in time order: each half walks it
        // through the whole block from the block's start state, using the samples of its own half (when it rests, as mostly,
        // that is a constant).
        const SignalView& sp = a.out[0];
        const bool storePitch = sp.base && isVoice;
        const float bendTerm = (heldBend * pitchBendScale) * (1.f / 12);  // :244
        float eff63 = slotsLive ? u2f(gs[(size_t)(5 + 63) * ln]) : 0.f;
        int cm[kBlock];
        bool cu[kBlock];
        float cstep[kBlock], cstart[kBlock], ctarget[kBlock], cuval[kBlock];
        bool wrote = false;
#pragma unroll
        for (int b = 0; b < kBlock; ++b)
        {
          cm[b] = 0;
          cu[b] = true;
          cstep[b] = cstart[b] = ctarget[b] = cuval[b] = 0.f;
          if (onB)
          {
            // the drift part of Voice::beginProcess (:115-126), then the drift glide's own start of a vector
            drift_step(driftSeed, driftCounter, driftNext, driftValue, a.s.sr);
            gd.beginVectorKnown(driftValue, a.s.driftGlideVectors, a.s.driftGlideDy, eff63);
            cm[b] = gd.mode();
            cu[b] = gd.isUniform();
            cstep[b] = gd.step;
            cstart[b] = gd.startValue;
            ctarget[b] = gd.target;
            cuval[b] = gd.uniformValue;
            // slot 63 after this vector (n = 63: (float)(n + 1) * 0.015625f == 1)
            if (cm[b] == 2) eff63 = cstart[b] + 1.0f * cstep[b];
            else if (cm[b] == 3) eff63 = (cu[b] ? cuval[b] : eff63) + cstep[b];
            wrote = wrote || (cm[b] >= 2);
            gd.endVector();
          }
        }
        const bool pgMoves = __builtin_amdgcn_ballot_w64(onB && !(pg.remaining < 0 && pg.target == pitch)) != 0;  // any lane's pitch glide
        const PitchGlide pg0 = pg;  // the pitch glide as the block starts
        constexpr int kHalf = 32;
#pragma unroll 1
        for (int h = 0; h < 64; h += kHalf)
        {
          float c[kHalf];
#pragma unroll
          for (int i = 0; i < kHalf; ++i) c[i] = slotsLive ? u2f(gs[(size_t)(5 + h + i) * ln]) : 0.f;
          pg = pg0;
          f32x4b* pb = (f32x4b*)sp.base + t * sp.strideT + outVoice * sp.strideV + (size_t)(h / 4) * sp.strideQ;
#pragma unroll
          for (int b = 0; b < kBlock; ++b, pb += sp.strideT)
          {
            if (onB && pgMoves)
              for (int n = 0; n < h; ++n) (void)pg.next(pitch);  // the samples of this vector before this half
            f32x4b* pq = pb;
#pragma unroll
            for (int q = 0; q < kHalf / 4; ++q, pq += sp.strideQ)
            {
              f32x4b o;
#pragma unroll
              for (int k = 0; k < 4; ++k)
              {
                const int i = q * 4 + k, n = h + i;
                float vPitch = 0.f;
                if (onB)
                {
                  const int m = cm[b];
                  float v;
                  if (m == 0) v = cu[b] ? cuval[b] : c[i];
                  else if (m == 1) v = ctarget[b];
                  else
                  {
                    if (m == 2) v = cstart[b] + ((float)(n + 1) * 0.015625f) * cstep[b];
                    else v = (cu[b] ? cuval[b] : c[i]) + cstep[b];
                    c[i] = v;
                  }
                  vPitch = pg.next(pitch);
                  vPitch = vPitch + bendTerm;
                  vPitch = vPitch + (v * a.s.driftAmount) * 0.02f;           // kDriftScale, :247
                }
                o[k] = vPitch;
              }
              if (storePitch) __builtin_nontemporal_store(o, pq);
            }
            if (onB && pgMoves)
              for (int n = h + kHalf; n < 64; ++n) (void)pg.next(pitch);  // ... and after it
          }
          if (wrote)
#pragma unroll
            for (int i = 0; i < kHalf; ++i) gs[(size_t)(5 + h + i) * ln] = f2u(c[i]);
        }
        if (onB) gd.store(gs, ln);
        t += kBlock - 1;
        continue;
      }
    }
    // records of this vector: [cursor, vend)
    uint32_t vend = cursor;
    while (vend < recEnd && a.recs[vend].vec == (uint32_t)t) ++vend;
    if (!awake)
      for (uint32_t r = cursor; r < vend; ++r)
        if ((a.recs[r].typeTimeFlags & 0xFF) == REC_AWAKE) awake = true;

    float finalVelocity = velocity;
    bool noteHere = false;  // a note record of this lane falls into this vector
    if (awake && active)
    {
      begin_process(a.s, needsRecalc, inhibit, pg, driftSeed, driftCounter, driftNext, driftValue);
      needsRecalc = false;
      // ---- values that only matter at the end of the vector: apply them now (endProcess, :218-247) ----
      for (uint32_t r = cursor; r < vend; ++r)
      {
        const Rec rc = a.recs[r];
        switch (rc.typeTimeFlags & 0xFF)
        {
          case REC_SET_BEND: bend = rc.v1; break;
          case REC_SET_MOD: mod = rc.v1; break;
          case REC_SET_X: cx = rc.v1; break;
          case REC_SET_Y: cy = rc.v1; break;
          case REC_SET_Z: cz = rc.v1; break;
          case REC_SET_CHANNEL_PRESSURE: chanPress = rc.v1; break;
          case REC_NOTE_ON: case REC_NOTE_RETRIG: finalVelocity = rc.v2; noteHere = true; break;
          case REC_NOTE_OFF: finalVelocity = 0.f; noteHere = true; break;
          default: break;
        }
      }
      if (finalVelocity == 0.f) cz = 0.f;  // :238-241
    }
    const bool on = awake && active;
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    auto put = [&](int row, int q, const f32x4 v) {
      const SignalView& sv = a.out[row];
      if (sv.base && isVoice) __builtin_nontemporal_store(v, (f32x4*)sv.base + t * sv.strideT + (size_t)q * sv.strideQ + outVoice * sv.strideV);
    };
    // MPE: the main voice's signal is added to every playing voice of its instrument (:447-458)
    auto withMain = [&](float v) {
      if (!a.s.mpe) return v;
      const float m = __shfl(v, mainLane, 64);
      return (isVoice && awake) ? v + m : v;
    };

    // ---- rows that are one glide each: mod, x, y; z adds the smoothed channel pressure in MIDI mode (:437-445) ----
    // One short loop per row keeps the live state of the other rows out of the registers.
    // A glide that is not moving gives one value for the whole vector (hold with a broadcast mCurrVec, or the vector that
    // ends a glide): when that is so for every lane of the wavefront - controllers rarely move - the row is 16 stores.
    auto heldValue = [&](const Glide& gl, bool& held) {
      const int m = gl.mode();
      held = (m == 1) || (m == 0 && gl.isUniform());
      return (m == 1) ? gl.target : gl.uniformValue;
    };
    auto glideRow = [&](int glideIdx, int row, float value) {
      Glide gl;
      gl.load(GS(glideIdx), ln);
      if (on) gl.beginVector(GS(glideIdx), ln, value, a.s.glideVectors, a.s.glideDy);
      bool held;
      const float hv = heldValue(gl, held);
      if (__builtin_amdgcn_ballot_w64(on && !held) == 0)
      {
        const float c = withMain(on ? hv : 0.f);
        const f32x4 v = {c, c, c, c};
#pragma unroll 1
        for (int q = 0; q < 16; ++q) put(row, q, v);
      }
      else
      {
        float nx[4] = {0.f, 0.f, 0.f, 0.f};
        if (on) gl.preload(GS(glideIdx), ln, 0, nx);
#pragma unroll 1
        for (int q = 0; q < 16; ++q)
        {
          const float cur[4] = {nx[0], nx[1], nx[2], nx[3]};
          if (on && q < 15) gl.preload(GS(glideIdx), ln, q + 1, nx);
          f32x4 v;
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = withMain(on ? gl.nextWith(GS(glideIdx), ln, q * 4 + k, cur[k]) : 0.f);
          put(row, q, v);
        }
      }
      if (on)
      {
        gl.endVector();
        gl.store(GS(glideIdx), ln);
      }
    };
    if (!ROWS01 && (a.rowMask & (1u << 6))) glideRow(1, 6, mod);
    if (!ROWS01 && (a.rowMask & (1u << 4))) glideRow(2, 4, cx);
    if (!ROWS01 && (a.rowMask & (1u << 5))) glideRow(3, 5, cy);
    if (!ROWS01 && (a.rowMask & (1u << 3)))
    {
      Glide gz, gp;
      gz.load(GS(4), ln);
      gp.load(GS(6), ln);
      if (on)
      {
        gz.beginVector(GS(4), ln, cz, a.s.glideVectors, a.s.glideDy);
        gp.beginVector(GS(6), ln, chanPress, a.s.ctlGlideVectors, a.s.ctlGlideDy);  // SmoothedController::process, :268-280
      }
      bool heldZ, heldP;
      const float hz = heldValue(gz, heldZ), hp = heldValue(gp, heldP);
      if (__builtin_amdgcn_ballot_w64(on && !(heldZ && heldP)) == 0)
      {
        float z = 0.f;
        if (on)
        {
          z = hz;
          if (!a.s.mpe) z = z + hp;
        }
        const float c = withMain(z);
        const f32x4 v = {c, c, c, c};
#pragma unroll 1
        for (int q = 0; q < 16; ++q) put(3, q, v);
      }
      else
#pragma unroll 1
      for (int q = 0; q < 16; ++q)
      {
        float cz4[4] = {0.f, 0.f, 0.f, 0.f}, cp4[4] = {0.f, 0.f, 0.f, 0.f};
        if (on)
        {
          gz.preload(GS(4), ln, q, cz4);
          gp.preload(GS(6), ln, q, cp4);
        }
        f32x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k)
        {
          float z = 0.f;
          if (on)
          {
            z = gz.nextWith(GS(4), ln, q * 4 + k, cz4[k]);
            const float press = gp.nextWith(GS(6), ln, q * 4 + k, cp4[k]);
            if (!a.s.mpe) z = z + press;
          }
          v[k] = withMain(z);
        }
        put(3, q, v);
      }
      if (on)
      {
        gz.endVector();
        gp.endVector();
        gz.store(GS(4), ln);
        gp.store(GS(6), ln);
      }
    }
    if (!ROWS01 && (a.rowMask & (1u << 2)))
    {
      const float vox = (float)(slot - 1);  // row kVoice: DSPVector((float)i - 1), :302
      const f32x4 v = {vox, vox, vox, vox};
#pragma unroll 1
      for (int q = 0; q < 16; ++q) put(2, q, v);
    }

    // ---- gate, pitch, elapsed time: writeNoteEvent (:115-216) and endProcess (:218-262) walked frame by frame ----
    Glide gb, gd;
    gb.load(GS(0), ln);
    gd.load(GS(5), ln);
    if (on)
    {
      gb.beginVector(GS(0), ln, bend, a.s.glideVectors, a.s.glideDy);
      gd.beginVector(GS(5), ln, driftValue, a.s.driftGlideVectors, a.s.driftGlideDy);
    }
    uint32_t nc = cursor;      // next note record
    bool preApplied = false;   // a note event's bookkeeping applies from the frame the previous one ended at
    // Most vectors of most wavefronts hold no note event at all: then every frame is the same few steps (gate = velocity,
    // one step of the pitch glide, the event age, bend and drift), written out without the record walk.
    const bool quietWave = __builtin_amdgcn_ballot_w64(noteHere) == 0;
    if (quietWave)
    {
      // one short loop per row, as above: the gate is the held velocity, the event age advances by ageStep per frame
      {
        const float g = on ? velocity : 0.f;
        const f32x4 v = {g, g, g, g};
#pragma unroll 1
        for (int q = 0; q < 16; ++q) put(1, q, v);
      }
      if (wantTime)
      {
#pragma unroll 1
        for (int q = 0; q < 16; ++q)
        {
          f32x4 v;
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = on ? (float)((double)(age + (uint32_t)(q * 4 + k + 1) * ageStep) / srD) : 0.f;
          put(7, q, v);
        }
      }
      if (on) age += (uint32_t)MLGPU_FLOATS_PER_DSPVECTOR * ageStep;
      float nb[4] = {0.f, 0.f, 0.f, 0.f}, nd[4] = {0.f, 0.f, 0.f, 0.f};  // bend / drift mCurrVec, one quad ahead
      if (on)
      {
        gb.preload(GS(0), ln, 0, nb);
        gd.preload(GS(5), ln, 0, nd);
      }
#pragma unroll 1
      for (int q = 0; q < 16; ++q)
      {
        const float cb[4] = {nb[0], nb[1], nb[2], nb[3]}, cd[4] = {nd[0], nd[1], nd[2], nd[3]};
        if (on && q < 15)
        {
          gb.preload(GS(0), ln, q + 1, nb);
          gd.preload(GS(5), ln, q + 1, nd);
        }
        f32x4 oPitch;
#pragma unroll
        for (int k = 0; k < 4; ++k)
        {
          const int n = q * 4 + k;
          float vPitch = 0.f;
          if (on)
          {
            vPitch = pg.next(pitch);
            const float bendSig = gb.nextWith(GS(0), ln, n, cb[k]), driftSig = gd.nextWith(GS(5), ln, n, cd[k]);
            vPitch = vPitch + (bendSig * pitchBendScale) * (1.f / 12);         // :244
            vPitch = vPitch + (driftSig * a.s.driftAmount) * 0.02f;           // kDriftScale, :247
          }
          oPitch[k] = withMain(vPitch);
        }
        put(0, q, oPitch);
      }
    }
    else
    {
    RecCache recCache;
    if (on) note_rewind(a.recs, nc, vend, velocity, pitch, age, ageStep, inhibit, pg, a.s.pitchGlideSamples);
#pragma unroll 1
    for (int q = 0; q < 16; ++q)
    {
      f32x4 oPitch = {0.f, 0.f, 0.f, 0.f}, oGate = oPitch, oTime = oPitch;
#pragma unroll 1
      for (int k = 0; k < 4; ++k)
      {
        const int n = q * 4 + k;
        float vPitch = 0.f, vGate = 0.f, vTime = 0.f;
        if (on)
        {
          note_frame(a.recs, recCache, nc, vend, n, preApplied, velocity, pitch, age, ageStep, inhibit, pg, a.s.pitchGlideSamples, wantTime, srD, vPitch, vGate,
                     vTime);
          const float bendSig = gb.next(GS(0), ln, n), driftSig = gd.next(GS(5), ln, n);
          vPitch = vPitch + (bendSig * pitchBendScale) * (1.f / 12);         // :244
          vPitch = vPitch + (driftSig * a.s.driftAmount) * 0.02f;           // kDriftScale, :247
        }
        vPitch = withMain(vPitch);
        // k is a loop variable here (the body is large): insert with selects instead of a dynamic register index
        oPitch = {k == 0 ? vPitch : oPitch[0], k == 1 ? vPitch : oPitch[1], k == 2 ? vPitch : oPitch[2], k == 3 ? vPitch : oPitch[3]};
        oGate = {k == 0 ? vGate : oGate[0], k == 1 ? vGate : oGate[1], k == 2 ? vGate : oGate[2], k == 3 ? vGate : oGate[3]};
        oTime = {k == 0 ? vTime : oTime[0], k == 1 ? vTime : oTime[1], k == 2 ? vTime : oTime[2], k == 3 ? vTime : oTime[3]};
      }
      put(0, q, oPitch);
      put(1, q, oGate);
      put(7, q, oTime);
    }
    }
    if (on)
    {
      gb.endVector();
      gd.endVector();
      gb.store(GS(0), ln);
      gd.store(GS(5), ln);
    }
    cursor = vend;
  }

  if (!live) return;
  // Recompute the state addresses from a value the optimiser cannot relate to the loads at the top: otherwise ~60 64-bit
  // per-lane pointers stay live across the whole kernel (it needed more than 256 VGPRs).
  {
    size_t Lend = L;
    asm volatile("" : "+v"(Lend));
    S = a.state + Lend;
    if (recRange.x != recRange.y) a.recRange[Lend] = make_uint2(0u, 0u);  // consumed: the next launch finds "no records" unless told otherwise
  }
  SW(S_AWAKE) = awake ? 1u : 0u;
  SW(S_VELOCITY) = f2u(velocity); SW(S_PITCH) = f2u(pitch); SW(S_BEND) = f2u(bend); SW(S_MOD) = f2u(mod);
  SW(S_X) = f2u(cx); SW(S_Y) = f2u(cy); SW(S_Z) = f2u(cz); SW(S_CHANPRESS) = f2u(chanPress);
  SW(S_AGE) = age; SW(S_AGE_STEP) = ageStep; SW(S_INHIBIT_GLIDE) = inhibit ? 1u : 0u; SW(S_RECALC) = needsRecalc ? 1u : 0u;
  SW(S_PG_CURR) = f2u(pg.curr); SW(S_PG_STEP) = f2u(pg.step); SW(S_PG_TARGET) = f2u(pg.target); SW(S_PG_REMAINING) = (uint32_t)pg.remaining;
  SW(S_PG_PER_GLIDE) = (uint32_t)pg.perGlide; SW(S_PG_DY) = f2u(pg.dyPerSample);
  SW(S_DRIFT_SEED) = driftSeed; SW(S_DRIFT_COUNTER) = (uint32_t)driftCounter; SW(S_DRIFT_VALUE) = f2u(driftValue); SW(S_DRIFT_NEXT) = (uint32_t)driftNext;
#undef GS
#undef SW
}

// ---- the control-rate half of EventsToSignals for voice graphs (mldsp_events.hpp: CtlVoice is the audio-rate half) ----------------
// One lane per voice (MIDI protocol). Per DSPVector: the records of the vector, Voice::beginProcess (:75-126) with the drift random
// walk, the bend glide's start of a vector, and a decision: does anything move INSIDE this vector apart from the drift glide? If
// not - no note event, the pitch glide at rest, the bend held: all but a few per cent of the vectors - the vector is four words
// (pitch before drift, gate, the drift glide's input, flags) and costs no per-sample work at all. If so, the lane walks the 64
// frames with note_frame() as e2s_kernel does and writes its pitch-before-drift and gate to the side signals (16 quads each);
// a portamento in progress with nothing else going on is the pitch glide's 64 steps alone (pitch side signal only). The drift glide is not touched here: its slots belong to the
// voice kernel, and nothing in this kernel depends on them (the drift term is added last, :247).
// the lanes that have records in the coming launch: {lane, first, one past the last}
__global__ void set_rec_ranges_kernel(const uint4* list, size_t n, uint2* ranges)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) ranges[list[i].x] = make_uint2(list[i].y, list[i].z);
}

// ... and the same lanes back to "no records": what the consuming kernel does itself, for a block whose consuming kernel was never
// launched (a failure between set_rec_ranges_kernel and that launch: abandonRanges)
__global__ void clear_rec_ranges_kernel(const uint4* list, size_t n, uint2* ranges)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) ranges[list[i].x] = make_uint2(0u, 0u);
}

struct E2SCtlArgs
{
  uint32_t* state;
  const Rec* recs;
  uint2* recRange;
  uint32_t* ctl;   // [T][kCtlRecWords][lanes]
  float4* rowP;    // QUAD [16 T][lanes][4], written for CF_ROWS vectors only
  float4* rowG;
  // ROWS: the controller rows a graph reads (EventsDev::held / rowC / ctlRowMask: bits 3..6)
  uint32_t* held;  // [T][rows of rowMask, ascending][lanes]
  float4* rowC[4]; // z, x, y, mod: QUAD, written for CF_ROW(r) vectors only
  uint32_t rowMask;
  int32_t group;     // the MPE instances: lane = instrument * group + (voice slot - slotBase), as E2SArgs has them. (The two sit where the
  size_t lanes, T;   // struct had padding: every other member, and the hidden kernel arguments behind the struct, stay where the MIDI
  uint32_t flags;    // instances' code reads them - tools/asm_compare.py.)
  int32_t slotBase;
  E2SSettings s;
};

// The 64 frames of a glide that moves inside the vector, into its row's side signal (what e2s_kernel's glideRow writes to the row
// itself). Out of line: it runs for the few vectors after a controller event, and inlined four times its address arithmetic took
// e2s_ctl_rows_kernel's per-vector path past every register there is.
__device__ __noinline__ void ctl_glide_frames(const Glide& gl, uint32_t* gs, size_t ln, float4* out)
{
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  f32x4* o = (f32x4*)out;
  float nx[4] = {0.f, 0.f, 0.f, 0.f};
  gl.preload(gs, ln, 0, nx);
#pragma unroll 1
  for (int q = 0; q < 16; ++q, o += ln)
  {
    const float cur[4] = {nx[0], nx[1], nx[2], nx[3]};
    if (q < 15) gl.preload(gs, ln, q + 1, nx);
    f32x4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = gl.nextWith(gs, ln, q * 4 + k, cur[k]);
    __builtin_nontemporal_store(v, o);
  }
}
// ... and of z: its own glide plus the smoothed channel pressure (:437-445, MIDI protocol), as e2s_kernel adds them
__device__ __noinline__ void ctl_z_frames(const Glide& gz, const Glide& gp, uint32_t* gsz, uint32_t* gsp, size_t ln, float4* out)
{
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  f32x4* o = (f32x4*)out;
#pragma unroll 1
  for (int q = 0; q < 16; ++q, o += ln)
  {
    float cz4[4] = {0.f, 0.f, 0.f, 0.f}, cp4[4] = {0.f, 0.f, 0.f, 0.f};
    gz.preload(gsz, ln, q, cz4);
    gp.preload(gsp, ln, q, cp4);
    f32x4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k)
    {
      float z = gz.nextWith(gsz, ln, q * 4 + k, cz4[k]);
      const float press = gp.nextWith(gsp, ln, q * 4 + k, cp4[k]);
      z = z + press;
      v[k] = z;
    }
    __builtin_nontemporal_store(v, o);
  }
}

// ... and of z under the MPE protocol: its own glide alone. The channel-pressure glide takes its steps all the same, as e2s_kernel's does
// (its state words are what the other call expects), but is not added (:437-445).
__device__ __noinline__ void ctl_z_frames_mpe(const Glide& gz, const Glide& gp, uint32_t* gsz, uint32_t* gsp, size_t ln, float4* out)
{
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  f32x4* o = (f32x4*)out;
#pragma unroll 1
  for (int q = 0; q < 16; ++q, o += ln)
  {
    float cz4[4] = {0.f, 0.f, 0.f, 0.f}, cp4[4] = {0.f, 0.f, 0.f, 0.f};
    gz.preload(gsz, ln, q, cz4);
    gp.preload(gsp, ln, q, cp4);
    f32x4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k)
    {
      v[k] = gz.nextWith(gsz, ln, q * 4 + k, cz4[k]);
      (void)gp.nextWith(gsp, ln, q * 4 + k, cp4[k]);
    }
    __builtin_nontemporal_store(v, o);
  }
}

// The MPE main voice's pitch row of a vector with no note event and a held bend: the pitch glide's 64 steps and the drift glide's, the
// drift term added last (:247). The drift glide moves in nearly every vector and every wavefront holds main voices, so its mCurrVec
// slots are fetched 16 at a time: four round trips per vector where a load per frame behind the frame before's store was 64 (the
// control kernel's whole time, profiles/graph_events_mpe.md). In line: out of line the pitch glide's words went through scratch, a
// memory round trip per frame again.
__device__ __forceinline__ void ctl_main_pitch_frames(PitchGlide& pg, float pitch, float bendTerm, const Glide& gd, uint32_t* gs, size_t ln, float amount, float4* out)
{
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  f32x4* o = (f32x4*)out;
  constexpr int kChunk = 16;  // (32 at a time measured no faster: 2788 against 2661 us for the kernel)
  const bool reads = gd.readsCurrVec();
#pragma unroll 1
  for (int h = 0; h < 64; h += kChunk)
  {
    float cur[kChunk];
#pragma unroll
    for (int i = 0; i < kChunk; ++i) cur[i] = 0.f;
    if (reads)
    {
#pragma unroll
      for (int i = 0; i < kChunk; ++i) cur[i] = u2f(gs[(size_t)(5 + h + i) * ln]);
    }
#pragma unroll
    for (int q = 0; q < kChunk / 4; ++q, o += ln)
    {
      f32x4 v;
#pragma unroll
      for (int k = 0; k < 4; ++k)
      {
        const float p = pg.next(pitch) + bendTerm;
        v[k] = p + (gd.nextWith(gs, ln, h + q * 4 + k, cur[q * 4 + k]) * amount) * 0.02f;
      }
      __builtin_nontemporal_store(v, o);
    }
  }
}

// ROWS: the graph reads some of the rows z, x, y, mod (a.rowMask). Their glides - 1 mod, 2 x, 3 y, 4 z with 6, the smoothed channel
// pressure - are run here as e2s_kernel's glideRow runs them, once per vector and lane: a glide that is held gives ONE word (the plane
// a.held), one that moves inside the vector its 64 frames in the row's side signal and CF_ROW(r) in the vector's flags. A row outside
// a.rowMask keeps its glide where it is (mlgpu_events_set_wanted_rows' rule). The instance without ROWS is the kernel of a graph
// that reads pitch and gate only: none of this is in its code.
// MPE: the instances for an events object under the MPE protocol (a graph built with mlgpu_graph_enable_mpe_events). A lane is slot
// lane % group + slotBase of its instrument: the padding lanes past the polyphony leave at once, the bend scale goes by slot (:417-423),
// z does not add the channel pressure. A slot-0 lane is the MAIN voice: no voice kernel expands its record, so this kernel owns its drift
// glide (glide 5) too - walked as e2s_kernel's general loop walks it - and its pitch is the complete row, (pitch glide + bend term) +
// drift * amount * 0.02 in the reference's order (:244, :247): one value in C_PITCH while pitch glide, bend and drift glide are all held,
// else 64 frames in rowP under CF_ROWS. The voice kernel adds it to the instrument's playing voices (mlev::CtlVoiceMpe). The MIDI
// instances hold none of this.
template <bool ROWS, bool MPE = false>
__device__ __forceinline__ void e2s_ctl_body(const E2SCtlArgs& a)
{
  apply_fp_mode(a.flags);
  size_t blk = blockIdx.x;
  const size_t nbFull = (size_t)gridDim.x & ~(size_t)7;
  if (blk < nbFull) blk = (blk & 7) * (nbFull >> 3) + (blk >> 3);
  const size_t lane = blk * 256 + threadIdx.x;
  if (lane >= a.lanes) return;
  [[maybe_unused]] bool isMain = false;
  if constexpr (MPE)
  {
    const int slot = (int)(lane % (size_t)a.group) + a.slotBase;
    if (slot > a.s.polyphony) return;  // padding
    isMain = slot == 0;
  }
  uint32_t* S = a.state + lane;
  const size_t ln = a.lanes;
#define SW(i) S[(size_t)(i) * ln]
  bool awake = SW(S_AWAKE) != 0;
  float velocity = u2f(SW(S_VELOCITY)), pitch = u2f(SW(S_PITCH)), bend = u2f(SW(S_BEND)), cz = u2f(SW(S_Z));
  uint32_t age = SW(S_AGE), ageStep = SW(S_AGE_STEP);
  bool inhibit = SW(S_INHIBIT_GLIDE) != 0, needsRecalc = SW(S_RECALC) != 0;
  PitchGlide pg;
  pg.curr = u2f(SW(S_PG_CURR)), pg.step = u2f(SW(S_PG_STEP)), pg.target = u2f(SW(S_PG_TARGET)), pg.dyPerSample = u2f(SW(S_PG_DY));
  pg.remaining = (int32_t)SW(S_PG_REMAINING), pg.perGlide = (int32_t)SW(S_PG_PER_GLIDE);
  uint32_t driftSeed = SW(S_DRIFT_SEED);
  int32_t driftCounter = (int32_t)SW(S_DRIFT_COUNTER), driftNext = (int32_t)SW(S_DRIFT_NEXT);
  float driftValue = u2f(SW(S_DRIFT_VALUE));
  // controller values that only pass through (their rows are not computed by this form): kept current as mlgpu_events_set_wanted_rows does
  // (ROWS: they feed this vector's glides, so they live in registers and go back to memory at the end)
  [[maybe_unused]] float mod = 0.f, cx = 0.f, cy = 0.f, chanPress = 0.f;
  if constexpr (ROWS)
  {
    mod = u2f(SW(S_MOD)), cx = u2f(SW(S_X)), cy = u2f(SW(S_Y)), chanPress = u2f(SW(S_CHANPRESS));
  }
#define GS(i) (S + (size_t)(S_GLIDES + (i) * kGlideWords) * ln)
  [[maybe_unused]] const int nHeld = ROWS ? ctl_row_count(a.rowMask) : 0;
  // ROWS: the wanted rows' glides (1 mod, 2 x, 3 y, 4 z, 6 channel pressure) live in registers for the whole launch, as the bend glide
  // does: one load and one store per launch, where a load per vector stands behind the vector's stores and waits out their
  // acknowledgement. (A moving glide's mCurrVec slots stay in memory: ctl_glide_frames - the walk of such a glide is what this kernel's
  // time is made of, profiles/graph_event_rows.md.)
  [[maybe_unused]] Glide gm, gx, gy, gz, gp;
  if constexpr (ROWS)
  {
    if (a.rowMask & (1u << 6)) gm.load(GS(1), ln);
    if (a.rowMask & (1u << 4)) gx.load(GS(2), ln);
    if (a.rowMask & (1u << 5)) gy.load(GS(3), ln);
    if (a.rowMask & (1u << 3))
    {
      gz.load(GS(4), ln);
      gp.load(GS(6), ln);
    }
  }
  uint32_t* GB = S + (size_t)(S_GLIDES + 0 * kGlideWords) * ln;
  Glide gb;
  gb.load(GB, ln);
  [[maybe_unused]] uint32_t* const GD = S + (size_t)(S_GLIDES + 5 * kGlideWords) * ln;  // MPE: the main voice's drift glide
  [[maybe_unused]] Glide gd;
  if constexpr (MPE)
  {
    if (isMain) gd.load(GD, ln);
  }

  const uint2 recRange = a.recRange[lane];  // this lane's records of this launch: [x, y)
  uint32_t cursor = recRange.x;
  const uint32_t recEnd = recRange.y;
  // the vector of this lane's next record, in a register: a lane with a record later in the launch does not ask memory every vector
  uint32_t nextVec = cursor < recEnd ? a.recs[cursor].vec : 0xFFFFFFFFu;
  float pitchBendScale = a.s.pitchBendRange;  // MIDI protocol, :417-423
  if constexpr (MPE) pitchBendScale = (a.s.mpe && !isMain) ? a.s.mpePitchBendRange : a.s.pitchBendRange;
  uint32_t* rec = a.ctl + lane;
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  for (size_t t = 0; t < a.T; ++t, rec += (size_t)kCtlRecWords * ln)
  {
    uint32_t vend = cursor;
    if (nextVec == (uint32_t)t)
      while (vend < recEnd && a.recs[vend].vec == (uint32_t)t) ++vend;
    if (!awake)
      for (uint32_t r = cursor; r < vend; ++r)
        if ((a.recs[r].typeTimeFlags & 0xFF) == REC_AWAKE) awake = true;
    const bool on = awake;
    bool noteHere = false;
    if (on)
    {
      begin_process(a.s, needsRecalc, inhibit, pg, driftSeed, driftCounter, driftNext, driftValue);
      needsRecalc = false;
      // ---- values that only matter at the end of the vector (endProcess, :218-247); the rows this form does not compute keep their
      //      values in memory ----
      float finalVelocity = velocity;
      for (uint32_t r = cursor; r < vend; ++r)
      {
        const Rec rc = a.recs[r];
        switch (rc.typeTimeFlags & 0xFF)
        {
          case REC_SET_BEND: bend = rc.v1; break;
          case REC_SET_MOD: if constexpr (ROWS) mod = rc.v1; else SW(S_MOD) = f2u(rc.v1); break;
          case REC_SET_X: if constexpr (ROWS) cx = rc.v1; else SW(S_X) = f2u(rc.v1); break;
          case REC_SET_Y: if constexpr (ROWS) cy = rc.v1; else SW(S_Y) = f2u(rc.v1); break;
          case REC_SET_Z: cz = rc.v1; break;
          case REC_SET_CHANNEL_PRESSURE: if constexpr (ROWS) chanPress = rc.v1; else SW(S_CHANPRESS) = f2u(rc.v1); break;
          case REC_NOTE_ON: case REC_NOTE_RETRIG: finalVelocity = rc.v2; noteHere = true; break;
          case REC_NOTE_OFF: finalVelocity = 0.f; noteHere = true; break;
          default: break;
        }
      }
      if (finalVelocity == 0.f) cz = 0.f;  // :238-241
      gb.beginVector(GB, ln, bend, a.s.glideVectors, a.s.glideDy);
      if constexpr (MPE)
      {
        if (isMain) gd.beginVector(GD, ln, driftValue, a.s.driftGlideVectors, a.s.driftGlideDy);
      }
    }
    const int bm = gb.mode();
    const bool heldB = (bm == 1) || (bm == 0 && gb.isUniform());
    const bool pgBusy = on && (pitch != pg.target || pg.remaining >= 0);
    const bool walk = on && (noteHere || !heldB);
    // (MPE, the main voice: its drift glide is part of its pitch row - while it moves, a vector with nothing else going on is 64 frames too)
    [[maybe_unused]] bool driftMoves = false;
    if constexpr (MPE)
    {
      const int dm = gd.mode();
      driftMoves = on && isMain && !((dm == 1) || (dm == 0 && gd.isUniform()));
    }
    const bool glideOnly = on && !walk && (pgBusy || driftMoves);  // a portamento in progress, nothing else: the pitch glide's 64 steps, the gate held
    const float hvB = (bm == 1) ? gb.target : gb.uniformValue;
    // the main voice's drift term of frame n, added last (:247); gd.next is the record-walking path's form of a glide's sample
    [[maybe_unused]] auto withDrift = [&](float v, int n) {
      if constexpr (MPE)
      {
        if (isMain) v = v + (gd.next(GD, ln, n) * a.s.driftAmount) * 0.02f;
      }
      return v;
    };
    float P = 0.f, gate = 0.f;
    if (!walk)
    {
      if (on)
      {
        gate = velocity;
        age += (uint32_t)MLGPU_FLOATS_PER_DSPVECTOR * ageStep;
        const float bendTerm = (hvB * pitchBendScale) * (1.f / 12);  // :244
        if (!glideOnly)
        {
          P = pg.curr + bendTerm;  // the same for all 64 frames
          if constexpr (MPE)
          {
            if (isMain) P = P + (((gd.mode() == 1) ? gd.target : gd.uniformValue) * a.s.driftAmount) * 0.02f;  // the drift glide is held
          }
        }
        else
        {
          f32x4* oP = (f32x4*)a.rowP + (t * 16) * ln + lane;
          // in the middle of a glide - 64 or more steps to go, the target unchanged - every frame of the vector is nextSample's last
          // branch (:571-576): mCurr += mStep. 64 dependent adds instead of 64 trips through the state machine.
          if (MPE && isMain) ctl_main_pitch_frames(pg, pitch, bendTerm, gd, GD, ln, a.s.driftAmount, a.rowP + (t * 16) * ln + lane);
          else if (pitch == pg.target && pg.remaining >= MLGPU_FLOATS_PER_DSPVECTOR && pg.remaining < pg.perGlide)
          {
#pragma unroll 4
            for (int q = 0; q < 16; ++q, oP += ln)
            {
              f32x4 vP;
#pragma unroll
              for (int k = 0; k < 4; ++k)
              {
                pg.curr += pg.step;
                vP[k] = pg.curr + bendTerm;
              }
              __builtin_nontemporal_store(vP, oP);
            }
            pg.remaining -= MLGPU_FLOATS_PER_DSPVECTOR;
          }
          else
#pragma unroll 1
          for (int q = 0; q < 16; ++q, oP += ln)
          {
            f32x4 vP;
#pragma unroll
            for (int k = 0; k < 4; ++k) vP[k] = pg.next(pitch) + bendTerm;
            __builtin_nontemporal_store(vP, oP);
          }
        }
      }
    }
    else
    {
      // ---- gate and pitch frame by frame: writeNoteEvent (:115-216) and endProcess (:218-244) ----
      // note_frame() is the whole state machine of a frame (~150 instructions); most frames of a vector with a note event need
      // none of it: until the frame before the next note record's own frame (where a retrigger opens its one-frame gap, and
      // where the rewrite pattern at the end of note_frame looks ahead) a frame is the held gate, one step of the pitch glide
      // and one of the event age - what note_frame does on such a frame, given that the pending record's bookkeeping (which
      // applies from the first frame that sees the record) has been done. plan() does that bookkeeping and says how far.
      uint32_t nc = cursor;
      bool preApplied = false;
      RecCache recCache;
      auto plan = [&](int from) -> int {
        while (nc < vend)
        {
          const Rec rc = recCache.at(a.recs, nc);
          const uint32_t type = rc.typeTimeFlags & 0xFF;
          if (type != REC_NOTE_ON && type != REC_NOTE_RETRIG && type != REC_NOTE_OFF)
          {
            ++nc;
            continue;
          }
          int dest = (int)((rc.typeTimeFlags >> 8) & 0xFF);
          if (!preApplied)
          {
            MLEV_NOTE_START(type, rc.typeTimeFlags >> 16, a.s.pitchGlideSamples, age, ageStep, inhibit, pg);
            preApplied = true;
          }
          if (type == REC_NOTE_RETRIG && dest == 0) dest = 1;
          return dest - 1 > from ? dest - 1 : from;
        }
        return 64;
      };
      note_rewind(a.recs, nc, vend, velocity, pitch, age, ageStep, inhibit, pg, a.s.pitchGlideSamples);
      int quietUntil = heldB ? plan(0) : 0;  // frames [n, quietUntil) need no state machine (a moving bend: every frame does)
      f32x4* oP = (f32x4*)a.rowP + (t * 16) * ln + lane;
      f32x4* oG = (f32x4*)a.rowG + (t * 16) * ln + lane;
      const float bendTerm = (hvB * pitchBendScale) * (1.f / 12);
#pragma unroll 1
      for (int q = 0; q < 16; ++q, oP += ln, oG += ln)
      {
        f32x4 vP = {0.f, 0.f, 0.f, 0.f}, vG = vP;
#pragma unroll 1
        for (int k = 0; k < 4; ++k)
        {
          const int n = q * 4 + k;
          float vPitch = 0.f, vGate = 0.f, vTime = 0.f;
          if (n < quietUntil)
          {
            vGate = velocity;
            vPitch = pg.next(pitch) + bendTerm;
            age += ageStep;
            if constexpr (MPE) vPitch = withDrift(vPitch, n);
          }
          else
          {
            note_frame(a.recs, recCache, nc, vend, n, preApplied, velocity, pitch, age, ageStep, inhibit, pg, a.s.pitchGlideSamples, false, 1.0, vPitch, vGate,
                       vTime);
            const float bendSig = gb.next(GB, ln, n);
            vPitch = vPitch + (bendSig * pitchBendScale) * (1.f / 12);  // :244
            if constexpr (MPE) vPitch = withDrift(vPitch, n);
            if (heldB) quietUntil = plan(n + 1);
          }
          vP = f32x4{k == 0 ? vPitch : vP[0], k == 1 ? vPitch : vP[1], k == 2 ? vPitch : vP[2], k == 3 ? vPitch : vP[3]};
          vG = f32x4{k == 0 ? vGate : vG[0], k == 1 ? vGate : vG[1], k == 2 ? vGate : vG[2], k == 3 ? vGate : vG[3]};
        }
        __builtin_nontemporal_store(vP, oP);
        __builtin_nontemporal_store(vG, oG);
      }
    }
    uint32_t rowFlags = 0u;
    if constexpr (ROWS)
    {
      // ---- the rows that are one glide each: mod, x, y; z adds the smoothed channel pressure (:437-445, MIDI protocol) ----
      uint32_t* const hw = a.held + (t * (size_t)nHeld) * ln + lane;
      auto heldValue = [&](const Glide& gl, bool& held) {
        const int m = gl.mode();
        held = (m == 1) || (m == 0 && gl.isUniform());
        return (m == 1) ? gl.target : gl.uniformValue;
      };
      auto glideRow = [&](Glide& gl, int glideIdx, int row, float value) {
        uint32_t* const gs = GS(glideIdx);
        if (on) gl.beginVector(gs, ln, value, a.s.glideVectors, a.s.glideDy);
        bool held;
        const float hv = heldValue(gl, held);
        if (on && !held)
        {
          ctl_glide_frames(gl, gs, ln, a.rowC[row - 3] + (t * 16) * ln + lane);
          rowFlags |= CF_ROW(row);
        }
        hw[(size_t)ctl_row_rank(a.rowMask, row) * ln] = f2u((on && held) ? hv : 0.f);
        if (on) gl.endVector();
      };
      if (a.rowMask & (1u << 6)) glideRow(gm, 1, 6, mod);
      if (a.rowMask & (1u << 4)) glideRow(gx, 2, 4, cx);
      if (a.rowMask & (1u << 5)) glideRow(gy, 3, 5, cy);
      if (a.rowMask & (1u << 3))
      {
        if (on)
        {
          gz.beginVector(GS(4), ln, cz, a.s.glideVectors, a.s.glideDy);
          gp.beginVector(GS(6), ln, chanPress, a.s.ctlGlideVectors, a.s.ctlGlideDy);  // SmoothedController::process, :268-280
        }
        bool heldZ, heldP;
        const float hz = heldValue(gz, heldZ), hp = heldValue(gp, heldP);
        const bool held = heldZ && heldP;
        float zv = 0.f;
        if (on && !held)
        {
          if (MPE && a.s.mpe) ctl_z_frames_mpe(gz, gp, GS(4), GS(6), ln, a.rowC[0] + (t * 16) * ln + lane);
          else ctl_z_frames(gz, gp, GS(4), GS(6), ln, a.rowC[0] + (t * 16) * ln + lane);
          rowFlags |= CF_ROW(3);
        }
        else if (on)
        {
          zv = hz;
          if (!(MPE && a.s.mpe)) zv = zv + hp;
        }
        hw[(size_t)ctl_row_rank(a.rowMask, 3) * ln] = f2u(zv);
        if (on)
        {
          gz.endVector();
          gp.endVector();
        }
      }
    }
    rec[0] = f2u(P);
    rec[ln] = f2u(gate);
    rec[2 * ln] = f2u(driftValue);
    rec[3 * ln] = (on ? CF_ON : 0u) | ((walk || glideOnly) ? CF_ROWS : 0u) | (walk ? CF_GATE_ROW : 0u) | rowFlags;
    if (on) gb.endVector();
    if constexpr (MPE)
    {
      if (on && isMain) gd.endVector();
    }
    if (vend != cursor)
    {
      cursor = vend;
      nextVec = cursor < recEnd ? a.recs[cursor].vec : 0xFFFFFFFFu;
    }
  }
  {
    size_t Lend = lane;
    asm volatile("" : "+v"(Lend));
    S = a.state + Lend;
    if (recRange.x != recRange.y) a.recRange[Lend] = make_uint2(0u, 0u);  // consumed
  }
  gb.store(S + (size_t)(S_GLIDES + 0 * kGlideWords) * ln, ln);
  if constexpr (MPE)
  {
    if (isMain) gd.store(S + (size_t)(S_GLIDES + 5 * kGlideWords) * ln, ln);
  }
  SW(S_AWAKE) = awake ? 1u : 0u;
  SW(S_VELOCITY) = f2u(velocity); SW(S_PITCH) = f2u(pitch); SW(S_BEND) = f2u(bend); SW(S_Z) = f2u(cz);
  SW(S_AGE) = age; SW(S_AGE_STEP) = ageStep; SW(S_INHIBIT_GLIDE) = inhibit ? 1u : 0u; SW(S_RECALC) = needsRecalc ? 1u : 0u;
  SW(S_PG_CURR) = f2u(pg.curr); SW(S_PG_STEP) = f2u(pg.step); SW(S_PG_TARGET) = f2u(pg.target); SW(S_PG_REMAINING) = (uint32_t)pg.remaining;
  SW(S_PG_PER_GLIDE) = (uint32_t)pg.perGlide; SW(S_PG_DY) = f2u(pg.dyPerSample);
  SW(S_DRIFT_SEED) = driftSeed; SW(S_DRIFT_COUNTER) = (uint32_t)driftCounter; SW(S_DRIFT_VALUE) = f2u(driftValue); SW(S_DRIFT_NEXT) = (uint32_t)driftNext;
  if constexpr (ROWS)
  {
    SW(S_MOD) = f2u(mod); SW(S_X) = f2u(cx); SW(S_Y) = f2u(cy); SW(S_CHANPRESS) = f2u(chanPress);
    if (a.rowMask & (1u << 6)) gm.store(GS(1), ln);
    if (a.rowMask & (1u << 4)) gx.store(GS(2), ln);
    if (a.rowMask & (1u << 5)) gy.store(GS(3), ln);
    if (a.rowMask & (1u << 3))
    {
      gz.store(GS(4), ln);
      gp.store(GS(6), ln);
    }
  }
#undef GS
#undef SW
}
// (two kernels rather than one template: the instance with the controller rows is bounded to two wavefronts per SIMD - left to itself
// it takes every register there is for the unrolled glide loops and runs one -, the pitch/gate instance keeps the attributes it had)
__global__ __launch_bounds__(256) void e2s_ctl_kernel(const E2SCtlArgs a) { e2s_ctl_body<false>(a); }
__global__ __launch_bounds__(256, 2) void e2s_ctl_rows_kernel(const E2SCtlArgs a) { e2s_ctl_body<true>(a); }
// ... and the two for an object under the MPE protocol (launched over all its lanes: main voices, playing voices, padding)
__global__ __launch_bounds__(256) void e2s_ctl_mpe_kernel(const E2SCtlArgs a) { e2s_ctl_body<false, true>(a); }
__global__ __launch_bounds__(256, 2) void e2s_ctl_rows_mpe_kernel(const E2SCtlArgs a) { e2s_ctl_body<true, true>(a); }

// ---- smoothed controller signals: one lane per (watched controller slot, instrument); CtlRec and the C_* state words are in
// mlev_format.hpp -------------------------------------------------------------------------------------------------------------
struct CtlArgs
{
  uint32_t* state;           // [kCtlWords][lanes]
  const CtlRec* recs;
  const uint32_t* recStart;  // [lanes + 1]
  float* out;                // [slot][16 maxVectors][nInstruments][4]: slot s is a QUAD signal of nInstruments voices
  size_t nInstruments, lanes, T, slotStride;
  int32_t glideVectors;
  float glideDy;
};
__global__ __launch_bounds__(256) void ctl_kernel(const CtlArgs a)
{
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  const size_t lane = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (lane >= a.lanes) return;
  const size_t slot = lane / a.nInstruments, inst = lane - slot * a.nInstruments, ln = a.lanes;
  uint32_t* st = a.state + lane;
  uint32_t* gs = st + (size_t)C_GLIDE * ln;
  bool awake = st[(size_t)C_AWAKE * ln] != 0;
  float input = u2f(st[(size_t)C_INPUT * ln]);
  uint32_t r = a.recStart[lane];
  const uint32_t rend = a.recStart[lane + 1];
  f32x4* out = (f32x4*)(a.out + slot * a.slotStride) + inst;
  Glide gl;
  gl.load(gs, ln);
  for (size_t t = 0; t < a.T; ++t)
  {
    for (; r < rend && (a.recs[r].vecKind >> 1) == (uint32_t)t; ++r)
    {
      if (a.recs[r].vecKind & 1u) awake = true;
      else input = a.recs[r].value;
    }
    f32x4* o = out + t * 16 * a.nInstruments;
    if (!awake)  // processVector returns before anything is computed (:386): the outputs keep their initial zeros
    {
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      for (int q = 0; q < 16; ++q) o[(size_t)q * a.nInstruments] = z;
      continue;
    }
    gl.beginVector(gs, ln, input, a.glideVectors, a.glideDy);
    const int m = gl.mode();
    if ((m == 1) || (m == 0 && gl.isUniform()))  // not moving: one value for the whole vector
    {
      const float c = (m == 1) ? gl.target : gl.uniformValue;
      const f32x4 v = {c, c, c, c};
      for (int q = 0; q < 16; ++q) o[(size_t)q * a.nInstruments] = v;
    }
    else
    {
      // mCurrVec[n] of the previous vector feeds sample n only: all 64 loads go out together (there are few controller lanes -
      // one wavefront per SIMD - so nothing else would hide 16 round trips in a row)
      float cur[64];
      if (gl.readsCurrVec())
      {
#pragma unroll
        for (int n = 0; n < 64; ++n) cur[n] = u2f(gs[(size_t)(5 + n) * ln]);
      }
#pragma unroll
      for (int q = 0; q < 16; ++q)
      {
        f32x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = gl.nextWith(gs, ln, q * 4 + k, cur[q * 4 + k]);
        o[(size_t)q * a.nInstruments] = v;
      }
    }
    gl.endVector();
  }
  gl.store(gs, ln);
  st[(size_t)C_AWAKE * ln] = awake ? 1u : 0u;
  st[(size_t)C_INPUT * ln] = f2u(input);
}
}  // namespace

// the kernels read a lane's range as a uint4; the host router writes it as a LaneRange
static_assert(sizeof(LaneRange) == sizeof(uint4) && offsetof(LaneRange, lane) == offsetof(uint4, x) && offsetof(LaneRange, first) == offsetof(uint4, y) &&
                  offsetof(LaneRange, last) == offsetof(uint4, z) && offsetof(LaneRange, pad) == offsetof(uint4, w),
              "LaneRange is the uint4 of set_rec_ranges_kernel");

// ---- host: the event routing is mlev::EventRouter (events_router.cpp, plain C++); here its records go to the device ----------------
struct mlgpu_events
{
  mlgpu_events(mlgpu_engine* engine, size_t nInstruments, int polyphony) : e(engine), router(nInstruments, polyphony) {}
  mlgpu_engine* e;
  EventRouter router;  // key states, voice allocation, the protocol and its lane grouping, this launch's records
  double sr{0};
  float pitchBendRange{7.f}, mpePitchBendRange{24.f}, pitchGlideSeconds{0.f}, driftAmount{0.f};
  uint32_t rowMask{0xFFu};                 // mlgpu_events_set_wanted_rows
  DeviceBuffer<uint32_t> d_state;
  // [lanes]: where a lane's records of the coming launch are, {0, 0} for none. Only the lanes that have records are written per
  // launch (a few hundred of 262 144: the list goes up in kilobytes where a start offset per lane was a megabyte over PCIe
  // every block), and a kernel that consumed a lane's records puts the {0, 0} back.
  DeviceBuffer<uint2> d_recRange;
  // Two sets of upload buffers (pinned host + device) that take turns ("Staging turns"): the records of launch
  // k + 1 are routed and copied while the kernel of launch k still runs.
  struct StagingSet
  {
    PinnedBuffer<Rec> h_recs;
    DeviceBuffer<Rec> d_recs;
    PinnedBuffer<LaneRange> h_dirty;  // every lane that has records in this launch
    DeviceBuffer<LaneRange> d_dirty;
    size_t recCapacity{0}, dirtyCapacity{0};
    size_t nDirtySet{0};       // lanes whose range set_rec_ranges_kernel has set for the block in flight and no kernel has consumed yet
  };
  StagingTurns<StagingSet> stage;
  using Staging = StagingTurns<StagingSet>::Slot;  // a set and its turn
  // watched controllers (mlgpu_events_watch_controllers): lane = slot * nInstruments + instrument
  size_t ctlMaxVectors{0}, ctlCapacityVectors{0};  // longest launch allowed / what d_ctlOut was allocated for
  DeviceBuffer<float> d_ctlOut;
  DeviceBuffer<uint32_t> d_ctlState;
  struct CtlStaging  // ctlStage[i] rides on the turn of stage.set[i]: it has no event of its own
  {
    PinnedBuffer<CtlRec> h_recs;
    DeviceBuffer<CtlRec> d_recs;
    PinnedBuffer<uint32_t> h_recStart;
    DeviceBuffer<uint32_t> d_recStart;
    size_t recCapacity{0};
  } ctlStage[2];
  // e2s_ctl_kernel's outputs (mlgpu_events_prepare_for_graph): control records [T][kCtlRecWords][lanes] and the two side signals
  DeviceBuffer<uint32_t> d_ctlRecs;
  DeviceBuffer<float> d_rowP;
  DeviceBuffer<float> d_rowG;
  // ... and for the controller rows z, x, y, mod of ctlRowMask (bits 3..6): the plane of held values [T][rows][lanes], a side signal each
  DeviceBuffer<uint32_t> d_held;
  DeviceBuffer<float> d_rowC[4];
  uint32_t ctlRowMask{0};
  size_t ctlRecVectors{0};
  bool ctlRecReserved{false};  // mlgpu_events_reserve_for_graph[_rows] was called: process calls never allocate, longer blocks and rows outside the mask are refused
};

void mlgpu_graph_forget_events(mlgpu_events* ev);  // graph.hip

namespace
{
int efail(mlgpu_events* ev, int st, const std::string& what)
{
  if (ev && ev->e) ev->e->lastError = what;
  return st;
}

// the settings the kernels need, from the object's
E2SSettings deviceSettings(const mlgpu_events* ev)
{
  E2SSettings s;
  memset(&s, 0, sizeof(s));
  s.sr = ev->sr;
  s.pitchBendRange = ev->pitchBendRange;
  s.mpePitchBendRange = ev->mpePitchBendRange;
  s.driftAmount = ev->driftAmount;
  s.pitchGlideSamples = (int32_t)(ev->sr * ev->pitchGlideSeconds);  // :90
  float c[2];
  mlgpu_linear_glide_make_coeffs((float)(ev->sr * 0.02f), c);          // kGlideTimeSeconds / kControllerGlideTimeSeconds
  memcpy(&s.glideVectors, &c[0], 4);
  s.glideDy = c[1];
  mlgpu_linear_glide_make_coeffs((float)(ev->sr * 8.0f), c);           // kDriftTimeSeconds
  memcpy(&s.driftGlideVectors, &c[0], 4);
  s.driftGlideDy = c[1];
  mlgpu_linear_glide_make_coeffs((float)(int)(ev->sr * 0.02f), c);    // SmoothedController: int glideTimeInSamples = sr * 0.02f (:275)
  memcpy(&s.ctlGlideVectors, &c[0], 4);
  s.ctlGlideDy = c[1];
  s.mpe = ev->router.mpe() ? 1 : 0;
  s.polyphony = ev->router.polyphony();
  return s;
}

// what E2SArgs and E2SCtlArgs both take from a prepared block
template <class Args>
Args kernelArgs(const EventsDev& dev, size_t nVectors, uint32_t flags)
{
  Args a;
  memset(&a, 0, sizeof(a));
  a.state = dev.state;
  a.recs = (const Rec*)dev.recs;
  a.recRange = dev.recRange;
  a.lanes = dev.lanes;
  a.T = nVectors;
  a.flags = flags;
  a.s = dev.s;
  return a;
}
}  // namespace

static void freeControllers(mlgpu_events* ev)
{
  ev->d_ctlOut.reset();
  ev->d_ctlState.reset();
  for (mlgpu_events::CtlStaging& st : ev->ctlStage) st = mlgpu_events::CtlStaging();
  ev->router.unwatch();
  ev->ctlMaxVectors = 0;
}
extern "C"
{
  // What a recorded sequence may still read is DEVICE memory only (event routing is refused while recording, so no replay ever
  // touches the pinned staging or the hipEvents): the host side goes at once, the device buffers with the object. A host that
  // keeps one long-lived sequence and churns events objects so holds on to their device buffers only - state and signals -, not
  // to pinned memory and events.
  int mlgpu_events_destroy(mlgpu_events* ev)
  {
    if (!ev) return MLGPU_ERR_INVALID;
    return ev->e->release(ev, "events_destroy", [](mlgpu_events* ev) {
      mlgpu_graph_forget_events(ev);  // graphs bound to this object (mlgpu_graph_bind_events) go back to "no events object"
      for (mlgpu_events::Staging& st : ev->stage.set)
      {
        st.h_recs.reset();
        st.h_dirty.reset();
        st.turn.reset();
      }
      for (mlgpu_events::CtlStaging& st : ev->ctlStage)
      {
        st.h_recs.reset();
        st.h_recStart.reset();
      }
      ev->router = EventRouter();
    });
  }

  int mlgpu_events_clear(mlgpu_events* ev)  // EventsToSignals::clear, :330-340
  {
    if (!ev) return MLGPU_ERR_INVALID;
    ev->router.clear();
    // Voice::reset keeps the glides' and the drift's running state except what setValue(0) touches; a freshly built
    // bank and a cleared one differ only there. This implementation resets the device state completely.
    std::vector<uint32_t> st;
    ev->router.initialVoiceState(st);
    // ... except that an instrument that has seen an event stays awake, as the reference's object does (awake_ is set by the first
    // event and never cleared, :374): the router sends a lane's awake record once, so S_AWAKE must survive here - cleared with the
    // rest, an instrument that had played stayed silent for good after mlgpu_events_clear / mlgpu_events_set_protocol.
    const size_t lanes = ev->router.lanes(), group = (size_t)ev->router.group();
    for (size_t i = 0; i < ev->router.instruments(); ++i)
      if (ev->router.awakeSent(i))
        for (size_t l = 0; l < group; ++l) st[(size_t)S_AWAKE * lanes + i * group + l] = 1u;
    if (hipSetDevice(ev->e->device) != hipSuccess) return efail(ev, MLGPU_ERR_HIP, "hipSetDevice");
    return mlgpu_upload(ev->e, ev->d_state.get(), st.data(), st.size() * sizeof(uint32_t));
  }

  int mlgpu_events_create(mlgpu_engine* e, size_t nInstruments, int polyphony, mlgpu_events** out)
  {
    if (!e || !out) return MLGPU_ERR_INVALID;
    *out = nullptr;
    if (nInstruments == 0 || polyphony < 1 || polyphony > kMaxVoices)
    {
      e->lastError = "events_create: 1+ instruments, polyphony 1..16 (EventsToSignals::kMaxVoices)";
      return MLGPU_ERR_INVALID;
    }
    std::unique_ptr<mlgpu_events> ev(new (std::nothrow) mlgpu_events(e, nInstruments, polyphony));
    if (!ev) return MLGPU_ERR_OOM;
    const size_t maxLanes = ev->router.maxLanes();
    hipError_t err = hipSetDevice(e->device);
    if (err == hipSuccess) err = allocate(ev->d_state, (size_t)kStateWords * maxLanes);
    if (err == hipSuccess) err = allocate(ev->d_recRange, maxLanes);
    if (err == hipSuccess) err = hipMemsetAsync(ev->d_recRange.get(), 0, sizeof(uint2) * maxLanes, e->stream());
    for (mlgpu_events::Staging& st : ev->stage.set)
      if (err == hipSuccess) err = createTurn(st.turn);
    if (err != hipSuccess)
    {
      e->lastError = std::string("events_create: ") + hipGetErrorString(err);
      return err == hipErrorOutOfMemory ? MLGPU_ERR_OOM : MLGPU_ERR_HIP;
    }
    const int st = mlgpu_events_clear(ev.get());
    if (st != MLGPU_OK) return st;
    *out = ev.release();
    return MLGPU_OK;
  }

  static int markRecalc(mlgpu_events* ev)
  {
    if (hipSetDevice(ev->e->device) != hipSuccess) return efail(ev, MLGPU_ERR_HIP, "hipSetDevice");
    const size_t lanes = ev->router.lanes();
    return mlgpu_fill32(ev->e, ev->d_state.get() + (size_t)S_RECALC * lanes, 1u, lanes);
  }
  int mlgpu_events_set_sample_rate(mlgpu_events* ev, double sr)
  {
    if (!ev) return MLGPU_ERR_INVALID;
    ev->sr = sr;
    return markRecalc(ev);
  }
  static int reserveCtlRecs(mlgpu_events* ev, size_t nVectors, uint32_t rowMask);
  // setProtocol clears (:92-96). The buffers of events-as-graph-source-nodes are sized by the protocol's lanes: what
  // mlgpu_events_reserve_for_graph[_rows] reserved (or an unreserved object grew) is made again for the new lane count, same vectors and
  // rows, the old buffers retired through the engine - so a reserve survives the call. MLGPU_ERR_OOM: the old protocol stays in force
  // (with buffers of its own size made again; only if even that fails is the object left without, and unreserved).
  int mlgpu_events_set_protocol(mlgpu_events* ev, int mpe)
  {
    if (!ev) return MLGPU_ERR_INVALID;
    const bool was = ev->router.mpe(), now = mpe != 0;
    if (ev->ctlRecVectors && was != now)
    {
      if (ev->e->recording) return efail(ev, MLGPU_ERR_INVALID, "events_set_protocol re-makes the buffers of events_reserve_for_graph: not while recording a sequence");
      const size_t vectors = ev->ctlRecVectors;
      const uint32_t rows = ev->ctlRowMask;
      ev->router.setProtocol(now);
      const int st = reserveCtlRecs(ev, vectors, rows);
      if (st != MLGPU_OK)
      {
        ev->router.setProtocol(was);
        if (reserveCtlRecs(ev, vectors, rows) != MLGPU_OK) ev->ctlRecReserved = false;
        mlgpu_events_clear(ev);  // (the router's setProtocol dropped its key states: the device state goes with them)
        return efail(ev, st, "events_set_protocol: control records and side signals for the new protocol's lanes; the old protocol stays in force");
      }
    }
    else
      ev->router.setProtocol(now);
    return mlgpu_events_clear(ev);
  }
  int mlgpu_events_set_unison(mlgpu_events* ev, int on) { return ev ? (ev->router.setUnison(on != 0), MLGPU_OK) : MLGPU_ERR_INVALID; }
  int mlgpu_events_set_mod_cc(mlgpu_events* ev, int cc) { return ev ? (ev->router.setModCC(cc), MLGPU_OK) : MLGPU_ERR_INVALID; }
  int mlgpu_events_set_pitch_bend_semitones(mlgpu_events* ev, float f) { return ev ? (ev->pitchBendRange = f, MLGPU_OK) : MLGPU_ERR_INVALID; }
  int mlgpu_events_set_mpe_pitch_bend_semitones(mlgpu_events* ev, float f) { return ev ? (ev->mpePitchBendRange = f, MLGPU_OK) : MLGPU_ERR_INVALID; }
  int mlgpu_events_set_drift_amount(mlgpu_events* ev, float f) { return ev ? (ev->driftAmount = f, MLGPU_OK) : MLGPU_ERR_INVALID; }
  int mlgpu_events_set_pitch_glide_seconds(mlgpu_events* ev, float f)
  {
    if (!ev) return MLGPU_ERR_INVALID;
    ev->pitchGlideSeconds = f;
    return markRecalc(ev);
  }
  int mlgpu_events_set_wanted_rows(mlgpu_events* ev, unsigned mask)
  {
    if (!ev) return MLGPU_ERR_INVALID;
    ev->rowMask = mask & 0xFFu;
    return MLGPU_OK;
  }
  size_t mlgpu_events_num_voices(mlgpu_events* ev) { return ev ? ev->router.instruments() * (size_t)ev->router.polyphony() : 0; }
  int mlgpu_events_newest_voice(mlgpu_events* ev, size_t instrument) { return (ev && instrument < ev->router.instruments()) ? ev->router.newestVoice(instrument) - 1 : -2; }

  // a launch routed ahead (mlgpu_events_route_ahead) is pending: the object takes no events and no other launch until that one is made
  static const char* const kAheadPending =
      "events: a launch routed ahead (mlgpu_events_route_ahead) is pending - the next process call takes its n_vectors and start_offset, and events are added after it";
  // What every call that routes - mlgpu_events_process, mlgpu_events_prepare_for_graph, mlgpu_events_route_ahead - refuses before the
  // router consumes a block's events: one list for the three
  static int checkBeforeRouting(mlgpu_events* ev, size_t nVectors)
  {
    if (ev->e->recording) return efail(ev, MLGPU_ERR_INVALID, "events route on the host: not while recording a sequence");
    if (ev->sr == 0) return efail(ev, MLGPU_ERR_INVALID, "events: no sample rate (the reference does nothing, :385)");
    if (!ev->router.watched().empty() && nVectors > ev->ctlMaxVectors)
      return efail(ev, MLGPU_ERR_RANGE, "events_process: more DSPVectors than events_watch_controllers reserved the controller signals for");
    return MLGPU_OK;
  }

  int mlgpu_events_add_event(mlgpu_events* ev, size_t instrument, const mlgpu_event* e)  // addEvent, :367-372
  {
    if (!ev || !e) return MLGPU_ERR_INVALID;
    if (instrument >= ev->router.instruments()) return efail(ev, MLGPU_ERR_RANGE, "events_add_event: instrument out of range");
    if (ev->router.aheadPending()) return efail(ev, MLGPU_ERR_INVALID, kAheadPending);
    ev->router.addEvent(instrument, *e);
    return MLGPU_OK;
  }
  int mlgpu_events_add_events(mlgpu_events* ev, const uint32_t* instruments, const mlgpu_event* events, size_t n)  // a block's events in one call
  {
    if (!ev || (n && (!instruments || !events))) return MLGPU_ERR_INVALID;
    for (size_t i = 0; i < n; ++i)
      if (instruments[i] >= ev->router.instruments()) return efail(ev, MLGPU_ERR_RANGE, "events_add_events: instrument out of range");
    if (n && ev->router.aheadPending()) return efail(ev, MLGPU_ERR_INVALID, kAheadPending);
    for (size_t i = 0; i < n; ++i) ev->router.addEvent(instruments[i], events[i]);
    return MLGPU_OK;
  }
  int mlgpu_events_clear_events(mlgpu_events* ev)  // clearEvents, once per host block (MLSignalProcessBuffer.cpp:89)
  {
    if (!ev) return MLGPU_ERR_INVALID;
    ev->router.clearEvents();
    return MLGPU_OK;
  }

  // The controller lanes of one launch: their records uploaded into the staging set of this launch (the one that goes with the set
  // prepare() has just taken), then ctl_kernel on the engine's stream - ahead of the kernel that reads the signals.
  static int processControllers(mlgpu_events* ev, size_t nVectors, int stageIdx, const E2SSettings& s)
  {
    mlgpu_engine* e = ev->e;
    const EventRouter& router = ev->router;
    mlgpu_events::CtlStaging& sg = ev->ctlStage[stageIdx];
    const size_t lanes = router.ctlLanes(), nRecs = router.ctlRecordCount();
    if (!growPair(sg.h_recs, sg.d_recs, sg.recCapacity, nRecs + 1, std::max<size_t>(1024, 2 * (nRecs + 1)))) return efail(ev, MLGPU_ERR_OOM, "events_process: controller record buffer");
    router.packControllers(sg.h_recs.get(), sg.h_recStart.get());
    hipError_t err = hipMemcpyAsync(sg.d_recStart.get(), sg.h_recStart.get(), sizeof(uint32_t) * (lanes + 1), hipMemcpyHostToDevice, e->stream());
    if (err == hipSuccess && nRecs) err = hipMemcpyAsync(sg.d_recs.get(), sg.h_recs.get(), sizeof(CtlRec) * nRecs, hipMemcpyHostToDevice, e->stream());
    if (err != hipSuccess) return efail(ev, MLGPU_ERR_HIP, std::string("events_process controller upload: ") + hipGetErrorString(err));
    CtlArgs a;
    a.state = ev->d_ctlState.get();
    a.recs = sg.d_recs.get();
    a.recStart = sg.d_recStart.get();
    a.out = ev->d_ctlOut.get();
    a.nInstruments = router.instruments();
    a.lanes = lanes;
    a.T = nVectors;
    a.slotStride = 64 * ev->ctlCapacityVectors * router.instruments();  // (the capacity, not the current limit: a slot's signal stays where it is while the buffer is not replaced)
    a.glideVectors = s.ctlGlideVectors;
    a.glideDy = s.ctlGlideDy;
    hipLaunchKernelGGL(ctl_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, e->stream(), a);
    err = hipGetLastError();
    if (err != hipSuccess) return efail(ev, MLGPU_ERR_HIP, std::string("events_process controller launch: ") + hipGetErrorString(err));
    return MLGPU_OK;
  }

  // The per-lane record ranges are device state: set from the block's lane list, cleared by the kernel that consumes them. A block that
  // fails after they were set and before that kernel ran would leave them pointing into a staging buffer the NEXT block does not
  // use: put them back to "no records" (stream-ordered, the list is still in sg.d_dirty). This is the way out of every block that
  // fails once its set was taken: whatever was enqueued - uploads, the clearing pass - reads the set, so the turn is submitted.
  static void abandonRanges(mlgpu_events* ev, mlgpu_events::Staging& sg)
  {
    if (sg.nDirtySet)
    {
      hipLaunchKernelGGL(clear_rec_ranges_kernel, dim3((unsigned)((sg.nDirtySet + 255) / 256)), dim3(256), 0, ev->e->stream(), (const uint4*)sg.d_dirty.get(), sg.nDirtySet, ev->d_recRange.get());
      (void)hipGetLastError();
      sg.nDirtySet = 0;
    }
    sg.turn.submitted(ev->e->stream());
  }

  // One block of nVectors DSPVectors starting at frame startOffset of the event times, up to the kernel that consumes it: the block's
  // events routed into per-voice records, the records uploaded (asynchronously, into the staging set that is free), the controller
  // lanes run, the settings the device needs. The caller launches the consuming kernel - e2s_kernel, or a voice graph whose pitch and
  // gate rows are source nodes (graph.hip) - and then calls launched().
  static int prepare(mlgpu_events* ev, size_t nVectors, int startOffset, EventsDev& dev, mlgpu_events::Staging*& sgOut)
  {
    mlgpu_engine* e = ev->e;
    EventRouter& router = ev->router;
    // (the callers have made checkBeforeRouting's checks)
    // (before the wait below: block k + 1 is routed while block k runs; a launch routed ahead keeps its records)
    if (!router.route(nVectors, startOffset)) return efail(ev, MLGPU_ERR_INVALID, kAheadPending);
    if (hipSetDevice(e->device) != hipSuccess) return efail(ev, MLGPU_ERR_HIP, "hipSetDevice");
    sgOut = ev->stage.take();
    if (!sgOut) return efail(ev, MLGPU_ERR_HIP, "events_process: waiting for the launch before last");
    mlgpu_events::Staging& sg = *sgOut;
    const auto giveUp = [&](int st, const std::string& what) {
      abandonRanges(ev, sg);
      return efail(ev, st, what);
    };
    const size_t nRecs = router.recordCount(), nDirty = router.dirtyLaneCount();
    if (!growPair(sg.h_recs, sg.d_recs, sg.recCapacity, nRecs + 1, std::max<size_t>(4096, 2 * (nRecs + 1)))) return giveUp(MLGPU_ERR_OOM, "events_process: record buffer");
    if (!growPair(sg.h_dirty, sg.d_dirty, sg.dirtyCapacity, nDirty, std::max<size_t>(1024, 2 * nDirty))) return giveUp(MLGPU_ERR_OOM, "events_process: lane list");
    router.pack(sg.h_recs.get(), sg.h_dirty.get());
    hipError_t cerr = hipSuccess;
    if (nDirty) cerr = hipMemcpyAsync(sg.d_dirty.get(), sg.h_dirty.get(), sizeof(LaneRange) * nDirty, hipMemcpyHostToDevice, e->stream());
    if (cerr == hipSuccess && nRecs) cerr = hipMemcpyAsync(sg.d_recs.get(), sg.h_recs.get(), sizeof(Rec) * nRecs, hipMemcpyHostToDevice, e->stream());
    if (cerr == hipSuccess && nDirty)
    {
      hipLaunchKernelGGL(set_rec_ranges_kernel, dim3((unsigned)((nDirty + 255) / 256)), dim3(256), 0, e->stream(), (const uint4*)sg.d_dirty.get(), nDirty, ev->d_recRange.get());
      cerr = hipGetLastError();
      if (cerr == hipSuccess) sg.nDirtySet = nDirty;
    }
    if (cerr != hipSuccess) return giveUp(MLGPU_ERR_HIP, std::string("events_process upload: ") + hipGetErrorString(cerr));

    dev.s = deviceSettings(ev);
    const int cst = router.watched().empty() ? MLGPU_OK : processControllers(ev, nVectors, (int)(&sg - ev->stage.set), dev.s);
    if (cst != MLGPU_OK)
    {
      abandonRanges(ev, sg);
      return cst;
    }
    dev.ctl = nullptr;
    dev.rowP = dev.rowG = nullptr;
    dev.held = nullptr;
    for (const float4*& r : dev.rowC) r = nullptr;
    dev.ctlRowMask = 0;
    dev.state = ev->d_state.get();
    dev.recs = sg.d_recs.get();
    dev.recRange = ev->d_recRange.get();
    dev.lanes = router.lanes();
    dev.group = router.group();
    dev.slotBase = router.slotBase();
    return MLGPU_OK;
  }
  static int launched(mlgpu_events* ev, mlgpu_events::Staging& sg)
  {
    sg.nDirtySet = 0;  // (the consuming kernel clears the ranges it read)
    sg.turn.submitted(ev->e->stream());  // no wait here: the host goes on routing the next block while this one runs
    return MLGPU_OK;
  }

  // processVector (:376-466) for n_vectors consecutive DSPVectors starting at frame start_offset of the event times.
  int mlgpu_events_process(mlgpu_events* ev, size_t nVectors, int startOffset, float* const* d_outputs, int layout)
  {
    if (!ev || !d_outputs) return MLGPU_ERR_INVALID;
    mlgpu_engine* e = ev->e;
    if (nVectors == 0) return MLGPU_OK;
    if (const int st = checkBeforeRouting(ev, nVectors)) return st;
    if (layout < 0 || layout > MLGPU_LAYOUT_VOICE_MAJOR) return efail(ev, MLGPU_ERR_INVALID, "events_process: bad layout");
    // everything that can be refused is refused BEFORE the router consumes the block's note events: after this point the
    // host-side voice allocator (keys, creatorKeyIdx, sustain pedal, lastFreeVoiceFound) has advanced, and an error return
    // (allocation, upload, launch) leaves host and device voice state out of step - reset the object with
    // mlgpu_events_set_protocol / a fresh mlgpu_events if that ever happens.
    for (int r = 0; r < 8; ++r)
    {
      if (d_outputs[r] && ((uintptr_t)d_outputs[r] & 15)) return efail(ev, MLGPU_ERR_INVALID, "events_process: misaligned output");
      if (d_outputs[r] && !((ev->rowMask >> r) & 1u)) return efail(ev, MLGPU_ERR_INVALID, "events_process: an output was passed for a row outside events_set_wanted_rows");
    }
    if (ev->router.aheadPending() && !ev->router.aheadIs(nVectors, startOffset)) return efail(ev, MLGPU_ERR_INVALID, kAheadPending);
    EventsDev dev;
    mlgpu_events::Staging* sg = nullptr;
    const int pst = prepare(ev, nVectors, startOffset, dev, sg);
    if (pst != MLGPU_OK) return pst;
    E2SArgs a = kernelArgs<E2SArgs>(dev, nVectors, e->kflags);
    const size_t lanes = dev.lanes;
    const size_t V = mlgpu_events_num_voices(ev);
    for (int r = 0; r < 8; ++r) a.out[r] = makeView(d_outputs[r], layout, V, nVectors);
    a.rowMask = ev->rowMask;
    a.group = ev->router.group();
    a.slotBase = ev->router.slotBase();
    a.polyphony = ev->router.polyphony();
    if ((a.rowMask & ~3u) == 0)
      hipLaunchKernelGGL(e2s_kernel<true>, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, e->stream(), a);
    else
      hipLaunchKernelGGL(e2s_kernel<false>, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, e->stream(), a);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess)
    {
      abandonRanges(ev, *sg);
      return efail(ev, MLGPU_ERR_HIP, std::string("events_process launch: ") + hipGetErrorString(err));
    }
    return launched(ev, *sg);
  }

  // control records [T][kCtlRecWords][lanes] + the two side signals [64 T][lanes] of e2s_ctl_kernel for blocks of up to nVectors
  // ... and, for each of the rows z, x, y, mod in rowMask (bits 3..6), a held word [T][lanes] and a side signal [64 T][lanes]
  static int reserveCtlRecs(mlgpu_events* ev, size_t nVectors, uint32_t rowMask)
  {
    mlgpu_engine* e = ev->e;
    const size_t lanes = ev->router.lanes();
    rowMask &= kCtlRowsMask;
    if (hipSetDevice(e->device) != hipSuccess) return efail(ev, MLGPU_ERR_HIP, "hipSetDevice");
    hipStreamSynchronize(e->stream());
    // recorded graph launches have these pointers baked in: the old buffers are retired, the new ones serve from now on
    e->retire(std::move(ev->d_ctlRecs));
    e->retire(std::move(ev->d_rowP));
    e->retire(std::move(ev->d_rowG));
    e->retire(std::move(ev->d_held));
    for (DeviceBuffer<float>& b : ev->d_rowC) e->retire(std::move(b));
    ev->ctlRecVectors = 0;
    ev->ctlRowMask = 0;
    bool ok = allocate(ev->d_ctlRecs, kCtlRecWords * nVectors * lanes) == hipSuccess && allocate(ev->d_rowP, 64 * nVectors * lanes) == hipSuccess &&
              allocate(ev->d_rowG, 64 * nVectors * lanes) == hipSuccess;
    if (ok && rowMask) ok = allocate(ev->d_held, (size_t)ctl_row_count(rowMask) * nVectors * lanes) == hipSuccess;
    for (int r = 3; ok && r <= 6; ++r)
      if ((rowMask >> r) & 1u) ok = allocate(ev->d_rowC[r - 3], 64 * nVectors * lanes) == hipSuccess;
    if (!ok)
    {
      ev->d_ctlRecs.reset();
      ev->d_rowP.reset();
      ev->d_rowG.reset();
      ev->d_held.reset();
      for (DeviceBuffer<float>& b : ev->d_rowC) b.reset();
      return efail(ev, MLGPU_ERR_OOM, "events as graph source nodes: control records and side signals");
    }
    ev->ctlRecVectors = nVectors;
    ev->ctlRowMask = rowMask;
    return MLGPU_OK;
  }
  int mlgpu_events_reserve_for_graph_rows(mlgpu_events* ev, size_t maxVectors, unsigned rowMask)
  {
    if (!ev || maxVectors == 0) return MLGPU_ERR_INVALID;
    if (rowMask & ~0x7Fu) return efail(ev, MLGPU_ERR_UNSUPPORTED, "events_reserve_for_graph_rows: rows 0 (pitch) to 6 (mod) can be source nodes of a graph");
    if (ev->e->recording) return efail(ev, MLGPU_ERR_INVALID, "events_reserve_for_graph allocates: not while recording a sequence");
    if (maxVectors != ev->ctlRecVectors || (rowMask & kCtlRowsMask) != ev->ctlRowMask)
    {
      const int st = reserveCtlRecs(ev, maxVectors, rowMask);
      if (st != MLGPU_OK) return st;
    }
    ev->ctlRecReserved = true;
    return MLGPU_OK;
  }
  int mlgpu_events_reserve_for_graph(mlgpu_events* ev, size_t maxVectors) { return mlgpu_events_reserve_for_graph_rows(ev, maxVectors, 3u); }
  size_t mlgpu_events_graph_reserve_bytes_rows(mlgpu_events* ev, size_t maxVectors, unsigned rowMask)
  {
    if (!ev || (rowMask & ~0x7Fu)) return 0;
    const size_t perRow = sizeof(uint32_t) + sizeof(float) * 64;  // a held word and 64 frames of side signal
    return (sizeof(uint32_t) * kCtlRecWords + 2 * sizeof(float) * 64 + perRow * (size_t)ctl_row_count(rowMask)) * maxVectors * ev->router.lanes();
  }
  size_t mlgpu_events_graph_reserve_bytes(mlgpu_events* ev, size_t maxVectors) { return mlgpu_events_graph_reserve_bytes_rows(ev, maxVectors, 3u); }

  // for graph.hip: a graph whose event rows are bound to this object (mlgpu_graph_bind_events)
  // rowMask: the graph's event rows (bit r = row r; only z, x, y, mod - bits 3..6 - need memory and work of their own here)
  // mpeForm: the graph's kernel is the MPE-capable form (mlgpu_graph_enable_mpe_events); every other kernel takes a voice for a lane
  int mlgpu_events_prepare_for_graph(mlgpu_events* ev, size_t nVectors, int startOffset, unsigned rowMask, int mpeForm, EventsDev* dev, void** staging)
  {
    if (!ev || !dev || !staging) return MLGPU_ERR_INVALID;
    if (nVectors == 0) return MLGPU_OK;
    if (const int st = checkBeforeRouting(ev, nVectors)) return st;
    const bool mpe = ev->router.mpe();
    if (mpe && !mpeForm) return efail(ev, MLGPU_ERR_UNSUPPORTED, "events as graph source nodes: MIDI protocol only (one lane per voice)");
    if (ev->router.aheadPending() && !ev->router.aheadIs(nVectors, startOffset)) return efail(ev, MLGPU_ERR_INVALID, kAheadPending);
    mlgpu_engine* e = ev->e;
    const size_t lanes = ev->router.lanes();
    // the control records and the two side signals of e2s_ctl_kernel: sized by mlgpu_events_reserve_for_graph at setup. An object that
    // was never reserved grows them here on the first / a longer block (a setup-time convenience: it waits for the stream and allocates);
    // once a host has reserved, a longer block is refused before the router consumes its events and nothing is ever allocated here.
    // The same goes for the rows: a graph with a controller row outside the reserved mask is refused here, an unreserved object grows.
    const uint32_t ctlRows = rowMask & kCtlRowsMask, missing = ctlRows & ~ev->ctlRowMask;
    if (nVectors > ev->ctlRecVectors || missing)
    {
      if (ev->ctlRecReserved && nVectors > ev->ctlRecVectors)
        return efail(ev, MLGPU_ERR_RANGE, "graph_process_events: more DSPVectors than mlgpu_events_reserve_for_graph reserved the control records for");
      if (ev->ctlRecReserved)
      {
        static const char* const names[] = {"3 (z)", "4 (x)", "5 (y)", "6 (mod)"};
        return efail(ev, MLGPU_ERR_INVALID, std::string("graph_process_events: the graph reads event row ") + names[__builtin_ctz(missing) - 3] +
                                                ", which is outside the row mask of mlgpu_events_reserve_for_graph_rows");
      }
      const int rst = reserveCtlRecs(ev, std::max(nVectors, ev->ctlRecVectors), ctlRows | ev->ctlRowMask);
      if (rst != MLGPU_OK) return rst;
    }
    mlgpu_events::Staging* sg = nullptr;
    const int st = prepare(ev, nVectors, startOffset, *dev, sg);
    *staging = sg;
    if (st != MLGPU_OK) return st;
    E2SCtlArgs a = kernelArgs<E2SCtlArgs>(*dev, nVectors, e->kflags);
    a.ctl = ev->d_ctlRecs.get();
    a.rowP = (float4*)ev->d_rowP.get();
    a.rowG = (float4*)ev->d_rowG.get();
    a.group = dev->group;
    a.slotBase = dev->slotBase;
    if (ctlRows)  // the instance that also runs the controller glides the graph reads
    {
      a.held = ev->d_held.get();
      for (int r = 0; r < 4; ++r) a.rowC[r] = (float4*)ev->d_rowC[r].get();
      a.rowMask = ctlRows;
      if (mpe) hipLaunchKernelGGL(e2s_ctl_rows_mpe_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, e->stream(), a);
      else hipLaunchKernelGGL(e2s_ctl_rows_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, e->stream(), a);
    }
    else if (mpe)
      hipLaunchKernelGGL(e2s_ctl_mpe_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, e->stream(), a);
    else
      hipLaunchKernelGGL(e2s_ctl_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, e->stream(), a);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess)
    {
      abandonRanges(ev, *sg);
      return efail(ev, MLGPU_ERR_HIP, std::string("events control kernel launch: ") + hipGetErrorString(err));
    }
    dev->ctl = ev->d_ctlRecs.get();
    dev->rowP = (const float4*)ev->d_rowP.get();
    dev->rowG = (const float4*)ev->d_rowG.get();
    if (ctlRows)
    {
      dev->held = ev->d_held.get();
      for (int r = 0; r < 4; ++r) dev->rowC[r] = (const float4*)ev->d_rowC[r].get();
      dev->ctlRowMask = ctlRows;
    }
    return MLGPU_OK;
  }
  // The router's work of the coming launch, now: the host reads mlgpu_events_sounding_voices and makes its voice list before the
  // launch. Every check a process call makes before it routes is made here, so the launch that follows has nothing left to refuse
  // in this object but other values than these.
  int mlgpu_events_route_ahead(mlgpu_events* ev, size_t nVectors, int startOffset)
  {
    if (!ev) return MLGPU_ERR_INVALID;
    if (nVectors == 0) return efail(ev, MLGPU_ERR_INVALID, "events_route_ahead: no DSPVectors (a process call of none routes nothing)");
    if (startOffset < 0) return efail(ev, MLGPU_ERR_INVALID, "events_route_ahead: negative frame offset");
    if (ev->router.aheadPending()) return efail(ev, MLGPU_ERR_INVALID, kAheadPending);
    if (const int st = checkBeforeRouting(ev, nVectors)) return st;
    if (ev->ctlRecReserved && nVectors > ev->ctlRecVectors)
      return efail(ev, MLGPU_ERR_RANGE, "events_route_ahead: more DSPVectors than mlgpu_events_reserve_for_graph reserved the control records for");
    ev->router.routeAhead(nVectors, startOffset);
    return MLGPU_OK;
  }
  int mlgpu_events_sounding_voices(mlgpu_events* ev, uint32_t* h_voices, size_t capacity, size_t* n)
  {
    if (!ev || !n || (capacity && !h_voices)) return MLGPU_ERR_INVALID;
    *n = 0;
    if (ev->router.mpe()) return efail(ev, MLGPU_ERR_UNSUPPORTED, "events_sounding_voices: MIDI protocol only (a voice index is a lane)");
    if (!ev->router.soundingVoices(h_voices, capacity, n))
      return efail(ev, MLGPU_ERR_RANGE, "events_sounding_voices: " + std::to_string(*n) + " voices sound, the caller's memory holds " + std::to_string(capacity));
    return MLGPU_OK;
  }
  // ... in either protocol, as graph voice indices instrument * polyphony + voice (EventRouter::soundingGraphVoices): what a host of
  // mlgpu_graph_enable_voice_list_mpe_events makes its list of. Under MIDI the set above.
  int mlgpu_events_sounding_graph_voices(mlgpu_events* ev, uint32_t* h_voices, size_t capacity, size_t* n)
  {
    if (!ev || !n || (capacity && !h_voices)) return MLGPU_ERR_INVALID;
    *n = 0;
    if (!ev->router.soundingGraphVoices(h_voices, capacity, n))
      return efail(ev, MLGPU_ERR_RANGE, "events_sounding_graph_voices: " + std::to_string(*n) + " voices sound, the caller's memory holds " + std::to_string(capacity));
    return MLGPU_OK;
  }
  // the graph's voice kernel could not be launched after prepare_for_graph had succeeded (e2s_ctl_kernel has consumed the lanes' record
  // ranges by then, or will: abandonRanges puts back whatever it has not, stream-ordered, and submits the staging set's turn)
  int mlgpu_events_abandoned_by_graph(mlgpu_events* ev, void* staging)
  {
    if (!ev || !staging) return MLGPU_ERR_INVALID;
    abandonRanges(ev, *(mlgpu_events::Staging*)staging);
    return MLGPU_OK;
  }
  int mlgpu_events_launched_by_graph(mlgpu_events* ev, void* staging)
  {
    if (!ev || !staging) return MLGPU_ERR_INVALID;
    return launched(ev, *(mlgpu_events::Staging*)staging);
  }
  int mlgpu_events_watch_controllers(mlgpu_events* ev, const int* numbers, int n, size_t maxVectors)
  {
    if (!ev || n < 0 || (n > 0 && !numbers)) return MLGPU_ERR_INVALID;
    mlgpu_engine* e = ev->e;
    if (e->recording) return efail(ev, MLGPU_ERR_INVALID, "events_watch_controllers allocates: not while recording a sequence");
    if (n > MLGPU_EVENTS_MAX_WATCHED_CONTROLLERS) return efail(ev, MLGPU_ERR_RANGE, "events_watch_controllers: at most MLGPU_EVENTS_MAX_WATCHED_CONTROLLERS");
    if (n > 0 && maxVectors == 0) return efail(ev, MLGPU_ERR_INVALID, "events_watch_controllers: max_vectors = the longest launch, at least 1");
    for (int i = 0; i < n; ++i)
    {
      if (numbers[i] < 0 || numbers[i] >= kNumControllers) return efail(ev, MLGPU_ERR_RANGE, "events_watch_controllers: controller numbers 0..128");
      for (int j = 0; j < i; ++j)
        if (numbers[j] == numbers[i]) return efail(ev, MLGPU_ERR_INVALID, "events_watch_controllers: a controller number twice");
    }
    if (hipSetDevice(e->device) != hipSuccess) return efail(ev, MLGPU_ERR_HIP, "hipSetDevice");
    hipStreamSynchronize(e->stream());
    if (n > 0 && ev->router.watched() == std::vector<int>(numbers, numbers + n))  // the same controllers: only the reserved length changes
    {
      if (maxVectors <= ev->ctlCapacityVectors)  // the signals' pointers (mlgpu_events_controller_signal) are only ever replaced to grow
      {
        ev->ctlMaxVectors = maxVectors;
        return MLGPU_OK;
      }
      if (e->liveSequences > 0)
        return efail(ev, MLGPU_ERR_INVALID, "events_watch_controllers would move the controller signals that recorded sequences of this engine may read: destroy them first");
      DeviceBuffer<float> fresh;
      if (allocate(fresh, 64 * maxVectors * ev->router.ctlLanes()) != hipSuccess) return efail(ev, MLGPU_ERR_OOM, "events_watch_controllers: controller signals");
      hipMemsetAsync(fresh.get(), 0, sizeof(float) * 64 * maxVectors * ev->router.ctlLanes(), e->stream());
      ev->d_ctlOut = std::move(fresh);
      ev->ctlMaxVectors = ev->ctlCapacityVectors = maxVectors;
      return MLGPU_OK;
    }
    if (e->liveSequences > 0 && ev->d_ctlOut)
      return efail(ev, MLGPU_ERR_INVALID, "events_watch_controllers would free controller signals that recorded sequences of this engine may read: destroy them first");
    freeControllers(ev);
    if (n == 0) return MLGPU_OK;
    ev->router.watch(numbers, n);
    ev->ctlMaxVectors = ev->ctlCapacityVectors = maxVectors;
    const size_t lanes = ev->router.ctlLanes();
    hipError_t err = allocate(ev->d_ctlOut, 64 * maxVectors * lanes);
    if (err == hipSuccess) err = allocate(ev->d_ctlState, (size_t)kCtlWords * lanes);
    for (mlgpu_events::CtlStaging& st : ev->ctlStage)
    {
      if (err == hipSuccess) err = allocate(st.d_recStart, lanes + 1);
      if (err == hipSuccess) err = allocate(st.h_recStart, lanes + 1);
    }
    if (err == hipSuccess) err = hipMemsetAsync(ev->d_ctlOut.get(), 0, sizeof(float) * 64 * maxVectors * lanes, e->stream());
    if (err != hipSuccess)
    {
      freeControllers(ev);
      return efail(ev, err == hipErrorOutOfMemory ? MLGPU_ERR_OOM : MLGPU_ERR_HIP, std::string("events_watch_controllers: ") + hipGetErrorString(err));
    }
    std::vector<uint32_t> st;
    ev->router.initialControllerState(st);
    return mlgpu_upload(e, ev->d_ctlState.get(), st.data(), st.size() * sizeof(uint32_t));
  }
  const float* mlgpu_events_controller_signal(mlgpu_events* ev, int slot)
  {
    if (!ev || slot < 0 || (size_t)slot >= ev->router.watched().size()) return nullptr;
    return ev->d_ctlOut.get() + (size_t)slot * 64 * ev->ctlCapacityVectors * ev->router.instruments();
  }
  int mlgpu_events_is_midi(mlgpu_events* ev) { return (ev && !ev->router.mpe()) ? 1 : 0; }
  mlgpu_engine* mlgpu_events_engine(mlgpu_events* ev) { return ev ? ev->e : nullptr; }
}
