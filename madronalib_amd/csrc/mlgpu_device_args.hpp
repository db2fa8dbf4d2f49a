// mlgpu_device_args.hpp — plain-old-data kernel argument blocks shared by the ahead-of-time
// kernels (chains.hip), the run-time generated graph kernels (graph.hip via hiprtc) and the host.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <stddef.h>
#endif
#include <stdint.h>

// signal addressing in float4 units: element (vector t, quad q, voice v) lives at
//   base + t*strideT + q*strideQ + v*strideV        (layouts: mlgpu_layout in include/mlgpu.h)
struct SignalView
{
  float4* base;
  size_t strideT, strideQ, strideV;
};

// bits of the `flags` word every arithmetic kernel receives
#define MLGPU_KFLAG_FLUSH_DENORMALS 1u  // run with f32 denormal sources and results flushed (mlgpu_engine_set_flush_denormals)
// the launch is at most one workgroup per CU, so each SIMD is expected to hold one wavefront of this kernel: they take no turns at the
// priority levels (mldsp_kernels.hpp: stream_voice). Set by the host for the kernels of a bank launch that goes out in parts (capi.hip).
#define MLGPU_KFLAG_LONE_WAVEFRONTS 2u
// host-side only (read by the cascade launchers, chains.hip): which form of an SVF cascade to run (mlgpu_engine_set_cascade_lanes).
// 0 = by bank size, 1 / 2 / 4 = that many wavefront lanes per channel, 7 = the round-2 kernel (cascade_kernel)
#define MLGPU_KFLAG_CASCADE_SHIFT 8
#define MLGPU_KFLAG_CASCADE_MASK (7u << MLGPU_KFLAG_CASCADE_SHIFT)

// a turn of the wavefronts of a SIMD at the priority levels (mldsp_math.hpp: take_turns_by_clock) lasts 2^13 ticks of 10 ns:
// 82 us, the best of 2^7 .. 2^18 (profiles/r04_take_turns.txt). The chain kernels and the graph generator both use it.
constexpr int kTurnClockShift = 13;

struct ChainArgs
{
  const float* coeffs;   // [NC][V]
  uint32_t* state;       // [NS][V]
  const float* inConst;  // [V] or nullptr
  SignalView in;         // base == nullptr when no streamed input
  SignalView out;
  size_t V, T;
  const float* impulseTable;
  uint32_t flags;  // MLGPU_KFLAG_*
  float* mix;      // chain_mix_kernel (mldsp_kernels.hpp: MixSink): the rows of 64-voice group sums, [(group * T + t) * 64 + sample] (mlgpu_mixdown's first stage); else unused
  const float* mixGains;  // ... and the per-voice gains the voices are scaled by before (mlgpu_mixdown's d_gains), or nullptr
  // chain_group_kernel (GroupSink; it scales by mixGains too, before its group sums): voice v reads row v >> inGroupShift of `in`, and
  // `out` is a signal of V / OUT_G channels; else unused
  uint32_t inGroupShift = 0;
  // chain_listed_kernel / chain_listed_mix_kernel (mlgpu_bank_process_listed; chain_kernel_body's LISTED with StoreSink / MixSink): lane i of the launch runs voice voiceList[i] of a
  // bank of tableStride voices - V is then the list's length, coeffs / state / inConst / in / mixGains are read at the voice, out /
  // mix / peaks written at i; peaks[i] (or nullptr) gets the largest |sample| bit pattern of the launch. Else unused.
  // chain_kernel itself reads tableStride too: non-zero, the launch is a window [v0, v0 + V) of a bank of tableStride voices - coeffs,
  // state, inConst and out are the host's pointers moved to voice v0, the table rows are tableStride apart (mlgpu_bank_process in two parts)
  const uint32_t* voiceList = nullptr;
  size_t tableStride = 0;
  uint32_t* peaks = nullptr;
  // chain_listed_group_kernel (mlgpu_bank_process_listed_groups; SegmentSink): the launch is V = N lanes laid out by the host (voice_list.hpp:
  // mlvl::planGroups), lane l's plan entry is the four words lanePlan[4 l .. 4 l + 3], one 16-byte load:
  //   .x voice (0xFFFFFFFF: a pad lane, which runs nothing)   .y list position i (peaks[i])
  //   .z output row j of `out`, a signal of J rows             .w rank | length << 8 of the lane in its segment
  // A segment - the listed voices of one instrument - never crosses a multiple of 64 lanes. coeffs / state / inConst / mixGains are
  // read at the voice, `in` at row voice >> inGroupShift, tableStride is the bank's voice count. Else unused.
  const uint32_t* lanePlan = nullptr;
  // chain_mix_channels_kernel / chain_listed_mix_channels_kernel (mlgpu_bank_process_mixdown_channels; MixChannelsSink): the voices'
  // sum once per channel, each voice scaled by its gain for that channel. mixGains is then [mixChannels][voices of the bank]
  // (required); mixChannelStride is the stride between the channels' regions of whatever the form sums into, in floats: channel
  // c's rows of group sums are at mix + c * mixChannelStride. chain_group_channels_kernel / chain_listed_group_channels_kernel
  // (mlgpu_bank_process_groups_channels, _listed_groups_channels; GroupChannelsSink, SegmentChannelsSink) read both the same way:
  // channel c's signal of rows is at out.base + c * mixChannelStride. Else unused.
  uint32_t mixChannels = 1;
  size_t mixChannelStride = 0;
};

// EventsToSignals settings the device needs (events.hip, mldsp_events.hpp)
struct E2SSettings
{
  double sr;
  float pitchBendRange, mpePitchBendRange, driftAmount;
  int32_t pitchGlideSamples;           // sr * pitchGlideTimeInSeconds (:90)
  int32_t glideVectors;  float glideDy;        // bend / mod / x / y / z / controllers: sr * 0.02 s (:97-101, 275)
  int32_t driftGlideVectors;  float driftGlideDy;  // sr * 8 s (:103)
  int32_t ctlGlideVectors;  float ctlGlideDy;      // SmoothedController: int(sr * 0.02 s) samples (:274-275) — truncated first
  int32_t mpe;                         // protocol
  int32_t polyphony;                   // voices per instrument: the vox row is (float)(voice % polyphony) under the MIDI protocol (:302)
};

// the EventsToSignals object whose pitch / gate rows are source nodes of a graph (mlgpu_graph_bind_events); state == nullptr: none
struct EventsDev
{
  uint32_t* state;           // [kStateWords][lanes]
  const void* recs;          // mlev::Rec: this launch's records, grouped by lane, time-ordered inside a lane
  uint2* recRange;           // [lanes]: a lane's records of this launch are recs[x .. y)
  size_t lanes;
  E2SSettings s;
  // the launch's control records [T][kCtlRecWords][lanes] and the two side signals (QUAD layout) of e2s_ctl_kernel: what a voice
  // kernel expands to audio rate (mlev::CtlVoice); null for mlgpu_events_process, which writes whole rows
  const uint32_t* ctl;
  const float4* rowP;
  const float4* rowG;
  // the controller rows z, x, y, mod (rows 3..6) of a graph that has them as source nodes (mlev::CtlRows): ctlRowMask has bit r for
  // row r of this launch, `held` is the plane [T][rows of the mask, ascending][lanes] of one value per vector, rowC[r - 3] row r's side
  // signal (QUAD layout, as rowP), written for the vectors whose C_FLAGS has CF_ROW(r) only. Null / 0 without such rows.
  const uint32_t* held;
  const float4* rowC[4];
  uint32_t ctlRowMask;
  // the protocol's lane layout (EventRouter::setProtocol): lane = instrument * group + (slot - slotBase), slot 0 the MPE main voice,
  // slots 1..polyphony the playing voices. MIDI: group = polyphony, slotBase = 1 (lane == voice); MPE: group = nextpow2(polyphony + 1),
  // slotBase = 0; s.mpe says which. Read by the MPE-capable forms only (mlev::CtlVoiceMpe, mlev::CtlRowsMpe).
  int32_t group, slotBase;
};

// a fused graph kernel: up to MLGPU_GRAPH_MAX_INPUTS (32) streamed inputs, MLGPU_GRAPH_MAX_OUTPUTS (8) outputs, per-voice constants [P][V]
#define MLGPU_GRAPH_MAX_INPUTS 32
#define MLGPU_GRAPH_MAX_OUTPUTS 8
#define MLGPU_GRAPH_MAX_CONTROLS 8
struct GraphArgs
{
  const float* coeffs;  // [NC][V]
  uint32_t* state;      // [NS][V]
  const float* params;  // [NP][V] per-voice constants (broadcast as DSPVector(f))
  SignalView in[MLGPU_GRAPH_MAX_INPUTS];
  SignalView out[MLGPU_GRAPH_MAX_OUTPUTS];
  const float* ctl[MLGPU_GRAPH_MAX_CONTROLS];  // control-rate inputs, [T][V]: one float per DSPVector per voice
  float* mem;  // delay-line rings of all delay nodes, [sample][V] each
  size_t V, T;
  const float* impulseTable;
  const float* consts;  // live constants (mlgpu_graph_set_live_constants): one float per const node, the same for all voices
  size_t t0;  // DSPVectors processed since the last clear (a Downsample2xFunction region pairs vectors 2k, 2k + 1)
  uint32_t flags;  // MLGPU_KFLAG_*
  EventsDev events;
  // the listed form of a graph kernel (mlgpu_graph_process_listed): lane i of the launch runs voice voiceList[i] of the graph's V
  // voices - tables, rings, input rows and control columns are read at the voice, out and peaks written at i; peaks[i] (or nullptr)
  // gets the largest |sample| bit pattern of the voice's outputs in the launch. Else unused.
  const uint32_t* voiceList;
  size_t listed;  // the list's length K
  uint32_t* peaks;
  // the listed form by a lane plan (mlgpu_graph_process_listed_groups): the launch is `listed` = N lanes laid out by the host, lane l's
  // entry the four words lanePlan[4 l .. 4 l + 3] of ChainArgs::lanePlan (voice or pad, list position, output row, rank | length << 8).
  // Tables, rings, input rows and control columns are read at the voice, plain outputs and peaks written at the list position, a
  // group-summed output at its row of a signal of J rows; voiceList is unused. Else unused.
  const uint32_t* lanePlan;
};

// row `row` of the state memory at the voice whose byte offset in a row is lane4: the row's address is wave-uniform (scalar
// arithmetic), the lane's place a 32-bit offset on it - the memory instruction's own addressing, no vector add (graph.hip: stateRef)
__device__ __forceinline__ uint32_t* state_row(const GraphArgs& a, size_t row, uint32_t lane4)
{
  return (uint32_t*)((char*)(a.state + row * a.V) + lane4);
}
