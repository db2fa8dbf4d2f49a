// mlgpu_internal.hpp — shared between the translation units of libmlgpu.so (not installed).
#pragma once
#include <atomic>
#include <memory>
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mlgpu.h"
#include "launch_parts.hpp"
#include "mixdown_tree.hpp"
#include "mlgpu_device_args.hpp"
#include "param_updates.hpp"
#include "staging_turns.hpp"
#include "voice_records.hpp"

// Owning device memory, pinned host memory and HIP events: every handle frees what it holds by deleting its members
struct DeviceFree
{
  static hipError_t allocate(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  void operator()(void* p) const { hipFree(p); }
};
struct HostFree
{
  static hipError_t allocate(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  void operator()(void* p) const { hipHostFree(p); }
};
struct EventDestroy
{
  void operator()(hipEvent_t ev) const { hipEventDestroy(ev); }
};
template <class T> using DeviceBuffer = std::unique_ptr<T[], DeviceFree>;
template <class T> using PinnedBuffer = std::unique_ptr<T[], HostFree>;
using OwnedEvent = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, EventDestroy>;

// `out` replaced by `count` fresh elements (empty if that fails): the old buffer is freed first
template <class T, class Free>
hipError_t allocate(std::unique_ptr<T[], Free>& out, size_t count)
{
  out.reset();
  T* p = nullptr;
  const hipError_t err = Free::allocate((void**)&p, sizeof(T) * count);
  out.reset(err == hipSuccess ? p : nullptr);
  return err;
}
inline hipError_t allocate(OwnedEvent& out, unsigned flags = hipEventDefault)
{
  hipEvent_t ev = nullptr;
  const hipError_t err = hipEventCreateWithFlags(&ev, flags);
  out.reset(err == hipSuccess ? ev : nullptr);
  return err;
}

// a pinned + device pair of upload buffers replaced by one of `fresh` elements - the caller's growth policy - when `need` do not fit
// (the old contents go; capacity 0 if that fails)
template <class T>
bool growPair(PinnedBuffer<T>& host, DeviceBuffer<T>& dev, size_t& capacity, size_t need, size_t fresh)
{
  if (need <= capacity) return true;
  capacity = 0;
  if (allocate(dev, fresh) != hipSuccess || allocate(host, fresh) != hipSuccess) return false;
  capacity = fresh;
  return true;
}

// The staging sets of host uploads take turns by mlstage's rule (staging_turns.hpp; DESIGN.md §3.7, "Staging turns") on HIP events
struct HipStagingApi
{
  using Event = hipEvent_t;
  using Stream = hipStream_t;
  static bool create(Event& ev) { return hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess; }
  static void destroy(Event ev) { hipEventDestroy(ev); }
  static bool wait(Event ev) { return hipEventSynchronize(ev) == hipSuccess; }
  static bool record(Event ev, Stream stream) { return hipEventRecord(ev, stream) == hipSuccess; }
  static void drain(Stream stream) { hipStreamSynchronize(stream); }
};
using StagingTurn = mlstage::Turn<HipStagingApi>;
template <class Set> using StagingTurns = mlstage::Turns<HipStagingApi, Set>;
inline hipError_t createTurn(StagingTurn& turn)  // (for the create functions, which report a hipError_t)
{
  if (turn.create()) return hipSuccess;
  const hipError_t err = hipGetLastError();
  return err != hipSuccess ? err : hipErrorUnknown;
}

// The two streams of launches that go out in parts fork and join by mlparts' rule (launch_parts.hpp; DESIGN.md §3.1, "Launch parts")
struct HipStreamsApi
{
  using Stream = hipStream_t;
  using Event = hipEvent_t;
  using Error = hipError_t;
  static constexpr Error kSuccess = hipSuccess;
  static Error priority(Stream stream, int& priority) { return hipStreamGetPriority(stream, &priority); }
  static Error createStream(Stream& stream, int priority) { return hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, priority); }
  static void destroyStream(Stream stream) { hipStreamDestroy(stream); }
  static Error createEvent(Event& ev) { return hipEventCreateWithFlags(&ev, hipEventDisableTiming); }
  static void destroyEvent(Event ev) { hipEventDestroy(ev); }
  static Error record(Event ev, Stream stream) { return hipEventRecord(ev, stream); }
  static Error wait(Stream stream, Event ev) { return hipStreamWaitEvent(stream, ev, 0); }
  static Error synchronize(Stream stream) { return hipStreamSynchronize(stream); }
};

struct mlgpu_engine
{
  explicit mlgpu_engine(hipStream_t main) : streams(main) {}  // (createEngine: the engine's own stream or the caller's)
  int device{0};
  bool ownsStream{false};
  int cuCount{256};
  std::string lastError;
  DeviceBuffer<float> d_impulseTable;  // 17 floats (ImpulseGen windowed sinc), built on the host
  OwnedEvent ev0, ev1;
  std::vector<OwnedEvent> lapEvents;  // mlgpu_timer_laps_*: created once, reused
  size_t lapCount{0}, lapMax{0};
  bool jitEnabled{true};  // fuse unknown chains / graphs with hiprtc (mlgpu_engine_set_jit)
  bool strictSvf{false};  // banks and graphs made from now on get kernels compiled with MLGPU_SVF_STRICT 1 (mlgpu_engine_set_strict_svf)
  DeviceBuffer<float> d_mixScratch;  // mixdown partial sums, grown on demand
  size_t mixScratchFloats{0};
  // Region `r` of `n` regions for the mixdown tree of V voices over T DSPVectors (mixdown_tree.hpp), or null where the scratch does
  // not hold the n: what a call hands its first stage before the launch and walks after it. The refusal's words are the caller's.
  // (A tree of no voices needs no floats and fits a scratch never reserved, which is null too: callers with V == 0 do not ask.)
  float* mixdownRegion(size_t V, size_t T, size_t r = 0, size_t n = 1) const
  {
    const size_t floats = mlmix::regionFloats(V, T);
    return n * floats > mixScratchFloats ? nullptr : d_mixScratch.get() + r * floats;
  }
  DeviceBuffer<unsigned long long> d_validate;  // {count, first index} of mlgpu_validate, allocated with the engine
  uint32_t kflags{0};  // MLGPU_KFLAG_* handed to every arithmetic kernel (mlgpu_engine_set_flush_denormals)
  bool recording{false};  // between mlgpu_engine_begin_recording and _end_recording: launches are captured, not run
  int liveSequences{0};   // recorded sequences not yet destroyed: they hold device pointers, so buffers handed out must not move
  // what recorded sequences might still replay launches that read (objects destroyed, buffers replaced): freed when the last
  // sequence goes (mlgpu_sequence_destroy) or with the engine
  std::vector<std::shared_ptr<void>> deferredFrees;
  void runDeferredFrees() { std::vector<std::shared_ptr<void>>().swap(deferredFrees); }
  // An object or buffer that recorded launches may read, given up: freed now, or with the last sequence while one lives
  void retire(std::shared_ptr<void> owner)
  {
    if (liveSequences > 0) deferredFrees.push_back(std::move(owner));
  }
  // The destroy function of every object this engine owns ends here. Refused while recording: waiting for the stream would
  // invalidate the capture. Otherwise the stream is drained, `atOnce` frees what no replay reads, and the object is retired.
  template <class T, class AtOnce>
  int release(T* obj, const char* what, AtOnce atOnce)
  {
    if (recording)
    {
      lastError = std::string(what) + " waits for the device: not while recording a sequence";
      return MLGPU_ERR_INVALID;
    }
    hipSetDevice(device);
    hipStreamSynchronize(stream());
    atOnce(obj);
    retire(std::unique_ptr<T>(obj));
    return MLGPU_OK;
  }
  template <class T>
  int release(T* obj, const char* what)
  {
    return release(obj, what, [](T*) {});
  }

  // ---- the engine's stream, and the side stream of launches that go out in parts (launch_parts.hpp) ----
  // Everything the engine enqueues, waits for or hands out goes through stream(), which first lets the main stream wait for
  // what is pending on the side stream: nobody can forget the join. The rule - fork, lazy join, the order of the parts - and the
  // two raw streams live in mlparts::Streams, which has no accessor for either: a launch in parts (capi.hip: mlgpu_bank_process)
  // is handed each part's stream by streams.launch() and nothing else sees one.
  hipStream_t stream() { return streams.stream(); }
  // May a launch go out in parts at all: the engine's stream is its own and nobody else's (mlgpu_engine_launch_parts_possible) ...
  bool ownsPrivateStream() const { return ownsStream && !streamHandedOut; }
  // ... and now: nothing is being recorded (mlgpu_bank_process)
  bool mayLaunchInPartsNow() const { return ownsPrivateStream() && !recording; }

  int launchParts{mlparts::kAuto};  // mlgpu_engine_set_launch_parts
  bool streamHandedOut{false};      // mlgpu_engine_stream has given the main stream away: every launch in one part from then on
  mlparts::Streams<HipStreamsApi> streams;  // (the last member: its side stream and events go first, the main stream is not its to destroy)
};

struct mlgpu_fence  // mlgpu_engine_signal / mlgpu_engine_wait: a point in one engine's stream that another engine's stream can wait for
{
  int device{0};
  OwnedEvent ev;
  std::atomic<bool> signalled{false};  // set by the signalling engine's host thread, read by the waiting engine's
};

struct mlgpu_sequence  // a recorded launch sequence: a hipGraph instantiated once, replayed with one launch
{
  mlgpu_engine* e{nullptr};
  hipGraph_t graph{nullptr};
  hipGraphExec_t exec{nullptr};
  size_t nodes{0};
};

inline SignalView makeView(const float* p, int layout, size_t V, size_t T)
{
  SignalView s;
  s.base = (float4*)p;
  switch (layout)
  {
    case MLGPU_LAYOUT_QUAD: s.strideT = 16 * V; s.strideQ = V; s.strideV = 1; break;
    case MLGPU_LAYOUT_ROWS: s.strideT = 16 * V; s.strideQ = 1; s.strideV = 16; break;
    case MLGPU_LAYOUT_BROADCAST: s.strideT = 16; s.strideQ = 1; s.strideV = 0; break;
    default: /* VOICE_MAJOR */ s.strideT = 16; s.strideQ = 1; s.strideV = 16 * T; break;
  }
  return s;
}

// the forms of a chain's kernel (mldsp_kernels.hpp: one loop, one sink per form)
enum ChainForm
{
  kFormPlain,         // chain_kernel, cascade_kernel / cascade_lanes_kernel: every entry has it
  kFormMix,           // chain_mix_kernel (the voices' sum instead of their signals): the fused voice chains
  kFormGroups,        // chain_group_kernel (voices in groups of 1, 2, 4, 8, 16): the chain kernels, not the cascades
  kFormListed,        // chain_listed_kernel (the voices of a list): where kFormGroups is
  kFormListedMix,     // chain_listed_mix_kernel: where kFormMix is
  kFormListedGroups,  // chain_listed_group_kernel (the listed voices summed by instrument): where kFormGroups is
  kFormMixChannels,        // chain_mix_channels_kernel<.., 2> (the voices' sum once per channel, two channels): where kFormMix is
  kFormListedMixChannels,  // chain_listed_mix_channels_kernel<.., 2>: where kFormMix is
  kFormGroupsChannels,        // chain_group_channels_kernel<.., 2, 4, 8 or 16, 2> (the sums by instrument once per channel): where kFormMix is
  kFormListedGroupsChannels,  // chain_listed_group_channels_kernel<.., 2>: where kFormMix is
  kChainForms
};
constexpr int kMixChannels = 2;  // the channel count the channel forms are instantiated for (the calls refuse any other but 1)
// outGroup: the group size of kFormGroups, which picks the instantiation; no other form reads it
typedef hipError_t (*ChainLauncher)(const ChainArgs& a, hipStream_t stream, int outGroup);

struct ChainEntry
{
  std::vector<int> kinds;
  ChainLauncher launch[kChainForms][2]{};  // [form][input is streamed]; null: the chain has no such form
  const char* kernelName;  // prefix of the name a profiler shows for the device kernel
  const char* (*kernelNameFor)(size_t V, uint32_t flags){nullptr};  // where the kernel depends on the bank's size (SVF cascades)
  const char* alias;       // e.g. "chain_kernel<SawGen,Bandpass,Gain>"
  bool plainTakesWindow{false};  // the plain form runs a window of a bank's voices (ChainArgs::tableStride): chain_kernel, not the cascades
  int nc, ns;
};

// chains.hip
const ChainEntry* mlgpu_find_chain(const int32_t* kinds, int n);
int mlgpu_proc_nc(int kind);  // -1 if unknown
int mlgpu_proc_ns(int kind);
constexpr int MLGPU_MAX_PROC_STATE = 80;  // LinearGlide: 3 + 64
constexpr int MLGPU_MAX_PROC_COEFFS = 8;
void mlgpu_proc_clear_state(int kind, uint32_t* words /*[ns <= MLGPU_MAX_PROC_STATE]*/, bool cleared);
void mlgpu_proc_default_coeffs(int kind, float* c /*[nc <= MLGPU_MAX_PROC_COEFFS]*/);
bool mlgpu_proc_is_graph_only(int kind);   // vector-rate ramps and delay lines: no chain kernel
int mlgpu_proc_rings(int kind);            // delay rings per voice (0 for processors without delay memory)
uint64_t mlgpu_proc_clear_mask(int kind);  // state words T::clear() resets
bool mlgpu_proc_is_vector_rate(int kind);  // one float per DSPVector in (Interpolator1, LinearGlide): graphs only

// ops.hip
hipError_t mlgpu_launch_op(int op, const void* a, const void* b, const void* c, void* out, size_t n,
                           hipStream_t stream, int cuCount, bool* known, uint32_t flags);
hipError_t mlgpu_launch_op_rows1(int op, const void* a, const void* b64, void* out, size_t nRows,
                                 hipStream_t stream, int cuCount, bool* known, uint32_t flags);
hipError_t mlgpu_launch_row_reduce(int rowop, const float* rows, float* out, size_t nRows,
                                   hipStream_t stream, bool* known, uint32_t flags);
hipError_t mlgpu_launch_layout_convert(const float* src, int srcLayout, float* dst, int dstLayout, size_t V,
                                       size_t T, hipStream_t stream);
hipError_t mlgpu_launch_fill32(uint32_t* dst, uint32_t value, size_t n, hipStream_t stream);
hipError_t mlgpu_launch_validate(const float* x, size_t n, unsigned long long* d_result, hipStream_t stream, int cuCount);
hipError_t mlgpu_launch_rows_map(int rule, long p0, long p1, int sampleRotate, const float* src, size_t srcRows, float* dst,
                                 size_t dstRows, size_t dstOffset, size_t dstStep, size_t count, size_t groups, hipStream_t stream);
hipError_t mlgpu_launch_rows_add(const float* rows, size_t rowsPerGroup, float* out, size_t groups, hipStream_t stream, uint32_t flags);
hipError_t mlgpu_launch_rows_normalize(const float* rows, float* out, size_t nRows, hipStream_t stream, uint32_t flags);
hipError_t mlgpu_launch_rows_index(float* out, size_t rowsPerGroup, size_t groups, hipStream_t stream);
hipError_t mlgpu_launch_mixdown(const float* sig, int layout, size_t V, size_t T, const float* gains, float* partial, float* out,
                                hipStream_t stream, uint32_t flags);
int mlgpu_mixdown_reserve_floats(mlgpu_engine* e, size_t floats);  // capi.hip: the mixdown scratch grown to at least that
// (reductions: mlmix::kToTheEnd, or the exact 64-to-1 passes of a shard's hand-over)
hipError_t mlgpu_launch_mixdown_rows(size_t groups, size_t T, float* partial, float* out, int reductions, hipStream_t stream, uint32_t flags);
hipError_t mlgpu_launch_mixdown_stage1(const float* sig, int layout, size_t V, size_t T, const float* gains, float* partial, hipStream_t stream, uint32_t flags);
hipError_t mlgpu_launch_mixdown_groups(const float* sig, int layout, size_t groups, size_t P, size_t T, float* out, int outLayout, hipStream_t stream, uint32_t flags);
hipError_t mlgpu_launch_route(bool demux, bool linear, const float* sel, size_t selElems, const float* const* ins, float* const* outs, int n,
                              size_t nElems, hipStream_t stream, uint32_t flags);

// jit.hip, graph.hip — run-time fused kernels (hiprtc)
bool mlgpu_jit_chain(mlgpu_engine* e, const int32_t* kinds, int n, void** fnSignal, void** fnConst, std::string& log);  // honours e->strictSvf
hipError_t mlgpu_jit_chain_launch(void* fn, const ChainArgs& a, hipStream_t stream);
bool mlgpu_jit_chain_mix(mlgpu_engine* e, const int32_t* kinds, int n, void** fnSignal, void** fnConst, std::string& log);
std::string mlgpu_jit_chain_source(const int32_t* kinds, int n, bool strictSvf, bool mix);
// the code object of a generated source: from the memory cache, the disk cache or hiprtc (mlgpu_jit_stats counts which)
bool mlgpu_jit_code(const std::string& source, std::vector<char>& code, std::string& log);
bool mlgpu_jit_compile_only(const std::string& source, std::string& log);  // hiprtc alone, no caches, no device (mlgpu_jit_selftest)
// a kernel of a generated source, its module loaded on `device` once per process (*loaded: the module is there, whatever the lookup found)
hipFunction_t mlgpu_jit_function(int device, const std::string& source, const char* name, std::string& log, bool* loaded = nullptr);
hipError_t mlgpu_jit_launch(hipFunction_t fn, void* args, size_t argBytes, size_t V, hipStream_t stream);  // blocks of 256 lanes over V
bool mlgpu_jit_code_number(const std::vector<char>& code, const char* key, long& value);  // a number of the kernel's metadata note

// updates.hip — sparse per-voice table updates (mlgpu_graph_apply_updates, mlgpu_bank_apply_updates): what a graph or a bank keeps
// for them. `desc` describes the owner's tables to the host planner and is made by the owner (once: the tables' shape is fixed
// when a graph is compiled / a bank created); the two staging sets take turns.
struct mlgpu_updater
{
  mlupd::UpdatePlanner planner;
  mlupd::TableDesc desc;
  bool described{false};
  struct Set
  {
    PinnedBuffer<mlupd::DevRec> h_recs;
    DeviceBuffer<mlupd::DevRec> d_recs;
    size_t capacity{0};
  };
  StagingTurns<Set> stage;
  size_t reserved{0};  // reserve_updates: device records per call (0: no reserve, the buffers grow inside apply)
};
int mlgpu_updater_reserve(mlgpu_engine* e, mlgpu_updater& u, size_t maxDeviceRecords, std::string& err);
size_t mlgpu_updater_device_records(mlgpu_updater& u, const mlgpu_update* recs, size_t n);
// tables[mlupd::kTables]: the device rows of params, coefficients, state and input constants (null where the owner has none);
// ringMem[ringMemWords]: a graph's delay-ring memory (null: none, and desc says so)
int mlgpu_updater_apply(mlgpu_engine* e, mlgpu_updater& u, uint32_t* const* tables, uint32_t* ringMem, size_t ringMemWords, const mlgpu_update* recs, size_t n,
                        std::string& err);
size_t mlgpu_updater_staging(const mlgpu_updater& u, const void** four);  // (test hook: buffer addresses and capacity)

// voice_records.hip — voice records (mlgpu_graph_export_voices / _import_voices and the bank's): what a graph or a bank keeps for
// them. `plan` holds the record layout, made by the owner from its updater's table description (once); the two staging sets carry a
// call's segments and entries and take turns.
struct mlgpu_recorder
{
  mlrec::RecordPlan plan;
  bool described{false};  // (tried: plan.described() says whether the object has a layout)
  struct Set
  {
    PinnedBuffer<uint32_t> h_words;
    DeviceBuffer<uint32_t> d_words;
    size_t capacity{0};
  };
  StagingTurns<Set> stage;
  size_t reserved{0};  // reserve_voice_records: voices per call (0: no reserve, the buffers grow inside the call)
};
int mlgpu_recorder_reserve(mlgpu_engine* e, mlgpu_recorder& r, size_t maxVoices, std::string& err);
// tables / ringMem as mlgpu_updater_apply takes them; d_records[n][plan.words()]; import: records -> the object, else the object -> records
int mlgpu_recorder_move(mlgpu_engine* e, mlgpu_recorder& r, uint32_t* const* tables, uint32_t* ringMem, size_t ringMemWords, const uint32_t* h_voices, size_t n,
                        uint32_t* d_records, bool import, std::string& err);
size_t mlgpu_recorder_staging(const mlgpu_recorder& r, const void** four);  // (test hook: buffer addresses and capacity in words)

// capi.hip — the voice list of a bank or a graph (mlgpu_bank_set_voice_list, mlgpu_graph_set_voice_list). The list in force lives in ONE
// device buffer, written by copies on the engine's stream: a listed launch - a recorded one too, which has the address - reads
// whatever the copies before it in stream order left. The host's copy goes through two pinned sets that take turns (DESIGN.md
// §3.7, "Staging turns").
struct mlgpu_voice_list
{
  DeviceBuffer<uint32_t> d_list;
  size_t capacity{0};  // entries of d_list and of each pinned set
  size_t reserved{0};  // reserve (0: none, the buffers grow inside set)
  size_t size{0};      // of the list set last: the K of the next listed launch (host order is stream order)
  // the lane plan of the listed group sum (mlgpu_bank_reserve_voice_list_groups; voice_list.hpp: mlvl::planGroups). outGroup == 0:
  // none, and nothing below is touched. Else every `set` makes the plan in its staging set and uploads it behind the list.
  int outGroup{0};
  DeviceBuffer<uint32_t> d_plan;     // [mlvl::kLaneWords][planCapacity]
  size_t planCapacity{0};            // lanes of d_plan and of each pinned set: mlvl::maxPlanLanes(reserved, outGroup)
  size_t planLanes{0}, planGroups{0};  // N and J of the list in force
  std::vector<uint32_t> groups;      // M[0 .. J) of the list in force (the host's copy: mlgpu_bank_listed_groups); sized at the reserve
  struct Set
  {
    PinnedBuffer<uint32_t> h_list;
    PinnedBuffer<uint32_t> h_plan;
    std::vector<uint32_t> h_groups;
  };
  StagingTurns<Set> stage;
  // `who`: the calling function's name for the engine's last error ("bank_set_voice_list"); nVoices: the owner's voice count
  int grow(mlgpu_engine* e, size_t need, const char* who);  // buffers of `need` entries, the list in force carried over. Allocates and waits: setup only.
  // newOutGroup: -1 keeps the plan's group size (and resizes its buffers with the list's), 0 turns the plan off, 2 / 4 / 8 / 16 set it
  int reserve(mlgpu_engine* e, size_t maxListed, const char* who, int newOutGroup = -1);
  int set(mlgpu_engine* e, size_t nVoices, const uint32_t* h_voices, size_t n, const char* who);
  // the listed instruments M[0 .. J) of the list in force into h_groups[capacity]: MLGPU_OK, or the refusal's status with `err` = who + ...
  int copyGroups(uint32_t* h_groups, size_t capacity, const char* who, std::string& err) const;
};

// coeffs.cpp
void mlgpu_build_impulse_table(float* out17);

// events.hip, for graph.hip: the host half of an EventsToSignals block (routing, record upload) for a graph kernel that computes
// the pitch and gate rows itself (mlgpu_graph_bind_events)
struct mlgpu_events;
extern "C" int mlgpu_events_abandoned_by_graph(mlgpu_events* ev, void* staging);
extern "C" int mlgpu_events_prepare_for_graph(mlgpu_events* ev, size_t nVectors, int startOffset, unsigned rowMask, int mpeForm, EventsDev* dev, void** staging);
extern "C" int mlgpu_events_launched_by_graph(mlgpu_events* ev, void* staging);
extern "C" int mlgpu_events_is_midi(mlgpu_events* ev);
extern "C" mlgpu_engine* mlgpu_events_engine(mlgpu_events* ev);

