// graph_codegen.hpp — a voice graph's description, its compile plan, and the HIP source made of the two (graph_codegen.cpp).
//
// description -> plan -> source. The description (GraphDesc) is what the mlgpu_graph_add_* / _set_* calls write. The plan
// (GraphPlan) is everything a compile derives from it - ring placement, the resolved ring layout, the early reads, the
// oscillator pairs, the default kernel form - computed once by planGraph and not changed afterwards. The source is a pure
// function of the two and the kernel's form. Host C++17: no HIP runtime, no device; graph.hip owns handles, buffers and launches.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/mlgpu.h"

// chains.hip: the processors' tables
int mlgpu_proc_rings(int kind);            // delay rings per voice (0 for processors without delay memory)
bool mlgpu_proc_is_vector_rate(int kind);  // one float per DSPVector in (Interpolator1, LinearGlide): graphs only

// What the generated kernels' device headers fix, for the host's LDS budget and the generated text (this file does not include the
// device headers; chains.hip asserts each equals its device-side counterpart): the LDS strips in floats per WAVEFRONT, the clock
// shift of take_turns_by_clock, and the sizes of GraphArgs' signal lists
constexpr int kHostMixStripFloats = 64 * 20 + 3 * 16 + 16;
constexpr int kHostGroup16StripFloats = 4 * (4 * 80 + 4);
constexpr int kHostSegmentStripFloats = 4 * 64 * 4, kHostSegmentTailFloats = 16 * 4;
constexpr int kHostTurnClockShift = 13;
constexpr int kHostGraphMaxInputs = 32, kHostGraphMaxOutputs = 8;

namespace mlgraph
{
enum NodeType
{
  NODE_INPUT = 0,
  NODE_PARAM = 1,
  NODE_CONST = 2,
  NODE_PROC = 3,
  NODE_OP = 4,
  NODE_CONTROL = 5,  // streamed, one float per DSPVector per voice
  NODE_VOP = 6,      // index-dependent vector generator (columnIndex, rangeOpen, ...)
  NODE_ROUTE = 7,    // multiplex / demultiplex (MLDSPRouting.h); in[0] is the selector
  NODE_FEEDBACK = 8,  // value of another node one DSPVector ago (64 state words per voice)
  NODE_EVENT_ROW = 9  // a row of the bound EventsToSignals object, computed in this kernel (slot: the row - 0 pitch, 1 gate, 2 vox, 3 z, 4 x, 5 y, 6 mod)
};

// how often a node's value changes: per voice (params, consts and ops on them), per DSPVector (controls and
// ops on them), per sample. Decides where the generated code evaluates it.
enum Rate
{
  RATE_VOICE = 0,
  RATE_VECTOR = 1,
  RATE_AUDIO = 2
};

enum { ROLE_NONE = 0, ROLE_REGION_IN = 1, ROLE_REGION_OUT = 2 };

struct Node
{
  int type;
  int kind;  // proc kind or op
  std::vector<int> in;
  std::string name;
  Node(int type_ = 0, int kind_ = 0, const char* name_ = nullptr) : type(type_), kind(kind_), name(name_ ? name_ : "") {}
  float value{0.f};
  int slot{0};            // input index / param index / control index; demultiplex: output index
  int nOut{0};            // demultiplex: number of outputs
  size_t ringLen{0};      // delay nodes: floats per ring (power of two), 0 = not set
  int fbSource{-1};       // feedback nodes: the node whose value is stored for the next vector
  int rate{RATE_AUDIO};
  int cOff{0}, sOff{0}, nc{0}, ns{0};
  int region{-1};         // the rate region whose function this node belongs to (-1: the outer graph)
  std::vector<uint32_t> table;  // MLGPU_VOP_TABLE: the 64 floats of a constant DSPVector (bit patterns)
  int role{0};            // ROLE_REGION_IN: HalfBandFilter carrying an outer node into region `region`;
                          // ROLE_REGION_OUT: HalfBandFilter bringing region `slot`'s result back (an outer node)
};

// Upsample2xFunction / Downsample2xFunction (MLDSPFunctional.h:114-213) with fn written out as nodes
struct Region
{
  int kind{0};            // mlgpu_region
  int parent{-1};         // the region this one is nested in (-1: the outer graph)
  std::vector<int> ins;   // ROLE_REGION_IN nodes
  int result{-1};         // fn's return value (a node of the region)
  int out{-1};            // ROLE_REGION_OUT node
};

// What the building calls write, and nothing a compile derives
struct GraphDesc
{
  size_t V{0};
  std::vector<Node> nodes;
  std::vector<int> outputs;
  int inputGroup[kHostGraphMaxInputs] = {};  // > 1: the input has one row per that many adjacent voices (mlgpu_graph_set_input_group)
  bool outputMix[kHostGraphMaxOutputs] = {};  // the output is the mixdown of all voices (graph_set_output_mixdown)
  bool outputMixShard[kHostGraphMaxOutputs] = {};  // ... handed over as the rows of a SHARD (graph_set_output_mixdown(.., 2): mlgpu_mixdown_shard_rows(V) rows for mlgpu_mixdown_finish)
  int outputGroup[kHostGraphMaxOutputs] = {};  // > 0: the output is the in-order sum of groups of that many adjacent voices
  std::vector<Region> regions;
  int openRegion{-1};            // between graph_begin_region and graph_end_region
  int nInputs{0}, nParams{0}, nControls{0}, nConsts{0}, NC{0}, NS{0};
  bool hasImpulse{false};
  bool hasEventRows{false};
  unsigned eventRowMask{0};      // bit r: row r is a NODE_EVENT_ROW node (0 pitch, 1 gate, 2 vox, 3 z, 4 x, 5 y, 6 mod)
  bool strictSvf{false};         // the engine's mode when the graph was made (mlgpu_engine_set_strict_svf)
  bool liveConsts{false};        // const nodes read d_consts instead of being literals of the generated code
  int delayLayout{0};            // as mlgpu_graph_set_delay_layout took it (3: the best of 2 / 4 / 1 for the graph)
  int voicesPerLane{0};          // 0 = choose at compile (graphVoicesPerLane); 1 or 2 = forced
  bool autotune{false};
  bool voiceLists{false};        // a compile makes the listed form of the kernel too (mlgpu_graph_enable_voice_lists)
  bool voiceListGroups{false};   // ... and that form goes by the host's lane plan, its group-summed outputs one row per listed instrument (mlgpu_graph_enable_voice_list_groups)
  bool mpeEvents{false};         // the plain kernel's event rows in the MPE-capable form: mlev::CtlVoiceMpe / CtlRowsMpe (mlgpu_graph_enable_mpe_events)
  bool voiceListEvents{false};   // ... and a graph with event rows has it too: CtlVoice of the gathered voice (mlgpu_graph_enable_voice_list_events)
  bool voiceListMpeEvents{false};  // ... in the form for either protocol: CtlVoiceMpe / CtlRowsMpe of the gathered voice (mlgpu_graph_enable_voice_list_mpe_events; implies the two above)
  bool voiceListRings{false};    // ... and a graph with delay rings has it in the sector layouts 1 and 4 too, layout 3 resolving to one of them (mlgpu_graph_enable_voice_list_rings)
};

// Where the delay rings live (mlgpu_graph_set_delay_layout 0, 1, 2 and 4; its layout 3 is resolved to one of them by planGraph)
enum class RingLayout  // (the values are MLGPU_RING_WINDOWS of the device headers)
{
  ROWS = 0,    // layout 0: ring rows of the bank's voices
  WINDOWS,     // layout 1: rings as [block][chunk][lane][8] behind LDS windows
  TRANSPOSED,  // layout 2: [block][chunk][lane][16], every global access a 64-byte piece made by four lanes, on a wave-uniform clock
  SECTORS      // layout 4: layout 1's memory, no LDS, trips of 8 samples with every ring's loads in the trip's prologue
};
// the layout's number in the API (and MLGPU_RING_WINDOWS of the device headers: 0, 1, 2 and, for layout 4, 3), and back
inline int apiLayout(RingLayout r) { return r == RingLayout::SECTORS ? 4 : (int)r; }
inline RingLayout ringLayoutOfApi(int layout) { return layout == 4 ? RingLayout::SECTORS : layout == 3 ? RingLayout::WINDOWS : (RingLayout)layout; }  // (3: laid out as 1 where neither 2 nor 4 applies)

// A graph kernel's form besides the graph: voices per lane, quads per trip of the sample loop, and the wavefronts per SIMD its
// register budget must allow (0: the compiler's choice; generateBudgeted). `listed`: the kernel of mlgpu_graph_process_listed - a
// lane's place in the launch is its position in the voice list, its voice GraphArgs::voiceList's entry there (one voice per lane).
// `planned` (with `listed`): the kernel of mlgpu_graph_process_listed_groups - a lane's voice, list position, output row and place in
// its segment are its entry of GraphArgs::lanePlan (voice_list.hpp: mlvl::planGroups), a pad lane leaves before anything else
struct KernelForm
{
  int voicesPerLane{1}, quadsPerTrip{1}, minWaves{0};
  bool listed{false};
  bool planned{false};
};

// Test hooks, not settings: the differential tests build a kernel's second form with these (environment variables, readTestHooks)
struct TestHooks
{
  int minWaves{-1};        // MLGPU_GRAPH_MIN_WAVES=N: generateBudgeted's bound, N wavefronts per SIMD (0: none); -1: not set
  bool rowAddr64{false};   // MLGPU_GRAPH_ROW_ADDR32=0: 64-bit state and ring row addresses
  bool earlyReads{true};   // MLGPU_GRAPH_EARLY_READS=0: the plain ring loads
  int oscTripQ{2};         // MLGPU_GRAPH_OSC_TRIP: 0: polyBLEP per sample, else 1, 2 or 4 quads per trip
  bool ringLaneClock{true};  // MLGPU_GRAPH_RING_LANE_CLOCK=0: the listed kernel of ring layout 4 keeps the plain kernel's aligned test (equal write indices)
};

struct NodePlan
{
  size_t memOff{0};       // delay nodes: first ring at d_mem + memOff * memVoices
  int ringSlot{0};        // delay nodes: index of this node's first ring among all rings of the graph (LDS windows)
  int earlySlot{-1};      // ring layout 0 with early reads: this node's first 256-byte landing slot in the wavefront's LDS,
  bool earlyTop{false};   //   its read issued at the top of the sample with the batch of such reads (RingCore::readEarly),
  int earlyPending{0};    //   and the loads the kernel issues there right after this node's (RingCore::earlyWait)
  bool earlyHoisted{false};  // a node such a read's delay time is made of: made at the top of the sample, before the reads
  // A SawGen / PulseGen of the outer graph whose frequency (and width) are per voice, not per sample: its samples are made a trip of
  // oscTripQ quads at a time (Proc<>::trip_u: the polyBLEP corrections once per zone per trip) into registers the sample loop reads.
  bool oscTrip{false};
  // SawGen trip node: the PulseGen trip node on the same frequency node (-1: none). The pair is run by trip_locked when, at the
  // start of a launch, every lane of the wavefront has the two phase counters equal (mldsp_procs.hpp).
  int lockedPartner{-1};
  // The same pairing for a STREAMED frequency (the instrument bank's voice: pitch signal -> exp2Approx -> freq): a SawGen of the outer
  // graph and the PulseGen on the same audio-rate frequency node, its width per voice. The pair runs as step_locked_stream
  // (mldsp_procs.hpp) while the two phase counters are equal in every lane of the wavefront (slocked<saw>, asked once per launch).
  int streamLockPulse{-1};  // the saw of such a pair: its pulse
  int streamLockSaw{-1};    // the saw or the pulse of such a pair: its saw
};

// Everything a compile derives from a description, made by planGraph and read-only afterwards
struct GraphPlan
{
  RingLayout rings{RingLayout::ROWS};  // the layout the kernel uses
  int totalRings{0};
  size_t memFloatsPerVoice{0};
  size_t memVoices{0};           // voices the ring memory is laid out for (whole 256-voice blocks but in layout 0)
  bool rowAddr32{false};         // layout 0: ring rows behind 32-bit offsets from a wave-uniform base where a ring allows it (VoiceMem::ringPtr)
  bool rowAddr64{false};         // TestHooks::rowAddr64
  bool earlyRows{false};         // layout 0: the ring reads of the outer graph's delay nodes issued ahead by LDS-DMA (RingCore::readEarly)
  int earlySlots{0};             // their landing slots per wavefront
  int oscTripQ{2};               // quads per trip of the oscillators' sparse polyBLEP (0: per sample; mldsp_procs.hpp: trip_u)
  bool oscTrips{false};          // some node is an oscillator trip
  int minWavesHook{-1};          // TestHooks::minWaves
  bool ringByLane{false};        // voice lists with rings in layout 4: the listed kernel decides per lane what the plain one decides per wavefront (MLGPU_RING_BY_LANE)
  bool ringsByLaneOnly{false};   // ... and the graph has a PitchbendableDelay: after a listed launch the plain kernel would read its second ring, which the listed one leaves unwritten
  bool ringLaneClock{false};     // the listed kernel of ring layout 4 asks each lane for a sector boundary, not the wavefront for one write index (MLGPU_RING_LANE_CLOCK; TestHooks::ringLaneClock)
  KernelForm form;               // the default form (autotune may run another: mlgpu_graph::activeForm)
  std::vector<NodePlan> nodes;   // indexed like GraphDesc::nodes
};

// Every check and decision of a compile that needs no device. MLGPU_OK, or a status with `error` set (plan is then unspecified).
int planGraph(const GraphDesc& d, const TestHooks& hooks, GraphPlan& plan, std::string& error);

// The source of a graph's kernel: a pure function of the description, the plan and the form
std::string generateGraphSource(const GraphDesc& d, const GraphPlan& plan, const KernelForm& form);
}  // namespace mlgraph
