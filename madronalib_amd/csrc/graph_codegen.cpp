// graph_codegen.cpp — a voice graph's compile plan (planGraph) and the HIP source of its fused kernel (generateGraphSource).
//
// Execution model: the graph is translated to HIP source that instantiates the hand-written device building blocks
// (mldsp_procs.hpp / mldsp_ops.hpp) in topological order inside the voice-bank loop (one lane per voice, state in registers,
// one 16-byte access per lane per quad). Every edge of the graph is a register; only graph inputs and outputs touch HBM.
// Nothing here needs a device or the HIP runtime: graph.hip hands the source to the run-time compiler (jit.hip).
#include "graph_codegen.hpp"

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <sstream>

using namespace mlgraph;

namespace
{
std::string floatLiteral(float f)
{
  uint32_t u;
  memcpy(&u, &f, 4);
  char buf[48];
  snprintf(buf, sizeof(buf), "u2f(0x%08xu)", u);  // exact bits, no decimal round trip
  return buf;
}

// the C++ expression of node i for lane-group l (its inputs are the locals n<j>_<l>)
// Inside a rate region the values of the region's nodes carry the phase suffix `ph` ("a" / "b" for the two samples an
// Upsample2x region makes per outer sample) and `idx` is the sample index inside fn's own DSPVector.
// number of Upsample2x regions on the way from the outer graph down to region r (each adds one phase letter to a value's name)
int upDepth(const GraphDesc& g, int r)
{
  int d = 0;
  for (; r >= 0; r = g.regions[(size_t)r].parent) d += (g.regions[(size_t)r].kind == MLGPU_REGION_UPSAMPLE_2X);
  return d;
}

// clamp(x, lo, hi) whose bounds are literal constants of the kernel (not NaN, not zero, lo <= hi) and whose x is produced by
// an arithmetic instruction - a node that can never hand a signaling NaN on: then two hardware instructions give what the
// six of the general form do (clamp_const_bounds, mldsp_math.hpp). Inputs, parameters, feedback vectors, delay lines,
// selects and the bit-twiddling approximations carry raw bit patterns and keep the general form.
bool clampHasConstBounds(const GraphDesc& g, const Node& n)
{
  if (n.in.size() != 3 || g.liveConsts) return false;
  const Node &x = g.nodes[(size_t)n.in[0]], &lo = g.nodes[(size_t)n.in[1]], &hi = g.nodes[(size_t)n.in[2]];
  if (lo.type != NODE_CONST || hi.type != NODE_CONST) return false;
  if (!(lo.value <= hi.value) || lo.value == 0.f || hi.value == 0.f) return false;  // (a NaN bound fails the comparison)
  if (x.type == NODE_OP)
    switch (x.kind)
    {
      case MLGPU_OP_ADD: case MLGPU_OP_SUBTRACT: case MLGPU_OP_MULTIPLY: case MLGPU_OP_DIVIDE: case MLGPU_OP_LERP: case MLGPU_OP_INVERSE_LERP: return true;
      default: return false;
    }
  if (x.type == NODE_PROC)
    switch (x.kind)
    {
      case MLGPU_PROC_SINE_GEN: case MLGPU_PROC_SAW_GEN: case MLGPU_PROC_PULSE_GEN: case MLGPU_PROC_NOISE_GEN:
      case MLGPU_PROC_LOPASS: case MLGPU_PROC_HIPASS: case MLGPU_PROC_BANDPASS: case MLGPU_PROC_LO_SHELF: case MLGPU_PROC_HI_SHELF: case MLGPU_PROC_BELL:
      case MLGPU_PROC_ONE_POLE: case MLGPU_PROC_DC_BLOCKER: case MLGPU_PROC_INTEGRATOR: case MLGPU_PROC_DIFFERENTIATOR: case MLGPU_PROC_GAIN:
        return true;  // every output sample is the result of an add / sub / mul / fma
      default: return false;
    }
  return false;
}

// The oscillator pairs on a streamed frequency (NodePlan::streamLockPulse / streamLockSaw): the first saw on a frequency node takes
// the first pulse on it.
void planStreamLocks(const GraphDesc& g, GraphPlan& p)
{
  auto streamedOsc = [&](const Node& m, int kind) {
    return m.type == NODE_PROC && m.kind == kind && m.region < 0 && m.rate == RATE_AUDIO && !m.in.empty() && g.nodes[m.in[0]].rate != RATE_VOICE;
  };
  for (size_t i = 0; i < g.nodes.size(); ++i)
  {
    const Node& n = g.nodes[i];
    if (!streamedOsc(n, MLGPU_PROC_SAW_GEN)) continue;
    bool first = true;
    for (size_t k = 0; k < i; ++k) first = first && !(streamedOsc(g.nodes[k], MLGPU_PROC_SAW_GEN) && g.nodes[k].in[0] == n.in[0]);
    for (size_t j = 0; first && j < g.nodes.size(); ++j)
    {
      const Node& m = g.nodes[j];
      if (streamedOsc(m, MLGPU_PROC_PULSE_GEN) && m.in[0] == n.in[0] && (m.in.size() == 1 || g.nodes[m.in[1]].rate == RATE_VOICE))
      {
        p.nodes[i].streamLockPulse = (int)j;
        p.nodes[i].streamLockSaw = p.nodes[j].streamLockSaw = (int)i;
        break;
      }
    }
  }
}

// The oscillator trips (NodePlan::oscTrip) and their pairs on a per-voice frequency (NodePlan::lockedPartner), likewise first to first
void planOscTrips(const GraphDesc& g, GraphPlan& p)
{
  for (size_t i = 0; i < g.nodes.size(); ++i)
  {
    const Node& n = g.nodes[i];
    if (p.oscTripQ <= 0 || n.type != NODE_PROC || n.region >= 0 || n.rate != RATE_AUDIO) continue;
    if (n.kind != MLGPU_PROC_SAW_GEN && n.kind != MLGPU_PROC_PULSE_GEN) continue;
    if (n.in.empty() || g.nodes[n.in[0]].rate != RATE_VOICE) continue;
    p.nodes[i].oscTrip = n.kind == MLGPU_PROC_SAW_GEN || n.in.size() == 1 || g.nodes[n.in[1]].rate == RATE_VOICE;
    p.oscTrips = p.oscTrips || p.nodes[i].oscTrip;
  }
  auto trip = [&](size_t j, int kind) { return p.nodes[j].oscTrip && g.nodes[j].kind == kind; };
  for (size_t i = 0; i < g.nodes.size(); ++i)
  {
    if (!trip(i, MLGPU_PROC_SAW_GEN)) continue;
    bool first = true;
    for (size_t k = 0; k < i; ++k) first = first && !(trip(k, MLGPU_PROC_SAW_GEN) && g.nodes[k].in[0] == g.nodes[i].in[0]);
    for (size_t j = 0; first && j < g.nodes.size(); ++j)
      if (trip(j, MLGPU_PROC_PULSE_GEN) && g.nodes[j].in[0] == g.nodes[i].in[0])
      {
        p.nodes[i].lockedPartner = (int)j;
        break;
      }
  }
}

// The early reads' plan, made with the landing slots (planGraph): the delay nodes whose reads are issued at the top of the
// sample (earlyTop), the nodes their delay times are made of (earlyHoisted) and what each read leaves in flight (earlyPending).
// The nodes a delay time is computed from go to the top of the sample with the reads behind them, where nothing of this sample
// has been stored yet: plain nodes only (operators, inputs, one-vector feedback values, processors without rings - each keeps its
// own state, so their order among independent nodes is free), and only those whose inputs are such nodes themselves.
void planEarlyReads(const GraphDesc& g, GraphPlan& p)
{
  std::vector<char> movable(g.nodes.size(), 0), wanted(g.nodes.size(), 0);
  if (!p.earlyRows) return;
  for (size_t j = 0; j < g.nodes.size(); ++j)
  {
    const Node& m = g.nodes[j];
    if (m.rate != RATE_AUDIO)
    {
      movable[j] = 1;  // (a value per voice or per DSPVector: there before the sample loop)
      continue;
    }
    bool ok = m.region < 0 && m.role == ROLE_NONE && (m.type == NODE_OP || m.type == NODE_INPUT || m.type == NODE_FEEDBACK || m.type == NODE_VOP || (m.type == NODE_PROC && !mlgpu_proc_rings(m.kind) && p.nodes[j].streamLockSaw < 0));
    if (m.type != NODE_FEEDBACK)
      for (int in : m.in) ok = ok && movable[(size_t)in];
    movable[j] = ok;
  }
  for (size_t j = 0; j < g.nodes.size(); ++j)
  {
    const Node& m = g.nodes[j];
    if (p.nodes[j].earlySlot < 0) continue;
    bool all = true;
    for (size_t a = 1; a < m.in.size(); ++a) all = all && movable[(size_t)m.in[a]];
    if (!all) continue;
    for (size_t a = 1; a < m.in.size(); ++a) wanted[(size_t)m.in[a]] = 1;
    p.nodes[j].earlyTop = true;
  }
  // the audio-rate nodes the batch's delay times need, and theirs in turn (a node's inputs come before it)
  for (size_t j = g.nodes.size(); j-- > 0;)
  {
    const Node& m = g.nodes[j];
    if (!wanted[j] || m.rate != RATE_AUDIO) continue;
    p.nodes[j].earlyHoisted = true;
    if (m.type != NODE_FEEDBACK)
      for (int in : m.in) wanted[(size_t)in] = 1;
  }
  // what is still in flight behind a node's loads when they have landed: at least the loads of the batch issued after them
  int after = 0;
  for (size_t b = g.nodes.size(); b-- > 0;)
    if (p.nodes[b].earlyTop)
    {
      p.nodes[b].earlyPending = after;
      after += g.nodes[b].kind == MLGPU_PROC_PITCHBENDABLE_DELAY ? 2 : 1;
    }
}

std::string nodeExpr(const GraphDesc& g, const GraphPlan& p, size_t i, int l, const std::string& ph = "", const std::string& idx = "q * 4 + k")
{
  const Node& n = g.nodes[i];
  std::ostringstream s;
  const std::string L = "_" + std::to_string(l);
  // an input that lives in an enclosing region (or outside) carries only the phase letters of ITS regions
  auto arg = [&](size_t j) { return "n" + std::to_string(n.in[j]) + ph.substr(0, (size_t)upDepth(g, g.nodes[n.in[j]].region)) + L; };
  auto argsFrom = [&](size_t j0) {  // ", " before each of the inputs from j0 on
    std::string t;
    for (size_t j = j0; j < n.in.size(); ++j) t += ", " + arg(j);
    return t;
  };
  switch (n.type)
  {
    case NODE_INPUT: s << "xin" << n.slot << L << "[k]"; break;
    case NODE_CONTROL: s << "ctl" << n.slot << L << "[t * a.V]"; break;
    case NODE_EVENT_ROW:  // pitch and gate are CtlVoice's, the rows from vox on CtlRows'
      if (n.slot < 2) s << (n.slot == 0 ? "evP" : "evG") << L << "[k]";
      else s << "evR" << n.slot << L << "[k]";
      break;
    case NODE_PARAM: s << "a.params[(size_t)" << n.slot << " * a.V + v" << L << "]"; break;
    case NODE_CONST:
      if (g.liveConsts) s << "a.consts[" << n.slot << "]";  // wave-uniform: a scalar load, kept in an SGPR
      else s << floatLiteral(n.value);
      break;
    case NODE_PROC:
      if (ph.empty() && p.nodes[i].streamLockSaw >= 0)  // made with its partner just before the first of the two (emitNodes)
        s << "sl" << p.nodes[i].streamLockSaw << (n.kind == MLGPU_PROC_SAW_GEN ? "s" : "p") << L;
      else if (n.kind == MLGPU_PROC_TEMPO_LOCK && g.nodes[n.in[0]].type != NODE_INPUT)  // the phasor to follow is computed in this graph
        s << "p" << i << L << ".next_x(" << idx << ", " << arg(0) << ", " << arg(1) << ", " << arg(2) << ")";
      else if (mlgpu_proc_is_vector_rate(n.kind))
        s << "p" << i << L << ".next_n(" << idx << ")";
      else if (p.nodes[i].earlySlot >= 0)  // ring layout 0: the read was issued as soon as the delay time was known (emitNodes: pre), here the write and the value
        s << "p" << i << L << (n.kind == MLGPU_PROC_PITCHBENDABLE_DELAY ? ".post_i<" : ".post<") << p.nodes[i].earlyPending << ">("
          << (n.kind == MLGPU_PROC_PITCHBENDABLE_DELAY ? idx + ", " : std::string()) << arg(0) << ")";
      else if (n.kind == MLGPU_PROC_PITCHBENDABLE_DELAY)
        s << "p" << i << L << ".next_i(" << idx << ", " << arg(0) << ", " << arg(1) << ((p.rings == RingLayout::SECTORS && n.region < 0) ? ", qq * 4 + k" : "") << ")";
      else if (p.rings == RingLayout::SECTORS && n.region < 0 && mlgpu_proc_rings(n.kind))  // ring layout 4: the sample's place in its trip of 8
        s << "p" << i << L << ".next_k(qq * 4 + k, " << arg(0) << argsFrom(1) << ")";     // (a constant once qq and k are unrolled)
      else if (p.nodes[i].oscTrip)
        s << "osc" << i << L << "[qq * 4 + k]";  // made for the whole trip before the sample loop
      else if ((n.kind == MLGPU_PROC_SAW_GEN || n.kind == MLGPU_PROC_PULSE_GEN) && g.nodes[n.in[0]].rate == RATE_VOICE)
      {
        // launch-constant frequency: the polyBLEP range test was done once per wavefront (odd<i>)
        const bool widthSignal = n.in.size() == 2 && g.nodes[n.in[1]].rate != RATE_VOICE;
        s << "p" << i << L << (widthSignal ? ".next_uw(" : ".next_u(") << arg(0);
        if (n.in.size() == 2) s << ", " << arg(1);
        s << ", odd" << i << ")";
      }
      else if (n.kind == MLGPU_PROC_PULSE_GEN && (n.in.size() == 1 || g.nodes[n.in[1]].rate == RATE_VOICE))
      {
        // streamed frequency, launch-constant width: the width's range test was done once per wavefront (oddw<i>)
        s << "p" << i << L << ".next_sw(" << arg(0);
        if (n.in.size() == 2) s << ", " << arg(1);
        s << ", oddw" << i << ")";
      }
      else if (n.kind == MLGPU_PROC_PULSE_GEN && n.in.size() == 2)
        s << "p" << i << L << ".next2(" << arg(0) << ", " << arg(1) << ")";
      else
        s << "p" << i << L << ".next(" << (n.in.empty() ? std::string("0.f") : arg(0)) << argsFrom(1) << ")";
      break;
    case NODE_OP:
      if (n.kind == MLGPU_OP_CLAMP && clampHasConstBounds(g, n))
      {
        s << "clamp_const_bounds(" << arg(0) << ", " << arg(1) << ", " << arg(2) << ")";  // two instructions (mldsp_math.hpp)
        break;
      }
      s << "apply_f<" << n.kind << ">(" << arg(0) << argsFrom(1) << ")";
      break;
    case NODE_FEEDBACK:
      if (n.region < 0)
        s << "fbv" << i << L << "[k]";  // fetched for the whole quad before the sample loop
      else
        s << "u2f(a.state[(size_t)(" << n.sOff << " + " << idx << ") * a.V + v" << L << "])";
      break;
    case NODE_ROUTE:
      if (n.kind == MLGPU_ROUTE_MULTIPLEX || n.kind == MLGPU_ROUTE_MULTIPLEX_LINEAR)
        s << (n.kind == MLGPU_ROUTE_MULTIPLEX ? "route_multiplex_v(" : "route_multiplex_linear_v(") << arg(0) << argsFrom(1) << ")";
      else
        s << (n.kind == MLGPU_ROUTE_DEMULTIPLEX ? "route_demultiplex(" : "route_demultiplex_linear(") << arg(0) << ", " << arg(1) << ", "
          << n.slot << ", " << n.nOut << ")";
      break;
    case NODE_VOP:
      if (n.kind == MLGPU_VOP_TABLE)
      {
        s << "u2f(cv" << i << "[" << idx << "])";  // same index for every lane: a scalar load from constant memory
        break;
      }
      s << "vop<" << n.kind << ">(" << idx << argsFrom(0) << ")";
      break;
  }
  return s.str();
}

// The source of a graph's kernel, a pure function of the graph and the form: the facts every section needs are worked out once,
// and each section of the kernel is written by a member, in the order the kernel has them.
struct GraphEmitter
{
  const GraphDesc& g;
  const GraphPlan& p;
  const KernelForm& form;
  const int VL;
  std::ostringstream s;
  bool windowed, partialWaves, stateAddr32, PF, oscTrips, ringTrips;
  const bool listed;  // the listed form: a lane's place is its position in the voice list (vr), its voice the list's entry there (v)
  // ... by the host's lane plan (mlgpu_graph_process_listed_groups): a lane's place in the launch (vr) is a plan entry - its voice (v), its
  // list position (pl), the row of its instrument and its place in the segment of that instrument's listed voices - or a pad
  const bool planned;
  std::string ringLane, places;
  // ring layout 4, per wavefront: every delay node's held sectors (512 floats per ring) and history rows (1024 floats per node)
  std::vector<size_t> sectorLdsOff;
  size_t sectorLdsPerWave{0};
  GraphEmitter(const GraphDesc& graph, const GraphPlan& plan, const KernelForm& f) : g(graph), p(plan), form(f), VL(f.listed ? 1 : f.voicesPerLane), listed(f.listed), planned(f.listed && f.planned), sectorLdsOff(graph.nodes.size(), 0)
  {
    windowed = p.rings != RingLayout::ROWS && p.totalRings;
    if (p.rings == RingLayout::SECTORS)
      for (size_t i = 0; i < g.nodes.size(); ++i)
        if (g.nodes[i].type == NODE_PROC && g.nodes[i].ringLen)
        {
          sectorLdsOff[i] = sectorLdsPerWave;
          sectorLdsPerWave += (size_t)mlgpu_proc_rings(g.nodes[i].kind) * 512 + 1024;
        }
    // Ring layout 2 moves a voice's pieces with its NEIGHBOURS' lanes: a bank whose last wavefront is not full keeps that wavefront's
    // spare lanes running. They run the bank's last voice again - same inputs, same state, same stores - on ring memory and LDS
    // columns of their own (vr: the lane's place; the rings are laid out for whole 256-voice blocks and cleared together, so a spare
    // lane's ring always holds what the last voice's holds).
    // (... and so does an output that is the mixdown of all voices: the tree over a wavefront's 64 lanes, a spare lane adds +0)
    bool anyMix = false;
    for (size_t o = 0; o < g.outputs.size(); ++o) anyMix = anyMix || g.outputMix[o];
    partialWaves = ((p.rings == RingLayout::TRANSPOSED && p.totalRings) || anyMix) && (g.V % 64);
    // (the listed form: the list's length is known at the launch only - with a mixed-down output the last wavefront's spare lanes
    // always stay and run the list's last voice again; without one a lane past the list's end returns)
    if (listed) partialWaves = anyMix;
    if (planned) partialWaves = false;  // (the lane plan has no mixdown tree - planGraph -, and a lane at or past its end leaves)
    ringLane = partialWaves ? "vr" : "v";
    places = listed ? "a.listed" : "a.V";
    // a row of the state memory at this lane: the row's address is wave-uniform (scalar arithmetic), the lane's place a 32-bit offset on
    // it - one memory instruction where `a.state[row * a.V + v]` with a 64-bit v is a 64-bit vector add in front of it
    stateAddr32 = g.V < ((size_t)1 << 30) && !p.rowAddr64;
    PF = g.nInputs > 0;
    oscTrips = p.oscTrips;
    ringTrips = p.rings == RingLayout::SECTORS && p.totalRings;  // ring layout 4: trips of two quads, every ring's loads in the trip's prologue
    evVoice = (g.eventRowMask & 3u) != 0;
    evRows = g.eventRowMask & 0x7Cu;
    evMpe = g.mpeEvents && ((!listed && !planned) || g.voiceListMpeEvents);
  }
  // ... in the forms for either protocol (mlgpu_graph_enable_mpe_events: the plain kernel; mlgpu_graph_enable_voice_list_mpe_events: the
  // listed and the planned form too - CtlVoiceMpe / CtlRowsMpe make the voice's lane and its main lane of the gathered voice index)
  bool evMpe{false};
  bool evVoice{false};   // the graph reads pitch or gate: mlev::CtlVoice
  unsigned evRows{0};    // its rows among vox, z, x, y, mod (bit r = row r): mlev::CtlRows<evRows>, emitted only where there is one
  static std::string sfx(int l) { return "_" + std::to_string(l); }
  static std::string name(int j, const std::string& ph, int l) { return "n" + std::to_string(j) + ph + sfx(l); }
  // a group sum of 16 voices (one instrument's voices): four quads of the wavefront's 64 voices are parked in LDS and every lane
  // then adds up ONE (instrument, sample) pair in voice order - 2.3 instructions per voice-sample where the lane-shift chain
  // (group_sum_in_order) takes 16
  bool ldsSum(size_t o) const { return !planned && VL == 1 && g.outputGroup[o] == 16; }
  // the lane plan's group sum, for every group size: a group's listed voices are a SEGMENT of the wavefront's lanes, parked in the
  // wavefront's segment strip and added up in rank order by the segment's last lane (mldsp_math.hpp: segment_park / segment_sum_store)
  bool segSum(size_t o) const { return planned && g.outputGroup[o] != 0; }
  std::string stateRef(const std::string& row, int l) const
  {
    return stateAddr32 ? "*state_row(a, " + row + ", v4" + sfx(l) + ")" : "a.state[(size_t)(" + row + ") * a.V + v" + sfx(l) + "]";
  }
  // a PulseGen's width: its input, or its own coefficient
  std::string width(size_t j, int l) const
  {
    const Node& m = g.nodes[j];
    return m.in.size() == 2 ? "n" + std::to_string(m.in[1]) + sfx(l) : "p" + std::to_string(j) + sfx(l) + ".width";
  }
  // expr(l) of every voice of the lane, or-ed; and the wave-uniform ballot of such a test
  template <class F>
  std::string anyVoice(F expr) const
  {
    std::string t;
    for (int l = 0; l < VL; ++l) t += (l ? " || " : "") + expr(l);
    return t;
  }
  static std::string ballot(const std::string& test) { return "__builtin_amdgcn_ballot_w64(" + test + ")"; }
  // node j's value for every voice of the lane, in a region's phase `ph` at sample index `idx`
  void value(size_t j, const std::string& indent, const std::string& ph = "", const std::string& idx = "q * 4 + k")
  {
    for (int l = 0; l < VL; ++l)
      s << indent << "const float " << name((int)j, ph, l) << " = " << nodeExpr(g, p, j, l, ph, idx) << ";"
        << (l == 0 && !g.nodes[j].name.empty() ? "  // " + g.nodes[j].name : std::string()) << "\n";
  }
  void header()
  {
    // (the listed kernel of ring layout 4 - mlgpu_graph_enable_voice_list_rings - runs its trips on each LANE's write clock: voices that
    // were off the list for different numbers of DSPVectors have write indices that differ by multiples of 64; RingCore::beginS)
    // (... and decides per LANE what a wavefront of the plain kernel decides once for voices that never change: MLGPU_RING_BY_LANE)
    const std::string ringWindows = p.rings == RingLayout::ROWS ? std::string() : "#define MLGPU_RING_WINDOWS " + std::to_string((int)p.rings) + "\n" +
                                    ((listed && p.ringByLane) ? "#define MLGPU_RING_BY_LANE 1\n" : "") + ((listed && p.ringLaneClock) ? "#define MLGPU_RING_LANE_CLOCK 1\n" : "");
    s << "// generated by libmlgpu graph.hip (" << VL << " voice" << (VL > 1 ? "s" : "") << " per lane" << (planned ? ", the voices of a list by its lane plan" : listed ? ", the voices of a list" : "") << ")\n" << ringWindows
      << (g.strictSvf ? "#define MLGPU_SVF_STRICT 1\n" : "") << "#include \"mldsp_kernels.hpp\"\n#include \"mldsp_ops.hpp\"\n"
      << (g.hasEventRows ? "#include \"mldsp_events.hpp\"\n" : "") << "using namespace mldev;\n";
    for (size_t i = 0; i < g.nodes.size(); ++i)
      if (g.nodes[i].type == NODE_VOP && g.nodes[i].kind == MLGPU_VOP_TABLE)
      {
        s << "__constant__ unsigned cv" << i << "[64] = {";
        for (int j = 0; j < 64; ++j) s << (j ? ", " : "") << "0x" << std::hex << g.nodes[i].table[j] << std::dec << "u";
        s << "};\n";
      }
    // windowed rings: the latency of a sector refill is hidden by other waves only, so keep at least two per SIMD
    // (the listed forms with rings - mlgpu_graph_enable_voice_list_rings - take the same bounds: they count wavefronts per SIMD and registers
    // per lane, and a lane of a listed launch holds one voice's windows like any other)
    const std::string bound = (p.rings == RingLayout::TRANSPOSED && p.totalRings == 1) ? ", 4" : ringTrips ? ", 1" : windowed ? ", 2"
                              : form.minWaves ? ", " + std::to_string(form.minWaves) : std::string();
    s << "extern \"C\" __global__ __launch_bounds__(256" << bound << ") void " << (listed ? "mlgpu_graph_listed_kernel" : "mlgpu_graph_kernel") << "(const GraphArgs a)\n{\n  apply_fp_mode(a.flags);\n";
  }
  void sharedMemory()
  {
    if (g.hasImpulse) s << "  __shared__ float ldsTable[32];\n  if (threadIdx.x < 17) ldsTable[threadIdx.x] = a.impulseTable[threadIdx.x];\n  __syncthreads();\n";
    s << "  const KernelTables tables{" << (g.hasImpulse ? "ldsTable" : "nullptr") << "};\n";
    if (p.rings == RingLayout::TRANSPOSED && p.totalRings)
      s << "  __shared__ float ldsRings[" << (size_t)p.totalRings * 4 << " * kTStrip];  // [ring][wavefront][40 rows][64]: write window + two read chunks\n";
    if (ringTrips) s << "  __shared__ __attribute__((aligned(16))) float ldsRings[" << 4 * sectorLdsPerWave << "];  // [wavefront][node: held sectors, history rows]\n";
    else if (p.rings == RingLayout::WINDOWS && p.totalRings) s << "  __shared__ float ldsRings[" << (size_t)p.totalRings * 8 * 256 << "];  // write windows, [ring][8][256 lanes]\n";
    if (p.earlyRows)
      s << "  __shared__ float ldsEarly[" << 4 * p.earlySlots * 64 << "];  // [wavefront][ring read][64 lanes]: where the early ring reads land\n"
        << "  float* const ldsEarlyWave = ldsEarly + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * " << p.earlySlots * 64 << ";\n";
    for (size_t o = 0; o < g.outputs.size(); ++o)
      if (ldsSum(o))
        s << "  __shared__ float ldsSum" << o << "[4 * kGroup16Strip];\n  float* const strip" << o << " = ldsSum" << o << " + (threadIdx.x >> 6) * kGroup16Strip;\n";
    for (size_t o = 0; o < g.outputs.size(); ++o)
      if (segSum(o))
        s << "  __shared__ __attribute__((aligned(16))) float ldsSeg" << o << "[4 * kSegmentStrip + kSegmentTail];\n  float* const seg" << o << " = ldsSeg" << o
          << " + (threadIdx.x >> 6) * kSegmentStrip;\n";
    for (size_t o = 0; o < g.outputs.size(); ++o)
      if (g.outputMix[o])
        s << "  __shared__ __attribute__((aligned(16))) float ldsMix" << o << "[4 * kMixStrip];\n  float* const mstrip" << o << " = ldsMix" << o << " + (threadIdx.x >> 6) * kMixStrip;\n";
  }
  // the lane's voices, then once per voice: processor state, signal bases, voice-rate nodes
  void voiceSetup()
  {
    s << "  size_t blk = blockIdx.x;\n  const size_t nbFull = (size_t)gridDim.x & ~(size_t)7;\n"
         "  if (blk < nbFull) blk = (blk & 7) * (nbFull >> 3) + (blk >> 3);\n";
    if (planned)
    {
      // The lane's place in the launch (vr) and its plan entry, one 16-byte load: .x the voice (v), .y the list position (pl: plain
      // outputs and peaks), .z the row of its instrument, .w rank | length << 8 in its segment. A lane at or past the plan's end and a
      // pad leave here - after the impulse table's barrier, the only one of the kernel, and before every wave-uniform ballot below,
      // which so counts the wavefront's voices alone. A pad loads, runs and stores nothing.
      // (Rings in layouts 1 and 4 - mlgpu_graph_enable_voice_list_rings: the return stays safe. Neither layout has a barrier - layout 1's
      // write window is the lane's own LDS column, layout 4's held sectors and history rows are the lane's own columns of its wavefront's
      // strip - and their ballots ask "some lane of those still here": RingCore's trip code then goes by the lane's own w, sectors and
      // column. A lane that left holds no sector and owes no flush.)
      s << "  const size_t vr_0 = blk * 256 + threadIdx.x;\n  if (vr_0 >= a.listed) return;\n  const uint4 plan = ((const uint4*)a.lanePlan)[vr_0];\n"
           "  if (plan.x == 0xFFFFFFFFu) return;  // a pad\n  const size_t v_0 = plan.x, pl_0 = plan.y;\n"
           "  const unsigned rank_0 = plan.w & 0xFFu, length_0 = plan.w >> 8;\n  __builtin_assume(length_0 != 0u);\n  uint32_t pk_0 = 0u;\n";
      // the wavefront's longest segment, rounded up to a size segment_sum_store has the reads of
      s << "  const int longest = " << ballot("length_0 > 8u") << " ? 16 : (" << ballot("length_0 > 4u") << " ? 8 : (" << ballot("length_0 > 2u") << " ? 4 : 2));\n";
    }
    else if (listed)
    {
      // the lane's place in the list (vr), the place whose voice it runs and whose rows it stores to (pl), the voice (v): everything
      // below that is made of v - tables, ring rows, input rows, control columns - is the gathered voice's
      // Rings in layouts 1 and 4 (mlgpu_graph_enable_voice_list_rings): ring MEMORY is addressed by v (procSetup: the voice's 32-byte
      // sectors of its 256-voice block), the LDS windows by threadIdx.x - the split a gathered voice needs. The early return of the lanes
      // past the list stands: after the impulse table's barrier these layouts have none (layout 2's wave barriers are not served), and
      // every ballot of RingCore asks the lanes that are still here.
      // The spare lanes of a mixed-down output's last wavefront run the list's last voice again in lockstep with its real lane: the same
      // state, inputs and delay times, so the same w, the same sectors and the same floats at every instruction. Layout 1: each keeps
      // the write window in its own LDS column and both flush the same sector with the same eight floats, by one store instruction -
      // whichever lane's write lands last, the sector holds those floats, and a later refill by either reads them. Layout 4: both store
      // and load the same positions by the same instructions, held sectors and history rows in columns of their own. Loads and stores
      // of a wavefront complete in issue order, so no lane ever reads a sector between two different values of it: there are none.
      s << "  const size_t vr_0 = blk * 256 + threadIdx.x;\n";
      if (partialWaves) s << "  if ((vr_0 & ~(size_t)63) >= a.listed) return;\n  const size_t pl_0 = vr_0 < a.listed ? vr_0 : a.listed - 1;\n";
      else s << "  if (vr_0 >= a.listed) return;\n  const size_t pl_0 = vr_0;\n";
      s << "  const size_t v_0 = a.voiceList[pl_0];\n  uint32_t pk_0 = 0u;\n";
    }
    else if (partialWaves)
      s << "  const size_t vr_0 = blk * 256 + threadIdx.x;\n  if ((vr_0 & ~(size_t)63) >= a.V) return;\n  const size_t v_0 = vr_0 < a.V ? vr_0 : a.V - 1;\n";
    else
      s << "  const size_t v_0 = blk * " << 256 * VL << " + threadIdx.x;\n  if (v_0 >= a.V) return;\n";
    if (stateAddr32) s << "  const uint32_t v4_0 = (uint32_t)v_0 * 4u;\n";
    // a lane whose second voice does not exist recomputes its first one: same inputs, same state, same stores
    for (int l = 1; l < VL; ++l)
    {
      s << "  const size_t v" << sfx(l) << " = (v_0 + " << 256 * l << " < a.V) ? v_0 + " << 256 * l << " : v_0;\n";
      if (stateAddr32) s << "  const uint32_t v4" << sfx(l) << " = (uint32_t)v" << sfx(l) << " * 4u;\n";
    }
    for (size_t i = 0; i < g.nodes.size(); ++i)
    {
      const Node& n = g.nodes[i];
      for (int l = 0; l < VL; ++l)
      {
        const std::string L = sfx(l);
        if (n.type == NODE_PROC)
          procSetup(i, L);
        else if (n.type == NODE_INPUT)
        {
          const std::string row = g.inputGroup[n.slot] > 1 ? "(v" + L + " / " + std::to_string(g.inputGroup[n.slot]) + ")" : "v" + L;
          s << "  const f32x4* in" << n.slot << L << " = (const f32x4*)a.in[" << n.slot << "].base + " << row << " * a.in[" << n.slot << "].strideV;\n";
        }
        else if (n.type == NODE_CONTROL)
          s << "  const float* ctl" << n.slot << L << " = a.ctl[" << n.slot << "] + v" << L << ";\n";
      }
      if (n.rate == RATE_VOICE && n.type != NODE_PROC) value(i, "  ");
    }
  }
  // processor i of voice L: its object, its memory (VoiceMem: coefficients, state, rings), its state loaded
  void procSetup(size_t i, const std::string& L)
  {
    const Node& n = g.nodes[i];
    s << "  Proc<" << n.kind << "> p" << i << L << ";\n  const VoiceMem m" << i << L << "{a.coeffs + (size_t)" << n.cOff << " * a.V + v" << L
      << ", a.state + (size_t)" << n.sOff << " * a.V + v" << L << ", a.V";
    // (a ring of at most 4 GiB over the bank: 32-bit row offsets from the wave-uniform start of the ring)
    const bool a32 = n.ringLen && p.rowAddr32 && (size_t)n.ringLen * g.V * sizeof(float) <= ((size_t)1 << 32) && n.ringLen < ((size_t)1 << 24);
    const bool rows = p.rings == RingLayout::ROWS;
    if (n.ringLen && rows) s << ", a.mem + (size_t)" << p.nodes[i].memOff << " * a.V" << (a32 ? std::string() : " + v" + L) << ", " << (n.ringLen - 1) << "u";
    if (n.ringLen && rows && (p.nodes[i].earlySlot >= 0 || a32)) s << ", " << (p.nodes[i].earlySlot >= 0 ? "ldsEarlyWave + " + std::to_string(p.nodes[i].earlySlot * 64) : std::string("nullptr"));
    if (a32) s << ", 0u, (uint32_t)v" << L << " * 4u, (uint32_t)a.V * 4u, true";
    if (n.ringLen && p.rings == RingLayout::TRANSPOSED)
      s << ", a.mem + (size_t)" << p.nodes[i].memOff << " * ((a.V + 255) & ~(size_t)255) + (" << ringLane << L << " >> 8) * (size_t)" << n.ringLen * (size_t)mlgpu_proc_rings(n.kind) * 256
        << " + (" << ringLane << L << " & 255) * 16, " << (n.ringLen - 1)
        << "u, ldsRings + (" << (size_t)p.nodes[i].ringSlot * 4 << " + (threadIdx.x >> 6)) * kTStrip + (threadIdx.x & 63)";
    else if (n.ringLen && !rows)
      s << ", a.mem + (size_t)" << p.nodes[i].memOff << " * ((a.V + 255) & ~(size_t)255) + (v" << L << " >> 8) * (size_t)" << n.ringLen * (size_t)mlgpu_proc_rings(n.kind) * 256
        << " + (v" << L << " & 255) * 8, " << (n.ringLen - 1)
        << "u, ldsRings + " << (p.rings == RingLayout::SECTORS ? "(threadIdx.x >> 6) * " + std::to_string(sectorLdsPerWave) + " + " + std::to_string(sectorLdsOff[i]) + ", " + std::to_string((size_t)mlgpu_proc_rings(n.kind) * 512) + "u"
                                                           : std::to_string((size_t)p.nodes[i].ringSlot * 8 * 256) + " + threadIdx.x");
    s << "};\n  p" << i << L << ".load(m" << i << L << ", tables);\n";
  }
  // the oscillators' wave-uniform tests, asked once per launch
  void oscillatorTests()
  {
    for (size_t i = 0; i < g.nodes.size(); ++i)
    {
      const Node& n = g.nodes[i];
      const bool pulseVoiceWidth = n.type == NODE_PROC && n.kind == MLGPU_PROC_PULSE_GEN && (n.in.size() == 1 || g.nodes[n.in[1]].rate == RATE_VOICE);
      auto widthOdd = [&](int l) { return "pulse_width_is_odd(" + width(i, l) + ")"; };
      if (n.type == NODE_PROC && (n.kind == MLGPU_PROC_SAW_GEN || n.kind == MLGPU_PROC_PULSE_GEN) && g.nodes[n.in[0]].rate == RATE_VOICE)
      {
        // a PulseGen whose width is per voice too (its own coefficient, or a voice-rate node): the width's range joins the test
        const std::string odd = anyVoice([&](int l) { return "blep_freq_is_odd(" + name(n.in[0], "", l) + ")"; });
        s << "  const bool odd" << i << " = " << ballot(pulseVoiceWidth ? odd + " || " + anyVoice(widthOdd) : odd) << " != 0;\n";
        if (p.nodes[i].oscTrip)
          s << "  const bool dense" << i << " = odd" << i << " || "
            << ballot(anyVoice([&](int l) { return "trip_freq_is_dense(" + name(n.in[0], "", l) + ", " + std::to_string(p.oscTripQ * 4) + ")"; })) << " != 0;\n";
      }
      else if (pulseVoiceWidth)
        s << "  const bool oddw" << i << " = " << ballot(anyVoice(widthOdd)) << " != 0;\n";
    }
    // a Saw / Pulse pair whose phase counters are equal in every lane of the wavefront
    auto counters = [&](size_t i, int j) {
      return ballot(anyVoice([&](int l) { return "p" + std::to_string(i) + sfx(l) + ".omega32 != p" + std::to_string(j) + sfx(l) + ".omega32"; })) + " == 0;\n";
    };
    for (size_t i = 0; i < g.nodes.size(); ++i)
      if (p.nodes[i].lockedPartner >= 0)
        s << "  const bool locked" << i << " = !dense" << i << " && !dense" << p.nodes[i].lockedPartner << " && " << counters(i, p.nodes[i].lockedPartner);
    for (size_t i = 0; i < g.nodes.size(); ++i)
      if (p.nodes[i].streamLockPulse >= 0) s << "  const bool slocked" << i << " = " << counters(i, p.nodes[i].streamLockPulse);
  }
  void outputsAndPrefetch()
  {
    for (size_t o = 0; o < g.outputs.size(); ++o)
      for (int l = 0; l < VL; ++l)
      {
        if (segSum(o))  // row j of a signal of J rows: the lane's instrument among the listed ones
          s << "  f32x4* out" << o << sfx(l) << " = (f32x4*)a.out[" << o << "].base + (size_t)plan.z * a.out[" << o << "].strideV;\n";
        else if (g.outputMix[o])  // the rows of 64-voice group sums (mlgpu_mixdown's first stage): [(group * T + t) * 64 + sample]
          s << "  float* const out" << o << sfx(l) << " = (float*)a.out[" << o << "].base + ((" << ringLane << sfx(l) << " >> 6) * a.T) * 64;\n";
        else if (g.outputGroup[o])
          s << "  f32x4* out" << o << sfx(l) << " = (f32x4*)a.out[" << o << "].base + (v" << sfx(l) << " / " << g.outputGroup[o] << ") * a.out[" << o << "].strideV;\n";
        else
          s << "  f32x4* out" << o << sfx(l) << " = (f32x4*)a.out[" << o << "].base + " << (listed ? "pl" : "v") << sfx(l) << " * a.out[" << o << "].strideV;\n";
      }
    // a Downsample2x region's filter pairs its parent's samples (m - 1, m): the previous sample of each of its sources
    for (const Region& R : g.regions)
      if (R.kind == MLGPU_REGION_DOWNSAMPLE_2X)
        for (int in : R.ins)
          for (int l = 0; l < VL; ++l) s << "  float prev" << in << sfx(l) << " = 0.f;\n";
    // EventsToSignals rows made here from the control records of e2s_ctl_kernel: one CtlVoice per voice (lane == voice index: MIDI protocol)
    // The listed forms (mlgpu_graph_enable_voice_list_events): v is the gathered voice - the control record, the two side signals and the
    // drift glide's words are all addressed by it. Pads and lanes past the plan's or the list's end have left before CtlVoice's
    // wave-uniform ballots. The spare lanes of a last wavefront (partialWaves: they run the list's - or the bank's - last voice again)
    // are NOT masked: their CtlVoice stores are the last voice's own words with the same bits. Read from mldsp_events.hpp: every word
    // CtlVoice stores (setGlideWord in quad() and store()) is a function of the words it loaded for voice v and of kernel arguments; the
    // spare lanes sit in the last voice's wavefront and take every branch it takes (fetch, moving, rows are the same per-voice values), so
    // a word's loads and stores are issued by the same instructions for all of them; and within a launch no word is loaded after it was
    // stored except by a LATER instruction that wants the stored value (slot 63 and the first quad's slots at the next begin_vector).
    // (CtlVoice where the graph reads pitch or gate; the rows vox, z, x, y, mod are mlev::CtlRows', which only reads - by the same voice)
    // The listed forms for either protocol (mlgpu_graph_enable_voice_list_mpe_events): all of the above holds for CtlVoiceMpe - its stores
    // are CtlVoice's, by the voice's lane, a function of v alone - and what it adds is read-only: the main lane's record, held words and
    // frames, by an address made of v. Nothing in the two structs looks at a neighbouring lane or assumes a wavefront of one instrument's
    // voices: the ballots ask "some lane of the wavefront" and each lane then goes by its own flag, so a wavefront of voices of arbitrary
    // instruments in arbitrary order reads each flagged main lane's frames where they are. A spare lane reads the last voice's lane and
    // main lane again.
    if (evVoice)
      for (int l = 0; l < VL; ++l) s << "  mlev::CtlVoice" << (evMpe ? "Mpe" : "") << " ev" << sfx(l) << ";\n  ev" << sfx(l) << ".load(a.events, v" << sfx(l) << ", a.T);\n";
    if (evRows)
      for (int l = 0; l < VL; ++l)
        s << "  mlev::CtlRows" << (evMpe ? "Mpe" : "") << "<" << evRows << "u> er" << sfx(l) << ";\n  er" << sfx(l) << ".load(a.events, v" << sfx(l) << ", a.T);\n";
    // Streamed inputs one quad (or one trip) ahead: a wavefront that loads a quad and waits for it right away stands still for a
    // whole HBM round trip per quad, and with four wavefronts per SIMD there are long stretches with only one or two of them able to
    // issue (one wavefront alone issues at 40 % of the SIMD's rate). The very last quad of a launch loads itself again.
    if (PF) s << "  if (a.T == 0) return;\n";
    for (int i = 0; PF && i < g.nInputs; ++i)
      for (int l = 0; l < VL; ++l)
        s << "  const f32x4* pf" << i << sfx(l) << " = in" << i << sfx(l) << ";\n  f32x4 nx" << i << sfx(l) << " = __builtin_nontemporal_load(pf" << i << sfx(l) << ");\n";
    for (size_t i = 0; i < g.nodes.size(); ++i)
      if (g.nodes[i].type == NODE_FEEDBACK && g.nodes[i].region < 0)
        for (int l = 0; l < VL; ++l)
        {
          const std::string nm = std::to_string(i) + sfx(l);
          s << "  float fbn" << nm << "[4], fbm" << nm << "[4];\n#pragma unroll\n  for (int kk = 0; kk < 4; ++kk)\n  {\n    fbn" << nm << "[kk] = u2f(" << stateRef(std::to_string(g.nodes[i].sOff) + " + kk", l)
            << ");\n    fbm" << nm << "[kk] = u2f(" << stateRef(std::to_string(g.nodes[i].sOff) + " + 4 + kk", l) << ");\n  }\n";
        }
    s << "  const uint32_t turn0 = wave_slot();\n";
  }
  // the DSPVector loop's head: vector-rate nodes, the vector-rate processors' begin_vector, the trips' and quads' loops
  void vectorHead()
  {
    s << "  for (size_t t = 0; t < a.T; ++t)\n  {\n";
    // (Rounds 3-4 walked the event records inside this kernel - 134 spilled registers, 0.35 scalar / branch instructions per vector
    // one; round 5: the record walk is e2s_ctl_kernel's, this kernel expands its control records - mldsp_events.hpp.)
    if (evVoice)
      for (int l = 0; l < VL; ++l) s << "    ev" << sfx(l) << ".begin_vector(t);\n";
    if (evRows)
      for (int l = 0; l < VL; ++l) s << "    er" << sfx(l) << ".begin_vector(t);\n";
    for (size_t i = 0; i < g.nodes.size(); ++i)
    {
      const Node& n = g.nodes[i];
      if (n.rate == RATE_VECTOR) value(i, "    ");
      if (n.type != NODE_PROC || (n.kind == MLGPU_PROC_TEMPO_LOCK && g.nodes[n.in[0]].type != NODE_INPUT)) continue;
      if (n.kind == MLGPU_PROC_TEMPO_LOCK)
      {
        const int slot = g.nodes[n.in[0]].slot;  // the streamed input: first two samples of this vector
        for (int l = 0; l < VL; ++l)
          s << "    { const f32x4 x01 = in" << slot << sfx(l) << "[t * a.in[" << slot << "].strideT]; p" << i << sfx(l) << ".begin_vector(x01[0], x01[1], n"
            << n.in[1] << sfx(l) << ", n" << n.in[2] << sfx(l) << "); }\n";
      }
      else if (mlgpu_proc_is_vector_rate(n.kind))
        for (int l = 0; l < VL; ++l) s << "    p" << i << sfx(l) << ".begin_vector(n" << n.in[0] << sfx(l) << ");\n";
    }
    if (oscTrips || ringTrips)
      tripHead();
    else
    {
      s << "#pragma unroll " << (windowed ? 1 : form.quadsPerTrip) << "\n    for (int q = 0; q < 16; ++q)\n    {\n";
      s << "      if ((q & 1) == 0) take_turns_by_clock(turn0, " << kHostTurnClockShift << ");\n";
    }
    quadHead();
  }
  // the quads in trips of oscTripQ: the oscillators' samples of a trip first, then its quads (fully unrolled: qq is a constant)
  void tripHead()
  {
    const int tq = ringTrips ? 2 : p.oscTripQ, unroll = windowed ? 1 : std::max(1, form.quadsPerTrip / tq);
    s << "#pragma unroll " << unroll << "\n    for (int q2 = 0; q2 < 16; q2 += " << tq << ")\n    {\n";
    s << "    take_turns_by_clock(turn0, " << kHostTurnClockShift << ");\n";
    std::vector<char> paired(g.nodes.size(), 0);
    for (size_t i = 0; i < g.nodes.size(); ++i)
      if (p.nodes[i].lockedPartner >= 0) paired[i] = paired[(size_t)p.nodes[i].lockedPartner] = 1;
    auto tripU = [&](size_t i, int l, const char* indent, bool withWidth) {
      const Node& n = g.nodes[i];
      s << indent << "p" << i << sfx(l) << ".trip_u<" << tq * 4 << ">(n" << n.in[0] << sfx(l);
      if (withWidth && n.in.size() == 2) s << ", n" << n.in[1] << sfx(l);
      s << ", odd" << i << ", dense" << i << ", osc" << i << sfx(l) << ");\n";
    };
    for (size_t i = 0; i < g.nodes.size(); ++i)
    {
      if (!p.nodes[i].oscTrip) continue;
      for (int l = 0; l < VL; ++l) s << "    float osc" << i << sfx(l) << "[" << tq * 4 << "];\n";
      if (paired[i]) continue;  // made with its partner below
      for (int l = 0; l < VL; ++l) tripU(i, l, "    ", true);
    }
    for (size_t i = 0; i < g.nodes.size(); ++i)
    {
      const int j = p.nodes[i].lockedPartner;
      if (j < 0) continue;
      for (int l = 0; l < VL; ++l) s << "    const uint32_t keep" << i << sfx(l) << " = p" << i << sfx(l) << ".omega32, keep" << j << sfx(l) << " = p" << j << sfx(l) << ".omega32;\n";
      s << "    bool made" << i << " = locked" << i << ";\n";
      for (int l = 0; l < VL; ++l)
        s << "    if (made" << i << ") made" << i << " = trip_locked<" << tq * 4 << ">(p" << i << sfx(l) << ", p" << j << sfx(l) << ", n" << g.nodes[i].in[0] << sfx(l) << ", " << width((size_t)j, l)
          << ", osc" << i << sfx(l) << ", osc" << j << sfx(l) << ");\n";
      // (two voices per lane: a suspect trip of the second voice sends both back - the first one's counters are restored below)
      s << "    if (!made" << i << ")\n    {\n";
      for (int l = 0; l < VL; ++l)
      {
        s << "      p" << i << sfx(l) << ".omega32 = keep" << i << sfx(l) << ";\n      p" << j << sfx(l) << ".omega32 = keep" << j << sfx(l) << ";\n";
        tripU(i, l, "      ", false);
        tripU((size_t)j, l, "      ", true);
      }
      s << "    }\n";
    }
    // ring layout 4: every ring's loads of the trip together, before any arithmetic. The listed forms too: each lane predicts its OWN
    // read position from its own w and delay time and loads its own voice's sectors (tripBegin), the ballots only ask whether some lane needs to
    if (ringTrips)
      for (size_t i = 0; i < g.nodes.size(); ++i)
        if (g.nodes[i].type == NODE_PROC && g.nodes[i].region < 0 && mlgpu_proc_rings(g.nodes[i].kind))
          for (int l = 0; l < VL; ++l) s << "    p" << i << sfx(l) << ".trip_begin();\n";
    s << "#pragma unroll\n    for (int qq = 0; qq < " << tq << "; ++qq)\n    {\n      const int q = q2 + qq;\n";
  }
  // the quad's head: the next quad's inputs, the quad's feedback values, then the sample loop
  void quadHead()
  {
    // the next quad's address: one step on; from a vector's last quad to the next vector's first; the launch's last quad stays
    if (PF) s << "      const bool lastQ = (q == 15), lastT = (t + 1 == a.T);\n";
    for (int i = 0; i < g.nInputs; ++i)
      for (int l = 0; l < VL; ++l)
      {
        s << "      const f32x4 xin" << i << sfx(l) << " = nx" << i << sfx(l) << ";\n      pf" << i << sfx(l) << " += lastQ ? (lastT ? (size_t)0 : a.in[" << i
          << "].strideT - 15 * a.in[" << i << "].strideQ) : a.in[" << i << "].strideQ;\n      nx" << i << sfx(l) << " = __builtin_nontemporal_load(pf" << i << sfx(l) << ");\n";
      }
    for (size_t o = 0; o < g.outputs.size(); ++o)
      for (int l = 0; l < VL; ++l) s << "      f32x4 y" << o << sfx(l) << ";\n";
    if (evVoice)
      for (int l = 0; l < VL; ++l)
        s << "      mlev::CtlVoice" << (evMpe ? "Mpe" : "") << "::f32x4e evP" << sfx(l) << ", evG" << sfx(l) << ";\n      ev" << sfx(l) << ".quad(t, q, evP" << sfx(l) << ", evG" << sfx(l) << ");\n";
    if (evRows)
      for (int l = 0; l < VL; ++l)
      {
        s << "      er" << sfx(l) << ".quad(t, q);\n";
        for (int r = 2; r <= 6; ++r)
          if ((evRows >> r) & 1u) s << "      const f32x4 evR" << r << sfx(l) << " = er" << sfx(l) << ".row<" << r << ">(t, q);\n";
      }
    // A kept DSPVector's slot n is read and rewritten at sample n only: the quad's four slots are fetched together - and TWO QUADS
    // AHEAD (round 5; they were written 14 quads ago). Fetched at the top of the quad that uses them, every quad of a feedback graph
    // stood still for a memory round trip, behind the stores of the quad before (memory operations of a wavefront complete in issue
    // order): 256 round trips per launch of 16 DSPVectors were the whole launch time of the plucked-string bank, whatever the ring
    // layout.
    for (size_t i = 0; i < g.nodes.size(); ++i)
      if (g.nodes[i].type == NODE_FEEDBACK && g.nodes[i].region < 0)
        for (int l = 0; l < VL; ++l)
        {
          const std::string nm = std::to_string(i) + sfx(l);
          s << "      float fbv" << nm << "[4];\n#pragma unroll\n      for (int kk = 0; kk < 4; ++kk)\n      {\n        fbv" << nm << "[kk] = fbn" << nm << "[kk];\n        fbn" << nm
            << "[kk] = fbm" << nm << "[kk];\n        fbm" << nm << "[kk] = u2f(" << stateRef(std::to_string(g.nodes[i].sOff) + " + ((q + 2) & 15) * 4 + kk", l) << ");\n      }\n";
        }
    for (size_t i = 0; i < g.nodes.size(); ++i)
      if (g.nodes[i].type == NODE_PROC && (g.nodes[i].kind == MLGPU_PROC_LINEAR_GLIDE || g.nodes[i].kind == MLGPU_PROC_HALF_BAND_BUFFERED))
        for (int l = 0; l < VL; ++l) s << "      p" << i << sfx(l) << ".begin_quad(q);\n";
    s << "#pragma unroll\n      for (int k = 0; k < 4; ++k)\n      {\n";
  }
  // Rate regions are emitted in place, recursively. A context = where we are in the tree of regions: the phase letters
  // that name its values, the sample index inside the current function's own DSPVector, and that function's vector count.
  struct Ctx { std::string sfx, idx, vec, indent; };
  bool isInside(int r, int ancestor) const  // r == ancestor or nested somewhere inside it
  {
    for (; r >= 0; r = g.regions[(size_t)r].parent)
      if (r == ancestor) return true;
    return false;
  }
  int childUnder(int r, int ancestor) const  // the region directly under `ancestor` that contains r
  {
    while (g.regions[(size_t)r].parent != ancestor) r = g.regions[(size_t)r].parent;
    return r;
  }
  // the outer value a region input carries, in the phase of ITS region
  std::string regionSource(int in, const Ctx& c, int l) const
  {
    const int src = g.nodes[(size_t)in].in[0];
    return name(src, c.sfx.substr(0, (size_t)upDepth(g, g.nodes[(size_t)src].region)), l);
  }
  // ring layout 0: where a delay node's read goes - right after the last audio-rate node its delay time needs (-1: at the sample's top)
  void emitPre(size_t dn, const Ctx& c)
  {
    const Node& m = g.nodes[dn];
    for (int l = 0; l < VL; ++l)
    {
      s << c.indent << "p" << dn << sfx(l) << (m.kind == MLGPU_PROC_PITCHBENDABLE_DELAY ? ".pre_i(" + c.idx : ".pre(");
      for (size_t a = 1; a < m.in.size(); ++a) s << ((a > 1 || m.kind == MLGPU_PROC_PITCHBENDABLE_DELAY) ? ", " : "") << name(m.in[a], "", l);
      s << ");\n";
    }
  }
  // a SawGen / PulseGen pair on one streamed frequency: both values are made where the first of the two stands
  void streamLockPair(int si, const Ctx& c)
  {
    const int pj = p.nodes[(size_t)si].streamLockPulse;
    const Node &sn = g.nodes[(size_t)si], &pn = g.nodes[(size_t)pj];
    for (int l = 0; l < VL; ++l)
    {
      const std::string freq = name(sn.in[0], "", l), w = width((size_t)pj, l);
      s << c.indent << "float sl" << si << "s" << sfx(l) << ", sl" << si << "p" << sfx(l) << ";\n";
      // (the usual case - counters equal, widths regular - behind ONE wave-uniform test per sample)
      s << c.indent << "if (slocked" << si << " && !oddw" << pj << ") step_locked_stream<true>(p" << si << sfx(l) << ", p" << pj << sfx(l) << ", " << freq << ", " << w << ", sl" << si
        << "s" << sfx(l) << ", sl" << si << "p" << sfx(l) << ");\n";
      s << c.indent << "else if (slocked" << si << ") step_locked_stream<false>(p" << si << sfx(l) << ", p" << pj << sfx(l) << ", " << freq << ", " << w << ", sl" << si << "s" << sfx(l)
        << ", sl" << si << "p" << sfx(l) << ");\n";
      s << c.indent << "else\n" << c.indent << "{\n";
      s << c.indent << "  sl" << si << "s" << sfx(l) << " = p" << si << sfx(l) << ".next(" << freq << ");\n";
      s << c.indent << "  sl" << si << "p" << sfx(l) << " = p" << pj << sfx(l) << ".next_sw(" << freq << (pn.in.size() == 2 ? ", " + w : std::string()) << ", oddw" << pj << ");\n";
      s << c.indent << "}\n";
    }
  }
  // the nodes of region r (-1: the outer graph) in context c
  void emitNodes(int r, const Ctx& c)
  {
    std::vector<char> entered(g.regions.size(), 0);
    if (r < 0 && p.earlyRows)
    {
      for (size_t j = 0; j < g.nodes.size(); ++j)
        if (p.nodes[j].earlyHoisted) value(j, c.indent, c.sfx, c.idx);
      for (size_t dn = 0; dn < g.nodes.size(); ++dn)
        if (p.nodes[dn].earlyTop) emitPre(dn, c);
    }
    for (size_t j = 0; j < g.nodes.size(); ++j)
    {
      const Node& m = g.nodes[j];
      if (m.rate != RATE_AUDIO) continue;
      if (r < 0 && p.earlyRows && p.nodes[j].earlyHoisted) continue;  // at the top of the sample
      if (m.region != r)
      {
        // the first node of a region nested directly here: the whole region goes in at this point
        if (m.region >= 0 && (r < 0 || isInside(m.region, r)))
        {
          const int child = childUnder(m.region, r);
          if (!entered[(size_t)child])
          {
            entered[(size_t)child] = 1;
            emitRegion(child, c);
          }
        }
        continue;
      }
      if (m.role == ROLE_REGION_IN) continue;  // made by emitRegion
      if (m.role == ROLE_REGION_OUT)
      {
        const Region& R = g.regions[(size_t)m.slot];
        if (R.kind == MLGPU_REGION_DOWNSAMPLE_2X) continue;  // read before the region's block, see emitRegion
        for (int l = 0; l < VL; ++l)
          s << c.indent << "const float " << name((int)j, c.sfx, l) << " = p" << j << sfx(l) << ".down(" << name(m.in[0], c.sfx + "a", l) << ", "
            << name(m.in[0], c.sfx + "b", l) << ");" << (l == 0 && !m.name.empty() ? "  // " + m.name : std::string()) << "\n";
        continue;
      }
      if (r < 0 && p.nodes[j].streamLockSaw >= 0)
      {
        const int si = p.nodes[j].streamLockSaw;
        if ((int)j == std::min(si, p.nodes[(size_t)si].streamLockPulse)) streamLockPair(si, c);
      }
      if (r < 0 && p.nodes[j].earlySlot >= 0 && !p.nodes[j].earlyTop) emitPre(j, c);  // (a delay time made of this sample's own signal: read and value together)
      value(j, c.indent, c.sfx, c.idx);
    }
    if (r < 0) return;
    // fn's own one-vector feedback (slot = the sample index inside fn's DSPVector), then the end of fn's DSPVector
    for (size_t j = 0; j < g.nodes.size(); ++j)
      if (g.nodes[j].region == r && g.nodes[j].type == NODE_FEEDBACK && g.nodes[j].fbSource >= 0)
        for (int l = 0; l < VL; ++l)
          s << c.indent << stateRef(std::to_string(g.nodes[j].sOff) + " + " + c.idx, l) << " = f2u(" << name(g.nodes[j].fbSource, c.sfx, l) << ");\n";
    bool any = false;
    for (size_t j = 0; j < g.nodes.size(); ++j)
    {
      const Node& m = g.nodes[j];
      if (m.type != NODE_PROC || m.region != r || m.role != ROLE_NONE) continue;
      if (!any) s << c.indent << "if (" << c.idx << " == 63)\n" << c.indent << "{\n";
      any = true;
      for (int l = 0; l < VL; ++l) s << c.indent << "  p" << j << sfx(l) << ".end_vector();\n";
    }
    if (any) s << c.indent << "}\n";
  }
  // region r, entered from context c of its parent
  void emitRegion(int r, const Ctx& c)
  {
    const Region& R = g.regions[(size_t)r];
    if (R.kind == MLGPU_REGION_UPSAMPLE_2X)
    {
      // fn on the two samples the HalfBandFilters make of this sample (upsampleFirstHalf / SecondHalf in stream order)
      for (int phase = 0; phase < 2; ++phase)
      {
        const std::string ph = phase ? "b" : "a";
        const Ctx cc{c.sfx + ph, "((2 * (" + c.idx + ") + " + std::to_string(phase) + ") & 63)",
                     "(2 * (" + c.vec + ") + ((2 * (" + c.idx + ") + " + std::to_string(phase) + ") >> 6))", c.indent};
        for (int in : R.ins)
          for (int l = 0; l < VL; ++l) s << c.indent << "const float " << name(in, cc.sfx, l) << " = p" << in << sfx(l) << ".up_" << ph << "(" << regionSource(in, c, l) << ");\n";
        emitNodes(r, cc);
      }
      return;
    }
    // the region's output is what its upsampler made one DSPVector (of the parent's) ago; fn runs on the parent's odd samples
    const bool top = (R.parent < 0);
    for (int l = 0; l < VL; ++l)
      s << c.indent << "const float " << name(R.out, c.sfx, l) << " = p" << R.out << sfx(l) << (top ? ".delayed(" : ".delayedAt(") << c.idx << ");\n";
    s << c.indent << "if ((" << c.idx << ") & 1)\n" << c.indent << "{\n";
    const Ctx cc{c.sfx, "((((" + c.idx + ") - 1) >> 1) + 32 * (int)((" + c.vec + ") & 1))", "((" + c.vec + ") >> 1)", c.indent + "  "};
    for (int in : R.ins)
      for (int l = 0; l < VL; ++l) s << cc.indent << "const float " << name(in, cc.sfx, l) << " = p" << in << sfx(l) << ".down(prev" << in << sfx(l) << ", " << regionSource(in, c, l) << ");\n";
    emitNodes(r, cc);
    for (int l = 0; l < VL; ++l) s << cc.indent << "p" << R.out << sfx(l) << ".push(" << c.idx << ", " << name(R.result, cc.sfx, l) << ");\n";
    s << c.indent << "}\n";
    for (int in : R.ins)
      for (int l = 0; l < VL; ++l) s << c.indent << "prev" << in << sfx(l) << " = " << regionSource(in, c, l) << ";\n";
  }
  // one sample of every voice of the lane: the graph, the outputs' values, the feedback values kept for the next DSPVector
  void sampleBody()
  {
    emitNodes(-1, Ctx{"", "(q * 4 + k)", "(a.t0 + t)", "        "});
    for (size_t o = 0; o < g.outputs.size(); ++o)
      for (int l = 0; l < VL; ++l)
      {
        if (g.outputGroup[o] && !ldsSum(o) && !segSum(o)) s << "        y" << o << sfx(l) << "[k] = group_sum_in_order<" << g.outputGroup[o] << ">(n" << g.outputs[o] << sfx(l) << ");\n";
        else s << "        y" << o << sfx(l) << "[k] = n" << g.outputs[o] << sfx(l) << ";\n";
      }
    // feedback: keep this sample's value for the same sample of the next DSPVector (its old value was read above)
    for (size_t i = 0; i < g.nodes.size(); ++i)
      if (g.nodes[i].type == NODE_FEEDBACK && g.nodes[i].fbSource >= 0 && g.nodes[i].region < 0)
        for (int l = 0; l < VL; ++l)
          s << "        " << stateRef(std::to_string(g.nodes[i].sOff) + " + q * 4 + k", l) << " = f2u(n" << g.nodes[i].fbSource << sfx(l) << ");\n";
    s << "      }\n";
  }
  // the quad's outputs: group sums and mixdowns through LDS, every other output straight to memory
  void outputStores()
  {
    // the listed form: the running maximum of every output's |sample| bit patterns, before any mixdown (GraphArgs::peaks)
    for (size_t o = 0; listed && o < g.outputs.size(); ++o)
      s << "#pragma unroll\n      for (int kk = 0; kk < 4; ++kk)\n      {\n        const uint32_t mag = f2u(y" << o << "_0[kk]) & 0x7fffffffu;\n        pk_0 = mag > pk_0 ? mag : pk_0;\n      }\n";
    for (size_t o = 0; o < g.outputs.size(); ++o)
      if (ldsSum(o))
        s << "      group16_park(strip" << o << ", q & 3, y" << o << "_0);\n      if ((q & 3) == 3) group16_sum_store(strip" << o << ", out" << o << "_0 + t * a.out[" << o
          << "].strideT + (q - 3) * a.out[" << o << "].strideQ, a.out[" << o << "].strideQ);\n";
    for (size_t o = 0; o < g.outputs.size(); ++o)
      if (segSum(o))
        s << "      segment_park(seg" << o << ", q & 3, y" << o << "_0);\n      if ((q & 3) == 3) segment_sum_store(seg" << o << ", rank_0, length_0, longest, out" << o
          << "_0 + t * a.out[" << o << "].strideT + (q - 3) * a.out[" << o << "].strideQ, a.out[" << o << "].strideQ);\n";
    for (size_t o = 0; o < g.outputs.size(); ++o)
      if (g.outputMix[o])
        s << "      mix64_park(mstrip" << o << ", q & 3, " << (partialWaves ? "(vr_0 < " + places + ") ? y" + std::to_string(o) + "_0 : f32x4{0.f, 0.f, 0.f, 0.f}" : "y" + std::to_string(o) + "_0")
          << ");\n      if ((q & 3) == 3) mix64_sum_store(mstrip" << o << ", out" << o << "_0 + t * 64 + (q - 3) * 4);\n";
    for (size_t o = 0; o < g.outputs.size(); ++o)
      for (int l = 0; l < VL && !ldsSum(o) && !segSum(o) && !g.outputMix[o]; ++l)
        s << "      " << (g.outputGroup[o] ? "if ((threadIdx.x & " + std::to_string(g.outputGroup[o] - 1) + ") == " + std::to_string(g.outputGroup[o] - 1) + ") " : std::string())
          << "__builtin_nontemporal_store(y" << o << sfx(l) << ", out" << o << sfx(l) << " + t * a.out[" << o << "].strideT + q * a.out[" << o << "].strideQ);\n";
    s << "    }\n";
    if (oscTrips || ringTrips) s << "    }\n";
  }
  // the end of every DSPVector, then the state stored back
  void epilogue()
  {
    for (size_t i = 0; i < g.nodes.size(); ++i)
      if (g.nodes[i].type == NODE_PROC && (g.nodes[i].region < 0 || g.nodes[i].role != ROLE_NONE))
        for (int l = 0; l < VL; ++l) s << "    p" << i << sfx(l) << ".end_vector();\n";
    if (evVoice)
      for (int l = 0; l < VL; ++l) s << "    ev" << sfx(l) << ".end_vector();\n";
    s << "  }\n";
    if (evVoice)
      for (int l = 0; l < VL; ++l) s << "  ev" << sfx(l) << ".store();\n";
    for (size_t i = 0; i < g.nodes.size(); ++i)
      if (g.nodes[i].type == NODE_PROC)
        for (int l = 0; l < VL; ++l) s << "  p" << i << sfx(l) << ".store(m" << i << sfx(l) << ");\n";
    if (planned) s << "  if (a.peaks != nullptr) a.peaks[pl_0] = pk_0;\n";
    else if (listed) s << "  if (a.peaks != nullptr && vr_0 < a.listed) a.peaks[vr_0] = pk_0;  // (a spare lane has no place in the list)\n";
    s << "}\n";
  }
};

// Voices per lane and quads per trip of the sample loop. A fused voice is ONE dependent chain of VALU instructions per lane;
// two voices per lane (voice v and v + 256 of the same workgroup: loads and stores stay coalesced) interleave two chains,
// two quads per trip give the scheduler a longer window. Both also double the code and cost registers, and on this chip the
// plain form - one voice, one quad - is the fastest for every graph measured so far (config 5: 0.82 ms per launch against
// 0.95 with two voices per lane and 0.93 with two quads; a 34 KiB loop body falls off the instruction cache and runs at half
// speed). So the plain form is the default; mlgpu_graph_set_voices_per_lane forces two voices, and
// mlgpu_graph_set_autotune lets the first launches try all four forms and keep the fastest.
int graphVoicesPerLane(const GraphDesc& g)
{
  for (size_t o = 0; o < g.outputs.size(); ++o)
    if (g.outputMix[o]) return 1;
  if (g.voicesPerLane > 0)
  {
    for (const Node& n : g.nodes)
      if (n.type == NODE_FEEDBACK || (n.type == NODE_PROC && (mlgpu_proc_rings(n.kind) || mlgpu_proc_is_vector_rate(n.kind)))) return 1;
    return g.voicesPerLane;
  }
  return 1;
}
}  // namespace

int mlgraph::planGraph(const GraphDesc& g, const TestHooks& hooks, GraphPlan& p, std::string& error)
{
  auto fail = [&](int status, const std::string& what) {
    error = what;
    return status;
  };
  p = GraphPlan();
  p.nodes.resize(g.nodes.size());
  if (g.outputs.empty()) return fail(MLGPU_ERR_INVALID, "graph_compile: no outputs");
  if (g.openRegion >= 0) return fail(MLGPU_ERR_INVALID, "graph_compile: a rate region is still open (graph_end_region)");
  for (int o : g.outputs)
    if (g.nodes[(size_t)o].region >= 0) return fail(MLGPU_ERR_INVALID, "graph_compile: an output is a node inside a rate region");
  for (const Node& n : g.nodes)
    if (n.type == NODE_FEEDBACK && n.fbSource >= 0 && g.nodes[(size_t)n.fbSource].region != n.region)
      return fail(MLGPU_ERR_INVALID, "graph_compile: a feedback node and its source must be in the same rate region (or both outside)");
  for (size_t i = 0; i < g.nodes.size(); ++i)
  {
    const Node& n = g.nodes[i];
    if (n.type == NODE_FEEDBACK && n.fbSource < 0) return fail(MLGPU_ERR_INVALID, "graph_compile: feedback node '" + n.name + "' has no source (graph_set_feedback)");
    if (n.type != NODE_PROC || mlgpu_proc_rings(n.kind) == 0) continue;
    if (n.ringLen == 0) return fail(MLGPU_ERR_INVALID, "graph_compile: delay node '" + n.name + "' has no memory (graph_set_max_delay)");
    p.nodes[i].memOff = p.memFloatsPerVoice;
    p.nodes[i].ringSlot = p.totalRings;
    p.totalRings += mlgpu_proc_rings(n.kind);
    p.memFloatsPerVoice += n.ringLen * (size_t)mlgpu_proc_rings(n.kind);
  }
  p.rings = ringLayoutOfApi(g.delayLayout);
  // (three rings: layout 2 fits but leaves a CU one workgroup, and layout 1 is 9 % faster - profiles/r05_ring_layouts.txt)
  // a bank whose last wavefront is not full: its spare lanes run the last voice again (GraphEmitter) - not where voices are
  // summed in groups inside the kernel or read event records, which go by lane
  // (mlgpu_graph_enable_voice_list_events: the event rows go by voice - CtlVoice below - and a spare lane's are the last voice's)
  // (mlgpu_graph_enable_mpe_events: CtlVoiceMpe goes by voice as well - the voice's lane and its main lane are made of the voice index)
  bool groupedOrEvents = g.hasEventRows && !g.voiceListEvents && !g.mpeEvents;
  for (size_t o = 0; o < g.outputs.size(); ++o) groupedOrEvents = groupedOrEvents || g.outputGroup[o] != 0;
  const bool partialOk = g.V % 64 == 0 || !groupedOrEvents;
  if (p.rings == RingLayout::TRANSPOSED && p.totalRings && !partialOk)
    return fail(MLGPU_ERR_UNSUPPORTED, "graph_compile: delay layout 2 with voice sums or event rows inside the kernel needs whole wavefronts (voices a multiple of 64)");
  for (size_t o = 0; o < g.outputs.size(); ++o)
    if (g.outputMix[o] && !partialOk)
      return fail(MLGPU_ERR_UNSUPPORTED, "graph_compile: an output that is the mixdown of all voices, next to group sums or event rows, needs whole wavefronts (voices a multiple of 64)");
  // LDS of a workgroup: the ring strips, the impulse table and a strip per output that is summed inside the kernel (a whole-bank
  // mixdown: 4 wavefronts x kMixStrip floats = 21 KiB; a 16-voice group sum: 4 x kGroup16Strip = 20.3 KiB). A layout that does not fit
  // next to them falls back (layout 3) or is refused here with the sizes, not by hiprtc / the module loader.
  size_t ldsOther = g.hasImpulse ? 128 : 0;
  for (size_t o = 0; o < g.outputs.size(); ++o)
  {
    if (g.outputMix[o]) ldsOther += sizeof(float) * 4 * (size_t)kHostMixStripFloats;
    else if (g.outputGroup[o] == 16) ldsOther += sizeof(float) * 4 * (size_t)kHostGroup16StripFloats;
  }
  constexpr size_t kLdsBytes = 160 * 1024;
  const size_t ldsLayout2 = (size_t)p.totalRings * 4 * 40 * 64 * sizeof(float), ldsLayout1 = (size_t)p.totalRings * 8 * 256 * sizeof(float);
  size_t ldsLayout4 = 0;  // per workgroup: 2 KiB per ring and wavefront (the held sector) + 4 KiB per delay node and wavefront (its last 16 samples)
  for (const Node& n : g.nodes)
    if (n.type == NODE_PROC && mlgpu_proc_rings(n.kind)) ldsLayout4 += 4 * sizeof(float) * ((size_t)mlgpu_proc_rings(n.kind) * 512 + 1024);
  auto kib = [](size_t b) { return std::to_string((b + 1023) / 1024) + " KiB"; };
  // layout 4 (sector trips) serves delay nodes of the outer graph; one inside a rate region keeps layout 1's per-sample form
  bool ringInRegion = false;
  for (const Node& n : g.nodes) ringInRegion = ringInRegion || (n.type == NODE_PROC && n.region >= 0 && mlgpu_proc_rings(n.kind) != 0);
  if (p.rings == RingLayout::SECTORS && ringInRegion)
    return fail(MLGPU_ERR_UNSUPPORTED, "graph_compile: delay layout 4 (sector trips) does not serve a delay line inside a rate region (layout 1 or 3 for this graph)");
  // mlgpu_graph_enable_voice_list_rings: the listed kernel keeps ring windows too. The lane plan's has LDS of its own beside them -
  // the tables and the segment strips (below; its early reads are the rows' alone) - where the plain kernel has ldsOther.
  const bool listRings = g.voiceLists && g.voiceListRings;
  size_t planSums = 0;
  for (size_t o = 0; o < g.outputs.size(); ++o) planSums += g.outputGroup[o] ? 1 : 0;
  const size_t ldsPlanned = !g.voiceListGroups ? 0 : (g.hasImpulse ? 128 : 0) + planSums * sizeof(float) * (4 * (size_t)kHostSegmentStripFloats + (size_t)kHostSegmentTailFloats);
  const size_t ldsBoth = std::max(ldsOther, ldsPlanned);
  if (listRings && !p.totalRings)
    return fail(MLGPU_ERR_INVALID, "graph_compile: voice lists with rings in the sector layouts (mlgpu_graph_enable_voice_list_rings): the graph has no delay node; "
                                   "without one mlgpu_graph_enable_voice_lists serves the graph");
  if (g.delayLayout == 3)
  {
    // "the best form": one or two rings - the transposed windows (0.72-0.74 of the HBM peak on the strings bank); more - the sector
    // trips (no LDS, every ring's loads in the trip's prologue: profiles/r06_ring_layouts.txt); where neither applies, layout 1
    // (measured, profiles/r06_ring_layouts.txt: one PitchbendableDelay 0.74 of the HBM peak in layout 4 - it keeps one ring and makes
    // one read for both cores - against 0.58 in layout 2; one / two FractionalDelays 0.63 / 0.60 in layout 2 against 0.50 / 0.40;
    // three / four 0.42 / 0.35 in layout 4 against 0.33 / 0.32 in layout 2 and 0.34 / 0.20 in layout 1)
    bool anyPitchbendable = false;
    for (const Node& n : g.nodes) anyPitchbendable = anyPitchbendable || (n.type == NODE_PROC && n.kind == MLGPU_PROC_PITCHBENDABLE_DELAY);
    const bool sectorFits = !ringInRegion && p.totalRings > 0 && ldsLayout4 + ldsOther <= kLdsBytes;
    const bool preferSectors = sectorFits && (anyPitchbendable || p.totalRings > 2);
    const bool transposed = !preferSectors && partialOk && p.totalRings <= 4 && ldsLayout2 + ldsOther <= kLdsBytes;
    // more rings than any windowed form has LDS for (the reference's reverb example: 24): the default rows
    p.rings = transposed ? RingLayout::TRANSPOSED : sectorFits ? RingLayout::SECTORS : ldsLayout1 + ldsOther > kLdsBytes ? RingLayout::ROWS : RingLayout::WINDOWS;
    // Voice lists with rings (mlgpu_graph_enable_voice_list_rings): never layout 2, whose pieces are moved by a block's neighbouring
    // lanes. The sector trips where their LDS fits and no delay line sits in a rate region, else layout 1 where its LDS fits, else
    // the rows - each next to the LDS of BOTH kernels, the plan is one value for the two (measured on listed launches of a string
    // bank and of four Allpass nodes: profiles/graph_voice_list_rings.md)
    if (listRings)
      p.rings = (!ringInRegion && ldsLayout4 + ldsBoth <= kLdsBytes) ? RingLayout::SECTORS : ldsLayout1 + ldsBoth <= kLdsBytes ? RingLayout::WINDOWS : RingLayout::ROWS;
  }
  if (p.rings == RingLayout::TRANSPOSED && ldsLayout2 + ldsOther > kLdsBytes)
    return fail(MLGPU_ERR_UNSUPPORTED, "graph_compile: delay layout 2 needs 40 KiB of LDS per ring (" + kib(ldsLayout2) + " for " + std::to_string(p.totalRings) +
                                           " rings) next to " + kib(ldsOther) + " of output strips and tables; a workgroup has 160 KiB (layout 1 or 3 for this graph)");
  if (p.rings == RingLayout::SECTORS && ldsLayout4 + ldsOther > kLdsBytes)
    return fail(MLGPU_ERR_UNSUPPORTED, "graph_compile: delay layout 4 needs 8 KiB of LDS per ring and 16 KiB per delay node (" + kib(ldsLayout4) + " for this graph) next to " +
                                           kib(ldsOther) + " of output strips and tables; a workgroup has 160 KiB (layout 1 or 3 for this graph)");
  if (p.rings == RingLayout::WINDOWS && ldsLayout1 + ldsOther > kLdsBytes)
    return fail(MLGPU_ERR_UNSUPPORTED, "graph_compile: delay layouts 1 and 4 need 8 KiB of LDS per ring (" + kib(ldsLayout1) + " for " + std::to_string(p.totalRings) +
                                           " rings) next to " + kib(ldsOther) + " of output strips and tables; a workgroup has 160 KiB");
  if (ldsOther > kLdsBytes)
    return fail(MLGPU_ERR_UNSUPPORTED, "graph_compile: " + kib(ldsOther) + " of LDS for the outputs summed inside the kernel (21 KiB per mixed-down output, 20.3 KiB per 16-voice group sum); a workgroup has 160 KiB");
  // The listed form (mlgpu_graph_enable_voice_lists) gathers a wavefront's 64 voices from anywhere in the graph: what goes by lane or
  // by a block's neighbouring voices has no listed form
  if (g.voiceLists)
  {
    const std::string who = g.voiceListGroups ? "graph_compile: voice lists by a lane plan (mlgpu_graph_enable_voice_list_groups): " : "graph_compile: voice lists (mlgpu_graph_enable_voice_lists): ";
    // (mlgpu_graph_enable_voice_list_rings: layouts 1 and 4 keep a voice's 32-byte sectors to the voice - memory goes by v, the LDS
    // windows by the lane, nothing looks at a neighbour; layout 2's stage registers hold other lanes' pieces)
    if (listRings && p.rings == RingLayout::TRANSPOSED)
      return fail(MLGPU_ERR_UNSUPPORTED, who + "delay layout 2 (transposed windows) moves a voice's 64-byte pieces with its neighbouring lanes and has no listed form; "
                                             "mlgpu_graph_enable_voice_list_rings serves the sector layouts 1 and 4, and layout 3, which then resolves to one of them: "
                                             "mlgpu_graph_set_delay_layout(g, 1), (g, 4) or (g, 3)");
    if (!listRings && p.rings != RingLayout::ROWS && p.totalRings)
      return fail(MLGPU_ERR_UNSUPPORTED, who + "delay layout " + std::to_string(apiLayout(p.rings)) + (g.delayLayout == 3 ? " (what layout 3 resolves to for this graph)" : "") +
                                             " keeps its rings in pieces made by the neighbouring voices of a 256-voice block; the rows are served: mlgpu_graph_set_delay_layout(g, 0)");
    // the lane plan (mlgpu_graph_enable_voice_list_groups): instruments of ONE size, and no mixdown - the tree of a K-voice graph goes
    // by list position in whole wavefronts, a lane plan has pads
    int planGroup = 0;
    for (size_t o = 0; g.voiceListGroups && o < g.outputs.size(); ++o)
    {
      if (g.outputGroup[o] && planGroup && g.outputGroup[o] != planGroup)
        return fail(MLGPU_ERR_INVALID, who + "the outputs' group sums are of " + std::to_string(planGroup) + " and of " + std::to_string(g.outputGroup[o]) +
                                           " voices; the lane plan lays out instruments of one size");
      if (g.outputGroup[o]) planGroup = g.outputGroup[o];
    }
    if (g.voiceListGroups && !planGroup)
      return fail(MLGPU_ERR_INVALID, who + "no output has a group sum (mlgpu_graph_set_output_group_sum); without one mlgpu_graph_enable_voice_lists serves the graph");
    for (size_t o = 0; o < g.outputs.size(); ++o)
    {
      if (g.voiceListGroups && g.outputMix[o])
        return fail(MLGPU_ERR_UNSUPPORTED, who + "an output that is the mixdown of all voices (mlgpu_graph_set_output_mixdown) goes by list position in whole wavefronts, a lane plan has pads: no such form");
      if (g.outputGroup[o] && !g.voiceListGroups)
        return fail(MLGPU_ERR_UNSUPPORTED, who + "an output group sum (mlgpu_graph_set_output_group_sum) has no listed form without the lane plan: mlgpu_graph_enable_voice_list_groups(g, 1)");
      if (g.outputMixShard[o]) return fail(MLGPU_ERR_UNSUPPORTED, who + "the shard form of a mixdown (mlgpu_graph_set_output_mixdown(.., 2)) has no listed form");
    }
    if (g.hasEventRows && !g.voiceListEvents)
      return fail(MLGPU_ERR_UNSUPPORTED, who + "event rows (mlgpu_graph_add_event_row) go by lane, not by voice: no listed form (mlgpu_graph_enable_voice_list_events(g, 1) makes one)");
    for (const Region& R : g.regions)
      if (R.kind == MLGPU_REGION_DOWNSAMPLE_2X)
        return fail(MLGPU_ERR_UNSUPPORTED, who + "a DOWNSAMPLE_2X region pairs DSPVectors by the graph's count, not by a voice's: no listed form");
  }
  p.memVoices = p.rings != RingLayout::ROWS ? ((g.V + 255) & ~(size_t)255) : g.V;
  p.minWavesHook = hooks.minWaves;
  p.rowAddr64 = hooks.rowAddr64;
  p.ringByLane = listRings && p.rings == RingLayout::SECTORS && p.totalRings;
  p.ringLaneClock = p.ringByLane && hooks.ringLaneClock;
  // ... and a PitchbendableDelay among them: a wavefront of the plain kernel that cannot run trips sends ALL its lanes through two rings,
  // where the listed kernel kept one for a lane whose two write indices agree (mldsp_procs.hpp, above RingCore::beginS)
  for (const Node& n : g.nodes) p.ringsByLaneOnly = p.ringsByLaneOnly || (p.ringByLane && n.type == NODE_PROC && n.kind == MLGPU_PROC_PITCHBENDABLE_DELAY);
  // ring layout 0: rows behind 32-bit offsets where every delay node's memory stays below 4 GiB (VoiceMem::ringPtr)
  // (node by node in the generator: a ring of the bank at most 4 GiB)
  p.rowAddr32 = p.rings == RingLayout::ROWS && p.totalRings && g.V < ((size_t)1 << 22) && !p.rowAddr64;
  // ring layout 0: the outer graph's ring reads by LDS-DMA ahead of the sample's arithmetic, a 256-byte landing slot per read and wavefront
  if (p.rings == RingLayout::ROWS && p.totalRings && hooks.earlyReads)
  {
    int slots = 0;
    for (const Node& n : g.nodes)
      if (n.type == NODE_PROC && n.region < 0 && n.role == ROLE_NONE && mlgpu_proc_rings(n.kind)) slots += n.kind == MLGPU_PROC_PITCHBENDABLE_DELAY ? 2 : 1;
    // (one ring - a plucked string - has nothing to issue together: 0.127 of the peak with the early read against 0.142 without)
    if (slots >= 3 && (size_t)slots * 4 * 64 * sizeof(float) + ldsOther <= kLdsBytes)
    {
      p.earlyRows = true;
      p.earlySlots = slots;
      slots = 0;
      for (size_t i = 0; i < g.nodes.size(); ++i)
      {
        const Node& n = g.nodes[i];
        if (n.type != NODE_PROC || n.region >= 0 || n.role != ROLE_NONE || !mlgpu_proc_rings(n.kind)) continue;
        p.nodes[i].earlySlot = slots;
        slots += n.kind == MLGPU_PROC_PITCHBENDABLE_DELAY ? 2 : 1;
      }
    }
  }
  // The lane plan's listed kernel has LDS of its own - the plan is one value for both kernels, so not in ldsOther: the impulse table
  // and the early reads' landing slots as in the plain kernel, and per group-summed output the four wavefronts' segment strips and
  // the tail behind them (16 KiB + 256 B) where the plain kernel has a 16-voice group's strip or none
  if (g.voiceListGroups)
  {
    size_t sums = 0;
    for (size_t o = 0; o < g.outputs.size(); ++o) sums += g.outputGroup[o] ? 1 : 0;
    const size_t ldsTables = g.hasImpulse ? 128 : 0, ldsEarly = (size_t)p.earlySlots * 4 * 64 * sizeof(float);
    const size_t ldsSegments = sums * sizeof(float) * (4 * (size_t)kHostSegmentStripFloats + (size_t)kHostSegmentTailFloats);
    // (mlgpu_graph_enable_voice_list_rings: and the ring windows of the layout in effect, as in the plain kernel)
    const size_t ldsRingWindows = !(listRings && p.totalRings) ? 0 : p.rings == RingLayout::SECTORS ? ldsLayout4 : p.rings == RingLayout::WINDOWS ? ldsLayout1 : 0;
    if (ldsRingWindows && ldsPlanned + ldsRingWindows > kLdsBytes)  // (ldsPlanned: the tables and the segment strips)
      return fail(MLGPU_ERR_UNSUPPORTED, "graph_compile: voice lists by a lane plan (mlgpu_graph_enable_voice_list_groups) with rings in the sector layouts (mlgpu_graph_enable_voice_list_rings): " +
                                             kib(ldsRingWindows) + " of LDS for the ring windows of delay layout " + std::to_string(apiLayout(p.rings)) + " next to " + kib(ldsSegments) +
                                             " for the segment strips of " + std::to_string(sums) + " group-summed outputs (16 KiB + 256 B each) and " + std::to_string(ldsTables) +
                                             " B of tables; a workgroup has 160 KiB (layout 3 or 0 for this graph)");
    if (ldsTables + ldsEarly + ldsSegments > kLdsBytes)
      return fail(MLGPU_ERR_UNSUPPORTED, "graph_compile: voice lists by a lane plan (mlgpu_graph_enable_voice_list_groups): " + kib(ldsSegments) + " of LDS for the segment strips of " +
                                             std::to_string(sums) + " group-summed outputs (16 KiB + 256 B each) next to " + kib(ldsEarly) + " of early ring reads and " +
                                             std::to_string(ldsTables) + " B of tables; a workgroup has 160 KiB");
  }
  planStreamLocks(g, p);
  planEarlyReads(g, p);
  p.oscTripQ = hooks.oscTripQ;
  if (p.rings == RingLayout::SECTORS && p.totalRings && p.oscTripQ > 0) p.oscTripQ = 2;  // (one trip structure: the rings' trips are two quads)
  planOscTrips(g, p);
  // delay graphs wait on their ring reads: two quads per trip keep more of them in flight (allpass4: 5.4 vs 4.5 x 10^10)
  p.form = KernelForm{graphVoicesPerLane(g), (p.totalRings && p.rings == RingLayout::ROWS) ? 2 : 1, 0};
  return MLGPU_OK;
}

std::string mlgraph::generateGraphSource(const GraphDesc& d, const GraphPlan& plan, const KernelForm& form)
{
  GraphEmitter e(d, plan, form);
  e.header();
  e.sharedMemory();
  e.voiceSetup();
  e.oscillatorTests();
  e.outputsAndPrefetch();
  e.vectorHead();
  e.sampleBody();
  e.outputStores();
  e.epilogue();
  return e.s.str();
}
