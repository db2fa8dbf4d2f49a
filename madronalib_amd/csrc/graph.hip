// graph.hip — run-time defined DSP graphs ("procs") compiled to ONE fused gfx950 kernel: the C ABI, the handle and its device state.
//
// The reference's dynamic-graph layer is a stub (source/procs/MLProcMultiply.cpp: named
// inputs/outputs/params, a process() that combines mldsp.h objects, registration by name),
// so this is the engine's own executor for BASELINE configs[4]: a DAG whose nodes are the same
// processors (MLGPU_PROC_*) and stateless ops (MLGPU_OP_*) the banks use, with named nodes.
//
// description -> plan -> source (graph_codegen.hpp): the building calls write a GraphDesc, a compile makes a GraphPlan of it and the
// HIP source of the two, and jit.hip compiles that for gfx950 with hiprtc. Identical graphs share one compiled module per process.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <mutex>
#include <new>
#include <set>

#include "graph_codegen.hpp"
#include "mlgpu_internal.hpp"

using namespace mlgraph;

struct mlgpu_graph;
static std::mutex g_boundMutex;
static std::set<mlgpu_graph*> g_boundGraphs;  // graphs with an events object bound (mlgpu_graph_bind_events)

namespace
{
int opArity(int op) { return op >= 64 ? 3 : (op >= 32 ? 2 : 1); }
bool opKnown(int op)
{
  return (op >= 0 && op <= MLGPU_OP_PHASOR_TO_SINE) || (op >= MLGPU_OP_ADD && op <= MLGPU_OP_PHASOR_TO_SAW) ||
         (op >= MLGPU_OP_LERP && op <= MLGPU_OP_PHASOR_TO_PULSE);
}

// What a compile makes of a description without a device: the plan, the source of the plan's default form and its code object
// (`code` empty: hiprtc refused the source, `log` says why)
struct GraphBuild
{
  GraphPlan plan;
  std::string source, log;
  std::vector<char> code;
  // the listed form (GraphDesc::voiceLists; else empty): the second kernel of the same plan
  std::string listedSource, listedLog;
  std::vector<char> listedCode;
};
// the listed kernel's form: one voice per lane, the plan's quads per trip (autotune and voices per lane do not apply to it); by the
// lane plan where the description says so (mlgpu_graph_enable_voice_list_groups)
KernelForm listedForm(const GraphDesc& d, const GraphPlan& p)
{
  KernelForm f{1, p.form.quadsPerTrip, 0};
  f.listed = true;
  f.planned = d.voiceListGroups;
  return f;
}
}  // namespace

struct mlgpu_graph
{
  mlgpu_engine* e{nullptr};
  GraphDesc desc;                     // what the building calls wrote; every edit drops `build` (checkEditable)
  std::unique_ptr<GraphBuild> build;  // made of `desc` by the first mlgpu_graph_emit / _compile after an edit
  bool compiled{false};
  hipFunction_t fn{nullptr};
  hipFunction_t fnListed{nullptr};  // the listed form's kernel (mlgpu_graph_enable_voice_lists), loaded by the same compile
  mlgpu_voice_list list;            // mlgpu_graph_set_voice_list
  KernelForm activeForm;         // of the kernel in `fn`: the plan's default form, or the one autotune found faster
  DeviceBuffer<float> d_coeffs;
  DeviceBuffer<uint32_t> d_state;
  DeviceBuffer<float> d_params;
  DeviceBuffer<float> d_consts;  // live constants: [nConsts] floats
  DeviceBuffer<float> d_mem;
  size_t vectorCount{0};         // DSPVectors processed since the last clear (GraphArgs::t0)
  bool listedSinceClear{false};  // a listed launch has run since the last mlgpu_graph_clear (GraphPlan::ringsByLaneOnly: the plain kernel is then refused)
  std::string lastError;         // mlgpu_graph_last_error
  mlgpu_events* events{nullptr}; // mlgpu_graph_bind_events: the object the NODE_EVENT_ROW nodes read
  // mlgpu_graph_compile_async: planning, code generation and hiprtc on a thread of the library's, off the caller's (audio) thread.
  // The worker reads `desc` and writes its job only; mlgpu_graph_compile_poll installs the result on the caller's thread. While the
  // job is in flight every other call on the graph answers MLGPU_ERR_BUSY (or refuses as it would for a graph that is not compiled
  // yet) without touching it.
  struct CompileResult
  {
    std::unique_ptr<GraphBuild> build;  // (empty: the graph's own build was there already, or planning failed)
    hipFunction_t fn{nullptr}, fnListed{nullptr};
    int status{MLGPU_OK};
    std::string error;
  };
  struct CompileJob
  {
    std::thread th;
    std::atomic<bool> done{false};
    CompileResult result;
  };
  CompileJob* job{nullptr};
  bool aotDone{false};           // an engine-less graph whose ahead-of-time compile has been collected (mlgpu_graph_compile_poll keeps answering MLGPU_OK)
  // Online tuning (mlgpu_graph_set_autotune): every variant (voices per lane x quads per trip) computes the same bits from
  // the same state arrays, so the first process calls simply take turns, are timed, and the fastest one stays.
  struct Variant
  {
    int vl{1}, unroll{1};
    hipFunction_t fn{nullptr};
    bool failed{false};
    int runs{0};
    float bestMs{1e30f};
  };
  bool tuned{false};
  std::vector<Variant> variants;
  OwnedEvent tuneEv0, tuneEv1;
  int inLayoutOverride[MLGPU_GRAPH_MAX_INPUTS];  // -1: none
  mlgpu_updater updates;         // mlgpu_graph_apply_updates: the planner, the tables' description, the staging sets
  mlgpu_recorder records;        // mlgpu_graph_export_voices / _import_voices: the record layout, the staging sets
  mlgpu_graph()
  {
    for (int& x : inLayoutOverride) x = -1;
  }
};

namespace
{
int gfail(mlgpu_graph* g, int status, const std::string& what)
{
  // a graph whose compile is in flight: a call that fails on it meanwhile writes nothing and says busy
  if (g && g->job) return MLGPU_ERR_BUSY;
  if (g && g->e) g->e->lastError = what;
  if (g) g->lastError = what;  // a graph created without an engine (offline code generation) has nowhere else to keep it
  return status;
}

// The test hooks of a planning, read at every one (tests change the environment between graphs of one process)
TestHooks readTestHooks()
{
  TestHooks h;
  const char* minWaves = getenv("MLGPU_GRAPH_MIN_WAVES");
  const char* rowAddr32 = getenv("MLGPU_GRAPH_ROW_ADDR32");
  const char* earlyReads = getenv("MLGPU_GRAPH_EARLY_READS");
  const char* oscTrip = getenv("MLGPU_GRAPH_OSC_TRIP");
  const char* laneClock = getenv("MLGPU_GRAPH_RING_LANE_CLOCK");
  h.ringLaneClock = !(laneClock && !strcmp(laneClock, "0"));
  if (minWaves) h.minWaves = atoi(minWaves);
  h.rowAddr64 = rowAddr32 && !strcmp(rowAddr32, "0");
  h.earlyReads = !(earlyReads && !strcmp(earlyReads, "0"));
  if (oscTrip)
  {
    const int t = atoi(oscTrip);
    h.oscTripQ = (t == 1 || t == 2 || t == 4) ? t : 0;
  }
  return h;
}

// Source + code object of the graph kernel of `form`, with the register budget chosen: a voice bank is launched
// as whole blocks of four wavefronts, one per SIMD, and a big bank is a few blocks per CU - so a kernel that needs more than
// 128 VGPRs (three, two or one wavefront per SIMD) runs its blocks in rounds where one that fits 128 runs them all at once. If
// the bank is big enough for that to matter (65 536 voices: a block per CU) and the kernel is above 128, it is generated again
// with a bound of four wavefronts per SIMD - then three, then two - and the first build that spills moderately (up to 640 bytes
// of scratch per lane) is kept (the patch of SURVEY 8d: 170 VGPRs ->
// 128 + 156 bytes of scratch per lane, 1.82 -> 1.46 ms; the voice with its EventsToSignals rows inside: 259 -> 128 + 528 bytes,
// 3.13 -> 1.56 ms, where bounds of two and three wavefronts give 1.96 and 1.85). The test hook MLGPU_GRAPH_MIN_WAVES=0 / N
// overrides (GraphPlan::minWavesHook).
// The lane plan's listed form (KernelForm::planned) takes a bound only if it costs no scratch at all: its segment sums hold up to
// 32 registers of LDS reads next to the voice's state every fourth quad, a spill there is paid in the loop, and its launches are the
// sounding voices of a bank, not the bank (the config-5 voice, K = V / 8: 397 us at p50 bounded to four wavefronts with 168 bytes of
// scratch, 278 us unbounded - profiles/graph_voice_list_groups.md).
// So does either listed form of a graph with event rows (mlgpu_graph_enable_voice_list_events), for the second reason: its launches are
// the voices that sound.
bool generateBudgeted(const GraphDesc& d, const GraphPlan& p, KernelForm form, std::string& source, std::vector<char>& code, std::string& log)
{
  const long maxScratch = (form.planned || (form.listed && d.hasEventRows)) ? 0 : 640;
  form.minWaves = std::max(0, p.minWavesHook);
  source = generateGraphSource(d, p, form);
  if (!mlgpu_jit_code(source, code, log)) return false;
  long vgprs = 0;
  if (p.minWavesHook >= 0 || (p.rings != RingLayout::ROWS && p.totalRings) || d.V < 65536 || !mlgpu_jit_code_number(code, ".vgpr_count", vgprs) || vgprs <= 128) return true;
  // the tightest bound whose build spills moderately: four wavefronts per SIMD, else three, else two
  for (int waves = 4; waves >= 2; --waves)
  {
    if (((vgprs + 7) & ~7L) * waves <= 512) break;  // the unbounded kernel already allows that many (registers come in blocks of 8 of a SIMD's 512)
    form.minWaves = waves;
    const std::string bounded = generateGraphSource(d, p, form);
    std::vector<char> boundedCode;
    std::string boundedLog;
    long scratch = 0;
    if (mlgpu_jit_code(bounded, boundedCode, boundedLog) && mlgpu_jit_code_number(boundedCode, ".private_segment_fixed_size", scratch) && scratch <= maxScratch)
    {
      source = bounded;
      code.swap(boundedCode);
      break;
    }
  }
  return true;
}

// Every call that changes the graph's description passes here: only before mlgpu_graph_compile, never while a compile job reads the
// description, and whatever an earlier mlgpu_graph_emit / failed compile made of the old description is dropped
int checkEditable(mlgpu_graph* g, const char* whenCompiled = "graph already compiled")
{
  if (!g) return MLGPU_ERR_INVALID;
  if (g->job) return MLGPU_ERR_BUSY;
  if (g->compiled) return gfail(g, MLGPU_ERR_INVALID, whenCompiled);
  g->build.reset();
  g->aotDone = false;
  return MLGPU_OK;
}

int addNode(mlgpu_graph* g, Node&& n)
{
  if (const int st = checkEditable(g)) return -st;
  for (int id : n.in)
    if (id < 0 || id >= (int)g->desc.nodes.size()) return -gfail(g, MLGPU_ERR_RANGE, "graph node input refers to an unknown node");
  switch (n.type)
  {
    case NODE_PARAM: case NODE_CONST: n.rate = RATE_VOICE; break;
    case NODE_CONTROL: n.rate = RATE_VECTOR; break;
    case NODE_OP: case NODE_ROUTE:
      n.rate = RATE_VOICE;
      for (int id : n.in) n.rate = std::max(n.rate, g->desc.nodes[id].rate);
      break;
    default: n.rate = RATE_AUDIO; break;
  }
  // rate regions: a region's nodes are visible only inside it, and inside it only the region's own nodes and per-voice
  // floats of the outer graph are (fn sees its upsampled / downsampled arguments, nothing else moves at its rate)
  if (n.role == ROLE_NONE)
  {
    for (int id : n.in)
    {
      const Node& src = g->desc.nodes[(size_t)id];
      if (src.region >= 0 && src.region != g->desc.openRegion) return -gfail(g, MLGPU_ERR_INVALID, "graph: a node of a closed rate region is used outside it");
      if (g->desc.openRegion >= 0 && src.region < 0 && src.rate != RATE_VOICE)
        return -gfail(g, MLGPU_ERR_INVALID, "graph: inside a rate region only the region's inputs and per-voice floats (params, consts) can be used");
    }
    if (g->desc.openRegion >= 0)
    {
      const bool vectorProc = (n.type == NODE_PROC && mlgpu_proc_is_vector_rate(n.kind));
      if (n.type == NODE_INPUT || n.type == NODE_CONTROL || n.type == NODE_EVENT_ROW || vectorProc || n.rate == RATE_VECTOR)
        return -gfail(g, MLGPU_ERR_UNSUPPORTED, "graph: streamed inputs, controls and vector-rate processors cannot live inside a rate region");
      if (n.rate == RATE_AUDIO) n.region = g->desc.openRegion;
    }
  }
  g->desc.nodes.push_back(std::move(n));
  return (int)g->desc.nodes.size() - 1;
}

// a processor node with its coefficient and state slots (the checks of mlgpu_graph_add_proc are the caller's)
int addProcNode(mlgpu_graph* g, int kind, const int* inputs, int nIn, const char* name, int role = ROLE_NONE, int region = -1, int slot = 0)
{
  Node n(NODE_PROC, kind, name);
  if (nIn) n.in.assign(inputs, inputs + nIn);
  n.nc = mlgpu_proc_nc(kind);
  n.ns = mlgpu_proc_ns(kind);
  n.cOff = g->desc.NC;
  n.sOff = g->desc.NS;
  n.role = role;
  n.region = region;
  n.slot = slot;
  const int nc = n.nc, ns = n.ns;
  const int id = addNode(g, std::move(n));
  if (id >= 0)
  {
    g->desc.NC += nc;
    g->desc.NS += ns;
    if (kind == MLGPU_PROC_IMPULSE_GEN) g->desc.hasImpulse = true;
  }
  return id;
}

int checkNode(mlgpu_graph* g, int node, int type)
{
  if (!g) return MLGPU_ERR_INVALID;
  if (g->job) return MLGPU_ERR_BUSY;
  if (node < 0 || node >= (int)g->desc.nodes.size()) return gfail(g, MLGPU_ERR_RANGE, "node index out of range");
  if (g->desc.nodes[node].type != type) return gfail(g, MLGPU_ERR_INVALID, "node has the wrong type for this call");
  return MLGPU_OK;
}
// nodes that own state words: processors and feedback nodes (their stored DSPVector, 64 words)
int checkStateNode(mlgpu_graph* g, int node)
{
  if (!g) return MLGPU_ERR_INVALID;
  if (g->job) return MLGPU_ERR_BUSY;
  if (node < 0 || node >= (int)g->desc.nodes.size()) return gfail(g, MLGPU_ERR_RANGE, "node index out of range");
  if (g->desc.nodes[node].type != NODE_PROC && g->desc.nodes[node].type != NODE_FEEDBACK) return gfail(g, MLGPU_ERR_INVALID, "node has no state");
  return MLGPU_OK;
}
}  // namespace

extern "C"
{
  int mlgpu_jit_selftest(char* logOut, size_t logLen)
  {
    std::string log, all;
    bool ok = true;
    // (1) a chain that has no ahead-of-time instantiation, including the LDS-table ImpulseGen
    const int32_t chain[] = {MLGPU_PROC_IMPULSE_GEN, MLGPU_PROC_LO_SHELF, MLGPU_PROC_ADSR, MLGPU_PROC_PEAK, MLGPU_PROC_GAIN};
    ok = mlgpu_jit_compile_only(mlgpu_jit_chain_source(chain, 5, false, false), log) && ok;
    all += log;
    // (1b) the strict-SVF forms: a generic chain and a plain cascade (which keeps its stage-skewed kernel)
    const int32_t svfChain[] = {MLGPU_PROC_SAW_GEN, MLGPU_PROC_BANDPASS, MLGPU_PROC_HI_SHELF, MLGPU_PROC_GAIN};
    ok = mlgpu_jit_compile_only(mlgpu_jit_chain_source(svfChain, 4, true, false), log) && ok;
    all += log;
    const int32_t casc[] = {MLGPU_PROC_HIPASS, MLGPU_PROC_HIPASS, MLGPU_PROC_HIPASS, MLGPU_PROC_HIPASS};
    ok = mlgpu_jit_compile_only(mlgpu_jit_chain_source(casc, 4, true, false), log) && ok;
    all += log;
    // (2) a graph touching every node type
    mlgpu_graph g;
    g.desc.V = 64;
    const int gate = mlgpu_graph_add_input(&g, "gate");
    const int pitch = mlgpu_graph_add_param(&g, "pitch");
    const int two = mlgpu_graph_add_const(&g, 2.0f);
    const int f = mlgpu_graph_add_op(&g, MLGPU_OP_EXP2_APPROX, &pitch, 1, "freq");
    const int saw = mlgpu_graph_add_proc(&g, MLGPU_PROC_SAW_GEN, &f, 1, "saw");
    const int pin[2] = {f, gate};
    const int pulse = mlgpu_graph_add_proc(&g, MLGPU_PROC_PULSE_GEN, pin, 2, "pulse");
    const int noise = mlgpu_graph_add_proc(&g, MLGPU_PROC_NOISE_GEN, nullptr, 0, "noise");
    const int env = mlgpu_graph_add_proc(&g, MLGPU_PROC_ADSR, &gate, 1, "env");
    const int mixIn[2] = {saw, pulse};
    const int mix = mlgpu_graph_add_op(&g, MLGPU_OP_ADD, mixIn, 2, "mix");
    const int lerpIn[3] = {mix, noise, two};
    const int l = mlgpu_graph_add_op(&g, MLGPU_OP_LERP, lerpIn, 3, "lerp");
    const int lp = mlgpu_graph_add_proc(&g, MLGPU_PROC_LOPASS, &l, 1, "lp");
    const int vcaIn[2] = {lp, env};
    const int vca = mlgpu_graph_add_op(&g, MLGPU_OP_MULTIPLY, vcaIn, 2, "vca");
    // control-rate inputs, ramps, index generators, the other operator() forms
    const int cut = mlgpu_graph_add_control(&g, "cutoff");
    const int glide = mlgpu_graph_add_proc(&g, MLGPU_PROC_LINEAR_GLIDE, &cut, 1, "glide");
    const int interp = mlgpu_graph_add_proc(&g, MLGPU_PROC_INTERPOLATOR1, &cut, 1, "interp");
    const int sg = mlgpu_graph_add_proc(&g, MLGPU_PROC_SAMPLE_ACCURATE_LINEAR_GLIDE, &gate, 1, "sglide");
    const int lp3In[3] = {vca, glide, interp};
    const int lp3 = mlgpu_graph_add_proc(&g, MLGPU_PROC_LOPASS, lp3In, 3, "lpmod");
    const int rampIn[2] = {pitch, cut};
    const int ramp = mlgpu_graph_add_vop(&g, MLGPU_VOP_INTERPOLATE_LINEAR, rampIn, 2, "ramp");
    const int ci = mlgpu_graph_add_vop(&g, MLGPU_VOP_COLUMN_INDEX, nullptr, 0, "idx");
    const int rc = mlgpu_graph_add_vop(&g, MLGPU_VOP_RANGE_CLOSED, rampIn, 2, "rc");
    const int ro = mlgpu_graph_add_vop(&g, MLGPU_VOP_RANGE_OPEN, rampIn, 2, "ro");
    const int lsIn[6] = {lp3, ramp, ci, rc, ro, sg};
    const int ls = mlgpu_graph_add_proc(&g, MLGPU_PROC_LO_SHELF, lsIn, 6, "loshelf");
    const int hsIn[7] = {ls, ramp, ci, rc, ro, sg, two};
    const int hs = mlgpu_graph_add_proc(&g, MLGPU_PROC_HI_SHELF, hsIn, 7, "hishelf");
    // delay lines and one-vector feedback (an Allpass<PitchbendableDelay> written out)
    const int fb = mlgpu_graph_add_feedback(&g, "vy1");
    const int idIn[2] = {hs, glide};
    const int idl = mlgpu_graph_add_proc(&g, MLGPU_PROC_INTEGER_DELAY, idIn, 2, "idelay");
    const int fdIn[3] = {idl, glide, gate};
    const int fdl = mlgpu_graph_add_proc(&g, MLGPU_PROC_FRACTIONAL_DELAY, fdIn, 3, "fdelay");
    const int pbIn[2] = {fdl, glide};
    const int pbd = mlgpu_graph_add_proc(&g, MLGPU_PROC_PITCHBENDABLE_DELAY, pbIn, 2, "pbdelay");
    const int ap1 = mlgpu_graph_add_proc(&g, MLGPU_PROC_ALLPASS1, &pbd, 1, "ap1");
    const int fbmIn[2] = {ap1, fb};
    const int fbm = mlgpu_graph_add_op(&g, MLGPU_OP_ADD, fbmIn, 2, "fbsum");
    ok = (fb > 0) && (fbm > 0) && (mlgpu_graph_set_feedback(&g, fb, fbm) == MLGPU_OK) && (mlgpu_graph_set_max_delay(&g, idl, 1000.f) == MLGPU_OK) &&
         (mlgpu_graph_set_max_delay(&g, fdl, 100.f) == MLGPU_OK) && (mlgpu_graph_set_max_delay(&g, pbd, 3000.f) == MLGPU_OK) &&
         (mlgpu_graph_add_output(&g, fbm) == MLGPU_OK) && ok;
    const int muxIn[4] = {gate, hs, ls, lp3};
    const int mux = mlgpu_graph_add_route(&g, MLGPU_ROUTE_MULTIPLEX, muxIn, 4, 0, 0, "mux");
    const int muxl = mlgpu_graph_add_route(&g, MLGPU_ROUTE_MULTIPLEX_LINEAR, muxIn, 4, 0, 0, "muxl");
    const int dmIn[2] = {gate, mux};
    const int dm = mlgpu_graph_add_route(&g, MLGPU_ROUTE_DEMULTIPLEX, dmIn, 2, 1, 3, "dm1");
    const int dmlIn[2] = {gate, muxl};
    const int dml = mlgpu_graph_add_route(&g, MLGPU_ROUTE_DEMULTIPLEX_LINEAR, dmlIn, 2, 2, 3, "dml2");
    ok = (vca > 0) && (hs > 0) && (dm > 0) && (dml > 0) && (mlgpu_graph_add_output(&g, hs) == MLGPU_OK) && (mlgpu_graph_add_output(&g, dm) == MLGPU_OK) &&
         (mlgpu_graph_add_output(&g, dml) == MLGPU_OK) && ok;
    GraphPlan plan;
    std::string planError;
    ok = planGraph(g.desc, TestHooks(), plan, planError) == MLGPU_OK && ok;
    log.clear();
    ok = mlgpu_jit_compile_only(generateGraphSource(g.desc, plan, plan.form), log) && ok;
    all += planError + log;
    // (3) the same graph with per-voice rings behind LDS windows
    g.desc.delayLayout = 1;
    g.desc.voicesPerLane = 1;
    ok = planGraph(g.desc, TestHooks(), plan, planError) == MLGPU_OK && ok;
    plan.totalRings = 20;  // the largest LDS footprint graph_compile accepts (160 KiB)
    log.clear();
    ok = mlgpu_jit_compile_only(generateGraphSource(g.desc, plan, plan.form), log) && ok;
    all += planError + log;
    if (logOut && logLen) snprintf(logOut, logLen, "%s", all.c_str());
    return ok ? MLGPU_OK : MLGPU_ERR_UNSUPPORTED;
  }

  int mlgpu_graph_create(mlgpu_engine* e, size_t nVoices, mlgpu_graph** out)
  {
    if (!out) return MLGPU_ERR_INVALID;  // e == NULL: a graph for mlgpu_graph_emit only (no device)
    *out = nullptr;
    if (nVoices == 0)
    {
      if (e) e->lastError = "graph_create: zero voices";
      return MLGPU_ERR_INVALID;
    }
    mlgpu_graph* g = new (std::nothrow) mlgpu_graph();
    if (!g) return MLGPU_ERR_OOM;
    g->e = e;
    g->desc.strictSvf = e && e->strictSvf;
    g->desc.V = nVoices;
    *out = g;
    return MLGPU_OK;
  }

  int mlgpu_graph_destroy(mlgpu_graph* g)
  {
    if (!g) return MLGPU_ERR_INVALID;
    const auto forget = [](mlgpu_graph* g)
    {
      if (g->job)  // a compile in flight owns the graph: wait for it (seconds at most), then let it go
      {
        g->job->th.join();
        delete g->job;
        g->job = nullptr;
      }
      std::lock_guard<std::mutex> lock(g_boundMutex);
      g_boundGraphs.erase(g);
    };
    if (g->e) return g->e->release(g, "graph_destroy", forget);
    forget(g);  // a graph for mlgpu_graph_emit only: no device memory
    delete g;
    return MLGPU_OK;
  }

  int mlgpu_graph_add_input(mlgpu_graph* g, const char* name)
  {
    if (!g) return -MLGPU_ERR_INVALID;
    if (g->desc.nInputs >= MLGPU_GRAPH_MAX_INPUTS) return -gfail(g, MLGPU_ERR_UNSUPPORTED, "too many graph inputs");
    Node n(NODE_INPUT, 0, name);
    n.slot = g->desc.nInputs;
    const int id = addNode(g, std::move(n));
    if (id >= 0) g->desc.nInputs++;
    return id;
  }
  int mlgpu_graph_add_param(mlgpu_graph* g, const char* name)
  {
    if (!g) return -MLGPU_ERR_INVALID;
    Node n(NODE_PARAM, 0, name);
    n.slot = g->desc.nParams;
    const int id = addNode(g, std::move(n));
    if (id >= 0) g->desc.nParams++;
    return id;
  }
  int mlgpu_graph_add_control(mlgpu_graph* g, const char* name)
  {
    if (!g) return -MLGPU_ERR_INVALID;
    if (g->desc.nControls >= MLGPU_GRAPH_MAX_CONTROLS) return -gfail(g, MLGPU_ERR_UNSUPPORTED, "too many graph control inputs");
    Node n(NODE_CONTROL, 0, name);
    n.slot = g->desc.nControls;
    const int id = addNode(g, std::move(n));
    if (id >= 0) g->desc.nControls++;
    return id;
  }
  // a row of an EventsToSignals object computed inside this graph's kernel instead of read from memory (mlgpu_event_row: 0 pitch .. 6 mod)
  int mlgpu_graph_add_event_row(mlgpu_graph* g, int row, const char* name)
  {
    if (!g) return -MLGPU_ERR_INVALID;
    if (row < MLGPU_EVENT_ROW_PITCH || row > MLGPU_EVENT_ROW_MOD)
      return -gfail(g, MLGPU_ERR_UNSUPPORTED, "graph_add_event_row: rows 0 (pitch), 1 (gate), 2 (vox), 3 (z), 4 (x), 5 (y) and 6 (mod) can be source nodes");
    for (const Node& m : g->desc.nodes)
      if (m.type == NODE_EVENT_ROW && m.slot == row) return -gfail(g, MLGPU_ERR_INVALID, "graph_add_event_row: this row is a node already");
    Node n(NODE_EVENT_ROW, 0, name);
    n.slot = row;
    const int id = addNode(g, std::move(n));
    if (id >= 0)
    {
      g->desc.hasEventRows = true;
      g->desc.eventRowMask |= 1u << row;
    }
    return id;
  }
  // (file scope, see below) every graph currently bound to an events object, so that destroying the object can unbind them
  int mlgpu_graph_bind_events(mlgpu_graph* g, mlgpu_events* ev)
  {
    if (!g || !ev) return MLGPU_ERR_INVALID;
    if (g->job) return MLGPU_ERR_BUSY;
    if (!g->desc.hasEventRows) return gfail(g, MLGPU_ERR_INVALID, "graph_bind_events: the graph has no event rows (graph_add_event_row)");
    if (mlgpu_events_engine(ev) != g->e) return gfail(g, MLGPU_ERR_INVALID, "graph_bind_events: the events object belongs to another engine");
    if (!g->desc.mpeEvents && !mlgpu_events_is_midi(ev)) return gfail(g, MLGPU_ERR_UNSUPPORTED, "graph_bind_events: MIDI protocol only (one lane per voice)");
    if (mlgpu_events_num_voices(ev) != g->desc.V) return gfail(g, MLGPU_ERR_INVALID, "graph_bind_events: instruments x polyphony must equal the graph's voices");
    {
      std::lock_guard<std::mutex> lock(g_boundMutex);  // (mlgpu_graph_forget_events reads and clears g->events under the same lock)
      g_boundGraphs.insert(g);
      g->events = ev;
    }
    return MLGPU_OK;
  }
  int mlgpu_graph_add_vop(mlgpu_graph* g, int vop, const int* inputs, int nIn, const char* name)
  {
    if (!g) return -MLGPU_ERR_INVALID;
    if (vop < MLGPU_VOP_COLUMN_INDEX || vop > MLGPU_VOP_INTERPOLATE_LINEAR) return -gfail(g, MLGPU_ERR_INVALID, "graph_add_vop: unknown generator");
    const int want = (vop == MLGPU_VOP_COLUMN_INDEX) ? 0 : 2;
    if (nIn != want || (nIn > 0 && !inputs)) return -gfail(g, MLGPU_ERR_INVALID, "graph_add_vop: wrong number of inputs");
    for (int j = 0; j < nIn; ++j)
      if (inputs[j] < 0 || inputs[j] >= (int)g->desc.nodes.size() || g->desc.nodes[inputs[j]].rate > RATE_VECTOR)
        return -gfail(g, MLGPU_ERR_INVALID, "graph_add_vop: start / end are floats (a control, param or const node)");
    Node n(NODE_VOP, vop, name);
    if (nIn) n.in.assign(inputs, inputs + nIn);
    return addNode(g, std::move(n));
  }
  int mlgpu_graph_add_const_vector(mlgpu_graph* g, const float* values, const char* name)
  {
    if (!g) return -MLGPU_ERR_INVALID;
    if (!values) return -gfail(g, MLGPU_ERR_INVALID, "graph_add_const_vector: 64 floats");
    Node n(NODE_VOP, MLGPU_VOP_TABLE, name);
    n.table.resize(MLGPU_FLOATS_PER_DSPVECTOR);
    memcpy(n.table.data(), values, sizeof(float) * MLGPU_FLOATS_PER_DSPVECTOR);
    return addNode(g, std::move(n));
  }
  int mlgpu_graph_add_feedback(mlgpu_graph* g, const char* name)
  {
    if (!g) return -MLGPU_ERR_INVALID;
    Node n(NODE_FEEDBACK, 0, name);
    n.ns = MLGPU_FLOATS_PER_DSPVECTOR;
    n.sOff = g->desc.NS;
    const int id = addNode(g, std::move(n));
    if (id >= 0) g->desc.NS += MLGPU_FLOATS_PER_DSPVECTOR;
    return id;
  }
  int mlgpu_graph_set_feedback(mlgpu_graph* g, int fbNode, int valueNode)
  {
    int st = checkNode(g, fbNode, NODE_FEEDBACK);
    if (!st) st = checkEditable(g);
    if (st) return st;
    if (valueNode < 0 || valueNode >= (int)g->desc.nodes.size()) return gfail(g, MLGPU_ERR_RANGE, "graph_set_feedback: unknown value node");
    g->desc.nodes[fbNode].fbSource = valueNode;
    return MLGPU_OK;
  }
  int mlgpu_graph_set_max_delay(mlgpu_graph* g, int node, float maxDelayInSamples)
  {
    int st = checkNode(g, node, NODE_PROC);
    if (!st) st = checkEditable(g);
    if (st) return st;
    if (mlgpu_proc_rings(g->desc.nodes[node].kind) == 0) return gfail(g, MLGPU_ERR_INVALID, "graph_set_max_delay: not a delay node");
    if (!(maxDelayInSamples >= 0.f) || maxDelayInSamples > 16777216.f) return gfail(g, MLGPU_ERR_RANGE, "graph_set_max_delay: 0 .. 2^24 samples");
    // IntegerDelay::setMaxDelayInSamples, MLDSPFilters.h:823-831
    const int dMax = (int)floorf(maxDelayInSamples);
    int bits = 0;
    while ((1 << bits) < dMax + MLGPU_FLOATS_PER_DSPVECTOR) bits++;
    g->desc.nodes[node].ringLen = (size_t)1 << bits;
    return MLGPU_OK;
  }
  int mlgpu_graph_add_route(mlgpu_graph* g, int route, const int* inputs, int nIn, int index, int nOutputs, const char* name)
  {
    if (!g) return -MLGPU_ERR_INVALID;
    if (route < MLGPU_ROUTE_MULTIPLEX || route > MLGPU_ROUTE_DEMULTIPLEX_LINEAR || !inputs) return -gfail(g, MLGPU_ERR_INVALID, "graph_add_route: unknown routing node");
    const bool mux = (route == MLGPU_ROUTE_MULTIPLEX || route == MLGPU_ROUTE_MULTIPLEX_LINEAR);
    if (mux && (nIn < 2 || nIn > 1 + MLGPU_ROUTE_MAX_SIGNALS)) return -gfail(g, MLGPU_ERR_INVALID, "graph_add_route: multiplex takes a selector and 1..8 signals");
    if (!mux && (nIn != 2 || nOutputs < 1 || nOutputs > MLGPU_ROUTE_MAX_SIGNALS || index < 0 || index >= nOutputs))
      return -gfail(g, MLGPU_ERR_INVALID, "graph_add_route: demultiplex takes (selector, signal), 1..8 outputs, 0 <= index < n_outputs");
    Node n(NODE_ROUTE, route, name);
    n.in.assign(inputs, inputs + nIn);
    n.slot = index;
    n.nOut = nOutputs;
    return addNode(g, std::move(n));
  }
  int mlgpu_graph_add_const(mlgpu_graph* g, float value)
  {
    if (!g) return -MLGPU_ERR_INVALID;
    Node n(NODE_CONST, 0, nullptr);
    n.value = value;
    n.slot = g->desc.nConsts;
    const int id = addNode(g, std::move(n));
    if (id >= 0) g->desc.nConsts++;
    return id;
  }
  int mlgpu_graph_add_proc(mlgpu_graph* g, int kind, const int* inputs, int nIn, const char* name)
  {
    if (!g) return -MLGPU_ERR_INVALID;
    const int nc = mlgpu_proc_nc(kind), ns = mlgpu_proc_ns(kind);
    if (nc < 0) return -gfail(g, MLGPU_ERR_INVALID, "graph_add_proc: unknown processor kind");
    if (kind == MLGPU_PROC_HALF_BAND || kind == MLGPU_PROC_HALF_BAND_BUFFERED)
      return -gfail(g, MLGPU_ERR_INVALID, "graph_add_proc: HalfBandFilter nodes are made by graph_begin_region / graph_end_region");
    // forms of operator(): 1 input, plus PulseGen(freq, width) MLDSPGens.h:390, Lopass(x, omega, k) MLDSPFilters.h:136,
    // LoShelf(x, 5 coefficient signals) :304, HiShelf(x, 6 coefficient signals) :385; NoiseGen has none
    bool okArity = (nIn == 1);
    if (kind == MLGPU_PROC_NOISE_GEN) okArity = (nIn == 0 || nIn == 1);
    if (kind == MLGPU_PROC_PULSE_GEN) okArity = (nIn == 1 || nIn == 2);
    if (kind == MLGPU_PROC_LOPASS) okArity = (nIn == 1 || nIn == 3);
    if (kind == MLGPU_PROC_LO_SHELF) okArity = (nIn == 1 || nIn == 6);
    if (kind == MLGPU_PROC_HI_SHELF) okArity = (nIn == 1 || nIn == 7);
    if (kind == MLGPU_PROC_INTEGER_DELAY) okArity = (nIn == 1 || nIn == 2);     // (x), (x, delay) MLDSPFilters.h:834,877
    if (kind == MLGPU_PROC_FRACTIONAL_DELAY) okArity = (nIn >= 1 && nIn <= 3);  // (x), (x, delay), (x, delay, ticks) :1013-1043
    if (kind == MLGPU_PROC_PITCHBENDABLE_DELAY) okArity = (nIn == 2);           // (x, delay) :1098
    if (kind == MLGPU_PROC_TEMPO_LOCK) okArity = (nIn == 3);                    // (x, dydx, isr) :1492
    if (!okArity || (nIn > 0 && !inputs)) return -gfail(g, MLGPU_ERR_INVALID, "graph_add_proc: wrong number of inputs");
    if (kind == MLGPU_PROC_TEMPO_LOCK)
    {
      for (int j = 0; j < 3; ++j)
        if (inputs[j] < 0 || inputs[j] >= (int)g->desc.nodes.size()) return -gfail(g, MLGPU_ERR_RANGE, "graph node input refers to an unknown node");
      if (g->desc.nodes[inputs[1]].rate > RATE_VECTOR || g->desc.nodes[inputs[2]].rate > RATE_VECTOR)
        return -gfail(g, MLGPU_ERR_INVALID, "graph_add_proc: TempoLock(x, dydx, isr): dydx and isr are floats per vector");
    }
    else if (mlgpu_proc_is_vector_rate(kind) && (inputs[0] < 0 || inputs[0] >= (int)g->desc.nodes.size() || g->desc.nodes[inputs[0]].rate > RATE_VECTOR))
      return -gfail(g, MLGPU_ERR_INVALID, "graph_add_proc: Interpolator1 / LinearGlide take one float per DSPVector (a control, param or const node)");
    (void)ns;
    return addProcNode(g, kind, inputs, nIn, name);
  }

  int mlgpu_graph_begin_region(mlgpu_graph* g, int region, const int* inputs, int nIn, int* regionInputs)
  {
    if (const int st = checkEditable(g)) return st;
    if (region != MLGPU_REGION_UPSAMPLE_2X && region != MLGPU_REGION_DOWNSAMPLE_2X) return gfail(g, MLGPU_ERR_INVALID, "graph_begin_region: unknown region kind");
    if (nIn < 0 || nIn > 8 || (nIn > 0 && (!inputs || !regionInputs))) return gfail(g, MLGPU_ERR_INVALID, "graph_begin_region: 0..8 inputs");
    int depth = 0;
    for (int r = g->desc.openRegion; r >= 0; r = g->desc.regions[(size_t)r].parent) depth++;
    if (depth >= 3) return gfail(g, MLGPU_ERR_UNSUPPORTED, "graph_begin_region: rate regions nest three deep at most");
    for (int j = 0; j < nIn; ++j)
    {
      if (inputs[j] < 0 || inputs[j] >= (int)g->desc.nodes.size()) return gfail(g, MLGPU_ERR_RANGE, "graph_begin_region: unknown input node");
      const Node& src = g->desc.nodes[(size_t)inputs[j]];
      // the inputs of a nested region are signals of the enclosing one (or per-voice floats)
      if (src.region != g->desc.openRegion && !(src.region < 0 && src.rate == RATE_VOICE))
        return gfail(g, MLGPU_ERR_INVALID, "graph_begin_region: an input must be a node of the enclosing region (or of the outer graph for an outermost region)");
    }
    const int r = (int)g->desc.regions.size();
    g->desc.regions.emplace_back();
    g->desc.regions.back().kind = region;
    g->desc.regions.back().parent = g->desc.openRegion;
    for (int j = 0; j < nIn; ++j)
    {
      // one HalfBandFilter per input row: mUppers[j] (MLDSPFunctional.h:125-130) / mDowners[j] (:181-184)
      const int id = addProcNode(g, MLGPU_PROC_HALF_BAND, &inputs[j], 1, nullptr, ROLE_REGION_IN, r);
      if (id < 0) return -id;  // (cannot happen after the checks above; the region then simply stays without a result)
      g->desc.nodes[(size_t)id].rate = RATE_AUDIO;
      g->desc.regions[(size_t)r].ins.push_back(id);
      regionInputs[j] = id;
    }
    g->desc.openRegion = r;
    return MLGPU_OK;
  }

  int mlgpu_graph_end_region(mlgpu_graph* g, int result, const char* name)
  {
    if (const int st = checkEditable(g)) return -st;
    const int r = g->desc.openRegion;
    if (r < 0) return -gfail(g, MLGPU_ERR_INVALID, "graph_end_region: no region is open");
    if (result < 0 || result >= (int)g->desc.nodes.size() || g->desc.nodes[(size_t)result].region != r)
      return -gfail(g, MLGPU_ERR_INVALID, "graph_end_region: the result must be an audio-rate node of the region");
    const int parent = g->desc.regions[(size_t)r].parent;
    g->desc.openRegion = parent;
    g->desc.regions[(size_t)r].result = result;
    // mDowners[0] (MLDSPFunctional.h:137-141) resp. mUppers[0] + mOutputBuffer (:191-197); the node belongs to the enclosing region
    const int kind = (g->desc.regions[(size_t)r].kind == MLGPU_REGION_UPSAMPLE_2X) ? MLGPU_PROC_HALF_BAND : MLGPU_PROC_HALF_BAND_BUFFERED;
    const int id = addProcNode(g, kind, &result, 1, name, ROLE_REGION_OUT, parent, r);
    if (id < 0)
    {
      g->desc.openRegion = r;
      return id;
    }
    g->desc.regions[(size_t)r].out = id;
    return id;
  }
  int mlgpu_graph_add_op(mlgpu_graph* g, int op, const int* inputs, int nIn, const char* name)
  {
    if (!g) return -MLGPU_ERR_INVALID;
    if (!opKnown(op)) return -gfail(g, MLGPU_ERR_INVALID, "graph_add_op: unknown op");
    if (nIn != opArity(op) || !inputs) return -gfail(g, MLGPU_ERR_INVALID, "graph_add_op: wrong number of inputs");
    Node n(NODE_OP, op, name);
    n.in.assign(inputs, inputs + nIn);
    return addNode(g, std::move(n));
  }
  int mlgpu_graph_add_output(mlgpu_graph* g, int node)
  {
    if (const int st = checkEditable(g)) return st;
    if (node < 0 || node >= (int)g->desc.nodes.size()) return gfail(g, MLGPU_ERR_RANGE, "graph_add_output: unknown node");
    if (g->desc.outputs.size() >= MLGPU_GRAPH_MAX_OUTPUTS) return gfail(g, MLGPU_ERR_UNSUPPORTED, "too many graph outputs");
    g->desc.outputs.push_back(node);
    return MLGPU_OK;
  }
  // Synth::processVector's voice sum (source/app/MLSynth.h:43-57) as an output mode: output `index` becomes a signal of
  // voices / group channels, channel c = ((0 + voice[c * group]) + voice[c * group + 1]) + ... in that order
  int mlgpu_graph_set_output_group_sum(mlgpu_graph* g, int index, int group)
  {
    if (const int st = checkEditable(g)) return st;
    if (index < 0 || index >= (int)g->desc.outputs.size()) return gfail(g, MLGPU_ERR_RANGE, "graph_set_output_group_sum: no such output");
    if (group != 0 && group != 2 && group != 4 && group != 8 && group != 16)
      return gfail(g, MLGPU_ERR_UNSUPPORTED, "graph_set_output_group_sum: groups of 2, 4, 8 or 16 voices (other sizes: mlgpu_mixdown_groups)");
    if (group && g->desc.V % (size_t)group) return gfail(g, MLGPU_ERR_INVALID, "graph_set_output_group_sum: the voices are not a whole number of groups");
    if (group && g->desc.outputMix[index]) return gfail(g, MLGPU_ERR_INVALID, "graph_set_output_group_sum: the output is a mixdown already");
    g->desc.outputGroup[index] = group;
    return MLGPU_OK;
  }
  // Output `index` becomes ONE channel: the mixdown of all voices (mlgpu_mixdown's order and bits, its first stage inside the voice
  // kernel - the voices' signal of that output is never written). graph_process then wants 64 * n_vectors floats for it, whatever
  // the output layout, and scratch reserved with mlgpu_mixdown_reserve(engine, voices x mixed outputs, vectors).
  int mlgpu_graph_set_output_mixdown(mlgpu_graph* g, int index, int on)
  {
    if (const int st = checkEditable(g)) return st;
    if (index < 0 || index >= (int)g->desc.outputs.size()) return gfail(g, MLGPU_ERR_RANGE, "graph_set_output_mixdown: no such output");
    if (on && g->desc.outputGroup[index]) return gfail(g, MLGPU_ERR_INVALID, "graph_set_output_mixdown: the output is a group sum already");
    if (on == 2 && mlmix::shardLevel(g->desc.V) == 0)
      return gfail(g, MLGPU_ERR_INVALID, "graph_set_output_mixdown: the shard form needs a voice count that is a multiple of 64 (whole first-stage groups of the tree)");
    g->desc.outputMix[index] = on != 0;
    g->desc.outputMixShard[index] = on == 2;
    return MLGPU_OK;
  }
  static size_t mixedOutputs(const mlgpu_graph* g)
  {
    size_t n = 0;
    for (size_t o = 0; o < g->desc.outputs.size(); ++o) n += g->desc.outputMix[o] ? 1 : 0;
    return n;
  }
  // setup: the engine's mixdown scratch for this graph's mixed-down outputs - a region of the voices' tree each (mixdown_tree.hpp) -
  // for launches of up to maxVectors DSPVectors
  int mlgpu_graph_reserve_mixdown(mlgpu_graph* g, size_t maxVectors)
  {
    if (!g) return MLGPU_ERR_INVALID;
    if (!g->e) return gfail(g, MLGPU_ERR_INVALID, "graph_reserve_mixdown: a graph without an engine");
    const int st = mlgpu_mixdown_reserve_floats(g->e, mixedOutputs(g) * mlmix::regionFloats(g->desc.V, maxVectors));
    return st == MLGPU_OK ? st : gfail(g, st, "graph_reserve_mixdown: see the engine's last error");
  }
  int mlgpu_graph_node(mlgpu_graph* g, const char* name)
  {
    if (!g || !name) return -MLGPU_ERR_INVALID;
    if (g->job) return -MLGPU_ERR_BUSY;  // (the worker reads the names; and a name may be set below by this thread only)
    for (size_t i = 0; i < g->desc.nodes.size(); ++i)
      if (g->desc.nodes[i].name == name) return (int)i;
    return -MLGPU_ERR_RANGE;
  }
  int mlgpu_graph_num_nodes(mlgpu_graph* g) { return g ? (int)g->desc.nodes.size() : -1; }
  int mlgpu_graph_set_node_name(mlgpu_graph* g, int node, const char* name)
  {
    if (g && g->job) return MLGPU_ERR_BUSY;
    if (!g || !name || node < 0 || node >= (int)g->desc.nodes.size()) return MLGPU_ERR_RANGE;
    if (!g->compiled) checkEditable(g);  // (code generation prints the names into the source's comments)
    g->desc.nodes[(size_t)node].name = name;
    return MLGPU_OK;
  }
  int mlgpu_graph_node_kind(mlgpu_graph* g, int node)
  {
    if (!g || node < 0 || node >= (int)g->desc.nodes.size()) return -MLGPU_ERR_RANGE;
    const Node& n = g->desc.nodes[(size_t)node];
    return (n.type == NODE_PROC || n.type == NODE_OP || n.type == NODE_VOP) ? n.kind : -MLGPU_ERR_INVALID;
  }
  int mlgpu_graph_node_use_count(mlgpu_graph* g, int node)
  {
    if (!g || node < 0 || node >= (int)g->desc.nodes.size()) return -MLGPU_ERR_RANGE;
    int n = 0;
    for (const Node& m : g->desc.nodes)
    {
      for (int id : m.in) n += (id == node);
      n += (m.type == NODE_FEEDBACK && m.fbSource == node);
    }
    for (int o : g->desc.outputs) n += (o == node);
    return n;
  }

  // (while a compile is in flight the strings are not handed out: "" until mlgpu_graph_compile_poll has collected the job)
  const char* mlgpu_graph_last_error(mlgpu_graph* g) { return (g && !g->job) ? g->lastError.c_str() : ""; }

  // What a compile does without a device, into `r`: the plan, the source of its default form and the code object
  static void planAndGenerate(const GraphDesc& d, mlgpu_graph::CompileResult& r)
  {
    r.build.reset(new GraphBuild());
    GraphBuild& b = *r.build;
    r.status = planGraph(d, readTestHooks(), b.plan, r.error);
    if (r.status != MLGPU_OK) return r.build.reset();
    if (!generateBudgeted(d, b.plan, b.plan.form, b.source, b.code, b.log))
    {
      r.status = MLGPU_ERR_UNSUPPORTED;  // (the build stays, for mlgpu_graph_source)
      r.error = "graph_compile (hiprtc): " + b.log;
      return;
    }
    if (!d.voiceLists || generateBudgeted(d, b.plan, listedForm(d, b.plan), b.listedSource, b.listedCode, b.listedLog)) return;
    r.status = MLGPU_ERR_UNSUPPORTED;
    r.error = "graph_compile (hiprtc, the listed form): " + b.listedLog;
  }
  // Everything a compile does that needs no stream: that (unless the graph has it since an mlgpu_graph_emit), then the module on the
  // engine's device. Reads the graph, writes `r`: a compile job runs it on its thread.
  static void compileBuild(const mlgpu_graph* g, mlgpu_graph::CompileResult& r)
  {
    const auto fail = [&r](int status, const std::string& what) { r.status = status, r.error = what; };
    if (!g->build) planAndGenerate(g->desc, r);
    if (r.status != MLGPU_OK) return;
    const mlgpu_engine* e = g->e;
    if (!e) return;  // ahead of time: the code is in the memory and disk caches now (mlgpu_graph_compile_async on a graph without an engine)
    if (hipSetDevice(e->device) != hipSuccess) return fail(MLGPU_ERR_HIP, "hipSetDevice");
    bool loaded = false;
    std::string log;
    r.fn = mlgpu_jit_function(e->device, (g->build ? g->build : r.build)->source, "mlgpu_graph_kernel", log, &loaded);
    if (!loaded) return fail(MLGPU_ERR_UNSUPPORTED, "graph_compile (hiprtc): " + log);
    if (!r.fn) return fail(MLGPU_ERR_HIP, log);
    if (!g->desc.voiceLists) return;
    loaded = false;
    r.fnListed = mlgpu_jit_function(e->device, (g->build ? g->build : r.build)->listedSource, "mlgpu_graph_listed_kernel", log, &loaded);
    if (!loaded) return fail(MLGPU_ERR_UNSUPPORTED, "graph_compile (hiprtc, the listed form): " + log);
    if (!r.fnListed) return fail(MLGPU_ERR_HIP, log);
  }
  // ... and its result taken over by the graph, on the caller's thread
  static int compileInstall(mlgpu_graph* g, mlgpu_graph::CompileResult& r)
  {
    if (r.build) g->build = std::move(r.build);
    g->fn = r.fn;
    g->fnListed = r.fnListed;
    return r.status == MLGPU_OK ? MLGPU_OK : gfail(g, r.status, r.error);
  }
  static int compileFinish(mlgpu_graph* g);

  int mlgpu_graph_emit(mlgpu_graph* g, const void** code, size_t* codeSize)
  {
    if (!g) return MLGPU_ERR_INVALID;
    if (g->job) return MLGPU_ERR_BUSY;
    if (!g->build)
    {
      mlgpu_graph::CompileResult r;
      planAndGenerate(g->desc, r);
      if (const int st = compileInstall(g, r)) return st;
    }
    if (g->build->code.empty()) return gfail(g, MLGPU_ERR_UNSUPPORTED, "graph_emit (hiprtc): " + g->build->log);
    if (code) *code = g->build->code.data();
    if (codeSize) *codeSize = g->build->code.size();
    return MLGPU_OK;
  }

  const char* mlgpu_graph_listed_source(mlgpu_graph* g) { return (g && !g->job && g->build) ? g->build->listedSource.c_str() : ""; }
  int mlgpu_graph_emit_listed(mlgpu_graph* g, const void** code, size_t* codeSize)
  {
    if (!g) return MLGPU_ERR_INVALID;
    if (g->job) return MLGPU_ERR_BUSY;
    if (!g->desc.voiceLists) return gfail(g, MLGPU_ERR_INVALID, "graph_emit_listed: the graph has no listed form (mlgpu_graph_enable_voice_lists before compile / emit)");
    if (const int st = mlgpu_graph_emit(g, nullptr, nullptr)) return st;
    if (g->build->listedCode.empty()) return gfail(g, MLGPU_ERR_UNSUPPORTED, "graph_emit_listed (hiprtc): " + g->build->listedLog);
    if (code) *code = g->build->listedCode.data();
    if (codeSize) *codeSize = g->build->listedCode.size();
    return MLGPU_OK;
  }

  int mlgpu_graph_compile(mlgpu_graph* g)
  {
    if (!g) return MLGPU_ERR_INVALID;
    if (g->job) return MLGPU_ERR_BUSY;  // (not gfail: the graph is the job's until mlgpu_graph_compile_poll has collected it)
    if (g->compiled) return MLGPU_OK;
    if (!g->e) return gfail(g, MLGPU_ERR_INVALID, "graph_compile: the graph was created without an engine (graph_emit only)");
    mlgpu_graph::CompileResult r;
    compileBuild(g, r);
    if (const int st = compileInstall(g, r)) return st;
    return compileFinish(g);
  }

  int mlgpu_graph_compile_async(mlgpu_graph* g)
  {
    if (!g) return MLGPU_ERR_INVALID;
    if (g->job) return MLGPU_ERR_BUSY;
    if (g->compiled || g->aotDone) return MLGPU_OK;
    mlgpu_graph::CompileJob* job = new (std::nothrow) mlgpu_graph::CompileJob();
    if (!job) return MLGPU_ERR_OOM;
    g->job = job;
    try
    {
      job->th = std::thread([g, job]() {
        compileBuild(g, job->result);
        job->done.store(true, std::memory_order_release);
      });
    }
    catch (...)
    {
      g->job = nullptr;
      delete job;
      return gfail(g, MLGPU_ERR_OOM, "graph_compile_async: could not start a thread");
    }
    return MLGPU_OK;
  }

  int mlgpu_graph_compile_poll(mlgpu_graph* g)
  {
    if (!g) return MLGPU_ERR_INVALID;
    if (!g->job) return (g->compiled || g->aotDone) ? MLGPU_OK : gfail(g, MLGPU_ERR_INVALID, "graph_compile_poll: no compile in flight (mlgpu_graph_compile_async)");
    if (!g->job->done.load(std::memory_order_acquire)) return MLGPU_ERR_BUSY;
    mlgpu_graph::CompileJob* job = g->job;
    job->th.join();
    g->job = nullptr;
    const int st = compileInstall(g, job->result);
    delete job;
    if (st != MLGPU_OK) return st;
    if (!g->e)
    {
      g->aotDone = true;  // ahead of time: nothing to allocate, the graph stays a description (and every later poll says OK)
      return MLGPU_OK;
    }
    return compileFinish(g);     // allocations and the initial fills, on the caller's thread and stream: microseconds
  }

  static int compileFinish(mlgpu_graph* g)
  {
    mlgpu_engine* e = g->e;
    if (hipSetDevice(e->device) != hipSuccess) return gfail(g, MLGPU_ERR_HIP, "hipSetDevice");
    const GraphPlan& plan = g->build->plan;
    g->activeForm = plan.form;
    if (g->desc.autotune)
    {
      // candidates: 1 or 2 voices per lane (where the graph allows two and the caller did not force one), 1 or 2 quads per trip
      const bool twoOk = g->desc.voicesPerLane == 0 && [&] {
        for (size_t o = 0; o < g->desc.outputs.size(); ++o)
          if (g->desc.outputMix[o]) return false;
        for (const Node& n : g->desc.nodes)
          if (n.type == NODE_FEEDBACK || n.type == NODE_EVENT_ROW || (n.type == NODE_PROC && (mlgpu_proc_rings(n.kind) || mlgpu_proc_is_vector_rate(n.kind)))) return false;
        return true;
      }();
      const bool unrollFree = !(plan.rings != RingLayout::ROWS && plan.totalRings);
      for (int vl = 1; vl <= (twoOk ? 2 : 1); ++vl)
        for (int u = 1; u <= (unrollFree ? 2 : 1); ++u)
        {
          mlgpu_graph::Variant v;
          v.vl = g->desc.voicesPerLane > 0 ? g->desc.voicesPerLane : vl;
          v.unroll = u;
          if (v.vl == plan.form.voicesPerLane && u == plan.form.quadsPerTrip) v.fn = g->fn;  // the default variant is already built
          g->variants.push_back(v);
        }
      g->tuned = g->variants.size() < 2;
    }
    const size_t V = g->desc.V;
    hipError_t err = allocate(g->d_coeffs, V * (size_t)(g->desc.NC + 1));
    if (err == hipSuccess) err = allocate(g->d_state, V * (size_t)(g->desc.NS + 1));
    if (err == hipSuccess) err = allocate(g->d_params, V * (size_t)(g->desc.nParams + 1));
    const size_t memV = plan.memVoices;
    if (err == hipSuccess && plan.memFloatsPerVoice) err = allocate(g->d_mem, memV * plan.memFloatsPerVoice);
    if (err == hipSuccess && plan.memFloatsPerVoice) err = hipMemsetAsync(g->d_mem.get(), 0, sizeof(float) * memV * plan.memFloatsPerVoice, e->stream());
    if (err == hipSuccess) err = hipMemsetAsync(g->d_state.get(), 0, sizeof(uint32_t) * V * (size_t)(g->desc.NS + 1), e->stream());
    if (err == hipSuccess) err = hipMemsetAsync(g->d_coeffs.get(), 0, sizeof(float) * V * (size_t)(g->desc.NC + 1), e->stream());
    if (err == hipSuccess) err = hipMemsetAsync(g->d_params.get(), 0, sizeof(float) * V * (size_t)(g->desc.nParams + 1), e->stream());
    if (err == hipSuccess && g->desc.liveConsts)
    {
      err = allocate(g->d_consts, (size_t)(g->desc.nConsts + 1));
      for (const Node& n : g->desc.nodes)
        if (n.type == NODE_CONST && err == hipSuccess)
        {
          uint32_t u;
          memcpy(&u, &n.value, 4);
          err = mlgpu_launch_fill32((uint32_t*)g->d_consts.get() + n.slot, u, 1, e->stream());
        }
    }
    for (const Node& n : g->desc.nodes)
    {
      if (n.type != NODE_PROC) continue;
      float dc[MLGPU_MAX_PROC_COEFFS];
      mlgpu_proc_default_coeffs(n.kind, dc);
      for (int i = 0; i < n.nc && err == hipSuccess; ++i)
      {
        uint32_t u;
        memcpy(&u, &dc[i], 4);
        if (u) err = mlgpu_launch_fill32((uint32_t*)g->d_coeffs.get() + (size_t)(n.cOff + i) * V, u, V, e->stream());
      }
      uint32_t words[MLGPU_MAX_PROC_STATE];
      mlgpu_proc_clear_state(n.kind, words, false);
      for (int i = 0; i < n.ns && err == hipSuccess; ++i)
        err = mlgpu_launch_fill32(g->d_state.get() + (size_t)(n.sOff + i) * V, words[i], V, e->stream());
    }
    if (err != hipSuccess) return gfail(g, err == hipErrorOutOfMemory ? MLGPU_ERR_OOM : MLGPU_ERR_HIP, std::string("graph_compile: ") + hipGetErrorString(err));
    g->compiled = true;
    return MLGPU_OK;
  }

  // Online tuning over those candidates: launches big enough to time take turns through the variants, 3 runs each with the first
  // one discarded. The variant this launch tries, built here before its first run - or null: too small to time, or the tuning is settled.
  static mlgpu_graph::Variant* tuningTrial(mlgpu_graph* g, size_t T)
  {
    if (!g->desc.autotune || g->tuned || g->desc.V * T * MLGPU_FLOATS_PER_DSPVECTOR < ((size_t)1 << 22)) return nullptr;
    mlgpu_graph::Variant* trial = nullptr;
    for (mlgpu_graph::Variant& v : g->variants)
      if (!v.failed && v.runs < 3 && (!trial || v.runs < trial->runs)) trial = &v;
    if (trial && !trial->fn)
    {
      std::string src, log;
      std::vector<char> code;
      if (generateBudgeted(g->desc, g->build->plan, KernelForm{trial->vl, trial->unroll, 0}, src, code, log)) trial->fn = mlgpu_jit_function(g->e->device, src, "mlgpu_graph_kernel", log);
      if (!trial->fn) trial->failed = true;
    }
    if (trial && !trial->failed) return trial;
    // keep the fastest; the default form stays unless another one is at least 3 % faster (two timed launches per form are a
    // coarse measurement)
    const auto score = [g](const mlgpu_graph::Variant& v) { return v.bestMs * ((v.fn == g->fn) ? 0.97f : 1.0f); };
    const mlgpu_graph::Variant* best = nullptr;
    for (const mlgpu_graph::Variant& v : g->variants)
      if (!v.failed && v.fn && v.runs >= 2 && (!best || score(v) < score(*best))) best = &v;
    if (best)
    {
      g->fn = best->fn;
      g->activeForm = KernelForm{best->vl, best->unroll, 0};
    }
    g->tuned = true;
    return nullptr;
  }
  // ... and the trial's time, taken between the graph's two events once the launch and what follows it are enqueued (waits for them)
  static void tuningRecord(mlgpu_graph* g, mlgpu_graph::Variant* trial, size_t T)
  {
    hipEventRecord(g->tuneEv1.get(), g->e->stream());
    float ms = 0.f;
    if (hipEventSynchronize(g->tuneEv1.get()) != hipSuccess || hipEventElapsedTime(&ms, g->tuneEv0.get(), g->tuneEv1.get()) != hipSuccess)
    {
      trial->failed = true;
      return;
    }
    if (trial->runs >= 1) trial->bestMs = std::min(trial->bestMs, ms / (float)T);
    trial->runs++;
  }

  const char* mlgpu_graph_source(mlgpu_graph* g) { return (g && !g->job && g->build) ? g->build->source.c_str() : ""; }

  // T::clear() of one node: the state words clear() resets (mlgpu_proc_clear_mask), a delay node's rings, a
  // feedback node's stored vector
  static int clearNode(mlgpu_graph* g, size_t node)
  {
    const Node& n = g->desc.nodes[node];
    hipError_t err = hipSetDevice(g->e->device);  // (a host thread may drive engines on several devices in turn)
    if (n.type == NODE_FEEDBACK)
    {
      for (int i = 0; i < n.ns && err == hipSuccess; ++i) err = mlgpu_launch_fill32(g->d_state.get() + (size_t)(n.sOff + i) * g->desc.V, 0u, g->desc.V, g->e->stream());
    }
    else if (n.type == NODE_PROC)
    {
      uint32_t words[MLGPU_MAX_PROC_STATE];
      mlgpu_proc_clear_state(n.kind, words, true);
      const uint64_t mask = mlgpu_proc_clear_mask(n.kind);
      for (int i = 0; i < n.ns && err == hipSuccess; ++i)
        if ((mask >> (i < 64 ? i : 63)) & 1) err = mlgpu_launch_fill32(g->d_state.get() + (size_t)(n.sOff + i) * g->desc.V, words[i], g->desc.V, g->e->stream());
      if (err == hipSuccess && n.ringLen)
        err = mlgpu_launch_fill32((uint32_t*)g->d_mem.get() + g->build->plan.nodes[node].memOff * g->build->plan.memVoices, 0u, n.ringLen * (size_t)mlgpu_proc_rings(n.kind) * g->build->plan.memVoices, g->e->stream());
    }
    if (err != hipSuccess) return gfail(g, MLGPU_ERR_HIP, hipGetErrorString(err));
    return MLGPU_OK;
  }

  int mlgpu_graph_clear(mlgpu_graph* g)
  {
    if (!g) return MLGPU_ERR_INVALID;
    if (g->job) return MLGPU_ERR_BUSY;
    if (!g->compiled) return MLGPU_ERR_INVALID;
    for (size_t node = 0; node < g->desc.nodes.size(); ++node)
    {
      const int st = clearNode(g, node);
      if (st) return st;
    }
    g->vectorCount = 0;
    g->listedSinceClear = false;
    return MLGPU_OK;
  }

  int mlgpu_graph_clear_proc(mlgpu_graph* g, int node)
  {
    if (!g) return MLGPU_ERR_INVALID;
    if (g->job) return MLGPU_ERR_BUSY;
    if (node < 0 || node >= (int)g->desc.nodes.size()) return gfail(g, MLGPU_ERR_RANGE, "node index out of range");
    if (g->desc.nodes[node].type != NODE_PROC && g->desc.nodes[node].type != NODE_FEEDBACK) return gfail(g, MLGPU_ERR_INVALID, "graph_clear_proc: not a processor / feedback node");
    if (!g->compiled) return gfail(g, MLGPU_ERR_INVALID, "graph_clear_proc: compile first");
    return clearNode(g, (size_t)node);
  }

  int mlgpu_graph_set_param(mlgpu_graph* g, int node, const float* h)
  {
    int st = checkNode(g, node, NODE_PARAM);
    if (st) return st;
    if (!g->compiled || !h) return gfail(g, MLGPU_ERR_INVALID, "graph_set_param: compile first / null");
    return mlgpu_upload(g->e, g->d_params.get() + (size_t)g->desc.nodes[node].slot * g->desc.V, h, sizeof(float) * g->desc.V);
  }
  int mlgpu_graph_set_param_uniform(mlgpu_graph* g, int node, float value)
  {
    int st = checkNode(g, node, NODE_PARAM);
    if (st) return st;
    if (!g->compiled) return gfail(g, MLGPU_ERR_INVALID, "graph_set_param: compile first");
    uint32_t u;
    memcpy(&u, &value, 4);
    return mlgpu_fill32(g->e, g->d_params.get() + (size_t)g->desc.nodes[node].slot * g->desc.V, u, g->desc.V);
  }
  int mlgpu_graph_num_coeffs(mlgpu_graph* g, int node) { return checkNode(g, node, NODE_PROC) ? -1 : g->desc.nodes[node].nc; }
  int mlgpu_graph_num_state(mlgpu_graph* g, int node) { return checkStateNode(g, node) ? -1 : g->desc.nodes[node].ns; }
  int mlgpu_graph_set_coeff(mlgpu_graph* g, int node, int idx, const float* h)
  {
    int st = checkNode(g, node, NODE_PROC);
    if (st) return st;
    if (!g->compiled || !h) return gfail(g, MLGPU_ERR_INVALID, "graph_set_coeff: compile first / null");
    if (idx < 0 || idx >= g->desc.nodes[node].nc) return gfail(g, MLGPU_ERR_RANGE, "coefficient index out of range");
    return mlgpu_upload(g->e, g->d_coeffs.get() + (size_t)(g->desc.nodes[node].cOff + idx) * g->desc.V, h, sizeof(float) * g->desc.V);
  }
  int mlgpu_graph_set_coeff_uniform(mlgpu_graph* g, int node, int idx, float value)
  {
    int st = checkNode(g, node, NODE_PROC);
    if (st) return st;
    if (!g->compiled) return gfail(g, MLGPU_ERR_INVALID, "graph_set_coeff: compile first");
    if (idx < 0 || idx >= g->desc.nodes[node].nc) return gfail(g, MLGPU_ERR_RANGE, "coefficient index out of range");
    uint32_t u;
    memcpy(&u, &value, 4);
    return mlgpu_fill32(g->e, g->d_coeffs.get() + (size_t)(g->desc.nodes[node].cOff + idx) * g->desc.V, u, g->desc.V);
  }
  int mlgpu_graph_get_state(mlgpu_graph* g, int node, int idx, uint32_t* h)
  {
    int st = checkStateNode(g, node);
    if (st) return st;
    if (!g->compiled || !h) return gfail(g, MLGPU_ERR_INVALID, "graph_get_state: compile first / null");
    if (idx < 0 || idx >= g->desc.nodes[node].ns) return gfail(g, MLGPU_ERR_RANGE, "state index out of range");
    return mlgpu_download(g->e, h, g->d_state.get() + (size_t)(g->desc.nodes[node].sOff + idx) * g->desc.V, sizeof(uint32_t) * g->desc.V);
  }
  int mlgpu_graph_set_state(mlgpu_graph* g, int node, int idx, const uint32_t* h)
  {
    int st = checkStateNode(g, node);
    if (st) return st;
    if (!g->compiled || !h) return gfail(g, MLGPU_ERR_INVALID, "graph_set_state: compile first / null");
    if (idx < 0 || idx >= g->desc.nodes[node].ns) return gfail(g, MLGPU_ERR_RANGE, "state index out of range");
    return mlgpu_upload(g->e, g->d_state.get() + (size_t)(g->desc.nodes[node].sOff + idx) * g->desc.V, h, sizeof(uint32_t) * g->desc.V);
  }

  int mlgpu_graph_get_param(mlgpu_graph* g, int node, float* h)
  {
    int st = checkNode(g, node, NODE_PARAM);
    if (st) return st;
    if (!g->compiled || !h) return gfail(g, MLGPU_ERR_INVALID, "graph_get_param: compile first / null");
    return mlgpu_download(g->e, h, g->d_params.get() + (size_t)g->desc.nodes[node].slot * g->desc.V, sizeof(float) * g->desc.V);
  }
  int mlgpu_graph_get_coeff(mlgpu_graph* g, int node, int idx, float* h)
  {
    int st = checkNode(g, node, NODE_PROC);
    if (st) return st;
    if (!g->compiled || !h) return gfail(g, MLGPU_ERR_INVALID, "graph_get_coeff: compile first / null");
    if (idx < 0 || idx >= g->desc.nodes[node].nc) return gfail(g, MLGPU_ERR_RANGE, "coefficient index out of range");
    return mlgpu_download(g->e, h, g->d_coeffs.get() + (size_t)(g->desc.nodes[node].cOff + idx) * g->desc.V, sizeof(float) * g->desc.V);
  }

  // ---- sparse, stream-ordered updates (param_updates.hpp plans, updates.hip applies) ----
  // The compiled graph's tables as the planner sees them: which rows each node owns, and what clearNode() writes to a node's state
  static int updatesReady(mlgpu_graph* g, const char* who)
  {
    if (!g) return MLGPU_ERR_INVALID;
    if (g->job) return MLGPU_ERR_BUSY;
    if (!g->compiled) return gfail(g, MLGPU_ERR_INVALID, std::string(who) + ": compile first");
    mlgpu_updater& u = g->updates;
    if (u.described) return MLGPU_OK;
    u.desc.bank = false;
    u.desc.V = g->desc.V;
    // where a voice's ring words lie (MLGPU_UPDATE_CLEAR_RINGS): the layout's granule, and the spare lanes of ring layout 2
    const GraphPlan& plan = g->build->plan;
    u.desc.ringGranule = plan.rings == RingLayout::ROWS ? 1u : plan.rings == RingLayout::TRANSPOSED ? 16u : 8u;
    u.desc.memVoices = plan.memVoices;
    u.desc.spareLanes = plan.rings == RingLayout::TRANSPOSED && plan.totalRings && (g->desc.V % 64) != 0;
    u.desc.nodes.assign(g->desc.nodes.size(), mlupd::NodeDesc());
    for (size_t i = 0; i < g->desc.nodes.size(); ++i)
    {
      const Node& n = g->desc.nodes[i];
      mlupd::NodeDesc& nd = u.desc.nodes[i];
      if (n.type == NODE_PARAM)
      {
        nd.kind = mlupd::NodeDesc::PARAM;
        nd.paramRow = n.slot;
      }
      else if (n.type == NODE_FEEDBACK)
      {
        nd.kind = mlupd::NodeDesc::FEEDBACK;
        nd.sOff = n.sOff;
        nd.ns = n.ns;
        nd.clearWords.assign((size_t)n.ns, 0u);
        nd.clearMask.assign((size_t)n.ns, 1);
      }
      else if (n.type == NODE_PROC)
      {
        nd.kind = mlupd::NodeDesc::PROC;
        nd.cOff = n.cOff;
        nd.nc = n.nc;
        nd.sOff = n.sOff;
        nd.ns = n.ns;
        nd.rings = n.ringLen != 0 || mlgpu_proc_rings(n.kind) > 0;
        nd.memOff = plan.nodes[i].memOff;
        nd.ringWords = (uint64_t)n.ringLen * (uint64_t)mlgpu_proc_rings(n.kind);
        uint32_t words[MLGPU_MAX_PROC_STATE];
        mlgpu_proc_clear_state(n.kind, words, true);
        const uint64_t mask = mlgpu_proc_clear_mask(n.kind);
        nd.clearWords.assign(words, words + n.ns);
        nd.clearMask.resize((size_t)n.ns);
        for (int w = 0; w < n.ns; ++w) nd.clearMask[(size_t)w] = (uint8_t)((mask >> (w < 64 ? w : 63)) & 1);
      }
    }
    u.described = true;
    return MLGPU_OK;
  }
  int mlgpu_graph_reserve_updates(mlgpu_graph* g, size_t maxDeviceRecords)
  {
    if (const int st = updatesReady(g, "graph_reserve_updates")) return st;
    std::string err;
    const int st = mlgpu_updater_reserve(g->e, g->updates, maxDeviceRecords, err);
    return st == MLGPU_OK ? st : gfail(g, st, "graph_" + err);
  }
  size_t mlgpu_graph_update_device_records(mlgpu_graph* g, const mlgpu_update* recs, size_t n)
  {
    if (updatesReady(g, "graph_update_device_records")) return 0;
    return mlgpu_updater_device_records(g->updates, recs, n);
  }
  int mlgpu_graph_apply_updates(mlgpu_graph* g, const mlgpu_update* recs, size_t n)
  {
    if (const int st = updatesReady(g, "graph_apply_updates")) return st;
    uint32_t* const tables[mlupd::kTables] = {(uint32_t*)g->d_params.get(), (uint32_t*)g->d_coeffs.get(), g->d_state.get(), nullptr};
    std::string err;
    const int st = mlgpu_updater_apply(g->e, g->updates, tables, (uint32_t*)g->d_mem.get(), g->build->plan.memVoices * g->build->plan.memFloatsPerVoice, recs, n, err);
    return st == MLGPU_OK ? st : gfail(g, st, "graph_" + err);
  }
  // Not in mlgpu.h: the tests' view of the staging sets (their four buffer addresses, the capacity in records), to see that
  // apply_updates after a reserve leaves them alone
  size_t mlgpu_graph_update_staging(mlgpu_graph* g, const void** four) { return (g && !g->job && four) ? mlgpu_updater_staging(g->updates, four) : 0; }

  // ---- voice records: listed voices' whole state to and from a device buffer (voice_records.hpp plans, voice_records.hip moves) ----
  // The compiled graph's record layout and signature, from the tables' description the updates keep
  static int recordsReady(mlgpu_graph* g, const char* who)
  {
    if (const int st = updatesReady(g, who)) return st;
    mlgpu_recorder& r = g->records;
    if (!r.described)
    {
      std::vector<mlrec::NodeSig> sigs(g->desc.nodes.size());
      for (size_t i = 0; i < sigs.size(); ++i)
      {
        const Node& n = g->desc.nodes[i];
        sigs[i].type = n.type;
        sigs[i].kind = n.kind;
        sigs[i].ringLen = (uint32_t)n.ringLen;
        sigs[i].rings = n.type == NODE_PROC ? (uint32_t)mlgpu_proc_rings(n.kind) : 0u;
      }
      r.plan.describe(g->updates.desc, sigs, apiLayout(g->build->plan.rings), mlgpu_behaviour_revision());
      r.described = true;
    }
    if (!r.plan.described()) return gfail(g, MLGPU_ERR_UNSUPPORTED, std::string(who) + ": " + r.plan.error());
    return MLGPU_OK;
  }
  // The refusals of a move that are the graph's own, before anything is enqueued
  static int recordsMovable(mlgpu_graph* g, const char* who, bool import)
  {
    for (const Region& R : g->desc.regions)
      if (R.kind == MLGPU_REGION_DOWNSAMPLE_2X)
        return gfail(g, MLGPU_ERR_UNSUPPORTED, std::string(who) + ": a graph with a DOWNSAMPLE_2X region pairs its DSPVectors by a count that is the graph's, not a voice's: a voice's record would not say which half of a pair it stands at");
    if (import && g->build->plan.rings == RingLayout::SECTORS && !g->build->plan.ringsByLaneOnly)
      for (const Node& n : g->desc.nodes)
        if (n.type == NODE_PROC && n.kind == MLGPU_PROC_PITCHBENDABLE_DELAY)
          return gfail(g, MLGPU_ERR_UNSUPPORTED,
                       std::string(who) + ": a PitchbendableDelay in delay layout 4 keeps one ring per WAVEFRONT while its voices' write indices agree, and an imported voice brings its own: "
                                          "its neighbours would read a second ring nobody wrote. Compile the graph with mlgpu_graph_enable_voice_list_rings (the listed kernels decide per lane), "
                                          "or use another delay layout");
    return MLGPU_OK;
  }
  size_t mlgpu_graph_voice_record_words(mlgpu_graph* g)
  {
    if (!g || g->job || !g->compiled) return 0;
    return recordsReady(g, "graph_voice_record_words") ? 0 : g->records.plan.words();
  }
  uint64_t mlgpu_graph_voice_record_signature(mlgpu_graph* g)
  {
    if (!g || g->job || !g->compiled) return 0;
    return recordsReady(g, "graph_voice_record_signature") ? 0 : g->records.plan.signature();
  }
  int mlgpu_graph_reserve_voice_records(mlgpu_graph* g, size_t maxVoices)
  {
    if (const int st = recordsReady(g, "graph_reserve_voice_records")) return st;
    std::string err;
    const int st = mlgpu_recorder_reserve(g->e, g->records, maxVoices, err);
    return st == MLGPU_OK ? st : gfail(g, st, "graph_" + err);
  }
  static int moveVoices(mlgpu_graph* g, const char* who, const uint32_t* h_voices, size_t n, uint32_t* d_records, bool import)
  {
    uint32_t* const tables[mlupd::kTables] = {(uint32_t*)g->d_params.get(), (uint32_t*)g->d_coeffs.get(), g->d_state.get(), nullptr};
    std::string err;
    const int st = mlgpu_recorder_move(g->e, g->records, tables, (uint32_t*)g->d_mem.get(), g->build->plan.memVoices * g->build->plan.memFloatsPerVoice, h_voices, n, d_records, import, err);
    return st == MLGPU_OK ? st : gfail(g, st, "graph_" + err);
  }
  int mlgpu_graph_export_voices(mlgpu_graph* g, const uint32_t* h_voices, size_t n, uint32_t* d_records)
  {
    if (const int st = recordsReady(g, "graph_export_voices")) return st;
    if (const int st = recordsMovable(g, "graph_export_voices", false)) return st;
    return moveVoices(g, "graph_export_voices", h_voices, n, d_records, false);
  }
  int mlgpu_graph_import_voices(mlgpu_graph* g, uint64_t signature, const uint32_t* h_voices, size_t n, const uint32_t* d_records)
  {
    if (const int st = recordsReady(g, "graph_import_voices")) return st;
    if (signature != g->records.plan.signature())
      return gfail(g, MLGPU_ERR_UNSUPPORTED, "graph_import_voices: the records' signature differs from this graph's (another description, ring layout, record format or behaviour revision): such objects do not exchange records");
    if (const int st = recordsMovable(g, "graph_import_voices", true)) return st;
    const int st = moveVoices(g, "graph_import_voices", h_voices, n, (uint32_t*)d_records, true);
    // the imported voices' write indices differ from their neighbours' now, as after a listed launch (processPlain)
    if (st == MLGPU_OK && n && g->build->plan.ringsByLaneOnly) g->listedSinceClear = true;
    return st;
  }
  size_t mlgpu_graph_voice_record_staging(mlgpu_graph* g, const void** four) { return (g && !g->job && four) ? mlgpu_recorder_staging(g->records, four) : 0; }  // (not in mlgpu.h: the tests' view, as mlgpu_graph_update_staging)

  int mlgpu_graph_set_delay_layout(mlgpu_graph* g, int windowed)
  {
    if (const int st = checkEditable(g)) return st;
    if (windowed < 0 || windowed > 4)
      return gfail(g, MLGPU_ERR_INVALID, "graph_set_delay_layout: 0 (rows), 1 (32-byte sectors), 2 (transposed 64-byte pieces), 4 (sector trips) or 3 (the best of 2 / 4 / 1 for the graph)");
    g->desc.delayLayout = windowed;  // (layout 3: decided at compile, when the number of rings is known)
    return MLGPU_OK;
  }

  int mlgpu_graph_set_autotune(mlgpu_graph* g, int on)
  {
    if (const int st = checkEditable(g)) return st;
    g->desc.autotune = on != 0;
    return MLGPU_OK;
  }
  int mlgpu_graph_enable_voice_lists(mlgpu_graph* g, int on)
  {
    if (const int st = checkEditable(g, "graph_enable_voice_lists: before mlgpu_graph_compile")) return st;
    g->desc.voiceLists = on != 0;
    if (!on) g->desc.voiceListGroups = g->desc.voiceListEvents = g->desc.voiceListMpeEvents = g->desc.voiceListRings = false;
    return MLGPU_OK;
  }
  // ... and a graph with delay rings has its listed form in the sector layouts too (1 and 4: a voice owns its 32-byte sectors, memory
  // goes by the voice and LDS by the lane; layout 3 then resolves to 4, 1 or the rows, never to 2 - planGraph). on = 1 turns voice lists
  // on too; mlgpu_graph_enable_voice_lists(g, 0) turns it off with the rest.
  int mlgpu_graph_enable_voice_list_rings(mlgpu_graph* g, int on)
  {
    if (const int st = checkEditable(g, "graph_enable_voice_list_rings: before mlgpu_graph_compile")) return st;
    g->desc.voiceListRings = on != 0;
    if (on) g->desc.voiceLists = true;
    return MLGPU_OK;
  }
  // ... and a graph with event rows has a listed form as well (mlgpu_graph_process_events_listed[_groups]): CtlVoice of the gathered
  // voice. on = 1 turns voice lists on too; mlgpu_graph_enable_voice_lists(g, 0) turns it off with the rest.
  int mlgpu_graph_enable_voice_list_events(mlgpu_graph* g, int on)
  {
    if (const int st = checkEditable(g, "graph_enable_voice_list_events: before mlgpu_graph_compile")) return st;
    g->desc.voiceListEvents = on != 0;
    if (on) g->desc.voiceLists = true;
    else g->desc.voiceListMpeEvents = false;  // (the MPE-capable listed form is a listed form of the event rows)
    return MLGPU_OK;
  }
  // ... in the form for either protocol (mlev::CtlVoiceMpe / CtlRowsMpe of the gathered voice): mlgpu_graph_process_events_listed[_groups]
  // then serve the protocol the bound object has at the call. on = 1 turns on mlgpu_graph_enable_voice_list_events (and through it voice
  // lists) and mlgpu_graph_enable_mpe_events; mlgpu_graph_enable_voice_lists(g, 0), mlgpu_graph_enable_voice_list_events(g, 0) and
  // mlgpu_graph_enable_mpe_events(g, 0) turn it off with the rest.
  int mlgpu_graph_enable_voice_list_mpe_events(mlgpu_graph* g, int on)
  {
    if (const int st = checkEditable(g, "graph_enable_voice_list_mpe_events: before mlgpu_graph_compile")) return st;
    g->desc.voiceListMpeEvents = on != 0;
    if (on) g->desc.voiceLists = g->desc.voiceListEvents = g->desc.mpeEvents = true;
    return MLGPU_OK;
  }
  // The plain kernel of a graph with event rows in its MPE-capable form (mlev::CtlVoiceMpe / CtlRowsMpe): the graph binds to an events
  // object in either protocol and mlgpu_graph_process_events serves the protocol the object has at the call. The listed forms keep
  // their text and their refusal under MPE unless mlgpu_graph_enable_voice_list_mpe_events is on as well.
  int mlgpu_graph_enable_mpe_events(mlgpu_graph* g, int on)
  {
    if (const int st = checkEditable(g, "graph_enable_mpe_events: before mlgpu_graph_compile")) return st;
    g->desc.mpeEvents = on != 0;
    if (!on) g->desc.voiceListMpeEvents = false;
    return MLGPU_OK;
  }
  // ... and the listed form goes by the host's lane plan: the graph's group-summed outputs get one row per listed instrument
  // (mlgpu_graph_process_listed_groups). on = 1 turns voice lists on too; mlgpu_graph_enable_voice_lists(g, 0) turns both off.
  int mlgpu_graph_enable_voice_list_groups(mlgpu_graph* g, int on)
  {
    if (const int st = checkEditable(g, "graph_enable_voice_list_groups: before mlgpu_graph_compile")) return st;
    g->desc.voiceListGroups = on != 0;
    if (on) g->desc.voiceLists = true;
    return MLGPU_OK;
  }
  int mlgpu_graph_set_live_constants(mlgpu_graph* g, int on)
  {
    if (const int st = checkEditable(g, "graph_set_live_constants: before mlgpu_graph_compile")) return st;
    g->desc.liveConsts = on != 0;
    return MLGPU_OK;
  }
  int mlgpu_graph_set_const(mlgpu_graph* g, int node, float value)
  {
    if (!g) return MLGPU_ERR_INVALID;
    if (g->job) return MLGPU_ERR_BUSY;  // (the worker turns the values into literals of the kernel)
    if (node < 0 || node >= (int)g->desc.nodes.size() || g->desc.nodes[node].type != NODE_CONST) return gfail(g, MLGPU_ERR_INVALID, "graph_set_const: not a const node");
    if (g->compiled && !g->desc.liveConsts)
      return gfail(g, MLGPU_ERR_INVALID, "graph_set_const: constants of this graph are literals of its kernel (mlgpu_graph_set_live_constants before compile)");
    if (!g->compiled) checkEditable(g);  // (the value is a literal of the kernel, or what compile fills d_consts with)
    g->desc.nodes[node].value = value;
    if (!g->compiled) return MLGPU_OK;
    uint32_t u;
    memcpy(&u, &value, 4);
    return mlgpu_fill32(g->e, g->d_consts.get() + g->desc.nodes[node].slot, u, 1);
  }
  // Same nodes, same wiring? (what a second capture of the same user code produces when only host-side numbers changed)
  static const char* structureDifference(const mlgpu_graph* a, const mlgpu_graph* b)
  {
    if (a->desc.V != b->desc.V) return "number of voices";
    if (a->desc.nodes.size() != b->desc.nodes.size()) return "number of nodes";
    for (size_t i = 0; i < a->desc.nodes.size(); ++i)
    {
      const Node &x = a->desc.nodes[i], &y = b->desc.nodes[i];
      if (x.type != y.type || x.kind != y.kind || x.in != y.in || x.slot != y.slot || x.nOut != y.nOut || x.fbSource != y.fbSource || x.region != y.region ||
          x.role != y.role || x.rate != y.rate)
        return "a node or its inputs";
      if (x.ringLen != y.ringLen) return "a delay line's maximum length";
      if (x.table != y.table) return "a constant DSPVector";
      if (x.type == NODE_CONST && !a->desc.liveConsts && memcmp(&x.value, &y.value, 4) != 0) return "a constant (this graph was not compiled with live constants)";
    }
    if (a->desc.outputs != b->desc.outputs) return "outputs";
    if (a->desc.regions.size() != b->desc.regions.size()) return "rate regions";
    return nullptr;
  }
  int mlgpu_graph_update_constants_from(mlgpu_graph* g, mlgpu_graph* other)
  {
    if (!g || !other) return MLGPU_ERR_INVALID;
    if (g->job || other->job) return MLGPU_ERR_BUSY;
    if (!g->compiled) return gfail(g, MLGPU_ERR_INVALID, "graph_update_constants_from: compile the graph first");
    if (const char* why = structureDifference(g, other)) return gfail(g, MLGPU_ERR_UNSUPPORTED, std::string("graph_update_constants_from: the graphs differ in ") + why);
    for (size_t i = 0; i < g->desc.nodes.size(); ++i)
    {
      Node& n = g->desc.nodes[i];
      if (n.type != NODE_CONST || memcmp(&n.value, &other->desc.nodes[i].value, 4) == 0) continue;
      const int st = mlgpu_graph_set_const(g, (int)i, other->desc.nodes[i].value);
      if (st != MLGPU_OK) return st;
    }
    return MLGPU_OK;
  }
  size_t mlgpu_graph_device_bytes(mlgpu_graph* g)
  {
    if (!g || g->job || !g->compiled) return 0;
    return sizeof(float) * g->desc.V * (size_t)(g->desc.NC + 1) + sizeof(uint32_t) * g->desc.V * (size_t)(g->desc.NS + 1) + sizeof(float) * g->desc.V * (size_t)(g->desc.nParams + 1) +
           sizeof(float) * g->build->plan.memVoices * g->build->plan.memFloatsPerVoice;
  }
  int mlgpu_graph_tuning(mlgpu_graph* g, int* voicesPerLane, int* quadsPerTrip)
  {
    if (!g) return -MLGPU_ERR_INVALID;
    if (g->job) return -MLGPU_ERR_BUSY;
    if (!g->compiled) return -MLGPU_ERR_INVALID;
    if (voicesPerLane) *voicesPerLane = g->activeForm.voicesPerLane;
    if (quadsPerTrip) *quadsPerTrip = g->activeForm.quadsPerTrip;
    return (g->desc.autotune && !g->tuned) ? 0 : 1;
  }

  // how many workgroups of this graph's kernel a CU holds at once (registers, LDS and wavefront slots together): what decides whether a
  // bank runs in one round (voices <= 256 x that x the CU count) or the last workgroups run alone after the others
  int mlgpu_graph_workgroups_per_cu(mlgpu_graph* g)
  {
    if (!g) return -MLGPU_ERR_INVALID;
    if (g->job) return -MLGPU_ERR_BUSY;
    if (!g->compiled || !g->fn) return -MLGPU_ERR_INVALID;
    int n = 0;
    if (hipSetDevice(g->e->device) != hipSuccess) return -MLGPU_ERR_HIP;
    if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&n, g->fn, 256, 0) != hipSuccess) return -MLGPU_ERR_HIP;
    return n;
  }

  // the ring layout in effect (after compile: what layout 3 came out as)
  int mlgpu_graph_delay_layout(mlgpu_graph* g)
  {
    if (!g) return -MLGPU_ERR_INVALID;
    if (g->job) return -MLGPU_ERR_BUSY;  // (layout 3 is being decided)
    return g->compiled ? apiLayout(g->build->plan.rings) : g->desc.delayLayout;
  }

  int mlgpu_graph_set_voices_per_lane(mlgpu_graph* g, int n)
  {
    if (const int st = checkEditable(g)) return st;
    if (n < 0 || n > 2) return gfail(g, MLGPU_ERR_INVALID, "graph_set_voices_per_lane: 0 (automatic), 1 or 2");
    g->desc.voicesPerLane = n;
    return MLGPU_OK;
  }

  int mlgpu_graph_set_input_layout(mlgpu_graph* g, int inputIndex, int layout)
  {
    if (!g) return MLGPU_ERR_INVALID;
    if (g->job) return MLGPU_ERR_BUSY;
    if (inputIndex < 0 || inputIndex >= g->desc.nInputs) return gfail(g, MLGPU_ERR_RANGE, "graph_set_input_layout: input index out of range");
    if (layout < -1 || layout > MLGPU_LAYOUT_BROADCAST) return gfail(g, MLGPU_ERR_INVALID, "graph_set_input_layout: bad layout");
    g->inLayoutOverride[inputIndex] = layout;
    return MLGPU_OK;
  }

  int mlgpu_graph_set_input_group(mlgpu_graph* g, int inputIndex, int group)
  {
    if (const int st = checkEditable(g)) return st;
    if (inputIndex < 0 || inputIndex >= g->desc.nInputs) return gfail(g, MLGPU_ERR_RANGE, "graph_set_input_group: input index out of range");
    if (group < 1 || (size_t)group > g->desc.V || g->desc.V % (size_t)group) return gfail(g, MLGPU_ERR_INVALID, "graph_set_input_group: the voices are not a whole number of groups");
    g->desc.inputGroup[inputIndex] = group;
    return MLGPU_OK;
  }

  int mlgpu_graph_set_state_uniform(mlgpu_graph* g, int node, int idx, uint32_t value)
  {
    int st = checkStateNode(g, node);
    if (st) return st;
    if (!g->compiled) return gfail(g, MLGPU_ERR_INVALID, "graph_set_state: compile first");
    if (idx < 0 || idx >= g->desc.nodes[node].ns) return gfail(g, MLGPU_ERR_RANGE, "state index out of range");
    return mlgpu_fill32(g->e, g->d_state.get() + (size_t)(g->desc.nodes[node].sOff + idx) * g->desc.V, value, g->desc.V);
  }

  // What every process call hands its kernel but the outputs: the tables, the streamed inputs as signals of the graph's voices (or of
  // its input groups) and the controls. MLGPU_OK, or the refusal in `who`'s name.
  static int signalArgs(mlgpu_graph* g, GraphArgs& a, const char* who, size_t T, const float* const* d_inputs, int inLayout, const float* const* d_controls,
                        float* const* d_outputs, int outLayout)
  {
    const auto name = [who] { return std::string(who); };  // (made where a refusal needs it: the success path allocates nothing)
    if (inLayout < 0 || inLayout > MLGPU_LAYOUT_BROADCAST || outLayout < 0 || outLayout > MLGPU_LAYOUT_VOICE_MAJOR) return gfail(g, MLGPU_ERR_INVALID, name() + ": bad layout");
    if ((g->desc.nInputs && !d_inputs) || (g->desc.nControls && !d_controls) || !d_outputs) return gfail(g, MLGPU_ERR_INVALID, name() + ": null signal list");
    memset(&a, 0, sizeof(a));
    a.coeffs = g->d_coeffs.get();
    a.state = g->d_state.get();
    a.params = g->d_params.get();
    a.consts = g->d_consts.get();
    a.mem = g->d_mem.get();
    a.V = g->desc.V;
    a.T = T;
    a.t0 = g->vectorCount;  // (advanced by the plain call only; no listed graph has a region that reads it)
    a.flags = g->e->kflags;
    a.impulseTable = g->e->d_impulseTable.get();
    for (int i = 0; i < g->desc.nInputs; ++i)
    {
      if (!d_inputs[i] || ((uintptr_t)d_inputs[i] & 15)) return gfail(g, MLGPU_ERR_INVALID, name() + ": null / misaligned input");
      const int lay = (g->inLayoutOverride[i] >= 0) ? g->inLayoutOverride[i] : inLayout;
      a.in[i] = makeView(d_inputs[i], lay, g->desc.inputGroup[i] > 1 ? g->desc.V / (size_t)g->desc.inputGroup[i] : g->desc.V, T);
    }
    for (int i = 0; i < g->desc.nControls; ++i)
    {
      if (!d_controls[i]) return gfail(g, MLGPU_ERR_INVALID, name() + ": null control signal");
      a.ctl[i] = d_controls[i];
    }
    for (size_t o = 0; o < g->desc.outputs.size(); ++o)
      if (!d_outputs[o] || ((uintptr_t)d_outputs[o] & 15)) return gfail(g, MLGPU_ERR_INVALID, name() + ": null / misaligned output");
    return MLGPU_OK;
  }

  // The outputs of a call whose kernel writes `rows` rows per output - voices, or list positions - and `groupRows` for a group-summed
  // one (0: rows / the output's group). A mixed-down output is the tree of the `rows` voices: the kernel writes its first stage into
  // that output's region of the engine's mixdown scratch, mixdownStages follows the launch. MLGPU_OK, or the refusal `noScratch`.
  static int outputViews(mlgpu_graph* g, GraphArgs& a, size_t T, float* const* d_outputs, int outLayout, size_t rows, size_t groupRows, const char* noScratch)
  {
    const size_t nMix = mixedOutputs(g);
    for (size_t o = 0, r = 0; o < g->desc.outputs.size(); ++o)
    {
      const size_t group = (size_t)g->desc.outputGroup[o];
      if (!g->desc.outputMix[o]) a.out[o] = makeView(d_outputs[o], outLayout, !group ? rows : (groupRows ? groupRows : rows / group), T);
      else if (rows)  // (no voices: no tree, nothing launched)
      {
        float* const region = g->e->mixdownRegion(rows, T, r++, nMix);
        if (!region) return gfail(g, MLGPU_ERR_INVALID, noScratch);
        a.out[o] = makeView(region, MLGPU_LAYOUT_QUAD, rows, T);
      }
    }
    return MLGPU_OK;
  }
  // ... over the region outputViews gave it (the shard form is the plain call's alone: planGraph refuses it a listed form)
  static int mixdownStages(mlgpu_graph* g, size_t T, float* const* d_outputs, size_t voices, const char* who)
  {
    const size_t nMix = mixedOutputs(g);
    for (size_t o = 0, r = 0; o < g->desc.outputs.size(); ++o)
      if (g->desc.outputMix[o] &&
          mlgpu_launch_mixdown_rows(mlmix::groupsOf(voices), T, g->e->mixdownRegion(voices, T, r++, nMix), d_outputs[o],
                                    g->desc.outputMixShard[o] ? mlmix::shardLevel(voices) - 1 : mlmix::kToTheEnd, g->e->stream(), g->e->kflags) != hipSuccess)
        return gfail(g, MLGPU_ERR_HIP, std::string(who) + ": the mixdown's later stages");
    return MLGPU_OK;
  }
  // ---- the events of a process call, plain or listed. The call has the block's frame offset as an argument (eventOffset; < 0: it is
  // not an events call) and goes through these three in this order; `listed` says which kernel it launches. The events object belongs
  // to ALL voices: its host half (routing the block's events into records, their upload) and e2s_ctl_kernel run for every lane in every
  // call, on the engine's stream - note state, the pitch and bend glides and the drift random walk advance for listed and unlisted
  // voices alike -, the voice kernel then expands the control records of its voices only. ----
  // The protocol form of the kernel the call launches: for an events object in either protocol, or MIDI only
  static bool eventsEitherProtocol(const mlgpu_graph* g, bool listed) { return listed ? g->desc.voiceListMpeEvents : g->desc.mpeEvents; }
  // What the call refuses without looking at the block
  static int eventsReady(mlgpu_graph* g, const char* who0, int eventOffset, bool listed)
  {
    const auto who = [who0] { return std::string(who0); };  // (made where a refusal needs it: the success path allocates nothing)
    if (!g->desc.hasEventRows) return MLGPU_OK;  // (an events call of such a graph: refused by its entry point)
    // (a call that is no events call and has no events object either: the plain call names the object, a listed call the call)
    if (eventOffset < 0 && (listed || g->events))
      return gfail(g, MLGPU_ERR_INVALID, who() + ": a graph with event rows is run with mlgpu_graph_process_events" + (listed ? "_listed[_groups]" : ""));
    if (!g->events) return gfail(g, MLGPU_ERR_INVALID, who() + ": the graph has event rows but no events object (graph_bind_events)");
    // (a plain kernel's protocol is settled when the object is bound: graph_bind_events)
    if (listed && !eventsEitherProtocol(g, listed) && !mlgpu_events_is_midi(g->events))
      return gfail(g, MLGPU_ERR_UNSUPPORTED, who() + ": events as graph source nodes: MIDI protocol only (one lane per voice) - mlgpu_graph_enable_voice_list_mpe_events(g, 1) "
                                                     "before compile makes the listed form for either protocol");
    return MLGPU_OK;
  }
  // ... and once nothing of the call can be refused any more: the host half and e2s_ctl_kernel. *staging: null if the call is not an
  // events call, else what the launch is reported with.
  static int eventsPrepare(mlgpu_graph* g, const char* who0, size_t T, int eventOffset, bool listed, GraphArgs& a, void** staging)
  {
    const auto who = [who0] { return std::string(who0); };
    *staging = nullptr;
    if (eventOffset < 0) return MLGPU_OK;
    const int est = mlgpu_events_prepare_for_graph(g->events, T, eventOffset, g->desc.eventRowMask, eventsEitherProtocol(g, listed) ? 1 : 0, &a.events, staging);
    return est == MLGPU_OK ? est : gfail(g, est, who() + ": the events object refused the block: " + g->e->lastError);
  }
  // ... and after the voice kernel's launch (or instead of it: an empty list - e2s_ctl_kernel has consumed the lanes' record ranges itself)
  static int eventsLaunched(mlgpu_graph* g, const char* who0, void* staging, hipError_t err)
  {
    const auto who = [who0] { return std::string(who0); };
    if (staging && err != hipSuccess) mlgpu_events_abandoned_by_graph(g->events, staging);  // (the lanes' record ranges back to "none": no kernel will consume them)
    if (err != hipSuccess) return gfail(g, MLGPU_ERR_HIP, who() + " launch: " + hipGetErrorString(err));
    if (staging)
      if (const int est = mlgpu_events_launched_by_graph(g->events, staging)) return gfail(g, est, who() + ": events bookkeeping after the launch");
    return MLGPU_OK;
  }

  // The plain call: all voices. Its refusals are in the name of graph_process, whichever entry point it came through.
  static int processPlain(mlgpu_graph* g, size_t T, int eventOffset, const float* const* d_inputs, int inLayout, const float* const* d_controls,
                          float* const* d_outputs, int outLayout)
  {
    if (!g) return MLGPU_ERR_INVALID;
    if (g->job) return MLGPU_ERR_BUSY;
    if (!g->compiled) return gfail(g, MLGPU_ERR_INVALID, "graph_process: compile first");
    if (T == 0) return MLGPU_OK;
    // A PitchbendableDelay in ring layout 4 next to voice lists (mlgpu_graph_enable_voice_list_rings): the listed kernel keeps ONE ring for
    // a voice whose two write indices agree, whatever its wavefront does; this kernel decides per wavefront, and a wavefront whose voices
    // were listed for different numbers of DSPVectors would send them all through two rings - the second never written (mldsp_procs.hpp,
    // above RingCore::beginS). Wrong samples are not an answer: refused until the next clear. A recorded launch is replayed later, after
    // who knows which listed launches: refused as well.
    if (g->build->plan.ringsByLaneOnly && (g->listedSinceClear || g->e->recording))
      return gfail(g, MLGPU_ERR_UNSUPPORTED,
                   std::string("graph_process: a PitchbendableDelay in delay layout 4 next to voice lists (mlgpu_graph_enable_voice_list_rings) ") +
                       (g->listedSinceClear ? "after a listed launch" : "while recording a sequence") +
                       ": the listed kernel keeps one ring per voice where this kernel decides per wavefront, and the listed voices' write indices now differ - run "
                       "all voices through mlgpu_graph_process_listed (every voice listed), or mlgpu_graph_clear first");
    GraphArgs a;
    if (const int st = signalArgs(g, a, "graph_process", T, d_inputs, inLayout, d_controls, d_outputs, outLayout)) return st;
    if (const int st = outputViews(g, a, T, d_outputs, outLayout, g->desc.V, 0,
                                   "graph_process: call mlgpu_graph_reserve_mixdown(graph, max vectors) at setup (mlgpu_mixdown_reserve's scratch; process calls do not allocate)"))
      return st;
    if (g->e->recording)
    {
      if (g->desc.autotune && !g->tuned) return gfail(g, MLGPU_ERR_INVALID, "graph_process: a graph that is still tuning cannot be recorded into a sequence");
      for (const Region& R : g->desc.regions)
        if (R.kind == MLGPU_REGION_DOWNSAMPLE_2X)
          return gfail(g, MLGPU_ERR_INVALID, "graph_process: a graph with a DOWNSAMPLE_2X region counts DSPVectors and cannot be recorded into a sequence");
    }
    if (hipSetDevice(g->e->device) != hipSuccess) return gfail(g, MLGPU_ERR_HIP, "hipSetDevice");
    mlgpu_graph::Variant* const trial = tuningTrial(g, T);
    const hipFunction_t fn = trial ? trial->fn : g->fn;
    const int vl = trial ? trial->vl : g->activeForm.voicesPerLane;
    if (trial && !g->tuneEv0 && (allocate(g->tuneEv0) != hipSuccess || allocate(g->tuneEv1) != hipSuccess))
      return gfail(g, MLGPU_ERR_HIP, "graph_process: hipEventCreate");
    void* eventStaging = nullptr;
    if (const int st = eventsReady(g, "graph_process", eventOffset, false)) return st;
    if (const int st = eventsPrepare(g, "graph_process", T, eventOffset, false, a, &eventStaging)) return st;
    if (trial) hipEventRecord(g->tuneEv0.get(), g->e->stream());
    const hipError_t err = mlgpu_jit_launch(fn, &a, sizeof(a), (g->desc.V + (size_t)vl - 1) / (size_t)vl, g->e->stream());
    if (const int st = eventsLaunched(g, "graph_process", eventStaging, err)) return st;
    if (const int st = mixdownStages(g, T, d_outputs, g->desc.V, "graph_process")) return st;
    if (trial) tuningRecord(g, trial, T);
    g->vectorCount += T;
    return MLGPU_OK;
  }
  int mlgpu_graph_process_ctl(mlgpu_graph* g, size_t T, const float* const* d_inputs, int inLayout, const float* const* d_controls,
                              float* const* d_outputs, int outLayout)
  {
    return processPlain(g, T, -1, d_inputs, inLayout, d_controls, d_outputs, outLayout);
  }
  int mlgpu_graph_process(mlgpu_graph* g, size_t T, const float* const* d_inputs, int inLayout, float* const* d_outputs, int outLayout)
  {
    return processPlain(g, T, -1, d_inputs, inLayout, nullptr, d_outputs, outLayout);
  }
  // a graph with event rows: T DSPVectors starting at frame startOffset of the bound object's event times (as mlgpu_events_process)
  int mlgpu_graph_process_events(mlgpu_graph* g, size_t T, int startOffset, const float* const* d_inputs, int inLayout, const float* const* d_controls,
                                 float* const* d_outputs, int outLayout)
  {
    if (!g) return MLGPU_ERR_INVALID;
    if (g->job) return MLGPU_ERR_BUSY;
    if (!g->desc.hasEventRows) return gfail(g, MLGPU_ERR_INVALID, "graph_process_events: the graph has no event rows");
    if (startOffset < 0) return gfail(g, MLGPU_ERR_INVALID, "graph_process_events: negative frame offset");
    return processPlain(g, T, startOffset, d_inputs, inLayout, d_controls, d_outputs, outLayout);
  }

  // ---- voice lists: run only the listed voices (mlgpu_voice_list keeps the list, the listed form of the generated kernel runs it);
  // `planned`: the call wants the listed form that goes by the host's lane plan (voice_list.hpp; the group-summed outputs summed by
  // instrument), else any listed form ----
  static int listsReady(mlgpu_graph* g, const char* who, bool planned = false)
  {
    if (!g) return MLGPU_ERR_INVALID;
    if (g->job) return MLGPU_ERR_BUSY;
    if (!(planned ? g->desc.voiceListGroups : g->desc.voiceLists))
      return gfail(g, MLGPU_ERR_INVALID,
                   std::string(who) + (planned ? ": the graph's listed form does not go by a lane plan - mlgpu_graph_enable_voice_list_groups(g, 1) before compile"
                                               : ": the graph has no listed form - mlgpu_graph_enable_voice_lists(g, 1) before compile"));
    if (!g->compiled) return gfail(g, MLGPU_ERR_INVALID, std::string(who) + ": compile first");
    return MLGPU_OK;
  }
  int mlgpu_graph_reserve_voice_list(mlgpu_graph* g, size_t maxListed)
  {
    if (const int st = listsReady(g, "graph_reserve_voice_list")) return st;
    const int st = g->list.reserve(g->e, maxListed, "graph_reserve_voice_list");
    return st == MLGPU_OK ? st : gfail(g, st, g->e->lastError);
  }
  int mlgpu_graph_set_voice_list(mlgpu_graph* g, const uint32_t* h_voices, size_t n)
  {
    if (const int st = listsReady(g, "graph_set_voice_list")) return st;
    const int st = g->list.set(g->e, g->desc.V, h_voices, n, "graph_set_voice_list");
    return st == MLGPU_OK ? st : gfail(g, st, g->e->lastError);
  }
  size_t mlgpu_graph_voice_list_size(mlgpu_graph* g) { return (g && !g->job) ? g->list.size : 0; }

  // The first checks of the two listed events calls: the switch, the graph's event rows, the offset
  static int listedEventsCall(mlgpu_graph* g, const char* who, int startOffset)
  {
    if (!g) return MLGPU_ERR_INVALID;
    if (g->job) return MLGPU_ERR_BUSY;
    if (!g->desc.voiceListEvents)
      return gfail(g, MLGPU_ERR_INVALID, std::string(who) + ": the graph's event rows have no listed form - mlgpu_graph_enable_voice_list_events(g, 1) before compile");
    if (!g->desc.hasEventRows) return gfail(g, MLGPU_ERR_INVALID, std::string(who) + ": the graph has no event rows");
    if (startOffset < 0) return gfail(g, MLGPU_ERR_INVALID, std::string(who) + ": negative frame offset");
    return MLGPU_OK;
  }

  static int processListed(mlgpu_graph* g, const char* who, size_t T, int eventOffset, const float* const* d_inputs, int inLayout, const float* const* d_controls,
                           float* const* d_outputs, int outLayout, uint32_t* d_peak)
  {
    const auto w = [who] { return std::string(who); };  // (made where a refusal needs it: the success path allocates nothing)
    if (const int st = listsReady(g, who)) return st;
    if (g->desc.voiceListGroups)
      return gfail(g, MLGPU_ERR_INVALID, w() + ": the graph's listed kernel goes by the lane plan (mlgpu_graph_enable_voice_list_groups): mlgpu_" + w() + "_groups runs it");
    if (const int st = eventsReady(g, who, eventOffset, true)) return st;
    if (((uintptr_t)d_peak) & 3) return gfail(g, MLGPU_ERR_INVALID, w() + ": misaligned peaks");
    if (T == 0) return MLGPU_OK;
    if (eventOffset >= 0 && g->e->recording) return gfail(g, MLGPU_ERR_INVALID, w() + ": events route on the host: not while recording a sequence");
    GraphArgs a;
    if (const int st = signalArgs(g, a, who, T, d_inputs, inLayout, d_controls, d_outputs, outLayout)) return st;
    const size_t K = g->list.size;
    a.voiceList = g->list.d_list.get();
    a.listed = K;
    a.peaks = d_peak;
    // outputs by list position: K rows each; a mixed-down output is the tree of a K-voice graph
    if (const int st = outputViews(g, a, T, d_outputs, outLayout, K, 0,
                                   eventOffset < 0 ? "graph_process_listed: call mlgpu_graph_reserve_mixdown(graph, max vectors) at setup (process calls do not allocate)"
                                                   : "graph_process_events_listed: call mlgpu_graph_reserve_mixdown(graph, max vectors) at setup (process calls do not allocate)"))
      return st;
    if (hipSetDevice(g->e->device) != hipSuccess) return gfail(g, MLGPU_ERR_HIP, "hipSetDevice");
    void* eventStaging = nullptr;
    if (const int st = eventsPrepare(g, who, T, eventOffset, true, a, &eventStaging)) return st;
    if (K == 0)  // (no voice kernel to launch; the sum of no voices: +0.0)
    {
      if (const int st = eventsLaunched(g, who, eventStaging, hipSuccess)) return st;
      for (size_t o = 0; o < g->desc.outputs.size(); ++o)
        if (g->desc.outputMix[o] && hipMemsetAsync(d_outputs[o], 0, sizeof(float) * 64 * T, g->e->stream()) != hipSuccess)
          return gfail(g, MLGPU_ERR_HIP, w() + ": clearing a mixed-down output");
      return MLGPU_OK;
    }
    g->listedSinceClear = true;
    if (const int st = eventsLaunched(g, who, eventStaging, mlgpu_jit_launch(g->fnListed, &a, sizeof(a), K, g->e->stream()))) return st;
    return mixdownStages(g, T, d_outputs, K, who);
  }
  int mlgpu_graph_process_listed(mlgpu_graph* g, size_t T, const float* const* d_inputs, int inLayout, const float* const* d_controls, float* const* d_outputs,
                                 int outLayout, uint32_t* d_peak)
  {
    return processListed(g, "graph_process_listed", T, -1, d_inputs, inLayout, d_controls, d_outputs, outLayout, d_peak);
  }
  // a listed graph with event rows (mlgpu_graph_enable_voice_list_events): mlgpu_graph_process_events for the listed voices
  int mlgpu_graph_process_events_listed(mlgpu_graph* g, size_t T, int startOffset, const float* const* d_inputs, int inLayout, const float* const* d_controls,
                                        float* const* d_outputs, int outLayout, uint32_t* d_peak)
  {
    if (const int st = listedEventsCall(g, "graph_process_events_listed", startOffset)) return st;
    return processListed(g, "graph_process_events_listed", T, startOffset, d_inputs, inLayout, d_controls, d_outputs, outLayout, d_peak);
  }

  // ---- the listed voices with the group-summed outputs summed by instrument (voice_list.hpp plans the lanes, the planned form of the generated kernel runs them) ----
  int mlgpu_graph_reserve_voice_list_groups(mlgpu_graph* g, size_t maxListed)
  {
    if (const int st = listsReady(g, "graph_reserve_voice_list_groups", true)) return st;
    int G = 0;  // (planGraph: every group-summed output has this size, and there is one)
    for (size_t o = 0; o < g->desc.outputs.size(); ++o) G = g->desc.outputGroup[o] ? g->desc.outputGroup[o] : G;
    const int st = g->list.reserve(g->e, maxListed, "graph_reserve_voice_list_groups", G);
    return st == MLGPU_OK ? st : gfail(g, st, g->e->lastError);
  }
  size_t mlgpu_graph_listed_group_count(mlgpu_graph* g) { return (g && !g->job) ? g->list.planGroups : 0; }
  int mlgpu_graph_listed_groups(mlgpu_graph* g, uint32_t* h_groups, size_t capacity)
  {
    if (!g) return MLGPU_ERR_INVALID;
    if (g->job) return MLGPU_ERR_BUSY;
    std::string err;
    const int st = g->list.copyGroups(h_groups, capacity, "graph", err);
    return st == MLGPU_OK ? st : gfail(g, st, err);
  }

  static int processListedGroups(mlgpu_graph* g, const char* who, size_t T, int eventOffset, const float* const* d_inputs, int inLayout, const float* const* d_controls,
                                 float* const* d_outputs, int outLayout, uint32_t* d_peak)
  {
    const auto w = [who] { return std::string(who); };  // (made where a refusal needs it: the success path allocates nothing)
    if (const int st = listsReady(g, who, true)) return st;
    if (g->e->recording)
      return gfail(g, MLGPU_ERR_INVALID,
                   w() + ": not while recording a sequence - the launch's lane count and its rows go with the list's contents, not "
                       "only its length, so a recorded launch could not follow a later list");
    if (const int st = eventsReady(g, who, eventOffset, true)) return st;
    if (g->list.outGroup == 0) return gfail(g, MLGPU_ERR_INVALID, w() + ": call mlgpu_graph_reserve_voice_list_groups(graph, max listed voices) at setup");
    if (((uintptr_t)d_peak) & 3) return gfail(g, MLGPU_ERR_INVALID, w() + ": misaligned peaks");
    if (T == 0) return MLGPU_OK;
    GraphArgs a;
    if (const int st = signalArgs(g, a, who, T, d_inputs, inLayout, d_controls, d_outputs, outLayout)) return st;
    const size_t K = g->list.size, N = g->list.planLanes, J = g->list.planGroups;
    if (K == 0 && eventOffset < 0) return MLGPU_OK;  // (no listed instrument: no row to write)
    a.listed = N;
    a.lanePlan = g->list.d_plan.get();
    a.peaks = d_peak;
    // a group-summed output: J rows, one per listed instrument; every other output: K rows by list position (none is mixed down: planGraph)
    if (const int st = outputViews(g, a, T, d_outputs, outLayout, K, J, "")) return st;
    if (hipSetDevice(g->e->device) != hipSuccess) return gfail(g, MLGPU_ERR_HIP, "hipSetDevice");
    void* eventStaging = nullptr;
    if (const int st = eventsPrepare(g, who, T, eventOffset, true, a, &eventStaging)) return st;
    if (K == 0) return eventsLaunched(g, who, eventStaging, hipSuccess);  // (the events object advanced; no voice kernel)
    g->listedSinceClear = true;
    return eventsLaunched(g, who, eventStaging, mlgpu_jit_launch(g->fnListed, &a, sizeof(a), N, g->e->stream()));
  }
  int mlgpu_graph_process_listed_groups(mlgpu_graph* g, size_t T, const float* const* d_inputs, int inLayout, const float* const* d_controls, float* const* d_outputs,
                                        int outLayout, uint32_t* d_peak)
  {
    return processListedGroups(g, "graph_process_listed_groups", T, -1, d_inputs, inLayout, d_controls, d_outputs, outLayout, d_peak);
  }
  int mlgpu_graph_process_events_listed_groups(mlgpu_graph* g, size_t T, int startOffset, const float* const* d_inputs, int inLayout, const float* const* d_controls,
                                               float* const* d_outputs, int outLayout, uint32_t* d_peak)
  {
    if (const int st = listedEventsCall(g, "graph_process_events_listed_groups", startOffset)) return st;
    return processListedGroups(g, "graph_process_events_listed_groups", T, startOffset, d_inputs, inLayout, d_controls, d_outputs, outLayout, d_peak);
  }
}

// events.hip, mlgpu_events_destroy: no graph keeps a pointer to an events object that is gone
void mlgpu_graph_forget_events(mlgpu_events* ev)
{
  std::lock_guard<std::mutex> lock(g_boundMutex);
  for (auto it = g_boundGraphs.begin(); it != g_boundGraphs.end();)
  {
    if ((*it)->events == ev)
    {
      (*it)->events = nullptr;
      it = g_boundGraphs.erase(it);
    }
    else
      ++it;
  }
}
