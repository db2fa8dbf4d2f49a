// voice_records_plan_test.cpp — the host half of voice records (madronalib_amd/csrc/voice_records.cpp) without a device: a host model
// of the tables and of ring memory holds each word's own address, the planned gather and scatter are applied with plain loops, and the
// result is compared with a brute-force walk of the address map. Built with g++ -fsanitize=address,undefined from the planner's one
// file and run directly (tests/test_voice_records_cpu.py).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <set>
#include <vector>

#include "../../madronalib_amd/csrc/voice_records.hpp"

using namespace mlrec;
using mlupd::NodeDesc;
using mlupd::TableDesc;

static int failures = 0;
#define CHECK(cond, ...)                                        \
  do                                                            \
  {                                                             \
    if (!(cond))                                                \
    {                                                           \
      ++failures;                                               \
      printf("FAILED %s:%d: %s : ", __FILE__, __LINE__, #cond); \
      printf(__VA_ARGS__);                                      \
      printf("\n");                                             \
      if (failures > 20) exit(1);                               \
    }                                                           \
  } while (0)

// ---- the objects under test ----
struct Object
{
  TableDesc d;
  std::vector<NodeSig> sigs;
  int layout{0};
  size_t nParams{0}, nCoeffs{0}, nState{0}, memWords{0};
};

static void addParam(Object& o)
{
  NodeDesc nd;
  nd.kind = NodeDesc::PARAM;
  nd.paramRow = (int)o.nParams++;
  o.d.nodes.push_back(nd);
  o.sigs.push_back(NodeSig{1, 0, 0, 0});
}
static void addOther(Object& o)
{
  o.d.nodes.push_back(NodeDesc());
  o.sigs.push_back(NodeSig{0, 0, 0, 0});
}
static void addFeedback(Object& o)
{
  NodeDesc nd;
  nd.kind = NodeDesc::FEEDBACK;
  nd.sOff = (int)o.nState;
  nd.ns = 64;
  o.nState += 64;
  o.d.nodes.push_back(nd);
  o.sigs.push_back(NodeSig{8, 0, 0, 0});
}
static void addProc(Object& o, int kind, int nc, int ns, uint32_t ringLen = 0, uint32_t rings = 0)
{
  NodeDesc nd;
  nd.kind = NodeDesc::PROC;
  nd.cOff = (int)o.nCoeffs;
  nd.nc = nc;
  nd.sOff = (int)o.nState;
  nd.ns = ns;
  o.nCoeffs += (size_t)nc;
  o.nState += (size_t)ns;
  nd.rings = rings != 0;
  nd.ringWords = (uint64_t)ringLen * rings;
  nd.memOff = o.memWords;  // (words per voice so far: made into the memory's size by finish())
  o.memWords += nd.ringWords;
  o.d.nodes.push_back(nd);
  o.sigs.push_back(NodeSig{3, kind, ringLen, rings});
}
static void finish(Object& o, size_t V, int layout)
{
  o.layout = layout;
  o.d.V = V;
  o.d.ringGranule = layout == 0 ? 1u : layout == 2 ? 16u : 8u;
  o.d.memVoices = layout == 0 ? V : (V + 255) & ~(size_t)255;
  o.d.spareLanes = layout == 2 && o.memWords && (V % 64) != 0;
  o.memWords *= o.d.memVoices;
}

// a graph: a param, an input, a feedback node, a processor with coefficients and state, a delay node with one ring of `ringLen`, a
// second param, a delay node of `kind2` with two rings of 128, a processor without coefficients
static Object makeGraph(size_t V, int layout, uint32_t ringLen = 256, int kind2 = 41)
{
  Object o;
  addParam(o);
  addOther(o);
  addFeedback(o);
  addProc(o, 7, 3, 2);
  addProc(o, 40, 0, 5, ringLen, 1);
  addParam(o);
  addProc(o, kind2, 1, 10, 128, 2);
  addProc(o, 9, 0, 1);
  finish(o, V, layout);
  return o;
}
static Object makeBank(size_t V)
{
  Object o;
  o.d.bank = true;
  addProc(o, 1, 1, 2);
  addProc(o, 5, 3, 2);
  addProc(o, 2, 1, 0);
  finish(o, V, 0);
  return o;
}

// ---- the host model: every word holds its own address, tagged by where it lives ----
struct Model
{
  std::vector<uint32_t> tables[mlupd::kTables];
  std::vector<uint32_t> mem;
};
static uint32_t tag(uint32_t where, uint64_t index) { return (where << 28) | (uint32_t)index; }
static Model makeModel(const Object& o)
{
  Model m;
  const size_t rows[mlupd::kTables] = {o.nParams, o.nCoeffs, o.nState, o.d.bank ? (size_t)1 : 0};
  for (uint32_t t = 0; t < mlupd::kTables; ++t)
  {
    m.tables[t].resize(rows[t] * o.d.V);
    for (size_t i = 0; i < m.tables[t].size(); ++i) m.tables[t][i] = tag(t, i);
  }
  m.mem.resize(o.memWords);
  for (size_t i = 0; i < m.mem.size(); ++i) m.mem[i] = tag(kRing, i);
  return m;
}

// ---- the planned work, applied with plain loops (what voice_records_kernel does, item by item) ----
static void apply(const Object& o, const RecordPlan& plan, const std::vector<uint32_t>& upload, bool import, Model& m, std::vector<uint32_t>& records)
{
  const size_t nSeg = plan.segments().size(), W = plan.words(), V = o.d.V, G = plan.granule();
  const Segment* segs = (const Segment*)upload.data();
  const Entry* entries = (const Entry*)(upload.data() + nSeg * 8);
  CHECK(upload.size() == plan.uploadWords(), "%zu %zu", upload.size(), plan.uploadWords());
  for (size_t s = 0; s < nSeg; ++s)
    for (size_t e = 0; e < plan.entries(); ++e)
    {
      const Segment& sg = segs[s];
      const uint32_t slot = entries[e].slot;
      CHECK((size_t)entries[e].record * W + W <= records.size(), "record %u", entries[e].record);
      uint32_t* rec = records.data() + (size_t)entries[e].record * W + sg.recOff;
      for (uint32_t r = 0; r < sg.rows; ++r)
      {
        uint32_t* own = nullptr;
        if (sg.where < kRing)
        {
          if (slot >= V) continue;
          own = &m.tables[sg.where][(size_t)r * V + slot];
        }
        else
        {
          const uint64_t at = G == 1 ? sg.base + (uint64_t)r * V + slot : sg.base + (uint64_t)(slot >> 8) * sg.rows * 256u + (uint64_t)(slot & 255u) * G + (uint64_t)(r / G) * 256u * G + r % G;
          CHECK(G != 1 || slot < V, "slot %u in layout 0", slot);
          CHECK(at < m.mem.size(), "ring word %llu of %zu", (unsigned long long)at, m.mem.size());
          if (at >= m.mem.size()) continue;
          own = &m.mem[at];
        }
        if (import)
          *own = rec[r];
        else
          rec[r] = *own;
      }
    }
}

// ---- the brute-force walk: the record of voice slot `v`, word by word, from the address map alone; pads are kNone ----
static const uint32_t kNone = 0xffffffffu;
static std::vector<uint32_t> expectedRecord(const Object& o, size_t v, bool tablesToo)
{
  std::vector<uint32_t> r;
  const size_t V = o.d.V, G = o.d.ringGranule;
  for (size_t row = 0; row < o.nParams; ++row) r.push_back(tablesToo ? tag(0, row * V + v) : kNone);
  for (size_t row = 0; row < o.nCoeffs; ++row) r.push_back(tablesToo ? tag(1, row * V + v) : kNone);
  for (size_t row = 0; row < o.nState; ++row) r.push_back(tablesToo ? tag(2, row * V + v) : kNone);
  if (o.d.bank) r.push_back(tablesToo ? tag(3, v) : kNone);
  while (r.size() % 4) r.push_back(kNone);
  for (const NodeDesc& nd : o.d.nodes)
  {
    if (!nd.rings || !nd.ringWords) continue;
    if (G == 1)
      for (uint64_t row = 0; row < nd.ringWords; ++row) r.push_back(tag(kRing, nd.memOff * V + row * V + v));
    else
      for (uint64_t k = 0; k < nd.ringWords / G; ++k)
        for (uint64_t j = 0; j < G; ++j) r.push_back(tag(kRing, nd.memOff * o.d.memVoices + (uint64_t)(v >> 8) * nd.ringWords * 256u + (uint64_t)(v & 255u) * G + k * 256u * G + j));
  }
  while (r.size() % 4) r.push_back(kNone);
  return r;
}

static void checkObject(const Object& o, const std::vector<uint32_t>& voices, const char* what)
{
  RecordPlan plan;
  CHECK(plan.describe(o.d, o.sigs, o.layout, 3), "%s: %s", what, plan.error());
  const size_t W = plan.words(), n = voices.size(), V = o.d.V;
  CHECK(W % 4 == 0 && W == expectedRecord(o, 0, true).size(), "%s: W %zu", what, W);
  // every word of the object belongs to exactly one voice slot (the map is a bijection): no record can hold another voice's word
  {
    std::set<uint32_t> all;
    size_t count = 0;
    const size_t slots = o.d.spareLanes ? (V + 63) & ~(size_t)63 : V;
    for (size_t v = 0; v < slots; ++v)
      for (uint32_t w : expectedRecord(o, v, v < V))
        if (w != kNone) all.insert(w), ++count;
    CHECK(all.size() == count, "%s: the address map gives a word to two voices", what);
  }

  // export: repeats allowed, the voice's own words only
  std::vector<uint32_t> twice = voices;
  twice.insert(twice.end(), voices.begin(), voices.end());
  CHECK(plan.validate(twice.data(), twice.size(), false) == MLGPU_OK, "%s: %s", what, plan.error());
  CHECK(plan.entries() == twice.size(), "%s: export entries %zu", what, plan.entries());
  std::vector<uint32_t> upload(plan.uploadWords());
  plan.pack(twice.data(), twice.size(), false, upload.data());
  Model m = makeModel(o);
  const Model untouched = m;
  std::vector<uint32_t> records(twice.size() * W, kNone);
  apply(o, plan, upload, false, m, records);
  for (size_t i = 0; i < twice.size(); ++i)
  {
    const std::vector<uint32_t> want = expectedRecord(o, twice[i], true);
    CHECK(memcmp(want.data(), records.data() + i * W, 4 * W) == 0, "%s: export, record %zu (voice %u)", what, i, twice[i]);
    std::set<uint32_t> once;
    for (size_t w = 0; w < W; ++w)
      if (want[w] != kNone) CHECK(once.insert(records[i * W + w]).second, "%s: a word twice in record %zu", what, i);
  }
  for (uint32_t t = 0; t < mlupd::kTables; ++t) CHECK(m.tables[t] == untouched.tables[t], "%s: export wrote table %u", what, t);
  CHECK(m.mem == untouched.mem, "%s: export wrote ring memory", what);

  // import: distinct voices; exactly the listed voices' words change, plus the spare lanes' for voice V - 1 in layout 2
  CHECK(plan.validate(voices.data(), n, true) == MLGPU_OK, "%s: %s", what, plan.error());
  bool last = false;
  for (uint32_t v : voices) last |= v == V - 1;
  const size_t spare = (o.d.spareLanes && last) ? ((V + 63) & ~(size_t)63) - V : 0;
  CHECK(plan.entries() == n + spare, "%s: import entries %zu, %zu voices + %zu spare lanes", what, plan.entries(), n, spare);
  CHECK(plan.entries() <= RecordPlan::maxEntries(n), "%s: more entries than a reserve holds", what);
  upload.assign(plan.uploadWords(), 0);
  plan.pack(voices.data(), n, true, upload.data());
  records.assign(n * W, 0);
  for (size_t i = 0; i < records.size(); ++i) records[i] = 0x80000000u | (uint32_t)i;
  const std::vector<uint32_t> recordsBefore = records;
  m = makeModel(o);
  apply(o, plan, upload, true, m, records);
  CHECK(records == recordsBefore, "%s: import wrote the records", what);
  std::map<uint32_t, uint32_t> want;  // a word's tag -> the record word it must hold now
  for (size_t i = 0; i < n; ++i)
  {
    const std::vector<uint32_t> own = expectedRecord(o, voices[i], true);
    for (size_t w = 0; w < W; ++w)
      if (own[w] != kNone) want[own[w]] = records[i * W + w];
    if (spare && voices[i] == V - 1)
      for (size_t s = V; s < V + spare; ++s)
      {
        const std::vector<uint32_t> lane = expectedRecord(o, s, false);
        for (size_t w = 0; w < W; ++w)
          if (lane[w] != kNone) want[lane[w]] = records[i * W + w];
      }
  }
  size_t changed = 0;
  for (uint32_t t = 0; t < mlupd::kTables; ++t)
    for (size_t i = 0; i < m.tables[t].size(); ++i)
    {
      const auto it = want.find(tag(t, i));
      const uint32_t expect = it == want.end() ? tag(t, i) : it->second;
      changed += it != want.end();
      CHECK(m.tables[t][i] == expect, "%s: import, table %u word %zu", what, t, i);
    }
  for (size_t i = 0; i < m.mem.size(); ++i)
  {
    const auto it = want.find(tag(kRing, i));
    const uint32_t expect = it == want.end() ? tag(kRing, i) : it->second;
    changed += it != want.end();
    CHECK(m.mem[i] == expect, "%s: import, ring word %zu", what, i);
  }
  CHECK(changed == want.size() && changed >= n * plan.tableWords(), "%s: %zu words changed, %zu wanted", what, changed, want.size());
}

static uint64_t signatureOf(const Object& o, int revision = 3)
{
  RecordPlan p;
  CHECK(p.describe(o.d, o.sigs, o.layout, revision), "%s", p.error());
  return p.signature();
}

int main()
{
  const std::vector<uint32_t> S600 = {255, 256, 599, 250, 251, 252, 253, 254, 257, 258, 259};
  const std::vector<uint32_t> S80 = {79, 60, 61, 62, 63, 64, 65, 66, 67, 68, 69, 0};
  const int layouts[] = {0, 1, 2, 4};  // granules 1, 8, 16, 8
  for (int layout : layouts)
  {
    char what[64];
    snprintf(what, sizeof(what), "graph, layout %d, 600 voices", layout);
    checkObject(makeGraph(600, layout), S600, what);
    snprintf(what, sizeof(what), "graph, layout %d, 80 voices", layout);
    checkObject(makeGraph(80, layout), S80, what);
    snprintf(what, sizeof(what), "graph, layout %d, 80 voices, one voice", layout);
    checkObject(makeGraph(80, layout), {17}, what);
    snprintf(what, sizeof(what), "graph, layout %d, 64 voices, all", layout);
    std::vector<uint32_t> all(64);
    for (uint32_t v = 0; v < 64; ++v) all[v] = 63 - v;
    checkObject(makeGraph(64, layout), all, what);
  }
  checkObject(makeBank(80), S80, "bank, 80 voices");
  checkObject(makeBank(2352), {2351, 0, 255, 256, 1024}, "bank, 2352 voices");
  {
    RecordPlan p;
    const Object b = makeBank(80);
    CHECK(p.describe(b.d, b.sigs, 0, 3) && p.words() == 12 && p.tableWords() == 5 + 4 + 1 && p.segments().size() == 3, "bank layout: W %zu", p.words());
    const Object g = makeGraph(600, 4);
    CHECK(p.describe(g.d, g.sigs, 4, 3) && p.tableWords() == 2 + 4 + 64 + 18 && p.words() == 88 + 256 + 256 && p.granule() == 8, "graph layout: W %zu", p.words());
    CHECK(p.segments().size() == 5 && p.segments()[3].recOff == 88 && p.segments()[4].recOff == 344 && p.segments()[4].base == 256u * 768u, "graph segments");
  }

  // the signature: equal across the number of voices, different across ring layout, node kind, ring length, revision, bank / graph
  CHECK(signatureOf(makeGraph(80, 4)) == signatureOf(makeGraph(600, 4)), "signature depends on V");
  CHECK(signatureOf(makeGraph(80, 0)) == signatureOf(makeGraph(262144, 0)), "signature depends on V");
  CHECK(signatureOf(makeGraph(80, 4)) != signatureOf(makeGraph(80, 1)), "signature: ring layout");
  CHECK(signatureOf(makeGraph(80, 4)) != signatureOf(makeGraph(80, 2)), "signature: ring layout");
  CHECK(signatureOf(makeGraph(80, 4)) != signatureOf(makeGraph(80, 0)), "signature: ring layout");
  CHECK(signatureOf(makeGraph(80, 4)) != signatureOf(makeGraph(80, 4, 512)), "signature: ring length");
  CHECK(signatureOf(makeGraph(80, 4)) != signatureOf(makeGraph(80, 4, 256, 42)), "signature: node kind");
  CHECK(signatureOf(makeGraph(80, 4)) != signatureOf(makeGraph(80, 4), 4), "signature: behaviour revision");
  CHECK(signatureOf(makeBank(80)) == signatureOf(makeBank(2352)) && signatureOf(makeBank(80)) != signatureOf(makeGraph(80, 0)), "signature: banks");

  // the refusals, and that a refused import leaves the distinctness scratch clean
  {
    const Object g = makeGraph(80, 2);
    RecordPlan p;
    const uint32_t ok[3] = {79, 3, 5}, high[3] = {1, 80, 2}, twice[4] = {4, 9, 70, 9};
    CHECK(p.validate(ok, 3, false) == MLGPU_ERR_INVALID, "not described");
    CHECK(p.describe(g.d, g.sigs, 2, 3), "%s", p.error());
    CHECK(p.validate(nullptr, 0, true) == MLGPU_OK && p.entries() == 0, "n == 0");
    CHECK(p.validate(nullptr, 3, false) == MLGPU_ERR_INVALID, "null list");
    CHECK(p.validate(high, 3, false) == MLGPU_ERR_RANGE && p.validate(high, 3, true) == MLGPU_ERR_RANGE && strstr(p.error(), "position 1"), "%s", p.error());
    CHECK(p.validate(twice, 4, false) == MLGPU_OK && p.entries() == 4, "export takes repeats");
    CHECK(p.validate(twice, 4, true) == MLGPU_ERR_INVALID && strstr(p.error(), "position 3") && p.entries() == 0, "%s", p.error());
    CHECK(p.validate(twice, 3, true) == MLGPU_OK && p.entries() == 3, "after a refusal: %s", p.error());
    CHECK(p.validate(twice, 3, true) == MLGPU_OK, "the same import twice: %s", p.error());
    CHECK(p.validate(ok, 3, true) == MLGPU_OK && p.entries() == 3 + 48, "spare lanes: %zu", p.entries());
    CHECK(p.validate(ok, 3, false) == MLGPU_OK && p.entries() == 3, "export has no spare lanes: %zu", p.entries());
    Object bad = makeGraph(80, 4);
    bad.d.nodes[4].ringWords = 250;  // (no multiple of the granule)
    CHECK(!p.describe(bad.d, bad.sigs, 4, 3) && !p.described() && p.words() == 0, "a ring that is no multiple of the granule");
    bad = makeGraph(80, 4);
    bad.sigs.pop_back();
    CHECK(!p.describe(bad.d, bad.sigs, 4, 3), "a description without every node's signature entry");
  }
  if (failures) return 1;
  printf("All tests passed\n");
  return 0;
}
