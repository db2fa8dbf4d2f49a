// tests/cpp/param_updates_test.cpp — the host planner of sparse per-voice table updates (madronalib_amd/csrc/param_updates.cpp) on
// its own: built with g++ -fsanitize=address,undefined from that one file, no HIP header on the include path
// (tests/test_param_updates_cpu.py). Hand-written lists go in, the packed device records and batch cuts come out and are compared
// with lists written down by hand: (table, row, first, count, bits). Then random lists, replayed batch by batch on host tables
// against the naive model "apply the records one at a time, in list order".
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../madronalib_amd/csrc/param_updates.hpp"

using namespace mlupd;

static int failures = 0;
#define REQUIRE(cond)                                             \
  do                                                              \
  {                                                               \
    if (!(cond))                                                  \
    {                                                             \
      printf("REQUIRE failed at line %d: %s\n", __LINE__, #cond); \
      ++failures;                                                 \
    }                                                             \
  } while (0)

struct R
{
  uint32_t table, row, first, count, bits;
  bool operator==(const R& o) const { return table == o.table && row == o.row && first == o.first && count == o.count && bits == o.bits; }
};
typedef std::vector<R> Rs;

static mlgpu_update upd(int node, int target, int index, uint32_t first, uint32_t count, uint32_t bits)
{
  mlgpu_update u{};
  u.node = node;
  u.target = (uint16_t)target;
  u.index = (uint16_t)index;
  u.first_voice = first;
  u.n_voices = count;
  u.bits = bits;
  return u;
}

static NodeDesc param(int row)
{
  NodeDesc n;
  n.kind = NodeDesc::PARAM;
  n.paramRow = row;
  return n;
}
static NodeDesc proc(int cOff, int nc, int sOff, int ns, std::vector<uint32_t> clearWords = {}, std::vector<uint8_t> clearMask = {})
{
  NodeDesc n;
  n.kind = NodeDesc::PROC;
  n.cOff = cOff;
  n.nc = nc;
  n.sOff = sOff;
  n.ns = ns;
  n.clearWords = clearWords.empty() ? std::vector<uint32_t>((size_t)ns, 0u) : clearWords;
  n.clearMask = clearMask.empty() ? std::vector<uint8_t>((size_t)ns, 1) : clearMask;
  return n;
}
static NodeDesc feedback(int sOff)
{
  NodeDesc n;
  n.kind = NodeDesc::FEEDBACK;
  n.sOff = sOff;
  n.ns = 64;
  n.clearWords.assign(64, 0u);
  n.clearMask.assign(64, 1);
  return n;
}

// The graph of the hand-written cases, V = 100. State rows: SineGen 0, TempoLock 1-3, LinearGlide 4-71, feedback 72-135, Lopass
// 136-137, the delay none.
enum { IN = 0, PITCH, CUTOFF, SINE, TEMPO, GLIDE, FB, LOPASS, DELAY, OP };
static TableDesc graphDesc()
{
  TableDesc d;
  d.V = 100;
  d.nodes.resize(10);
  d.nodes[PITCH] = param(0);
  d.nodes[CUTOFF] = param(1);
  d.nodes[SINE] = proc(0, 0, 0, 1, {0xC0000000u});                         // SineGen::clear(): kZeroPhase
  d.nodes[TEMPO] = proc(0, 0, 1, 3, {0xBF800000u, 0u, 0u}, {1, 0, 0});     // TempoLock::clear(): _omega = -1, nothing else
  std::vector<uint32_t> glide(68, 0u);
  glide[2] = 0xFFFFFFFFu;                                                  // LinearGlide: mVectorsRemaining = -1
  d.nodes[GLIDE] = proc(0, 2, 4, 68, glide);
  d.nodes[FB] = feedback(72);
  d.nodes[LOPASS] = proc(2, 3, 136, 2);
  d.nodes[DELAY] = proc(5, 0, 138, 0);
  return d;
}

struct Packed
{
  int status;
  Rs recs;
  std::vector<size_t> ends;
  std::string error;
};
// validate + pack into a buffer of exactly the announced size, framed by guard records that must survive
static Packed run(UpdatePlanner& p, const TableDesc& d, const std::vector<mlgpu_update>& list)
{
  Packed out;
  out.status = p.validate(d, list.data(), list.size());
  out.error = p.error();
  const DevRec guard{0xDEADBEEFu, 1u, 2u, 3u};
  if (out.status != MLGPU_OK)
  {
    REQUIRE(p.deviceRecords() == 0);
    return out;
  }
  std::vector<DevRec> buf(p.deviceRecords() + 2, guard);
  p.pack(d, list.data(), list.size(), buf.data() + 1);
  REQUIRE(!memcmp(&buf.front(), &guard, sizeof(guard)) && !memcmp(&buf.back(), &guard, sizeof(guard)));
  for (size_t i = 1; i + 1 < buf.size(); ++i) out.recs.push_back(R{buf[i].tableRow >> kRowBits, buf[i].tableRow & kRowMask, buf[i].first, buf[i].count, buf[i].bits});
  for (size_t b = 0; b < p.batches(); ++b) out.ends.push_back(p.batchEnd(b));
  return out;
}

static void handWritten()
{
  UpdatePlanner p;
  const TableDesc d = graphDesc();
  static_assert(sizeof(DevRec) == 16, "one dwordx4 load per record");
  static_assert(sizeof(mlgpu_update) == 20, "the C ABI's record");

  // single records of every graph target
  Packed r = run(p, d, {upd(CUTOFF, MLGPU_UPDATE_PARAM, 7 /* ignored */, 16, 16, 0x3F000000u)});
  REQUIRE(r.status == MLGPU_OK && r.recs == Rs({{TABLE_PARAMS, 1, 16, 16, 0x3F000000u}}) && r.ends == std::vector<size_t>({1}));
  r = run(p, d, {upd(LOPASS, MLGPU_UPDATE_COEFF, 2, 99, 1, 0x80000000u)});
  REQUIRE(r.status == MLGPU_OK && r.recs == Rs({{TABLE_COEFFS, 4, 99, 1, 0x80000000u}}) && r.ends == std::vector<size_t>({1}));
  r = run(p, d, {upd(FB, MLGPU_UPDATE_STATE, 63, 0, 100, 0x7FC00001u)});
  REQUIRE(r.status == MLGPU_OK && r.recs == Rs({{TABLE_STATE, 135, 0, 100, 0x7FC00001u}}) && r.ends == std::vector<size_t>({1}));
  r = run(p, d, {});
  REQUIRE(r.status == MLGPU_OK && r.recs.empty() && r.ends.empty());

  // CLEAR: one device record per state word clear() resets
  r = run(p, d, {upd(SINE, MLGPU_UPDATE_CLEAR, 0, 64, 16, 0x12345678u /* ignored */)});
  REQUIRE(r.status == MLGPU_OK && r.recs == Rs({{TABLE_STATE, 0, 64, 16, 0xC0000000u}}));
  r = run(p, d, {upd(TEMPO, MLGPU_UPDATE_CLEAR, 0, 3, 2, 0)});
  REQUIRE(r.status == MLGPU_OK && r.recs == Rs({{TABLE_STATE, 1, 3, 2, 0xBF800000u}}));
  r = run(p, d, {upd(GLIDE, MLGPU_UPDATE_CLEAR, 0, 10, 5, 0)});
  REQUIRE(r.status == MLGPU_OK && r.recs.size() == 68 && r.ends == std::vector<size_t>({68}));
  for (size_t i = 0; i < r.recs.size(); ++i) REQUIRE(r.recs[i] == (R{TABLE_STATE, (uint32_t)(4 + i), 10, 5, i == 2 ? 0xFFFFFFFFu : 0u}));
  r = run(p, d, {upd(DELAY, MLGPU_UPDATE_CLEAR, 0, 0, 100, 0)});  // (no state words: nothing to do, no batch)
  REQUIRE(r.status == MLGPU_OK && r.recs.empty() && r.ends.empty());
  // node = -1: every processor and feedback node, in node order: 1 + 1 + 68 + 64 + 2 records
  const std::vector<mlgpu_update> all = {upd(-1, MLGPU_UPDATE_CLEAR, 0, 64, 16, 0)};
  r = run(p, d, all);
  REQUIRE(r.status == MLGPU_OK && r.recs.size() == 136 && r.ends == std::vector<size_t>({136}));
  REQUIRE(r.recs[0] == (R{TABLE_STATE, 0, 64, 16, 0xC0000000u}) && r.recs[1] == (R{TABLE_STATE, 1, 64, 16, 0xBF800000u}));
  REQUIRE(r.recs[2] == (R{TABLE_STATE, 4, 64, 16, 0u}) && r.recs[4] == (R{TABLE_STATE, 6, 64, 16, 0xFFFFFFFFu}));
  REQUIRE(r.recs[70] == (R{TABLE_STATE, 72, 64, 16, 0u}) && r.recs[134] == (R{TABLE_STATE, 136, 64, 16, 0u}) && r.recs[135] == (R{TABLE_STATE, 137, 64, 16, 0u}));
  // what a list costs against the reserve is what pack produces
  REQUIRE(p.validate(d, all.data(), all.size()) == MLGPU_OK && p.deviceRecords() == 136);

  // overlap cutting: A, B, A' with A' over A: two batches, A' in the second
  const mlgpu_update A = upd(PITCH, MLGPU_UPDATE_PARAM, 0, 32, 16, 1), B = upd(CUTOFF, MLGPU_UPDATE_PARAM, 0, 32, 16, 2), A2 = upd(PITCH, MLGPU_UPDATE_PARAM, 0, 47, 4, 3);
  r = run(p, d, {A, B, A2});
  REQUIRE(r.status == MLGPU_OK && r.ends == std::vector<size_t>({2, 3}));
  REQUIRE(r.recs == Rs({{TABLE_PARAMS, 0, 32, 16, 1}, {TABLE_PARAMS, 1, 32, 16, 2}, {TABLE_PARAMS, 0, 47, 4, 3}}));
  // ... next to each other is not over each other, in any list order
  r = run(p, d, {upd(PITCH, MLGPU_UPDATE_PARAM, 0, 48, 4, 3), B, A});
  REQUIRE(r.status == MLGPU_OK && r.ends == std::vector<size_t>({3}));
  // a long record over short ones that do not touch each other; the same row of another table is another row
  r = run(p, d, {upd(SINE, MLGPU_UPDATE_STATE, 0, 10, 2, 1), upd(SINE, MLGPU_UPDATE_STATE, 0, 20, 2, 2), upd(PITCH, MLGPU_UPDATE_PARAM, 0, 0, 100, 9),
                 upd(SINE, MLGPU_UPDATE_STATE, 0, 0, 100, 3), upd(SINE, MLGPU_UPDATE_STATE, 0, 11, 1, 4), upd(SINE, MLGPU_UPDATE_STATE, 0, 11, 1, 5)});
  REQUIRE(r.status == MLGPU_OK && r.ends == std::vector<size_t>({3, 4, 5, 6}));
  // a CLEAR's words and STATE records of them: the cuts fall between device records (row 137 twice, then row 136 twice)
  r = run(p, d, {upd(LOPASS, MLGPU_UPDATE_STATE, 1, 70, 1, 7), upd(LOPASS, MLGPU_UPDATE_CLEAR, 0, 64, 16, 0), upd(LOPASS, MLGPU_UPDATE_STATE, 0, 64, 1, 8)});
  REQUIRE(r.status == MLGPU_OK && r.recs.size() == 4 && r.ends == std::vector<size_t>({2, 4}));

  // refusals: status, a message naming the record's position, nothing written
  struct Bad
  {
    mlgpu_update u;
    int status;
  };
  const Bad bad[] = {
      {upd(IN, MLGPU_UPDATE_PARAM, 0, 0, 1, 0), MLGPU_ERR_INVALID},       // a node of the wrong type ...
      {upd(LOPASS, MLGPU_UPDATE_PARAM, 0, 0, 1, 0), MLGPU_ERR_INVALID},
      {upd(PITCH, MLGPU_UPDATE_COEFF, 0, 0, 1, 0), MLGPU_ERR_INVALID},
      {upd(FB, MLGPU_UPDATE_COEFF, 0, 0, 1, 0), MLGPU_ERR_INVALID},
      {upd(OP, MLGPU_UPDATE_STATE, 0, 0, 1, 0), MLGPU_ERR_INVALID},
      {upd(PITCH, MLGPU_UPDATE_CLEAR, 0, 0, 1, 0), MLGPU_ERR_INVALID},
      {upd(10, MLGPU_UPDATE_STATE, 0, 0, 1, 0), MLGPU_ERR_RANGE},         // ... or no node at all
      {upd(-1, MLGPU_UPDATE_STATE, 0, 0, 1, 0), MLGPU_ERR_RANGE},
      {upd(-2, MLGPU_UPDATE_CLEAR, 0, 0, 1, 0), MLGPU_ERR_RANGE},
      {upd(LOPASS, MLGPU_UPDATE_COEFF, 3, 0, 1, 0), MLGPU_ERR_RANGE},     // an index beyond nc / ns
      {upd(GLIDE, MLGPU_UPDATE_COEFF, 2, 0, 1, 0), MLGPU_ERR_RANGE},
      {upd(DELAY, MLGPU_UPDATE_COEFF, 0, 0, 1, 0), MLGPU_ERR_RANGE},
      {upd(LOPASS, MLGPU_UPDATE_STATE, 2, 0, 1, 0), MLGPU_ERR_RANGE},
      {upd(FB, MLGPU_UPDATE_STATE, 64, 0, 1, 0), MLGPU_ERR_RANGE},
      {upd(SINE, MLGPU_UPDATE_STATE, 0xFFFF, 0, 1, 0), MLGPU_ERR_RANGE},
      {upd(PITCH, MLGPU_UPDATE_PARAM, 0, 100, 1, 0), MLGPU_ERR_RANGE},    // a range beyond V
      {upd(PITCH, MLGPU_UPDATE_PARAM, 0, 99, 2, 0), MLGPU_ERR_RANGE},
      {upd(PITCH, MLGPU_UPDATE_PARAM, 0, 0, 101, 0), MLGPU_ERR_RANGE},
      {upd(PITCH, MLGPU_UPDATE_PARAM, 0, 0xFFFFFFFFu, 2, 0), MLGPU_ERR_RANGE},  // (first + count wraps in 32 bits)
      {upd(-1, MLGPU_UPDATE_CLEAR, 0, 90, 11, 0), MLGPU_ERR_RANGE},
      {upd(PITCH, MLGPU_UPDATE_PARAM, 0, 5, 0, 0), MLGPU_ERR_INVALID},    // n_voices == 0
      {upd(-1, MLGPU_UPDATE_CLEAR, 0, 5, 0, 0), MLGPU_ERR_INVALID},
      {upd(0, MLGPU_UPDATE_INPUT_CONST, 0, 0, 1, 0), MLGPU_ERR_INVALID},  // INPUT_CONST on a graph
      {upd(PITCH, 5, 0, 0, 1, 0), MLGPU_ERR_INVALID},                     // no such target
  };
  for (const Bad& b : bad)
  {
    // the bad record third of four: the good ones around it must not get anywhere either
    r = run(p, d, {A, B, b.u, A2});
    REQUIRE(r.status == b.status);
    REQUIRE(r.error.find("record 2 of 4") != std::string::npos);
    REQUIRE(r.recs.empty() && r.ends.empty());
  }
  // a node with delay rings: CLEAR of it, and of every node of a graph that has one
  TableDesc rings = d;
  rings.nodes[DELAY].rings = true;
  r = run(p, rings, {A, upd(DELAY, MLGPU_UPDATE_CLEAR, 0, 0, 1, 0)});
  REQUIRE(r.status == MLGPU_ERR_UNSUPPORTED && r.error.find("record 1 of 2") != std::string::npos && r.error.find("rings") != std::string::npos);
  r = run(p, rings, {upd(-1, MLGPU_UPDATE_CLEAR, 0, 0, 1, 0)});
  REQUIRE(r.status == MLGPU_ERR_UNSUPPORTED && r.error.find("record 0 of 1") != std::string::npos);
  r = run(p, rings, {upd(SINE, MLGPU_UPDATE_CLEAR, 0, 0, 1, 0), upd(DELAY, MLGPU_UPDATE_COEFF, 0, 0, 1, 0)});  // (its other nodes clear; its tables update - here nc = 0)
  REQUIRE(r.status == MLGPU_ERR_RANGE);

  // a bank: node = processor index, an input-const table, no params
  TableDesc bank;
  bank.bank = true;
  bank.V = 80;
  bank.nodes = {proc(0, 0, 0, 2), proc(0, 3, 2, 2), proc(3, 1, 4, 0)};  // SawGen, Bandpass, Gain
  r = run(p, bank, {upd(1, MLGPU_UPDATE_COEFF, 2, 64, 16, 5), upd(2, MLGPU_UPDATE_COEFF, 0, 0, 80, 6), upd(0, MLGPU_UPDATE_STATE, 1, 79, 1, 7),
                    upd(123, MLGPU_UPDATE_INPUT_CONST, 9, 60, 10, 8), upd(-1, MLGPU_UPDATE_CLEAR, 0, 0, 1, 0)});
  REQUIRE(r.status == MLGPU_OK && r.ends == std::vector<size_t>({8}));  // (Gain has no state: 2 + 2 words cleared)
  REQUIRE(r.recs == Rs({{TABLE_COEFFS, 2, 64, 16, 5}, {TABLE_COEFFS, 3, 0, 80, 6}, {TABLE_STATE, 1, 79, 1, 7}, {TABLE_INPUT_CONST, 0, 60, 10, 8},
                        {TABLE_STATE, 0, 0, 1, 0}, {TABLE_STATE, 1, 0, 1, 0}, {TABLE_STATE, 2, 0, 1, 0}, {TABLE_STATE, 3, 0, 1, 0}}));
  r = run(p, bank, {upd(0, MLGPU_UPDATE_PARAM, 0, 0, 1, 0)});  // PARAM on a bank
  REQUIRE(r.status == MLGPU_ERR_INVALID && r.error.find("record 0 of 1") != std::string::npos);
  r = run(p, bank, {upd(3, MLGPU_UPDATE_COEFF, 0, 0, 1, 0)});
  REQUIRE(r.status == MLGPU_ERR_RANGE);
  r = run(p, bank, {upd(0, MLGPU_UPDATE_INPUT_CONST, 0, 79, 2, 0)});
  REQUIRE(r.status == MLGPU_ERR_RANGE);
}

// 2 000 random lists on a small graph (so that overlaps are common), replayed batch by batch - within a batch in REVERSE, which
// leaves the same words only if no two records of the batch share one - against the records applied in list order
static void randomLists()
{
  uint32_t seed = 2463534242u;
  auto rnd = [&](uint32_t n) {
    seed ^= seed << 13;
    seed ^= seed >> 17;
    seed ^= seed << 5;
    return seed % n;
  };
  UpdatePlanner p;
  p.reserve(64);  // (less than most lists need: the planner's own vectors grow like the caller's buffers without a reserve)
  for (int trial = 0; trial < 2000; ++trial)
  {
    TableDesc d;
    d.V = 1 + rnd(trial % 4 == 0 ? 300 : 24);
    d.bank = trial % 5 == 4;
    const int nNodes = 1 + (int)rnd(6);
    int nParams = 0, NC = 0, NS = 0;
    for (int i = 0; i < nNodes; ++i)
    {
      const uint32_t k = d.bank ? 1 : rnd(4);
      if (k == 0)
        d.nodes.push_back(param(nParams++));
      else if (k == 3)
      {
        d.nodes.push_back(feedback(NS));
        NS += 64;
      }
      else
      {
        const int nc = (int)rnd(4), ns = (int)rnd(5);
        std::vector<uint32_t> words;
        std::vector<uint8_t> mask;
        for (int w = 0; w < ns; ++w)
        {
          words.push_back(rnd(3) ? 0u : 0xC0000000u + rnd(9));
          mask.push_back((uint8_t)(rnd(4) != 0));
        }
        NodeDesc n = proc(NC, nc, NS, ns, words, mask);
        if (!ns) n.clearWords.clear(), n.clearMask.clear();
        d.nodes.push_back(n);
        NC += nc;
        NS += ns;
      }
    }
    const size_t rows[kTables] = {(size_t)nParams, (size_t)NC, (size_t)NS, d.bank ? 1u : 0u};
    std::vector<uint32_t> naive[kTables], got[kTables];
    for (uint32_t t = 0; t < kTables; ++t) naive[t].assign(rows[t] * d.V, 0xAAAA0000u + t), got[t] = naive[t];

    std::vector<mlgpu_update> list;
    const size_t n = rnd(trial % 10 == 0 ? 400 : 40);
    while (list.size() < n)
    {
      const int node = rnd(12) == 0 ? -1 : (int)rnd((uint32_t)nNodes);
      const uint32_t first = rnd((uint32_t)d.V), count = 1 + rnd(rnd(3) ? 4 : (uint32_t)d.V);
      mlgpu_update u = upd(node, (int)rnd(5), (int)rnd(5), first, std::min<uint32_t>(count, (uint32_t)d.V - first), 0x1000u + (uint32_t)list.size());
      if (rnd(16) == 0 && node >= 0 && d.nodes[(size_t)node].kind == NodeDesc::FEEDBACK) u.index = (uint16_t)rnd(64);
      UpdatePlanner probe;
      if (probe.validate(d, &u, 1) != MLGPU_OK) continue;  // (the refusals have their own cases above)
      list.push_back(u);
      // the naive model: this record now, word by word
      std::vector<DevRec> one(probe.deviceRecords());
      probe.pack(d, &u, 1, one.data());
      for (const DevRec& r : one)
        for (uint32_t v = 0; v < r.count; ++v) naive[r.tableRow >> kRowBits][(size_t)(r.tableRow & kRowMask) * d.V + r.first + v] = r.bits;
    }
    REQUIRE(p.validate(d, list.data(), list.size()) == MLGPU_OK);
    std::vector<DevRec> recs(p.deviceRecords());
    p.pack(d, list.data(), list.size(), recs.data());
    size_t begin = 0, total = 0;
    for (size_t b = 0; b < p.batches(); ++b)
    {
      const size_t end = p.batchEnd(b);
      REQUIRE(end > begin && end <= recs.size());
      for (size_t i = end; i-- > begin;)
      {
        const DevRec& r = recs[i];
        const uint32_t t = r.tableRow >> kRowBits, row = r.tableRow & kRowMask;
        REQUIRE(row < rows[t] && (size_t)r.first + r.count <= d.V && r.count > 0);
        if (row >= rows[t] || (size_t)r.first + r.count > d.V) return;
        for (uint32_t v = 0; v < r.count; ++v) got[t][(size_t)row * d.V + r.first + v] = r.bits;
      }
      total += end - begin;
      begin = end;
    }
    REQUIRE(total == recs.size());
    for (uint32_t t = 0; t < kTables; ++t) REQUIRE(got[t] == naive[t]);
    // a batch is as long as it can be: the record after it shares a word with one of its records
    begin = 0;
    for (size_t b = 0; b + 1 < p.batches(); ++b)
    {
      const size_t end = p.batchEnd(b);
      bool shares = false;
      for (size_t i = begin; i < end && !shares; ++i)
        shares = recs[i].tableRow == recs[end].tableRow && recs[i].first < recs[end].first + recs[end].count && recs[end].first < recs[i].first + recs[i].count;
      REQUIRE(shares);
      begin = end;
    }
    if (failures) return;
  }
}

int main()
{
  handWritten();
  randomLists();
  if (failures)
  {
    printf("%d failure(s)\n", failures);
    return 1;
  }
  printf("All tests passed\n");
  return 0;
}
