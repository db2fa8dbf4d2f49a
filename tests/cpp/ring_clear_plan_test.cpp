// tests/cpp/ring_clear_plan_test.cpp — MLGPU_UPDATE_CLEAR_RINGS in the host planner of sparse updates
// (madronalib_amd/csrc/param_updates.cpp) on its own: built with g++ -fsanitize=address,undefined from that one file
// (tests/test_ring_clear_cpu.py). Hand-written voice ranges go in and the ring records (offset, span, stride, rows) are compared
// with records worked out by hand from the ring layouts' address maps; then random graphs, layouts and ranges, where the set of
// ring-memory words the records cover must be exactly the set a brute-force walk over (voice, ring, sample) gives - every word of
// the cleared voices and no word of any other voice, lane or node.
#include <algorithm>
#include <cstdio>
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
struct Ring
{
  uint64_t offset;
  uint32_t span, stride, rows;
  bool operator==(const Ring& o) const { return offset == o.offset && span == o.span && stride == o.stride && rows == o.rows; }
};
typedef std::vector<Ring> Rings;

static mlgpu_update upd(int node, int target, int index, uint32_t first, uint32_t count, uint32_t bits = 0)
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
static mlgpu_update rings(int node, uint32_t first, uint32_t count) { return upd(node, MLGPU_UPDATE_CLEAR_RINGS, 0xFFFF /* ignored */, first, count, 0xDEADu /* ignored */); }

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
// a delay node: `nRings` rings of `len` samples from word memOff * memVoices on; its state words as given
static NodeDesc delay(int sOff, int ns, std::vector<uint8_t> clearMask, uint64_t memOff, uint64_t len, int nRings)
{
  NodeDesc n = proc(0, 0, sOff, ns, {}, clearMask);
  n.rings = true;
  n.memOff = memOff;
  n.ringWords = len * (uint64_t)nRings;
  return n;
}

struct Packed
{
  int status;
  Rs recs;
  Rings rings;
  std::vector<size_t> ends;
  std::string error;
  size_t nDev;
};
// validate + pack into a buffer of exactly the announced size, framed by guard records that must survive
static Packed run(UpdatePlanner& p, const TableDesc& d, const std::vector<mlgpu_update>& list)
{
  Packed out;
  out.status = p.validate(d, list.data(), list.size());
  out.error = p.error();
  out.nDev = p.deviceRecords();
  const DevRec guard{0xDEADBEEFu, 1u, 2u, 3u};
  if (out.status != MLGPU_OK)
  {
    REQUIRE(p.deviceRecords() == 0 && p.tableRecords() == 0 && p.ringRecords() == 0);
    return out;
  }
  REQUIRE(p.deviceRecords() == p.tableRecords() + 2 * p.ringRecords());
  std::vector<DevRec> buf(p.deviceRecords() + 2, guard);
  p.pack(d, list.data(), list.size(), buf.data() + 1);
  REQUIRE(!memcmp(&buf.front(), &guard, sizeof(guard)) && !memcmp(&buf.back(), &guard, sizeof(guard)));
  for (size_t i = 1; i < 1 + p.tableRecords(); ++i) out.recs.push_back(R{buf[i].tableRow >> kRowBits, buf[i].tableRow & kRowMask, buf[i].first, buf[i].count, buf[i].bits});
  for (size_t i = 0; i < p.ringRecords(); ++i)
  {
    RingRec rr;
    memcpy(&rr, buf.data() + 1 + p.tableRecords() + 2 * i, sizeof(rr));
    REQUIRE(rr.pad[0] == 0 && rr.pad[1] == 0 && rr.pad[2] == 0);
    out.rings.push_back(Ring{rr.offset, rr.span, rr.stride, rr.rows});
  }
  for (size_t b = 0; b < p.batches(); ++b) out.ends.push_back(p.batchEnd(b));
  if (!out.ends.empty()) REQUIRE(out.ends.back() == p.tableRecords());  // (batches are of the table records alone)
  return out;
}

// The graph of the hand-written cases, V = 600: a param, a feedback node (state rows 0-63), a Lopass (64-65), an IntegerDelay D1
// (row 66, the write index: clear() leaves it) with one ring of 256 at memOff 0, a FractionalDelay-like D2 (rows 67-69: index,
// two allpass words) with one ring of 512 at memOff 256, and a PitchbendableDelay-like P (no state here) with two rings of 256 at
// memOff 768. Ring words per voice in all: 1280.
enum { PITCH = 0, FB, LOPASS, D1, D2, P, SINE };
static TableDesc graphDesc(uint32_t G, size_t V = 600)
{
  TableDesc d;
  d.V = V;
  d.ringGranule = G;
  d.memVoices = G == 1 ? V : ((V + 255) & ~(size_t)255);
  d.spareLanes = G == 16 && V % 64;
  d.nodes.resize(7);
  d.nodes[PITCH] = param(0);
  d.nodes[FB] = feedback(0);
  d.nodes[LOPASS] = proc(0, 3, 64, 2);
  d.nodes[D1] = delay(66, 1, {0}, 0, 256, 1);
  d.nodes[D2] = delay(67, 3, {0, 1, 1}, 256, 512, 1);
  d.nodes[P] = delay(70, 0, {}, 768, 256, 2);
  d.nodes[SINE] = proc(3, 0, 70, 1, {0xC0000000u});
  return d;
}

static void handWritten()
{
  UpdatePlanner p;
  static_assert(sizeof(RingRec) == 32, "two 16-byte slots");
  static_assert(MLGPU_UPDATE_CLEAR_RINGS == 5, "the C ABI's value");

  // ---- layout ROWS (G = 1): [ring position][voice], one record per node and range
  TableDesc d = graphDesc(1);
  Packed r = run(p, d, {rings(D1, 300, 1)});
  REQUIRE(r.status == MLGPU_OK && r.recs.empty() && r.ends.empty() && r.nDev == 2);
  REQUIRE(r.rings == Rings({{300, 1, 600, 256}}));
  r = run(p, d, {rings(D1, 250, 270)});  // (crossing 255 | 256 and 511 | 512 means nothing here)
  REQUIRE(r.status == MLGPU_OK && r.rings == Rings({{250, 270, 600, 256}}) && r.nDev == 2);
  r = run(p, d, {rings(D2, 300, 1)});    // memOff 256, another length; its two allpass words are CLEAR's
  REQUIRE(r.status == MLGPU_OK && r.rings == Rings({{256 * 600 + 300, 1, 600, 512}}) && r.nDev == 4);
  REQUIRE(r.recs == Rs({{TABLE_STATE, 68, 300, 1, 0}, {TABLE_STATE, 69, 300, 1, 0}}) && r.ends == std::vector<size_t>({2}));
  r = run(p, d, {rings(P, 300, 1)});     // two rings: one record over both
  REQUIRE(r.status == MLGPU_OK && r.rings == Rings({{768 * 600 + 300, 1, 600, 512}}));
  r = run(p, d, {rings(P, 599, 1)});
  REQUIRE(r.status == MLGPU_OK && r.rings == Rings({{768 * 600 + 599, 1, 600, 512}}));

  // ---- layouts WINDOWS / SECTORS (G = 8): [256-voice block][sample / 8][lane][8], memVoices 768
  d = graphDesc(8);
  r = run(p, d, {rings(D1, 300, 1)});
  REQUIRE(r.status == MLGPU_OK && r.rings == Rings({{1 * 256 * 256 + 44 * 8, 8, 2048, 32}}) && r.nDev == 2);
  r = run(p, d, {rings(D1, 250, 270)});
  REQUIRE(r.status == MLGPU_OK && r.nDev == 6);
  REQUIRE(r.rings == Rings({{250 * 8, 6 * 8, 2048, 32}, {65536, 256 * 8, 2048, 32}, {131072, 8 * 8, 2048, 32}}));
  r = run(p, d, {rings(D1, 255, 2)});
  REQUIRE(r.status == MLGPU_OK && r.rings == Rings({{255 * 8, 8, 2048, 32}, {65536, 8, 2048, 32}}));
  r = run(p, d, {rings(D1, 511, 2)});
  REQUIRE(r.status == MLGPU_OK && r.rings == Rings({{65536 + 255 * 8, 8, 2048, 32}, {131072, 8, 2048, 32}}));
  r = run(p, d, {rings(D2, 300, 1)});
  REQUIRE(r.status == MLGPU_OK && r.rings == Rings({{256 * 768 + 1 * 512 * 256 + 44 * 8, 8, 2048, 64}}));
  r = run(p, d, {rings(P, 300, 1)});
  REQUIRE(r.status == MLGPU_OK && r.rings == Rings({{768 * 768 + 1 * 512 * 256 + 44 * 8, 8, 2048, 64}}));
  r = run(p, d, {rings(P, 599, 1)});  // (no spare lanes in this layout)
  REQUIRE(r.status == MLGPU_OK && r.rings == Rings({{768 * 768 + 2 * 512 * 256 + 87 * 8, 8, 2048, 64}}));

  // ---- layout TRANSPOSED (G = 16): [256-voice block][sample / 16][lane][16]
  d = graphDesc(16);
  r = run(p, d, {rings(D1, 300, 1)});
  REQUIRE(r.status == MLGPU_OK && r.rings == Rings({{65536 + 44 * 16, 16, 4096, 16}}));
  r = run(p, d, {rings(D1, 250, 270)});
  REQUIRE(r.status == MLGPU_OK && r.rings == Rings({{250 * 16, 6 * 16, 4096, 16}, {65536, 256 * 16, 4096, 16}, {131072, 8 * 16, 4096, 16}}));
  r = run(p, d, {rings(D2, 300, 1)});
  REQUIRE(r.status == MLGPU_OK && r.rings == Rings({{256 * 768 + 1 * 512 * 256 + 44 * 16, 16, 4096, 32}}));
  r = run(p, d, {rings(P, 300, 1)});
  REQUIRE(r.status == MLGPU_OK && r.rings == Rings({{768 * 768 + 1 * 512 * 256 + 44 * 16, 16, 4096, 32}}));
  // V = 600 is no multiple of 64: voice 599 takes the spare lanes 600 .. 639 with it (lanes 87 .. 127 of block 2)
  r = run(p, d, {rings(D1, 599, 1)});
  REQUIRE(r.status == MLGPU_OK && r.rings == Rings({{131072 + 87 * 16, 41 * 16, 4096, 16}}));
  r = run(p, d, {rings(D1, 598, 1)});
  REQUIRE(r.status == MLGPU_OK && r.rings == Rings({{131072 + 86 * 16, 16, 4096, 16}}));

  // ---- node = -1 over the feedback node, the Lopass, the delays and the SineGen: state-word records in node order, then the rings
  for (uint32_t G : {1u, 8u, 16u})
  {
    d = graphDesc(G);
    r = run(p, d, {rings(-1, 250, 270)});
    const size_t segs = G == 1 ? 1 : 3;
    REQUIRE(r.status == MLGPU_OK && r.recs.size() == 64 + 2 + 0 + 2 + 0 + 1 && r.rings.size() == 3 * segs && r.nDev == 69 + 2 * 3 * segs);
    REQUIRE(r.ends == std::vector<size_t>({69}));
    REQUIRE(r.recs[0] == (R{TABLE_STATE, 0, 250, 270, 0}) && r.recs[64] == (R{TABLE_STATE, 64, 250, 270, 0}) && r.recs[66] == (R{TABLE_STATE, 68, 250, 270, 0}));
    REQUIRE(r.recs[68] == (R{TABLE_STATE, 70, 250, 270, 0xC0000000u}));
    // (node order: D1's segments, D2's, P's)
    REQUIRE(r.rings[0].rows == 256 / G && r.rings[segs].rows == 512 / G && r.rings[2 * segs].rows == 512 / G);
    REQUIRE(r.rings[segs].offset == 256 * d.memVoices + 250 * G && r.rings[2 * segs].offset == 768 * d.memVoices + 250 * G);
  }

  // ---- the spare lanes of layout 2 at V = 80: lanes 80 .. 127 run voice 79 again on rings of their own
  d = graphDesc(16, 80);
  REQUIRE(d.spareLanes && d.memVoices == 256);
  r = run(p, d, {rings(D1, 79, 1)});
  REQUIRE(r.status == MLGPU_OK && r.rings == Rings({{79 * 16, 49 * 16, 4096, 16}}));
  r = run(p, d, {rings(D1, 60, 10)});  // (ends before the last voice: no extension)
  REQUIRE(r.status == MLGPU_OK && r.rings == Rings({{60 * 16, 10 * 16, 4096, 16}}));
  r = run(p, d, {rings(D1, 70, 10)});
  REQUIRE(r.status == MLGPU_OK && r.rings == Rings({{70 * 16, 58 * 16, 4096, 16}}));
  // (the state-word records keep the range as given: the spare lanes have no state of their own)
  r = run(p, d, {rings(D2, 70, 10)});
  REQUIRE(r.status == MLGPU_OK && r.recs == Rs({{TABLE_STATE, 68, 70, 10, 0}, {TABLE_STATE, 69, 70, 10, 0}}));
  // ... and none in the other layouts, or where the last wavefront is full
  d = graphDesc(8, 80);
  r = run(p, d, {rings(D1, 79, 1)});
  REQUIRE(r.status == MLGPU_OK && r.rings == Rings({{79 * 8, 8, 2048, 32}}));
  d = graphDesc(16, 128);
  REQUIRE(!d.spareLanes);
  r = run(p, d, {rings(D1, 127, 1)});
  REQUIRE(r.status == MLGPU_OK && r.rings == Rings({{127 * 16, 16, 4096, 16}}));

  // ---- without rings the new target is CLEAR: the same records, the same count
  d = graphDesc(8);
  for (int node : {(int)FB, (int)LOPASS, (int)SINE})
  {
    const Packed a = run(p, d, {upd(node, MLGPU_UPDATE_CLEAR, 0, 64, 16)}), b = run(p, d, {rings(node, 64, 16)});
    REQUIRE(a.status == MLGPU_OK && b.status == MLGPU_OK && !a.recs.empty() && a.recs == b.recs && a.ends == b.ends && a.nDev == b.nDev && b.rings.empty());
  }
  TableDesc bank;
  bank.bank = true;
  bank.V = 80;
  bank.nodes = {proc(0, 0, 0, 2), proc(0, 3, 2, 2), proc(3, 1, 4, 0)};
  for (int node : {-1, 0, 1, 2})
  {
    const Packed a = run(p, bank, {upd(node, MLGPU_UPDATE_CLEAR, 0, 60, 20)}), b = run(p, bank, {rings(node, 60, 20)});
    REQUIRE(a.status == MLGPU_OK && b.status == MLGPU_OK && a.recs == b.recs && a.ends == b.ends && a.nDev == b.nDev && b.rings.empty());
    REQUIRE(a.recs.size() == (node == -1 ? 4u : node == 2 ? 0u : 2u));
  }

  // ---- mixed lists: table records in list order, ring records behind them in list order; cuts among the table records alone
  r = run(p, d, {upd(PITCH, MLGPU_UPDATE_PARAM, 0, 0, 600, 7), rings(D2, 10, 4), upd(D2, MLGPU_UPDATE_STATE, 1, 12, 1, 9), rings(D2, 12, 300), rings(D1, 0, 1)});
  REQUIRE(r.status == MLGPU_OK && r.nDev == 6 + 2 * (1 + 2 + 1));
  REQUIRE(r.recs == Rs({{TABLE_PARAMS, 0, 0, 600, 7}, {TABLE_STATE, 68, 10, 4, 0}, {TABLE_STATE, 69, 10, 4, 0}, {TABLE_STATE, 68, 12, 1, 9}, {TABLE_STATE, 68, 12, 300, 0},
                        {TABLE_STATE, 69, 12, 300, 0}}));
  REQUIRE(r.ends == std::vector<size_t>({3, 4, 6}));
  const uint64_t d2 = 256 * 768;
  REQUIRE(r.rings == Rings({{d2 + 10 * 8, 4 * 8, 2048, 64}, {d2 + 12 * 8, 244 * 8, 2048, 64}, {d2 + 512 * 256, 56 * 8, 2048, 64}, {0, 8, 2048, 32}}));

  // ---- refusals
  struct Bad
  {
    mlgpu_update u;
    int status;
  };
  const Bad bad[] = {
      {rings(PITCH, 0, 1), MLGPU_ERR_INVALID},                        // target 5 on a param node
      {upd(D1, 6, 0, 0, 1), MLGPU_ERR_INVALID},                       // no target 6
      {upd(D1, 0xFFFF, 0, 0, 1), MLGPU_ERR_INVALID},
      {rings(7, 0, 1), MLGPU_ERR_RANGE},                              // no such node
      {rings(-2, 0, 1), MLGPU_ERR_RANGE},
      {rings(D1, 599, 2), MLGPU_ERR_RANGE},                           // beyond the last voice
      {rings(-1, 0, 601), MLGPU_ERR_RANGE},
      {rings(D1, 5, 0), MLGPU_ERR_INVALID},                           // n_voices == 0
      {upd(D1, MLGPU_UPDATE_CLEAR, 0, 0, 1), MLGPU_ERR_UNSUPPORTED},  // CLEAR itself still stops at rings
      {upd(-1, MLGPU_UPDATE_CLEAR, 0, 0, 1), MLGPU_ERR_UNSUPPORTED},
  };
  for (const Bad& b : bad)
  {
    r = run(p, d, {rings(D1, 0, 600), rings(-1, 3, 1), b.u, rings(P, 0, 1)});
    REQUIRE(r.status == b.status);
    REQUIRE(r.error.find("record 2 of 4") != std::string::npos);
    REQUIRE(r.recs.empty() && r.rings.empty() && r.ends.empty() && r.nDev == 0);
    if (b.status == MLGPU_ERR_UNSUPPORTED) REQUIRE(r.error.find("rings") != std::string::npos && r.error.find("CLEAR_RINGS") != std::string::npos);
  }
  r = run(p, d, {rings(PITCH, 0, 1)});
  REQUIRE(r.status == MLGPU_ERR_INVALID && r.error.find("not a processor / feedback node") != std::string::npos);
  r = run(p, d, {upd(D1, 6, 0, 0, 1)});
  REQUIRE(r.status == MLGPU_ERR_INVALID && r.error.find("unknown target") != std::string::npos);
  // a ring node described without geometry (no memory): nothing to zero, CLEAR still refused
  TableDesc bare = d;
  bare.nodes[D1].ringWords = 0;
  r = run(p, bare, {rings(D1, 0, 600)});
  REQUIRE(r.status == MLGPU_OK && r.rings.empty() && r.nDev == 0);
  r = run(p, bare, {upd(D1, MLGPU_UPDATE_CLEAR, 0, 0, 1)});
  REQUIRE(r.status == MLGPU_ERR_UNSUPPORTED);
}

// Where sample i of ring `ring` of voice (lane) v of a delay node lies, written out from the layouts' address maps - layout 0:
// rows of V voices; the windowed layouts: this lane's G-word piece of the 256-voice block's granule i / G.
static uint64_t wordOf(const TableDesc& d, const NodeDesc& nd, uint64_t len, uint64_t v, uint64_t ring, uint64_t i)
{
  const uint64_t G = d.ringGranule;
  if (G == 1) return nd.memOff * d.V + (ring * len + i) * d.V + v;
  const uint64_t base = nd.memOff * d.memVoices + (v >> 8) * nd.ringWords * 256 + (v & 255) * G;
  return base + (ring * len + (i & ~(G - 1))) * 256 + (i & (G - 1));
}

// At least 2 000 random (V, layout, nodes, ranges): the words the records cover against the brute-force set
static void randomCases()
{
  uint32_t seed = 88172645u;
  auto rnd = [&](uint32_t n) {
    seed ^= seed << 13;
    seed ^= seed >> 17;
    seed ^= seed << 5;
    return seed % n;
  };
  UpdatePlanner p;
  size_t cleared = 0, extended = 0;
  for (int trial = 0; trial < 2400; ++trial)
  {
    TableDesc d;
    static const uint32_t Vs[] = {1, 63, 64, 65, 80, 255, 256, 257, 511, 512, 513, 600};
    d.V = trial % 3 == 0 ? Vs[rnd(12)] : 1 + rnd(trial % 8 == 1 ? 700 : 300);
    static const uint32_t Gs[] = {1, 8, 8, 16};  // layouts ROWS, WINDOWS, SECTORS, TRANSPOSED
    d.ringGranule = Gs[trial % 4];
    d.memVoices = d.ringGranule == 1 ? d.V : ((d.V + 255) & ~(size_t)255);
    d.spareLanes = d.ringGranule == 16 && d.V % 64;
    const int nNodes = 1 + (int)rnd(6);
    int nParams = 0, NS = 0;
    uint64_t memFloats = 0;
    std::vector<uint64_t> lens((size_t)nNodes, 0);
    std::vector<int> nRings((size_t)nNodes, 0);
    for (int i = 0; i < nNodes; ++i)
    {
      const uint32_t k = rnd(6);
      if (k == 0)
        d.nodes.push_back(param(nParams++));
      else if (k == 1)
      {
        d.nodes.push_back(feedback(NS));
        NS += 64;
      }
      else if (k == 2)
      {
        const int ns = (int)rnd(4);
        d.nodes.push_back(proc(0, 0, NS, ns));
        NS += ns;
      }
      else
      {
        const int ns = (int)rnd(4);
        std::vector<uint8_t> mask;
        for (int w = 0; w < ns; ++w) mask.push_back((uint8_t)(w != 0));  // (word 0: the write index)
        lens[(size_t)i] = (uint64_t)64 << rnd(3);
        nRings[(size_t)i] = 1 + (int)rnd(2);
        d.nodes.push_back(delay(NS, ns, mask, memFloats, lens[(size_t)i], nRings[(size_t)i]));
        memFloats += lens[(size_t)i] * (uint64_t)nRings[(size_t)i];
        NS += ns;
      }
    }
    const uint64_t memWords = memFloats * d.memVoices;
    std::vector<uint8_t> want(memWords, 0), got(memWords, 0);
    std::vector<mlgpu_update> list;
    const size_t n = 1 + rnd(4);
    size_t wantTable = 0;
    while (list.size() < n)
    {
      const int node = rnd(5) == 0 ? -1 : (int)rnd((uint32_t)nNodes);
      const uint32_t first = rnd((uint32_t)d.V), count = std::min<uint32_t>(1 + rnd(rnd(3) ? 4 : (uint32_t)d.V), (uint32_t)d.V - first);
      const mlgpu_update u = rnd(8) == 0 && node >= 0 && d.nodes[(size_t)node].kind == NodeDesc::PARAM ? upd(node, MLGPU_UPDATE_PARAM, 0, first, count, 5) : rings(node, first, count);
      UpdatePlanner probe;
      if (probe.validate(d, &u, 1) != MLGPU_OK) continue;
      list.push_back(u);
      wantTable += probe.tableRecords();
      if (u.target != MLGPU_UPDATE_CLEAR_RINGS) continue;
      // brute force, per voice, ring and sample; the spare lanes behind voice V - 1 in layout 2 hold what it holds
      for (int j = 0; j < nNodes; ++j)
      {
        if ((node != -1 && node != j) || !d.nodes[(size_t)j].rings) continue;
        uint64_t end = (uint64_t)first + count;
        if (d.spareLanes && end == d.V)
        {
          end = (d.V + 63) & ~(uint64_t)63;
          ++extended;
        }
        for (uint64_t v = first; v < end; ++v)
          for (int ring = 0; ring < nRings[(size_t)j]; ++ring)
            for (uint64_t i = 0; i < lens[(size_t)j]; ++i)
            {
              const uint64_t w = wordOf(d, d.nodes[(size_t)j], lens[(size_t)j], v, (uint64_t)ring, i);
              REQUIRE(w < memWords);
              if (w < memWords) want[w] = 1;
            }
        ++cleared;
      }
    }
    REQUIRE(p.validate(d, list.data(), list.size()) == MLGPU_OK);
    REQUIRE(p.tableRecords() == wantTable && p.deviceRecords() == wantTable + 2 * p.ringRecords());
    std::vector<DevRec> buf(p.deviceRecords());
    p.pack(d, list.data(), list.size(), buf.data());
    for (size_t i = 0; i < p.ringRecords(); ++i)
    {
      RingRec rr;
      memcpy(&rr, buf.data() + p.tableRecords() + 2 * i, sizeof(rr));
      REQUIRE(rr.span > 0 && rr.rows > 0 && rr.span <= rr.stride);
      // what the 16-byte stores of the windowed layouts need
      if (d.ringGranule >= 8) REQUIRE(rr.offset % 4 == 0 && rr.span % 4 == 0 && rr.stride % 4 == 0);
      REQUIRE(rr.offset + (uint64_t)(rr.rows - 1) * rr.stride + rr.span <= memWords);
      if (rr.offset + (uint64_t)(rr.rows - 1) * rr.stride + rr.span > memWords) return;
      for (uint64_t row = 0; row < rr.rows; ++row)
        for (uint64_t j = 0; j < rr.span; ++j) got[rr.offset + row * rr.stride + j] = 1;
    }
    REQUIRE(got == want);
    if (failures) return;
  }
  REQUIRE(cleared > 2000 && extended > 20);  // (the cases were not vacuous)
}

int main()
{
  handWritten();
  randomCases();
  if (failures)
  {
    printf("%d failure(s)\n", failures);
    return 1;
  }
  printf("All tests passed\n");
  return 0;
}
