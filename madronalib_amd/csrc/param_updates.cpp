// param_updates.cpp — see param_updates.hpp. No HIP header, no device call.
#include "param_updates.hpp"

#include <stdio.h>
#include <string.h>

#include <algorithm>

namespace mlupd
{
namespace
{
// One record of the list: refused (status, `why`), or `count` table records and `rings` ring records, written to dst / ringDst
// where those are given
struct Expansion
{
  int status{MLGPU_OK};
  const char* why{nullptr};
  size_t count{0}, rings{0};
};

Expansion refuse(int status, const char* why)
{
  Expansion x;
  x.status = status;
  x.why = why;
  return x;
}

// T::clear() of one node for a voice range: a device record per state word clear() resets
size_t clearNode(const NodeDesc& nd, const mlgpu_update& u, DevRec* dst)
{
  size_t k = 0;
  for (int i = 0; i < nd.ns; ++i)
  {
    if (!nd.clearMask[(size_t)i]) continue;
    if (dst) dst[k] = makeRec(TABLE_STATE, (uint32_t)(nd.sOff + i), u.first_voice, u.n_voices, nd.clearWords[(size_t)i]);
    ++k;
  }
  return k;
}

// The ring words of one node for a voice range, as strided spans (RingRec). A voice's words, from the address map of the generated
// kernels (VoiceMem's ring base, RingCore::chunkMem / chunkOf): layout ROWS - memOff * V + row * V + v for every row of the node's
// ringWords; the windowed layouts - G words at base + k * 256 * G, k < ringWords / G, with base = memOff * memVoices + (v >> 8) *
// ringWords * 256 + (v & 255) * G. Neighbouring voices of a 256-voice block are neighbours in memory, so a range is one record per
// block it touches (ROWS: one in all).
inline void putRing(RingRec* dst, const RingRec& r) { memcpy((void*)dst, &r, sizeof(r)); }  // (slots of a DevRec buffer)
size_t clearRings(const TableDesc& d, const NodeDesc& nd, const mlgpu_update& u, RingRec* dst)
{
  if (!nd.rings || !nd.ringWords) return 0;
  const uint64_t first = u.first_voice, G = d.ringGranule;
  uint64_t end = first + u.n_voices;
  if (G == 1)
  {
    if (dst) putRing(dst, RingRec{nd.memOff * d.V + first, u.n_voices, (uint32_t)d.V, (uint32_t)nd.ringWords, {0u, 0u, 0u}});
    return 1;
  }
  // the spare lanes' rings must go on holding what the last voice's holds
  if (d.spareLanes && end == d.V) end = (end + 63u) & ~(uint64_t)63;
  size_t k = 0;
  for (uint64_t blk = first >> 8; blk <= (end - 1) >> 8; ++blk, ++k)
  {
    const uint64_t lo = std::max(first, blk << 8), hi = std::min(end, (blk + 1) << 8);
    if (dst)
      putRing(dst + k, RingRec{nd.memOff * d.memVoices + blk * nd.ringWords * 256u + (lo & 255u) * G, (uint32_t)((hi - lo) * G), (uint32_t)(256u * G), (uint32_t)(nd.ringWords / G), {0u, 0u, 0u}});
  }
  return k;
}

Expansion expand(const TableDesc& d, const mlgpu_update& u, DevRec* dst, RingRec* ringDst)
{
  Expansion x;
  if (u.n_voices == 0) return refuse(MLGPU_ERR_INVALID, "n_voices is 0");
  if ((uint64_t)u.first_voice + (uint64_t)u.n_voices > (uint64_t)d.V) return refuse(MLGPU_ERR_RANGE, "the voice range ends beyond the last voice");
  if (u.target > MLGPU_UPDATE_CLEAR_RINGS) return refuse(MLGPU_ERR_INVALID, "unknown target");
  const bool withRings = u.target == MLGPU_UPDATE_CLEAR_RINGS;
  if (u.target == MLGPU_UPDATE_INPUT_CONST)
  {
    if (!d.bank) return refuse(MLGPU_ERR_INVALID, "INPUT_CONST is a bank's table, not a graph's");
    if (dst) dst[0] = makeRec(TABLE_INPUT_CONST, 0, u.first_voice, u.n_voices, u.bits);
    x.count = 1;
    return x;
  }
  if (u.target == MLGPU_UPDATE_PARAM && d.bank) return refuse(MLGPU_ERR_INVALID, "PARAM is a graph's table, not a bank's");
  if ((u.target == MLGPU_UPDATE_CLEAR || withRings) && u.node == -1)
  {
    for (const NodeDesc& nd : d.nodes)
      if (!withRings && (nd.kind == NodeDesc::PROC || nd.kind == NodeDesc::FEEDBACK) && nd.rings)
        return refuse(MLGPU_ERR_UNSUPPORTED, "CLEAR of every node: a node has delay rings, which CLEAR leaves alone (CLEAR_RINGS zeroes them too)");
    for (const NodeDesc& nd : d.nodes)
      if (nd.kind == NodeDesc::PROC || nd.kind == NodeDesc::FEEDBACK)
      {
        x.count += clearNode(nd, u, dst ? dst + x.count : nullptr);
        if (withRings) x.rings += clearRings(d, nd, u, ringDst ? ringDst + x.rings : nullptr);
      }
    return x;
  }
  if (u.node < 0 || (size_t)u.node >= d.nodes.size()) return refuse(MLGPU_ERR_RANGE, d.bank ? "processor index out of range" : "node index out of range");
  const NodeDesc& nd = d.nodes[(size_t)u.node];
  switch (u.target)
  {
    case MLGPU_UPDATE_PARAM:
      if (nd.kind != NodeDesc::PARAM) return refuse(MLGPU_ERR_INVALID, "PARAM: not a param node");
      if (dst) dst[0] = makeRec(TABLE_PARAMS, (uint32_t)nd.paramRow, u.first_voice, u.n_voices, u.bits);
      x.count = 1;
      break;
    case MLGPU_UPDATE_COEFF:
      if (nd.kind != NodeDesc::PROC) return refuse(MLGPU_ERR_INVALID, "COEFF: not a processor node");
      if ((int)u.index >= nd.nc) return refuse(MLGPU_ERR_RANGE, "COEFF: coefficient index out of range");
      if (dst) dst[0] = makeRec(TABLE_COEFFS, (uint32_t)(nd.cOff + (int)u.index), u.first_voice, u.n_voices, u.bits);
      x.count = 1;
      break;
    case MLGPU_UPDATE_STATE:
      if (nd.kind != NodeDesc::PROC && nd.kind != NodeDesc::FEEDBACK) return refuse(MLGPU_ERR_INVALID, "STATE: the node has no state");
      if ((int)u.index >= nd.ns) return refuse(MLGPU_ERR_RANGE, "STATE: state index out of range");
      if (dst) dst[0] = makeRec(TABLE_STATE, (uint32_t)(nd.sOff + (int)u.index), u.first_voice, u.n_voices, u.bits);
      x.count = 1;
      break;
    default:  // MLGPU_UPDATE_CLEAR / _CLEAR_RINGS of one node
      if (nd.kind != NodeDesc::PROC && nd.kind != NodeDesc::FEEDBACK) return refuse(MLGPU_ERR_INVALID, withRings ? "CLEAR_RINGS: not a processor / feedback node" : "CLEAR: not a processor / feedback node");
      if (nd.rings && !withRings) return refuse(MLGPU_ERR_UNSUPPORTED, "CLEAR: the node has delay rings, which CLEAR leaves alone (CLEAR_RINGS zeroes them too)");
      x.count = clearNode(nd, u, dst);
      if (withRings) x.rings = clearRings(d, nd, u, ringDst);
      break;
  }
  return x;
}

inline bool before(const DevRec& a, const DevRec& b) { return a.tableRow != b.tableRow ? a.tableRow < b.tableRow : a.first < b.first; }
// (a not after b in that order:) do they share a word?
inline bool overlap(const DevRec& a, const DevRec& b) { return a.tableRow == b.tableRow && (uint64_t)a.first + a.count > (uint64_t)b.first; }
}  // namespace

void UpdatePlanner::reserve(size_t maxDeviceRecords)
{
  order.reserve(maxDeviceRecords);
  ends.reserve(maxDeviceRecords);  // (the worst list: every record over the one before)
}

int UpdatePlanner::validate(const TableDesc& d, const mlgpu_update* recs, size_t n)
{
  nDev = nTable = 0;
  err[0] = 0;
  size_t total = 0, rings = 0;
  for (size_t i = 0; i < n; ++i)
  {
    const Expansion x = expand(d, recs[i], nullptr, nullptr);
    if (x.status != MLGPU_OK)
    {
      snprintf(err, sizeof(err), "update record %zu of %zu (node %d, target %u, index %u, voices %u + %u): %s", i, n, (int)recs[i].node, (unsigned)recs[i].target,
               (unsigned)recs[i].index, (unsigned)recs[i].first_voice, (unsigned)recs[i].n_voices, x.why);
      return x.status;
    }
    total += x.count;
    rings += x.rings;
  }
  nTable = total;
  nDev = total + 2 * rings;
  return MLGPU_OK;
}

// Do records [s, e) write no word twice? Sorted by row and first voice, only neighbours can be the first to overlap.
bool UpdatePlanner::disjoint(const DevRec* r, size_t s, size_t e)
{
  // a list that comes in row and voice order needs no sorting (the common one: instruments in order)
  bool sorted = true;
  for (size_t i = s + 1; i < e && sorted; ++i) sorted = !before(r[i], r[i - 1]);
  if (sorted)
  {
    for (size_t i = s + 1; i < e; ++i)
      if (overlap(r[i - 1], r[i])) return false;
    return true;
  }
  order.resize(e - s);
  for (size_t i = s; i < e; ++i) order[i - s] = (uint32_t)i;
  std::sort(order.begin(), order.end(), [r](uint32_t a, uint32_t b) { return before(r[a], r[b]); });
  for (size_t i = 1; i < order.size(); ++i)
    if (overlap(r[order[i - 1]], r[order[i]])) return false;
  return true;
}

void UpdatePlanner::pack(const TableDesc& d, const mlgpu_update* recs, size_t n, DevRec* dst)
{
  size_t k = 0, rk = 0;
  RingRec* const ringDst = (RingRec*)(dst + nTable);  // (16-byte slots of one buffer: the ring records behind the table records)
  for (size_t i = 0; i < n; ++i)
  {
    const Expansion x = expand(d, recs[i], dst + k, ringDst + rk);
    k += x.count;
    rk += x.rings;
  }
  ends.clear();
  if (!k) return;
  if (disjoint(dst, 0, k))
  {
    ends.push_back(k);
    return;
  }
  // Batches are runs of the list: each the longest run from its start that writes no word twice, found by doubling the run while it
  // stays disjoint and bisecting the last step (the sorting is of the run, not of the list)
  size_t s = 0;
  while (s < k)
  {
    size_t good = s + 1, bad = k + 1, step = 1;  // [s, good) is disjoint, [s, bad) is not (k + 1: nothing known)
    while (good < k)
    {
      const size_t e = std::min(good + step, k);
      if (disjoint(dst, s, e))
      {
        good = e;
        step *= 2;
      }
      else
      {
        bad = e;
        break;
      }
    }
    while (bad <= k && bad - good > 1)
    {
      const size_t mid = good + (bad - good) / 2;
      if (disjoint(dst, s, mid))
        good = mid;
      else
        bad = mid;
    }
    ends.push_back(good);
    s = good;
  }
}
}  // namespace mlupd
