// voice_records.cpp — see voice_records.hpp. No HIP header, no device call.
#include "voice_records.hpp"

#include <stdio.h>
#include <string.h>

#include <algorithm>

namespace mlrec
{
namespace
{
struct Fnv  // FNV-1a over 64-bit values, byte by byte
{
  uint64_t h{1469598103934665603ull};
  void add(uint64_t x)
  {
    for (int i = 0; i < 8; ++i)
    {
      h ^= (x >> (8 * i)) & 0xffu;
      h *= 1099511628211ull;
    }
  }
};

Segment makeSegment(uint64_t base, size_t rows, size_t recOff, uint32_t where) { return Segment{base, (uint32_t)rows, (uint32_t)recOff, where, {0u, 0u, 0u}}; }
}  // namespace

bool RecordPlan::describe(const mlupd::TableDesc& d, const std::vector<NodeSig>& sigs, int ringLayout, int revision)
{
  W = nTableWords = nEntries = 0;
  sig = 0;
  segs.clear();
  err[0] = 0;
  if (sigs.size() != d.nodes.size() || d.V == 0 || d.V > 0xffffffffull)
  {
    snprintf(err, sizeof(err), "voice records: the object's description is incomplete");
    return false;
  }
  V = d.V;
  G = d.ringGranule;
  memVoices = d.memVoices;
  spareLanes = d.spareLanes;
  if (G != 1 && G != 8 && G != 16)
  {
    snprintf(err, sizeof(err), "voice records: ring granule %u (1, 8 or 16)", (unsigned)G);
    return false;
  }
  size_t nParams = 0, nCoeffs = 0, nState = 0;
  for (const mlupd::NodeDesc& nd : d.nodes)
  {
    if (nd.kind == mlupd::NodeDesc::PARAM) nParams = std::max(nParams, (size_t)nd.paramRow + 1);
    if (nd.kind == mlupd::NodeDesc::PROC) nCoeffs = std::max(nCoeffs, (size_t)(nd.cOff + nd.nc));
    if (nd.kind == mlupd::NodeDesc::PROC || nd.kind == mlupd::NodeDesc::FEEDBACK) nState = std::max(nState, (size_t)(nd.sOff + nd.ns));
  }
  size_t at = 0;
  if (nParams) segs.push_back(makeSegment(0, nParams, at, mlupd::TABLE_PARAMS)), at += nParams;
  if (nCoeffs) segs.push_back(makeSegment(0, nCoeffs, at, mlupd::TABLE_COEFFS)), at += nCoeffs;
  if (nState) segs.push_back(makeSegment(0, nState, at, mlupd::TABLE_STATE)), at += nState;
  if (d.bank) segs.push_back(makeSegment(0, 1, at, mlupd::TABLE_INPUT_CONST)), at += 1;
  nTableWords = at;
  at = (at + 3) & ~(size_t)3;
  const size_t ringUnit = std::max<size_t>(G, 4);  // (the kernels move ring words four at a time)
  for (const mlupd::NodeDesc& nd : d.nodes)
  {
    if (!nd.rings || !nd.ringWords) continue;
    if (nd.ringWords % ringUnit || nd.ringWords > 0xffffffffull || at + nd.ringWords > 0xffffffffull)
    {
      snprintf(err, sizeof(err), "voice records: a node's %llu ring words per voice are no multiple of %zu, or a record would exceed 2^32 words", (unsigned long long)nd.ringWords, ringUnit);
      segs.clear();
      return false;
    }
    segs.push_back(makeSegment(nd.memOff * (uint64_t)(G == 1 ? V : memVoices), (size_t)nd.ringWords, at, kRing));
    at += (size_t)nd.ringWords;
  }
  if (at == 0)
  {
    snprintf(err, sizeof(err), "voice records: the object keeps nothing per voice");
    return false;
  }
  W = (at + 3) & ~(size_t)3;
  seen.assign((V + 63) / 64, 0);

  Fnv f;
  f.add(kFormatVersion);
  f.add((uint64_t)(int64_t)revision);
  f.add((uint64_t)(int64_t)ringLayout);
  f.add(d.bank ? 1u : 0u);
  f.add(nParams);
  f.add(d.nodes.size());
  for (size_t i = 0; i < d.nodes.size(); ++i)
  {
    const mlupd::NodeDesc& nd = d.nodes[i];
    f.add((uint64_t)(int64_t)sigs[i].type);
    f.add((uint64_t)(int64_t)sigs[i].kind);
    f.add((uint64_t)(int64_t)nd.nc);
    f.add((uint64_t)(int64_t)nd.ns);
    f.add(sigs[i].ringLen);
    f.add(sigs[i].rings);
  }
  sig = f.h;
  return true;
}

int RecordPlan::validate(const uint32_t* voices, size_t n, bool import)
{
  nEntries = 0;
  err[0] = 0;
  if (!described())
  {
    snprintf(err, sizeof(err), "the object has no voice record layout");
    return MLGPU_ERR_INVALID;
  }
  if (n == 0) return MLGPU_OK;
  if (!voices)
  {
    snprintf(err, sizeof(err), "null voice list");
    return MLGPU_ERR_INVALID;
  }
  for (size_t i = 0; i < n; ++i)
    if (voices[i] >= V)
    {
      snprintf(err, sizeof(err), "voice %u at position %zu of %zu: the object has %zu voices", (unsigned)voices[i], i, n, V);
      return MLGPU_ERR_RANGE;
    }
  size_t spare = 0;
  if (import)
  {
    size_t i = 0;
    for (; i < n; ++i)
    {
      uint64_t& word = seen[voices[i] >> 6];
      const uint64_t bit = (uint64_t)1 << (voices[i] & 63u);
      if (word & bit) break;
      word |= bit;
      if (spareLanes && voices[i] == V - 1) spare = ((V + 63) & ~(size_t)63) - V;
    }
    const size_t repeated = i;
    for (size_t k = 0; k < repeated; ++k) seen[voices[k] >> 6] = 0;  // (all zero again for the next call)
    if (repeated < n)
    {
      snprintf(err, sizeof(err), "voice %u at position %zu of %zu is in the list twice: an import wants distinct voices", (unsigned)voices[repeated], repeated, n);
      return MLGPU_ERR_INVALID;
    }
  }
  nEntries = n + spare;
  return MLGPU_OK;
}

void RecordPlan::pack(const uint32_t* voices, size_t n, bool import, uint32_t* dst) const
{
  if (!segs.empty()) memcpy(dst, segs.data(), sizeof(Segment) * segs.size());
  Entry* e = (Entry*)(dst + segs.size() * (sizeof(Segment) / 4));
  size_t k = 0;
  for (size_t i = 0; i < n; ++i) e[k++] = Entry{voices[i], (uint32_t)i};
  if (import && spareLanes)
    for (size_t i = 0; i < n; ++i)
      if (voices[i] == V - 1)
        for (size_t s = V; s < ((V + 63) & ~(size_t)63); ++s) e[k++] = Entry{(uint32_t)s, (uint32_t)i};
}
}  // namespace mlrec
