// voice_records.hip — the DEVICE half of voice records (mlgpu_graph_export_voices / _import_voices and the bank's), and the staging
// both owners share (graph.hip, capi.hip).
//
// voice_records.cpp lays a voice's whole state out as a record of W words and turns a call's voice list into segments (the pieces of
// a record: a table's rows, a node's ring words) and entries (voice slot, record); here one launch of voice_records_kernel on the
// engine's stream gathers tables + ring memory -> records [n][W] or scatters them back, behind the asynchronous upload of the
// segments and entries from one of two pinned staging sets that take turns ("Staging turns").
#include <string.h>

#include <algorithm>
#include <string>

#include "mlgpu_internal.hpp"

using mlrec::Entry;
using mlrec::Segment;

namespace
{
struct RecordArgs
{
  const uint4* segs;     // two per segment (mlrec::Segment)
  const uint2* entries;  // {voice slot, record}
  uint32_t* tables[mlupd::kTables];  // params, coefficients, state, input constants: rows of V words each (null: the object has none)
  uint32_t* mem;         // a graph's ring memory ...
  uint64_t memWords;     // ... and its size: nothing is loaded or stored beyond it
  uint32_t* records;     // [records][W], 16-byte aligned
  uint64_t V, W, nEntries;
  uint32_t granule;      // 1, 8 or 16 ring words a voice owns in one piece
  uint32_t padOff, padWords;  // the words between the table words and the next multiple of 4: export writes them as zeros
};

constexpr uint32_t kLaneQuads = 8;  // 16-byte quads of one record a lane moves per item (mlgpu_recorder_move sizes the grid by it)

template <bool kImport>
__device__ __forceinline__ void move1(uint32_t* __restrict__ own, uint32_t* __restrict__ rec)
{
  if (kImport)
    *own = *rec;
  else
    *rec = *own;
}

// One segment of every entry's record. A table: items are (row, entry), the entry fastest - neighbouring listed voices are
// neighbours in a row, and a short list (one instrument of 16 voices) still fills a wavefront with four rows. A node's rings: items
// are 16-byte quads of the record. In the windowed layouts (granule G = 8 or 16: G / 4 quads contiguous per voice and chunk, the
// voices of a 256-voice block side by side) the order is (chunk, entry, quad): a wavefront's lanes cover the chunk's words of
// neighbouring voices - 16 adjacent voices are 512 or 1 024 contiguous bytes of ring memory - with one 16-byte access per lane on
// either side. In layout ROWS (granule 1) a quad is four ring rows: four dword accesses, each coalesced over neighbouring voices,
// against one 16-byte access of the record; a single voice is a sector per word there by the layout's nature. A lane takes
// kLaneQuads consecutive chunks (quads, in layout ROWS) of its voice, so that the record's side, whose voices lie W words apart, is
// written and read in runs of 128 to 512 bytes: with one quad per lane all 262 144 voices of a string bank moved at 0.13 to 0.41 of
// a device copy's rate, in this form at 0.43 to 0.63 of it (profiles/voice_records.md has the figures of this form).
// Index: items of a segment in 32 bits where they fit (the divisions), else in 64. Every offset is 64-bit: ring memory and n * W can
// exceed 4 GiB. Every access to the object's own memory is checked against its size.
template <bool kImport, class Index>
__device__ __forceinline__ void move_segment(const RecordArgs& a, uint64_t base, uint32_t rows, uint32_t recOff, uint32_t where)
{
  const Index nE = (Index)a.nEntries;
  const Index stride = (Index)gridDim.x * 256u;
  const Index first = (Index)blockIdx.x * 256u + threadIdx.x;
  if (where < mlrec::kRing)
  {
    uint32_t* const table = a.tables[where];
    if (!table) return;
    const Index items = (Index)rows * nE;
    for (Index i = first; i < items; i += stride)
    {
      const Index row = i / nE, e = i - row * nE;
      const uint2 ent = a.entries[e];
      if (ent.x >= a.V) continue;  // (a spare lane's slot: rings only)
      move1<kImport>(table + (uint64_t)row * a.V + ent.x, a.records + (uint64_t)ent.y * a.W + recOff + row);
    }
    return;
  }
  // a lane's item is kLaneQuads consecutive quads of one record: its loads are all in flight before its first store, and its accesses
  // to the record make one run of up to kLaneQuads * 16 bytes, issued back to back, where the records [n][W] lie W words apart
  if (a.granule == 1u)
  {
    const uint32_t nQuads = rows >> 2;
    const Index items = (Index)((nQuads + kLaneQuads - 1u) / kLaneQuads) * nE;
    for (Index i = first; i < items; i += stride)
    {
      const Index kg = i / nE, e = i - kg * nE;
      const uint2 ent = a.entries[e];
      if (ent.x >= a.V) continue;
      const uint32_t k0 = (uint32_t)kg * kLaneQuads;
      uint4* const rec = (uint4*)(a.records + (uint64_t)ent.y * a.W + recOff + (uint64_t)k0 * 4u);
      uint32_t* const m = a.mem + base + (uint64_t)k0 * 4u * a.V + ent.x;
      // (the quad's last word is the furthest: memory of the quads before it lies below)
      const uint64_t last = base + (uint64_t)k0 * 4u * a.V + ent.x + 3u * a.V;
      uint4 v[kLaneQuads];
#pragma unroll
      for (uint32_t u = 0; u < kLaneQuads; ++u)
      {
        v[u] = make_uint4(0u, 0u, 0u, 0u);
        const uint32_t* const mu = m + (uint64_t)u * 4u * a.V;
        if (k0 + u < nQuads && last + (uint64_t)u * 4u * a.V < a.memWords) v[u] = kImport ? rec[u] : make_uint4(mu[0], mu[a.V], mu[2u * a.V], mu[3u * a.V]);
      }
#pragma unroll
      for (uint32_t u = 0; u < kLaneQuads; ++u)
      {
        uint32_t* const mu = m + (uint64_t)u * 4u * a.V;
        if (k0 + u < nQuads && last + (uint64_t)u * 4u * a.V < a.memWords)
        {
          if (kImport)
          {
            mu[0] = v[u].x;
            mu[a.V] = v[u].y;
            mu[2u * a.V] = v[u].z;
            mu[3u * a.V] = v[u].w;
          }
          else
            rec[u] = v[u];
        }
      }
    }
    return;
  }
  const uint32_t G = a.granule, qShift = G == 16u ? 2u : 1u;  // G / 4 quads per chunk
  const uint32_t nChunks = rows / G;
  const Index perChunk = nE << qShift;
  const Index items = (Index)((nChunks + kLaneQuads - 1u) / kLaneQuads) * perChunk;
  for (Index i = first; i < items; i += stride)
  {
    const Index kg = i / perChunk, r = i - kg * perChunk, e = r >> qShift;
    const uint32_t q = (uint32_t)(r & ((1u << qShift) - 1u));
    const uint2 ent = a.entries[e];
    const uint32_t k0 = (uint32_t)kg * kLaneQuads;
    const uint64_t at = base + (uint64_t)(ent.x >> 8) * rows * 256u + (uint64_t)(ent.x & 255u) * G + (uint64_t)k0 * 256u * G + q * 4u;
    uint32_t* const rec = a.records + (uint64_t)ent.y * a.W + recOff + (uint64_t)k0 * G + q * 4u;
    uint4 v[kLaneQuads];
#pragma unroll
    for (uint32_t u = 0; u < kLaneQuads; ++u)
    {
      v[u] = make_uint4(0u, 0u, 0u, 0u);
      if (k0 + u < nChunks && at + (uint64_t)u * 256u * G + 4u <= a.memWords) v[u] = kImport ? *(const uint4*)(rec + u * G) : *(const uint4*)(a.mem + at + (uint64_t)u * 256u * G);
    }
#pragma unroll
    for (uint32_t u = 0; u < kLaneQuads; ++u)
    {
      if (k0 + u < nChunks && at + (uint64_t)u * 256u * G + 4u <= a.memWords)
      {
        if (kImport)
          *(uint4*)(a.mem + at + (uint64_t)u * 256u * G) = v[u];
        else
          *(uint4*)(rec + u * G) = v[u];
      }
    }
  }
}

// grid.y is the segment (wave-uniform: its two slots are scalar loads), grid.x * 256 lanes stride its items
template <bool kImport>
__global__ __launch_bounds__(256) void voice_records_kernel(const RecordArgs a)
{
  const uint32_t seg = (uint32_t)__builtin_amdgcn_readfirstlane((int)blockIdx.y);
  const uint4 lo = a.segs[2u * seg], hi = a.segs[2u * seg + 1u];  // {base lo, base hi, rows, recOff}, {where, -, -, -}
  const uint64_t base = ((uint64_t)lo.y << 32) | lo.x;
  // a record's words between its table words and its rings belong to no segment: the first segment's workgroups zero them on export
  if (!kImport && seg == 0u && a.padWords != 0u)
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < a.nEntries * a.padWords; i += (uint64_t)gridDim.x * 256u)
    {
      const uint64_t e = i / a.padWords;
      a.records[(uint64_t)a.entries[e].y * a.W + a.padOff + (i - e * a.padWords)] = 0u;
    }
  // the most items a segment can have: a quad or a word per (row, entry); 32 bits with room for the loop's last step (at most 2^22)
  if ((uint64_t)lo.z * a.nEntries < ((uint64_t)1 << 31))
    move_segment<kImport, uint32_t>(a, base, lo.z, lo.w, hi.x);
  else
    move_segment<kImport, uint64_t>(a, base, lo.z, lo.w, hi.x);
}
}  // namespace

static int rfail(std::string& err, int status, const std::string& what)
{
  err = what;
  return status;
}

// the entries of one call: record indices and slots are 32-bit, and a reserve is a pinned allocation of 8 bytes per voice
static constexpr size_t kMaxVoicesPerCall = (size_t)1 << 28;

int mlgpu_recorder_reserve(mlgpu_engine* e, mlgpu_recorder& r, size_t maxVoices, std::string& err)
{
  if (e->recording) return rfail(err, MLGPU_ERR_INVALID, "reserve_voice_records allocates: not while recording a sequence");
  if (maxVoices == 0 || maxVoices > kMaxVoicesPerCall) return rfail(err, MLGPU_ERR_INVALID, "reserve_voice_records: 1 .. 2^28 voices");
  if (hipSetDevice(e->device) != hipSuccess) return rfail(err, MLGPU_ERR_HIP, "hipSetDevice");
  // (launches that read the old buffers may be in flight)
  if (hipStreamSynchronize(e->stream()) != hipSuccess) return rfail(err, MLGPU_ERR_HIP, "reserve_voice_records: hipStreamSynchronize");
  r.stage.drained();
  if (!r.stage.create()) return rfail(err, MLGPU_ERR_HIP, "reserve_voice_records: hipEventCreate");
  const size_t words = r.plan.uploadWordsFor(mlrec::RecordPlan::maxEntries(maxVoices));
  for (mlgpu_recorder::Set& sg : r.stage.set)
    if (!growPair(sg.h_words, sg.d_words, sg.capacity, words, words)) return rfail(err, MLGPU_ERR_OOM, "reserve_voice_records: staging buffers");
  r.reserved = maxVoices;
  return MLGPU_OK;
}

int mlgpu_recorder_move(mlgpu_engine* e, mlgpu_recorder& r, uint32_t* const* tables, uint32_t* ringMem, size_t ringMemWords, const uint32_t* h_voices, size_t n,
                        uint32_t* d_records, bool import, std::string& err)
{
  const std::string who = import ? "import_voices: " : "export_voices: ";
  if (n == 0) return MLGPU_OK;
  if (!h_voices || !d_records) return rfail(err, MLGPU_ERR_INVALID, who + "null pointer");
  if (((uintptr_t)d_records & 15u) != 0) return rfail(err, MLGPU_ERR_INVALID, who + "the record buffer is not 16-byte aligned");
  if (e->recording) return rfail(err, MLGPU_ERR_INVALID, who + "reads host memory: not while recording a sequence (call between the sequence's launches)");
  if (r.reserved && n > r.reserved)
    return rfail(err, MLGPU_ERR_RANGE, who + std::to_string(n) + " voices, reserve_voice_records reserved " + std::to_string(r.reserved));
  if (n > kMaxVoicesPerCall) return rfail(err, MLGPU_ERR_RANGE, who + "more than 2^28 voices in one call");
  // everything that can be refused is refused before anything is enqueued
  const int vst = r.plan.validate(h_voices, n, import);
  if (vst != MLGPU_OK) return rfail(err, vst, who + r.plan.error());
  const std::vector<Segment>& segs = r.plan.segments();
  for (const Segment& s : segs)
    if (s.where == mlrec::kRing ? !ringMem : !tables[s.where]) return rfail(err, MLGPU_ERR_INVALID, who + "the object's memory is not there");
  if (hipSetDevice(e->device) != hipSuccess) return rfail(err, MLGPU_ERR_HIP, "hipSetDevice");
  auto* const taken = r.stage.take();
  if (!taken) return rfail(err, MLGPU_ERR_HIP, who + "waiting for the call before last");
  auto& sg = *taken;
  if (!sg.turn.create()) return rfail(err, MLGPU_ERR_HIP, who + "hipEventCreate");  // (no reserve: the event is made here)
  // after a reserve both sets hold the reserve's words and nothing is allocated here, ever; without one the buffers grow here, a
  // setup convenience that allocates and may wait (nothing of this set is in flight: it was taken)
  const size_t words = r.plan.uploadWords();
  if (!r.reserved && !growPair(sg.h_words, sg.d_words, sg.capacity, words, std::max<size_t>(1024, 2 * words))) return rfail(err, MLGPU_ERR_OOM, who + "staging buffers");
  r.plan.pack(h_voices, n, import, sg.h_words.get());
  hipError_t herr = hipMemcpyAsync(sg.d_words.get(), sg.h_words.get(), sizeof(uint32_t) * words, hipMemcpyHostToDevice, e->stream());
  if (herr == hipSuccess)
  {
    RecordArgs a;
    a.segs = (const uint4*)sg.d_words.get();
    a.entries = (const uint2*)(sg.d_words.get() + segs.size() * (sizeof(Segment) / 4));
    for (uint32_t t = 0; t < mlupd::kTables; ++t) a.tables[t] = tables[t];
    a.mem = ringMem;
    a.memWords = ringMemWords;
    a.records = d_records;
    a.V = r.plan.voices();
    a.W = r.plan.words();
    a.nEntries = r.plan.entries();
    a.granule = r.plan.granule();
    a.padOff = (uint32_t)r.plan.tableWords();
    a.padWords = (uint32_t)((0 - r.plan.tableWords()) & 3u);
    // grid.x: a lane per item of the largest segment, within 16 384 workgroups of a segment (the rest is the kernel's loop)
    uint64_t items = 1;
    for (const Segment& s : segs)
    {
      const uint64_t quads = s.rows / 4u, perLane = (uint64_t)kLaneQuads * (a.granule == 1u ? 1u : a.granule / 4u);  // (a ring: kLaneQuads chunks of each quad of the granule)
      items = std::max<uint64_t>(items, s.where == mlrec::kRing ? (quads + perLane - 1u) / perLane * (a.granule == 1u ? 1u : a.granule / 4u) * a.nEntries : (uint64_t)s.rows * a.nEntries);
    }
    const uint32_t gx = (uint32_t)std::min<uint64_t>((items + 255u) / 256u, 16384u);
    const dim3 grid(gx, (uint32_t)segs.size());
    if (import)
      hipLaunchKernelGGL(voice_records_kernel<true>, grid, dim3(256), 0, e->stream(), a);
    else
      hipLaunchKernelGGL(voice_records_kernel<false>, grid, dim3(256), 0, e->stream(), a);
    herr = hipGetLastError();
  }
  sg.turn.submitted(e->stream());  // (after a failed copy or launch too)
  if (herr != hipSuccess) return rfail(err, MLGPU_ERR_HIP, who + hipGetErrorString(herr));
  return MLGPU_OK;
}

// what the tests look at: the staging buffers' addresses {host 0, device 0, host 1, device 1} and the smaller capacity, in words
size_t mlgpu_recorder_staging(const mlgpu_recorder& r, const void** four)
{
  for (int i = 0; i < 2; ++i)
  {
    four[2 * i] = r.stage.set[i].h_words.get();
    four[2 * i + 1] = r.stage.set[i].d_words.get();
  }
  return std::min(r.stage.set[0].capacity, r.stage.set[1].capacity);
}
