// updates.hip — the DEVICE half of sparse per-voice table updates, and the staging both callers share (graph.hip, capi.hip).
//
// param_updates.cpp turns a list of mlgpu_update records into batches of 16-byte device records none of which writes a word twice;
// here a batch is one launch of apply_updates_kernel on the engine's stream, behind the asynchronous upload of its records from one
// of two pinned staging sets that take turns ("Staging turns"). The ring records of MLGPU_UPDATE_CLEAR_RINGS lie behind the table records in the same upload and
// are one launch of clear_rings_kernel.
#include <string.h>

#include <algorithm>
#include <string>

#include "mlgpu_internal.hpp"

using mlupd::DevRec;
using mlupd::RingRec;

namespace
{
struct UpdateArgs
{
  const uint4* recs;
  uint32_t* tables[mlupd::kTables];  // params, coefficients, state, input constants: rows of V words each (null: the object has none)
  size_t V;
  uint32_t n;
};

// One wavefront per record, its lanes striding the record's voices in coalesced dword stores: the same launch serves very many
// short ranges (100 000 instruments of 16 voices: a quarter of a wavefront's lanes each) and a few long ones (a whole row of 2^20
// voices: 16 384 trips of one wavefront). The kernel moves a few MB at most and is bound by latency, not bandwidth. A record is
// the same for every lane: its index goes through readfirstlane so that the record and the table's base are scalar loads.
__global__ __launch_bounds__(256) void apply_updates_kernel(const UpdateArgs a)
{
  const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (w >= a.n) return;
  const uint4 r = a.recs[w];
  uint32_t* __restrict__ row = a.tables[r.x >> mlupd::kRowBits] + (size_t)(r.x & mlupd::kRowMask) * a.V + r.y;
  for (uint32_t i = threadIdx.x & 63u; i < r.z; i += 64u) row[i] = r.w;
}

struct RingClearArgs
{
  const uint4* recs;  // two per record (mlupd::RingRec)
  uint32_t* mem;      // the graph's ring memory ...
  uint64_t memWords;  // ... and its size: nothing is stored beyond it
  uint32_t wide;      // the ring layout's granule is 8 words or more: spans are 16-byte aligned multiples of 16 bytes
};

// Zeros to the strided spans of one ring record: `rows` spans of `span` words, `stride` words apart. The lanes of a wavefront go
// over the flattened (row, place in the span) space, so that one voice's clear - spans of 8 words in ring layout 4, of 1 word in
// layout 0 - keeps all 64 busy; a lane's store is W words (16 bytes where the layout's granule allows, a dword in layout 0). A
// record is cut into slabs of 16 KiB of stores, one per wavefront at a time: grid.x is the record, grid.y * 4 wavefronts stride
// its slabs, and a wavefront with no slab left (a short record next to a long one) leaves - every test on the way is wave-uniform.
// Offsets are 64-bit: a graph's ring memory can exceed 4 GiB.
constexpr uint32_t kSlabWords = 4096;

template <int W>
__device__ __forceinline__ void clear_ring_slabs(const RingClearArgs& a, uint64_t offset, uint32_t span, uint32_t stride, uint32_t rows, uint32_t wave)
{
  constexpr uint32_t kSlab = kSlabWords / W;  // stores per slab
  const uint32_t perSpan = span / W;
  if (!perSpan) return;
  const uint64_t stores = (uint64_t)rows * perSpan;
  const uint64_t nSlabs = (stores + kSlab - 1) / kSlab;
  for (uint64_t slab = (uint64_t)blockIdx.y * 4u + wave; slab < nSlabs; slab += (uint64_t)gridDim.y * 4u)
  {
    // the slab's first store: its row once per slab in 64 bits, every store's row from there in 32 (perSpan + kSlab fits easily)
    const uint64_t s0 = slab * kSlab, row0 = s0 / perSpan;
    const uint32_t rem0 = (uint32_t)(s0 - row0 * perSpan);
    const uint32_t count = (uint32_t)(stores - s0 < kSlab ? stores - s0 : kSlab);
    const uint64_t base = offset + row0 * stride;
    for (uint32_t j = threadIdx.x & 63u; j < count; j += 64u)
    {
      const uint32_t t = rem0 + j, r = t / perSpan, p = t - r * perSpan;
      const uint64_t at = base + (uint64_t)r * stride + (uint64_t)p * W;
      if (at + W > a.memWords) continue;
      if (W == 4)
        *(uint4*)(a.mem + at) = make_uint4(0u, 0u, 0u, 0u);
      else
        a.mem[at] = 0u;
    }
  }
}

__global__ __launch_bounds__(256) void clear_rings_kernel(const RingClearArgs a)
{
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t rec = (uint32_t)__builtin_amdgcn_readfirstlane((int)blockIdx.x);
  const uint4 lo = a.recs[2u * rec], hi = a.recs[2u * rec + 1u];  // {offset lo, offset hi, span, stride}, {rows, -, -, -}
  const uint64_t offset = ((uint64_t)lo.y << 32) | lo.x;
  if (a.wide)
    clear_ring_slabs<4>(a, offset, lo.z, lo.w, hi.x, wave);
  else
    clear_ring_slabs<1>(a, offset, lo.z, lo.w, hi.x, wave);
}
}  // namespace

static int ufail(std::string& err, int status, const std::string& what)
{
  err = what;
  return status;
}

// One batch is one launch of a 1-D grid of a wavefront per record, and a grid holds fewer than 2^32 threads: lists are held to what a
// single launch can take, at reserve and before anything of a list is enqueued
static constexpr size_t kMaxDeviceRecords = (size_t)1 << 25;

int mlgpu_updater_reserve(mlgpu_engine* e, mlgpu_updater& u, size_t maxDeviceRecords, std::string& err)
{
  if (e->recording) return ufail(err, MLGPU_ERR_INVALID, "reserve_updates allocates: not while recording a sequence");
  if (maxDeviceRecords == 0 || maxDeviceRecords > kMaxDeviceRecords) return ufail(err, MLGPU_ERR_INVALID, "reserve_updates: 1 .. 2^25 device records");
  if (hipSetDevice(e->device) != hipSuccess) return ufail(err, MLGPU_ERR_HIP, "hipSetDevice");
  // (launches that read the old buffers may be in flight)
  if (hipStreamSynchronize(e->stream()) != hipSuccess) return ufail(err, MLGPU_ERR_HIP, "reserve_updates: hipStreamSynchronize");
  u.stage.drained();
  if (!u.stage.create()) return ufail(err, MLGPU_ERR_HIP, "reserve_updates: hipEventCreate");
  for (mlgpu_updater::Set& sg : u.stage.set)
    if (!growPair(sg.h_recs, sg.d_recs, sg.capacity, maxDeviceRecords, maxDeviceRecords)) return ufail(err, MLGPU_ERR_OOM, "reserve_updates: record buffers");
  u.planner.reserve(maxDeviceRecords);
  u.reserved = maxDeviceRecords;
  return MLGPU_OK;
}

size_t mlgpu_updater_device_records(mlgpu_updater& u, const mlgpu_update* recs, size_t n)
{
  if (!recs || !n) return 0;
  return u.planner.validate(u.desc, recs, n) == MLGPU_OK ? u.planner.deviceRecords() : 0;
}

int mlgpu_updater_apply(mlgpu_engine* e, mlgpu_updater& u, uint32_t* const* tables, uint32_t* ringMem, size_t ringMemWords, const mlgpu_update* recs, size_t n,
                        std::string& err)
{
  if (n == 0) return MLGPU_OK;
  if (!recs) return ufail(err, MLGPU_ERR_INVALID, "apply_updates: null record list");
  if (e->recording) return ufail(err, MLGPU_ERR_INVALID, "apply_updates reads host memory: not while recording a sequence (apply between the sequence's launches)");
  // everything that can be refused is refused before anything is enqueued
  const int vst = u.planner.validate(u.desc, recs, n);
  if (vst != MLGPU_OK) return ufail(err, vst, std::string("apply_updates: ") + u.planner.error());
  const size_t nDev = u.planner.deviceRecords(), nTable = u.planner.tableRecords(), nRing = u.planner.ringRecords();
  if (nRing && !ringMem) return ufail(err, MLGPU_ERR_INVALID, "apply_updates: ring records without ring memory");
  if (nDev == 0) return MLGPU_OK;  // (a CLEAR of nodes without state words that clear() resets)
  if (u.reserved && nDev > u.reserved)
    return ufail(err, MLGPU_ERR_RANGE, "apply_updates: the list needs " + std::to_string(nDev) + " device records, reserve_updates reserved " + std::to_string(u.reserved));
  if (nDev > kMaxDeviceRecords || nRing >= kMaxDeviceRecords / 2) return ufail(err, MLGPU_ERR_RANGE, "apply_updates: more than 2^25 device records in one list");
  if (hipSetDevice(e->device) != hipSuccess) return ufail(err, MLGPU_ERR_HIP, "hipSetDevice");
  auto* const taken = u.stage.take();
  if (!taken) return ufail(err, MLGPU_ERR_HIP, "apply_updates: waiting for the call before last");
  auto& sg = *taken;
  if (!sg.turn.create()) return ufail(err, MLGPU_ERR_HIP, "apply_updates: hipEventCreate");  // (no reserve: the event is made here)
  // after a reserve both sets hold `reserved` records and nothing is allocated here, ever; without one the buffers grow here, a
  // setup convenience that allocates and may wait (nothing of this set is in flight: it was taken)
  if (!u.reserved && !growPair(sg.h_recs, sg.d_recs, sg.capacity, nDev, std::max<size_t>(1024, 2 * nDev))) return ufail(err, MLGPU_ERR_OOM, "apply_updates: record buffers");
  u.planner.pack(u.desc, recs, n, sg.h_recs.get());
  hipError_t herr = hipMemcpyAsync(sg.d_recs.get(), sg.h_recs.get(), sizeof(DevRec) * nDev, hipMemcpyHostToDevice, e->stream());
  UpdateArgs a;
  for (uint32_t t = 0; t < mlupd::kTables; ++t) a.tables[t] = tables[t];
  a.V = u.desc.V;
  size_t begin = 0;
  for (size_t b = 0; b < u.planner.batches() && herr == hipSuccess; ++b)
  {
    const size_t end = u.planner.batchEnd(b);
    a.recs = (const uint4*)(sg.d_recs.get() + begin);
    a.n = (uint32_t)(end - begin);
    hipLaunchKernelGGL(apply_updates_kernel, dim3(a.n / 4u + (a.n % 4u ? 1u : 0u)), dim3(256), 0, e->stream(), a);
    herr = hipGetLastError();
    begin = end;
  }
  if (nRing && herr == hipSuccess)
  {
    // grid.y: enough wavefronts for the longest record's slabs, within a million workgroups in all (the rest is the kernel's loop)
    const uint32_t wordsPerStore = u.desc.ringGranule >= 8 ? 4u : 1u, slab = kSlabWords / wordsPerStore;
    uint64_t slabs = 1;
    for (size_t i = 0; i < nRing; ++i)
    {
      RingRec rr;
      memcpy(&rr, sg.h_recs.get() + nTable + 2 * i, sizeof(rr));
      slabs = std::max<uint64_t>(slabs, ((uint64_t)rr.rows * (rr.span / wordsPerStore) + slab - 1) / slab);
    }
    const uint64_t y = std::max<uint64_t>(1, std::min<uint64_t>({(slabs + 3) / 4, (uint64_t)65535, ((uint64_t)1 << 20) / nRing}));
    RingClearArgs ra;
    ra.recs = (const uint4*)(sg.d_recs.get() + nTable);
    ra.mem = ringMem;
    ra.memWords = ringMemWords;
    ra.wide = wordsPerStore == 4u;
    hipLaunchKernelGGL(clear_rings_kernel, dim3((uint32_t)nRing, (uint32_t)y), dim3(256), 0, e->stream(), ra);
    herr = hipGetLastError();
  }
  sg.turn.submitted(e->stream());  // (after a failed copy or launch too)
  if (herr != hipSuccess) return ufail(err, MLGPU_ERR_HIP, std::string("apply_updates: ") + hipGetErrorString(herr));
  return MLGPU_OK;
}

// what the tests look at: the staging buffers' addresses {host 0, device 0, host 1, device 1} and the smaller capacity, in records
size_t mlgpu_updater_staging(const mlgpu_updater& u, const void** four)
{
  for (int i = 0; i < 2; ++i)
  {
    four[2 * i] = u.stage.set[i].h_recs.get();
    four[2 * i + 1] = u.stage.set[i].d_recs.get();
  }
  return std::min(u.stage.set[0].capacity, u.stage.set[1].capacity);
}
