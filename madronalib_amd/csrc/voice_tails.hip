// voice_tails.hip — the DEVICE half of voice tails and their C entry points (include/mlgpu.h: VOICE TAILS).
//
// voice_tails.cpp keeps the rule's books on the host. Here a note becomes, on the engine's stream: one launch of voice_tails_kernel,
// which turns the K peak words a listed process call wrote into ceil(K / 64) words of loud bits; their copy into the slot's pinned
// words; and an event behind both, which the host half only ever queries. `depth` slots, all sized at create.
#include <new>

#include "mlgpu_internal.hpp"
#include "voice_tails.hpp"

namespace
{
// One lane per list position, one 64-bit word per wavefront: bit l of word w says that d_peak[64 w + l] > quietBits, as unsigned
// integers (a NaN's bits are above every finite threshold's). Lanes at or beyond K vote 0, so the last word is clean for any K; a
// wavefront wholly beyond K (the last block's spare ones) stores nothing: words has ceil(K / 64) words.
__global__ __launch_bounds__(256) void voice_tails_kernel(const uint32_t* __restrict__ peak, unsigned long long* __restrict__ words, uint32_t K,
                                                          uint32_t quietBits)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const bool loud = i < K && peak[i] > quietBits;
  const unsigned long long bits = __ballot(loud);
  if ((threadIdx.x & 63u) == 0u && i < K) words[i >> 6] = bits;
}
}  // namespace

struct mlgpu_tails
{
  mlgpu_engine* e{nullptr};
  struct Slot
  {
    DeviceBuffer<unsigned long long> d_words;
    PinnedBuffer<unsigned long long> h_words;
  };
  Slot slot[mltail::kMaxDepth];
  size_t words{0};     // of every slot's two buffers: ceil(max_listed / 64)
  mltail::Tails host;  // (declared last: its events go first)
};

namespace
{
bool tailsCreateEvent(void*, void** event)
{
  hipEvent_t ev = nullptr;
  if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return false;
  *event = ev;
  return true;
}
void tailsDestroyEvent(void*, void* event) { hipEventDestroy((hipEvent_t)event); }
bool tailsLaunch(void* ctx, unsigned slot, const uint32_t* d_peak, size_t K, uint32_t quietBits)
{
  mlgpu_tails* const t = (mlgpu_tails*)ctx;
  mlgpu_tails::Slot& s = t->slot[slot];
  const size_t nWords = mltail::Tails::wordsFor(K);
  if (K == 0 || nWords > t->words) return false;  // (the host half never asks)
  hipStream_t stream = t->e->stream();
  hipLaunchKernelGGL(voice_tails_kernel, dim3((uint32_t)((K + 255u) / 256u)), dim3(256), 0, stream, d_peak, s.d_words.get(), (uint32_t)K, quietBits);
  if (hipGetLastError() != hipSuccess) return false;
  return hipMemcpyAsync(s.h_words.get(), s.d_words.get(), sizeof(unsigned long long) * nWords, hipMemcpyDeviceToHost, stream) == hipSuccess;
}
bool tailsRecord(void* ctx, void* event) { return hipEventRecord((hipEvent_t)event, ((mlgpu_tails*)ctx)->e->stream()) == hipSuccess; }
int tailsQuery(void*, void* event)
{
  const hipError_t err = hipEventQuery((hipEvent_t)event);
  return err == hipSuccess ? 1 : (err == hipErrorNotReady ? 0 : -1);
}
bool tailsWait(void*, void* event) { return hipEventSynchronize((hipEvent_t)event) == hipSuccess; }

int tailsFail(mlgpu_tails* t, int status, const char* who)
{
  t->e->lastError = std::string(who) + ": " + t->host.error();
  return status;
}
}  // namespace

extern "C"
{
  int mlgpu_tails_create(mlgpu_engine* e, size_t nVoices, size_t maxListed, int depth, mlgpu_tails** out)
  {
    if (!e || !out) return MLGPU_ERR_INVALID;
    *out = nullptr;
    if (e->recording)
    {
      e->lastError = "tails_create allocates: not while recording a sequence";
      return MLGPU_ERR_INVALID;
    }
    if (nVoices == 0 || maxListed == 0 || maxListed > ((size_t)1 << 28) || depth < 1 || depth > (int)mltail::kMaxDepth)
    {
      e->lastError = "tails_create: 1+ voices, 1 .. 2^28 listed, a depth of 1 .. 8";
      return MLGPU_ERR_INVALID;
    }
    std::unique_ptr<mlgpu_tails> t(new (std::nothrow) mlgpu_tails());
    if (!t) return MLGPU_ERR_OOM;
    t->e = e;
    t->words = mltail::Tails::wordsFor(maxListed < nVoices ? maxListed : nVoices);
    hipError_t err = hipSetDevice(e->device);
    const uint64_t* words[mltail::kMaxDepth] = {};
    for (int s = 0; err == hipSuccess && s < depth; ++s)
    {
      err = allocate(t->slot[s].d_words, t->words);
      if (err == hipSuccess) err = allocate(t->slot[s].h_words, t->words);
      words[s] = (const uint64_t*)t->slot[s].h_words.get();
    }
    if (err != hipSuccess)
    {
      e->lastError = std::string("tails_create: ") + hipGetErrorString(err);
      return err == hipErrorOutOfMemory ? MLGPU_ERR_OOM : MLGPU_ERR_HIP;
    }
    const mltail::Api api{t.get(), tailsCreateEvent, tailsDestroyEvent, tailsLaunch, tailsRecord, tailsQuery, tailsWait};
    const int st = t->host.init(nVoices, maxListed, (unsigned)depth, api, words);
    if (st != MLGPU_OK) return tailsFail(t.get(), st, "tails_create");
    *out = t.release();
    return MLGPU_OK;
  }

  int mlgpu_tails_destroy(mlgpu_tails* t)
  {
    if (!t) return MLGPU_ERR_INVALID;
    return t->e->release(t, "tails_destroy");  // (the stream is drained: every copy into the pinned words is over)
  }

  int mlgpu_tails_set_threshold(mlgpu_tails* t, uint32_t quietBits, uint32_t holdVectors)
  {
    if (!t) return MLGPU_ERR_INVALID;
    const int st = t->host.setThreshold(quietBits, holdVectors);
    return st == MLGPU_OK ? st : tailsFail(t, st, "tails_set_threshold");
  }

  int mlgpu_tails_clear(mlgpu_tails* t)
  {
    if (!t) return MLGPU_ERR_INVALID;
    t->host.clear();
    return MLGPU_OK;
  }

  int mlgpu_tails_next_list(mlgpu_tails* t, const uint32_t* h_must, size_t nMust, uint32_t* h_list, size_t capacity, size_t* n)
  {
    if (!t) return MLGPU_ERR_INVALID;
    const int st = t->host.nextList(h_must, nMust, h_list, capacity, n);
    return st == MLGPU_OK ? st : tailsFail(t, st, "tails_next_list");
  }

  int mlgpu_tails_note(mlgpu_tails* t, size_t nVectors, const uint32_t* d_peak)
  {
    if (!t) return MLGPU_ERR_INVALID;
    mlgpu_engine* const e = t->e;
    if (e->recording)
    {
      e->lastError = "tails_note: not while recording a sequence - the launch's size goes with the list, and its result is for the host to read";
      return MLGPU_ERR_INVALID;
    }
    if (hipSetDevice(e->device) != hipSuccess) return MLGPU_ERR_HIP;
    const int st = t->host.note(nVectors, d_peak);
    return st == MLGPU_OK ? st : tailsFail(t, st, "tails_note");
  }

  size_t mlgpu_tails_pending(mlgpu_tails* t) { return t ? t->host.pending() : 0; }

  int mlgpu_tails_wait(mlgpu_tails* t)
  {
    if (!t) return MLGPU_ERR_INVALID;
    if (t->e->recording)
    {
      t->e->lastError = "tails_wait waits for the device: not while recording a sequence";
      return MLGPU_ERR_INVALID;
    }
    const int st = t->host.wait();
    return st == MLGPU_OK ? st : tailsFail(t, st, "tails_wait");
  }
}
