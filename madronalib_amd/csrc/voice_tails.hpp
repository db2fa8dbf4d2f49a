// voice_tails.hpp — the HOST half of voice tails (mlgpu_tails_*, include/mlgpu.h: VOICE TAILS): which of the voices listed earlier
// have died away, decided from the loud bits of every noted launch without ever waiting for the device. The rule is the header's;
// this is its bookkeeping. Plain C++ that never touches a device: built and tested without any HIP header. Whatever needs one - the
// events, and the kernel and copy behind a note - comes in through `Api` (voice_tails.hip binds HIP, tests/cpp/voice_tails_test.cpp
// a fake whose events complete when the test says and which counts the waits).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/mlgpu.h"

namespace mltail
{
constexpr unsigned kMaxDepth = 8;

struct Api
{
  void* ctx;
  bool (*create)(void* ctx, void** event);
  void (*destroy)(void* ctx, void* event);
  // the loud bits of peak[0 .. K) against quietBits into the slot's words, enqueued where `record` records (K > 0)
  bool (*launch)(void* ctx, unsigned slot, const uint32_t* d_peak, size_t K, uint32_t quietBits);
  bool (*record)(void* ctx, void* event);
  int (*query)(void* ctx, void* event);  // 1: complete, 0: not yet, negative: the query failed
  bool (*wait)(void* ctx, void* event);
};

class Tails
{
 public:
  Tails() = default;
  Tails(const Tails&) = delete;
  Tails& operator=(const Tails&) = delete;
  ~Tails();

  // Setup, the one place that allocates. words[s]: where slot s's loud bits arrive, wordsFor(maxListed) 64-bit words each, the
  // caller's (pinned) memory; bit i % 64 of word i / 64 is list position i. MLGPU_ERR_INVALID / _OOM / _HIP (an event).
  int init(size_t nVoices, size_t maxListed, unsigned depth, const Api& api, const uint64_t* const* words);
  static size_t wordsFor(size_t K) { return (K + 63) / 64; }

  int setThreshold(uint32_t quietBits, uint32_t holdVectors);
  // no list, every voice as never listed, the outstanding results given up (what is in flight lands in its own slot's words, and a
  // later note of that slot is enqueued behind it)
  void clear();
  int nextList(const uint32_t* must, size_t nMust, uint32_t* list, size_t capacity, size_t* n);
  int note(size_t nVectors, const uint32_t* d_peak);
  size_t pending() const { return count_; }
  int wait();

  size_t maxListed() const { return maxListed_; }
  uint32_t quietBits() const { return quietBits_; }
  const char* error() const { return err_; }

 private:
  struct Slot
  {
    void* event{nullptr};
    uint32_t* list{nullptr};  // the host's copy of the noted list
    size_t K{0};
    uint64_t number{0};  // j of L_j
    uint32_t vectors{0};
  };
  void takeIn(const Slot& s, const uint64_t* words);
  int takeInComplete();
  void dropFront();

  Api api_{};
  size_t nVoices_{0}, maxListed_{0};
  unsigned depth_{0}, head_{0}, count_{0};  // the outstanding results: slots head_ .. head_ + count_ - 1 (mod depth_), oldest first
  Slot slot_[kMaxDepth];
  const uint64_t* words_[kMaxDepth]{};
  uint32_t* quiet_{nullptr};      // [nVoices] quiet DSPVectors behind a voice (0 while lastMust_ is beyond what was taken in)
  uint64_t* lastMust_{nullptr};   // [nVoices] the number of the last list whose must-set held the voice
  uint32_t* cur_{nullptr};        // L_m ...
  uint32_t* next_{nullptr};       // ... and where L_m+1 is made
  size_t curN_{0};
  uint64_t made_{0};              // m
  bool awaiting_{false};          // L_m has not been noted
  uint32_t quietBits_{0x38d1b717u}, hold_{1};  // 1e-4f, one DSPVector
  char err_[200]{};
};
}  // namespace mltail
