// voice_tails.cpp — see voice_tails.hpp
#include "voice_tails.hpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "voice_list.hpp"

namespace mltail
{
// How the bookkeeping meets the header's rule without a walk over the voices and without keeping the lists that were never noted:
//   * a voice of a must-set is stamped when its list is MADE: lastMust_[v] = the list's number, quiet_[v] = 0;
//   * taking in launch j resets every voice of L_j that was loud or whose stamp is j or later, and adds to the others.
// While a voice's stamp lies beyond c, the last launch taken in, its count stays 0 - every launch taken in is at or before the stamp -
// which keeps the voice as the rule's second clause does; once c has reached the stamp, the count holds exactly the quiet launches
// after the stamp's list that were taken in since the last loud one - what taking in the must-sets' resets in order, noted lists or
// not, leaves. A list that was never noted therefore needs no slot and no turn: its resets are in the stamps already.
Tails::~Tails()
{
  for (unsigned s = 0; s < kMaxDepth; ++s)
  {
    if (slot_[s].event) api_.destroy(api_.ctx, slot_[s].event);
    free(slot_[s].list);
  }
  free(quiet_);
  free(lastMust_);
  free(cur_);
  free(next_);
}

int Tails::init(size_t nVoices, size_t maxListed, unsigned depth, const Api& api, const uint64_t* const* words)
{
  if (depth_ != 0 || nVoices == 0 || nVoices > ((size_t)1 << 32) || maxListed == 0 || depth == 0 || depth > kMaxDepth || !words)
  {
    snprintf(err_, sizeof(err_), "1 .. 2^32 voices, 1+ listed, a depth of 1 .. %u", kMaxDepth);
    return MLGPU_ERR_INVALID;
  }
  if (maxListed > nVoices) maxListed = nVoices;
  api_ = api;
  // calloc: the operating system's zero pages, not a walk
  quiet_ = (uint32_t*)calloc(nVoices, sizeof(uint32_t));
  lastMust_ = (uint64_t*)calloc(nVoices, sizeof(uint64_t));
  cur_ = (uint32_t*)calloc(maxListed, sizeof(uint32_t));
  next_ = (uint32_t*)calloc(maxListed, sizeof(uint32_t));
  bool ok = quiet_ && lastMust_ && cur_ && next_;
  for (unsigned s = 0; ok && s < depth; ++s)
  {
    words_[s] = words[s];
    slot_[s].list = (uint32_t*)calloc(maxListed, sizeof(uint32_t));
    ok = slot_[s].list && words_[s];
  }
  if (!ok)
  {
    snprintf(err_, sizeof(err_), "out of host memory for %zu voices, %zu listed", nVoices, maxListed);
    return MLGPU_ERR_OOM;
  }
  for (unsigned s = 0; s < depth; ++s)
    if (!api_.create(api_.ctx, &slot_[s].event))
    {
      slot_[s].event = nullptr;
      snprintf(err_, sizeof(err_), "creating an event");
      return MLGPU_ERR_HIP;
    }
  nVoices_ = nVoices;
  maxListed_ = maxListed;
  depth_ = depth;
  return MLGPU_OK;
}

int Tails::setThreshold(uint32_t quietBits, uint32_t holdVectors)
{
  if (holdVectors == 0)
  {
    snprintf(err_, sizeof(err_), "hold_vectors is 1 or more");
    return MLGPU_ERR_INVALID;
  }
  quietBits_ = quietBits;
  hold_ = holdVectors;
  return MLGPU_OK;
}

void Tails::clear()
{
  // (the counts and stamps of the voices stay as they are: a voice comes back only through a must-set, which stamps it anew with a
  // number beyond every stamp there is)
  head_ = count_ = 0;
  curN_ = 0;
  awaiting_ = false;
}

void Tails::takeIn(const Slot& s, const uint64_t* words)
{
  for (size_t i = 0; i < s.K; ++i)
  {
    const uint32_t v = s.list[i];
    const bool loud = (words[i >> 6] >> (i & 63)) & 1u;
    if (loud || lastMust_[v] >= s.number)
      quiet_[v] = 0;
    else
      quiet_[v] = s.vectors > UINT32_MAX - quiet_[v] ? UINT32_MAX : quiet_[v] + s.vectors;
  }
}

void Tails::dropFront()
{
  head_ = (head_ + 1) % depth_;
  --count_;
}

int Tails::takeInComplete()
{
  while (count_ > 0)
  {
    const Slot& s = slot_[head_];
    const int done = api_.query(api_.ctx, s.event);
    if (done < 0)
    {
      snprintf(err_, sizeof(err_), "asking whether the result of list %llu is there", (unsigned long long)s.number);
      return MLGPU_ERR_HIP;
    }
    if (done == 0) break;
    takeIn(s, words_[head_]);
    dropFront();
  }
  return MLGPU_OK;
}

int Tails::wait()
{
  while (count_ > 0)
  {
    const Slot& s = slot_[head_];
    if (!api_.wait(api_.ctx, s.event))
    {
      snprintf(err_, sizeof(err_), "waiting for the result of list %llu", (unsigned long long)s.number);
      return MLGPU_ERR_HIP;
    }
    takeIn(s, words_[head_]);
    dropFront();
  }
  return MLGPU_OK;
}

int Tails::nextList(const uint32_t* must, size_t nMust, uint32_t* list, size_t capacity, size_t* n)
{
  if (n) *n = 0;
  if (depth_ == 0 || !n || (!list && capacity > 0))
  {
    snprintf(err_, sizeof(err_), "null pointer");
    return MLGPU_ERR_INVALID;
  }
  const int vst = mlvl::validate(must, nMust, nVoices_, 0, err_, sizeof(err_));
  if (vst != MLGPU_OK) return vst;
  // (taking in is no change of the rule's outcome: a refusal below leaves the lists and their numbering as they were)
  const int tst = takeInComplete();
  if (tst != MLGPU_OK) return tst;
  // the ascending union of the must-set and the kept voices of L_m, into next_ (a voice of a must-set not yet taken in has a count
  // of 0: the rule's second clause is in the first)
  size_t i = 0, j = 0, k = 0;
  while (i < curN_ || j < nMust)
  {
    uint32_t v;
    if (j < nMust && (i >= curN_ || must[j] <= cur_[i]))
    {
      v = must[j];
      if (i < curN_ && cur_[i] == v) ++i;
      ++j;
    }
    else
    {
      v = cur_[i++];
      if (quiet_[v] >= hold_) continue;
    }
    if (k < maxListed_) next_[k] = v;
    ++k;
  }
  *n = k;
  if (k > maxListed_ || k > capacity)
  {
    snprintf(err_, sizeof(err_), "the list has %zu voices: max_listed is %zu, the capacity %zu", k, maxListed_, capacity);
    return MLGPU_ERR_RANGE;
  }
  ++made_;
  for (j = 0; j < nMust; ++j)
  {
    lastMust_[must[j]] = made_;
    quiet_[must[j]] = 0;
  }
  uint32_t* const t = cur_;
  cur_ = next_;
  next_ = t;
  curN_ = k;
  awaiting_ = true;
  if (k) memcpy(list, cur_, sizeof(uint32_t) * k);
  return MLGPU_OK;
}

int Tails::note(size_t nVectors, const uint32_t* d_peak)
{
  if (depth_ == 0 || !awaiting_)
  {
    snprintf(err_, sizeof(err_), "no list is waiting for its peaks (one note for every next_list)");
    return MLGPU_ERR_INVALID;
  }
  if (!d_peak || ((uintptr_t)d_peak & 3u) != 0)
  {
    snprintf(err_, sizeof(err_), "null or misaligned peaks");
    return MLGPU_ERR_INVALID;
  }
  awaiting_ = false;  // whatever happens below: a list that is not noted now is never noted
  if (curN_ == 0) return MLGPU_OK;  // nothing to ask the device: complete at once
  if (count_ == depth_)
  {
    snprintf(err_, sizeof(err_), "%u results are outstanding: the list goes without its peaks", depth_);
    return MLGPU_ERR_BUSY;
  }
  const unsigned at = (head_ + count_) % depth_;
  Slot& s = slot_[at];
  if (!api_.launch(api_.ctx, at, d_peak, curN_, quietBits_))
  {
    snprintf(err_, sizeof(err_), "enqueueing the loud bits");
    return MLGPU_ERR_HIP;
  }
  if (!api_.record(api_.ctx, s.event))
  {
    snprintf(err_, sizeof(err_), "recording the event");
    return MLGPU_ERR_HIP;
  }
  memcpy(s.list, cur_, sizeof(uint32_t) * curN_);
  s.K = curN_;
  s.number = made_;
  s.vectors = nVectors > UINT32_MAX ? UINT32_MAX : (uint32_t)nVectors;
  ++count_;
  return MLGPU_OK;
}
}  // namespace mltail
