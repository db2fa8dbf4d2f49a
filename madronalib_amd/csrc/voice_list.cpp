// voice_list.cpp — see voice_list.hpp
#include "voice_list.hpp"

#include <stdio.h>

namespace mlvl
{
int validate(const uint32_t* list, size_t n, size_t nVoices, size_t reserved, char* err, size_t errLen)
{
  if (err && errLen) err[0] = 0;
  if (n == 0) return MLGPU_OK;
  if (!list)
  {
    if (err) snprintf(err, errLen, "null voice list of %zu entries", n);
    return MLGPU_ERR_INVALID;
  }
  if (reserved && n > reserved)
  {
    if (err) snprintf(err, errLen, "the list has %zu entries, reserve_voice_list reserved %zu", n, reserved);
    return MLGPU_ERR_RANGE;
  }
  for (size_t i = 0; i < n; ++i)
  {
    if (i > 0 && list[i] <= list[i - 1])
    {
      if (err) snprintf(err, errLen, "not strictly ascending at position %zu: voice %u after voice %u", i, list[i], list[i - 1]);
      return MLGPU_ERR_INVALID;
    }
    if ((size_t)list[i] >= nVoices)
    {
      if (err) snprintf(err, errLen, "voice %u at position %zu is out of range: the bank has %zu voices", list[i], i, nVoices);
      return MLGPU_ERR_RANGE;
    }
  }
  return MLGPU_OK;
}

LanePlan planGroups(const uint32_t* list, size_t n, unsigned G, uint32_t* lanes, uint32_t* groups)
{
  LanePlan plan{0, 0};
  size_t i = 0;
  while (i < n)
  {
    const uint32_t c = list[i] / G;
    size_t len = 1;
    while (i + len < n && list[i + len] / G == c) ++len;  // (ascending and distinct: at most G of them)
    const size_t room = kWave - plan.lanes % kWave;
    if (len > room)
    {
      for (size_t p = 0; p < room; ++p)
      {
        uint32_t* w = lanes + kLaneWords * (plan.lanes + p);
        w[0] = kPad;
        w[1] = w[2] = w[3] = 0;
      }
      plan.lanes += room;
    }
    for (size_t r = 0; r < len; ++r)
    {
      uint32_t* w = lanes + kLaneWords * (plan.lanes + r);
      w[0] = list[i + r];
      w[1] = (uint32_t)(i + r);
      w[2] = (uint32_t)plan.groups;
      w[3] = (uint32_t)r | ((uint32_t)len << 8);
    }
    groups[plan.groups++] = c;
    plan.lanes += len;
    i += len;
  }
  return plan;
}
}  // namespace mlvl
