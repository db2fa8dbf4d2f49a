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
}  // namespace mlvl
