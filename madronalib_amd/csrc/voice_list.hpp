// voice_list.hpp — the HOST check of a bank's voice list (mlgpu_bank_set_voice_list): the indices of the voices a listed process call
// runs, strictly ascending and all below the bank's voice count. Ascending is not a convenience of the check: lane i of a listed
// launch gathers its voice's table words (4 bytes) and input quads (16 bytes) at index list[i], and 64 ascending indices touch each
// cache line they span once, in address order - nearly coalesced - where an unordered list would scatter them. Plain C++ that never
// touches a device: built and tested without any HIP header; capi.hip is the caller.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/mlgpu.h"

namespace mlvl
{
// MLGPU_OK, or the status of the first fault found with `err` (errLen bytes, always terminated) naming its position:
//   MLGPU_ERR_RANGE    more than `reserved` entries (reserved == 0: no reserve, any length), or list[i] >= nVoices
//   MLGPU_ERR_INVALID  a null list of n > 0 entries, or list[i] <= list[i - 1]
// The whole list is looked at before the answer: nothing is written anywhere but `err`. n == 0 is a valid, empty list.
int validate(const uint32_t* list, size_t n, size_t nVoices, size_t reserved, char* err, size_t errLen);
}  // namespace mlvl
