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

// ---- the lane plan of a listed group sum (mlgpu_bank_process_listed_groups, mlgpu_graph_process_listed_groups) ----
// The bank's voices are instruments of G adjacent voices (G = 2, 4, 8, 16). The listed voices of one instrument - a SEGMENT, a
// maximal run of equal list[i] / G - are consecutive list positions, and their in-order float sum must not cross a wavefront: a
// segment that does not fit into what is left of the current 64 lanes starts at the next multiple of 64, the lanes in between are
// PADS that run nothing. One plan entry per lane, kLaneWords consecutive words:
//   [0] voice   list[i], or kPad
//   [1] pos     the list position i (a pad: 0)
//   [2] row     the output row j: the segment's number, 0 .. J-1 (a pad: 0)
//   [3] seg     rank | length << 8: the lane's place 0 .. length-1 in its segment, the segment's length 1 .. G (a pad: 0)
constexpr size_t kLaneWords = 4;
constexpr uint32_t kPad = 0xFFFFFFFFu;
constexpr size_t kWave = 64;

struct LanePlan
{
  size_t lanes;   // N: up to and including the last voice's lane (0 for an empty list)
  size_t groups;  // J: the listed instruments
};

// the most lanes a list of n voices can take: every wavefront but the last holds at least 65 - G voices. A multiple of 64.
inline size_t maxPlanLanes(size_t n, unsigned G) { return kWave * ((n + (kWave - G)) / (kWave + 1 - G)); }

// The plan of a VALID list (validate above) into lanes[kLaneWords * maxPlanLanes(n, G)] and the listed instruments M[0 .. J) - the
// distinct list[i] / G, ascending - into groups[J <= n]. Allocates nothing, touches nothing else: the arrays are the caller's pinned
// staging set. G must be 2, 4, 8 or 16.
LanePlan planGroups(const uint32_t* list, size_t n, unsigned G, uint32_t* lanes, uint32_t* groups);
}  // namespace mlvl
