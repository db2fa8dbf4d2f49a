// The host check of a bank's voice list (madronalib_amd/csrc/voice_list.cpp) without a device: built by g++ from that one file by
// tests/test_voice_list_cpu.py. Accepted: ascending lists, the empty list, a list exactly as long as the reserve. Refused, with the
// position in the message: an equal neighbour, a descending pair, an index out of range; and a list longer than the reserve.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../madronalib_amd/csrc/voice_list.hpp"

static int failures = 0;

static void expect(const char* what, const std::vector<uint32_t>& list, size_t nVoices, size_t reserved, int status, const char* inMessage)
{
  char msg[256];
  memset(msg, 'x', sizeof(msg));
  const int got = mlvl::validate(list.empty() ? nullptr : list.data(), list.size(), nVoices, reserved, msg, sizeof(msg));
  const bool terminated = memchr(msg, 0, sizeof(msg)) != nullptr;
  const bool said = terminated && (inMessage ? strstr(msg, inMessage) != nullptr : msg[0] == 0);
  if (got != status || !said)
  {
    ++failures;
    printf("FAILED %s: status %d (want %d), message \"%s\" (want \"%s\")\n", what, got, status, terminated ? msg : "<unterminated>", inMessage ? inMessage : "");
  }
}

int main()
{
  expect("ascending", {0, 1, 2, 7, 63, 64, 2351}, 2352, 0, MLGPU_OK, nullptr);
  expect("one voice, the last", {2351}, 2352, 0, MLGPU_OK, nullptr);
  expect("empty", {}, 2352, 0, MLGPU_OK, nullptr);
  expect("empty under a reserve", {}, 2352, 4, MLGPU_OK, nullptr);
  expect("as long as the reserve", {1, 2, 3, 4}, 2352, 4, MLGPU_OK, nullptr);
  expect("every voice", {0, 1, 2, 3}, 4, 4, MLGPU_OK, nullptr);
  expect("equal neighbours", {0, 5, 9, 9, 12}, 2352, 0, MLGPU_ERR_INVALID, "position 3");
  expect("equal neighbours at the start", {4, 4}, 2352, 0, MLGPU_ERR_INVALID, "position 1");
  expect("a descending pair", {0, 5, 9, 8, 12}, 2352, 0, MLGPU_ERR_INVALID, "position 3");
  expect("a descending pair at the end", {0, 5, 9, 10, 3}, 2352, 0, MLGPU_ERR_INVALID, "position 4");
  expect("out of range", {0, 5, 2352}, 2352, 0, MLGPU_ERR_RANGE, "position 2");
  expect("out of range, first", {7}, 7, 0, MLGPU_ERR_RANGE, "position 0");
  expect("out of range, far", {1, 0xFFFFFFFFu}, 2352, 0, MLGPU_ERR_RANGE, "position 1");
  expect("the first fault decides: order before a later range fault", {3, 2, 9999}, 2352, 0, MLGPU_ERR_INVALID, "position 1");
  expect("capacity exceeded", {1, 2, 3, 4, 5}, 2352, 4, MLGPU_ERR_RANGE, "reserved 4");
  {
    // a null list of n > 0 entries; and a null message buffer is allowed
    char msg[64];
    if (mlvl::validate(nullptr, 3, 10, 0, msg, sizeof(msg)) != MLGPU_ERR_INVALID || !strstr(msg, "null")) { ++failures; printf("FAILED null list\n"); }
    const uint32_t bad[2] = {5, 5};
    if (mlvl::validate(bad, 2, 10, 0, nullptr, 0) != MLGPU_ERR_INVALID) { ++failures; printf("FAILED null message buffer\n"); }
    // a short message buffer is terminated, not overrun
    char tiny[8];
    memset(tiny, 'x', sizeof(tiny));
    if (mlvl::validate(bad, 2, 10, 0, tiny, 4) != MLGPU_ERR_INVALID || tiny[3] != 0 || tiny[4] != 'x') { ++failures; printf("FAILED short message buffer\n"); }
  }
  if (failures == 0) printf("All tests passed\n");
  return failures ? 1 : 0;
}
