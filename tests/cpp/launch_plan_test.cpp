// The plan of a bank launch that goes out in up to four kernels on two streams (madronalib_amd/csrc/launch_parts.cpp: splitPlan)
// without a device: built by g++ from that one file, with -fsanitize=address,undefined, by tests/test_launch_plan_cpu.py. For every
// voice count of a sweep and every mode: the cuts ascend from 0 to V in whole units, no part is empty, the boundary between the
// streams is where the two-part launch has it; then the shapes each mode is there for, and the gate on short launches.
#include <cstdio>
#include <vector>

#include "../../madronalib_amd/csrc/launch_parts.hpp"

using namespace mlparts;

static int failures = 0;
#define EXPECT(cond)                                                                  \
  do                                                                                  \
  {                                                                                   \
    if (!(cond))                                                                      \
    {                                                                                 \
      if (++failures < 40) printf("FAILED line %d: %s (V = %zu, mode %d)\n", __LINE__, #cond, curV, curMode); \
    }                                                                                 \
  } while (0)
static size_t curV = 0;
static int curMode = 0;

static bool is(const Plan& p, int firstSide, std::vector<size_t> cuts)
{
  if (p.n != (int)cuts.size() - 1 || p.firstSide != firstSide) return false;
  for (size_t i = 0; i < cuts.size(); ++i)
    if (p.cut[i] != cuts[i]) return false;
  return true;
}

int main()
{
  const size_t CU = 256, WG = 256, T = 30;
  std::vector<size_t> sweep{0, 1, 255, 256, 2047, 2048, 2049, 2304, 4095, 4096, 4097, 6144, 8191, 8192, 8448, 65536, 131071, 131072, 262144, 1048576, 1000003};
  for (size_t i = 0; i < 400; ++i) sweep.push_back(1 + 2 * ((i * 7919 + i * i * 31) % 300000));  // odd sizes up to 600 000
  for (size_t V : sweep)
    for (int mode : {kAuto, kNever, kHalves, kQuarters})
      for (size_t cus : {CU, (size_t)304})
      {
        curV = V;
        curMode = mode;
        EXPECT(validMode(mode));
        const Plan p = splitPlan(V, T, mode, cus, WG);
        const size_t v0 = splitPoint(V, mode, cus, WG);
        EXPECT(p.n >= 1 && p.n <= kMaxParts);
        EXPECT(p.firstSide >= 1 && p.firstSide <= p.n);
        EXPECT(p.cut[0] == 0 && p.cut[p.n] == V);
        for (int k = 0; k < p.n; ++k)
        {
          EXPECT(p.cut[k] < p.cut[k + 1] || (V == 0 && p.n == 1));  // ascending, no part empty (a bank of no voices has one, empty)
          EXPECT(p.cut[k] % kSplitUnit == 0);                      // every cut but the last in whole units
        }
        if (mode == kNever) EXPECT(p.n == 1);
        // one launch exactly where the two-part launch is one, and else the streams divide the voices where it divides them
        EXPECT((p.n == 1) == (v0 == 0));
        if (p.n == 1) EXPECT(p.firstSide == 1);
        if (p.n > 1) EXPECT(p.firstSide < p.n && p.cut[p.firstSide] == v0);
        if (mode == kHalves) EXPECT(v0 == 0 ? is(p, 1, {0, V}) : is(p, 1, {0, v0, V}));
        // at most two kernels a stream
        EXPECT(p.firstSide <= 2 && p.n - p.firstSide <= 2);
        if (mode == kQuarters && v0 != 0)
        {
          // each stream's window in two whenever it has a second unit
          EXPECT((p.firstSide == 2) == (v0 > kSplitUnit));
          EXPECT((p.n - p.firstSide == 2) == (V - v0 > kSplitUnit));
        }
        if (mode == kAuto)
          for (int k = 0; k < p.n && p.n > 1; ++k) EXPECT((p.cut[k + 1] - p.cut[k]) / WG >= cus);  // a workgroup for every CU
      }
  curV = 0;
  curMode = -1;
  EXPECT(!validMode(-1) && !validMode(4));

  // ---- kQuarters: 2 + 2 whenever the windows have the units ----
  EXPECT(is(splitPlan(8448, 3, kQuarters, CU, WG), 2, {0, 2048, 4096, 6144, 8448}));  // a ragged last part of 2304
  EXPECT(is(splitPlan(8192, 3, kQuarters, CU, WG), 2, {0, 2048, 4096, 6144, 8192}));
  EXPECT(is(splitPlan(4096, 3, kQuarters, CU, WG), 1, {0, 2048, 4096}));               // one unit a window: the two halves
  EXPECT(is(splitPlan(4352, 3, kQuarters, CU, WG), 1, {0, 2048, 4096, 4352}));         // only the side stream's window has a second
  EXPECT(is(splitPlan(6144, 3, kQuarters, CU, WG), 1, {0, 2048, 4096, 6144}));
  EXPECT(is(splitPlan(2304, 3, kQuarters, CU, WG), 1, {0, 2048, 2304}));
  EXPECT(is(splitPlan(2048, 3, kQuarters, CU, WG), 1, {0, 2048}));
  EXPECT(is(splitPlan(256, 3, kQuarters, CU, WG), 1, {0, 256}));
  EXPECT(is(splitPlan(262144, 1, kQuarters, CU, WG), 2, {0, 65536, 131072, 196608, 262144}));  // (no gate on short launches here)

  // ---- kAuto: the four-kernel plan where every kernel has a workgroup for every CU, else the halves, else one launch ----
  EXPECT(is(splitPlan(262144, 30, kAuto, CU, WG), 2, {0, 65536, 131072, 196608, 262144}));
  EXPECT(is(splitPlan(131072, 30, kAuto, CU, WG), 1, {0, 65536, 131072}));
  EXPECT(is(splitPlan(131071, 30, kAuto, CU, WG), 1, {0, 131071}));
  EXPECT(is(splitPlan(262144, 30, kAuto, 304, WG), 1, {0, 131072, 262144}));  // a quarter is 256 workgroups
  EXPECT(is(splitPlan(4096, 30, kAuto, CU, WG), 1, {0, 4096}));
  EXPECT(is(splitPlan(1048576, 30, kAuto, CU, WG), 2, {0, 262144, 524288, 786432, 1048576}));

  // ---- the gate on short launches: four kernels only where each has kMinSamplesPerQuarter voice-samples ----
  EXPECT(kMinSamplesPerQuarter == (size_t)65536 * 64 * 16);
  EXPECT(is(splitPlan(262144, 15, kAuto, CU, WG), 1, {0, 131072, 262144}));
  EXPECT(is(splitPlan(262144, 16, kAuto, CU, WG), 2, {0, 65536, 131072, 196608, 262144}));  // 65 536 x 64 x 16: the threshold
  EXPECT(is(splitPlan(262144, 17, kAuto, CU, WG), 2, {0, 65536, 131072, 196608, 262144}));
  EXPECT(is(splitPlan(1048576, 1, kAuto, CU, WG), 1, {0, 524288, 1048576}));  // the real-time workload's free-running leg: 2^24 a quarter
  EXPECT(is(splitPlan(1048576, 3, kAuto, CU, WG), 1, {0, 524288, 1048576}));
  EXPECT(is(splitPlan(1048576, 4, kAuto, CU, WG), 2, {0, 262144, 524288, 786432, 1048576}));
  EXPECT(is(splitPlan(262144, 0, kAuto, CU, WG), 1, {0, 131072, 262144}));    // (no launch is made of T = 0)
  EXPECT(is(splitPlan(262144, ~(size_t)0, kAuto, CU, WG), 2, {0, 65536, 131072, 196608, 262144}));  // nothing wraps

  if (failures == 0) printf("All tests passed\n");
  return failures ? 1 : 0;
}
