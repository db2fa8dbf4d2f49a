// Which kernels of a bank launch in parts are "at most a workgroup per CU" (mlparts::atMostAWorkgroupPerCu: the parts that get
// MLGPU_KFLAG_LONE_WAVEFRONTS from mlgpu_bank_process) - plain host C++, no device. Built and run by tests/test_launch_parts_lone_cpu.py
// under the address and undefined-behaviour sanitizers.
#include <cstdio>

#include "../../madronalib_amd/csrc/launch_parts.hpp"

using namespace mlparts;

static int failures = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); ++failures; } } while (0)

// how many of the plan's parts qualify
static int loneParts(const Plan& p, size_t cuCount)
{
  int n = 0;
  for (int i = 0; i < p.n; ++i) n += atMostAWorkgroupPerCu(p.cut[i + 1] - p.cut[i], cuCount, kLanesPerWorkgroup) ? 1 : 0;
  return n;
}

int main()
{
  constexpr size_t W = kLanesPerWorkgroup, CU = 256;
  // the boundary: cuCount workgroups qualify, a lane more is one workgroup more and does not; a ragged last workgroup counts whole
  CHECK(atMostAWorkgroupPerCu(CU * W, CU, W));
  CHECK(!atMostAWorkgroupPerCu(CU * W + 1, CU, W));
  CHECK(atMostAWorkgroupPerCu(CU * W - 1, CU, W));
  CHECK(atMostAWorkgroupPerCu((CU - 1) * W + 1, CU, W));
  CHECK(atMostAWorkgroupPerCu(1, CU, W) && atMostAWorkgroupPerCu(0, CU, W));
  CHECK(atMostAWorkgroupPerCu(W, 1, W) && !atMostAWorkgroupPerCu(W + 1, 1, W));
  CHECK(!atMostAWorkgroupPerCu(~(size_t)0, CU, W));  // (no sum that could wrap)

  // the headline launch: 262 144 voices x 30 DSPVectors on 256 CUs, by size - four kernels of 256 workgroups, every one of them
  const Plan head = splitPlan(262144, 30, kAuto, CU, W);
  CHECK(head.n == 4 && loneParts(head, CU) == 4);
  // ... the same four kernels on a chip of 255 CUs are a workgroup too many
  CHECK(loneParts(head, CU - 1) == 0);
  // the rt workload's block: 2^20 voices x 1 DSPVector - two kernels of 2 048 workgroups, neither
  const Plan rt = splitPlan((size_t)1 << 20, 1, kAuto, CU, W);
  CHECK(rt.n == 2 && loneParts(rt, CU) == 0);
  // 131 072 voices x 30: halves of 256 workgroups, both
  const Plan half = splitPlan(131072, 30, kAuto, CU, W);
  CHECK(half.n == 2 && loneParts(half, CU) == 2);
  // the test modes at 8 192 voices: two kernels of 16 workgroups, four of 8 - all; and 8 448 with its ragged last part
  const Plan h = splitPlan(8192, 3, kHalves, CU, W), q = splitPlan(8192, 3, kQuarters, CU, W), r = splitPlan(8448, 3, kQuarters, CU, W);
  CHECK(h.n == 2 && loneParts(h, CU) == 2);
  CHECK(q.n == 4 && loneParts(q, CU) == 4);
  CHECK(r.n == 4 && loneParts(r, CU) == 4);
  // ... and on a chip of 8 CUs only the quarters (8 workgroups each; the ragged one has 9)
  CHECK(loneParts(h, 8) == 0 && loneParts(q, 8) == 4 && loneParts(r, 8) == 3);

  if (failures == 0) printf("All tests passed\n");
  return failures == 0 ? 0 : 1;
}
