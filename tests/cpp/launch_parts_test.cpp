// The bookkeeping of launches that go out in two parts (madronalib_amd/csrc/launch_parts.cpp) without a device: built by g++ from
// that one file, with -fsanitize=address,undefined, by tests/test_launch_parts_cpu.py. Where a bank is cut and under which mode;
// which launch may follow pending ones with no join - the pending bank's, into a pending output exactly or one apart from all of them -
// and which may not: another bank, an output that overlaps a pending one at another address, size, layout or length, one more
// output than the engine remembers.
#include <cstdio>
#include <initializer_list>

#include "../../madronalib_amd/csrc/launch_parts.hpp"

using namespace mlparts;

static int failures = 0;
#define EXPECT(cond)                                          \
  do                                                          \
  {                                                           \
    if (!(cond))                                              \
    {                                                         \
      ++failures;                                             \
      printf("FAILED line %d: %s\n", __LINE__, #cond);        \
    }                                                         \
  } while (0)

int main()
{
  // ---- where a bank is cut ----
  const size_t CU = 256, WG = 256;
  EXPECT(splitPoint(256, kHalves, CU, WG) == 0);    // one workgroup
  EXPECT(splitPoint(2048, kHalves, CU, WG) == 0);   // one unit: no second part
  EXPECT(splitPoint(2049, kHalves, CU, WG) == 2048);
  EXPECT(splitPoint(2304, kHalves, CU, WG) == 2048);  // a ragged second part of 256
  EXPECT(splitPoint(4096, kHalves, CU, WG) == 2048);
  EXPECT(splitPoint(6144, kHalves, CU, WG) == 2048);  // whole units of V / 2
  EXPECT(splitPoint(262144, kHalves, CU, WG) == 131072);
  for (size_t V : {2049u, 2304u, 4096u, 5000u, 65536u, 131071u, 131072u, 262144u, 1048576u, 1000003u})
  {
    const size_t v0 = splitPoint(V, kHalves, CU, WG);
    EXPECT(v0 > 0 && v0 < V && v0 % kSplitUnit == 0);
    EXPECT(splitPoint(V, kNever, CU, WG) == 0);
    const size_t a = splitPoint(V, kAuto, CU, WG);
    EXPECT(a == 0 || a == v0);
    // automatic: only where the smaller part still has a workgroup for every CU
    const size_t smaller = v0 < V - v0 ? v0 : V - v0;
    EXPECT((a != 0) == (smaller / WG >= CU));
  }
  EXPECT(splitPoint(4096, kAuto, CU, WG) == 0);
  EXPECT(splitPoint(131071, kAuto, CU, WG) == 0);
  EXPECT(splitPoint(131072, kAuto, CU, WG) == 65536);
  EXPECT(splitPoint(262144, kAuto, CU, WG) == 131072);
  EXPECT(splitPoint(262144, kAuto, 304, WG) == 131072);  // (a device with more CUs than the MI355X: 512 workgroups a part)
  EXPECT(splitPoint(131072, kAuto, 304, WG) == 0);
  EXPECT(splitPoint(0, kHalves, CU, WG) == 0);

  // ---- what may follow with no join ----
  int bankX = 0, bankY = 0;
  const Output A{0x10000, 0x4000, 0, 3}, B{0x20000, 0x4000, 0, 3};
  Pending p;
  EXPECT(!p.any() && p.outputs() == 0);
  EXPECT(!p.admits(&bankX, A));  // nothing pending: there is a fork to make
  p.launched(&bankX, A);
  EXPECT(p.any() && p.owner() == &bankX && p.outputs() == 1);
  EXPECT(p.admits(&bankX, A));   // the same output again
  EXPECT(p.admits(&bankX, B));   // a ring of two
  EXPECT(!p.admits(&bankY, A));  // another bank
  EXPECT(!p.admits(&bankY, B));
  p.launched(&bankX, B);
  p.launched(&bankX, A);
  EXPECT(p.outputs() == 2);
  EXPECT(p.admits(&bankX, A) && p.admits(&bankX, B));
  // overlapping a pending output at another address, from below and from above, by one byte
  EXPECT(!p.admits(&bankX, Output{0x10000 + 16, 0x4000, 0, 3}));
  EXPECT(!p.admits(&bankX, Output{0x10000 - 0x4000 + 1, 0x4000, 0, 3}));
  EXPECT(!p.admits(&bankX, Output{0x13FFF, 0x4000, 0, 3}));
  EXPECT(p.admits(&bankX, Output{0x14000, 0x4000, 0, 3}));           // touching, apart
  EXPECT(p.admits(&bankX, Output{0x10000 - 0x4000, 0x4000, 0, 3}));
  EXPECT(!p.admits(&bankX, Output{0x0, 0x100000, 0, 3}));             // around both
  // the same address in another layout, over another length, of another size
  EXPECT(!p.admits(&bankX, Output{0x10000, 0x4000, 1, 3}));
  EXPECT(!p.admits(&bankX, Output{0x10000, 0x4000, 0, 2}));
  EXPECT(!p.admits(&bankX, Output{0x10000, 0x2000, 0, 3}));
  // no more outputs than the engine remembers: the next new one joins, a known one does not
  for (size_t i = 2; i < kMaxPendingOutputs; ++i)
  {
    const Output o{0x100000 + 0x4000 * i, 0x4000, 0, 3};
    EXPECT(p.admits(&bankX, o));
    p.launched(&bankX, o);
  }
  EXPECT(p.outputs() == kMaxPendingOutputs);
  EXPECT(!p.admits(&bankX, Output{0x900000, 0x4000, 0, 3}));
  EXPECT(p.admits(&bankX, A));
  p.launched(&bankX, Output{0x900000, 0x4000, 0, 3});  // (never after a refusal; were it to happen, nothing is overrun)
  EXPECT(p.outputs() == kMaxPendingOutputs);
  p.joined();
  EXPECT(!p.any() && p.outputs() == 0 && !p.admits(&bankX, A));
  // a launch of another bank after a join starts over
  p.launched(&bankY, B);
  EXPECT(p.owner() == &bankY && p.outputs() == 1 && p.admits(&bankY, B) && p.admits(&bankY, A) && !p.admits(&bankX, B));
  // an output at the top of the address space does not wrap
  p.joined();
  p.launched(&bankX, Output{~(uintptr_t)0 - 0x3FFF, 0x4000, 0, 3});
  EXPECT(p.admits(&bankX, A));
  EXPECT(!p.admits(&bankX, Output{~(uintptr_t)0 - 0xFFF, 0x1000, 0, 3}));

  if (failures == 0) printf("All tests passed\n");
  return failures ? 1 : 0;
}
