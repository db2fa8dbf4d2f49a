// The shape of the mixdown tree (madronalib_amd/csrc/mixdown_tree.hpp) without a device: built by g++ from the header alone, with
// -fsanitize=address,undefined, by tests/test_mixdown_tree_cpu.py. The region's size; the pass lists - that they chain to one row,
// never read the part they write, fit the parts, end in `out`, and name the kernels the launch loops named before the tree was a
// value (those loops restated below as the expectation); a shard's level and rows.
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "../../madronalib_amd/csrc/mixdown_tree.hpp"

using namespace mlmix;

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

// One launch of the loops as they were: which kernel, over how many rows, from which buffer into which ('a': the region's start,
// 'b': a + groups rows, 'o': out)
struct Launch
{
  Kernel kernel;
  size_t rows, rowsOut;
  char src, dst;
};
static bool operator==(const Launch& x, const Launch& y) { return x.kernel == y.kernel && x.rows == y.rows && x.rowsOut == y.rowsOut && x.src == y.src && x.dst == y.dst; }

// mlgpu_launch_mixdown_rows as it stood, a launch written down instead of made
static std::vector<Launch> loopToTheEnd(size_t groups)
{
  std::vector<Launch> made;
  char a = 'a', b = 'b';
  size_t rows = groups;
  do
  {
    if (rows <= 4096)
    {
      made.push_back({kLast2, rows, 1, a, 'o'});
      break;
    }
    const size_t rowsOut = (rows + 63) / 64;
    made.push_back({kRows64, rows, rowsOut, a, rowsOut == 1 ? 'o' : b});
    char t = a;
    a = b;
    b = t;
    rows = rowsOut;
  } while (rows > 1);
  return made;
}
// mlgpu_launch_mixdown_rows_partial as it stood
static std::vector<Launch> loopPartial(size_t groups, int reductions)
{
  std::vector<Launch> made;
  char a = 'a', b = 'b';
  size_t rows = groups;
  if (reductions == 0)
  {
    made.push_back({kCopy, groups, groups, 'a', 'o'});
    return made;
  }
  for (int r = 0; r < reductions; ++r)
  {
    const size_t rowsOut = (rows + 63) / 64;
    made.push_back({kRows64, rows, rowsOut, a, r + 1 == reductions ? 'o' : b});
    char t = a;
    a = b;
    b = t;
    rows = rowsOut;
  }
  return made;
}

static char bufferOf(Part p) { return p == kFirst ? 'a' : (p == kSecond ? 'b' : 'o'); }

// what every pass list must satisfy, and that it is `want` launch for launch
static void checkPasses(size_t groups, const Passes& ps, const std::vector<Launch>& want, size_t lastRows)
{
  EXPECT(ps.n >= 1 && ps.n <= kMaxPasses);
  EXPECT((size_t)ps.n == want.size());
  size_t rows = groups;
  Part at = kFirst;
  int i = 0;
  for (const Pass& p : ps)
  {
    EXPECT(p.rowsIn == rows && p.from == at);  // chained: reads what the pass before wrote, where it wrote it
    EXPECT(p.from != kOut && p.from != p.to);  // no pass reads the part it writes
    if (p.to == kFirst) EXPECT(p.rowsOut <= groups);
    if (p.to == kSecond) EXPECT(p.rowsOut <= groupsOf(groups));
    if (p.kernel == kRows64) EXPECT(p.rowsOut == (p.rowsIn + 63) / 64);
    if (p.kernel == kLast2) EXPECT(p.rowsIn <= 4096 && p.rowsOut == 1);
    if (p.kernel == kCopy) EXPECT(p.rowsOut == p.rowsIn);
    EXPECT((i + 1 == ps.n) == (p.to == kOut));  // the last pass, and only that, writes `out`
    if ((size_t)i < want.size()) EXPECT((Launch{p.kernel, p.rowsIn, p.rowsOut, bufferOf(p.from), bufferOf(p.to)} == want[(size_t)i]));
    rows = p.rowsOut;
    at = p.to;
    ++i;
  }
  EXPECT(rows == lastRows && at == kOut);
}

int main()
{
  const size_t cube = (size_t)64 * 64 * 64;
  // ---- the region, and the passes to the end ----
  for (size_t groups : {(size_t)1, (size_t)2, (size_t)63, (size_t)64, (size_t)65, (size_t)4095, (size_t)4096, (size_t)4097, (size_t)4162, (size_t)262144,
                        (size_t)262145, cube + 1})
    for (size_t T : {(size_t)1, (size_t)3})
    {
      EXPECT(regionFloatsOfGroups(groups, T) == (groups + (groups + 63) / 64) * T * 64);
      EXPECT(secondPartFloats(groups, T) == groups * T * 64);
      for (size_t V : {groups * 64, groups * 64 - 63})  // whole groups, and one voice in the last
      {
        EXPECT(groupsOf(V) == groups);
        EXPECT(regionFloats(V, T) == regionFloatsOfGroups(groups, T));
      }
      checkPasses(groups, passes(groups), loopToTheEnd(groups), 1);
      checkPasses(groups, passes(groups, kToTheEnd), loopToTheEnd(groups), 1);
    }
  EXPECT(passes(1).n == 1 && passes(4096).n == 1 && passes(4097).n == 2 && passes(262144).n == 2 && passes(262145).n == 3 && passes(cube + 1).n == 3);
  EXPECT(passes(4162).pass[0].to == kSecond && passes(4162).pass[0].rowsOut == 66 && passes(4162).pass[1].kernel == kLast2);
  EXPECT(passes(262145).pass[1].to == kFirst && passes(262145).pass[1].rowsOut == 65);
  EXPECT(groupsOf(0) == 0 && regionFloats(0, 5) == 0 && regionFloats(777, 2) == (13 + 1) * 2 * 64);

  // ---- n exact reductions: never the last-two kernel; 0 is a copy ----
  for (int n = 0; n <= 2; ++n)
  {
    const size_t unit = n == 0 ? 1 : (n == 1 ? 64 : 4096);
    for (size_t k : {(size_t)1, (size_t)2, (size_t)63, (size_t)64, (size_t)65, (size_t)72, (size_t)4097})
    {
      const size_t groups = k * unit;
      const Passes ps = passes(groups, n);
      checkPasses(groups, ps, loopPartial(groups, n), k);
      EXPECT(ps.n == (n == 0 ? 1 : n));
      for (const Pass& p : ps) EXPECT(p.kernel == (n == 0 ? kCopy : kRows64));
    }
  }

  // ---- a shard's level and rows ----
  struct
  {
    size_t V;
    int level;
    size_t rows;
  } const shards[] = {{0, 0, 0},           {63, 0, 0},          {64, 1, 1},
                      {100, 0, 0},         {4096, 2, 1},        {8192, 2, 2},
                      {64 * 72, 1, 72},    {64 * 64 * 6, 2, 6}, {262144, 3, 1}};
  for (const auto& s : shards)
  {
    EXPECT(shardLevel(s.V) == s.level);
    EXPECT(shardRows(s.V) == s.rows);
    // what a shard hands over is what `level - 1` exact reductions leave of its group sums
    if (s.level > 0)
    {
      const Passes ps = passes(groupsOf(s.V), s.level - 1);
      EXPECT(ps.pass[ps.n - 1].rowsOut == s.rows);
    }
  }

  if (failures == 0) printf("All tests passed\n");
  return failures == 0 ? 0 : 1;
}
