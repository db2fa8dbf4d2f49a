// mixdown_tree.hpp — the SHAPE of the mixdown's 64-ary tree and of its scratch ("The mixdown tree"): what
// mlgpu_mixdown, the summing forms of banks and graphs, the shard calls and mlgpu_mixdown_finish go by. Plain C++ that knows nothing
// of streams or kernels, built and tested without any HIP header; ops.hip walks the passes, capi.hip and graph.hip size the scratch.
// The voices are summed 64 at a time, in voice order: 64 voices make one ROW (a group sum, 64 floats per DSPVector), 64 rows make
// one row of the next level, until one row is left. A tree's scratch REGION has two parts: the first holds the rows of group sums
// (written by the first stage, or by a voice kernel that sums its wavefronts itself), the second the rows of the first pass over
// them. Later passes alternate between the parts - each level fits where the level before last was - and the last one writes
// the caller's `out`.
#pragma once
#include <stddef.h>

namespace mlmix
{
constexpr size_t kFan = 64;              // voices per group, rows per pass output row
constexpr size_t kRowFloats = 64;        // floats of one row per DSPVector
constexpr size_t kLastTwoRows = 4096;    // up to here the last two levels run in one kernel (kFan * kFan rows -> 1)

// the groups of V voices; also the rows a 64-to-1 pass makes of `n`
inline size_t groupsOf(size_t n) { return (n + kFan - 1) / kFan; }
// float offset of a region's second part, for a tree of `groups` rows over T DSPVectors
inline size_t secondPartFloats(size_t groups, size_t T) { return groups * T * kRowFloats; }
// floats of one tree's region: the group sums, and their sums 64 at a time
inline size_t regionFloatsOfGroups(size_t groups, size_t T) { return (groups + groupsOf(groups)) * T * kRowFloats; }
inline size_t regionFloats(size_t V, size_t T) { return regionFloatsOfGroups(groupsOf(V), T); }

// ---- a voice bank split over several engines: every shard hands over the rows of the tree at the highest level its voice count
// is whole at (mlgpu_mixdown_shard), and the host finishes the same tree over all shards' rows (mlgpu_mixdown_finish) ----
// 0: not a whole number of groups, no shard form. Level L: the rows after L - 1 exact 64-to-1 passes over the group sums.
inline int shardLevel(size_t voicesPerShard)
{
  if (voicesPerShard == 0 || voicesPerShard % kFan) return 0;
  int level = 1;
  for (size_t rows = voicesPerShard / kFan; rows % kFan == 0; rows /= kFan) ++level;
  return level;
}
inline size_t shardRows(size_t voicesPerShard)
{
  const int level = shardLevel(voicesPerShard);
  if (level == 0) return 0;
  size_t rows = voicesPerShard / kFan;
  for (int l = 1; l < level; ++l) rows /= kFan;
  return rows;
}

// ---- the passes over a region, after its first part has been written ----
enum Part
{
  kFirst,   // the region's first part: `groups` rows
  kSecond,  // its second part: groupsOf(groups) rows
  kOut      // the caller's output
};
enum Kernel
{
  kRows64,  // mixdown_rows64_kernel: 64 rows -> 1
  kLast2,   // mixdown_rows_last2_kernel: up to kLastTwoRows rows -> 1, two levels in one kernel
  kCopy     // no reduction: the rows as they are
};
struct Pass
{
  size_t rowsIn, rowsOut;
  Part from, to;
  Kernel kernel;
};
constexpr int kToTheEnd = -1;  // `reductions`: until one row is left
constexpr int kMaxPasses = 11;  // 64^11 > SIZE_MAX

struct Passes
{
  int n{0};
  Pass pass[kMaxPasses];
  const Pass* begin() const { return pass; }
  const Pass* end() const { return pass + n; }
};

// The passes over `groups` rows in a region's first part.
//   kToTheEnd       kRows64 passes while more than kLastTwoRows rows are left, then one kLast2 into `out`
//   reductions n    exactly n kRows64 passes, the last one into `out` (each exact where groups is a multiple of 64^n: what a shard
//                   of level n + 1 hands over); 0: a copy of the group sums
inline Passes passes(size_t groups, int reductions = kToTheEnd)
{
  Passes p;
  size_t rows = groups;
  Part from = kFirst;
  auto add = [&](size_t rowsOut, Part to, Kernel k) {
    p.pass[p.n++] = Pass{rows, rowsOut, from, to, k};
    rows = rowsOut;
    from = to;
  };
  const auto other = [&] { return from == kFirst ? kSecond : kFirst; };
  if (reductions == 0) add(rows, kOut, kCopy);
  else if (reductions == kToTheEnd)
  {
    while (rows > kLastTwoRows) add(groupsOf(rows), other(), kRows64);
    add(1, kOut, kLast2);
  }
  else
    for (int r = 0; r < reductions && p.n < kMaxPasses; ++r) add(groupsOf(rows), r + 1 == reductions ? kOut : other(), kRows64);
  return p;
}
}  // namespace mlmix
