// launch_parts.cpp — see launch_parts.hpp
#include "launch_parts.hpp"

namespace mlparts
{
size_t splitPoint(size_t V, int mode, size_t cuCount, size_t lanesPerWorkgroup)
{
  if (mode == kNever || V <= kSplitUnit) return 0;
  size_t v0 = (V / 2) / kSplitUnit * kSplitUnit;
  if (v0 == 0) v0 = kSplitUnit;
  if (mode == kHalves || mode == kQuarters) return v0;
  // automatic: the smaller part still puts at least one workgroup on every CU
  const size_t smaller = v0 < V - v0 ? v0 : V - v0;
  return smaller / lanesPerWorkgroup >= cuCount ? v0 : 0;
}

namespace
{
// where the window [lo, hi) of one stream is cut once more, or 0 for "not at all"
size_t cutWindow(size_t lo, size_t hi, size_t T, int mode, size_t cuCount, size_t lanesPerWorkgroup)
{
  const size_t W = hi - lo;
  if (mode == kHalves || W <= kSplitUnit) return 0;
  size_t w0 = (W / 2) / kSplitUnit * kSplitUnit;
  if (w0 == 0) w0 = kSplitUnit;
  if (mode == kQuarters) return lo + w0;
  const size_t smaller = w0 < W - w0 ? w0 : W - w0;
  if (smaller / lanesPerWorkgroup < cuCount) return 0;
  // (smaller * 64 * T >= kMinSamplesPerQuarter, with no product or sum that could wrap)
  constexpr size_t vectors = kMinSamplesPerQuarter / 64;
  if (T == 0 || smaller < vectors / T + (vectors % T != 0)) return 0;
  return lo + w0;
}
}  // namespace

Plan splitPlan(size_t V, size_t T, int mode, size_t cuCount, size_t lanesPerWorkgroup)
{
  Plan p{};
  const size_t v0 = splitPoint(V, mode, cuCount, lanesPerWorkgroup);
  if (v0 == 0)
  {
    p.cut[1] = V;
    p.n = p.firstSide = 1;
    return p;
  }
  int n = 0;
  p.cut[n++] = 0;
  if (const size_t c = cutWindow(0, v0, T, mode, cuCount, lanesPerWorkgroup)) p.cut[n++] = c;
  p.firstSide = n;
  p.cut[n++] = v0;
  if (const size_t c = cutWindow(v0, V, T, mode, cuCount, lanesPerWorkgroup)) p.cut[n++] = c;
  p.cut[n] = V;
  p.n = n;
  return p;
}

bool Pending::admits(const void* owner, const Output& out) const
{
  if (!any() || owner != owner_) return false;
  bool known = false;
  for (size_t i = 0; i < n_; ++i)
  {
    if (sameOutput(out_[i], out))
      known = true;
    else if (!disjoint(out_[i], out))
      return false;
  }
  return known || n_ < kMaxPendingOutputs;
}

void Pending::launched(const void* owner, const Output& out)
{
  if (owner != owner_)
  {
    owner_ = owner;
    n_ = 0;
  }
  for (size_t i = 0; i < n_; ++i)
    if (sameOutput(out_[i], out)) return;
  if (n_ < kMaxPendingOutputs) out_[n_++] = out;
}
}  // namespace mlparts
