// launch_parts.cpp — see launch_parts.hpp
#include "launch_parts.hpp"

namespace mlparts
{
size_t splitPoint(size_t V, int mode, size_t cuCount, size_t lanesPerWorkgroup)
{
  if (mode == kNever || V <= kSplitUnit) return 0;
  size_t v0 = (V / 2) / kSplitUnit * kSplitUnit;
  if (v0 == 0) v0 = kSplitUnit;
  if (mode == kHalves) return v0;
  // automatic: the smaller part still puts at least one workgroup on every CU
  const size_t smaller = v0 < V - v0 ? v0 : V - v0;
  return smaller / lanesPerWorkgroup >= cuCount ? v0 : 0;
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
