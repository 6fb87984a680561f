// Host-side plan of the converting lattice copy (igg/select.hpp).
#include <algorithm>

#include "igg/common.hpp"
#include "igg/select.hpp"

namespace igg {

SelectPlan plan_select(const int64_t c[3], const int64_t S[3], const int64_t T[3]) {
  SelectPlan p;
  p.total = 1;
  double total = 1.0, span = 0.0;
  for (int d = 0; d < 3; ++d) {
    if (c[d] < 0) fail("plan_select: negative count in dimension ", d);
    if (S[d] < 0 || T[d] < 0) fail("plan_select: negative stride in dimension ", d);
    if (c[d] > 0x7fffffffLL) fail("plan_select: count ", c[d], " too large in dimension ", d);
    total *= static_cast<double>(c[d]);
    span += static_cast<double>(c[d]) * static_cast<double>(std::max(S[d], T[d]));
  }
  // (far beyond any memory: keeps every product below in 64 bits)
  if (total > 0x1p60 || span > 0x1p60) fail("plan_select: box too large");
  for (int d = 0; d < 3; ++d) p.total *= c[d];
  p.path = (S[2] == 1 && T[2] == 1) ? SelectPath::rows : SelectPath::element;
  if (p.total == 0) return p;
  p.rows = c[0] * c[1];
  for (int d = 0; d < 3; ++d) {
    p.src_span += (c[d] - 1) * S[d];
    p.dst_span += (c[d] - 1) * T[d];
  }
  // (the 32-bit form also counts elements, rows and its grid stride in 32 bits)
  const int64_t lim = 0x7fffffffLL - int64_t{SELECT_MAX_BLOCKS} * SELECT_BLOCK;
  p.index_bits = (p.src_span > lim || p.dst_span > lim || p.total > lim) ? 64 : 32;
  const int64_t per_block = p.path == SelectPath::rows ? SELECT_BLOCK / 64 : SELECT_BLOCK;
  const int64_t work = p.path == SelectPath::rows ? p.rows : p.total;
  p.blocks = std::min<int64_t>((work + per_block - 1) / per_block, SELECT_MAX_BLOCKS);
  return p;
}

}  // namespace igg
